"""Random Fourier features (pmh_rff_*, csrc/rff.hip): z(x) = sqrt(2 / D) cos(Omega'x + beta) with the columns of Omega drawn from a shift-invariant kernel's
spectral density, so that z(x) . z(x') ~ k(x, x') (Rahimi and Recht, 2007).  A linear SVM, SVMMulticlass or SVR on Z = transform(X) is an approximate kernel
machine, and every tool of the linear front ends -- subsets, cross-validation, grid search, warm starts, penalties, Platt scaling -- works on it unchanged:

    fmap = RFFMap(ctx, d=X.shape[1], D=256, gamma=0.5)
    Z = fmap.transform(X)                       # DeviceSamples: computed and kept on the device
    svm = SVM(ctx, C=10).fit(Z, y)
    svm.predict(fmap.transform(Xt))          # stores the (n, D) features of the test samples, or
    svm.predict(fmap.lazy(Xt))               # MappedSamples: scores them from the map's registers, no (n, D) array (pmh_rffdots, csrc/rff_score.hip)

    rbf:        k(x, x') = exp(-gamma |x - x'|_2^2),  Omega = sqrt(2 gamma) N(0, 1)
    laplacian:  k(x, x') = exp(-gamma |x - x'|_1),    Omega = gamma standard Cauchy

The draw is the host's (numpy.random.default_rng(seed)); the map itself is one HIP kernel on the fp64 matrix cores; there is no CPU fallback.

lazy(X) is accepted wherever a front end takes TEST samples (decision_function, predict, predict_both, predict_proba, calibrate, test) and refused, with a
TypeError, where it takes training samples.  The features are fp64 there and never rounded: a handle trained on float32 features (sample_dtype = float32) scores
lazy features that were not rounded to float32.  The classes go through the kernel four at a time and the features are computed again for every four: nothing
chooses between the lazy and the stored path for the caller.  dots(X, W) is the raw entry: the features' dot products with the rows of any W.

Not here: sparse X, gamma = "scale", training on lazy features.  Polynomial kernels and data-dependent (Nystroem) features: NystroemMap, nystroem.py."""
import ctypes as ct
import math

import numpy as np

from ._lib import check
from .core import MappedSamples, Vec
from .featuremap import TYPE_CODES, FeatureMap

KERNELS = ("rbf", "laplacian")
# pmh_rff_info: the tiling of the map's kernel, then (classes_per_chunk, dots_lds_bytes) of the scoring kernel behind lazy() and dots()
INFO = ("rows_per_workgroup", "rows_per_wave", "column_tile", "k_block", "lds_bytes", "waves_per_workgroup", "classes_per_chunk", "dots_lds_bytes")


def draw(d, D=256, gamma=1.0, kernel="rbf", seed=0):
    """(omega (d, D), beta (D,), scale) of the map for `kernel`: one generator default_rng(seed), Omega first, then beta = 2 pi U[0, 1); scale = sqrt(2 / D).
    Host only."""
    d, D, gamma = int(d), int(D), float(gamma)
    if kernel not in KERNELS:
        raise ValueError("RFFMap: kernel must be one of %s, not %r" % (", ".join(KERNELS), kernel))
    if d < 1 or D < 1:
        raise ValueError("RFFMap: d = %d, D = %d, both must be at least 1" % (d, D))
    if not (gamma > 0.0 and math.isfinite(gamma)):
        raise ValueError("RFFMap: gamma = %r, must be positive and finite" % gamma)
    rng = np.random.default_rng(seed)
    omega = math.sqrt(2.0 * gamma) * rng.standard_normal((d, D)) if kernel == "rbf" else gamma * rng.standard_cauchy((d, D))
    beta = 2.0 * math.pi * rng.random(D)
    return omega, beta, math.sqrt(2.0 / D)


class RFFMap(FeatureMap):
    ENTRY, INFO = "pmh_rff", INFO

    def __init__(self, ctx, d, D=256, gamma=1.0, kernel="rbf", seed=0):
        self._create(ctx, *draw(d, D, gamma, kernel, seed))
        self.gamma, self.kernel, self.seed = float(gamma), kernel, seed

    @classmethod
    def from_arrays(cls, ctx, omega, beta, scale):
        """A saved map: omega (d, D), beta (D,) or None (all 0), scale."""
        f = cls.__new__(cls)
        f._create(ctx, omega, beta, scale)
        f.gamma = f.kernel = f.seed = None
        return f

    def _create(self, ctx, omega, beta, scale):
        omega = np.ascontiguousarray(omega, dtype=np.float64)
        if omega.ndim != 2:
            raise ValueError("RFFMap: omega must be (d, D)")
        self.ctx, self.L, self.h = ctx, ctx.L, None
        self.d, self.D = omega.shape
        if beta is not None:
            beta = np.ascontiguousarray(beta, dtype=np.float64).ravel()
            if beta.size != self.D:
                raise ValueError("RFFMap: beta must have %d entries" % self.D)
        od = Vec.from_numpy(ctx, omega.ravel())
        bd = Vec.from_numpy(ctx, beta) if beta is not None else None
        try:
            h = ct.c_void_p()
            check(self.L.pmh_rff_create(ctx.h, self.d, self.D, od.p, bd.p if bd is not None else None, float(scale), ct.byref(h)))
            self.h = h
        finally:
            od.free()
            if bd is not None:
                bd.free()

    def _get(self, what):
        self._need()
        omega, beta, scale = np.empty((self.d, self.D)), np.empty(self.D), ct.c_double()
        check(self.L.pmh_rff_get(self.h, None, None, omega.ctypes.data_as(ct.c_void_p) if what == 0 else None, beta.ctypes.data_as(ct.c_void_p) if what == 1 else None,
                                 ct.byref(scale)))
        return (omega, beta, scale.value)[what]

    omega = property(lambda self: self._get(0))
    beta = property(lambda self: self._get(1))
    scale = property(lambda self: self._get(2))

    def transform(self, X, out_dtype=np.float64):
        """Z = scale cos(X Omega + beta) as DeviceSamples (n, D) of out_dtype (float64 or float32: rounded once, at the store), computed and left on the device
        (pmh_rff_apply).  X: an (n, d) ndarray -- float32 goes up and is read as float32, anything else as float64 -- or a DeviceSamples; all arithmetic is fp64."""
        odt = self._out_dtype(out_dtype)
        return self._run(X, "D", odt, lambda src, Z: self.L.pmh_rff_apply(self.h, src.n, src.p, TYPE_CODES[src.dtype], Z.p, TYPE_CODES[odt]))

    def arguments(self, X):
        """tests: T = X Omega + beta as an (n, D) float64 host array, from the SAME kernel with the identity in place of scale cos(.) (pmh_rff_test_args)."""
        return self._run_host(X, "D", lambda src, T: self.L.pmh_rff_test_args(self.h, src.n, src.p, TYPE_CODES[src.dtype], T.p))

    def lazy(self, X):
        """X seen through the map as MappedSamples (n, D), for the scoring calls of SVM, SVMMulticlass and SVR: nothing is computed until a handle scores it, and
        then no (n, D) array is made.  X as in transform; an ndarray is uploaded here and freed by the result's free(), a DeviceSamples stays the caller's."""
        self._need()
        src, made = self._source(X)
        return MappedSamples(self, src, made)

    def _dots(self, entry, X, W, ldw):
        W = np.asarray(W, dtype=np.float64)
        W = np.ascontiguousarray(W.reshape(1, -1) if W.ndim == 1 else W)
        if W.ndim != 2 or W.shape[1] != self.D:
            raise ValueError("RFFMap.dots: W must be (K, %d) or (%d,)" % (self.D, self.D))
        K, ldw = W.shape[0], self.D if ldw is None else int(ldw)
        Wp = W
        if ldw > self.D:  # (rows ldw apart, the gaps NaN: nothing of them may be read)
            Wp = np.full((K, ldw), np.nan)
            Wp[:, :self.D] = W
        src, made = self._source(X)
        wd = out = None
        try:
            self._need()
            wd = Vec.from_numpy(self.ctx, Wp.ravel()[:(K - 1) * ldw + self.D] if K else Wp.ravel())
            out = Vec(self.ctx, max(src.n * K, 1), zero=False)
            check(entry(self.h, src.n, src.p, TYPE_CODES[src.dtype], K, wd.p, ldw, out.p))
            return out.to_numpy()[:src.n * K].reshape(src.n, K)
        finally:
            for v in (wd, out):
                if v is not None:
                    v.free()
            if made:
                src.free()

    def dots(self, X, W, ldw=None):
        """(n, K): transform(X) @ W.T without the features being stored (pmh_rffdots); W (K, D), or (D,) for K = 1; no bias.  ldw: the row stride W is given
        to the device with (None: D)."""
        return self._dots(self.L.pmh_rffdots, X, W, ldw)

    def dot_arguments(self, X, W, ldw=None):
        """tests: arguments(X) @ W.T from the SAME kernel with the identity in place of scale cos(.) (pmh_rffdots_test_args)."""
        return self._dots(self.L.pmh_rffdots_test_args, X, W, ldw)
