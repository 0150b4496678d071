"""Random Fourier features (pmh_rff_*, csrc/rff.hip): z(x) = sqrt(2 / D) cos(Omega'x + beta) with the columns of Omega drawn from a shift-invariant kernel's
spectral density, so that z(x) . z(x') ~ k(x, x') (Rahimi and Recht, 2007).  A linear SVM, SVMMulticlass or SVR on Z = transform(X) is an approximate kernel
machine, and every tool of the linear front ends -- subsets, cross-validation, grid search, warm starts, penalties, Platt scaling -- works on it unchanged:

    fmap = RFFMap(ctx, d=X.shape[1], D=256, gamma=0.5)
    Z = fmap.transform(X)                       # DeviceSamples: computed and kept on the device
    svm = SVM(ctx, C=10).fit(Z, y)
    svm.predict(fmap.transform(Xt))

    rbf:        k(x, x') = exp(-gamma |x - x'|_2^2),  Omega = sqrt(2 gamma) N(0, 1)
    laplacian:  k(x, x') = exp(-gamma |x - x'|_1),    Omega = gamma standard Cauchy

The draw is the host's (numpy.random.default_rng(seed)); the map itself is one HIP kernel on the fp64 matrix cores; there is no CPU fallback.  Not here: sparse
X, polynomial kernels, gamma = "scale", Nystroem features."""
import ctypes as ct
import math

import numpy as np

from ._lib import check
from .core import DeviceSamples, Vec
from .mat import is_sparse

KERNELS = ("rbf", "laplacian")
TYPE_CODES = {np.dtype(np.float64): 0, np.dtype(np.float32): 1}  # PMH_F64, PMH_F32
INFO = ("rows_per_workgroup", "rows_per_wave", "column_tile", "k_block", "lds_bytes", "waves_per_workgroup")


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


class RFFMap:
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

    def _need(self):
        if self.h is None:
            raise RuntimeError("RFFMap: the map has been destroyed")

    def _get(self, what):
        self._need()
        omega, beta, scale = np.empty((self.d, self.D)), np.empty(self.D), ct.c_double()
        check(self.L.pmh_rff_get(self.h, None, None, omega.ctypes.data_as(ct.c_void_p) if what == 0 else None, beta.ctypes.data_as(ct.c_void_p) if what == 1 else None,
                                 ct.byref(scale)))
        return (omega, beta, scale.value)[what]

    omega = property(lambda self: self._get(0))
    beta = property(lambda self: self._get(1))
    scale = property(lambda self: self._get(2))

    def info(self):
        """The kernel's tiling (pmh_rff_info): dict(rows_per_workgroup, rows_per_wave, column_tile, k_block, lds_bytes, waves_per_workgroup)."""
        self._need()
        v = (ct.c_int * 8)()
        check(self.L.pmh_rff_info(self.h, v))
        return dict(zip(INFO, (int(x) for x in v)))

    def _source(self, X):
        """X as (DeviceSamples, made here): an ndarray goes up as float32 if it is float32 and as float64 otherwise."""
        if is_sparse(X):
            raise TypeError("RFFMap.transform: X is a scipy.sparse matrix; sparse samples are not supported by the map (it reads dense rows): pass X.toarray(), or dense blocks of rows")
        if isinstance(X, DeviceSamples):
            src, made = X, False
        else:
            src, made = DeviceSamples.from_numpy(self.ctx, X), True
        if src.d != self.d:
            if made:
                src.free()
            raise ValueError("RFFMap: X must be (n, %d), not (n, %d)" % (self.d, src.d))
        return src, made

    def transform(self, X, out_dtype=np.float64):
        """Z = scale cos(X Omega + beta) as DeviceSamples (n, D) of out_dtype (float64 or float32: rounded once, at the store), computed and left on the device
        (pmh_rff_apply).  X: an (n, d) ndarray -- float32 goes up and is read as float32, anything else as float64 -- or a DeviceSamples; all arithmetic is fp64."""
        src, made = self._source(X)
        Z = None
        try:
            self._need()
            odt = np.dtype(out_dtype)
            if odt not in TYPE_CODES:
                raise ValueError("RFFMap.transform: out_dtype must be numpy.float64 or numpy.float32, not %r" % (out_dtype,))
            Z = DeviceSamples.empty(self.ctx, src.n, self.D, odt)
            check(self.L.pmh_rff_apply(self.h, src.n, src.p, TYPE_CODES[src.dtype], Z.p, TYPE_CODES[odt]))
            out, Z = Z, None
            return out
        finally:
            if Z is not None:
                Z.free()
            if made:
                src.free()

    def arguments(self, X):
        """tests: T = X Omega + beta as an (n, D) float64 host array, from the SAME kernel with the identity in place of scale cos(.) (pmh_rff_test_args)."""
        src, made = self._source(X)
        T = None
        try:
            self._need()
            T = DeviceSamples.empty(self.ctx, src.n, self.D, np.float64)
            check(self.L.pmh_rff_test_args(self.h, src.n, src.p, TYPE_CODES[src.dtype], T.p))
            return T.numpy()
        finally:
            if T is not None:
                T.free()
            if made:
                src.free()

    def destroy(self):
        if self.h is not None:
            self.L.pmh_rff_destroy(self.h)
            self.h = None
