"""Nystroem features (pmh_nys_*, csrc/nys.hip): z(x) = M'k(L, x) with landmarks L (m, d) taken from the data and M = U_r Lambda_r^{-1/2} from the
eigen-decomposition k(L, L) = U Lambda U', so that z(x) . z(x') = k(x, L) k(L, L)^+ k(L, x') ~ k(x, x') (Williams and Seeger, 2001).  A linear SVM, SVMMulticlass
or SVR on Z = transform(X) is an approximate kernel machine, and every tool of the linear front ends -- subsets, cross-validation, grid search, warm starts,
penalties, Platt scaling -- works on it unchanged:

    L = nystroem.sample_landmarks(X, 256, seed=0)
    fmap = NystroemMap(ctx, L, kernel="rbf", gamma=0.5)      # or kernel="poly", gamma, coef0, degree
    Z = fmap.transform(X)                                     # DeviceSamples (n, fmap.D): computed and kept on the device
    svm = SVM(ctx, C=10).fit(Z, y)
    svm.predict(fmap.transform(Xt))

    rbf:   k(x, l) = exp(-gamma |x - l|_2^2)
    poly:  k(x, l) = (gamma x . l + coef0)^degree

The landmarks and the whitening M are the host's (numpy: default_rng(seed).choice, eigh); the map itself is two HIP kernels on the fp64 matrix cores per chunk of
rows, C = k(X, L) and Z = C M; there is no CPU fallback.  D, the number of eigenvalues kept (those above rcond lambda_max, at most n_components), depends on the
data: the polynomial kernel of degree 2 in 2 dimensions has rank 6, whatever m is, and the map is then exact.

The device forms |x - l|^2 from |x|^2, |l|^2 and x . l, as the matrix cores require: a sample that is itself a landmark gets a squared distance of the order of
u d |x|^2, not exactly 0.

Not here: sparse X, the Laplacian kernel (it is no function of x . l and the norms: RFFMap has it), k-means landmarks, gamma = "scale", scoring without storing Z
(RFFMap.lazy), the eigen-decomposition on the device."""
import ctypes as ct
import math

import numpy as np

from ._lib import check
from .core import Vec
from .featuremap import TYPE_CODES, FeatureMap
from .mat import is_sparse

KERNELS = ("rbf", "poly")  # PMH_NYS_RBF, PMH_NYS_POLY
MAX_DEGREE = 16
# pmh_nys_info: the tiling of the kernel behind kernel_block, then (chunk_rows, workspace_bytes) of transform
INFO = ("rows_per_workgroup", "rows_per_wave", "column_tile", "k_block", "lds_bytes", "waves_per_workgroup", "chunk_rows", "workspace_bytes")


def _check_kernel(kernel, gamma, coef0, degree):
    if kernel not in KERNELS:
        raise ValueError("NystroemMap: kernel must be one of %s, not %r" % (", ".join(KERNELS), kernel))
    if not (gamma > 0.0 and math.isfinite(gamma)):
        raise ValueError("NystroemMap: gamma = %r, must be positive and finite" % gamma)
    if not math.isfinite(coef0):
        raise ValueError("NystroemMap: coef0 = %r, must be finite" % coef0)
    if int(degree) != degree or not 1 <= degree <= MAX_DEGREE:
        raise ValueError("NystroemMap: degree = %r, must be an integer in 1 .. %d" % (degree, MAX_DEGREE))


def gram(A, B, kernel="rbf", gamma=1.0, coef0=1.0, degree=3):
    """k(A, B) (a, b) for A (a, d), B (b, d): rbf from the differences, exp(-gamma |a - b|^2); poly (gamma a . b + coef0)^degree.  Host only, for the set-up."""
    gamma, coef0 = float(gamma), float(coef0)
    _check_kernel(kernel, gamma, coef0, degree)
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    if A.ndim != 2 or B.ndim != 2 or A.shape[1] != B.shape[1]:
        raise ValueError("nystroem.gram: A and B must be (a, d) and (b, d)")
    if kernel == "rbf":
        return np.exp(-gamma * ((A[:, None, :] - B[None, :, :]) ** 2).sum(-1))
    return (gamma * (A @ B.T) + coef0) ** int(degree)


def sample_landmarks(X, m, seed=0):
    """X[default_rng(seed).choice(n, m, replace=False)]: m rows of X, without repetition.  Host only."""
    if is_sparse(X):
        raise TypeError("nystroem.sample_landmarks: X is a scipy.sparse matrix; sparse samples are not supported: pass X.toarray()")
    X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError("nystroem.sample_landmarks: X must be (n, d)")
    n, m = X.shape[0], int(m)
    if m < 1 or m > n:
        raise ValueError("nystroem.sample_landmarks: m = %d, must be 1 .. n = %d" % (m, n))
    return X[np.random.default_rng(seed).choice(n, m, replace=False)]


def whitening(landmarks, kernel="rbf", gamma=1.0, coef0=1.0, degree=3, n_components=None, rcond=1e-12):
    """(M (m, D), eigenvalues (D,)) with M = U_r / sqrt(lambda_r) from eigh of the symmetrised gram(L, L): the eigenvalues above rcond lambda_max, in descending
    order, at most n_components of them.  Host only."""
    L = np.asarray(landmarks, dtype=np.float64)
    K = gram(L, L, kernel, gamma, coef0, degree)
    if n_components is not None and int(n_components) < 1:
        raise ValueError("NystroemMap: n_components = %r, must be at least 1" % (n_components,))
    lam, U = np.linalg.eigh(0.5 * (K + K.T))
    lam, U = lam[::-1], U[:, ::-1]
    keep = int((lam > rcond * lam[0]).sum())
    if n_components is not None:
        keep = min(keep, int(n_components))
    if keep < 1:
        raise ValueError("NystroemMap: k(L, L) has no positive eigenvalue")
    return np.ascontiguousarray(U[:, :keep] / np.sqrt(lam[:keep])), lam[:keep].copy()


class NystroemMap(FeatureMap):
    ENTRY, INFO = "pmh_nys", INFO

    def __init__(self, ctx, landmarks, kernel="rbf", gamma=1.0, coef0=1.0, degree=3, n_components=None, rcond=1e-12):
        M, lam = whitening(landmarks, kernel, gamma, coef0, degree, n_components, rcond)
        self._create(ctx, landmarks, M, kernel, gamma, coef0, degree)
        self.eigenvalues = lam

    @classmethod
    def from_arrays(cls, ctx, landmarks, M, kernel="rbf", gamma=1.0, coef0=1.0, degree=3):
        """A saved map: landmarks (m, d) and M (m, D).  Nothing is decomposed and nothing drawn."""
        f = cls.__new__(cls)
        f._create(ctx, landmarks, M, kernel, gamma, coef0, degree)
        f.eigenvalues = None
        return f

    def _create(self, ctx, landmarks, M, kernel, gamma, coef0, degree):
        gamma, coef0 = float(gamma), float(coef0)
        _check_kernel(kernel, gamma, coef0, degree)
        L, M = np.ascontiguousarray(landmarks, dtype=np.float64), np.ascontiguousarray(M, dtype=np.float64)
        if L.ndim != 2 or M.ndim != 2 or M.shape[0] != L.shape[0]:
            raise ValueError("NystroemMap: landmarks must be (m, d) and M (m, D)")
        self.ctx, self.L, self.h = ctx, ctx.L, None
        (self.m, self.d), self.D = L.shape, M.shape[1]
        self.kernel, self.gamma, self.coef0, self.degree = kernel, gamma, coef0, int(degree)
        ld, md = Vec.from_numpy(ctx, L.ravel()), Vec.from_numpy(ctx, M.ravel())
        try:
            h = ct.c_void_p()
            check(self.L.pmh_nys_create(ctx.h, self.d, self.m, self.D, ld.p, KERNELS.index(kernel), gamma, coef0, self.degree, md.p, ct.byref(h)))
            self.h = h
        finally:
            ld.free()
            md.free()

    def _get(self, what):
        self._need()
        a = np.empty((self.m, self.d if what == 0 else self.D))
        p = a.ctypes.data_as(ct.c_void_p)
        check(self.L.pmh_nys_get(self.h, None, None, None, None, None, None, None, p if what == 0 else None, p if what == 1 else None))
        return a

    landmarks = property(lambda self: self._get(0))
    M = property(lambda self: self._get(1))

    def set_chunk_rows(self, rows):
        """The rows of C = k(X, L) that exist at a time in transform: a positive multiple of rows_per_workgroup.  No result depends on it."""
        self._need()
        check(self.L.pmh_nys_set_chunk_rows(self.h, int(rows)))
        return self

    def transform(self, X, out_dtype=np.float64):
        """Z = k(X, L) M as DeviceSamples (n, D) of out_dtype (float64 or float32: rounded once, at the store), computed and left on the device (pmh_nys_apply).
        X: an (n, d) ndarray -- float32 goes up and is read as float32, anything else as float64 -- or a DeviceSamples; all arithmetic is fp64."""
        odt = self._out_dtype(out_dtype)
        return self._run(X, "D", odt, lambda src, Z: self.L.pmh_nys_apply(self.h, src.n, src.p, TYPE_CODES[src.dtype], Z.p, TYPE_CODES[odt]))

    def kernel_block(self, X):
        """C = k(X, L) as DeviceSamples (n, m), float64 (pmh_nys_kernel).  X as in transform."""
        return self._run(X, "m", np.float64, lambda src, Cb: self.L.pmh_nys_kernel(self.h, src.n, src.p, TYPE_CODES[src.dtype], Cb.p))

    def _test_args(self, X, what):
        return self._run_host(X, "m", lambda src, T: self.L.pmh_nys_test_args(self.h, src.n, src.p, TYPE_CODES[src.dtype], what, T.p))

    def arguments(self, X):
        """tests: t = X L' as an (n, m) float64 host array, from the SAME kernel as kernel_block with the identity in place of the kernel function."""
        return self._test_args(X, 0)

    def distances(self, X):
        """tests, rbf maps: q = max((|x|^2 + |l|^2) - 2 x . l, 0) as an (n, m) float64 host array, what the SAME kernel exponentiates."""
        return self._test_args(X, 1)
