"""Data and bounds of tests/test_rff_score_host.py and tests/test_gpu_rff_score.py (no test in here): scoring on random Fourier features that are never
stored, dots[i, k] = sum_c s cos(x_i . omega_c + beta_c) W[k, c] (csrc/rff_score.hip).  The map's own data and bounds are tests/rff_cases.py's."""
import numpy as np

import rff_cases as R
from rff_cases import U, args_bound, args_longdouble, cos_bound, edge_shapes, int_case, real_case, rings  # noqa: F401

# ---- 1. indexing, exact -------------------------------------------------------------------------------------------------------------------------------------------
# X, Omega, beta: int_case (magnitude <= 8); W: integers of magnitude <= 8.  |t| <= 8 * 8 d + 8 and |dot| <= 8 D (64 d + 8): at the largest edge shape
# (d = 130, D = 257) 1.8e7, and every partial sum is an integer below that: far below 2^53, so fp64 is exact in any order, fused or not


def int_weights(K, D, seed):
    return np.random.default_rng(seed).integers(-8, 9, (K, D)).astype(np.float64)


def chunk_counts(kc):
    """The class counts on both sides of the chunk boundary, up to one past two whole chunks."""
    return sorted({1, kc - 1, kc, kc + 1, 2 * kc + 1} - {0})


# ---- 2. the cosine path: a derived bound --------------------------------------------------------------------------------------------------------------------------
# REAL_SHAPES and three narrow, ragged last tiles: D = 1 and 17 (one group of 64 columns, nearly all of it padding) and 65 (one column into the second group).  A
# padded column's feature is s cos(0 + 0) = s, not 0: only its zero weight keeps it out of the sum, and with the identity epilogue of test 1 the pad is 0
SCORE_SHAPES = R.REAL_SHAPES + [(5, 3, 1), (20, 7, 17), (33, 64, 65)]
SCORE_K = 5


def real_weights(K, D, seed):
    return np.random.default_rng(seed).standard_normal((K, D))


def dots_longdouble(X, omega, beta, scale, W):
    """(Z W', Z, T) in long double: T the arguments, Z = s cos T."""
    T = args_longdouble(X, omega, beta)
    Z = np.longdouble(scale) * np.cos(T)
    return Z @ W.astype(np.longdouble).T, Z, T


def dots_bound(X, omega, beta, scale, W):
    """|dots_dev - Z W'| <= E |W|' + (D + 9) u (|Z| + E) |W|', component-wise, with E = |s| A + c, A = args_bound, c = cos_bound(s).

    The feature: the device forms z~ = fl(s cos~(t~)) from its own argument t~, |t~ - t| <= A (args_bound).  |cos'| <= 1 carries the argument's error through the
    cosine unchanged, |s cos t~ - s cos t| <= |s| A, and cos_bound covers the device cosine's documented 2 ulp and the rounding of the product with s (and numpy's
    own cosine and product in the reference's place): |z~ - z| <= |s| A + c = E.
    The sum: sum_c z~_c w_c over D terms, each product fused into the sum (the kernel) or rounded on its own (numpy), in any order -- per lane, over the lanes'
    tree, over the column tiles -- accumulates at most D roundings of partial sums bounded by sum |z~_c||w_c| <= (|Z| + E)|W|': the bound args_bound uses for its
    d-term sum, constant 8 again for the second-order terms and the long-double reference's own error, and one more rounding for whoever adds the tiles.
    Together |sum z~ w - sum z w| <= sum |z~ - z||w| + (D + 9) u sum |z~||w| <= E |W|' + (D + 9) u (|Z| + E) |W|'."""
    D = omega.shape[1]
    _, Z, _ = dots_longdouble(X, omega, beta, scale, W)
    E = abs(scale) * args_bound(X, omega, beta) + cos_bound(scale)
    aW = np.abs(W).T
    return E @ aW + (D + 9) * U * ((np.abs(Z).astype(np.float64) + E) @ aW)


# ---- 3. bit identities ---------------------------------------------------------------------------------------------------------------------------------------------
BIT_SHAPES = [(64, 256), (37, 100), (130, 257)]
BIT_K = 7

# ---- 5. the front ends on the rings --------------------------------------------------------------------------------------------------------------------------------
RINGS = R.RINGS
MAPPED_ACCURACY_FLOOR = R.MAPPED_ACCURACY_FLOOR


def radius_classes(X):
    """Three classes by radius bins: inside the inner ring's radius, between the rings, outside the outer ring's radius (the noise puts points in all three)."""
    rad = np.hypot(X[:, 0], X[:, 1])
    return np.where(rad < 1.0, 0.0, np.where(rad < 2.0, 1.0, 2.0))


def score_bound(X, omega, beta, scale, w, b, score):
    """|score_dev - (Z w + b)| <= dots_bound + u (|score| + |b|): the bias is added to the ready dot product in one rounding of a number bounded by |score|, and
    |b| covers the reference's own addition.  w (D,) or (K, D), b scalar or (K,); (n,) or (n, K) like score."""
    w2 = np.atleast_2d(w)
    bd = dots_bound(X, omega, beta, scale, w2) + U * (np.abs(np.asarray(score).reshape(X.shape[0], -1)) + np.abs(np.atleast_1d(b)))
    return bd.reshape(np.shape(score))


def sigmoid(z):
    """1 / (1 + e^z) in the two-branch form the library uses."""
    z = np.asarray(z, dtype=np.float64)
    e = np.exp(-np.abs(z))
    return np.where(z >= 0.0, e / (1.0 + e), 1.0 / (1.0 + e))
