"""Nystroem features restated in numpy, and the data and bounds of tests/test_nys_host.py and tests/test_gpu_nys.py (no test in here).

    z(x) = M'k(L, x),  M = U_r Lambda_r^{-1/2} from k(L, L) = U Lambda U' (the eigenvalues above rcond lambda_max, descending, at most n_components)
    rbf   k(x, l) = exp(-gamma |x - l|_2^2)
    poly  k(x, l) = (gamma x . l + coef0)^degree

The set-up is restated, not imported.  The data of tests/rff_cases.py is shared: the rings, density_points, real_case, edge_shapes."""
import numpy as np

import rff_cases as R

U = R.U  # unit roundoff of fp64


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------------------------------
def poly_of_args(T, gamma, coef0, degree):
    """(gamma t + coef0)^degree as the device forms it: two roundings for b, then b multiplied by b another degree - 1 times, left to right."""
    b = gamma * T + coef0
    v = b
    for _ in range(degree - 1):
        v = v * b
    return v


def gram(A, B, kernel, gamma=1.0, coef0=1.0, degree=3):
    if kernel == "rbf":
        return np.exp(-gamma * ((A[:, None, :] - B[None, :, :]) ** 2).sum(-1))
    return poly_of_args(A @ B.T, gamma, coef0, degree)


def whitening(L, kernel, gamma=1.0, coef0=1.0, degree=3, n_components=None, rcond=1e-12):
    K = gram(L, L, kernel, gamma, coef0, degree)
    lam, Q = np.linalg.eigh(0.5 * (K + K.T))
    lam, Q = lam[::-1], Q[:, ::-1]
    keep = int((lam > rcond * lam[0]).sum())
    if n_components is not None:
        keep = min(keep, n_components)
    return Q[:, :keep] / np.sqrt(lam[:keep]), lam[:keep]


def features(X, L, M, kernel, gamma=1.0, coef0=1.0, degree=3):
    return gram(X, L, kernel, gamma, coef0, degree) @ M


def landmarks(X, m, seed):
    return X[np.random.default_rng(seed).choice(X.shape[0], m, replace=False)]


# ---- host: Z Z' against the projected and the exact kernel matrix -----------------------------------------------------------------------------------------------
DENSITY_GAMMA = R.DENSITY_GAMMA  # 0.25 on the 40 points of rff_cases.density_points(): k(L, L) of all 40 has the condition number 1.4e3


def projection_cap(eigenvalues, m):
    """|Z Z' - C K^+ C'| and, with the landmarks all the points, |Z Z' - K| <= 8 cond m 2^-52, for kernel values of magnitude <= 1: an eigenvector of a symmetric
    matrix comes out of eigh with an error of u times the norm over the gap, so K^+ = U Lambda^-1 U', whichever way it is formed, is off by a relative u cond in
    norm, and the three products of m terms each add m u times values that C K^+ C' <= 1 bounds; 8 for the constants left out (the one tests/rff_cases.py uses)."""
    return 8.0 * (eigenvalues[0] / eigenvalues[-1]) * m * 2.0 ** -52


# ---- 1. indexing, exact: small integers, every intermediate an integer below 2^53 --------------------------------------------------------------------------------
def int_case(n, d, m, D, seed):
    """X (n, d), L (m, d), M (m, D), coef0: integers of magnitude <= 8, as float64 (exact in float32 too).  |x . l| <= 64 d, so at d <= 130 (x . l + coef0)^3 stays
    below 6e11, |x - l|^2 below 4e4 and a row of (X L' + coef0) M below 2e7 at m <= 257."""
    r = np.random.default_rng(seed)
    return (r.integers(-8, 9, (n, d)).astype(np.float64), r.integers(-8, 9, (m, d)).astype(np.float64), r.integers(-8, 9, (m, D)).astype(np.float64), float(r.integers(-8, 9)))


def stage_b_shapes():
    """(m, D) around the k-block and the column tile of the second product, D capped at m."""
    return sorted({(m, min(D, m)) for m in (63, 64, 65, 130) for D in (1, 63, 64, 65, 257)})


# ---- 2. real data: the derived bounds -----------------------------------------------------------------------------------------------------------------------------
REAL_SHAPES = R.REAL_SHAPES  # read as (n, d, m)


def real_case(n, d, m, D, seed):
    """X ~ 3 N(0, 1), L ~ 4 N(0, 1) (rff_cases.real_case with Omega = L'), M ~ N(0, 1), and the gamma that puts gamma |x - l|^2 around 1 (E |x - l|^2 = 25 d)."""
    X, omega, _ = R.real_case(n, d, m, seed)
    return X, np.ascontiguousarray(omega.T), np.random.default_rng(seed + 1).standard_normal((m, D)), 1.0 / (25.0 * d)


def args_longdouble(X, L):
    return X.astype(np.longdouble) @ L.T.astype(np.longdouble)


def args_bound(X, L):
    return R.args_bound(X, L.T, np.zeros(L.shape[0]))


def dist_longdouble(X, L):
    return ((X.astype(np.longdouble)[:, None, :] - L.astype(np.longdouble)[None, :, :]) ** 2).sum(-1)


def dist_bound(X, L):
    """|q_dev - |x - l|^2| <= (d + 9) u (|x|^2 + |l|^2 + 2 |x|.|l|), component-wise.  A norm is a sum of d squares, each rounded and then added: (d + 1) u |x|^2, and
    the same for |l|^2; the product t = x . l is off by at most d u |x|.|l| (rff_cases.args_bound without its constant), and is doubled exactly; (nx + nl) and the
    difference with 2 t are one rounding each of numbers bounded by |x|^2 + |l|^2 + 2 |x|.|l|.  Together (d + 3) u of that sum; the constant 9 leaves the room
    rff_cases.args_bound leaves for the reference's own error and the second-order terms.  The maximum with 0 only moves q towards the exact value, which is >= 0."""
    d = X.shape[1]
    return (d + 9) * U * ((X ** 2).sum(1)[:, None] + (L ** 2).sum(1)[None, :] + 2.0 * (np.abs(X) @ np.abs(L.T)))


# |C_dev - exp(-(gamma q_dev))| with numpy's exponential of the device's own q: the device library documents 1 ulp for the double exponential, numpy's own is within
# 1 ulp, and the argument -(gamma q) has the same bits on either side (one product, rounded once); a value is at most 1, so an ulp is at most 2^-52
RBF_BOUND = 2.0 * 2.0 ** -52


def product_bound(Cb, M):
    """|Z_dev - C M| <= (m + 9) u |C||M|, component-wise, for the device's own C: a sum of m products as in rff_cases.args_bound."""
    return (Cb.shape[1] + 9) * U * (np.abs(Cb) @ np.abs(M))


# ---- 3. bit identities -----------------------------------------------------------------------------------------------------------------------------------------------
BIT_SHAPES = [(64, 256, 256), (37, 100, 60), (130, 257, 257)]  # (d, m, D)

# ---- 5. the point of it: the rings of rff_cases ----------------------------------------------------------------------------------------------------------------------
RINGS = dict(R.RINGS, m=32, landmark_seed=0, gamma=1.0, poly=dict(degree=2, gamma=1.0, coef0=1.0, D=6))
MAPPED_ACCURACY_FLOOR, MAPPED_R2_FLOOR = R.MAPPED_ACCURACY_FLOOR, R.MAPPED_R2_FLOOR  # 0.95, 0.9
EXACT_FACTOR, EXACT_FLOOR = 100.0, 1e-14  # Z Z' of the rank-6 polynomial map against the exact kernel matrix: within 100 x the restatement's own error, the cap floored at 1e-14 max|K|
