"""Random Fourier features restated in numpy, and the data of tests/test_rff_host.py and tests/test_gpu_rff.py (no test in here).

    z(x) = s cos(Omega'x + beta),  s = sqrt(2 / D),  beta = 2 pi U[0, 1)
    rbf        k(x, x') = exp(-gamma |x - x'|_2^2):  Omega = sqrt(2 gamma) N(0, 1)   (the density of exp(-gamma r^2) is N(0, 2 gamma I))
    laplacian  k(x, x') = exp(-gamma |x - x'|_1):    Omega = gamma standard Cauchy

The draw is restated, not imported: one default_rng(seed), Omega first, then beta."""
import math

import numpy as np

U = 2.0 ** -53  # unit roundoff of fp64


def draw(d, D, gamma, kernel, seed):
    rng = np.random.default_rng(seed)
    if kernel == "rbf":
        omega = math.sqrt(2.0 * gamma) * rng.standard_normal((d, D))
    else:
        omega = gamma * rng.standard_cauchy((d, D))
    return omega, 2.0 * math.pi * rng.random(D), math.sqrt(2.0 / D)


def features(X, omega, beta, scale):
    return scale * np.cos(X @ omega + beta)


def gram(X, gamma, kernel):
    diff = X[:, None, :] - X[None, :, :]
    return np.exp(-gamma * ((diff ** 2).sum(-1) if kernel == "rbf" else np.abs(diff).sum(-1)))


# ---- the spectral density: D features against the exact Gram matrix ----------------------------------------------------------------------------------------------
DENSITY_D, DENSITY_GAMMA, DENSITY_SEED = 4096, 0.25, 0
DENSITY_CAP = 5.0 / math.sqrt(DENSITY_D)  # 0.078: five standard deviations of a mean of D terms that are bounded by 2 in magnitude (variance <= 1)


def density_points():
    return 0.5 * np.random.default_rng(5).standard_normal((40, 8))


# ---- 1. indexing, exact: small integers, every partial sum an integer below 2^53 --------------------------------------------------------------------------------
BASE = (37, 7, 40)


def int_case(n, d, D, seed):
    """X (n, d), Omega (d, D), beta (D): integers of magnitude <= 8, as float64 (exact in float32 too)."""
    r = np.random.default_rng(seed)
    return (r.integers(-8, 9, (n, d)).astype(np.float64), r.integers(-8, 9, (d, D)).astype(np.float64), r.integers(-8, 9, D).astype(np.float64))


def edge_shapes(RW, CT, KB):
    """(n, d, D): one axis at a time around BASE over the kernel's edges, then the four corners with all three axes at an edge."""
    n0, d0, D0 = BASE
    ns = [1, 15, 16, 17, RW - 1, RW, RW + 1, 2 * RW + 3]
    ds = [1, 3, 4, 5, KB - 1, KB, KB + 1, 2 * KB + 2]
    Ds = [1, 15, 16, 17, CT - 1, CT, CT + 1, 250, 256, 257]
    Ds += [q * CT // 4 + e for q in (1, 2, 3) for e in (0, 1)]  # the kernel's instances cover a last tile of 1, 2, 3 or 4 quarters of the column tile
    shapes = [(n, d0, D0) for n in ns] + [(n0, d, D0) for d in ds] + [(n0, d0, D) for D in Ds]
    shapes += [(RW + 1, KB + 1, CT + 1), (RW - 1, KB - 1, CT - 1), (1, 1, 1), (2 * RW + 3, 2 * KB + 2, 257)]
    return sorted(set(shapes))


# ---- 2. real data: the derived bounds -----------------------------------------------------------------------------------------------------------------------------
REAL_SHAPES = [(300, 64, 256), (131, 37, 100), (77, 130, 257)]


def real_case(n, d, D, seed):
    """X ~ 3 N(0, 1), Omega ~ 4 N(0, 1), beta in [0, 2 pi): arguments of up to a few hundred in magnitude."""
    r = np.random.default_rng(seed)
    return 3.0 * r.standard_normal((n, d)), 4.0 * r.standard_normal((d, D)), 2.0 * math.pi * r.random(D)


def args_longdouble(X, omega, beta):
    return X.astype(np.longdouble) @ omega.astype(np.longdouble) + beta.astype(np.longdouble)


def args_bound(X, omega, beta):
    """|T_dev - T| <= (d + 9) u (|X||Omega| + |beta|), component-wise: a sum of d products, each fused into the sum or rounded on its own, in any order, accumulates
    at most d roundings of partial sums bounded by |X||Omega| (the bound tests/orbit_cases.py derives, constant 8 for the reference's own error and the second-order
    terms); adding beta is one more rounding of a number bounded by |X||Omega| + |beta|."""
    return (X.shape[1] + 9) * U * (np.abs(X) @ np.abs(omega) + np.abs(beta))


def cos_bound(scale):
    """|Z_dev - s cos(T_dev)| <= 4 * 2^-52 |s|: the device library documents 2 ulp for the double cosine (|cos| <= 1: an ulp is at most 2^-52), numpy's own cosine
    is within 1 ulp, and the product with s is rounded once on either side (2^-53 each)."""
    return 4.0 * 2.0 ** -52 * abs(scale)


# ---- 6. the point of it: two rings ---------------------------------------------------------------------------------------------------------------------------------
def rings(n, seed):
    """n points on two rings of radius 1 (label +1) and 2 (label -1) with 0.1 N(0, 1) radial noise: X (n, 2), y, and the ring's radius as a regression target."""
    r = np.random.default_rng(seed)
    y = np.where(r.random(n) < 0.5, 1.0, -1.0)
    t = np.where(y > 0, 1.0, 2.0)
    rad = t + 0.1 * r.standard_normal(n)
    phi = 2.0 * math.pi * r.random(n)
    return np.column_stack([rad * np.cos(phi), rad * np.sin(phi)]), y, t


RINGS = dict(n_train=400, seed_train=1, n_test=400, seed_test=2, d=2, D=64, gamma=1.0, seed=0)
LINEAR_ACCURACY_CAP, MAPPED_ACCURACY_FLOOR = 0.70, 0.95
LINEAR_R2_CAP, MAPPED_R2_FLOOR = 0.2, 0.9
