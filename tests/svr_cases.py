"""Helpers shared by tests/test_svr_host.py and tests/test_gpu_svr.py (no test in here): numpy's restatement of the regression dual

    min 1/2 u'H^u - c^'u,  u = [p; q],  H^ = [Q + D, -Q; -Q, Q + D],  Q = X X',  c^ = [t - eps; -t - eps]

of its model (w = X'(p - q), b_free) and the cases of the operator tests."""
import numpy as np

from svm_train_cases import ASTOL, EPS, gamma  # noqa: F401

# the operator, exact: every n with every d
OP_N = [1, 3, 301, 2003]
OP_D = [1, 37, 63, 64, 65, 130, 256]
# (shift, diagonal, sigma): plain; shift; diagonal; shift and sigma; diagonal and sigma -- powers of two
OP_TERMS = {"plain": (0.0, False, 0.0), "shift": (0.5, False, 0.0), "diag": (0.0, True, 0.0), "shift_sigma": (0.25, False, 2.0), "diag_sigma": (0.0, True, 4.0)}


def toarray(X):
    return X.toarray() if hasattr(X, "toarray") else np.asarray(X)


def int_case(n, d, seed):
    """Integer-valued data on which every sum of a product is exact in fp64: X in {-3..3}, p, q in {0..4}, the diagonal a power of two per sample."""
    r = np.random.default_rng(seed)
    X = r.integers(-3, 4, size=(n, d)).astype(np.float64)
    u = r.integers(0, 5, size=2 * n).astype(np.float64)
    diag = 2.0 ** r.integers(-2, 3, size=n)
    return X, u, diag


def int_case_csr(n, d, per_row, empty_frac, seed):
    """The same as a scipy CSR matrix with per_row entries a row (none in a fraction empty_frac of the rows)."""
    import scipy.sparse as sp

    r = np.random.default_rng(seed)
    cols = np.argsort(r.random((n, d)), axis=1)[:, :per_row]
    vals = r.integers(1, 4, size=(n, per_row)) * r.choice([-1.0, 1.0], size=(n, per_row))
    if empty_frac > 0:
        vals[r.random(n) < empty_frac] = 0.0
    X = sp.csr_matrix((vals.ravel(), (np.repeat(np.arange(n), per_row), cols.ravel())), shape=(n, d))
    X.eliminate_zeros()
    X.sort_indices()
    u = r.integers(0, 5, size=2 * n).astype(np.float64)
    diag = 2.0 ** r.integers(-2, 3, size=n)
    return X, u, diag


def D_of(n, shift=0.0, diag=None):
    return np.full(n, float(shift)) if diag is None else np.asarray(diag, dtype=np.float64)


def apply(X, u, D, sigma=0.0):
    """H^ u by the formulas of the operator: s = p - q, w = X's, S = sum s; out_p = X w + sigma S + D p, out_q = -X w - sigma S + D q."""
    n = X.shape[0]
    p, q = u[:n], u[n:]
    s = p - q
    v = X @ (X.T @ s) + sigma * s.sum()
    return np.concatenate([v + D * p, -v + D * q])


def hessian(X, D, sigma=0.0):
    """H^ as a dense 2n x 2n matrix, block by block."""
    X = toarray(X)
    n = X.shape[0]
    Q = X @ X.T + sigma * np.ones((n, n))
    return np.block([[Q + np.diag(D), -Q], [-Q, Q + np.diag(D)]])


def doubled_hessian(X, D, sigma=0.0):
    """The classification Hessian diag(y~) X~ X~' diag(y~) + D~ + sigma y~ y~' on the doubled samples X~ = [X; X], y~ = [+1; -1]."""
    X = toarray(X)
    n = X.shape[0]
    Xd, yd = np.vstack([X, X]), np.concatenate([np.ones(n), -np.ones(n)])
    return np.diag(yd) @ (Xd @ Xd.T) @ np.diag(yd) + np.diag(np.concatenate([D, D])) + sigma * np.outer(yd, yd)


def objective(X, t, eps, D, u):
    n = X.shape[0]
    s = u[:n] - u[n:]
    w = X.T @ s
    return 0.5 * (w @ w) + 0.5 * (np.concatenate([D, D]) * u) @ u - np.concatenate([t - eps, -t - eps]) @ u


def free_mask(u, ub):
    """The free entries of the box: astol < u_k and, where ub is given (L1: [C_i; C_i]), u_k < ub_k - astol."""
    return (u > ASTOL) & ((u < ub - ASTOL) if ub is not None else True)


def np_model(X, t, eps, u, D, ub, with_D=True):
    """w, b_free and the free mask of the dual u: b_free is the mean over the free entries of t_i - eps - D_i p_i - x_i . w (p side) and
    t_i + eps + D_i q_i - x_i . w (q side), each evaluated left to right as the library does.  with_D=False leaves the D terms out (what a restatement that
    forgot them would give)."""
    n = X.shape[0]
    p, q = u[:n], u[n:]
    w = X.T @ (p - q)
    dot = X @ w
    Dd = D if with_D else np.zeros(n)
    terms = np.concatenate([((t - eps) - Dd * p) - dot, ((t + eps) + Dd * q) - dot])
    free = free_mask(u, ub)
    return w, (float(np.mean(terms[free])) if free.any() else float("nan")), free


def b_bound(X, u, w, free, terms_mag):
    """What the library's b_free may differ from np_model's by: the dot products x_i . w of the free entries (the library's w is within 2 gamma_{n+1} |X|'|beta|
    of numpy's, a d-term dot on either side), and the mean of nf terms of magnitude terms_mag summed in another order (gamma_{nf+4}: the term's own three
    roundings and the division)."""
    n, d = X.shape
    aX = abs(X)
    rows = np.concatenate([np.arange(n), np.arange(n)])[free]
    Wc = aX.T @ np.abs(u[:n] - u[n:])
    nf = int(free.sum())
    return float(2 * gamma(d + 1) * np.mean(aX[rows] @ np.abs(w)) + 2 * gamma(n + 1) * np.mean(aX[rows] @ Wc) + 2 * gamma(nf + 4) * np.mean(terms_mag[free]))


def oracle_mpgp(oracle, X, t, eps, D, ub, rtol=1e-6):
    """The CPU oracle's MPGP on the 2n problem, the operator a function (as svm_train_cases.oracle_train)."""
    n = X.shape[0]
    Xt = X.T.tocsr() if hasattr(X, "tocsr") else X.T
    DD = np.concatenate([D, D])

    def fn(u):
        v = X @ (Xt @ (u[:n] - u[n:]))
        return np.concatenate([v, -v]) + DD * u

    box = oracle.Box(2 * n, lb=np.zeros(2 * n), ub=ub)
    return oracle.mpgp(oracle.Op(2 * n, fn=fn), np.concatenate([t - eps, -t - eps]), np.zeros(2 * n), box, rtol=rtol)


def oracle_smalxe(oracle, X, t, eps, D, ub, rtol=1e-6, max_it=100):
    """The CPU oracle's SMALXE on the 2n problem with the unit row [1; -1] / sqrt(2n)."""
    n = X.shape[0]
    Xt = X.T.tocsr() if hasattr(X, "tocsr") else X.T
    DD = np.concatenate([D, D])

    def fn(u):
        v = X @ (Xt @ (u[:n] - u[n:]))
        return np.concatenate([v, -v]) + DD * u

    row = np.concatenate([np.ones(n), -np.ones(n)]) / np.sqrt(2 * n)
    pf = oracle.Qppf(oracle.Csr(1, 2 * n, [0, 2 * n], np.arange(2 * n), row), orthonormal=True)
    box = oracle.Box(2 * n, lb=np.zeros(2 * n), ub=ub)
    return oracle.smalxe(oracle.Op(2 * n, fn=fn), np.concatenate([t - eps, -t - eps]), np.zeros(2 * n), box, pf, rtol=rtol, max_it=max_it)


# "what the model is for", noise-free: svr_linear(TUBE_N, TUBE_D, 0, TUBE_SEED) with eps = 0.05 and C = TUBE_C, which the CPU test shows to be large enough
# that no entry of the oracle's solution is at its bound
TUBE_N, TUBE_D, TUBE_SEED, TUBE_EPS, TUBE_C = 400, 8, 11, 0.05, 100.0
