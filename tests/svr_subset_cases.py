"""Helpers shared by tests/test_svr_subset_host.py and tests/test_gpu_svr_subset.py (no test in here): the held-out pattern, numpy's restatement of the
regression operator under a sample subset S (mask m)

    out = M^ [Q + D, -Q; -Q, Q + D] M^ u + sigma (e^'u) e^,   M^ = diag([m; m]),  e^ = [m; -m]

and the pooled metrics of a cross-validation, all on top of svr_cases.py."""
import numpy as np

import svr_cases as S


def train_mask(n):
    """The training mask over n samples.  n >= 301: held out are rows 0 and n - 1, the block 61 .. 194 (row groups of 8 or 16 that are wholly held out, and
    groups cut in the middle at both ends) and every 5th row from 3.  n = 3: row 1.  n = 1: nothing is held out."""
    m = np.ones(n, dtype=bool)
    if n == 3:
        m[1] = False
    elif n > 3:
        assert n >= 301
        m[[0, n - 1]] = False
        m[61:195] = False
        m[3::5] = False
    return m


def doubled(m):
    return np.concatenate([m, m])


def mask_operand(u, m):
    """M^ u by selection."""
    return np.where(doubled(m), u, 0.0)


def apply_sub(X, u, D, sigma, m):
    """m^ o apply(X, m^ o u, D, sigma): with the operand masked, s = p - q vanishes outside S, so w = X_S's_S and the sigma term's sum run over S."""
    return np.where(doubled(m), S.apply(X, mask_operand(u, m), D, sigma), 0.0)


def hessian_sub(X, D, sigma, m):
    """The matrix of apply_sub: M^ H^ M^ + sigma e^ e^' (the sigma term of S.hessian is sigma e e', and M^ e = e^)."""
    M = np.diag(doubled(m).astype(np.float64))
    return M @ S.hessian(X, D, sigma) @ M


def poison(u, m, seed=0):
    """u with NaN and 1e300 (alternating, random signs) written into the held-out entries of both halves."""
    v = u.copy()
    out = np.flatnonzero(~doubled(m))
    r = np.random.default_rng(seed)
    v[out] = np.where(np.arange(out.size) % 2 == 0, np.nan, 1e300 * r.choice([-1.0, 1.0], size=out.size))
    return v


def pooled(folds):
    """The pooled metrics of a cross-validation from the folds' sums, written out independently of permon_amd.svm.pooled_metrics."""
    n = sum(f["n"] for f in folds)
    sr2, sar = sum(f["sum_r2"] for f in folds), sum(f["sum_abs_r"] for f in folds)
    st, st2 = sum(f["sum_t"] for f in folds), sum(f["sum_t2"] for f in folds)
    return dict(n=n, mse=sr2 / n, mae=sar / n, r2=1.0 - sr2 / (st2 - st * st / n), max_abs=max(f["max_abs"] for f in folds))
