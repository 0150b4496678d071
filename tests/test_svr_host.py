"""CPU-only checks behind tests/test_gpu_svr.py: the numpy restatement of the regression dual against the doubled classification Hessian, problems.svr_linear,
and the choices of data the GPU tests rely on (the C of the noise-free case, the share of samples near the edge of the tube)."""
import numpy as np
import pytest

from permon_amd import problems as P
import svr_cases as S
from svr_cases import ASTOL, gamma


@pytest.mark.parametrize("kind", ["plain", "shift", "diag", "shift_sigma", "diag_sigma"])
def test_restated_hessian_is_the_doubled_classification_hessian(kind):
    """H^ = [Q + D, -Q; -Q, Q + D] (+ sigma e e') equals diag(y~) X~ X~' diag(y~) + D~ (+ sigma y~ y~') on X~ = [X; X], y~ = [+1; -1] as a matrix, and the
    formulas of the operator (s = p - q, w = X's, both halves from the one X w) apply it.  Integer data: every entry and every product is exact, so ==."""
    shift, use_diag, sigma = S.OP_TERMS[kind]
    X, u, diag = S.int_case(23, 7, 3)
    D = S.D_of(23, shift, diag if use_diag else None)
    H = S.hessian(X, D, sigma)
    assert np.array_equal(H, S.doubled_hessian(X, D, sigma))
    assert np.array_equal(H, H.T)
    assert np.array_equal(H @ u, S.apply(X, u, D, sigma))
    Xs, us, ds = S.int_case_csr(40, 30, 5, 0.2, 4)
    Ds = S.D_of(40, shift, ds if use_diag else None)
    assert (np.diff(Xs.indptr) == 0).any()  # (the case has empty rows)
    assert np.array_equal(S.hessian(Xs, Ds, sigma) @ us, S.apply(Xs, us, Ds, sigma))


def test_objective_and_model_restatements_agree_with_the_matrix():
    """1/2 u'H^u - c^'u through w = X'(p - q) equals the matrix form, and b_free's two expressions are stationarity in a free entry: with g = H^u - c^ + b e,
    t - eps - D p - x.w - b = -g_p and t + eps + D q - x.w - b = g_q."""
    p = P.svr_linear(60, 5, 0.3, 2)
    X, t, n = p["X"], p["t"], p["n"]
    r = np.random.default_rng(0)
    u, D = r.uniform(0.0, 1.0, 2 * n), r.uniform(0.5, 2.0, n)
    H, c = S.hessian(X, D), np.concatenate([t - 0.1, -t - 0.1])
    assert abs(S.objective(X, t, 0.1, D, u) - (0.5 * u @ H @ u - c @ u)) <= 1e-12 * abs(c @ u)
    w = X.T @ (u[:n] - u[n:])
    b = 0.7
    g = H @ u - c + b * np.concatenate([np.ones(n), -np.ones(n)])
    assert np.allclose((t - 0.1 - D * u[:n] - X @ w) - b, -g[:n], atol=1e-12) and np.allclose((t + 0.1 + D * u[n:] - X @ w) - b, g[n:], atol=1e-12)
    # np_model: the mean of exactly those expressions over the free entries, and the D terms matter once D varies
    ub = np.full(2 * n, 0.9)
    w1, b1, free = S.np_model(X, t, 0.1, u, D, ub)
    assert np.array_equal(free, (u > ASTOL) & (u < 0.9 - ASTOL)) and 0 < free.sum() < 2 * n
    terms = np.concatenate([t - 0.1 - D * u[:n] - X @ w, t + 0.1 + D * u[n:] - X @ w])
    assert abs(b1 - terms[free].mean()) <= 1e-13 and np.array_equal(w1, w)
    assert abs(S.np_model(X, t, 0.1, u, D, ub, with_D=False)[1] - b1) > 1e-3


def test_svr_linear():
    p = P.svr_linear(200, 9, 0.25, 4, b_true=-1.5, eps=0.2, C=3.0, n_test=50)
    X, t, n = p["X"], p["t"], p["n"]
    assert X.shape == (200, 9) and t.shape == (200,) and p["w_true"].shape == (9,) and p["b_true"] == -1.5 and n == 200
    assert np.isfinite(t).all()
    noise = t - X @ p["w_true"] - p["b_true"]
    assert 0.2 < noise.std() < 0.3 and abs(noise.mean()) < 0.06  # noise * N(0, 1), 200 draws
    assert np.array_equal(p["c"], np.concatenate([t - 0.2, -t - 0.2])) and p["c"].shape == (400,)
    assert np.array_equal(p["lb"], np.zeros(400)) and np.array_equal(p["ub"], np.full(400, 3.0)) and np.array_equal(p["x0"], np.zeros(400))
    assert p["X_test"].shape == (50, 9) and p["t_test"].shape == (50,)
    q = P.svr_linear(200, 9, 0.25, 4, b_true=-1.5, eps=0.2, C=3.0)
    assert np.array_equal(q["X"], X) and np.array_equal(q["t"], t)  # the same seed, the same draw
    assert not np.array_equal(P.svr_linear(200, 9, 0.25, 5)["X"], X)
    z = P.svr_linear(100, 4, 0.0, 1)
    assert np.allclose(z["t"], z["X"] @ z["w_true"] + z["b_true"], rtol=0, atol=1e-14)  # noise-free


def test_svr_linear_sparse():
    """In the style of svm_sparse: unit rows, sorted indices, popular features first."""
    p = P.svr_linear(300, 200, 0.1, 6, sparse=(12, 1.0), n_test=40)
    X = p["X"]
    assert hasattr(X, "tocsr") and X.shape == (300, 200) and X.has_sorted_indices and p["X_test"].shape == (40, 200)
    nr = np.sqrt(np.asarray(X.multiply(X).sum(axis=1)).ravel())
    assert np.allclose(nr, 1.0) and np.diff(X.indptr).max() <= 12
    cnt = np.bincount(X.indices, minlength=200)
    assert cnt[:20].sum() > cnt[-100:].sum()  # 1 / rank popularity
    assert np.allclose(p["t"] - X @ p["w_true"] - p["b_true"], p["t"] - np.asarray(X @ p["w_true"]).ravel() - p["b_true"])
    assert abs((p["t"] - X @ p["w_true"] - p["b_true"]).std() - 0.1) < 0.02


def test_noise_free_case_has_no_entry_at_its_bound(oracle):
    """The data of test_gpu_svr.py::test_noise_free_residuals_stay_in_the_tube: with C = TUBE_C the oracle's solution (SMALXE on the 2n problem) has no entry
    at the upper bound, so the box does not bind and every residual of the model lies in the tube up to the tolerance of the solve."""
    p = P.svr_linear(S.TUBE_N, S.TUBE_D, 0.0, S.TUBE_SEED, eps=S.TUBE_EPS, C=S.TUBE_C)
    X, t, n = p["X"], p["t"], p["n"]
    ub = np.full(2 * n, S.TUBE_C)
    r = S.oracle_smalxe(oracle, X, t, S.TUBE_EPS, np.zeros(n), ub)
    u = r["u"]
    print("oracle: reason", r["reason"], "outer/inner", r["iteration"], r["inner_iter_accu"], "max u", u.max(), "C", S.TUBE_C)
    assert r["reason"] == 2 and u.max() < 0.01 * S.TUBE_C
    w, b, free = S.np_model(X, t, S.TUBE_EPS, u, np.zeros(n), ub)
    assert free.sum() > 0 and np.array_equal(free, u > ASTOL)
    res = X @ w + b - t
    print("oracle: max |r|", np.abs(res).max(), "b", b)
    assert np.abs(res).max() <= S.TUBE_EPS + 1e-6 * np.linalg.norm(p["c"])


def test_few_samples_sit_on_the_edge_of_the_tube():
    """The n_in_tube check of the GPU tests leaves out the samples whose |r| - eps is within the rounding bound of a score.  On the data those tests score (the
    planted model standing in for the trained one: both have residuals of the noise's size), that bound is some 1e-14 and at most 1 % are left out."""
    for sparse, d in ((None, 64), ((12, 1.0), 200)):
        p = P.svr_linear(1500, d, 0.2, 9, sparse=sparse, n_test=1000)
        Xt, tt, w, b = p["X_test"], p["t_test"], p["w_true"], p["b_true"]
        sb = 2 * gamma(d + 1) * (abs(Xt) @ np.abs(w))
        r = Xt @ w + b - tt
        out = np.abs(np.abs(r) - 0.1) <= sb
        print("left out", int(out.sum()), "of", out.size, "score bound", sb.max())
        assert out.sum() <= 0.01 * out.size and (np.abs(r) <= 0.1).sum() > 100 and (np.abs(r) > 0.1).sum() > 100
