"""GPU tests of support vector regression: the dual operator of csrc/svr.hip (exact on integer data, against the doubled classification operator, to rounding on
real data, its accounting), training with and without bias against the QP interface, the CPU oracle and numpy's restatement (tests/svr_cases.py), the model,
prediction, the regression metrics, set_epsilon / set_penalties and the refusals."""
import math

import numpy as np
import pytest

import permon_amd as pa
from permon_amd import problems as P
from permon_amd._lib import PermonHipError
import svr_cases as S
from svr_cases import ASTOL, EPS, gamma

pytestmark = pytest.mark.gpu
RTOL = 1e-6
OPTS = "-qps_rtol 1e-6"


def _mult(ctx, op, u):
    out = ctx.vec(u.size)
    op.mult(ctx.vec_from(u), out)
    return out.to_numpy()


def _set(op, n, kind, diag):
    """The terms `kind` of S.OP_TERMS on an operator; returns D (n) and sigma."""
    shift, use_diag, sigma = S.OP_TERMS[kind]
    op.set_diag(None)
    op.set_terms(shift, sigma)
    if use_diag:
        op.set_diag(diag)
    return S.D_of(n, shift, diag if use_diag else None), sigma


# ---- 1. the operator, exact -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", S.OP_N)
def test_operator_is_exact_on_integer_data(n, dtype):
    """X in {-3..3}, p, q in {0..4}, sigma and the diagonal powers of two: every sum is exact in fp64 whatever its order, so the product == numpy's H^ u, for
    every d (the generic layout, d = 64's own, the widths around it, the widest) and every form of the terms -- and == the classification operator of
    MatCreateSVMDual on vstack(X, X) with labels [+1; -1]."""
    ctx = pa.Context(0)
    yd = np.concatenate([np.ones(n), -np.ones(n)])
    for d in S.OP_D:
        X, u, diag = S.int_case(n, d, 1000 * n + d)
        H = pa.MatCreateSVRDual(ctx, X, sample_dtype=dtype)
        Hc = pa.MatCreateSVMDual(ctx, np.vstack([X, X]), yd, sample_dtype=dtype)
        for kind in S.OP_TERMS:
            D, sigma = _set(H, n, kind, diag)
            _set(Hc, 2 * n, kind, np.concatenate([diag, diag]))
            got = _mult(ctx, H, u)
            assert np.array_equal(got, S.apply(X, u, D, sigma)), (n, d, kind)
            assert np.array_equal(got, _mult(ctx, Hc, u)), (n, d, kind)
    ctx.close()


@pytest.mark.parametrize("empty", [0.0, 0.05])
def test_csr_operator_is_exact_on_integer_data(empty):
    ctx = pa.Context(0)
    n, d = 300, 200
    X, u, diag = S.int_case_csr(n, d, 12, empty, 77)
    assert ((np.diff(X.indptr) == 0).sum() > 0) == (empty > 0)
    H = pa.MatCreateSVRDual(ctx, X)
    Xd = X.toarray()
    import scipy.sparse as sp

    Hc = pa.MatCreateSVMDual(ctx, sp.vstack([X, X]).tocsr(), np.concatenate([np.ones(n), -np.ones(n)]))
    for kind in S.OP_TERMS:
        D, sigma = _set(H, n, kind, diag)
        _set(Hc, 2 * n, kind, np.concatenate([diag, diag]))
        got = _mult(ctx, H, u)
        assert np.array_equal(got, S.apply(Xd, u, D, sigma)), kind
        assert np.array_equal(got, _mult(ctx, Hc, u)), kind
    ctx.close()


# ---- 2. the operator, real data ---------------------------------------------------------------------------------------------------------------------------------
def _op_bound(X, u, ref, sigma):
    """The component-wise bound of test_gpu_svm_train.py::test_augmented_operator_against_numpy with one more rounding for s_i = p_i - q_i."""
    n, d = X.shape
    aX = abs(X)
    s = np.abs(u[:n] - u[n:])
    row = aX @ (aX.T @ s)
    return 2 * (gamma(n + d + 3) * np.concatenate([row, row]) + sigma * gamma(n + 2) * s.sum() + 4 * EPS * np.abs(ref))


@pytest.mark.parametrize("n,d", [(3000, 64), (1111, 37), (500, 130)])
def test_operator_against_numpy_on_real_data(n, d):
    ctx = pa.Context(0)
    p = P.svr_linear(n, d, 0.1, n + d)
    X = p["X"]
    r = np.random.default_rng(1)
    u, diag = r.uniform(0, 1, 2 * n), r.uniform(0.5, 2.0, n)
    H = pa.MatCreateSVRDual(ctx, X)
    fresh = _mult(ctx, H, u)
    H32 = pa.MatCreateSVRDual(ctx, X, sample_dtype=np.float32)
    Hw = pa.MatCreateSVRDual(ctx, X.astype(np.float32).astype(np.float64))  # the fp64 operator on the widened samples
    for kind in S.OP_TERMS:
        D, sigma = _set(H, n, kind, diag)
        got = _mult(ctx, H, u)
        ref = S.apply(X, u, D, sigma)
        bound = _op_bound(X, u, ref, sigma)
        err = np.abs(got - ref)
        print(n, d, kind, "max err / bound", (err / bound).max())
        assert (err <= bound).all(), kind
        assert np.array_equal(got, _mult(ctx, H, u))  # two calls, equal bits
        _set(H32, n, kind, diag), _set(Hw, n, kind, diag)
        g32 = _mult(ctx, H32, u)
        if d != 64:
            assert np.array_equal(g32, _mult(ctx, Hw, u)), kind
        else:  # a layout of its own: to rounding, on the samples it holds
            X32 = X.astype(np.float32).astype(np.float64)
            r32 = S.apply(X32, u, D, sigma)
            assert (np.abs(g32 - r32) <= _op_bound(X32, u, r32, sigma)).all(), kind
            assert np.array_equal(g32, _mult(ctx, H32, u))
    # terms set back to zero: the bits of a fresh operator
    _set(H, n, "plain", diag)
    assert np.array_equal(_mult(ctx, H, u), fresh)
    ctx.close()


def test_csr_operator_against_numpy_on_real_data():
    ctx = pa.Context(0)
    n, d = 700, 200
    p = P.svr_linear(n, d, 0.1, 3, sparse=(12, 1.0))
    X, Xd = p["X"], p["X"].toarray()
    r = np.random.default_rng(2)
    u, diag = r.uniform(0, 1, 2 * n), r.uniform(0.5, 2.0, n)
    H = pa.MatCreateSVRDual(ctx, X)
    fresh = _mult(ctx, H, u)
    for kind in S.OP_TERMS:
        D, sigma = _set(H, n, kind, diag)
        got = _mult(ctx, H, u)
        ref = S.apply(Xd, u, D, sigma)
        assert (np.abs(got - ref) <= _op_bound(Xd, u, ref, sigma)).all(), kind
        assert np.array_equal(got, _mult(ctx, H, u))
    _set(H, n, "plain", diag)
    assert np.array_equal(_mult(ctx, H, u), fresh)
    ctx.close()


# ---- 3. accounting ----------------------------------------------------------------------------------------------------------------------------------------------
def test_passes_and_memory():
    """passes rises by 2 per product, dense and CSR.  Dense: creation allocates nothing of the size of X (the labels of the doubled problem, 16 n bytes, w and
    one partial row per workgroup).  CSR: creation takes ONE column-ordered copy, 12 (nnz + n) bytes, plus 6 n-vectors of doubles (the header's list), the
    sweeps' tables (20 bytes per span of 2048 entries, two tables) and the copy's pointer array -- not twice the copy.  The device allocator hands memory out in
    granules of up to 2 MiB, so each of the 16 allocations may show up to that much more in pmh_mem_info: 32 MiB of slack, against a copy of 75 MB."""
    import ctypes as C
    import scipy.sparse as sp

    check = pa._lib.check
    ctx = pa.Context(0)
    n, d = 200000, 64
    Xd = ctx.vec_from(np.random.default_rng(0).standard_normal(n * d))  # (X itself, as the operator borrows it: allocated before the measurement)
    u, out = ctx.vec_from(np.ones(2 * n)), ctx.vec(2 * n)
    f0 = ctx.mem_info()[0]
    h = C.c_void_p()
    check(ctx.L.pmh_op_create_svr_dual(ctx.h, n, d, Xd.p, C.byref(h)))
    used = f0 - ctx.mem_info()[0]
    print("dense: X is", 8 * n * d, "bytes; creation took", used)
    assert used <= 8 * n * d // 8
    H = pa.Op(ctx, h, 2 * n)
    k = C.c_longlong()
    for j in range(3):
        H.mult(u, out)
        check(ctx.L.pmh_op_svr_dual_passes(h, C.byref(k)))
        assert k.value == 2 * (j + 1)
    ns, ds, per = 300000, 5000, 20
    r = np.random.default_rng(1)
    Xs = sp.csr_matrix((r.standard_normal(ns * per), (np.repeat(np.arange(ns), per), r.integers(0, ds, ns * per))), shape=(ns, ds))
    Xs.sum_duplicates()
    Xs.sort_indices()
    nnz = Xs.nnz
    Xc = pa.mat.csr_from_scipy(ctx, Xs)
    us, outs = ctx.vec_from(np.ones(2 * ns)), ctx.vec(2 * ns)
    f0 = ctx.mem_info()[0]
    hs = C.c_void_p()
    check(ctx.L.pmh_op_create_svr_dual_csr(ctx.h, Xc.h, C.byref(hs)))
    used = f0 - ctx.mem_info()[0]
    spans = (nnz + ns) // 2048 + 2
    allowed = 12 * (nnz + ns) + 6 * 8 * ns + 2 * 20 * spans + 12 * (ds + 2) + (32 << 20)
    print("CSR: 12 (nnz + n) =", 12 * (nnz + ns), "creation took", used, "allowed", allowed)
    assert allowed < 2 * 12 * (nnz + ns) and used <= allowed
    Hs = pa.Op(ctx, hs, 2 * ns)
    for j in range(3):
        Hs.mult(us, outs)
        check(ctx.L.pmh_op_svr_dual_passes(hs, C.byref(k)))
        assert k.value == 2 * (j + 1)
    ctx.close()


# ---- 4. training without bias -----------------------------------------------------------------------------------------------------------------------------------
def _qp_solve(ctx, p, loss):
    """The QP interface on MatCreateSVRDual with right-hand side c^ and the box, rtol 1e-6 (svm_train_cases.solve for SVM)."""
    H = pa.MatCreateSVRDual(ctx, p["X"])
    if loss == "L2":
        H.set_terms(1.0 / p["C"], 0.0)
    qp = pa.QP(ctx)
    qp.SetOperator(H)
    qp.SetRhs(ctx.vec_from(p["c"]))
    x = ctx.vec_from(p["x0"])
    qp.SetInitialVector(x)
    qp.SetBox(None, ctx.vec_from(p["lb"]), ctx.vec_from(p["ub"]) if loss == "L1" else None)
    qps = pa.QPS(ctx)
    qps.SetQP(qp)
    qps.SetType("mpgp")
    qps.SetTolerances(rtol=RTOL)
    st = qps.Solve()
    return st, x.to_numpy()


@pytest.mark.parametrize("loss", ["L1", "L2"])
@pytest.mark.parametrize("n,d", [(1500, 37), (2000, 64)])
def test_unbiased_fit_is_the_qp_solve_and_matches_the_oracle(oracle, n, d, loss):
    ctx = pa.Context(0)
    p = P.svr_linear(n, d, 0.05, 5, eps=0.1, C=0.1)
    X, t, Cc = p["X"], p["t"], p["C"]
    st, x = _qp_solve(ctx, p, loss)
    svr = pa.SVR(ctx, loss=loss, C=Cc, epsilon=0.1, bias=False, options=OPTS).fit(X, t)
    s = svr.stats
    print(n, d, loss, "iterations", s.inner_iterations, "nmv", s.nmv, "reason", s.reason)
    assert s.reason == 2 and np.array_equal(svr.alpha, x)
    assert (s.inner_iterations, s.nmv, s.ncg, s.nexp, s.nprop, s.reason) == (st.iteration, st.nmv, st.ncg, st.nexp, st.nprop, st.reason)
    assert svr.b == 0.0 and np.array_equal(svr.beta, x[:n] - x[n:])
    D = np.zeros(n) if loss == "L1" else np.full(n, 1.0 / Cc)
    ub = p["ub"] if loss == "L1" else None
    # (the oracle's power method starts from all ones, an eigenvector of H^'s smallest eigenvalue; it is given the bound 2 |X|_2^2 + max D instead)
    Xt = X.T

    def fn(v):
        z = X @ (Xt @ (v[:n] - v[n:]))
        return np.concatenate([z, -z]) + np.concatenate([D, D]) * v

    ref = oracle.mpgp(oracle.Op(2 * n, fn=fn), p["c"], p["x0"], oracle.Box(2 * n, lb=p["lb"], ub=ub), rtol=RTOL, maxeig=2 * np.linalg.norm(X, 2) ** 2 + D.max())
    f, fr = S.objective(X, t, 0.1, D, x), S.objective(X, t, 0.1, D, ref["x"])
    print(n, d, loss, "objective", f, "oracle", fr, "rel", abs(f - fr) / abs(fr), "oracle iterations", ref["iteration"])
    assert ref["reason"] == 2 and abs(f - fr) <= 1e-6 * abs(fr)
    ctx.close()


# ---- 5. training with bias ----------------------------------------------------------------------------------------------------------------------------------------
def _check_biased(svr, X, t, eps, D, ub, loss):
    """From the returned dual alone (items 5 and 6 of test_gpu_svm_train.py::test_biased_training_against_the_oracle, restated for u = [p; q]).  Returns the
    KKT threshold with its rounding, and numpy's model."""
    n, d = X.shape
    st, u = svr.stats, svr.alpha
    c = np.concatenate([t - eps, -t - eps])
    e = np.concatenate([np.ones(n), -np.ones(n)])
    assert st.reason == 2
    assert u.min() >= -ASTOL and (ub is None or (u <= ub + ASTOL).all())
    # SMALXE stops when max(|B u|, |gP|) <= rtol |c^| =: thr, B u = e'u / sqrt(2n), gP the projected gradient of 1/2 u'H^u - c^'u + mu (e / sqrt(2n))'u at
    # mu = b_multiplier sqrt(2n), i.e. g = H^u - c^ + b_multiplier e.  Recomputing in numpy repeats the sums: item 1's bound on either side
    thr = RTOL * np.linalg.norm(c)
    eq_round = 2 * gamma(2 * n) * np.abs(u).sum() / np.sqrt(2 * n)
    print(loss, "|e'u|/sqrt(2n)", abs(e @ u) / np.sqrt(2 * n), "thr", thr, "+", eq_round, "sum_beta", st.sum_beta)
    assert abs(e @ u) / np.sqrt(2 * n) <= thr + eq_round
    assert abs(st.sum_beta - e @ u) <= 2 * gamma(2 * n) * np.abs(u).sum()
    g = S.apply(X, u, D) - c + st.b_multiplier * e
    aX = abs(X)
    Wc = aX.T @ np.abs(u[:n] - u[n:])
    row = aX @ Wc
    er = 2 * gamma(n + d + 3) * np.concatenate([row, row]) + 4 * EPS * (np.abs(g) + np.abs(c)) + EPS * abs(st.b_multiplier)
    lo, hi = u <= ASTOL, (u >= ub - ASTOL) if ub is not None else np.zeros(2 * n, bool)
    gP = np.where(lo, np.minimum(g, 0.0), np.where(hi, np.maximum(g, 0.0), g))
    kkt = thr + np.linalg.norm(er)
    print(loss, "|gP|", np.linalg.norm(gP), "thr", thr, "+ rounding", np.linalg.norm(er))
    assert np.linalg.norm(gP) <= kkt
    # the model
    w_np, b_np, free = S.np_model(X, t, eps, u, D, ub)
    assert free.sum() > 0 and st.n_free_sv == free.sum() and st.n_sv == (u > ASTOL).sum()
    assert (np.abs(svr.w - w_np) <= 2 * gamma(n + 1) * Wc).all()
    mag = np.concatenate([np.abs(t) + eps + D * u[:n], np.abs(t) + eps + D * u[n:]]) + np.concatenate([np.abs(X @ w_np)] * 2)
    db = S.b_bound(X, u, w_np, free, mag)
    print(loss, "b", svr.b, "numpy", b_np, "bound", db, "multiplier", st.b_multiplier)
    assert abs(svr.b - b_np) <= db and svr.b == st.b_free
    # in a free entry (b_free's term) - b_multiplier = -+g_k, so the mean over the nf free entries differs from b_multiplier by at most |gP| / sqrt(nf)
    # (Cauchy-Schwarz) plus the rounding of the mean itself
    nf = int(free.sum())
    assert abs(st.b_multiplier - st.b_free) <= kkt / np.sqrt(nf) + db
    return kkt, w_np, b_np, db


@pytest.mark.parametrize("loss", ["L1", "L2"])
def test_biased_training(loss):
    ctx = pa.Context(0)
    n, d, eps, Cc = 1500, 64, 0.1, 0.1
    p = P.svr_linear(n, d, 0.05, 5, b_true=3.0, eps=eps, C=Cc)
    X, t = p["X"], p["t"]
    svr = pa.SVR(ctx, loss=loss, C=Cc, epsilon=eps, bias=True, options=OPTS + " -qps_max_it 100").fit(X, t)
    st = svr.stats
    print(loss, "outer/inner", st.outer_iterations, st.inner_iterations, "passes", st.passes_X, "nmv", st.nmv)
    D = np.zeros(n) if loss == "L1" else np.full(n, 1.0 / Cc)
    _check_biased(svr, X, t, eps, D, p["ub"] if loss == "L1" else None, loss)
    assert abs(svr.b - 3.0) < 0.1  # (the planted b*)
    ctx.close()


def test_biased_training_with_sample_weights_needs_the_diagonal_in_b():
    """L2 with unequal C_i = C weight_i: b_free's terms carry D_i p_i and D_i q_i, which no longer cancel in the mean.  numpy's restatement without them differs
    from the one with them by more than the bound (asserted first); the library agrees with the one that has them."""
    ctx = pa.Context(0)
    n, d, eps, Cc = 1500, 64, 0.1, 0.1
    p = P.svr_linear(n, d, 0.05, 5, b_true=3.0, eps=eps, C=Cc)
    X, t = p["X"], p["t"]
    # heavier penalties where the target lies above the plane's offset: the p side and the q side then see different D_i
    wt = np.where(t > 3.0, 8.0, 0.125)
    svr = pa.SVR(ctx, loss="L2", C=Cc, epsilon=eps, bias=True, options=OPTS + " -qps_max_it 100").fit(X, t, sample_weight=wt)
    D = 1.0 / (Cc * wt)
    _, w_np, b_np, db = _check_biased(svr, X, t, eps, D, None, "L2 weighted")
    b_without = S.np_model(X, t, eps, svr.alpha, D, None, with_D=False)[1]
    print("b with D", b_np, "without", b_without, "bound", db)
    assert abs(b_without - b_np) > 100 * db
    assert abs(svr.b - b_without) > db
    ctx.close()


# ---- 6. what the model is for -------------------------------------------------------------------------------------------------------------------------------------
def test_noise_free_residuals_stay_in_the_tube():
    """Noise-free data, eps = 0.05, C = TUBE_C (no entry of the oracle's solution at its bound: test_svr_host.py).  With p_i, q_i below C the projected gradient
    of an entry is min(g_k, 0) or g_k, so g_p[i] = r_i + eps >= -|gP| and g_q[i] = -r_i + eps >= -|gP| with r_i the residual at b_multiplier: |r_i| <= eps +
    |gP|, and |gP| obeys the stopping threshold plus its recomputation's rounding (kkt).  The model uses b_free: + |b_free - b_multiplier|; numpy's residual
    repeats the score: + the score's bound."""
    ctx = pa.Context(0)
    p = P.svr_linear(S.TUBE_N, S.TUBE_D, 0.0, S.TUBE_SEED, eps=S.TUBE_EPS, C=S.TUBE_C)
    X, t, n = p["X"], p["t"], p["n"]
    svr = pa.SVR(ctx, loss="L1", C=S.TUBE_C, epsilon=S.TUBE_EPS, bias=True, options=OPTS + " -qps_max_it 100").fit(X, t)
    ub = np.full(2 * n, S.TUBE_C)
    kkt, w_np, b_np, db = _check_biased(svr, X, t, S.TUBE_EPS, np.zeros(n), ub, "tube")
    assert svr.alpha.max() < S.TUBE_C - ASTOL
    st = svr.stats
    r = X @ svr.w + svr.b - t
    sb = 2 * gamma(S.TUBE_D + 1) * (abs(X) @ np.abs(svr.w) + abs(svr.b))
    thr = kkt + abs(st.b_free - st.b_multiplier)
    print("max |r|", np.abs(r).max(), "eps", S.TUBE_EPS, "thr", thr)
    assert (np.abs(r) <= S.TUBE_EPS + thr + sb).all()
    assert np.abs(r).max() > 0.9 * S.TUBE_EPS  # (the tube is used: this is not the least-squares fit)
    ctx.close()


def test_bias_lowers_the_held_out_error():
    ctx = pa.Context(0)
    p = P.svr_linear(1500, 64, 0.2, 9, b_true=3.0, eps=0.1, C=0.1, n_test=1000)
    with_b = pa.SVR(ctx, loss="L2", C=0.1, epsilon=0.1, bias=True, options=OPTS).fit(p["X"], p["t"]).test(p["X_test"], p["t_test"])
    flat = pa.SVR(ctx, loss="L2", C=0.1, epsilon=0.1, bias=False, options=OPTS).fit(p["X"], p["t"]).test(p["X_test"], p["t_test"])
    print("held-out mse with bias", with_b["mse"], "without", flat["mse"])
    assert with_b["mse"] < flat["mse"] and with_b["mse"] < 0.1
    ctx.close()


# ---- 7. predict and test ------------------------------------------------------------------------------------------------------------------------------------------
def _fsum(a):
    return math.fsum(a.tolist())


def _check_scoring(svr, Xt, tt, eps):
    """predict against numpy within the dot product's bound; the seven sums of test against exactly rounded sums of the library's own scores, each within gamma_m of
    the sum of its terms' magnitudes (m test samples: what any order of summation obeys); max |r| exact; n_in_tube against numpy's count on the samples the
    score decides beyond its bound."""
    Xd = S.toarray(Xt)
    m, d = Xd.shape
    w, b = svr.w, svr.b
    f = svr.predict(Xt)
    ref = Xd @ w + b
    sb = 2 * gamma(d + 1) * (np.abs(Xd) @ np.abs(w))
    print("predict: max err / bound", (np.abs(f - ref) / sb).max())
    assert (np.abs(f - ref) <= sb).all()
    got = svr.test(Xt, tt)
    r = f - tt
    gm = gamma(m)
    for key, terms in (("sum_r", r), ("sum_r2", r * r), ("sum_abs_r", np.abs(r)), ("sum_t", tt), ("sum_t2", tt * tt)):
        assert abs(got[key] - _fsum(terms)) <= gm * _fsum(np.abs(terms)), key
    assert got["max_abs"] == np.abs(r).max() and got["n"] == m
    assert got["mse"] == got["sum_r2"] / m and got["mae"] == got["sum_abs_r"] / m
    assert abs(got["r2"] - (1.0 - got["sum_r2"] / (got["sum_t2"] - got["sum_t"] ** 2 / m))) <= 4 * EPS
    r_np = ref - tt
    sure = np.abs(np.abs(r_np) - eps) > sb
    out = int((~sure).sum())
    cnt = int(((np.abs(r_np) <= eps) & sure).sum())
    print("n_in_tube", got["n_in_tube"], "numpy on the sure samples", cnt, "left out", out)
    assert out <= 0.01 * m and cnt <= got["n_in_tube"] <= cnt + out and 0 < cnt < m
    return f


@pytest.mark.parametrize("kind", ["f64", "f32", "d37", "csr"])
def test_predict_and_test(kind):
    ctx = pa.Context(0)
    eps = 0.1
    if kind == "csr":
        p = P.svr_linear(1500, 200, 0.2, 9, sparse=(12, 1.0), eps=eps, C=1.0, n_test=1000)
    else:
        p = P.svr_linear(1500, 37 if kind == "d37" else 64, 0.2, 9, eps=eps, C=0.1, n_test=1003)
    svr = pa.SVR(ctx, loss="L2", C=p["C"], epsilon=eps, bias=True, options=OPTS, sample_dtype=np.float32 if kind == "f32" else None).fit(p["X"], p["t"])
    Xt = p["X_test"].astype(np.float32) if kind == "f32" else p["X_test"]
    f = _check_scoring(svr, Xt, p["t_test"], eps)
    if kind == "csr":  # a CSR-trained model of d <= 256 on dense test samples
        fd = _check_scoring(svr, Xt.toarray(), p["t_test"], eps)
        assert (np.abs(fd - f) <= 2 * gamma(201) * (np.abs(Xt.toarray()) @ np.abs(svr.w))).all()
    if kind == "d37":  # and the reverse: a dense-trained model on CSR test samples
        import scipy.sparse as sp

        _check_scoring(svr, sp.csr_matrix(Xt), p["t_test"], eps)
    ctx.close()


# ---- 8. set_epsilon and set_penalties -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("loss", ["L1", "L2"])
def test_set_epsilon_and_set_penalties_give_a_fresh_handles_bits(loss, bias):
    ctx = pa.Context(0)
    n = 600
    p = P.svr_linear(n, 37, 0.05, 5, b_true=3.0 if bias else 0.0, C=0.1)
    X, t = p["X"], p["t"]
    wt = np.random.default_rng(4).uniform(0.5, 2.0, n)
    mk = lambda e, c: pa.SVR(ctx, loss=loss, C=c, epsilon=e, bias=bias, options=OPTS)
    svr = mk(0.3, 0.1).fit(X, t)
    fresh = mk(0.1, 0.1).fit(X, t)
    svr.set_epsilon(0.1)
    with pytest.raises(PermonHipError, match="call pmh_svr_train first"):  # untrained afterwards
        svr.w
    svr.train()
    assert np.array_equal(svr.alpha, fresh.alpha) and np.array_equal(svr.w, fresh.w) and svr.b == fresh.b and svr.stats.nmv == fresh.stats.nmv
    fresh_w = mk(0.1, 0.2).create(X, t, sample_weight=wt).train()
    svr.set_penalties(0.2, wt)
    with pytest.raises(PermonHipError, match="call pmh_svr_train first"):
        svr.b
    svr.train()
    assert np.array_equal(svr.alpha, fresh_w.alpha) and np.array_equal(svr.w, fresh_w.w) and svr.b == fresh_w.b
    assert not np.array_equal(fresh_w.alpha, fresh.alpha)
    ctx.close()


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    ctx = pa.Context(0)
    p = P.svr_linear(300, 10, 0.1, 1)
    X, t = p["X"], p["t"]
    for e, word in ((-0.5, "epsilon = -0.5"), (float("nan"), "epsilon = nan"), (float("inf"), "epsilon = inf")):
        with pytest.raises(PermonHipError, match=word) as ei:
            pa.SVR(ctx, epsilon=e).create(X, t)
        assert ei.value.code == 2
    for c in (0.0, -2.0):
        with pytest.raises(PermonHipError, match="C = %g" % c) as ei:
            pa.SVR(ctx, C=c).create(X, t)
        assert ei.value.code == 2
    tb = t.copy()
    tb[[3, 77, 200]] = [np.nan, np.inf, -np.inf]
    with pytest.raises(PermonHipError, match="3 of the targets are not finite") as ei:
        pa.SVR(ctx).create(X, tb)
    assert ei.value.code == 2
    svr = pa.SVR(ctx, options=OPTS).create(X, t)
    with pytest.raises(PermonHipError, match="call pmh_svr_train first") as ei:
        svr.w
    assert ei.value.code == 3
    with pytest.raises(PermonHipError, match="call pmh_svr_train first"):
        svr.predict(X)
    with pytest.raises(PermonHipError, match="epsilon = -1"):
        svr.set_epsilon(-1.0)
    with pytest.raises(PermonHipError, match="C = 0"):
        svr.set_penalties(0.0)
    wt = np.ones(300)
    wt[[1, 2]] = [0.0, np.nan]
    with pytest.raises(PermonHipError, match="2 of the sample weights are not positive and finite"):
        svr.set_penalties(1.0, wt)
    svr.train()  # (the refusals left the handle usable)
    assert svr.stats.reason == 2
    # the operator: the limits and the refusal of the classification operator, a shift against a diagonal, what the doubled operator does not take
    with pytest.raises(PermonHipError) as ei:
        pa.MatCreateSVRDual(ctx, np.zeros((4, 257)))
    assert ei.value.code == 2
    H = pa.MatCreateSVRDual(ctx, X)
    H.set_terms(0.5, 0.0)
    with pytest.raises(PermonHipError, match="a scalar shift or a diagonal, not both"):
        H.set_diag(np.ones(300))
    with pytest.raises(PermonHipError, match="takes no sample subset"):
        pa._lib.check(ctx.L.pmh_op_svm_dual_set_subset(H.h, ctx.vec_from(np.ones(600)).p))
    with pytest.raises(PermonHipError, match="not an operator of pmh_op_create_svr_dual"):
        pa._lib.check(ctx.L.pmh_op_svr_dual_set_terms(pa.MatCreateSVMDual(ctx, X, np.ones(300)).h, 0.0, 0.0))
    ctx.close()
