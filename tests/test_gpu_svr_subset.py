"""GPU tests of SVR sample subsets: the operator of csrc/svr.hip under pmh_op_svr_dual_set_subset (exact on integer data, against the doubled classification
operator under its own subset, to rounding on real data), held-out rows of X that never reach a sum, training on a subset against the CPU oracle, a fresh handle
on the subset's rows and numpy's restatement, the state a handle keeps, scoring the handle's own rows, and cross_validate on an SVR handle.  The bounds are those
of tests/test_gpu_svr.py, restated on the subset's rows."""
import math

import numpy as np
import pytest

import permon_amd as pa
from permon_amd import problems as P
from permon_amd._lib import PermonHipError
from permon_amd.svm import cross_validate
import svr_cases as S
import svr_subset_cases as SC
from svr_cases import ASTOL, EPS, gamma

pytestmark = pytest.mark.gpu
RTOL = 1e-6
OPTS = "-qps_rtol 1e-6"
STAT_FIELDS = [k for k, _ in pa._lib.SvrStats._fields_]


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


def _stats(st):
    return tuple(getattr(st, k) for k in STAT_FIELDS)


# ---- 1. the operator, exact -------------------------------------------------------------------------------------------------------------------------------------
def _exact(ctx, H, Hc, X, u, diag, m, tag):
    n = X.shape[0]
    mm = SC.doubled(m)
    H.set_subset(m)
    Hc.set_subset(mm)
    up = SC.poison(u, m, n)
    for kind in S.OP_TERMS:
        D, sigma = _set(H, n, kind, diag)
        _set(Hc, 2 * n, kind, np.concatenate([diag, diag]))
        got = _mult(ctx, H, u)
        assert np.array_equal(got, SC.apply_sub(X, u, D, sigma, m)), (tag, kind)
        assert np.array_equal(got, _mult(ctx, Hc, u)), (tag, kind)
        assert (got[~mm] == 0.0).all() and not np.signbit(got[~mm]).any(), (tag, kind)
        assert np.array_equal(_mult(ctx, H, up), got), (tag, kind)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", S.OP_N)
def test_operator_under_a_subset_is_exact_on_integer_data(n, dtype):
    """Integer data, powers of two: every sum is exact whatever its order, so the product == numpy's m^ o apply(X, m^ o u, D, sigma) with the sigma term over S,
    == the classification operator on vstack(X, X) with labels [+1; -1] under set_subset([m; m]); held-out rows are +0; NaN and 1e300 in the held-out entries of
    the operand change no bit."""
    ctx = pa.Context(0)
    yd = np.concatenate([np.ones(n), -np.ones(n)])
    m = SC.train_mask(n)
    for d in S.OP_D:
        X, u, diag = S.int_case(n, d, 1000 * n + d)
        H = pa.MatCreateSVRDual(ctx, X, sample_dtype=dtype)
        Hc = pa.MatCreateSVMDual(ctx, np.vstack([X, X]), yd, sample_dtype=dtype)
        _exact(ctx, H, Hc, X, u, diag, m, (n, d))
    ctx.close()


@pytest.mark.parametrize("empty", [0.0, 0.05])
def test_csr_operator_under_a_subset_is_exact_on_integer_data(empty):
    import scipy.sparse as sp

    ctx = pa.Context(0)
    n, d = 301, 200
    X, u, diag = S.int_case_csr(n, d, 12, empty, 77)
    H = pa.MatCreateSVRDual(ctx, X)
    Hc = pa.MatCreateSVMDual(ctx, sp.vstack([X, X]).tocsr(), np.concatenate([np.ones(n), -np.ones(n)]))
    _exact(ctx, H, Hc, X.toarray(), u, diag, SC.train_mask(n), "csr")
    ctx.close()


# ---- 2. the operator, real data ---------------------------------------------------------------------------------------------------------------------------------
def _op_bound(X, u, ref, sigma):
    """The component-wise bound of test_gpu_svr.py, restated: under a subset u is the masked operand, so every sum it bounds is at most as long."""
    n, d = X.shape
    aX = abs(X)
    s = np.abs(u[:n] - u[n:])
    row = aX @ (aX.T @ s)
    return 2 * (gamma(n + d + 3) * np.concatenate([row, row]) + sigma * gamma(n + 2) * s.sum() + 4 * EPS * np.abs(ref))


@pytest.mark.parametrize("kind", ["f64", "f32", "d37", "d130", "csr"])
def test_operator_under_a_subset_on_real_data(kind):
    ctx = pa.Context(0)
    n, d = {"f64": (2003, 64), "f32": (2003, 64), "d37": (301, 37), "d130": (500, 130), "csr": (1500, 300)}[kind]
    p = P.svr_linear(n, d, 0.1, n + d, sparse=(12, 1.0) if kind == "csr" else None)
    dt = np.float32 if kind == "f32" else None
    Xd = S.toarray(p["X"])
    Xs = Xd.astype(np.float32).astype(np.float64) if kind == "f32" else Xd  # the samples the operator holds
    r = np.random.default_rng(1)
    u, diag = r.uniform(0, 1, 2 * n), r.uniform(0.5, 2.0, n)
    m = SC.train_mask(n)
    mm = SC.doubled(m)
    H = pa.MatCreateSVRDual(ctx, p["X"], sample_dtype=dt)
    fresh = {}
    for tk in S.OP_TERMS:
        _set(H, n, tk, diag)
        fresh[tk] = _mult(ctx, H, u)
    for tk in S.OP_TERMS:
        D, sigma = _set(H, n, tk, diag)
        H.set_subset(m)
        p0 = H.passes()
        got = _mult(ctx, H, u)
        assert H.passes() == p0 + 2
        ref = SC.apply_sub(Xs, u, D, sigma, m)
        bound = _op_bound(Xs, SC.mask_operand(u, m), ref, sigma)
        err = np.abs(got - ref)
        print(kind, tk, "max err / bound", (err[mm] / bound[mm]).max())
        assert (err <= bound).all() and (got[~mm] == 0.0).all(), tk
        assert np.array_equal(got, _mult(ctx, H, u)) and np.array_equal(got, _mult(ctx, H, SC.poison(u, m))), tk
        # an all-ones mask: the SUB = 1 instances add only exact zeros in the same positions
        H.set_subset(np.ones(n))
        assert np.array_equal(_mult(ctx, H, u), fresh[tk]), tk
        # and without the subset again the bits of a fresh operator
        H.set_subset(None)
        assert np.array_equal(_mult(ctx, H, u), fresh[tk]), tk
    ctx.close()


# ---- 3. held-out rows of X never reach a sum ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,loss,bias,f32", [(64, "L1", True, False), (64, "L2", True, False), (37, "L1", True, False), (37, "L2", True, False), (130, "L1", True, False),
                                             (130, "L2", True, False), (64, "L2", True, True), (64, "L1", False, False)])
def test_held_out_rows_are_not_used(d, loss, bias, f32):
    """A handle whose X has NaN in the held-out rows trains to the bits of the handle on X: no load of a held-out row reaches a sum -- the operator's two
    passes, its pass 1 for w, and the bias pass, which visits the row but lets its dot product reach nothing (p_i = q_i = 0).  The NaN rows are written into
    the handle's device copy of X after create (whose eigenvalue estimate multiplies by the whole X); set_subset builds the solver anew over S."""
    n = 1500
    p = P.svr_linear(n, d, 0.05, 5, b_true=3.0 if bias else 0.0, C=0.1)
    X, t = p["X"], p["t"]
    m = SC.train_mask(n)
    Xn = X.copy()
    Xn[~m] = np.nan
    ctx = pa.Context(0)
    res = []
    for Xk in (X, Xn):
        svr = pa.SVR(ctx, loss=loss, C=0.1, epsilon=0.1, bias=bias, options=OPTS, sample_dtype=np.float32 if f32 else None).create(X, t)
        svr._keep[0].set_numpy(Xk.ravel())
        svr.set_subset(m).train()
        res.append((svr.alpha, svr.w, svr.b, _stats(svr.stats)))
        svr.destroy()
    (a1, w1, b1, s1), (a2, w2, b2, s2) = res
    print(d, loss, bias, f32, "outer/inner", s1[1], s1[2], "n_sv", s1[STAT_FIELDS.index("n_sv")])
    assert s1[0] == 2
    assert np.isfinite(a2).all() and np.isfinite(w2).all() and np.isfinite(b2) and np.isfinite(np.array(s2, dtype=float)).all()
    assert np.array_equal(a1, a2) and np.array_equal(w1, w2) and b1 == b2 and s1 == s2
    assert (a1[~SC.doubled(m)] == 0.0).all()
    ctx.close()


# ---- 4. training under a subset against independent answers ------------------------------------------------------------------------------------------------------
def _check_biased_on(st, u, w, b, X, t, eps, D, ub, tag):
    """_check_biased of test_gpu_svr.py on the subset's rows: X, t, D, ub and u = [p_S; q_S] are those of S, n is n_S."""
    n, d = X.shape
    c = np.concatenate([t - eps, -t - eps])
    e = np.concatenate([np.ones(n), -np.ones(n)])
    assert st.reason == 2
    assert u.min() >= -ASTOL and (ub is None or (u <= ub + ASTOL).all())
    thr = RTOL * np.linalg.norm(c)
    eq_round = 2 * gamma(2 * n) * np.abs(u).sum() / np.sqrt(2 * n)
    print(tag, "|e'u|/sqrt(2 n_S)", abs(e @ u) / np.sqrt(2 * n), "thr", thr, "+", eq_round, "sum_beta", st.sum_beta)
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
    print(tag, "|gP|", np.linalg.norm(gP), "thr", thr, "+ rounding", np.linalg.norm(er))
    assert np.linalg.norm(gP) <= kkt
    w_np, b_np, free = S.np_model(X, t, eps, u, D, ub)
    assert free.sum() > 0 and st.n_free_sv == free.sum() and st.n_sv == (u > ASTOL).sum()
    assert (np.abs(w - w_np) <= 2 * gamma(n + 1) * Wc).all()
    mag = np.concatenate([np.abs(t) + eps + D * u[:n], np.abs(t) + eps + D * u[n:]]) + np.concatenate([np.abs(X @ w_np)] * 2)
    db = S.b_bound(X, u, w_np, free, mag)
    print(tag, "b", b, "numpy", b_np, "bound", db, "multiplier", st.b_multiplier)
    assert abs(b - b_np) <= db and b == st.b_free
    nf = int(free.sum())
    assert abs(st.b_multiplier - st.b_free) <= kkt / np.sqrt(nf) + db


def _subset_fit(ctx, X, t, m, loss, bias, Cc, eps):
    svr = pa.SVR(ctx, loss=loss, C=Cc, epsilon=eps, bias=bias, options=OPTS + (" -qps_max_it 100" if bias else "")).create(X, t)
    assert svr.subset is None and svr.n_subset == m.size
    svr.set_subset(m).train()
    assert np.array_equal(svr.subset, m) and svr.n_subset == int(m.sum())
    u = svr.alpha
    assert (u[~SC.doubled(m)] == 0.0).all()
    return svr, u[SC.doubled(m)]


@pytest.mark.parametrize("loss", ["L1", "L2"])
@pytest.mark.parametrize("n,d", [(1500, 37), (2000, 64)])
def test_unbiased_training_under_a_subset(oracle, n, d, loss):
    """Without bias: the objective over S within 1e-6 relative of the CPU oracle's MPGP on X[m] and of a fresh handle on (X[m], t[m]), all solved to the same
    rtol (the margin of test_gpu_svr.py::test_unbiased_fit_is_the_qp_solve_and_matches_the_oracle).  Not bit for bit against the fresh handle: the rows sit in
    other waves there, so the summation groups differ."""
    ctx = pa.Context(0)
    eps, Cc = 0.1, 0.1
    p = P.svr_linear(n, d, 0.05, 5, eps=eps, C=Cc)
    X, t = p["X"], p["t"]
    m = SC.train_mask(n)
    Xs, ts, ns = X[m], t[m], int(m.sum())
    svr, us = _subset_fit(ctx, X, t, m, loss, False, Cc, eps)
    assert svr.stats.reason == 2 and svr.b == 0.0
    D = np.zeros(ns) if loss == "L1" else np.full(ns, 1.0 / Cc)
    ub = np.full(2 * ns, Cc) if loss == "L1" else None
    Xt = Xs.T

    def fn(v):
        z = Xs @ (Xt @ (v[:ns] - v[ns:]))
        return np.concatenate([z, -z]) + np.concatenate([D, D]) * v

    ref = oracle.mpgp(oracle.Op(2 * ns, fn=fn), np.concatenate([ts - eps, -ts - eps]), np.zeros(2 * ns), oracle.Box(2 * ns, lb=np.zeros(2 * ns), ub=ub), rtol=RTOL,
                      maxeig=2 * np.linalg.norm(Xs, 2) ** 2 + D.max())
    fresh = pa.SVR(ctx, loss=loss, C=Cc, epsilon=eps, bias=False, options=OPTS).fit(Xs, ts)
    f, fr, ff = S.objective(Xs, ts, eps, D, us), S.objective(Xs, ts, eps, D, ref["x"]), S.objective(Xs, ts, eps, D, fresh.alpha)
    print(n, d, loss, "objective", f, "oracle", fr, "rel", abs(f - fr) / abs(fr), "fresh", ff, "rel", abs(f - ff) / abs(ff))
    assert ref["reason"] == 2 and fresh.stats.reason == 2
    assert abs(f - fr) <= 1e-6 * abs(fr) and abs(f - ff) <= 1e-6 * abs(ff)
    assert (np.abs(svr.w - Xs.T @ (us[:ns] - us[ns:])) <= 2 * gamma(ns + 1) * (abs(Xs).T @ np.abs(us[:ns] - us[ns:]))).all()
    ctx.close()


@pytest.mark.parametrize("loss", ["L1", "L2"])
@pytest.mark.parametrize("n,d", [(1500, 37), (2000, 64)])
def test_biased_training_under_a_subset(n, d, loss):
    ctx = pa.Context(0)
    eps, Cc = 0.1, 0.1
    p = P.svr_linear(n, d, 0.05, 5, b_true=3.0, eps=eps, C=Cc)
    X, t = p["X"], p["t"]
    m = SC.train_mask(n)
    ns = int(m.sum())
    svr, us = _subset_fit(ctx, X, t, m, loss, True, Cc, eps)
    D = np.zeros(ns) if loss == "L1" else np.full(ns, 1.0 / Cc)
    _check_biased_on(svr.stats, us, svr.w, svr.b, X[m], t[m], eps, D, np.full(2 * ns, Cc) if loss == "L1" else None, (n, d, loss))
    assert abs(svr.b - 3.0) < 0.1  # (the planted b*)
    ctx.close()


def test_biased_training_under_a_subset_csr():
    ctx = pa.Context(0)
    n, d, eps, Cc = 1500, 300, 0.1, 1.0
    p = P.svr_linear(n, d, 0.05, 5, sparse=(12, 1.0), b_true=3.0, eps=eps, C=Cc)
    X, t = p["X"], p["t"]
    m = SC.train_mask(n)
    ns = int(m.sum())
    svr, us = _subset_fit(ctx, X, t, m, "L2", True, Cc, eps)
    _check_biased_on(svr.stats, us, svr.w, svr.b, X.toarray()[m], t[m], eps, np.full(ns, 1.0 / Cc), None, "csr")
    ctx.close()


# ---- 5. state ---------------------------------------------------------------------------------------------------------------------------------------------------
def _bits(svr):
    return svr.alpha, svr.w, svr.b, _stats(svr.stats)


def _same(a, b):
    # (b_free is NaN where no entry is free: equal where both are)
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and np.array_equal(np.array(a[3], dtype=float), np.array(b[3], dtype=float), equal_nan=True)


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("loss", ["L1", "L2"])
def test_state_under_a_subset(loss, bias):
    ctx = pa.Context(0)
    n = 600
    p = P.svr_linear(n, 37, 0.05, 5, b_true=3.0 if bias else 0.0, C=0.1)
    X, t = p["X"], p["t"]
    m = SC.train_mask(n)
    wt = np.random.default_rng(4).uniform(0.5, 2.0, n)
    mk = lambda e, c: pa.SVR(ctx, loss=loss, C=c, epsilon=e, bias=bias, options=OPTS)
    never = _bits(mk(0.1, 0.1).fit(X, t))
    svr = mk(0.3, 0.1).create(X, t).set_subset(m).train()
    # set_epsilon keeps the subset and refills the masked right-hand side
    svr.set_epsilon(0.1)
    with pytest.raises(PermonHipError, match="call pmh_svr_train first"):
        svr.w
    assert np.array_equal(svr.subset, m)
    fresh = _bits(mk(0.1, 0.1).create(X, t).set_subset(m).train())
    assert _same(_bits(svr.train()), fresh) and not _same(fresh, never)
    # all samples again: the bits of a handle that never had a subset
    svr.set_subset(None)
    assert svr.subset is None and svr.n_subset == n
    with pytest.raises(PermonHipError, match="call pmh_svr_train first"):
        svr.b
    assert _same(_bits(svr.train()), never)
    # set_penalties with weights keeps a subset too
    svr.set_subset(m).set_penalties(0.2, wt)
    assert np.array_equal(svr.subset, m)
    fresh_w = _bits(mk(0.1, 0.2).create(X, t, sample_weight=wt).set_subset(m).train())
    assert _same(_bits(svr.train()), fresh_w) and not _same(fresh_w, fresh)
    # refused masks leave a handle that still trains to the same bits
    for bad, word in ((np.where(np.arange(n) == 7, 0.5, 1.0), "1 entries of the mask are neither 0 nor 1"), (np.where(np.arange(n) < 2, np.nan, 1.0), "2 entries of the mask"),
                      (np.zeros(n), "holds no sample")):
        with pytest.raises(PermonHipError, match=word) as ei:
            svr.set_subset(bad)
        assert ei.value.code == 2
    with pytest.raises(ValueError, match="must have %d entries" % n):
        svr.set_subset(np.ones(n + 1))
    assert np.array_equal(svr.subset, m)
    assert np.array_equal(svr.w, fresh_w[1])  # (still trained: nothing changed)
    assert _same(_bits(svr.train()), fresh_w)
    ctx.close()


def test_refusals():
    ctx = pa.Context(0)
    p = P.svr_linear(301, 10, 0.1, 1)
    X, t = p["X"], p["t"]
    m = SC.train_mask(301)
    svr = pa.SVR(ctx, options=OPTS).create(X, t)
    with pytest.raises(PermonHipError, match="no subset is set") as ei:
        svr.test_own("held_out")
    assert ei.value.code == 3
    for which in ("subset", "all"):
        with pytest.raises(PermonHipError, match="call pmh_svr_train first") as ei:
            svr.test_own(which)
        assert ei.value.code == 3
    with pytest.raises(PermonHipError, match="call pmh_svr_train first"):
        svr.predict_own()
    svr.set_subset(m)
    with pytest.raises(PermonHipError, match="call pmh_svr_train first"):
        svr.test_own("held_out")
    # the operator's entry on a classification operator; the classification entry on the regression operator (pinned by test_gpu_svr.py too)
    Hc = pa.MatCreateSVMDual(ctx, X, np.ones(301))
    with pytest.raises(PermonHipError, match="not an operator of pmh_op_create_svr_dual") as ei:
        pa._lib.check(ctx.L.pmh_op_svr_dual_set_subset(Hc.h, ctx.vec_from(np.ones(301)).p))
    assert ei.value.code == 2
    H = pa.MatCreateSVRDual(ctx, X)
    with pytest.raises(ValueError, match="the operator has 301 samples"):
        H.set_subset(np.ones(602))
    u = np.random.default_rng(0).uniform(0, 1, 602)
    before = _mult(ctx, H, u)
    with pytest.raises(PermonHipError, match="3 entries of the mask are neither 0 nor 1"):
        H.set_subset(np.where(np.arange(301) < 3, 2.0, 1.0))
    assert np.array_equal(_mult(ctx, H, u), before)  # a refused mask leaves the operator as it was
    H.set_subset(m)
    sub = _mult(ctx, H, u)
    with pytest.raises(PermonHipError, match="holds no sample"):
        H.set_subset(np.zeros(301))
    assert np.array_equal(_mult(ctx, H, u), sub)
    ctx.close()


# ---- 6. the handle's own rows -------------------------------------------------------------------------------------------------------------------------------------
def _fsum(a):
    return math.fsum(a.tolist())


@pytest.fixture(scope="module", params=["f64", "f32", "d37", "csr"])
def own_case(request):
    kind = request.param
    ctx = pa.Context(0)
    eps = 0.1
    if kind == "csr":
        p = P.svr_linear(1500, 200, 0.2, 9, sparse=(12, 1.0), eps=eps, C=1.0)
    else:
        p = P.svr_linear(1500, 37 if kind == "d37" else 64, 0.2, 9, eps=eps, C=0.1)
    m = SC.train_mask(1500)
    svr = pa.SVR(ctx, loss="L2", C=p["C"], epsilon=eps, bias=True, options=OPTS, sample_dtype=np.float32 if kind == "f32" else None).create(p["X"], p["t"])
    svr.set_subset(m).train()
    X = p["X"].astype(np.float32) if kind == "f32" else p["X"]
    yield kind, svr, X, p["t"], m, eps
    svr.destroy()
    ctx.close()


def test_predict_own_is_predict(own_case):
    kind, svr, X, t, m, eps = own_case
    f = svr.predict_own()
    assert np.array_equal(f, svr.predict(X))
    Xd = S.toarray(X).astype(np.float64)
    sb = 2 * gamma(Xd.shape[1] + 1) * (np.abs(Xd) @ np.abs(svr.w))
    assert (np.abs(f - (Xd @ svr.w + svr.b)) <= sb).all()


@pytest.mark.parametrize("which", ["held_out", "subset", "all"])
def test_test_own_against_numpy(own_case, which):
    """The seven sums over the selected rows against exactly rounded sums of the library's own scores, each within gamma_k of the sum of its terms' magnitudes (k
    selected samples); max |r| and n exact; n_in_tube against numpy's count on the samples the score decides beyond its bound (_check_scoring of
    test_gpu_svr.py, restated)."""
    kind, svr, X, t, m, eps = own_case
    sel = {"held_out": ~m, "subset": m, "all": np.ones(m.size, bool)}[which]
    got = svr.test_own(which)
    k = int(sel.sum())
    assert got["n"] == k
    f = svr.predict_own()
    r, tt = (f - t)[sel], t[sel]
    gm = gamma(k)
    for key, terms in (("sum_r", r), ("sum_r2", r * r), ("sum_abs_r", np.abs(r)), ("sum_t", tt), ("sum_t2", tt * tt)):
        assert abs(got[key] - _fsum(terms)) <= gm * _fsum(np.abs(terms)), key
    assert got["max_abs"] == np.abs(r).max()
    assert got["mse"] == got["sum_r2"] / k and got["mae"] == got["sum_abs_r"] / k
    assert abs(got["r2"] - (1.0 - got["sum_r2"] / (got["sum_t2"] - got["sum_t"] ** 2 / k))) <= 4 * EPS
    Xd = S.toarray(X).astype(np.float64)
    sb = (2 * gamma(Xd.shape[1] + 1) * (np.abs(Xd) @ np.abs(svr.w)))[sel]
    r_np = (Xd @ svr.w + svr.b - t)[sel]
    sure = np.abs(np.abs(r_np) - eps) > sb
    out = int((~sure).sum())
    cnt = int(((np.abs(r_np) <= eps) & sure).sum())
    print(kind, which, "n_in_tube", got["n_in_tube"], "numpy on the sure samples", cnt, "left out", out)
    assert out <= 0.01 * k and cnt <= got["n_in_tube"] <= cnt + out and 0 < cnt < k
    if which == "all":
        assert got == svr.test(X, t)


# ---- 7. cross_validate ----------------------------------------------------------------------------------------------------------------------------------------------
def test_cross_validate():
    ctx = pa.Context(0)
    n, k = 600, 3
    p = P.svr_linear(n, 37, 0.2, 9, eps=0.1, C=0.1)
    X, t = p["X"], p["t"]
    before = SC.train_mask(n)
    mk = lambda: pa.SVR(ctx, loss="L2", C=0.1, epsilon=0.1, bias=True, options=OPTS).create(X, t)
    svr = mk().set_subset(before).train()
    out = cross_validate(svr, k=k, seed=3)
    masks = pa.svm.kfold(t, k, 3, stratified=False)
    assert len(out["masks"]) == k and all(np.array_equal(a, b) for a, b in zip(out["masks"], masks))
    assert (np.sum([~mk_ for mk_ in out["masks"]], axis=0) == 1).all()  # the complements partition the rows
    # the handle gets back the subset it had and is left untrained
    assert np.array_equal(svr.subset, before)
    with pytest.raises(PermonHipError, match="call pmh_svr_train first"):
        svr.w
    # the hand-written loop on another handle, bit for bit
    other = mk()
    hand = [other.set_subset(mk_).train().test_own("held_out") for mk_ in masks]
    assert out["folds"] == hand
    assert [f["n"] for f in hand] == [int((~mk_).sum()) for mk_ in masks] and sum(f["n"] for f in hand) == n
    pooled = SC.pooled(hand)
    print("pooled", pooled)
    assert {key: out[key] for key in pooled} == pooled
    assert 0.0 < out["mse"] < np.var(t) and out["r2"] > 0.5
    # stratified does not apply to an SVR handle
    assert cross_validate(svr, k=k, seed=3, stratified=False)["folds"] == hand
    ctx.close()
