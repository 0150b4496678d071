"""GPU tests of the SVM front end: the one-row projector (the MATONEROW role), the SVM dual operator's diagonal shift and rank-one term, the penalised operator that
folds the bias equality into it, training with and without bias against the CPU oracle, the model, prediction and the cost of the bias term in passes over X."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import permon_amd as pa
from permon_amd import _lib
from permon_amd import problems as P
from permon_amd._lib import check
from svm_train_cases import ASTOL, EPS, gamma, check_counts as _check_counts, np_model as _np_model, oracle_train as _oracle_train, solve as _solve

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the one-row projector against the same row as a 1 x n CSR ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,kind", [(4000, "unit"), (1037, "zeros"), (70001, "general")])
def test_onerow_projector_equals_the_csr_projector(n, kind):
    """Both sides evaluate s = a'v in floating point, in different orders: each is within gamma_n S, S = sum |a_i v_i|, of the exact value, so they differ by at most
    2 gamma_n S =: D (n + 2 would cover the rounding of the products' own scaling; n >> 2).  Through each formula, with t = a'a (both sides sum it too: relative
    error gamma_n each) and three more roundings per entry for the scaling, the subtraction and the division:
      G v      = s                 |diff| <= D
      G'G v    = s a_i             |diff| <= (D + 3 eps |s|) |a_i|
      halfQ v  = s / t             |diff| <= (D + (2 gamma_n + 3 eps) |s|) / t
      Q v      = (s / t) a_i       |diff| <= (D + (2 gamma_n + 3 eps) |s|) |a_i| / t
      P v      = v_i - (Q v)_i     the bound of Q v plus eps (|v_i| + |Q v|_i) for the subtraction on either side
      CP x     = x / t             |diff| <= (2 gamma_n + 3 eps) |x| / t
    n is not a multiple of the 256-thread workgroup in two of the cases; "zeros" has a third of the row zero."""
    rng = np.random.default_rng(n)
    a = rng.standard_normal(n)
    if kind == "zeros":
        a[rng.random(n) < 1 / 3] = 0.0
    if kind == "unit":
        a = np.sign(a) / np.sqrt(n)
    v = rng.standard_normal(n)
    ctx = pa.Context(0)
    one = pa.QPPF.onerow(ctx, a)
    nz = np.flatnonzero(a)
    ref = pa.QPPF.from_scipy(ctx, sp.csr_matrix((a[nz], (np.zeros(nz.size, dtype=int), nz)), shape=(1, n)), orthonormal=False)
    vd = ctx.vec_from(v)
    S, s, t = np.abs(a * v).sum(), abs(float(a @ v)), float(a @ a)
    D, g = 2 * gamma(n) * S, 2 * gamma(n) + 3 * EPS
    if kind == "unit":  # |a'a - 1| <= n eps: the library treats the row as orthonormal (Q = G'G); the CSR side divides by its t, |t - 1| <= gamma_n
        g += gamma(n)

    def both(name, m):
        out = []
        for pf in (one, ref):
            y = ctx.vec(m)
            getattr(pf, name)(vd, y)
            out.append(y.to_numpy())
        return out

    o, r = both("ApplyG", 1)
    print("G v", abs(o[0] - r[0]), D)
    assert abs(o[0] - r[0]) <= D
    o, r = both("ApplyGtG", n)
    assert (np.abs(o - r) <= (D + 3 * EPS * s) * np.abs(a)).all()
    o, r = both("ApplyHalfQ", 1)
    assert abs(o[0] - r[0]) <= (D + g * s) / t
    oq, rq = both("ApplyQ", n)
    bq = (D + g * s) * np.abs(a) / t
    print("Q v", np.abs(oq - rq).max(), bq.max())
    assert (np.abs(oq - rq) <= bq).all()
    assert (np.abs(oq - a * (a @ v) / t) <= bq).all()  # and against numpy directly
    o, r = both("ApplyP", n)
    assert (np.abs(o - r) <= bq + EPS * (np.abs(v) + np.abs(rq) + bq)).all()
    x1 = ctx.vec_from(np.array([1.7]))
    y1, y2 = ctx.vec(1), ctx.vec(1)
    one.ApplyCP(x1, y1), ref.ApplyCP(x1, y2)
    assert abs(y1.to_numpy()[0] - y2.to_numpy()[0]) <= g * 1.7 / t
    # halfQ' x = (x / t) a
    yo, yr = ctx.vec(n), ctx.vec(n)
    one.ApplyHalfQTranspose(x1, yo), ref.ApplyHalfQTranspose(x1, yr)
    assert (np.abs(yo.to_numpy() - yr.to_numpy()) <= (g + 3 * EPS) * 1.7 * np.abs(a) / t).all()
    ctx.close()


# ---- 2. the operator ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d", [(3000, 64), (1111, 37), (500, 130)])
def test_augmented_operator_against_numpy(N, d):
    """(H + I/C + sigma y y') v.  Row i is y_i (x_i . w) + sigma s y_i + v_i / C with w_c = sum_j y_j v_j X_jc (N terms) and s = sum_j y_j v_j (N terms); the
    computed w_c is within gamma_{N+1} W_c, W_c = sum_j |v_j X_jc|, of the exact one and the row's d-term dot with it adds gamma_{d+1} of sum_c |X_ic| |w_c|:
      |err_i| <= gamma_{N+d+2} sum_c |X_ic| W_c + sigma gamma_{N+2} sum_j |v_j| + 4 eps |row_i|   (the last: the three additions and the shift's product),
    and numpy's own evaluation obeys the same bound, hence the factor 2."""
    ctx = pa.Context(0)
    p = P.svm_dual(N, d)
    X, y = p["X"], p["y"]
    v = np.random.default_rng(1).uniform(0, 1, N)
    H = pa.MatCreateSVMDual(ctx, X, y)
    out0 = ctx.vec(N)
    H.mult(ctx.vec_from(v), out0)
    Cc, sigma = 0.7, 2.5
    H.set_terms(1.0 / Cc, sigma)
    out = ctx.vec(N)
    H.mult(ctx.vec_from(v), out)
    ref = y * (X @ (X.T @ (y * v))) + v / Cc + sigma * y * (y @ v)
    W = np.abs(X).T @ np.abs(v)
    bound = 2 * (gamma(N + d + 2) * (np.abs(X) @ W) + sigma * gamma(N + 2) * np.abs(v).sum() + 4 * EPS * np.abs(ref))
    err = np.abs(out.to_numpy() - ref)
    print("augmented operator: max err / bound", (err / bound).max())
    assert (err <= bound).all()
    # shift 0, sigma 0: today's operator, bit for bit (a fresh operator that never saw the terms)
    H.set_terms(0.0, 0.0)
    out1 = ctx.vec(N)
    H.mult(ctx.vec_from(v), out1)
    H2 = pa.MatCreateSVMDual(ctx, X, y)
    out2 = ctx.vec(N)
    H2.mult(ctx.vec_from(v), out2)
    assert np.array_equal(out1.to_numpy(), out2.to_numpy()) and np.array_equal(out1.to_numpy(), out0.to_numpy())
    ctx.close()


def _solve_terms(ctx, p, shift, sigma, rtol=1e-6):
    H = pa.MatCreateSVMDual(ctx, p["X"], p["y"])
    H.set_terms(shift, sigma)
    qp = pa.QP(ctx)
    qp.SetOperator(H)
    qp.SetRhs(ctx.vec_from(p["b"]))
    x = ctx.vec_from(p["x0"])
    qp.SetInitialVector(x)
    qp.SetBox(None, ctx.vec_from(p["lb"]), ctx.vec_from(p["ub"]))
    qps = pa.QPS(ctx)
    qps.SetQP(qp)
    qps.SetType("mpgp")
    qps.SetTolerances(rtol=rtol)
    st = qps.Solve()
    return H, st, x.to_numpy()


@pytest.mark.parametrize("N", [4003, 777])
def test_augmented_paired_passes_equal_separate_passes(N):
    """The criterion of test_gpu_svm.py::test_svm_paired_passes_equal_separate_passes with sigma != 0 and a shift: s = sum y_i v_i has to travel with the column
    sums from one application to the next, or the prepared expansion step loses the rank-one term."""
    ctx = pa.Context(0)
    p = P.svm_dual(N, 64)
    X, y = p["X"], p["y"]
    shift, sigma = 0.5, 30.0
    Hp, st_p, x_p = _solve_terms(ctx, p, shift, sigma)
    check(ctx.L.pmh_set_knob(b"svm_pairing", 0))
    try:
        Hs, st_s, x_s = _solve_terms(ctx, p, shift, sigma)
    finally:
        check(ctx.L.pmh_set_knob(b"svm_pairing", 1))
    assert st_p.reason == st_s.reason == 2
    assert abs(st_p.iteration - st_s.iteration) <= max(3, st_s.iteration // 6) and st_p.nexp > 0
    w_p, w_s = X.T @ (y * x_p), X.T @ (y * x_s)
    assert np.linalg.norm(w_p - w_s) <= 1e-3 * np.linalg.norm(w_s)
    f = lambda a: 0.5 * np.dot(X.T @ (y * a), X.T @ (y * a)) + 0.5 * shift * a @ a + 0.5 * sigma * (y @ a) ** 2 - a.sum()
    assert abs(f(x_p) - f(x_s)) <= 1e-6 * abs(f(x_s))
    assert x_p.min() >= -ASTOL and x_p.max() <= 1.0 + ASTOL
    per_s, per_p = Hs.passes() / st_s.nmv, Hp.passes() / st_p.nmv
    assert 2.0 <= per_s <= 2.2
    assert per_p <= per_s - 0.9 * (st_p.nexp - 1) / st_p.nmv, (per_p, per_s, st_p.nexp, st_p.nmv)
    _, st_q, x_q = _solve_terms(ctx, p, shift, sigma)
    assert st_q.iteration == st_p.iteration and np.array_equal(x_q, x_p)
    ctx.close()


@pytest.mark.parametrize("d", [64, 37])
def test_penalized_operator_folds_the_one_row_equality(d):
    """A + rho B'B over the SVM operator and the one-row projector with row y / sqrt(n) (folded into the operator) against numpy, and against the generic branch
    (the same row as a 1 x n CSR), also after pmh_op_penalized_set_penalty; an operator that is not the SVM's takes the generic branch over the one-row projector."""
    N = 2500
    ctx = pa.Context(0)
    p = P.svm_offset(N, d, 2.0)
    X, y = p["X"], p["y"]
    a = y / np.sqrt(N)
    v = np.random.default_rng(3).standard_normal(N)
    H = pa.MatCreateSVMDual(ctx, X, y)
    one = pa.QPPF.onerow(ctx, a)
    Ar = pa.MatCreatePenalized(H, one, 7.0)
    csr = pa.QPPF.from_scipy(ctx, sp.csr_matrix(a[None, :]), orthonormal=True)
    H2 = pa.MatCreateSVMDual(ctx, X, y)
    Ag = pa.MatCreatePenalized(H2, csr, 7.0)
    W = np.abs(X).T @ np.abs(v)
    for rho in (7.0, 91.0):
        check(ctx.L.pmh_op_penalized_set_penalty(Ar.h, rho))
        check(ctx.L.pmh_op_penalized_set_penalty(Ag.h, rho))
        o1, o2 = ctx.vec(N), ctx.vec(N)
        Ar.mult(ctx.vec_from(v), o1), Ag.mult(ctx.vec_from(v), o2)
        ref = y * (X @ (X.T @ (y * v))) + rho * a * (a @ v)
        bound = 2 * (gamma(N + d + 2) * (np.abs(X) @ W) + rho / N * gamma(N + 2) * np.abs(v).sum() + 6 * EPS * np.abs(ref))
        assert (np.abs(o1.to_numpy() - ref) <= bound).all() and (np.abs(o2.to_numpy() - ref) <= bound).all()
    # generic branch over the one-row projector: a CSR operator
    M = sp.diags(np.linspace(1.0, 2.0, N)).tocsr()
    A = pa.Op.from_csr(pa.CsrMat(ctx, N, N, M.indptr, M.indices, M.data))
    Ac = pa.MatCreatePenalized(A, one, 5.0)
    o3 = ctx.vec(N)
    Ac.mult(ctx.vec_from(v), o3)
    ref = M @ v + 5.0 * a * (a @ v)
    assert (np.abs(o3.to_numpy() - ref) <= 2 * 5.0 / N * gamma(N + 2) * np.abs(v).sum() + 6 * EPS * np.abs(ref)).all()
    ctx.close()


# ---- 3. no behaviour change ---------------------------------------------------------------------------------------------------------------------------------
def test_unbiased_l1_fit_is_the_existing_solve():
    ctx = pa.Context(0)
    p = P.svm_dual(4000, 64)
    _, st, x = _solve(ctx, p)
    svm = pa.SVM(ctx, loss="L1", C=1.0, bias=False, options="-qps_rtol 1e-6").fit(p["X"], p["y"])
    s = svm.stats
    assert np.array_equal(svm.alpha, x)
    assert (s.inner_iterations, s.nmv, s.ncg, s.nexp, s.nprop, s.reason) == (st.iteration, st.nmv, st.ncg, st.nexp, st.nprop, st.reason)
    assert svm.b == 0.0
    ctx.close()


# ---- 4. - 6. biased training ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["L1", "L2"])
def test_biased_training_against_the_oracle(oracle, loss):
    """svm_offset(4000, 64, 3.0), rtol 1e-6, at most 100 outer iterations (the CPU oracle needs 27 for L1 and 19 for L2).  Then, from the returned dual solution
    alone: feasibility and the KKT residual that SMALXE's own stopping test bounds; the model and the predictions against numpy."""
    ctx = pa.Context(0)
    p = P.svm_offset(4000, 64, 3.0, N_test=2000)
    X, y, n, Cc = p["X"], p["y"], p["n"], p["C"]
    ref = _oracle_train(oracle, p, loss)
    svm = pa.SVM(ctx, loss=loss, C=Cc, bias=True, options="-qps_rtol 1e-6 -qps_max_it 100").fit(X, y)
    st, a = svm.stats, svm.alpha
    print(loss, "HIP outer/inner", st.outer_iterations, st.inner_iterations, "oracle", ref["iteration"], ref["inner_iter_accu"], "reason", st.reason, ref["reason"])
    assert st.reason == ref["reason"] == 2
    assert abs(st.outer_iterations - ref["iteration"]) <= max(3, ref["iteration"] // 6)
    assert abs(st.inner_iterations - ref["inner_iter_accu"]) <= max(3, ref["inner_iter_accu"] // 6)
    sh = 0.0 if loss == "L1" else 1.0 / Cc
    w, w_ref = X.T @ (y * a), X.T @ (y * ref["u"])
    f = lambda z: 0.5 * np.dot(X.T @ (y * z), X.T @ (y * z)) + 0.5 * sh * z @ z - z.sum()
    print(loss, "w rel", np.linalg.norm(w - w_ref) / np.linalg.norm(w_ref), "f rel", abs(f(a) - f(ref["u"])) / abs(f(ref["u"])))
    assert np.linalg.norm(w - w_ref) <= 1e-3 * np.linalg.norm(w_ref)
    assert abs(f(a) - f(ref["u"])) <= 1e-6 * abs(f(ref["u"]))

    # 5. optimality from alpha alone.  SMALXE stops when max(|B a| / rtol_E, |gP|) <= rtol |b| =: thr (rtol_E = 1, b = 1: |b| = sqrt(n)), gP the projected gradient
    # of the Lagrangian 1/2 a'Ha - 1'a + mu (y / sqrt(n))'a at the multiplier it ends with, mu = b_multiplier sqrt(n) by the header's convention.  Recomputing in
    # numpy repeats the n-term sums: |B a| = |y'a| / sqrt(n) moves by at most 2 gamma_n sum |a_i| / sqrt(n) (item 1's bound, either side once), and entry i of the
    # gradient by at most e_i, the operator bound of test_augmented_operator_against_numpy (both evaluations, hence its factor 2) plus 4 eps (|g_i| + 1) + eps |b|
    # for the additions; in norm that is |e|.  So the recomputed quantities obey thr + these terms -- no other factor.
    thr = 1e-6 * np.sqrt(n)
    assert a.min() >= -ASTOL and (loss == "L2" or a.max() <= Cc + ASTOL)
    eq_round = 2 * gamma(n) * np.abs(a).sum() / np.sqrt(n)
    print(loss, "|y'a|/sqrt(n)", abs(y @ a) / np.sqrt(n), "thr", thr, "+ rounding", eq_round, "stats.yTalpha", st.yTalpha)
    assert abs(y @ a) / np.sqrt(n) <= thr + eq_round
    assert abs(st.yTalpha - y @ a) <= 2 * gamma(n) * np.abs(a).sum()
    g = y * (X @ w) + sh * a - 1.0 + st.b_multiplier * y
    e = 2 * gamma(n + 64 + 2) * (np.abs(X) @ (np.abs(X).T @ np.abs(a))) + 4 * EPS * (np.abs(g) + 1.0) + EPS * abs(st.b_multiplier)
    lo, hi = a <= ASTOL, (a >= Cc - ASTOL) if loss == "L1" else np.zeros(n, bool)
    gP = np.where(lo, np.minimum(g, 0.0), np.where(hi, np.maximum(g, 0.0), g))
    kkt = thr + np.linalg.norm(e)
    print(loss, "|gP|", np.linalg.norm(gP), "thr", thr, "+ rounding", np.linalg.norm(e))
    assert np.linalg.norm(gP) <= kkt

    # 6. the model: w and b against numpy restatements; the multiplier's b agrees with the free vectors' to the tolerance of the solve
    w_np, b_np, free = _np_model(p, a, loss)
    assert free.sum() > 0 and st.n_free_sv == free.sum() and st.n_sv == (a > ASTOL).sum()
    Wc = np.abs(X).T @ np.abs(a)
    assert (np.abs(svm.w - w_np) <= 2 * gamma(n + 1) * Wc).all()
    db = 2 * gamma(64 + 1) * float(np.mean(np.abs(X[free]) @ np.abs(w_np))) + 2 * gamma(n + 1) * float(np.mean(np.abs(X[free]) @ Wc)) + gamma(int(free.sum()) + 2) * (1 + abs(b_np))
    print(loss, "b", svm.b, "numpy", b_np, "bound", db, "multiplier", st.b_multiplier, "oracle-side b", _np_model(p, ref["u"], loss)[1])
    assert abs(svm.b - b_np) <= db and svm.b == st.b_free
    # the sign convention of the header, b = mu / sqrt(n): in a free sample y_i - x_i . w - b_mult = -y_i g_i + y_i a_i sh, so the mean over the nf free samples
    # differs from b_mult by at most mean |g_i| <= |gP| / sqrt(nf) (Cauchy-Schwarz) plus, for L2, |sum_free y_i a_i| / (C nf) <= (|y'a| + n astol) / (C nf) (every
    # a_i > astol is free there; the others add at most astol each), plus the rounding db of the mean itself
    nf = int(free.sum())
    b_tie = kkt / np.sqrt(nf) + sh * (abs(y @ a) + n * ASTOL) / nf + db
    print(loss, "|b_free - b_mult|", abs(st.b_multiplier - st.b_free), "bound", b_tie)
    assert abs(st.b_multiplier - st.b_free) <= b_tie
    Xt, yt = p["X_test"], p["y_test"]
    sc_np = Xt @ w_np + b_np
    sb = 2 * gamma(64 + 2) * (np.abs(Xt) @ np.abs(w_np) + abs(b_np)) + np.abs(Xt) @ (2 * gamma(n + 1) * Wc) + db
    sc = svm.decision_function(Xt)
    assert (np.abs(sc - sc_np) <= sb).all()
    sure = np.abs(sc_np) > sb
    print(loss, "test samples left out of the label comparison:", int((~sure).sum()), "of", sure.size)
    assert (~sure).sum() <= 0.01 * sure.size
    lab = svm.predict(Xt)
    assert set(np.unique(lab)) <= {-1.0, 1.0} and np.array_equal(lab[sure], np.where(sc_np >= 0, 1.0, -1.0)[sure])
    t = svm.test(Xt, yt)
    assert t["TP"] + t["FP"] + t["TN"] + t["FN"] == yt.size
    _check_counts(t, sc_np, yt, sure)
    # the bias term is what this data needs (CPU oracle on the same held-out draw: 0.9845 / 0.9855 with bias, 0.8745 without)
    flat = pa.SVM(ctx, loss=loss, C=Cc, bias=False, options="-qps_rtol 1e-6").fit(X, y)
    acc_flat = flat.test(Xt, yt)["accuracy"]
    print(loss, "held-out accuracy with bias", t["accuracy"], "without", acc_flat)
    assert t["accuracy"] > acc_flat
    # the penalised operator SMALXE ended with, probed at its final rho
    _, _, _, sx = svm.solver_handles()
    Arho = C.c_void_p()
    check(ctx.L.pmh_smalxe_get_penalized(sx, C.byref(Arho), None, None))
    v = np.random.default_rng(5).standard_normal(n)
    out = ctx.vec(n)
    check(ctx.L.pmh_op_mult(Arho, ctx.vec_from(v).p, out.p))
    refv = y * (X @ (X.T @ (y * v))) + sh * v + st.rho / n * y * (y @ v)
    bound = 2 * (gamma(n + 66) * (np.abs(X) @ (np.abs(X).T @ np.abs(v))) + st.rho / n * gamma(n + 2) * np.abs(v).sum() + 6 * EPS * np.abs(refv))
    assert st.rho > 0 and (np.abs(out.to_numpy() - refv) <= bound).all()
    ctx.close()


@pytest.mark.parametrize("loss", ["L1", "L2"])
@pytest.mark.parametrize("d", [37, 130])
def test_biased_training_other_widths(d, loss):
    """The generic-d kernels (no fused epilogue), both losses (L1: the upper-bound mask of the bias kernel): the solve converges; the equality and the KKT residual
    are within SMALXE's threshold plus the recomputation's rounding (derived as in test_biased_training_against_the_oracle); scores within the dot-product bound
    of numpy's; labels and the four counts equal numpy's wherever the score decides the label beyond that bound (at most 1 % may be left out)."""
    ctx = pa.Context(0)
    p = P.svm_offset(1500, d, 2.0, N_test=500)
    X, y, n, Cc = p["X"], p["y"], p["n"], p["C"]
    svm = pa.SVM(ctx, loss=loss, C=Cc, bias=True, options="-qps_rtol 1e-6").fit(X, y)
    a, st = svm.alpha, svm.stats
    sh = 0.0 if loss == "L1" else 1.0 / Cc
    thr = 1e-6 * np.sqrt(n)
    print(d, loss, "reason", st.reason, "outer/inner", st.outer_iterations, st.inner_iterations)
    assert st.reason == 2 and a.min() >= -ASTOL and (loss == "L2" or a.max() <= Cc + ASTOL)
    assert abs(y @ a) / np.sqrt(n) <= thr + 2 * gamma(n) * np.abs(a).sum() / np.sqrt(n)
    w_np, b_np, free = _np_model(p, a, loss)
    assert free.sum() > 0 and st.n_free_sv == free.sum() and st.n_sv == (a > ASTOL).sum()
    Wc = np.abs(X).T @ np.abs(a)
    g = y * (X @ w_np) + sh * a - 1.0 + st.b_multiplier * y
    e = 2 * gamma(n + d + 2) * (np.abs(X) @ Wc) + 4 * EPS * (np.abs(g) + 1.0) + EPS * abs(st.b_multiplier)
    lo, hi = a <= ASTOL, (a >= Cc - ASTOL) if loss == "L1" else np.zeros(n, bool)
    gP = np.where(lo, np.minimum(g, 0.0), np.where(hi, np.maximum(g, 0.0), g))
    print(d, loss, "|gP|", np.linalg.norm(gP), "thr", thr, "+", np.linalg.norm(e))
    assert np.linalg.norm(gP) <= thr + np.linalg.norm(e)
    assert (np.abs(svm.w - w_np) <= 2 * gamma(n + 1) * Wc).all()
    db = 2 * gamma(d + 1) * float(np.mean(np.abs(X[free]) @ np.abs(w_np))) + 2 * gamma(n + 1) * float(np.mean(np.abs(X[free]) @ Wc)) + gamma(int(free.sum()) + 2) * (1 + abs(b_np))
    assert abs(svm.b - b_np) <= db
    Xt, yt = p["X_test"], p["y_test"]
    sc_np = Xt @ w_np + b_np
    sb = 2 * gamma(d + 2) * (np.abs(Xt) @ np.abs(w_np) + abs(b_np)) + np.abs(Xt) @ (2 * gamma(n + 1) * Wc) + db
    sc = svm.decision_function(Xt)
    assert (np.abs(sc - sc_np) <= sb).all()
    sure = np.abs(sc_np) > sb
    assert (~sure).sum() <= 0.01 * sure.size
    assert np.array_equal(svm.predict(Xt)[sure], np.where(sc_np >= 0, 1.0, -1.0)[sure])
    _check_counts(svm.test(Xt, yt), sc_np, yt, sure)
    ctx.close()


# ---- 7. the bias term is free in passes over X -----------------------------------------------------------------------------------------------------------------
def _fixed(ctx, H, pf, rho, p, iters):
    """`iters` MPGP iterations (RunFixed) on A = H (+ rho B'B through the penalised operator); returns (stats, passes over X of the run)."""
    A = pa.MatCreatePenalized(H, pf, rho) if pf is not None else H
    qp = pa.QP(ctx)
    qp.SetOperator(A)
    qp.SetRhs(ctx.vec_from(p["b"]))
    qp.SetInitialVector(ctx.vec_from(p["x0"]))
    qp.SetBox(None, ctx.vec_from(p["lb"]), ctx.vec_from(p["ub"]))
    qps = pa.QPS(ctx)
    qps.SetQP(qp)
    qps.SetType("mpgp")
    qps.SetUp()
    p0 = H.passes()
    st = qps.RunFixed(iters)
    return st, H.passes() - p0


def test_bias_costs_no_pass_over_X():
    """Fixed iterations so that the step sequences match: the penalised operator over (SVM operator, one-row projector) against the SVM operator carrying the SAME
    rank-one term itself (one mathematical operator: the same steps), and the passes-per-multiplication of both against the plain unbiased run's, which takes the same sequence of
    step types on this instance (asserted)."""
    ctx = pa.Context(0)
    p = P.svm_offset(4000, 64, 3.0)
    n, rho = p["n"], 500.0
    a = p["y"] / np.sqrt(n)
    H1 = pa.MatCreateSVMDual(ctx, p["X"], p["y"])
    st1, pass1 = _fixed(ctx, H1, pa.QPPF.onerow(ctx, a), rho, p, 60)
    H2 = pa.MatCreateSVMDual(ctx, p["X"], p["y"])
    H2.set_terms(0.0, rho / n)
    st2, pass2 = _fixed(ctx, H2, None, 0.0, p, 60)
    H3 = pa.MatCreateSVMDual(ctx, p["X"], p["y"])
    st3, pass3 = _fixed(ctx, H3, None, 0.0, p, 60)
    print("folded", (st1.nmv, st1.ncg, st1.nexp, st1.nprop, pass1), "own term", (st2.nmv, st2.ncg, st2.nexp, st2.nprop, pass2), "plain", (st3.nmv, st3.ncg, st3.nexp, st3.nprop, pass3))
    assert (st1.nmv, st1.ncg, st1.nexp, st1.nprop) == (st2.nmv, st2.ncg, st2.nexp, st2.nprop)
    assert pass1 / st1.nmv == pass2 / st2.nmv
    # the PLAIN operator (the kernels without the 65th column sum) takes the same sequence of step types on this instance over these 60 iterations -- asserted,
    # not assumed: the runs are reproducible bit for bit, so this either holds or the instance has to be changed -- and then streams X exactly as often
    assert (st1.nmv, st1.ncg, st1.nexp, st1.nprop) == (st3.nmv, st3.ncg, st3.nexp, st3.nprop)
    assert pass1 == pass3 and pass1 / st1.nmv == pass3 / st3.nmv
    assert pass1 / st1.nmv < 2.0 and st1.nexp > 0  # (pairing is live in all three)
    ctx.close()


_TRACE_JOB = r'''
import sys
sys.path.insert(0, %r)
import ctypes as C
import permon_amd as pa
from permon_amd import problems as P
from permon_amd._lib import check
bias, iters = int(sys.argv[1]), int(sys.argv[2])
ctx = pa.Context(0)
p = P.svm_offset(4000, 64, 3.0)
svm = pa.SVM(ctx, loss="L1", C=1.0, bias=bool(bias), options="-qps_rtol 1e-6").create(p["X"], p["y"])
H, pf, mpgp, sx = svm.solver_handles()
if bias:
    mpgp = C.c_void_p()
    check(ctx.L.pmh_smalxe_get_inner(sx, C.byref(mpgp)))
    check(ctx.L.pmh_smalxe_set_inner_max_it(sx, iters))  # the injected test ends the run by ITS limit (smalxe.c:626-631), not by the inner solver's own
check(ctx.L.pmh_mpgp_run_fixed(mpgp, iters))
ctx.close()
'''


def _kernel_counts(tmp, bias, iters):
    job = os.path.join(tmp, "job.py")
    with open(job, "w") as fh:
        fh.write(_TRACE_JOB % ROOT)
    out = os.path.join(tmp, "t_%d_%d" % (bias, iters))
    # its own session: a time limit ends the profiler AND the Python child it started
    pr = subprocess.Popen(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "svm", "--", sys.executable, job, str(bias), str(iters)],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, start_new_session=True)
    try:
        rc = pr.wait(timeout=300)
    except subprocess.TimeoutExpired:
        import signal

        os.killpg(pr.pid, signal.SIGKILL)
        pr.wait()
        raise
    assert rc == 0, "rocprofv3 run failed with status %d" % rc
    import csv
    import glob
    import re

    f = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    assert f, "no kernel stats written"
    cnt = {}
    for row in csv.DictReader(open(f[0])):
        name = re.sub(r"^void ", "", row["Name"]).split("(")[0].split("<")[0].strip()
        cnt[name] = cnt.get(name, 0) + int(row["Calls"])
    return cnt, f[0]


def test_inner_loop_launches_only_the_svm_kernels(tmp_path):
    """Kernel traces (rocprofv3 --kernel-trace --stats) of 20 and of 80 inner iterations, biased (SMALXE's inner MPGP on the folded penalised operator, ||B u||
    evaluated every iteration) and unbiased: the kernels whose call counts grow with the iteration count are the inner loop's.  With the bias term they are the
    SVM operator's kernels and whatever the unbiased loop launches too -- no projector kernel, no vector kernel of its own.  (In a full solve the projector's dot,
    16 n bytes, does run at the iterations where MPGP holds the next product back until the convergence test has been read: the ends of the inner solves.)"""
    grown = {}
    for bias in (1, 0):
        c20, _ = _kernel_counts(str(tmp_path), bias, 20)
        c80, f = _kernel_counts(str(tmp_path), bias, 80)
        grown[bias] = {k for k in c80 if c80[k] > c20.get(k, 0)}
        print("bias", bias, "inner-loop kernels:", sorted(grown[bias]))
        dst = os.environ.get("PMH_SVM_TRACE_DIR")
        if dst:
            import shutil

            shutil.copy(f, os.path.join(dst, "svm_train_inner_loop_bias%d_kernel_stats.csv" % bias))
    assert {"k_svm_x64_p1", "k_svm_aux_finish"} <= grown[1] and "k_svm_x64_p1" in grown[0]  # (the comparison is not empty)
    # with the bias term: what the unbiased loop launches, the same SVM pass / column-sum kernels, and the one-workgroup finisher of ||B u|| -- by name
    allowed = grown[0] | {"k_svm_x64_p1", "k_svm_x64_grad", "k_svm_colsum_feas", "k_svm_xt64", "k_svm_colsum", "k_svm_aux_finish"}
    assert grown[1] <= allowed, grown[1] - allowed
