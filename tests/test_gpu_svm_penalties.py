"""GPU tests of the SVM penalties per class and per sample (pmh_op_svm_dual_set_diag, pmh_svm_set_penalties, pmh_svm_get_penalties): the operator with a diagonal
against numpy (dense rows of three widths, CSR), the paired passes with a diagonal, uniform penalties against the scalar path bit for bit, weighted training
against the CPU oracle, what the class penalties do to the two kinds of error, retraining, and the errors of the C entries."""
import ctypes as C

import numpy as np
import pytest

import permon_amd as pa
from permon_amd import problems as P
from permon_amd._lib import check
from svm_train_cases import ASTOL, EPS, gamma, check_counts as _check_counts, np_model as _np_model

pytestmark = pytest.mark.gpu
PMH_ERR_ARG, PMH_ERR_STATE = 2, 3


def _sparse_instance():
    return P.svm_sparse(1500, 300, 8, 1.0, 0.5, 1.0)


# ---- 2. the operator with a diagonal ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3000, 64), (1111, 37), (500, 130), "csr"])
def test_operator_with_diagonal_against_numpy(shape):
    """(H + diag(dg) + sigma y y') v within the bound of test_gpu_svm_train.py::test_augmented_operator_against_numpy (its 4 eps |ref_i| term covers the diagonal's
    product and addition as it covered the shift's); set_diag(None) gives back the plain operator bit for bit; a diagonal and a non-zero shift exclude each other
    in either order of arrival."""
    ctx = pa.Context(0)
    if shape == "csr":
        p = _sparse_instance()
        Xop, X, y = p["X"], p["X"].toarray(), p["y"]
    else:
        p = P.svm_dual(*shape)
        Xop, X, y = p["X"], p["X"], p["y"]
    N, d = X.shape
    rng = np.random.default_rng(1)
    v = rng.uniform(0, 1, N)
    dg, sigma = 1.0 / rng.uniform(0.2, 5.0, N), 2.5
    H = pa.MatCreateSVMDual(ctx, Xop, y)
    H.set_terms(0.0, sigma)
    H.set_diag(dg)
    out = ctx.vec(N)
    H.mult(ctx.vec_from(v), out)
    ref = y * (X @ (X.T @ (y * v))) + dg * v + sigma * y * (y @ v)
    W = np.abs(X).T @ np.abs(v)
    bound = 2 * (gamma(N + d + 2) * (np.abs(X) @ W) + sigma * gamma(N + 2) * np.abs(v).sum() + 4 * EPS * np.abs(ref))
    err = np.abs(out.to_numpy() - ref)
    print("operator with a diagonal", shape, ": max err / bound", (err / bound).max())
    assert (err <= bound).all()
    # the diagonal alone (sigma 0) takes the augmented kernels too
    H.set_terms(0.0, 0.0)
    H.mult(ctx.vec_from(v), out)
    ref0 = y * (X @ (X.T @ (y * v))) + dg * v
    assert (np.abs(out.to_numpy() - ref0) <= 2 * (gamma(N + d + 2) * (np.abs(X) @ W) + 4 * EPS * np.abs(ref0))).all()
    # off again: the plain operator, bit for bit (a fresh operator that never saw a diagonal)
    H.set_diag(None)
    out1, out2 = ctx.vec(N), ctx.vec(N)
    H.mult(ctx.vec_from(v), out1)
    H2 = pa.MatCreateSVMDual(ctx, Xop, y)
    H2.mult(ctx.vec_from(v), out2)
    assert np.array_equal(out1.to_numpy(), out2.to_numpy())
    # a shift and a diagonal exclude each other, whichever arrives second
    dv = ctx.vec_from(dg)
    H.set_terms(0.7, 0.0)
    rc = ctx.L.pmh_op_svm_dual_set_diag(H.h, dv.p)
    msg = ctx.L.pmh_last_error()
    assert rc == PMH_ERR_ARG and b"shift" in msg and b"diagonal" in msg, (rc, msg)
    H.set_terms(0.0, 0.0)
    H.set_diag(dv)
    rc = ctx.L.pmh_op_svm_dual_set_terms(H.h, 0.7, 0.0)
    msg = ctx.L.pmh_last_error()
    assert rc == PMH_ERR_ARG and b"shift" in msg and b"diagonal" in msg, (rc, msg)
    H.set_terms(0.0, 3.0)  # (a rank-one term beside the diagonal is no conflict)
    ctx.close()


# ---- 3. the paired passes keep their pairing ----------------------------------------------------------------------------------------------------------------------
def _fixed(ctx, p, iters, diag=None, shift=0.0, rho=None):
    """`iters` MPGP iterations (RunFixed, tests/test_gpu_svm_train.py::_fixed) on H + diag / shift (+ rho B'B through the penalised operator over the one-row
    projector with row y / sqrt(n)); returns (step counts, passes over X of the run, the iterate)."""
    H = pa.MatCreateSVMDual(ctx, p["X"], p["y"])
    if shift:
        H.set_terms(shift, 0.0)
    if diag is not None:
        H.set_diag(diag)
    A = pa.MatCreatePenalized(H, pa.QPPF.onerow(ctx, p["y"] / np.sqrt(p["n"])), rho) if rho is not None else H
    qp = pa.QP(ctx)
    qp.SetOperator(A)
    qp.SetRhs(ctx.vec_from(p["b"]))
    x = ctx.vec_from(p["x0"])
    qp.SetInitialVector(x)
    qp.SetBox(None, ctx.vec_from(p["lb"]), ctx.vec_from(p["ub"]))
    qps = pa.QPS(ctx)
    qps.SetQP(qp)
    qps.SetType("mpgp")
    qps.SetUp()
    p0 = H.passes()
    st = qps.RunFixed(iters)
    return (st.nmv, st.ncg, st.nexp, st.nprop), H.passes() - p0, x.to_numpy()


@pytest.mark.parametrize("rho", [None, 500.0])
def test_paired_passes_keep_their_pairing_with_a_diagonal(rho):
    """d = 64, N = 3000, 60 fixed MPGP iterations, on the operator alone and through the penalised operator with the one-row projector at rho = 500.  Pairing on
    and off take the same step sequence and their iterates agree by the criterion of test_augmented_paired_passes_equal_separate_passes (w to 1e-3, the objective
    to 1e-6, relative: the two runs differ by the order of the partial sums only).  With pairing on, a diagonal that holds 0.7 everywhere is the run with the
    scalar shift 0.7: the same expression on the same numbers, so the same bits and the same count of passes over X; the non-uniform diagonal streams X no more
    often per multiplication than that, and less than twice (pairing is live)."""
    ctx = pa.Context(0)
    p = P.svm_offset(3000, 64, 2.0)
    X, y, n = p["X"], p["y"], p["n"]
    dg = 1.0 / np.random.default_rng(1).uniform(0.2, 5.0, n)
    steps_p, pass_p, x_p = _fixed(ctx, p, 60, diag=dg, rho=rho)
    check(ctx.L.pmh_set_knob(b"svm_pairing", 0))
    try:
        steps_s, pass_s, x_s = _fixed(ctx, p, 60, diag=dg, rho=rho)
    finally:
        check(ctx.L.pmh_set_knob(b"svm_pairing", 1))
    print("rho", rho, "paired", steps_p, pass_p, "separate", steps_s, pass_s)
    assert steps_p == steps_s and steps_p[2] > 0
    w_p, w_s = X.T @ (y * x_p), X.T @ (y * x_s)
    assert np.linalg.norm(w_p - w_s) <= 1e-3 * np.linalg.norm(w_s)
    sg = 0.0 if rho is None else rho / n
    f = lambda a: 0.5 * np.dot(X.T @ (y * a), X.T @ (y * a)) + 0.5 * a @ (dg * a) + 0.5 * sg * (y @ a) ** 2 - a.sum()
    assert abs(f(x_p) - f(x_s)) <= 1e-6 * abs(f(x_s))
    assert 2.0 <= pass_s / steps_s[0] <= 2.2 and pass_p < pass_s
    # the scalar shift and the diagonal that holds it everywhere
    steps_c, pass_c, x_c = _fixed(ctx, p, 60, shift=0.7, rho=rho)
    steps_u, pass_u, x_u = _fixed(ctx, p, 60, diag=np.full(n, 0.7), rho=rho)
    print("rho", rho, "shift 0.7", steps_c, pass_c, "diagonal of 0.7", steps_u, pass_u)
    assert steps_u == steps_c and pass_u == pass_c and np.array_equal(x_u, x_c)
    assert pass_u / steps_u[0] < 2.0 and pass_p / steps_p[0] < 2.0
    ctx.close()


# ---- 4. uniform penalties are the scalar path, bit for bit ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("loss", ["L1", "L2"])
@pytest.mark.parametrize("inst", [64, 37, "csr"])
def test_uniform_penalties_are_the_scalar_path(inst, loss, bias):
    """C_pos = C_neg = 0.7 with weights of 1 is C = 0.7: the bounds hold 0.7 * 1.0 = 0.7 and the diagonal 1.0 / 0.7, the numbers of the scalar path in the same
    expression, so every iterate, the model and the counts are equal, not close."""
    ctx = pa.Context(0)
    p = _sparse_instance() if inst == "csr" else P.svm_offset(1500, inst, 2.0)
    X, y, n = p["X"], p["y"], p["n"]
    opts = "-qps_rtol 1e-6"
    s0 = pa.SVM(ctx, loss=loss, C=0.7, bias=bias, options=opts).fit(X, y)
    s1 = pa.SVM(ctx, loss=loss, C=0.7, bias=bias, options=opts, C_pos=0.7, C_neg=0.7).fit(X, y, sample_weight=np.ones(n))
    assert np.array_equal(s1.penalties, np.full(n, 0.7)) and np.array_equal(s0.penalties, np.full(n, 0.7))
    t0, t1 = s0.stats, s1.stats
    it = lambda t: (t.reason, t.outer_iterations, t.inner_iterations, t.nmv, t.ncg, t.nexp, t.nprop, t.n_sv, t.n_free_sv)
    print(inst, loss, bias, it(t0), it(t1))
    assert it(t0) == it(t1) and t0.reason > 0
    assert np.array_equal(s0.alpha, s1.alpha) and np.array_equal(s0.w, s1.w) and s0.b == s1.b
    ctx.close()


# ---- 5. weighted training against the CPU oracle ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["L1", "L2"])
@pytest.mark.parametrize("n,d", [(2000, 64), (1500, 37)])
def test_weighted_training_against_the_oracle(oracle, n, d, loss):
    """C_pos = 0.5, C_neg = 4, weights uniform in (0.5, 2), bias on, rtol 1e-6, at most 100 outer iterations.  The oracle is SMALXE on the operator
    a -> y o (X (X' (y o a))) + diag o a with the box 0 <= a <= C_i (L1) or 0 <= a (L2, diag = 1 / C_i) and the one-row equality; it ends with reason 2 after
    16 / 13 outer iterations (n = 2000, d = 64, L1 / L2) and 34 / 28 (n = 1500, d = 37).  The checks and their bounds are those of
    test_gpu_svm_train.py::test_biased_training_against_the_oracle, with C_i where C stood and 1/2 a' diag a in the objective."""
    ctx = pa.Context(0)
    p = P.svm_offset(n, d, 2.0, N_test=500)
    X, y = p["X"], p["y"]
    cp, cn = 0.5, 4.0
    wt = np.random.default_rng(11).uniform(0.5, 2.0, n)
    Ci = np.where(y > 0, cp, cn) * wt
    dg = np.zeros(n) if loss == "L1" else 1.0 / Ci
    op = oracle.Op(n, fn=lambda a: y * (X @ (X.T @ (y * a))) + dg * a)
    pf = oracle.Qppf(oracle.Csr(1, n, [0, n], np.arange(n), y / np.sqrt(n)), orthonormal=True)
    box = oracle.Box(n, lb=p["lb"], ub=Ci if loss == "L1" else None)
    ref = oracle.smalxe(op, p["b"], p["x0"], box, pf, rtol=1e-6, max_it=100)
    svm = pa.SVM(ctx, loss=loss, C=1.0, bias=True, options="-qps_rtol 1e-6 -qps_max_it 100", C_pos=cp, C_neg=cn).fit(X, y, sample_weight=wt)
    assert np.array_equal(svm.penalties, Ci)
    st, a = svm.stats, svm.alpha
    print(n, d, loss, "HIP outer/inner", st.outer_iterations, st.inner_iterations, "oracle", ref["iteration"], ref["inner_iter_accu"], "reason", st.reason, ref["reason"])
    assert st.reason == ref["reason"] == 2
    assert abs(st.outer_iterations - ref["iteration"]) <= max(3, ref["iteration"] // 6)
    assert abs(st.inner_iterations - ref["inner_iter_accu"]) <= max(3, ref["inner_iter_accu"] // 6)
    w, w_ref = X.T @ (y * a), X.T @ (y * ref["u"])
    f = lambda z: 0.5 * np.dot(X.T @ (y * z), X.T @ (y * z)) + 0.5 * z @ (dg * z) - z.sum()
    print(n, d, loss, "w rel", np.linalg.norm(w - w_ref) / np.linalg.norm(w_ref), "f rel", abs(f(a) - f(ref["u"])) / abs(f(ref["u"])))
    assert np.linalg.norm(w - w_ref) <= 1e-3 * np.linalg.norm(w_ref)
    assert abs(f(a) - f(ref["u"])) <= 1e-6 * abs(f(ref["u"]))

    # optimality from alpha alone, the active sets taken against C_i
    thr = 1e-6 * np.sqrt(n)
    assert a.min() >= -ASTOL and (loss == "L2" or (a <= Ci + ASTOL).all())
    eq_round = 2 * gamma(n) * np.abs(a).sum() / np.sqrt(n)
    print(n, d, loss, "|y'a|/sqrt(n)", abs(y @ a) / np.sqrt(n), "thr", thr, "+ rounding", eq_round)
    assert abs(y @ a) / np.sqrt(n) <= thr + eq_round
    assert abs(st.yTalpha - y @ a) <= 2 * gamma(n) * np.abs(a).sum()
    g = y * (X @ w) + dg * a - 1.0 + st.b_multiplier * y
    e = 2 * gamma(n + d + 2) * (np.abs(X) @ (np.abs(X).T @ np.abs(a))) + 4 * EPS * (np.abs(g) + 1.0) + EPS * abs(st.b_multiplier)
    lo, hi = a <= ASTOL, (a >= Ci - ASTOL) if loss == "L1" else np.zeros(n, bool)
    gP = np.where(lo, np.minimum(g, 0.0), np.where(hi, np.maximum(g, 0.0), g))
    kkt = thr + np.linalg.norm(e)
    print(n, d, loss, "|gP|", np.linalg.norm(gP), "thr", thr, "+ rounding", np.linalg.norm(e))
    assert np.linalg.norm(gP) <= kkt

    # the model and the counts with per-sample bounds
    w_np, b_np, free = _np_model(p, a, loss, Ci)
    print(n, d, loss, "free support vectors", int(free.sum()), "support vectors", int((a > ASTOL).sum()))
    assert free.sum() > 0 and st.n_free_sv == free.sum() and st.n_sv == (a > ASTOL).sum()
    Wc = np.abs(X).T @ np.abs(a)
    assert (np.abs(svm.w - w_np) <= 2 * gamma(n + 1) * Wc).all()
    db = 2 * gamma(d + 1) * float(np.mean(np.abs(X[free]) @ np.abs(w_np))) + 2 * gamma(n + 1) * float(np.mean(np.abs(X[free]) @ Wc)) + gamma(int(free.sum()) + 2) * (1 + abs(b_np))
    print(n, d, loss, "b", svm.b, "numpy", b_np, "bound", db)
    assert abs(svm.b - b_np) <= db and svm.b == st.b_free
    Xt, yt = p["X_test"], p["y_test"]
    sc_np = Xt @ w_np + b_np
    sb = 2 * gamma(d + 2) * (np.abs(Xt) @ np.abs(w_np) + abs(b_np)) + np.abs(Xt) @ (2 * gamma(n + 1) * Wc) + db
    sc = svm.decision_function(Xt)
    assert (np.abs(sc - sc_np) <= sb).all()
    sure = np.abs(sc_np) > sb
    print(n, d, loss, "test samples left out of the label comparison:", int((~sure).sum()), "of", sure.size)
    assert (~sure).sum() <= 0.01 * sure.size
    lab = svm.predict(Xt)
    assert set(np.unique(lab)) <= {-1.0, 1.0} and np.array_equal(lab[sure], np.where(sc_np >= 0, 1.0, -1.0)[sure])
    _check_counts(svm.test(Xt, yt), sc_np, yt, sure)
    ctx.close()


# ---- 6. the penalties do what they are for ------------------------------------------------------------------------------------------------------------------------------
def test_class_penalties_move_the_errors():
    """svm_offset(2000, 64, 2.0), L1 with bias: a larger penalty on the negative class must not raise the false positives on the training samples, a larger one
    on the positive class not the false negatives.  The CPU oracle's own solutions give FP / FN = 6 / 7 (balanced), 0 / 22 (C_neg = 8), 25 / 0 (C_pos = 8)."""
    ctx = pa.Context(0)
    p = P.svm_offset(2000, 64, 2.0)
    X, y = p["X"], p["y"]
    t = {}
    for cp, cn in ((1.0, 1.0), (1.0, 8.0), (8.0, 1.0)):
        svm = pa.SVM(ctx, loss="L1", C=1.0, bias=True, options="-qps_rtol 1e-6 -qps_max_it 100", C_pos=cp, C_neg=cn).fit(X, y)
        assert svm.stats.reason == 2
        t[cp, cn] = svm.test(X, y)
        print("C_pos", cp, "C_neg", cn, t[cp, cn])
    assert t[1.0, 8.0]["FP"] <= t[1.0, 1.0]["FP"]
    assert t[8.0, 1.0]["FN"] <= t[1.0, 1.0]["FN"]
    ctx.close()


# ---- 7. retraining ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["L1", "L2"])
def test_penalties_set_twice_equal_a_fresh_handle(loss):
    ctx = pa.Context(0)
    p = P.svm_offset(1500, 64, 2.0)
    X, y, n = p["X"], p["y"], p["n"]
    w1, w2 = np.random.default_rng(3).uniform(0.5, 2.0, n), np.random.default_rng(4).uniform(0.5, 2.0, n)
    opts = "-qps_rtol 1e-6"
    svm = pa.SVM(ctx, loss=loss, C=1.0, bias=True, options=opts).create(X, y)
    svm.set_penalties(0.5, 4.0, w1).train()
    a1 = svm.alpha
    svm.set_penalties(3.0, 0.8, w2)
    # untrained again: no model to hand out
    rc = ctx.L.pmh_svm_get_model(svm.h, None, None)
    assert rc == PMH_ERR_STATE and b"pmh_svm_train" in ctx.L.pmh_last_error()
    svm.train()
    fresh = pa.SVM(ctx, loss=loss, C=1.0, bias=True, options=opts, C_pos=3.0, C_neg=0.8).fit(X, y, sample_weight=w2)
    Ci = np.where(y > 0, 3.0, 0.8) * w2
    assert np.array_equal(svm.penalties, Ci) and np.array_equal(fresh.penalties, Ci)
    assert svm.stats.reason == 2 and not np.array_equal(a1, svm.alpha)
    assert np.array_equal(svm.alpha, fresh.alpha) and np.array_equal(svm.w, fresh.w) and svm.b == fresh.b
    assert (svm.stats.outer_iterations, svm.stats.inner_iterations) == (fresh.stats.outer_iterations, fresh.stats.inner_iterations)
    ctx.close()


# ---- 8. errors through the C entries ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["L1", "L2"])
def test_penalty_errors(loss):
    ctx = pa.Context(0)
    p = P.svm_offset(700, 37, 2.0)
    n = p["n"]
    svm = pa.SVM(ctx, loss=loss, C=1.0, bias=True).create(p["X"], p["y"])
    L = ctx.L
    for cp, cn, name, val in ((0.0, 1.0, b"C_pos", b"0"), (1.0, -1.0, b"C_neg", b"-1"), (float("inf"), 1.0, b"C_pos", b"inf")):
        rc = L.pmh_svm_set_penalties(svm.h, cp, cn, None)
        msg = L.pmh_last_error()
        assert rc == PMH_ERR_ARG and name in msg and val in msg, (rc, msg)
    w = np.random.default_rng(5).uniform(0.5, 2.0, n)
    w[3], w[400], w[699] = 0.0, -1.5, np.nan
    wd = ctx.vec_from(w)
    rc = L.pmh_svm_set_penalties(svm.h, 1.0, 1.0, wd.p)
    msg = L.pmh_last_error()
    assert rc == PMH_ERR_ARG and b"3 of the sample weights" in msg, (rc, msg)
    # the refused calls changed nothing
    assert np.array_equal(svm.penalties, np.ones(n))
    svm.train()
    assert svm.stats.reason == 2
    ctx.close()
