"""GPU tests of the SVM on sparse samples (csrc/svm_csr.hip): the dual operator for X in CSR against scipy and against the dense operator, the penalised operator
that folds the bias equality into it, training with and without bias against the CPU oracle, the model, prediction on held-out sparse samples, reproducibility,
the one-rank communicator and the argument errors of the C entries.

Rounding bounds are Higham's gamma_k = k eps / (1 - k eps) as in test_gpu_svm_train.py, with the dense test's N replaced by cmax + 1 (cmax = the largest column
count: the longest sum in w_c) and d by kmax + 1 (kmax = the largest row count): any summation order of those terms obeys them."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

import permon_amd as pa
from permon_amd import _lib
from permon_amd import problems as P
from permon_amd._lib import check
from svm_train_cases import ASTOL, EPS, gamma, check_counts as _check_counts, np_model as _np_model, oracle_train as _oracle_train, solve as _solve

pytestmark = pytest.mark.gpu
PMH_ERR_ARG = 2

INST = dict(A=(4000, 5000, 30, 1.0, 0.5, 1.0), B=(4000, 300, 12, 1.2, 0.5, 1.0), C=(3000, 20000, 40, 0.8, 0.5, 10.0))


def _cmax_kmax(X):
    X = X.tocsr()
    return int(np.bincount(X.indices, minlength=X.shape[1]).max()) if X.nnz else 0, int(np.diff(X.indptr).max()) if X.shape[0] else 0


def _op_bound(X, v, ref, sigma, extra_eps=4):
    """|out - ref| entry by entry for (H + shift I + sigma y y') v: item 1 of the issue."""
    Xa = abs(X)
    cmax, kmax = _cmax_kmax(X)
    N = X.shape[0]
    return 2 * (gamma(cmax + kmax + 2) * (Xa @ (Xa.T @ np.abs(v))) + sigma * gamma(N + 2) * np.abs(v).sum() + extra_eps * EPS * np.abs(ref))


def _zero_rows(X, frac, seed):
    X = X.tolil(copy=True)
    for i in np.random.default_rng(seed).choice(X.shape[0], int(frac * X.shape[0]), replace=False):
        X.rows[i], X.data[i] = [], []
    return X.tocsr()


def _operator_cases():
    for k, a in INST.items():
        yield k, a
    yield "A_empty_rows", INST["A"]
    yield "odd_N", (1037, 700, 9, 1.0, 0.5, 1.0)


# ---- 1. the operator against scipy -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,args", list(_operator_cases()))
def test_sparse_operator_against_scipy(name, args):
    """Plain and with set_terms(1 / 0.7, 2.5): row i is y_i (x_i . w) + sigma s y_i + v_i / C with w_c a sum of at most cmax terms and the row's dot one of at most
    kmax: |err_i| <= gamma_{cmax+kmax+2} sum_c |X_ic| W_c + sigma gamma_{N+2} sum_j |v_j| + 4 eps |row_i|, W = |X|'|v|; scipy's own evaluation obeys the same bound,
    hence the factor 2.  A_empty_rows: 5 % of A's samples have no stored entry.  odd_N: N is not a multiple of the 256-thread workgroup."""
    p = P.svm_sparse(*args)
    X, y = p["X"], p["y"]
    if name == "A_empty_rows":
        X = _zero_rows(X, 0.05, 11)
        assert (np.diff(X.indptr) == 0).sum() == 200
    N = X.shape[0]
    ctx = pa.Context(0)
    v = np.random.default_rng(1).uniform(0, 1, N)
    vd = ctx.vec_from(v)
    H = pa.MatCreateSVMDual(ctx, X, y)
    out0, out0b = ctx.vec(N), ctx.vec(N)
    H.mult(vd, out0), H.mult(vd, out0b)
    ref0 = y * (X @ (X.T @ (y * v)))
    err, bound = np.abs(out0.to_numpy() - ref0), _op_bound(X, v, ref0, 0.0)
    print(name, "plain: max err / bound", (err / np.maximum(bound, 1e-300)).max(), "passes", H.passes())
    assert (err <= bound).all()
    assert np.array_equal(out0.to_numpy(), out0b.to_numpy())  # two applications to the same vector: the same bits
    assert H.passes() == 4
    Cc, sigma = 0.7, 2.5
    H.set_terms(1.0 / Cc, sigma)
    out, outb = ctx.vec(N), ctx.vec(N)
    H.mult(vd, out), H.mult(vd, outb)
    ref = ref0 + v / Cc + sigma * y * (y @ v)
    err, bound = np.abs(out.to_numpy() - ref), _op_bound(X, v, ref, sigma)
    print(name, "augmented: max err / bound", (err / bound).max())
    assert (err <= bound).all()
    assert np.array_equal(out.to_numpy(), outb.to_numpy())
    # shift 0, sigma 0: the plain operator, bit for bit (a fresh operator that never saw the terms)
    H.set_terms(0.0, 0.0)
    out1 = ctx.vec(N)
    H.mult(vd, out1)
    H2 = pa.MatCreateSVMDual(ctx, X, y)
    out2 = ctx.vec(N)
    H2.mult(vd, out2)
    assert np.array_equal(out1.to_numpy(), out2.to_numpy()) and np.array_equal(out1.to_numpy(), out0.to_numpy())
    ctx.close()


# ---- 2. sparse equals dense --------------------------------------------------------------------------------------------------------------------------------
def test_sparse_operator_equals_the_dense_operator():
    """svm_offset(1111, 37) as ndarray and as a fully stored CSR matrix: each operator is within item 1's bound (once: its own rounding, no factor 2) of the exact
    result, so the two differ by at most that bound with its factor 2."""
    p = P.svm_offset(1111, 37)
    X, y, N = p["X"], p["y"], p["n"]
    Xs = sp.csr_matrix(X)
    assert Xs.nnz == N * 37
    ctx = pa.Context(0)
    v = np.random.default_rng(2).uniform(0, 1, N)
    Hd, Hs = pa.MatCreateSVMDual(ctx, X, y), pa.MatCreateSVMDual(ctx, Xs, y)
    for shift, sigma in ((0.0, 0.0), (1 / 0.7, 2.5)):
        Hd.set_terms(shift, sigma), Hs.set_terms(shift, sigma)
        od, os_ = ctx.vec(N), ctx.vec(N)
        Hd.mult(ctx.vec_from(v), od), Hs.mult(ctx.vec_from(v), os_)
        ref = y * (X @ (X.T @ (y * v))) + shift * v + sigma * y * (y @ v)
        bound = _op_bound(Xs, v, ref, sigma)
        err = np.abs(od.to_numpy() - os_.to_numpy())
        print("sparse vs dense", (shift, sigma), "max err / bound", (err / bound).max())
        assert (err <= bound).all()
    ctx.close()


# ---- 3. the penalised operator -----------------------------------------------------------------------------------------------------------------------------
def test_penalized_operator_folds_the_one_row_equality_sparse():
    """A + rho B'B over (sparse operator, one-row projector y / sqrt(n)) -- folded into the operator -- against scipy and against the generic branch (the same row
    as a 1 x n CSR projector), at rho = 7 and after pmh_op_penalized_set_penalty(91); on the folded side a product streams X exactly twice."""
    p = P.svm_sparse(*INST["B"])
    X, y, N = p["X"], p["y"], p["n"]
    a = y / np.sqrt(N)
    v = np.random.default_rng(3).standard_normal(N)
    ctx = pa.Context(0)
    H = pa.MatCreateSVMDual(ctx, X, y)
    Ar = pa.MatCreatePenalized(H, pa.QPPF.onerow(ctx, a), 7.0)
    H2 = pa.MatCreateSVMDual(ctx, X, y)
    Ag = pa.MatCreatePenalized(H2, pa.QPPF.from_scipy(ctx, sp.csr_matrix(a[None, :]), orthonormal=True), 7.0)
    for rho in (7.0, 91.0):
        check(ctx.L.pmh_op_penalized_set_penalty(Ar.h, rho))
        check(ctx.L.pmh_op_penalized_set_penalty(Ag.h, rho))
        o1, o2 = ctx.vec(N), ctx.vec(N)
        p0 = H.passes()
        Ar.mult(ctx.vec_from(v), o1)
        assert H.passes() - p0 == 2
        Ag.mult(ctx.vec_from(v), o2)
        ref = y * (X @ (X.T @ (y * v))) + rho * a * (a @ v)
        bound = _op_bound(X, v, ref, rho / N, extra_eps=6)
        e1, e2 = np.abs(o1.to_numpy() - ref), np.abs(o2.to_numpy() - ref)
        print("penalised rho", rho, "folded / generic max err / bound", (e1 / bound).max(), (e2 / bound).max())
        assert (e1 <= bound).all() and (e2 <= bound).all()
    # the folded operator on its own stays unpenalised
    o3 = ctx.vec(N)
    H.mult(ctx.vec_from(v), o3)
    ref = y * (X @ (X.T @ (y * v)))
    assert (np.abs(o3.to_numpy() - ref) <= _op_bound(X, v, ref, 0.0)).all()
    ctx.close()


# ---- 4. / 5. training against the oracle, the model, prediction ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["L1", "L2"])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_biased_training_against_the_oracle_sparse(oracle, name, loss):
    """The instances of the issue's table, rtol 1e-6, at most 100 outer iterations; the CPU oracle needs (outer / inner) A: 21 / 871 (L1), 29 / 366 (L2);
    B: 25 / 1263, 16 / 543; C: 14 / 375, 12 / 283.  Then, from the returned dual solution alone, feasibility and the KKT residual SMALXE's stopping test bounds,
    the model against numpy, and prediction on the 2000 held-out samples (derivations: test_gpu_svm_train.py::test_biased_training_against_the_oracle)."""
    args = INST[name]
    p = P.svm_sparse(*args, N_test=2000)
    X, y, n, Cc = p["X"], p["y"], p["n"], p["C"]
    Xa = abs(X)
    cmax, kmax = _cmax_kmax(X)
    ref = _oracle_train(oracle, p, loss)
    ctx = pa.Context(0)
    svm = pa.SVM(ctx, loss=loss, C=Cc, bias=True, options="-qps_rtol 1e-6 -qps_max_it 100").fit(X, y)
    st, a = svm.stats, svm.alpha
    print(name, loss, "HIP outer/inner", st.outer_iterations, st.inner_iterations, "oracle", ref["iteration"], ref["inner_iter_accu"], "reason", st.reason, ref["reason"])
    assert st.reason == ref["reason"] == 2
    assert abs(st.outer_iterations - ref["iteration"]) <= max(3, ref["iteration"] // 6)
    assert abs(st.inner_iterations - ref["inner_iter_accu"]) <= max(3, ref["inner_iter_accu"] // 6)
    sh = 0.0 if loss == "L1" else 1.0 / Cc
    w, w_ref = X.T @ (y * a), X.T @ (y * ref["u"])
    f = lambda z: 0.5 * np.dot(X.T @ (y * z), X.T @ (y * z)) + 0.5 * sh * z @ z - z.sum()
    print(name, loss, "w rel", np.linalg.norm(w - w_ref) / np.linalg.norm(w_ref), "f rel", abs(f(a) - f(ref["u"])) / abs(f(ref["u"])))
    assert np.linalg.norm(w - w_ref) <= 1e-3 * np.linalg.norm(w_ref)
    assert abs(f(a) - f(ref["u"])) <= 1e-6 * abs(f(ref["u"]))

    # optimality from alpha alone
    thr = 1e-6 * np.sqrt(n)
    assert a.min() >= -ASTOL and (loss == "L2" or a.max() <= Cc + ASTOL)
    eq_round = 2 * gamma(n) * np.abs(a).sum() / np.sqrt(n)
    print(name, loss, "|y'a|/sqrt(n)", abs(y @ a) / np.sqrt(n), "thr", thr, "+ rounding", eq_round)
    assert abs(y @ a) / np.sqrt(n) <= thr + eq_round
    assert abs(st.yTalpha - y @ a) <= 2 * gamma(n) * np.abs(a).sum()
    Wc = Xa.T @ np.abs(a)
    g = y * (X @ w) + sh * a - 1.0 + st.b_multiplier * y
    e = 2 * gamma(cmax + kmax + 2) * (Xa @ Wc) + 4 * EPS * (np.abs(g) + 1.0) + EPS * abs(st.b_multiplier)
    lo, hi = a <= ASTOL, (a >= Cc - ASTOL) if loss == "L1" else np.zeros(n, bool)
    gP = np.where(lo, np.minimum(g, 0.0), np.where(hi, np.maximum(g, 0.0), g))
    kkt = thr + np.linalg.norm(e)
    print(name, loss, "|gP|", np.linalg.norm(gP), "thr", thr, "+ rounding", np.linalg.norm(e))
    assert np.linalg.norm(gP) <= kkt

    # the model
    w_np, b_np, free = _np_model(p, a, loss)
    assert free.sum() > 0 and st.n_free_sv == free.sum() and st.n_sv == (a > ASTOL).sum()
    assert (np.abs(svm.w - w_np) <= 2 * gamma(cmax + 1) * Wc).all()
    db = 2 * gamma(kmax + 1) * float(np.mean(Xa[free] @ np.abs(w_np))) + 2 * gamma(cmax + 1) * float(np.mean(Xa[free] @ Wc)) + gamma(int(free.sum()) + 2) * (1 + abs(b_np))
    print(name, loss, "b", svm.b, "numpy", b_np, "bound", db, "multiplier", st.b_multiplier)
    assert abs(svm.b - b_np) <= db and svm.b == st.b_free
    nf = int(free.sum())
    b_tie = kkt / np.sqrt(nf) + sh * (abs(y @ a) + n * ASTOL) / nf + db
    print(name, loss, "|b_free - b_mult|", abs(st.b_multiplier - st.b_free), "bound", b_tie)
    assert abs(st.b_multiplier - st.b_free) <= b_tie

    # prediction on the held-out samples (other row counts than the training set's, the same d)
    Xt, yt = p["X_test"], p["y_test"]
    Xta = abs(Xt)
    kt = _cmax_kmax(Xt)[1]
    sc_np = Xt @ w_np + b_np
    sb = 2 * gamma(max(kmax, kt) + 2) * (Xta @ np.abs(w_np) + abs(b_np)) + Xta @ (2 * gamma(cmax + 1) * Wc) + db
    sc = svm.decision_function(Xt)
    print(name, loss, "scores: max err / bound", (np.abs(sc - sc_np) / sb).max())
    assert (np.abs(sc - sc_np) <= sb).all()
    sure = np.abs(sc_np) > sb
    print(name, loss, "test samples left out of the label comparison:", int((~sure).sum()), "of", sure.size)
    assert (~sure).sum() <= 0.01 * sure.size
    lab = svm.predict(Xt)
    assert set(np.unique(lab)) <= {-1.0, 1.0} and np.array_equal(lab[sure], np.where(sc_np >= 0, 1.0, -1.0)[sure])
    t = svm.test(Xt, yt)
    _check_counts(t, sc_np, yt, sure)
    if name in ("A", "B"):  # the labels carry an offset: the bias term is what this data needs
        flat = pa.SVM(ctx, loss=loss, C=Cc, bias=False, options="-qps_rtol 1e-6").fit(X, y)
        acc_flat = flat.test(Xt, yt)["accuracy"]
        print(name, loss, "held-out accuracy with bias", t["accuracy"], "without", acc_flat)
        assert t["accuracy"] > acc_flat
    ctx.close()


def test_sparse_model_predicts_dense_samples_and_back():
    """d <= 256: a model trained on sparse samples scores dense test samples through pmh_svm_predict, and a model trained on dense samples scores sparse ones
    through pmh_svm_predict_csr; both within the dot-product bound of numpy's scores from the model's own w and b."""
    p = P.svm_sparse(1500, 200, 12, 1.0, 0.5, 1.0, N_test=300)
    X, y, Xt = p["X"], p["y"], p["X_test"]
    ctx = pa.Context(0)
    for Xtrain in (X, X.toarray()):
        svm = pa.SVM(ctx, loss="L1", C=1.0, bias=True, options="-qps_rtol 1e-6").fit(Xtrain, y)
        assert svm.stats.reason == 2
        w, b = svm.w, svm.b
        ref = Xt @ w + b
        bound = 2 * gamma(200 + 2) * (abs(Xt) @ np.abs(w) + abs(b))
        s_sparse, s_dense = svm.decision_function(Xt), svm.decision_function(Xt.toarray())
        assert (np.abs(s_sparse - ref) <= bound).all() and (np.abs(s_dense - ref) <= bound).all()
        sure = np.abs(ref) > bound
        assert np.array_equal(svm.predict(Xt)[sure], svm.predict(Xt.toarray())[sure])
    ctx.close()


# ---- 6. - 8. no bias: the plain MPGP solve; reproducibility; the one-rank communicator ---------------------------------------------------------------------
def test_unbiased_l1_fit_is_the_plain_mpgp_solve_sparse():
    ctx = pa.Context(0)
    p = P.svm_sparse(*INST["A"])
    H, st, x = _solve(ctx, p)
    svm = pa.SVM(ctx, loss="L1", C=1.0, bias=False, options="-qps_rtol 1e-6").fit(p["X"], p["y"])
    s = svm.stats
    assert st.reason == 2 and np.array_equal(svm.alpha, x)
    assert (s.inner_iterations, s.nmv, s.ncg, s.nexp, s.nprop, s.reason) == (st.iteration, st.nmv, st.ncg, st.nexp, st.nprop, st.reason)
    assert svm.b == 0.0
    ctx.close()


def test_training_is_reproducible_bit_for_bit():
    ctx = pa.Context(0)
    p = P.svm_sparse(*INST["A"])
    runs = []
    for _ in range(2):
        svm = pa.SVM(ctx, loss="L1", C=1.0, bias=True, options="-qps_rtol 1e-6 -qps_max_it 100").fit(p["X"], p["y"])
        s = svm.stats
        runs.append((svm.alpha, svm.w, (s.reason, s.outer_iterations, s.inner_iterations, s.nmv, s.ncg, s.nexp, s.nprop)))
        svm.destroy()
    assert runs[0][2] == runs[1][2] and runs[0][2][0] == 2
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    ctx.close()


def test_single_rank_communicator_sparse():
    """The unbiased MPGP solve on the sparse operator under a 1-rank communicator (the all-reduce of w is live) against the local mode: equal counters, the same
    iterate bit for bit."""
    os.environ["PMH_COMM_FORCE"] = "1"
    try:
        ctx = pa.Context(0)
        ctx.comm_init(0, 1, ctx.comm_unique_id())
        p = P.svm_sparse(*INST["B"])
        _, st_d, x_d = _solve(ctx, p, distributed=True)
        _, st_l, x_l = _solve(ctx, p, distributed=False)
        assert st_d.reason == 2
        assert (st_d.iteration, st_d.nmv, st_d.ncg, st_d.nexp, st_d.nprop, st_d.reason) == (st_l.iteration, st_l.nmv, st_l.ncg, st_l.nexp, st_l.nprop, st_l.reason)
        assert np.array_equal(x_d, x_l)
        # no samples on a rank: the dense operator's error
        E = pa.CsrMat(ctx, 0, 5, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
        yd = ctx.vec(1)
        h = C.c_void_p()
        check(ctx.L.pmh_op_create_svm_dual_csr(ctx.h, E.h, yd.p, C.byref(h)))
        rc = ctx.L.pmh_op_mult(h, yd.p, yd.p)
        assert rc == PMH_ERR_ARG and b"holds no samples" in ctx.L.pmh_last_error()
        ctx.L.pmh_op_destroy(h)
        ctx.close()
    finally:
        del os.environ["PMH_COMM_FORCE"]


def test_no_samples_without_a_communicator_is_a_no_op():
    ctx = pa.Context(0)
    E = pa.CsrMat(ctx, 0, 5, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    yd = ctx.vec(1)
    h = C.c_void_p()
    check(ctx.L.pmh_op_create_svm_dual_csr(ctx.h, E.h, yd.p, C.byref(h)))
    k = C.c_longlong(-1)
    check(ctx.L.pmh_op_mult(h, yd.p, yd.p))
    check(ctx.L.pmh_op_svm_dual_passes(h, C.byref(k)))
    assert k.value == 0  # no launch
    ctx.L.pmh_op_destroy(h)
    ctx.close()


def test_empty_columns_and_all_empty_matrix():
    """A matrix without any stored entry: w = 0, H v = 0 (plain) and sigma s y + shift v (augmented)."""
    ctx = pa.Context(0)
    N, d = 300, 17
    y = np.where(np.random.default_rng(4).random(N) < 0.5, -1.0, 1.0)
    v = np.random.default_rng(5).standard_normal(N)
    H = pa.MatCreateSVMDual(ctx, sp.csr_matrix((N, d)), y)
    out = ctx.vec_from(np.full(N, 7.0))
    H.mult(ctx.vec_from(v), out)
    assert np.array_equal(out.to_numpy(), np.zeros(N))
    H.set_terms(0.5, 2.0)
    H.mult(ctx.vec_from(v), out)
    ref = 2.0 * y * (y @ v) + 0.5 * v
    assert (np.abs(out.to_numpy() - ref) <= 2 * (2.0 * gamma(N + 2) * np.abs(v).sum() + 4 * EPS * np.abs(ref))).all()
    ctx.close()


# ---- 9. errors through the C entries -----------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    ctx = pa.Context(0)
    L = ctx.L
    p = P.svm_sparse(600, 300, 8, 1.0, 0.5, 1.0)
    X, y = p["X"], p["y"]
    yd = ctx.vec_from(y)
    o = _lib.SvmOpts()
    check(L.pmh_svm_default_opts(o))

    def err(rc, *words):
        msg = L.pmh_last_error().decode()
        assert rc == PMH_ERR_ARG, (rc, msg)
        assert msg and all(w in msg for w in words), msg

    # a column index >= d: refused where the matrix is made
    h = C.c_void_p()
    rp, col, val = np.array([0, 2], np.int32), np.array([1, 300], np.int32), np.ones(2)
    err(L.pmh_csr_create(ctx.h, 1, 300, rp.ctypes.data_as(C.c_void_p), col.ctypes.data_as(C.c_void_p), val.ctypes.data_as(C.c_void_p), C.byref(h)), "out of range")
    # unsorted columns: refused by the operator and by the front end
    rp, col, val = np.array([0, 3, 4], np.int32), np.array([5, 2, 7, 1], np.int32), np.ones(4)
    U = pa.CsrMat(ctx, 2, 300, rp, col, val)
    y2 = ctx.vec_from(np.array([1.0, -1.0]))
    err(L.pmh_op_create_svm_dual_csr(ctx.h, U.h, y2.p, C.byref(h)), "not sorted", "sample 0")
    err(L.pmh_svm_create_csr(ctx.h, U.h, y2.p, o, C.byref(h)), "not sorted")
    # C <= 0
    Xc = pa.mat.csr_from_scipy(ctx, X)
    o.C = 0.0
    err(L.pmh_svm_create_csr(ctx.h, Xc.h, yd.p, o, C.byref(h)), "C = 0")
    o.C = 1.0
    # d mismatch at prediction
    svm = pa.SVM(ctx, loss="L1", C=1.0, bias=True, options="-qps_rtol 1e-4").fit(X, y)
    T = pa.CsrMat(ctx, 2, 299, np.array([0, 1, 2], np.int32), np.array([3, 4], np.int32), np.ones(2))
    sc = ctx.vec(2)
    err(L.pmh_svm_predict_csr(svm.h, T.h, sc.p, None), "299", "300")
    cnt = (C.c_longlong * 4)()
    err(L.pmh_svm_test_csr(svm.h, T.h, y2.p, cnt), "299", "300")
    # a model wider than the dense kernels take, asked to score dense rows
    dense = ctx.vec(2 * 300)
    err(L.pmh_svm_predict(svm.h, 2, dense.p, sc.p, None), "d = 300")
    # Python: a sparse matrix of another width
    with pytest.raises(ValueError):
        svm.decision_function(sp.csr_matrix((2, 299)))
    ctx.close()
