"""Sample subsets on the SVM dual operator and the SVM handle (pmh_op_svm_dual_set_subset, pmh_svm_set_subset), scoring of the handle's own rows
(pmh_svm_predict_own, pmh_svm_test_own) and cross_validate on top.  The held-out set of every test is {0} u [64, 192) u {i : i % 5 == 3} u {n - 1}: the first
row, two whole 64-row workgroups, isolated rows, one row of a half-wave pair, the last row.  Bounds and tolerances are those of test_gpu_svm_train.py and
test_gpu_svm_sparse.py (test_augmented_operator_against_numpy, test_biased_training_against_the_oracle), restated for the subset: sums run over S, n_S stands
where n stood."""
import numpy as np
import pytest

import permon_amd as pa
from permon_amd import _lib
from permon_amd import problems as P
from permon_amd.svm import cross_validate, kfold
from svm_train_cases import ASTOL, EPS, gamma, check_counts, np_model, oracle_train

pytestmark = pytest.mark.gpu
PMH_ERR_ARG, PMH_ERR_STATE = 2, 3
OPTS = "-qps_rtol 1e-6 -qps_max_it 100"


def train_mask(n):
    h = np.zeros(n, dtype=bool)
    h[0] = h[n - 1] = True
    h[64:192] = True
    h[3::5] = True
    return ~h


_DATA = {}


def data(kind):
    """The issue's instances, drawn once: dense 2000 x 64, 1500 x 37, 1500 x 130 and CSR 1500 x 300; "dense64_tail": 2003 rows, no multiple of the 8 rows a
    wave has in flight."""
    if kind not in _DATA:
        if kind == "csr":
            _DATA[kind] = P.svm_sparse(1500, 300, 12, 1.2, 0.5, 1.0)
        elif kind == "dense64_tail":
            _DATA[kind] = P.svm_offset(2003, 64, 3.0)
        else:
            d = int(kind[5:])
            _DATA[kind] = P.svm_offset(2000, 64, 3.0) if d == 64 else P.svm_offset(1500, d, 2.0)
    return _DATA[kind]


def sums(X):
    """(cmax, kmax): the longest sums of pass 1 and of a row's dot product (dense: N and d)."""
    if hasattr(X, "tocsr"):
        X = X.tocsr()
        return int(np.bincount(X.indices, minlength=X.shape[1]).max()), int(np.diff(X.indptr).max())
    return X.shape


def rows(X, m):
    return X[m] if not hasattr(X, "tocsr") else X.tocsr()[np.flatnonzero(m)]


# ---- 1. the operator against numpy ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dense64", "dense64_tail", "dense37", "dense130", "csr"])
def test_subset_operator_against_numpy(kind):
    """out = m o ((H + D)(m o v)) with the sigma term over S, in the plain, shift, diagonal and sigma forms, within the bound of
    test_augmented_operator_against_numpy (the sums are at most as long as there); held-out rows exactly 0; held-out entries of v without effect, a NaN or 1e300
    included."""
    p = data(kind)
    X, y, n = p["X"], p["y"], p["n"]
    m = train_mask(n)
    mf = m.astype(float)
    Xa = abs(X)
    cmax, kmax = sums(X)
    rng = np.random.default_rng(1)
    v = rng.standard_normal(n)
    assert (v[~m] != 0).all()
    v2 = v.copy()
    v2[~m] = np.where(np.arange((~m).sum()) % 2 == 0, np.nan, 1e300)
    dg = rng.uniform(0.5, 2.0, n)
    ctx = pa.Context(0)
    H = pa.MatCreateSVMDual(ctx, X, y)
    H.set_subset(m)
    vd, v2d = ctx.vec_from(v), ctx.vec_from(v2)
    mv = mf * v
    Hv = y * (X @ (X.T @ (y * mv)))
    for name, shift, diag, sigma in [("plain", 0.0, None, 0.0), ("shift", 1.0 / 0.7, None, 0.0), ("diag", 0.0, dg, 0.0), ("shift+sigma", 1.0 / 0.7, None, 2.5), ("diag+sigma", 0.0, dg, 2.5)]:
        H.set_diag(None), H.set_terms(shift, sigma), H.set_diag(diag)  # (the subset survives both)
        D = dg if diag is not None else shift
        ref = mf * (Hv + D * mv + sigma * y * (y @ mv))
        bound = 2 * (gamma(cmax + kmax + 2) * (Xa @ (Xa.T @ np.abs(mv))) + sigma * gamma(n + 2) * np.abs(mv).sum() + 4 * EPS * np.abs(ref))
        out, out2 = ctx.vec(n), ctx.vec(n)
        H.mult(vd, out), H.mult(v2d, out2)
        o = out.to_numpy()
        err = np.abs(o - ref)
        print(kind, name, "max err / bound", (err[m] / bound[m]).max())
        assert np.isfinite(o).all() and (err <= bound).all()
        assert (o[~m] == 0.0).all()
        assert np.array_equal(o, out2.to_numpy())
    # all samples again: the plain operator's bits
    H.set_diag(None), H.set_terms(0.0, 0.0), H.set_subset(None)
    o1, o2 = ctx.vec(n), ctx.vec(n)
    H.mult(vd, o1), pa.MatCreateSVMDual(ctx, X, y).mult(vd, o2)
    assert np.array_equal(o1.to_numpy(), o2.to_numpy())
    ctx.close()


# ---- 2. held-out rows are not read -----------------------------------------------------------------------------------------------------------------------------
STAT_FIELDS = [f for f, _ in _lib.SvmStats._fields_]


def _stats(st):
    return tuple(getattr(st, f) for f in STAT_FIELDS)


@pytest.mark.parametrize("loss", ["L1", "L2"])
@pytest.mark.parametrize("d", [64, 37, 130])
def test_held_out_rows_are_not_used(d, loss):
    """A handle whose X has NaN in the held-out rows trains to the bits of the handle on X: no load of a held-out row reaches a sum.  pmh_svm_create builds a
    solver on ALL rows (its eigenvalue estimate multiplies by the whole X, and a NaN there is refused as a bad penalty), so the NaN rows are written into the
    handle's device copy of X right after creation: set_subset, which builds the solver anew over S, and train then run on the NaN copy."""
    p = data("dense%d" % d)
    X, y, n = p["X"], p["y"], p["n"]
    m = train_mask(n)
    Xn = X.copy()
    Xn[~m] = np.nan
    ctx = pa.Context(0)
    res = []
    for Xk in (X, Xn):
        svm = pa.SVM(ctx, loss=loss, C=p["C"], bias=True, options=OPTS).create(X, y)
        svm._keep[0].set_numpy(Xk.ravel())
        svm.set_subset(m).train()
        res.append((svm.alpha, svm.w, svm.b, _stats(svm.stats)))
        svm.destroy()
    (a1, w1, b1, s1), (a2, w2, b2, s2) = res
    print(d, loss, "outer/inner", s1[1], s1[2], "n_sv", s1[STAT_FIELDS.index("n_sv")])
    assert s1[0] == 2
    assert np.isfinite(a2).all() and np.isfinite(w2).all() and np.isfinite(b2) and np.isfinite(np.array(s2, dtype=float)).all()
    assert np.array_equal(a1, a2) and np.array_equal(w1, w2) and b1 == b2 and s1 == s2
    ctx.close()


def _fixed(ctx, X, y, m, rho, iters, own_term=False):
    """`iters` MPGP iterations on H_S + rho B'B, B the row (m o y) / sqrt(n_S): through the penalised operator, or (own_term) as the operator's own rank-one term."""
    n, nS = y.size, int(m.sum())
    H = pa.MatCreateSVMDual(ctx, X, y)
    H.set_subset(m)
    if own_term:
        H.set_terms(0.0, rho / nS)
        A = H
    else:
        A = pa.MatCreatePenalized(H, pa.QPPF.onerow(ctx, m * y / np.sqrt(nS)), rho)
    qp = pa.QP(ctx)
    qp.SetOperator(A)
    qp.SetRhs(ctx.vec_from(m.astype(float)))
    x = ctx.vec_from(np.zeros(n))
    qp.SetInitialVector(x)
    qp.SetBox(None, ctx.vec_from(np.zeros(n)), ctx.vec_from(np.ones(n)))
    qps = pa.QPS(ctx)
    qps.SetQP(qp)
    qps.SetType("mpgp")
    qps.SetUp()
    p0 = H.passes()
    st = qps.RunFixed(iters)
    return st, H.passes() - p0, x.to_numpy()


def test_paired_passes_under_a_subset():
    """d = 64, the bias equality folded, pairing on (k_svm_x64_grad / k_svm_x64_p1 with the subset): NaN held-out rows change no bit of the iterate (2.), the
    passes over X per product stay below 2 with expansion steps taken (6., as test_bias_costs_no_pass_over_X), and the folded equality costs what the
    operator's own rank-one term costs: the same steps, the same passes."""
    p = data("dense64")
    X, y, n = p["X"], p["y"], p["n"]
    m = train_mask(n)
    Xn = X.copy()
    Xn[~m] = np.nan
    ctx = pa.Context(0)
    st1, pass1, x1 = _fixed(ctx, X, y, m, 500.0, 60)
    st2, pass2, x2 = _fixed(ctx, Xn, y, m, 500.0, 60)
    st3, pass3, x3 = _fixed(ctx, X, y, m, 500.0, 60, own_term=True)
    print("folded", (st1.nmv, st1.ncg, st1.nexp, st1.nprop, pass1), "NaN rows", (st2.nmv, st2.ncg, st2.nexp, st2.nprop, pass2), "own term", (st3.nmv, st3.ncg, st3.nexp, st3.nprop, pass3))
    assert np.isfinite(x2).all() and np.array_equal(x1, x2) and (x1[~m] == 0.0).all() and np.abs(x1).max() > 0
    assert (st1.nmv, st1.ncg, st1.nexp, st1.nprop, pass1) == (st2.nmv, st2.ncg, st2.nexp, st2.nprop, pass2)
    assert (st1.nmv, st1.ncg, st1.nexp, st1.nprop, pass1) == (st3.nmv, st3.ncg, st3.nexp, st3.nprop, pass3)
    assert pass1 / st1.nmv < 2.0 and st1.nexp > 0
    ctx.close()


# ---- 3. against a fresh handle and the CPU oracle on (X[m], y[m]) ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["L1", "L2"])
@pytest.mark.parametrize("kind", ["dense64", "dense37", "csr"])
def test_subset_training_against_fresh_handle_and_oracle(oracle, kind, loss):
    p = data(kind)
    X, y, n, Cc = p["X"], p["y"], p["n"], p["C"]
    m = train_mask(n)
    nS = int(m.sum())
    Xs, ys = rows(X, m), y[m]
    ps = dict(X=Xs, y=ys, n=nS, C=Cc, b=np.ones(nS), x0=np.zeros(nS), lb=np.zeros(nS), ub=np.full(nS, Cc))
    ref = oracle_train(oracle, ps, loss)
    ctx = pa.Context(0)
    fresh = pa.SVM(ctx, loss=loss, C=Cc, bias=True, options=OPTS).fit(Xs, ys)
    svm = pa.SVM(ctx, loss=loss, C=Cc, bias=True, options=OPTS).create(X, y).set_subset(m).train()
    st, a = svm.stats, svm.alpha
    print(kind, loss, "subset outer/inner", st.outer_iterations, st.inner_iterations, "fresh", fresh.stats.outer_iterations, fresh.stats.inner_iterations, "oracle", ref["iteration"], ref["inner_iter_accu"])
    assert st.reason == ref["reason"] == 2
    assert (a[~m] == 0.0).all()
    assert abs(st.outer_iterations - ref["iteration"]) <= max(3, ref["iteration"] // 6)
    assert abs(st.inner_iterations - ref["inner_iter_accu"]) <= max(3, ref["inner_iter_accu"] // 6)
    sh = 0.0 if loss == "L1" else 1.0 / Cc
    am = a[m]
    f = lambda z: 0.5 * np.dot(Xs.T @ (ys * z), Xs.T @ (ys * z)) + 0.5 * sh * z @ z - z.sum()
    w = Xs.T @ (ys * am)
    for who, z in (("oracle", ref["u"]), ("fresh", fresh.alpha)):
        wz = Xs.T @ (ys * z)
        print(kind, loss, who, "w rel", np.linalg.norm(w - wz) / np.linalg.norm(wz), "f rel", abs(f(am) - f(z)) / abs(f(z)))
        assert np.linalg.norm(w - wz) <= 1e-3 * np.linalg.norm(wz)
        assert abs(f(am) - f(z)) <= 1e-6 * abs(f(z))
    # the equality over S: SMALXE's threshold with n_S in place of n, plus the recomputation's rounding
    thr = 1e-6 * np.sqrt(nS)
    eq_round = 2 * gamma(nS) * np.abs(am).sum() / np.sqrt(nS)
    print(kind, loss, "|y'a|/sqrt(n_S)", abs(ys @ am) / np.sqrt(nS), "thr", thr, "+ rounding", eq_round)
    assert abs(ys @ am) / np.sqrt(nS) <= thr + eq_round
    assert am.min() >= -ASTOL and (loss == "L2" or am.max() <= Cc + ASTOL)
    # the model from alpha: counts equal numpy's, b within the rounding of its mean
    w_np, b_np, free = np_model(ps, am, loss)
    assert free.sum() > 0 and st.n_free_sv == free.sum() and st.n_sv == (am > ASTOL).sum()
    cmax, kmax = sums(Xs)
    Xsa = abs(Xs)
    Wc = Xsa.T @ np.abs(am)
    assert (np.abs(svm.w - w_np) <= 2 * gamma(cmax + 1) * Wc).all()
    db = 2 * gamma(kmax + 1) * float(np.mean(Xsa[free] @ np.abs(w_np))) + 2 * gamma(cmax + 1) * float(np.mean(Xsa[free] @ Wc)) + gamma(int(free.sum()) + 2) * (1 + abs(b_np))
    print(kind, loss, "b", svm.b, "numpy", b_np, "bound", db, "multiplier", st.b_multiplier, "fresh", fresh.b)
    assert abs(svm.b - b_np) <= db and svm.b == st.b_free
    ctx.close()


# ---- 4. state ------------------------------------------------------------------------------------------------------------------------------------------------
def _model(svm):
    svm.train()
    return svm.alpha, svm.w, svm.b


def _same(r1, r2):
    return np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1]) and r1[2] == r2[2]


@pytest.mark.parametrize("loss", ["L1", "L2"])
@pytest.mark.parametrize("kind", ["dense64", "csr"])
def test_subset_state(kind, loss):
    p = data(kind)
    X, y, n, Cc = p["X"], p["y"], p["n"], p["C"]
    m = train_mask(n)
    ctx = pa.Context(0)
    new = lambda: pa.SVM(ctx, loss=loss, C=Cc, bias=True, options=OPTS).create(X, y)
    s = new()
    assert s.subset is None
    r0 = _model(s)
    s.set_subset(m)
    assert np.array_equal(s.subset, m)
    rm = _model(s)
    assert (rm[0][~m] == 0.0).all() and not _same(r0, rm)
    s.set_subset(None)
    assert s.subset is None and _same(_model(s), r0)
    # labels and penalties commute with the subset
    y2 = y.copy()
    y2[::7] *= -1.0
    wt = np.random.default_rng(2).uniform(0.5, 2.0, n)
    s1, s2 = new(), new()
    r1 = _model(s1.set_subset(m).set_labels(y2))
    r2 = _model(s2.set_labels(y2).set_subset(m))
    assert _same(r1, r2) and (r1[0][~m] == 0.0).all() and not _same(r1, rm)
    r1 = _model(s1.set_penalties(2.0, 0.5, wt))
    r2 = _model(new().set_labels(y2).set_penalties(2.0, 0.5, wt).set_subset(m))
    assert _same(r1, r2) and (r1[0][~m] == 0.0).all() and np.array_equal(s1.subset, m)
    # a new subset clears the calibration
    s.set_subset(None).train()
    s.set_calibration(-2.0, 0.1)
    Xt = rows(X, np.arange(n) < 50)
    assert s.predict_proba(Xt).shape == (50,)
    s.set_subset(m).train()
    with pytest.raises(_lib.PermonHipError) as e:
        s.predict_proba(Xt)
    assert e.value.code == PMH_ERR_STATE
    # refused masks leave the handle as it was
    before = _model(s)
    for bad in (np.where(np.arange(n) == 5, 0.5, 1.0), np.where(np.arange(n) == 5, np.nan, 1.0), np.zeros(n)):
        with pytest.raises(_lib.PermonHipError) as e:
            s.set_subset(bad)
        assert e.value.code == PMH_ERR_ARG
    with pytest.raises(ValueError):
        s.set_subset(np.ones(n - 1))
    assert np.array_equal(s.subset, m) and _same(_model(s), before)
    ctx.close()


# ---- 5. scoring the handle's own rows ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dense64", "dense37", "csr"])
def test_own_row_scoring(kind):
    p = data(kind)
    X, y, n, Cc = p["X"], p["y"], p["n"], p["C"]
    m = train_mask(n)
    ctx = pa.Context(0)
    svm = pa.SVM(ctx, loss="L1", C=Cc, bias=True, options=OPTS).create(X, y)
    svm.train()
    with pytest.raises(_lib.PermonHipError) as e:
        svm.test_own("held_out")
    assert e.value.code == PMH_ERR_STATE
    assert svm.test_own("subset") == svm.test_own("all") == svm.test(X, y)
    svm.set_subset(m).train()
    sc = svm.decision_function_own()
    assert np.array_equal(sc, svm.decision_function(X))
    # numpy's scores and the dot-product bound of the existing tests: which labels the score decides beyond rounding
    a = svm.alpha
    Xs, ys, am = rows(X, m), y[m], a[m]
    w_np, b_np, free = np_model(dict(X=Xs, y=ys, C=Cc), am, "L1")
    cmax, kmax = sums(Xs)
    Xa, Xsa = abs(X), abs(Xs)
    Wc = Xsa.T @ np.abs(am)
    db = 2 * gamma(kmax + 1) * float(np.mean(Xsa[free] @ np.abs(w_np))) + 2 * gamma(cmax + 1) * float(np.mean(Xsa[free] @ Wc)) + gamma(int(free.sum()) + 2) * (1 + abs(b_np))
    sc_np = X @ w_np + b_np
    sb = 2 * gamma(sums(X)[1] + 2) * (Xa @ np.abs(w_np) + abs(b_np)) + Xa @ (2 * gamma(cmax + 1) * Wc) + db
    assert (np.abs(sc - sc_np) <= sb).all()
    sure = np.abs(sc_np) > sb
    print(kind, "rows left out of the label comparison:", int((~sure).sum()), "of", n)
    assert (~sure).sum() <= 0.01 * n
    t = {}
    for which, sel in (("held_out", ~m), ("subset", m), ("all", np.ones(n, dtype=bool))):
        t[which] = svm.test_own(which)
        check_counts(t[which], sc_np[sel], y[sel], sure[sel])
    for k in ("TP", "FP", "TN", "FN"):
        assert t["held_out"][k] + t["subset"][k] == t["all"][k]
    print(kind, "accuracy held out", t["held_out"]["accuracy"], "subset", t["subset"]["accuracy"])
    ctx.close()


# ---- 7. cross_validate ---------------------------------------------------------------------------------------------------------------------------------------
def test_cross_validate():
    p = data("dense64")
    X, y, n, Cc = p["X"], p["y"], p["n"], p["C"]
    ctx = pa.Context(0)
    svm = pa.SVM(ctx, loss="L1", C=Cc, bias=True, options=OPTS).create(X, y)
    cv = cross_validate(svm, k=5, seed=0)
    assert svm.subset is None and len(cv["folds"]) == 5
    masks = kfold(y, 5, seed=0)
    for mk, mc, f in zip(masks, cv["masks"], cv["folds"]):
        assert np.array_equal(mk, mc)
        assert svm.set_subset(mk).train().test_own("held_out") == f
        assert f["TP"] + f["FP"] + f["TN"] + f["FN"] == int((~mk).sum())
    assert cv["accuracy"] == float(np.mean([f["accuracy"] for f in cv["folds"]]))
    # the subset the handle had comes back
    m = train_mask(n)
    svm.set_subset(m)
    cv2 = cross_validate(svm, k=5, seed=0)
    assert np.array_equal(svm.subset, m) and cv2["folds"] == cv["folds"]
    flat = pa.SVM(ctx, loss="L1", C=Cc, bias=False, options="-qps_rtol 1e-6").create(X, y)
    cvf = cross_validate(flat, k=5, seed=0)
    print("5-fold accuracy with bias", cv["accuracy"], [f["accuracy"] for f in cv["folds"]], "without", cvf["accuracy"])
    assert cv["accuracy"] > cvf["accuracy"]  # the labels carry a planted offset
    ctx.close()
