"""GPU tests of the SVM probability model (csrc/svm_proba.hip and the proba kernels of svm_train.hip / svm_multi.hip): the Platt fit against its numpy
restatement, its reproducibility and edge cases, predict_proba against numpy's sigmoid of the handle's own scores, calibrate against platt_fit bit for bit, the
state rules, and the same for the one-vs-rest front end without any training (set_model)."""
import numpy as np
import pytest
import scipy.sparse as sp

import permon_amd as pa
import svm_proba_cases as PC
from permon_amd import problems as P
from permon_amd._lib import PermonHipError
from permon_amd.svm import platt_fit

pytestmark = pytest.mark.gpu
PMH_ERR_ARG, PMH_ERR_STATE = 2, 3
OPT = "-qps_rtol 1e-6"
EPS = PC.EPS


def _raises(code, f, *a):
    with pytest.raises(PermonHipError) as e:
        f(*a)
    assert e.value.code == code, str(e.value)
    return str(e.value)


# ---- 1. the fit against the restatement -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inst", PC.INSTANCES)
def test_fit_against_numpy(inst):
    ctx = pa.Context(0)
    f, y = PC.scores(*inst)
    ref = PC.platt_np(f, y)
    A, B, st = platt_fit(ctx, f, y)
    t, n_pos, n_neg = PC.targets(y)
    h = PC.sums(f, t, A, B)
    lam = float(np.linalg.eigvalsh(np.array([[h[3], h[5]], [h[5], h[4]]]))[0])
    dist = float(np.hypot(A - ref["A"], B - ref["B"]))
    print("platt", inst, "device (A, B) = (%.17g, %.17g) reason %d it %d ev %d | numpy's gradient there (%.3e, %.3e) | lambda_min %.4g | distance to numpy's point %.3e, bound %.3e"
          % (A, B, st.reason, st.iterations, st.evaluations, h[1], h[2], lam, dist, 2.0 * np.sqrt(2.0) * 1e-5 / lam + 1e-9))
    assert st.reason == PC.CONVERGED
    assert (st.n_pos, st.n_neg) == (n_pos, n_neg)
    assert abs(h[1]) < 1e-5 + 1e-9 and abs(h[2]) < 1e-5 + 1e-9
    assert dist <= 2.0 * np.sqrt(2.0) * 1e-5 / lam + 1e-9
    assert st.iterations <= 100 and st.evaluations >= st.iterations + 1
    ctx.close()


# ---- 2. two fits, the same bits ---------------------------------------------------------------------------------------------------------------------------------
def test_two_fits_give_equal_bits():
    ctx = pa.Context(0)
    f, y = PC.scores(2000, 0.1, 2)
    a = platt_fit(ctx, f, y)
    b = platt_fit(ctx, f, y)
    assert (a[0], a[1], a[2].fval) == (b[0], b[1], b[2].fval)
    assert (a[2].g1, a[2].g2, a[2].iterations, a[2].evaluations) == (b[2].g1, b[2].g2, b[2].iterations, b[2].evaluations)
    ctx.close()


# ---- 3. edge cases of the fit -----------------------------------------------------------------------------------------------------------------------------------
def test_fit_edge_cases():
    ctx = pa.Context(0)
    A, B, st = platt_fit(ctx, np.linspace(-1.0, 2.0, 50), np.ones(50))
    assert A == 0.0 and abs(B - np.log(1.0 / 51.0)) <= 1e-12
    assert (st.n_pos, st.n_neg, st.iterations) == (50, 0, 0)
    f, y = PC.separable_scores()
    A, B, st = platt_fit(ctx, f, y)
    print("separable: A %.6g B %.6g reason %d iterations %d evaluations %d" % (A, B, st.reason, st.iterations, st.evaluations))
    assert np.isfinite(A) and np.isfinite(B) and A < 0.0
    assert st.reason in (PC.CONVERGED, PC.MAX_IT, PC.LINE_SEARCH)
    f, y = PC.scores(257, 0.5, 1)
    y[100] = 0.5
    assert "1 of the 257 labels" in _raises(PMH_ERR_ARG, platt_fit, ctx, f, y)
    _raises(PMH_ERR_ARG, platt_fit, ctx, np.zeros(0), np.zeros(0))
    ctx.close()


# ---- 4. predict_proba against numpy -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained():
    """One trained handle per (shape, bias), with its samples; shared, and only calibrated (never re-trained) by the tests that use it."""
    ctx = pa.Context(0)
    made = {}

    def get(shape, bias):
        if (shape, bias) not in made:
            X, y = PC.samples(shape)
            made[(shape, bias)] = (pa.SVM(ctx, "L1", 1.0, bias, OPT).fit(X, y), X, y)
        return made[(shape, bias)]

    yield ctx, get
    for s, _, _ in made.values():
        s.destroy()
    ctx.close()


@pytest.mark.parametrize("bias", [0, 1])
@pytest.mark.parametrize("shape", PC.SHAPES)
def test_predict_proba_against_numpy(trained, shape, bias):
    ctx, get = trained
    s, X, y = get(shape, bias)
    S = s.decision_function(X)
    s.set_calibration(-0.8, 0.1)
    p = s.predict_proba(X)
    err = np.abs(p - PC.sigma(-0.8 * S + 0.1))
    print("predict_proba", shape, bias, ": max error %.2f eps, proba in [%.3g, %.3g]" % (err.max() / EPS, p.min(), p.max()))
    assert p.shape == S.shape
    assert (err <= 32.0 * EPS).all()
    # the order of the probabilities is the order of the scores
    o = np.argsort(S, kind="stable")
    assert (np.diff(p[o]) >= 0.0).all()
    assert np.array_equal(s.predict_proba(X), p)
    # a steep sigmoid saturates, it does not overflow
    s.set_calibration(-50.0, 0.0)
    q = s.predict_proba(X)
    assert np.isfinite(q).all() and (q >= 0.0).all() and (q <= 1.0).all()
    assert (np.diff(q[o]) >= 0.0).all()
    # a dense model scores the same test samples in CSR: the dot products are summed in another order, the scores agree to rounding and so do the probabilities
    # (the CSR model has d = 3000: dense test samples are refused, test_state_and_errors; a CSR model of d <= 256: test_sparse_model_scores_dense_samples)
    if shape != "csr":
        s.set_calibration(-0.8, 0.1)
        Xo = sp.csr_matrix(X)
        Xo.sort_indices()
        So, po = s.decision_function(Xo), s.predict_proba(Xo)
        assert (np.abs(po - PC.sigma(-0.8 * So + 0.1)) <= 32.0 * EPS).all()
        assert np.abs(po - p).max() <= 0.8 * 0.25 * np.abs(So - S).max() + 64.0 * EPS  # |sigma'| <= 1/4


def test_sparse_model_scores_dense_samples():
    """A model trained on CSR samples of d <= 256 scores dense test samples, and the other way round (test_predict_proba_against_numpy)."""
    ctx = pa.Context(0)
    p = P.svm_sparse(300, 200, 12, 1.0, 0.5)
    s = pa.SVM(ctx, "L1", 1.0, True, OPT).fit(p["X"], p["y"]).set_calibration(-0.8, 0.1)
    Xd = p["X"].toarray()
    for Xt in (p["X"], Xd):
        S = s.decision_function(Xt)
        assert (np.abs(s.predict_proba(Xt) - PC.sigma(-0.8 * S + 0.1)) <= 32.0 * EPS).all()
    s.destroy()
    ctx.close()


# ---- 5. calibrate is the fit of its own scores ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(300, 64), (257, 37), "csr"])
def test_calibrate_equals_platt_fit_of_the_scores(trained, shape):
    ctx, get = trained
    s, X, y = get(shape, 1)
    s.calibrate(X, y)
    A, B, st = platt_fit(ctx, s.decision_function(X), y)
    got, gst = s.calibration, s.calibration_stats
    print("calibrate", shape, got, "reason", gst.reason, "iterations", gst.iterations)
    assert got == (A, B)
    assert (gst.reason, gst.iterations, gst.evaluations, gst.n_pos, gst.n_neg, gst.fval, gst.g1, gst.g2) == (st.reason, st.iterations, st.evaluations, st.n_pos, st.n_neg, st.fval, st.g1, st.g2)
    # and predict_proba applies exactly that pair
    S = s.decision_function(X)
    assert (np.abs(s.predict_proba(X) - PC.sigma(A * S + B)) <= 32.0 * EPS).all()


# ---- 6. state ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_state_and_errors():
    ctx = pa.Context(0)
    X, y = PC.samples((257, 37))
    s = pa.SVM(ctx, "L1", 1.0, True, OPT).create(X, y)
    _raises(PMH_ERR_STATE, s.calibrate, X, y)  # untrained
    s.train()
    for _ in range(2):
        _raises(PMH_ERR_STATE, s.predict_proba, X)
        _raises(PMH_ERR_STATE, lambda: s.calibration)
        s.set_calibration(-1.25, 0.375)
        assert s.calibration == (-1.25, 0.375) and s.calibration_stats.reason == 0
        s.predict_proba(X)
        s.train()  # a new model: the calibration is gone
    for change in (lambda: s.set_labels(-y), lambda: s.set_penalties(2.0, 0.5)):
        s.set_calibration(-1.0, 0.0)
        change()
        _raises(PMH_ERR_STATE, s.set_calibration, -1.0, 0.0)  # untrained now
        s.train()
        _raises(PMH_ERR_STATE, s.predict_proba, X)
        _raises(PMH_ERR_STATE, lambda: s.calibration)
    s.calibrate(X, -y)
    assert s.calibration[0] < 0.0
    _raises(PMH_ERR_ARG, s.set_calibration, np.nan, 0.0)
    s.destroy()
    # the dense test-sample limit is predict's, with predict's text
    Xc, yc = PC.samples("csr")
    s = pa.SVM(ctx, "L1", 1.0, True, OPT).fit(Xc, yc).set_calibration(-1.0, 0.0)
    assert "dense test samples need d <= 256, the model has d = 3000" in _raises(PMH_ERR_ARG, s.predict_proba, np.zeros((2, 3000)))
    s.destroy()
    ctx.close()


# ---- 7. multiclass, no training ---------------------------------------------------------------------------------------------------------------------------------
def _multi_handle(ctx, case):
    K, d, sparse = case
    X, labels, W, b = PC.multi_case(*case)
    m = pa.SVMMulticlass(ctx, options=OPT).create(X, labels)
    assert m.K == K
    return m.set_model(W, b), X, labels


def _normalised(S, A, B):
    sg = PC.sigma(A * S + B)
    tot = np.zeros(S.shape[0])
    for k in range(S.shape[1]):  # k ascending, as the kernel sums
        tot = tot + sg[:, k]
    with np.errstate(all="ignore"):
        return np.where(tot[:, None] == 0.0, 1.0 / S.shape[1], sg / tot[:, None])


@pytest.mark.parametrize("case", PC.MULTI)
def test_multiclass_predict_proba_and_calibrate(case):
    K = case[0]
    ctx = pa.Context(0)
    m, X, labels = _multi_handle(ctx, case)
    S = m.decision_function(X)
    A, B = -0.5 - 0.1 * np.arange(K), 0.05 * np.arange(K) - 0.1
    m.set_calibration(A, B)
    assert np.array_equal(m.calibration[0], A) and np.array_equal(m.calibration[1], B)
    PR = m.predict_proba(X)
    ref = _normalised(S, A, B)
    print("multi predict_proba", case, ": max |row sum - 1| %.2f eps, max error %.2f eps" % (np.abs(PR.sum(axis=1) - 1.0).max() / EPS, np.abs(PR - ref).max() / EPS))
    assert PR.shape == (X.shape[0], K)
    assert (np.abs(PR.sum(axis=1) - 1.0) <= 4.0 * EPS).all()
    assert (np.abs(PR - ref) <= 64.0 * EPS).all()
    assert np.array_equal(m.predict_proba(X), PR)
    # scoring is what it was: the arg-max of the raw scores
    assert np.array_equal(m.predict(X), m.classes_[np.argmax(S, axis=1)]) and np.array_equal(m.decision_function(X), S)
    # every sigmoid underflows to 0: 1 / K
    m.set_calibration(np.zeros(K), np.full(K, 800.0))
    assert np.array_equal(m.predict_proba(X), np.full((X.shape[0], K), 1.0 / K))
    # calibrate: K fits, fit k on column k against "label == class k"; a label that is no class counts among the rest
    lab = labels.copy()
    lab[5] = 77.0
    m.calibrate(X, lab)
    Ac, Bc = m.calibration
    st = m.calibration_stats
    for k in range(K):
        a, b, s1 = platt_fit(ctx, S[:, k].copy(), np.where(lab == m.classes_[k], 1.0, -1.0))
        assert (Ac[k], Bc[k]) == (a, b), (case, k)
        assert (st[k].reason, st[k].iterations, st[k].evaluations, st[k].n_pos, st[k].n_neg, st[k].fval) == (s1.reason, s1.iterations, s1.evaluations, s1.n_pos, s1.n_neg, s1.fval)
        assert st[k].reason == PC.CONVERGED and st[k].n_pos + st[k].n_neg == X.shape[0]
    PR = m.predict_proba(X)
    assert (np.abs(PR - _normalised(S, Ac, Bc)) <= 64.0 * EPS).all() and (np.abs(PR.sum(axis=1) - 1.0) <= 4.0 * EPS).all()
    m.destroy()
    ctx.close()


# ---- 8. multiclass state and errors -----------------------------------------------------------------------------------------------------------------------------
def test_multiclass_state_and_errors():
    ctx = pa.Context(0)
    case = (3, 37, None)
    X, labels, W, b = PC.multi_case(*case)
    m = pa.SVMMulticlass(ctx, options=OPT).create(X, labels)
    _raises(PMH_ERR_STATE, m.calibrate, X, labels)  # no model
    _raises(PMH_ERR_STATE, m.predict_proba, X)
    m.set_model(W, b)
    _raises(PMH_ERR_STATE, m.predict_proba, X)
    _raises(PMH_ERR_STATE, lambda: m.calibration)
    m.set_calibration(-np.ones(3), np.zeros(3))
    m.predict_proba(X)
    m.set_model(W, b)  # a new model: the calibration is gone
    _raises(PMH_ERR_STATE, m.predict_proba, X)
    _raises(PMH_ERR_STATE, lambda: m.calibration)
    for bad in ((-np.ones(2), np.zeros(3)), (-np.ones(3), np.zeros(4))):
        with pytest.raises(ValueError):
            m.set_calibration(*bad)
    m.destroy()
    ctx.close()
