"""GPU tests of the multiclass SVM: pmh_svm_set_labels against a fresh handle bit for bit (dense d = 64, dense d != 64, CSR), one-vs-rest training against K
binary fits, the K-column scoring kernels of csrc/svm_multi.hip against numpy without any training (pmh_svm_multi_set_model), the confusion matrix, the errors."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import permon_amd as pa
import svm_multiclass_cases as MC
from permon_amd import problems as P
from permon_amd._lib import PermonHipError

pytestmark = pytest.mark.gpu
PMH_ERR_ARG, PMH_ERR_STATE = 2, 3
OPT = "-qps_rtol 1e-6"
COUNTERS = ("reason", "outer_iterations", "inner_iterations", "nmv", "ncg", "nexp", "nprop", "passes_X", "n_sv", "n_free_sv")
KC = {p: pa.SVMMulticlass.chunk(p) for p in ("dense64", "dense", "csr")}


def _counters(st):
    return tuple(getattr(st, k) for k in COUNTERS)


def _two_labellings(shape):
    """X with two labellings y1, y2 of different planes."""
    if shape == "csr":
        p = P.svm_sparse(400, 3000, 12, 1.0, 0.5)
        keep = np.ones(400)
        keep[123] = 0.0  # one sample without entries
        X = (sp.diags(keep) @ p["X"]).tocsr()
        X.eliminate_zeros()
        X.sort_indices()
        assert X.indptr[124] == X.indptr[123]
        d = 3000
    else:
        p = P.svm_offset(*shape)
        X, d = p["X"], shape[1]
    w2 = np.random.default_rng(99).standard_normal(d)
    y2 = np.sign(np.asarray(X @ w2).ravel() + 0.3)
    y2[y2 == 0] = 1.0
    assert (y2 != p["y"]).any()
    return X, p["y"], y2


# ---- 1. set_labels equals a fresh handle ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [0, 1])
@pytest.mark.parametrize("loss", ["L1", "L2"])
@pytest.mark.parametrize("shape", [(300, 64), (257, 37), (130, 130), "csr"])
def test_set_labels_equals_a_fresh_handle(shape, loss, bias):
    ctx = pa.Context(0)
    X, y1, y2 = _two_labellings(shape)
    n = y1.size
    fresh = pa.SVM(ctx, loss, 1.0, bias, OPT).fit(X, y2)
    ref = (fresh.alpha, fresh.w, fresh.b, _counters(fresh.stats))
    for in_place in (False, True):
        yv = ctx.vec_from(y1)
        s = pa.SVM(ctx, loss, 1.0, bias, OPT).fit(X, yv)
        assert not np.array_equal(s.w, ref[1])
        # penalties set before are gone after set_labels: C everywhere
        s.set_penalties(2.0, 0.5, np.linspace(0.5, 1.5, n))
        assert not np.array_equal(s.penalties, np.full(n, 1.0))
        if in_place:
            yv.set_numpy(y2)  # the buffer the handle borrows, overwritten
            s.set_labels(yv)
        else:
            s.set_labels(y2)
        assert np.array_equal(s.penalties, np.full(n, 1.0))
        with pytest.raises(PermonHipError) as e:
            s.w
        assert e.value.code == PMH_ERR_STATE
        s.train()
        assert np.array_equal(s.alpha, ref[0]), (shape, loss, bias, in_place)
        assert np.array_equal(s.w, ref[1]) and s.b == ref[2]
        assert _counters(s.stats) == ref[3]
        s.destroy()
    fresh.destroy()
    ctx.close()


# ---- 2. one-vs-rest equals K binary fits ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,balanced", [(c, bal) for c in [(300, 64, 3, None, "L1"), (250, 20, 5, None, "L1"), (400, 2000, 4, 10, "L1")] for bal in (False, True)]
                         + [((250, 20, 5, None, "L2"), True)])  # L2, balanced: set_labels takes the diagonal off, set_penalties puts the next class's on
def test_one_vs_rest_equals_binary_fits(case, balanced):
    n, d, K, sparse, loss = case
    ctx = pa.Context(0)
    p = P.svm_blobs(n, d, K, 4.0, 5, sparse=sparse)
    X = p["X_csr"] if sparse else p["X"]
    lab = 10.0 * p["labels"] - 7.0  # class values that are not their indices
    m = pa.SVMMulticlass(ctx, loss, 1.0, True, OPT, balanced=balanced).fit(X, lab)
    cls = m.classes_
    assert np.array_equal(cls, 10.0 * np.arange(K) - 7.0)
    W, b, st = m.W, m.b, m.stats
    assert W.shape == (K, d) and b.shape == (K,) and len(st) == K
    for k in range(K):
        y = np.where(lab == cls[k], 1.0, -1.0)
        nk = int((y > 0).sum())
        cp, cn = (1.0 * n / (2 * nk), 1.0 * n / (2 * (n - nk))) if balanced else (1.0, 1.0)
        assert m.class_penalties(k) == (cp, cn)
        s = pa.SVM(ctx, loss, 1.0, True, OPT, C_pos=cp if balanced else None, C_neg=cn if balanced else None).fit(X, y)
        assert np.array_equal(W[k], s.w) and b[k] == s.b, (case, k)
        assert _counters(st[k]) == _counters(s.stats)
        if sparse:  # both CSR scoring paths are one segmented sum (svm_csr_seg.h): equal models, equal products, one order of addition, b last -> equal bits
            assert np.array_equal(m.decision_function(X)[:, k], s.decision_function(X)), (case, k)
        s.destroy()
    m.destroy()
    ctx.close()


# ---- 3. the scoring kernels against numpy, no training ----------------------------------------------------------------------------------------------------------
def _model_handle(ctx, d, K, sparse):
    """A handle with K classes (values 3 k + 0.5) and d features that never trains: created on K samples, then given the model."""
    rng = np.random.default_rng(5)
    if sparse:
        X0 = sp.csr_matrix((rng.standard_normal(K), np.arange(K, dtype=np.int32), np.arange(K + 1, dtype=np.int32)), shape=(K, d))
    else:
        X0 = rng.standard_normal((K, d))
    classes = 3.0 * np.arange(K) + 0.5
    m = pa.SVMMulticlass(ctx, options=OPT).create(X0, classes[::-1].copy())
    assert np.array_equal(m.classes_, classes)
    W, b = MC.model(d, K)
    return m.set_model(W, b), W, b, classes


def _check_scoring(m, X, W, b, classes, what):
    S_np, bound, open_rows = MC.reference(X, W, b)
    n = X.shape[0]
    S, lab = m.predict_both(X)
    err = np.abs(S - S_np)
    print("scoring", what, ": max err / bound %.3f, rows left open %d of %d" % ((err / bound).max(), int(open_rows.sum()), n))
    assert (err <= bound).all(), what
    # the label is the first maximum of the device's own scores
    assert np.array_equal(lab, classes[np.argmax(S, axis=1)]), what
    # and numpy's arg-max wherever the bound decides it
    assert open_rows.sum() <= 0.01 * n
    assert np.array_equal(lab[~open_rows], classes[np.argmax(S_np, axis=1)][~open_rows]), what
    # scores alone, labels alone, and again: the same bits
    assert np.array_equal(m.decision_function(X), S) and np.array_equal(m.predict(X), lab), what
    S2, lab2 = m.predict_both(X)
    assert np.array_equal(S2, S) and np.array_equal(lab2, lab), what


@pytest.mark.parametrize("d,K", [(d, K) for d in MC.DENSE_D for K in MC.chunk_Ks(KC["dense64" if d == 64 else "dense"])])
def test_dense_scoring_against_numpy(d, K):
    ctx = pa.Context(0)
    m, W, b, classes = _model_handle(ctx, d, K, False)
    for n in MC.DENSE_N:
        _check_scoring(m, MC.dense_samples(n, d), W, b, classes, "dense d=%d n=%d K=%d" % (d, n, K))
    m.destroy()
    ctx.close()


@pytest.mark.parametrize("K", MC.chunk_Ks(KC["csr"]))
def test_csr_scoring_against_numpy(K):
    ctx = pa.Context(0)
    m, W, b, classes = _model_handle(ctx, MC.CSR_D, K, True)
    for which in ("many", "one"):
        X = MC.csr_samples(which)
        _check_scoring(m, X, W, b, classes, "csr %s K=%d" % (which, K))
        if which == "many":  # a sample without entries scores b
            empty = np.diff(X.indptr) == 0
            assert empty.any() and np.array_equal(m.decision_function(X)[empty], np.tile(b, (int(empty.sum()), 1)))
    m.destroy()
    ctx.close()


def test_ties_go_to_the_lowest_class():
    """Equal rows of W give equal scores bit for bit, wherever in their chunks the classes sit: the label is the lowest of them."""
    ctx = pa.Context(0)
    for d, sparse in ((64, False), (37, False), (MC.CSR_D, True)):
        K = 2 * max(KC.values()) + 3
        m, W, b, classes = _model_handle(ctx, d, K, sparse)
        W[:], b[:] = W[1], b[1]  # all classes alike ...
        W[0], b[0] = -W[1], -10.0 - abs(b[1])
        m.set_model(W, b)
        X = MC.csr_samples("many") if sparse else MC.dense_samples(67, d)
        S, lab = m.predict_both(X)
        assert (S[:, 1:] == S[:, 1:2]).all()
        top = np.where(S[:, 0] > S[:, 1], 0, 1)  # ... but class 0
        assert np.array_equal(lab, classes[top]) and (top == 1).any()
        m.destroy()
    ctx.close()


# ---- 4. test ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [None, 10])
def test_confusion_matrix(sparse):
    ctx = pa.Context(0)
    n, d, K = (400, 2000, 4) if sparse else (300, 64, 3)
    p = P.svm_blobs(n, d, K, 4.0, 5, N_test=203, sparse=sparse)
    m = pa.SVMMulticlass(ctx, "L1", 1.0, True, OPT).fit(p["X_csr"] if sparse else p["X"], p["labels"])
    Xt, lt = (p["X_test_csr"] if sparse else p["X_test"]), p["labels_test"].copy()
    lt[[3, 77, 150]] = [99.0, -1.0, 0.5]  # no classes
    t = m.test(Xt, lt)
    lab = m.predict(Xt)
    cls = m.classes_
    conf = np.zeros((K, K), dtype=np.int64)
    known = np.isin(lt, cls)
    for a, c in zip(lt[known], lab[known]):
        conf[int(np.searchsorted(cls, a)), int(np.searchsorted(cls, c))] += 1
    assert np.array_equal(t["confusion"], conf)
    assert t["n_unknown"] == 3 and t["confusion"].sum() + t["n_unknown"] == 203
    assert t["accuracy"] == np.trace(conf) / 203
    assert t["accuracy"] > 0.8  # separated blobs
    m.destroy()
    ctx.close()


# ---- 5. errors ----------------------------------------------------------------------------------------------------------------------------------------------------
def _raises(code, text, f, *a):
    with pytest.raises(PermonHipError) as e:
        f(*a)
    assert e.value.code == code and text in str(e.value), str(e.value)


def test_errors():
    ctx = pa.Context(0)
    rng = np.random.default_rng(0)
    X = rng.standard_normal((12, 5))
    lab = np.arange(12.0) % 3
    _raises(PMH_ERR_ARG, "at least two", pa.SVMMulticlass(ctx).create, X, np.ones(12))
    bad = lab.copy()
    bad[4] = np.nan
    _raises(PMH_ERR_ARG, "not finite", pa.SVMMulticlass(ctx).create, X, bad)
    m = pa.SVMMulticlass(ctx, options=OPT).create(X, lab)
    _raises(PMH_ERR_STATE, "pmh_svm_multi_train", m.predict, X)
    _raises(PMH_ERR_STATE, "pmh_svm_multi_train", m.test, X, lab)
    with pytest.raises(PermonHipError) as e:
        m.W
    assert e.value.code == PMH_ERR_STATE
    m.destroy()
    # a model of 300 features (trained on CSR samples) takes no dense test samples; CSR test samples need its width
    Xs = sp.random(30, 300, density=0.05, format="csr", random_state=1)
    m = pa.SVMMulticlass(ctx, options=OPT).fit(Xs, np.arange(30.0) % 3)
    _raises(PMH_ERR_ARG, "dense test samples need d <= 256, the model has d = 300: hand them over in CSR (pmh_svm_multi_predict_csr)", m.predict, np.zeros((30, 300)))
    _raises(PMH_ERR_ARG, "the test samples have 299 features, the model has 300", m.predict, sp.random(5, 299, density=0.1, format="csr", random_state=2))
    m.destroy()
    ctx.close()


def test_communicator_is_refused():
    os.environ["PMH_COMM_FORCE"] = "1"
    try:
        ctx = pa.Context(0)
        ctx.comm_init(0, 1, ctx.comm_unique_id())
        X = np.random.default_rng(0).standard_normal((12, 5))
        _raises(PMH_ERR_ARG, "communicator", pa.SVMMulticlass(ctx).create, X, np.arange(12.0) % 3)
        ctx.close()
    finally:
        del os.environ["PMH_COMM_FORCE"]
