"""Sample subsets on SVMMulticlass (pmh_svm_multi_set_subset), K-class scoring of the handle's own rows (pmh_svm_multi_predict_own, pmh_svm_multi_test_own) and
cross_validate on top.  The held-out set of every test is H(n) = {0} u [64, 192) u {i : i % 7 == 3} u {n - 1}, clipped to the range: the first row, two
whole 64-row workgroups, isolated rows, one row of a half-wave pair, the last row (% 7 and not the binary tests' % 5: with labels i mod 5 that would hold out
a whole class, which is the refusal of test_state_and_refusals).  Nothing here has a tolerance: training is compared with K binary handles under the same
subset (pinned against the oracle in test_gpu_svm_subset.py), own-row scoring with decision_function / predict on an uploaded copy (pinned against numpy in
test_gpu_svm_multiclass.py), bit for bit."""
import ctypes as ct

import numpy as np
import pytest

import permon_amd as pa
import svm_multiclass_cases as MC
from permon_amd import problems as P
from permon_amd._lib import PermonHipError
from permon_amd.svm import cross_validate, kfold

pytestmark = pytest.mark.gpu
PMH_ERR_ARG, PMH_ERR_STATE = 2, 3
OPT = "-qps_rtol 1e-6"
COUNTERS = ("reason", "outer_iterations", "inner_iterations", "nmv", "ncg", "nexp", "nprop", "passes_X", "n_sv", "n_free_sv")
KC = {p: pa.SVMMulticlass.chunk(p) for p in ("dense64", "dense", "csr")}
WHICH = ("held_out", "subset", "all")


def _counters(st):
    return tuple(getattr(st, k) for k in COUNTERS)


def held_out(n):
    h = np.zeros(n, dtype=bool)
    h[0] = h[n - 1] = True
    h[64:192] = True
    h[3::7] = True
    return h


def _blobs(n, d, K, sparse=None):
    """problems.svm_blobs with seed 5 (labels i mod K), the class values 10 k - 7."""
    p = P.svm_blobs(n, d, K, 4.0, 5, sparse=sparse)
    return (p["X_csr"] if sparse else p["X"]), 10.0 * p["labels"] - 7.0


# ---- 1. training equals K binary handles under the same subset ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,balanced", [(c, bal) for c in [(300, 64, 3, None, "L1"), (250, 20, 5, None, "L1"), (400, 2000, 4, 10, "L1")] for bal in (False, True)]
                         + [((250, 20, 5, None, "L2"), True)])
def test_subset_training_equals_binary_handles(case, balanced):
    n, d, K, sparse, loss = case
    ctx = pa.Context(0)
    X, lab = _blobs(n, d, K, sparse)
    mask = ~held_out(n)
    m = pa.SVMMulticlass(ctx, loss, 1.0, True, OPT, balanced=balanced).create(X, lab)
    assert m.subset is None and np.array_equal(m.subset_class_counts, [int((lab == c).sum()) for c in m.classes_])
    m.set_subset(mask).train()
    cls = m.classes_
    assert np.array_equal(cls, 10.0 * np.arange(K) - 7.0) and np.array_equal(m.subset, mask)
    counts = np.array([int((lab[mask] == c).sum()) for c in cls], dtype=np.int64)
    assert m.subset_class_counts.dtype == np.int64 and np.array_equal(m.subset_class_counts, counts)
    W, b, st = m.W, m.b, m.stats
    nS = int(mask.sum())
    for k in range(K):
        y = np.where(lab == cls[k], 1.0, -1.0)
        nk = int(counts[k])
        cp, cn = (1.0 * nS / (2 * nk), 1.0 * nS / (2 * (nS - nk))) if balanced else (1.0, 1.0)
        assert m.class_penalties(k) == (cp, cn)
        s = pa.SVM(ctx, loss, 1.0, True, OPT, C_pos=cp if balanced else None, C_neg=cn if balanced else None).create(X, y).set_subset(mask).train()
        assert np.array_equal(W[k], s.w) and b[k] == s.b, (case, k)
        assert _counters(st[k]) == _counters(s.stats), (case, k)
        s.destroy()
    m.destroy()
    ctx.close()


# ---- 2. held-out rows are not used in training ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 37])
def test_held_out_rows_are_not_used_in_training(d):
    """As test_gpu_svm_subset.py's test_held_out_rows_are_not_used: NaN goes into the held-out rows of the handle's device copy of X after create (whose solver
    multiplies by the whole X); set_subset builds the solver anew over S, and the K trainings give the bits of the clean handle."""
    n, K = 300, 3
    X, lab = _blobs(n, d, K)
    mask = ~held_out(n)
    Xn = X.copy()
    Xn[~mask] = np.nan
    ctx = pa.Context(0)
    res = []
    for Xk in (X, Xn):
        m = pa.SVMMulticlass(ctx, "L1", 1.0, True, OPT).create(X, lab)
        m._keep[0].set_numpy(Xk.ravel())
        m.set_subset(mask).train()
        res.append((m.W, m.b, [_counters(s) for s in m.stats]))
        m.destroy()
    (W1, b1, s1), (W2, b2, s2) = res
    assert np.isfinite(W2).all() and np.isfinite(b2).all() and np.abs(W1).max() > 0
    assert np.array_equal(W1, W2) and np.array_equal(b1, b2) and s1 == s2
    ctx.close()


# ---- 3. own-row scoring without training --------------------------------------------------------------------------------------------------------------------------
def _np_confusion(cls, lab, pred, sel):
    conf = np.zeros((cls.size, cls.size), dtype=np.int64)
    np.add.at(conf, (np.searchsorted(cls, lab[sel]), np.searchsorted(cls, pred[sel])), 1)
    return conf


def _check_own(m, X, lab, mask, what):
    """m: created on (X, lab) with the subset mask and a model set.  Scores and labels of the own rows equal those of an uploaded copy; the three confusion
    matrices equal numpy's count over the device's own labels."""
    n = lab.size
    S, pred = m.decision_function(X), m.predict(X)
    assert np.array_equal(m.decision_function_own(), S) and np.array_equal(m.predict_own(), pred), what
    cls = m.classes_
    t = {}
    for which, sel in zip(WHICH, (~mask, mask, np.ones(n, dtype=bool))):
        t[which] = m.test_own(which)
        conf = _np_confusion(cls, lab, pred, sel)
        assert np.array_equal(t[which]["confusion"], conf), (what, which)
        assert t[which]["n"] == int(sel.sum()) == int(conf.sum()), (what, which)
        assert t[which]["accuracy"] == np.trace(conf) / int(sel.sum()), (what, which)
        again = m.test_own(which)
        assert np.array_equal(again["confusion"], conf) and again["n"] == t[which]["n"], (what, which)
    assert np.array_equal(t["held_out"]["confusion"] + t["subset"]["confusion"], t["all"]["confusion"]), what


def _model_handle(ctx, X, K, mask):
    """A handle on X with the labels i mod K and the subset mask that never trains: the model is MC.model's."""
    n, d = X.shape
    lab = (np.arange(n) % K).astype(np.float64)
    assert np.unique(lab[mask]).size == K
    m = pa.SVMMulticlass(ctx, options=OPT).create(X, lab).set_subset(mask)
    with pytest.raises(PermonHipError) as e:
        m.decision_function_own()
    assert e.value.code == PMH_ERR_STATE
    m.set_model(*MC.model(d, K))
    assert np.array_equal(m.subset, mask)  # (set_model keeps the subset)
    return m, lab


@pytest.mark.parametrize("d,K", [(d, K) for d in MC.DENSE_D for K in MC.chunk_Ks(KC["dense64" if d == 64 else "dense"])])
def test_dense_own_row_scoring(d, K):
    ctx = pa.Context(0)
    for n in (K + 1, 67, 1025):
        if n == K + 1:  # hold out the last row only: its label is the one that occurs twice
            mask = np.arange(n) != n - 1
        else:
            mask = ~held_out(n)
        X = MC.dense_samples(n, d)
        m, lab = _model_handle(ctx, X, K, mask)
        _check_own(m, X, lab, mask, "dense d=%d n=%d K=%d" % (d, n, K))
        m.destroy()
    ctx.close()


@pytest.mark.parametrize("K", MC.chunk_Ks(KC["csr"]))
def test_csr_own_row_scoring(K):
    ctx = pa.Context(0)
    X = MC.csr_samples("many")
    n = X.shape[0]
    mask = ~held_out(n)
    assert (np.diff(X.indptr)[~mask] == 0).any()  # a sample without entries is held out
    m, lab = _model_handle(ctx, X, K, mask)
    _check_own(m, X, lab, mask, "csr K=%d" % K)
    m.destroy()
    ctx.close()


# ---- 4. unselected rows are not loaded and not read ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,n", [(64, 1025), (65, 67)])
def test_unselected_rows_are_not_read(d, n):
    """K = 5: two chunks, so the best workspace is in play.  With NaN in the rows of the device copy of X that a selection leaves out, test_own over the
    selection is what it is on the clean X -- an unselected row would poison the counts through its label, which the confusion kernel must not read either."""
    K = 5
    ctx = pa.Context(0)
    X = MC.dense_samples(n, d)
    mask = ~held_out(n)
    m, lab = _model_handle(ctx, X, K, mask)
    clean = {w: m.test_own(w) for w in WHICH}
    for which, sel in (("held_out", ~mask), ("subset", mask)):
        Xn = X.copy()
        Xn[~sel] = np.nan
        m._keep[0].set_numpy(Xn.ravel())
        t = m.test_own(which)
        assert np.array_equal(t["confusion"], clean[which]["confusion"]) and t["n"] == clean[which]["n"] == int(sel.sum()), which
        S = m.decision_function_own()
        assert np.array_equal(np.isfinite(S).all(axis=1), sel) and np.array_equal(np.isnan(S).all(axis=1), ~sel), which
    m.destroy()
    ctx.close()


# ---- 5. state and refusals ---------------------------------------------------------------------------------------------------------------------------------------
def _state_error(f, *a):
    with pytest.raises(PermonHipError) as e:
        f(*a)
    assert e.value.code == PMH_ERR_STATE, str(e.value)


def test_state_and_refusals():
    n, d, K = 250, 20, 5
    ctx = pa.Context(0)
    X, lab = _blobs(n, d, K)
    mask = ~held_out(n)
    m = pa.SVMMulticlass(ctx, "L1", 1.0, True, OPT).fit(X, lab)
    W0, b0 = m.W, m.b
    # without a subset
    _state_error(m.test_own, "held_out")
    t = m.test(X, lab)
    for which in ("subset", "all"):
        o = m.test_own(which)
        assert np.array_equal(o["confusion"], t["confusion"]) and o["accuracy"] == t["accuracy"] and o["n"] == n
    with pytest.raises(ValueError):
        m.test_own("everything")
    conf = np.zeros((K, K), dtype=np.int64)
    assert m.L.pmh_svm_multi_test_own(m.h, 3, conf.ctypes.data_as(ct.c_void_p), None) == PMH_ERR_ARG
    # a new subset clears the model, the statistics and the calibration
    m.set_calibration(np.full(K, -2.0), np.full(K, 0.1))
    assert m.predict_proba(X[:7]).shape == (7, K)
    m.set_subset(mask)
    for f in (lambda: m.W, lambda: m.b, lambda: m.stats, m.decision_function_own, m.predict_own, lambda: m.test_own("held_out"), lambda: m.predict(X[:7])):
        _state_error(f)
    m.set_model(W0, b0)
    _state_error(m.predict_proba, X[:7])
    _state_error(lambda: m.stats)
    assert np.array_equal(m.subset, mask)
    # all samples again: the bits of a handle that never had a subset
    m.set_subset(None).train()
    assert m.subset is None and np.array_equal(m.W, W0) and np.array_equal(m.b, b0)
    # refusals leave everything as it was
    m.set_subset(mask).train()
    W1, b1 = m.W, m.b
    assert not np.array_equal(W1, W0)
    i = np.arange(n)
    no_class_3 = i % 5 != 3
    bad_masks = [("class", no_class_3.astype(float)), ("0.5", np.where(i == 5, 0.5, mask)), ("nan", np.where(i == 5, np.nan, mask)), ("empty", np.zeros(n))]
    for name, bad in bad_masks:
        with pytest.raises(PermonHipError) as e:
            m.set_subset(bad)
        assert e.value.code == PMH_ERR_ARG, name
        if name == "class":
            assert "class 23" in str(e.value), str(e.value)  # the class value 10 * 3 - 7
        assert np.array_equal(m.subset, mask) and np.array_equal(m.W, W1) and np.array_equal(m.b, b1), name
        m.train()
        assert np.array_equal(m.W, W1) and np.array_equal(m.b, b1), name
    m.destroy()
    ctx.close()


# ---- 6. cross_validate ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(300, 64, 3, None), (400, 2000, 4, 10)])
def test_cross_validate(case):
    n, d, K, sparse = case
    ctx = pa.Context(0)
    X, lab = _blobs(n, d, K, sparse)
    m = pa.SVMMulticlass(ctx, "L1", 1.0, True, OPT).create(X, lab)
    cv = cross_validate(m, k=5, seed=0)
    assert set(cv) == {"folds", "accuracy", "confusion", "masks"} and len(cv["folds"]) == 5 and m.subset is None
    _state_error(lambda: m.W)  # left untrained
    masks = kfold(lab, 5, seed=0)
    for mk, mc, f in zip(masks, cv["masks"], cv["folds"]):
        assert np.array_equal(mk, mc)
        t = m.set_subset(mk).train().test_own("held_out")
        assert np.array_equal(t["confusion"], f["confusion"]) and t["n"] == f["n"] == int((~mk).sum()) and t["accuracy"] == f["accuracy"]
    assert np.array_equal(cv["confusion"], sum(f["confusion"] for f in cv["folds"])) and cv["confusion"].sum() == n
    assert cv["accuracy"] == float(np.mean([f["accuracy"] for f in cv["folds"]]))
    print(case, "5-fold accuracy", cv["accuracy"])
    # the subset the handle had comes back
    mask = ~held_out(n)
    m.set_subset(mask)
    cv2 = cross_validate(m, k=5, seed=0)
    assert np.array_equal(m.subset, mask) and np.array_equal(cv2["confusion"], cv["confusion"])
    m.destroy()
    ctx.close()


def test_cross_validate_binary_keys_and_a_one_sample_class():
    n, d, K = 250, 20, 5
    ctx = pa.Context(0)
    X, lab = _blobs(n, d, K)
    s = pa.SVM(ctx, "L1", 1.0, True, OPT).create(X, np.where(lab == lab[0], 1.0, -1.0))
    assert set(cross_validate(s, k=5, seed=0)) == {"folds", "accuracy", "masks"}
    s.destroy()
    # a class of one sample: the fold that holds it out cannot train
    lone = lab.copy()
    lone[18] = 99.0
    m = pa.SVMMulticlass(ctx, "L1", 1.0, True, OPT).create(X, lone)
    assert m.K == K + 1
    mask = ~held_out(n)
    assert mask[18]
    for before in (None, mask):
        m.set_subset(before)
        with pytest.raises(PermonHipError) as e:
            cross_validate(m, k=5, seed=0)
        assert e.value.code == PMH_ERR_ARG and "class 99" in str(e.value)
        assert m.subset is None if before is None else np.array_equal(m.subset, before)
    m.destroy()
    ctx.close()
