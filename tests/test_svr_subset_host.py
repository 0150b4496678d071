"""Host tests (no GPU) of what SVR subsets and cross-validation rest on: numpy's restatement of the operator under a subset (tests/svr_subset_cases.py) against
the Hessian of the subset's samples, kfold without strata on continuous targets, the pooled metrics, the loop of cross_validate on a stand-in handle, and the
ValueErrors SVR raises before it calls the library."""
import numpy as np
import pytest

import permon_amd.svm as svm_mod
from permon_amd.svr import SVR
import svr_cases as S
import svr_subset_cases as SC


@pytest.mark.parametrize("kind", list(S.OP_TERMS))
def test_masked_hessian_is_the_subsets_hessian_embedded(kind):
    """M^ H^(X) M^ + sigma e^ e^' has the Hessian of X[m] (with the sigma term over S: e_S = [1; -1] of length 2 n_S) in the rows and columns of S and zeros
    elsewhere; apply_sub is its product, exactly on integer data."""
    n, d = 301, 7
    X, u, diag = S.int_case(n, d, 5)
    m = SC.train_mask(n)
    shift, use_diag, sigma = S.OP_TERMS[kind]
    D = S.D_of(n, shift, diag if use_diag else None)
    Hs = SC.hessian_sub(X, D, sigma, m)
    mm = SC.doubled(m)
    assert np.array_equal(Hs[np.ix_(mm, mm)], S.hessian(X[m], D[m], sigma))
    assert not Hs[~mm].any() and not Hs[:, ~mm].any()
    assert np.array_equal(SC.apply_sub(X, u, D, sigma, m), Hs @ u)
    # the sigma term alone: sigma (e^'u) e^ with the sum over S
    e = np.concatenate([m, -1.0 * m])
    assert np.array_equal(SC.apply_sub(X, u, D, sigma, m) - SC.apply_sub(X, u, D, 0.0, m), sigma * (e @ u) * e)
    # held-out entries of the operand are selected away
    assert np.array_equal(SC.apply_sub(X, SC.poison(u, m), D, sigma, m), SC.apply_sub(X, u, D, sigma, m))


def test_train_mask_reaches_the_edges():
    """Row groups of 8 (double) and 16 (float) rows: the block 61 .. 194 holds groups that are wholly held out, and is cut inside a group at both ends."""
    m = SC.train_mask(2003)
    for g in (8, 16):
        whole = [k for k in range(2003 // g) if not m[g * k:g * k + g].any()]
        assert whole, g
        assert m[(61 // g) * g:61].any() and not m[61:(61 // g + 1) * g].any()
        assert not m[(194 // g) * g:195].any() and m[195:(194 // g + 1) * g].any()
    assert not m[0] and not m[-1] and not m[3::5].any()
    assert SC.train_mask(1).all() and list(SC.train_mask(3)) == [True, False, True]


@pytest.mark.parametrize("n,k", [(600, 3), (601, 5), (7, 7)])
def test_kfold_without_strata_on_continuous_targets(n, k):
    t = np.random.default_rng(n).standard_normal(n)
    masks = svm_mod.kfold(t, k, seed=4, stratified=False)
    assert len(masks) == k and all(mk.dtype == bool and mk.shape == (n,) for mk in masks)
    held = np.array([~mk for mk in masks])
    assert (held.sum(axis=0) == 1).all()  # the complements partition the rows
    sizes = held.sum(axis=1)
    assert sizes.max() - sizes.min() <= 1
    again = svm_mod.kfold(t, k, seed=4, stratified=False)
    assert all(np.array_equal(a, b) for a, b in zip(masks, again))
    # the targets play no part: any other targets give the same masks
    other = svm_mod.kfold(np.zeros(n), k, seed=4, stratified=False)
    assert all(np.array_equal(a, b) for a, b in zip(masks, other))


def _fold_sums(f, t):
    r = f - t
    return dict(n=int(t.size), sum_r=float(r.sum()), sum_r2=float(r @ r), sum_abs_r=float(np.abs(r).sum()), max_abs=float(np.abs(r).max()), sum_t=float(t.sum()),
                sum_t2=float(t @ t), n_in_tube=0, mse=float(r @ r) / t.size, mae=float(np.abs(r).sum()) / t.size, r2=0.0)


def test_pooled_metrics():
    r = np.random.default_rng(1)
    parts = [(r.standard_normal(k), 3.0 + r.standard_normal(k)) for k in (200, 201, 199)]
    folds = [_fold_sums(f, t) for f, t in parts]
    got = svm_mod.pooled_metrics(folds)
    assert got == SC.pooled(folds)
    f, t = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    res = f - t
    assert got["n"] == 600 and got["max_abs"] == np.abs(res).max()
    assert abs(got["mse"] - np.mean(res ** 2)) <= 1e-13 * np.mean(res ** 2)
    assert abs(got["mae"] - np.mean(np.abs(res))) <= 1e-13 * np.mean(np.abs(res))
    r2 = 1.0 - (res @ res) / ((t - t.mean()) @ (t - t.mean()))
    assert abs(got["r2"] - r2) <= 1e-11
    # the pooled r2 is not the mean of the folds' (each fold has its own mean target)
    empty = svm_mod.pooled_metrics([])
    assert empty["n"] == 0 and np.isnan(empty["mse"]) and np.isnan(empty["r2"])
    const = svm_mod.pooled_metrics([_fold_sums(np.ones(4), np.full(4, 2.0))])
    assert np.isnan(const["r2"]) and const["mse"] == 1.0


class _Stub:
    """A library that must not be reached: every entry raises."""

    def __getattr__(self, name):
        raise AssertionError("the library was called: " + name)


def _bare(n):
    s = SVR.__new__(SVR)
    s.ctx, s.L, s.h, s.n, s.d, s._keep = None, _Stub(), object(), n, 3, None
    return s


def test_value_errors_come_before_the_call():
    s = _bare(5)
    with pytest.raises(ValueError, match="must have 5 entries"):
        s.set_subset(np.ones(4))
    with pytest.raises(ValueError, match="must have 5 entries"):
        s.set_subset(np.ones((5, 2), dtype=bool))
    for bad in (np.array(["a"] * 5), np.ones(5, dtype=complex), np.array([None] * 5, dtype=object)):
        with pytest.raises(ValueError, match="booleans or 0 / 1 numbers"):
            s.set_subset(bad)
    with pytest.raises(ValueError, match="which must be one of"):
        s.test_own("training")
    s.h = None
    for call in (lambda: s.set_subset(np.ones(5)), lambda: s.subset, lambda: s.predict_own(), lambda: s.test_own("all")):
        with pytest.raises(RuntimeError, match="call fit first"):
            call()


class _FakeSVR:
    """What cross_validate uses of an SVR handle, on the host: test_own returns sums that identify the mask."""

    _who = "SVR"

    def __init__(self, t, subset=None):
        self._keep = (None, type("V", (), {"to_numpy": lambda self_: t})())
        self.t, self.subset, self.trained, self.log = t, subset, False, []

    def _need(self):
        pass

    def set_subset(self, m):
        self.subset, self.trained = (None if m is None else np.array(m)), False
        self.log.append("set")
        return self

    def train(self):
        self.trained = True
        self.log.append("train")
        return self

    def test_own(self, which):
        assert which == "held_out" and self.trained
        t = self.t[~self.subset]
        return _fold_sums(np.zeros(t.size), t)


def test_cross_validate_loops_an_svr_handle_without_strata():
    t = np.random.default_rng(2).standard_normal(60) + 1.0
    before = np.arange(60) % 2 == 0
    h = _FakeSVR(t, before)
    for stratified in (True, False):  # does not apply to an SVR handle
        out = svm_mod.cross_validate(h, k=3, seed=9, stratified=stratified)
        want = svm_mod.kfold(t, 3, 9, stratified=False)
        assert all(np.array_equal(a, b) for a, b in zip(out["masks"], want))
        assert len(out["folds"]) == 3 and sum(f["n"] for f in out["folds"]) == 60
        pooled = SC.pooled(out["folds"])
        assert {key: out[key] for key in pooled} == pooled and "accuracy" not in out
        assert np.array_equal(h.subset, before) and not h.trained
    assert h.log[:7] == ["set", "train", "set", "train", "set", "train", "set"]
