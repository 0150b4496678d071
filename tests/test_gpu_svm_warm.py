"""Warm-started SVM training (pmh_svm_warm_start_vector, pmh_svm_train_warm, pmh_smalxe_set_initial_multiplier; SVM.train(warm_start=True)) and the grid search
over C on top of it (permon_amd.svm.grid_search).  The start vector is pinned bit for bit against numpy's restatement (svm_warm_cases.start_vector_np); a warm
training is compared as a SOLUTION -- the solver's own stopping quantity recomputed on the host, and the distance to a training 1000 times tighter against the
distance a cold training keeps to it; grid_search in cold mode is the hand-written loop, in warm mode it may differ from it only on samples whose score the
two models' difference can turn."""
import ctypes as ct

import numpy as np
import pytest

import permon_amd as pa
from permon_amd import _lib
from permon_amd import problems as P
from permon_amd._lib import PermonHipError, check
from permon_amd.core import Vec
from permon_amd.svm import grid_search, kfold, scores, select_C
from svm_train_cases import gamma
import svm_warm_cases as WC

pytestmark = pytest.mark.gpu
PMH_ERR_ARG, PMH_ERR_STATE = 2, 3
RTOL, ATOL = 1e-6, 1e-50
MAX_VEC = 2048 * 256  # PMH_MAX_VEC_BLOCKS * PMH_BLOCK: beyond it the grid-stride loops of the n-vector kernels wrap
# e_warm <= K max(e_cold, 1e-12 |tight|) in test_warm_equals_cold / test_warm_across_folds.  Measured e_warm / e_cold over their 18 cases: 0.035 ... 2.159, the
# largest at 301 x 37, L1, no bias (2.151 from fold to fold without bias); K is that times 4, rounded up to a power of two.  A ratio beyond 64 would not be
# covered by a larger K: the warm path would then be converging somewhere else
K = 16.0
SCALES = (0.5, 1.0, 3.7)


def opts(bias, rtol=RTOL, more=""):
    """(-qps_max_it is SMALXE's outer limit with a bias, MPGP's own without one: left at its default there)"""
    return "-qps_rtol %g%s %s" % (rtol, " -qps_max_it 100" if bias else "", more)


def _raises(code, f, *a, **kw):
    with pytest.raises(PermonHipError) as e:
        f(*a, **kw)
    assert e.value.code == code, str(e.value)
    return str(e.value)


# ---- 1. the start vector, bit for bit ---------------------------------------------------------------------------------------------------------------------------
def _noisy(n, d, seed):
    """Labels that no plane separates (a fifth of them flipped): some duals end at their bound."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    y = np.sign(X @ rng.standard_normal(d) + 1e-3)
    y[rng.random(n) < 0.2] *= -1.0
    return rng, X, y


def _check_vector(svm, a, scale, m, ub):
    v = svm.warm_start_vector(scale)
    ref, masked, clipped = WC.start_vector_np(a, scale, m, ub)
    assert np.array_equal(v, ref)
    assert svm.warm_start_counts == dict(masked=masked, clipped=clipped)
    return masked, clipped


@pytest.mark.parametrize("variant", ["L1", "L1w", "L2"])
@pytest.mark.parametrize("n", [1, 63, 257])
def test_start_vector_bits(n, variant):
    rng, X, y = _noisy(n, 5, 100 + n)
    loss = "L2" if variant == "L2" else "L1"
    cpos, cneg, wt = (1.5, 0.5, rng.uniform(0.5, 2.0, n)) if variant == "L1w" else (1.0, 1.0, None)
    Ci = np.where(y > 0, cpos, cneg) * (wt if wt is not None else 1.0)
    ub = Ci if loss == "L1" else None
    ctx = pa.Context(0)
    svm = pa.SVM(ctx, loss=loss, C=1.0, bias=n > 1, options=opts(n > 1), C_pos=cpos, C_neg=cneg).create(X, y, wt).train()
    a = svm.alpha
    assert (a > 0).any()
    mask = np.arange(n) % 3 != 1
    for m in [None] + ([mask] if n > 1 else []):
        svm.set_subset(m)
        for scale in SCALES:
            _check_vector(svm, a, scale, m, ub)
        assert np.array_equal(svm.alpha, a)  # set_subset keeps the dual
    if n > 1:
        # smaller penalties after the training clip, the new subset masks: both counts at once
        svm.set_subset(None).set_penalties(cpos / 4, cneg / 4, wt).set_subset(mask)
        assert np.array_equal(svm.alpha, a)  # set_penalties keeps it too
        masked, clipped = _check_vector(svm, a, 1.0, mask, ub / 4 if ub is not None else None)
        print(n, variant, "masked", masked, "clipped", clipped)
        assert masked > 0 and (clipped > 0 if loss == "L1" else clipped == 0)
    ctx.close()


def test_start_vector_beyond_one_grid():
    """n = 524 289 > PMH_MAX_VEC_BLOCKS * PMH_BLOCK: the grid-stride loop takes a second turn.  The dual is whatever three MPGP iterations leave (what is pinned
    is the kernel); the bound afterwards is the median of its positive entries, so that scaling by 3.7 clips about half of them."""
    n = MAX_VEC + 1
    rng, X, y = _noisy(n, 2, 7)
    ctx = pa.Context(0)
    svm = pa.SVM(ctx, loss="L1", C=1.0, bias=False, options="-qps_rtol 1e-6 -qps_max_it 3").create(X, y).train()
    a = svm.alpha
    assert (a[:MAX_VEC] > 0).any()
    c = float(np.median(a[a > 0]))
    mask = np.arange(n) % 3 != 1
    assert mask[MAX_VEC]
    svm.set_penalties(c, c).set_subset(mask)
    for scale in SCALES:
        masked, clipped = _check_vector(svm, a, scale, mask, np.full(n, c))
    print("n", n, "masked", masked, "clipped", clipped, "alpha beyond the first turn of the grid", a[MAX_VEC:])
    assert masked > 0 and clipped > 0
    ctx.close()


# ---- 2. state and arguments --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [False, True])
def test_warm_state_and_arguments(bias):
    _, X, y = _noisy(63, 5, 3)
    ctx = pa.Context(0)
    svm = pa.SVM(ctx, loss="L1", C=1.0, bias=bias, options=opts(bias)).create(X, y)
    for f in (lambda: svm.train(warm_start=True), svm.warm_start_vector):
        msg = _raises(PMH_ERR_STATE, f)
        assert "no dual" in msg and "pmh_svm_train first" in msg
    svm.train()
    a = svm.alpha
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        for f in (lambda s: svm.train(warm_start=True, alpha_scale=s), svm.warm_start_vector):
            msg = _raises(PMH_ERR_ARG, f, bad)
            assert "alpha_scale" in msg and "positive and finite" in msg
    assert np.array_equal(svm.alpha, a)  # a refusal changes nothing
    assert svm.w.shape == (5,)  # (still trained)
    # allowed after set_penalties and after set_subset, each of which leaves the handle untrained
    svm.set_penalties(2.0, 2.0).train(warm_start=True, alpha_scale=2.0)
    assert svm.stats.reason > 0
    m = np.arange(63) % 4 != 0
    svm.set_subset(m).train(warm_start=True)
    assert svm.stats.reason > 0 and (svm.alpha[~m] == 0.0).all()
    # new labels drop the dual
    y2 = y.copy()
    y2[::5] *= -1.0
    svm.set_labels(y2)
    msg = _raises(PMH_ERR_STATE, svm.train, warm_start=True)
    assert "pmh_svm_train_warm" in msg and "pmh_svm_set_labels drops the dual" in msg
    _raises(PMH_ERR_STATE, svm.warm_start_vector)
    svm.train().train(warm_start=True)
    assert svm.stats.reason > 0
    ctx.close()


# ---- 3. warm equals cold, as a solution --------------------------------------------------------------------------------------------------------------------------
_SHAPES = {}


def shape_data(kind):
    """-> (X as the handle takes it, X as fp64 on the host, y, sample_dtype)"""
    if kind not in _SHAPES:
        if kind == "csr":
            p = P.svm_sparse(300, 200, 12, 1.2, 0.5, 1.0)
            _SHAPES[kind] = (p["X"], p["X"].toarray(), p["y"], None)
        else:
            p = P.svm_offset(301, 37 if kind == "dense37" else 64, 2.0)
            if kind == "dense64_f32":
                X32 = p["X"].astype(np.float32)
                _SHAPES[kind] = (X32, X32.astype(np.float64), p["y"], np.float32)
            else:
                _SHAPES[kind] = (p["X"], p["X"], p["y"], None)
    return _SHAPES[kind]


def _model(svm):
    return svm.alpha, svm.w, svm.b


def _same(r1, r2):
    return np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1]) and r1[2] == r2[2]


def check_against_tight(tag, warm, cold, tight):
    """e = |(w, b) - (w, b)_tight|: the warm model is as near the tight one as the cold one is, up to K.  (w and b in one vector: a scalar's distance alone is
    small by chance too often to divide by.)"""
    v = lambda r: np.append(r[1], r[2])
    e_cold, e_warm = np.linalg.norm(v(cold) - v(tight)), np.linalg.norm(v(warm) - v(tight))
    floor = 1e-12 * np.linalg.norm(v(tight))
    print(tag, "e_cold %.3e e_warm %.3e ratio %.3f" % (e_cold, e_warm, e_warm / max(e_cold, floor)))
    assert e_warm <= K * max(e_cold, floor)


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("loss", ["L1", "L2"])
@pytest.mark.parametrize("kind", ["dense64", "dense37", "dense64_f32", "csr"])
def test_warm_equals_cold(kind, loss, bias):
    Xh, X, y, dt = shape_data(kind)
    n = y.size
    C0, C1 = 0.25, 1.0
    ctx = pa.Context(0)
    new = lambda rtol=RTOL: pa.SVM(ctx, loss=loss, C=C0, bias=bias, options=opts(bias, rtol), sample_dtype=dt).create(Xh, y)
    svm = new().train()
    st0 = svm.stats
    svm.set_penalties(C1, C1).train(warm_start=True, alpha_scale=C1 / C0)
    st, warm = svm.stats, _model(svm)
    assert st0.reason > 0 and st.reason > 0
    if not bias:
        # MPGP's own criterion at the returned alpha: |gP| <= max(rtol |rhs|, atol), the host's product in another order of summation
        pg = WC.projected_gradient_norm(WC.dual_hessian(X, y, None if loss == "L1" else np.full(n, 1.0 / C1)), np.ones(n), warm[0], np.full(n, C1) if loss == "L1" else None)
        thr = max(RTOL * np.sqrt(n), ATOL)
        print(kind, loss, "|gP| %.3e threshold %.3e" % (pg, thr))
        assert pg <= thr * (1 + 1e-6)
    fresh = new().set_penalties(C1, C1)
    cold = _model(fresh.train())
    stc = fresh.stats
    tsvm = new(RTOL * 1e-3).set_penalties(C1, C1).train()
    assert stc.reason > 0 and tsvm.stats.reason > 0
    print(kind, loss, "bias" if bias else "no bias", "nmv cold from C0: %d, warm: %d, cold: %d, tight: %d" % (st0.nmv, st.nmv, stc.nmv, tsvm.stats.nmv))
    check_against_tight("%s %s bias=%d" % (kind, loss, bias), warm, cold, _model(tsvm))
    # the cold path is untouched: after the warm training, train() gives the fresh handle's bits
    assert _same(_model(svm.train()), cold)
    ctx.close()


# ---- 4. SMALXE from a given multiplier ---------------------------------------------------------------------------------------------------------------------------
def test_smalxe_initial_multiplier():
    Xh, X, y, dt = shape_data("dense37")
    n = y.size
    ctx = pa.Context(0)
    L = ctx.L
    svm = pa.SVM(ctx, loss="L1", C=1.0, bias=True, options=opts(True)).create(Xh, y).train()
    a_train = svm.alpha
    sx = svm.solver_handles()[3]
    u, Btmu = ct.c_void_p(), ct.c_void_p()
    check(L.pmh_smalxe_get_solution(sx, None, ct.byref(u), None))
    check(L.pmh_smalxe_get_penalized(sx, None, None, ct.byref(Btmu)))
    u, Btmu = Vec.borrowed(ctx, u, n), Vec.borrowed(ctx, Btmu, n)

    def solve(zero_u):
        if zero_u:
            u.set(0.0)
        check(L.pmh_smalxe_reset(sx))
        check(L.pmh_smalxe_solve(sx))
        st = _lib.SmalxeStats()
        check(L.pmh_smalxe_get_stats(sx, ct.byref(st)))
        return st.reason, st.iteration, st.inner_iter_accu, u.to_numpy(), Btmu.to_numpy()

    cold = solve(True)
    assert cold[0] > 0 and np.array_equal(cold[3], a_train)
    mu = Vec.from_numpy(ctx, cold[4])  # a copy of the converged solve's B'mu; u stays at the solution
    check(L.pmh_smalxe_set_initial_multiplier(sx, mu.p))
    warm = solve(False)
    print("outer / inner iterations cold", cold[1:3], "from the converged multiplier and solution", warm[1:3])
    assert warm[0] > 0 and warm[1] <= cold[1]
    # one-shot: the next solve starts from zero again
    again = solve(True)
    assert again[:3] == cold[:3] and np.array_equal(again[3], cold[3]) and np.array_equal(again[4], cold[4])
    # NULL is no call, and takes a multiplier given before back
    check(L.pmh_smalxe_set_initial_multiplier(sx, mu.p))
    check(L.pmh_smalxe_set_initial_multiplier(sx, None))
    null = solve(True)
    assert null[:3] == cold[:3] and np.array_equal(null[3], cold[3]) and np.array_equal(null[4], cold[4])
    mu.free()
    ctx.close()


# ---- 5. across folds ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [False, True])
def test_warm_across_folds(bias):
    Xh, X, y, dt = shape_data("dense37")
    m0, m1, _ = kfold(y, 3, seed=0)
    ctx = pa.Context(0)
    svm = pa.SVM(ctx, loss="L1", C=1.0, bias=bias, options=opts(bias)).create(X, y)
    svm.set_subset(m0).train()
    a0 = svm.alpha
    svm.set_subset(m1).train(warm_start=True)
    warm = _model(svm)
    assert svm.stats.reason > 0 and (a0[~m1] != 0.0).any() and (warm[0][~m1] == 0.0).all()
    assert svm.warm_start_counts["masked"] == int((a0[~m1] != 0.0).sum())
    fit = lambda rtol: pa.SVM(ctx, loss="L1", C=1.0, bias=bias, options=opts(bias, rtol)).fit(X[m1], y[m1])
    cold, tight = fit(RTOL), fit(RTOL * 1e-3)
    assert cold.stats.reason > 0 and tight.stats.reason > 0
    print("bias" if bias else "no bias", "nmv warm from the other fold %d, cold %d" % (svm.stats.nmv, cold.stats.nmv))
    check_against_tight("folds bias=%d" % bias, warm, _model(cold), _model(tight))
    ctx.close()


# ---- 6. - 8. grid_search -----------------------------------------------------------------------------------------------------------------------------------------
CONFIGS = [("dense", False, False), ("dense", True, True), ("csr", True, False)]  # (instance, bias, C_pos != C_neg and sample weights)
CPOS, CNEG = 1.5, 0.75
_RUNS = {}


def _weights(n):
    return np.random.default_rng(11).uniform(0.5, 2.0, n)


def _new(ctx, kind, bias, weighted):
    X, y = WC.grid_data(kind)
    wt = _weights(y.size) if weighted else None
    kw = dict(C_pos=CPOS, C_neg=CNEG) if weighted else {}
    return pa.SVM(ctx, loss="L1", C=1.0, bias=bias, options=opts(bias), **kw).create(X, y, wt), wt


def grid_run(kind, bias, weighted, warm):
    """grid_search over GRID_CS (handed over unsorted) with k = 3, refit and the models, run once per configuration: (result, the handle's state afterwards)."""
    key = (kind, bias, weighted, warm)
    if key not in _RUNS:
        ctx = pa.Context(0)
        svm, wt = _new(ctx, kind, bias, weighted)
        out = grid_search(svm, [WC.GRID_CS[2], WC.GRID_CS[0], WC.GRID_CS[1]], k=WC.GRID_K, warm_start=warm, sample_weight=wt, refit=True, return_models=True)
        _RUNS[key] = (out, dict(subset=svm.subset, penalties=svm.penalties, model=_model(svm)))
        ctx.close()
    return _RUNS[key]


@pytest.mark.parametrize("kind,bias,weighted", CONFIGS)
def test_grid_search_cold_is_the_hand_written_loop(kind, bias, weighted):
    out, after = grid_run(kind, bias, weighted, False)
    X, y = WC.grid_data(kind)
    rp, rn = (CPOS, CNEG) if weighted else (1.0, 1.0)
    ctx = pa.Context(0)
    svm, wt = _new(ctx, kind, bias, weighted)
    hand = WC.hand_grid(svm, y, WC.GRID_CS, WC.GRID_K, rp, rn, wt)
    assert out["Cs"] == WC.GRID_CS and len(out["masks"]) == WC.GRID_K
    for g in range(len(WC.GRID_CS)):
        for f in range(WC.GRID_K):
            for key in ("TP", "FP", "TN", "FN"):
                assert out["counts"][g][f][key] == hand[g][f][key], (g, f, key)
            assert sum(out["counts"][g][f][key] for key in ("TP", "FP", "TN", "FN")) == int((~out["masks"][f]).sum())
            assert out["nmv"][g][f] > 0 and out["passes_X"][g][f] > 0
    sc = [scores(row)["accuracy"] for row in hand]
    print(kind, bias, weighted, "accuracy over C", sc, "best", out["best_C"])
    assert out["score"] == sc
    assert out["best_index"] == int(np.flatnonzero(np.array(sc) == max(sc))[0]) and out["best_C"] == WC.GRID_CS[out["best_index"]]
    assert (out["best_C"], out["best_index"]) == select_C(out["Cs"], out["score"])
    # refit: all samples again (the subset it had), best_C's penalties, trained -- the model of that training written by hand
    Cb = out["best_C"]
    assert after["subset"] is None
    assert np.array_equal(after["penalties"], np.where(y > 0, Cb * rp, Cb * rn) * (wt if weighted else 1.0))
    assert _same(after["model"], _model(svm.set_subset(None).set_penalties(Cb * rp, Cb * rn, wt).train()))
    ctx.close()


def test_grid_search_leaves_the_handle_as_asked():
    """refit=False on a handle with a subset: the subset comes back, the penalties are those the handle was constructed with, it is untrained; another score;
    the refusals."""
    X, y = WC.grid_data("dense")
    n = y.size
    ctx = pa.Context(0)
    svm, wt = _new(ctx, "dense", False, True)
    m = np.arange(n) % 7 != 2
    svm.set_subset(m)
    out = grid_search(svm, [0.5, 2.0], k=2, score="f1", warm_start=True, sample_weight=wt, refit=False)
    assert np.array_equal(svm.subset, m)
    assert np.array_equal(svm.penalties, np.where(y > 0, CPOS, CNEG) * wt)
    _raises(PMH_ERR_STATE, lambda: svm.w)
    assert "W" not in out and out["score"] == [scores(row)["f1"] for row in out["counts"]]
    for bad in ([], [1.0, 0.0], [-1.0], [float("inf")], [float("nan")]):
        with pytest.raises(ValueError):
            grid_search(svm, bad)
    with pytest.raises(ValueError):
        grid_search(svm, [1.0], score="auc")
    assert np.array_equal(svm.subset, m)
    ctx.close()


@pytest.mark.parametrize("kind,bias,weighted", CONFIGS)
def test_grid_search_warm_against_cold(kind, bias, weighted):
    """Cell by cell: |s_warm(x) - s_cold(x)| <= |W_warm - W_cold| |x| + |b_warm - b_cold|, so a held-out sample can change its label only where its cold score
    is no larger than that (plus the rounding of the two dot products formed here: gamma_{d+2} (|x| . |w| + |b|) each); the counts of a cell differ by at most
    the number of such samples."""
    cold, _ = grid_run(kind, bias, weighted, False)
    warm, _ = grid_run(kind, bias, weighted, True)
    X, y = WC.grid_data(kind)
    X = X.toarray() if hasattr(X, "toarray") else X
    d = X.shape[1]
    changed = 0
    for g in range(len(WC.GRID_CS)):
        for f, m in enumerate(cold["masks"]):
            assert np.array_equal(m, warm["masks"][f])
            Xo = X[~m]
            Wc, bc, Ww, bw = cold["W"][g][f], cold["b"][g][f], warm["W"][g][f], warm["b"][g][f]
            sc, sw = Xo @ Wc + bc, Xo @ Ww + bw
            bound = np.linalg.norm(Ww - Wc) * np.linalg.norm(Xo, axis=1) + abs(bw - bc)
            bound = bound + gamma(d + 2) * (np.abs(Xo) @ (np.abs(Wc) + np.abs(Ww)) + abs(bc) + abs(bw))
            differ = (sc >= 0) != (sw >= 0)
            assert (np.abs(sc[differ]) <= bound[differ]).all()
            may = int((np.abs(sc) <= bound).sum())
            for key in ("TP", "FP", "TN", "FN"):
                assert abs(warm["counts"][g][f][key] - cold["counts"][g][f][key]) <= may, (g, f, key)
            changed += int(differ.sum())
            if g == 0:  # the first C of a fold is cold in either mode
                assert np.array_equal(Wc, Ww) and bc == bw and cold["nmv"][g][f] == warm["nmv"][g][f]
    print(kind, bias, weighted, "labels that differ over the grid:", changed, "nmv cold", np.sum(cold["nmv"]), "warm", np.sum(warm["nmv"]), "scores", cold["score"], warm["score"])


def test_warm_grid_takes_no_more_products():
    """L1, no bias, the dense 240 x 8 grid: on these nine QPs the oracle's MPGP needs 3060 products from zero and 1534 from the warm starts (a factor 1.99; the
    notebook, "SVM warm starts"), so the condition has a margin of that size."""
    cold, _ = grid_run("dense", False, False, False)
    warm, _ = grid_run("dense", False, False, True)
    print("nmv cold", cold["nmv"], "warm", warm["nmv"])
    assert np.sum(warm["nmv"]) <= np.sum(cold["nmv"])
