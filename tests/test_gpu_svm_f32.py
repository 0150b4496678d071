"""Dense SVM samples stored in float32 (pmh_op_create_svm_dual_f32, pmh_svm_create_f32, pmh_svm_*_f32; SVM(sample_dtype=numpy.float32)).

Inputs are problems.svm_dual / svm_offset with their seeds, rounded once: X32 = X.astype(float32), Xw = X32.astype(float64); every reference is computed on Xw,
so the rounding of the samples is no part of any error here.  Widening is exact and all arithmetic is fp64, hence:
  * any d but 64 (one wavefront per row, the fp64 kernels with another load): bit for bit what the fp64 handle gives on Xw -- array_equal throughout;
  * d = 64 (a layout of its own: four rows per wave-instruction, 16-byte loads): another summation order, so the bounds are those the fp64 tests use where two
    orders meet -- Higham's gamma for any order of summation (test_gpu_svm_subset.py::test_subset_operator_against_numpy), the trajectory criteria of
    test_gpu_svm.py and the training criteria of test_gpu_svm_train.py::test_biased_training_other_widths, none widened.
The held-out set is train_mask's of test_gpu_svm_subset.py: {0} u [64, 192) u {i : i % 5 == 3} u {n - 1}."""
import ctypes as ct

import numpy as np
import pytest

import permon_amd as pa
from permon_amd import _lib
from permon_amd import problems as P
from permon_amd._lib import PermonHipError, check
from permon_amd.core import VecF32
from permon_amd.svm import cross_validate, platt_fit
from svm_proba_cases import sigma as np_sigma
from svm_train_cases import ASTOL, EPS, check_counts, gamma, np_model

pytestmark = pytest.mark.gpu
PMH_ERR_ARG = 2
F32 = np.float32
OPTS = "-qps_rtol 1e-6 -qps_max_it 100"
FORMS = [("plain", 0.0, False, 0.0), ("shift", 1.0 / 0.7, False, 0.0), ("diag", 0.0, True, 0.0), ("shift+sigma", 1.0 / 0.7, False, 2.5), ("diag+sigma", 0.0, True, 2.5)]
STAT_FIELDS = [f for f, _ in _lib.SvmStats._fields_]


def train_mask(n):
    """test_gpu_svm_subset.py's mask; n = 1: that mask holds no sample (row 0 is both the first and the last), which set_subset refuses, so the one sample stays in."""
    h = np.zeros(n, dtype=bool)
    h[0] = h[n - 1] = True
    h[64:192] = True
    h[3::5] = True
    return ~h if (~h).any() else np.ones(n, dtype=bool)


_DATA = {}


def rounded(kind, *args, **kw):
    """The problem with X (and X_test) rounded once: p["X32"] float32, p["X"] its widening, drawn once per argument list."""
    key = (kind, args, tuple(sorted(kw.items())))
    if key not in _DATA:
        p = dict(getattr(P, kind)(*args, **kw))
        p["X32"] = p["X"].astype(F32)
        p["X"] = p["X32"].astype(np.float64)
        if "X_test" in p:
            p["X_test32"] = p["X_test"].astype(F32)
            p["X_test"] = p["X_test32"].astype(np.float64)
        _DATA[key] = p
    return _DATA[key]


def _stats(st):
    return np.array([getattr(st, f) for f in STAT_FIELDS], dtype=np.float64)


def _result(svm):
    return svm.alpha, svm.w, svm.b, _stats(svm.stats)


def _same(r1, r2):
    """alpha, w, b and every statistic, bit for bit (b_free is NaN where no support vector is free: equal NaNs are equal)."""
    return all(np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True) for a, b in zip(r1, r2))


def _raises(code, f, *a, **kw):
    with pytest.raises(PermonHipError) as e:
        f(*a, **kw)
    assert e.value.code == code, str(e.value)
    return str(e.value)


def _set_form(H, shift, dg, sigma):
    H.set_diag(None), H.set_terms(shift, sigma), H.set_diag(dg)


# ---- 1. any d but 64: the fp64 kernels' bits ---------------------------------------------------------------------------------------------------------------------
GENERIC = [(301, 1), (301, 37), (301, 130), (301, 256), (3, 37)]  # (3 rows: fewer than the four waves of one workgroup)


@pytest.mark.parametrize("n,d", GENERIC)
def test_generic_operator_equals_the_fp64_operator_on_the_widened_samples(n, d):
    p = rounded("svm_dual", n, d)
    y = p["y"]
    rng = np.random.default_rng(1)
    v, dg = rng.standard_normal(n), rng.uniform(0.5, 2.0, n)
    ctx = pa.Context(0)
    H32 = pa.MatCreateSVMDual(ctx, p["X32"], y, sample_dtype=F32)
    H64 = pa.MatCreateSVMDual(ctx, p["X"], y)
    assert H32.sample_dtype is F32 and H64.sample_dtype is np.float64 and H32._keep[0].n == n * d and H32._keep[0].to_numpy().dtype == F32
    vd = ctx.vec_from(v)
    for m in (None, train_mask(n)):
        H32.set_subset(m), H64.set_subset(m)
        for name, shift, diag, sg in FORMS:
            for H in (H32, H64):
                _set_form(H, shift, dg if diag else None, sg)
            o32, o64 = ctx.vec(n), ctx.vec(n)
            H32.mult(vd, o32), H64.mult(vd, o64)
            a, b = o32.to_numpy(), o64.to_numpy()
            assert np.isfinite(a).all() and np.abs(a).max() > 0 and np.array_equal(a, b), (name, m is not None)
    ctx.close()


@pytest.mark.parametrize("n,d", GENERIC)
def test_generic_training_and_scores_equal_the_fp64_handle(n, d):
    p = rounded("svm_offset", n, d, 2.0, N_test=97)
    y, Cc, Xt32, Xt, yt = p["y"], p["C"], p["X_test32"], p["X_test"], p["y_test"]
    ctx = pa.Context(0)
    for loss in ("L1", "L2"):
        for bias in (True, False):
            s32 = pa.SVM(ctx, loss=loss, C=Cc, bias=bias, options=OPTS, sample_dtype=F32).fit(p["X32"], y)
            s64 = pa.SVM(ctx, loss=loss, C=Cc, bias=bias, options=OPTS).fit(p["X"], y)
            assert s32.sample_dtype is F32 and s64.sample_dtype is np.float64
            r32, r64 = _result(s32), _result(s64)
            print(n, d, loss, bias, "reason", s32.stats.reason, "inner", s32.stats.inner_iterations)
            assert np.isfinite(r32[0]).all() and np.isfinite(r32[1]).all() and _same(r32, r64)
            # float32 test samples through the _f32 entries against the widened ones through the fp64 entries
            assert np.array_equal(s32.decision_function(Xt32), s64.decision_function(Xt)) and np.array_equal(s32.predict(Xt32), s64.predict(Xt))
            assert s32.test(Xt32, yt) == s64.test(Xt, yt)
            assert np.array_equal(s32.decision_function_own(), s64.decision_function_own()) and s32.test_own("all") == s64.test_own("all")
            s32.calibrate(Xt32, yt), s64.calibrate(Xt, yt)
            assert s32.calibration == s64.calibration
            assert np.array_equal(s32.predict_proba(Xt32), s64.predict_proba(Xt))
            # a float32 handle takes float64 arrays too: they are rounded on the way up, here back to Xt32
            assert np.array_equal(s32.decision_function(Xt), s32.decision_function(Xt32))
            s32.destroy(), s64.destroy()
    ctx.close()


# ---- 2. d = 64: the operator against numpy -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [777, 13, 1])  # 777: no multiple of the 16 rows a wave has in flight; 13, 1: fewer rows than one group
def test_d64_operator_against_numpy(n):
    """out = m o ((H + D)(m o v)) with the sigma term over S in the five forms, on all samples and under the subset, within
    2 (gamma_{n+d+2} |X| (|X|' |m o v|) + sigma gamma_{n+2} sum |m o v| + 4 eps |ref|) elementwise: Higham's bound holds for any order of summation, so the float32
    layout's order needs no margin of its own.  Held-out rows exactly 0; NaN / 1e300 in held-out entries of v without effect; two calls give equal bits."""
    d = 64
    p = rounded("svm_dual", n, d)
    X, y = p["X"], p["y"]
    Xa = np.abs(X)
    rng = np.random.default_rng(1)
    v, dg = rng.standard_normal(n), rng.uniform(0.5, 2.0, n)
    ctx = pa.Context(0)
    H = pa.MatCreateSVMDual(ctx, p["X32"], y, sample_dtype=F32)
    for m in (np.ones(n, dtype=bool), train_mask(n)):
        sub = not m.all()
        H.set_subset(m if sub else None)
        mf = m.astype(float)
        v2 = v.copy()
        v2[~m] = np.where(np.arange((~m).sum()) % 2 == 0, np.nan, 1e300)
        vd, v2d = ctx.vec_from(v), ctx.vec_from(v2)
        mv = mf * v
        Hv = y * (X @ (X.T @ (y * mv)))
        for name, shift, diag, sg in FORMS:
            _set_form(H, shift, dg if diag else None, sg)
            D = dg if diag else shift
            ref = mf * (Hv + D * mv + sg * y * (y @ mv))
            bound = 2 * (gamma(n + d + 2) * (Xa @ (Xa.T @ np.abs(mv))) + sg * gamma(n + 2) * np.abs(mv).sum() + 4 * EPS * np.abs(ref))
            out, out2, out3 = ctx.vec(n), ctx.vec(n), ctx.vec(n)
            H.mult(vd, out), H.mult(v2d, out2), H.mult(vd, out3)
            o = out.to_numpy()
            err = np.abs(o - ref)
            print(n, "subset" if sub else "all", name, "max err / bound", (err[m] / bound[m]).max())
            assert np.isfinite(o).all() and np.abs(o).max() > 0 and (err <= bound).all()
            assert (o[~m] == 0.0).all()
            assert np.array_equal(o, out2.to_numpy()) and np.array_equal(o, out3.to_numpy())
    ctx.close()


# ---- 3. held-out rows of X are not loaded --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["L1", "L2"])
@pytest.mark.parametrize("n,d,offset", [(777, 64, 3.0), (301, 37, 2.0)])
def test_held_out_rows_are_not_loaded(n, d, offset, loss):
    """test_gpu_svm_subset.py::test_held_out_rows_are_not_used on the float32 copy: NaN rows written into the handle's device samples after create; set_subset and
    train then give the bits of the clean handle, all finite."""
    p = rounded("svm_offset", n, d, offset)
    X32, y = p["X32"], p["y"]
    m = train_mask(n)
    Xn = X32.copy()
    Xn[~m] = np.nan
    ctx = pa.Context(0)
    res = []
    for Xk in (X32, Xn):
        svm = pa.SVM(ctx, loss=loss, C=p["C"], bias=True, options=OPTS, sample_dtype=F32).create(X32, y)
        assert isinstance(svm._keep[0], VecF32)
        svm._keep[0].set_numpy(Xk.ravel())
        svm.set_subset(m).train()
        res.append(_result(svm))
        svm.destroy()
    r1, r2 = res
    print(n, d, loss, "reason", r1[3][0], "outer/inner", r1[3][1], r1[3][2])
    assert r1[3][0] == 2
    assert np.isfinite(r2[0]).all() and np.isfinite(r2[1]).all() and np.isfinite(r2[2]) and np.isfinite(r2[3]).all()
    assert (r1[0][~m] == 0.0).all() and np.abs(r1[0]).max() > 0 and _same(r1, r2)
    ctx.close()


# ---- 4. the paired kernels -----------------------------------------------------------------------------------------------------------------------------------------
def _mpgp(ctx, p, shift=0.0, sigma=0.0, dg=None, mask=None, X32=None, rtol=1e-6, max_it=None, fixed=None):
    """MPGP on the float32 operator in the given form: (H, stats, x, passes over X of the run)."""
    n = p["n"]
    H = pa.MatCreateSVMDual(ctx, p["X32"] if X32 is None else X32, p["y"], sample_dtype=F32)
    if mask is not None:
        H.set_subset(mask)
    H.set_terms(shift, sigma), H.set_diag(dg)
    qp = pa.QP(ctx)
    qp.SetOperator(H)
    qp.SetRhs(ctx.vec_from(p["b"] if mask is None else mask.astype(float)))
    x = ctx.vec_from(p["x0"])
    qp.SetInitialVector(x)
    qp.SetBox(None, ctx.vec_from(p["lb"]), ctx.vec_from(p["ub"]))
    qps = pa.QPS(ctx)
    qps.SetQP(qp)
    qps.SetType("mpgp")
    qps.SetTolerances(rtol=rtol, max_it=max_it)
    qps.SetUp()
    p0 = H.passes()
    st = qps.RunFixed(fixed) if fixed else qps.Solve()
    assert x.n == n
    return H, st, x.to_numpy(), H.passes() - p0


def _both(ctx, f):
    """f() with the paired passes and with the separate ones."""
    rp = f()
    check(ctx.L.pmh_set_knob(b"svm_pairing", 0))
    try:
        rs = f()
    finally:
        check(ctx.L.pmh_set_knob(b"svm_pairing", 1))
    return rp, rs


def test_paired_kernels_first_iterations_equal_the_oracle(oracle):
    """test_gpu_svm.py::test_svm_mpgp_first_iterations_equal_the_oracle with the float32 operator on the device and numpy on the widened samples in the oracle:
    over 60 iterations the same steps, the same iterate (1e-10 relative) and the same three norms (1e-9), pairing on and off."""
    ctx = pa.Context(0)
    p = rounded("svm_dual", 4000, 64)
    X, y = p["X"], p["y"]
    op = oracle.Op(p["n"], fn=lambda a: y * (X @ (X.T @ (y * a))))
    ref = oracle.mpgp(op, p["b"], p["x0"], oracle.Box(p["n"], lb=p["lb"], ub=p["ub"]), rtol=1e-30, max_it=60)
    assert ref["nexp"] > 1  # (expansion steps, so the prepared forms are among the kernels that ran)
    runs = _both(ctx, lambda: _mpgp(ctx, p, rtol=1e-30, max_it=60))
    for (H, st, x, passes), paired in zip(runs, (True, False)):
        print("paired" if paired else "separate", "steps", (st.ncg, st.nexp, st.nprop, st.nmv), "passes", passes, "x rel", np.linalg.norm(x - ref["x"]) / np.linalg.norm(ref["x"]))
        assert (st.iteration, st.reason) == (ref["iteration"], ref["reason"]) and st.reason == -3
        assert (st.ncg, st.nexp, st.nprop, st.nmv) == (ref["ncg"], ref["nexp"], ref["nprop"], ref["nmv"])
        assert np.linalg.norm(x - ref["x"]) <= 1e-10 * np.linalg.norm(ref["x"])
        for k in ("rnorm", "gfnorm", "gcnorm"):
            assert abs(getattr(st, k) - ref[k]) <= 1e-9 * max(ref["rnorm"], 1e-300), (k, getattr(st, k), ref[k])
        assert (passes < 2 * st.nmv) if paired else (passes >= 2 * st.nmv)
    ctx.close()


def _paired_equals_separate(ctx, p, f, solve):
    """The criteria of test_svm_paired_passes_equal_separate_passes / test_augmented_paired_passes_equal_separate_passes; f: the objective."""
    X, y = p["X"], p["y"]
    (Hp, st_p, x_p, pass_p), (Hs, st_s, x_s, pass_s) = _both(ctx, solve)
    print("paired", (st_p.iteration, st_p.nmv, st_p.nexp, pass_p), "separate", (st_s.iteration, st_s.nmv, st_s.nexp, pass_s))
    assert st_p.reason == st_s.reason == 2
    assert abs(st_p.iteration - st_s.iteration) <= max(3, st_s.iteration // 6) and st_p.nexp > 0
    w_p, w_s = X.T @ (y * x_p), X.T @ (y * x_s)
    assert np.linalg.norm(w_p - w_s) <= 1e-3 * np.linalg.norm(w_s)
    assert abs(f(x_p) - f(x_s)) <= 1e-6 * abs(f(x_s))
    assert x_p.min() >= -ASTOL and x_p.max() <= 1.0 + ASTOL
    per_s, per_p = Hs.passes() / st_s.nmv, Hp.passes() / st_p.nmv
    assert 2.0 <= per_s <= 2.2
    assert per_p <= per_s - 0.9 * (st_p.nexp - 1) / st_p.nmv, (per_p, per_s, st_p.nexp, st_p.nmv)
    assert pass_p < 2 * st_p.nmv  # the fused instances ran
    _, st_q, x_q, _ = solve()
    assert st_q.iteration == st_p.iteration and np.array_equal(x_q, x_p)
    return x_p


@pytest.mark.parametrize("N", [4003, 777])
def test_paired_passes_equal_separate_passes(N):
    ctx = pa.Context(0)
    p = rounded("svm_dual", N, 64)
    X, y = p["X"], p["y"]
    _paired_equals_separate(ctx, p, lambda a: 0.5 * np.dot(X.T @ (y * a), X.T @ (y * a)) - a.sum(), lambda: _mpgp(ctx, p))
    ctx.close()


@pytest.mark.parametrize("form", ["shift", "diag", "subset"])
def test_augmented_and_subset_paired_passes_equal_separate_passes(form):
    """The scalar shift and the diagonal, each with the rank-one term (s = sum y_i v_i travels with the column sums), and the plain form under train_mask (rhs = m;
    test_gpu_svm_subset.py::test_paired_passes_under_a_subset: NaN held-out rows change no bit, the held-out entries stay 0, fewer than two passes per product)."""
    ctx = pa.Context(0)
    N = 777
    p = rounded("svm_dual", N, 64)
    X, y = p["X"], p["y"]
    sigma = 30.0
    if form == "subset":
        m = train_mask(N)
        mf = m.astype(float)
        f = lambda a: 0.5 * np.dot(X.T @ (y * mf * a), X.T @ (y * mf * a)) - mf @ a
        x_p = _paired_equals_separate(ctx, p, f, lambda: _mpgp(ctx, p, mask=m))
        Xn = p["X32"].copy()
        Xn[~m] = np.nan
        _, st_n, x_n, _ = _mpgp(ctx, p, mask=m, X32=Xn)
        assert np.isfinite(x_n).all() and np.array_equal(x_n, x_p) and (x_p[~m] == 0.0).all() and np.abs(x_p).max() > 0
    else:
        D = 0.5 if form == "shift" else np.random.default_rng(2).uniform(0.3, 0.7, N)
        f = lambda a: 0.5 * np.dot(X.T @ (y * a), X.T @ (y * a)) + 0.5 * a @ (D * a) + 0.5 * sigma * (y @ a) ** 2 - a.sum()
        solve = (lambda: _mpgp(ctx, p, shift=D, sigma=sigma)) if form == "shift" else (lambda: _mpgp(ctx, p, sigma=sigma, dg=D))
        _paired_equals_separate(ctx, p, f, solve)
    ctx.close()


# ---- 5. training at d = 64, judged from alpha alone ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["L1", "L2"])
def test_biased_training_d64(loss):
    """The body of test_gpu_svm_train.py::test_biased_training_other_widths on svm_offset(1500, 64, 3.0, N_test=500) rounded to float32: the solve converges; the
    equality and the KKT residual are within SMALXE's threshold plus the recomputation's rounding; w, b and the scores within their dot-product bounds of numpy's
    on the widened samples; labels and counts equal numpy's wherever the score decides beyond the bound (at most 1 % may be left out: a condition on the draw).
    Then against the fp64 handle on the widened samples by the criteria for two solves whose sums differ in order: the same reason, |w32 - w64| <= 1e-3 |w64|,
    objectives within 1e-6 relative."""
    ctx = pa.Context(0)
    d = 64
    p = rounded("svm_offset", 1500, d, 3.0, N_test=500)
    X, y, n, Cc = p["X"], p["y"], p["n"], p["C"]
    svm = pa.SVM(ctx, loss=loss, C=Cc, bias=True, options="-qps_rtol 1e-6", sample_dtype=F32).fit(p["X32"], y)
    a, st = svm.alpha, svm.stats
    sh = 0.0 if loss == "L1" else 1.0 / Cc
    thr = 1e-6 * np.sqrt(n)
    print(loss, "reason", st.reason, "outer/inner", st.outer_iterations, st.inner_iterations, "passes", st.passes_X, "nmv", st.nmv)
    assert st.reason == 2 and a.min() >= -ASTOL and (loss == "L2" or a.max() <= Cc + ASTOL)
    assert abs(y @ a) / np.sqrt(n) <= thr + 2 * gamma(n) * np.abs(a).sum() / np.sqrt(n)
    w_np, b_np, free = np_model(p, a, loss)
    assert free.sum() > 0 and st.n_free_sv == free.sum() and st.n_sv == (a > ASTOL).sum()
    Wc = np.abs(X).T @ np.abs(a)
    g = y * (X @ w_np) + sh * a - 1.0 + st.b_multiplier * y
    e = 2 * gamma(n + d + 2) * (np.abs(X) @ Wc) + 4 * EPS * (np.abs(g) + 1.0) + EPS * abs(st.b_multiplier)
    lo, hi = a <= ASTOL, (a >= Cc - ASTOL) if loss == "L1" else np.zeros(n, bool)
    gP = np.where(lo, np.minimum(g, 0.0), np.where(hi, np.maximum(g, 0.0), g))
    print(loss, "|gP|", np.linalg.norm(gP), "thr", thr, "+", np.linalg.norm(e))
    assert np.linalg.norm(gP) <= thr + np.linalg.norm(e)
    assert (np.abs(svm.w - w_np) <= 2 * gamma(n + 1) * Wc).all()
    db = 2 * gamma(d + 1) * float(np.mean(np.abs(X[free]) @ np.abs(w_np))) + 2 * gamma(n + 1) * float(np.mean(np.abs(X[free]) @ Wc)) + gamma(int(free.sum()) + 2) * (1 + abs(b_np))
    assert abs(svm.b - b_np) <= db
    Xt, yt = p["X_test"], p["y_test"]
    sc_np = Xt @ w_np + b_np
    sb = 2 * gamma(d + 2) * (np.abs(Xt) @ np.abs(w_np) + abs(b_np)) + np.abs(Xt) @ (2 * gamma(n + 1) * Wc) + db
    sc = svm.decision_function(p["X_test32"])
    print(loss, "max score err / bound", (np.abs(sc - sc_np) / sb).max(), "least |score|", np.abs(sc_np).min(), "greatest bound", sb.max())
    assert (np.abs(sc - sc_np) <= sb).all()
    sure = np.abs(sc_np) > sb
    assert (~sure).sum() <= 0.01 * sure.size
    assert np.array_equal(svm.predict(p["X_test32"])[sure], np.where(sc_np >= 0, 1.0, -1.0)[sure])
    check_counts(svm.test(p["X_test32"], yt), sc_np, yt, sure)
    s64 = pa.SVM(ctx, loss=loss, C=Cc, bias=True, options="-qps_rtol 1e-6").fit(X, y)
    a64 = s64.alpha
    f = lambda z: 0.5 * np.dot(X.T @ (y * z), X.T @ (y * z)) + 0.5 * sh * z @ z - z.sum()
    print(loss, "fp64 handle: w rel", np.linalg.norm(svm.w - s64.w) / np.linalg.norm(s64.w), "f rel", abs(f(a) - f(a64)) / abs(f(a64)))
    assert s64.stats.reason == st.reason
    assert np.linalg.norm(svm.w - s64.w) <= 1e-3 * np.linalg.norm(s64.w)
    assert abs(f(a) - f(a64)) <= 1e-6 * abs(f(a64))
    ctx.close()


# ---- 6. the handle's life cycle on float32 samples -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,offset", [(64, 3.0), (37, 2.0)])
def test_handle_life_cycle(d, offset):
    n = 600
    p = rounded("svm_offset", n, d, offset, N_test=200)
    X32, y, Cc, Xt32, yt = p["X32"], p["y"], p["C"], p["X_test32"], p["y_test"]
    y2 = rounded("svm_offset", n, d, offset, seed_w=9)["y"]  # the same X (seed_x), another plane
    assert (y2 != y).any()
    ctx = pa.Context(0)
    new = lambda loss="L1": pa.SVM(ctx, loss=loss, C=Cc, bias=True, options=OPTS, sample_dtype=F32)
    # two fits give equal bits
    svm = new().fit(X32, y)
    r1 = _result(svm)
    assert svm.stats.reason == 2 and _same(r1, _result(new().fit(X32, y)))
    # the handle's own rows are scored by the sweep that scores an upload of them
    own = svm.decision_function_own()
    assert np.array_equal(own, svm.decision_function(X32)) and svm.test_own("all") == svm.test(X32, y)
    # probabilities: calibrate is platt_fit of the float32 samples' scores; predict_proba applies the pair to them in the scores' order
    S = svm.decision_function(Xt32)
    svm.calibrate(Xt32, yt)
    A, B, _ = platt_fit(ctx, S, yt)
    assert svm.calibration == (A, B)
    pr = svm.predict_proba(Xt32)
    assert (np.abs(pr - np_sigma(A * S + B)) <= 32.0 * EPS).all() and np.array_equal(svm.predict_proba(Xt32), pr)
    o = np.argsort(S, kind="stable")
    assert (np.diff(pr[o]) >= 0.0).all() if A <= 0 else (np.diff(pr[o]) <= 0.0).all()
    # cross-validation on the handle: three folds, the subset restored
    cv = cross_validate(svm, 3)
    assert len(cv["folds"]) == 3 and all(f["TP"] + f["FP"] + f["TN"] + f["FN"] == (~m).sum() for f, m in zip(cv["folds"], cv["masks"])) and svm.subset is None
    assert 0.5 < cv["accuracy"] <= 1.0
    # new labels on the handle: the bits of a fresh float32 handle on (X32, y2)
    r2 = _result(svm.set_labels(y2).train())
    fresh = new().fit(X32, y2)
    assert _same(r2, _result(fresh)) and not np.array_equal(r2[1], r1[1])
    # per-sample penalties, L2: the diagonal form
    wgt = np.random.default_rng(3).uniform(0.5, 2.0, n)
    l2 = new("L2").create(X32, y).set_penalties(1.0, 2.0, wgt).train()
    a2 = l2.alpha
    assert l2.stats.reason == 2 and np.isfinite(a2).all() and a2.min() >= -ASTOL and np.isfinite(l2.w).all() and (a2 > ASTOL).sum() == l2.stats.n_sv
    assert np.array_equal(l2.penalties, np.where(y > 0, 1.0, 2.0) * wgt)
    for s in (svm, fresh, l2):
        s.destroy()
    ctx.close()


def test_sparse_model_scores_float32_dense_samples():
    """A model trained on CSR samples of d = 200 scores float32 dense test samples (pmh_svm_predict_f32 on a handle that was not created on float32) within the
    dot-product bound of its CSR scores of the same values: both sum at most d + 1 fp64 terms, in different orders, so each is within gamma_{d+2} (|x|.|w| + |b|) of
    the exact score.  And a float32-trained handle scores CSR samples (the other direction)."""
    ctx = pa.Context(0)
    p = P.svm_sparse(300, 200, 12, 1.0, 0.5)
    d = 200
    X32 = p["X"].toarray().astype(F32)
    Xc = p["X"].copy()
    Xc.data = Xc.data.astype(F32).astype(np.float64)  # the CSR values the float32 samples widen to
    s = pa.SVM(ctx, "L1", 1.0, True, "-qps_rtol 1e-6").fit(Xc, p["y"])
    Sc = s.decision_function(Xc)
    n = X32.shape[0]
    Xd, sd, ld = VecF32.from_numpy(ctx, X32.ravel()), ctx.vec(n), ctx.vec(n)
    assert s.sample_dtype is np.float64
    check(s.L.pmh_svm_predict_f32(s.h, n, Xd.p, sd.p, ld.p))
    Sd = sd.to_numpy()
    bound = 2 * gamma(d + 2) * (np.abs(X32.astype(np.float64)) @ np.abs(s.w) + abs(s.b))
    print("CSR model, float32 dense samples: max |diff| / bound", (np.abs(Sd - Sc) / bound).max())
    assert (np.abs(Sd - Sc) <= bound).all() and np.array_equal(ld.to_numpy(), np.where(Sd >= 0, 1.0, -1.0))
    cnt = (ct.c_longlong * 4)()
    yd = ctx.vec_from(p["y"])
    check(s.L.pmh_svm_test_f32(s.h, n, Xd.p, yd.p, cnt))
    assert sum(cnt) == n
    s.set_calibration(-0.8, 0.1)
    pd = ctx.vec(n)
    check(s.L.pmh_svm_predict_proba_f32(s.h, n, Xd.p, pd.p))
    assert (np.abs(pd.to_numpy() - np_sigma(-0.8 * Sd + 0.1)) <= 32.0 * EPS).all()
    check(s.L.pmh_svm_calibrate_f32(s.h, n, Xd.p, yd.p))
    assert s.calibration == platt_fit(ctx, Sd, p["y"])[:2]
    # the other direction: a handle created on float32 samples scores CSR and fp64 test samples of the same values
    t = pa.SVM(ctx, "L1", 1.0, True, "-qps_rtol 1e-6", sample_dtype=F32).fit(X32, p["y"])
    bt = 2 * gamma(d + 2) * (np.abs(X32.astype(np.float64)) @ np.abs(t.w) + abs(t.b))
    assert (np.abs(t.decision_function(Xc) - t.decision_function(X32)) <= bt).all()
    Xdd, s2 = ctx.vec_from(X32.astype(np.float64).ravel()), ctx.vec(n)
    check(t.L.pmh_svm_predict(t.h, n, Xdd.p, s2.p, None))
    assert np.array_equal(s2.to_numpy(), t.decision_function(X32))  # (d = 200: the generic sweep, the same bits from either type)
    for v in (Xd, sd, ld, yd, pd, Xdd, s2):
        v.free()
    s.destroy(), t.destroy()
    ctx.close()


# ---- 7. errors -------------------------------------------------------------------------------------------------------------------------------------------------------
def test_errors():
    ctx = pa.Context(0)
    y = np.where(np.arange(10) % 2 == 0, 1.0, -1.0)
    X = np.random.default_rng(0).standard_normal((10, 257))
    # d = 257: PMH_ERR_ARG with the message of the fp64 entry (the argument check is written once for both)
    assert _raises(PMH_ERR_ARG, pa.MatCreateSVMDual, ctx, X.astype(F32), y, sample_dtype=F32) == _raises(PMH_ERR_ARG, pa.MatCreateSVMDual, ctx, X, y)
    m32 = _raises(PMH_ERR_ARG, pa.SVM(ctx, sample_dtype=F32).create, X.astype(F32), y)
    assert m32 == _raises(PMH_ERR_ARG, pa.SVM(ctx).create, X, y) and "d <= 64 * SVM_KMAX" in m32
    # test samples of another width: refused by the front end before any upload, as on an fp64 handle; no samples at all: the library's argument check
    p = rounded("svm_offset", 301, 37, 2.0)
    s = pa.SVM(ctx, options=OPTS, sample_dtype=F32).fit(p["X32"], p["y"])
    for f in (s.decision_function, s.predict, s.predict_proba):
        with pytest.raises(ValueError, match=r"\(n, 37\)"):
            f(np.zeros((5, 36), dtype=F32))
    with pytest.raises(ValueError):
        s.calibrate(np.zeros((5, 36), dtype=F32), np.ones(5))
    sd = ctx.vec(5)
    assert _raises(PMH_ERR_ARG, lambda: check(s.L.pmh_svm_predict_f32(s.h, 5, None, sd.p, None))) == _raises(PMH_ERR_ARG, lambda: check(s.L.pmh_svm_predict(s.h, 5, None, sd.p, None)))
    # a CSR model wider than the dense sweeps refuses float32 dense samples with the fp64 entry's message
    q = P.svm_sparse(100, 300, 12, 1.0, 0.5)
    c = pa.SVM(ctx, options=OPTS).fit(q["X"], q["y"])
    Xd = VecF32.from_numpy(ctx, np.zeros(5 * 300, dtype=F32))
    m = _raises(PMH_ERR_ARG, lambda: check(c.L.pmh_svm_predict_f32(c.h, 5, Xd.p, sd.p, None)))
    assert "d <= 256" in m and m == _raises(PMH_ERR_ARG, c.decision_function, np.zeros((5, 300)))
    # a storage type that is neither
    with pytest.raises(ValueError, match="sample_dtype"):
        pa.SVM(ctx, sample_dtype=np.float16)
    with pytest.raises(ValueError, match="sample_dtype"):
        pa.MatCreateSVMDual(ctx, X[:, :8], y, sample_dtype=np.float16)
    Xd.free(), sd.free()
    s.destroy(), c.destroy()
    ctx.close()
