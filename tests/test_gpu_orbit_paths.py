"""GPU tests of the orbit GEMM (storage "class_orbit"): every instantiation of k_fxo_gemm16 that fxo_gemm dispatches, every plan variant of fxo_prepare and both finishing
kernels, against an independent reference -- W_c is loaded directly (MatExplicitDual.test_load_class: no K^+ solve), the structure of every case is asserted through
orbit_plan_info, integer data are compared with == against an int64 product, real data component by component against numpy.longdouble within
(n_c + 8) 2^-53 (|W| |x|)_i (tests/orbit_cases.py: cases, data, references and where the bound comes from).

Entries of Y off every block's touched positions are exactly zero, in every case and under every plan variant: a column is listed for a whole row tile, and the finishing
kernel sums and writes a (row, column) pair only where the block of that column touches the row (its device copy of the touch mask)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import orbit_cases as oc
import permon_amd as pa
from permon_amd._lib import check

pytestmark = pytest.mark.gpu

PLAN_ENV = ("PMH_FXO_TM", "PMH_FXO_NO_KSEG", "PMH_FXO_NO_STREAMK", "PMH_FXO_SEGMIN", "PMH_FXO_SLOTS", "PMH_FXO_MINCH", "PMH_FXO_SPLIT", "PMH_FXO_NO_PRUNE")
SINGLE = [("single", tm, 128) for tm in (144, 128, 112, 96, 80)]
MULTI = [("multi", tm, tn) for tm in (144, 128, 112, 96, 80) for tn in (128, 64)] + [("multi", tm, 48) for tm in (192, 128, 64)]
LAUNCHED = set()  # the instantiations plan_info reported over the module (test_all_instantiations_launched, last in the file)
SEEN = {}  # (case, variant) -> plan_info rows, for the assertions over several variants
WORST = [0.0]


@pytest.fixture(scope="module")
def ctx():
    c = pa.Context(0)
    v = C.c_int()
    check(c.L.pmh_get_knob(b"orbit_adapted", C.byref(v)))
    check(c.L.pmh_set_knob(b"orbit_adapted", 0))
    yield c
    check(c.L.pmh_set_knob(b"orbit_adapted", v.value))
    c.close()


class Operator:
    """The case's operator with W loaded directly; the environment variables of the plan are set around the load only."""

    def __init__(self, ctx, d, monkeypatch, env=None, stripe=None):
        self.ctx, self.d = ctx, d
        K = sp.identity(d.N, format="csr")  # never solved with
        self.K = pa.MatBlockDiag.from_scipy(ctx, d.block_rowstart, K)
        self.B = pa.MatGluing(ctx, d.N, d.n_lambda, d.leaf_row, d.leaf_root, d.leaf_sign)
        extra = [c["extra"] for c in d.cls]
        self.E = pa.MatExplicitDual(self.B, self.K, storage="class_orbit", block_class=d.block_class, class_extra=extra)
        if stripe is not None:
            self.E.set_stripe(*stripe)
        for ci, c in enumerate(d.cls):
            assert np.array_equal(self.E.class_union(ci), c["urel"])
            if c["n_c"]:
                assert self.E.set_class_symmetry(ci, c["perm"], c["sign"]) == c["nsym"]
        with monkeypatch.context() as m:
            for k in PLAN_ENV:
                m.delenv(k, raising=False)
            for k, v in (env or {}).items():
                m.setenv(k, str(v))
            self.load(real=False)
        self.info = [self.E.orbit_plan_info(ci) for ci in range(len(d.cls))]
        self.layout = [(p["xoff"], p["ld"], p["slots"]) for p in self.info]
        for p in self.info:
            if p["n_c"]:
                LAUNCHED.add(("single", p["tm"], 128) if p["launch"] == 0 else ("multi", p["tm"], 48 if p["tnw"] else p["tn"]))
        assert self.E.compressed_size()[0] == d.nX

    def load(self, real):
        for ci, c in enumerate(self.d.cls):
            if c["n_c"]:
                self.E.test_load_class(ci, self.d.W(ci, real))

    def dense(self, x):
        xv, yv = self.ctx.vec_from(x), self.ctx.vec(self.d.nX)
        self.E.dense_mult(xv, yv)
        y = yv.to_numpy()
        xv.free(), yv.free()
        return y

    def destroy(self):
        self.E.destroy(), self.B.destroy(), self.K.destroy()


_refs = {}


def _reference(d, layout, real):
    """One reference per case and kind, shared by every variant of the case (the layout does not depend on the plan)."""
    key = (d.case.name, real)
    if key not in _refs:
        xs = d.X(real)
        _refs[key] = (tuple(layout), xs, d.scatter(xs, layout)) + d.reference(xs, real, layout)
    assert _refs[key][0] == tuple(layout)
    return _refs[key][1:]


def check_structure(op, tm_forced=None):
    """What the case is meant to be, through plan_info: layout, class structure, the row tile rule, the launch and finishing kinds."""
    d = op.d
    for ci, (c, exp, p) in enumerate(zip(d.cls, d.case.expect, op.info)):
        assert (p["n_c"], p["ld"], p["slots"], p["groups"], p["xoff"]) == (c["n_c"], c["ld"], c["S"], c["groups"], c["xoff"])
        if not c["n_c"]:
            assert p["workgroups"] == 0
            continue
        reps = oc.orbits(c["pm"])[0]
        assert (p["nsym"], p["M"], p["rep0"], p["rep1"]) == (c["nsym"], reps.size, 0, reps.size) and p["nsymp"] % 16 == 0 and p["nsymp"] >= p["nsym"]
        tm, tnw = oc.expected_row_tile(reps.size, c["S"], c["nsym"])
        if tm_forced and not tnw:
            tm = tm_forced
        assert (p["tm"], p["tnw"]) == (tm, tnw) and p["Mp"] == p["row_tiles"] * tm and p["Mp"] - tm < p["M"] <= p["Mp"]
        assert p["chunks"] * 16 >= p["n_c"] and p["segments"] >= 1 and p["units"] == p["groups"] * p["row_tiles"] * p["segments"] and 1 <= p["units_work"] <= p["units"]
        for key in ("tn", "tnw", "launch", "finish", "row_tiles"):
            if key in exp:
                assert p[key] == exp[key], (d.case.name, ci, key, p[key])
        if c["S"] == 8:
            assert p["tn"] == 128
        assert p["finish"] == (1 if len(d.cls) > 1 else 0)


def check_integer(op, share=None):
    """Every integer check of one loaded operator; share = (r, size): a stripe's partial result is returned instead of compared."""
    d = op.d
    xs, x, ref, _ = _reference(d, op.layout, False)
    y = op.dense(x)
    assert np.array_equal(y.view(np.int64), op.dense(x).view(np.int64))  # two applies: the same bits
    touched = d.touched_mask(op.layout)
    assert not np.any(y[~touched])  # untouched entries are exactly zero: padding rows, slots without a block, rows a block does not touch
    if share is not None:
        return y
    assert np.array_equal(y[touched], ref[touched].astype(np.float64))
    for b in range(d.nblocks):
        Wb, g = op.E.block(b)
        ci, k = d.order[b]
        assert np.array_equal(g, d.block_rowstart[b] + d.cls[ci]["rel"][k])
        assert np.array_equal(Wb, d.block_matrix(b).astype(np.float64))
    lam = np.random.default_rng(3).integers(-3, 4, size=d.n_lambda)
    lv, fv = op.ctx.vec_from(lam.astype(np.float64)), op.ctx.vec(d.n_lambda)
    op.E.mult(lv, fv)
    assert np.array_equal(fv.to_numpy(), d.F_reference(lam).astype(np.float64))
    lv.free(), fv.free()
    return y


def check_real(op):
    """The component-wise bound on the real data (the same plan, W reloaded)."""
    d = op.d
    op.load(real=True)
    xs, x, ref, mag = _reference(d, op.layout, True)
    y = op.dense(x)
    touched = d.touched_mask(op.layout)
    worst = 0.0
    for ci, c in enumerate(d.cls):
        if not c["n_c"]:
            continue
        m = touched.copy()
        lo, hi = op.layout[ci][0], op.layout[ci][0] + c["groups"] * c["ld"] * c["S"]
        m[:lo], m[hi:] = False, False
        err, bound = np.abs(y[m].astype(np.longdouble) - ref[m]), (c["n_c"] + 8) * oc.U53 * mag[m]
        print("orbit GEMM %s class %d: worst err / bound %.3e" % (d.case.name, ci, float((err / bound).max())))
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound)
    WORST[0] = max(WORST[0], worst)
    return worst


def run_case(ctx, name, monkeypatch, env=None, variant="default", tm_forced=None):
    d = oc.data(name)
    op = Operator(ctx, d, monkeypatch, env)
    try:
        SEEN[(name, variant)] = op.info
        print("plan_info %s [%s]: %s" % (name, variant, [[p[k] for k in pa.MatExplicitDual.ORBIT_PLAN_FIELDS] for p in op.info]))
        check_structure(op, tm_forced)
        check_integer(op)
        check_real(op)
    finally:
        op.destroy()
    return op.info


@pytest.mark.parametrize("name", list(oc.CASES))
def test_case(ctx, name, monkeypatch):
    """Every case under the default plan: single-class kernel (two ragged row tiles; three column tiles; one full column tile), two groups, the table-driven kernels at
    TN = 64 / 128 / 48, merged and per-class launches with k_fxo_fin_all, a class without touched dofs, and the edges (n_c a multiple of 32, n_c = 1, M = 1)."""
    info = run_case(ctx, name, monkeypatch)
    p = info[0]
    if name == "box8_two_tiles":
        assert p["launch"] == 0 and p["row_tiles"] == 2 and p["M"] % p["tm"]
    if name == "cube48_three_coltiles":
        assert p["launch"] == 0 and p["nsym"] * 8 == 3 * 128 and p["units"] == 1 and p["workgroups"] == 3 * p["max_split"]  # one unit: workgroups = column tiles x pieces
    if name == "box16_one_coltile":
        assert p["launch"] == 0 and p["nsym"] * 8 == 128 and p["units"] == 1 and p["workgroups"] == p["max_split"]
    if name == "two_groups_11":
        assert p["groups"] == 2 and p["units"] == 2 * p["row_tiles"] * p["segments"]
    if name == "one_dof":
        assert p["n_c"] == 1 and p["chunks"] == 1 and p["M"] == 1  # a segment shorter than one chunk
    if name == "nc_multiple_of_32":
        assert p["ld"] == p["n_c"] + 32


@pytest.mark.parametrize("tm", [144, 128, 112, 96, 80])
@pytest.mark.parametrize("name", ["box8_two_tiles", "pair8_tn64", "triple16_tn64", "pair48_tn128", "merged_two_tiles"])
def test_row_tiles(ctx, name, tm, monkeypatch):
    """Every row tile through PMH_FXO_TM: the single-class kernel (two row tiles, the second ragged, at every size), the table-driven kernel at TN = 64 (8 and 16 operations)
    and at TN = 128 (48 operations x 2 blocks; two 8-block classes in one merged launch)."""
    info = run_case(ctx, name, monkeypatch, {"PMH_FXO_TM": tm}, "tm%d" % tm, tm_forced=tm)
    for p in info:
        assert p["tm"] == tm
        if name in ("box8_two_tiles", "pair8_tn64", "merged_two_tiles"):
            assert p["row_tiles"] == 2 and p["M"] % tm
    kinds = {"box8_two_tiles": (0, 128), "pair8_tn64": (2, 64), "triple16_tn64": (2, 64), "pair48_tn128": (2, 128), "merged_two_tiles": (2, 128)}[name]
    assert all((p["launch"], p["tn"]) == kinds for p in info)


VARIANTS = {
    "no_kseg": {"PMH_FXO_NO_KSEG": 1},
    "no_streamk": {"PMH_FXO_NO_STREAMK": 1},
    "no_kseg_no_streamk": {"PMH_FXO_NO_KSEG": 1, "PMH_FXO_NO_STREAMK": 1},
    "segmin1": {"PMH_FXO_SEGMIN": 1},
    "segmin1_slots4096": {"PMH_FXO_SEGMIN": 1, "PMH_FXO_SLOTS": 4096},
    "slots48": {"PMH_FXO_SLOTS": 48},
    "slots4096_minch1": {"PMH_FXO_SLOTS": 4096, "PMH_FXO_MINCH": 1},
    "split3": {"PMH_FXO_SPLIT": 3},
    "split11": {"PMH_FXO_SPLIT": 11},
    "split11_minch1": {"PMH_FXO_SPLIT": 11, "PMH_FXO_MINCH": 1},  # more than 8 splits also where no unit has 88 chunks
    "no_prune": {"PMH_FXO_NO_PRUNE": 1},
}
VARIANT_CASES = {"cube48_multi_tile": {"PMH_FXO_TM": 80}, "pair8_tn64": {}}  # two row tiles of 80 at 48 operations; TN = 64


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", list(VARIANT_CASES))
def test_plan_variants(ctx, name, variant, monkeypatch):
    """Every plan variant against the ONE reference of the case."""
    base = VARIANT_CASES[name]
    info = run_case(ctx, name, monkeypatch, dict(base, **VARIANTS[variant]), variant, tm_forced=base.get("PMH_FXO_TM"))
    p = info[0]
    if name == "cube48_multi_tile":
        assert p["row_tiles"] == 2 and p["launch"] == 0
    if variant == "split11_minch1":
        assert p["max_split"] > 8  # fxo_fin_body's tail loop (PMH_FXO_SPLIT=11 alone: test_more_than_eight_splits)
    if variant == "split3":
        assert p["max_split"] == 3
    if variant in ("no_kseg", "no_kseg_no_streamk", "no_prune"):
        assert p["segments"] == 1
    if variant.startswith("segmin1") and name == "cube48_multi_tile":  # (the two blocks of the TN = 64 case never list more than one column tile: its segments are joined again)
        assert p["segments"] > 1


def test_plan_variants_reach_the_paths(ctx, monkeypatch):
    """Over the variants: some plan has workgroups with two or more items (stream-K pieces that end one unit and begin the next)."""
    for name, base in VARIANT_CASES.items():
        if (name, "default") not in SEEN:
            run_case(ctx, name, monkeypatch, base, "default", tm_forced=base.get("PMH_FXO_TM"))
        for variant in VARIANTS:
            if (name, variant) not in SEEN:
                run_case(ctx, name, monkeypatch, dict(base, **VARIANTS[variant]), variant, tm_forced=base.get("PMH_FXO_TM"))
    rows = [p for (name, _), info in SEEN.items() if name in VARIANT_CASES for p in info]
    assert any(p["workgroups_multi"] > 0 for p in rows)
    assert any(p["max_split"] > 8 for p in rows) and any(p["segments"] > 1 for p in rows)


def test_more_than_eight_splits(ctx, monkeypatch):
    """PMH_FXO_SPLIT=11 alone splits a unit 11 ways only where it has 88 chunks (8 per split at least): the one segment of the one-block class with two row tiles of 192
    (n_c = 1440: 90 chunks) -- fxo_fin_body sums the first 8 splits in its unrolled block and the other 3 in its tail loop."""
    info = run_case(ctx, "single_two_tiles_192", monkeypatch, {"PMH_FXO_SPLIT": 11}, "split11")
    assert info[0]["segments"] == 1 and info[0]["chunks"] >= 88 and info[0]["max_split"] == 11 and info[0]["tnw"] == 48


@pytest.mark.parametrize("name", ["box8_two_tiles"])
def test_stripes(ctx, name, monkeypatch):
    """set_stripe(r, 3): every rank multiplies its share of the k range; the three integer results sum exactly to the reference, each reproducible."""
    d = oc.data(name)
    total = np.zeros(d.nX)
    for r in range(3):
        op = Operator(ctx, d, monkeypatch, None, stripe=(r, 3))
        try:
            p = op.info[0]
            assert p["row_tiles"] == 2 and (p["rep0"], p["rep1"]) == (0, p["M"]) and 1 <= p["units_work"] <= p["units"]
            total += check_integer(op, share=(r, 3))
        finally:
            op.destroy()
    xs, x, ref, _ = _reference(d, op.layout, False)
    touched = d.touched_mask(op.layout)
    assert np.array_equal(total[touched], ref[touched].astype(np.float64))


def test_untouched_entries_zero(ctx, monkeypatch):
    """Entries of Y off every block's touched positions are exactly zero, every case under the default plan -- also after an apply with ANOTHER multivector on the same
    operator (nothing stale), and with every entry of X non-zero on the touched positions.  (Before the finishing kernel read the touch mask it wrote every (row, column)
    pair of a tile's list: 0 ... 6954 non-zero untouched entries per case, docs/LAB_NOTEBOOK.md.)"""
    bad = {}
    for name in oc.CASES:
        d = oc.data(name)
        op = Operator(ctx, d, monkeypatch)
        try:
            xs, x, ref, _ = _reference(d, op.layout, False)
            touched = d.touched_mask(op.layout)
            for xv in (x, -2.0 * x):
                y = op.dense(xv)
                if np.any(y[~touched]):
                    bad[name] = int(np.count_nonzero(y[~touched]))
            print("untouched entries of Y, %s: %d of %d non-zero" % (name, bad.get(name, 0), int((~touched).sum())))
        finally:
            op.destroy()
    assert not bad, bad


@pytest.mark.parametrize("name,env", [("triple16_tn64", {}), ("cube48_multi_tile", {"PMH_FXO_TM": 80})])
def test_padded_k_reads_the_zero_row(ctx, name, env, monkeypatch):
    """The padded k positions of a segment must gather the ZERO row of X: their columns of A are zero, so on finite data 0 x anything leaves no trace.  One entry of X
    at position 0 set to +inf does: a padded position that gathered row 0 would add 0 x inf = NaN to every sum of that block's columns, while the true product is
    sign(W[r][0]) inf on the block's rows (column 0 of W has no zero in these cases) and unchanged for every other block."""
    d = oc.data(name)
    op = Operator(ctx, d, monkeypatch, env)
    try:
        p = op.info[0]
        assert p["chunks"] * 16 > p["n_c"]  # there are padded positions
        xs = [x.astype(np.float64) for x in d.X()]
        b = next(b for b in range(d.nblocks) if d.cls[d.order[b][0]]["pos"][d.order[b][1]][0] == 0)
        assert d.order[b][0] == 0 and np.all(d.W(0)[:, 0] != 0)
        xs[b][0] = np.inf
        y = op.dense(d.scatter(xs, op.layout))
        _, _, ref, _ = _reference(d, op.layout, False)
        for c in range(d.nblocks):
            idx = d.index(c, op.layout)
            want = np.sign(d.block_matrix(b)[:, 0]) * np.inf if c == b else ref[idx].astype(np.float64)
            assert np.array_equal(y[idx], want)
    finally:
        op.destroy()


def test_errors(ctx, monkeypatch):
    """PMH_ERR_ARG / PMH_ERR_STATE of the test entries: another storage, a class out of range, a missing symmetry, no plan yet."""
    d = oc.data("one_orbit")
    K = pa.MatBlockDiag.from_scipy(ctx, d.block_rowstart, sp.identity(d.N, format="csr"))
    B = pa.MatGluing(ctx, d.N, d.n_lambda, d.leaf_row, d.leaf_root, d.leaf_sign)
    W = d.W(0).astype(np.float64)
    E = pa.MatExplicitDual(B, K, storage="class", block_class=d.block_class)
    for call in (lambda: E.test_load_class(0, W), lambda: E.orbit_plan_info(0)):
        with pytest.raises(pa.PermonHipError) as e:
            call()
        assert e.value.code == 2  # PMH_ERR_ARG
    E.destroy()
    E = pa.MatExplicitDual(B, K, storage="class_orbit", block_class=d.block_class)
    with pytest.raises(pa.PermonHipError) as e:
        E.orbit_plan_info(0)
    assert e.value.code == 3  # PMH_ERR_STATE: no plan yet
    with pytest.raises(pa.PermonHipError) as e:
        E.test_load_class(0, W)
    assert e.value.code == 3  # PMH_ERR_STATE: no symmetries
    with pytest.raises(pa.PermonHipError) as e:
        check(ctx.L.pmh_fexplicit_test_load_class(E.h, 1, W.ctypes.data_as(C.c_void_p)))
    assert e.value.code == 2
    E.destroy(), B.destroy(), K.destroy()


def test_all_instantiations_launched(ctx):
    """Coverage: the 18 instantiations of k_fxo_gemm16 that fxo_gemm dispatches were all launched by the tests above (this test is the last of the file)."""
    print("orbit GEMM, real data: worst err / bound over the module %.3e" % WORST[0])
    missing = [k for k in SINGLE + MULTI if k not in LAUNCHED]
    assert len(SINGLE + MULTI) == 18 and not missing, missing
