"""The one-launch projector (k_gt_fused1d of csrc/qppf.hip) with the MPGP vector phase folded in, the path of every penalised operator the dual-space chain does not
take and of chain = 0: the staged operator of tests/test_gpu_chain_paths.py at the sizes where G0 gets the long-row plan (tests/dual_cases.py PROJECTOR_CASES, tied
to what they reach in tests/test_dual_reference_host.py), created with the knob "chain" at 0.

Every comparison is exact.  The expected values never come from the kernel under test: the plain product is the unfused sequence of the same operator (knob gt_fusion
= 0: the projector's separate launches and the Vec kernels), the block partials are those of k_p1_dots and k_axpy + k_split_setp as tests/dual_cases.py restates them
on the 256-thread grid (pinned by tests/test_gpu_mpgp_phases.py), and the ||G u|| request riding on the product is held to the two launches of
pmh_qppf_apply_G_norm2."""
import ctypes as C

import numpy as np
import pytest

import dual_cases as D
import permon_amd as pa
from permon_amd._lib import check
from test_gpu_chain_paths import CAP, SENT, SENT_PINNED, SUP, Chained, _rows, _same

pytestmark = pytest.mark.gpu

ONE_LAUNCH, PLAIN = 2, 5  # PMH_PEN_ONE_LAUNCH, PMH_PEN_PLAIN
SLOT = 41
BOUNDS = (("lb", "ub"), ("lb",), ("ub",), ())


@pytest.fixture(scope="module")
def ctx():
    c = pa.Context(0)
    yield c
    for knob in (b"chain", b"gt_fusion", b"vec_epi"):
        check(c.L.pmh_set_knob(knob, 1))
    c.close()


def _form(ctx, ch):
    f = C.c_int(-1)
    check(ctx.L.pmh_op_penalized_test_form(ch.A.h, C.byref(f)))
    return f.value


@pytest.fixture(scope="module", params=list(D.PROJECTOR_CASES))
def setup(ctx, request):
    """The operator, and the product of the unfused sequence on the case's x -- computed once, never written again."""
    case = D.chain_case(request.param)
    ch = Chained(ctx, case, chain=0)
    x = ch.vec(case["x"])
    assert _form(ctx, ch) == ONE_LAUNCH
    check(ctx.L.pmh_set_knob(b"gt_fusion", 0))
    try:
        assert _form(ctx, ch) == PLAIN
        y0 = ch.apply(0, x)["y"]
    finally:
        check(ctx.L.pmh_set_knob(b"gt_fusion", 1))
    assert _form(ctx, ch) == ONE_LAUNCH and np.all(np.isfinite(y0))
    y0.setflags(write=False)
    yield ch, case, x, y0
    ch.close()


def _untouched(got, what):
    _same(got["pinned"], _rows(None, 0, 0, True), (what, "the pinned block partials keep their sentinel: this path writes device rows only"))


def test_plain_product_equals_the_unfused_sequence(setup):
    ch, case, x, y0 = setup
    got = ch.apply(0, x)
    _same(got["y"], y0, "k_gt_fused1d<0> against the product with gt_fusion = 0")
    _same(got["partials"], _rows(None, 0, 0, False), "plain product: block partials untouched")
    _untouched(got, "plain product")
    assert (got["nblocks"], got["replayed"]) == (0, 0)


def test_p1_epilogue_equals_k_p1_dots(setup):
    ch, case, x, y0 = setup
    n, nwg = case["n"], D.vec_grid(case["n"])
    pc = D.phase_case(n, "both", 3)
    for bounds in BOUNDS:
        e = dict(g=pc["g"], xx=pc["x"], lb=pc["lb"] if "lb" in bounds else None, ub=pc["ub"] if "ub" in bounds else None)
        got = ch.apply(1, x, **e)
        _same(got["y"], y0, ("P1, Ap", bounds))
        _same(got["partials"], _rows(D.p1_dots(case["x"], y0, e["g"], e["xx"], e["lb"], e["ub"]), 4, nwg, False), ("P1, block partials rows 4..6", bounds))
        _untouched(got, ("P1", bounds))
        assert (got["nblocks"], got["replayed"]) == (nwg, 0)


def test_gradient_split_epilogue_equals_k_axpy_and_k_split_setp(setup):
    ch, case, x, y0 = setup
    n, nwg = case["n"], D.vec_grid(case["n"])
    pc = D.phase_case(n, "both", 3)
    g = y0 + -1.0 * pc["b"]  # k_axpy(g, -1, b)
    for bounds in BOUNDS:
        lb, ub = pc["lb"] if "lb" in bounds else None, pc["ub"] if "ub" in bounds else None
        r = D.split_setp(case["x"], g, lb, ub, D.ASTOL, emit=False)
        got = ch.apply(2, x, b=pc["b"], lb=lb, ub=ub)
        _same(got["y"], g, ("gradient split, g", bounds))
        _same(got["gf"], r["gf"], ("gradient split, gf", bounds))
        _same(got["p"], r["p"], ("gradient split, p", bounds))
        _same(got["partials"], _rows(r["partials"], 0, nwg, False), ("gradient split, block partials rows 0..3", bounds))
        _untouched(got, ("gradient split", bounds))
        assert (got["nblocks"], got["replayed"]) == (nwg, 0)


def test_the_epilogue_is_refused_where_the_product_has_none(ctx, setup):
    """vec_epi = 0 and the unfused sequence decline; the chain's arguments are not for this operator."""
    ch, case, x, y0 = setup
    pc = D.phase_case(case["n"], "both", 3)
    for knob in (b"vec_epi", b"gt_fusion"):
        check(ctx.L.pmh_set_knob(knob, 0))
        try:
            with pytest.raises(pa.PermonHipError, match="no vector epilogue") as e:
                ch.apply(2, x, b=pc["b"])
            assert e.value.code == SUP
        finally:
            check(ctx.L.pmh_set_knob(knob, 1))
    for kw in (dict(in_slot=1), dict(same_input=1)):
        with pytest.raises(pa.PermonHipError, match="does not run on the dual-space chain") as e:
            ch.apply(2, x, b=pc["b"], **kw)
        assert e.value.code == SUP


def test_norm_request_riding_on_the_product_equals_the_projectors_two_launches(ctx, setup):
    ch, case, x, y0 = setup
    m = case["m"]
    u = ch.vec(D.phase_case(case["n"], "none", 5)["x"])

    def run(armed):
        Gu, y = ch.vec(np.full(m, SENT)), ch.vec(np.full(case["n"], SENT))
        scal, served = (C.c_double * 2)(SENT, SENT_PINNED), C.c_int(-1)
        check(ctx.L.pmh_op_penalized_test_aux_normG(ch.A.h, armed, u.p, Gu.p, SLOT, x.p, y.p, scal, C.byref(served)))
        return Gu.to_numpy(), np.array(list(scal)), served.value, y.to_numpy()

    Gu0, scal0, served0, _ = run(0)
    assert served0 == 0 and scal0[0] == scal0[1] and np.isfinite(scal0[0]) and scal0[0] > 0.0 and np.all(np.isfinite(Gu0))
    Gu1, scal1, served1, y = run(1)
    assert served1 == 1
    _same(Gu1, Gu0, "T G0 u from workgroup 0 of k_gt_fused1d against pmh_qppf_apply_G_norm2")
    _same(scal1, scal0, "||T G0 u||^2, device slot and pinned mirror")
    _same(y, y0, "the product the request rode on")
    # where the request cannot ride it is dropped: the caller's own launches follow
    check(ctx.L.pmh_set_knob(b"gt_fusion", 0))
    try:
        Gu2, scal2, served2, y = run(1)
    finally:
        check(ctx.L.pmh_set_knob(b"gt_fusion", 1))
    assert served2 == 0
    _same(Gu2, np.full(m, SENT), "a dropped request writes nothing")
    _same(scal2, np.array([SENT, SENT_PINNED]), "a dropped request leaves the slot alone")
    _same(y, y0, "the product of a dropped request")
