"""The five kernels of the dual-space chain (csrc/dualchain.hip: k_dc_emit, k_dc_norm, k_dc_gather, k_dc_scatter, k_dc_final) and the emission of the MPGP vector
kernels (pmh_emit_tail of csrc/emit_inline.h with live targets), on a staged operator from three CSR matrices (pmh_op_test_create_staged) whose shapes are chosen
for the edges, against the numpy restatement of tests/dual_cases.py -- which tests/test_dual_reference_host.py ties to long-double arithmetic and to the plans
each case is named after, without a GPU.

Every comparison is exact (==, NaN equal to NaN), one assertion per vector; every intermediate one application leaves behind is compared, and the info entry must
show the plan (W, NU, records, partner rows, tails) the case is named after.  S = (G0 G0')^-1 and T' come from the projector's set-up on the matrix cores, whose
inner order the source does not fix: they are read back and taken as given by the restatement -- how they are APPLIED is what is pinned.  The middle stage has
at most two entries per row (a sum of two products is the same in either order): it has its own tests."""
import ctypes as C

import numpy as np
import pytest

import dual_cases as D
import permon_amd as pa
from permon_amd._lib import MpgpPhaseTest, check

pytestmark = pytest.mark.gpu

SUP = 4  # PMH_ERR_SUP
SENT, SENT_PINNED = 7.25e77, -3.5e66
CAP = D.MAX_BLOCKS
NORM_SLOT = 40


@pytest.fixture(scope="module")
def ctx():
    c = pa.Context(0)
    check(c.L.pmh_set_knob(b"chain", 1))
    yield c
    check(c.L.pmh_set_knob(b"chain", 1))
    c.close()


def _same(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, exp.dtype, got.shape, exp.shape)
    bad = np.argwhere(~((got == exp) | (np.isnan(got) & np.isnan(exp))))
    assert bad.size == 0, (what, "%d entries differ from the kernel-order reference" % len(bad), bad[:6].tolist(), got[tuple(bad[:6].T)], exp[tuple(bad[:6].T)])


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Chained:
    """Penalized(Projected(staged, pf, symmetric), pf, rho) of a case's matrices, with the knob "chain" as given while the penalised operator is created."""

    def __init__(self, ctx, case, chain=1, share=None):
        self.ctx, self.case, self.n, self.m = ctx, case, case["n"], case["m"]
        if share is None:
            to = lambda M: pa.CsrMat(ctx, M["nrows"], M["ncols"], M["rowptr"], M["col"], M["val"])  # noqa: E731
            self.mats = [to(case[k]) for k in ("G0", "gather", "middle", "scatter")]
            self.pf = pa.QPPF(ctx, self.mats[0], "implicit")
            h = C.c_void_p()
            check(ctx.L.pmh_op_test_create_staged(self.mats[1].h, self.mats[2].h, self.mats[3].h, C.byref(h)))
            self.F = pa.Op(ctx, h, self.n, keep=self.mats)
            self.PFP = pa.MatCreateProjected(self.F, self.pf, True)
        else:
            self.mats, self.pf, self.F, self.PFP = share.mats, share.pf, share.F, share.PFP
        self.shared = share is not None
        check(ctx.L.pmh_set_knob(b"chain", chain))
        self.A = pa.MatCreatePenalized(self.PFP, self.pf, case["rho"])
        check(ctx.L.pmh_set_knob(b"chain", 1))
        self.vecs = []

    def vec(self, a):
        v = self.ctx.vec_from(a)
        self.vecs.append(v)
        return v

    def info(self):
        info = (C.c_longlong * 10)()
        check(self.ctx.L.pmh_op_penalized_test_chain_info(self.A.h, info))
        return list(info)

    def read(self, what):
        cap = self.n + 64 * 130 + self.case["nmid"] + self.m * self.m + 64
        a, k = np.full(cap, np.nan), C.c_int()
        check(self.ctx.L.pmh_op_penalized_test_chain_read(self.A.h, what, cap, _ptr(a), C.byref(k)))
        return a[:k.value].copy()

    def apply(self, kind, x, same_input=0, in_slot=0, b=None, g=None, xx=None, lb=None, ub=None):
        """One application to the device vector x -> what y, gf, p and both copies of the block partials hold afterwards (sentinels where nothing was written)."""
        dv = {k: self.vec(v) for k, v in (("b", b), ("g", g), ("xx", xx), ("lb", lb), ("ub", ub)) if v is not None}
        p_ = lambda k: dv[k].p if k in dv else None  # noqa: E731
        y, gf, p = (self.vec(np.full(self.n, SENT)) for _ in range(3))
        pd, pp = np.full((8, CAP), SENT), np.full((8, CAP), SENT_PINNED)
        nb, rep = C.c_int(), C.c_int()
        check(self.ctx.L.pmh_op_penalized_test_mult_epi2(self.A.h, kind, same_input, in_slot, x.p, p_("b"), p_("g"), p_("xx"), p_("lb"), p_("ub"), D.ASTOL, y.p, gf.p, p.p,
                                                         _ptr(pd), _ptr(pp), C.byref(nb), C.byref(rep)))
        return dict(y=y.to_numpy(), gf=gf.to_numpy(), p=p.to_numpy(), partials=pd, pinned=pp, nblocks=nb.value, replayed=rep.value)

    def close(self):
        for v in self.vecs:
            v.free()
        self.A.destroy()
        if not self.shared:
            self.PFP.destroy(), self.F.destroy(), self.pf.destroy()
            for a in self.mats:
                a.destroy()


def _rows(rows, row0, nb, pinned):
    a = np.full((8, CAP), SENT_PINNED if pinned else SENT)
    if rows is not None:
        assert rows.shape[1] == nb
        a[row0:row0 + len(rows), :nb] = rows
    return a


def _compare_intermediates(ch, o, slot, what):
    _same(ch.read(slot), o["part"], (what, "segment sums of G0 x, target %d" % slot))
    _same(ch.read(3), o["c"], (what, "c = S G0 x"))
    _same(ch.read(4), o["mid_in"], (what, "mid_in"))
    _same(ch.read(5), o["mid_out"], (what, "mid_out"))
    _same(ch.read(6), np.concatenate([o["w"], o["wsums"]]), (what, "[w; segment sums of G0 w]"))


@pytest.mark.parametrize("name", list(D.CHAIN_CASES))
def test_chain_equals_the_restatement(ctx, name):
    case = D.chain_case(name)
    plan = D.chain_plan(case["G0"], case["gather"], case["scatter"])
    n, m, nwg, rho = case["n"], case["m"], plan["nwg"], case["rho"]
    ch = Chained(ctx, case)
    try:
        assert ch.info() == plan["info"] and (plan["W"], plan["NU"]) == D.CHAIN_CASES[name][3:], (ch.info(), plan["info"])
        S, Tt = ch.read(9).reshape(m, m), ch.read(10).reshape(m, m)
        Gu = ch.vec(np.full(m, SENT))
        check(ctx.L.pmh_op_penalized_test_norm_target(ch.A.h, Gu.p, NORM_SLOT, None, None))
        pc = D.phase_case(n, "both", 3)
        x, x2 = ch.vec(case["x"]), ch.vec(pc["x"])

        # a plain application: k_dc_emit -> scratch target, k_dc_gather, the middle stage, k_dc_scatter, k_dc_final<0>
        o = D.chain_apply(case, plan, S, case["x"], rho)
        got = ch.apply(0, x)
        _same(got["y"], o["y"], "plain application, y")
        _compare_intermediates(ch, o, 2, "plain application")
        _same(got["partials"], _rows(None, 0, nwg, False), "plain application: block partials untouched")
        _same(got["pinned"], _rows(None, 0, nwg, True), "plain application: pinned block partials untouched")
        assert (got["replayed"], got["nblocks"]) == (0, 0)
        # ... the same vector again: the last kernel alone, with another penalty
        check(ctx.L.pmh_op_penalized_set_penalty(ch.A.h, 0.625))
        got = ch.apply(0, x, same_input=1)
        assert got["replayed"] == 1
        _same(got["y"], D.chain_apply(case, plan, S, case["x"], 0.625)["y"], "replayed last stage with another rho, y")
        check(ctx.L.pmh_op_penalized_set_penalty(ch.A.h, rho))

        # P1: x is the direction; its sums go to the direction's target; rows 4..6 in both copies
        e1 = dict(g=pc["g"], xx=pc["x"], lb=pc["lb"], ub=pc["ub"])
        o = D.chain_apply(case, plan, S, case["x"], rho, 1, epi=e1)
        got = ch.apply(1, x, **e1)
        _same(got["y"], o["y"], "P1, Ap")
        _compare_intermediates(ch, o, 1, "P1")
        _same(got["partials"], _rows(o["rows"], 4, nwg, False), "P1, block partials rows 4..6")
        _same(got["pinned"], _rows(o["rows"], 4, nwg, True), "P1, pinned block partials rows 4..6")
        assert got["nblocks"] == nwg
        for bounds in (dict(lb=pc["lb"]), dict(ub=pc["ub"]), dict()):
            e = dict(g=pc["g"], xx=pc["x"], lb=None, ub=None, **{})
            e.update(bounds)
            _same(ch.apply(1, x, **e)["partials"], _rows(D.chain_apply(case, plan, S, case["x"], rho, 1, epi=e)["rows"], 4, nwg, False), ("P1 rows", sorted(bounds)))

        # the gradient split of an iterate nobody emitted: its sums go to the iterate's target, and ||T G0 u||^2 rides on the gather's extra workgroup
        e2 = dict(b=pc["b"], lb=pc["lb"], ub=pc["ub"])
        o = D.chain_apply(case, plan, S, case["x"], rho, 2, epi=dict(e2, astol=D.ASTOL))
        yn, sq = D.chain_norm(plan, o["part"], Tt)

        def check_split(got, o, what):
            _same(got["y"], o["y"], (what, "g"))
            _same(got["gf"], o["gf"], (what, "gf"))
            _same(got["p"], o["p"], (what, "p"))
            _same(got["partials"], _rows(o["rows"], 0, nwg, False), (what, "block partials rows 0..3"))
            _same(got["pinned"], _rows(o["rows"], 0, nwg, True), (what, "pinned block partials rows 0..3"))
            _same(ch.read(1), o["psums"], (what, "segment sums of G0 p"))
            assert got["nblocks"] == nwg

        got = ch.apply(2, x, **e2)
        check_split(got, o, "gradient split")
        _compare_intermediates(ch, o, 0, "gradient split")
        _same(Gu.to_numpy(), yn, "T G0 u from the gather's extra workgroup (k_dc_gather)")
        _same(ch.read(8), np.array([sq, sq]), "||T G0 u||^2, device slot and pinned mirror")
        for bounds in (dict(lb=pc["lb"]), dict(ub=pc["ub"]), dict()):
            e = dict(b=pc["b"], lb=None, ub=None)
            e.update(bounds)
            check_split(ch.apply(2, x, **e), D.chain_apply(case, plan, S, case["x"], rho, 2, epi=dict(e, astol=D.ASTOL)), ("gradient split", sorted(bounds)))
        # ... replayed: k_dc_emit and the last kernel; the norm then forms in a launch of its own (k_dc_norm)
        Gu.set_numpy(np.full(m, SENT))
        got = ch.apply(2, x, same_input=1, **e2)
        assert got["replayed"] == 1
        check_split(got, o, "replayed gradient split")
        ready = C.c_int()
        check(ctx.L.pmh_op_penalized_test_norm_target(ch.A.h, None, 0, x.p, C.byref(ready)))
        assert ready.value == 1
        _same(Gu.to_numpy(), yn, "T G0 u from k_dc_norm<%d>" % plan["NU"])
        _same(ch.read(8), np.array([sq, sq]), "||T G0 u||^2 from k_dc_norm")

        # the gradient split after an emission of the iterate (in_slot 1): the sums in the iterate's target are consumed as they are -- those of ANOTHER vector here,
        # which a kernel that formed them again would not reproduce
        check(ctx.L.pmh_op_penalized_test_emit(ch.A.h, 1, x2.p))
        sums2 = D.emit_sums(plan, case["G0"], pc["x"])
        _same(ch.read(0), sums2, "k_dc_emit through emit_begin, target 0")
        got = ch.apply(2, x, in_slot=1, **e2)
        check_split(got, D.chain_apply(case, plan, S, case["x"], rho, 2, part_in=sums2, epi=dict(e2, astol=D.ASTOL)), "gradient split on emitted sums")
        _same(ch.read(0), sums2, "the iterate's target after an application that consumed it")

        # P1 after an emission of the direction (in_slot 2): the proportioning step of MPGP writes x and p = gf on 1024-entry tiles and leaves the sums of both
        st = D.step_update(0.41, pc["x"], pc["g"], pc["p"], pc["Ap"], pc["lb"], pc["ub"], D.ASTOL, True, True)
        t = MpgpPhaseTest()
        dv = {k: ch.vec(pc[k]) for k in ("x", "g", "p", "Ap", "gf", "lb", "ub")}
        for k, v in dv.items():
            setattr(t, k, v.p)
        pd, pp = np.full((8, CAP), SENT), np.full((8, CAP), SENT_PINNED)
        t.partials_dev, t.partials_pinned, t.op = _ptr(pd), _ptr(pp), ch.A.h
        t.emit, t.setp, t.acg_host, t.astol = 1, 1, 0.41, D.ASTOL
        check(ctx.L.pmh_mpgp_test_phase(ctx.h, 1, n, C.byref(t)))
        for k in ("x", "g", "p", "gf"):
            _same(dv[k].to_numpy(), st[k], ("k_step_update<true, false, true> behind the chain", k))
        _same(pd, _rows(st["partials"], 0, nwg, False), "k_step_update<true, false, true> behind the chain, block partials")
        _same(pp, _rows(st["partials"], 0, nwg, True), "k_step_update<true, false, true> behind the chain, pinned block partials")
        sx, sp = D.emit_sums(plan, case["G0"], st["x"]), D.emit_sums(plan, case["G0"], st["p"])
        _same(ch.read(0), sx, "pmh_emit_tail of the step, target 0 (G0 x)")
        _same(ch.read(1), sp, "pmh_emit_tail of the step, target 1 (G0 p)")
        e1 = dict(g=st["g"], xx=st["x"], lb=pc["lb"], ub=pc["ub"])
        o = D.chain_apply(case, plan, S, st["p"], rho, 1, part_in=sp, epi=e1)
        got = ch.apply(1, dv["p"], in_slot=2, **e1)
        _same(got["y"], o["y"], "P1 on emitted sums, Ap")
        _same(got["partials"], _rows(o["rows"], 4, nwg, False), "P1 on emitted sums, block partials rows 4..6")
        _same(got["pinned"], _rows(o["rows"], 4, nwg, True), "P1 on emitted sums, pinned block partials rows 4..6")
        _same(ch.read(1), sp, "the direction's target after an application that consumed it")

        # every other 1024-thread kernel with the chain's emission arguments: what it writes, and the segment sums it leaves in the target of the vector it wrote
        # (0: x, 1: p) -- the other target keeps what it held
        def emitting(phase, what, wrote, target, **kw):
            t = MpgpPhaseTest()
            dv = {k: ch.vec(pc[k]) for k in ("x", "g", "p", "Ap", "gf", "lb", "ub")}
            for k, v in dv.items():
                setattr(t, k, v.p)
            pd, pp = np.full((8, CAP), SENT), np.full((8, CAP), SENT_PINNED)
            pd[0, :nwg] = D.reduction_rows(nwg, 5)[0]  # (the row k_dir_update<true> adds)
            t.partials_dev, t.partials_pinned, t.op, t.emit, t.astol = _ptr(pd), _ptr(pp), ch.A.h, 1, D.ASTOL
            for k, v in kw.items():
                setattr(t, k, v)
            before = [ch.read(0), ch.read(1)]
            check(ctx.L.pmh_mpgp_test_phase(ctx.h, phase, n, C.byref(t)))
            for k in ("x", "g", "p", "gf"):
                _same(dv[k].to_numpy(), wrote.get(k, pc[k]), (what, k))
            _same(ch.read(target), D.emit_sums(plan, case["G0"], wrote["x" if target == 0 else "p"]), (what, "segment sums in target %d" % target))
            _same(ch.read(1 - target), before[1 - target], (what, "the other target"))
            return pd

        bd = (pc["lb"], pc["ub"], D.ASTOL)
        r = D.split_setp(pc["x"], pc["g"], *bd, True)
        emitting(0, "k_split_setp<true> behind the chain", dict(gf=r["gf"], p=r["p"]), 1)
        r = D.step_update(0.41, pc["x"], pc["g"], pc["p"], pc["Ap"], *bd, False, True)
        emitting(1, "k_step_update<false, false, true> behind the chain", {k: r[k] for k in ("x", "g", "gf")}, 0, acg_host=0.41)
        pd = np.full((8, CAP), SENT)
        pd[0, :nwg] = D.reduction_rows(nwg, 5)[0]
        pnew = D.dir_update(D.sum_block_partials(pd[0], nwg) / 1.7, pc["gf"], pc["p"])
        emitting(2, "k_dir_update<true> behind the chain", dict(p=pnew), 1, nb=nwg, pAp_host=1.7)
        emitting(3, "k_prop_dir<true> behind the chain", dict(p=D.prop_dir(pc["x"], pc["g"], *bd)), 1)
        emitting(4, "k_expansion_std<true> behind the chain", dict(x=D.expansion_std(0.3, 0.7, pc["x"], pc["g"], pc["p"], pc["Ap"], *bd)), 0, afeas=0.3, alpha=0.7)
    finally:
        ch.close()


def _refusal_case(kind):
    """The small two-tile case with one thing the chain does not take."""
    c = dict(D.chain_case("n1500_m6"))
    G0 = c["G0"]
    rp, col, val = G0["rowptr"].copy(), G0["col"].copy(), G0["val"].copy()
    rng = np.random.default_rng(9)
    if kind == "m65":
        rows = [(np.arange(r, c["n"], 65).astype(np.int32), rng.uniform(0.5, 1.5, len(range(r, c["n"], 65)))) for r in range(65)]
        c.update(G0=D._csr(rows, c["n"]), m=65)
        return c
    if kind == "column_with_17_entries":
        rows = [(np.union1d(np.arange(r, c["n"], 17), [5]).astype(np.int32), None) for r in range(17)]
        c.update(G0=D._csr([(cc, rng.uniform(0.5, 1.5, len(cc))) for cc, _ in rows], c["n"]), m=17)
        return c
    a, b = rp[4], rp[4] + 1  # the first two entries of row 4
    if kind == "unsorted_columns":
        col[[a, b]], val[[a, b]] = col[[b, a]], val[[b, a]]
    else:  # duplicate_columns
        col[b] = col[a]
    c["G0"] = dict(G0, rowptr=rp, col=col, val=val)
    return c


@pytest.mark.parametrize("kind", ("m65", "column_with_17_entries", "unsorted_columns", "duplicate_columns"))
def test_chain_refusals(ctx, kind):
    """What pmh_dc_create does not take leaves the operator off the chain: the test entries say so, and the plain product is the launch sequence of chain = 0, bit
    for bit (the two operators share one projector)."""
    case = _refusal_case(kind)
    ch = Chained(ctx, case)
    off = Chained(ctx, case, chain=0, share=ch)
    try:
        for op in (ch, off):
            with pytest.raises(pa.PermonHipError, match="does not run on the dual-space chain") as e:
                op.info()
            assert e.value.code == SUP
        x = ch.vec(case["x"])
        y, y0 = ch.vec(np.full(case["n"], SENT)), ch.vec(np.full(case["n"], SENT))
        ch.A.mult(x, y), off.A.mult(x, y0)
        _same(y.to_numpy(), y0.to_numpy(), "an operator the chain refused against the chain = 0 sequence")
        assert np.all(np.isfinite(y.to_numpy()))
        if kind != "duplicate_columns":  # (the set-up of G0 G0' takes one of two duplicates: no dense reference for that one)
            G, Bg, M, Bs = (D.csr_dense(case[k]) for k in ("G0", "gather", "middle", "scatter"))
            Q = G.T @ np.linalg.solve(G @ G.T, G)
            P = np.eye(case["n"]) - Q
            ref = case["rho"] * Q @ case["x"] + P @ (Bs @ (M @ (Bg @ (P @ case["x"]))))
            assert np.linalg.norm(y.to_numpy() - ref) <= 1e-11 * np.linalg.norm(ref)
    finally:
        off.close(), ch.close()


def test_accepted_case_also_agrees_with_the_chain_off_sequence(ctx):
    """The same operator with the knob off: the separate launches, within rounding of the chain (they sum in another order)."""
    case = D.chain_case("n1500_m6")
    ch = Chained(ctx, case)
    off = Chained(ctx, case, chain=0, share=ch)
    try:
        assert ch.info()[0] == case["n"]
        with pytest.raises(pa.PermonHipError, match="does not run on the dual-space chain"):
            off.info()
        x = ch.vec(case["x"])
        y, y0 = ch.vec(np.full(case["n"], SENT)), ch.vec(np.full(case["n"], SENT))
        ch.A.mult(x, y), off.A.mult(x, y0)
        assert np.linalg.norm(y.to_numpy() - y0.to_numpy()) <= 1e-12 * np.linalg.norm(y0.to_numpy())
    finally:
        off.close(), ch.close()


def test_fused_solve_on_the_chain_equals_the_restated_solve(ctx):
    """solve_fused on the chained staged operator: both epilogues in the chain's last kernel, every vector kernel in its 1024-thread form behind a live chain, every
    sum finished by the host from the pinned block partials (hsum3 / hsum4), the proportioning step and the direction forming their scalars from block partials.
    The step string, every monitor norm and the final x equal the restated solve; the case takes CG, expansion and proportioning steps
    (tests/test_dual_reference_host.py establishes that with S computed on the host)."""
    sc = D.solve_case("chain")
    case = sc["chain"]
    plan = D.chain_plan(case["G0"], case["gather"], case["scatter"])
    ch = Chained(ctx, case)
    try:
        assert ch.info() == plan["info"]
        S = ch.read(9).reshape(case["m"], case["m"])
        steps, mon, x_ref, reason = D.solve_fused(D.ChainModel(case, plan, S), sc["b"], sc["x0"], sc["lb"], sc["ub"], 0.38, rtol=1e-4)
        assert {"c", "e", "p"} <= set(steps) and reason == 2 and len(steps) <= 61
        qp, x = pa.QP(ctx), ch.vec(sc["x0"])
        qp.SetOperator(ch.A), qp.SetRhs(ch.vec(sc["b"])), qp.SetInitialVector(x), qp.SetBox(None, ch.vec(sc["lb"]), ch.vec(sc["ub"]))
        qps = pa.QPS(ctx)
        qps.SetQP(qp), qps.SetType("mpgp"), qps.MPGPSetAlpha(0.38, direct=True), qps.MonitorSet(), qps.SetTolerances(rtol=1e-4, max_it=60)
        check(ctx.L.pmh_set_knob(b"chain_applies", 0))
        st = qps.Solve()
        got_steps, gp, gf, gc, _ = qps.MPGPGetTrace()
        applies = C.c_int()
        check(ctx.L.pmh_get_knob(b"chain_applies", C.byref(applies)))
        assert applies.value >= st.nmv > 0  # every product ran on the chain
        assert (got_steps, st.reason, st.iteration) == (steps, reason, len(steps) - 1)
        _same(gp, mon[:, 0], "monitor |gP|")
        _same(gf, mon[:, 1], "monitor |gf|")
        _same(gc, mon[:, 2], "monitor |gc|")
        _same(x.to_numpy(), x_ref, "x")
        # the same handle again from a carried gradient (pmh_mpgp_set_gradient_valid, as SMALXE hands one over): no first product, k_split_setp<true> behind the chain
        # with its four sums left to the host, a lone first P1.  The vector handed over is NOT the gradient at the starting point: a driver that formed its own
        # would take other steps
        model = D.ChainModel(case, plan, S)
        g0 = D.carried_gradient(sc, model.grad_split(sc["x0"], sc["b"], sc["lb"], sc["ub"], D.ASTOL)[0])
        steps2, mon2, x2, reason2 = D.solve_fused(model, sc["b"], sc["x0"], sc["lb"], sc["ub"], 0.38, rtol=1e-4, g0=g0)
        assert {"c", "e", "p"} <= set(steps2) and len(steps2) <= 62 and steps2 != steps
        x.set_numpy(sc["x0"])
        check(ctx.L.pmh_mpgp_test_set_gradient_valid(qps.h, ch.vec(g0).p))
        st = qps.Solve()
        got_steps, gp, gf, gc, _ = qps.MPGPGetTrace()
        assert (got_steps, st.reason, st.iteration) == (steps2, reason2, len(steps2) - 1)
        _same(gp, mon2[:, 0], "carried gradient: monitor |gP|")
        _same(gf, mon2[:, 1], "carried gradient: monitor |gf|")
        _same(gc, mon2[:, 2], "carried gradient: monitor |gc|")
        _same(x.to_numpy(), x2, "carried gradient: x")
        qps.Destroy()
    finally:
        ch.close()


def test_a_g0_with_an_empty_row_never_reaches_the_chain(ctx):
    """The projector's set-up refuses a G0 without full row rank, an empty row included: no chain case can hold one."""
    case = D.chain_case("n37_m6")
    G0 = case["G0"]
    rp = G0["rowptr"].copy()
    a, b = rp[2], rp[3]
    rp[3:] -= b - a  # row 2 loses its entries
    G = pa.CsrMat(ctx, G0["nrows"], G0["ncols"], rp, np.delete(G0["col"], np.s_[a:b]), np.delete(G0["val"], np.s_[a:b]))
    with pytest.raises(pa.PermonHipError, match="full row rank") as e:
        pa.QPPF(ctx, G, "implicit")
    assert e.value.code == 2  # PMH_ERR_ARG
    G.destroy()
