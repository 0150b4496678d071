"""The MPGP phase kernels (csrc/mpgp.hip) and the reduction finishers (k_finalize of csrc/vec.hip; pmh_block_partials, pmh_sum_block_partials and pmh_wave_all of
csrc/emit_inline.h; host_sum_row of csrc/mpgp.hip), one launch at a time through pmh_mpgp_test_phase / pmh_vec_test_finalize / pmh_mpgp_test_block_*, against the
numpy restatement of tests/dual_cases.py -- which tests/test_dual_reference_host.py ties to long-double arithmetic without a GPU.

Every comparison is exact (==, NaN equal to NaN): the library is built without contraction and every sum of these kernels has a fixed order.  Every buffer a launch
may write is preset to a sentinel and compared whole, one assertion per buffer, so that a failure names the stage and a stray write shows.  The 1024-thread
variants run with their emission targets off here: their entry map, their block partials in both copies and the sums of block partials they consume.  With the
emission arguments of a chained operator every one of them runs in tests/test_gpu_chain_paths.py, which compares the segment sums it leaves."""
import ctypes as C

import numpy as np
import pytest

import dual_cases as D
import permon_amd as pa
from permon_amd._lib import MpgpPhaseTest, check

pytestmark = pytest.mark.gpu

SENT, SENT_PINNED, SENT_SCAL = 7.25e77, -3.5e66, 1.75e55
SPLIT, STEP, DIR, PROP_DIR, EXPANSION, P1_DOTS, THREE_NORMS, OBJ = range(8)
VECS = ("x", "g", "p", "Ap", "gf")
CAP = D.MAX_BLOCKS  # row length of the context's block partials


@pytest.fixture(scope="module")
def ctx():
    c = pa.Context(0)
    yield c
    c.close()


def _same(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, exp.dtype, got.shape, exp.shape)
    bad = np.argwhere(~((got == exp) | (np.isnan(got) & np.isnan(exp))))
    assert bad.size == 0, (what, "%d entries differ from the kernel-order reference" % len(bad), bad[:6].tolist(), got[tuple(bad[:6].T)], exp[tuple(bad[:6].T)])


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def launch(ctx, phase, n, vecs, lb=None, ub=None, b=None, partials=None, scal=None, ctl=(0, 0, 0, 0), ring=None, **kw):
    """One pmh_mpgp_test_phase.  vecs: name -> array for the vectors the phase reads; every other vector is a sentinel.  Returns what every buffer holds afterwards."""
    t = MpgpPhaseTest()
    dev = {k: ctx.vec_from(vecs[k] if k in vecs else np.full(n, SENT)) for k in VECS}
    ro = {k: ctx.vec_from(v) for k, v in (("lb", lb), ("ub", ub), ("b", b)) if v is not None}
    for k in VECS:
        setattr(t, k, dev[k].p)
    for k, v in ro.items():
        setattr(t, k, v.p)
    pd = np.full((8, CAP), SENT) if partials is None else np.array(partials, np.float64)
    pp = np.full((8, CAP), SENT_PINNED)
    sd = np.full(64, SENT_SCAL) if scal is None else np.array(scal, np.float64)
    sp = np.full(64, SENT_PINNED)
    t.partials_dev, t.partials_pinned = _ptr(pd), _ptr(pp)
    t.scal_dev[:], t.scal_pinned[:] = sd.tolist(), sp.tolist()
    t.ring[:] = (np.full(48, SENT) if ring is None else np.asarray(ring, np.float64)).tolist()
    t.ctl[:] = list(ctl)
    for k, v in kw.items():
        assert hasattr(t, k), k
        setattr(t, k, v)
    check(ctx.L.pmh_mpgp_test_phase(ctx.h, phase, n, C.byref(t)))
    out = {k: dev[k].to_numpy() for k in VECS}
    out.update(partials=pd, pinned=pp, scal=np.array(t.scal_dev[:]), scal_pinned=np.array(t.scal_pinned[:]), ctl=list(t.ctl[:]), ring=np.array(t.ring[:]))
    for v in list(dev.values()) + list(ro.values()):
        v.free()
    return out


def expect(n, vecs, written=None, rows=None, row0=0, emit=False, partials=None, scal=None, scal_written=None, ctl=(0, 0, 0, 0), ring=None):
    """What every buffer must hold: the inputs and sentinels as they were, except the vectors in `written`, the leading nblocks entries of the rows `rows` writes (in
    the pinned copy too under emit) and the scalar slots in scal_written (device and pinned mirror alike)."""
    e = {k: np.array(vecs[k], np.float64) if k in vecs else np.full(n, SENT) for k in VECS}
    e.update(written or {})
    pd = np.full((8, CAP), SENT) if partials is None else np.array(partials, np.float64)
    pp = np.full((8, CAP), SENT_PINNED)
    if rows is not None:
        nb = rows.shape[1]
        assert nb == D.nblocks_of(n, emit)
        pd[row0:row0 + len(rows), :nb] = rows
        if emit:
            pp[row0:row0 + len(rows), :nb] = rows
    sd = np.full(64, SENT_SCAL) if scal is None else np.array(scal, np.float64)
    sp = np.full(64, SENT_PINNED)
    for slot, v in (scal_written or {}).items():
        sd[slot] = sp[slot] = v
    e.update(partials=pd, pinned=pp, scal=sd, scal_pinned=sp, ctl=list(ctl), ring=np.full(48, SENT) if ring is None else np.asarray(ring, np.float64))
    return e


def compare(got, exp, what):
    assert got["ctl"] == exp["ctl"], (what, "control words", got["ctl"], exp["ctl"])
    for k in VECS + ("partials", "pinned", "scal", "scal_pinned", "ring"):
        _same(got[k], exp[k], (what, k))


def _slots(base, values):
    return {base + k: v for k, v in enumerate(values)}


# ---- plain grid ----------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bounds", D.BOUNDS)
@pytest.mark.parametrize("n", D.PLAIN_N)
def test_plain_phases_equal_the_restatement(ctx, n, bounds):
    """Every phase kernel on the grid of pmh_vec_grid, followed by the driver's finalising launch: vectors, block partials and finished scalars."""
    c = D.phase_case(n, bounds)
    x, g, p, Ap, gf, b, lb, ub = (c[k] for k in ("x", "g", "p", "Ap", "gf", "b", "lb", "ub"))
    bd = dict(lb=lb, ub=ub)
    S4, S3 = [D.SUM] * 4, [D.SUM, D.SUM, D.MIN]
    scal = np.full(64, SENT_SCAL)
    scal[D.S_GP], scal[D.S_PAP], scal[D.S_APGF] = 0.6, 1.7, 0.45

    r = D.split_setp(x, g, lb, ub, D.ASTOL)
    v = dict(x=x, g=g)
    compare(launch(ctx, SPLIT, n, v, finalize=1, astol=D.ASTOL, **bd),
            expect(n, v, dict(gf=r["gf"], p=r["p"]), r["partials"], scal_written=_slots(D.S_APGF, D.finalize(r["partials"], S4))), "k_split_setp<false>")
    compare(launch(ctx, SPLIT, n, v, finalize=0, astol=D.ASTOL, **bd), expect(n, v, dict(gf=r["gf"], p=r["p"]), r["partials"]), "k_split_setp<false>, no finalising launch")

    v = dict(x=x, g=g, p=p, Ap=Ap)
    for setp in (0, 1):
        r = D.step_update(D.step_acg(scal=scal), x, g, p, Ap, lb, ub, D.ASTOL, setp)
        compare(launch(ctx, STEP, n, v, scal=scal, setp=setp, finalize=1, astol=D.ASTOL, **bd),
                expect(n, v, {k: r[k] for k in ("x", "g", "gf", "p")}, r["partials"], scal=scal, scal_written=_slots(D.S_APGF, D.finalize(r["partials"], S4))),
                "k_step_update<%d, false>" % setp)

    v = dict(gf=gf, p=p)
    compare(launch(ctx, DIR, n, v, scal=scal), expect(n, v, dict(p=D.dir_update(scal[D.S_APGF] / scal[D.S_PAP], gf, p)), scal=scal), "k_dir_update<false>")
    v = dict(x=x, g=g)
    compare(launch(ctx, PROP_DIR, n, v, astol=D.ASTOL, **bd), expect(n, v, dict(p=D.prop_dir(x, g, lb, ub, D.ASTOL))), "k_prop_dir<false>")
    v = dict(x=x, g=g, p=p, Ap=Ap)
    compare(launch(ctx, EXPANSION, n, v, afeas=0.3, alpha=0.7, astol=D.ASTOL, **bd),
            expect(n, v, dict(x=D.expansion_std(0.3, 0.7, x, g, p, Ap, lb, ub, D.ASTOL))), "k_expansion_std<false>")

    rows = D.p1_dots(p, Ap, g, x, lb, ub)
    compare(launch(ctx, P1_DOTS, n, v, finalize=1, **bd), expect(n, v, None, rows, scal_written=_slots(D.S_PAP, D.finalize(rows, S3))), "k_p1_dots")
    rows = D.three_norms(x, g, gf)
    v = dict(x=x, g=g, gf=gf)
    compare(launch(ctx, THREE_NORMS, n, v, finalize=1), expect(n, v, None, rows, scal_written=_slots(D.S_APGF, D.finalize(rows, S4))), "k_three_norms")
    rows = D.obj_from_grad(x, g, b)
    v = dict(x=x, g=g)
    compare(launch(ctx, OBJ, n, v, b=b, finalize=1), expect(n, v, None, rows, scal_written={D.S_TMP: D.finalize(rows, [D.SUM])[0]}), "k_obj_from_grad")


# ---- 1024-entry tiles ------------------------------------------------------------------------------------------------------------------------------------------------------
def _host_rows(ctx, rows, op=D.SUM):
    out = np.empty(len(rows))
    for k, r in enumerate(rows):
        v = C.c_double()
        check(ctx.L.pmh_mpgp_test_host_sum_row(_ptr(np.ascontiguousarray(r)), len(r), op, C.byref(v)))
        out[k] = v.value
    return out


@pytest.mark.parametrize("bounds", D.BOUNDS)
@pytest.mark.parametrize("n", D.EMIT_N)
def test_tile_phases_equal_the_restatement(ctx, n, bounds):
    """The 1024-thread variants: vectors, block partials on the device AND in the pinned copy, the step length and the direction's beta formed from block partials,
    and what the host then makes of the pinned rows (host_sum_row)."""
    c = D.phase_case(n, bounds)
    x, g, p, Ap, gf, lb, ub = (c[k] for k in ("x", "g", "p", "Ap", "gf", "lb", "ub"))
    bd = dict(lb=lb, ub=ub)
    nb = D.emit_blocks(n)
    seeded = np.full((8, CAP), SENT)  # the rows a P1 product and a step left behind: the kernels below add them themselves
    rr = D.reduction_rows(nb, 11)
    seeded[0, :nb], seeded[4, :nb], seeded[5, :nb] = rr[0], np.abs(rr[1]) + 1.0, 0.3 * rr[2]  # Ap'gf, p'Ap > 0, g'p

    r = D.split_setp(x, g, lb, ub, D.ASTOL, True)
    v = dict(x=x, g=g)
    got = launch(ctx, SPLIT, n, v, emit=1, astol=D.ASTOL, **bd)
    compare(got, expect(n, v, dict(gf=r["gf"], p=r["p"]), r["partials"], emit=True), "k_split_setp<true>")
    _same(_host_rows(ctx, got["pinned"][:4, :nb]), np.array([D.host_sum_row(row, nb) for row in r["partials"]]), "host_sum_row of the split's rows")

    v = dict(x=x, g=g, p=p, Ap=Ap)
    for setp, nb_p1 in ((0, 0), (1, 0), (1, nb), (0, nb)):
        acg = D.step_acg(acg_host=0.41, partials=seeded, nb_p1=nb_p1)
        r = D.step_update(acg, x, g, p, Ap, lb, ub, D.ASTOL, setp, True)
        compare(launch(ctx, STEP, n, v, partials=seeded, emit=1, setp=setp, nb=nb_p1, acg_host=0.41, astol=D.ASTOL, **bd),
                expect(n, v, {k: r[k] for k in ("x", "g", "gf", "p")}, r["partials"], emit=True, partials=seeded), "k_step_update<%d, false, true>, %d P1 blocks" % (setp, nb_p1))
    # ... and finalised on the device after all (finalize_vec4_from)
    r = D.step_update(0.41, x, g, p, Ap, lb, ub, D.ASTOL, 0, True)
    compare(launch(ctx, STEP, n, v, emit=1, acg_host=0.41, finalize=1, astol=D.ASTOL, **bd),
            expect(n, v, {k: r[k] for k in ("x", "g", "gf", "p")}, r["partials"], emit=True, scal_written=_slots(D.S_APGF, D.finalize(r["partials"], [D.SUM] * 4))),
            "k_step_update<false, false, true> + k_finalize")

    v = dict(gf=gf, p=p)
    compare(launch(ctx, DIR, n, v, partials=seeded, emit=1, nb=nb, pAp_host=1.7),
            expect(n, v, dict(p=D.dir_update(D.sum_block_partials(seeded[0], nb) / 1.7, gf, p)), partials=seeded), "k_dir_update<true>")
    v = dict(x=x, g=g)
    compare(launch(ctx, PROP_DIR, n, v, emit=1, astol=D.ASTOL, **bd), expect(n, v, dict(p=D.prop_dir(x, g, lb, ub, D.ASTOL))), "k_prop_dir<true>")
    v = dict(x=x, g=g, p=p, Ap=Ap)
    compare(launch(ctx, EXPANSION, n, v, emit=1, afeas=0.3, alpha=0.7, astol=D.ASTOL, **bd),
            expect(n, v, dict(x=D.expansion_std(0.3, 0.7, x, g, p, Ap, lb, ub, D.ASTOL))), "k_expansion_std<true>")


# ---- the device-side verdict ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(D.spec_cases()))
def test_spec_verdict(ctx, name):
    """k_step_update<false, true>, the finalising launch and k_dir_update under the chain's control words.  A halt leaves x, g, p, gf, the partials, the scalars and
    the ring as they were, sets the halt word and bumps no counter -- and so do the two launches that follow it.  The go case takes the step of the host-scalar
    variant bit for bit, writes ring slot iteration - base and bumps both counters."""
    ctl, scal, const, go = D.spec_cases()[name]
    n = 4099
    c = D.phase_case(n, "both")
    x, g, p, Ap, gf, lb, ub = (c[k] for k in ("x", "g", "p", "Ap", "gf", "lb", "ub"))
    v = dict(x=x, g=g, p=p, Ap=Ap, gf=gf)
    kw = dict(lb=lb, ub=ub, astol=D.ASTOL, scal=scal, ctl=ctl, use_ctl=1)
    got = launch(ctx, STEP, n, v, spec=1, finalize=1, **kw, **const)
    assert D.spec_go(ctl, scal, D.step_acg(scal=scal), **const) is go
    if not go:
        halted = [1] + list(ctl[1:])
        compare(got, expect(n, v, scal=scal, ctl=halted), "halted step + k_finalize")
        compare(launch(ctx, DIR, n, v, scal=scal, ctl=halted, use_ctl=1), expect(n, v, scal=scal, ctl=halted), "k_dir_update under the halt word")
        compare(launch(ctx, SPLIT, n, v, finalize=1, **dict(kw, ctl=halted)),
                expect(n, v, dict(gf=D.split_setp(x, g, lb, ub, D.ASTOL)["gf"], p=D.split_setp(x, g, lb, ub, D.ASTOL)["p"]), D.split_setp(x, g, lb, ub, D.ASTOL)["partials"], scal=scal, ctl=halted),
                "k_finalize under the halt word: fresh partials, no scalar and no counter written")
        return
    r = D.step_update(D.step_acg(scal=scal), x, g, p, Ap, lb, ub, D.ASTOL, False)
    ring = np.full(48, SENT)
    k = ctl[D.ITER] - ctl[D.BASE]
    ring[3 * k:3 * k + 3] = scal[D.S_GP2], scal[D.S_GF2], scal[D.S_GC2]
    after = [0, ctl[1] + 1, ctl[2] + 1, ctl[3]]
    fin = _slots(D.S_APGF, D.finalize(r["partials"], [D.SUM] * 4))
    compare(got, expect(n, v, {k: r[k] for k in ("x", "g", "gf", "p")}, r["partials"], scal=scal, scal_written=fin, ctl=after, ring=ring), "go: step + k_finalize")
    host = launch(ctx, STEP, n, v, lb=lb, ub=ub, astol=D.ASTOL, scal=scal, finalize=1)
    for key in VECS + ("partials", "scal", "scal_pinned"):
        _same(got[key], host[key], ("the speculative step against the host-scalar step", key))
    s2 = np.array(got["scal"])
    compare(launch(ctx, DIR, n, dict(gf=got["gf"], p=got["p"]), scal=s2, ctl=after, use_ctl=1),
            expect(n, dict(gf=got["gf"], p=got["p"]), dict(p=D.dir_update(s2[D.S_APGF] / s2[D.S_PAP], got["gf"], got["p"])), scal=s2, ctl=after), "k_dir_update under a clear halt word")


# ---- the finishers -----------------------------------------------------------------------------------------------------------------------------------------------------------
def _finalize(ctx, rows, ops, slots, halt=-1, post=None):
    K, nb = rows.shape
    sd, sp = np.full(K, SENT_SCAL), np.full(K, SENT_PINNED)
    pi = None if post is None else (C.c_int * 2)(*post)
    check(ctx.L.pmh_vec_test_finalize(ctx.h, K, nb, _ptr(np.ascontiguousarray(rows)), _ptr(np.array(ops, np.int32)), _ptr(np.array(slots, np.int32)), halt, pi, _ptr(sd), _ptr(sp)))
    return sd, sp, None if post is None else list(pi)


@pytest.mark.parametrize("nb", (0, 1, 2, 3, 64, 65, 1023, 1024, 1025, 2047, 2048))
def test_k_finalize_equals_the_restatement(ctx, nb):
    """8 quantities, SUM and MIN mixed, into scattered slots; the halt word and the counters; 7 quantities in one launch against the 4 + 3 they replace."""
    rows = D.reduction_rows(nb, 21)
    ops = [D.SUM, D.MIN, D.SUM, D.SUM, D.MIN, D.SUM, D.MIN, D.SUM]
    slots = [40, 3, 63, 0, 17, 8, 25, 31]
    exp = D.finalize(rows, ops)
    for halt, post in ((-1, None), (0, [5, 9]), (-1, [0, 0])):
        sd, sp, cnt = _finalize(ctx, rows, ops, slots, halt, post)
        _same(sd, exp, ("k_finalize, device slots", halt))
        _same(sp, exp, ("k_finalize, pinned mirror", halt))
        assert cnt == (None if post is None else [post[0] + 1, post[1] + 1])
    sd, sp, cnt = _finalize(ctx, rows, ops, slots, 1, [5, 9])
    _same(sd, np.full(8, SENT_SCAL), "halted k_finalize, device slots")
    _same(sp, np.full(8, SENT_PINNED), "halted k_finalize, pinned mirror")
    assert cnt == [5, 9]
    for K in range(1, 8):  # fewer quantities: the rows past K are not read, the slots past K not written
        sd, sp, _ = _finalize(ctx, rows[:K], ops[:K], slots[:K])
        _same(sd, exp[:K], ("k_finalize", K))
    ops7, slots7 = [D.SUM] * 6 + [D.MIN], [D.S_APGF, D.S_GP2, D.S_GC2, D.S_GF2, D.S_PAP, D.S_GP, D.S_FEAS]
    seven = _finalize(ctx, rows[:7], ops7, slots7)[0]
    four, three = _finalize(ctx, rows[:4], ops7[:4], slots7[:4])[0], _finalize(ctx, rows[4:7], ops7[4:], slots7[4:])[0]
    _same(seven, np.concatenate([four, three]), "7 quantities in one launch against 4 + 3")
    _same(seven, D.finalize(rows[:7], ops7), "7 quantities")


@pytest.mark.parametrize("nb", (0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 300, 511, 512))
def test_row_sums_equal_the_restatement(ctx, nb):
    """pmh_sum_block_partials in every lane, host_sum_row (SUM and MIN), and k_finalize on the same row: the first two are one order, k_finalize is another --
    the same bits up to two blocks, and from three blocks on exactly what its own restatement says (tests/test_dual_reference_host.py shows that the two orders
    differ on this very data)."""
    rows = D.reduction_rows(nb, 6) if nb else np.zeros((8, 0))
    lanes = np.full(64, SENT)
    for k in (0, 3):
        row = np.ascontiguousarray(rows[k])
        check(ctx.L.pmh_mpgp_test_block_sum(ctx.h, nb, _ptr(row), _ptr(lanes)))
        _same(lanes, np.full(64, D.sum_block_partials(row, nb)), ("pmh_sum_block_partials", k))
        _same(_host_rows(ctx, [row]), np.array([D.host_sum_row(row, nb)]), ("host_sum_row", k))
        _same(_host_rows(ctx, [row], D.MIN), np.array([D.host_sum_row(row, nb, D.MIN)]), ("host_sum_row, MIN", k))
        _same(_host_rows(ctx, [row]), lanes[:1], "host_sum_row against pmh_sum_block_partials")
        fin = _finalize(ctx, row[None, :], [D.SUM], [5])[0]
        _same(fin, D.finalize(row[None, :], [D.SUM]), "k_finalize on the same row")
        if nb <= 2:
            _same(fin, lanes[:1], "k_finalize against host_sum_row: one addition at the most")
        _same(_finalize(ctx, row[None, :], [D.MIN], [5])[0], _host_rows(ctx, [row], D.MIN), "MIN: exact in any order")


@pytest.mark.parametrize("n", (1, 1500, 64 * 1024 + 1))
def test_block_partials_equal_the_restatement(ctx, n):
    """pmh_block_partials<3> with SUM, SUM and MIN (the P1 form of the chain's last kernel): device rows and pinned rows."""
    rng = np.random.default_rng(n)
    a, b, c = D.reduction_rows(n, 31)[:3]
    c = np.abs(c)
    c[rng.random(n) < 0.5] = np.inf
    nb = D.emit_blocks(n)
    pad = lambda v, fill: np.concatenate([v, np.full(nb * D.TILE - n, fill)]).reshape(nb, D.TILE)  # noqa: E731
    exp = np.stack([D.block_partials(0.0 + pad(a, 0.0)), D.block_partials(0.0 + pad(b, 0.0)), D.block_partials(pad(c, np.inf), D.MIN)])
    dev, pinned = np.full((3, nb), SENT), np.full((3, nb), SENT_PINNED)
    va, vb, vc = (ctx.vec_from(v) for v in (a, b, c))
    check(ctx.L.pmh_mpgp_test_block_partials(ctx.h, n, va.p, vb.p, vc.p, _ptr(dev), _ptr(pinned)))
    for v in (va, vb, vc):
        v.free()
    _same(dev, exp, "pmh_block_partials, device rows")
    _same(pinned, exp, "pmh_block_partials, pinned rows")


# ---- a whole solve ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vec_epi", (1, 0))
def test_fused_solve_on_a_shell_operator_equals_the_restated_solve(ctx, vec_epi):
    """solve_fused on an operator that refuses mult_epi (k_split_setp, k_p1_dots, the host-scalar steps, k_dir_update, k_prop_dir, k_expansion_std and a finalising
    launch behind each reduction): the step string, every monitor norm and the final x equal the phases of tests/dual_cases.py chained in numpy.  The shell's product
    is the ELL product of a tridiagonal matrix: every row left to right."""
    sc = D.solve_case("shell")
    M, n = sc["A"], sc["n"]
    steps, mon, x_ref, reason = D.solve_fused(D.ShellModel(lambda v: D._rows_left_to_right(M, M["val"] * v[M["col"]])), sc["b"], sc["x0"], sc["lb"], sc["ub"], 0.45)
    assert {"c", "e", "p"} <= set(steps) and reason == 2 and len(steps) <= 61
    A = pa.CsrMat(ctx, n, n, M["rowptr"], M["col"], M["val"])
    assert A.kernel_info()[0][0] == 0  # the ELL product
    op = pa.Op.shell(ctx, n, lambda xp, yp: check(ctx.L.pmh_csr_mult(A.h, xp, yp)))
    was = C.c_int()
    check(ctx.L.pmh_get_knob(b"vec_epi", C.byref(was)))
    check(ctx.L.pmh_set_knob(b"vec_epi", vec_epi))
    try:
        qp, x = pa.QP(ctx), ctx.vec_from(sc["x0"])
        qp.SetOperator(op), qp.SetRhs(ctx.vec_from(sc["b"])), qp.SetInitialVector(x), qp.SetBox(None, ctx.vec_from(sc["lb"]), ctx.vec_from(sc["ub"]))
        qps = pa.QPS(ctx)
        qps.SetQP(qp), qps.SetType("mpgp"), qps.MPGPSetAlpha(0.45, direct=True), qps.MonitorSet(), qps.SetTolerances(max_it=60)
        st = qps.Solve()
        got_steps, gp, gf, gc, _ = qps.MPGPGetTrace()
    finally:
        check(ctx.L.pmh_set_knob(b"vec_epi", was.value))
    assert (got_steps, st.reason, st.iteration) == (steps, reason, len(steps) - 1)
    _same(gp, mon[:, 0], "monitor |gP|")
    _same(gf, mon[:, 1], "monitor |gf|")
    _same(gc, mon[:, 2], "monitor |gc|")
    _same(x.to_numpy(), x_ref, "x")
    qps.Destroy(), op.destroy(), A.destroy()


@pytest.mark.parametrize("spec", (1, 0))
def test_fused_solve_on_a_csr_operator_equals_the_restated_solve(ctx, spec):
    """solve_fused on a CSR operator (the SUB and MPGP epilogues of the ELL product, tests/test_gpu_spmv_paths.py), with the speculative device-side CG chain
    (k_step_update<false, true>, the finalising launch and k_dir_update under the control words, monitor norms from the ring) and without it: the same steps, norms
    and x as the restated solve, bit for bit, both ways."""
    sc = D.solve_case("shell")
    M, n = sc["A"], sc["n"]
    A = pa.CsrMat(ctx, n, n, M["rowptr"], M["col"], M["val"])
    info = A.kernel_info()[0]
    assert info[0] == 0 and info[4] == -(-n // 256)  # ELL, blocks of 256 rows
    steps, mon, x_ref, reason = D.solve_fused(D.CsrModel(M, info[5], info[4]), sc["b"], sc["x0"], sc["lb"], sc["ub"], 0.45)
    assert {"c", "e", "p"} <= set(steps) and "cc" in steps and reason == 2 and len(steps) <= 61
    op = pa.Op.from_csr(A)
    was = C.c_int()
    check(ctx.L.pmh_get_knob(b"mpgp_spec", C.byref(was)))
    check(ctx.L.pmh_set_knob(b"mpgp_spec", spec))
    try:
        qp, x = pa.QP(ctx), ctx.vec_from(sc["x0"])
        qp.SetOperator(op), qp.SetRhs(ctx.vec_from(sc["b"])), qp.SetInitialVector(x), qp.SetBox(None, ctx.vec_from(sc["lb"]), ctx.vec_from(sc["ub"]))
        qps = pa.QPS(ctx)
        qps.SetQP(qp), qps.SetType("mpgp"), qps.MPGPSetAlpha(0.45, direct=True), qps.MonitorSet(), qps.SetTolerances(max_it=60)
        st = qps.Solve()
        got_steps, gp, gf, gc, _ = qps.MPGPGetTrace()
        words = (C.c_int * 5)()
        check(ctx.L.pmh_mpgp_test_spec_words(qps.h, words))
    finally:
        check(ctx.L.pmh_set_knob(b"mpgp_spec", was.value))
    # the case reached the path it is named after: the solver sets the device-side chain up only where it may use it, and a batch that ran leaves its words behind --
    # no halt word but 0 / 1, the device's count of CG steps = its iterations, all inside the solve.  Without the knob nothing is set up.
    if spec:
        halt, it, ncg, base = list(words)[1:]
        assert words[0] == 1 and halt in (0, 1) and 1 <= base <= it <= st.iteration and ncg == it - base, list(words)
    else:
        assert words[0] == 0, list(words)
    assert (got_steps, st.reason, st.iteration) == (steps, reason, len(steps) - 1)
    _same(gp, mon[:, 0], "monitor |gP|")
    _same(gf, mon[:, 1], "monitor |gf|")
    _same(gc, mon[:, 2], "monitor |gc|")
    _same(x.to_numpy(), x_ref, "x")
    qps.Destroy(), op.destroy(), A.destroy()


@pytest.mark.parametrize("kind", ("shell", "csr"))
def test_fused_solve_from_a_carried_gradient_equals_the_restated_solve(ctx, kind):
    """The g_valid branch of solve_fused on a plain operator (pmh_mpgp_set_gradient_valid, as SMALXE hands a gradient over): no first product, k_split_setp<false> and
    the finalising launch on the vector handed over -- which is NOT the gradient at the starting point here, so a driver that formed its own would take other steps.
    A first solve of the same handle runs before, as in SMALXE."""
    sc = D.solve_case("shell")
    M, n = sc["A"], sc["n"]
    mult = lambda v: D._rows_left_to_right(M, M["val"] * v[M["col"]])  # noqa: E731
    A = pa.CsrMat(ctx, n, n, M["rowptr"], M["col"], M["val"])
    info = A.kernel_info()[0]
    model = D.ShellModel(mult) if kind == "shell" else D.CsrModel(M, info[5], info[4])
    op = pa.Op.shell(ctx, n, lambda xp, yp: check(ctx.L.pmh_csr_mult(A.h, xp, yp))) if kind == "shell" else pa.Op.from_csr(A)
    g0 = D.carried_gradient(sc, mult(sc["x0"]) - sc["b"])
    first = D.solve_fused(model, sc["b"], sc["x0"], sc["lb"], sc["ub"], 0.45)
    steps, mon, x_ref, reason = D.solve_fused(model, sc["b"], sc["x0"], sc["lb"], sc["ub"], 0.45, g0=g0)
    assert {"c", "e", "p"} <= set(steps) and len(steps) <= 62 and not np.array_equal(mon[0], first[1][0])
    qp, x = pa.QP(ctx), ctx.vec_from(sc["x0"])
    qp.SetOperator(op), qp.SetRhs(ctx.vec_from(sc["b"])), qp.SetInitialVector(x), qp.SetBox(None, ctx.vec_from(sc["lb"]), ctx.vec_from(sc["ub"]))
    qps = pa.QPS(ctx)
    qps.SetQP(qp), qps.SetType("mpgp"), qps.MPGPSetAlpha(0.45, direct=True), qps.MonitorSet(), qps.SetTolerances(max_it=60)
    qps.Solve()
    assert qps.MPGPGetTrace()[0] == first[0]
    x.set_numpy(sc["x0"])
    gd = ctx.vec_from(g0)
    check(ctx.L.pmh_mpgp_test_set_gradient_valid(qps.h, gd.p))
    st = qps.Solve()
    got_steps, gp, gf, gc, _ = qps.MPGPGetTrace()
    assert (got_steps, st.reason, st.iteration) == (steps, reason, len(steps) - 1)
    _same(gp, mon[:, 0], "monitor |gP|")
    _same(gf, mon[:, 1], "monitor |gf|")
    _same(gc, mon[:, 2], "monitor |gc|")
    _same(x.to_numpy(), x_ref, "x")
    # the word is spent: the next solve forms its own gradient again
    x.set_numpy(sc["x0"])
    qps.Solve()
    assert qps.MPGPGetTrace()[0] == first[0]
    qps.Destroy(), op.destroy(), A.destroy()
