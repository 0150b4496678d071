"""CPU checks of tests/dual_cases.py, the numpy restatement tests/test_gpu_mpgp_phases.py compares the device with bit for bit.  Three questions, no GPU:
is every restated sum a sum of the right numbers (dyadic data, exact in any order: the restatement must equal the plain float64 result bit for bit, which pins
its index work -- a lane visited twice or never shows at once); is it the right mathematics on real data (a long-double evaluation of the same formula, within
the a-priori bound gamma_k sum |a_j b_j| with k the number of roundings on the longest path of that stage, derived below and never tuned); and does every case
generator produce the grid, the laps and the box arms its name claims, so that a device test that silently ran the common path fails here as well."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import dual_cases as D

LD = np.longdouble
U = 2.0 ** -53
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gamma(k):
    return k * U / (1 - k * U)


def _dyadic(rng, shape):
    return rng.integers(-512, 513, shape).astype(np.float64) / 64.0  # sums of < 2^20 of these (and of their pairwise products) are exact in float64


def _close(got, ref_ld, k, mag_ld, what):
    """|got - ref| <= gamma_k * mag, mag = the sum of the absolute values of the terms, both evaluated in long double."""
    err = np.max(np.abs(np.asarray(got, LD) - ref_ld))
    bound = np.max(gamma(k) * mag_ld)
    assert err <= bound, (what, float(err), float(bound))


# ---- the reductions ------------------------------------------------------------------------------------------------------------------------------------------------------
# roundings on the longest path: wave trees 6 (five exchanges inside the rows + the rows' two levels: 4 + 2; the shuffle tree: 6), waves in order 3 (4 waves) or 15 (16 waves),
# a lane's 8 strided entries 8 (the first is added to 0.0: exact, counted anyway), k_finalize's laps ceil(nblocks / 1024)
K_WAVE, K_BLOCK, K_TILE, K_ROW = 6, 6 + 3, 6 + 15, 8 + 6


def k_fin(nblocks):
    return -(-nblocks // 1024) + 6 + 15


def test_reductions_sum_every_entry_once():
    rng = np.random.default_rng(1)
    for op, exact in ((D.SUM, np.sum), (D.MIN, np.min)):
        v = _dyadic(rng, (5, 64))
        assert np.array_equal(D.wave_reduce(v, op), exact(v, axis=-1)) and np.array_equal(D.wave_all(v, op), exact(v, axis=-1))
        v = _dyadic(rng, (3, D.BLOCK))
        assert np.array_equal(D.block_reduce(v, op), exact(v, axis=-1))
        v = _dyadic(rng, (3, D.TILE))
        assert np.array_equal(D.block_partials(v, op), exact(v, axis=-1))
        for nb in (1, 2, 63, 64, 65, 127, 128, 129, 511, 512):
            row = _dyadic(rng, nb)
            assert D.host_sum_row(row, nb, op) == exact(row), (op, nb)
        for nb in (1, 1023, 1024, 1025, 2047, 2048):
            rows = _dyadic(rng, (2, nb))
            assert np.array_equal(D.finalize(rows, [op, op]), exact(rows, axis=-1)), (op, nb)
    for nb in (1, 64, 65, 512):
        row = _dyadic(rng, nb)
        assert D.sum_block_partials(row, nb) == np.sum(row)
    # empty rows: the identities
    assert D.host_sum_row(np.zeros(0), 0, D.SUM) == 0.0 and D.host_sum_row(np.zeros(0), 0, D.MIN) == np.inf and D.sum_block_partials(np.zeros(0), 0) == 0.0
    assert np.array_equal(D.finalize(np.zeros((2, 0)), [D.SUM, D.MIN]), [0.0, np.inf])


def test_reductions_against_long_double():
    rng = np.random.default_rng(2)
    v = D.reduction_rows(64, 1)
    _close(D.wave_reduce(v), v.astype(LD).sum(-1), K_WAVE, np.abs(v).astype(LD).sum(-1), "pmh_wave_sum")
    _close(D.wave_all(v), v.astype(LD).sum(-1), K_WAVE, np.abs(v).astype(LD).sum(-1), "pmh_wave_all")
    v = D.reduction_rows(D.BLOCK, 2)
    _close(D.block_reduce(v), v.astype(LD).sum(-1), K_BLOCK, np.abs(v).astype(LD).sum(-1), "pmh_block_reduce")
    v = D.reduction_rows(D.TILE, 3)
    _close(D.block_partials(v), v.astype(LD).sum(-1), K_TILE, np.abs(v).astype(LD).sum(-1), "pmh_block_partials")
    for nb in (3, 64, 65, 300, 512):
        row = D.reduction_rows(nb, 4)[0]
        _close(D.sum_block_partials(row, nb), row.astype(LD).sum(), K_ROW, np.abs(row).astype(LD).sum(), ("pmh_sum_block_partials", nb))
    for nb in (3, 1024, 1025, 2048):
        rows = D.reduction_rows(nb, 5)
        _close(D.finalize(rows, [D.SUM] * 8), rows.astype(LD).sum(-1), k_fin(nb), np.abs(rows).astype(LD).sum(-1), ("k_finalize", nb))
    assert rng is not None


def test_host_row_sum_and_device_row_sum_are_one_order():
    """host_sum_row and pmh_sum_block_partials: the same bits for every row length of the contract, 0..512.  A row of 513 blocks is out of contract (a lane holds
    8 entries: both would drop entry 512); nothing is asserted about it, and the restatement refuses it."""
    for nb in range(513):
        row = D.reduction_rows(nb, 6)[3] if nb else np.zeros(0)
        a, b = D.host_sum_row(row, nb, D.SUM), D.sum_block_partials(row, nb)
        assert a == b, nb
    with pytest.raises(AssertionError, match="out of contract"):
        D.host_sum_row(np.zeros(513), 513, D.SUM)


def test_k_finalize_and_host_row_sum_are_two_orders():
    """k_finalize (block t in thread t, shuffle tree, waves in order) and host_sum_row (block l + 64 u in lane l, butterflies) add in different orders: one or two
    blocks give the same bits by commutativity, from three blocks on ((a + c) + b against (a + b) + c) they need not -- and on this data they do not, at every
    length the device test uses, so that test tells the two apart.  MIN is exact in any order."""
    for nb in (1, 2):
        rows = D.reduction_rows(nb, 7)
        assert all(D.finalize(rows, [D.SUM] * 8)[k] == D.host_sum_row(rows[k], nb) for k in range(8))
    for nb in (3, 64, 65, 512):
        rows = D.reduction_rows(nb, 7)
        fin = D.finalize(rows, [D.SUM] * 8)
        assert any(fin[k] != D.host_sum_row(rows[k], nb) for k in range(8)), nb
        assert all(D.finalize(rows, [D.MIN] * 8)[k] == D.host_sum_row(rows[k], nb, D.MIN) == rows[k].min() for k in range(8))


def test_seven_quantities_are_reduced_as_four_and_three():
    rows = D.reduction_rows(1500, 8)[:7]
    ops = [D.SUM] * 6 + [D.MIN]
    assert np.array_equal(D.finalize(rows, ops), np.concatenate([D.finalize(rows[:4], ops[:4]), D.finalize(rows[4:], ops[4:])]))


# ---- the grids -----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_cases_reach_the_grids_they_are_named_after():
    assert [D.vec_grid(n) for n in D.PLAIN_N] == [1, 1, 1, 2, 17, 1026, 2048]
    assert D.vec_grid(262144 + 300) > D.FIN_THREADS  # k_finalize: threads 0 and 1 take a second block
    assert 524288 + 300 - 2048 * D.BLOCK == 300  # the first 300 threads of the capped grid take a second entry
    assert [D.emit_blocks(n) for n in D.EMIT_N] == [2, 64, 65, 512]
    for n in (1, 255, 257, 4099, 1500):
        for emit in (False, True):
            t = _dyadic(np.random.default_rng(n), n)
            assert D.grid_partials(t, emit).sum() == t.sum() and len(D.grid_partials(t, emit)) == D.nblocks_of(n, emit)
    # the second grid-stride lap and the tiles, entry by entry: block b of the plain grid owns entries 256 b + t and 256 (2048 + b) + t
    n = 524288 + 300
    t = _dyadic(np.random.default_rng(5), n)
    got = D.grid_partials(t, False)
    pad = np.zeros(2 * 2048 * 256)
    pad[:n] = t
    assert np.array_equal(got, pad.reshape(2, 2048, 256).sum(axis=(0, 2)))
    got = D.grid_partials(t[:65 * 1024 - 3], True)
    pad = np.zeros(65 * 1024)
    pad[:65 * 1024 - 3] = t[:65 * 1024 - 3]
    assert np.array_equal(got, pad.reshape(65, 1024).sum(-1))
    # MIN skips the entries it does not have
    q = np.abs(t[:4099]) + 1.0
    have = np.arange(4099) % 3 == 0
    assert D.grid_partials(q, False, D.MIN, have).min() == q[have].min() and D.grid_partials(q, False, D.MIN, np.zeros(4099, bool)).min() == np.inf


@pytest.mark.parametrize("bounds", D.BOUNDS)
def test_cases_reach_every_arm_of_the_box_predicates(bounds):
    for n in (255, 4099):
        c = D.phase_case(n, bounds)
        arms = set(D.box_arms(c["x"], c["g"], c["lb"], c["ub"], D.ASTOL).tolist())
        want = {0} | ({1, 2} if c["lb"] is not None else set()) | ({3, 4} if c["ub"] is not None else set())
        assert arms == want, (n, bounds, arms)
        k = np.arange(n) % 37
        f, g = D.box_split(c["x"], c["g"], c["lb"], c["ub"], D.ASTOL)
        if c["lb"] is not None:
            assert np.all(f[k == 1] == 0.0) and np.all(f[k == 2] == c["g"][k == 2])  # within astol; one ulp outside
            assert np.all(g[k == 6] == c["g"][k == 6]) and np.all(c["g"][k == 6] < 0)  # lb == ub: the lower bound's arm (the upper one would give 0)
            assert np.any(np.isinf(c["lb"]))
        if c["ub"] is not None:
            assert np.all(f[k == 4] == 0.0) and np.all(f[k == 5] == c["g"][k == 5])
            assert np.any(np.isinf(c["ub"]))
        if bounds == "ub":
            assert np.all(g[k == 6] == 0.0)  # without lb the same entries take the upper arm with g < 0
        # the reduced gradient: both clipped and unclipped, on both sides, after an expansion's first half
        xi = c["x"] + (-0.3) * c["p"]
        fi, _ = D.box_split(xi, c["g"] + (-0.3) * c["Ap"], c["lb"], c["ub"], D.ASTOL)
        r = D.box_reduced(xi, fi, c["lb"], c["ub"], 0.7)
        if c["lb"] is not None:
            assert np.any((fi > 0) & (r != fi)) and np.any((fi > 0) & (r == fi))
        if c["ub"] is not None:
            assert np.any((fi < 0) & (r != fi)) and np.any((fi < 0) & (r == fi))
        # the feasible step: entries that bound it from either side, entries without a bound, p = 0
        assert np.any(c["p"] == 0) and np.any(c["p"] > 0) and np.any(c["p"] < 0)


# ---- the phases against long double --------------------------------------------------------------------------------------------------------------------------------------
def _sum_path(n, emit):
    """Roundings on the longest path from a product to a finished scalar: the product, a thread's laps, the workgroup, then k_finalize (plain grid) or a row sum
    (tiles)."""
    nb = D.nblocks_of(n, emit)
    return 1 + (1 + K_TILE + K_ROW if emit else -(-n // (nb * D.BLOCK)) + K_BLOCK + k_fin(nb))


@pytest.mark.parametrize("emit", (False, True))
@pytest.mark.parametrize("bounds", D.BOUNDS)
def test_phases_against_long_double(bounds, emit):
    n = 4099
    c = D.phase_case(n, bounds)
    x, g, p, Ap, lb, ub = (c[k] for k in ("x", "g", "p", "Ap", "lb", "ub"))
    fin = (lambda rows: np.array([D.host_sum_row(r, len(r)) for r in rows])) if emit else (lambda rows: D.finalize(rows, [D.SUM] * len(rows)))
    k = _sum_path(n, emit)
    # gradient split: the selections are exact; the norms
    s = D.split_setp(x, g, lb, ub, D.ASTOL, emit)
    arms = D.box_arms(x, g, lb, ub, D.ASTOL)
    fL = np.where(arms == 0, g, 0.0).astype(LD)
    cL = np.where((arms == 1) | (arms == 3), g, 0.0).astype(LD)
    assert np.array_equal(s["gf"], fL.astype(np.float64)) and np.array_equal(s["p"], s["gf"])
    got = fin(s["partials"])
    assert got[0] == 0.0
    for j, ref in ((1, ((fL + cL) ** 2).sum()), (2, (cL ** 2).sum()), (3, (fL ** 2).sum())):
        _close(got[j], ref, k, ref, ("split", j))
    # step: x - acg p and g - acg Ap carry two roundings; edge entries have p = 0 and stay on their bounds, the others are 0.1 or more inside: the same arms
    acg = 0.37
    for setp in (False, True):
        st = D.step_update(acg, x, g, p, Ap, lb, ub, D.ASTOL, setp, emit)
        xL, gL = x.astype(LD) - LD(acg) * p.astype(LD), g.astype(LD) - LD(acg) * Ap.astype(LD)
        assert np.all(np.abs(st["x"].astype(LD) - xL) <= gamma(2) * (np.abs(x) + np.abs(acg * p)))
        assert np.all(np.abs(st["g"].astype(LD) - gL) <= gamma(2) * (np.abs(g) + np.abs(acg * Ap)))
        a2 = D.box_arms(st["x"], st["g"], lb, ub, D.ASTOL)
        assert np.array_equal(a2 != 0, D.box_arms(xL.astype(np.float64), gL.astype(np.float64), lb, ub, D.ASTOL) != 0)
        assert np.array_equal(st["gf"], np.where(a2 == 0, st["g"], 0.0)) and np.array_equal(st["p"], st["gf"] if setp else p)
        got = fin(st["partials"])
        f2 = st["gf"].astype(LD)
        _close(got[0], (Ap.astype(LD) * f2).sum(), k, np.abs(Ap.astype(LD) * f2).sum(), "Ap'gf")
        _close(got[3], (f2 ** 2).sum(), k, (f2 ** 2).sum(), "|gf|^2")
    # direction, proportioning direction, expansion
    assert np.all(np.abs(D.dir_update(0.61, s["gf"], p).astype(LD) - (s["gf"].astype(LD) - LD(0.61) * p.astype(LD))) <= gamma(2) * (np.abs(s["gf"]) + np.abs(0.61 * p)))
    assert np.array_equal(D.prop_dir(x, g, lb, ub, D.ASTOL), cL.astype(np.float64))
    afeas, alpha = 0.3, 0.7
    xe = D.expansion_std(afeas, alpha, x, g, p, Ap, lb, ub, D.ASTOL)
    xi = x + (-afeas) * p
    fi, _ = D.box_split(xi, g + (-afeas) * Ap, lb, ub, D.ASTOL)
    rL = fi.astype(LD)
    with np.errstate(invalid="ignore"):
        if lb is not None:
            rL = np.where(fi > 0, np.minimum(rL, (xi.astype(LD) - lb.astype(LD)) / LD(alpha)), rL)
        if ub is not None:
            rL = np.where(fi < 0, np.maximum(rL, (xi.astype(LD) - ub.astype(LD)) / LD(alpha)), rL)
    ref = xi.astype(LD) - LD(alpha) * rL
    # (x - bound) / alpha: two roundings; times alpha and the subtraction: two more, all on numbers no larger than |xi| + |alpha r|
    assert np.all(np.abs(xe.astype(LD) - ref) <= gamma(4) * (np.abs(xi) + 2 * np.abs(alpha * rL))), "expansion"
    if emit:
        return
    # the three P1 scalars of k_p1_dots; the minimum is exact in any order, each quotient carries two roundings
    rows = D.p1_dots(p, Ap, g, x, lb, ub)
    got = D.finalize(rows, [D.SUM, D.SUM, D.MIN])
    _close(got[0], (p.astype(LD) * Ap.astype(LD)).sum(), k, np.abs(p * Ap).astype(LD).sum(), "p'Ap")
    _close(got[1], (g.astype(LD) * p.astype(LD)).sum(), k, np.abs(g * p).astype(LD).sum(), "g'p")
    q = np.full(n, np.inf, LD)
    if lb is not None:
        m = (p > 0) & np.isfinite(lb)
        q[m] = (x[m].astype(LD) - lb[m].astype(LD)) / p[m].astype(LD)
    if ub is not None:
        m = (p < 0) & np.isfinite(ub)
        q[m] = (x[m].astype(LD) - ub[m].astype(LD)) / p[m].astype(LD)
    if np.isfinite(q.min()):
        assert abs(LD(got[2]) - q.min()) <= gamma(2) * q.min() and got[2] > 0
    else:
        assert got[2] == np.inf
    n3 = D.finalize(D.three_norms(x, g, p), [D.SUM] * 4)
    _close(n3[1:], np.array([(v.astype(LD) ** 2).sum() for v in (x, g, p)]), k, np.array([(v.astype(LD) ** 2).sum() for v in (x, g, p)]), "three norms")
    o = D.finalize(D.obj_from_grad(x, g, c["b"]), [D.SUM])[0]
    _close(o, (x.astype(LD) * (g.astype(LD) - c["b"].astype(LD))).sum(), k + 1, (np.abs(x) * (np.abs(g) + np.abs(c["b"]))).astype(LD).sum(), "objective")


def test_phase_sums_count_every_entry_once():
    """Dyadic vectors: every restated phase sum equals the plain float64 dot product bit for bit, on both entry maps and at the sizes with a second lap."""
    for n, emit in ((4099, False), (524288 + 300, False), (1500, True), (64 * 1024 + 1, True)):
        rng = np.random.default_rng(n)
        x, g, p, Ap, b = (_dyadic(rng, n) for _ in range(5))
        fin = (lambda rows: np.array([D.host_sum_row(r, len(r)) for r in rows])) if emit else (lambda rows: D.finalize(rows, [D.SUM] * len(rows)))
        s = fin(D.split_setp(x, g, None, None, D.ASTOL, emit)["partials"])
        assert list(s) == [0.0, g @ g, 0.0, g @ g]
        st = D.step_update(0.5, x, g, p, Ap, None, None, D.ASTOL, False, emit)
        assert np.array_equal(st["g"], g - 0.5 * Ap) and list(fin(st["partials"])) == [Ap @ st["g"], st["g"] @ st["g"], 0.0, st["g"] @ st["g"]]
        if not emit:
            lb = x - 1.0
            assert list(D.finalize(D.p1_dots(p, Ap, g, x, lb, None), [D.SUM, D.SUM, D.MIN])) == [p @ Ap, g @ p, np.min(1.0 / p[p > 0])]
            assert list(D.finalize(D.three_norms(x, g, p), [D.SUM] * 4)) == [0.0, x @ x, g @ g, p @ p]
            assert D.finalize(D.obj_from_grad(x, g, b), [D.SUM])[0] == x @ (g - b)


def test_spec_verdict_table():
    """One reason to halt at a time, and the go case (tests/test_gpu_mpgp_phases.py runs the same table on the device)."""
    for name, (ctl, scal, kw, go) in D.spec_cases().items():
        acg = D.step_acg(scal=scal)
        assert D.spec_go(ctl, scal, acg, **kw) is go, name


def test_phase_struct_layout_matches_header():
    from permon_amd import _lib

    src = '#include <stdio.h>\n#include <stddef.h>\n#include "permon_hip.h"\nint main(void){ printf("%zu %zu %zu %zu\\n", sizeof(pmh_mpgp_phase_test), ' \
          'offsetof(pmh_mpgp_phase_test, astol), offsetof(pmh_mpgp_phase_test, emit), offsetof(pmh_mpgp_phase_test, ctl)); return 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        sizes = list(map(int, subprocess.check_output([os.path.join(d, "s")]).split()))
    T = _lib.MpgpPhaseTest
    assert [ctypes.sizeof(T), T.astol.offset, T.emit.offset, T.ctl.offset] == sizes


# ---- the dual-space chain ----------------------------------------------------------------------------------------------------------------------------------------------
SMALL_CHAINS = ("n1_m1", "n37_m6", "n1024_m17_w16", "n1025_m64", "n1500_m6")


def _dense_chain(c, S, x, rho, T=np.float64):
    """y = rho Q x + P F P x, Q = G0' S G0, P = I - Q, F = scatter middle gather, with dense matrices in the arithmetic T; and the same with every matrix and vector
    replaced by its absolute values and every minus by a plus: the sum of the absolute values of all the terms."""
    G, Bg, M, Bs = (D.csr_dense(c[k], T) for k in ("G0", "gather", "middle", "scatter"))
    S, x = S.astype(T), x.astype(T)
    Q = lambda v: G.T @ (S @ (G @ v))  # noqa: E731
    Px = x - Q(x)
    w = Bs @ (M @ (Bg @ Px))
    y = T(rho) * Q(x) + (w - Q(w))
    aG, aBg, aM, aBs, aS, ax = (np.abs(v) for v in (G, Bg, M, Bs, S, x))
    aQ = lambda v: aG.T @ (aS @ (aG @ v))  # noqa: E731
    aw = aBs @ (aM @ (aBg @ (ax + aQ(ax))))
    return y, T(rho) * aQ(ax) + aw + aQ(aw), dict(Px=Px, w=w)


def test_chain_cases_reach_the_plans_they_are_named_after():
    for name, (n, m, wide, W, NU) in D.CHAIN_CASES.items():
        c = D.chain_case(name)
        p = D.chain_plan(c["G0"], c["gather"], c["scatter"])
        info = p["info"]
        assert info[:3] == [n, m, -(-n // 1024)] and (info[4], info[5]) == (W, NU), (name, info)
        assert (info[2] <= 128) == (NU == 2)
        if n > 1:
            assert info[7] > 0 and info[8] > 0 and info[9] > 0 and info[6] < c["gather"]["nrows"] - info[7], (name, info)  # partners, long rows on both sides, empty rows
        glen, slen = np.diff(c["gather"]["rowptr"]), np.diff(c["scatter"]["rowptr"])
        assert set(glen.tolist()) >= ({0, 1} if n == 1 else {0, 1, 2, 3, 5}) and (n < 4 or set(slen.tolist()) == {0, 1, 2, 4})
        mr = np.repeat(np.arange(c["nmid"]), np.diff(c["middle"]["rowptr"]))
        assert set(zip(mr[:50].tolist(), c["middle"]["col"][:50].tolist())) != set(zip(c["middle"]["col"][:50].tolist(), mr[:50].tolist())) and np.diff(c["middle"]["rowptr"]).max() <= 2
        # a row that shares its key with another row and is not its opposite: listed on its own
        same = [r for r in p["listed"][1:200] if p["partner"][r] == -1 and glen[r] and glen[r - 1] == glen[r]
                and np.array_equal(c["gather"]["val"][c["gather"]["rowptr"][r]:c["gather"]["rowptr"][r + 1]], c["gather"]["val"][c["gather"]["rowptr"][r - 1]:c["gather"]["rowptr"][r]])]
        assert same or n == 1, name
    seglen = lambda name: {k1 - k0 for t in D.chain_plan(*(D.chain_case(name)[k] for k in ("G0", "gather", "scatter")))["tiles"] for k0, k1, _, _ in t}  # noqa: E731
    assert seglen("n1024_m17_w16") >= {1, 256, 257, 1024}
    tiles = lambda name: [len(t) for t in D.chain_plan(*(D.chain_case(name)[k] for k in ("G0", "gather", "scatter")))["tiles"]]  # noqa: E731
    assert tiles("n1025_m64")[0] == 64 and tiles("n1500_m6") == [6, 0] and tiles("n1_m1") == [1]
    cnt = np.bincount(D.chain_case("n1024_m17_w16")["G0"]["col"])
    assert 9 <= cnt.max() <= 16 and np.bincount(D.chain_case("n1025_m64")["G0"]["col"]).max() <= 8


def test_projector_cases_reach_the_long_row_plan_and_every_loop():
    """The cases of tests/test_gpu_projector_paths.py: G0 on the long-row plan, the chunk counts and workgroups each is named for, a one-lane-per-row G0' (at most 16
    entries per column: one trip of the row loop), m at both ends -- and n4300 close enough to the threshold that a tenth fewer columns would leave the plan."""
    for name, (n, m, _, chunks0, nwg) in D.PROJECTOR_CASES.items():
        c = D.chain_case(name)
        G0 = c["G0"]
        is_long, chunks = D.long_rows(G0)
        assert is_long and (c["n"], c["m"]) == (n, m) and chunks[0] == chunks0 and D.vec_grid(n) == nwg == -(-n // D.BLOCK), (name, chunks)
        assert chunks[1:].min() == 1 and chunks[1:].max() <= 2 and n % D.LONG_CHUNK and n % D.BLOCK  # ragged last chunk, ragged last workgroup
        assert 1 <= np.bincount(G0["col"], minlength=n).min() and np.bincount(G0["col"], minlength=n).max() <= 4
    assert D.PROJECTOR_CASES["n36900_m6"][3] > 8 and D.PROJECTOR_CASES["n36900_m6"][3] % 8  # a second, ragged trip of the 8-in-flight loop
    assert max(v[1] for v in D.PROJECTOR_CASES.values()) == 64
    rp = D.chain_case("n4300_m6")["G0"]["rowptr"]
    assert (rp[-1] - 0.1 * 4300 * 4 / 3) / 6 <= D.LONG_AVG


@pytest.mark.parametrize("name", SMALL_CHAINS)
def test_chain_restatement_counts_every_entry_once(name):
    """Small integers everywhere (G0, S, the three stages, x, rho = 2): every sum is exact in any order, and the restated chain must equal the dense float64 product bit
    for bit, stage by stage -- the segment table, the slot copy, the records, the partner rows and the tails are then all in place."""
    c = D.chain_case(name, True)
    p = D.chain_plan(c["G0"], c["gather"], c["scatter"])
    m = c["m"]
    S = np.eye(m) + np.diag(np.ones(m - 1), 1) - np.diag(np.ones(m - 1), -1)  # not symmetric: a transposed S shows
    y, _, mid = _dense_chain(c, S.T, c["x"], 2.0)  # (the kernels take S by rows with lane = column: c = S' a)
    o = D.chain_apply(c, p, S, c["x"], 2.0)
    G = D.csr_dense(c["G0"])
    assert np.array_equal(o["c"], S.T @ (G @ c["x"]))
    assert np.array_equal(o["mid_in"], D.csr_dense(c["gather"]) @ mid["Px"]) and np.array_equal(o["w"], mid["w"])
    a, _ = D.coarse_share(p, o["wsums"], S)
    assert np.array_equal(a, G @ mid["w"])
    assert np.array_equal(o["y"], y) and np.max(np.abs(y)) < 2.0 ** 52
    b = D.chain_case(name, True)["x"][::-1].copy()
    gs = D.chain_apply(c, p, S, c["x"], 2.0, 2, epi=dict(b=b, lb=None, ub=None, astol=D.ASTOL))
    assert np.array_equal(gs["y"], y - b) and np.array_equal(gs["gf"], y - b) and np.array_equal(gs["psums"], D.emit_sums(p, c["G0"], y - b))
    yn, sq = D.chain_norm(p, o["part"], S)
    assert np.array_equal(yn, S.T @ (G @ c["x"])) and sq == yn @ yn


@pytest.mark.parametrize("name", SMALL_CHAINS)
def test_chain_restatement_against_long_double(name):
    """Real data, S = (G0 G0')^-1 rounded to float64 and taken as given by both sides.  Roundings on the longest path, stage by stage: a segment 1 + 16 + 6 (product, a
    lane's entries, the butterflies); a row's segments NU + 6; c = S a: 1 + 4 + 16; (G0' c)_j: 1 + W; P x: 2; a gather row 1 + its entries; the middle stage 3; a
    scatter row 1 + its entries; then the second projection again and the last line: 4.  The sum of all of them bounds the composition."""
    c = D.chain_case(name)
    p = D.chain_plan(c["G0"], c["gather"], c["scatter"])
    G = D.csr_dense(c["G0"], LD)
    S = np.linalg.inv((G @ G.T).astype(np.float64))
    proj = (1 + 16 + 6) + (p["NU"] + 6) + (1 + 4 + 16) + (1 + p["W"])
    k = 2 * proj + 2 + (1 + int(np.diff(c["gather"]["rowptr"]).max())) + 3 + (1 + int(np.diff(c["scatter"]["rowptr"]).max())) + 4
    y, mag, _ = _dense_chain(c, S.T, c["x"], c["rho"], LD)
    o = D.chain_apply(c, p, S, c["x"], c["rho"])
    assert np.all(np.abs(o["y"].astype(LD) - y) <= gamma(k) * mag), (name, float(np.max(np.abs(o["y"].astype(LD) - y) / mag)), gamma(k))
    # the two epilogues on top of the same product
    pc = D.phase_case(c["n"], "both", 3)
    gs = D.chain_apply(c, p, S, c["x"], c["rho"], 2, epi=dict(b=pc["b"], lb=pc["lb"], ub=pc["ub"], astol=D.ASTOL))
    assert np.array_equal(gs["y"], o["y"] + -1.0 * pc["b"])
    f, cc = D.box_split(c["x"], gs["y"], pc["lb"], pc["ub"], D.ASTOL)
    assert np.array_equal(gs["gf"], f) and np.array_equal(gs["p"], f)
    got = np.array([D.host_sum_row(r, len(r)) for r in gs["rows"]])
    kk = 1 + 1 + K_TILE + K_ROW
    for j, v in ((1, f + cc), (2, cc), (3, f)):
        _close(got[j], (v.astype(LD) ** 2).sum(), kk, (v.astype(LD) ** 2).sum(), ("gradient split", j))
    p1 = D.chain_apply(c, p, S, c["x"], c["rho"], 1, epi=dict(g=pc["g"], xx=pc["x"], lb=pc["lb"], ub=pc["ub"]))
    assert np.array_equal(p1["y"], o["y"])
    _close(D.host_sum_row(p1["rows"][0], p["nwg"]), (c["x"].astype(LD) * o["y"].astype(LD)).sum(), kk, np.abs(c["x"] * o["y"]).astype(LD).sum(), "p'Ap")
    _close(D.host_sum_row(p1["rows"][1], p["nwg"]), (pc["g"].astype(LD) * c["x"].astype(LD)).sum(), kk, np.abs(pc["g"] * c["x"]).astype(LD).sum(), "g'p")
    assert D.host_sum_row(p1["rows"][2], p["nwg"], D.MIN) == D.box_feas(pc["x"], c["x"], pc["lb"], pc["ub"]).min()


def test_solve_cases_take_every_step_type():
    """The two whole-solve cases of the device tests, restated: CG, expansion and proportioning steps all occur, within 60 iterations, and the solves converge.  (The
    chain's S comes from the device there and from numpy here: the step string may differ by a rounding, the property must not be a knife's edge -- it holds for
    both step lengths below.)"""
    sc = D.solve_case("shell")
    M = sc["A"]
    steps, mon, x, reason = D.solve_fused(D.ShellModel(lambda v: D._rows_left_to_right(M, M["val"] * v[M["col"]])), sc["b"], sc["x0"], sc["lb"], sc["ub"], 0.45)
    assert {"c", "e", "p"} <= set(steps) and reason == 2 and len(steps) <= 61 and steps[0] == " "
    assert np.all(x >= sc["lb"] - 1e-12) and np.all(x <= sc["ub"] + 1e-12)
    Ad = D.csr_dense(M)
    g = Ad @ x - sc["b"]
    free = (x > sc["lb"] + 1e-9) & (x < sc["ub"] - 1e-9)
    assert np.linalg.norm(g[free]) <= 1e-4 * np.linalg.norm(sc["b"])  # a KKT point: the restated solve solves the problem
    sc = D.solve_case("chain")
    c = sc["chain"]
    plan = D.chain_plan(c["G0"], c["gather"], c["scatter"])
    assert plan["info"][7] > 0 and plan["info"][8] > 0 and plan["info"][9] > 0
    G = D.csr_dense(c["G0"])
    S = np.linalg.inv(G @ G.T)
    for alpha in (0.38, 0.37):
        steps, mon, x, reason = D.solve_fused(D.ChainModel(c, plan, S), sc["b"], sc["x0"], sc["lb"], sc["ub"], alpha, rtol=1e-4)
        assert {"c", "e", "p"} <= set(steps) and reason == 2 and len(steps) <= 61, (alpha, steps)


def test_csr_model_counts_every_row_once():
    """The persistent grid of the ELL product's MPGP epilogue, restated: whatever the grid, every row is added exactly once (small integers: exact)."""
    rng = np.random.default_rng(3)
    for n, nl, nrb in ((700, 8, 3), (256 * 21 + 5, 24, 22), (256 * 21 + 5, 8, 22), (256 * 64, 64, 64)):
        m = D.CsrModel(D.tridiagonal(4), nl, nrb)
        m.n = n
        t = rng.integers(-9, 10, n).astype(np.float64)
        assert m._partials(t).sum() == t.sum() and len(m._partials(t)) == nl
        have = rng.random(n) < 0.3
        assert m._partials(np.abs(t), D.MIN, have).min() == np.abs(t)[have].min()
    sc = D.solve_case("shell")
    M = sc["A"]
    ref = D.solve_fused(D.ShellModel(lambda v: D._rows_left_to_right(M, M["val"] * v[M["col"]])), sc["b"], sc["x0"], sc["lb"], sc["ub"], 0.45)
    got = D.solve_fused(D.CsrModel(M, 8, 3), sc["b"], sc["x0"], sc["lb"], sc["ub"], 0.45)
    assert {"c", "e", "p"} <= set(got[0]) and got[3] == 2 and len(got[0]) <= 61
    assert np.linalg.norm(got[2] - ref[2]) <= 1e-6 * np.linalg.norm(ref[2])  # the two drivers' orders differ by roundings only


def test_carried_gradient_solves_take_every_step_type():
    """The solves that start from a carried gradient (the device tests hand over a vector that is NOT the gradient at the starting point, so that a driver which formed
    its own would show): CG, expansion and proportioning steps within 60 iterations, on the plain operators and on the chain."""
    sc = D.solve_case("shell")
    M = sc["A"]
    mult = lambda v: D._rows_left_to_right(M, M["val"] * v[M["col"]])  # noqa: E731
    g0 = D.carried_gradient(sc, mult(sc["x0"]) - sc["b"])
    for model in (D.ShellModel(mult), D.CsrModel(M, 8, 3)):
        own = D.solve_fused(model, sc["b"], sc["x0"], sc["lb"], sc["ub"], 0.45)
        steps, mon, x, reason = D.solve_fused(model, sc["b"], sc["x0"], sc["lb"], sc["ub"], 0.45, g0=g0)
        assert {"c", "e", "p"} <= set(steps) and len(steps) <= 62 and reason in (2, -3), steps
        assert not np.array_equal(mon[0], own[1][0])  # the first monitor line already tells a carried gradient from a formed one
    sc = D.solve_case("chain")
    c = sc["chain"]
    plan = D.chain_plan(c["G0"], c["gather"], c["scatter"])
    G = D.csr_dense(c["G0"])
    model = D.ChainModel(c, plan, np.linalg.inv(G @ G.T))
    g0 = D.carried_gradient(sc, model.grad_split(sc["x0"], sc["b"], sc["lb"], sc["ub"], D.ASTOL)[0])
    steps, mon, x, reason = D.solve_fused(model, sc["b"], sc["x0"], sc["lb"], sc["ub"], 0.38, rtol=1e-4, g0=g0)
    assert {"c", "e", "p"} <= set(steps) and len(steps) <= 62 and reason in (2, -3), steps
