"""Plain numpy restatements, every sum in the order the source fixes, of: the reduction finishers (csrc/reduce.h, csrc/emit_inline.h, k_finalize of csrc/vec.hip,
host_sum_row of csrc/mpgp.hip); the box predicates (csrc/box_inline.h) and the MPGP phase kernels (csrc/mpgp.hip) on both entry maps; the dual-space chain
(csrc/dualchain.hip: segment table, slot copy, gather records, emission, coarse share, the five kernels with both epilogues); and solve_fused for a shell operator,
a CSR operator on the ELL plan and the chained operator, from a fresh or a carried gradient.  With them the case generators of tests/test_gpu_mpgp_phases.py and
tests/test_gpu_chain_paths.py.  The library is built without contraction and these kernels use no atomics and no matrix cores, so the device must give the same
bits.  tests/test_dual_reference_host.py ties this file to long-double and exact-integer arithmetic and pins what each generator claims to reach.  No GPU here."""
import functools

import numpy as np

BLOCK, TILE, MAX_BLOCKS, FIN_THREADS = 256, 1024, 2048, 1024  # PMH_BLOCK, PMH_EMIT_TILE, PMH_MAX_VEC_BLOCKS, PMH_FIN_THREADS
SUM, MIN = 0, 1  # PMH_RED_SUM, PMH_RED_MIN
S_PAP, S_GP, S_FEAS, S_APGF, S_GP2, S_GC2, S_GF2, S_TMP = 8, 9, 10, 16, 17, 18, 19, 24  # scalar slots of mpgp.hip
HALT, ITER, NCG, BASE = 0, 1, 2, 3  # control words of the speculative chain
ASTOL = 10 * 2.220446049250313e-16  # pmh_mpgp_default_opts
INF = np.inf


def _comb(a, b, op):
    return a + b if op == SUM else np.fmin(a, b)


# ---- reductions ----------------------------------------------------------------------------------------------------------------------------------------------------
def wave_reduce(v, op=SUM):
    """pmh_wave_sum / pmh_wave_min (reduce.h): lane l takes lane l + o for o = 32, 16, .. 1; the value of lane 0.  v[..., 64]."""
    v = np.asarray(v, np.float64)
    for o in (32, 16, 8, 4, 2, 1):
        v = _comb(v[..., :o], v[..., o:2 * o], op)  # the lanes lane 0 still depends on
    return v[..., 0]


_L = np.arange(64)
BUTTERFLY = (_L ^ 1, _L ^ 2, (_L & ~7) | (7 - (_L & 7)), (_L & ~15) | (15 - (_L & 15)))  # quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror


def wave_all(v, op=SUM):
    """pmh_wave_all (emit_inline.h): four butterflies inside a row of 16 lanes, then the four rows as (r0 + r1) + (r2 + r3).  v[..., 64] -> [...]."""
    v = np.asarray(v, np.float64)
    for partner in BUTTERFLY:
        v = _comb(v, v[..., partner], op)
    return _comb(_comb(v[..., 0], v[..., 16], op), _comb(v[..., 32], v[..., 48], op), op)


def _in_order(w, op):
    r = w[..., 0]
    for k in range(1, w.shape[-1]):
        r = _comb(r, w[..., k], op)
    return r


def block_reduce(v, op=SUM):
    """pmh_block_reduce (reduce.h): the shuffle tree in each of the 4 waves, then the waves in order.  v[nblocks, 256] -> [nblocks]."""
    return _in_order(wave_reduce(v.reshape(v.shape[0], BLOCK // 64, 64), op), op)


def block_partials(v, op=SUM):
    """pmh_block_partials (emit_inline.h): the butterflies in each of the 16 waves, then the waves in order.  v[nblocks, 1024] -> [nblocks]."""
    return _in_order(wave_all(v.reshape(v.shape[0], TILE // 64, 64), op), op)


def _lane_strided(row, nb, op):
    assert 0 <= nb <= 512, "out of contract: a lane holds 8 entries"
    p = np.full(512, 0.0 if op == SUM else INF)
    p[:nb] = row[:nb]
    p = p.reshape(8, 64)
    acc = np.full(64, 0.0 if op == SUM else INF)
    for u in range(8):
        acc = _comb(acc, p[u], op)
    return acc


def sum_block_partials(row, nb):
    """pmh_sum_block_partials (emit_inline.h): lane l adds entries l, l + 64, ... in that order from 0.0, then the butterflies."""
    return wave_all(_lane_strided(np.asarray(row, np.float64), nb, SUM), SUM)


def host_sum_row(row, nb, op=SUM):
    """host_sum_row (mpgp.hip): the same on the host, also for MIN."""
    return wave_all(_lane_strided(np.asarray(row, np.float64), nb, op), op)


def finalize(rows, ops):
    """k_finalize (vec.hip): thread t takes blocks t, t + 1024, ... in that order, the shuffle tree in each of the 16 waves, the waves in order.
    rows[K, nblocks] -> [K]."""
    rows = np.asarray(rows, np.float64)
    out = np.empty(len(ops))
    for k, op in enumerate(ops):
        nblocks = rows.shape[1]
        laps = max(1, -(-nblocks // FIN_THREADS))
        ident = 0.0 if op == SUM else INF
        p = np.full(laps * FIN_THREADS, ident)
        p[:nblocks] = rows[k]
        have = (np.arange(laps * FIN_THREADS) < nblocks).reshape(laps, FIN_THREADS)
        p = p.reshape(laps, FIN_THREADS)
        v = np.full(FIN_THREADS, ident)
        for lap in range(laps):
            v = np.where(have[lap], _comb(v, p[lap], op), v)
        out[k] = _in_order(wave_reduce(v.reshape(FIN_THREADS // 64, 64), op), op)
    return out


# ---- the two entry maps of a vector kernel -------------------------------------------------------------------------------------------------------------------------
def vec_grid(n):
    """pmh_vec_grid (vec.hip)."""
    return int(min(max((n + BLOCK - 1) // BLOCK, 1), MAX_BLOCKS))


def emit_blocks(n):
    return (n + TILE - 1) // TILE


def nblocks_of(n, emit):
    return emit_blocks(n) if emit else vec_grid(n)


def grid_partials(term, emit, op=SUM, have=None):
    """The block partials of one accumulator.  Plain grid: thread t of workgroup b adds its entries 256 b + t, + 256 grid, ... in that order from 0.0 (+inf for MIN;
    entries with have == False are skipped), then pmh_block_reduce.  1024-entry tiles: one entry per thread, added to 0.0, then pmh_block_partials."""
    n = len(term)
    ident = 0.0 if op == SUM else INF
    have = np.ones(n, bool) if have is None else have
    if emit:
        nb = emit_blocks(n)
        t = np.full(nb * TILE, ident)
        t[:n] = np.where(have, _comb(np.full(n, ident), term, op), ident)
        return block_partials(t.reshape(nb, TILE), op)
    G = vec_grid(n)
    laps = -(-n // (G * BLOCK))
    t = np.full(laps * G * BLOCK, ident)
    t[:n] = term
    h = np.zeros(laps * G * BLOCK, bool)
    h[:n] = have
    t, h = t.reshape(laps, G, BLOCK), h.reshape(laps, G, BLOCK)
    acc = np.full((G, BLOCK), ident)
    for lap in range(laps):
        acc = np.where(h[lap], _comb(acc, t[lap], op), acc)
    return block_reduce(acc, op)


# ---- box predicates (box_inline.h) ------------------------------------------------------------------------------------------------------------------------------------
def box_split(x, g, lb, ub, astol):
    """pmh_box_split: (gf, gc); the lower bound wins ties; a null array and an infinite entry both leave the entry free."""
    with np.errstate(invalid="ignore"):
        at_l = np.zeros(len(x), bool) if lb is None else np.abs(x - lb) <= astol
        at_u = ~at_l & (np.zeros(len(x), bool) if ub is None else np.abs(x - ub) <= astol)
    gf = np.where(at_l | at_u, 0.0, g)
    gc = np.where(at_l, np.where(g < 0.0, g, 0.0), np.where(at_u, np.where(g > 0.0, g, 0.0), 0.0))
    return gf, gc


def box_reduced(x, gf, lb, ub, alpha):
    """pmh_box_reduced."""
    r = gf.copy()
    with np.errstate(invalid="ignore"):
        if lb is not None:
            t = (x - lb) / alpha
            r = np.where(gf > 0.0, np.where(gf < t, gf, t), r)
        if ub is not None:
            t = (x - ub) / alpha
            r = np.where(gf < 0.0, np.where(gf < t, t, gf), r)
    return r


def box_arms(x, g, lb, ub, astol):
    """Which arm of pmh_box_split each entry takes: 0 free, 1 lower with g < 0, 2 lower with g >= 0, 3 upper with g > 0, 4 upper with g <= 0."""
    with np.errstate(invalid="ignore"):
        at_l = np.zeros(len(x), bool) if lb is None else np.abs(x - lb) <= astol
        at_u = ~at_l & (np.zeros(len(x), bool) if ub is None else np.abs(x - ub) <= astol)
    return np.where(at_l, np.where(g < 0.0, 1, 2), np.where(at_u, np.where(g > 0.0, 3, 4), 0))


# ---- phase kernels (mpgp.hip) ------------------------------------------------------------------------------------------------------------------------------------
def _norm_rows(f, c, emit, row0):
    gP = f + c
    return np.stack([row0, grid_partials(gP * gP, emit), grid_partials(c * c, emit), grid_partials(f * f, emit)])


def split_setp(x, g, lb, ub, astol, emit=False):
    """k_split_setp: gf, p = gf, and the block partials (0, |gP|^2, |gc|^2, |gf|^2)."""
    f, c = box_split(x, g, lb, ub, astol)
    return dict(gf=f, p=f.copy(), partials=_norm_rows(f, c, emit, grid_partials(np.zeros(len(x)), emit)))


def step_update(acg, x, g, p, Ap, lb, ub, astol, setp, emit=False):
    """k_step_update past its verdict: x -= acg p, g -= acg Ap, the split, (Ap'gf, |gP|^2, |gc|^2, |gf|^2)."""
    ma = -acg
    xi = x + ma * p
    gi = g + ma * Ap
    f, c = box_split(xi, gi, lb, ub, astol)
    return dict(x=xi, g=gi, gf=f, p=f.copy() if setp else p.copy(), partials=_norm_rows(f, c, emit, grid_partials(Ap * f, emit)))


def step_acg(scal=None, acg_host=None, partials=None, nb_p1=0):
    """The step length as k_step_update forms it: device scalars (plain grid), the host's number or the P1 block partials, rows 4 and 5 (1024-entry tiles)."""
    if scal is not None:
        return scal[S_GP] / scal[S_PAP]
    return sum_block_partials(partials[5], nb_p1) / sum_block_partials(partials[4], nb_p1) if nb_p1 > 0 else acg_host


def spec_go(ctl, scal, acg, ring_cap, max_it, ttol, divtol_rhs, gamma2):
    """The verdict of k_step_update<false, true>; None where the halt word is already set (the kernel returns before it looks)."""
    if ctl[HALT]:
        return None
    it = ctl[ITER]
    gP2, gc2, gf2 = scal[S_GP2], scal[S_GC2], scal[S_GF2]
    with np.errstate(invalid="ignore"):
        rnorm = np.sqrt(gP2)
        go = (it <= max_it) and (rnorm > ttol) and (rnorm < divtol_rhs)
        return bool(go and (gc2 <= gamma2 * gf2) and (acg <= scal[S_FEAS]) and (it - ctl[BASE] < ring_cap))


def dir_update(bcg, gf, p):
    """k_dir_update: p = gf - bcg p."""
    return gf + (-bcg) * p


def prop_dir(x, g, lb, ub, astol):
    """k_prop_dir: p = gc."""
    return box_split(x, g, lb, ub, astol)[1]


def expansion_std(afeas, alpha, x, g, p, Ap, lb, ub, astol):
    """k_expansion_std: the new x."""
    xi = x + (-afeas) * p
    gi = g + (-afeas) * Ap
    f, _ = box_split(xi, gi, lb, ub, astol)
    return xi + (-alpha) * box_reduced(xi, f, lb, ub, alpha)


def p1_dots(p, Ap, g, x, lb, ub):
    """k_p1_dots: the block partials of p'Ap, g'p and the feasible step (MIN)."""
    n = len(p)
    q, have = np.full(n, INF), np.zeros(n, bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        if lb is not None:
            k = (p > 0.0) & (lb > -INF)
            q, have = np.where(k, (x - lb) / p, q), have | k
        if ub is not None:
            k = (p < 0.0) & (ub < INF)
            q, have = np.where(k, (x - ub) / p, q), have | k
    return np.stack([grid_partials(p * Ap, False), grid_partials(g * p, False), grid_partials(q, False, MIN, have)])


def three_norms(gP, gc, gf):
    """k_three_norms."""
    return np.stack([grid_partials(np.zeros(len(gP)), False), grid_partials(gP * gP, False), grid_partials(gc * gc, False), grid_partials(gf * gf, False)])


def obj_from_grad(x, g, b):
    """k_obj_from_grad."""
    return grid_partials(x * (-1.0 * b + g), False)[None, :]


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------------------------------
PLAIN_N = (1, 255, 256, 257, 4099, 262144 + 300, 524288 + 300)  # > 1024 workgroups: k_finalize's second lap; grid capped at 2048: a second grid-stride lap
EMIT_N = (1500, 64 * 1024, 64 * 1024 + 1, 524288)  # one entry per lane of pmh_sum_block_partials, a second entry for lane 0, the contract's 512 blocks
BOUNDS = ("none", "lb", "ub", "both")
EDGE = 12  # entries i with i % 37 < EDGE carry one of the edge patterns below


@functools.lru_cache(maxsize=None)
def phase_case(n, bounds, seed=0):
    """Vectors for one launch.  Entries i % 37 == k < 12 sit, with p = 0 so that a step leaves them there, at: 0 on lb; 1 lb + astol (lb = 0); 2 one ulp outside
    that; 3 on ub; 4 ub - astol (ub = 0); 5 one ulp outside; 6 lb == ub == x (the lower bound must win); 7 on lb with g >= 0; 8 on ub with g <= 0; 9 on lb with
    g = 0; 10 lb = -inf; 11 ub = +inf.  Everywhere else the bounds are random with a fifth of each side infinite, x inside, and p of both signs."""
    rng = np.random.default_rng([n, BOUNDS.index(bounds), seed])
    x = rng.standard_normal(n)
    g, p, Ap, b = (rng.standard_normal(n) for _ in range(4))
    lb = x - rng.uniform(0.1, 2.0, n)
    ub = x + rng.uniform(0.1, 2.0, n)
    lb[rng.random(n) < 0.2] = -INF
    ub[rng.random(n) < 0.2] = INF
    k = np.arange(n) % 37
    p[k < EDGE] = 0.0
    up = np.nextafter(ASTOL, INF)
    for kk, (xv, lv, uv, gs) in enumerate([(None, 0, 1, -1), (ASTOL, 0.0, 1.0, -1), (up, 0.0, 1.0, -1), (None, -1, 0, 1), (-ASTOL, -1.0, 0.0, 1), (-up, -1.0, 0.0, 1),
                                            (None, 0, 0, -1), (None, 0, 1, 1), (None, -1, 0, -1), (None, 0, 1, 0), (None, -INF, 1, 1), (None, -1, INF, -1)]):
        m = k == kk
        if xv is None:  # x stays; a bound given as 0 sits on x, as +-1 that far away
            lb[m] = x[m] + lv if np.isfinite(lv) else lv
            ub[m] = x[m] + uv if np.isfinite(uv) else uv
        else:
            x[m], lb[m], ub[m] = xv, lv, uv
        g[m] = gs * np.abs(g[m])
    return dict(n=n, x=x, g=g, p=p, Ap=Ap, b=b, gf=rng.standard_normal(n), lb=lb if bounds in ("lb", "both") else None, ub=ub if bounds in ("ub", "both") else None)


def reduction_rows(nb, seed=0):
    """Rows of block partials: normal numbers of both signs over ten decades, where no two orders of summation agree by accident."""
    rng = np.random.default_rng([nb, seed, 7])
    return rng.standard_normal((8, nb)) * 10.0 ** rng.integers(-5, 5, (8, nb))


def spec_cases():
    """name -> (control words, scalar slots, constants of pmh_spec_args, verdict): the go case, the go case with every comparison at equality, and one case per
    reason to halt.  The verdict None: the halt word was set before the launch."""
    def scal(**kw):
        s = np.full(64, 7.25e77)
        v = dict(GP2=4.0, GC2=1.0, GF2=2.0, GP=0.6, PAP=2.0, FEAS=0.5, APGF=0.25)
        v.update(kw)
        for k, x in v.items():
            s[globals()["S_" + k]] = x
        return s

    def const(**kw):
        return dict(dict(ring_cap=16, max_it=100, ttol=1e-3, divtol_rhs=1e4, gamma2=1.0), **kw)

    return {
        "go": ([0, 5, 2, 3], scal(), const(), True),
        "go_at_equality": ([0, 100, 2, 98], scal(GC2=2.0, FEAS=0.6 / 2.0), const(ring_cap=3), True),
        "max_it": ([0, 101, 2, 99], scal(), const(), False),
        "ttol": ([0, 5, 2, 3], scal(GP2=0.25), const(ttol=0.5), False),
        "diverged": ([0, 5, 2, 3], scal(GP2=4.0), const(divtol_rhs=2.0), False),
        "nan": ([0, 5, 2, 3], scal(GP2=np.nan), const(), False),
        "not_proportional": ([0, 5, 2, 3], scal(GC2=np.nextafter(2.0, 3.0)), const(), False),
        "acg_above_afeas": ([0, 5, 2, 3], scal(FEAS=np.nextafter(0.3, 0.0)), const(), False),
        "ring_full": ([0, 5, 2, 3], scal(), const(ring_cap=2), False),
        "halted_before": ([1, 5, 2, 3], scal(), const(), None),
    }


# ==== the dual-space chain (csrc/dualchain.hip, csrc/emit_inline.h) ====================================================================================================
def _csr(rows, ncols):
    """rows: list of (columns, values) -> CSR dict."""
    rp = np.zeros(len(rows) + 1, np.int32)
    rp[1:] = np.cumsum([len(c) for c, _ in rows])
    col = np.concatenate([np.asarray(c, np.int32) for c, _ in rows] + [np.zeros(0, np.int32)])
    val = np.concatenate([np.asarray(v, np.float64) for _, v in rows] + [np.zeros(0)])
    return dict(nrows=len(rows), ncols=ncols, rowptr=rp, col=col.astype(np.int32), val=val)


def csr_dense(M, dtype=np.float64):
    D = np.zeros((M["nrows"], M["ncols"]), dtype)
    r = np.repeat(np.arange(M["nrows"]), np.diff(M["rowptr"]))
    np.add.at(D, (r, M["col"]), M["val"].astype(dtype))
    return D


def chain_plan(G0, gather, scatter):
    """What pmh_dc_create and dc_prepare_stages build: the segment table (per tile of 1024 columns up to 64 fixed places, a tile's segments by ascending row; the sum of
    row r's i-th segment at lrow[r] + i), the slot copy of G0' (column j's entries by ascending row, zero padding), the gather records (rows with entries, without
    the rows that are somebody's partner) and the counts the info entry reports."""
    n, m, rp = G0["ncols"], G0["nrows"], G0["rowptr"]
    nwg = (n + TILE - 1) // TILE
    tiles, lrow = [[] for _ in range(nwg)], np.zeros(m + 1, np.int64)
    for r in range(m):
        c = G0["col"][rp[r]:rp[r + 1]]
        assert np.all(np.diff(c) > 0)
        cut = np.flatnonzero(np.diff(c // TILE)) + 1
        for i, (a, b) in enumerate(zip(np.concatenate([[0], cut]), np.concatenate([cut, [len(c)]]))) if len(c) else ():
            tiles[c[a] // TILE].append((rp[r] + a, rp[r] + b, i, r))
        lrow[r + 1] = lrow[r] + (len(cut) + 1 if len(c) else 0)
    cnt = np.bincount(G0["col"], minlength=n)
    W = 8 if cnt.max(initial=0) <= 8 else 16
    assert cnt.max(initial=0) <= 16 and m <= 64
    ev, ec, fill = np.zeros((n, W)), np.zeros((n, W), np.int64), np.zeros(n, np.int64)
    for r in range(m):
        j = G0["col"][rp[r]:rp[r + 1]]
        ev[j, fill[j]], ec[j, fill[j]] = G0["val"][rp[r]:rp[r + 1]], r
        fill[j] += 1
    # partner rows: among the rows with the same columns and the same |values|, ascending, a free row takes the first free later row with the opposite values
    grp, gp = {}, gather["rowptr"]
    for r in range(gather["nrows"]):
        if gp[r + 1] > gp[r]:
            grp.setdefault((gather["col"][gp[r]:gp[r + 1]].tobytes(), np.abs(gather["val"][gp[r]:gp[r + 1]]).tobytes()), []).append(r)
    partner = np.full(gather["nrows"], -1)
    for rows in grp.values():
        for a, r in enumerate(rows):
            if partner[r] != -1:
                continue
            for q in rows[a + 1:]:
                if partner[q] == -1 and np.array_equal(gather["val"][gp[r]:gp[r + 1]], -gather["val"][gp[q]:gp[q + 1]]):
                    partner[r], partner[q] = q, -2
                    break
    listed = [r for r in range(gather["nrows"]) if gp[r + 1] > gp[r] and partner[r] != -2]
    glen, slen = np.diff(gp), np.diff(scatter["rowptr"])
    info = [n, m, nwg, int(lrow[m]), W, 2 if nwg <= 128 else 8, len(listed), int(sum(partner[r] >= 0 for r in listed)), int(sum(glen[r] > 3 for r in listed)), int(np.sum(slen > 2))]
    return dict(n=n, m=m, nwg=nwg, tiles=tiles, lrow=lrow, nseg=int(lrow[m]), W=W, NU=info[5], ev=ev, ec=ec, listed=listed, partner=partner, info=info)


def emit_sums(plan, G0, v):
    """pmh_emit_prefetch + pmh_emit_tail: per segment, lane l adds the products of its entries k0 + l, k0 + l + 64, ... in that order (the four prefetched ones, then the
    rest from k0 + l + 256), then the butterflies; the sum goes to its fixed place."""
    part = np.zeros(plan["nseg"])
    for segs in plan["tiles"]:
        assert len(segs) <= 64
        for k0, k1, i, r in segs:
            pr = np.zeros(-(-(k1 - k0) // 64) * 64)
            pr[:k1 - k0] = G0["val"][k0:k1] * v[G0["col"][k0:k1]]
            acc = np.zeros(64)
            for chunk in pr.reshape(-1, 64):
                acc = acc + chunk
            part[plan["lrow"][r] + i] = wave_all(acc)
    return part


def coarse_share(plan, part, M):
    """pmh_coarse_share<4, NU> and its callers' sum over the waves: a[r] = the row's segment sums lane-strided (NU per lane, from 0.0) and the butterflies; wave w of 16
    owns rows w, w + 16, ...: its share per column is sum_q M[r_q][lane] a[r_q] in that order; the shares are added in wave order.  -> (a [m], M' a [64])."""
    m, NU, lrow = plan["m"], plan["NU"], plan["lrow"]
    a = np.zeros(m)
    for r in range(m):
        p = np.zeros(64 * NU)
        seg = part[lrow[r]:lrow[r + 1]]
        assert len(seg) <= 64 * NU
        p[:len(seg)] = seg
        acc = np.zeros(64)
        for chunk in p.reshape(NU, 64):
            acc = acc + chunk
        a[r] = wave_all(acc)
    Mp = np.zeros((m, 64))
    Mp[:, :m] = M
    out = np.zeros(64)
    for w in range(16):
        s = np.zeros(64)
        for r in range(w, m, 16):
            s = s + Mp[r] * a[r]
        out = out + s
    return a, out


def _slot_sums(plan, cs):
    """(G0' c)_j over the slot copy, left to right from 0.0."""
    q = np.zeros(plan["n"])
    for e in range(plan["W"]):
        q = q + plan["ev"][:, e] * cs[plan["ec"][:, e]]
    return q


def _rows_left_to_right(M, term):
    """Per CSR row the sum of term[k] over its entries, left to right from 0.0."""
    rp, out = M["rowptr"], np.zeros(M["nrows"])
    length = np.diff(rp)
    for u in range(int(length.max(initial=0))):
        rows = np.flatnonzero(length > u)
        out[rows] = out[rows] + term[rp[rows] + u]
    return out


def box_feas(x, p, lb, ub):
    """pmh_box_feas_v per entry from +inf (a null bound array: no bound)."""
    q = np.full(len(p), INF)
    with np.errstate(invalid="ignore", divide="ignore"):
        if lb is not None:
            q = np.where((p > 0.0) & (lb > -INF), np.fmin(q, (x - lb) / p), q)
        if ub is not None:
            q = np.where((p < 0.0) & (ub < INF), np.fmin(q, (x - ub) / p), q)
    return q


def _tiles(v, fill):
    nb = emit_blocks(len(v))
    t = np.full(nb * TILE, fill)
    t[:len(v)] = v
    return t.reshape(nb, TILE)


def chain_apply(case, plan, S, x, rho, kind=0, part_in=None, epi=None):
    """One application y = rho Q x + P F P x in the kernels' order; every intermediate.  part_in: the segment sums of G0 x an earlier kernel left (None: k_dc_emit
    forms them).  kind 1: the P1 epilogue (epi: g, xx, lb, ub); kind 2: the gradient split (epi: b, lb, ub, astol)."""
    G0, Bg, Md, Bs, n = case["G0"], case["gather"], case["middle"], case["scatter"], plan["n"]
    o = dict(part=emit_sums(plan, G0, x) if part_in is None else part_in)
    _, cs = coarse_share(plan, o["part"], S)
    o["c"] = cs[:plan["m"]]
    px = -1.0 * _slot_sums(plan, cs) + x  # (P x)_j as QPPFApplyP's VecAYPX forms it
    rows = _rows_left_to_right(Bg, Bg["val"] * px[Bg["col"]])
    mid_in = np.zeros(Bg["nrows"])
    L = np.array(plan["listed"], np.int64)
    mid_in[L] = rows[L]
    has = plan["partner"][L] >= 0
    mid_in[plan["partner"][L][has]] = -rows[L][has]
    o["mid_in"] = mid_in
    o["mid_out"] = _rows_left_to_right(Md, Md["val"] * mid_in[Md["col"]])  # at most two entries per row: exact in any order
    o["w"] = _rows_left_to_right(Bs, Bs["val"] * o["mid_out"][Bs["col"]])
    o["wsums"] = emit_sums(plan, G0, o["w"])
    _, es = coarse_share(plan, o["wsums"], S)
    out = _slot_sums(plan, cs) * rho + (o["w"] + -1.0 * _slot_sums(plan, es))
    if kind == 0:
        o["y"] = out
    elif kind == 1:
        o["y"] = out
        o["rows"] = np.stack([block_partials(_tiles(0.0 + x * out, 0.0)), block_partials(_tiles(0.0 + epi["g"] * x, 0.0)), block_partials(_tiles(box_feas(epi["xx"], x, epi["lb"], epi["ub"]), INF), MIN)])
    else:
        g = out + -1.0 * epi["b"]
        f, c = box_split(x, g, epi["lb"], epi["ub"], epi["astol"])
        gP = f + c
        o.update(y=g, gf=f, p=f.copy(), psums=emit_sums(plan, G0, f))
        o["rows"] = np.stack([block_partials(_tiles(np.zeros(n), 0.0)), block_partials(_tiles(0.0 + gP * gP, 0.0)), block_partials(_tiles(0.0 + c * c, 0.0)), block_partials(_tiles(0.0 + f * f, 0.0))])
    return o


def chain_norm(plan, part, Tt):
    """k_dc_norm / the gather's extra workgroup: T G0 u [m] and its squared norm."""
    _, y = coarse_share(plan, part, Tt)
    m = plan["m"]
    return y[:m], wave_all(np.where(np.arange(64) < m, y * y, 0.0))


CHAIN_CASES = {  # name -> (n, m, columns every row of G0 shares (pushes W to 16), W, NU)
    "n1_m1": (1, 1, 0, 8, 2),
    "n37_m6": (37, 6, 0, 8, 2),
    "n1024_m17_w16": (1024, 17, 10, 16, 2),
    "n1025_m64": (1025, 64, 0, 8, 2),
    "n1500_m6": (1500, 6, 0, 8, 2),
    "n131072_m6": (128 * 1024, 6, 0, 8, 2),
    "n131077_m6": (128 * 1024 + 5, 6, 0, 8, 8),
    "n131077_m17_w16": (128 * 1024 + 5, 17, 10, 16, 8),
}


# The same generator at the sizes where pmh_csr_create gives G0 the long-row plan (more than LONG_AVG entries per row on average, chunks of LONG_CHUNK) and the
# penalised operator created with chain = 0 takes the one-launch projector (k_gt_fused1d, csrc/qppf.hip): name -> (n, m, 0, chunks of row 0, 256-row workgroups)
LONG_AVG, LONG_CHUNK = 1024, 4096
PROJECTOR_CASES = {
    "n4300_m6": (4300, 6, 0, 2, 17),  # just above the threshold: two chunks, a ragged last workgroup
    "n36900_m6": (36900, 6, 0, 10, 145),  # a second trip of the 8-in-flight chunk loop with a ragged tail
    "n33793_m64": (33793, 64, 0, 9, 133),  # the full 64 x 64 matrix in LDS, t < m on every lane of wave 0; one row in the last workgroup
}


def long_rows(G0):
    """pmh_csr_create's long-row plan: whether it applies, and the chunks per row."""
    length = np.diff(G0["rowptr"])
    return bool(length.sum() / G0["nrows"] > LONG_AVG), -(-length // LONG_CHUNK)


@functools.lru_cache(maxsize=None)
def chain_case(name, dyadic=False):
    """G0 (m x n): row r holds the columns r, r + m, ... below `span` (1024 for the two-tile case of 1500: its second tile has no segment), but row 0 every column of
    that span (a segment of 1024 entries in each full tile), row 1 the first 256, row 2 the first 257, row 3 column 3 alone; `wide` > 0: rows 4..12 also the first `wide`
    columns (columns with up to 14 entries).  gather (nmid x n): rows of 1, 0, 2, 3, 1, 5 entries in turn, every 7th row followed by its negative (a partner) and
    every 11th by a copy of itself (the same key, no partner).  middle: two entries per row, not symmetric.  scatter (n x nmid): rows of 1, 2, 0, 4 entries."""
    n, m, wide, _, _ = CHAIN_CASES[name] if name in CHAIN_CASES else PROJECTOR_CASES[name]
    rng = np.random.default_rng([n, m, wide])
    val = (lambda k: rng.choice([-2.0, -1.0, 1.0, 2.0], k)) if dyadic else (lambda k: rng.uniform(0.5, 1.5, k) * rng.choice([-1.0, 1.0], k))
    span = 1024 if n == 1500 else n
    rows = []
    for r in range(m):
        c = np.arange(span) if r == 0 else np.arange(min(256, span)) if r == 1 else np.arange(min(257, span)) if r == 2 else np.arange(r, span, m)
        if r == 3 and n > 3:
            c = np.array([3])
        if wide and 4 <= r <= 12:
            c = np.union1d(c, np.arange(wide))
        rows.append((c.astype(np.int32), val(len(c))))
    G0 = _csr(rows, n)
    nmid = max(3, min(2 * n + 7, n // 4 + 600))
    grow, i = [], 0
    while len(grow) < nmid:
        k = min((1, 0, 2, 3, 1, 5)[i % 6], n)
        c = np.sort(rng.choice(n, k, replace=False)).astype(np.int32)
        v = val(k)
        grow.append((c, v))
        if k and i % 7 == 0:
            grow.append((c, -v))
        if k and i % 11 == 0:
            grow.append((c, v.copy()))
        i += 1
    gather = _csr(grow[:nmid], n)
    mrow = []
    for i in range(nmid):
        c = sorted({(7 * i + 3) % nmid, (13 * i + 5) % nmid})
        mrow.append((np.array(c, np.int32), val(len(c))))
    k = np.minimum(np.array((1, 2, 0, 4))[np.arange(n) % 4], nmid)
    sc = np.sort((5 * np.arange(n)[:, None] + max(1, nmid // 4) * np.arange(4)[None, :]) % nmid, axis=1)  # four distinct columns per row (nmid >= 4 wherever k = 4)
    keep = np.arange(4)[None, :] < k[:, None]
    rp = np.zeros(n + 1, np.int32)
    rp[1:] = np.cumsum(k)
    scatter = dict(nrows=n, ncols=nmid, rowptr=rp, col=sc[keep].astype(np.int32), val=val(int(k.sum())))
    x = val(n)
    return dict(name=name, n=n, m=m, G0=G0, gather=gather, middle=_csr(mrow, nmid), scatter=scatter, nmid=nmid, x=x, rho=1.75)


# ==== solve_fused restated (csrc/mpgp.hip): the phases above chained as the driver chains them ===========================================================================
def box_project(x, lb, ub):
    """k_box_project."""
    v = x.copy()
    if lb is not None:
        v = np.where(v > lb, v, lb)
    if ub is not None:
        v = np.where(v < ub, v, ub)
    return v


class ShellModel:
    """An operator that refuses mult_epi: the plain-grid kernels, k_p1_dots and a finalising launch after every reduction.  mult: the restated product."""

    def __init__(self, mult):
        self.mult = mult

    def grad_split(self, x, b, lb, ub, astol):
        g = self.mult(x) + (-1.0) * b  # k_axpy
        r = split_setp(x, g, lb, ub, astol)
        return g, r["gf"], r["p"], finalize(r["partials"], [SUM] * 4)

    def split(self, x, g, lb, ub, astol):
        """A carried gradient: k_split_setp<false> and the finalising launch."""
        r = split_setp(x, g, lb, ub, astol)
        return r["gf"], r["p"], finalize(r["partials"], [SUM] * 4)

    def p1(self, p, g, x, lb, ub):
        Ap = self.mult(p)
        return Ap, finalize(p1_dots(p, Ap, g, x, lb, ub), [SUM, SUM, MIN])

    def step(self, pAp, gp, x, g, p, Ap, lb, ub, astol, setp):
        r = step_update(gp / pAp, x, g, p, Ap, lb, ub, astol, setp)
        return r["x"], r["g"], r["gf"], r["p"], finalize(r["partials"], [SUM] * 4), r["partials"]

    def direction(self, sums, rows, pAp, gf, p):
        return dir_update(sums[0] / pAp, gf, p)

    emit = False


class ChainModel:
    """The chained staged operator: both epilogues in the chain's last kernel, every vector kernel on 1024-entry tiles, every sum finished by host_sum_row -- and the
    proportioning step and the direction forming their scalars from block partials themselves.  (What the kernels emit is what the chain would form: see
    tests/test_gpu_chain_paths.py.)"""

    emit = True

    def __init__(self, case, plan, S):
        self.case, self.plan, self.S, self.nb = case, plan, S, plan["nwg"]

    def _host(self, rows, ops):
        return np.array([host_sum_row(r, self.nb, op) for r, op in zip(rows, ops)])

    def grad_split(self, x, b, lb, ub, astol):
        o = chain_apply(self.case, self.plan, self.S, x, self.case["rho"], 2, epi=dict(b=b, lb=lb, ub=ub, astol=astol))
        return o["y"], o["gf"], o["p"], self._host(o["rows"], [SUM] * 4)

    def split(self, x, g, lb, ub, astol):
        """A carried gradient: k_split_setp<true> (it emits G0 p), its four rows finished by the host."""
        r = split_setp(x, g, lb, ub, astol, True)
        return r["gf"], r["p"], self._host(r["partials"], [SUM] * 4)

    def p1(self, p, g, x, lb, ub):
        o = chain_apply(self.case, self.plan, self.S, p, self.case["rho"], 1, epi=dict(g=g, xx=x, lb=lb, ub=ub))
        self.p1_rows = o["rows"]
        return o["y"], self._host(o["rows"], [SUM, SUM, MIN])

    def step(self, pAp, gp, x, g, p, Ap, lb, ub, astol, setp):
        # CG: the host's quotient; proportioning: the kernel's own, from the P1 block partials
        acg = sum_block_partials(self.p1_rows[1], self.nb) / sum_block_partials(self.p1_rows[0], self.nb) if setp else gp / pAp
        r = step_update(acg, x, g, p, Ap, lb, ub, astol, setp, True)
        return r["x"], r["g"], r["gf"], r["p"], self._host(r["partials"], [SUM] * 4), r["partials"]

    def direction(self, sums, rows, pAp, gf, p):
        return dir_update(sum_block_partials(rows[0], self.nb) / pAp, gf, p)


def solve_fused(model, b, x0, lb, ub, alpha, rtol=1e-5, atol=1e-50, divtol=1e4, max_it=60, gamma=1.0, astol=ASTOL, g0=None):
    """-> (step string, |gP|, |gf|, |gc| per monitor line, x, reason).  The speculative product changes no number and is left out.  g0: the gradient the caller
    carried over (pmh_mpgp_set_gradient_valid): no first product, the split kernel on it."""
    x = box_project(x0, lb, ub)
    norm_rhs = np.sqrt(finalize(grid_partials(b * b, False)[None, :], [SUM])[0])
    ttol = max(rtol * norm_rhs, atol)
    if g0 is None:
        g, gf, p, s4 = model.grad_split(x, b, lb, ub, astol)
    else:
        g = g0.copy()
        gf, p, s4 = model.split(x, g, lb, ub, astol)
    steps, mon, step, it = "", [], " ", 0
    while True:
        with np.errstate(invalid="ignore"):
            rnorm, gf2, gc2 = np.sqrt(s4[1]), s4[3], s4[2]
            steps += step
            mon.append((rnorm, np.sqrt(gf2), np.sqrt(gc2)))
        if it > max_it:
            reason = -3
        elif np.isnan(rnorm) or np.isinf(rnorm):
            reason = -9
        elif rnorm <= ttol:
            reason = 3 if rnorm < atol else 2
        elif rnorm >= divtol * norm_rhs:
            reason = -4
        else:
            reason = 0
        if reason:
            return steps, np.array(mon), x, reason
        if gc2 <= gamma * gamma * gf2:
            Ap, (pAp, gp, feas) = model.p1(p, g, x, lb, ub)
            if gp / pAp <= feas:
                step = "c"
                x, g, gf, _, s4, rows = model.step(pAp, gp, x, g, p, Ap, lb, ub, astol, False)
                p = model.direction(s4, rows, pAp, gf, p)
            else:
                step = "e"
                x = expansion_std(feas, alpha, x, g, p, Ap, lb, ub, astol)
                g, gf, p, s4 = model.grad_split(x, b, lb, ub, astol)
        else:
            step = "p"
            p = prop_dir(x, g, lb, ub, astol)
            Ap, (pAp, gp, feas) = model.p1(p, g, x, lb, ub)
            x, g, gf, p, s4, _ = model.step(pAp, gp, x, g, p, Ap, lb, ub, astol, True)
        it += 1


def tridiagonal(n):
    """A symmetric positive definite matrix of three entries per row (the ELL product: every row left to right) for the shell operator."""
    rows = []
    for i in range(n):
        c = [j for j in (i - 1, i, i + 1) if 0 <= j < n]
        rows.append((c, [2.0 + 0.01 * (i % 7) if j == i else -1.0 + 0.001 * ((i + j) % 5) for j in c]))
    return _csr(rows, n)


def csr_transpose(M):
    """Rows = the columns of M, entries by ascending row of M."""
    r = np.repeat(np.arange(M["nrows"]), np.diff(M["rowptr"]))
    o = np.argsort(M["col"], kind="stable")
    rp = np.zeros(M["ncols"] + 1, np.int32)
    rp[1:] = np.cumsum(np.bincount(M["col"], minlength=M["ncols"]))
    return dict(nrows=M["ncols"], ncols=M["nrows"], rowptr=rp, col=r[o].astype(np.int32), val=M["val"][o])


@functools.lru_cache(maxsize=None)
def solve_case(kind):
    """kind "shell": the tridiagonal matrix on 700 entries (3 workgroups of the plain grid); kind "chain": the two-tile chain case with F = gather' D gather (symmetric
    positive semidefinite, D diagonal) so that MPGP has a problem to solve.  Bounds on both sides close to the unconstrained solution's path: every step type occurs."""
    rng = np.random.default_rng(17)
    if kind == "shell":
        n, c = 700, None
    else:
        c = dict(chain_case("n1500_m6"))
        n = c["n"]
        # a gather matrix of full column rank (a diagonally dominant square block on top), then rows of 3 and 5 entries and a pair of opposite rows
        grow = [([i, (7 * i + 1) % n], [1.0 + 0.5 * rng.random(), 0.3 * rng.standard_normal()]) for i in range(n)]
        for i in range(200):
            cc = np.sort(rng.choice(n, 3 if i % 2 else 5, replace=False))
            grow.append((cc, rng.uniform(-0.5, 0.5, len(cc))))
            if i % 20 == 0:
                grow.append((cc, -grow[-1][1]))
        c.update(gather=_csr(grow, n), nmid=len(grow))
        d = rng.uniform(0.5, 1.5, c["nmid"])
        c["middle"] = _csr([([i], [d[i]]) for i in range(c["nmid"])], c["nmid"])
        c["scatter"] = csr_transpose(c["gather"])
        n = c["n"]
    b = rng.standard_normal(n)
    side = rng.random(n)  # a bound on one side at the most: a proportioning step cannot overshoot into the opposite one
    frac, far = (0.35, 0.3) if kind == "shell" else (0.1, 0.1)
    lb = np.where(side < frac, -rng.uniform(0.0, far, n), -INF)
    ub = np.where(side > 1.0 - frac, rng.uniform(0.0, far, n), INF)
    x0 = np.where(rng.random(n) < 0.5, np.where(np.isfinite(lb), lb, np.where(np.isfinite(ub), ub, 0.0)), 0.0) if kind == "chain" else np.zeros(n)  # the chain's solve starts on half of its bounds
    return dict(n=n, b=b, x0=x0, lb=lb, ub=ub, chain=c, A=tridiagonal(n) if kind == "shell" else None)


class CsrModel(ShellModel):
    """A CSR operator on the ELL plan (csrc/spmv.hip): g = A x - b in the product's SUB epilogue, and P1 in its MPGP epilogue -- workgroup w of the persistent grid of
    nl (XCD w & 7, position w >> 3 of nl / 8) takes the blocks of 256 rows b = xcd chunk + position, + nl / 8, ... below min(nrb, (xcd + 1) chunk), chunk =
    ceil(nrb / 8); thread t adds row 256 b + t of each in that order; then pmh_block_reduce and k_finalize over the nl workgroups.  The steps read their scalars on
    the device (k_step_update<false, true> under the speculative chain, else the host-scalar form): the same numbers."""

    def __init__(self, M, nl, nrb):
        super().__init__(lambda v: _rows_left_to_right(M, M["val"] * v[M["col"]]))
        self.n, self.nl, self.nrb = M["nrows"], nl, nrb

    def grad_split(self, x, b, lb, ub, astol):
        g = self.mult(x) - b
        r = split_setp(x, g, lb, ub, astol)
        return g, r["gf"], r["p"], finalize(r["partials"], [SUM] * 4)

    def _partials(self, term, op=SUM, have=None):
        ident = 0.0 if op == SUM else INF
        t, h = np.full(self.nrb * BLOCK, ident), np.zeros(self.nrb * BLOCK, bool)
        t[:self.n], h[:self.n] = term, True if have is None else have
        t, h = t.reshape(self.nrb, BLOCK), h.reshape(self.nrb, BLOCK)
        chunk, wg = (self.nrb + 7) // 8, self.nl >> 3
        acc = np.full((self.nl, BLOCK), ident)
        for w in range(self.nl):
            xcd = w & 7
            for b in range(xcd * chunk + (w >> 3), min(self.nrb, (xcd + 1) * chunk), wg):
                acc[w] = np.where(h[b], _comb(acc[w], t[b], op), acc[w])
        return block_reduce(acc, op)

    def p1_rows(self, p, Ap, g, x, lb, ub):
        q = box_feas(x, p, lb, ub)
        return np.stack([self._partials(p * Ap), self._partials(g * p), self._partials(q, MIN, np.isfinite(q) | np.isnan(q))])

    def p1(self, p, g, x, lb, ub):
        Ap = self.mult(p)
        return Ap, finalize(self.p1_rows(p, Ap, g, x, lb, ub), [SUM, SUM, MIN])


def carried_gradient(sc, g):
    """The vector the carried-gradient solves hand over: the gradient g at the starting point with every 9th entry moved by a tenth of itself -- a solve that formed
    its own gradient would take other steps from its first monitor line on."""
    g0 = g.copy()
    g0[::9] *= 1.1
    return g0
