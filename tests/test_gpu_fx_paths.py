"""GPU tests of the four streaming storages of the explicit dual operator -- "full" (k_fx_gemv), "sym" (k_fx_symv, k_fx_symv_fin), "class" (k_fxs_gemm8, k_fxs_fin) and
"class_sym" (k_fxs_symm8, k_fxs_symfin) -- with their store kernels (fx_extract_row, k_fx_extract_tiled, k_fx_store_sym, k_fxs_extract_sym, k_fxs_extract_symg), against an
independent reference.  The matrices are loaded directly (MatExplicitDual.test_load_rows: the set-up's own store launches, no K^+ solve), the structure of every case is
asserted through test_info first, integer data are compared with == against an int64 product of the EFFECTIVE matrix the storage rule defines, real data component by
component against numpy.longdouble within (T + A) 2^-53 (|E| |x|)_i (tests/fx_cases.py: cases, layouts, ownership rules, references, and where T and A come from).

Per case: dense_mult == reference, two applies give the same bits, every entry off the blocks' columns (pad rows, slots without a block) is exactly zero, get_block returns the effective matrix,
the raw storage equals the packed reference with zero pads, mult equals the int64 B E B' lambda.  Stripes: every rank's share equals its own reference and the shares add up
exactly; a rank that owns nothing returns exact zeros (two launches of grid 0 were guarded for this: k_fx_symv when a rank owns no super band, k_fxs_symfin for a class B
does not touch)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import fx_cases as fc
import permon_amd as pa
from permon_amd._lib import check

pytestmark = pytest.mark.gpu

WORST = {}  # storage -> worst err / bound seen on real data (printed when the module's context closes)
_real_refs = {}  # (case, variant) -> (xs, reference, magnitude): one long-double reference per case, shared by every plan variant


@pytest.fixture(scope="module")
def ctx():
    c = pa.Context(0)
    yield c
    c.close()
    if WORST:  # for the lab notebook; every single ratio was asserted <= 1 where it was measured
        print("fx paths worst err / bound: %s" % {k: "%.3e" % v for k, v in sorted(WORST.items())})


class Operator:
    def __init__(self, ctx, d, stripe=None, symmetry=False):
        self.ctx, self.d, self.stripe = ctx, d, stripe
        self.K = pa.MatBlockDiag.from_scipy(ctx, d.block_rowstart, sp.identity(d.N, format="csr"))  # never solved with
        self.B = pa.MatGluing(ctx, d.N, d.n_lambda, d.leaf_row, d.leaf_root, d.leaf_sign)
        self.E = pa.MatExplicitDual(self.B, self.K, storage=d.storage, block_class=d.block_class if d.cls else None)
        assert list(self.E.n_gamma) == d.ngam
        if stripe is not None:
            self.E.set_stripe(*stripe)
        if d.cls:
            for u, n in enumerate(d.n_unit):
                assert np.array_equal(self.E.class_union(u), d.urel[u])
                if symmetry and n:
                    pm, sg = d.sym_group[u]
                    check(ctx.L.pmh_fexplicit_set_class_symmetry(self.E.h, u, 4, np.ascontiguousarray(pm, dtype=np.int32).ctypes.data_as(C.c_void_p),
                                                                 np.ascontiguousarray(sg, dtype=np.int8).ctypes.data_as(C.c_void_p)))
        self.units = range(len(d.n_unit))
        self.refresh()
        assert self.E.compressed_size()[0] == d.nX

    def refresh(self):
        self.info = [self.E.test_info(u) for u in self.units]

    def load(self, real=False, variant=0, mode=0, W=None):
        for u in self.units:
            if not self.d.n_unit[u]:
                continue
            if mode:
                self.E.test_load_rows(u, 0, W[u], mode=1)
                continue
            for a, b in self.d.ranges(u):
                self.E.test_load_rows(u, a, W[u][a:b] if W is not None else self.d.W_rows(u, a, b, real, variant))

    def dense(self, x):
        xv, yv = self.ctx.vec_from(x), self.ctx.vec(self.d.nX)
        self.E.dense_mult(xv, yv)
        y = yv.to_numpy()
        xv.free(), yv.free()
        return y

    def destroy(self):
        self.E.destroy(), self.B.destroy(), self.K.destroy()


def check_structure(op):
    """Layout and launch tables through test_info: what the case is meant to exercise must be there."""
    d, st = op.d, op.d.storage
    ranks = op.stripe or (0, 1)
    for u, p in enumerate(op.info):
        n = d.n_unit[u]
        assert (p["storage"], p["n"], p["ld"], p["offset"], p["woff"]) == (fc.STORAGES.index(st), n, d.ld[u], d.xoff[u], d.woff[u]), (u, p)
        own = fc.owned_rows(st, d.n_unit, u, op.stripe)
        if st == "full":
            assert p["rw"] == 4 and p["workgroups"] == sum((m + 15) // 16 for m in d.n_unit)
            continue
        width = {"sym": 128, "class": 32, "class_sym": 1024}[st]
        nbands = (d.ld[u] + width - 1) // width
        rows_own = np.zeros(nbands * width, dtype=bool)  # (padding rows follow their band: ownership is by band)
        if op.stripe is None:
            rows_own[:] = True
        elif st == "sym":
            rows_own[:] = np.repeat(fc.sym_stripe_owner(d.n_unit, ranks[1])[u] == ranks[0], width)
        elif st == "class":
            r0, r1 = fc.class_row_range(n, *ranks) if n else (0, 0)
            rows_own[r0:r1] = True
        else:
            rows_own[:] = np.repeat(fc.class_sym_owner(n, ranks[1]) == ranks[0], width) if n else False
        assert np.array_equal(rows_own[:n], own)
        assert p["bands"] == nbands and p["owned"] == [k for k in range(nbands) if rows_own[k * width]] and p["owned_bands"] == len(p["owned"])
        if st == "sym":
            seg = p["seg"]
            assert seg in (2, 4, 8, 16) and p["seg_rule"] == 2  # (no test shape comes near the 3072 workgroups that keep a longer segment)
            assert p["last_segments"] == ((nbands - 1) // seg + 1 if nbands else 0)
            nsw = 0
            for v in op.units:
                o = fc.sym_stripe_owner(d.n_unit, ranks[1])[v] == ranks[0]
                nsw += sum((sb + seg) // seg for sb in range(o.size) if o[sb])
            assert p["nsw"] == nsw and p["nfw"] == sum(ld // 128 for ld in d.ld)
        elif st == "class":
            maxrows = max((fc.class_row_range(m, *ranks)[1] - fc.class_row_range(m, *ranks)[0]) if m else 0 for m in d.n_unit)
            chunks = sum(g * (ld // 128) for g, ld in zip(d.groups, d.ld))
            nseg = max(1, min(32, (4096 + max(1, chunks) - 1) // max(1, chunks)))
            assert p["nseg"] == max(1, min(nseg, maxrows // 16)) and p["groups"] == d.groups[u]
            assert (p["r0"], p["r1"]) == (fc.class_row_range(n, *ranks) if n else (0, 0))
        else:
            assert p["super_bands"] == d.ld[u] // 256 and p["groups"] == d.groups[u] and p["items"] >= p["max_items"] >= (1 if p["owned"] else 0)
        for k, v in (d.case.expect.items() if op.stripe is None else ()):  # (the case's own structure: that of the whole operator)
            assert p[k] == v, (d.case.name, u, k, p[k])


def check_storage(op, real=False, variant=0, W=None):
    """The raw dense allocation against the packed reference, pads (and the rows of other ranks' stripes) zero."""
    d = op.d
    for u, n in enumerate(d.n_unit):
        size = fc.storage_size(d.storage, n)
        if size:
            got = op.E.test_read_storage(d.woff[u], size)
            assert np.array_equal(got, d.image(u, real, variant, op.stripe, None if W is None else W[u])), (d.case.name, u)


def check_integer(op, variant=0, W=None, full=True):
    """Every integer check of one loaded operator; returns the result of dense_mult (a stripe rank's share)."""
    d = op.d
    xs = d.X()
    x = d.scatter(xs)
    # (W given: a matrix of half-integers, (S + S') / 2 -- the reference is taken with 2 W and compared with 2 y)
    ref, _ = d.reference(xs, False, variant, op.stripe, W_override=None if W is None else [np.rint(2 * w).astype(np.int64) for w in W])
    y = op.dense(x)
    assert np.array_equal(y.view(np.int64), op.dense(x).view(np.int64))  # two applies: the same bits
    touched = d.column_mask()
    assert not np.any(y[~touched])  # padding rows and slots without a block: exactly zero
    assert np.array_equal(y * (1 if W is None else 2), ref.astype(np.float64))
    if full:
        check_storage(op, False, variant, W)
    if op.stripe is None and full:
        for b in range(d.nblocks):
            Wb, g = op.E.block(b)
            assert np.array_equal(g, d.block_rowstart[b] + d.rel[b])
            u = d.unit_of(b)
            Eb = d.block_matrix(b, False, variant) if W is None else (W[u] if d.storage == "class" else fc.effective(d.storage, W[u]))[np.ix_(d.pos[b], d.pos[b])]
            assert np.array_equal(Wb, Eb.astype(np.float64))
    if op.stripe is None:
        lam = np.random.default_rng(3).integers(1, 9, size=d.n_lambda) * np.random.default_rng(4).choice([-1, 1], size=d.n_lambda)
        lv, fv = op.ctx.vec_from(lam.astype(np.float64)), op.ctx.vec(d.n_lambda)
        op.E.mult(lv, fv)
        if W is None:
            assert np.array_equal(fv.to_numpy(), d.F_reference(lam, variant).astype(np.float64))
        lv.free(), fv.free()
    return y


def check_real(op, variant=0, label=""):
    d = op.d
    op.load(real=True, variant=variant)
    key = (d.case.name, variant)
    if key not in _real_refs:
        xs = d.X(real=True)
        _real_refs[key] = (xs,) + d.reference(xs, True, variant)
    xs, ref, mag = _real_refs[key]
    y = op.dense(d.scatter(xs))
    touched = d.column_mask()
    assert not np.any(y[~touched])
    err, bound = np.abs(y.astype(np.longdouble) - ref)[touched], d.bound(mag)[touched]  # ("class_sym": with the most items a mega band can be cut into, not the count the library reports)
    nz = bound > 0
    assert np.all(err[~nz] == 0)
    worst = float((err[nz] / bound[nz]).max()) if nz.any() else 0.0
    print("fx paths %s%s: worst err / bound %.3e" % (d.case.name, label, worst))
    WORST[d.storage] = max(WORST.get(d.storage, 0.0), worst)
    assert np.all(err <= bound)


def run_case(ctx, name, big=False):
    d = fc.data(name)
    op = Operator(ctx, d)
    try:
        print("test_info %s: %s" % (name, op.info))
        check_structure(op)
        op.load()
        op.refresh()
        check_integer(op, full=not big)
        if big:
            check_storage(op)
        check_real(op)
    finally:
        op.destroy()
        if big:
            d.drop()
    return op.info


SIMPLE = ["full_0_1_33", "full_127_128_129", "full_5_0_260", "sym_0_1_33", "sym_127_128_129", "sym_5_0_260", "sym_300", "sym_300_unsym", "class_100", "class_129",
          "class_700", "class_9_blocks", "class_two_and_untouched", "csym_100", "csym_257", "csym_257_unsym", "csym_1025", "csym_9_blocks", "csym_untouched"]


@pytest.mark.parametrize("name", SIMPLE)
def test_case(ctx, name):
    """FULL: ld = 128 / 256 / 384 (tail only, one double trip, trip plus tail), an empty block, n no multiple of 16 or 4, unsymmetric W.  SYM: the same triples; 300 = three
    super bands, two segments.  CLASS: nseg 8 / 16 / 32 (k_fxs_fin: plain loop, one unrolled trip, four; 700: segments of 24 rows), two groups, an untouched class between two
    touched ones.  CLASS_SYM: one super band; two; a second mega band of one super band (the sb < nsb guards); two groups; an untouched class in front of a touched one."""
    info = run_case(ctx, name)
    if name == "class_700":
        assert (info[0]["r1"] - info[0]["r0"]) // info[0]["nseg"] == 24
    if name == "class_9_blocks":
        assert info[0]["groups"] == 2 and fc.data(name).nblocks % 8 == 1  # the second group has one slot
    if name in ("class_two_and_untouched", "csym_untouched"):
        assert [p["n"] == 0 for p in info].count(True) == 1


def test_sym_segment_lengths(ctx):
    """n = 2177 (18 tile columns): k_fx_symv and the segment loop of k_fx_symv_fin at the segment lengths 2, 4, 8, 16 -- 9 / 5 / 3 / 2 segments in the last super band --
    give the same integers; 0 restores the rule."""
    d = fc.data("sym_2177")
    op = Operator(ctx, d)
    try:
        check_structure(op)
        op.load()
        ys = {}
        for seg, last in ((2, 9), (4, 5), (8, 3), (16, 2), (0, 9)):
            op.E.test_set_seg(seg)
            op.refresh()
            check_structure(op)
            assert (op.info[0]["seg"], op.info[0]["last_segments"]) == (seg or 2, last)
            ys[seg] = check_integer(op, full=seg == 2)
        assert all(np.array_equal(ys[2], y) for y in ys.values())
        for seg in (16, 8, 4, 2):
            op.E.test_set_seg(seg)
            check_real(op, label=" seg %d" % seg)
    finally:
        op.destroy()
        d.drop()


def test_sym_34_super_bands(ctx):
    """n = 4230: 34 super bands below the first column tile, the second trip of the q += 32 loop of k_fx_symv_fin; rows loaded in ranges."""
    info = run_case(ctx, "sym_4230", big=True)
    assert info[0]["bands"] == 34 and info[0]["owned_bands"] == 34


def test_sym_store_symmetrized(ctx):
    """k_fx_store_sym (the Dirichlet preconditioner's way in) on an unsymmetric S, FULL and SYM: the storage holds (S + S') / 2 as the rows would."""
    for name in ("sym_300_unsym", "full_127_128_129"):
        d = fc.data(name)
        op = Operator(ctx, d)
        try:
            S = [d.W(u).astype(np.float64) for u in op.units]
            op.load(mode=1, W=S)
            H = [(s + s.T) / 2 for s in S]  # halves of integers: exact
            op.refresh()
            check_integer(op, W=H)
        finally:
            op.destroy()


@pytest.mark.parametrize("name", ["sym_300", "full_5_0_260", "class_129", "csym_257"])
def test_reload(ctx, name):
    """Load, apply, load other data, apply: nothing of the first matrix or of its partial sums is left."""
    d = fc.data(name)
    op = Operator(ctx, d)
    try:
        op.load(variant=0)
        check_integer(op, variant=0)
        op.load(variant=1)
        check_integer(op, variant=1)
    finally:
        op.destroy()


STRIPES = [("sym_129_300", 2), ("sym_129_300", 3), ("sym_100_100", 8), ("class_300", 3), ("class_100", 8), ("csym_4_megabands", 2), ("csym_4_megabands", 3), ("csym_2_megabands", 8)]


@pytest.mark.parametrize("name,size", STRIPES)
def test_stripes(ctx, name, size):
    """Every stripe rank's share equals its own reference exactly (its stored rows too) and the shares add up exactly to the whole; ranks that own nothing -- six of eight
    on two blocks of one super band, on four row groups and on two mega bands -- return exact zeros without an error."""
    d = fc.data(name)
    xs = d.X()
    whole, _ = d.reference(xs)
    total, empty = np.zeros(d.nX), 0
    for r in range(size):
        op = Operator(ctx, d, stripe=(r, size))
        try:
            check_structure(op)
            op.load()
            y = check_integer(op)
            if not any(p["owned"] for p in op.info):
                empty += 1
                assert not np.any(y)
            total += y
        finally:
            op.destroy()
    assert np.array_equal(total, whole.astype(np.float64))
    if size == 8:
        assert empty == (4 if name == "class_100" else 6)
    d.drop()


@pytest.mark.parametrize("nwg", [1, 3, None])
def test_class_sym_items(ctx, monkeypatch, nwg):
    """n_c = 1300 under PMH_FXM_NWG = 1, 3 and unset: one item per mega band, a mega band cut in two, and more than 8 items per mega band (the second j += 8 trip of
    k_fxs_symfin)."""
    if nwg is None:
        monkeypatch.delenv("PMH_FXM_NWG", raising=False)
    else:
        monkeypatch.setenv("PMH_FXM_NWG", str(nwg))
    info = run_case(ctx, "csym_1300")
    p = info[0]
    if nwg == 1:
        assert (p["nwg"], p["items"], p["max_items"]) == (1, 2, 1)
    elif nwg == 3:
        # 80 steps (48 of mega band 1, then 32 of mega band 0) in shares of 26 / 27 / 27: each mega band is cut in two
        assert (p["nwg"], p["items"], p["max_items"]) == (3, 4, 2)
    else:
        assert p["max_items"] > 8


def test_class_sym_nine_mega_bands_integer(ctx):
    """n_c = 8200: 33 super bands, 9 mega bands -- the second k += 8 trip of k_fxs_symfin.  Rows generated and loaded in ranges; integer data."""
    d = fc.data("csym_8200")
    op = Operator(ctx, d)
    try:
        check_structure(op)
        assert op.info[0]["bands"] == 9 and op.info[0]["owned_bands"] == 9
        op.load()
        check_integer(op, full=False)
        check_storage(op)
    finally:
        op.destroy()
        d.drop()


def test_class_sym_nine_mega_bands_real(ctx):
    """The same on real data, within the bound."""
    d = fc.data("csym_8200")
    op = Operator(ctx, d)
    try:
        check_real(op)
    finally:
        op.destroy()
        d.drop()


def test_class_sym_symmetry_rows(ctx):
    """A class with an order-4 group of signed permutations: the representatives' rows arrive through k_fxs_extract_symg for every row of their orbits, and the stored
    image is the one loaded row by row without symmetries."""
    d = fc.data("csym_group")
    ops = Operator(ctx, d, symmetry=True), Operator(ctx, d)
    try:
        for op in ops:
            op.load()
            check_integer(op)
        n = fc.storage_size("class_sym", d.n_unit[0])
        assert np.array_equal(ops[0].E.test_read_storage(0, n), ops[1].E.test_read_storage(0, n))
        check_real(ops[0], label=" by symmetry")
    finally:
        for op in ops:
            op.destroy()


@pytest.mark.parametrize("storage", ["sym", "full"])
def test_dirichlet_blocks(ctx, storage):
    """PCDualDirichletOp on the smallest elasticity case of its own tests: block(b) is exactly symmetric (k_fx_store_sym) and the dense apply of its operator equals the
    product with what block(b) returns within the real-data bound of the storage."""
    from permon_amd.feti import DmdaFeti

    prob = DmdaFeti((8, 6, 4), 7, "elasticity")
    B = pa.MatGluing(ctx, prob.N, prob.n_lambda, prob.leaves_row, prob.leaves_root, prob.leaves_sign)
    K = pa.MatBlockDiag.from_scipy(ctx, prob.block_rowstart, prob.K)
    M = pa.PCDualDirichletOp(B, K, storage=storage, rtol=1e-12)
    try:
        e, ntot, gs = M.explicit(), C.c_int(), np.zeros(prob.nsub + 1, dtype=np.int32)
        check(ctx.L.pmh_fexplicit_compressed_size(e, C.byref(ntot), gs.ctypes.data_as(C.c_void_p)))
        rng = np.random.default_rng(5)
        x, ref, bound = np.zeros(ntot.value), np.zeros(ntot.value, dtype=np.longdouble), np.zeros(ntot.value)
        for b in range(prob.nsub):
            S, g = M.block(b)
            n = g.size
            assert np.array_equal(S, S.T)
            xb = rng.standard_normal(n)
            x[gs[b]:gs[b] + n] = xb
            ref[gs[b]:gs[b] + n] = S.astype(np.longdouble) @ xb.astype(np.longdouble)
            bound[gs[b]:gs[b] + n] = fc.bound_factor(storage, n) * fc.U53 * (np.abs(S) @ np.abs(xb))
        xv, yv = ctx.vec_from(x), ctx.vec(ntot.value)
        check(ctx.L.pmh_fexplicit_dense_mult(e, xv.p, yv.p))
        err = np.abs(yv.to_numpy().astype(np.longdouble) - ref)
        print("fx paths dirichlet %s: worst err / bound %.3e" % (storage, float((err[bound > 0] / bound[bound > 0]).max())))
        assert np.all(err <= bound)
        xv.free(), yv.free()
    finally:
        M.destroy(), B.destroy(), K.destroy()
