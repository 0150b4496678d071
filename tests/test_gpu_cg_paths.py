"""The block CG under the iterative K^+ -- the one-column solver of csrc/feti.hip and the 8-column solver of csrc/matinv_mv.hip -- against the numpy restatement of
tests/cg_cases.py, bit for bit: the result u and, per block or column, the iteration count, the active flag, r'z and the threshold that pmh_matinv_test_info reads back.
tests/test_cg_reference_host.py ties the restatement to long-double arithmetic without a GPU.

The matrices are the pair couplings of cg_cases.PairMatrix: every product term is exact and a row sum has at most two non-zero terms, so the product has no order and
the model's K p is scipy's; every case first asserts that premise on the device, through the product entry its solver uses.  Each shape is the smallest that reaches
what it is aimed at, and the info entry must show that it landed there (wgs, the product, the solver):
  one column    3 rows: one workgroup, most lanes idle | 1025 rows: the first wgs = 2 | {65537, 3, 1029}: wgs = 65, seg_total over two waves, workgroups without rows
                | 40 blocks, one of 65537 rows: the cap 2048 / nblocks sets wgs = 51
  3 x 3 blocks  3 rows | 1026 rows (wgs = 2)
  8 columns     3 rows | {4101, 3, 129}: wgs = 33, mvc_total's second lap
No tolerance appears below: every comparison is == (or both NaN)."""
import ctypes as C

import numpy as np
import pytest

import cg_cases as CC
import permon_amd as pa
from permon_amd._lib import check

pytestmark = pytest.mark.gpu
KEYS = ("u", "its", "active", "rz", "tol")


@pytest.fixture(scope="module")
def ctx():
    c = pa.Context(0)
    yield c
    c.close()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _read(ctx, fn, h, entries):
    info, scal, ints = (C.c_longlong * 8)(), np.zeros(2 * entries), np.zeros(2 * entries, np.int32)
    check(fn(h, info, entries, _p(scal), _p(ints)))
    assert info[5] == entries
    return dict(wgs=info[0], product=info[1], solver=info[2], nactive=info[3], done=info[4], last=info[6], rz=scal[0::2].copy(), tol=scal[1::2].copy(),
                active=ints[0::2].astype(int), its=ints[1::2].astype(int))


def _premise(ctx, A, path, K):
    """The device's K p for a random p is scipy's, entry for entry, through the product the solver uses."""
    rng = np.random.default_rng(1)
    if path == CC.ELL8:
        X = rng.standard_normal((A.n, 8)) * CC.SCALES[None, :]
        y = ctx.vec(A.n * 8)
        check(ctx.L.pmh_mv_test_spmv(K.K.h, 0, ctx.vec_from(X.reshape(-1)).p, y.p, 1, None))
        assert np.array_equal(y.to_numpy().reshape(A.n, 8), A.K @ X)
        return
    x = rng.standard_normal(A.n)
    y = ctx.vec(A.n)
    if path == CC.BSR3:
        Kb = pa.MatBlockDiag.from_scipy(ctx, A.rs.astype(np.int32), A.K)
        Kb.enable_bsr3()
        Kb.mult(ctx.vec_from(x), y)
        ctx.sync()
        Kb.destroy()
    else:
        K.mult(ctx.vec_from(x), y)
    assert np.array_equal(y.to_numpy(), A.K @ x)


class Solver:
    """A fresh K^+ on the pair matrix A.  path: CC.CSR / CC.BSR3 (pmh_matinv_mult) or CC.ELL8 (the 8-column solver, its handle kept: pmh_matinv_test_mv_*)."""

    def __init__(self, ctx, A, path, jacobi, aimed_wgs, rtol=1e-10, atol=1e-50, max_it=10000, R=None, kernel_tol=None, fix=None):
        self.ctx, self.A, self.path, self.jacobi, self.R, self.fix = ctx, A, path, jacobi, R, fix
        self.opts = dict(rtol=rtol, atol=atol, max_it=max_it, kernel_tol=64.0 if kernel_tol is None else kernel_tol)
        self.K = pa.MatBlockDiag.from_scipy(ctx, A.rs.astype(np.int32), A.K)
        _premise(ctx, A, path, self.K)
        self.M = pa.MatInv(self.K, rtol=rtol, atol=atol, max_it=max_it, jacobi=jacobi, nullspace=R)
        if path == CC.BSR3:
            self.M.enable_bsr3()
        if kernel_tol is not None:
            check(ctx.L.pmh_matinv_set_kernel_load_tolerance(self.M.h, float(kernel_tol)))
        if fix is not None:
            self.M.set_left_inverse(fix)
        self.V = C.c_void_p()
        if path == CC.ELL8:
            check(ctx.L.pmh_matinv_test_mv_create(self.M.h, C.byref(self.V)))
        self.aimed = (aimed_wgs, path, CC.EIGHT if path == CC.ELL8 else CC.ONE)

    def set_tolerances(self, rtol, atol=1e-50, max_it=10000):
        self.M.set_tolerances(rtol, atol, max_it)
        self.opts.update(rtol=rtol, atol=atol, max_it=max_it)

    def apply(self, f):
        """-> the device's result and state; asserts where the case landed."""
        ctx, A = self.ctx, self.A
        nb = len(A.rs) - 1
        u = ctx.vec(f.size)
        if self.path == CC.ELL8:
            check(ctx.L.pmh_matinv_test_mv_mult(self.V, ctx.vec_from(f.reshape(-1)).p, u.p))
            d = _read(ctx, ctx.L.pmh_matinv_test_mv_info, self.V, 8 * nb)
            d["u"] = u.to_numpy().reshape(A.n, 8)
        else:
            self.M.mult(ctx.vec_from(f), u)
            d = _read(ctx, ctx.L.pmh_matinv_test_info, self.M.h, nb)
            d["u"] = u.to_numpy()
        assert (d["wgs"], d["product"], d["solver"]) == self.aimed, "the case did not land where it was aimed"
        return d

    def model(self, f, **kw):
        A, o = self.A, dict(self.opts, **kw)
        K = lambda p: A.K @ p  # noqa: E731
        if self.path == CC.ELL8:
            return CC.solve_eight(K, A.rs, f, dinv=A.dinv(self.jacobi), R=self.R, wgs=self.aimed[0], **o)
        return CC.solve_one(K, A.rs, f, dinv=A.dinv(self.jacobi), R=self.R, fix=self.fix, wgs=self.aimed[0], **o)

    def close(self):
        if self.V:
            check(self.ctx.L.pmh_matinv_test_mv_destroy(self.V))
        self.M.destroy()
        self.K.destroy()


def _same(dev, ref, what=""):
    for k in KEYS:
        assert np.array_equal(dev[k], ref[k], equal_nan=k in ("u", "rz", "tol")), (what, k, dev[k], ref[k])
    assert (dev["nactive"], dev["done"]) == (ref["nactive"], ref["done"]), what


def _shape(path, name):
    sizes, wgs = {CC.CSR: CC.SHAPES_ONE, CC.BSR3: CC.SHAPES_BSR3, CC.ELL8: CC.SHAPES_EIGHT}[path][name]
    return {CC.CSR: "", CC.BSR3: "3:", CC.ELL8: "8:"}[path] + name, wgs


def _fresh(ctx, path, name, jacobi, f, unit_lone=False, singular=False, **kw):
    """One application on a fresh handle -> (device, model)."""
    shape, wgs = _shape(path, name)
    s = Solver(ctx, CC.matrix(shape, unit_lone=unit_lone, singular=singular), path, jacobi, wgs, **kw)
    try:
        return s.apply(f), s.model(f)
    finally:
        s.close()


# ---- every shape, rtol alone ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jacobi", [True, False], ids=["jacobi", "none"])
@pytest.mark.parametrize("path,name", [(CC.CSR, n) for n in CC.SHAPES_ONE] + [(CC.BSR3, n) for n in CC.SHAPES_BSR3], ids=lambda v: {0: "csr", 1: "bsr3"}.get(v, v))
def test_one_column(ctx, path, name, jacobi):
    """Blocks that stop at different iterations (staggered loads), then a random load scaled 1e-3 .. 1e3 block by block (Jacobi: 6-7 steps; none: ~30)."""
    A = CC.matrix(_shape(path, name)[0])
    for i, f in enumerate((CC.staggered_load(A, jacobi, 9), CC.random_load(A, 3))):
        dev, ref = _fresh(ctx, path, name, jacobi, f)
        _same(dev, ref, i)
        assert dev["done"] == 1 and dev["its"].max() > 0


@pytest.mark.parametrize("kind", ["staggered", "sign"])
@pytest.mark.parametrize("jacobi", [True, False], ids=["jacobi", "none"])
@pytest.mark.parametrize("name", list(CC.SHAPES_EIGHT))
def test_eight_columns(ctx, name, jacobi, kind):
    """Columns that stop at different iterations, a zero column, columns of 1e-3 .. 1e3; kind sign: one column with a single sign."""
    A = CC.matrix(_shape(CC.ELL8, name)[0])
    dev, ref = _fresh(ctx, CC.ELL8, name, jacobi, CC.columns(A, jacobi, 4, kind))
    _same(dev, ref)
    assert dev["done"] == 1 and np.all(dev["u"][:, 6] == 0.0)


# ---- iterate by iterate: alpha_k and p_k, hence beta_(k-1), one at a time -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kdim", [0, 1])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("path,name", [(CC.CSR, "b65537"), (CC.BSR3, "b1026"), (CC.ELL8, "b4101")], ids=lambda v: {0: "csr", 1: "bsr3", 2: "ell8"}.get(v, v))
def test_iterate_by_iterate(ctx, path, name, k, kdim):
    """max_it = k on a fresh handle: u is the model's k-th iterate (projected where R is set), its = k for what is still active and the model's smaller count for the rest."""
    A = CC.matrix(_shape(path, name)[0])
    R = CC.kernel_basis(A.rs, kdim) if kdim else None
    if path == CC.ELL8:  # odd columns: long runs; even columns stop after 1, 3, 5 steps (column 6: zero)
        f = CC.columns(A, False, 4) + 0.125 * CC.columns(A, False, 5, "random") * (np.arange(8) % 2)
    else:  # block 2 (where there is one) stops after 3 steps, the others run on
        f = CC.staggered_load(A, False, 9) + (A.block != 2) * CC.random_load(A, 3)
    dev, ref = _fresh(ctx, path, name, False, f, max_it=k, R=R)
    _same(dev, ref, k)
    assert dev["its"].max() == k and dev["done"] == 1  # (the cut at max_it freezes every block: nactive = 0)


# ---- stopping -------------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,name", [(CC.CSR, "b40"), (CC.ELL8, "b4101")], ids=lambda v: {0: "csr", 2: "ell8"}.get(v, v))
def test_atol(ctx, path, name):
    """The atol branch of the threshold: blocks / columns below atol from the start, and ones atol stops before rtol would (tests/test_cg_reference_host.py::test_atol_case)."""
    c = CC.ATOL_CASE
    A = CC.matrix(_shape(path, name)[0])
    if path == CC.ELL8:
        f = np.random.default_rng(12).standard_normal((A.n, 8)) * c["scales"][None, :]
    else:
        f = np.random.default_rng(13).standard_normal(A.n) * c["scales"][A.block % 8]
    dev, ref = _fresh(ctx, path, name, False, f, rtol=c["rtol"], atol=c["atol"])
    _same(dev, ref)
    assert np.any(dev["its"] == 0) and np.any(dev["tol"] == c["atol"]) and np.any(dev["tol"] > c["atol"])


@pytest.mark.parametrize("path,name", [(CC.CSR, "b65537"), (CC.ELL8, "b4101")], ids=lambda v: {0: "csr", 2: "ell8"}.get(v, v))
def test_nan_in_one_load(ctx, path, name):
    """A NaN in one block's / column's load: it takes the model's exit (r'r is NaN: never active, u = 0), everything else has the bits of the run without the NaN."""
    A = CC.matrix(_shape(path, name)[0])
    f = CC.columns(A, True, 4) if path == CC.ELL8 else CC.random_load(A, 3)
    clean, _ = _fresh(ctx, path, name, True, f)
    g = f.copy()
    if path == CC.ELL8:
        g[A.rs[0] + 5, 2] = np.nan  # column 2 of block 0
        hit = np.zeros(clean["its"].size, bool)
        hit[2] = True
        rows = np.zeros_like(f, bool)
        rows[A.rs[0]:A.rs[1], 2] = True
    else:
        g[A.rs[2] + 5] = np.nan  # block 2
        hit = np.arange(3) == 2
        rows = A.block == 2
    dev, ref = _fresh(ctx, path, name, True, g)
    _same(dev, ref)
    assert np.all(dev["its"][hit] == 0) and np.all(dev["active"] == 0) and np.all(np.isnan(dev["rz"][hit])) and np.all(dev["u"][rows] == 0.0)
    for k in KEYS:
        assert np.array_equal(dev[k][~(rows if k == "u" else hit)], clean[k][~(rows if k == "u" else hit)]), k


@pytest.mark.parametrize("jacobi", [True, False], ids=["jacobi", "none"])
@pytest.mark.parametrize("path,name", [(CC.CSR, "b65537"), (CC.ELL8, "b4101")], ids=lambda v: {0: "csr", 2: "ell8"}.get(v, v))
def test_nan_exit_of_the_iteration(ctx, path, name, jacobi):
    """The rr != rr exit: the last block's load (column 4 of it) lies in the kernel of a singular pair, p'K p = 0 exactly, alpha = inf, r = NaN after one step; the block
    leaves with its = 1 and everything else runs on to its own end."""
    A = CC.matrix(_shape(path, name)[0], singular=True)
    last = len(A.rs) - 2
    rows = A.block == last
    if path == CC.ELL8:
        f = CC.columns(A, jacobi, 4)
        f[rows] = 0.0  # (the other columns of the singular block stay out of it: CG on an inconsistent singular system has no end to pin)
        f[rows, 4] = CC.breakdown_load(A, 0.75)[rows]
        e = 8 * last + 4
    else:
        f = np.where(rows, CC.breakdown_load(A, 0.75), CC.random_load(A, 3))
        e = last
    dev, ref = _fresh(ctx, path, name, jacobi, f, singular=True)
    _same(dev, ref)
    assert dev["its"][e] == 1 and np.isnan(dev["rz"][e]) and dev["done"] == 1 and dev["its"].max() > 1


# ---- projection -----------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kdim", [1, 6, 8])
@pytest.mark.parametrize("path,name", [(CC.CSR, "b65537"), (CC.ELL8, "b4101")], ids=lambda v: {0: "csr", 2: "ell8"}.get(v, v))
def test_projection(ctx, path, name, kdim):
    """K^+ = P_R K^-1 P_R with kdim columns of exactly representable entries, block-wise orthonormal and zero for block 1 (P_R is applied whatever R is; K is non-singular)."""
    A = CC.matrix(_shape(path, name)[0])
    R = CC.kernel_basis(A.rs, kdim, zero_block=1)
    f = CC.columns(A, True, 4, "random") if path == CC.ELL8 else CC.random_load(A, 3)
    dev, ref = _fresh(ctx, path, name, True, f, R=R)
    _same(dev, ref)


@pytest.mark.parametrize("ratio,kernel_tol,iterates", [(CC.INSIDE, None, False), (CC.OUTSIDE, None, True), (CC.INSIDE, 0.0, True)], ids=["inside", "outside", "inside-rule-off"])
@pytest.mark.parametrize("path,name", [(CC.CSR, "b65537"), (CC.ELL8, "b4101")], ids=lambda v: {0: "csr", 2: "ell8"}.get(v, v))
def test_kernel_load_rule(ctx, path, name, ratio, kernel_tol, iterates):
    """|P_R f| <= 64 eps |f|: the load counts as lying in the kernel (u = 0, never active).  The largest block's load has |P_R f| / (eps |f|) = 16 (inside) or 1024 (outside);
    with the rule switched off the inside load iterates as the model does."""
    A = CC.matrix(_shape(path, name)[0])
    R = CC.kernel_basis(A.rs, 1)
    b = int(np.argmax(np.diff(A.rs)))
    f = CC.columns(A, True, 4, "random") if path == CC.ELL8 else CC.random_load(A, 3)
    load = CC.kernel_load(R, A.rs, b, ratio)
    if path == CC.ELL8:
        f[A.rs[b]:A.rs[b + 1], 1] = load
        e = 8 * b + 1
    else:
        f[A.rs[b]:A.rs[b + 1]] = load
        e = b
    dev, ref = _fresh(ctx, path, name, True, f, R=R, kernel_tol=kernel_tol)
    _same(dev, ref)
    assert (dev["its"][e] > 0) == iterates


def test_left_inverse(ctx):
    """K^+ = K^- P_R with two fixing dofs (identity rows of K): their entries of u are exactly 0, and u is not projected."""
    A = CC.matrix("b65537", unit_lone=True)
    fix = A.lone[:2]
    assert np.all(A.d[fix] == 1.0)
    dev, ref = _fresh(ctx, CC.CSR, "b65537", True, CC.random_load(A, 3), unit_lone=True, R=CC.kernel_basis(A.rs, 1), fix=fix)
    _same(dev, ref)
    assert np.all(dev["u"][fix] == 0.0)


# ---- reuse of a handle ----------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,name", [(CC.CSR, "b65537"), (CC.BSR3, "b1026"), (CC.ELL8, "b4101")], ids=lambda v: {0: "csr", 1: "bsr3", 2: "ell8"}.get(v, v))
def test_reuse_of_a_handle(ctx, path, name):
    """The load with the most iterations, then the one with the fewest, then the first again, on ONE handle: the previous count steers where the host looks at the device, so
    the second application enqueues ~30 iterations past `done` -- products, dots, updates -- and none of them may change a bit; the third starts from the small estimate.
    set_tolerances in between resets the estimate.  Every result equals the model, i.e. a fresh handle's."""
    shape, wgs = _shape(path, name)
    A = CC.matrix(shape)
    if path == CC.ELL8:
        long_, short = CC.columns(A, False, 5, "random"), CC.columns(A, False, 4)[:, [0] * 8] * CC.SCALES[None, :]
    else:
        long_, short = CC.random_load(A, 3), A.eigen_load(np.random.default_rng(2), False, [1] * (len(A.rs) - 1))
    s = Solver(ctx, A, path, False, wgs)
    try:
        ref_long, ref_short = s.model(long_), s.model(short)
        assert ref_long["its"].max() >= 25 and ref_short["its"].max() == 1
        for what, f, ref in (("long", long_, ref_long), ("short", short, ref_short), ("long again", long_, ref_long)):
            dev = s.apply(f)
            _same(dev, ref, what)
            assert dev["last"] == ref["its"].max()
        s.apply(long_)
        s.set_tolerances(1e-6)
        _same(s.apply(short), s.model(short), "after set_tolerances")
        _same(s.apply(long_), s.model(long_), "after set_tolerances, long")
    finally:
        s.close()
    fresh, _ = _fresh(ctx, path, name, False, short)
    _same(fresh, ref_short, "fresh")


# ---- with a V-cycle ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# Real stiffness matrices: the smallest boxes set_pc_mg_box accepts (cubes of nel = 4, min_nodes = 27; 375 rows a block, not a multiple of 32).  The model's K is the pinned
# restatement of the product (bsr3_cases.product for the one-column solver on its 3 x 3-block copy, mv_cases.product for the 8-column ELL copy).  The model's V-cycle is the
# device's own single-launch entry under halt = 0 (pmh_mg_test_apply, pmh_mg_mv_test_apply; tests/test_gpu_mg_paths.py pins them to mg_cases): the box hierarchy is built
# inside the library, so mg_cases, which needs the transfer matrices, cannot build it.
def _cube(sub):
    from permon_amd.feti import CubeFeti

    f = CubeFeti(sub, 4, "elasticity", contact=False)
    K = f.K.tocsr()
    K.sort_indices()
    rhs = np.random.default_rng(6).standard_normal(f.N) * np.repeat(CC.SCALES[:f.nsub], f.n_i)
    return f, K, rhs


def _with_box_cycle(ctx, f, Ksp, prec, bsr3):
    K = pa.MatBlockDiag.from_scipy(ctx, f.block_rowstart, Ksp)
    M = pa.MatInv(K, rtol=1e-10, nullspace=f.R)
    if bsr3:
        M.enable_bsr3()
    nn = f.nel + 1
    mg = M.set_pc_mg_box(Ksp, [(nn, nn, nn)] * f.nsub, 3, R=f.R, min_nodes=27, degree=2, precision=prec)
    return K, M, mg


@pytest.mark.parametrize("fusion", [1, 0], ids=["d0-fused", "d0-apart"])
@pytest.mark.parametrize("prec", ["fp32", "fp64"])
def test_one_column_with_v_cycle(ctx, prec, fusion):
    """pmh_matinv_mult on two cubes with the box V-cycle, fp32 and fp64, the first smoothing direction written by k_cg_update_ur (knob mg_d0_fusion = 1) or by the cycle
    (0): both equal the model, hence each other.  K: bsr3_cases.product; V-cycle: pmh_mg_test_apply, halt = 0 (see above)."""
    import bsr3_cases as BC

    f, Ksp, rhs = _cube((2, 1, 1))
    K, M, mg = _with_box_cycle(ctx, f, Ksp, prec, True)
    S = BC.restate(dict(n=f.N, rowptr=Ksp.indptr, col=Ksp.indices, val=Ksp.data), BC.F64, 0, f.nsub)

    def pc(r):
        z = ctx.vec(f.N)
        check(ctx.L.pmh_mg_test_apply(mg.h, ctx.vec_from(r).p, z.p, 0))
        return z.to_numpy()

    u = ctx.vec(f.N)
    try:
        check(ctx.L.pmh_set_knob(b"mg_d0_fusion", fusion))
        M.mult(ctx.vec_from(rhs), u)
        dev = _read(ctx, ctx.L.pmh_matinv_test_info, M.h, f.nsub)
    finally:
        ctx.L.pmh_set_knob(b"mg_d0_fusion", 1)
    dev["u"] = u.to_numpy()
    assert (dev["wgs"], dev["product"], dev["solver"]) == (1, CC.BSR3, CC.ONE)
    ref = CC.solve_one(lambda p: BC.product(S, p), f.block_rowstart, rhs, pc=pc, rtol=1e-10, R=f.R, wgs=1)
    _same(dev, ref)
    assert dev["done"] == 1 and 3 < dev["its"].max() < 40
    M.destroy()
    K.destroy()


def _mv_cycle(ctx, mg, nrep, n):
    E = C.c_void_p()
    check(ctx.L.pmh_mg_mv_test_create(mg.h, nrep, C.byref(E)))

    def pc(r):
        z = ctx.vec(n * 8)
        check(ctx.L.pmh_mg_mv_test_apply(E, ctx.vec_from(r.reshape(-1)).p, z.p, 0))
        return z.to_numpy().reshape(n, 8)

    return E, pc


def test_eight_columns_with_v_cycle(ctx):
    """The 8-column solver on two cubes with the fused fp32 cycle.  K: mv_cases.product; V-cycle: pmh_mg_mv_test_apply, halt = 0 (see above)."""
    import bsr3_cases as BC
    import mv_cases as MC

    f, Ksp, _ = _cube((2, 1, 1))
    K, M, mg = _with_box_cycle(ctx, f, Ksp, "fp32", False)
    S = MC.restate(dict(nrows=f.N, ncols=f.N, rowptr=Ksp.indptr, col=Ksp.indices, val=Ksp.data), BC.F64, MC.SQUARE, 1)
    F = np.random.default_rng(7).standard_normal((f.N, 8)) * CC.SCALES[None, :]
    F[:, 3] = 0.0
    V = C.c_void_p()
    check(ctx.L.pmh_matinv_test_mv_create(M.h, C.byref(V)))
    E, pc = _mv_cycle(ctx, mg, 1, f.N)
    u = ctx.vec(f.N * 8)
    check(ctx.L.pmh_matinv_test_mv_mult(V, ctx.vec_from(F.reshape(-1)).p, u.p))
    dev = _read(ctx, ctx.L.pmh_matinv_test_mv_info, V, 8 * f.nsub)
    dev["u"] = u.to_numpy().reshape(f.N, 8)
    assert (dev["wgs"], dev["product"], dev["solver"]) == (3, CC.ELL8, CC.EIGHT)
    ref = CC.solve_eight(lambda p: MC.product(S, p), f.block_rowstart, F, pc=pc, rtol=1e-10, R=f.R, wgs=3)
    _same(dev, ref)
    assert dev["done"] == 1 and 3 < dev["its"].max() < 40 and np.all(dev["its"][3::8] == 0)
    check(ctx.L.pmh_mg_mv_test_destroy(E))
    check(ctx.L.pmh_matinv_test_mv_destroy(V))
    M.destroy()
    K.destroy()


def test_eight_congruent_blocks_as_columns(ctx):
    """pmh_matinv_mult on the 8 congruent cubes of a 2 x 2 x 2 decomposition (knob kplus_mv = 1): block b is column b of the 8-column model on ONE block of 375 rows, with
    block 0's kernel basis.  Pins k_mvc_from_columns and k_mvc_columns too, on a row count that is no multiple of 32.  K, V-cycle: as above, nrep = 8."""
    import bsr3_cases as BC
    import mv_cases as MC

    f, Ksp, rhs = _cube((2, 2, 2))
    n = f.n_i
    K, M, mg = _with_box_cycle(ctx, f, Ksp, "fp32", True)
    assert M.multi_rhs_active()
    S = MC.restate(dict(nrows=f.N, ncols=f.N, rowptr=Ksp.indptr, col=Ksp.indices, val=Ksp.data), BC.F64, MC.SQUARE, 8)
    E, pc = _mv_cycle(ctx, mg, 8, n)
    u = ctx.vec(f.N)
    M.mult(ctx.vec_from(rhs), u)
    dev = _read(ctx, ctx.L.pmh_matinv_test_info, M.h, 8)
    dev["u"] = u.to_numpy().reshape(8, n).T
    assert (dev["wgs"], dev["product"], dev["solver"]) == (3, CC.ELL8, CC.CONGRUENT)
    ref = CC.solve_eight(lambda p: MC.product(S, p), [0, n], np.ascontiguousarray(rhs.reshape(8, n).T), pc=pc, rtol=1e-10, R=f.R[:, :n], wgs=3)
    _same(dev, ref)
    assert dev["done"] == 1 and 3 < dev["its"].max() < 40
    check(ctx.L.pmh_mg_mv_test_destroy(E))
    M.destroy()
    K.destroy()
