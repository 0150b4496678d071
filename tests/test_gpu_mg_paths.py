"""The multigrid V-cycle as an OPERATOR, one column (csrc/mg.hip) and 8 interleaved columns (csrc/mg_mv.hip), one cycle at a time through pmh_mg_test_* /
pmh_mg_mv_test_*, against the numpy restatement of tests/mg_cases.py -- which tests/test_mg_reference_host.py ties to float64 / long-double arithmetic without a GPU.

Every comparison is exact (==): the library is built without contraction and every sum of these kernels has a fixed order.  The one exception is the matrix-core
coarse solve, whose inner k order the source does not fix: dyadic data (exact in any order) pins its lane map, guards, block lookup and C layout, real data is held
to the a-priori bound gamma_{m+16} sum_j |a_j b_j| scale.  The result AND every work vector that survives a cycle are compared, one assertion per vector, so that a
failure names the stage; the info entries must show that each case reached the kernels it is named after (tests/test_mg_reference_host.py pins those plans)."""
import ctypes as C

import numpy as np
import pytest

import mg_cases as G
import mv_cases as MC
import permon_amd as pa
from permon_amd._lib import check

pytestmark = pytest.mark.gpu

ARG, SUP = 2, 4  # PMH_ERR_ARG, PMH_ERR_SUP
SENT64 = 7.25e77


@pytest.fixture(scope="module")
def ctx():
    c = pa.Context(0)
    yield c
    c.close()


def _same(got, exp, what):
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, exp.dtype, got.shape, exp.shape)
    bad = np.argwhere(~((got == exp) | (np.isnan(got) & np.isnan(exp))))
    assert bad.size == 0, (what, "%d entries differ from the kernel-order reference" % len(bad), bad[:6].tolist(), got[tuple(bad[:6].T)], exp[tuple(bad[:6].T)])


class Cycle:
    """One hierarchy on the device (pa.MG of the case's matrices under the run's knobs)."""

    def __init__(self, ctx, name, precision, degree, fused, no_bsr, monkeypatch, H=None, window=(G.LO, G.HI)):
        import scipy.sparse as sp

        monkeypatch.delenv("PMH_MG_WINDOW", raising=False)
        for key, val in (("PMH_MG_FUSED", None if fused is None else str(fused)), ("PMH_MG_NO_BSR", "1" if no_bsr else None)):
            monkeypatch.delenv(key, raising=False) if val is None else monkeypatch.setenv(key, val)
        H = G.hierarchy(name) if H is None else H
        to = lambda M: sp.csr_matrix((M["val"], M["col"], M["rowptr"]), shape=(M["nrows"], M["ncols"]))  # noqa: E731
        fine = pa.CsrMat(ctx, H["A"][0]["nrows"], H["A"][0]["ncols"], H["A"][0]["rowptr"], H["A"][0]["col"], H["A"][0]["val"])  # as given: duplicates stay
        self.ctx, self.H, self.M = ctx, H, None
        self.T = np.float64 if precision == "fp64" else np.float32
        self.rows = [a["nrows"] for a in H["A"]]
        self.mg = pa.MG(ctx, dict(H, A=[to(a) for a in H["A"]], P=[to(p) for p in H["P"]]), degree=degree, lo=window[0], hi=window[1], fine=fine, precision=precision)

    def info(self, l):
        info, scale = (C.c_longlong * 10)(), C.c_double()
        check(self.ctx.L.pmh_mg_test_info(self.mg.h, l, info, C.byref(scale)))
        return list(info), scale.value

    def apply(self, b, halt=0, x=None):
        bd = self.ctx.vec_from(np.ascontiguousarray(b, np.float64))
        xd = self.ctx.vec_from(np.full(b.shape, SENT64) if x is None else x)
        check(self.ctx.L.pmh_mg_test_apply(self.mg.h, bd.p, xd.p, int(halt)))
        out = xd.to_numpy()
        bd.free(), xd.free()
        return out

    def vector(self, l, name):
        a = np.full(self.rows[l], np.nan, self.T)
        check(self.ctx.L.pmh_mg_test_vector(self.mg.h, l, G.WHICH[name], a.ctypes.data_as(C.c_void_p)))
        return a

    # ---- 8 columns ----
    def create8(self, nrep=1):
        M = C.c_void_p()
        check(self.ctx.L.pmh_mg_mv_test_create(self.mg.h, nrep, C.byref(M)))
        self.M, self.nrep = M, nrep

    def info8(self, l):
        info = (C.c_longlong * 8)()
        check(self.ctx.L.pmh_mg_mv_test_info(self.M, l, info))
        return list(info)

    def apply8(self, b, z64=True, halt=0, z=None):
        """(fp32 result read through level 0's x, z64 or what its buffer holds afterwards)."""
        bd = self.ctx.vec_from(np.ascontiguousarray(b, np.float64).reshape(-1))
        zd = self.ctx.vec_from(np.full(b.size, SENT64) if z is None else np.ascontiguousarray(z).reshape(-1))
        check(self.ctx.L.pmh_mg_mv_test_apply(self.M, bd.p, zd.p if z64 else None, int(halt)))
        out = zd.to_numpy().reshape(b.shape)
        bd.free(), zd.free()
        return self.vector8(0, "x"), out

    def vector8(self, l, name):
        n = self.rows[l] // self.nrep
        a = np.full(n if name == "dinv" else (n, G.R), np.nan, np.float32)
        check(self.ctx.L.pmh_mg_mv_test_vector(self.M, l, G.WHICH[name], a.ctypes.data_as(C.c_void_p)))
        return a

    def close(self):
        if self.M is not None:
            check(self.ctx.L.pmh_mg_mv_test_destroy(self.M))
        self.mg.destroy()
        for a in self.mg.A + self.mg.P:
            a.destroy()


def _refused8(cy, nrep, text):
    M = C.c_void_p()
    with pytest.raises(pa.PermonHipError, match=text) as e:
        check(cy.ctx.L.pmh_mg_mv_test_create(cy.mg.h, nrep, C.byref(M)))
    assert e.value.code == SUP and not M.value


@pytest.mark.parametrize("run", G.RUNS, ids=G.run_id)
def test_cycle_equals_the_restatement(ctx, run, monkeypatch):
    """The plan, the result and every surviving work vector of one cycle: one column (columns 0 and 4 of the case's right-hand sides) and, where the 8-column form
    accepts the hierarchy, 8 columns -- with z64 and without, and single columns alone, which must reproduce their column of the full result and leave every
    other column exactly zero."""
    name, prec, degree, fused, no_bsr = run
    hy, b, one, h8, r8 = G.reference(run)
    cy = Cycle(ctx, name, prec, degree, fused, no_bsr, monkeypatch)
    try:
        for l in range(hy.nlevels):
            info, scale = cy.info(l)
            assert info == hy.info(l) and scale == hy.cp_scale, (l, info, hy.info(l), scale, hy.cp_scale)
        for r, (z, vec) in one.items():
            _same(cy.apply(b[:, r]), z, (G.run_id(run), "column", r, "result"))
            for l, v in enumerate(vec):
                for k, exp in v.items():
                    _same(cy.vector(l, k), exp, (G.run_id(run), "column", r, "level", l, k))
        if isinstance(h8, str):
            _refused8(cy, 1, h8.replace("(", r"\(").replace(")", r"\)"))
            return
        cy.create8(h8.nrep)
        for l in range(hy.nlevels):
            assert cy.info8(l) == h8.info(l), (l, cy.info8(l), h8.info(l))
        x, vec = r8
        b8 = b[:x.shape[0]]
        got, z64 = cy.apply8(b8)
        _same(got, x, (G.run_id(run), "8 columns", "result"))
        _same(z64, x.astype(np.float64), (G.run_id(run), "8 columns", "z64"))
        for l, v in enumerate(vec):
            for k, exp in v.items():
                _same(cy.vector8(l, k), exp, (G.run_id(run), "8 columns", "level", l, k))
        got, z64 = cy.apply8(b8, z64=False)  # the production call
        _same(got, x, (G.run_id(run), "8 columns without z64", "result"))
        assert np.all(z64 == SENT64)
        for r in (1, MC.ONE_SIGN_COLUMN):
            alone = np.zeros_like(b8)
            alone[:, r] = b8[:, r]
            got, _ = cy.apply8(alone)
            exp = np.zeros_like(x)
            exp[:, r] = x[:, r]
            _same(got, exp, (G.run_id(run), "column", r, "alone among 8"))
    finally:
        cy.close()


def test_dinv_rules(ctx, monkeypatch):
    """k_mg_dinv on the CSR fine operator: no stored diagonal -> 1, a stored 0.0 -> 1, the diagonal stored twice -> the last one."""
    H = G.hierarchy("diag_rules")
    hy = G.Hierarchy(H, 0, 2, None, True)
    cy = Cycle(ctx, "diag_rules", "fp64", 2, None, True, monkeypatch)
    try:
        assert cy.info(0)[0] == hy.info(0) and hy.info(0)[1] == 0
        dinv = cy.vector(0, "dinv")
        _same(dinv, hy.L[0]["dinv"], "dinv")
        assert dinv[5] == 1.0 and dinv[9] == 1.0 and dinv[14] == -0.125
    finally:
        cy.close()


def test_csr_operator_cycle_on_dyadic_data(ctx, monkeypatch):
    """Scalar CSR level operators (PMH_MG_NO_BSR), degree 1, theta = 1 and small dyadic data: every sum is exact in fp64 in any order, so the device must return
    the cycle evaluated in integer arithmetic -- the CSR-operator cycle pinned without restating which path the CSR kernel takes."""
    H = G.hierarchy("csr_dyadic")
    hy = G.Hierarchy(H, 0, 1, None, True, *G.CSR_DYADIC_WINDOW)
    cy = Cycle(ctx, "csr_dyadic", "fp64", 1, None, True, monkeypatch, window=G.CSR_DYADIC_WINDOW)
    try:
        for l in range(3):
            assert cy.info(l)[0] == hy.info(l) and hy.info(l)[1] == 0 and hy.info(l)[4] == 0
        b8 = G.rhs_dyadic("csr_dyadic", cy.rows[0])
        for r in (0, 4, 5):
            exact = G.exact_cycle_degree1(H, b8[:, r])
            assert np.array_equal(hy.apply(b8[:, r]), exact) and np.abs(exact).max() > 1
            _same(cy.apply(b8[:, r]), exact, ("csr_dyadic", "column", r, "result"))
            for l, v in enumerate(hy.vec):
                for k, exp in v.items():
                    _same(cy.vector(l, k), exp, ("csr_dyadic", "column", r, "level", l, k))
    finally:
        cy.close()


def _mfma_cycle(ctx, name, monkeypatch):
    hy = G.Hierarchy(G.hierarchy(name), 2)
    h8 = G.Hierarchy8(hy)
    cy = Cycle(ctx, name, "fp16", 2, None, False, monkeypatch)
    cy.create8()
    assert h8.coarse_kind() == G.COARSE_MFMA and cy.info8(1) == h8.info(1) and cy.info8(0) == h8.info(0) and cy.info(1)[0][7] == 1
    return hy, h8, cy


def _after_coarse(cy, h8, b, xc, tag):
    """The rest of the cycle from the device's own coarse result: everything after the matrix-core kernel is in a fixed order again."""
    x = h8.apply(b, coarse_x=xc)
    _same(cy.vector8(0, "x"), x, (tag, "result from the device's coarse solve"))
    for k in ("r", "d", "t", "xa"):
        _same(cy.vector8(0, k), h8.vec[0][k], (tag, k))


@pytest.mark.parametrize("name", list(G.MFMA_BLOCKS))
def test_mfma_coarse_solve_on_dyadic_data(ctx, name, monkeypatch):
    """Pseudo-inverse entries: integers in [-8, 8]; right-hand side: integers in [-16, 16] times the column's power of two.  Every partial sum is below 2^24 units:
    exact in fp32 in any order, so == against exact arithmetic pins the lane map, the k guards (m % 32 == 16: the last step half full), the idle wavefronts, the block
    found from row0 (two sizes) and the C layout."""
    hy, h8, cy = _mfma_cycle(ctx, name + "_dyadic", monkeypatch)
    try:
        n = hy.L[0]["n"]
        b = G.rhs_dyadic(name, n)
        cy.apply8(b, z64=False)
        bc = cy.vector8(1, "b")
        _same(bc, (-b).astype(np.float32), (name, "coarse right-hand side"))
        exact = np.concatenate([(hy.pinv_block(k).astype(np.float64) * hy.cp_scale) @ bc[hy.crs[k]:hy.crs[k + 1]].astype(np.float64) for k in range(hy.nb)])
        assert hy.cp_scale == 8.0 and np.array_equal(exact, exact.astype(np.float32).astype(np.float64)) and np.abs(exact).max() > 1000
        xc = cy.vector8(1, "x")
        _same(xc, exact.astype(np.float32), (name, "matrix-core coarse solve"))
        _after_coarse(cy, h8, b, xc, name)
    finally:
        cy.close()


@pytest.mark.parametrize("name", list(G.MFMA_BLOCKS))
def test_mfma_coarse_solve_within_the_a_priori_bound(ctx, name, monkeypatch):
    """Real data: |x - x_exact| <= gamma_{m+16} sum_j |a_j b_j| scale entry by entry, gamma_k = k u / (1 - k u), u = 2^-24: m products and the 16 wavefront
    partials in any order.  (Worst observed ratio to the bound: docs/LAB_NOTEBOOK.md.)"""
    hy, h8, cy = _mfma_cycle(ctx, name, monkeypatch)
    try:
        n = hy.L[0]["n"]
        b = G.rhs(name, n)
        cy.apply8(b, z64=False)
        bc = cy.vector8(1, "b")
        _same(bc, (-b).astype(np.float32), (name, "coarse right-hand side"))
        xc = cy.vector8(1, "x")
        worst = 0.0
        for k in range(hy.nb):
            r0, r1 = int(hy.crs[k]), int(hy.crs[k + 1])
            a, bb = hy.pinv_block(k).astype(np.float64), bc[r0:r1].astype(np.float64)
            u, kk = 2.0 ** -24, (r1 - r0) + 16
            bound = kk * u / (1 - kk * u) * (np.abs(a) @ np.abs(bb)) * hy.cp_scale
            err = np.abs(xc[r0:r1].astype(np.float64) - (a @ bb) * hy.cp_scale)
            nz = bound > 0
            assert np.all(err[~nz] == 0)
            worst = max(worst, float((err[nz] / bound[nz]).max()))
        print("mfma %s: worst error / a-priori bound = %.4f" % (name, worst))
        assert worst <= 1.0
        _after_coarse(cy, h8, b, xc, name)
    finally:
        cy.close()


@pytest.mark.parametrize("what", ["fused fp32", "unfused fp64", "8 columns"])
def test_halt_makes_every_launch_a_no_op(ctx, what, monkeypatch):
    """A first cycle fills the output and every work vector; a second one on ANOTHER right-hand side under halt = 1 must leave all of them bitwise as they were (the
    block CG relies on every launch after convergence being a no-op)."""
    prec, fused = ("fp64", 0) if what == "unfused fp64" else ("fp32", None)
    run = ("nodal3", prec, 2, fused, False)
    hy, b, one, h8, r8 = G.reference(run)
    cy = Cycle(ctx, "nodal3", prec, 2, fused, False, monkeypatch)
    try:
        if what == "8 columns":
            cy.create8()
            x, z = cy.apply8(b)
            names = [(l, k) for l, v in enumerate(r8[1]) for k in v]
            before = {lk: cy.vector8(*lk) for lk in names}
            _same(x, r8[0], "first cycle")
            x2, z2 = cy.apply8(b[:, ::-1] * 3.0, halt=1, z=z)
            _same(z2, z, "z64 under halt")
            for lk in names:
                _same(cy.vector8(*lk), before[lk], ("under halt", lk))
        else:
            z = cy.apply(b[:, 0])
            _same(z, one[0][0], "first cycle")
            names = [(l, k) for l, v in enumerate(one[0][1]) for k in v]
            before = {lk: cy.vector(*lk) for lk in names}
            assert len(names) >= 17
            _same(cy.apply(b[:, 4] * 3.0, halt=1, x=z), z, "x under halt")
            for lk in names:
                _same(cy.vector(*lk), before[lk], ("under halt", lk))
    finally:
        cy.close()


@pytest.mark.parametrize("nrep", [2, 8])
def test_congruent_blocks_equal_the_single_block(ctx, nrep, monkeypatch):
    """The 8-column cycle on the first of nrep congruent blocks returns the bits of the same cycle on that block's own hierarchy; a copy whose last coarse
    pseudo-inverse differs in one entry, or whose level-1 operator differs in one entry, is declined with the reason."""
    prec = "fp32" if nrep == 2 else "fp16"
    base = Cycle(ctx, "congruent1", prec, 2, None, False, monkeypatch)
    rep = Cycle(ctx, "congruent%d" % nrep, prec, 2, None, False, monkeypatch)
    H = G.hierarchy("congruent%d" % nrep)
    Hp = dict(H, coarse_pinv=H["coarse_pinv"].copy())
    Hp["coarse_pinv"][-1] *= 1.5
    A1 = dict(H["A"][1], val=H["A"][1]["val"].copy())
    A1["val"][-1] *= 1.5
    bad_pinv = Cycle(ctx, None, prec, 2, None, False, monkeypatch, H=Hp)
    bad_a1 = Cycle(ctx, None, prec, 2, None, False, monkeypatch, H=dict(H, A=[H["A"][0], A1, H["A"][2]]))
    try:
        base.create8(1)
        rep.create8(nrep)
        assert rep.info8(0)[:2] == [base.rows[0], nrep] and rep.info(0)[0][9] == nrep
        b = G.rhs("congruent", base.rows[0])
        x1, z1 = base.apply8(b)
        xr, zr = rep.apply8(b)
        _same(xr, x1, "result")
        _same(zr, z1, "z64")
        for l in range(3):
            for k in ("x", "b") + (("r", "d", "t", "xa") if l < 2 else ()):
                _same(rep.vector8(l, k), base.vector8(l, k), (l, k))
        _refused8(bad_pinv, nrep, "coarse pseudo-inverses of the congruent blocks differ")
        _refused8(bad_a1, nrep, "blocks are not congruent on every level")
    finally:
        for c in (base, rep, bad_pinv, bad_a1):
            c.close()


def test_refusals_and_argument_errors(ctx, monkeypatch):
    """The 8-column form declines an fp64 cycle, degree 3, PMH_MG_FUSED=0 and a one-level hierarchy with PMH_ERR_SUP and the reason; mistaken calls of the test
    entries are refused on the host with PMH_ERR_ARG."""
    for args, text in ((("nodal3", "fp64", 2, None, False), "runs in fp64"), (("nodal3", "fp32", 3, None, False), "not of degree 2"),
                       (("nodal3", "fp32", 2, 0, False), r"not the fused form \(PMH_MG_FUSED=0"), (("one_level", "fp32", 2, None, False), "has one level")):
        cy = Cycle(ctx, *args, monkeypatch)
        try:
            _refused8(cy, 1, text)
        finally:
            cy.close()
    L = ctx.L
    cy = Cycle(ctx, "nodal3", "fp32", 2, None, False, monkeypatch)
    cy64 = Cycle(ctx, "nodal3", "fp64", 2, None, False, monkeypatch)
    try:
        cy.create8()
        n = cy.rows[0]
        out = np.zeros(n * G.R, np.float64)
        p = out.ctypes.data_as(C.c_void_p)
        info, info8 = (C.c_longlong * 10)(), (C.c_longlong * 8)()
        v, w = ctx.vec(n), ctx.vec(n * G.R)
        M = C.c_void_p()
        bad = [
            L.pmh_mg_test_info(None, 0, info, None), L.pmh_mg_test_info(cy.mg.h, -1, info, None), L.pmh_mg_test_info(cy.mg.h, 4, info, None), L.pmh_mg_test_info(cy.mg.h, 0, None, None),
            L.pmh_mg_test_apply(None, v.p, w.p, 0), L.pmh_mg_test_apply(cy.mg.h, None, w.p, 0), L.pmh_mg_test_apply(cy.mg.h, v.p, None, 0), L.pmh_mg_test_apply(cy.mg.h, v.p, v.p, 0),
            L.pmh_mg_test_vector(None, 0, 0, p), L.pmh_mg_test_vector(cy.mg.h, 4, 0, p), L.pmh_mg_test_vector(cy.mg.h, 0, 7, p), L.pmh_mg_test_vector(cy.mg.h, 0, -1, p),
            L.pmh_mg_test_vector(cy.mg.h, 0, 0, None), L.pmh_mg_test_vector(cy.mg.h, 3, G.RR, p),  # the coarsest level has x and b only
            L.pmh_mg_test_vector(cy64.mg.h, 0, G.X, p), L.pmh_mg_test_vector(cy64.mg.h, 0, G.B, p),  # the caller's in fp64
            L.pmh_mg_mv_test_create(None, 1, C.byref(M)), L.pmh_mg_mv_test_create(cy.mg.h, 0, C.byref(M)), L.pmh_mg_mv_test_create(cy.mg.h, 1, None),
            L.pmh_mg_mv_test_info(None, 0, info8), L.pmh_mg_mv_test_info(cy.M, 4, info8), L.pmh_mg_mv_test_info(cy.M, 0, None),
            L.pmh_mg_mv_test_apply(None, w.p, None, 0), L.pmh_mg_mv_test_apply(cy.M, None, None, 0), L.pmh_mg_mv_test_apply(cy.M, w.p, w.p, 0),
            L.pmh_mg_mv_test_vector(None, 0, 0, p), L.pmh_mg_mv_test_vector(cy.M, -1, 0, p), L.pmh_mg_mv_test_vector(cy.M, 0, 7, p), L.pmh_mg_mv_test_vector(cy.M, 3, G.TT, p),
            L.pmh_mg_mv_test_vector(cy.M, 0, 0, None),
        ]
        assert bad == [ARG] * len(bad), bad
        assert L.pmh_mg_mv_test_destroy(None) == 0
        v.free(), w.free()
    finally:
        cy.close()
        cy64.close()
