"""Every lane map, storage, builder and epilogue of the multi-right-hand-side 3x3-block product k_mv_spmv (csrc/mv.hip), one launch at a time through
pmh_mv_test_*, against the numpy restatement of tests/mv_cases.py -- which tests/test_mv_reference_host.py ties to long-double arithmetic without a GPU.

Every comparison is exact (==, or both NaN): the library is built without contraction and the kernel sums in a fixed order.  Each case is the smallest shape at
which one part of the kernel can still be wrong, and pmh_mv_test_info must show that the case landed there (lanes per block row, W, workgroups, XCD order, scale):
one block in 16 slots; ragged rows over the trip boundaries of the 16-lane map; the XCD order with a remainder; a row of 2048 blocks; the smallest copy the plan
gives 4 lanes per block row and the largest it does not; the staged 4-lane exchange over 12 trips with a partial last workgroup, and the same with one block more
(16 lanes); prefix copies of congruent blocks; rectangular copies, plain and negated, on both lane maps; fp16 entries below half's normal range converted on
the device.  The 8 columns of every operand differ in magnitude, one is zero and one has a single sign."""
import ctypes as C

import numpy as np
import pytest

import mv_cases as MC
import permon_amd as pa
from permon_amd._lib import check

pytestmark = pytest.mark.gpu

SENTINEL = {np.dtype(np.float64): 7.25e77, np.dtype(np.float32): -3.5e33}
ARG = 2  # PMH_ERR_ARG


@pytest.fixture(scope="module")
def ctx():
    c = pa.Context(0)
    yield c
    c.close()


class Buf:
    """Device array of any dtype (pa.Vec is fp64 only)."""

    def __init__(self, ctx, a):
        a = np.ascontiguousarray(a)
        self.ctx, self.dtype, self.shape, self.n, self.p = ctx, a.dtype, a.shape, a.size, C.c_void_p()
        check(ctx.L.pmh_malloc(ctx.h, max(a.nbytes, 8), C.byref(self.p)))
        self.set(a)

    def set(self, a):
        a = np.ascontiguousarray(a, self.dtype)
        assert a.size == self.n
        check(self.ctx.L.pmh_memcpy_h2d(self.ctx.h, self.p, a.ctypes.data_as(C.c_void_p), a.nbytes))

    def get(self):
        a = np.empty(self.shape, self.dtype)
        check(self.ctx.L.pmh_memcpy_d2h(self.ctx.h, a.ctypes.data_as(C.c_void_p), self.p, a.nbytes))
        return a

    def free(self):
        self.ctx.L.pmh_free(self.ctx.h, self.p)


def _csr(ctx, M):
    return pa.CsrMat(ctx, M["nrows"], M["ncols"], M["rowptr"], M["col"], M["val"])


def _create(ctx, A, storage, kind=MC.SQUARE, nrep=1):
    E = C.c_void_p()
    check(ctx.L.pmh_mv_test_create(A.h, storage, kind, nrep, C.byref(E)))
    return E if E.value else None


def _info(ctx, E):
    info, scale = (C.c_longlong * 8)(), C.c_double()
    check(ctx.L.pmh_mv_test_info(E, info, C.byref(scale)))
    return list(info), scale.value


def _launch(ctx, E, epi, x, y, y1=None, dinv=None, r=None, d=None, z64=None, halt=0, c=(MC.C0, MC.C1, MC.C2)):
    p = lambda v: v.p if v is not None else None  # noqa: E731
    return ctx.L.pmh_mv_test_mult_epi(E, epi, p(x), p(y), p(y1), p(dinv), p(r), p(d), p(z64), c[0], c[1], c[2], int(halt))


def _same(got, exp, what):
    assert got.dtype == exp.dtype and got.shape == exp.shape, what
    bad = np.argwhere(~((got == exp) | (np.isnan(got) & np.isnan(exp))))
    assert bad.size == 0, (what, "entries (row, column) differ from the kernel-order reference", bad[:8].tolist(), got[tuple(bad[:8].T)], exp[tuple(bad[:8].T)])


class Handle:
    """One (case, storage, kind) on the device with its operands and the restated results."""

    def __init__(self, ctx, name, storage, kind):
        self.ctx, self.name, self.storage, self.kind = ctx, name, storage, kind
        self.M, self.nrep = MC.case(name, storage)
        self.S, self.v, self.out = MC.reference(name, storage, kind)
        self.T = MC.arith(storage)
        self.A = _csr(ctx, self.M)
        self.E = _create(ctx, self.A, storage, kind, self.nrep)
        assert self.E is not None, (name, storage, kind)
        self.d = {k: Buf(ctx, a) for k, a in self.v.items()}  # x, y1, r, y, dinv
        n = 3 * self.S["nbr"]
        self.sent = np.full((n, MC.R), SENTINEL[np.dtype(self.T)], self.T)
        self.sent64 = np.full((n, MC.R), SENTINEL[np.dtype(np.float64)])
        self.o = {k: Buf(ctx, self.sent) for k in ("y", "r", "d")}
        self.z64 = Buf(ctx, self.sent64)

    def info(self):
        info, scale = _info(self.ctx, self.E)
        print("info %-12s %-4s kind %d: nbr %5d nbc %5d W %4d lpr %2d storage %d workgroups %4d xcd %d kind %d scale %g"
              % ((self.name, {0: "fp64", 1: "fp32", 2: "fp16"}[self.storage], self.kind) + tuple(info) + (scale,)))
        return info, scale

    def run(self, ename, z64=True, halt=0):
        """One launch on outputs pre-filled with the sentinel (POST2: y with the operand y; ADD in place: y with y1); returns what the launch may have written."""
        d, o, epi = self.d, self.o, MC.EPILOGUES[ename.split()[0]]
        for b in o.values():
            b.set(self.sent)
        self.z64.set(self.sent64)
        L = lambda *a, **k: check(_launch(self.ctx, self.E, epi, d["x"], o["y"], *a, halt=halt, **k))  # noqa: E731
        if ename == "POST2":
            o["y"].set(self.v["y"])
            L(dinv=d["dinv"], r=d["r"], z64=self.z64 if z64 else None)
        elif ename == "POST1":
            L(y1=d["y1"], dinv=d["dinv"], r=o["r"], d=o["d"])
        elif ename == "ADD in place":
            o["y"].set(self.v["y1"])
            L(y1=o["y"])
        elif ename == "RESTRICT":
            L(dinv=d["dinv"], d=o["d"])
        elif ename == "RESTRICT y":  # without d: y alone, dinv not needed
            L()
        else:
            L(y1=d["y1"], dinv=d["dinv"])
        return dict(y=o["y"].get(), r=o["r"].get(), d=o["d"].get(), z64=self.z64.get())

    def close(self):
        check(self.ctx.L.pmh_mv_test_destroy(self.E))
        self.A.destroy()
        for b in list(self.d.values()) + list(self.o.values()) + [self.z64]:
            b.free()


def _check_all(h):
    """Every admissible epilogue, ADD in place, RESTRICT without d, POST2 without z64, the halt flag and a repeated launch on one handle."""
    names = MC.admissible(h.kind) + ["ADD in place", "RESTRICT y"]
    for ename in names:
        exp = h.out[ename.split()[0]]
        before = h.v["y"] if ename == "POST2" else h.v["y1"] if ename == "ADD in place" else h.sent
        got = h.run(ename)
        tag = (h.name, h.storage, h.kind, ename)
        _same(got["y"], exp["y"], tag + ("y",))
        _same(got["r"], exp["r"] if ename == "POST1" else h.sent, tag + ("r",))
        _same(got["d"], exp["d"] if ename in ("POST1", "RESTRICT") else h.sent, tag + ("d",))
        _same(got["z64"], exp["z64"] if ename == "POST2" else h.sent64, tag + ("z64",))
        again = h.run(ename)
        for k in got:
            assert np.array_equal(got[k], again[k], equal_nan=True), (tag, k, "two launches differ")
        halted = h.run(ename, halt=1)
        _same(halted["y"], before, tag + ("halted y",))
        _same(halted["r"], h.sent, tag + ("halted r",))
        _same(halted["d"], h.sent, tag + ("halted d",))
        _same(halted["z64"], h.sent64, tag + ("halted z64",))
    if h.kind == MC.SQUARE:
        got = h.run("POST2", z64=False)
        _same(got["y"], h.out["POST2"]["y"], "POST2 without z64")
        _same(got["z64"], h.sent64, "POST2 without z64 leaves it alone")
    empty = np.repeat(np.diff(h.S["browptr"]) == 0, 3)
    if empty.any():  # empty rows: exactly 0, and exactly y1 under ADD
        assert np.all(h.run("NONE")["y"][empty] == 0)
        _same(h.run("ADD")["y"][empty], h.v["y1"][empty], "ADD on empty rows")
        _same(h.run("ADD in place")["y"][empty], h.v["y1"][empty], "ADD in place on empty rows")


def _check_info(h):
    info, scale = h.info()
    S = MC.restate(h.M, h.storage, h.kind, h.nrep)
    assert info == MC.info_of(S) and scale == S["scale"], (info, MC.info_of(S), scale, S["scale"])
    nbr, nbc, W, lpr, nwg, xmap = MC.PLAN[h.name]
    assert (info[0], info[1], info[3], info[5], info[6]) == (nbr, nbc, lpr, nwg, xmap) and info[4] == h.storage and info[7] == h.kind and W in (None, info[2]), info
    assert (scale < 0) == (h.kind == MC.RECT_NEG and h.storage == MC.F16) and (h.storage == MC.F16 or scale == 1.0)
    return info, scale


@pytest.mark.parametrize("sname", list(MC.STORAGES))
@pytest.mark.parametrize("name", list(MC.CASES))
def test_paths(ctx, name, sname):
    storage = MC.STORAGES[sname]
    plain = None
    for kind in MC.CASES[name][0]:
        h = Handle(ctx, name, storage, kind)
        try:
            info, scale = _check_info(h)
            if h.nrep > 1:  # the prefix copy is the first block's: the plan, the operands and every result of the base case
                Sb, vb, outb = MC.reference(name.split("_x")[0], storage)
                assert info == MC.info_of(Sb) and h.M["nrows"] == h.nrep * 3 * info[0] and all(np.array_equal(h.v[k], vb[k]) for k in vb)
                assert all(np.array_equal(h.out[e][k], outb[e][k]) for e in outb for k in outb[e])
            _check_all(h)
            if kind == MC.RECT:
                plain = h.run("NONE")["y"]
            if kind == MC.RECT_NEG:  # the exact negation of the plain copy's product, in all three storages
                _same(h.run("NONE")["y"], -plain, (name, sname, "negated copy"))
                assert np.any(plain != 0)
        finally:
            h.close()


def test_fp16_range(ctx):
    """Entries down to 2^-30 max|v|: the device conversion (_Float16)(float)(v / scale) must round as IEEE (numpy) does -- to nearest even, into half's subnormals,
    to zero below 2^-25 -- and the product must widen the subnormals exactly."""
    h = Handle(ctx, "fp16_range", MC.F16, MC.SQUARE)
    try:
        info, scale = _check_info(h)
        assert scale == 1.0
        st = np.abs(h.S["stored"].astype(np.float64))[h.S["blocks"] != 0]
        assert (st == 0).any() and ((st > 0) & (st < 2.0 ** -14)).any()
        _check_all(h)
    finally:
        h.close()


def _mat(nr, nc, rowptr, col):
    return dict(nrows=nr, ncols=nc, rowptr=np.asarray(rowptr, np.int32), col=np.asarray(col, np.int32), val=np.ones(len(col)))


@pytest.mark.parametrize("sname", list(MC.STORAGES))
def test_declines(ctx, sname):
    """No handle and no error -- and the restatement declines the same matrices; their nearest neighbours are accepted."""
    storage = MC.STORAGES[sname]
    SQ, RE = MC.SQUARE, MC.RECT
    declined = [
        ("no rows", _mat(0, 0, [0], []), SQ, 1),
        ("3 does not divide the rows", _mat(4, 4, [0, 1, 1, 1, 1], [0]), SQ, 1),
        ("3 does not divide the columns", _mat(3, 4, [0, 1, 1, 1], [0]), RE, 1),
        ("a square copy of a rectangular matrix", _mat(3, 6, [0, 1, 1, 1], [0]), SQ, 1),
        ("3 nrep does not divide the rows", _mat(9, 9, [0, 1, 1, 1, 2, 2, 2, 2, 2, 2], [0, 3]), SQ, 2),
        ("nrep does not divide the entries", _mat(6, 6, [0, 2, 2, 2, 3, 3, 3], [0, 1, 3]), SQ, 2),
        ("unsorted columns", _mat(3, 3, [0, 2, 2, 2], [1, 0]), SQ, 1),
        ("unsorted block columns", _mat(6, 6, [0, 0, 2, 2, 2, 2, 2], [4, 2]), SQ, 1),
        ("repeated column", _mat(3, 3, [0, 2, 2, 2], [1, 1]), SQ, 1),
        ("no block at all", _mat(3, 3, [0, 0, 0, 0], []), SQ, 1),
        ("a block row of 2049", MC.case("w2049", storage)[0], SQ, 1),
        ("a padded copy beyond 2 GB", MC.case("cap", storage)[0], SQ, 1),
    ]
    accepted = [
        ("rectangular", _mat(3, 6, [0, 1, 1, 1], [0]), RE, 1),
        ("two congruent blocks", _mat(6, 6, [0, 1, 1, 1, 2, 2, 2], [0, 3]), SQ, 2),
        ("descending across rows", _mat(3, 3, [0, 1, 2, 2], [1, 0]), SQ, 1),
    ]
    for what, M, kind, nrep in declined + accepted:
        A = _csr(ctx, M)
        E = _create(ctx, A, storage, kind, nrep)
        S = MC.restate(M, storage, kind, nrep)
        assert (E is None) == (S is None), what
        assert (E is None) == any(what == d[0] for d in declined), what
        if E is not None:
            info, scale = _info(ctx, E)
            assert info == MC.info_of(S) and scale == S["scale"], what
            check(ctx.L.pmh_mv_test_destroy(E))
        A.destroy()


@pytest.mark.parametrize("sname", list(MC.STORAGES))
def test_argument_errors(ctx, sname):
    """A mistaken call is refused on the host: PMH_ERR_ARG, and nothing launched (the sentinels stay)."""
    storage = MC.STORAGES[sname]
    h = Handle(ctx, "ragged16", storage, MC.SQUARE)
    t = Handle(ctx, "tall", storage, MC.RECT)
    try:
        d, o = h.d, h.o
        L = lambda *a, **k: _launch(ctx, h.E, *a, **k)  # noqa: E731
        check(L(MC.NONE, d["x"], o["y"]))
        o["y"].set(h.sent)
        bad = [
            L(MC.NONE, d["x"], d["x"]), L(MC.ADD, d["x"], d["x"], y1=d["y1"]), L(MC.POST2, d["x"], d["x"], dinv=d["dinv"], r=d["r"]),  # y == x
            L(MC.RESTRICT, d["x"], d["x"]), L(MC.RESTRICT, d["x"], o["y"], dinv=d["dinv"], d=d["x"]),
            L(MC.NONE, None, o["y"]), L(MC.NONE, d["x"], None), L(5, d["x"], o["y"]), L(3, d["x"], o["y"], y1=d["y1"]), L(21, d["x"], o["y"]),  # no x, no y, no such epilogue
            L(MC.ADD, d["x"], o["y"]), L(MC.SUB, d["x"], o["y"], dinv=d["dinv"]),  # no y1
            L(MC.PRE, d["x"], o["y"], y1=d["y1"]), L(MC.PRE, d["x"], o["y"], dinv=d["dinv"]),
            L(MC.POST1, d["x"], o["y"], y1=d["y1"], dinv=d["dinv"], r=o["r"]), L(MC.POST1, d["x"], o["y"], y1=d["y1"], dinv=d["dinv"], d=o["d"]),
            L(MC.POST1, d["x"], o["y"], y1=d["y1"], r=o["r"], d=o["d"]), L(MC.POST1, d["x"], o["y"], dinv=d["dinv"], r=o["r"], d=o["d"]),
            L(MC.POST1, d["x"], o["y"], y1=d["y1"], dinv=d["dinv"], r=d["x"], d=o["d"]), L(MC.POST1, d["x"], o["y"], y1=d["y1"], dinv=d["dinv"], r=o["r"], d=d["x"]),
            L(MC.POST1, d["x"], o["y"], y1=d["y1"], dinv=d["dinv"], r=o["r"], d=o["r"]),
            L(MC.POST2, d["x"], o["y"], dinv=d["dinv"]), L(MC.POST2, d["x"], o["y"], r=d["r"]), L(MC.POST2, d["x"], o["y"], dinv=d["dinv"], r=d["r"], z64=d["x"]),
            L(MC.RESTRICT, d["x"], o["y"], d=o["d"]),  # d without dinv
        ]
        assert bad == [ARG] * len(bad), bad
        assert ctx.L.pmh_mv_test_info(None, (C.c_longlong * 8)(), None) == ARG
        for b in o.values():  # none of them launched
            _same(b.get(), h.sent, "a refused call wrote")
        # the smoothing epilogues read x at the row's own offset: refused on a rectangular copy, whose rows outnumber its columns
        Lt = lambda *a, **k: _launch(ctx, t.E, *a, **k)  # noqa: E731
        td, to = t.d, t.o
        bad = [Lt(MC.PRE, td["x"], to["y"], y1=td["y1"], dinv=td["dinv"]), Lt(MC.POST1, td["x"], to["y"], y1=td["y1"], dinv=td["dinv"], r=to["r"], d=to["d"]),
               Lt(MC.POST2, td["x"], to["y"], dinv=td["dinv"], r=td["r"])]
        assert bad == [ARG] * len(bad), bad
        for b in to.values():
            _same(b.get(), t.sent, "a refused call wrote")
        # the entry's own preconditions: a rectangular copy of congruent blocks, a kind that does not exist, a first block that is not closed
        E = C.c_void_p()
        assert ctx.L.pmh_mv_test_create(t.A.h, storage, MC.RECT, 2, C.byref(E)) == ARG and ctx.L.pmh_mv_test_create(t.A.h, storage, 3, 1, C.byref(E)) == ARG
        A = _csr(ctx, _mat(6, 6, [0, 1, 1, 1, 2, 2, 2], [3, 0]))  # block 0 reaches into block 1's columns
        assert ctx.L.pmh_mv_test_create(A.h, storage, MC.SQUARE, 2, C.byref(E)) == ARG and not E.value
        A.destroy()
    finally:
        h.close()
        t.close()


@pytest.mark.parametrize("sname", list(MC.STORAGES))
@pytest.mark.parametrize("name", ["ragged16", "quad_min"])
def test_test_spmv_is_the_same_launch(ctx, name, sname):
    """pmh_mv_test_spmv (tests/test_gpu_mv.py, the timing scripts; fp64 vectors converted on its host side) returns the bits of the entry's NONE launch."""
    storage = MC.STORAGES[sname]
    M, _ = MC.case(name, storage)
    S, v, out = MC.reference(name, storage)
    A = _csr(ctx, M)
    x, y = ctx.vec_from(v["x"].astype(np.float64).reshape(-1)), ctx.vec_from(np.full(M["nrows"] * MC.R, 7.25e77))
    check(ctx.L.pmh_mv_test_spmv(A.h, storage, x.p, y.p, 1, None))
    _same(y.to_numpy().reshape(-1, MC.R), out["NONE"]["y"].astype(np.float64), (name, sname))
    A.destroy()
    x.free()
    y.free()
