"""Every storage, tile, epilogue and replica of the 3x3-block product k_bsr3 (csrc/bsr.hip), one launch at a time through pmh_bsr3_test_*, against the numpy
restatement of tests/bsr3_cases.py -- which tests/test_bsr3_reference_host.py ties to long-double arithmetic without a GPU.

Every comparison is exact (==, or both NaN): the library is built without contraction and the kernel sums in a fixed order.  Each case is the smallest shape at
which one part of the kernel can still be wrong, and pmh_bsr3_test_info must show that the case landed there (tiles, padding, replicas, W, scale):
ragged rows in one padded tile; more tiles than XCDs with workgroups that find no tile; a block row that fills a tile alone; a tile of 4500 scalar rows;
3 and 8 replicas with every operand different per replica; a matrix without entries; fp16 entries below half's normal range."""
import ctypes as C

import numpy as np
import pytest

import bsr3_cases as BC
import permon_amd as pa
from permon_amd._lib import check

pytestmark = pytest.mark.gpu

SENTINEL = {np.dtype(np.float64): 7.25e77, np.dtype(np.float32): -3.5e33}


@pytest.fixture(scope="module")
def ctx():
    c = pa.Context(0)
    yield c
    c.close()


class Buf:
    """Device array of any dtype (pa.Vec is fp64 only)."""

    def __init__(self, ctx, a):
        a = np.ascontiguousarray(a)
        self.ctx, self.dtype, self.n, self.p = ctx, a.dtype, a.size, C.c_void_p()
        check(ctx.L.pmh_malloc(ctx.h, max(a.nbytes, 8), C.byref(self.p)))
        self.set(a)

    def set(self, a):
        a = np.ascontiguousarray(a, self.dtype)
        assert a.size == self.n
        check(self.ctx.L.pmh_memcpy_h2d(self.ctx.h, self.p, a.ctypes.data_as(C.c_void_p), a.nbytes))

    def get(self):
        a = np.empty(self.n, self.dtype)
        check(self.ctx.L.pmh_memcpy_d2h(self.ctx.h, a.ctypes.data_as(C.c_void_p), self.p, a.nbytes))
        return a

    def free(self):
        self.ctx.L.pmh_free(self.ctx.h, self.p)


def _csr(ctx, M):
    return pa.CsrMat(ctx, M["n"], M["n"], M["rowptr"], M["col"], M["val"])


def _create(ctx, A, storage, tile, hint):
    B = C.c_void_p()
    check(ctx.L.pmh_bsr3_test_create(A.h, storage, tile, hint, C.byref(B)))
    return B if B.value else None


def _info(ctx, B):
    info, scale = (C.c_longlong * 8)(), C.c_double()
    check(ctx.L.pmh_bsr3_test_info(B, info, C.byref(scale)))
    return list(info), scale.value


def _launch(ctx, B, epi, x, y, y1=None, dinv=None, r=None, d=None, z64=None, halt=0, c=(BC.C0, BC.C1, BC.C2)):
    p = lambda v: v.p if v is not None else None  # noqa: E731
    return ctx.L.pmh_bsr3_test_mult_epi(B, epi, p(x), p(y), p(y1), p(dinv), p(r), p(d), p(z64), c[0], c[1], c[2], int(halt))


def _same(got, exp, what):
    assert got.dtype == exp.dtype and got.shape == exp.shape, what
    bad = np.flatnonzero(~((got == exp) | (np.isnan(got) & np.isnan(exp))))
    assert bad.size == 0, (what, "rows differ from the kernel-order reference", bad[:8], got[bad[:8]], exp[bad[:8]])


class Handle:
    """One (case, storage, tile) on the device with its operands and the restated results."""

    def __init__(self, ctx, name, storage, tile, hint=None):
        self.ctx, self.name, self.storage, self.tile = ctx, name, storage, tile
        M, case_hint = BC.case(name, storage)
        self.M, self.hint = M, case_hint if hint is None else hint
        self.S, self.v, self.out = BC.reference(name, storage)
        self.T = BC.arith(storage)
        self.A = _csr(ctx, M)
        self.B = _create(ctx, self.A, storage, tile, self.hint)
        assert self.B is not None, (name, storage, tile)
        self.d = {k: Buf(ctx, a) for k, a in self.v.items()}  # x, y1, r, y, dinv
        n = M["n"]
        self.sent = np.full(n, SENTINEL[np.dtype(self.T)], self.T)
        self.sent64 = np.full(n, SENTINEL[np.dtype(np.float64)])
        self.o = {k: Buf(ctx, self.sent) for k in ("y", "r", "d")}
        self.z64 = Buf(ctx, self.sent64)

    def info(self):
        info, scale = _info(self.ctx, self.B)
        print("info %-14s %-4s tile %4d: n %5d nbr %4d ntiles %2d tb %4d nrep %d nblocks %5d npad %5d W %d scale %g"
              % ((self.name, {0: "fp64", 1: "fp32", 2: "fp16"}[self.storage], self.tile) + tuple(info) + (scale,)))
        return info, scale

    def run(self, epi, z64=True, halt=0):
        """One launch on outputs pre-filled with the sentinel (POST2: y with the operand y); returns what the launch may have written."""
        d, o = self.d, self.o
        for b in o.values():
            b.set(self.sent)
        self.z64.set(self.sent64)
        if epi == BC.POST2:
            o["y"].set(self.v["y"])
            check(_launch(self.ctx, self.B, epi, d["x"], o["y"], dinv=d["dinv"], r=d["r"], z64=self.z64 if z64 else None, halt=halt))
        elif epi == BC.POST1:
            check(_launch(self.ctx, self.B, epi, d["x"], o["y"], y1=d["y1"], dinv=d["dinv"], r=o["r"], d=o["d"], halt=halt))
        else:
            check(_launch(self.ctx, self.B, epi, d["x"], o["y"], y1=d["y1"], dinv=d["dinv"], halt=halt))
        return dict(y=o["y"].get(), r=o["r"].get(), d=o["d"].get(), z64=self.z64.get())

    def close(self):
        check(self.ctx.L.pmh_bsr3_test_destroy(self.B))
        self.A.destroy()
        for b in list(self.d.values()) + list(self.o.values()) + [self.z64]:
            b.free()


def _check_all(h):
    """All six epilogues, the halt flag and a repeated launch on one handle; per replica slice where there are replicas."""
    nr, nrep = h.S["rep_rows"], h.S["nrep"]

    def same(got, exp, what):
        for q in range(nrep):  # every replica multiplied ITS slice
            _same(got[q * nr:(q + 1) * nr], exp[q * nr:(q + 1) * nr], (h.name, h.storage, h.tile, what, "replica %d" % q))

    for ename, epi in BC.EPILOGUES.items():
        exp = h.out[ename]
        got = h.run(epi)
        same(got["y"], exp["y"], ename + " y")
        same(got["r"], exp["r"] if epi == BC.POST1 else h.sent, ename + " r")
        same(got["d"], exp["d"] if epi == BC.POST1 else h.sent, ename + " d")
        same(got["z64"], exp["z64"] if epi == BC.POST2 else h.sent64, ename + " z64")
        again = h.run(epi)
        for k in got:
            assert np.array_equal(got[k], again[k], equal_nan=True), (ename, k, "two launches differ")
        halted = h.run(epi, halt=1)
        _same(halted["y"], h.v["y"] if epi == BC.POST2 else h.sent, ename + " halted y")
        _same(halted["r"], h.sent, ename + " halted r")
        _same(halted["d"], h.sent, ename + " halted d")
        _same(halted["z64"], h.sent64, ename + " halted z64")
    got = h.run(BC.POST2, z64=False)
    same(got["y"], h.out["POST2"]["y"], "POST2 without z64")
    _same(got["z64"], h.sent64, "POST2 without z64 leaves it alone")
    empty = np.repeat(np.diff(h.S["browptr"]) == 0, 3)
    if empty.any():  # empty rows: exactly 0, and the exact epilogue value of a zero sum
        y = h.run(BC.NONE)["y"]
        for q in range(nrep):
            sl = slice(q * nr, (q + 1) * nr)
            assert np.all(y[sl][empty] == 0)
            _same(h.run(BC.ADD)["y"][sl][empty], h.v["y1"][sl][empty], "ADD on empty rows")


def _check_info(h, tile):
    info, scale = h.info()
    S = BC.restate(h.M, h.storage, tile, h.hint)
    assert info == BC.info_of(S) and scale == S["scale"], (info, BC.info_of(S), scale, S["scale"])
    assert info[3] == (512 if tile == 512 else 1024) and info[7] == BC.load_width(h.storage)
    return info, scale


CASE_TILES = [(n, t) for n in BC.CASES for t in (512, 1024) if (n, t) != ("fills_1024", 512)]


@pytest.mark.parametrize("sname", list(BC.STORAGES))
@pytest.mark.parametrize("name,tile", CASE_TILES)
def test_paths(ctx, name, tile, sname):
    storage = BC.STORAGES[sname]
    h = Handle(ctx, name, storage, tile)
    info, scale = _check_info(h, tile)
    n, nbr, ntiles, tb, nrep, nblocks, npad, W = info
    if name == "ragged":
        assert (n, nbr, ntiles, nrep) == (111, 37, 1, 1) and nblocks % 2 == 1 and npad == -(-nblocks // W) * W > nblocks
    if name.startswith("many_tiles"):
        assert ntiles >= 9 and ntiles % 8 != 0  # chunk >= 2, and workgroups beyond the last tile
        assert (-(-ntiles // 8) * 8) > ntiles
    if name.startswith("fills"):
        assert nbr == 1030 and int(np.diff(h.S["browptr"]).max()) == (tb if name == "fills_%d" % tb else 512)
    if name == "many_rows":
        assert nbr == 1500 and nblocks == 1000 and ntiles == (1 if tb == 1024 else 2)
    if name == "ragged_x3":
        assert (n, nbr, nrep) == (333, 37, 3)
    if name == "many_tiles_x8":
        assert (n, nbr, nrep) == (16800, 700, 8)
    if nrep > 1:  # every operand differs from replica to replica
        for k, a in h.v.items():
            rows = a.reshape(nrep, -1)
            assert all(not np.array_equal(rows[0], rows[q]) for q in range(1, nrep)), k
    if name == "no_entries":
        assert (n, nbr, ntiles, nrep, nblocks, npad) == (9, 3, 1, 1, 0, 0) and scale == 1.0
    if storage != BC.F16:
        assert scale == 1.0
    _check_all(h)
    h.close()


@pytest.mark.parametrize("tile", [512, 1024])
def test_fp16_range(ctx, tile):
    """Entries down to 2^-30 max|v|: the host conversion must round as IEEE (numpy) does -- to nearest even, into half's subnormals, to zero below 2^-25 -- and
    the device must widen the subnormals exactly."""
    h = Handle(ctx, "fp16_range", BC.F16, tile)
    info, scale = _check_info(h, tile)
    assert scale == 1.0 and info[4] == 1
    st = np.abs(h.S["stored"].astype(np.float64))[h.S["blocks"] != 0]
    assert (st == 0).any() and ((st > 0) & (st < 2.0 ** -14)).any()
    _check_all(h)
    h.close()


@pytest.mark.parametrize("sname", list(BC.STORAGES))
def test_declines(ctx, sname):
    """No handle and no error: a block row longer than the tile, n = 0, n no multiple of 3."""
    storage = BC.STORAGES[sname]
    A = _csr(ctx, BC.case("fills_1024", storage)[0])
    assert _create(ctx, A, storage, 512, 1) is None
    A.destroy()
    A = _csr(ctx, BC.fills_tile(storage, longest=1025))
    assert _create(ctx, A, storage, 1024, 1) is None and _create(ctx, A, storage, 512, 1) is None
    A.destroy()
    for n in (0, 10):
        A = pa.CsrMat(ctx, n, n, np.zeros(n + 1, np.int32), np.zeros(0, np.int32), np.zeros(0))
        assert _create(ctx, A, storage, 1024, 1) is None
        A.destroy()


@pytest.mark.parametrize("sname", list(BC.STORAGES))
@pytest.mark.parametrize("name", ["ragged_x3", "many_tiles_x8"])
def test_replica_fallback(ctx, name, sname):
    """A hint the matrix does not bear out -- one entry of the last copy off by one bit, or a hint that does not divide n -- leaves nrep = 1 and the same product."""
    storage = BC.STORAGES[sname]
    M, hint = BC.case(name, storage)
    S, v, out = BC.reference(name, storage)
    x = Buf(ctx, v["x"])
    y = Buf(ctx, np.zeros(M["n"], BC.arith(storage)))
    for what, Mq, hq in (("hint does not divide n", M, 2 if hint == 3 else 9), ("last copy perturbed", BC.perturbed_last(M), hint)):
        A = _csr(ctx, Mq)
        B = _create(ctx, A, storage, 1024, hq)
        info, _scale = _info(ctx, B)
        Sq = BC.restate(Mq, storage, 1024, hq)
        assert info[4] == 1 and Sq["nrep"] == 1 and info == BC.info_of(Sq), (what, info)
        assert info[1] == hint * S["nbr"] and info[5] == hint * S["nblocks"]  # the whole matrix, one copy of every block
        check(_launch(ctx, B, BC.NONE, x, y))
        _same(y.get(), BC.product(Sq, v["x"]), what)
        if Mq is M:
            _same(y.get(), out["NONE"]["y"], what + ": as with replicas")
        check(ctx.L.pmh_bsr3_test_destroy(B))
        A.destroy()
    x.free()
    y.free()


@pytest.mark.parametrize("sname", list(BC.STORAGES))
def test_argument_errors(ctx, sname):
    storage = BC.STORAGES[sname]
    h = Handle(ctx, "ragged", storage, 1024)
    d, o = h.d, h.o
    L = lambda *a, **k: _launch(ctx, h.B, *a, **k)  # noqa: E731
    ARG = 2  # PMH_ERR_ARG
    try:
        check(L(BC.NONE, d["x"], o["y"]))
        o["y"].set(h.sent)
        bad = [
            L(BC.NONE, d["x"], d["x"]), L(BC.ADD, d["x"], d["x"], y1=d["y1"]), L(BC.POST2, d["x"], d["x"], dinv=d["dinv"], r=d["r"]),  # y == x
            L(BC.NONE, None, o["y"]), L(BC.NONE, d["x"], None), L(5, d["x"], o["y"]), L(3, d["x"], o["y"], y1=d["y1"]),  # no x, no y, no such epilogue
            L(BC.ADD, d["x"], o["y"]), L(BC.SUB, d["x"], o["y"], dinv=d["dinv"]),  # no y1
            L(BC.PRE, d["x"], o["y"], y1=d["y1"]), L(BC.PRE, d["x"], o["y"], dinv=d["dinv"]),
            L(BC.POST1, d["x"], o["y"], y1=d["y1"], dinv=d["dinv"], r=o["r"]), L(BC.POST1, d["x"], o["y"], y1=d["y1"], dinv=d["dinv"], d=o["d"]),
            L(BC.POST1, d["x"], o["y"], y1=d["y1"], r=o["r"], d=o["d"]), L(BC.POST1, d["x"], o["y"], dinv=d["dinv"], r=o["r"], d=o["d"]),
            L(BC.POST1, d["x"], o["y"], y1=d["y1"], dinv=d["dinv"], r=d["x"], d=o["d"]), L(BC.POST1, d["x"], o["y"], y1=d["y1"], dinv=d["dinv"], r=o["r"], d=d["x"]),
            L(BC.POST2, d["x"], o["y"], dinv=d["dinv"]), L(BC.POST2, d["x"], o["y"], r=d["r"]), L(BC.POST2, d["x"], o["y"], dinv=d["dinv"], r=d["r"], z64=d["x"]),
        ]
        assert bad == [ARG] * len(bad), bad
        assert ctx.L.pmh_bsr3_test_info(None, (C.c_longlong * 8)(), None) == ARG
        for b in o.values():  # none of them launched
            _same(b.get(), h.sent, "a refused call wrote")
    finally:
        h.close()


@pytest.mark.parametrize("name", ["ragged", "many_tiles", "ragged_x3", "many_tiles_x8"])
def test_blockdiag_mult_is_the_same_launch(ctx, name):
    """Production: MatBlockDiag.mult after enable_bsr3 (fp64 storage, tile 1024), with ONE shared device copy and with a copy per block, returns the bits of the entry's
    NONE launch -- the row sum does not depend on which tile a row falls into."""
    M, hint = BC.case(name, BC.F64)
    S, v, out = BC.reference(name, BC.F64)
    nr = M["n"] // hint
    K = pa.MatBlockDiag(ctx, np.arange(hint + 1) * nr, _csr(ctx, M))
    x, y = ctx.vec_from(v["x"]), ctx.vec_from(np.full(M["n"], 7.25e77))
    for share in (True, False):
        K.enable_bsr3(share=share)
        y.set(7.25e77)
        K.mult(x, y)
        _same(y.to_numpy(), out["NONE"]["y"], (name, "share", share))
    K.destroy()
    K.K.destroy()
