"""The numpy restatement of the 3x3-block kernel (tests/bsr3_cases.py) IS the operation: without a GPU, every case and storage of
tests/test_gpu_bsr3_paths.py is checked against long-double arithmetic on the stored (rounded) entries, so the GPU test cannot pass only by agreeing with itself.

Bounds (u: unit roundoff of the arithmetic type, 2^-53 or 2^-24):
* plain product, per scalar row of nb blocks: |s - sum_j a_ij x_j| <= (3 nb + 2) u sum_j |a_ij x_j| -- 3 nb products (one rounding each) added in some order
  by 3 nb - 1 additions, each term passing through at most ceil(nb / 4) + 3 of them; 3 nb + 2 covers every order the lanes could use and the second-order terms;
* epilogues, from the restated s: k u (sum of the absolute values of the formula's terms), k the roundings the longest chain of the formula carries plus one:
  ADD / SUB 2, PRE 5, POST1 r 3, d 4, y 5, POST2 6; z64 is the exact widening of y."""
import numpy as np
import pytest
import scipy.sparse as sp

import bsr3_cases as BC

LD = np.longdouble
NAMES = list(BC.CASES)
PAIRS = [(n, s) for n in NAMES for s in BC.STORAGES] + [("fp16_range", "fp16")]
_worst = {}


def _ratio(tag, err, bound):
    """Every row within its bound (0 <= 0 included); remembers and prints the worst err / bound."""
    bad = np.flatnonzero(~(err <= bound))
    assert bad.size == 0, (tag, bad[:8], err[bad[:8]], bound[bad[:8]])
    nz = bound > 0
    w = float(np.max(err[nz] / bound[nz])) if nz.any() else 0.0
    _worst[tag] = max(_worst.get(tag, 0.0), w)
    print("%-40s worst err / bound = %.3f" % (tag, w))
    return w


def _stored_csr(S):
    """The stored entries of one replica as a scalar CSR in long double (fp16 storage: times the scale, exact) -- blocks' absent entries are explicit zeros."""
    n, nb = S["rep_rows"], S["nblocks"]
    a = S["stored"].astype(LD) * LD(S["scale"])
    brow = np.repeat(np.arange(S["nbr"]), np.diff(S["browptr"]))
    rows = (3 * brow[:, None, None] + np.arange(3)[None, :, None]) + np.zeros((nb, 3, 3), np.int64)
    cols = (3 * S["bcol"].astype(np.int64)[:, None, None] + np.arange(3)[None, None, :]) + np.zeros((nb, 3, 3), np.int64)
    return n, rows.ravel(), cols.ravel(), a.ravel()


@pytest.mark.parametrize("name,sname", PAIRS)
def test_product_against_long_double(name, sname):
    storage = BC.STORAGES[sname]
    S, v, out = BC.reference(name, storage)
    u, nr = BC.UNIT[storage], S["rep_rows"]
    n, rows, cols, a = _stored_csr(S)
    nb_row = np.repeat(np.diff(S["browptr"]), 3)
    s = out["NONE"]["y"]
    assert s.dtype == BC.arith(storage) and s.shape == (S["n"],)
    for q in range(S["nrep"]):
        xq = v["x"][q * nr:(q + 1) * nr].astype(LD)
        exact, ab = np.zeros(n, LD), np.zeros(n, LD)
        np.add.at(exact, rows, a * xq[cols])
        np.add.at(ab, rows, np.abs(a * xq[cols]))
        err = np.abs(s[q * nr:(q + 1) * nr].astype(LD) - exact)
        _ratio("%s/%s product" % (name, sname), err, (3 * nb_row + 2) * LD(u) * ab)
        assert np.all(s[q * nr:(q + 1) * nr][nb_row == 0] == 0)


@pytest.mark.parametrize("name,sname", PAIRS)
def test_epilogues_against_long_double(name, sname):
    storage = BC.STORAGES[sname]
    S, v, out = BC.reference(name, storage)
    T, u = BC.arith(storage), LD(BC.UNIT[storage])
    s = out["NONE"]["y"].astype(LD)
    x, y, y1, dinv, r = (v[k].astype(LD) for k in ("x", "y", "y1", "dinv", "r"))
    c0, c1, c2 = (LD(T(c)) for c in (BC.C0, BC.C1, BC.C2))
    tag = "%s/%s " % (name, sname)
    A = np.abs
    _ratio(tag + "ADD", A(out["ADD"]["y"].astype(LD) - (y1 + s)), 2 * u * (A(y1) + A(s)))
    _ratio(tag + "SUB", A(out["SUB"]["y"].astype(LD) - (s - y1)), 2 * u * (A(y1) + A(s)))
    _ratio(tag + "PRE", A(out["PRE"]["y"].astype(LD) - (c0 * x + c2 * dinv * (y1 - s))), 5 * u * (A(c0 * x) + A(c2 * dinv) * (A(y1) + A(s))))
    rr = dinv * (y1 - s)
    _ratio(tag + "POST1 r", A(out["POST1"]["r"].astype(LD) - rr), 3 * u * dinv * (A(y1) + A(s)))
    _ratio(tag + "POST1 d", A(out["POST1"]["d"].astype(LD) - c0 * rr), 4 * u * A(c0) * dinv * (A(y1) + A(s)))
    _ratio(tag + "POST1 y", A(out["POST1"]["y"].astype(LD) - (x + c0 * rr)), 5 * u * (A(x) + A(c0) * dinv * (A(y1) + A(s))))
    _ratio(tag + "POST2", A(out["POST2"]["y"].astype(LD) - (y + c1 * x + c2 * (r - dinv * s))), 6 * u * (A(y) + A(c1 * x) + A(c2) * (A(r) + A(dinv * s))))
    assert out["POST2"]["z64"].dtype == np.float64 and np.array_equal(out["POST2"]["z64"], out["POST2"]["y"].astype(np.float64))
    assert len({BC.C0, BC.C1, BC.C2}) == 3 and min(BC.C0, BC.C1, BC.C2) < 0 < max(BC.C0, BC.C1, BC.C2)
    assert np.all(v["dinv"] > 0)
    for k in ("x", "y", "y1", "r"):
        assert (v[k] > 0).any() and (v[k] < 0).any(), k


@pytest.mark.parametrize("name,sname", PAIRS)
def test_structure_against_scipy_bsr(name, sname):
    """Block columns = sorted union over the three scalar rows, absent entries zero: scipy's BSR conversion of replica 0, indices sorted."""
    storage = BC.STORAGES[sname]
    S = BC.reference(name, storage)[0]
    M, _ = BC.case(name, storage)
    n = S["rep_rows"]
    nnz = int(M["rowptr"][n])
    A = sp.csr_matrix((M["val"][:nnz], M["col"][:nnz], M["rowptr"][:n + 1]), shape=(n, n))
    B = sp.bsr_matrix(A, blocksize=(3, 3))
    B.sort_indices()
    assert np.array_equal(B.indptr, S["browptr"]) and np.array_equal(B.indices, S["bcol"])
    assert np.array_equal(B.data.reshape(-1, 3, 3), S["blocks"])
    assert 9 * S["nblocks"] <= 2 * nnz + 64  # generators remove at most 3 of a block's 9 entries
    if name != "fp16_range" and storage == BC.F16 and nnz:
        a = np.abs(M["val"])
        assert a.min() >= 2.0 ** -13 * a.max()  # the normal half range after scaling
        assert np.all(np.abs(S["stored"][S["blocks"] != 0].astype(np.float64)) >= 2.0 ** -14)


def test_data_spans_the_decades():
    for name in ("many_tiles", "fills_1024"):
        for storage, decades in ((BC.F64, 12), (BC.F32, 6)):
            M, _ = BC.case(name, storage)
            rowmax = np.maximum.reduceat(np.abs(M["val"]), M["rowptr"][:-1][np.diff(M["rowptr"]) > 0])
            assert np.log10(rowmax.max() / rowmax.min()) >= decades - 1, (name, storage)
    # every fifth scalar row (of two or more entries) cancels: its sum is far below its terms
    for storage in BC.STORAGES.values():
        M, _ = BC.case("many_tiles", storage)
        for i in range(0, M["n"], 5):
            k0, k1 = M["rowptr"][i], M["rowptr"][i + 1]
            t = M["val"][k0:k1] * M["x"][M["col"][k0:k1]]
            assert k1 - k0 >= 2 and abs(t.sum()) <= 1e-6 * np.abs(t).max()
    # the fp16 range case reaches half's subnormals and flushes some entries
    S = BC.reference("fp16_range", BC.F16)[0]
    st = np.abs(S["stored"].astype(np.float64))[S["blocks"] != 0]
    assert S["scale"] == 1.0 and (st == 0).sum() >= 10 and ((st > 0) & (st < 2.0 ** -14)).sum() >= 10 and (st >= 2.0 ** -14).sum() >= 10


def test_tiling_and_scale_by_hand():
    """Block rows of 2, 1, 2, 4, 0, 3 blocks and a tile of 4: {0, 1} (3 blocks), {2} (2), {3, 4} (4), {5} (3)."""
    browptr = np.array([0, 2, 3, 5, 9, 9, 12])
    ntiles, npad, tile_br = BC.tiling(browptr, 4, 2)
    assert (ntiles, npad, tile_br) == (4, 4 + 2 + 4 + 4, [0, 2, 3, 5, 6])
    assert BC.tiling(browptr, 4, 4)[:2] == (4, 16)
    assert BC.tiling(browptr, 1024, 2)[:2] == (1, 12) and BC.tiling(browptr, 1024, 4)[:2] == (1, 12)
    assert BC.tiling(np.array([0, 0, 0, 0]), 1024, 4) == (1, 0, [0, 3])  # no entries: one empty tile
    assert [BC.fp16_scale(a) for a in (5.0, 1.0, 0.75, 1.999, 2.0, 3e-5, 0.0)] == [4.0, 1.0, 0.5, 1.0, 2.0, 2.0 ** -16, 1.0]
    # the tiny case end to end: 2 block rows, blocks (0,0), (0,1), (1,1); entry 5.0 is the largest
    M = dict(n=6, rowptr=np.array([0, 2, 4, 4, 5, 5, 6], np.int32), col=np.array([0, 3, 1, 5, 4, 3], np.int32), val=np.array([5.0, 0.5, -1.0, 2.0, 0.25, 3e-5]))
    for storage, W, npad in ((BC.F64, 2, 4), (BC.F32, 4, 4), (BC.F16, 4, 4)):
        S = BC.restate(M, storage, 512)
        assert BC.info_of(S) == [6, 2, 1, 512, 1, 3, npad, W] and S["scale"] == (4.0 if storage == BC.F16 else 1.0)
        assert S["browptr"].tolist() == [0, 2, 3] and S["bcol"].tolist() == [0, 1, 1]
    S = BC.restate(M, BC.F16, 0)
    assert S["tb"] == 1024 and S["stored"][0, 0, 0] == np.float16(1.25) and S["stored"][2, 2, 0] == np.float16(np.float32(3e-5 / 4.0))
    x = np.arange(1.0, 7.0)
    # rows: 5 x0 + 0.5 x3 = 7; -x1 + 2 x5 = 10; 0.25 x4 = 1.25; 3e-5 x3 (as stored)
    s = BC.product(S, x)
    assert s.dtype == np.float32 and s[:5].tolist() == [7.0, 10.0, 0.0, 1.25, 0.0]
    assert s[5] == np.float32(np.float32(np.float16(np.float32(3e-5 / 4.0))) * np.float32(4.0)) * np.float32(4.0)
    assert BC.restate(dict(M, n=0), BC.F64, 0) is None and BC.restate(dict(M, n=10), BC.F64, 0) is None


def test_declines_and_replicas_restated():
    """What `info` must show for each GPU case, decided here without a GPU."""
    for sname, storage in BC.STORAGES.items():
        W = BC.load_width(storage)
        S = BC.reference("ragged", storage)[0]
        nb = np.diff(S["browptr"])
        assert S["nbr"] == 37 and S["n"] == 111 and nb[0] == 0 and nb[-1] == 0 and set(nb.tolist()) == set(range(10)) and S["ntiles"] == 1
        assert S["nblocks"] % 2 == 1 and S["npad"] > S["nblocks"] and S["npad"] == -(-S["nblocks"] // W) * W
        M, _ = BC.case("many_tiles", storage)
        for tile in (512, 1024):
            S = BC.restate(M, storage, tile)
            assert S["ntiles"] >= 9 and S["ntiles"] % 8 != 0 and S["ntiles"] < S["nbr"], (tile, S["ntiles"])
        assert BC.restate(M, storage, 512)["ntiles"] > BC.restate(M, storage, 1024)["ntiles"]
        # a block row that fills a tile, and one that does not fit
        M512, M1024 = BC.case("fills_512", storage)[0], BC.case("fills_1024", storage)[0]
        M1025 = BC.fills_tile(storage, longest=1025)
        for M, tile in ((M512, 512), (M1024, 1024)):
            S = BC.restate(M, storage, tile)
            k = S["tile_br"].index(300 if tile == 512 else 700)
            assert S["tile_br"][k + 1] == S["tile_br"][k] + 1 and S["browptr"][S["tile_br"][k + 1]] - S["browptr"][S["tile_br"][k]] == tile  # alone in its tile
        assert BC.restate(M512, storage, 1024) is not None
        assert BC.restate(M1024, storage, 512) is None and BC.restate(M1025, storage, 1024) is None and BC.restate(M1025, storage, 512) is None
        S = BC.restate(BC.case("many_rows", storage)[0], storage, 1024)
        assert S["ntiles"] == 1 and S["nbr"] == 1500 and S["nblocks"] == 1000 and set(np.diff(S["browptr"]).tolist()) == {0, 1}
        assert BC.restate(BC.case("many_rows", storage)[0], storage, 512)["ntiles"] == 2
        # replicas
        for name, nrep in (("ragged_x3", 3), ("many_tiles_x8", 8)):
            M, hint = BC.case(name, storage)
            S1 = BC.reference(name.split("_x")[0], storage)[0]
            S = BC.restate(M, storage, 1024, hint)
            assert hint == nrep and S["nrep"] == nrep and S["n"] == nrep * S1["n"]
            assert (S["nbr"], S["ntiles"], S["nblocks"], S["npad"]) == (S1["nbr"], S1["ntiles"], S1["nblocks"], S1["npad"])  # one replica, as the struct
            assert BC.restate(BC.perturbed_last(M), storage, 1024, hint)["nrep"] == 1
            assert BC.restate(M, storage, 1024, 2 if nrep == 3 else 9)["nrep"] == 1  # 333 % 2, 16800 % 9: the hint does not divide n
            x = M["x"].reshape(nrep, -1)
            assert all(not np.array_equal(x[0], x[q]) for q in range(1, nrep))
        S = BC.reference("no_entries", storage)[0]
        assert BC.info_of(S) == [9, 3, 1, 1024, 1, 0, 0, W] and S["scale"] == 1.0


def test_zz_worst_ratio():
    """Reported last: the worst err / bound over everything above (a ratio near 1 would mean a bound with no room; above 1 has already failed)."""
    if _worst:
        k = max(_worst, key=_worst.get)
        print("worst err / bound over %d checks: %.3f (%s)" % (len(_worst), _worst[k], k))
        assert _worst[k] <= 1.0
