"""The numpy restatement of the multi-right-hand-side product (tests/mv_cases.py) IS the operation: without a GPU, every case, storage and kind of
tests/test_gpu_mv_paths.py is checked against long-double arithmetic on the stored (rounded) entries, so the GPU test cannot pass only by agreeing with itself;
and the plan facts each case is there for (lanes per block row, W, workgroups, XCD order) are asserted from the restatement alone.

Bounds (u: unit roundoff of the arithmetic type, 2^-53 or 2^-24), as tests/test_bsr3_reference_host.py derives them:
* plain product, per scalar row of nb blocks and per column: |s - sum_j a_ij x_j| <= (3 nb + 2) u sum_j |a_ij x_j| -- 3 nb products (one rounding each) added in
  some order by 3 nb - 1 additions; 3 nb + 2 covers every order 4 or 16 lanes could use and the second-order terms;
* epilogues, from the restated s: k u (sum of the absolute values of the formula's terms), k the roundings the longest chain of the formula carries plus one:
  ADD / SUB 2, PRE 5, POST1 r 3, d 4, y 5, POST2 6, RESTRICT d 3 (dinv c0, times s, plus one); z64 is the exact widening of y."""
import numpy as np
import pytest
import scipy.sparse as sp

import mv_cases as MC

LD = np.longdouble
TRIPLES = [(n, s, k) for n, (kinds, _) in MC.CASES.items() for s in MC.STORAGES for k in kinds] + [("fp16_range", "fp16", MC.SQUARE)]
_worst = {}


def _ratio(tag, err, bound):
    """Every entry within its bound (0 <= 0 included); remembers and prints the worst err / bound."""
    err, bound = np.ravel(err), np.ravel(bound)
    bad = np.flatnonzero(~(err <= bound))
    assert bad.size == 0, (tag, bad[:8], err[bad[:8]], bound[bad[:8]])
    nz = bound > 0
    w = float(np.max(err[nz] / bound[nz])) if nz.any() else 0.0
    _worst[tag] = max(_worst.get(tag, 0.0), w)
    print("%-44s worst err / bound = %.3f" % (tag, w))
    return w


def _tag(name, sname, kind):
    return "%s/%s%s " % (name, sname, ("", "", " negated")[kind])


@pytest.mark.parametrize("name,sname,kind", TRIPLES)
def test_product_against_long_double(name, sname, kind):
    storage = MC.STORAGES[sname]
    S, v, out = MC.reference(name, storage, kind)
    u, nbr = MC.UNIT[storage], S["nbr"]
    a = S["stored"].astype(LD) * LD(S["scale"])  # fp16 storage: times the (signed) power of two, exact
    xg = v["x"].astype(LD).reshape(S["nbc"], 3, MC.R)[S["bcol"]]  # (nblocks, 3 c, R)
    terms = a[:, :, :, None] * xg[:, None, :, :]  # (nblocks, 3 q, 3 c, R)
    brow = np.repeat(np.arange(nbr), np.diff(S["browptr"]))
    exact, ab = np.zeros((nbr, 3, MC.R), LD), np.zeros((nbr, 3, MC.R), LD)
    np.add.at(exact, brow, terms.sum(axis=2))
    np.add.at(ab, brow, np.abs(terms).sum(axis=2))
    s = out["NONE"]["y"]
    assert s.dtype == MC.arith(storage) and s.shape == (3 * nbr, MC.R)
    nb_row = np.repeat(np.diff(S["browptr"]), 3)
    _ratio(_tag(name, sname, kind) + "product", np.abs(s.astype(LD) - exact.reshape(3 * nbr, MC.R)), (3 * nb_row + 2)[:, None] * LD(u) * ab.reshape(3 * nbr, MC.R))
    assert np.all(s[nb_row == 0] == 0) and np.all(s[:, MC.ZERO_COLUMN] == 0)
    # the stored entries are the matrix's: negated where the copy is (fp16: through the sign of the scale), rounded once (fp32) or twice (fp16) at most
    sign = -1.0 if kind == MC.RECT_NEG else 1.0
    assert (S["scale"] < 0) == (kind == MC.RECT_NEG and storage == MC.F16) and np.all(S["stored"][S["blocks"] > 0] >= 0) == (storage == MC.F16 or kind != MC.RECT_NEG)
    if storage == MC.F64:
        assert np.array_equal(S["stored"], sign * S["blocks"])
    elif storage == MC.F32:
        assert np.array_equal(S["stored"], (sign * S["blocks"]).astype(np.float32))
    elif name != "fp16_range":
        assert np.all(np.abs(S["stored"].astype(np.float64) * S["scale"] - sign * S["blocks"]) <= 2.0 ** -11 * np.abs(S["blocks"]))


@pytest.mark.parametrize("name,sname,kind", TRIPLES)
def test_epilogues_against_long_double(name, sname, kind):
    storage = MC.STORAGES[sname]
    S, v, out = MC.reference(name, storage, kind)
    T, u = MC.arith(storage), LD(MC.UNIT[storage])
    s = out["NONE"]["y"].astype(LD)
    y, y1, r = (v[k].astype(LD) for k in ("y", "y1", "r"))
    dinv = v["dinv"].astype(LD)[:, None]
    c0, c1, c2 = (LD(T(c)) for c in (MC.C0, MC.C1, MC.C2))
    tag = _tag(name, sname, kind)
    A = np.abs
    assert list(out) == MC.admissible(kind)
    _ratio(tag + "ADD", A(out["ADD"]["y"].astype(LD) - (y1 + s)), 2 * u * (A(y1) + A(s)))
    _ratio(tag + "RESTRICT d", A(out["RESTRICT"]["d"].astype(LD) - dinv * c0 * s), 3 * u * A(dinv * c0 * s))
    assert np.array_equal(out["RESTRICT"]["y"], out["NONE"]["y"]) and sorted(out["RESTRICT"]) == ["d", "y"]
    assert np.all(v["dinv"] > 0) and v["dinv"].shape == (3 * S["nbr"],)
    if kind != MC.SQUARE:
        return
    x = v["x"].astype(LD)
    _ratio(tag + "SUB", A(out["SUB"]["y"].astype(LD) - (s - y1)), 2 * u * (A(y1) + A(s)))
    _ratio(tag + "PRE", A(out["PRE"]["y"].astype(LD) - (c0 * x + c2 * dinv * (y1 - s))), 5 * u * (A(c0 * x) + A(c2 * dinv) * (A(y1) + A(s))))
    rr = dinv * (y1 - s)
    _ratio(tag + "POST1 r", A(out["POST1"]["r"].astype(LD) - rr), 3 * u * dinv * (A(y1) + A(s)))
    _ratio(tag + "POST1 d", A(out["POST1"]["d"].astype(LD) - c0 * rr), 4 * u * A(c0) * dinv * (A(y1) + A(s)))
    _ratio(tag + "POST1 y", A(out["POST1"]["y"].astype(LD) - (x + c0 * rr)), 5 * u * (A(x) + A(c0) * dinv * (A(y1) + A(s))))
    _ratio(tag + "POST2", A(out["POST2"]["y"].astype(LD) - (y + c1 * x + c2 * (r - dinv * s))), 6 * u * (A(y) + A(c1 * x) + A(c2) * (A(r) + A(dinv * s))))
    assert out["POST2"]["z64"].dtype == np.float64 and np.array_equal(out["POST2"]["z64"], out["POST2"]["y"].astype(np.float64))


@pytest.mark.parametrize("name,sname,kind", TRIPLES)
def test_columns_differ(name, sname, kind):
    """A lane that read another column's piece of any operand would read other values: the 8 columns differ pairwise (also in magnitude), one is identically
    zero, one has a single sign, the others both."""
    storage = MC.STORAGES[sname]
    S, v, out = MC.reference(name, storage, kind)
    assert v["x"].shape == (3 * S["nbc"], MC.R) and all(v[k].shape == (3 * S["nbr"], MC.R) for k in ("y", "y1", "r"))
    for k in ("x", "y", "y1", "r"):
        a = v[k]
        assert a.dtype == MC.arith(storage)
        assert not a[:, MC.ZERO_COLUMN].any() and np.all(a[:, MC.ONE_SIGN_COLUMN] > 0)
        for p in range(MC.R):
            for q in range(p):
                assert not np.array_equal(a[:, p], a[:, q]) and not np.array_equal(np.abs(a[:, p]), np.abs(a[:, q])), (k, p, q)
            if p not in (MC.ZERO_COLUMN, MC.ONE_SIGN_COLUMN) and a.shape[0] > 3:
                assert (a[:, p] > 0).any() and (a[:, p] < 0).any(), (k, p)
        m = np.abs(a).max(axis=0)
        assert len(set(np.frexp(m[m > 0])[1].tolist())) >= 5, k  # the magnitudes spread over the columns
    if S["nbr"] > 1 and kind == MC.SQUARE:  # the results differ from column to column as well
        s = out["NONE"]["y"]
        assert all(not np.array_equal(s[:, p], s[:, q]) for p in range(MC.R) for q in range(p))


@pytest.mark.parametrize("name,sname,kind", TRIPLES)
def test_structure_against_scipy_bsr(name, sname, kind):
    """Block columns = sorted union over the three scalar rows, absent entries zero: scipy's BSR conversion of the (first) block, indices sorted."""
    storage = MC.STORAGES[sname]
    S = MC.reference(name, storage, kind)[0]
    M, nrep = MC.case(name, storage)
    n, nz = M["nrows"] // nrep, int(M["rowptr"][-1]) // nrep
    A = sp.csr_matrix((M["val"][:nz], M["col"][:nz], M["rowptr"][:n + 1]), shape=(n, 3 * S["nbc"]))
    B = sp.bsr_matrix(A, blocksize=(3, 3))
    B.sort_indices()
    assert np.array_equal(B.indptr, S["browptr"]) and np.array_equal(B.indices, S["bcol"])
    assert np.array_equal(B.data.reshape(-1, 3, 3), S["blocks"])
    assert S["wmax"] == int(np.diff(S["browptr"]).max()) and S["W"] % S["lpr"] == 0 and 0 <= S["W"] - S["wmax"] < S["lpr"]
    assert np.all((S["blocks"] == 0).sum(axis=(1, 2)) <= 3)  # up to three entries of a block absent
    if name != "fp16_range" and storage == MC.F16:
        a = np.abs(M["val"])
        assert a.min() >= 2.0 ** -13 * a.max()  # the normal half range after scaling
        assert np.all(np.abs(S["stored"][S["blocks"] != 0].astype(np.float64)) >= 2.0 ** -14)


@pytest.mark.parametrize("name", list(MC.PLAN))
def test_plan_facts(name):
    """What pmh_mv_test_info must show for each GPU case, decided here without a GPU."""
    for sname, storage in MC.STORAGES.items():
        if name == "fp16_range" and storage != MC.F16:
            continue
        for kind in MC.CASES[name][0] if name in MC.CASES else (MC.SQUARE,):
            S = MC.reference(name, storage, kind)[0]
            nbr, nbc, W, lpr, nwg, xmap = MC.PLAN[name]
            got = (S["nbr"], S["nbc"], S["W"] if W is not None else None, S["lpr"], S["nwg"], S["xmap"])
            assert got == MC.PLAN[name], (name, sname, kind, got)
            assert S["lpr"] == (16 if (S["wmax"] > 48 or nbr < 16384) else 4) and S["nwg"] == -(-nbr * lpr // 256) and S["xmap"] == (nwg >= 64)
            assert (S["scale"] == 1.0) == (storage != MC.F16 or name == "fp16_range")
    nb = np.diff(MC.reference(name, MC.F16 if name == "fp16_range" else MC.F64, MC.CASES[name][0][0] if name in MC.CASES else MC.SQUARE)[0]["browptr"])
    counts = set(nb.tolist())
    if name == "one_block":
        assert nb.tolist() == [1]  # 15 padded slots
    if name in ("ragged16", "ragged16_x3", "fp16_range"):
        assert nb[0] == 0 and nb[-1] == 0 and counts >= set(range(18)) | {31, 32, 33, 37} and nb.max() == 37
    if name == "remap16":
        assert counts == set(range(1, 10)) and nwg % 8 == 4 and 1077 * 16 % 256 != 0  # a remainder for the XCD order, a partial last workgroup
    if name == "w2048":
        assert nb.max() == 2048 and sorted(counts)[:-1] == [1, 2, 3] and W // lpr == 128
        M = MC.case("w2049", MC.F64)[0]
        assert MC.restate(M, MC.F64) is None and int(np.diff(MC.block_structure(M["nrows"], M["ncols"], M["rowptr"], M["col"], M["val"])[0]).max()) == 2049
    if name in ("quad_min", "below_quad", "quad_min_x2"):
        assert 4 < nb.max() <= 8 and nb.min() >= 4
        S = MC.reference(name, MC.F64)[0]
        i = np.arange(1, nbr - 1)  # chain neighbours: i - 1, i, i + 1 in every row
        for off in (-1, 0, 1):
            assert np.all([(S["bcol"][S["browptr"][j]:S["browptr"][j + 1]] == j + off).any() for j in i[::97]])
    if name == "quad_min":
        assert np.array_equal(MC.structure("quad_min")[1][:16383], MC.structure("below_quad")[1])  # the same, one block row fewer
    if name in ("quad_ragged", "quad_to_16"):
        assert counts >= set(range(49)) and nb.max() == (48 if name == "quad_ragged" else 49) and np.mean(nb <= 9) > 0.99
        if name == "quad_ragged":  # 12 trips; remap remainder 1; the last workgroup holds 37 quads
            assert W // lpr == 12 and nwg % 8 == 1 and nbr - 256 * 64 == 37
        assert nb[-36:].max() > 9 and nb[:64].max() > 9  # long rows inside the first and the last workgroup
        if name == "quad_to_16":
            a, b = MC.structure("quad_ragged")[1], MC.structure("quad_to_16")[1]
            assert (a != b).sum() == 1 and W == 64
    if name == "tall":
        assert counts == {0, 1, 2, 3, 4}
    if name == "wide":
        assert nb[-1] == 0 and 16 < nb.max() <= 48
        St, Sw = MC.reference("tall", MC.F64, MC.RECT)[0], MC.reference("wide", MC.F64, MC.RECT)[0]
        tall = sp.csr_matrix((np.ones(St["bcol"].size), St["bcol"], St["browptr"]), shape=(700, 90))
        wide = sp.csr_matrix((np.ones(Sw["bcol"].size), Sw["bcol"], Sw["browptr"]), shape=(90, 700))
        assert (tall.T != wide).nnz == 0  # the transposed structure
    if name == "tall_quad":
        assert counts == {0, 1, 2, 3, 4}


def test_data_spans_the_decades():
    for name in ("remap16", "quad_ragged"):
        for storage, decades in ((MC.F64, 12), (MC.F32, 6)):
            M, _ = MC.case(name, storage)
            rowmax = np.maximum.reduceat(np.abs(M["val"]), M["rowptr"][:-1][np.diff(M["rowptr"]) > 0])
            assert np.log10(rowmax.max() / rowmax.min()) >= decades - 1, (name, storage)
    # every fifth scalar row (of two or more entries) cancels in its column: its sum is far below its terms
    for name in ("remap16", "tall", "quad_min"):
        for storage in MC.STORAGES.values():
            M, _ = MC.case(name, storage)
            seen = set()
            for i in range(0, min(M["nrows"], 3000), 5):
                k0, k1 = M["rowptr"][i], M["rowptr"][i + 1]
                if k1 - k0 >= 2:
                    r = int(MC.cancel_column(i))
                    t = M["val"][k0:k1] * M["x"][M["col"][k0:k1], r]
                    assert abs(t.sum()) <= 1e-6 * np.abs(t).max(), (name, storage, i)
                    seen.add(r)
            assert seen == set(range(MC.R)) - {MC.ZERO_COLUMN}
    # the fp16 range case reaches half's subnormals and flushes some entries; numpy rounds to nearest even into them
    S = MC.reference("fp16_range", MC.F16)[0]
    st = np.abs(S["stored"].astype(np.float64))[S["blocks"] != 0]
    assert S["scale"] == 1.0 and (st == 0).sum() >= 10 and ((st > 0) & (st < 2.0 ** -14)).sum() >= 10 and (st >= 2.0 ** -14).sum() >= 10
    b = np.abs(S["blocks"][S["blocks"] != 0])
    assert np.all(st[b < 2.0 ** -25] == 0) and np.all(st[b > 2.0 ** -25] >= 2.0 ** -24) and np.all(np.abs(st - b) <= np.maximum(2.0 ** -25, 2.0 ** -11 * b))


def test_lane_order_and_scale_by_hand():
    """One block row of 9 blocks (diagonal blocks of one entry, so a slot's product is its value) with values that expose the association: 4 lanes sum
    (s0 + s1) + (s2 + s3) with s0 = (v0 + v4) + v8; 16 lanes sum the same slots one per lane, quad after quad."""
    big, one = 2.0 ** 54, 1.0
    vals = np.array([big, one, -big, one, one, one, one, one, one])  # slots 0 .. 8 of block row 0
    nbr = 9
    rowptr = np.zeros(3 * nbr + 1, np.int32)
    rowptr[1:] = 9  # scalar row 0 holds everything
    M = dict(nrows=3 * nbr, ncols=3 * nbr, rowptr=rowptr, col=(3 * np.arange(9)).astype(np.int32), val=vals)
    x = np.zeros((3 * nbr, MC.R))
    x[:, 0] = 1.0
    x[:, 1] = 2.0
    S = MC.restate(M, MC.F64)
    assert MC.info_of(S) == [9, 9, 16, 16, 0, 1, 0, 0] and S["bcol"].tolist() == list(range(9))
    s16 = MC.product(S, x)
    # 16 lanes: q0 = (big + 1) + (-big + 1) = 0 [big + 1 rounds to big, -big + 1 to -big], q1 = 4, q2 = 1: (0 + 4) + (1 + 0); exact arithmetic gives 7
    assert s16[0, 0] == ((big + one) + (-big + one)) + 4.0 + 1.0 == 5.0 and s16[0, 1] == 10.0 and not s16[1:].any()
    S4 = dict(S, lpr=4, W=12)  # the same row on the 4-lane map (the plan picks it from 16384 block rows on)
    s4 = MC.product(S4, x)
    # lanes: s0 = ((0 + big) + 1) + 1 = big [each + 1 is lost], s1 = 1 + 1, s2 = -big + 1 = -big, s3 = 1 + 1: (big + 2) + (-big + 2) = big - (big - 2) = 2, where
    # (s0 + s2) + (s1 + s3) would give 4
    assert s4[0, 0] == ((((0 + big) + one) + one) + 2.0) + ((-big + one) + 2.0) == 2.0
    assert [MC.BC.fp16_scale(a) for a in (5.0, 1.0, 0.75, 1.999, 2.0, 3e-5, 0.0)] == [4.0, 1.0, 0.5, 1.0, 2.0, 2.0 ** -16, 1.0]
    S = MC.restate(dict(M, val=vals / big * 5.0), MC.F16, MC.SQUARE)  # max|v| = 5: scale 4
    assert S["scale"] == 4.0 and S["stored"][0, 0, 0] == np.float16(1.25) and S["stored"][1, 0, 0] == np.float16(np.float32(5.0 / big / 4.0)) == 0


def test_declines_restated():
    """Every decline of the builder, and what the nearest accepted matrix looks like."""
    M = MC.case("ragged16", MC.F64)[0]
    e = np.zeros(1, np.int32)
    mat = lambda nr, nc, rowptr, col, val=None: dict(nrows=nr, ncols=nc, rowptr=np.asarray(rowptr, np.int32), col=np.asarray(col, np.int32),  # noqa: E731
                                                    val=np.ones(len(col)) if val is None else val)
    for storage in MC.STORAGES.values():
        assert MC.restate(mat(0, 0, e, []), storage) is None  # no rows
        assert MC.restate(mat(4, 4, [0, 1, 1, 1, 1], [0]), storage) is None and MC.restate(mat(3, 4, [0, 1, 1, 1], [0]), storage, MC.RECT) is None  # 3 does not divide
        assert MC.restate(mat(3, 6, [0, 1, 1, 1], [0]), storage) is None and MC.restate(mat(3, 6, [0, 1, 1, 1], [0]), storage, MC.RECT) is not None  # square copies only
        assert MC.restate(mat(6, 6, [0, 1, 1, 1, 2, 2, 2], [0, 3]), storage, nrep=2) is not None
        assert MC.restate(mat(9, 9, [0, 1, 1, 1, 2, 2, 2, 2, 2, 2], [0, 3]), storage, nrep=2) is None  # 3 nrep does not divide the rows
        assert MC.restate(mat(6, 6, [0, 2, 2, 2, 3, 3, 3], [0, 1, 3]), storage, nrep=2) is None  # nrep does not divide the entries
        assert MC.restate(mat(3, 3, [0, 2, 2, 2], [1, 0]), storage) is None and MC.restate(mat(3, 3, [0, 2, 2, 2], [1, 1]), storage) is None  # unsorted, repeated
        assert MC.restate(mat(3, 3, [0, 1, 2, 2], [1, 0]), storage) is not None  # descending ACROSS rows is fine
        assert MC.restate(mat(3, 3, [0, 0, 0, 0], []), storage) is None  # no block at all
        assert MC.restate(MC.case("w2049", storage)[0], storage) is None and MC.restate(MC.case("w2048", storage)[0], storage) is not None
        cap = MC.case("cap", storage)[0]
        assert MC.restate(cap, storage) is None and 1616.0 * 16384 * 76 > 2.0e9 > 1600.0 * 16384 * 76
    S = MC.restate(MC.case("ragged16_x3", MC.F64)[0], MC.F64, nrep=3)
    S1 = MC.restate(M, MC.F64)
    assert MC.info_of(S) == MC.info_of(S1) and np.array_equal(S["stored"], S1["stored"]) and np.array_equal(S["bcol"], S1["bcol"])  # the prefix copy = the first block's
    assert MC.restate(MC.case("ragged16_x3", MC.F64)[0], MC.F64)["nbr"] == 3 * 37


def test_zz_worst_ratio():
    """Reported last: the worst err / bound over everything above (a ratio near 1 would mean a bound with no room; above 1 has already failed)."""
    if _worst:
        k = max(_worst, key=_worst.get)
        print("worst err / bound over %d checks: %.3f (%s)" % (len(_worst), _worst[k], k))
        assert _worst[k] <= 1.0
