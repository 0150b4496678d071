"""Every kernel path of the CSR product (csrc/spmv.hip) against a reference that follows the kernel's own summation order.

pmh_csr_create picks a path from the matrix's structure: ELL (uniformly short rows), stream with one lane per row, medium stream (8 lanes per
row), vector (32 / 64 lanes per row) or long-row chunks.  Each case below is built to land on one path, proves it with kernel_info(), and then checks
the plain product, ADD (also in place), SUB, both transposes and the fused MPGP epilogue with the halt flag:

* rows the kernel sums left to right (ELL, stream rows within the 1024-entry tile): bit for bit against the oracle's MatMult_SeqAIJ;
* rows summed by lanes (medium, vector): bit for bit against a numpy restatement -- lane l sums entries k0 + l, k0 + l + L, ..., then the
  __shfl_down tree of width L;
* rows reduced by a whole workgroup (longer than the tile, long-row chunks): |y^ - y| <= (len + 2) u sum_j |a_ij x_j| per row, y in long double.

Row scales span 16 decades and every fifth row cancels to a small sum, so a dropped or doubled term fails in any row, whatever its size."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

import permon_amd as pa
from permon_amd._lib import check

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
ELL, STREAM, MEDIUM, VECTOR, LONG = 0, 1, 2, 3, 4  # info[0]
NONE, ADD, SUB, MPGP = 0, 1, 2, 3  # epilogues of pmh_csr_test_mult_epi
STREAM_TILE, MEDIUM_TILE = 1024, 2047  # longest row a stream / medium row block sums from its LDS tile


@pytest.fixture(scope="module")
def ctx():
    c = pa.Context(0)
    yield c
    c.close()


# ---- plan: the thresholds of pmh_csr_create, restated (the transposes' paths are asserted against this) ---------------------------------------
def _spans_fit16(rowptr, col, bounds):
    for r0, r1 in zip(bounds[:-1], bounds[1:]):
        c = col[rowptr[r0]:rowptr[r1]]
        if c.size and int(c.max()) - int(c.min()) > 65535:
            return 0
    return 1


def _rowblocks(rowptr, nnzb=STREAM_TILE - 1, max_rows=1024):
    n, rb, r = len(rowptr) - 1, [0], 0
    while r < n:
        start, base = r, rowptr[r]
        while r < n and r - start < max_rows and rowptr[r + 1] - base <= nnzb:
            r += 1
        if r == start:
            r += 1
        rb.append(r)
    return rb


def plan(rowptr, col):
    """(path, width, 16-bit columns) of a plain product."""
    n, nnz = len(rowptr) - 1, int(rowptr[-1])
    avg = nnz / n if n else 0.0
    if avg > 1024:
        return LONG, 0, 0
    if 24 < avg <= 256:
        return MEDIUM, 8, 0
    if avg > 256:
        return VECTOR, 32 if avg <= 512 else 64, 0
    wmax = int(np.diff(rowptr).max()) if n else 0
    if 1 <= wmax <= 8 and wmax * n <= 1.25 * nnz:
        return ELL, wmax, _spans_fit16(rowptr, col, list(range(0, n, 256)) + [n])
    return STREAM, 1, _spans_fit16(rowptr, col, _rowblocks(rowptr)) if n else 0


# ---- references ----------------------------------------------------------------------------------------------------------------------------
def lane_tree(rowptr, prod, L):
    """Lane l of a row sums entries k0 + l, k0 + l + L, ... in order; lane 0 then gathers the __shfl_down tree o = L/2, ..., 1."""
    n = len(rowptr) - 1
    lens = np.diff(rowptr)
    S = np.zeros((n, L))
    if n == 0 or prod.size == 0:
        return S[:, 0].copy()
    lane = np.arange(L)[None, :]
    for j in range(int(-(-lens.max() // L))):
        k = rowptr[:-1, None] + j * L + lane
        inside = k < rowptr[1:, None]
        S = S + np.where(inside, prod[np.minimum(k, prod.size - 1)], 0.0)  # +0.0 leaves a lane sum unchanged
    o = L // 2
    while o >= 1:
        S[:, :o] = S[:, :o] + S[:, o:2 * o]
        o //= 2
    return S[:, 0].copy()


def check_product(got, M, x, path, width, seq, y1=None, sub=False):
    """got = A x (+ y1, or - y1 with sub) on `path`; seq: the oracle's left-to-right sums of every row."""
    rowptr, col, val = M["rowptr"], M["col"], M["val"]
    n, lens = len(rowptr) - 1, np.diff(rowptr)
    assert got.shape == (n,)
    prod = val * x[col]
    if path == ELL:
        exact, s = np.ones(n, bool), seq
    elif path == STREAM:
        exact, s = lens <= STREAM_TILE, seq
    elif path == MEDIUM:
        exact, s = lens <= MEDIUM_TILE, lane_tree(rowptr, prod, 8)
    elif path == VECTOR:
        exact, s = np.ones(n, bool), lane_tree(rowptr, prod, width)
    else:
        exact, s = np.zeros(n, bool), seq
    e = s if y1 is None else (s - y1 if sub else y1 + s)
    bad = np.flatnonzero(exact & ~((got == e) | (np.isnan(got) & np.isnan(e))))
    assert bad.size == 0, ("rows differ from the kernel-order reference", bad[:8], got[bad[:8]], e[bad[:8]])
    rows = ~exact
    if rows.any():  # workgroup-reduced rows: per-row bound against a long-double sum
        nz = lens > 0  # reduceat runs each segment up to the next start: every non-empty row is one
        yl = np.zeros(n, np.longdouble)
        ab = np.zeros(n)
        if nz.any():
            starts = rowptr[:-1][nz]
            yl[nz] = np.add.reduceat(val.astype(np.longdouble) * x.astype(np.longdouble)[col], starts)
            ab[nz] = np.add.reduceat(np.abs(prod), starts)
        if y1 is not None:
            yl = yl - y1.astype(np.longdouble) if sub else yl + y1.astype(np.longdouble)
            ab = ab + np.abs(y1)
        err = np.abs(got.astype(np.longdouble) - yl)
        tol = (lens + 2) * U * ab
        bad = np.flatnonzero(rows & ~(err <= tol))
        assert bad.size == 0, ("rows outside the per-row bound", bad[:8], err[bad[:8]], tol[bad[:8]])


def transpose(M):
    """A' as build_transpose lays it out: rows of A' = columns of A, entries in ascending row of A."""
    rowptr, col, val = M["rowptr"], M["col"], M["val"]
    n, m = len(rowptr) - 1, M["ncols"]
    order = np.argsort(col, kind="stable")
    row_of = np.repeat(np.arange(n, dtype=np.int32), np.diff(rowptr))
    trp = np.zeros(m + 1, np.int64)
    np.cumsum(np.bincount(col, minlength=m), out=trp[1:])
    return dict(nrows=m, ncols=n, rowptr=trp.astype(np.int32), col=row_of[order], val=val[order])


# ---- matrices ------------------------------------------------------------------------------------------------------------------------------
def _assemble(rng, nrows, ncols, cols_of_row, cancel=True):
    """CSR from per-row sorted column lists; values of random sign whose magnitude depends on the row (1e-8 .. 1e8); every fifth row of two or more
    entries cancels against x0 (its last value is set so that the row's sum is nearly zero).  Returns the matrix and x0."""
    lens = np.array([len(c) for c in cols_of_row], dtype=np.int64)
    rowptr = np.zeros(nrows + 1, np.int64)
    np.cumsum(lens, out=rowptr[1:])
    assert rowptr[-1] < 2 ** 31
    col = np.concatenate(cols_of_row).astype(np.int32) if nrows and rowptr[-1] else np.zeros(0, np.int32)
    scale = 10.0 ** rng.uniform(-8, 8, nrows)
    val = rng.uniform(0.5, 1.5, col.size) * rng.choice([-1.0, 1.0], col.size) * np.repeat(scale, lens)
    x0 = rng.uniform(0.5, 1.5, ncols) * rng.choice([-1.0, 1.0], ncols)
    if cancel:
        for r in range(0, nrows, 5):
            k0, k1 = rowptr[r], rowptr[r + 1]
            if k1 - k0 >= 2:
                partial = 0.0
                for k in range(k0, k1 - 1):
                    partial += val[k] * x0[col[k]]
                val[k1 - 1] = -partial / x0[col[k1 - 1]] * (1.0 + 1e-9)
    return dict(nrows=nrows, ncols=ncols, rowptr=rowptr.astype(np.int32), col=col, val=val, x0=x0)


def _random_cols(rng, ncols, lens, center=None, halfwidth=None):
    out = []
    for i, L in enumerate(lens):
        L = int(L)
        if center is not None:
            lo, hi = max(0, center(i) - halfwidth), min(ncols, center(i) + halfwidth + 1)
            if hi - lo < L:
                lo, hi = 0, ncols
        else:
            lo, hi = 0, ncols
        out.append(np.sort(lo + rng.permutation(hi - lo)[:L]))
    return out


def _lengths_with_total(rng, n, lo, hi, total, fixed=None):
    """n row lengths in [lo, hi] summing to `total`; fixed: {row: length} set first."""
    fixed = fixed or {}
    lens = rng.integers(lo, hi + 1, n)
    for r, L in fixed.items():
        lens[r] = L
    free = np.array([r for r in range(n) if r not in fixed])
    while lens.sum() != total:
        d = total - lens.sum()
        r = free[rng.integers(free.size)]
        step = 1 if d > 0 else -1
        if lo <= lens[r] + step <= hi:
            lens[r] += step
    return lens


def ell_case(w, edge):
    """n = 1000 rows (not a multiple of 256), longest row w, nnz = 800 w: exactly 25 % padding (ELL) -- or one entry less (stream)."""
    rng = np.random.default_rng(100 + 2 * w + edge)
    n = 1000
    lens = np.full(n, w)
    empty = [3, 100, 257, 600]  # empty rows inside 256-row blocks
    lens[empty] = 0
    remove = n * w // 5 - 4 * w + (0 if edge else 1)
    slots = np.setdiff1d(np.arange(n), empty + [0])  # row 0 keeps length w
    drop = rng.choice(np.repeat(slots, w), remove, replace=False)
    lens -= np.bincount(drop, minlength=n)
    assert lens.sum() == (800 * w if edge else 800 * w - 1) and lens.max() == w
    M = _assemble(rng, n, n, _random_cols(rng, n, lens, center=lambda i: i, halfwidth=10))
    return M, ((ELL, w, 1) if edge else (STREAM, 1, 1))


def wide_case(far, stream):
    """65 600 rows of 4 neighbours; row 0 also reaches column `far`: the first 256-row block (ELL) or row block (stream) spans `far` columns.
    stream: row 10 has 12 entries, so there is no ELL copy."""
    rng = np.random.default_rng(far + stream)
    n = 65600
    cols = [np.arange(max(0, i - 1), min(n, i + 3)) for i in range(n)]
    cols[0] = np.array([0, 1, 2, far])
    if stream:
        cols[10] = np.arange(10, 22)
    M = _assemble(rng, n, n, cols)
    fit = 1 if far <= 65535 else 0
    return M, ((STREAM, 1, fit) if stream else (ELL, 4, fit))


def stream_tile_case():
    """Rows of 1023, 1024 (summed from the tile, left to right) and 1025 entries (reduced by the workgroup) among rows of 0-8."""
    rng = np.random.default_rng(7)
    n = 2000
    lens = rng.integers(0, 9, n)
    lens[[5, 700, 1400]] = (1023, 1024, 1025)
    return _assemble(rng, n, n, _random_cols(rng, n, lens)), (STREAM, 1, 1)


def stream_many_rows_case():
    """5000 rows, most of them empty: row blocks of 1024 rows (PMH_MAX_ROWS_PER_BLOCK), more than the 256 lanes of a workgroup."""
    rng = np.random.default_rng(8)
    n = 5000
    lens = np.where(np.arange(n) % 7 == 0, 3, 0)
    lens[4321] = 12
    return _assemble(rng, n, n, _random_cols(rng, n, lens, center=lambda i: i, halfwidth=20)), (STREAM, 1, 1)


def avg_case(n, total, lo, hi, fixed=None, seed=0, ncols=None):
    rng = np.random.default_rng(seed)
    lens = _lengths_with_total(rng, n, lo, hi, total, fixed)
    ncols = ncols or n
    M = _assemble(rng, n, ncols, _random_cols(rng, ncols, lens))
    return M, plan(M["rowptr"], M["col"])


CASES = {
    **{"ell_w%d" % w: functools.partial(ell_case, w, True) for w in range(1, 9)},
    **{"ell_w%d_over_padding" % w: functools.partial(ell_case, w, False) for w in range(1, 9)},
    "ell_span65535": functools.partial(wide_case, 65535, False),
    "ell_span65536": functools.partial(wide_case, 65536, False),
    "stream_span65535": functools.partial(wide_case, 65535, True),
    "stream_span65536": functools.partial(wide_case, 65536, True),
    "stream_tile_edge": stream_tile_case,
    "stream_many_rows": stream_many_rows_case,
    # average exactly 24: stream; just above: medium (odd row starts, rows of 2047 / 2048 / 2049 entries)
    "stream_avg24": functools.partial(avg_case, 600, 24 * 600, 9, 40, None, 11),
    "medium_avg24+": functools.partial(avg_case, 2100, 24 * 2100 + 1, 0, 40, {7: 2047, 1000: 2048, 2099: 2049}, 12),
    "medium_avg256": functools.partial(avg_case, 2100, 256 * 2100, 150, 362, {0: 0, 1: 1, 2099: 2049}, 13),
    "vector32_avg256+": functools.partial(avg_case, 3000, 256 * 3000 + 1, 100, 412, {17: 0, 18: 0, 2000: 3000}, 14),
    "vector32_avg512": functools.partial(avg_case, 1500, 512 * 1500, 200, 824, {5: 0, 800: 1500}, 15),
    "vector64_avg512+": functools.partial(avg_case, 1500, 512 * 1500 + 1, 200, 824, {5: 0, 6: 0, 801: 1500}, 16),
    "vector64_avg1024": functools.partial(avg_case, 1100, 1024 * 1100, 950, 1100, {9: 0, 10: 1}, 17),
    "long_avg1024+": functools.partial(avg_case, 4100, 1024 * 4100 + 1, 600, 1450, {3: 4096, 4: 4097, 5: 1024, 6: 1025, 7: 0}, 18),
    # degenerate shapes
    "rows0": lambda: (_assemble(np.random.default_rng(19), 0, 0, []), (STREAM, 1, 0)),
    "rows0_cols5": lambda: (_assemble(np.random.default_rng(20), 0, 5, []), (STREAM, 1, 0)),
    "row1_1x1": lambda: (_assemble(np.random.default_rng(21), 1, 1, [np.array([0])]), (ELL, 1, 1)),
    "row1_medium": lambda: (_assemble(np.random.default_rng(22), 1, 100, [np.arange(3, 100, 3)]), (MEDIUM, 8, 0)),
    "row1_long": lambda: (_assemble(np.random.default_rng(23), 1, 5000, [np.sort(np.random.default_rng(5).choice(5000, 4097, replace=False))]), (LONG, 0, 0)),
    "cols0": lambda: (_assemble(np.random.default_rng(24), 5, 0, [np.zeros(0, int)] * 5), (STREAM, 1, 1)),
    "no_entries": lambda: (_assemble(np.random.default_rng(25), 300, 300, [np.zeros(0, int)] * 300), (STREAM, 1, 1)),
    "rect_700x3000": functools.partial(avg_case, 700, 700 * 6, 0, 12, None, 26, 3000),
    "rect_3000x700": functools.partial(avg_case, 3000, 3000 * 30, 0, 60, None, 27, 700),
}
PATH_OF_CASE = {  # the path each hand-built case is aimed at (avg_case plans are checked against these too)
    "stream_avg24": (STREAM, 1, 1), "medium_avg24+": (MEDIUM, 8, 0), "medium_avg256": (MEDIUM, 8, 0),
    "vector32_avg256+": (VECTOR, 32, 0), "vector32_avg512": (VECTOR, 32, 0), "vector64_avg512+": (VECTOR, 64, 0), "vector64_avg1024": (VECTOR, 64, 0),
    "long_avg1024+": (LONG, 0, 0), "rect_700x3000": (STREAM, 1, 1), "rect_3000x700": (MEDIUM, 8, 0),
}


@functools.lru_cache(maxsize=None)
def case(name):
    M, expect = CASES[name]()
    if name in PATH_OF_CASE:
        assert expect == PATH_OF_CASE[name], (name, expect)
    assert plan(M["rowptr"], M["col"]) == expect, (name, plan(M["rowptr"], M["col"]), expect)
    return M, expect


def _csr(ctx, M):
    return pa.CsrMat(ctx, M["nrows"], M["ncols"], M["rowptr"], M["col"], M["val"])


def _info(A, M, expect):
    info, uid = A.kernel_info()
    assert tuple(info[:3]) == tuple(expect), (info, expect)
    assert uid != 0
    n, lens = M["nrows"], np.diff(M["rowptr"])
    if expect[0] == ELL:
        assert info[4] == (n + 255) // 256
    if expect[0] in (STREAM, MEDIUM):
        assert info[3] == (1024 if expect[0] == STREAM else 2048)
    if expect[0] == LONG:
        assert info[3] == int(np.sum(-(-lens // 4096)))
    assert (info[5] == 0) == (n == 0)
    return info


def _mult_epi(ctx, A, kind, x, y, y1=None, g=None, xx=None, lb=None, ub=None, halt=0):
    s = (C.c_double * 3)()
    p = lambda v: v.p if v is not None else None  # noqa: E731
    check(ctx.L.pmh_csr_test_mult_epi(A.h, kind, p(x), p(y1), p(g), p(xx), p(lb), p(ub), int(halt), p(y), s))
    return np.array(s[:])


NAMES = list(CASES)


@pytest.mark.parametrize("name", NAMES)
def test_products(ctx, oracle, name):
    M, expect = case(name)
    n, m = M["nrows"], M["ncols"]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    A = _csr(ctx, M)
    info = _info(A, M, expect)
    if name == "stream_many_rows":
        assert info[4] >= 5  # row blocks capped at 1024 rows
    if expect[0] == MEDIUM and n > 1:
        lens = np.diff(M["rowptr"])
        assert np.any((M["rowptr"][:-1] % 2 == 1) & (lens >= 9))  # 16-byte loads aligned down to an even index
    Ao = oracle.Csr(n, m, M["rowptr"], M["col"], M["val"])
    x = M["x0"]
    xd = ctx.vec_from(x)
    sentinel = np.full(n, 7.25e77)
    # y = A x
    yd = ctx.vec_from(sentinel)
    A.mult(xd, yd)
    y = yd.to_numpy()
    check_product(y, M, x, expect[0], expect[1], oracle.spmv(Ao, x))
    # ADD, out of place and in place (y1 is y)
    y1 = rng.standard_normal(n) * 10.0 ** rng.uniform(-8, 8, n)
    y1d, yd2 = ctx.vec_from(y1), ctx.vec_from(sentinel)
    A.mult_add(xd, y1d, yd2)
    ya = yd2.to_numpy()
    check_product(ya, M, x, expect[0], expect[1], oracle.spmv(Ao, x), y1=y1)
    A.mult_add(xd, y1d, y1d)
    assert np.array_equal(y1d.to_numpy(), ya)
    # SUB: y = A x - y1 (the fused -b of the gradient)
    y1d.set_numpy(y1)
    yd3 = ctx.vec_from(sentinel)
    _mult_epi(ctx, A, SUB, xd, yd3, y1=y1d)
    check_product(yd3.to_numpy(), M, x, expect[0], expect[1], oracle.spmv(Ao, x), y1=y1, sub=True)
    # plain product through the test entry: the same launch as mult
    yd4 = ctx.vec_from(sentinel)
    _mult_epi(ctx, A, NONE, xd, yd4)
    assert np.array_equal(yd4.to_numpy(), y)
    # transposes: A' is built on the host (build_transpose) and planned like any matrix; the same arrays handed over directly take the same path
    T = transpose(M)
    tpath = plan(T["rowptr"], T["col"])
    At = _csr(ctx, T)
    _info(At, T, tpath)
    xt = rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-3, 3, n)
    xtd = ctx.vec_from(xt)
    ytd, ytd2 = ctx.vec_from(np.full(m, -3.5e-70)), ctx.vec_from(np.full(m, -3.5e-70))
    A.mult_transpose(xtd, ytd)
    At.mult(xtd, ytd2)
    yt = ytd.to_numpy()
    assert np.array_equal(yt, ytd2.to_numpy())
    seq_t = oracle.spmv_transpose(Ao, xt)
    check_product(yt, T, xt, tpath[0], tpath[1], seq_t)
    yt1 = rng.standard_normal(m)
    yt1d = ctx.vec_from(yt1)
    check(ctx.L.pmh_csr_mult_transpose_add(A.h, xtd.p, yt1d.p, ytd.p))
    check_product(ytd.to_numpy(), T, xt, tpath[0], tpath[1], seq_t, y1=yt1)
    check(ctx.L.pmh_csr_mult_transpose_add(A.h, xtd.p, yt1d.p, yt1d.p))  # in place
    assert np.array_equal(yt1d.to_numpy(), ytd.to_numpy())
    At.destroy()
    A.destroy()


SQUARE = [k for k in NAMES if k not in ("rows0_cols5", "row1_medium", "row1_long", "cols0", "rect_700x3000", "rect_3000x700")]


def _feasible(p, xx, lb, ub):
    """QPCFeas of the box: min over the active bounds of the step to them, with the kernel's divisions; +inf when none is active."""
    c = [np.array([np.inf])]
    if lb is not None:
        a = (p > 0) & (lb > -np.inf)
        c.append((xx[a] - lb[a]) / p[a])
    if ub is not None:
        a = (p < 0) & (ub < np.inf)
        c.append((xx[a] - ub[a]) / p[a])
    return float(np.min(np.concatenate(c)))


@pytest.mark.parametrize("name", SQUARE)
def test_mpgp_epilogue(ctx, oracle, name):
    """Ap with p'Ap, g'p and the feasible step fused; the same y as a plain product; a halted launch changes nothing."""
    M0, expect = case(name)
    n = M0["nrows"]
    M = dict(M0, val=np.abs(M0["val"]))  # |A| and p >= 0: every term of p'Ap is >= 0, so a lost workgroup partial cannot hide
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 1)
    A = _csr(ctx, M)
    info = _info(A, M, expect)
    assert n < 1000 or info[5] > 1  # several workgroups leave partials
    Ao = oracle.Csr(n, n, M["rowptr"], M["col"], M["val"])
    mpgp_path = STREAM if expect[0] == LONG else expect[0]  # the MPGP epilogue runs long rows on the stream kernel

    def vec(a):
        return ctx.vec_from(a) if a is not None else None

    zero = rng.random(n) < 0.1
    mag = rng.uniform(0.5, 1.5, n) * 10.0 ** rng.uniform(-2, 2, n)
    sign = rng.choice([-1.0, 1.0], n)
    xx = rng.uniform(-1.0, 1.0, n)
    lb = np.where(rng.random(n) < 0.2, -np.inf, xx - rng.uniform(0.0, 2.0, n))
    ub = np.where(rng.random(n) < 0.2, np.inf, xx + rng.uniform(0.0, 2.0, n))
    sets = {
        "positive": (np.where(zero, 0.0, mag), lb, None),
        "mixed": (np.where(zero, 0.0, mag * sign), lb, ub),
        "ub_only": (np.where(zero, 0.0, mag * sign), None, ub),
        "no_bounds": (mag * sign, None, None),
        "inactive": (mag * sign, np.full(n, -np.inf), np.full(n, np.inf)),
    }
    xxd = ctx.vec_from(xx)
    for tag, (p, lo, hi) in sets.items():
        g = rng.uniform(0.5, 2.0, n) * (1.0 if tag == "positive" else rng.choice([-1.0, 1.0], n))
        pd, gd, yd = ctx.vec_from(p), ctx.vec_from(g), ctx.vec_from(np.full(n, 7.25e77))
        s = _mult_epi(ctx, A, MPGP, pd, yd, g=gd, xx=xxd, lb=vec(lo), ub=vec(hi))
        y = yd.to_numpy()
        yplain = ctx.vec(n)
        A.mult(pd, yplain)
        if mpgp_path == expect[0]:
            assert np.array_equal(y, yplain.to_numpy()), tag
        check_product(y, M, p, mpgp_path, expect[1], oracle.spmv(Ao, p))
        t_pap, t_gp = p * y, g * p
        pap = float(np.sum(t_pap.astype(np.longdouble)))
        gp = float(np.sum(t_gp.astype(np.longdouble)))
        assert abs(s[0] - pap) <= (n + 1) * U * np.sum(np.abs(t_pap)), (tag, s[0], pap)
        assert abs(s[1] - gp) <= (n + 1) * U * np.sum(np.abs(t_gp)), (tag, s[1], gp)
        assert s[2] == _feasible(p, xx, lo, hi), (tag, s[2], _feasible(p, xx, lo, hi))
        if tag in ("no_bounds", "inactive"):
            assert s[2] == np.inf
        if tag == "positive" and n:
            assert np.all(t_pap >= 0) and np.all(t_gp >= 0)
        if n == 0:
            assert s.tolist() == [0.0, 0.0, np.inf]
        if tag == "positive":
            # halt: a different p, y pre-filled with a sentinel -- y and the three scalars stay as they are
            p2 = rng.standard_normal(n)
            y2d = ctx.vec_from(np.full(n, -1.5e-300))
            s2 = _mult_epi(ctx, A, MPGP, ctx.vec_from(p2), y2d, g=gd, xx=xxd, lb=vec(lo), ub=vec(hi), halt=1)
            assert np.array_equal(y2d.to_numpy(), np.full(n, -1.5e-300))
            assert np.array_equal(s2, s)
            # the three plain forms honour the flag too
            for kind in (NONE, ADD, SUB):
                _mult_epi(ctx, A, kind, ctx.vec_from(p2), y2d, y1=gd, halt=1)
                assert np.array_equal(y2d.to_numpy(), np.full(n, -1.5e-300)), kind
    A.destroy()


def test_mpgp_no_rows_is_identities(ctx):
    """A 0 x 0 operator (a rank that owns no rows): the MPGP scalars are the identities (0, 0, +inf), whatever the partial buffer holds."""
    for _ in range(2):
        A = pa.CsrMat(ctx, 0, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
        info, _uid = A.kernel_info()
        assert info[5] == 0
        v = ctx.vec(0)
        s = _mult_epi(ctx, A, MPGP, v, ctx.vec(0), g=v, xx=v, lb=v, ub=v)
        assert s.tolist() == [0.0, 0.0, np.inf]
        A.destroy()


def test_uid_distinct_nonzero(ctx):
    """Caches keyed on a matrix compare uid, not the address a later matrix may reuse: every live matrix has its own non-zero uid."""
    M, _ = case("ell_w3")
    A, B = _csr(ctx, M), _csr(ctx, M)
    ua, ub = A.kernel_info()[1], B.kernel_info()[1]
    assert ua != 0 and ub != 0 and ua != ub
    B.destroy()
    C_ = _csr(ctx, M)  # possibly at B's old address
    uc = C_.kernel_info()[1]
    assert uc not in (0, ua, ub)
    A.destroy()
    C_.destroy()
