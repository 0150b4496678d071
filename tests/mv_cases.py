"""Inputs and references shared by tests/test_gpu_mv_paths.py and tests/test_mv_reference_host.py (no test in here, no GPU): a numpy restatement of the ELL
builder (mv_ell_build, k_mv_ell_fill) and of the multi-right-hand-side product k_mv_spmv (csrc/mv.hip) -- the block structure, the plan (lanes per block row, W,
workgroups, XCD order), the stored entry of each storage, the block product on 8 interleaved columns, the lane sums of both lane maps and the seven epilogues in
the kernel's own association -- and the matrices each test case is built from.

The library is compiled with -ffp-contract=off and the kernel sums in a fixed order, so the restatement is bit for bit what the device must return in all three
storages.  A padded slot and an absent entry of a block multiply a finite operand by zero; neither is modelled beyond that.  What says the same thing for the
one-column product comes from tests/bsr3_cases.py."""
import functools
import zlib

import numpy as np

import bsr3_cases as BC
from bsr3_cases import C0, C1, C2, F16, F32, F64, STORAGES, UNIT, arith  # noqa: F401

R = 8  # PMH_MV_R
NONE, ADD, SUB, PRE, POST1, POST2, RESTRICT = BC.NONE, BC.ADD, BC.SUB, BC.PRE, BC.POST1, BC.POST2, 20  # PMH_EPI_* / PMH_BSR_EPI_* / PMH_MV_EPI_RESTRICT
SQUARE, RECT, RECT_NEG = 0, 1, 2  # pmh_mv_test_create's kind
BLOCK = 256  # PMH_BLOCK: lanes per workgroup
ZERO_COLUMN, ONE_SIGN_COLUMN = 3, 5
COLUMN_EXP = (0, 3, -2, 1, 5, -4, 2, -1)  # column r of every operand carries 2^COLUMN_EXP[r]


# ---- the builder, restated ----------------------------------------------------------------------------------------------------------------------
def block_structure(nrows, ncols, rowptr, col, val):
    """bsr3_cases.block_structure on the matrix completed to a square one with empty rows (its key needs one bound for block rows and block columns)."""
    n = max(nrows, ncols)
    rp = np.concatenate([rowptr.astype(np.int64), np.full(n - nrows, rowptr[-1], np.int64)])
    browptr, bcol, blocks = BC.block_structure(n, rp, col, val)
    return browptr[:nrows // 3 + 1], bcol, blocks


def plan(nbr, wmax):
    """(lanes per block row, W, workgroups, XCD order of the workgroups) of a copy with nbr block rows of at most wmax blocks."""
    lpr = 16 if (wmax > 48 or nbr < 16384) else 4
    W = -(-wmax // lpr) * lpr
    nwg = -(-nbr * lpr // BLOCK)
    return lpr, W, nwg, int(nwg >= 64)


def restate(M, storage, kind=SQUARE, nrep=1):
    """What mv_ell_build lays out for the CSR M, or None where it declines: no rows, 3 not dividing rows or columns, a square copy of a matrix that is not, 3 nrep
    not dividing the rows or nrep the entries, a row (of the prefix) whose columns do not ascend strictly, no block at all or a block row of more than 2048, a padded
    copy beyond 2 GB.  nrep > 1: the first nrows / nrep rows and nnz / nrep entries."""
    nrows, ncols = M["nrows"], M["ncols"]
    rowptr = M["rowptr"].astype(np.int64)
    nnz = int(rowptr[-1])
    assert nrep == 1 or kind == SQUARE
    if (kind == SQUARE and nrows != ncols) or ncols % 3 or nrows % (3 * nrep) or nrows == 0 or nnz % nrep:
        return None
    n, nz = nrows // nrep, nnz // nrep
    nbr = n // 3
    rowptr = rowptr[:n + 1]
    col, val = M["col"][:nz], M["val"][:nz]
    assert int(rowptr[-1]) == nz and (nrep == 1 or nz == 0 or int(col.max()) < n), "the first diagonal block is not closed: the entry refuses it"
    if nz > 1:
        first = np.zeros(nz, bool)
        first[rowptr[:-1][np.diff(rowptr) > 0]] = True
        if np.any((np.diff(col.astype(np.int64)) <= 0) & ~first[1:]):
            return None
    nbc = ncols // 3 if kind != SQUARE else nbr
    browptr, bcol, blocks = block_structure(n, 3 * nbc, rowptr, col, val)
    wmax = int(np.diff(browptr).max())
    if wmax < 1 or wmax > 2048 or float(-(-wmax // 16) * 16) * nbr * 76.0 > 2.0e9:
        return None
    lpr, W, nwg, xmap = plan(nbr, wmax)
    scale, s = 1.0, (-1.0 if kind == RECT_NEG else 1.0)
    if storage == F64:
        stored = blocks * s
    elif storage == F32:
        stored = (blocks * s).astype(np.float32)
    else:
        scale = BC.fp16_scale(float(np.abs(val).max()) if nz else 0.0)
        stored = (blocks * (1.0 / scale)).astype(np.float32).astype(np.float16)  # float16(float32(v / scale)), as numpy rounds: to nearest even, subnormals kept
        scale *= s  # a negated fp16 copy keeps A / |scale| and multiplies by the negative scale
    return dict(nbr=nbr, nbc=nbc, W=W, lpr=lpr, wmax=wmax, nwg=nwg, xmap=xmap, kind=kind, storage=storage, scale=scale, browptr=browptr, bcol=bcol, blocks=blocks,
                stored=stored)


def info_of(S):
    """pmh_mv_test_info's eight numbers."""
    return [S["nbr"], S["nbc"], S["W"], S["lpr"], S["storage"], S["nwg"], S["xmap"], S["kind"]]


# ---- the kernel, restated -----------------------------------------------------------------------------------------------------------------------
def block_products(S, x):
    """(nblocks, 3, R) in T: ((a0 x0) + (a1 x1)) + (a2 x2) per scalar row of every block and per column; x: (3 nbc, R)."""
    T = arith(S["storage"])
    a = S["stored"].astype(T)  # half -> float is exact
    xg = np.asarray(x, T).reshape(S["nbc"], 3, R)[S["bcol"]]  # (nblocks, 3, R): the ONE contiguous piece of a block column
    return ((a[:, :, 0, None] * xg[:, None, 0, :]) + (a[:, :, 1, None] * xg[:, None, 1, :])) + (a[:, :, 2, None] * xg[:, None, 2, :])


def row_sums(S, prod):
    """Lane lw of lpr adds the products of the row's slots lw, lw + lpr, lw + 2 lpr, ... in that order, starting from +0; a quad of lanes combines as
    (s0 + s1) + (s2 + s3), the four quads of a 16-lane row as (q0 + q1) + (q2 + q3); fp16 storage: times the scale.  (3 nbr, R)."""
    T = arith(S["storage"])
    browptr, nbr, lpr = S["browptr"], S["nbr"], S["lpr"]
    nb = np.diff(browptr)
    lanes = np.zeros((nbr, lpr, 3, R), T)
    lane = np.arange(lpr)[None, :]
    for j in range(-(-S["wmax"] // lpr)):
        rows = np.flatnonzero(nb > lpr * j)
        k = browptr[rows, None] + lpr * j + lane
        inside = k < browptr[rows + 1, None]
        p = prod[np.minimum(k, prod.shape[0] - 1)]  # (rows, lpr, 3, R)
        lanes[rows] = lanes[rows] + np.where(inside[:, :, None, None], p, T(0))
    q = (lanes[:, 0::4] + lanes[:, 1::4]) + (lanes[:, 2::4] + lanes[:, 3::4])  # (nbr, lpr / 4, 3, R)
    s = q[:, 0] if lpr == 4 else (q[:, 0] + q[:, 1]) + (q[:, 2] + q[:, 3])
    if S["storage"] == F16:
        s = s * T(S["scale"])
    return s.reshape(3 * nbr, R)


def product(S, x):
    return row_sums(S, block_products(S, x))


def epilogue(epi, s, T, x, y, y1, dinv, r, c0=C0, c1=C1, c2=C2):
    """bsr3_cases.epilogue on (rows, R) multivectors with dinv per ROW, plus RESTRICT: y = s and d = (dinv c0) s."""
    dv = dinv[:, None]
    if epi == RESTRICT:
        return dict(y=s, d=(dv * T(c0)) * s)
    return BC.epilogue(epi, s, T, x, y, y1, dv, r, c0, c1, c2)


# ---- matrices -----------------------------------------------------------------------------------------------------------------------------------
def columns(rng, n, T, amp=1.0, normal=False):
    """(n, R) in T, exactly representable: column r = amp 2^COLUMN_EXP[r] times its own random values; one column identically zero, one of a single sign."""
    a = rng.standard_normal((n, R)) if normal else rng.uniform(0.5, 1.5, (n, R)) * rng.choice([-1.0, 1.0], (n, R))
    a = a * amp * np.ldexp(1.0, np.array(COLUMN_EXP))[None, :]
    a[:, ONE_SIGN_COLUMN] = np.abs(a[:, ONE_SIGN_COLUMN])
    a[:, ZERO_COLUMN] = 0.0
    return a.astype(T)


def cancel_column(i):
    """The column in which scalar row i (a multiple of 5) cancels: every column but the zero one takes its turn."""
    return np.array([r for r in range(R) if r != ZERO_COLUMN])[(i // 5) % (R - 1)]


def _cols(rng, nbc, lens, halfwidth=None, chain=False):
    """Flat sorted block columns of every block row: lens[i] distinct ones from the window around i (from all of them where the window is too small); chain: the
    neighbours i - 1, i, i + 1 come first."""
    out = []
    for i, L in enumerate(lens):
        L = int(L)
        lo, hi = (0, nbc) if halfwidth is None else (max(0, i - halfwidth), min(nbc, i + halfwidth + 1))
        if hi - lo < L:
            lo, hi = 0, nbc
        if chain:
            own = np.arange(max(0, i - 1), min(nbc, i + 2))
            rest = np.setdiff1d(lo + rng.permutation(hi - lo)[:L + 3], own)[:max(0, L - own.size)]
            out.append(np.sort(np.concatenate([own[:L], rest])))
        else:
            out.append(np.sort(lo + rng.permutation(hi - lo)[:L]))
    return np.concatenate(out).astype(np.int64) if out else np.zeros(0, np.int64)


def _assemble(rng, lens, bcol, nbc, storage, wide16=False):
    """bsr3_cases._assemble for 8 columns and any shape, vectorised: CSR of 3 x 3 blocks from the block columns of every block row, up to three of a block's nine
    entries absent (a block never vanishes).  Entry = block-row scale * [0.5, 1.5) with a random sign; the scales span 12 decades (fp64 storage), 6 (fp32) or
    2^-6 .. 2^-3 (fp16: every entry within [2^-13, 1] max|v|, the normal half range; wide16: 2^-30 .. 1 instead).  Every fifth scalar row with two or more entries
    cancels against column cancel_column(row) of x: the signs of its products are chosen against the running sum and its last value closes the sum to ~1e-9 of its
    terms.  Returns the matrix with its x."""
    lens = np.asarray(lens, np.int64)
    nbr, nb = lens.size, int(lens.sum())
    T = arith(storage)
    x = columns(rng, 3 * nbc, T).astype(np.float64)
    bscale = 10.0 ** rng.uniform(-6, 6, nbr) if storage == F64 else 10.0 ** rng.uniform(-3, 3, nbr) if storage == F32 else 2.0 ** rng.uniform(-6, -3, nbr)
    brow = np.repeat(np.arange(nbr), lens)
    keep = np.argsort(np.argsort(rng.random((nb, 9)), axis=1), axis=1) >= rng.integers(0, 4, nb)[:, None]  # 0 .. 3 random entries of a block absent
    k, e = np.nonzero(keep)
    row, c = 3 * brow[k] + e // 3, 3 * bcol[k] + e % 3
    order = np.lexsort((c, row))
    row, c = row[order], c[order]
    mag = 2.0 ** rng.uniform(-30, 0, row.size) if wide16 else bscale[row // 3] * rng.uniform(0.5, 1.5, row.size)
    v = mag * rng.choice([-1.0, 1.0], row.size)
    rowptr = np.zeros(3 * nbr + 1, np.int64)
    np.cumsum(np.bincount(row, minlength=3 * nbr), out=rowptr[1:])
    if not wide16:
        m = np.diff(rowptr)
        rows = np.flatnonzero((np.arange(3 * nbr) % 5 == 0) & (m >= 2))
        start, m = rowptr[rows], m[rows]
        xc = x[c, cancel_column(row)]  # per entry: the operand value of its row's cancelling column
        partial = np.zeros(rows.size)
        for j in range(int(m.max()) - 1 if rows.size else 0):
            act = np.flatnonzero(m - 1 > j)
            i = start[act] + j
            v[i] = np.abs(v[i]) * np.where(partial[act] > 0, -1.0, 1.0) * np.sign(xc[i])
            partial[act] += v[i] * xc[i]
        last = start + m - 1
        if storage == F16:  # the closing value would leave [2^-13, 1] max|v|: move the partial sum by half a term
            small = np.flatnonzero(np.abs(partial / xc[last]) < 2.0 ** -12)
            partial[small] += 0.5 * v[last[small] - 1] * xc[last[small] - 1]
            v[last[small] - 1] *= 1.5
        v[last] = -partial / xc[last] * (1.0 + 1e-9)
    if storage == F16 and v.size and not wide16:
        a = np.abs(v)
        assert a.max() < 1.0 and a.min() >= 2.0 ** -13 * a.max(), (a.min(), a.max())
    return dict(nrows=3 * nbr, ncols=3 * nbc, rowptr=rowptr.astype(np.int32), col=c.astype(np.int32), val=v, x=x)


def _ragged16_lens(rng):
    """37 block rows: every count 0 .. 17 and 31 .. 33, the full row of 37 (the most a square matrix of 37 block rows can hold), first and last row empty."""
    lens = np.concatenate([[0], np.arange(18), [31, 32, 33, 37], rng.integers(0, 38, 13), [0]])
    assert lens.size == 37
    return lens


def _quad_lens(rng, nbr, longest):
    """Mostly 0 .. 9 blocks; every count 0 .. 48 somewhere (so every residue mod 4 at every trip count), some of them inside the first and the last workgroup;
    one row of `longest`."""
    lens = rng.integers(0, 10, nbr)
    at = np.concatenate([np.arange(3, 64, 4)[:12], nbr - 36 + np.arange(0, 36, 3), rng.permutation(np.arange(100, nbr - 100))[:25]])
    lens[at] = np.arange(49)
    lens[70] = longest
    return lens


@functools.lru_cache(maxsize=None)
def structure(name):
    """(block columns, lens, flat sorted block columns of the rows) of a case -- the same for every storage."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    hw = None
    if name == "one_block":
        nbc, lens = 1, np.array([1])
    elif name in ("ragged16", "fp16_range"):
        nbc, lens = 37, _ragged16_lens(np.random.default_rng(11))
    elif name == "remap16":
        nbc, lens, hw = 1077, rng.integers(1, 10, 1077), 30
    elif name in ("w2048", "w2049"):
        nbc = 2048 if name == "w2048" else 2049
        lens = rng.integers(1, 4, nbc)
        lens[1000] = nbc
    elif name in ("quad_min", "below_quad"):
        nbc = 16384 if name == "quad_min" else 16383
        lens, hw = np.minimum(3, nbc) + np.random.default_rng(12).integers(1, 4, nbc), 30
        return nbc, lens, _cols(np.random.default_rng(13), nbc, lens, hw, chain=True)
    elif name in ("quad_ragged", "quad_to_16"):
        nbc, hw = 16421, 30
        lens = _quad_lens(np.random.default_rng(14), nbc, 48 if name == "quad_ragged" else 49)
        rng = np.random.default_rng(15)
    elif name == "tall":
        lens = rng.integers(1, 5, 700)
        lens[rng.permutation(700)[:20]] = 0
        return 90, lens, _cols(rng, 89, lens)  # block column 89 stays empty: an empty row of the transpose
    elif name == "wide":
        nbc_t, lens_t, bcol_t = structure("tall")
        brow_t = np.repeat(np.arange(700), lens_t)
        order = np.lexsort((brow_t, bcol_t))
        return 700, np.bincount(bcol_t, minlength=90), brow_t[order]
    elif name == "tall_quad":
        lens = rng.integers(0, 5, 16421)
        return 2100, lens, _cols(rng, 2100, lens)
    elif name == "cap":  # 16384 block rows, one of 1616 blocks: 1616 x 16384 x 76 bytes > 2 GB
        nbc, lens = 16384, np.ones(16384, np.int64)
        lens[5000] = 1616
    else:
        raise KeyError(name)
    return nbc, lens, _cols(rng, nbc, lens, hw)


def replicate(M, nrep):
    """nrep congruent copies of the square M on the diagonal; the vectors stay those of ONE block."""
    n, nnz = M["nrows"], int(M["rowptr"][-1])
    rowptr = np.concatenate([[0]] + [M["rowptr"][1:].astype(np.int64) + q * nnz for q in range(nrep)])
    col = np.concatenate([M["col"].astype(np.int64) + q * n for q in range(nrep)])
    return dict(nrows=n * nrep, ncols=n * nrep, rowptr=rowptr.astype(np.int32), col=col.astype(np.int32), val=np.tile(M["val"], nrep), x=M["x"])


# name -> (kinds it is built with, nrep); every storage gets its own values (the block-row scales depend on it), the structure is the same
CASES = {
    "one_block": ((SQUARE,), 1),
    "ragged16": ((SQUARE,), 1),
    "remap16": ((SQUARE,), 1),
    "w2048": ((SQUARE,), 1),
    "quad_min": ((SQUARE,), 1),
    "below_quad": ((SQUARE,), 1),
    "quad_ragged": ((SQUARE,), 1),
    "quad_to_16": ((SQUARE,), 1),
    "ragged16_x3": ((SQUARE,), 3),
    "quad_min_x2": ((SQUARE,), 2),
    "tall": ((RECT, RECT_NEG), 1),
    "wide": ((RECT, RECT_NEG), 1),
    "tall_quad": ((RECT, RECT_NEG), 1),
}
# what pmh_mv_test_info must report: (block rows, block columns, W, lanes per block row, workgroups, XCD order); None: whatever the restatement says
PLAN = {
    "one_block": (1, 1, 16, 16, 1, 0),
    "ragged16": (37, 37, 48, 16, 3, 0),
    "fp16_range": (37, 37, 48, 16, 3, 0),
    "remap16": (1077, 1077, 16, 16, 68, 1),
    "w2048": (2048, 2048, 2048, 16, 128, 1),
    "quad_min": (16384, 16384, 8, 4, 256, 1),
    "below_quad": (16383, 16383, 16, 16, 1024, 1),
    "quad_ragged": (16421, 16421, 48, 4, 257, 1),
    "quad_to_16": (16421, 16421, 64, 16, 1027, 1),
    "ragged16_x3": (37, 37, 48, 16, 3, 0),
    "quad_min_x2": (16384, 16384, 8, 4, 256, 1),
    "tall": (700, 90, 16, 16, 44, 0),
    "wide": (90, 700, None, 16, 6, 0),
    "tall_quad": (16421, 2100, 4, 4, 257, 1),
}


@functools.lru_cache(maxsize=None)
def case(name, storage):
    """(matrix with its x, nrep).  Built once; nobody writes into it."""
    if name == "fp16_range":
        assert storage == F16
        nbc, lens, bcol = structure(name)
        M = _assemble(np.random.default_rng(5), lens, bcol, nbc, storage, wide16=True)
        M["val"][0] = np.copysign(1.0, M["val"][0])  # max|v| = 1: scale 1
        return M, 1
    nrep = CASES[name][1] if name in CASES else 1
    base = name.split("_x")[0] if nrep > 1 else name
    if nrep > 1:
        return replicate(case(base, storage)[0], nrep), nrep
    nbc, lens, bcol = structure(name)
    return _assemble(np.random.default_rng(zlib.crc32(("%s/%d" % (name, storage)).encode())), lens, bcol, nbc, storage), 1


def operands(name, storage):
    """x (3 nbc, R), y1, r and a pre-filled y (3 nbr, R) of both signs, dinv > 0 per ROW (3 nbr), all in T; the 8 columns of each differ in magnitude, one is
    identically zero and one has a single sign (columns)."""
    M, nrep = case(name, storage)
    if nrep > 1:  # congruent copies: the vectors of ONE block, the base case's
        return operands(name.split("_x")[0], storage)
    n, T = M["nrows"], arith(storage)
    rng = np.random.default_rng(zlib.crc32(("operands %s/%d" % (name, storage)).encode()))
    amp = float(np.abs(M["val"]).max()) if M["val"].size else 1.0
    return dict(x=M["x"].astype(T), y1=columns(rng, n, T, amp, normal=True), r=columns(rng, n, T, normal=True), y=columns(rng, n, T, normal=True),
                dinv=(rng.uniform(0.1, 2.0, n) / amp).astype(T))


EPILOGUES = {"NONE": NONE, "ADD": ADD, "SUB": SUB, "PRE": PRE, "POST1": POST1, "POST2": POST2, "RESTRICT": RESTRICT}


def admissible(kind):
    """PRE, POST1 and POST2 read x at the row's own offset: square copies only."""
    return list(EPILOGUES) if kind == SQUARE else ["NONE", "ADD", "RESTRICT"]


@functools.lru_cache(maxsize=None)
def reference(name, storage, kind=None):
    """(restated copy, operands, {epilogue name: vectors written}).  ADD in place (y1 is y) writes what ADD writes; RESTRICT without d writes RESTRICT's y."""
    M, nrep = case(name, storage)
    kind = (CASES[name][0][0] if name in CASES else SQUARE) if kind is None else kind
    S = restate(M, storage, kind, nrep)
    assert S is not None, name
    T, v = arith(storage), operands(name, storage)
    s = product(S, v["x"])
    xr = v["x"] if kind == SQUARE else None
    out = {k: epilogue(EPILOGUES[k], s, T, xr, v["y"], v["y1"], v["dinv"], v["r"]) for k in admissible(kind)}
    for d in out.values():
        for a in d.values():
            a.setflags(write=False)
    for a in v.values():
        a.setflags(write=False)
    return S, v, out
