"""Inputs and references shared by tests/test_gpu_bsr3_paths.py and tests/test_bsr3_reference_host.py (no test in here, no GPU): a numpy restatement of
pmh_bsr3_from_csr and k_bsr3 (csrc/bsr.hip) -- the block structure, the tiling, the stored entry of each storage, the block product, the four-lane row sum and
the six epilogues in the kernel's own association -- and the matrices each test case is built from.

The library is compiled with -ffp-contract=off and the kernel sums in a fixed order, so the restatement is bit for bit what the device must return in all
three storages.  The row sum does not depend on the tile or on W (a lane starts at the row's first block, wherever the tile starts); the tiling only decides
ntiles and npad, which pmh_bsr3_test_info reports."""
import functools

import numpy as np

F64, F32, F16 = 0, 1, 2  # PMH_BSR_*
STORAGES = {"fp64": F64, "fp32": F32, "fp16": F16}
NONE, ADD, SUB, PRE, POST1, POST2 = 0, 1, 2, 10, 11, 12  # PMH_EPI_* / PMH_BSR_EPI_*
EPILOGUES = {"NONE": NONE, "ADD": ADD, "SUB": SUB, "PRE": PRE, "POST1": POST1, "POST2": POST2}
C0, C1, C2 = 0.8125, -1.37, 0.4321  # three distinct constants, mixed signs, none of them 0 or +-1
UNIT = {F64: 2.0 ** -53, F32: 2.0 ** -24, F16: 2.0 ** -24}  # unit roundoff of the arithmetic type T


def arith(storage):
    """T: the type of the vectors and of every operation (fp64; fp32 for both reduced storages)."""
    return np.float64 if storage == F64 else np.float32


def load_width(storage):
    """W: blocks per vector load."""
    return 2 if storage == F64 else 4


# ---- the conversion, restated -------------------------------------------------------------------------------------------------------------------
def block_structure(n, rowptr, col, val):
    """(browptr, bcol, blocks): the block columns of a block row are the sorted union over its three scalar rows; blocks[k] is the dense 3 x 3 block,
    absent entries zero."""
    nbr = n // 3
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    key = (row // 3) * (n // 3 + 1) + col.astype(np.int64) // 3  # (block row, block column), ordered
    uniq, inv = np.unique(key, return_inverse=True)
    bcol = (uniq % (n // 3 + 1)).astype(np.int32)
    browptr = np.zeros(nbr + 1, np.int64)
    np.cumsum(np.bincount(uniq // (n // 3 + 1), minlength=nbr), out=browptr[1:])
    blocks = np.zeros((uniq.size, 3, 3))
    np.add.at(blocks, (inv, row % 3, col % 3), val)
    return browptr, bcol, blocks


def tiling(browptr, tb, W):
    """(ntiles, npad, first block row of every tile + [nbr]): whole block rows per tile; a tile closes before the block row that would take it past tb blocks;
    every tile's block count is padded to a multiple of W."""
    nbr = len(browptr) - 1
    tile_br, start = [0], 0
    for br in range(nbr):
        if browptr[br + 1] - browptr[start] > tb:
            tile_br.append(br)
            start = br
    tile_br.append(nbr)
    npad = sum(-(-int(browptr[b] - browptr[a]) // W) * W for a, b in zip(tile_br[:-1], tile_br[1:]))
    return len(tile_br) - 1, npad, tile_br


def fp16_scale(amax):
    """The power of two that puts max|v| in [1, 2); 1 for a matrix without a non-zero entry."""
    return float(np.ldexp(1.0, int(np.frexp(amax)[1]) - 1)) if amax > 0 else 1.0  # amax = m 2^e with m in [0.5, 1): 2^(e - 1)


def replicas(M, hint):
    """nrep as the conversion settles it: the hint is believed only when it divides n, n / hint (a multiple of 3) and nnz, and every diagonal block repeats
    block 0 entry by entry."""
    n, rowptr, col, val = M["n"], M["rowptr"].astype(np.int64), M["col"], M["val"]
    nnz = int(rowptr[-1])
    if not (hint > 1 and n % hint == 0 and (n // hint) % 3 == 0 and nnz % hint == 0):
        return 1
    nr, nz = n // hint, nnz // hint
    for q in range(1, hint):
        same = (np.array_equal(rowptr[q * nr:(q + 1) * nr + 1] - q * nz, rowptr[:nr + 1]) and np.array_equal(col[q * nz:(q + 1) * nz] - q * nr, col[:nz])
                and np.array_equal(val[q * nz:(q + 1) * nz], val[:nz]) and (nz == 0 or int(col[:nz].max()) < nr))
        if not same:
            return 1
    return hint


def restate(M, storage, tile, hint=1):
    """What pmh_bsr3_from_csr builds from the CSR M for (storage, tile, hint), or None where it declines: n == 0 or n % 3 != 0, a block row with more blocks
    than a tile, blocks mostly empty (9 nblocks > 2 nnz + 64)."""
    n_all = M["n"]
    if n_all == 0 or n_all % 3:
        return None
    nrep = replicas(M, hint)
    n = n_all // nrep
    rowptr = M["rowptr"].astype(np.int64)[:n + 1]
    nnz = int(rowptr[-1])
    col, val = M["col"][:nnz], M["val"][:nnz]
    tb, W = (512 if tile == 512 else 1024), load_width(storage)
    browptr, bcol, blocks = block_structure(n, rowptr, col, val)
    if n and int(np.diff(browptr).max()) > tb:
        return None
    if 9 * len(bcol) > 2 * nnz + 64:
        return None
    ntiles, npad, tile_br = tiling(browptr, tb, W)
    scale = 1.0
    if storage == F32:
        stored = blocks.astype(np.float32)
    elif storage == F16:
        scale = fp16_scale(float(np.abs(val).max()) if nnz else 0.0)
        stored = (blocks / scale).astype(np.float32).astype(np.float16)  # float16(float32(v / scale)), as numpy rounds: to nearest even, subnormals kept
    else:
        stored = blocks
    return dict(n=n_all, rep_rows=n, nbr=n // 3, nrep=nrep, tb=tb, W=W, ntiles=ntiles, npad=npad, nblocks=len(bcol), tile_br=tile_br, browptr=browptr, bcol=bcol,
                blocks=blocks, stored=stored, scale=scale, storage=storage)


def info_of(S):
    """pmh_bsr3_test_info's eight numbers."""
    return [S["n"], S["nbr"], S["ntiles"], S["tb"], S["nrep"], S["nblocks"], S["npad"], S["W"]]


# ---- the kernel, restated -----------------------------------------------------------------------------------------------------------------------
def block_products(S, x):
    """(nblocks, 3) in T: ((a0 x0) + (a1 x1)) + (a2 x2) per scalar row of every block of ONE replica; x: that replica's slice."""
    T = arith(S["storage"])
    a = S["stored"].astype(T)  # half -> float is exact
    xg = np.asarray(x, T)[3 * S["bcol"].astype(np.int64)[:, None] + np.arange(3)[None, :]]
    return ((a[:, :, 0] * xg[:, None, 0]) + (a[:, :, 1] * xg[:, None, 1])) + (a[:, :, 2] * xg[:, None, 2])


def row_sums(S, prod):
    """Lane l of 4 adds the products of the row's blocks l, l + 4, l + 8, ... in order, starting from 0; then (s0 + s2) + (s1 + s3); fp16 storage: times scale."""
    T = arith(S["storage"])
    browptr, nbr = S["browptr"], S["nbr"]
    lanes = np.zeros((nbr, 3, 4), T)
    if prod.shape[0]:
        lane = np.arange(4)[None, :]
        for j in range(int(-(-np.diff(browptr).max() // 4))):
            k = browptr[:-1, None] + 4 * j + lane
            inside = k < browptr[1:, None]
            p = prod[np.minimum(k, prod.shape[0] - 1)]  # (nbr, 4 lanes, 3 rows)
            lanes = lanes + np.where(inside[:, None, :], np.transpose(p, (0, 2, 1)), T(0))
    s = (lanes[:, :, 0] + lanes[:, :, 2]) + (lanes[:, :, 1] + lanes[:, :, 3])
    if S["storage"] == F16:
        s = s * T(S["scale"])
    return s.reshape(3 * nbr)


def product(S, x):
    """s = A x in T: replica q applies replica 0's matrix to slice q of x."""
    T, nr = arith(S["storage"]), S["rep_rows"]
    x = np.asarray(x, T)
    return np.concatenate([row_sums(S, block_products(S, x[q * nr:(q + 1) * nr])) for q in range(S["nrep"])])


def epilogue(epi, s, T, x, y, y1, dinv, r, c0=C0, c1=C1, c2=C2):
    """The vectors the launch writes, in T with the kernel's association: {"y": ..} and, POST1, {"r", "d"}; POST2, {"z64"}.  y: what y held before (POST2)."""
    c0, c1, c2 = T(c0), T(c1), T(c2)
    if epi == NONE:
        return dict(y=s)
    if epi == ADD:
        return dict(y=y1 + s)
    if epi == SUB:
        return dict(y=s - y1)
    if epi == PRE:
        return dict(y=(c0 * x) + ((c2 * dinv) * (y1 - s)))
    if epi == POST1:
        rr = dinv * (y1 - s)
        dd = c0 * rr
        return dict(r=rr, d=dd, y=x + dd)
    if epi == POST2:
        v = (y + (c1 * x)) + (c2 * (r - (dinv * s)))
        return dict(y=v, z64=v.astype(np.float64))
    raise ValueError(epi)


# ---- matrices -----------------------------------------------------------------------------------------------------------------------------------
def _assemble(rng, bcols_of_row, storage, wide16=False):
    """CSR of whole 3 x 3 blocks from per-block-row sorted block-column lists; at most 3 of a block's 9 entries are removed, so a block never vanishes from
    the union and 9 nblocks <= 1.5 nnz.  Entry = block-row scale * [0.5, 1.5) with a random sign; the scales span 12 decades (fp64 storage), 6 (fp32) or
    2^-6 .. 2^-3 (fp16: every entry then lies in [2^-13, 1] max|v|, the normal half range; wide16: entries 2^-30 .. 1 instead, below half's normal and
    subnormal ranges).  Every fifth scalar row with two or more entries cancels against x: the signs of its products are chosen against the running sum,
    and its last value closes the sum to ~1e-9 of it (the partial sum, hence that value, stays within one term's size; fp16: where that value would fall below 2^-12, the entry before it grows by half first).
    Returns the matrix with its x."""
    nbr = len(bcols_of_row)
    n = 3 * nbr
    T = arith(storage)
    x = (rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n)).astype(T).astype(np.float64)
    if storage == F64:
        bscale = 10.0 ** rng.uniform(-6, 6, nbr)
    elif storage == F32:
        bscale = 10.0 ** rng.uniform(-3, 3, nbr)
    else:
        bscale = 2.0 ** rng.uniform(-6, -3, nbr)
    rows_c, rows_v = [], []
    for br, bc in enumerate(bcols_of_row):
        bc = np.asarray(bc, np.int64)
        keep = np.ones((bc.size, 9), bool)
        for k in range(bc.size):
            keep[k, rng.permutation(9)[:rng.integers(0, 4)]] = False
        for r in range(3):
            kk = keep[:, 3 * r:3 * r + 3]
            c = (3 * bc[:, None] + np.arange(3)[None, :])[kk]
            mag = 2.0 ** rng.uniform(-30, 0, c.size) if wide16 else bscale[br] * rng.uniform(0.5, 1.5, c.size)
            v = mag * rng.choice([-1.0, 1.0], c.size)
            if (3 * br + r) % 5 == 0 and c.size >= 2 and not wide16:
                partial = 0.0
                for k in range(c.size - 1):
                    v[k] = -abs(v[k]) * np.sign(x[c[k]]) if partial > 0 else abs(v[k]) * np.sign(x[c[k]])
                    partial += v[k] * x[c[k]]
                if storage == F16 and abs(partial / x[c[-1]]) < 2.0 ** -12:  # the closing value would leave [2^-13, 1] max|v|: move the partial sum by half a term
                    v[-2] *= 1.5
                    partial = float(np.sum(v[:-1] * x[c[:-1]]))
                v[-1] = -partial / x[c[-1]] * (1.0 + 1e-9)
            rows_c.append(c)
            rows_v.append(v)
    lens = np.array([c.size for c in rows_c], np.int64)
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=rowptr[1:])
    col = np.concatenate(rows_c).astype(np.int32) if n and rowptr[-1] else np.zeros(0, np.int32)
    val = np.concatenate(rows_v) if n and rowptr[-1] else np.zeros(0)
    if storage == F16 and val.size and not wide16:
        a = np.abs(val)
        assert a.max() < 1.0 and a.min() >= 2.0 ** -13 * a.max(), (a.min(), a.max())
    return dict(n=n, rowptr=rowptr.astype(np.int32), col=col, val=val, x=x)


def _cols(rng, nbr, lens, halfwidth=None):
    out = []
    for i, L in enumerate(lens):
        lo, hi = (0, nbr) if halfwidth is None else (max(0, i - halfwidth), min(nbr, i + halfwidth + 1))
        if hi - lo < L:
            lo, hi = 0, nbr
        out.append(np.sort(lo + rng.permutation(hi - lo)[:int(L)]))
    return out


def ragged(storage, seed=1):
    """37 block rows of 0 .. 9 blocks, every count present (so every residue mod 4), first and last row empty; the total is odd and no multiple of 4: W = 2 and
    W = 4 both pad the single tile."""
    rng = np.random.default_rng(seed)
    lens = np.concatenate([[0], np.arange(10), rng.integers(0, 10, 25), [0]])
    while lens.sum() % 2 == 0:
        lens[20] = (lens[20] + 1) % 10
    assert lens.size == 37 and lens.sum() % 4 in (1, 3)
    return _assemble(rng, _cols(rng, 37, lens), storage)


def many_tiles(storage, seed=2):
    """700 block rows of 9 .. 19 blocks (about 9 800): more tiles than XCDs, a tile count that is no multiple of 8."""
    rng = np.random.default_rng(seed)
    return _assemble(rng, _cols(rng, 700, rng.integers(9, 20, 700), halfwidth=30), storage)


def fills_tile(storage, longest, seed=3):
    """1030 block rows of 1 block; row 300 has 512 blocks and, with longest >= 1024, row 700 has `longest`: a row that fills a tile alone (or exceeds it)."""
    rng = np.random.default_rng(seed + longest)
    lens = np.ones(1030, np.int64)
    lens[300] = 512
    if longest >= 1024:
        lens[700] = longest
    return _assemble(rng, _cols(rng, 1030, lens), storage)


def many_rows(storage, seed=4):
    """1500 block rows of 0 or 1 block, exactly 1000 blocks: at 1024 blocks per tile ONE tile of 4500 scalar rows, far beyond the 64 rows of one sweep."""
    rng = np.random.default_rng(seed)
    lens = np.zeros(1500, np.int64)
    lens[rng.permutation(1500)[:1000]] = 1
    return _assemble(rng, _cols(rng, 1500, lens, halfwidth=40), storage)


def no_entries(storage):
    return dict(n=9, rowptr=np.zeros(10, np.int32), col=np.zeros(0, np.int32), val=np.zeros(0), x=np.linspace(-1.0, 1.0, 9).astype(arith(storage)).astype(np.float64))


def fp16_range(storage, seed=5):
    """60 block rows of 3 .. 12 blocks whose entries go down to 2^-30 max|v|: below 2^-14 they are subnormal in half, below 2^-25 they round to zero."""
    rng = np.random.default_rng(seed)
    M = _assemble(rng, _cols(rng, 60, rng.integers(3, 13, 60)), storage, wide16=True)
    M["val"][0] = np.copysign(1.0, M["val"][0])  # max|v| = 1: scale 1
    return M


def replicate(M, nrep, seed=6):
    """nrep congruent copies of M on the diagonal; x differs per copy."""
    n, nnz = M["n"], int(M["rowptr"][-1])
    rng = np.random.default_rng(seed)
    rowptr = np.concatenate([[0]] + [M["rowptr"][1:].astype(np.int64) + q * nnz for q in range(nrep)])
    col = np.concatenate([M["col"].astype(np.int64) + q * n for q in range(nrep)])
    x = np.concatenate([M["x"]] + [np.float64(np.float32(rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n))) for _ in range(nrep - 1)])
    return dict(n=n * nrep, rowptr=rowptr.astype(np.int32), col=col.astype(np.int32), val=np.tile(M["val"], nrep), x=x)


def perturbed_last(M):
    """One entry of the last diagonal block changed in its last bit: the blocks are no longer congruent."""
    P = dict(M, val=M["val"].copy())
    P["val"][-1] = np.nextafter(P["val"][-1], np.inf)
    return P


# name -> (builder(storage), replicas hinted); every storage gets its own values (the block-row scales depend on it), the structure is the same
CASES = {
    "ragged": (ragged, 1),
    "many_tiles": (many_tiles, 1),
    "fills_512": (functools.partial(fills_tile, longest=512), 1),
    "fills_1024": (functools.partial(fills_tile, longest=1024), 1),
    "many_rows": (many_rows, 1),
    "ragged_x3": (lambda st: replicate(ragged(st), 3), 3),
    "many_tiles_x8": (lambda st: replicate(many_tiles(st), 8), 8),
    "no_entries": (no_entries, 1),
}


@functools.lru_cache(maxsize=None)
def case(name, storage):
    """(matrix with its x, hint).  Built once; nobody writes into it."""
    if name == "fp16_range":
        assert storage == F16
        return fp16_range(storage), 1
    build, hint = CASES[name]
    return build(storage), hint


def operands(name, storage):
    """x, y1, r and a pre-filled y of both signs, dinv > 0, all exactly representable in T (as float64 arrays; cast with .astype(T))."""
    import zlib

    M, _ = case(name, storage)
    n, T = M["n"], arith(storage)
    rng = np.random.default_rng(zlib.crc32(("%s/%d" % (name, storage)).encode()))
    amp = float(np.abs(M["val"]).max()) if M["val"].size else 1.0
    mk = lambda a: a.astype(T)  # noqa: E731
    return dict(x=mk(M["x"]), y1=mk(rng.standard_normal(n) * amp), r=mk(rng.standard_normal(n)), y=mk(rng.standard_normal(n)), dinv=mk(rng.uniform(0.1, 2.0, n) / amp))


@functools.lru_cache(maxsize=None)
def reference(name, storage):
    """(restated structure at tile 1024 with the case's hint, operands, {epilogue name: vectors written}).  The row sums are the same at both tiles."""
    M, hint = case(name, storage)
    S = restate(M, storage, 1024, hint)
    assert S is not None, name
    T, v = arith(storage), operands(name, storage)
    s = product(S, v["x"])
    out = {k: epilogue(e, s, T, v["x"], v["y"], v["y1"], v["dinv"], v["r"]) for k, e in EPILOGUES.items()}
    for d in out.values():
        for a in d.values():
            a.setflags(write=False)
    return S, v, out
