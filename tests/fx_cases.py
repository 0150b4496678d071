"""Cases, data, layouts and references for the four streaming storages of the explicit dual operator -- "full" (k_fx_gemv), "sym" (k_fx_symv / k_fx_symv_fin),
"class" (k_fxs_gemm8 / k_fxs_fin) and "class_sym" (k_fxs_symm8 / k_fxs_symfin) -- numpy only, no device, no library call.

As in orbit_cases.py nothing here needs an elasticity matrix or a K^+ solve: K is an identity that is never solved with, the gluing is arbitrary (one to three leaves of
sign +-1 per touched dof, the dual rows drawn from a small range so that blocks share them), and the matrix of every unit -- a block for "full" / "sym", a class for the
class storages -- is handed to the library row by row (MatExplicitDual.test_load_rows).  The gluing alone decides every n_Gamma and every class union.

Data.  Integer: W and x / lambda in +-{1 .. 8} (no zeros: a zero would hide a wrong index), so every product and every partial sum is an integer (a multiple of 1/2 where
"class_sym" halves a diagonal entry) far below 2^53: exact under any summation order and with fused multiply-adds, compared with ==.  Real: standard normal, judged component
by component against numpy.longdouble.  W is a function of (unit, row range), generated range by range, so that a case of 8200 rows never holds the matrix.

W need not be symmetric.  The reference is the EFFECTIVE matrix E that the storage rule defines from the rows handed over (n = rows of the unit):
  full       E = W.
  sym        row p supplies the columns c < min(n, 32 (p // 32 + 1)) -- its band, the diagonal 32 x 32 tile in full; the entries left of that tile, c < 32 (p // 32),
             are mirrored: E[p][c] = E[c][p] = W[p][c].
  class      the kernel takes Y[c] = sum_r W[r][c] X[r]: E = W' (get_block still returns the rows as stored, W).
  class_sym  row p supplies c <= p, mirrored: E[p][c] = E[c][p] = W[p][c]; the diagonal is stored halved and counted twice.
  k_fx_store_sym (mode 1 of test_load_rows)  W := (S + S') / 2, then as "full" / "sym".
For symmetric W all of them are W.  A stripe rank's share is what its owned rows supply: their direct part plus their mirrored part; the shares add up to E.

The real-data bound.  |y - ref|_i <= (T + A) 2^-53 (|E| |x|)_i, with T the number of products of the component's sum (the padded row length) and A the longest chain of
additions that combines partial sums in that storage.  A term of the sum passes through at most k <= T + A - 1 roundings -- its own chain of (fused) multiply-adds
inside one lane or accumulator, fewer than T of them wherever partial sums are combined at all, then one rounding per combining addition -- and
gamma_k = k u / (1 - k u) <= (k + 1) u as long as k (k + 1) u <= 1; derived, not measured:
  full       a lane adds its products (rounded: one more) in column order, pmh_wave_sum is a tree of 6 levels: A = 7.
  sym        direct sums: tree of 6, then the segments of the super band one after the other in k_fx_symv_fin (at most (nsb - 1) // 2 + 1 at the shortest segment length 2);
             transposed sums: 3 additions over the waves in k_fx_symv, in k_fx_symv_fin a wave adds every fourth owned super band in turn (at most nsb // 4 + 1), 3 additions
             over the waves; both kinds meet in one register: A = 6 + 3 + (nsb // 4 + 1) + 3 + ((nsb - 1) // 2 + 1).
  class      one lane owns the column: its chain is the row segment's; k_fxs_fin adds the nseg <= 32 segment sums in order: A = 32.
  class_sym  (the fp64 matrix instruction adds four products to the accumulator: within T.)  Direct: the odd wave's sum joins the even wave's (1); transposed: 3 additions
             over the four super bands of a mega band; k_fxs_symfin: one of 8 lanes adds every eighth item's direct sum, then every eighth owned mega band's transposed sum
             (items // 8 + 1 + nmb // 8 + 1), then a tree of 3: A = 1 + 3 + items // 8 + nmb // 8 + 2 + 3, items = the most work items a mega band is cut into (at most one
             per pair of column tiles: 8 * nsb)."""
import numpy as np

U53 = 2.0 ** -53
FX_TC, FX_RB, FX_TILE = 128, 32, 32 * 128
FXM_RS, FXM_RT, FXM_MB, FXS_S = 256, 16, 4, 8
STORAGES = ("full", "sym", "class", "class_sym")


def pad_to(n, m):
    return (n + m - 1) // m * m


def ld_of(storage, n):
    return pad_to(n, FXM_RS if storage == "class_sym" else FX_TC)


# ---- layouts -------------------------------------------------------------------------------------------------------------------------
def fx_band_tiles(k):
    """Tiles of 32 x 128 before band k of the "sym" storage (band j has j // 4 + 1 of them)."""
    return (k // 4 + 1) * (2 * (k // 4) + (k & 3))


def fx_band_off(k):
    return FX_TILE * fx_band_tiles(k)


def storage_size(storage, n):
    ld = ld_of(storage, n)
    if storage == "sym":
        return fx_band_off(ld // FX_RB)
    if storage == "class_sym":
        nsb = ld // FXM_RS
        return FXM_RS * FXM_RS * (nsb * (nsb + 1) // 2)
    return ld * ld


def stored_mask(storage, n, p, c):
    """Whether entry (p, c) of the unit's matrix is kept (p, c broadcastable index arrays)."""
    if storage == "sym":
        return c < np.minimum(n, FX_RB * (p // FX_RB + 1))
    if storage == "class_sym":
        return c <= p
    return np.ones(np.broadcast(p, c).shape, dtype=bool)


def offsets(storage, n, p, c):
    """Offset (doubles, from the unit's start in the dense allocation) of the stored entry (p, c)."""
    ld = ld_of(storage, n)
    p, c = np.asarray(p, dtype=np.int64), np.asarray(c, dtype=np.int64)
    if storage in ("full", "class"):
        return p * ld + c
    if storage == "sym":  # band -> tile (32 rows x 128 columns, contiguous) -> row-major inside the tile
        k = p // FX_RB
        kq, kr = k // 4, k & 3
        return FX_TILE * ((kq + 1) * (2 * kq + kr) + c // FX_TC) + (p % FX_RB) * FX_TC + c % FX_TC
    sb, Il, r = p // FXM_RS, (p % FXM_RS) // 16, p & 15  # super band -> column tile -> row tile -> (q >> 1) 128 + 2 l + (q & 1)
    q, l = r >> 2, 16 * (r & 3) + (c & 15)
    return FXM_RS * FXM_RS * (sb * (sb + 1) // 2) + ((c >> 4) * FXM_RT + Il) * 256 + (q >> 1) * 128 + 2 * l + (q & 1)


def pack_rows(storage, n, row0, rows, own=None):
    """(offsets, values) of the stored entries of the rows row0 .. of the unit's matrix (rows: k x n; own: mask of the rows that are kept at all); "class_sym" halves
    the diagonal."""
    rows = np.asarray(rows)
    p = (row0 + np.arange(rows.shape[0], dtype=np.int64))[:, None]
    c = np.arange(n, dtype=np.int64)[None, :]
    keep = stored_mask(storage, n, p, c)
    if own is not None:
        keep = keep & np.asarray(own, dtype=bool)[:, None]
    vals = rows.astype(np.float64)
    if storage == "class_sym":
        vals = np.where(c == p, 0.5 * vals, vals)
    pp, cc = np.broadcast_arrays(p, c)
    return offsets(storage, n, pp[keep], cc[keep]), vals[keep]


def pack(storage, W):
    """The whole stored image of a unit (pads zero)."""
    n = W.shape[0]
    img = np.zeros(storage_size(storage, n))
    off, val = pack_rows(storage, n, 0, W)
    img[off] = val
    return img


def unpack(storage, n, img):
    """What get_block reads back from a stored image: the rows as stored, the mirrored part filled in."""
    p, c = np.meshgrid(np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64), indexing="ij")
    keep = stored_mask(storage, n, p, c)
    out = np.zeros((n, n))
    out[keep] = img[offsets(storage, n, p[keep], c[keep])]
    if storage == "sym":
        mir = keep & (c < FX_RB * (p // FX_RB))
        out[c[mir], p[mir]] = out[p[mir], c[mir]]
    if storage == "class_sym":
        mir = c < p
        out[c[mir], p[mir]] = out[p[mir], c[mir]]
        out[np.arange(n), np.arange(n)] *= 2.0
    return out


def effective(storage, W):
    """The matrix the storage's product applies, from the rows handed over (module docstring)."""
    n = W.shape[0]
    if storage == "full":
        return W.copy()
    if storage == "class":
        return W.T.copy()
    p, c = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    E = np.where(stored_mask(storage, n, p, c), W, 0)
    mir = c < (FX_RB * (p // FX_RB) if storage == "sym" else p)
    E[c[mir], p[mir]] = W[p[mir], c[mir]]
    return E


# ---- ownership -----------------------------------------------------------------------------------------------------------------------
def sym_stripe_owner(ngam, size):
    """fx_stripe_plan restated: the super bands (128 rows) of all blocks are counted from the largest index down, blocks in order inside one index, and dealt round
    robin.  Per block the owner of every super band."""
    nsb = [pad_to(n, FX_TC) // FX_TC for n in ngam]
    owner = [np.full(k, -1, dtype=np.int64) for k in nsb]
    idx = 0
    for sb in range(max(nsb + [0]) - 1, -1, -1):
        for b in range(len(ngam)):
            if sb < nsb[b]:
                owner[b][sb] = idx % size
                idx += 1
    return owner


def class_row_range(n_c, rank, size):
    """"class": contiguous row ranges in groups of 32 rows of the padded matrix."""
    nrg = pad_to(n_c, FX_TC) // 32
    return (nrg * rank // size) * 32, (nrg * (rank + 1) // size) * 32


def class_sym_owner(n_c, size):
    """"class_sym": mega bands of 1024 rows dealt from the longest down in snake order."""
    nsb = pad_to(n_c, FXM_RS) // FXM_RS
    nmb = (nsb + FXM_MB - 1) // FXM_MB
    out = np.zeros(nmb, dtype=np.int64)
    for m in range(nmb):
        i = nmb - 1 - m
        rnd, k = divmod(i, size)
        out[m] = size - 1 - k if rnd & 1 else k
    return out


def owned_rows(storage, ngam, unit, stripe):
    """Boolean mask over the rows of `unit` that the stripe rank assembles and applies (stripe None: all)."""
    n = ngam[unit]
    own = np.ones(n, dtype=bool)
    if stripe is None or storage == "full":
        return own
    rank, size = stripe
    p = np.arange(n)
    if storage == "sym":
        return sym_stripe_owner(ngam, size)[unit][p // FX_TC] == rank
    if storage == "class":
        r0, r1 = class_row_range(n, rank, size)
        return (p >= r0) & (p < r1)
    return class_sym_owner(n, size)[p // (FXM_MB * FXM_RS)] == rank


# ---- the bound -----------------------------------------------------------------------------------------------------------------------
def bound_factor(storage, n, items=None):
    """T + A of the module docstring for a unit of n rows; items ("class_sym"): the most work items a mega band is cut into (default: the most there can be)."""
    ld = ld_of(storage, n)
    if storage == "full":
        return ld + 7
    if storage == "sym":
        nsb = ld // FX_TC
        return ld + 6 + 3 + (nsb // 4 + 1) + 3 + ((nsb - 1) // 2 + 1)
    if storage == "class":
        return ld + 32
    nsb = ld // FXM_RS
    nmb = (nsb + FXM_MB - 1) // FXM_MB
    items = 8 * nsb if items is None else items
    return ld + 1 + 3 + items // 8 + nmb // 8 + 2 + 3


# ---- signed permutation groups (the "class_sym" set-up by symmetry) ------------------------------------------------------------------------
def klein_group(n, rng):
    """A signed permutation group of order 4 on n positions (n a multiple of 4): a = the reversal p -> n - 1 - p, b = the exchange inside the pairs (2 i, 2 i + 1); they
    commute, and with signs constant on every orbit {p, a p, b p, a b p} so do the signed operations.  (pm, sg)[g][p]: image and sign, g = e, a, b, ab."""
    assert n % 4 == 0
    p = np.arange(n)
    a, b = n - 1 - p, p ^ 1
    orbit = np.minimum(np.minimum(p, a), np.minimum(b, a[b]))
    sa, sb = rng.choice([-1, 1], size=n)[orbit], rng.choice([-1, 1], size=n)[orbit]
    return np.stack([p, a, b, a[b]]).astype(np.int64), np.stack([np.ones(n, dtype=np.int64), sa, sb, sa * sb]).astype(np.int64)


def group_sum(S, pm, sg):
    """W = sum_g D_g P_g S P_g' D_g: invariant under the group, symmetric and integer as S is."""
    n = S.shape[0]
    W = np.zeros_like(S)
    for g in range(pm.shape[0]):
        inv = np.empty(n, dtype=np.int64)
        inv[pm[g]] = np.arange(n)
        s = sg[g][inv]
        W += S[np.ix_(inv, inv)] * s[:, None] * s[None, :]
    return W


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
class Case:
    """storage; units: FULL / SYM: one n_Gamma per block; class storages: (n_c, blocks of the class) per class.  symmetric: W = W'; group: a class with the order-4
    group (its W is invariant); chunk: rows per generated / loaded range."""

    def __init__(self, name, storage, units, seed, symmetric=True, group=False, chunk=512, expect=None):
        self.name, self.storage, self.units, self.seed, self.symmetric, self.group, self.chunk, self.expect = name, storage, list(units), seed, symmetric, group, chunk, expect or {}

    def __repr__(self):
        return self.name


class CaseData:
    """Block layout, gluing, touched sets, the unit matrices range by range, vectors, references."""

    def __init__(self, case):
        self.case, self.storage = case, case.storage
        self.cls = case.storage in ("class", "class_sym")
        rng = np.random.default_rng(case.seed)
        self.n_lambda = 37
        rel, nloc, bclass = [], [], []
        self.urel, self.cblocks = [], []
        if self.cls:
            b = 0
            for ci, (n_c, nblocks) in enumerate(case.units):
                nl = n_c + 5
                u = np.sort(rng.choice(nl, size=n_c, replace=False)).astype(np.int64)
                self.urel.append(u)
                self.cblocks.append(list(range(b, b + nblocks)))
                touched = np.zeros(n_c, dtype=bool)
                for k in range(nblocks):  # every block its own part of the union; the last one takes what nobody touched
                    t = rng.random(n_c) < 0.7 if nblocks > 1 else np.ones(n_c, dtype=bool)
                    if k == nblocks - 1:
                        t |= ~touched
                    touched |= t
                    rel.append(u[t]), nloc.append(nl), bclass.append(ci)
                b += nblocks
            self.n_unit = [int(n_c) for n_c, _ in case.units]
        else:
            for n in case.units:
                nl = n + 7
                rel.append(np.sort(rng.choice(nl, size=n, replace=False)).astype(np.int64)), nloc.append(nl), bclass.append(len(bclass))
            self.n_unit = [int(n) for n in case.units]
        self.rel, self.nblocks = rel, len(rel)
        self.block_class = np.array(bclass, dtype=np.int32)
        self.block_rowstart = np.concatenate([[0], np.cumsum(nloc)]).astype(np.int32)
        self.N = int(self.block_rowstart[-1])
        self.ngam = [int(r.size) for r in rel]
        self.ld = [ld_of(case.storage, n) for n in self.n_unit]
        # positions of a block's touched dofs in its unit's numbering
        if self.cls:
            self.pos = []
            for b in range(self.nblocks):
                lut = -np.ones(nloc[b], dtype=np.int64)
                lut[self.urel[bclass[b]]] = np.arange(self.n_unit[bclass[b]])
                self.pos.append(lut[rel[b]])
            self.groups = [(len(cb) + FXS_S - 1) // FXS_S for cb in self.cblocks]
            self.xoff = np.concatenate([[0], np.cumsum([g * ld * FXS_S for g, ld in zip(self.groups, self.ld)])]).astype(np.int64)
            self.woff = np.concatenate([[0], np.cumsum([storage_size(case.storage, n) for n in self.n_unit])]).astype(np.int64)
            self.nX = int(self.xoff[-1])
        else:
            self.pos = [np.arange(n, dtype=np.int64) for n in self.ngam]
            self.xoff = np.concatenate([[0], np.cumsum(self.ld)]).astype(np.int64)
            self.woff = np.concatenate([[0], np.cumsum([storage_size(case.storage, n) for n in self.n_unit])]).astype(np.int64)
            self.nX = int(self.xoff[-1])
        # leaves: one to three dual rows of sign +-1 per touched dof
        rows, roots, signs = [], [], []
        for b in range(self.nblocks):
            k = rng.integers(1, 4, size=rel[b].size)
            r = np.repeat(self.block_rowstart[b] + rel[b], k)
            rows.append(r), roots.append(rng.integers(0, self.n_lambda, size=r.size)), signs.append(rng.choice([-1.0, 1.0], size=r.size))
        self.leaf_row = np.concatenate(rows).astype(np.int32)
        self.leaf_root = np.concatenate(roots).astype(np.int32)
        self.leaf_sign = np.concatenate(signs)
        self.sym_group = None
        if case.group:
            self.sym_group = [klein_group(n, np.random.default_rng([case.seed, 5, u])) if n else None for u, n in enumerate(self.n_unit)]
        self._W = {}

    # ---- the unit matrices, by row ranges -----------------------------------------------------------------------------------------------
    def unit_of(self, b):
        return int(self.block_class[b]) if self.cls else b

    def W_rows(self, unit, row0, row1, real=False, variant=0):
        """Rows [row0, row1) of the unit's matrix (int64 or float64).  Symmetric cases and the group case build the whole (small) matrix once; the others draw every
        range of case.chunk rows from its own generator, so no more than a range is ever held."""
        n, case = self.n_unit[unit], self.case
        if case.symmetric or case.group:
            key = (unit, real, variant)
            if key not in self._W:
                rng = np.random.default_rng([case.seed, 11, unit, int(real), variant])
                A = rng.standard_normal((n, n)) if real else rng.integers(1, 9, size=(n, n)) * rng.choice([-1, 1], size=(n, n))
                if case.group:
                    pm, sg = self.sym_group[unit]
                    A = np.round(A * 2.0 ** 20) / 2.0 ** 20 if real else rng.integers(1, 3, size=(n, n)) * rng.choice([-1, 1], size=(n, n))  # four terms of at most 2; exact sums
                    A = group_sum(np.tril(A) + np.tril(A, -1).T, pm, sg)
                else:
                    A = np.tril(A) + np.tril(A, -1).T
                self._W[key] = A
            return self._W[key][row0:row1]
        assert row0 % case.chunk == 0 and row1 <= min(n, row0 + case.chunk)
        key = (unit, real, variant, row0)
        if key not in self._W:  # (kept until drop(): integers as int8)
            rng = np.random.default_rng([case.seed, 13, unit, int(real), variant, row0 // case.chunk])
            k = min(case.chunk, n - row0)
            self._W[key] = rng.standard_normal((k, n)) if real else (rng.integers(1, 9, size=(k, n), dtype=np.int8) * rng.choice(np.array([-1, 1], dtype=np.int8), size=(k, n)))
        A = self._W[key][:row1 - row0]
        return A if real else A.astype(np.int64)

    def drop(self):
        """Forget the generated matrices (a large case holds a few hundred MB of them)."""
        self._W.clear()


    def ranges(self, unit):
        n = self.n_unit[unit]
        return [(a, min(n, a + self.case.chunk)) for a in range(0, n, self.case.chunk)]

    def W(self, unit, real=False, variant=0):
        n = self.n_unit[unit]
        return np.concatenate([self.W_rows(unit, a, b, real, variant) for a, b in self.ranges(unit)]) if n else np.zeros((0, 0), dtype=np.float64 if real else np.int64)

    # ---- vectors: the compressed numbering (FULL / SYM) or the multivector numbering (class storages) ---------------------------------------------
    def index(self, b):
        if not self.cls:
            return self.xoff[b] + self.pos[b]
        c = self.unit_of(b)
        j = self.cblocks[c].index(b)
        return self.xoff[c] + (j // FXS_S) * self.ld[c] * FXS_S + self.pos[b] * FXS_S + j % FXS_S

    def column(self, b):
        """Every entry of the output that belongs to block b: its touched positions (FULL / SYM); class storages: all n_c positions of its slot -- the product fills the
        whole column of W_c X, whether the block touches a position or not (the operator reads the touched ones)."""
        if not self.cls:
            return self.index(b)
        c = self.unit_of(b)
        j = self.cblocks[c].index(b)
        return self.xoff[c] + (j // FXS_S) * self.ld[c] * FXS_S + np.arange(self.n_unit[c], dtype=np.int64) * FXS_S + j % FXS_S

    def X(self, real=False, seed=0):
        rng = np.random.default_rng([self.case.seed, 17, seed, int(real)])
        return [rng.standard_normal(n) if real else rng.integers(1, 9, size=n) * rng.choice([-1, 1], size=n) for n in self.ngam]

    def scatter(self, xs):
        v = np.zeros(self.nX)
        for b, x in enumerate(xs):
            v[self.index(b)] = x
        return v

    def column_mask(self):
        """The entries some block's column covers; everything else -- padding rows, slots without a block -- must stay exactly zero."""
        m = np.zeros(self.nX, dtype=bool)
        for b in range(self.nblocks):
            m[self.column(b)] = True
        return m

    # ---- references --------------------------------------------------------------------------------------------------------------------
    def apply_unit(self, unit, Xu, real=False, variant=0, stripe=None, dtype=None, W_override=None):
        """E_unit Xu (Xu: n x columns) and |E| |Xu|, range by range from the rows handed over, in int64 (integer data: the halved diagonal of "class_sym" is added as
        diagonal * x, once) or numpy.longdouble; stripe = (rank, size): that rank's share."""
        st, n = self.storage, self.n_unit[unit]
        dt = dtype or (np.longdouble if real else np.int64)
        Xu = Xu.astype(dt)
        ref, mag = np.zeros(Xu.shape, dtype=dt), np.zeros(Xu.shape, dtype=dt)
        own = owned_rows(st, self.n_unit, unit, stripe)
        for a, b in self.ranges(unit):
            Wc = (W_override[a:b] if W_override is not None else self.W_rows(unit, a, b, real, variant)).astype(dt)
            Wc = Wc * own[a:b, None].astype(dt)
            p, c = np.arange(a, b)[:, None], np.arange(n)[None, :]
            if st == "full":
                D, M = Wc, None
            elif st == "class":
                D, M = None, Wc
            elif st == "sym":
                D, M = Wc * stored_mask(st, n, p, c), Wc * (c < FX_RB * (p // FX_RB))
            else:
                D, M = Wc * (c <= p), Wc * (c < p)
            if D is not None:
                ref[a:b] += D @ Xu
                mag[a:b] += np.abs(D) @ np.abs(Xu)
            if M is not None:
                ref += M.T @ Xu[a:b]
                mag += np.abs(M).T @ np.abs(Xu[a:b])
        return ref, mag

    def reference(self, xs, real=False, variant=0, stripe=None, dtype=None, W_override=None):
        """blockdiag(E) x in the numbering of dense_mult, and |E| |x|.  W_override: {unit: matrix} instead of W_rows."""
        dt = dtype or (np.longdouble if real else np.int64)
        ref, mag = np.zeros(self.nX, dtype=dt), np.zeros(self.nX, dtype=dt)
        units = range(len(self.n_unit))
        for u in units:
            n = self.n_unit[u]
            if not n:
                continue
            blocks = self.cblocks[u] if self.cls else [u]
            Xu = np.zeros((n, len(blocks)), dtype=dt)
            for j, b in enumerate(blocks):
                Xu[self.pos[b], j] = xs[b]
            r, m = self.apply_unit(u, Xu, real, variant, stripe, dt, None if W_override is None else W_override[u])
            for j, b in enumerate(blocks):
                ref[self.column(b)], mag[self.column(b)] = (r[self.pos[b], j], m[self.pos[b], j]) if not self.cls else (r[:, j], m[:, j])
        return ref, mag

    def block_matrix(self, b, real=False, variant=0, stored=False):
        """What get_block returns for block b: the effective matrix on the block's touched positions ("class": the rows as stored, i.e. W itself)."""
        u = self.unit_of(b)
        W = self.W(u, real, variant)
        E = W if (stored or self.storage == "class") else effective(self.storage, W)
        return E[np.ix_(self.pos[b], self.pos[b])]

    def F_reference(self, lam, variant=0):
        """B E B' lambda in int64 for an integer lambda (through the same range-by-range product)."""
        lam = np.asarray(lam, dtype=np.int64)
        sg = self.leaf_sign.astype(np.int64)
        u = np.zeros(self.N, dtype=np.int64)
        np.add.at(u, self.leaf_row, sg * lam[self.leaf_root])
        xs = [u[self.block_rowstart[b] + self.rel[b]] for b in range(self.nblocks)]
        ref, _ = self.reference(xs, False, variant)
        v = np.zeros(self.N, dtype=np.int64)
        for b in range(self.nblocks):
            v[self.block_rowstart[b] + self.rel[b]] = ref[self.index(b)]
        y = np.zeros(self.n_lambda, dtype=np.int64)
        np.add.at(y, self.leaf_root, sg * v[self.leaf_row])
        return y

    def bound(self, mag, items=None):
        """(T + A) 2^-53 (|E| |x|) over the numbering of dense_mult."""
        f = np.zeros(self.nX)
        for b in range(self.nblocks):
            u = self.unit_of(b)
            f[self.column(b)] = bound_factor(self.storage, self.n_unit[u], None if items is None else items[u])
        return f * U53 * mag.astype(np.float64)

    def image(self, unit, real=False, variant=0, stripe=None, W_override=None):
        """The unit's stored image (pads zero), the rows of other ranks' stripes left out."""
        n = self.n_unit[unit]
        img = np.zeros(storage_size(self.storage, n))
        own = owned_rows(self.storage, self.n_unit, unit, stripe)
        for a, b in self.ranges(unit):
            rows = W_override[a:b] if W_override is not None else self.W_rows(unit, a, b, real, variant)
            off, val = pack_rows(self.storage, n, a, rows, own[a:b])
            img[off] = val
        return img


def _cases():
    c = {}

    def add(*a, **k):
        c[a[0]] = Case(*a, **k)
    # FULL: ld = 128 / 256 / 384 (tail only, one double trip, trip plus tail), n no multiple of 16 or 4, an empty block, non-congruent blocks
    add("full_0_1_33", "full", (0, 1, 33), 101)
    add("full_127_128_129", "full", (127, 128, 129), 102, symmetric=False)
    add("full_5_0_260", "full", (5, 0, 260), 103, symmetric=False)
    # SYM
    add("sym_0_1_33", "sym", (0, 1, 33), 111)
    add("sym_127_128_129", "sym", (127, 128, 129), 112)
    add("sym_5_0_260", "sym", (5, 0, 260), 113)
    add("sym_300", "sym", (300,), 114, expect=dict(bands=3, last_segments=2))
    add("sym_300_unsym", "sym", (300,), 115, symmetric=False, expect=dict(bands=3, last_segments=2))
    add("sym_2177", "sym", (2177,), 116, symmetric=False, expect=dict(bands=18))
    add("sym_4230", "sym", (4230,), 117, symmetric=False, expect=dict(bands=34))
    add("sym_129_300", "sym", (129, 300), 118, symmetric=False)
    add("sym_100_100", "sym", (100, 100), 119)
    # CLASS: nseg = maxrows / 16 = 8, 16, 32 (the plain loop, one unrolled trip, four of k_fxs_fin); 700: segments of 24 rows
    add("class_100", "class", ((100, 3),), 121, symmetric=False, expect=dict(nseg=8))
    add("class_129", "class", ((129, 3),), 122, expect=dict(nseg=16))
    add("class_700", "class", ((700, 3),), 123, symmetric=False, expect=dict(nseg=32))
    add("class_9_blocks", "class", ((129, 9),), 124, expect=dict(groups=2))
    add("class_two_and_untouched", "class", ((100, 2), (0, 1), (129, 3)), 125, symmetric=False)
    add("class_300", "class", ((300, 3),), 126, symmetric=False)  # stripes of 3
    # CLASS_SYM
    add("csym_100", "class_sym", ((100, 3),), 131, expect=dict(super_bands=1, bands=1))
    add("csym_257", "class_sym", ((257, 3),), 132, expect=dict(super_bands=2, bands=1))
    add("csym_257_unsym", "class_sym", ((257, 3),), 133, symmetric=False)
    add("csym_1025", "class_sym", ((1025, 2),), 134, symmetric=False, expect=dict(super_bands=5, bands=2))
    add("csym_1300", "class_sym", ((1300, 2),), 135, symmetric=False, expect=dict(super_bands=6, bands=2))
    add("csym_8200", "class_sym", ((8200, 1),), 136, symmetric=False, chunk=256, expect=dict(super_bands=33, bands=9))
    add("csym_9_blocks", "class_sym", ((257, 9),), 137, expect=dict(groups=2))
    add("csym_untouched", "class_sym", ((0, 2), (100, 2)), 138)
    add("csym_group", "class_sym", ((300, 3),), 139, group=True)
    add("csym_4_megabands", "class_sym", ((3100, 1),), 140, symmetric=False, expect=dict(bands=4))
    add("csym_2_megabands", "class_sym", ((1100, 2),), 141, symmetric=False, expect=dict(bands=2))
    return c


CASES = _cases()
_data = {}


def data(name):
    if name not in _data:
        _data[name] = CaseData(CASES[name])
    return _data[name]
