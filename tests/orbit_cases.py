"""Cases, data and references for the orbit GEMM (storage "class_orbit": fxo_prepare, k_fxo_gemm16, k_fxo_fin / k_fxo_fin_all) -- numpy only, no device, no library call.

The orbit operator is defined for ANY matrix W_c that is invariant under the class's signed permutations, so a case needs no elasticity matrix and no K^+ solve: boxes of
`dims` nodes x 3 dofs, the operations of feti.box_symmetries under which the class's touched set U_c is closed, blocks that touch chosen faces of the box (one or two dual rows
of sign +-1 per touched dof) and a W_c handed to the library as it stands (MatExplicitDual.test_load_class).

Integer data: S symmetric with entries in +-{1, 2, 3}, W = sum_g D_g P_g S P_g' D_g (invariant, symmetric, integer), X of entries in +-{1, 2, 3} -- every product and every
partial sum of W X is an integer far below 2^53, hence the same bits for every summation order, row tile, segment layout, split and finishing order: the device result is
compared with == against an int64 product.  Two things the construction needs beyond the bare group sum:
  * an operation that fixes positions i and j with s_g(i) s_g(j) = -1 forces W[i][j] = 0 in EVERY invariant matrix (a node on a mirror plane: its normal component against
    a tangential one) -- forced_zero() lists those entries from the operations alone;
  * elsewhere a group sum of up to 48 terms of either sign cancels to 0 now and then; such entries get the group sum of a second (third, ...) S restricted to them, so that W
    is free of zeros wherever invariance allows a non-zero (a zero entry would hide a wrong gather index there).
  (An operation that EXCHANGES i and j with s_g(i) s_g(j) = -1 forces a zero as well, W being symmetric.)
Real data (precision): the same group sum of a standard-normal S rounded to multiples of 2^-20 (so that the 48 terms add exactly in any order and W is invariant to the
bit: the library rebuilds row g p from the representative's row p, the reference reads row g p itself), a standard-normal X, judged component by component against numpy.longdouble:
|y - ref|_i <= (n_c + 8) 2^-53 (|W| |x|)_i, the bound of a sum of n_c fused terms in any order (n_c u / (1 - n_c u) <= (n_c + 8) u for n_c u < 1e-3; derived, not measured)."""
import itertools

import numpy as np

from permon_amd.feti import box_symmetries

U53 = 2.0 ** -53
FACES = ("x0", "x1", "y0", "y1", "z0", "z1")


def face_dofs(dims, faces, comps=(0, 1, 2)):
    """Sorted block-relative dofs (node * 3 + component, x fastest) of the nodes on the given faces of a box of dims nodes; faces: names of FACES ("xm": the mid-plane of an odd edge), or "all" (every node)."""
    nx, ny, nz = dims
    nodes = np.arange(nx * ny * nz)
    ijk = (nodes % nx, (nodes // nx) % ny, nodes // (nx * ny))
    if faces == "all":
        on = np.ones(nodes.size, dtype=bool)
    else:
        on = np.zeros(nodes.size, dtype=bool)
        for f in faces:
            a = "xyz".index(f[0])
            on |= ijk[a] == {"0": 0, "1": dims[a] - 1, "m": dims[a] // 2}[f[1]]
    return np.sort((nodes[on][:, None] * 3 + np.asarray(comps)[None, :]).ravel())


class ClassSpec:
    """One block class: a box of dims nodes, blocks = one face list per block (face_dofs), extra = dofs added to the class's set (the closure where the case wants every
    operation), comps = the components the blocks touch."""

    def __init__(self, dims, blocks, extra=None, comps=(0, 1, 2)):
        self.dims, self.blocks, self.extra, self.comps = tuple(dims), list(blocks), extra, tuple(comps)


class Case:
    def __init__(self, name, classes, seed, expect, interleave=False):
        """expect: per class a dict of the structure the case is meant to have (checked on the host and, through plan_info, on the device)."""
        self.name, self.classes, self.seed, self.expect, self.interleave = name, classes, seed, expect, interleave

    def __repr__(self):
        return self.name


def _closure(dims, rel):
    perm, _ = box_symmetries(dims, 3)
    return np.unique(perm[:, rel].ravel())


class CaseData:
    """Everything a test needs, built once per case: the block layout, the gluing's leaves, per class U_c, its operations (pm, sg), the blocks' positions, W (integer and
    real)."""

    def __init__(self, case):
        self.case = case
        rng = np.random.default_rng(case.seed)
        order = []  # (class, index within the class) per block of the operator
        if case.interleave:
            for k in range(max(len(c.blocks) for c in case.classes)):
                order += [(ci, k) for ci, c in enumerate(case.classes) if k < len(c.blocks)]
        else:
            for ci, c in enumerate(case.classes):
                order += [(ci, k) for k in range(len(c.blocks))]
        self.block_class = np.array([ci for ci, _ in order], dtype=np.int32)
        self.nloc = [int(np.prod(c.dims)) * 3 for c in case.classes]
        self.block_rowstart = np.concatenate([[0], np.cumsum([self.nloc[ci] for ci, _ in order])]).astype(np.int32)
        self.N = int(self.block_rowstart[-1])
        self.nblocks = len(order)
        self.cls = []
        for ci, c in enumerate(case.classes):
            rels = [face_dofs(c.dims, f, c.comps) if not isinstance(f, np.ndarray) else np.sort(f) for f in c.blocks]
            extra = np.zeros(0, dtype=np.int64)
            if isinstance(c.extra, str) and c.extra == "closure":
                extra = _closure(c.dims, np.unique(np.concatenate(rels))) if rels and sum(r.size for r in rels) else extra
            elif isinstance(c.extra, str) and c.extra == "all":
                extra = np.arange(self.nloc[ci], dtype=np.int64)
            elif c.extra is not None:
                extra = np.asarray(c.extra, dtype=np.int64)
            urel = np.unique(np.concatenate(rels + [extra])).astype(np.int64) if rels else extra
            n_c = urel.size
            perm, sign = box_symmetries(c.dims, 3)
            pos = -np.ones(self.nloc[ci], dtype=np.int64)
            pos[urel] = np.arange(n_c)
            pm = pos[perm[:, urel]]
            keep = np.all(pm >= 0, axis=1)
            keep[0] = True
            pm, sg = pm[keep], sign[keep][:, urel].astype(np.int64)
            blocks = [b for b, (cj, _) in enumerate(order) if cj == ci]  # ascending: slot = index % 8, group = index // 8
            S = 1
            while S < 8 and S < len(blocks):
                S *= 2
            ld = (n_c + 31) // 32 * 32
            ld += 32 if ld == n_c else 0
            self.cls.append(dict(dims=c.dims, urel=urel, n_c=n_c, pm=pm, sg=sg, nsym=pm.shape[0], blocks=blocks, pos=[pos[r] for r in rels], rel=rels, extra=extra, S=S, ld=ld,
                                 groups=(len(blocks) + 7) // 8, perm=perm, sign=sign))
        xoff = 0
        for d in self.cls:
            d["xoff"] = xoff
            xoff += d["groups"] * d["ld"] * d["S"]
        self.nX = xoff
        # leaves: one or two dual rows of sign +-1 per touched dof
        self.n_lambda = 61
        rows, roots, signs = [], [], []
        for b, (ci, k) in enumerate(order):
            rel = self.cls[ci]["rel"][k]
            two = rng.integers(0, 2, size=rel.size).astype(bool)
            r1 = rng.integers(0, self.n_lambda, size=rel.size)
            r2 = (r1 + 1 + rng.integers(0, self.n_lambda - 1, size=rel.size)) % self.n_lambda  # a different dual row
            for sel, rt in ((np.ones(rel.size, dtype=bool), r1), (two, r2)):
                rows.append(self.block_rowstart[b] + rel[sel]), roots.append(rt[sel]), signs.append(rng.choice([-1.0, 1.0], size=int(sel.sum())))
        self.leaf_row = np.concatenate(rows).astype(np.int32) if rows else np.zeros(0, dtype=np.int32)
        self.leaf_root = np.concatenate(roots).astype(np.int32) if roots else np.zeros(0, dtype=np.int32)
        self.leaf_sign = np.concatenate(signs) if signs else np.zeros(0)
        self.order = order
        self._W = {}

    # ---- matrices -------------------------------------------------------------------------------------------------------------
    def W(self, ci, real=False):
        """The invariant matrix of class ci: integer (int64) or real (float64)."""
        key = (ci, real)
        if key not in self._W:
            d = self.cls[ci]
            rng = np.random.default_rng([self.case.seed, ci, int(real)])
            n = d["n_c"]
            if real:
                A = np.round(rng.standard_normal((n, n)) * 2.0 ** 20) / 2.0 ** 20  # 24 bits + 6 for 48 terms: the group sum is exact, W exactly invariant
                self._W[key] = group_sum(np.tril(A) + np.tril(A, -1).T, d["pm"], d["sg"])
            else:
                W = group_sum(_int_sym(rng, n), d["pm"], d["sg"])
                free = ~forced_zero(d["pm"], d["sg"])
                for _ in range(40):
                    zi, zj = np.nonzero((W == 0) & free)
                    if not zi.size:
                        break
                    W[zi, zj] += group_sum(_int_sym(rng, n), d["pm"], d["sg"], (zi, zj))  # the zero set is invariant and symmetric as W is: so is the sum restricted to it
                self._W[key] = W.astype(np.int64)
        return self._W[key]

    def X(self, real=False, seed=0):
        """Per block the vector on its touched positions (integer: entries of +-{1, 2, 3}, none zero; real: standard normal), as a list over the operator's blocks."""
        rng = np.random.default_rng([self.case.seed, 77, seed, int(real)])
        out = []
        for b, (ci, k) in enumerate(self.order):
            n = self.cls[ci]["pos"][k].size
            out.append(rng.standard_normal(n) if real else rng.integers(1, 4, size=n) * rng.choice([-1, 1], size=n))
        return out

    # ---- the multivector numbering: xoff + group ld S + position S + slot ----------------------------------------------------------
    def index(self, b, layout=None):
        """Multivector indices of block b's touched positions; layout: per class (xoff, ld, S) as plan_info reports them (default: this module's own restatement)."""
        ci, k = self.order[b]
        d = self.cls[ci]
        xoff, ld, S = layout[ci] if layout is not None else (d["xoff"], d["ld"], d["S"])
        j = d["blocks"].index(b)
        return xoff + (j // 8) * ld * S + d["pos"][k] * S + j % 8

    def scatter(self, xs, layout=None, dtype=np.float64):
        v = np.zeros(self.nX, dtype=dtype)
        for b, x in enumerate(xs):
            v[self.index(b, layout)] = x
        return v

    def touched_mask(self, layout=None):
        m = np.zeros(self.nX, dtype=bool)
        for b in range(self.nblocks):
            m[self.index(b, layout)] = True
        return m

    def block_slot_mask(self, layout=None):
        """Entries (position < n_c, slot of an existing block): everything else -- padding rows, slots without a block -- no block can touch."""
        m = np.zeros(self.nX, dtype=bool)
        for ci, d in enumerate(self.cls):
            xoff, ld, S = layout[ci] if layout is not None else (d["xoff"], d["ld"], d["S"])
            for j in range(len(d["blocks"])):
                m[xoff + (j // 8) * ld * S + np.arange(d["n_c"]) * S + j % 8] = True
        return m

    def reference(self, xs, real=False, layout=None):
        """Per block W[pos_b, pos_b] x_b in int64 / longdouble, placed into the multivector numbering; real: also (|W| |x|) for the bound."""
        dt = np.longdouble if real else np.int64
        ref, mag = np.zeros(self.nX, dtype=dt), np.zeros(self.nX, dtype=dt)
        for b, x in enumerate(xs):
            ci, k = self.order[b]
            p = self.cls[ci]["pos"][k]
            Wb = self.W(ci, real)[np.ix_(p, p)].astype(dt)
            ref[self.index(b, layout)] = Wb @ x.astype(dt)
            mag[self.index(b, layout)] = np.abs(Wb) @ np.abs(x.astype(dt))
        return ref, mag

    def block_matrix(self, b, real=False):
        ci, k = self.order[b]
        p = self.cls[ci]["pos"][k]
        return self.W(ci, real)[np.ix_(p, p)]

    def F_reference(self, lam):
        """B_c W B_c' lambda in int64 for an integer lambda."""
        lam = np.asarray(lam, dtype=np.int64)
        sg = self.leaf_sign.astype(np.int64)
        u = np.zeros(self.N, dtype=np.int64)
        np.add.at(u, self.leaf_row, sg * lam[self.leaf_root])
        v = np.zeros(self.N, dtype=np.int64)
        for b, (ci, k) in enumerate(self.order):
            g = self.block_rowstart[b] + self.cls[ci]["rel"][k]
            v[g] = self.block_matrix(b) @ u[g]
        y = np.zeros(self.n_lambda, dtype=np.int64)
        np.add.at(y, self.leaf_root, sg * v[self.leaf_row])
        return y


def _int_sym(rng, n):
    A = rng.integers(1, 4, size=(n, n), dtype=np.int32) * rng.choice(np.array([-1, 1], dtype=np.int32), size=(n, n))
    return np.tril(A) + np.tril(A, -1).T


def group_sum(S, pm, sg, at=None):
    """W = sum_g D_g P_g S P_g' D_g: W[g i][g j] += s_g(i) s_g(j) S[i][j]; at = (rows, columns): only those entries of W, as a vector."""
    n = S.shape[0]
    W = np.zeros_like(S) if at is None else np.zeros(at[0].size, dtype=S.dtype)
    idx = np.arange(n)
    for g in range(pm.shape[0]):
        inv = np.empty(n, dtype=np.int64)
        inv[pm[g]] = idx
        s = sg[g][inv].astype(S.dtype)
        if at is not None:
            W += S[inv[at[0]], inv[at[1]]] * s[at[0]] * s[at[1]]
            continue
        T = np.take(np.take(S, inv, axis=0), inv, axis=1)
        T *= s[:, None]
        T *= s[None, :]
        W += T
    return W


def forced_zero(pm, sg):
    """Entries (i, j) that vanish in every invariant SYMMETRIC matrix: some operation fixes i and j, or exchanges them, with s_g(i) s_g(j) = -1."""
    n = pm.shape[1]
    F = np.zeros((n, n), dtype=bool)
    idx = np.arange(n)
    for g in range(pm.shape[0]):
        fix = pm[g] == idx
        plus, minus = fix & (sg[g] > 0), fix & (sg[g] < 0)
        if plus.any() and minus.any():
            F |= plus[:, None] & minus[None, :]
            F |= minus[:, None] & plus[None, :]
        swap = (pm[g][pm[g]] == idx) & ~fix & (sg[g] * sg[g][pm[g]] < 0)  # g exchanges i and j with s_g(i) s_g(j) = -1: W[i][j] = -W[j][i], and W is symmetric
        F[idx[swap], pm[g][swap]] = True
    return F


def orbits(pm):
    """Representatives and, per row, its representative and the operation that reaches it -- restated from the definition: the rows in ascending order, a row not yet
    reached opens an orbit and claims the images nobody has claimed, operation by operation (a row fixed by several operations keeps the first)."""
    nsym, n = pm.shape
    rep_of, op_of, reps = -np.ones(n, dtype=np.int64), np.zeros(n, dtype=np.int64), []
    for p in range(n):
        if rep_of[p] >= 0:
            continue
        reps.append(p)
        for g in range(nsym):
            r = pm[g, p]
            if rep_of[r] < 0:
                rep_of[r], op_of[r] = p, g
    return np.array(reps, dtype=np.int64), rep_of, op_of


def orbit_apply(W, pm, sg, X):
    """The orbit formula from the representatives' rows alone: Y[g p] = s_g(p) sum_c W[p][c] s_g(c) X[g c] for every row g p of the orbit of p; X, Y: n_c x columns."""
    reps, rep_of, op_of = orbits(pm)
    Y = np.zeros((W.shape[0], X.shape[1]), dtype=np.result_type(W.dtype, X.dtype))
    for r in range(W.shape[0]):
        p, g = rep_of[r], op_of[r]
        Y[r] = sg[g, p] * (W[p] * sg[g]) @ X[pm[g]]
    return Y


def expected_row_tile(M, S, nsym):
    """The row tile rule restated: one-block classes (48-column kernel): 192 unless 128 or 64 pad less; otherwise the tile among 144, 128, 112, 96, 80 that pads least
    (ties: the larger)."""
    pad = lambda t: (M + t - 1) // t * t  # noqa: E731
    if S == 1 and nsym <= 48:
        tm = 192
        for t in (128, 64):
            if pad(t) < pad(tm):
                tm = t
        return tm, 48
    best = 144
    for t in (128, 112, 96, 80):
        if pad(t) < pad(best):
            best = t
    return best, 0


# ---- the cases -----------------------------------------------------------------------------------------------------------------
ALL6 = ("x0", "x1", "y0", "y1", "z0", "z1")
# eight blocks, every one its own three faces (the corners of a 2 x 2 x 2 decomposition): pruning, column lists and k segments differ from block to block
CORNER_FACES = [tuple(a + str(v) for a, v in zip("xyz", bits)) for bits in itertools.product((0, 1), repeat=3)]


def _cases():
    c = {}
    # single-class kernel: 8 blocks, S = 8
    c["box8_two_tiles"] = Case("box8_two_tiles", [ClassSpec((6, 10, 12), CORNER_FACES, "closure")], 11,
                               [dict(blocks=8, S=8, groups=1, nsym=8, M=(145, 159))])  # M strictly between 144 and 160: two row tiles, a ragged second, at every tile size
    c["cube48_three_coltiles"] = Case("cube48_three_coltiles", [ClassSpec((5, 5, 5), CORNER_FACES, "closure")], 12, [dict(blocks=8, S=8, groups=1, nsym=48)])
    c["box16_one_coltile"] = Case("box16_one_coltile", [ClassSpec((4, 4, 3), [ALL6] * 8, "closure")], 13, [dict(blocks=8, S=8, groups=1, nsym=16)])
    # two groups: 11 blocks, the second group uses 3 slots
    c["two_groups_11"] = Case("two_groups_11", [ClassSpec((4, 5, 6), (CORNER_FACES + [("x0", "y1"), ("z0",), ALL6]), "closure")], 14, [dict(blocks=11, S=8, groups=2, nsym=8)])
    # table-driven kernels: classes of 2 and 3 blocks, TN = 64 (8 / 16 operations)
    c["pair8_tn64"] = Case("pair8_tn64", [ClassSpec((6, 10, 12), [("x0", "y0", "z0"), ("x1", "y1")], "closure")], 15, [dict(blocks=2, S=2, groups=1, nsym=8, tn=64)])
    c["triple16_tn64"] = Case("triple16_tn64", [ClassSpec((7, 7, 5), [("x0", "y0", "z0"), ("x1", "z1"), ("y1",)], "closure")], 16, [dict(blocks=3, S=4, groups=1, nsym=16, tn=64)])
    # TN = 128 on the table-driven kernel: 48 operations x 2 blocks = 96 listed columns
    c["pair48_tn128"] = Case("pair48_tn128", [ClassSpec((5, 5, 5), [("x0", "y0", "z0", "x1"), ("x1", "y1", "z1")], "closure")], 17, [dict(blocks=2, S=2, groups=1, nsym=48, tn=128)])
    # one-block classes (S = 1, 48-column kernel): M in 1 .. 64, 65 .. 128, 129 .. 192 and two row tiles of 192
    c["single_tm64"] = Case("single_tm64", [ClassSpec((4, 5, 6), [("x0", "y1", "z0")], "closure")], 18, [dict(blocks=1, S=1, groups=1, nsym=8, tm=64, tnw=48, M=(1, 64))])
    c["single_tm128"] = Case("single_tm128", [ClassSpec((6, 8, 10), [("x0", "y1")], "closure")], 19, [dict(blocks=1, S=1, groups=1, nsym=8, tm=128, tnw=48, M=(65, 128))])
    c["single_tm192"] = Case("single_tm192", [ClassSpec((6, 10, 12), [("x0", "y1", "z0")], "closure")], 20, [dict(blocks=1, S=1, groups=1, nsym=8, tm=192, tnw=48, M=(129, 192))])
    c["single_two_tiles_192"] = Case("single_two_tiles_192", [ClassSpec((5, 20, 24), [("x0",)])], 21, [dict(blocks=1, S=1, groups=1, nsym=4, tm=192, tnw=48, M=(321, 384), row_tiles=2)])  # n_c = 1440: one segment of 90 chunks
    # several classes in one operator
    c["merged_two_classes"] = Case("merged_two_classes", [ClassSpec((4, 5, 6), CORNER_FACES, "closure"), ClassSpec((4, 5, 6), CORNER_FACES[::-1], "closure")], 22,
                                   [dict(blocks=8, S=8, groups=1, nsym=8, launch=2, finish=1)] * 2, interleave=True)
    c["merged_two_tiles"] = Case("merged_two_tiles", [ClassSpec((6, 10, 12), CORNER_FACES, "closure"), ClassSpec((6, 10, 12), CORNER_FACES[::-1], "closure")], 28,
                                 [dict(blocks=8, S=8, groups=1, nsym=8, launch=2, finish=1, M=(145, 159))] * 2)
    c["mixed_classes"] = Case("mixed_classes", [ClassSpec((4, 5, 6), CORNER_FACES, "closure"), ClassSpec((3, 3, 3), [np.zeros(0, dtype=np.int64)], None), ClassSpec((5, 5, 5), [("x0", "y0"), ("x1", "z1"), ("y1",)], "closure"),
                                                ClassSpec((4, 4, 3), [("x0", "z1")], "closure")], 23,
                              [dict(blocks=8, S=8, groups=1, nsym=8, launch=0, finish=1), dict(blocks=1, S=1, groups=1, n_c=0), dict(blocks=3, S=4, groups=1, nsym=48, launch=1, finish=1, tn=128),
                               dict(blocks=1, S=1, groups=1, nsym=16, launch=1, finish=1, tnw=48)], interleave=True)
    # the multi-tile 48-operation case of the plan variants (row tile 80 through PMH_FXO_TM in the tests)
    c["cube48_multi_tile"] = Case("cube48_multi_tile", [ClassSpec((11, 11, 11), [f + (("xm", "ym", "zm")[i % 3],) for i, f in enumerate(CORNER_FACES)], "closure")], 24, [dict(blocks=8, S=8, groups=1, nsym=48, M=(81, 10 ** 6))])
    # edges
    c["nc_multiple_of_32"] = Case("nc_multiple_of_32", [ClassSpec((4, 4, 4), [("x0", "y0"), ("x1", "y1", "z0"), ("z1",)], "all")], 25, [dict(blocks=3, S=4, groups=1, nsym=48, nc_mod32=0)])
    c["one_dof"] = Case("one_dof", [ClassSpec((3, 3, 3), [np.array([13 * 3 + 1])] * 2)], 26, [dict(blocks=2, S=2, groups=1, n_c=1, M=(1, 1))])
    c["one_orbit"] = Case("one_orbit", [ClassSpec((2, 2, 2), [ALL6] * 8)], 27, [dict(blocks=8, S=8, groups=1, nsym=48, n_c=24, M=(1, 1))])
    return c


CASES = _cases()
_data = {}


def data(name):
    if name not in _data:
        _data[name] = CaseData(CASES[name])
    return _data[name]
