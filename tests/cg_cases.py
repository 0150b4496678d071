"""Plain numpy restatement, launch by launch and in fp64, of the block CG under the iterative K^+: the one-column solver (csrc/feti.hip: pmh_matinv_mult) and the 8-column
solver (csrc/matinv_mv.hip: pmh_matinv_mv_mult), every sum in the order the kernels fix, every scalar and stopping decision as the kernels take it.  wave_reduce and
block_reduce come from tests/dual_cases.py (pinned there); the operator product and the preconditioner are callables handed to the model.  With it the pair-coupling
matrices whose product has no order (every row sum has at most two non-zero terms, all of them exact), the loads and the case list of tests/test_gpu_cg_paths.py.
The library is built without contraction: a multiply and an add are always two roundings here.  tests/test_cg_reference_host.py ties this file to long-double
arithmetic and to a lane-by-lane simulation of the shuffles, and asserts what each case claims to reach.  No GPU here."""
import functools

import numpy as np
import scipy.sparse as sp

from dual_cases import BLOCK, MAX_BLOCKS, block_reduce, wave_reduce  # noqa: F401  (wave_reduce: the tree inside block_reduce, checked lane by lane by the host tests)

EPS = 2.220446049250313e-16
MV_R, MVC_ROWS, MAX_KDIM = 8, 32, 8
CSR, BSR3, ELL8 = 0, 1, 2  # pmh_matinv_test_info: info[1]
ONE, EIGHT, CONGRUENT = 1, 8, 9  # info[2]


# ---- launch geometry -----------------------------------------------------------------------------------------------------------------------------------------------
def wgs_one(rs):
    """pmh_matinv_create: >= 4 rows per lane, at most 256 partials per block, at most the resident-grid cap over all blocks."""
    nb = len(rs) - 1
    return max(1, min(256, MAX_BLOCKS // nb, (int(np.max(np.diff(rs))) + 1023) // 1024))


def wgs_eight(rs, num_cus=256):
    """mvc_create: 8 per CU over all blocks, at most 512 a block, 4 rows of 8 columns per thread."""
    nb = len(rs) - 1
    return max(1, min(2 * BLOCK, (max(1, int(np.max(np.diff(rs)))) + 4 * MVC_ROWS - 1) // (4 * MVC_ROWS), max(1, 8 * num_cus // max(1, nb))))


# ---- one column: SEG_LOOP, pmh_block_reduce, seg_total -------------------------------------------------------------------------------------------------------------
def seg_lane_sums(term, lo, hi, wgs):
    """SEG_LOOP: thread t of workgroup w adds the rows lo + 256 w + t, + 256 wgs, ... in that order.  -> [wgs, 256]"""
    lap = BLOCK * wgs
    nlap = max(1, -(-(hi - lo) // lap))
    v = np.zeros(nlap * lap)
    v[:hi - lo] = term[lo:hi]
    v = v.reshape(nlap, wgs, BLOCK)
    s = np.zeros((wgs, BLOCK))
    for k in range(nlap):
        s = s + v[k]  # (the zeros past the block's end add nothing)
    return s


def seg_part(term, rs, wgs):
    """One launch of a segmented sum: part[b, w] = pmh_block_reduce of workgroup (b, w)'s lane sums."""
    return np.stack([block_reduce(seg_lane_sums(term, rs[b], rs[b + 1], wgs)) for b in range(len(rs) - 1)])


def seg_total(part):
    """seg_total: thread t < wgs holds part[t], the others 0, then pmh_block_reduce.  part[..., wgs] -> [...]"""
    part = np.asarray(part, np.float64)
    v = np.zeros(part.shape[:-1] + (BLOCK,))
    v[..., :part.shape[-1]] = part
    return block_reduce(v.reshape(-1, BLOCK)).reshape(part.shape[:-1])


def seg_coef_total(part):
    """k_seg_coef's own form: thread t adds part[t], part[t + 256], ..., then pmh_block_reduce."""
    part = np.asarray(part, np.float64)
    wgs = part.shape[-1]
    nlap = -(-wgs // BLOCK)
    v = np.zeros(part.shape[:-1] + (nlap * BLOCK,))
    v[..., :wgs] = part
    v = v.reshape(part.shape[:-1] + (nlap, BLOCK))
    s = np.zeros(part.shape[:-1] + (BLOCK,))
    for k in range(nlap):
        s = s + v[..., k, :]
    return block_reduce(s.reshape(-1, BLOCK)).reshape(part.shape[:-1])


def project_one(v, R, rs, wgs, want_norm=False):
    """matinv_project: k_seg_rt_dot, k_seg_coef, k_seg_project.  R [kdim, n].  -> (v - R coef block by block, |v_b|^2 or None)"""
    kdim = R.shape[0]
    vn = seg_coef_total(seg_part(v * v, rs, wgs)) if want_norm else None
    coef = np.stack([seg_coef_total(seg_part(R[k] * v, rs, wgs)) for k in range(kdim)], axis=1)  # [nb, kdim]
    out = v.copy()
    for b in range(len(rs) - 1):
        sl = slice(rs[b], rs[b + 1])
        for k in range(kdim):
            out[sl] = out[sl] - coef[b, k] * R[k, sl]
    return out, vn


def threshold(rr, rtol, atol):
    return np.fmax(rtol * np.sqrt(rr), atol)


def solve_one(K, rs, f, dinv=None, pc=None, rtol=1e-10, atol=1e-50, max_it=10000, R=None, kernel_tol=64.0, fix=None, wgs=None):
    """pmh_matinv_mult.  K: callable p -> K p over all blocks.  dinv: Jacobi's vector (ones: none) or pc: callable r -> z (the V-cycle).  R [kdim, n] or None;
    fix: the fixing dofs of the left inverse (needs R).  -> dict u, its, active, rz, tol (per block), nactive, done."""
    rs = np.asarray(rs)
    nb, n = len(rs) - 1, len(f)
    wgs = wgs_one(rs) if wgs is None else wgs
    blk = np.repeat(np.arange(nb), np.diff(rs))
    f = np.array(f, np.float64)
    fnorm2 = None
    with np.errstate(all="ignore"):
        if R is not None:
            f, fnorm2 = project_one(f, R, rs, wgs, True)
        if fix is not None:
            f[np.asarray(fix, int)] = 0.0
        u, r = np.zeros(n), f.copy()
        z = pc(r) if pc else dinv * r
        p = z.copy()
        rz, rr = seg_total(seg_part(r * z, rs, wgs)), seg_total(seg_part(r * r, rs, wgs))
        tol = threshold(rr, rtol, atol)
        act = np.sqrt(rr) > tol
        if fnorm2 is not None:
            act &= ~(np.sqrt(rr) <= kernel_tol * EPS * np.sqrt(fnorm2))  # the load lies in the kernel
        its = np.zeros(nb, int)
        it = 0
        while it < max_it and act.any():  # (done: every later launch is a no-op)
            Ap = K(p)
            a = act[blk]
            pAp = seg_total(seg_part(np.where(a, p * Ap, 0.0), rs, wgs))
            alpha = (rz / pAp)[blk]
            r = np.where(a, r - alpha * Ap, r)
            u = np.where(a, u + alpha * p, u)
            z = pc(r) if pc else np.where(a, dinv * r, z)
            rzn, rr = seg_total(seg_part(np.where(a, r * z, 0.0), rs, wgs)), seg_total(seg_part(np.where(a, r * r, 0.0), rs, wgs))
            beta = rzn / rz
            conv = (np.sqrt(rr) <= tol) | (it + 1 >= max_it) | (rr != rr)
            go = act & ~conv
            p = np.where(go[blk], z + beta[blk] * p, p)
            rz, its = np.where(act, rzn, rz), np.where(act, it + 1, its)
            act = go
            it += 1
        if R is not None and fix is None:
            u, _ = project_one(u, R, rs, wgs)
    return dict(u=u, its=its, active=act.astype(int), rz=rz, tol=tol, nactive=int(act.sum()), done=int(not act.any()))


# ---- 8 columns: MV_ROW_LOOP, mvc_red8, mvc_total -------------------------------------------------------------------------------------------------------------------
def tree32(v):
    """mvc_red8 over the 32 rows a workgroup holds per column: xor 8, 16, 32 inside a wave and (l0 + l1) + (l2 + l3) over the waves are together the balanced tree of
    adjacent pairs.  v[..., 32, C] -> [..., C]"""
    while v.shape[-2] > 1:
        v = v[..., 0::2, :] + v[..., 1::2, :]
    return v[..., 0, :]


def mv_lane_sums(term, lo, hi, wgs):
    """MV_ROW_LOOP: thread t of workgroup w adds row lo + 32 w + t / 8, + 32 wgs, ... of column t % 8.  term [n, 8] -> [wgs, 32, 8]"""
    lap = MVC_ROWS * wgs
    nlap = max(1, -(-(hi - lo) // lap))
    v = np.zeros((nlap * lap, MV_R))
    v[:hi - lo] = term[lo:hi]
    v = v.reshape(nlap, wgs, MVC_ROWS, MV_R)
    s = np.zeros((wgs, MVC_ROWS, MV_R))
    for k in range(nlap):
        s = s + v[k]
    return s


def mv_part(term, rs, wgs):
    """-> part[b, w, c]"""
    return np.stack([tree32(mv_lane_sums(term, rs[b], rs[b + 1], wgs)) for b in range(len(rs) - 1)])


def mv_total(part):
    """mvc_total: lane t / 8 adds the partials w = t / 8, t / 8 + 32, ..., then mvc_red8.  part[b, wgs, c] -> [b, c]"""
    nb, wgs, _ = part.shape
    nlap = -(-wgs // MVC_ROWS)
    v = np.zeros((nb, nlap * MVC_ROWS, MV_R))
    v[:, :wgs] = part
    v = v.reshape(nb, nlap, MVC_ROWS, MV_R)
    s = np.zeros((nb, MVC_ROWS, MV_R))
    for k in range(nlap):
        s = s + v[:, k]
    return tree32(s)


def project_eight(v, R, rs, wgs, want_norm=False):
    """mvc_project: k_mvc_rt_dot, k_mvc_coef, k_mvc_project.  v [n, 8], R [kdim, n]"""
    kdim = R.shape[0]
    vn = mv_total(mv_part(v * v, rs, wgs)) if want_norm else None
    coef = [mv_total(mv_part(R[k][:, None] * v, rs, wgs)) for k in range(kdim)]  # [kdim][nb, 8]
    out = v.copy()
    for b in range(len(rs) - 1):
        sl = slice(rs[b], rs[b + 1])
        for k in range(kdim):
            out[sl] = out[sl] - coef[k][b][None, :] * R[k, sl][:, None]
    return out, vn


def solve_eight(K, rs, F, dinv=None, pc=None, rtol=1e-10, atol=1e-50, max_it=10000, R=None, kernel_tol=64.0, wgs=None):
    """pmh_matinv_mv_mult.  F [n, 8]; K: P [n, 8] -> K P; pc: R [n, 8] -> Z (the V-cycle's fp32 result as doubles).  A frozen column gets alpha = 0 and still feeds
    the partials (which nothing reads for it); z is written for the active columns only.  State per column c = 8 b + column."""
    rs = np.asarray(rs)
    nb, n = len(rs) - 1, F.shape[0]
    wgs = wgs_eight(rs) if wgs is None else wgs
    blk = np.repeat(np.arange(nb), np.diff(rs))
    F = np.array(F, np.float64)
    fnorm2 = None
    with np.errstate(all="ignore"):
        if R is not None:
            F, fnorm2 = project_eight(F, R, rs, wgs, True)
        U, r = np.zeros((n, MV_R)), F.copy()
        z = pc(r) if pc else dinv[:, None] * r
        p = z.copy()
        rz, rr = mv_total(mv_part(r * z, rs, wgs)), mv_total(mv_part(r * r, rs, wgs))  # [nb, 8]
        tol = threshold(rr, rtol, atol)
        act = np.sqrt(rr) > tol
        if fnorm2 is not None:
            act &= ~(np.sqrt(rr) <= kernel_tol * EPS * np.sqrt(fnorm2))
        its = np.zeros((nb, MV_R), int)
        it = 0
        while it < max_it and act.any():
            Ap = K(p)
            pAp = mv_total(mv_part(p * Ap, rs, wgs))
            a = act[blk]
            alpha = np.where(act, rz / pAp, 0.0)[blk]
            r = np.where(a, r - alpha * Ap, r)
            U = np.where(a, U + alpha * p, U)
            z = pc(r) if pc else np.where(a, dinv[:, None] * r, z)
            rzn, rr = mv_total(mv_part(r * z, rs, wgs)), mv_total(mv_part(r * r, rs, wgs))
            beta = rzn / rz
            conv = (np.sqrt(rr) <= tol) | (it + 1 >= max_it) | (rr != rr)
            go = act & ~conv
            p = np.where(go[blk], z + beta[blk] * p, p)
            rz, its = np.where(act, rzn, rz), np.where(act, it + 1, its)
            act = go
            it += 1
        if R is not None:
            U, _ = project_eight(U, R, rs, wgs)
    return dict(u=U, its=its.reshape(-1), active=act.astype(int).reshape(-1), rz=rz.reshape(-1), tol=tol.reshape(-1), nactive=int(act.sum()), done=int(not act.any()))


# ---- matrices whose product has no order -----------------------------------------------------------------------------------------------------------------------------
class PairMatrix:
    """Row i holds d = 2^e on the diagonal and at most one coupling c = +-2^(e - k), k in {1, 2, 3}, to a partner row half a block away (another 3 x 3 block as soon as
    the block has 6 rows); the partner carries the same e.  A block of odd size leaves its last row alone.  Every product term is exact and a row sum has at most two of
    them; each coupled pair is an SPD 2 x 2 matrix with the eigenvalues d -+ |c|, so Jacobi leaves at most 7 distinct ones (1, 1 -+ 2^-k)."""

    def __init__(self, sizes, erange, seed, unit_lone=False, dense3=False, singular=False):
        """dense3: the pairing for the 3 x 3-block copy of the one-column solver, whose conversion declines a matrix whose blocks are mostly empty (9 blocks > 2 nnz + 64):
        of a block's m / 3 blocks of 3 x 3 the first m / 42 are coupled row by row to the block half a block further, every other one couples its rows 0 and 1 and
        leaves row 2 alone."""
        rng = np.random.default_rng(seed)
        self.rs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self.n = n = int(self.rs[-1])
        self.i, self.j, lone = [], [], []
        for b, m in enumerate(sizes):
            lo, h = int(self.rs[b]), m // 2
            if dense3:
                nb3 = m // 3
                g = np.arange(nb3 // 14)
                far = np.concatenate([g, g + nb3 // 2])
                near = np.setdiff1d(np.arange(nb3), far)
                self.i += [lo + (3 * g[:, None] + np.arange(3)).reshape(-1), lo + 3 * near]
                self.j += [lo + (3 * (g + nb3 // 2)[:, None] + np.arange(3)).reshape(-1), lo + 3 * near + 1]
                lone.append(lo + 3 * near + 2)
            else:
                self.i.append(lo + np.arange(h))
                self.j.append(lo + h + np.arange(h))
                if m % 2:
                    lone.append(np.array([lo + m - 1]))
        self.i, self.j, self.lone = np.concatenate(self.i), np.concatenate(self.j), (np.concatenate(lone) if lone else np.zeros(0, int))
        e = np.zeros(n, int)
        e[self.i] = e[self.j] = rng.integers(erange[0], erange[1] + 1, size=self.i.size)
        e[self.lone] = 0 if unit_lone else rng.integers(erange[0], erange[1] + 1, size=self.lone.size)
        self.k = rng.integers(1, 4, size=self.i.size)
        if singular:  # the LAST pair gets |c| = d: a singular 2 x 2 matrix, p'K p = 0 exactly along (1, -sign) -- the way into the NaN exit of the iteration
            self.k[-1] = 0
        self.sign = rng.choice([-1.0, 1.0], size=self.i.size)
        self.d = np.ldexp(1.0, e)
        self.c = self.sign * np.ldexp(1.0, e[self.i] - self.k)
        self.K = sp.csr_matrix((np.concatenate([self.d, self.c, self.c]), (np.concatenate([np.arange(n), self.i, self.j]), np.concatenate([np.arange(n), self.j, self.i]))), shape=(n, n))
        self.K.sort_indices()
        self.block = np.repeat(np.arange(len(sizes)), sizes)

    def dinv(self, jacobi):
        return 1.0 / self.d if jacobi else np.ones(self.n)

    def eigen_load(self, rng, jacobi, counts):
        """A load per block that excites counts[b] distinct eigenvalues of (D^-1) K and no others: (a, a) on a pair excites d + c, (a, -a) d - c, a lone row its d.  The CG
        of that block then stops after counts[b] steps (fewer where the block has fewer eigenvalues)."""
        f = np.zeros(self.n)
        sc = (1.0 / self.d[self.i]) if jacobi else np.ones(self.i.size)
        lam = np.concatenate([(self.d[self.i] + self.c) * sc, (self.d[self.i] - self.c) * sc])  # [(1, 1) vectors | (1, -1) vectors]
        for b, m in enumerate(counts):
            mine = np.flatnonzero(self.block[self.i] == b)
            lb = np.concatenate([lam[mine], lam[self.i.size + mine]])
            pick = rng.permutation(np.unique(lb))[:m]
            for t in np.flatnonzero(np.isin(lb, pick)):
                pr, s = mine[t % mine.size], (1.0 if t < mine.size else -1.0)
                a = rng.uniform(0.5, 2.0)
                f[self.i[pr]] += a
                f[self.j[pr]] += s * a
        return f


def kernel_basis(rs, kdim, zero_block=None):
    """R [kdim, n], block-wise orthonormal with exactly representable entries: column k of a block is +-2^-j on the 4^j rows [k 4^j, (k + 1) 4^j) of the block (the largest j
    for which kdim such strips fit) and 0 elsewhere; a block with fewer than kdim rows gets unit vectors and zero columns."""
    n, R = int(rs[-1]), None
    R = np.zeros((kdim, n))
    for b in range(len(rs) - 1):
        lo, m = int(rs[b]), int(rs[b + 1] - rs[b])
        if b == zero_block:
            continue
        j = 0
        while kdim * 4 ** (j + 1) <= m:
            j += 1
        s = 4 ** j
        for k in range(min(kdim, m)):
            R[k, lo + k * s:lo + (k + 1) * s] = np.ldexp(1.0, -j) * np.where((np.arange(s) * (k + 3)) % 5 < 2, -1.0, 1.0)
    return R


INSIDE, OUTSIDE = 16.0, 1024.0  # |P_R f| / (eps |f|) of the two kernel-load cases, either side of the rule's 64


def kernel_load(R, rs, b, ratio):
    """Block b's load R_0 + ratio eps e_last: R_0' f = 1 exactly and P_R f = ratio eps e_last, so |P_R f| / (eps |f|) = ratio to rounding."""
    f = R[0, rs[b]:rs[b + 1]].copy()
    assert f[-1] == 0.0 and np.sum(f * f) == 1.0
    f[-1] = ratio * EPS
    return f


# ---- cases -----------------------------------------------------------------------------------------------------------------------------------------------------------
SCALES = np.array([1e-3, 1e-2, 1e-1, 1.0, 1e1, 1e2, 1e3, 1.0])
SHAPES_ONE = {  # name: (block sizes, the wgs the case is aimed at)
    "b3": ([3], 1),
    "b1025": ([1025], 2),
    "b65537": ([65537, 3, 1029], 65),
    "b40": ([3, 6, 9, 1029] * 9 + [3, 6, 65537, 9], 51),
}
SHAPES_BSR3 = {"b3": ([3], 1), "b1026": ([1026], 2)}
SHAPES_EIGHT = {"b3": ([3], 1), "b4101": ([4101, 3, 129], 33)}


@functools.lru_cache(maxsize=None)
def matrix(shape, wide=False, unit_lone=False, singular=False):
    sizes = dict(SHAPES_ONE, **{"3:" + k: v for k, v in SHAPES_BSR3.items()}, **{"8:" + k: v for k, v in SHAPES_EIGHT.items()})[shape][0]
    return PairMatrix(sizes, (-4, 4) if wide else (-2, 2), seed=sum(map(ord, shape)), unit_lone=unit_lone, dense3=shape.startswith("3:"), singular=singular)


def random_load(A, seed, scale_by_block=True):
    """Random entries, block b scaled by 1e-3 .. 1e3."""
    f = np.random.default_rng(seed).standard_normal(A.n)
    return f * SCALES[A.block % 8] if scale_by_block else f


def staggered_load(A, jacobi, seed):
    """Blocks that stop at different iterations: block b excites 1 + b % 5 eigenvalues."""
    nb = len(A.rs) - 1
    return A.eigen_load(np.random.default_rng(seed), jacobi, [1 + b % 5 for b in range(nb)])


def columns(A, jacobi, seed, kind="staggered"):
    """8 columns [n, 8].  staggered: column c excites 1 + c eigenvalues per block, column 6 is zero, column 7 random; scaled 1e-3 .. 1e3.  sign: one column with a single sign.
    random: all random."""
    rng = np.random.default_rng(seed)
    nb = len(A.rs) - 1
    F = np.zeros((A.n, MV_R))
    for c in range(MV_R):
        if kind == "random" or c == 7:
            F[:, c] = rng.standard_normal(A.n)
        elif c != 6:
            F[:, c] = A.eigen_load(rng, jacobi, [1 + c] * nb)
    F *= SCALES[None, :]
    if kind == "sign":
        F[:, 3] = np.abs(F[:, 7])
    return F


def breakdown_load(A, amp=1.0):
    """For a matrix built with singular = True: the kernel direction of its singular pair.  K p = 0 exactly, alpha = r'z / 0 = inf, r = r - inf 0 = NaN: the block leaves by
    the rr != rr exit after one step with u = +-inf on the pair."""
    f = np.zeros(A.n)
    f[A.i[-1]], f[A.j[-1]] = amp, -A.sign[-1] * amp
    return f


ATOL_CASE = dict(rtol=1e-10, atol=1e-6, scales=np.array([1e-9, 1e-3, 1.0, 1e5, 1e-9, 1e-3, 1.0, 1e5]))  # |f| < atol: never active; rtol |f| < atol <= |f|: atol stops it first; 1e5: rtol |f| > atol


def dense_blocks(A):
    return [A.K[A.rs[b]:A.rs[b + 1], A.rs[b]:A.rs[b + 1]].toarray() for b in range(len(A.rs) - 1)]
