"""Inputs and references shared by tests/test_gpu_mg_paths.py and tests/test_mg_reference_host.py (no test in here, no GPU): a numpy restatement of the multigrid
V-cycle of csrc/mg.hip (one column: mg_cycle / mg_level_fused / mg_smooth) and csrc/mg_mv.hip (8 interleaved columns: mvg_cycle) -- what pmh_mg_create decides
per level, k_mg_dinv, the Chebyshev constants, every smoothing, transfer and coarse kernel in its own association -- and the synthetic hierarchies each case is
built from.  The operator products and their epilogues come from tests/bsr3_cases.py and tests/mv_cases.py.

The library is compiled with -ffp-contract=off and every sum in these kernels has a fixed order, so the restatement is bit for bit what the device must return,
with ONE exception: the order of the four k-slots inside the matrix-core instruction of k_mvg_coarse_mfma is not written in the source; that kernel is compared on
dyadic data (exact in any order) and against an a-priori bound.

The cycle is a linear operator whatever the matrices are: the hierarchies here are neither Galerkin nor positive definite and coarse_pinv inverts nothing, which
keeps every case at a few hundred to a few thousand rows."""
import functools
import zlib

import numpy as np

import bsr3_cases as BC
import mv_cases as MC
from bsr3_cases import F16, F32, F64  # noqa: F401

R = MC.R
PRECISIONS = {"fp64": 0, "fp32": 1, "fp16": 2}  # PMH_MG_FP64 / FP32 / FP16
NONE_T, NODAL, SHORT, LONG = 0, 1, 2, 3  # pmh_mg_test_info's transfer kernels
MV_NONE, MV_NODAL, MV_ELL, MV_SCALAR = 0, 1, 2, 3  # pmh_mg_mv_test_info's
COARSE_F32, COARSE_F16, COARSE_MFMA = 0, 1, 2
X, B, RR, D, TT, XA, DINV = range(7)  # pmh_mg_test_vector's `which`
WHICH = dict(x=X, b=B, r=RR, d=D, t=TT, xa=XA, dinv=DINV)
LO, HI = 0.1, 1.1  # the window fractions pa.MG passes


class Unsupported(Exception):
    """What pmh_mg_create / pmh_mg_mv_create refuse (PMH_ERR_SUP); the text holds the library's reason."""


# ---- small pieces -------------------------------------------------------------------------------------------------------------------------------
def csr(nrows, ncols, rows):
    """CSR dict from per-row (columns, values) with ascending columns."""
    lens = np.array([len(c) for c, _ in rows], np.int64)
    rowptr = np.zeros(nrows + 1, np.int64)
    np.cumsum(lens, out=rowptr[1:])
    col = np.concatenate([np.asarray(c, np.int64) for c, _ in rows]) if rowptr[-1] else np.zeros(0, np.int64)
    val = np.concatenate([np.asarray(v, np.float64) for _, v in rows]) if rowptr[-1] else np.zeros(0)
    return dict(nrows=nrows, ncols=ncols, n=nrows, rowptr=rowptr.astype(np.int32), col=col.astype(np.int32), val=val)


def transpose(M):
    """pmh_csr_ensure_transpose: row j of M' lists the rows of M that hold column j, ascending (a counting sort keeps M's row order)."""
    nnz = int(M["rowptr"][-1])
    row = np.repeat(np.arange(M["nrows"], dtype=np.int64), np.diff(M["rowptr"]))
    order = np.argsort(M["col"][:nnz], kind="stable")
    rowptr = np.zeros(M["ncols"] + 1, np.int64)
    np.cumsum(np.bincount(M["col"][:nnz], minlength=M["ncols"]), out=rowptr[1:])
    return dict(nrows=M["ncols"], ncols=M["nrows"], n=M["ncols"], rowptr=rowptr.astype(np.int32), col=row[order].astype(np.int32), val=M["val"][:nnz][order])


def lane_sums(rowptr, terms, nlanes):
    """(nrows, nlanes, ...) in the dtype of terms: lane q of a row adds the row's terms q, q + nlanes, q + 2 nlanes, ... in that order, starting from +0."""
    rowptr = np.asarray(rowptr, np.int64)
    nrows, lens = len(rowptr) - 1, np.diff(rowptr)
    out = np.zeros((nrows, nlanes) + terms.shape[1:], terms.dtype)
    if nrows == 0 or terms.shape[0] == 0:
        return out
    lane = np.arange(nlanes)[None, :]
    tail = (None,) * (terms.ndim - 1)
    for j in range(int(-(-lens.max() // nlanes))):
        rows = np.flatnonzero(lens > nlanes * j)
        k = rowptr[rows, None] + nlanes * j + lane
        inside = k < rowptr[rows + 1, None]
        p = terms[np.minimum(k, terms.shape[0] - 1)]
        out[rows] = out[rows] + np.where(inside[(slice(None), slice(None)) + tail], p, terms.dtype.type(0))
    return out


def tree_halving(lanes):
    """Lane 0 after s += shfl(s, L/2), ..., s += shfl(s, 1) (shfl_down, or shfl_xor with descending offsets): (..((s_0 + s_L/2) + (s_L/4 + s_3L/4)) + ..)."""
    while lanes.shape[1] > 1:
        h = lanes.shape[1] // 2
        lanes = lanes[:, :h] + lanes[:, h:]
    return lanes[:, 0]


def tree_adjacent(groups):
    """Group 0 after shfl_xor with ASCENDING offsets over the groups: ((g0 + g1) + (g2 + g3)) + ((g4 + g5) + (g6 + g7))."""
    while groups.shape[1] > 1:
        groups = groups[:, 0::2] + groups[:, 1::2]
    return groups[:, 0]


def dinv_of(A, T):
    """k_mg_dinv: 1 / the LAST stored entry (i, i) of row i, computed in double and then cast; 1 where the row stores none or stores 0.0."""
    n, rowptr = A["nrows"], A["rowptr"].astype(np.int64)
    nnz = int(rowptr[-1])
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    k = np.flatnonzero(A["col"][:nnz] == row)
    d = np.zeros(n)
    d[row[k]] = A["val"][k]  # ascending k: the last one stays
    with np.errstate(divide="ignore"):
        return np.where(d != 0.0, 1.0 / d, 1.0).astype(T)


def cheb_constants(lam, degree, lo=LO, hi=HI):
    """theta, delta, c1[j], c2[j] as pmh_mg_create computes them in double."""
    a, b = lo * lam, hi * lam
    theta, delta = 0.5 * (a + b), 0.5 * (b - a)
    sigma = theta / delta
    rho = 1.0 / sigma
    c1, c2 = [0.0] * degree, [0.0] * degree
    for j in range(1, degree):
        rho_new = 1.0 / (2.0 * sigma - rho)
        c1[j], c2[j] = rho_new * rho, 2.0 * rho_new / delta
        rho = rho_new
    return theta, delta, c1, c2


def nodal_transfer(P):
    """mg_build_nodal_transfer: (P_node, P_node') where P = P_node (x) I_3 entry by entry, else None."""
    n, nc, rp = P["nrows"], P["ncols"], P["rowptr"].astype(np.int64)
    nnz = int(rp[-1])
    if n % 3 or nc % 3 or n == 0 or nnz % 3:
        return None
    lens = np.diff(rp).reshape(-1, 3)
    if np.any(lens != lens[:, :1]):
        return None
    rows = []
    for i in range(n // 3):
        k0, m = rp[3 * i], lens[i, 0]
        c, v = P["col"][k0:k0 + m].astype(np.int64), P["val"][k0:k0 + m]
        if np.any(c % 3):
            return None
        for q in (1, 2):
            kq = rp[3 * i + q]
            if not (np.array_equal(P["col"][kq:kq + m], c + q) and np.array_equal(P["val"][kq:kq + m], v)):
                return None
        rows.append((c // 3, v))
    Pn = csr(n // 3, nc // 3, rows)
    return Pn, transpose(Pn)


# ---- what pmh_mg_create builds ------------------------------------------------------------------------------------------------------------------
class Hierarchy:
    """The restated pmh_mg for H = {A: [CSR dict], P: [CSR dict], lambda_max, coarse_rowstart, coarse_pinv}; fused: PMH_MG_FUSED (None: unset); no_bsr:
    PMH_MG_NO_BSR is set."""

    def __init__(self, H, precision, degree=2, fused=None, no_bsr=False, lo=LO, hi=HI):
        self.H, self.precision, self.degree = H, precision, degree
        self.nlevels = nl = len(H["A"])
        self.fl = precision != 0
        self.T = T = np.float32 if self.fl else np.float64
        self.fused = degree == 2 and (fused is None or bool(fused))
        crs = np.asarray(H["coarse_rowstart"], np.int64)
        self.crs, self.nb = crs, len(crs) - 1
        self.L = []
        for l in range(nl):
            A = H["A"][l]
            Lv = dict(n=A["nrows"], S=None, A=A, transfer=NONE_T)
            if l + 1 < nl:
                storage = F64 if not self.fl else (F16 if (precision == 2 and l < 2) else F32)
                if not no_bsr or self.fl:
                    Lv["S"] = BC.restate(A, storage, 1024 if l == 0 else 512, self.nb if (self.nb > 1 and A["nrows"] % self.nb == 0) else 1)
                if self.fl and Lv["S"] is None:
                    raise Unsupported("PMH_MG_FP32/FP16 needs 3x3-block operators on every smoothed level")
                P = H["P"][l]
                Pt = transpose(P)
                Lv["P"], Lv["Pt"] = P, Pt
                Lv["pv"], Lv["rv"] = P["val"].astype(T), Pt["val"].astype(T)
                Lv["pv_owned"] = self.fl and int(P["rowptr"][-1]) > 0
                Lv["dinv"] = dinv_of(A, T)
                nod = nodal_transfer(P)
                if nod is not None:
                    Lv["Pn"], Lv["Rn"] = nod
                    Lv["transfer"] = NODAL
                else:
                    Lv["transfer"] = LONG if (P["nrows"] > 0 and float(P["rowptr"][-1]) / P["nrows"] > 12.0) else SHORT
                Lv["theta"], Lv["delta"], Lv["c1"], Lv["c2"] = cheb_constants(float(H["lambda_max"][l]), degree, lo, hi)
            self.L.append(Lv)
        m = np.diff(crs)
        self.coarse_m16 = int(np.all((m % 16 == 0) & (m >= 512)))
        self.cp_half = int(precision == 2 and nl > 1)
        self.cp_scale = 1.0
        pinv = np.asarray(H["coarse_pinv"], np.float64)
        if self.cp_half:
            self.cp_scale = BC.fp16_scale(float(np.abs(pinv).max()) if pinv.size else 0.0)
            self.pinv = (pinv / self.cp_scale).astype(np.float32).astype(np.float16)
        else:
            self.pinv = pinv.astype(T)
        self.cofs = np.concatenate([[0], np.cumsum(m * m)])

    def fused_level(self, l):
        return l < self.nlevels - 1 and self.fused and self.L[l]["S"] is not None

    def info(self, l):
        """pmh_mg_test_info's ten numbers."""
        Lv = self.L[l]
        S = Lv["S"]
        return [Lv["n"], int(S is not None), S["storage"] if S is not None else -1, Lv["transfer"], int(self.fused_level(l)), int(self.fl), self.cp_half, self.coarse_m16,
                self.nb, S["nrep"] if S is not None else 1]

    def pinv_block(self, k):
        m = int(self.crs[k + 1] - self.crs[k])
        return self.pinv[self.cofs[k]:self.cofs[k] + m * m].reshape(m, m)

    def stored(self):
        """The operators AS STORED, in float64 (dense level operators would be large: scalar CSR triplets instead): per smoothed level (rowptr, col, val) of A, the
        values of P in the cycle's precision, dinv; the coarse blocks pinv x scale."""
        out = []
        for Lv in self.L[:-1]:
            S = Lv["S"]
            if S is None:
                A = Lv["A"]
                trip = (np.repeat(np.arange(A["nrows"]), np.diff(A["rowptr"])), A["col"].astype(np.int64), A["val"].astype(np.float64))
            else:
                nr, nbk = S["rep_rows"], len(S["bcol"])
                brow = np.repeat(np.arange(S["nbr"]), np.diff(S["browptr"]))
                a = S["stored"].astype(np.float64) * (S["scale"] if S["storage"] == F16 else 1.0)
                r1 = (3 * brow[:, None, None] + np.arange(3)[None, :, None] + np.zeros((1, 1, 3), np.int64)).reshape(-1)
                c1 = (3 * S["bcol"].astype(np.int64)[:, None, None] + np.arange(3)[None, None, :] + np.zeros((1, 3, 1), np.int64)).reshape(-1)
                v1 = a.reshape(-1)
                assert nbk * 9 == v1.size
                trip = (np.concatenate([r1 + q * nr for q in range(S["nrep"])]), np.concatenate([c1 + q * nr for q in range(S["nrep"])]), np.tile(v1, S["nrep"]))
            out.append(dict(A=trip, pv=Lv["pv"].astype(np.float64), dinv=Lv["dinv"].astype(np.float64)))
        blocks = [self.pinv_block(k).astype(np.float64) * (self.cp_scale if self.cp_half else 1.0) for k in range(self.nb)]
        return out, blocks

    # ---- the kernels, one column ----
    def spmv(self, l, x):
        Lv = self.L[l]
        if Lv["S"] is not None:
            return BC.product(Lv["S"], x)
        A = Lv["A"]  # the CSR kernel's own order is not restated: only for data on which every order gives the same bits
        y = np.zeros(Lv["n"], self.T)
        np.add.at(y, np.repeat(np.arange(A["nrows"]), np.diff(A["rowptr"])), A["val"].astype(self.T) * x[A["col"]])
        return y

    def restrict(self, l, t, with_d0):
        """(b_c, d_c or None): k_mg_restrict3 / k_mg_restrict / k_mg_restrict_w."""
        Lv, Lc, T = self.L[l], self.L[l + 1], self.T
        if Lv["transfer"] == NODAL:
            Rn = Lv["Rn"]
            w = Rn["val"].astype(T)
            terms = w[:, None] * t.reshape(-1, 3)[Rn["col"]]
            s = tree_halving(lane_sums(Rn["rowptr"], terms, 8)).reshape(-1)
        else:
            Pt = Lv["Pt"]
            terms = Lv["rv"] * t[Pt["col"]]
            s = tree_halving(lane_sums(Pt["rowptr"], terms, 64 if Lv["transfer"] == LONG else 8))
        if not with_d0:
            return s, None
        return s, (Lc["dinv"] * s) * T(1.0 / Lc["theta"])

    def prolong_sub(self, l, x, xc):
        """x - P x_c: k_mg_prolong_sub3 / k_mg_prolong_sub (serial row walks) / k_mg_prolong_sub8 (8 lanes)."""
        Lv, T = self.L[l], self.T
        if Lv["transfer"] == NODAL:
            Pn = Lv["Pn"]
            terms = Pn["val"].astype(T)[:, None] * xc.reshape(-1, 3)[Pn["col"]]
            return x - lane_sums(Pn["rowptr"], terms, 1)[:, 0].reshape(-1)
        P = Lv["P"]
        terms = Lv["pv"] * xc[P["col"]]
        if Lv["transfer"] == LONG:
            return x - tree_halving(lane_sums(P["rowptr"], terms, 8))
        return x - lane_sums(P["rowptr"], terms, 1)[:, 0]

    def coarse(self, b):
        """k_mg_coarse: per lane four streams of 256 while j + 192 < m, the stride-64 tail into s0, (s0 + s1) + (s2 + s3), the down-tree, x scale for fp16 entries."""
        T, out = self.T, []
        lane = np.arange(64)
        for k in range(self.nb):
            r0, m = int(self.crs[k]), int(self.crs[k + 1] - self.crs[k])
            prod = self.pinv_block(k).astype(T) * b[None, r0:r0 + m]  # (m rows, m)
            s = np.zeros((4, m, 64), T)
            j = lane.copy()
            while True:
                go = j + 192 < m
                if not go.any():
                    break
                for q in range(4):
                    s[q][:, go] = s[q][:, go] + prod[:, j[go] + 64 * q]
                j = np.where(go, j + 256, j)
            while True:
                go = j < m
                if not go.any():
                    break
                s[0][:, go] = s[0][:, go] + prod[:, j[go]]
                j = np.where(go, j + 64, j)
            v = tree_halving((s[0] + s[1]) + (s[2] + s[3]))
            out.append(v * T(self.cp_scale) if self.cp_half else v)
        return np.concatenate(out) if out else np.zeros(0, T)

    def smooth(self, l, b, x, v):
        """mg_smooth: k_cheb_first_zero (x is None) or k_cheb_first, then degree - 1 times k_cheb_step."""
        Lv, T = self.L[l], self.T
        dinv, itheta = Lv["dinv"], T(1.0 / Lv["theta"])
        if x is None:
            r = dinv * b
            d = r * itheta
            x = d
        else:
            v["t"] = t = self.spmv(l, x)
            r = dinv * (b - t)
            d = r * itheta
            x = x + d
        for j in range(1, self.degree):
            v["t"] = t = self.spmv(l, d)
            r = r - dinv * t
            d = T(Lv["c1"][j]) * d + T(Lv["c2"][j]) * r
            x = x + d
        v["r"], v["d"] = r, d
        return x

    def cycle(self, l, b, b64=None, d0=None):
        """mg_cycle; records what every work vector holds when the cycle returns in self.vec[l]."""
        T, v = self.T, self.vec[l]
        if l == self.nlevels - 1:
            return self.coarse(b)
        Lv = self.L[l]
        if self.fused_level(l):
            dinv, itheta, c1, c2 = Lv["dinv"], T(1.0 / Lv["theta"]), T(Lv["c1"][1]), T(Lv["c2"][1])
            if d0 is None:
                if b64 is not None:
                    b = b64.astype(T)  # k_cheb_d0<TV, double>: the cycle-precision copy of b on the way
                    v["b"] = b
                d0 = dinv * b * itheta
            S = Lv["S"]
            xa = BC.epilogue(BC.PRE, BC.product(S, d0), T, d0, None, b, dinv, None, T(1) + c1, c1, c2)["y"]
            v["t"] = t = BC.epilogue(BC.SUB, BC.product(S, xa), T, xa, None, b, dinv, None)["y"]
            cf = self.fused_level(l + 1)
            bc, dc = self.restrict(l, t, cf)
            self.vec[l + 1]["b"] = bc
            self.vec[l + 1]["x"] = xc = self.cycle(l + 1, bc, d0=dc)
            v["xa"] = xa = self.prolong_sub(l, xa, xc)
            o = BC.epilogue(BC.POST1, BC.product(S, xa), T, xa, None, b, dinv, None, itheta, c1, c2)
            v["r"], v["d"] = o["r"], o["d"]
            return BC.epilogue(BC.POST2, BC.product(S, o["d"]), T, o["d"], o["y"], b, dinv, o["r"], itheta, c1, c2)["y"]
        x = self.smooth(l, b, None, v)
        v["t"] = t = self.spmv(l, x) - b
        bc, _ = self.restrict(l, t, False)
        self.vec[l + 1]["b"] = bc
        self.vec[l + 1]["x"] = xc = self.cycle(l + 1, bc)
        x = self.prolong_sub(l, x, xc)
        return self.smooth(l, b, x, v)

    def apply(self, b64):
        """pmh_mg_apply on one fp64 column: the fp64 result; self.vec[l][name]: the level's work vectors afterwards (the names pmh_mg_test_vector can read)."""
        b64 = np.asarray(b64, np.float64)
        self.vec = [dict() for _ in range(self.nlevels)]
        if self.fl and self.fused and self.nlevels > 1:
            x = self.cycle(0, None, b64=b64)
            self.vec[0]["x"] = x
        elif self.fl:
            self.vec[0]["b"] = b = b64.astype(self.T)  # k_mg_convert both ways
            self.vec[0]["x"] = x = self.cycle(0, b)
        else:
            x = self.cycle(0, b64)
        for l, Lv in enumerate(self.L[:-1]):
            self.vec[l]["dinv"] = Lv["dinv"]
        return x.astype(np.float64)


# ---- what pmh_mg_mv_create builds on top, and mvg_cycle -----------------------------------------------------------------------------------------
class Hierarchy8:
    """The restated pmh_mg_mv on a Hierarchy (of the first of nrep congruent blocks)."""

    def __init__(self, hy, nrep=1):
        self.hy, self.nrep = hy, nrep
        nl = hy.nlevels
        if nrep > 1:
            if any(hy.L[l]["S"] is None or hy.L[l]["S"]["nrep"] != nrep for l in range(nl - 1)):
                raise Unsupported("the blocks are not congruent on every level of the hierarchy")
            if hy.nb != nrep or hy.L[-1]["n"] % nrep:
                raise Unsupported("the coarse level does not have one block per congruent block")
            m2 = (hy.L[-1]["n"] // nrep) ** 2
            if hy.fl and any(not np.array_equal(hy.pinv[q * m2:(q + 1) * m2].astype(np.float32), hy.pinv[:m2].astype(np.float32)) for q in range(1, nrep)):
                raise Unsupported("the coarse pseudo-inverses of the congruent blocks differ")
        if not (hy.fl and hy.fused and nl > 1 and hy.degree == 2):
            raise Unsupported("the V-cycle runs in fp64" if not hy.fl else "the smoother is not of degree 2" if hy.degree != 2 else "the hierarchy has one level" if nl < 2
                              else "the V-cycle is not the fused form (PMH_MG_FUSED=0 or a level without 3 x 3 blocks)")
        for Lv in hy.L[:-1]:
            if Lv["n"] % 3 or (Lv["transfer"] != NODAL and (nrep > 1 or not Lv["pv_owned"])):
                raise Unsupported("a prolongation that is not node-wise (P = P_node (x) I_3) on congruent blocks")
        self.L = []
        for l, Lv in enumerate(hy.L[:-1]):
            A = Lv["A"]
            E = MC.restate(dict(A, nrows=A["nrows"], ncols=A["ncols"]), Lv["S"]["storage"] if Lv["S"]["storage"] != F64 else F32, MC.SQUARE, nrep)
            if E is None:
                raise Unsupported("a level operator has rows with unsorted columns or more than 2048 blocks of 3 x 3 in a block row")
            Ml = dict(E=E, kind=MV_NODAL if Lv["transfer"] == NODAL else MV_SCALAR)
            if Lv["transfer"] != NODAL and Lv["P"]["ncols"] % 3 == 0:
                EP = MC.restate(Lv["P"], F32, MC.RECT_NEG)
                ER = MC.restate(Lv["Pt"], F32, MC.RECT) if EP is not None else None
                if ER is not None:
                    Ml.update(EP=EP, ER=ER, kind=MV_ELL)
            self.L.append(Ml)

    def coarse_kind(self):
        hy = self.hy
        return COARSE_MFMA if (hy.cp_half and hy.coarse_m16) else COARSE_F16 if hy.cp_half else COARSE_F32

    def info(self, l):
        """pmh_mg_mv_test_info's eight numbers."""
        hy, last = self.hy, l == self.hy.nlevels - 1
        return [hy.L[l]["n"] // self.nrep, self.nrep, MV_NONE if last else self.L[l]["kind"], self.coarse_kind() if last else -1, -1 if last else self.L[l]["E"]["storage"],
                int(not last and l + 2 < hy.nlevels), hy.nb // self.nrep, 0]

    def restrict(self, l, t, cf):
        hy, Ml, Lv, Lc = self.hy, self.L[l], self.hy.L[l], self.hy.L[l + 1]
        T = np.float32
        itc = T(1.0 / Lc["theta"]) if cf else None
        nc = Lc["n"] // self.nrep
        if Ml["kind"] == MV_ELL:
            o = MC.epilogue(MC.RESTRICT, MC.product(Ml["ER"], t), T, None, None, None, Lc["dinv"][:nc] if cf else np.zeros(nc, T), None, itc if cf else T(0))
            return o["y"], (o["d"] if cf else None)
        if Ml["kind"] == MV_NODAL:  # k_mvg_restrict: 4 entry groups, xor 8 then 16
            Rn = Lv["Rn"]
            rp = Rn["rowptr"][:nc // 3 + 1]
            nz = int(rp[-1])
            terms = Rn["val"][:nz].astype(T)[:, None, None] * t.reshape(-1, 3, R)[Rn["col"][:nz]]
            s = tree_adjacent(lane_sums(rp, terms, 4)).reshape(-1, R)
        else:  # k_mvg_restrict_s: 8 entry groups, xor 8, 16, 32
            Pt = Lv["Pt"]
            terms = Lv["rv"][:, None] * t[Pt["col"]]
            s = tree_adjacent(lane_sums(Pt["rowptr"], terms, 8))
        return s, ((Lc["dinv"][:nc, None] * s) * itc if cf else None)

    def prolong_sub(self, l, xa, xc):
        Ml, Lv, T = self.L[l], self.hy.L[l], np.float32
        if Ml["kind"] == MV_ELL:  # xa += (-P) x_c
            return MC.epilogue(MC.ADD, MC.product(Ml["EP"], xc), T, None, None, xa, np.zeros(xa.shape[0], T), None)["y"]
        if Ml["kind"] == MV_NODAL:
            Pn = Lv["Pn"]
            rp = Pn["rowptr"][:xa.shape[0] // 3 + 1]
            nz = int(rp[-1])
            terms = Pn["val"][:nz].astype(T)[:, None, None] * xc.reshape(-1, 3, R)[Pn["col"][:nz]]
            return xa - lane_sums(rp, terms, 1)[:, 0].reshape(-1, R)
        P = Lv["P"]
        return xa - lane_sums(P["rowptr"], Lv["pv"][:, None] * xc[P["col"]], 1)[:, 0]

    def coarse(self, b):
        """k_mvg_coarse: lanes stride the row by 64, the halving tree per column, x scale for fp16 entries.  (The matrix-core form is not restated: MFMA cases.)"""
        hy, T, out = self.hy, np.float32, []
        for k in range(hy.nb // self.nrep):
            r0, m = int(hy.crs[k]), int(hy.crs[k + 1] - hy.crs[k])
            a, bb = hy.pinv_block(k).astype(T), b[r0:r0 + m]
            lanes = np.zeros((m, 64, R), T)
            for j0 in range(0, m, 64):
                w = min(64, m - j0)
                lanes[:, :w] = lanes[:, :w] + a[:, j0:j0 + w, None] * bb[None, j0:j0 + w, :]
            v = tree_halving(lanes)
            out.append(v * T(hy.cp_scale) if hy.cp_half else v)
        return np.concatenate(out)

    def cycle(self, l, b, b64=None, d0=None, coarse_x=None):
        hy, T, v = self.hy, np.float32, self.vec[l]
        if l == hy.nlevels - 1:
            return self.coarse(b) if coarse_x is None else coarse_x
        Lv, Ml = hy.L[l], self.L[l]
        n = Lv["n"] // self.nrep
        dinv, itheta, c1, c2 = Lv["dinv"][:n], T(1.0 / Lv["theta"]), T(Lv["c1"][1]), T(Lv["c2"][1])
        if d0 is None:
            if b64 is not None:
                v["b"] = b = b64.astype(T)
            d0 = (dinv * itheta)[:, None] * b  # k_mvg_d0: (dinv itheta) first
        E = Ml["E"]
        xa = MC.epilogue(MC.PRE, MC.product(E, d0), T, d0, None, b, dinv, None, T(1) + c1, c1, c2)["y"]
        v["t"] = t = MC.epilogue(MC.SUB, MC.product(E, xa), T, xa, None, b, dinv, None)["y"]
        cf = l + 2 < hy.nlevels
        bc, dc = self.restrict(l, t, cf)
        self.vec[l + 1]["b"] = bc
        self.vec[l + 1]["x"] = xc = self.cycle(l + 1, bc, d0=dc, coarse_x=coarse_x)
        v["xa"] = xa = self.prolong_sub(l, xa, xc)
        o = MC.epilogue(MC.POST1, MC.product(E, xa), T, xa, None, b, dinv, None, itheta, c1, c2)
        v["r"], v["d"] = o["r"], o["d"]
        return MC.epilogue(MC.POST2, MC.product(E, o["d"]), T, o["d"], o["y"], b, dinv, o["r"], itheta, c1, c2)["y"]

    def apply(self, b64, coarse_x=None):
        """pmh_mg_mv_apply on (rows, 8) fp64: the fp32 result (z64 is its widening); self.vec as Hierarchy.apply.  coarse_x: take the coarse solve's result as given
        (the matrix-core kernel, whose inner order is not fixed by the source)."""
        self.vec = [dict() for _ in range(self.hy.nlevels)]
        self.vec[0]["x"] = x = self.cycle(0, None, b64=np.asarray(b64, np.float64), coarse_x=coarse_x)
        for l, Lv in enumerate(self.hy.L[:-1]):
            self.vec[l]["dinv"] = Lv["dinv"][:Lv["n"] // self.nrep]
        return x


# ---- synthetic hierarchies ----------------------------------------------------------------------------------------------------------------------
def block_operator(rng, nbr, maxlen=7, halfwidth=6, diag=(4.0, 8.0), zero=False):
    """Square CSR of FULL 3 x 3 blocks: every block row holds its diagonal block and up to maxlen - 1 others from a window; off-diagonal entries +-[0.25, 0.75),
    the scalar diagonal in diag (away from zero, so that dinv ~ 1/6); zero: the same structure with every value 0.0."""
    rows = []
    for br in range(nbr):
        lo, hi = max(0, br - halfwidth), min(nbr, br + halfwidth + 1)
        others = np.setdiff1d(np.arange(lo, hi), [br])
        k = int(rng.integers(0, min(maxlen, others.size + 1)))
        bc = np.sort(np.concatenate([[br], rng.permutation(others)[:k]]))
        c = (3 * bc[:, None] + np.arange(3)[None, :]).reshape(-1)
        for q in range(3):
            v = rng.uniform(0.25, 0.75, c.size) * rng.choice([-1.0, 1.0], c.size)
            v[c == 3 * br + q] = rng.uniform(*diag)
            rows.append((c, np.zeros(c.size) if zero else v))
    return csr(3 * nbr, 3 * nbr, rows)


def from_columns(rng, nrows, lens, weights=None):
    """nrows x len(lens) CSR whose COLUMN j has lens[j] entries (so row j of the transpose has that many) in distinct random rows; values: weights, or +-[0.25, 1)."""
    ncols = len(lens)
    cols_of_row = [[] for _ in range(nrows)]
    for j, L in enumerate(lens):
        for i in np.sort(rng.permutation(nrows)[:int(L)]):
            cols_of_row[i].append(j)
    rows = []
    for c in cols_of_row:
        v = rng.choice(weights, len(c)) if weights is not None else rng.uniform(0.25, 1.0, len(c)) * rng.choice([-1.0, 1.0], len(c))
        rows.append((np.asarray(c, np.int64), v))
    return csr(nrows, ncols, rows)


def eye(n):
    """The coarsest level's operator: the cycle never multiplies by it."""
    return csr(n, n, [((i,), (1.0,)) for i in range(n)])


def kron3(Pn):
    """P_node (x) I_3 as scalar CSR."""
    rows = []
    rp = Pn["rowptr"]
    for i in range(Pn["nrows"]):
        c, v = Pn["col"][rp[i]:rp[i + 1]].astype(np.int64), Pn["val"][rp[i]:rp[i + 1]]
        for q in range(3):
            rows.append((3 * c + q, v))
    return csr(3 * Pn["nrows"], 3 * Pn["ncols"], rows)


def _lens(rng, n, present, lo, hi):
    """n row lengths: every one of `present` first, the rest random in [lo, hi]."""
    assert n >= len(present)
    return np.concatenate([np.asarray(present, np.int64), rng.integers(lo, hi + 1, n - len(present))])


def _pinv(rng, sizes, amp=0.125):
    return np.concatenate([(rng.uniform(0.5, 1.5, m * m) * rng.choice([-1.0, 1.0], m * m) * amp) for m in sizes])


def _hier(A, P, sizes, pinv, lam=None):
    return dict(A=A, P=P, lambda_max=np.array(lam if lam is not None else [2.0, 1.5, 2.5][:len(P)]), coarse_rowstart=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32),
                coarse_pinv=pinv)


def nodal3(seed=11):
    """3 smoothed levels + coarsest, P = P_node (x) I_3 with random dyadic weights; node counts 300 > 90 > 30 > 11; restriction rows of 0, 1, 3, 8, 9 and 27 entries on
    every level; two coarse blocks of 21 and 12 rows."""
    rng = np.random.default_rng(seed)
    nodes = [300, 90, 30, 11]
    A = [block_operator(rng, nn) for nn in nodes[:-1]] + [eye(3 * nodes[-1])]
    P = [kron3(from_columns(rng, nodes[l], _lens(rng, nodes[l + 1], [0, 1, 3, 8, 9, 27], 1, 27), weights=[1.0, 0.5, 0.25, 0.125, -0.5])) for l in range(3)]
    return _hier(A, P, [21, 12], _pinv(rng, [21, 12]))


def scalar_short(seed=12):
    """Block operators, P not node-wise with <= 12 entries per row on average: rows of P' with 0, 1, 7, 8, 9 entries; 300 > 120 > 45 rows, one coarse block."""
    rng = np.random.default_rng(seed)
    n = [300, 120, 45]
    A = [block_operator(rng, n[0] // 3), block_operator(rng, n[1] // 3), eye(n[2])]
    P = [from_columns(rng, n[l], _lens(rng, n[l + 1], [0, 1, 7, 8, 9], 1, 12)) for l in range(2)]
    return _hier(A, P, [45], _pinv(rng, [45]))


def scalar_s(seed=13):
    """As scalar_short with a coarsest level of 50 rows (no multiple of 3): the 8-column form has no rectangular block copy of the last P and takes its scalar
    kernels.  600 > 360 > 50 rows; rows of the last P' with 0, 1, 8, 9, 63, 64, 65 and 300 entries."""
    rng = np.random.default_rng(seed)
    n = [600, 360, 50]
    A = [block_operator(rng, n[0] // 3), block_operator(rng, n[1] // 3), eye(n[2])]
    P = [from_columns(rng, n[0], _lens(rng, n[1], [0, 1, 7, 8, 9], 1, 12)), from_columns(rng, n[1], _lens(rng, n[2], [0, 1, 8, 9, 63, 64, 65, 300], 10, 30))]
    return _hier(A, P, [30, 20], _pinv(rng, [30, 20]))


def scalar_s_d0(seed=20):
    """6600 > 120 > 45 rows, P not node-wise; ONE row of the first P' has 2100 entries in as many block columns: more than the 2048 blocks a rectangular block copy
    takes per block row, so the 8-column form keeps NEITHER copy on the fine level and its scalar kernels run with the next level's d0 riding on the restriction."""
    rng = np.random.default_rng(seed)
    n = [6600, 120, 45]
    A = [block_operator(rng, n[0] // 3), block_operator(rng, n[1] // 3), eye(n[2])]
    lens = _lens(rng, n[1], [0, 1, 8, 9, 63, 64, 65], 1, 12)
    P0 = from_columns(rng, n[0], lens)
    rows, rp = [], P0["rowptr"]
    for i in range(n[0]):  # column 7 (65 entries so far) gains one entry in the first scalar row of 2100 fine nodes
        c, v = P0["col"][rp[i]:rp[i + 1]].astype(np.int64), P0["val"][rp[i]:rp[i + 1]]
        if i % 3 == 0 and i < 3 * 2100 and 7 not in c:
            k = int(np.searchsorted(c, 7))
            c, v = np.insert(c, k, 7), np.insert(v, k, 0.03125 * (1 + i % 5) * (-1) ** i)
        rows.append((c, v))
    P = [csr(n[0], n[1], rows), from_columns(rng, n[1], _lens(rng, n[2], [0, 1, 7, 8, 9], 1, 12))]
    return _hier(A, P, [45], _pinv(rng, [45]))


def long_rows(seed=14):
    """Two levels, P with 14.2 entries per row on average (> 12: the wavefront-per-row restriction, 8 lanes per row in the prolongation): 1500 fine rows, 8448 coarse rows
    (a second grid-stride trip of the restriction's 2048 workgroups of 4 rows) in 1056 coarse blocks of 8; rows of P' with 0, 1, 63, 64, 65, 200 entries."""
    rng = np.random.default_rng(seed)
    n, nc = 1500, 8448
    lens = _lens(rng, nc, [0, 1, 63, 64, 65, 200], 1, 4)
    lens[-3:] = [65, 0, 64]  # the rows of the second trip end on the special lengths too
    A = [block_operator(rng, n // 3), eye(nc)]
    P = [from_columns(rng, n, lens)]
    assert int(P[0]["rowptr"][-1]) > 12 * n
    return _hier(A, P, [8] * (nc // 8), _pinv(rng, [8] * (nc // 8)))


def long_rows_d0(seed=22):
    """Three levels, 1500 > 360 > 45 rows, one coarse block: the first P has 13 entries per row on average (> 12: the wavefront-per-row restriction, 8 lanes per row in
    the prolongation) and level 1 is a smoothed one, so its d0 rides on THAT restriction; rows of the first P' with 0, 1, 63, 64, 65, 200 entries.  The second P is short."""
    rng = np.random.default_rng(seed)
    n = [1500, 360, 45]
    A = [block_operator(rng, n[0] // 3), block_operator(rng, n[1] // 3), eye(n[2])]
    P = [from_columns(rng, n[0], _lens(rng, n[1], [0, 1, 63, 64, 65, 200], 40, 70)), from_columns(rng, n[1], _lens(rng, n[2], [0, 1, 7, 8, 9], 1, 12))]
    assert int(P[0]["rowptr"][-1]) > 12 * n[0] and int(P[1]["rowptr"][-1]) <= 12 * n[1]
    return _hier(A, P, [45], _pinv(rng, [45]))


COARSE_STREAM_BLOCKS = [193, 256, 257, 449, 520, 2]  # around the four-stream threshold j + 192 < m and its tail; 1677 rows = 3 x 559


def coarse_streams(seed=15):
    """Two levels, coarse blocks of 193, 256, 257, 449, 520 and 2 rows; 600 fine rows, a short scalar P."""
    rng = np.random.default_rng(seed)
    n, nc = 600, sum(COARSE_STREAM_BLOCKS)
    A = [block_operator(rng, n // 3), eye(nc)]
    P = [from_columns(rng, n, _lens(rng, nc, [0, 1, 8], 1, 4))]
    return _hier(A, P, COARSE_STREAM_BLOCKS, _pinv(rng, COARSE_STREAM_BLOCKS, amp=2.0 ** -5))


def one_level(seed=16):
    """nlevels == 1: the coarse solve alone, blocks of 70 and 30 rows."""
    rng = np.random.default_rng(seed)
    return _hier([eye(100)], [], [70, 30], _pinv(rng, [70, 30]), lam=[])


def diag_rules(seed=17):
    """Two levels; the fine operator (scalar CSR, for the CSR kernel) has row 5 without a stored diagonal, row 9 with a stored 0.0 and row 14 with the diagonal stored
    twice (4.0 then -8.0: the last one counts)."""
    rng = np.random.default_rng(seed)
    n, nc = 48, 12
    rows = []
    for i in range(n):
        c = np.unique(np.concatenate([[i], rng.integers(0, n, 3)]))
        v = rng.uniform(0.25, 0.75, c.size)
        v[c == i] = rng.uniform(2.0, 4.0)
        if i == 5:
            keep = c != i
            c, v = c[keep], v[keep]
        if i == 9:
            v[c == i] = 0.0
        if i == 14:
            k = int(np.flatnonzero(c == i)[0])
            c, v = np.insert(c, k, i), np.insert(v, k, 4.0)
            v[k + 1] = -8.0
        rows.append((c, v))
    A = [csr(n, n, rows), eye(nc)]
    P = [from_columns(rng, n, _lens(rng, nc, [0, 1], 2, 6))]
    return _hier(A, P, [nc], _pinv(rng, [nc]))


CSR_DYADIC_WINDOW = (0.25, 0.75)  # x lambda_max = 2: theta = 1, a power of two


def csr_dyadic(seed=21):
    """Scalar CSR operators (1 dof per node; PMH_MG_NO_BSR) for the degree-1 cycle on dyadic data: entries of A multiples of 1/4 in [-2, 2] with diagonals 2 or 4, P
    entries +-{1, 1/2, 1/4}, pinv multiples of 1/8 in [-1, 1], lambda_max = 2 under the window CSR_DYADIC_WINDOW (theta = 1).  With an integer b in [-16, 16] every
    intermediate is a multiple of 2^-15 (2^-26 on three levels) far below 2^53 of them: every sum is exact in fp64 in any order."""
    rng = np.random.default_rng(seed)
    n = [200, 61, 17]

    def op(m):
        rows = []
        for i in range(m):
            c = np.unique(np.concatenate([[i], rng.integers(max(0, i - 9), min(m, i + 10), 5)]))
            v = rng.integers(-8, 9, c.size) / 4.0
            v[c == i] = rng.choice([2.0, 4.0])
            rows.append((c, v))
        return csr(m, m, rows)
    A = [op(n[0]), op(n[1]), eye(n[2])]
    P = [from_columns(rng, n[l], _lens(rng, n[l + 1], [0, 1, 8, 9], 1, 6), weights=[1.0, -1.0, 0.5, -0.5, 0.25]) for l in range(2)]
    pinv = rng.integers(-8, 9, n[2] * n[2]) / 8.0
    return _hier(A, P, [n[2]], pinv, lam=[2.0, 2.0])


def exact_cycle_degree1(H, b):
    """The degree-1 cycle on a csr_dyadic hierarchy in EXACT integer arithmetic (int64 numerators over a power-of-two denominator that every stage widens by the
    fraction bits of its operator: A 2, dinv 2, P 2, pinv 3), for theta = 1.  Returns float64 (the division by the power of two is exact)."""
    nl = len(H["A"])
    crs = np.asarray(H["coarse_rowstart"], np.int64)

    def ints(v, f):
        q = np.asarray(v, np.float64) * 2.0 ** f
        assert np.array_equal(q, np.round(q)) and np.abs(q).max() < 2.0 ** 40
        return q.astype(np.int64)

    def mult(M, x, f):  # (x, fx) -> (M x, fx + f)
        y = np.zeros(M["nrows"], np.int64)
        np.add.at(y, np.repeat(np.arange(M["nrows"]), np.diff(M["rowptr"])), ints(M["val"], f) * x[0][M["col"]])
        return y, x[1] + f

    def to(x, f):
        assert f >= x[1]
        return x[0] << (f - x[1])

    def V(l, b):
        if l == nl - 1:
            pinv = ints(H["coarse_pinv"], 3)
            o, out = 0, []
            for k in range(len(crs) - 1):
                m = int(crs[k + 1] - crs[k])
                out.append(pinv[o:o + m * m].reshape(m, m) @ b[0][crs[k]:crs[k + 1]])
                o += m * m
            return np.concatenate(out), b[1] + 3
        A, P = H["A"][l], H["P"][l]
        dinv = ints(dinv_of(A, np.float64), 2)
        x = (dinv * b[0], b[1] + 2)  # r = D^-1 b, d = r / theta = r, x = d
        t = mult(A, x, 2)
        t = (t[0] - to(b, t[1]), t[1])
        xc = V(l + 1, mult(transpose(P), t, 2))
        pc = mult(P, xc, 2)
        x = (to(x, pc[1]) - pc[0], pc[1])
        t = mult(A, x, 2)
        r = (dinv * (to(b, t[1]) - t[0]), t[1] + 2)
        return to(x, r[1]) + r[0], r[1]

    f0 = next(f for f in range(12) if np.array_equal(np.asarray(b) * 2.0 ** f, np.round(np.asarray(b) * 2.0 ** f)))  # b: integers times a power of two
    x, f = V(0, (ints(b, f0), f0))
    assert np.abs(x).max() < 2 ** 52
    return x.astype(np.float64) * 2.0 ** -f


def mfma(blocks, dyadic, seed=18):
    """Two levels for the matrix-core coarse solve: the fine operator has a full block structure whose VALUES are all 0.0 (dinv = 1 by the missing-diagonal rule) and
    P = I, so that t = A xa - b = -b exactly and the coarse right-hand side is -float(b) whatever the smoothing constants are.  dyadic: pseudo-inverse entries are
    integers in [-8, 8] (max |.| = 8: the fp16 copy k / 8 is exact)."""
    rng = np.random.default_rng(seed + sum(blocks))
    n = sum(blocks)
    A = [block_operator(rng, n // 3, maxlen=3, zero=True), eye(n)]
    P = [eye(n)]
    if dyadic:
        pinv = np.concatenate([rng.integers(-8, 9, m * m).astype(np.float64) for m in blocks])
        pinv[0] = 8.0
    else:
        pinv = _pinv(rng, blocks, amp=2.0 ** -4)
    return _hier(A, P, blocks, pinv, lam=[2.0])


MFMA_BLOCKS = {"m528": [528], "m1008_528": [1008, 528], "m1584": [1584]}


def replicate(H, nrep):
    """nrep congruent copies of the hierarchy H on the diagonal of every level (H has ONE coarse block)."""
    def rep(M):
        nnz = int(M["rowptr"][-1])
        rowptr = np.concatenate([[0]] + [M["rowptr"][1:].astype(np.int64) + q * nnz for q in range(nrep)])
        col = np.concatenate([M["col"][:nnz].astype(np.int64) + q * M["ncols"] for q in range(nrep)])
        return dict(nrows=M["nrows"] * nrep, ncols=M["ncols"] * nrep, n=M["nrows"] * nrep, rowptr=rowptr.astype(np.int32), col=col.astype(np.int32), val=np.tile(M["val"][:nnz], nrep))
    m = int(H["coarse_rowstart"][-1])
    return dict(A=[rep(a) for a in H["A"]], P=[rep(p) for p in H["P"]], lambda_max=H["lambda_max"], coarse_rowstart=(m * np.arange(nrep + 1)).astype(np.int32),
                coarse_pinv=np.tile(H["coarse_pinv"], nrep))


def congruent_base(seed=19):
    """The block every congruent case repeats: node-wise P, 60 > 18 > 6 nodes, one coarse block of 18 rows."""
    rng = np.random.default_rng(seed)
    nodes = [60, 18, 6]
    A = [block_operator(rng, nodes[0]), block_operator(rng, nodes[1]), eye(18)]
    P = [kron3(from_columns(rng, nodes[l], _lens(rng, nodes[l + 1], [0, 1, 3, 8, 9], 1, 12), weights=[1.0, 0.5, 0.25, 0.125])) for l in range(2)]
    return _hier(A, P, [18], _pinv(rng, [18]))


BUILDERS = dict(nodal3=nodal3, scalar_short=scalar_short, scalar_s=scalar_s, scalar_s_d0=scalar_s_d0, csr_dyadic=csr_dyadic, long_rows=long_rows, long_rows_d0=long_rows_d0, coarse_streams=coarse_streams, one_level=one_level,
                diag_rules=diag_rules, congruent1=congruent_base, congruent2=lambda: replicate(congruent_base(), 2), congruent8=lambda: replicate(congruent_base(), 8))
for _k, _b in MFMA_BLOCKS.items():
    BUILDERS[_k] = functools.partial(mfma, _b, False)
    BUILDERS[_k + "_dyadic"] = functools.partial(mfma, _b, True)
BUILDERS["m520"] = functools.partial(mfma, [520, 8], False)  # 520 = 8 mod 16: the wavefront-per-row kernel


@functools.lru_cache(maxsize=None)
def hierarchy(name):
    """The case's H.  Built once; nobody writes into it."""
    return BUILDERS[name]()


# (case, precision, degree, PMH_MG_FUSED or None, PMH_MG_NO_BSR): what the exact tests run; the 8-column form joins wherever Hierarchy8 accepts the hierarchy
RUNS = [(c, p, 2, None, False) for c in ("nodal3", "scalar_short", "scalar_s", "long_rows", "coarse_streams") for p in ("fp64", "fp32", "fp16")]
RUNS += [("long_rows_d0", p, 2, None, False) for p in ("fp64", "fp32", "fp16")]  # the long-row restriction with the coarse level's d0 riding on it
RUNS += [("one_level", p, 2, None, False) for p in ("fp64", "fp32", "fp16")]
RUNS += [("nodal3", p, 2, 0, False) for p in ("fp64", "fp32")]  # unfused
RUNS += [("nodal3", p, d, None, False) for d in (1, 3) for p in ("fp64", "fp32")]
RUNS += [("scalar_short", "fp32", 3, None, False), ("long_rows", "fp32", 1, None, False)]  # the scalar transfers in float on the unfused cycle
RUNS += [("m520", "fp16", 2, None, False), ("scalar_s_d0", "fp32", 2, None, False), ("scalar_s_d0", "fp16", 2, None, False)]
RUNS += [("congruent1", "fp32", 2, None, False), ("congruent2", "fp32", 2, None, False), ("congruent8", "fp16", 2, None, False)]


def run_id(run):
    c, p, d, f, nb = run
    return "%s-%s-deg%d%s%s" % (c, p, d, "" if f is None else "-fused%d" % f, "-csr" if nb else "")


@functools.lru_cache(maxsize=None)
def restated(run):
    c, p, d, f, nb = run
    return Hierarchy(hierarchy(c), PRECISIONS[p], d, f, nb)


def rhs(name, n):
    """(n, 8) fp64 right-hand sides in the manner of mv_cases.columns: column r carries 2^COLUMN_EXP[r], one column zero, one of a single sign, random signs (hence
    cancellation) elsewhere; NOT rounded to fp32, so that the fp64 -> fp32 copy of b rounds."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    return MC.columns(rng, n, np.float64)


def rhs_dyadic(name, n):
    """Integers in [-16, 16] times the column's power of two."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    b = rng.integers(-16, 17, (n, R)).astype(np.float64) * np.ldexp(1.0, np.array(MC.COLUMN_EXP))[None, :]
    b[:, MC.ZERO_COLUMN] = 0.0
    b[:, MC.ONE_SIGN_COLUMN] = np.abs(b[:, MC.ONE_SIGN_COLUMN])
    return b


@functools.lru_cache(maxsize=None)
def reference(run):
    """(Hierarchy, b (n, 8), {column: (fp64 result, vec)} for the one-column cycle on columns 0 and 4, Hierarchy8 or the refusal text, its (result, vec) or None)."""
    hy = restated(run)
    nrep = {"congruent2": 2, "congruent8": 8}.get(run[0], 1)
    b = rhs(run_id(run), hy.L[0]["n"])
    one = {}
    for r in (0, 4):
        z = hy.apply(b[:, r])
        one[r] = (z, hy.vec)
    try:
        h8 = Hierarchy8(hy, nrep)
    except Unsupported as e:
        return hy, b, one, str(e), None
    n1 = hy.L[0]["n"] // nrep
    x = h8.apply(b[:n1])
    return hy, b, one, h8, (x, h8.vec)
