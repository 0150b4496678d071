"""CPU checks of tests/mg_cases.py, the numpy restatement tests/test_gpu_mg_paths.py compares the device with bit for bit: the restated V-cycle against
oracle.mg_host.vcycle in float64 on the operators AS STORED (dequantised fp32 / fp16 entries, stored dinv, stored pinv x scale: only the rounding of the
arithmetic separates the two), the fp64 restatement against a long-double evaluation, the plan each case must reach (the numbers pmh_mg_test_info /
pmh_mg_mv_test_info report), and the row lengths each case is named after.  No GPU."""
import numpy as np
import pytest

import mg_cases as G

# worst max-norm relative error (max |x - ref| / max |ref| per column) over all runs and columns, MEASURED here on the CPU (numpy 2, x86-64 with an 80-bit long double;
# the restatement uses no BLAS, so it is deterministic) and asserted at twice that -- the margin only covers another numpy build:
#   restatement in float64 arithmetic vs oracle.mg_host.vcycle in float64             fp64 cycle: 2.02e-15  (scalar_s)
#   restatement in float32 arithmetic vs the same on the operators as stored          fp32 cycle: 1.16e-06  (scalar_s_d0, 8 columns)   fp16 cycle: 8.85e-07  (scalar_s)
#   fp64 restatement vs the long-double evaluation on the same operators              1.56e-15  (scalar_s)
# (one column and 8 columns pooled; the per-run figures are printed under -s and listed in docs/LAB_NOTEBOOK.md)
MEASURED = {"fp64": 2.02e-15, "fp32": 1.16e-06, "fp16": 8.85e-07, "fp64 vs long double": 1.56e-15}

class _Op:
    """A level operator for oracle.mg_host.vcycle: the stored matrix, and a diagonal whose reciprocal is the STORED dinv."""

    def __init__(self, M, dinv):
        self.M, self.d = M, 1.0 / dinv

    def diagonal(self):
        return self.d

    def __matmul__(self, x):
        return self.M @ x


def _oracle(hy):
    import scipy.sparse as sp

    from oracle.mg_host import vcycle

    ops, blocks = hy.stored()
    A, P = [], []
    for l, o in enumerate(ops):
        n = hy.L[l]["n"]
        r, c, v = o["A"]
        A.append(_Op(sp.csr_matrix((v, (r, c)), shape=(n, n)), o["dinv"]))
        Pl = hy.L[l]["P"]
        P.append(sp.csr_matrix((o["pv"], Pl["col"], Pl["rowptr"]), shape=(Pl["nrows"], Pl["ncols"])))
    A.append(_Op(None, np.ones(hy.L[-1]["n"])))
    H = dict(A=A, P=P, lambda_max=hy.H["lambda_max"], coarse_rowstart=hy.crs, coarse_pinv=np.concatenate([b.reshape(-1) for b in blocks]))
    return vcycle(H, hy.degree, G.LO, G.HI)


def _long_double(hy, b):
    """The cycle of oracle.mg_host.vcycle written out once more in long double on the stored operators (scipy has no long-double product)."""
    LD = np.longdouble
    ops, blocks = hy.stored()
    nl = hy.nlevels

    def mult(trip, n, x):
        y = np.zeros(n, LD)
        np.add.at(y, trip[0], trip[2].astype(LD) * x[trip[1]])
        return y

    def Ptrip(l):
        P = hy.L[l]["P"]
        return np.repeat(np.arange(P["nrows"]), np.diff(P["rowptr"])), P["col"].astype(np.int64), ops[l]["pv"]

    def smooth(l, b, x):
        Lv, dinv, n = hy.L[l], ops[l]["dinv"].astype(LD), hy.L[l]["n"]
        th, de = LD(Lv["theta"]), LD(Lv["delta"])
        sig = th / de
        rho = 1 / sig
        if x is None:
            r = dinv * b
            d = r / th
            x = d.copy()
        else:
            r = dinv * (b - mult(ops[l]["A"], n, x))
            d = r / th
            x = x + d
        for _ in range(1, hy.degree):
            rn = 1 / (2 * sig - rho)
            r = r - dinv * mult(ops[l]["A"], n, d)
            d = rn * rho * d + 2 * rn / de * r
            x = x + d
            rho = rn
        return x

    def V(l, b):
        if l == nl - 1:
            return np.concatenate([blocks[k].astype(LD) @ b[hy.crs[k]:hy.crs[k + 1]] for k in range(hy.nb)])
        n, (pr, pc, pv) = hy.L[l]["n"], Ptrip(l)
        x = smooth(l, b, None)
        xc = V(l + 1, mult((pc, pr, pv), hy.L[l + 1]["n"], b - mult(ops[l]["A"], n, x)))
        return smooth(l, b, x + mult((pr, pc, pv), n, xc))

    return V(0, np.asarray(b, LD))


def _relerr(x, ref):
    scale = float(np.abs(ref).max())
    if scale == 0.0:
        assert not np.any(x)  # the zero column stays exactly zero
        return 0.0
    return float(np.abs(np.asarray(x, np.longdouble) - ref).max() / scale)


@pytest.mark.parametrize("run", G.RUNS, ids=G.run_id)
def test_restatement_against_high_precision(run):
    """One column: columns 0 and 4 of the run's right-hand sides; 8 columns: every column.  Measured worst errors (asserted at 2 x): fp64 2.02e-15, fp32 1.16e-06,
    fp16 storage 8.85e-07 against the float64 oracle; the fp64 restatement 1.56e-15 against long double."""
    hy, b, one, h8, r8 = G.reference(run)
    V = _oracle(hy)
    prec = run[1]
    worst = 0.0
    for r, (z, _) in one.items():
        worst = max(worst, _relerr(z, V(b[:, r])))
    if r8 is not None:
        n1 = r8[0].shape[0]
        for r in range(G.R):
            full = np.zeros(b.shape[0])
            full[:n1] = b[:n1, r]
            worst = max(worst, _relerr(r8[0][:, r], V(full)[:n1]))
    print("%-32s worst relative error vs float64 oracle %.2e" % (G.run_id(run), worst))
    assert worst <= 2 * MEASURED[prec], (worst, MEASURED[prec])
    if prec == "fp64":
        ld = max(_relerr(z, _long_double(hy, b[:, r])) for r, (z, _) in one.items())
        print("%-32s worst relative error vs long double    %.2e" % (G.run_id(run), ld))
        assert np.finfo(np.longdouble).nmant >= 63 and ld <= 2 * MEASURED["fp64 vs long double"], ld


def test_trees_are_the_shuffle_sequences():
    """tree_halving is lane 0 after shfl_down / descending shfl_xor steps; tree_adjacent is group 0 after ascending shfl_xor steps over the groups -- simulated
    lane by lane on float32 data whose sums round."""
    rng = np.random.default_rng(0)
    for width in (8, 64):
        s = (rng.standard_normal((50, width)) * 10.0 ** rng.uniform(-3, 3, (50, width))).astype(np.float32)
        idx = np.arange(width)
        down, xor = s.copy(), s.copy()
        o = width // 2
        while o:
            down = down + np.where(idx + o < width, down[:, np.minimum(idx + o, width - 1)], down)
            xor = xor + xor[:, idx ^ o]
            o //= 2
        assert np.array_equal(down[:, 0], G.tree_halving(s)) and np.array_equal(xor[:, 0], G.tree_halving(s))
    for groups in (4, 8):  # lanes = groups x 8 columns; xor 8, 16(, 32)
        s = (rng.standard_normal((50, groups * 8)) * 10.0 ** rng.uniform(-3, 3, (50, groups * 8))).astype(np.float32)
        idx = np.arange(groups * 8)
        v, o = s.copy(), 8
        while o < groups * 8:
            v = v + v[:, idx ^ o]
            o *= 2
        assert np.array_equal(v[:, :8], G.tree_adjacent(s.reshape(50, groups, 8)))
    lanes = G.lane_sums(np.array([0, 0, 1, 20]), np.arange(1.0, 21.0, dtype=np.float32), 8)
    assert lanes.shape == (3, 8) and not lanes[0].any() and lanes[1].tolist() == [1.0] + [0.0] * 7 and lanes[2, 0] == 2.0 + 10.0 + 18.0 and lanes[2, 3] == 5.0 + 13.0


# case -> (transfer kernels per level of the one-column cycle, of the 8-column cycle where it accepts the hierarchy)
TRANSFERS = {
    "nodal3": ([G.NODAL] * 3, [G.MV_NODAL] * 3), "scalar_short": ([G.SHORT] * 2, [G.MV_ELL] * 2), "scalar_s": ([G.SHORT] * 2, [G.MV_ELL, G.MV_SCALAR]),
    "scalar_s_d0": ([G.SHORT] * 2, [G.MV_SCALAR, G.MV_ELL]), "long_rows": ([G.LONG], [G.MV_ELL]), "long_rows_d0": ([G.LONG, G.SHORT], [G.MV_ELL] * 2), "coarse_streams": ([G.SHORT], [G.MV_ELL]), "one_level": ([], []),
    "m520": ([G.NODAL], [G.MV_NODAL]), "congruent1": ([G.NODAL] * 2, [G.MV_NODAL] * 2), "congruent2": ([G.NODAL] * 2, [G.MV_NODAL] * 2), "congruent8": ([G.NODAL] * 2, [G.MV_NODAL] * 2),
}
REFUSAL = {"fp64": "runs in fp64", 1: "not of degree 2", 3: "not of degree 2", 0: "not the fused form", "one_level": "has one level"}


@pytest.mark.parametrize("run", G.RUNS, ids=G.run_id)
def test_plan_of_every_run(run):
    """The info vectors the GPU tests compare the library's with, spelled out from the rules of pmh_mg_create / pmh_mg_mv_create: a case that took another kernel
    than the one it is named after fails here."""
    name, prec, degree, fused, _ = run
    hy, b, one, h8, r8 = G.reference(run)
    H = G.hierarchy(name)
    nl, nb = len(H["A"]), len(H["coarse_rowstart"]) - 1
    t1, t8 = TRANSFERS[name]
    fl = prec != "fp64"
    is_fused = degree == 2 and fused != 0
    nrep = {"congruent2": 2, "congruent8": 8}.get(name, 1)
    for l in range(nl):
        last = l == nl - 1
        storage = -1 if last else 0 if not fl else 2 if (prec == "fp16" and l < 2) else 1
        exp = [H["A"][l]["nrows"], int(not last), storage, 0 if last else t1[l], int(is_fused and not last), int(fl), int(prec == "fp16" and nl > 1), 0, nb, 1 if last else nrep]
        assert hy.info(l) == exp, (l, hy.info(l), exp)
    if not fl or degree != 2 or fused == 0 or nl == 1:
        why = REFUSAL["fp64"] if not fl else REFUSAL[degree] if degree != 2 else REFUSAL["one_level"] if nl == 1 else REFUSAL[0]
        assert isinstance(h8, str) and why in h8, (h8, why)
        return
    for l in range(nl):
        last = l == nl - 1
        exp = [H["A"][l]["nrows"] // nrep, nrep, 0 if last else t8[l], (1 if prec == "fp16" else 0) if last else -1, -1 if last else (2 if (prec == "fp16" and l < 2) else 1),
               int(l + 2 < nl), nb // nrep, 0]
        assert h8.info(l) == exp, (l, h8.info(l), exp)


def _row_lengths(M):
    return set(np.diff(M["rowptr"]).tolist())


def test_cases_hold_the_shapes_they_are_named_after():
    hy = G.restated(("nodal3", "fp32", 2, None, False))
    for l in range(3):
        assert {0, 1, 3, 8, 9, 27} <= _row_lengths(hy.L[l]["Rn"]) and max(_row_lengths(hy.L[l]["Rn"])) <= 27
    assert np.diff(hy.crs).tolist() == [21, 12] and hy.fused_level(1) and hy.fused_level(2) and not hy.fused_level(3)  # d_c rides at l = 0, 1 and not at the last smoothed level
    hy = G.restated(("scalar_short", "fp32", 2, None, False))
    for l in range(2):
        assert {0, 1, 7, 8, 9} <= _row_lengths(hy.L[l]["Pt"]) and hy.L[l]["P"]["rowptr"][-1] <= 12 * hy.L[l]["n"]
    hy = G.restated(("scalar_s", "fp32", 2, None, False))
    assert {0, 1, 8, 9, 63, 64, 65, 300} <= _row_lengths(hy.L[1]["Pt"]) and hy.L[2]["n"] % 3 != 0
    hy = G.restated(("scalar_s_d0", "fp32", 2, None, False))
    assert max(_row_lengths(hy.L[0]["Pt"])) >= 2100 and {0, 1, 8, 9, 63, 64} <= _row_lengths(hy.L[0]["Pt"])
    hy = G.restated(("long_rows", "fp32", 2, None, False))
    lens = np.diff(hy.L[0]["Pt"]["rowptr"])
    assert {0, 1, 63, 64, 65, 200} <= set(lens.tolist()) and hy.L[1]["n"] > 8192 and {0, 64, 65} <= set(lens[8192:].tolist())
    assert hy.L[0]["P"]["rowptr"][-1] > 12 * hy.L[0]["n"] and max(_row_lengths(hy.L[0]["P"])) > 8  # the 8-lane prolongation takes a second step over a row
    hy = G.restated(("long_rows_d0", "fp32", 2, None, False))
    assert {0, 1, 63, 64, 65, 200} <= _row_lengths(hy.L[0]["Pt"]) and hy.L[0]["P"]["rowptr"][-1] > 12 * hy.L[0]["n"] and hy.L[1]["P"]["rowptr"][-1] <= 12 * hy.L[1]["n"]
    assert [hy.L[l]["n"] for l in range(3)] == [1500, 360, 45] and np.diff(hy.crs).tolist() == [45] and hy.fused_level(1)  # d_c rides on the long-row restriction
    hy = G.restated(("coarse_streams", "fp16", 2, None, False))
    m = np.diff(hy.crs)
    assert m.tolist() == [193, 256, 257, 449, 520, 2]
    # lanes with no, one and two four-stream trips, with and without a tail behind them: lane 0 alone takes one at 193 rows (0 + 192 < 193) and a second one at 449 (256 + 192 < 449)
    trips = lambda lane, mm: len(range(lane, mm - 192, 256)) if mm > 192 + lane else 0  # noqa: E731
    assert [trips(0, x) for x in m] == [1, 1, 1, 2, 2, 0] and [trips(1, x) for x in m] == [0, 1, 1, 1, 2, 0] and [trips(63, x) for x in m] == [0, 1, 1, 1, 2, 0]
    assert hy.cp_half == 1 and hy.cp_scale == 2.0 ** -5  # max |pinv| in [2^-5, 2^-4)
    for p in ("fp64", "fp32", "fp16"):
        hy = G.restated(("one_level", p, 2, None, False))
        assert hy.nlevels == 1 and hy.cp_half == 0
    for name, blocks in G.MFMA_BLOCKS.items():
        for suffix in ("", "_dyadic"):
            hy = G.Hierarchy(G.hierarchy(name + suffix), 2)
            h8 = G.Hierarchy8(hy)
            assert np.diff(hy.crs).tolist() == blocks and hy.coarse_m16 == 1 and h8.coarse_kind() == G.COARSE_MFMA and h8.info(1)[3] == 2
            assert np.all(hy.L[0]["dinv"] == 1.0)  # a stored 0.0 diagonal
    assert 528 % 32 == 16 and -(-528 // 32) == 17 and 1008 % 32 == 16 and -(-1584 // 32) == 50  # the last k-step half full; 17 steps on 16 wavefronts; 50 = 4 per wavefront, the last short
    hy = G.Hierarchy(G.hierarchy("m520"), 2)
    assert hy.coarse_m16 == 0 and G.Hierarchy8(hy).coarse_kind() == G.COARSE_F16 and np.diff(hy.crs).tolist() == [520, 8]


def test_dinv_rules_and_dyadic_cycle():
    hy = G.Hierarchy(G.hierarchy("diag_rules"), 0, 2, None, True)
    A = G.hierarchy("diag_rules")["A"][0]
    row = lambda i: A["col"][A["rowptr"][i]:A["rowptr"][i + 1]].tolist()  # noqa: E731
    assert 5 not in row(5) and row(14).count(14) == 2 and hy.info(0)[1] == 0
    d = hy.L[0]["dinv"]
    assert d[5] == 1.0 and d[9] == 1.0 and d[14] == -0.125 and np.all(np.abs(np.delete(d, [5, 9, 14])) < 0.51)
    H = G.hierarchy("csr_dyadic")
    hy = G.Hierarchy(H, 0, 1, None, True, *G.CSR_DYADIC_WINDOW)
    assert [hy.L[l]["theta"] for l in range(2)] == [1.0, 1.0] and [hy.info(l)[1] for l in range(3)] == [0, 0, 0]
    b = G.rhs_dyadic("csr_dyadic", 200)
    for r in range(G.R):
        exact = G.exact_cycle_degree1(H, b[:, r])
        assert np.array_equal(hy.apply(b[:, r]), exact)
        assert np.array_equal(np.asarray(_long_double(hy, b[:, r]), np.float64), exact)  # and exact in long double, in another order


def test_refusals_of_the_8_column_form():
    base = G.hierarchy("congruent8")
    hy = G.Hierarchy(base, 2)
    assert G.Hierarchy8(hy, 8).info(0)[:2] == [180, 8]
    Hp = dict(base, coarse_pinv=base["coarse_pinv"].copy())
    Hp["coarse_pinv"][-1] *= 1.5
    with pytest.raises(G.Unsupported, match="coarse pseudo-inverses of the congruent blocks differ"):
        G.Hierarchy8(G.Hierarchy(Hp, 2), 8)
    A1 = dict(base["A"][1], val=base["A"][1]["val"].copy())
    A1["val"][-1] *= 1.5
    with pytest.raises(G.Unsupported, match="not congruent on every level"):
        G.Hierarchy8(G.Hierarchy(dict(base, A=[base["A"][0], A1, base["A"][2]]), 2), 8)
    with pytest.raises(G.Unsupported, match="needs 3x3-block operators"):
        G.Hierarchy(G.hierarchy("csr_dyadic"), 1)
