"""tests/cg_cases.py against arithmetic that owes it nothing: a lane-by-lane simulation of the shuffles for its summation trees, a long-double direct solve and a plain
long-double CG for the model, three summation orders for the claim that the pair matrices' product has no order, and the conditions the GPU cases rely on (which
columns and blocks stop where, what the atol and the kernel-load cases reach, which wgs each shape gives).  No GPU."""
import numpy as np
import pytest

import cg_cases as CC

LD = np.longdouble


# ---- trees ---------------------------------------------------------------------------------------------------------------------------------------------------------
def _shfl_down_block(v):
    """pmh_block_reduce lane by lane: v[256] -> thread 0's value."""
    w = v.reshape(4, 64).copy()
    for o in (32, 16, 8, 4, 2, 1):
        src = np.arange(64) + o
        w = w + np.where(src < 64, w[:, np.minimum(src, 63)], w)  # __shfl_down past the wave's end returns the lane's own value
    r = w[0, 0]
    for k in range(1, 4):
        r = r + w[k, 0]
    return r


def _xor_red8(v):
    """mvc_red8 lane by lane: v[256] -> the 8 values threads 0 .. 7 return."""
    w = v.reshape(4, 64).copy()
    for o in (8, 16, 32):
        w = w + w[:, np.arange(64) ^ o]
    lds = w[:, :8].reshape(-1)  # lds[wave * 8 + lane]
    return np.array([(lds[c] + lds[8 + c]) + (lds[16 + c] + lds[24 + c]) for c in range(8)])


@pytest.mark.parametrize("wgs", [1, 2, 33, 65, 256])
def test_seg_total_is_the_shuffle_tree(wgs):
    rng = np.random.default_rng(wgs)
    part = rng.standard_normal(wgs) * 10.0 ** rng.integers(-6, 7, size=wgs)
    v = np.zeros(256)
    v[:wgs] = part
    assert CC.seg_total(part) == _shfl_down_block(v)
    assert CC.seg_coef_total(part) == _shfl_down_block(v)
    lanes = rng.standard_normal((3, 256)) * 10.0 ** rng.integers(-6, 7, size=(3, 256))
    assert np.array_equal(CC.block_reduce(lanes), [_shfl_down_block(x) for x in lanes])
    one_wave = np.concatenate([lanes[0, :64], np.zeros(192)])
    assert CC.wave_reduce(lanes[0, :64]) == _shfl_down_block(one_wave)


@pytest.mark.parametrize("wgs", [1, 2, 33, 65, 256, 512])
def test_mvc_total_is_the_xor_tree(wgs):
    rng = np.random.default_rng(100 + wgs)
    part = rng.standard_normal((2, wgs, 8)) * 10.0 ** rng.integers(-6, 7, size=(2, wgs, 8))
    for b in range(2):
        s = np.zeros(256)
        for t in range(256):  # thread t: column t % 8, partials w = t / 8, t / 8 + 32, ...
            for w in range(t // 8, wgs, 32):
                s[t] = s[t] + part[b, w, t % 8]
        assert np.array_equal(CC.mv_total(part)[b], _xor_red8(s))
    lanes = rng.standard_normal((5, 32, 8)) * 10.0 ** rng.integers(-6, 7, size=(5, 32, 8))
    assert np.array_equal(CC.tree32(lanes), [_xor_red8(x.reshape(-1)) for x in lanes])


def test_lane_maps():
    """SEG_LOOP and MV_ROW_LOOP element by element on blocks that leave workgroups without rows."""
    rng = np.random.default_rng(5)
    term = rng.standard_normal(1300)
    for lo, hi, wgs in ((7, 10, 3), (0, 1300, 2), (100, 1129, 5)):
        want = np.zeros((wgs, 256))
        for w in range(wgs):
            for t in range(256):
                for i in range(lo + 256 * w + t, hi, 256 * wgs):
                    want[w, t] = want[w, t] + term[i]
        assert np.array_equal(CC.seg_lane_sums(term, lo, hi, wgs), want)
    term8 = rng.standard_normal((300, 8))
    for lo, hi, wgs in ((7, 10, 3), (0, 300, 2), (11, 140, 33)):
        want = np.zeros((wgs, 32, 8))
        for w in range(wgs):
            for t in range(256):
                for i in range(lo + 32 * w + t // 8, hi, 32 * wgs):
                    want[w, t // 8, t % 8] = want[w, t // 8, t % 8] + term8[i, t % 8]
        assert np.array_equal(CC.mv_lane_sums(term8, lo, hi, wgs), want)


def test_shapes_give_the_workgroup_counts_they_are_aimed_at():
    for name, (sizes, wgs) in CC.SHAPES_ONE.items():
        assert CC.wgs_one(np.concatenate([[0], np.cumsum(sizes)])) == wgs, name
    for name, (sizes, wgs) in CC.SHAPES_BSR3.items():
        assert CC.wgs_one(np.concatenate([[0], np.cumsum(sizes)])) == wgs and all(s % 3 == 0 for s in sizes), name
    for name, (sizes, wgs) in CC.SHAPES_EIGHT.items():
        assert CC.wgs_eight(np.concatenate([[0], np.cumsum(sizes)])) == wgs and all(s % 3 == 0 for s in sizes), name
    assert len(CC.SHAPES_ONE["b40"][0]) == 40
    import bsr3_cases as BC

    for name in CC.SHAPES_BSR3:  # the conversion to 3 x 3 blocks must not decline them (blocks mostly empty), and some rows couple to another 3 x 3 block
        A = CC.matrix("3:" + name)
        M = dict(n=A.n, rowptr=A.K.indptr, col=A.K.indices, val=A.K.data)
        assert BC.restate(M, BC.F64, 0, 1) is not None, name
        assert A.n == 3 or np.any(A.i // 3 != A.j // 3)


# ---- the model against long-double arithmetic -----------------------------------------------------------------------------------------------------------------------
def _ld_cholesky_solve(Kd, f):
    """Dense long-double Cholesky solve (small blocks)."""
    n = len(f)
    L = np.zeros((n, n), LD)
    Kd = Kd.astype(LD)
    for j in range(n):
        L[j, j] = np.sqrt(Kd[j, j] - L[j, :j] @ L[j, :j])
        L[j + 1:, j] = (Kd[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    y = np.zeros(n, LD)
    for j in range(n):
        y[j] = (LD(f[j]) - L[j, :j] @ y[:j]) / L[j, j]
    x = np.zeros(n, LD)
    for j in range(n - 1, -1, -1):
        x[j] = (y[j] - L[j + 1:, j] @ x[j + 1:]) / L[j, j]
    return x


def _ld_solve(A, f):
    """K^-1 f in long double: K is a direct sum of SPD 2 x 2 matrices [d c; c d] and lone diagonal entries, solved pair by pair in closed form; every block of at most
    130 rows also by the dense Cholesky above, which must agree."""
    f = np.asarray(f).astype(LD)
    d, c = A.d.astype(LD), A.c.astype(LD)
    u = f / d
    det = d[A.i] * d[A.i] - c * c
    u[A.i], u[A.j] = (d[A.i] * f[A.i] - c * f[A.j]) / det, (d[A.i] * f[A.j] - c * f[A.i]) / det
    for b, m in enumerate(np.diff(A.rs)):
        if m <= 130 and f.ndim == 1:
            sl = slice(A.rs[b], A.rs[b + 1])
            x = _ld_cholesky_solve(A.K[sl, sl].toarray(), f[sl])
            assert np.max(np.abs(x - u[sl])) <= 1e-17 * np.max(np.abs(x)) + 1e-300
    return u


def _ld_matvec(A, p):
    y = A.d.astype(LD) * p
    np.add.at(y, A.i, A.c.astype(LD) * p[A.j])
    np.add.at(y, A.j, A.c.astype(LD) * p[A.i])
    return y


def _ld_cg(A, b, dinv, f, k):
    """k steps of plain preconditioned CG in long double for block b (the other blocks' entries are zero and stay zero)."""
    mask = A.block == b
    dinv, f = np.where(mask, dinv, 0.0).astype(LD), np.where(mask, f, 0.0).astype(LD)
    u, r = np.zeros_like(f), f.copy()
    z = dinv * r
    p, rz = z.copy(), r @ z
    for _ in range(k):
        Ap = _ld_matvec(A, p)
        alpha = rz / (p @ Ap)
        u, r = u + alpha * p, r - alpha * Ap
        z = dinv * r
        rzn = r @ z
        p, rz = z + (rzn / rz) * p, rzn
    return u


HOST_SHAPES = ["b3", "b1025", "3:b1026", "8:b4101"]


@pytest.mark.parametrize("jacobi", [True, False])
@pytest.mark.parametrize("shape", HOST_SHAPES)
def test_model_against_direct_solve_and_long_double_cg(shape, jacobi):
    A = CC.matrix(shape)
    K = lambda p: A.K @ p  # noqa: E731
    f = CC.random_load(A, 3)
    rtol = 1e-10
    m = CC.solve_one(K, A.rs, f, dinv=A.dinv(jacobi), rtol=rtol)
    assert m["done"] == 1 and m["nactive"] == 0
    assert np.linalg.norm(A.K @ m["u"] - f) <= 10 * rtol * np.linalg.norm(f)
    ref = _ld_solve(A, f)
    # |u - K^-1 f| <= |K^-1| |residual| <= cond(K) 10 rtol |K^-1 f|; the eigenvalues 2^e (1 -+ 2^-k), e in [-2, 2], lie in [1/8, 6]: cond(K) <= 48
    assert np.linalg.norm((m["u"] - ref).astype(np.float64)) <= 48 * 10 * rtol * np.linalg.norm(ref.astype(np.float64))
    F = CC.columns(A, jacobi, 4, "random")
    m8 = CC.solve_eight(K, A.rs, F, dinv=A.dinv(jacobi), rtol=rtol)
    assert np.linalg.norm(A.K @ m8["u"] - F) <= 10 * rtol * np.linalg.norm(F)
    checked = 0
    for k in range(1, 6):
        mk, mk8 = CC.solve_one(K, A.rs, f, dinv=A.dinv(jacobi), rtol=rtol, max_it=k), CC.solve_eight(K, A.rs, F, dinv=A.dinv(jacobi), rtol=rtol, max_it=k)
        for b in range(len(A.rs) - 1):
            sl = slice(A.rs[b], A.rs[b + 1])
            if mk["its"][b] == k:  # (a block that stopped earlier holds its last iterate)
                want = _ld_cg(A, b, A.dinv(jacobi), f, k)[sl]
                assert np.linalg.norm((mk["u"][sl] - want).astype(np.float64)) <= 1e-12 * np.linalg.norm(want.astype(np.float64))
                checked += 1
            for c in (0, 5):
                if mk8["its"][8 * b + c] == k:
                    want = _ld_cg(A, b, A.dinv(jacobi), F[:, c], k)[sl]
                    assert np.linalg.norm((mk8["u"][sl, c] - want).astype(np.float64)) <= 1e-12 * np.linalg.norm(want.astype(np.float64))
                    checked += 1
    assert checked >= 6


def test_projected_model_against_direct_solve():
    """With R set the model's u is P_R K^-1 P_R f (R need not be K's kernel)."""
    A = CC.matrix("b65537")
    K = lambda p: A.K @ p  # noqa: E731
    rtol = 1e-10
    for kdim in (1, 6, 8):
        R = CC.kernel_basis(A.rs, kdim, zero_block=1)
        f = CC.random_load(A, 7)
        m = CC.solve_one(K, A.rs, f, dinv=A.dinv(True), rtol=rtol, R=R)
        P = lambda v: v - sum(np.where(A.block == b, R[k], 0.0) * (R[k, A.rs[b]:A.rs[b + 1]] @ v[A.rs[b]:A.rs[b + 1]]) for b in range(3) for k in range(kdim))  # noqa: E731
        ref = P(_ld_solve(A, P(f)).astype(np.float64))
        assert np.linalg.norm(m["u"] - ref) <= 48 * 10 * rtol * np.linalg.norm(_ld_solve(A, P(f)).astype(np.float64))  # (as above; P_R does not increase a norm)


# ---- the product has no order ------------------------------------------------------------------------------------------------------------------------------------------
def _three_orders(Kcsr, p):
    ip, ci, va = Kcsr.indptr, Kcsr.indices, Kcsr.data
    assert np.max(np.diff(ip)) <= 2
    t = np.zeros((Kcsr.shape[0], 2) + p.shape[1:])
    has2 = np.diff(ip) == 2
    first = va[ip[:-1]].reshape((-1,) + (1,) * (p.ndim - 1)) * p[ci[ip[:-1]]]
    second = np.zeros_like(first)
    second[has2] = va[ip[:-1][has2] + 1].reshape((-1,) + (1,) * (p.ndim - 1)) * p[ci[ip[:-1][has2] + 1]]
    t[:, 0], t[:, 1] = first, second
    left = (0.0 + t[:, 0]) + t[:, 1]
    right = (0.0 + t[:, 1]) + t[:, 0]
    pairwise = (t[:, 0] + 0.0) + (t[:, 1] + 0.0)
    return left, right, pairwise


@pytest.mark.parametrize("shape", HOST_SHAPES)
def test_product_of_the_pair_matrices_has_no_order(shape):
    """Along the whole model run: K p summed left to right, right to left and pairwise are the same bits, and they are scipy's."""
    A = CC.matrix(shape)
    seen = []

    def K(p):
        y = A.K @ p
        for o in _three_orders(A.K, p):
            assert np.array_equal(o, y)
        seen.append(1)
        return y

    CC.solve_one(K, A.rs, CC.random_load(A, 3), dinv=A.dinv(False), rtol=1e-10)
    CC.solve_eight(K, A.rs, CC.columns(A, True, 4), dinv=A.dinv(True), rtol=1e-10)
    assert len(seen) > (20 if A.n > 3 else 4)  # (3 rows: 3 eigenvalues, 3 steps)
    assert np.all(np.log2(np.abs(A.K.data)) % 1 == 0)  # every entry a power of two: every product term exact


# ---- conditions of the cases -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jacobi", [True, False])
@pytest.mark.parametrize("shape", ["8:b3", "8:b4101"])
def test_staggered_columns_stop_at_different_iterations(shape, jacobi):
    A = CC.matrix(shape)
    m = CC.solve_eight(lambda p: A.K @ p, A.rs, CC.columns(A, jacobi, 4), dinv=A.dinv(jacobi))
    its = m["its"].reshape(-1, 8)
    b = int(np.argmax(np.diff(A.rs)))
    assert len(set(its[b])) >= 4, its
    assert np.all(its[:, 6] == 0) and m["done"] == 1


@pytest.mark.parametrize("jacobi", [True, False])
@pytest.mark.parametrize("shape", ["b65537", "b40"])
def test_staggered_blocks_stop_at_different_iterations(shape, jacobi):
    A = CC.matrix(shape)
    m = CC.solve_one(lambda p: A.K @ p, A.rs, CC.staggered_load(A, jacobi, 9), dinv=A.dinv(jacobi))
    assert len(set(m["its"])) >= 3 and m["done"] == 1, m["its"]


def test_atol_case():
    c = CC.ATOL_CASE
    A = CC.matrix("8:b4101")
    K = lambda p: A.K @ p  # noqa: E731
    F = np.random.default_rng(12).standard_normal((A.n, 8)) * c["scales"][None, :]
    m, m0 = CC.solve_eight(K, A.rs, F, dinv=A.dinv(False), rtol=c["rtol"], atol=c["atol"]), CC.solve_eight(K, A.rs, F, dinv=A.dinv(False), rtol=c["rtol"])
    big = slice(0, 8)  # the block of 4101 rows
    assert np.any(m["its"][big] == 0) and np.any((m["its"][big] > 0) & (m["its"][big] < m0["its"][big]))
    A1 = CC.matrix("b40")
    f = np.random.default_rng(13).standard_normal(A1.n) * c["scales"][A1.block % 8]
    m, m0 = CC.solve_one(lambda p: A1.K @ p, A1.rs, f, dinv=A1.dinv(False), rtol=c["rtol"], atol=c["atol"]), CC.solve_one(lambda p: A1.K @ p, A1.rs, f, dinv=A1.dinv(False), rtol=c["rtol"])
    assert np.any(m["its"] == 0) and np.any((m["its"] > 0) & (m["its"] < m0["its"]))


@pytest.mark.parametrize("shape", ["b65537", "8:b4101"])
def test_kernel_load_cases_are_not_decided_by_a_last_bit(shape):
    A = CC.matrix(shape)
    R = CC.kernel_basis(A.rs, 1)
    b = int(np.argmax(np.diff(A.rs)))
    for ratio, lo, hi in ((CC.INSIDE, 4, 32), (CC.OUTSIDE, 256, np.inf)):
        f = np.zeros(A.n)
        f[A.rs[b]:A.rs[b + 1]] = CC.kernel_load(R, A.rs, b, ratio)
        fp, fn = CC.project_one(f, R, A.rs, CC.wgs_one(A.rs), True)
        got = np.linalg.norm(fp[A.rs[b]:A.rs[b + 1]]) / (CC.EPS * np.sqrt(fn[b]))
        assert lo < got < hi, got


def test_breakdown_load_takes_the_nan_exit():
    for shape, solve in (("b65537", CC.solve_one), ("8:b4101", CC.solve_eight)):
        A = CC.matrix(shape, singular=True)
        f = CC.breakdown_load(A)
        assert np.all((A.K @ f) == 0.0)
        if solve is CC.solve_eight:
            f = np.stack([f] * 8, axis=1)
        m = solve(lambda p: A.K @ p, A.rs, f, dinv=A.dinv(True))
        assert m["its"].max() == 1 and m["done"] == 1 and np.isnan(m["rz"]).any() and np.isinf(m["u"]).any()
