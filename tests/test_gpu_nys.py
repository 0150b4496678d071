"""GPU tests of the Nystroem map (csrc/nys.hip, permon_amd/nystroem.py): the two kernels' indexing exactly on integer data over every edge of their tilings,
real data against the bounds derived in tests/nys_cases.py, the bit identities of the contract (storage types, repeatability, a row alone and in a batch, the chunk
size, stage B against the kernel tests/test_gpu_rff.py pins), guards around every array, the refusals, and the rings through SVM, SVR and SVMMulticlass."""
import ctypes as ct

import numpy as np
import pytest

import permon_amd as pa
from permon_amd import nystroem, problems
from permon_amd._lib import PermonHipError
from permon_amd.core import Vec, VecF32
import nys_cases as N
import rff_cases as R

pytestmark = pytest.mark.gpu
PMH_ERR_ARG = 2
OPTS = "-qps_rtol 1e-6"


@pytest.fixture(scope="module")
def ctx():
    c = pa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tiles(ctx):
    f = pa.NystroemMap.from_arrays(ctx, np.eye(2), np.eye(2))
    info = f.info()
    f.destroy()
    assert info["rows_per_workgroup"] == info["rows_per_wave"] * info["waves_per_workgroup"] and info["rows_per_wave"] % 16 == 0
    assert info["column_tile"] % 16 == 0 and info["k_block"] % 4 == 0 and 0 < info["lds_bytes"] <= 160 * 1024
    assert info["chunk_rows"] % info["rows_per_workgroup"] == 0 and info["workspace_bytes"] == 8 * info["chunk_rows"] * 2
    return info["rows_per_workgroup"], info["column_tile"], info["k_block"]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _host(S):
    try:
        return S.numpy()
    finally:
        S.free()


def _transform(fmap, X, out_dtype=np.float64):
    return _host(fmap.transform(X, out_dtype))


def _block(fmap, X):
    return _host(fmap.kernel_block(X))


# ---- 1. indexing, exact ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("xdt", [np.float64, np.float32])
def test_indexing_exact(ctx, tiles, xdt):
    for n, d, m in R.edge_shapes(*tiles):
        D = max(1, m - n % 3)
        X, L, M, c0 = N.int_case(n, d, m, D, 10000 * n + 100 * d + m)
        Xs, T = X.astype(xdt), X @ L.T
        lin = pa.NystroemMap.from_arrays(ctx, L, M, "poly", 1.0, c0, 1)
        assert np.array_equal(lin.arguments(Xs), T), (n, d, m)
        Cb = _block(lin, Xs)
        assert Cb.shape == (n, m) and np.array_equal(Cb, T + c0), (n, d, m)
        Z = _transform(lin, Xs)
        assert Z.shape == (n, D) and np.array_equal(Z, (T + c0) @ M), (n, d, m, D)
        lin.destroy()
        cub = pa.NystroemMap.from_arrays(ctx, L, M, "poly", 1.0, c0, 3)
        assert np.array_equal(_block(cub, Xs), (T + c0) * (T + c0) * (T + c0)), (n, d, m)
        cub.destroy()
        rbf = pa.NystroemMap.from_arrays(ctx, L, M, "rbf", 1.0)
        assert np.array_equal(rbf.distances(Xs), ((X[:, None, :] - L[None, :, :]) ** 2).sum(-1)), (n, d, m)  # the row norms reach the accumulator rows g + 4 r
        assert np.array_equal(rbf.arguments(Xs), T), (n, d, m)
        rbf.destroy()


@pytest.mark.parametrize("ztype", [np.float64, np.float32])
def test_stage_b_edges_exact(ctx, ztype):
    n, d = 37, 7
    for m, D in N.stage_b_shapes():
        X, L, M, c0 = N.int_case(n, d, m, D, 100 * m + D)
        f = pa.NystroemMap.from_arrays(ctx, L, M, "poly", 1.0, c0, 1)
        Z = _transform(f, X, ztype)
        f.destroy()
        assert Z.dtype == ztype and Z.shape == (n, D) and np.array_equal(Z, (X @ L.T + c0) @ M), (m, D)  # (below 2^24: exact in float32 too)


# ---- 2. real data, derived bounds --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,m", N.REAL_SHAPES)
def test_real_data_within_derived_bounds(ctx, n, d, m):
    D = max(1, m // 2)
    X, L, M, gamma = N.real_case(n, d, m, D, n + d + m)
    f = pa.NystroemMap.from_arrays(ctx, L, M, "rbf", gamma)
    T, Q, Cb, Z = f.arguments(X), f.distances(X), _block(f, X), _transform(f, X)
    f.destroy()
    errT = np.abs(T.astype(np.longdouble) - N.args_longdouble(X, L)).astype(np.float64)
    print("t: max |t| %.1f, max error / bound %.3f" % (np.abs(T).max(), (errT / N.args_bound(X, L)).max()))
    assert (errT <= N.args_bound(X, L)).all()
    errQ = np.abs(Q.astype(np.longdouble) - N.dist_longdouble(X, L)).astype(np.float64)
    print("q: max q %.1f, max error / bound %.3f" % (Q.max(), (errQ / N.dist_bound(X, L)).max()))
    assert (Q >= 0.0).all() and (errQ <= N.dist_bound(X, L)).all()
    errC = np.abs(Cb - np.exp(-(gamma * Q)))
    print("rbf: values in [%.3e, %.3f], max error %.3e = %.2f of the bound %.3e" % (Cb.min(), Cb.max(), errC.max(), errC.max() / N.RBF_BOUND, N.RBF_BOUND))
    assert (Cb <= 1.0).all() and Cb.max() > 0.1 and (errC <= N.RBF_BOUND).all()
    errZ = np.abs(Z.astype(np.longdouble) - Cb.astype(np.longdouble) @ M.astype(np.longdouble)).astype(np.float64)
    print("Z: max |Z| %.3f, max error / bound %.3f" % (np.abs(Z).max(), (errZ / N.product_bound(Cb, M)).max()))
    assert (errZ <= N.product_bound(Cb, M)).all()


# ---- 3. bit identities -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["rbf", "poly"])
@pytest.mark.parametrize("d,m,D", N.BIT_SHAPES)
def test_bit_identities(ctx, tiles, kernel, d, m, D):
    RW = tiles[0]
    n = 2 * RW + 3
    X, L, M, gamma = N.real_case(n, d, m, D, 7 * d + m)
    kw = dict(kernel="rbf", gamma=gamma) if kernel == "rbf" else dict(kernel="poly", gamma=0.01, coef0=1.0, degree=3)
    fmap = pa.NystroemMap.from_arrays(ctx, L, M, **kw)
    Z, Cb = _transform(fmap, X), _block(fmap, X)
    assert Z.dtype == np.float64 and Z.shape == (n, D) and np.isfinite(Z).all() and Cb.shape == (n, m)
    assert _same_bits(_transform(fmap, X), Z) and _same_bits(_block(fmap, X), Cb)  # two calls
    Z32 = _transform(fmap, X, np.float32)
    assert Z32.dtype == np.float32 and _same_bits(Z32, Z.astype(np.float32))  # rounded once, at the store
    X32 = X.astype(np.float32)
    assert _same_bits(_transform(fmap, X32), _transform(fmap, X32.astype(np.float64)))  # a float32 enters as (double)x
    assert _same_bits(_block(fmap, X32), _block(fmap, X32.astype(np.float64)))
    assert _same_bits(_transform(fmap, X32, np.float32), _transform(fmap, X32.astype(np.float64)).astype(np.float32))
    Xd = pa.DeviceSamples.from_numpy(ctx, X)
    assert _same_bits(_transform(fmap, Xd), Z) and _same_bits(_block(fmap, Xd), Cb) and np.array_equal(Xd.numpy(), X)  # a DeviceSamples in, still the caller's
    Xd.free()
    for i in (0, 5, RW + 17, 2 * RW - 1, 2 * RW, n - 1):  # the first, a middle and the last (partial) tile
        assert _same_bits(_transform(fmap, X[i:i + 1])[0], Z[i]) and _same_bits(_block(fmap, X[i:i + 1])[0], Cb[i]), i
    # three chunks, the last one partial, give the bits of one chunk
    assert fmap.info()["chunk_rows"] > n
    fmap.set_chunk_rows(RW)
    assert fmap.info()["chunk_rows"] == RW and fmap.info()["workspace_bytes"] == 8 * RW * m
    assert _same_bits(_transform(fmap, X), Z) and _same_bits(_transform(fmap, X, np.float32), Z32) and _same_bits(_block(fmap, X), Cb)
    if kernel == "rbf":
        Q = fmap.distances(X)
        fmap.set_chunk_rows(2 * RW)
        assert _same_bits(fmap.distances(X), Q)
        assert (np.abs(Cb - np.exp(-(gamma * Q))) <= N.RBF_BOUND).all()  # kernel_block is exp(-(gamma .)) of the very q test_args shows
    else:
        assert _same_bits(Cb, N.poly_of_args(fmap.arguments(X), 0.01, 1.0, 3))  # the epilogue, bit for bit, on the device's own products
    # stage B is the kernel that is already pinned: RFFMap's identity on the device's own C
    ident = pa.RFFMap.from_arrays(ctx, M, None, 1.0)
    assert _same_bits(ident.arguments(Cb), Z)
    ident.destroy()
    fmap.destroy()


def test_round_trip(ctx):
    X, _, _ = R.rings(50, 3)
    L = nystroem.sample_landmarks(X, 12, 1)
    f = pa.NystroemMap(ctx, L, kernel="rbf", gamma=0.5, n_components=9)
    Mr, lamr = N.whitening(L, "rbf", 0.5, n_components=9)
    assert (f.d, f.m, f.D) == (2, 12, 9) and _same_bits(f.landmarks, L) and _same_bits(f.M, Mr) and np.array_equal(f.eigenvalues, lamr)
    g = pa.NystroemMap.from_arrays(ctx, f.landmarks, f.M, "rbf", 0.5)
    assert g.eigenvalues is None and _same_bits(_transform(g, X), _transform(f, X))
    f.destroy(), g.destroy()
    with pytest.raises(RuntimeError):
        f.M
    with pytest.raises(RuntimeError):
        f.transform(X)


# ---- 4. guards ---------------------------------------------------------------------------------------------------------------------------------------------------
def _view(ctx, a, pad, fill, f32=False):
    """a inside a larger device buffer filled with `fill`, pad entries in front and behind: (the buffer, the pointer of the view)."""
    a = np.ascontiguousarray(a).ravel()
    host = np.full(a.size + 2 * pad, fill, dtype=np.float32 if f32 else np.float64)
    host[pad:pad + a.size] = a
    buf = (VecF32 if f32 else Vec).from_numpy(ctx, host)
    return buf, ct.c_void_p(buf.p.value + host.itemsize * pad)


@pytest.mark.parametrize("pad", [3, 4, 64])  # 3: no vector access is aligned; 4, 64: all are
@pytest.mark.parametrize("xdt,zdt", [(np.float64, np.float64), (np.float32, np.float32)])
def test_guards(ctx, tiles, pad, xdt, zdt):
    RW = tiles[0]
    SENT = 7.25
    for n, d, m, D in ((RW + 5, 36, 100, 64), (37, 7, 41, 41)):
        X, L, M, gamma = N.real_case(n, d, m, D, 3 * n + d)
        X = X.astype(xdt)
        plain = pa.NystroemMap.from_arrays(ctx, L, M, "rbf", gamma)
        wantZ, wantC = _transform(plain, X, zdt), _block(plain, X)
        plain.destroy()
        bl, pl = _view(ctx, L, pad, np.nan)
        bm, pm = _view(ctx, M, pad, np.nan)
        h = ct.c_void_p()
        pa._lib.check(ctx.L.pmh_nys_create(ctx.h, d, m, D, pl, 0, gamma, 1.0, 3, pm, ct.byref(h)))
        bl.free(), bm.free()  # (copied)
        f32x, f32z = xdt is np.float32, zdt is np.float32
        bx, px = _view(ctx, X, pad, np.nan, f32x)
        bz, pz = _view(ctx, np.full(n * D, SENT), pad, SENT, f32z)
        bc, pc = _view(ctx, np.full(n * m, SENT), pad, SENT)
        pa._lib.check(ctx.L.pmh_nys_apply(h, n, px, int(f32x), pz, int(f32z)))
        pa._lib.check(ctx.L.pmh_nys_kernel(h, n, px, int(f32x), pc))
        got, gotc = bz.to_numpy(), bc.to_numpy()
        assert (got[:pad] == SENT).all() and (got[pad + n * D:] == SENT).all(), (n, d, m, D)  # nothing written beside Z
        assert (gotc[:pad] == SENT).all() and (gotc[pad + n * m:] == SENT).all(), (n, d, m, D)  # nor beside C
        Z, Cb = got[pad:pad + n * D].reshape(n, D), gotc[pad:pad + n * m].reshape(n, m)
        assert np.isfinite(Z).all() and _same_bits(Z, wantZ) and _same_bits(Cb, wantC), (n, d, m, D)  # no NaN beside X, the landmarks or M reached a result
        # a NaN inside row i of X: row i of C and of Z is NaN, every other row keeps its bits
        for i in (0, n // 2, n - 1):
            Xn = X.copy()
            Xn[i, d // 2] = np.nan
            bxn, pxn = _view(ctx, Xn, pad, np.nan, f32x)
            pa._lib.check(ctx.L.pmh_nys_apply(h, n, pxn, int(f32x), pz, int(f32z)))
            pa._lib.check(ctx.L.pmh_nys_kernel(h, n, pxn, int(f32x), pc))
            Zn, Cn = bz.to_numpy()[pad:pad + n * D].reshape(n, D), bc.to_numpy()[pad:pad + n * m].reshape(n, m)
            bxn.free()
            assert np.isnan(Zn[i]).all() and _same_bits(np.delete(Zn, i, 0), np.delete(wantZ, i, 0)), (n, d, m, D, i)
            assert np.isnan(Cn[i]).all() and _same_bits(np.delete(Cn, i, 0), np.delete(wantC, i, 0)), (n, d, m, D, i)
        bx.free(), bz.free(), bc.free()
        ctx.L.pmh_nys_destroy(h)


# ---- 5. the point of it --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ring_data():
    c = N.RINGS
    X, y, t = R.rings(c["n_train"], c["seed_train"])
    Xt, yt, tt = R.rings(c["n_test"], c["seed_test"])
    return X, y, t, Xt, yt, tt, nystroem.sample_landmarks(X, c["m"], c["landmark_seed"])


def test_rings_rbf(ctx, ring_data):
    """A linear fit is a coin on these points (tests/test_gpu_rff.py); with 32 landmarks the CPU gives the accuracy 1.00 and the r2 0.981 (landmark seeds 0 .. 2)."""
    X, y, t, Xt, yt, tt, L = ring_data
    fmap = pa.NystroemMap(ctx, L, kernel="rbf", gamma=N.RINGS["gamma"])
    assert fmap.D <= fmap.m == N.RINGS["m"]
    Z, Zt = fmap.transform(X), fmap.transform(Xt)
    svm = pa.SVM(ctx, C=10.0, options=OPTS).fit(Z, y)
    acc = svm.test(Zt, yt)["accuracy"]
    svm.destroy()
    svr = pa.SVR(ctx, C=10.0, epsilon=0.1, options=OPTS).fit(Z, t)
    r2 = svr.test(Zt, tt)["r2"]
    svr.destroy(), Z.free(), Zt.free(), fmap.destroy()
    print("rings, rbf, m = %d, D = %d: accuracy %.4f, r2 %.4f" % (fmap.m, fmap.D, acc, r2))
    assert acc >= N.MAPPED_ACCURACY_FLOOR
    assert r2 >= N.MAPPED_R2_FLOOR


def test_rings_poly_is_exact(ctx, ring_data):
    """Degree 2 in 2 dimensions has rank 6: the map is exact once the landmarks span the feature space, which an indexing error in the rank-deficient path (D < m)
    would turn into an O(1) error."""
    X, y, _, Xt, yt, _, L = ring_data
    p = N.RINGS["poly"]
    kw = dict(kernel="poly", gamma=p["gamma"], coef0=p["coef0"], degree=p["degree"])
    fmap = pa.NystroemMap(ctx, L, **kw)
    assert fmap.D == p["D"] and fmap.m == N.RINGS["m"]
    Z, Zt = fmap.transform(X), fmap.transform(Xt)
    svm = pa.SVM(ctx, C=10.0, options=OPTS).fit(Z, y)
    acc = svm.test(Zt, yt)["accuracy"]
    svm.destroy()
    Zh = Zt.numpy()
    Z.free(), Zt.free(), fmap.destroy()
    K = N.gram(Xt, Xt, **kw)
    Zr = N.features(Xt, L, N.whitening(L, **kw)[0], **kw)
    own = float(np.abs(Zr @ Zr.T - K).max())
    err, cap = float(np.abs(Zh @ Zh.T - K).max()), max(N.EXACT_FACTOR * own, N.EXACT_FLOOR * float(np.abs(K).max()))
    print("rings, poly degree 2: D = %d, accuracy %.4f, |Z Z' - K| = %.3e (restatement %.3e, cap %.3e, max|K| %.1f)" % (p["D"], acc, err, own, cap, np.abs(K).max()))
    assert acc >= N.MAPPED_ACCURACY_FLOOR
    assert err <= cap


def test_multiclass_through_the_map(ctx):
    """The third front end: blobs mapped by an rbf map train and predict."""
    p = problems.svm_blobs(300, 4, 3, 4.0, 0, N_test=150)
    fmap = pa.NystroemMap(ctx, nystroem.sample_landmarks(p["X"], 24, 0), kernel="rbf", gamma=0.1)
    Z, Zt = fmap.transform(p["X"]), fmap.transform(p["X_test"])
    svm = pa.SVMMulticlass(ctx, C=10.0, options=OPTS).fit(Z, p["labels"])
    pred = svm.predict(Zt)
    acc = svm.test(Zt, p["labels_test"])["accuracy"]
    svm.destroy(), Z.free(), Zt.free(), fmap.destroy()
    print("blobs through an rbf map: accuracy %.4f" % acc)
    assert pred.shape == (150,) and set(np.unique(pred)) <= {0.0, 1.0, 2.0} and acc >= 0.9


# ---- 6. errors -----------------------------------------------------------------------------------------------------------------------------------------------------
def _refused(ctx, rc):
    assert rc == PMH_ERR_ARG
    msg = ctx.L.pmh_last_error().decode()
    assert "pmh_nys" in msg and len(msg) > 20
    return msg


def test_errors(ctx, tiles):
    RW = tiles[0]
    L, M = np.arange(24.0).reshape(8, 3), np.eye(8)[:, :5].copy()
    ld, md = ctx.vec_from(L.ravel()), ctx.vec_from(M.ravel())
    h = ct.c_void_p()

    def create(d=3, m=8, D=5, kernel=0, gamma=1.0, coef0=1.0, degree=3):
        msg = _refused(ctx, ctx.L.pmh_nys_create(ctx.h, d, m, D, ld.p, kernel, gamma, coef0, degree, md.p, ct.byref(h)))
        assert not h.value
        return msg

    for kw in (dict(d=0), dict(m=0), dict(D=0), dict(d=-1), dict(D=9)):
        create(**kw)
    for k in (2, -1):
        assert "kernel" in create(kernel=k)
    for g in (0.0, -1.0, float("nan"), float("inf")):
        assert "gamma" in create(gamma=g)
    for c in (float("nan"), float("inf")):
        assert "coef0" in create(coef0=c)
    for p in (0, 17, -3):
        assert "degree" in create(kernel=1, degree=p)
    ld.free(), md.free()
    for what in (0, 1):
        bad = [L.copy(), M.copy()]
        bad[what].flat[5] = np.nan if what else np.inf
        with pytest.raises(PermonHipError) as e:
            pa.NystroemMap.from_arrays(ctx, bad[0], bad[1], "rbf", 1.0)
        assert e.value.code == PMH_ERR_ARG and "not finite" in str(e.value)
    rbf, poly = pa.NystroemMap.from_arrays(ctx, L, M, "rbf", 1.0), pa.NystroemMap.from_arrays(ctx, L, M, "poly", 1.0, 1.0, 2)
    X = ctx.vec_from(np.ones(3 * 4))
    SENT = 7.25
    Z = ctx.vec_from(np.full(8 * 4, SENT))
    for xt, zt in ((2, 0), (0, 2), (-1, 0), (0, -1)):
        assert "type" in _refused(ctx, ctx.L.pmh_nys_apply(rbf.h, 4, X.p, xt, Z.p, zt))
    for xt in (2, -1):
        assert "type" in _refused(ctx, ctx.L.pmh_nys_kernel(rbf.h, 4, X.p, xt, Z.p))
        assert "type" in _refused(ctx, ctx.L.pmh_nys_test_args(rbf.h, 4, X.p, xt, 0, Z.p))
    _refused(ctx, ctx.L.pmh_nys_apply(rbf.h, -1, X.p, 0, Z.p, 0))
    _refused(ctx, ctx.L.pmh_nys_kernel(rbf.h, -1, X.p, 0, Z.p))
    _refused(ctx, ctx.L.pmh_nys_test_args(rbf.h, -1, X.p, 0, 0, Z.p))
    assert "what" in _refused(ctx, ctx.L.pmh_nys_test_args(poly.h, 4, X.p, 0, 1, Z.p))  # q on a polynomial map
    assert "what" in _refused(ctx, ctx.L.pmh_nys_test_args(rbf.h, 4, X.p, 0, 2, Z.p))
    with pytest.raises(PermonHipError):
        poly.distances(np.ones((4, 3)))
    for rows in (0, -RW, RW - 1, RW + 1, 3 * RW // 2):
        assert "rows" in _refused(ctx, ctx.L.pmh_nys_set_chunk_rows(rbf.h, rows))
    assert rbf.info()["chunk_rows"] % RW == 0
    # n = 0: nothing is launched
    for f in (rbf, poly):
        assert ctx.L.pmh_nys_apply(f.h, 0, X.p, 0, Z.p, 0) == 0 and ctx.L.pmh_nys_apply(f.h, 0, None, 0, None, 0) == 0
        assert ctx.L.pmh_nys_kernel(f.h, 0, None, 0, None) == 0 and ctx.L.pmh_nys_test_args(f.h, 0, None, 0, 0, None) == 0
    assert (Z.to_numpy() == SENT).all()
    Z0, C0 = rbf.transform(np.empty((0, 3))), rbf.kernel_block(np.empty((0, 3)))
    assert (Z0.n, Z0.d) == (0, 5) and Z0.numpy().shape == (0, 5) and C0.numpy().shape == (0, 8)
    Z0.free(), C0.free()
    with pytest.raises(ValueError):
        rbf.transform(np.ones((4, 5)))  # another width
    with pytest.raises(ValueError):
        rbf.transform(np.ones((4, 3)), np.int32)
    X.free(), Z.free(), rbf.destroy(), poly.destroy()
