"""GPU tests of the random Fourier feature map (csrc/rff.hip, permon_amd/rff.py): the kernel's indexing exactly on integer data over every edge of its tiling,
real data against bounds derived in tests/rff_cases.py, the bit identities of its contract (storage types, repeatability, a row alone and in a batch), guards
around every array, DeviceSamples through SVM / SVMMulticlass / SVR, the two rings a linear fit cannot separate, and the refusals."""
import ctypes as ct
import math

import numpy as np
import pytest

import permon_amd as pa
from permon_amd import rff
from permon_amd._lib import PermonHipError
from permon_amd.core import Vec, VecF32
from permon_amd.svm import cross_validate
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
    f = pa.RFFMap(ctx, 2, 4)
    info = f.info()
    f.destroy()
    assert info["rows_per_workgroup"] == info["rows_per_wave"] * info["waves_per_workgroup"] and info["rows_per_wave"] % 16 == 0
    assert info["column_tile"] % 16 == 0 and info["k_block"] % 4 == 0 and 0 < info["lds_bytes"] <= 160 * 1024
    return info["rows_per_workgroup"], info["column_tile"], info["k_block"]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _transform(fmap, X, out_dtype=np.float64):
    Z = fmap.transform(X, out_dtype)
    try:
        return Z.numpy()
    finally:
        Z.free()


# ---- 1. indexing, exact ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("xdt", [np.float64, np.float32])
def test_indexing_exact(ctx, tiles, xdt):
    for n, d, D in R.edge_shapes(*tiles):
        X, omega, beta = R.int_case(n, d, D, 10000 * n + 100 * d + D)
        fmap = pa.RFFMap.from_arrays(ctx, omega, beta, 1.0)
        T = fmap.arguments(X.astype(xdt))
        fmap.destroy()
        assert T.shape == (n, D) and np.array_equal(T, X @ omega + beta), (n, d, D)


# ---- 2. real data, derived bounds --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,D", R.REAL_SHAPES)
def test_real_data_within_derived_bounds(ctx, n, d, D):
    X, omega, beta = R.real_case(n, d, D, n + d + D)
    scale = math.sqrt(2.0 / D)
    fmap = pa.RFFMap.from_arrays(ctx, omega, beta, scale)
    T, Z = fmap.arguments(X), _transform(fmap, X)
    fmap.destroy()
    errT = np.abs(T.astype(np.longdouble) - R.args_longdouble(X, omega, beta)).astype(np.float64)
    bound = R.args_bound(X, omega, beta)
    print("arguments: max |T| %.1f, max error / bound %.3f" % (np.abs(T).max(), (errT / bound).max()))
    assert (errT <= bound).all()
    errZ = np.abs(Z - scale * np.cos(T))
    k = np.unravel_index(np.argmax(errZ), errZ.shape)
    print("features: max error %.3e = %.2f of the bound %.3e, at the argument %r" % (errZ[k], errZ[k] / R.cos_bound(scale), R.cos_bound(scale), T[k]))
    assert np.abs(T).max() > 100.0
    assert errZ[k] <= R.cos_bound(scale), "argument %r: %r against %r" % (T[k], Z[k], scale * np.cos(T[k]))


# ---- 3. bit identities -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,D", [(64, 256), (37, 100), (36, 160), (130, 257)])
def test_bit_identities(ctx, tiles, d, D):
    RW = tiles[0]
    n = 2 * RW + 3
    X, omega, beta = R.real_case(n, d, D, 7 * d + D)
    scale = math.sqrt(2.0 / D)
    fmap = pa.RFFMap.from_arrays(ctx, omega, beta, scale)
    Z = _transform(fmap, X)
    assert Z.dtype == np.float64 and Z.shape == (n, D) and np.isfinite(Z).all()
    assert _same_bits(_transform(fmap, X), Z)  # two calls
    Z32 = _transform(fmap, X, np.float32)
    assert Z32.dtype == np.float32 and _same_bits(Z32, Z.astype(np.float32))  # rounded once, at the store
    X32 = X.astype(np.float32)
    assert _same_bits(_transform(fmap, X32), _transform(fmap, X32.astype(np.float64)))  # a float32 enters as (double)x
    assert _same_bits(_transform(fmap, X32, np.float32), _transform(fmap, X32.astype(np.float64)).astype(np.float32))
    Xd = pa.DeviceSamples.from_numpy(ctx, X)
    assert _same_bits(_transform(fmap, Xd), Z) and np.array_equal(Xd.numpy(), X)  # a DeviceSamples in, still the caller's
    Xd.free()
    for i in (0, 5, RW + 17, 2 * RW - 1, 2 * RW, n - 1):  # the first, a middle and the last (partial) tile
        assert _same_bits(_transform(fmap, X[i:i + 1])[0], Z[i]), i
    T = fmap.arguments(X)
    assert _same_bits(fmap.arguments(X), T)
    assert (np.abs(Z - scale * np.cos(T)) <= R.cos_bound(scale)).all()  # apply is scale cos(.) of the very arguments test_args shows
    fmap.destroy()


def test_round_trip(ctx):
    omega, beta, scale = rff.draw(7, 40, 0.5, "laplacian", 4)
    f = pa.RFFMap.from_arrays(ctx, omega, beta, scale)
    assert (f.d, f.D) == (7, 40) and _same_bits(f.omega, omega) and _same_bits(f.beta, beta) and f.scale == scale
    f.destroy()
    with pytest.raises(RuntimeError):
        f.omega
    g = pa.RFFMap(ctx, 7, 40, gamma=0.5, kernel="laplacian", seed=4)
    assert _same_bits(g.omega, omega) and _same_bits(g.beta, beta) and g.scale == scale == math.sqrt(2.0 / 40)
    g.destroy()
    h = pa.RFFMap.from_arrays(ctx, omega, None, 2.0)  # no beta: all 0
    assert not h.beta.any() and h.scale == 2.0
    h.destroy()


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
    for n, d, D in ((RW + 5, 36, 100), (37, 7, 41)):
        X, omega, beta = R.real_case(n, d, D, 3 * n + d)
        X = X.astype(xdt)
        scale = math.sqrt(2.0 / D)
        plain = pa.RFFMap.from_arrays(ctx, omega, beta, scale)
        want = _transform(plain, X, zdt)
        plain.destroy()
        bo, po = _view(ctx, omega, pad, np.nan)
        bb, pb = _view(ctx, beta, pad, np.nan)
        h = ct.c_void_p()
        pa._lib.check(ctx.L.pmh_rff_create(ctx.h, d, D, po, pb, scale, ct.byref(h)))
        bo.free(), bb.free()  # (copied)
        f32x, f32z = xdt is np.float32, zdt is np.float32
        bx, px = _view(ctx, X, pad, np.nan, f32x)
        bz, pz = _view(ctx, np.full(n * D, SENT), pad, SENT, f32z)
        pa._lib.check(ctx.L.pmh_rff_apply(h, n, px, int(f32x), pz, int(f32z)))
        got = bz.to_numpy()
        assert (got[:pad] == SENT).all() and (got[pad + n * D:] == SENT).all(), (n, d, D)  # nothing written beside Z
        Z = got[pad:pad + n * D].reshape(n, D)
        assert np.isfinite(Z).all() and _same_bits(Z, want), (n, d, D)  # no NaN beside X, omega or beta reached a result
        # a NaN inside row i of X: row i of Z is NaN, every other row keeps its bits
        for i in (0, n // 2, n - 1):
            Xn = X.copy()
            Xn[i, d // 2] = np.nan
            bxn, pxn = _view(ctx, Xn, pad, np.nan, f32x)
            pa._lib.check(ctx.L.pmh_rff_apply(h, n, pxn, int(f32x), pz, int(f32z)))
            Zn = bz.to_numpy()[pad:pad + n * D].reshape(n, D)
            bxn.free()
            assert np.isnan(Zn[i]).all() and _same_bits(np.delete(Zn, i, 0), np.delete(want, i, 0)), (n, d, D, i)
        bx.free(), bz.free()
        ctx.L.pmh_rff_destroy(h)


# ---- 5. plumbing: DeviceSamples through the front ends ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ring_features(ctx):
    """The mapped rings, once: (fmap, X, y, t, Xt, yt, tt)."""
    c = R.RINGS
    X, y, t = R.rings(c["n_train"], c["seed_train"])
    Xt, yt, tt = R.rings(c["n_test"], c["seed_test"])
    fmap = pa.RFFMap(ctx, c["d"], c["D"], gamma=c["gamma"], seed=c["seed"])
    yield fmap, X, y, t, Xt, yt, tt
    fmap.destroy()


def _classes3(X, y):
    """Three classes on the rings: the inner ring, and the outer ring's two halves."""
    return np.where(y > 0, 0.0, np.where(X[:, 0] > 0, 1.0, 2.0))


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_plumbing_svm(ctx, ring_features, dt):
    fmap, X, y, _, Xt, yt, _ = ring_features
    Z, Zt = fmap.transform(X, dt), fmap.transform(Xt, dt)
    assert (Z.n, Z.d, Z.dtype) == (X.shape[0], fmap.D, dt)
    a = pa.SVM(ctx, C=10.0, options=OPTS, sample_dtype=dt).fit(Z, y)
    b = pa.SVM(ctx, C=10.0, options=OPTS, sample_dtype=dt).fit(Z.numpy(), y)
    assert _same_bits(a.w, b.w) and a.b == b.b and _same_bits(a.alpha, b.alpha)
    a.calibrate(Z, y), b.calibrate(Z.numpy(), y)
    assert a.calibration == b.calibration
    Zth = Zt.numpy()
    for call in ("decision_function", "predict", "predict_proba"):
        on_dev = getattr(a, call)(Zt)
        assert _same_bits(on_dev, getattr(a, call)(Zth)) and _same_bits(on_dev, getattr(b, call)(Zth)), call
    assert a.test(Zt, yt) == a.test(Zth, yt) == b.test(Zth, yt)
    m = np.arange(Z.n) % 4 != 0
    own = a.set_subset(m).train().test_own("held_out")
    assert own == b.set_subset(m).train().test_own("held_out") and own["TP"] + own["FP"] + own["TN"] + own["FN"] == int((~m).sum())
    cv = cross_validate(a.set_subset(None), k=3)
    assert len(cv["folds"]) == 3 and cv["accuracy"] == cross_validate(b.set_subset(None), k=3)["accuracy"] >= R.MAPPED_ACCURACY_FLOOR
    a.destroy(), b.destroy()
    assert _same_bits(Z.numpy(), _transform(fmap, X, dt))  # the handle is gone, the samples are still the caller's
    other = np.float32 if dt is np.float64 else np.float64
    with pytest.raises(ValueError) as e:
        pa.SVM(ctx, sample_dtype=other).fit(Z, y)
    assert "float32" in str(e.value) and "float64" in str(e.value)
    Z.free(), Zt.free()
    with pytest.raises(RuntimeError):
        pa.SVM(ctx, sample_dtype=dt).fit(Z, y)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_plumbing_svr(ctx, ring_features, dt):
    fmap, X, _, t, Xt, _, tt = ring_features
    Z, Zt = fmap.transform(X, dt), fmap.transform(Xt, dt)
    a = pa.SVR(ctx, C=10.0, epsilon=0.1, options=OPTS, sample_dtype=dt).fit(Z, t)
    b = pa.SVR(ctx, C=10.0, epsilon=0.1, options=OPTS, sample_dtype=dt).fit(Z.numpy(), t)
    assert _same_bits(a.w, b.w) and a.b == b.b and _same_bits(a.alpha, b.alpha)
    Zth = Zt.numpy()
    assert _same_bits(a.predict(Zt), a.predict(Zth)) and _same_bits(a.predict(Zt), b.predict(Zth))
    assert a.test(Zt, tt) == a.test(Zth, tt) == b.test(Zth, tt)
    m = np.arange(Z.n) % 4 != 0
    own = a.set_subset(m).train().test_own("held_out")
    assert own == b.set_subset(m).train().test_own("held_out") and own["n"] == int((~m).sum())
    cv = cross_validate(a.set_subset(None), k=3)
    assert len(cv["folds"]) == 3 and cv["r2"] == cross_validate(b.set_subset(None), k=3)["r2"] >= R.MAPPED_R2_FLOOR
    a.destroy(), b.destroy()
    assert _same_bits(Z.numpy(), _transform(fmap, X, dt))
    Z.free(), Zt.free()


def test_plumbing_multiclass(ctx, ring_features):
    """SVMMulticlass keeps its samples in fp64 (it has no sample_dtype): fp64 DeviceSamples go through, float32 ones are refused by name."""
    fmap, X, y, _, Xt, yt, _ = ring_features
    lab, labt = _classes3(X, y), _classes3(Xt, yt)
    Z, Zt = fmap.transform(X), fmap.transform(Xt)
    a = pa.SVMMulticlass(ctx, C=10.0, options=OPTS).fit(Z, lab)
    b = pa.SVMMulticlass(ctx, C=10.0, options=OPTS).fit(Z.numpy(), lab)
    assert a.K == 3 and _same_bits(a.W, b.W) and _same_bits(a.b, b.b)
    a.calibrate(Z, lab), b.calibrate(Z.numpy(), lab)
    Zth = Zt.numpy()
    for call in ("decision_function", "predict", "predict_proba"):
        on_dev = getattr(a, call)(Zt)
        assert _same_bits(on_dev, getattr(a, call)(Zth)) and _same_bits(on_dev, getattr(b, call)(Zth)), call
    ta, tb = a.test(Zt, labt), b.test(Zth, labt)
    assert ta["accuracy"] == tb["accuracy"] and np.array_equal(ta["confusion"], tb["confusion"]) and ta["accuracy"] >= 0.9
    m = np.arange(Z.n) % 4 != 0
    oa, ob = a.set_subset(m).train().test_own("held_out"), b.set_subset(m).train().test_own("held_out")
    assert oa["n"] == ob["n"] == int((~m).sum()) and np.array_equal(oa["confusion"], ob["confusion"])
    cv = cross_validate(a.set_subset(None), k=3)
    assert len(cv["folds"]) == 3 and cv["accuracy"] == cross_validate(b.set_subset(None), k=3)["accuracy"]
    a.destroy(), b.destroy()
    assert _same_bits(Z.numpy(), _transform(fmap, X))
    Z32 = fmap.transform(X, np.float32)
    with pytest.raises(ValueError) as e:
        pa.SVMMulticlass(ctx).fit(Z32, lab)
    assert "float32" in str(e.value) and "float64" in str(e.value)
    Z.free(), Zt.free(), Z32.free()


# ---- 6. the point of it --------------------------------------------------------------------------------------------------------------------------------------------
def test_rings_classification(ctx, ring_features):
    """A linear fit is a coin (0.56 with a CPU trainer on these points), the mapped fit separates the rings (1.00 on the CPU for D in {32, 64, 128}, gamma in
    {0.5, 1, 2}, seeds 0 .. 2)."""
    fmap, X, y, _, Xt, yt, _ = ring_features
    lin = pa.SVM(ctx, C=1.0, options=OPTS).fit(X, y)
    acc_lin = lin.test(Xt, yt)["accuracy"]
    lin.destroy()
    Z, Zt = fmap.transform(X), fmap.transform(Xt)
    svm = pa.SVM(ctx, C=10.0, options=OPTS).fit(Z, y)
    acc = svm.test(Zt, yt)["accuracy"]
    svm.destroy(), Z.free(), Zt.free()
    print("rings: linear accuracy %.4f, mapped accuracy %.4f" % (acc_lin, acc))
    assert acc_lin <= R.LINEAR_ACCURACY_CAP
    assert acc >= R.MAPPED_ACCURACY_FLOOR


def test_rings_regression(ctx, ring_features):
    """The ring's radius as the target: the linear r2 is below 0 on the CPU (-0.35), the mapped one 0.975 (0.95 .. 0.98 over the same grid as above)."""
    fmap, X, _, t, Xt, _, tt = ring_features
    lin = pa.SVR(ctx, C=10.0, epsilon=0.1, options=OPTS).fit(X, t)
    r2_lin = lin.test(Xt, tt)["r2"]
    lin.destroy()
    Z, Zt = fmap.transform(X), fmap.transform(Xt)
    svr = pa.SVR(ctx, C=10.0, epsilon=0.1, options=OPTS).fit(Z, t)
    r2 = svr.test(Zt, tt)["r2"]
    svr.destroy(), Z.free(), Zt.free()
    print("rings: linear r2 %.4f, mapped r2 %.4f" % (r2_lin, r2))
    assert r2_lin <= R.LINEAR_R2_CAP
    assert r2 >= R.MAPPED_R2_FLOOR


# ---- 7. errors -----------------------------------------------------------------------------------------------------------------------------------------------------
def _refused(ctx, rc):
    assert rc == PMH_ERR_ARG
    msg = ctx.L.pmh_last_error().decode()
    assert "pmh_rff" in msg and len(msg) > 20
    return msg


def test_errors(ctx):
    omega, beta, scale = rff.draw(3, 8, 1.0, "rbf", 0)
    od, bd = ctx.vec_from(omega.ravel()), ctx.vec_from(beta)
    h = ct.c_void_p()
    for d, D in ((0, 8), (3, 0), (-1, 8)):
        _refused(ctx, ctx.L.pmh_rff_create(ctx.h, d, D, od.p, bd.p, scale, ct.byref(h)))
        assert not h.value
    for s in (float("nan"), float("inf")):
        assert "scale" in _refused(ctx, ctx.L.pmh_rff_create(ctx.h, 3, 8, od.p, bd.p, s, ct.byref(h)))
    for what in (0, 1):
        bad = [omega.copy(), beta.copy()]
        bad[what].flat[5] = np.nan
        with pytest.raises(PermonHipError) as e:
            pa.RFFMap.from_arrays(ctx, bad[0], bad[1], scale)
        assert e.value.code == PMH_ERR_ARG and "not finite" in str(e.value)
    od.free(), bd.free()
    fmap = pa.RFFMap.from_arrays(ctx, omega, beta, scale)
    X = ctx.vec_from(np.ones(3 * 4))
    SENT = 7.25
    Z = ctx.vec_from(np.full(8 * 4, SENT))
    for xt, zt in ((2, 0), (0, 2), (-1, 0), (0, -1)):
        assert "type" in _refused(ctx, ctx.L.pmh_rff_apply(fmap.h, 4, X.p, xt, Z.p, zt))
    _refused(ctx, ctx.L.pmh_rff_test_args(fmap.h, 4, X.p, 2, Z.p))
    _refused(ctx, ctx.L.pmh_rff_apply(fmap.h, -1, X.p, 0, Z.p, 0))
    assert ctx.L.pmh_rff_apply(fmap.h, 0, X.p, 0, Z.p, 0) == 0 and ctx.L.pmh_rff_apply(fmap.h, 0, None, 0, None, 0) == 0  # n = 0: nothing is launched
    assert (Z.to_numpy() == SENT).all()
    Z0 = fmap.transform(np.empty((0, 3)))
    assert (Z0.n, Z0.d) == (0, 8) and Z0.numpy().shape == (0, 8)
    Z0.free()
    with pytest.raises(ValueError):
        fmap.transform(np.ones((4, 5)))  # another width
    with pytest.raises(ValueError):
        fmap.transform(np.ones((4, 3)), np.int32)
    X.free(), Z.free(), fmap.destroy()
