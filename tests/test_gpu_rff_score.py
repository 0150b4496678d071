"""GPU tests of the scoring on random Fourier features that are never stored (csrc/rff_score.hip, RFFMap.lazy / dots): the kernel's indexing exactly on integer
data over every edge of the map's tiling and both sides of the class chunk, the cosine path inside the bound derived in tests/rff_score_cases.py, the bit
identities of its contract, guards around every array, the three front ends on lazy samples against the host's reductions of the very scores, and the
refusals."""
import ctypes as ct
import math

import numpy as np
import pytest

import permon_amd as pa
from permon_amd._lib import PermonHipError
from permon_amd.core import Vec, VecF32
import rff_score_cases as S

pytestmark = pytest.mark.gpu
PMH_ERR_ARG, PMH_ERR_STATE = 2, 3
OPTS = "-qps_rtol 1e-6"
U = S.U


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
    assert info["classes_per_chunk"] in (1, 2, 4) and info["lds_bytes"] < info["dots_lds_bytes"] <= 160 * 1024
    assert info["dots_lds_bytes"] == info["lds_bytes"] + 8 * info["classes_per_chunk"] * info["column_tile"]
    return info["rows_per_workgroup"], info["column_tile"], info["k_block"], info["classes_per_chunk"]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same_bits(a, b):
    return a.dtype == b.dtype == np.float64 and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ---- 1. indexing, exact ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("xdt", [np.float64, np.float32])
def test_indexing_exact(ctx, tiles, xdt):
    RW, CT, KB, kc = tiles
    Ks = S.chunk_counts(kc)
    for n, d, D in S.edge_shapes(RW, CT, KB):
        X, omega, beta = S.int_case(n, d, D, 10000 * n + 100 * d + D)
        W = S.int_weights(max(Ks), D, n + d + D)
        fmap = pa.RFFMap.from_arrays(ctx, omega, beta, 1.0)
        Xd = pa.DeviceSamples.from_numpy(ctx, X.astype(xdt))
        want = (X @ omega + beta) @ W.T
        for K in Ks:
            for ldw in (D, D + 3):
                got = fmap.dot_arguments(Xd, W[:K], ldw=ldw)
                assert got.shape == (n, K) and np.array_equal(got, want[:, :K]), (n, d, D, K, ldw)
        Xd.free(), fmap.destroy()


# ---- 2. the cosine path, derived bound -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,D", S.SCORE_SHAPES)
def test_cosine_path_within_derived_bound(ctx, n, d, D):
    X, omega, beta = S.real_case(n, d, D, n + d + D)
    scale = math.sqrt(2.0 / D)
    W = S.real_weights(S.SCORE_K, D, 31 * D + d)
    fmap = pa.RFFMap.from_arrays(ctx, omega, beta, scale)
    got = fmap.dots(X, W)
    fmap.destroy()
    ref, _, _ = S.dots_longdouble(X, omega, beta, scale, W)
    bound = S.dots_bound(X, omega, beta, scale, W)
    err = np.abs(got.astype(np.longdouble) - ref).astype(np.float64)
    k = np.unravel_index(np.argmax(err / bound), err.shape)
    print("(%d, %d, %d): max |dot| %.2f, max error %.3e, worst error / bound %.4f at %r" % (n, d, D, np.abs(got).max(), err.max(), err[k] / bound[k], k))
    assert got.shape == (n, S.SCORE_K) and np.isfinite(got).all()
    assert (err <= bound).all(), (k, got[k], ref[k])


# ---- 3. bit identities -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,D", S.BIT_SHAPES)
def test_bit_identities(ctx, tiles, d, D):
    RW = tiles[0]
    n = 2 * RW + 3
    X, omega, beta = S.real_case(n, d, D, 7 * d + D)
    W = S.real_weights(S.BIT_K, D, d + D)
    fmap = pa.RFFMap.from_arrays(ctx, omega, beta, math.sqrt(2.0 / D))
    dots = fmap.dots(X, W)
    assert dots.shape == (n, S.BIT_K) and np.isfinite(dots).all()
    assert _same_bits(fmap.dots(X, W), dots)  # two calls
    assert _same_bits(fmap.dots(X[:RW + 1], W), dots[:RW + 1])  # a batch of RW + 1
    for i in (0, 5, RW, RW + 17, 2 * RW - 1, 2 * RW, n - 1):  # a row alone, in the batch of RW + 1 (where it is inside) and in the batch of 2 RW + 3
        assert _same_bits(fmap.dots(X[i:i + 1], W)[0], dots[i]), i
    shifted = fmap.dots(X[3:RW + 4], W)  # another batch of RW + 1: the rows at other positions
    assert _same_bits(shifted, dots[3:RW + 4])
    for k in range(S.BIT_K):  # class k of the K = 7 model against the K = 1 call on W[k]
        assert _same_bits(fmap.dots(X, W[k])[:, 0], dots[:, k]), k
    assert _same_bits(fmap.dots(X, W, ldw=D + 3), dots)
    X32 = X.astype(np.float32)
    assert _same_bits(fmap.dots(X32, W), fmap.dots(X32.astype(np.float64), W))  # a float32 enters as (double)x
    for i in (0, RW - 1, n - 1):  # a NaN in one sample stays in that sample's dots
        Xn = X.copy()
        Xn[i, d // 2] = np.nan
        dn = fmap.dots(Xn, W)
        assert np.isnan(dn[i]).all() and _same_bits(np.delete(dn, i, 0), np.delete(dots, i, 0)), i
    fmap.destroy()


# ---- 4. guards ---------------------------------------------------------------------------------------------------------------------------------------------------
def _view(ctx, a, pad, fill, f32=False):
    """a inside a larger device buffer filled with `fill`, pad entries in front and behind: (the buffer, the pointer of the view)."""
    a = np.ascontiguousarray(a).ravel()
    host = np.full(a.size + 2 * pad, fill, dtype=np.float32 if f32 else np.float64)
    host[pad:pad + a.size] = a
    buf = (VecF32 if f32 else Vec).from_numpy(ctx, host)
    return buf, ct.c_void_p(buf.p.value + host.itemsize * pad)


@pytest.mark.parametrize("pad", [3, 4, 64])  # 3: no vector access is aligned; 4, 64: all are
@pytest.mark.parametrize("xdt", [np.float64, np.float32])
def test_guards(ctx, tiles, pad, xdt):
    RW, kc = tiles[0], tiles[3]
    SENT = 7.25
    f32x = xdt is np.float32
    for n, d, D in ((RW + 5, 36, 100), (37, 7, 41), (RW + 5, 8, 260)):
        K = kc + 1
        X, omega, beta = S.real_case(n, d, D, 3 * n + d)
        X = X.astype(xdt)
        W = S.real_weights(K, D, n + D)
        scale = math.sqrt(2.0 / D)
        fmap = pa.RFFMap.from_arrays(ctx, omega, beta, scale)
        want = fmap.dots(X, W)
        bx, px = _view(ctx, X, pad, np.nan, f32x)
        bw, pw = _view(ctx, W, pad, np.nan)  # ldw = D: nothing past W[K - 1, D - 1] may be read
        bz, pz = _view(ctx, np.full(n * K, SENT), pad, SENT)
        pa._lib.check(ctx.L.pmh_rffdots(fmap.h, n, px, int(f32x), K, pw, D, pz))
        got = bz.to_numpy()
        assert (got[:pad] == SENT).all() and (got[pad + n * K:] == SENT).all(), (n, d, D)  # nothing written beside dots
        Z = got[pad:pad + n * K].reshape(n, K)
        assert np.isfinite(Z).all() and _same_bits(Z, want), (n, d, D)  # no NaN beside X or W reached a result
        bx.free(), bw.free(), bz.free(), fmap.destroy()


# ---- 5. the front ends on the rings ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ring(ctx):
    """The rings, the map, the stored training features and the lazy test samples, once."""
    c = S.RINGS
    X, y, t = S.rings(c["n_train"], c["seed_train"])
    Xt, yt, tt = S.rings(c["n_test"], c["seed_test"])
    fmap = pa.RFFMap(ctx, c["d"], c["D"], gamma=c["gamma"], seed=c["seed"])
    Z, lazy = fmap.transform(X), fmap.lazy(Xt)
    assert isinstance(lazy, pa.MappedSamples) and lazy.shape == (Xt.shape[0], fmap.D) and lazy.map is fmap and lazy.owned
    yield dict(fmap=fmap, X=X, y=y, t=t, Xt=Xt, yt=yt, tt=tt, Z=Z, lazy=lazy, omega=fmap.omega, beta=fmap.beta, scale=fmap.scale)
    lazy.free(), Z.free(), fmap.destroy()


def _check_scores(r, w, b, score):
    """score against the long-double Z w + b of the model read back, within score_bound."""
    ref = S.dots_longdouble(r["Xt"], r["omega"], r["beta"], r["scale"], np.atleast_2d(w))[0] + np.atleast_1d(b).astype(np.longdouble)
    ref = ref.reshape(np.shape(score))
    err = np.abs(score.astype(np.longdouble) - ref).astype(np.float64)
    bound = S.score_bound(r["Xt"], r["omega"], r["beta"], r["scale"], w, b, score)
    print("scores: max |score| %.3f, max error %.3e, worst error / bound %.4f" % (np.abs(score).max(), err.max(), (err / bound).max()))
    assert (err <= bound).all()


def test_svm_on_lazy_samples(ctx, ring):
    r = ring
    lazy, yt = r["lazy"], r["yt"]
    svm = pa.SVM(ctx, C=10.0, options=OPTS).fit(r["Z"], r["y"])
    s = svm.decision_function(lazy)
    _check_scores(r, svm.w, svm.b, s)
    lab = svm.predict(lazy)
    host = np.where(s >= 0.0, 1.0, -1.0)  # svm_classify_row: s >= 0 is +1
    assert np.array_equal(lab, host)
    t = svm.test(lazy, yt)
    want = dict(TP=int(((host > 0) & (yt > 0)).sum()), FP=int(((host > 0) & (yt <= 0)).sum()), TN=int(((host <= 0) & (yt <= 0)).sum()), FN=int(((host <= 0) & (yt > 0)).sum()))
    assert {k: t[k] for k in want} == want and t["accuracy"] == (want["TP"] + want["TN"]) / yt.size
    print("rings through the lazy path: accuracy %.4f" % t["accuracy"])
    assert t["accuracy"] >= S.MAPPED_ACCURACY_FLOOR
    svm.calibrate(lazy, yt)
    A, B = svm.calibration
    assert (A, B) == pa.svm.platt_fit(ctx, s, yt)[:2]  # the fit on the very scores
    p = svm.predict_proba(lazy)
    errp = np.abs(p - S.sigmoid(A * s + B))
    print("probabilities: max error %.3e (%.2f u)" % (errp.max(), errp.max() / U))
    assert (errp <= 4 * U).all()
    # the features are never rounded: a handle trained on float32 features scores the same fp64 lazy features, whatever X's own type is
    Z32 = r["fmap"].transform(r["X"], np.float32)
    s32 = pa.SVM(ctx, C=10.0, options=OPTS, sample_dtype=np.float32).fit(Z32, r["y"])
    _check_scores(r, s32.w, s32.b, s32.decision_function(lazy))
    lazy32 = r["fmap"].lazy(r["Xt"].astype(np.float32))
    assert _same_bits(svm.decision_function(lazy32), svm.decision_function(r["fmap"].lazy(r["Xt"].astype(np.float32).astype(np.float64))))
    lazy32.free(), s32.destroy(), Z32.free(), svm.destroy()


def test_multiclass_on_lazy_samples(ctx, ring):
    r = ring
    lazy = r["lazy"]
    lab, labt = S.radius_classes(r["X"]), S.radius_classes(r["Xt"])
    m = pa.SVMMulticlass(ctx, C=10.0, options=OPTS).fit(r["Z"], lab)
    assert m.K == 3
    s = m.decision_function(lazy)
    assert s.shape == (lazy.n, 3)
    _check_scores(r, m.W, m.b, s)
    host = m.classes_[np.argmax(s, axis=1)]  # the greatest score; numpy's argmax takes the first of equals: the lowest class
    assert np.array_equal(m.predict(lazy), host)
    s2, l2 = m.predict_both(lazy)
    assert _same_bits(s2, s) and np.array_equal(l2, host)
    t = m.test(lazy, labt)
    conf = np.zeros((3, 3), dtype=np.int64)
    np.add.at(conf, (labt.astype(int), host.astype(int)), 1)
    assert np.array_equal(t["confusion"], conf) and t["n_unknown"] == 0 and t["accuracy"] == np.trace(conf) / labt.size
    m.calibrate(lazy, labt)
    A, B = m.calibration
    p = m.predict_proba(lazy)
    sig = S.sigmoid(A * s + B)
    tot = sig.sum(axis=1, keepdims=True)
    # sigma within 4 u each (the binary bound), its error and the sum's carried through p = sigma / sum, one rounding of the quotient
    bound = (4 * U + (sig / tot) * 3 * 4 * U) / tot + 2 * U
    errp = np.abs(p - sig / tot)
    print("multiclass probabilities: max error %.3e, worst error / bound %.3f; max |row sum - 1| %.3e" % (errp.max(), (errp / bound).max(), np.abs(p.sum(axis=1) - 1.0).max()))
    assert (errp <= bound).all()
    assert (np.abs(p.sum(axis=1) - 1.0) <= 2 * 3 * U).all()  # K quotients of one sum, each rounded once, added with K - 1 roundings
    # more classes than a chunk: a model that is set, K = 9 (the chunks 4 + 4 + 1 at four classes per chunk), ties to the lowest class across chunks
    lab9 = np.arange(r["X"].shape[0]) % 9.0
    m9 = pa.SVMMulticlass(ctx, options=OPTS).create(r["Z"], lab9)
    W9 = S.real_weights(9, r["fmap"].D, 9)
    W9[7] = W9[2]  # two classes in different chunks with equal scores everywhere
    b9 = np.linspace(-0.2, 0.2, 9)
    b9[7] = b9[2] = 1.0  # (and they lead on many samples)
    m9.set_model(W9, b9)
    s9, l9 = m9.predict_both(lazy)
    _check_scores(r, W9, b9, s9)
    assert _same_bits(s9[:, 7], s9[:, 2]) and np.array_equal(l9, np.argmax(s9, axis=1).astype(np.float64)) and (l9 == 2).any() and not (l9 == 7).any()
    assert np.array_equal(m9.predict(lazy), l9)
    m9.destroy(), m.destroy()


def test_svr_on_lazy_samples(ctx, ring):
    r = ring
    lazy, tt = r["lazy"], r["tt"]
    svr = pa.SVR(ctx, C=10.0, epsilon=0.1, options=OPTS).fit(r["Z"], r["t"])
    f = svr.predict(lazy)
    _check_scores(r, svr.w, svr.b, f)
    got = svr.test(lazy, tt)
    res = f - tt
    assert got["n"] == tt.size and got["n_in_tube"] == int((np.abs(res) <= svr.epsilon).sum()) and got["max_abs"] == np.abs(res).max()
    for key, want in (("sum_r", res.sum()), ("sum_r2", (res * res).sum()), ("sum_abs_r", np.abs(res).sum()), ("sum_t", tt.sum()), ("sum_t2", (tt * tt).sum())):
        scale = {"sum_r": np.abs(res).sum()}.get(key, abs(want))  # (a sum of signed terms: relative to the sum of their magnitudes)
        assert abs(got[key] - want) <= 1e-12 * scale, (key, got[key], want)
    print("rings through the lazy path: r2 %.4f" % got["r2"])
    assert got["r2"] >= S.R.MAPPED_R2_FLOOR
    svr.destroy()


# ---- 6. errors -----------------------------------------------------------------------------------------------------------------------------------------------------
def _refused(ctx, rc, code=PMH_ERR_ARG):
    assert rc == code
    msg = ctx.L.pmh_last_error().decode()
    assert len(msg) > 20
    return msg


def test_errors(ctx, ring):
    r = ring
    fmap, lazy = r["fmap"], r["lazy"]
    D = fmap.D
    X = ctx.vec_from(np.ones(2 * 4))
    W = ctx.vec_from(np.ones(2 * (D + 1)))
    SENT = 7.25
    out = ctx.vec_from(np.full(2 * 4, SENT))
    for entry in (ctx.L.pmh_rffdots, ctx.L.pmh_rffdots_test_args):
        for K in (0, -1):
            assert ("K = %d" % K) in _refused(ctx, entry(fmap.h, 4, X.p, 0, K, W.p, D, out.p))
        msg = _refused(ctx, entry(fmap.h, 4, X.p, 0, 2, W.p, D - 1, out.p))
        assert ("ldw = %d" % (D - 1)) in msg and ("D = %d" % D) in msg
        assert "n = -1" in _refused(ctx, entry(fmap.h, -1, X.p, 0, 2, W.p, D, out.p))
        assert "type" in _refused(ctx, entry(fmap.h, 4, X.p, 2, 2, W.p, D, out.p))
        for args in ((None, W.p, out.p), (X.p, None, out.p), (X.p, W.p, None)):
            assert "NULL" in _refused(ctx, entry(fmap.h, 4, args[0], 0, 2, args[1], D, args[2]))
        assert entry(fmap.h, 0, X.p, 0, 2, W.p, D, out.p) == 0 and entry(fmap.h, 0, None, 0, 2, None, D, None) == 0  # n = 0: nothing is launched
    assert (out.to_numpy() == SENT).all()
    assert fmap.dots(np.empty((0, 2)), np.ones((3, D))).shape == (0, 3)
    with pytest.raises(ValueError):
        fmap.dots(np.ones((4, 2)), np.ones((3, D + 1)))
    X.free(), W.free(), out.free()
    # the front ends
    svm = pa.SVM(ctx, C=10.0, options=OPTS).create(r["Z"], r["y"])
    n, args = lazy.n, lazy.entry_args()
    with _vec(ctx, n) as v:
        assert "train" in _refused(ctx, ctx.L.pmh_svm_predict_rff(svm.h, *args, v.p, None), PMH_ERR_STATE)  # an untrained handle
        svm.train()
        with pytest.raises(PermonHipError) as e:
            svm.predict_proba(lazy)  # no calibration
        assert e.value.code == PMH_ERR_STATE and "calibrat" in str(e.value)
        other = pa.RFFMap(ctx, 2, D + 8)  # another D than the handle's d
        ol = other.lazy(r["Xt"])
        msg = _refused(ctx, ctx.L.pmh_svm_predict_rff(svm.h, *ol.entry_args(), v.p, None))
        assert ("D = %d" % (D + 8)) in msg and ("d = %d" % D) in msg
        with pytest.raises(ValueError) as e:
            svm.decision_function(ol)
        assert str(D) in str(e.value)
        ol.free(), other.destroy()
    empty = fmap.lazy(np.empty((0, 2)))
    assert svm.decision_function(empty).shape == (0,)  # n = 0 succeeds
    cnt = (ct.c_longlong * 4)(1, 1, 1, 1)
    y0 = ctx.vec_from(np.ones(1))
    assert ctx.L.pmh_svm_test_rff(svm.h, fmap.h, 0, None, 0, y0.p, cnt) == 0 and list(cnt) == [0, 0, 0, 0]
    y0.free()
    empty.free()
    for train in (lambda: pa.SVM(ctx).fit(lazy, r["yt"]), lambda: pa.SVM(ctx).create(lazy, r["yt"]), lambda: pa.SVMMulticlass(ctx).fit(lazy, S.radius_classes(r["Xt"])),
                  lambda: pa.SVR(ctx).fit(lazy, r["tt"]), lambda: pa.MatCreateSVMDual(ctx, lazy, r["yt"])):
        with pytest.raises(TypeError) as e:
            train()
        assert "transform" in str(e.value)
    gone = fmap.lazy(r["Xt"][:4])
    gone.free()
    with pytest.raises(RuntimeError):
        svm.predict(gone)
    svm.destroy()


class _vec:
    def __init__(self, ctx, n):
        self.v = Vec(ctx, n, zero=False)

    def __enter__(self):
        return self.v

    def __exit__(self, *exc):
        self.v.free()
