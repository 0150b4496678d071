"""The K-column scoring sweep of csrc/svm_multi.hip against K calls of the binary predict, and SVMMulticlass.fit against K separate SVM.fit calls
(docs/LAB_NOTEBOOK.md, "SVM multiclass"): one process, one GPU.

  predict  (a) one pmh_svm_multi_predict / _csr (scores n x K and labels) on a model set with pmh_svm_multi_set_model;
           (b) K calls of pmh_svm_predict / _csr (scores and labels) on a binary handle of the same width -- the time of a sweep does not depend on the values of
               w, so one trained binary handle stands for "w = W_k" K times.
           Test samples stay on the device; device events; after a warm-up, `--reps` alternating rounds of `--inner` calls each; spread = (max - min) / median.
           Dense 2 M x 64 and 2 M x 130 (--dense-d for other widths); CSR 2 M x 50 000 x 60 (problems.svm_sparse, skew 1.0); K in {4, 10, 32}.  The copy ceiling of the same visit: a
           device-to-device copy of 1 GiB (read + write bytes over time).
  fit      wall time (host clock around calls that end in a synchronise) of SVMMulticlass.fit against K SVM.fit calls, uploads included, K = 10:
           dense 500 k x 64 (problems.svm_blobs) and sparse 500 k x 50 000 x 60 with the labels arg-max of ten random planes.

    python scripts/dev/svm_multi_speed.py --what dense,csr,fit --out out/svm_multi_speed.json
"""
import argparse
import ctypes as ct
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import permon_amd as pa  # noqa: E402
from permon_amd import _lib, problems as P  # noqa: E402
from permon_amd._lib import check  # noqa: E402
from permon_amd.mat import csr_from_scipy  # noqa: E402

KS = (4, 10, 32)
OPT = "-qps_rtol 1e-6"


def window(ctx, fn, inner):
    ctx.sync()
    ctx.timer_start()
    for _ in range(inner):
        fn()
    return ctx.timer_stop() / inner


def alternate(ctx, fa, fb, reps, inner):
    for _ in range(2):
        window(ctx, fa, 1), window(ctx, fb, 1)
    ta, tb = [], []
    for _ in range(reps):
        ta.append(window(ctx, fa, inner))
        tb.append(window(ctx, fb, inner))
    return ta, tb


def summary(ta, tb, bytes_a, bytes_b):
    ma, mb = float(np.median(ta)), float(np.median(tb))
    return dict(multi_ms=ta, binary_ms=tb, multi_ms_median=ma, binary_ms_median=mb, multi_spread_rel=(max(ta) - min(ta)) / ma, binary_spread_rel=(max(tb) - min(tb)) / mb,
                multi_algorithmic_bytes=bytes_a, binary_algorithmic_bytes=bytes_b, multi_TBs=bytes_a / ma / 1e9, binary_TBs=bytes_b / mb / 1e9, speedup=mb / ma,
                beats_beyond_spread=bool(max(ta) < min(tb)))


def copy_ceiling(ctx, reps):
    n = 1 << 27  # 1 GiB of doubles
    a, b = ctx.vec(n), ctx.vec(n)
    t = [window(ctx, lambda: check(ctx.L.pmh_vec_copy(ctx.h, n, a.p, b.p)), 5) for _ in range(reps + 1)][1:]
    a.free(), b.free()
    return dict(copy_ms=t, copy_TBs=16.0 * n / float(np.median(t)) / 1e9)


def predict_case(ctx, X, reps, inner):
    """X: (n, d) ndarray or scipy CSR, test samples; returns {K: summary}."""
    L, sparse = ctx.L, hasattr(X, "tocsr")
    n, d = X.shape
    path = "csr" if sparse else ("dense64" if d == 64 else "dense")
    Xd = csr_from_scipy(ctx, X) if sparse else ctx.vec_from(X.ravel())
    rng = np.random.default_rng(3)
    # the binary handle: trained on a few samples of the same width
    import scipy.sparse as sp
    X0 = sp.random(64, d, density=min(1.0, 20.0 / d), format="csr", random_state=1) if sparse else rng.standard_normal((64, d))
    y0 = np.where(np.arange(64) % 2 == 0, 1.0, -1.0)
    sb = pa.SVM(ctx, options=OPT).fit(X0, y0)
    sc, lb = ctx.vec(n), ctx.vec(n)
    out = {}
    for K in KS:
        m = pa.SVMMulticlass(ctx, options=OPT).create(X0, np.arange(64.0) % K)
        m.set_model(rng.standard_normal((K, d)), rng.standard_normal(K))
        S, Lb = ctx.vec(n * K), ctx.vec(n)
        if sparse:
            fa = lambda: check(L.pmh_svm_multi_predict_csr(m.h, Xd.h, S.p, Lb.p))  # noqa: E731
            fb = lambda: [check(L.pmh_svm_predict_csr(sb.h, Xd.h, sc.p, lb.p)) for _ in range(K)]  # noqa: E731
            nnz, nch = float(X.nnz), -(-K // m.chunk(path))
            ba, bb = 12.0 * nnz * nch + 4.0 * n + 8.0 * n * K + 8.0 * n, K * (12.0 * nnz + 4.0 * n + 16.0 * n)
        else:
            fa = lambda: check(L.pmh_svm_multi_predict(m.h, n, Xd.p, S.p, Lb.p))  # noqa: E731
            fb = lambda: [check(L.pmh_svm_predict(sb.h, n, Xd.p, sc.p, lb.p)) for _ in range(K)]  # noqa: E731
            # the issue's yardstick: one read of X for the K-column sweep (a sweep per chunk of classes reads it again: counted in multi_passes)
            ba, bb = 8.0 * n * d + 8.0 * n * K, K * (8.0 * n * d + 8.0 * n)
        ta, tb = alternate(ctx, fa, fb, reps, inner)
        r = summary(ta, tb, ba, bb)
        r["multi_passes"] = -(-K // m.chunk(path))
        out[K] = r
        print("predict", "csr" if sparse else "dense", (n, d), "K", K, json.dumps({k: v for k, v in r.items() if not k.endswith("_ms")}), flush=True)
        S.free(), Lb.free(), m.destroy()
    sc.free(), lb.free(), sb.destroy()
    Xd.destroy() if sparse else Xd.free()
    return out


def fit_case(ctx, X, labels, K):
    def timed(f):
        ctx.sync()
        t0 = time.perf_counter()
        f()
        ctx.sync()
        return time.perf_counter() - t0

    cls = np.unique(labels)
    assert cls.size == K
    m = pa.SVMMulticlass(ctx, options=OPT)
    tm = timed(lambda: m.fit(X, labels))
    W = m.W
    m.destroy()

    ys, done = [np.where(labels == c, 1.0, -1.0) for c in cls], []

    def binaries():
        for k in range(K):
            s = pa.SVM(ctx, options=OPT).fit(X, ys[k])
            done.append(s)  # compared and destroyed after the clock stops (SVMMulticlass.fit's own destroy is not timed either)

    tb = timed(binaries)
    for k, s in enumerate(done):
        assert np.array_equal(s.w, W[k])
        s.destroy()
    r = dict(n=X.shape[0], d=X.shape[1], K=K, multiclass_fit_seconds=tm, binary_fits_seconds=tb)
    print("fit", json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="dense,csr,fit")
    ap.add_argument("--n", type=int, default=2000000)
    ap.add_argument("--n-fit", type=int, default=500000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--dense-d", default="64,130", help="widths of the dense cases (64: the row-pair kernel; any other: one wavefront per row)")
    ap.add_argument("--lib", default="", help="another build of libpermonhip.so (csrc/svm_multi.hip compiled with -DSVMM_KC64= / -DSVMM_KCD= / -DSVMM_KCC=)")
    ap.add_argument("--out", default="out/svm_multi_speed.json")
    a = ap.parse_args()
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    assert a.reps >= 5
    what = a.what.split(",")
    ctx = pa.Context(0)
    res = dict(device=ctx.name(), n=a.n, reps=a.reps, inner=a.inner, KC={p: pa.SVMMulticlass.chunk(p) for p in ("dense64", "dense", "csr")}, copy=copy_ceiling(ctx, a.reps))
    print("copy ceiling %.2f TB/s" % res["copy"]["copy_TBs"], flush=True)

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)

    if "dense" in what:
        for d in [int(v) for v in a.dense_d.split(",")]:
            res["dense_%d" % d] = predict_case(ctx, np.random.default_rng(d).standard_normal((a.n, d)), a.reps, a.inner)
            save()
    if "csr" in what:
        res["csr"] = predict_case(ctx, P.svm_sparse(a.n, 50000, 60, 1.0, 0.5)["X"], a.reps, a.inner)
        save()
    if "fit" in what:
        p = P.svm_blobs(a.n_fit, 64, 10, 4.0, 1)
        res["fit_dense"] = fit_case(ctx, p["X"], p["labels"], 10)
        save()
        X = P.svm_sparse(a.n_fit, 50000, 60, 1.0, 0.5)["X"]
        planes = np.random.default_rng(2).standard_normal((10, 50000))
        res["fit_sparse"] = fit_case(ctx, X, np.argmax(np.asarray(X @ planes.T), axis=1).astype(np.float64), 10)
        save()
    res["copy_after"] = copy_ceiling(ctx, a.reps)
    save()
    ctx.close()


if __name__ == "__main__":
    main()
