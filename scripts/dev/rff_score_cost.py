"""What scoring on unstored random Fourier features costs against storing them first (docs/LAB_NOTEBOOK.md, "SVM fused feature scoring"): one process, one GPU.

At n x d -> D (default 5 M x 64 -> 256) and K = 1, 4 and 10 classes, device events around each call: one warm-up call per variant, then `--runs` timed calls,
the variants alternated; median, minimum, maximum and the relative spread are reported.

    fused     the scores of a handle on lazy samples: pmh_svm_predict_rff (K = 1), pmh_svm_multi_predict_rff (K = 4, 10), with fp64 and with float32 X;
              and pmh_rffdots alone, the same without the front end's kernel over the ready sums
    two-step  the same process's yardstick: pmh_rff_apply into a stored Z, then pmh_svm_predict / pmh_svm_multi_predict on it; fp64 Z, and (K = 1, the binary
              handle has a float32 sample type) float32 Z on a float32 handle
    floor     pmh_rff_test_args: the map's kernel without the cosines (it stores its n x D arguments)

The handles are created on the first `--train` rows of Z: the binary ones are trained on them, the multiclass ones get a model that is set (the timings do not
depend on the weights).  The copy rate is measured in the same process.  Device memory at the peak of each path is what its arrays hold: X, the n x K
workspace of dot products and the scores (fused); X, Z and the scores (two-step).

    python scripts/dev/rff_score_cost.py --out out/rff_score_cost.json
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import permon_amd as pa  # noqa: E402
from permon_amd._lib import check  # noqa: E402
from permon_amd.core import Vec  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rff_cost import copy_rate  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5_000_000)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--D", type=int, default=256)
    ap.add_argument("--K", type=int, nargs="+", default=[1, 4, 10])
    ap.add_argument("--train", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.runs >= 5 and a.n >= a.train
    ctx = pa.Context(0)
    L = ctx.L
    res = dict(device=ctx.name(), n=a.n, d=a.d, D=a.D, runs=a.runs)
    res["copy_GBps"] = copy_rate(ctx)
    fmap = pa.RFFMap(ctx, a.d, a.D, gamma=0.5 / a.d, seed=0)
    res["info"] = fmap.info()
    rng = np.random.default_rng(1)
    X = rng.standard_normal((a.n, a.d))
    src = {"f64": pa.DeviceSamples.from_numpy(ctx, X), "f32": pa.DeviceSamples.from_numpy(ctx, X.astype(np.float32))}
    Xs = X[:a.train].copy()
    del X
    Z = {"f64": pa.DeviceSamples.empty(ctx, a.n, a.D, np.float64), "f32": pa.DeviceSamples.empty(ctx, a.n, a.D, np.float32)}
    code = {"f64": 0, "f32": 1}
    Kmax = max(a.K)
    scores, dots = Vec(ctx, a.n * Kmax, zero=False), Vec(ctx, a.n * Kmax, zero=False)
    Wd = ctx.vec_from(rng.standard_normal(Kmax * a.D))
    # the handles, on the first rows' features
    Zs = {}
    for zs, dt in (("f64", np.float64), ("f32", np.float32)):
        Zd = fmap.transform(Xs, dt)
        Zs[zs] = Zd.numpy()
        Zd.free()
    y = np.where(rng.random(a.train) < 0.5, 1.0, -1.0)
    handles = {}
    if 1 in a.K:
        handles[(1, "f64")] = pa.SVM(ctx, C=1.0, options="-qps_rtol 1e-3").fit(Zs["f64"], y)
        handles[(1, "f32")] = pa.SVM(ctx, C=1.0, options="-qps_rtol 1e-3", sample_dtype=np.float32).fit(Zs["f32"], y)
    for K in a.K:
        if K > 1:
            m = pa.SVMMulticlass(ctx).create(Zs["f64"], np.arange(a.train) % float(K))
            handles[(K, "f64")] = m.set_model(rng.standard_normal((K, a.D)), rng.standard_normal(K))

    def fused(K, xs):
        h = handles[(K, "f64")]
        entry = L.pmh_svm_predict_rff if K == 1 else L.pmh_svm_multi_predict_rff
        return lambda: check(entry(h.h, fmap.h, a.n, src[xs].p, code[xs], scores.p, None))

    def two_step(K, zs):
        h = handles[(K, zs)]
        entry = (L.pmh_svm_predict_f32 if zs == "f32" else L.pmh_svm_predict) if K == 1 else L.pmh_svm_multi_predict

        def run():
            check(L.pmh_rff_apply(fmap.h, a.n, src["f64"].p, 0, Z[zs].p, code[zs]))
            check(entry(h.h, a.n, Z[zs].p, scores.p, None))
        return run

    variants = {"floor_test_args": lambda: check(L.pmh_rff_test_args(fmap.h, a.n, src["f64"].p, 0, Z["f64"].p))}
    mem = {}
    for K in a.K:
        for xs in ("f64", "f32"):
            variants["fused_K%d_x_%s" % (K, xs)] = fused(K, xs)
            variants["dots_K%d_x_%s" % (K, xs)] = (lambda K=K, xs=xs: check(L.pmh_rffdots(fmap.h, a.n, src[xs].p, code[xs], K, Wd.p, a.D, dots.p)))
            mem["fused_K%d_x_%s" % (K, xs)] = float(a.n) * (a.d * (8 if xs == "f64" else 4) + 16 * K)
        for zs in ("f64", "f32") if K == 1 else ("f64",):
            variants["two_step_K%d_z_%s" % (K, zs)] = two_step(K, zs)
            mem["two_step_K%d_z_%s" % (K, zs)] = float(a.n) * (a.d * 8 + a.D * (8 if zs == "f64" else 4) + 8 * K)
    times = {v: [] for v in variants}
    for f in variants.values():  # warm-up
        f()
    ctx.sync()
    for _ in range(a.runs):
        for v, f in variants.items():
            ctx.timer_start()
            f()
            times[v].append(ctx.timer_stop() * 1e-3)
    res["variants"] = {}
    for v, t in times.items():
        med = float(np.median(t))
        r = dict(ms_median=1e3 * med, ms_min=1e3 * min(t), ms_max=1e3 * max(t), spread_rel=(max(t) - min(t)) / med)
        if v in mem:
            r["device_GB_held"] = mem[v] / 1e9
        res["variants"][v] = r
        print("%-22s %8.2f ms (min %.2f, max %.2f, spread %.1f %%)%s" % (v, r["ms_median"], r["ms_min"], r["ms_max"], 100 * r["spread_rel"],
                                                                       "  %.2f GB held" % r["device_GB_held"] if v in mem else ""), flush=True)
    x_bytes = float(a.n) * a.d * 8
    print("copy rate %.0f GB/s: reading X once takes %.2f ms; tiling %s" % (res["copy_GBps"], 1e3 * x_bytes / (res["copy_GBps"] * 1e9), res["info"]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    for h in handles.values():
        h.destroy()
    for s in list(src.values()) + list(Z.values()) + [scores, dots, Wd]:
        s.free()
    fmap.destroy()
    ctx.close()


if __name__ == "__main__":
    main()
