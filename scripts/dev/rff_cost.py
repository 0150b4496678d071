"""What the random Fourier feature map costs (docs/LAB_NOTEBOOK.md, "SVM random features"): one process, one GPU.

pmh_rff_apply at n x d -> D (default 5 M x 64 -> 256) with fp64 and with float32 output (and, --x32, float32 input; --args, the arguments alone), device events around each call: one
warm-up call per variant, then `--runs` timed calls, the variants alternated; median, minimum, maximum and the relative spread are reported.  Two floors, taken
in the same process:

    bytes   (n d size_x + n D size_z) / the device's copy rate (pmh_vec_copy of 2^27 doubles, 16 bytes of traffic per entry: the median of 10 after 3)
    flops   2 n d D / 78.6 TFLOP/s, the fp64 matrix rate DESIGN.md holds k_fxo_gemm16 against

and the ratio of the measured median to each.  The n D cosines belong to neither floor: how far they hide under the products is what the ratios show.

    python scripts/dev/rff_cost.py --out out/rff_cost.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import permon_amd as pa  # noqa: E402
from permon_amd._lib import check  # noqa: E402

FP64_MATRIX_TFLOPS = 78.6


def copy_rate(ctx, m=1 << 27):
    """GB/s of a device-to-device copy of m doubles, the median of 10 after 3 warm-up copies."""
    x, y = ctx.vec(m), ctx.vec(m)
    t = []
    for it in range(13):
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(4):
            check(ctx.L.pmh_vec_copy(ctx.h, m, x.p, y.p))
        ctx.sync()
        if it >= 3:
            t.append((time.perf_counter() - t0) / 4)
    x.free(), y.free()
    return 16.0 * m / float(np.median(t)) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5_000_000)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--D", type=int, default=256)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--x32", action="store_true", help="also float32 input")
    ap.add_argument("--args", action="store_true", help="also pmh_rff_test_args (the same kernel with the identity in place of scale cos(.)): what the cosines cost")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.runs >= 5
    ctx = pa.Context(0)
    res = dict(device=ctx.name(), n=a.n, d=a.d, D=a.D, runs=a.runs, fp64_matrix_tflops=FP64_MATRIX_TFLOPS)
    res["copy_GBps"] = copy_rate(ctx)
    fmap = pa.RFFMap(ctx, a.d, a.D, gamma=0.5 / a.d, seed=0)
    res["info"] = fmap.info()
    rng = np.random.default_rng(1)
    X = rng.standard_normal((a.n, a.d))
    srcs = {"f64": pa.DeviceSamples.from_numpy(ctx, X)}
    if a.x32:
        srcs["f32"] = pa.DeviceSamples.from_numpy(ctx, X.astype(np.float32))
    del X
    variants = [(xs, zs) for xs in srcs for zs in ("f64", "f32")] + ([("f64", "args")] if a.args else [])
    outs = {zs: pa.DeviceSamples.empty(ctx, a.n, a.D, np.float64 if zs == "f64" else np.float32) for zs in ("f64", "f32")}
    code = {"f64": 0, "f32": 1}

    def call(xs, zs):
        if zs == "args":
            return check(ctx.L.pmh_rff_test_args(fmap.h, a.n, srcs[xs].p, code[xs], outs["f64"].p))
        check(ctx.L.pmh_rff_apply(fmap.h, a.n, srcs[xs].p, code[xs], outs[zs].p, code[zs]))

    times = {v: [] for v in variants}
    for v in variants:  # warm-up
        call(*v)
    ctx.sync()
    for _ in range(a.runs):
        for v in variants:
            ctx.timer_start()
            call(*v)
            times[v].append(ctx.timer_stop() * 1e-3)
    flop_floor = 2.0 * a.n * a.d * a.D / (FP64_MATRIX_TFLOPS * 1e12)
    res["flop_floor_ms"] = 1e3 * flop_floor
    res["variants"] = {}
    for (xs, zs), t in times.items():
        size = {"f64": 8, "f32": 4, "args": 8}
        nbytes = float(a.n) * a.d * size[xs] + float(a.n) * a.D * size[zs]
        byte_floor = nbytes / (res["copy_GBps"] * 1e9)
        med = float(np.median(t))
        r = dict(ms_median=1e3 * med, ms_min=1e3 * min(t), ms_max=1e3 * max(t), spread_rel=(max(t) - min(t)) / med, bytes=nbytes, byte_floor_ms=1e3 * byte_floor,
                 ratio_to_byte_floor=med / byte_floor, ratio_to_flop_floor=med / flop_floor, TFLOPs=2.0 * a.n * a.d * a.D / med / 1e12, GBps=nbytes / med / 1e9)
        res["variants"]["x_%s_z_%s" % (xs, zs)] = r
        print("X %s -> Z %s: %.2f ms (min %.2f, max %.2f, spread %.1f %%) = %.2f x the byte floor %.2f ms, %.2f x the flop floor %.2f ms"
              % (xs, zs, r["ms_median"], r["ms_min"], r["ms_max"], 100 * r["spread_rel"], r["ratio_to_byte_floor"], r["byte_floor_ms"], r["ratio_to_flop_floor"], res["flop_floor_ms"]), flush=True)
    print("copy rate %.0f GB/s; tiling %s" % (res["copy_GBps"], res["info"]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    for s in list(srcs.values()) + list(outs.values()):
        s.free()
    fmap.destroy()
    ctx.close()


if __name__ == "__main__":
    main()
