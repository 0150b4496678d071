"""What the Nystroem map costs (docs/LAB_NOTEBOOK.md, "SVM Nystroem features"): one process, one GPU.

At n x d with m landmarks and D features (default 5 M x 64, m = D = 256), device events around each call: one warm-up call per variant, then `--runs` timed
calls, the variants alternated; median, minimum, maximum and the relative spread are reported.

    transform      pmh_nys_apply, rbf and poly (degree 3), fp64 and float32 Z
    kernel_block   pmh_nys_kernel alone (C = k(X, L), n x m doubles written to HBM)
    product        the identity product alone, Z = C M from an n x m array in HBM (pmh_rff_test_args at d = m)
    rff            RFFMap.transform at the same n, d, D, fp64 and float32 Z
    chunk sweep    transform (rbf and poly, fp64 Z) over chunk_rows from 4 096 up to n

Yardsticks, taken in the same process:

    copy    the device's copy rate (pmh_vec_copy of 2^27 doubles, 16 bytes of traffic per entry: the median of 10 after 3)
    bytes   the traffic a call cannot avoid over that rate: transform n (d size_x + D size_z); kernel_block n (d size_x + 8 m); product n (8 m + 8 D)
    flops   2 n (d m + m D) / 78.6 TFLOP/s for transform (2 n d m, 2 n m D for its halves), the fp64 matrix rate DESIGN.md holds k_fxo_gemm16 against

    python scripts/dev/nys_cost.py --out out/nys_cost.json
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import permon_amd as pa  # noqa: E402
from permon_amd import nystroem  # noqa: E402
from permon_amd._lib import check  # noqa: E402
from rff_cost import FP64_MATRIX_TFLOPS, copy_rate  # noqa: E402


def timed(ctx, calls, runs):
    """{name: [seconds]}: one warm-up call each, then `runs` rounds over all of them in turn."""
    for c in calls.values():
        c()
    ctx.sync()
    times = {k: [] for k in calls}
    for _ in range(runs):
        for k, c in calls.items():
            ctx.timer_start()
            c()
            times[k].append(ctx.timer_stop() * 1e-3)
    return times


def report(name, t, nbytes, flops, copy_GBps):
    med, byte_floor, flop_floor = float(np.median(t)), nbytes / (copy_GBps * 1e9), flops / (FP64_MATRIX_TFLOPS * 1e12)
    r = dict(ms_median=1e3 * med, ms_min=1e3 * min(t), ms_max=1e3 * max(t), spread_rel=(max(t) - min(t)) / med, bytes=nbytes, flops=flops, byte_floor_ms=1e3 * byte_floor,
             flop_floor_ms=1e3 * flop_floor, ratio_to_byte_floor=med / byte_floor, ratio_to_flop_floor=med / flop_floor, TFLOPs=flops / med / 1e12, GBps=nbytes / med / 1e9)
    print("%-28s %8.2f ms (min %.2f, max %.2f, spread %.1f %%) = %.2f x the byte floor %.2f ms, %.2f x the flop floor %.2f ms"
          % (name, r["ms_median"], r["ms_min"], r["ms_max"], 100 * r["spread_rel"], r["ratio_to_byte_floor"], r["byte_floor_ms"], r["ratio_to_flop_floor"], r["flop_floor_ms"]), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5_000_000)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--m", type=int, default=256)
    ap.add_argument("--D", type=int, default=256)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.runs >= 5 and a.D <= a.m
    n, d, m, D = a.n, a.d, a.m, a.D
    ctx = pa.Context(0)
    res = dict(device=ctx.name(), n=n, d=d, m=m, D=D, runs=a.runs, fp64_matrix_tflops=FP64_MATRIX_TFLOPS)
    cp = res["copy_GBps"] = copy_rate(ctx)
    X = np.random.default_rng(1).standard_normal((n, d))
    L = nystroem.sample_landmarks(X[:100000], m, 0)
    M, lam = nystroem.whitening(L, "rbf", 0.5 / d, n_components=D)
    assert M.shape == (m, D), "k(L, L) has only %d eigenvalues above rcond" % M.shape[1]
    res["condition"] = float(lam[0] / lam[-1])
    maps = dict(rbf=pa.NystroemMap.from_arrays(ctx, L, M, "rbf", 0.5 / d), poly=pa.NystroemMap.from_arrays(ctx, L, M, "poly", 1.0 / d, 1.0, 3))  # (the cost does not depend on M)
    ident, rff = pa.RFFMap.from_arrays(ctx, M, None, 1.0), pa.RFFMap(ctx, d, D, gamma=0.5 / d, seed=0)
    res["info"] = maps["rbf"].info()
    Xd = pa.DeviceSamples.from_numpy(ctx, X)
    del X
    Z = {8: pa.DeviceSamples.empty(ctx, n, D, np.float64), 4: pa.DeviceSamples.empty(ctx, n, D, np.float32)}
    Cb = pa.DeviceSamples.empty(ctx, n, m, np.float64)
    code = {8: 0, 4: 1}
    calls, cost = {}, {}
    for k, f in maps.items():
        for sz in (8, 4):
            calls["transform_%s_z%d" % (k, 8 * sz)] = lambda f=f, sz=sz: check(ctx.L.pmh_nys_apply(f.h, n, Xd.p, 0, Z[sz].p, code[sz]))
            cost["transform_%s_z%d" % (k, 8 * sz)] = (float(n) * (8 * d + sz * D), 2.0 * n * (d * m + m * D))
        calls["kernel_block_%s" % k] = lambda f=f: check(ctx.L.pmh_nys_kernel(f.h, n, Xd.p, 0, Cb.p))
        cost["kernel_block_%s" % k] = (float(n) * (8 * d + 8 * m), 2.0 * n * d * m)
    calls["product_identity"] = lambda: check(ctx.L.pmh_rff_test_args(ident.h, n, Cb.p, 0, Z[8].p))  # (Cb holds the last kernel block)
    cost["product_identity"] = (float(n) * (8 * m + 8 * D), 2.0 * n * m * D)
    for sz in (8, 4):
        calls["rff_transform_z%d" % (8 * sz)] = lambda sz=sz: check(ctx.L.pmh_rff_apply(rff.h, n, Xd.p, 0, Z[sz].p, code[sz]))
        cost["rff_transform_z%d" % (8 * sz)] = (float(n) * (8 * d + sz * D), 2.0 * n * d * D)
    print("copy rate %.0f GB/s; %s" % (cp, res["info"]), flush=True)
    res["variants"] = {k: report(k, t, *cost[k], cp) for k, t in timed(ctx, calls, a.runs).items()}
    if not a.no_sweep:
        RW = res["info"]["rows_per_workgroup"]
        rows = [r for r in (4096, 16384, 65536, 262144, 1048576) if r < n] + [(n + RW - 1) // RW * RW]
        res["chunk_sweep"] = {}
        for k, f in maps.items():
            sweep = {r: [] for r in rows}
            for rnd in range(a.runs + 1):  # the chunk sizes in turn, one round per run
                for r in rows:
                    f.set_chunk_rows(r)  # (the workspace is allocated anew here, outside the events)
                    ctx.sync()
                    ctx.timer_start()
                    check(ctx.L.pmh_nys_apply(f.h, n, Xd.p, 0, Z[8].p, 0))
                    t = ctx.timer_stop() * 1e-3
                    if rnd:  # (round 0 is the warm-up)
                        sweep[r].append(t)
            res["chunk_sweep"][k] = {str(r): report("transform_%s chunk %d" % (k, r), t, *cost["transform_%s_z64" % k], cp) for r, t in sweep.items()}
            f.set_chunk_rows(res["info"]["chunk_rows"])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    for s in [Xd, Cb] + list(Z.values()):
        s.free()
    for f in list(maps.values()) + [ident, rff]:
        f.destroy()
    ctx.close()


if __name__ == "__main__":
    main()
