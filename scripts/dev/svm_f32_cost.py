"""What storing the dense SVM samples in float32 saves in time and memory (docs/LAB_NOTEBOOK.md, "SVM float32 samples"): one process, one GPU.

The samples of problems.svm_offset(n, d, 3.0) are rounded to float32 once; an fp64 handle on the widened values and a float32 handle on the rounded ones then
hold the same numbers, and only the storage type of X differs.  Per type:
  * the lone product H v (two passes over X), `--products` of them per window;
  * d = 64: MPGP for `--steps` iterations from the zero iterate with the paired passes on (RunFixed), with no subset and under a random subset of the share
    `--share`: ms per pass over X by the operator's own pass count, and iterations per second.
The types are alternated `--rounds` times after `--warmup` iterations each, timed by a host clock around work that ends in a device synchronise.  The yardstick
is the fp64 handle of the same call.  `--types float64` runs on a library without the float32 entries too (the parent commit's, to show its fp64 figures did
not move).

    python scripts/dev/svm_f32_cost.py --n 5000000 --d 64 --out out/svm_f32_cost_5M_64.json
    python scripts/dev/svm_f32_cost.py --n 2000000 --d 130 --out out/svm_f32_cost_2M_130.json
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
from permon_amd import problems as P  # noqa: E402


def operator(ctx, X, y, typ):
    if typ == "float64":
        return pa.MatCreateSVMDual(ctx, X, y)  # (no keyword: the parent's library and front end run this line too)
    return pa.MatCreateSVMDual(ctx, X, y, sample_dtype=np.float32)


class Lone:
    """k products H v on one operator."""

    def __init__(self, ctx, H, n):
        self.ctx, self.H = ctx, H
        self.v, self.out = ctx.vec_from(np.random.default_rng(1).uniform(0.0, 1.0, n)), ctx.vec(n)

    def run(self, k):
        self.ctx.sync()
        p0, t0 = self.H.passes(), time.perf_counter()
        for _ in range(k):
            self.H.mult(self.v, self.out)
        self.ctx.sync()
        dt = time.perf_counter() - t0
        return dict(ms_per_product=1e3 * dt / k, ms_per_pass=1e3 * dt / max(self.H.passes() - p0, 1), products=k)


class Fixed:
    """MPGP on H_S (rhs = m, 0 <= a <= C) that runs exactly k iterations from the zero iterate."""

    def __init__(self, ctx, H, n, C, mask):
        self.ctx, self.H = ctx, H
        if mask is not None:
            H.set_subset(mask)
        qp = pa.QP(ctx)
        qp.SetOperator(H)
        qp.SetRhs(ctx.vec_from(np.ones(n) if mask is None else mask.astype(float)))
        self.x = ctx.vec_from(np.zeros(n))
        qp.SetInitialVector(self.x)
        qp.SetBox(None, ctx.vec_from(np.zeros(n)), ctx.vec_from(np.full(n, float(C))))
        self.qps = pa.QPS(ctx)
        self.qps.SetQP(qp)
        self.qps.SetType("mpgp")
        self.qps.SetUp()

    def run(self, k):
        self.x.set(0.0)
        check(self.ctx.L.pmh_mpgp_reset_statistics(self.qps._mpgp_handle()))
        self.ctx.sync()
        p0, t0 = self.H.passes(), time.perf_counter()
        st = self.qps.RunFixed(k)
        self.ctx.sync()
        dt = time.perf_counter() - t0
        passes = self.H.passes() - p0
        return dict(ms_per_pass=1e3 * dt / max(passes, 1), iterations_per_s=st.iteration / dt, ms_per_iteration=1e3 * dt / max(st.iteration, 1), iterations=st.iteration,
                    hessian_mults=st.nmv, cg=st.ncg, expansion=st.nexp, proportioning=st.nprop, passes_over_X=passes)


def summary(v, key):
    x = [r[key] for r in v]
    med = float(np.median(x))
    return {key + "_median": med, key + "_min": min(x), key + "_max": max(x), key + "_spread_rel": (max(x) - min(x)) / med}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5000000)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--types", default="float64,float32")
    ap.add_argument("--share", type=float, default=0.8)
    ap.add_argument("--products", type=int, default=20)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out", default="out/svm_f32_cost.json")
    a = ap.parse_args()
    types = a.types.split(",")
    ctx = pa.Context(0)
    p = P.svm_offset(a.n, a.d, 3.0)
    n, y = p["n"], p["y"]
    X32 = p["X"].astype(np.float32)
    del p["X"]
    host = dict(float32=X32, float64=X32.astype(np.float64) if "float64" in types else None)  # the same numbers in both types
    mask = np.random.default_rng(5).random(n) < a.share
    res = dict(device=ctx.name(), n=n, d=a.d, products=a.products, steps=a.steps, warmup=a.warmup, rounds=a.rounds, share=float(mask.mean()), device_bytes_of_X={t: int(host[t].nbytes) for t in types})
    work = {}
    for t in types:
        work[t, "lone_product"] = Lone(ctx, operator(ctx, host[t], y, t), n)
        if a.d == 64:  # (the paired passes are the d = 64 kernels': elsewhere MPGP costs lone products)
            work[t, "mpgp_paired"] = Fixed(ctx, work[t, "lone_product"].H, n, p["C"], None)
            work[t, "mpgp_paired_subset"] = Fixed(ctx, operator(ctx, host[t], y, t), n, p["C"], mask)
    for w in work.values():
        w.run(a.warmup)
    runs = {k: [] for k in work}
    for _ in range(a.rounds):  # alternated: a drift of the box hits every type alike
        for k, w in work.items():
            runs[k].append(w.run(a.products if k[1] == "lone_product" else a.steps))
    for (t, what), v in runs.items():
        keys = ["ms_per_product", "ms_per_pass"] if what == "lone_product" else ["ms_per_pass", "iterations_per_s", "ms_per_iteration"]
        res.setdefault(what, {})[t] = dict(**{k: x for key in keys for k, x in summary(v, key).items()}, runs=v)
    if len(types) == 2:
        for what, r in res.items():
            if isinstance(r, dict) and isinstance(r.get("float64"), dict) and isinstance(r.get("float32"), dict):
                r["fp64_over_fp32_ms_per_pass"] = r["float64"]["ms_per_pass_median"] / r["float32"]["ms_per_pass_median"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    strip = lambda v: {k: (strip(x) if isinstance(x, dict) else x) for k, x in v.items() if k != "runs"}
    print(json.dumps(strip(res)))
    ctx.close()


if __name__ == "__main__":
    main()
