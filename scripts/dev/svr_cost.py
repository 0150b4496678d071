"""What the regression operator saves over posing SVR through the classification operator (docs/LAB_NOTEBOOK.md, "SVR"): one process, one GPU.

Per case: ms per product of MatCreateSVRDual on X (X kept once, streamed twice) against ms per product of MatCreateSVMDual on vstack(X, X) with labels
[+1; -1] (X stored twice, streamed four times) on the same vector u = [p; q], and a whole SVR fit.  Medians of `--rounds` windows of `--products` products,
the two operators alternated, timed by a host clock around work that ends in a device synchronise.  The device's copy rate (a device-to-device copy of 1 GiB,
read + write) is measured in the same process; the achieved rate of a product is its algorithmic bytes over its time:
  SVR, dense:           2 * s n d + 48 n      (s = 8 or 4 bytes per feature; p, q read twice, both halves written)
  doubled, dense:       4 * s n d + 80 n      (2n rows: a, y read, H a written, y read again)
The classification operator's kernels are the parent's (tests/golden pins their bits).  CSR carries no expectation: its figure is recorded.

    python scripts/dev/svr_cost.py --case dense64 --out out/svr_cost_dense64.json
    python scripts/dev/svr_cost.py --case dense64_f32 | dense130 | csr
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

CASES = {  # n, d, sample type, sparse
    "dense64": (2500000, 64, np.float64, None),
    "dense64_f32": (2500000, 64, np.float32, None),
    "dense130": (1000000, 130, np.float64, None),
    "csr": (2000000, 50000, np.float64, (60, 1.0)),
}


def window(ctx, H, u, out, k):
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(k):
        H.mult(u, out)
    ctx.sync()
    return 1e3 * (time.perf_counter() - t0) / k


def copy_rate(ctx, rounds):
    m = 1 << 27  # 1 GiB of doubles
    a, b = ctx.vec(m), ctx.vec(m)
    a.set(1.0)
    r = []
    for _ in range(rounds + 1):
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(4):
            check(ctx.L.pmh_vec_copy(ctx.h, m, a.p, b.p))
        ctx.sync()
        r.append(4 * 16.0 * m / (time.perf_counter() - t0) / 1e12)
    a.free(), b.free()
    return float(np.median(r[1:]))


def med(x):
    return dict(median=float(np.median(x)), min=min(x), max=max(x), spread_rel=(max(x) - min(x)) / float(np.median(x)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="dense64", choices=sorted(CASES))
    ap.add_argument("--n", type=int, default=0, help="override the case's n")
    ap.add_argument("--products", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--fit_rtol", type=float, default=1e-3)
    ap.add_argument("--fit_rounds", type=int, default=0, help="whole fits timed (0: as --rounds)")
    ap.add_argument("--out", default="out/svr_cost.json")
    a = ap.parse_args()
    n, d, dt, sparse = CASES[a.case]
    n = a.n or n
    ctx = pa.Context(0)
    res = dict(device=ctx.name(), case=a.case, n=n, d=d, sample_dtype=np.dtype(dt).name, products=a.products, rounds=a.rounds)
    res["copy_rate_TBps"] = copy_rate(ctx, a.rounds)
    p = P.svr_linear(n, d, 0.05, 5, sparse=sparse, b_true=3.0, C=0.1)
    X, t = p["X"], p["t"]
    if sparse is None and dt is np.float32:
        X = X.astype(np.float32)
    u = ctx.vec_from(np.random.default_rng(1).uniform(0.0, 1.0, 2 * n))
    out = ctx.vec(2 * n)
    work = {"svr": pa.MatCreateSVRDual(ctx, X, sample_dtype=None if sparse else dt)}
    try:
        if sparse is None:
            Xd = np.vstack([X, X])
        else:
            import scipy.sparse as sp

            Xd = sp.vstack([X, X]).tocsr()
        work["doubled_classification"] = pa.MatCreateSVMDual(ctx, Xd, np.concatenate([np.ones(n), -np.ones(n)]), sample_dtype=None if sparse else dt)
        del Xd
    except (pa._lib.PermonHipError, MemoryError) as ex:  # (the doubled samples may not fit: say so)
        res["doubled_classification"] = dict(error=str(ex))
    for H in work.values():
        window(ctx, H, u, out, 3)
    runs = {k: [] for k in work}
    for _ in range(a.rounds):  # alternated: a drift of the box hits both alike
        for k, H in work.items():
            runs[k].append(window(ctx, H, u, out, a.products))
    s = 4 if dt is np.float32 else 8
    nbytes = dict(svr=2.0 * s * n * d + 48.0 * n, doubled_classification=4.0 * s * n * d + 80.0 * n)
    for k, v in runs.items():
        res[k] = dict(ms_per_product=med(v), runs=v)
        if sparse is None:
            res[k]["algorithmic_bytes"] = nbytes[k]
            res[k]["achieved_TBps"] = nbytes[k] / (res[k]["ms_per_product"]["median"] * 1e-3) / 1e12
            res[k]["fraction_of_copy_rate"] = res[k]["achieved_TBps"] / res["copy_rate_TBps"]
    if "doubled_classification" in runs:
        a_, b_ = res["svr"]["ms_per_product"], res["doubled_classification"]["ms_per_product"]
        res["svr_over_doubled"] = a_["median"] / b_["median"]
        res["expected_by_bytes"] = nbytes["svr"] / nbytes["doubled_classification"] if sparse is None else None
        res["faster_beyond_spread"] = bool(a_["max"] < b_["min"])
    for H in work.values():  # the operators and the samples they keep on the device
        H.destroy()
        for v in H._keep:
            v.destroy() if hasattr(v, "destroy") else v.free()
    fits = []
    for _ in range(a.fit_rounds or a.rounds):
        svr = pa.SVR(ctx, loss="L2", C=0.1, epsilon=0.1, bias=True, options="-qps_rtol %g" % a.fit_rtol, sample_dtype=None if sparse else dt)
        svr.create(X, t)
        ctx.sync()
        t0 = time.perf_counter()
        svr.train()
        ctx.sync()
        st = svr.stats
        fits.append(dict(s=time.perf_counter() - t0, outer=st.outer_iterations, inner=st.inner_iterations, nmv=st.nmv, passes_X=st.passes_X, reason=st.reason, b=svr.b))
        svr.destroy()
    res["fit"] = dict(loss="L2", C=0.1, epsilon=0.1, bias=True, rtol=a.fit_rtol, seconds=med([f["s"] for f in fits]), runs=fits)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    strip = lambda v: {k: (strip(x) if isinstance(x, dict) else x) for k, x in v.items() if k != "runs"}
    print(json.dumps(strip(res)))
    ctx.close()


if __name__ == "__main__":
    main()
