"""What warm starts save in a grid search over C (docs/LAB_NOTEBOOK.md, "SVM warm starts"): one process, one GPU.

grid_search over `--Cs` (default 2^-4 ... 2^4, five points) with `--k` folds on one handle, warm against cold -- cold is the yardstick, run in the same process,
the two alternated `--rounds` times: wall time (a host clock around work that ends in a device synchronise), the Hessian multiplications and the passes over X
summed over the grid.  Beside it: the passes over X one set_penalties call spends (the eigenvalue estimate of the solver it builds anew; pmh_op_svm_dual_passes
before and after) as a share of a grid's passes, and the time of the start-vector entry (one launch over the n-vectors and the read of its two counts) beside one
product with H.

    python scripts/dev/svm_warm_cost.py --n 5000000 --d 64 --out profiles/svm_warm_cost_dense.json
    python scripts/dev/svm_warm_cost.py --n 5000000 --d 64 --f32 --out profiles/svm_warm_cost_f32.json
    python scripts/dev/svm_warm_cost.py --n 2000000 --csr 50000 60 --out profiles/svm_warm_cost_csr.json
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
from permon_amd import problems as P  # noqa: E402
from permon_amd._lib import check  # noqa: E402
from permon_amd.svm import grid_search  # noqa: E402


def passes(svm):
    k = ct.c_longlong()
    check(svm.L.pmh_op_svm_dual_passes(svm.solver_handles()[0], ct.byref(k)))
    return k.value


def one_grid(ctx, svm, a, warm):
    ctx.sync()
    p0, t0 = passes(svm), time.perf_counter()
    r = grid_search(svm, a.Cs, k=a.k, warm_start=warm, refit=False)
    ctx.sync()
    dt = time.perf_counter() - t0
    return dict(s_total=dt, nmv=int(np.sum(r["nmv"])), passes_X_solves=int(np.sum(r["passes_X"])), passes_X_all=passes(svm) - p0, nmv_cells=r["nmv"], score=r["score"], best_C=r["best_C"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5000000)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--f32", action="store_true", help="dense samples stored in float32")
    ap.add_argument("--csr", type=int, nargs=2, default=None, metavar=("N_FEATURES", "NNZ_ROW"))
    ap.add_argument("--Cs", type=float, nargs="+", default=[2.0 ** e for e in (-4, -2, 0, 2, 4)])
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--loss", default="L1")
    ap.add_argument("--bias", type=int, default=1)
    ap.add_argument("--rtol", type=float, default=1e-3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20, help="repetitions of the start-vector entry and of the product")
    ap.add_argument("--out", default="out/svm_warm_cost.json")
    a = ap.parse_args()
    ctx = pa.Context(0)
    p = P.svm_sparse(a.n, a.csr[0], a.csr[1], 1.0, 0.5, 1.0) if a.csr else P.svm_offset(a.n, a.d, 3.0)
    n = p["n"]
    svm = pa.SVM(ctx, loss=a.loss, C=1.0, bias=bool(a.bias), options="-qps_rtol %g" % a.rtol, sample_dtype=np.float32 if a.f32 else None).create(p["X"], p["y"])
    res = dict(device=ctx.name(), n=n, d=a.csr[0] if a.csr else a.d, csr=bool(a.csr), f32=bool(a.f32), loss=a.loss, bias=bool(a.bias), rtol=a.rtol, Cs=sorted(a.Cs), k=a.k, rounds=a.rounds)
    # one set_penalties call: the passes over X of the solver it builds anew
    p0 = passes(svm)
    svm.set_penalties(1.0, 1.0)
    res["passes_X_per_set_penalties"] = passes(svm) - p0
    # the start-vector entry beside one product
    svm.train()
    L, H = ctx.L, svm.solver_handles()[0]
    x, y = ctx.vec_from(np.random.default_rng(1).random(n)), ctx.vec(n)
    for name, f in (("start_vector", lambda: check(L.pmh_svm_warm_start_vector(svm.h, 2.0, y.p))), ("product", lambda: check(L.pmh_op_mult(H, x.p, y.p)))):
        f()
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            f()
        ctx.sync()
        res["ms_per_" + name] = 1e3 * (time.perf_counter() - t0) / a.reps
    x.free(), y.free()
    runs = dict(cold=[], warm=[])
    for _ in range(a.rounds):  # alternated: a drift of the machine hits both alike
        for mode in ("cold", "warm"):
            runs[mode].append(one_grid(ctx, svm, a, mode == "warm"))
    for mode, v in runs.items():
        res[mode] = dict(s_total_median=float(np.median([r["s_total"] for r in v])), s_total_min=min(r["s_total"] for r in v), s_total_max=max(r["s_total"] for r in v), nmv=v[0]["nmv"],
                         passes_X_solves=v[0]["passes_X_solves"], passes_X_all=v[0]["passes_X_all"], runs=v)
    res["cold_over_warm_time"] = res["cold"]["s_total_median"] / res["warm"]["s_total_median"]
    res["cold_over_warm_nmv"] = res["cold"]["nmv"] / res["warm"]["nmv"]
    calls = len(a.Cs) * a.k + 1  # (one per cell, one that puts the penalties back)
    res["set_penalties_share_of_passes_cold"] = calls * res["passes_X_per_set_penalties"] / res["cold"]["passes_X_all"]
    res["set_penalties_share_of_passes_warm"] = calls * res["passes_X_per_set_penalties"] / res["warm"]["passes_X_all"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({k: (v if not isinstance(v, dict) else {kk: vv for kk, vv in v.items() if kk != "runs"}) for k, v in res.items()}))
    svm.destroy()
    ctx.close()


if __name__ == "__main__":
    main()
