"""What a sample subset on the SVR dual operator costs or saves in time (docs/LAB_NOTEBOOK.md, "SVR subsets"): one GPU, every step a process of its own
under its own time limit (--what all runs them one after the other and stops at the first that fails or runs out of time).

--what product: ms per product of MatCreateSVRDual (L2 form: the scalar shift 1 / C, and the rank-one term, so the AUG = 1 instances run) with no subset, a
random subset and a contiguous subset of the share `--share` of the samples, all on ONE operator in one process (set_subset between the windows), so every
figure is relative to the same process's full-set product.  Dense rows in fp64 or float32 (--f32): --d; CSR: --csr N_FEATURES NNZ_ROW.  Windows of `--steps`
products after `--warmup`, the variants alternated `--rounds` times, timed by a host clock around work that ends in a device synchronise.

--what cv: k-fold cross_validate on one SVR handle (X uploaded once; CSR: one column-ordered copy) against k fresh handles on (X[mask], t[mask]) scored on the
held-out rows, wall time, alternated `--rounds` times; the folds' mse of both are reported side by side.

    python scripts/dev/svr_subset_cost.py --what all --out-dir out/svr_subset
    python scripts/dev/svr_subset_cost.py --what product --n 5000000 --d 64 --f32 --out out/svr_subset_f32.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def summary(x, key):
    med = float(np.median(x))
    return {key + "_median": med, key + "_min": float(min(x)), key + "_max": float(max(x)), key + "_spread_rel": (max(x) - min(x)) / med}


def samples(a, n, seed):
    """X alone (the product needs no targets): dense N(0, 1), or CSR with --csr[1] entries a row."""
    r = np.random.default_rng(seed)
    if not a.csr:
        return r.standard_normal((n, a.d), dtype=np.float32 if a.f32 else np.float64)
    import scipy.sparse as sp

    d, per = a.csr
    X = sp.csr_matrix((r.standard_normal(n * per), (np.repeat(np.arange(n), per), r.integers(0, d, n * per))), shape=(n, d))
    X.sum_duplicates()
    X.sort_indices()
    return X


def product(a, pa, ctx, res):
    n = a.n
    X = samples(a, n, 5)
    rng = np.random.default_rng(6)
    masks = dict(none=None, random=rng.random(n) < a.share, contiguous=np.arange(n) < int(a.share * n))
    H = pa.MatCreateSVRDual(ctx, X, sample_dtype=np.float32 if a.f32 else None)
    H.set_terms(1.0, 0.5 / n)
    u, out = ctx.vec_from(rng.uniform(0, 1, 2 * n)), ctx.vec(2 * n)
    res["nnz"] = int(X.nnz) if a.csr else None

    def window(k):
        ctx.sync()
        p0, t0 = H.passes(), time.perf_counter()
        for _ in range(k):
            H.mult(u, out)
        ctx.sync()
        dt = time.perf_counter() - t0
        assert H.passes() - p0 == 2 * k
        return 1e3 * dt / k

    runs = {k: [] for k in masks}
    for k, m in masks.items():
        H.set_subset(m)
        window(a.warmup)
    for _ in range(a.rounds):  # alternated: a drift of the box hits every variant alike
        for k, m in masks.items():
            H.set_subset(m)
            window(2)
            runs[k].append(window(a.steps))
    for k, v in runs.items():
        res[k] = dict(share=1.0 if masks[k] is None else float(masks[k].mean()), **summary(v, "ms_per_product"), runs=v)
    for k in ("random", "contiguous"):
        res[k + "_over_none"] = res[k]["ms_per_product_median"] / res["none"]["ms_per_product_median"]


def cv(a, pa, ctx, res):
    from permon_amd import problems as P
    from permon_amd.svm import cross_validate, kfold

    p = P.svr_linear(a.n, a.csr[0] if a.csr else a.d, 0.1, 5, sparse=(a.csr[1], 1.0) if a.csr else None, eps=0.1, C=0.1)
    X, t = p["X"], p["t"]
    sparse = bool(a.csr)
    masks = kfold(t, a.k, seed=0, stratified=False)
    opts = "-qps_rtol %g" % a.rtol
    dt = np.float32 if a.f32 else None
    mk = lambda: pa.SVR(ctx, loss="L2", C=0.1, epsilon=0.1, bias=True, options=opts, sample_dtype=dt)
    one, fresh, mse = [], [], {}
    for _ in range(a.rounds):
        ctx.sync()
        t0 = time.perf_counter()
        svr = mk().create(X, t)
        t1 = time.perf_counter()
        r = cross_validate(svr, k=a.k, seed=0)
        ctx.sync()
        t2 = time.perf_counter()
        svr.destroy()
        one.append(dict(s_create=t1 - t0, s_folds=t2 - t1, s_total=t2 - t0))
        mse["one_handle"] = [f["mse"] for f in r["folds"]]
        t0 = time.perf_counter()
        ms, t_slice = [], 0.0
        for m in masks:
            ts = time.perf_counter()
            Xm, tm, Xh, th = (X[np.flatnonzero(m)] if sparse else X[m]), t[m], (X[np.flatnonzero(~m)] if sparse else X[~m]), t[~m]
            t_slice += time.perf_counter() - ts  # (the host's row selection: reported, and left in the total: a caller pays it)
            s = mk().fit(Xm, tm)
            ms.append(s.test(Xh, th)["mse"])
            s.destroy()
        ctx.sync()
        t3 = time.perf_counter()
        fresh.append(dict(s_total=t3 - t0, s_host_row_selection=t_slice))
        mse["fresh_handles"] = ms
    res["one_handle"] = dict(**summary([x["s_total"] for x in one], "s_total"), **summary([x["s_create"] for x in one], "s_create"), **summary([x["s_folds"] for x in one], "s_folds"), runs=one)
    res["fresh_handles"] = dict(**summary([x["s_total"] for x in fresh], "s_total"), **summary([x["s_host_row_selection"] for x in fresh], "s_host_row_selection"), runs=fresh)
    res["fold_mse"] = mse
    res["fresh_over_one"] = res["fresh_handles"]["s_total_median"] / res["one_handle"]["s_total_median"]
    res["fresh_over_one_without_host_selection"] = (res["fresh_handles"]["s_total_median"] - res["fresh_handles"]["s_host_row_selection_median"]) / res["one_handle"]["s_total_median"]


def run_all(a):
    """Every step a child process under its own time limit; the first that fails or is killed at its limit ends the run (nothing more is started on the GPU)."""
    me = os.path.abspath(__file__)
    os.makedirs(a.out_dir, exist_ok=True)
    steps = [("dense_f64", ["--what", "product", "--n", str(a.n), "--d", "64"], 240), ("dense_f32", ["--what", "product", "--n", str(a.n), "--d", "64", "--f32"], 240),
             ("csr", ["--what", "product", "--n", str(a.n_csr), "--csr", "50000", "60"], 300), ("cv", ["--what", "cv", "--n", str(a.n_cv), "--d", "64", "--k", "5"], 300)]
    for name, args, limit in steps:
        cmd = [sys.executable, me] + args + ["--steps", str(a.steps), "--warmup", str(a.warmup), "--rounds", str(a.rounds), "--share", str(a.share), "--out", os.path.join(a.out_dir, name + ".json")]
        print("step", name, "limit", limit, "s:", " ".join(cmd[2:]), flush=True)
        try:
            rc = subprocess.run(cmd, timeout=limit).returncode
        except subprocess.TimeoutExpired:
            print("step", name, "ran into its time limit of", limit, "s: stopping", flush=True)
            return 124
        if rc != 0:
            print("step", name, "ended with status", rc, ": stopping", flush=True)
            return rc
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["product", "cv", "all"], default="product")
    ap.add_argument("--n", type=int, default=5000000)
    ap.add_argument("--n-csr", type=int, default=2000000, help="all: the samples of the CSR product")
    ap.add_argument("--n-cv", type=int, default=500000, help="all: the samples of the cross-validation")
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--f32", action="store_true", help="dense samples kept in float32")
    ap.add_argument("--csr", type=int, nargs=2, default=None, metavar=("N_FEATURES", "NNZ_ROW"))
    ap.add_argument("--share", type=float, default=0.8)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--rtol", type=float, default=1e-3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out", default="out/svr_subset_cost.json")
    ap.add_argument("--out-dir", default="out/svr_subset", help="all: one JSON file per step")
    a = ap.parse_args()
    if a.what == "all":
        sys.exit(run_all(a))
    import permon_amd as pa

    ctx = pa.Context(0)
    res = dict(device=ctx.name(), what=a.what, n=a.n, d=a.csr[0] if a.csr else a.d, csr=bool(a.csr), f32=bool(a.f32), steps=a.steps, warmup=a.warmup, rounds=a.rounds)
    (product if a.what == "product" else cv)(a, pa, ctx, res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({k: (v if not isinstance(v, dict) else {kk: vv for kk, vv in v.items() if kk != "runs"}) for k, v in res.items()}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
