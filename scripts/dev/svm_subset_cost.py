"""What a sample subset on the SVM dual operator costs or saves in time (docs/LAB_NOTEBOOK.md, "SVM subsets"): one process, one GPU.

--what product: L1-loss dual without bias, MPGP on H_S for a fixed number of iterations with no subset, a random subset and a contiguous subset of the share
`--share` of the samples (dense rows: --d; CSR: --csr N_FEATURES NNZ_ROW).  `--shift S` / `--diag` put the scalar shift / a diagonal on the operator, so that
the AUG = 1 / AUG = 2 instances of the dense kernels run in place of the plain ones; `--unbounded` makes every step a CG step (k_svm_x64_p1<0, ...>).  A subset changes the problem, hence the steps; the figure that compares is the time
per pass over X (every variant's windows count their own passes).  Windows of `--steps` iterations from the zero iterate after `--warmup` iterations, the
variants alternated `--rounds` times, timed by a host clock around work that ends in a device synchronise.  `--variants none` runs on a library without the
subset entries too (the parent commit's, for the A/B of the unchanged instances).

--what cv: k-fold cross-validation of one handle (cross_validate: X uploaded once, one column-ordered copy) against k fresh handles on X[mask] (upload and,
for CSR, the copy build included), wall time, alternated `--rounds` times; the fold accuracies of both must agree.

    python scripts/dev/svm_subset_cost.py --what product --n 5000000 --d 64 --steps 100 --warmup 10 --rounds 4 --out out/svm_subset_dense.json
    python scripts/dev/svm_subset_cost.py --what product --n 2000000 --csr 50000 60 --out out/svm_subset_csr.json
    python scripts/dev/svm_subset_cost.py --what cv --n 2000000 --d 64 --out out/svm_subset_cv.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import permon_amd as pa  # noqa: E402
from permon_amd import problems as P  # noqa: E402
from permon_amd._lib import check  # noqa: E402


class Fixed:
    """MPGP on H_S (rhs = m, 0 <= a <= C) that runs exactly k iterations from the zero iterate."""

    def __init__(self, ctx, p, mask, shift=0.0, diag=None, unbounded=False):
        n = p["n"]
        self.ctx, self.H = ctx, pa.MatCreateSVMDual(ctx, p["X"], p["y"])
        if mask is not None:
            self.H.set_subset(mask)
        if shift:
            self.H.set_terms(shift, 0.0)  # (the AUG = 1 kernel instances)
        if diag is not None:
            self.H.set_diag(diag)  # (AUG = 2)
        qp = pa.QP(ctx)
        qp.SetOperator(self.H)
        qp.SetRhs(ctx.vec_from(np.ones(n) if mask is None else mask.astype(float)))
        self.x = ctx.vec_from(np.zeros(n))
        qp.SetInitialVector(self.x)
        # (unbounded: bounds nothing reaches, so MPGP takes CG steps alone: pass 1 and k_svm_x64_p1<0, ...>, which the expansion steps of the box hardly run)
        qp.SetBox(None, ctx.vec_from(np.full(n, -1e300 if unbounded else 0.0)), ctx.vec_from(np.full(n, 1e300 if unbounded else float(p["C"]))))
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
        return dict(ms_per_iteration=1e3 * dt / max(st.iteration, 1), iterations=st.iteration, hessian_mults=st.nmv, cg=st.ncg, expansion=st.nexp, proportioning=st.nprop,
                    passes_over_X=self.H.passes() - p0, ms_per_pass=1e3 * dt / max(self.H.passes() - p0, 1), ms_per_product=1e3 * dt / max(st.nmv, 1))


def summary(v, key):
    x = [r[key] for r in v]
    med = float(np.median(x))
    return {key + "_median": med, key + "_min": min(x), key + "_max": max(x), key + "_spread_rel": (max(x) - min(x)) / med}


def product(a, ctx, p, res):
    n = p["n"]
    rng = np.random.default_rng(5)
    masks = dict(none=None, random=rng.random(n) < a.share, contiguous=np.arange(n) < int(a.share * n))
    diag = ctx.vec_from(rng.uniform(0.5, 2.0, n)) if a.diag else None  # (one device vector, shared by the variants)
    solvers = {k: Fixed(ctx, p, masks[k], a.shift, diag, a.unbounded) for k in a.variants.split(",")}
    for s in solvers.values():
        s.run(a.warmup)
    runs = {k: [] for k in solvers}
    for _ in range(a.rounds):  # alternated: a drift of the box hits every variant alike
        for k, s in solvers.items():
            runs[k].append(s.run(a.steps))
    for k, v in runs.items():
        res[k] = dict(share=1.0 if masks[k] is None else float(masks[k].mean()), **summary(v, "ms_per_pass"), **summary(v, "ms_per_product"), **summary(v, "ms_per_iteration"), runs=v)
    for k in runs:
        if k != "none" and "none" in runs:
            res[k + "_over_none_per_pass"] = res[k]["ms_per_pass_median"] / res["none"]["ms_per_pass_median"]


def cv(a, ctx, p, res):
    from permon_amd.svm import cross_validate, kfold

    X, y = p["X"], p["y"]
    sparse = hasattr(X, "tocsr")
    masks = kfold(y, a.k, seed=0)
    opts = "-qps_rtol %g" % a.rtol
    one, fresh, acc = [], [], {}
    for _ in range(a.rounds):
        ctx.sync()
        t0 = time.perf_counter()
        svm = pa.SVM(ctx, loss="L1", C=p["C"], bias=True, options=opts).create(X, y)
        t1 = time.perf_counter()
        r = cross_validate(svm, k=a.k, seed=0)
        ctx.sync()
        t2 = time.perf_counter()
        svm.destroy()
        one.append(dict(s_create=t1 - t0, s_folds=t2 - t1, s_total=t2 - t0))
        acc["one_handle"] = [f["accuracy"] for f in r["folds"]]
        t0 = time.perf_counter()
        accs, t_slice = [], 0.0
        for m in masks:
            ts = time.perf_counter()
            Xm, ym, Xh, yh = (X[np.flatnonzero(m)] if sparse else X[m]), y[m], (X[np.flatnonzero(~m)] if sparse else X[~m]), y[~m]
            t_slice += time.perf_counter() - ts  # (the host's row selection: reported, and left in the total: a caller pays it)
            s = pa.SVM(ctx, loss="L1", C=p["C"], bias=True, options=opts).fit(Xm, ym)
            accs.append(s.test(Xh, yh)["accuracy"])
            s.destroy()
        ctx.sync()
        t3 = time.perf_counter()
        fresh.append(dict(s_total=t3 - t0, s_host_row_selection=t_slice))
        acc["fresh_handles"] = accs
    res["one_handle"] = dict(**summary(one, "s_total"), **summary(one, "s_create"), **summary(one, "s_folds"), runs=one)
    res["fresh_handles"] = dict(**summary(fresh, "s_total"), **summary(fresh, "s_host_row_selection"), runs=fresh)
    res["fold_accuracy"] = acc
    res["fresh_over_one"] = res["fresh_handles"]["s_total_median"] / res["one_handle"]["s_total_median"]
    res["fresh_over_one_without_host_selection"] = (res["fresh_handles"]["s_total_median"] - res["fresh_handles"]["s_host_row_selection_median"]) / res["one_handle"]["s_total_median"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["product", "cv"], default="product")
    ap.add_argument("--n", type=int, default=5000000)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--csr", type=int, nargs=2, default=None, metavar=("N_FEATURES", "NNZ_ROW"))
    ap.add_argument("--share", type=float, default=0.8)
    ap.add_argument("--variants", default="none,random,contiguous")
    ap.add_argument("--shift", type=float, default=0.0, help="product: H + shift I (the operator's scalar-shift kernels); excludes --diag")
    ap.add_argument("--unbounded", action="store_true", help="product: bounds of +-1e300 in place of 0 <= a <= C: CG steps only (use with --shift or --diag: H alone is singular)")
    ap.add_argument("--diag", action="store_true", help="product: H + diag(D), D uniform in [0.5, 2) (the operator's diagonal kernels)")
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--rtol", type=float, default=1e-3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out", default="out/svm_subset_cost.json")
    a = ap.parse_args()
    ctx = pa.Context(0)
    p = P.svm_sparse(a.n, a.csr[0], a.csr[1], 1.0, 0.5, 1.0) if a.csr else P.svm_offset(a.n, a.d, 3.0)
    res = dict(device=ctx.name(), what=a.what, shift=a.shift, diag=bool(a.diag), unbounded=bool(a.unbounded), n=p["n"], d=a.csr[0] if a.csr else a.d, csr=bool(a.csr), nnz=int(p["X"].nnz) if a.csr else None, steps=a.steps, warmup=a.warmup, rounds=a.rounds)
    (product if a.what == "product" else cv)(a, ctx, p, res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({k: (v if not isinstance(v, dict) else {kk: vv for kk, vv in v.items() if kk != "runs"}) for k, v in res.items()}))
    ctx.close()


if __name__ == "__main__":
    main()
