"""One application of the SVM dual operator on sparse samples (csrc/svm_csr.hip) against the same product composed from the CSR kernels the library had before
it (docs/LAB_NOTEBOOK.md, "SVM on sparse samples"): one process, one GPU.

  (a) H a through pmh_op_create_svm_dual_csr (two entry-balanced sweeps);
  (b) Xy (Xy' a) with Xy = diag(y) X through pmh_csr_mult_transpose and pmh_csr_mult.  The library exports no elementwise product, so y is folded into the
      matrix: (b) is spared the two vector kernels for y o a and y o (.) it would otherwise need.

Two instances of problems.svm_sparse: feature popularity ~ 1 / rank^skew (skew 1.0) and uniform (skew 0).  The results of (a) and (b) are compared first, entry by
entry, within the rounding bound of tests/test_gpu_svm_sparse.py.  Then both are warmed up and timed with device events, alternating, `--reps` windows of `--inner`
applications each; the spread is (max - min) / median over the windows.  (a) is also given as a share of the HBM peak on its algorithmic bytes.

    python scripts/dev/svm_sparse_speed.py --n 2000000 --d 50000 --nnz-row 60 --out out/svm_sparse_speed.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import permon_amd as pa  # noqa: E402
from permon_amd import problems as P  # noqa: E402
from permon_amd.mat import csr_from_scipy  # noqa: E402

EPS = np.finfo(float).eps
HBM_PEAK_GBS = 8000.0  # MI355X: 8 TB/s HBM3E (specification)


def algorithmic_bytes(nnz, n, d):
    """Both copies' values and indices, the two pointer arrays, a, y and H a, w written and read."""
    return 24.0 * nnz + 4.0 * (n + d) + 8.0 * (3.0 * n + 2.0 * d)


def gamma(k):
    return k * EPS / (1.0 - k * EPS)


def window(ctx, fn, inner):
    ctx.sync()
    ctx.timer_start()
    for _ in range(inner):
        fn()
    return ctx.timer_stop() / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2000000)
    ap.add_argument("--d", type=int, default=50000)
    ap.add_argument("--nnz-row", type=int, default=60)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--only", default="", help="skewed | uniform: one instance only (a profiler run)")
    ap.add_argument("--out", default="out/svm_sparse_speed.json")
    a = ap.parse_args()
    assert a.reps >= 5
    ctx = pa.Context(0)
    res = dict(device=ctx.name(), n=a.n, d=a.d, nnz_row=a.nnz_row, reps=a.reps, inner=a.inner, hbm_peak_GBs=HBM_PEAK_GBS, instances={})
    for name, skew in (("skewed", 1.0), ("uniform", 0.0)):
        if a.only and a.only != name:
            continue
        t0 = time.perf_counter()
        p = P.svm_sparse(a.n, a.d, a.nnz_row, skew, 0.5)
        X, y, n, d = p["X"], p["y"], p["n"], p["d"]
        cc, rc = np.bincount(X.indices, minlength=d), np.diff(X.indptr)
        print(name, "generated in %.1f s: nnz %d, column counts max / median / empty %d / %d / %d, row counts max %d" % (time.perf_counter() - t0, X.nnz, cc.max(), np.median(cc), (cc == 0).sum(), rc.max()), flush=True)
        t0 = time.perf_counter()
        H = pa.MatCreateSVMDual(ctx, X, y)
        ctx.sync()
        t_create = time.perf_counter() - t0
        Xy = csr_from_scipy(ctx, sp.diags(y) @ X)
        v = np.random.default_rng(1).uniform(0, 1, n)
        vd, oa, ob, t = ctx.vec_from(v), ctx.vec(n), ctx.vec(n), ctx.vec(d)

        def fa():
            H.mult(vd, oa)

        def fb():
            Xy.mult_transpose(vd, t)
            Xy.mult(t, ob)

        fa(), fb()
        ctx.sync()
        # the two results against each other: each within the bound once (its own rounding), so their difference within the bound with its factor 2
        Xa = abs(X)
        ra, rb = oa.to_numpy(), ob.to_numpy()
        bound = 2 * (gamma(int(cc.max()) + int(rc.max()) + 2) * (Xa @ (Xa.T @ np.abs(v))) + 4 * EPS * np.abs(ra))
        ratio = float((np.abs(ra - rb) / np.maximum(bound, 1e-300)).max())
        print(name, "(a) against (b): max |difference| / bound = %.3f" % ratio, flush=True)
        assert ratio <= 1.0, "the two products disagree beyond rounding"
        for _ in range(3):
            window(ctx, fa, 2), window(ctx, fb, 2)
        ta, tb = [], []
        for _ in range(a.reps):  # alternated: a drift of the machine hits both alike
            ta.append(window(ctx, fa, a.inner))
            tb.append(window(ctx, fb, a.inner))
        nb = algorithmic_bytes(X.nnz, n, d)
        ma, mb = float(np.median(ta)), float(np.median(tb))
        r = dict(nnz=int(X.nnz), col_max=int(cc.max()), col_median=float(np.median(cc)), col_empty=int((cc == 0).sum()), row_max=int(rc.max()), create_seconds=t_create,
                 agreement_over_bound=ratio, a_ms=ta, b_ms=tb, a_ms_median=ma, b_ms_median=mb, a_spread_rel=(max(ta) - min(ta)) / ma, b_spread_rel=(max(tb) - min(tb)) / mb,
                 algorithmic_bytes=nb, a_GBs=nb / ma / 1e6, a_share_of_hbm_peak=nb / ma / 1e6 / HBM_PEAK_GBS, bound="HBM bandwidth", b_plans=(Xy.kernel_info()[0][0],))
        res["instances"][name] = r
        print(name, json.dumps({k: v for k, v in r.items() if k not in ("a_ms", "b_ms")}), flush=True)
        for o in (vd, oa, ob, t):
            o.free()
        H.destroy(), Xy.destroy()
        for k in H._keep:
            k.destroy() if hasattr(k, "destroy") else k.free()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
