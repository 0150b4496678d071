"""What the SVM's bias term costs in time (docs/LAB_NOTEBOOK.md, "SVM front end"): one process, one GPU.

  (a) ms per inner MPGP iteration of the biased L1 solve (SMALXE's inner solver on the penalised operator that folds the one-row equality into the SVM operator,
      ||B u|| evaluated every iteration) against the unbiased one (MPGP on the SVM operator), alternated `--rounds` times; the spread of the repeated unbiased
      runs is what a difference has to exceed;
  (b) the same biased step posed the way the library could before the one-row projector: the row as a 1 x n CSR through pmh_qppf_create and the generic branch
      of the penalised operator;
  (c) the one-row Q v and the prediction pass against the device copy rate measured in the same process (algorithmic bytes 24 n and 8 n d + 16 n).

Every window is `--steps` iterations from the zero iterate after `--warmup` iterations, timed by a host clock around work that ends in a device synchronise.
The step sequences of the biased and the unbiased problem differ, so the passes over X of each window are reported with the time.

    python scripts/dev/svm_bias_cost.py --n 5000000 --d 64 --steps 100 --warmup 10 --rounds 4 --out out/svm_bias_cost.json
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import permon_amd as pa  # noqa: E402
from permon_amd import problems as P  # noqa: E402
from permon_amd._lib import check  # noqa: E402


class Fixed:
    """A solver that runs exactly k inner MPGP iterations from the zero iterate."""

    def __init__(self, ctx, p, pf):
        self.ctx, self.H = ctx, pa.MatCreateSVMDual(ctx, p["X"], p["y"])
        qp = pa.QP(ctx)
        qp.SetOperator(self.H)
        qp.SetRhs(ctx.vec_from(p["b"]))
        self.x = ctx.vec_from(p["x0"])
        qp.SetInitialVector(self.x)
        qp.SetBox(None, ctx.vec_from(p["lb"]), ctx.vec_from(p["ub"]))
        self.qps = pa.QPS(ctx)
        if pf is not None:
            qp.SetEq(pf)
        self.qps.SetQP(qp)
        self.qps.SetType("smalxe" if pf is not None else "mpgp")
        self.smalxe = pf is not None
        self.qps.SetUp()

    def run(self, k):
        self.x.set(0.0)
        if self.smalxe:  # the injected convergence test ends the run by ITS iteration limit
            check(self.ctx.L.pmh_smalxe_set_inner_max_it(self.qps.h, k))
        check(self.ctx.L.pmh_mpgp_reset_statistics(self.qps._mpgp_handle()))
        self.ctx.sync()
        p0, t0 = self.H.passes(), time.perf_counter()
        st = self.qps.RunFixed(k)
        self.ctx.sync()
        dt = time.perf_counter() - t0
        return dict(ms_per_iteration=1e3 * dt / max(st.iteration, 1), iterations=st.iteration, hessian_mults=st.nmv, cg=st.ncg, expansion=st.nexp, proportioning=st.nprop,
                    passes_over_X=self.H.passes() - p0, ms_per_pass=1e3 * dt / max(self.H.passes() - p0, 1))


def copy_rate(ctx, n=1 << 26, reps=10):
    x, w = ctx.vec(n), ctx.vec(n)
    x.set(1.0)
    for _ in range(2):
        ctx.L.pmh_vec_copy(ctx.h, n, x.p, w.p)
    ctx.sync()
    ctx.timer_start()
    for _ in range(reps):
        ctx.L.pmh_vec_copy(ctx.h, n, x.p, w.p)
    ms = ctx.timer_stop() / reps
    x.free(), w.free()
    return 16.0 * n / ms / 1e6


def timed(ctx, fn, reps):
    for _ in range(2):
        fn()
    ctx.sync()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return ctx.timer_stop() / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5000000)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out", default="out/svm_bias_cost.json")
    a = ap.parse_args()
    ctx = pa.Context(0)
    p = P.svm_offset(a.n, a.d, 3.0)
    n, y = p["n"], p["y"]
    row = y / np.sqrt(n)
    res = dict(device=ctx.name(), n=n, d=a.d, steps=a.steps, warmup=a.warmup, rounds=a.rounds, copy_GBs=copy_rate(ctx))
    solvers = {"unbiased": Fixed(ctx, p, None), "biased_folded": Fixed(ctx, p, pa.QPPF.onerow(ctx, row))}
    try:
        solvers["biased_csr_row_generic"] = Fixed(ctx, p, pa.QPPF.from_scipy(ctx, sp.csr_matrix(row[None, :]), orthonormal=True))
    except Exception as ex:  # reported, not hidden
        res["biased_csr_row_generic"] = "set-up failed: %r" % (ex,)
    for s in solvers.values():
        s.run(a.warmup)
    runs = {k: [] for k in solvers}
    for _ in range(a.rounds):  # alternated: a drift of the box hits every variant alike
        for k, s in solvers.items():
            runs[k].append(s.run(a.steps))
    for k, v in runs.items():
        ms = [r["ms_per_iteration"] for r in v]
        res[k] = dict(ms_per_iteration_median=float(np.median(ms)), ms_per_iteration_min=min(ms), ms_per_iteration_max=max(ms), ms_per_pass_median=float(np.median([r["ms_per_pass"] for r in v])), runs=v)
    u = res["unbiased"]
    res["unbiased_spread_rel"] = (u["ms_per_iteration_max"] - u["ms_per_iteration_min"]) / u["ms_per_iteration_median"]
    # (c) the one-row Q v and the prediction pass
    pf = pa.QPPF.onerow(ctx, row)
    v, q = ctx.vec_from(np.random.default_rng(1).standard_normal(n)), ctx.vec(n)
    ms = timed(ctx, lambda: pf.ApplyQ(v, q), 20)
    res["onerow_Qv"] = dict(ms=ms, algorithmic_bytes=24.0 * n, GBs=24.0 * n / ms / 1e6, frac_of_copy=24.0 * n / ms / 1e6 / res["copy_GBs"], traffic_bytes_if_row_read_twice=32.0 * n)
    svm = pa.SVM(ctx, loss="L1", C=1.0, bias=False, options="-qps_max_it 5").fit(p["X"], y)  # a model, not a converged one: the pass does the same work
    Xd, yd = svm._keep
    sc, lab = ctx.vec(n), ctx.vec(n)
    ms = timed(ctx, lambda: check(ctx.L.pmh_svm_predict(svm.h, n, Xd.p, sc.p, lab.p)), 10)
    nb = 8.0 * n * a.d + 16.0 * n
    res["predict"] = dict(ms=ms, algorithmic_bytes=nb, GBs=nb / ms / 1e6, frac_of_copy=nb / ms / 1e6 / res["copy_GBs"])
    cnt = (ctypes.c_longlong * 4)()
    ms = timed(ctx, lambda: check(ctx.L.pmh_svm_test(svm.h, n, Xd.p, yd.p, cnt)), 10)
    nb = 8.0 * n * a.d + 8.0 * n
    res["test_counts"] = dict(ms=ms, algorithmic_bytes=nb, GBs=nb / ms / 1e6, frac_of_copy=nb / ms / 1e6 / res["copy_GBs"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    brief = {k: (v if not isinstance(v, dict) else {kk: vv for kk, vv in v.items() if kk != "runs"}) for k, v in res.items()}
    print(json.dumps(brief))
    ctx.close()


if __name__ == "__main__":
    main()
