"""What the diagonal of the SVM dual operator costs in time (docs/LAB_NOTEBOOK.md, "SVM penalties"): one process, one GPU.

L2-loss dual without bias, MPGP on H + I/C posed twice: with the scalar shift 1/C (pmh_op_svm_dual_set_terms) and with a diagonal that holds 1/C in every entry
(pmh_op_svm_dual_set_diag).  The two are the same expression on the same numbers, so both take the same steps and stream X equally often; the diagonal reads 8
bytes more per sample in every pass 2.  Windows of `--steps` fixed iterations from the zero iterate after `--warmup` iterations, the variants alternated
`--rounds` times, timed by a host clock around work that ends in a device synchronise.

    python scripts/dev/svm_diag_cost.py --n 5000000 --d 64 --steps 100 --warmup 10 --rounds 4 --out out/svm_diag_cost.json
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
    """MPGP on H + shift I or H + diag(diag) that runs exactly k iterations from the zero iterate."""

    def __init__(self, ctx, p, shift, diag):
        self.ctx, self.H = ctx, pa.MatCreateSVMDual(ctx, p["X"], p["y"])
        if diag is not None:
            self.H.set_diag(diag)
        else:
            self.H.set_terms(shift, 0.0)
        qp = pa.QP(ctx)
        qp.SetOperator(self.H)
        qp.SetRhs(ctx.vec_from(p["b"]))
        self.x = ctx.vec_from(p["x0"])
        qp.SetInitialVector(self.x)
        qp.SetBox(None, ctx.vec_from(p["lb"]), None)
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
                    passes_over_X=self.H.passes() - p0, ms_per_pass=1e3 * dt / max(self.H.passes() - p0, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5000000)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--C", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out", default="out/svm_diag_cost.json")
    a = ap.parse_args()
    ctx = pa.Context(0)
    p = P.svm_offset(a.n, a.d, 3.0)
    n = p["n"]
    res = dict(device=ctx.name(), n=n, d=a.d, C=a.C, steps=a.steps, warmup=a.warmup, rounds=a.rounds)
    solvers = {"scalar_shift": Fixed(ctx, p, 1.0 / a.C, None), "diagonal": Fixed(ctx, p, 0.0, np.full(n, 1.0 / a.C))}
    for s in solvers.values():
        s.run(a.warmup)
    runs = {k: [] for k in solvers}
    for _ in range(a.rounds):  # alternated: a drift of the box hits both variants alike
        for k, s in solvers.items():
            runs[k].append(s.run(a.steps))
    for k, v in runs.items():
        ms = [r["ms_per_iteration"] for r in v]
        res[k] = dict(ms_per_iteration_median=float(np.median(ms)), ms_per_iteration_min=min(ms), ms_per_iteration_max=max(ms),
                      spread_rel=(max(ms) - min(ms)) / float(np.median(ms)), ms_per_pass_median=float(np.median([r["ms_per_pass"] for r in v])), runs=v)
    res["same_iterates"] = bool(np.array_equal(solvers["scalar_shift"].x.to_numpy(), solvers["diagonal"].x.to_numpy()))
    res["diagonal_over_scalar"] = res["diagonal"]["ms_per_iteration_median"] / res["scalar_shift"]["ms_per_iteration_median"]
    res["expected_share_of_bytes"] = 8.0 / (8.0 * a.d + 40.0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({k: (v if not isinstance(v, dict) else {kk: vv for kk, vv in v.items() if kk != "runs"}) for k, v in res.items()}))
    ctx.close()


if __name__ == "__main__":
    main()
