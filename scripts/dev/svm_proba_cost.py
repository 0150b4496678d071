"""What a probability costs beside a score (docs/LAB_NOTEBOOK.md, "SVM probabilities"): one process, one GPU, one step per call.

  dense64, dense130, csr   pmh_svm_predict_proba / _csr against pmh_svm_predict / _csr (scores only) of the same handle: 2 M x 64, 2 M x 130 and the CSR
                           instance 2 M x 50 000 x 60 (problems.svm_sparse, skew 1.0).  The time of a sweep does not depend on the values of w, so a handle
                           trained on a few samples of the same width stands for the model.
  multi                    pmh_svm_multi_predict_proba against pmh_svm_multi_predict (scores only) at K = 4 and K = 10 on 2 M x 64 (set_model, set_calibration).
  fit                      one pmh_svm_platt_fit of 5 M overlapping scores (scores resident): time, iterations, evaluations.

Test samples stay on the device; device events; after a warm-up, `--reps` alternating rounds of `--inner` calls each; medians, spread = (max - min) / median,
ratio = proba median / score median, inside_spread = the two samples' ranges overlap.  Every step is a process of its own under its own time limit:

    timeout -k 10 240 python scripts/dev/svm_proba_cost.py --what dense64 --out out/proba_dense64.json && \\
    timeout -k 10 240 python scripts/dev/svm_proba_cost.py --what dense130 --out out/proba_dense130.json && \\
    timeout -k 10 420 python scripts/dev/svm_proba_cost.py --what csr --out out/proba_csr.json && \\
    timeout -k 10 240 python scripts/dev/svm_proba_cost.py --what multi --out out/proba_multi.json && \\
    timeout -k 10 120 python scripts/dev/svm_proba_cost.py --what fit --out out/proba_fit.json
"""
import argparse
import ctypes as ct
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import permon_amd as pa  # noqa: E402
from permon_amd import _lib, problems as P  # noqa: E402
from permon_amd._lib import check  # noqa: E402
from permon_amd.mat import csr_from_scipy  # noqa: E402

OPT = "-qps_rtol 1e-6"


def window(ctx, fn, inner):
    ctx.sync()
    ctx.timer_start()
    for _ in range(inner):
        fn()
    return ctx.timer_stop() / inner


def alternate(ctx, fa, fb, reps, inner):
    for _ in range(2):
        window(ctx, fa, 1), window(ctx, fb, 1)
    ta, tb = [], []
    for _ in range(reps):
        ta.append(window(ctx, fa, inner))
        tb.append(window(ctx, fb, inner))
    return ta, tb


def summary(tp, ts, nbytes):
    mp, ms = float(np.median(tp)), float(np.median(ts))
    return dict(proba_ms=tp, score_ms=ts, proba_ms_median=mp, score_ms_median=ms, proba_spread_rel=(max(tp) - min(tp)) / mp, score_spread_rel=(max(ts) - min(ts)) / ms,
                ratio=mp / ms, inside_spread=bool(min(tp) <= max(ts) and min(ts) <= max(tp)), algorithmic_bytes=nbytes, proba_TBs=nbytes / mp / 1e9, score_TBs=nbytes / ms / 1e9)


def small_model(ctx, d, sparse):
    import scipy.sparse as sp

    X0 = sp.random(64, d, density=min(1.0, 20.0 / d), format="csr", random_state=1) if sparse else np.random.default_rng(3).standard_normal((64, d))
    return X0, np.where(np.arange(64) % 2 == 0, 1.0, -1.0)


def binary_case(ctx, X, reps, inner):
    L, sparse = ctx.L, hasattr(X, "tocsr")
    n, d = X.shape
    Xd = csr_from_scipy(ctx, X) if sparse else ctx.vec_from(X.ravel())
    s = pa.SVM(ctx, options=OPT).fit(*small_model(ctx, d, sparse)).set_calibration(-0.8, 0.1)
    out = ctx.vec(n)
    if sparse:
        fp = lambda: check(L.pmh_svm_predict_proba_csr(s.h, Xd.h, out.p))  # noqa: E731
        fs = lambda: check(L.pmh_svm_predict_csr(s.h, Xd.h, out.p, None))  # noqa: E731
        nbytes = 12.0 * X.nnz + 4.0 * n + 24.0 * n  # the sweep, then the n dot products read and written in place
    else:
        fp = lambda: check(L.pmh_svm_predict_proba(s.h, n, Xd.p, out.p))  # noqa: E731
        fs = lambda: check(L.pmh_svm_predict(s.h, n, Xd.p, out.p, None))  # noqa: E731
        nbytes = 8.0 * n * d + 8.0 * n
    r = summary(*alternate(ctx, fp, fs, reps, inner), nbytes)
    r.update(n=n, d=d)
    out.free(), s.destroy()
    Xd.destroy() if sparse else Xd.free()
    return r


def multi_case(ctx, X, K, reps, inner):
    L = ctx.L
    n, d = X.shape
    rng = np.random.default_rng(K)
    Xd = ctx.vec_from(X.ravel())
    X0, _ = small_model(ctx, d, False)
    m = pa.SVMMulticlass(ctx, options=OPT).create(X0, np.arange(64.0) % K)
    m.set_model(rng.standard_normal((K, d)), rng.standard_normal(K)).set_calibration(-0.5 - rng.random(K), 0.1 * rng.standard_normal(K))
    out = ctx.vec(n * K)
    fp = lambda: check(L.pmh_svm_multi_predict_proba(m.h, n, Xd.p, out.p))  # noqa: E731
    fs = lambda: check(L.pmh_svm_multi_predict(m.h, n, Xd.p, out.p, None))  # noqa: E731
    nch = -(-K // m.chunk("dense64" if d == 64 else "dense"))
    r = summary(*alternate(ctx, fp, fs, reps, inner), 8.0 * n * d * nch + 8.0 * n * K)
    r.update(n=n, d=d, K=K, passes=nch, normalise_bytes=16.0 * n * K)
    out.free(), Xd.free(), m.destroy()
    return r


def fit_case(ctx, n, reps):
    rng = np.random.default_rng(0)
    y = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    f, yv = ctx.vec_from(y + 1.5 * rng.standard_normal(n)), ctx.vec_from(y)
    A, B, st = ct.c_double(), ct.c_double(), _lib.SvmPlattStats()
    fit = lambda: check(ctx.L.pmh_svm_platt_fit(ctx.h, n, f.p, yv.p, ct.byref(A), ct.byref(B), ct.byref(st)))  # noqa: E731
    window(ctx, fit, 1)
    t = [window(ctx, fit, 1) for _ in range(reps)]
    md = float(np.median(t))
    r = dict(n=n, fit_ms=t, fit_ms_median=md, fit_spread_rel=(max(t) - min(t)) / md, A=A.value, B=B.value, reason=st.reason, iterations=st.iterations, evaluations=st.evaluations,
             ms_per_evaluation=md / st.evaluations, evaluation_bytes=16.0 * n, fval=st.fval, g1=st.g1, g2=st.g2, n_pos=st.n_pos, n_neg=st.n_neg)
    f.free(), yv.free()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", required=True, choices=["dense64", "dense130", "csr", "multi", "fit"])
    ap.add_argument("--n", type=int, default=2000000)
    ap.add_argument("--n-fit", type=int, default=5000000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default="out/svm_proba_cost.json")
    a = ap.parse_args()
    assert a.reps >= 5
    ctx = pa.Context(0)
    res = dict(device=ctx.name(), what=a.what, reps=a.reps, inner=a.inner)
    if a.what in ("dense64", "dense130"):
        d = int(a.what[5:])
        res["case"] = binary_case(ctx, np.random.default_rng(d).standard_normal((a.n, d)), a.reps, a.inner)
    elif a.what == "csr":
        res["case"] = binary_case(ctx, P.svm_sparse(a.n, 50000, 60, 1.0, 0.5)["X"], a.reps, a.inner)
    elif a.what == "multi":
        X = np.random.default_rng(64).standard_normal((a.n, 64))
        res["case"] = {K: multi_case(ctx, X, K, a.reps, a.inner) for K in (4, 10)}
    else:
        res["case"] = fit_case(ctx, a.n_fit, a.reps)
    ctx.close()
    print(json.dumps({k: v for k, v in res.items()}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
