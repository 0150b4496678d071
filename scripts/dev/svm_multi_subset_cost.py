"""What the subset and own-row entries of SVMMulticlass save in time (docs/LAB_NOTEBOOK.md, "SVM multiclass subsets"): one process, one GPU.

--what score: on a handle with a set model (no training), test_own("held_out") on a selection of `--share` of the rows, against test_own("all"), against
test(X, labels) with its upload (the only route without the own-row entries), alternated `--rounds` times after one warm-up call each; host clock around
calls that end in a device synchronise.  The byte counts beside the times are those of the header of csrc/svm_multi.hip, with the selector's 8 n and the
confusion kernel's 16 n; the device's copy rate is measured in the same process (pmh_vec_copy of 2^28 bytes, 16 bytes of traffic per entry).

--what cv: k-fold cross_validate on one SVMMulticlass handle (X uploaded once, CSR: one column-ordered copy) against k fresh SVMMulticlass handles on X[mask]
that score X[~mask] (uploads and copies included), wall time, alternated `--rounds` times; the fold accuracies of both are reported side by side.
`--progress` prints a line per fold (the one-handle loop is then cross_validate's, written out): K trainings per fold at this size take minutes.

Dense rows: problems.svm_blobs(n, d, K); CSR: the samples of problems.svm_sparse(n, N_FEATURES, NNZ_ROW) labelled by the greatest of K random planes.

    python scripts/dev/svm_multi_subset_cost.py --what score --n 2000000 --d 64 --K 10 --out out/svm_multi_subset_score.json
    python scripts/dev/svm_multi_subset_cost.py --what score --n 2000000 --csr 50000 60 --K 10 --out out/svm_multi_subset_score_csr.json
    python scripts/dev/svm_multi_subset_cost.py --what cv --n 2000000 --d 64 --K 10 --out out/svm_multi_subset_cv.json
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
from permon_amd.svm import cross_validate, kfold  # noqa: E402


def problem(a):
    if a.csr:
        X = P.svm_sparse(a.n, a.csr[0], a.csr[1], 1.0, 0.5, 1.0)["X"].tocsr()
        planes = np.random.default_rng(3).standard_normal((a.K, a.csr[0]))
        return X, np.argmax(np.asarray(X @ planes.T), axis=1).astype(np.float64)
    p = P.svm_blobs(a.n, a.d, a.K, 4.0, 5)
    return p["X"], p["labels"]


def summary(v, key):
    x = [r[key] for r in v]
    med = float(np.median(x))
    return {key + "_median": med, key + "_min": min(x), key + "_max": max(x), key + "_spread_rel": (max(x) - min(x)) / med}


def copy_rate(ctx):
    """GB/s of a device-to-device copy, the median of 20 after 3 warm-up copies."""
    m = 1 << 25
    x, y = ctx.vec_from(np.zeros(m)), ctx.vec(m)
    t = []
    for it in range(23):
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(10):
            check(ctx.L.pmh_vec_copy(ctx.h, m, x.p, y.p))
        ctx.sync()
        if it >= 3:
            t.append((time.perf_counter() - t0) / 10)
    x.free(), y.free()
    return 16.0 * m / float(np.median(t)) / 1e9


def timed(ctx, f):
    ctx.sync()
    t0 = time.perf_counter()
    r = f()
    ctx.sync()
    return time.perf_counter() - t0, r


def rows(X, m):
    return X[np.flatnonzero(m)] if hasattr(X, "tocsr") else X[m]


def score(a, ctx, X, lab, res):
    n, d = X.shape
    sparse = hasattr(X, "tocsr")
    K = int(np.unique(lab).size)
    mask = np.random.default_rng(5).random(n) >= a.share  # the subset; the held-out rows are `share` of all
    m = pa.SVMMulticlass(ctx, options="-qps_rtol %g" % a.rtol).create(X, lab).set_subset(mask)
    rng = np.random.default_rng(6)
    m.set_model(rng.standard_normal((K, d)), rng.standard_normal(K))
    kc = pa.SVMMulticlass.chunk("csr" if sparse else ("dense64" if d == 64 else "dense"))
    nch = -(-K // kc)
    sweep = (12.0 * X.nnz + 4.0 * n) if sparse else 8.0 * n * d  # one chunk's read of the samples
    held = float((~mask).mean())
    variants = dict(held_out=lambda: m.test_own("held_out"), all=lambda: m.test_own("all"), upload=lambda: m.test(X, lab))
    # per scored row: the label written per chunk and, K > chunk, best written per chunk and read by every chunk after the first; the confusion kernel reads
    # label and prediction of a counted row; the selector (8 n) is read by every dense sweep and by the confusion kernel
    written = lambda r: 8.0 * r * nch + (8.0 * r * (2 * nch - 1) if nch > 1 else 0.0)
    scored = n if sparse else n * held
    res["bytes"] = dict(held_out=sweep * nch * (1.0 if sparse else held) + written(scored) + (0.0 if sparse else 8.0 * n * nch) + 8.0 * n + 16.0 * n * held, all=sweep * nch + written(n) + 16.0 * n)
    for f in variants.values():
        f()
    runs = {k: [] for k in variants}
    out = {}
    for _ in range(a.rounds):
        for k, f in variants.items():
            dt, out[k] = timed(ctx, f)
            runs[k].append(dict(ms=1e3 * dt))
    for k, v in runs.items():
        res[k] = dict(**summary(v, "ms"), accuracy=out[k]["accuracy"], runs=v)
    assert np.array_equal(out["all"]["confusion"], out["upload"]["confusion"])
    for k in ("held_out", "all"):
        res[k]["GBs_on_algorithmic_bytes"] = res["bytes"][k] / (1e-3 * res[k]["ms_median"]) / 1e9
    res["held_out_over_all"] = res["held_out"]["ms_median"] / res["all"]["ms_median"]
    res["upload_over_all"] = res["upload"]["ms_median"] / res["all"]["ms_median"]
    res["held_out_share"] = held
    m.destroy()


def cv(a, ctx, X, lab, res):
    masks = kfold(lab, a.k, seed=0)
    opts = "-qps_rtol %g" % a.rtol
    one, fresh, acc = [], [], {}
    for _ in range(a.rounds):
        ctx.sync()
        t0 = time.perf_counter()
        m = pa.SVMMulticlass(ctx, "L1", 1.0, True, opts).create(X, lab)
        t1 = time.perf_counter()
        if a.progress:  # cross_validate's loop written out, a line per fold (a long run that prints nothing looks hung)
            folds = []
            for mk in masks:
                folds.append(m.set_subset(mk).train().test_own("held_out"))
                print("one handle: fold %d done after %.1f s" % (len(folds), time.perf_counter() - t1), flush=True)
            m.set_subset(None)
        else:
            folds = cross_validate(m, k=a.k, seed=0)["folds"]
        ctx.sync()
        t2 = time.perf_counter()
        m.destroy()
        one.append(dict(s_create=t1 - t0, s_folds=t2 - t1, s_total=t2 - t0))
        acc["one_handle"] = [f["accuracy"] for f in folds]
        t0 = time.perf_counter()
        accs, t_slice = [], 0.0
        for mk in masks:
            ts = time.perf_counter()
            Xm, lm, Xh, lh = rows(X, mk), lab[mk], rows(X, ~mk), lab[~mk]
            t_slice += time.perf_counter() - ts  # (the host's row selection: reported, and left in the total: a caller pays it)
            s = pa.SVMMulticlass(ctx, "L1", 1.0, True, opts).fit(Xm, lm)
            accs.append(s.test(Xh, lh)["accuracy"])
            s.destroy()
            if a.progress:
                print("fresh handles: fold %d done after %.1f s" % (len(accs), time.perf_counter() - t0), flush=True)
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
    ap.add_argument("--what", choices=["score", "cv"], default="score")
    ap.add_argument("--n", type=int, default=2000000)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--K", type=int, default=10)
    ap.add_argument("--csr", type=int, nargs=2, default=None, metavar=("N_FEATURES", "NNZ_ROW"))
    ap.add_argument("--share", type=float, default=0.2, help="score: the share of the rows that is held out")
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--rtol", type=float, default=1e-3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--progress", action="store_true", help="cv: a line per fold; the one-handle loop is then cross_validate's written out")
    ap.add_argument("--out", default="out/svm_multi_subset_cost.json")
    a = ap.parse_args()
    ctx = pa.Context(0)
    X, lab = problem(a)
    res = dict(device=ctx.name(), what=a.what, n=X.shape[0], d=X.shape[1], K=int(np.unique(lab).size), csr=bool(a.csr), nnz=int(X.nnz) if a.csr else None, rounds=a.rounds,
               copy_GBs=copy_rate(ctx))
    (score if a.what == "score" else cv)(a, ctx, X, lab, res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({k: (v if not isinstance(v, dict) else {kk: vv for kk, vv in v.items() if kk != "runs"}) for k, v in res.items()}))
    ctx.close()


if __name__ == "__main__":
    main()
