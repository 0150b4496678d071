"""What the scoring and bias passes of the SVM and SVR front ends cost on two or more builds of the library (docs/LAB_NOTEBOOK.md, "One training core, one family
of row kernels"): one GPU, one child process per build and visit, the builds visited in turn (A H B H ...), so that a difference between two builds can be
read against the difference one build shows against a copy of itself.

    python scripts/dev/svm_front_cost.py --lib parentA=/path/a.so --lib head=permon_amd/libpermonhip.so --lib parentB=/path/b.so --lib head=... --out out/f.json

Per visit and case: SVM.test, SVM.predict_proba and SVR.test on device-resident test samples (pmh_svm_test, pmh_svm_predict_proba, pmh_svr_test and their _f32 /
_csr forms called directly: nothing is uploaded inside the window), and a training cut off after two iterations (form_w, the bias pass and the model's tail
beside two solver iterations whose code is the same in every build).  Windows of `--calls` calls between HIP events on the launch stream
(pmh_timer_start / pmh_timer_stop), `--rounds` windows after one of warm-up; the figure of a visit is the median window in ms per call.
Cases: 2.5M x 64 fp64, 2.5M x 64 float32, 1M x 130 fp64, and CSR samples drawn as bench.py's sparse SVM rows are (problems.svm_sparse)."""
import argparse
import ctypes as ct
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CASES = {  # n, d, float32, sparse (nnz_row, skew)
    "dense64": (2500000, 64, False, None),
    "dense64_f32": (2500000, 64, True, None),
    "dense130": (1000000, 130, False, None),
    "csr": (1000000, 50000, False, (60, 1.0)),
}


def visit(lib, calls, rounds, scale):
    sys.path.insert(0, ROOT)
    from permon_amd import _lib

    _lib.LIB_PATH = os.path.abspath(lib)
    import permon_amd as pa
    from permon_amd import problems as P
    from permon_amd._lib import check
    from permon_amd.core import Vec, VecF32
    from permon_amd.mat import csr_from_scipy

    ctx = pa.Context(0)
    L, out = ctx.L, {}

    def timed(f):
        t = []
        for r in range(rounds + 1):
            ctx.timer_start()
            for _ in range(calls):
                f()
            t.append(ctx.timer_stop() / calls)
        return float(np.median(t[1:]))

    for name, (n, d, f32, sparse) in CASES.items():
        n = max(1000, int(n * scale))
        if sparse:
            p = P.svm_sparse(n, d, sparse[0], sparse[1], 0.5, seed=3)
            X, y = p["X"], p["y"]
        else:
            r = np.random.default_rng(5)
            X = r.standard_normal((n, d), dtype=np.float32)
            y = np.where(X[:, 0] + 0.3 * X[:, 1] + 0.5 > 0, 1.0, -1.0)
            X = X if f32 else X.astype(np.float64)
        t = (X[:, :8].sum(axis=1) if not sparse else np.asarray(X.sum(axis=1)).ravel()).astype(np.float64) + 3.0
        dt = np.float32 if f32 else None
        opts = "-qps_max_it 2"
        svm = pa.SVM(ctx, loss="L1", C=1.0, bias=False, options=opts, sample_dtype=dt).create(X, y)
        svr = pa.SVR(ctx, loss="L2", C=1.0, epsilon=0.1, bias=False, options=opts, sample_dtype=dt).create(X, t)
        res = {"train_svm": timed(lambda: check(L.pmh_svm_train(svm.h))), "train_svr": timed(lambda: check(L.pmh_svr_train(svr.h)))}
        svm.set_calibration(-1.7, 0.3)
        Xd = svm._keep[0]  # the handle's own device copy serves as the test set
        xa = (Xd.h,) if sparse else (n, Xd.p)
        yd, td, pd = Vec.from_numpy(ctx, y), Vec.from_numpy(ctx, t), Vec(ctx, n, zero=False)
        cnt, m = (ct.c_longlong * 4)(), _lib.SvrMetrics()
        res["svm_test"] = timed(lambda: check(svm._entry("test", bool(sparse), f32)(svm.h, *xa, yd.p, cnt)))
        res["svm_proba"] = timed(lambda: check(svm._entry("predict_proba", bool(sparse), f32)(svm.h, *xa, pd.p)))
        res["svr_test"] = timed(lambda: check(svr._entry("test", bool(sparse), f32)(svr.h, *xa, td.p, ct.byref(m))))
        res["check"] = [int(c) for c in cnt] + [float(m.sum_r2).hex(), float(np.sum(pd.to_numpy())).hex()]  # (equal over the builds: same results)
        for v in (yd, td, pd):
            v.free()
        svm.destroy(), svr.destroy()
        out[name] = res
        print(lib, name, res, flush=True)
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", action="append", default=[], help="NAME=PATH, in the order of the visits; a name may come several times")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--scale", type=float, default=1.0, help="the cases' sample counts times this (a rehearsal)")
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "svm_front_cost.json"))
    ap.add_argument("--visit", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.visit:
        print("RESULT " + json.dumps(visit(a.visit, a.calls, a.rounds, a.scale)))
        return
    visits = []
    for spec in a.lib:
        name, path = spec.split("=", 1)
        o = subprocess.run([sys.executable, os.path.abspath(__file__), "--visit", path, "--calls", str(a.calls), "--rounds", str(a.rounds), "--scale", str(a.scale)], stdout=subprocess.PIPE, text=True, timeout=600)
        if o.returncode != 0:
            sys.exit("the visit of %s ended with status %d: nothing more is started" % (name, o.returncode))
        visits.append({"lib": name, "ms_per_call": json.loads([ln for ln in o.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])})
        print(name, "done", flush=True)
    names = sorted({v["lib"] for v in visits})
    summary = {}
    for case in CASES:
        for key in ("svm_test", "svm_proba", "svr_test", "train_svm", "train_svr"):
            summary["%s/%s" % (case, key)] = {nm: [round(v["ms_per_call"][case][key], 4) for v in visits if v["lib"] == nm] for nm in names}
        chk = [v["ms_per_call"][case]["check"] for v in visits]
        assert all(c == chk[0] for c in chk), ("the builds disagree on the results of", case, chk)
    for k, v in summary.items():
        print(k, v)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"command": " ".join(sys.argv), "calls": a.calls, "rounds": a.rounds, "scale": a.scale, "visits": visits, "summary": summary}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
