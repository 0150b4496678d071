#!/usr/bin/env python3
"""The bits of the SVM and SVR front ends (csrc/svm_train.hip, svr_train.hip, svm_proba.hip), recorded where tests/golden/svm_dense_bits.json does not look: one
SHA-256 per output array (its little-endian float64 bytes), floats as float.hex(), integers as they are.  tests/test_gpu_svm_front_bits.py recomputes compute()
and compares for equality, so a change that reassociates a sum of the bias pass, of the scoring sweeps, of the Platt fit or of a finishing kernel shows even
where every comparison to rounding still passes.

    python tests/golden/make_svm_front_bits.py [--commit HASH] [--out FILE]

needs a GPU and the built library; it writes tests/golden/svm_front_bits.json, whose meta names the commit and the compiler that produced the bits.  Run it again
(on the commit whose bits are to be kept) only when the toolchain or the intended arithmetic changes.

Shapes (all seeded; the smallest at which each kernel can still go wrong): dense 333 x 64 (several workgroups of the 64-row sweeps, a ragged last row group, an
odd n for the d == 64 layout), 301 x 37 and 301 x 130 (the generic sweep below and above 64 features), each in fp64 and in float32; CSR 300 x 200 with 12 draws
per row and 5 % of the rows emptied (problems.svm_sparse / problems.svr_linear, the rows emptied as tests/test_gpu_svm_sparse.py empties them).  n > 256 gives
the one-thread-per-dot kernels work in their second workgroup.  Test sets: 333 rows.  -qps_rtol 1e-6, and -qps_max_it 100 with bias.

Cases:
  svr/<data>/<L1|L2|L2w|L1w>/<bias|flat>   SVR on every data set: alpha (u = [p; q]), w, b, every field of stats; predict on the test set (a hash of the scores)
             and every field of test's metrics.  Seven of the trainings without bias (L1 on the CSR case and on 301 x 37 with weights: targets with an offset of 3
             and no bias term) end after a few iterations with MPGP's divergence reason; their bits are recorded like the others'
  svr_re/<data>/<bias|flat>/...   on 301 x 37 fp64 and the CSR case (L1): set_epsilon then train (SMALXE is rebuilt, MPGP kept), set_penalties then train, and
             train once more: the second training's statistics show what the solver's counters do between trainings
  svm/<data>/<L1|L2|L1w>/<bias|flat>   SVM on the CSR case; L1w (the per-sample upper bound in the bias pass) on every dense data set as well
  svm_predict/<data>   333 x 64 and 301 x 37 in fp64 and float32, and the CSR case (L1, bias): scores, labels and the four counts of test; predict_proba after
             set_calibration(-1.7, 0.3); calibrate on the 333 test samples: A, B and every field of the Platt statistics; then under train_mask: test_own for
             held_out, subset and all
  svm_warm/<data>/<bias|flat>   333 x 64 fp64 and the CSR case (L1): train, set_penalties with twice the C, train(warm_start=True, alpha_scale=2): alpha, stats
             and warm_start_counts.  The warm training follows a cold one on the same solver, so its statistics record what carries over
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
JSON = os.path.join(HERE, "svm_front_bits.json")
OPTS = "-qps_rtol 1e-6 -qps_max_it 100"
OPTS_FLAT = "-qps_rtol 1e-6"
SHAPES = [(333, 64, 3.0), (301, 37, 2.0), (301, 130, 2.0)]
CSR = (300, 200, 12, 1.0)  # n, d, draws per row, skew
N_TEST = 333
EMPTY = 0.05


def train_mask(n):
    """A copy of tests/test_gpu_svm_subset.py::train_mask (this file runs without pytest); test_gpu_svm_front_bits.py asserts that the two agree."""
    h = np.zeros(n, dtype=bool)
    h[0] = h[n - 1] = True
    h[64:192] = True
    h[3::5] = True
    return ~h


def zero_rows(X, frac, seed):
    """tests/test_gpu_svm_sparse.py::_zero_rows: a fraction frac of the samples without a stored entry."""
    X = X.tolil(copy=True)
    for i in np.random.default_rng(seed).choice(X.shape[0], int(frac * X.shape[0]), replace=False):
        X.rows[i], X.data[i] = [], []
    return X.tocsr()


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<f8").tobytes()).hexdigest()


def _num(v):
    return float(v).hex() if isinstance(v, float) else int(v)


def _fields(st):
    return {f: _num(getattr(st, f)) for f, _ in st._fields_}


def _opts(bias):
    return OPTS if bias else OPTS_FLAT


def svm_data(P):
    """name -> (X, y, C, X_test, y_test, sample_dtype)"""
    out = {}
    for n, d, off in SHAPES:
        p = P.svm_offset(n, d, off, N_test=N_TEST)
        out["%dx%d" % (n, d)] = (p["X"], p["y"], p["C"], p["X_test"], p["y_test"], None)
        out["%dx%d_f32" % (n, d)] = (p["X"].astype(np.float32), p["y"], p["C"], p["X_test"].astype(np.float32), p["y_test"], np.float32)
    n, d, per, skew = CSR
    p = P.svm_sparse(n, d, per, skew, 0.5, C=1.0, N_test=N_TEST)
    out["csr"] = (zero_rows(p["X"], EMPTY, 11), p["y"], p["C"], zero_rows(p["X_test"], EMPTY, 12), p["y_test"], None)
    return out


def svr_data(P):
    """name -> (X, t, C, X_test, t_test, sample_dtype)"""
    out = {}
    for n, d, _ in SHAPES:
        p = P.svr_linear(n, d, 0.2, 9, eps=0.1, C=0.1, n_test=N_TEST)
        out["%dx%d" % (n, d)] = (p["X"], p["t"], p["C"], p["X_test"], p["t_test"], None)
        out["%dx%d_f32" % (n, d)] = (p["X"].astype(np.float32), p["t"], p["C"], p["X_test"].astype(np.float32), p["t_test"], np.float32)
    n, d, per, skew = CSR
    p = P.svr_linear(n, d, 0.2, 9, sparse=(per, skew), eps=0.1, C=1.0, n_test=N_TEST)
    out["csr"] = (zero_rows(p["X"], EMPTY, 11), p["t"], p["C"], zero_rows(p["X_test"], EMPTY, 12), p["t_test"], None)
    return out


def _model(out, key, m):
    out[key + "/alpha"], out[key + "/w"], out[key + "/b"], out[key + "/stats"] = sha(m.alpha), sha(m.w), float(m.b).hex(), _fields(m.stats)


def _svr(pa, ctx, data, out):
    for name, (X, t, C, Xt, tt, dt) in data.items():
        wt = np.random.default_rng(2).uniform(0.5, 2.0, X.shape[0])
        for case, loss, weights in (("L1", "L1", None), ("L2", "L2", None), ("L2w", "L2", wt), ("L1w", "L1", wt)):
            for bias in (False, True):
                svr = pa.SVR(ctx, loss=loss, C=C, epsilon=0.1, bias=bias, options=_opts(bias), sample_dtype=dt).create(X, t, weights).train()
                key = "svr/%s/%s/%s" % (name, case, "bias" if bias else "flat")
                _model(out, key, svr)
                out[key + "/predict"] = sha(svr.predict(Xt))
                out[key + "/test"] = {k: _num(v) for k, v in svr.test(Xt, tt).items()}
                svr.destroy()
    for name in ("301x37", "csr"):
        X, t, C, Xt, tt, dt = data[name]
        wt = np.random.default_rng(4).uniform(0.5, 2.0, X.shape[0])
        for bias in (False, True):
            svr = pa.SVR(ctx, loss="L1", C=C, epsilon=0.3, bias=bias, options=_opts(bias)).fit(X, t)
            key = "svr_re/%s/%s" % (name, "bias" if bias else "flat")
            svr.set_epsilon(0.1).train()
            _model(out, key + "/set_epsilon", svr)
            svr.set_penalties(2.0 * C, wt).train()
            _model(out, key + "/set_penalties", svr)
            svr.train()
            _model(out, key + "/train_again", svr)
            svr.destroy()


def _svm(pa, ctx, data, out):
    for name, (X, y, C, Xt, yt, dt) in data.items():
        wt = np.random.default_rng(2).uniform(0.5, 2.0, X.shape[0])
        cases = (("L1", "L1", None), ("L2", "L2", None), ("L1w", "L1", wt)) if name == "csr" else (("L1w", "L1", wt),)
        for case, loss, weights in cases:
            for bias in (False, True):
                svm = pa.SVM(ctx, loss=loss, C=C, bias=bias, options=_opts(bias), sample_dtype=dt).create(X, y, weights).train()
                _model(out, "svm/%s/%s/%s" % (name, case, "bias" if bias else "flat"), svm)
                svm.destroy()


def _svm_predict(pa, ctx, data, out):
    for name in ("333x64", "333x64_f32", "301x37", "301x37_f32", "csr"):
        X, y, C, Xt, yt, dt = data[name]
        svm = pa.SVM(ctx, loss="L1", C=C, bias=True, options=OPTS, sample_dtype=dt).fit(X, y)
        key = "svm_predict/" + name
        out[key + "/scores"], out[key + "/labels"] = sha(svm.decision_function(Xt)), sha(svm.predict(Xt))
        out[key + "/test"] = {k: _num(v) for k, v in svm.test(Xt, yt).items()}
        out[key + "/proba"] = sha(svm.set_calibration(-1.7, 0.3).predict_proba(Xt))
        A, B = svm.calibrate(Xt, yt).calibration
        out[key + "/calibrate"] = dict(A=float(A).hex(), B=float(B).hex(), stats=_fields(svm.calibration_stats))
        svm.set_subset(train_mask(X.shape[0])).train()
        for which in ("held_out", "subset", "all"):
            out[key + "/test_own/" + which] = {k: _num(v) for k, v in svm.test_own(which).items()}
        svm.destroy()


def _svm_warm(pa, ctx, data, out):
    for name in ("333x64", "csr"):
        X, y, C, Xt, yt, dt = data[name]
        for bias in (False, True):
            svm = pa.SVM(ctx, loss="L1", C=C, bias=bias, options=_opts(bias)).fit(X, y)
            svm.set_penalties(2.0 * C, 2.0 * C).train(warm_start=True, alpha_scale=2.0)
            key = "svm_warm/%s/%s" % (name, "bias" if bias else "flat")
            out[key + "/alpha"], out[key + "/stats"], out[key + "/warm_start_counts"] = sha(svm.alpha), _fields(svm.stats), svm.warm_start_counts
            svm.destroy()


def compute():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import permon_amd as pa
    from permon_amd import problems as P

    ctx = pa.Context(0)
    out = {}
    try:
        dc, dr = svm_data(P), svr_data(P)
        for X in (dc["csr"][0], dc["csr"][3], dr["csr"][0], dr["csr"][3]):  # a condition on the input: the empty rows are there
            assert (np.diff(X.indptr) == 0).sum() >= int(EMPTY * X.shape[0])
        _svr(pa, ctx, dr, out)
        _svm(pa, ctx, dc, out)
        _svm_predict(pa, ctx, dc, out)
        _svm_warm(pa, ctx, dc, out)
    finally:
        ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None, help="the commit the library was built from (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=JSON)
    a = ap.parse_args()
    commit = a.commit or subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
    hipcc = [ln for ln in subprocess.check_output(["hipcc", "--version"], text=True).splitlines() if ln.strip()]
    cases = compute()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"meta": {"generator": "tests/golden/make_svm_front_bits.py", "commit": commit, "hipcc": hipcc[0]}, "cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out, len(cases), "entries")


if __name__ == "__main__":
    main()
