#!/usr/bin/env python3
"""The bits of the dense SVM path (csrc/svm.hip, svm_rows.h, svm_train.hip), recorded: one SHA-256 per output array (its little-endian float64 bytes), plus the
MPGP step strings, pass counts and training statistics.  tests/test_gpu_svm_dense_bits.py recomputes compute() and compares for equality, so a change of the
kernels that reassociates a sum, or moves a launch, shows even where both pass forms move together.

    python tests/golden/make_svm_dense_bits.py [--commit HASH] [--out FILE]

needs a GPU and the built library; it writes tests/golden/svm_dense_bits.json, whose meta names the commit and the compiler that produced the bits.  Run it again
(on the commit whose bits are to be kept) only when the toolchain or the intended arithmetic changes.

Cases (all seeded; the smallest shapes with several workgroups and a ragged last row group):
  op/...     X of 777 x 64 (four workgroups of the paired kernels; 777 is no multiple of 8), 301 x 37, 301 x 130; the five forms of
             test_subset_operator_against_numpy (plain, shift, diag, shift+sigma, diag+sigma), each on all samples and under train_mask: H.mult(v).
             The model pass w = X'(y o a) (form_w) is not hashed per form: it is always the plain pass 1, whatever terms the operator carries, and only a
             trained handle hands it out, so the train/ cases pin it, for every X with and without the mask.
  mpgp/...   777 x 64 (problems.svm_dual, the instance of test_svm_paired_passes_equal_separate_passes at N = 777, its seeds unchanged), box 0 <= a <= 1, MPGP_ITERS
             iterations by RunFixed, plain / shift / diag, all samples and train_mask, svm_pairing on and off: the iterate, the step string, passes().
             compute(record=True) asserts of every paired run that its step string holds "ee" and a "c" and that it streamed X fewer than twice per product:
             then k_svm_x64_p1<1,...>, the prepared gradient and k_svm_colsum_feas ran.  A condition on the input, checked when the file is recorded.  From
             x0 = 0 this instance takes expansion steps alone for its first 90 to 150 iterations (60 iterations give " peee...e" in all six runs): the seeds
             stay, the iteration count is 200, by which every run has mixed CG and expansion steps.
  train/...  pa.SVM on the three X, all samples and train_mask, L1 (plain), L2 (shift) and L2 with sample weights (diag), without bias (MPGP) and with (SMALXE:
             sigma_fold and the ||B u|| rider): alpha, w (the model pass form_w), b and every field of the statistics, iteration and pass counts included.
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
JSON = os.path.join(HERE, "svm_dense_bits.json")
MPGP_ITERS = 200
OPTS = "-qps_rtol 1e-6 -qps_max_it 100"
SHAPES = [(777, 64, 3.0), (301, 37, 2.0), (301, 130, 2.0)]
UNMET = []  # paired MPGP runs that miss the condition on their step string (compute(record=True))
FORMS = [("plain", 0.0, False, 0.0), ("shift", 1.0 / 0.7, False, 0.0), ("diag", 0.0, True, 0.0), ("shift+sigma", 1.0 / 0.7, False, 2.5), ("diag+sigma", 0.0, True, 2.5)]


def train_mask(n):
    """A copy of tests/test_gpu_svm_subset.py::train_mask (this file runs without pytest); test_gpu_svm_dense_bits.py asserts that the two agree."""
    h = np.zeros(n, dtype=bool)
    h[0] = h[n - 1] = True
    h[64:192] = True
    h[3::5] = True
    return ~h


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<f8").tobytes()).hexdigest()


def _num(v):
    return float(v).hex() if isinstance(v, float) else int(v)


def _operator(pa, P, ctx, out):
    for n, d, off in SHAPES:
        p = P.svm_offset(n, d, off)
        X, y = p["X"], p["y"]
        rng = np.random.default_rng(1)
        vd = ctx.vec_from(rng.standard_normal(n))
        dg = rng.uniform(0.5, 2.0, n)
        H = pa.MatCreateSVMDual(ctx, X, y)
        for sub in (False, True):
            H.set_subset(train_mask(n) if sub else None)
            for name, shift, diag, sigma in FORMS:
                H.set_diag(None), H.set_terms(shift, sigma), H.set_diag(dg if diag else None)
                o = ctx.vec(n)
                H.mult(vd, o)
                out["op/%dx%d/%s/%s" % (n, d, "subset" if sub else "all", name)] = sha(o.to_numpy())


def _mpgp(pa, P, ctx, out, record):
    import ctypes

    from permon_amd._lib import check

    found = ctypes.c_int()
    check(ctx.L.pmh_get_knob(b"svm_pairing", ctypes.byref(found)))
    n = 777
    p = P.svm_dual(n, 64)
    X, y = p["X"], p["y"]
    dg = np.random.default_rng(1).uniform(0.5, 2.0, n)
    for pairing in (1, 0):
        check(ctx.L.pmh_set_knob(b"svm_pairing", pairing))
        try:
            for sub in (False, True):
                m = train_mask(n) if sub else np.ones(n, dtype=bool)
                for name, shift, diag, _ in FORMS[:3]:
                    H = pa.MatCreateSVMDual(ctx, X, y)
                    if sub:
                        H.set_subset(m)
                    H.set_terms(shift, 0.0), H.set_diag(dg if diag else None)
                    qp = pa.QP(ctx)
                    qp.SetOperator(H)
                    qp.SetRhs(ctx.vec_from(m.astype(float)))
                    x = ctx.vec_from(p["x0"])
                    qp.SetInitialVector(x)
                    qp.SetBox(None, ctx.vec_from(p["lb"]), ctx.vec_from(p["ub"]))
                    qps = pa.QPS(ctx)
                    qps.SetQP(qp)
                    qps.SetType("mpgp")
                    qps.MonitorSet(True)
                    qps.SetUp()
                    p0 = H.passes()
                    st = qps.RunFixed(MPGP_ITERS)
                    steps, passes = qps.MPGPGetTrace()[0], H.passes() - p0
                    if record and pairing and not ("ee" in steps and "c" in steps and passes < 2 * st.nmv):
                        UNMET.append((name, sub, steps, passes, st.nmv))
                    key = "mpgp/%s/%s/%s" % ("paired" if pairing else "separate", "subset" if sub else "all", name)
                    out[key + "/x"] = sha(x.to_numpy())
                    out[key + "/steps"] = steps
                    out[key + "/counts"] = [int(st.nmv), int(st.ncg), int(st.nexp), int(st.nprop), int(passes)]
        finally:
            check(ctx.L.pmh_set_knob(b"svm_pairing", found.value))


def _train(pa, P, ctx, out):
    from permon_amd import _lib

    for n, d, off in SHAPES:
        p = P.svm_offset(n, d, off)
        X, y = p["X"], p["y"]
        wt = np.random.default_rng(2).uniform(0.5, 2.0, n)
        for sub in (False, True):
            for name, loss, weights in (("L1", "L1", None), ("L2", "L2", None), ("L2w", "L2", wt)):
                for bias in (False, True):
                    svm = pa.SVM(ctx, loss=loss, C=p["C"], bias=bias, options=OPTS if bias else "-qps_rtol 1e-6").create(X, y, weights)
                    if sub:
                        svm.set_subset(train_mask(n))
                    svm.train()
                    key = "train/%dx%d/%s/%s/%s" % (n, d, "subset" if sub else "all", name, "bias" if bias else "flat")
                    out[key + "/alpha"], out[key + "/w"], out[key + "/b"] = sha(svm.alpha), sha(svm.w), float(svm.b).hex()
                    st = svm.stats
                    out[key + "/stats"] = {f: _num(getattr(st, f)) for f, _ in _lib.SvmStats._fields_}
                    svm.destroy()


def compute(record=False):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import permon_amd as pa
    from permon_amd import problems as P

    ctx = pa.Context(0)
    out = {}
    try:
        _operator(pa, P, ctx, out)
        _mpgp(pa, P, ctx, out, record)
        _train(pa, P, ctx, out)
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
    cases = compute(record=True)
    for k in sorted(cases):
        if k.endswith("/steps") or k.endswith("/counts"):
            print(k, cases[k])
    assert not UNMET, ("paired runs without 'ee' and 'c' in the step string: change the seed or MPGP_ITERS", UNMET)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"meta": {"generator": "tests/golden/make_svm_dense_bits.py", "commit": commit, "hipcc": hipcc[0], "mpgp_iters": MPGP_ITERS}, "cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out, len(cases), "entries")


if __name__ == "__main__":
    main()
