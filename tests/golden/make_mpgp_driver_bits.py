#!/usr/bin/env python3
"""The fused MPGP driver (csrc/mpgp.hip solve_fused) under SMALXE, recorded bit for bit: the whole-solve tests of tests/test_gpu_mpgp_phases.py run MPGP alone, so
the hooks SMALXE hangs on the inner solve (pre_test, pre_p1), the gradient it carries from one inner solve to the next, its word that the first gradient repeats
the last application (with the projection's word beside it) and the decision not to enqueue a product ahead of a test that is likely to end the solve are held
elsewhere by counts and tolerances only.  tests/test_gpu_mpgp_driver_bits.py recomputes compact(compute_case()) and compares for equality.

    python tests/golden/make_mpgp_driver_bits.py [--commit HASH] [--out FILE]

needs a GPU and the built library; it writes tests/golden/mpgp_driver_bits.json, whose meta names the commit and the compiler that produced the bits.  Run it
again (on the commit whose bits are to be kept) only when the toolchain or the intended arithmetic changes.

The problem: the contact problem of tests/test_gpu_chain_replay.py::_problem, 2 x 2 x 2 cubes of 3^3 and of 4^3 elements, on each K^+ path that file
parametrises (KPLUS).  A case is named <K^+ path>/nel<elements per edge>/<mode>.
Modes, each a SMALXE solve from lambda = 0 with the knob `chain` on:
  replay   `chain_replay` on: the first gradient of every inner solve after the first is the caller's "same vector again" (first_applied, the projection's word)
  full     `chain_replay` off
  reuse    `chain_replay` on and pmh_smalxe_set_reuse_products: every inner solve after the first starts from the carried gradient
  dist     `distributed` = 1 on a one-rank communicator: every sum finalised on the device at once, no emission, no word from the caller
  prop, prop_dist   as replay and as dist, with the inner solver's proportioning constant Gamma = 0.01 in place of 1: with Gamma = 1 no inner solve of either size
           takes a proportioning step (measured: 40 CG and 6 expansion steps on 3^3, 35 and 9 on 4^3); with 0.01 the solves take one (3^3) and two (4^3)

SMALXE keeps the trace of its last inner solve only, so the K inner solves of a case are recorded from K solves with the outer iteration limit at 1, 2, ... K: the
arithmetic is deterministic (fixed summation orders), solve k repeats the first k - 1 inner solves of the full one and ends on the k-th.  Per inner solve: the step
string, the monitor's three norms per test as float.hex(), nmv / ncg / nexp / nprop (the differences of the running totals) and the number of tests; for the full
solve: lambda as a SHA-256 of its little-endian float64 bytes, and the outer and inner totals.  The file keeps each case on one line (compact): the norms of a
case go into one SHA-256.

`carried` of an inner solve is derived, not read: the driver counts one product for the first gradient unless it was carried, one per CG or proportioning step and
two per expansion step, so nmv == ncg + 2 nexp + nprop exactly where the gradient was carried.  main() asserts what the cases must cover between them.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
JSON = os.path.join(HERE, "mpgp_driver_bits.json")
SUB, NELS = (2, 2, 2), (3, 4)
KPLUS = {  # a copy of tests/test_gpu_chain_replay.py::KPLUS (this file runs without pytest); test_gpu_mpgp_driver_bits.py asserts that the two agree
    "orbit": lambda nn: dict(explicit=dict(rtol=1e-13, storage="class_orbit", symmetry=dict(dims=(nn, nn, nn), ndof=3))),
    "sym": lambda nn: dict(explicit=dict(rtol=1e-13, storage="sym")),
    "iterative": lambda nn: dict(),
}
MODES = ("replay", "full", "reuse", "dist", "prop", "prop_dist")
GAMMA_PROP = 0.01
CASES = [(k, nel, m) for k in KPLUS for nel in NELS for m in MODES]


def _pa():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import permon_amd as pa

    return pa


def problem(ctx, kplus, nel):
    pa = _pa()
    from permon_amd.chain import FetiDualQP

    f = pa.CubeFeti(SUB, nel, contact=True)
    G0, e0 = f.coarse(orthonormalize=False)
    return FetiDualQP(ctx, f.subset(range(f.nsub)), G0, e0, f.c, f.lb, orthonormal="implicit", kplus_rtol=1e-13, **KPLUS[kplus](nel + 1))


def _inner_trace(qps):
    from permon_amd import _lib

    cap, ln = 4096, C.c_int()
    step = C.create_string_buffer(cap + 1)
    arrs = [np.zeros(cap) for _ in range(3)]
    _lib.check(qps.L.pmh_mpgp_get_trace(qps._mpgp_handle(), cap, step, *[a.ctypes.data_as(_lib.c_double_p) for a in arrs], None, C.byref(ln)))
    assert ln.value <= cap
    return (step.raw[:ln.value].decode(),) + tuple([float(v).hex() for v in a[:ln.value]] for a in arrs)


def _solve(ctx, q, mode, max_it):
    """One SMALXE solve from lambda = 0 with at most max_it outer iterations: (stats, lambda, the last inner solve's trace)"""
    from permon_amd._lib import check

    check(ctx.L.pmh_set_knob(b"chain", 1)), check(ctx.L.pmh_set_knob(b"chain_replay", 0 if mode == "full" else 1))
    q.lam.set(0.0)
    qps = q.make_smalxe(max_it=max_it, inner=dict(monitor=1, distributed=int(mode.endswith("dist")), gamma=GAMMA_PROP if mode.startswith("prop") else 1.0))
    if mode == "reuse":
        qps.SMALXESetReuseProducts(True)
    st = qps.Solve()
    out = st, q.lam.to_numpy().copy(), _inner_trace(qps)
    qps.Destroy()
    check(ctx.L.pmh_set_knob(b"chain_replay", 1))
    return out


def _counts(i):
    return [i.nmv, i.ncg, i.nexp, i.nprop]


def compute_case(ctx, q, mode):
    """ctx: for the modes "dist" and "prop_dist" a context with a one-rank communicator (dist_context), q = problem(ctx, kplus, nel)"""
    st, lam, last = _solve(ctx, q, mode, 100)
    K = st.iteration
    assert st.reason > 0 and 1 < K < 40
    out = {"lambda": hashlib.sha256(np.ascontiguousarray(lam, dtype="<f8").tobytes()).hexdigest(), "n": int(lam.size),
           "outer": dict(reason=st.reason, iteration=st.iteration, inner_iter_accu=st.inner_iter_accu, M1_hits=st.M1_hits, eta_hits=st.eta_hits, M1_updates=st.M1_updates,
                         rho_updates=st.rho_updates, rho=float(st.rho).hex(), M1=float(st.M1).hex(), normBu=float(st.normBu).hex(), rnorm=float(st.rnorm).hex()),
           "inner_totals": dict(zip(("nmv", "ncg", "nexp", "nprop"), _counts(st.inner))), "inner": []}
    prev, accu = [0, 0, 0, 0], 0
    for k in range(1, K + 1):
        sk, _, tr = (st, lam, last) if k == K else _solve(ctx, q, mode, k)
        assert sk.iteration == k
        now = _counts(sk.inner)
        nmv, ncg, nexp, nprop = [a - b for a, b in zip(now, prev)]
        its = sk.inner_iter_accu - accu
        prev, accu = now, sk.inner_iter_accu
        assert len(tr[0]) == its + 1 and tr[0][0] == " " and ncg + nexp + nprop == its, (k, tr[0], its)
        assert nmv - (ncg + 2 * nexp + nprop) in (0, 1)
        out["inner"].append(dict(steps=tr[0], gp=tr[1], gf=tr[2], gc=tr[3], nmv=nmv, ncg=ncg, nexp=nexp, nprop=nprop, iteration=its, carried=nmv == ncg + 2 * nexp + nprop))
    return out


def dist_context():
    """A context of its own with a one-rank communicator (as tests/test_gpu_chain.py::test_chain_with_device_finalised_scalars makes it); the caller closes it"""
    pa = _pa()
    old = os.environ.get("PMH_COMM_FORCE")
    os.environ["PMH_COMM_FORCE"] = "1"
    try:
        c = pa.Context(0)
        c.comm_init(0, 1, c.comm_unique_id())
    finally:
        if old is None:
            os.environ.pop("PMH_COMM_FORCE", None)
        else:
            os.environ["PMH_COMM_FORCE"] = old
    return c


def compact(case):
    """A case as the file keeps it, one line: the inner solves' step strings joined by "|" (each begins with the blank of its first test), their four counters
    as "nmv,ncg,nexp,nprop" joined by ";", `carried` as a string of 0 / 1, and ONE SHA-256 over the bit patterns of all monitor norms of all inner solves in
    order (gp, gf, gc of solve 1, then of solve 2 ...) -- every bit still takes part in the comparison, the file stays readable."""
    inner = case["inner"]
    norms = "\n".join(",".join(s[k]) for s in inner for k in ("gp", "gf", "gc"))
    return {"lambda": case["lambda"], "n": case["n"], "outer": case["outer"], "inner_totals": case["inner_totals"],
            "steps": "|".join(s["steps"] for s in inner), "counts": ";".join("%d,%d,%d,%d" % (s["nmv"], s["ncg"], s["nexp"], s["nprop"]) for s in inner),
            "carried": "".join("01"[s["carried"]] for s in inner), "norms": hashlib.sha256(norms.encode()).hexdigest()}


def covers(cases):
    """What the recorded inner solves (compact form) must hold between them (main() asserts it): all three step types, a carried gradient, a solve that ends
    within three steps -- and in mode reuse every inner solve after the first starts from the carried gradient, in the other modes none does."""
    solves = [(name, i, st, c["carried"][i]) for name, c in cases.items() for i, st in enumerate(c["steps"].split("|"))]
    assert all(any(t in st for _, _, st, _ in solves) for t in "cep")
    assert any(ca == "1" for _, _, _, ca in solves)
    assert any(len(st) - 1 <= 3 for _, _, st, _ in solves)
    assert all("p" in c["steps"] for name, c in cases.items() if "/prop" in name)
    for name, i, _, ca in solves:
        assert (ca == "1") == (name.endswith("/reuse") and i > 0), (name, i)


def compute():
    pa = _pa()
    out = {}
    ctx, dctx = pa.Context(0), None
    try:
        for kplus in KPLUS:
            for nel in NELS:
                q = problem(ctx, kplus, nel)
                for mode in MODES:
                    if not mode.endswith("dist"):
                        out["%s/nel%d/%s" % (kplus, nel, mode)] = compute_case(ctx, q, mode)
        dctx = dist_context()
        for kplus in KPLUS:
            for nel in NELS:
                q = problem(dctx, kplus, nel)
                for mode in MODES:
                    if mode.endswith("dist"):
                        out["%s/nel%d/%s" % (kplus, nel, mode)] = compute_case(dctx, q, mode)
    finally:
        ctx.close()
        if dctx is not None:
            dctx.close()
    return out


def write(f, meta, cases):
    """One line per case"""
    f.write('{"meta": %s,\n "cases": {\n' % json.dumps(meta, sort_keys=True))
    f.write(",\n".join('  %s: %s' % (json.dumps(name), json.dumps(cases[name], sort_keys=True)) for name in sorted(cases)))
    f.write("\n }}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None, help="the commit the library was built from (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=JSON)
    a = ap.parse_args()
    commit = a.commit or subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
    hipcc = [ln for ln in subprocess.check_output(["hipcc", "--version"], text=True).splitlines() if ln.strip()]
    cases = {name: compact(c) for name, c in compute().items()}
    covers(cases)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        write(f, {"generator": "tests/golden/make_mpgp_driver_bits.py", "commit": commit, "hipcc": hipcc[0]}, cases)
    print("wrote", a.out, len(cases), "cases,", sum(len(c["carried"]) for c in cases.values()), "inner solves")


if __name__ == "__main__":
    main()
