#!/usr/bin/env python3
"""The orbit operator in the symmetry-adapted basis (csrc/fshared_adapted.h: forward transform, k_fxa_prod, inverse transform), recorded bit for bit:
tests/test_gpu_orbit_adapted.py judges it against a long-double product within a multiple of the GEMM's error, which a change of how or when k_fxa_prod
loads its operands must not use up -- every output entry keeps its order of summation, so the bits stay.  tests/test_gpu_orbit_adapted_bits.py recomputes compute_case() and compares
for equality.

    python tests/golden/make_orbit_adapted_bits.py [--commit HASH] [--out FILE]

needs a GPU and the built library; it writes tests/golden/orbit_adapted_bits.json, whose meta names the commit and the compiler that produced the bits.  Run it
again (on the commit whose bits are to be kept) only when the toolchain or the intended arithmetic changes.

The problem of a case is tests/test_gpu_orbit_adapted.py::_problem (contact problem on sub cubes of nel^3 elements, adapted form on, kplus_rtol = rtol = 1e-13).
Per case: one SHA-256 over the little-endian float64 bytes of dense_mult's output for a seeded random multivector that is zero off every block's touched set,
one over F.mult's output for a seeded lambda, and the plan of k_fxa_prod as pmh_fexplicit_orbit_adapted_info reports it (per irrep d, m, nks, items per width,
trips per wave), which covers() checks: the cases are the smallest at which the k loop of k_fxa_prod can go wrong.

  2x2x2/nel4, nel5   every irrep is ONE trip in all: waves 0 .. 2 run none, wave 3 one (first loads and last products with nothing between)
  2x2x2/nel12        the three-dimensional irreps: nks = 24, three trips, waves 1 .. 3 one each, wave 0 none
  2x2x2/nel22        the three-dimensional irreps (m = 529 .. 562, nks = 72): nine trips, 2 / 2 / 2 / 3 -- unequal waves, every wave past its first trip
  4x2x2/nel12        16 blocks = 2 groups: the three-dimensional irreps have 48 columns, ONE item of 3 blocks of columns per block of rows (trips of 4 k steps), 1 / 2 / 1 / 2
  4x4x4/nel12        64 blocks = 8 groups: items of 4 blocks of columns (trips of 4 k steps), six trips, 1 / 2 / 1 / 2
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
JSON = os.path.join(HERE, "orbit_adapted_bits.json")
CASES = {"2x2x2/nel4": ((2, 2, 2), 4), "2x2x2/nel5": ((2, 2, 2), 5), "2x2x2/nel12": ((2, 2, 2), 12), "2x2x2/nel22": ((2, 2, 2), 22), "4x2x2/nel12": ((4, 2, 2), 12), "4x4x4/nel12": ((4, 4, 4), 12)}


def _pa():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import permon_amd as pa

    return pa


def problem(ctx, sub, nel):
    """tests/test_gpu_orbit_adapted.py::_problem"""
    pa = _pa()
    from permon_amd._lib import check
    from permon_amd.chain import FetiDualQP

    check(ctx.L.pmh_set_knob(b"orbit_adapted", 1))
    f = pa.CubeFeti(sub, nel, contact=True)
    G, e = f.coarse()
    nn = nel + 1
    q = FetiDualQP(ctx, f.subset(range(f.nsub)), G, e, f.c, f.lb, kplus_rtol=1e-13, explicit=dict(rtol=1e-13, storage="class_orbit", symmetry=dict(dims=(nn, nn, nn), ndof=3)))
    assert q.explicit_storage == "class_orbit" and q.explicit_symmetries == 48 and q.E.orbit_adapted(0)
    return f, q


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<f8").tobytes()).hexdigest()


def compute_case(ctx, f, q, nel):
    """The case as the file keeps it; two applications of either operator must give the same bits (asserted here, so by the test too)"""
    from permon_amd._lib import check

    E = q.E
    ngroups = (f.nsub + 7) // 8
    ntot, _ = E.compressed_size()
    ld = ntot // (8 * ngroups)
    urel = E.class_union(0)
    rng = np.random.default_rng(100 + nel)
    x = np.zeros(ntot)
    for b in range(f.nsub):
        g = np.zeros(int(E.n_gamma[b]), dtype=np.int32)  # Gamma_b alone (E.block(b) would copy the whole of W_b to the host)
        check(ctx.L.pmh_fexplicit_get_block(E.h, b, None, g.ctypes.data_as(C.c_void_p)))
        idx = (b // 8) * ld * 8 + np.searchsorted(urel, g - b * f.n_i) * 8 + b % 8
        x[idx] = rng.standard_normal(idx.size)
    xv, y, y2 = ctx.vec_from(x), ctx.vec(ntot), ctx.vec(ntot)
    E.dense_mult(xv, y)
    E.dense_mult(xv, y2)
    y, y2 = y.to_numpy(), y2.to_numpy()
    assert np.array_equal(y, y2) and np.any(y)
    lam = np.random.default_rng(6).standard_normal(f.n_lambda)
    lv, z, z2 = ctx.vec_from(lam), ctx.vec(f.n_lambda), ctx.vec(f.n_lambda)
    q.F.mult(lv, z)
    q.F.mult(lv, z2)
    z, z2 = z.to_numpy(), z2.to_numpy()
    assert np.array_equal(z, z2) and np.any(z)
    plan = [dict(d=i["d"], m=i["m"], nks=i["nks"], items=i["items"], trips=i["trips_wide"] if i["items"][2] + i["items"][3] else i["trips"]) for i in E.orbit_adapted_info(0)]
    for i, full in zip(plan, E.orbit_adapted_info(0)):  # an irrep's items are of one kind in every case here, so `trips` is what each of them runs
        assert not ((full["items"][0] + full["items"][1]) and (full["items"][2] + full["items"][3]))
    return {"groups": ngroups, "n": int(ntot), "n_lambda": int(f.n_lambda), "dense_mult": _sha(y), "F_mult": _sha(z), "plan": plan}


def covers(cases):
    """What the cases must hold between them (the table in the module's docstring); main() asserts it of what it computed, the test of the file"""
    def irreps(name, d=None):
        return [i for i in cases[name]["plan"] if sum(i["items"]) and (d is None or i["d"] == d)]

    for name in ("2x2x2/nel4", "2x2x2/nel5"):
        assert irreps(name) and all(i["nks"] == 8 and i["trips"] == [0, 0, 0, 1] and not (i["items"][2] + i["items"][3]) for i in irreps(name)), name
    t = irreps("2x2x2/nel12", 3)
    assert len(t) == 4 and all(i["nks"] == 24 and i["trips"] == [0, 1, 1, 1] and i["items"][1] and not i["items"][3] for i in t)
    t = irreps("2x2x2/nel22", 3)
    assert len(t) == 4 and all(i["nks"] == 72 and i["trips"] == [2, 2, 2, 3] and i["items"][1] for i in t)
    assert cases["4x2x2/nel12"]["groups"] == 2
    t = irreps("4x2x2/nel12", 3)
    assert len(t) == 4 and all(i["nks"] == 24 and i["items"][2] > 0 and not (i["items"][0] + i["items"][1] + i["items"][3]) and i["trips"] == [1, 2, 1, 2] for i in t)
    assert cases["4x4x4/nel12"]["groups"] == 8
    t = irreps("4x4x4/nel12", 3)
    assert len(t) == 4 and all(i["items"][3] and not (i["items"][0] + i["items"][1]) and i["trips"] == [1, 2, 1, 2] for i in t)
    assert all(i["items"][3] for i in irreps("4x4x4/nel12"))
    assert all(any(i["items"][w] for c in cases.values() for i in c["plan"]) for w in range(4))  # every instantiation of the loop runs somewhere


def compute():
    pa = _pa()
    out = {}
    ctx = pa.Context(0)
    try:
        for name, (sub, nel) in CASES.items():
            f, q = problem(ctx, sub, nel)
            out[name] = compute_case(ctx, f, q, nel)
            del f, q
    finally:
        ctx.close()
    return out


def write(fh, meta, cases):
    fh.write('{"meta": %s,\n "cases": {\n' % json.dumps(meta, sort_keys=True))
    fh.write(",\n".join('  %s: %s' % (json.dumps(name), json.dumps(cases[name], sort_keys=True)) for name in sorted(cases)))
    fh.write("\n }}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None, help="the commit the library's kernels were built from (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=JSON)
    a = ap.parse_args()
    commit = a.commit or subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
    hipcc = [ln for ln in subprocess.check_output(["hipcc", "--version"], text=True).splitlines() if ln.strip()]
    cases = compute()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        write(fh, {"generator": "tests/golden/make_orbit_adapted_bits.py", "commit": commit, "hipcc": hipcc[0]}, cases)
    for name in sorted(cases):
        print(name, [(i["d"], i["m"], i["nks"], i["trips"]) for i in cases[name]["plan"]])
    covers(cases)
    print("wrote", a.out, len(cases), "cases")


if __name__ == "__main__":
    main()
