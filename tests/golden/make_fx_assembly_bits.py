#!/usr/bin/env python3
"""The set-up of the explicit local dual operators (pmh_fexplicit_assemble: batches of K^+ solves on unit right-hand sides, one row of W per solve), recorded bit for bit.
tests/test_gpu_explicit.py judges the assembled blocks against pinv to 1e-10, which would not notice a column solved in another slot or batch (another companion in the
batched CG, the same W to 1e-13) or a row written twice.  The K^+ solvers use no floating-point atomics and reduce in fixed orders, so the same schedule gives the same
bits: tests/test_gpu_fx_assembly_bits.py recomputes every case and compares for equality.

    python tests/golden/make_fx_assembly_bits.py [--commit HASH] [--out FILE]

needs a GPU and the built library; it writes tests/golden/fx_assembly_bits.json, whose meta names the commit and the compiler that produced the bits.  Run it again (on
the commit whose bits are to be kept) only when the toolchain or the intended arithmetic changes.

Per case: one SHA-256 per block over the little-endian float64 bytes of E.block(b) (where the storage hands blocks out: not the striped orbit form), the number of K^+
solves (assemble_stats()[0]) and, for striped shares, a SHA-256 of E.mult for a seeded lambda.  The cases are the smallest at which each branch of the set-up is taken
(the constructions of tests/test_gpu_explicit.py):

  edge/<counts>/<full|sym>/mv<0|1>   three 5^3-node cubes, block 1 = 1.5 K (a class of its own), touched counts (5, 0, 260) / (127, 128, 129): an untouched block, two
                                     congruent blocks with different Gamma sharing a union, classes of unequal column counts (idle slots in late batches), rows in several
                                     32-row bands and on both sides of the 128-column tile edge; one column per block, and 8 on the multi-right-hand-side K^+
  noclass/full                       no classes given: slot s <-> block s
  replica/sym                        one block, four replica slots of its matrix
  class/..., class_sym/...           the class-shared storages without symmetries (2x2x1, nel 5)
  class_sym+sym/...                  set-up by symmetry: orbit members, the self-check batch (48 operations at 2x2x2 / nel 4, 8 at 2x2x1 / nel 5)
  class_orbit/...                    the representatives' rows alone, the closing symmetry-adapted form
  striped/...                        rank 1 of 3: sym and class (nel 8), class_sym by symmetry over four mega bands (nel 14), class_orbit
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
JSON = os.path.join(HERE, "fx_assembly_bits.json")


def _pa():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import permon_amd as pa

    return pa


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<f8").tobytes()).hexdigest()


# ---- the constructions: each returns (E, keep) with E assembled through MatExplicitDual.assemble; `keep` holds what E borrows ----------------------------------------
def edge(ctx, ntouch, storage, mv):
    """tests/test_gpu_explicit.py::test_explicit_edge_cases; mv: the V-cycle of tests/test_gpu_general.py on the blocks, which the multi-right-hand-side K^+ needs"""
    import scipy.sparse as sp

    pa = _pa()
    rng = np.random.default_rng(21 + sum(ntouch))
    f = pa.CubeFeti((3, 1, 1), 4, contact=False)
    K = sp.block_diag([f.Ki, 1.5 * f.Ki, f.Ki], format="csr")
    rows, roots, vals = [], [], []
    for b, nt in enumerate(ntouch):
        for d in np.sort(rng.choice(f.n_i, size=nt, replace=False)) + b * f.n_i:
            for _ in range(1 + int(rng.integers(0, 2))):
                rows.append(d), roots.append(int(rng.integers(0, 40))), vals.append(float(rng.choice([-1.0, 1.0, 0.5])))
    Kd = pa.MatBlockDiag.from_scipy(ctx, f.block_rowstart, K)
    Kp = pa.MatInv(Kd, rtol=1e-13, max_it=5000, nullspace=f.R)
    if mv:
        Kp.enable_bsr3()
        Kp.set_pc_mg_box(K, [(5, 5, 5)] * 3, 3, R=f.R, min_nodes=27, precision="fp32")
    B = pa.MatGluing(ctx, f.N, 40, np.array(rows, dtype=np.int32), np.array(roots, dtype=np.int32), np.array(vals))
    E = pa.MatExplicitDual(B, Kd, storage=storage)
    assert E.n_gamma.tolist() == list(ntouch)
    cls = pa.csr_block_classes(f.block_rowstart, K)
    assert cls.tolist() == [0, 1, 0]
    E.assemble(Kp, slot_class=cls, block_class=cls, rtol=1e-13, multi_rhs=mv)
    return E, (f, Kd, Kp, B)


def _qp(ctx, f, loc):
    from permon_amd.chain import FetiDualQP

    G, e = f.coarse()
    return FetiDualQP(ctx, loc, G, e, f.c, f.lb, kplus_rtol=1e-13)


def noclass(ctx):
    pa = _pa()
    f = pa.CubeFeti((2, 2, 1), 2, contact=True)
    q = _qp(ctx, f, f.subset(range(f.nsub)))
    E = pa.MatExplicitDual(q.B, q.K, storage="full")
    E.assemble(q.Kplus, rtol=1e-13)
    return E, (f, q)


def replica(ctx):
    """tests/test_gpu_explicit.py::test_explicit_replica_solver"""
    import scipy.sparse as sp

    pa = _pa()
    f = pa.CubeFeti((2, 1, 1), 4, contact=True)
    loc = f.subset([0])

    def factory(nslots):
        Kb = pa.MatBlockDiag.from_scipy(ctx, np.arange(nslots + 1, dtype=np.int32) * f.n_i, sp.block_diag([f.Ki] * nslots, format="csr"))
        return pa.MatInv(Kb, rtol=1e-13, max_it=20000, nullspace=np.tile(loc["R"], (1, nslots)))

    q = _qp(ctx, f, loc)
    E = q.assemble_explicit(loc, rtol=1e-13, min_slots=4, solver_factory=factory, multi_rhs=False)
    return E, (f, q)


def shared(ctx, sub, nel, storage, symmetry=None, stripe=None):
    """FetiDualQP.assemble_explicit on the contact problem of sub cubes of nel^3 elements; symmetry: None, "tiles" (class_sym by symmetry) or "orbit"; stripe: rank of 3"""
    pa = _pa()
    f = pa.CubeFeti(sub, nel, contact=True)
    nn = nel + 1
    sym = None if symmetry is None else dict(dims=(nn, nn, nn), ndof=3, orbit=symmetry == "orbit")
    if stripe is None:
        loc, st = f.subset(range(f.nsub)), None
    else:
        loc = f.subset([stripe])
        st = (stripe, 3, dict(n_x=f.N, block_rowstart=f.block_rowstart, leaves_row=f.leaves_row, leaves_root=f.leaves_root, leaves_sign=f.leaves_sign))
    q = _qp(ctx, f, loc)
    E = q.assemble_explicit(loc, rtol=1e-13, storage=storage, symmetry=sym, stripe=st, multi_rhs=False)
    assert q.explicit_storage == storage
    return E, (f, q)


CASES = {}
for _nt in ((5, 0, 260), (127, 128, 129)):
    for _st in ("full", "sym"):
        for _mv in (False, True):
            CASES["edge/%d-%d-%d/%s/mv%d" % (_nt + (_st, int(_mv)))] = (edge, (_nt, _st, _mv))
CASES.update({
    "noclass/full": (noclass, ()),
    "replica/sym": (replica, ()),
    "class/2x2x1/nel5": (shared, ((2, 2, 1), 5, "class")),
    "class_sym/2x2x1/nel5": (shared, ((2, 2, 1), 5, "class_sym")),
    "class_sym+sym/2x2x2/nel4": (shared, ((2, 2, 2), 4, "class_sym", "tiles")),
    "class_sym+sym/2x2x1/nel5": (shared, ((2, 2, 1), 5, "class_sym", "tiles")),
    "class_orbit/2x2x2/nel5": (shared, ((2, 2, 2), 5, "class_orbit", "orbit")),
    "class_orbit/2x2x1/nel5": (shared, ((2, 2, 1), 5, "class_orbit", "orbit")),
    "striped/sym/2x2x1/nel8": (shared, ((2, 2, 1), 8, "sym", None, 1)),
    "striped/class/2x2x1/nel8": (shared, ((2, 2, 1), 8, "class", None, 1)),
    "striped/class_sym+sym/2x2x1/nel14": (shared, ((2, 2, 1), 14, "class_sym", "tiles", 1)),
    "striped/class_orbit/2x2x2/nel5": (shared, ((2, 2, 2), 5, "class_orbit", "orbit", 1)),
})
STRIPED = [n for n in CASES if n.startswith("striped/")]
NO_BLOCKS = ["striped/class_orbit/2x2x2/nel5"]  # (the orbit storage holds only this rank's representatives: no block can be rebuilt from them)


def record(ctx, name, E):
    """What the file keeps of an assembled operator"""
    out = {"n_solves": int(E.assemble_stats()[0]), "n_gamma": [int(n) for n in E.n_gamma]}
    if name not in NO_BLOCKS:
        out["blocks"] = [_sha(E.block(b)[0]) for b in range(E.nblocks)]
    if name in STRIPED:
        lam = np.random.default_rng(6).standard_normal(E.B.n_lambda)
        y = ctx.vec(E.B.n_lambda)
        E.mult(ctx.vec_from(lam), y)
        assert np.any(y.to_numpy())
        out["mult"] = _sha(y.to_numpy())
    return out


def compute_case(ctx, name):
    fn, args = CASES[name]
    E, keep = fn(ctx, *args)
    out = record(ctx, name, E)
    del keep
    return out


def compute(names=None):
    import time

    pa = _pa()
    out = {}
    ctx = pa.Context(0)
    try:
        for name in names or CASES:
            t0 = time.time()
            out[name] = compute_case(ctx, name)
            print("%-40s %6d solves  %.1f s" % (name, out[name]["n_solves"], time.time() - t0), flush=True)
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
        write(fh, {"generator": "tests/golden/make_fx_assembly_bits.py", "commit": commit, "hipcc": hipcc[0]}, cases)
    print("wrote", a.out, len(cases), "cases")


if __name__ == "__main__":
    main()
