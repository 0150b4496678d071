"""pmh_feti_contact_solve's K^+ choice (explicit_dual = PMH_KPLUS_AUTO) against the two forced paths: set-up, solve and time to solution of one default contact solve,
the probe's estimates next to them, and the F applications the solve took.
usage: python scripts/kplus_auto.py CASE [CASE ...] [--paths auto,iterative,explicit] [--out FILE]
  CASE: c2 (configs[2]: 2 x 2 x 2 boxes of 43^3 elements, orbit storage), stair21 / stair43 (the staircase cut of permon_amd.feti.irregular_partition at 21^3 / 43^3 scale).
The set-up stages and the probe's line (its CG iterations per K^+ among them) go to stderr (PMH_CONTACT_TIMING=1)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import permon_amd as pa  # noqa: E402
from permon_amd import feti  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("cases", nargs="+", choices=["c2", "stair21", "stair43"])
ap.add_argument("--paths", default="auto,iterative,explicit")
ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
a = ap.parse_args()
os.environ.setdefault("PMH_CONTACT_TIMING", "1")

ctx = pa.Context(0)
for case in a.cases:
    t = time.perf_counter()
    if case == "c2":
        f, kw = pa.CubeFeti((2, 2, 2), 43, contact=True), dict(explicit_storage="class_orbit")
    else:
        f, kw = feti.MeshFeti(feti.irregular_partition(int(case[5:]), "staircase"), contact=True), dict(dims=None)
    build = time.perf_counter() - t
    for path in a.paths.split(","):
        explicit = {"auto": "auto", "iterative": False, "explicit": True}[path]
        print("---- %s %s" % (case, path), file=sys.stderr, flush=True)
        t = time.perf_counter()
        u, lam, st = pa.FETIContactSolve(ctx, f, explicit=explicit, **kw)
        wall = time.perf_counter() - t
        s = st.smalxe
        rec = {"case": case, "path": path, "N": int(f.N), "n_lambda": int(f.n_lambda), "problem_build_s": round(build, 2), "kplus_path": ["iterative", "explicit"][st.kplus_path],
               "setup_s": round(st.setup_seconds, 3), "solve_s": round(st.solve_seconds, 3), "time_to_solution_s": round(st.setup_seconds + st.solve_seconds, 3),
               "wall_s_incl_upload": round(wall, 3), "explicit_assembly_s": round(st.explicit_seconds, 3), "explicit_solves": int(st.explicit_solves),
               "setup_solves_planned": int(st.setup_solves_planned), "f_applies": int(st.f_applies), "outer": int(s.iteration), "inner": int(s.inner_iter_accu), "reason": int(s.reason),
               "norm_Glambda_minus_e": st.norm_Glambda_minus_e}
        if st.kplus_auto:
            rec.update({"expected_applies_used": st.expected_applies_used, "est_explicit_s": round(st.est_explicit_seconds, 3), "est_iterative_s": round(st.est_iterative_seconds, 3),
                        "probe_s": round(st.probe_seconds, 3)})
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(line + "\n")
ctx.close()
