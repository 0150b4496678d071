#!/usr/bin/env python3
"""Kernel names of a launch list (scripts/dev/kernel_order.py list) taken AFTER the V-cycle's transfer kernels became two templates, spelled as they were before, so
that `kernel_order.py compare` can hold the list against one taken before:

    python scripts/dev/mg_transfer_names.py after.txt > after_old_names.txt

Instances of k_mg_restrict<TV, R, NC, G, ASC> / k_mg_prolong_sub<TV, R, NC, G> -> the ten kernels of mg.hip and mg_mv.hip; k_extract_dinv<TV> -> k_mg_dinv<TV> (right
for a process that builds hierarchies and no MATINV solver, such as tests/test_gpu_mg_paths.py: the solver's own k_extract_dinv had no template argument);
pmh_bsr3_epi in the signature of k_mv_spmv -> pmh_mv_epi (one struct now)."""
import gzip
import re
import sys

ARGS_R = "(int, int const*, int const*, int const*, {t} const*, {t} const*, {t}*, {t} const*, {t}, {t}*)"
ARGS_P = "(int, int const*, int const*, int const*, {t} const*, {t} const*, {t}*)"
ONE = {("restrict", "1, 1, 8, 0"): "k_mg_restrict", ("restrict", "1, 1, 64, 0"): "k_mg_restrict_w", ("restrict", "1, 3, 8, 0"): "k_mg_restrict3",
       ("prolong_sub", "1, 1, 1"): "k_mg_prolong_sub", ("prolong_sub", "1, 1, 8"): "k_mg_prolong_sub8", ("prolong_sub", "1, 3, 1"): "k_mg_prolong_sub3"}
EIGHT = {("restrict", "8, 3, 4, 1"): "k_mvg_restrict", ("restrict", "8, 1, 8, 1"): "k_mvg_restrict_s", ("prolong_sub", "8, 3, 1"): "k_mvg_prolong_sub",
         ("prolong_sub", "8, 1, 1"): "k_mvg_prolong_sub_s"}


def old_name(name):
    m = re.match(r"void k_mg_(restrict|prolong_sub)<(float|double), ([0-9, ]+)>\(", name)
    if m:
        what, t, inst = m.groups()
        args = (ARGS_R if what == "restrict" else ARGS_P).format(t=t)
        if (what, inst) in ONE:
            return "void %s<%s>%s" % (ONE[(what, inst)], t, args)
        return EIGHT[(what, inst)] + args
    m = re.match(r"void k_extract_dinv<(float|double)>\(int, int const\*, int const\*, double const\*, int, (float|double)\*\)", name)
    if m:
        return "void k_mg_dinv<%s>(int, int const*, int const*, double const*, %s*)" % (m.group(1), m.group(2))
    if name.startswith("void k_mv_spmv<"):
        return name.replace("pmh_bsr3_epi<", "pmh_mv_epi<")
    if name.startswith("_Z9k_mv_spmv"):
        return name.replace("12pmh_bsr3_epiI", "10pmh_mv_epiI")
    return name


def main():
    path = sys.argv[1]
    with (gzip.open(path, "rt") if path.endswith(".gz") else open(path)) as f:
        lines = f.read().splitlines()
    for line in lines:
        name, rest = line.split("\t", 1)
        print(old_name(name) + "\t" + rest)


if __name__ == "__main__":
    main()
