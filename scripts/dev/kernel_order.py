#!/usr/bin/env python3
"""The ordered launch list of one traced process, for a host-side refactor that must neither add, drop nor reorder a launch:

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python -m pytest ...      (a run of its own, once per build)
    python scripts/dev/kernel_order.py list OUT/**/*_kernel_trace.csv > before.txt    one line per dispatch, in dispatch order: name grid workgroup
    python scripts/dev/kernel_order.py compare before.txt after.txt                   exit status 1 and the first differing lines unless equal line for line
    python scripts/dev/kernel_order.py digest before.txt                              "<count> <sha256>": what profiles/ keeps where the list itself is too long
    (compare and digest also read a list that went through gzip, by its name: before.txt.gz)

Grid and workgroup size are the three extents each, as the trace gives them.  Dispatches are ordered by their dispatch id (the order in which the process enqueued
them), not by start time: two streams may overlap on the device."""
import csv
import gzip
import hashlib
import sys


def lines_of(path):
    """The lines of a list written by `list`, plain or gzipped (a test process launches millions of kernels)"""
    with (gzip.open(path, "rt") if path.endswith(".gz") else open(path)) as f:
        return f.read().splitlines()


def rows(path):
    out = []
    for r in csv.DictReader(open(path)):
        grid = "x".join(r[k] for k in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z")) if "Grid_Size_X" in r else r["Grid_Size"]
        wg = "x".join(r[k] for k in ("Workgroup_Size_X", "Workgroup_Size_Y", "Workgroup_Size_Z")) if "Workgroup_Size_X" in r else r["Workgroup_Size"]
        out.append((int(r["Dispatch_Id"]), "%s\t%s\t%s" % (r["Kernel_Name"], grid, wg)))
    return [line for _, line in sorted(out)]


def main():
    cmd, files = sys.argv[1], sys.argv[2:]
    if cmd == "list":
        for f in files:
            print("\n".join(rows(f)))
    elif cmd == "digest":
        lines = lines_of(files[0])
        print(len(lines), hashlib.sha256("\n".join(lines).encode()).hexdigest())
    elif cmd == "compare":
        a, b = [lines_of(f) for f in files]
        bad = [i for i in range(min(len(a), len(b))) if a[i] != b[i]]
        print("%d launches before, %d after, %d lines differ%s" % (len(a), len(b), len(bad), "" if len(a) == len(b) else ", the lengths differ"))
        for i in bad[:10]:
            print("line %d\n  before %s\n  after  %s" % (i + 1, a[i], b[i]))
        sys.exit(1 if bad or len(a) != len(b) else 0)
    else:
        sys.exit(__doc__)


if __name__ == "__main__":
    main()
