#!/usr/bin/env python3
"""Compare two gfx950 assembly listings kernel by kernel (a one-off check of a refactor that must leave the generated code alone):

    hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S svm.hip -o before/svm.s     (at the parent, then at the head -> after/svm.s)
    python scripts/dev/svm_isa_diff.py before/svm.s after/svm.s

Per kernel: the instructions only, comments stripped, assembler directives dropped, local labels renamed in order of appearance.  Prints one line per kernel:
"identical", or the register counts, scratch size, floating-point instruction count and instruction count of both sides and a unified diff with -v."""
import difflib
import re
import subprocess
import sys

LABEL = re.compile(r"^([A-Za-z_][\w$.]*):")
LOCAL = re.compile(r"\.L[\w$]+")
META = re.compile(r";\s*(NumVgprs|TotalNumSgprs|ScratchSize|NumAgprs):\s*(\d+)")
FP = re.compile(r"^\w+_f(16|32|64)\b")


def kernels(path):
    out, name, body, meta, seen = {}, None, None, None, None
    for raw in open(path):
        m = LABEL.match(raw)
        if m and not m.group(1).startswith(".L") and name is None and raw.split(";")[0].strip().endswith(":"):
            name, body, meta, seen = m.group(1), [], {}, {}
            continue
        if name is None:
            continue
        mm = META.search(raw)
        if mm:
            meta[mm.group(1)] = int(mm.group(2))
            if mm.group(1) == "ScratchSize":
                out[name] = (body, meta)
                name = None
            continue
        line = raw.split(";")[0].strip()
        if not line or (line.startswith(".") and not line.startswith(".L")):
            continue
        line = LOCAL.sub(lambda x: seen.setdefault(x.group(0), "L%d" % len(seen)), line)
        if not meta and ".Lfunc_end" not in raw:
            body.append(line)
    return out


def demangle(names):
    try:
        return dict(zip(names, subprocess.check_output(["c++filt"] + names, text=True).splitlines()))
    except Exception:
        return {n: n for n in names}


KERNEL = re.compile(r"^(?:void )?(\w+)(?:<([^()]*)>)?(?=\()")


def drop_sample_type(name):
    """The kernel's name without a trailing template argument `double` (the sample type the dense SVM kernels gained) and without the return type a
    template's demangled name carries: k_svm_xt<0, 0, double>(...) and k_svm_predict<double>(...) pair up with k_svm_xt<0, 0>(...) and k_svm_predict(...)."""
    m = KERNEL.match(name)
    if not m:
        return name
    args = [t for t in (m.group(2) or "").split(", ") if t]
    if args and args[-1] == "double":
        args.pop()
    return m.group(1) + ("<%s>" % ", ".join(args) if args else "") + name[m.end():]


def main():
    verbose = "-v" in sys.argv
    a, b = [kernels(p) for p in sys.argv[1:] if p != "-v"]
    dm = demangle(sorted(set(a) | set(b)))
    # pair the kernels up by their demangled names less the sample type
    a, b = [{drop_sample_type(dm[k]): v for k, v in side.items()} for side in (a, b)]
    dm = {k: k for k in set(a) | set(b)}
    same = 0
    for k in sorted(set(a) | set(b), key=lambda k: dm[k]):
        if k not in a or k not in b:
            print("ONLY %s: %s" % ("before" if k in a else "after", dm[k]))
            continue
        (ia, ma), (ib, mb) = a[k], b[k]
        if ia == ib:
            same += 1
            print("identical  %s" % dm[k])
            continue
        fa, fb = sum(1 for l in ia if FP.match(l)), sum(1 for l in ib if FP.match(l))
        print("DIFFERS    %s\n           before %s fp %d instructions %d\n           after  %s fp %d instructions %d" % (dm[k], ma, fa, len(ia), mb, fb, len(ib)))
        if verbose:
            print("\n".join(difflib.unified_diff(ia, ib, lineterm="", n=2)))
    print("%d kernels before, %d after, %d identical" % (len(a), len(b), same))


if __name__ == "__main__":
    main()
