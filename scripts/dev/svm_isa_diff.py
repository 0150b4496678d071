#!/usr/bin/env python3
"""Compare two gfx950 assembly listings kernel by kernel (a one-off check of a refactor that must leave the generated code alone):

    hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S svm.hip -o before/svm.s     (at the parent, then at the head -> after/svm.s)
    python scripts/dev/svm_isa_diff.py before/svm.s after/svm.s [--pair OLD=NEW ...] [-v]

--pair OLD=NEW compares the kernel that was OLD before with the kernel that is NEW after, both given as the demangled name up to its argument list and
without the return type: --pair 'k_svm_predict64<float>=k_svm_rows64<float, svm_classify_f>'.  Both listings may be concatenations of several files' output.

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
        if m and not m.group(1).startswith(".L") and raw.split(";")[0].strip().endswith(":"):  # (also after a symbol that is no kernel, as between concatenated listings)
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


def kernel_id(name):
    """The demangled name up to its argument list, without the return type: what --pair names a kernel by."""
    return re.sub(r"^void ", "", name).split("(")[0]


def main():
    args = sys.argv[1:]
    verbose = "-v" in args
    pairs = dict(args[i + 1].split("=", 1) for i, x in enumerate(args) if x == "--pair")
    files = [x for i, x in enumerate(args) if x not in ("-v", "--pair") and (i == 0 or args[i - 1] != "--pair")]
    a, b = [kernels(p) for p in files]
    dm = demangle(sorted(set(a) | set(b)))
    # a renamed kernel takes its new name on the before side (--pair)
    new = {kernel_id(dm[k]): dm[k] for k in b}
    for old, to in pairs.items():
        hit = [k for k in a if kernel_id(dm[k]) == old]
        if len(hit) != 1 or to not in new:
            sys.exit("--pair %s=%s: %s" % (old, to, "no such kernel after" if len(hit) == 1 else "%d kernels of that name before" % len(hit)))
        key = new[to] + " [was %s]" % old
        a[key], b[key], dm[key] = a.pop(hit[0]), b.pop([k for k in b if dm[k] == new[to]][0]), key
    # pair the other kernels up by their demangled names less the sample type
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
