#!/usr/bin/env python3
"""Which kernels of a translation unit did a source change move?  Splits two assembly files (hipcc <the Makefile's flags>
--cuda-device-only -S) by kernel symbol and compares the bodies as text.

    hipcc <flags> --cuda-device-only -S csrc/cf_mbconv3.hip -o new.s          # and the same for the parent commit -> old.s
    python tools/asm_kernel_diff.py old.s new.s [--md]

A body is every line from the symbol's label to its .Lfunc_end, comments and blank lines dropped.  Prints one line per kernel
(demangled through c++filt when it is there): `identical`, `differs` with the instruction counts of both, `only in old` / `only in new`.
Exit status 1 when anything differs.  Text only: resources and loop counts are tools/isa_loop_counts.py's and the compiler remarks'.
"""
import argparse
import collections
import re
import shutil
import subprocess
import sys


def bodies(path):
    out, name = collections.OrderedDict(), None
    lines = open(path).read().splitlines()
    funcs = {m.group(1) for m in (re.match(r"^\s*\.type\s+(_Z\w+),@function", l) for l in lines) if m}
    for line in lines:
        s = line.split(";", 1)[0].rstrip()
        if name is None:
            m = re.match(r"^(_Z\w+):", s)
            if m and m.group(1) in funcs:
                name = m.group(1)
                out[name] = []
            continue
        if s.strip().startswith(".Lfunc_end"):
            name = None
            continue
        if s.strip():
            out[name].append(s.strip())
    return out


def demangle(names):
    if not names or not shutil.which("c++filt"):
        return dict(zip(names, names))
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return dict(zip(names, r.stdout.splitlines()))


def instructions(body):
    return sum(1 for s in body if not s.startswith(".") and not s.endswith(":"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--md", action="store_true", help="markdown table rows")
    a = ap.parse_args()
    old, new = bodies(a.old), bodies(a.new)
    names = list(old) + [n for n in new if n not in old]
    pretty = demangle(names)
    moved = 0
    for n in names:
        if n not in new:
            verdict = "only in old"
        elif n not in old:
            verdict = "only in new"
        elif old[n] == new[n]:
            verdict = "identical"
        else:
            verdict = "differs (%d -> %d instructions)" % (instructions(old[n]), instructions(new[n]))
        moved += verdict != "identical"
        short = pretty[n].replace("void cf::", "").replace("(cf::MbParams)", "").replace("(cf::Stem0Params)", "")
        print(("| `%s` | %s |" if a.md else "%-90s %s") % (short, verdict))
    print("%s%d kernels, %d not identical" % ("\n" if a.md else "", len(names), moved))
    return 1 if moved else 0


if __name__ == "__main__":
    sys.exit(main())
