#!/usr/bin/env python3
"""Per-kernel comparison of two device assemblies of fmm.hip / fmg.hip (hipcc -O3 -std=c++17 -fPIC
--offload-arch=gfx950 --cuda-device-only -S -x hip): the instruction stream and the .amdhsa_
resource block of every kernel, after dropping comments, renumbering local labels by function
and cutting the compile-unit hash out of symbol names.

    fm_isa_equal.py PARENT_DIR THIS_DIR     (each holds fmm.s and fmg.s)

fm_isa_equal.txt is its output for the commit that moved the two files' shared code into
csrc/fm_dev.h against the commit before it, with a note on the one kernel that differs."""
import re
import subprocess
import sys


def kernels(path):
    """{demangled kernel name: (instruction lines, .amdhsa_ lines)}"""
    text = open(path).read()
    text = re.sub(r"\.intern\.[0-9a-f]+|\.hip\.[0-9a-f]+|__hip_cuid_[0-9a-f]+", "", text)
    body, hsa, cur, in_hsa = {}, {}, None, None
    for line in text.splitlines():
        line = line.split(";")[0].rstrip()
        s = line.strip()
        if not s:
            continue
        m = re.match(r"^(_Z\w+):$", s)
        if m and "k_fm" in m.group(1):
            cur = m.group(1)
            body[cur] = []
            continue
        if s.startswith(".Lfunc_end"):
            cur = None
        if s.startswith(".amdhsa_kernel "):
            in_hsa = s.split()[1]
            hsa[in_hsa] = []
            continue
        if s == ".end_amdhsa_kernel":
            in_hsa = None
        if in_hsa:
            hsa[in_hsa].append(s)
        elif cur and not s.startswith(".") or cur and re.match(r"^\.LBB\d+_\d+:", s):
            body[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    names = sorted(body)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return {d.replace("(anonymous namespace)::", ""): (body[n], hsa[n]) for n, d in zip(names, dem)}


def main():
    parent, this = sys.argv[1], sys.argv[2]
    bad = total = 0
    print("%-8s %-60s %6s  %s" % ("file", "kernel", "instrs", "against the parent commit"))
    for f in ("fmm", "fmg"):
        a, b = kernels("%s/%s.s" % (parent, f)), kernels("%s/%s.s" % (this, f))
        for k in sorted(set(a) | set(b)):
            if k not in a or k not in b:
                verdict = "only in " + ("parent" if k in a else "this")
            elif a[k] == b[k]:
                verdict = "equal"
            else:
                verdict = "NOT equal: instructions %s, resource block %s" % tuple(
                    "equal" if a[k][i] == b[k][i] else "differ" for i in (0, 1))
            bad += verdict != "equal"
            total += 1
            n = len([l for l in (b.get(k) or a[k])[0] if not l.endswith(":")])
            print("%-8s %-60s %6d  %s" % (f + ".hip", re.sub(r"^void sbmf::|\(.*$", "", k), n, verdict))
    print("%d of %d kernels differ" % (bad, total))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
