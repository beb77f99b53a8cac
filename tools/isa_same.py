#!/usr/bin/env python3
"""Do two builds of one source file compile to the same kernels?

    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-result -S --cuda-device-only \\
        acids_transforms_amd/csrc/stft2048.hip -o /tmp/new.s          (the Makefile's flags; the same for the other tree)
    python tools/isa_same.py /tmp/old.s /tmp/new.s

For every kernel of the two listings compares the sequence of instruction mnemonics (operands, and so register numbers
and argument offsets, are left out), the VGPR and SGPR counts and the scratch size, prints `same` or `differ` per kernel
with the first differing span, and exits non-zero on any difference or on a kernel that only one listing has.  Kernels
are matched by their demangled name without the parameter list (c++filt), so that renaming an argument struct does not
hide a kernel from the comparison.  What a refactor of kernel code has to show before anything is timed: the same
listing needs no A/B."""
import difflib
import re
import subprocess
import sys

COUNTS = ("num_vgpr", "numbered_sgpr", "private_seg_size")


def kernels(path):
    """{demangled name without parameters: (mnemonics, {count: value})} of a hipcc -S listing."""
    lines = open(path).read().split("\n")
    is_kernel = {l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")}
    ops, counts = {}, {}
    i = 0
    while i < len(lines):
        m = re.match(r"^(\w+):", lines[i])
        if m and m.group(1) in is_kernel:
            body = ops.setdefault(m.group(1), [])
            i += 1
            while not lines[i].startswith(".Lfunc_end"):
                l = lines[i].strip()
                if l and not l.startswith((";", ".", "//")) and not re.match(r"^[\w.$]+:", l):
                    body.append(l.split()[0])
                i += 1
        m = re.match(r"^\s*\.set (\w+)\.(\w+), (\S+)$", lines[i])
        if m and m.group(1) in is_kernel and m.group(2) in COUNTS:
            counts.setdefault(m.group(1), {})[m.group(2)] = m.group(3)
        i += 1
    syms = sorted(ops)
    plain = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True, check=True).stdout.split("\n")
    out = {}
    for sym, name in zip(syms, plain):
        name = name[:name.rindex("(")] if name.endswith(")") else name
        assert name not in out, name
        out[name] = (ops[sym], counts.get(sym, {}))
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print("differ  %s: only in %s" % (name, sys.argv[1] if name in a else sys.argv[2]))
            bad += 1
            continue
        (oa, ca), (ob, cb) = a[name], b[name]
        why = ["%s %s -> %s" % (k, ca.get(k), cb.get(k)) for k in COUNTS if ca.get(k) != cb.get(k)]
        if oa != ob:
            _, i1, i2, j1, j2 = next(o for o in difflib.SequenceMatcher(None, oa, ob, autojunk=False).get_opcodes()
                                     if o[0] != "equal")
            why.append("%d -> %d instructions, first at %d: [%s] -> [%s]"
                       % (len(oa), len(ob), i1, " ".join(oa[i1:i2][:8]), " ".join(ob[j1:j2][:8])))
        print("%-7s %s (%d instructions, %s VGPRs)%s" % ("differ" if why else "same", name, len(ob), cb.get("num_vgpr"),
                                                          "".join("\n        " + w for w in why)))
        bad += bool(why)
    print("%d kernels, %d differ" % (len(set(a) | set(b)), bad))
    sys.exit(1 if bad or not a else 0)


if __name__ == "__main__":
    main()
