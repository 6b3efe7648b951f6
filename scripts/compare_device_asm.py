#!/usr/bin/env python3
"""Compare the device assembly of two builds of one translation unit, function by function.

    hipcc <product flags> --cuda-device-only -S unit.hip -o a.s      (once per build)
    python scripts/compare_device_asm.py a.s b.s

A refactor that moves kernels between files may reorder them, and the compiler numbers its local labels by
the function's position in the unit.  So: every function (kernel or not) is cut out with its kernel descriptor and
its resource summary, the per-function index in local labels (.LBB<n>_, .Lfunc_end<n>, BB<n>_ in comments) is
normalised (with the padding in front of a label's comment, which follows the label's width), and the bodies are
compared name by name.  What is left of the file (header, metadata, trailer) must be
equal as a multiset of lines; lines naming the per-compilation __hip_cuid_ symbol are dropped.

Prints the kernel count of each file and every function that is missing or differs; exits 1 if anything does.
"""
import collections
import re
import sys

BEGIN = re.compile(r"^\t\.(globl|protected|weak|hidden|p2align)\t([^;]+); -- Begin function (\S+)")
LOCAL = re.compile(r"(\.LBB|\.Lfunc_end|\.Lfunc_begin|\bBB)\d+")
LABEL_PAD = re.compile(r"^(\.LBB#_\d+:)\s+;")


def split(path):
    lines = [l for l in open(path).read().split("\n") if "__hip_cuid_" not in l]
    starts = []
    for i, l in enumerate(lines):
        m = BEGIN.match(l)
        if m:
            first = i - 1 if i > 0 and lines[i - 1].startswith("\t.section\t.text") else i
            starts.append((first, m.group(3)))
    funcs, rest = {}, list(lines[: starts[0][0]] if starts else lines)
    for k, (first, name) in enumerate(starts):
        if k + 1 < len(starts):
            end = starts[k + 1][0]
        else:  # the last function ends behind its resource summary: at the first directive after "; -- End function"
            end = first
            while end < len(lines) and "-- End function" not in lines[end]:
                end += 1
            while end < len(lines) and (lines[end].startswith((";", "\t.set ", "\t.section\t.AMDGPU.csdata")) or
                                        "-- End function" in lines[end]):
                end += 1
        if name in funcs:
            sys.exit(f"{path}: function {name} appears twice")
        funcs[name] = [LABEL_PAD.sub(r"\1 ;", LOCAL.sub(lambda m: m.group(1) + "#", l)) for l in lines[first:end]]
        if k + 1 == len(starts):
            rest += lines[end:]
    kernels = sum(1 for l in lines if l.lstrip().startswith(".amdhsa_kernel "))
    return funcs, collections.Counter(rest), kernels


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    (fa, ra, ka), (fb, rb, kb) = split(sys.argv[1]), split(sys.argv[2])
    print(f"{sys.argv[1]}: {ka} kernels, {len(fa)} functions")
    print(f"{sys.argv[2]}: {kb} kernels, {len(fb)} functions")
    bad = 0
    for name in sorted(set(fa) | set(fb)):
        if name not in fa or name not in fb:
            print(f"only in {sys.argv[2] if name in fb else sys.argv[1]}: {name}")
            bad += 1
        elif fa[name] != fb[name]:
            n = next((i for i, (x, y) in enumerate(zip(fa[name], fb[name])) if x != y), min(len(fa[name]), len(fb[name])))
            print(f"differs: {name} ({len(fa[name])} / {len(fb[name])} lines, first difference at line {n} of the function)")
            bad += 1
    if ra != rb:
        only_a, only_b = ra - rb, rb - ra
        print(f"outside the functions: {sum(only_a.values())} lines only in the first file, {sum(only_b.values())} only in the second")
        for l in list(only_a)[:5]:
            print("  - " + l)
        for l in list(only_b)[:5]:
            print("  + " + l)
        bad += 1
    print("identical" if not bad else f"{bad} difference(s)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
