#!/usr/bin/env python3
"""Are the instances of k_fused_all in two `hipcc -S` outputs of evc_fused_all.hip the same, instruction for instruction?

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --offload-device-only -S exemplars_vc_amd/csrc/evc_fused_all.hip -o new.s
    python tools/fused_all_isa_diff.py parent.s new.s

Compares, per mangled name, the text from the kernel's label to its .Lfunc_end and its .amdhsa_kernel descriptor, with
block labels (.LBB<function>_<block>, also where the loop comments name them), .Lfunc_end<n>, .Ltmp<n> and __hip_cuid
lines normalised: the function's ordinal in the file is part of those and changes when a kernel is added.  Prints one
summary line per difference and the totals; exit status 1 if any instance differs or is missing."""
import re
import sys

NAME = re.compile(r"^(_ZN3evc11k_fused_allILi\dELin?\d+ELb[01]EEEvNS_9FusedArgsE):", re.M)


def instances(path):
    text = open(path).read()
    out = {}
    for m in NAME.finditer(text):
        name = m.group(1)
        end = text.index(".Lfunc_end", m.end())
        body = text[m.start():end]
        desc = re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\n(.*?)\.end_amdhsa_kernel", text, re.S).group(1)
        body = re.sub(r"BB\d+_(\d+)", r"BB_\1", body)
        body = re.sub(r"\.L(tmp|func_begin|func_end)\d+", r".L\1", body)
        lines = [l for l in (body + desc).split("\n") if "__hip_cuid" not in l]
        out[name] = lines
    return out


def main(a, b):
    A, B = instances(a), instances(b)
    bad = 0
    for name in sorted(set(A) | set(B)):
        if name not in A or name not in B:
            print(f"{name}: only in {a if name in A else b}")
            bad += 1
        elif A[name] != B[name]:
            n = sum(1 for x, y in zip(A[name], B[name]) if x != y) + abs(len(A[name]) - len(B[name]))
            print(f"{name}: {len(A[name])} vs {len(B[name])} lines, {n} differ")
            bad += 1
    print(f"{len(A)} instances in {a}, {len(B)} in {b}, {sum(len(v) for v in A.values())} lines compared: "
          f"{bad} instances differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
