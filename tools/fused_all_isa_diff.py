#!/usr/bin/env python3
"""Are the instances of k_fused_all, k_fused_lone and k_fused_quad in two `hipcc -S` outputs of evc_fused_all.hip the
same, instruction for instruction?

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --offload-device-only -S exemplars_vc_amd/csrc/evc_fused_all.hip -o new.s
    python tools/fused_all_isa_diff.py parent.s new.s

Compares, per mangled name, the text from the kernel's label to its .Lfunc_end and its .amdhsa_kernel descriptor, with
block labels (.LBB<function>_<block>, also where the loop comments name them), .Lfunc_end<n>, .Ltmp<n> and __hip_cuid
lines normalised: the function's ordinal in the file is part of those and changes when a kernel is added.  Prints one
summary line per difference and the totals; exit status 1 if any instance differs or is missing.

An instance that differs is sorted into one of two kinds:
  order      the same instructions with the same operands in another order (s_waitcnt and s_nop set aside: they follow
             the order), the same descriptor - registers, scratch and LDS are what they were;
  registers  anything else; the line then gives VGPRs, AGPRs, scratch bytes per lane and the number of scratch
             instructions of both."""
import collections
import re
import sys

NAME = re.compile(r"^(_ZN3evc1[12]k_fused_(?:allILi\dELin?\d+ELb[01]E|(?:lone|quad)ILi\dELi\d+E)EEvNS_9FusedArgsE):", re.M)
FOLLOWS_ORDER = re.compile(r"^\s*(s_waitcnt|s_nop)\b")


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
        keep = lambda s: [l for l in s.split("\n") if "__hip_cuid" not in l]
        out[name] = (keep(body), keep(desc))
    return out


def resources(body, desc):
    d = "\n".join(desc)
    num = lambda key: int(re.search(key + r" (\d+)", d).group(1))
    return (num(r"\.amdhsa_next_free_vgpr"), num(r"\.amdhsa_accum_offset"),
            num(r"\.amdhsa_private_segment_fixed_size"), sum(1 for l in body if re.search(r"\bscratch_", l)))


def instructions(body):
    """the multiset of instruction lines (comments stripped), without those that merely follow the order"""
    out = collections.Counter()
    for l in body:
        l = l.split(";")[0].rstrip()
        if l.startswith("\t") and not l.lstrip().startswith(".") and not FOLLOWS_ORDER.match(l):
            out[l.strip()] += 1
    return out


def main(a, b):
    A, B = instances(a), instances(b)
    bad = order = 0
    for name in sorted(set(A) | set(B)):
        if name not in A or name not in B:
            print(f"{name}: only in {a if name in A else b}")
            bad += 1
        elif A[name] != B[name]:
            (ba, da), (bb, db) = A[name], B[name]
            la, lb = ba + da, bb + db
            n = sum(1 for x, y in zip(la, lb) if x != y) + abs(len(la) - len(lb))
            if da == db and instructions(ba) == instructions(bb):
                kind = "order"
                order += 1
            else:
                ra, rb = resources(ba, da), resources(bb, db)
                kind = "registers (vgpr+agpr, accum offset, scratch bytes, scratch instructions): %s -> %s" % (ra, rb)
            print(f"{name}: {len(la)} vs {len(lb)} lines, {n} differ: {kind}")
            bad += 1
    print(f"{len(A)} instances in {a}, {len(B)} in {b}, {sum(len(x) + len(y) for x, y in A.values())} lines compared: "
          f"{bad} instances differ, {order} of them in instruction order alone")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
