"""k_fused_quad (evc_fused_all.hip + evc_fused_all_body.inc with EVC_ALL_LONE 2), without a GPU.

k_fused_lone at M = 25 but for the sweep's V' += A_j H'_j: bins 0 .. 15 keep their four v_mfma_f64_16x16x4_f64, bins
16 .. 24 - 9 real rows of a 16-row tile - run on twelve v_mfma_f64_4x4x4_4b_f64: three bin blocks of four (16 .. 19,
20 .. 23, 24 and three zero slots) x the four exemplar registers.  The instruction's operand map, measured by
tools/ubench/mfma64_quad.hip (profiles/quad_rows_ubench.txt):
    A[i][k] of block b in lane i + 4 b + 16 k,  B[k][j] in lane j + 4 b + 16 k,  D[i][j] in lane j + 4 b + 16 i,
and cbsz / abid are ignored by the f64 form, so that the A fragment is read replicated over the four blocks: aq[beta][r],
twelve ds_read_b64 per unit (lanes l, l + 4, l + 8, l + 12 share an address), not three with a broadcast.

* The fragment map on the LDS image helpers of tests/test_fused_all_lds_host.py: for every lane, beta, r and tile the
  word read is A[bin][exemplar] of the streamed A2p, 0 for bins past 24, and the address stays in its row.
* The twelve reads are free of bank conflicts under that file's ds_read_b64 model (at most 2-way was the requirement).
* A numpy restatement on integer-valued data: ten 16x16x4 k-steps' worth of V' for bins 0 .. 15 plus twelve block products
  laid out by the map above equal the 14-MFMA unit's V', exactly, and land in the exchange image's slots 4 .. 6.
* The code object of the three instances.
"""
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_fused_all_lds_host import (AKT, ATILES, AW, LDS_BYTES, bin_of, conflicts, lane_rows, lds_image, mfma_runs,  # noqa: E402
                                     packed, shape)
from test_fused_all_lds_host import device_asm  # noqa: E402,F401  (the module-scoped fixture: one compilation)
from test_fused_step_chain_host import VECTOR, check_sweep  # noqa: E402

M, MS, MT = 25, 7, 2
DS = MS - 1                      # k-steps of the D and P chains (the lone bin is folded, as in k_fused_lone)
NQ = MS - 4                      # bin blocks of four on the small MFMAs
BL = 24                          # the last block's only real bin
LARGE, SMALL = DS + 4, 4 * NQ    # MFMAs per unit


def quad_addr(w, lane, k, beta, r, pr):
    """the kernel's dQ[k * TPD + r * PR + 4 beta] (beta < NQ - 1) and dQL[k * TPD + r * PR]"""
    rowB = lane_rows(w, lane, MS, M, pr)[2] - (lane & 15)
    base = rowB + 16 + (lane & 3) + 4 * beta if beta < NQ - 1 else rowB + min(BL + (lane & 3), M)
    return base + k * 16 * pr + r * pr


def test_the_fragment_map():
    rng = np.random.default_rng(25)
    pr = shape(MS, 2, False)[0]
    assert pr == 26
    members, N = 2, 2 * 512 - 7
    NT = members * ATILES
    A = rng.random((M, N)) + 0.5
    _, A2p = packed(A, NT, MS, MT)
    Apad = np.zeros((M + 3, NT * 16))
    Apad[:M, :N] = A
    for member in range(members):
        img = lds_image(A2p, member, MS, M, pr)
        for w in range(AW):
            for lane in range(64):
                for k in range(AKT):
                    j = member * ATILES + w + AW * k
                    slot = w * AKT + k
                    for beta in range(NQ):
                        for r in range(4):
                            x = quad_addr(w, lane, k, beta, r, pr)
                            b, e = 16 + 4 * beta + (lane & 3), 4 * (lane >> 4) + r
                            assert x // (16 * pr) == slot, (w, lane, k, beta, r)             # the unit's tile
                            assert x % pr == min(b, M), (w, lane, k, beta, r)                # the bin, or the zero slot
                            assert img[x] == Apad[b, 16 * j + e], (member, w, lane, k, beta, r)
                            # the row is exemplar e's: bin 0 of that row is what the V' fragment of bin 0 reads there
                            assert img[x - x % pr] == Apad[0, 16 * j + e]


def test_the_twelve_reads_are_free_of_bank_conflicts():
    pr = shape(MS, 2, False)[0]
    worst = 0
    for w in range(AW):
        for k in range(AKT):
            for beta in range(NQ):
                for r in range(4):
                    worst = max(worst, conflicts([quad_addr(w, lane, k, beta, r, pr) for lane in range(64)]))
    assert worst == 0


def test_ten_large_k_steps_and_twelve_block_products_are_the_14_mfma_unit():
    """integer-valued operands: every sum is exact.  One unit: exemplar tile A [M][16], activations H [16 exemplars][16
    frames]; register r of lane l holds exemplar 4 (l >> 4) + r of frame l & 15"""
    rng = np.random.default_rng(4)
    A = rng.integers(0, 9, (M, 16)).astype(np.float64)
    H = rng.integers(0, 9, (16, 16)).astype(np.float64)
    want = A @ H                                                     # V' [bin][frame]
    h = np.array([[H[4 * (l >> 4) + r, l & 15] for l in range(64)] for r in range(4)])
    # the 14-MFMA unit's second tile: accumulator register rho of lane l = V'[16 + 4 rho + (l >> 4)][l & 15]
    image = np.zeros((8, 64))
    for s in range(4):                                               # bins 0 .. 15: the first tile, unchanged
        for l in range(64):
            image[s, l] = want[bin_of(s, l >> 4), l & 15]
    # the twelve small MFMAs, by the measured operand map
    for beta in range(NQ):
        acc = np.zeros(64)
        for r in range(4):
            aq = np.array([A[16 + 4 * beta + (l & 3), 4 * (l >> 4) + r] if 16 + 4 * beta + (l & 3) < M else 0.0
                           for l in range(64)])
            d = np.zeros(64)
            for blk in range(4):
                for i in range(4):
                    for j in range(4):
                        d[j + 4 * blk + 16 * i] = sum(aq[i + 4 * blk + 16 * kk] * h[r][j + 4 * blk + 16 * kk] for kk in range(4))
            acc += d
        image[4 + beta] = acc
    for s in range(MS):
        for l in range(64):
            b = bin_of(s, l >> 4)
            assert image[s, l] == (want[b, l & 15] if b < M else 0.0), (s, l)
    assert [bin_of(4 + beta, q) for beta in range(NQ) for q in range(4)] == list(range(16, 28))


# ---------------------------------------------------------------------------------------------------------------------
# the code object


def quad_kernels(asm, kernel="quad"):
    for m in re.finditer(r"^(_ZN3evc12k_fused_" + kernel + r"ILi(\d)ELi(\d+)EEEvNS_9FusedArgsE):[^\n]*\n(.*?)s_endpgm", asm,
                         re.S | re.M):
        name, ms, c, body = m.group(1), int(m.group(2)), int(m.group(3)), m.group(4)
        desc = re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\n(.*?)\.end_amdhsa_kernel", asm, re.S).group(1)
        num = lambda key: int(re.search(key + r" (\d+)", desc).group(1))
        yield ms, c, body.split("\n"), {"group": num(r"\.amdhsa_group_segment_fixed_size"), "vgpr": num(r"\.amdhsa_next_free_vgpr"),
                                        "scratch": num(r"\.amdhsa_private_segment_fixed_size")}


def longest_nop(lines):
    return max([int(m.group(1)) for l in lines for m in [re.match(r"\s+s_nop (\d+)", l)] if m] + [-1])


def test_code_object_of_the_three_instances(device_asm):  # noqa: F811
    seen = []
    sweep, numerator, y_pass = AKT * (LARGE + SMALL), AKT * DS, AKT * 4 * (MT + 1)
    lone = {c: (lines, res) for _, c, lines, res in quad_kernels(device_asm, "lone")}
    for ms, c, lines, res in quad_kernels(device_asm):
        seen.append((ms, c))
        pr, on, rest = shape(ms, c, False)
        assert on and res["group"] <= LDS_BYTES and res["group"] == lone[c][1]["group"], (c, res)
        # two wavefronts per SIMD (512 registers per lane and SIMD), scratch no higher than k_fused_lone<7, C>'s
        assert res["vgpr"] <= 256 and res["scratch"] <= lone[c][1]["scratch"], (c, res, lone[c][1])
        runs = mfma_runs(lines)
        sizes = sorted(len(r) for r in runs)
        assert sum(sizes) == numerator + sweep + y_pass, (c, sizes)
        assert sizes.count(sweep) == 1 and sizes.count(numerator) == 1, (c, sizes)
        idx = next(r for r in runs if len(r) == sweep)
        seg = lines[idx[0]:idx[-1] + 1]
        large = [l for l in seg if "v_mfma_f64_16x16x4" in l]
        small = [l for l in seg if "v_mfma_f64_4x4x4" in l]
        assert (len(large), len(small)) == (AKT * LARGE, AKT * SMALL), c
        # the f64 form ignores cbsz / abid (profiles/quad_rows_ubench.txt): none is set, the fragments come replicated
        assert not any(re.search(r"cbsz|abid|blgp", l) for l in small), c
        # per unit: ten large and twelve small between two vector phases
        assert len(check_sweep(lines, idx, ("k_fused_quad", ms, c))) == AKT
        cuts = [i for i, (a, b) in enumerate(zip(idx, idx[1:])) if any(VECTOR.match(l) for l in lines[a + 1:b])]
        units = [idx[a + 1:b + 1] for a, b in zip([-1] + cuts, cuts + [len(idx) - 1])]
        # (the first stretch is unit 0's D chain, the last unit 7's V': AKT + 1 stretches, D of unit k + 1 behind V' of unit k)
        assert [len(u) for u in units] == [DS] + [4 + SMALL + DS] * (AKT - 1) + [4 + SMALL], (c, [len(u) for u in units])
        for u in units[1:]:
            names = ["S" if "4x4x4" in lines[i] else "L" for i in u]
            assert names.count("S") == SMALL and names.count("L") == len(u) - SMALL, (c, names)
            first, last = names.index("S"), len(names) - 1 - names[::-1].index("S")
            # the twelve rotate over three accumulators: no wait states to cover, so no s_nop longer than the parent's
            # between them (k_fused_lone's V' run has none at all)
            assert longest_nop(lines[u[first]:u[last] + 1]) <= longest_nop(lines[u[0]:u[-1] + 1]), c
            assert longest_nop(lines[u[first]:u[last] + 1]) <= 3, c
        assert sum(1 for l in seg if re.search(r"\b(buffer|global|flat)_(load|store)", l)) == 0, c
        assert sum(1 for l in seg if "scratch_" in l) == 0, c
        assert sum(1 for l in seg if "ds_read2" in l) == 0, c
        # per unit: 6 D fragments, 4 lone-bin words, 4 V' fragments, 12 replicated ones (unit 0's D and lone-bin words: before)
        assert sum(1 for l in seg if re.search(r"\bds_read_b64\b", l)) >= AKT * (DS + 4 + 4 + SMALL) - (DS + 4), c
    assert sorted(seen) == [(7, 2), (7, 4), (7, 8)]


def test_the_90_earlier_instances_are_still_there(device_asm):  # noqa: F811
    old = re.findall(r"^_ZN3evc1[12]k_fused_(?:allILi\dELin?\d+ELb[01]E|loneILi\dELi\d+E)EEvNS_9FusedArgsE:", device_asm, re.M)
    assert len(old) == len(set(old)) == 8 * 5 * 2 + 7 + 3
