"""The direct exchange of k_fused_quad<7, 2 | 4 | 8> (evc_fused_all_body.inc, the QUAD branch), without a GPU.

The exchange runs beside the other half's sweep on the same SIMDs, and on gfx950 an f64 MFMA and a vector instruction of
one SIMD do not overlap (tools/ubench/mfma_valu_f64.hip): every vector instruction of the exchange is time of the sweep.
k_fused_quad's exchange therefore keeps the protocol of k_fused_lone's and drops the instructions the result does not need:
no zeroing of the slots and no copies of the thread's own pair (every fetch round loads all C slots, the own one
included), and the tag test as one chain per epoch value (the epoch is wave-uniform), two low words per three-input
instruction.

* The code object: the region between `s_setprio 3` and `s_setprio 0` of the three instances - its vector instructions
  against the parent's count, its memory sites, no scratch, no atomics.
* A restatement of the tag test on all 2^16 patterns of sixteen epoch bits, for both epoch values.
"""
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_fused_all_lds_host import device_asm  # noqa: E402,F401  (the module-scoped fixture: one compilation)
from test_fused_quad_host import quad_kernels  # noqa: E402
from test_fused_step_chain_host import VECTOR  # noqa: E402

# vector instructions (VECTOR: v_ but for the MFMAs) between `s_setprio 3` and `s_setprio 0` of k_fused_quad<7, C> at commit
# fb7e793, counted the way exchange_regions / this file's test count them, and that commit's scratch
PARENT_VECTOR = {2: 55, 4: 83, 8: 138}
PARENT_SCRATCH = {2: (336, 97), 4: (312, 88), 8: (320, 89)}     # bytes per lane, scratch instructions in the kernel
# at 8 members at least 40 fewer than the parent's 138; at 2 and 4 the proportionate drop, rounded up
BOUND = {c: n - -(-40 * n // 138) for c, n in PARENT_VECTOR.items()}


def exchange_regions(lines):
    out, start = [], None
    for i, l in enumerate(lines):
        if re.match(r"\s+s_setprio 3\b", l):
            assert start is None, "s_setprio 3 twice"
            start = i
        elif re.match(r"\s+s_setprio 0\b", l):
            assert start is not None, "s_setprio 0 without s_setprio 3"
            out.append(lines[start:i + 1])
            start = None
    assert start is None
    return out


def test_the_bounds():
    assert BOUND == {2: 39, 4: 58, 8: 98}


def test_code_object_of_the_exchange(device_asm):  # noqa: F811
    seen = []
    for ms, c, lines, res in quad_kernels(device_asm):
        seen.append((ms, c))
        # one fragment source (the LDS dictionary; k_fused_quad has no streamed copy of the step loop): one exchange
        regions = exchange_regions(lines)
        assert len(regions) == 1, (c, len(regions))
        region = regions[0]
        vector = [l.split()[0] for l in region if VECTOR.match(l)]
        print(f"k_fused_quad<7, {c}>: {len(vector)} vector instructions in the exchange (parent {PARENT_VECTOR[c]}, bound {BOUND[c]})")
        assert not any(v.startswith("v_mov_b64") for v in vector), c
        assert len(vector) <= BOUND[c], (c, len(vector), sorted(vector))
        # the sums keep their orders: 2 x 4 over the wavefronts' partials, 2 x C over the members
        assert vector.count("v_add_f64") == 8 + 2 * c, c
        sites = lambda pattern: sum(1 for l in region if re.search(pattern, l))
        assert sites(r"\bbuffer_store_dwordx4\b.*\bsc1\b") == 1 and sites(r"\b(buffer|global|flat)_store") == 1, c
        assert sites(r"\bbuffer_load_dwordx4\b.*\bsc1\b") == c and sites(r"\b(buffer|global|flat)_load_dwordx4\b") == c, c
        assert sites(r"\b(buffer|global)_load_dwordx2\b.*\bsc1\b") == 1 and sites(r"\b(buffer|global|flat)_load_dwordx2\b") == 1, c
        # (what is left: coop_abort, looked at every 64th poll of either wait)
        assert sites(r"\b(buffer|global|flat)_load_") == c + 1 + sites(r"\bglobal_load_dword\b"), c
        assert sites(r"\b(buffer|global|flat)_atomic") == 0, c
        assert sum(1 for l in lines if re.search(r"\b(buffer|global|flat)_atomic", l)) == 0, c
        assert sites(r"\bscratch_") == 0, c
        assert res["vgpr"] <= 256 and res["scratch"] <= PARENT_SCRATCH[c][0], (c, res)
        assert sum(1 for l in lines if re.search(r"\bscratch_", l)) <= PARENT_SCRATCH[c][1], c
    assert sorted(seen) == [(7, 2), (7, 4), (7, 8)]


# ---------------------------------------------------------------------------------------------------------------------
# the tag test

MASK = np.uint32(0xFFFFFFFF)


def stale(words, tag):
    """the kernel's chain on the 2 C low words of a fetch round, words [patterns][2 C] uint32: epoch 0 - OR of the words,
    two per step (v_or_b32, v_or3_b32); epoch 1 - OR of their complements, formed as NOT of the AND (v_and_b32,
    v_bitop3_b32 0x80, at last 0x7f); then bit 0"""
    acc = words[:, 0] | words[:, 1] if tag == 0 else words[:, 0] & words[:, 1]
    for i in range(2, words.shape[1], 2):
        acc = acc | words[:, i] | words[:, i + 1] if tag == 0 else acc & words[:, i] & words[:, i + 1]
    if tag == 1:
        acc = ~acc & MASK
    return (acc & np.uint32(1)) != 0


def test_the_tag_test_on_every_pattern_of_sixteen_epoch_bits():
    rng = np.random.default_rng(16)
    patterns = np.arange(1 << 16, dtype=np.uint32)
    epoch = (patterns[:, None] >> np.arange(16, dtype=np.uint32)[None, :]) & np.uint32(1)
    for c in (2, 4, 8):
        for tag in (0, 1):
            # bits 1 .. 31 are a double's mantissa: anything
            words = (rng.integers(0, 1 << 31, size=(1 << 16, 2 * c), dtype=np.uint32) << np.uint32(1)) | epoch[:, :2 * c]
            want = (epoch[:, :2 * c] != tag).any(axis=1)
            assert np.array_equal(stale(words, tag), want), (c, tag)
            # each 8-byte half is checked by itself: one stale word among 2 C fresh ones is found wherever it is
            for i in range(2 * c):
                one = np.full((1, 2 * c), tag, dtype=np.uint32)
                one[0, i] ^= 1
                assert stale(one, tag)[0], (c, tag, i)
            assert not stale(np.full((1, 2 * c), tag, dtype=np.uint32), tag)[0]
