"""k_fused_lone (evc_fused_all.hip + evc_fused_all_body.inc with EVC_ALL_LONE 1), without a GPU.

At M = 25 the seventh k-step of D = A_j^T V holds bin 24 and three zero slots.  k_fused_lone does not issue it: bin 24
enters the accumulator's start value, d[r] = fma(A[24, e_r], V[24, f], d0), and six MFMAs follow.

* A numpy restatement of the fold on the layout helpers of tests/test_fused_all_lds_host.py: for every wavefront, lane and
  tile the four `a24` addresses return A[24, exemplar] of the lane's four accumulator rows, `v24` is bin 24 of frame
  lane & 15, and each of the four reads is conflict-free under that file's ds_read_b64 model.
* The fold followed by six k-steps equals the seven-k-step product to 1e-15 relative on random positive data.
* The code object: the three instances (7 k-steps; 2, 4, 8 members) hold one sweep of 8 x (6 + 8) MFMAs and a numerator pass
  of 8 x 6, no vector-memory load, scratch access or ds_read2 inside the sweep, and a group segment within 160 KiB.  The
  87 instances of k_fused_all are still found by their old names (the existing tests assert the rest about them).
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_fused_all_lds_host import (AKT, ATILES, AW, LDS_BYTES, SRC, bin_of, conflicts, lane_rows, lds_image, mfma_runs,  # noqa: E402
                                     msteps_of, packed, shape)

M, MS, MT = 25, 7, 2
DS = MS - 1                      # k-steps of the D and P chains
BL = 4 * (MS - 1)                # the lone bin: first (and only real) bin of the last k-step


def lone_addr(w, lane, k, r, pr):
    """the kernel's dL[k * TPD + r * PR]: dL = s_dict + rowB + BL, rowB as in lane_rows (its third entry minus lane & 15)"""
    rowB = lane_rows(w, lane, MS, M, pr)[2] - (lane & 15)
    return rowB + BL + k * 16 * pr + r * pr


def test_the_lone_bin_is_the_last_k_steps_only_real_bin():
    assert msteps_of(M) == MS and M == 4 * MS - 3 and BL == M - 1
    assert [bin_of(MS - 1, q) for q in range(4)] == [BL, BL + 1, BL + 2, BL + 3]     # lane group 0: bin 24; 25 .. 27: none
    pr, on, _ = shape(MS, 2, False)
    assert on and M < pr


def test_a24_and_v24_are_what_the_fold_needs():
    rng = np.random.default_rng(24)
    pr = shape(MS, 2, False)[0]
    members, N = 2, 2 * 512 - 7
    NT = members * ATILES
    A = rng.random((M, N)) + 0.5
    _, A2p = packed(A, NT, MS, MT)
    Apad = np.zeros((M, NT * 16))
    Apad[:, :N] = A
    V = rng.random((M, 16)) + 0.5
    vL = np.zeros(MT * 256)                      # the B-operand image of one frame tile
    for s in range(MS):
        for l in range(64):
            b = bin_of(s, l >> 4)
            vL[s * 64 + l] = V[b, l & 15] if b < M else 0.0
    for member in range(members):
        img = lds_image(A2p, member, MS, M, pr)
        for w in range(AW):
            for lane in range(64):
                assert vL[DS * 64 + (lane & 15)] == V[BL, lane & 15]
                for k in range(AKT):
                    j = member * ATILES + w + AW * k
                    for r in range(4):
                        x = lone_addr(w, lane, k, r, pr)
                        assert 0 <= x < ATILES * 16 * pr
                        assert img[x] == Apad[BL, 16 * j + 4 * (lane >> 4) + r], (member, w, lane, k, r)


def test_the_four_reads_are_free_of_bank_conflicts():
    pr = shape(MS, 2, False)[0]
    for w in range(AW):
        for k in range(AKT):
            for r in range(4):
                assert conflicts([lone_addr(w, lane, k, r, pr) for lane in range(64)]) == 0, (w, k, r)


def test_the_fold_and_six_k_steps_equal_seven_k_steps():
    """per accumulator element: the MFMA chain adds its k-steps in order, four bins each; the fold adds bin 24 first"""
    rng = np.random.default_rng(7)
    A = rng.random((M, 16)) + 0.01               # one exemplar tile
    V = rng.random((M, 16)) + 0.01               # one frame tile
    for d0 in (0.0, 0.25):
        seven = np.full((16, 16), d0)
        for s in range(MS):
            bins = [b for b in (bin_of(s, q) for q in range(4)) if b < M]
            seven = seven + A[bins].T @ V[bins]
        six = d0 + np.outer(A[BL], V[BL])        # (the kernel's fma rounds once: within the same bound)
        for s in range(DS):
            bins = [bin_of(s, q) for q in range(4)]
            six = six + A[bins].T @ V[bins]
        assert np.max(np.abs(six - seven) / seven) <= 1e-15
        np.testing.assert_allclose(seven, d0 + A.T @ V, rtol=1e-14)


# ---------------------------------------------------------------------------------------------------------------------
# the code object


@pytest.fixture(scope="module")
def device_asm():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc) and not shutil.which(hipcc):
        pytest.fail("hipcc not found: the package cannot be built without it either")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "fused_all.s")
        p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--offload-device-only", "-S", SRC,
                            "-o", out], capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
        return open(out).read()


def lone_kernels(asm):
    for m in re.finditer(r"^(_ZN3evc12k_fused_loneILi(\d)ELi(\d+)EEEvNS_9FusedArgsE):[^\n]*\n(.*?)s_endpgm", asm, re.S | re.M):
        name, ms, c, body = m.group(1), int(m.group(2)), int(m.group(3)), m.group(4)
        desc = re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\n(.*?)\.end_amdhsa_kernel", asm, re.S).group(1)
        group = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", desc).group(1))
        yield ms, c, body.split("\n"), group


def test_code_object_of_the_three_instances(device_asm):
    seen = []
    sweep, numerator, y_pass = AKT * (DS + 4 * MT), AKT * DS, AKT * 4 * (MT + 1)
    for ms, c, lines, group in lone_kernels(device_asm):
        seen.append((ms, c))
        pr, on, rest = shape(ms, c, False)
        assert on and group <= LDS_BYTES and group >= rest + 8 * ATILES * 16 * pr - 256, (c, group)
        runs = sorted(len(r) for r in mfma_runs(lines))
        # one copy of the frame-tile loop (the dictionary in LDS only): the numerator pass, one sweep, the Y pass for
        # B's two bin-tile counts
        assert sum(runs) == numerator + sweep + y_pass, (c, runs)
        assert runs.count(sweep) == 1 and runs.count(numerator) == 1, (c, runs)
        seg = next(lines[r[0]:r[-1] + 1] for r in mfma_runs(lines) if len(r) == sweep)
        assert sum(1 for l in seg if re.search(r"\b(buffer|global|flat)_load", l)) == 0, c
        assert sum(1 for l in seg if "scratch_" in l) == 0, c
        assert sum(1 for l in seg if "ds_read2" in l) == 0, c                         # not paired: see LDS_NO_PAIR
        # per unit: 6 D fragments, 4 lone-bin words, 8 V' fragments (unit 0's D fragments and lone-bin words: before)
        assert sum(1 for l in seg if re.search(r"\bds_read_b64\b", l)) >= AKT * (DS + 4 + 4 * MT) - (DS + 4), c
        npass = next(lines[r[0]:r[-1] + 1] for r in mfma_runs(lines) if len(r) == numerator)
        assert sum(1 for l in npass if "scratch_" in l) == 0, c
    assert sorted(seen) == [(7, 2), (7, 4), (7, 8)]


def test_the_87_instances_of_k_fused_all_are_still_there(device_asm):
    old = re.findall(r"^_ZN3evc11k_fused_allILi\dELin?\d+ELb[01]EEEvNS_9FusedArgsE:", device_asm, re.M)
    assert len(old) == len(set(old)) == 8 * 5 * 2 + 7
