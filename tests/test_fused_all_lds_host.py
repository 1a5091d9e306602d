"""k_fused_all's LDS-resident dictionary (evc_fused_all.hip, AllShape), without a GPU.

* A float64 restatement of the layout: the fill from A2p followed by the sweep's reads returns, for every lane, tile,
  k-step and bin tile, exactly what the streamed path loads from A1p / A2p (bins past M: zero), and neither read pattern
  has a bank conflict under the ds_read_b64 model (two groups of 32 lanes, bank = dword address mod 64).
* The code object: the instances that the compile-time budget selects hold the dictionary (group segment within
  160 KiB) and have a sweep without a single vector-memory load or scratch access; the others keep the buffer loads.
"""
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "exemplars_vc_amd", "csrc", "evc_fused_all.hip")

AW, AKT, ATILES, ALL_MAX_MEMBERS = 4, 8, 32, 128
BUDGET = 160 * 1024 - 256
LDS_BYTES = 160 * 1024


def shape(msteps, c, kl):
    """mirror of AllShape<MSTEPS, C, KL>: (row pitch, LDS dictionary on, static LDS besides the dictionary)"""
    mt = 2 if msteps > 4 else 1
    e, ne = mt * 256, msteps * 64
    rstr = max(ne, 256)
    stg = 1 if c > 0 else (ne if c == 0 else ne + ALL_MAX_MEMBERS - 1)
    rest = 8 * 2 * (AW * rstr + 2 * e + (e if kl else 1) + stg) + 12
    dict_bytes = lambda pr: 8 * ATILES * 16 * pr
    pr_all = 4 * msteps + 2
    pr = 0 if kl else (pr_all if rest + dict_bytes(pr_all) <= BUDGET else
                       pr_all - 4 if rest + dict_bytes(pr_all - 4) <= BUDGET else 0)
    return pr, c != 1 and pr > 0 and pr - 1 >= 4 * msteps - 3, rest


def msteps_of(m):
    return (m + 3) // 4 if m <= 16 else 4 + (m - 16 + 3) // 4


def bin_of(s, q):
    return 16 * (s >> 2) + q + 4 * (s & 3)


def row(e):
    return 4 * (((e >> 2) & 1) * 2 + (e >> 3)) + (e & 3)


def lds_image(A2p, member, msteps, M, pr):
    """the kernel's fill loop"""
    mt = 2 if msteps > 4 else 1
    tpd = 16 * pr
    img = np.empty(ATILES * tpd)
    for x in range(ATILES * tpd):
        slot, e, b = x // tpd, row((x // pr) % 16), x % pr
        j = member * ATILES + slot // AKT + AW * (slot % AKT)
        q, r = e >> 2, e & 3
        img[x] = A2p[((j * mt + (b >> 4)) * 2 + (r >> 1)) * 128 + (16 * q + (b & 15)) * 2 + (r & 1)] if b < M else 0.0
    return img


def lane_rows(w, lane, msteps, M, pr):
    """the kernel's four per-lane addresses (doubles): D/P order, its last k-step, V' order, its last bin tile"""
    mt = 2 if msteps > 4 else 1
    tpd = 16 * pr
    bl = 16 * ((msteps - 1) >> 2) + 4 * ((msteps - 1) & 3)
    rowA = w * AKT * tpd + row(4 * (lane & 3) + ((lane & 15) >> 2)) * pr
    rowB = w * AKT * tpd + row(4 * (lane >> 4)) * pr
    return (rowA + (lane >> 4), rowA + min(lane >> 4, M - bl),
            rowB + (lane & 15), rowB + min(lane & 15, M - 16 * (mt - 1)))


def packed(A, NT, msteps, mt):
    """k_pack_dict's A1p / A2p of a [M][N] dictionary (no spare bin: k_fused_all does not use it)"""
    M, N = A.shape
    msp = (msteps + 1) & ~1
    A1p = np.zeros(NT * msp * 64)
    for g in range(A1p.size):
        e, l = g & 1, (g >> 1) & 63
        s, j = 2 * ((g >> 7) % (msp // 2)) + e, (g >> 7) // (msp // 2)
        i = l & 15
        n, b = 16 * j + 4 * (i & 3) + (i >> 2), bin_of(s, l >> 4)
        A1p[g] = A[b, n] if (s < msteps and b < M and n < N) else 0.0
    A2p = np.zeros(NT * mt * 4 * 64)
    for g in range(A2p.size):
        e, l = g & 1, (g >> 1) & 63
        r, u, j = 2 * ((g >> 7) & 1) + e, (g >> 8) % mt, (g >> 8) // mt
        n, b = 16 * j + 4 * (l >> 4) + r, 16 * u + (l & 15)
        A2p[g] = A[b, n] if (b < M and n < N) else 0.0
    return A1p, A2p


def lds_cases():
    for m in range(1, 33):
        ms = msteps_of(m)
        pr, on, _ = shape(ms, 0, False)
        if on and m < pr:
            yield m


def test_the_budget_selects_the_expected_instances():
    on = {(ms, c): shape(ms, c, False)[1] for ms in range(1, 9) for c in (1, 2, 4, 8, 0, -1)}
    assert all(on[(ms, c)] for ms in range(1, 8) for c in (2, 4, 8, 0, -1))         # C2, C5 (M = 25) and the rest
    assert not any(on[(ms, 1)] for ms in range(1, 9))                            # one member (C1): streamed
    assert not any(on[(8, c)] for c in (1, 2, 4, 0, -1))                         # M 29 .. 32: streamed
    assert not any(shape(ms, c, True)[1] for ms in range(1, 9) for c in (1, 2, 4, 0, -1))   # KL: streamed
    assert shape(7, 0, False)[0] == 26 and list(lds_cases())[-1] == 25           # C2: M <= 25 in LDS, 26 .. 28 not
    assert all(shape(ms, c, False)[0] == 4 * ms + 2 for ms in range(1, 7) for c in (2, 4, 0, -1))


@pytest.mark.parametrize("M", [3, 8, 13, 16, 17, 20, 21, 24, 25])
def test_lds_reads_equal_the_streamed_fragments(M):
    ms, rng = msteps_of(M), np.random.default_rng(M)
    mt = 2 if ms > 4 else 1
    pr = shape(ms, 0, False)[0]
    members, N = 2, 2 * 512 - 7                   # a short last member: exemplars past N are zero in both images
    NT = members * ATILES
    A = rng.random((M, N)) + 0.5
    A1p, A2p = packed(A, NT, ms, mt)
    msp = (ms + 1) & ~1
    for member in range(members):
        img = lds_image(A2p, member, ms, M, pr)
        assert np.all(img.reshape(ATILES, 16, pr)[:, :, M:] == 0.0)          # the zero slots
        for w in range(AW):
            for lane in range(64):
                dA, dAL, dB, dBL = lane_rows(w, lane, ms, M, pr)
                for k in range(AKT):
                    j = member * ATILES + w + AW * k
                    for s in range(ms):
                        got = img[(dAL if s == ms - 1 else dA) + k * 16 * pr + 16 * (s >> 2) + 4 * (s & 3)]
                        assert got == A1p[((j * (msp // 2) + (s >> 1)) * 64 + lane) * 2 + (s & 1)], (w, lane, k, s)
                    for u in range(mt):
                        for r in range(4):
                            got = img[(dBL if u == mt - 1 else dB) + k * 16 * pr + r * pr + 16 * u]
                            want = A2p[(((j * mt + u) * 2 + (r >> 1)) * 64 + lane) * 2 + (r & 1)]
                            assert got == want, (w, lane, k, u, r)


def conflicts(addrs):
    """extra LDS cycles of one ds_read_b64 wave instruction (lane -> double index): per 32-lane group, the most
    distinct addresses on one bank, minus one"""
    extra = 0
    for g in (range(0, 32), range(32, 64)):
        banks = {}
        for lane in g:
            for dw in (2 * addrs[lane], 2 * addrs[lane] + 1):
                banks.setdefault(dw % 64, set()).add(dw)
        extra += max(len(v) for v in banks.values()) - 1
    return extra


@pytest.mark.parametrize("M", list(lds_cases()))
def test_both_read_patterns_are_free_of_bank_conflicts(M):
    ms = msteps_of(M)
    mt = 2 if ms > 4 else 1
    pr = shape(ms, 0, False)[0]
    for w in range(AW):
        rows = [lane_rows(w, lane, ms, M, pr) for lane in range(64)]
        for k in range(AKT):
            for s in range(ms):
                a = [(r[1] if s == ms - 1 else r[0]) + k * 16 * pr + 16 * (s >> 2) + 4 * (s & 3) for r in rows]
                assert conflicts(a) == 0, ("D/P", M, w, k, s)
            for u in range(mt):
                for rr in range(4):
                    a = [(r[3] if u == mt - 1 else r[2]) + k * 16 * pr + rr * pr + 16 * u for r in rows]
                    assert conflicts(a) == 0, ("V'", M, w, k, u, rr)


def test_the_conflict_model_sees_a_plain_pitch():
    """the model is not blind: rows of 25 doubles in natural order conflict in both patterns"""
    a = [(4 * (lane & 3) + ((lane & 15) >> 2)) * 25 + (lane >> 4) for lane in range(64)]
    b = [(4 * (lane >> 4)) * 25 + (lane & 15) for lane in range(64)]
    assert conflicts(a) > 0 and conflicts(b) > 0


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


def kernels(asm):
    for m in re.finditer(r"^(_ZN3evc11k_fused_allILi(\d)ELi(n?\d+)ELb([01])EEEvNS_9FusedArgsE):[^\n]*\n(.*?)s_endpgm", asm,
                         re.S | re.M):
        name, ms, c, kl, body = m.group(1), int(m.group(2)), m.group(3), m.group(4) == "1", m.group(5)
        c = -int(c[1:]) if c.startswith("n") else int(c)
        desc = re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\n(.*?)\.end_amdhsa_kernel", asm, re.S).group(1)
        group = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", desc).group(1))
        yield ms, c, kl, body.split("\n"), group


def mfma_runs(lines, gap=200):
    idx = [i for i, l in enumerate(lines) if "v_mfma" in l]
    runs = []
    for i in idx:
        if runs and i - runs[-1][-1] < gap:
            runs[-1].append(i)
        else:
            runs.append([i])
    return runs


def test_code_object_lds_instances(device_asm):
    seen = 0
    for ms, c, kl, lines, group in kernels(device_asm):
        seen += 1
        mt = 2 if ms > 4 else 1
        pr, on, rest = shape(ms, c, kl)
        assert group <= LDS_BYTES, (ms, c, kl, group)
        sweep = AKT * (ms + 4 * mt)                 # MFMAs of one sweep (D and V') - KL: the same count
        lds_sweeps = []
        for r in mfma_runs(lines):
            if len(r) < sweep:
                continue                            # the numerator pass
            seg = lines[r[0]:r[-1] + 1]
            vmem = sum(1 for l in seg if re.search(r"\b(buffer|global|flat)_load", l))
            if vmem == 0:
                lds_sweeps.append(seg)
        if on:
            assert group >= rest + 8 * ATILES * 16 * pr - 256, (ms, c, group)
            assert len(lds_sweeps) == 1, (ms, c, kl, len(lds_sweeps))
            seg = lds_sweeps[0]
            assert sum(1 for l in seg if "scratch_" in l) == 0, (ms, c)
            assert sum(1 for l in seg if re.search(r"\bds_read_b64\b", l)) >= sweep - ms, (ms, c)   # (unit 0: before)
            assert sum(1 for l in seg if "ds_read2" in l) == 0, (ms, c)       # not paired: see LDS_NO_PAIR
        else:
            assert not lds_sweeps, (ms, c, kl)
    assert seen == 8 * 5 * 2 + 7                  # + C = 8 (direct exchange) where the dictionary fits: M <= 25
