"""The end of a frame tile in k_fused_all (evc_fused_all.hip, round 9), without a GPU.

* A numpy model of the members' slabs of Y and of k_unpack_y's sum over them: every member writes its share of B H in
  the Yp image format ([tt][8][64], k-step 4 u + th / 64 and lane th % 64 for thread th of pass u), inside its slab;
  the sum over the slabs in member order is B H; the order of the sum is the members' (a permuted order gives other
  bits, so the model tells them apart).
* The code object: still 87 instances; every copy of the tile's end holds, beside the 16 16-byte stores of the packed
  activations (8 tiles x 2), 16 more for the caller's frame-major H (8 tiles x 2 pairs of a lane's four exemplars),
  and the 8 x 8 MFMAs of the Y pass per bin-tile count it is compiled for.
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


def msteps_of(m):
    return (m + 3) // 4 if m <= 16 else 4 + (m - 16 + 3) // 4


def bin_of(s, q):
    return 16 * (s >> 2) + q + 4 * (s & 3)


def lds_dict(msteps, c, kl):
    """AllShape<MSTEPS, C, KL>::LDS_DICT: such an instance holds two copies of the frame-tile loop"""
    mt = 2 if msteps > 4 else 1
    e, ne = mt * 256, msteps * 64
    rstr = max(ne, 256)
    stg = 1 if c > 0 else (ne if c == 0 else ne + ALL_MAX_MEMBERS - 1)
    rest = 8 * 2 * (AW * rstr + 2 * e + (e if kl else 1) + stg) + 12
    dict_bytes = lambda pr: 8 * ATILES * 16 * pr
    pr_all = 4 * msteps + 2
    pr = 0 if kl else (pr_all if rest + dict_bytes(pr_all) <= BUDGET else
                       pr_all - 4 if rest + dict_bytes(pr_all - 4) <= BUDGET else 0)
    return c != 1 and pr > 0 and pr - 1 >= 4 * msteps - 3


# ---------------------------------------------------------------------------------------------------------------------
# the slabs


def member_slabs(B, H, members, TTp):
    """what the kernel's Y pass leaves: slab[m][tt][s][l] = sum over member m's exemplars, wavefront by wavefront"""
    Mb, N = B.shape
    T = H.shape[1]
    ut = 2 if Mb > 16 else 1
    stride = TTp * 512
    slabs = np.full(members * stride, np.nan)
    Bp = np.zeros((32, members * 512))
    Bp[:Mb, :N] = B
    Hp = np.zeros((members * 512, 16 * TTp))
    Hp[:N, :T] = H
    for m in range(members):
        for tt in range((T + 15) // 16):
            part = np.zeros((AW, ut * 256))
            for w in range(AW):
                for k in range(AKT):                     # the wavefront's tiles, in its order
                    n0 = 16 * (m * ATILES + w + AW * k)
                    for u in range(ut):
                        for th in range(256):
                            mb, fr = bin_of(4 * u + (th >> 6), (th & 63) >> 4), th & 15
                            part[w, 256 * u + th] += Bp[mb, n0:n0 + 16] @ Hp[n0:n0 + 16, 16 * tt + fr]
            for u in range(ut):
                for th in range(256):
                    idx = m * stride + (tt * 8 + 4 * u) * 64 + th
                    assert m * stride <= idx < (m + 1) * stride
                    assert np.isnan(slabs[idx])                      # every word once
                    slabs[idx] = ((part[0, 256 * u + th] + part[1, 256 * u + th]) + part[2, 256 * u + th]) + \
                        part[3, 256 * u + th]
    return slabs, stride


def unpack_y(slabs, stride, members, msteps, Mb, T, order=None):
    """k_unpack_y: one thread per (tt, s, l), the members added in order"""
    Y = np.zeros((Mb, T))
    for gid in range(((T + 15) // 16) * msteps * 64):
        l, s, tt = gid & 63, (gid >> 6) % msteps, (gid >> 6) // msteps
        t, mb = 16 * tt + (l & 15), bin_of(s, l >> 4)
        if t >= T or mb >= Mb:
            continue
        ms = list(order if order is not None else range(members))
        v = slabs[ms[0] * stride + (tt * 8 + s) * 64 + l]
        for m in ms[1:]:
            v += slabs[m * stride + (tt * 8 + s) * 64 + l]
        Y[mb, t] = v
    return Y


@pytest.mark.parametrize("Mb,members,N,T", [(25, 3, 1500, 21), (7, 2, 1024, 16), (32, 1, 500, 5)])
def test_the_slabs_sum_to_b_h_in_member_order(Mb, members, N, T):
    rng = np.random.default_rng(Mb)
    B, H = rng.random((Mb, N)), rng.random((N, T)) * (rng.random((N, T)) < 0.05)
    TTp = -(-((T + 15) // 16) // 4) * 4
    slabs, stride = member_slabs(B, H, members, TTp)
    Y = unpack_y(slabs, stride, members, msteps_of(Mb), Mb, T)
    assert np.isfinite(Y).all()                                      # nothing read that nobody wrote
    np.testing.assert_allclose(Y, B @ H, rtol=1e-13, atol=0)
    if members > 2:                                                  # the order is part of the result
        other = unpack_y(slabs, stride, members, msteps_of(Mb), Mb, T, order=list(range(members))[::-1])
        np.testing.assert_allclose(other, Y, rtol=1e-13, atol=0)
        assert not np.array_equal(other, Y)


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
        ms, c, kl, body = int(m.group(2)), m.group(3), m.group(4) == "1", m.group(5)
        c = -int(c[1:]) if c.startswith("n") else int(c)
        yield ms, c, kl, body.split("\n")


def test_the_tile_end_of_every_instance(device_asm):
    seen = 0
    for ms, c, kl, lines in kernels(device_asm):
        seen += 1
        mt = 2 if ms > 4 else 1
        copies = 2 if lds_dict(ms, c, kl) else 1
        x16 = sum(1 for l in lines if re.search(r"\bglobal_store_dwordx4\b", l))
        # the packed activations (8 tiles x 2) and the caller's frame-major H (8 tiles x 2 pairs), per copy
        assert x16 >= copies * (2 * AKT + 2 * AKT), (ms, c, kl, x16)
        mfma = sum(1 for l in lines if "v_mfma" in l)
        numerator = 0 if kl else AKT * ms
        sweep = AKT * (ms + 4 * mt)
        y_pass = AKT * 4 * (mt + (1 if mt > 1 else 0))               # one copy per bin-tile count of B: MT, and 1
        # (at least: the compiler lays out a second sweep in the one-member instances, whose halves sweep together)
        assert mfma >= copies * (numerator + sweep + y_pass), (ms, c, kl, mfma)
        if c != 1:
            assert mfma == copies * (numerator + sweep + y_pass), (ms, c, kl, mfma)
    assert seen == 8 * 5 * 2 + 7
