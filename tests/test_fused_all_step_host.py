"""k_fused_all's direct exchange on 16-byte words (evc_fused_all.hip), without a GPU.

* A numpy mirror of the pair ownership for every k-step count 1 .. 8: thread th < NE / 2 of the exchanging half owns the
  elements 2 th and 2 th + 1; every element is published exactly once, every access is 16-byte aligned and inside the
  member's 512 words for every group, parity and member, threads from NE / 2 on touch nothing - and a mapping that breaks
  one of these is rejected.
* The code object: every instance with 2, 4 or 8 members publishes with ONE 16-byte sc1 vector store per thread and
  fetches with C guarded 16-byte sc1 vector loads per fetch round, of which the one of the member's own words is skipped:
  C - 1 execute.  The loads sit in the poll loop.  The only 8-byte agent-scope load left is the watch word (one per
  wavefront and poll), the only 4-byte one the abort word; no 8-byte agent-scope store is left.  The other instances keep
  their 8-byte words.  No kernel holds a scalar store to memory, a scalar atomic or a scalar-cache write-back.
* Every instance of the kernel is there, and in none does a scratch access stand inside a cluster of MFMAs: whatever the
  register allocator spills, it does not spill inside a unit of the sweep.
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

AW, MEMBER_WORDS = 4, 512


# ---------------------------------------------------------------------------------------------------------------------
# the pair ownership


def pair_of(msteps, th):
    """the kernel's mapping: (first element, byte offset within the member's words) of thread th, None: no part"""
    ne = 64 * msteps
    if th >= ne // 2:
        return None
    return 2 * th, 16 * th


def wave_takes_part(msteps, w):
    return w * 64 < 64 * msteps // 2


def check_plan(msteps, plan):
    ne = 64 * msteps
    published = np.zeros(MEMBER_WORDS, dtype=int)
    for th in range(AW * 64):
        got = plan(msteps, th)
        if th >= ne // 2:
            assert got is None, (msteps, th)                     # idle threads touch nothing
            continue
        assert wave_takes_part(msteps, th // 64)
        e, off = got
        assert off % 16 == 0 and off == 8 * e, (msteps, th)      # the 16 bytes are the pair's two words, aligned
        assert 0 <= off and off + 16 <= 8 * MEMBER_WORDS, (msteps, th)
        published[e:e + 2] += 1
    assert np.all(published[:ne] == 1) and np.all(published[ne:] == 0), msteps
    for w in range(AW):                                          # a wavefront without work has no thread with work
        assert wave_takes_part(msteps, w) == any(plan(msteps, th) is not None for th in range(64 * w, 64 * w + 64))


@pytest.mark.parametrize("msteps", range(1, 9))
def test_every_element_is_published_once_aligned_and_in_bounds(msteps):
    check_plan(msteps, pair_of)
    assert 64 * msteps // 2 <= AW * 64


@pytest.mark.parametrize("C", [2, 4, 8])
def test_every_group_buffer_is_16_byte_aligned(C):
    """byte offset of member m's words of group g, parity q, from the (16-byte aligned, checked at launch) base"""
    for groups in (2, 4, 64, 128, 256):
        for q in range(2):
            for g in range(groups):
                xo = (q * groups + g) * C * 4096
                assert xo % 16 == 0 and xo + C * 4096 <= 2 * groups * C * 4096     # inside the buffer resource
                for m in range(C):
                    assert (xo + m * 4096) % 16 == 0 and xo + m * 4096 == 8 * ((q * groups + g) * C * 512 + m * 512)


def test_a_wrong_pair_mapping_is_rejected():
    shifted = lambda ms, th: None if th >= 32 * ms else (2 * th + 1, 16 * th + 8)           # misaligned pairs
    strided = lambda ms, th: None if th >= 32 * ms else (th, 8 * th)                        # overlapping pairs
    eager = lambda ms, th: (2 * th, 16 * th) if th < 256 else None                          # idle threads publish
    for mutant in (shifted, strided, eager):
        with pytest.raises(AssertionError):
            for ms in range(1, 9):
                check_plan(ms, mutant)


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


def count(lines, pattern):
    return sum(1 for l in lines if re.search(pattern, l))


def loop_depth(lines, i):
    """loop depth of the basic block that holds line i, from the compiler's block comments"""
    for j in range(i, -1, -1):
        t = lines[j].lstrip()
        if t.startswith(".LBB") or t.startswith("; %bb."):
            m = re.search(r"in Loop: .*Depth=(\d+)", lines[j])
            for k in range(j, min(j + 5, len(lines))):          # a loop header: its depth stands below its label
                m = m or re.search(r"Loop Header: Depth=(\d+)", lines[k])
            return int(m.group(1)) if m else 0
    return 0


ST16 = r"\bbuffer_store_dwordx4\b.*\bsc1\b"
LD16 = r"\bbuffer_load_dwordx4\b.*\bsc1\b"
LD8 = r"\b(global|buffer|flat)_load_dwordx2\b.*\bsc1\b"
ST8 = r"\b(global|buffer|flat)_store_dwordx2\b.*\bsc1\b"
ATOMIC = r"\b(global|buffer|flat)_atomic"


def test_code_object_exchanges_16_byte_words(device_asm):
    seen = 0
    for ms, c, kl, lines in kernels(device_asm):
        copies = count(lines, r"\bs_setprio 3\b")      # the exchange is compiled once per fragment source (LDS / streamed)
        assert copies in (1, 2), (ms, c, kl)
        assert count(lines, ATOMIC) == 0, (ms, c, kl)               # no floating-point (or other) global atomics
        if c not in (2, 4, 8):
            assert count(lines, ST16) == 0 and count(lines, LD16) == 0, (ms, c, kl)     # these keep their 8-byte words
            continue
        seen += 1
        # per thread and exchange: 1 store; per fetch round: C load sites, the member's own one skipped - C - 1 execute
        assert count(lines, ST16) == copies, (ms, c, kl)
        assert count(lines, LD16) == c * copies, (ms, c, kl)
        assert count(lines, ST8) == 0, (ms, c, kl)
        assert count(lines, LD8) == copies, (ms, c, kl)             # the watch word
        for i, l in enumerate(lines):
            if re.search(LD16, l):
                assert loop_depth(lines, i) == 3, (ms, c, kl, i, l)     # frame tiles > steps > the poll loop
                guard = [t for t in lines[max(0, i - 12):i] if "s_cbranch" in t or t.lstrip().startswith(".LBB")]
                assert guard, (ms, c, kl, i)                            # reached through the test against `member`
            if re.search(ST16, l):
                assert loop_depth(lines, i) == 2, (ms, c, kl, i, l)
            if re.search(LD8, l):
                assert loop_depth(lines, i) == 3, (ms, c, kl, i, l)
    assert seen == 8 * 2 * 2 + 7          # C = 2, 4: every k-step count, both losses; C = 8: where the dictionary fits


def test_no_scratch_access_inside_a_cluster_of_mfmas(device_asm):
    """A cluster is a run of MFMAs at most 60 lines apart: a unit of the sweep, or the numerator pass.  (The definition
    is tools/spill_audit.py's, repeated here: that tool prints, it has no function to share.)  The kernel's text runs to
    the end of the function, past every early exit."""
    lines = device_asm.split("\n")
    starts = [i for i, l in enumerate(lines) if re.match(r"_ZN3evc11k_fused_allILi\dELin?\d+ELb[01]EEEvNS_9FusedArgsE:", l)]
    # k-steps 1 .. 8 x both losses x C = 1, 2, 4, 0, -1, and C = 8 where the dictionary fits in LDS (Frobenius, k-steps <= 7)
    assert len(starts) == 8 * 2 * 5 + 7
    for start in starts:
        name = lines[start].split(":")[0]
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        body = lines[start:end]
        clusters = []
        for i, l in enumerate(body):
            if "v_mfma" in l:
                if clusters and i - clusters[-1][1] <= 60:
                    clusters[-1][1] = i
                else:
                    clusters.append([i, i])
        assert clusters, name
        inside = [body[i].strip() for i, l in enumerate(body)
                  if "scratch_" in l and any(lo <= i <= hi for lo, hi in clusters)]
        assert not inside, (name, inside[:4])


def test_no_kernel_writes_memory_from_the_scalar_unit(device_asm):
    """scalar stores, scalar atomics and scalar-cache write-backs are not to appear in any kernel"""
    s = "s" + "_"
    families = [s + "store" + "_", s + "buffer_" + "store", s + "scratch_" + "store", s + "atomic" + "_",
                s + "buffer_" + "atomic", s + "dcache_" + "wb", s + "dcache_" + "discard"]
    body = [l for l in device_asm.split("\n") if not l.lstrip().startswith((";", "//"))]
    for f in families:
        assert not any(re.search(r"\b" + f, l, re.I) for l in body), f
