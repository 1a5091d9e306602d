"""The update's range test decided once per sweep (mu_tile_hoisted in evc_fused_common.h, HOIST in
evc_fused_all_body.inc), without a GPU.

A sweep of k_fused_all / k_fused_lone (1, 2, 4 or 8 members, Frobenius) skips the per-unit range test of the
denominators d = d0 + A_j^T V when the member is tame (no padding exemplar, entries finite and >= 0, column sums in
[2^-100, 2^100], d0 in [0, 2^100], fast_lo <= the high word of 2^-201) and every element of V of a bin < M lies in
[2^-100, 2^100).

* A numpy restatement of the bound: at the corners of the tame ranges (column sums and V at 2^-100 and 2^100, d0 at 0 and
  2^100, M = 1, 25, 32) d as the kernel accumulates it - the lone bin's FMA first at M = 25, then k-steps of four bins -
  stays in the fast range [lo, 2^250) for every lo the tame rule admits.  The low corner also shows why the rule stops
  one binade short of 2^-200: there d may round to just below 2^-200.
* The high-word thresholds in the header equal the ones derived here.
* Ownership: every element of V of a bin < M is tested by exactly one thread and every element of a bin >= M by none,
  for the direct exchange's pairs at every NE in use and for the one-member path's e0 / e1.
* The code object, compiled as tests/test_fused_all_lds_host.py compiles it: k_fused_lone<7, 8> and k_fused_all<7, 8, false>
  keep one LDS sweep of the pinned length without vector-memory loads, scratch accesses or ds_read2, the group segment
  stays within 160 KiB, the 87 + 3 instances keep their names, and inside the sweep the range test is branched over
  (its v_max3_u32 stands out of line, behind one scalar branch per unit), not computed and discarded.
"""
import os
import re
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_fused_all_lds_host import AKT, AW, LDS_BYTES, ROOT, bin_of, kernels, mfma_runs, msteps_of, shape  # noqa: E402
from test_fused_all_lds_host import device_asm  # noqa: E402,F401  (the module-scoped fixture: one compilation)
from test_fused_lone_host import lone_kernels  # noqa: E402

HEADER = os.path.join(ROOT, "exemplars_vc_amd", "csrc", "evc_fused_common.h")
FAST_LO_DEFAULT = 0x30500000                     # fast_lo without a clamp: 2^-250


def hi_word(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0] >> 32


def header_constant(name):
    m = re.search(r"constexpr unsigned " + name + r" = (0x[0-9A-Fa-f]+)u;", open(HEADER).read())
    assert m, name
    return int(m.group(1), 16)


def in_v_range(x, lo, hi):
    """the kernel's range_v_ok: one unsigned comparison of the high word"""
    return ((hi_word(x) - lo) & 0xFFFFFFFF) < hi - lo


def test_the_thresholds_are_the_derived_ones():
    v_lo, v_hi = header_constant("RANGE_V_LO"), header_constant("RANGE_V_HI")
    lo_max, fast_hi = header_constant("RANGE_LO_MAX"), header_constant("FAST_HI_WORD")
    assert v_lo == hi_word(2.0 ** -100) == (1023 - 100) << 20
    assert v_hi == hi_word(2.0 ** 100) == (1023 + 100) << 20
    assert lo_max == hi_word(2.0 ** -201) == (1023 - 201) << 20
    assert fast_hi == hi_word(2.0 ** 250)
    assert FAST_LO_DEFAULT == hi_word(2.0 ** -250) <= lo_max          # no clamp: always admissible
    # CLAMP: fast_lo = hi_word(eps) + 0x00200000 - tame up to eps < 2^-202, so the test's eps = 1e-3 is not
    assert hi_word(2.0 ** -203) + 0x00200000 == lo_max and hi_word(1e-3) + 0x00200000 > lo_max
    text = open(HEADER).read()
    assert re.search(r"RANGE_SUM_LO = 0x1p-100, RANGE_SUM_HI = 0x1p100;", text)
    # the test on V: [2^-100, 2^100) and nothing else
    below, top = np.nextafter(2.0 ** -100, 0.0), np.nextafter(2.0 ** 100, 0.0)
    for x, want in ((2.0 ** -100, True), (below, False), (top, True), (2.0 ** 100, False), (1.0, True), (0.0, False),
                    (-0.0, False), (-1.0, False), (5e-324, False), (2.0 ** -1022, False), (np.inf, False), (-np.inf, False),
                    (np.nan, False), (-np.nan, False)):
        assert in_v_range(x, v_lo, v_hi) == want, x


def accumulate(a, v, d0, lone):
    """d of one (exemplar, frame) as the kernel forms it: the start value (with the lone last bin folded in by one FMA -
    here a product and a sum, two roundings, inside the same bound), then one k-step of four bins after the other"""
    M = len(a)
    ms = msteps_of(M)
    d = np.float64(d0)
    steps = range(ms)
    if lone:
        d = a[M - 1] * v[M - 1] + d
        steps = range(ms - 1)
    for s in steps:
        for q in range(4):
            b = bin_of(s, q)
            if b < M:
                d = d + a[b] * v[b]
    return d


def seq_sum(a):
    """the tame test's column sum: bins 0 .. M - 1 in order"""
    cs = np.float64(0.0)
    for x in a:
        cs = cs + x
    return cs


def columns(M, total):
    """dictionary columns whose computed sum passes the tame test at the corner `total`"""
    one = np.zeros(M)
    one[M // 2] = total
    yield one
    x = np.float64(total) / M
    if total < 1.0:
        while seq_sum(np.full(M, x)) < total:
            x = np.nextafter(x, np.inf)
    else:
        while seq_sum(np.full(M, x)) > total:
            x = np.nextafter(x, 0.0)
    yield np.full(M, x)
    ramp = np.arange(1, M + 1, dtype=np.float64)
    ramp *= total / ramp.sum()
    if total < 1.0:
        while seq_sum(ramp) < total:
            ramp[0] = np.nextafter(ramp[0], np.inf)
    else:
        while seq_sum(ramp) > total:
            ramp[-1] = np.nextafter(ramp[-1], 0.0)
    yield ramp


@pytest.mark.parametrize("M", [1, 25, 32])
def test_d_stays_in_the_fast_range_at_the_corners(M):
    lo_max, fast_hi = header_constant("RANGE_LO_MAX"), header_constant("FAST_HI_WORD")
    v_lo, v_hi = header_constant("RANGE_V_LO"), header_constant("RANGE_V_HI")
    v_top = np.nextafter(2.0 ** 100, 0.0)
    smallest, largest = np.inf, 0.0
    for total in (2.0 ** -100, 2.0 ** 100):
        for a in columns(M, total):
            assert (a >= 0).all() and 2.0 ** -100 <= seq_sum(a) <= 2.0 ** 100             # tame
            for vval in (2.0 ** -100, v_top):
                v = np.full(M, vval)
                assert in_v_range(vval, v_lo, v_hi)
                for d0 in (0.0, 2.0 ** 100):
                    for lone in ((False, True) if M == 25 else (False,)):
                        d = accumulate(a, v, d0, lone)
                        smallest, largest = min(smallest, d), max(largest, d)
                        for lo in (FAST_LO_DEFAULT, lo_max):
                            assert ((hi_word(d) - lo) & 0xFFFFFFFF) < fast_hi - lo, (M, total, vval, d0, lone, d)
    # the corners are where the argument puts them: 2^-200 and 2^200 (+ d0), up to the chain's rounding
    assert 2.0 ** -200 * (1 - 2.0 ** -46) <= smallest <= 2.0 ** -200 * (1 + 2.0 ** -46)
    assert largest <= 2.0 ** 200 * (1 + 2.0 ** -46) + 2.0 ** 100
    assert hi_word(smallest) >= lo_max and hi_word(largest) < fast_hi


def test_the_low_corner_can_round_below_two_to_the_minus_200():
    """why the rule asks for fast_lo <= hi_word(2^-201), not 2^-200: a column whose computed sum is exactly 2^-100 under
    the tame test's order of summation can give a d one ulp short of 2^-200 in the chain's order"""
    rng = np.random.default_rng(200)
    M, found = 25, False
    for _ in range(2000):
        a = rng.random(M)
        a *= 2.0 ** -100 / seq_sum(a)
        if seq_sum(a) != 2.0 ** -100:
            continue
        d = accumulate(a, np.full(M, 2.0 ** -100), 0.0, True)
        if d < 2.0 ** -200:
            found = True
            assert hi_word(d) == hi_word(2.0 ** -200) - 1 and hi_word(d) >= header_constant("RANGE_LO_MAX")
            break
    assert found


# ---------------------------------------------------------------------------------------------------------------------
# who tests which element of V


def real_elements(ms, M):
    ne = 64 * ms
    return {e for e in range(ne) if bin_of(e >> 6, (e & 63) >> 4) < M}


@pytest.mark.parametrize("M", range(1, 33))
def test_direct_exchange_every_real_element_has_one_tester(M):
    """thread th < NE / 2 of a wavefront w with 64 w < NE / 2 owns the pair 2 th, 2 th + 1 and tests it when the pair's
    bin (one lane group of one k-step) is < M"""
    ms = msteps_of(M)
    ne = 64 * ms
    tested = []
    for th in range(AW * 64):
        w = th >> 6
        if not w * 64 < ne // 2:
            continue                             # the wavefront stores 1 for itself
        act = th < ne // 2
        ep = 2 * th if act else 0
        assert bin_of(ep >> 6, (ep & 63) >> 4) == bin_of((ep + 1) >> 6, ((ep + 1) & 63) >> 4)
        if act and bin_of(ep >> 6, (ep & 63) >> 4) < M:
            tested += [ep, ep + 1]
    assert len(tested) == len(set(tested)) and set(tested) == real_elements(ms, M)


@pytest.mark.parametrize("M", range(1, 33))
def test_one_member_every_real_element_has_one_tester(M):
    """thread th holds e0 = th and, where it is < NE, e1 = th + 256"""
    ms = msteps_of(M)
    ne = 64 * ms
    tested = []
    for th in range(AW * 64):
        e0, e1 = th, th + AW * 64
        if e0 < ne and bin_of(e0 >> 6, (e0 & 63) >> 4) < M:
            tested.append(e0)
        if e1 < ne and bin_of(e1 >> 6, (e1 & 63) >> 4) < M:
            tested.append(e1)
    assert len(tested) == len(set(tested)) and set(tested) == real_elements(ms, M)


def test_the_elements_left_out_are_the_image_s_zeros():
    """bins >= M of the B-operand image are exact zeros wherever V is formed (the dictionary's fragments are zero there)"""
    for M in (20, 25):
        ms = msteps_of(M)
        assert len(real_elements(ms, M)) == 16 * M and 64 * ms - 16 * M == 16 * (4 * ms - M)


# ---------------------------------------------------------------------------------------------------------------------
# the code object


def sweep_checks(lines, sweep, what):
    runs = [r for r in mfma_runs(lines) if len(r) == sweep]
    segs = [lines[r[0]:r[-1] + 1] for r in runs]
    lds = [s for s in segs if not any(re.search(r"\b(buffer|global|flat)_load", l) for l in s)]
    assert len(lds) == 1, (what, len(lds))
    seg = lds[0]
    assert not any("scratch_" in l for l in seg), what
    assert not any("ds_read2" in l for l in seg), what
    # the per-unit range test (three subtractions, v_max, v_max3, a compare) is not in the sweep's straight line: each
    # unit branches over it on the sweep's scalar flag
    assert sum(1 for l in seg if "v_max3_u32" in l) == 0, what
    assert sum(1 for l in seg if re.search(r"\bs_cbranch_(vccz|vccnz|scc0|scc1)\b", l)) >= AKT, what
    # ... and it is still there for the sweeps that need it
    assert sum(1 for l in lines if "v_max3_u32" in l) >= AKT, what


def test_code_object_of_the_c2_instances(device_asm):  # noqa: F811
    ms, mt = 7, 2
    seen = 0
    for k_ms, c, lines, group in lone_kernels(device_asm):
        if (k_ms, c) == (ms, 8):
            seen += 1
            assert group <= LDS_BYTES
            sweep_checks(lines, AKT * (ms - 1 + 4 * mt), "k_fused_lone<7, 8>")
    for k_ms, c, kl, lines, group in kernels(device_asm):
        if (k_ms, c, kl) == (ms, 8, False):
            seen += 1
            pr, on, rest = shape(ms, c, kl)
            assert on and rest + 8 * 32 * 16 * pr - 256 <= group <= LDS_BYTES
            sweep_checks(lines, AKT * (ms + 4 * mt), "k_fused_all<7, 8, false>")
    assert seen == 2


def test_the_instances_keep_their_names(device_asm):  # noqa: F811
    old = re.findall(r"^_ZN3evc11k_fused_allILi\dELin?\d+ELb[01]EEEvNS_9FusedArgsE:", device_asm, re.M)
    lone = re.findall(r"^_ZN3evc12k_fused_loneILi7ELi[248]EEEvNS_9FusedArgsE:", device_asm, re.M)
    assert len(old) == len(set(old)) == 87 and len(lone) == len(set(lone)) == 3
