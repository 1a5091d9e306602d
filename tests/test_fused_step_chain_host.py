"""One vector phase per unit in the sweeps of k_fused_lone and of k_fused_all with one member or the direct exchange
(evc_fused_all_body.inc), without a GPU.

A unit of a sweep is a chain of D MFMAs, the update (vector instructions) and the V' MFMAs.  The update is closed towards
the V' MFMAs by a scheduling barrier, so that the last h *= q and the next unit's lone-bin fold issue before the unit's
first V' MFMA, and V' and the next D chain run back to back.  The reduce-scatter instances (template C <= 0) are left
as the compiler orders them: their step is the exchange, which shares its SIMDs with the sweep, and with the barrier C5
(32 members) measured 0.8 % slower (profiles/step_chain_README.md); nothing is asserted about their phases.

The code object, compiled as tests/test_fused_all_lds_host.py compiles it.  A vector phase is a stretch between two
consecutive MFMAs that holds at least one vector instruction that is not an MFMA (LDS reads, waits and scalar
instructions do not count).  In every instance of k_fused_lone and every instance of k_fused_all with C >= 1 (55 of its
87, Frobenius and KL) the sweep's MFMA run - AKT * (MSTEPS + 4 MT) MFMAs,
AKT * 14 in k_fused_lone - holds exactly AKT vector phases.

Where the sweep is: MFMAs less than 200 lines apart are one run (mfma_runs).  The compiler lays some passes straight
next to the sweep, so a run may be longer than the sweep; the lengths that occur are pinned here, and the sweep is then
  Frobenius: the run's last MFMAs - what stands in front is the numerator pass (one member: all of it, AKT * MSTEPS; two
             k-steps or fewer with the dictionary in LDS likewise);
  KL:        the run's first MFMAs - there is no numerator pass, and what stands behind is the Y pass (AKT * 4 MFMAs per
             bin tile of B, both tile counts where MT = 2) or, at one member and up to three k-steps, a second copy of the
             sweep in front of it.
(One member, Frobenius: the compiler rotates the step loop, and the textual run holds seven updates and the step's
boundary, whose stretch holds the barrier; the eighth update stands with the loop's other code.  Each is one stretch.)

Also pinned here, for every sweep found: no scratch access inside it, and the three instances of k_fused_lone take the
four lone-bin words' wait once in front of each fold (no s_waitcnt between the fold's four v_fma_f64).
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_fused_all_lds_host import AKT, kernels, mfma_runs  # noqa: E402
from test_fused_all_lds_host import device_asm  # noqa: E402,F401  (the module-scoped fixture: one compilation)
from test_fused_lone_host import lone_kernels  # noqa: E402

VECTOR = re.compile(r"^\s+v_(?!mfma)")


def stretches(lines, idx):
    """the lines between consecutive MFMAs of idx"""
    return [lines[a + 1:b] for a, b in zip(idx, idx[1:])]


def vector_phases(lines, idx):
    return [s for s in stretches(lines, idx) if any(VECTOR.match(l) for l in s)]


def sweeps_of(lines, sweep, ms, mt, c, kl):
    """the MFMA line numbers of every copy of the sweep in one kernel (see the module's text)"""
    y_pass = AKT * 4 * mt + (AKT * 4 if mt == 2 else 0)
    out = []
    for r in mfma_runs(lines):
        if len(r) < sweep:
            continue
        extra = len(r) - sweep
        layout = f"layout changed (not a phase count): instance ({ms}, {c}, {kl}) has an MFMA run of {len(r)}, the sweep is " \
                 f"{sweep} - the compiler lays the passes out differently; find the sweep anew (see the module's text)"
        if kl:
            assert extra in (0, y_pass, sweep + y_pass), layout
            out.append(r[:sweep])
        else:
            assert extra in (0, AKT * ms), layout
            out.append(r[-sweep:])
    return out


def check_sweep(lines, idx, what, closed=True):
    phases = vector_phases(lines, idx)
    if closed:
        assert len(phases) == AKT, (what, [sum(1 for l in s if VECTOR.match(l)) for s in phases])
    assert not any("scratch_" in l for l in lines[idx[0]:idx[-1] + 1]), what
    return phases


def test_one_vector_phase_per_unit_in_k_fused_all_with_one_member_or_the_direct_exchange(device_asm):  # noqa: F811
    seen = copies = closed = 0
    for ms, c, kl, lines, group in kernels(device_asm):
        seen += 1
        mt = 2 if ms > 4 else 1
        found = sweeps_of(lines, AKT * (ms + 4 * mt), ms, mt, c, kl)
        # (2: streamed and from the LDS dictionary)
        assert len(found) in (1, 2), f"layout changed (not a phase count): {len(found)} sweeps found in ({ms}, {c}, {kl})"
        for idx in found:
            copies += 1
            check_sweep(lines, idx, ("k_fused_all", ms, c, kl), closed=c >= 1)
        closed += c >= 1
    assert seen == 87 and copies >= seen and closed == 3 * 8 * 2 + 7        # C = 1, 2, 4 (Frobenius and KL) and 8


def test_one_vector_phase_per_unit_in_every_instance_of_k_fused_lone(device_asm):  # noqa: F811
    seen = []
    for ms, c, lines, group in lone_kernels(device_asm):
        seen.append((ms, c))
        runs = [r for r in mfma_runs(lines) if len(r) == AKT * 14]
        assert len(runs) == 1, f"layout changed (not a phase count): k_fused_lone<7, {c}> has MFMA runs of " \
                               f"{[len(r) for r in mfma_runs(lines)]}, none or several of {AKT * 14}"
        phases = check_sweep(lines, runs[0], ("k_fused_lone", ms, c))
        # V' and the next D chain back to back: every phase stands behind a D chain (6 MFMAs) and in front of 8 + 6
        starts = [i for i, s in enumerate(stretches(lines, runs[0])) if any(VECTOR.match(l) for l in s)]
        assert starts == [5 + 14 * k for k in range(AKT)], (c, starts)
        # the fold of the next unit (units 0 .. AKT - 2): four v_fma_f64 in a row behind one wait
        for s in phases[:-1]:
            text = "\n".join(l.split(";")[0] for l in s)
            assert re.search(r"(\s+v_fma_f64[^\n]*\n(\s*s_nop[^\n]*\n)?){4}", text + "\n"), c
            fmas = [i for i, l in enumerate(s) if re.match(r"\s+v_fma_f64", l)]
            fold = next(fmas[i:i + 4] for i in range(len(fmas) - 3) if fmas[i + 3] - fmas[i] <= 4)
            assert not any("s_waitcnt" in l for l in s[fold[0]:fold[3]]), c
    assert sorted(seen) == [(7, 2), (7, 4), (7, 8)]

