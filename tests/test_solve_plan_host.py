"""What evc_nmf_solve / evc_nmf_convert decide and carve before they launch anything (csrc/evc_solve_plan.h), without a device.

tests/solve_plan_host_main.hip, a program of its own built with the host half of hipcc and linked against the library for the
layout functions, prints every field of plan_route, every field of plan_fused_tail and the byte offsets of every sub-array of
carve<T>, carve_wide<T> and dict_image<T> over a fixed grid.  tests/golden/solve_plan.json holds what the same program printed
on the commit before the header existed (tools/make_golden_solve_plan.py --parent: plan_route and the carvers were local to
csrc/evc_api.hip then, and the tail of a fused attempt was decided inside the launch loop, whose conditions that build
restates literally).  The lines must be the same, one by one; the tail plan also keeps the invariants its readers rely on,
over every combination of its inputs; and the program runs clean under the address and undefined-behaviour sanitizers."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import make_golden_solve_plan as g  # noqa: E402

KERNEL_FUSED_ALL = 5
Y_NONE, Y_SLABS, Y_PREPASS, Y_ROWS = range(4)

with open(g.OUT) as f:
    GOLDEN = json.load(f)["lines"]


@pytest.fixture(scope="module")
def printed():
    return g.lines()


def of_kind(lines, kind):
    return [ln for ln in lines if ln.startswith(kind + " ")]


def test_the_fixture_is_small_and_covers_every_kind():
    assert os.path.getsize(g.OUT) < 128 * 1024
    for kind, at_least in (("route", 400), ("tail", 24), ("carve", 100), ("wide", 25), ("dict", 100), ("branch", 26)):
        assert len(of_kind(GOLDEN, kind)) >= at_least, kind


def test_every_branch_of_plan_route_and_use_wide_is_reached(printed):
    branches = {ln.split()[1]: int(ln.split()[2]) for ln in of_kind(printed, "branch")}
    print(branches)
    assert len(branches) == 26
    assert all(n > 0 for n in branches.values()), branches


@pytest.mark.parametrize("kind", ["#", "route", "branch", "tail", "carve", "wide", "dict"])
def test_lines_are_those_of_the_parent(printed, kind):
    have, want = of_kind(printed, kind), of_kind(GOLDEN, kind)
    assert len(have) == len(want)
    for h, w in zip(have, want):
        assert h == w


def test_the_whole_output_is_the_parents(printed):
    assert printed == GOLDEN


def tails(lines):
    """((kernel, direct_export, iters, given, want_h, synth, packed_synth, slabs), the plan's seven fields) of every input"""
    for ln in of_kind(lines, "tail"):
        ins, outs = ln[5:].split(" :")
        plans = outs.split()
        assert len(plans) == 32
        for bits, plan in enumerate(plans):
            yield tuple(map(int, ins.split())) + tuple((bits >> b) & 1 for b in range(5)), tuple(map(int, plan))


def test_tail_plan_invariants(printed):
    seen = set()
    for (kernel, direct_export, iters, given, want_h, synth, packed, slabs), \
            (direct_h, y_in_kernel, skip_hp, variant, export_h, y_from, check_first) in tails(printed):
        seen.add((kernel, direct_export, iters, given, want_h, synth, packed, slabs))
        # skip_hp: nothing after the launch reads the packed tiles (the export of H, the two-pass synthesis, the rows)
        if skip_hp:
            assert not export_h and y_from in (Y_NONE, Y_SLABS)
        if y_in_kernel:
            assert kernel == KERNEL_FUSED_ALL and direct_export and iters > 0
        assert not (direct_h and given)
        assert (variant != 0) == bool(y_in_kernel)
        # what the drivers take for granted beyond the four: H reaches the caller exactly once when wanted, Y from one place
        assert direct_h + export_h == want_h
        assert (y_from == Y_NONE) == (not synth) and (y_from == Y_SLABS) == bool(y_in_kernel)
        assert check_first == given
        if iters == 0:      # no last launch
            assert not (direct_h or y_in_kernel or skip_hp or variant)
    assert len(seen) == 4 * 2 * 3 * 32      # kernels x direct_export x iters x the five switches


def test_the_program_runs_clean_under_the_sanitizers(printed):
    """a stand-alone program: address + undefined-behaviour sanitizers on the host code, nothing preloaded anywhere"""
    assert g.lines(sanitize=True) == printed
