"""Which block shape and split count the two contraction kernels run with (csrc/evc_gemm_plan.h), without a device.

tests/gemm_plan_host_main.hip, a program of its own built with the host half of hipcc, prints the plans of gemm_nt,
gemm_nt_mu, gemm2 and gemm2_mu over a fixed grid.  tests/golden/gemm_plan.json holds what the same program printed from
a literal copy of the conditions as they stood inside csrc/evc_gemm.hip and csrc/evc_gemm2.hip on the commit before the
header existed (tools/make_golden_gemm_plan.py --parent).  The lines must be the same, one by one; every way through the
four rules is taken somewhere on the grid; the Python restatement that tests/test_gpu_gemm_steps.py asserts
evc_solve_info.variant with agrees with the program on every line; the instances the plans can name are the ones in the
built library; and the program runs clean under the address and undefined-behaviour sanitizers.  Also here, because it
needs no device: the data of the GPU stop tests keep their stop iterations when the tolerance is halved or doubled."""
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import make_golden_gemm_plan as g  # noqa: E402
import test_gpu_gemm_steps as steps  # noqa: E402

with open(g.OUT) as f:
    GOLDEN = json.load(f)["lines"]

N_BRANCHES = 24


@pytest.fixture(scope="module")
def printed():
    return g.lines()


def of_kind(lines, kind):
    return [ln for ln in lines if ln.startswith(kind + " ")]


def test_the_fixture_is_small_and_covers_every_kind():
    assert os.path.getsize(g.OUT) < 128 * 1024
    for kind, at_least in (("nt", 800), ("g2", 800), ("ntmu", 100), ("g2mu", 600), ("use2", 2), ("branch", N_BRANCHES)):
        assert len(of_kind(GOLDEN, kind)) >= at_least, kind
    for n_cus in (64, 256, 304):
        assert any(ln.split()[5] == str(n_cus) for ln in of_kind(GOLDEN, "nt"))
        assert any(ln.split()[4] == str(n_cus) for ln in of_kind(GOLDEN, "g2mu"))
    assert {ln.split()[6] for ln in of_kind(GOLDEN, "g2")} == {"0", "1"}      # with and without scratch


def test_every_branch_of_the_four_rules_is_reached(printed):
    branches = {ln.split()[1]: int(ln.split()[2]) for ln in of_kind(printed, "branch")}
    print(branches)
    assert len(branches) == N_BRANCHES
    assert all(n > 0 for n in branches.values()), branches
    for rule in ("nt.", "ntmu.", "g2.", "g2mu."):
        assert any(b.startswith(rule) for b in branches)


@pytest.mark.parametrize("kind", ["#", "nt", "ntmu", "g2", "g2mu", "use2", "branch"])
def test_lines_are_those_of_the_parent(printed, kind):
    have, want = of_kind(printed, kind), of_kind(GOLDEN, kind)
    assert len(have) == len(want)
    for h, w in zip(have, want):
        assert h == w


def test_the_whole_output_is_the_parents(printed):
    assert printed == GOLDEN


def test_the_python_restatement_agrees_on_the_whole_grid(printed):
    n = 0
    for ln in printed:
        if ln.startswith(("#", "branch", "use2")):
            continue
        ins, outs = (list(map(int, part.split())) for part in ln.split(" ", 1)[1].split(":"))
        kind = ln.split()[0]
        if kind == "nt":
            I, J, Kd, ldc, n_cus, have, se = ins
            got = steps.plan_nt(I, J, Kd, ldc, n_cus, bool(have), se)
        elif kind == "ntmu":
            got = steps.plan_nt_mu(*ins)
        elif kind == "g2":
            I, J, Kd, ldc, n_cus, have, se = ins
            got = steps.plan_g2(I, J, Kd, ldc, n_cus, bool(have), se)
        else:
            assert kind == "g2mu", ln
            got = steps.plan_g2_mu(*ins)
        assert list(got) == outs, ln
        n += 1
    assert n == len(printed) - len(of_kind(printed, "#")) - len(of_kind(printed, "branch")) - 2


def test_expected_variant_of_the_step_cases_on_256_cus():
    """the sizes of tests/test_gpu_gemm_steps.py's cases reach the instance each was written for"""
    ev = steps.expected_variant
    assert ev(8, 40, 1000, 1950, 256) == ("k_gemm_nt", {"update": (64, 128), "v": (64, 64), "v_splits": 2, "p": (64, 128),
                                                        "deep": False})
    assert ev(8, 40, 1000, 2100, 256)[1]["update"] == (128, 128) and ev(8, 40, 1000, 2100, 256)[1]["p"] == (128, 128)
    assert ev(8, 40, 1000, 2100, 256, "gram")[1]["v"] is None
    assert ev(8, 150, 128, 11008, 256)[1]["v"] == (128, 64)
    assert ev(8, 1030, 128, 1984, 256)[1]["v"] == (64, 64) and ev(8, 1030, 128, 1984, 256)[1]["v_splits"] == 1
    assert [ev(8, 40, N, 70, 256)[1]["v_splits"] for N in (100, 256, 384, 512, 896)] == [2, 4, 6, 8, 8]
    for M in (16, 20, 40, 65, 100, 130):
        assert ev(4, M, 200, 100, 256)[1]["update"] == (64, 64)
    assert ev(4, 40, 2048, 3072, 256)[1] == {"update": (64, 128), "v": (64, 64), "v_splits": ev(4, 40, 2048, 3072, 256)[1]["v_splits"],
                                             "p": (64, 128), "deep": False}
    assert ev(4, 40, 4096, 8192, 256)[1]["update"] == (128, 128)
    assert ev(4, 201, 128, 24576, 256)[1]["v"] == (64, 128)
    assert ev(4, 40, 128, 2200, 256, loss="kl")[1]["p"] is None
    for n_cus in (64, 256, 304):
        assert ev(4, 40, 2048, steps.frames_update_shape2(n_cus), n_cus)[1]["update"] == (64, 128)
        assert ev(4, 40, 4096, steps.frames_update_shape1(n_cus), n_cus)[1]["update"] == (128, 128)
        assert ev(4, 201, 128, steps.frames_plain_wide(n_cus, 2), n_cus)[1]["v"] == (64, 128)
        assert ev(4, 40, 128, steps.stop_frames(4, n_cus, True), n_cus)[1]["update"] == (64, 128)


def _nm():
    import shutil
    for c in ("nm", "/opt/rocm/llvm/bin/llvm-nm"):
        if shutil.which(c) or os.path.exists(c):
            return c
    pytest.fail("no nm on this machine to list the library's symbols")


def test_gemm_instance_inventory(printed):
    """every k_gemm_nt<BM, BN, MU> and k_gemm2 shape the plans can name is in the built library and is run step by step
    by tests/test_gpu_gemm_steps.py, and the library holds no other - but for the ones only diagnostic builds reach
    (k_gemm2's deep-slab case 0, its 128 x 128 plain product and all of float64 k_gemm2), listed as such and not tested"""
    from exemplars_vc_amd import _lib
    out = subprocess.run([_nm(), "-C", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    nt = {(t, int(bm), int(bn), mu == "true")
          for t, bm, bn, mu in re.findall(r"k_gemm_nt<(\w+), (\d+), (\d+), \d+, \d+, (true|false)>", out)}
    g2 = set()
    for t, bf, br, bk, mu, depth in re.findall(r"k_gemm2<(\w+), (\d+), (\d+), \d+, \d+, (\d+), (true|false), \d+, (\d+)>", out):
        deep = int(bk) * (4 if t == "float" else 8) == 256
        shape = 0 if deep else {(128, 128): 1, (64, 128): 2, (64, 64): 3}[(int(bf), int(br))]
        assert (int(depth) == 2) == (shape == 3)
        g2.add((t, shape, mu == "true"))
    assert nt and g2, "no k_gemm_nt / k_gemm2 symbols found"
    # what the plans name over the grid (both element sizes go through the same k_gemm_nt rules: float32 operands that are
    # not 16-byte aligned, Griffin-Lim's frames at odd hops, run on k_gemm_nt<float>)
    named_nt = {(int(ln.split()[-3]), int(ln.split()[-2]), False) for ln in of_kind(printed, "nt")}
    named_nt |= {(int(ln.split()[-2]), int(ln.split()[-1]), True) for ln in of_kind(printed, "ntmu")}
    named_g2 = {(int(ln.split(":")[1].split()[0]), False) for ln in of_kind(printed, "g2")}
    named_g2 |= {(int(ln.split(":")[1].split()[0]), True) for ln in of_kind(printed, "g2mu")}
    assert named_nt == set(steps.INSTANCES["k_gemm_nt"]), named_nt ^ set(steps.INSTANCES["k_gemm_nt"])
    assert named_g2 == set(steps.INSTANCES["k_gemm2"]), named_g2 ^ set(steps.INSTANCES["k_gemm2"])
    assert nt == {(t,) + i for t in ("double", "float") for i in named_nt}, nt
    assert {i[1:] for i in g2 if i[0] == "float"} == named_g2 | steps.DIAGNOSTIC_ONLY["k_gemm2"]
    assert not (named_g2 & steps.DIAGNOSTIC_ONLY["k_gemm2"])
    # float64 k_gemm2: instantiated, reached with -DEVC_DIAG_GEMM2_F64 only
    assert {i[1:] for i in g2 if i[0] == "double"} == {i[1:] for i in g2 if i[0] == "float"}
    assert of_kind(printed, "use2") == ["use2 4 : 1", "use2 8 : 0"]


@pytest.mark.parametrize("esize", [4, 8])
@pytest.mark.parametrize("loss", ["frobenius", "kl"])
@pytest.mark.parametrize("who", ["some", "all"])
def test_stop_iterations_of_the_gpu_stop_cases_do_not_move_with_the_tolerance(esize, loss, who):
    """test_l_stopped_utterances compares n_iter of a float32 / float64 solve with the float64 oracle's: the data must not
    sit near a decision.  Half and double the tolerance give the same stop iterations (2200 frames; the long float32
    case has the same utterances but for a longer third one)"""
    W_rows, X_rows, offs = steps.stops_problem(esize, 2200)
    tol = steps.STOP_TOLS[who][loss]
    want = [n for _, n in steps.stops_reference(W_rows, X_rows, offs, loss, tol)]
    print(who, loss, want)
    if esize == 8 and who == "some":      # a stopped frame that went on being updated would be seen: H_12 is not H_4
        for u in (1, 3):
            Xu = X_rows[offs[u]:offs[u + 1]]
            far = steps.stops_reference(W_rows, Xu, [0, len(Xu)], loss, 0.0)[0][0]      # (tol 0: never stops)
            near = steps.stops_reference(W_rows, Xu, [0, len(Xu)], loss, tol)[0][0]
            assert steps.score(far, near) > 10 * steps.RTOL
    for f in (0.5, 2.0):
        assert [n for _, n in steps.stops_reference(W_rows, X_rows, offs, loss, tol * f)] == want, f
    if who == "some":
        assert want == [steps.STOP_ITERS, 4, steps.STOP_ITERS, 4], want
    else:
        assert max(want) <= steps.STOP_ITERS // 2, want


def test_the_program_runs_clean_under_the_sanitizers(printed):
    """a stand-alone program: address + undefined-behaviour sanitizers on the host code, nothing preloaded anywhere"""
    assert g.lines(sanitize=True) == printed
