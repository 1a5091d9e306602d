"""One vector phase per unit in the sweeps of k_fused_lone and of k_fused_all with one member or the direct exchange
(template C >= 1; evc_fused_all_body.inc; `-m gpu`): the update closed towards the V' MFMAs by a scheduling barrier, the
lone-bin words waited for once per fold.  The reduce-scatter instances (C <= 0) are left as they were.

The change reorders instructions and has no switch: the arithmetic and its order are the parent's, so what is checked
on the GPU is every route it touches against the float64 oracle (oracle.mu_solve, algo="factored"; RTOL64 of
tests/test_gpu_fused_lone.py and tests/test_gpu_fused_all_step.py: float64, summation order only), run against rerun
and solve against convert() bitwise, and the switches that do exist (lone_bin, range_hoist) across the reordered code.
(That H and Y are the parent's bit for bit is recorded in profiles/step_chain_dump_cmp.txt.)

T = 16 * 3 + 5 = 53 frames in two utterances of 30 and 23: the frame tiles mix utterances and the last one is ragged
(padding frames).  One more length, 16 * 2 + 5 = 37 frames, makes three tiles: the second half of the last pair of groups
then has no tile (`valid` false) beside a half that works.  iters = 1, 2 and 30.  Shapes: M = 25 with 2, 4 and 8 members
(k_fused_lone, and k_fused_all with lone_bin=False), M = 24 and M = 6 at two members, one member (N = 512) and, as an
instance that the change leaves alone, the reduce-scatter (N = 8192).
"""
import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu

RTOL64 = 1e-8
T, UTT = 53, [0, 30, 53]
T3, UTT3 = 37, [0, 20, 37]

_problems, _wanted = {}, {}


def oracle():
    from oracle import evc_oracle
    return evc_oracle


def problem(M, N, frames=T):
    key = (M, N, frames)
    if key not in _problems:
        p = oracle().synth_problem(M, N, frames, seed=5300 + M + N // 512)
        p["H0"] = np.random.default_rng(M + N + frames).random((N, frames)) * 0.02 + 1e-4
        for v in p.values():
            v.setflags(write=False)
        _problems[key] = p
    return _problems[key]


def wanted(M, N, iters, frames=T):
    """the oracle's H for problem(M, N, frames) from its H0, computed once"""
    key = (M, N, iters, frames)
    if key not in _wanted:
        o, p = oracle(), problem(M, N, frames)
        H = o.mu_solve(p["A"], p["X"], p["H0"], iters, eps_mode=o.EPS_ZERO_REPLACE, eps=o.SK_EPSILON, algo="factored")
        H.setflags(write=False)
        _wanted[key] = H
    return _wanted[key]


def assert_close64(got, want, what, rtol=RTOL64):
    r, z = rel_err(got, want)
    print(f"{what}: max rel err {r:.3e}, max |got| where want==0 {z:.3e}")
    assert r <= rtol and z == 0.0, f"{what}: max rel err {r:.3e}, max |got| where want==0 {z:.3e}"


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def solved(A, X, H0, N, what, **kw):
    """one solve: routed to k_fused_all with N / 512 members, not redone, and the same bits when run again"""
    import exemplars_vc_amd as evc
    H, info = evc.solve_activations(A, X, H0.copy(), info=True, **kw)
    assert (info["kernel"], info["members"], info["redo"]) == ("k_fused_all", N // 512, 0), (what, info)
    assert same(H, evc.solve_activations(A, X, H0.copy(), **kw)), what
    return H


@pytest.mark.parametrize("iters", [1, 2, 30])
@pytest.mark.parametrize("lone_bin", [True, False], ids=["lone", "all"])
@pytest.mark.parametrize("N", [1024, 2048, 4096])
def test_m25_against_the_oracle(N, lone_bin, iters):
    import exemplars_vc_amd as evc
    p = problem(25, N)
    what = f"M=25 N={N} lone_bin={lone_bin} iters={iters}"
    kw = dict(iters=iters, eps_mode="zero_replace", utt_offsets=UTT, lone_bin=lone_bin)
    H = solved(p["A"], p["X"], p["H0"], N, what, **kw)
    assert_close64(H, wanted(25, N, iters), what + ": vs the oracle")
    Hc, Y = evc.convert(p["A"], p["X"], p["B"], p["H0"].copy(), **kw)
    assert same(Hc, H), what
    assert_close64(Y, p["B"] @ H, what + ": Y")


@pytest.mark.parametrize("M", [24, 6])
def test_other_widths_at_two_members(M):
    p = problem(M, 1024)
    what = f"M={M} N=1024"
    H = solved(p["A"], p["X"], p["H0"], 1024, what, iters=30, eps_mode="zero_replace", utt_offsets=UTT)
    assert_close64(H, wanted(M, 1024, 30), what + ": vs the oracle")


@pytest.mark.parametrize("N", [1024, 4096])
def test_three_tiles_one_half_without_a_tile(N):
    p = problem(25, N, T3)
    what = f"M=25 N={N} T={T3}"
    H = solved(p["A"], p["X"], p["H0"], N, what, iters=30, eps_mode="zero_replace", utt_offsets=UTT3)
    assert_close64(H, wanted(25, N, 30, T3), what + ": vs the oracle")


def test_with_the_range_test_in_front_of_every_unit():
    """range_hoist=False: the update with its test and its out-of-line exact path inside the closed vector phase"""
    p = problem(25, 4096)
    what = "M=25 N=4096 range_hoist=False"
    kw = dict(iters=30, eps_mode="zero_replace", utt_offsets=UTT)
    H = solved(p["A"], p["X"], p["H0"], 4096, what, range_hoist=False, **kw)
    assert same(H, solved(p["A"], p["X"], p["H0"], 4096, what, range_hoist=True, **kw)), what
    assert_close64(H, wanted(25, 4096, 30), what + ": vs the oracle")


def test_an_all_zero_frame():
    o = oracle()
    p = problem(25, 2048)
    X = p["X"].copy()
    X[:, 5] = 0.0
    what = "M=25 N=2048 zero frame"
    H = solved(p["A"], X, p["H0"], 2048, what, iters=30, eps_mode="zero_replace", utt_offsets=UTT)
    want = o.mu_solve(p["A"], X, p["H0"], 30, eps_mode=o.EPS_ZERO_REPLACE, eps=o.SK_EPSILON, algo="factored")
    assert (H[:, 5] == 0.0).all() and (want[:, 5] == 0.0).all()
    assert_close64(H, want, what + ": vs the oracle")


def test_a_nan_in_x():
    o = oracle()
    p = problem(25, 2048)
    X = p["X"].copy()
    X[3, 27] = np.nan
    what = "M=25 N=2048 NaN in X"
    H = solved(p["A"], X, p["H0"], 2048, what, iters=30, eps_mode="zero_replace", utt_offsets=UTT)
    with np.errstate(invalid="ignore"):
        want = o.mu_solve(p["A"], X, p["H0"], 30, eps_mode=o.EPS_ZERO_REPLACE, eps=o.SK_EPSILON, algo="factored")
    assert np.array_equal(np.isnan(H), np.isnan(want)) and np.isnan(H[:, 27]).all() and not np.isnan(H[:, :27]).any(), what
    ok = ~np.isnan(want).any(axis=0)
    assert_close64(H[:, ok], want[:, ok], what + ": the other frames vs the oracle")


def test_launches_in_pieces():
    """check_every = 10: three launches of ten iterations, each starting and ending its frame tiles - the same bits as
    one launch of thirty"""
    import exemplars_vc_amd as evc
    p = problem(25, 4096)
    kw = dict(iters=30, eps_mode="zero_replace", utt_offsets=UTT)
    H3, i3 = evc.solve_activations(p["A"], p["X"], p["H0"].copy(), check_every=10, info=True, **kw)
    assert (i3["kernel"], i3["members"], i3["redo"], i3["launches"]) == ("k_fused_all", 8, 0, 3), i3
    assert same(H3, evc.solve_activations(p["A"], p["X"], p["H0"].copy(), **kw))
    assert_close64(H3, wanted(25, 4096, 30), "three launches of ten: vs the oracle")


@pytest.mark.parametrize("N", [512, 8192])
def test_one_member_and_the_reduce_scatter(N):
    """N = 512: the streamed one-member sweep carries the closed update as well.  N = 8192 (16 members, reduce-scatter):
    that instance does not - it is here as a check that it was left alone and still agrees with the oracle"""
    p = problem(25, N)
    what = f"M=25 N={N}"
    H = solved(p["A"], p["X"], p["H0"], N, what, iters=30, eps_mode="zero_replace", utt_offsets=UTT)
    assert_close64(H, wanted(25, N, 30), what + ": vs the oracle")
