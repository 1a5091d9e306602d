"""k_fused_quad (evc_fused_all.hip, EVC_ALL_LONE 2; `-m gpu`): k_fused_lone at M = 25 with bins 16 .. 24 of V' on twelve
v_mfma_f64_4x4x4_4b_f64 per unit instead of a second 16-row tile - against the float64 oracle and against k_fused_lone
(quad_rows=False, EVC_FLAG_NO_QUAD_ROWS).

evc_solve_info reports k_fused_all for all three kernels.  Per accumulator the products are grouped as in k_fused_lone (by
exemplar register, contracting the four lane groups); only the hardware's order inside a 4-term dot product may differ, so
the two results are bit-identical or differ in the last places - each test prints which, none asserts either.  That the
small MFMAs ran and ran right shows in the dictionaries that live in bins 16 .. 24 alone.

Shapes of tests/test_gpu_fused_lone.py: T = 33 frames (two full frame tiles and one frame into a third), 30 iterations,
N = 1024 / 2048 / 4096 (2, 4, 8 members).  Tolerances: that file's RTOL64 against the oracle and between the kernels
(float64, summation order only); one float32 ulp (2^-23) for the float32 caller.

With quad_rows=False the call is the parent's, bit for bit: PARENT_DIGESTS holds sha256 of the activations of FLAG_OFF_CASES
run with the library of the commit before k_fused_quad.
"""
import hashlib

import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu

RTOL64 = 1e-8
T, K = 33, 30
IN_KERNEL = {"y_in_kernel": True, "packed_h_stored": False}
EPS = {"zero_replace": ("EPS_ZERO_REPLACE", "SK_EPSILON"), "add": ("EPS_ADD", "PYMF_EPS_ADD"), "clamp": ("EPS_CLAMP", None)}


def oracle():
    from oracle import evc_oracle
    return evc_oracle


def assert_close64(got, want, what, rtol=RTOL64):
    r, z = rel_err(got, want)
    print(f"{what}: max rel err {r:.3e}, max |got| where want==0 {z:.3e}")
    assert r <= rtol and z == 0.0, f"{what}: max rel err {r:.3e}, max |got| where want==0 {z:.3e}"


def same_bits(a, b, what):
    same = np.array_equal(a, b)
    print(f"{what}: k_fused_quad and k_fused_lone are {'bit-identical' if same else 'different in the last places'}")
    return same


_problems = {}


def problem(M, N, frames=T):
    key = (M, N, frames)
    if key not in _problems:
        p = oracle().synth_problem(M, N, frames, seed=2500 + M + N // 512)
        p["H0"] = np.random.default_rng(M + N).random((N, frames)) * 0.02 + 1e-4
        for v in p.values():
            v.setflags(write=False)
        _problems[key] = p
    return _problems[key]


def routed(info, N):
    return (info["kernel"], info["members"], info["redo"], info["exchange"]) == ("k_fused_all", N // 512, 0, 1)


@pytest.mark.parametrize("eps_mode", ["zero_replace", "add", "clamp"])
@pytest.mark.parametrize("start", ["const", "given"])
@pytest.mark.parametrize("l1", [0.0, 0.25])
@pytest.mark.parametrize("N", [1024, 2048, 4096])
def test_against_the_oracle_and_k_fused_lone(N, l1, start, eps_mode):
    import exemplars_vc_amd as evc
    o = oracle()
    p = problem(25, N)
    what = f"N={N} l1={l1} {start} {eps_mode}"
    mode, eps_name = EPS[eps_mode]
    eps = getattr(o, eps_name) if eps_name else 1e-15
    kw = dict(iters=K, eps_mode=eps_mode, eps=eps, l1=l1)
    if start == "const":
        H0, kw["init"] = np.full((N, T), np.sqrt(p["X"].mean() / N)), "sklearn"
        call = lambda **more: evc.solve_activations(p["A"], p["X"], **kw, **more)
    else:
        H0 = p["H0"]
        call = lambda **more: evc.solve_activations(p["A"], p["X"], H0.copy(), **kw, **more)
    H_on, i_on = call(quad_rows=True, info=True)
    H_off, i_off = call(quad_rows=False, info=True)
    assert routed(i_on, N) and routed(i_off, N), (what, i_on, i_off)
    same_bits(H_on, H_off, what)
    assert_close64(H_on, H_off, what + ": vs quad_rows=False")
    want = o.mu_solve(p["A"], p["X"], H0, K, eps_mode=getattr(o, mode), eps=eps, l1=l1, algo="factored")
    assert_close64(H_on, want, what + ": vs the oracle")


def upper_bins_only(N, one_per_lane_group):
    """a dictionary that is zero in bins 0 .. 15: V lives in the small MFMAs alone.  one_per_lane_group: of the exemplars
    4 q .. 4 q + 3 of every tile only one is non-zero - which one (the accumulator's register r) changes with q and the tile"""
    p = problem(25, N)
    A, X = p["A"].copy(), p["X"].copy()
    A[:16] = 0.0
    if one_per_lane_group:
        n = np.arange(N)
        A[:, (n & 3) != ((n >> 2) + (n >> 4)) & 3] = 0.0
    rng = np.random.default_rng(N)
    Hs = rng.random((N, T)) * (rng.random((N, T)) < 0.02)
    X = A @ Hs + 1e-6
    X[:16] = 0.0
    return A, X, p["H0"]


@pytest.mark.parametrize("one_per_lane_group", [False, True])
@pytest.mark.parametrize("N", [1024, 2048, 4096])
def test_a_dictionary_that_is_zero_in_bins_0_to_15(N, one_per_lane_group):
    import exemplars_vc_amd as evc
    o = oracle()
    A, X, H0 = upper_bins_only(N, one_per_lane_group)
    what = f"N={N} bins 16..24 only, one exemplar per lane group: {one_per_lane_group}"
    kw = dict(iters=K, eps_mode="add", eps=o.PYMF_EPS_ADD)
    H_on, info = evc.solve_activations(A, X, H0.copy(), info=True, **kw)
    H_off = evc.solve_activations(A, X, H0.copy(), quad_rows=False, **kw)
    assert routed(info, N), info
    same_bits(H_on, H_off, what)
    want = o.mu_solve(A, X, H0, K, eps_mode=o.EPS_ADD, eps=o.PYMF_EPS_ADD, algo="factored")
    assert np.isfinite(want).all() and (want > 0).any()
    assert_close64(H_on, want, what + ": vs the oracle")
    assert_close64(H_on, H_off, what + ": vs quad_rows=False")
    # V itself, through the in-kernel synthesis with B = A: bins 16 .. 24 are what the small MFMAs' operands produce
    _, Y = evc.convert(A, X, A, H0.copy(), **kw)
    assert_close64(Y, A @ want, what + ": A H vs the oracle")


@pytest.mark.parametrize("N", [1024, 4096])
def test_batch_equals_solo_and_run_equals_rerun_bitwise(N):
    import exemplars_vc_amd as evc
    p = problem(25, N, 96)
    kw = dict(iters=K, eps_mode="zero_replace", init="const", init_value=0.01)
    H1, i1 = evc.solve_activations(p["A"], p["X"], info=True, **kw)
    H2 = evc.solve_activations(p["A"], p["X"], **kw)
    assert routed(i1, N), i1
    assert np.array_equal(H1, H2)
    Hs = evc.solve_activations(p["A"], np.ascontiguousarray(p["X"][:, :48]), **kw)
    assert np.array_equal(H1[:, :48], Hs)
    assert np.array_equal(H1, evc.solve_activations(p["A"], p["X"], range_hoist=False, **kw))


@pytest.mark.parametrize("N", [1024, 4096])
def test_the_exact_path_with_an_all_zero_frame(N):
    """l1 = 0 under zero_replace: the zero frame's activations are 0 after one update, its denominators 0 from then on -
    every tile of that frame's lanes takes the update's exact path"""
    import exemplars_vc_amd as evc
    o = oracle()
    p = problem(25, N)
    X = p["X"].copy()
    X[:, 5] = 0.0
    kw = dict(iters=K, eps_mode="zero_replace", l1=0.0)
    H_on, info = evc.solve_activations(p["A"], X, p["H0"].copy(), info=True, **kw)
    H_off = evc.solve_activations(p["A"], X, p["H0"].copy(), quad_rows=False, **kw)
    assert routed(info, N), info
    assert np.array_equal(np.isnan(H_on), np.isnan(H_off)) and np.array_equal(np.isinf(H_on), np.isinf(H_off))
    want = o.mu_solve(p["A"], X, p["H0"], K, eps_mode=o.EPS_ZERO_REPLACE, eps=o.SK_EPSILON, l1=0.0, algo="factored")
    assert np.array_equal(np.isnan(H_on), np.isnan(want)) and np.array_equal(np.isinf(H_on), np.isinf(want))
    assert (H_on[:, 5] == 0.0).all() and (want[:, 5] == 0.0).all()
    assert_close64(H_on, want, f"N={N}: zero frame, vs the oracle")
    assert np.array_equal(H_on, evc.solve_activations(p["A"], X, p["H0"].copy(), range_hoist=False, **kw))


def test_three_launches_of_ten_are_one_launch_of_thirty_bitwise():
    import exemplars_vc_amd as evc
    p = problem(25, 2048)
    kw = dict(iters=K, eps_mode="zero_replace", init="sklearn")
    H3, i3 = evc.solve_activations(p["A"], p["X"], check_every=10, info=True, **kw)
    H1, i1 = evc.solve_activations(p["A"], p["X"], info=True, **kw)
    assert routed(i3, 2048) and routed(i1, 2048) and (i3["launches"], i1["launches"]) == (3, 1), (i3, i1)
    assert np.array_equal(H3, H1)
    assert np.array_equal(H1, evc.solve_activations(p["A"], p["X"], range_hoist=False, **kw))


@pytest.mark.parametrize("N", [1024, 4096])
def test_convert_forms_y_in_the_kernel(N):
    import exemplars_vc_amd as evc
    p = problem(25, N)
    kw = dict(iters=K, eps_mode="zero_replace", init="sklearn")
    H, Y, info = evc.convert(p["A"], p["X"], p["B"], info=True, **kw)
    assert routed(info, N) and info["variant"] == IN_KERNEL, info
    assert_close64(Y, p["B"] @ H, f"Y, N={N}")
    assert np.array_equal(H, evc.solve_activations(p["A"], p["X"], **kw))
    H_off, Y_off, i_off = evc.convert(p["A"], p["X"], p["B"], info=True, quad_rows=False, **kw)
    assert i_off["variant"] == IN_KERNEL
    same_bits(H, H_off, f"convert, N={N}")
    assert_close64(Y, Y_off, f"Y vs quad_rows=False, N={N}")


def test_a_float32_caller():
    import exemplars_vc_amd as evc
    o = oracle()
    p = problem(25, 1024)
    A, X, H0 = (p[k].astype(np.float32) for k in ("A", "X", "H0"))
    kw = dict(iters=K, eps_mode="zero_replace")
    H, info = evc.solve_activations(A, X, H0.copy(), info=True, **kw)
    assert H.dtype == np.float32 and routed(info, 1024), info
    want = o.mu_solve(A.astype(np.float64), X.astype(np.float64), H0.astype(np.float64), K, eps_mode=o.EPS_ZERO_REPLACE,
                      eps=o.SK_EPSILON, algo="factored")
    assert_close64(H, want, "float32 caller vs the float64 oracle", rtol=2.0 ** -23)
    assert_close64(H, evc.solve_activations(A, X, H0.copy(), quad_rows=False, **kw), "float32 caller vs quad_rows=False",
                   rtol=2.0 ** -23)


@pytest.mark.parametrize("N", [1024, 4096])
def test_a_voided_launch_is_redone_without_exchange(N):
    import exemplars_vc_amd as evc
    p = problem(25, N)
    kw = dict(iters=K, eps_mode="add")
    want, iw = evc.solve_activations(p["A"], p["X"], p["H0"].copy(), cooperative=False, info=True, **kw)
    got, ig = evc.solve_activations(p["A"], p["X"], p["H0"].copy(), _fake_coop_timeout=True, info=True, **kw)
    assert ig["redo"] == 1 and ig["exchange"] == 0 and iw["redo"] == 0, (ig, iw)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("M,N,loss", [(24, 1024, "frobenius"), (26, 1024, "frobenius"), (21, 1024, "frobenius"),
                                      (25, 16384, "frobenius"), (25, 512, "frobenius"), (25, 1536, "frobenius"),
                                      (25, 1024, "kl")])
def test_other_shapes_are_not_routed(M, N, loss):
    """one k-step less or a full last k-step, 32 members, one member, three members (ragged slices), KL: the flag changes
    nothing, bit for bit"""
    import exemplars_vc_amd as evc
    p = problem(M, N)
    kw = dict(iters=10, eps_mode="zero_replace", loss=loss)
    H_on, i_on = evc.solve_activations(p["A"], p["X"], p["H0"].copy(), quad_rows=True, info=True, **kw)
    H_off, i_off = evc.solve_activations(p["A"], p["X"], p["H0"].copy(), quad_rows=False, info=True, **kw)
    assert i_on["kernel"] == i_off["kernel"] and i_on["members"] == i_off["members"], (i_on, i_off)
    if loss == "frobenius":
        assert i_on["kernel"] == "k_fused_all", i_on
    assert np.isfinite(H_on).all() and np.array_equal(H_on, H_off)


# ---- quad_rows=False is the parent's call, bit for bit

def flag_off_case(N, eps_mode, start, l1):
    import exemplars_vc_amd as evc
    o = oracle()
    p = problem(25, N)
    _, eps_name = EPS[eps_mode]
    kw = dict(iters=K, eps_mode=eps_mode, eps=getattr(o, eps_name) if eps_name else 1e-15, l1=l1, quad_rows=False)
    if start == "const":
        return evc.solve_activations(p["A"], p["X"], init="sklearn", **kw)
    return evc.solve_activations(p["A"], p["X"], p["H0"].copy(), **kw)


FLAG_OFF_CASES = {f"N{N}_{eps_mode}_{start}_l1_{l1}": (N, eps_mode, start, l1)
                  for N, eps_mode, start, l1 in [(1024, "zero_replace", "const", 0.0), (1024, "add", "given", 0.25),
                                                 (2048, "clamp", "given", 0.0), (2048, "zero_replace", "const", 0.25),
                                                 (4096, "zero_replace", "given", 0.0), (4096, "add", "const", 0.25)]}

# sha256 of the float64 activations, printed by this file's cases run with the parent commit's library (EVC_LIB)
PARENT_DIGESTS = {
    "N1024_add_given_l1_0.25": "3a6e61122fd8341d0842b331a55818cbc2071306bfd4e7562e11f2053d74d070",
    "N1024_zero_replace_const_l1_0.0": "2e152704ba2a19612f1de0acc53149cdd5cf55d36144b83f85b3651e0fd0a2af",
    "N2048_clamp_given_l1_0.0": "d6cdc11077205d5148743387e48ff4d6cd19e397032dee4c06f8704c4a4b758f",
    "N2048_zero_replace_const_l1_0.25": "981d3640c8364497f90cd1b2787034f1150560d2230ec4e1f359fe169e1910be",
    "N4096_add_const_l1_0.25": "9a71b3214eb86ac307fa494fae121125539c37a7d21e7c68cb709bfc46e2858d",
    "N4096_zero_replace_given_l1_0.0": "3bdf7229e1d3ad2d5badf811fa7fd82fab960389f7523e0397e5c14ac035321b",
}


def digest(H):
    return hashlib.sha256(np.ascontiguousarray(H, dtype=np.float64).tobytes()).hexdigest()


@pytest.mark.parametrize("case", sorted(FLAG_OFF_CASES))
def test_with_the_flag_off_the_parent_runs_bit_for_bit(case):
    got = digest(flag_off_case(*FLAG_OFF_CASES[case]))
    print(case, got)
    assert got == PARENT_DIGESTS[case]
