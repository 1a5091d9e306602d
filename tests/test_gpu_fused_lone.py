"""k_fused_lone (evc_fused_all.hip, EVC_ALL_LONE 1; `-m gpu`): k_fused_all at M = 25 with bin 24 folded into the
denominators' start value - 14 MFMAs per unit, not 15 - against the float64 oracle and against k_fused_all's own unit
(lone_bin=False, EVC_FLAG_NO_LONE_BIN).

evc_solve_info reports k_fused_all either way, so that the other kernel ran shows in the bits alone: bin 24 is added
first, not last, and the two results differ in the last places.  T = 33 frames: two full frame tiles and one frame into
a third; 30 iterations.  Tolerances: RTOL64 of tests/test_gpu_fused_all_step.py against the oracle and between the two
kernels (float64, summation order only); one float32 ulp (2^-23) for the float32 caller, whose result is the float64 one
narrowed.
"""
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
def test_against_the_oracle_and_the_15_mfma_unit(N, l1, start, eps_mode):
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
    H_on, i_on = call(lone_bin=True, info=True)
    H_off, i_off = call(lone_bin=False, info=True)
    assert routed(i_on, N) and routed(i_off, N), (what, i_on, i_off)
    assert not np.array_equal(H_on, H_off), what             # the other kernel ran: bin 24 first, not last
    assert_close64(H_on, H_off, what + ": vs lone_bin=False")
    want = o.mu_solve(p["A"], p["X"], H0, K, eps_mode=getattr(o, mode), eps=eps, l1=l1, algo="factored")
    assert_close64(H_on, want, what + ": vs the oracle")


@pytest.mark.parametrize("N", [1024, 4096])
def test_batch_equals_solo_and_run_equals_rerun_bitwise(N):
    import exemplars_vc_amd as evc
    p = problem(25, N, 96)
    kw = dict(iters=K, eps_mode="zero_replace", init="const", init_value=0.01, lone_bin=True)
    H1, i1 = evc.solve_activations(p["A"], p["X"], info=True, **kw)
    H2 = evc.solve_activations(p["A"], p["X"], **kw)
    assert routed(i1, N), i1
    assert np.array_equal(H1, H2)
    Hs = evc.solve_activations(p["A"], np.ascontiguousarray(p["X"][:, :48]), **kw)
    assert np.array_equal(H1[:, :48], Hs)
    assert not np.array_equal(H1, evc.solve_activations(p["A"], p["X"], **dict(kw, lone_bin=False)))


@pytest.mark.parametrize("N", [1024, 4096])
def test_the_exact_path_with_an_all_zero_frame(N):
    """l1 = 0 under zero_replace: the zero frame's numerators are 0, its activations 0 after one update, its denominators
    0 from then on - every tile of that frame's lanes takes the update's exact path, the start value of the fold is 0"""
    import exemplars_vc_amd as evc
    o = oracle()
    p = problem(25, N)
    X = p["X"].copy()
    X[:, 5] = 0.0
    kw = dict(iters=K, eps_mode="zero_replace", l1=0.0, lone_bin=True)
    H_on, info = evc.solve_activations(p["A"], X, p["H0"].copy(), info=True, **kw)
    H_off = evc.solve_activations(p["A"], X, p["H0"].copy(), **dict(kw, lone_bin=False))
    assert routed(info, N), info
    assert np.array_equal(np.isnan(H_on), np.isnan(H_off)) and np.array_equal(np.isinf(H_on), np.isinf(H_off))
    want = o.mu_solve(p["A"], X, p["H0"], K, eps_mode=o.EPS_ZERO_REPLACE, eps=o.SK_EPSILON, l1=0.0, algo="factored")
    assert np.array_equal(np.isnan(H_on), np.isnan(want)) and np.array_equal(np.isinf(H_on), np.isinf(want))
    assert (H_on[:, 5] == 0.0).all() and (want[:, 5] == 0.0).all()
    assert_close64(H_on, want, f"N={N}: zero frame, vs the oracle")
    assert not np.array_equal(H_on, H_off)


def test_three_launches_of_ten_are_one_launch_of_thirty_bitwise():
    import exemplars_vc_amd as evc
    p = problem(25, 2048)
    kw = dict(iters=K, eps_mode="zero_replace", init="sklearn", lone_bin=True)
    H3, i3 = evc.solve_activations(p["A"], p["X"], check_every=10, info=True, **kw)
    H1, i1 = evc.solve_activations(p["A"], p["X"], info=True, **kw)
    assert routed(i3, 2048) and routed(i1, 2048) and (i3["launches"], i1["launches"]) == (3, 1), (i3, i1)
    assert np.array_equal(H3, H1)
    assert not np.array_equal(H1, evc.solve_activations(p["A"], p["X"], **dict(kw, lone_bin=False)))


@pytest.mark.parametrize("N", [1024, 4096])
def test_convert_forms_y_in_the_kernel(N):
    import exemplars_vc_amd as evc
    p = problem(25, N)
    kw = dict(iters=K, eps_mode="zero_replace", init="sklearn", lone_bin=True)
    H, Y, info = evc.convert(p["A"], p["X"], p["B"], info=True, **kw)
    assert routed(info, N) and info["variant"] == IN_KERNEL, info
    assert_close64(Y, p["B"] @ H, f"Y, N={N}")
    assert np.array_equal(H, evc.solve_activations(p["A"], p["X"], **kw))
    H_off, Y_off, i_off = evc.convert(p["A"], p["X"], p["B"], info=True, **dict(kw, lone_bin=False))
    assert i_off["variant"] == IN_KERNEL and not np.array_equal(H, H_off)
    assert_close64(Y, Y_off, f"Y vs lone_bin=False, N={N}")


def test_a_float32_caller():
    import exemplars_vc_amd as evc
    o = oracle()
    p = problem(25, 1024)
    A, X, H0 = (p[k].astype(np.float32) for k in ("A", "X", "H0"))
    kw = dict(iters=K, eps_mode="zero_replace", lone_bin=True)
    H, info = evc.solve_activations(A, X, H0.copy(), info=True, **kw)
    assert H.dtype == np.float32 and routed(info, 1024), info
    want = o.mu_solve(A.astype(np.float64), X.astype(np.float64), H0.astype(np.float64), K, eps_mode=o.EPS_ZERO_REPLACE,
                      eps=o.SK_EPSILON, algo="factored")
    assert_close64(H, want, "float32 caller vs the float64 oracle", rtol=2.0 ** -23)
    assert_close64(H, evc.solve_activations(A, X, H0.copy(), **dict(kw, lone_bin=False)), "float32 caller vs lone_bin=False",
                   rtol=2.0 ** -23)


@pytest.mark.parametrize("N", [1024, 4096])
def test_a_voided_launch_is_redone_without_exchange(N):
    import exemplars_vc_amd as evc
    p = problem(25, N)
    kw = dict(iters=K, eps_mode="add", lone_bin=True)
    want, iw = evc.solve_activations(p["A"], p["X"], p["H0"].copy(), cooperative=False, info=True, **kw)
    got, ig = evc.solve_activations(p["A"], p["X"], p["H0"].copy(), _fake_coop_timeout=True, info=True, **kw)
    assert ig["redo"] == 1 and ig["exchange"] == 0 and iw["redo"] == 0, (ig, iw)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("M,N,loss", [(24, 1024, "frobenius"), (26, 1024, "frobenius"), (21, 1024, "frobenius"),
                                      (25, 16384, "frobenius"), (25, 512, "frobenius"), (25, 1536, "frobenius"),
                                      (25, 1024, "kl"), (25, 8192, "kl")])
def test_other_shapes_are_not_routed(M, N, loss):
    """one k-step less or a full last k-step, 32 members, one member, three members (ragged slices), KL: the flag changes
    nothing, bit for bit"""
    import exemplars_vc_amd as evc
    p = problem(M, N)
    kw = dict(iters=10, eps_mode="zero_replace", loss=loss)
    H_on, i_on = evc.solve_activations(p["A"], p["X"], p["H0"].copy(), lone_bin=True, info=True, **kw)
    H_off, i_off = evc.solve_activations(p["A"], p["X"], p["H0"].copy(), lone_bin=False, info=True, **kw)
    assert i_on["kernel"] == i_off["kernel"] and i_on["members"] == i_off["members"], (i_on, i_off)
    if loss == "frobenius" or N >= 8192:
        assert i_on["kernel"] == "k_fused_all", i_on
    assert np.isfinite(H_on).all() and np.array_equal(H_on, H_off)
