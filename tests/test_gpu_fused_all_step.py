"""k_fused_all's direct exchange on 16-byte words (evc_fused_all.hip: 2, 4 and 8 members) against the float64
oracle and the kernels without an exchange (`-m gpu`).

Thread th of the exchanging half owns the elements 2 th and 2 th + 1 of V' (th < NE / 2 = 32 k-steps): M = 25, 21, 17, 13, 9
and 5 have an odd k-step count, so the half's last working wavefront is half filled; M = 1 and 4 leave three of its four
wavefronts without work, M = 12 and 24 (3 and 6 k-steps) one.  Every shape runs with 2, 4 and 8 members, with and without
L1, from constant and from given start values.  The sums run in a fixed order (wavefronts, then members), so batch = solo and
run = re-run hold bitwise, and a voided launch is redone to the result of a call that never exchanged - also where the redo
must find the caller's start values (float32, widened again) or a prepared dictionary's image as the first attempt did.
"""
import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu

RTOL64 = 1e-8
SLICE = 48
T, K = 176, 30


def oracle():
    from oracle import evc_oracle
    return evc_oracle


def assert_close64(got, want, what, rtol=RTOL64):
    r, z = rel_err(got, want)
    print(f"{what}: max rel err {r:.3e}, max |got| where want==0 {z:.3e}")
    assert r <= rtol and z == 0.0, f"{what}: max rel err {r:.3e}, max |got| where want==0 {z:.3e}"


@pytest.mark.parametrize("start", ["const", "given"])
@pytest.mark.parametrize("l1", [0.0, 0.25])
@pytest.mark.parametrize("N", [1024, 2048, 4096])
@pytest.mark.parametrize("M", [25, 21, 17, 13, 9, 5, 1, 4, 12, 16, 24])
def test_pair_exchange_against_the_oracle_and_the_non_exchanging_kernels(M, N, l1, start):
    import exemplars_vc_amd as evc
    o = oracle()
    p = o.synth_problem(M, N, T, seed=M * 100 + N // 512)
    what = f"M={M} N={N} l1={l1} {start}"
    kw = dict(iters=K, eps_mode="zero_replace", l1=l1)
    if start == "const":
        h0 = np.sqrt(p["X"].mean() / N)
        H0, kw["init"] = np.full((N, T), h0), "sklearn"
        call = lambda **more: evc.solve_activations(p["A"], p["X"], **kw, **more)
    else:
        H0 = np.random.default_rng(M + N).random((N, T)) * 0.02 + 1e-4
        call = lambda **more: evc.solve_activations(p["A"], p["X"], H0.copy(), **kw, **more)
    H, info = call(info=True)
    assert (info["kernel"], info["members"], info["redo"], info["exchange"]) == ("k_fused_all", N // 512, 0, 1), (what, info)
    assert_close64(H, call(all_resident=False), what + ": vs all_resident=False")
    want = o.mu_solve(p["A"], p["X"][:, :SLICE], H0[:, :SLICE], K, eps_mode=o.EPS_ZERO_REPLACE, eps=o.SK_EPSILON, l1=l1,
                      algo="factored")
    assert_close64(H[:, :SLICE], want, what + ": vs the oracle")


@pytest.mark.parametrize("M,N", [(25, 4096), (24, 2048), (9, 1024), (1, 4096)])
def test_batch_equals_solo_and_run_equals_rerun_bitwise(M, N):
    """member order and wavefront order of the sums are fixed: neither the batch around a frame nor the run shows"""
    import exemplars_vc_amd as evc
    o = oracle()
    p = o.synth_problem(M, N, 688 * 2, seed=M + N)
    kw = dict(iters=K, eps_mode="zero_replace", init="const", init_value=0.01)
    H1, i1 = evc.solve_activations(p["A"], p["X"], info=True, **kw)
    H2 = evc.solve_activations(p["A"], p["X"], **kw)
    assert i1["kernel"] == "k_fused_all" and i1["members"] == N // 512 and i1["redo"] == 0 and i1["exchange"] == 1, i1
    assert np.array_equal(H1, H2)
    Hs = evc.solve_activations(p["A"], np.ascontiguousarray(p["X"][:, :688]), **kw)
    assert np.array_equal(H1[:, :688], Hs)


@pytest.mark.parametrize("M,N", [(25, 4096), (13, 1024)])
def test_a_voided_launch_is_redone_without_exchange(M, N):
    """the abort flag raised as a timed-out wait would raise it (evc_solve_opts.test_abort_at): every wait of the 16-byte
    exchange ends, the solve is redone, and the result is that of a call that never exchanged"""
    import exemplars_vc_amd as evc
    o = oracle()
    p = o.synth_problem(M, N, 90, seed=5)
    H0 = np.random.default_rng(5).random((N, 90)) + 1e-4
    kw = dict(iters=30, eps_mode="add")
    want, iw = evc.solve_activations(p["A"], p["X"], H0.copy(), cooperative=False, info=True, **kw)
    got, ig = evc.solve_activations(p["A"], p["X"], H0.copy(), _fake_coop_timeout=True, info=True, **kw)
    assert ig["redo"] == 1 and ig["exchange"] == 0 and iw["redo"] == 0, (ig, iw)
    assert np.array_equal(got, want)


# The one redo path (solve_checked) plans and runs the whole call again.  Two situations in which the second attempt
# needs something the first one must have left alone: M = 25, N = 1024 (two members: the smallest dictionary that
# exchanges), one full frame tile and one frame into a second, two launches of two iterations; the flag is up from the
# start, or goes up in front of the second launch: test_abort_at counts the launches of the loop from 0, so that is 1 (a
# 2 would never go up in a solve of two launches).
REDO_KW = dict(iters=4, check_every=2, eps_mode="zero_replace")


@pytest.mark.parametrize("fake", [True, 1])
@pytest.mark.parametrize("frames", [16, 17])
def test_staged_redo_widens_the_callers_start_again(frames, fake):
    """float32 on the float64 kernels: the redo widens the caller's H0 a second time, so nothing of the voided attempt may
    have been narrowed into it"""
    import torch
    import exemplars_vc_amd as evc
    p = oracle().synth_problem(25, 1024, frames, seed=frames)
    A, X = p["A"].astype(np.float32), p["X"].astype(np.float32)
    start = (np.random.default_rng(frames).random((1024, frames)) * 0.02 + 1e-4).astype(np.float32)
    H0 = torch.from_numpy(start).cuda()
    want, iw = evc.solve_activations(A, X, H0, cooperative=False, info=True, **REDO_KW)
    out = torch.full_like(H0, -1.0)
    got, ig = evc.solve_activations(A, X, H0, out=out, _fake_coop_timeout=fake, info=True, **REDO_KW)
    print(frames, fake, ig, iw)
    assert ig["redo"] == 1 and ig["exchange"] == 0 and iw["redo"] == 0, (ig, iw)
    assert got.data_ptr() == out.data_ptr() and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(H0.cpu().numpy(), start)


@pytest.mark.parametrize("fake", [True, 1])
@pytest.mark.parametrize("frames", [16, 17])
def test_prepared_redo_reuses_the_image(frames, fake):
    """a prepared dictionary with B (Mb = 25), only Y wanted: the second attempt reads the image the first one read, and
    forms Y by the pre-pass where the first attempt's last launch would have formed it in the kernel"""
    import exemplars_vc_amd as evc
    p = oracle().synth_problem(25, 1024, frames, seed=frames)
    B = np.random.default_rng(frames + 1).random((25, 1024)) + 0.01
    pd = evc.prepare_dictionary(p["A"], B, dtype="f64")
    Yw, iw = evc.convert(pd, p["X"], None, want_h=False, cooperative=False, info=True, **REDO_KW)
    Y, ig = evc.convert(pd, p["X"], None, want_h=False, _fake_coop_timeout=fake, info=True, **REDO_KW)
    print(frames, fake, ig, iw)
    assert ig["redo"] == 1 and ig["prepared"] == 1 and iw["redo"] == 0, (ig, iw)
    assert np.array_equal(Y, Yw)
