"""k_fused_all with the member's dictionary in LDS (evc_fused_all.hip, AllShape) against the kernels without an exchange
(all_resident=False) and the float64 oracle (`-m gpu`).

Shapes: C2- and C5-shaped slices (8 members - the direct exchange - and 32 members), 2 and 3 members (the ragged
reduce-scatter), M = 25 (the largest M in LDS), every k-step count that keeps the dictionary in LDS, M = 26 (just past the
budget: the streamed path of the same instance, reduce-scatter) and C1 (one member: streamed).  Each run must report
k_fused_all with the expected members and no redo.
"""
import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu

RTOL64 = 1e-8
SLICE = 48


def oracle():
    from oracle import evc_oracle
    return evc_oracle


def assert_close64(got, want, what, rtol=RTOL64):
    r, z = rel_err(got, want)
    assert r <= rtol and z == 0.0, f"{what}: max rel err {r:.3e}, max |got| where want==0 {z:.3e}"


@pytest.mark.parametrize("M,N,T,K,l1,what", [
    (25, 4096, 688, 40, 0.0, "C2-shaped, 8 members, direct exchange"),
    (25, 16384, 344, 30, 0.25, "C5-shaped, 32 members, L1"),
    (25, 1024, 500, 40, 0.0, "2 members"),
    (25, 1536, 300, 40, 0.0, "3 members, ragged slices"),
    (24, 4096, 300, 40, 0.0, "M = 24, 6 k-steps"),
    (21, 2048, 300, 40, 0.0, "M = 21"),
    (17, 4096, 300, 40, 0.0, "M = 17, 5 k-steps"),
    (13, 4096, 300, 40, 0.0, "M = 13, 4 k-steps"),
    (6, 2048, 300, 40, 0.0, "M = 6, 2 k-steps"),
    (2, 4096, 300, 40, 0.0, "M = 2, 1 k-step"),
    (26, 4096, 688, 40, 0.0, "M = 26: past the LDS budget, streamed"),
    (28, 2048, 300, 40, 0.0, "M = 28: streamed, 4 members"),
    (25, 512, 688, 50, 0.0, "C1, one member: streamed"),
])
def test_lds_dictionary_against_the_non_exchanging_kernels_and_the_oracle(M, N, T, K, l1, what):
    import exemplars_vc_amd as evc
    o = oracle()
    p = o.synth_problem(M, N, T, seed=M * 1000 + N // 512)
    kw = dict(iters=K, eps_mode="zero_replace", init="sklearn", l1=l1)
    H, info = evc.solve_activations(p["A"], p["X"], info=True, **kw)
    assert (info["kernel"], info["members"], info["redo"], info["exchange"]) == \
        ("k_fused_all", N // 512, 0, 1 if N > 512 else 0), (what, info)
    ref = evc.solve_activations(p["A"], p["X"], all_resident=False, **kw)
    assert_close64(H, ref, what + ": vs all_resident=False")
    h0 = np.sqrt(p["X"].mean() / N)
    want = o.mu_solve(p["A"], p["X"][:, :SLICE], np.full((N, SLICE), h0), K, eps_mode=o.EPS_ZERO_REPLACE,
                      eps=o.SK_EPSILON, l1=l1, algo="factored")
    assert_close64(H[:, :SLICE], want, what + ": vs the oracle")


def test_lds_dictionary_batch_equals_solo_and_repeats_bitwise():
    """the direct exchange sums the members in member order: a frame's activations do not depend on the batch around
    it nor on the run"""
    import exemplars_vc_amd as evc
    o = oracle()
    M, N, K = 25, 4096, 30
    p = o.synth_problem(M, N, 688 * 2, seed=77)
    kw = dict(iters=K, eps_mode="zero_replace", init="const", init_value=0.01)
    H1, i1 = evc.solve_activations(p["A"], p["X"], info=True, **kw)
    H2 = evc.solve_activations(p["A"], p["X"], **kw)
    assert i1["kernel"] == "k_fused_all" and i1["members"] == 8 and i1["redo"] == 0, i1
    assert np.array_equal(H1, H2)
    Hs = evc.solve_activations(p["A"], np.ascontiguousarray(p["X"][:, :688]), **kw)
    assert np.array_equal(H1[:, :688], Hs)
