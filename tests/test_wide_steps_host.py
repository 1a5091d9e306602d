"""CPU side of tests/test_gpu_wide_steps.py: the oracle trajectory it compares with, the evc_solve_info.variant field it
asserts, and the inventory of wide-kernel template instances it must cover."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT


@pytest.mark.parametrize("eps_mode,eps,l1", [(0, 1e-9, 0.0), (1, 1.1920929e-07, 0.7), (2, 0.0, 0.0), (3, 1e-15, 0.2)])
def test_mu_trajectory_is_mu_solve_step_by_step(eps_mode, eps, l1):
    from oracle import evc_oracle as o
    p = o.synth_problem(40, 70, 33, seed=eps_mode)
    X = p["X"].copy()
    X[:, 4] = 0.0                                  # a zero frame: zero denominators from the second iteration on
    H0 = np.random.default_rng(1).random((70, 33)) + 1e-3
    K = 7
    Hs, res = o.mu_trajectory(p["A"], X, H0, K, eps_mode, eps, l1)
    assert len(Hs) == K and res.shape == (K,)
    for k in range(1, K + 1):
        want = o.mu_solve(p["A"], X, H0, k, eps_mode=eps_mode, eps=eps, l1=l1, algo="factored")
        assert np.array_equal(Hs[k - 1], want, equal_nan=True), k
        assert res[k - 1] == o.residual_fro(p["A"], X, Hs[k - 1]) or (np.isnan(res[k - 1]) and eps_mode == 2)
    assert not np.shares_memory(Hs[0], Hs[1])
    assert np.array_equal(H0, np.random.default_rng(1).random((70, 33)) + 1e-3)      # the start is not written to


def test_mu_trajectory_kl_is_sklearns_update():
    from oracle import evc_oracle as o
    p = o.synth_problem(30, 50, 20, seed=3)
    K = 6
    W_rows, X_rows = p["A"].T.copy(), p["X"].T.copy()
    act, _, _ = o.sklearn_mu_fixed_dictionary_kl(X_rows, W_rows, K, 0.0)
    H0 = np.full((50, 20), o.sklearn_init_value(X_rows, 50))
    Hs, res = o.mu_trajectory(p["A"], p["X"], H0, K, o.EPS_ZERO_REPLACE, o.SK_EPSILON, loss="kl")
    np.testing.assert_allclose(Hs[-1], act.T, rtol=1e-12)
    assert res[-1] == pytest.approx(o.kl_error(X_rows, act, W_rows), rel=1e-12)
    with pytest.raises(ValueError):
        o.mu_trajectory(p["A"], p["X"], H0, 1, o.EPS_ZERO_REPLACE, o.SK_EPSILON, l1=0.1, loss="kl")


def test_solve_info_variant_field_and_decoding():
    from exemplars_vc_amd import _lib
    names = [f[0] for f in _lib.SolveInfo._fields_]
    assert names[-1] == "variant" and "reserved" not in names
    assert _lib.decode_variant(6, 1 | 2 | 4 | (8 << 8) | (13 << 16)) == {
        "static": True, "reduce": True, "tagged": True, "w": 8, "mt": 13}
    assert _lib.decode_variant(6, (4 << 8) | (6 << 16)) == {"static": False, "reduce": False, "tagged": False, "w": 4,
                                                           "mt": 6}
    assert _lib.decode_variant(7, 1 | 2 | (3 << 8) | (13 << 16)) == {
        "static": True, "reduce": True, "tagged": False, "tpw": 3, "tiles": 13}
    for k in (0, 1, 2, 3, 4, 5, 8):
        assert _lib.decode_variant(k, 0) is None
    # the contraction kernels: update 64 x 128, V 64 x 64 in 7 k-ranges, P 64 x 128; GRAM on 128 x 128 without a V product
    assert _lib.decode_variant(1, 2 | (1 << 4) | (7 << 8) | (2 << 16)) == {
        "update": (64, 128), "v": (64, 64), "v_splits": 7, "p": (64, 128), "deep": False}
    assert _lib.decode_variant(2, 4 | (2 << 16)) == {
        "update": (128, 128), "v": None, "v_splits": 0, "p": (64, 128), "deep": False}
    assert _lib.decode_variant(2, 3 | (2 << 4) | (1 << 8))["p"] is None      # KL: no numerator


def _nm():
    for c in ("nm", "/opt/rocm/llvm/bin/llvm-nm"):
        if shutil.which(c) or os.path.exists(c):
            return c
    pytest.fail("no nm on this machine to list the library's symbols")


def test_wide_instance_inventory():
    """every k_fused_wide<MT, W, TG> and k_fused_wide64<TPW> instance the library ships is one the step-by-step GPU tests
    run, and the other way round: a new instance cannot ship untested"""
    from exemplars_vc_amd import _lib
    import test_gpu_wide_steps as steps
    out = subprocess.run([_nm(), "-C", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    wide = {(int(a), int(b), c == "true")
            for a, b, c in re.findall(r"k_fused_wide<(\d+), (\d+), (true|false)>", out)}
    wide64 = {(int(a),) for a in re.findall(r"k_fused_wide64<(\d+)>", out)}
    assert wide and wide64, "no k_fused_wide / k_fused_wide64 symbols found"
    assert wide == steps.INSTANCES["k_fused_wide"], sorted(wide ^ steps.INSTANCES["k_fused_wide"])
    assert wide64 == steps.INSTANCES["k_fused_wide64"], sorted(wide64 ^ steps.INSTANCES["k_fused_wide64"])
    assert os.path.dirname(steps.__file__) == os.path.join(ROOT, "tests")
