"""CPU side of tests/test_gpu_cd_steps.py: the geometry mirror it picks its shapes with (proved against
evc_cd_workspace_bytes), the inventory of k_cd_sweep instances it must launch, the restatement it compares with (against
scikit-learn's own sweeps at the matrix's shapes) and the power of its comparisons (four wrong variants of the algebra
must each be rejected on some case)."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_cd_steps as steps  # noqa: E402
from cd_restatement import cd_iterations  # noqa: E402


def _ws_mirror(M, N, T, n_utt, esize):
    """cd_workspace_bytes (evc_cd.hip) rebuilt from the geometry mirror: [Ac | Gb | hess | R | tiles | utt_tile0 |
    part | stop | vinit | trace], each rounded up to 256 bytes, plus 256 for the base alignment"""
    g = steps.geometry(M)
    if g is None or N < 1 or T < 0 or n_utt < 1:
        return 0
    a = lambda x: -(-x // 256) * 256            # noqa: E731
    Np = -(-N // steps.CD_B) * steps.CD_B
    nt = -(-T // g["F"]) + n_utt
    return (a(Np * g["Mr"] * esize) + a(Np * steps.CD_B * esize) + a(Np * esize) + a(nt * g["F"] * g["Mr"] * esize)
            + a(nt * 16) + a((n_utt + 1) * 4) + a(2 * nt * 8) + a(n_utt * 4) + a(n_utt * 8)
            + a(n_utt * steps.CD_TRACE_CAP * 8) + 256)


def test_geometry_mirror_rebuilds_the_workspace_size():
    from exemplars_vc_amd import _lib
    q = _lib.lib().evc_cd_workspace_bytes
    combos = [(1, 0, 1), (15, 1, 1), (17, 63, 3), (100, 200, 2), (16, 1000, 7), (33, 65, 1)]
    for M in range(1, 1025):
        g = steps.geometry(M)
        assert g["mpl"] <= 16 and (g["L"] == 1 or -(-M // (g["L"] // 2)) > 16), M
        for N, T, n_utt in combos:
            for code, esize in ((_lib.F64, 8), (_lib.F32, 4)):
                assert q(M, N, T, n_utt, code) == _ws_mirror(M, N, T, n_utt, esize), (M, N, T, n_utt, esize)
    assert steps.geometry(1025) is None
    assert q(1025, 16, 10, 1, _lib.F64) == 0 and q(1025, 16, 10, 1, _lib.F32) == 0
    # the mirror sees what the size sees: Mr (dictionary, residual) and F (tile count)
    assert {steps.geometry(m)["L"] for m in range(1, 1025)} == {1, 2, 4, 8, 16, 32, 64}
    assert {steps.geometry(m)["MPL"] for m in range(1, 1025)} == {1, 8, 16}


def _nm():
    for c in ("nm", "/opt/rocm/llvm/bin/llvm-nm"):
        if shutil.which(c) or os.path.exists(c):
            return c
    pytest.fail("no nm on this machine to list the library's symbols")


def test_cd_instance_inventory():
    """every k_cd_sweep<T, MPL> the library ships is launched by the step-by-step GPU tests, and the other way round"""
    from exemplars_vc_amd import _lib
    out = subprocess.run([_nm(), "-C", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    shipped = {(t, int(m)) for t, m in re.findall(r"k_cd_sweep<(double|float), (\d+)>", out)}
    assert shipped, "no k_cd_sweep symbols found"
    assert shipped == steps.INSTANCES, sorted(shipped ^ steps.INSTANCES)
    assert os.path.dirname(steps.__file__) == os.path.join(ROOT, "tests")


def _matrix_shapes():
    return sorted({(M, N) for M, N, _, _ in steps.MATRIX})


@pytest.mark.parametrize("M,N", _matrix_shapes(), ids=[f"m{m}_n{n}" for m, n in _matrix_shapes()])
def test_restatement_matches_sklearn_sweeps(M, N):
    pytest.importorskip("sklearn")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_golden_cd as g
    X, W = steps.problem(M, N, 3, seed=M * 1000 + N)
    X[1] = 0.0                                          # a zero frame next to two others
    for K in (1, 2, 3):
        H_sk, n_iter, trace = g.run_sklearn(X, W, tol=0.0, max_iter=K)
        H, v = cd_iterations(X, W, K)
        assert steps.h_err(H, H_sk.T) <= 1e-13, (K, steps.h_err(H, H_sk.T))
        big = trace > 1e-8 * trace[0]                   # M = 1 sits at its fixed point after one sweep
        np.testing.assert_allclose(v[:n_iter][big], trace[big], rtol=1e-12, atol=0)
        assert n_iter == K or trace[-1] == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# the comparisons of test_gpu_cd_steps.py reject wrong algebra
# ---------------------------------------------------------------------------------------------------------------------
def mutant_iterations(X_rows, W_rows, iters, H0=None, l1=0.0, l2=0.0, kind=None):
    """cd_restatement.cd_iterations with one defect (kind None: the same bits):
       jacobi         no in-block Gram correction (the 16 steps of a block all use the block's start gradients)
       l1_sign        l1 subtracted from the gradient instead of added
       raw_violation  the violation sums |grad| instead of the projected gradient
       padded_real    the padding components of the last block take the clamped H read (H[:, N-1]) as their value and
                      count in the violation, as a kernel that dropped the `c0 + j < N` masks would"""
    X = np.asarray(X_rows, dtype=np.float64)
    A = np.asarray(W_rows, dtype=np.float64)
    T, M = X.shape
    N = A.shape[0]
    H = np.zeros((T, N)) if H0 is None else np.array(H0, dtype=np.float64)
    R = H @ A - X
    hess = np.einsum("nm,nm->n", A, A) + l2
    sl1 = -l1 if kind == "l1_sign" else l1
    viols = []
    for _ in range(iters):
        viol = 0.0
        for c0 in range(0, N, steps.CD_B):
            Ab = A[c0:c0 + steps.CD_B]
            nb = Ab.shape[0]
            nj = steps.CD_B if kind == "padded_real" else nb
            G = Ab @ Ab.T
            Hb = H[:, np.minimum(np.arange(c0, c0 + nj), N - 1)]
            g = np.zeros((T, nj))
            g[:, :nb] = R @ Ab.T
            g = g + l2 * Hb + sl1
            d = np.zeros_like(g)
            for j in range(nj):
                w = Hb[:, j]
                grad = g[:, j]
                pg = grad if kind == "raw_violation" else np.where(w == 0, np.minimum(grad, 0), grad)
                viol += float(np.abs(pg).sum())
                h = hess[c0 + j] if j < nb else l2
                if h != 0:
                    nw = np.maximum(w - grad / h, 0)
                    d[:, j] = nw - w
                    Hb[:, j] = nw
                if kind != "jacobi" and j < nb:
                    g[:, j + 1:nb] += d[:, j:j + 1] * G[j, j + 1:]
            H[:, c0:c0 + nb] = Hb[:, :nb]
            R = R + d[:, :nb] @ Ab
        viols.append(viol)
    return H, np.array(viols)


def _mutant_cases():
    """(name, X, W, K, l1, l2): the geometry matrix, then the regularised cases of every L"""
    for M, N, T, K in steps.MATRIX:
        X, W = steps.problem(M, N, T, seed=M * 1000 + N)
        yield f"m{M}_n{N}_t{T}", X, W, K, 0.0, 0.0
    for M in steps.L_M.values():
        X, W = steps.l_problem(M, seed=M + 7, zero_frames=True)
        for opt, (a1, a2) in sorted(steps.OPTIONS.items()):
            yield f"{opt}_m{M}", X, W, 3, M * a1, M * a2


def test_mutant_of_kind_none_is_the_restatement():
    K = 3
    X, W = steps.l_problem(40, seed=3, zero_frames=True)
    for l1, l2 in ((0.0, 0.0), (2.0, 4.0)):
        H, v = cd_iterations(X, W, K, l1=l1, l2=l2)
        Hm, vm = mutant_iterations(X, W, K, l1=l1, l2=l2)
        assert np.array_equal(H, Hm) and np.array_equal(v, vm)


@pytest.mark.parametrize("kind", ["jacobi", "l1_sign", "raw_violation", "padded_real"])
def test_step_comparisons_reject_the_mutant(kind):
    seen = []
    for name, X, W, K, l1, l2 in _mutant_cases():
        HK, v = cd_iterations(X, W, K, l1=l1, l2=l2)
        Hm, vm = mutant_iterations(X, W, K, l1=l1, l2=l2, kind=kind)
        eh, ev = steps.h_err(Hm, HK), steps.v_err(vm, v)
        seen.append((name, eh, ev))
        if eh > steps.H_BOUND or ev > steps.V_RTOL:
            print(f"MUTANT {kind} rejected by {name}: H {eh:.3e} violation {ev:.3e}")
            return
    pytest.fail(f"no case rejects the {kind} mutant: {seen}")
