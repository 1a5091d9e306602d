"""Beta-divergence activation solve (evc_beta_solve / k_beta_sweep) on the GPU against scikit-learn's recorded results
(tests/golden/betamu_*.npz, tools/make_golden_beta.py) and the numpy restatement (tests/beta_restatement.py).

Tolerances (the project's own, as in tests/test_gpu_learn_kl.py): float64 relative 1e-9 on the entries the reference
has non-zero and zeros exact; float32 norm-relative 1e-4."""
import ctypes as C
import functools
import glob
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beta_restatement as br  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "betamu_*.npz")))
SENTINEL = -12345.25

pytestmark = pytest.mark.gpu


def close64(got, ref, what=""):
    """relative 1e-9 on the non-zero entries of the reference, zeros exact; prints the figure before asserting"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    nz = ref != 0
    worst = float(np.max(np.abs(got[nz] - ref[nz]) / np.abs(ref[nz]))) if nz.any() else 0.0
    print(f"{what}: worst relative deviation {worst:.3e}, zeros kept {bool((got[~nz] == 0).all())}")
    assert (got[~nz] == 0).all(), what
    assert worst <= 1e-9, (what, worst)


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / np.linalg.norm(b))


def _reg(d):
    M = d["X_rows"].shape[1]
    a, r = float(d["alpha_W"]), float(d["l1_ratio"])
    return M * a * r, M * a * (1 - r)


def solve(W, X, H0=None, **kw):
    import exemplars_vc_amd as evc
    kw.setdefault("layout", "frame_major")
    return evc.solve_activations_beta(W, X, H0, info=True, **kw)


def schedule(tol):
    return dict(check_every=10 if tol > 0 else 0, stop_rule="sklearn" if tol > 0 else "none", tol=tol)


@pytest.mark.parametrize("path", FILES, ids=os.path.basename)
def test_fixture(path, monkeypatch):
    from exemplars_vc_amd.compat import factorize as fz
    d = np.load(path)
    X, W, beta, tol, K, n_ref = d["X_rows"], d["W_rows"], float(d["beta"]), float(d["tol"]), int(d["max_iter"]), int(d["n_iter"])
    l1, l2 = _reg(d)
    f32 = X.dtype == np.float32

    def check(H, what):
        assert H.dtype == X.dtype and H.shape == d["H"].shape
        if f32:
            print(f"{what}: norm-relative {rel(H, d['H']):.3e} (float32 sklearn), {rel(H, d['H_f64']):.3e} (float64 sklearn)")
            assert rel(H, d["H"]) <= 1e-4 and rel(H, d["H_f64"]) <= 1e-4, what
        else:
            close64(H, d["H"], what)

    act, info = solve(W, X, beta=beta, iters=K, l1=l1, l2=l2, **schedule(tol))
    assert info["kernel"] == "k_beta_sweep" and int(info["n_iter"][0]) == n_ref
    check(act.T, "solve_activations_beta")
    err = info["err"][0]
    k = n_ref // 10 if tol > 0 else 0
    assert err.shape == (1 + (K // 10 if tol > 0 else 0),)
    if tol > 0:
        assert np.isfinite(err[:k + 1]).all() and np.isnan(err[k + 1:]).all()
        if not f32:
            np.testing.assert_allclose(err[:k + 1], d["err"][:k + 1], rtol=1e-9, atol=0)
    else:
        assert np.isnan(err).all()
    if "zeros" in path:
        assert (act[3] == 0).all() and (act[:, 7] == 0).all() and np.isfinite(act).all()
    if l1 or l2:
        return          # the compat mirrors have no alpha_W / l1_ratio
    monkeypatch.setattr(fz, "MAX_ITER", K)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        H = fz._factorize(X, W, beta_loss=beta if beta else "itakura-saito", tol=tol, honor_beta_loss=True)
    assert np.array_equal(H, act.T)                      # the same call underneath
    assert not [x for x in w if "Maximum number of iterations" in str(x.message)]
    W0 = np.full((X.shape[0], W.shape[0]), np.sqrt(X.mean() / W.shape[0]), dtype=X.dtype)
    Wa, Hd, n_it = fz.non_negative_factorization_mu(X, W0, W, update_H=False, tol=tol, max_iter=K, beta_loss=beta)
    assert n_it == n_ref and Hd is not None and np.array_equal(Hd, W)
    check(Wa.T, "non_negative_factorization_mu")


@functools.lru_cache(maxsize=None)
def _batch_problem():
    d = np.load(os.path.join(GOLDEN, "betamu_m25_n64_t50_b0_tol2e-2.npz"))
    X, W = d["X_rows"], d["W_rows"]
    utts = [X[:23].copy(), X[:0].copy(), X[7:20] + 0.2]     # stops at 20, empty, stops at 50 (margins 14 % and 4.9 %)
    ref = [br.beta_solve(x, W, 0.0, 150, 2e-2) if len(x) else None for x in utts]
    return W, utts, ref


def test_ragged_batch_is_bitwise_the_solo_solves():
    W, utts, ref = _batch_problem()
    kw = dict(beta=0.0, iters=150, **schedule(2e-2))
    offs = np.concatenate([[0], np.cumsum([len(x) for x in utts])])
    act, info = solve(W, np.concatenate(utts), utt_offsets=offs, **kw)
    assert info["n_iter"][1] == 150 and np.isnan(info["err"][1]).all()          # the empty utterance: nothing ran
    for u in (0, 2):
        solo, si = solve(W, utts[u], **kw)
        assert np.array_equal(act[offs[u]:offs[u + 1]], solo)
        assert info["n_iter"][u] == si["n_iter"][0] == ref[u][1]
        np.testing.assert_array_equal(info["err"][u], si["err"][0])
        close64(solo, ref[u][0], f"utterance {u}")
        k = ref[u][1] // 10
        assert np.isfinite(info["err"][u][:k + 1]).all() and np.isnan(info["err"][u][k + 1:]).all()
    assert info["n_iter"][0] == 20 and info["n_iter"][2] == 50                   # one stops early, the other runs on


def test_two_runs_are_bitwise_equal():
    W, utts, _ = _batch_problem()
    X = np.concatenate(utts)
    offs = np.concatenate([[0], np.cumsum([len(x) for x in utts])])
    kw = dict(beta=0.5, iters=40, utt_offsets=offs, **schedule(1e-3))
    a, ia = solve(W, X, **kw)
    b, ib = solve(W, X, **kw)
    assert np.array_equal(a, b) and np.array_equal(ia["n_iter"], ib["n_iter"])
    np.testing.assert_array_equal(ia["err"], ib["err"])


def raw_beta_solve(W, X, H0, offs, layout, pad, iters, beta, init, dtype=np.float64, init_value=0.0):
    """evc_beta_solve through ctypes with lda / ldx / ldh = minimum + pad and no host outputs (the asynchronous form);
    returns (H buffer with its padding, frames-as-rows view of H)"""
    import torch
    from exemplars_vc_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    tr = (lambda z: z) if layout == "frame_major" else (lambda z: np.ascontiguousarray(z.T))

    def padded(a, fill):
        a = tr(a)
        buf = torch.full((a.shape[0], a.shape[1] + pad), fill, dtype=tdt, device=dev)
        buf[:, :a.shape[1]] = torch.from_numpy(a.astype(dtype)).to(dev)
        return buf
    T, N, M = X.shape[0], W.shape[0], W.shape[1]
    A_b, X_b = padded(W, 7.5), padded(X, float("nan"))
    H_b = padded(np.full((T, N), 3.25) if H0 is None else H0, SENTINEL)
    o = _lib.BetaOpts()
    o.struct_bytes = C.sizeof(_lib.BetaOpts)
    o.dtype = _lib.F64 if dtype == np.float64 else _lib.F32
    o.layout = _lib.FRAME_MAJOR if layout == "frame_major" else _lib.BIN_MAJOR
    o.init_mode = {"given": _lib.INIT_GIVEN, "sklearn": _lib.INIT_SKLEARN, "const": _lib.INIT_CONST}[init]
    o.iters, o.beta, o.init_value = iters, beta, init_value
    off = np.ascontiguousarray(offs, dtype=np.int32)
    n_utt = len(off) - 1
    ws = torch.empty(int(L.evc_beta_workspace_bytes(M, N, T, n_utt, o.dtype)), dtype=torch.uint8, device=dev)
    st = L.evc_beta_solve(A_b.data_ptr(), A_b.stride(0), X_b.data_ptr(), X_b.stride(0), H_b.data_ptr(), H_b.stride(0),
                          M, N, T, off.ctypes.data_as(C.POINTER(C.c_int)), n_utt, C.byref(o), ws.data_ptr(), ws.numel(),
                          None, None, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert st == 0, st
    Hb = H_b.cpu().numpy()
    view = Hb[:, :Hb.shape[1] - pad]
    return Hb, (view if layout == "frame_major" else view.T)


def _problem(M, N, T, seed):
    rng = np.random.default_rng(seed)
    W = rng.random((N, M)) ** 2 + 0.05
    X = (rng.random((T, N)) * (rng.random((T, N)) < 0.3)) @ W + 0.05 * rng.random((T, M)) + 1e-3
    return X, W


@pytest.mark.parametrize("init", ["sklearn", "given", "const"])
@pytest.mark.parametrize("layout", ["frame_major", "bin_major"])
def test_leading_dimensions_above_the_minimum(layout, init):
    M, N, pad = 40, 17, 3                             # utterances of 9 and 12 frames: partial tiles, N % 16 != 0
    X, W = _problem(M, N, 21, seed=5)
    offs = [0, 9, 21]
    H0 = np.random.default_rng(3).random((21, N)) + 0.01 if init == "given" else None
    Hb, H = raw_beta_solve(W, X, H0, offs, layout, pad, 4, 0.5, init, init_value=0.37)
    assert (Hb[:, Hb.shape[1] - pad:] == SENTINEL).all()
    tr = (lambda z: z) if layout == "frame_major" else (lambda z: np.ascontiguousarray(z.T))
    packed, _ = solve(tr(W), tr(X), None if H0 is None else tr(H0), layout=layout, beta=0.5, iters=4, init=init,
                      init_value=0.37, utt_offsets=offs)
    assert np.array_equal(tr(H), packed)
    ref = np.concatenate([br.beta_solve(X[a:b], W, 0.5, 4, W0=None if init == "sklearn" else
                                        (H0[a:b] if init == "given" else np.full((b - a, N), 0.37)))[0]
                          for a, b in zip(offs[:-1], offs[1:])])
    close64(H, ref, f"{layout} {init}")


def test_zero_iterations_and_no_frames():
    X, W = _problem(25, 20, 7, seed=2)
    act, info = solve(W, X, beta=0.0, iters=0, check_every=10)
    assert act.shape == (7, 20) and rel(act, np.full((7, 20), np.sqrt(X.mean() / 20))) <= 1e-15
    assert info["n_iter"][0] == 0 and info["err"].shape == (1, 1)
    np.testing.assert_allclose(info["err"][0, 0], br.beta_solve(X, W, 0.0, 0)[2][0], rtol=1e-9)
    act, info = solve(W, X[:0], beta=0.0, iters=3)
    assert act.shape == (0, 20) and info["n_iter"][0] == 3


@pytest.mark.parametrize("beta,dtype", [(2.0, np.float64), (1.0, np.float64), (0.7, np.float64), (-0.3, np.float64),
                                         (0.7, np.float32)])
def test_generic_statement(beta, dtype):
    """beta = 2 and beta = 1 against the special-cased solves; a general float beta (the pow path) against the restatement"""
    import exemplars_vc_amd as evc
    X, W = _problem(40, 50, 37, seed=int(10 * abs(beta)))
    X, W = X.astype(dtype), W.astype(dtype)
    act, _ = solve(W, X, beta=beta, iters=30)
    ref = br.beta_solve(X, W, beta, 30)[0]
    if dtype == np.float32:
        print(f"beta {beta} float32: norm-relative {rel(act, ref):.3e}")
        assert rel(act, ref) <= 1e-4
        return
    close64(act, ref, f"beta {beta} vs the restatement")
    if beta == 2.0:
        other = evc.solve_activations(W, X, layout="frame_major", iters=30, eps_mode="zero_replace", init="sklearn")
        close64(act, other, "beta 2 vs solve_activations(zero_replace)")
    if beta == 1.0:
        other = evc.solve_activations(W, X, layout="frame_major", iters=30, eps_mode="zero_replace", init="sklearn",
                                      loss="kl")
        close64(act, other, "beta 1 vs solve_activations(loss='kl')")


@pytest.mark.parametrize("M,N,T,beta", [(528, 19, 5, 0.5), (130, 70, 33, 3.0), (16, 16, 16, 0.0)])
def test_tile_edges(M, N, T, beta):
    """the widest supported spectrum (both LDS images full), more than one pass of phase 1 (M > 128), exact tile sizes"""
    X, W = _problem(M, N, T, seed=M)
    act, info = solve(W, X, beta=beta, iters=6, check_every=3)
    ref, _, tr = br.beta_solve(X, W, beta, 6, tol=1e-300, check_every=3)
    close64(act, ref, f"M {M}")
    np.testing.assert_allclose(info["err"][0], tr, rtol=1e-9)


def test_nan_stays_in_its_frame():
    """(a constant start: scikit-learn's own start is the utterance's mean, which a non-finite entry reaches by definition)"""
    X, W = _problem(25, 40, 37, seed=9)
    kw = dict(beta=0.5, iters=12, init="const", init_value=0.3)
    clean, _ = solve(W, X, **kw)
    assert np.isfinite(clean).all()
    for bad in (np.nan, np.inf):
        Xb = X.copy()
        Xb[18, 4] = bad
        got, _ = solve(W, Xb, **kw)
        keep = np.arange(37) != 18
        assert np.array_equal(got[keep], clean[keep])
        assert not np.isfinite(got[18]).all()
