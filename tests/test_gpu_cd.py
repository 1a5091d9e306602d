"""Coordinate-descent solve (evc_cd_solve / k_cd_sweep) on the GPU against scikit-learn's recorded results
(tests/golden/cdnmf_*.npz, tools/make_golden_cd.py) and the numpy restatement of the blocked algebra."""
import glob
import os
import sys
import time
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cd_restatement import cd_iterations  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
F64_FILES = [p for p in sorted(glob.glob(os.path.join(GOLDEN, "cdnmf_*.npz"))) if not p.endswith("_f32.npz")]
F32_FILES = [p for p in sorted(glob.glob(os.path.join(GOLDEN, "cdnmf_*.npz"))) if p.endswith("_f32.npz")]

pytestmark = pytest.mark.gpu


def _rel(a, b):
    nb = np.linalg.norm(b)
    return np.linalg.norm(a - b) / nb if nb > 0 else np.linalg.norm(a)


def _reg(d):
    M = d["X_rows"].shape[1]
    a, r = float(d["alpha_W"]), float(d["l1_ratio"])
    return M * a * r, M * a * (1 - r)


@pytest.mark.parametrize("path", F64_FILES, ids=os.path.basename)
def test_fixture_f64(path):
    import exemplars_vc_amd as evc
    from exemplars_vc_amd.compat import factorize_cd
    d = np.load(path)
    l1, l2 = _reg(d)
    tol, n_ref = float(d["tol"]), int(d["n_iter"])
    act, info = evc.solve_activations_cd(d["W_rows"], d["X_rows"], layout="frame_major", max_iter=200, tol=tol,
                                         l1=l1, l2=l2, info=True)
    assert info["kernel"] == "k_cd_sweep"
    assert int(info["n_iter"][0]) == n_ref
    assert _rel(act.T, d["H"]) <= 1e-10
    v = info["violation"][0]
    np.testing.assert_allclose(v[:n_ref], d["violation"], rtol=1e-9, atol=0)
    assert np.isnan(v[n_ref:]).all()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        H = factorize_cd._factorize(d["X_rows"], d["W_rows"], tol=tol, alpha_W=float(d["alpha_W"]),
                                    l1_ratio=float(d["l1_ratio"]))
    assert np.array_equal(H, act.T)
    capped = [x for x in w if "Maximum number of iterations" in str(x.message)]
    assert len(capped) == (1 if n_ref == 200 and tol > 0 else 0)


def test_fixture_f32():
    from exemplars_vc_amd import solve_activations_cd
    assert len(F32_FILES) >= 2
    for path in F32_FILES:
        d = np.load(path)
        assert d["X_rows"].dtype == np.float32
        act, info = solve_activations_cd(d["W_rows"], d["X_rows"], layout="frame_major", tol=float(d["tol"]),
                                         info=True)
        assert act.dtype == np.float32
        assert _rel(act.T.astype(np.float64), d["H_f64"]) <= 1e-4, path
        assert abs(int(info["n_iter"][0]) - int(d["n_iter"])) <= 1, path


def test_bin_major_gives_the_frame_major_result():
    from exemplars_vc_amd import solve_activations_cd
    d = np.load(os.path.join(GOLDEN, "cdnmf_m201_n128_t40.npz"))
    fm = solve_activations_cd(d["W_rows"], d["X_rows"], layout="frame_major", max_iter=20, tol=0)
    bm = solve_activations_cd(np.ascontiguousarray(d["W_rows"].T), np.ascontiguousarray(d["X_rows"].T),
                              layout="bin_major", max_iter=20, tol=0)
    assert np.array_equal(fm, bm.T)


@pytest.mark.parametrize("name", ["cdnmf_m25_n64_t32", "cdnmf_m513_n96_t21"])
def test_batch_is_bitwise_the_solo_calls(name):
    from exemplars_vc_amd import solve_activations_cd
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    X, W = d["X_rows"], d["W_rows"]
    utts = [X, np.zeros((5, X.shape[1])), 3.0 * X[: X.shape[0] // 2], X[::-1].copy(), X[:1]]
    solo = [solve_activations_cd(W, x, layout="frame_major", tol=1e-3, info=True) for x in utts]
    offs = np.concatenate([[0], np.cumsum([x.shape[0] for x in utts])])
    act, info = solve_activations_cd(W, np.concatenate(utts), layout="frame_major", tol=1e-3, utt_offsets=offs,
                                     info=True)
    assert int(info["n_iter"][1]) == 1
    assert len(set(int(s[1]["n_iter"][0]) for s in solo)) >= 2          # the batch mixes stop iterations
    for u, (h, inf) in enumerate(solo):
        assert int(info["n_iter"][u]) == int(inf["n_iter"][0])
        assert np.array_equal(act[offs[u]:offs[u + 1]], h), u
        np.testing.assert_array_equal(info["violation"][u], inf["violation"][0])


def test_warm_start_continues_the_iteration():
    from exemplars_vc_amd import solve_activations_cd
    d = np.load(os.path.join(GOLDEN, "cdnmf_m201_audio.npz"))
    X, W = d["X_rows"], d["W_rows"]
    H5 = solve_activations_cd(W, X, layout="frame_major", max_iter=5, tol=0)
    H3 = solve_activations_cd(W, X, layout="frame_major", max_iter=3, tol=0)
    H3_2 = solve_activations_cd(W, X, H3, layout="frame_major", max_iter=2, tol=0)
    assert not np.array_equal(H3, H5)
    assert _rel(H3_2, H5) <= 1e-10


@pytest.mark.parametrize("M,N,T,dtype", [(25, 4096, 688, np.float64), (513, 8192, 688, np.float64),
                                         (201, 4096, 688, np.float32)], ids=["C2", "C3", "STFT_f32"])
def test_full_size_against_the_restatement(M, N, T, dtype):
    from exemplars_vc_amd import solve_activations_cd
    rng = np.random.default_rng(M + N)
    W = rng.random((N, M)) ** 2
    X = (rng.random((T, N)) * (rng.random((T, N)) < 0.01)) @ W + 1e-3 * rng.random((T, M))
    iters = 5
    act = solve_activations_cd(W.astype(dtype), X.astype(dtype), layout="frame_major", max_iter=iters, tol=0)
    frames = np.arange(0, T, 7) if M > 32 else np.arange(T)     # keep the numpy side seconds-long
    ref, _ = cd_iterations(X[frames], W, iters)
    assert _rel(act[frames].astype(np.float64), ref) <= (1e-10 if dtype == np.float64 else 1e-4)


def test_world_streams_concurrent_equal_sequential():
    from exemplars_vc_amd.compat import factorize_cd
    rng = np.random.default_rng(7)
    T, N, Nf = 688, 1024, 256
    src = [{"sp": rng.random((N // 2, 513)) ** 2, "ap": rng.random((N // 2, 513)),
            "f0": np.where(rng.random(Nf // 2) < 0.3, 0.0, 100 + 100 * rng.random(Nf // 2))} for _ in range(2)]
    for s in src:
        s["f0"] = np.concatenate([s["f0"], np.zeros(N // 2 - Nf // 2)])
    conv = {"sp": rng.random((T, 513)) ** 2, "ap": rng.random((T, 513)),
            "f0": np.where(rng.random(T) < 0.3, 0.0, 100 + 100 * rng.random(T))}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        factorize_cd.factorize(conv, src, use_stft=False)             # warm-up: library, streams, workspaces
        t0 = time.perf_counter()
        seq = factorize_cd.factorize(conv, src, use_stft=False, concurrent=False)
        t_seq = time.perf_counter() - t0
        t0 = time.perf_counter()
        par = factorize_cd.factorize(conv, src, use_stft=False)
        t_par = time.perf_counter() - t0
    assert sorted(par) == ["H_ap", "H_f0", "H_sp"]
    for k in par:
        assert par[k].shape == (N, T)
        assert np.array_equal(par[k], seq[k]), k
    assert t_par <= 1.25 * t_seq + 0.05, (t_par, t_seq)
