"""Coordinate descent that also learns the dictionary (evc_cd_learn, k_cd_dict_sweep) on the GPU: scikit-learn's recorded
results, the restatement at every lane geometry of the dictionary sweep, determinism, layouts and the compaction."""
import glob
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cd_learn_restatement import cd_learn  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "cdlearn_*.npz")))
F64_FILES = [p for p in FILES if not p.endswith("_f32.npz")]
F32_FILES = [p for p in FILES if p.endswith("_f32.npz")]
ids = lambda files: [os.path.basename(p)[:-4] for p in files]  # noqa: E731


def rel(a, b):
    """||a - b|| / ||b||; against an all-zero reference (the penalties can clip a tiny problem to zero) only an exact
    match counts"""
    diff, ref = float(np.linalg.norm(np.asarray(a, np.float64) - b)), float(np.linalg.norm(b))
    if ref == 0.0:
        return 0.0 if diff == 0.0 else float("inf")
    return diff / ref


def penalties(d):
    T, M = d["X_rows"].shape
    a, r = float(d["alpha_W"]), float(d["l1_ratio"])
    return dict(l1_h=M * a * r, l2_h=M * a * (1 - r), l1_w=T * a * r, l2_w=T * a * (1 - r))


def synth(M, R, T, seed):
    rng = np.random.default_rng(seed)
    Wt = rng.random((R, M)) ** 2 + 0.05
    X = (rng.random((T, R)) * (rng.random((T, R)) < 0.4)) @ Wt + 0.05 * rng.random((T, M))
    return X, rng.random((R, M)) + 0.1, rng.random((T, R)) + 0.1


@pytest.mark.parametrize("path", F64_FILES, ids=ids(F64_FILES))
def test_fixture_float64(path):
    import exemplars_vc_amd as evc
    from exemplars_vc_amd.compat.factorize import ConvergenceWarning
    from exemplars_vc_amd.compat.factorize_cd import non_negative_factorization_cd
    d = np.load(path)
    max_iter, tol, ref = int(d["max_iter"]), float(d["tol"]), d["violation"]
    W, H, info = evc.learn_dictionary_cd(d["X_rows"], d["W0_rows"], d["H0_rows"], layout="frame_major", max_iter=max_iter,
                                         tol=tol, info=True, **penalties(d))
    n = info["n_iter"]
    viol = info["violation"]
    print(os.path.basename(path), n, rel(W, d["W_rows"]), rel(H, d["H_rows"]),
          np.abs(viol[:min(n, len(ref))] - ref[:min(n, len(ref))]).max() / ref[0].sum())
    assert n == int(d["n_iter"])
    assert rel(W, d["W_rows"]) <= 1e-9 and rel(H, d["H_rows"]) <= 1e-9
    assert viol.shape == (max_iter, 2)
    assert np.abs(viol[:n] - ref).max() <= 1e-9 * ref[0].sum()
    assert np.isnan(viol[n:]).all()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        Ws, Hs, n2 = non_negative_factorization_cd(d["X_rows"], d["H0_rows"], d["W0_rows"], tol=tol, max_iter=max_iter,
                                                   alpha_W=float(d["alpha_W"]), l1_ratio=float(d["l1_ratio"]))
    assert n2 == n and np.array_equal(Ws, H) and np.array_equal(Hs, W)          # sklearn's W is the activations
    capped = [w for w in caught if issubclass(w.category, ConvergenceWarning)]
    assert len(capped) == (1 if (n == max_iter and tol > 0) else 0)


@pytest.mark.parametrize("path", F32_FILES, ids=ids(F32_FILES))
def test_fixture_float32(path):
    import exemplars_vc_amd as evc
    d = np.load(path)
    W, H, info = evc.learn_dictionary_cd(d["X_rows"], d["W0_rows"], d["H0_rows"], layout="frame_major",
                                         max_iter=int(d["max_iter"]), tol=float(d["tol"]), info=True)
    print(os.path.basename(path), info["n_iter"], rel(W, d["W_rows_f64"]), rel(H, d["H_rows_f64"]))
    assert W.dtype == np.float32 and H.dtype == np.float32
    assert info["n_iter"] == int(d["n_iter_f64"])
    assert rel(W, d["W_rows_f64"]) <= 1e-4 and rel(H, d["H_rows_f64"]) <= 1e-4


@pytest.mark.parametrize("shape", [(25, 17, 70), (201, 48, 130), (513, 16, 40)])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_first_activation_sweep_is_bitwise_the_fixed_dictionary_solve(shape, dtype):
    import exemplars_vc_amd as evc
    X, W0, H0 = (a.astype(dtype) for a in synth(*shape, seed=11))
    _, H = evc.learn_dictionary_cd(X, W0, H0, layout="frame_major", max_iter=1, tol=0.0)
    Hs = evc.solve_activations_cd(W0, X, H0=H0, layout="frame_major", max_iter=1, tol=0.0)
    assert np.array_equal(H, Hs)
    _, Hp = evc.learn_dictionary_cd(X, W0, H0, layout="frame_major", max_iter=1, tol=0.0, l1_h=0.3, l2_h=0.2)
    Hps = evc.solve_activations_cd(W0, X, H0=H0, layout="frame_major", max_iter=1, tol=0.0, l1=0.3, l2=0.2)
    assert np.array_equal(Hp, Hps) and not np.array_equal(Hp, H)


@pytest.mark.parametrize("S", [1, 3, 7])
def test_two_runs_are_bitwise_equal(S):
    import exemplars_vc_amd as evc
    d = np.load(os.path.join(GOLDEN, "cdlearn_m50_r33_t520_zero.npz"))
    runs = [evc.learn_dictionary_cd(d["X_rows"], d["W0_rows"], d["H0_rows"], layout="frame_major", max_iter=25, tol=1e-4,
                                    info=True, splits=S) for _ in range(2)]
    (W1, H1, i1), (W2, H2, i2) = runs
    assert i1["splits"] == S
    assert np.array_equal(W1, W2) and np.array_equal(H1, H2)
    assert np.array_equal(i1["violation"], i2["violation"], equal_nan=True)
    assert rel(W1, d["W_rows"]) <= 1e-9 and rel(H1, d["H_rows"]) <= 1e-9
    assert (W1[2] == 0).all() and (H1[:, 2] == 0).all()           # hess == 0 on both sides: the component is left alone


def test_layouts_and_padded_leading_dimensions():
    import torch
    import exemplars_vc_amd as evc
    X, W0, H0 = synth(70, 33, 130, seed=5)
    kw = dict(max_iter=6, tol=0.0, l1_h=0.01, l2_w=0.02)
    Wf, Hf, info = evc.learn_dictionary_cd(X, W0, H0, layout="frame_major", info=True, **kw)
    Wb, Hb, infob = evc.learn_dictionary_cd(X.T, W0.T, H0.T, layout="bin_major", info=True, **kw)
    assert np.array_equal(Wb.T, Wf) and np.array_equal(Hb.T, Hf)
    assert np.array_equal(info["violation"], infob["violation"])

    def padded(a, pad, fill):
        t = torch.full((a.shape[0], a.shape[1] + pad), fill, dtype=torch.float64, device="cuda")
        t[:, :a.shape[1]] = torch.from_numpy(np.ascontiguousarray(a))
        return t, t[:, :a.shape[1]]
    for lay, (x, w, h) in (("frame_major", (X, W0, H0)), ("bin_major", (X.T, W0.T, H0.T))):
        (xs, xv), (ws, wv), (hs, hv) = padded(x, 3, 7.0), padded(w, 5, -3.0), padded(h, 9, -5.0)
        evc.learn_dictionary_cd(xv, None, None, layout=lay, out_w=wv, out_h=hv, **kw)
        torch.cuda.synchronize()
        Wp, Hp = wv.cpu().numpy(), hv.cpu().numpy()
        assert np.array_equal(Wp if lay == "frame_major" else Wp.T, Wf)
        assert np.array_equal(Hp if lay == "frame_major" else Hp.T, Hf)
        assert (ws[:, w.shape[1]:] == -3.0).all() and (hs[:, h.shape[1]:] == -5.0).all()      # the padding is untouched


# (M, R, T, L): every lane geometry of k_cd_dict_sweep; M = 70 at L = 4 fills more than one wavefront and leaves a ragged
# last one
GEOMETRIES = [(8, 5, 64, 1), (8, 17, 64, 2), (70, 33, 64, 4), (8, 130, 300, 16), (5, 300, 400, 32), (3, 1024, 1100, 64),
              (1, 1, 1, 1)]


@pytest.mark.parametrize("M,R,T,L", GEOMETRIES, ids=[f"m{g[0]}_r{g[1]}_L{g[3]}" for g in GEOMETRIES])
def test_dictionary_sweep_at_every_lane_geometry(M, R, T, L):
    import exemplars_vc_amd as evc
    lanes = 1
    while -(-R // lanes) > 16:
        lanes *= 2
    assert lanes == L
    from exemplars_vc_amd import _lib
    X, W0, H0 = synth(M, R, T, seed=1000 + R)
    if R > 16:
        W0[5, ::2] = 0.0            # bins that start at zero in a component: the projected gradient's other branch
        H0[:, 3] = 0.0              # an unused component: its row of G is l2 on the diagonal alone
    S = _lib.lib().evc_cd_learn_splits(M, R, T)     # the one-row calls below take the same frame ranges
    kw = dict(layout="frame_major", max_iter=2, tol=0.0, l1_w=0.05, l2_w=0.1, update="dict", splits=S)
    W, H, info = evc.learn_dictionary_cd(X, W0, H0, info=True, **kw)
    assert info["splits"] == S
    Wr, Hr, n, viol = cd_learn(X, W0, H0, 2, 0.0, l1_w=0.05, l2_w=0.1, S=S, update="dict")
    print(M, R, T, L, S, rel(W, Wr), np.abs(info["violation"] - viol).max() / viol[0].sum())
    assert info["n_iter"] == 2 and np.array_equal(H, H0)
    assert rel(W, Wr) <= 1e-9
    assert (info["violation"][:, 0] == 0).all()
    assert np.abs(info["violation"][:, 1] - viol[:, 1]).max() <= 1e-9 * viol[0, 1]
    # rows that share a wavefront are bitwise the rows of a call on that row alone
    for m in sorted({0, M // 2, M - 1}):
        Wm, _ = evc.learn_dictionary_cd(X[:, m:m + 1], W0[:, m:m + 1], H0, **kw)
        assert np.array_equal(Wm[:, 0], W[:, m]), m


def test_frobenius_error_never_rises():
    import exemplars_vc_amd as evc
    X, W, H = synth(50, 33, 520, seed=9)
    err0 = prev = np.linalg.norm(X - H @ W)
    for _ in range(12):
        W, H = evc.learn_dictionary_cd(X, W, H, layout="frame_major", max_iter=1, tol=0.0)
        err = np.linalg.norm(X - H @ W)
        assert err <= prev + 1e-12 * err0
        prev = err
    assert prev < 0.5 * err0


def test_compact_dictionary_by_coordinate_descent():
    import exemplars_vc_amd as evc
    rng = np.random.default_rng(4)
    G = rng.random((12, 90)) * (rng.random((12, 90)) < 0.5)
    A = (rng.random((40, 12)) ** 2 + 0.05) @ G + 0.01 * rng.random((40, 90))
    B = (rng.random((25, 12)) ** 2 + 0.05) @ G + 0.01 * rng.random((25, 90))
    Wa0, Wb0, G0, _ = evc.compact_dictionary(A, B, 12, iters=0, solver="cd")
    Wa, Wb, Gc, info = evc.compact_dictionary(A, B, 12, iters=30, solver="cd")
    assert Wa.shape == (40, 12) and Wb.shape == (25, 12) and Gc.shape == (12, 90) and info["n_iter"] == 30
    for a in (Wa, Wb, Gc):
        assert np.isfinite(a).all() and (a >= 0).all()
    D = np.vstack([A, B])
    err = lambda wa, wb, g: np.linalg.norm(D - np.vstack([wa, wb]) @ g)  # noqa: E731
    assert err(Wa, Wb, Gc) < 0.5 * err(Wa0, Wb0, G0)
