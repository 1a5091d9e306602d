"""Dictionary learning under the Kullback-Leibler loss on the GPU (evc_nmf_learn, loss = EVC_LOSS_KL) against
scikit-learn's recorded results (tests/golden/dictkl_sk_*.npz) and the numpy restatement that reproduces them
(learn_kl_restatement.py, test_learn_kl_host.py).  `-m gpu`.

float64: W and H within rtol 1e-9 with zeros exact, n_iter equal.  float32: ||delta|| / ||ref|| <= 1e-4."""
import ctypes as C
import glob
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from learn_kl_restatement import error as kl_error, learn  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "dictkl_sk_*.npz")))
RTOL = 1e-9


def close(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    if want.dtype == np.float32:
        r = np.linalg.norm(got.astype(float) - want) / np.linalg.norm(want)
        print(f"{what}: float32 norm-relative error {r:.3e}")
        assert got.dtype == np.float32 and r <= 1e-4, (what, r)
        return
    nz = want != 0
    r = float(np.max(np.abs(got[nz] - want[nz]) / np.abs(want[nz])))
    print(f"{what}: max relative error {r:.3e}")
    assert r <= RTOL and not got[~nz].any(), (what, r)


def test_there_are_fixtures():
    assert len(FILES) == 7


@pytest.mark.parametrize("path", FILES, ids=os.path.basename)
def test_fixture_through_learn_dictionary(path):
    import exemplars_vc_amd as evc
    d = np.load(path)
    tol = float(d["tol"])
    W, H, info = evc.learn_dictionary(d["X"], d["W0"], d["H0"], layout="bin_major", iters=int(d["max_iter"]),
                                      surface="sklearn", check_every=10 if tol > 0 else 0, tol=tol, info=True, loss="kl")
    assert info["n_iter"] == int(d["n_iter"])
    close(W, d["W"], "W")
    close(H, d["H"], "H")
    if tol > 0:
        k = 1 + info["n_iter"] // 10
        assert np.isfinite(info["err"][:k]).all() and np.isnan(info["err"][k:]).all()
    if path.endswith("_zeros.npz"):
        assert np.isfinite(W).all() and np.isfinite(H).all()
        assert not W[:, 5].any() and not H[5].any() and not H[:, [3, 77]].any()


@pytest.mark.parametrize("path", FILES, ids=os.path.basename)
def test_fixture_through_the_sklearn_mirror(path):
    from exemplars_vc_amd.compat.factorize import non_negative_factorization_mu
    d = np.load(path)
    Wsk, Hsk, n_iter = non_negative_factorization_mu(np.ascontiguousarray(d["X"].T), np.ascontiguousarray(d["H0"].T),
                                                     np.ascontiguousarray(d["W0"].T), update_H=True,
                                                     tol=float(d["tol"]), max_iter=int(d["max_iter"]),
                                                     beta_loss="kullback-leibler")
    assert n_iter == int(d["n_iter"])
    close(Hsk.T, d["W"], "W")
    close(Wsk.T, d["H"], "H")


@pytest.mark.parametrize("S", [1, 3, 7])
def test_split_reduction_is_deterministic(S):
    """T = 150 in 7 ranges: 21 or 22 frames each, no multiple of the MFMA's 4"""
    import exemplars_vc_amd as evc
    d = np.load(os.path.join(GOLDEN, "dictkl_sk_m50_r24_t150_k40.npz"))
    runs = [evc.learn_dictionary(d["X"], d["W0"], d["H0"], layout="bin_major", iters=40, check_every=0, splits=S,
                                 info=True, loss="kl") for _ in range(2)]
    assert runs[0][2]["splits"] == S
    close(runs[0][0], d["W"], "W")
    close(runs[0][1], d["H"], "H")
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])


SENTINEL = -12345.25


@pytest.mark.parametrize("layout", ["bin_major", "frame_major"])
def test_leading_dimensions_and_layouts(layout):
    """a raw call with every leading dimension at its minimum + 3: the padding of W and H keeps its sentinels"""
    import torch
    from exemplars_vc_amd import _lib
    L = _lib.lib()
    d = np.load(os.path.join(GOLDEN, "dictkl_sk_m50_r24_t150_k40.npz"))
    fm = layout == "frame_major"
    mats = {k: (np.ascontiguousarray(d[k].T) if fm else d[k]) for k in ("X", "W0", "H0")}
    M, T = d["X"].shape
    R = d["W0"].shape[1]

    def padded(a):
        b = np.full((a.shape[0], a.shape[1] + 3), SENTINEL)
        b[:, :a.shape[1]] = a
        return torch.from_numpy(b).cuda()
    Xb, Wb, Hb = padded(mats["X"]), padded(mats["W0"]), padded(mats["H0"])
    o = _lib.LearnOpts()
    o.struct_bytes = C.sizeof(_lib.LearnOpts)
    o.dtype, o.layout, o.surface, o.iters = _lib.F64, _lib.FRAME_MAJOR if fm else _lib.BIN_MAJOR, _lib.LEARN_SKLEARN, 40
    o.loss = _lib.LOSS_KL
    nb = int(L.evc_learn_workspace_bytes(M, R, T, _lib.F64))
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    st = L.evc_nmf_learn(Xb.data_ptr(), Xb.shape[1], Wb.data_ptr(), Wb.shape[1], Hb.data_ptr(), Hb.shape[1], M, R, T,
                         C.byref(o), ws.data_ptr(), nb, None, None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == 0
    torch.cuda.synchronize()
    Wh, Hh = Wb.cpu().numpy(), Hb.cpu().numpy()
    assert (Wh[:, -3:] == SENTINEL).all() and (Hh[:, -3:] == SENTINEL).all()
    close(Wh[:, :-3].T if fm else Wh[:, :-3], d["W"], "W")
    close(Hh[:, :-3].T if fm else Hh[:, :-3], d["H"], "H")


def close_err(got, want, X, W, H):
    """the error trace against the restatement's, as err^2 = 2 KL(X || W H).  W and H are held to a relative 1e-9 each,
    so V = W H moves by at most delta = 2e-9 relative, and d(2 KL) <= 2 delta sum |V - X| <= 4e-9 (sum X + sum V), V
    taken from the restatement's result (the updates keep sum V at sum X from the first iteration on).  Where the fit is
    exact (one frame) the divergence itself is rounding noise and no relative bound on it means anything"""
    got, want = np.asarray(got), np.asarray(want)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    atol = 4e-9 * (float(np.sum(X)) + float(np.sum(W @ H)))
    print("err^2", got[ok] ** 2, "restatement", want[ok] ** 2, "atol", atol)
    np.testing.assert_allclose(got[ok] ** 2, want[ok] ** 2, rtol=1e-8, atol=atol)


def _random_case(M, R, T, seed):
    rng = np.random.default_rng(seed)
    return rng.random((M, T)) + 0.01, rng.random((M, R)) + 1e-4, rng.random((R, T)) + 1e-4


@pytest.mark.parametrize("M,R,T", [(50, 24, 1), (50, 1, 150), (17, 3, 5)])
def test_edges_one_frame_one_component(M, R, T):
    import exemplars_vc_amd as evc
    X, W0, H0 = _random_case(M, R, T, 7 * M + R + T)
    W, H, info = evc.learn_dictionary(X, W0, H0, layout="bin_major", iters=12, check_every=4, info=True, loss="kl")
    Wr, Hr, n_iter, err = learn(X, W0, H0, 12, 4, 0.0)
    assert info["n_iter"] == n_iter == 12
    close(W, Wr, "W")
    close(H, Hr, "H")
    close_err(info["err"], err, X, Wr, Hr)


def test_zero_iterations_return_the_start_and_its_error():
    import exemplars_vc_amd as evc
    X, W0, H0 = _random_case(50, 24, 150, 11)
    W, H, info = evc.learn_dictionary(X, W0, H0, layout="bin_major", iters=0, check_every=10, info=True, loss="kl")
    assert np.array_equal(W, W0) and np.array_equal(H, H0) and info["n_iter"] == 0
    assert info["err"].shape == (1,)
    np.testing.assert_allclose(info["err"][0], kl_error(X, W0, H0), rtol=1e-12)


def test_error_never_rises():
    """the multiplicative updates do not increase the divergence (Lee & Seung); the restatement's trace holds the same
    bound (test_learn_kl_host.py)"""
    import exemplars_vc_amd as evc
    d = np.load(os.path.join(GOLDEN, "dictkl_sk_m50_r24_t150_k40.npz"))
    _, _, info = evc.learn_dictionary(d["X"], d["W0"], d["H0"], layout="bin_major", iters=40, check_every=1, info=True,
                                      loss="kl")
    err = info["err"]
    assert err.shape == (41,) and np.isfinite(err).all()
    rise = np.diff(err).max()
    print(f"largest rise {rise:.3e} of err_init {err[0]:.3e}")
    assert rise <= 1e-12 * err[0]
    assert err[-1] < err[0]


def _rank16(seed=3):
    rng = np.random.default_rng(seed)
    Wa, Wb = rng.random((25, 16)) + 0.05, rng.random((25, 16)) + 0.05
    G = rng.random((16, 300)) * (rng.random((16, 300)) < 0.4) + 1e-3
    return Wa @ G, Wb @ G


@pytest.mark.parametrize("layout", ["bin_major", "frame_major"])
def test_compact_dictionary(layout):
    import exemplars_vc_amd as evc
    A, B = _rank16()
    fm = layout == "frame_major"
    args = (np.ascontiguousarray(A.T), np.ascontiguousarray(B.T)) if fm else (A, B)
    Wa, Wb, G, info = evc.compact_dictionary(*args, 16, iters=60, layout=layout, loss="kl")
    if fm:
        Wa, Wb, G = Wa.T, Wb.T, G.T
    D = np.vstack([A, B])
    W0 = np.maximum(D[:, (np.arange(16) * 300) // 16], 1e-6)
    G0 = np.full((16, 300), np.sqrt(D.mean() / 16))
    Wr, Gr, n_iter, err = learn(D, W0, G0, 60, 10, 0.0, S=info["splits"])
    assert info["n_iter"] == n_iter == 60
    close(np.vstack([Wa, Wb]), Wr, "W")
    close(G, Gr, "G")
    close_err(info["err"], err, D, Wr, Gr)
    assert info["err"][-1] < info["err"][0]


def test_frobenius_is_unchanged_by_the_keyword():
    import exemplars_vc_amd as evc
    d = np.load(os.path.join(GOLDEN, "dictmu_sk_m50_r24_t150_k40.npz"))
    kw = dict(layout="bin_major", iters=40, check_every=10, info=True)
    W0, H0, i0 = evc.learn_dictionary(d["X"], d["W0"], d["H0"], **kw)
    W1, H1, i1 = evc.learn_dictionary(d["X"], d["W0"], d["H0"], loss="frobenius", **kw)
    assert np.array_equal(W0, W1) and np.array_equal(H0, H1) and np.array_equal(i0["err"], i1["err"])
    close(W1, d["W"], "W")
    close(H1, d["H"], "H")


def test_pymf_surface_rejects_the_loss():
    import exemplars_vc_amd as evc
    X, W0, H0 = _random_case(17, 3, 5, 1)
    with pytest.raises(ValueError, match="pymf"):
        evc.learn_dictionary(X, W0, H0, layout="bin_major", iters=1, surface="pymf", loss="kullback-leibler")
