"""Dictionary learning under any beta-divergence on the GPU (evc_beta_learn) against scikit-learn's recorded results
(tests/golden/dictbeta_sk_*.npz) and the numpy restatement that reproduces them (beta_learn_restatement.py,
test_beta_learn_host.py).  `-m gpu`.

float64: W and H within rtol 1e-9 with zeros exact, n_iter equal.  float32: ||delta|| / ||ref|| <= 1e-4."""
import ctypes as C
import functools
import glob
import hashlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beta_learn_restatement as blr  # noqa: E402
from beta_restatement import EPS  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "dictbeta_sk_*.npz")))
RTOL = 1e-9
FUSED_MAX_R = 256           # what the fused route holds when forced (include/evc.h)


def close(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    if want.dtype == np.float32:
        r = np.linalg.norm(got.astype(float) - want) / np.linalg.norm(want)
        print(f"{what}: float32 norm-relative error {r:.3e}")
        assert got.dtype == np.float32 and r <= 1e-4, (what, r)
        return
    nz = want != 0
    r = float(np.max(np.abs(got[nz] - want[nz]) / np.abs(want[nz])))
    print(f"{what}: max relative error {r:.3e}, zeros {int((~nz).sum())}")
    assert r <= RTOL and not got[~nz].any(), (what, r)


def _slack(X, W, H, beta):
    V = np.maximum(W @ H, EPS)
    return float(np.sum(V ** (beta - 1.0) * np.abs(V - X)))


def close_err(got, want, X, beta, factors):
    """the error trace against the reference's, as err^2 = 2 D_beta(X || W H).  dD/dV = V^(beta-2) (V - X) per entry; W and
    H are held to a relative 1e-9 each, so V = W H moves by at most delta = 2e-9 relative and
    d(2 D) <= 2 delta sum V^(beta-1) |V - X|, the sum taken at the start and at the result (the larger of the two: the
    updates do not increase the divergence).  Where the fit is exact (one frame) the divergence itself is rounding noise
    and no relative bound on it means anything.  beta = 1: sum V |1 - X / V| <= sum X + sum V, test_gpu_learn_kl's term"""
    got, want = np.asarray(got), np.asarray(want)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    atol = 4e-9 * max(_slack(X, W, H, beta) for W, H in factors)
    print("err^2", got[ok] ** 2, "reference", want[ok] ** 2, "atol", atol)
    np.testing.assert_allclose(got[ok] ** 2, want[ok] ** 2, rtol=1e-8, atol=atol)


def penalties(d):
    M, T = d["X"].shape
    a, r = float(d["alpha"]), float(d["l1_ratio"])
    return dict(l1_h=M * a * r, l2_h=M * a * (1 - r), l1_w=T * a * r, l2_w=T * a * (1 - r))


@functools.lru_cache(maxsize=None)
def restated(path):
    """the restatement's run of a fixture, computed once: (W, H, n_iter, err)"""
    d = np.load(path)
    return blr.learn(d["X"], d["W0"], d["H0"], float(d["beta"]), int(d["max_iter"]), 10, float(d["tol"]),
                     *penalties(d).values(), dtype=np.dtype(str(d["dtype"])))


def test_there_are_fixtures():
    assert len(FILES) == 18


def _check_fixture(path, route):
    import exemplars_vc_amd as evc
    d = np.load(path)
    tol, beta = float(d["tol"]), float(d["beta"])
    R = d["W0"].shape[1]
    kw = dict(beta=beta, layout="bin_major", iters=int(d["max_iter"]), check_every=10, tol=tol, info=True, route=route,
              **penalties(d))
    if route == "fused" and R > FUSED_MAX_R:
        with pytest.raises(evc._lib.EvcError) as e:
            evc.learn_dictionary_beta(d["X"], d["W0"], d["H0"], **kw)
        assert e.value.status == -3
        return
    W, H, info = evc.learn_dictionary_beta(d["X"], d["W0"], d["H0"], **kw)
    assert info["n_iter"] == int(d["n_iter"])
    M, T = d["X"].shape
    assert info["route"] == (route or ("fused", "unfused")[evc._lib.lib().evc_beta_learn_route(M, R, T) - 1])
    close(W, d["W"], "W")
    close(H, d["H"], "H")
    k = 1 + info["n_iter"] // 10
    assert np.isfinite(info["err"][:k]).all() and np.isnan(info["err"][k:]).all()
    if d["X"].dtype == np.float64:
        Wr, Hr, n_iter, err = restated(path)
        assert n_iter == info["n_iter"]
        close_err(info["err"], err, d["X"], beta, [(d["W0"], d["H0"]), (Wr, Hr)])
    else:
        np.testing.assert_allclose(info["err"][:k], d["err"][:k], rtol=1e-4)
    if "_zeros_" in path:
        assert np.isfinite(W).all() and np.isfinite(H).all()
        assert not H[5].any() and not H[:, [3, 77]].any()
    if "_flush_" in path:
        assert (W == 0).sum() >= 10 and ((H == 0).sum() >= 10) == (beta < 1)


@pytest.mark.parametrize("path", FILES, ids=os.path.basename)
def test_fixture_through_learn_dictionary_beta(path):
    _check_fixture(path, None)


@pytest.mark.parametrize("route", ["fused", "unfused"])
@pytest.mark.parametrize("path", FILES, ids=os.path.basename)
def test_fixture_with_the_route_forced(path, route):
    _check_fixture(path, route)


def test_default_routes():
    import exemplars_vc_amd as evc
    for name, route in (("dictbeta_sk_m17_r300_t40_k20_b0p5", "unfused"), ("dictbeta_sk_m25_r17_t70_k40_b0", "fused")):
        d = np.load(os.path.join(GOLDEN, name + ".npz"))
        _, _, info = evc.learn_dictionary_beta(d["X"], d["W0"], d["H0"], beta=float(d["beta"]), layout="bin_major", iters=1,
                                               check_every=0, info=True)
        assert info["route"] == route


@pytest.mark.parametrize("path", FILES, ids=os.path.basename)
def test_fixture_through_the_sklearn_mirror(path):
    from exemplars_vc_amd.compat.factorize import non_negative_factorization_beta
    d = np.load(path)
    Wsk, Hsk, n_iter = non_negative_factorization_beta(np.ascontiguousarray(d["X"].T), np.ascontiguousarray(d["H0"].T),
                                                       np.ascontiguousarray(d["W0"].T), float(d["beta"]),
                                                       tol=float(d["tol"]), max_iter=int(d["max_iter"]),
                                                       alpha_W=float(d["alpha"]), l1_ratio=float(d["l1_ratio"]))
    assert n_iter == int(d["n_iter"])
    close(Hsk.T, d["W"], "W")
    close(Wsk.T, d["H"], "H")


@pytest.mark.parametrize("route", ["fused", "unfused"])
@pytest.mark.parametrize("S", [1, 3, 7])
def test_split_reduction_is_deterministic(S, route):
    """T = 150 in 7 ranges: 21 or 22 frames each, no multiple of the MFMA's 4 (nor of the fused kernel's 16)"""
    import exemplars_vc_amd as evc
    d = np.load(os.path.join(GOLDEN, "dictbeta_sk_m50_r24_t150_k40_reg_b0p5.npz"))
    runs = [evc.learn_dictionary_beta(d["X"], d["W0"], d["H0"], beta=0.5, layout="bin_major", iters=40, check_every=0,
                                      splits=S, info=True, route=route, **penalties(d)) for _ in range(2)]
    assert runs[0][2]["splits"] == S and runs[0][2]["route"] == route
    close(runs[0][0], d["W"], "W")
    close(runs[0][1], d["H"], "H")
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])


SENTINEL = -12345.25


@pytest.mark.parametrize("route", [1, 2])
@pytest.mark.parametrize("layout", ["bin_major", "frame_major"])
def test_leading_dimensions_and_layouts(layout, route):
    """a raw call with every leading dimension at its minimum + 3: the padding of W and H keeps its sentinels"""
    import torch
    from exemplars_vc_amd import _lib
    L = _lib.lib()
    d = np.load(os.path.join(GOLDEN, "dictbeta_sk_m25_r17_t70_k30_flush_b0.npz"))
    fm = layout == "frame_major"
    mats = {k: (np.ascontiguousarray(d[k].T) if fm else d[k]) for k in ("X", "W0", "H0")}
    M, T = d["X"].shape
    R = d["W0"].shape[1]

    def padded(a):
        b = np.full((a.shape[0], a.shape[1] + 3), SENTINEL)
        b[:, :a.shape[1]] = a
        return torch.from_numpy(b).cuda()
    Xb, Wb, Hb = padded(mats["X"]), padded(mats["W0"]), padded(mats["H0"])
    o = _lib.BetaLearnOpts()
    o.struct_bytes = C.sizeof(_lib.BetaLearnOpts)
    o.dtype, o.layout, o.iters, o.beta = _lib.F64, _lib.FRAME_MAJOR if fm else _lib.BIN_MAJOR, 30, 0.0
    o.reserved = route << 16
    nb = int(L.evc_beta_learn_workspace_bytes(M, R, T, _lib.F64))
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    st = L.evc_beta_learn(Xb.data_ptr(), Xb.shape[1], Wb.data_ptr(), Wb.shape[1], Hb.data_ptr(), Hb.shape[1], M, R, T,
                          C.byref(o), ws.data_ptr(), nb, None, None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == 0
    torch.cuda.synchronize()
    Wh, Hh = Wb.cpu().numpy(), Hb.cpu().numpy()
    assert (Wh[:, -3:] == SENTINEL).all() and (Hh[:, -3:] == SENTINEL).all()
    close(Wh[:, :-3].T if fm else Wh[:, :-3], d["W"], "W")
    close(Hh[:, :-3].T if fm else Hh[:, :-3], d["H"], "H")


def _random_case(M, R, T, seed):
    rng = np.random.default_rng(seed)
    return rng.random((M, T)) + 0.01, rng.random((M, R)) + 1e-4, rng.random((R, T)) + 1e-4


@pytest.mark.parametrize("route", ["fused", "unfused"])
@pytest.mark.parametrize("beta", [0.0, 1.5])
@pytest.mark.parametrize("M,R,T", [(50, 24, 1), (50, 1, 150), (1, 1, 37), (17, 3, 5)])
def test_edges_one_frame_one_component(M, R, T, beta, route):
    import exemplars_vc_amd as evc
    X, W0, H0 = _random_case(M, R, T, 7 * M + R + T)
    W, H, info = evc.learn_dictionary_beta(X, W0, H0, beta=beta, layout="bin_major", iters=12, check_every=4, info=True,
                                           route=route)
    Wr, Hr, n_iter, err = blr.learn(X, W0, H0, beta, 12, 4, 0.0)
    assert info["n_iter"] == n_iter == 12
    close(W, Wr, "W")
    close(H, Hr, "H")
    close_err(info["err"], err, X, beta, [(W0, H0), (Wr, Hr)])


def test_zero_iterations_return_the_start_and_its_error():
    import exemplars_vc_amd as evc
    X, W0, H0 = _random_case(50, 24, 150, 11)
    W, H, info = evc.learn_dictionary_beta(X, W0, H0, beta=0.0, layout="bin_major", iters=0, check_every=10, info=True)
    assert np.array_equal(W, W0) and np.array_equal(H, H0) and info["n_iter"] == 0
    assert info["err"].shape == (1,)
    np.testing.assert_allclose(info["err"][0], blr.error(X, W0, H0, 0.0), rtol=1e-12)


def test_one_iteration_activations_are_the_fixed_dictionary_solve():
    """beta = 1.5 flushes nothing: the activation half is bitwise one iteration of evc_beta_solve"""
    import exemplars_vc_amd as evc
    for layout in ("bin_major", "frame_major"):
        X, W0, H0 = _random_case(50, 24, 150, 13)
        if layout == "frame_major":
            X, W0, H0 = (np.ascontiguousarray(a.T) for a in (X, W0, H0))
        _, H = evc.learn_dictionary_beta(X, W0, H0, beta=1.5, layout=layout, iters=1, check_every=0)
        Hs = evc.solve_activations_beta(W0, X, H0, beta=1.5, layout=layout, iters=1)
        assert np.array_equal(H, Hs)


def _rank16(seed=3):
    """test_gpu_learn_kl._rank16"""
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
    Wa, Wb, G, info = evc.compact_dictionary(*args, 16, iters=60, layout=layout, beta=0)
    if fm:
        Wa, Wb, G = Wa.T, Wb.T, G.T
    D = np.vstack([A, B])
    W0 = np.maximum(D[:, (np.arange(16) * 300) // 16], 1e-6)
    G0 = np.full((16, 300), np.sqrt(D.mean() / 16))
    Wr, Gr, n_iter, err = blr.learn(D, W0, G0, 0.0, 60, 10, 0.0, S=info["splits"])
    assert info["n_iter"] == n_iter == 60 and info["route"] == "fused"
    close(np.vstack([Wa, Wb]), Wr, "W")
    close(G, Gr, "G")
    close_err(info["err"], err, D, 0.0, [(W0, G0), (Wr, Gr)])
    assert info["err"][-1] < info["err"][0]


# sha256 of the float64 activations evc_beta_solve returned for this call before BetaArgs gained its flush threshold
PARENT_DIGEST = "88510d8e5a3389e00aa07815c97f321344d920092a16dc2e5fe61d0ccbdb30b8"


def test_the_fixed_dictionary_solve_is_bitwise_unchanged():
    import exemplars_vc_amd as evc
    d = np.load(os.path.join(GOLDEN, "betamu_m25_n64_t50_reg_b0p5.npz"))
    M = d["X_rows"].shape[1]
    a, r = float(d["alpha_W"]), float(d["l1_ratio"])
    H = evc.solve_activations_beta(d["W_rows"], d["X_rows"], beta=0.5, layout="frame_major", iters=int(d["max_iter"]),
                                   init="sklearn", l1=M * a * r, l2=M * a * (1 - r))
    digest = hashlib.sha256(np.ascontiguousarray(H, dtype=np.float64).tobytes()).hexdigest()
    print("digest", digest)
    assert digest == PARENT_DIGEST
