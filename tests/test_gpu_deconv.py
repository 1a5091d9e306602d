"""evc_deconv_solve / evc_deconv_synthesize on the GPU against the numpy restatement (tests/deconv_restatement.py), which the
L = 1 cases anchor to recorded scikit-learn results.  Tolerances are the project's own: float64 relative 1e-9 on the
reference's non-zero entries with the zeros exact, float32 norm-relative 1e-4 (the restatement in float64 and in extended
precision differ by at most 4.4e-14 on these shapes; a float32 run of the same arithmetic drifts by at most 6.0e-6)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deconv_restatement as dr  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LOSSES = ("frobenius", "kullback-leibler")
_cache = {}


def evc():
    import exemplars_vc_amd
    return exemplars_vc_amd


def rloss(loss):
    return "frobenius" if loss == "frobenius" else "kl"


def problem(M, N, T, L, offs=None):
    key = (M, N, T, L, None if offs is None else tuple(offs))
    if key not in _cache:
        _cache[key] = dr.problem(M, N, T, L, utt_offsets=offs)         # shared: the tests copy before they change one
    return _cache[key]


def reference(M, N, T, L, loss, K, **kw):
    key = ("ref", M, N, T, L, loss, K, tuple(sorted(kw.items())))
    if key not in _cache:
        A, X = problem(M, N, T, L)
        _cache[key] = dr.solve(A, X, loss=rloss(loss), iters=K, **kw)
    return _cache[key]


def close64(got, ref, rtol=1e-9):
    assert got.dtype == np.float64 and got.shape == ref.shape
    nz = ref != 0
    assert np.array_equal(got == 0, ~nz)
    worst = float(np.max(np.abs(got[nz] - ref[nz]) / np.abs(ref[nz]))) if nz.any() else 0.0
    print("worst relative error %.3e" % worst)
    assert worst <= rtol


def close32(got, ref):
    assert got.dtype == np.float32
    err = float(np.linalg.norm(got.astype(np.float64) - ref) / np.linalg.norm(ref))
    print("norm-relative error %.3e" % err)
    assert err <= 1e-4


GEOMETRY = [(25, 64, 50, 4, 50), (25, 80, 37, 16, 40), (7, 33, 5, 8, 40), (256, 40, 21, 2, 40), (1, 48, 37, 5, 40),
            (201, 48, 40, 3, 40)]


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("shape", GEOMETRY, ids=lambda s: "m%d_n%d_t%d_l%d_k%d" % s)
def test_geometry_float64(shape, loss):
    M, N, T, L, K = shape
    A, X = problem(M, N, T, L)
    ref, n_ref, tr_ref = reference(M, N, T, L, loss, K, check_every=10)
    H, info = evc().solve_activations_deconv(A, X, loss=loss, iters=K, check_every=10, info=True)
    assert info["kernel"] == "k_deconv_update" and info["taps"] == L and info["n_iter"].tolist() == [K]
    close64(H, ref)
    np.testing.assert_allclose(info["err"], tr_ref, rtol=1e-9, atol=0)
    assert np.all(np.diff(info["err"][0]) <= 0)


@pytest.mark.parametrize("loss", LOSSES)
def test_geometry_float32(loss):
    M, N, T, L, K = GEOMETRY[-1]
    A, X = problem(M, N, T, L)
    ref, _, _ = reference(M, N, T, L, loss, K, check_every=10)
    H = evc().solve_activations_deconv(A.astype(np.float32), X.astype(np.float32), loss=loss, iters=K)
    close32(H, ref)


@pytest.mark.parametrize("name,loss", [("sklearn_m25_n64_t32_k50", "frobenius"), ("sklearnkl_m25_n64_t32_k50", "kullback-leibler"),
                                       ("sklearn_l1_m25_n256_t64_k100", "frobenius")])
def test_one_tap_is_recorded_sklearn(name, loss):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    A, X, K, l1 = d["W_rows"][None], d["X_rows"], int(d["n_iter"]), float(d["l1_reg"])
    H = evc().solve_activations_deconv(A, X, loss=loss, layout="frame_major", iters=K, l1=l1)
    close64(H.T, d["H"])
    Hb = evc().solve_activations_beta(A[0], X, beta=2.0 if loss == "frobenius" else 1.0, layout="frame_major", iters=K, l1=l1)
    close64(H, Hb, rtol=1e-12)


BATCH = (37, 0, 5, 16, 50)


@pytest.mark.parametrize("loss", LOSSES)
def test_batch_is_bitwise_the_per_utterance_calls(loss):
    offs = np.concatenate([[0], np.cumsum(BATCH)]).tolist()
    A, X = problem(25, 64, offs[-1], 4, offs)
    kw = dict(loss=loss, iters=30, check_every=10, stop_rule="sklearn", tol=1e-9, info=True)
    H, info = evc().solve_activations_deconv(A, X, utt_offsets=offs, **kw)
    assert np.isfinite(H).all() and info["n_iter"].tolist() == [30] * 5 and np.isnan(info["err"][1]).all()
    for u, (a, b) in enumerate(zip(offs[:-1], offs[1:])):
        if b == a:
            continue
        Hu, iu = evc().solve_activations_deconv(A, np.ascontiguousarray(X[:, a:b]), **kw)
        assert H[:, a:b].tobytes() == Hu.tobytes() and info["err"][u].tobytes() == iu["err"][0].tobytes()
    ref, _, tr = dr.solve(A, X, loss=rloss(loss), iters=30, check_every=10, utt_offsets=offs)
    close64(H, ref)
    np.testing.assert_allclose(info["err"], tr, rtol=1e-9, atol=0)
    # a NaN in one frame of utterance 2 spreads inside it (the model couples its frames) and nowhere else
    Xn = X.copy()
    Xn[3, offs[2] + 1] = np.nan
    Hn = evc().solve_activations_deconv(A, Xn, utt_offsets=offs, loss=loss, iters=30)
    keep = np.ones(offs[-1], dtype=bool)
    keep[offs[2]:offs[3]] = False
    assert Hn[:, keep].tobytes() == H[:, keep].tobytes() and np.isnan(Hn[:, offs[2]:offs[3]]).any()


@pytest.mark.parametrize("loss", LOSSES)
def test_layouts_and_strides(loss):
    import torch
    M, N, T, L, K = 25, 64, 50, 4, 20
    A, X = problem(M, N, T, L)
    ref, _, _ = reference(M, N, T, L, loss, K)
    e = evc()
    H = e.solve_activations_deconv(A, X, loss=loss, iters=K)
    close64(H, ref)
    Hf = e.solve_activations_deconv(np.ascontiguousarray(A.transpose(0, 2, 1)), np.ascontiguousarray(X.T), loss=loss,
                                    layout="frame_major", iters=K)
    assert Hf.T.tobytes() == H.tobytes()
    # lda / ldx / ldh beyond the extent, a tap_stride beyond one matrix, the padding untouched
    for layout in ("bin_major", "frame_major"):
        fm = layout == "frame_major"
        a, x = (A.transpose(0, 2, 1), X.T) if fm else (A, X)
        Ab = torch.full((L, a.shape[1] + 3, a.shape[2] + 5), -7.0, dtype=torch.float64, device="cuda")
        Xb = torch.full((x.shape[0], x.shape[1] + 2), -7.0, dtype=torch.float64, device="cuda")
        hshape = (T, N) if fm else (N, T)
        Hb = torch.full((hshape[0], hshape[1] + 9), -7.0, dtype=torch.float64, device="cuda")
        Ab[:, :a.shape[1], :a.shape[2]] = torch.from_numpy(np.ascontiguousarray(a))
        Xb[:, :x.shape[1]] = torch.from_numpy(np.ascontiguousarray(x))
        out = e.solve_activations_deconv(Ab[:, :a.shape[1], :a.shape[2]], Xb[:, :x.shape[1]], loss=loss, layout=layout,
                                         iters=K, out=Hb[:, :hshape[1]])
        assert out.data_ptr() == Hb.data_ptr()
        got = Hb.cpu().numpy()
        assert (got[:, hshape[1]:] == -7.0).all() and (Xb[:, x.shape[1]:] == -7.0).all().item()
        assert (Ab[:, a.shape[1]:, :] == -7.0).all().item() and (Ab[:, :, a.shape[2]:] == -7.0).all().item()
        res = got[:, :hshape[1]]
        assert (res.T if fm else res).tobytes() == H.tobytes()
    # the taps as overlapping windows of one matrix: tap_stride = 1
    rng = np.random.default_rng(0)
    D = torch.from_numpy(rng.random((M, N + L - 1)) + 1e-3).cuda()
    Aov = torch.as_strided(D, (L, M, N), (1, N + L - 1, 1))
    assert e.solve_activations_deconv(Aov, torch.from_numpy(X).cuda(), loss=loss, iters=K).cpu().numpy().tobytes() == H.tobytes()


@pytest.mark.parametrize("loss,tol,stop_at", [("frobenius", 1.2e-3, 50), ("kullback-leibler", 2.2e-3, 60)])
def test_stop_rule(loss, tol, stop_at):
    M, N, T, L, K = 25, 64, 50, 4, 100
    A, X = problem(M, N, T, L)
    ref, n_ref, tr_ref = reference(M, N, T, L, loss, K, check_every=10, stop_rule="sklearn", tol=tol)
    margin = dr.stop_margin(tr_ref[0], tol)
    print("the nearest deciding ratio is %.3e of tol away from it" % margin)
    assert margin > 1e-6 and n_ref.tolist() == [stop_at] and 10 < stop_at < K
    H, info = evc().solve_activations_deconv(A, X, loss=loss, iters=K, check_every=10, stop_rule="sklearn", tol=tol, info=True)
    assert info["n_iter"].tolist() == [stop_at]
    np.testing.assert_allclose(info["err"], tr_ref, rtol=1e-9, atol=0)          # NaN after the stop on both sides
    assert np.isnan(info["err"][0, stop_at // 10 + 1:]).all() and not np.isnan(info["err"][0, :stop_at // 10 + 1]).any()
    close64(H, ref)
    _, free = evc().solve_activations_deconv(A, X, loss=loss, iters=K, check_every=10, stop_rule="sklearn", tol=0.0, info=True)
    assert free["n_iter"].tolist() == [K] and np.all(np.diff(free["err"][0]) <= 0)


@pytest.mark.parametrize("loss", LOSSES)
def test_zeros_stay_zero(loss):
    M, N, T, L, K = 25, 64, 50, 4, 20
    A, X = problem(M, N, T, L)
    X = X.copy()
    X[:, 17] = 0.0
    H0 = np.random.default_rng(1).random((N, T)) + 0.1
    H0[5] = 0.0
    ref, _, _ = dr.solve(A, X, H0, loss=rloss(loss), iters=K)
    H = evc().solve_activations_deconv(A, X, H0, loss=loss, iters=K)
    assert np.isfinite(H).all() and (H[5] == 0).all()
    close64(H, ref)
    # with one tap a zero frame of X gives an exactly zero column
    H1 = evc().solve_activations_deconv(A[:1], X, H0, loss=loss, iters=K)
    assert np.isfinite(H1).all() and (H1[:, 17] == 0).all() and (H1[5] == 0).all()
    close64(H1, dr.solve(A[:1], X, H0, loss=rloss(loss), iters=K)[0])


@pytest.mark.parametrize("loss", LOSSES)
def test_two_calls_agree_bitwise(loss):
    A, X = problem(201, 48, 40, 3)
    kw = dict(loss=loss, iters=15, check_every=5, info=True)
    H1, i1 = evc().solve_activations_deconv(A, X, **kw)
    H2, i2 = evc().solve_activations_deconv(A, X, **kw)
    assert H1.tobytes() == H2.tobytes() and i1["err"].tobytes() == i2["err"].tobytes()


def test_make_dict_taps_path_and_the_recipe():
    """compat.make_dict.aligned_dictionary(taps=L): the parallel multi-frame dictionaries on the device are
    multiframe_dictionary (numpy) of the aligned frames, and convert_deconv runs on them"""
    import torch
    from exemplars_vc_amd.compat import make_dict
    e = evc()
    rng = np.random.default_rng(11)
    la, lb, order, L = [40, 31, 55], [37, 35, 50], 13, 3
    dtw_a = [rng.standard_normal((order, n)) for n in la]
    dtw_b = [rng.standard_normal((order, n)) for n in lb]
    src = [{"sp": rng.random((n, 33)) + 0.1} for n in la]
    tar = [{"sp": rng.random((n, 40)) + 0.1} for n in lb]
    A, B, rows = e.dtw_dictionary([a.T for a in dtw_a], [b.T for b in dtw_b], [f["sp"] for f in src], [f["sp"] for f in tar])
    (At, Bt), rows2 = make_dict.aligned_dictionary(dtw_a, dtw_b, src, tar, use_stft=False, key="sp", taps=L)
    assert isinstance(At, torch.Tensor) and not At.is_cpu and list(rows2) == list(rows)
    N = int(rows[-1])
    assert tuple(At.shape) == (L, N, 33) and tuple(Bt.shape) == (L, N, 40)
    assert np.array_equal(At.cpu().numpy(), e.multiframe_dictionary(A.cpu().numpy(), rows, L, layout="frame_major"))
    assert np.array_equal(Bt.cpu().numpy(), e.multiframe_dictionary(B.cpu().numpy(), rows, L, layout="frame_major"))
    assert not At[1:, np.asarray(rows[1:]) - 1].any().item()          # the last frame of a file has no successor
    X = rng.random((20, 33)) + 0.1
    Y, H = e.convert_deconv(At, X, Bt, layout="frame_major", loss="kullback-leibler", iters=10)
    ref = dr.solve(At.cpu().numpy().transpose(0, 2, 1), X.T, loss="kl", iters=10)[0]
    close64(H.T, ref)
    close64(Y.T, dr.synthesize(Bt.cpu().numpy().transpose(0, 2, 1), ref), rtol=1e-9)


def test_synthesis():
    e = evc()
    rng = np.random.default_rng(2)
    N, L, Mb = 64, 4, 513
    offs = np.concatenate([[0], np.cumsum(BATCH)]).tolist()
    T = offs[-1]
    B = rng.random((L, Mb, N))
    H = rng.random((N, T)) * (rng.random((N, T)) < 0.2)
    ref = dr.synthesize(B, H, offs)
    Y = e.synthesize_deconv(B, H, utt_offsets=offs)
    assert Y.shape == (Mb, T)
    close64(Y, ref, rtol=1e-12)
    Yf = e.synthesize_deconv(np.ascontiguousarray(B.transpose(0, 2, 1)), np.ascontiguousarray(H.T), layout="frame_major",
                             utt_offsets=offs)
    assert Yf.T.tobytes() == Y.tobytes()
    close64(e.synthesize_deconv(B, H), dr.synthesize(B, H), rtol=1e-12)
    close32(e.synthesize_deconv(B.astype(np.float32), H.astype(np.float32), utt_offsets=offs), ref)
    # convert = solve, then synthesis
    A, X = problem(25, 64, T, 4, offs)
    Y2, H2 = e.convert_deconv(A, X, B, loss="kullback-leibler", iters=10, utt_offsets=offs)
    Hs = e.solve_activations_deconv(A, X, loss="kullback-leibler", iters=10, utt_offsets=offs)
    assert H2.tobytes() == Hs.tobytes() and Y2.tobytes() == e.synthesize_deconv(B, Hs, utt_offsets=offs).tobytes()
