"""evc_deconv_learn on the GPU against the numpy restatement (tests/deconv_learn_restatement.py), which test_deconv_learn_host.py
anchors to recorded scikit-learn results.  Tolerances are the project's own: float64 relative 1e-9 on the reference's non-zero
entries with the zeros exact, float32 norm-relative 1e-4, error traces relative 1e-9.  `-m gpu`."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deconv_learn_restatement as dlr  # noqa: E402
import deconv_restatement as dr  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LOSSES = ("frobenius", "kullback-leibler")
SK = ["dictmu_sk_m50_r24_t150_k40", "dictkl_sk_m50_r24_t150_k40", "dictmu_sk_m25_r130_t70_k40", "dictkl_sk_m201_r20_t100_k40",
      "dictmu_sk_m50_r24_t150_zeros", "dictkl_sk_m50_r24_t150_zeros", "dictmu_sk_m50_r24_t150_tol", "dictkl_sk_m50_r24_t150_tol"]
_cache = {}


def evc():
    import exemplars_vc_amd
    return exemplars_vc_amd


def problem(M, R, T, L, offs=None):
    key = (M, R, T, L, None if offs is None else tuple(offs))
    if key not in _cache:
        _cache[key] = dlr.problem(M, R, T, L, offs)        # shared: the tests copy before they change one
    return _cache[key]


def reference(M, R, T, L, offs, loss, K, **kw):
    key = ("ref", M, R, T, L, None if offs is None else tuple(offs), loss, K, tuple(sorted(kw.items())))
    if key not in _cache:
        X, W0, H0 = problem(M, R, T, L, offs)
        _cache[key] = dlr.learn(W0, X, H0, loss, K, offs, **kw)
    return _cache[key]


def close64(got, ref, what, rtol=1e-9):
    got = np.asarray(got)
    assert got.dtype == np.float64 and got.shape == ref.shape
    nz = ref != 0
    assert np.array_equal(got == 0, ~nz), what
    worst = float(np.max(np.abs(got[nz] - ref[nz]) / np.abs(ref[nz]))) if nz.any() else 0.0
    print("%s: worst relative error %.3e" % (what, worst))
    assert worst <= rtol, what


def close32(got, ref, what):
    assert got.dtype == np.float32
    err = float(np.linalg.norm(got.astype(np.float64) - ref) / np.linalg.norm(ref))
    print("%s: norm-relative error %.3e" % (what, err))
    assert err <= 1e-4, what


GEOMETRY = [(25, 12, 90, 4, (0, 37, 37, 40, 90)), (7, 33, 21, 8, None), (1, 5, 37, 5, None), (256, 20, 40, 2, None),
            (25, 130, 70, 3, (0, 1, 70)), (25, 17, 33, 16, (0, 16, 33))]
geo_id = lambda s: "m%d_r%d_t%d_l%d" % s[:4]


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("shape", GEOMETRY, ids=geo_id)
def test_geometry_float64(shape, loss):
    M, R, T, L, offs = shape
    X, W0, H0 = problem(*shape)
    Wr, Hr, n_ref, tr = reference(*shape, loss, 5, check_every=1)
    W, H, info = evc().learn_dictionary_deconv(X, W0, H0, loss=loss, layout="bin_major", iters=5, check_every=1, utt_offsets=offs,
                                               info=True)
    assert info["n_iter"] == n_ref == 5 and W.shape == (L, M, R)
    close64(W, Wr, "W")
    close64(H, Hr, "H")
    print("trace", info["err"], "restatement", tr)
    np.testing.assert_allclose(info["err"], tr, rtol=1e-9, atol=0)
    assert np.all(np.diff(info["err"]) <= 0)


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("shape", [GEOMETRY[0], GEOMETRY[3]], ids=geo_id)
def test_geometry_float32(shape, loss):
    offs = shape[4]
    X, W0, H0 = problem(*shape)
    Wr, Hr, _, _ = reference(*shape, loss, 5, check_every=1)
    W, H = evc().learn_dictionary_deconv(X.astype(np.float32), W0.astype(np.float32), H0.astype(np.float32), loss=loss,
                                         layout="bin_major", iters=5, check_every=0, utt_offsets=offs)
    close32(W, Wr, "W")
    close32(H, Hr, "H")


@pytest.mark.parametrize("loss", LOSSES)
def test_layouts_and_strides(loss):
    """frame-major gives the bits of bin-major; padded caller arrays (ldx, ldw, ldh and tap_stride beyond the extents) give the
    same bits again and keep the sentinels in their padding"""
    import torch
    shape = GEOMETRY[0]
    M, R, T, L, offs = shape
    X, W0, H0 = problem(*shape)
    Wr, Hr, _, _ = reference(*shape, loss, 5, check_every=1)
    e = evc()
    kw = dict(loss=loss, iters=5, check_every=0, utt_offsets=offs)
    W, H = e.learn_dictionary_deconv(X, W0, H0, layout="bin_major", **kw)
    close64(W, Wr, "W")
    close64(H, Hr, "H")
    Wf, Hf = e.learn_dictionary_deconv(np.ascontiguousarray(X.T), np.ascontiguousarray(W0.transpose(0, 2, 1)),
                                       np.ascontiguousarray(H0.T), layout="frame_major", **kw)
    assert Wf.transpose(0, 2, 1).tobytes() == W.tobytes() and Hf.T.tobytes() == H.tobytes()
    for layout in ("bin_major", "frame_major"):
        fm = layout == "frame_major"
        w, x, h = (W0.transpose(0, 2, 1), X.T, H0.T) if fm else (W0, X, H0)
        Wb = torch.full((L, w.shape[1] + 3, w.shape[2] + 5), -7.0, dtype=torch.float64, device="cuda")
        Xb = torch.full((x.shape[0], x.shape[1] + 2), -7.0, dtype=torch.float64, device="cuda")
        Hb = torch.full((h.shape[0], h.shape[1] + 9), -7.0, dtype=torch.float64, device="cuda")
        Wb[:, :w.shape[1], :w.shape[2]] = torch.from_numpy(np.ascontiguousarray(w))
        Xb[:, :x.shape[1]] = torch.from_numpy(np.ascontiguousarray(x))
        Hb[:, :h.shape[1]] = torch.from_numpy(np.ascontiguousarray(h))
        ow, oh = e.learn_dictionary_deconv(Xb[:, :x.shape[1]], None, None, layout=layout, out_w=Wb[:, :w.shape[1], :w.shape[2]],
                                           out_h=Hb[:, :h.shape[1]], **kw)
        assert ow.data_ptr() == Wb.data_ptr() and oh.data_ptr() == Hb.data_ptr()
        gw, gh = Wb.cpu().numpy(), Hb.cpu().numpy()
        assert (gw[:, w.shape[1]:, :] == -7.0).all() and (gw[:, :, w.shape[2]:] == -7.0).all()
        assert (gh[:, h.shape[1]:] == -7.0).all() and (Xb[:, x.shape[1]:] == -7.0).all().item()
        rw, rh = gw[:, :w.shape[1], :w.shape[2]], gh[:, :h.shape[1]]
        assert np.ascontiguousarray(rw.transpose(0, 2, 1) if fm else rw).tobytes() == W.tobytes()
        assert np.ascontiguousarray(rh.T if fm else rh).tobytes() == H.tobytes()


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("S", [1, 3, 7])
@pytest.mark.parametrize("shape", [GEOMETRY[0], (50, 24, 150, 4, (0, 61, 150))], ids=geo_id)
def test_frame_ranges(shape, S, loss):
    """the ranges are whole frame tiles: 8 tiles (3 + 0 + 1 + 4) and 10 tiles (4 + 6) in 3 and 7 ranges put range boundaries
    inside utterances and on their boundaries"""
    offs = shape[4]
    X, W0, H0 = problem(*shape)
    Wr, Hr, _, _ = reference(*shape, loss, 5, check_every=1)
    runs = [evc().learn_dictionary_deconv(X, W0, H0, loss=loss, layout="bin_major", iters=5, check_every=0, utt_offsets=offs,
                                          splits=S, info=True) for _ in range(2)]
    assert runs[0][2]["splits"] == S and runs[0][2]["n_iter"] == 5
    close64(runs[0][0], Wr, "W")
    close64(runs[0][1], Hr, "H")
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("shape", [(513, 16, 40, 3, None), (1056, 16, 24, 2, None)], ids=geo_id)
def test_dict_only(shape, loss):
    import torch
    M, R, T, L, offs = shape
    X, W0, H0 = problem(*shape)
    Wr, Hr, n_ref, tr = reference(*shape, loss, 5, check_every=1, update="dict")
    assert np.array_equal(Hr, H0)
    Hd = torch.from_numpy(H0).cuda()
    W, H, info = evc().learn_dictionary_deconv(torch.from_numpy(X).cuda(), torch.from_numpy(W0).cuda(), None, loss=loss,
                                               layout="bin_major", iters=5, check_every=1, update="dict", out_h=Hd, info=True)
    assert H.data_ptr() == Hd.data_ptr() and Hd.cpu().numpy().tobytes() == H0.tobytes()       # only read
    assert info["n_iter"] == 5
    close64(W.cpu().numpy(), Wr, "W")
    print("trace", info["err"], "restatement", tr)
    np.testing.assert_allclose(info["err"], tr, rtol=1e-9, atol=0)


@pytest.mark.parametrize("name", SK)
def test_one_tap_is_recorded_sklearn(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    loss = "kullback-leibler" if name.startswith("dictkl") else "frobenius"
    tol, K = float(d["tol"]), int(d["max_iter"])
    ce = 10 if tol > 0 else 0
    W, H, info = evc().learn_dictionary_deconv(d["X"], d["W0"][None], d["H0"], loss=loss, layout="bin_major", iters=K,
                                               check_every=ce, tol=tol, info=True)
    assert info["n_iter"] == int(d["n_iter"]) and (tol == 0 or info["n_iter"] == 60)
    close64(W[0], d["W"], "W against scikit-learn")
    close64(H, d["H"], "H against scikit-learn")
    W1, H1, i1 = evc().learn_dictionary(d["X"], d["W0"], d["H0"], layout="bin_major", iters=K, surface="sklearn", check_every=ce,
                                        tol=tol, info=True, loss=loss)
    assert i1["n_iter"] == info["n_iter"]
    close64(W[0], W1, "W against learn_dictionary")
    close64(H, H1, "H against learn_dictionary")


@pytest.mark.parametrize("loss", LOSSES)
def test_first_activation_half_is_bitwise_the_solve(loss):
    shape = GEOMETRY[0]
    offs = shape[4]
    X, W0, H0 = problem(*shape)
    _, H = evc().learn_dictionary_deconv(X, W0, H0, loss=loss, layout="bin_major", iters=1, check_every=0, utt_offsets=offs,
                                         l1_h=0.01, l2_h=0.02)
    Hs = evc().solve_activations_deconv(W0, X, H0, loss=loss, iters=1, check_every=0, utt_offsets=offs, l1=0.01, l2=0.02)
    assert H.tobytes() == Hs.tobytes()


@pytest.mark.parametrize("loss", LOSSES)
def test_stop_rule(loss):
    shape = GEOMETRY[0]
    offs = shape[4]
    K = 100
    X, W0, H0 = problem(*shape)
    _, _, _, free = reference(*shape, loss, K, check_every=10)
    ratios = (free[:-1] - free[1:]) / free[0]               # what the rule sees at the checks 1 .. 10
    c = 4                                                   # the stop falls at check 4, after 40 iterations
    tol = float(np.sqrt(ratios[c - 2] * ratios[c - 1]))
    assert ratios[:c - 1].min() > tol > ratios[c - 1], ratios
    Wr, Hr, n_ref, tr = reference(*shape, loss, K, check_every=10, tol=tol)
    margin = dr.stop_margin(tr, tol)
    print("tol %.3e; the nearest deciding ratio is %.3e of tol away from it" % (tol, margin))
    assert margin > 1e-6 and n_ref == 10 * c and 10 < n_ref < K
    W, H, info = evc().learn_dictionary_deconv(X, W0, H0, loss=loss, layout="bin_major", iters=K, check_every=10, tol=tol,
                                               utt_offsets=offs, info=True)
    assert info["n_iter"] == n_ref
    np.testing.assert_allclose(info["err"], tr, rtol=1e-9, atol=0)              # NaN after the stop on both sides
    assert np.isnan(info["err"][c + 1:]).all() and not np.isnan(info["err"][:c + 1]).any()
    close64(W, Wr, "W")
    close64(H, Hr, "H")


def frames(Ma, Mb, N, seed=5):
    rng = np.random.default_rng(seed)
    return rng.random((Ma, N)) + 1e-3, rng.random((Mb, N)) + 1e-3


@pytest.mark.parametrize("loss", LOSSES)
def test_compaction_with_one_tap_is_compact_dictionary(loss):
    A, B = frames(25, 25, 150)
    Wa, Wb, G, info = evc().compact_dictionary_deconv(A, B, [0, 150], 16, 1, iters=30, loss=loss)
    Wa1, Wb1, G1, info1 = evc().compact_dictionary(A, B, 16, iters=30, loss=loss)
    assert Wa.shape == (1, 25, 16) and info["stages"] == 1 and info["n_iter"] == info1["n_iter"] == 30
    close64(Wa[0], Wa1, "Wa")
    close64(Wb[0], Wb1, "Wb")
    close64(G, G1, "G")
    np.testing.assert_allclose(info["err"], info1["err"], rtol=1e-9, atol=0)


@pytest.mark.parametrize("loss", LOSSES)
def test_compaction_with_four_taps(loss):
    A, B = frames(25, 25, 150)
    offs = [0, 61, 150]
    Wa, Wb, G, info = evc().compact_dictionary_deconv(A, B, offs, 16, 4, iters=40, loss=loss)
    assert Wa.shape == (4, 25, 16) and Wb.shape == (4, 25, 16) and G.shape == (16, 150) and info["stages"] == 1
    print("err", info["err"])
    assert np.isfinite(info["err"]).all() and np.all(np.diff(info["err"]) <= 0) and info["err"][-1] < info["err"][0]
    Y, H = evc().convert_deconv(Wa, A[:, :61], Wb, loss=loss, iters=20)
    assert Y.shape == (25, 61) and np.isfinite(Y).all() and (Y >= 0).all() and H.shape == (16, 61)


@pytest.mark.parametrize("loss", LOSSES)
def test_compaction_in_two_stages(loss):
    """201 + 201 bins do not fit one factorisation: (Wa, G) on the source, then Wb under G"""
    e = evc()
    Ma = Mb = 201
    N, R, L, K = 60, 8, 3, 10
    A, B = frames(Ma, Mb, N)
    offs = [0, 25, 60]
    Wa, Wb, G, info = e.compact_dictionary_deconv(A, B, offs, R, L, iters=K, loss=loss)
    assert info["stages"] == 2 and Wa.shape == (L, Ma, R) and Wb.shape == (L, Mb, R)
    pick = np.arange(R) * N // R
    start = lambda F: np.maximum(e.multiframe_dictionary(F, offs, L)[:, :, pick], 1e-6)
    G0 = np.full((R, N), np.sqrt(A.mean() / R))
    Wa_r, G_r, _, tr_a = dlr.learn(start(A), A, G0, loss, K, offs, check_every=10)
    Wb_r, _, _, tr_b = dlr.learn(start(B), B, G_r, loss, K, offs, check_every=10, update="dict")
    close64(Wa, Wa_r, "Wa")
    close64(G, G_r, "G")
    close64(Wb, Wb_r, "Wb")
    np.testing.assert_allclose(info["err"], tr_a, rtol=1e-9, atol=0)
    np.testing.assert_allclose(info["err_b"], tr_b, rtol=1e-9, atol=0)


def test_taps_a_chunk_at_a_time():
    """256 bins x 2176 components x 16 taps: the slab pairs of all taps (16 x 8 912 896 bytes) exceed the 128 MiB cap, so the
    dictionary half runs one range and the taps in two chunks, 15 and then 1, each contracted and applied on its own"""
    import torch
    from exemplars_vc_amd import _lib
    M, R, T, L = 256, 2176, 20, 16
    assert _lib.lib().evc_deconv_learn_splits(M, R, T, 1, L) == 1
    rng = np.random.default_rng(7)
    X, W0, H0 = rng.random((M, T)) + 1e-3, rng.random((L, M, R)) + 0.1, rng.random((R, T)) + 0.1
    Wr, Hr, _, _ = dlr.learn(W0, X, H0, "frobenius", 2)
    Wd = torch.from_numpy(W0).cuda()
    _, H, info = evc().learn_dictionary_deconv(torch.from_numpy(X).cuda(), None, H0, layout="bin_major", iters=2, check_every=0,
                                               out_w=Wd, info=True)
    assert info["n_iter"] == 2 and info["splits"] == 1
    close64(Wd.cpu().numpy(), Wr, "W")
    close64(H.cpu().numpy(), Hr, "H")


def test_make_dict_compact_hook():
    """compat.make_dict.aligned_dictionary(taps=L, compact=R) is compact_dictionary_deconv (frame-major) of the aligned frames,
    which is the bin-major compaction transposed, and convert_deconv runs on the result"""
    import torch
    from exemplars_vc_amd.compat import make_dict
    e = evc()
    rng = np.random.default_rng(11)
    la, lb, order, L, R = [40, 31, 55], [37, 35, 50], 13, 3, 8
    dtw_a = [rng.standard_normal((order, n)) for n in la]
    dtw_b = [rng.standard_normal((order, n)) for n in lb]
    src = [{"sp": rng.random((n, 33)) + 0.1} for n in la]
    tar = [{"sp": rng.random((n, 40)) + 0.1} for n in lb]
    A, B, rows = e.dtw_dictionary([a.T for a in dtw_a], [b.T for b in dtw_b], [f["sp"] for f in src], [f["sp"] for f in tar])
    (Wa, Wb), rows2 = make_dict.aligned_dictionary(dtw_a, dtw_b, src, tar, use_stft=False, key="sp", taps=L, compact=R)
    assert isinstance(Wa, torch.Tensor) and not Wa.is_cpu and list(rows2) == list(rows)
    assert tuple(Wa.shape) == (L, R, 33) and tuple(Wb.shape) == (L, R, 40)
    Wa2, Wb2, G2, info = e.compact_dictionary_deconv(A.cpu().numpy().T, B.cpu().numpy().T, rows, R, L)
    assert info["stages"] == 1 and np.all(np.diff(info["err"]) <= 0)
    assert Wa.cpu().numpy().transpose(0, 2, 1).tobytes() == np.ascontiguousarray(Wa2).tobytes()
    assert Wb.cpu().numpy().transpose(0, 2, 1).tobytes() == np.ascontiguousarray(Wb2).tobytes()
    X = rng.random((20, 33)) + 0.1
    Y, H = e.convert_deconv(Wa, X, Wb, layout="frame_major", iters=10)
    assert Y.shape == (20, 40) and H.shape == (20, R) and np.isfinite(Y).all()
    with pytest.raises(ValueError, match="compact needs taps"):
        make_dict.aligned_dictionary(dtw_a, dtw_b, src, tar, use_stft=False, key="sp", compact=R)
