"""evc_mfcc on the GPU against the numpy restatement of librosa.feature.mfcc (tests/mfcc_restatement.py, rfft form; librosa
is absent, parity with the package is UNPINNED).  float64.  Tolerance: atol 1e-9, rtol 0 on coefficients of magnitude up
to ~1100 - 20 x the 5e-11 measured between two CPU summation orders of the STFT (rfft against a DFT-matrix product); the
GPU's split-K contraction is a third order.  Every test prints the deviation it saw before it asserts (largest seen on an
MI355X over all cases: 3.3e-12)."""
import functools
import os
import sys

import numpy as np
import pytest

import exemplars_vc_amd as evc
from conftest import GOLDEN, load_golden
from exemplars_vc_amd.compat import features, make_dict
from oracle import evc_oracle as o

import mfcc_restatement as mr

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

ATOL = 1e-9


def _close(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    dev = float(np.abs(got - want).max()) if want.size else 0.0
    print(f"{what}: max |deviation| {dev:.3e} (max |value| {float(np.abs(want).max()) if want.size else 0.0:.1f})")
    assert dev <= ATOL, (what, dev)
    return dev


@functools.lru_cache(maxsize=None)
def _batch_signals():
    rng = np.random.default_rng(20)
    loud = np.concatenate([1e-7 * rng.standard_normal(800), rng.standard_normal(800)])
    return (rng.standard_normal(1000), 0.3 * rng.standard_normal(90), loud, 1e-3 * loud)


@functools.lru_cache(maxsize=None)
def _batch_reference():
    return tuple(mr.mfcc(y) for y in _batch_signals())


def test_batch_of_four_matches_the_restatement_and_the_single_calls():
    sigs = _batch_signals()
    _, raw = mr.mel_db(sigs[2])
    assert (raw < raw.max() - 80.0).mean() > 0.3             # the clamp bites in the quiet-then-loud utterance
    got = evc.mfcc_batch(list(sigs))
    assert [g.shape for g in got] == [(13, 20), (2, 20), (21, 20), (21, 20)]
    for u, (g, w) in enumerate(zip(got, _batch_reference())):
        _close(g, w, f"batch utterance {u}")
    # utterance 3 is utterance 2 at 1e-3 of its level: with the clamp's maximum taken over the batch instead of per
    # utterance its quiet half would sit 60 dB too high (the restatement differs by more than 100 in c0 there)
    _, raw3 = mr.mel_db(sigs[3])
    wrong = mr.dct_ortho(np.maximum(raw3, mr.mel_db(sigs[2])[1].max() - 80.0), 20)
    assert np.abs(wrong - _batch_reference()[3]).max() > 100.0
    for u, y in enumerate(sigs):
        single = evc.mfcc(y)
        _close(single, _batch_reference()[u], f"single call {u}")
        _close(single, got[u], f"single against batch {u}")


@pytest.mark.parametrize("kw", [
    dict(sr=22050, n_fft=512, hop_length=128, n_mels=40, n_mfcc=13, fmin=50.0, fmax=8000.0),      # wide filters, fmin > 0
    dict(n_mels=20, n_mfcc=20),
    dict(n_mels=64, n_mfcc=40),                               # more coefficients than one LDS chunk of the basis (32)
    dict(center=False),
    dict(top_db=-1.0),                                        # no clamp
    dict(sr=22050, n_fft=2048, hop_length=512),               # librosa's own defaults
], ids=["wide-filters", "nmels20", "nmfcc40", "uncentred", "no-clamp", "librosa-defaults"])
def test_other_parameters(kw):
    rng = np.random.default_rng(5)
    sigs = [rng.standard_normal(3000), np.concatenate([1e-6 * rng.standard_normal(2500), rng.standard_normal(2100)]),
            rng.standard_normal(700)]
    rkw = dict(kw)
    if rkw.get("top_db", 0) < 0:
        rkw["top_db"] = None
    got = evc.mfcc_batch(sigs, **kw)
    for u, y in enumerate(sigs):
        _close(got[u], mr.mfcc(y, **rkw), f"{kw} utterance {u}")
    _close(evc.mfcc(sigs[1], **kw), mr.mfcc(sigs[1], **rkw), f"{kw} single")


def test_silence_has_the_closed_form():
    c = evc.mfcc(np.zeros(800))
    assert c.shape == (11, 20)
    _close(c[:, 0], np.full(11, -100.0 * np.sqrt(128)), "silence c0")
    _close(c[:, 1:], np.zeros((11, 19)), "silence c1..")
    # an utterance without samples has no frames, and does not disturb its neighbours
    got = evc.mfcc_batch([np.zeros(0), np.zeros(800), np.zeros(0)])
    assert [g.shape for g in got] == [(0, 20), (11, 20), (0, 20)]
    _close(got[1], c, "silence between two empty utterances")
    assert evc.mfcc_batch([]) == [] and evc.mfcc(np.zeros(0)).shape == (0, 20)
    with pytest.raises(ValueError):
        evc.mfcc(np.array([0.0, np.nan, 1.0]))
    with pytest.raises(ValueError):
        evc.mfcc(np.zeros(100), n_fft=401)


def test_stft_outputs_match_the_stft_front_end():
    sigs = _batch_signals()
    mf, res, ims = evc.mfcc_batch(list(sigs), want_stft=True)
    for u, y in enumerate(sigs):
        re, im = evc.stft(y, 400, 80)
        assert res[u].shape == re.shape and ims[u].shape == im.shape
        scale = max(float(np.abs(re).max()), float(np.abs(im).max()))
        dev = max(float(np.abs(res[u] - re).max()), float(np.abs(ims[u] - im).max()))
        print(f"stft utterance {u}: deviation {dev:.3e}, bound {1e-11 * scale:.3e}")
        assert dev <= 1e-11 * scale
        _close(mf[u], _batch_reference()[u], f"mfcc with want_stft, utterance {u}")


def test_real_speech_fixture():
    g = load_golden(os.path.join(GOLDEN, "mfcc_audio.npz"))       # generated by the restatement, not pinned to librosa
    ys = [g["pcm_src"].astype(np.float64) / 32768.0, g["pcm_tar"].astype(np.float64) / 32768.0]
    assert g["clamped_src"] > 0.3 and g["clamped_tar"] > 0.4 and g["floor_src"] > 0 and g["floor_tar"] > 0
    got = evc.mfcc_batch(ys)
    _close(got[0], g["mfcc_src"], "speech, source speaker")
    _close(got[1], g["mfcc_tar"], "speech, target speaker")
    (pa, pb), = evc.dtw_align([got[0]], [got[1]])
    assert np.array_equal(pa, g["path_a"]) and np.array_equal(pb, g["path_b"])


@functools.lru_cache(maxsize=None)
def _voice_pairs():
    import pipeline_synthetic as ps
    src, tar = ps.training_pairs(4, 0.5)
    ref = [o.dtw_align(mr.mfcc(a), mr.mfcc(b)) for a, b in zip(src, tar)]
    paths = [(np.asarray(p), np.asarray(q)) for _, (p, q) in ref]
    return src, tar, paths, np.array([acc[-1, -1] for acc, _ in ref])


def _same_paths(got, want):
    assert len(got) == len(want)
    for (ga, gb), (wa, wb) in zip(got, want):
        assert np.array_equal(ga, wa) and np.array_equal(gb, wb)


def test_dtw_on_the_gpu_features_gives_the_oracle_paths():
    src, tar, want, cost = _voice_pairs()
    fa, fb = evc.mfcc_batch(src), evc.mfcc_batch(tar)
    got, tot = evc.dtw_align(fa, fb, want_cost=True)
    _same_paths(got, want)
    print("accumulated cost, relative deviation:", np.abs(tot - cost) / cost)
    np.testing.assert_allclose(tot, cost, rtol=1e-9, atol=0)


def test_dictionary_from_wavs_matches_the_step_by_step_route():
    src, tar, want, _ = _voice_pairs()
    pd, rows = make_dict.dictionary_from_wavs(src, tar)
    A, B, rows_d = make_dict.aligned_frames_from_wavs(src, tar)
    assert not A.is_cpu and A.dtype == B.dtype and str(A.dtype) == "torch.float32"
    # step by step through the compat surfaces (host lists between the stages)
    fa, feat = features.extract_features(src, "SF1", feat="mfcc")
    fb, _ = features.extract_features(tar, "TF1", feat="mfcc")
    assert feat == "mfcc" and fa[0].shape == (20, 101)
    paths, _, _ = make_dict.dtw_alignment(fa, fb)
    _same_paths(paths, want)
    sf = [features.conversion_features(w, 16000) for w in src]
    tf = [features.conversion_features(w, 16000) for w in tar]
    pd2, rows2 = make_dict.aligned_dictionary(fa, fb, sf, tf)
    assert np.array_equal(rows, rows2) and np.array_equal(rows_d.cpu().numpy(), rows2)
    assert (pd.N, pd.M, pd.Mb, pd.dcode) == (pd2.N, pd2.M, pd2.Mb, pd2.dcode) and pd.N == int(rows[-1]) == A.shape[0]
    A2 = np.abs(np.concatenate([f["stft"].real[p] for f, (p, _) in zip(sf, paths)]))
    B2 = np.abs(np.concatenate([f["stft"].real[q] for f, (_, q) in zip(tf, paths)]))
    # the complex64 bound of test_gpu_stft.py: the batch and the single STFT may sum in different orders
    for got_, want_, what in ((A.cpu().numpy(), A2, "A"), (B.cpu().numpy(), B2, "B")):
        dev = float(np.abs(got_ - want_).max())
        print(f"{what}: deviation {dev:.3e}, bound {2e-6 * float(want_.max()):.3e}")
        assert got_.shape == want_.shape and dev <= 2e-6 * float(want_.max())


def test_example_composes_with_mfcc_alignment():
    import pipeline_synthetic as ps
    out = ps.main(n_pairs=4, seconds=0.5, gl_iters=10, verbose=False, dtw_features="mfcc")
    T = 1 + int(0.5 * ps.FS) // 80
    assert out["converted"].shape == (T, 201) and out["H"].shape == (out["N"], T)
    assert out["H"].dtype == np.float32
    assert np.isfinite(out["converted"]).all() and (out["converted"] >= 0).all()
    assert out["wav"].shape == (T * 80 + 400,) and np.isfinite(out["wav"]).all()
    _same_paths(out["paths"], _voice_pairs()[2])
    assert out["N"] == sum(len(p) for p, _ in out["paths"])


def test_repeatable_and_device_tensors_stay_on_the_device():
    import torch
    sigs = _batch_signals()
    a = evc.mfcc_batch(list(sigs), want_stft=True)
    b = evc.mfcc_batch(list(sigs), want_stft=True)
    for x, y in zip(a, b):
        for p, q in zip(x, y):
            assert np.array_equal(p, q)                        # bitwise
    dev = [torch.from_numpy(y).cuda() for y in sigs]
    c = evc.mfcc_batch(dev)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 for t in c)
    for t, want in zip(c, a[0]):
        assert np.array_equal(t.cpu().numpy(), want)
    single = evc.mfcc(dev[0], want_stft=True)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in single)


def test_an_utterance_across_two_row_chunks():
    """8192 rows of S per contraction: 8751 frames span two chunks (the first unsplit, the short second one split over k),
    with a short utterance in front so that the long one starts off a chunk boundary."""
    rng = np.random.default_rng(9)
    t = np.arange(700000) / 16000.0
    long_ = (0.5 + 0.5 * np.sin(2 * np.pi * 0.37 * t)) ** 4 * np.sin(2 * np.pi * 440 * t) + 1e-4 * rng.standard_normal(t.size)
    short = rng.standard_normal(500)
    got, res, _ = evc.mfcc_batch([short, long_, short], want_stft=True)
    assert got[1].shape == (8751, 20)
    _close(got[1], mr.mfcc(long_), "long utterance")
    _close(got[0], mr.mfcc(short), "short utterance in front")
    _close(got[2], got[0], "short utterance behind")
    S = mr.stft(long_, 400, 80)
    assert np.abs(res[1] - S.real).max() <= 1e-11 * np.abs(S).max()


def test_compat_mfcc_has_librosas_orientation_and_defaults():
    rng = np.random.default_rng(3)
    y = rng.standard_normal(6000)
    c = features.mfcc(y)
    assert c.shape == (20, 1 + 6000 // 512)
    _close(c.T, mr.mfcc(y, sr=22050, n_fft=2048, hop_length=512), "compat.features.mfcc defaults")
    c = features._extract_features(y, "SF1", feat="MFCC")
    _close(c.T, mr.mfcc(y), "_extract_features")
    with pytest.raises(NotImplementedError, match="pysptk"):
        features._extract_features(y, "SF1")
    with pytest.raises(NotImplementedError, match="pysptk"):
        features.extract_features([y], "SF1")
