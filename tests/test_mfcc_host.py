"""evc_mfcc without a device: the numpy restatement the GPU tests compare against (tests/mfcc_restatement.py; NOT pinned
to librosa, which is absent here) checks itself, and the C ABI rejects bad arguments before any device work."""
import ctypes as C

import numpy as np
import pytest

import mfcc_restatement as mr


def test_slaney_scale():
    assert float(mr.hz_to_mel(1000.0)) == 15.0
    f = np.array([0.0, 1.0, 133.3, 999.9, 1000.0, 1000.1, 4000.0, 8000.0, 11025.0])
    np.testing.assert_allclose(mr.mel_to_hz(mr.hz_to_mel(f)), f, rtol=1e-13, atol=1e-12)
    assert np.all(np.diff(mr.hz_to_mel(np.linspace(0, 8000, 500))) > 0)


def test_filterbank_is_sparse_at_the_script_sizes():
    w = mr.mel_filterbank(16000, 400, 128)
    assert w.shape == (128, 201) and (w >= 0).all()
    nz = w > 0
    assert int(nz.sum()) == 394
    per_filter = nz.sum(axis=1)
    assert per_filter.min() >= 1 and per_filter.max() <= 9
    assert nz.sum(axis=0).max() <= 2
    for row in nz:                                      # a filter's support is contiguous: the row-compressed table
        k = np.flatnonzero(row)
        assert k[-1] - k[0] + 1 == len(k)


def test_dct_matches_scipy():
    from scipy.fft import dct
    rng = np.random.default_rng(0)
    x = rng.standard_normal((7, 128)) * 50
    np.testing.assert_allclose(mr.dct_ortho(x, 20), dct(x, type=2, norm="ortho", axis=-1)[:, :20], rtol=0, atol=1e-12)
    x = rng.standard_normal((3, 40))
    np.testing.assert_allclose(mr.dct_ortho(x, 40), dct(x, type=2, norm="ortho", axis=-1), rtol=0, atol=1e-12)


def test_clamp_uses_the_utterance_maximum_and_amin_floors_silence():
    rng = np.random.default_rng(1)
    y = np.concatenate([1e-7 * rng.standard_normal(800), rng.standard_normal(800)])
    db, raw = mr.mel_db(y)
    assert db.min() == pytest.approx(raw.max() - 80.0, abs=0) and (raw < raw.max() - 80.0).mean() > 0.3
    # the quiet half alone is not clamped to the loud half's maximum
    db_q, raw_q = mr.mel_db(y[:800])
    assert db_q.min() >= raw_q.max() - 80.0 and db_q.max() < db.min()
    c = mr.mfcc(np.zeros(800))
    assert c.shape == (11, 20)
    np.testing.assert_allclose(c[:, 0], -100.0 * np.sqrt(128), rtol=0, atol=1e-9)
    np.testing.assert_allclose(c[:, 1:], 0.0, rtol=0, atol=1e-9)


def test_dft_matrix_form_agrees_with_rfft():
    rng = np.random.default_rng(2)
    y = rng.standard_normal(3000)
    a, b = mr.mfcc(y), mr.mfcc(y, form="dft")
    assert np.abs(a - b).max() < 1e-9


def _load():
    from exemplars_vc_amd import _lib
    return _lib, _lib.lib()


def _opts(_lib, **kw):
    o = _lib.MfccOpts()
    o.struct_bytes = C.sizeof(_lib.MfccOpts)
    o.sr, o.fft_size, o.hop, o.n_mels, o.n_mfcc, o.center = 16000, 400, 80, 128, 20, 1
    o.fmin, o.fmax, o.amin, o.top_db = 0.0, 0.0, 1e-10, 80.0
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _offsets(*v):
    return (C.c_long * len(v))(*v)


def test_struct_mirror_matches_the_header():
    import os
    import re
    from conftest import ROOT
    _lib, _ = _load()
    hdr = open(os.path.join(ROOT, "include", "evc.h")).read()
    body = hdr[hdr.index("typedef struct evc_mfcc_opts {"):hdr.index("} evc_mfcc_opts;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(?:int|double)\s+([a-z_0-9]+);", body) == [f[0] for f in _lib.MfccOpts._fields_]
    assert C.sizeof(_lib.MfccOpts) == 64
    m = re.search(r"EVC_MFCC_MAX_MELS = (\d+), EVC_MFCC_MAX_FFT = (\d+)", hdr)
    assert (int(m.group(1)), int(m.group(2))) == (_lib.MFCC_MAX_MELS, _lib.MFCC_MAX_FFT)


def test_workspace_bytes():
    _lib, L = _load()
    o = _opts(_lib)
    small = L.evc_mfcc_workspace_bytes(_offsets(0, 8000), 1, C.byref(o))
    big = L.evc_mfcc_workspace_bytes(_offsets(0, 8000, 80000), 2, C.byref(o))
    huge = L.evc_mfcc_workspace_bytes(_offsets(0, 8000, 8000000), 2, C.byref(o))
    more = L.evc_mfcc_workspace_bytes(_offsets(0, 8000, 16000000), 2, C.byref(o))
    assert 0 < small < big < huge < more
    # past one chunk of rows only the padded samples and the decibel values grow with the batch: 8 + 8 * 128 / 80 bytes
    # per sample and a little rounding, not the 9 * 448 * 8 / 80 of a whole-batch S with its split-K slabs
    assert (more - huge) / 8000000 < 8 + 8 * 128 / 80 + 0.5
    for bad in (dict(struct_bytes=8), dict(fft_size=401), dict(hop=0), dict(n_mfcc=129), dict(amin=0.0),
                dict(fmin=9000.0), dict(n_mels=257, n_mfcc=20)):
        assert L.evc_mfcc_workspace_bytes(_offsets(0, 8000), 1, C.byref(_opts(_lib, **bad))) == 0, bad
    assert L.evc_mfcc_workspace_bytes(_offsets(0, 8000, 7000), 2, C.byref(o)) == 0
    assert L.evc_mfcc_workspace_bytes(_offsets(0, 8000), 1, None) == 0


def test_bad_arguments_are_rejected_before_any_device_work():
    _lib, L = _load()
    one = C.c_void_p(8)

    def call(o, off=(0, 8000), n_utt=None, ldc=20, re=None, ldre=201):
        n = len(off) - 1 if n_utt is None else n_utt
        return L.evc_mfcc(one, _offsets(*off), n, C.byref(o), one, ldc, re, ldre, None, 201, one, 1 << 40, None)

    bad = [dict(struct_bytes=8), dict(fft_size=401), dict(fft_size=0), dict(hop=0), dict(n_mfcc=0), dict(n_mfcc=129),
           dict(n_mels=0), dict(fmin=-1.0), dict(fmin=4000.0, fmax=4000.0), dict(fmin=5000.0, fmax=4000.0),
           dict(fmax=8000.5), dict(fmin=8000.0), dict(amin=0.0), dict(amin=-1.0), dict(sr=0), dict(top_db=float("nan"))]
    for kw in bad:
        assert call(_opts(_lib, **kw)) == -1, kw
    o = _opts(_lib)
    assert call(o, off=(0, 8000, 7999)) == -1                  # descending offsets
    assert call(o, off=(-1, 8000)) == -1
    assert call(o, ldc=19) == -1
    assert call(o, re=one, ldre=200) == -1
    assert call(o, n_utt=-1) == -1
    assert L.evc_mfcc(one, _offsets(0, 8000), 1, None, one, 20, None, 0, None, 0, one, 1 << 40, None) == -1
    assert L.evc_mfcc(None, _offsets(0, 8000), 1, C.byref(o), one, 20, None, 0, None, 0, one, 1 << 40, None) == -1
    assert call(_opts(_lib, n_mels=257)) == -3
    assert call(_opts(_lib, n_mels=256, n_mfcc=256, fft_size=8194)) == -3
    assert call(_opts(_lib, n_mels=257, n_mfcc=300)) == -1     # an invalid argument stays one beside an unsupported size
    # nothing to do is not an error, and nothing is launched: no utterance, no samples, no frames
    assert call(o, n_utt=0) == 0
    assert L.evc_mfcc(None, None, 0, C.byref(o), None, 20, None, 0, None, 0, None, 0, None) == 0
    assert call(o, off=(5, 5, 5)) == 0
    assert call(_opts(_lib, center=0), off=(0, 399)) == 0
    # a workspace that is too small
    assert L.evc_mfcc(one, _offsets(0, 8000), 1, C.byref(o), one, 20, None, 0, None, 0, one, 1024, None) == -2
