"""Feature extraction of the scripts on the GPU: the STFT of the conversion script (front half) and the
MFCC alignment features of the dictionary build (01_make_dict_parallel.py:86-178).

Mirrors the STFT branch of extract_feature_for_conversion() (04_align_n_nmf.py:419-429) and of
_get_conversion_data() (03_a_b_r_parallel.py:101-104) from the decoded samples on: reading the wav file
(librosa.load) stays with the caller.  librosa is absent in this environment, so the window / padding
conventions follow its published algorithm (restated for the tests as `librosa_stft`): parity with librosa
itself is unpinned.
"""
from __future__ import annotations

import numpy as np

from ..solver import mfcc as _mfcc, mfcc_batch, stft

FRAME_LENGTH = 400      # 04_align_n_nmf.py:46
HOP_LENGTH = 80         # 04_align_n_nmf.py:47


def stft_features(samples, *, n_fft=FRAME_LENGTH, hop_length=HOP_LENGTH, dtype=np.complex64, device=None):
    """-> {'stft': (T, 201) complex, 'real': ..., 'imag': ...}: `feat_stft.T` and its parts, as
    extract_feature_for_conversion() returns them.  dtype=np.complex64 is librosa's default output type
    (so 'real' is float32 and the solve downstream runs in float32, as it does in the reference);
    dtype=np.complex128 keeps the float64 the transform is computed in."""
    re, im = stft(np.asarray(samples, dtype=np.float64), n_fft, hop_length, center=True, device=device)
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.complex64), np.dtype(np.complex128)):
        raise ValueError("dtype must be complex64 or complex128")
    z = (re + 1j * im).astype(dtype)
    return {"stft": z, "real": np.real(z), "imag": np.imag(z)}


def conversion_features(samples, fs, *, n_fft=FRAME_LENGTH, hop_length=HOP_LENGTH, dtype=np.complex64, device=None):
    """The per-file dict of `<spk>_feat_stft.pkl`: {'stft': (T, 201) complex, 'fs': fs}
    (03_a_b_r_parallel.py:101-104)."""
    return {"stft": stft_features(samples, n_fft=n_fft, hop_length=hop_length, dtype=dtype, device=device)["stft"],
            "fs": fs}


def mfcc(y, sr=22050, n_mfcc=20, n_fft=2048, hop_length=512, **kw):
    """librosa.feature.mfcc(y, sr, n_mfcc=..., n_fft=..., hop_length=...) with librosa's own defaults and orientation:
    (n_mfcc, T).  Further keywords: n_mels, fmin, fmax, top_db, center, device.  librosa's published algorithm restated
    (parity with the package is unpinned)."""
    c = _mfcc(y, sr=sr, n_fft=n_fft, hop_length=hop_length, n_mfcc=n_mfcc, **kw)
    return c.T


def _extract_features(audiodatum, speaker, sr=16000, feat='mcep'):
    """_extract_features() of 01_make_dict_parallel.py:86-139 for one utterance: feat='mfcc' (what the script's live
    call passes, :358-359) -> (20, T) MFCCs at n_fft = frame_length = 400, hop_length = 80.  feat='mcep', the
    signature's default, needs pysptk's iterative mel-cepstral analysis, which is absent and out of scope."""
    f = str(feat).lower()
    if f == 'mfcc':
        return mfcc(audiodatum, sr=sr, n_fft=FRAME_LENGTH, hop_length=HOP_LENGTH)
    if f in ('mcep', 'mcc'):
        raise NotImplementedError("feat='mcep' needs pysptk.mcep, which this package does not restate; use feat='mfcc'")
    raise ValueError(f"{feat} feature is not supported")


def extract_features(audiodata, speaker, sr=16000, feat='mcep'):
    """extract_features() of 01_make_dict_parallel.py:142-178: the features of all of a speaker's utterances, here in
    ONE native call instead of a process pool, and without the pickle the script leaves behind.
    Returns (list of (20, T_u) arrays, feat)."""
    f = str(feat).lower()
    if f != 'mfcc':
        return [_extract_features(a, speaker, sr, feat) for a in audiodata], feat
    return [c.T for c in mfcc_batch(list(audiodata), sr=sr, n_fft=FRAME_LENGTH, hop_length=HOP_LENGTH)], feat
