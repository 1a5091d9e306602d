"""numpy restatement of librosa.feature.mfcc(y, sr, n_fft, hop_length) with librosa's defaults, as
01_make_dict_parallel.py:96-104 calls it - the yardstick of evc_mfcc.

librosa is absent here: this restates its published chain and is NOT pinned to the package.
  stft       reflect-padded centred frames, periodic Hann window, rfft (`form="rfft"`; `form="dft"` forms the same
             transform as a product with the windowed DFT matrix, the order the GPU sums in)
  mel        Slaney scale, Slaney area normalisation (librosa.filters.mel, htk=False, norm='slaney')
  power_to_db   10 log10(max(amin, S)) with ref = 1, then max(., max over the utterance - top_db)
  dct        scipy.fftpack.dct(type=2, norm='ortho') over the mel axis, restated as its defining sum
"""
import numpy as np

F_SP = 200.0 / 3
MIN_LOG_HZ = 1000.0
MIN_LOG_MEL = 15.0          # 1000 / (200/3); the quotient itself rounds to 14.999999999999998
LOGSTEP = np.log(6.4) / 27.0


def hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(f < MIN_LOG_HZ, f / F_SP, MIN_LOG_MEL + np.log(f / MIN_LOG_HZ) / LOGSTEP)


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m < MIN_LOG_MEL, F_SP * m, MIN_LOG_HZ * np.exp(LOGSTEP * (m - MIN_LOG_MEL)))


def mel_filterbank(sr, n_fft, n_mels=128, fmin=0.0, fmax=None):
    """(n_mels, 1 + n_fft/2) weights."""
    fmax = sr / 2.0 if fmax is None else float(fmax)
    nb = n_fft // 2 + 1
    fftfreqs = np.linspace(0.0, sr / 2.0, nb)
    mel_f = mel_to_hz(np.linspace(float(hz_to_mel(fmin)), float(hz_to_mel(fmax)), n_mels + 2))
    fdiff = np.diff(mel_f)
    w = np.zeros((n_mels, nb))
    for i in range(n_mels):
        lower = (fftfreqs - mel_f[i]) / fdiff[i]
        upper = (mel_f[i + 2] - fftfreqs) / fdiff[i + 1]
        w[i] = np.maximum(0.0, np.minimum(lower, upper))
    return w * (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]


def stft(y, n_fft, hop_length, center=True, form="rfft"):
    """(n_frames, 1 + n_fft/2) complex128, rows are time slices."""
    y = np.asarray(y, dtype=np.float64)
    nb = n_fft // 2 + 1
    if y.shape[0] == 0:
        return np.zeros((0, nb), dtype=np.complex128)
    if center:
        y = np.pad(y, n_fft // 2, mode="reflect")
    if y.shape[0] < n_fft:
        return np.zeros((0, nb), dtype=np.complex128)
    n_frames = 1 + (y.shape[0] - n_fft) // hop_length
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)
    idx = np.arange(n_fft)[None, :] + hop_length * np.arange(n_frames)[:, None]
    frames = y[idx]
    if form == "rfft":
        return np.fft.rfft(frames * win[None, :], axis=1)
    if form != "dft":
        raise ValueError(form)
    ang = 2.0 * np.pi * ((np.arange(n_fft)[:, None] * np.arange(nb)[None, :]) % n_fft) / n_fft
    return frames @ (win[:, None] * np.cos(ang)) - 1j * (frames @ (win[:, None] * np.sin(ang)))


def power_to_db(S, amin=1e-10, top_db=80.0):
    """The maximum is taken over the whole array: one utterance."""
    db = 10.0 * np.log10(np.maximum(amin, S))
    if top_db is not None and top_db >= 0 and db.size:
        db = np.maximum(db, db.max() - top_db)
    return db


def dct_basis(n_mfcc, n_mels):
    q = np.arange(n_mfcc)[:, None]
    n = np.arange(n_mels)[None, :]
    s = np.where(q == 0, np.sqrt(1.0 / n_mels), np.sqrt(2.0 / n_mels))
    return s * np.cos(np.pi * q * (2 * n + 1) / (2.0 * n_mels))


def dct_ortho(x, n_out):
    """DCT-II, norm='ortho', over the last axis; the first n_out coefficients."""
    return np.asarray(x, dtype=np.float64) @ dct_basis(n_out, np.shape(x)[-1]).T


def mel_db(y, sr=16000, n_fft=400, hop_length=80, n_mels=128, fmin=0.0, fmax=None, amin=1e-10, top_db=80.0,
           center=True, form="rfft"):
    """(n_frames, n_mels) decibels after the clamp, and before it."""
    S = stft(y, n_fft, hop_length, center, form)
    P = S.real ** 2 + S.imag ** 2
    mel = P @ mel_filterbank(sr, n_fft, n_mels, fmin, fmax).T
    raw = 10.0 * np.log10(np.maximum(amin, mel))
    return power_to_db(mel, amin, top_db), raw


def mfcc(y, sr=16000, n_fft=400, hop_length=80, n_mfcc=20, n_mels=128, fmin=0.0, fmax=None, amin=1e-10, top_db=80.0,
         center=True, form="rfft"):
    """(n_frames, n_mfcc): frames as rows - the transpose of what librosa returns."""
    db, _ = mel_db(y, sr, n_fft, hop_length, n_mels, fmin, fmax, amin, top_db, center, form)
    return dct_ortho(db, n_mfcc)
