"""Golden vectors of scikit-learn's coordinate-descent solve with a fixed dictionary: the call of the reference's
04_align_n_nmf_pytorch.py:205-208,

    non_negative_factorization(X=X, H=W, init="custom", update_H=False, n_components=W.shape[0],
                               beta_loss="frobenius", solver='cd', tol=tol, max_iter=200)

run by the installed scikit-learn (1.7.2) on inputs of the existing fixtures, and on seeded synthetic inputs at
the lane geometries of k_cd_sweep.  Writes tests/golden/cdnmf_*.npz with
X_rows, W_rows, H (N x T, float64 unless noted), n_iter, tol, max_iter, alpha_W, l1_ratio, dtype and `violation`, the
per-iteration violation trace (recorded by wrapping _update_coordinate_descent here, nowhere else).  float32 cases
also store H_f64 / n_iter_f64 (the same call in float64).  The prefix `cdnmf_` keeps these out of the globs of the
multiplicative-update tests.

    python tools/make_golden_cd.py [--check]     (--check: recompute and compare instead of writing)
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def run_sklearn(X_rows, W_rows, tol, max_iter=200, alpha_W=0.0, l1_ratio=0.0):
    import sklearn.decomposition._nmf as nmf
    trace = []
    orig = nmf._update_coordinate_descent

    def wrapped(*a, **k):
        v = orig(*a, **k)
        trace.append(float(v))
        return v

    nmf._update_coordinate_descent = wrapped
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            W, _, n_iter = nmf.non_negative_factorization(
                X=X_rows, H=W_rows, init="custom", update_H=False, n_components=W_rows.shape[0],
                beta_loss="frobenius", solver="cd", tol=tol, max_iter=max_iter, alpha_W=alpha_W, l1_ratio=l1_ratio)
    finally:
        nmf._update_coordinate_descent = orig
    return W.T, int(n_iter), np.array(trace)


def _load(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    return np.array(d["X_rows"], dtype=np.float64), np.array(d["W_rows"], dtype=np.float64)


def _synth(M, N, T, seed):
    """seeded synthetic inputs: squared uniform exemplars with rows 1, 8, 15 ... zero, 30 % active activations,
    1/20 noise"""
    rng = np.random.default_rng(seed)
    W = rng.random((N, M)) ** 2 + 0.05
    W[1::7] = 0.0
    X = (rng.random((T, N)) * (rng.random((T, N)) < 0.3)) @ W + 0.05 * rng.random((T, M))
    return X, W


def cases():
    """name -> (X_rows, W_rows, tol, alpha_W, l1_ratio, dtype)"""
    c = {}
    X, W = _load("sklearn_m25_n64_t32_k50")
    c["cdnmf_m25_n64_t32"] = (X, W, 1e-4, 0.0, 0.0, np.float64)                 # runs to 200: ConvergenceWarning
    c["cdnmf_m25_n64_t32_l1"] = (X, W, 1e-4, 0.05, 1.0, np.float64)             # L1 only
    c["cdnmf_m25_n64_t32_l1l2"] = (X, W, 1e-4, 0.05, 0.5, np.float64)           # L1 + L2
    c["cdnmf_m25_n64_t32_l2"] = (X, W, 1e-4, 0.05, 0.0, np.float64)             # L2 only
    X, W = _load("sklearn_m1_n48_t37_tol")
    c["cdnmf_m1_n48_t37"] = (X, W, 1e-4, 0.0, 0.0, np.float64)                  # f0-like: zero exemplar rows
    X, W = _load("sklearn_audio_stft")
    c["cdnmf_m201_audio"] = (X, W, 1e-4, 0.0, 0.0, np.float64)                  # real-audio STFT magnitudes
    X, W = _load("sklearn_m201_n128_t40_tol")
    c["cdnmf_m201_n128_t40"] = (X, W, 1e-4, 0.0, 0.0, np.float64)               # early stop (163)
    c["cdnmf_m201_n128_t40_f32"] = (X, W, 1e-4, 0.0, 0.0, np.float32)
    X, W = _load("sklearn_m513_n96_t21_tol")
    c["cdnmf_m513_n96_t21"] = (X, W, 1e-4, 0.0, 0.0, np.float64)                # early stop (138)
    X, W = _load("sklearn_m25_n64_t32_k50")
    c["cdnmf_m25_zero_utt"] = (np.zeros((5, 25)), W, 1e-4, 0.0, 0.0, np.float64)  # all-zero frames: n_iter = 1
    W0 = W.copy()
    W0[::7] = 0                                                                 # zero exemplar rows
    c["cdnmf_m25_zero_rows"] = (X, W0, 1e-2, 0.0, 0.0, np.float64)
    return c


def geometry_cases():
    """name -> (X_rows, W_rows, tol, alpha_W, l1_ratio, dtype) on seeded synthetic inputs: the lane geometries of
    k_cd_sweep (L lanes per frame, F = 64 / L frames per tile) with N % 16 != 0"""
    c = {}
    c["cdnmf_m6_n17_t70"] = _synth(6, 17, 70, 6) + (1e-4, 0.0, 0.0, np.float64)             # L 1, MPL 8, 64 + 6
    c["cdnmf_m40_n100_t50"] = _synth(40, 100, 50, 40) + (1e-4, 0.0, 0.0, np.float64)        # L 4
    c["cdnmf_m100_n47_t20_f32"] = _synth(100, 47, 20, 100) + (1e-4, 0.0, 0.0, np.float32)   # L 8
    c["cdnmf_m257_n33_t9_l1l2"] = _synth(257, 33, 9, 257) + (1e-4, 0.05, 0.5, np.float64)   # L 32
    c["cdnmf_m1024_n15_t3"] = _synth(1024, 15, 3, 1024) + (1e-4, 0.0, 0.0, np.float64)      # L 64, N < 16
    return c


def make(name, spec):
    X, W, tol, alpha_W, l1_ratio, dt = spec
    Xd, Wd = X.astype(dt), W.astype(dt)
    H, n_iter, trace = run_sklearn(Xd, Wd, tol, 200, alpha_W, l1_ratio)
    out = dict(X_rows=Xd, W_rows=Wd, H=H, n_iter=n_iter, tol=tol, max_iter=200, alpha_W=alpha_W, l1_ratio=l1_ratio,
               dtype=np.dtype(dt).name, violation=trace)
    if dt == np.float32:
        H64, n64, tr64 = run_sklearn(X, W, tol, 200, alpha_W, l1_ratio)
        out.update(H_f64=H64, n_iter_f64=n64, violation_f64=tr64)
    return out


def main():
    check = "--check" in sys.argv
    bad = 0
    for name, spec in {**cases(), **geometry_cases()}.items():
        out = make(name, spec)
        path = os.path.join(GOLDEN, name + ".npz")
        if check:
            ref = np.load(path)
            same = all(np.array_equal(np.asarray(ref[k]), np.asarray(v)) for k, v in out.items())
            print(name, "same" if same else "DIFFERENT")
            bad += not same
        else:
            np.savez_compressed(path, **out)
            print(name, "n_iter", out["n_iter"], os.path.getsize(path), "bytes")
    return bad


if __name__ == "__main__":
    sys.exit(main())
