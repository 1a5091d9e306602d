"""Golden vectors of scikit-learn's coordinate-descent solve with a fixed dictionary: the call of the reference's
04_align_n_nmf_pytorch.py:205-208,

    non_negative_factorization(X=X, H=W, init="custom", update_H=False, n_components=W.shape[0],
                               beta_loss="frobenius", solver='cd', tol=tol, max_iter=200)

run by the installed scikit-learn (1.7.2) on inputs of the existing fixtures.  Writes tests/golden/cdnmf_*.npz with
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
    for name, spec in cases().items():
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
