"""Golden vectors of scikit-learn's coordinate descent with BOTH factors updated (the default solver of
NMF(...).fit_transform, the call of the reference's 05_conversion.py:100-106), run by the installed scikit-learn (1.7.2):

    non_negative_factorization(X, W=H0, H=W0, init="custom", update_H=True, solver="cd", n_components=R,
                               beta_loss="frobenius", tol=tol, max_iter=max_iter, alpha_W=..., alpha_H="same",
                               l1_ratio=..., shuffle=False)

on seeded synthetic inputs (squared-uniform dictionary + 0.05, 40 % active activations, 0.05 noise, starts rand + 0.1).
Every case is well posed, R < min(M, T), apart from the tiny M = 6 and M = 1 ones; over-complete ranks amplify rounding
and are left out.  Seeds: the shape's first dimension, except where that draw is badly conditioned - at (25, 17, 70)
and (100, 64, 260), which also serve as float32 fixtures, the seed among 1..5 (and the default) is kept at which
scikit-learn's OWN float32 run lies closest to its float64 run (9e-6 and 1.2e-4 in W; other draws reach 9e-3, where a
float32 trajectory says nothing about a kernel), and at (201, 48, 130) seed 201 meets a near-tie at a clip (a reassociated
float64 restatement sits 1e-10 from scikit-learn there, 1e-12 at five other seeds), so seed 1 is used.  Writes tests/golden/cdlearn_*.npz with
X_rows (T x M), W0_rows (R x M), H0_rows (T x R), the results W_rows and H_rows (float64 unless noted), n_iter, tol, max_iter,
alpha_W, l1_ratio, dtype and `violation` (n_iter x 2: the activation and the dictionary half of every iteration, recorded
by wrapping _update_coordinate_descent here, nowhere else).  float32 cases also store W_rows_f64 / H_rows_f64 / n_iter_f64
/ violation_f64 (the same call in float64).  The prefix `cdlearn_` keeps these out of every other test's glob.

    python tools/make_golden_cd_learn.py [--check]     (--check: recompute and compare instead of writing)
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def run_sklearn(X_rows, W0_rows, H0_rows, tol, max_iter, alpha_W=0.0, l1_ratio=0.0):
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
            Hs, Ws, n_iter = nmf.non_negative_factorization(
                X=X_rows, W=H0_rows.copy(), H=W0_rows.copy(), init="custom", update_H=True,
                n_components=W0_rows.shape[0], beta_loss="frobenius", solver="cd", tol=tol, max_iter=max_iter,
                alpha_W=alpha_W, alpha_H="same", l1_ratio=l1_ratio, shuffle=False)
    finally:
        nmf._update_coordinate_descent = orig
    return Ws, Hs, int(n_iter), np.array(trace).reshape(-1, 2)


def _synth(M, R, T, seed):
    rng = np.random.default_rng(seed)
    Wt = rng.random((R, M)) ** 2 + 0.05
    X = (rng.random((T, R)) * (rng.random((T, R)) < 0.4)) @ Wt + 0.05 * rng.random((T, M))
    W0 = rng.random((R, M)) + 0.1
    H0 = rng.random((T, R)) + 0.1
    return X, W0, H0


def cases():
    """name -> (X_rows, W0_rows, H0_rows, max_iter, tol, alpha_W, l1_ratio, dtype)"""
    c = {}
    X, W0, H0 = _synth(25, 17, 70, 3)
    c["cdlearn_m25_r17_t70"] = (X, W0, H0, 30, 1e-4, 0.0, 0.0, np.float64)            # R % 16 = 1
    c["cdlearn_m25_r17_t70_f32"] = (X, W0, H0, 30, 1e-4, 0.0, 0.0, np.float32)
    c["cdlearn_m25_r17_t70_early"] = (X, W0, H0, 200, 1e-2, 0.0, 0.0, np.float64)     # stops well before max_iter
    c["cdlearn_m25_r17_t70_reg"] = (X, W0, H0, 40, 1e-4, 0.01, 0.5, np.float64)       # all four penalties
    c["cdlearn_m6_r5_t300"] = _synth(6, 5, 300, 6) + (200, 1e-4, 0.0, 0.0, np.float64)  # L = 1, many frames
    X, W0, H0 = _synth(50, 33, 520, 50)
    c["cdlearn_m50_r33_t520_late"] = (X, W0, H0, 200, 1e-3, 0.0, 0.0, np.float64)     # a late stop
    W0z, H0z = W0.copy(), H0.copy()
    W0z[2] = 0.0
    H0z[:, 2] = 0.0                                   # hess == 0 on both sides: the component is left alone
    c["cdlearn_m50_r33_t520_zero"] = (X, W0z, H0z, 25, 1e-4, 0.0, 0.0, np.float64)
    c["cdlearn_m201_r48_t130"] = _synth(201, 48, 130, 1) + (20, 0.0, 0.0, 0.0, np.float64)   # STFT width
    X, W0, H0 = _synth(100, 64, 260, 1)
    c["cdlearn_m100_r64_t260"] = (X, W0, H0, 20, 0.0, 0.0, 0.0, np.float64)           # R a multiple of 16
    c["cdlearn_m100_r64_t260_f32"] = (X, W0, H0, 20, 0.0, 0.0, 0.0, np.float32)
    c["cdlearn_m513_r16_t40"] = _synth(513, 16, 40, 513) + (15, 0.0, 0.0, 0.0, np.float64)     # WORLD width, one block
    c["cdlearn_m1_r1_t40"] = _synth(1, 1, 40, 1) + (50, 1e-4, 0.0, 0.0, np.float64)   # M = R = 1
    return c


def make(spec):
    X, W0, H0, max_iter, tol, alpha_W, l1_ratio, dt = spec
    Xd, Wd, Hd = X.astype(dt), W0.astype(dt), H0.astype(dt)
    W, H, n_iter, trace = run_sklearn(Xd, Wd, Hd, tol, max_iter, alpha_W, l1_ratio)
    out = dict(X_rows=Xd, W0_rows=Wd, H0_rows=Hd, W_rows=W, H_rows=H, n_iter=n_iter, tol=tol, max_iter=max_iter,
               alpha_W=alpha_W, l1_ratio=l1_ratio, dtype=np.dtype(dt).name, violation=trace)
    if dt == np.float32:
        W64, H64, n64, tr64 = run_sklearn(X, W0, H0, tol, max_iter, alpha_W, l1_ratio)
        out.update(W_rows_f64=W64, H_rows_f64=H64, n_iter_f64=n64, violation_f64=tr64)
    return out


def main():
    check = "--check" in sys.argv
    bad = 0
    for name, spec in cases().items():
        out = make(spec)
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
