"""Golden vectors of scikit-learn's multiplicative-update solve with a fixed dictionary under the beta-divergences that
evc_beta_solve serves: the call of the reference's _factorize (04_align_n_nmf.py:212-213) with the
beta_loss the caller asked for,

    non_negative_factorization(X=X, H=W, init="custom", update_H=False, n_components=W.shape[0],
                               beta_loss=beta, solver="mu", tol=tol, max_iter=K, alpha_W=..., l1_ratio=...)

run by the installed scikit-learn (1.7.2) on seeded synthetic inputs drawn as tools/make_golden.py draws them.  Writes
tests/golden/betamu_*.npz with X_rows, W_rows, H (N x T), n_iter, beta, tol, max_iter, alpha_W, l1_ratio, dtype and `err`:
the error at the start, then at every check scikit-learn evaluated (recorded by wrapping _beta_divergence here, nowhere
else; NaN where not evaluated).  float32 cases also store H_f64 (the same call in float64).

Every early-stop case asserts that each evaluated check sits at least 1 % of tol off the threshold, so that no fixture
hangs on a rounding.

    python tools/make_golden_beta.py [--check]     (--check: recompute and compare instead of writing)
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import synth  # noqa: E402


def run_sklearn(X_rows, W_rows, beta, tol, max_iter, alpha_W=0.0, l1_ratio=0.0):
    import sklearn.decomposition._nmf as nmf
    seen = []
    orig = nmf._beta_divergence

    def wrapped(*a, **k):
        v = orig(*a, **k)
        if k.get("square_root"):
            seen.append(float(v))
        return v

    nmf._beta_divergence = wrapped
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            W, _, n_iter = nmf.non_negative_factorization(
                X=X_rows, H=W_rows, init="custom", update_H=False, n_components=W_rows.shape[0], beta_loss=beta,
                solver="mu", tol=tol, max_iter=max_iter, alpha_W=alpha_W, l1_ratio=l1_ratio)
    finally:
        nmf._beta_divergence = orig
    n_checks = int(n_iter) // 10 if tol > 0 else 0
    err = np.full(1 + max_iter // 10, np.nan)
    err[:1 + n_checks] = seen[:1 + n_checks]
    return np.ascontiguousarray(W.T), int(n_iter), err


def _inputs(M, N, T, seed):
    A, _, X = synth(M, N, T, seed)
    return np.ascontiguousarray(X.T), np.ascontiguousarray(A.T)      # T x M, N x M (the script's orientation)


def _tag(beta):
    return ("m" if beta < 0 else "") + ("%g" % abs(beta)).replace(".", "p")


def cases():
    """name -> dict(X, W, beta, tol, K, alpha_W, l1_ratio, dtype, stop)"""
    c = {}

    def add(name, X, W, beta, tol=0.0, K=50, alpha_W=0.0, l1_ratio=0.0, dtype=np.float64, stop=None):
        c[name] = dict(X=X, W=W, beta=float(beta), tol=tol, K=K, alpha_W=alpha_W, l1_ratio=l1_ratio, dtype=dtype, stop=stop)

    X, W = _inputs(25, 64, 32, 401)
    for beta in (-1, 0, 0.5, 1.5, 3):                                   # fixed K, no stop
        add(f"betamu_m25_n64_t32_k50_b{_tag(beta)}", X, W, beta)
    # early stops (seeds chosen for the margin; the stop iteration is scikit-learn's).  Seed 345 was picked because it stops
    # at iteration 40 under beta = 0 (other seeds of this draw stop at 60 - 80); beta = 1.5 at tol 2e-2 only ever stops at
    # 50 or 60 on this draw and beta = 0.5 at tol 5e-3 at 130 - 150, so those two keep a seed with a wide margin
    add("betamu_m25_n64_t50_b0_tol2e-2", *_inputs(25, 64, 50, 345), 0, tol=2e-2, K=150, stop=40)
    add("betamu_m25_n64_t50_b1p5_tol2e-2", *_inputs(25, 64, 50, 0), 1.5, tol=2e-2, K=150, stop=50)
    add("betamu_m25_n64_t50_b3_tol2e-2", *_inputs(25, 64, 50, 6), 3, tol=2e-2, K=150, stop=20)
    add("betamu_m25_n64_t50_b0p5_tol5e-3", *_inputs(25, 64, 50, 6), 0.5, tol=5e-3, K=150, stop=140)
    # geometry: one bin, ragged N, the STFT and WORLD widths
    add("betamu_m1_n48_t37_b0p5", *_inputs(1, 48, 37, 11), 0.5, K=30)
    add("betamu_m100_n47_t20_b0", *_inputs(100, 47, 20, 12), 0, tol=3e-2, K=150, stop=80)
    add("betamu_m201_n128_t40_b0p5", *_inputs(201, 128, 40, 13), 0.5, tol=2e-2, K=150, stop=20)
    add("betamu_m513_n96_t21_b0", *_inputs(513, 96, 21, 14), 0, K=30)
    # a zero frame, a zero bin and a zero exemplar (beta > 0: scikit-learn refuses zeros in X for beta <= 0)
    X, W = _inputs(25, 64, 50, 21)
    X[3] = 0.0
    X[:, 5] = 0.0
    W[7] = 0.0
    for beta in (0.5, 1.5):
        add(f"betamu_m25_n64_t50_zeros_b{_tag(beta)}", X, W, beta, K=40)
    add("betamu_m25_n64_t50_reg_b0p5", *_inputs(25, 64, 50, 22), 0.5, K=40, alpha_W=0.01, l1_ratio=0.3)
    add("betamu_m25_n64_t32_b0_f32", *_inputs(25, 64, 32, 23), 0, dtype=np.float32)
    add("betamu_m201_n128_t40_b0p5_f32", *_inputs(201, 128, 40, 24), 0.5, dtype=np.float32)
    return c


def make(name, s):
    dt = s["dtype"]
    X, W = s["X"].astype(dt), s["W"].astype(dt)
    H, n_iter, err = run_sklearn(X, W, s["beta"], s["tol"], s["K"], s["alpha_W"], s["l1_ratio"])
    assert np.all(np.isfinite(H)), name
    if s["tol"] > 0:
        assert n_iter == s["stop"] and n_iter < s["K"], (name, n_iter)
        k = n_iter // 10
        dec = (err[:k] - err[1:k + 1]) / err[0]
        assert np.min(np.abs(dec - s["tol"])) >= 0.01 * s["tol"], (name, dec)
    if "zeros" in name:
        assert np.all(H[:, 3] == 0) and np.all(H[7] == 0), name
    out = dict(X_rows=X, W_rows=W, H=H, n_iter=n_iter, err=err, beta=s["beta"], tol=s["tol"], max_iter=s["K"],
               alpha_W=s["alpha_W"], l1_ratio=s["l1_ratio"], dtype=np.dtype(dt).name)
    if dt == np.float32:
        out["H_f64"] = run_sklearn(s["X"], s["W"], s["beta"], s["tol"], s["K"], s["alpha_W"], s["l1_ratio"])[0]
    return out


def main():
    check = "--check" in sys.argv
    bad = 0
    for name, spec in cases().items():
        out = make(name, spec)
        path = os.path.join(GOLDEN, name + ".npz")
        if check:
            ref = np.load(path)
            same = all(np.array_equal(np.asarray(ref[k]), np.asarray(v), equal_nan=np.asarray(v).dtype.kind == "f")
                       for k, v in out.items())
            print(name, "same" if same else "DIFFERENT")
            bad += not same
        else:
            np.savez_compressed(path, **out)
            print(name, "n_iter", out["n_iter"], os.path.getsize(path), "bytes")
    return bad


if __name__ == "__main__":
    sys.exit(main())
