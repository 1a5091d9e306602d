"""Golden vectors of the multiplicative-update loop that also learns the dictionary, Kullback-Leibler loss.

scikit-learn 1.7.2, `non_negative_factorization(X, W, H, n_components=R, init='custom', update_H=True, solver='mu',
beta_loss='kullback-leibler', tol=tol, max_iter=K)` on the seeded synthetic inputs of tools/make_golden_learn.py.
scikit-learn's X is T x M, its W is T x R (our H^T) and its H is R x M (our W^T); the fixtures store the bin-major
orientation: X (M, T), W0 / W (M, R), H0 / H (R, T), plus n_iter, tol, max_iter, dtype.

Writes tests/golden/dictkl_sk_*.npz; the prefix keeps them out of every other test's glob.

    python tools/make_golden_learn_kl.py [--check]     (--check: recompute and compare instead of writing)
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden_learn import synth  # noqa: E402


def run_sklearn(X, W0, H0, tol, max_iter):
    """bin-major in, bin-major out: (W, H, n_iter)"""
    from sklearn.decomposition import non_negative_factorization
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        Wsk, Hsk, n_iter = non_negative_factorization(
            np.ascontiguousarray(X.T), W=np.ascontiguousarray(H0.T), H=np.ascontiguousarray(W0.T),
            n_components=W0.shape[1], init="custom", update_H=True, solver="mu", beta_loss="kullback-leibler", tol=tol,
            max_iter=max_iter)
    return np.ascontiguousarray(Hsk.T), np.ascontiguousarray(Wsk.T), int(n_iter)


def kl_error(X, W, H):
    """sqrt(2 KL(X || W H)), scikit-learn's own _beta_divergence(beta=1, square_root=True)"""
    from sklearn.decomposition._nmf import _beta_divergence
    return float(_beta_divergence(np.ascontiguousarray(X.T), np.ascontiguousarray(H.T), np.ascontiguousarray(W.T), 1,
                                  square_root=True))


def error_trace(X, W0, H0, checks):
    """the error of scikit-learn's own iterates at the start and after 10, 20, ... iterations"""
    errs = [kl_error(X, W0, H0)]
    for c in range(1, checks + 1):
        W, H, _ = run_sklearn(X, W0, H0, 0.0, 10 * c)
        errs.append(kl_error(X, W, H))
    return np.array(errs)


def cases():
    """name -> (M, R, T, seed, K, tol, dtype, zeros); tol None: picked from the recorded error trace"""
    return {
        "dictkl_sk_m50_r24_t150_k40": (50, 24, 150, 501, 40, 0.0, np.float64, False),
        "dictkl_sk_m201_r20_t100_k40": (201, 20, 100, 502, 40, 0.0, np.float64, False),
        "dictkl_sk_m25_r130_t70_k40": (25, 130, 70, 503, 40, 0.0, np.float64, False),       # crosses a component block
        "dictkl_sk_m1026_r16_t40_k40": (1026, 16, 40, 504, 40, 0.0, np.float64, False),     # several bin blocks
        "dictkl_sk_m50_r24_t150_tol": (50, 24, 150, 501, 200, None, np.float64, False),     # stops early
        "dictkl_sk_m50_r24_t150_k40_f32": (50, 24, 150, 501, 40, 0.0, np.float32, False),
        "dictkl_sk_m50_r24_t150_zeros": (50, 24, 150, 505, 40, 0.0, np.float64, True),
    }


def make(name, spec):
    M, R, T, seed, K, tol, dt, zeros = spec
    X, W0, H0 = synth(M, R, T, seed)
    if zeros:       # a component without activations (its dictionary column stays positive), two silent frames
        H0[5, :] = 0.0
        X[:, [3, 77]] = 0.0
    X, W0, H0 = X.astype(dt), W0.astype(dt), H0.astype(dt)
    out = {}
    if tol is None:
        errs = error_trace(X, W0, H0, 10)
        ratio = (errs[:-1] - errs[1:]) / errs[0]            # what the stop rule sees at checks 1 .. 10
        tol = float(np.sqrt(ratio[4] * ratio[5]))           # between checks 5 and 6: the stop falls at check 6
        assert ratio[:5].min() > 1.1 * tol and tol > 1.1 * ratio[5], ratio
        out["err_trace"] = errs
    W, H, n_iter = run_sklearn(X, W0, H0, tol, K)
    if "err_trace" in out:
        assert 20 < n_iter < K and n_iter % 10 == 0, n_iter
    out.update(surface="sklearn", loss="kullback-leibler", X=X, W0=W0, H0=H0, W=W, H=H, n_iter=n_iter, tol=tol,
               max_iter=K, dtype=np.dtype(dt).name)
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
