"""Golden vectors of the multiplicative-update loop that also learns the dictionary.

  * scikit-learn 1.7.2, `non_negative_factorization(X, W, H, n_components=R, init='custom', update_H=True, solver='mu',
    beta_loss='frobenius', tol=tol, max_iter=K)` on seeded synthetic inputs.  scikit-learn's X is T x M, its W is T x R
    (our H^T) and its H is R x M (our W^T); the fixtures store the bin-major orientation: X (M, T), W0 / W (M, R),
    H0 / H (R, T), plus n_iter, tol, max_iter, dtype.
  * the vendored pymf, `NMF(data, num_bases=R).factorize(niter=K, compute_w=True, compute_err=...)`, imported from where
    it lies exactly as tools/make_golden.py does: data, W0, H0, W, H, niter, compute_err, ferr.

Writes tests/golden/dictmu_*.npz; the prefix keeps them out of every other test's glob.

    python tools/make_golden_learn.py [--check]     (--check: recompute and compare instead of writing)
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def run_sklearn(X, W0, H0, tol, max_iter):
    """bin-major in, bin-major out: (W, H, n_iter)"""
    from sklearn.decomposition import non_negative_factorization
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        Wsk, Hsk, n_iter = non_negative_factorization(
            np.ascontiguousarray(X.T), W=np.ascontiguousarray(H0.T), H=np.ascontiguousarray(W0.T),
            n_components=W0.shape[1], init="custom", update_H=True, solver="mu", beta_loss="frobenius", tol=tol,
            max_iter=max_iter)
    return np.ascontiguousarray(Hsk.T), np.ascontiguousarray(Wsk.T), int(n_iter)


def synth(M, R, T, seed):
    """X = a sparse combination of 2 R smooth-ish exemplars plus noise; random positive starts"""
    rng = np.random.default_rng(seed)
    A = rng.random((M, 2 * R)) ** 2 + 1e-3
    X = A @ (rng.random((2 * R, T)) * (rng.random((2 * R, T)) < 0.25)) + 0.01 * rng.random((M, T))
    W0 = rng.random((M, R)) + 1e-4
    H0 = rng.random((R, T)) + 1e-4
    return X, W0, H0


def error_trace(X, W0, H0, checks):
    """||X - W H||_F of scikit-learn's own iterates at the start and after 10, 20, ... iterations"""
    errs = [float(np.linalg.norm(X - W0 @ H0))]
    for c in range(1, checks + 1):
        W, H, _ = run_sklearn(X, W0, H0, 0.0, 10 * c)
        errs.append(float(np.linalg.norm(X - W @ H)))
    return np.array(errs)


def sklearn_cases():
    """name -> (M, R, T, seed, K, tol, dtype, zeros); tol None: picked from the recorded error trace"""
    return {
        "dictmu_sk_m50_r24_t150_k40": (50, 24, 150, 501, 40, 0.0, np.float64, False),
        "dictmu_sk_m201_r20_t100_k40": (201, 20, 100, 502, 40, 0.0, np.float64, False),
        "dictmu_sk_m25_r130_t70_k40": (25, 130, 70, 503, 40, 0.0, np.float64, False),       # crosses a component block
        "dictmu_sk_m1026_r16_t40_k40": (1026, 16, 40, 504, 40, 0.0, np.float64, False),     # several bin blocks
        "dictmu_sk_m50_r24_t150_tol": (50, 24, 150, 501, 200, None, np.float64, False),     # stops early
        "dictmu_sk_m50_r24_t150_k40_f32": (50, 24, 150, 501, 40, 0.0, np.float32, False),
        "dictmu_sk_m50_r24_t150_zeros": (50, 24, 150, 505, 40, 0.0, np.float64, True),
    }


def pymf_cases():
    """name -> (M, R, T, seed, K, compute_err)"""
    return {
        "dictmu_pymf_m50_r24_t150_k40_err": (50, 24, 150, 501, 40, True),
        "dictmu_pymf_m50_r24_t150_k40_noerr": (50, 24, 150, 501, 40, False),
    }


def make(name, spec):
    M, R, T, seed, K, tol, dt, zeros = spec
    X, W0, H0 = synth(M, R, T, seed)
    if zeros:       # a component absent from both factors, two silent frames
        W0[:, 5] = 0.0
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
        assert 20 < n_iter < 100 and n_iter % 10 == 0, n_iter
    out.update(surface="sklearn", X=X, W0=W0, H0=H0, W=W, H=H, n_iter=n_iter, tol=tol, max_iter=K,
               dtype=np.dtype(dt).name)
    return out


def make_pymf(NMF, name, spec):
    M, R, T, seed, K, compute_err = spec
    X, W0, H0 = synth(M, R, T, seed)
    mdl = NMF(X.copy(), num_bases=R)
    mdl.W = W0.copy()
    mdl.H = H0.copy()
    mdl.factorize(niter=K, compute_w=True, compute_err=compute_err)
    ferr = np.asarray(mdl.ferr) if compute_err else np.zeros(0)
    return dict(surface="pymf_full", data=X, W0=W0, H0=H0, W=mdl.W, H=mdl.H, niter=K, compute_err=compute_err, ferr=ferr)


def main():
    check = "--check" in sys.argv
    todo = [(n, make(n, s)) for n, s in sklearn_cases().items()]
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import make_golden
    try:
        NMF = make_golden.import_pymf()
        todo += [(n, make_pymf(NMF, n, s)) for n, s in pymf_cases().items()]
    except Exception as e:  # noqa: BLE001 - report and continue without the pymf fixtures
        print("pymf import failed, pymf fixtures skipped:", repr(e))
    bad = 0
    for name, out in todo:
        path = os.path.join(GOLDEN, name + ".npz")
        if check:
            ref = np.load(path)
            same = all(np.array_equal(np.asarray(ref[k]), np.asarray(v)) for k, v in out.items())
            print(name, "same" if same else "DIFFERENT")
            bad += not same
        else:
            np.savez_compressed(path, **out)
            print(name, "n_iter", out.get("n_iter", len(out.get("ferr", []))), os.path.getsize(path), "bytes")
    return bad


if __name__ == "__main__":
    sys.exit(main())
