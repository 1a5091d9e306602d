"""Golden vectors of the multiplicative-update loop that also learns the dictionary, under any beta-divergence.

scikit-learn 1.7.2, `non_negative_factorization(X, W, H, n_components=R, init='custom', update_H=True, solver='mu',
beta_loss=beta, tol=tol, max_iter=K, alpha_W=alpha, alpha_H='same', l1_ratio=l1_ratio)` on the seeded synthetic inputs of
tools/make_golden_learn.py.  scikit-learn's X is T x M, its W is T x R (our H^T) and its H is R x M (our W^T); the
fixtures store the bin-major orientation: X (M, T), W0 / W (M, R), H0 / H (R, T), plus n_iter, max_iter, tol, beta, err
(scikit-learn's own _beta_divergence of its own iterates at the start and after every 10 iterations), alpha, l1_ratio,
dtype.

Every case asserts, for scikit-learn alone, that no positive entry of any iterate of either factor lies within a factor
1 +- 1e-3 of 2^-52 (the flush threshold: a kernel within 1e-9 cannot then flip a flush); the early stops that
20 < n_iter < max_iter with every evaluated check at least 1 % of tol away from the threshold; the `flush` cases that at
least 10 entries end at exact zero in each factor that flushes at that beta.

Writes tests/golden/dictbeta_sk_*.npz; the prefix keeps them out of every other test's glob.

    python tools/make_golden_beta_learn.py [--check] [name ...]     (--check: recompute and compare instead of writing)
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden_learn import synth  # noqa: E402

E64 = np.finfo(np.float64).eps


def run_sklearn(X, W0, H0, beta, tol, max_iter, alpha=0.0, l1_ratio=0.0):
    """bin-major in, bin-major out: (W, H, n_iter)"""
    from sklearn.decomposition import non_negative_factorization
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        Wsk, Hsk, n_iter = non_negative_factorization(
            np.ascontiguousarray(X.T), W=np.ascontiguousarray(H0.T), H=np.ascontiguousarray(W0.T),
            n_components=W0.shape[1], init="custom", update_H=True, solver="mu", beta_loss=beta, tol=tol,
            max_iter=max_iter, alpha_W=alpha, alpha_H="same", l1_ratio=l1_ratio)
    return np.ascontiguousarray(Hsk.T), np.ascontiguousarray(Wsk.T), int(n_iter)


def sk_error(X, W, H, beta):
    from sklearn.decomposition._nmf import _beta_divergence
    return float(_beta_divergence(np.ascontiguousarray(X.T), np.ascontiguousarray(H.T), np.ascontiguousarray(W.T), beta,
                                  square_root=True))


def iterates(X, W0, H0, beta, K, alpha, l1_ratio):
    """scikit-learn's own iterates after 1 .. K iterations, one at a time (each run restarts from the last result: the
    loop carries no state but the factors); checks the flush margin on the way"""
    out = []
    W, H = W0, H0
    for _ in range(K):
        W, H, _n = run_sklearn(X, W, H, beta, 0.0, 1, alpha, l1_ratio)
        for F in (W, H):
            pos = F[F > 0]
            assert not np.any((pos > E64 * (1 - 1e-3)) & (pos < E64 * (1 + 1e-3))), "an entry sits at the flush threshold"
        out.append((W, H))
    return out


def cases():
    """name -> dict(M, R, T, seed, K, beta, tol (None: picked from the error trace), dtype, alpha, l1_ratio, flush, zeros)"""
    def c(M, R, T, seed, K, beta, tol=0.0, dtype=np.float64, alpha=0.0, l1_ratio=0.0, flush=False, zeros=False):
        return dict(M=M, R=R, T=T, seed=seed, K=K, beta=beta, tol=tol, dtype=dtype, alpha=alpha, l1_ratio=l1_ratio,
                    flush=flush, zeros=zeros)
    d = {}
    for tag, beta in (("bm1", -1.0), ("b0", 0.0), ("b0p5", 0.5), ("b1p5", 1.5), ("b3", 3.0), ("b0p3", 0.3)):
        d[f"dictbeta_sk_m25_r17_t70_k40_{tag}"] = c(25, 17, 70, 601, 40, beta)       # b0p3: the general pow
    d["dictbeta_sk_m201_r20_t100_k40_b0"] = c(201, 20, 100, 602, 40, 0.0)            # wide, ragged
    d["dictbeta_sk_m513_r16_t40_k20_b0p5"] = c(513, 16, 40, 603, 20, 0.5)            # widest
    d["dictbeta_sk_m25_r130_t70_k40_b0"] = c(25, 130, 70, 604, 40, 0.0)              # crosses a component block
    d["dictbeta_sk_m17_r300_t40_k20_b0p5"] = c(17, 300, 40, 605, 20, 0.5)            # beyond the fused bound
    d["dictbeta_sk_m50_r24_t150_tol_b0"] = c(50, 24, 150, 606, 200, 0.0, tol=None)   # stops early
    d["dictbeta_sk_m50_r24_t150_tol_b1p5"] = c(50, 24, 150, 606, 200, 1.5, tol=None)
    d["dictbeta_sk_m50_r24_t150_k40_reg_b0p5"] = c(50, 24, 150, 607, 40, 0.5, alpha=0.01, l1_ratio=0.5)
    d["dictbeta_sk_m50_r24_t150_k40_f32_b0"] = c(50, 24, 150, 608, 40, 0.0, dtype=np.float32)
    for tag, beta in (("b0p5", 0.5), ("b0", 0.0), ("b1", 1.0)):
        d[f"dictbeta_sk_m25_r17_t70_k30_flush_{tag}"] = c(25, 17, 70, 609, 30, beta, flush=True)
    d["dictbeta_sk_m50_r24_t150_k40_zeros_b1p5"] = c(50, 24, 150, 610, 40, 1.5, zeros=True)
    return d


def make(name, s):
    X, W0, H0 = synth(s["M"], s["R"], s["T"], s["seed"])
    beta, K, dt = s["beta"], s["K"], s["dtype"]
    if s["flush"]:      # ~4 % of W0 (425 entries: enough for 10 zeros) and ~3 % of H0 far below the flush threshold
        rng = np.random.default_rng(s["seed"] + 1000)
        W0[rng.random(W0.shape) < 0.04] = 1e-19
        H0[rng.random(H0.shape) < 0.03] = 1e-19
    if s["zeros"]:      # a component without activations, two silent frames
        H0[5, :] = 0.0
        X[:, [3, 77]] = 0.0
    X, W0, H0 = X.astype(dt), W0.astype(dt), H0.astype(dt)
    tol = s["tol"]
    steps = iterates(X, W0, H0, beta, K if tol is not None else 150, s["alpha"], s["l1_ratio"])
    checks = len(steps) // 10
    errs = np.array([sk_error(X, W0, H0, beta)] + [sk_error(X, *steps[10 * c - 1], beta) for c in range(1, checks + 1)])
    if tol is None:
        # what the stop rule sees at checks 1 .. 15 (not monotone under Itakura-Saito): the stop falls at the first check
        # c >= 3 whose ratio lies clearly below every earlier one, tol halfway (geometrically) between the two
        ratio = (errs[:-1] - errs[1:]) / errs[0]
        c = next(c for c in range(3, checks + 1) if 1.05 * ratio[c - 1] < ratio[:c - 1].min())
        tol = float(np.sqrt(ratio[c - 1] * ratio[:c - 1].min()))
        assert ratio[:c - 1].min() > 1.01 * tol and tol > 1.01 * ratio[c - 1], ratio
    W, H, n_iter = run_sklearn(X, W0, H0, beta, tol, K, s["alpha"], s["l1_ratio"])
    if s["tol"] is None:
        assert 20 < n_iter < K and n_iter % 10 == 0, n_iter
        errs = errs[:1 + n_iter // 10]
    assert np.array_equal(W, steps[n_iter - 1][0]) and np.array_equal(H, steps[n_iter - 1][1]), "restart changed the iterates"
    if s["flush"]:
        assert (H == 0).sum() >= 10 or not beta < 1, (H == 0).sum()
        assert (W == 0).sum() >= 10, (W == 0).sum()
    return dict(X=X, W0=W0, H0=H0, W=W, H=H, n_iter=n_iter, max_iter=K, tol=tol, beta=beta, err=errs, alpha=s["alpha"],
                l1_ratio=s["l1_ratio"], dtype=np.dtype(dt).name)


def main():
    check = "--check" in sys.argv
    names = [a for a in sys.argv[1:] if not a.startswith("--")]
    bad = 0
    for name, spec in cases().items():
        if names and name not in names:
            continue
        out = make(name, spec)
        path = os.path.join(GOLDEN, name + ".npz")
        if check:
            ref = np.load(path)
            same = all(np.array_equal(np.asarray(ref[k]), np.asarray(v)) for k, v in out.items())
            print(name, "same" if same else "DIFFERENT")
            bad += not same
        else:
            np.savez_compressed(path, **out)
            print(name, "n_iter", out["n_iter"], "zeros W/H", int((out["W"] == 0).sum()), int((out["H"] == 0).sum()),
                  os.path.getsize(path), "bytes")
    return bad


if __name__ == "__main__":
    sys.exit(main())
