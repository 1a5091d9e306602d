"""evc_kmeans in plain numpy: the statement the device is tested against (tests/test_gpu_kmeans.py) and that reproduces
every recorded pymf result (tests/test_kmeans_host.py).  pymf kmeans.py:57-83 on base.py:238-270 with dist.py:54-60, 104-127.

One assignment with the start centres; per round the means (an empty cluster keeps its centre), the assignment and
err = ||X - W[:, labels]||_F in float64.  labels[t] is the first index of the least direct-form distance
sum_m (x_m - w_m)^2, bins ascending, in the working type.  Stops: "pymf" (from the third round on, |err - err_prev| / T < tol)
and "labels" (a round changed no label).

The margin that assign() and run() return is the condition a test states before it demands EQUAL labels of another
arithmetic: the least, over every sample of every assignment pass, of (d2 - d1) / (||x_t|| + max_r ||w_r||) with d1 <= d2 the
two least distances, or inf where the two are exactly equal (the first index then wins in every arithmetic that gives
identical centres identical distances)."""
import numpy as np

PYMF_TOL = float(np.finfo(float).eps)


def unit_roundoff(dtype):
    return float(np.finfo(dtype).eps) / 2


def margin_bound(M, dtype):
    """what the least margin of a case must reach for labels of `dtype` arithmetic to be comparable: 16 (M + 4) u"""
    return 16.0 * (M + 4) * unit_roundoff(dtype)


def problem(M, T, R, seed, spread=0.3):
    """signed samples around R centres, in no order"""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((M, R))
    X = centres[:, rng.integers(0, R, T)] + spread * rng.standard_normal((M, T))
    return X


def spread_start(T, R):
    """the start compact_dictionary_kmeans takes: the samples at ((2 i + 1) T) // (2 R)"""
    return ((2 * np.arange(R, dtype=np.int64) + 1) * T) // (2 * R)


def distances2(X, W):
    """[R][T] squared distances by the direct form in X's dtype, bins ascending"""
    d = np.empty((W.shape[1], X.shape[1]), dtype=X.dtype)
    for r in range(W.shape[1]):
        d[r] = ((X - W[:, r:r + 1]) ** 2).sum(axis=0)
    return d


def assign(X, W):
    """-> labels (the first of the least), and the pass's least margin (module docstring)"""
    d2 = distances2(X, W)
    labels = np.argmin(d2, axis=0)
    if W.shape[1] == 1:
        return labels, np.inf
    two = np.sqrt(np.partition(d2.astype(np.float64), 1, axis=0)[:2])
    scale = np.linalg.norm(X.astype(np.float64), axis=0) + np.linalg.norm(W.astype(np.float64), axis=0).max()
    with np.errstate(divide="ignore", invalid="ignore"):
        m = np.where(two[1] == two[0], np.inf, (two[1] - two[0]) / scale)
    return labels, float(np.min(m))


def update_centres(X, W, labels):
    for r in range(W.shape[1]):
        idx = labels == r
        n = int(np.sum(idx))
        if n > 0:
            W[:, r] = X[:, idx].sum(axis=1, dtype=X.dtype) / X.dtype.type(n)


def error(X, W, labels):
    return float(np.sqrt(np.sum((X.astype(np.float64) - W.astype(np.float64)[:, labels]) ** 2)))


def run(X, W0, iters, *, update="both", stop="pymf", tol=PYMF_TOL, dtype=np.float64):
    """-> W, labels, counts, n_iter (rounds carried out), trace ([1 + iters], NaN where not evaluated), the least margin"""
    X = np.asarray(X, dtype=dtype)
    W = np.array(W0, dtype=dtype)
    T, R = X.shape[1], W.shape[1]
    trace = np.full(1 + iters, np.nan)
    labels, margin = assign(X, W)
    trace[0] = error(X, W, labels)
    n_iter = iters
    for it in range(1, iters + 1):
        if update == "both":
            update_centres(X, W, labels)
        new, m = assign(X, W)
        margin = min(margin, m)
        changed = int(np.sum(new != labels))
        labels = new
        trace[it] = error(X, W, labels)
        if stop == "pymf" and it >= 3 and abs(trace[it] - trace[it - 1]) / T < tol:
            n_iter = it
            break
        if stop == "labels" and changed == 0:
            n_iter = it
            break
    return W, labels.astype(np.int32), np.bincount(labels, minlength=R).astype(np.int32), n_iter, trace, margin


def pymf_ferr(trace, n_iter, niter, T):
    """pymf's ferr from a trace with stop = "pymf" and tol = PYMF_TOL: base.py:266-270 cuts it to ferr[:i] when the stop fires in
    round i + 1"""
    ferr = np.asarray(trace[1:1 + n_iter])
    if n_iter >= 3 and abs(ferr[n_iter - 1] - ferr[n_iter - 2]) / T < PYMF_TOL:
        return ferr[:n_iter - 1].copy()
    out = np.zeros(niter)
    out[:n_iter] = ferr
    return out
