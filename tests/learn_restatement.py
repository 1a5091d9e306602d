"""numpy restatement of evc_nmf_learn (include/evc.h): multiplicative updates of both factors, X ~ W H, in the
bin-major orientation (X: M x T, W: M x R, H: R x T).

The dictionary update is evaluated factored, V = W H, Num = X H^T, Den = V H^T, and the sums over the frames are taken
the way k_dict_grad / k_dict_apply take them: S contiguous frame ranges [s T / S, (s + 1) T / S), each summed on its own
(in steps of `chunk` frames), the partial sums added in the order s = 0 .. S - 1.

  surface "sklearn"  per iteration H first, then W: Den[Den == 0] = float32 eps; W <- W * (Num / Den); the activation
                     update with the same guard; err = ||X - W H||_F at the start and every check_every iterations, stop
                     when (prev - err) / err_init < tol (scikit-learn's _fit_multiplicative_update, update_H=True, beta 2,
                     whose W is H^T here and whose H is W^T)
  surface "pymf"     per iteration W first, then H: W <- (W * Num) / (Den + 1e-9), every column divided by its Euclidean
                     norm; H <- (H * P) / (D + 1e-9); from the third error on stop when |err - prev| / T < tol
"""
import numpy as np

EPS32 = 1.1920929e-7


def frame_ranges(T, S):
    return [(s * T // S, (s + 1) * T // S) for s in range(S)]


def dict_terms(X, V, H, S=1, chunk=16):
    """(Num, Den) = (X H^T, V H^T) with the split reduction"""
    dt = X.dtype
    num = np.zeros((X.shape[0], H.shape[0]), dtype=dt)
    den = np.zeros_like(num)
    for b, e in frame_ranges(X.shape[1], S):
        pn, pd = np.zeros_like(num), np.zeros_like(num)
        for t in range(b, e, chunk):
            u = min(t + chunk, e)
            pn += X[:, t:u] @ H[:, t:u].T
            pd += V[:, t:u] @ H[:, t:u].T
        num += pn
        den += pd
    return num, den


def update_w(X, W, H, surface, S=1, chunk=16):
    num, den = dict_terms(X, W @ H, H, S, chunk)
    dt = X.dtype.type
    if surface == "pymf":
        W = (W * num) / (den + dt(1e-9))
        with np.errstate(invalid="ignore", divide="ignore"):
            return W / np.sqrt(np.sum(W * W, axis=0))
    den[den == 0] = dt(EPS32)
    return W * (num / den)


def update_h(X, W, H, surface):
    dt = X.dtype.type
    P = W.T @ X
    D = W.T @ (W @ H)
    if surface == "pymf":
        return (H * P) / (D + dt(1e-9))
    D[D == 0] = dt(EPS32)
    return H * (P / D)


def error(X, W, H):
    R = X.astype(np.float64) - (W @ H).astype(np.float64)
    return float(np.sqrt(np.sum(R * R)))


def learn(X, W0, H0, iters, surface="sklearn", check_every=10, tol=0.0, S=1, chunk=16, dtype=np.float64):
    """-> (W, H, n_iter, err): err[0] the error at the start, err[c] after check c (NaN where not evaluated)"""
    X = np.asarray(X, dtype=dtype)
    W = np.array(W0, dtype=dtype)
    H = np.array(H0, dtype=dtype)
    T = X.shape[1]
    n_checks = iters // check_every if check_every > 0 else 0
    err = np.full(1 + n_checks, np.nan)
    if check_every > 0:
        err[0] = prev = error(X, W, H)
    n_iter = 0
    for it in range(1, iters + 1):
        if surface == "pymf":
            W = update_w(X, W, H, surface, S, chunk)
            H = update_h(X, W, H, surface)
        else:
            H = update_h(X, W, H, surface)
            W = update_w(X, W, H, surface, S, chunk)
        n_iter = it
        if check_every <= 0 or it % check_every:
            continue
        c = it // check_every
        err[c] = e = error(X, W, H)
        if tol > 0 and ((c >= 3 and abs(e - prev) / T < tol) if surface == "pymf" else ((prev - e) / err[0] < tol)):
            break
        prev = e
    return W, H, n_iter, err


def pymf_ferr(err, n_iter, niter):
    """pymf's `ferr` (base.py:238-270) from the trace of a check_every = 1 run that applied n_iter updates: the stop
    test cuts the value that triggered it and the one before stays the last"""
    ferr = np.zeros(niter)
    got = np.asarray(err[1:1 + n_iter])
    T_stop = n_iter < niter
    if not T_stop:
        ferr[:n_iter] = got
        return ferr
    return got[:n_iter - 1].copy()
