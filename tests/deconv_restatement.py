"""numpy restatement of evc_deconv_solve / evc_deconv_synthesize (include/evc.h): the activation solve with multi-frame
exemplars, utterance by utterance, bin-major throughout (A_taps (L, M, N), X (M, T), H (N, T)).  float64 unless `dtype` says
otherwise.  With L = 1 it is scikit-learn's fixed-dictionary multiplicative update (tests/golden/sklearn*_m25_*.npz)."""
import numpy as np

EPS = float(np.finfo(np.float32).eps)


def forward(A, H):
    """V[:, t] = sum_{tau <= min(L-1, t)} A_tau H[:, t - tau] over one utterance"""
    L, M, _ = A.shape
    T = H.shape[1]
    V = np.zeros((M, T), dtype=H.dtype)
    for tau in range(min(L, T)):
        V[:, tau:] += A[tau] @ H[:, :T - tau]
    return V


def adjoint(A, Q):
    """out[n, t] = sum_{tau: t + tau < T} A_tau[:, n] . Q[:, t + tau] over one utterance"""
    L, _, N = A.shape
    T = Q.shape[1]
    out = np.zeros((N, T), dtype=Q.dtype)
    for tau in range(min(L, T)):
        out[:, :T - tau] += A[tau].T @ Q[:, tau:]
    return out


def error(X, V, loss):
    """evc_beta_solve's error for beta = 2 (||X - V||_F) and beta = 1, in float64"""
    X, V = X.astype(np.float64), V.astype(np.float64)
    if loss == "frobenius":
        return float(np.sqrt(2.0 * max(0.5 * np.sum((X - V) ** 2), 0.0)))
    sel = X > EPS
    res = np.sum(X[sel] * np.log(X[sel] / np.maximum(V[sel], EPS)) - X[sel]) + np.sum(V)
    return float(np.sqrt(2.0 * max(res, 0.0)))


def update(A, X, H, loss, l1=0.0, l2=0.0):
    """one iteration on one utterance; returns the new H"""
    dt = H.dtype.type
    V = forward(A, H)
    if loss == "frobenius":
        num, den = adjoint(A, X), adjoint(A, V)
    else:
        num, den = adjoint(A, X / np.maximum(V, dt(EPS))), adjoint(A, np.ones_like(X))
    den = den + dt(l1) + dt(l2) * H
    den[den == 0] = dt(EPS)
    return H * (num / den)


def solve_one(A, X, H, loss, iters, l1=0.0, l2=0.0, check_every=0, stop_rule="none", tol=0.0):
    """(H, n_iter, trace[1 + iters // check_every]) of one utterance from the start H"""
    n_slots = 1 + (iters // check_every if check_every > 0 else 0)
    trace = np.full(n_slots, np.nan)
    if X.shape[1] == 0:
        return H, iters, trace
    err0 = prev = None
    if check_every > 0:
        err0 = prev = trace[0] = error(X, forward(A, H), loss)
    for it in range(1, iters + 1):
        H = update(A, X, H, loss, l1, l2)
        if check_every > 0 and it % check_every == 0:
            err = trace[it // check_every] = error(X, forward(A, H), loss)
            if stop_rule == "sklearn" and (prev - err) / err0 < tol:
                return H, it, trace
            prev = err
    return H, iters, trace


def stop_margin(trace, tol):
    """how far, relative to tol, the nearest deciding ratio of a trace is from tol"""
    t = trace[~np.isnan(trace)]
    ratios = (t[:-1] - t[1:]) / t[0]
    return float(np.min(np.abs(ratios - tol)) / tol)


def solve(A, X, H0=None, *, loss, iters, l1=0.0, l2=0.0, init=None, init_value=0.0, check_every=0, stop_rule="none", tol=0.0,
          utt_offsets=None, dtype=np.float64):
    A, X = np.asarray(A, dtype=dtype), np.asarray(X, dtype=dtype)
    N, T = A.shape[2], X.shape[1]
    offs = [0, T] if utt_offsets is None else list(utt_offsets)
    if init is None:
        init = "given" if H0 is not None else "sklearn"
    H = np.zeros((N, T), dtype=dtype) if H0 is None else np.array(H0, dtype=dtype)
    n_iter, traces = [], []
    for a, b in zip(offs[:-1], offs[1:]):
        Xu = X[:, a:b]
        if init == "sklearn" and b > a:
            H[:, a:b] = np.sqrt(np.ascontiguousarray(Xu.T).astype(np.float64).mean() / N)
        elif init == "const":
            H[:, a:b] = init_value
        Hu, n, tr = solve_one(A, Xu, H[:, a:b].copy(), loss, iters, l1, l2, check_every, stop_rule, tol)
        H[:, a:b] = Hu
        n_iter.append(n)
        traces.append(tr)
    return H, np.array(n_iter, dtype=np.int32), np.array(traces)


def synthesize(B, H, utt_offsets=None):
    B, H = np.asarray(B), np.asarray(H)
    T = H.shape[1]
    offs = [0, T] if utt_offsets is None else list(utt_offsets)
    Y = np.zeros((B.shape[1], T), dtype=H.dtype)
    for a, b in zip(offs[:-1], offs[1:]):
        Y[:, a:b] = forward(B, H[:, a:b])
    return Y


def problem(M, N, T, L, seed=0, active=6, utt_offsets=None):
    """the inputs of tests/test_gpu_deconv.py: overlapping taps of one random dictionary, X = V(H*) + 1e-6 with about `active`
    active exemplars per frame"""
    rng = np.random.default_rng(seed)
    D = rng.random((M, N + L - 1)) + 1e-3
    A = np.stack([D[:, tau:tau + N] for tau in range(L)])
    Hs = rng.random((N, T)) * (rng.random((N, T)) < min(1.0, active / N))
    X = synthesize(A, Hs, utt_offsets) + 1e-6
    return A, X
