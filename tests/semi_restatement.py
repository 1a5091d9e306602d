"""Semi-NMF activations (evc_semi_solve) restated in numpy, utterance by utterance: the reference of the GPU tests for shapes
without a recorded fixture, itself checked against every recorded pymf result (tests/test_semi_host.py).

Bin-major throughout: A is M x N and X is M x T, both signed; H is N x T with a non-negative start.  Per iteration
    P = A^T X;  G = A^T A;  H1 = pos(P) + neg(G) H;  H2 = (neg(P) + pos(G) H) + eps;  H <- H * sqrt(H1 / H2)
with pos(m) = (|m| + m) / 2 and neg(m) = (|m| - m) / 2.  The error of an utterance is ||X_u - A H_u||_F; check c (after
iteration c * check_every) stops it under the "pymf" rule when c >= 3 and |err_c - err_(c-1)| / T_u < tol."""
import numpy as np

PYMF_TOL = float(np.finfo(float).eps)


def pos(m):
    return (np.abs(m) + m) / 2


def neg(m):
    return (np.abs(m) - m) / 2


def problem(M, N, T, seed, active=6):
    """a signed dictionary, signed frames near its non-negative cone and a start as pymf draws it"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((M, N))
    Hs = rng.random((N, T)) * (rng.random((N, T)) < min(1.0, active / N))
    X = A @ Hs + 0.05 * rng.standard_normal((M, T))
    H0 = rng.random((N, T)) + 1e-4
    return A, X, H0


def update(G, P, H, eps):
    """one update of the columns H; every operand keeps H's dtype"""
    e = H.dtype.type(eps)
    with np.errstate(divide="ignore", invalid="ignore"):
        H1 = pos(P) + neg(G) @ H
        H2 = (neg(P) + pos(G) @ H) + e
        return H * np.sqrt(H1 / H2)


def frobenius(A, X, H):
    """||X - A H||_F in float64 from the operands as they are"""
    V = (A @ H).astype(np.float64)
    return float(np.sqrt(np.sum((X.astype(np.float64) - V) ** 2)))


def n_slots(iters, check_every):
    return 1 + (iters // check_every if check_every > 0 else 0)


def solve(A, X, H0, iters, *, eps=1e-9, check_every=0, stop_rule="none", tol=0.0, utt_offsets=None, dtype=np.float64):
    """-> H (N x T), n_iter (updates applied per utterance), trace (n_utt x slots: the error at the start, then at every
    check that was evaluated, NaN elsewhere).  An empty utterance: n_iter = iters, all NaN.  dtype=np.float32 runs the
    update's arithmetic in float32 (the errors stay float64)."""
    A, X = np.asarray(A, dtype=dtype), np.asarray(X, dtype=dtype)
    H = np.array(H0, dtype=dtype)
    offs = [0, X.shape[1]] if utt_offsets is None else list(utt_offsets)
    slots = n_slots(iters, check_every)
    n_iter = np.full(len(offs) - 1, iters, dtype=np.int32)
    trace = np.full((len(offs) - 1, slots), np.nan)
    G = A.T @ A
    for u in range(len(offs) - 1):
        t0, t1 = offs[u], offs[u + 1]
        if t0 == t1:
            continue
        Xu, Hu = X[:, t0:t1], H[:, t0:t1].copy()
        P = A.T @ Xu
        if check_every > 0:
            trace[u, 0] = frobenius(A, Xu, Hu)
        prev = trace[u, 0]
        for it in range(1, iters + 1):
            Hu = update(G, P, Hu, eps)
            if check_every > 0 and it % check_every == 0:
                c = it // check_every
                err = trace[u, c] = frobenius(A, Xu, Hu)
                if stop_rule == "pymf" and c >= 3 and abs(err - prev) / (t1 - t0) < tol:
                    n_iter[u] = it
                    break
                prev = err
        H[:, t0:t1] = Hu
    return H, n_iter, trace


def pymf_ferr(trace_row, n_iter, niter, T):
    """pymf's ferr of one utterance from a trace with check_every = 1: base.py:268 cuts it to ferr[:i] when the stop fires at
    update i + 1 (the last update's included)"""
    ferr = np.asarray(trace_row[1:1 + n_iter])
    if n_iter >= 3 and abs(ferr[n_iter - 1] - ferr[n_iter - 2]) / T < PYMF_TOL:
        return ferr[:n_iter - 1].copy()
    out = np.zeros(niter)
    out[:n_iter] = ferr
    return out


def factorize_w(X, H0, niter):
    """pymf's default call, factorize(compute_w=True): per iteration W = X H^T (H H^T)^-1 (snmf.py:61-64), then one update of
    H, then the error and the stop.  -> W, H, ferr"""
    X = np.asarray(X, dtype=np.float64)
    H = np.array(H0, dtype=np.float64)
    ferr = np.zeros(niter)
    W = None
    for i in range(niter):
        W = np.dot(np.dot(X, H.T), np.linalg.inv(np.dot(H, H.T)))
        H = update(W.T @ W, W.T @ X, H, 1e-9)
        ferr[i] = frobenius(W, X, H)
        if i > 1 and abs(ferr[i] - ferr[i - 1]) / X.shape[1] < PYMF_TOL:
            ferr = ferr[:i]
            break
    return W, H, ferr
