"""Convex NMF (evc_convex_learn) restated in numpy: the reference of the GPU tests for shapes without a recorded fixture,
itself checked against every recorded pymf result (tests/test_convex_host.py).

Bin-major throughout: X is M x T, signed; G is T x R and H is R x T, both with a non-negative start.  With
pos(m) = (|m| + m) / 2, neg(m) = (|m| - m) / 2 and K = X^T X, per iteration
    Np = pos(K) G;  Nn = neg(K) G
    H:  Sp = G^T Np;  Sn = G^T Nn;  Ha = Np + H^T Sn;  Hb = (Nn + H^T Sp) + eps;  H^T <- H^T * sqrt(Ha / Hb)
    G (with the new H):  C = H H^T;  Wa = pos(K) H^T + Nn C;  Wb = (neg(K) H^T + Np C) + eps;  G <- G * sqrt(Wa / Wb)
pymf (cnmf.py:152-154) multiplies the T x T product H^T G^T by Nn; here the R x R matrix G^T Nn stands in the middle.  The error
is ||X - (X G) H||_F; check c (after iteration c * check_every) stops the loop when c >= 3 and |err_c - err_(c-1)| / T < tol."""
import numpy as np

PYMF_TOL = float(np.finfo(float).eps)


def pos(m):
    return (np.abs(m) + m) / 2


def neg(m):
    return (np.abs(m) - m) / 2


def problem(M, T, R, seed):
    """signed exemplars in R loose groups that follow one another in time, and the labels of the groups"""
    rng = np.random.default_rng(seed)
    assign = (np.arange(T) * R) // T
    centres = rng.standard_normal((M, R))
    X = centres[:, assign] + 0.3 * rng.standard_normal((M, T))
    return X, assign


def cluster_start(assign, R):
    """pymf's start from cluster labels (cnmf.py:77-89): G0 = (one-hot + 0.01) / cluster size (T x R), H0 = one-hot + 0.2"""
    assign = np.asarray(assign)
    T = len(assign)
    num = np.array([np.sum(assign == i) for i in range(R)], dtype=np.float64)
    H = np.zeros((R, T))
    H[assign, np.arange(T)] = 1.0
    H += 0.2
    G = np.zeros((T, R))
    G[np.arange(T), assign] = 1.0
    G += 0.01
    G /= num[assign].reshape(-1, 1)
    return G, H


def frobenius(X, G, H):
    """||X - (X G) H||_F in float64 from the operands as they are"""
    V = ((X @ G) @ H).astype(np.float64)
    return float(np.sqrt(np.sum((X.astype(np.float64) - V) ** 2)))


def n_slots(iters, check_every):
    return 1 + (iters // check_every if check_every > 0 else 0)


def learn(X, G0, H0, iters, *, update="both", eps=1e-9, check_every=1, tol=0.0, dtype=np.float64):
    """-> G (T x R), H (R x T), n_iter (iterations carried out), trace (the error at the start, then at every check that was
    evaluated, NaN elsewhere).  dtype=np.float32 runs the updates' arithmetic in float32 (the errors stay float64)."""
    X = np.asarray(X, dtype=dtype)
    G, H = np.array(G0, dtype=dtype), np.array(H0, dtype=dtype)
    e = dtype(eps)
    T = X.shape[1]
    trace = np.full(n_slots(iters, check_every), np.nan)
    K = X.T @ X
    Kp, Kn = pos(K), neg(K)
    if check_every > 0:
        trace[0] = frobenius(X, G, H)
    prev, n_iter = trace[0], iters
    with np.errstate(divide="ignore", invalid="ignore"):
        for it in range(1, iters + 1):
            Np, Nn = Kp @ G, Kn @ G
            if update in ("both", "h"):
                Sp, Sn = G.T @ Np, G.T @ Nn
                Ha = Np + H.T @ Sn
                Hb = (Nn + H.T @ Sp) + e
                H = (H.T * np.sqrt(Ha / Hb)).T
            if update in ("both", "g"):
                C = H @ H.T
                Wa = Kp @ H.T + Nn @ C
                Wb = (Kn @ H.T + Np @ C) + e
                G = G * np.sqrt(Wa / Wb)
            if check_every > 0 and it % check_every == 0:
                c = it // check_every
                err = trace[c] = frobenius(X, G, H)
                if c >= 3 and abs(err - prev) / T < tol:
                    n_iter = it
                    break
                prev = err
    return G, np.ascontiguousarray(H), n_iter, trace


def pymf_ferr(trace, n_iter, niter, T):
    """pymf's ferr from a trace with check_every = 1 and tol = PYMF_TOL: cnmf.py:172-175 cuts it to ferr[:i] when the stop
    fires at update i + 1 (the last update's included)"""
    ferr = np.asarray(trace[1:1 + n_iter])
    if n_iter >= 3 and abs(ferr[n_iter - 1] - ferr[n_iter - 2]) / T < PYMF_TOL:
        return ferr[:n_iter - 1].copy()
    out = np.zeros(niter)
    out[:n_iter] = ferr
    return out
