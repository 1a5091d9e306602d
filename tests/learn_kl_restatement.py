"""numpy restatement of evc_nmf_learn with loss = EVC_LOSS_KL (include/evc.h): scikit-learn's multiplicative updates of
both factors under the generalised Kullback-Leibler divergence (_fit_multiplicative_update, beta_loss = 1,
update_H=True, no regularisation), in the bin-major orientation (X: M x T, W: M x R, H: R x T; scikit-learn's W is H^T
here and its H is W^T).

One iteration:
  1. activations:  c_r = sum_m W[m, r], c_r == 0 -> eps;  V = W H;  Q = X / max(V, eps);  H <- H * ((W^T Q) / c)
  2. dictionary, with the new H:  V = W H;  Q = X / max(V, eps);  Num = Q H^T;  s_r = sum_t H[r, t], s_r == 0 -> 1.0
     (_nmf.py:679-680: 1, not eps);  W <- W * (Num / s)
  3. err = sqrt(max(sum_t e_t, 0)), e_t = 2 (sum_m V[m, t] + sum_{m: X > eps} (X log(X / max(V, eps)) - X)[m, t]) in
     float64, at the start and every check_every iterations; stop when (prev - err) / err_at_start < tol (tol = 0: never)
eps = 1.1920929e-7 in the call's dtype.

The sums over the frames (Num and s_r) are taken the way k_dict_grad / k_dict_apply take them: S contiguous frame ranges
[s T / S, (s + 1) T / S), each summed on its own (in steps of `chunk` frames), the partial sums added in the order
s = 0 .. S - 1.
"""
import numpy as np

EPS32 = 1.1920929e-7


def frame_ranges(T, S):
    return [(s * T // S, (s + 1) * T // S) for s in range(S)]


def quotient(X, W, H):
    dt = X.dtype.type
    V = W @ H
    V[V < dt(EPS32)] = dt(EPS32)
    return X / V


def dict_terms(Q, H, S=1, chunk=16):
    """(Num, s) = (Q H^T, row sums of H) with the split reduction"""
    dt = Q.dtype
    num = np.zeros((Q.shape[0], H.shape[0]), dtype=dt)
    hs = np.zeros(H.shape[0], dtype=dt)
    for b, e in frame_ranges(Q.shape[1], S):
        pn, ps = np.zeros_like(num), np.zeros_like(hs)
        for t in range(b, e, chunk):
            u = min(t + chunk, e)
            pn += Q[:, t:u] @ H[:, t:u].T
            ps += H[:, t:u].sum(axis=1)
        num += pn
        hs += ps
    return num, hs


def update_w(X, W, H, S=1, chunk=16):
    num, hs = dict_terms(quotient(X, W, H), H, S, chunk)
    hs[hs == 0] = X.dtype.type(1.0)
    return W * (num / hs)


def update_h(X, W, H):
    c = W.sum(axis=0)
    c[c == 0] = X.dtype.type(EPS32)
    return H * ((W.T @ quotient(X, W, H)) / c[:, None])


def error(X, W, H):
    X = X.astype(np.float64)
    V = (W @ H).astype(np.float64)
    live = X > EPS32
    terms = np.where(live, X * np.log(np.where(live, X, 1.0) / np.maximum(V, EPS32)) - X, 0.0)
    e = 2.0 * (V.sum(axis=0) + terms.sum(axis=0))          # one term per frame
    return float(np.sqrt(max(float(e.sum()), 0.0)))


def learn(X, W0, H0, iters, check_every=10, tol=0.0, S=1, chunk=16, dtype=np.float64):
    """-> (W, H, n_iter, err): err[0] the error at the start, err[c] after check c (NaN where not evaluated)"""
    X = np.asarray(X, dtype=dtype)
    W = np.array(W0, dtype=dtype)
    H = np.array(H0, dtype=dtype)
    n_checks = iters // check_every if check_every > 0 else 0
    err = np.full(1 + n_checks, np.nan)
    if check_every > 0:
        err[0] = prev = error(X, W, H)
    n_iter = 0
    for it in range(1, iters + 1):
        H = update_h(X, W, H)
        W = update_w(X, W, H, S, chunk)
        n_iter = it
        if check_every <= 0 or it % check_every:
            continue
        c = it // check_every
        err[c] = e = error(X, W, H)
        if tol > 0 and (prev - e) / err[0] < tol:
            break
        prev = e
    return W, H, n_iter, err
