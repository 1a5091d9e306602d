"""numpy restatement of evc_deconv_learn (include/evc.h): convolutive NMF, X ~ sum_tau W_tau shift_tau(H), both factors by
multiplicative updates, bin-major throughout (W (L, M, R), X (M, T), H (R, T)), float64.  The activation half is
deconv_restatement.update utterance by utterance; the dictionary half updates every tap from the same V.  With L = 1 it is
scikit-learn's _fit_multiplicative_update with update_H=True (tests/golden/dict{mu,kl}_sk_*.npz)."""
import numpy as np

import deconv_restatement as dr

EPS = dr.EPS


def _offs(offs, T):
    return [0, T] if offs is None else [int(v) for v in offs]


def shifted(H, tau, offs=None):
    """Hs[r, t] = H[r, t - tau] where t - tau lies in t's utterance, else 0"""
    Hs = np.zeros_like(H)
    o = _offs(offs, H.shape[1])
    for a, b in zip(o[:-1], o[1:]):
        if b - a > tau:
            Hs[:, a + tau:b] = H[:, a:b - tau]
    return Hs


def model(W, H, offs=None):
    """V[:, t] = sum_tau W_tau Hs_tau[:, t]"""
    V = np.zeros((W.shape[1], H.shape[1]))
    for tau in range(W.shape[0]):
        V += W[tau] @ shifted(H, tau, offs)
    return V


def dict_step(W, X, H, loss, offs=None):
    """the dictionary half: every tap from the same V; returns the new W"""
    V = model(W, H, offs)
    out = np.empty_like(W)
    Q = X / np.maximum(V, EPS) if loss != "frobenius" else None
    for tau in range(W.shape[0]):
        Hs = shifted(H, tau, offs)
        if loss == "frobenius":
            num, den = X @ Hs.T, V @ Hs.T
            den[den == 0] = EPS
        else:
            num, s = Q @ Hs.T, Hs.sum(axis=1)
            s[s == 0] = 1.0
            den = s[None, :]
        out[tau] = W[tau] * (num / den)
    return out


def act_step(W, X, H, loss, offs=None, l1=0.0, l2=0.0):
    """the activation half: one iteration of evc_deconv_solve's statement per utterance; returns the new H"""
    out = H.copy()
    o = _offs(offs, H.shape[1])
    for a, b in zip(o[:-1], o[1:]):
        if b > a:
            out[:, a:b] = dr.update(W, X[:, a:b], H[:, a:b], loss, l1, l2)
    return out


def error(W, X, H, loss, offs=None):
    """one value for the call: ||X - V||_F or sqrt(2 KL(X || V))"""
    return dr.error(X, model(W, H, offs), loss)


def learn(W, X, H, loss, iters, offs=None, check_every=0, tol=0.0, update="both", l1_h=0.0, l2_h=0.0):
    """(W, H, n_iter, trace[1 + iters // check_every]) from the start (W, H)"""
    loss = "frobenius" if loss == "frobenius" else "kl"
    W, X, H = (np.array(a, dtype=np.float64) for a in (W, X, H))
    trace = np.full(1 + (iters // check_every if check_every > 0 else 0), np.nan)
    err0 = prev = None
    if check_every > 0:
        err0 = prev = trace[0] = error(W, X, H, loss, offs)
    n_iter = 0
    for it in range(1, iters + 1):
        if update == "both":
            H = act_step(W, X, H, loss, offs, l1_h, l2_h)
        W = dict_step(W, X, H, loss, offs)
        n_iter = it
        if check_every > 0 and it % check_every == 0:
            err = trace[it // check_every] = error(W, X, H, loss, offs)
            if tol > 0 and (prev - err) / err0 < tol:
                break
            prev = err
    return W, H, n_iter, trace


def problem(M, R, T, L, offs=None, seed=0):
    """the inputs of tests/test_gpu_deconv_learn.py: X = V(W*, H*) + 1e-6 from a sparse H*, and a random positive start"""
    rng = np.random.default_rng(seed)
    Ws = rng.random((L, M, R)) + 1e-3
    Hs = rng.random((R, T)) * (rng.random((R, T)) < min(1.0, 4.0 / R))
    X = model(Ws, Hs, offs) + 1e-6
    return X, rng.random((L, M, R)) + 0.1, rng.random((R, T)) + 0.1
