"""Sparse activations by proximal gradient (evc_prox_solve) restated in numpy, utterance by utterance: the reference of the
GPU tests for shapes without a recorded fixture, itself checked bit for bit against every recorded deComP run
(tests/test_prox_host.py).

deComP's orientation throughout (frame-major): y is T x M, A is N x M with the exemplars as rows, x is T x N.
    min_x 1/2 ||y - x A||^2 + sum_n lambda_n x_n,   x >= 0 (positive) or signed
With normalize (deComP): d = sqrt(sum(A^2, -1)); A <- A / d; lambda = alpha / d * M; tol_n = tol d; the start is multiplied
by d and the result divided by it.  Without: lambda = alpha, tol_n = tol.  G = A A^T, P = y A^T, s = 1 / max_n sum_k |G_kn|
(or 1 / lipschitz), thr = s lambda.  Per iteration i, W_0 = x_0:
    V = W + s (P - W G);  x_new = max(V - thr, 0) | max(|V| - thr, 0) sign(V);  W' = x_new + c_i (x_new - x_old)
c_i: 0 ("ista"), (beta_i - 1) / beta_(i+1) ("fista"), i / (i + 3) ("nesterov").  At i % check_every == 0 the statistic
max(|x_new - x_old| - tol_n) is recorded and, under the "decomp" rule, a negative one stops the utterance with x_new; n_iter
is the number of updates applied (deComP's `it` + 1).  Every operation is written in deComP's order, so float64 runs
reproduce it to the last bit."""
import zlib

import numpy as np

MOMENTA = ("ista", "fista", "nesterov")


def schedule(momentum, iters):
    """the momentum coefficients c_0 .. c_(iters-1) as Python floats (double precision)"""
    if momentum not in MOMENTA:
        raise ValueError(momentum)
    out, beta = [], 1.0
    for i in range(iters):
        if momentum == "ista":
            out.append(0.0)
        elif momentum == "nesterov":
            out.append(i / (i + 3))
        else:
            beta_new = 0.5 * (1.0 + float(np.sqrt(1.0 + 4.0 * beta * beta)))
            out.append((beta - 1.0) / beta_new)
            beta = beta_new
    return out


def n_slots(iters, check_every):
    return (iters - 1) // check_every + 1 if (check_every > 0 and iters > 0) else 0


def problem(M, N, T, seed, signed=False, active=6):
    """a dictionary of N exemplars (rows), frames that a few of them explain, in deComP's orientation: y (T x M), A (N x M)"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((N, M)) if signed else rng.random((N, M)) + 0.05
    Hs = rng.random((T, N)) * (rng.random((T, N)) < min(1.0, active / N))
    if signed:
        Hs = Hs * rng.choice([-1.0, 1.0], size=Hs.shape)
    y = Hs @ A + 0.01 * rng.standard_normal((T, M))
    return y, A


def _threshold(v, thr, positive):
    if positive:
        return np.maximum(v - thr, 0.0)
    return np.maximum(np.abs(v) - thr, 0.0) * np.sign(v)


def prepare(y, A, alpha, tol, x, normalize, lipschitz):
    """-> P, G, s, thr, tol_n, x (scaled), d: what the iteration needs, in deComP's order of operations (lasso.py:123-146)"""
    M = A.shape[-1]
    if normalize:
        d = np.sqrt(np.sum(np.square(A), axis=-1))
        A = A / np.expand_dims(d, axis=-1)
        alpha = alpha / d
        tol = tol * d
        x = x * d
        alpha = alpha * M
    else:
        d = None
    At = A.T
    G = np.dot(A, At)
    if lipschitz:
        s = np.asarray([1.0 / lipschitz], dtype=A.dtype)
    else:
        s = 1.0 / np.max(np.sum(np.abs(G), axis=-2), axis=-1, keepdims=True)
    thr = s * alpha
    P = np.tensordot(y, At, axes=1)
    return P, G, s, thr, tol, x, d


def blas_fingerprint(y, A):
    """CRC-32 of the three matrix products of a normalised float64 solve - G, P and P G, the shapes every iteration
    multiplies.  numpy hands them to the machine's BLAS, whose summation order depends on the processor and the thread
    count: a recorded run can be reproduced to the last bit only where these agree with the recording machine's."""
    y, A = np.asarray(y, dtype=np.float64), np.asarray(A, dtype=np.float64)
    P, G, _, _, _, _, _ = prepare(y, A, 1e-3, 0.0, np.zeros((y.shape[0], A.shape[0])), True, None)
    return [zlib.crc32(np.ascontiguousarray(m).tobytes()) for m in (G, P, np.tensordot(P, G, axes=1))]


def solve_one(y, A, alpha, x, tol, iters, *, positive=True, momentum="fista", normalize=True, check_every=10, stop=True,
              lipschitz=None, want_pre=False):
    """one utterance -> x, n_iter, trace (n_slots statistics, NaN where not evaluated)"""
    P, G, s, thr, tol_n, x, d = prepare(y, A, alpha, tol, x, normalize, lipschitz)
    cs = schedule(momentum, iters)
    trace = np.full(n_slots(iters, check_every), np.nan)
    w, n_iter, pre = x, iters, None
    for i in range(iters):
        v = w + s * (P - np.tensordot(w, G, axes=1))
        pre = (v - thr) if positive else (np.abs(v) - thr)
        x_new = _threshold(v, thr, positive)
        if check_every > 0 and i % check_every == 0:
            stat = trace[i // check_every] = np.max(np.abs(x_new - x) - tol_n)
            if stop and stat < 0.0:
                x, n_iter = x_new, i + 1
                break
        w = x_new if momentum == "ista" else x_new + x.dtype.type(cs[i]) * (x_new - x)
        x = x_new
    out = x / d if normalize else x
    if want_pre:
        return out, n_iter, trace, pre, np.broadcast_to(thr, x.shape)
    return out, n_iter, trace


def solve(y, A, alpha, x0=None, *, tol=1e-3, iters=1000, positive=True, momentum="fista", normalize=True, check_every=10,
          stop=True, lipschitz=None, utt_offsets=None, dtype=np.float64):
    """-> x (T x N), n_iter (updates applied per utterance), trace (n_utt x slots).  One solve_one per utterance; an empty
    utterance: n_iter = iters, all NaN.  dtype=np.float32 runs every operation in float32."""
    y, A = np.asarray(y, dtype=dtype), np.asarray(A, dtype=dtype)
    T, N = y.shape[0], A.shape[0]
    x = np.zeros((T, N), dtype=dtype) if x0 is None else np.array(x0, dtype=dtype)
    offs = [0, T] if utt_offsets is None else list(utt_offsets)
    n_iter = np.full(len(offs) - 1, iters, dtype=np.int32)
    trace = np.full((len(offs) - 1, n_slots(iters, check_every)), np.nan)
    if iters == 0:
        return x, n_iter, trace
    for u in range(len(offs) - 1):
        t0, t1 = offs[u], offs[u + 1]
        if t0 == t1:
            continue
        x[t0:t1], n_iter[u], trace[u] = solve_one(y[t0:t1], A, alpha, x[t0:t1], tol, iters, positive=positive,
                                                  momentum=momentum, normalize=normalize, check_every=check_every, stop=stop,
                                                  lipschitz=lipschitz)
    return x, n_iter, trace


def method_of(positive, momentum):
    """deComP's method name"""
    return {"ista": "ista", "fista": "fista", "nesterov": "acc_ista"}[momentum] + ("_pos" if positive else "")


def split_method(method):
    """deComP's method name -> (positive, momentum)"""
    positive = method.endswith("_pos")
    base = method[:-4] if positive else method
    return positive, {"ista": "ista", "fista": "fista", "acc_ista": "nesterov"}[base]
