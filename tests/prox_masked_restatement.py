"""Missing-data sparse activations (evc_prox_masked_solve) restated in numpy, utterance by utterance: the reference of the GPU
tests for shapes without a recorded fixture, itself checked bit for bit against every recorded deComP run
(tests/test_prox_masked_host.py).

deComP's orientation throughout (frame-major): y is T x M, A is N x M with the exemplars as rows, x is T x N, mask is T x M,
weights >= 0 of every bin of every frame (0: the bin is missing).
    min_x 1/2 sum_m mask_m (y_m - (x A)_m)^2 + sum_n lambda_n x_n,   x >= 0 (positive) or signed
With normalize (deComP, lasso.py:120-189): d = sqrt(sum(A^2, -1)) from the unmasked A; A <- A / d; tol_n = tol d; the start
is multiplied by d and the result divided by it; lambda_tn = alpha / d_n * cnt_t with cnt_t = sum_m mask_tm.  Without:
lambda = alpha, tol_n = tol.  wbar = the mean of the mask over the utterance's frames (lip_weights "mean", deComP,
lasso.py:317) or its maximum ("max": an upper bound of every frame's curvature); s = 1 / max_n sum_k |(A wbar) A^T|_kn, or
1 / lipschitz; thr = s lambda; P = (y mask) A^T.  Per iteration i, W_0 = x_0 (lasso.py:259-271):
    V = W + s (P - ((W A) mask) A^T);  x_new = threshold(V, thr);  W' = x_new + c_i (x_new - x_old)
Schedules, checks and the stop are prox_restatement's.  mask None is prox_restatement itself (the Gram form).  Every
operation is written in deComP's order, so float64 runs reproduce it to the last bit."""
import zlib

import numpy as np

import prox_restatement as pr

LIP_WEIGHTS = ("mean", "max")


def problem_mask(T, M, seed, kind="binary", keep=0.7):
    """a mask of float32-representable weights: "binary" keeps a bin with probability `keep`, "weights" draws uniform
    weights in [0, 1) and zeroes one bin in ten.  The first frame always has a zero and a non-zero (M = 1: the first two
    frames)."""
    rng = np.random.default_rng(seed + 7000)
    if kind == "binary":
        mask = (rng.random((T, M)) < keep).astype(np.float64)
    elif kind == "weights":
        mask = rng.random((T, M)).astype(np.float32).astype(np.float64) * (rng.random((T, M)) < 0.9)
    else:
        raise ValueError(kind)
    if T > 0 and M > 1:
        mask[0, 0], mask[0, 1] = 0.0, 1.0
    elif T > 1:
        mask[0, 0], mask[1, 0] = 0.0, 1.0
    return mask


def prepare(y, A, mask, alpha, tol, x, normalize, lipschitz, lip_weights):
    """-> P, A (scaled), s, thr, tol_n, x (scaled), d: what the iteration needs, in deComP's order of operations
    (lasso.py:123-131, 163, 317-321)"""
    if lip_weights not in LIP_WEIGHTS:
        raise ValueError(lip_weights)
    if normalize:
        d = np.sqrt(np.sum(np.square(A), axis=-1))
        A = A / np.expand_dims(d, axis=-1)
        alpha = alpha / d
        tol = tol * d
        x = x * d
        alpha = alpha * np.sum(mask, axis=-1, keepdims=True)
    else:
        d = None
    At = A.T
    with np.errstate(divide="ignore", invalid="ignore"):
        if lipschitz:
            s = np.asarray([1.0 / lipschitz], dtype=A.dtype)
        else:
            wbar = np.mean(mask, 0) if lip_weights == "mean" else np.max(mask, 0)
            G = np.dot(A * wbar, At)
            s = 1.0 / np.max(np.sum(np.abs(G), axis=-2), axis=-1, keepdims=True)
        thr = s * alpha
    P = np.tensordot(y * mask, At, axes=1)
    return P, A, s, thr, tol, x, d


def lipschitz_of(A, mask, normalize=True, lip_weights="mean"):
    """the bound L the restatement uses for one utterance"""
    A, mask = np.asarray(A, dtype=np.float64), np.asarray(mask, dtype=np.float64)
    s = prepare(np.zeros_like(mask), A, mask, 0.0, 0.0, np.zeros((mask.shape[0], A.shape[0])), normalize, None, lip_weights)[2]
    return float(1.0 / s[0])


def blas_fingerprint(y, A, mask):
    """CRC-32 of the matrix products of a normalised float64 masked solve - the weighted Gram matrix, P, P A and (P A) A^T,
    the shapes every iteration multiplies.  numpy hands them to the machine's BLAS, whose summation order depends on the
    processor and the thread count: a recorded run can be reproduced to the last bit only where these agree with the
    recording machine's."""
    y, A, mask = (np.asarray(m, dtype=np.float64) for m in (y, A, mask))
    P, As, _, _, _, _, _ = prepare(y, A, mask, 1e-3, 0.0, np.zeros((y.shape[0], A.shape[0])), True, None, "mean")
    G = np.dot(As * np.mean(mask, 0), As.T)
    R = np.tensordot(P, As, axes=1)
    return [zlib.crc32(np.ascontiguousarray(m).tobytes()) for m in (G, P, R, np.tensordot(R * mask, As.T, axes=1))]


def solve_one(y, A, mask, alpha, x, tol, iters, *, positive=True, momentum="fista", normalize=True, check_every=10, stop=True,
              lipschitz=None, lip_weights="mean", want_pre=False):
    """one utterance -> x, n_iter, trace (n_slots statistics, NaN where not evaluated)"""
    if mask is None:
        return pr.solve_one(y, A, alpha, x, tol, iters, positive=positive, momentum=momentum, normalize=normalize,
                            check_every=check_every, stop=stop, lipschitz=lipschitz, want_pre=want_pre)
    P, A, s, thr, tol_n, x, d = prepare(y, A, mask, alpha, tol, x, normalize, lipschitz, lip_weights)
    At = A.T
    cs = pr.schedule(momentum, iters)
    trace = np.full(pr.n_slots(iters, check_every), np.nan)
    w, n_iter, pre = x, iters, None
    with np.errstate(invalid="ignore"):
        for i in range(iters):
            v = w + s * (P - np.tensordot(np.tensordot(w, A, axes=1) * mask, At, axes=1))
            pre = (v - thr) if positive else (np.abs(v) - thr)
            x_new = pr._threshold(v, thr, positive)
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


def solve(y, A, alpha, x0=None, *, mask=None, tol=1e-3, iters=1000, positive=True, momentum="fista", normalize=True,
          check_every=10, stop=True, lipschitz=None, lip_weights="mean", utt_offsets=None, dtype=np.float64):
    """-> x (T x N), n_iter (updates applied per utterance), trace (n_utt x slots).  One solve_one per utterance - wbar, the
    step and the stop statistic are the utterance's own; an empty utterance: n_iter = iters, all NaN.  dtype=np.float32 runs
    every operation in float32."""
    y, A = np.asarray(y, dtype=dtype), np.asarray(A, dtype=dtype)
    mask = None if mask is None else np.asarray(mask, dtype=dtype)
    T, N = y.shape[0], A.shape[0]
    x = np.zeros((T, N), dtype=dtype) if x0 is None else np.array(x0, dtype=dtype)
    offs = [0, T] if utt_offsets is None else list(utt_offsets)
    n_iter = np.full(len(offs) - 1, iters, dtype=np.int32)
    trace = np.full((len(offs) - 1, pr.n_slots(iters, check_every)), np.nan)
    if iters == 0:
        return x, n_iter, trace
    for u in range(len(offs) - 1):
        t0, t1 = offs[u], offs[u + 1]
        if t0 == t1:
            continue
        x[t0:t1], n_iter[u], trace[u] = solve_one(y[t0:t1], A, None if mask is None else mask[t0:t1], alpha, x[t0:t1], tol,
                                                  iters, positive=positive, momentum=momentum, normalize=normalize,
                                                  check_every=check_every, stop=stop, lipschitz=lipschitz,
                                                  lip_weights=lip_weights)
    return x, n_iter, trace


def permutation_figure(y, A, mask, K, dtype, x0=None, seed=5, floor=True, **kw):
    """how far the restatement's result moves, relative to max |x|, when the exemplars AND the bins are summed in another
    order (the factored sweep sums over both) - and at least K eps for K updates"""
    kw = dict(kw, iters=K, stop=False, dtype=dtype)
    kw.pop("utt_offsets", None)
    rng = np.random.default_rng(seed)
    pn, pm = rng.permutation(A.shape[0]), rng.permutation(A.shape[1])
    base = solve(y, A, x0=x0, mask=mask, **kw)[0].astype(np.float64)
    moved = solve(y[:, pm], A[pn][:, pm], x0=None if x0 is None else x0[:, pn], mask=None if mask is None else mask[:, pm],
                  **kw)[0].astype(np.float64)
    back = np.empty_like(moved)
    back[:, pn] = moved
    good = np.isfinite(base)
    top = np.max(np.abs(base[good])) if good.any() else 0.0
    fig = float(np.max(np.abs(back[good] - base[good])) / top) if top > 0 else 0.0
    return max(fig, K * float(np.finfo(dtype).eps)) if floor else fig
