"""Missing-data multiplicative updates of the activations (evc_mu_masked_solve) restated in numpy, utterance by utterance: the
reference of the GPU tests, itself checked bit for bit against every recorded deComP run (tests/test_mu_masked_host.py).

deComP's orientation throughout (frame-major): y is T x M, D is N x M with the exemplars as rows, x is T x N, mask is T x M,
weights >= 0 of every bin of every frame (0: the bin is missing; None: no mask).  With J = 1e-15 (deComP's _JITTER), per
update (Likelihood.update_x, decomp/nmf_methods/grads.py:77-84, 108-115, 143-150):
    l2:  f = (x D) mask;   Num = (y mask) D^T;         Den = f D^T
    kl:  f = x D + J;      Num = ((y mask) / f) D^T;   Den = mask D^T        (no mask: the column sums of D^T)
    x <- x * max(Num, 0) / max(Den, J)
Every operation is written in deComP's order, so float64 runs reproduce it to the last bit.  The error and the stop rule are
evc_mu_masked_solve's own (deComP has no fixed-dictionary surface): per utterance, with V = x D (kl: + J),
    l2:  sqrt(sum mask (y - V)^2)        kl:  sqrt(2 max(sum mask (y log(y / V) - y + V), 0)),  terms with y = 0: mask V
at the start and after every `check_every` updates; the utterance stops at a check when (err_prev - err) / err_start < tol.

`learn` restates deComP's nmf.solve(method='mu') itself (decomp/nmf.py:52-80, nmf_methods/batch_mu.py, utils/normalize.py
l2_strict): the start dictionary normalised, then per iteration update_x, update_d with the new x, the normalisation and
the statistic max |D - D_new| - evc_mu_masked_learn's reference."""
import zlib

import numpy as np

J = 1.0e-15
LOSSES = ("l2", "kl")


def problem(M, N, T, seed, active=6):
    """non-negative data that a few of N exemplars (rows) explain, in deComP's orientation: y (T x M), D (N x M); no frame of y
    and no exemplar is all zero"""
    rng = np.random.default_rng(seed)
    D = rng.random((N, M)) + 0.05
    Hs = rng.random((T, N)) * (rng.random((T, N)) < min(1.0, active / N))
    if T > 0:
        Hs[np.arange(T), np.arange(T) % N] += 0.5
    y = Hs @ D + 0.01 * np.abs(rng.standard_normal((T, M)))
    return y, D


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


def update_x(y, x, d, mask, loss):
    """one multiplicative update of the activations, in deComP's order of operations"""
    if loss == "l2":
        if mask is None:
            f = x.dot(d)
            num, den = y.dot(d.T), f.dot(d.T)
        else:
            f = x.dot(d) * mask
            ym = y * mask
            num, den = ym.dot(d.T), f.dot(d.T)
    elif loss == "kl":
        f = x.dot(d) + J
        if mask is None:
            num, den = (y / f).dot(d.T), d.T.sum(axis=0, keepdims=True)
        else:
            ym = y * mask
            num, den = (ym / f).dot(d.T), mask.dot(d.T)
    else:
        raise ValueError(loss)
    return x * np.maximum(num, 0.0) / np.maximum(den, J)


def error(y, x, d, mask, loss):
    """the error of one utterance, summed in float64"""
    v = x.dot(d).astype(np.float64)
    y = y.astype(np.float64)
    w = np.ones_like(y) if mask is None else mask.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        if loss == "l2":
            return float(np.sqrt(np.sum(w * np.square(y - v))))
        vj = v + J
        terms = np.where(y > 0.0, y * np.log(np.where(y > 0.0, y, 1.0) / vj) - y + vj, vj)
        total = np.sum(w * terms)
        return float(np.sqrt(2.0 * (total if not total < 0.0 else 0.0)))


def n_slots(iters, check_every):
    return 1 + (iters // check_every if check_every > 0 else 0)


def solve_one(y, d, mask, x, loss, iters, check_every=0, tol=0.0, stop=True):
    """one utterance -> x, n_iter, trace (n_slots errors, NaN where not evaluated)"""
    trace = np.full(n_slots(iters, check_every), np.nan)
    n_iter = iters
    with np.errstate(divide="ignore", invalid="ignore"):
        if check_every > 0:
            trace[0] = e0 = eprev = error(y, x, d, mask, loss)
        for it in range(1, iters + 1):
            x = update_x(y, x, d, mask, loss)
            if check_every > 0 and it % check_every == 0:
                e = trace[it // check_every] = error(y, x, d, mask, loss)
                if stop and (eprev - e) / e0 < tol:
                    n_iter = it
                    break
                eprev = e
    return x, n_iter, trace


def solve(y, D, x0=None, *, mask=None, loss="l2", iters=100, check_every=0, tol=0.0, stop=True, utt_offsets=None,
          dtype=np.float64):
    """-> x (T x N), n_iter (updates applied per utterance), trace (n_utt x slots).  One solve_one per utterance; an empty
    utterance: n_iter = iters, all NaN.  x0 None starts at ones (deComP's default).  dtype=np.float32 runs every operation of
    the update in float32."""
    y, D = np.asarray(y, dtype=dtype), np.asarray(D, dtype=dtype)
    mask = None if mask is None else np.asarray(mask, dtype=dtype)
    T, N = y.shape[0], D.shape[0]
    x = np.ones((T, N), dtype=dtype) if x0 is None else np.array(x0, dtype=dtype)
    offs = [0, T] if utt_offsets is None else list(utt_offsets)
    n_iter = np.full(len(offs) - 1, iters, dtype=np.int32)
    trace = np.full((len(offs) - 1, n_slots(iters, check_every)), np.nan)
    for u in range(len(offs) - 1):
        t0, t1 = offs[u], offs[u + 1]
        if t0 == t1:
            continue
        x[t0:t1], n_iter[u], trace[u] = solve_one(y[t0:t1], D, None if mask is None else mask[t0:t1], x[t0:t1], loss, iters,
                                                  check_every, tol, stop)
    return x, n_iter, trace


def stop_margin(trace, tol):
    """the smallest distance of a stop statistic (err_prev - err) / err_start from `tol`, over the rows of `trace` (inf: no check)"""
    best = np.inf
    for row in np.atleast_2d(trace):
        e = row[np.isfinite(row)]
        if len(e) > 1:
            best = min(best, float(np.min(np.abs((e[:-1] - e[1:]) / e[0] - tol))))
    return best


def blas_fingerprint(y, D, mask):
    """CRC-32 of the matrix products one float64 update multiplies (x D, (y mask) D^T, ((x D) mask) D^T, mask D^T) from a start
    of ones.  numpy hands them to the machine's BLAS, whose summation order depends on the processor and the thread count: a
    recorded run can be reproduced to the last bit only where these agree with the recording machine's."""
    y, D, mask = (np.asarray(m, dtype=np.float64) for m in (y, D, mask))
    f = np.ones((y.shape[0], D.shape[0])).dot(D)
    return [zlib.crc32(np.ascontiguousarray(m).tobytes()) for m in (f, (y * mask).dot(D.T), (f * mask).dot(D.T), mask.dot(D.T))]


def permutation_figure(y, D, mask, K, dtype, loss="l2", x0=None, seed=5, floor=True):
    """how far the restatement's result moves, relative to max |x|, when the exemplars AND the bins are summed in another
    order (the factored sweep sums over both) - and at least K eps for K updates"""
    rng = np.random.default_rng(seed)
    pn, pm = rng.permutation(D.shape[0]), rng.permutation(D.shape[1])
    base = solve(y, D, x0, mask=mask, loss=loss, iters=K, dtype=dtype)[0].astype(np.float64)
    moved = solve(y[:, pm], D[pn][:, pm], None if x0 is None else x0[:, pn], mask=None if mask is None else mask[:, pm],
                  loss=loss, iters=K, dtype=dtype)[0].astype(np.float64)
    back = np.empty_like(moved)
    back[:, pn] = moved
    good = np.isfinite(base)
    top = np.max(np.abs(base[good])) if good.any() else 0.0
    fig = float(np.max(np.abs(back[good] - base[good])) / top) if top > 0 else 0.0
    return max(fig, K * float(np.finfo(dtype).eps)) if floor else fig


def l2_strict(U):
    """every row divided by its Euclidean norm (deComP utils/normalize.py; a zero row becomes NaN)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return U / np.sqrt(np.sum(U * U, axis=-1, keepdims=True))


def update_d(y, x, d, mask, loss):
    """one multiplicative update of the dictionary, in deComP's order of operations"""
    if loss == "l2":
        if mask is None:
            f = x.dot(d)
            num, den = x.T.dot(y), x.T.dot(f)
        else:
            f = x.dot(d) * mask
            ym = y * mask
            num, den = x.T.dot(ym), x.T.dot(f)
    elif loss == "kl":
        f = x.dot(d) + J
        if mask is None:
            num, den = x.T.dot(y / f), x.T.sum(axis=1, keepdims=True)
        else:
            ym = y * mask
            num, den = x.T.dot(ym / f), x.T.dot(mask)
    else:
        raise ValueError(loss)
    return d * np.maximum(num, 0.0) / np.maximum(den, J)


def learn(y, D, x0=None, *, mask=None, loss="l2", tol=1e-3, maxiter=1000, dtype=np.float64):
    """deComP's nmf.solve(y, D, x0, tol, maxiter=maxiter, method='mu', likelihood=loss, mask=mask) -> it, D, x, stats: `it` as
    deComP returns it (the iteration that stopped, else maxiter), stats[k] = max |D - D_new| of iteration k + 1"""
    y, D = np.asarray(y, dtype=dtype), np.asarray(D, dtype=dtype)
    mask = None if mask is None else np.asarray(mask, dtype=dtype)
    x = np.ones((y.shape[0], D.shape[0]), dtype=dtype) if x0 is None else np.array(x0, dtype=dtype)
    D = l2_strict(D)
    stats = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for it in range(1, maxiter):
            x = update_x(y, x, D, mask, loss)
            D_new = l2_strict(update_d(y, x, D, mask, loss))
            stats.append(float(np.max(np.abs(D - D_new))))
            if stats[-1] < tol:
                return it, D_new, x, np.array(stats)
            D = D_new
    return maxiter, D, x, np.array(stats)


def learn_permutation_figure(y, D, mask, K, dtype, loss="l2", x0=None, seed=5, floor=True):
    """how far K iterations of `learn` move, relative to max |D| and max |x| (the larger of the two figures), when the atoms,
    the bins AND the frames are summed in another order - and at least K eps"""
    rng = np.random.default_rng(seed)
    pn, pm, pt = rng.permutation(D.shape[0]), rng.permutation(D.shape[1]), rng.permutation(y.shape[0])
    _, Db, xb, _ = learn(y, D, x0, mask=mask, loss=loss, tol=0.0, maxiter=K + 1, dtype=dtype)
    _, Dm, xm, _ = learn(y[pt][:, pm], D[pn][:, pm], None if x0 is None else x0[pt][:, pn],
                         mask=None if mask is None else mask[pt][:, pm], loss=loss, tol=0.0, maxiter=K + 1, dtype=dtype)
    Dback, xback = np.empty_like(Dm), np.empty_like(xm)
    Dback[np.ix_(pn, pm)] = Dm
    xback[np.ix_(pt, pn)] = xm
    fig = 0.0
    for b, m in ((Db, Dback), (xb, xback)):
        b, m = b.astype(np.float64), m.astype(np.float64)
        good = np.isfinite(b)
        top = np.max(np.abs(b[good])) if good.any() else 0.0
        if top > 0:
            fig = max(fig, float(np.max(np.abs(m[good] - b[good])) / top))
    return max(fig, K * float(np.finfo(dtype).eps)) if floor else fig
