"""Sparse dictionary learning (evc_prox_learn) restated in numpy: the reference of the GPU tests for shapes without a recorded
fixture, itself checked against every recorded deComP run (tests/test_prox_learn_host.py).

deComP's orientation throughout (dictionary_learning.py:114-168): y is T x M, D is N x M with the atoms as rows, x is T x N.
A call with resume off divides every atom by its norm and zeroes S (N x N), Q (N x M) and count.  Epoch e takes
floor(T / bs) batches of bs frames in the order of order[e]; the last T mod bs frames of the row are left alone.  One step on
the frames F of a batch:
    lasso       x[F] <- prox_restatement.solve_one(y[F], D, alpha, x[F], lasso_tol, lasso_iters, ...) with normalize and the
                deComP stop, the batch as one utterance
    statistics  theta = count bs + 1;  beta = (theta - bs) / theta (double, cast to the dtype);
                S <- beta S + x_F^T x_F;  Q <- beta Q + x_F^T y_F
    sweep       for k ascending: u = (Q[k] - S[k] D_cur) / (S[k, k] + 1e-15) + d_k;  d_k <- u / sqrt(max(|u|^2, 1))
                written blocked and right-looking with nb = plearn_block(M, dtype) atoms per block, as the kernels run it:
                Rm = Q - S D once, inside a block r = Rm[k] - sum_{j < i, ascending} S[k, k0 + j] dD_j, behind a block
                Rm[rows] -= S[rows, K] dD (j ascending) - the same algorithm as deComP's left-looking loop, to rounding
    stop        stat = max |D - D_new| (a NaN wins and compares false);  D <- D_new;  count += 1;  stat < tol ends the call
"""
import numpy as np

import prox_restatement as pr

LDS_BYTES = 40 * 1024


def plearn_block(M, dtype):
    """atoms per block of the sweep: evc_prox_learn_plan.h's rule"""
    es = np.dtype(dtype).itemsize
    for nb in (32, 16, 8):
        if nb * M * es <= LDS_BYTES:
            return nb
    return 4


def decomp_order(T, epochs, seed):
    """the rows deComP's shuffles give: index shuffled in place and cumulatively, applied to the already shuffled frames"""
    rng = np.random.RandomState(seed)
    index, pos = np.arange(T), np.arange(T)
    rows = np.empty((max(epochs, 0), T), dtype=np.int32)
    for e in range(rows.shape[0]):
        rng.shuffle(index)
        pos = pos[index]
        rows[e] = pos
    return rows


def unit_atoms(D):
    return D / np.sqrt(np.sum(D * D, axis=-1, keepdims=True))


def sweep(S, Q, D, nb):
    """one blocked, right-looking pass over the atoms -> D_new"""
    N, M = D.shape
    dt = D.dtype.type
    jitter = dt(1e-15)
    Rm = Q - np.dot(S, D)
    Dn = D.copy()
    for k0 in range(0, N, nb):
        nbk = min(nb, N - k0)
        dD = np.zeros((nbk, M), dtype=D.dtype)
        for i in range(nbk):
            k = k0 + i
            r = Rm[k].copy()
            for j in range(i):
                r = r - S[k, k0 + j] * dD[j]
            u = r / (S[k, k] + jitter) + D[k]
            dn = u / np.sqrt(np.maximum(np.sum(u * u), dt(1)))
            dD[i] = dn - D[k]
            Dn[k] = dn
        for j in range(nbk):
            Rm[k0 + nbk:] = Rm[k0 + nbk:] - np.outer(S[k0 + nbk:, k0 + j], dD[j])
    return Dn


def solve(y, D, alpha, x0=None, *, batch_size, epochs, order=None, tol=0.0, lasso_iters=10, lasso_tol=1e-5, positive=True,
          momentum="fista", check_every=10, state=None, dtype=np.float64, nb=None, max_steps=None, cuts=None):
    """-> D (N x M), x (T x N), n_epochs, n_steps, trace (epochs * (T // bs) statistics, NaN after the stop), state =
    (S, Q, count).  state: that of an earlier call (resume): D is then taken as it is.  max_steps: the call ends after that
    many steps (the generator's fixed-count reruns of a run that stopped).  cuts: a dict that receives "pre" and "thr" (T x N):
    per frame, the last lasso update's value before the cut at 0 and its threshold (NaN for a frame no step took)."""
    y, D = np.asarray(y, dtype=dtype), np.array(D, dtype=dtype)
    T, (N, M) = y.shape[0], D.shape
    bs = int(batch_size)
    x = np.ones((T, N), dtype=dtype) if x0 is None else np.array(x0, dtype=dtype)
    nb = plearn_block(M, dtype) if nb is None else nb
    if state is None:
        D = unit_atoms(D)
        S, Q, count = np.zeros((N, N), dtype=dtype), np.zeros((N, M), dtype=dtype), 0
    else:
        S, Q, count = state[0].copy(), state[1].copy(), int(state[2])
    nbat = T // bs
    trace = np.full(epochs * nbat, np.nan)
    n_steps, n_epochs = 0, epochs
    if cuts is not None:
        cuts["pre"], cuts["thr"] = np.full((T, N), np.nan), np.full((T, N), np.nan)
    for e in range(epochs):
        row = np.arange(T) if order is None else np.asarray(order[e])
        for b in range(nbat):
            F = row[b * bs:(b + 1) * bs]
            if lasso_iters > 0:
                res = pr.solve_one(y[F], D, alpha, x[F], lasso_tol, lasso_iters, positive=positive, momentum=momentum,
                                   normalize=True, check_every=check_every, stop=True, want_pre=cuts is not None)
                x[F] = res[0]
                if cuts is not None:
                    cuts["pre"][F], cuts["thr"][F] = res[3], res[4]
            theta = float(count) * float(bs) + 1.0
            beta = np.dtype(dtype).type((theta - float(bs)) / theta)
            xF = x[F]
            S = beta * S + np.dot(xF.T, xF)
            Q = beta * Q + np.dot(xF.T, y[F])
            Dn = sweep(S, Q, D, nb)
            stat = np.max(np.abs(D - Dn))
            D = Dn
            count += 1
            trace[n_steps] = stat
            n_steps += 1
            if stat < tol or n_steps == max_steps:
                return D, x, e + 1, n_steps, trace, (S, Q, count)
    return D, x, n_epochs, n_steps, trace, (S, Q, count)


def problem(M, N, T, seed, signed=False, scale=1.0):
    """frames that a few of N hidden atoms explain and a start dictionary: y (T x M), D0 (N x M), deComP's orientation"""
    y, A = pr.problem(M, N, T, seed, signed=signed, active=min(3, N))
    rng = np.random.default_rng(seed + 77)
    D0 = A + 0.3 * (rng.standard_normal((N, M)) if signed else rng.random((N, M)))
    return y * scale, D0
