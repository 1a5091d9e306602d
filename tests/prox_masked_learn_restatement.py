"""Sparse dictionary learning with missing data (evc_prox_masked_learn) restated in numpy: the reference of the GPU tests for
shapes without a recorded fixture, itself checked against every recorded deComP run (tests/test_prox_masked_learn_host.py).

deComP's orientation throughout (dictionary_learning.py:171-231): y is T x M, D is N x M with the atoms as rows, x is T x N,
mask is T x M with weights >= 0.  A call with resume off divides every atom by its norm and zeroes S ([M][N][N]: one Gram
matrix per bin), Q (N x M) and count.  Epochs, batches and the frames left alone are prox_learn_restatement's.  One step on
the frames F of a batch:
    lasso       x[F] <- prox_masked_restatement.solve_one(y[F], D, mask[F], alpha, x[F], lasso_tol, lasso_iters, ...,
                lip_weights="mean") with normalize and the deComP stop, the batch as one utterance
    statistics  theta = count bs + 1;  beta = (theta - bs) / theta (double, cast to the dtype);
                S_m <- beta S_m + x_F^T diag(mask_F[:, m]) x_F for every bin m;  Q <- beta Q + x_F^T (mask_F . y_F)
    atoms       all from the OLD D (a Jacobi step, dictionary_learning.py:218):
                G[k, m] = sum_j S_m[k, j] D[j, m];  a_k = sum_m (S_m[k, k] + 1e-15), m ascending;
                u_k = (Q[k] - G[k]) / a_k + D[k];  D_new[k] = u_k / sqrt(max(|u_k|^2, 1))
    stop        stat = max |D - D_new| (a NaN wins and compares false);  D <- D_new;  count += 1;  stat < tol ends the call
"""
import numpy as np

import prox_learn_restatement as plr
import prox_masked_restatement as pmr

decomp_order = plr.decomp_order
unit_atoms = plr.unit_atoms
problem = plr.problem
problem_mask = pmr.problem_mask


def atoms(S, Q, D):
    """one Jacobi pass over the atoms -> D_new"""
    dt = D.dtype.type
    G = np.einsum("mkj,jm->km", S, D)
    diag = np.einsum("mkk->mk", S) + dt(1e-15)
    a = np.zeros(D.shape[0], dtype=D.dtype)
    for m in range(S.shape[0]):
        a = a + diag[m]
    u = (Q - G) / a[:, None] + D
    return u / np.sqrt(np.maximum(np.sum(u * u, axis=1, keepdims=True), dt(1)))


def solve(y, D, alpha, x0=None, *, mask, batch_size, epochs, order=None, tol=0.0, lasso_iters=10, lasso_tol=1e-5, positive=True,
          momentum="fista", check_every=10, state=None, dtype=np.float64, max_steps=None, cuts=None):
    """-> D (N x M), x (T x N), n_epochs, n_steps, trace (epochs * (T // bs) statistics, NaN after the stop), state =
    (S, Q, count) with S [M][N][N].  state, max_steps and cuts as prox_learn_restatement.solve has them."""
    y, D, mask = np.asarray(y, dtype=dtype), np.array(D, dtype=dtype), np.asarray(mask, dtype=dtype)
    T, (N, M) = y.shape[0], D.shape
    bs = int(batch_size)
    x = np.ones((T, N), dtype=dtype) if x0 is None else np.array(x0, dtype=dtype)
    if state is None:
        D = unit_atoms(D)
        S, Q, count = np.zeros((M, N, N), dtype=dtype), np.zeros((N, M), dtype=dtype), 0
    else:
        S, Q, count = state[0].copy(), state[1].copy(), int(state[2])
    nbat = T // bs
    trace = np.full(epochs * nbat, np.nan)
    n_steps, n_epochs = 0, epochs
    if cuts is not None:
        cuts["pre"], cuts["thr"] = np.full((T, N), np.nan), np.full((T, N), np.nan)
    with np.errstate(invalid="ignore", divide="ignore"):
        for e in range(epochs):
            row = np.arange(T) if order is None else np.asarray(order[e])
            for b in range(nbat):
                F = row[b * bs:(b + 1) * bs]
                if lasso_iters > 0:
                    res = pmr.solve_one(y[F], D, mask[F], alpha, x[F], lasso_tol, lasso_iters, positive=positive,
                                        momentum=momentum, normalize=True, check_every=check_every, stop=True,
                                        lip_weights="mean", want_pre=cuts is not None)
                    x[F] = res[0]
                    if cuts is not None:
                        cuts["pre"][F], cuts["thr"][F] = res[3], res[4]
                theta = float(count) * float(bs) + 1.0
                beta = np.dtype(dtype).type((theta - float(bs)) / theta)
                xF, wF = x[F], mask[F]
                S = beta * S + np.stack([np.dot((xF * wF[:, m:m + 1]).T, xF) for m in range(M)])
                Q = beta * Q + np.dot(xF.T, wF * y[F])
                Dn = atoms(S, Q, D)
                stat = np.max(np.abs(D - Dn))
                D = Dn
                count += 1
                trace[n_steps] = stat
                n_steps += 1
                if stat < tol or n_steps == max_steps:
                    return D, x, e + 1, n_steps, trace, (S, Q, count)
    return D, x, n_epochs, n_steps, trace, (S, Q, count)
