"""numpy restatement of the alternating coordinate descent that evc_cd_learn runs.

scikit-learn's solver='cd' with update_H=True (_fit_coordinate_descent, shuffle=False) alternates two calls of
_update_coordinate_descent per iteration.  In the library's names (X is T x M frames as rows, H is T x R, the dictionary W
is M x R with one ROW per bin):
  activations  one sweep of tests/cd_restatement.cd_iterations from the current H (blocked, residual form);
  dictionary   G = H^T H + l2 I (R x R) and P = X^T H - l1 (M x R), both summed over S contiguous frame ranges whose
               partial sums are added in ascending order; then, for every bin row w, the components in blocks of 16:
               the block's 16 gradients G[t, :] . w - P[m, t] at the block's start, 16 in-order steps
               w_t <- max(w_t - grad / G[t, t], 0) (skipped where G[t, t] == 0) that correct the block's later
               gradients with the diagonal block of G.
The iteration's violation is the sum of the two halves' sums of |projected gradient|; sklearn's rule stops the loop.
Same coordinate order as sklearn, only the rounding differs.
"""
import numpy as np

from cd_restatement import cd_iterations

B = 16


def split_sum(L, Rm, S):
    """C = L^T Rm with the frames (rows) cut into S contiguous ranges [s T / S, (s + 1) T / S), the ranges' partial
    sums added in ascending order"""
    T = L.shape[0]
    acc = np.zeros((L.shape[1], Rm.shape[1]), dtype=L.dtype)
    for s in range(S):
        tb, te = s * T // S, (s + 1) * T // S
        acc = acc + L[tb:te].T @ Rm[tb:te]
    return acc


def dict_sweep(X, H, W, l1=0.0, l2=0.0, S=1):
    """One sweep over every row of W (M x R), in place.  X: (T, M), H: (T, R).  Returns the violation (float64)."""
    dt = W.dtype.type
    R = W.shape[1]
    G = split_sum(H, H, S)
    G[np.arange(R), np.arange(R)] += dt(l2)
    P = split_sum(X, H, S) - dt(l1)
    viol = 0.0
    for c0 in range(0, R, B):
        c1 = min(c0 + B, R)
        g = W @ G[c0:c1].T - P[:, c0:c1]
        for j in range(c1 - c0):
            w = W[:, c0 + j]
            grad = g[:, j]
            pg = np.where(w == 0, np.minimum(grad, 0), grad)
            viol += float(np.abs(pg.astype(np.float64)).sum())
            h = G[c0 + j, c0 + j]
            d = np.zeros_like(w)
            if h != 0:
                nw = np.maximum(w - grad / h, 0)
                d = nw - w
                W[:, c0 + j] = nw
            g[:, j + 1:] += d[:, None] * G[c0 + j, c0 + j + 1:c1]
    return viol


def cd_learn(X_rows, W_rows, H_rows, max_iter=200, tol=1e-4, l1_h=0.0, l2_h=0.0, l1_w=0.0, l2_w=0.0, S=1, update="both",
             dtype=np.float64):
    """sklearn's _fit_coordinate_descent with update_H=True.  X_rows: (T, M); W_rows: (R, M) start of the dictionary
    (sklearn's H); H_rows: (T, R) start of the activations (sklearn's W).  update="dict": the activations stay fixed and
    only the dictionary half runs and counts.  Returns (W_rows, H_rows, n_iter, violation (max_iter, 2): activation and
    dictionary half of every iteration, NaN after the stop)."""
    X = np.asarray(X_rows, dtype=dtype)
    W = np.array(np.asarray(W_rows, dtype=dtype).T)      # (M, R): rows are bins
    H = np.array(H_rows, dtype=dtype)
    viol = np.full((max_iter, 2), np.nan)
    n_iter, vinit = 0, None
    for it in range(1, max_iter + 1):
        va = 0.0
        if update == "both":
            H, v = cd_iterations(X, W.T, 1, H0=H, l1=l1_h, l2=l2_h, dtype=dtype)
            va = float(v[0])
        vd = dict_sweep(X, H, W, l1_w, l2_w, S)
        viol[it - 1] = (va, vd)
        n_iter = it
        v = va + vd
        if it == 1:
            vinit = v
        if vinit == 0 or v / vinit <= tol:
            break
    return np.array(W.T), H, n_iter, viol
