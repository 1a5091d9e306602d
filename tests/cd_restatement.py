"""numpy restatement of the blocked, factored coordinate descent that evc_cd_solve runs.

scikit-learn's solver='cd' with the dictionary fixed (_update_cdnmf_fast, shuffle=False) visits the components
t = 0..N-1 in order; for every frame grad = (A^T A h)_t + l2 h_t - (A^T x)_t + l1 and h_t <- max(h_t - grad / hess_t, 0)
with hess_t = |a_t|^2 + l2 (skipped where 0).  Here the residual r = h A - x is kept per frame, components are taken
in blocks of 16: the block's gradients from r at its start, 16 in-order steps corrected by the block's Gram block,
then r += delta A_block.  Same coordinate order, only the rounding differs.  All frames are processed at once.
"""
import numpy as np

B = 16


def cd_iterations(X_rows, W_rows, iters, H0=None, l1=0.0, l2=0.0, dtype=np.float64):
    """Run `iters` sweeps on every frame (no stop rule).  X_rows: (T, M), W_rows: (N, M).
    Returns (H (T, N), per-sweep violations (iters,), float64)."""
    X = np.asarray(X_rows, dtype=dtype)
    A = np.asarray(W_rows, dtype=dtype)
    T, M = X.shape
    N = A.shape[0]
    H = np.zeros((T, N), dtype=dtype) if H0 is None else np.array(H0, dtype=dtype)
    R = H @ A - X
    l1, l2 = dtype(l1), dtype(l2)
    hess = np.einsum("nm,nm->n", A, A) + l2
    viols = []
    for _ in range(iters):
        viol = 0.0
        for c0 in range(0, N, B):
            Ab = A[c0:c0 + B]
            G = Ab @ Ab.T
            g = R @ Ab.T + l2 * H[:, c0:c0 + B] + l1
            d = np.zeros_like(g)
            for j in range(Ab.shape[0]):
                w = H[:, c0 + j]
                grad = g[:, j]
                pg = np.where(w == 0, np.minimum(grad, 0), grad)
                viol += float(np.abs(pg.astype(np.float64)).sum())
                h = hess[c0 + j]
                if h != 0:
                    nw = np.maximum(w - grad / h, 0)
                    d[:, j] = nw - w
                    H[:, c0 + j] = nw
                g[:, j + 1:] += d[:, j:j + 1] * G[j, j + 1:]
            R = R + d @ Ab
        viols.append(viol)
    return H, np.array(viols)


def cd_solve(X_rows, W_rows, max_iter=200, tol=1e-4, l1=0.0, l2=0.0, dtype=np.float64):
    """sklearn's _fit_coordinate_descent stop rule on one utterance.  Returns (H (T, N), n_iter, violations)."""
    X = np.asarray(X_rows, dtype=dtype)
    A = np.asarray(W_rows, dtype=dtype)
    H = np.zeros((X.shape[0], A.shape[0]), dtype=dtype)
    viols = []
    n_iter = 0
    vinit = None
    for it in range(1, max_iter + 1):
        H, v = cd_iterations(X, A, 1, H0=H, l1=l1, l2=l2, dtype=dtype)
        v = float(v[0])
        viols.append(v)
        n_iter = it
        if it == 1:
            vinit = v
        if vinit == 0 or v / vinit <= tol:
            break
    return H, n_iter, np.array(viols)
