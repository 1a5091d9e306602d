"""numpy restatement of evc_beta_learn (include/evc.h): scikit-learn 1.7.2's multiplicative updates of BOTH factors under
any beta-divergence (_fit_multiplicative_update with update_H=True), in the bin-major orientation (X: M x T, W: M x R,
H: R x T; scikit-learn's W is H^T here and its H is W^T).  Built on tests/beta_restatement.update, applied to both
orientations:

  1. activations:  update(X^T, H^T, W^T, beta, l1_h, l2_h);  then H[H < E64] = 0 if beta < 1
  2. dictionary, with the new H:  update(X, W, H, beta, l1_w, l2_w);  then W[W < E64] = 0 if beta <= 1
  3. err = beta_divergence(X^T, H^T, W^T, beta) at the start and every check_every iterations; stop when
     (prev - err) / err_at_start < tol (tol = 0: never)
E64 = 2^-52 in both element types.  beta = 1 and beta = 2 go through the generic statement, as in the kernels.

With S > 1 the dictionary half's sums over the frames (Num and Den) are taken the way the kernels take them: S contiguous
frame ranges [s T / S, (s + 1) T / S), each summed on its own, the partial sums added in the order s = 0 .. S - 1.
"""
import numpy as np

from beta_restatement import EPS, beta_divergence, gamma_of, update

E64 = np.finfo(np.float64).eps


def frame_ranges(T, S):
    return [(s * T // S, (s + 1) * T // S) for s in range(S)]


def update_h(X, W, H, beta, l1=0.0, l2=0.0):
    Ht = np.ascontiguousarray(H.T)
    update(np.ascontiguousarray(X.T), Ht, np.ascontiguousarray(W.T), beta, l1, l2)
    if beta < 1:
        Ht[Ht < E64] = 0.0
    return np.ascontiguousarray(Ht.T)


def update_w(X, W, H, beta, l1=0.0, l2=0.0, S=1):
    W = np.array(W)
    if S == 1:
        update(X, W, H, beta, l1, l2)
    else:       # beta_restatement.update with the two products split over the frames
        V = np.dot(W, H)
        Vd = V.copy()
        if beta - 1.0 < 0:
            Vd[Vd < EPS] = EPS
        if beta - 2.0 < 0:
            V[V < EPS] = EPS
        if beta == 0:
            V **= -1
            V **= 2
        else:
            V **= beta - 2
        V *= X
        Vd **= beta - 1
        num, den = np.zeros_like(W), np.zeros_like(W)
        for b, e in frame_ranges(X.shape[1], S):
            num += np.dot(V[:, b:e], H[:, b:e].T)
            den += np.dot(Vd[:, b:e], H[:, b:e].T)
        if l1 > 0:
            den += l1
        if l2 > 0:
            den = den + l2 * W
        den[den == 0] = EPS
        num /= den
        g = gamma_of(beta)
        if g != 1:
            num **= g
        W *= num
    if beta <= 1:
        W[W < E64] = 0.0
    return W


def error(X, W, H, beta):
    return float(beta_divergence(np.ascontiguousarray(X.T), np.ascontiguousarray(H.T), np.ascontiguousarray(W.T), beta))


def learn(X, W0, H0, beta, iters, check_every=10, tol=0.0, l1_h=0.0, l2_h=0.0, l1_w=0.0, l2_w=0.0, S=1, dtype=np.float64):
    """-> (W, H, n_iter, err): err[0] the error at the start, err[c] after check c (NaN where not evaluated)"""
    X = np.asarray(X, dtype=dtype)
    W = np.array(W0, dtype=dtype)
    H = np.array(H0, dtype=dtype)
    n_checks = iters // check_every if check_every > 0 else 0
    err = np.full(1 + n_checks, np.nan)
    if check_every > 0:
        err[0] = prev = error(X, W, H, beta)
    n_iter = 0
    for it in range(1, iters + 1):
        H = update_h(X, W, H, beta, l1_h, l2_h)
        W = update_w(X, W, H, beta, l1_w, l2_w, S)
        n_iter = it
        if check_every <= 0 or it % check_every:
            continue
        c = it // check_every
        err[c] = e = error(X, W, H, beta)
        if tol > 0 and (prev - e) / err[0] < tol:
            break
        prev = e
    return W, H, n_iter, err
