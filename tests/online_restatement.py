"""numpy restatement of evc_online_learn (include/evc.h): scikit-learn 1.7.2's MiniBatchNMF._fit_transform with
init='custom' and fresh_restarts=False, in the bin-major orientation (X: M x T, W: M x R, H: R x T; scikit-learn's W is
H^T here and its H is W^T).  Built on beta_restatement / beta_learn_restatement.

Batches are contiguous ranges of bs = min(batch_size, T) frames, in order and cycled; rho = forget_factor ** (bs / T).
Step k = 1, 2, ... on batch b of T_b frames:

  1. activations:  beta_learn_restatement.update_h on the batch's columns (one update; H_b[H_b < E64] = 0 if beta < 1)
  2. cost = (res + l1_h sum H_b + T_b l1_w sum W + l2_h sum H_b^2 + T_b l2_w sum W^2) / T_b, res the raw divergence
  3. dictionary, with the new H_b:  Num, Den over the batch's frames (S contiguous frame ranges, added in ascending
     order), Den += T_b l1_w + T_b l2_w W, 0 -> EPS;  P = W^(1/gamma);  A <- rho A + Num P;  B <- rho B + Den;
     W <- (A / B)^gamma;  W[W < E64] = 0 if beta <= 1.  A = W0, B = 1 on a fresh start.
  4. convergence as _minibatch_convergence (step 1 ignored)
l1_w and l2_w are PER FRAME.  S: an int, or a function of the batch's frame count (the kernels' learn_splits)."""
import numpy as np

from beta_learn_restatement import E64, frame_ranges, update_h
from beta_restatement import EPS, gamma_of


def raw_divergence(X, W, H, beta):
    """_beta_divergence(X^T, H^T, W^T, beta, square_root=False) for dense X: not clamped at 0"""
    Xs, Ws, Ds = np.ascontiguousarray(X.T), np.ascontiguousarray(H.T), np.ascontiguousarray(W.T)
    WH = np.dot(Ws, Ds)
    if beta == 2:
        d = (Xs - WH).ravel()
        return np.dot(d, d) / 2.0
    WH_data, X_data = WH.ravel(), Xs.ravel()
    idx = X_data > EPS
    WH_data, X_data = WH_data[idx], X_data[idx]
    WH_data[WH_data < EPS] = EPS
    if beta == 1:
        res = np.dot(X_data, np.log(X_data / WH_data))
        res += np.dot(np.sum(Ws, axis=0), np.sum(Ds, axis=1)) - X_data.sum()
    elif beta == 0:
        div = X_data / WH_data
        res = np.sum(div) - np.prod(Xs.shape) - np.sum(np.log(div))
    else:
        res = (X_data ** beta).sum() - beta * np.dot(X_data, WH_data ** (beta - 1))
        res += np.sum(WH ** beta) * (beta - 1)
        res /= beta * (beta - 1)
    return res


def num_den(X, W, H, beta, l1=0.0, l2=0.0, S=1):
    """Num and Den of the dictionary update over the frames given, as beta_learn_restatement.update_w forms them"""
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
    if S == 1:
        num, den = np.dot(V, H.T), np.dot(Vd, H.T)
    else:
        num, den = np.zeros_like(W), np.zeros_like(W)
        for b, e in frame_ranges(X.shape[1], S):
            num += np.dot(V[:, b:e], H[:, b:e].T)
            den += np.dot(Vd[:, b:e], H[:, b:e].T)
    if l1 > 0:
        den += l1
    if l2 > 0:
        den = den + l2 * W
    den[den == 0] = EPS
    return num, den


def update_w(X, W, H, A, B, rho, beta, l1=0.0, l2=0.0, S=1):
    """the online update of W, A and B (new arrays) from one batch"""
    dt = W.dtype
    num, den = num_den(X, W, H, beta, l1, l2, S)
    g = gamma_of(beta)
    P = W.copy()
    if g != 1:
        P **= 1 / g
    num *= P
    A = (A * dt.type(rho) + num).astype(dt)
    B = (B * dt.type(rho) + den).astype(dt)
    Wn = A / B
    if g != 1:
        Wn **= g
    if beta <= 1:
        Wn[Wn < E64] = 0.0
    return Wn.astype(dt), A, B


class Stop:
    """_minibatch_convergence: step(k, frames, cost, change) -> whether the loop ends with step k = 1, 2, ..."""

    def __init__(self, T, tol=0.0, max_no_improvement=None):
        self.T, self.tol, self.mni = T, tol, max_no_improvement
        self.ewa = self.ewa_min = None
        self.no_improvement = 0

    def step(self, k, frames, cost, change):
        if k == 1:
            return False
        if self.ewa is None:
            self.ewa = cost
        else:
            alpha = min(frames / (self.T + 1), 1)
            self.ewa = self.ewa * (1 - alpha) + cost * alpha
        if self.tol > 0 and change <= self.tol:
            return True
        if self.ewa_min is None or self.ewa < self.ewa_min:
            self.no_improvement, self.ewa_min = 0, self.ewa
        else:
            self.no_improvement += 1
        return self.mni is not None and self.mni >= 0 and self.no_improvement >= self.mni


def learn(X, W0, H0, beta, batch_size, max_iter, forget_factor=0.7, tol=0.0, max_no_improvement=None, l1_h=0.0, l2_h=0.0,
          l1_w=0.0, l2_w=0.0, S=1, dtype=np.float64, state=None, on_step=None):
    """-> (W, H, n_iter, n_steps, cost, change, (A, B)): cost[k], change[k] of step k + 1, NaN after the stop.
    on_step(k, t0, t1, W, Hb): called with what step k's cost is evaluated on"""
    X = np.asarray(X, dtype=dtype)
    W = np.array(W0, dtype=dtype)
    H = np.array(H0, dtype=dtype)
    M, T = X.shape
    bs = min(int(batch_size), T)
    per_pass = -(-T // bs)
    total = max_iter * per_pass
    rho = forget_factor ** (bs / T)
    A, B = (W.copy(), np.ones_like(W)) if state is None else (np.array(state[0], dtype=dtype), np.array(state[1], dtype=dtype))
    cost, change = np.full(total, np.nan), np.full(total, np.nan)
    stop = Stop(T, tol, max_no_improvement)
    n_steps = 0
    for k in range(1, total + 1):
        t0 = ((k - 1) % per_pass) * bs
        t1 = min(t0 + bs, T)
        Tb = t1 - t0
        Xb = X[:, t0:t1]
        Hb = update_h(Xb, W, H[:, t0:t1], beta, l1_h, l2_h)
        H[:, t0:t1] = Hb
        c = raw_divergence(Xb, W, Hb, beta) + l1_h * Hb.sum() + Tb * l1_w * W.sum() + l2_h * (Hb ** 2).sum() \
            + Tb * l2_w * (W ** 2).sum()
        cost[k - 1] = c = float(c) / Tb
        if on_step is not None:
            on_step(k, t0, t1, W, Hb)
        Wn, A, B = update_w(Xb, W, Hb, A, B, rho, beta, Tb * l1_w, Tb * l2_w, S(Tb) if callable(S) else S)
        change[k - 1] = ch = float(np.linalg.norm(Wn - W) / np.linalg.norm(Wn))
        W = Wn
        n_steps = k
        if stop.step(k, Tb, c, ch):
            break
    return W, H, -(-n_steps // per_pass), n_steps, cost, change, (A, B)
