"""numpy restatements of the three flows of scikit-learn 1.7.2's MiniBatchNMF that rest on _solve_W: transform
(evc_online_transform), the fit with fresh restarts and partial_fit (evc_online_learn_fresh; learn_fresh and partial_fit
below, built on online_restatement).  First MiniBatchNMF._solve_W (_nmf.py:2046-2071) - the activation solve behind
MiniBatchNMF.transform, which evc_online_transform runs - in the bin-major orientation of the fixtures:
X (M, T), the dictionary W (M, R), the activations H (R, T).  Built on beta_restatement.update, the one multiplicative
update of evc_beta_solve.

Every activation starts at sqrt(mean(X) / R); after EVERY update ratio = ||H_new - H_old||_F / ||H_new||_F (float64 sums,
as the kernel forms them) and the solve stops, keeping that update, once tol > 0 and ratio <= tol.

sklearn=True follows scikit-learn's special-cased updates at beta = 1 and beta = 2 (other groupings of the same products);
False runs the generic statement for every beta, as the kernel does."""
import numpy as np

import beta_restatement as br
import online_restatement as onr

EPS = br.EPS
E64 = onr.E64


def update(X, Wsk, D, beta, l1, l2, sklearn):
    """one update of scikit-learn's W (T, R) in place; D (R, M) is scikit-learn's H"""
    if not sklearn or beta not in (1, 2):
        return br.update(X, Wsk, D, beta, l1, l2)
    if beta == 2:
        num = np.dot(X, D.T)
        den = np.dot(Wsk, np.dot(D, D.T))
    else:
        V = np.dot(Wsk, D)
        V[V < EPS] = EPS
        np.divide(X, V, out=V)
        num = np.dot(V, D.T)
        den = np.sum(D, axis=1)[np.newaxis, :]
    if l1 > 0:
        den = den + l1
    if l2 > 0:
        den = den + l2 * Wsk
    den[den == 0] = EPS
    num /= den
    Wsk *= num
    return Wsk


def solve_w(X, W, beta, max_iter, tol=0.0, l1=0.0, l2=0.0, dtype=None, sklearn=False):
    """-> (H (R, T), n_iter, change[max_iter]): n_iter the iteration the solve stopped at (max_iter if it never did),
    change[i] the ratio of iteration i + 1, NaN after the stop"""
    dt = np.dtype(dtype or X.dtype)
    Xs, D = np.ascontiguousarray(np.asarray(X, dtype=dt).T), np.ascontiguousarray(np.asarray(W, dtype=dt).T)
    R = D.shape[0]
    Wsk = np.full((Xs.shape[0], R), np.sqrt(Xs.mean() / R), dtype=dt)
    buf = Wsk.copy()
    change = np.full(max_iter, np.nan)
    n_iter = max_iter
    for it in range(1, max_iter + 1):
        update(Xs, Wsk, D, beta, l1, l2, sklearn)
        new, old = Wsk.astype(np.float64), buf.astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            change[it - 1] = np.sqrt(np.sum((new - old) ** 2)) / np.sqrt(np.sum(new ** 2))
        if tol > 0 and change[it - 1] <= tol:
            n_iter = it
            break
        buf[:] = Wsk
    return np.ascontiguousarray(Wsk.T), n_iter, change


def transform(X, W, beta, max_iter, tol=0.0, l1=0.0, l2=0.0, utt_offsets=None, dtype=None, sklearn=False):
    """one solve_w per utterance: (H (R, T), n_iter[n_utt], change[n_utt, max_iter]); an empty utterance keeps n_iter =
    max_iter and NaN ratios"""
    T = X.shape[1]
    offs = [0, T] if utt_offsets is None else list(utt_offsets)
    dt = np.dtype(dtype or X.dtype)
    H = np.zeros((W.shape[1], T), dtype=dt)
    n_iter = np.full(len(offs) - 1, max_iter, dtype=np.int32)
    change = np.full((len(offs) - 1, max_iter), np.nan)
    for u, (a, b) in enumerate(zip(offs[:-1], offs[1:])):
        if b > a:
            H[:, a:b], n_iter[u], change[u] = solve_w(X[:, a:b], W, beta, max_iter, tol, l1, l2, dt, sklearn)
    return H, n_iter, change


def learn_fresh(X, W0, beta, batch_size, max_iter, forget_factor=0.7, tol=0.0, max_no_improvement=None, l1_h=0.0, l2_h=0.0,
                l1_w=0.0, l2_w=0.0, fresh_max_iter=30, final_max_iter=0, S=1, dtype=np.float64, state=None, on_step=None):
    """online_restatement.learn with fresh restarts (MiniBatchNMF(fresh_restarts=True)._fit_transform): a step's activations
    are solve_w on the batch (then H_b[H_b < E64] = 0 if beta < 1, AFTER the solve), and the fit ends with solve_w over all
    frames (final_max_iter; 0: none - H then holds the steps' activations, zeros where no step ran).
    -> (W, H, n_iter, n_steps, cost, change, (A, B), iterations of every solve)"""
    X = np.asarray(X, dtype=dtype)
    W = np.array(W0, dtype=dtype)
    M, T = X.shape
    H = np.zeros((W.shape[1], T), dtype=dtype)
    bs = min(int(batch_size), T)
    per_pass = -(-T // bs)
    total = max_iter * per_pass
    rho = forget_factor ** (bs / T)
    A, B = (W.copy(), np.ones_like(W)) if state is None else (np.array(state[0], dtype=dtype), np.array(state[1], dtype=dtype))
    cost, change = np.full(total, np.nan), np.full(total, np.nan)
    stop = onr.Stop(T, tol, max_no_improvement)
    n_steps, solves = 0, []
    for k in range(1, total + 1):
        t0 = ((k - 1) % per_pass) * bs
        t1 = min(t0 + bs, T)
        Tb = t1 - t0
        Xb = X[:, t0:t1]
        Hb, n, _ = solve_w(Xb, W, beta, fresh_max_iter, tol, l1_h, l2_h, dtype)
        solves.append(n)
        if beta < 1:
            Hb[Hb < E64] = 0.0
        H[:, t0:t1] = Hb
        c = onr.raw_divergence(Xb, W, Hb, beta) + l1_h * Hb.sum() + Tb * l1_w * W.sum() + l2_h * (Hb ** 2).sum() \
            + Tb * l2_w * (W ** 2).sum()
        cost[k - 1] = c = float(c) / Tb
        if on_step is not None:
            on_step(k, t0, t1, W, Hb)
        Wn, A, B = onr.update_w(Xb, W, Hb, A, B, rho, beta, Tb * l1_w, Tb * l2_w, S(Tb) if callable(S) else S)
        change[k - 1] = ch = float(np.linalg.norm(Wn - W) / np.linalg.norm(Wn))
        W = Wn
        n_steps = k
        if stop.step(k, Tb, c, ch):
            break
    if final_max_iter > 0:
        H, n, _ = solve_w(X, W, beta, final_max_iter, tol, l1_h, l2_h, dtype)
        solves.append(n)
    return W, H, -(-n_steps // per_pass), n_steps, cost, change, (A, B), solves


def partial_fit(chunks, W0, beta, batch_size, forget_factor=0.7, tol=0.0, alpha=0.0, l1_ratio=0.0, fresh_max_iter=30, S=1,
                dtype=np.float64):
    """consecutive MiniBatchNMF.partial_fit calls on `chunks` (each M x T_c): one step of learn_fresh per chunk with the whole
    chunk as its batch, rho = forget_factor ** (min(batch_size, T_0) / T_0) fixed by the FIRST chunk, the penalties scaled
    per chunk as _compute_regularization does.  -> per chunk (W, A, B, iterations of the solve)"""
    T0 = chunks[0].shape[1]
    rho = forget_factor ** (min(batch_size, T0) / T0)
    M = chunks[0].shape[0]
    W, state, out = W0, None, []
    for Xc in chunks:
        W, _, _, _, _, _, state, solves = learn_fresh(Xc, W, beta, Xc.shape[1], 1, rho, tol, None, M * alpha * l1_ratio,
                                                      M * alpha * (1 - l1_ratio), alpha * l1_ratio, alpha * (1 - l1_ratio),
                                                      fresh_max_iter, 0, S, dtype, state)
        out.append((W, state[0], state[1], solves[0]))
    return out
