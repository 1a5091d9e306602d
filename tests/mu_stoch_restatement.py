"""deComP's mini-batch NMF (evc_mu_stoch_learn) restated in numpy: the reference of the GPU tests, itself checked bit for bit
against every recorded deComP run (tests/test_mu_stoch_host.py).

deComP's orientation throughout (frame-major): y is T x M, D is R x M with the atoms as rows, x is T x R, mask is T x M or
None.  nmf.solve(minibatch=bs, method=...) (decomp/nmf.py:16-114, nmf_methods/serizel.py, nmf_methods/kasai.py) normalises
D, then runs epochs = maxiter - 1 epochs of n_loop = int(T / bs) steps; step b of epoch e takes the frames
F = order[e][b bs : (b + 1) bs], the last T mod bs frames of the row are left alone.  deComP shuffles its arrays in place and
slices them; here the same frames are taken through `order`, whose rows `frame_orders` builds as deComP's shuffles compose.
Per step, with mu_masked_restatement's update_x and the gradients of Likelihood.grad_d (J = 1e-15):
    x_F <- update_x(y_F, x_F, D, mask_F)                       (svrmu: inner_iters times)
    g+, g- = grad_d(y_F, x_F, D, mask_F)
    asg    D_new = D max(g+, 0) / max(g-, J)                    every step      ('asg-mu'; deComP sends 'gsg-mu' here too)
    asag   a+- <- (1 - rho) a+- + rho g+-  (zero at an epoch's start);  D_new from a+-, every step
    gsag   the same accumulation; D_new from a+- once, after the epoch's last step
    svrmu  at an epoch's start full+- = (sum_b g+-_b) / n_loop from the current x and D, no x update;  per step
           P = g+ + prev-[b] + full+,  Q = g- + prev+[b] + full-  (the crossed signs are deComP's),
           D_new = max(D ((1 - alpha) + alpha P / max(Q, J)), 0),  then prev+-[b] <- g+-
    D_new <- l2_strict(D_new);  max |D - D_new| < tol returns (it, D, x) with the OLD D;  else D <- D_new
Every operation is written in deComP's order, so float64 runs reproduce it to the last bit where the BLAS agrees."""
import numpy as np

import mu_masked_restatement as mmr

J = mmr.J
METHODS = ("asg", "asag", "gsag", "svrmu")
# deComP's method names -> the four native methods
NATIVE = {"asg-mu": "asg", "gsg-mu": "asg", "asag-mu": "asag", "gsag-mu": "gsag", "svrmu": "svrmu", "svrmu-acc": "svrmu"}


def frame_orders(T, epochs, seed, method):
    """the rows deComP's shuffles with RandomState(seed) amount to: Serizel's methods shuffle an index array in place and
    cumulatively every epoch and apply it to the already shuffled frames (epochs rows); svrmu shuffles once (one row)"""
    rng = np.random.RandomState(seed)
    index, pos = np.arange(T), np.arange(T)
    rows = np.empty((1 if method == "svrmu" else max(epochs, 0), T), dtype=np.int32)
    for e in range(rows.shape[0]):
        rng.shuffle(index)
        pos = pos[index]
        rows[e] = pos
    return rows


def svrmu_acc_inner(R, M, T, beta=0.5):
    """deComP's iter_minibatch of 'svrmu-acc' (kasai.py:24-27; F = atoms, K = channels, N = frames)"""
    return int(np.maximum(beta * R * (3 * M + 2 * T) / (3 * R * T + 2 * M), 1.0))


def grad_d(y, x, d, mask, loss):
    """Likelihood.grad_d (grads.py:117-125, 152-160), in deComP's order of operations"""
    if loss == "l2":
        if mask is None:
            f = x.dot(d)
            return x.T.dot(y), x.T.dot(f)
        f = x.dot(d) * mask
        ym = y * mask
        return x.T.dot(ym), x.T.dot(f)
    if loss == "kl":
        f = x.dot(d) + J
        if mask is None:
            return x.T.dot(y / f), x.T.sum(axis=1, keepdims=True)
        ym = y * mask
        return x.T.dot(ym / f), x.T.dot(mask)
    raise ValueError(loss)


def learn(y, D, x0=None, *, mask=None, method="asg", loss="l2", batch_size, epochs, tol=0.0, forget_rate=0.5, alpha=1.0,
          inner_iters=1, order=None, dtype=np.float64):
    """-> dict(it, D, x, stats, n_steps, n_epochs, visited): `it` as deComP returns it (the epoch, from 1, of the update that
    stopped, else epochs + 1), stats[k] = max |D - D_new| of dictionary update k, n_steps = steps carried out (the stopping
    one included), n_epochs = the stopping epoch else `epochs` (evc_mu_stoch_learn's count), visited = a T mask of the
    frames some step updated.  order: None (the frames as they lie), one row (every epoch) or at least `epochs` rows."""
    assert method in METHODS
    y, D = np.asarray(y, dtype=dtype), np.asarray(D, dtype=dtype)
    mask = None if mask is None else np.asarray(mask, dtype=dtype)
    T, R = y.shape[0], D.shape[0]
    x = np.ones((T, R), dtype=dtype) if x0 is None else np.array(x0, dtype=dtype)
    bs, n_loop = int(batch_size), int(T / int(batch_size))
    if order is None:
        order = np.arange(T)[None, :]
    order = np.asarray(order)
    assert order.ndim == 2 and order.shape[1] == T and (order.shape[0] == 1 or order.shape[0] >= epochs)
    D = mmr.l2_strict(D)
    stats, n_steps = [], 0
    visited = np.zeros(T, dtype=bool)
    prev_pos = np.zeros((n_loop,) + D.shape, dtype=dtype)
    prev_neg = np.zeros((n_loop,) + D.shape, dtype=dtype)

    def batch(row, b):
        F = row[b * bs:(b + 1) * bs]
        return F, y[F], (None if mask is None else mask[F])

    def result(it, e):
        return dict(it=it, D=D, x=x, stats=np.array(stats), n_steps=n_steps, n_epochs=e, visited=visited)

    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for it in range(1, epochs + 1):
            row = order[0 if order.shape[0] == 1 else it - 1]
            if method == "svrmu":
                full_pos, full_neg = np.zeros_like(D), np.zeros_like(D)
                for b in range(n_loop):
                    F, yb, mb = batch(row, b)
                    gp, gn = grad_d(yb, x[F], D, mb, loss)
                    full_pos += gp
                    full_neg += gn
                full_pos /= n_loop
                full_neg /= n_loop
            else:
                sum_pos, sum_neg = np.zeros_like(D), np.zeros_like(D)
            for b in range(n_loop):
                F, yb, mb = batch(row, b)
                xb = x[F]
                for _ in range(inner_iters):
                    xb = mmr.update_x(yb, xb, D, mb, loss)
                x[F] = xb
                visited[F] = True
                n_steps += 1
                gp, gn = grad_d(yb, xb, D, mb, loss)
                if method == "svrmu":
                    P = gp + prev_neg[b] + full_pos
                    Q = gn + prev_pos[b] + full_neg
                    D_new = D * ((1.0 - alpha) + alpha * P / np.maximum(Q, J))
                    D_new = mmr.l2_strict(np.maximum(D_new, 0.0))
                else:
                    if method == "asg":
                        num, den = gp, gn
                    else:
                        sum_pos = (1.0 - forget_rate) * sum_pos + forget_rate * gp
                        sum_neg = (1.0 - forget_rate) * sum_neg + forget_rate * gn
                        num, den = sum_pos, sum_neg
                        if method == "gsag" and b < n_loop - 1:
                            continue
                    D_new = mmr.l2_strict(D * np.maximum(num, 0.0) / np.maximum(den, J))
                stats.append(float(np.max(np.abs(D - D_new))))
                if stats[-1] < tol:
                    return result(it, it)
                D = D_new
                if method == "svrmu":
                    prev_pos[b] = gp
                    prev_neg[b] = gn
    return result(epochs + 1, epochs)


def n_updates(method, epochs, T, batch_size):
    return epochs if method == "gsag" else epochs * int(T / batch_size)


def permutation_figure(y, D, mask, dtype, x0=None, seed=5, floor=True, **kw):
    """how far `learn` (tol = 0) moves, relative to max |D| and max |x| (the larger of the two figures), when the atoms, the
    bins AND the frames inside every batch are summed in another order - and at least (updates) eps"""
    rng = np.random.default_rng(seed)
    T, bs = y.shape[0], int(kw["batch_size"])
    pn, pm = rng.permutation(D.shape[0]), rng.permutation(D.shape[1])
    order = kw.pop("order", None)
    order = np.arange(T)[None, :] if order is None else np.asarray(order)
    moved_order = order.copy()
    for row in moved_order:
        for b in range(int(T / bs)):
            row[b * bs:(b + 1) * bs] = rng.permutation(row[b * bs:(b + 1) * bs])
    kw = dict(kw, tol=0.0, dtype=dtype)
    base = learn(y, D, x0, mask=mask, order=order, **kw)
    moved = learn(y[:, pm], D[pn][:, pm], None if x0 is None else x0[:, pn], mask=None if mask is None else mask[:, pm],
                  order=moved_order, **kw)
    Dback, xback = np.empty_like(moved["D"]), np.empty_like(moved["x"])
    Dback[np.ix_(pn, pm)] = moved["D"]
    xback[:, pn] = moved["x"]
    fig = 0.0
    for b, m in ((base["D"], Dback), (base["x"], xback)):
        b, m = b.astype(np.float64), m.astype(np.float64)
        good = np.isfinite(b)
        top = np.max(np.abs(b[good])) if good.any() else 0.0
        if top > 0:
            fig = max(fig, float(np.max(np.abs(m[good] - b[good])) / top))
    updates = max(len(base["stats"]), 1)
    return max(fig, updates * float(np.finfo(dtype).eps)) if floor else fig
