"""numpy restatement of scikit-learn 1.7.2's multiplicative update with the dictionary fixed, for any beta_loss
(_multiplicative_update_w, _beta_divergence and the loop of _fit_multiplicative_update with update_H=False) - the
arithmetic evc_beta_solve runs and the yardstick of its tests.  scikit-learn's orientation: X (T, M)
frames as rows, the dictionary D (N, M) exemplars as rows, the activations W (T, N).

beta = 1 and beta = 2 go through the generic statement here (scikit-learn special-cases them), as in the kernel."""
import numpy as np

EPS = np.finfo(np.float32).eps          # scikit-learn's EPSILON: 1.1920929e-7


def beta_divergence(X, W, D, beta):
    """sqrt(2 max(res, 0)): _beta_divergence(X, W, D, beta, square_root=True) for dense X"""
    WH = np.dot(W, D)
    if beta == 2:
        d = (X - WH).ravel()
        return np.sqrt(np.dot(d, d) / 2.0 * 2)
    WH_data, X_data = WH.ravel(), X.ravel()
    idx = X_data > EPS
    WH_data, X_data = WH_data[idx], X_data[idx]
    WH_data[WH_data < EPS] = EPS
    if beta == 1:
        res = np.dot(X_data, np.log(X_data / WH_data))
        res += np.dot(np.sum(W, axis=0), np.sum(D, axis=1)) - X_data.sum()
    elif beta == 0:
        div = X_data / WH_data
        res = np.sum(div) - np.prod(X.shape) - np.sum(np.log(div))
    else:
        res = (X_data ** beta).sum() - beta * np.dot(X_data, WH_data ** (beta - 1))
        res += np.sum(WH ** beta) * (beta - 1)
        res /= beta * (beta - 1)
    return np.sqrt(2 * max(res, 0))


def gamma_of(beta):
    return 1.0 / (2.0 - beta) if beta < 1 else 1.0 / (beta - 1.0) if beta > 2 else 1.0


def update(X, W, D, beta, l1=0.0, l2=0.0):
    """one multiplicative update of W in place, the generic branch of _multiplicative_update_w for every beta"""
    V = np.dot(W, D)
    Vd = V.copy()
    if beta - 1.0 < 0:
        Vd[Vd < EPS] = EPS
    if beta - 2.0 < 0:
        V[V < EPS] = EPS
    if beta == 0:
        V **= -1
        V **= 2
        V *= X
    else:
        V **= beta - 2
        V *= X
    num = np.dot(V, D.T)
    Vd **= beta - 1
    den = np.dot(Vd, D.T)
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
    return W


def beta_solve(X, D, beta, max_iter, tol=0.0, l1=0.0, l2=0.0, W0=None, dtype=None, check_every=10):
    """-> (W (T, N), n_iter, trace): trace[0] the error at the start, trace[c] the error after c * check_every iterations
    (evaluated only with tol > 0, NaN elsewhere and after the stop)"""
    dt = np.dtype(dtype or X.dtype)
    X, D = np.asarray(X, dtype=dt), np.asarray(D, dtype=dt)
    if W0 is None:
        W = np.full((X.shape[0], D.shape[0]), np.sqrt(X.mean() / D.shape[0]), dtype=dt)
    else:
        W = np.array(W0, dtype=dt)
    trace = np.full(1 + max_iter // check_every, np.nan)
    err0 = prev = trace[0] = beta_divergence(X, W, D, beta)
    n_iter = 0
    for n_iter in range(1, max_iter + 1):
        update(X, W, D, beta, l1, l2)
        if tol > 0 and n_iter % check_every == 0:
            err = trace[n_iter // check_every] = beta_divergence(X, W, D, beta)
            if (prev - err) / err0 < tol:
                break
            prev = err
    return W, n_iter, trace
