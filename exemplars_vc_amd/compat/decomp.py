"""Drop-in mirror of deComP's `lasso.solve` and `nnls.solve` (decomp/lasso.py, decomp/nnls.py) on the GPU.

    from exemplars_vc_amd.compat.decomp import lasso, nnls      # instead of: from decomp import lasso, nnls
    it, x = lasso.solve(y, A, alpha, tol=1e-3, method='fista', maxiter=1000)
    it, x = nnls.solve(y, A, alpha, method='fista')             # lasso.solve with method + '_pos'

deComP's orientation: y is [..., n_channels], A is [n_features, n_channels] (exemplars as rows), x is [..., n_features];
leading dimensions of y are flattened to frames.  It minimises 1 / (2 n_channels) ||y - x A||^2 + alpha |x| per frame in the
scaling that gives every exemplar unit norm, with the step of the Gershgorin bound, checks max(|dx| - tol_n) < 0 over the
whole call every 10th iteration, and returns (it, x): the index of the last iteration and the activations.  The methods
`ista`, `fista`, `ista_pos` and `fista_pos` are one native call each (evc_prox_solve).

`mask` (missing data): a float array of y's shape and dtype kind, >= 0, that weights every bin of every frame; a zero marks a
missing bin.  It runs natively for the same four methods (evc_prox_masked_solve, the factored sweep), with deComP's step:
the Gershgorin bound of A diag(mean of the mask over all frames) A^T.  A negative mask is refused with AssertionError and
a mask that is not float with ValueError (deComP: DtypeMismatchError, a ValueError), where deComP's assertions refuse them.

Not mirrored, NotImplementedError: a 1-D `mask` (weights per bin: multiply y and A by them), complex input, `cd`,
`parallel_cd`, `admm` - and `acc_ista`, which at an exhausted `maxiter` returns the iterate before the last (lasso.py:357);
its schedule is offered natively, solve_activations_prox(momentum="nesterov"), where the last iterate is returned.

`dictionary_learning.solve(y, D, alpha, x=None, tol, minibatch, maxiter, method='block_cd', lasso_method=..., ...)` mirrors
deComP's online sparse dictionary learning (decomp/dictionary_learning.py) as one native call (evc_prox_learn) and returns
(it, D, x) with D in deComP's orientation, atoms as rows.  Its lasso half is one of the four methods above, which must be
named: deComP's default there, 'cd', is not mirrored.  Its `mask` is refused here with NotImplementedError;
exemplars_vc_amd.learn_dictionary_sparse(mask=..., seed=...) runs deComP's masked learning natively (evc_prox_masked_learn).

`nmf.solve(y, D, x=None, tol=1e-3, minibatch=None, maxiter=1000, method='mu', likelihood='l2', mask=None)` mirrors deComP's
batch NMF by multiplicative updates (decomp/nmf.py, nmf_methods/batch_mu.py) as one native call (evc_mu_masked_learn) and
returns (it, D, x); with `minibatch=bs` and method 'asg-mu', 'gsg-mu', 'asag-mu', 'gsag-mu', 'svrmu' or 'svrmu-acc' it mirrors deComP's
mini-batch NMF (nmf_methods/serizel.py, nmf_methods/kasai.py) as one native call (evc_mu_stoch_learn), with their options
forget_rate / alpha, beta.  As in deComP, `minibatch` with 'mu' and a mini-batch method without `minibatch` raise
NotImplementedError.
"""
from __future__ import annotations

import types

import numpy as np

from ..solver import solve_activations_prox

AVAILABLE_METHODS = ['ista', 'cd', 'acc_ista', 'fista', 'parallel_cd', 'admm']
AVAILABLE_NNLS_METHODS = ['ista_pos', 'cd_pos', 'acc_ista_pos', 'fista_pos', 'parallel_cd_pos', 'admm_pos']
_NATIVE = {"ista": "ista", "fista": "fista"}


def _lasso_solve(y, A, alpha, x=None, tol=1.0e-3, method='ista', maxiter=1000, mask=None, device=None, **kwargs):
    """deComP's lasso.solve -> (it, x).  `device`: the GPU to run on (default: the current one)."""
    if mask is not None:
        mask = np.asarray(mask)
        if mask.dtype.kind != 'f':               # deComP: assert_dtypes(mask=mask, dtypes='f')
            raise ValueError("compat.decomp: Data type should be one of f, but given %s for mask" % mask.dtype)
        assert (mask >= 0.0).all()               # deComP: assert_nonnegative(mask)
        if mask.ndim == 1:
            raise NotImplementedError("compat.decomp: a 1-D `mask` (weights per bin) is not mirrored: multiply y and A by it")
    if kwargs:
        raise NotImplementedError("compat.decomp: unknown options %s" % sorted(kwargs))
    if method not in AVAILABLE_METHODS + AVAILABLE_NNLS_METHODS:
        raise ValueError('Available methods are {0:s}. Given {1:s}'.format(str(AVAILABLE_METHODS), method))
    positive = method.endswith("_pos")
    base = method[:-4] if positive else method
    if base not in _NATIVE:
        raise NotImplementedError("compat.decomp: method '%s' is not mirrored (ista, fista, ista_pos, fista_pos are)" % method)
    y, A = np.asarray(y), np.asarray(A)
    if y.dtype.kind == 'c' or A.dtype.kind == 'c' or (x is not None and np.asarray(x).dtype.kind == 'c'):
        raise NotImplementedError("compat.decomp: complex input is not mirrored")
    if A.ndim != 2:
        raise ValueError("A must be 2-D [n_features, n_channels], got shape %s" % (A.shape,))
    if y.ndim < 1 or y.shape[-1] != A.shape[1]:
        raise ValueError("y %s and A %s disagree on the number of channels" % (y.shape, A.shape))
    dtype = np.float32 if y.dtype == np.float32 else np.float64
    lead, N = y.shape[:-1], A.shape[0]
    frames = y.reshape(-1, y.shape[-1])
    if mask is not None:
        if mask.shape != y.shape:
            raise ValueError("mask has shape %s, expected y's shape %s" % (mask.shape, y.shape))
        mask = np.ascontiguousarray(mask.reshape(frames.shape), dtype=dtype)
    x0 = None
    if x is not None:
        x = np.asarray(x)
        if x.shape != lead + (N,):
            raise ValueError("x has shape %s, expected %s" % (x.shape, lead + (N,)))
        x0 = np.ascontiguousarray(x.reshape(-1, N), dtype=dtype)
    maxiter = int(maxiter)
    if maxiter <= 0:                             # no update: deComP returns the start, scaled and unscaled
        return maxiter - 1, (np.zeros(lead + (N,), dtype=dtype) if x0 is None else x0.reshape(lead + (N,)).copy())
    H, info = solve_activations_prox(np.ascontiguousarray(A, dtype=dtype), np.ascontiguousarray(frames, dtype=dtype), x0,
                                     alpha=float(alpha), positive=positive, momentum=_NATIVE[base], normalize=True,
                                     iters=maxiter, tol=float(tol), check_every=10, stop_rule="decomp", layout="frame_major",
                                     dtype="f64" if dtype == np.float64 else "f32", device=device, info=True,
                                     **({} if mask is None else dict(mask=mask, lip_weights="mean")))
    return int(info["n_iter"][0]) - 1, np.asarray(H).reshape(lead + (N,))


def _nnls_solve(y, A, alpha, x=None, tol=1.0e-3, method='ista_pos', maxiter=1000, mask=None, **kwargs):
    """deComP's nnls.solve: lasso.solve with method + '_pos' (its own default, 'ista_pos', therefore names no method: pass
    method='ista' or 'fista')"""
    return _lasso_solve(y, A, alpha, x, tol, method + '_pos', maxiter, mask, **kwargs)


def _dictionary_learning_solve(y, D, alpha, x=None, tol=1.0e-3, minibatch=None, maxiter=1000, method='block_cd',
                               lasso_method='cd', lasso_iter=10, lasso_tol=1.0e-5, mask=None, random_seed=None, device=None):
    """deComP's dictionary_learning.solve -> (it, D, x): y is [n_samples, n_channels], D [n_features, n_channels] (atoms as
    rows), x [n_samples, n_features] (None: ones).  One native call (evc_prox_learn) of maxiter - 1 epochs over
    int(n_samples / minibatch) batches each, the frames in the order deComP shuffles them with `random_seed`; `it` is the
    epoch (from 1) in which max |D_new - D| < tol stopped the loop, else maxiter.  Mirrored lasso methods: ista, fista,
    ista_pos, fista_pos.  NotImplementedError: deComP's default lasso_method='cd' (name one of the four), 'parallel_cd',
    'admm', 'acc_ista' (its exhausted-maxiter quirk, see the module's text), `mask`, complex input, minibatch=None (deComP
    itself raises there) and any method but 'block_cd'."""
    from ..solver import decomp_frame_order, learn_dictionary_sparse
    if minibatch is None:
        raise NotImplementedError('Only online methods are implemented. minibatch is required.')
    if method != 'block_cd':
        raise NotImplementedError("compat.decomp: method '%s' is not mirrored (block_cd is)" % method)
    if mask is not None:
        raise NotImplementedError("compat.decomp: dictionary_learning with a `mask` is not mirrored here; "
                                  "learn_dictionary_sparse(mask=..., seed=...) runs it natively (evc_prox_masked_learn)")
    positive = lasso_method.endswith("_pos")
    base = lasso_method[:-4] if positive else lasso_method
    if base not in _NATIVE:
        raise NotImplementedError("compat.decomp: lasso_method '%s' is not mirrored: name one of ista, fista, ista_pos, "
                                  "fista_pos" % lasso_method)
    y, D = np.asarray(y), np.asarray(D)
    if y.dtype.kind == 'c' or D.dtype.kind == 'c' or (x is not None and np.asarray(x).dtype.kind == 'c'):
        raise NotImplementedError("compat.decomp: complex input is not mirrored")
    if y.ndim != 2 or D.ndim != 2 or y.shape[1] != D.shape[1]:
        raise ValueError("y %s and D %s must be 2-D and agree on the number of channels" % (y.shape, D.shape))
    dtype = np.float32 if y.dtype == np.float32 else np.float64
    T, N = y.shape[0], D.shape[0]
    minibatch = int(minibatch)
    if T < minibatch:                            # deComP: MinibatchBase.__init__
        raise ValueError('Minibatch size should be smaller than the total size. Given {} < {}'.format(T, minibatch))
    x0 = np.ones((T, N), dtype=dtype) if x is None else np.ascontiguousarray(x, dtype=dtype)
    if x0.shape != (T, N):
        raise ValueError("x has shape %s, expected %s" % (x0.shape, (T, N)))
    maxiter = int(maxiter)
    epochs = max(maxiter - 1, 0)
    Dn, H, info = learn_dictionary_sparse(np.ascontiguousarray(y, dtype=dtype), np.ascontiguousarray(D, dtype=dtype), x0,
                                          alpha=float(alpha), layout="frame_major", batch_size=minibatch, epochs=epochs,
                                          tol=float(tol), lasso_iters=int(lasso_iter), lasso_tol=float(lasso_tol),
                                          positive=positive, momentum=_NATIVE[base],
                                          order=decomp_frame_order(T, epochs, random_seed),   # None: unseeded, as deComP
                                          dtype="f64" if dtype == np.float64 else "f32", device=device, info=True)
    change = info["change"][:info["n_steps"]]
    stopped = info["n_steps"] > 0 and bool(change[-1] < float(tol))
    return (info["n_epochs"] if stopped else maxiter), np.asarray(Dn), np.asarray(H)


def _nmf_solve(y, D, x=None, tol=1.0e-3, minibatch=None, maxiter=1000, method='mu', likelihood='l2', mask=None,
               random_seed=None, device=None, **kwargs):
    """deComP's nmf.solve -> (it, D, x): y is [n_samples, n_channels], D [n_features, n_channels] (atoms as rows), x
    [n_samples, n_features] (None: ones), mask like y.  One native call (evc_mu_masked_learn) of at most maxiter - 1
    iterations (deComP's loop is `range(1, maxiter)`), the statistic max |D - D_new| checked after every one; `it` is the
    iteration (from 1) at which it fell below tol, else maxiter.  Negative y (likelihood 'kl'), D or x: AssertionError;
    mismatched shapes, dimensions or dtypes: ValueError (deComP's ShapeMismatchError, DimInvalidError and DtypeMismatchError
    are ValueErrors); `minibatch` with 'mu', a mini-batch method without `minibatch`, unknown options, complex input:
    NotImplementedError.  With `minibatch`: _nmf_solve_minibatch."""
    from ..solver import learn_dictionary_masked
    y, D = np.asarray(y), np.asarray(D)
    x = np.ones((y.shape[0], D.shape[0]), dtype=y.dtype) if x is None else np.asarray(x)
    mask = None if mask is None else np.asarray(mask)
    arrays = [("y", y), ("D", D), ("x", x)] + ([] if mask is None else [("mask", mask)])
    for name, a in arrays:                       # deComP: assert_dtypes
        if name != "mask" and a.dtype.kind == 'c':
            raise NotImplementedError("compat.decomp: complex input is not mirrored")
        if a.dtype != y.dtype:
            raise ValueError('Data type should be all identical, y: {0:s} and {1:s}: {2:s}'.format(str(y.dtype), name, str(a.dtype)))
        if a.dtype.kind != 'f':
            raise ValueError('Data type should be one of f, but given {0:s} for {1:s}'.format(str(a.dtype), name))
    for name, a in arrays[:3]:                   # deComP: assert_ndim
        if a.ndim != 2:
            raise ValueError('Dimension of {0:s} should be 2 but given {1:d}'.format(name, a.ndim))
    if x.shape[-1:] != D.shape[:1]:              # deComP: assert_shapes
        raise ValueError('x.shape[-1:] == D.shape[:1] should be satisfied. Given: x.shape = {0:s} and D.shape = {1:s}'.format(
            str(x.shape), str(D.shape)))
    if y.shape[-1] != D.shape[-1]:
        raise ValueError('y.shape[[-1]] == D.shape[[-1]] should be satisfied. Given: y.shape = {0:s} and D.shape = {1:s}'.format(
            str(y.shape), str(D.shape)))
    if mask is not None and mask.shape != y.shape:
        raise ValueError('Shapes of y and mask should be identical. Given y: {0:s} and mask: {1:s}'.format(
            str(y.shape), str(mask.shape)))
    if x.shape[0] != y.shape[0]:
        raise ValueError("x has shape %s, expected %s" % (x.shape, (y.shape[0], D.shape[0])))
    assert (D >= 0.0).all() and (x >= 0.0).all()             # deComP: assert_nonnegative
    if likelihood == 'kl':
        assert (y >= 0.0).all()
    if likelihood not in ('l2', 'kl'):
        raise NotImplementedError("compat.decomp: likelihood '%s' is not mirrored (l2 and kl are)" % likelihood)
    if minibatch is None and method != 'mu':
        raise NotImplementedError('Batch-NMF with {} algorithm is not yet implemented.'.format(method))
    if minibatch is not None and method not in MINIBATCH_METHODS:      # 'mu' among them, as in deComP
        raise NotImplementedError('NMF with {} algorithm is not yet implemented.'.format(method))
    allowed = () if minibatch is None else ('alpha', 'beta') if method in ('svrmu', 'svrmu-acc') else ('forget_rate',)
    if any(k not in allowed for k in kwargs):
        raise NotImplementedError("compat.decomp: unknown options %s" % sorted(k for k in kwargs if k not in allowed))
    dtype = np.float32 if y.dtype == np.float32 else np.float64
    if mask is not None:
        assert (mask >= 0.0).all()               # a negative weight: the native calls do not look for it
    maxiter = int(maxiter)
    if minibatch is not None:
        return _nmf_solve_minibatch(y, D, x, mask, float(tol), int(minibatch), maxiter, method, likelihood, random_seed, dtype,
                                    device, kwargs)
    Dn, H, info = learn_dictionary_masked(np.ascontiguousarray(y, dtype=dtype), np.ascontiguousarray(D, dtype=dtype),
                                          np.ascontiguousarray(x, dtype=dtype),
                                          None if mask is None else np.ascontiguousarray(mask, dtype=dtype),
                                          loss={"l2": "frobenius", "kl": "kl"}[likelihood], layout="frame_major",
                                          iters=max(maxiter - 1, 0), check_every=1, tol=float(tol),
                                          dtype="f64" if dtype == np.float64 else "f32", device=device, info=True)
    return (info["n_iter"] if info["stopped"] else maxiter), np.asarray(Dn), np.asarray(H)


MINIBATCH_METHODS = ['asg-mu', 'gsg-mu', 'asag-mu', 'gsag-mu', 'svrmu', 'svrmu-acc']
_STOCH_NATIVE = {'asg-mu': 'asg', 'gsg-mu': 'asg', 'asag-mu': 'asag', 'gsag-mu': 'gsag', 'svrmu': 'svrmu', 'svrmu-acc': 'svrmu'}


def _nmf_solve_minibatch(y, D, x, mask, tol, minibatch, maxiter, method, likelihood, random_seed, dtype, device, kwargs):
    """nmf.solve's mini-batch half -> (it, D, x): one native call (evc_mu_stoch_learn) of maxiter - 1 epochs over
    int(n_samples / minibatch) batches each.  The frames go in the order deComP shuffles them with `random_seed`: Serizel's
    four methods reshuffle cumulatively every epoch, Kasai's two shuffle once.  'gsg-mu' runs 'asg-mu' (deComP's dispatch);
    'svrmu-acc' is 'svrmu' with int(max(beta F (3 K + 2 N) / (3 F N + 2 K), 1)) activation updates per step.  `it` is the
    epoch (from 1) of the update that stopped the loop, else maxiter."""
    from ..solver import decomp_frame_order, learn_dictionary_stochastic
    T, (F, K) = y.shape[0], D.shape
    if T < minibatch:                            # deComP: MinibatchBase.__init__
        raise ValueError('Minibatch size should be smaller than the total size. Given {} < {}'.format(T, minibatch))
    kasai = method in ('svrmu', 'svrmu-acc')
    inner = 1
    if method == 'svrmu-acc':
        inner = int(np.maximum(float(kwargs.get('beta', 0.5)) * F * (3 * K + 2 * T) / (3 * F * T + 2 * K), 1.0))
    epochs = max(maxiter - 1, 0)
    order = decomp_frame_order(T, 1 if kasai else epochs, random_seed)   # None: unseeded, as deComP
    Dn, H, info = learn_dictionary_stochastic(np.ascontiguousarray(y, dtype=dtype), np.ascontiguousarray(D, dtype=dtype),
                                              np.ascontiguousarray(x, dtype=dtype),
                                              None if mask is None else np.ascontiguousarray(mask, dtype=dtype),
                                              method=_STOCH_NATIVE[method], loss={"l2": "frobenius", "kl": "kl"}[likelihood],
                                              layout="frame_major", batch_size=minibatch, epochs=epochs, tol=tol,
                                              forget_rate=float(kwargs.get('forget_rate', 0.5)),
                                              alpha=float(kwargs.get('alpha', 1.0)), inner_iters=inner,
                                              order=order if epochs > 0 else None,
                                              dtype="f64" if dtype == np.float64 else "f32", device=device, info=True)
    return (info["n_epochs"] if info["stopped"] else maxiter), np.asarray(Dn), np.asarray(H)


nmf = types.SimpleNamespace(solve=_nmf_solve, BATCH_METHODS=['mu'], MINIBATCH_METHODS=MINIBATCH_METHODS)
lasso = types.SimpleNamespace(solve=_lasso_solve, AVAILABLE_METHODS=AVAILABLE_METHODS,
                              AVAILABLE_NNLS_METHODS=AVAILABLE_NNLS_METHODS)
nnls = types.SimpleNamespace(solve=_nnls_solve)
dictionary_learning = types.SimpleNamespace(solve=_dictionary_learning_solve)
