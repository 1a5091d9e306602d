"""S2: pymf's `NMF(data, num_bases).factorize(compute_w=False)` on the GPU.

Mirrors /root/reference/dependencies/pymf-29e3490d.../pymf/nmf.py:21-77 and
pymf/base.py:102-270: `data` is M x T, `W` M x N (set by the caller), `H` N x T is created
lazily as random((N,T)) + 1e-4 from the global numpy RNG, updated IN PLACE by
`factorize`, with `ferr[i] = ||data - W H||_F` per iteration and the machine-epsilon stop.
Only the fixed-dictionary path (`compute_w=False`) is the accelerated path.  pymf's DEFAULT is
`compute_w=True` (base.py:208): the dictionary update (nmf.py:72-76, a few small products per
iteration) then runs on the host in numpy, as SURVEY 8(b) S2 allows, while every activation
update still goes through the GPU solver - a drop-in must not raise on the default arguments
(round 3 did).  A RuntimeWarning says so once per call.
`NMF(..., dictionary_update="device")` opts in to the accelerated loop instead: both updates run on the GPU in one
call (evc_nmf_learn, pymf surface), W and H are updated in place and `ferr` is as pymf makes it.

`SNMF` is pymf's semi-NMF (pymf/snmf.py): `data` and `W` are signed, only `H` is non-negative.  `compute_w=False` is one
native call (evc_semi_solve); the default `compute_w=True` forms W = data H^T (H H^T)^-1 on the host (snmf.py:61-64) and
runs one GPU activation update per iteration, with the same warning.

`CNMF` is pymf's convex NMF (pymf/cnmf.py): data ~ (data G) H with signed data and G, H >= 0.  `factorize` is one native
call (evc_convex_learn) for every combination of compute_w / compute_h; the default start is pymf's k-means on the host,
`CNMF(..., start="device")` runs the same k-means from the same random draw on the GPU (evc_kmeans).

`Kmeans` is pymf's k-means (pymf/kmeans.py, "unary-convex matrix factorization"): `factorize` is one native call (evc_kmeans),
`compute_w=False` is pymf's `vq` against the given centres.
"""
from __future__ import annotations

import logging

import numpy as np

from ..solver import (convex_cluster_start, frame_residuals, kmeans, learn_dictionary, learn_dictionary_convex,
                      solve_activations, solve_activations_semi, synthesize)

_EPS = np.finfo(float).eps


class NMF:
    _EPS = _EPS

    def __init__(self, data, num_bases=4, **kwargs):
        self._logger = logging.getLogger("pymf")
        self.data = data
        self._num_bases = num_bases
        self._data_dimension, self._num_samples = self.data.shape
        self._device = kwargs.get("device")
        self._algo = kwargs.get("algo", "auto")
        self._dictionary_update = kwargs.get("dictionary_update", "host")
        if self._dictionary_update not in ("host", "device"):
            raise ValueError("dictionary_update must be 'host' or 'device'")

    # -- pymf/base.py:133-165 --
    def residual(self):
        WH = synthesize(np.asarray(self.W, dtype=np.float64), np.asarray(self.H, dtype=np.float64),
                        layout="bin_major", device=self._device)
        res = np.sum(np.abs(self.data - WH))
        return 100.0 * res / np.sum(np.abs(self.data))

    def frobenius_norm(self):
        if hasattr(self, "H") and hasattr(self, "W"):
            e2 = frame_residuals(self.W, self.data, self.H, layout="bin_major", dtype="f64",
                                 device=self._device)
            return np.sqrt(np.sum(e2))
        return None

    def _init_h(self):
        self.H = np.random.random((self._num_bases, self._num_samples)) + 10 ** -4

    def _init_w(self):
        self.W = np.random.random((self._data_dimension, self._num_bases)) + 10 ** -4

    def _update_w(self):
        """pymf/nmf.py:72-76: W <- W (.) (data H^T) (/) (W H H^T + 1e-9), columns scaled to unit norm; in place.
        Host numpy: the dictionary update is not on the accelerated path."""
        W2 = np.dot(np.dot(self.W, self.H), self.H.T) + 10 ** -9
        self.W *= np.dot(self.data, self.H.T)
        self.W /= W2
        self.W /= np.sqrt(np.sum(self.W ** 2.0, axis=0))

    def _activation_solve(self, niter, check, info):
        """`niter` updates of H with W fixed, one native call.  info: also the counts and, with `check`, the error after every
        update and pymf's stop -> (H, info); else H alone"""
        kw = dict(check_every=1 if check else 0, stop_rule="pymf" if check else "none", tol=self._EPS, info=True) if info else {}
        return solve_activations(
            np.asarray(self.W, dtype=np.float64), np.asarray(self.data, dtype=np.float64),
            np.asarray(self.H, dtype=np.float64), layout="bin_major", iters=niter,
            eps_mode="add", eps=10 ** -9, init="given", algo=self._algo, device=self._device, **kw)

    def _factorize_on_device(self, niter, compute_err):
        """pymf/base.py:238-270 with compute_w=True in one native call: per iteration W, then H, then the error and
        the machine-epsilon stop test; W and H are updated in place"""
        if not hasattr(self, "W"):
            self._init_w()
        if not hasattr(self, "H"):
            self._init_h()
        if compute_err:
            self.ferr = np.zeros(niter)
        if niter <= 0:
            return
        W, H, info = learn_dictionary(
            np.asarray(self.data, dtype=np.float64), np.asarray(self.W, dtype=np.float64),
            np.asarray(self.H, dtype=np.float64), layout="bin_major", iters=niter, surface="pymf",
            check_every=1 if compute_err else 0, tol=self._EPS if compute_err else 0.0, dtype="f64",
            device=self._device, info=True)
        self.W[...] = W
        self.H[...] = H
        if compute_err:
            n = info["n_iter"]
            ferr = info["err"][1:1 + n]
            if n < niter or (n >= 3 and abs(ferr[n - 1] - ferr[n - 2]) / self._num_samples < self._EPS):
                self.ferr = ferr[:n - 1].copy()     # base.py:268: ferr = ferr[:i], i = n - 1
            else:
                self.ferr[:n] = ferr
            for i, e in enumerate(self.ferr):
                self._logger.info("FN: %s (%s/%s)" % (e, i + 1, niter))

    def _factorize_with_dictionary_update(self, niter, compute_h, compute_err):
        """pymf/base.py:238-270 with compute_w=True: per iteration W (host), then H (one update on the GPU), then the
        error and the machine-epsilon stop test"""
        import warnings
        warnings.warn("pymf's dictionary update (compute_w=True) is outside the accelerated path: it runs in numpy on "
                      "the host, one GPU activation update per iteration; pass compute_w=False for the fixed-dictionary "
                      "solve", RuntimeWarning, stacklevel=3)
        if not hasattr(self, "W"):
            self._init_w()
        if not hasattr(self, "H") and compute_h:
            self._init_h()
        self.W = np.asarray(self.W, dtype=np.float64)
        if compute_err:
            self.ferr = np.zeros(niter)
        for i in range(niter):
            self._update_w()
            if compute_h:
                self.H[...] = self._activation_solve(1, False, False)
            if compute_err:
                self.ferr[i] = self.frobenius_norm()
                self._logger.info("FN: %s (%s/%s)" % (self.ferr[i], i + 1, niter))
                if i > 1 and np.abs(self.ferr[i] - self.ferr[i - 1]) / self._num_samples < self._EPS:
                    self.ferr = self.ferr[:i]
                    break
            else:
                self._logger.info("Iteration: (%s/%s)" % (i + 1, niter))

    def factorize(self, niter=100, show_progress=False, compute_w=True, compute_h=True,
                  compute_err=True):
        if show_progress:
            self._logger.setLevel(logging.INFO)
        else:
            self._logger.setLevel(logging.ERROR)
        if compute_w and compute_h and self._dictionary_update == "device":
            return self._factorize_on_device(niter, compute_err)
        if compute_w:
            return self._factorize_with_dictionary_update(niter, compute_h, compute_err)
        if not hasattr(self, "W"):
            raise AttributeError("set .W (data_dimension x num_bases) before factorize(compute_w=False)")
        if not hasattr(self, "H") and compute_h:
            self._init_h()
        if compute_err:
            self.ferr = np.zeros(niter)
        if not compute_h or niter <= 0:
            return
        H, info = self._activation_solve(niter, compute_err, True)
        self.H[...] = H                     # in place, like `self.H *= ...; self.H /= ...`
        if compute_err:
            n = int(info["n_iter"][0])      # updates applied
            ferr = info["err"][0, 1:1 + n]
            stopped = n < niter or (n >= 3 and abs(ferr[n - 1] - ferr[n - 2]) / self._num_samples < self._EPS)
            if stopped:
                self.ferr = ferr[:n - 1].copy()   # base.py:268: ferr = ferr[:i], i = n-1
            else:
                self.ferr[:n] = ferr
            for i, e in enumerate(self.ferr):
                self._logger.info("FN: %s (%s/%s)" % (e, i + 1, niter))


class SNMF(NMF):
    """pymf's SNMF(data, num_bases): semi-NMF, data ~ W H with signed data and W and H >= 0 (pymf/snmf.py:21-85).  The loop,
    `ferr` and the stop are NMF's (pymf/base.py); the two updates are its own."""

    def __init__(self, data, num_bases=4, **kwargs):
        NMF.__init__(self, data, num_bases, **kwargs)
        if self._dictionary_update != "host":
            raise ValueError("SNMF updates its dictionary on the host only")

    def _update_w(self):
        """pymf/snmf.py:61-64: W = data H^T (H H^T)^-1.  Host numpy: outside the accelerated path."""
        W1 = np.dot(self.data[:, :], self.H.T)
        W2 = np.dot(self.H, self.H.T)
        self.W = np.dot(W1, np.linalg.inv(W2))

    def _activation_solve(self, niter, check, info):
        """pymf/snmf.py:66-85, `niter` times in one native call (evc_semi_solve)"""
        kw = dict(check_every=1 if check else 0, stop_rule="pymf" if check else "none", tol=self._EPS, info=True) if info else {}
        return solve_activations_semi(
            np.asarray(self.W, dtype=np.float64), np.asarray(self.data, dtype=np.float64),
            np.asarray(self.H, dtype=np.float64), layout="bin_major", iters=niter, eps=10 ** -9, init="given", dtype="f64",
            device=self._device, **kw)


def kmeans_assign(data, num_bases, niter=10):
    """pymf's Kmeans(data, num_bases).factorize(niter=10).assigned (pymf/kmeans.py, pymf/dist.py:54-127, base.py:238-270) in
    numpy on the host: centres drawn by random.sample (the global `random` state), every sample assigned to the nearest
    centre (Euclidean, the first of equals), centres moved to their samples' means (an empty cluster keeps its centre),
    at most `niter` rounds, stopped by base.py's machine-epsilon test on ||data - W H||_F."""
    import random
    data = np.asarray(data)
    T = data.shape[1]
    sel = random.sample(range(T), num_bases)
    W = data[:, np.sort(sel)]

    def vq():
        d = np.zeros((num_bases, T))
        for a in range(num_bases):
            d[a:a + 1, :] = np.sqrt(((data[:, :] - W[:, a:a + 1]) ** 2.0).sum(axis=0)).reshape((1, -1))
        return np.argmin(d, axis=0)

    assigned = vq()
    ferr = np.zeros(niter)
    for i in range(niter):
        for k in range(num_bases):
            idx = assigned == k
            n = np.sum(idx)
            if n > 0:
                W[:, k] = np.sum(data[:, idx], axis=1) / n
        assigned = vq()
        H = np.zeros((num_bases, T))
        H[assigned, range(T)] = 1.0
        ferr[i] = np.sqrt(np.sum((data[:, :] - np.dot(W, H)) ** 2))
        if i > 1 and np.abs(ferr[i] - ferr[i - 1]) / T < _EPS:
            break
    return assigned


class Kmeans(NMF):
    """pymf's Kmeans(data, num_bases): data ~ W H with H one-hot and every column of W the mean of its samples (pymf/kmeans.py:14-83
    on base.py:208-270).  factorize() is one native call (evc_kmeans): the centres drawn by random.sample (the global `random`
    state, sorted) unless .W is set, one assignment, then per round the means, the assignment and ||data - W H||_F with
    base.py's machine-epsilon stop.  `W`, `H` (one-hot float64), `assigned` and `ferr` are left as pymf leaves them;
    compute_w=False assigns against the given .W (pymf's vq).  The assignment always starts from the current .W: an .H set by
    hand is not read."""

    def __init__(self, data, num_bases=4, **kwargs):
        NMF.__init__(self, data, num_bases, **kwargs)
        if self._dictionary_update != "host":
            raise ValueError("Kmeans has no dictionary_update option: centres and labels are always updated on the device")

    def _init_w(self):
        """kmeans.py:62-67: some random data samples, their indices sorted"""
        import random
        sel = random.sample(range(self._num_samples), self._num_bases)
        self.W = np.asarray(self.data)[:, np.sort(sel)]

    def _init_h(self):
        self.factorize(niter=0, compute_w=False, compute_err=False)

    def factorize(self, niter=100, show_progress=False, compute_w=True, compute_h=True, compute_err=True):
        if show_progress:
            self._logger.setLevel(logging.INFO)
        else:
            self._logger.setLevel(logging.ERROR)
        if not compute_h:
            raise NotImplementedError("Kmeans.factorize(compute_h=False): the assignment is the factorisation; only "
                                      "compute_w=False (vq against fixed centres) is offered besides the default")
        if not hasattr(self, "W"):
            if not compute_w:
                raise AttributeError("set .W (data_dimension x num_bases) before factorize(compute_w=False)")
            self._init_w()
        data = np.asarray(self.data, dtype=np.float64)
        W, assigned, info = kmeans(data, np.asarray(self.W, dtype=np.float64), layout="bin_major", iters=max(int(niter), 0),
                                   stop="pymf" if compute_err else "none", tol=self._EPS, update="both" if compute_w else "assign",
                                   dtype="f64", device=self._device, info=True)
        if compute_w:
            if isinstance(self.W, np.ndarray) and self.W.dtype == np.float64:
                self.W[...] = W                  # in place, like `self.W[:, i] = ...`
            else:
                self.W = W
        self.assigned = assigned.astype(np.int64)
        self.H = np.zeros((self._num_bases, self._num_samples))
        self.H[self.assigned, np.arange(self._num_samples)] = 1.0
        if compute_err:
            self.ferr = np.zeros(max(int(niter), 0))
            n = info["n_iter"]
            ferr = info["err"][1:1 + n]
            if n < niter or (n >= 3 and abs(ferr[n - 1] - ferr[n - 2]) / self._num_samples < self._EPS):
                self.ferr = ferr[:n - 1].copy()     # base.py:268: ferr = ferr[:i], i = n - 1
            else:
                self.ferr[:n] = ferr
            for i, e in enumerate(self.ferr):
                self._logger.info("FN: %s (%s/%s)" % (e, i + 1, niter))


class CNMF(NMF):
    """pymf's CNMF(data, num_bases): convex NMF, data ~ W H with W = data G, signed data and G, H >= 0 (pymf/cnmf.py:18-175).
    `G` is num_samples x num_bases.  factorize() is one native call (evc_convex_learn): per iteration H, then G with the
    new H, then the error and base.py's machine-epsilon stop; `W`, `G`, `H` and `ferr` are left as pymf leaves them."""

    def __init__(self, data, num_bases=4, **kwargs):
        NMF.__init__(self, data, num_bases, **kwargs)
        if self._dictionary_update != "host":
            raise ValueError("CNMF has no dictionary_update option: both factors are always updated on the device")
        self._start = kwargs.get("start", "host")
        if self._start not in ("host", "device"):
            raise ValueError("start must be 'host' or 'device'")

    def _kmeans_start(self):
        """the labels of pymf's Kmeans(data, num_bases).factorize(niter=10): on the host in numpy, or (start="device") the
        same random.sample draw and evc_kmeans"""
        if self._start == "host":
            return kmeans_assign(self.data, self._num_bases, 10)
        mdl = Kmeans(self.data, self._num_bases, device=self._device)
        mdl.factorize(niter=10)
        return mdl.assigned

    def _init_h(self):
        """cnmf.py:67-92: H and G from a k-means clustering of the samples, W = data G"""
        need_h, need_g = not hasattr(self, "H"), not hasattr(self, "G")
        if need_g and not need_h:
            raise AttributeError("set .G (num_samples x num_bases) along with .H: pymf builds G only from its own k-means start")
        if need_h:
            assign = self._kmeans_start()
            G0, self.H = convex_cluster_start(assign, self._num_bases)
            if need_g:
                self.G = G0
        if not hasattr(self, "W"):
            self.W = np.dot(self.data[:, :], self.G)

    def _init_w(self):
        pass

    def factorize(self, niter=10, compute_w=True, compute_h=True, compute_err=True, show_progress=False):
        if show_progress:
            self._logger.setLevel(logging.INFO)
        else:
            self._logger.setLevel(logging.ERROR)
        if not hasattr(self, "H") or not hasattr(self, "G"):
            self._init_h()
        data = np.asarray(self.data, dtype=np.float64)
        G, H = np.asarray(self.G, dtype=np.float64), np.asarray(self.H, dtype=np.float64)
        XG = np.dot(data, G)
        if not hasattr(self, "W"):
            self.W = XG
        elif not compute_w and not np.allclose(np.asarray(self.W, dtype=np.float64), XG, rtol=1e-10,
                                               atol=1e-12 * max(float(np.abs(XG).max()), 1e-300)):
            raise NotImplementedError("factorize(compute_w=False) with a W that is not data G: pymf then measures ferr against "
                                      "the stale W while it updates H for data G; evc_convex_learn always measures "
                                      "||data - (data G) H||.  Set W = data G, or leave W unset")
        self.ferr = np.zeros(niter)
        if niter <= 0:
            return
        if not compute_w and not compute_h:           # nothing moves: the error repeats and base.py's test fires at i = 2
            if compute_err:
                err = float(np.sqrt(np.sum((data - np.dot(np.asarray(self.W, dtype=np.float64), H)) ** 2)))
                self.ferr = np.full(min(niter, 2), err) if niter >= 3 else np.full(niter, err)
            return
        update = "both" if compute_w and compute_h else ("h" if compute_h else "g")
        W, G, H, info = learn_dictionary_convex(data, G, H, layout="bin_major", iters=niter, update=update,
                                                check_every=1 if compute_err else 0, tol=self._EPS if compute_err else 0.0,
                                                eps=10 ** -9, dtype="f64", device=self._device, info=True)
        if compute_w:
            if isinstance(self.G, np.ndarray) and self.G.dtype == np.float64:
                self.G[...] = G                  # in place, like `self.G *= ...`
            else:
                self.G = G
            self.W = W
        if compute_h:
            self.H = H
        if compute_err:
            n = info["n_iter"]
            ferr = info["err"][1:1 + n]
            if n < niter or (n >= 3 and abs(ferr[n - 1] - ferr[n - 2]) / self._num_samples < self._EPS):
                self.ferr = ferr[:n - 1].copy()     # cnmf.py:174: ferr = ferr[:i], i = n - 1
            else:
                self.ferr[:n] = ferr
            for i, e in enumerate(self.ferr):
                self._logger.info("FN: %s (%s/%s)" % (e, i + 1, niter))
