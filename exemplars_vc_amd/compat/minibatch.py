"""scikit-learn's `MiniBatchNMF` estimator on the GPU, in scikit-learn's orientation: X (n_samples, n_features), W
(n_samples, n_components) the activations, components_ (n_components, n_features) the dictionary.

    est = MiniBatchNMF(n_components=R, init="custom", beta_loss=..., ...)
    W = est.fit_transform(X, W=W0, H=H0)      evc_online_learn, or evc_online_learn_fresh with fresh_restarts=True
    W2 = est.transform(X2)                    evc_online_transform
    est.partial_fit(chunk, H=H0)              one step of evc_online_learn_fresh per call; components_ and the statistics
                                              A, B stay on the device between calls

Only init='custom' is served (the nndsvd family is out of scope), dense X, unshuffled batches, at most 528 features.
random_state and verbose are accepted and unused.  beta <= 0 refuses zeros in X as scikit-learn does."""
import numpy as np

from ..solver import _torch, learn_dictionary_online, require_device, solve_activations_beta, transform_online
from .factorize import _beta_of, _check_beta_zeros


class MiniBatchNMF:
    def __init__(self, n_components="auto", *, init="custom", batch_size=1024, beta_loss="frobenius", tol=1e-4,
                 max_no_improvement=10, max_iter=200, alpha_W=0.0, alpha_H="same", l1_ratio=0.0, forget_factor=0.7,
                 fresh_restarts=False, fresh_restarts_max_iter=30, transform_max_iter=None, random_state=None, verbose=0,
                 device=None):
        if init != "custom":
            raise ValueError(f"init={init!r} is out of scope here (nndsvd and random starts are not served): pass "
                             "init='custom' and give W and H")
        self.n_components, self.init, self.batch_size, self.beta_loss, self.tol = n_components, init, batch_size, beta_loss, tol
        self.max_no_improvement, self.max_iter, self.alpha_W, self.alpha_H = max_no_improvement, max_iter, alpha_W, alpha_H
        self.l1_ratio, self.forget_factor, self.fresh_restarts = l1_ratio, forget_factor, fresh_restarts
        self.fresh_restarts_max_iter, self.transform_max_iter = fresh_restarts_max_iter, transform_max_iter
        self.random_state, self.verbose, self.device = random_state, verbose, device

    # ---- what every entry shares ----
    def _data(self, X, reset):
        X = np.asarray(X)
        if X.ndim != 2:
            raise ValueError(f"Expected 2D array, got {X.ndim}D array instead")
        beta = _beta_of(self.beta_loss)
        _check_beta_zeros(X, beta)
        if X.dtype not in (np.float64, np.float32):
            X = X.astype(np.float64)
        if reset:
            self.n_features_in_ = X.shape[1]
        elif X.shape[1] != self.n_features_in_:
            raise ValueError(f"X has {X.shape[1]} features, but MiniBatchNMF is expecting {self.n_features_in_} features as input.")
        return X, beta

    def _penalties(self, n_features):
        """(l1_h, l2_h, l1_w, l2_w) as the C ABI takes them: the activations' scaled by the features, the dictionary's per
        sample (each step multiplies them by its batch's samples, as _compute_regularization does)"""
        a_w = float(self.alpha_W)
        a_h = a_w if isinstance(self.alpha_H, str) and self.alpha_H == "same" else float(self.alpha_H)
        r = float(self.l1_ratio)
        return n_features * a_w * r, n_features * a_w * (1.0 - r), a_h * r, a_h * (1.0 - r)

    def _components_device(self, dtype):
        torch = _torch()
        return self._components_d.to(torch.float64 if dtype == np.float64 else torch.float32)

    def _custom(self, X, W, H):
        if H is None:
            raise ValueError("init='custom' needs H (the dictionary, n_components x n_features)")
        H = np.asarray(H, dtype=X.dtype)
        if self.n_components not in (None, "auto") and H.shape[0] != self.n_components:
            raise ValueError(f"H has {H.shape[0]} components, n_components is {self.n_components}")
        if W is not None and np.asarray(W).shape != (X.shape[0], H.shape[0]):
            raise ValueError(f"W has shape {np.asarray(W).shape}, expected {(X.shape[0], H.shape[0])}")
        return H

    # ---- the estimator's surface ----
    def fit_transform(self, X, y=None, W=None, H=None):
        X, beta = self._data(X, True)
        H = self._custom(X, W, H)
        if W is None and not self.fresh_restarts:
            raise ValueError("init='custom' without fresh restarts needs W (the start of the activations)")
        l1_h, l2_h, l1_w, l2_w = self._penalties(X.shape[1])
        dev = require_device(self.device)
        torch = _torch()
        Xd, Hd = torch.from_numpy(np.ascontiguousarray(X)).to(dev), torch.from_numpy(np.ascontiguousarray(H)).to(dev)
        Wd = None if W is None else torch.from_numpy(np.ascontiguousarray(np.asarray(W, dtype=X.dtype))).to(dev)
        comp, act, info = learn_dictionary_online(
            Xd, Hd, Wd, beta=beta, layout="frame_major", batch_size=int(self.batch_size), max_iter=int(self.max_iter),
            forget_factor=float(self.forget_factor), tol=float(self.tol), max_no_improvement=self.max_no_improvement, l1_h=l1_h,
            l2_h=l2_h, l1_w=l1_w, l2_w=l2_w, device=dev, info=True, fresh_restarts=bool(self.fresh_restarts),
            fresh_restarts_max_iter=int(self.fresh_restarts_max_iter), transform_max_iter=self.transform_max_iter)
        self._components_d, self._state = comp, info["state"]
        self._rho = float(self.forget_factor) ** (min(int(self.batch_size), X.shape[0]) / X.shape[0])
        self.n_components_, self.n_iter_, self.n_steps_ = comp.shape[0], info["n_iter"], info["n_steps"]
        self.reconstruction_err_ = self._reconstruction_err(Xd, act, beta)
        return act.cpu().numpy()

    def fit(self, X, y=None, **params):
        self.fit_transform(X, **params)
        return self

    def transform(self, X):
        if not hasattr(self, "_components_d"):
            raise RuntimeError("This MiniBatchNMF instance is not fitted yet")
        X, beta = self._data(X, False)
        l1_h, l2_h, _, _ = self._penalties(X.shape[1])
        K = int(self.max_iter if self.transform_max_iter is None else self.transform_max_iter)
        return transform_online(self._components_device(X.dtype), X, beta=beta, layout="frame_major", max_iter=K,
                                tol=float(self.tol), l1=l1_h, l2=l2_h, device=self.device)

    def partial_fit(self, X, y=None, W=None, H=None):
        first = not hasattr(self, "_components_d")
        X, beta = self._data(X, first)
        dev = require_device(self.device)
        torch = _torch()
        if first:
            H = self._custom(X, W, H)
            self._components_d = torch.from_numpy(np.ascontiguousarray(H)).to(dev)
            self._state = None
            self._rho = float(self.forget_factor) ** (min(int(self.batch_size), X.shape[0]) / X.shape[0])      # fixed here
            self.n_steps_ = 0
        l1_h, l2_h, l1_w, l2_w = self._penalties(X.shape[1])
        comp = self._components_device(X.dtype)
        comp, _, info = learn_dictionary_online(
            torch.from_numpy(np.ascontiguousarray(X)).to(dev), comp, None, beta=beta, layout="frame_major",
            batch_size=X.shape[0], max_iter=1, forget_factor=self._rho, tol=float(self.tol), max_no_improvement=None, l1_h=l1_h,
            l2_h=l2_h, l1_w=l1_w, l2_w=l2_w, state=self._state, device=dev, info=True, fresh_restarts=True,
            fresh_restarts_max_iter=int(self.fresh_restarts_max_iter), transform_max_iter=0)
        self._components_d, self._state = comp, info["state"]
        self.n_components_ = comp.shape[0]
        self.n_steps_ += 1
        return self

    def inverse_transform(self, X):
        return np.asarray(X) @ self.components_

    @property
    def components_(self):
        if not hasattr(self, "_components_d"):
            raise AttributeError("components_")
        return self._components_d.cpu().numpy()

    def _reconstruction_err(self, Xd, act, beta):
        """_beta_divergence(X, W, H, beta, square_root=True): the start error of an activation solve of no iterations"""
        _, info = solve_activations_beta(self._components_d, Xd, act, beta=beta, layout="frame_major", iters=0, check_every=1,
                                         init="given", device=self.device, info=True)
        return float(info["err"][0, 0])
