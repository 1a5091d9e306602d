"""The coordinate-descent variant of the activation solve, on the GPU.

Mirrors the reference's 04_align_n_nmf_pytorch.py (despite its name it holds no torch):
  _factorize(X, W, beta_loss, tol)   :189-210   (sklearn non_negative_factorization, init="custom",
                                                 update_H=False, solver='cd', max_iter=200)
  factorize(tobe_converted, src_feat) :213-289   (one solve per feature stream; returns the H dict only)
Its convert() (:292-327) is the existing synthesis (compat.factorize.synthesize_rows / convert).
Argument meaning, return orientation, errors and warnings follow scikit-learn 1.7.2 (_check_init, the dtype
check, ConvergenceWarning when max_iter is reached with tol > 0, _nmf.py:1727-1732).
"""
from __future__ import annotations

import warnings

import numpy as np

from ..solver import learn_dictionary_cd, solve_activations_cd
from .factorize import ConvergenceWarning, _check_dictionary, _stack

MAX_ITER = 200          # 04_align_n_nmf_pytorch.py:207-208


def _check_frames(X):
    X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError(f"Expected 2D array, got {X.ndim}D array instead")
    if not np.all(np.isfinite(X)):
        raise ValueError("Input contains NaN or infinity.")
    if (X < 0).any():       # scikit-learn does not check X on this route either
        warnings.warn("X has negative entries; coordinate descent is only meaningful for non-negative data",
                      RuntimeWarning, stacklevel=3)
    if X.dtype not in (np.float64, np.float32):
        X = X.astype(np.float64)
    return X


def _reg(n_features, alpha_W, l1_ratio):
    """sklearn's _compute_regularization for W: (l1_reg_W, l2_reg_W)."""
    return n_features * alpha_W * l1_ratio, n_features * alpha_W * (1.0 - l1_ratio)


def _factorize(X, W, beta_loss="kullback-leibler", tol=1e-4, *, device=None, alpha_W=0.0, l1_ratio=0.0,
               max_iter=MAX_ITER, warn_sink=None):
    """H (N x T) with W.T @ H ~ X.T by sklearn's coordinate descent.  X: (T, M) frames as rows, W: (N, M)
    exemplars as rows.  As in the reference the Frobenius loss is forced whatever `beta_loss` says (:205); the
    activations start at 0; the loop stops per sklearn's violation rule, at most 200 iterations.
    alpha_W / l1_ratio: sklearn's regularisation (the script passes none)."""
    X = _check_frames(X)
    W = _check_dictionary(W, X.shape[1])
    if W.dtype != X.dtype:
        raise TypeError(f"H should have the same dtype as X. Got H.dtype = {W.dtype}.")
    l1, l2 = _reg(X.shape[1], alpha_W, l1_ratio)
    act, info = solve_activations_cd(W, X, layout="frame_major", max_iter=max_iter, tol=tol, l1=l1, l2=l2,
                                     device=device, info=True)
    _warn_if_capped(int(info["n_iter"][0]), max_iter, tol, warn_sink)
    return act.T


def _warn_if_capped(n_iter, max_iter, tol, warn_sink=None):
    if n_iter == max_iter and tol > 0:
        msg = f"Maximum number of iterations {max_iter} reached. Increase it to improve convergence."
        if warn_sink is not None:
            warn_sink.append(msg)
        else:
            warnings.warn(msg, ConvergenceWarning, stacklevel=3)


def non_negative_factorization_cd(X, W, H, update_H=True, tol=1e-4, max_iter=200, alpha_W=0.0, alpha_H="same",
                                  l1_ratio=0.0, *, device=None):
    """scikit-learn's non_negative_factorization(X, W, H, init="custom", solver="cd", beta_loss="frobenius",
    shuffle=False) on the GPU, in scikit-learn's orientation: X (n_samples, n_features), W (n_samples, n_components),
    H (n_components, n_features), X ~ W H.  update_H=True (NMF(...).fit_transform, 05_conversion.py:100-106) updates both
    factors from the given starts (evc_cd_learn); update_H=False is the existing fixed-dictionary solve, which starts W at
    0 as scikit-learn does.  The penalties are scaled as _compute_regularization does: l1_reg_W = n_features alpha_W
    l1_ratio, l1_reg_H = n_samples alpha_H l1_ratio (alpha_H="same": alpha_W), likewise l2 with (1 - l1_ratio).
    Returns (W, H, n_iter); ConvergenceWarning when max_iter is reached with tol > 0."""
    X = _check_frames(X)
    H = _check_dictionary(H, X.shape[1])
    if H.dtype != X.dtype:
        raise TypeError(f"H should have the same dtype as X. Got H.dtype = {H.dtype}.")
    n_samples, n_features = X.shape
    l1_h, l2_h = _reg(n_features, alpha_W, l1_ratio)
    if not update_H:
        act, info = solve_activations_cd(H, X, layout="frame_major", max_iter=max_iter, tol=tol, l1=l1_h, l2=l2_h,
                                         device=device, info=True)
        n_iter = int(info["n_iter"][0])
        _warn_if_capped(n_iter, max_iter, tol)
        return act, H, n_iter
    W = np.asarray(W)
    if W.shape != (n_samples, H.shape[0]):
        raise ValueError(f"Array with wrong shape passed to NMF (input W). Expected {(n_samples, H.shape[0])}, "
                         f"but got {W.shape}")
    if W.dtype != X.dtype:
        raise TypeError(f"W should have the same dtype as X. Got W.dtype = {W.dtype}.")
    if not np.all(np.isfinite(W)) or (W < 0).any():
        raise ValueError("Negative or non-finite values in data passed to NMF (input W)")
    l1_w, l2_w = _reg(n_samples, alpha_W if isinstance(alpha_H, str) and alpha_H == "same" else alpha_H, l1_ratio)
    Wd, act, info = learn_dictionary_cd(X, H, W, layout="frame_major", max_iter=max_iter, tol=tol, l1_h=l1_h, l2_h=l2_h,
                                        l1_w=l1_w, l2_w=l2_w, device=device, info=True)
    _warn_if_capped(info["n_iter"], max_iter, tol)
    return act, Wd, info["n_iter"]


def factorize_utterances(X_list, W, tol=1e-4, *, device=None, max_iter=MAX_ITER, alpha_W=0.0, l1_ratio=0.0,
                         return_info=False):
    """`_factorize` for many utterances in ONE call: the frames are concatenated and the per-call semantics (zero
    start, stop rule) apply per utterance on the device; each utterance's activations are bitwise those of its own
    call.  Returns a list of (N x T_u) arrays and the per-utterance iteration counts (return_info: also the info
    dict).  ConvergenceWarning once if any utterance ran to max_iter with tol > 0."""
    X_list = [_check_frames(x) for x in X_list]
    W = _check_dictionary(W, X_list[0].shape[1])
    for x in X_list:
        if x.shape[1] != W.shape[1]:
            raise ValueError(f"every utterance needs {W.shape[1]} bins, got {x.shape[1]}")
        if x.dtype != W.dtype:
            raise TypeError(f"H should have the same dtype as X. Got H.dtype = {W.dtype}.")
    offs = np.concatenate([[0], np.cumsum([x.shape[0] for x in X_list])]).astype(np.int32)
    X = np.concatenate(X_list, axis=0)
    l1, l2 = _reg(W.shape[1], alpha_W, l1_ratio)
    act, info = solve_activations_cd(W, X, layout="frame_major", max_iter=max_iter, tol=tol, l1=l1, l2=l2,
                                     utt_offsets=offs, device=device, info=True)
    if (info["n_iter"] == max_iter).any():
        _warn_if_capped(max_iter, max_iter, tol)
    out = [act[offs[i]:offs[i + 1]].T for i in range(len(X_list))]
    return (out, info["n_iter"], info) if return_info else (out, info["n_iter"])


def factorize(tobe_converted, src_feat, *, use_stft=True, tol=1e-4, device=None, concurrent=True):
    """`factorize(tobe_converted, src_feat)` of 04_align_n_nmf_pytorch.py:213-289 without its pickle cache: stack the
    aligned source exemplars into a dictionary per stream and solve the activations of the utterance.  Returns the H
    dict only (this script forms no residual).

      use_stft=True : {'H_stft': N x T}.  The script reads tobe_converted['real'] but stacks src_feat[i]['stft']
                      (complex, which sklearn rejects); as in compat.factorize, the dictionary is stacked from
                      |src_feat[i]['real']| and the frames are |tobe_converted['real']|.
      use_stft=False: {'H_sp', 'H_ap', 'H_f0'} from 'sp', 'ap' (T x 513) and 'f0' (T,).  The three solves run
                      concurrently on side streams (concurrent=False: one after the other); the coordinate-descent
                      kernels exchange nothing between workgroups, so concurrent solves cannot starve each other.
    """
    if use_stft:
        conv = np.abs(np.asarray(tobe_converted["real"]))
        return {"H_stft": _factorize(conv, _stack(src_feat, "real", np.abs), tol=tol, device=device)}
    streams = {"sp": (np.asarray(tobe_converted["sp"]), _stack(src_feat, "sp")),
               "ap": (np.asarray(tobe_converted["ap"]), _stack(src_feat, "ap")),
               "f0": (np.asarray(tobe_converted["f0"])[:, np.newaxis], _stack(src_feat, "f0"))}
    if not concurrent:
        return {"H_" + n: _factorize(conv, A, tol=tol, device=device) for n, (conv, A) in streams.items()}
    return _solve_streams(streams, tol, device)


_side_streams = {}      # (device index, slot) -> torch.cuda.Stream, reused (and so is the solver's per-stream scratch)


def _solve_streams(streams, tol, device):
    """one host thread and one HIP stream per feature stream; warnings are issued by the caller's thread after the
    join, the first exception is re-raised"""
    import threading
    import torch
    from ..solver import require_device
    dev = require_device(device)
    H, caught, errors = {}, {}, {}

    def work(name, conv, A, slot):
        try:
            torch.cuda.set_device(dev)
            st = _side_streams.get((dev.index, slot))
            if st is None:
                st = _side_streams[(dev.index, slot)] = torch.cuda.Stream(device=dev)
            sink = []
            with torch.cuda.stream(st):
                H["H_" + name] = _factorize(conv, A, tol=tol, device=dev, warn_sink=sink)
            caught[name] = sink
        except BaseException as e:  # noqa: BLE001 - handed to the caller's thread
            errors[name] = e

    names = list(streams)
    threads = [threading.Thread(target=work, args=(n, *streams[n], k + 1)) for k, n in enumerate(names[1:])]
    for t in threads:
        t.start()
    work(names[0], *streams[names[0]], 0)
    for t in threads:
        t.join()
    for n in names:
        if n in errors:
            raise errors[n]
        for msg in caught.get(n, ()):
            warnings.warn(msg, ConvergenceWarning, stacklevel=3)
    return {"H_" + n: H["H_" + n] for n in names}
