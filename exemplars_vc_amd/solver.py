"""Host-side plumbing for the HIP activation solver: device buffers, streams, workspace.

PyTorch is used for device memory and stream handles only; all arithmetic happens in
libevc_hip.so (hand-written gfx950 kernels) behind the C ABI of include/evc.h.

Orientation (`layout`):
  "bin_major"   - north_star / pymf / nmf_tool: A (M,N), X (M,T), H (N,T), B (Mb,N), Y (Mb,T)
  "frame_major" - the reference scripts (04_align_n_nmf.py): A (N,M), X (T,M), H (T,N),
                  B (N,Mb), Y (T,Mb)
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import threading
import types
from typing import Optional, Sequence

import numpy as np

from . import _lib

_EPS_MODES = {"add": _lib.EPS_ADD, "zero_replace": _lib.EPS_ZERO_REPLACE, "none": _lib.EPS_NONE,
              "clamp": _lib.EPS_CLAMP}
_EPS_DEFAULT = {"add": 1e-9, "zero_replace": float(np.finfo(np.float32).eps), "none": 0.0,
                "clamp": 1e-15}
_ALGOS = {"gram": _lib.ALGO_GRAM, "factored": _lib.ALGO_FACTORED, "literal": _lib.ALGO_LITERAL,
          "auto": _lib.ALGO_AUTO}
_INITS = {"given": _lib.INIT_GIVEN, "sklearn": _lib.INIT_SKLEARN, "const": _lib.INIT_CONST}
_STOPS = {"none": _lib.STOP_NONE, "sklearn": _lib.STOP_SKLEARN, "pymf": _lib.STOP_PYMF}
_PROX_STOPS = {"none": _lib.STOP_NONE, "decomp": _lib.STOP_DECOMP}      # evc_prox_solve's own: no other entry takes "decomp"
_PROX_MOMENTA = {"ista": _lib.PROX_ISTA, "fista": _lib.PROX_FISTA, "nesterov": _lib.PROX_NESTEROV}
_LAYOUTS = {"frame_major": _lib.FRAME_MAJOR, "bin_major": _lib.BIN_MAJOR}
_LOSSES = {"frobenius": _lib.LOSS_FROBENIUS, "kullback-leibler": _lib.LOSS_KL, "kl": _lib.LOSS_KL}

# scratch memory handed to the C ABI, one buffer per (device, stream): include/evc.h promises that calls on
# distinct streams are independent, so two streams (or two host threads on two streams) must never share
# scratch.  A buffer belongs to the stream it was allocated on (torch's allocator is stream-ordered), so
# growing it is safe: the old block is only reused by later work of the same stream.
_workspaces = {}
_ws_lock = threading.Lock()


def _torch():
    import torch
    return torch


def require_device(device=None):
    """Resolve the HIP device to run on; raise if there is none (no CPU fallback)."""
    torch = _torch()
    _lib.lib()  # fail early and loudly when the native library is missing
    if not torch.cuda.is_available():
        raise RuntimeError("exemplars_vc_amd needs a HIP device (torch.cuda.is_available() is False); "
                           "there is no CPU fallback")
    if device is None:
        return torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"exemplars_vc_amd runs on HIP devices only, got {device}")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


class _Scratch:
    def __init__(self):
        self.lock = threading.Lock()
        self.buf = None


@contextlib.contextmanager
def _workspace(nbytes: int, device):
    """The scratch buffer of (device, current stream), held for the duration of one native call."""
    torch = _torch()
    key = (device.index, int(torch.cuda.current_stream(device).cuda_stream))
    with _ws_lock:
        slot = _workspaces.get(key)
        if slot is None:
            slot = _workspaces[key] = _Scratch()
    with slot.lock:
        if slot.buf is None or slot.buf.numel() < nbytes:
            slot.buf = None
            with torch.cuda.device(device):
                slot.buf = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
        yield slot.buf


def release_workspaces():
    with _ws_lock:
        _workspaces.clear()


def _to_dev(x, tdtype, device):
    """2-D array/tensor -> device tensor with unit inner stride; returns (tensor, was_numpy)."""
    torch = _torch()
    was_numpy = not isinstance(x, torch.Tensor)
    if was_numpy:
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
    if x.dim() != 2:
        raise ValueError(f"expected a 2-D matrix, got shape {tuple(x.shape)}")
    x = x.to(device=device, dtype=tdtype)
    if x.shape[1] > 1 and x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        x = x.contiguous()
    return x, was_numpy


def _to_host(t):
    """Device tensor -> numpy.  Large results go through page-locked memory (torch caches the pinned
    blocks): a pageable download of one utterance's activations (22 MB) costs as much as its solve."""
    torch = _torch()
    if t.numel() * t.element_size() < (1 << 20):
        return t.cpu().numpy()
    t = t.contiguous()
    host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    host.copy_(t, non_blocking=True)
    torch.cuda.current_stream(t.device).synchronize()
    return host.numpy()


def _ld(x):
    return int(x.stride(0)) if x.shape[0] > 1 else int(max(x.shape[1], 1))


def _pick_dtype(dtype, *arrs):
    torch = _torch()
    if dtype is None:
        for a in arrs:
            if a is None:
                continue
            dt = a.dtype
            if dt in (np.float32, torch.float32):
                return torch.float32, _lib.F32
            break
        return torch.float64, _lib.F64
    if dtype in ("f32", "float32", np.float32, torch.float32):
        return torch.float32, _lib.F32
    if dtype in ("f64", "float64", np.float64, torch.float64, float):
        return torch.float64, _lib.F64
    raise ValueError(f"unsupported dtype {dtype!r}")


class PreparedDictionary:
    """A dictionary imported once into the layouts the kernels read (evc_dict_prepare): pass it in place of `A` (and
    leave `B` out) to solve_activations / convert.  The reference builds A and B once per run
    (04_align_n_nmf.py:230-246,350-361); results are bitwise those of the unprepared calls."""

    def __init__(self, handle, buf, layout, tdtype, dcode, device, loss, eps):
        self.handle, self._buf = handle, buf           # the device image must outlive the handle's uses
        self.layout, self.tdtype, self.dcode, self.device, self.loss, self.eps = layout, tdtype, dcode, device, loss, eps
        self.M, self.Mb, self.N = int(handle.M), int(handle.Mb), int(handle.N)


def prepare_dictionary(A, B=None, *, layout="bin_major", dtype=None, loss="frobenius", eps=None, device=None):
    """Import A (and the parallel target dictionary B) once; see PreparedDictionary."""
    torch = _torch()
    device = require_device(device)
    L = _lib.lib()
    lay = _LAYOUTS[layout]
    tdtype, dcode = _pick_dtype(dtype, A)
    A_d, _ = _to_dev(A, tdtype, device)
    M, N = A_d.shape if lay == _lib.BIN_MAJOR else A_d.shape[::-1]
    Mb, B_d = 0, None
    if B is not None:
        B_d, _ = _to_dev(B, tdtype, device)
        Mb, N2 = B_d.shape if lay == _lib.BIN_MAJOR else B_d.shape[::-1]
        if N2 != N:
            raise ValueError(f"A and B disagree on the number of exemplars: {N} vs {N2}")
    lcode = _LOSSES[loss]
    if eps is None:
        eps = _EPS_DEFAULT["zero_replace"] if lcode == _lib.LOSS_KL else 0.0
    nbytes = int(L.evc_dict_bytes(M, Mb, N, dcode, lcode))
    if nbytes == 0:
        raise ValueError("unsupported dictionary shape / dtype")
    with torch.cuda.device(device):
        buf = torch.empty(nbytes + 256, dtype=torch.uint8, device=device)
        off = (-buf.data_ptr()) % 256
        handle = _lib.Dict()
        st = L.evc_dict_prepare(A_d.data_ptr(), _ld(A_d), B_d.data_ptr() if B_d is not None else None,
                                _ld(B_d) if B_d is not None else 0, M, Mb, N, lay, dcode, lcode, float(eps),
                                buf.data_ptr() + off, nbytes, C.byref(handle),
                                C.c_void_p(torch.cuda.current_stream(device).cuda_stream))
    _lib.check(st, "evc_dict_prepare")
    # evc.h promises the images to later calls on the SAME stream only; a prepared dictionary is used from side streams
    # and other host threads (compat's three WORLD streams, cached_dictionary hits), so the packing kernels are waited
    # for here, once per dictionary
    torch.cuda.current_stream(device).synchronize()
    return PreparedDictionary(handle, buf, lay, tdtype, dcode, device, lcode, float(eps))


_dict_cache = {}


def cached_dictionary(A, B=None, **kw):
    """prepare_dictionary, remembered per (A, B) object identity: the compat surfaces take plain arrays, and a caller
    converting utterance after utterance against one dictionary passes the same arrays again.  The arrays are held
    weakly; an entry dies with them.  (Content is NOT hashed: mutate a dictionary in place and you must not use this.)"""
    import weakref
    key = (id(A), id(B) if B is not None else None, tuple(getattr(A, "shape", ())), str(getattr(A, "dtype", "")),
           tuple(sorted((k, str(v)) for k, v in kw.items())))
    ent = _dict_cache.get(key)
    if ent is not None and ent[1]() is A and (B is None or ent[2]() is B):
        return ent[0]
    pd = prepare_dictionary(A, B, **kw)
    try:
        ra = weakref.ref(A, lambda _r, k=key: _dict_cache.pop(k, None))
        rb = weakref.ref(B) if B is not None else None
    except TypeError:
        return pd
    if len(_dict_cache) >= 8:
        _dict_cache.pop(next(iter(_dict_cache)))
    _dict_cache[key] = (pd, ra, rb)
    return pd


def workspace_bytes(M, N, T, n_utt=1, dtype="f64", algo="auto", Mb=0):
    _, code = _pick_dtype(dtype)
    return int(_lib.lib().evc_workspace_bytes(M, Mb, N, T, n_utt, code, _ALGOS[algo]))


def solve_activations(A, X, H0=None, **kw):
    """H <- H (.) A^T X (/) guard(A^T A H + l1), `iters` times, on the GPU.

    Returns H in the caller's orientation (numpy in -> numpy out, device tensor in -> device
    tensor out); with info=True also a dict(n_iter=int array per utterance, err=array
    [n_utt, 1+iters//check_every] of residuals, NaN where not evaluated).
    Keywords: see `_solve`.
    """
    return _solve(A, X, H0, None, **kw)


def convert(A, X, B=None, H0=None, *, want_h=True, **kw):
    """Activation solve followed by the synthesis Y = B H in one launch sequence
    (factorize() + convert() of 04_align_n_nmf.py).  Returns (H, Y), or Y alone with
    want_h=False (the activations then never leave the solver's tile layout); with info=True
    the info dict is appended.  `A` may be a PreparedDictionary made with B: then leave B out."""
    if B is None:
        if not (isinstance(A, PreparedDictionary) and A.Mb > 0):
            raise ValueError("convert() needs B (or a prepared dictionary that holds it)")
        B = True
    return _solve(A, X, H0, B, want_h=want_h, **kw)


def _operands(A, X, H0, init, layout, dtype, device, utt_offsets, out=None, want_h=True):
    """What _solve and the fixed-dictionary solves (cd, beta, transform, deconv) share in front of their C entry.  A: the
    dictionary (deconv: its first tap) or a PreparedDictionary; device: already resolved (require_device).  Returns a namespace of
      tdtype, dcode, lay     the call's element type (torch, C ABI) and layout code
      A_d, X_d, x_np         the operands on the device (A_d None for a prepared dictionary), whether X came as numpy
      M, N, T, hshape        the sizes and the activations' shape in the caller's orientation
      init, H_d              the start rule ("given" with H0 unless the caller says otherwise, else "sklearn") and the
                             tensor the entry writes: `out` when given (H0 copied into it), else H0's device copy - cloned
                             if that is the caller's own tensor - or a fresh one; None when want_h is False and no start is
                             given
      n_utt, off_ptr         the utterance count and the int32 offsets for the C ABI (off_arr keeps them alive)"""
    torch = _torch()
    lay = _LAYOUTS[layout]
    pd = A if isinstance(A, PreparedDictionary) else None
    tdtype, dcode = _pick_dtype(dtype, X, None if pd is not None else A)
    A_d = None if pd is not None else _to_dev(A, tdtype, device)[0]
    X_d, x_np = _to_dev(X, tdtype, device)
    if lay == _lib.BIN_MAJOR:
        M, N = (pd.M, pd.N) if pd is not None else A_d.shape
        M2, T = X_d.shape
        hshape = (N, T)
    else:
        N, M = (pd.N, pd.M) if pd is not None else A_d.shape
        T, M2 = X_d.shape
        hshape = (T, N)
    if M2 != M:
        raise ValueError(f"A and X disagree on the number of bins: {M} vs {M2}")
    if init is None:
        init = "given" if H0 is not None else "sklearn"
    if init == "given":
        if H0 is None:
            raise ValueError("init='given' needs H0")
        H_d, _ = _to_dev(H0, tdtype, device)
        if tuple(H_d.shape) != hshape:
            raise ValueError(f"H0 has shape {tuple(H_d.shape)}, expected {hshape}")
        if out is not None:
            out.copy_(H_d)
            H_d = out
        elif isinstance(H0, torch.Tensor) and H_d.data_ptr() == H0.data_ptr():
            H_d = H_d.clone()       # never clobber the caller's H0
    elif not want_h:
        H_d = None
    else:
        H_d = out if out is not None else torch.empty(hshape, dtype=tdtype, device=device)
    if H_d is not None and (tuple(H_d.shape) != hshape or H_d.dtype != tdtype
                            or (H_d.shape[1] > 1 and H_d.stride(1) != 1)):
        raise ValueError("`out` must be a contiguous device tensor of the activation shape/dtype")
    n_utt, off_arr, off_ptr = _offsets(utt_offsets)
    return types.SimpleNamespace(tdtype=tdtype, dcode=dcode, lay=lay, A_d=A_d, X_d=X_d, x_np=x_np, M=M, N=N, T=T,
                                 hshape=hshape, init=init, H_d=H_d, n_utt=n_utt, off_arr=off_arr, off_ptr=off_ptr)


def _offsets(utt_offsets):
    """utt_offsets -> (n_utt, the int32 array, its pointer for the C ABI); the array keeps the pointer alive.  None is one
    utterance and a NULL pointer."""
    if utt_offsets is None:
        return 1, None, None
    off_arr = np.ascontiguousarray(np.asarray(utt_offsets, dtype=np.int32))
    n_utt = len(off_arr) - 1
    if n_utt < 1:
        raise ValueError("utt_offsets needs at least two entries")
    return n_utt, off_arr, off_arr.ctypes.data_as(C.POINTER(C.c_int))


def _n_slots(iters, check_every):
    """the error slots of a loop checked every `check_every` iterations: one at the start, one per check"""
    return 1 + (int(iters) // int(check_every) if check_every > 0 else 0)


def _finite_beta(beta):
    beta = float(beta)
    if not np.isfinite(beta):
        raise ValueError(f"beta must be finite, got {beta!r}")
    return beta


def _beta_bins_limit(shape, lay):
    """the bins of a 2-D operand addressed like the dictionary, against the beta kernels' limit - before the device is asked for"""
    if len(shape) == 2 and shape[0 if lay == _lib.BIN_MAJOR else 1] > _lib.BETA_MAX_M:     # what the ABI answers with -3
        raise ValueError(f"unsupported beta-divergence shape: M = {shape[0 if lay == _lib.BIN_MAJOR else 1]} bins, the "
                         f"kernel holds at most {_lib.BETA_MAX_M}")


def _common_opts(opts, dcode, lay, loop_events, splits=0):
    """The fields every options struct has (the entry's own are set by its wrapper): its size, the element type, the layout,
    forced `splits` in bits 8..15 of `reserved`, and loop_events = (torch.cuda.Event, torch.cuda.Event), already created:
    recorded around the entry's iteration loop."""
    opts.struct_bytes = C.sizeof(opts)
    opts.dtype, opts.layout = dcode, lay
    opts.reserved |= (int(splits) & 0xff) << 8
    if loop_events is not None:
        opts.ev_loop_start = int(loop_events[0].cuda_event)
        opts.ev_loop_stop = int(loop_events[1].cuda_event)


def _trace_arrays(n_utt, width, info):
    """(n_iter, trace, their ctypes pointers) an entry fills per utterance when info is asked for; else four None"""
    if not info:
        return None, None, None, None
    n_iter, trace = np.zeros(n_utt, dtype=np.int32), np.full((n_utt, width), np.nan)
    return n_iter, trace, n_iter.ctypes.data_as(C.POINTER(C.c_int)), trace.ctypes.data_as(C.POINTER(C.c_double))


def _call(L, entry, device, head, ws_bytes=None, tail=()):
    """The one native-call path: `entry`(*head[, workspace, its size], *tail, stream) on the device's current stream, with the
    stream's workspace leased for the duration of the call when the entry takes one (ws_bytes is not None).  A status other
    than 0 raises EvcError naming the entry."""
    torch = _torch()
    lease = _workspace(ws_bytes, device) if ws_bytes is not None else contextlib.nullcontext()
    with torch.cuda.device(device), lease as ws:
        stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        if ws is None:
            st = getattr(L, entry)(*head, *tail, stream)
        else:
            st = getattr(L, entry)(*head, ws.data_ptr(), ws.numel(), *tail, stream)
    _lib.check(st, entry)


def _solve(A, X, H0, B, *, layout="bin_major", iters=100, eps_mode="add", eps=None,
           l1=0.0, algo="auto", init=None, init_value=0.0, check_every=0,
           stop_rule="none", tol=0.0, utt_offsets: Optional[Sequence[int]] = None,
           dtype=None, device=None, info=False, out=None, loop_events=None,
           fused=True, fused_c=0, fused_w=0, want_h=True, out_y=None, loss="frobenius", exact_div=False,
           cooperative=True, all_resident=True, pair_tiles=False, lone_bin=True, range_hoist=True, quad_rows=True,
           _fake_coop_timeout=False,
           solve_info=None):
    torch = _torch()
    device = require_device(device)
    L = _lib.lib()
    lay = _LAYOUTS[layout]
    pd = A if isinstance(A, PreparedDictionary) else None
    if pd is not None:
        if dtype is None:
            dtype = pd.tdtype
        if pd.device != device:
            raise ValueError("the prepared dictionary lives on another device")
        if _pick_dtype(dtype)[1] != pd.dcode or _LOSSES[loss] != pd.loss:
            raise ValueError("the prepared dictionary was made for another dtype / loss")
    p = _operands(A, X, H0, init, layout, dtype, device, utt_offsets, out, want_h or B is None)
    tdtype, dcode, A_d, X_d, H_d, M, N, T, n_utt = p.tdtype, p.dcode, p.A_d, p.X_d, p.H_d, p.M, p.N, p.T, p.n_utt
    Mb = 0
    B_d = None
    if B is True:                 # convert() with the prepared dictionary's own B
        if pd is None or pd.Mb == 0:
            raise ValueError("convert() without B needs a prepared dictionary that holds B")
        Mb = pd.Mb
    elif B is not None:
        B_d, _ = _to_dev(B, tdtype, device)
        Mb, N2 = B_d.shape if lay == _lib.BIN_MAJOR else B_d.shape[::-1]
        if N2 != N:
            raise ValueError(f"A and B disagree on the number of exemplars: {N} vs {N2}")
    if B is not None:
        yshape = (Mb, T) if lay == _lib.BIN_MAJOR else (T, Mb)
        Y_d = out_y if out_y is not None else torch.empty(yshape, dtype=tdtype, device=device)

    opts = _lib.SolveOpts()
    opts.algo = _ALGOS[algo]
    opts.iters, opts.eps_mode, opts.init_mode = int(iters), _EPS_MODES[eps_mode], _INITS[p.init]
    opts.check_every, opts.stop_rule = int(check_every), _STOPS[stop_rule]
    opts.eps = _EPS_DEFAULT[eps_mode] if eps is None else float(eps)
    opts.l1, opts.tol, opts.init_value = float(l1), float(tol), float(init_value)
    opts.loss = _LOSSES[loss]
    # EVC_FLAG_* of include/evc.h: NO_FUSED, EXACT_DIV, NO_EXCHANGE (cooperative=False: no kernel in which
    # workgroups exchange data inside a launch - the call is then fully asynchronous), NO_ALL_RESIDENT, PAIR_TILES
    # (pair_tiles=True: the experimental k_fused_xy instead of k_fused_all), NO_LONE_BIN (lone_bin=False: M = 25 with 2, 4
    # or 8 members on k_fused_all's own 15-MFMA unit, not k_fused_lone's 14 - A/B and tests), NO_RANGE_HOIST
    # (range_hoist=False: k_fused_all / k_fused_lone test every unit's denominators instead of once per sweep - A/B and
    # tests, bitwise the same result), NO_QUAD_ROWS (quad_rows=False: k_fused_lone's shapes on that kernel, not on
    # k_fused_quad, whose bins 16 .. 24 of V' run on 4x4x4 MFMAs - A/B and tests); bits
    # 8..15 = 1 or 2 force the general streamed kernel with that many frame tiles per workgroup (tuning; on the wide
    # float32 path: exemplar ranges per frame group), bits 16..19 = wavefronts per workgroup of k_fused_wide (4 / 8)
    opts.reserved = ((0 if fused else _lib.FLAG_NO_FUSED) | (_lib.FLAG_EXACT_DIV if exact_div else 0)
                     | (0 if cooperative else _lib.FLAG_NO_EXCHANGE)
                     | (0 if all_resident else _lib.FLAG_NO_ALL_RESIDENT) | (_lib.FLAG_PAIR_TILES if pair_tiles else 0)
                     | (0 if lone_bin else _lib.FLAG_NO_LONE_BIN) | (0 if range_hoist else _lib.FLAG_NO_RANGE_HOIST)
                     | (0 if quad_rows else _lib.FLAG_NO_QUAD_ROWS)
                     | ((int(fused_c) & 0xff) << 8)
                     | ((int(fused_w) & 0xf) << 16))
    if _fake_coop_timeout is not False and _fake_coop_timeout is not None:
        # tests (evc_solve_opts.test_abort_at).  True: the call starts with the abort flag raised; an int k > 0: it is
        # raised in front of the k-th launch of the iteration loop
        opts.test_abort_at = -1 if _fake_coop_timeout is True else int(_fake_coop_timeout)
    sinfo = _lib.SolveInfo()
    sinfo.struct_bytes = C.sizeof(_lib.SolveInfo)
    opts.info = C.addressof(sinfo)
    if pd is not None:
        if loss in ("kl", "kullback-leibler") and opts.eps != pd.eps:
            raise ValueError("the prepared dictionary's KL guard differs from this call's eps")
        opts.dict = C.addressof(pd.handle)
    _common_opts(opts, dcode, lay, loop_events)

    ws_bytes = int(L.evc_workspace_bytes(M, Mb, N, T, n_utt, dcode, opts.algo))
    n_iter, err, ni_p, er_p = _trace_arrays(n_utt, _n_slots(iters, check_every), info)
    h_args = (H_d.data_ptr(), _ld(H_d)) if H_d is not None else (None, 0)
    ax_args = ((A_d.data_ptr(), _ld(A_d)) if A_d is not None else (None, 0)) + (X_d.data_ptr(), _ld(X_d))
    if B is None:
        entry, head = "evc_nmf_solve", (*ax_args, *h_args, M, N, T)
    else:
        b_args = (B_d.data_ptr(), _ld(B_d)) if B_d is not None else (None, 0)
        entry, head = "evc_nmf_convert", (*ax_args, *b_args, *h_args, Y_d.data_ptr(), _ld(Y_d), M, Mb, N, T)
    _call(L, entry, device, (*head, p.off_ptr, n_utt, C.byref(opts)), ws_bytes, (ni_p, er_p))
    to_np = p.x_np and out is None
    H_out = None if H_d is None else (_to_host(H_d) if to_np else H_d)
    res = [H_out] if B is None else ([H_out] if want_h else [])
    if B is not None:
        res.append(_to_host(Y_d) if (p.x_np and out_y is None) else Y_d)
    variant = _lib.decode_variant(int(sinfo.kernel), int(sinfo.variant))
    if info:
        res.append({"n_iter": n_iter, "err": err, "kernel": _lib.KERNEL_NAMES.get(sinfo.kernel, str(sinfo.kernel)),
                    "members": int(sinfo.members), "launches": int(sinfo.launches), "redo": int(sinfo.redo),
                    "exchange": int(sinfo.exchange), "prepared": int(sinfo.prepared), "variant": variant})
    if solve_info is not None:      # caller-supplied dict: filled without the synchronisation info=True implies
        solve_info.update(kernel=_lib.KERNEL_NAMES.get(sinfo.kernel, str(sinfo.kernel)), members=int(sinfo.members),
                          launches=int(sinfo.launches), redo=int(sinfo.redo), exchange=int(sinfo.exchange),
                          prepared=int(sinfo.prepared), variant=variant)
    return res[0] if len(res) == 1 else tuple(res)


def _solve_fixed(L, entry, device, p, dict_args, opts, ws_bytes, trace, info, mid=(), **extra):
    """The call and the return rule of the solves with the dictionary fixed (cd, beta, transform, deconv), after the wrapper
    has validated, staged the operands `p` (_operands) and filled `opts`.  dict_args: the dictionary as the entry takes it
    (pointer, leading dimension - and the tap stride where it has taps); trace = (name, width) of the per-utterance float64
    array the entry fills when info is asked for; mid: what the entry takes between X and H (evc_prox_masked_solve: the mask
    and its leading dimension); extra: the wrapper's own info fields.  Returns the activations like X came
    (numpy or device tensor), with info=True also dict(n_iter, <name>, **extra).  Without info both outputs are NULL and the
    call stays asynchronous."""
    n_iter, tr, ni_p, tr_p = _trace_arrays(p.n_utt, trace[1], info)
    _call(L, entry, device, (*dict_args, p.X_d.data_ptr(), _ld(p.X_d), *mid, p.H_d.data_ptr(), _ld(p.H_d), p.M, p.N, p.T, p.off_ptr,
                             p.n_utt, C.byref(opts)), ws_bytes, (ni_p, tr_p))
    H_out = _to_host(p.H_d) if p.x_np else p.H_d
    if info:
        return H_out, {"n_iter": n_iter, trace[0]: tr, **extra}
    return H_out


def solve_activations_cd(A, X, H0=None, *, layout="bin_major", max_iter=200, tol=1e-4, l1=0.0, l2=0.0,
                         utt_offsets: Optional[Sequence[int]] = None, dtype=None, device=None, info=False,
                         loop_events=None):
    """scikit-learn's coordinate-descent solve with the dictionary fixed (solver='cd', update_H=False,
    shuffle=False, Frobenius), on the GPU (evc_cd_solve).  H starts at 0 as in sklearn, or at H0 when given (a
    warm start).  l1 / l2 are sklearn's scaled l1_reg_W / l2_reg_W.  Per utterance: stop after the iteration whose
    violation / violation_init <= tol (or violation_init == 0), else at max_iter.

    Returns the activations in the caller's orientation (numpy in -> numpy out, device tensor in -> device tensor
    out); with info=True also dict(n_iter=int array per utterance, violation=[n_utt, max_iter] array (NaN after the
    stop), kernel="k_cd_sweep", launches=int).  No CPU fallback: without a HIP device this raises RuntimeError."""
    device = require_device(device)
    L = _lib.lib()
    p = _operands(A, X, H0, None, layout, dtype, device, utt_offsets)
    M, N, T = p.M, p.N, p.T
    opts = _lib.CdOpts()
    opts.init_mode = _lib.INIT_GIVEN if H0 is not None else _lib.INIT_SKLEARN
    opts.max_iter, opts.tol, opts.l1, opts.l2 = int(max_iter), float(tol), float(l1), float(l2)
    _common_opts(opts, p.dcode, p.lay, loop_events)
    ws_bytes = int(L.evc_cd_workspace_bytes(M, N, T, p.n_utt, p.dcode))
    if ws_bytes == 0:
        raise ValueError(f"unsupported coordinate-descent shape M={M}, N={N}, T={T}")
    return _solve_fixed(L, "evc_cd_solve", device, p, (p.A_d.data_ptr(), _ld(p.A_d)), opts, ws_bytes,
                        ("violation", max(int(max_iter), 0)), info, kernel="k_cd_sweep",
                        launches=int(max_iter) + 1 if (T > 0 and max_iter > 0) else 0)


def solve_activations_beta(A, X, H0=None, *, beta, layout="bin_major", iters=100, init=None, init_value=0.0, check_every=0,
                           stop_rule="none", tol=0.0, l1=0.0, l2=0.0, utt_offsets: Optional[Sequence[int]] = None,
                           dtype=None, device=None, info=False, loop_events=None):
    """scikit-learn's multiplicative update with the dictionary fixed under any beta-divergence (solver='mu',
    update_H=False, beta_loss=beta: 0 is Itakura-Saito, any finite float goes), on the GPU (evc_beta_solve).  beta = 1
    and beta = 2 run the same generic statement; solve_activations serves them with kernels of their own.  init:
    "given" (H0), "sklearn" (sqrt(mean(X_u) / N) per utterance) or "const" (init_value); default "given" with H0, else
    "sklearn".  l1 / l2 are sklearn's scaled l1_reg_W / l2_reg_W.  stop_rule "sklearn": per utterance, every
    `check_every` iterations, stop when (err_prev - err) / err_at_start < tol.

    Returns the activations in the caller's orientation (numpy in -> numpy out, device tensor in -> device tensor out);
    with info=True also dict(n_iter=int array per utterance, err=[n_utt, 1 + iters // check_every] array (NaN where not
    evaluated), kernel="k_beta_sweep", launches=int: the launches the iteration loop and its checks enqueue - one sweep per
    iteration, two kernels per error slot, whether or not an utterance has stopped; the import and start kernels are not
    counted).  No CPU fallback: without a HIP device this raises RuntimeError."""
    lay = _LAYOUTS[layout]
    beta = _finite_beta(beta)
    if stop_rule not in ("none", "sklearn"):
        raise ValueError("stop_rule must be 'none' or 'sklearn'")
    _beta_bins_limit(tuple(getattr(A, "shape", ())), lay)
    device = require_device(device)
    L = _lib.lib()
    p = _operands(A, X, H0, init, layout, dtype, device, utt_offsets)
    M, N, T = p.M, p.N, p.T
    if M < 1 or N < 1:
        raise ValueError(f"empty beta-divergence problem M={M}, N={N}, T={T}")
    iters, check_every = int(iters), int(check_every)
    opts = _lib.BetaOpts()
    opts.iters, opts.init_mode = iters, _INITS[p.init]
    opts.check_every, opts.stop_rule = check_every, _STOPS[stop_rule]
    opts.beta, opts.tol, opts.l1, opts.l2, opts.init_value = beta, float(tol), float(l1), float(l2), float(init_value)
    _common_opts(opts, p.dcode, lay, loop_events)
    ws_bytes = int(L.evc_beta_workspace_bytes(M, N, T, p.n_utt, p.dcode))
    n_slots = _n_slots(iters, check_every)
    return _solve_fixed(L, "evc_beta_solve", device, p, (p.A_d.data_ptr(), _ld(p.A_d)), opts, ws_bytes, ("err", n_slots), info,
                        kernel="k_beta_sweep", launches=iters + 2 * n_slots * (check_every > 0) if T > 0 else 0)


def _semi_shapes(A, X, lay, what="semi-NMF"):
    """the sizes (M, N) of a semi-NMF call from the operands' shapes alone, checked against each other and against the
    kernel's limits - before the device is asked for"""
    ashape, xshape = tuple(getattr(A, "shape", ())), tuple(getattr(X, "shape", ()))
    if len(ashape) != 2 or len(xshape) != 2:
        raise ValueError(f"A and X must be 2-D, got shapes {ashape} and {xshape}")
    M, N = ashape if lay == _lib.BIN_MAJOR else ashape[::-1]
    M2 = xshape[0 if lay == _lib.BIN_MAJOR else 1]
    if M2 != M:
        raise ValueError(f"A and X disagree on the number of bins: {M} vs {M2}")
    if M < 1 or N < 1:
        raise ValueError(f"empty {what} problem M={M}, N={N}")
    if M > _lib.SEMI_MAX_M or N > _lib.SEMI_MAX_N:           # what the ABI answers with -3
        raise ValueError(f"unsupported {what} shape: M = {M} bins, N = {N} exemplars; the kernel holds at most "
                         f"{_lib.SEMI_MAX_M} bins and {_lib.SEMI_MAX_N} exemplars")
    return M, N


def solve_activations_semi(A, X, H0=None, *, layout="bin_major", iters=100, eps=1e-9, init=None, init_value=0.0,
                           check_every=0, stop_rule="none", tol=0.0, utt_offsets: Optional[Sequence[int]] = None, dtype=None,
                           device=None, info=False, loop_events=None):
    """Semi-NMF activations with the dictionary fixed (Ding, Li and Jordan; pymf's SNMF with compute_w=False), on the GPU
    (evc_semi_solve): A and X are SIGNED - mel-cepstra, MFCCs - and only H >= 0.  Per iteration
    H <- H * sqrt((pos(A^T X) + neg(A^T A) H) / (neg(A^T X) + pos(A^T A) H + eps)).  init: "given" (H0, non-negative) or
    "const" (init_value); default "given", so H0 is needed unless init="const".  stop_rule "pymf": per utterance, from
    the third check on, stop when |err - err_prev| / T_u < tol (pymf: check_every=1, tol=2.22e-16).  At most 1056 bins and
    16384 exemplars.

    Returns the activations in the caller's orientation (numpy in -> numpy out, device tensor in -> device tensor out);
    with info=True also dict(n_iter=int array per utterance, err=[n_utt, 1 + iters // check_every] array of
    ||X_u - A H_u||_F (NaN where not evaluated), kernel="k_semi_sweep", launches=int: one sweep per iteration and three
    kernels per error slot).  No CPU fallback: without a HIP device this raises RuntimeError."""
    lay = _LAYOUTS[layout]
    if stop_rule not in ("none", "pymf"):
        raise ValueError("stop_rule must be 'none' or 'pymf'")
    if init is None:
        init = "given"
    if init not in ("given", "const"):
        raise ValueError("init must be 'given' or 'const'")
    _semi_shapes(A, X, lay)
    _pick_dtype(dtype, X, A)
    device = require_device(device)
    L = _lib.lib()
    p = _operands(A, X, H0, init, layout, dtype, device, utt_offsets)
    M, N, T = p.M, p.N, p.T
    iters, check_every = int(iters), int(check_every)
    opts = _lib.SemiOpts()
    opts.iters, opts.init_mode = iters, _INITS[p.init]
    opts.check_every, opts.stop_rule = check_every, _STOPS[stop_rule]
    opts.eps, opts.tol, opts.init_value = float(eps), float(tol), float(init_value)
    _common_opts(opts, p.dcode, lay, loop_events)
    ws_bytes = int(L.evc_semi_workspace_bytes(M, N, T, p.n_utt, p.dcode))
    n_slots = _n_slots(iters, check_every)
    return _solve_fixed(L, "evc_semi_solve", device, p, (p.A_d.data_ptr(), _ld(p.A_d)), opts, ws_bytes, ("err", n_slots), info,
                        kernel="k_semi_sweep", launches=iters + 3 * n_slots * (check_every > 0) if T > 0 else 0)


def convert_semi(A, B, X, H0=None, *, layout="bin_major", dtype=None, device=None, info=False, **kw):
    """solve_activations_semi on the signed source side (A, X) followed by synthesize with the parallel target dictionary B
    (non-negative spectra, or signed) on the same activations: returns (Y, H), with info=True (Y, H, info).  Keywords as for
    solve_activations_semi."""
    torch = _torch()
    lay = _LAYOUTS[layout]
    _, N = _semi_shapes(A, X, lay)
    bshape = tuple(getattr(B, "shape", ()))
    if len(bshape) != 2 or bshape[1 if lay == _lib.BIN_MAJOR else 0] != N:
        raise ValueError(f"A and B disagree on the number of exemplars: {N} vs shape {bshape}")
    tdtype, _ = _pick_dtype(dtype, X, A)
    device = require_device(device)
    x_np = not isinstance(X, torch.Tensor)
    X_d, _ = _to_dev(X, tdtype, device)
    out = solve_activations_semi(A, X_d, H0, layout=layout, dtype=tdtype, device=device, info=info, **kw)
    H_d, inf = out if info else (out, None)
    Y_d = synthesize(B, H_d, layout=layout, dtype=tdtype, device=device)
    Y, H = (_to_host(Y_d), _to_host(H_d)) if x_np else (Y_d, H_d)
    return (Y, H, inf) if info else (Y, H)


def _prox_slots(iters, check_every):
    """the statistic slots of evc_prox_solve: one per check, at iterations 0, check_every, 2 check_every, ... < iters"""
    return (int(iters) - 1) // int(check_every) + 1 if (check_every > 0 and iters > 0) else 0


_PROX_LIPS = {"mean": _lib.PROX_LIP_MEAN, "max": _lib.PROX_LIP_MAX}


def _prox_mask_ok(mask, X):
    """the mask of solve_activations_prox against X: same shape, finite, >= 0 - a numpy mask before any device is touched"""
    torch = _torch()
    mshape, xshape = tuple(getattr(mask, "shape", ())), tuple(getattr(X, "shape", ()))
    if mshape != xshape:
        raise ValueError(f"mask has shape {mshape}, expected X's shape {xshape}")
    if isinstance(mask, torch.Tensor):
        ok = mask.dtype.is_floating_point and bool(torch.isfinite(mask).all()) and bool((mask >= 0).all())
    else:
        m = np.asarray(mask)
        ok = m.dtype.kind in "fiub" and bool(np.isfinite(m).all()) and bool((m >= 0).all())
    if not ok:
        raise ValueError("mask must hold finite weights >= 0")


def solve_activations_prox(A, X, H0=None, *, alpha, positive=True, momentum="fista", normalize=True, iters=1000, tol=1e-3,
                           check_every=10, stop_rule="decomp", lipschitz=None, layout="bin_major",
                           utt_offsets: Optional[Sequence[int]] = None, dtype=None, device=None, info=False, loop_events=None,
                           mask=None, factored=False, lip_weights="max"):
    """Sparse activations by proximal gradient (deComP's lasso.solve / nnls.solve: ISTA, FISTA), on the GPU (evc_prox_solve):
    min_h 1/2 ||x - A h||^2 + sum_n lambda_n h_n per frame, h >= 0 (positive=True) or signed; A and X may be signed.
    Activations the threshold cuts are exactly 0.  momentum: "ista", "fista" or "nesterov" (c_i = i / (i + 3)).
    normalize=True solves in deComP's scaling (unit-norm exemplars, lambda_n = alpha M / ||a_n||, tol_n = tol ||a_n||);
    False solves the problem as given (lambda_n = alpha).  The step is 1 / L with L the Gershgorin bound of A^T A, or
    `lipschitz`.  H0 None starts at 0.  stop_rule "decomp": per utterance, at iterations 0, check_every, ... stop when
    max(|H_new - H_old| - tol_n) < 0.  At most 1056 bins and 16384 exemplars.

    mask: missing data (deComP's 2-D `mask`): finite weights >= 0 of X's shape, one per bin of every frame, a zero marks a
    missing bin; the squared error of a frame becomes sum_m mask_m (x_m - (A h)_m)^2 and, with normalize, lambda_n =
    alpha cnt_t / ||a_n|| with cnt_t the frame's sum of weights.  It runs on the factored sweep (evc_prox_masked_solve), which
    never forms A^T A: 4 M N flop per frame and iteration instead of 2 N^2.  factored=True runs that sweep without a mask -
    the same problem in another summation order, for M << N.  lip_weights: the per-bin weights wbar of the bound
    L_u = Gershgorin(A diag(wbar) A^T) of every utterance: "max" (the largest weight of the bin over the utterance, an upper
    bound of every frame's curvature) or "mean" (deComP's choice, which is none); `lipschitz` overrides both.  Per-bin (1-D)
    weights are not offered: multiply A and X by them.  With mask=None and factored=False everything is as before.

    Returns the activations in the caller's orientation (numpy in -> numpy out, device tensor in -> device tensor out);
    with info=True also dict(n_iter=int array per utterance: the updates applied, change=[n_utt, slots] array of the stop
    statistic at every check (NaN where not evaluated), kernel="k_prox_sweep" or "k_prox_resid+k_prox_back", launches=int).
    No CPU fallback: without a HIP device this raises RuntimeError."""
    lay = _LAYOUTS[layout]
    if stop_rule not in _PROX_STOPS:
        raise ValueError("stop_rule must be 'none' or 'decomp'")
    if momentum not in _PROX_MOMENTA:
        raise ValueError("momentum must be 'ista', 'fista' or 'nesterov'")
    alpha, tol, lipschitz = float(alpha), float(tol), 0.0 if lipschitz is None else float(lipschitz)
    if not (alpha >= 0.0 and np.isfinite(alpha)) or not (tol >= 0.0 and np.isfinite(tol)):
        raise ValueError("alpha and tol must be finite and >= 0")
    if not (lipschitz >= 0.0 and np.isfinite(lipschitz)):
        raise ValueError("lipschitz must be finite and > 0, or None")
    iters, check_every = int(iters), int(check_every)
    n_slots = _prox_slots(iters, check_every)
    if iters < 0 or check_every < 0 or n_slots > _lib.PROX_MAX_SLOTS:
        raise ValueError(f"iters and check_every must be >= 0 with at most {_lib.PROX_MAX_SLOTS} checks")
    if lip_weights not in _PROX_LIPS:
        raise ValueError("lip_weights must be 'mean' or 'max'")
    _semi_shapes(A, X, lay, "proximal-gradient")
    if mask is not None:
        _prox_mask_ok(mask, X)
    masked = mask is not None or bool(factored)
    _pick_dtype(dtype, X, A)
    device = require_device(device)
    L = _lib.lib()
    p = _operands(A, X, H0, "given" if H0 is not None else "const", layout, dtype, device, utt_offsets)
    opts = _lib.ProxMaskedOpts() if masked else _lib.ProxOpts()
    opts.iters, opts.init_mode = iters, _INITS[p.init]
    opts.mode = _lib.PROX_POSITIVE if positive else _lib.PROX_SIGNED
    opts.momentum, opts.normalize = _PROX_MOMENTA[momentum], 1 if normalize else 0
    opts.check_every, opts.stop_rule = check_every, _PROX_STOPS[stop_rule]
    opts.alpha, opts.tol, opts.init_value, opts.lipschitz = alpha, tol, 0.0, lipschitz
    _common_opts(opts, p.dcode, lay, loop_events)
    live = p.T > 0 and iters > 0
    if masked:
        opts.lip_weights = _PROX_LIPS[lip_weights]
        mask_d = None if mask is None else _to_dev(mask, p.tdtype, device)[0]
        mid = (None, 0) if mask_d is None else (mask_d.data_ptr(), _ld(mask_d))
        ws_bytes = int(L.evc_prox_masked_workspace_bytes(p.M, p.N, p.T, p.n_utt, p.dcode))
        return _solve_fixed(L, "evc_prox_masked_solve", device, p, (p.A_d.data_ptr(), _ld(p.A_d)), opts, ws_bytes,
                            ("change", n_slots), info, mid=mid, kernel="k_prox_resid+k_prox_back",
                            launches=2 * iters + n_slots if live else 0)
    ws_bytes = int(L.evc_prox_workspace_bytes(p.M, p.N, p.T, p.n_utt, p.dcode))
    return _solve_fixed(L, "evc_prox_solve", device, p, (p.A_d.data_ptr(), _ld(p.A_d)), opts, ws_bytes, ("change", n_slots),
                        info, kernel="k_prox_sweep", launches=iters + n_slots if live else 0)


def convert_prox(A, B, X, H0=None, *, layout="bin_major", dtype=None, device=None, info=False, **kw):
    """solve_activations_prox on the source side (A, X) followed by synthesize with the parallel target dictionary B on the
    same activations: returns (Y, H), with info=True (Y, H, info).  Keywords as for solve_activations_prox."""
    torch = _torch()
    lay = _LAYOUTS[layout]
    _, N = _semi_shapes(A, X, lay, "proximal-gradient")
    bshape = tuple(getattr(B, "shape", ()))
    if len(bshape) != 2 or bshape[1 if lay == _lib.BIN_MAJOR else 0] != N:
        raise ValueError(f"A and B disagree on the number of exemplars: {N} vs shape {bshape}")
    if kw.get("mask") is not None:
        _prox_mask_ok(kw["mask"], X)
    tdtype, _ = _pick_dtype(dtype, X, A)
    device = require_device(device)
    x_np = not isinstance(X, torch.Tensor)
    X_d, _ = _to_dev(X, tdtype, device)
    out = solve_activations_prox(A, X_d, H0, layout=layout, dtype=tdtype, device=device, info=info, **kw)
    H_d, inf = out if info else (out, None)
    Y_d = synthesize(B, H_d, layout=layout, dtype=tdtype, device=device)
    Y, H = (_to_host(Y_d), _to_host(H_d)) if x_np else (Y_d, H_d)
    return (Y, H, inf) if info else (Y, H)


def _mu_masked_shapes(A, X, lay):
    """the sizes (M, N) of a masked multiplicative-update call from the operands' shapes alone, checked against each other and
    against the kernel's limit - before the device is asked for"""
    ashape, xshape = tuple(getattr(A, "shape", ())), tuple(getattr(X, "shape", ()))
    if len(ashape) != 2 or len(xshape) != 2:
        raise ValueError(f"A and X must be 2-D, got shapes {ashape} and {xshape}")
    M, N = ashape if lay == _lib.BIN_MAJOR else ashape[::-1]
    M2 = xshape[0 if lay == _lib.BIN_MAJOR else 1]
    if M2 != M:
        raise ValueError(f"A and X disagree on the number of bins: {M} vs {M2}")
    if M < 1 or N < 1:
        raise ValueError(f"empty masked multiplicative-update problem M={M}, N={N}")
    if M > _lib.MU_MASKED_MAX_M:                              # what the ABI answers with -3
        raise ValueError(f"unsupported masked multiplicative-update shape: M = {M} bins, the kernel holds at most "
                         f"{_lib.MU_MASKED_MAX_M}")
    return M, N


def solve_activations_masked(A, X, mask=None, H0=None, *, loss="frobenius", iters=100, check_every=0, tol=0.0,
                             stop_rule=None, init=None, init_value=1.0, layout="bin_major",
                             utt_offsets: Optional[Sequence[int]] = None, dtype=None, device=None, info=False,
                             loop_events=None):
    """Multiplicative updates of the activations with missing data, the dictionary fixed (the activation half of deComP's
    nmf.solve(method='mu', likelihood='l2' | 'kl', mask=...)), on the GPU (evc_mu_masked_solve).  mask: finite weights >= 0 of
    X's shape, one per bin of every frame, a zero marks a missing bin; None is the unmasked update.  loss: "frobenius"
    (deComP's 'l2') or "kl".  Per update h <- h * max(Num, 0) / max(Den, 1e-15) with Num | Den = A^T (mask x) | A^T (mask (A h))
    (frobenius) or A^T ((mask x) / (A h + 1e-15)) | A^T mask (kl).  A frame whose mask is all zero gets h = 0.  init: "given"
    (H0) or "const" (init_value; deComP starts at ones); default "given" with H0, else "const".  stop_rule "sklearn" (the
    default when tol > 0 and check_every > 0): per utterance, every `check_every` iterations, stop when (err_prev - err) /
    err_at_start < tol, with err the masked sqrt-divergence of the loss.  At most 528 bins.

    Returns the activations in the caller's orientation (numpy in -> numpy out, device tensor in -> device tensor out);
    with info=True also dict(n_iter=int array per utterance, err=[n_utt, 1 + iters // check_every] array (NaN where not
    evaluated), kernel="k_mum_sweep", launches=int).  No CPU fallback: without a HIP device this raises RuntimeError."""
    lay = _LAYOUTS[layout]
    if loss not in _LOSSES:
        raise ValueError("loss must be 'frobenius' or 'kl'")
    iters, check_every, tol = int(iters), int(check_every), float(tol)
    if stop_rule is None:
        stop_rule = "sklearn" if (tol > 0.0 and check_every > 0) else "none"
    if stop_rule not in ("none", "sklearn"):
        raise ValueError("stop_rule must be 'none' or 'sklearn'")
    if not (tol >= 0.0 and np.isfinite(tol)):
        raise ValueError("tol must be finite and >= 0")
    n_slots = _n_slots(iters, check_every)
    if iters < 0 or check_every < 0 or n_slots > _lib.MU_MASKED_MAX_SLOTS:
        raise ValueError(f"iters and check_every must be >= 0 with at most {_lib.MU_MASKED_MAX_SLOTS} error slots")
    if init is None:
        init = "given" if H0 is not None else "const"
    if init not in ("given", "const"):
        raise ValueError("init must be 'given' or 'const'")
    _mu_masked_shapes(A, X, lay)
    if mask is not None:
        _prox_mask_ok(mask, X)
    _pick_dtype(dtype, X, A)
    device = require_device(device)
    L = _lib.lib()
    p = _operands(A, X, H0, init, layout, dtype, device, utt_offsets)
    opts = _lib.MuMaskedOpts()
    opts.loss, opts.iters, opts.init_mode = _LOSSES[loss], iters, _INITS[p.init]
    opts.check_every, opts.stop_rule = check_every, _STOPS[stop_rule]
    opts.tol, opts.init_value = tol, float(init_value)
    _common_opts(opts, p.dcode, lay, loop_events)
    mask_d = None if mask is None else _to_dev(mask, p.tdtype, device)[0]
    mid = (None, 0) if mask_d is None else (mask_d.data_ptr(), _ld(mask_d))
    ws_bytes = int(L.evc_mu_masked_workspace_bytes(p.M, p.N, p.T, p.n_utt, p.dcode))
    return _solve_fixed(L, "evc_mu_masked_solve", device, p, (p.A_d.data_ptr(), _ld(p.A_d)), opts, ws_bytes, ("err", n_slots),
                        info, mid=mid, kernel="k_mum_sweep",
                        launches=iters + 2 * n_slots * (check_every > 0) if p.T > 0 else 0)


def convert_masked(A, B, X, mask=None, H0=None, *, layout="bin_major", dtype=None, device=None, info=False, **kw):
    """solve_activations_masked on the source side (A, X, mask) followed by synthesize with the dictionary B on the same
    activations: returns (Y, H) with Y = B H, with info=True (Y, H, info).  With B = A, Y imputes the missing bins of X.
    Keywords as for solve_activations_masked."""
    torch = _torch()
    lay = _LAYOUTS[layout]
    _, N = _mu_masked_shapes(A, X, lay)
    bshape = tuple(getattr(B, "shape", ()))
    if len(bshape) != 2 or bshape[1 if lay == _lib.BIN_MAJOR else 0] != N:
        raise ValueError(f"A and B disagree on the number of exemplars: {N} vs shape {bshape}")
    if mask is not None:
        _prox_mask_ok(mask, X)
    tdtype, _ = _pick_dtype(dtype, X, A)
    device = require_device(device)
    x_np = not isinstance(X, torch.Tensor)
    X_d, _ = _to_dev(X, tdtype, device)
    out = solve_activations_masked(A, X_d, mask, H0, layout=layout, dtype=tdtype, device=device, info=info, **kw)
    H_d, inf = out if info else (out, None)
    Y_d = synthesize(B, H_d, layout=layout, dtype=tdtype, device=device)
    Y, H = (_to_host(Y_d), _to_host(H_d)) if x_np else (Y_d, H_d)
    return (Y, H, inf) if info else (Y, H)


def transform_online(W, X, *, beta=2.0, layout, max_iter=200, tol=1e-4, l1=0.0, l2=0.0, H0=None, init=None,
                     utt_offsets: Optional[Sequence[int]] = None, dtype=None, device=None, info=False, init_value=0.0,
                     out=None, loop_events=None):
    """scikit-learn's MiniBatchNMF.transform (_solve_W) with the dictionary W fixed, on the GPU (evc_online_transform): the
    activations of X under a dictionary learned online (learn_dictionary_online, compact_dictionary(batch_size=...)).
    Multiplicative updates under any beta-divergence as in solve_activations_beta, checked EVERY iteration: an utterance stops
    once ||H_new - H_old||_F / ||H_new||_F <= tol and keeps that update (tol = 0: never).  One utterance (utt_offsets) is one
    transform call: its own start sqrt(mean(X_u) / R), ratio and stop, all decided on the device.  init: "sklearn" (the
    default without H0), "given" (H0) or "const" (init_value).  l1 / l2 are sklearn's scaled l1_reg_W / l2_reg_W.  At most 528
    bins.  out: a device tensor of the activations' shape and type (rows may be padded) that receives them.

    Returns the activations in the caller's orientation (numpy in -> numpy out, device tensor in -> device tensor out); with
    info=True also dict(n_iter=int array per utterance, change=[n_utt, max_iter] the ratio of every iteration carried out
    (NaN after the stop), kernel="k_beta_sweep<change>").  info=False enqueues without waiting.  No CPU fallback: without a
    HIP device this raises RuntimeError."""
    lay = _LAYOUTS[layout]
    beta = _finite_beta(beta)
    max_iter = int(max_iter)
    if max_iter < 0:
        raise ValueError(f"max_iter must not be negative, got {max_iter!r}")
    _beta_bins_limit(tuple(getattr(W, "shape", ())), lay)
    device = require_device(device)
    L = _lib.lib()
    p = _operands(W, X, H0, init, layout, dtype, device, utt_offsets, out=out)
    M, R, T = p.M, p.N, p.T
    if M < 1 or R < 1:
        raise ValueError(f"empty beta-divergence problem M={M}, R={R}, T={T}")
    opts = _lib.TransformOpts()
    opts.max_iter, opts.init_mode = max_iter, _INITS[p.init]
    opts.beta, opts.tol, opts.l1, opts.l2, opts.init_value = beta, float(tol), float(l1), float(l2), float(init_value)
    _common_opts(opts, p.dcode, lay, loop_events)
    ws_bytes = int(L.evc_online_transform_workspace_bytes(M, R, T, p.n_utt, p.dcode))
    return _solve_fixed(L, "evc_online_transform", device, p, (p.A_d.data_ptr(), _ld(p.A_d)), opts, ws_bytes,
                        ("change", max_iter), info, kernel="k_beta_sweep<change>")


def multiframe_dictionary(frames, seg_offsets, L, *, layout="bin_major"):
    """The taps of a multi-frame exemplar dictionary from an aligned frame sequence: exemplar n is the segment of L
    consecutive frames that starts at frame n, so tap tau's column n is frame n + tau - or zero where that frame belongs to
    another source file (seg_offsets: the first frame of every file, then the frame count, as utt_offsets).  frames is
    (M, N) for bin_major, (N, M) for frame_major; returns (L, M, N) or (L, N, M) of the same kind (numpy array in, numpy
    array out, without a GPU; a tensor on any device in, a tensor there out).  L = 1 returns the frames themselves."""
    lay = _LAYOUTS[layout]
    L = int(L)
    if L < 1:
        raise ValueError(f"L must be at least 1, got {L!r}")
    offs = np.asarray(seg_offsets, dtype=np.int64)
    if frames.ndim != 2:
        raise ValueError(f"expected a 2-D matrix of frames, got shape {tuple(frames.shape)}")
    N = int(frames.shape[1 if lay == _lib.BIN_MAJOR else 0])
    if offs.ndim != 1 or len(offs) < 2 or offs[0] != 0 or offs[-1] != N or np.any(np.diff(offs) < 0):
        raise ValueError(f"seg_offsets must rise from 0 to the frame count {N}")
    n = np.arange(N)
    end = offs[np.searchsorted(offs, n, side="right")] if N else n          # the end of every frame's file
    is_np = isinstance(frames, np.ndarray)
    taps = []
    for tau in range(L):
        inside = n + tau < end
        src = np.where(inside, n + tau, 0)
        if is_np:
            where, zero = np.where, frames.dtype.type(0)
        else:
            torch = _torch()
            src, inside = torch.from_numpy(src).to(frames.device), torch.from_numpy(inside).to(frames.device)
            where, zero = torch.where, torch.zeros((), dtype=frames.dtype, device=frames.device)
        if lay == _lib.BIN_MAJOR:
            taps.append(where(inside[None, :], frames[:, src], zero))
        else:
            taps.append(where(inside[:, None], frames[src, :], zero))
    return np.stack(taps) if is_np else _torch().stack(taps)


def _taps_to_dev(D_taps, tdtype, device, what):
    """(L, rows, cols) array / tensor -> device tensor with unit inner stride (a padded view stays one); (tensor, was_numpy)"""
    torch = _torch()
    was_numpy = not isinstance(D_taps, torch.Tensor)
    D = torch.from_numpy(np.ascontiguousarray(np.asarray(D_taps))) if was_numpy else D_taps
    if D.dim() != 3:
        raise ValueError(f"{what} must be 3-D (taps, rows, columns), got shape {tuple(D.shape)}")
    D = D.to(device=device, dtype=tdtype)
    if (D.shape[2] > 1 and D.stride(2) != 1) or (D.shape[1] > 1 and D.stride(1) < D.shape[2]) or \
            (D.shape[0] > 1 and D.stride(0) < 0):
        D = D.contiguous()
    return D, was_numpy


def _taps_args(D):
    """(L, rows, cols) device taps as the deconvolution entries take them: pointer, row stride, tap stride (0 for one tap)"""
    return D.data_ptr(), _ld(D[0]), int(D.stride(0)) if D.shape[0] > 1 else 0


def _deconv_limits(shape, lay, max_bins, what):
    if len(shape) != 3:
        raise ValueError(f"{what} must be 3-D (taps, rows, columns), got shape {shape}")
    bins = shape[1 if lay == _lib.BIN_MAJOR else 2]
    if shape[0] > _lib.DECONV_MAX_TAPS or bins > max_bins:       # what the ABI answers with -3
        raise ValueError(f"unsupported deconvolution shape: {shape[0]} taps and {bins} bins, the kernels hold at most "
                         f"{_lib.DECONV_MAX_TAPS} taps and {max_bins} bins")
    if shape[0] < 1:
        raise ValueError(f"{what} needs at least one tap")


def solve_activations_deconv(A_taps, X, H0=None, *, loss="frobenius", layout="bin_major", iters=100, l1=0.0, l2=0.0, init=None,
                             init_value=0.0, check_every=0, stop_rule="none", tol=0.0,
                             utt_offsets: Optional[Sequence[int]] = None, dtype=None, device=None, info=False, out=None,
                             loop_events=None):
    """The activation solve with multi-frame exemplars (non-negative spectrogram deconvolution), on the GPU
    (evc_deconv_solve): X[:, t] ~ sum_tau A_tau H[:, t - tau] per utterance, multiplicative updates under loss "frobenius"
    or "kullback-leibler".  A_taps: (L, M, N) for bin_major, (L, N, M) for frame_major (multiframe_dictionary builds it); at
    most 16 taps and 256 bins.  With L = 1 this is scikit-learn's fixed-dictionary update.  init, l1 / l2, check_every,
    stop_rule, tol and utt_offsets as in solve_activations_beta; nothing crosses an utterance boundary.  out: a device tensor of
    the activations' shape and type (rows may be padded) that receives them.

    Returns the activations in the caller's orientation (numpy in -> numpy out, device tensor in -> device tensor out); with
    info=True also dict(n_iter=int array per utterance, err=[n_utt, 1 + iters // check_every] array (NaN where not
    evaluated), kernel="k_deconv_update", taps=L).  No CPU fallback: without a HIP device this raises RuntimeError."""
    lay = _LAYOUTS[layout]
    if loss not in _LOSSES:
        raise ValueError(f"loss must be one of {sorted(_LOSSES)}, got {loss!r}")
    if stop_rule not in ("none", "sklearn"):
        raise ValueError("stop_rule must be 'none' or 'sklearn'")
    _deconv_limits(tuple(getattr(A_taps, "shape", ())), lay, _lib.DECONV_MAX_M, "A_taps")
    device = require_device(device)
    L = _lib.lib()
    tdtype, _ = _pick_dtype(dtype, X, A_taps)
    A_d, _ = _taps_to_dev(A_taps, tdtype, device, "A_taps")
    taps = int(A_d.shape[0])
    p = _operands(A_d[0], X, H0, init, layout, tdtype, device, utt_offsets, out=out)
    M, N, T = p.M, p.N, p.T
    if M < 1 or N < 1:
        raise ValueError(f"empty deconvolution problem M={M}, N={N}, T={T}")
    iters, check_every = int(iters), int(check_every)
    opts = _lib.DeconvOpts()
    opts.loss, opts.taps, opts.iters = _LOSSES[loss], taps, iters
    opts.init_mode, opts.check_every, opts.stop_rule = _INITS[p.init], check_every, _STOPS[stop_rule]
    opts.tol, opts.l1, opts.l2, opts.init_value = float(tol), float(l1), float(l2), float(init_value)
    _common_opts(opts, p.dcode, lay, loop_events)
    ws_bytes = int(L.evc_deconv_workspace_bytes(M, N, T, p.n_utt, taps, p.dcode))
    return _solve_fixed(L, "evc_deconv_solve", device, p, _taps_args(A_d), opts, ws_bytes,
                        ("err", _n_slots(iters, check_every)), info, kernel="k_deconv_update", taps=taps)


def _synthesis_target(bshape, H_d, lay, what):
    """The sizes (Mb, N, T) and the empty Y of a synthesis, from the shape of the target dictionary's matrix (one tap's, where
    it has taps) and the activations on the device; `what` names the dictionary in the error."""
    if lay == _lib.BIN_MAJOR:
        Mb, N = bshape
        N2, T = H_d.shape
        yshape = (Mb, T)
    else:
        N, Mb = bshape
        T, N2 = H_d.shape
        yshape = (T, Mb)
    if N2 != N:
        raise ValueError(f"{what} and H disagree on the number of exemplars: {N} vs {N2}")
    return Mb, N, T, _torch().empty(yshape, dtype=H_d.dtype, device=H_d.device)


def synthesize_deconv(B_taps, H, *, layout="bin_major", utt_offsets: Optional[Sequence[int]] = None, dtype=None, device=None):
    """Y[:, t] = sum_tau B_tau H[:, t - tau] per utterance (evc_deconv_synthesize): the target rebuilt from the parallel target
    segments.  B_taps: (L, Mb, N) for bin_major, (L, N, Mb) for frame_major, at most 16 taps and 1056 bins; H and the
    returned Y as in synthesize."""
    lay = _LAYOUTS[layout]
    _deconv_limits(tuple(getattr(B_taps, "shape", ())), lay, _lib.DECONV_MAX_MB, "B_taps")
    device = require_device(device)
    L = _lib.lib()
    tdtype, dcode = _pick_dtype(dtype, H, B_taps)
    B_d, _ = _taps_to_dev(B_taps, tdtype, device, "B_taps")
    H_d, h_np = _to_dev(H, tdtype, device)
    Mb, N, T, Y = _synthesis_target(B_d.shape[1:], H_d, lay, "B_taps")
    n_utt, off_arr, off_ptr = _offsets(utt_offsets)
    _call(L, "evc_deconv_synthesize", device, (*_taps_args(B_d), H_d.data_ptr(), _ld(H_d), Y.data_ptr(), _ld(Y), Mb, N, T,
                                               off_ptr, n_utt, int(B_d.shape[0]), lay, dcode))
    return _to_host(Y) if h_np else Y


def convert_deconv(A_taps, X, B_taps, H0=None, *, layout="bin_major", utt_offsets: Optional[Sequence[int]] = None, dtype=None,
                   device=None, info=False, **kw):
    """solve_activations_deconv followed by synthesize_deconv on the same activations: returns (Y, H), with info=True
    (Y, H, info).  Keywords as for solve_activations_deconv."""
    torch = _torch()
    device = require_device(device)
    tdtype, _ = _pick_dtype(dtype, X, A_taps)
    x_np = not isinstance(X, torch.Tensor)
    X_d, _ = _to_dev(X, tdtype, device)
    out = solve_activations_deconv(A_taps, X_d, H0, layout=layout, utt_offsets=utt_offsets, dtype=tdtype, device=device,
                                   info=info, **kw)
    H_d, inf = out if info else (out, None)
    Y_d = synthesize_deconv(B_taps, H_d, layout=layout, utt_offsets=utt_offsets, dtype=tdtype, device=device)
    Y, H = (_to_host(Y_d), _to_host(H_d)) if x_np else (Y_d, H_d)
    return (Y, H, inf) if info else (Y, H)


def _taps_overlap(t):
    """whether the taps of a (L, rows, columns) tensor share memory: they are written, so they must not"""
    return t.shape[0] > 1 and t.stride(0) < (t.shape[1] - 1) * t.stride(1) + t.shape[2]


def _factor_start(a0, out, what, tdtype, device, rank=2, written=True):
    """The device tensor a learner's entry updates in place, for one factor (rank 2: a matrix; rank 3: taps): `out_<what>`
    itself when given (the start a0, if any, copied into it), else a0's device copy - never the caller's own tensor when the
    entry writes it (written), and never taps that overlap in memory."""
    torch = _torch()
    if rank == 2:
        to_dev = lambda a: _to_dev(a, tdtype, device)[0]
    else:
        to_dev = lambda a: _taps_to_dev(a, tdtype, device, "W0_taps")[0]
    if out is not None:
        if a0 is not None:
            out.copy_(to_dev(a0))
        if rank == 2 and (out.dtype != tdtype or out.dim() != 2 or (out.shape[1] > 1 and out.stride(1) != 1)):
            raise ValueError(f"`out_{what}` must be a device matrix of the call's dtype with unit inner stride")
        if rank == 3 and out.dtype != tdtype:   # its rank, inner stride and overlap: checked before the device was asked for
            raise ValueError(f"`out_{what}` must have the call's dtype")
        return out
    a_d = to_dev(a0)
    if rank == 3 and _taps_overlap(a_d):
        return a_d.contiguous()
    if written and isinstance(a0, torch.Tensor) and a_d.data_ptr() == a0.data_ptr():
        a_d = a_d.clone()       # never clobber the caller's start
    return a_d


# The dictionary learners (learn_dictionary, _beta, _cd, _online, _deconv) are four stages around their C entry, composed by
# each wrapper after its own validation: _learn_operands (operands and shapes), _common_opts (the options every struct has;
# the entry's own are set by the wrapper), _learn_run (workspace, call, counters and trace) and _learn_result (return rule).

def _learn_operands(X, W0, H0, out_w, out_h, layout, dtype, device, w_rank=2, h_written=True):
    """Stage 1: the device is resolved and the operands staged on it - X, and the two factors by _factor_start (out_w / out_h
    in place, a caller's start never clobbered; w_rank 3: the dictionary has taps; h_written False: the entry only reads the
    activations) - and their shapes checked against each other.  Returns a namespace of device, lay, tdtype, dcode, X_d, x_np
    (X came as numpy), W_d, H_d, M, R, T."""
    device = require_device(device)
    lay = _LAYOUTS[layout]
    tdtype, dcode = _pick_dtype(dtype, X, W0 if W0 is not None else out_w)
    X_d, x_np = _to_dev(X, tdtype, device)
    W_d = _factor_start(W0, out_w, "w", tdtype, device, w_rank)
    H_d = _factor_start(H0, out_h, "h", tdtype, device, written=h_written)
    bm = lay == _lib.BIN_MAJOR
    M, T = X_d.shape if bm else X_d.shape[::-1]
    M2, R = W_d.shape[-2:] if bm else W_d.shape[:-3:-1]
    R2, T2 = H_d.shape if bm else H_d.shape[::-1]
    if M2 != M or R2 != R or T2 != T:
        raise ValueError(f"X {tuple(X_d.shape)}, {'W' if w_rank == 2 else 'W_taps'} {tuple(W_d.shape)} and H "
                         f"{tuple(H_d.shape)} do not fit ({layout})")
    return types.SimpleNamespace(device=device, lay=lay, tdtype=tdtype, dcode=dcode, X_d=X_d, x_np=x_np, W_d=W_d, H_d=H_d,
                                 M=M, R=R, T=T)


def _xwh_args(p):
    """the argument list most learning entries start with: X, W, H with their leading dimensions, then M, R, T"""
    return (p.X_d.data_ptr(), _ld(p.X_d), p.W_d.data_ptr(), _ld(p.W_d), p.H_d.data_ptr(), _ld(p.H_d), p.M, p.R, p.T)


def _learn_run(L, entry, p, head, opts, nbytes, unsupported, trace_shape, want_counts, info, n_counts=1):
    """Stage 3: `entry`(*head, opts, workspace of nbytes, its n_counts int outputs, its trace, stream).  nbytes == 0 ->
    ValueError(unsupported).  The int outputs (n_iter_out, and n_steps_out where the entry has one) are asked for only with
    want_counts, the float64 trace of trace_shape only with info: with both NULL the entry enqueues without waiting.
    Returns (the counts, the trace or None)."""
    if nbytes == 0:
        raise ValueError(unsupported)
    counts = [C.c_int(0) for _ in range(n_counts)]
    tr = np.full(trace_shape, np.nan) if info else None
    tail = [C.byref(c) if want_counts else None for c in counts]
    tail.append(tr.ctypes.data_as(C.POINTER(C.c_double)) if info else None)
    _call(L, entry, p.device, (*head, C.byref(opts)), nbytes, tail)
    return [int(c.value) for c in counts], tr


def _learn_result(p, out_w, out_h, info):
    """Stage 4: (W, H) like X came - numpy for numpy operands unless out_w / out_h were given, else the device tensors - and
    the wrapper's info dict appended when there is one."""
    to_np = p.x_np and out_w is None and out_h is None
    res = (_to_host(p.W_d), _to_host(p.H_d)) if to_np else (p.W_d, p.H_d)
    return res + (info,) if info is not None else res


def _splits_info(splits, query, *sizes):
    """the `splits` field of info: what the caller forced, else the library's own choice"""
    return int(splits) if splits else int(query(*sizes))


def _route_info(L, route, M, R, T):
    """the `route` field of info: what the caller forced, else the library's own choice"""
    return route or ("fused", "unfused")[int(L.evc_beta_learn_route(M, R, T)) - 1]


_SURFACES = {"sklearn": _lib.LEARN_SKLEARN, "pymf": _lib.LEARN_PYMF}


def learn_dictionary(X, W0, H0, *, layout, iters, surface="sklearn", check_every=10, tol=0.0, dtype=None, device=None,
                     info=False, out_w=None, out_h=None, loop_events=None, splits=0, loss="frobenius"):
    """Multiplicative updates of BOTH factors, X ~ W H, on the GPU (evc_nmf_learn): W is addressed like the
    dictionary A of solve_activations, H like its activations.  surface="sklearn": scikit-learn's
    _fit_multiplicative_update with update_H=True (per iteration H, then W; the error every `check_every` iterations and
    its stop on `tol`); surface="pymf": pymf's factorize(compute_w=True) (W, then H; columns of W scaled to unit norm).
    loss: "frobenius" (default), or "kullback-leibler" / "kl" - scikit-learn's beta_loss='kullback-leibler' updates and
    error sqrt(2 KL(X || W H)), on the sklearn surface only (pymf has no such update: ValueError).

    Returns (W, H) in the caller's orientation (numpy in -> numpy out, device tensor in -> device tensor out); with
    info=True also dict(n_iter=int, err=[1 + iters // check_every] errors (the first at the start; NaN where not
    evaluated), splits=frame ranges of the dictionary update's sums).  out_w / out_h: device tensors updated in place
    (they then hold the start, W0 / H0 are ignored when None).  splits: tuning and tests, 1..64 frame ranges.
    No CPU fallback: without a HIP device this raises RuntimeError."""
    if loss not in _LOSSES:
        raise ValueError(f"loss must be one of {sorted(_LOSSES)}, got {loss!r}")
    if _LOSSES[loss] == _lib.LOSS_KL and surface == "pymf":
        raise ValueError("the pymf surface has no Kullback-Leibler update; use surface='sklearn'")
    opts = _lib.LearnOpts()
    opts.surface, opts.loss = _SURFACES[surface], _LOSSES[loss]
    opts.iters, opts.check_every, opts.tol = int(iters), int(check_every), float(tol)
    p = _learn_operands(X, W0, H0, out_w, out_h, layout, dtype, device)
    L = _lib.lib()
    _common_opts(opts, p.dcode, p.lay, loop_events, splits)
    M, R, T = p.M, p.R, p.T
    (n_iter,), err = _learn_run(L, "evc_nmf_learn", p, _xwh_args(p), opts, int(L.evc_learn_workspace_bytes(M, R, T, p.dcode)),
                                f"unsupported dictionary-learning shape M={M}, R={R}, T={T}", _n_slots(iters, check_every),
                                info or tol > 0, info)
    return _learn_result(p, out_w, out_h, {"n_iter": n_iter, "err": err,
                                           "splits": _splits_info(splits, L.evc_learn_splits, M, R, T)} if info else None)


def learn_dictionary_masked(X, W0, H0, mask=None, *, loss="frobenius", layout, iters, check_every=1, tol=0.0, dtype=None,
                            device=None, info=False, out_w=None, out_h=None, loop_events=None, splits=0):
    """deComP's batch NMF with missing data, X ~ W H with unit-norm atoms (nmf.solve(method='mu', likelihood='l2' | 'kl',
    mask=...)), on the GPU (evc_mu_masked_learn).  W is addressed like the dictionary A of solve_activations, H like its
    activations, both start at W0 / H0; mask: finite weights >= 0 of X's shape (None: the unmasked nmf.solve).  W0's atoms are
    divided by their norms first; then per iteration H by one update of solve_activations_masked's kernel, W by the same
    update, every atom divided by its norm, and the statistic max |W_before - W_after|: with tol > 0 the call stops after the
    iteration whose statistic is < tol (checked every `check_every` iterations; deComP: 1).  At most 528 bins and 4096 atoms.

    Returns (W, H) as learn_dictionary does; with info=True also dict(n_iter=int, stat=[1 + iters // check_every] statistics
    (NaN in slot 0 and where not evaluated), stopped=bool, splits=frame ranges of the dictionary half's sums).  out_w / out_h,
    loop_events, splits: as learn_dictionary's.  No CPU fallback: without a HIP device this raises RuntimeError."""
    if loss not in _LOSSES:
        raise ValueError("loss must be 'frobenius' or 'kl'")
    tol = float(tol)
    if not (tol >= 0.0 and np.isfinite(tol)):
        raise ValueError("tol must be finite and >= 0")
    xshape = tuple(getattr(X, "shape", ()))
    if len(xshape) == 2 and xshape[0 if _LAYOUTS[layout] == _lib.BIN_MAJOR else 1] > _lib.MU_MASKED_MAX_M:   # the ABI's -3
        raise ValueError(f"unsupported masked multiplicative-update shape: M = "
                         f"{xshape[0 if _LAYOUTS[layout] == _lib.BIN_MAJOR else 1]} bins, the kernel holds at most "
                         f"{_lib.MU_MASKED_MAX_M}")
    if mask is not None:
        _prox_mask_ok(mask, X)
    opts = _lib.MuMaskedLearnOpts()
    opts.loss, opts.iters, opts.check_every, opts.tol = _LOSSES[loss], int(iters), int(check_every), tol
    p = _learn_operands(X, W0, H0, out_w, out_h, layout, dtype, device)
    L = _lib.lib()
    _common_opts(opts, p.dcode, p.lay, loop_events, splits)
    M, R, T = p.M, p.R, p.T
    mask_d = None if mask is None else _to_dev(mask, p.tdtype, p.device)[0]
    head = (p.X_d.data_ptr(), _ld(p.X_d), None if mask_d is None else mask_d.data_ptr(), 0 if mask_d is None else _ld(mask_d),
            p.W_d.data_ptr(), _ld(p.W_d), p.H_d.data_ptr(), _ld(p.H_d), M, R, T)
    (n_iter,), stat = _learn_run(L, "evc_mu_masked_learn", p, head, opts,
                                 int(L.evc_mu_masked_learn_workspace_bytes(M, R, T, p.dcode)),
                                 f"unsupported masked multiplicative-update learning shape M={M}, R={R}, T={T} "
                                 f"(M <= {_lib.MU_MASKED_MAX_M}, R <= {_lib.MU_MASKED_LEARN_MAX_R})",
                                 _n_slots(iters, check_every), info or tol > 0, info)
    if not info:
        return _learn_result(p, out_w, out_h, None)
    slot = n_iter // int(check_every) if check_every > 0 and n_iter % max(int(check_every), 1) == 0 else 0
    stopped = bool(tol > 0 and slot > 0 and stat[slot] < tol)
    return _learn_result(p, out_w, out_h, {"n_iter": n_iter, "stat": stat, "stopped": stopped,
                                           "splits": _splits_info(splits, L.evc_mu_masked_learn_splits, M, R, T)})


_BETA_ROUTES = {None: 0, "fused": 1, "unfused": 2}


def learn_dictionary_beta(X, W0, H0, *, beta, layout, iters, check_every=10, tol=0.0, l1_h=0.0, l2_h=0.0, l1_w=0.0,
                          l2_w=0.0, dtype=None, device=None, info=False, out_w=None, out_h=None, loop_events=None,
                          splits=0, route=None):
    """scikit-learn's multiplicative updates of BOTH factors under any beta-divergence, X ~ W H (solver='mu',
    update_H=True, beta_loss=beta: 0 is Itakura-Saito, any finite float goes), on the GPU (evc_beta_learn).  W is
    addressed like the dictionary A of solve_activations, H like its activations, both start at W0 / H0.  Per iteration
    H by one update of solve_activations_beta's kernel, then W; the error every `check_every` iterations and the stop when
    (err_prev - err) / err_at_start < tol.  beta = 1 and beta = 2 run the same generic statement (learn_dictionary serves
    them with kernels of their own).  l1_h / l2_h are sklearn's scaled l1_reg_W / l2_reg_W (activations), l1_w / l2_w its
    l1_reg_H / l2_reg_H (dictionary).  At most 528 bins.

    Returns (W, H) as learn_dictionary does; with info=True also dict(n_iter=int, err=[1 + iters // check_every] errors,
    splits=frame ranges of the dictionary half's sums, route="fused" | "unfused": the kernels that formed those sums).
    out_w / out_h, loop_events, splits: as learn_dictionary's.  route: tests and tuning, "fused" or "unfused" instead of
    the library's choice.  No CPU fallback: without a HIP device this raises RuntimeError."""
    beta = _finite_beta(beta)
    if route not in _BETA_ROUTES:
        raise ValueError(f"route must be None, 'fused' or 'unfused', got {route!r}")
    _beta_bins_limit(tuple(getattr(X, "shape", ())), _LAYOUTS[layout])
    opts = _lib.BetaLearnOpts()
    opts.iters, opts.check_every = int(iters), int(check_every)
    opts.reserved = _BETA_ROUTES[route] << 16
    opts.beta, opts.tol = beta, float(tol)
    opts.l1_h, opts.l2_h, opts.l1_w, opts.l2_w = float(l1_h), float(l2_h), float(l1_w), float(l2_w)
    p = _learn_operands(X, W0, H0, out_w, out_h, layout, dtype, device)
    L = _lib.lib()
    _common_opts(opts, p.dcode, p.lay, loop_events, splits)
    M, R, T = p.M, p.R, p.T
    (n_iter,), err = _learn_run(L, "evc_beta_learn", p, _xwh_args(p), opts,
                                int(L.evc_beta_learn_workspace_bytes(M, R, T, p.dcode)),
                                f"unsupported beta-divergence learning shape M={M}, R={R}, T={T} "
                                f"(M <= {_lib.BETA_MAX_M}, R <= 4096)", _n_slots(iters, check_every), info or tol > 0, info)
    return _learn_result(p, out_w, out_h, {"n_iter": n_iter, "err": err,
                                           "splits": _splits_info(splits, L.evc_beta_learn_splits, M, R, T),
                                           "route": _route_info(L, route, M, R, T)} if info else None)


def learn_dictionary_online(X, W0, H0, *, beta=2.0, layout, batch_size=1024, max_iter=200, forget_factor=0.7, tol=1e-4,
                            max_no_improvement=10, l1_h=0.0, l2_h=0.0, l1_w=0.0, l2_w=0.0, state=None, dtype=None,
                            device=None, info=False, route=None, splits=None, out_w=None, out_h=None, loop_events=None,
                            fresh_restarts=False, fresh_restarts_max_iter=30, transform_max_iter=None):
    """scikit-learn's mini-batch dictionary learning, X ~ W H (MiniBatchNMF(init='custom', fresh_restarts=False,
    beta_loss=beta).fit_transform), on the GPU (evc_online_learn).  W is addressed like the dictionary A of
    solve_activations, H like its activations, both start at W0 / H0.  The frames are taken in contiguous batches of
    min(batch_size, T), in order and cycled; per step the batch's activations by one update of solve_activations_beta's
    kernel, then the dictionary from the statistics A <- rho A + Num W^(1/gamma), B <- rho B + Den, W <- (A / B)^gamma with
    rho = forget_factor ** (batch / T).  max_iter counts passes over the frames.  The loop stops when the relative change of
    W in a step is <= tol (tol = 0: off) or the smoothed batch cost has not improved for max_no_improvement steps (None or
    negative: off).  l1_h / l2_h are sklearn's scaled l1_reg_W / l2_reg_W (activations, scaled by the bins); l1_w / l2_w
    are PER FRAME (alpha_H * l1_ratio and alpha_H * (1 - l1_ratio)): each step multiplies them by its batch's frames.  At
    most 528 bins.  transform_online gives the activations of new frames under the learned W (MiniBatchNMF.transform).
    fresh_restarts=True (evc_online_learn_fresh) solves every step's activations afresh - from sqrt(mean(X_b) / R), up to
    fresh_restarts_max_iter updates, stopped by tol on their own change - and ends with such a solve over all frames
    (transform_max_iter updates; None: max_iter; 0: none): H0's values are then ignored, and H0 may be None.  Not served:
    sparse X, shuffling.

    Returns (W, H) as learn_dictionary does; with info=True also dict(n_iter=passes begun, n_steps=steps carried out,
    cost=[steps] batch costs, change=[steps] ||W_new - W_old|| / ||W_new|| (both NaN after the stop), route="fused" |
    "unfused", state=(A, B) device tensors).  state: the (A, B) of an earlier call's info: the statistics continue from
    them (the batch cycle and the stop rules restart) instead of starting at A = W0, B = 1.  info=False with tol=0 and
    max_no_improvement off enqueues max_iter passes without waiting.  route, splits: tests and tuning, as
    learn_dictionary_beta's (splits: frame ranges per batch).  No CPU fallback: without a HIP device this raises
    RuntimeError."""
    torch = _torch()
    lay = _LAYOUTS[layout]
    beta = _finite_beta(beta)
    if route not in _BETA_ROUTES:
        raise ValueError(f"route must be None, 'fused' or 'unfused', got {route!r}")
    if int(batch_size) < 1:
        raise ValueError(f"batch_size must be at least 1, got {batch_size!r}")
    if not 0.0 < float(forget_factor) <= 1.0:
        raise ValueError(f"forget_factor must lie in (0, 1], got {forget_factor!r}")
    xshape = tuple(getattr(X, "shape", ()))
    if len(xshape) != 2:
        raise ValueError(f"expected a 2-D matrix, got shape {xshape}")
    bm = lay == _lib.BIN_MAJOR
    _beta_bins_limit(xshape, lay)
    T = int(xshape[1 if bm else 0])
    bs = max(min(int(batch_size), T), 1)
    per_pass = -(-T // bs)
    splits = int(splits or 0)
    mni = -1 if max_no_improvement is None else int(max_no_improvement)
    fresh = bool(fresh_restarts)
    entry = "evc_online_learn_fresh" if fresh else "evc_online_learn"
    opts = _lib.OnlineFreshOpts() if fresh else _lib.OnlineOpts()
    if fresh:
        opts.fresh_max_iter = int(fresh_restarts_max_iter)
        opts.final_max_iter = int(max_iter if transform_max_iter is None else transform_max_iter)
        if opts.fresh_max_iter < 1 or opts.final_max_iter < 0:
            raise ValueError("fresh_restarts_max_iter must be at least 1 and transform_max_iter must not be negative")
        if H0 is None and out_h is None:        # the start is ignored: any matrix of the activations' shape
            R = int(tuple(W0.shape)[1 if bm else 0])
            hshape = (R, T) if bm else (T, R)
            H0 = torch.empty(hshape, dtype=W0.dtype, device=W0.device) if isinstance(W0, torch.Tensor) \
                else np.empty(hshape, dtype=np.asarray(W0).dtype)
    opts.batch_size, opts.max_iter, opts.max_no_improvement = int(batch_size), int(max_iter), mni
    opts.resume = 0 if state is None else 1
    opts.reserved = _BETA_ROUTES[route] << 16
    opts.beta, opts.tol, opts.forget_factor = beta, float(tol), float(forget_factor)
    opts.l1_h, opts.l2_h, opts.l1_w, opts.l2_w = float(l1_h), float(l2_h), float(l1_w), float(l2_w)
    p = _learn_operands(X, W0, H0, out_w, out_h, layout, dtype, device)
    L = _lib.lib()
    _common_opts(opts, p.dcode, p.lay, loop_events, splits)
    M, R, T, W_d = p.M, p.R, p.T, p.W_d
    ws_query = L.evc_online_fresh_workspace_bytes if fresh else L.evc_online_workspace_bytes
    nbytes = int(ws_query(M, R, T, int(batch_size), p.dcode))
    unsupported = f"unsupported mini-batch learning shape M={M}, R={R}, T={T} (M <= {_lib.BETA_MAX_M}, R <= 4096)"
    if nbytes == 0:         # refused here already, before `state` is looked at
        raise ValueError(unsupported)
    if state is None:
        A_d, B_d = torch.empty_like(W_d).contiguous(), torch.empty_like(W_d).contiguous()
    else:
        A_d, B_d = state
        for t in (A_d, B_d):
            if not isinstance(t, torch.Tensor) or t.shape != W_d.shape or t.dtype != W_d.dtype \
                    or t.device != W_d.device or not t.is_contiguous():
                raise ValueError("`state` must be the (A, B) device tensors of an earlier call's info, shaped like W")
    xwh = _xwh_args(p)
    (n_iter, n_steps), tr = _learn_run(L, entry, p, (*xwh[:6], A_d.data_ptr(), B_d.data_ptr(), _ld(A_d), *xwh[6:]), opts,
                                       nbytes, unsupported, (max(int(max_iter), 0) * per_pass, 2), info or tol > 0 or mni >= 0,
                                       info, n_counts=2)
    return _learn_result(p, out_w, out_h, {"n_iter": n_iter, "n_steps": n_steps, "state": (A_d, B_d),
                                           "route": _route_info(L, route, M, R, T),
                                           "cost": np.ascontiguousarray(tr[:, 0]),
                                           "change": np.ascontiguousarray(tr[:, 1])} if info else None)


def decomp_frame_order(T, epochs, seed):
    """The frame orders of `epochs` passes as deComP's dictionary_learning.solve shuffles them with random_seed=seed: an
    index array shuffled in place and cumulatively by RandomState(seed) every epoch, applied to the already shuffled frames.
    Returns an int32 array (epochs, T): row e lists the frames in the order epoch e takes them."""
    rng = np.random.RandomState(seed)
    index, pos = np.arange(int(T)), np.arange(int(T))
    rows = np.empty((max(int(epochs), 0), int(T)), dtype=np.int32)
    for e in range(rows.shape[0]):
        rng.shuffle(index)
        pos = pos[index]
        rows[e] = pos
    return rows


_STOCH_METHODS = {"asg": _lib.STOCH_ASG, "asag": _lib.STOCH_ASAG, "gsag": _lib.STOCH_GSAG, "svrmu": _lib.STOCH_SVRMU}


def learn_dictionary_stochastic(X, W0, H0, mask=None, *, method, loss="frobenius", layout, batch_size, epochs, tol=0.0,
                                forget_rate=0.5, alpha=1.0, inner_iters=1, order=None, seed=None, route=None, dtype=None,
                                device=None, info=False, out_w=None, out_h=None, loop_events=None):
    """deComP's mini-batch NMF, X ~ W H with unit-norm atoms (nmf.solve(minibatch=batch_size, method='asg-mu' | 'asag-mu' |
    'gsag-mu' | 'svrmu' | 'svrmu-acc', likelihood='l2' | 'kl', mask=...)), on the GPU (evc_mu_stoch_learn).  W and H are
    addressed and start as learn_dictionary_masked's; mask: finite weights >= 0 of X's shape (None: no mask).  method: "asg"
    (W from every batch's own gradients; deComP's 'gsg-mu' runs the same code), "asag" (gradients averaged with
    forget_rate, W every step), "gsag" (the same average, W once per epoch), "svrmu" (Kasai's variance-reduced update with
    step alpha; inner_iters > 1 activation updates per step is deComP's 'svrmu-acc').  An epoch takes floor(T / batch_size)
    batches of batch_size frames in the order of its row of `order` ((epochs, T) or (1, T) ints, every row a permutation;
    None: as the frames lie); seed (when order is None) builds the rows as deComP does with random_seed=seed: one row per
    epoch (decomp_frame_order), for "svrmu" one row for all epochs.  The call stops at the first update with
    max |W - W_new| < tol and then keeps the old W, as deComP does (tol = 0: never).  At most 528 bins and 4096 atoms.

    Returns (W, H) as learn_dictionary does; with info=True also dict(n_epochs=the epoch (from 1) of the stopping update, else
    epochs, n_steps=steps carried out, stat=[epochs * (T // batch_size); gsag: epochs] max |W - W_new| of every update (NaN
    after the stop), stopped=bool, route="fused" | "unfused", splits=frame ranges of a batch's gradient sums).  route: tests
    and tuning, "fused" (R <= 256) or "unfused" instead of the library's choice.  info=False with tol=0 enqueues without
    waiting.  No CPU fallback: without a HIP device this raises RuntimeError."""
    if method not in _STOCH_METHODS:
        raise ValueError(f"method must be one of {sorted(_STOCH_METHODS)}, got {method!r}")
    if loss not in _LOSSES:
        raise ValueError("loss must be 'frobenius' or 'kl'")
    if route not in _BETA_ROUTES:
        raise ValueError(f"route must be None, 'fused' or 'unfused', got {route!r}")
    tol, forget_rate, alpha = float(tol), float(forget_rate), float(alpha)
    if not (tol >= 0.0 and np.isfinite(tol)):
        raise ValueError("tol must be finite and >= 0")
    if not 0.0 < forget_rate <= 1.0:
        raise ValueError(f"forget_rate must lie in (0, 1], got {forget_rate!r}")
    if not np.isfinite(alpha):
        raise ValueError("alpha must be finite")
    batch_size, epochs, inner_iters = int(batch_size), int(epochs), int(inner_iters)
    lay = _LAYOUTS[layout]
    xshape = tuple(getattr(X, "shape", ()))
    if len(xshape) != 2:
        raise ValueError(f"expected a 2-D matrix, got shape {xshape}")
    bm = lay == _lib.BIN_MAJOR
    T, M0 = int(xshape[1 if bm else 0]), int(xshape[0 if bm else 1])
    if M0 > _lib.MU_MASKED_MAX_M:                                          # the ABI's -3
        raise ValueError(f"unsupported mini-batch multiplicative-update shape: M = {M0} bins, the kernel holds at most "
                         f"{_lib.MU_MASKED_MAX_M}")
    if not 1 <= batch_size <= T:
        raise ValueError(f"batch_size must be between 1 and the number of frames ({T}), got {batch_size}")
    if epochs < 0:
        raise ValueError("epochs must be >= 0")
    if inner_iters < 1 or (inner_iters != 1 and method != "svrmu"):
        raise ValueError("inner_iters must be >= 1, and 1 unless method='svrmu'")
    if order is None and seed is not None:
        order = decomp_frame_order(T, 1 if method == "svrmu" else epochs, seed)
    if order is not None:
        order = np.ascontiguousarray(order, dtype=np.int32)
        rows = order.shape[0] if order.ndim == 2 else -1
        if order.ndim != 2 or order.shape[1] != T or rows not in (1, epochs) or \
                not np.array_equal(np.sort(order, axis=1), np.broadcast_to(np.arange(T), (rows, T))):
            raise ValueError(f"order must hold 1 or {epochs} rows, each a permutation of the {T} frames")
        if rows == 0:
            order = None
    if mask is not None:
        _prox_mask_ok(mask, X)
    opts = _lib.MuStochOpts()
    opts.loss, opts.method, opts.batch_size, opts.epochs = _LOSSES[loss], _STOCH_METHODS[method], batch_size, epochs
    opts.inner_iters, opts.order_rows, opts.route = inner_iters, 0 if order is None else int(order.shape[0]), _BETA_ROUTES[route]
    opts.forget_rate, opts.alpha, opts.tol = forget_rate, alpha, tol
    p = _learn_operands(X, W0, H0, out_w, out_h, layout, dtype, device)
    L = _lib.lib()
    _common_opts(opts, p.dcode, p.lay, loop_events)
    M, R = p.M, p.R
    if route == "fused" and R > _lib.MU_STOCH_FUSED_MAX_R:
        raise ValueError(f"the fused route holds at most {_lib.MU_STOCH_FUSED_MAX_R} atoms, got R={R}")
    mask_d = None if mask is None else _to_dev(mask, p.tdtype, p.device)[0]
    order_p = None if order is None else order.ctypes.data_as(C.POINTER(C.c_int))
    head = (p.X_d.data_ptr(), _ld(p.X_d), None if mask_d is None else mask_d.data_ptr(), 0 if mask_d is None else _ld(mask_d),
            p.W_d.data_ptr(), _ld(p.W_d), p.H_d.data_ptr(), _ld(p.H_d), order_p, M, R, T)
    n_loop = T // batch_size
    n_upd = epochs if method == "gsag" else epochs * n_loop
    (n_epochs, n_steps), stat = _learn_run(L, "evc_mu_stoch_learn", p, head, opts,
                                           int(L.evc_mu_stoch_learn_workspace_bytes(M, R, T, batch_size, opts.method, p.dcode)),
                                           f"unsupported mini-batch multiplicative-update shape M={M}, R={R}, T={T} "
                                           f"(M <= {_lib.MU_MASKED_MAX_M}, R <= {_lib.MU_STOCH_MAX_R})",
                                           (n_upd,), info or tol > 0, info, n_counts=2)
    if not info:
        return _learn_result(p, out_w, out_h, None)
    done = -(-n_steps // n_loop) if method == "gsag" else n_steps
    stopped = bool(tol > 0 and done > 0 and n_steps % (n_loop if method == "gsag" else 1) == 0 and stat[done - 1] < tol)
    rcode = _BETA_ROUTES[route]
    return _learn_result(p, out_w, out_h, {"n_epochs": n_epochs, "n_steps": n_steps, "stat": stat, "stopped": stopped,
                                           "route": ("fused", "unfused")[int(L.evc_mu_stoch_learn_route(R, rcode)) - 1],
                                           "splits": int(L.evc_mu_stoch_learn_splits(M, R, batch_size, rcode))})


def learn_dictionary_sparse(X, D0, H0=None, *, alpha, layout, batch_size, epochs, tol=0.0, lasso_iters=10, lasso_tol=1e-5,
                            positive=True, momentum="fista", order=None, seed=None, state=None, dtype=None, device=None,
                            info=False, out_w=None, out_h=None, loop_events=None, lasso_check_every=10, skip=(), mask=None):
    """Sparse dictionary learning, X ~ D H with sparse H and atoms of norm <= 1, on the GPU (evc_prox_learn): Mairal et al.'s
    online method as deComP's dictionary_learning.solve(method='block_cd') runs it.  D is addressed like the dictionary A of
    solve_activations_prox, H like its activations; D0 is divided by its atoms' norms first, H0 None starts at ones (deComP's
    default).  An epoch takes floor(T / batch_size) batches of batch_size frames in the order of its row of `order`
    ((epochs, T) ints, every row a permutation; None: as the frames lie), the last T mod batch_size frames of the row are
    left alone; seed (when order is None) builds the rows as deComP does with random_seed=seed (decomp_frame_order).  Per
    step: the batch's activations by solve_activations_prox's statement (normalize, alpha, lasso_iters updates, lasso_tol,
    positive, momentum), the statistics S <- beta S + H_F H_F^T, Q <- beta Q + H_F X_F^T, one block-coordinate sweep over the
    atoms with the projection |d_j| <= 1; the call stops when max |D_new - D| < tol (tol = 0: never).  At most 1056 bins and
    4096 atoms.

    Returns (D, H) as learn_dictionary does; with info=True also dict(n_epochs=epochs begun, n_steps=steps carried out,
    change=[epochs * (T // batch_size)] max |D_new - D| of every step (NaN after the stop), block=atoms per block of the
    sweep, state=(stats, count): the N x (N + M) device tensor [S | Q] and the step count).  state: that of an earlier
    call's info: the statistics and the count continue (D is then not normalised again); the caller passes the remaining rows
    of `order`.  info=False with tol=0 enqueues without waiting.  skip: measurement only (tools/bench_prox_learn.py), the halves
    of the step to leave out, of "lasso", "statistics", "sweep".

    mask: missing data (deComP's dictionary_learning.solve(..., mask=)): finite weights >= 0 of X's shape, one per bin of
    every frame, a zero marks a missing bin.  The call then runs evc_prox_masked_learn, another algorithm: the lasso is
    solve_activations_prox(mask=, lip_weights="mean")'s, the Gram statistic is one N x N matrix per bin, Q takes mask . X,
    and all atoms are updated at once from the old dictionary (a Jacobi step) with one denominator per atom, the sum over the
    bins of S_m[k, k] + 1e-15 - a mask of ones does NOT give the unmasked call's result.  info["state"] is then (stats_s,
    stats_q, count): the (M, N, N) and (N, M) device tensors and the step count, and resumes likewise; info["block"] is 0;
    "sweep" in skip stands for the atom update.  At most 1056 bins, 1024 atoms and M N^2 <= 2^28.

    No CPU fallback: without a HIP device this raises RuntimeError."""
    torch = _torch()
    lay = _LAYOUTS[layout]
    if momentum not in _PROX_MOMENTA:
        raise ValueError("momentum must be 'ista', 'fista' or 'nesterov'")
    alpha, tol, lasso_tol = float(alpha), float(tol), float(lasso_tol)
    if not all(v >= 0.0 and np.isfinite(v) for v in (alpha, tol, lasso_tol)):
        raise ValueError("alpha, tol and lasso_tol must be finite and >= 0")
    batch_size, epochs, lasso_iters, lasso_check_every = int(batch_size), int(epochs), int(lasso_iters), int(lasso_check_every)
    xshape = tuple(getattr(X, "shape", ()))
    if len(xshape) != 2:
        raise ValueError(f"expected a 2-D matrix, got shape {xshape}")
    bm = lay == _lib.BIN_MAJOR
    T = int(xshape[1 if bm else 0])
    if not 1 <= batch_size <= T:
        raise ValueError(f"batch_size must be between 1 and the number of frames ({T}), got {batch_size}")
    if epochs < 0 or lasso_iters < 0 or lasso_check_every < 0:
        raise ValueError("epochs, lasso_iters and lasso_check_every must be >= 0")
    if order is None and seed is not None:
        order = decomp_frame_order(T, epochs, seed)
    if order is not None:
        order = np.ascontiguousarray(order, dtype=np.int32)
        if order.shape != (epochs, T) or (epochs and not np.array_equal(np.sort(order, axis=1),
                                                                          np.broadcast_to(np.arange(T), (epochs, T)))):
            raise ValueError(f"order must hold {epochs} rows, each a permutation of the {T} frames")
    if mask is not None:
        _prox_mask_ok(mask, X)
    if H0 is None and out_h is None:
        N0 = int(tuple((D0 if D0 is not None else out_w).shape)[1 if bm else 0])
        hshape = (N0, T) if bm else (T, N0)
        ref = D0 if D0 is not None else out_w
        H0 = torch.ones(hshape, dtype=ref.dtype, device=ref.device) if isinstance(ref, torch.Tensor) \
            else np.ones(hshape, dtype=np.asarray(ref).dtype)
    opts = _lib.ProxLearnOpts() if mask is None else _lib.ProxMaskedLearnOpts()
    opts.batch_size, opts.epochs, opts.lasso_iters, opts.lasso_check_every = batch_size, epochs, lasso_iters, lasso_check_every
    opts.mode = _lib.PROX_POSITIVE if positive else _lib.PROX_SIGNED
    opts.momentum, opts.resume = _PROX_MOMENTA[momentum], 0 if state is None else 1
    opts.alpha, opts.tol, opts.lasso_tol = alpha, tol, lasso_tol
    opts.reserved = sum({"lasso": 1, "statistics": 2, "sweep": 4}[h] for h in set(skip))
    p = _learn_operands(X, D0, H0, out_w, out_h, layout, dtype, device)
    L = _lib.lib()
    _common_opts(opts, p.dcode, p.lay, loop_events)
    M, N = p.M, p.R
    if mask is not None:
        return _learn_sparse_masked(L, p, opts, mask, order, state, T, batch_size, epochs, tol, info, out_w, out_h)
    nbytes = int(L.evc_prox_learn_workspace_bytes(M, N, T, batch_size, p.dcode))
    unsupported = (f"unsupported sparse dictionary-learning shape M={M}, N={N}, T={T} (M <= {_lib.PROX_LEARN_MAX_M}, "
                   f"N <= {_lib.PROX_LEARN_MAX_N})")
    if nbytes == 0:         # refused here already, before `state` is looked at
        raise ValueError(unsupported)
    if state is None:
        stats, count = torch.empty((N, N + M), dtype=p.tdtype, device=p.device), C.c_longlong(0)
    else:
        stats, count = state[0], C.c_longlong(int(state[1]))
        if not isinstance(stats, torch.Tensor) or tuple(stats.shape) != (N, N + M) or stats.dtype != p.tdtype \
                or stats.device != p.W_d.device or not stats.is_contiguous() or count.value < 0:
            raise ValueError("`state` must be the (stats, count) of an earlier call's info: an N x (N + M) device tensor and "
                             "a step count")
    xwh = _xwh_args(p)
    order_p = None if order is None else order.ctypes.data_as(C.POINTER(C.c_int))
    (n_epochs, n_steps), tr = _learn_run(L, "evc_prox_learn", p,
                                         (*xwh[:6], stats.data_ptr(), _ld(stats), C.byref(count), order_p, *xwh[6:]), opts,
                                         nbytes, unsupported, (epochs * (T // batch_size),), info or tol > 0, info, n_counts=2)
    return _learn_result(p, out_w, out_h, {"n_epochs": n_epochs, "n_steps": n_steps, "change": tr,
                                           "block": int(L.evc_prox_learn_block(M, p.dcode)),
                                           "state": (stats, int(count.value))} if info else None)


def _learn_sparse_masked(L, p, opts, mask, order, state, T, batch_size, epochs, tol, info, out_w, out_h):
    """learn_dictionary_sparse's tail with a mask: the statistics' tensors, evc_prox_masked_learn and the result"""
    torch = _torch()
    M, N = p.M, p.R
    mask_d = _to_dev(mask, p.tdtype, p.device)[0]
    nbytes = int(L.evc_prox_masked_learn_workspace_bytes(M, N, T, batch_size, p.dcode))
    unsupported = (f"unsupported masked sparse dictionary-learning shape M={M}, N={N}, T={T} (M <= "
                   f"{_lib.PROX_MASKED_LEARN_MAX_M}, N <= {_lib.PROX_MASKED_LEARN_MAX_N}, M N^2 <= "
                   f"{_lib.PROX_MASKED_LEARN_MAX_S})")
    if nbytes == 0:         # refused here already, before `state` is looked at
        raise ValueError(unsupported)
    if state is None:
        stats_s = torch.empty((M, N, N), dtype=p.tdtype, device=p.device)
        stats_q, count = torch.empty((N, M), dtype=p.tdtype, device=p.device), C.c_longlong(0)
    else:
        ok = len(state) == 3
        if ok:
            stats_s, stats_q, count = state[0], state[1], C.c_longlong(int(state[2]))
            ok = count.value >= 0 and all(isinstance(t, torch.Tensor) and tuple(t.shape) == shape and t.dtype == p.tdtype
                                          and t.device == p.W_d.device and t.is_contiguous()
                                          for t, shape in ((stats_s, (M, N, N)), (stats_q, (N, M))))
        if not ok:
            raise ValueError("`state` must be the (stats_s, stats_q, count) of an earlier masked call's info: (M, N, N) and "
                             "(N, M) device tensors and a step count")
    xwh = _xwh_args(p)
    order_p = None if order is None else order.ctypes.data_as(C.POINTER(C.c_int))
    head = (*xwh[:2], mask_d.data_ptr(), _ld(mask_d), *xwh[2:6], stats_s.data_ptr(), N, stats_q.data_ptr(), M, C.byref(count),
            order_p, *xwh[6:])
    (n_epochs, n_steps), tr = _learn_run(L, "evc_prox_masked_learn", p, head, opts, nbytes, unsupported,
                                         (epochs * (T // batch_size),), info or tol > 0, info, n_counts=2)
    return _learn_result(p, out_w, out_h, {"n_epochs": n_epochs, "n_steps": n_steps, "change": tr, "block": 0,
                                           "state": (stats_s, stats_q, int(count.value))} if info else None)


def compact_dictionary_sparse(A, B, R, *, alpha, batch_size, epochs=10, tol=0.0, layout="bin_major", prepared=False, dtype=None,
                              device=None, seed=None, mask_a=None, mask_b=None, **kw):
    """A compact parallel dictionary for the sparse solve: the aligned source and target exemplars are stacked, D = [A; B]
    ((Ma + Mb) x N) as compact_dictionary stacks them, and R << N joint atoms [Wa; Wb] are learnt by
    learn_dictionary_sparse with the exemplars as the frames, from R evenly spaced exemplars and activations of ones.  The
    stacked atoms have norm <= 1.  Returns (Wa, Wb, G, info) in the caller's orientation, info as
    learn_dictionary_sparse's; prepared=True: (PreparedDictionary of (Wa, Wb), G, info).  The pair is ready for
    convert_prox(Wa, Wb, X, ...).  mask_a, mask_b: weights >= 0 of A's and B's shape (a zero: the bin of that exemplar is
    missing), stacked as the exemplars are, a side not given counting as ones; with either the atoms are learnt by
    learn_dictionary_sparse(mask=...).  Further keywords (lasso_iters, lasso_tol, positive, momentum, order) go to
    learn_dictionary_sparse."""
    torch = _torch()
    if mask_a is not None:
        _prox_mask_ok(mask_a, A)
    if mask_b is not None:
        _prox_mask_ok(mask_b, B)
    device = require_device(device)
    lay = _LAYOUTS[layout]
    tdtype, _ = _pick_dtype(dtype, A, B)
    A_d, a_np = _to_dev(A, tdtype, device)
    B_d, _ = _to_dev(B, tdtype, device)
    bm = lay == _lib.BIN_MAJOR
    D = torch.cat([A_d, B_d], dim=0 if bm else 1)              # bin-major: (Ma + Mb, N); frame-major: (N, Ma + Mb)
    Ma = A_d.shape[0] if bm else A_d.shape[1]
    N = D.shape[1] if bm else D.shape[0]
    R = int(R)
    if not 1 <= R <= N:
        raise ValueError(f"R must be between 1 and the number of exemplars ({N}), got {R}")
    pick = torch.div(torch.arange(R, device=device) * N, R, rounding_mode="floor")
    W0 = (D[:, pick] if bm else D[pick, :]).contiguous()
    G0 = torch.ones((R, N) if bm else (N, R), dtype=tdtype, device=device)
    mask = None
    if mask_a is not None or mask_b is not None:
        sides = [torch.ones_like(side) if m is None else _to_dev(m, tdtype, device)[0] for m, side in ((mask_a, A_d), (mask_b, B_d))]
        mask = torch.cat(sides, dim=0 if bm else 1)
    W, G, info = learn_dictionary_sparse(D, None, None, alpha=alpha, layout=layout, batch_size=batch_size, epochs=epochs,
                                         tol=tol, seed=seed, dtype=tdtype, device=device, info=True, out_w=W0, out_h=G0,
                                         mask=mask, **kw)
    Wa, Wb = (W[:Ma], W[Ma:]) if bm else (W[:, :Ma], W[:, Ma:])
    if prepared:
        return prepare_dictionary(Wa, Wb, layout=layout, dtype=tdtype, device=device), (_to_host(G) if a_np else G), info
    if a_np:
        return _to_host(Wa), _to_host(Wb), _to_host(G), info
    return Wa, Wb, G, info


_CDL_UPDATES = {"both": _lib.CDL_BOTH, "dict": _lib.CDL_DICT_ONLY}


def _cd_learn_workspace(L, M, R, T, dcode, splits):
    """bytes evc_cd_learn needs; `splits` forced frame ranges beyond evc_cd_learn_splits() add their slabs (include/evc.h)"""
    nbytes = int(L.evc_cd_learn_workspace_bytes(M, R, T, dcode))
    extra = int(splits) - int(L.evc_cd_learn_splits(M, R, T)) if nbytes else 0
    if extra > 0:
        tiles = lambda n: (-(-n // 16) + 3) // 4 * 4
        nbytes += extra * 2 * 16 * (tiles(M) + tiles(R)) * (-(-R // 128) * 128) * (8 if dcode == _lib.F64 else 4)
    return nbytes


def learn_dictionary_cd(X, W0, H0, *, layout, max_iter=200, tol=1e-4, l1_h=0.0, l2_h=0.0, l1_w=0.0, l2_w=0.0, update="both",
                        dtype=None, device=None, info=False, out_w=None, out_h=None, loop_events=None, splits=0):
    """scikit-learn's coordinate descent on BOTH factors, X ~ W H (solver='cd', update_H=True, shuffle=False, Frobenius), on
    the GPU (evc_cd_learn): W is addressed like the dictionary A of solve_activations, H like its activations, both start
    at W0 / H0.  Per iteration one activation sweep (that of solve_activations_cd), then one sweep over the dictionary's
    rows; the loop stops after the iteration whose violation / violation_init <= tol (or violation_init == 0), else at
    max_iter.  l1_h / l2_h are sklearn's scaled l1_reg_W / l2_reg_W (activations), l1_w / l2_w its l1_reg_H / l2_reg_H
    (dictionary).  update="dict": the activations stay at H0 and only the dictionary half runs and counts.

    Returns (W, H) in the caller's orientation (numpy in -> numpy out, device tensor in -> device tensor out); with
    info=True also dict(n_iter=int, violation=[max_iter, 2] array: the activation and the dictionary half of every
    iteration, NaN after the stop, splits=frame ranges of the sums over the frames).  out_w / out_h: device tensors updated
    in place (they then hold the start, W0 / H0 are ignored when None).  splits: tuning and tests, 1..64 frame ranges.
    info=False with tol=0 enqueues max_iter iterations without waiting.  No CPU fallback: without a HIP device this raises
    RuntimeError."""
    if update not in _CDL_UPDATES:
        raise ValueError(f"update must be one of {sorted(_CDL_UPDATES)}, got {update!r}")
    opts = _lib.CdLearnOpts()
    opts.max_iter, opts.update = int(max_iter), _CDL_UPDATES[update]
    opts.tol, opts.l1_h, opts.l2_h, opts.l1_w, opts.l2_w = float(tol), float(l1_h), float(l2_h), float(l1_w), float(l2_w)
    p = _learn_operands(X, W0, H0, out_w, out_h, layout, dtype, device)
    L = _lib.lib()
    _common_opts(opts, p.dcode, p.lay, loop_events, splits)
    M, R, T = p.M, p.R, p.T
    (n_iter,), viol = _learn_run(L, "evc_cd_learn", p, _xwh_args(p), opts, _cd_learn_workspace(L, M, R, T, p.dcode, splits),
                                 f"unsupported coordinate-descent learning shape M={M}, R={R}, T={T} (M, R <= 1024)",
                                 (max(int(max_iter), 0), 2), info or tol > 0, info)
    return _learn_result(p, out_w, out_h, {"n_iter": n_iter, "violation": viol,
                                           "splits": _splits_info(splits, L.evc_cd_learn_splits, M, R, T)} if info else None)


def compact_dictionary(A, B, R, *, iters=100, tol=0.0, layout="bin_major", prepared=False, dtype=None, device=None,
                       loss="frobenius", solver="mu", batch_size=None, forget_factor=0.7, beta=None):
    """A compact parallel dictionary: the aligned source and target exemplars are stacked, D = [A; B] ((Ma + Mb) x N),
    and factored jointly, D ~ [Wa; Wb] G, with R << N components by learn_dictionary (scikit-learn surface, the error
    every 10 iterations); (Wa, Wb) then stand in for (A, B) in solve_activations / convert at R / N of the cost.

    The start is deterministic: W0 = R evenly spaced exemplars (columns of D) floored at 1e-6, G0 = sqrt(mean(D) / R)
    everywhere, whatever the loss.  Returns (Wa, Wb, G, info) in the caller's orientation; info as learn_dictionary's.
    prepared=True: (PreparedDictionary of (Wa, Wb), G, info) instead, ready for convert().  loss: as learn_dictionary's
    (the prepared dictionary itself is the plain one: pass the loss to convert / prepare_dictionary to solve under it).
    solver="cd": the same stacked compaction by learn_dictionary_cd (scikit-learn's default solver; Frobenius only, at most
    1024 stacked bins and components; `iters` is its max_iter and `tol` its violation ratio; info as learn_dictionary_cd's).
    beta: when given, the compaction minimises that beta-divergence by learn_dictionary_beta from the same start (0 is
    Itakura-Saito, the usual loss for power spectra; at most 528 stacked bins; info as learn_dictionary_beta's); `loss`
    must then be left at its default and solver at "mu".
    batch_size: when given, the compaction is learnt online by learn_dictionary_online in batches of that many exemplars
    (scikit-learn's MiniBatchNMF; forget_factor is its forgetting of old batches) under `beta` (default 2) from the same
    start; `iters` is then the number of passes and `tol` the stop on the relative change of the dictionary, the
    no-improvement stop is off; `loss` and `solver` must be left at their defaults; info as learn_dictionary_online's."""
    if batch_size is not None and (loss != "frobenius" or solver != "mu"):
        raise ValueError("batch_size selects the online learner: leave `loss` and `solver` at their defaults")
    if beta is not None and (loss != "frobenius" or solver != "mu"):
        raise ValueError("beta names the loss itself: leave `loss` and `solver` at their defaults")
    if loss not in _LOSSES:
        raise ValueError(f"loss must be one of {sorted(_LOSSES)}, got {loss!r}")
    if solver not in ("mu", "cd"):
        raise ValueError(f"solver must be 'mu' or 'cd', got {solver!r}")
    if solver == "cd" and _LOSSES[loss] != _lib.LOSS_FROBENIUS:
        raise ValueError("solver='cd' minimises the Frobenius loss only")
    torch = _torch()
    device = require_device(device)
    lay = _LAYOUTS[layout]
    tdtype, _ = _pick_dtype(dtype, A, B)
    A_d, a_np = _to_dev(A, tdtype, device)
    B_d, _ = _to_dev(B, tdtype, device)
    bm = lay == _lib.BIN_MAJOR
    D = torch.cat([A_d, B_d], dim=0 if bm else 1)              # bin-major: (Ma + Mb, N); frame-major: (N, Ma + Mb)
    Ma = A_d.shape[0] if bm else A_d.shape[1]
    N = D.shape[1] if bm else D.shape[0]
    R = int(R)
    if not 1 <= R <= N:
        raise ValueError(f"R must be between 1 and the number of exemplars ({N}), got {R}")
    pick = torch.div(torch.arange(R, device=device) * N, R, rounding_mode="floor")
    W0 = (D[:, pick] if bm else D[pick, :]).clamp_min(1e-6).contiguous()
    G0 = torch.full((R, N) if bm else (N, R), float(torch.sqrt(D.mean() / R)), dtype=tdtype, device=device)
    if batch_size is not None:
        W, G, info = learn_dictionary_online(D, None, None, beta=2.0 if beta is None else beta, layout=layout,
                                             batch_size=batch_size, max_iter=iters, forget_factor=forget_factor, tol=tol,
                                             max_no_improvement=None, dtype=tdtype, device=device, info=True, out_w=W0,
                                             out_h=G0)
    elif beta is not None:
        W, G, info = learn_dictionary_beta(D, None, None, beta=beta, layout=layout, iters=iters, tol=tol, check_every=10,
                                           dtype=tdtype, device=device, info=True, out_w=W0, out_h=G0)
    elif solver == "cd":
        W, G, info = learn_dictionary_cd(D, None, None, layout=layout, max_iter=iters, tol=tol, dtype=tdtype, device=device,
                                         info=True, out_w=W0, out_h=G0)
    else:
        W, G, info = learn_dictionary(D, None, None, layout=layout, iters=iters, tol=tol, check_every=10, surface="sklearn",
                                      dtype=tdtype, device=device, info=True, out_w=W0, out_h=G0, loss=loss)
    Wa, Wb = (W[:Ma], W[Ma:]) if bm else (W[:, :Ma], W[:, Ma:])
    if prepared:
        return prepare_dictionary(Wa, Wb, layout=layout, dtype=tdtype, device=device), (_to_host(G) if a_np else G), info
    if a_np:
        return _to_host(Wa), _to_host(Wb), _to_host(G), info
    return Wa, Wb, G, info


_CONVEX_UPDATES = {"both": _lib.CONVEX_BOTH, "h": _lib.CONVEX_H_ONLY, "g": _lib.CONVEX_G_ONLY}


def convex_cluster_start(assign, R):
    """pymf's convex-NMF start from cluster labels (cnmf.py:77-89), float64 numpy: G0 = (one-hot + 0.01) / cluster size
    (T x R), H0 = one-hot + 0.2 (R x T)"""
    assign = np.asarray(assign)
    if assign.ndim != 1 or len(assign) < 1 or assign.min() < 0 or assign.max() >= R:
        raise ValueError(f"assign must hold one label in 0 .. {R - 1} per exemplar")
    T = len(assign)
    num = np.bincount(assign, minlength=R).astype(np.float64)
    H0 = np.zeros((R, T))
    H0[assign, np.arange(T)] = 1.0
    H0 += 0.2
    G0 = np.zeros((T, R))
    G0[np.arange(T), assign] = 1.0
    G0 += 0.01
    G0 /= num[assign].reshape(-1, 1)
    return G0, H0


def learn_dictionary_convex(X, G0, H0, *, layout, iters, update="both", check_every=1, tol=0.0, eps=1e-9, dtype=None,
                            device=None, info=False, out_g=None, out_h=None, loop_events=None, splits=0, waves=0):
    """Convex NMF on the GPU (evc_convex_learn; Ding, Li and Jordan, pymf's CNMF): X ~ (X G) H with X SIGNED and G, H >= 0,
    so that the R atoms W = X G are non-negative combinations of the exemplars (the columns of X) themselves.  X and H are
    addressed as in learn_dictionary; G is always T x R, a row per exemplar, whatever the layout.  G0 / H0: the
    non-negative start.  update: "both", or "h" / "g" to leave the other factor untouched.  The error ||X - (X G) H||_F is
    evaluated at the start and every `check_every` iterations; with tol > 0 the loop stops, from the third check on, when
    |err - err_prev| / T < tol (pymf: check_every=1, tol=2.22e-16).  At most 1056 bins, 16384 exemplars and
    min(T, 1024) atoms.

    Returns (W, G, H) (numpy in -> numpy out, device tensor in -> device tensor out), W addressed like X; with info=True
    also dict(n_iter=int, err=[1 + iters // check_every] errors (NaN where not evaluated), splits=k-ranges of the Gram
    sweeps).  out_g / out_h: device tensors updated in place (they then hold the start, G0 / H0 are ignored when None).
    splits / waves: tuning and tests, 1..16 k-ranges and 8, 4 or 2 wavefronts per workgroup of the sweeps.
    No CPU fallback: without a HIP device this raises RuntimeError."""
    if update not in _CONVEX_UPDATES:
        raise ValueError(f"update must be one of {sorted(_CONVEX_UPDATES)}, got {update!r}")
    lay = _LAYOUTS[layout]
    bm = lay == _lib.BIN_MAJOR
    g_like = G0 if G0 is not None else out_g
    xshape, gshape = tuple(getattr(X, "shape", ())), tuple(getattr(g_like, "shape", ()))
    if len(xshape) != 2 or len(gshape) != 2:
        raise ValueError(f"X and G must be 2-D, got shapes {xshape} and {gshape}")
    M, T = xshape if bm else xshape[::-1]
    R = gshape[1]
    if gshape[0] != T:
        raise ValueError(f"G must have one row per exemplar: X has {T}, G has shape {gshape}")
    if M < 1 or T < 1 or R < 1:
        raise ValueError(f"empty convex-NMF problem M={M}, T={T}, R={R}")
    if M > _lib.CONVEX_MAX_M or T > _lib.CONVEX_MAX_T or R > min(T, _lib.CONVEX_MAX_R):      # what the ABI answers with -3
        raise ValueError(f"unsupported convex-NMF shape: M = {M} bins, T = {T} exemplars, R = {R} atoms; the kernel holds at "
                         f"most {_lib.CONVEX_MAX_M} bins, {_lib.CONVEX_MAX_T} exemplars and min(T, {_lib.CONVEX_MAX_R}) atoms")
    tdtype, dcode = _pick_dtype(dtype, X, g_like)
    device = require_device(device)
    torch = _torch()
    X_d, x_np = _to_dev(X, tdtype, device)
    G_d = _factor_start(G0, out_g, "g", tdtype, device)
    H_d = _factor_start(H0, out_h, "h", tdtype, device)
    if tuple(G_d.shape) != (T, R) or tuple(H_d.shape) != ((R, T) if bm else (T, R)):
        raise ValueError(f"X {xshape}, G {tuple(G_d.shape)} and H {tuple(H_d.shape)} do not fit ({layout})")
    W_d = torch.empty((M, R) if bm else (R, M), dtype=tdtype, device=device)
    opts = _lib.ConvexOpts()
    opts.iters, opts.check_every, opts.update = int(iters), int(check_every), _CONVEX_UPDATES[update]
    opts.tol, opts.eps = float(tol), float(eps)
    opts.reserved = (int(waves) & 0xff) << 16
    _common_opts(opts, dcode, lay, loop_events, splits)
    L = _lib.lib()
    nbytes = int(L.evc_convex_workspace_bytes(M, R, T, dcode))
    extra = int(splits) - int(L.evc_convex_splits(R, T))
    if nbytes and extra > 0:                     # forced k-ranges beyond the plan's: their slabs of partial sums
        nbytes += 2 * (extra + 1) * T * R * (8 if dcode == _lib.F64 else 4) + 256
    p = types.SimpleNamespace(device=device)
    head = (X_d.data_ptr(), _ld(X_d), G_d.data_ptr(), _ld(G_d), H_d.data_ptr(), _ld(H_d), W_d.data_ptr(), _ld(W_d), M, R, T)
    (n_iter,), err = _learn_run(L, "evc_convex_learn", p, head, opts, nbytes,
                                f"unsupported convex-NMF shape M={M}, T={T}, R={R}", _n_slots(iters, check_every),
                                info or tol > 0, info)
    res = (W_d, G_d, H_d)
    if x_np and out_g is None and out_h is None:
        res = tuple(_to_host(t) for t in res)
    if info:
        res += ({"n_iter": n_iter, "err": err, "splits": _splits_info(splits, L.evc_convex_splits, R, T)},)
    return res


def compact_dictionary_convex(A, B, R, *, iters=100, tol=0.0, assign=None, layout="bin_major", dtype=None, device=None,
                              kmeans_iters=10):
    """A compact parallel dictionary of SIGNED exemplars (mel-cepstra, MFCCs): the aligned source and target exemplars are
    stacked, D = [A; B] ((Ma + Mb) x N), and factored by learn_dictionary_convex, D ~ (D G) H with G, H >= 0.  The atoms
    [Wa; Wb] = D G = [A G; B G] are non-negative combinations of the exemplars with the SAME weights on both sides, so they
    stay parallel whatever the sign of the features; (Wa, Wb) then stand in for (A, B) in convert_semi at (R / N)^2 of the
    Gram sweep's cost.

    The start is deterministic: exemplar t belongs to cluster assign[t] (default t * R // N: aligned exemplars are in time
    order, neighbours are alike; or the caller's own labels, 0 .. R-1), G0 = (one-hot + 0.01) / cluster size and
    H0 = one-hot + 0.2, pymf's construction.  assign="kmeans": the labels come from compact_dictionary_kmeans on the same
    stack (at most `kmeans_iters` rounds), a clustering on the device in place of the time-order split.  The error is
    checked every iteration (tol: pymf's stop).  Returns
    (Wa, Wb, G, H, info) in the caller's orientation (G is N x R); info as learn_dictionary_convex's."""
    torch = _torch()
    lay = _LAYOUTS[layout]
    bm = lay == _lib.BIN_MAJOR
    ashape, bshape = tuple(getattr(A, "shape", ())), tuple(getattr(B, "shape", ()))
    if len(ashape) != 2 or len(bshape) != 2 or ashape[1 if bm else 0] != bshape[1 if bm else 0]:
        raise ValueError(f"A and B must be 2-D with the same number of exemplars, got shapes {ashape} and {bshape}")
    N, R = ashape[1 if bm else 0], int(R)
    if not 1 <= R <= N:
        raise ValueError(f"R must be between 1 and the number of exemplars ({N}), got {R}")
    if isinstance(assign, str):
        if assign != "kmeans":
            raise ValueError(f"assign must be None, 'kmeans' or one label per exemplar, got {assign!r}")
        lab = compact_dictionary_kmeans(A, B, R, iters=kmeans_iters, layout=layout, dtype=dtype, device=device)[2]
        assign = lab.cpu().numpy() if isinstance(lab, torch.Tensor) else lab
    G0, H0 = convex_cluster_start((np.arange(N) * R) // N if assign is None else np.asarray(assign, dtype=np.int64), R)
    if assign is not None and len(assign) != N:
        raise ValueError(f"assign must hold one label per exemplar ({N}), got {len(assign)}")
    tdtype, _ = _pick_dtype(dtype, A, B)
    device = require_device(device)
    A_d, a_np = _to_dev(A, tdtype, device)
    B_d, _ = _to_dev(B, tdtype, device)
    D = torch.cat([A_d, B_d], dim=0 if bm else 1)
    Ma = ashape[0 if bm else 1]
    G_d = torch.from_numpy(G0).to(device=device, dtype=tdtype)
    H_d = torch.from_numpy(H0 if bm else np.ascontiguousarray(H0.T)).to(device=device, dtype=tdtype)
    W, G, H, info = learn_dictionary_convex(D, None, None, layout=layout, iters=iters, tol=tol, check_every=1, dtype=tdtype,
                                            device=device, info=True, out_g=G_d, out_h=H_d)
    Wa, Wb = (W[:Ma], W[Ma:]) if bm else (W[:, :Ma], W[:, Ma:])
    if a_np:
        return _to_host(Wa), _to_host(Wb), _to_host(G), _to_host(H), info
    return Wa, Wb, G, H, info


_KM_UPDATES = {"both": _lib.KM_BOTH, "assign": _lib.KM_ASSIGN_ONLY}
_KM_STOPS = {"none": _lib.KM_STOP_NONE, "pymf": _lib.KM_STOP_PYMF, "labels": _lib.KM_STOP_LABELS}


def kmeans(X, W0, *, layout, iters=10, stop="pymf", tol=None, update="both", dtype=None, device=None, info=False, splits=0,
           loop_events=None, redecide=False):
    """k-means on the GPU (evc_kmeans; pymf's Kmeans): the columns of X (signed allowed) are clustered around the R centres
    W0, addressed like learn_dictionary_convex's X and W.  One assignment with the start centres comes first; each of `iters`
    rounds then moves every centre to the mean of its members (update="assign": the centres stay; an empty cluster keeps its
    centre), assigns again and evaluates ||X - W[:, labels]||_F.  labels[t] is the smallest index among the nearest centres
    (Euclidean), decided as the direct form sum_m (x_m - w_m)^2 decides it.  stop: "pymf" (from the third round on,
    |err - err_prev| / T < tol, tol = 2.22e-16 unless given), "labels" (a round changed no label) or "none".  At most 1056
    bins, 2^20 samples and min(T, 4096) centres.

    Returns (W, labels) (numpy in -> numpy out, device tensor in -> device tensor out; labels int32); with info=True also
    dict(n_iter=rounds carried out, err=[1 + iters] errors (the first after the start's assignment; NaN where not evaluated),
    counts=members per centre, splits=centre ranges of the assignment).  splits / redecide: tuning and tests, 1..16 centre
    ranges, and every sample through the direct-form re-decision.
    No CPU fallback: without a HIP device this raises RuntimeError."""
    if update not in _KM_UPDATES:
        raise ValueError(f"update must be one of {sorted(_KM_UPDATES)}, got {update!r}")
    if stop not in _KM_STOPS:
        raise ValueError(f"stop must be one of {sorted(_KM_STOPS)}, got {stop!r}")
    lay = _LAYOUTS[layout]
    bm = lay == _lib.BIN_MAJOR
    xshape, wshape = tuple(getattr(X, "shape", ())), tuple(getattr(W0, "shape", ()))
    if len(xshape) != 2 or len(wshape) != 2:
        raise ValueError(f"X and W must be 2-D, got shapes {xshape} and {wshape}")
    M, T = xshape if bm else xshape[::-1]
    M2, R = wshape if bm else wshape[::-1]
    if M2 != M:
        raise ValueError(f"X {xshape} and W {wshape} do not fit ({layout})")
    if M < 1 or T < 1 or R < 1:
        raise ValueError(f"empty k-means problem M={M}, T={T}, R={R}")
    if int(iters) < 0 or int(iters) > 4096:
        raise ValueError(f"iters must be between 0 and 4096, got {iters}")
    r_max = min(T, _lib.KMEANS_MAX_R) if update == "both" else _lib.KMEANS_MAX_R        # the assignment alone: any codebook
    if M > _lib.KMEANS_MAX_M or T > _lib.KMEANS_MAX_T or R > r_max:      # what the ABI answers with -3
        raise ValueError(f"unsupported k-means shape: M = {M} bins, T = {T} samples, R = {R} centres; the kernel holds at "
                         f"most {_lib.KMEANS_MAX_M} bins, {_lib.KMEANS_MAX_T} samples and min(T, {_lib.KMEANS_MAX_R}) centres")
    tdtype, dcode = _pick_dtype(dtype, X, W0)
    device = require_device(device)
    torch = _torch()
    X_d, x_np = _to_dev(X, tdtype, device)
    W_d = _factor_start(W0, None, "w", tdtype, device)
    labels = torch.empty(T, dtype=torch.int32, device=device)
    counts = torch.empty(R, dtype=torch.int32, device=device) if info else None
    opts = _lib.KmeansOpts()
    opts.iters, opts.update, opts.stop_rule = int(iters), _KM_UPDATES[update], _KM_STOPS[stop]
    opts.tol = float(np.finfo(float).eps if stop == "pymf" else 0.0) if tol is None else float(tol)
    opts.reserved = 1 if redecide else 0
    _common_opts(opts, dcode, lay, loop_events, splits)
    L = _lib.lib()
    nbytes = int(L.evc_kmeans_workspace_bytes(M, R, T, dcode))
    extra = int(splits) - int(L.evc_kmeans_splits(R, T))
    if nbytes and extra > 0:                     # forced centre ranges beyond the plan's: their slabs of partial results
        nbytes += (extra + 1) * (T * (2 * (8 if dcode == _lib.F64 else 4) + 4) + 3 * 256)
    p = types.SimpleNamespace(device=device)
    head = (X_d.data_ptr(), _ld(X_d), W_d.data_ptr(), _ld(W_d), labels.data_ptr(), counts.data_ptr() if info else None, M, R, T)
    (n_iter,), err = _learn_run(L, "evc_kmeans", p, head, opts, nbytes, f"unsupported k-means shape M={M}, T={T}, R={R}",
                                1 + int(iters), info, info)
    res = (_to_host(W_d), _to_host(labels)) if x_np else (W_d, labels)
    if info:
        res += ({"n_iter": n_iter, "err": err, "counts": _to_host(counts) if x_np else counts,
                 "splits": _splits_info(splits, L.evc_kmeans_splits, R, T)},)
    return res


def vq(W, X, *, layout, dtype=None, device=None, splits=0, redecide=False):
    """The nearest centre of every column of X among the columns of W (pymf dist.py's vq(W, X), Euclidean, the first of
    equals): kmeans' assignment alone.  Returns the int32 labels, numpy for numpy operands."""
    return kmeans(X, W, layout=layout, iters=0, stop="none", update="assign", dtype=dtype, device=device, splits=splits,
                  redecide=redecide)[1]


def compact_dictionary_kmeans(A, B, R, *, iters=10, stop="labels", init="spread", layout="bin_major", dtype=None, device=None):
    """A compact parallel dictionary by vector quantisation: the aligned source and target exemplars are stacked,
    D = [A; B] ((Ma + Mb) x N) as in compact_dictionary_convex, and clustered by kmeans; the two halves of the R centroids are
    the parallel codebook (centroids of non-negative spectra are non-negative, so convert takes them as they stand).  The
    start centres are the exemplars at ((2 i + 1) N) // (2 R) (init="spread": aligned exemplars are in time order), or at
    the caller's R indices.  Returns (Wa, Wb, labels, info) in the caller's orientation; info as kmeans'."""
    torch = _torch()
    lay = _LAYOUTS[layout]
    bm = lay == _lib.BIN_MAJOR
    ashape, bshape = tuple(getattr(A, "shape", ())), tuple(getattr(B, "shape", ()))
    if len(ashape) != 2 or len(bshape) != 2 or ashape[1 if bm else 0] != bshape[1 if bm else 0]:
        raise ValueError(f"A and B must be 2-D with the same number of exemplars, got shapes {ashape} and {bshape}")
    N, R = ashape[1 if bm else 0], int(R)
    if not 1 <= R <= N:
        raise ValueError(f"R must be between 1 and the number of exemplars ({N}), got {R}")
    if isinstance(init, str):
        if init != "spread":
            raise ValueError(f"init must be 'spread' or R exemplar indices, got {init!r}")
        pick = ((2 * np.arange(R, dtype=np.int64) + 1) * N) // (2 * R)
    else:
        pick = np.asarray(init, dtype=np.int64)
        if pick.shape != (R,) or pick.min() < 0 or pick.max() >= N:
            raise ValueError(f"init must hold {R} exemplar indices in 0 .. {N - 1}")
    tdtype, _ = _pick_dtype(dtype, A, B)
    device = require_device(device)
    A_d, a_np = _to_dev(A, tdtype, device)
    B_d, _ = _to_dev(B, tdtype, device)
    D = torch.cat([A_d, B_d], dim=0 if bm else 1)
    Ma = ashape[0 if bm else 1]
    idx = torch.from_numpy(pick).to(device)
    W0 = (D[:, idx] if bm else D[idx, :]).contiguous()
    W, labels, info = kmeans(D, W0, layout=layout, iters=iters, stop=stop, dtype=tdtype, device=device, info=True)
    Wa, Wb = (W[:Ma], W[Ma:]) if bm else (W[:, :Ma], W[:, Ma:])
    if a_np:
        info["counts"] = _to_host(info["counts"])
        return _to_host(Wa), _to_host(Wb), _to_host(labels), info
    return Wa, Wb, labels, info


_DCL_UPDATES = {"both": _lib.DCL_BOTH, "dict": _lib.DCL_DICT_ONLY}


def learn_dictionary_deconv(X, W0_taps, H0, *, loss="frobenius", layout, iters, check_every=10, tol=0.0, l1_h=0.0, l2_h=0.0,
                            update="both", utt_offsets: Optional[Sequence[int]] = None, dtype=None, device=None, info=False,
                            out_w=None, out_h=None, loop_events=None, splits=0):
    """Convolutive NMF (NMFD) on the GPU (evc_deconv_learn): BOTH factors of X[:, t] ~ sum_tau W_tau H[:, t - tau] per
    utterance by multiplicative updates under loss "frobenius" or "kullback-leibler" - solve_activations_deconv's model with
    the taps learnt too.  W0_taps: (L, M, R) for bin_major, (L, R, M) for frame_major; X and H0 as in learn_dictionary.  Per
    iteration H by one update of solve_activations_deconv's kernels (penalties l1_h / l2_h), then every tap of W from the
    same model of the new H (scikit-learn's order; with L = 1 this is learn_dictionary's scikit-learn surface).  One error for
    the call every `check_every` iterations, and the stop when (err_prev - err) / err_at_start < tol.  update="dict": the
    activations stay at H0 and only the dictionary half runs (target taps fitted under the source's activations).
    At most 16 taps and 4096 components; 256 bins under update="both", 1056 under update="dict".  utt_offsets as in
    solve_activations_deconv: nothing crosses an utterance boundary.

    Returns (W_taps, H) in the caller's orientation (numpy in -> numpy out, device tensor in -> device tensor out); with
    info=True also dict(n_iter=int, err=[1 + iters // check_every] errors (the first at the start; NaN where not evaluated),
    splits=frame ranges of the dictionary half's sums).  out_w / out_h: device tensors updated in place (they then hold the
    start, W0_taps / H0 are ignored when None); the taps of out_w must not overlap in memory.  splits: tuning and tests,
    1..64 frame ranges.  No CPU fallback: without a HIP device this raises RuntimeError."""
    lay = _LAYOUTS[layout]
    bm = lay == _lib.BIN_MAJOR
    if loss not in _LOSSES:
        raise ValueError(f"loss must be one of {sorted(_LOSSES)}, got {loss!r}")
    if update not in _DCL_UPDATES:
        raise ValueError(f"update must be one of {sorted(_DCL_UPDATES)}, got {update!r}")
    w_src = W0_taps if W0_taps is not None else out_w
    wshape = tuple(getattr(w_src, "shape", ()))
    if len(wshape) != 3:
        raise ValueError(f"W0_taps must be 3-D (taps, rows, columns), got shape {wshape}")
    max_bins = _lib.DECONV_MAX_M if update == "both" else _lib.DECONV_MAX_MB
    bins, comps = (wshape[1], wshape[2]) if bm else (wshape[2], wshape[1])
    if wshape[0] > _lib.DECONV_MAX_TAPS or bins > max_bins or comps > _lib.DECONV_LEARN_MAX_R:     # what the ABI answers with -3
        raise ValueError(f"unsupported convolutive learning shape: {wshape[0]} taps, {bins} bins and {comps} components; "
                         f"update={update!r} holds at most {_lib.DECONV_MAX_TAPS} taps, {max_bins} bins and "
                         f"{_lib.DECONV_LEARN_MAX_R} components")
    if wshape[0] < 1:
        raise ValueError("W0_taps needs at least one tap")
    torch = _torch()
    if out_w is not None:
        if not isinstance(out_w, torch.Tensor) or out_w.dim() != 3 or (out_w.shape[2] > 1 and out_w.stride(2) != 1):
            raise ValueError("`out_w` must be a 3-D device tensor (taps, rows, columns) with unit inner stride")
        if _taps_overlap(out_w):
            raise ValueError("the taps of `out_w` overlap in memory: they are written, so tap_stride must cover one tap")
    p = _learn_operands(X, W0_taps, H0, out_w, out_h, layout, dtype, device, w_rank=3, h_written=update == "both")
    L = _lib.lib()
    M, R, T, taps = p.M, p.R, p.T, int(p.W_d.shape[0])
    n_utt, off_arr, off_ptr = _offsets(utt_offsets)
    iters, check_every = int(iters), int(check_every)
    opts = _lib.DeconvLearnOpts()
    opts.loss, opts.taps = _LOSSES[loss], taps
    opts.iters, opts.check_every, opts.update = iters, check_every, _DCL_UPDATES[update]
    opts.tol, opts.l1_h, opts.l2_h = float(tol), float(l1_h), float(l2_h)
    _common_opts(opts, p.dcode, lay, loop_events, splits)
    head = (p.X_d.data_ptr(), _ld(p.X_d), *_taps_args(p.W_d), p.H_d.data_ptr(), _ld(p.H_d), M, R, T, off_ptr, n_utt)
    (n_iter,), err = _learn_run(L, "evc_deconv_learn", p, head, opts,
                                int(L.evc_deconv_learn_workspace_bytes(M, R, T, n_utt, taps, opts.update, p.dcode)),
                                f"unsupported convolutive learning shape M={M}, R={R}, T={T}, taps={taps}",
                                _n_slots(iters, check_every), info or tol > 0, info)
    return _learn_result(p, out_w, out_h, {"n_iter": n_iter, "err": err,
                                           "splits": _splits_info(splits, L.evc_deconv_learn_splits, M, R, T, n_utt, taps)}
                         if info else None)


def compact_dictionary_deconv(A_frames, B_frames, seg_offsets, R, taps, *, iters=100, tol=0.0, loss="frobenius",
                              layout="bin_major", dtype=None, device=None):
    """A compact parallel MULTI-FRAME dictionary: what compact_dictionary is for one-frame exemplars, for taps > 1.
    A_frames / B_frames: the aligned source and target frames of the training files ((Ma, N) and (Mb, N) for bin_major,
    (N, Ma) and (N, Mb) for frame_major), seg_offsets the first frame of every file and then N, as multiframe_dictionary
    takes them.  With Ma + Mb <= 256 the stacked frames D = [A; B] are learnt jointly by learn_dictionary_deconv,
    D[:, t] ~ sum_tau [Wa_tau; Wb_tau] G[:, t - tau] within every file.  Otherwise (Wa, G) are learnt on the source frames
    (Ma <= 256) and Wb is then fitted to the target frames under update="dict" with G fixed, for `iters` iterations
    (Mb <= 1056).  The error is checked every 10 iterations.

    The start is deterministic: W0_tau = the frames tau after R evenly spaced ones (beyond their file's end: 0), floored at
    1e-6; G0 = sqrt(mean(D) / R) everywhere, D the frames the first stage factors.  With taps = 1 that is compact_dictionary's
    start.  Returns (Wa_taps, Wb_taps, G, info), ready for convert_deconv(Wa_taps, X, Wb_taps); info as
    learn_dictionary_deconv's, plus stages=1 | 2 and, for two stages, err_b (the second stage's errors)."""
    torch = _torch()
    lay = _LAYOUTS[layout]
    bm = lay == _lib.BIN_MAJOR
    taps, R = int(taps), int(R)
    if not 1 <= taps <= _lib.DECONV_MAX_TAPS:
        raise ValueError(f"taps must be between 1 and {_lib.DECONV_MAX_TAPS} taps, got {taps}")
    ashape, bshape = tuple(getattr(A_frames, "shape", ())), tuple(getattr(B_frames, "shape", ()))
    if len(ashape) != 2 or len(bshape) != 2:
        raise ValueError(f"expected 2-D matrices of frames, got shapes {ashape} and {bshape}")
    Ma, Mb, N = (ashape[0], bshape[0], ashape[1]) if bm else (ashape[1], bshape[1], ashape[0])
    joint = Ma + Mb <= _lib.DECONV_MAX_M
    if not joint and (Ma > _lib.DECONV_MAX_M or Mb > _lib.DECONV_MAX_MB):
        raise ValueError(f"unsupported compaction shape: {Ma} source and {Mb} target bins; the two-stage route holds at most "
                         f"{_lib.DECONV_MAX_M} source and {_lib.DECONV_MAX_MB} target bins")
    if not 1 <= R <= min(N, _lib.DECONV_LEARN_MAX_R):
        raise ValueError(f"R must be between 1 and min(frames, {_lib.DECONV_LEARN_MAX_R}) = "
                         f"{min(N, _lib.DECONV_LEARN_MAX_R)}, got {R}")
    device = require_device(device)
    tdtype, _ = _pick_dtype(dtype, A_frames, B_frames)
    A_d, a_np = _to_dev(A_frames, tdtype, device)
    B_d, _ = _to_dev(B_frames, tdtype, device)
    offs = [int(v) for v in seg_offsets]
    pick = torch.div(torch.arange(R, device=device) * N, R, rounding_mode="floor")

    def start(F):
        t = multiframe_dictionary(F, offs, taps, layout=layout)
        return (t[:, :, pick] if bm else t[:, pick, :]).clamp_min(1e-6).contiguous()

    def g0(F):
        return torch.full((R, N) if bm else (N, R), float(torch.sqrt(F.mean() / R)), dtype=tdtype, device=device)

    kw = dict(loss=loss, layout=layout, iters=iters, check_every=10, utt_offsets=offs, dtype=tdtype, device=device, info=True)
    if joint:
        D = torch.cat([A_d, B_d], dim=0 if bm else 1)
        W, G, info = learn_dictionary_deconv(D, None, None, tol=tol, out_w=start(D), out_h=g0(D), **kw)
        Wa, Wb = (W[:, :Ma], W[:, Ma:]) if bm else (W[:, :, :Ma], W[:, :, Ma:])
        info["stages"] = 1
    else:
        Wa, G, info = learn_dictionary_deconv(A_d, None, None, tol=tol, out_w=start(A_d), out_h=g0(A_d), **kw)
        Wb, _, info_b = learn_dictionary_deconv(B_d, None, None, update="dict", out_w=start(B_d), out_h=G, **kw)
        info["stages"], info["err_b"] = 2, info_b["err"]
    if a_np:
        return Wa.cpu().numpy(), Wb.cpu().numpy(), _to_host(G), info
    return Wa, Wb, G, info


def synthesize(B, H, *, layout="bin_major", dtype=None, device=None):
    """Y = B H (bin_major, (Mb,T)) or H B (frame_major: np.matmul(H.T, B) of
    04_align_n_nmf.py:391 with H already frames-as-rows, giving (T,Mb))."""
    device = require_device(device)
    L = _lib.lib()
    lay = _LAYOUTS[layout]
    tdtype, dcode = _pick_dtype(dtype, H, B)
    B_d, _ = _to_dev(B, tdtype, device)
    H_d, h_np = _to_dev(H, tdtype, device)
    Mb, N, T, Y = _synthesis_target(B_d.shape, H_d, lay, "B")
    _call(L, "evc_synthesize", device, (B_d.data_ptr(), _ld(B_d), H_d.data_ptr(), _ld(H_d), Y.data_ptr(), _ld(Y), Mb, N, T,
                                        lay, dcode))
    return _to_host(Y) if h_np else Y


def frame_residuals(A, X, H, *, layout="bin_major", dtype=None, device=None):
    """Per-frame squared residual sum_m (X - A H)^2 (float64, length T)."""
    torch = _torch()
    device = require_device(device)
    L = _lib.lib()
    lay = _LAYOUTS[layout]
    tdtype, dcode = _pick_dtype(dtype, X, A)
    A_d, _ = _to_dev(A, tdtype, device)
    X_d, x_np = _to_dev(X, tdtype, device)
    H_d, _ = _to_dev(H, tdtype, device)
    if lay == _lib.BIN_MAJOR:
        M, N = A_d.shape
        T = X_d.shape[1]
    else:
        N, M = A_d.shape
        T = X_d.shape[0]
    err2 = torch.zeros(max(T, 1), dtype=torch.float64, device=device)
    ws_bytes = int(L.evc_workspace_bytes(M, 0, N, T, 1, dcode, _lib.ALGO_GRAM))
    _call(L, "evc_residual", device, (A_d.data_ptr(), _ld(A_d), X_d.data_ptr(), _ld(X_d), H_d.data_ptr(), _ld(H_d), M, N, T,
                                      lay, dcode, err2.data_ptr()), ws_bytes)
    err2 = err2[:T]
    return err2.cpu().numpy() if x_np else err2


def griffin_lim(magnitude_spectrogram, fft_size, hopsamp, iterations, x0, *, device=None, want_rmse=False):
    """Griffin-Lim reconstruction on the GPU (float64): magnitudes (T, fft_size/2+1) with rows as time
    slices and the initial signal x0 (T*hopsamp + fft_size samples) -> reconstructed signal
    [, per-iteration RMSE].  Mirrors zz_audio_utilities.reconstruct_signal_griffin_lim."""
    torch = _torch()
    device = require_device(device)
    L = _lib.lib()
    mag, m_np = _to_dev(magnitude_spectrogram, torch.float64, device)
    T, nb = mag.shape
    fft_size, hopsamp, iterations = int(fft_size), int(hopsamp), int(iterations)
    if nb != fft_size // 2 + 1:
        raise ValueError(f"expected {fft_size // 2 + 1} frequency bins for fft_size={fft_size}, got {nb}")
    n = T * hopsamp + fft_size
    was_np = not isinstance(x0, torch.Tensor)
    x = torch.as_tensor(np.asarray(x0, dtype=np.float64) if was_np else x0, dtype=torch.float64).to(device).clone()
    if x.numel() != n:
        raise ValueError(f"x0 must have {n} samples, got {x.numel()}")
    ws_bytes = int(L.evc_griffin_lim_workspace_bytes(T, fft_size, hopsamp, iterations))
    if ws_bytes == 0:
        raise ValueError("unsupported Griffin-Lim configuration (fft_size must be even and >= 2)")
    rmse = np.zeros(max(iterations, 1)) if want_rmse else None
    with torch.cuda.device(device), _workspace(ws_bytes, device) as ws:
        stream = torch.cuda.current_stream(device).cuda_stream
        st = L.evc_griffin_lim(mag.data_ptr(), _ld(mag), T, fft_size, hopsamp, iterations, x.data_ptr(),
                               ws.data_ptr(), ws.numel(),
                               rmse.ctypes.data_as(C.POINTER(C.c_double)) if want_rmse else None,
                               C.c_void_p(stream))
    _lib.check(st, "evc_griffin_lim")
    out = x.cpu().numpy() if (m_np and was_np) else x
    return (out, rmse[:iterations]) if want_rmse else out


def griffin_lim_batch(magnitude_spectrograms, fft_size, hopsamp, iterations, x0s, *, device=None, want_rmse=False):
    """Griffin-Lim for several utterances in ONE call (evc_griffin_lim_batch): a list of (T_u, fft_size/2+1)
    magnitude arrays and the list of their initial signals (T_u*hopsamp + fft_size samples each) -> list of
    reconstructed signals [, (n_utt, iterations) RMSE].  One utterance leaves two thirds of the GPU idle; a batch
    does not.  Results equal per-utterance griffin_lim() calls up to the summation order of the contractions."""
    torch = _torch()
    device = require_device(device)
    L = _lib.lib()
    fft_size, hopsamp, iterations = int(fft_size), int(hopsamp), int(iterations)
    n_utt = len(magnitude_spectrograms)
    if n_utt == 0 or len(x0s) != n_utt:
        raise ValueError("need as many initial signals as magnitude spectrograms (at least one)")
    nb = fft_size // 2 + 1
    mags = [_to_dev(m, torch.float64, device) for m in magnitude_spectrograms]
    all_np = all(np_ for _, np_ in mags) and not any(isinstance(x, torch.Tensor) for x in x0s)
    off = [0]
    for m, _ in mags:
        if m.dim() != 2 or m.shape[1] != nb:
            raise ValueError(f"expected (T, {nb}) magnitudes for fft_size={fft_size}, got {tuple(m.shape)}")
        off.append(off[-1] + int(m.shape[0]))
    mag = torch.cat([m for m, _ in mags], dim=0).contiguous()
    lens = [(off[u + 1] - off[u]) * hopsamp + fft_size for u in range(n_utt)]
    xs = []
    for u, x0 in enumerate(x0s):
        x = torch.as_tensor(x0 if isinstance(x0, torch.Tensor) else np.asarray(x0, dtype=np.float64),
                            dtype=torch.float64).to(device).reshape(-1)
        if x.numel() != lens[u]:
            raise ValueError(f"x0 of utterance {u} must have {lens[u]} samples, got {x.numel()}")
        xs.append(x)
    x = torch.cat(xs)
    offs = (C.c_int * (n_utt + 1))(*off)
    ws_bytes = int(L.evc_griffin_lim_batch_workspace_bytes(offs, n_utt, fft_size, hopsamp, iterations))
    if ws_bytes == 0:
        raise ValueError("unsupported Griffin-Lim configuration (fft_size must be even and >= 2, at least one frame)")
    rmse = np.zeros((n_utt, max(iterations, 1))) if want_rmse else None
    with torch.cuda.device(device), _workspace(ws_bytes, device) as ws:
        stream = torch.cuda.current_stream(device).cuda_stream
        st = L.evc_griffin_lim_batch(mag.data_ptr(), _ld(mag), offs, n_utt, fft_size, hopsamp, iterations,
                                     x.data_ptr(), ws.data_ptr(), ws.numel(),
                                     rmse.ctypes.data_as(C.POINTER(C.c_double)) if want_rmse else None,
                                     C.c_void_p(stream))
    _lib.check(st, "evc_griffin_lim_batch")
    outs = list(torch.split(x, lens))
    if all_np:
        outs = [o.cpu().numpy() for o in outs]
    return (outs, rmse[:, :iterations]) if want_rmse else outs


def stft(y, n_fft=400, hop_length=80, *, center=True, device=None):
    """STFT front end on the GPU (float64): samples y -> (re, im), each (n_frames, n_fft/2+1) with rows
    as time slices - the transposed layout the scripts store (`lbr.core.stft(...).T`,
    04_align_n_nmf.py:422-427).  Periodic Hann window, reflect-padded centred frames (librosa's
    defaults)."""
    torch = _torch()
    device = require_device(device)
    L = _lib.lib()
    was_np = not isinstance(y, torch.Tensor)
    x = torch.as_tensor(np.asarray(y, dtype=np.float64) if was_np else y, dtype=torch.float64).to(device).contiguous()
    if x.dim() != 1:
        raise ValueError("y must be one-dimensional")
    n, n_fft, hop_length = int(x.numel()), int(n_fft), int(hop_length)
    if n_fft < 2 or n_fft % 2 or hop_length < 1:
        raise ValueError("n_fft must be even and >= 2, hop_length >= 1")
    nb = n_fft // 2 + 1
    T = int(L.evc_stft_frames(n, n_fft, hop_length, int(center))) if n else 0
    re = torch.empty(T, nb, dtype=torch.float64, device=device)
    im = torch.empty(T, nb, dtype=torch.float64, device=device)
    if T:
        with torch.cuda.device(device), \
                _workspace(int(L.evc_stft_workspace_bytes(n, n_fft, hop_length, int(center))), device) as ws:
            stream = torch.cuda.current_stream(device).cuda_stream
            st = L.evc_stft(x.data_ptr(), n, n_fft, hop_length, int(center), re.data_ptr(), nb, im.data_ptr(), nb,
                            ws.data_ptr(), ws.numel(), C.c_void_p(stream))
        _lib.check(st, "evc_stft")
    return (re.cpu().numpy(), im.cpu().numpy()) if was_np else (re, im)


def _mfcc_device(signals, sr, n_fft, hop_length, n_mfcc, n_mels, fmin, fmax, top_db, center, want_stft, device):
    """One evc_mfcc call on a list of 1-D signals (numpy arrays or device tensors).  Returns device tensors
    (mfcc (T, n_mfcc), re, im (T, nb) or None) for all utterances back to back, the frame offsets (numpy, n + 1) and
    whether every input was numpy."""
    torch = _torch()
    device = require_device(device)
    L = _lib.lib()
    sr, n_fft, hop_length, n_mfcc, n_mels = int(sr), int(n_fft), int(hop_length), int(n_mfcc), int(n_mels)
    if n_fft < 2 or n_fft % 2 or hop_length < 1:
        raise ValueError("n_fft must be even and >= 2, hop_length >= 1")
    all_np = True
    xs = []
    for y in signals:
        if isinstance(y, torch.Tensor):
            all_np = False
            t = y.to(device=device, dtype=torch.float64)
        else:
            a = np.asarray(y, dtype=np.float64)
            if not np.isfinite(a).all():
                raise ValueError("Audio buffer is not finite everywhere")       # librosa.util.valid_audio
            t = torch.from_numpy(np.ascontiguousarray(a)).to(device)
        if t.dim() != 1:
            raise ValueError("every signal must be one-dimensional")
        xs.append(t)
    n = len(xs)
    soff = np.concatenate([[0], np.cumsum([int(t.numel()) for t in xs])]).astype(np.int64)
    foff = np.concatenate([[0], np.cumsum([int(L.evc_stft_frames(int(t.numel()), n_fft, hop_length, int(center)))
                                           if t.numel() else 0 for t in xs])]).astype(np.int64)
    T, nb = int(foff[-1]), n_fft // 2 + 1
    o = _lib.MfccOpts()
    o.struct_bytes = C.sizeof(_lib.MfccOpts)
    o.sr, o.fft_size, o.hop, o.n_mels, o.n_mfcc, o.center = sr, n_fft, hop_length, n_mels, n_mfcc, int(bool(center))
    o.fmin, o.fmax, o.amin = float(fmin), 0.0 if fmax is None else float(fmax), 1e-10
    o.top_db = -1.0 if top_db is None else float(top_db)
    with torch.cuda.device(device):
        mf = torch.empty(T, n_mfcc, dtype=torch.float64, device=device)
        re = torch.empty(T, nb, dtype=torch.float64, device=device) if want_stft else None
        im = torch.empty(T, nb, dtype=torch.float64, device=device) if want_stft else None
        if n:
            x = torch.cat(xs) if n > 1 else xs[0].contiguous()
            sp = soff.ctypes.data_as(C.POINTER(C.c_long))
            ws_bytes = int(L.evc_mfcc_workspace_bytes(sp, n, C.byref(o)))
            with _workspace(ws_bytes, device) as ws:
                stream = torch.cuda.current_stream(device).cuda_stream
                st = L.evc_mfcc(x.data_ptr(), sp, n, C.byref(o), mf.data_ptr(), n_mfcc,
                                re.data_ptr() if want_stft else None, nb, im.data_ptr() if want_stft else None, nb,
                                ws.data_ptr(), ws.numel(), C.c_void_p(stream))
            _lib.check(st, "evc_mfcc")
    return mf, re, im, foff, all_np


def mfcc_batch(signals, sr=16000, n_fft=400, hop_length=80, n_mfcc=20, n_mels=128, fmin=0.0, fmax=None, top_db=80.0,
               center=True, want_stft=False, device=None):
    """MFCCs of a batch of utterances in one native call (float64): librosa.feature.mfcc(y, sr=sr, n_fft=n_fft,
    hop_length=hop_length) with librosa's defaults for the rest, as 01_make_dict_parallel.py:96-104 calls it (librosa's
    published algorithm restated; parity with the package is unpinned).  signals: 1-D arrays.  Returns a list of
    (T_u, n_mfcc) arrays, frames as rows - what `dtw_align` takes; with want_stft=True (mfccs, re, im), re / im being
    lists of the (T_u, n_fft/2+1) STFT parts of `stft`.  numpy in -> numpy out (non-finite samples raise ValueError, as
    librosa does); device tensors in -> device tensors out, with no host copy.  top_db=None: no clamp."""
    mf, re, im, foff, all_np = _mfcc_device(signals, sr, n_fft, hop_length, n_mfcc, n_mels, fmin, fmax, top_db, center,
                                            want_stft, device)

    def parts(t):
        if all_np:
            t = _to_host(t)
        return [t[int(a):int(b)] for a, b in zip(foff[:-1], foff[1:])]

    return (parts(mf), parts(re), parts(im)) if want_stft else parts(mf)


def mfcc(y, sr=16000, n_fft=400, hop_length=80, n_mfcc=20, n_mels=128, fmin=0.0, fmax=None, top_db=80.0, center=True,
         want_stft=False, device=None):
    """`mfcc_batch` for one utterance: (T, n_mfcc) [, re, im]."""
    out = mfcc_batch([y], sr, n_fft, hop_length, n_mfcc, n_mels, fmin, fmax, top_db, center, want_stft, device)
    return (out[0][0], out[1][0], out[2][0]) if want_stft else out[0]


def dtw_dictionary(dtw_a, dtw_b, src_feats, tar_feats, *, op="copy", real_part=False, dtype=None, device=None):
    """DTW alignment of parallel utterance pairs AND the gather of the aligned frames, on the GPU with no round trip of
    frames through the host (01_make_dict_parallel.py:215-249, 04_align_n_nmf.py:100-169,230-246,320-324): the paths stay
    on the device, an exclusive scan of their lengths places every pair in the dictionary, one kernel copies the rows.

      dtw_a[p], dtw_b[p]        : (frames, features) float64 - what the alignment is computed on (the script: MFCCs)
      src_feats[p], tar_feats[p]: (frames_a, cols) / (frames_b, cols_b) - the frames the dictionary is made of; complex
                                  arrays with real_part=True contribute their real parts (the script's `real`)
      op                        : "copy" | "abs" (the STFT flow stacks np.abs of the real parts, :320-324)
    Returns (A, B, row_start): device tensors N x cols and N x cols_b (frames / exemplars as rows, the orientation
    `prepare_dictionary(layout="frame_major")` and the solver take) and the first row of every pair (numpy, n_pairs + 1).
    Only N (one int) is read back - it sizes the dictionary."""
    torch = _torch()
    device = require_device(device)
    L = _lib.lib()
    n = len(dtw_a)
    if n == 0 or not (len(dtw_b) == len(src_feats) == len(tar_feats) == n):
        raise ValueError("need the same, non-zero number of utterances in every list")
    dtw_a = [np.ascontiguousarray(np.asarray(f, dtype=np.float64)) for f in dtw_a]
    dtw_b = [np.ascontiguousarray(np.asarray(f, dtype=np.float64)) for f in dtw_b]
    D = dtw_a[0].shape[1]
    if any(f.ndim != 2 or f.shape[1] != D for f in dtw_a + dtw_b):
        raise ValueError("every utterance must be (frames, features) with the same number of features")
    for fa, fb, sa, sb in zip(dtw_a, dtw_b, src_feats, tar_feats):
        if len(sa) != len(fa) or len(sb) != len(fb):
            raise ValueError("alignment features and dictionary frames must have the same number of frames per utterance")
    aoff = np.concatenate([[0], np.cumsum([len(f) for f in dtw_a])]).astype(np.int32)
    boff = np.concatenate([[0], np.cumsum([len(f) for f in dtw_b])]).astype(np.int32)

    def stack(feats):
        m = np.concatenate([np.asarray(f) for f in feats], axis=0)
        if np.iscomplexobj(m):
            if not real_part:
                raise ValueError("complex frames need real_part=True")
            base = np.float32 if m.dtype == np.complex64 else np.float64
            v = np.ascontiguousarray(m).view(base)                 # interleaved re / im: the kernel strides by 2
            return v, 2, m.shape[1]
        base = np.float32 if (m.dtype == np.float32 and dtype != "f64") else np.float64
        return np.ascontiguousarray(m.astype(base, copy=False)), 1, m.shape[1]

    sa, stride_a, cols_a = stack(src_feats)
    sb, stride_b, cols_b = stack(tar_feats)
    if sa.dtype != sb.dtype:
        sa, sb = sa.astype(np.float64), sb.astype(np.float64)
    opc = {"copy": 0, "abs": 1}[op]
    with torch.cuda.device(device):
        FA = torch.from_numpy(np.concatenate(dtw_a, axis=0)).to(device)
        FB = torch.from_numpy(np.concatenate(dtw_b, axis=0)).to(device)
        SA, SB = torch.from_numpy(sa).to(device), torch.from_numpy(sb).to(device)
    A, B, rows = _dtw_gather_device(FA, FB, aoff, boff, SA, stride_a, cols_a, SB, stride_b, cols_b, opc, device)
    return A, B, rows.cpu().numpy()


def _dtw_gather_device(FA, FB, aoff, boff, SA, stride_a, cols_a, SB, stride_b, cols_b, opc, device):
    """The device part of `dtw_dictionary`: alignment features FA / FB (device, float64, frames as rows, unit inner
    stride), the frames SA / SB the dictionary is made of (device, both float64 or both float32; element stride and
    columns each) and the frame offsets of the pairs (host int32, n + 1).  DTW, scan of the path lengths, two gathers.
    Returns device tensors (A, B, row_start); only N (one int) is read back."""
    torch = _torch()
    L = _lib.lib()
    n = len(aoff) - 1
    D = int(FA.shape[1])
    tdt = SA.dtype
    dcode = _lib.F64 if tdt == torch.float64 else _lib.F32
    ap, bp = aoff.ctypes.data_as(C.POINTER(C.c_int)), boff.ctypes.data_as(C.POINTER(C.c_int))
    ws_bytes = int(L.evc_dtw_workspace_bytes(ap, bp, n))
    if ws_bytes == 0:
        raise ValueError("utterance too long for the DTW kernel's wavefront buffers")
    cap = int(aoff[-1] + boff[-1])
    with torch.cuda.device(device):
        pa = torch.empty(max(cap, 1), dtype=torch.int32, device=device)
        pb = torch.empty(max(cap, 1), dtype=torch.int32, device=device)
        plen = torch.empty(n, dtype=torch.int32, device=device)
        rows = torch.empty(n + 1, dtype=torch.int32, device=device)
        d_aoff = torch.from_numpy(aoff[:-1].copy()).to(device)
        d_boff = torch.from_numpy(boff[:-1].copy()).to(device)
        d_poff = torch.from_numpy((aoff[:-1] + boff[:-1]).astype(np.int32)).to(device)
        stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        with _workspace(ws_bytes, device) as ws:
            st = L.evc_dtw_align(FA.data_ptr(), _ld(FA), ap, FB.data_ptr(), _ld(FB), bp, D, n, pa.data_ptr(), pb.data_ptr(),
                                 plen.data_ptr(), None, ws.data_ptr(), ws.numel(), stream)
        _lib.check(st, "evc_dtw_align")
        n_rows = C.c_int(0)
        _lib.check(L.evc_dtw_path_rows(plen.data_ptr(), n, rows.data_ptr(), C.byref(n_rows), stream), "evc_dtw_path_rows")
        N = int(n_rows.value)
        A = torch.empty((N, cols_a), dtype=tdt, device=device)
        B = torch.empty((N, cols_b), dtype=tdt, device=device)
        _lib.check(L.evc_dtw_gather_rows(SA.data_ptr(), _ld(SA), stride_a, pa.data_ptr(), plen.data_ptr(),
                                         d_aoff.data_ptr(), d_poff.data_ptr(), rows.data_ptr(), n, cols_a, opc,
                                         A.data_ptr(), cols_a, dcode, stream), "evc_dtw_gather_rows")
        _lib.check(L.evc_dtw_gather_rows(SB.data_ptr(), _ld(SB), stride_b, pb.data_ptr(), plen.data_ptr(),
                                         d_boff.data_ptr(), d_poff.data_ptr(), rows.data_ptr(), n, cols_b, opc,
                                         B.data_ptr(), cols_b, dcode, stream), "evc_dtw_gather_rows")
    return A, B, rows


def dtw_align(feats_a, feats_b, *, device=None, want_cost=False):
    """DTW paths of parallel utterance pairs on the GPU.  feats_a[p], feats_b[p]: (frames, features)
    float64 arrays of pair p.  Returns a list of (path_a, path_b) int arrays [, accumulated costs]:
    what `dtw.dtw(x, y, dist=lambda u, v: sum(np.square(u - v)))[3]` returns per pair."""
    torch = _torch()
    device = require_device(device)
    L = _lib.lib()
    feats_a = [np.ascontiguousarray(np.asarray(f, dtype=np.float64)) for f in feats_a]
    feats_b = [np.ascontiguousarray(np.asarray(f, dtype=np.float64)) for f in feats_b]
    n = len(feats_a)
    if n == 0 or len(feats_b) != n:
        raise ValueError("need the same, non-zero number of utterances on both sides")
    D = feats_a[0].shape[1]
    if any(f.ndim != 2 or f.shape[1] != D for f in feats_a + feats_b):
        raise ValueError("every utterance must be (frames, features) with the same number of features")
    aoff = np.concatenate([[0], np.cumsum([len(f) for f in feats_a])]).astype(np.int32)
    boff = np.concatenate([[0], np.cumsum([len(f) for f in feats_b])]).astype(np.int32)
    A = torch.from_numpy(np.concatenate(feats_a, axis=0)).to(device)
    B = torch.from_numpy(np.concatenate(feats_b, axis=0)).to(device)
    ap, bp = aoff.ctypes.data_as(C.POINTER(C.c_int)), boff.ctypes.data_as(C.POINTER(C.c_int))
    ws_bytes = int(L.evc_dtw_workspace_bytes(ap, bp, n))
    if ws_bytes == 0:
        raise ValueError("utterance too long for the DTW kernel's wavefront buffers")
    cap = int(aoff[-1] + boff[-1])
    pa = torch.empty(max(cap, 1), dtype=torch.int32, device=device)
    pb = torch.empty(max(cap, 1), dtype=torch.int32, device=device)
    plen = torch.empty(n, dtype=torch.int32, device=device)
    tot = torch.empty(n, dtype=torch.float64, device=device)
    with torch.cuda.device(device), _workspace(ws_bytes, device) as ws:
        stream = torch.cuda.current_stream(device).cuda_stream
        st = L.evc_dtw_align(A.data_ptr(), D, ap, B.data_ptr(), D, bp, D, n, pa.data_ptr(), pb.data_ptr(),
                             plen.data_ptr(), tot.data_ptr(), ws.data_ptr(), ws.numel(), C.c_void_p(stream))
    _lib.check(st, "evc_dtw_align")
    pa, pb, plen = pa.cpu().numpy(), pb.cpu().numpy(), plen.cpu().numpy()
    paths = []
    for p in range(n):
        o = int(aoff[p] + boff[p])
        paths.append((pa[o:o + plen[p]].astype(np.int64), pb[o:o + plen[p]].astype(np.int64)))
    return (paths, tot.cpu().numpy()) if want_cost else paths
