"""The Python wrappers of the factorisation family, pinned without a GPU: what each one hands to its C entry.

Five module-level names are replaced (monkeypatch only): `_lib.lib` by a library that records every call and answers 0,
`solver.require_device` by the CPU device, `solver._workspace` by a lease of a CPU buffer of the size asked for,
`torch.cuda.device` by a null context and `torch.cuda.current_stream` by stream 0.  The wrappers then run end to end on CPU
tensors, and every argument of every native call - pointers, leading dimensions, sizes, offsets, the whole options
struct, which optional pointers are NULL - is compared with what the inputs' shapes and strides say it must be.  Nothing
here is recorded from the code under test."""
import contextlib
import ctypes as C
import types

import numpy as np
import pytest
import torch

from exemplars_vc_amd import _lib, solver

M, N, T, MB, R = 5, 7, 9, 4, 3
OFFS2, OFFS3 = [0, 4, 9], [0, 2, 6, 9]
WS_BYTES = 4096
LAYOUTS = ("bin_major", "frame_major")
LAY = {"bin_major": _lib.BIN_MAJOR, "frame_major": _lib.FRAME_MAJOR}
# where (utt_offsets, n_utt) stand in the entries that take them
OFFSETS_AT = {"evc_nmf_solve": 9, "evc_nmf_convert": 14, "evc_cd_solve": 9, "evc_beta_solve": 9, "evc_online_transform": 9,
              "evc_deconv_solve": 10, "evc_deconv_synthesize": 10, "evc_deconv_learn": 10}


class _Any:
    def __init__(self, nonnull):
        self.nonnull = nonnull

    def __eq__(self, other):
        return not self.nonnull or (other is not None and other != 0)

    def __repr__(self):
        return "NONNULL" if self.nonnull else "ANY"


ANY, NONNULL = _Any(False), _Any(True)
STREAM0 = ("void_p", None)


def _snap(a):
    """an argument as the entry saw it, in a form that outlives the call"""
    if a is None or isinstance(a, (int, float)):
        return a
    if isinstance(a, C.c_void_p):
        return ("void_p", a.value)
    obj = getattr(a, "_obj", None)          # byref(...)
    if isinstance(obj, C.Structure):
        d = {name: getattr(obj, name) for name, _ in obj._fields_}
        d["_struct"] = type(obj).__name__
        return d
    return "ptr"                            # byref(c_int) or a POINTER instance: not NULL


class StubLib:
    def __init__(self):
        self.calls, self.queries, self.status, self.nbytes = [], [], {}, WS_BYTES

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)

        def entry(*args):
            if name == "evc_strerror":
                return b"stub status"
            if name.endswith("_bytes"):
                self.queries.append((name, tuple(args)))
                return self.nbytes
            if name.endswith("splits"):
                return 3
            if name.endswith("route"):
                return 1
            snap = [_snap(a) for a in args]
            at = OFFSETS_AT.get(name)
            if at is not None and args[at] is not None:
                snap[at] = [int(args[at][i]) for i in range(args[at + 1] + 1)]
            self.calls.append((name, snap))
            return self.status.get(name, 0)
        return entry


@pytest.fixture
def env(monkeypatch):
    stub, leases = StubLib(), []

    @contextlib.contextmanager
    def workspace(nbytes, device):
        leases.append(torch.empty(nbytes, dtype=torch.uint8))
        yield leases[-1]

    monkeypatch.setattr(_lib, "lib", lambda: stub)
    monkeypatch.setattr(solver, "require_device", lambda device=None: torch.device("cpu"))
    monkeypatch.setattr(solver, "_workspace", workspace)
    monkeypatch.setattr(torch.cuda, "device", lambda device=None: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "current_stream",
                        lambda device=None: types.SimpleNamespace(cuda_stream=0, synchronize=lambda: None))
    return types.SimpleNamespace(stub=stub, leases=leases)


def mat(bins, cols, layout, pad=0, dtype=torch.float64):
    """a (bins, cols) matrix in `layout`'s orientation; pad > 0: a view of a wider buffer (row stride = width + pad)"""
    r, c = (bins, cols) if layout == "bin_major" else (cols, bins)
    return (torch.rand(r, c + pad, dtype=dtype) + 0.1)[:, :c]


def taps_of(L, bins, cols, layout, pad=0, dtype=torch.float64):
    """(L, bins, cols) taps in `layout`'s orientation; pad > 0: rows and taps both padded"""
    r, c = (bins, cols) if layout == "bin_major" else (cols, bins)
    return (torch.rand(L, r + pad, c + pad, dtype=dtype) + 0.1)[:, :r, :c]


def oshape(bins, cols, layout):
    return (bins, cols) if layout == "bin_major" else (cols, bins)


def opts_of(cls, **fields):
    d = {name: (None if ctype is C.c_void_p else 0) for name, ctype in cls._fields_}
    d.update(struct_bytes=C.sizeof(cls), _struct=cls.__name__, **fields)
    return d


def events():
    ev = (types.SimpleNamespace(cuda_event=0x1230), types.SimpleNamespace(cuda_event=0x4560))
    return ev, dict(ev_loop_start=0x1230, ev_loop_stop=0x4560)


def the_call(env, name, k=-1):
    got, args = env.stub.calls[k]
    assert got == name
    return args


def assert_args(args, expected):
    assert len(args) == len(expected)
    for i, (a, e) in enumerate(zip(args, expected)):
        assert e == a, f"argument {i}: expected {e!r}, got {a!r}"


def lease_args(env):
    """the workspace pointer and size of the latest lease: the size is what the query answered"""
    ws = env.leases[-1]
    assert ws.numel() == env.stub.nbytes
    return [ws.data_ptr() if ws.numel() else ANY, env.stub.nbytes]


def assert_nan(a, shape):
    assert isinstance(a, np.ndarray) and a.shape == tuple(shape) and a.dtype == np.float64 and np.isnan(a).all()


# ------------------------------------------------------------------ solve_activations / convert

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("info", (False, True))
def test_solve_activations(env, layout, info):
    A, X, H0 = mat(M, N, layout, 3), mat(M, T, layout, 2), mat(N, T, layout, 1)
    ev, ev_fields = events()
    res = solver.solve_activations(A, X, H0, layout=layout, iters=20, check_every=5, stop_rule="sklearn", tol=1e-3, l1=0.5,
                                   eps_mode="clamp", utt_offsets=OFFS3, info=info, loop_events=ev, fused=False,
                                   exact_div=True, cooperative=False, all_resident=False, pair_tiles=True, lone_bin=False,
                                   fused_c=2, fused_w=8)
    assert env.stub.queries == [("evc_workspace_bytes", (M, 0, N, T, 3, _lib.F64, _lib.ALGO_AUTO))]
    assert len(env.stub.calls) == 1
    args = the_call(env, "evc_nmf_solve")
    opts = opts_of(_lib.SolveOpts, dtype=_lib.F64, layout=LAY[layout], algo=_lib.ALGO_AUTO, iters=20,
                   eps_mode=_lib.EPS_CLAMP, init_mode=_lib.INIT_GIVEN, check_every=5, stop_rule=_lib.STOP_SKLEARN,
                   reserved=1 | 2 | 4 | 16 | 32 | 64 | (2 << 8) | (8 << 16), loss=_lib.LOSS_FROBENIUS, eps=1e-15, l1=0.5,
                   tol=1e-3, info=NONNULL, **ev_fields)
    H = res[0] if info else res
    assert_args(args, [A.data_ptr(), A.stride(0), X.data_ptr(), X.stride(0), H.data_ptr(), H.stride(0), M, N, T, OFFS3, 3,
                       opts] + lease_args(env) + (["ptr", "ptr"] if info else [None, None]) + [STREAM0])
    assert isinstance(H, torch.Tensor) and tuple(H.shape) == oshape(N, T, layout)
    assert H.data_ptr() != H0.data_ptr() and torch.equal(H, H0)          # the start is a copy of H0, never H0 itself
    if info:
        assert set(res[1]) == {"n_iter", "err", "kernel", "members", "launches", "redo", "exchange", "prepared", "variant"}
        assert res[1]["n_iter"].shape == (3,) and res[1]["n_iter"].dtype == np.int32
        assert_nan(res[1]["err"], (3, 5))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_solve_activations_numpy_defaults_and_out(env, layout):
    A, X = mat(M, N, layout).numpy().astype(np.float32), mat(M, T, layout).numpy().astype(np.float32)
    H = solver.solve_activations(A, X, layout=layout, iters=7)
    args = the_call(env, "evc_nmf_solve")
    opts = opts_of(_lib.SolveOpts, dtype=_lib.F32, layout=LAY[layout], algo=_lib.ALGO_AUTO, iters=7, eps_mode=_lib.EPS_ADD,
                   init_mode=_lib.INIT_SKLEARN, eps=1e-9, info=NONNULL)
    assert_args(args, [NONNULL, A.shape[1], NONNULL, X.shape[1], NONNULL, oshape(N, T, layout)[1], M, N, T, None, 1, opts]
                + lease_args(env) + [None, None, STREAM0])
    assert env.stub.queries == [("evc_workspace_bytes", (M, 0, N, T, 1, _lib.F32, _lib.ALGO_AUTO))]
    assert isinstance(H, np.ndarray) and H.shape == oshape(N, T, layout) and H.dtype == np.float32
    # `out`: a padded device tensor receives the start and the result, and comes back itself - also for numpy operands
    out, H0 = mat(N, T, layout, 4, torch.float32), mat(N, T, layout, 0, torch.float32)
    got = solver.solve_activations(A, X, H0, layout=layout, iters=7, out=out)
    args = the_call(env, "evc_nmf_solve")
    assert got is out and args[4] == out.data_ptr() and args[5] == out.stride(0) and torch.equal(out, H0)
    assert args[11]["init_mode"] == _lib.INIT_GIVEN


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("want_h", (True, False))
def test_convert(env, layout, want_h):
    A, X, B = mat(M, N, layout, 1), mat(M, T, layout, 2), mat(MB, N, layout, 3)
    res = solver.convert(A, X, B, layout=layout, iters=4, utt_offsets=OFFS2, want_h=want_h, loss="kl", eps_mode="zero_replace")
    assert env.stub.queries == [("evc_workspace_bytes", (M, MB, N, T, 2, _lib.F64, _lib.ALGO_AUTO))]
    args = the_call(env, "evc_nmf_convert")
    H, Y = res if want_h else (None, res)
    opts = opts_of(_lib.SolveOpts, dtype=_lib.F64, layout=LAY[layout], algo=_lib.ALGO_AUTO, iters=4,
                   eps_mode=_lib.EPS_ZERO_REPLACE, init_mode=_lib.INIT_SKLEARN, loss=_lib.LOSS_KL,
                   eps=float(np.finfo(np.float32).eps), info=NONNULL)
    h_args = [H.data_ptr(), H.stride(0)] if want_h else [None, 0]
    assert_args(args, [A.data_ptr(), A.stride(0), X.data_ptr(), X.stride(0), B.data_ptr(), B.stride(0)] + h_args
                + [Y.data_ptr(), Y.stride(0), M, MB, N, T, OFFS2, 2, opts] + lease_args(env) + [None, None, STREAM0])
    assert isinstance(Y, torch.Tensor) and tuple(Y.shape) == oshape(MB, T, layout)
    if want_h:
        assert isinstance(H, torch.Tensor) and tuple(H.shape) == oshape(N, T, layout)
    # numpy in -> numpy out, the info dict appended
    res = solver.convert(A.numpy(), X.numpy(), B.numpy(), layout=layout, iters=4, check_every=2, want_h=want_h, info=True)
    assert len(res) == (3 if want_h else 2) and all(isinstance(r, np.ndarray) for r in res[:-1])
    assert res[-2].shape == oshape(MB, T, layout) and "kernel" in res[-1]
    assert_nan(res[-1]["err"], (1, 3))
    assert the_call(env, "evc_nmf_convert")[-3:-1] == ["ptr", "ptr"]


def test_convert_needs_b(env):
    with pytest.raises(ValueError, match="needs B"):
        solver.convert(mat(M, N, "bin_major"), mat(M, T, "bin_major"))


@pytest.mark.parametrize("name, call", [
    ("evc_nmf_solve", lambda A, X, W, H: solver.solve_activations(A, X)),
    ("evc_nmf_convert", lambda A, X, W, H: solver.convert(A, X, A)),
    ("evc_cd_learn", lambda A, X, W, H: solver.learn_dictionary_cd(X, W, H, layout="bin_major")),
    ("evc_beta_learn", lambda A, X, W, H: solver.learn_dictionary_beta(X, W, H, beta=0.0, layout="bin_major", iters=1))])
def test_status_raises_evc_error(env, name, call):
    ops = mat(M, N, "bin_major"), mat(M, T, "bin_major"), mat(M, R, "bin_major"), mat(R, T, "bin_major")
    call(*ops)
    env.stub.status[name] = -2
    with pytest.raises(_lib.EvcError, match=f"{name}: stub status \\(status -2\\)") as ei:
        call(*ops)
    assert ei.value.status == -2


# ------------------------------------------------------------------ the fixed-dictionary solves: cd, beta, transform, deconv

def _fixed_args(env, A, X, H, sizes, offs, opts, info, tap_stride=None):
    lda = A.stride(0) if tap_stride is None else A.stride(1)
    return ([A.data_ptr(), lda] + ([] if tap_stride is None else [tap_stride])
            + [X.data_ptr(), X.stride(0), H.data_ptr(), H.stride(0)] + list(sizes)
            + [offs, 1 if offs is None else len(offs) - 1, opts] + lease_args(env)
            + (["ptr", "ptr"] if info else [None, None]) + [STREAM0])


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("info", (False, True))
def test_solve_activations_cd(env, layout, info):
    A, X, H0 = mat(M, N, layout, 2), mat(M, T, layout, 1), mat(N, T, layout, 3)
    ev, ev_fields = events()
    res = solver.solve_activations_cd(A, X, H0, layout=layout, max_iter=6, tol=1e-3, l1=0.25, l2=0.5, utt_offsets=OFFS2,
                                      info=info, loop_events=ev)
    assert env.stub.queries == [("evc_cd_workspace_bytes", (M, N, T, 2, _lib.F64))]
    H = res[0] if info else res
    opts = opts_of(_lib.CdOpts, dtype=_lib.F64, layout=LAY[layout], init_mode=_lib.INIT_GIVEN, max_iter=6, tol=1e-3, l1=0.25,
                   l2=0.5, **ev_fields)
    assert_args(the_call(env, "evc_cd_solve"), _fixed_args(env, A, X, H, (M, N, T), OFFS2, opts, info))
    assert isinstance(H, torch.Tensor) and tuple(H.shape) == oshape(N, T, layout)
    assert H.data_ptr() != H0.data_ptr() and torch.equal(H, H0)
    if info:
        assert set(res[1]) == {"n_iter", "violation", "kernel", "launches"}
        assert res[1]["n_iter"].shape == (2,) and res[1]["kernel"] == "k_cd_sweep" and res[1]["launches"] == 7
        assert_nan(res[1]["violation"], (2, 6))
    # numpy, no start: sklearn's start, no events, numpy back
    Hn = solver.solve_activations_cd(A.numpy(), X.numpy(), layout=layout, max_iter=6)
    args = the_call(env, "evc_cd_solve")
    assert args[11] == opts_of(_lib.CdOpts, dtype=_lib.F64, layout=LAY[layout], init_mode=_lib.INIT_SKLEARN, max_iter=6,
                               tol=1e-4)
    assert args[1] == A.shape[1] and args[3] == X.shape[1] and args[9] is None and args[10] == 1
    assert isinstance(Hn, np.ndarray) and Hn.shape == oshape(N, T, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("info", (False, True))
def test_solve_activations_beta(env, layout, info):
    A, X, H0 = mat(M, N, layout, 2, torch.float32), mat(M, T, layout, 1, torch.float32), mat(N, T, layout, 3, torch.float32)
    ev, ev_fields = events()
    res = solver.solve_activations_beta(A, X, H0, beta=0.5, layout=layout, iters=11, check_every=5, stop_rule="sklearn",
                                        tol=1e-2, l1=0.25, l2=0.5, utt_offsets=OFFS3, info=info, loop_events=ev)
    assert env.stub.queries == [("evc_beta_workspace_bytes", (M, N, T, 3, _lib.F32))]
    H = res[0] if info else res
    opts = opts_of(_lib.BetaOpts, dtype=_lib.F32, layout=LAY[layout], iters=11, init_mode=_lib.INIT_GIVEN, check_every=5,
                   stop_rule=_lib.STOP_SKLEARN, beta=0.5, tol=1e-2, l1=0.25, l2=0.5, **ev_fields)
    assert_args(the_call(env, "evc_beta_solve"), _fixed_args(env, A, X, H, (M, N, T), OFFS3, opts, info))
    assert isinstance(H, torch.Tensor) and tuple(H.shape) == oshape(N, T, layout) and H.dtype == torch.float32
    assert H.data_ptr() != H0.data_ptr() and torch.equal(H, H0)
    if info:
        assert set(res[1]) == {"n_iter", "err", "kernel", "launches"}
        assert res[1]["n_iter"].shape == (3,) and res[1]["kernel"] == "k_beta_sweep" and res[1]["launches"] == 11 + 2 * 3
        assert_nan(res[1]["err"], (3, 3))
    # numpy, init="const": the start value travels, no checks -> one trace slot
    Hn, inf = solver.solve_activations_beta(A.numpy(), X.numpy(), beta=0, layout=layout, iters=4, init="const", init_value=0.3,
                                            info=True)
    args = the_call(env, "evc_beta_solve")
    assert args[11] == opts_of(_lib.BetaOpts, dtype=_lib.F32, layout=LAY[layout], iters=4, init_mode=_lib.INIT_CONST,
                               init_value=0.3)
    assert isinstance(Hn, np.ndarray) and Hn.shape == oshape(N, T, layout) and Hn.dtype == np.float32
    assert_nan(inf["err"], (1, 1))
    assert inf["launches"] == 4


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("info", (False, True))
def test_transform_online(env, layout, info):
    W, X, H0 = mat(M, R, layout, 2), mat(M, T, layout, 1), mat(R, T, layout, 3)
    out = mat(R, T, layout, 5)
    ev, ev_fields = events()
    res = solver.transform_online(W, X, beta=1.5, layout=layout, max_iter=8, tol=1e-3, l1=0.25, l2=0.5, H0=H0,
                                  utt_offsets=OFFS2, info=info, out=out, loop_events=ev)
    assert env.stub.queries == [("evc_online_transform_workspace_bytes", (M, R, T, 2, _lib.F64))]
    H = res[0] if info else res
    opts = opts_of(_lib.TransformOpts, dtype=_lib.F64, layout=LAY[layout], max_iter=8, init_mode=_lib.INIT_GIVEN, beta=1.5,
                   tol=1e-3, l1=0.25, l2=0.5, **ev_fields)
    assert_args(the_call(env, "evc_online_transform"), _fixed_args(env, W, X, out, (M, R, T), OFFS2, opts, info))
    assert H is out and torch.equal(out, H0)
    if info:
        assert set(res[1]) == {"n_iter", "change", "kernel"}
        assert res[1]["n_iter"].shape == (2,) and res[1]["kernel"] == "k_beta_sweep<change>"
        assert_nan(res[1]["change"], (2, 8))
    # numpy, the defaults; max_iter = 0 leaves an empty trace
    Hn, inf = solver.transform_online(W.numpy(), X.numpy(), layout=layout, max_iter=0, info=True)
    args = the_call(env, "evc_online_transform")
    assert args[11] == opts_of(_lib.TransformOpts, dtype=_lib.F64, layout=LAY[layout], max_iter=0,
                               init_mode=_lib.INIT_SKLEARN, beta=2.0, tol=1e-4)
    assert isinstance(Hn, np.ndarray) and Hn.shape == oshape(R, T, layout) and inf["change"].shape == (1, 0)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("taps", (1, 3))
@pytest.mark.parametrize("info", (False, True))
def test_solve_activations_deconv(env, layout, taps, info):
    A, X, H0 = taps_of(taps, M, N, layout, 2), mat(M, T, layout, 1), mat(N, T, layout, 3)
    ev, ev_fields = events()
    res = solver.solve_activations_deconv(A, X, H0, loss="kl", layout=layout, iters=10, l1=0.25, l2=0.5, check_every=3,
                                          stop_rule="sklearn", tol=1e-2, utt_offsets=OFFS3, info=info, loop_events=ev)
    assert env.stub.queries == [("evc_deconv_workspace_bytes", (M, N, T, 3, taps, _lib.F64))]
    H = res[0] if info else res
    opts = opts_of(_lib.DeconvOpts, dtype=_lib.F64, layout=LAY[layout], loss=_lib.LOSS_KL, taps=taps, iters=10,
                   init_mode=_lib.INIT_GIVEN, check_every=3, stop_rule=_lib.STOP_SKLEARN, tol=1e-2, l1=0.25, l2=0.5,
                   **ev_fields)
    assert_args(the_call(env, "evc_deconv_solve"),
                _fixed_args(env, A, X, H, (M, N, T), OFFS3, opts, info, tap_stride=A.stride(0) if taps > 1 else 0))
    assert isinstance(H, torch.Tensor) and tuple(H.shape) == oshape(N, T, layout)
    assert H.data_ptr() != H0.data_ptr() and torch.equal(H, H0)
    if info:
        assert set(res[1]) == {"n_iter", "err", "kernel", "taps"}
        assert res[1]["n_iter"].shape == (3,) and res[1]["kernel"] == "k_deconv_update" and res[1]["taps"] == taps
        assert_nan(res[1]["err"], (3, 4))
    # numpy operands, `out` given: the tensor comes back
    out = mat(N, T, layout, 2)
    got = solver.solve_activations_deconv(A.numpy(), X.numpy(), layout=layout, iters=2, out=out)
    args = the_call(env, "evc_deconv_solve")
    r, c = A.shape[1:]
    assert args[1] == c and args[2] == (r * c if taps > 1 else 0) and args[5] == out.data_ptr() and args[6] == out.stride(0)
    assert args[12] == opts_of(_lib.DeconvOpts, dtype=_lib.F64, layout=LAY[layout], taps=taps, iters=2,
                               init_mode=_lib.INIT_SKLEARN)
    assert isinstance(got, np.ndarray) and got.shape == oshape(N, T, layout)


@pytest.mark.parametrize("name, call", [
    ("evc_cd_solve", lambda A, X, **kw: solver.solve_activations_cd(A, X, **kw)),
    ("evc_beta_solve", lambda A, X, **kw: solver.solve_activations_beta(A, X, beta=1.0, **kw)),
    ("evc_online_transform", lambda A, X, **kw: solver.transform_online(A, X, **kw)),
    ("evc_deconv_solve", lambda A, X, **kw: solver.solve_activations_deconv(A[None], X, **kw))])
def test_fixed_dictionary_contiguity_and_errors(env, name, call):
    """a transposed view (inner stride != 1) arrives contiguous; a status other than 0 raises EvcError naming the entry"""
    layout = "bin_major"
    A, X = mat(M, N, layout), torch.rand(T, M, dtype=torch.float64).t()
    call(A, X, layout=layout)
    args = the_call(env, name)
    x_at = 3 if name == "evc_deconv_solve" else 2
    assert args[x_at] != X.data_ptr() and args[x_at + 1] == T
    env.stub.status[name] = -3
    with pytest.raises(_lib.EvcError, match=name) as ei:
        call(A, X, layout=layout)
    assert ei.value.status == -3


def test_fixed_dictionary_workspace_query_zero(env):
    """only the coordinate descent turns a workspace query of 0 into a ValueError; the others hand the entry 0 bytes"""
    A, X = mat(M, N, "bin_major"), mat(M, T, "bin_major")
    env.stub.nbytes = 0
    with pytest.raises(ValueError, match=f"unsupported coordinate-descent shape M={M}, N={N}, T={T}"):
        solver.solve_activations_cd(A, X)
    assert env.stub.calls == []
    solver.solve_activations_beta(A, X, beta=0.0)
    solver.transform_online(A, X, layout="bin_major")
    solver.solve_activations_deconv(A[None], X)
    solver.solve_activations(A, X)
    solver.frame_residuals(A, X, mat(N, T, "bin_major"))
    assert [c[0] for c in env.stub.calls] == ["evc_beta_solve", "evc_online_transform", "evc_deconv_solve", "evc_nmf_solve",
                                              "evc_residual"]
    assert [c[1][14 if c[0] == "evc_deconv_solve" else 13] for c in env.stub.calls] == [0] * 5


def test_validation_order(env):
    """the checks that come before the device is asked for keep their messages"""
    A, X = mat(M, N, "bin_major"), mat(M, T, "bin_major")
    wide = np.zeros((_lib.BETA_MAX_M + 1, 2))
    limit = f"unsupported beta-divergence shape: M = {_lib.BETA_MAX_M + 1} bins, the kernel holds at most {_lib.BETA_MAX_M}"
    for call in (lambda **kw: solver.solve_activations_beta(A, X, **kw),
                 lambda **kw: solver.transform_online(A, X, layout="bin_major", **kw),
                 lambda **kw: solver.learn_dictionary_beta(X, A, A, layout="bin_major", iters=1, **kw),
                 lambda **kw: solver.learn_dictionary_online(X, A, A, layout="bin_major", **kw)):
        with pytest.raises(ValueError, match="beta must be finite, got nan"):
            call(beta=float("nan"))
    for call in (lambda: solver.solve_activations_beta(wide, X, beta=1.0),
                 lambda: solver.transform_online(wide.T, X, layout="frame_major"),
                 lambda: solver.learn_dictionary_beta(wide, A, A, beta=1.0, layout="bin_major", iters=1),
                 lambda: solver.learn_dictionary_online(wide, A, A, layout="bin_major")):
        with pytest.raises(ValueError, match=limit):
            call()
    for call in (lambda: solver.solve_activations(A, X, utt_offsets=[0]),
                 lambda: solver.synthesize_deconv(A[None], mat(N, T, "bin_major"), utt_offsets=[0]),
                 lambda: solver.learn_dictionary_deconv(X, taps_of(2, M, R, "bin_major"), mat(R, T, "bin_major"),
                                                        layout="bin_major", iters=1, utt_offsets=[9])):
        with pytest.raises(ValueError, match="utt_offsets needs at least two entries"):
            call()
    with pytest.raises(ValueError, match="A and X disagree on the number of bins: 5 vs 4"):
        solver.solve_activations_cd(A, mat(4, T, "bin_major"))
    with pytest.raises(ValueError, match=r"H0 has shape \(7, 8\), expected \(7, 9\)"):
        solver.solve_activations_beta(A, X, mat(N, 8, "bin_major"), beta=1.0)
    with pytest.raises(ValueError, match="`out` must be a contiguous device tensor of the activation shape/dtype"):
        solver.transform_online(A, X, layout="bin_major", out=mat(N, T, "bin_major", 0, torch.float32))
    assert env.stub.calls == []


# ------------------------------------------------------------------ synthesis and residuals

@pytest.mark.parametrize("layout", LAYOUTS)
def test_synthesize(env, layout):
    B, H = mat(MB, N, layout, 2, torch.float32), mat(N, T, layout, 3, torch.float32)
    Y = solver.synthesize(B, H, layout=layout)
    assert_args(the_call(env, "evc_synthesize"), [B.data_ptr(), B.stride(0), H.data_ptr(), H.stride(0), Y.data_ptr(),
                                                  Y.stride(0), MB, N, T, LAY[layout], _lib.F32, STREAM0])
    assert isinstance(Y, torch.Tensor) and tuple(Y.shape) == oshape(MB, T, layout) and env.leases == []
    Yn = solver.synthesize(B.numpy(), H.numpy(), layout=layout)
    assert isinstance(Yn, np.ndarray) and Yn.shape == oshape(MB, T, layout) and Yn.dtype == np.float32
    with pytest.raises(ValueError, match=f"B and H disagree on the number of exemplars: {N} vs {N + 1}"):
        solver.synthesize(B, mat(N + 1, T, layout), layout=layout)
    env.stub.status["evc_synthesize"] = -1
    with pytest.raises(_lib.EvcError, match="evc_synthesize"):
        solver.synthesize(B, H, layout=layout)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("taps", (1, 2))
def test_synthesize_deconv(env, layout, taps):
    B, H = taps_of(taps, MB, N, layout, 2), mat(N, T, layout, 3)
    Y = solver.synthesize_deconv(B, H, layout=layout, utt_offsets=OFFS2)
    assert_args(the_call(env, "evc_deconv_synthesize"),
                [B.data_ptr(), B.stride(1), B.stride(0) if taps > 1 else 0, H.data_ptr(), H.stride(0), Y.data_ptr(),
                 Y.stride(0), MB, N, T, OFFS2, 2, taps, LAY[layout], _lib.F64, STREAM0])
    assert isinstance(Y, torch.Tensor) and tuple(Y.shape) == oshape(MB, T, layout) and env.leases == []
    Yn = solver.synthesize_deconv(B.numpy(), H.numpy(), layout=layout)
    args = the_call(env, "evc_deconv_synthesize")
    assert args[10] is None and args[11] == 1
    assert isinstance(Yn, np.ndarray) and Yn.shape == oshape(MB, T, layout)
    with pytest.raises(ValueError, match=f"B_taps and H disagree on the number of exemplars: {N} vs {N + 1}"):
        solver.synthesize_deconv(B, mat(N + 1, T, layout), layout=layout)
    env.stub.status["evc_deconv_synthesize"] = -1
    with pytest.raises(_lib.EvcError, match="evc_deconv_synthesize"):
        solver.synthesize_deconv(B, H, layout=layout)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("as_numpy", (False, True))
def test_convert_deconv(env, layout, as_numpy):
    A, X, B = taps_of(2, M, N, layout, 1), mat(M, T, layout, 2), taps_of(2, MB, N, layout, 3)
    if as_numpy:
        Y, H, inf = solver.convert_deconv(A.numpy(), X.numpy(), B.numpy(), layout=layout, utt_offsets=OFFS2, iters=3, info=True)
    else:
        Y, H = solver.convert_deconv(A, X, B, layout=layout, utt_offsets=OFFS2, iters=3)
    assert [c[0] for c in env.stub.calls] == ["evc_deconv_solve", "evc_deconv_synthesize"]
    s, y = the_call(env, "evc_deconv_solve", 0), the_call(env, "evc_deconv_synthesize", 1)
    assert y[3:5] == s[5:7] and s[7:12] == [M, N, T, OFFS2, 2] and y[7:13] == [MB, N, T, OFFS2, 2, 2]
    assert s[12]["iters"] == 3 and s[-3:-1] == (["ptr", "ptr"] if as_numpy else [None, None])
    kind = np.ndarray if as_numpy else torch.Tensor
    assert isinstance(Y, kind) and isinstance(H, kind)
    assert tuple(Y.shape) == oshape(MB, T, layout) and tuple(H.shape) == oshape(N, T, layout)
    if as_numpy:
        assert set(inf) == {"n_iter", "err", "kernel", "taps"}
    else:
        assert s[3:5] == [X.data_ptr(), X.stride(0)] and s[5] == H.data_ptr() and y[5] == Y.data_ptr()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_frame_residuals(env, layout):
    A, X, H = mat(M, N, layout, 1), mat(M, T, layout, 2), mat(N, T, layout, 3)
    e = solver.frame_residuals(A, X, H, layout=layout)
    assert env.stub.queries == [("evc_workspace_bytes", (M, 0, N, T, 1, _lib.F64, _lib.ALGO_GRAM))]
    assert_args(the_call(env, "evc_residual"), [A.data_ptr(), A.stride(0), X.data_ptr(), X.stride(0), H.data_ptr(),
                                                H.stride(0), M, N, T, LAY[layout], _lib.F64, e.data_ptr()] + lease_args(env)
                + [STREAM0])
    assert isinstance(e, torch.Tensor) and tuple(e.shape) == (T,) and e.dtype == torch.float64
    en = solver.frame_residuals(A.numpy(), X.numpy(), H.numpy(), layout=layout)
    assert isinstance(en, np.ndarray) and en.shape == (T,)
    env.stub.status["evc_residual"] = -1
    with pytest.raises(_lib.EvcError, match="evc_residual"):
        solver.frame_residuals(A, X, H, layout=layout)


# ------------------------------------------------------------------ the learners

def _learn_args(env, X, W, H, sizes, opts, quiet, info):
    return ([X.data_ptr(), X.stride(0), W.data_ptr(), W.stride(0), H.data_ptr(), H.stride(0)] + list(sizes) + [opts]
            + lease_args(env) + [None if quiet else "ptr", "ptr" if info else None, STREAM0])


def _assert_fresh_copies(W, H, W0, H0):
    """the factors come back as tensors of the caller's orientation that started as copies of W0 / H0"""
    assert isinstance(W, torch.Tensor) and isinstance(H, torch.Tensor)
    assert W.data_ptr() != W0.data_ptr() and H.data_ptr() != H0.data_ptr()
    assert torch.equal(W, W0) and torch.equal(H, H0)


LEARN_CASES = [dict(info=False, tol=0.0), dict(info=False, tol=1e-3), dict(info=True, tol=0.0)]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", LEARN_CASES)
def test_learn_dictionary(env, layout, case):
    info, tol = case["info"], case["tol"]
    X, W0, H0 = mat(M, T, layout, 1), mat(M, R, layout, 2), mat(R, T, layout, 3)
    ev, ev_fields = events()
    res = solver.learn_dictionary(X, W0, H0, layout=layout, iters=12, surface="pymf", check_every=5, tol=tol, info=info,
                                  loop_events=ev, splits=2)
    assert env.stub.queries == [("evc_learn_workspace_bytes", (M, R, T, _lib.F64))]
    W, H = res[:2]
    opts = opts_of(_lib.LearnOpts, dtype=_lib.F64, layout=LAY[layout], surface=_lib.LEARN_PYMF, iters=12, check_every=5,
                   reserved=2 << 8, loss=_lib.LOSS_FROBENIUS, tol=tol, **ev_fields)
    assert_args(the_call(env, "evc_nmf_learn"), _learn_args(env, X, W, H, (M, R, T), opts, not (info or tol > 0), info))
    _assert_fresh_copies(W, H, W0, H0)
    assert tuple(W.shape) == oshape(M, R, layout) and tuple(H.shape) == oshape(R, T, layout) and len(res) == 2 + info
    if info:
        assert set(res[2]) == {"n_iter", "err", "splits"} and res[2]["n_iter"] == 0 and res[2]["splits"] == 2
        assert_nan(res[2]["err"], (3,))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_learn_dictionary_numpy_and_out(env, layout):
    X, W0, H0 = mat(M, T, layout).numpy(), mat(M, R, layout).numpy(), mat(R, T, layout).numpy()
    W, H, inf = solver.learn_dictionary(X, W0, H0, layout=layout, iters=4, loss="kl", info=True)
    args = the_call(env, "evc_nmf_learn")
    assert args[1] == X.shape[1] and args[3] == W0.shape[1] and args[5] == H0.shape[1]
    assert args[9] == opts_of(_lib.LearnOpts, dtype=_lib.F64, layout=LAY[layout], surface=_lib.LEARN_SKLEARN, iters=4,
                              check_every=10, loss=_lib.LOSS_KL)
    assert isinstance(W, np.ndarray) and isinstance(H, np.ndarray)
    assert W.shape == oshape(M, R, layout) and H.shape == oshape(R, T, layout) and inf["splits"] == 3
    assert_nan(inf["err"], (1,))
    # out_w / out_h (padded): written in place, the start copied in, tensors back even for numpy operands
    out_w, out_h = mat(M, R, layout, 3), mat(R, T, layout, 2)
    W, H = solver.learn_dictionary(X, W0, H0, layout=layout, iters=4, out_w=out_w, out_h=out_h)
    args = the_call(env, "evc_nmf_learn")
    assert W is out_w and H is out_h
    assert args[2:6] == [out_w.data_ptr(), out_w.stride(0), out_h.data_ptr(), out_h.stride(0)]
    assert np.array_equal(out_w.numpy(), W0) and np.array_equal(out_h.numpy(), H0)
    # no start at all: out_w / out_h hold it
    before = out_w.clone()
    solver.learn_dictionary(X, None, None, layout=layout, iters=4, out_w=out_w, out_h=out_h)
    assert torch.equal(out_w, before)
    with pytest.raises(ValueError, match="`out_w` must be a device matrix of the call's dtype with unit inner stride"):
        solver.learn_dictionary(X, W0, H0, layout=layout, iters=4, out_w=mat(M, R, layout, 0, torch.float32), out_h=out_h)
    with pytest.raises(ValueError, match="do not fit"):
        solver.learn_dictionary(X, W0, mat(R, T + 1, layout).numpy(), layout=layout, iters=4)
    env.stub.nbytes = 0
    with pytest.raises(ValueError, match=f"unsupported dictionary-learning shape M={M}, R={R}, T={T}"):
        solver.learn_dictionary(X, W0, H0, layout=layout, iters=4)
    env.stub.nbytes = WS_BYTES
    env.stub.status["evc_nmf_learn"] = -3
    with pytest.raises(_lib.EvcError, match="evc_nmf_learn"):
        solver.learn_dictionary(X, W0, H0, layout=layout, iters=4)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", LEARN_CASES)
def test_learn_dictionary_beta(env, layout, case):
    info, tol = case["info"], case["tol"]
    X, W0, H0 = mat(M, T, layout, 1, torch.float32), mat(M, R, layout, 2, torch.float32), mat(R, T, layout, 3, torch.float32)
    res = solver.learn_dictionary_beta(X, W0, H0, beta=0.0, layout=layout, iters=12, check_every=4, tol=tol, l1_h=0.1,
                                       l2_h=0.2, l1_w=0.3, l2_w=0.4, info=info, splits=5, route="unfused")
    assert env.stub.queries == [("evc_beta_learn_workspace_bytes", (M, R, T, _lib.F32))]
    W, H = res[:2]
    opts = opts_of(_lib.BetaLearnOpts, dtype=_lib.F32, layout=LAY[layout], iters=12, check_every=4,
                   reserved=(2 << 16) | (5 << 8), beta=0.0, tol=tol, l1_h=0.1, l2_h=0.2, l1_w=0.3, l2_w=0.4)
    assert_args(the_call(env, "evc_beta_learn"), _learn_args(env, X, W, H, (M, R, T), opts, not (info or tol > 0), info))
    _assert_fresh_copies(W, H, W0, H0)
    if info:
        assert set(res[2]) == {"n_iter", "err", "splits", "route"}
        assert res[2]["splits"] == 5 and res[2]["route"] == "unfused"
        assert_nan(res[2]["err"], (4,))
        # the library's own choices when nothing is forced
        inf = solver.learn_dictionary_beta(X, W0, H0, beta=1.0, layout=layout, iters=12, info=True)[2]
        assert inf["splits"] == 3 and inf["route"] == "fused" and the_call(env, "evc_beta_learn")[9]["reserved"] == 0
    env.stub.nbytes = 0
    with pytest.raises(ValueError, match=f"unsupported beta-divergence learning shape M={M}, R={R}, T={T} "):
        solver.learn_dictionary_beta(X, W0, H0, beta=0.0, layout=layout, iters=1)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", LEARN_CASES)
def test_learn_dictionary_cd(env, layout, case):
    info, tol = case["info"], case["tol"]
    X, W0, H0 = mat(M, T, layout, 1), mat(M, R, layout, 2), mat(R, T, layout, 3)
    res = solver.learn_dictionary_cd(X, W0, H0, layout=layout, max_iter=6, tol=tol, l1_h=0.1, l2_h=0.2, l1_w=0.3, l2_w=0.4,
                                     update="dict", info=info, splits=2)
    assert env.stub.queries == [("evc_cd_learn_workspace_bytes", (M, R, T, _lib.F64))]
    W, H = res[:2]
    opts = opts_of(_lib.CdLearnOpts, dtype=_lib.F64, layout=LAY[layout], max_iter=6, update=_lib.CDL_DICT_ONLY,
                   reserved=2 << 8, tol=tol, l1_h=0.1, l2_h=0.2, l1_w=0.3, l2_w=0.4)
    assert_args(the_call(env, "evc_cd_learn"), _learn_args(env, X, W, H, (M, R, T), opts, not (info or tol > 0), info))
    _assert_fresh_copies(W, H, W0, H0)
    if info:
        assert set(res[2]) == {"n_iter", "violation", "splits"} and res[2]["splits"] == 2
        assert_nan(res[2]["violation"], (6, 2))
    env.stub.nbytes = 0
    with pytest.raises(ValueError, match=f"unsupported coordinate-descent learning shape M={M}, R={R}, T={T} "):
        solver.learn_dictionary_cd(X, W0, H0, layout=layout)


def _online_args(env, X, W, H, A, B, opts, quiet, info):
    return ([X.data_ptr(), X.stride(0), W.data_ptr(), W.stride(0), H.data_ptr(), H.stride(0), A.data_ptr(), B.data_ptr(),
             A.stride(0), M, R, T, opts] + lease_args(env)
            + [None if quiet else "ptr", None if quiet else "ptr", "ptr" if info else None, STREAM0])


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", [dict(info=False, tol=0.0, mni=None), dict(info=False, tol=1e-3, mni=None),
                                  dict(info=False, tol=0.0, mni=4), dict(info=True, tol=0.0, mni=-1)])
def test_learn_dictionary_online(env, layout, case):
    info, tol, mni = case["info"], case["tol"], case["mni"]
    X, W0, H0 = mat(M, T, layout, 1), mat(M, R, layout, 2), mat(R, T, layout, 3)
    ev, ev_fields = events()
    # info=True leaves the statistics in info["state"]; otherwise the caller's own state tensors are continued
    state = None if info else (torch.rand(oshape(M, R, layout), dtype=torch.float64),
                               torch.rand(oshape(M, R, layout), dtype=torch.float64))
    res = solver.learn_dictionary_online(X, W0, H0, beta=1.0, layout=layout, batch_size=4, max_iter=5, forget_factor=0.5,
                                         tol=tol, max_no_improvement=mni, l1_h=0.1, l2_h=0.2, l1_w=0.3, l2_w=0.4, state=state,
                                         info=info, route="fused", splits=2, loop_events=ev)
    assert env.stub.queries == [("evc_online_workspace_bytes", (M, R, T, 4, _lib.F64))]
    W, H = res[:2]
    opts = opts_of(_lib.OnlineOpts, dtype=_lib.F64, layout=LAY[layout], batch_size=4, max_iter=5,
                   max_no_improvement=-1 if mni is None else mni, resume=0 if state is None else 1,
                   reserved=(1 << 16) | (2 << 8), beta=1.0, tol=tol, forget_factor=0.5, l1_h=0.1, l2_h=0.2, l1_w=0.3,
                   l2_w=0.4, **ev_fields)
    quiet = not (info or tol > 0 or (mni is not None and mni >= 0))
    A, B = res[2]["state"] if info else state
    assert_args(the_call(env, "evc_online_learn"), _online_args(env, X, W, H, A, B, opts, quiet, info))
    _assert_fresh_copies(W, H, W0, H0)
    if info:
        assert set(res[2]) == {"n_iter", "n_steps", "cost", "change", "route", "state"}
        assert res[2]["n_iter"] == 0 and res[2]["n_steps"] == 0 and res[2]["route"] == "fused"
        assert A.shape == W.shape and B.shape == W.shape and A.is_contiguous() and B.is_contiguous()
        assert A.data_ptr() != B.data_ptr()
        steps = 5 * 3                    # 5 passes of ceil(9 / 4) batches
        assert_nan(res[2]["cost"], (steps,))
        assert_nan(res[2]["change"], (steps,))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_learn_dictionary_online_fresh_and_errors(env, layout):
    X, W0 = mat(M, T, layout, 1).numpy(), mat(M, R, layout).numpy()
    W, H, inf = solver.learn_dictionary_online(X, W0, None, layout=layout, batch_size=100, max_iter=3, fresh_restarts=True,
                                               fresh_restarts_max_iter=7, transform_max_iter=0, info=True)
    assert env.stub.queries == [("evc_online_fresh_workspace_bytes", (M, R, T, 100, _lib.F64))]
    args = the_call(env, "evc_online_learn_fresh")
    opts = opts_of(_lib.OnlineFreshOpts, dtype=_lib.F64, layout=LAY[layout], batch_size=100, max_iter=3, max_no_improvement=10,
                   fresh_max_iter=7, final_max_iter=0, beta=2.0, tol=1e-4, forget_factor=0.7)
    A, B = inf["state"]
    assert_args(args, [NONNULL, X.shape[1], NONNULL, W0.shape[1], NONNULL, oshape(R, T, layout)[1], A.data_ptr(),
                       B.data_ptr(), A.stride(0), M, R, T, opts] + lease_args(env) + ["ptr", "ptr", "ptr", STREAM0])
    assert isinstance(W, np.ndarray) and isinstance(H, np.ndarray)
    assert W.shape == oshape(M, R, layout) and H.shape == oshape(R, T, layout)
    assert_nan(inf["cost"], (3,))           # one batch per pass: min(batch_size, T) frames
    # transform_max_iter None: max_iter
    solver.learn_dictionary_online(X, W0, None, layout=layout, max_iter=3, fresh_restarts=True)
    assert the_call(env, "evc_online_learn_fresh")[12]["final_max_iter"] == 3
    with pytest.raises(ValueError, match="`state` must be the"):
        solver.learn_dictionary_online(X, W0, mat(R, T, layout).numpy(), layout=layout,
                                       state=(torch.zeros(2, 2, dtype=torch.float64),) * 2)
    env.stub.nbytes = 0
    with pytest.raises(ValueError, match=f"unsupported mini-batch learning shape M={M}, R={R}, T={T} "):
        solver.learn_dictionary_online(X, W0, None, layout=layout, fresh_restarts=True)
    env.stub.nbytes = WS_BYTES
    env.stub.status["evc_online_learn"] = -2
    with pytest.raises(_lib.EvcError, match="evc_online_learn:"):
        solver.learn_dictionary_online(X, W0, mat(R, T, layout).numpy(), layout=layout)


def _deconv_learn_args(env, X, W, H, offs, opts, quiet, info):
    taps = W.shape[0]
    return ([X.data_ptr(), X.stride(0), W.data_ptr(), W.stride(1), W.stride(0) if taps > 1 else 0, H.data_ptr(), H.stride(0),
             M, R, T, offs, 1 if offs is None else len(offs) - 1, opts] + lease_args(env)
            + [None if quiet else "ptr", "ptr" if info else None, STREAM0])


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("update", ("both", "dict"))
@pytest.mark.parametrize("case", LEARN_CASES)
def test_learn_dictionary_deconv(env, layout, update, case):
    info, tol = case["info"], case["tol"]
    taps = 3
    X, W0, H0 = mat(M, T, layout, 1), taps_of(taps, M, R, layout, 2), mat(R, T, layout, 3)
    ev, ev_fields = events()
    res = solver.learn_dictionary_deconv(X, W0, H0, loss="kl", layout=layout, iters=9, check_every=4, tol=tol, l1_h=0.1,
                                         l2_h=0.2, update=update, utt_offsets=OFFS3, info=info, loop_events=ev, splits=2)
    code = _lib.DCL_BOTH if update == "both" else _lib.DCL_DICT_ONLY
    assert env.stub.queries == [("evc_deconv_learn_workspace_bytes", (M, R, T, 3, taps, code, _lib.F64))]
    W, H = res[:2]
    opts = opts_of(_lib.DeconvLearnOpts, dtype=_lib.F64, layout=LAY[layout], loss=_lib.LOSS_KL, taps=taps, iters=9,
                   check_every=4, update=code, reserved=2 << 8, tol=tol, l1_h=0.1, l2_h=0.2, **ev_fields)
    assert_args(the_call(env, "evc_deconv_learn"),
                _deconv_learn_args(env, X, W, H, OFFS3, opts, not (info or tol > 0), info))
    assert isinstance(W, torch.Tensor) and isinstance(H, torch.Tensor)
    assert tuple(W.shape) == (taps,) + oshape(M, R, layout) and tuple(H.shape) == oshape(R, T, layout)
    assert W.data_ptr() != W0.data_ptr() and torch.equal(W, W0) and torch.equal(H, H0)
    # update="dict" reads the activations only: the one case in which the caller's own tensor is handed to the entry
    assert (H.data_ptr() == H0.data_ptr()) == (update == "dict")
    if info:
        assert set(res[2]) == {"n_iter", "err", "splits"} and res[2]["n_iter"] == 0 and res[2]["splits"] == 2
        assert_nan(res[2]["err"], (3,))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_learn_dictionary_deconv_taps_and_out(env, layout):
    X, H0 = mat(M, T, layout), mat(R, T, layout)
    r, c = oshape(M, R, layout)
    # overlapping taps (tap tau = rows tau .. tau + r - 1 of one buffer) are written, so they are made contiguous first
    W0 = torch.rand(r + 1, c, dtype=torch.float64).as_strided((2, r, c), (c, c, 1))
    W, H, inf = solver.learn_dictionary_deconv(X, W0, H0, layout=layout, iters=2, info=True)
    args = the_call(env, "evc_deconv_learn")
    assert args[2] == W.data_ptr() != W0.data_ptr() and args[3] == c and args[4] == r * c and torch.equal(W, W0)
    assert args[10] is None and args[11] == 1 and inf["splits"] == 3
    assert args[12] == opts_of(_lib.DeconvLearnOpts, dtype=_lib.F64, layout=LAY[layout], taps=2, iters=2, check_every=10)
    # one tap: no tap stride; numpy in -> numpy out
    Wn, Hn = solver.learn_dictionary_deconv(X.numpy(), W0[:1].numpy(), H0.numpy(), layout=layout, iters=2)
    assert the_call(env, "evc_deconv_learn")[4] == 0
    assert isinstance(Wn, np.ndarray) and isinstance(Hn, np.ndarray) and Wn.shape == (1, r, c)
    # out_w / out_h in place
    out_w, out_h = taps_of(2, M, R, layout, 2), mat(R, T, layout, 1)
    W, H = solver.learn_dictionary_deconv(X.numpy(), W0, H0, layout=layout, iters=2, out_w=out_w, out_h=out_h)
    args = the_call(env, "evc_deconv_learn")
    assert W is out_w and H is out_h and torch.equal(out_w, W0) and torch.equal(out_h, H0)
    assert args[2:7] == [out_w.data_ptr(), out_w.stride(1), out_w.stride(0), out_h.data_ptr(), out_h.stride(0)]
    with pytest.raises(ValueError, match="the taps of `out_w` overlap in memory"):
        solver.learn_dictionary_deconv(X, None, H0, layout=layout, iters=2, out_w=W0)
    with pytest.raises(ValueError, match="`out_w` must have the call's dtype"):
        solver.learn_dictionary_deconv(X, None, H0, layout=layout, iters=2, out_w=out_w.float())
    with pytest.raises(ValueError, match="`out_h` must be a device matrix of the call's dtype with unit inner stride"):
        solver.learn_dictionary_deconv(X, W0, H0, layout=layout, iters=2, out_h=out_h.float())
    with pytest.raises(ValueError, match="do not fit"):
        solver.learn_dictionary_deconv(X, W0, mat(R, T + 1, layout), layout=layout, iters=2)
    env.stub.nbytes = 0
    with pytest.raises(ValueError, match=f"unsupported convolutive learning shape M={M}, R={R}, T={T}, taps=2"):
        solver.learn_dictionary_deconv(X, W0, H0, layout=layout, iters=2)
    env.stub.nbytes = WS_BYTES
    env.stub.status["evc_deconv_learn"] = -3
    with pytest.raises(_lib.EvcError, match="evc_deconv_learn"):
        solver.learn_dictionary_deconv(X, W0, H0, layout=layout, iters=2)


# ------------------------------------------------------------------ the compactions

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("route", ("mu", "cd", "beta", "online"))
@pytest.mark.parametrize("as_numpy", (False, True))
def test_compact_dictionary(env, layout, route, as_numpy):
    A, B = mat(M, N, layout, 1), mat(MB, N, layout, 2)
    kw = {"mu": dict(loss="kl"), "cd": dict(solver="cd"), "beta": dict(beta=0.5), "online": dict(batch_size=4, beta=1.0)}[route]
    Wa, Wb, G, inf = solver.compact_dictionary(A.numpy() if as_numpy else A, B.numpy() if as_numpy else B, R, iters=6,
                                               tol=1e-3, layout=layout, **kw)
    entry = {"mu": "evc_nmf_learn", "cd": "evc_cd_learn", "beta": "evc_beta_learn", "online": "evc_online_learn"}[route]
    assert len(env.stub.calls) == 1
    args = the_call(env, entry)
    Ms = M + MB
    common = dict(dtype=_lib.F64, layout=LAY[layout])
    opts = {"mu": opts_of(_lib.LearnOpts, surface=_lib.LEARN_SKLEARN, iters=6, check_every=10, loss=_lib.LOSS_KL, tol=1e-3,
                          **common),
            "cd": opts_of(_lib.CdLearnOpts, max_iter=6, update=_lib.CDL_BOTH, tol=1e-3, **common),
            "beta": opts_of(_lib.BetaLearnOpts, iters=6, check_every=10, beta=0.5, tol=1e-3, **common),
            "online": opts_of(_lib.OnlineOpts, batch_size=4, max_iter=6, max_no_improvement=-1, beta=1.0, tol=1e-3,
                              forget_factor=0.7, **common)}[route]
    # the stacked exemplars are the frames; the start tensors are contiguous and written in place
    wld, gld = oshape(Ms, R, layout)[1], oshape(R, N, layout)[1]
    sizes_at = 9 if route == "online" else 6
    assert args[1] == oshape(Ms, N, layout)[1] and args[3] == wld and args[5] == gld
    assert args[sizes_at:sizes_at + 4] == [Ms, R, N, opts]
    assert args[sizes_at + 6:] == ["ptr"] * (3 if route == "online" else 2) + [STREAM0]
    kind = np.ndarray if as_numpy else torch.Tensor
    assert all(isinstance(t, kind) for t in (Wa, Wb, G))
    assert tuple(Wa.shape) == oshape(M, R, layout) and tuple(Wb.shape) == oshape(MB, R, layout)
    assert tuple(G.shape) == oshape(R, N, layout)
    if not as_numpy:
        assert args[2] == Wa.data_ptr() and args[4] == G.data_ptr()
    assert inf["n_iter"] == 0 and ("violation" if route == "cd" else "cost" if route == "online" else "err") in inf


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("mb", (MB, 254))
def test_compact_dictionary_deconv(env, layout, mb):
    """mb = 4: source and target stacked and learnt jointly; mb = 254 (5 + 254 > 256 bins): two stages"""
    A, B = mat(M, N, layout, 1), mat(mb, N, layout, 2)
    seg = [0, 3, N]
    Wa, Wb, G, inf = solver.compact_dictionary_deconv(A, B, seg, R, 2, iters=6, tol=1e-3, loss="kl", layout=layout)
    common = dict(dtype=_lib.F64, layout=LAY[layout], loss=_lib.LOSS_KL, taps=2, iters=6, check_every=10)
    r, c = oshape(1, R, layout)
    if mb == MB:
        assert [c_[0] for c_ in env.stub.calls] == ["evc_deconv_learn"]
        args = the_call(env, "evc_deconv_learn")
        Ms = M + mb
        assert env.stub.queries == [("evc_deconv_learn_workspace_bytes", (Ms, R, N, 2, 2, _lib.DCL_BOTH, _lib.F64))]
        assert args[7:13] == [Ms, R, N, seg, 2, opts_of(_lib.DeconvLearnOpts, update=_lib.DCL_BOTH, tol=1e-3, **common)]
        assert args[3] == oshape(Ms, R, layout)[1] and args[4] == Ms * R and args[5] == G.data_ptr()
        assert args[2] == Wa.data_ptr() and inf["stages"] == 1 and "err_b" not in inf
    else:
        assert [c_[0] for c_ in env.stub.calls] == ["evc_deconv_learn", "evc_deconv_learn"]
        a, b = the_call(env, "evc_deconv_learn", 0), the_call(env, "evc_deconv_learn", 1)
        assert a[7:13] == [M, R, N, seg, 2, opts_of(_lib.DeconvLearnOpts, update=_lib.DCL_BOTH, tol=1e-3, **common)]
        assert b[7:13] == [mb, R, N, seg, 2, opts_of(_lib.DeconvLearnOpts, update=_lib.DCL_DICT_ONLY, **common)]
        # the second stage fits the target taps under the first stage's activations, themselves
        assert a[5] == b[5] == G.data_ptr() and a[2] == Wa.data_ptr() and b[2] == Wb.data_ptr()
        assert a[4] == M * R and b[4] == mb * R
        assert inf["stages"] == 2
        assert_nan(inf["err_b"], (1,))
    assert all(isinstance(t, torch.Tensor) for t in (Wa, Wb, G))
    assert tuple(Wa.shape) == (2,) + oshape(M, R, layout) and tuple(Wb.shape) == (2,) + oshape(mb, R, layout)
    assert tuple(G.shape) == oshape(R, N, layout) and set(inf) >= {"n_iter", "err", "splits", "stages"}
    res = solver.compact_dictionary_deconv(A.numpy(), B.numpy(), seg, R, 2, iters=6, layout=layout)
    assert all(isinstance(t, np.ndarray) for t in res[:3])
