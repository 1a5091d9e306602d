"""The activation solve with multi-frame exemplars (evc_deconv_solve, evc_deconv_synthesize), host side: the C ABI's
declarations, struct mirror, status codes and their order, the workspace query, the numpy restatement against recorded
scikit-learn results, multiframe_dictionary on numpy and the stand-alone host program (csrc/evc_deconv_plan.h), plainly and
under the sanitizers.  No GPU needed."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deconv_restatement as dr  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def lib():
    from exemplars_vc_amd import _lib
    return _lib, _lib.lib()


def test_symbols_declared_and_exported():
    _lib, L = lib()
    hdr = open(os.path.join(ROOT, "include", "evc.h")).read()
    declared = set(re.findall(r"\b(evc_[a-z_0-9]+)\s*\(", hdr))
    for sym in ("evc_deconv_workspace_bytes", "evc_deconv_solve", "evc_deconv_synthesize"):
        assert sym in declared and sym in _lib.SYMBOLS and hasattr(L, sym)
    top = hdr[:hdr.index("#ifndef EVC_H")]
    assert "evc_deconv_solve " in top and "(13) evc_deconv_solve" in top          # listed, and its synchronisation case said


def test_opts_mirror_matches_header():
    _lib, _ = lib()
    hdr = open(os.path.join(ROOT, "include", "evc.h")).read()
    body = hdr[hdr.index("typedef struct evc_deconv_opts {"):hdr.index("} evc_deconv_opts;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for grp in re.findall(r"\b(?:int|double|void\*)\s+([a-zA-Z_0-9, ]+);", body)
             for n in grp.replace(" ", "").split(",")]
    assert names == [f[0] for f in _lib.DeconvOpts._fields_]
    assert names == ["struct_bytes", "dtype", "layout", "loss", "taps", "iters", "init_mode", "check_every", "stop_rule",
                     "reserved", "tol", "l1", "l2", "init_value", "ev_loop_start", "ev_loop_stop"]
    assert C.sizeof(_lib.DeconvOpts) == 10 * 4 + 4 * 8 + 2 * 8
    # the existing structs did not move
    assert C.sizeof(_lib.BetaOpts) == 8 * 4 + 5 * 8 + 2 * 8 and C.sizeof(_lib.TransformOpts) == 6 * 4 + 5 * 8 + 2 * 8


def _opts(_lib, **kw):
    o = _lib.DeconvOpts()
    o.struct_bytes = C.sizeof(_lib.DeconvOpts)
    o.dtype, o.layout, o.loss, o.taps, o.iters = _lib.F64, _lib.FRAME_MAJOR, _lib.LOSS_FROBENIUS, 4, 100
    o.init_mode, o.check_every, o.stop_rule, o.tol = _lib.INIT_SKLEARN, 10, _lib.STOP_SKLEARN, 1e-4
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_status_codes_and_their_order():
    _lib, L = lib()
    one = C.c_void_p(8)              # never dereferenced: every case fails validation first

    def call(o, M=25, N=17, T=70, lda=25, ldx=25, ldh=17, ws=1 << 40, A=one, X=one, H=one, wsp=one, offs=None, n_utt=1,
             tap_stride=25 * 17):
        po = None if offs is None else (C.c_int * len(offs))(*offs)
        return L.evc_deconv_solve(A, lda, tap_stride, X, ldx, H, ldh, M, N, T, po, n_utt, None if o is None else C.byref(o),
                                  wsp, ws, None, None, None)
    bad = _opts(_lib)
    bad.struct_bytes = 4
    assert call(bad) == -1 and call(None) == -1
    assert call(_opts(_lib), M=0) == -1 and call(_opts(_lib), N=0) == -1 and call(_opts(_lib), T=-1) == -1
    assert call(_opts(_lib), n_utt=0) == -1 and call(_opts(_lib), tap_stride=-1) == -1
    for ld in ("lda", "ldx"):
        assert call(_opts(_lib), **{ld: 24}) == -1
    assert call(_opts(_lib), ldh=16) == -1
    for ld in (dict(lda=16), dict(ldx=69), dict(ldh=69)):
        assert call(_opts(_lib, layout=_lib.BIN_MAJOR), **dict(dict(lda=17, ldx=70, ldh=70), **ld)) == -1
    assert call(_opts(_lib, layout=_lib.BIN_MAJOR), lda=17, ldx=70, ldh=70, ws=16) == -2
    for p in ("A", "X", "H", "wsp"):
        assert call(_opts(_lib), **{p: None}) == -1
    assert call(_opts(_lib), T=0, X=None, H=None, ws=16) == -2       # no frames: X and H are never touched
    assert call(_opts(_lib), offs=[0, 40, 30, 70], n_utt=3) == -1
    assert call(_opts(_lib), offs=[0, 30, 30, 70], n_utt=3, ws=16) == -2
    for f in ("tol", "l1", "l2"):
        assert call(_opts(_lib, **{f: -1e-4})) == -1
        assert call(_opts(_lib, **{f: float("nan")})) == -1
    for v in (float("nan"), float("inf")):
        assert call(_opts(_lib, init_value=v)) == -1
    assert call(_opts(_lib, taps=0)) == -1 and call(_opts(_lib, taps=-3)) == -1
    assert call(_opts(_lib, loss=2)) == -1 and call(_opts(_lib, loss=-1)) == -1
    assert call(_opts(_lib, init_mode=3)) == -1 and call(_opts(_lib, stop_rule=_lib.STOP_PYMF)) == -1
    assert call(_opts(_lib, dtype=7)) == -1 and call(_opts(_lib, layout=5)) == -1 and call(_opts(_lib, reserved=1)) == -1
    assert call(_opts(_lib, iters=-1)) == -1 and call(_opts(_lib, check_every=-1)) == -1
    assert call(_opts(_lib, iters=4096, check_every=1), ws=16) == -2
    assert call(_opts(_lib, iters=4097, check_every=1)) == -1                        # more than 4097 error slots
    for kw in (dict(), dict(loss=_lib.LOSS_KL), dict(taps=1), dict(taps=16), dict(iters=0), dict(tol=0.0), dict(dtype=_lib.F32)):
        assert call(_opts(_lib, **kw), ws=16) == -2, kw
    assert call(_opts(_lib), ws=int(L.evc_deconv_workspace_bytes(25, 17, 70, 1, 4, _lib.F64)) - 1) == -2
    # beyond the limits: -3, after -1 and before -2
    assert call(_opts(_lib), M=257, lda=257, ldx=257) == -3 and call(_opts(_lib, taps=17)) == -3
    assert call(_opts(_lib), M=257, lda=257, ldx=257, ws=16) == -3 and call(_opts(_lib, taps=17), ws=16) == -3
    assert call(_opts(_lib, tol=float("nan")), M=257, lda=257, ldx=257, ws=16) == -1
    assert call(_opts(_lib, taps=0), M=257, lda=257, ldx=257, ws=16) == -1
    assert call(_opts(_lib, taps=17, iters=4097, check_every=1), ws=16) == -1
    assert call(_opts(_lib), M=256, lda=256, ldx=256, ws=16) == -2

    def synth(Mb=513, N=17, T=70, taps=4, layout=_lib.FRAME_MAJOR, dtype=_lib.F64, ldb=None, ldh=None, ldy=None, B=one, H=one,
              Y=one, tap_stride=1):
        fm = layout == _lib.FRAME_MAJOR
        ldb = (Mb if fm else N) if ldb is None else ldb
        ldh = (N if fm else T) if ldh is None else ldh
        ldy = (Mb if fm else T) if ldy is None else ldy
        return L.evc_deconv_synthesize(B, ldb, tap_stride, H, ldh, Y, ldy, Mb, N, T, None, 1, taps, layout, dtype, None)
    assert synth(T=0) == 0 and synth(T=0, H=None, Y=None) == 0       # nothing to do is not an error
    assert synth(Mb=0) == -1 and synth(N=0) == -1 and synth(T=-1) == -1 and synth(taps=0) == -1 and synth(tap_stride=-1) == -1
    assert synth(B=None) == -1 and synth(H=None) == -1 and synth(Y=None) == -1
    assert synth(ldb=512) == -1 and synth(ldh=16) == -1 and synth(ldy=512) == -1
    assert synth(layout=_lib.BIN_MAJOR, ldb=16) == -1 and synth(layout=_lib.BIN_MAJOR, ldy=69) == -1
    assert synth(layout=7) == -1 and synth(dtype=7) == -1
    assert synth(Mb=1057) == -3 and synth(taps=17) == -3 and synth(Mb=1057, taps=0) == -1


def test_workspace_query():
    _lib, L = lib()
    q = L.evc_deconv_workspace_bytes
    assert q(257, 64, 100, 1, 4, 0) == 0 and q(25, 64, 100, 1, 17, 0) == 0 and q(25, 64, 100, 1, 0, 0) == 0
    assert q(256, 64, 100, 1, 16, 0) > 0 and q(256, 100000, 0, 1, 16, 1) > 0
    assert q(0, 64, 100, 1, 4, 0) == 0 and q(25, 0, 100, 1, 4, 0) == 0 and q(25, 64, -1, 1, 4, 0) == 0
    assert q(25, 64, 100, 0, 4, 0) == 0 and q(25, 64, 100, 1, 4, 9) == 0
    assert q(25, 64, 688, 1, 1, 0) < q(25, 64, 688, 1, 4, 0) < q(25, 64, 688, 1, 8, 0) < q(25, 4096, 688, 1, 8, 0)
    assert q(25, 64, 688, 1, 4, 0) < q(25, 64, 6880, 1, 4, 0) < q(25, 64, 6880, 10, 4, 0)
    assert q(201, 64, 688, 1, 4, _lib.F32) < q(201, 64, 688, 1, 4, _lib.F64)
    # the packed taps, the two images and the activation half's workspace
    for M, N, T, n, taps, dt, es in ((25, 24, 70, 1, 4, _lib.F64, 8), (201, 4096, 11008, 16, 4, _lib.F32, 4)):
        MP, NP, tiles = -(-M // 16) * 16, -(-N // 16) * 16, (T + 15) // 16 + n
        own = 2 * taps * NP * MP * es + 2 * tiles * MP * 16 * es
        extra = int(q(M, N, T, n, taps, dt)) - int(L.evc_beta_workspace_bytes(M, N, T, n, dt))
        assert own <= extra <= own + 2048
    # the existing query did not move
    assert int(L.evc_beta_workspace_bytes(25, 24, 70, 1, _lib.F64)) == 76800


@pytest.mark.parametrize("name,loss", [("sklearn_m25_n64_t32_k50", "frobenius"), ("sklearnkl_m25_n64_t32_k50", "kl"),
                                       ("sklearn_l1_m25_n256_t64_k100", "frobenius")])
def test_restatement_with_one_tap_reproduces_sklearn(name, loss):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    H, n_iter, _ = dr.solve(d["W_rows"].T[None], d["X_rows"].T, loss=loss, iters=int(d["n_iter"]), l1=float(d["l1_reg"]))
    assert n_iter.tolist() == [int(d["n_iter"])] and np.array_equal(H == 0, d["H"] == 0)
    np.testing.assert_allclose(H, d["H"], rtol=1e-12, atol=0)


@pytest.mark.parametrize("loss", ["frobenius", "kl"])
def test_restatement_properties(loss):
    offs = [0, 37, 37, 42, 58, 108]
    A, X = dr.problem(25, 64, offs[-1], 4, utt_offsets=offs)
    H, n_iter, tr = dr.solve(A, X, loss=loss, iters=40, check_every=10, utt_offsets=offs)
    assert np.isnan(tr[1]).all() and n_iter.tolist() == [40] * 5
    for u in (0, 2, 3, 4):
        assert np.all(np.diff(tr[u]) <= 0)                 # the error never rises
        Hu, _, tu = dr.solve(A, X[:, offs[u]:offs[u + 1]], loss=loss, iters=40, check_every=10)
        assert np.array_equal(H[:, offs[u]:offs[u + 1]], Hu) and np.array_equal(tr[u], tu[0])
    # the adjoint is the adjoint: <forward(H), Q> == <H, adjoint(Q)>
    rng = np.random.default_rng(3)
    Hr, Q = rng.random((64, 21)), rng.random((25, 21))
    assert np.sum(dr.forward(A, Hr) * Q) == pytest.approx(np.sum(Hr * dr.adjoint(A, Q)), rel=1e-12)
    # a stop at an interior check
    Hs, ns, ts = dr.solve(A, X[:, :37], loss=loss, iters=100, check_every=10, stop_rule="sklearn", tol=3e-3)
    assert 10 <= ns[0] < 100 and np.isnan(ts[0, ns[0] // 10 + 1:]).all() and dr.stop_margin(ts[0], 3e-3) > 1e-6


def test_multiframe_dictionary_on_numpy():
    import exemplars_vc_amd as evc
    rng = np.random.default_rng(0)
    F = rng.random((6, 11)) + 0.5
    offs = [0, 4, 4, 9, 11]
    assert np.array_equal(evc.multiframe_dictionary(F, offs, 1)[0], F)
    taps = evc.multiframe_dictionary(F, offs, 3)
    assert taps.shape == (3, 6, 11) and taps.dtype == F.dtype and isinstance(taps, np.ndarray)
    ends = [4, 4, 4, 4, 9, 9, 9, 9, 9, 11, 11]
    for tau in range(3):
        for n in range(11):
            want = F[:, n + tau] if n + tau < ends[n] else np.zeros(6)
            assert np.array_equal(taps[tau][:, n], want), (tau, n)
    fm = evc.multiframe_dictionary(np.ascontiguousarray(F.T), offs, 3, layout="frame_major")
    assert np.array_equal(fm, taps.transpose(0, 2, 1))
    import torch
    tt = evc.multiframe_dictionary(torch.from_numpy(F), offs, 3)
    assert isinstance(tt, torch.Tensor) and np.array_equal(tt.numpy(), taps)
    for bad in ([1, 11], [0, 5, 4, 11], [0, 10], [0]):
        with pytest.raises(ValueError, match="seg_offsets"):
            evc.multiframe_dictionary(F, bad, 2)
    with pytest.raises(ValueError, match="at least 1"):
        evc.multiframe_dictionary(F, offs, 0)
    # the forward model on such a dictionary: one activation places the whole segment
    H = np.zeros((11, 8))
    H[4, 2] = 2.0
    V = dr.forward(taps, H)
    assert np.array_equal(V[:, 2:5], 2.0 * F[:, 4:7]) and not V[:, :2].any() and not V[:, 5:].any()


def test_python_surface():
    import exemplars_vc_amd as evc
    for name in ("solve_activations_deconv", "synthesize_deconv", "convert_deconv", "multiframe_dictionary"):
        assert name in evc.__all__ and callable(getattr(evc, name))
    sig = inspect.signature(evc.solve_activations_deconv).parameters
    assert list(sig)[:3] == ["A_taps", "X", "H0"]
    for k in ("loss", "layout", "iters", "l1", "l2", "init", "check_every", "stop_rule", "tol", "utt_offsets", "dtype", "device",
              "info"):
        assert sig[k].kind is inspect.Parameter.KEYWORD_ONLY, k
    assert "taps" in inspect.signature(evc.compat.make_dict.aligned_dictionary).parameters
    A, X = np.ones((2, 5, 7)), np.ones((5, 3))
    with pytest.raises(ValueError, match="16 taps"):
        evc.solve_activations_deconv(np.ones((17, 5, 7)), X)
    with pytest.raises(ValueError, match="256 bins"):
        evc.solve_activations_deconv(np.ones((2, 257, 7)), np.ones((257, 3)))
    with pytest.raises(ValueError, match="256 bins"):
        evc.solve_activations_deconv(np.ones((2, 7, 257)), np.ones((3, 257)), layout="frame_major")
    with pytest.raises(ValueError, match="3-D"):
        evc.solve_activations_deconv(A[0], X)
    with pytest.raises(ValueError, match="loss"):
        evc.solve_activations_deconv(A, X, loss="itakura-saito")
    with pytest.raises(ValueError, match="1056 bins"):
        evc.synthesize_deconv(np.ones((2, 1057, 7)), np.ones((7, 3)))
    import torch
    if torch.cuda.is_available():
        H = evc.solve_activations_deconv(A, X, iters=3)
        assert H.shape == (7, 3) and np.isfinite(H).all()
    else:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            evc.solve_activations_deconv(A, X, iters=3)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            evc.synthesize_deconv(A, np.ones((7, 3)))


# ---- the host pieces of the driver (csrc/evc_deconv_plan.h) in a program of their own, plainly and under the sanitizers ----
SRC = os.path.join(ROOT, "tests", "deconv_host_main.hip")
PKG = os.path.join(ROOT, "exemplars_vc_amd")


def _program_lines(tmp, sanitize):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = os.path.join(tmp, "deconv_host_main" + ("_san" if sanitize else ""))
    cmd = [hipcc, "--offload-host-only", "-O1", "-std=c++17", SRC, "-o", exe, "-L" + PKG, "-levc_hip", "-Wl,-rpath," + PKG]
    if sanitize:
        cmd[1:1] = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-g"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr)
    return p.stdout.split("\n")[:-1]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("deconv_host"))
    return _program_lines(tmp, False), tmp


def test_host_carving_and_argument_checks(program):
    _lib, L = lib()
    carves = [ln.split() for ln in program[0] if ln.startswith("carve ")]
    assert len(carves) == 12 and not any("BAD" in ln for ln in program[0])
    for c in carves:
        M, N, T, n_utt, taps, esize, shift = (int(v) for v in c[1:7] + [c[8]])
        offs = [int(v) for v in c[10:15]]
        assert offs[0] == (256 - shift) % 256 and offs == sorted(offs) and all((o + shift) % 256 == 0 for o in offs)
        query = int(L.evc_deconv_workspace_bytes(M, N, T, n_utt, taps, _lib.F64 if esize == 8 else _lib.F32))
        assert int(c[-1]) == query and int(c[-3]) <= query
    args = {ln.split()[1]: int(ln.split()[2]) for ln in program[0] if ln.startswith("args ")}
    want = dict(ok=0, ok_exact=0, short_by_one=-2, fewer_taps_ws=-2, ok_utts=0, bad_utts=-1, no_frames_no_x=0, frames_no_x=-1,
                tap_stride_0=0, tap_stride_neg=-1, struct_bytes=-1, taps_0=-1, taps_1=0, taps_16=0, taps_17=-3,
                taps_17_small_ws=-3, loss=-1, frobenius=0, iters_neg=-1, iters_0=0, slots_4097=0, slots_4098=-1, reserved=-1,
                init_mode=-1, stop_rule=-1, tol_neg=-1, tol_0=0, l1_neg=-1, l2_nan=-1, init_value_inf=-1, dtype=-1, M_256=0,
                M_257=-3, M_257_small_ws=-3, N_100000=0, nan_before_limits=-1, taps_0_before_limits=-1)
    assert args == want
    sargs = {ln.split()[1]: int(ln.split()[2]) for ln in program[0] if ln.startswith("sargs ")}
    assert sargs == dict(ok=0, ok_bin_major=0, ok_utts=0, bad_utts=-1, no_frames_no_h=0, frames_no_h=-1, Mb_0=-1, Mb_1056=0,
                         Mb_1057=-3, taps_0=-1, taps_16=0, taps_17=-3, taps_0_before_limits=-1, layout=-1, dtype=-1,
                         tap_stride_neg=-1)


def test_the_host_program_runs_clean_under_the_sanitizers(program):
    """a stand-alone program: address + undefined-behaviour sanitizers on the host code, nothing preloaded anywhere"""
    assert _program_lines(program[1], True) == program[0]
