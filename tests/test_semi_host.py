"""The semi-NMF activation solve (evc_semi_solve), host side: the C ABI's declarations, struct mirror, status codes and their
order, the workspace query, the numpy restatement against recorded pymf results, the Python surface's errors and the
stand-alone host program (csrc/evc_semi_plan.h), plainly and under the sanitizers.  No GPU needed."""
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
import semi_restatement as sr  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXED = ["snmf_m25_n64_t32_k50", "snmf_m40_n130_t33_k100", "snmf_m1_n5_t3_k10", "snmf_doctest", "snmf_zero_collapse"]
FULL = "snmfw_m25_r8_t70_k30"


def lib():
    from exemplars_vc_amd import _lib
    return _lib, _lib.lib()


def nrel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), np.finfo(float).tiny))


def test_symbols_declared_and_exported():
    _lib, L = lib()
    hdr = open(os.path.join(ROOT, "include", "evc.h")).read()
    declared = set(re.findall(r"\b(evc_[a-z_0-9]+)\s*\(", hdr))
    for sym in ("evc_semi_workspace_bytes", "evc_semi_solve"):
        assert sym in declared and sym in _lib.SYMBOLS and hasattr(L, sym)
    assert "evc_semi_solve " in hdr[:hdr.index("#ifndef EVC_H")]


def test_opts_mirror_matches_header():
    _lib, _ = lib()
    hdr = open(os.path.join(ROOT, "include", "evc.h")).read()
    body = hdr[hdr.index("typedef struct evc_semi_opts {"):hdr.index("} evc_semi_opts;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for grp in re.findall(r"\b(?:int|double|void\*)\s+([a-zA-Z_0-9, ]+);", body)
             for n in grp.replace(" ", "").split(",")]
    assert names == [f[0] for f in _lib.SemiOpts._fields_]
    assert names == ["struct_bytes", "dtype", "layout", "iters", "init_mode", "check_every", "stop_rule", "reserved", "eps", "tol",
                     "init_value", "ev_loop_start", "ev_loop_stop"]
    assert C.sizeof(_lib.SemiOpts) == 8 * 4 + 3 * 8 + 2 * 8
    # the existing structs did not move
    assert C.sizeof(_lib.BetaOpts) == 8 * 4 + 5 * 8 + 2 * 8 and C.sizeof(_lib.DeconvOpts) == 10 * 4 + 4 * 8 + 2 * 8


def _opts(_lib, **kw):
    o = _lib.SemiOpts()
    o.struct_bytes = C.sizeof(_lib.SemiOpts)
    o.dtype, o.layout, o.iters = _lib.F64, _lib.FRAME_MAJOR, 100
    o.init_mode, o.check_every, o.stop_rule, o.tol, o.eps = _lib.INIT_GIVEN, 1, _lib.STOP_PYMF, 2.22e-16, 1e-9
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_status_codes_and_their_order():
    _lib, L = lib()
    one = C.c_void_p(8)              # never dereferenced: every case fails validation first

    def call(o, M=25, N=17, T=70, lda=25, ldx=25, ldh=17, ws=16, A=one, X=one, H=one, wsp=one, offs=None, n_utt=1):
        po = None if offs is None else (C.c_int * len(offs))(*offs)
        return L.evc_semi_solve(A, lda, X, ldx, H, ldh, M, N, T, po, n_utt, None if o is None else C.byref(o), wsp, ws, None,
                                None, None)
    # every valid call below is handed a 16-byte workspace: it gets as far as -2 and touches no device
    assert call(_opts(_lib)) == -2
    bad = _opts(_lib)
    bad.struct_bytes = 4
    assert call(bad) == -1 and call(None) == -1
    assert call(_opts(_lib), M=0) == -1 and call(_opts(_lib), N=0) == -1 and call(_opts(_lib), T=-1) == -1
    assert call(_opts(_lib), n_utt=0) == -1
    for ld in ("lda", "ldx"):
        assert call(_opts(_lib), **{ld: 24}) == -1
    assert call(_opts(_lib), ldh=16) == -1
    for ld in (dict(lda=16), dict(ldx=69), dict(ldh=69)):
        assert call(_opts(_lib, layout=_lib.BIN_MAJOR), **dict(dict(lda=17, ldx=70, ldh=70), **ld)) == -1
    assert call(_opts(_lib, layout=_lib.BIN_MAJOR), lda=17, ldx=70, ldh=70) == -2
    for p in ("A", "X", "H", "wsp"):
        assert call(_opts(_lib), **{p: None}) == -1
    assert call(_opts(_lib), T=0, X=None, H=None) == -2              # no frames: X and H are never touched
    assert call(_opts(_lib), offs=[0, 40, 30, 70], n_utt=3) == -1
    assert call(_opts(_lib), offs=[0, 30, 30, 70], n_utt=3) == -2
    for f in ("tol", "eps"):
        assert call(_opts(_lib, **{f: -1e-12})) == -1 and call(_opts(_lib, **{f: float("nan")})) == -1
        assert call(_opts(_lib, **{f: 0.0})) == -2
    assert call(_opts(_lib, eps=float("inf"))) == -1
    for v in (float("nan"), float("inf")):
        assert call(_opts(_lib, init_value=v)) == -1
    assert call(_opts(_lib, init_mode=_lib.INIT_SKLEARN)) == -1 and call(_opts(_lib, init_mode=3)) == -1
    assert call(_opts(_lib, init_mode=_lib.INIT_CONST, init_value=0.5)) == -2
    assert call(_opts(_lib, stop_rule=_lib.STOP_SKLEARN)) == -1 and call(_opts(_lib, stop_rule=3)) == -1
    assert call(_opts(_lib, stop_rule=_lib.STOP_NONE)) == -2
    assert call(_opts(_lib, dtype=7)) == -1 and call(_opts(_lib, layout=5)) == -1 and call(_opts(_lib, reserved=1)) == -1
    assert call(_opts(_lib, iters=-1)) == -1 and call(_opts(_lib, check_every=-1)) == -1
    assert call(_opts(_lib, iters=4096)) == -2 and call(_opts(_lib, iters=0)) == -2 and call(_opts(_lib, dtype=_lib.F32)) == -2
    assert call(_opts(_lib, iters=4097)) == -1                                        # more than 4097 error slots
    assert call(_opts(_lib, iters=40970, check_every=10)) == -1 and call(_opts(_lib, iters=40969, check_every=10)) == -2
    assert call(_opts(_lib), ws=int(L.evc_semi_workspace_bytes(25, 17, 70, 1, _lib.F64)) - 1) == -2
    # beyond the limits: -3, after every -1 and before -2, even with a tiny workspace
    assert call(_opts(_lib), M=1057, lda=1057, ldx=1057) == -3 and call(_opts(_lib), N=16385, ldh=16385) == -3
    assert call(_opts(_lib), M=1057, lda=1057, ldx=1057, ws=1 << 40) == -3
    assert call(_opts(_lib), N=16385, ldh=16385, ws=1 << 40) == -3
    assert call(_opts(_lib), M=1056, lda=1056, ldx=1056) == -2 and call(_opts(_lib), N=16384, ldh=16384) == -2
    assert call(_opts(_lib, tol=float("nan")), M=1057, lda=1057, ldx=1057) == -1
    assert call(_opts(_lib, reserved=4), N=16385, ldh=16385) == -1
    assert call(_opts(_lib, iters=4097), N=16385, ldh=16385) == -1
    assert call(_opts(_lib), M=1057, lda=1057, ldx=1057, X=None) == -1
    assert call(_opts(_lib), N=16385, ldh=16384) == -1


def test_workspace_query():
    _lib, L = lib()
    q = L.evc_semi_workspace_bytes
    assert q(1057, 64, 100, 1, 0) == 0 and q(25, 16385, 100, 1, 0) == 0
    assert q(0, 64, 100, 1, 0) == 0 and q(25, 0, 100, 1, 0) == 0 and q(25, 64, -1, 1, 0) == 0
    assert q(25, 64, 100, 0, 0) == 0 and q(25, 64, 100, 1, 9) == 0
    assert q(1056, 64, 100, 1, 0) > 0 and q(25, 64, 0, 1, 1) > 0
    assert q(25, 64, 688, 1, 0) < q(25, 129, 688, 1, 0) < q(25, 4096, 688, 1, 0) < q(25, 4096, 6880, 1, 0) < q(25, 4096, 6880, 10, 0)
    assert q(25, 64, 688, 1, _lib.F32) < q(25, 64, 688, 1, _lib.F64) and q(25, 64, 688, 1, 0) < q(201, 64, 688, 1, 0)
    # G (padded to whole row blocks of 128), P, the second H, A H at a check, the per-frame and per-utterance state
    for M, N, T, n, dt, es in ((25, 64, 32, 1, _lib.F64, 8), (25, 4096, 11008, 16, _lib.F32, 4), (40, 130, 33, 2, _lib.F64, 8)):
        NP = -(-N // 128) * 128
        own = NP * NP * es + 2 * N * T * es + T * M * es + T * 12 + n * (4097 * 8 + 16) + 4
        assert own <= int(q(M, N, T, n, dt)) <= own + 11 * 256
    assert 2 << 30 <= int(q(25, 16384, 688, 1, _lib.F64)) < (2 << 30) + (1 << 28)          # the 2 GiB Gram matrix
    # the existing query did not move
    assert int(L.evc_beta_workspace_bytes(25, 24, 70, 1, _lib.F64)) == 76800


@pytest.mark.parametrize("name", FIXED)
def test_restatement_reproduces_pymf(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    niter, T = int(d["niter"]), d["data"].shape[1]
    H, n_iter, tr = sr.solve(d["W"], d["data"], d["H0"], niter, check_every=1, stop_rule="pymf", tol=sr.PYMF_TOL)
    ferr = sr.pymf_ferr(tr[0], int(n_iter[0]), niter, T)
    print(name, "H", nrel(H, d["H"]), "ferr", nrel(ferr, d["ferr"]) if len(ferr) == len(d["ferr"]) else None)
    assert int(n_iter[0]) == int(d["n_iter"]) and len(ferr) == len(d["ferr"])
    assert nrel(H, d["H"]) <= 1e-12 and nrel(ferr, d["ferr"]) <= 1e-12
    assert np.array_equal(H == 0, d["H"] == 0)
    assert np.all(np.diff(tr[0, 1:1 + int(n_iter[0])]) <= 0)           # the error never rises
    assert (H >= 0).all() and float(d["frobenius_norm"]) == pytest.approx(sr.frobenius(d["W"], d["data"], H), rel=1e-12)


def test_zero_collapse_stops_with_a_difference_of_exactly_zero():
    d = np.load(os.path.join(GOLDEN, "snmf_zero_collapse.npz"))
    H, n_iter, tr = sr.solve(d["W"], d["data"], d["H0"], 20, check_every=1, stop_rule="pymf", tol=sr.PYMF_TOL)
    assert not H.any() and not d["H"].any() and n_iter.tolist() == [3] and len(d["ferr"]) == 2
    assert tr[0, 1] == tr[0, 2] == tr[0, 3] == 1.0 and np.isnan(tr[0, 4:]).all()
    H1, _, _ = sr.solve(d["W"], d["data"], d["H0"], 1)
    assert not H1.any()                                                # exactly 0 after ONE update


def test_restatement_reproduces_the_default_call():
    d = np.load(os.path.join(GOLDEN, FULL + ".npz"))
    W, H, ferr = sr.factorize_w(d["data"], d["H0"], int(d["niter"]))
    print(FULL, "W", nrel(W, d["W"]), "H", nrel(H, d["H"]), "ferr", nrel(ferr, d["ferr"]))
    assert len(ferr) == len(d["ferr"]) and np.array_equal(H == 0, d["H"] == 0)
    assert nrel(W, d["W"]) <= 1e-12 and nrel(H, d["H"]) <= 1e-12 and nrel(ferr, d["ferr"]) <= 1e-12
    assert np.all(np.diff(ferr) <= 0)


def test_restatement_batch_equals_per_utterance():
    offs = [0, 37, 37, 40, 90]
    A, X, H0 = sr.problem(25, 33, 90, 5)
    H, n_iter, tr = sr.solve(A, X, H0, 12, check_every=2, utt_offsets=offs)
    assert np.isnan(tr[1]).all() and n_iter.tolist() == [12] * 4 and tr.shape == (4, 7)
    for u in (0, 2, 3):
        Hu, _, tu = sr.solve(A, X[:, offs[u]:offs[u + 1]], H0[:, offs[u]:offs[u + 1]], 12, check_every=2)
        assert np.array_equal(H[:, offs[u]:offs[u + 1]], Hu) and np.array_equal(tr[u], tu[0])


def test_python_surface():
    import exemplars_vc_amd as evc
    from exemplars_vc_amd.compat import pymf
    for name in ("solve_activations_semi", "convert_semi"):
        assert name in evc.__all__ and callable(getattr(evc, name))
    sig = inspect.signature(evc.solve_activations_semi).parameters
    assert list(sig)[:3] == ["A", "X", "H0"] and sig["eps"].default == 1e-9
    for k in ("layout", "iters", "eps", "check_every", "stop_rule", "tol", "utt_offsets", "dtype", "device", "info"):
        assert sig[k].kind is inspect.Parameter.KEYWORD_ONLY, k
    assert list(inspect.signature(evc.convert_semi).parameters)[:3] == ["A", "B", "X"]
    fsig = inspect.signature(pymf.SNMF.factorize).parameters
    assert list(fsig)[1:] == ["niter", "show_progress", "compute_w", "compute_h", "compute_err"]
    assert fsig["niter"].default == 100 and fsig["compute_w"].default is True
    for attr in ("frobenius_norm", "residual", "factorize"):
        assert callable(getattr(pymf.SNMF, attr))
    mdl = pymf.SNMF(np.array([[1.5], [1.2]]), num_bases=2)
    assert mdl.data.shape == (2, 1) and mdl._num_bases == 2
    with pytest.raises(AttributeError, match="set .W"):
        mdl.factorize(niter=1, compute_w=False)
    A, X, H0 = np.ones((5, 7)), -np.ones((5, 3)), np.ones((7, 3))
    with pytest.raises(ValueError, match="number of bins"):
        evc.solve_activations_semi(A, np.ones((4, 3)), H0)
    with pytest.raises(ValueError, match="number of bins"):
        evc.solve_activations_semi(A.T, np.ones((3, 4)), H0.T, layout="frame_major")
    with pytest.raises(ValueError, match="2-D"):
        evc.solve_activations_semi(A[0], X, H0)
    with pytest.raises(ValueError, match="dtype"):
        evc.solve_activations_semi(A, X, H0, dtype="f16")
    with pytest.raises(ValueError, match="1056 bins"):
        evc.solve_activations_semi(np.ones((1057, 7)), np.ones((1057, 3)), H0)
    with pytest.raises(ValueError, match="16384 exemplars"):
        evc.solve_activations_semi(np.ones((16385, 2)), np.ones((3, 2)), np.ones((3, 16385)), layout="frame_major")
    with pytest.raises(ValueError, match="stop_rule"):
        evc.solve_activations_semi(A, X, H0, stop_rule="sklearn")
    with pytest.raises(ValueError, match="init"):
        evc.solve_activations_semi(A, X, H0, init="sklearn")
    with pytest.raises(ValueError, match="number of exemplars"):
        evc.convert_semi(A, np.ones((9, 6)), X, H0)
    import torch
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="needs H0"):
            evc.solve_activations_semi(A, X)
        with pytest.raises(ValueError, match="H0 has shape"):
            evc.solve_activations_semi(A, X, np.ones((3, 7)))
        H = evc.solve_activations_semi(A, X, H0, iters=3)
        assert H.shape == (7, 3) and not H.any()                       # A^T X < 0 and A^T A > 0: H1 is exactly 0
    else:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            evc.solve_activations_semi(A, X, H0, iters=3)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            evc.convert_semi(A, np.ones((9, 7)), X, H0)


# ---- the host pieces of the driver (csrc/evc_semi_plan.h) in a program of their own, plainly and under the sanitizers ----
SRC = os.path.join(ROOT, "tests", "semi_host_main.hip")
PKG = os.path.join(ROOT, "exemplars_vc_amd")


def _program_lines(tmp, sanitize):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = os.path.join(tmp, "semi_host_main" + ("_san" if sanitize else ""))
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
    tmp = str(tmp_path_factory.mktemp("semi_host"))
    return _program_lines(tmp, False), tmp


def test_host_carving_and_argument_checks(program):
    _lib, L = lib()
    carves = [ln.split() for ln in program[0] if ln.startswith("carve ")]
    assert len(carves) == 12 and not any("BAD" in ln for ln in program[0])
    for c in carves:
        M, N, T, n_utt, esize, shift = (int(v) for v in c[1:6] + [c[7]])
        offs = [int(v) for v in c[9:19]]
        assert offs[0] == (256 - shift) % 256 and offs == sorted(offs) and all((o + shift) % 256 == 0 for o in offs)
        query = int(L.evc_semi_workspace_bytes(M, N, T, n_utt, _lib.F64 if esize == 8 else _lib.F32))
        assert int(c[-1]) == query and int(c[-3]) <= query
    args = {ln.split()[1]: int(ln.split()[2]) for ln in program[0] if ln.startswith("args ")}
    want = dict(ok=0, ok_exact=0, short_by_one=-2, f32_ws=-2, ok_utts=0, bad_utts=-1, no_frames_no_x=0, frames_no_x=-1,
                struct_bytes=-1, iters_neg=-1, iters_0=0, slots_4097=0, slots_4098=-1, check_every_neg=-1, reserved=-1,
                init_sklearn=-1, init_const=0, stop_sklearn=-1, stop_none=0, tol_neg=-1, tol_0=0, eps_neg=-1, eps_0=0, eps_nan=-1,
                eps_inf=-1, init_value_inf=-1, dtype=-1, layout=-1, M_1056=0, M_1057=-3, M_1057_small_ws=-3, N_16384=0,
                N_16384_small_ws=-2, N_16385=-3, N_16385_small_ws=-3, nan_before_limits=-1, reserved_before_limits=-1)
    assert args == want
    # the wavefronts per workgroup: 8 from 512 workgroups of 128 rows x 64 frames on, else 4
    waves = {(int(ln.split()[1]), int(ln.split()[2])): int(ln.split()[3]) for ln in program[0] if ln.startswith("waves ")}
    for (N, T), W in waves.items():
        fb, rows = -(-T // 64), -(-N // 128) * 128
        assert W == (8 if fb * (rows // 128) >= 512 else 4), (N, T)
    assert [waves[k] for k in ((257, 5440), (257, 10880), (257, 10881))] == [4, 4, 8]
    assert waves[(1024, 688)] == 4 and waves[(4096, 688)] == 4 and waves[(4096, 1024)] == 8 and waves[(25, 0)] == 4
    assert waves[(16384, 128)] == 4 and waves[(16384, 256)] == 8 and waves[(128, 2000000000)] == 8 and waves[(1, 1)] == 4


def test_the_host_program_runs_clean_under_the_sanitizers(program):
    """a stand-alone program: address + undefined-behaviour sanitizers on the host code, nothing preloaded anywhere"""
    assert _program_lines(program[1], True) == program[0]
