"""Convolutive dictionary learning (evc_deconv_learn), host side: the numpy restatement against recorded scikit-learn results,
the C ABI's declarations and struct mirror, the frame ranges, the Python wrappers' limits and the stand-alone host program
(csrc/evc_deconv_learn_plan.h), plainly and under the sanitizers.  No GPU needed."""
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
import deconv_learn_restatement as dlr  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
SK = ["dictmu_sk_m50_r24_t150_k40", "dictkl_sk_m50_r24_t150_k40", "dictmu_sk_m25_r130_t70_k40", "dictkl_sk_m201_r20_t100_k40",
      "dictmu_sk_m50_r24_t150_zeros", "dictkl_sk_m50_r24_t150_zeros", "dictmu_sk_m50_r24_t150_tol", "dictkl_sk_m50_r24_t150_tol"]
OFFS = [0, 37, 37, 40, 90]


def lib():
    from exemplars_vc_amd import _lib
    return _lib, _lib.lib()


def close(got, want, rtol, what):
    nz = want != 0
    r = float(np.max(np.abs(got[nz] - want[nz]) / np.abs(want[nz])))
    print(f"{what}: max relative error {r:.3e}")
    assert r <= rtol and not got[~nz].any(), (what, r)


# ---- the restatement ----
@pytest.mark.parametrize("name", SK)
def test_restatement_with_one_tap_reproduces_sklearn(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    tol = float(d["tol"])
    W, H, n_iter, _ = dlr.learn(d["W0"][None], d["X"], d["H0"], "kl" if name.startswith("dictkl") else "frobenius",
                                int(d["max_iter"]), check_every=10 if tol > 0 else 0, tol=tol)
    assert n_iter == int(d["n_iter"]) and (tol == 0 or n_iter == 60)
    close(W[0], d["W"], 1e-9, "W")
    close(H, d["H"], 1e-9, "H")


@pytest.mark.parametrize("loss", ["fro", "kl"])
def test_restatement_reproduces_the_dictionary_half_of_sklearn(loss):
    d = np.load(os.path.join(GOLDEN, f"deconvlearn_dicthalf_{loss}_m25_r12_t90_l4.npz"))
    assert d["offsets"].tolist() == OFFS and d["W0"].shape == (4, 25, 12)
    W = dlr.dict_step(d["W0"], d["X"], d["H0"], str(d["loss"]), OFFS)
    close(W, d["W"], 1e-12, "W after one dictionary half")


@pytest.mark.parametrize("loss", ["frobenius", "kl"])
@pytest.mark.parametrize("update", ["both", "dict"])
def test_restatement_error_never_rises(loss, update):
    X, W0, H0 = dlr.problem(25, 12, 90, 4, OFFS)
    W, H, n_iter, tr = dlr.learn(W0, X, H0, loss, 60, OFFS, check_every=1, update=update)
    assert n_iter == 60 and np.isfinite(tr).all() and np.all(np.diff(tr) <= 0)
    if update == "dict":
        assert np.array_equal(H, H0)


def test_restatement_shift_respects_the_utterances():
    H = np.arange(1.0, 1 + 2 * 9).reshape(2, 9)
    Hs = dlr.shifted(H, 2, [0, 4, 4, 5, 9])
    assert np.array_equal(Hs[0], [0, 0, 1, 2, 0, 0, 0, 6, 7])
    assert np.array_equal(dlr.shifted(H, 0, [0, 4, 4, 5, 9]), H) and np.array_equal(dlr.shifted(H, 3), np.c_[np.zeros((2, 3)), H[:, :6]])
    # the activation half is deconv_restatement's, the model agrees with its forward
    import deconv_restatement as dr
    W = np.random.default_rng(1).random((3, 5, 2))
    assert np.allclose(dlr.model(W, H), dr.forward(W, H), rtol=1e-15)


# ---- the C ABI ----
def test_symbols_declared_and_exported():
    _lib, L = lib()
    hdr = open(os.path.join(ROOT, "include", "evc.h")).read()
    declared = set(re.findall(r"\b(evc_[a-z_0-9]+)\s*\(", hdr))
    for sym in ("evc_deconv_learn_workspace_bytes", "evc_deconv_learn_splits", "evc_deconv_learn"):
        assert sym in declared and sym in _lib.SYMBOLS and hasattr(L, sym)
    assert "evc_deconv_learn " in hdr[:hdr.index("#ifndef EVC_H")]
    assert re.search(r"EVC_DCL_BOTH = 0, EVC_DCL_DICT_ONLY = 1", hdr) and (_lib.DCL_BOTH, _lib.DCL_DICT_ONLY) == (0, 1)


def test_opts_mirror_matches_header():
    _lib, _ = lib()
    hdr = open(os.path.join(ROOT, "include", "evc.h")).read()
    body = hdr[hdr.index("typedef struct evc_deconv_learn_opts {"):hdr.index("} evc_deconv_learn_opts;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for grp in re.findall(r"\b(?:int|double|void\*)\s+([a-zA-Z_0-9, ]+);", body)
             for n in grp.replace(" ", "").split(",")]
    assert names == [f[0] for f in _lib.DeconvLearnOpts._fields_]
    assert names == ["struct_bytes", "dtype", "layout", "loss", "taps", "iters", "check_every", "update", "reserved", "tol",
                     "l1_h", "l2_h", "ev_loop_start", "ev_loop_stop"]
    assert C.sizeof(_lib.DeconvLearnOpts) == 10 * 4 + 3 * 8 + 2 * 8          # nine ints and their padding
    assert C.sizeof(_lib.DeconvOpts) == 10 * 4 + 4 * 8 + 2 * 8               # the existing struct did not move


def _opts(_lib, **kw):
    o = _lib.DeconvLearnOpts()
    o.struct_bytes = C.sizeof(_lib.DeconvLearnOpts)
    o.dtype, o.layout, o.loss, o.taps, o.iters = _lib.F64, _lib.BIN_MAJOR, _lib.LOSS_FROBENIUS, 4, 100
    o.check_every, o.update, o.tol = 10, _lib.DCL_BOTH, 1e-4
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_status_codes_and_their_order_through_the_library():
    _lib, L = lib()
    one = C.c_void_p(256)              # never dereferenced: every case fails validation first

    def call(o, M=25, R=17, T=70, ws=1 << 40, tap_stride=None, X=one, W=one, H=one, wsp=one):
        return L.evc_deconv_learn(X, T, W, R, M * R if tap_stride is None else tap_stride, H, T, M, R, T, None, 1,
                                  None if o is None else C.byref(o), wsp, ws, None, None, None)
    assert call(None) == -1 and call(_opts(_lib, struct_bytes=4)) == -1
    for p in ("X", "W", "H", "wsp"):
        assert call(_opts(_lib), **{p: None}) == -1
    assert call(_opts(_lib, tol=float("nan")), M=257, ws=16) == -1          # every -1 before the limits
    assert call(_opts(_lib), M=257) == -3 and call(_opts(_lib), M=257, ws=16) == -3
    assert call(_opts(_lib, update=_lib.DCL_DICT_ONLY), M=257, ws=16) == -2
    assert call(_opts(_lib, update=_lib.DCL_DICT_ONLY), M=1056, ws=16) == -2
    assert call(_opts(_lib, update=_lib.DCL_DICT_ONLY), M=1057) == -3 and call(_opts(_lib), M=1057) == -3
    assert call(_opts(_lib, taps=17)) == -3 and call(_opts(_lib), R=4097) == -3
    assert call(_opts(_lib), tap_stride=25 * 17 - 1) == -1 and call(_opts(_lib), tap_stride=0) == -1
    assert call(_opts(_lib, taps=17), tap_stride=3, ws=16) == -1           # overlap is an argument error: before -3
    assert call(_opts(_lib, taps=1), tap_stride=0, ws=16) == -2
    assert call(_opts(_lib), ws=16) == -2
    assert call(_opts(_lib), ws=int(L.evc_deconv_learn_workspace_bytes(25, 17, 70, 1, 4, 0, _lib.F64)) - 1) == -2
    assert call(_opts(_lib, reserved=1)) == -1 and call(_opts(_lib, reserved=65 << 8)) == -1
    assert call(_opts(_lib, reserved=64 << 8), ws=16) == -2
    assert call(_opts(_lib, update=2)) == -1 and call(_opts(_lib, loss=2)) == -1 and call(_opts(_lib, iters=-1)) == -1
    assert call(_opts(_lib, iters=4097, check_every=1)) == -1 and call(_opts(_lib, iters=4096, check_every=1), ws=16) == -2
    assert call(_opts(_lib), T=0) == -1


def test_workspace_query():
    _lib, L = lib()
    q = L.evc_deconv_learn_workspace_bytes
    B, D = _lib.DCL_BOTH, _lib.DCL_DICT_ONLY
    assert q(256, 64, 100, 1, 16, B, 0) > 0 and q(257, 64, 100, 1, 4, B, 0) == 0 and q(257, 64, 100, 1, 4, D, 0) > 0
    assert q(1056, 64, 100, 1, 4, D, 0) > 0 and q(1057, 64, 100, 1, 4, D, 0) == 0
    assert q(25, 4096, 100, 1, 4, B, 0) > 0 and q(25, 4097, 100, 1, 4, B, 0) == 0 and q(25, 64, 100, 1, 17, B, 0) == 0
    for bad in ((0, 64, 100, 1, 4, B, 0), (25, 0, 100, 1, 4, B, 0), (25, 64, 0, 1, 4, B, 0), (25, 64, 100, 0, 4, B, 0),
                (25, 64, 100, 1, 0, B, 0), (25, 64, 100, 1, 4, 2, 0), (25, 64, 100, 1, 4, B, 9)):
        assert q(*bad) == 0, bad
    assert q(25, 64, 688, 1, 1, B, 0) < q(25, 64, 688, 1, 4, B, 0) < q(25, 64, 6880, 1, 4, B, 0) < q(25, 64, 6880, 10, 4, B, 0)
    assert q(201, 64, 688, 1, 4, B, _lib.F32) < q(201, 64, 688, 1, 4, B, _lib.F64)
    assert q(25, 64, 688, 1, 4, D, 0) < q(25, 64, 688, 1, 4, B, 0)          # no packed taps without the activation half
    assert q(1056, 4096, 4096, 1, 16, D, 0) < (3 << 28)                     # the slabs are capped


CAP = 128 << 20


def test_splits_depend_on_the_sizes_only_and_keep_the_slabs_under_the_cap():
    _lib, L = lib()
    s = L.evc_deconv_learn_splits
    assert s(0, 64, 100, 1, 4) == 0 and s(25, 64, 100, 1, 17) == 0 and s(1057, 64, 100, 1, 4) == 0 and s(25, 4097, 100, 1, 4) == 0
    seen = set()
    for M in (1, 25, 50, 201, 256, 513, 1056):
        for R in (1, 24, 512, 4096):
            for T in (1, 90, 4096, 65536, 1 << 22):
                for taps in (1, 4, 16):
                    S = s(M, R, T, 1, taps)
                    assert 1 <= S <= 64 and S == s(M, R, T, 96, taps) == s(M, R, T, 1, taps), (M, R, T, taps)
                    pair = 2 * ((-(-M // 16) + 3) // 4 * 4) * 16 * (-(-R // 128) * 128) * 8
                    assert S == 1 or S * taps * pair <= CAP, (M, R, T, taps, S)
                    seen.add(S)
    assert 1 in seen and 64 in seen and len(seen) > 4
    assert s(50, 512, 65536, 96, 1) > s(50, 512, 65536, 96, 4) >= s(50, 512, 65536, 96, 16) >= 1
    assert s(1056, 4096, 1 << 22, 1, 16) == 1 and s(1056, 4096, 1 << 22, 1, 1) == 1       # one pair there is 71 303 168 bytes


# ---- the Python wrappers ----
def test_python_surface_and_limits():
    import exemplars_vc_amd as evc
    import torch
    for name in ("learn_dictionary_deconv", "compact_dictionary_deconv"):
        assert name in evc.__all__ and callable(getattr(evc, name))
    sig = inspect.signature(evc.learn_dictionary_deconv).parameters
    assert list(sig)[:3] == ["X", "W0_taps", "H0"]
    for k in ("loss", "layout", "iters", "check_every", "tol", "l1_h", "l2_h", "update", "utt_offsets", "dtype", "device", "info",
              "out_w", "out_h"):
        assert sig[k].kind is inspect.Parameter.KEYWORD_ONLY, k
    assert list(inspect.signature(evc.compact_dictionary_deconv).parameters)[:5] == ["A_frames", "B_frames", "seg_offsets", "R",
                                                                                     "taps"]
    assert inspect.signature(evc.compat.make_dict.aligned_dictionary).parameters["compact"].default is None
    X, H = np.ones((257, 9)), np.ones((3, 9))
    with pytest.raises(ValueError, match="256 bins"):
        evc.learn_dictionary_deconv(X, np.ones((2, 257, 3)), H, layout="bin_major", iters=1)
    with pytest.raises(ValueError, match="256 bins"):
        evc.learn_dictionary_deconv(X.T, np.ones((2, 3, 257)), H.T, layout="frame_major", iters=1)
    with pytest.raises(ValueError, match="1056 bins"):
        evc.learn_dictionary_deconv(np.ones((1057, 9)), np.ones((2, 1057, 3)), H, layout="bin_major", iters=1, update="dict")
    with pytest.raises(ValueError, match="16 taps"):
        evc.learn_dictionary_deconv(np.ones((5, 9)), np.ones((17, 5, 3)), H, layout="bin_major", iters=1)
    with pytest.raises(ValueError, match="4096 components"):
        evc.learn_dictionary_deconv(np.ones((5, 9)), np.ones((2, 5, 4097)), np.ones((4097, 9)), layout="bin_major", iters=1)
    overlapping = torch.ones(5 * 3 + 10).as_strided((3, 5, 3), (5, 3, 1))      # taps 5 elements apart, 15 long
    with pytest.raises(ValueError, match="overlap"):
        evc.learn_dictionary_deconv(np.ones((5, 9)), None, H, layout="bin_major", iters=1, out_w=overlapping)
    with pytest.raises(ValueError, match="3-D"):
        evc.learn_dictionary_deconv(np.ones((5, 9)), np.ones((5, 3)), H, layout="bin_major", iters=1)
    with pytest.raises(ValueError, match="update"):
        evc.learn_dictionary_deconv(np.ones((5, 9)), np.ones((2, 5, 3)), H, layout="bin_major", iters=1, update="h")
    with pytest.raises(ValueError, match="16 taps"):
        evc.compact_dictionary_deconv(np.ones((5, 9)), np.ones((5, 9)), [0, 9], 2, 17)
    with pytest.raises(ValueError, match="1056 target bins"):
        evc.compact_dictionary_deconv(np.ones((5, 9)), np.ones((1057, 9)), [0, 9], 2, 2)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            evc.learn_dictionary_deconv(np.ones((5, 9)), np.ones((2, 5, 3)), H, layout="bin_major", iters=1)


# ---- the host pieces of the driver (csrc/evc_deconv_learn_plan.h) in a program of their own, plainly and under the sanitizers
SRC = os.path.join(ROOT, "tests", "deconv_learn_host_main.hip")
PKG = os.path.join(ROOT, "exemplars_vc_amd")


def _program_lines(tmp, sanitize):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = os.path.join(tmp, "deconv_learn_host_main" + ("_san" if sanitize else ""))
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
    tmp = str(tmp_path_factory.mktemp("deconv_learn_host"))
    return _program_lines(tmp, False), tmp


def test_host_carving_and_argument_checks(program):
    _lib, L = lib()
    carves = [ln.split() for ln in program[0] if ln.startswith("carve ")]
    assert len(carves) == 12 and not any("BAD" in ln for ln in program[0])
    for c in carves:
        M, R, T, n_utt, taps, update, esize, shift = (int(v) for v in c[1:8] + [c[9]])
        offs = [int(v) for v in c[11:23]]
        assert offs[0] == (256 - shift) % 256 and offs == sorted(offs) and all((o + shift) % 256 == 0 for o in offs)
        query = int(L.evc_deconv_learn_workspace_bytes(M, R, T, n_utt, taps, update, _lib.F64 if esize == 8 else _lib.F32))
        assert int(c[-1]) == query and int(c[-3]) <= query
    args = {ln.split()[1]: int(ln.split()[2]) for ln in program[0] if ln.startswith("args ")}
    want = dict(ok=0, ok_exact=0, short_by_one=-2, ok_utts=0, bad_utts=-1, no_utts=-1, no_h=-1, no_frames=-1, ok_frame_major=0,
                overlap_frame_major=-1, overlap=-1, overlap_0=-1, tap_stride_neg=-1, one_tap_any_stride=0, struct_bytes=-1,
                taps_0=-1, taps_16=0, taps_17=-3, taps_17_small_ws=-3, loss=-1, frobenius=0, update=-1, iters_neg=-1, iters_0=0,
                check_every_neg=-1, slots_4097=0, slots_4098=-1, reserved_bit0=-1, reserved_bit16=-1, forced_7=0, forced_64=0,
                forced_65=-1, tol_neg=-1, tol_0=0, l1_neg=-1, l2_nan=-1, dtype=-1, layout=-1, M_256=0, M_257_both=-3,
                M_257_both_small_ws=-3, M_257_dict_small_ws=-2, M_1056_dict=0, M_1057_dict=-3, M_1057_both=-3, R_4096=0,
                R_4097=-3, R_4097_small_ws=-3, nan_before_limits=-1, taps_0_before_limits=-1, overlap_before_limits=-1)
    assert args == want
    # the query is 0 exactly where these sizes, update mode and type can give neither 0 nor -2
    query = {ln.split()[1]: int(ln.split()[2]) for ln in program[0] if ln.startswith("query ")}
    by_sizes = ("ok", "ok_utts", "no_utts", "no_frames", "taps_0", "taps_16", "taps_17", "update", "dtype", "M_256", "M_257_both",
                "M_257_dict_small_ws", "M_1056_dict", "M_1057_dict", "M_1057_both", "R_4096", "R_4097")
    for name in by_sizes:
        assert query[name] == (1 if args[name] in (0, -2) else 0), name
    plans = [[int(v) for v in ln.split()[1:]] for ln in program[0] if ln.startswith("plan ")]
    assert len(plans) == 21
    for M, R, T, taps, forced, S, chunk, nbytes in plans:
        assert 1 <= S <= 64 and 1 <= chunk <= taps and nbytes <= CAP, (M, R, T, taps, forced)
        if forced == 0:
            assert S == L.evc_deconv_learn_splits(M, R, T, 1, taps)
        elif (M, R) == (25, 12):
            assert S == forced and chunk == taps
    assert [p[5:7] for p in plans if p[:2] == [1056, 4096] and p[3] == 16] == [[1, 1], [1, 1]]


def test_the_host_program_runs_clean_under_the_sanitizers(program):
    """a stand-alone program: address + undefined-behaviour sanitizers on the host code, nothing preloaded anywhere"""
    assert _program_lines(program[1], True) == program[0]
