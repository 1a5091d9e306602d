"""The device k-means (evc_kmeans), host side: the C ABI's declarations, struct mirror, status codes and their order, the two
queries, the numpy restatement against recorded pymf results, the Python surface's errors and the stand-alone host program
(csrc/evc_kmeans_plan.h), plainly and under the sanitizers.  No GPU needed."""
import ctypes as C
import glob
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
import kmeans_restatement as kr  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ["kmeans_doctest", "kmeans_doctest_vq", "kmeans_m25_t70_r8", "kmeans_m40_t257_r17", "kmeans_m1_t64_r5",
            "kmeans_m513_t200_r17", "kmeans_vq_m25_t70_r8", "kmeans_dup_m25_t70_r8"]


def lib():
    from exemplars_vc_amd import _lib
    return _lib, _lib.lib()


def nrel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), np.finfo(float).tiny))


def test_every_recorded_fixture_is_listed():
    names = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN, "kmeans_*.npz")))
    assert names == sorted(FIXTURES)
    for name in FIXTURES:
        d = np.load(os.path.join(GOLDEN, name + ".npz"))
        assert sorted(d.files) == sorted(["data", "W0", "niter", "compute_w", "seed", "W", "assigned", "ferr", "n_iter"])


def test_symbols_declared_and_exported():
    _lib, L = lib()
    hdr = open(os.path.join(ROOT, "include", "evc.h")).read()
    declared = set(re.findall(r"\b(evc_[a-z_0-9]+)\s*\(", hdr))
    for sym in ("evc_kmeans_workspace_bytes", "evc_kmeans_splits", "evc_kmeans"):
        assert sym in declared and sym in _lib.SYMBOLS and hasattr(L, sym)
    assert "evc_kmeans " in hdr[:hdr.index("#ifndef EVC_H")]
    assert (_lib.KM_BOTH, _lib.KM_ASSIGN_ONLY) == (0, 1) and "EVC_KM_BOTH = 0, EVC_KM_ASSIGN_ONLY = 1" in hdr
    assert (_lib.KM_STOP_NONE, _lib.KM_STOP_PYMF, _lib.KM_STOP_LABELS) == (0, 1, 2)
    assert "EVC_KM_STOP_NONE = 0, EVC_KM_STOP_PYMF = 1, EVC_KM_STOP_LABELS = 2" in hdr
    assert (_lib.KMEANS_MAX_M, _lib.KMEANS_MAX_T, _lib.KMEANS_MAX_R) == (1056, 1 << 20, 4096)


def test_opts_mirror_matches_header():
    _lib, _ = lib()
    hdr = open(os.path.join(ROOT, "include", "evc.h")).read()
    body = hdr[hdr.index("typedef struct evc_kmeans_opts {"):hdr.index("} evc_kmeans_opts;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for grp in re.findall(r"\b(?:int|double|void\*)\s+([a-zA-Z_0-9, ]+);", body)
             for n in grp.replace(" ", "").split(",")]
    assert names == [f[0] for f in _lib.KmeansOpts._fields_]
    assert names == ["struct_bytes", "dtype", "layout", "iters", "update", "stop_rule", "reserved", "tol", "ev_loop_start",
                     "ev_loop_stop"]
    assert C.sizeof(_lib.KmeansOpts) == 8 * 4 + 8 + 2 * 8 and _lib.KmeansOpts.tol.offset == 32
    # the existing structs did not move
    assert C.sizeof(_lib.ConvexOpts) == 8 * 4 + 2 * 8 + 2 * 8 and C.sizeof(_lib.SemiOpts) == 8 * 4 + 3 * 8 + 2 * 8


def _opts(_lib, **kw):
    o = _lib.KmeansOpts()
    o.struct_bytes = C.sizeof(_lib.KmeansOpts)
    o.dtype, o.layout, o.iters = _lib.F64, _lib.FRAME_MAJOR, 10
    o.update, o.stop_rule, o.tol = _lib.KM_BOTH, _lib.KM_STOP_PYMF, 2.22e-16
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_status_codes_and_their_order():
    _lib, L = lib()
    one = C.c_void_p(8)              # never dereferenced: every case fails validation first

    def call(o, M=25, R=17, T=70, ldx=25, ldw=25, ws=16, X=one, W=one, wsp=one):
        return L.evc_kmeans(X, ldx, W, ldw, None, None, M, R, T, None if o is None else C.byref(o), wsp, ws, None, None, None)
    # every valid call below is handed a 16-byte workspace: it gets as far as -2 and touches no device
    assert call(_opts(_lib)) == -2
    bad = _opts(_lib)
    bad.struct_bytes = 4
    assert call(bad) == -1 and call(None) == -1
    assert call(_opts(_lib), M=0) == -1 and call(_opts(_lib), R=0) == -1 and call(_opts(_lib), T=0) == -1
    assert call(_opts(_lib), ldx=24) == -1 and call(_opts(_lib), ldw=24) == -1
    bm = dict(ldx=70, ldw=17)
    assert call(_opts(_lib, layout=_lib.BIN_MAJOR), **bm) == -2
    assert call(_opts(_lib, layout=_lib.BIN_MAJOR), ldx=69, ldw=17) == -1 and call(_opts(_lib, layout=_lib.BIN_MAJOR), ldx=70, ldw=16) == -1
    for p in ("X", "W", "wsp"):
        assert call(_opts(_lib), **{p: None}) == -1
    assert call(_opts(_lib, tol=-1e-12)) == -1 and call(_opts(_lib, tol=float("nan"))) == -1 and call(_opts(_lib, tol=0.0)) == -2
    assert call(_opts(_lib, update=2)) == -1 and call(_opts(_lib, update=-1)) == -1 and call(_opts(_lib, update=_lib.KM_ASSIGN_ONLY)) == -2
    assert call(_opts(_lib, stop_rule=3)) == -1 and call(_opts(_lib, stop_rule=_lib.KM_STOP_LABELS)) == -2
    assert call(_opts(_lib, dtype=7)) == -1 and call(_opts(_lib, layout=5)) == -1 and call(_opts(_lib, dtype=_lib.F32)) == -2
    assert call(_opts(_lib, reserved=1)) == -2 and call(_opts(_lib, reserved=2)) == -1 and call(_opts(_lib, reserved=1 << 16)) == -1
    assert call(_opts(_lib, reserved=17 << 8)) == -1 and call(_opts(_lib, reserved=(16 << 8) | 1)) == -2
    assert call(_opts(_lib, iters=-1)) == -1 and call(_opts(_lib, iters=0)) == -2
    assert call(_opts(_lib, iters=4096)) == -2 and call(_opts(_lib, iters=4097)) == -1          # more than 4097 error slots
    assert call(_opts(_lib), ws=int(L.evc_kmeans_workspace_bytes(25, 17, 70, _lib.F64)) - 1) == -2
    # beyond the limits: -3, after every -1 and before -2, even with a tiny workspace
    big = 1 << 40
    assert call(_opts(_lib), M=1057, ldx=1057, ldw=1057) == -3 and call(_opts(_lib), M=1057, ldx=1057, ldw=1057, ws=big) == -3
    assert call(_opts(_lib), T=(1 << 20) + 1) == -3 and call(_opts(_lib), T=(1 << 20) + 1, ws=big) == -3
    assert call(_opts(_lib), R=4097, T=8192) == -3 and call(_opts(_lib), R=4096, T=8192) == -2
    assert call(_opts(_lib), R=71) == -3 and call(_opts(_lib), R=70) == -2
    assert call(_opts(_lib, update=_lib.KM_ASSIGN_ONLY), R=71) == -2              # the assignment alone: any codebook
    assert call(_opts(_lib, update=_lib.KM_ASSIGN_ONLY), R=4097) == -3
    assert call(_opts(_lib), M=1056, ldx=1056, ldw=1056) == -2 and call(_opts(_lib), T=1 << 20) == -2
    assert call(_opts(_lib, tol=float("nan")), M=1057, ldx=1057, ldw=1057) == -1
    assert call(_opts(_lib, reserved=4), T=(1 << 20) + 1) == -1
    assert call(_opts(_lib), M=1057, ldx=1057, ldw=1057, X=None) == -1


def test_workspace_query_and_splits():
    _lib, L = lib()
    q, sp = L.evc_kmeans_workspace_bytes, L.evc_kmeans_splits
    assert q(1057, 8, 100, 0) == 0 and q(25, 8, (1 << 20) + 1, 0) == 0 and q(25, 4097, 8192, 0) == 0
    assert q(0, 8, 100, 0) == 0 and q(25, 0, 100, 0) == 0 and q(25, 8, 0, 0) == 0 and q(25, 8, 100, 9) == 0
    assert q(1056, 8, 100, 0) > 0 and q(25, 100, 100, 1) > 0 and q(25, 4096, 1 << 20, 0) > 0
    assert q(25, 8, 70, 0) < q(25, 8, 300, 0) < q(25, 33, 300, 0) and q(25, 8, 70, 1) < q(25, 8, 70, 0)
    for M, R, T, dt, es in ((25, 8, 70, _lib.F64, 8), (50, 256, 4096, _lib.F32, 4), (40, 17, 257, _lib.F64, 8), (50, 1024, 16384, _lib.F64, 8)):
        S = int(sp(R, T))
        own = (3 * T + R) * es + (S * T * (2 * es + 4) if S > 1 else 0) + 4 * T * 4 + R * 4 + T * 8 + 4097 * 8 + 12
        assert own <= int(q(M, R, T, dt)) <= own + 18 * 256
    assert sp(0, 100) == 0 and sp(8, 0) == 0 and sp(4097, 8192) == 0 and sp(8, (1 << 20) + 1) == 0
    # 256 workgroups from ceil(T / 64) sample tiles, never more ranges than centre tiles of 32, at most 16
    assert sp(64, 4096) == 2 and sp(256, 4096) == 4 and sp(1024, 4096) == 4 and sp(1024, 16384) == 1 and sp(1024, 1024) == 16
    assert sp(8, 70) == 1 and sp(33, 300) == 2 and sp(300, 300) == 10 and sp(4096, 1 << 20) == 1
    # the existing query did not move
    assert int(L.evc_beta_workspace_bytes(25, 24, 70, 1, _lib.F64)) == 76800


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_reproduces_pymf(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    niter, (M, T) = int(d["niter"]), d["data"].shape
    W, labels, counts, n_iter, tr, margin = kr.run(d["data"], d["W0"], niter, update="both" if bool(d["compute_w"]) else "assign",
                                                   stop="pymf", tol=kr.PYMF_TOL)
    ferr = kr.pymf_ferr(tr, n_iter, niter, T)
    print(name, "W", nrel(W, d["W"]), "ferr", nrel(ferr, d["ferr"]) if len(ferr) == len(d["ferr"]) else None, "margin", margin)
    assert margin >= kr.margin_bound(M, np.float64)            # the condition of a comparison of labels (kmeans_restatement.py)
    assert n_iter == int(d["n_iter"]) and len(ferr) == len(d["ferr"])
    assert np.array_equal(labels, d["assigned"]) and counts.sum() == T and np.array_equal(counts, np.bincount(d["assigned"], minlength=len(counts)))
    assert nrel(W, d["W"]) <= 1e-12 and nrel(ferr, d["ferr"]) <= 1e-12
    if not bool(d["compute_w"]):
        assert np.array_equal(W, d["W0"])
    empty = counts == 0
    assert np.array_equal(W[:, empty], d["W"][:, empty])              # an empty cluster keeps its centre, bit for bit
    if name == "kmeans_m25_t70_r8":
        assert empty.sum() == 1
    if name == "kmeans_dup_m25_t70_r8":
        lab0 = kr.assign(d["data"], d["W0"])[0]
        assert not np.isin(lab0, [2, 4, 5, 7]).any()               # of identical start centres the lowest index takes all


def test_restatement_stops():
    X = kr.problem(25, 300, 9, 31)
    W0 = X[:, kr.spread_start(300, 9)]
    W, labels, counts, n_lab, tr, _ = kr.run(X, W0, 50, stop="labels")
    assert n_lab < 50 and np.isnan(tr[n_lab + 1:]).all() and not np.isnan(tr[:n_lab + 1]).any()
    _, lab2, _, n_none, tr2, _ = kr.run(X, W0, n_lab + 3, stop="none")
    # unchanged labels leave the same centres, and those the same bits of the error: what pymf's stop waits for, a round later
    assert n_none == n_lab + 3 and np.array_equal(lab2, labels) and np.all(tr2[n_lab:] == tr[n_lab]) and tr[n_lab] < tr[n_lab - 1]
    _, lab3, _, n_pymf, tr3, _ = kr.run(X, W0, 50, stop="pymf")
    assert n_pymf == max(n_lab + 1, 3) and np.array_equal(lab3, labels)
    assert np.all(np.diff(tr[:n_lab + 1]) <= 0)                         # the error never rises
    _, lab4, _, n4, tr4, _ = kr.run(X, W0, 4, update="assign", stop="pymf")
    assert n4 == 3 and tr4[0] == tr4[3] and np.array_equal(lab4, kr.assign(X, W0)[0])


def test_restatement_float32_labels_need_the_margin():
    d = np.load(os.path.join(GOLDEN, "kmeans_m40_t257_r17.npz"))
    W, labels, _, n_iter, _, margin = kr.run(d["data"], d["W0"], 30)
    W32, l32, _, n32, tr32, m32 = kr.run(d["data"], d["W0"], 30, dtype=np.float32)
    assert W32.dtype == np.float32 and tr32.dtype == np.float64
    assert min(margin, m32) >= kr.margin_bound(40, np.float32)
    assert np.array_equal(l32, labels) and n32 == n_iter and 1e-9 < nrel(W32, W) < 1e-5


def test_python_surface():
    import exemplars_vc_amd as evc
    from exemplars_vc_amd.compat import pymf
    for name in ("kmeans", "vq", "compact_dictionary_kmeans"):
        assert name in evc.__all__ and callable(getattr(evc, name))
    sig = inspect.signature(evc.kmeans).parameters
    assert list(sig)[:2] == ["X", "W0"] and sig["iters"].default == 10 and sig["stop"].default == "pymf"
    assert sig["update"].default == "both" and sig["tol"].default is None and sig["splits"].default == 0
    for k in ("layout", "iters", "stop", "tol", "update", "dtype", "device", "info", "splits", "loop_events"):
        assert sig[k].kind is inspect.Parameter.KEYWORD_ONLY, k
    assert list(inspect.signature(evc.vq).parameters)[:2] == ["W", "X"]
    csig = inspect.signature(evc.compact_dictionary_kmeans).parameters
    assert list(csig)[:3] == ["A", "B", "R"] and csig["iters"].default == 10 and csig["stop"].default == "labels"
    assert csig["init"].default == "spread" and csig["layout"].default == "bin_major"
    xsig = inspect.signature(evc.compact_dictionary_convex).parameters
    assert xsig["assign"].default is None and xsig["kmeans_iters"].default == 10
    fsig = inspect.signature(pymf.Kmeans.factorize).parameters
    assert set(fsig) == {"self", "niter", "compute_w", "compute_h", "compute_err", "show_progress"}
    assert fsig["niter"].default == 100 and fsig["compute_w"].default is True               # base.py:208-209
    assert inspect.signature(pymf.Kmeans.__init__).parameters["num_bases"].default == 4
    X, W0 = np.ones((5, 7)), np.ones((5, 3))
    with pytest.raises(ValueError, match="do not fit"):
        evc.kmeans(X, np.ones((4, 3)), layout="bin_major")
    with pytest.raises(ValueError, match="2-D"):
        evc.kmeans(X[0], W0, layout="bin_major")
    with pytest.raises(ValueError, match="update"):
        evc.kmeans(X, W0, layout="bin_major", update="w")
    with pytest.raises(ValueError, match="stop"):
        evc.kmeans(X, W0, layout="bin_major", stop="sklearn")
    with pytest.raises(ValueError, match="1056 bins"):
        evc.kmeans(np.ones((1057, 7)), np.ones((1057, 3)), layout="bin_major")
    with pytest.raises(ValueError, match="centres"):
        evc.kmeans(X, np.ones((5, 8)), layout="bin_major")
    with pytest.raises(ValueError, match="dtype"):
        evc.kmeans(X, W0, layout="bin_major", dtype="f16")
    with pytest.raises(ValueError, match="number of exemplars"):
        evc.compact_dictionary_kmeans(np.ones((5, 7)), np.ones((4, 6)), 2)
    with pytest.raises(ValueError, match="R must be"):
        evc.compact_dictionary_kmeans(np.ones((5, 7)), np.ones((4, 7)), 8)
    with pytest.raises(ValueError, match="init"):
        evc.compact_dictionary_kmeans(np.ones((5, 7)), np.ones((4, 7)), 2, init=[0, 7])
    with pytest.raises(ValueError, match="init"):
        evc.compact_dictionary_kmeans(np.ones((5, 7)), np.ones((4, 7)), 2, init="random")
    with pytest.raises(ValueError, match="assign"):
        evc.compact_dictionary_convex(np.ones((5, 7)), np.ones((4, 7)), 2, assign="spread")
    with pytest.raises(ValueError, match="start"):
        pymf.CNMF(np.ones((2, 3)), num_bases=2, start="gpu")
    assert pymf.CNMF(np.ones((2, 3)), num_bases=2)._start == "host"                          # the default did not move
    with pytest.raises(AttributeError, match="set .W"):
        pymf.Kmeans(np.ones((2, 3)), num_bases=2).factorize(niter=1, compute_w=False)
    with pytest.raises(NotImplementedError, match="compute_h"):
        pymf.Kmeans(np.ones((2, 3)), num_bases=2).factorize(niter=1, compute_h=False)
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            evc.kmeans(X, W0, layout="bin_major")
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            evc.vq(W0, X, layout="bin_major")
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            evc.compact_dictionary_kmeans(np.ones((5, 7)), np.ones((4, 7)), 2)


# ---- the host pieces of the driver (csrc/evc_kmeans_plan.h) in a program of their own, plainly and under the sanitizers ----
SRC = os.path.join(ROOT, "tests", "kmeans_host_main.hip")
PKG = os.path.join(ROOT, "exemplars_vc_amd")


def _program_lines(tmp, sanitize):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = os.path.join(tmp, "kmeans_host_main" + ("_san" if sanitize else ""))
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
    lib()                                   # the program links against the built library
    tmp = str(tmp_path_factory.mktemp("kmeans_host"))
    return _program_lines(tmp, False), tmp


def test_host_carving(program):
    _lib, L = lib()
    carves = [ln.split() for ln in program[0] if ln.startswith("carve ")]
    assert len(carves) == 14 and not any("BAD" in ln for ln in program[0])
    for c in carves:
        R, T, S, esize, shift = (int(v) for v in c[1:5] + [c[6]])
        offs = [int(v) for v in c[8:24]]
        # disjoint (the program checked every array's room against its successor), ascending and 256-byte aligned
        assert offs[0] == (256 - shift) % 256 and offs == sorted(offs) and all((o + shift) % 256 == 0 for o in offs)
        if S == int(L.evc_kmeans_splits(R, T)):
            assert int(c[-1]) == int(L.evc_kmeans_workspace_bytes(25, R, T, _lib.F64 if esize == 8 else _lib.F32))
        assert int(c[-3]) <= int(c[-1])


def test_host_argument_checks_in_status_order(program):
    rows = {ln.split()[1]: tuple(int(v) for v in ln.split()[2:]) for ln in program[0] if ln.startswith("args ")}
    status = {k: v[0] for k, v in rows.items()}
    want = dict(ok=0, ok_exact=0, short_by_one=-2, f32_ws=-2, no_x=-1, no_w=-1, no_ws=-1, ldx_short=-1, ldw_short=-1, ld_padded=0,
                bin_major=0, bin_major_ldx_short=-1, bin_major_ldw_short=-1, struct_bytes=-1, iters_neg=-1, iters_0=0,
                slots_4097=0, slots_4098=-1, iters_int_max=-1, redecide=0, reserved_bit1=-1, reserved_high=-1, forced_s7=0,
                forced_s7_plan_ws=-2, forced_s7_own_ws=0, forced_s16_redecide=0, forced_s17=-1, assign_only=0, update_2=-1,
                stop_none=0, stop_labels=0, stop_3=-1, tol_neg=-1, tol_0=0, tol_nan=-1, dtype=-1, layout=-1, M_0=-1, R_0=-1,
                T_0=-1, M_1056=0, M_1057=-3, M_1057_small_ws=-3, T_max=0, T_max_small_ws=-2, T_past=-3, T_past_small_ws=-3,
                R_4096=0, R_4097=-3, R_eq_T=0, R_above_T=-3, R_above_T_small_ws=-3, R_above_T_assign_only=0,
                R_4097_assign_only=-3, nan_before_limits=-1, reserved_before_limits=-1)
    assert status == want
    # the centre ranges a good call leaves: the sizes' own, or what `reserved` forces
    assert rows["ok"][1] == 1 and rows["forced_s7"][1] == 7 and rows["forced_s16_redecide"][1] == 16 and rows["R_4096"][1] == 2


def test_host_queries_at_the_limits(program):
    q = {ln.split()[1]: int(ln.split()[2]) for ln in program[0] if ln.startswith("query ")}
    for name in ("M_1057", "T_past", "R_4097", "zero_M", "zero_R", "zero_T", "dtype"):
        assert q[name] == 0, name
    assert 0 < q["small_f32"] < q["small"] == q["M_1056"] < q["T_max"] < q["R_4096"]        # M takes no workspace
    assert q["T_max"] < 64 << 20


def test_host_splits_depend_on_the_sizes_only_and_fill_the_chip(program):
    _lib, L = lib()
    sp = {(int(v[1]), int(v[2])): int(v[3]) for v in (ln.split() for ln in program[0]) if v[0] == "splits"}
    assert len(sp) > 250
    for (T, R), S in sp.items():
        tiles, ctiles = -(-T // 64), -(-R // 32)
        assert S == max(1, min(-(-256 // tiles), ctiles, 16)) == int(L.evc_kmeans_splits(R, T))
        assert S == 1 or (S - 1) * tiles < 256                       # never more ranges than it takes
        assert S * tiles >= 256 or S == min(ctiles, 16)                # short of 256 workgroups only at a cap
    assert sp[(4096, 64)] == 2 and sp[(4096, 1024)] == 4 and sp[(16384, 1024)] == 1 and sp[(300, 130)] == 5 and sp[(1, 1)] == 1


def test_the_host_program_runs_clean_under_the_sanitizers(program):
    """a stand-alone program: address + undefined-behaviour sanitizers on the host code, nothing preloaded anywhere"""
    assert _program_lines(program[1], True) == program[0]
