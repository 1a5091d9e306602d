"""The convex-NMF learner (evc_convex_learn), host side: the C ABI's declarations, struct mirror, status codes and their
order, the workspace query, the numpy restatement against recorded pymf results, the mirror's k-means start, the Python
surface's errors and the stand-alone host program (csrc/evc_convex_plan.h), plainly and under the sanitizers.  No GPU needed."""
import ctypes as C
import glob
import inspect
import os
import random
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convex_restatement as cr  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
GIVEN = ["cnmf_m25_t70_r8", "cnmf_m40_t257_r17", "cnmf_m3_t5_r2", "cnmf_m25_t300_r33", "cnmf_zeros", "cnmf_honly", "cnmf_gonly"]
DEFAULT = ["cnmfd_doctest", "cnmfd_m25_t70_r8", "cnmfd_m40_t257_r17"]


def lib():
    from exemplars_vc_amd import _lib
    return _lib, _lib.lib()


def nrel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), np.finfo(float).tiny))


def fixture_update(d):
    return "both" if bool(d["compute_w"]) and bool(d["compute_h"]) else ("h" if bool(d["compute_h"]) else "g")


def test_every_recorded_fixture_is_listed():
    names = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN, "cnmf*.npz")))
    assert names == sorted(GIVEN + DEFAULT)


def test_symbols_declared_and_exported():
    _lib, L = lib()
    hdr = open(os.path.join(ROOT, "include", "evc.h")).read()
    declared = set(re.findall(r"\b(evc_[a-z_0-9]+)\s*\(", hdr))
    for sym in ("evc_convex_workspace_bytes", "evc_convex_splits", "evc_convex_learn"):
        assert sym in declared and sym in _lib.SYMBOLS and hasattr(L, sym)
    assert "evc_convex_learn " in hdr[:hdr.index("#ifndef EVC_H")]
    assert (_lib.CONVEX_BOTH, _lib.CONVEX_H_ONLY, _lib.CONVEX_G_ONLY) == (0, 1, 2)
    assert "EVC_CONVEX_BOTH = 0, EVC_CONVEX_H_ONLY = 1, EVC_CONVEX_G_ONLY = 2" in hdr


def test_opts_mirror_matches_header():
    _lib, _ = lib()
    hdr = open(os.path.join(ROOT, "include", "evc.h")).read()
    body = hdr[hdr.index("typedef struct evc_convex_opts {"):hdr.index("} evc_convex_opts;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for grp in re.findall(r"\b(?:int|double|void\*)\s+([a-zA-Z_0-9, ]+);", body)
             for n in grp.replace(" ", "").split(",")]
    assert names == [f[0] for f in _lib.ConvexOpts._fields_]
    assert names == ["struct_bytes", "dtype", "layout", "iters", "check_every", "update", "reserved", "tol", "eps",
                     "ev_loop_start", "ev_loop_stop"]
    assert C.sizeof(_lib.ConvexOpts) == 8 * 4 + 2 * 8 + 2 * 8 and _lib.ConvexOpts.tol.offset == 32
    # the existing structs did not move
    assert C.sizeof(_lib.SemiOpts) == 8 * 4 + 3 * 8 + 2 * 8 and C.sizeof(_lib.BetaOpts) == 8 * 4 + 5 * 8 + 2 * 8


def _opts(_lib, **kw):
    o = _lib.ConvexOpts()
    o.struct_bytes = C.sizeof(_lib.ConvexOpts)
    o.dtype, o.layout, o.iters = _lib.F64, _lib.FRAME_MAJOR, 100
    o.check_every, o.update, o.tol, o.eps = 1, _lib.CONVEX_BOTH, 2.22e-16, 1e-9
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_status_codes_and_their_order():
    _lib, L = lib()
    one = C.c_void_p(8)              # never dereferenced: every case fails validation first

    def call(o, M=25, R=17, T=70, ldx=25, ldg=17, ldh=17, ldw=25, ws=16, X=one, G=one, H=one, W=one, wsp=one):
        return L.evc_convex_learn(X, ldx, G, ldg, H, ldh, W, ldw, M, R, T, None if o is None else C.byref(o), wsp, ws, None,
                                  None, None)
    # every valid call below is handed a 16-byte workspace: it gets as far as -2 and touches no device
    assert call(_opts(_lib)) == -2
    bad = _opts(_lib)
    bad.struct_bytes = 4
    assert call(bad) == -1 and call(None) == -1
    assert call(_opts(_lib), M=0) == -1 and call(_opts(_lib), R=0) == -1 and call(_opts(_lib), T=0) == -1
    for ld in (dict(ldx=24), dict(ldg=16), dict(ldh=16), dict(ldw=24)):
        assert call(_opts(_lib), **ld) == -1
    bin_major = dict(ldx=70, ldg=17, ldh=70, ldw=17)
    for ld in (dict(ldx=69), dict(ldg=16), dict(ldh=69), dict(ldw=16)):
        assert call(_opts(_lib, layout=_lib.BIN_MAJOR), **dict(bin_major, **ld)) == -1
    assert call(_opts(_lib, layout=_lib.BIN_MAJOR), **bin_major) == -2
    for p in ("X", "G", "H", "wsp"):
        assert call(_opts(_lib), **{p: None}) == -1
    assert call(_opts(_lib), W=None, ldw=0) == -2                         # W is optional
    for f in ("tol", "eps"):
        assert call(_opts(_lib, **{f: -1e-12})) == -1 and call(_opts(_lib, **{f: float("nan")})) == -1
        assert call(_opts(_lib, **{f: 0.0})) == -2
    assert call(_opts(_lib, eps=float("inf"))) == -1
    assert call(_opts(_lib, update=3)) == -1 and call(_opts(_lib, update=-1)) == -1
    assert call(_opts(_lib, update=_lib.CONVEX_H_ONLY)) == -2 and call(_opts(_lib, update=_lib.CONVEX_G_ONLY)) == -2
    assert call(_opts(_lib, dtype=7)) == -1 and call(_opts(_lib, layout=5)) == -1
    assert call(_opts(_lib, reserved=1)) == -1 and call(_opts(_lib, reserved=1 << 24)) == -1
    assert call(_opts(_lib, reserved=17 << 8)) == -1 and call(_opts(_lib, reserved=16 << 8)) == -2
    assert call(_opts(_lib, reserved=3 << 16)) == -1 and call(_opts(_lib, reserved=(2 << 16) | (7 << 8))) == -2
    assert call(_opts(_lib, iters=-1)) == -1 and call(_opts(_lib, check_every=-1)) == -1
    assert call(_opts(_lib, iters=4096)) == -2 and call(_opts(_lib, iters=0)) == -2 and call(_opts(_lib, dtype=_lib.F32)) == -2
    assert call(_opts(_lib, iters=4097)) == -1                                        # more than 4097 error slots
    assert call(_opts(_lib, iters=4097, check_every=0)) == -2
    assert call(_opts(_lib), ws=int(L.evc_convex_workspace_bytes(25, 17, 70, _lib.F64)) - 1) == -2
    # beyond the limits: -3, after every -1 and before -2, even with a tiny workspace
    big = 1 << 40
    assert call(_opts(_lib), M=1057, ldx=1057, ldw=1057) == -3 and call(_opts(_lib), M=1057, ldx=1057, ldw=1057, ws=big) == -3
    assert call(_opts(_lib), T=16385) == -3 and call(_opts(_lib), T=16385, ws=big) == -3
    assert call(_opts(_lib), R=1025, T=4096, ldg=1025, ldh=1025) == -3
    assert call(_opts(_lib), R=71, ldg=71, ldh=71) == -3 and call(_opts(_lib), R=70, ldg=70, ldh=70) == -2
    assert call(_opts(_lib), M=1056, ldx=1056, ldw=1056) == -2 and call(_opts(_lib), T=16384) == -2
    assert call(_opts(_lib, tol=float("nan")), M=1057, ldx=1057, ldw=1057) == -1
    assert call(_opts(_lib, reserved=4), T=16385) == -1
    assert call(_opts(_lib), M=1057, ldx=1057, ldw=1057, X=None) == -1
    assert call(_opts(_lib), R=71, ldg=70, ldh=71) == -1


def test_workspace_query_and_splits():
    _lib, L = lib()
    q, sp = L.evc_convex_workspace_bytes, L.evc_convex_splits
    assert q(1057, 8, 100, 0) == 0 and q(25, 8, 16385, 0) == 0 and q(25, 1025, 4096, 0) == 0 and q(25, 101, 100, 0) == 0
    assert q(0, 8, 100, 0) == 0 and q(25, 0, 100, 0) == 0 and q(25, 8, 0, 0) == 0 and q(25, 8, 100, 9) == 0
    assert q(1056, 8, 100, 0) > 0 and q(25, 100, 100, 1) > 0
    assert q(25, 8, 70, 0) < q(25, 8, 300, 0) < q(25, 33, 300, 0) < q(50, 33, 300, 0) and q(25, 8, 70, 1) < q(25, 8, 70, 0)
    for M, R, T, dt, es in ((25, 8, 70, _lib.F64, 8), (50, 256, 4096, _lib.F32, 4), (40, 17, 257, _lib.F64, 8)):
        TP, S = -(-T // 128) * 128, int(sp(R, T))
        Z = max(1, min(-(-256 // (-(-R // 64)) ** 2), -(-T // 16) // 4, 64))
        own = TP * TP * es + (4 + (2 * S if S > 1 else 0)) * T * R * es + (2 + (Z if Z > 1 else 0)) * R * R * es + (M * R + T * M) * es + T * 8 + 4097 * 8 + 12
        assert own <= int(q(M, R, T, dt)) <= own + 17 * 256
    assert 2 << 30 <= int(q(25, 64, 16384, _lib.F64)) < (2 << 30) + (1 << 28)              # the 2 GiB Gram matrix
    assert sp(0, 100) == 0 and sp(8, 0) == 0 and sp(101, 100) == 0 and sp(1025, 4096) == 0 and sp(8, 16385) == 0
    assert sp(64, 4096) == 16 and sp(256, 4096) == 4 and sp(1024, 4096) == 1 and sp(512, 16384) == 1 and sp(1, 16384) == 4
    assert sp(8, 70) == 1 and sp(33, 300) == 4
    # the existing query did not move
    assert int(L.evc_beta_workspace_bytes(25, 24, 70, 1, _lib.F64)) == 76800


@pytest.mark.parametrize("name", GIVEN + DEFAULT)
def test_restatement_reproduces_pymf(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    niter, T = int(d["niter"]), d["data"].shape[1]
    G, H, n_iter, tr = cr.learn(d["data"], d["G0"], d["H0"], niter, update=fixture_update(d), check_every=1, tol=cr.PYMF_TOL)
    ferr = cr.pymf_ferr(tr, n_iter, niter, T)
    print(name, "G", nrel(G, d["G"]), "H", nrel(H, d["H"]), "ferr", nrel(ferr, d["ferr"]) if len(ferr) == len(d["ferr"]) else None)
    assert n_iter == int(d["n_iter"]) and len(ferr) == len(d["ferr"])
    assert nrel(G, d["G"]) <= 1e-12 and nrel(H, d["H"]) <= 1e-12 and nrel(ferr, d["ferr"]) <= 1e-12
    assert np.array_equal(G == 0, d["G"] == 0) and np.array_equal(H == 0, d["H"] == 0)
    assert (G >= 0).all() and (H >= 0).all() and nrel(d["data"] @ G, d["W"]) <= 1e-12
    assert np.all(np.diff(tr[1:1 + n_iter]) <= 0)                      # the error never rises
    if name == "cnmf_zeros":
        assert (d["G0"] == 0).sum() == 70 * 7 and np.array_equal(G == 0, d["G0"] == 0)
    if name == "cnmf_honly":
        assert np.array_equal(G, d["G0"])
    if name == "cnmf_gonly":
        assert np.array_equal(H, d["H0"])


def test_restatement_float32_stays_near_float64():
    d = np.load(os.path.join(GOLDEN, "cnmf_m25_t70_r8.npz"))
    G, H, _, tr = cr.learn(d["data"], d["G0"], d["H0"], 30, dtype=np.float32)
    assert G.dtype == np.float32 and H.dtype == np.float32 and tr.dtype == np.float64
    assert 1e-9 < nrel(G, d["G"]) < 1e-4 and 1e-9 < nrel(H, d["H"]) < 1e-4


@pytest.mark.parametrize("name", DEFAULT)
def test_kmeans_start_reproduces_pymf_bit_for_bit(name):
    from exemplars_vc_amd.compat import pymf
    from exemplars_vc_amd.solver import convex_cluster_start
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    R = d["G0"].shape[1]
    state = random.getstate()
    try:
        random.seed(int(d["seed"]))
        mdl = pymf.CNMF(d["data"].copy(), num_bases=R)
        mdl._init_h()
    finally:
        random.setstate(state)
    assert np.array_equal(mdl.G, d["G0"]) and np.array_equal(mdl.H, d["H0"]) and np.array_equal(mdl.W, d["data"] @ d["G0"])
    assign = np.argmax(d["H0"], axis=0)
    G0, H0 = convex_cluster_start(assign, R)
    assert np.array_equal(G0, d["G0"]) and np.array_equal(H0, d["H0"])
    g2, h2 = cr.cluster_start(assign, R)
    assert np.array_equal(g2, G0) and np.array_equal(h2, H0)


def test_python_surface():
    import exemplars_vc_amd as evc
    from exemplars_vc_amd.compat import pymf
    for name in ("learn_dictionary_convex", "compact_dictionary_convex"):
        assert name in evc.__all__ and callable(getattr(evc, name))
    sig = inspect.signature(evc.learn_dictionary_convex).parameters
    assert list(sig)[:3] == ["X", "G0", "H0"] and sig["eps"].default == 1e-9 and sig["update"].default == "both"
    assert sig["check_every"].default == 1 and sig["tol"].default == 0.0
    for k in ("layout", "iters", "update", "check_every", "tol", "eps", "dtype", "device", "info", "out_g", "out_h"):
        assert sig[k].kind is inspect.Parameter.KEYWORD_ONLY, k
    csig = inspect.signature(evc.compact_dictionary_convex).parameters
    assert list(csig)[:3] == ["A", "B", "R"] and csig["iters"].default == 100 and csig["assign"].default is None
    fsig = inspect.signature(pymf.CNMF.factorize).parameters
    assert list(fsig)[1:] == ["niter", "compute_w", "compute_h", "compute_err", "show_progress"]
    assert fsig["niter"].default == 10 and fsig["compute_w"].default is True
    X, G0, H0 = np.ones((5, 7)), np.ones((7, 3)), np.ones((3, 7))
    with pytest.raises(ValueError, match="one row per exemplar"):
        evc.learn_dictionary_convex(X, np.ones((6, 3)), H0, layout="bin_major", iters=1)
    with pytest.raises(ValueError, match="2-D"):
        evc.learn_dictionary_convex(X[0], G0, H0, layout="bin_major", iters=1)
    with pytest.raises(ValueError, match="update"):
        evc.learn_dictionary_convex(X, G0, H0, layout="bin_major", iters=1, update="w")
    with pytest.raises(ValueError, match="1056 bins"):
        evc.learn_dictionary_convex(np.ones((1057, 7)), G0, H0, layout="bin_major", iters=1)
    with pytest.raises(ValueError, match="16384 exemplars"):
        evc.learn_dictionary_convex(np.ones((16385, 2)), np.ones((16385, 3)), np.ones((16385, 3)), layout="frame_major", iters=1)
    with pytest.raises(ValueError, match="atoms"):
        evc.learn_dictionary_convex(X, np.ones((7, 8)), np.ones((8, 7)), layout="bin_major", iters=1)
    with pytest.raises(ValueError, match="dtype"):
        evc.learn_dictionary_convex(X, G0, H0, layout="bin_major", iters=1, dtype="f16")
    with pytest.raises(ValueError, match="number of exemplars"):
        evc.compact_dictionary_convex(np.ones((5, 7)), np.ones((4, 6)), 2)
    with pytest.raises(ValueError, match="R must be"):
        evc.compact_dictionary_convex(np.ones((5, 7)), np.ones((4, 7)), 8)
    with pytest.raises(ValueError, match="label"):
        evc.compact_dictionary_convex(np.ones((5, 7)), np.ones((4, 7)), 2, assign=[0, 1, 2, 0, 1, 0, 1])
    mdl = pymf.CNMF(np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]]), num_bases=2)
    mdl.H = np.ones((2, 3))
    with pytest.raises(AttributeError, match="set .G"):
        mdl.factorize(niter=1)
    mdl.G = np.ones((3, 2))
    mdl.W = np.ones((2, 2))
    with pytest.raises(NotImplementedError, match="stale W"):
        mdl.factorize(niter=1, compute_w=False)
    with pytest.raises(ValueError, match="dictionary_update"):
        pymf.CNMF(np.ones((2, 3)), num_bases=2, dictionary_update="device")
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            evc.learn_dictionary_convex(X, G0, H0, layout="bin_major", iters=3)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            evc.compact_dictionary_convex(np.ones((5, 7)), np.ones((4, 7)), 2)


# ---- the host pieces of the driver (csrc/evc_convex_plan.h) in a program of their own, plainly and under the sanitizers ----
SRC = os.path.join(ROOT, "tests", "convex_host_main.hip")
PKG = os.path.join(ROOT, "exemplars_vc_amd")


def _program_lines(tmp, sanitize):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = os.path.join(tmp, "convex_host_main" + ("_san" if sanitize else ""))
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
    tmp = str(tmp_path_factory.mktemp("convex_host"))
    return _program_lines(tmp, False), tmp


def test_host_carving(program):
    _lib, L = lib()
    carves = [ln.split() for ln in program[0] if ln.startswith("carve ")]
    assert len(carves) == 12 and not any("BAD" in ln for ln in program[0])
    for c in carves:
        M, R, T, S, esize, shift = (int(v) for v in c[1:6] + [c[7]])
        offs = [int(v) for v in c[9:24]]
        # disjoint (the program checked every array's room against its successor), ascending and 256-byte aligned
        assert offs[0] == (256 - shift) % 256 and offs == sorted(offs) and all((o + shift) % 256 == 0 for o in offs)
        if S == int(L.evc_convex_splits(R, T)):
            assert int(c[-1]) == int(L.evc_convex_workspace_bytes(M, R, T, _lib.F64 if esize == 8 else _lib.F32))
        assert int(c[-3]) <= int(c[-1])


def test_host_argument_checks_in_status_order(program):
    rows = {ln.split()[1]: tuple(int(v) for v in ln.split()[2:]) for ln in program[0] if ln.startswith("args ")}
    status = {k: v[0] for k, v in rows.items()}
    want = dict(ok=0, ok_exact=0, short_by_one=-2, f32_ws=-2, no_w=0, no_g=-1, ldg_short=-1, ldg_padded=0, struct_bytes=-1,
                iters_neg=-1, iters_0=0, slots_4097=0, slots_4098=-1, check_every_neg=-1, check_every_0=0, reserved_low=-1,
                reserved_high=-1, forced_s7=0, forced_s7_plan_ws=-2, forced_s7_own_ws=0, forced_s16=0, forced_s17=-1, forced_w8=0,
                forced_w4_s3=0, forced_w3=-1, forced_w1=-1, h_only=0, g_only=0, update_3=-1, tol_neg=-1, tol_0=0, eps_neg=-1,
                eps_0=0, eps_nan=-1, eps_inf=-1, dtype=-1, layout=-1, M_0=-1, R_0=-1, T_0=-1, M_1056=0, M_1057=-3,
                M_1057_small_ws=-3, T_16384=0, T_16384_small_ws=-2, T_16385=-3, T_16385_small_ws=-3, R_1024=0, R_1025=-3,
                R_eq_T=0, R_above_T=-3, R_above_T_small_ws=-3, nan_before_limits=-1, reserved_before_limits=-1)
    assert status == want
    # the plan a good call leaves: the sizes' own, or what `reserved` forces
    assert rows["ok"][1:] == (2, 1) and rows["forced_s7"][1:] == (2, 7) and rows["forced_w8"][1:] == (8, 1)
    assert rows["forced_w4_s3"][1:] == (4, 3) and rows["forced_s16"][1:] == (2, 16)


def test_host_plan_depends_on_the_sizes_only_and_fills_the_chip(program):
    _lib, L = lib()
    plan = {(int(v[1]), int(v[2])): (int(v[3]), int(v[4]), int(v[5])) for v in (ln.split() for ln in program[0]) if v[0] == "plan"}
    rr = {(int(v[1]), int(v[2])): int(v[6]) for v in (ln.split() for ln in program[0]) if v[0] == "plan"}
    assert len(plan) > 200
    for (T, R), (W, S, wgs) in plan.items():
        TP, cols, slabs = -(-T // 128) * 128, -(-R // 64), -(-T // 16)
        assert W in (8, 4, 2) and 1 <= S <= 16 and wgs == TP // (16 * W) * cols * S
        assert S == int(L.evc_convex_splits(R, T))                    # the library's own answer: the same function
        # k is split first - ranges of at least four slabs, at most 16 - and the block narrows only where that cap is short of
        # 512 workgroups: the widest block that gets there, else the narrowest with every range at the cap
        cap = max(1, min(16, slabs // 4))
        need = {w: -(-512 // (TP // (16 * w) * cols)) for w in (8, 4, 2)}
        want = next(((w, need[w]) for w in (8, 4, 2) if need[w] <= cap), (2, cap))
        assert (W, S) == want
        # at least 512 workgroups wherever T R allows: short of them only at the narrowest block with S at its cap
        assert wgs >= 512 or (W, S) == (2, cap)
        assert S == 1 or wgs - TP // (16 * W) * cols < 512              # never more ranges than it takes
    # monotone: more columns or more rows never narrow the block; at one width more columns never add ranges
    Ts, Rs = sorted({k[0] for k in plan}), sorted({k[1] for k in plan})
    for T in Ts:
        row = [plan[(T, R)] for R in Rs if (T, R) in plan]
        assert all(a[0] <= b[0] and (a[0] != b[0] or a[1] >= b[1]) for a, b in zip(row, row[1:]))
    for R in Rs:
        col = [plan[(T, R)] for T in Ts if (T, R) in plan]
        assert all(a[0] <= b[0] for a, b in zip(col, col[1:]))
        big = [p for T, p in zip([T for T in Ts if (T, R) in plan], col) if T >= 1024]     # the cap is 16 from there on
        assert all(a[0] != b[0] or a[1] >= b[1] for a, b in zip(big, big[1:]))
    # the issue's shapes: T = 4096 with R = 64 gives 32 workgroups of 128 rows - split into 16 ranges
    assert plan[(4096, 64)] == (8, 16, 512) and plan[(4096, 256)] == (8, 4, 512) and plan[(4096, 1024)] == (8, 1, 512)
    assert plan[(16384, 512)] == (8, 1, 1024) and plan[(16384, 1)] == (8, 4, 512) and plan[(1, 1)] == (2, 1, 4)
    # the k-ranges of the R x R products: 256 workgroups from ceil(R / 64)^2 tiles, ranges of at least four slabs, at most 64
    for (T, R), z in rr.items():
        assert z == max(1, min(-(-256 // (-(-R // 64)) ** 2), -(-T // 16) // 4, 64))
    assert rr[(4096, 64)] == 64 and rr[(4096, 256)] == 16 and rr[(4096, 1024)] == 1 and rr[(16384, 512)] == 4 and rr[(63, 17)] == 1
    assert plan[(1024, 64)] == (2, 16, 512) and plan[(300, 33)] == (2, 4, 48)


def test_the_host_program_runs_clean_under_the_sanitizers(program):
    """a stand-alone program: address + undefined-behaviour sanitizers on the host code, nothing preloaded anywhere"""
    assert _program_lines(program[1], True) == program[0]
