"""The mini-batch estimator's activation solve (evc_online_transform), its fit with fresh restarts and partial_fit
(evc_online_learn_fresh), host side: the C ABI's declarations, struct mirror
and argument checks, the numpy restatement against scikit-learn's recorded MiniBatchNMF.transform runs
(tests/golden/mbnmf_tr_*.npz), the fixture generator, the stand-alone host program and the Python surface's validation.
No GPU needed."""
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
import minibatch_restatement as mr  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "mbnmf_tr_*.npz")))
FR_FILES = sorted(glob.glob(os.path.join(GOLDEN, "mbnmf_fr_*.npz")))
PF_FILES = sorted(glob.glob(os.path.join(GOLDEN, "mbnmf_pf_*.npz")))
E64 = 2.0 ** -52
KEYS = {"X", "W", "H", "n_iter", "change", "max_iter", "tol", "beta", "alpha", "l1_ratio", "dtype", "margin"}
MARGIN = {"float64": 1e-6, "float32": 1e-2}         # tools/make_golden_online.MARGIN


def lib():
    from exemplars_vc_amd import _lib
    return _lib, _lib.lib()


def test_symbols_declared_and_exported():
    _lib, L = lib()
    hdr = open(os.path.join(ROOT, "include", "evc.h")).read()
    declared = set(re.findall(r"\b(evc_[a-z_0-9]+)\s*\(", hdr))
    for sym in ("evc_online_transform", "evc_online_transform_workspace_bytes", "evc_online_learn_fresh",
                "evc_online_fresh_workspace_bytes"):
        assert sym in declared and sym in _lib.SYMBOLS and hasattr(L, sym)
    top = hdr[:hdr.index("#ifndef EVC_H")]
    assert "evc_online_transform " in top and "evc_online_learn_fresh " in top          # listed in the header comment
    sync = hdr[hdr.index("Host synchronisation"):hdr.index("No global mutable state")]
    order = [sync.index(c) for c in ("(10) evc_online_learn", "(11) evc_online_transform", "(12) evc_online_learn_fresh")]
    assert order == sorted(order)
    body = hdr[hdr.index("Mini-batch (online) dictionary learning"):]
    assert "served by\n * evc_online_transform" in body and "by\n * evc_online_learn_fresh" in body
    for out_of_scope in ("fresh_restarts=True", "partial_fit", "sparse X", "shuffled"):
        assert out_of_scope in body
    assert L.evc_version() == 100


def test_opts_mirror_matches_header():
    _lib, _ = lib()
    hdr = open(os.path.join(ROOT, "include", "evc.h")).read()
    body = hdr[hdr.index("typedef struct evc_transform_opts {"):hdr.index("} evc_transform_opts;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for grp in re.findall(r"\b(?:int|double|void\*)\s+([a-zA-Z_0-9, ]+);", body)
             for n in grp.replace(" ", "").split(",")]
    assert names == [f[0] for f in _lib.TransformOpts._fields_]
    assert names == ["struct_bytes", "dtype", "layout", "max_iter", "init_mode", "reserved", "beta", "tol", "l1", "l2",
                     "init_value", "ev_loop_start", "ev_loop_stop"]
    assert C.sizeof(_lib.TransformOpts) == 6 * 4 + 5 * 8 + 2 * 8
    body = hdr[hdr.index("typedef struct evc_online_fresh_opts {"):hdr.index("} evc_online_fresh_opts;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for grp in re.findall(r"\b(?:int|double|void\*)\s+([a-zA-Z_0-9, ]+);", body)
             for n in grp.replace(" ", "").split(",")]
    assert names == [f[0] for f in _lib.OnlineFreshOpts._fields_]
    shared = [f[0] for f in _lib.OnlineOpts._fields_]
    assert names == shared[:8] + ["fresh_max_iter", "final_max_iter"] + shared[8:]
    assert C.sizeof(_lib.OnlineFreshOpts) == 10 * 4 + 7 * 8 + 2 * 8
    # the existing structs did not move
    assert C.sizeof(_lib.BetaOpts) == 8 * 4 + 5 * 8 + 2 * 8 and C.sizeof(_lib.OnlineOpts) == 8 * 4 + 7 * 8 + 2 * 8


def _opts(_lib, **kw):
    o = _lib.TransformOpts()
    o.struct_bytes = C.sizeof(_lib.TransformOpts)
    o.dtype, o.layout, o.max_iter, o.init_mode = _lib.F64, _lib.FRAME_MAJOR, 200, _lib.INIT_SKLEARN
    o.beta, o.tol = 0.5, 1e-4
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_bad_arguments_rejected_before_device_work():
    _lib, L = lib()
    one = C.c_void_p(8)              # never dereferenced: every case fails validation first

    def call(o, M=25, R=17, T=70, ldw=25, ldx=25, ldh=17, ws=1 << 40, W=one, X=one, H=one, wsp=one, offs=None, n_utt=1):
        po = None if offs is None else (C.c_int * len(offs))(*offs)
        return L.evc_online_transform(W, ldw, X, ldx, H, ldh, M, R, T, po, n_utt, None if o is None else C.byref(o), wsp, ws,
                                      None, None, None)
    bad = _opts(_lib)
    bad.struct_bytes = 4
    assert call(bad) == -1 and call(None) == -1
    assert call(_opts(_lib), M=0) == -1 and call(_opts(_lib), R=0) == -1 and call(_opts(_lib), T=-1) == -1
    assert call(_opts(_lib), n_utt=0) == -1
    for ld in ("ldw", "ldx"):
        assert call(_opts(_lib), **{ld: 24}) == -1
    assert call(_opts(_lib), ldh=16) == -1
    for ld in (dict(ldw=16), dict(ldx=69), dict(ldh=69)):
        assert call(_opts(_lib, layout=_lib.BIN_MAJOR), **dict(dict(ldw=17, ldx=70, ldh=70), **ld)) == -1
    assert call(_opts(_lib, layout=_lib.BIN_MAJOR), ldw=17, ldx=70, ldh=70, ws=16) == -2
    for p in ("W", "X", "H", "wsp"):
        assert call(_opts(_lib), **{p: None}) == -1
    assert call(_opts(_lib), T=0, X=None, H=None, ws=16) == -2       # no frames: X and H are never touched
    assert call(_opts(_lib), offs=[0, 40, 30, 70], n_utt=3) == -1
    assert call(_opts(_lib), offs=[0, 30, 30, 70], n_utt=3, ws=16) == -2
    for v in (float("nan"), float("inf"), -float("inf")):
        assert call(_opts(_lib, beta=v)) == -1
        assert call(_opts(_lib, init_value=v)) == -1
    for f in ("tol", "l1", "l2"):
        assert call(_opts(_lib, **{f: -1e-4})) == -1
        assert call(_opts(_lib, **{f: float("nan")})) == -1
    assert call(_opts(_lib, tol=0.0), ws=16) == -2
    assert call(_opts(_lib, max_iter=-1)) == -1
    assert call(_opts(_lib, max_iter=0), ws=16) == -2
    assert call(_opts(_lib, max_iter=4097), ws=16) == -2
    assert call(_opts(_lib, max_iter=4098)) == -1                      # evc_beta_solve's slot limit
    assert call(_opts(_lib, reserved=1)) == -1
    assert call(_opts(_lib, init_mode=3)) == -1 and call(_opts(_lib, init_mode=-1)) == -1
    for mode in (_lib.INIT_GIVEN, _lib.INIT_SKLEARN, _lib.INIT_CONST):
        assert call(_opts(_lib, init_mode=mode), ws=16) == -2
    assert call(_opts(_lib, dtype=7)) == -1 and call(_opts(_lib, layout=5)) == -1
    assert call(_opts(_lib), ws=16) == -2                         # workspace too small
    assert call(_opts(_lib), ws=int(L.evc_online_transform_workspace_bytes(25, 17, 70, 1, _lib.F64)) - 1) == -2
    assert call(_opts(_lib), M=529, ldw=529, ldx=529) == -3
    assert call(_opts(_lib), M=529, ldw=529, ldx=529, ws=16) == -3             # -3 before -2
    assert call(_opts(_lib, beta=float("nan")), M=529, ldw=529, ldx=529) == -1        # -1 before -3
    assert call(_opts(_lib, max_iter=4098), M=529, ldw=529, ldx=529, ws=16) == -1


def _fopts(_lib, **kw):
    o = _lib.OnlineFreshOpts()
    o.struct_bytes = C.sizeof(_lib.OnlineFreshOpts)
    o.dtype, o.layout, o.batch_size, o.max_iter, o.max_no_improvement = _lib.F64, _lib.FRAME_MAJOR, 32, 5, 10
    o.fresh_max_iter, o.final_max_iter = 30, 200
    o.beta, o.tol, o.forget_factor = 0.5, 1e-4, 0.7
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_fresh_bad_arguments_rejected_before_device_work():
    _lib, L = lib()
    one = C.c_void_p(8)              # never dereferenced: every case fails validation first

    def call(o, M=25, R=17, T=70, ldx=25, ldw=25, ldh=17, lda=25, ws=1 << 40, X=one, W=one, H=one, A=one, B=one, wsp=one):
        return L.evc_online_learn_fresh(X, ldx, W, ldw, H, ldh, A, B, lda, M, R, T, C.byref(o), wsp, ws, None, None, None, None)
    assert call(_fopts(_lib, struct_bytes=C.sizeof(_lib.OnlineOpts))) == -1
    for kw in (dict(fresh_max_iter=0), dict(fresh_max_iter=-1), dict(fresh_max_iter=4098), dict(final_max_iter=-1),
               dict(final_max_iter=4098), dict(batch_size=0), dict(max_iter=-1), dict(resume=2), dict(forget_factor=0.0),
               dict(beta=float("nan")), dict(tol=-1.0), dict(l1_w=-1.0), dict(dtype=7), dict(layout=5), dict(reserved=1)):
        assert call(_fopts(_lib, **kw)) == -1, kw
    for p in ("X", "W", "H", "A", "B", "wsp"):
        assert call(_fopts(_lib), **{p: None}) == -1
    assert call(_fopts(_lib), M=0) == -1 and call(_fopts(_lib), T=0) == -1 and call(_fopts(_lib), ldh=16) == -1
    for kw in (dict(), dict(final_max_iter=0), dict(fresh_max_iter=4097, final_max_iter=4097), dict(tol=0.0, max_no_improvement=-1)):
        assert call(_fopts(_lib, **kw), ws=16) == -2, kw
    assert call(_fopts(_lib), ws=int(L.evc_online_workspace_bytes(25, 17, 70, 32, _lib.F64))) == -2       # the plain learner's
    assert call(_fopts(_lib), ws=int(L.evc_online_fresh_workspace_bytes(25, 17, 70, 32, _lib.F64)) - 1) == -2
    assert call(_fopts(_lib), M=529, ldx=529, ldw=529, lda=529, ws=16) == -3             # -3 before -2
    assert call(_fopts(_lib, reserved=1 << 16), R=257, ldh=257) == -3
    assert call(_fopts(_lib, fresh_max_iter=0), M=529, ldx=529, ldw=529, lda=529, ws=16) == -1        # -1 before -3
    q, q0 = L.evc_online_fresh_workspace_bytes, L.evc_online_workspace_bytes
    for a in ((25, 24, 330, 100, 0), (201, 32, 200, 1024, 1), (50, 512, 65536, 1024, 0)):
        M, R, T, bs, dt = a
        extra = int(q(*a)) - int(q0(*a))
        nb = -(-T // min(bs, T))
        assert extra >= int(L.evc_beta_workspace_bytes(M, R, T, 1, dt)) + ((T + 15) // 16 + nb) * 16 * 2 * 8
    assert q(25, 16, 6880, 1024, 0) < q(25, 128, 6880, 1024, 0) < q(25, 128, 68800, 1024, 0)
    assert q(529, 1, 1, 1, 0) == 0 and q(25, 4097, 1, 1, 0) == 0 and q(25, 1, 0, 1, 0) == 0 and q(25, 1, 1, 0, 0) == 0
    assert q(25, 1, 1, 1, 9) == 0 and q(528, 4096, 1, 1, 0) > 0


def test_workspace_query():
    _lib, L = lib()
    q = L.evc_online_transform_workspace_bytes
    assert q(25, 16, 688, 1, _lib.F64) < q(25, 128, 688, 1, _lib.F64) < q(25, 128, 6880, 1, _lib.F64)
    assert q(25, 128, 6880, 1, _lib.F64) < q(25, 128, 6880, 10, _lib.F64)
    assert q(25, 16, 688, 1, _lib.F64) < q(201, 16, 688, 1, _lib.F64)
    assert q(201, 20, 688, 1, _lib.F32) < q(201, 20, 688, 1, _lib.F64)
    assert q(528, 100000, 0, 1, 0) > 0 and q(529, 1, 1, 1, 0) == 0
    assert q(0, 1, 1, 1, 0) == 0 and q(25, 0, 1, 1, 0) == 0 and q(25, 1, -1, 1, 0) == 0 and q(25, 1, 1, 0, 0) == 0
    assert q(25, 1, 1, 1, 9) == 0
    # the activation half's workspace plus the per-frame shares of the change sums
    for M, R, T, n in ((25, 24, 70, 1), (201, 512, 11008, 16), (50, 512, 65536, 1)):
        extra = int(q(M, R, T, n, _lib.F64)) - int(L.evc_beta_workspace_bytes(M, R, T, n, _lib.F64))
        assert ((T + 15) // 16 + n) * 16 * 2 * 8 <= extra <= ((T + 15) // 16 + n) * 16 * 2 * 8 + 1024
    # the existing query did not move: carved sizes at the parent commit
    assert int(L.evc_beta_workspace_bytes(25, 24, 70, 1, _lib.F64)) == 76800 and int(L.evc_beta_workspace_bytes(201, 512, 11008, 16, _lib.F32)) == 10851328


def options(d):
    M = d["X"].shape[0]
    a, r = float(d["alpha"]), float(d["l1_ratio"])
    return dict(beta=float(d["beta"]), max_iter=int(d["max_iter"]), tol=float(d["tol"]), l1=M * a * r, l2=M * a * (1 - r))


def test_fixture_table():
    names = [os.path.basename(p)[:-4] for p in FILES]
    assert len(FILES) == 15
    assert len(glob.glob(os.path.join(GOLDEN, "online_sk_*.npz"))) == 18         # the neighbouring prefix is untouched
    shapes, betas, stops, counts = set(), set(), {"tol": 0, "none": 0}, set()
    for p in FILES:
        d = np.load(p)
        assert os.path.getsize(p) <= 1 << 20 and set(d.files) == KEYS
        (M, T), R = d["X"].shape, d["W"].shape[1]
        shapes.add((M, R, T))
        betas.add(float(d["beta"]))
        dt = np.dtype(str(d["dtype"]))
        assert d["X"].dtype == d["W"].dtype == d["H"].dtype == dt and d["H"].shape == (R, T)
        n, K, tol = int(d["n_iter"]), int(d["max_iter"]), float(d["tol"])
        ch = d["change"]
        assert ch.shape == (n,) and tol > 0 and 2 < n <= 140
        # every decision is clear of its threshold
        assert (ch[:-1] > tol * (1 + MARGIN[dt.name])).all() and float(d["margin"]) >= MARGIN[dt.name]
        assert float(d["margin"]) == pytest.approx(float(np.min(np.abs(ch - tol) / tol)), rel=1e-12)
        stopped = ch[-1] <= tol
        assert stopped == (n < K) and (stopped or ch[-1] > tol * (1 + MARGIN[dt.name]))
        stops["tol" if stopped else "none"] += 1
        counts.add(n)
        pos = d["H"][d["H"] > 0].astype(np.float64)
        assert np.isfinite(d["H"]).all() and not np.any((pos > E64 * (1 - 1e-3)) & (pos < E64 * (1 + 1e-3)))
    assert shapes == {(25, 24, 70), (33, 272, 50), (201, 32, 40)}
    assert betas == {2.0, 1.0, 0.0, 0.5, 1.5, 3.0}
    assert stops == {"tol": 13, "none": 2} and len(counts) >= 8
    assert sum("_f32_" in n for n in names) == 2 and sum("_reg_" in n for n in names) == 1
    reg = np.load(os.path.join(GOLDEN, "mbnmf_tr_m25_r24_t70_tol_reg_b1p5.npz"))
    assert float(reg["alpha"]) == 1e-3 and float(reg["l1_ratio"]) == 0.5


def test_fresh_and_partial_fixture_tables():
    assert (len(FR_FILES), len(PF_FILES)) == (6, 3)
    shapes, stops = set(), {"tol": 0, "mni": 0, "none": 0}
    for p in FR_FILES:
        d = np.load(p)
        dt = np.dtype(str(d["dtype"]))
        assert os.path.getsize(p) <= 1 << 20 and "H0" not in d.files
        (M, T), R, bs = d["X"].shape, d["W0"].shape[1], int(d["batch_size"])
        shapes.add((M, R, T, bs))
        n, per_pass = int(d["n_steps"]), -(-T // bs)
        assert d["cost"].shape == d["change"].shape == (n,) and int(d["n_iter"]) == -(-n // per_pass)
        solves, F, K2 = d["solve_iters"], int(d["fresh_max_iter"]), int(d["final_max_iter"])
        assert solves.shape == (n + 1,) and (solves[:-1] <= F).all() and solves[-1] <= K2 and solves.max() <= 140
        full = n == int(d["max_iter"]) * per_pass
        tol = float(d["tol"])
        stops["none" if full else "tol" if d["change"][-1] <= tol else "mni"] += 1
        assert float(d["margin"]) >= MARGIN[dt.name]
        if tol == 0:
            assert (solves[:-1] == F).all() and solves[-1] == K2          # nothing stops a solve
        for Fm in (d["W"], d["H"]):
            pos = Fm[Fm > 0].astype(np.float64)
            assert np.isfinite(Fm).all() and not np.any((pos > E64 * (1 - 1e-3)) & (pos < E64 * (1 + 1e-3)))
    assert shapes == {(25, 24, 300, 100), (25, 24, 330, 100)}
    assert stops == {"tol": 1, "mni": 1, "none": 4}
    d = np.load(os.path.join(GOLDEN, "mbnmf_fr_m25_r24_t330_bs100_k2_flush_b0p5.npz"))
    assert float(d["beta"]) < 1 and (d["W0"] == 1e-19).sum() >= 10 and (d["W"] > 0).all() and (d["H"] > 0).all()
    d = np.load(os.path.join(GOLDEN, "mbnmf_fr_m25_r24_t300_bs100_tol_b0p5.npz"))
    assert (d["solve_iters"] < int(d["fresh_max_iter"])).all()            # every solve of that fit stops by tol
    for p in PF_FILES:
        d = np.load(p)
        o = d["offsets"]
        assert os.path.getsize(p) <= 1 << 20 and o.tolist() == [0, 150, 220, 330] and int(d["batch_size"]) == 100
        assert float(d["rho"]) == float(d["forget_factor"]) ** (100 / 150) != float(d["forget_factor"])
        assert float(d["margin"]) >= 1e-6 and (d["solve_iters"] < int(d["fresh_max_iter"])).all() and d["solve_iters"].max() <= 140
        assert len(set(d["solve_iters"].tolist())) == 3
    assert {float(np.load(p)["beta"]) for p in PF_FILES} == {2.0, 0.5, 1.5}
    assert any(float(np.load(p)["alpha"]) == 1e-3 for p in PF_FILES)


def close_factor(got, ref, rtol=1e-12):
    assert np.array_equal(got == 0, ref == 0)
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=0)


@pytest.mark.parametrize("path", FR_FILES, ids=os.path.basename)
def test_fresh_restatement_reproduces_sklearn_fixture(path):
    """counts exactly, factors to 1e-12 in float64 (the generic statement at beta = 2 included); float32 as test_online_host"""
    d = np.load(path)
    dt = np.dtype(str(d["dtype"]))
    mni = int(d["max_no_improvement"])
    W, H, n_iter, n_steps, cost, change, _, solves = mr.learn_fresh(
        d["X"], d["W0"], float(d["beta"]), int(d["batch_size"]), int(d["max_iter"]), float(d["forget_factor"]), float(d["tol"]),
        None if mni < 0 else mni, fresh_max_iter=int(d["fresh_max_iter"]), final_max_iter=int(d["final_max_iter"]), dtype=dt)
    assert (n_iter, n_steps, solves) == (int(d["n_iter"]), int(d["n_steps"]), d["solve_iters"].tolist())
    assert W.dtype == H.dtype == dt and np.isnan(cost[n_steps:]).all()
    if dt == np.float64:
        close_factor(W, d["W"])
        close_factor(H, d["H"])
        np.testing.assert_allclose(cost[:n_steps], d["cost"], rtol=1e-12, atol=0)
        np.testing.assert_allclose(change[:n_steps], d["change"], rtol=1e-9, atol=1e-12)
    else:
        for got, ref in ((W, d["W"]), (H, d["H"])):
            assert np.linalg.norm(got.astype(np.float64) - ref) / np.linalg.norm(ref) <= 1e-4
        np.testing.assert_allclose(cost[:n_steps], d["cost"], rtol=1e-4, atol=0)
        np.testing.assert_allclose(change[:n_steps], d["change"], rtol=1e-3, atol=1e-6)


@pytest.mark.parametrize("path", PF_FILES, ids=os.path.basename)
def test_partial_fit_restatement_reproduces_sklearn_fixture(path):
    d = np.load(path)
    o = d["offsets"]
    out = mr.partial_fit([d["X"][:, a:b] for a, b in zip(o[:-1], o[1:])], d["W0"], float(d["beta"]), int(d["batch_size"]),
                         float(d["forget_factor"]), float(d["tol"]), float(d["alpha"]), float(d["l1_ratio"]),
                         int(d["fresh_max_iter"]))
    assert [n for _, _, _, n in out] == d["solve_iters"].tolist()
    for c, (W, A, B, _) in enumerate(out):
        close_factor(W, d[f"W_{c}"])
        close_factor(A, d[f"A_{c}"])
        close_factor(B, d[f"B_{c}"])


@pytest.mark.parametrize("path", FILES, ids=os.path.basename)
def test_restatement_reproduces_sklearn_fixture(path):
    """n_iter exactly; float64 to 1e-12 (test_beta_host's bound), with scikit-learn's special cases at beta = 1 and 2 and with
    the generic statement the kernel runs; float32 to what test_online_host allows its restatement (1e-4 norm-relative,
    the ratios rtol 1e-3 / atol 1e-6)"""
    d = np.load(path)
    dt = np.dtype(str(d["dtype"]))
    n = int(d["n_iter"])
    for sk in (True, False):
        H, n_iter, change = mr.solve_w(d["X"], d["W"], dtype=dt, sklearn=sk, **options(d))
        assert H.dtype == dt and n_iter == n
        assert np.isnan(change[n:]).all() and change.shape == (int(d["max_iter"]),)
        err = float(np.linalg.norm(H.astype(np.float64) - d["H"]) / np.linalg.norm(d["H"]))
        print(os.path.basename(path), "sklearn" if sk else "generic", "norm-relative error %.3e" % err)
        if dt == np.float64:
            assert err <= 1e-12 and np.array_equal(H == 0, d["H"] == 0)
            np.testing.assert_allclose(H, d["H"], rtol=1e-12, atol=0)
            np.testing.assert_allclose(change[:n], d["change"], rtol=1e-12, atol=0)
        else:
            assert err <= 1e-4
            np.testing.assert_allclose(change[:n], d["change"], rtol=1e-3, atol=1e-6)


def test_restatement_per_utterance():
    d = np.load(os.path.join(GOLDEN, "mbnmf_tr_m25_r24_t70_tol_b0p5.npz"))
    X, W = d["X"], d["W"]
    offs = [0, 30, 30, 70]
    H, n_iter, change = mr.transform(X, W, 0.5, 60, 1e-2, utt_offsets=offs)
    assert n_iter[1] == 60 and np.isnan(change[1]).all()
    for u in (0, 2):
        Hu, nu, cu = mr.solve_w(X[:, offs[u]:offs[u + 1]], W, 0.5, 60, 1e-2)
        assert np.array_equal(H[:, offs[u]:offs[u + 1]], Hu) and n_iter[u] == nu and np.array_equal(change[u], cu, equal_nan=True)
    H0, n0, c0 = mr.solve_w(X, W, 0.5, 0)
    assert n0 == 0 and c0.shape == (0,) and (H0 == np.sqrt(np.ascontiguousarray(X.T).mean() / 24)).all()


def test_generator_reproduces_the_fixtures():
    pytest.importorskip("sklearn")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_golden_minibatch as g
    specs = g.cases()
    assert sorted(specs) == sorted(os.path.basename(p)[:-4] for p in FILES)
    for name in ("mbnmf_tr_m25_r24_t70_tol_b0", "mbnmf_tr_m201_r32_t40_tol_b1p5"):
        out = g.make(name, specs[name])
        ref = np.load(os.path.join(GOLDEN, name + ".npz"))
        assert set(out) == set(ref.files)
        for k, v in out.items():
            v = np.asarray(v)
            assert np.asarray(ref[k]).dtype == v.dtype and np.asarray(ref[k]).tobytes() == v.tobytes(), (name, k)
    assert sorted(g.all_cases()) == sorted(os.path.basename(p)[:-4] for p in FILES + FR_FILES + PF_FILES)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_golden_minibatch.py"), "--check",
                        "mbnmf_tr_m25_r24_t70_tol_f32_b2", "mbnmf_fr_m25_r24_t300_bs100_tol_b0p5",
                        "mbnmf_pf_m25_r24_t150_70_110_bs100_reg_b1p5"], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.count(" same") == 3, p.stdout + p.stderr


# ---- the host pieces of the driver (csrc/evc_transform_plan.h) in a program of their own, plainly and under the sanitizers ----
SRC = os.path.join(ROOT, "tests", "transform_host_main.hip")
PKG = os.path.join(ROOT, "exemplars_vc_amd")


def _program_lines(tmp, sanitize):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = os.path.join(tmp, "transform_host_main" + ("_san" if sanitize else ""))
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
    tmp = str(tmp_path_factory.mktemp("transform_host"))
    return _program_lines(tmp, False), tmp


def test_host_carving_and_argument_checks(program):
    _lib, L = lib()
    carves = [ln.split() for ln in program[0] if ln.startswith("carve ")]
    assert len(carves) == 12 and not any("BAD" in ln for ln in program[0])
    for c in carves:
        M, R, T, n_utt, esize, shift = int(c[1]), int(c[2]), int(c[3]), int(c[4]), int(c[5]), int(c[7])
        offs = [int(v) for v in c[9:11]]
        assert offs[0] == (256 - shift) % 256 and offs == sorted(offs)
        assert offs[1] - offs[0] >= ((T + 15) // 16 + n_utt) * 16 * 2 * 8
        query = int(L.evc_online_transform_workspace_bytes(M, R, T, n_utt, _lib.F64 if esize == 8 else _lib.F32))
        assert int(c[-1]) == query and int(c[-3]) <= query
    args = {ln.split()[1]: int(ln.split()[2]) for ln in program[0] if ln.startswith("args ")}
    want = dict(ok=0, ok_exact=0, short_by_one=-2, ok_utts=0, bad_utts=-1, no_frames_no_x=0, frames_no_x=-1, struct_bytes=-1,
                max_iter_neg=-1, max_iter_0=0, max_iter_4097=0, max_iter_4098=-1, reserved=-1, init_mode=-1, beta_inf=-1,
                tol_neg=-1, tol_0=0, l2_nan=-1, init_value_inf=-1, M_528=0, M_529=-3, M_529_small_ws=-3, R_100000=0,
                nan_before_limits=-1)
    assert args == want
    fcarves = [ln.split() for ln in program[0] if ln.startswith("fcarve ")]
    assert len(fcarves) == 10
    for c in fcarves:
        M, R, T, bs, esize, shift = int(c[1]), int(c[2]), int(c[3]), int(c[4]), int(c[5]), int(c[7])
        offs = [int(v) for v in c[9:12]]
        dt = _lib.F64 if esize == 8 else _lib.F32
        assert offs[0] == (256 - shift) % 256 and offs == sorted(offs)
        assert offs[1] - offs[0] >= int(L.evc_online_workspace_bytes(M, R, T, bs, dt))
        assert int(c[-1]) == int(L.evc_online_fresh_workspace_bytes(M, R, T, bs, dt)) and int(c[-3]) <= int(c[-1])
    fargs = {ln.split()[1]: ln.split()[2:] for ln in program[0] if ln.startswith("fargs ")}
    assert {k: int(v[0]) for k, v in fargs.items()} == dict(
        ok=0, ok_exact=0, short_by_one=-2, plain_ws_is_too_small=-2, struct_bytes=-1, fresh_0=-1, fresh_4098=-1, final_neg=-1,
        final_0=0, final_4098=-1, forget_0=-1, resume=-1, fused_257=-3, R_65=0, M_529=-3, count_before_limits=-1)
    assert fargs["ok"][1:] == "fresh 30 final 200 slots 200 batch_size 32 fused 1".split()
    assert fargs["final_0"][1:] == "fresh 30 final 0 slots 30 batch_size 32 fused 1".split() and fargs["R_65"][-1] == "0"
    slots = [ln.split()[1:] for ln in program[0] if ln.startswith("slots ")]
    assert slots == [["0", "1"], ["1", "1"], ["200", "200"], ["4097", "4097"]]


def test_the_host_program_runs_clean_under_the_sanitizers(program):
    """a stand-alone program: address + undefined-behaviour sanitizers on the host code, nothing preloaded anywhere"""
    assert _program_lines(program[1], True) == program[0]


def _small():
    rng = np.random.default_rng(0)
    return rng.random((6, 4)) + 0.1, rng.random((5, 4)) + 0.1      # X, the dictionary (frames / atoms as rows)


def test_python_surface():
    import exemplars_vc_amd as evc
    X, D = _small()
    assert "transform_online" in evc.__all__
    sig = inspect.signature(evc.transform_online).parameters
    assert list(sig)[:2] == ["W", "X"]
    want = dict(beta=2.0, max_iter=200, tol=1e-4, l1=0.0, l2=0.0, H0=None, init=None, utt_offsets=None, dtype=None,
                device=None, info=False)
    assert [k for k in sig if k in want or k == "layout"] == ["beta", "layout", "max_iter", "tol", "l1", "l2", "H0", "init",
                                                              "utt_offsets", "dtype", "device", "info"]
    for k, v in want.items():
        assert sig[k].default == v and sig[k].kind is inspect.Parameter.KEYWORD_ONLY, k
    assert sig["layout"].default is inspect.Parameter.empty
    ldo = inspect.signature(evc.learn_dictionary_online).parameters
    assert {k: ldo[k].default for k in ("fresh_restarts", "fresh_restarts_max_iter", "transform_max_iter")} == dict(
        fresh_restarts=False, fresh_restarts_max_iter=30, transform_max_iter=None)
    with pytest.raises(ValueError, match="fresh_restarts_max_iter"):
        evc.learn_dictionary_online(X.T, D.T, None, layout="bin_major", fresh_restarts=True, fresh_restarts_max_iter=0)
    with pytest.raises(ValueError, match="528"):
        evc.transform_online(np.ones((2, 529)), np.ones((3, 529)), layout="frame_major")
    with pytest.raises(ValueError, match="528"):
        evc.transform_online(np.ones((529, 2)), np.ones((529, 3)), layout="bin_major")
    with pytest.raises(ValueError, match="finite"):
        evc.transform_online(D, X, beta=float("inf"), layout="frame_major")
    with pytest.raises(ValueError, match="max_iter"):
        evc.transform_online(D, X, max_iter=-1, layout="frame_major")
    import torch
    if torch.cuda.is_available():
        H = evc.transform_online(D, X, layout="frame_major", max_iter=3)
        assert H.shape == (6, 5) and np.isfinite(H).all()
    else:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            evc.transform_online(D, X, layout="frame_major", max_iter=3)


def test_estimator_surface():
    import sklearn.decomposition
    from exemplars_vc_amd.compat.minibatch import MiniBatchNMF
    X, D = _small()
    ours = inspect.signature(MiniBatchNMF.__init__).parameters
    theirs = inspect.signature(sklearn.decomposition.MiniBatchNMF.__init__).parameters
    for k, v in theirs.items():
        if k not in ("self", "init"):
            assert ours[k].default == v.default, k
    assert ours["init"].default == "custom"
    for init in (None, "nndsvd", "nndsvda", "random"):
        with pytest.raises(ValueError, match="nndsvd"):
            MiniBatchNMF(5, init=init)
    for name in ("fit_transform", "fit", "transform", "partial_fit", "inverse_transform"):
        assert callable(getattr(MiniBatchNMF, name))
    est = MiniBatchNMF(5, init="custom", beta_loss="itakura-saito", random_state=0, verbose=1)
    Xz = X.copy()
    Xz[2, 1] = 0.0
    for call in (lambda: est.fit_transform(Xz, W=np.ones((6, 5)), H=D), lambda: est.partial_fit(Xz, H=D)):
        with pytest.raises(ValueError, match="When beta_loss <= 0 and X contains zeros"):
            call()
    with pytest.raises(ValueError, match="needs H"):
        MiniBatchNMF(5).fit_transform(X, W=np.ones((6, 5)))
    with pytest.raises(ValueError, match="needs W"):
        MiniBatchNMF(5).fit_transform(X, H=D)
    with pytest.raises(RuntimeError, match="not fitted"):
        MiniBatchNMF(5).transform(X)
    with pytest.raises(AttributeError):
        MiniBatchNMF(5).components_
    with pytest.raises(ValueError, match="Invalid beta_loss"):
        MiniBatchNMF(5, beta_loss="bogus").fit_transform(X, W=np.ones((6, 5)), H=D)
