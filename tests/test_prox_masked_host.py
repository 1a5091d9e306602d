"""The missing-data proximal-gradient solve (evc_prox_masked_solve), host side: the C ABI's declarations and struct mirror, the
numpy restatement against every recorded masked deComP run (bit for bit), its options, the Python surfaces' errors and the
stand-alone host program (csrc/evc_prox_masked_plan.h), plainly and under the sanitizers.  No GPU needed."""
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
import prox_masked_restatement as pmr  # noqa: E402
import prox_restatement as pr  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ["proxm_m25_n64_t32_fista_pos", "proxm_m40_n130_t33_ista_pos", "proxm_m25_n64_t32_fista", "proxm_m1_n5_t3_fista_pos",
            "proxm_m201_n300_t20_fista_pos", "proxm_m25_n64_t32_fista_pos_k50", "proxm_m25_n64_t32_fista_pos_start"]


def lib():
    from exemplars_vc_amd import _lib
    return _lib, _lib.lib()


def load(name):
    d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    d["y"], d["A"], d["mask"] = d["y"].astype(np.float64), d["A"].astype(np.float64), d["mask"].astype(np.float64)
    d["positive"], d["momentum"] = pr.split_method(str(d["method"]))
    return d


def restate(d, offs=None, **kw):
    return pmr.solve(d["y"], d["A"], float(d["alpha"]), d.get("x0"), mask=d["mask"], tol=float(d["tol"]),
                     iters=int(d["maxiter"]), positive=d["positive"], momentum=d["momentum"], utt_offsets=offs, **kw)


# ---- the C ABI's face ----
def test_symbols_declared_and_exported():
    _lib, L = lib()
    hdr = open(os.path.join(ROOT, "include", "evc.h")).read()
    declared = set(re.findall(r"\b(evc_[a-z_0-9]+)\s*\(", hdr))
    for sym in ("evc_prox_masked_workspace_bytes", "evc_prox_masked_solve"):
        assert sym in declared and sym in _lib.SYMBOLS and hasattr(L, sym)
    assert "evc_prox_masked_solve " in hdr[:hdr.index("#ifndef EVC_H")]
    assert "enum { EVC_PROX_LIP_MEAN = 0, EVC_PROX_LIP_MAX = 1 };" in hdr
    assert (_lib.PROX_LIP_MEAN, _lib.PROX_LIP_MAX) == (0, 1)


def test_opts_mirror_matches_header():
    _lib, _ = lib()
    hdr = open(os.path.join(ROOT, "include", "evc.h")).read()

    def names_of(struct):
        body = hdr[hdr.index("typedef struct %s {" % struct):hdr.index("} %s;" % struct)]
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        return [n for grp in re.findall(r"\b(?:int|double|void\*)\s+([a-zA-Z_0-9, ]+);", body)
                for n in grp.replace(" ", "").split(",")]
    names = names_of("evc_prox_masked_opts")
    assert names == [f[0] for f in _lib.ProxMaskedOpts._fields_]
    assert [n for n in names if n not in ("lip_weights", "reserved3")] == names_of("evc_prox_opts")   # evc_prox_opts' fields plus
    assert C.sizeof(_lib.ProxMaskedOpts) == 14 * 4 + 4 * 8 + 2 * 8
    assert C.sizeof(_lib.ProxOpts) == 12 * 4 + 4 * 8 + 2 * 8                        # the existing struct did not move


def test_statuses_through_the_library():
    """the same checks as the host program's, through the shared library: before any device work, in the statuses' order"""
    _lib, L = lib()
    one = C.c_void_p(8)              # never dereferenced: every case fails validation first

    def opts(**kw):
        o = _lib.ProxMaskedOpts()
        o.struct_bytes = C.sizeof(o)
        o.dtype, o.layout, o.iters = _lib.F64, _lib.FRAME_MAJOR, 100
        o.mode, o.momentum, o.normalize, o.check_every = _lib.PROX_POSITIVE, _lib.PROX_FISTA, 1, 10
        o.stop_rule, o.init_mode, o.alpha, o.tol = _lib.STOP_DECOMP, _lib.INIT_CONST, 1e-3, 1e-3
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def call(o, M=25, N=17, T=70, lda=25, ldx=25, ldm=25, ldh=17, ws=16, A=one, X=one, mask=one, H=one, wsp=one):
        return L.evc_prox_masked_solve(A, lda, X, ldx, mask, ldm, H, ldh, M, N, T, None, 1, None if o is None else C.byref(o),
                                       wsp, ws, None, None, None)
    assert call(opts()) == -2 and call(opts(), mask=None, ldm=0) == -2 and call(None) == -1
    assert call(opts(), ldm=24) == -1 and call(opts(), ldm=40) == -2
    assert call(opts(layout=_lib.BIN_MAJOR), lda=17, ldx=70, ldm=69, ldh=70) == -1
    assert call(opts(layout=_lib.BIN_MAJOR), lda=17, ldx=70, ldm=70, ldh=70) == -2
    assert call(opts(lip_weights=2)) == -1 and call(opts(lip_weights=_lib.PROX_LIP_MAX)) == -2
    assert call(opts(reserved3=1)) == -1 and call(opts(struct_bytes=C.sizeof(_lib.ProxOpts))) == -1
    for p in ("A", "X", "H", "wsp"):
        assert call(opts(), **{p: None}) == -1
    assert call(opts(), T=0, X=None, H=None, mask=None) == -2
    assert call(opts(), M=1057, lda=1057, ldx=1057, ldm=1057) == -3 and call(opts(), N=16385, ldh=16385) == -3
    assert call(opts(), M=1057, lda=1057, ldx=1057, ldm=1056) == -1 and call(opts(lip_weights=5), N=16385, ldh=16385) == -1
    assert call(opts(), ws=int(L.evc_prox_masked_workspace_bytes(25, 17, 70, 1, _lib.F64)) - 1) == -2


def test_workspace_query_has_no_square_term():
    _lib, L = lib()
    q = L.evc_prox_masked_workspace_bytes
    assert q(1057, 64, 100, 1, 0) == 0 and q(25, 16385, 100, 1, 0) == 0 and q(0, 64, 100, 1, 0) == 0
    assert q(25, 64, -1, 1, 0) == 0 and q(25, 64, 100, 0, 0) == 0 and q(25, 64, 100, 1, 9) == 0
    assert q(1056, 64, 100, 1, 0) > 0 and q(25, 64, 0, 1, 1) > 0
    assert q(25, 64, 688, 1, _lib.F32) < q(25, 64, 688, 1, _lib.F64) < q(201, 64, 688, 1, _lib.F64)
    ru = lambda v, m: -(-v // m) * m      # noqa: E731
    for M, N, T, n, dt, es in ((25, 64, 32, 1, _lib.F64, 8), (25, 4096, 11008, 16, _lib.F32, 4), (40, 130, 33, 2, _lib.F64, 8),
                               (25, 16384, 688, 1, _lib.F64, 8)):
        own = (ru(N, 16) * ru(M, 128) + ru(M, 16) * ru(N, 128) + 3 * N * T + 2 * M * T + 3 * N + n * (N + M + 1) + T) * es \
            + ru(N, 128) // 64 * T * 8 + T * 4 + n * (4097 * 8 + 8) + 4
        assert own <= int(q(M, N, T, n, dt)) <= own + 21 * 256
    # it grows as N (M + T): doubling N doubles it where evc_prox_solve's, with its Gram matrix, quadruples
    a, b = int(q(25, 8192, 64, 1, _lib.F64)), int(q(25, 16384, 64, 1, _lib.F64))
    assert b < 2.1 * a and b < (1 << 27) < (2 << 30) <= int(L.evc_prox_workspace_bytes(25, 16384, 64, 1, _lib.F64))
    assert int(L.evc_prox_workspace_bytes(25, 17, 70, 1, _lib.F64)) > 0               # the existing query did not move away


# ---- the restatement against every recorded deComP run, bit for bit ----
def same_run(x, ref, d):
    """Bit for bit where this machine's BLAS sums the fixture's products as the recording machine's did (`blas_crc`,
    pmr.blas_fingerprint); elsewhere within 100 x the fixture's permutation figure of max |x|."""
    if pmr.blas_fingerprint(d["y"], d["A"], d["mask"]) == d["blas_crc"].tolist():
        return np.array_equal(x, ref)
    worst = float(np.max(np.abs(x - ref)) / np.max(np.abs(ref)))
    print("another BLAS summation order here: max error %.3e of max |x| (allowed %.3e)" % (worst, 100 * float(d["perm64"])))
    return worst <= 100 * float(d["perm64"])


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_reproduces_decomp(name):
    d = load(name)
    x, n_iter, tr = restate(d)
    assert same_run(x, d["x"], d) and int(n_iter[0]) == int(d["it"]) + 1
    assert x.dtype == np.float64 and tr.shape == (1, pr.n_slots(int(d["maxiter"]), 10))
    if d["positive"]:
        assert (x >= 0).all()
    assert x.any() and (x == 0).any()
    if float(d["tol"]) > 0:                                         # no stop decision sits on its threshold
        done = tr[0][np.isfinite(tr[0])]
        assert np.min(np.abs(done)) >= 1e-6 * float(d["tol"])
    if "offs" in d:
        offs = d["offs"].tolist()
        xs, ns, trs = restate(d, offs)
        assert same_run(xs, d["x_split"], d) and np.array_equal(ns, d["it_split"] + 1)
        for u in range(len(offs) - 1):                              # a batch is one call per utterance
            sub = dict(d, y=d["y"][offs[u]:offs[u + 1]], mask=d["mask"][offs[u]:offs[u + 1]])
            xu, nu, tu = restate(sub)
            assert np.array_equal(xu, xs[offs[u]:offs[u + 1]]) and nu[0] == ns[u] and np.array_equal(tu[0], trs[u], equal_nan=True)


def test_fixture_set_is_what_the_tests_need():
    kinds = {name: load(name) for name in FIXTURES}
    batches = [d for d in kinds.values() if "offs" in d]
    assert len(batches) == 3 and any(len(set(d["it_split"].tolist())) > 1 for d in batches)
    assert sum(1 for d in kinds.values() if "x0" in d) == 1 and sum(1 for d in kinds.values() if not d["positive"]) == 1
    assert sorted(int(d["maxiter"]) for d in kinds.values() if float(d["tol"]) == 0) == [50]
    assert {str(d["kind"]) for d in kinds.values()} == {"binary", "weights"}
    signed = kinds["proxm_m25_n64_t32_fista"]
    assert (signed["A"] < 0).any() and (signed["y"] < 0).any() and (signed["x"] < 0).any()
    for name, d in kinds.items():
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 300 * 1024
        assert 0 < float(d["perm64"]) < 1e-6 and 0 < float(d["perm32"]) < 1e-1
        assert d["mask"].shape == d["y"].shape and (d["mask"] >= 0).all() and (d["mask"] == 0).any() and (d["mask"] > 0).any()
        assert np.array_equal(d["mask"], d["mask"].astype(np.float32)) and d["x"].any()
        assert (str(d["kind"]) == "binary") == bool(np.isin(d["mask"], (0.0, 1.0)).all())


def test_restatement_options():
    y, A = pr.problem(25, 33, 40, 3)
    mask = pmr.problem_mask(40, 25, 3, "binary")
    # a null mask is prox_restatement itself, bit for bit
    for kw in (dict(), dict(normalize=False), dict(positive=False, momentum="ista"), dict(utt_offsets=[0, 20, 20, 40])):
        a, b = pmr.solve(y, A, 1e-3, iters=30, tol=1e-3, **kw), pr.solve(y, A, 1e-3, iters=30, tol=1e-3, **kw)
        assert all(np.array_equal(u, v, equal_nan=True) for u, v in zip(a, b))
    # a mask of ones is the unmasked problem in the factored summation order
    ones, _, _ = pmr.solve(y, A, 1e-3, mask=np.ones_like(y), iters=30, tol=0.0)
    base, _, _ = pr.solve(y, A, 1e-3, iters=30, tol=0.0)
    assert np.max(np.abs(ones - base)) < 1e-12 and not np.array_equal(ones, base)
    # lip_weights "max" on a binary mask that is constant over the utterance: the problem with the masked bins deleted
    keep = mask[0] > 0
    const = np.tile(mask[0], (40, 1))
    got, n1, t1 = pmr.solve(y, A, 1e-3, mask=const, iters=30, tol=1e-3, normalize=False, lip_weights="max")
    red, n2, t2 = pr.solve(y[:, keep], A[:, keep], 1e-3, iters=30, tol=1e-3, normalize=False)
    np.testing.assert_allclose(got, red, rtol=0, atol=1e-13 * np.abs(red).max())
    assert n1.tolist() == n2.tolist() and red.any() and 0 < keep.sum() < 25
    mean, _, _ = pmr.solve(y, A, 1e-3, mask=const, iters=30, tol=1e-3, normalize=False, lip_weights="mean")
    np.testing.assert_allclose(mean, red, rtol=0, atol=1e-13 * np.abs(red).max())     # a constant mask: its mean is its maximum
    # on a mask that varies, the maximum is the larger bound, and an explicit lipschitz replaces both
    Lmean, Lmax = pmr.lipschitz_of(A, mask, lip_weights="mean"), pmr.lipschitz_of(A, mask, lip_weights="max")
    assert 0 < Lmean < Lmax
    for lw, Lw in (("mean", Lmean), ("max", Lmax)):
        a = pmr.solve(y, A, 1e-3, mask=mask, iters=20, tol=0.0, lip_weights=lw)[0]
        b = pmr.solve(y, A, 1e-3, mask=mask, iters=20, tol=0.0, lipschitz=Lw, lip_weights="mean")[0]
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        pmr.solve(y, A, 1e-3, mask=mask, iters=3, lip_weights="median")
    # float32 mode, an empty utterance, iters = 0, an utterance whose mask is all zero
    x32, _, _ = pmr.solve(y, A, 1e-3, mask=mask, iters=30, tol=0.0, dtype=np.float32, lip_weights="max")
    x64, _, _ = pmr.solve(y, A, 1e-3, mask=mask, iters=30, tol=0.0, lip_weights="max")
    assert x32.dtype == np.float32 and np.max(np.abs(x32 - x64)) < 1e-3
    xs, ns, ts = pmr.solve(y, A, 1e-3, mask=mask, iters=20, tol=1e-3, utt_offsets=[0, 20, 20, 40])
    assert ns[1] == 20 and np.isnan(ts[1]).all() and np.isfinite(ts[0, 0])
    x0 = np.full((40, 33), 0.25)
    assert np.array_equal(pmr.solve(y, A, 1e-3, x0, mask=mask, iters=0)[0], x0)
    zero = mask.copy()
    zero[20:] = 0.0
    xz, nz, tz = pmr.solve(y, A, 1e-3, mask=zero, iters=12, tol=1e-3, utt_offsets=[0, 20, 40])
    assert np.isnan(xz[20:]).all() and np.isfinite(xz[:20]).all() and nz.tolist()[1] == 12 and np.isnan(tz[1, :2]).all()
    # the generator
    for kind in ("binary", "weights"):
        m = pmr.problem_mask(9, 7, 1, kind)
        assert m.shape == (9, 7) and (m >= 0).all() and m[0, 0] == 0 and m[0, 1] == 1 and np.array_equal(m, m.astype(np.float32))
    assert 0.5 < pmr.problem_mask(200, 50, 2, "binary", keep=0.7).mean() < 0.9
    with pytest.raises(ValueError):
        pmr.problem_mask(3, 3, 0, "gaussian")


# ---- the Python surfaces ----
def test_solve_activations_prox_rejects_a_bad_mask_before_any_device(monkeypatch):
    import exemplars_vc_amd as evc
    from exemplars_vc_amd import solver
    sig = inspect.signature(evc.solve_activations_prox).parameters
    for k, dflt in (("mask", None), ("factored", False), ("lip_weights", "max")):
        assert sig[k].kind is inspect.Parameter.KEYWORD_ONLY and sig[k].default == dflt, k
    monkeypatch.setattr(solver, "require_device", lambda device=None: pytest.fail("a device was asked for"))
    Ab, Xb = np.ones((4, 5)), np.ones((4, 3))
    with pytest.raises(ValueError, match="mask has shape"):
        evc.solve_activations_prox(Ab, Xb, alpha=1e-3, mask=np.ones((3, 4)))
    with pytest.raises(ValueError, match="mask has shape"):
        evc.solve_activations_prox(Ab, Xb, alpha=1e-3, mask=np.ones(4))
    for bad in (-1.0, np.nan, np.inf):
        m = np.ones((4, 3))
        m[2, 1] = bad
        with pytest.raises(ValueError, match="finite weights >= 0"):
            evc.solve_activations_prox(Ab, Xb, alpha=1e-3, mask=m)
        with pytest.raises(ValueError, match="finite weights >= 0"):
            evc.convert_prox(Ab, np.ones((9, 5)), Xb, alpha=1e-3, mask=m)
    with pytest.raises(ValueError, match="finite weights >= 0"):
        evc.solve_activations_prox(Ab, Xb, alpha=1e-3, mask=np.ones((4, 3), dtype=complex))
    with pytest.raises(ValueError, match="lip_weights"):
        evc.solve_activations_prox(Ab, Xb, alpha=1e-3, mask=np.ones((4, 3)), lip_weights="median")


def test_a_good_mask_reaches_the_device_or_raises_without_one():
    import torch
    import exemplars_vc_amd as evc
    Ab, Xb = np.ones((4, 5)), np.ones((4, 3))
    if torch.cuda.is_available():
        for kw in (dict(mask=np.ones((4, 3))), dict(factored=True)):
            H = evc.solve_activations_prox(Ab, -Xb, alpha=1e-3, iters=3, **kw)
            assert H.shape == (5, 3) and not H.any()                  # A^T X < 0: the threshold cuts everything
    else:
        for kw in (dict(mask=np.ones((4, 3))), dict(factored=True)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                evc.solve_activations_prox(Ab, Xb, alpha=1e-3, **kw)


def test_compat_decomp_masks(monkeypatch):
    from exemplars_vc_amd.compat import decomp
    calls = []

    def fake(A, X, H0=None, **kw):
        calls.append((A, X, H0, kw))
        return np.zeros((X.shape[0], A.shape[0]), dtype=X.dtype), {"n_iter": np.array([7], dtype=np.int32)}
    monkeypatch.setattr(decomp, "solve_activations_prox", fake)
    y, A = np.ones((2, 3, 4)), np.ones((5, 4))
    mask = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    for method, positive, momentum in (("ista", False, "ista"), ("fista", False, "fista"), ("ista_pos", True, "ista"),
                                       ("fista_pos", True, "fista")):
        it, x = decomp.lasso.solve(y, A, 1e-3, method=method, mask=mask, maxiter=50)
        kw = calls[-1][3]
        assert it == 6 and x.shape == (2, 3, 5)
        assert kw["mask"].shape == (6, 4) and kw["mask"].dtype == np.float64 and np.array_equal(kw["mask"], mask.reshape(6, 4))
        assert kw["lip_weights"] == "mean" and kw["positive"] is positive and kw["momentum"] == momentum and kw["normalize"]
        assert kw["layout"] == "frame_major" and calls[-1][1].shape == (6, 4)
    decomp.nnls.solve(y, A, 1e-3, method="fista", mask=mask.astype(np.float64))
    assert calls[-1][3]["positive"] is True and "mask" in calls[-1][3]
    decomp.lasso.solve(y, A, 1e-3)                                    # without a mask: the call of before, no new keyword
    assert "mask" not in calls[-1][3] and "lip_weights" not in calls[-1][3] and "factored" not in calls[-1][3]
    n = len(calls)
    with pytest.raises(NotImplementedError, match="mask"):
        decomp.lasso.solve(y, A, 1e-3, mask=np.ones(4))               # 1-D: weights per bin
    with pytest.raises(NotImplementedError, match="not mirrored"):
        decomp.lasso.solve(y, A, 1e-3, method="acc_ista", mask=mask)
    with pytest.raises(NotImplementedError, match="complex"):
        decomp.lasso.solve(y.astype(complex), A.astype(complex), 1e-3, mask=mask)
    neg = mask.copy()
    neg[1, 2, 3] = -1.0
    with pytest.raises(AssertionError):
        decomp.lasso.solve(y, A, 1e-3, mask=neg)
    with pytest.raises(ValueError, match="Data type"):
        decomp.lasso.solve(y, A, 1e-3, mask=np.ones((2, 3, 4), dtype=np.int64))
    with pytest.raises(ValueError, match="Data type"):
        decomp.lasso.solve(y, A, 1e-3, mask=np.ones((2, 3, 4), dtype=complex))
    with pytest.raises(ValueError, match="mask has shape"):
        decomp.lasso.solve(y, A, 1e-3, mask=np.ones((3, 2, 4)))
    assert len(calls) == n                                            # none of them reached the native call
    assert "mask" in decomp.__doc__ and "1-D" in decomp.__doc__


# ---- the host pieces of the driver (csrc/evc_prox_masked_plan.h) in a program of their own, plainly and under the sanitizers ----
SRC = os.path.join(ROOT, "tests", "prox_masked_host_main.hip")
PKG = os.path.join(ROOT, "exemplars_vc_amd")


def _program_lines(tmp, sanitize):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = os.path.join(tmp, "prox_masked_host_main" + ("_san" if sanitize else ""))
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
    tmp = str(tmp_path_factory.mktemp("prox_masked_host"))
    return _program_lines(tmp, False), tmp


def test_host_carving_and_argument_checks(program):
    _lib, L = lib()
    carves = [ln.split() for ln in program[0] if ln.startswith("carve ")]
    assert len(carves) == 12 and not any("BAD" in ln for ln in program[0])
    for c in carves:
        M, N, T, n_utt, esize, shift = (int(v) for v in c[1:6] + [c[7]])
        offs = [int(v) for v in c[9:28]]
        assert len(offs) == 19 and c[28] == "bytes"
        assert offs[0] == (256 - shift) % 256 and offs == sorted(offs) and all((o + shift) % 256 == 0 for o in offs)
        query = int(L.evc_prox_masked_workspace_bytes(M, N, T, n_utt, _lib.F64 if esize == 8 else _lib.F32))
        assert int(c[-1]) == query and int(c[-3]) <= query <= int(c[-3]) + 512
    # nothing N x N: at N = 16384 the whole workspace is smaller than evc_prox_solve's Gram matrix alone
    big = [c for c in carves if c[2] == "16384"][0]
    assert int(big[-1]) < 16384 * 16384 * 8 // 3
    args = {ln.split()[1]: int(ln.split()[2]) for ln in program[0] if ln.startswith("args ")}
    want = dict(ok=0, ok_exact=0, short_by_one=-2, f32_ws=-2, ok_utts=0, bad_utts=-1, no_frames_no_x=0, frames_no_x=-1,
                no_mask=0, no_mask_any_ldm=0, ldm_short=-1, ldm_padded=0, ldm_short_bin_major=-1,
                struct_bytes=-1, iters_neg=-1, iters_0=0, slots_4097=0, slots_4098=-1, no_checks_many_iters=0,
                check_every_neg=-1, reserved=-1, reserved2=-1, reserved3=-1, lip_weights=-1, lip_weights_neg=-1,
                lip_weights_max=0, mode=-1, mode_signed=0, momentum=-1, momentum_nesterov=0,
                normalize=-1, normalize_0=0, init_sklearn=-1, init_given=0, stop_sklearn=-1, stop_pymf=-1, stop_none=0,
                tol_neg=-1, tol_0=0, tol_inf=-1, alpha_neg=-1, alpha_0=0, alpha_nan=-1, lipschitz_neg=-1, lipschitz_set=0,
                lipschitz_inf=-1, init_value_inf=-1, dtype=-1, layout=-1, M_1056=0, M_1057=-3, M_1057_small_ws=-3, N_16384=0,
                N_16384_small_ws=-2, N_16385=-3, N_16385_small_ws=-3, nan_before_limits=-1, reserved_before_limits=-1,
                lip_weights_before_limits=-1, ldm_before_limits=-1)
    assert args == want
    # the wavefronts per workgroup: prox_waves' rule on each kernel's own rows
    waves = {tuple(int(v) for v in ln.split()[1:4]): tuple(int(v) for v in ln.split()[4:6]) for ln in program[0]
             if ln.startswith("waves ")}
    for (M, N, T), (wr, wb) in waves.items():
        fb = -(-T // 64)
        assert wr == (8 if fb * (-(-M // 128)) >= 512 else 4) and wb == (8 if fb * (-(-N // 128)) >= 512 else 4), (M, N, T)
    assert waves[(25, 4096, 11008)] == (4, 8) and waves[(513, 4096, 11008)] == (8, 8) and waves[(25, 4096, 688)] == (4, 4)
    slots = {(int(ln.split()[1]), int(ln.split()[2])): int(ln.split()[3]) for ln in program[0] if ln.startswith("slots ")}
    assert len(slots) == 10
    for (iters, ce), n in slots.items():
        assert n == pr.n_slots(iters, ce), (iters, ce)
    # both dictionary images: whole k-slabs of 16 rows, whole row blocks of 128 columns, every slab load inside them
    pads = {tuple(int(v) for v in ln.split()[1:3]): [int(v) for v in ln.split()[3:]] for ln in program[0] if ln.startswith("pad ")}
    sizes = (1, 15, 16, 17, 128, 129)
    assert sorted(pads) == sorted((M, N) for M in sizes for N in sizes)
    ru = lambda v, m: -(-v // m) * m      # noqa: E731
    for (M, N), p in pads.items():
        assert p == [ru(N, 16), ru(M, 128), ru(M, 16), ru(N, 128)]
    assert sum(1 for ln in program[0] if ln.startswith("image ") and ln.endswith(" ok")) == 36


def test_the_host_program_runs_clean_under_the_sanitizers(program):
    """a stand-alone program: address + undefined-behaviour sanitizers on the host code, nothing preloaded anywhere"""
    assert _program_lines(program[1], True) == program[0]
