"""The proximal-gradient activation solve (evc_prox_solve), host side: the C ABI's declarations, struct mirror, status codes
and their order, the workspace query, the numpy restatement against every recorded deComP run (bit for bit), the momentum
schedules, the Python surface's errors and the stand-alone host program (csrc/evc_prox_plan.h), plainly and under the
sanitizers.  No GPU needed."""
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
import prox_restatement as pr  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ["prox_m25_n64_t32_fista_pos", "prox_m40_n130_t33_ista_pos", "prox_m25_n64_t32_fista", "prox_m1_n5_t3_fista_pos",
            "prox_m201_n300_t20_fista_pos", "prox_m25_n64_t32_fista_pos_k50", "prox_m25_n64_t32_fista_pos_k100",
            "prox_m25_n64_t32_nnls_ista", "prox_m25_n64_t32_fista_pos_start"]


def lib():
    from exemplars_vc_amd import _lib
    return _lib, _lib.lib()


def load(name):
    d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    d["y"], d["A"] = d["y"].astype(np.float64), d["A"].astype(np.float64)
    d["positive"], d["momentum"] = pr.split_method(str(d["method"]))
    return d


def restate(d, offs=None, **kw):
    return pr.solve(d["y"], d["A"], float(d["alpha"]), d.get("x0"), tol=float(d["tol"]), iters=int(d["maxiter"]),
                    positive=d["positive"], momentum=d["momentum"], utt_offsets=offs, **kw)


def test_symbols_declared_and_exported():
    _lib, L = lib()
    hdr = open(os.path.join(ROOT, "include", "evc.h")).read()
    declared = set(re.findall(r"\b(evc_[a-z_0-9]+)\s*\(", hdr))
    for sym in ("evc_prox_workspace_bytes", "evc_prox_solve"):
        assert sym in declared and sym in _lib.SYMBOLS and hasattr(L, sym)
    assert "evc_prox_solve " in hdr[:hdr.index("#ifndef EVC_H")]
    # the new stop rule is an addition: the existing values did not move
    assert "enum { EVC_STOP_NONE = 0, EVC_STOP_SKLEARN = 1, EVC_STOP_PYMF = 2, EVC_STOP_DECOMP = 3 };" in hdr
    assert (_lib.STOP_NONE, _lib.STOP_SKLEARN, _lib.STOP_PYMF, _lib.STOP_DECOMP) == (0, 1, 2, 3)
    assert "enum { EVC_PROX_POSITIVE = 0, EVC_PROX_SIGNED = 1 };" in hdr
    assert "enum { EVC_PROX_ISTA = 0, EVC_PROX_FISTA = 1, EVC_PROX_NESTEROV = 2 };" in hdr
    assert (_lib.PROX_POSITIVE, _lib.PROX_SIGNED, _lib.PROX_ISTA, _lib.PROX_FISTA, _lib.PROX_NESTEROV) == (0, 1, 0, 1, 2)


def test_opts_mirror_matches_header():
    _lib, _ = lib()
    hdr = open(os.path.join(ROOT, "include", "evc.h")).read()
    body = hdr[hdr.index("typedef struct evc_prox_opts {"):hdr.index("} evc_prox_opts;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for grp in re.findall(r"\b(?:int|double|void\*)\s+([a-zA-Z_0-9, ]+);", body)
             for n in grp.replace(" ", "").split(",")]
    assert names == [f[0] for f in _lib.ProxOpts._fields_]
    assert names == ["struct_bytes", "dtype", "layout", "iters", "mode", "momentum", "normalize", "check_every", "stop_rule",
                     "init_mode", "reserved", "reserved2", "alpha", "tol", "init_value", "lipschitz", "ev_loop_start",
                     "ev_loop_stop"]
    assert C.sizeof(_lib.ProxOpts) == 12 * 4 + 4 * 8 + 2 * 8
    # the existing structs did not move
    assert C.sizeof(_lib.SemiOpts) == 8 * 4 + 3 * 8 + 2 * 8 and C.sizeof(_lib.BetaOpts) == 8 * 4 + 5 * 8 + 2 * 8


def _opts(_lib, **kw):
    o = _lib.ProxOpts()
    o.struct_bytes = C.sizeof(_lib.ProxOpts)
    o.dtype, o.layout, o.iters = _lib.F64, _lib.FRAME_MAJOR, 100
    o.mode, o.momentum, o.normalize, o.check_every = _lib.PROX_POSITIVE, _lib.PROX_FISTA, 1, 10
    o.stop_rule, o.init_mode, o.alpha, o.tol = _lib.STOP_DECOMP, _lib.INIT_CONST, 1e-3, 1e-3
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_status_codes_and_their_order():
    _lib, L = lib()
    one = C.c_void_p(8)              # never dereferenced: every case fails validation first

    def call(o, M=25, N=17, T=70, lda=25, ldx=25, ldh=17, ws=16, A=one, X=one, H=one, wsp=one, offs=None, n_utt=1):
        po = None if offs is None else (C.c_int * len(offs))(*offs)
        return L.evc_prox_solve(A, lda, X, ldx, H, ldh, M, N, T, po, n_utt, None if o is None else C.byref(o), wsp, ws, None,
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
    for f in ("tol", "alpha", "lipschitz"):
        for v in (-1e-12, float("nan"), float("inf")):
            assert call(_opts(_lib, **{f: v})) == -1, (f, v)
        assert call(_opts(_lib, **{f: 0.0})) == -2 and call(_opts(_lib, **{f: 2.5})) == -2
    for v in (float("nan"), float("inf")):
        assert call(_opts(_lib, init_value=v)) == -1
    assert call(_opts(_lib, init_mode=_lib.INIT_SKLEARN)) == -1 and call(_opts(_lib, init_mode=3)) == -1
    assert call(_opts(_lib, init_mode=_lib.INIT_GIVEN)) == -2
    assert call(_opts(_lib, stop_rule=_lib.STOP_SKLEARN)) == -1 and call(_opts(_lib, stop_rule=_lib.STOP_PYMF)) == -1
    assert call(_opts(_lib, stop_rule=4)) == -1 and call(_opts(_lib, stop_rule=_lib.STOP_NONE)) == -2
    assert call(_opts(_lib, mode=2)) == -1 and call(_opts(_lib, mode=-1)) == -1 and call(_opts(_lib, mode=_lib.PROX_SIGNED)) == -2
    assert call(_opts(_lib, momentum=3)) == -1 and call(_opts(_lib, momentum=-1)) == -1
    assert call(_opts(_lib, momentum=_lib.PROX_ISTA)) == -2 and call(_opts(_lib, momentum=_lib.PROX_NESTEROV)) == -2
    assert call(_opts(_lib, normalize=2)) == -1 and call(_opts(_lib, normalize=0)) == -2
    assert call(_opts(_lib, dtype=7)) == -1 and call(_opts(_lib, layout=5)) == -1
    assert call(_opts(_lib, reserved=1)) == -1 and call(_opts(_lib, reserved2=1)) == -1
    assert call(_opts(_lib, iters=-1)) == -1 and call(_opts(_lib, check_every=-1)) == -1
    assert call(_opts(_lib, iters=0)) == -2 and call(_opts(_lib, dtype=_lib.F32)) == -2
    assert call(_opts(_lib, iters=4097, check_every=1)) == -2 and call(_opts(_lib, iters=4098, check_every=1)) == -1
    assert call(_opts(_lib, iters=40970, check_every=10)) == -2 and call(_opts(_lib, iters=40971, check_every=10)) == -1
    assert call(_opts(_lib, iters=1000000, check_every=0)) == -2                       # no checks, no slots
    assert call(_opts(_lib), ws=int(L.evc_prox_workspace_bytes(25, 17, 70, 1, _lib.F64)) - 1) == -2
    # beyond the limits: -3, after every -1 and before -2, even with a tiny workspace
    assert call(_opts(_lib), M=1057, lda=1057, ldx=1057) == -3 and call(_opts(_lib), N=16385, ldh=16385) == -3
    assert call(_opts(_lib), M=1057, lda=1057, ldx=1057, ws=1 << 40) == -3
    assert call(_opts(_lib), N=16385, ldh=16385, ws=1 << 40) == -3
    assert call(_opts(_lib), M=1056, lda=1056, ldx=1056) == -2 and call(_opts(_lib), N=16384, ldh=16384) == -2
    assert call(_opts(_lib, tol=float("nan")), M=1057, lda=1057, ldx=1057) == -1
    assert call(_opts(_lib, reserved=4), N=16385, ldh=16385) == -1
    assert call(_opts(_lib, iters=4098, check_every=1), N=16385, ldh=16385) == -1
    assert call(_opts(_lib), M=1057, lda=1057, ldx=1057, X=None) == -1
    assert call(_opts(_lib), N=16385, ldh=16384) == -1


def test_workspace_query():
    _lib, L = lib()
    q = L.evc_prox_workspace_bytes
    assert q(1057, 64, 100, 1, 0) == 0 and q(25, 16385, 100, 1, 0) == 0
    assert q(0, 64, 100, 1, 0) == 0 and q(25, 0, 100, 1, 0) == 0 and q(25, 64, -1, 1, 0) == 0
    assert q(25, 64, 100, 0, 0) == 0 and q(25, 64, 100, 1, 9) == 0
    assert q(1056, 64, 100, 1, 0) > 0 and q(25, 64, 0, 1, 1) > 0
    assert q(25, 64, 688, 1, 0) < q(25, 129, 688, 1, 0) < q(25, 4096, 688, 1, 0) < q(25, 4096, 6880, 1, 0) < q(25, 4096, 6880, 10, 0)
    assert q(25, 64, 688, 1, _lib.F32) < q(25, 64, 688, 1, _lib.F64) and q(25, 64, 688, 1, 0) == q(201, 64, 688, 1, 0)
    # G (padded to whole row blocks of 128), P, the two W, four vectors over N, the shares of the statistic per 64 rows
    # and frame, the per-frame and per-utterance state
    for M, N, T, n, dt, es in ((25, 64, 32, 1, _lib.F64, 8), (25, 4096, 11008, 16, _lib.F32, 4), (40, 130, 33, 2, _lib.F64, 8)):
        NP = -(-N // 128) * 128
        own = NP * NP * es + 3 * N * T * es + (4 * N + 1) * es + NP // 64 * T * 8 + T * 4 + n * (4097 * 8 + 8) + 4
        assert own <= int(q(M, N, T, n, dt)) <= own + 15 * 256
    assert 2 << 30 <= int(q(25, 16384, 688, 1, _lib.F64)) < (2 << 30) + (1 << 29)          # the 2 GiB Gram matrix
    # the existing queries did not move
    assert int(L.evc_beta_workspace_bytes(25, 24, 70, 1, _lib.F64)) == 76800


# ---- the restatement against every recorded deComP run, bit for bit ----
def same_run(x, ref, d):
    """Bit for bit where this machine's BLAS sums the fixture's products as the recording machine's did (`blas_crc`,
    pr.blas_fingerprint).  Elsewhere deComP itself would not reproduce its recorded bits: there the restatement is held to
    the bound of another summation order, 100 x the fixture's permutation figure of max |x| (tests/test_gpu_prox.py)."""
    if pr.blas_fingerprint(d["y"], d["A"]) == d["blas_crc"].tolist():
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
    frac = float(np.mean(x != 0))
    print(name, "it", int(d["it"]), "non-zero", frac)
    assert 0.05 < frac < 0.9 and (x == 0).any()                     # real zeros, and not only zeros
    if float(d["tol"]) > 0:                                         # no stop decision sits on its threshold
        done = tr[0][np.isfinite(tr[0])]
        assert np.min(np.abs(done)) >= 1e-6 * float(d["tol"])
        stopped = int(n_iter[0]) < int(d["maxiter"]) or done[-1] < 0
        assert (done[:-1] >= 0).all() and (done[-1] < 0) == stopped
    if "offs" in d:
        offs = d["offs"].tolist()
        xs, ns, trs = restate(d, offs)
        assert same_run(xs, d["x_split"], d) and np.array_equal(ns, d["it_split"] + 1)
        assert len(set(d["it_split"].tolist())) > 1                 # the utterances stop at different iterations
        for u in range(len(offs) - 1):                              # a batch is one call per utterance
            sub = dict(d, y=d["y"][offs[u]:offs[u + 1]])
            xu, nu, tu = restate(sub)
            assert np.array_equal(xu, xs[offs[u]:offs[u + 1]]) and nu[0] == ns[u] and np.array_equal(tu[0], trs[u], equal_nan=True)


def test_fixture_set_is_what_the_tests_need():
    kinds = {name: load(name) for name in FIXTURES}
    assert sum(1 for d in kinds.values() if "offs" in d) == 3 and sum(1 for d in kinds.values() if bool(d["nnls"])) == 1
    assert sum(1 for d in kinds.values() if "x0" in d) == 1 and sum(1 for d in kinds.values() if not d["positive"]) == 1
    assert sorted(int(d["maxiter"]) for d in kinds.values() if float(d["tol"]) == 0) == [50, 100]
    signed = kinds["prox_m25_n64_t32_fista"]
    assert (signed["A"] < 0).any() and (signed["y"] < 0).any() and (signed["x"] < 0).any()
    assert 100 * float(signed["perm64"]) <= 1e-6                     # the signed fixture is conditioned well enough
    for name, d in kinds.items():
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 300 * 1024
        assert 0 < float(d["perm64"]) < 1e-8 and 0 < float(d["perm32"]) < 1e-2


def test_momentum_schedules_against_a_literal_loop():
    assert pr.schedule("ista", 5) == [0.0] * 5
    assert pr.schedule("nesterov", 6) == [0 / 3, 1 / 4, 2 / 5, 3 / 6, 4 / 7, 5 / 8]
    beta, want = 1.0, []
    for _ in range(50):
        beta_new = 0.5 * (1.0 + np.sqrt(1.0 + 4.0 * beta * beta))
        want.append((beta - 1.0) / beta_new)
        beta = beta_new
    got = pr.schedule("fista", 50)
    assert got == [float(w) for w in want] and got[0] == 0.0 and all(0 <= a < b < 1 for a, b in zip(got, got[1:]))
    with pytest.raises(ValueError):
        pr.schedule("adam", 3)
    assert [pr.n_slots(i, c) for i, c in ((0, 10), (1, 10), (10, 10), (11, 10), (300, 10), (301, 10), (5, 0), (7, 1))] == \
        [0, 1, 1, 2, 30, 31, 0, 7]


def test_restatement_options():
    y, A = pr.problem(25, 33, 40, 3)
    base, n0, t0 = pr.solve(y, A, 1e-3, iters=30, tol=0.0)
    assert n0.tolist() == [30] and t0.shape == (1, 3) and (t0 >= 0).all()
    # an override of the step by the bound itself changes nothing; a larger L takes smaller steps
    G = (A / np.linalg.norm(A, axis=1, keepdims=True))
    L = float(np.max(np.sum(np.abs(G @ G.T), axis=0)))
    same, _, _ = pr.solve(y, A, 1e-3, iters=30, tol=0.0, lipschitz=L)
    slow, _, _ = pr.solve(y, A, 1e-3, iters=30, tol=0.0, lipschitz=4 * L)
    assert np.allclose(same, base, rtol=0, atol=1e-12) and not np.allclose(slow, base, rtol=0, atol=1e-6)
    # without the scaling the penalty is alpha itself: a large one leaves nothing
    none, _, _ = pr.solve(y, A, 1e3, iters=5, tol=0.0, normalize=False)
    assert not none.any()
    plain, _, _ = pr.solve(y, A, 1e-3, iters=30, tol=0.0, normalize=False)
    assert plain.any() and (plain >= 0).all() and (plain == 0).any()
    x32, _, _ = pr.solve(y, A, 1e-3, iters=30, tol=0.0, dtype=np.float32)
    assert x32.dtype == np.float32 and np.max(np.abs(x32 - base)) < 1e-4
    # an empty utterance and iters = 0
    xs, ns, ts = pr.solve(y, A, 1e-3, iters=20, tol=1e-3, utt_offsets=[0, 20, 20, 40])
    assert ns[1] == 20 and np.isnan(ts[1]).all() and np.isfinite(ts[0, 0])
    x0 = np.full((40, 33), 0.25)
    assert np.array_equal(pr.solve(y, A, 1e-3, x0, iters=0)[0], x0)


def test_python_surface():
    import exemplars_vc_amd as evc
    from exemplars_vc_amd.compat import decomp
    for name in ("solve_activations_prox", "convert_prox"):
        assert name in evc.__all__ and callable(getattr(evc, name))
    sig = inspect.signature(evc.solve_activations_prox).parameters
    assert list(sig)[:3] == ["A", "X", "H0"] and sig["alpha"].default is inspect.Parameter.empty
    for k, dflt in (("positive", True), ("momentum", "fista"), ("normalize", True), ("check_every", 10), ("lipschitz", None)):
        assert sig[k].kind is inspect.Parameter.KEYWORD_ONLY and sig[k].default == dflt, k
    for k in ("alpha", "iters", "tol", "layout", "dtype", "device", "utt_offsets", "info"):
        assert sig[k].kind is inspect.Parameter.KEYWORD_ONLY, k
    assert list(inspect.signature(evc.convert_prox).parameters)[:3] == ["A", "B", "X"]
    lsig = inspect.signature(decomp.lasso.solve).parameters
    assert list(lsig)[:7] == ["y", "A", "alpha", "x", "tol", "method", "maxiter"]
    assert (lsig["tol"].default, lsig["method"].default, lsig["maxiter"].default) == (1e-3, "ista", 1000)
    assert list(inspect.signature(decomp.nnls.solve).parameters)[:7] == list(lsig)[:7]
    y, A = np.ones((3, 4)), np.ones((5, 4))
    for method in ("cd", "parallel_cd", "admm", "acc_ista", "cd_pos", "acc_ista_pos"):
        with pytest.raises(NotImplementedError, match="not mirrored"):
            decomp.lasso.solve(y, A, 1e-3, method=method)
    with pytest.raises(NotImplementedError, match="mask"):
        decomp.lasso.solve(y, A, 1e-3, mask=np.ones(4))
    with pytest.raises(NotImplementedError, match="complex"):
        decomp.lasso.solve(y.astype(complex), A.astype(complex), 1e-3)
    with pytest.raises(ValueError, match="Available methods"):
        decomp.lasso.solve(y, A, 1e-3, method="newton")
    with pytest.raises(ValueError, match="Available methods"):
        decomp.nnls.solve(y, A, 1e-3)                                 # deComP's own default names 'ista_pos_pos'
    with pytest.raises(ValueError, match="channels"):
        decomp.lasso.solve(np.ones((3, 6)), A, 1e-3)
    with pytest.raises(ValueError, match="x has shape"):
        decomp.lasso.solve(y, A, 1e-3, x=np.ones((3, 4)))
    it, x = decomp.lasso.solve(np.ones((2, 3, 4)), A, 1e-3, maxiter=0)
    assert it == -1 and x.shape == (2, 3, 5) and not x.any()
    Ab, Xb = np.ones((4, 5)), np.ones((4, 3))
    with pytest.raises(ValueError, match="number of bins"):
        evc.solve_activations_prox(Ab, np.ones((6, 3)), alpha=1e-3)
    with pytest.raises(ValueError, match="2-D"):
        evc.solve_activations_prox(Ab[0], Xb, alpha=1e-3)
    with pytest.raises(ValueError, match="dtype"):
        evc.solve_activations_prox(Ab, Xb, alpha=1e-3, dtype="f16")
    with pytest.raises(ValueError, match="1056 bins"):
        evc.solve_activations_prox(np.ones((1057, 7)), np.ones((1057, 3)), alpha=1e-3)
    with pytest.raises(ValueError, match="16384 exemplars"):
        evc.solve_activations_prox(np.ones((16385, 2)), np.ones((3, 2)), alpha=1e-3, layout="frame_major")
    with pytest.raises(ValueError, match="stop_rule"):
        evc.solve_activations_prox(Ab, Xb, alpha=1e-3, stop_rule="pymf")
    with pytest.raises(ValueError, match="momentum"):
        evc.solve_activations_prox(Ab, Xb, alpha=1e-3, momentum="adam")
    with pytest.raises(ValueError, match="alpha"):
        evc.solve_activations_prox(Ab, Xb, alpha=-1.0)
    with pytest.raises(ValueError, match="lipschitz"):
        evc.solve_activations_prox(Ab, Xb, alpha=1e-3, lipschitz=float("inf"))
    with pytest.raises(ValueError, match="checks"):
        evc.solve_activations_prox(Ab, Xb, alpha=1e-3, iters=5000, check_every=1)
    with pytest.raises(ValueError, match="number of exemplars"):
        evc.convert_prox(Ab, np.ones((9, 6)), Xb, alpha=1e-3)
    with pytest.raises(TypeError):
        evc.solve_activations_prox(Ab, Xb)                            # alpha has no default
    import torch
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="H0 has shape"):
            evc.solve_activations_prox(Ab, Xb, np.ones((3, 5)), alpha=1e-3)
        H = evc.solve_activations_prox(Ab, -Xb, alpha=1e-3, iters=3)
        assert H.shape == (5, 3) and not H.any()                      # A^T X < 0: the threshold cuts everything
    else:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            evc.solve_activations_prox(Ab, Xb, alpha=1e-3, iters=3)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            evc.convert_prox(Ab, np.ones((9, 5)), Xb, alpha=1e-3)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            decomp.lasso.solve(y, A, 1e-3)


# ---- the host pieces of the driver (csrc/evc_prox_plan.h) in a program of their own, plainly and under the sanitizers ----
SRC = os.path.join(ROOT, "tests", "prox_host_main.hip")
PKG = os.path.join(ROOT, "exemplars_vc_amd")


def _program_lines(tmp, sanitize):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = os.path.join(tmp, "prox_host_main" + ("_san" if sanitize else ""))
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
    tmp = str(tmp_path_factory.mktemp("prox_host"))
    return _program_lines(tmp, False), tmp


def test_host_carving_and_argument_checks(program):
    _lib, L = lib()
    carves = [ln.split() for ln in program[0] if ln.startswith("carve ")]
    assert len(carves) == 12 and not any("BAD" in ln for ln in program[0])
    for c in carves:
        M, N, T, n_utt, esize, shift = (int(v) for v in c[1:6] + [c[7]])
        offs = [int(v) for v in c[9:22]]
        assert offs[0] == (256 - shift) % 256 and offs == sorted(offs) and all((o + shift) % 256 == 0 for o in offs)
        query = int(L.evc_prox_workspace_bytes(M, N, T, n_utt, _lib.F64 if esize == 8 else _lib.F32))
        assert int(c[-1]) == query and int(c[-3]) <= query
    args = {ln.split()[1]: int(ln.split()[2]) for ln in program[0] if ln.startswith("args ")}
    want = dict(ok=0, ok_exact=0, short_by_one=-2, f32_ws=-2, ok_utts=0, bad_utts=-1, no_frames_no_x=0, frames_no_x=-1,
                struct_bytes=-1, iters_neg=-1, iters_0=0, slots_4097=0, slots_4098=-1, no_checks_many_iters=0,
                check_every_neg=-1, reserved=-1, reserved2=-1, mode=-1, mode_signed=0, momentum=-1, momentum_nesterov=0,
                normalize=-1, normalize_0=0, init_sklearn=-1, init_given=0, stop_sklearn=-1, stop_pymf=-1, stop_none=0,
                tol_neg=-1, tol_0=0, tol_inf=-1, alpha_neg=-1, alpha_0=0, alpha_nan=-1, lipschitz_neg=-1, lipschitz_set=0,
                lipschitz_inf=-1, init_value_inf=-1, dtype=-1, layout=-1, M_1056=0, M_1057=-3, M_1057_small_ws=-3, N_16384=0,
                N_16384_small_ws=-2, N_16385=-3, N_16385_small_ws=-3, nan_before_limits=-1, reserved_before_limits=-1)
    assert args == want
    # the wavefronts per workgroup: 8 from 512 workgroups of 128 rows x 64 frames on, else 4
    waves = {(int(ln.split()[1]), int(ln.split()[2])): int(ln.split()[3]) for ln in program[0] if ln.startswith("waves ")}
    for (N, T), W in waves.items():
        fb, rows = -(-T // 64), -(-N // 128) * 128
        assert W == (8 if fb * (rows // 128) >= 512 else 4), (N, T)
    assert [waves[k] for k in ((257, 5440), (257, 10880), (257, 10881))] == [4, 4, 8]
    assert waves[(4096, 688)] == 4 and waves[(4096, 1024)] == 8 and waves[(25, 0)] == 4 and waves[(1, 1)] == 4
    slots = {(int(ln.split()[1]), int(ln.split()[2])): int(ln.split()[3]) for ln in program[0] if ln.startswith("slots ")}
    for (iters, ce), n in slots.items():
        assert n == pr.n_slots(iters, ce), (iters, ce)
    assert slots[(2147483647, 1)] == 2147483647 and slots[(2147483647, 2147483647)] == 1
    # the momentum schedule of the host plan is the restatement's, to the last bit
    moms = {int(ln.split()[1]): [float(v) for v in ln.split()[2:]] for ln in program[0] if ln.startswith("mom ")}
    for kind, name in ((0, "ista"), (1, "fista"), (2, "nesterov")):
        assert moms[kind] == pr.schedule(name, 8), name


def test_the_iteration_loop_with_fake_callables(program):
    """prox_loop (csrc/evc_prox_plan.h), driven without a device: the checks at 0, k, 2k, ... < iters, the coefficients the
    sweep is handed against the restatement's schedule to the bit (the ping-pong and the hand-over of `partials` are
    checked in the program)"""
    loops = {}
    for ln in program[0]:
        if ln.startswith("loop "):
            w = ln.split()
            loops[w[1]] = (int(w[3]), [int(v) for v in w[5:w.index("c")]], [float(v) for v in w[w.index("c") + 1:]])
    want = {"fista_7_every_3": (7, 3, "fista"), "nesterov_5_every_1": (5, 1, "nesterov"), "ista_4_no_checks": (4, 0, "ista"),
            "masked_fista_10_every_10": (10, 10, "fista"), "masked_fista_11_every_10": (11, 10, "fista")}
    assert sorted(loops) == sorted(list(want) + ["nothing_live"])
    for name, (iters, every, momentum) in want.items():
        sweeps, checked, cs = loops[name]
        assert sweeps == iters and checked == (list(range(0, iters, every)) if every else []), name
        assert len(checked) == pr.n_slots(iters, every) and cs == pr.schedule(momentum, iters), name
    assert loops["nothing_live"] == (0, [], [])                     # no frames or no iterations: the two events only


def test_the_host_program_runs_clean_under_the_sanitizers(program):
    """a stand-alone program: address + undefined-behaviour sanitizers on the host code, nothing preloaded anywhere"""
    assert _program_lines(program[1], True) == program[0]
