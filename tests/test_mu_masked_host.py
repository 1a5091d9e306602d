"""The missing-data multiplicative-update solve and learning (evc_mu_masked_solve, evc_mu_masked_learn), host side: the C ABI's declarations and struct mirror,
the numpy restatement against every recorded deComP run (bit for bit), the Python surfaces' errors and the stand-alone host
program (csrc/evc_mu_masked_plan.h), plainly and under the sanitizers.  No GPU needed."""
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
import mu_masked_restatement as mmr  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
SHAPES = ["m25_n64_t32", "m40_n130_t33", "m1_n5_t3", "m201_n300_t20"]
FIXTURES = ["mum_%s_%s" % (s, l) for l in mmr.LOSSES for s in SHAPES]
LEARN_FIXTURES = ["mum_learn_m25_r8_t48_l2", "mum_learn_m40_r19_t33_kl", "mum_learn_m201_r12_t40_kl_k12"]


def lib():
    from exemplars_vc_amd import _lib
    return _lib, _lib.lib()


def load(name):
    d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    d["y"], d["D"], d["mask"] = d["y"].astype(np.float64), d["D"].astype(np.float64), d["mask"].astype(np.float64)
    d["loss"] = str(d["loss"])
    if "K" in d:
        d["K"] = int(d["K"])
    else:
        d["D0"], d["K"] = d["D0"].astype(np.float64), int(d["n_iter"])
        d["x0"] = d["x0"].astype(np.float64) if "x0" in d else None
    return d


# ---- the C ABI's face ----
def test_symbols_declared_and_exported():
    _lib, L = lib()
    hdr = open(os.path.join(ROOT, "include", "evc.h")).read()
    declared = set(re.findall(r"\b(evc_[a-z_0-9]+)\s*\(", hdr))
    for sym in ("evc_mu_masked_workspace_bytes", "evc_mu_masked_solve", "evc_mu_masked_learn_workspace_bytes",
                "evc_mu_masked_learn_splits", "evc_mu_masked_learn"):
        assert sym in declared and sym in _lib.SYMBOLS and hasattr(L, sym)
    assert "evc_mu_masked_solve " in hdr[:hdr.index("#ifndef EVC_H")]
    assert (_lib.MU_MASKED_MAX_M, _lib.MU_MASKED_MAX_SLOTS) == (528, 4097)


def test_opts_mirror_matches_header():
    _lib, _ = lib()
    hdr = open(os.path.join(ROOT, "include", "evc.h")).read()
    body = hdr[hdr.index("typedef struct evc_mu_masked_opts {"):hdr.index("} evc_mu_masked_opts;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for grp in re.findall(r"\b(?:int|double|void\*)\s+([a-zA-Z_0-9, ]+);", body) for n in grp.replace(" ", "").split(",")]
    assert names == [f[0] for f in _lib.MuMaskedOpts._fields_]
    assert C.sizeof(_lib.MuMaskedOpts) == 10 * 4 + 2 * 8 + 2 * 8
    body = hdr[hdr.index("typedef struct evc_mu_masked_learn_opts {"):hdr.index("} evc_mu_masked_learn_opts;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for grp in re.findall(r"\b(?:int|double|void\*)\s+([a-zA-Z_0-9, ]+);", body) for n in grp.replace(" ", "").split(",")]
    assert names == [f[0] for f in _lib.MuMaskedLearnOpts._fields_] and C.sizeof(_lib.MuMaskedLearnOpts) == 8 * 4 + 8 + 2 * 8
    assert C.sizeof(_lib.BetaOpts) == 8 * 4 + 5 * 8 + 2 * 8                         # the existing struct did not move


def test_statuses_through_the_library():
    """the same checks as the host program's, through the shared library: before any device work, in the statuses' order"""
    _lib, L = lib()
    one = C.c_void_p(8)              # never dereferenced: every case fails validation first

    def opts(**kw):
        o = _lib.MuMaskedOpts()
        o.struct_bytes = C.sizeof(o)
        o.dtype, o.layout, o.loss, o.iters = _lib.F64, _lib.FRAME_MAJOR, _lib.LOSS_KL, 100
        o.init_mode, o.check_every, o.stop_rule, o.tol, o.init_value = _lib.INIT_CONST, 10, _lib.STOP_SKLEARN, 1e-3, 1.0
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def call(o, M=25, N=17, T=70, lda=25, ldx=25, ldm=25, ldh=17, ws=16, A=one, X=one, mask=one, H=one, wsp=one):
        return L.evc_mu_masked_solve(A, lda, X, ldx, mask, ldm, H, ldh, M, N, T, None, 1, None if o is None else C.byref(o),
                                     wsp, ws, None, None, None)
    assert call(opts()) == -2 and call(opts(), mask=None, ldm=0) == -2 and call(None) == -1
    assert call(opts(), ldm=24) == -1 and call(opts(), ldm=40) == -2 and call(opts(), lda=24) == -1 and call(opts(), ldx=24) == -1
    assert call(opts(), ldh=16) == -1
    assert call(opts(layout=_lib.BIN_MAJOR), lda=17, ldx=70, ldm=69, ldh=70) == -1
    assert call(opts(layout=_lib.BIN_MAJOR), lda=17, ldx=70, ldm=70, ldh=70) == -2
    assert call(opts(loss=2)) == -1 and call(opts(loss=_lib.LOSS_FROBENIUS)) == -2
    assert call(opts(reserved=1)) == -1 and call(opts(reserved2=1)) == -1
    assert call(opts(struct_bytes=C.sizeof(_lib.BetaOpts))) == -1 and call(opts(tol=-1e-9)) == -1 and call(opts(tol=float("nan"))) == -1
    assert call(opts(init_mode=_lib.INIT_SKLEARN)) == -1 and call(opts(stop_rule=_lib.STOP_DECOMP)) == -1
    for p in ("A", "X", "H", "wsp"):
        assert call(opts(), **{p: None}) == -1
    assert call(opts(), T=0, X=None, H=None, mask=None) == -2
    assert call(opts(), M=529, lda=529, ldx=529, ldm=529) == -3 and call(opts(), M=528, lda=528, ldx=528, ldm=528) == -2
    assert call(opts(), M=529, lda=529, ldx=529, ldm=528) == -1 and call(opts(tol=-1.0), M=529, lda=529, ldx=529, ldm=529) == -1
    assert call(opts(), ws=int(L.evc_mu_masked_workspace_bytes(25, 17, 70, 1, _lib.F64)) - 1) == -2


def test_workspace_query():
    _lib, L = lib()
    q = L.evc_mu_masked_workspace_bytes
    assert q(529, 64, 100, 1, 0) == 0 and q(0, 64, 100, 1, 0) == 0 and q(25, 0, 100, 1, 0) == 0
    assert q(25, 64, -1, 1, 0) == 0 and q(25, 64, 100, 0, 0) == 0 and q(25, 64, 100, 1, 9) == 0
    assert q(528, 64, 100, 1, 0) > 0 and q(25, 64, 0, 1, 1) > 0
    assert q(25, 64, 688, 1, _lib.F32) < q(25, 64, 688, 1, _lib.F64) < q(201, 64, 688, 1, _lib.F64)
    ru = lambda v, m: -(-v // m) * m      # noqa: E731
    for M, N, T, n, dt, es in ((25, 64, 32, 1, _lib.F64, 8), (201, 4096, 11008, 16, _lib.F32, 4), (40, 130, 33, 2, _lib.F64, 8)):
        nt = -(-T // 16) + n
        own = (2 * ru(N, 16) * ru(M, 16) + nt * 16 * 3 * ru(M, 16)) * es + nt * 16 * 8 + nt * 16 + (n + 1) * 4 \
            + n * 4 + n * 16 + n * 4097 * 8
        assert own <= int(q(M, N, T, n, dt)) <= own + 14 * 256
    assert int(L.evc_beta_workspace_bytes(25, 17, 70, 1, _lib.F64)) > 0               # the existing query did not move away


# ---- the restatement against every recorded deComP run, bit for bit ----
def same_run(x, ref, d):
    """Bit for bit where this machine's BLAS sums the fixture's products as the recording machine's did (`blas_crc`,
    mmr.blas_fingerprint); elsewhere within 100 x the fixture's permutation figure (at least K eps) of max |x|."""
    if mmr.blas_fingerprint(d["y"], d["D"], d["mask"]) == d["blas_crc"].tolist():
        return np.array_equal(x, ref)
    fig = max(float(d["perm64"]), d["K"] * np.finfo(np.float64).eps)
    worst = float(np.max(np.abs(x - ref)) / np.max(np.abs(ref)))
    print("another BLAS summation order here: max error %.3e of max |x| (allowed %.3e)" % (worst, 100 * fig))
    return worst <= 100 * fig


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_reproduces_decomp(name):
    d = load(name)
    x, n_iter, tr = mmr.solve(d["y"], d["D"], d.get("x0"), mask=d["mask"], loss=d["loss"], iters=d["K"])
    assert same_run(x, d["x"], d) and n_iter.tolist() == [d["K"]] and np.isnan(tr).all() and tr.shape == (1, 1)
    assert x.dtype == np.float64 and np.isfinite(x).all() and x.any() and (x >= 0).all()
    dead = ~d["mask"].any(axis=1)
    assert (x[dead] == 0).all() and (x[~dead] > 0).all()            # a frame without data is exactly 0, nothing else is
    if "offs" in d:
        offs, tol = d["offs"].tolist(), float(d["tol"])
        xs, ns, trs = mmr.solve(d["y"], d["D"], d.get("x0"), mask=d["mask"], loss=d["loss"], iters=int(d["iters"]),
                                check_every=int(d["check_every"]), tol=tol, utt_offsets=offs)
        exact = mmr.blas_fingerprint(d["y"], d["D"], d["mask"]) == d["blas_crc"].tolist()
        assert ns.tolist() == d["n_iter_stop"].tolist() and np.isfinite(xs).all()
        assert np.array_equal(trs, d["trace_stop"], equal_nan=True) or not exact
        assert mmr.stop_margin(d["trace_stop"], tol) >= 1e-6 * tol                   # no stop decision sits on its threshold
        for u in range(len(offs) - 1):                              # a batch is one call per utterance
            a, b = offs[u], offs[u + 1]
            xu, nu, tu = mmr.solve(d["y"][a:b], d["D"], None if "x0" not in d else d["x0"][a:b], mask=d["mask"][a:b],
                                   loss=d["loss"], iters=int(d["iters"]), check_every=int(d["check_every"]), tol=tol)
            assert np.array_equal(xu, xs[a:b]) and nu[0] == ns[u] and np.array_equal(tu[0], trs[u], equal_nan=True)


def test_fixture_set_is_what_the_tests_need():
    kinds = {name: load(name) for name in FIXTURES}
    batches = [d for d in kinds.values() if "offs" in d]
    assert len(batches) == 4 and all(len(set(d["n_iter_stop"].tolist())) > 1 for d in batches)
    assert {str(d["kind"]) for d in kinds.values()} == {"binary", "weights"} and {d["loss"] for d in kinds.values()} == set(mmr.LOSSES)
    assert sorted({d["y"].shape[::-1] + (d["D"].shape[0],) for d in kinds.values()}) == [(1, 3, 5), (25, 32, 64), (40, 33, 130),
                                                                                         (201, 20, 300)]
    for name, d in kinds.items():
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 120 * 1024
        assert 0 < float(d["perm64"]) < 1e-12 and 0 < float(d["perm32"]) < 1e-3
        assert d["mask"].shape == d["y"].shape and (d["mask"] >= 0).all() and (d["mask"] == 0).any() and (d["mask"] > 0).any()
        assert (d["y"] >= 0).all() and (d["D"] > 0).all() and d["x"].any()
        assert (str(d["kind"]) == "binary") == bool(np.isin(d["mask"], (0.0, 1.0)).all())


def test_restatement_options():
    y, D = mmr.problem(25, 33, 40, 3)
    mask = mmr.problem_mask(40, 25, 3, "binary")
    for loss in mmr.LOSSES:
        # a mask of ones is the unmasked update to rounding
        ones = mmr.solve(y, D, mask=np.ones_like(y), loss=loss, iters=30)[0]
        base = mmr.solve(y, D, loss=loss, iters=30)[0]
        assert np.max(np.abs(ones - base)) < 1e-12 * np.max(base)
        # a binary mask that is constant over the frames: the problem with the masked bins deleted
        keep = mask[0] > 0
        const = np.tile(mask[0], (40, 1))
        got = mmr.solve(y, D, mask=const, loss=loss, iters=30)[0]
        red = mmr.solve(y[:, keep], D[:, keep], loss=loss, iters=30)[0]
        np.testing.assert_allclose(got, red, rtol=0, atol=1e-12 * np.abs(red).max())
        assert 0 < keep.sum() < 25
        # the error falls, the stop rule stops, an empty utterance is left alone, iters = 0 returns the start
        xs, ns, ts = mmr.solve(y, D, mask=mask, loss=loss, iters=60, check_every=2, tol=1e-3, utt_offsets=[0, 20, 20, 40])
        assert ns[1] == 60 and np.isnan(ts[1]).all() and (ns[[0, 2]] < 60).all()
        e = ts[0][np.isfinite(ts[0])]
        assert (np.diff(e) < 0).all() and len(e) == ns[0] // 2 + 1
        x0 = np.full((40, 33), 0.25)
        assert np.array_equal(mmr.solve(y, D, x0, mask=mask, loss=loss, iters=0)[0], x0)
        x32 = mmr.solve(y, D, mask=mask, loss=loss, iters=30, dtype=np.float32)[0]
        assert x32.dtype == np.float32 and np.max(np.abs(x32 - mmr.solve(y, D, mask=mask, loss=loss, iters=30)[0])) < 1e-3
        # a frame without data: exactly 0 after one update; a NaN stays in its frame
        dead = mask.copy()
        dead[4] = 0.0
        assert (mmr.solve(y, D, mask=dead, loss=loss, iters=1)[0][4] == 0).all()
        bad = y.copy()
        bad[7, 3] = np.nan
        xb = mmr.solve(bad, D, mask=np.ones_like(y), loss=loss, iters=3)[0]
        assert np.isnan(xb[7]).all() and np.isfinite(np.delete(xb, 7, axis=0)).all()
        assert mmr.permutation_figure(y, D, mask, 30, np.float64, loss) >= 30 * np.finfo(np.float64).eps
    with pytest.raises(ValueError):
        mmr.solve(y, D, mask=mask, loss="is", iters=1)
    for kind in ("binary", "weights"):
        m = mmr.problem_mask(9, 7, 1, kind)
        assert m.shape == (9, 7) and (m >= 0).all() and m[0, 0] == 0 and m[0, 1] == 1 and np.array_equal(m, m.astype(np.float32))
    with pytest.raises(ValueError):
        mmr.problem_mask(3, 3, 0, "gaussian")


# ---- the learning: the restatement against deComP's nmf.solve, bit for bit ----
@pytest.mark.parametrize("name", LEARN_FIXTURES)
def test_learn_restatement_reproduces_decomp(name):
    d = load(name)
    tol, maxiter = float(d["tol"]), int(d["maxiter"])
    it, D, x, stats = mmr.learn(d["y"], d["D0"], d["x0"], mask=d["mask"], loss=d["loss"], tol=tol, maxiter=maxiter)
    if mmr.blas_fingerprint(d["y"], d["D0"], d["mask"]) == d["blas_crc"].tolist():
        assert it == int(d["it"]) and np.array_equal(D, d["D"]) and np.array_equal(x, d["x"]) and np.array_equal(stats, d["stats"])
    else:
        fig = max(float(d["perm64"]), d["K"] * np.finfo(np.float64).eps)
        assert it == int(d["it"]) and np.max(np.abs(D - d["D"])) <= 100 * fig * np.max(d["D"])
        assert np.max(np.abs(x - d["x"])) <= 100 * fig * np.max(d["x"])
    assert len(d["stats"]) == d["K"] and np.isfinite(d["D"]).all() and (d["D"] >= 0).all() and (d["x"] >= 0).all()
    np.testing.assert_allclose(np.linalg.norm(d["D"], axis=1), 1.0, rtol=0, atol=4 * np.finfo(np.float64).eps)
    if tol > 0:
        assert np.min(np.abs(d["stats"] - tol)) >= 1e-6 * tol        # no stop decision sits on its threshold
    # the loop runs at most maxiter - 1 iterations; `it` is the stopping iteration, else maxiter
    assert (int(d["it"]) == d["K"] < maxiter and d["stats"][-1] < tol) or (int(d["it"]) == maxiter == d["K"] + 1)
    # iterations of the restatement are update_x, update_d, the normalisation: one by hand
    Dn = mmr.l2_strict(d["D0"])
    x0 = np.ones((d["y"].shape[0], Dn.shape[0])) if d["x0"] is None else d["x0"]
    x1 = mmr.update_x(d["y"], x0, Dn, d["mask"], d["loss"])
    D1 = mmr.l2_strict(mmr.update_d(d["y"], x1, Dn, d["mask"], d["loss"]))
    one = mmr.learn(d["y"], d["D0"], d["x0"], mask=d["mask"], loss=d["loss"], tol=0.0, maxiter=2)
    assert one[0] == 2 and np.array_equal(one[1], D1) and np.array_equal(one[2], x1) and one[3].tolist() == [np.max(np.abs(Dn - D1))]
    assert np.array_equal(x1, mmr.solve(d["y"], Dn, x0, mask=d["mask"], loss=d["loss"], iters=1)[0])


def test_learn_fixture_set():
    ds = [load(n) for n in LEARN_FIXTURES]
    assert any(int(d["it"]) < int(d["maxiter"]) for d in ds) and any(int(d["it"]) == int(d["maxiter"]) for d in ds)
    assert {d["loss"] for d in ds} == set(mmr.LOSSES) and {str(d["kind"]) for d in ds} == {"binary", "weights"}
    assert sum(1 for d in ds if d["x0"] is not None) == 1
    for n, d in zip(LEARN_FIXTURES, ds):
        assert os.path.getsize(os.path.join(GOLDEN, n + ".npz")) < 120 * 1024
        assert 0 < float(d["perm64"]) < 1e-12 and 0 < float(d["perm32"]) < 1e-3 and (d["mask"] == 0).any()


def test_compat_nmf_solve(monkeypatch):
    """deComP's refusals and the maxiter mapping, without a device"""
    from exemplars_vc_amd import solver
    from exemplars_vc_amd.compat import decomp
    calls = []

    def fake(X, W0, H0, mask=None, **kw):
        calls.append((X, W0, H0, mask, kw))
        n = min(kw["iters"], 7)
        return W0 * 0.5, H0 * 2.0, {"n_iter": n, "stopped": kw["tol"] > 0 and n == 7, "stat": np.zeros(1 + kw["iters"])}
    monkeypatch.setattr(solver, "learn_dictionary_masked", fake)
    y, D = np.ones((6, 4)), np.ones((5, 4))
    mask = np.ones((6, 4))
    it, Dn, x = decomp.nmf.solve(y, D, maxiter=50, likelihood='kl', mask=mask)
    X, W0, H0, m, kw = calls[-1]
    assert it == 7 and Dn.shape == (5, 4) and x.shape == (6, 5) and np.array_equal(H0, np.ones((6, 5)))     # x=None: ones
    assert kw["iters"] == 49 and kw["check_every"] == 1 and kw["tol"] == 1e-3 and kw["loss"] == "kl" and kw["layout"] == "frame_major"
    assert m is not None and m.shape == (6, 4) and X.shape == (6, 4) and W0.shape == (5, 4)
    assert decomp.nmf.solve(y, D, tol=0.0, maxiter=50)[0] == 50 and calls[-1][3] is None and calls[-1][4]["loss"] == "frobenius"
    assert decomp.nmf.solve(y, D, maxiter=5)[0] == 5 and calls[-1][4]["iters"] == 4        # ran to the end: maxiter
    assert decomp.nmf.solve(y, D, maxiter=1)[0] == 1 and calls[-1][4]["iters"] == 0
    assert decomp.nmf.solve(y.astype(np.float32), D.astype(np.float32), maxiter=3)[1].dtype == np.float32
    n = len(calls)
    with pytest.raises(NotImplementedError):
        decomp.nmf.solve(y, D, minibatch=2)
    with pytest.raises(NotImplementedError, match="algorithm"):
        decomp.nmf.solve(y, D, method='svrmu')
    with pytest.raises(NotImplementedError):
        decomp.nmf.solve(y, D, likelihood='is')
    with pytest.raises(AssertionError):
        decomp.nmf.solve(y, -D)
    with pytest.raises(AssertionError):
        decomp.nmf.solve(y, D, x=-np.ones((6, 5)))
    with pytest.raises(AssertionError):
        decomp.nmf.solve(-y, D, likelihood='kl')
    with pytest.raises(ValueError, match="should be satisfied"):
        decomp.nmf.solve(y, np.ones((5, 3)))
    with pytest.raises(ValueError, match="should be satisfied"):
        decomp.nmf.solve(y, D, x=np.ones((6, 4)))
    with pytest.raises(ValueError, match="identical"):
        decomp.nmf.solve(y, D, mask=np.ones((6, 3)))
    with pytest.raises(ValueError, match="Dimension"):
        decomp.nmf.solve(np.ones((2, 3, 4)), D, x=np.ones((2, 5)))
    with pytest.raises(ValueError, match="Data type"):
        decomp.nmf.solve(y, D.astype(np.float32))
    with pytest.raises(ValueError, match="Data type"):
        decomp.nmf.solve(y.astype(np.int64), D.astype(np.int64))
    assert len(calls) == n and "nmf.solve" in decomp.__doc__
    decomp.nmf.solve(-y, D)                                                    # l2: deComP does not look at y's sign
    assert len(calls) == n + 1


def test_learn_statuses_through_the_library():
    _lib, L = lib()
    one = C.c_void_p(8)

    def opts(**kw):
        o = _lib.MuMaskedLearnOpts()
        o.struct_bytes = C.sizeof(o)
        o.dtype, o.layout, o.loss, o.iters, o.check_every, o.tol = _lib.F64, _lib.FRAME_MAJOR, _lib.LOSS_KL, 100, 1, 1e-3
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def call(o, M=25, R=8, T=48, ldx=25, ldm=25, ldw=25, ldh=8, ws=16, X=one, mask=one, W=one, H=one, wsp=one):
        return L.evc_mu_masked_learn(X, ldx, mask, ldm, W, ldw, H, ldh, M, R, T, None if o is None else C.byref(o), wsp, ws, None,
                                     None, None)
    assert call(opts()) == -2 and call(opts(), mask=None, ldm=0) == -2 and call(None) == -1 and call(opts(), ldm=24) == -1
    assert call(opts(reserved=3 << 8)) == -2 and call(opts(reserved=65 << 8)) == -1 and call(opts(reserved=1)) == -1
    assert call(opts(tol=-1.0)) == -1 and call(opts(loss=2)) == -1 and call(opts(), T=0) == -1
    assert call(opts(), M=529, ldx=529, ldm=529, ldw=529) == -3 and call(opts(), R=4097, ldh=4097) == -3
    q, sp = L.evc_mu_masked_learn_workspace_bytes, L.evc_mu_masked_learn_splits
    assert q(529, 8, 48, 0) == 0 and q(25, 4097, 48, 0) == 0 and q(25, 8, 0, 0) == 0 and q(25, 8, 48, 4) == 0 and q(25, 8, 48, 1) > 0
    assert sp(529, 8, 48) == 0 and sp(25, 8, 48) == 1 and sp(25, 8, 48) == L.evc_beta_learn_splits(25, 8, 48)
    assert sp(25, 64, 11008) == L.evc_beta_learn_splits(25, 64, 11008) > 1
    assert call(opts(), ws=int(q(25, 8, 48, 0)) - 1) == -2


# ---- the Python surfaces ----
def test_wrappers_reject_bad_arguments_before_any_device(monkeypatch):
    import exemplars_vc_amd as evc
    from exemplars_vc_amd import solver
    for name in ("solve_activations_masked", "convert_masked", "learn_dictionary_masked"):
        assert name in evc.__all__ and callable(getattr(evc, name))
    sig = inspect.signature(evc.solve_activations_masked).parameters
    assert list(sig)[:4] == ["A", "X", "mask", "H0"] and sig["mask"].default is None and sig["loss"].default == "frobenius"
    for k in ("loss", "iters", "check_every", "tol", "utt_offsets"):
        assert sig[k].kind is inspect.Parameter.KEYWORD_ONLY, k
    monkeypatch.setattr(solver, "require_device", lambda device=None: pytest.fail("a device was asked for"))
    Ab, Xb = np.ones((4, 5)), np.ones((4, 3))
    with pytest.raises(ValueError, match="mask has shape"):
        evc.solve_activations_masked(Ab, Xb, np.ones((3, 4)))
    for bad in (-1.0, np.nan, np.inf):
        m = np.ones((4, 3))
        m[2, 1] = bad
        with pytest.raises(ValueError, match="finite weights >= 0"):
            evc.solve_activations_masked(Ab, Xb, m)
        with pytest.raises(ValueError, match="finite weights >= 0"):
            evc.convert_masked(Ab, Ab, Xb, m)
    with pytest.raises(ValueError, match="loss"):
        evc.solve_activations_masked(Ab, Xb, loss="itakura-saito")
    with pytest.raises(ValueError, match="stop_rule"):
        evc.solve_activations_masked(Ab, Xb, stop_rule="decomp")
    with pytest.raises(ValueError, match="tol"):
        evc.solve_activations_masked(Ab, Xb, tol=-1.0)
    with pytest.raises(ValueError, match="init"):
        evc.solve_activations_masked(Ab, Xb, init="sklearn")
    with pytest.raises(ValueError, match="error slots"):
        evc.solve_activations_masked(Ab, Xb, iters=5000, check_every=1)
    with pytest.raises(ValueError, match="number of bins"):
        evc.solve_activations_masked(Ab, np.ones((5, 3)))
    with pytest.raises(ValueError, match="at most 528"):
        evc.solve_activations_masked(np.ones((529, 5)), np.ones((529, 3)))
    with pytest.raises(ValueError, match="number of exemplars"):
        evc.convert_masked(Ab, np.ones((9, 4)), Xb)
    sig = inspect.signature(evc.learn_dictionary_masked).parameters
    assert list(sig)[:4] == ["X", "W0", "H0", "mask"] and sig["tol"].default == 0.0 and sig["layout"].default is inspect.Parameter.empty
    W0, H0 = np.ones((4, 2)), np.ones((2, 3))
    with pytest.raises(ValueError, match="mask has shape"):
        evc.learn_dictionary_masked(Xb, W0, H0, np.ones((3, 4)), layout="bin_major", iters=3)
    with pytest.raises(ValueError, match="finite weights >= 0"):
        evc.learn_dictionary_masked(Xb, W0, H0, -np.ones((4, 3)), layout="bin_major", iters=3)
    with pytest.raises(ValueError, match="loss"):
        evc.learn_dictionary_masked(Xb, W0, H0, loss="is", layout="bin_major", iters=3)
    with pytest.raises(ValueError, match="tol"):
        evc.learn_dictionary_masked(Xb, W0, H0, layout="bin_major", iters=3, tol=-1.0)
    with pytest.raises(ValueError, match="at most 528"):
        evc.learn_dictionary_masked(np.ones((529, 3)), np.ones((529, 2)), H0, layout="bin_major", iters=3)


def test_a_good_call_reaches_the_device_or_raises_without_one():
    import torch
    import exemplars_vc_amd as evc
    Ab, Xb = np.ones((4, 5)), np.ones((4, 3))
    if torch.cuda.is_available():
        H = evc.solve_activations_masked(Ab, Xb, np.zeros((4, 3)), iters=1)
        assert H.shape == (5, 3) and not H.any()                      # nothing is observed: (h 0) / J
    else:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            evc.solve_activations_masked(Ab, Xb, np.ones((4, 3)))


# ---- the host pieces of the driver (csrc/evc_mu_masked_plan.h) in a program of their own, plainly and under the sanitizers ----
SRC = os.path.join(ROOT, "tests", "mu_masked_host_main.hip")
PKG = os.path.join(ROOT, "exemplars_vc_amd")


def _program_lines(tmp, sanitize):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = os.path.join(tmp, "mu_masked_host_main" + ("_san" if sanitize else ""))
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
    tmp = str(tmp_path_factory.mktemp("mu_masked_host"))
    return _program_lines(tmp, False), tmp


def test_host_carving_and_argument_checks(program):
    _lib, L = lib()
    carves = [ln.split() for ln in program[0] if ln.startswith("carve ")]
    assert len(carves) == 32 and not any("BAD" in ln for ln in program[0])
    for c in carves:
        M, N, T, n_utt, esize, shift = (int(v) for v in c[1:6] + [c[7]])
        offs = [int(v) for v in c[9:21]]
        assert len(offs) == 12 and c[21] == "bytes"
        # no overlap (the program checks every array's room), every start a multiple of 256 bytes, the total is the query
        assert offs[0] == (256 - shift) % 256 and offs == sorted(offs) and all((o + shift) % 256 == 0 for o in offs)
        query = int(L.evc_mu_masked_workspace_bytes(M, N, T, n_utt, _lib.F64 if esize == 8 else _lib.F32))
        assert int(c[-1]) == query and int(c[-3]) <= query <= int(c[-3]) + 512
    args = {ln.split()[1]: int(ln.split()[2]) for ln in program[0] if ln.startswith("args ")}
    want = dict(ok=0, ok_exact=0, short_by_one=-2, f32_ws=-2, ok_utts=0, bad_utts=-1, no_frames_no_x=0, frames_no_x=-1,
                no_mask=0, no_mask_any_ldm=0, ldm_short=-1, ldm_padded=0, lda_short=-1, ldh_short=-1, ldm_short_bin_major=-1,
                struct_bytes=-1, struct_bytes_0=-1, iters_neg=-1, iters_0=0, slots_4097=0, slots_4098=-1, no_checks_many_iters=0,
                check_every_neg=-1, reserved=-1, reserved2=-1, loss=-1, loss_l2=0, init_sklearn=-1, init_given=0,
                stop_decomp=-1, stop_pymf=-1, stop_none=0, tol_neg=-1, tol_0=0, tol_inf=-1, tol_nan=-1, init_value_inf=-1,
                dtype=-1, layout=-1, M_528=0, M_529=-3, M_529_small_ws=-3, N_large=0, tol_before_limits=-1,
                struct_bytes_before_limits=-1, ldm_before_limits=-1, M_0=-1, N_0=-1, T_neg=-1, n_utt_0=-1)
    assert args == want
    # the size query is 0 exactly where the call refuses with -1 or -3
    query = {ln.split()[1]: int(ln.split()[2]) for ln in program[0] if ln.startswith("query ")}
    assert all(query[k] > 0 for k in ("ok", "M_528", "T_0"))
    assert all(query[k] == 0 for k in ("M_529", "M_0", "N_0", "T_neg", "n_utt_0", "dtype")) and len(query) == 9
    slots = {(int(ln.split()[1]), int(ln.split()[2])): int(ln.split()[3]) for ln in program[0] if ln.startswith("slots ")}
    assert len(slots) == 7
    for (iters, ce), n in slots.items():
        assert n == mmr.n_slots(iters, ce), (iters, ce)
    # the learning: its own nine arrays, the activation half's carving inside its share
    lcarves = [ln.split() for ln in program[0] if ln.startswith("lcarve ")]
    assert len(lcarves) == 24
    for c in lcarves:
        M, R, T, esize, shift = (int(v) for v in c[1:5] + [c[6]])
        offs = [int(v) for v in c[8:17]]
        assert len(offs) == 9 and c[17] == "bytes"
        assert offs[0] == (256 - shift) % 256 and offs == sorted(offs) and all((o + shift) % 256 == 0 for o in offs)
        query = int(L.evc_mu_masked_learn_workspace_bytes(M, R, T, _lib.F64 if esize == 8 else _lib.F32))
        assert int(c[-1]) == query and int(c[-3]) <= query <= int(c[-3]) + 512
    largs = {ln.split()[1]: (int(ln.split()[2]), int(ln.split()[3])) for ln in program[0] if ln.startswith("largs ")}
    lwant = dict(ok=0, ok_exact=0, short_by_one=-2, no_mask=0, ldm_short=-1, ldw_short=-1, no_w=-1, struct_bytes=-1, forced_7=0,
                 forced_65=-1, reserved=-1, reserved2=-1, loss=-1, loss_kl=0, iters_neg=-1, iters_0=0, slots_4098=-1,
                 no_checks_many_iters=0, tol_neg=-1, tol_nan=-1, tol_0=0, dtype=-1, T_0=-1, M_528=0, M_529=-3, R_4096=0, R_4097=-3,
                 tol_before_limits=-1)
    assert {k: v[0] for k, v in largs.items()} == lwant and largs["forced_7"][1] == 7 and largs["ok"][1] == 0
    lquery = {ln.split()[1]: int(ln.split()[2]) for ln in program[0] if ln.startswith("lquery ")}
    assert lquery["ok"] > 0 and lquery["limits"] > 0 and len(lquery) == 8
    assert all(lquery[k] == 0 for k in ("M_529", "R_4097", "T_0", "M_0", "R_0", "dtype"))


def test_the_host_program_runs_clean_under_the_sanitizers(program):
    """a stand-alone program: address + undefined-behaviour sanitizers on the host code, nothing preloaded anywhere"""
    assert _program_lines(program[1], True) == program[0]
