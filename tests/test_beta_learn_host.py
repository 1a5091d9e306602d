"""Beta-divergence dictionary learning (evc_beta_learn), host side: the C ABI's declarations, struct mirror and argument
checks, the numpy restatement against scikit-learn's recorded results (tests/golden/dictbeta_sk_*.npz), the fixture
generator and the Python surface's validation.  No GPU needed."""
import ctypes as C
import glob
import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beta_learn_restatement as blr  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "dictbeta_sk_*.npz")))
ZERO_MSG = "When beta_loss <= 0 and X contains zeros, the solver may diverge"
E64 = 2.0 ** -52


def lib():
    from exemplars_vc_amd import _lib
    return _lib, _lib.lib()


def penalties(d):
    """(l1_h, l2_h, l1_w, l2_w) as scikit-learn scales them (_nmf.py:1254-1265), alpha_H = 'same'"""
    M, T = d["X"].shape
    a, r = float(d["alpha"]), float(d["l1_ratio"])
    return M * a * r, M * a * (1 - r), T * a * r, T * a * (1 - r)


def test_symbols_declared_and_exported():
    _lib, L = lib()
    hdr = open(os.path.join(ROOT, "include", "evc.h")).read()
    declared = set(re.findall(r"\b(evc_[a-z_0-9]+)\s*\(", hdr))
    for sym in ("evc_beta_learn", "evc_beta_learn_workspace_bytes", "evc_beta_learn_splits", "evc_beta_learn_route"):
        assert sym in declared and sym in _lib.SYMBOLS and hasattr(L, sym)
    assert "evc_beta_learn " in hdr[:hdr.index("#ifndef EVC_H")]          # listed in the header comment
    sync = hdr[hdr.index("Host synchronisation"):hdr.index("No global mutable state")]
    assert "(9) evc_beta_learn" in sync
    assert "1026" in hdr[hdr.index("Multiplicative updates of BOTH factors under any beta-divergence"):]
    assert L.evc_version() == 100


def test_opts_mirror_matches_header():
    _lib, _ = lib()
    hdr = open(os.path.join(ROOT, "include", "evc.h")).read()
    body = hdr[hdr.index("typedef struct evc_beta_learn_opts {"):hdr.index("} evc_beta_learn_opts;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for grp in re.findall(r"\b(?:int|double|void\*)\s+([a-zA-Z_0-9, ]+);", body)
             for n in grp.replace(" ", "").split(",")]
    assert names == [f[0] for f in _lib.BetaLearnOpts._fields_]
    assert names == ["struct_bytes", "dtype", "layout", "iters", "check_every", "reserved", "beta", "tol", "l1_h", "l2_h",
                     "l1_w", "l2_w", "ev_loop_start", "ev_loop_stop"]
    assert C.sizeof(_lib.BetaLearnOpts) == 6 * 4 + 6 * 8 + 2 * 8


def _opts(_lib, **kw):
    o = _lib.BetaLearnOpts()
    o.struct_bytes = C.sizeof(_lib.BetaLearnOpts)
    o.dtype, o.layout, o.iters, o.beta = _lib.F64, _lib.FRAME_MAJOR, 5, 0.5
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_bad_arguments_rejected_before_device_work():
    _lib, L = lib()
    one = C.c_void_p(8)              # never dereferenced: every case fails validation first

    def call(o, M=25, R=17, T=70, ldx=25, ldw=25, ldh=17, ws=1 << 40, X=one, W=one, H=one, wsp=one):
        return L.evc_beta_learn(X, ldx, W, ldw, H, ldh, M, R, T, C.byref(o), wsp, ws, None, None, None)
    bad = _opts(_lib)
    bad.struct_bytes = 4
    assert call(bad) == -1
    assert L.evc_beta_learn(one, 25, one, 25, one, 17, 25, 17, 70, None, one, 1 << 40, None, None, None) == -1
    assert call(_opts(_lib), M=0) == -1
    assert call(_opts(_lib), R=0) == -1
    assert call(_opts(_lib), T=0) == -1
    assert call(_opts(_lib), ldx=24) == -1
    assert call(_opts(_lib), ldw=24) == -1
    assert call(_opts(_lib), ldh=16) == -1
    for ld in (dict(ldx=69, ldw=17, ldh=70), dict(ldx=70, ldw=16, ldh=70), dict(ldx=70, ldw=17, ldh=69)):
        assert call(_opts(_lib, layout=_lib.BIN_MAJOR), **ld) == -1
    assert call(_opts(_lib, layout=_lib.BIN_MAJOR), ldx=70, ldw=17, ldh=70, ws=16) == -2
    for p in ("X", "W", "H", "wsp"):
        assert call(_opts(_lib), **{p: None}) == -1
    for v in (float("nan"), float("inf"), -float("inf")):
        assert call(_opts(_lib, beta=v)) == -1
    for f in ("tol", "l1_h", "l2_h", "l1_w", "l2_w"):
        assert call(_opts(_lib, **{f: -1e-4})) == -1
        assert call(_opts(_lib, **{f: float("nan")})) == -1
    assert call(_opts(_lib, iters=-1)) == -1
    assert call(_opts(_lib, check_every=-1)) == -1
    assert call(_opts(_lib, iters=5000, check_every=1)) == -1      # more error slots than the workspace holds
    assert call(_opts(_lib, iters=4096, check_every=1), ws=16) == -2
    assert call(_opts(_lib, dtype=7)) == -1
    assert call(_opts(_lib, layout=5)) == -1
    for r in (1, 0x80, 65 << 8, 3 << 16, 1 << 18, -1):            # low bits, too many ranges, route 3, a bit beyond
        assert call(_opts(_lib, reserved=r)) == -1
    assert call(_opts(_lib, reserved=(64 << 8) | (2 << 16)), ws=16) == -2
    assert call(_opts(_lib), ws=16) == -2                         # workspace too small
    assert call(_opts(_lib), M=529, ldx=529, ldw=529) == -3       # beyond k_beta_sweep's two LDS images
    assert call(_opts(_lib), M=529, ldx=529, ldw=529, ws=16) == -3
    assert call(_opts(_lib), R=4097, ldh=4097, ws=16) == -3
    assert call(_opts(_lib, reserved=1 << 16), R=257, ldh=257) == -3      # the fused route forced where it does not hold
    assert call(_opts(_lib, reserved=1 << 16), R=256, ldh=256, ws=16) == -2
    assert call(_opts(_lib, beta=float("nan")), M=529, ldx=529, ldw=529) == -1        # -1 before -3


def test_workspace_splits_and_route_queries():
    _lib, L = lib()
    q = L.evc_beta_learn_workspace_bytes
    assert q(25, 16, 688, _lib.F64) < q(25, 128, 688, _lib.F64) < q(25, 128, 6880, _lib.F64)
    assert q(513, 16, 688, _lib.F64) > q(25, 16, 688, _lib.F64)
    assert q(201, 20, 688, _lib.F32) < q(201, 20, 688, _lib.F64)
    assert q(528, 4096, 1, 0) > 0 and q(529, 1, 1, 0) == 0 and q(25, 4097, 1, 0) == 0
    assert q(0, 1, 1, 0) == 0 and q(25, 0, 1, 0) == 0 and q(25, 1, 0, 0) == 0 and q(25, 1, 1, 9) == 0
    for M, R, T in ((25, 17, 70), (50, 24, 150), (514, 16, 100000), (201, 300, 5000)):
        assert L.evc_beta_learn_splits(M, R, T) == L.evc_learn_splits(M, R, T) >= 1
    assert L.evc_beta_learn_splits(529, 1, 1) == 0 and L.evc_beta_learn_route(529, 1, 1) == 0
    assert L.evc_beta_learn_route(25, 17, 70) == 1 and L.evc_beta_learn_route(50, 16, 65536) == 1
    assert L.evc_beta_learn_route(17, 300, 40) == 2 and L.evc_beta_learn_route(25, 257, 70) == 2
    routes = [L.evc_beta_learn_route(25, R, 70) for R in range(1, 300)]          # one bound in R: fused below it
    assert routes == sorted(routes) and set(routes) == {1, 2}


def test_fixture_table():
    names = [os.path.basename(p)[:-4] for p in FILES]
    for beta in ("bm1", "b0", "b0p5", "b1p5", "b3", "b0p3"):
        assert f"dictbeta_sk_m25_r17_t70_k40_{beta}" in names
    for beta in ("b0p5", "b0", "b1"):
        assert f"dictbeta_sk_m25_r17_t70_k30_flush_{beta}" in names
    shapes = set()
    for p in FILES:
        d = np.load(p)
        assert os.path.getsize(p) <= 1 << 20
        assert set(d.files) == {"X", "W0", "H0", "W", "H", "n_iter", "max_iter", "tol", "beta", "err", "alpha", "l1_ratio",
                                "dtype"}
        shapes.add(d["X"].shape + (d["W0"].shape[1],))
        assert d["W"].dtype == d["H"].dtype == d["X"].dtype == np.dtype(str(d["dtype"]))
    assert {(25, 70, 17), (201, 100, 20), (513, 40, 16), (25, 70, 130), (17, 40, 300), (50, 150, 24)} <= shapes
    assert len(FILES) == 18


def test_early_stop_and_flush_fixture_properties():
    stops = 0
    for p in FILES:
        d = np.load(p)
        tol, beta = float(d["tol"]), float(d["beta"])
        if tol > 0:
            assert 20 < int(d["n_iter"]) < int(d["max_iter"])
            k = int(d["n_iter"]) // 10
            e = d["err"]
            dec = (e[:k] - e[1:k + 1]) / e[0]
            assert (dec[:-1] >= tol).all() and dec[-1] < tol
            assert np.min(np.abs(dec - tol)) >= 0.01 * tol, p
            stops += 1
        if "flush" in p:
            assert ((d["W0"] == 1e-19).sum() >= 10) and ((d["H0"] == 1e-19).sum() >= 10)
            assert (d["W"] == 0).sum() >= 10
            assert ((d["H"] == 0).sum() >= 10) == (beta < 1)
        for F in (d["W"], d["H"]):
            pos = F[F > 0].astype(np.float64)
            assert not np.any((pos > E64 * (1 - 1e-3)) & (pos < E64 * (1 + 1e-3)))
    assert stops == 2
    d = np.load(os.path.join(GOLDEN, "dictbeta_sk_m50_r24_t150_k40_zeros_b1p5.npz"))
    assert (d["H0"][5] == 0).all() and (d["X"][:, [3, 77]] == 0).all() and np.isfinite(d["W"]).all()
    assert (d["H"][5] == 0).all() and (d["H"][:, [3, 77]] == 0).all()


def close_factor(got, ref, rtol=1e-9):
    """non-zero entries within rtol, zeros exact"""
    assert np.array_equal(got == 0, ref == 0)
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=0)


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("path", FILES, ids=os.path.basename)
def test_restatement_reproduces_sklearn_fixture(path, S):
    d = np.load(path)
    dt = np.dtype(str(d["dtype"]))
    W, H, n_iter, err = blr.learn(d["X"], d["W0"], d["H0"], float(d["beta"]), int(d["max_iter"]), 10, float(d["tol"]),
                                  *penalties(d), S=S, dtype=dt)
    assert W.dtype == H.dtype == dt
    assert n_iter == int(d["n_iter"])
    if dt == np.float64:
        close_factor(W, d["W"])
        close_factor(H, d["H"])
        np.testing.assert_allclose(err[:len(d["err"])], d["err"], rtol=1e-9, atol=0)
    else:
        for got, ref in ((W, d["W"]), (H, d["H"])):
            assert np.linalg.norm(got.astype(np.float64) - ref) / np.linalg.norm(ref) <= 1e-4
        np.testing.assert_allclose(err[:len(d["err"])], d["err"], rtol=1e-4, atol=0)


def test_restatement_one_and_two_agree_with_the_special_cased_updates():
    """beta = 1 and beta = 2 through the generic statement: scikit-learn's special-cased results to rounding"""
    for name, beta in (("dictkl_sk_m50_r24_t150_k40", 1.0), ("dictmu_sk_m50_r24_t150_k40", 2.0)):
        d = np.load(os.path.join(GOLDEN, name + ".npz"))
        W, H, n_iter, _ = blr.learn(d["X"], d["W0"], d["H0"], beta, int(d["max_iter"]), 10, float(d["tol"]))
        assert n_iter == int(d["n_iter"])
        np.testing.assert_allclose(W, d["W"], rtol=1e-9, atol=0)
        np.testing.assert_allclose(H, d["H"], rtol=1e-9, atol=0)


def test_generator_reproduces_the_fixtures():
    pytest.importorskip("sklearn")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_golden_beta_learn as g
    specs = g.cases()
    assert sorted(specs) == sorted(os.path.basename(p)[:-4] for p in FILES)
    for name in ("dictbeta_sk_m25_r17_t70_k30_flush_b0", "dictbeta_sk_m50_r24_t150_tol_b1p5"):
        out = g.make(name, specs[name])
        ref = np.load(os.path.join(GOLDEN, name + ".npz"))
        assert set(out) == set(ref.files)
        for k, v in out.items():
            v = np.asarray(v)
            assert np.asarray(ref[k]).dtype == v.dtype and np.asarray(ref[k]).tobytes() == v.tobytes(), (name, k)


def _small():
    rng = np.random.default_rng(0)
    return rng.random((6, 4)) + 0.1, rng.random((5, 4)) + 0.1, rng.random((6, 5)) + 0.1      # X, dictionary, activations


def _runs_or_refuses(fn):
    """with a device the call answers; without one it refuses (there is no CPU fallback)"""
    import torch
    if torch.cuda.is_available():
        return fn()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fn()


def test_python_surface():
    import exemplars_vc_amd as evc
    from exemplars_vc_amd.compat import factorize as fz
    X, D, W0 = _small()
    assert "learn_dictionary_beta" in evc.__all__
    sig = inspect.signature(evc.learn_dictionary_beta)
    assert list(sig.parameters)[:3] == ["X", "W0", "H0"] and sig.parameters["route"].default is None
    assert list(inspect.signature(evc.compact_dictionary).parameters)[-1] == "beta"
    assert inspect.signature(evc.compact_dictionary).parameters["beta"].default is None
    for loss in ("itakura-saito", 0, 0.5, 1, "frobenius", np.float64(3.0), np.int64(-1)):
        _runs_or_refuses(lambda: fz.non_negative_factorization_beta(X, W0, D, loss, tol=0, max_iter=2))
    _runs_or_refuses(lambda: evc.learn_dictionary_beta(X, D, W0, beta=0.0, layout="frame_major", iters=2))
    _runs_or_refuses(lambda: evc.compact_dictionary(X[:3], X[3:], 2, iters=2, beta=0))


def test_python_surface_refusals():
    import exemplars_vc_amd as evc
    from exemplars_vc_amd.compat import factorize as fz
    X, D, W0 = _small()
    Xz = X.copy()
    Xz[2, 1] = 0.0
    for loss in ("itakura-saito", 0, -0.5):                  # scikit-learn's refusal, before anything runs
        with pytest.raises(ValueError, match=ZERO_MSG):
            fz.non_negative_factorization_beta(Xz, W0, D, loss)
    for loss in ("bogus", float("nan"), float("inf"), True, None, [0.5]):
        with pytest.raises(ValueError, match="Invalid beta_loss parameter"):
            fz.non_negative_factorization_beta(X, W0, D, loss)
    with pytest.raises(ValueError, match="528"):
        evc.learn_dictionary_beta(np.ones((3, 529)), np.ones((2, 529)), np.ones((3, 2)), beta=0.5, layout="frame_major",
                                  iters=1)
    with pytest.raises(ValueError, match="528"):
        evc.learn_dictionary_beta(np.ones((529, 3)), np.ones((529, 2)), np.ones((2, 3)), beta=0.5, layout="bin_major",
                                  iters=1)
    with pytest.raises(ValueError, match="528"):
        fz.non_negative_factorization_beta(np.ones((3, 529)), np.ones((3, 2)), np.ones((2, 529)), 0.5)
    with pytest.raises(ValueError, match="finite"):
        evc.learn_dictionary_beta(X, D, W0, beta=float("nan"), layout="frame_major", iters=1)
    with pytest.raises(ValueError, match="route"):
        evc.learn_dictionary_beta(X, D, W0, beta=0.5, layout="frame_major", iters=1, route="both")
    for kw in (dict(loss="kl"), dict(loss="kullback-leibler"), dict(solver="cd")):
        with pytest.raises(ValueError, match="beta names the loss"):
            evc.compact_dictionary(X[:3], X[3:], 2, beta=0, **kw)
    # the old entry points keep their pinned refusals
    with pytest.raises(ValueError, match="loss"):
        evc.learn_dictionary(X, D, W0, layout="frame_major", iters=1, loss="itakura-saito")
    for loss in ("itakura-saito", 0, 0.5):
        with pytest.raises(ValueError, match="beta_loss"):
            fz.non_negative_factorization_mu(X, W0, D, beta_loss=loss)
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            evc.learn_dictionary_beta(X, D, W0, beta=0.5, layout="frame_major", iters=1)
