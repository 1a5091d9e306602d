"""Beta-divergence activation solve (evc_beta_solve), host side: the C ABI's declarations, struct mirror and argument
checks, the numpy restatement against scikit-learn's recorded results (tests/golden/betamu_*.npz), the fixture generator
and the Python surface's validation.  No GPU needed."""
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
import beta_restatement as br  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "betamu_*.npz")))
ZERO_MSG = "When beta_loss <= 0 and X contains zeros, the solver may diverge"


def lib():
    from exemplars_vc_amd import _lib
    return _lib, _lib.lib()


def _reg(d):
    M = d["X_rows"].shape[1]
    a, r = float(d["alpha_W"]), float(d["l1_ratio"])
    return M * a * r, M * a * (1 - r)


def test_beta_symbols_declared_and_exported():
    _lib, L = lib()
    hdr = open(os.path.join(ROOT, "include", "evc.h")).read()
    declared = set(re.findall(r"\b(evc_[a-z_0-9]+)\s*\(", hdr))
    for sym in ("evc_beta_solve", "evc_beta_workspace_bytes"):
        assert sym in declared and sym in _lib.SYMBOLS and hasattr(L, sym)
    assert "evc_beta_solve" in hdr[:hdr.index("#ifndef EVC_H")]          # listed in the header comment
    sync = hdr[hdr.index("Host synchronisation"):hdr.index("No global mutable state")]
    assert "(8) evc_beta_solve" in sync
    assert L.evc_version() == 100


def test_beta_opts_mirror_matches_header():
    _lib, _ = lib()
    hdr = open(os.path.join(ROOT, "include", "evc.h")).read()
    body = hdr[hdr.index("typedef struct evc_beta_opts {"):hdr.index("} evc_beta_opts;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for grp in re.findall(r"\b(?:int|double|void\*)\s+([a-zA-Z_0-9, ]+);", body)
             for n in grp.replace(" ", "").split(",")]
    assert names == [f[0] for f in _lib.BetaOpts._fields_]
    assert names == ["struct_bytes", "dtype", "layout", "iters", "init_mode", "check_every", "stop_rule", "reserved",
                     "beta", "tol", "l1", "l2", "init_value", "ev_loop_start", "ev_loop_stop"]
    assert C.sizeof(_lib.BetaOpts) == 8 * 4 + 5 * 8 + 2 * 8


def _opts(_lib, **kw):
    o = _lib.BetaOpts()
    o.struct_bytes = C.sizeof(_lib.BetaOpts)
    o.dtype, o.layout, o.init_mode, o.iters, o.beta = _lib.F64, _lib.FRAME_MAJOR, _lib.INIT_SKLEARN, 5, 0.5
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_beta_bad_arguments_rejected_before_device_work():
    _lib, L = lib()
    one = C.c_void_p(8)              # never dereferenced: every case fails validation first

    def call(o, M=25, N=64, T=10, lda=25, ldx=25, ldh=64, offs=None, n_utt=1, ws=1 << 40, A=one):
        return L.evc_beta_solve(A, lda, one, ldx, one, ldh, M, N, T, offs, n_utt, C.byref(o), one, ws, None, None, None)
    bad = _opts(_lib)
    bad.struct_bytes = 4
    assert call(bad) == -1
    assert L.evc_beta_solve(one, 25, one, 25, one, 64, 25, 64, 10, None, 1, None, one, 1 << 40, None, None, None) == -1
    assert call(_opts(_lib), M=0) == -1
    assert call(_opts(_lib), N=0) == -1
    assert call(_opts(_lib), T=-1) == -1
    assert call(_opts(_lib), lda=24) == -1
    assert call(_opts(_lib), ldx=24) == -1
    assert call(_opts(_lib), ldh=63) == -1
    assert call(_opts(_lib, layout=_lib.BIN_MAJOR), lda=63, ldx=10, ldh=10) == -1
    assert call(_opts(_lib), A=None) == -1
    for v in (float("nan"), float("inf"), -float("inf")):
        assert call(_opts(_lib, beta=v)) == -1
    assert call(_opts(_lib, tol=-1e-4)) == -1
    assert call(_opts(_lib, tol=float("nan"))) == -1
    assert call(_opts(_lib, iters=-1)) == -1
    assert call(_opts(_lib, check_every=-1)) == -1
    assert call(_opts(_lib, iters=5000, check_every=1)) == -1      # more error slots than the workspace holds
    assert call(_opts(_lib, l1=-1.0)) == -1
    assert call(_opts(_lib, l2=-1.0)) == -1
    assert call(_opts(_lib, init_value=float("nan"))) == -1
    assert call(_opts(_lib, dtype=7)) == -1
    assert call(_opts(_lib, layout=5)) == -1
    assert call(_opts(_lib, init_mode=3)) == -1
    assert call(_opts(_lib, stop_rule=_lib.STOP_PYMF)) == -1
    assert call(_opts(_lib, reserved=1)) == -1
    offs = (C.c_int * 3)(0, 4, 9)                                 # does not end at T
    assert call(_opts(_lib), offs=offs, n_utt=2) == -1
    assert call(_opts(_lib), n_utt=2) == -1                       # n_utt > 1 needs offsets
    assert call(_opts(_lib), ws=16) == -2                         # workspace too small
    assert call(_opts(_lib), M=529, lda=529, ldx=529) == -3       # beyond the two LDS images
    assert call(_opts(_lib), M=529, lda=529, ldx=529, ws=16) == -3


def test_beta_workspace_queries():
    _lib, L = lib()
    q = L.evc_beta_workspace_bytes
    assert q(25, 512, 688, 1, _lib.F64) < q(25, 4096, 688, 1, _lib.F64) < q(25, 4096, 6880, 1, _lib.F64)
    assert q(25, 4096, 688, 1, _lib.F64) < q(25, 4096, 688, 10, _lib.F64)
    assert q(513, 4096, 688, 1, _lib.F64) > q(25, 4096, 688, 1, _lib.F64)
    assert q(201, 4096, 688, 1, _lib.F32) < q(201, 4096, 688, 1, _lib.F64)
    assert q(528, 1, 0, 1, 0) > 0 and q(529, 1, 1, 1, 0) == 0
    assert q(0, 1, 1, 1, 0) == 0 and q(25, 0, 1, 1, 0) == 0 and q(25, 1, -1, 1, 0) == 0
    assert q(25, 1, 1, 0, 0) == 0 and q(25, 1, 1, 1, 9) == 0


def test_fixture_table():
    """the cases the fixtures must cover: every T no multiple of 16, the five fixed-K betas, four early stops, the widths"""
    names = [os.path.basename(p)[:-4] for p in FILES]
    for beta in ("bm1", "b0", "b0p5", "b1p5", "b3"):
        assert f"betamu_m25_n64_t32_k50_{beta}" in names
    stops = {}
    for p in FILES:
        d = np.load(p)
        assert os.path.getsize(p) <= 1 << 20
        assert d["X_rows"].shape[0] % 16 != 0 or "t32" in p        # (25, 64, 32) is the issue's own fixed-K shape
        assert (d["X_rows"] >= 0).all() and (d["W_rows"] >= 0).all()
        if float(d["tol"]) > 0:
            stops[os.path.basename(p)] = int(d["n_iter"])
            assert int(d["n_iter"]) < int(d["max_iter"])
    assert len([s for s in stops if "m25_n64_t50" in s]) == 4
    shapes = {(d["X_rows"].shape[1], d["W_rows"].shape[0], d["X_rows"].shape[0]) for d in map(np.load, FILES)}
    assert {(1, 48, 37), (100, 47, 20), (201, 128, 40), (513, 96, 21), (25, 64, 50), (25, 64, 32)} <= shapes


@pytest.mark.parametrize("path", FILES, ids=os.path.basename)
def test_restatement_reproduces_sklearn_fixture(path):
    d = np.load(path)
    l1, l2 = _reg(d)
    W, n_iter, trace = br.beta_solve(d["X_rows"], d["W_rows"], float(d["beta"]), int(d["max_iter"]), float(d["tol"]), l1, l2)
    assert W.dtype == d["H"].dtype == np.dtype(str(d["dtype"]))
    assert n_iter == int(d["n_iter"])
    ref = d["H"].T
    assert np.linalg.norm(W.astype(np.float64) - ref) / np.linalg.norm(ref) <= 1e-12
    seen = ~np.isnan(d["err"])
    np.testing.assert_allclose(trace[seen], d["err"][seen], rtol=1e-12, atol=0)
    assert np.isnan(trace[1:][~seen[1:]]).all()


def test_early_stop_margins():
    """every evaluated check of an early-stop fixture sits at least 1 % of tol off the threshold"""
    n = 0
    for p in FILES:
        d = np.load(p)
        tol = float(d["tol"])
        if tol == 0:
            continue
        k = int(d["n_iter"]) // 10
        e = d["err"]
        dec = (e[:k] - e[1:k + 1]) / e[0]
        assert (dec[:-1] >= tol).all() and dec[-1] < tol
        assert np.min(np.abs(dec - tol)) >= 0.01 * tol, p
        n += 1
    assert n >= 6


def test_zeros_fixture_properties():
    for beta in ("b0p5", "b1p5"):
        d = np.load(os.path.join(GOLDEN, f"betamu_m25_n64_t50_zeros_{beta}.npz"))
        assert (d["X_rows"][3] == 0).all() and (d["X_rows"][:, 5] == 0).all() and (d["W_rows"][7] == 0).all()
        assert (d["H"][:, 3] == 0).all() and (d["H"][7] == 0).all() and np.isfinite(d["H"]).all()


def test_restatement_one_and_two_agree_with_the_special_cased_updates():
    """beta = 1 and beta = 2 through the generic statement: scikit-learn's special-cased results to rounding"""
    kl = np.load(os.path.join(GOLDEN, "sklearnkl_m25_n64_t50_tol2e-2.npz"))
    W, n_iter, _ = br.beta_solve(kl["X_rows"], kl["W_rows"], 1.0, int(kl["max_iter"]), float(kl["tol"]))
    assert n_iter == int(kl["n_iter"]) and np.linalg.norm(W.T - kl["H"]) / np.linalg.norm(kl["H"]) <= 1e-9
    fr = np.load(os.path.join(GOLDEN, "sklearn_m25_n64_t50_tol5e-2.npz"))
    W, n_iter, _ = br.beta_solve(fr["X_rows"], fr["W_rows"], 2.0, int(fr["max_iter"]), float(fr["tol"]))
    assert n_iter == int(fr["n_iter"]) and np.linalg.norm(W.T - fr["H"]) / np.linalg.norm(fr["H"]) <= 1e-9


def test_generator_reproduces_the_fixtures():
    pytest.importorskip("sklearn")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_golden_beta as g
    specs = g.cases()
    assert sorted(specs) == sorted(os.path.basename(p)[:-4] for p in FILES)
    for name in ("betamu_m25_n64_t32_k50_b0", "betamu_m25_n64_t50_b3_tol2e-2", "betamu_m1_n48_t37_b0p5",
                 "betamu_m25_n64_t50_zeros_b1p5", "betamu_m25_n64_t50_reg_b0p5", "betamu_m25_n64_t32_b0_f32"):
        out = g.make(name, specs[name])
        ref = np.load(os.path.join(GOLDEN, name + ".npz"))
        for k, v in out.items():
            v = np.asarray(v)
            assert np.array_equal(np.asarray(ref[k]), v, equal_nan=v.dtype.kind == "f"), (name, k)


def _small():
    rng = np.random.default_rng(0)
    return rng.random((6, 4)) + 0.1, rng.random((5, 4)) + 0.1, rng.random((6, 5)) + 0.1      # X, dictionary, activations


def _runs_or_refuses(fn, shape):
    """with a device the call answers; without one it refuses (there is no CPU fallback)"""
    import torch
    if torch.cuda.is_available():
        assert np.asarray(fn()).shape == shape
    else:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn()


def test_python_surface_accepts_the_new_losses():
    import exemplars_vc_amd as evc
    from exemplars_vc_amd.compat import factorize as fz
    X, D, W0 = _small()
    assert "solve_activations_beta" in evc.__all__
    for loss in ("itakura-saito", 0, 0.5, 1.5, np.float64(3.0), np.int64(-1)):
        _runs_or_refuses(lambda: fz._factorize(X, D, beta_loss=loss, tol=0, honor_beta_loss=True), (5, 6))
        _runs_or_refuses(lambda: fz.non_negative_factorization_mu(X, W0, D, update_H=False, tol=0, max_iter=3,
                                                                  beta_loss=loss)[0], (6, 5))
    _runs_or_refuses(lambda: evc.solve_activations_beta(D, X, beta=0.5, layout="frame_major", iters=2), (6, 5))
    assert fz._beta_of(0) == 0.0 and fz._beta_of("itakura-saito") == 0.0 and fz._beta_of(np.float32(0.5)) == 0.5
    assert fz._beta_of("kullback-leibler") == 1.0 and fz._beta_of(2) == 2.0


def test_python_surface_refusals():
    import exemplars_vc_amd as evc
    from exemplars_vc_amd.compat import factorize as fz
    X, D, W0 = _small()
    Xz = X.copy()
    Xz[2, 1] = 0.0
    for loss in ("itakura-saito", 0, -0.5):                  # scikit-learn's refusal, before anything runs
        with pytest.raises(ValueError, match=ZERO_MSG):
            fz._factorize(Xz, D, beta_loss=loss, honor_beta_loss=True)
        with pytest.raises(ValueError, match=ZERO_MSG):
            fz.non_negative_factorization_mu(Xz, W0, D, update_H=False, beta_loss=loss)
    for loss in ("bogus", float("nan"), float("inf"), True, None, [0.5]):
        with pytest.raises(ValueError, match="Invalid beta_loss parameter"):
            fz._factorize(X, D, beta_loss=loss, honor_beta_loss=True)
        with pytest.raises(ValueError, match="Invalid beta_loss parameter"):
            fz.non_negative_factorization_mu(X, W0, D, update_H=False, beta_loss=loss)
    # dictionary learning under other betas stays out: the two refusals tests/test_learn_kl_host.py pins
    with pytest.raises(ValueError, match="loss"):
        evc.learn_dictionary(X, D, W0, layout="frame_major", iters=1, loss="itakura-saito")
    for loss in ("itakura-saito", 0, 0.5):
        with pytest.raises(ValueError, match="beta_loss"):
            fz.non_negative_factorization_mu(X, W0, D, beta_loss=loss)
    params = list(inspect.signature(fz.non_negative_factorization_mu).parameters.values())
    assert params[-1].name == "beta_loss" and params[-1].default == "frobenius"
    for name in ("alpha_W", "l1_ratio"):
        assert name not in inspect.signature(fz.non_negative_factorization_mu).parameters
        assert name not in inspect.signature(fz._factorize).parameters
    # the shapes the ABI answers with -3, and a non-finite beta
    with pytest.raises(ValueError, match="528"):
        evc.solve_activations_beta(np.ones((3, 529)), np.ones((2, 529)), beta=0.5, layout="frame_major")
    with pytest.raises(ValueError, match="528"):
        evc.solve_activations_beta(np.ones((529, 3)), np.ones((529, 2)), beta=0.5, layout="bin_major")
    with pytest.raises(ValueError, match="finite"):
        evc.solve_activations_beta(D, X, beta=float("nan"), layout="frame_major")


def test_sklearn_refuses_zeros_on_this_route():
    sk = pytest.importorskip("sklearn.decomposition")
    X, D, _ = _small()
    X[2, 1] = 0.0
    with pytest.raises(ValueError, match=ZERO_MSG):
        sk.non_negative_factorization(X=X, H=D, init="custom", update_H=False, n_components=5, beta_loss=0, solver="mu")
