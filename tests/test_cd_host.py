"""Coordinate-descent solve (evc_cd_solve), host side: the C ABI's declarations, struct mirror and argument checks,
the numpy restatement of the blocked factored algebra against scikit-learn's recorded results, the fixture
generator, and the compat layer's validation.  No GPU needed."""
import ctypes as C
import glob
import os
import re
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cd_restatement import cd_iterations, cd_solve  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CD_FILES = sorted(glob.glob(os.path.join(GOLDEN, "cdnmf_*.npz")))


def lib():
    from exemplars_vc_amd import _lib
    return _lib, _lib.lib()


def test_cd_symbols_declared_and_exported():
    _lib, L = lib()
    hdr = open(os.path.join(ROOT, "include", "evc.h")).read()
    declared = set(re.findall(r"\b(evc_[a-z_0-9]+)\s*\(", hdr))
    for sym in ("evc_cd_solve", "evc_cd_workspace_bytes"):
        assert sym in declared and sym in _lib.SYMBOLS and hasattr(L, sym)
    assert "evc_cd_solve" in hdr[:hdr.index("#ifndef EVC_H")]          # listed in the header comment
    sync = hdr[hdr.index("Host synchronisation"):hdr.index("No global mutable state")]
    assert "evc_cd_solve" in sync


def test_cd_opts_mirror_matches_header():
    _lib, _ = lib()
    hdr = open(os.path.join(ROOT, "include", "evc.h")).read()
    body = hdr[hdr.index("typedef struct evc_cd_opts {"):hdr.index("} evc_cd_opts;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for grp in re.findall(r"\b(?:int|double|void\*)\s+([a-zA-Z_0-9, ]+);", body)
             for n in grp.replace(" ", "").split(",")]
    assert names == [f[0] for f in _lib.CdOpts._fields_]
    assert C.sizeof(_lib.CdOpts) == 6 * 4 + 3 * 8 + 2 * 8


def _opts(_lib, **kw):
    o = _lib.CdOpts()
    o.struct_bytes = C.sizeof(_lib.CdOpts)
    o.dtype, o.layout, o.init_mode, o.max_iter, o.tol = _lib.F64, _lib.FRAME_MAJOR, _lib.INIT_SKLEARN, 5, 1e-4
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_cd_bad_arguments_rejected_before_device_work():
    _lib, L = lib()
    one = C.c_void_p(8)              # never dereferenced: every case fails validation first

    def call(o, M=25, N=64, T=10, lda=25, ldx=25, ldh=64, offs=None, n_utt=1, ws=1 << 30):
        return L.evc_cd_solve(one, lda, one, ldx, one, ldh, M, N, T, offs, n_utt, C.byref(o), one, ws, None, None,
                              None)
    bad = _opts(_lib)
    bad.struct_bytes = 4
    assert call(bad) == -1
    assert call(_opts(_lib), M=0) == -1
    assert call(_opts(_lib), N=0) == -1
    assert call(_opts(_lib), lda=24) == -1
    assert call(_opts(_lib), ldx=24) == -1
    assert call(_opts(_lib), ldh=63) == -1
    assert call(_opts(_lib, tol=-1e-4)) == -1
    assert call(_opts(_lib, tol=float("nan"))) == -1
    assert call(_opts(_lib, max_iter=-1)) == -1
    assert call(_opts(_lib, l1=-1.0)) == -1
    assert call(_opts(_lib, l2=-1.0)) == -1
    assert call(_opts(_lib, dtype=7)) == -1
    assert call(_opts(_lib, layout=5)) == -1
    assert call(_opts(_lib, init_mode=_lib.INIT_CONST)) == -1
    assert call(_opts(_lib, reserved=1)) == -1
    offs = (C.c_int * 3)(0, 4, 9)                                 # does not end at T
    assert call(_opts(_lib), offs=offs, n_utt=2) == -1
    assert call(_opts(_lib), n_utt=2) == -1                       # n_utt > 1 needs offsets
    assert call(_opts(_lib), ws=16) == -2                         # workspace too small
    assert call(_opts(_lib), M=5000, lda=5000, ldx=5000) == -3    # beyond the kernel's bins per frame


def test_cd_workspace_queries():
    _lib, L = lib()
    q = L.evc_cd_workspace_bytes
    assert q(25, 512, 688, 1, _lib.F64) < q(25, 4096, 688, 1, _lib.F64) < q(25, 4096, 6880, 1, _lib.F64)
    assert q(25, 4096, 688, 1, _lib.F64) < q(25, 4096, 688, 10, _lib.F64)
    assert q(513, 4096, 688, 1, _lib.F64) > q(25, 4096, 688, 1, _lib.F64)
    assert q(201, 4096, 688, 1, _lib.F32) < q(201, 4096, 688, 1, _lib.F64)
    assert q(0, 1, 1, 1, 0) == 0 and q(25, 0, 1, 1, 0) == 0 and q(25, 1, -1, 1, 0) == 0
    assert q(25, 1, 1, 0, 0) == 0 and q(25, 1, 1, 1, 9) == 0 and q(5000, 1, 1, 1, 0) == 0


def _reg(d):
    M = d["X_rows"].shape[1]
    a, r = float(d["alpha_W"]), float(d["l1_ratio"])
    return M * a * r, M * a * (1 - r)


@pytest.mark.parametrize("path", [p for p in CD_FILES if not p.endswith("_f32.npz")], ids=os.path.basename)
def test_restatement_reproduces_sklearn_fixture(path):
    d = np.load(path)
    l1, l2 = _reg(d)
    H, n_iter, viol = cd_solve(d["X_rows"], d["W_rows"], int(d["max_iter"]), float(d["tol"]), l1, l2)
    assert n_iter == int(d["n_iter"])
    ref = d["H"].T
    den = max(np.linalg.norm(ref), 1e-300)
    assert np.linalg.norm(H - ref) / den <= 1e-12 or np.linalg.norm(ref) == 0 and np.linalg.norm(H) == 0
    np.testing.assert_allclose(viol, d["violation"], rtol=1e-9, atol=0)


def test_restatement_float32_is_close_to_sklearn_float64():
    paths = [p for p in CD_FILES if p.endswith("_f32.npz")]
    assert len(paths) >= 2
    for path in paths:
        d = np.load(path)
        H, n_iter, _ = cd_solve(d["X_rows"], d["W_rows"], 200, float(d["tol"]), dtype=np.float32)
        ref = d["H_f64"].T
        assert np.linalg.norm(H - ref) / np.linalg.norm(ref) <= 1e-4, path
        assert abs(n_iter - int(d["n_iter"])) <= 1, path


def test_restatement_warm_start_continues_the_trajectory():
    d = np.load(os.path.join(GOLDEN, "cdnmf_m25_n64_t32.npz"))
    H5, _ = cd_iterations(d["X_rows"], d["W_rows"], 5)
    H3, _ = cd_iterations(d["X_rows"], d["W_rows"], 3)
    H3_2, _ = cd_iterations(d["X_rows"], d["W_rows"], 2, H0=H3)
    # the warm start re-forms r = h A - x from scratch: the trajectory goes on up to rounding
    assert np.linalg.norm(H3_2 - H5) / np.linalg.norm(H5) <= 1e-12


def test_fixture_names_stay_out_of_the_mu_globs():
    for p in CD_FILES:
        b = os.path.basename(p)
        assert not b.startswith(("sklearn_", "sklearnkl_", "pymf_", "pymfw_", "gl_"))
        assert os.path.getsize(p) <= 1 << 20


def test_generator_reproduces_the_fixtures():
    pytest.importorskip("sklearn")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_golden_cd as g
    specs, geo = g.cases(), g.geometry_cases()
    assert not set(specs) & set(geo)
    specs.update(geo)
    assert sorted(specs) == sorted(os.path.basename(p)[:-4] for p in CD_FILES)
    for name in ("cdnmf_m1_n48_t37", "cdnmf_m25_zero_utt", "cdnmf_m25_n64_t32_l1", "cdnmf_m6_n17_t70"):
        out = g.make(name, specs[name])
        ref = np.load(os.path.join(GOLDEN, name + ".npz"))
        for k, v in out.items():
            assert np.array_equal(np.asarray(ref[k]), np.asarray(v)), (name, k)


def test_compat_validation_mirrors_sklearn():
    from exemplars_vc_amd.compat import factorize_cd as fcd
    X = np.abs(np.random.default_rng(0).standard_normal((6, 4)))
    W = np.abs(np.random.default_rng(1).standard_normal((5, 4)))
    cases = [
        (dict(X=X, W=W[:, :3]), ValueError, "wrong second dimension"),
        (dict(X=X, W=np.zeros_like(W)), ValueError, "full of zeros"),
        (dict(X=X, W=-W), ValueError, "Negative values"),
        (dict(X=X, W=W.astype(np.float32)), TypeError, "same dtype"),
        (dict(X=X[0], W=W), ValueError, "Expected 2D array"),
    ]
    for kw, exc, msg in cases:
        with pytest.raises(exc, match=msg):
            fcd._factorize(kw["X"], kw["W"])
    sk = pytest.importorskip("sklearn.decomposition")
    for kw, exc, msg in cases:
        with pytest.raises(exc, match=msg), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sk.non_negative_factorization(X=kw["X"], H=kw["W"], init="custom", update_H=False,
                                          n_components=kw["W"].shape[0] if kw["W"].ndim == 2 else 1,
                                          beta_loss="frobenius", solver="cd", max_iter=200)


def test_solve_without_a_device_raises():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a HIP device is present")
    import exemplars_vc_amd as evc
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evc.solve_activations_cd(np.ones((4, 3)), np.ones((5, 4)), layout="frame_major")
