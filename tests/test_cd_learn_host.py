"""Coordinate descent that also learns the dictionary (evc_cd_learn), host side: the numpy restatement of the blocked,
split-sum algebra against scikit-learn's recorded results, the fixture generator, and the C ABI's declarations, struct
mirror and argument checks.  No GPU needed."""
import ctypes as C
import glob
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cd_learn_restatement import cd_learn, dict_sweep, split_sum  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "cdlearn_*.npz")))
F64_FILES = [p for p in FILES if not p.endswith("_f32.npz")]
F32_FILES = [p for p in FILES if p.endswith("_f32.npz")]


def penalties(d):
    """(l1_h, l2_h, l1_w, l2_w) as sklearn's _compute_regularization scales them (alpha_H = 'same')"""
    T, M = d["X_rows"].shape
    a, r = float(d["alpha_W"]), float(d["l1_ratio"])
    return M * a * r, M * a * (1 - r), T * a * r, T * a * (1 - r)


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


def lib():
    from exemplars_vc_amd import _lib
    return _lib, _lib.lib()


def test_fixture_set():
    names = [os.path.basename(p)[:-4] for p in FILES]
    assert len(F64_FILES) == 10 and len(F32_FILES) == 2
    for p in FILES:
        assert os.path.getsize(p) <= 1 << 20
    for n in names:                                  # well posed: R < min(M, T), apart from the tiny cases
        M, R, T = (int(x) for x in re.match(r"cdlearn_m(\d+)_r(\d+)_t(\d+)", n).groups())
        assert R < min(M, T) or M in (1, 6)
    stops = {n: int(np.load(os.path.join(GOLDEN, n + ".npz"))["n_iter"]) for n in names}
    assert 1 < stops["cdlearn_m25_r17_t70_early"] < 200 and 100 < stops["cdlearn_m50_r33_t520_late"] < 200
    assert stops["cdlearn_m1_r1_t40"] == 2


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("path", F64_FILES, ids=[os.path.basename(p)[:-4] for p in F64_FILES])
def test_restatement_reproduces_sklearn(path, S):
    d = np.load(path)
    l1_h, l2_h, l1_w, l2_w = penalties(d)
    W, H, n_iter, viol = cd_learn(d["X_rows"], d["W0_rows"], d["H0_rows"], int(d["max_iter"]), float(d["tol"]), l1_h, l2_h,
                                  l1_w, l2_w, S=S)
    ref = d["violation"]
    print(os.path.basename(path), S, n_iter, rel(W, d["W_rows"]), rel(H, d["H_rows"]),
          np.abs(viol[:n_iter] - ref).max() / ref[0].sum())
    assert n_iter == int(d["n_iter"])
    assert rel(W, d["W_rows"]) <= 1e-9 and rel(H, d["H_rows"]) <= 1e-9
    assert np.abs(viol[:n_iter] - ref).max() <= 1e-9 * ref[0].sum()
    assert np.isnan(viol[n_iter:]).all()


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("path", F32_FILES, ids=[os.path.basename(p)[:-4] for p in F32_FILES])
def test_restatement_float32_is_close_to_sklearn_float64(path, S):
    d = np.load(path)
    assert d["X_rows"].dtype == np.float32
    W, H, n_iter, _ = cd_learn(d["X_rows"], d["W0_rows"], d["H0_rows"], int(d["max_iter"]), float(d["tol"]), S=S,
                               dtype=np.float32)
    print(os.path.basename(path), S, rel(W, d["W_rows_f64"]), rel(H, d["H_rows_f64"]))
    assert W.dtype == np.float32 and n_iter == int(d["n_iter_f64"])
    assert rel(W, d["W_rows_f64"]) <= 1e-4 and rel(H, d["H_rows_f64"]) <= 1e-4


def test_restatement_pieces():
    rng = np.random.default_rng(0)
    X, H = rng.random((37, 9)), rng.random((37, 5))
    assert np.allclose(split_sum(X, H, 4), X.T @ H, rtol=1e-14)
    # one exact coordinate minimisation per component: a second sweep from the optimum of a rank-1 fit changes nothing
    h = rng.random((20, 1)) + 0.1
    w = rng.random((1, 6)) + 0.1
    W = np.full((6, 1), 0.3)
    v1 = dict_sweep(h @ w, h, W)
    assert v1 > 0 and np.allclose(W[:, 0], w[0], rtol=1e-12)
    assert dict_sweep(h @ w, h, W) <= 1e-12 * v1
    # update="dict" leaves the activations alone
    W2, H2, n, viol = cd_learn(X, rng.random((5, 9)), H, 3, 0.0, update="dict")
    assert np.array_equal(H2, H) and n == 3 and (viol[:, 0] == 0).all() and (viol[:, 1] > 0).all()


def test_generator_reproduces_the_fixtures():
    pytest.importorskip("sklearn")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_golden_cd_learn as g
    specs = g.cases()
    assert sorted(specs) == sorted(os.path.basename(p)[:-4] for p in FILES)
    for name, spec in specs.items():
        if spec[0].shape[0] * spec[3] > 300 * 200:     # the long ones are left to `--check`
            continue
        out = g.make(spec)
        ref = np.load(os.path.join(GOLDEN, name + ".npz"))
        for k, v in out.items():
            assert np.array_equal(np.asarray(ref[k]), np.asarray(v)), (name, k)


def test_symbols_declared_and_exported():
    _lib, L = lib()
    hdr = open(os.path.join(ROOT, "include", "evc.h")).read()
    declared = set(re.findall(r"\b(evc_[a-z_0-9]+)\s*\(", hdr))
    for sym in ("evc_cd_learn", "evc_cd_learn_workspace_bytes", "evc_cd_learn_splits"):
        assert sym in declared and sym in _lib.SYMBOLS and hasattr(L, sym)
    assert "evc_cd_learn" in hdr[:hdr.index("#ifndef EVC_H")]
    sync = hdr[hdr.index("Host synchronisation"):hdr.index("No global mutable state")]
    assert "(6) evc_cd_learn" in sync


def test_opts_mirror_matches_header():
    _lib, _ = lib()
    hdr = open(os.path.join(ROOT, "include", "evc.h")).read()
    body = hdr[hdr.index("typedef struct evc_cd_learn_opts {"):hdr.index("} evc_cd_learn_opts;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for grp in re.findall(r"\b(?:int|double|void\*)\s+([a-zA-Z_0-9, ]+);", body)
             for n in grp.replace(" ", "").split(",")]
    assert names == [f[0] for f in _lib.CdLearnOpts._fields_]
    assert C.sizeof(_lib.CdLearnOpts) == 6 * 4 + 5 * 8 + 2 * 8
    assert (_lib.CDL_BOTH, _lib.CDL_DICT_ONLY) == (0, 1)
    assert re.search(r"EVC_CDL_BOTH = 0, EVC_CDL_DICT_ONLY = 1", hdr)


def _opts(_lib, **kw):
    o = _lib.CdLearnOpts()
    o.struct_bytes = C.sizeof(_lib.CdLearnOpts)
    o.dtype, o.layout, o.max_iter, o.tol = _lib.F64, _lib.FRAME_MAJOR, 5, 1e-4
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_bad_arguments_rejected_before_device_work():
    _lib, L = lib()
    one = C.c_void_p(8)              # never dereferenced: every case fails validation first

    def call(o, M=25, R=17, T=70, ldx=25, ldw=25, ldh=17, ws=1 << 30):
        return L.evc_cd_learn(one, ldx, one, ldw, one, ldh, M, R, T, C.byref(o) if o is not None else None, one, ws, None,
                              None, None)
    bad = _opts(_lib)
    bad.struct_bytes = 4
    assert call(bad) == -1
    assert call(None) == -1
    for kw in (dict(M=0), dict(R=0), dict(T=0), dict(ldx=24), dict(ldw=24), dict(ldh=16)):
        assert call(_opts(_lib), **kw) == -1, kw
    for kw in (dict(tol=-1e-4), dict(tol=float("nan")), dict(max_iter=-1), dict(l1_h=-1.0), dict(l2_h=-1.0), dict(l1_w=-1.0),
               dict(l2_w=-1.0), dict(dtype=7), dict(layout=5), dict(update=2), dict(update=-1), dict(reserved=1),
               dict(reserved=65 << 8), dict(reserved=1 << 16)):
        assert call(_opts(_lib, **kw)) == -1, kw
    assert call(_opts(_lib), ws=16) == -2                                     # workspace too small
    need = L.evc_cd_learn_workspace_bytes(25, 17, 70, _lib.F64)
    assert L.evc_cd_learn_splits(25, 17, 70) == 1
    assert call(_opts(_lib, reserved=7 << 8), ws=need) == -2                  # forced ranges need their slabs
    assert call(_opts(_lib), M=1025, ldx=1025, ldw=1025) == -3                # beyond k_cd_sweep's bins per frame
    assert call(_opts(_lib), R=1025, ldh=1025) == -3                          # beyond the dictionary sweep's components


def test_size_queries():
    _lib, L = lib()
    q, sp = L.evc_cd_learn_workspace_bytes, L.evc_cd_learn_splits
    assert q(25, 17, 70, _lib.F64) > 0 and q(1, 1, 1, _lib.F32) > 0 and q(1024, 1024, 1100, _lib.F64) > 0
    assert q(50, 512, 65536, _lib.F32) < q(50, 512, 65536, _lib.F64)
    assert q(50, 64, 4096, _lib.F64) < q(50, 512, 4096, _lib.F64) < q(50, 512, 65536, _lib.F64)
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1025, 1, 1), (1, 1025, 1)):
        assert q(*bad, _lib.F64) == 0 and sp(*bad) == 0, bad
    assert q(25, 17, 70, 9) == 0
    assert sp(50, 33, 520) == 2 and sp(1, 1, 1) == 1 and 1 <= sp(1024, 1024, 1 << 20) <= 64
    # the slabs are sized by the ranges in use, not by the 64 a forced count may ask for: at R = 1024 in float64 a slab of
    # G is 8 MB, and the whole workspace of a one-range call stays below what 64 ranges of that slab alone would take
    assert sp(64, 1024, 300) == 1 and q(64, 1024, 300, _lib.F64) < 40 * (1 << 20)


def test_python_entry_points_validate_before_the_device():
    import exemplars_vc_amd as evc
    from exemplars_vc_amd.compat import factorize_cd as fcd
    assert "learn_dictionary_cd" in evc.__all__
    X = np.ones((6, 4))
    with pytest.raises(ValueError, match="update must be"):
        evc.learn_dictionary_cd(X, np.ones((3, 4)), np.ones((6, 3)), layout="frame_major", update="h")
    with pytest.raises(ValueError, match="solver must be"):
        evc.compact_dictionary(np.ones((4, 8)), np.ones((3, 8)), 2, solver="als")
    with pytest.raises(ValueError, match="Frobenius"):
        evc.compact_dictionary(np.ones((4, 8)), np.ones((3, 8)), 2, solver="cd", loss="kl")
    with pytest.raises(ValueError, match="wrong second dimension"):
        fcd.non_negative_factorization_cd(X, np.ones((6, 3)), np.ones((3, 5)))
    with pytest.raises(ValueError, match="wrong shape"):
        fcd.non_negative_factorization_cd(X, np.ones((5, 3)), np.ones((3, 4)))
    with pytest.raises(TypeError, match="same dtype"):
        fcd.non_negative_factorization_cd(X, np.ones((6, 3), np.float32), np.ones((3, 4)))


def test_learn_without_a_device_raises():
    import torch
    if torch.cuda.is_available():
        return                       # with a device the call succeeds: tests/test_gpu_cd_learn.py
    import exemplars_vc_amd as evc
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evc.learn_dictionary_cd(np.ones((6, 4)), np.ones((3, 4)), np.ones((6, 3)), layout="frame_major")
