"""Dictionary learning (evc_nmf_learn), host side: the C ABI's declarations, struct mirror and argument checks, the numpy
restatement of the split factored update against scikit-learn's and pymf's recorded results, and the fixture generator.
No GPU needed."""
import ctypes as C
import glob
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from learn_restatement import learn, pymf_ferr  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
SK_FILES = sorted(glob.glob(os.path.join(GOLDEN, "dictmu_sk_*.npz")))
PYMF_FILES = sorted(glob.glob(os.path.join(GOLDEN, "dictmu_pymf_*.npz")) + glob.glob(os.path.join(GOLDEN, "pymfw_*.npz")))
RTOL = 1e-9         # the project's tolerance for the pymfw_ fixtures (test_gpu_parity.py)


def lib():
    from exemplars_vc_amd import _lib
    return _lib, _lib.lib()


def test_learn_symbols_declared_and_exported():
    _lib, L = lib()
    hdr = open(os.path.join(ROOT, "include", "evc.h")).read()
    declared = set(re.findall(r"\b(evc_[a-z_0-9]+)\s*\(", hdr))
    for sym in ("evc_nmf_learn", "evc_learn_workspace_bytes", "evc_learn_splits"):
        assert sym in declared and sym in _lib.SYMBOLS and hasattr(L, sym)
    assert "evc_nmf_learn" in hdr[:hdr.index("#ifndef EVC_H")]          # listed in the header comment
    sync = hdr[hdr.index("Host synchronisation"):hdr.index("No global mutable state")]
    assert "(5) evc_nmf_learn" in sync
    assert L.evc_version() == 100


def test_learn_opts_mirror_matches_header():
    _lib, _ = lib()
    hdr = open(os.path.join(ROOT, "include", "evc.h")).read()
    body = hdr[hdr.index("typedef struct evc_learn_opts {"):hdr.index("} evc_learn_opts;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for grp in re.findall(r"\b(?:int|double|void\*)\s+([a-zA-Z_0-9, ]+);", body)
             for n in grp.replace(" ", "").split(",")]
    assert names == [f[0] for f in _lib.LearnOpts._fields_]
    assert C.sizeof(_lib.LearnOpts) == 7 * 4 + 4 + 8 + 2 * 8
    assert (_lib.LEARN_SKLEARN, _lib.LEARN_PYMF) == (0, 1)
    assert re.search(r"EVC_LEARN_SKLEARN = 0, EVC_LEARN_PYMF = 1", hdr)


def _opts(_lib, **kw):
    o = _lib.LearnOpts()
    o.struct_bytes = C.sizeof(_lib.LearnOpts)
    o.dtype, o.layout, o.surface, o.iters, o.check_every = _lib.F64, _lib.BIN_MAJOR, _lib.LEARN_SKLEARN, 5, 0
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_learn_bad_arguments_rejected_before_device_work():
    _lib, L = lib()
    one = C.c_void_p(8)              # never dereferenced: every case fails validation first

    def call(o, M=25, R=12, T=40, ldx=None, ldw=None, ldh=None, ws=1 << 40):
        fm = o.layout == _lib.FRAME_MAJOR
        ldx = (M if fm else T) if ldx is None else ldx
        ldw = (M if fm else R) if ldw is None else ldw
        ldh = (R if fm else T) if ldh is None else ldh
        return L.evc_nmf_learn(one, ldx, one, ldw, one, ldh, M, R, T, C.byref(o), one, ws, None, None, None)
    bad = _opts(_lib)
    bad.struct_bytes = 4
    assert call(bad) == -1
    assert L.evc_nmf_learn(one, 40, one, 12, one, 40, 25, 12, 40, None, one, 1 << 40, None, None, None) == -1
    for lay in (_lib.BIN_MAJOR, _lib.FRAME_MAJOR):
        fm = lay == _lib.FRAME_MAJOR
        assert call(_opts(_lib, layout=lay), M=0) == -1
        assert call(_opts(_lib, layout=lay), R=0) == -1
        assert call(_opts(_lib, layout=lay), T=0) == -1
        assert call(_opts(_lib, layout=lay), ldx=(25 if fm else 40) - 1) == -1
        assert call(_opts(_lib, layout=lay), ldw=(25 if fm else 12) - 1) == -1
        assert call(_opts(_lib, layout=lay), ldh=(12 if fm else 40) - 1) == -1
    assert call(_opts(_lib, tol=-1e-4)) == -1
    assert call(_opts(_lib, tol=float("nan"))) == -1
    assert call(_opts(_lib, iters=-1)) == -1
    assert call(_opts(_lib, check_every=-1)) == -1
    assert call(_opts(_lib, surface=2)) == -1
    assert call(_opts(_lib, dtype=7)) == -1
    assert call(_opts(_lib, layout=5)) == -1
    assert call(_opts(_lib, reserved=65 << 8)) == -1              # a forced split above 64
    assert call(_opts(_lib, reserved=1)) == -1                    # bits outside 8..15
    assert call(_opts(_lib), ws=16) == -2                         # workspace too small
    assert call(_opts(_lib), M=1057) == -3
    assert call(_opts(_lib), R=4097) == -3
    assert call(_opts(_lib), M=1056, ws=16) == -2                 # the largest M is supported


def test_learn_workspace_and_split_queries():
    _lib, L = lib()
    q = L.evc_learn_workspace_bytes
    assert 0 < q(50, 512, 4096, _lib.F64) < q(50, 512, 65536, _lib.F64)
    assert q(50, 24, 150, _lib.F64) < q(402, 24, 150, _lib.F64)
    for bad in ((0, 1, 1, 0), (1, 0, 1, 0), (1, 1, 0, 0), (1, 1, -1, 0), (1057, 1, 1, 0), (1, 4097, 1, 0), (1, 1, 1, 9)):
        assert q(*bad) == 0
    s = L.evc_learn_splits
    assert s(50, 24, 150) == 1 and 1 < s(50, 512, 65536) <= 64 and s(0, 1, 1) == 0
    assert s(50, 512, 1 << 20) <= 64


def _check(got, want, what):
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=0, err_msg=what)


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("path", [p for p in SK_FILES if not p.endswith("_f32.npz")], ids=os.path.basename)
def test_restatement_reproduces_sklearn_fixture(path, S):
    d = np.load(path)
    tol = float(d["tol"])
    W, H, n_iter, _ = learn(d["X"], d["W0"], d["H0"], int(d["max_iter"]), "sklearn", 10 if tol > 0 else 0, tol, S=S)
    assert n_iter == int(d["n_iter"])
    _check(W, d["W"], "W")
    _check(H, d["H"], "H")
    if path.endswith("_zeros.npz"):          # the absent component stays absent, the silent frames stay silent
        assert not W[:, 5].any() and not H[5].any() and not H[:, [3, 77]].any()
        assert not np.asarray(d["W"])[:, 5].any() and not np.asarray(d["H"])[5].any()
    if path.endswith("_tol.npz"):
        assert 20 < n_iter < 100


def test_restatement_float32_is_close_to_sklearn_float32():
    paths = [p for p in SK_FILES if p.endswith("_f32.npz")]
    assert paths
    for path in paths:
        d = np.load(path)
        assert d["W"].dtype == np.float32
        W, H, n_iter, _ = learn(d["X"], d["W0"], d["H0"], int(d["max_iter"]), "sklearn", 0, 0.0, S=3, dtype=np.float32)
        assert n_iter == int(d["n_iter"]) and W.dtype == np.float32
        for got, ref in ((W, d["W"]), (H, d["H"])):
            assert np.linalg.norm(got.astype(float) - ref) / np.linalg.norm(ref) <= 1e-4


@pytest.mark.parametrize("S", [1, 7])
@pytest.mark.parametrize("path", PYMF_FILES, ids=os.path.basename)
def test_restatement_reproduces_pymf_fixture(path, S):
    d = np.load(path)
    niter, with_err = int(d["niter"]), bool(d["compute_err"])
    W, H, n_iter, err = learn(d["data"], d["W0"], d["H0"], niter, "pymf", 1 if with_err else 0,
                              np.finfo(float).eps if with_err else 0.0, S=S)
    _check(W, d["W"], "W")
    _check(H, d["H"], "H")
    if with_err:
        ferr = pymf_ferr(err, n_iter, niter)
        assert len(ferr) == len(d["ferr"])
        np.testing.assert_allclose(ferr, d["ferr"], rtol=1e-8)
    else:
        assert n_iter == niter


def test_fixture_names_and_sizes():
    assert len(SK_FILES) == 7 and len(glob.glob(os.path.join(GOLDEN, "dictmu_pymf_*.npz"))) == 2
    for p in glob.glob(os.path.join(GOLDEN, "dictmu_*.npz")):
        assert os.path.getsize(p) <= 1 << 20


def test_generator_reproduces_two_sklearn_fixtures():
    pytest.importorskip("sklearn")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_golden_learn as g
    specs = g.sklearn_cases()
    assert sorted(list(specs) + list(g.pymf_cases())) == sorted(
        os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "dictmu_*.npz")))
    for name in ("dictmu_sk_m50_r24_t150_k40", "dictmu_sk_m50_r24_t150_zeros"):
        out = g.make(name, specs[name])
        ref = np.load(os.path.join(GOLDEN, name + ".npz"))
        for k, v in out.items():
            assert np.array_equal(np.asarray(ref[k]), np.asarray(v)), (name, k)


def test_pymf_keyword_and_default():
    from exemplars_vc_amd.compat.pymf import NMF
    assert NMF(np.ones((3, 4)), num_bases=2)._dictionary_update == "host"
    assert NMF(np.ones((3, 4)), num_bases=2, dictionary_update="device")._dictionary_update == "device"
    with pytest.raises(ValueError):
        NMF(np.ones((3, 4)), num_bases=2, dictionary_update="gpu")


def test_learn_without_a_device_raises():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a HIP device is present")
    import exemplars_vc_amd as evc
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evc.learn_dictionary(np.ones((4, 5)), np.ones((4, 2)), np.ones((2, 5)), layout="bin_major", iters=1)
