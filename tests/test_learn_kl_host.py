"""Dictionary learning under the Kullback-Leibler loss (evc_nmf_learn, evc_learn_opts.loss), host side: the struct and
its ctypes mirror, the argument checks, the numpy restatement of the split update against scikit-learn's recorded
results (tests/golden/dictkl_sk_*.npz), and the fixture generator.  No GPU needed."""
import ctypes as C
import glob
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from learn_kl_restatement import learn  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "dictkl_sk_*.npz")))
RTOL = 1e-9         # the project's float64 bar (test_learn_host.py)


def lib():
    from exemplars_vc_amd import _lib
    return _lib, _lib.lib()


def test_loss_field_follows_reserved_in_header_and_mirror():
    _lib, L = lib()
    hdr = open(os.path.join(ROOT, "include", "evc.h")).read()
    body = hdr[hdr.index("typedef struct evc_learn_opts {"):hdr.index("} evc_learn_opts;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for grp in re.findall(r"\b(?:int|double|void\*)\s+([a-zA-Z_0-9, ]+);", body)
             for n in grp.replace(" ", "").split(",")]
    mirror = [f[0] for f in _lib.LearnOpts._fields_]
    assert names == mirror
    assert names[names.index("reserved") + 1] == "loss" and names[names.index("loss") + 1] == "tol"
    assert re.search(r"\bint\s+loss;", body)
    assert C.sizeof(_lib.LearnOpts) == 56
    assert _lib.LearnOpts.tol.offset == 32 and _lib.LearnOpts.loss.offset == 28
    assert _lib.LearnOpts().loss == _lib.LOSS_FROBENIUS == 0          # a zero-initialised struct asks for Frobenius
    assert L.evc_version() == 100
    head = hdr[:hdr.index("#ifndef EVC_H")]
    assert "EVC_LOSS_KL" in head[head.index("evc_nmf_learn"):]         # the header comment's list names the loss


def _opts(_lib, **kw):
    o = _lib.LearnOpts()
    o.struct_bytes = C.sizeof(_lib.LearnOpts)
    o.dtype, o.layout, o.surface, o.iters, o.check_every = _lib.F64, _lib.BIN_MAJOR, _lib.LEARN_SKLEARN, 5, 0
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_loss_is_validated_before_device_work():
    _lib, L = lib()
    one = C.c_void_p(8)              # never dereferenced: every case fails validation first

    def call(o, ws=1 << 40):
        return L.evc_nmf_learn(one, 40, one, 12, one, 40, 25, 12, 40, C.byref(o), one, ws, None, None, None)
    assert call(_opts(_lib, loss=2)) == -1
    assert call(_opts(_lib, loss=-1)) == -1
    assert call(_opts(_lib, loss=_lib.LOSS_KL, surface=_lib.LEARN_PYMF)) == -3
    assert call(_opts(_lib, loss=_lib.LOSS_KL), ws=16) == -2                  # it passed validation
    assert call(_opts(_lib, loss=_lib.LOSS_FROBENIUS), ws=16) == -2
    assert call(_opts(_lib, loss=_lib.LOSS_KL, reserved=1)) == -1             # the present rejections stay
    assert call(_opts(_lib, loss=_lib.LOSS_KL, surface=2)) == -1


def _check(got, want, what):
    nz = want != 0
    np.testing.assert_allclose(got[nz], want[nz], rtol=RTOL, atol=0, err_msg=what)
    assert not got[~nz].any(), what + ": a zero of the fixture is not zero"


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("path", [p for p in FILES if not p.endswith("_f32.npz")], ids=os.path.basename)
def test_restatement_reproduces_sklearn_kl_fixture(path, S):
    d = np.load(path)
    tol = float(d["tol"])
    W, H, n_iter, _ = learn(d["X"], d["W0"], d["H0"], int(d["max_iter"]), 10 if tol > 0 else 0, tol, S=S)
    assert n_iter == int(d["n_iter"])
    _check(W, d["W"], "W")
    _check(H, d["H"], "H")
    if path.endswith("_tol.npz"):
        assert 20 < n_iter < int(d["max_iter"])


def test_restatement_float32_is_close_to_sklearn_float32():
    paths = [p for p in FILES if p.endswith("_f32.npz")]
    assert paths
    for path in paths:
        d = np.load(path)
        assert d["W"].dtype == np.float32
        W, H, n_iter, _ = learn(d["X"], d["W0"], d["H0"], int(d["max_iter"]), 0, 0.0, S=3, dtype=np.float32)
        assert n_iter == int(d["n_iter"]) and W.dtype == np.float32
        for got, ref in ((W, d["W"]), (H, d["H"])):
            assert np.linalg.norm(got.astype(float) - ref) / np.linalg.norm(ref) <= 1e-4


def test_zeros_fixture_takes_the_unit_guard():
    """H0[5] = 0 with W0[:, 5] positive: s_5 = 0 divides by 1, Num[:, 5] = 0, so the column becomes exactly 0"""
    d = np.load(os.path.join(GOLDEN, "dictkl_sk_m50_r24_t150_zeros.npz"))
    assert (d["W0"][:, 5] > 0).all() and not d["H0"][5].any() and not d["X"][:, [3, 77]].any()
    Wr, Hr, _, _ = learn(d["X"], d["W0"], d["H0"], 40, 0, 0.0, S=3)
    for W, H in ((d["W"], d["H"]), (Wr, Hr)):
        assert np.isfinite(W).all() and np.isfinite(H).all()
        assert not W[:, 5].any() and not H[5].any() and not H[:, [3, 77]].any()


def test_fixture_names_and_sizes():
    want = ["m1026_r16_t40_k40", "m201_r20_t100_k40", "m25_r130_t70_k40", "m50_r24_t150_k40", "m50_r24_t150_k40_f32",
            "m50_r24_t150_tol", "m50_r24_t150_zeros"]
    assert [os.path.basename(p)[len("dictkl_sk_"):-4] for p in FILES] == want
    assert FILES == sorted(glob.glob(os.path.join(GOLDEN, "dictkl_*.npz")))
    for p in FILES:
        assert os.path.getsize(p) <= 1 << 20


def test_generator_reproduces_two_fixtures():
    pytest.importorskip("sklearn")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_golden_learn_kl as g
    specs = g.cases()
    assert sorted(specs) == sorted(os.path.basename(p)[:-4] for p in FILES)
    for name in ("dictkl_sk_m50_r24_t150_k40", "dictkl_sk_m50_r24_t150_zeros"):
        out = g.make(name, specs[name])
        ref = np.load(os.path.join(GOLDEN, name + ".npz"))
        for k, v in out.items():
            assert np.array_equal(np.asarray(ref[k]), np.asarray(v)), (name, k)


def test_restatement_error_never_rises():
    """the multiplicative updates do not increase the divergence (Lee & Seung); the GPU test relies on this trace"""
    d = np.load(os.path.join(GOLDEN, "dictkl_sk_m50_r24_t150_k40.npz"))
    _, _, _, err = learn(d["X"], d["W0"], d["H0"], 40, 1, 0.0, S=3)
    assert err.shape == (41,) and np.isfinite(err).all()
    assert np.diff(err).max() <= 1e-12 * err[0]
    assert err[-1] < err[0]


def test_python_surface_checks_the_loss():
    import inspect
    import exemplars_vc_amd as evc
    from exemplars_vc_amd.compat.factorize import non_negative_factorization_mu
    assert inspect.signature(evc.learn_dictionary).parameters["loss"].default == "frobenius"
    assert inspect.signature(evc.compact_dictionary).parameters["loss"].default == "frobenius"
    sig = inspect.signature(non_negative_factorization_mu)
    assert list(sig.parameters)[-1] == "beta_loss" and sig.parameters["beta_loss"].default == "frobenius"
    X, W, H = np.ones((4, 5)), np.ones((4, 2)), np.ones((2, 5))
    with pytest.raises(ValueError, match="pymf"):
        evc.learn_dictionary(X, W, H, layout="bin_major", iters=1, surface="pymf", loss="kl")
    with pytest.raises(ValueError, match="loss"):
        evc.learn_dictionary(X, W, H, layout="bin_major", iters=1, loss="itakura-saito")
    with pytest.raises(ValueError, match="beta_loss"):
        non_negative_factorization_mu(X.T, H.T, W.T, beta_loss="itakura-saito")


def test_learn_kl_without_a_device_raises():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a HIP device is present")
    import exemplars_vc_amd as evc
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evc.learn_dictionary(np.ones((4, 5)), np.ones((4, 2)), np.ones((2, 5)), layout="bin_major", iters=1, loss="kl")
