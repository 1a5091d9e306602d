"""The three dictionary-learning entries (evc_nmf_learn, evc_cd_learn, evc_beta_learn) give bit for bit what they gave
before their host drivers came to share one skeleton: sha256 of W, H, n_iter and the error / violation
trace of the calls below, recorded on the commit before that change by tools/make_learn_digests.py, which runs CASES
as they stand here.  Every call reads a fixture of tests/golden; together they take the paths the shared code has: both
layouts, both stop rules and their early stops, no checks at all, forced frame ranges, float32 (frames padded to 64),
both routes of the beta dictionary half, coordinate descent's own loop in both update modes, and a workspace that does
not start at a multiple of 256 bytes.

evc_nmf_learn has no case with such a workspace: it carves from the pointer it is given (the caller aligns it), so the
kernels' 16-byte accesses would be misaligned - not a supported call before or after."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")

PYMF_TOL = 2.58e-3      # |err - err_prev| / T first falls below it at the 7th of the fixture's 40 iterations


def fixture(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def digest(W, H, info, trace):
    h = hashlib.sha256()
    for a in (W, H, info[trace]):
        h.update(np.ascontiguousarray(a).tobytes())
    h.update(str(int(info["n_iter"])).encode())
    return h.hexdigest()


def nmf(name, layout="bin_major", x="X", **kw):
    import exemplars_vc_amd as evc
    d = fixture(name)
    t = (lambda a: a) if layout == "bin_major" else (lambda a: np.ascontiguousarray(a.T))
    W, H, info = evc.learn_dictionary(t(d[x]), t(d["W0"]), t(d["H0"]), layout=layout, info=True, **kw)
    return digest(W, H, info, "err"), info


def sk_tol(layout):
    d = fixture("dictmu_sk_m50_r24_t150_tol")
    dg, info = nmf("dictmu_sk_m50_r24_t150_tol", layout, iters=int(d["max_iter"]), check_every=10, tol=float(d["tol"]))
    assert info["n_iter"] == int(d["n_iter"]) < int(d["max_iter"])
    return dg


def pymf_tol():
    dg, info = nmf("dictmu_pymf_m50_r24_t150_k40_err", x="data", iters=40, surface="pymf", check_every=1, tol=PYMF_TOL)
    assert 3 <= info["n_iter"] < 40
    return dg


def beta(name, **kw):
    import exemplars_vc_amd as evc
    d = fixture(name)
    W, H, info = evc.learn_dictionary_beta(d["X"], d["W0"], d["H0"], beta=float(d["beta"]), layout="bin_major",
                                           iters=int(d["max_iter"]), check_every=10, tol=float(d["tol"]), info=True, **kw)
    return digest(W, H, info, "err")


def cd(name, **kw):
    import exemplars_vc_amd as evc
    d = fixture(name)
    kw.setdefault("max_iter", int(d["max_iter"]))
    W, H, info = evc.learn_dictionary_cd(d["X_rows"], d["W0_rows"], d["H0_rows"], layout="frame_major", tol=float(d["tol"]),
                                         info=True, **kw)
    if name.endswith("_early"):
        assert info["n_iter"] < kw["max_iter"]
    return digest(W, H, info, "violation")


def raw_shifted(entry):
    """one call through the C ABI, float64, the workspace 8 bytes past a multiple of 256"""
    import torch
    from exemplars_vc_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    if entry == "evc_cd_learn":
        d = fixture("cdlearn_m25_r17_t70")
        X, W, H = (torch.from_numpy(d[k]).to(dev) for k in ("X_rows", "W0_rows", "H0_rows"))
        (T, M), R = X.shape, W.shape[0]
        o = _lib.CdLearnOpts()
        o.struct_bytes, o.layout, o.max_iter, o.tol = C.sizeof(o), _lib.FRAME_MAJOR, 12, 1e-4
        trace = np.zeros((12, 2))
        nbytes = int(L.evc_cd_learn_workspace_bytes(M, R, T, _lib.F64))
    else:
        d = fixture("dictbeta_sk_m25_r17_t70_k30_flush_b0")
        X, W, H = (torch.from_numpy(d[k]).to(dev) for k in ("X", "W0", "H0"))
        (M, T), R = X.shape, W.shape[1]
        o = _lib.BetaLearnOpts()
        o.struct_bytes, o.layout, o.iters, o.check_every, o.beta = C.sizeof(o), _lib.BIN_MAJOR, 12, 4, 0.0
        trace = np.zeros(4)
        nbytes = int(L.evc_beta_learn_workspace_bytes(M, R, T, _lib.F64))
    assert nbytes > 0
    buf = torch.empty(nbytes + 512, dtype=torch.uint8, device=dev)
    ws = (buf.data_ptr() + 255) // 256 * 256 + 8
    n_iter = C.c_int(0)
    with torch.cuda.device(dev):
        st = getattr(L, entry)(X.data_ptr(), X.stride(0), W.data_ptr(), W.stride(0), H.data_ptr(), H.stride(0), M, R, T,
                               C.byref(o), ws, nbytes, C.byref(n_iter), trace.ctypes.data_as(C.POINTER(C.c_double)),
                               C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    _lib.check(st, entry)
    torch.cuda.synchronize()
    return digest(W.cpu().numpy(), H.cpu().numpy(), {"n_iter": n_iter.value, "t": trace}, "t")


CASES = {
    "nmf_sk_tol_bin_major": lambda: sk_tol("bin_major"),
    "nmf_sk_tol_frame_major": lambda: sk_tol("frame_major"),
    "nmf_pymf_tol": pymf_tol,
    "nmf_kl_f32": lambda: nmf("dictkl_sk_m50_r24_t150_k40_f32", iters=40, check_every=10, loss="kl")[0],
    "nmf_sk_no_checks": lambda: nmf("dictmu_sk_m50_r24_t150_k40", iters=40, check_every=0)[0],
    "nmf_sk_splits3": lambda: nmf("dictmu_sk_m50_r24_t150_k40", iters=40, check_every=10, splits=3)[0],
    "beta_b0_fused": lambda: beta("dictbeta_sk_m25_r17_t70_k30_flush_b0", route="fused"),
    "beta_b0_unfused": lambda: beta("dictbeta_sk_m25_r17_t70_k30_flush_b0", route="unfused"),
    "beta_b1p5_tol": lambda: beta("dictbeta_sk_m50_r24_t150_tol_b1p5"),
    "cd_early": lambda: cd("cdlearn_m25_r17_t70_early"),
    "cd_f32": lambda: cd("cdlearn_m25_r17_t70_f32"),
    "cd_dict_only_splits2": lambda: cd("cdlearn_m25_r17_t70", update="dict", splits=2),
    "cd_raw_workspace_plus_8": lambda: raw_shifted("evc_cd_learn"),
    "beta_raw_workspace_plus_8": lambda: raw_shifted("evc_beta_learn"),
}

# printed by tools/make_learn_digests.py on the commit before the drivers shared their skeleton
PARENT_DIGESTS = {
    "beta_b0_fused": "a28af613ea88586a21b5735af824886942c885bdad23c0805ac80a30d18f719d",
    "beta_b0_unfused": "9c21b362fad94f8ae80b9e3a411c31b96922fce0672b514ae8b0e857b82270dd",
    "beta_b1p5_tol": "c2885770cc8d4cbf1e0899a2553b890f7a858844ece4c3db43e8cdb5bb22936a",
    "beta_raw_workspace_plus_8": "de06b2629c643503ad9dd74024f434521de160067345716611a3a4ac0b4ac6d0",
    "cd_dict_only_splits2": "c1a5db94d20332c917c3560ca9b76bb60741c88e561355d1c8ba0927eafe90a2",
    "cd_early": "7a02e9a4e5835d921e5ab9f2d9177377b1fc7312bd88b696fcbf6c00c29bf780",
    "cd_f32": "b92d3b69bccb34167827be63b6204af5eb3001c9a7d3ef5a179a048fdcc9b757",
    "cd_raw_workspace_plus_8": "ac488e321b826f8469b2554d0f7365a98509aa1f71efdcdebb10ba6481912fc9",
    "nmf_kl_f32": "c828baa16b8f46fd0b89e4e81aa1c45dbb4f0620ed2eb20e701cc9f8250f335a",
    "nmf_pymf_tol": "d1e633e217055cd77cc5b076f57344ba2d0ca53a067f9fd17e50302d3f889dc5",
    "nmf_sk_no_checks": "cf0c3410b49b96f4c641206b9a0b17ed80d3909157996aefa292f194b948ebe8",
    "nmf_sk_splits3": "a00a0dd7d426d6107b79b0190ff648462bd7353e0ddf9d8888bf3e9daa4de6f1",
    "nmf_sk_tol_bin_major": "5ab86a24f58ade828d1a4b6375a77f7c16c6c0f5e9ef285c9ad78d25cefff551",
    "nmf_sk_tol_frame_major": "5d992b1aa3a11aa963e0a45fbd599c8a01f080c2e18e46b0ee325745cd7b9118",
}


def test_every_case_is_pinned():
    assert sorted(PARENT_DIGESTS) == sorted(CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_bitwise_what_the_parent_gave(case):
    got = CASES[case]()
    print(case, got)
    assert got == PARENT_DIGESTS[case]
