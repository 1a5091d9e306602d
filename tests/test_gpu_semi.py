"""evc_semi_solve on the GPU against recorded pymf results (tests/golden/snmf*.npz) and the numpy restatement
(tests/semi_restatement.py), which reproduces every one of them (tests/test_semi_host.py).

float64 bound, per frame column: ||h - h_ref||_2 <= 1e-8 ||h_ref||_2, the bound of the project's float64 parity tests; the
restatement with its sums in a permuted order stays within 3.4e-15 of pymf, far inside it.  The exact-zero pattern, n_iter and
len(ferr) are equal and ferr is held to 1e-8 relative.  Measured on an MI355X, worst column over this file: 2.0e-15 (the routed
size, N = 4096), over the fixtures 1.4e-15 (N = 130; the smaller ones agree to the last bit); worst ferr 1.8e-9, on
snmf_m1_n5_t3_k10, whose last errors (1.8e-8 on data of magnitude 1) are differences of nearly equal numbers.
float32 bound, measured in the test: the restatement run in float32 numpy arithmetic on the same case lies d32 (norm-relative)
from the float64 reference; the GPU is allowed 4 d32 - two float32 runs that sum in different orders can differ from each
other by twice what each differs from float64, the other factor of 2 is slack for the deeper N."""
import ctypes as C
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import semi_restatement as sr  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXED = ["snmf_m25_n64_t32_k50", "snmf_m40_n130_t33_k100", "snmf_m1_n5_t3_k10", "snmf_doctest", "snmf_zero_collapse"]
FULL = "snmfw_m25_r8_t70_k30"
RTOL = 1e-8
_cache = {}


def evc():
    import exemplars_vc_amd
    return exemplars_vc_amd


def problem(M, N, T, seed=0):
    key = (M, N, T, seed)
    if key not in _cache:
        _cache[key] = sr.problem(M, N, T, 1000 * seed + 7 * M + 3 * N + T)      # shared: the tests copy before they change one
    return _cache[key]


def reference(M, N, T, K, seed=0, **kw):
    key = ("ref", M, N, T, K, seed, tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = sr.solve(*problem(M, N, T, seed), K, **kw)
    return _cache[key]


def worst_column(H, ref):
    """max over the frame columns of ||h - h_ref|| / ||h_ref||; the exact zeros must coincide (bin-major N x T)"""
    H, ref = np.asarray(H, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert H.shape == ref.shape and np.array_equal(H == 0, ref == 0)
    num, den = np.linalg.norm(H - ref, axis=0), np.linalg.norm(ref, axis=0)
    assert not num[den == 0].any()
    return float(np.max(num[den > 0] / den[den > 0])) if (den > 0).any() else 0.0


def close64(H, ref, what=""):
    assert H.dtype == np.float64
    worst = worst_column(H, ref)
    print("%s worst column %.3e" % (what, worst))
    assert worst <= RTOL
    return worst


def nrel(a, b):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / np.linalg.norm(b))


def cabi(A, X, H0, iters, *, layout="bin_major", dtype=np.float64, pad=0, offs=None, check_every=0, stop_rule="none", tol=0.0,
         eps=1e-9, init="given", init_value=0.0):
    """evc_semi_solve through ctypes on bin-major numpy operands: every matrix is laid out as `layout` says inside a buffer
    whose leading dimension is `pad` longer than needed and whose padding holds NaN, which must still be there afterwards.
    -> H (N x T), n_iter, trace"""
    import torch
    from exemplars_vc_amd import _lib
    L = _lib.lib()
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    fm = layout == "frame_major"
    (M, N), T = A.shape, X.shape[1]

    def stage(mat):
        m = np.asarray(mat, dtype=dtype)
        m = m.T if fm else m
        buf = torch.full((m.shape[0], m.shape[1] + pad), float("nan"), dtype=tdt, device="cuda")
        buf[:, :m.shape[1]] = torch.from_numpy(np.ascontiguousarray(m))
        return buf, m.shape[1]
    (A_d, _), (X_d, _), (H_d, hcols) = stage(A), stage(X), stage(H0)
    o = _lib.SemiOpts()
    o.struct_bytes = C.sizeof(o)
    o.dtype, o.layout, o.iters = (_lib.F64 if dtype == np.float64 else _lib.F32), (_lib.FRAME_MAJOR if fm else _lib.BIN_MAJOR), iters
    o.init_mode = _lib.INIT_GIVEN if init == "given" else _lib.INIT_CONST
    o.check_every, o.stop_rule = check_every, {"none": _lib.STOP_NONE, "pymf": _lib.STOP_PYMF}[stop_rule]
    o.eps, o.tol, o.init_value = eps, tol, init_value
    n_utt = 1 if offs is None else len(offs) - 1
    po = None if offs is None else (C.c_int * len(offs))(*offs)
    slots = sr.n_slots(iters, check_every)
    n_iter, trace = np.zeros(n_utt, dtype=np.int32), np.full((n_utt, slots), -1.0)
    nbytes = int(L.evc_semi_workspace_bytes(M, N, T, n_utt, o.dtype))
    assert nbytes > 0
    ws = torch.empty(nbytes + 8, dtype=torch.uint8, device="cuda")
    ld = lambda t: int(t.stride(0))      # noqa: E731
    st = L.evc_semi_solve(A_d.data_ptr(), ld(A_d), X_d.data_ptr(), ld(X_d), H_d.data_ptr(), ld(H_d), M, N, T, po, n_utt,
                          C.byref(o), ws.data_ptr() + 8, nbytes, n_iter.ctypes.data_as(C.POINTER(C.c_int)),
                          trace.ctypes.data_as(C.POINTER(C.c_double)), None)
    assert st == 0, st
    torch.cuda.synchronize()
    out = H_d.cpu().numpy()
    if pad:
        assert np.isnan(out[:, hcols:]).all()                   # the padding of H was not overwritten
    out = out[:, :hcols]
    return (out.T if fm else out).copy(), n_iter, trace


# ---- the fixtures, through the C ABI and through compat.pymf.SNMF ----
@pytest.mark.parametrize("name", FIXED)
def test_fixture_through_the_c_abi(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    niter, T = int(d["niter"]), d["data"].shape[1]
    for layout in ("bin_major", "frame_major"):
        H, n_iter, tr = cabi(d["W"], d["data"], d["H0"], niter, layout=layout, pad=3, check_every=1, stop_rule="pymf",
                             tol=sr.PYMF_TOL)
        assert int(n_iter[0]) == int(d["n_iter"])
        ferr = sr.pymf_ferr(tr[0], int(n_iter[0]), niter, T)
        assert len(ferr) == len(d["ferr"]) and np.isnan(tr[0, 1 + int(n_iter[0]):]).all()
        close64(H, d["H"], name + " " + layout)
        print("ferr %.3e" % np.max(np.abs(ferr - d["ferr"]) / d["ferr"]))
        np.testing.assert_allclose(ferr, d["ferr"], rtol=1e-8, atol=0)


@pytest.mark.parametrize("name", FIXED)
def test_fixture_through_compat_snmf(name):
    from exemplars_vc_amd.compat import pymf
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    mdl = pymf.SNMF(d["data"].copy(), num_bases=d["W"].shape[1])
    mdl.W, mdl.H = d["W"].copy(), d["H0"].copy()
    held = mdl.H
    mdl.factorize(niter=int(d["niter"]), compute_w=False)
    assert mdl.H is held and len(mdl.ferr) == len(d["ferr"])       # in place, ferr cut as base.py:268 cuts it
    close64(mdl.H, d["H"], name)
    np.testing.assert_allclose(mdl.ferr, d["ferr"], rtol=1e-8, atol=0)
    assert mdl.frobenius_norm() == pytest.approx(float(d["frobenius_norm"]), rel=1e-8)
    assert mdl.residual() == pytest.approx(float(d["residual"]), rel=1e-8)


def test_the_default_call_with_compute_w():
    from exemplars_vc_amd.compat import pymf
    d = np.load(os.path.join(GOLDEN, FULL + ".npz"))
    np.random.seed(int(d["seed"]))
    mdl = pymf.SNMF(d["data"].copy(), num_bases=d["W"].shape[1])
    with pytest.warns(RuntimeWarning, match="outside the accelerated path"):
        mdl.factorize(niter=int(d["niter"]))
    assert len(mdl.ferr) == len(d["ferr"])
    close64(mdl.H, d["H"], FULL + " H")
    close64(mdl.W.T, d["W"].T, FULL + " W")                       # W by its rows: the columns of W^T
    np.testing.assert_allclose(mdl.ferr, d["ferr"], rtol=1e-8, atol=0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m2 = pymf.SNMF(d["data"].copy(), num_bases=d["W"].shape[1])
        m2.H = d["H0"].copy()
        m2.factorize(niter=2, compute_err=False)                   # no ferr asked for, none made
    assert not hasattr(m2, "ferr") and m2.W.shape == d["W"].shape


# ---- iteration counts: both parities of the buffer swap end in the caller's H ----
@pytest.mark.parametrize("layout", ["bin_major", "frame_major"])
def test_iteration_counts(layout):
    A, X, H0 = problem(25, 33, 70)
    for iters in (0, 1, 2, 3):
        H, n_iter, tr = cabi(A, X, H0, iters, layout=layout, pad=5, check_every=1)
        ref, _, rtr = reference(25, 33, 70, iters, check_every=1)
        assert n_iter.tolist() == [iters] and tr.shape == (1, iters + 1)
        if iters == 0:
            assert np.array_equal(H, H0)                            # the start stays in place
        close64(H, ref, "iters %d" % iters)
        np.testing.assert_allclose(tr, rtr, rtol=1e-8, atol=0)
    Hc, _, _ = cabi(A, X, np.full_like(H0, np.nan), 3, layout=layout, pad=5, init="const", init_value=0.25)
    close64(Hc, sr.solve(A, X, np.full_like(H0, 0.25), 3)[0], "const start")
    Hc0, _, _ = cabi(A, X, np.full_like(H0, np.nan), 0, layout=layout, pad=5, init="const", init_value=0.25)
    assert np.array_equal(Hc0, np.full_like(H0, 0.25))


# ---- geometry: exemplars around the k-slab (16) and the row block (128), frames around 16 and the frame block (64) ----
NS, TS, MS = (1, 5, 16, 17, 127, 129, 257), (1, 15, 17, 63, 65, 130), (1, 3, 25, 40)


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("T", TS)
def test_geometry(N, T):
    M = MS[(NS.index(N) + TS.index(T)) % 4]
    A, X, H0 = problem(M, N, T)
    ref, _, rtr = reference(M, N, T, 3, check_every=3)
    for layout in ("bin_major", "frame_major"):
        H, n_iter, tr = cabi(A, X, H0, 3, layout=layout, pad=7, check_every=3)
        assert n_iter.tolist() == [3]
        close64(H, ref, "M %d N %d T %d %s" % (M, N, T, layout))
        np.testing.assert_allclose(tr, rtr, rtol=1e-8, atol=0)


def test_every_bin_count_meets_both_layouts():
    for M in MS:
        A, X, H0 = problem(M, 129, 65, seed=1)
        ref = reference(M, 129, 65, 3, seed=1)[0]
        for layout in ("bin_major", "frame_major"):
            close64(cabi(A, X, H0, 3, layout=layout, pad=1)[0], ref, "M %d %s" % (M, layout))


# ---- a batch is its utterances; the same call twice is the same bits ----
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_batch_equals_per_utterance(dtype):
    offs = [0, 37, 37, 40, 90]
    A, X, H0 = problem(25, 129, 90)
    kw = dict(dtype=dtype, check_every=2, stop_rule="pymf", tol=sr.PYMF_TOL, layout="frame_major", pad=2)
    H, n_iter, tr = cabi(A, X, H0, 6, offs=offs, **kw)
    H2, n_iter2, tr2 = cabi(A, X, H0, 6, offs=offs, **kw)
    assert np.array_equal(H, H2) and np.array_equal(n_iter, n_iter2) and np.array_equal(tr, tr2, equal_nan=True)
    assert n_iter.tolist() == [6] * 4 and np.isnan(tr[1]).all() and np.isfinite(tr[[0, 2, 3]]).all()
    for u in (0, 2, 3):
        Hu, nu, tu = cabi(A, X[:, offs[u]:offs[u + 1]], H0[:, offs[u]:offs[u + 1]], 6, **kw)
        assert np.array_equal(H[:, offs[u]:offs[u + 1]], Hu) and nu[0] == n_iter[u] and np.array_equal(tr[u], tu[0])
    if dtype == np.float64:
        ref, _, rtr = sr.solve(A, X, H0, 6, check_every=2, utt_offsets=offs)
        close64(H, ref, "batch")
        np.testing.assert_allclose(tr[[0, 2, 3]], rtr[[0, 2, 3]], rtol=1e-8, atol=0)


# ---- the two workgroup widths, 8 and 4 wavefronts, chosen from the sizes alone (semi_waves), give the same bits ----
def test_every_workgroup_width_gives_the_same_bits():
    offs = [0, 5440, 10881]                     # N = 257: the batch runs 8 wavefronts (171 x 3 workgroups), its utterances alone 4
    A, X, H0 = problem(3, 257, 10881)
    H, n_iter, tr = cabi(A, X, H0, 3, offs=offs, check_every=3, layout="frame_major")
    ref, _, rtr = reference(3, 257, 10881, 3, check_every=3, utt_offsets=tuple(offs))
    close64(H, ref, "8 wavefronts")
    np.testing.assert_allclose(tr, rtr, rtol=1e-8, atol=0)
    for u in (0, 1):
        Hu, _, tu = cabi(A, X[:, offs[u]:offs[u + 1]], H0[:, offs[u]:offs[u + 1]], 3, check_every=3, layout="frame_major")
        assert np.array_equal(H[:, offs[u]:offs[u + 1]], Hu) and np.array_equal(tr[u], tu[0])
    # one frame below the threshold the whole batch runs 4 wavefronts: the shared frames keep their bits
    Hb, _, _ = cabi(A, X[:, :10880], H0[:, :10880], 3, layout="frame_major")
    assert np.array_equal(Hb[:, :5440], H[:, :5440])


# ---- the stop: the zero-collapse utterance stops with a difference of exactly 0 and stays frozen ----
def test_stop_rule_freezes_one_utterance():
    M, N, T2, K = 25, 33, 50, 8
    A, X2, H02 = (a.copy() for a in problem(M, N, T2))
    A[:, 0], A[:, 1] = 0.0, 0.0
    A[0, 0], A[0, 1] = 1.0, -1.0                                    # the zero-collapse dictionary in the first two exemplars
    x1, h1 = np.zeros((M, 1)), np.zeros((N, 1))
    x1[0, 0], h1[0, 0] = -1.0, 1.0                                  # its frame and its start, the rows padded to the common N
    X, H0, offs = np.hstack([x1, X2]), np.hstack([h1, H02]), [0, 1, 1 + T2]
    kw = dict(check_every=1, stop_rule="pymf", tol=sr.PYMF_TOL)
    H, n_iter, tr = cabi(A, X, H0, K, offs=offs, **kw)
    ref, rn, rtr = sr.solve(A, X, H0, K, utt_offsets=offs, **kw)
    # pymf stops at update index i = 2, the third update, and cuts ferr to 2 entries
    assert n_iter.tolist() == rn.tolist() == [3, K] and len(sr.pymf_ferr(tr[0], 3, K, 1)) == 2
    assert not H[:, 0].any() and tr[0, :4].tolist() == [2.0, 1.0, 1.0, 1.0] and np.isnan(tr[0, 4:]).all()
    close64(H, ref, "stop batch")
    Ha, na, ta = cabi(A, X[:, 1:], H0[:, 1:], K, **kw)
    assert np.array_equal(H[:, 1:], Ha) and na[0] == n_iter[1] and np.array_equal(tr[1], ta[0])
    # frozen: with a start that is already at a fixed point of the stop (H = 0), later updates leave the column as it is
    H0b = H0.copy()
    H0b[:, 0] = 0.0
    H0b[3, 0] = 0.5                                                 # exemplar 3 is not matched by x1: it would keep moving
    Hb, nb, _ = cabi(A, X, H0b, K, offs=offs, check_every=1, stop_rule="pymf", tol=1e300)
    rb, rnb, _ = sr.solve(A, X, H0b, K, utt_offsets=offs, check_every=1, stop_rule="pymf", tol=1e300)
    assert nb.tolist() == rnb.tolist() == [3, 3]
    close64(Hb, rb, "frozen after 3 of %d" % K)


# ---- containment ----
def test_nan_in_a_frame_stays_in_its_column():
    A, X, H0 = problem(25, 129, 65)
    H, _, _ = cabi(A, X, H0, 3)
    Xn = X.copy()
    Xn[7, 20] = np.nan
    Hn, _, _ = cabi(A, Xn, H0, 3)
    keep = np.arange(65) != 20
    assert np.isnan(Hn[:, 20]).all() and np.array_equal(Hn[:, keep], H[:, keep])


def test_nan_in_the_dictionary_reaches_every_activation():
    A, X, H0 = (a.copy() for a in problem(25, 129, 65))
    A[3, 40] = np.nan
    H, n_iter, tr = cabi(A, X, H0, 2, check_every=1, stop_rule="pymf", tol=sr.PYMF_TOL)
    assert np.isnan(H).all() and n_iter.tolist() == [2] and np.isnan(tr).all()


# ---- the Python surface ----
def test_convert_semi():
    import torch
    rng = np.random.default_rng(5)
    A, X, H0 = problem(25, 64, 40)
    B = rng.random((201, 64))
    Y, H, info = evc().convert_semi(A, B, X, H0, iters=10, check_every=5, info=True)
    ref, _, rtr = reference(25, 64, 40, 10, check_every=5)
    close64(H, ref, "convert_semi")
    assert info["kernel"] == "k_semi_sweep" and info["n_iter"].tolist() == [10] and info["launches"] == 10 + 3 * 3
    np.testing.assert_allclose(info["err"], rtr, rtol=1e-8, atol=0)
    assert Y.shape == (201, 40) and (Y >= 0).all()
    np.testing.assert_allclose(Y, B @ H, rtol=1e-12, atol=1e-12 * np.abs(B @ H).max())
    # frame-major device tensors in, device tensors out; a signed target side
    Bs = rng.standard_normal((64, 30))
    Yt, Ht = evc().convert_semi(torch.from_numpy(A.T.copy()).cuda(), torch.from_numpy(Bs).cuda(), torch.from_numpy(X.T.copy()).cuda(),
                                torch.from_numpy(H0.T.copy()).cuda(), layout="frame_major", iters=10)
    assert isinstance(Yt, torch.Tensor) and Yt.is_cuda and tuple(Yt.shape) == (40, 30)
    close64(Ht.cpu().numpy().T, ref, "convert_semi frame_major")
    np.testing.assert_allclose(Yt.cpu().numpy(), Ht.cpu().numpy() @ Bs, rtol=1e-12, atol=1e-12 * np.abs(Ht.cpu().numpy() @ Bs).max())


# ---- the routed size of the flagship: N = 4096, one utterance of 688 frames ----
def test_routed_size():
    A, X, H0 = problem(25, 4096, 688)
    ref, _, rtr = reference(25, 4096, 688, 5, check_every=5)
    H, info = evc().solve_activations_semi(A, X, H0, iters=5, check_every=5, info=True)
    close64(H, ref, "N 4096 T 688")
    np.testing.assert_allclose(info["err"], rtr, rtol=1e-8, atol=0)


# ---- float32 ----
@pytest.mark.parametrize("case", ["snmf_m25_n64_t32_k50", (25, 17, 63), (3, 129, 65), (40, 257, 130), (1, 127, 15)])
def test_float32(case):
    if isinstance(case, str):
        d = np.load(os.path.join(GOLDEN, case + ".npz"))
        A, X, H0, K, ref = d["W"], d["data"], d["H0"], int(d["niter"]), d["H"]
    else:
        (A, X, H0), K = problem(*case), 3
        ref = reference(*case, K)[0]
    r32 = sr.solve(A, X, H0, K, dtype=np.float32)[0]
    assert r32.dtype == np.float32
    d32 = nrel(r32, ref)
    for layout in ("bin_major", "frame_major"):
        H, n_iter, _ = cabi(A, X, H0, K, dtype=np.float32, layout=layout, pad=3)
        got = nrel(H, ref)
        print("%s %s: float32 numpy %.3e, GPU %.3e (allowed %.3e)" % (case, layout, d32, got, 4 * d32))
        assert H.dtype == np.float32 and n_iter.tolist() == [K] and got <= 4 * d32
