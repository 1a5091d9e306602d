"""evc_convex_learn on the GPU against recorded pymf results (tests/golden/cnmf*.npz) and the numpy restatement
(tests/convex_restatement.py), which reproduces every one of them (tests/test_convex_host.py).

float64 bound, per column of G and per frame column of H: ||v - v_ref||_2 <= 1e-8 ||v_ref||_2, the bound of the project's
float64 parity tests; the restatement stays within 1.8e-15 of pymf, far inside it.  The exact-zero patterns and n_iter are
equal and ferr is held to 1e-8 relative.  A forced split of k into S ranges only reorders sums of non-negative terms of at
most 300 addends: 1e-12 norm-relative is some 30 times the worst case of such a reordering in float64 (300 x 1.1e-16).
float32 bound, measured in the test: the restatement run in float32 numpy arithmetic on the same case lies d32
(norm-relative) from the float64 reference; the GPU is allowed 4 d32 - two float32 runs that sum in different orders can
differ from each other by twice what each differs from float64, the other factor of 2 is slack.
Measured on an MI355X, worst column over this file: 4.8e-15 (cnmf_m25_t300_r33, 100 iterations), 1.9e-15 at the routed size;
worst ferr 4.4e-16 relative; forced splits within 2.5e-16 of S = 1; float32 7.3e-8 ... 1.7e-6 where numpy's float32 run lies
7.3e-8 ... 1.7e-6."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convex_restatement as cr  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GIVEN = ["cnmf_m25_t70_r8", "cnmf_m40_t257_r17", "cnmf_m3_t5_r2", "cnmf_m25_t300_r33", "cnmf_zeros", "cnmf_honly", "cnmf_gonly"]
DEFAULT = ["cnmfd_doctest", "cnmfd_m25_t70_r8", "cnmfd_m40_t257_r17"]
SHAPES = ["cnmf_m25_t70_r8", "cnmf_m40_t257_r17", "cnmf_m3_t5_r2", "cnmf_m25_t300_r33"]
GEOMETRY = [(1, 1), (5, 2), (16, 16), (17, 15), (63, 17), (64, 64), (65, 65), (129, 63), (130, 33), (257, 130), (300, 1)]
RTOL = 1e-8
_cache = {}


def evc():
    import exemplars_vc_amd
    return exemplars_vc_amd


def problem(M, T, R):
    key = (M, T, R)
    if key not in _cache:
        X, assign = cr.problem(M, T, R, 7 * M + 3 * T + R)
        _cache[key] = (X,) + cr.cluster_start(assign, R)          # shared: the tests copy before they change one
    return _cache[key]


def reference(M, T, R, K, **kw):
    key = ("ref", M, T, R, K, tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = cr.learn(*problem(M, T, R), K, **kw)
    return _cache[key]


def fixture_update(d):
    return "both" if bool(d["compute_w"]) and bool(d["compute_h"]) else ("h" if bool(d["compute_h"]) else "g")


def worst_column(A, ref):
    """max over the columns of ||a - a_ref|| / ||a_ref||; the exact zeros must coincide"""
    A, ref = np.asarray(A, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert A.shape == ref.shape and np.array_equal(A == 0, ref == 0)
    num, den = np.linalg.norm(A - ref, axis=0), np.linalg.norm(ref, axis=0)
    assert not num[den == 0].any()
    return float(np.max(num[den > 0] / den[den > 0])) if (den > 0).any() else 0.0


def close64(G, H, Gref, Href, what=""):
    assert G.dtype == np.float64 and H.dtype == np.float64
    wg, wh = worst_column(G, Gref), worst_column(H, Href)
    print("%s worst column G %.3e H %.3e" % (what, wg, wh))
    assert wg <= RTOL and wh <= RTOL


def nrel(a, b):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / np.linalg.norm(b))


def cabi(X, G0, H0, iters, *, layout="bin_major", dtype=np.float64, pad=0, update="both", check_every=0, tol=0.0, eps=1e-9,
         splits=0, waves=0, want_w=True):
    """evc_convex_learn through ctypes on bin-major numpy operands: X, H and W are laid out as `layout` says, G is always
    T x R; every buffer's leading dimension is `pad` longer than needed and its padding holds NaN, which must still be there
    afterwards.  -> G (T x R), H (R x T), W (M x R, or None), n_iter, trace"""
    import torch
    from exemplars_vc_amd import _lib
    L = _lib.lib()
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    fm = layout == "frame_major"
    (M, T), R = X.shape, G0.shape[1]

    def stage(mat, transpose):
        m = np.asarray(mat, dtype=dtype)
        m = m.T if transpose else m
        buf = torch.full((m.shape[0], m.shape[1] + pad), float("nan"), dtype=tdt, device="cuda")
        buf[:, :m.shape[1]] = torch.from_numpy(np.ascontiguousarray(m))
        return buf, m.shape[1]
    (X_d, _), (G_d, gcols), (H_d, hcols) = stage(X, fm), stage(G0, False), stage(H0, fm)
    wshape = (R, M) if fm else (M, R)
    W_d = torch.full((wshape[0], wshape[1] + pad), float("nan"), dtype=tdt, device="cuda")
    o = _lib.ConvexOpts()
    o.struct_bytes = C.sizeof(o)
    o.dtype, o.layout, o.iters = (_lib.F64 if dtype == np.float64 else _lib.F32), (_lib.FRAME_MAJOR if fm else _lib.BIN_MAJOR), iters
    o.check_every, o.update = check_every, {"both": _lib.CONVEX_BOTH, "h": _lib.CONVEX_H_ONLY, "g": _lib.CONVEX_G_ONLY}[update]
    o.tol, o.eps, o.reserved = tol, eps, (waves << 16) | (splits << 8)
    slots = cr.n_slots(iters, check_every)
    n_iter, trace = C.c_int(-1), np.full(slots, -1.0)
    nbytes = int(L.evc_convex_workspace_bytes(M, R, T, o.dtype))
    assert nbytes > 0
    if splits > 1:
        nbytes += 2 * splits * T * R * (8 if dtype == np.float64 else 4) + 256
    ws = torch.empty(nbytes + 8, dtype=torch.uint8, device="cuda")
    ld = lambda t: int(t.stride(0))      # noqa: E731
    st = L.evc_convex_learn(X_d.data_ptr(), ld(X_d), G_d.data_ptr(), ld(G_d), H_d.data_ptr(), ld(H_d),
                            W_d.data_ptr() if want_w else None, ld(W_d) if want_w else 0, M, R, T, C.byref(o), ws.data_ptr() + 8,
                            nbytes, C.byref(n_iter), trace.ctypes.data_as(C.POINTER(C.c_double)), None)
    assert st == 0, st
    torch.cuda.synchronize()
    G, H, W = G_d.cpu().numpy(), H_d.cpu().numpy(), W_d.cpu().numpy()
    if pad:
        assert np.isnan(G[:, gcols:]).all() and np.isnan(H[:, hcols:]).all() and np.isnan(W[:, wshape[1]:]).all()
    G, H, W = G[:, :gcols].copy(), H[:, :hcols], W[:, :wshape[1]]
    if not want_w:
        assert np.isnan(W).all()                                # never touched
    return G, (H.T if fm else H).copy(), ((W.T if fm else W).copy() if want_w else None), int(n_iter.value), trace


# ---- the fixtures, through the C ABI and through compat.pymf.CNMF ----
@pytest.mark.parametrize("name", GIVEN + DEFAULT)
def test_fixture_through_the_c_abi(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    niter, T = int(d["niter"]), d["data"].shape[1]
    for layout in ("bin_major", "frame_major"):
        G, H, W, n_iter, tr = cabi(d["data"], d["G0"], d["H0"], niter, layout=layout, pad=3, update=fixture_update(d),
                                   check_every=1, tol=cr.PYMF_TOL)
        assert n_iter == int(d["n_iter"])
        ferr = cr.pymf_ferr(tr, n_iter, niter, T)
        assert len(ferr) == len(d["ferr"]) and np.isnan(tr[1 + n_iter:]).all()
        close64(G, H, d["G"], d["H"], name + " " + layout)
        print("W %.3e ferr %.3e" % (worst_column(W, d["W"]), np.max(np.abs(ferr - d["ferr"]) / d["ferr"])))
        assert worst_column(W, d["W"]) <= RTOL
        np.testing.assert_allclose(ferr, d["ferr"], rtol=1e-8, atol=0)
    if name == "cnmf_zeros":
        assert np.array_equal(G == 0, d["G0"] == 0) and (G == 0).sum() == 70 * 7


@pytest.mark.parametrize("name", GIVEN + DEFAULT)
def test_fixture_through_compat_cnmf(name):
    from exemplars_vc_amd.compat import pymf
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    R = d["G0"].shape[1]
    mdl = pymf.CNMF(d["data"].copy(), num_bases=R)
    if name in DEFAULT:                                     # the default call: the mirror's own k-means start
        state = random.getstate()
        random.seed(int(d["seed"]))
        try:
            mdl.factorize(niter=int(d["niter"]))
        finally:
            random.setstate(state)
    else:
        mdl.G, mdl.H = d["G0"].copy(), d["H0"].copy()
        mdl.W = np.dot(d["data"], mdl.G)
        mdl.factorize(niter=int(d["niter"]), compute_w=bool(d["compute_w"]), compute_h=bool(d["compute_h"]))
    close64(mdl.G, mdl.H, d["G"], d["H"], name)
    assert worst_column(mdl.W, d["W"]) <= RTOL
    assert len(mdl.ferr) == len(d["ferr"])
    np.testing.assert_allclose(mdl.ferr, d["ferr"], rtol=1e-8, atol=0)
    assert mdl.frobenius_norm() == pytest.approx(float(d["ferr"][-1]), rel=1e-8)


# ---- every geometry of the sweep against the restatement ----
@pytest.mark.parametrize("T,R", GEOMETRY)
def test_geometry_against_the_restatement(T, R):
    for M in (1, 25):
        X, G0, H0 = problem(M, T, R)
        Gref, Href, _, _ = reference(M, T, R, 3, check_every=0)
        for layout in ("bin_major", "frame_major"):
            G, H, W, n_iter, _ = cabi(X, G0, H0, 3, layout=layout, pad=5)
            assert n_iter == 3
            close64(G, H, Gref, Href, "M=%d T=%d R=%d %s" % (M, T, R, layout))
            assert nrel(W, X @ Gref) <= RTOL


@pytest.mark.parametrize("T,R", [(257, 33), (130, 130)])
def test_forced_splits_and_block_widths(T, R):
    X, G0, H0 = problem(25, T, R)
    base = {}
    for waves in (8, 4, 2):
        G, H, W, _, tr = cabi(X, G0, H0, 3, splits=1, waves=waves, check_every=1)
        base[waves] = (G, H, W, tr)
    for waves in (4, 2):                                     # with S = 1 an output's bits do not depend on the width
        assert all(np.array_equal(a, b) for a, b in zip(base[8], base[waves]))
    Gref, Href, _, _ = reference(25, T, R, 3, check_every=0)
    close64(base[8][0], base[8][1], Gref, Href, "S=1")
    for splits in (1, 2, 3, 7):
        for waves in (8, 4, 2):
            G, H, W, _, tr = cabi(X, G0, H0, 3, splits=splits, waves=waves, check_every=1, pad=2)
            dg, dh = nrel(G, base[8][0]), nrel(H, base[8][1])
            print("S=%d W=%d G %.3e H %.3e" % (splits, waves, dg, dh))
            assert dg <= 1e-12 and dh <= 1e-12 and nrel(tr, base[8][3]) <= 1e-12
            again = cabi(X, G0, H0, 3, splits=splits, waves=waves, check_every=1, pad=2)
            assert np.array_equal(G, again[0]) and np.array_equal(H, again[1]) and np.array_equal(W, again[2])
            assert np.array_equal(tr, again[4])
    # the plan's own choice is one of those
    G, H, _, _, _ = cabi(X, G0, H0, 3)
    assert nrel(G, base[8][0]) <= 1e-12 and nrel(H, base[8][1]) <= 1e-12


def test_update_modes():
    X, G0, H0 = problem(25, 130, 33)
    for update in ("both", "h", "g"):
        Gref, Href, _, trref = reference(25, 130, 33, 4, update=update, check_every=2)
        for layout in ("bin_major", "frame_major"):
            G, H, W, n_iter, tr = cabi(X, G0, H0, 4, layout=layout, pad=1, update=update, check_every=2)
            close64(G, H, Gref, Href, update + " " + layout)
            assert n_iter == 4 and tr.shape == (3,)
            np.testing.assert_allclose(tr, trref, rtol=1e-8, atol=0)
            if update == "h":
                assert np.array_equal(G, G0)
            if update == "g":
                assert np.array_equal(H, H0)


def test_the_stop_sits_between_two_recorded_steps():
    d = np.load(os.path.join(GOLDEN, "cnmf_m25_t70_r8.npz"))
    T = d["data"].shape[1]
    stat = np.abs(np.diff(d["ferr"])) / T                   # stat[i]: what the test at update i + 2 compares with tol
    tol = float(np.sqrt(stat[16] * stat[17]))
    print("statistic %.3e then %.3e, tol %.3e" % (stat[16], stat[17], tol))
    assert stat[17] < 0.97 * tol and tol < 0.97 * stat[16]  # the decision sits some percent from either side
    Gref, Href, nref, trref = cr.learn(d["data"], d["G0"], d["H0"], 30, check_every=1, tol=tol)
    assert nref == 19
    for layout in ("bin_major", "frame_major"):
        G, H, _, n_iter, tr = cabi(d["data"], d["G0"], d["H0"], 30, layout=layout, check_every=1, tol=tol)
        assert n_iter == nref and np.array_equal(np.isnan(tr), np.isnan(trref))
        np.testing.assert_allclose(tr[:1 + nref], trref[:1 + nref], rtol=1e-8, atol=0)
        close64(G, H, Gref, Href, "stopped " + layout)
    # checks every second iteration: the third check is the first that may stop
    Gref, Href, nref, trref = cr.learn(d["data"], d["G0"], d["H0"], 30, check_every=2, tol=1.0)
    G, H, _, n_iter, tr = cabi(d["data"], d["G0"], d["H0"], 30, check_every=2, tol=1.0)
    assert n_iter == nref == 6 and np.array_equal(np.isnan(tr), np.isnan(trref))
    close64(G, H, Gref, Href, "check_every=2")


@pytest.mark.parametrize("name", SHAPES)
def test_float32_within_four_times_the_restatements_distance(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    niter = int(d["niter"])
    G32, H32, _, tr32 = cr.learn(d["data"], d["G0"], d["H0"], niter, check_every=1, dtype=np.float32)
    dg, dh = nrel(G32, d["G"]), nrel(H32, d["H"])
    dt = max(nrel(tr32[1:], d["ferr"]), float(np.finfo(np.float32).eps))      # (at least the rounding of the stored factors)
    for layout in ("bin_major", "frame_major"):
        G, H, W, n_iter, tr = cabi(d["data"], d["G0"], d["H0"], niter, layout=layout, dtype=np.float32, pad=3, check_every=1)
        assert G.dtype == np.float32 and H.dtype == np.float32 and n_iter == niter
        print("%s %s G %.3e (d32 %.3e) H %.3e (d32 %.3e)" % (name, layout, nrel(G, d["G"]), dg, nrel(H, d["H"]), dh))
        assert nrel(G, d["G"]) <= 4 * dg and nrel(H, d["H"]) <= 4 * dh
        assert nrel(W, d["W"]) <= 4 * max(dg, nrel((d["data"].astype(np.float32) @ G32), d["W"]))
        print("ferr %.3e (d32 %.3e)" % (nrel(tr[1:], d["ferr"]), dt))
        assert nrel(tr[1:], d["ferr"]) <= 4 * dt


def test_nan_iters_zero_and_no_w():
    X, G0, H0 = problem(25, 70, 8)
    # iters = 0 touches only W; the error at the start is still evaluated
    G, H, W, n_iter, tr = cabi(X, G0, H0, 0, pad=2, check_every=1)
    assert np.array_equal(G, G0) and np.array_equal(H, H0) and n_iter == 0 and tr.shape == (1,)
    assert nrel(W, X @ G0) <= RTOL and tr[0] == pytest.approx(cr.frobenius(X, G0, H0), rel=1e-8)
    # W = NULL: the same bits in G and H
    with_w = cabi(X, G0, H0, 3, pad=2)
    without = cabi(X, G0, H0, 3, pad=2, want_w=False)
    assert np.array_equal(with_w[0], without[0]) and np.array_equal(with_w[1], without[1]) and without[2] is None
    # a NaN in one exemplar reaches K's row and column, and through pos(K) G everything - as in the restatement, no fault
    Xn = X.copy()
    Xn[3, 11] = np.nan
    Gref, Href, nref, trref = cr.learn(Xn, G0, H0, 3, check_every=1, tol=cr.PYMF_TOL)
    for layout in ("bin_major", "frame_major"):
        G, H, W, n_iter, tr = cabi(Xn, G0, H0, 3, layout=layout, pad=2, check_every=1, tol=cr.PYMF_TOL)
        assert np.array_equal(np.isnan(G), np.isnan(Gref)) and np.array_equal(np.isnan(H), np.isnan(Href))
        assert np.isnan(G).all() and np.isnan(H).all() and np.isnan(W).all()
        assert n_iter == nref == 3 and np.array_equal(np.isnan(tr), np.isnan(trref)) and np.isnan(tr).all()


def test_one_routed_size():
    M, T, R = 50, 4096, 256
    X, G0, H0 = problem(M, T, R)
    Gref, Href, _, trref = reference(M, T, R, 3, check_every=3)
    G, H, W, n_iter, tr = cabi(X, G0, H0, 3, layout="frame_major", check_every=3)
    close64(G, H, Gref, Href, "routed")
    assert n_iter == 3 and nrel(W, X @ Gref) <= RTOL
    np.testing.assert_allclose(tr, trref, rtol=1e-8, atol=0)


# ---- the Python surface ----
def test_compact_dictionary_convex_feeds_convert_semi():
    rng = np.random.default_rng(5)
    N, R, Ma = 300, 12, 25
    assign = (np.arange(N) * R) // N
    Ca, Cb = rng.standard_normal((Ma, R)), rng.standard_normal((Ma, R))       # planted, signed, parallel
    A = Ca[:, assign] + 0.2 * rng.standard_normal((Ma, N))
    B = Cb[:, assign] + 0.2 * rng.standard_normal((Ma, N))
    Wa, Wb, G, H, info = evc().compact_dictionary_convex(A, B, R, iters=40)
    assert Wa.shape == (Ma, R) and Wb.shape == (Ma, R) and G.shape == (N, R) and H.shape == (R, N)
    assert (G >= 0).all() and (H >= 0).all() and info["n_iter"] == 40
    D = np.vstack([A, B])
    assert nrel(np.vstack([Wa, Wb]), D @ G) <= 1e-12
    err = info["err"]
    assert err.shape == (41,) and np.isfinite(err).all() and err[-1] < err[0]
    assert np.all(np.diff(err) <= 1e-12 * err[:-1])                 # the error trace never rises
    assert err[-1] == pytest.approx(np.linalg.norm(D - (D @ G) @ H), rel=1e-8)
    # frame-major operands give the same factors
    Wa2, Wb2, G2, H2, _ = evc().compact_dictionary_convex(A.T.copy(), B.T.copy(), R, iters=40, layout="frame_major")
    assert nrel(G2, G) <= 1e-10 and nrel(H2.T, H) <= 1e-10 and nrel(Wa2.T, Wa) <= 1e-10 and nrel(Wb2.T, Wb) <= 1e-10
    # the caller's own labels
    _, _, G3, _, _ = evc().compact_dictionary_convex(A, B, R, iters=5, assign=assign[::-1].copy())
    assert G3.shape == (N, R) and np.isfinite(G3).all()
    # the compact pair goes straight into convert_semi
    X = Ca[:, rng.integers(0, R, 40)] + 0.1 * rng.standard_normal((Ma, 40))
    Y, Hx = evc().convert_semi(Wa, Wb, X, init="const", init_value=1.0, iters=30)
    assert Hx.shape == (R, 40) and Y.shape == (Ma, 40) and np.isfinite(Y).all() and (Hx >= 0).all()


def test_learn_dictionary_convex_surfaces():
    import torch
    X, G0, H0 = problem(25, 70, 8)
    Gref, Href, _, trref = reference(25, 70, 8, 4, check_every=2)
    W, G, H, info = evc().learn_dictionary_convex(X, G0, H0, layout="bin_major", iters=4, check_every=2, info=True)
    close64(G, H, Gref, Href, "numpy")
    assert info["n_iter"] == 4 and info["splits"] == 1 and nrel(W, X @ Gref) <= RTOL
    np.testing.assert_allclose(info["err"], trref, rtol=1e-8, atol=0)
    # device tensors in, device tensors out; out_g / out_h are updated in place; forced geometry
    Xd = torch.from_numpy(X.T.copy()).cuda()
    Gd, Hd = torch.from_numpy(G0).cuda(), torch.from_numpy(H0.T.copy()).cuda()
    W2, G2, H2 = evc().learn_dictionary_convex(Xd, None, None, layout="frame_major", iters=4, check_every=0, out_g=Gd, out_h=Hd,
                                               splits=3, waves=4)
    assert G2 is Gd and H2 is Hd and W2.shape == (8, 25) and W2.is_cuda
    assert nrel(Gd.cpu().numpy(), G) <= 1e-12 and nrel(Hd.cpu().numpy().T, H) <= 1e-12
