"""evc_kmeans on the GPU against recorded pymf results (tests/golden/kmeans_*.npz) and the numpy restatement
(tests/kmeans_restatement.py), which reproduces every one of them (tests/test_kmeans_host.py).

Labels, counts and n_iter are compared for EQUALITY.  Every such test first asserts, on the CPU, the margin condition of
tests/kmeans_restatement.py: over every sample of every assignment pass of the restatement the two least distances are
exactly equal or (d2 - d1) / (||x_t|| + max_r ||w_r||) >= 16 (M + 4) u of the type under test - a gap that no rounding of
either form of the distance can close, so a differing label would be a wrong label.  No sample is excluded.
float64 bounds: W per column ||w - w_ref|| <= 1e-8 ||w_ref||, the bound of the project's float64 parity tests (equal labels
leave means that differ by the order of at most T additions, some 1e-14); err 1e-8 relative.  float32: the labels are the
float64 restatement's; W within 4 d32, d32 the distance of the restatement run in float32 numpy from float64 (the rule of
tests/test_gpu_convex.py)."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmeans_restatement as kr  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ["kmeans_doctest", "kmeans_doctest_vq", "kmeans_m25_t70_r8", "kmeans_m40_t257_r17", "kmeans_m1_t64_r5",
            "kmeans_m513_t200_r17", "kmeans_vq_m25_t70_r8", "kmeans_dup_m25_t70_r8"]
CNMFD = ["cnmfd_doctest", "cnmfd_m25_t70_r8", "cnmfd_m40_t257_r17"]
GEOMETRY = [(1, 1), (5, 2), (16, 16), (17, 15), (63, 17), (64, 64), (65, 65), (129, 63), (257, 130), (300, 1), (300, 300)]
RTOL = 1e-8
_cache = {}


def evc():
    import exemplars_vc_amd
    return exemplars_vc_amd


def problem(M, T, R):
    key = (M, T, R)
    if key not in _cache:
        X = kr.problem(M, T, max(R // 2, 1), 11 * M + 5 * T + R)
        _cache[key] = (X, X[:, kr.spread_start(T, R)].copy())          # shared: the tests copy before they change one
    return _cache[key]


def reference(M, T, R, K, **kw):
    key = ("ref", M, T, R, K, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _cache:
        _cache[key] = kr.run(*problem(M, T, R), K, **kw)
    return _cache[key]


def worst_column(A, ref):
    A, ref = np.asarray(A, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert A.shape == ref.shape
    num, den = np.linalg.norm(A - ref, axis=0), np.linalg.norm(ref, axis=0)
    assert not num[den == 0].any()
    return float(np.max(num[den > 0] / den[den > 0])) if (den > 0).any() else 0.0


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), np.finfo(float).tiny))) if a.size else 0.0


def cabi(X, W0, iters, *, layout="bin_major", dtype=np.float64, pad=0, update="both", stop="pymf", tol=kr.PYMF_TOL, splits=0,
         redecide=False, want=True):
    """evc_kmeans through ctypes on bin-major numpy operands, laid out as `layout` says; every buffer's leading dimension is
    `pad` longer than needed and its padding holds NaN, which must still be there afterwards; labels and counts lie between
    guard words.  -> W (M x R), labels, counts, n_iter, trace"""
    import torch
    from exemplars_vc_amd import _lib
    L = _lib.lib()
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    fm = layout == "frame_major"
    (M, T), R = X.shape, W0.shape[1]

    def stage(mat):
        m = np.asarray(mat, dtype=dtype)
        m = m.T if fm else m
        buf = torch.full((m.shape[0], m.shape[1] + pad), float("nan"), dtype=tdt, device="cuda")
        buf[:, :m.shape[1]] = torch.from_numpy(np.ascontiguousarray(m))
        return buf, m.shape[1]
    (X_d, xcols), (W_d, wcols) = stage(X), stage(W0)
    lab = torch.full((T + 2,), -7, dtype=torch.int32, device="cuda")
    cnt = torch.full((R + 2,), -7, dtype=torch.int32, device="cuda")
    o = _lib.KmeansOpts()
    o.struct_bytes = C.sizeof(o)
    o.dtype, o.layout, o.iters = (_lib.F64 if dtype == np.float64 else _lib.F32), (_lib.FRAME_MAJOR if fm else _lib.BIN_MAJOR), iters
    o.update = {"both": _lib.KM_BOTH, "assign": _lib.KM_ASSIGN_ONLY}[update]
    o.stop_rule = {"none": _lib.KM_STOP_NONE, "pymf": _lib.KM_STOP_PYMF, "labels": _lib.KM_STOP_LABELS}[stop]
    o.tol, o.reserved = tol, (splits << 8) | (1 if redecide else 0)
    n_iter, trace = C.c_int(-1), np.full(1 + iters, -1.0)
    nbytes = int(L.evc_kmeans_workspace_bytes(M, R, T, o.dtype))
    assert nbytes > 0
    if splits > 1:
        nbytes += splits * (T * (2 * (8 if dtype == np.float64 else 4) + 4) + 3 * 256)
    ws = torch.empty(nbytes + 8, dtype=torch.uint8, device="cuda")
    ld = lambda t: int(t.stride(0))      # noqa: E731
    st = L.evc_kmeans(X_d.data_ptr(), ld(X_d), W_d.data_ptr(), ld(W_d), lab.data_ptr() + 4 if want else None,
                      cnt.data_ptr() + 4 if want else None, M, R, T, C.byref(o), ws.data_ptr() + 8, nbytes, C.byref(n_iter),
                      trace.ctypes.data_as(C.POINTER(C.c_double)), None)
    assert st == 0, st
    torch.cuda.synchronize()
    Xa, Wa, lab, cnt = X_d.cpu().numpy(), W_d.cpu().numpy(), lab.cpu().numpy(), cnt.cpu().numpy()
    if pad:
        assert np.isnan(Xa[:, xcols:]).all() and np.isnan(Wa[:, wcols:]).all()        # nothing outside the logical elements
    assert np.array_equal(Xa[:, :xcols], np.asarray(X, dtype=dtype).T if fm else np.asarray(X, dtype=dtype))
    assert lab[0] == -7 and lab[-1] == -7 and cnt[0] == -7 and cnt[-1] == -7
    if not want:
        assert (lab == -7).all() and (cnt == -7).all()
    W = Wa[:, :wcols].T if fm else Wa[:, :wcols]
    return np.ascontiguousarray(W), lab[1:-1], cnt[1:-1], int(n_iter.value), trace


def check64(got, ref, M, what=""):
    """(W, labels, counts, n_iter, trace) of the device against the restatement's (W, labels, counts, n_iter, trace, margin)"""
    W, labels, counts, n_iter, trace = got
    Wr, lr, cr_, nr, tr, margin = ref
    assert margin >= kr.margin_bound(M, np.float64), margin            # the condition of a comparison of labels
    ww = worst_column(W, Wr)
    we = rel(trace[:nr + 1], tr[:nr + 1])
    print("%s worst column W %.3e err %.3e margin %.3e" % (what, ww, we, margin))
    assert np.array_equal(labels, lr) and np.array_equal(counts, cr_) and n_iter == nr and counts.sum() == len(labels)
    assert ww <= RTOL and we <= RTOL
    assert np.isnan(trace[nr + 1:]).all()


@pytest.mark.parametrize("name", FIXTURES)
def test_goldens_through_ctypes_and_the_mirror(name):
    from exemplars_vc_amd.compat import pymf
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    niter, (M, T), cw = int(d["niter"]), d["data"].shape, bool(d["compute_w"])
    R = d["W0"].shape[1]
    ref = kr.run(d["data"], d["W0"], niter, update="both" if cw else "assign")
    assert ref[5] >= kr.margin_bound(M, np.float64)
    for layout in ("bin_major", "frame_major"):
        W, labels, counts, n_iter, trace = cabi(d["data"], d["W0"], niter, layout=layout, pad=3, update="both" if cw else "assign")
        ferr = kr.pymf_ferr(trace, n_iter, niter, T)
        print(name, layout, "W", worst_column(W, d["W"]), "ferr", rel(ferr, d["ferr"]) if len(ferr) == len(d["ferr"]) else None)
        assert np.array_equal(labels, d["assigned"]) and np.array_equal(counts, np.bincount(d["assigned"], minlength=R))
        assert n_iter == int(d["n_iter"]) and len(ferr) == len(d["ferr"])
        assert worst_column(W, d["W"]) <= RTOL and rel(ferr, d["ferr"]) <= RTOL
    state = random.getstate()
    try:
        random.seed(int(d["seed"]))
        mdl = pymf.Kmeans(d["data"].copy(), num_bases=R)
        if not cw or name == "kmeans_dup_m25_t70_r8":
            mdl.W = d["W0"].copy()
        mdl.factorize(niter=niter, compute_w=cw)
    finally:
        random.setstate(state)
    assert np.array_equal(mdl.assigned, d["assigned"]) and mdl.ferr.shape == d["ferr"].shape
    assert worst_column(mdl.W, d["W"]) <= RTOL and rel(mdl.ferr, d["ferr"]) <= RTOL
    H = np.zeros((R, T))
    H[d["assigned"], np.arange(T)] = 1.0
    assert mdl.H.dtype == np.float64 and np.array_equal(mdl.H, H)


@pytest.mark.parametrize("T,R", GEOMETRY)
def test_geometry_against_the_restatement(T, R):
    for i, M in enumerate((1, 25, 40)):
        X, W0 = problem(M, T, R)
        ref = reference(M, T, R, 5)
        for layout in ("bin_major", "frame_major"):
            got = cabi(X, W0, 5, layout=layout, pad=1 + 2 * i)
            check64(got, ref, M, "M=%d T=%d R=%d %s" % (M, T, R, layout))


@pytest.mark.parametrize("M,T,R", [(513, 63, 17), (1056, 129, 63)])
def test_geometry_with_more_than_one_chunk_of_bins(M, T, R):
    X, W0 = problem(M, T, R)
    for layout in ("bin_major", "frame_major"):
        check64(cabi(X, W0, 4, layout=layout, pad=5), reference(M, T, R, 4), M, "M=%d %s" % (M, layout))


def test_stop_rules_and_the_options():
    X, W0 = problem(25, 300, 9)
    for stop in ("labels", "none", "pymf"):
        check64(cabi(X, W0, 12, stop=stop), reference(25, 300, 9, 12, stop=stop), 25, stop)
    assert reference(25, 300, 9, 12, stop="labels")[3] < 12                     # the rule fired
    check64(cabi(X, W0, 4, update="assign"), reference(25, 300, 9, 4, update="assign"), 25, "assign")
    check64(cabi(X, W0, 0), reference(25, 300, 9, 0), 25, "iters=0")
    got = cabi(X, W0, 3, want=False)                                            # labels and counts are optional
    assert worst_column(got[0], reference(25, 300, 9, 3)[0]) <= RTOL


def test_forced_centre_ranges_give_the_same_bits():
    X, W0 = problem(40, 257, 130)
    ref = reference(40, 257, 130, 5)
    base = cabi(X, W0, 5, splits=1)
    check64(base, ref, 40, "S=1")
    for S in (2, 3, 16):
        for layout in ("bin_major", "frame_major"):
            got = cabi(X, W0, 5, splits=S, layout=layout, pad=2)
            assert np.array_equal(got[1], base[1]) and np.array_equal(got[2], base[2]) and got[3] == base[3]
            assert worst_column(got[0], base[0]) <= 1e-12 and rel(got[4][:got[3] + 1], base[4][:base[3] + 1]) <= 1e-12


def test_forced_redecision_of_every_sample_changes_nothing():
    for M, T, R in ((40, 257, 130), (25, 129, 63)):
        X, W0 = problem(M, T, R)
        base = cabi(X, W0, 5)
        check64(base, reference(M, T, R, 5), M)
        for S in (0, 3):
            got = cabi(X, W0, 5, redecide=True, splits=S)
            assert np.array_equal(got[1], base[1]) and np.array_equal(got[0], base[0]) and np.array_equal(got[4], base[4], equal_nan=True)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_ties_go_to_the_lowest_index(dtype):
    """integer-valued data and centres: both forms of the distance are exact, duplicated centres tie exactly"""
    rng = np.random.default_rng(5)
    M, T, R = 25, 200, 130
    W0 = rng.integers(-4, 5, (M, R)).astype(np.float64)
    groups = [(3, 19, 35, 99, 129), (40, 41), (64, 128)]              # other MFMA tile, other centre tile, other centre range
    for g in groups:
        W0[:, g[1:]] = W0[:, g[:1]]
    X = W0[:, rng.integers(0, R, T)] + rng.integers(-1, 2, (M, T))
    X[:, :len(groups)] = W0[:, [g[-1] for g in groups]]               # a sample on each duplicated centre
    ref = kr.assign(X.astype(dtype), W0.astype(dtype))[0]
    higher = [r for g in groups for r in g[1:]]
    assert not np.isin(ref, higher).any() and list(ref[:len(groups)]) == [g[0] for g in groups]
    for S in (0, 1, 2, 3, 16):
        for redecide in (False, True):
            for layout in ("bin_major", "frame_major"):
                got = cabi(X, W0, 0, dtype=dtype, update="assign", stop="none", splits=S, redecide=redecide, layout=layout, pad=1)
                assert np.array_equal(got[1], ref), (S, redecide, layout)


def test_guard_hands_close_calls_to_the_direct_form():
    """a sample ON one centre and 1e-9 ||x|| from another of LOWER index, ||x||^2 ~ 1e6: the expanded scores cannot tell them
    apart (their rounding error is some 1e-10 ||x||^2, the gap 1e-18 ||x||^2); the direct form's answer is the centre at 0"""
    rng = np.random.default_rng(9)
    M, T, R = 25, 70, 17
    X = rng.standard_normal((M, T))
    X *= 1000.0 / np.linalg.norm(X, axis=0)
    W0 = X[:, kr.spread_start(T, R)].copy()
    for t, (near, on) in ((5, (2, 11)), (33, (0, 16)), (69, (7, 8))):
        W0[:, on] = X[:, t]
        W0[:, near] = X[:, t]
        W0[3, near] += 1e-9 * np.linalg.norm(X[:, t])
        assert 0 < np.linalg.norm(W0[:, near] - X[:, t]) < 2e-6
    ref = kr.assign(X, W0)[0]
    assert ref[5] == 11 and ref[33] == 16 and ref[69] == 8
    for S in (0, 2):
        for layout in ("bin_major", "frame_major"):
            got = cabi(X, W0, 0, update="assign", stop="none", splits=S, layout=layout)
            assert np.array_equal(got[1], ref), (S, layout)


def test_an_empty_cluster_keeps_its_centre_bit_for_bit():
    X, W0 = problem(25, 129, 63)
    W0 = W0.copy()
    W0[:, [0, 17, 62]] = 50.0 + np.arange(3)                       # nobody's nearest
    for dtype in (np.float64, np.float32):
        for layout in ("bin_major", "frame_major"):
            W, labels, counts, n_iter, _ = cabi(X, W0, 4, dtype=dtype, layout=layout, pad=2)
            assert counts.sum() == 129 and (counts[[0, 17, 62]] == 0).all() and np.array_equal(counts, np.bincount(labels, minlength=63))
            assert np.array_equal(W[:, [0, 17, 62]], W0[:, [0, 17, 62]].astype(dtype))
            moved = counts > 1
            assert moved.any() and not (W[:, moved] == W0[:, moved].astype(dtype)).all(axis=0).any()      # every other centre is a mean now


def test_the_same_call_gives_the_same_bits():
    X, W0 = problem(40, 257, 130)
    for dtype in (np.float64, np.float32):
        a = cabi(X, W0, 6, dtype=dtype, stop="none")
        b = cabi(X, W0, 6, dtype=dtype, stop="none")
        assert all(np.array_equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("name", ["kmeans_m40_t257_r17", "kmeans_m25_t70_r8", "kmeans_dup_m25_t70_r8", "kmeans_m1_t64_r5"])
def test_float32_against_the_float64_restatement(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    M, niter = d["data"].shape[0], int(d["niter"])
    ref = kr.run(d["data"], d["W0"], niter)
    r32 = kr.run(d["data"], d["W0"], niter, dtype=np.float32)
    assert min(ref[5], r32[5]) >= kr.margin_bound(M, np.float32), (ref[5], r32[5])       # float32 labels are comparable here
    d32 = worst_column(r32[0], ref[0])
    for layout in ("bin_major", "frame_major"):
        W, labels, counts, n_iter, trace = cabi(d["data"], d["W0"], niter, dtype=np.float32, layout=layout, pad=3)
        ww = worst_column(W, ref[0])
        print(name, layout, "float32 worst column %.3e, numpy float32 %.3e" % (ww, d32))
        assert W.dtype == np.float32 and np.array_equal(labels, ref[1]) and np.array_equal(counts, ref[2]) and n_iter == ref[3]
        assert ww <= 4 * d32 and rel(trace[:n_iter + 1], ref[4][:n_iter + 1]) <= 1e-5


@pytest.mark.parametrize("name", CNMFD)
def test_cnmf_start_on_the_device(name):
    from exemplars_vc_amd.compat import pymf
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    (M, T), R, niter = d["data"].shape, d["G0"].shape[1], int(d["niter"])
    state = random.getstate()
    try:
        random.seed(int(d["seed"]))
        W0 = d["data"][:, np.sort(random.sample(range(T), R))]
        assert kr.run(d["data"], W0, 10)[5] >= kr.margin_bound(M, np.float64)
        random.seed(int(d["seed"]))
        mdl = pymf.CNMF(d["data"].copy(), num_bases=R, start="device")
        mdl._init_h()
        assert np.array_equal(mdl.G, d["G0"]) and np.array_equal(mdl.H, d["H0"])
        mdl.factorize(niter=niter)
    finally:
        random.setstate(state)
    assert mdl.ferr.shape == d["ferr"].shape
    assert worst_column(mdl.G, d["G"]) <= RTOL and worst_column(mdl.H, d["H"]) <= RTOL and rel(mdl.ferr, d["ferr"]) <= RTOL


def test_compaction_by_vector_quantisation():
    e = evc()
    rng = np.random.default_rng(77)
    N, R, Ma, Mb = 300, 33, 25, 20
    lab0 = rng.integers(0, 12, N)
    A = np.abs(rng.standard_normal((Ma, 12)))[:, lab0] + 0.1 * rng.random((Ma, N))
    B = np.abs(rng.standard_normal((Mb, 12)))[:, lab0] + 0.1 * rng.random((Mb, N))
    D = np.vstack([A, B])
    ref = kr.run(D, D[:, kr.spread_start(N, R)], 10, stop="labels")
    assert ref[5] >= kr.margin_bound(Ma + Mb, np.float64)
    Wa, Wb, labels, info = e.compact_dictionary_kmeans(A, B, R)
    assert np.array_equal(labels, ref[1]) and info["n_iter"] == ref[3] and np.array_equal(info["counts"], ref[2])
    assert Wa.shape == (Ma, R) and Wb.shape == (Mb, R) and (Wa >= 0).all() and (Wb >= 0).all()
    for r in range(R):
        idx = labels == r
        assert idx.any()
        assert np.linalg.norm(Wa[:, r] - A[:, idx].mean(axis=1)) <= 1e-12 * np.linalg.norm(Wa[:, r])
        assert np.linalg.norm(Wb[:, r] - B[:, idx].mean(axis=1)) <= 1e-12 * np.linalg.norm(Wb[:, r])
    H, Y = e.convert(Wa, A[:, :40], Wb, layout="bin_major", iters=20)        # the codebook as a parallel dictionary
    assert H.shape == (R, 40) and Y.shape == (Mb, 40) and np.isfinite(Y).all() and (Y >= 0).all()
    WaT, WbT, labT, _ = e.compact_dictionary_kmeans(A.T.copy(), B.T.copy(), R, layout="frame_major")
    assert np.array_equal(labT, labels) and np.array_equal(WaT.T, Wa) and np.array_equal(WbT.T, Wb)
    picked = e.compact_dictionary_kmeans(A, B, R, init=kr.spread_start(N, R))
    assert np.array_equal(picked[2], labels) and np.array_equal(picked[0], Wa)
    c1 = e.compact_dictionary_convex(A, B, R, iters=5, assign="kmeans")
    c2 = e.compact_dictionary_convex(A, B, R, iters=5, assign=labels)
    assert all(np.array_equal(p, q) for p, q in zip(c1[:4], c2[:4])) and np.array_equal(c1[4]["err"], c2[4]["err"])
    c0 = e.compact_dictionary_convex(A, B, R, iters=5)                          # the default start did not move
    c3 = e.compact_dictionary_convex(A, B, R, iters=5, assign=(np.arange(N) * R) // N)
    assert all(np.array_equal(p, q) for p, q in zip(c0[:4], c3[:4]))


def test_python_surface_on_the_device():
    import torch
    e = evc()
    X, W0 = problem(25, 129, 63)
    ref = reference(25, 129, 63, 5)
    W, labels, info = e.kmeans(X, W0, layout="bin_major", iters=5, info=True)
    assert isinstance(W, np.ndarray) and labels.dtype == np.int32 and info["splits"] == 2
    check64((W, labels, info["counts"], info["n_iter"], info["err"]), ref, 25, "kmeans()")
    Xd, Wd = torch.from_numpy(X.T.copy()).cuda(), torch.from_numpy(W0.T.copy()).cuda()
    keep = Wd.clone()
    Wt, lt, it = e.kmeans(Xd, Wd, layout="frame_major", iters=5, info=True, splits=3)
    assert isinstance(Wt, torch.Tensor) and torch.equal(Wd, keep) and it["splits"] == 3          # the start is not clobbered
    assert np.array_equal(lt.cpu().numpy(), labels) and np.array_equal(Wt.cpu().numpy().T, W)
    assert np.array_equal(e.vq(W0, X, layout="bin_major"), kr.assign(X, W0)[0])
    assert np.array_equal(e.vq(W0, X[:, :7], layout="bin_major"), kr.assign(X[:, :7], W0)[0])      # more centres than samples
    with pytest.raises(ValueError, match="centres"):
        e.kmeans(X[:, :7], W0, layout="bin_major")
