"""evc_prox_masked_solve on the GPU against recorded masked deComP runs (tests/golden/proxm_*.npz) and the numpy restatement
(tests/prox_masked_restatement.py), which reproduces every one of them bit for bit (tests/test_prox_masked_host.py).

Everything here is in deComP's orientation: y is T x M, A is N x M (exemplars as rows), x is T x N, mask is T x M.

The bound is tests/test_gpu_prox.py's scheme: max |x - ref| <= 100 figure max |ref|.  `figure` is the fixture's `perm64` /
`perm32`: how far the restatement's result moves when the exemplars AND the bins are permuted (the factored sweep sums over
both), as tools/make_golden_prox_masked.py records it.  Shapes without a fixture get the same recipe computed in the test
(pmr.permutation_figure), with a floor of K eps for K updates.  n_iter equals the recorded `it` + 1 and every activation that
the reference's threshold cuts by more than 1e-6 thr is exactly 0.0.  float32: fixed iteration counts, against the float64
restatement within 100 perm32.
Measured on an MI355X, float64 (the table of DESIGN.md §5.18; permutation figures 2.7e-16 .. 3.6e-13, signed 4.9e-9):
1.4e-16 .. 1.3e-13 on the non-negative fixtures, 5.3e-9 on the signed one, at most 5.1e-15 over the geometry sweep (1 % of its
bound) and 1.2e-15 at N = 4096; a NULL mask against evc_prox_solve 1.3e-14, deleted bins against evc_prox_solve 8.9e-15;
float32 (figures 2.2e-7 .. 1.9e-4, signed 5.0e-3): 3.8e-7 .. 2.1e-4 and 4.9e-3."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prox_masked_restatement as pmr  # noqa: E402
import prox_restatement as pr  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ["proxm_m25_n64_t32_fista_pos", "proxm_m40_n130_t33_ista_pos", "proxm_m25_n64_t32_fista", "proxm_m1_n5_t3_fista_pos",
            "proxm_m201_n300_t20_fista_pos", "proxm_m25_n64_t32_fista_pos_k50", "proxm_m25_n64_t32_fista_pos_start"]
_cache = {}


def evc():
    import exemplars_vc_amd
    return exemplars_vc_amd


def load(name):
    if name not in _cache:
        d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
        d["y"], d["A"], d["mask"] = d["y"].astype(np.float64), d["A"].astype(np.float64), d["mask"].astype(np.float64)
        d["positive"], d["momentum"] = pr.split_method(str(d["method"]))
        d["kw"] = dict(alpha=float(d["alpha"]), tol=float(d["tol"]), positive=d["positive"], momentum=d["momentum"])
        _cache[name] = d                                          # shared: the tests copy before they change one
    return _cache[name]


def problem(M, N, T, seed=0, signed=False, kind="binary"):
    """y, A, mask - computed once per shape and left unchanged"""
    key = (M, N, T, seed, signed, kind)
    if key not in _cache:
        s = 1000 * seed + 7 * M + 3 * N + T
        _cache[key] = pr.problem(M, N, T, s, signed=signed) + (pmr.problem_mask(T, M, s, kind),)
    return _cache[key]


def reference(y, A, mask, K, **kw):
    """the restatement of K updates and its permutation figure: (x, n_iter, trace), figure"""
    kw = dict(dict(alpha=1e-3, tol=0.0), **kw)
    fkw = {k: v for k, v in kw.items() if k != "utt_offsets"}
    offs = kw.get("utt_offsets")
    if offs is None:
        fig = pmr.permutation_figure(y, A, mask, K, np.float64, **fkw)
    else:                                                           # wbar is per utterance: so is the figure
        fig = max(pmr.permutation_figure(y[a:b], A, None if mask is None else mask[a:b], K, np.float64, **fkw)
                  for a, b in zip(offs[:-1], offs[1:]) if b > a)
    return pmr.solve(y, A, mask=mask, iters=K, **kw), fig


def close(x, ref, figure, what=""):
    """max |x - ref| <= 100 figure max |ref|; NaN where and only where the reference has NaN"""
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert x.shape == ref.shape and np.array_equal(np.isnan(x), np.isnan(ref))
    good = ~np.isnan(ref)
    top = float(np.max(np.abs(ref[good]))) if good.any() else 0.0
    diff = float(np.max(np.abs(x[good] - ref[good]))) if good.any() else 0.0
    worst = diff / top if top > 0 else diff
    print("%s: max error %.3e of max |x| (allowed %.3e)" % (what, worst, 100 * figure))
    assert worst <= 100 * figure
    return worst


def stat_close(tr, rtr, fig, ref, A, normalize=True):
    """the stop statistics: differences of activations in the solve's own scaling (x d, d the exemplars' norms), so twice
    the activations' bound times the largest norm"""
    d = float(np.max(np.linalg.norm(A, axis=1))) if normalize else 1.0
    assert np.array_equal(np.isfinite(tr), np.isfinite(rtr))
    np.testing.assert_allclose(tr, rtr, rtol=0, atol=2 * 100 * fig * float(np.nanmax(np.abs(ref))) * d)


def cabi(y, A, mask, x0, iters, *, alpha=1e-3, tol=0.0, positive=True, momentum="fista", normalize=True, check_every=10,
         stop_rule="decomp", lipschitz=0.0, lip_weights="mean", layout="frame_major", dtype=np.float64, pad=0, mpad=None,
         offs=None, init_value=None):
    """evc_prox_masked_solve through ctypes: every matrix is laid out as `layout` says inside a buffer whose leading dimension
    is `pad` longer than needed (the mask's: `mpad`, by default pad + 2, so ldm differs from ldx) and whose padding holds
    NaN, which must still be there afterwards.  mask None: a NULL pointer.  x0 None: EVC_INIT_CONST with init_value (default 0)
    over a buffer full of NaN.  -> x (T x N), n_iter, trace"""
    import torch
    from exemplars_vc_amd import _lib
    L = _lib.lib()
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    fm = layout == "frame_major"
    (N, M), T = A.shape, y.shape[0]
    mpad = pad + 2 if mpad is None else mpad

    def stage(mat, extra):
        m = np.asarray(mat, dtype=dtype)
        m = m if fm else m.T
        buf = torch.full((m.shape[0], m.shape[1] + extra), float("nan"), dtype=tdt, device="cuda")
        buf[:, :m.shape[1]] = torch.from_numpy(np.ascontiguousarray(m))
        return buf, m.shape[1]
    (A_d, acols), (X_d, xcols) = stage(A, pad), stage(y, pad)
    M_d, mcols = (None, 0) if mask is None else stage(mask, mpad)
    H_d, hcols = stage(np.full((T, N), np.nan) if x0 is None else x0, pad)
    o = _lib.ProxMaskedOpts()
    o.struct_bytes = C.sizeof(o)
    o.dtype, o.layout, o.iters = (_lib.F64 if dtype == np.float64 else _lib.F32), (_lib.FRAME_MAJOR if fm else _lib.BIN_MAJOR), iters
    o.mode = _lib.PROX_POSITIVE if positive else _lib.PROX_SIGNED
    o.momentum = {"ista": _lib.PROX_ISTA, "fista": _lib.PROX_FISTA, "nesterov": _lib.PROX_NESTEROV}[momentum]
    o.normalize, o.check_every = int(normalize), check_every
    o.stop_rule = {"none": _lib.STOP_NONE, "decomp": _lib.STOP_DECOMP}[stop_rule]
    o.init_mode = _lib.INIT_CONST if x0 is None else _lib.INIT_GIVEN
    o.lip_weights = {"mean": _lib.PROX_LIP_MEAN, "max": _lib.PROX_LIP_MAX}[lip_weights]
    o.alpha, o.tol, o.init_value, o.lipschitz = alpha, tol, (0.0 if init_value is None else init_value), lipschitz
    n_utt = 1 if offs is None else len(offs) - 1
    po = None if offs is None else (C.c_int * len(offs))(*offs)
    slots = pr.n_slots(iters, check_every)
    n_iter, trace = np.zeros(n_utt, dtype=np.int32), np.full((n_utt, max(slots, 1)), -1.0)
    nbytes = int(L.evc_prox_masked_workspace_bytes(M, N, T, n_utt, o.dtype))
    assert nbytes > 0
    ws = torch.empty(nbytes + 8, dtype=torch.uint8, device="cuda")
    ld = lambda t: int(t.stride(0))      # noqa: E731
    st = L.evc_prox_masked_solve(A_d.data_ptr(), ld(A_d), X_d.data_ptr(), ld(X_d), None if M_d is None else M_d.data_ptr(),
                                 0 if M_d is None else ld(M_d), H_d.data_ptr(), ld(H_d), M, N, T, po, n_utt, C.byref(o),
                                 ws.data_ptr() + 8, nbytes, n_iter.ctypes.data_as(C.POINTER(C.c_int)),
                                 trace.ctypes.data_as(C.POINTER(C.c_double)), None)
    assert st == 0, st
    torch.cuda.synchronize()
    out = H_d.cpu().numpy()
    for buf, cols in ((H_d, hcols), (A_d, acols), (X_d, xcols)) + (() if M_d is None else ((M_d, mcols),)):
        if buf.shape[1] > cols:
            assert bool(torch.isnan(buf[:, cols:]).all())           # no padding was overwritten
    out = out[:, :hcols]
    trace = trace.reshape(-1)[:n_utt * slots].reshape(n_utt, slots)
    return (out if fm else out.T).copy(), n_iter, trace


def gram(y, A, x0, iters, *, alpha=1e-3, tol=0.0, positive=True, momentum="fista", normalize=True, check_every=10, lipschitz=0.0,
         offs=None):
    """evc_prox_solve (the Gram sweep) on the same problem, through the Python API -> x (T x N), n_iter"""
    H, info = evc().solve_activations_prox(A, y, x0, alpha=alpha, tol=tol, positive=positive, momentum=momentum,
                                           normalize=normalize, iters=iters, check_every=check_every,
                                           lipschitz=lipschitz or None, layout="frame_major", utt_offsets=offs, info=True)
    assert info["kernel"] == "k_prox_sweep"
    return H, info["n_iter"]


# ---- 1. the fixtures, through the C ABI in both layouts and through compat.decomp ----
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_through_the_c_abi(name):
    d = load(name)
    K = int(d["maxiter"])
    x0 = np.zeros_like(d["x"]) if "x0" not in d else d["x0"]
    _, _, rtr, pre, thr = pmr.solve_one(d["y"], d["A"], d["mask"], d["kw"]["alpha"], x0, d["kw"]["tol"], K,
                                        positive=d["positive"], momentum=d["momentum"], want_pre=True)
    cut = pre < -1e-6 * thr
    assert cut.any() or d["A"].shape[1] == 1      # one bin: the zeros are the masked frames', whose threshold is 0 (cnt_t = 0)
    for layout in ("frame_major", "bin_major"):
        x, n_iter, tr = cabi(d["y"], d["A"], d["mask"], d.get("x0"), K, layout=layout, pad=3, **d["kw"])
        assert x.dtype == np.float64 and int(n_iter[0]) == int(d["it"]) + 1
        close(x, d["x"], float(d["perm64"]), name + " " + layout)
        assert not x[cut].any()                                     # exact zeros where the threshold cuts
        if d["positive"]:
            assert (x >= 0).all()
        stat_close(tr[0], rtr, float(d["perm64"]), d["x"], d["A"])
    if "offs" in d:                                                 # the recorded per-utterance deComP runs
        offs = d["offs"].tolist()
        x, n_iter, tr = cabi(d["y"], d["A"], d["mask"], None, K, offs=offs, layout="bin_major", pad=1, **d["kw"])
        assert n_iter.tolist() == (d["it_split"] + 1).tolist()
        close(x, d["x_split"], float(d["perm64"]), name + " batch")


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_through_compat_decomp(name):
    from exemplars_vc_amd.compat import decomp
    d = load(name)
    x0 = None if "x0" not in d else d["x0"].copy()
    mask = d["mask"].copy()
    it, x = decomp.lasso.solve(d["y"], d["A"], d["kw"]["alpha"], x=x0, tol=d["kw"]["tol"], method=str(d["method"]),
                               maxiter=int(d["maxiter"]), mask=mask)
    assert it == int(d["it"]) and x.dtype == np.float64
    close(x, d["x"], float(d["perm64"]), name)
    assert np.array_equal(mask, d["mask"]) and (x0 is None or np.array_equal(x0, d["x0"]))      # the caller's arrays are not written
    if name == "proxm_m25_n64_t32_fista_pos_k50":                   # leading dimensions are flattened, nnls adds '_pos'
        it, x3 = decomp.nnls.solve(d["y"].reshape(4, 8, 25), d["A"], 1e-3, tol=0.0, method="fista", maxiter=50,
                                   mask=d["mask"].reshape(4, 8, 25))
        assert it == 49 and x3.shape == (4, 8, 64) and np.array_equal(x3.reshape(32, 64), x)


# ---- 2. geometry: every tile edge of both kernels and the fully idle wavefronts, 10 updates, binary mask ----
GEOMETRY = [(M, 130, 65) for M in (1, 15, 16, 17, 65, 129)] + [(25, N, 65) for N in (1, 15, 16, 17, 127, 128, 129, 257)] + \
           [(25, 130, T) for T in (1, 15, 63, 64, 65, 130)]


@pytest.mark.parametrize("M,N,T", GEOMETRY)
def test_geometry(M, N, T):
    y, A, mask = problem(M, N, T)
    (ref, _, rtr), fig = reference(y, A, mask, 10, check_every=5, lip_weights="max")
    for layout in ("frame_major", "bin_major"):
        x, n_iter, tr = cabi(y, A, mask, None, 10, layout=layout, pad=7, check_every=5, lip_weights="max")
        assert n_iter.tolist() == [10] and tr.shape == (1, 2)
        close(x, ref, fig, "M %d N %d T %d %s" % (M, N, T, layout))
        stat_close(tr, rtr, fig, ref, A)
        assert (x >= 0).all()


# ---- 3. layouts: every leading dimension padded, ldm differently from ldx; a non-contiguous device tensor ----
def test_layouts_and_strides():
    import torch
    y, A, mask = problem(25, 33, 70, signed=True, kind="weights")
    (ref, _, _), fig = reference(y, A, mask, 8, positive=False, lip_weights="max")
    assert (ref < 0).any() and (ref == 0).any()
    for layout in ("frame_major", "bin_major"):
        for pad, mpad in ((0, 0), (1, 6), (4, 0)):
            x, _, _ = cabi(y, A, mask, None, 8, layout=layout, pad=pad, mpad=mpad, positive=False, lip_weights="max")
            close(x, ref, fig, "%s pad %d mask pad %d" % (layout, pad, mpad))
    # the Python API: a transposed (non-contiguous) mask and a column slice of a wider X on the device
    wide = torch.from_numpy(np.concatenate([y, np.full((70, 3), np.nan)], axis=1)).cuda()
    Xs, Mt = wide[:, :25], torch.from_numpy(np.ascontiguousarray(mask.T)).cuda().t()
    assert not Mt.is_contiguous() and not Xs.is_contiguous()
    H = evc().solve_activations_prox(torch.from_numpy(A).cuda(), Xs, alpha=1e-3, tol=0.0, iters=8, positive=False, mask=Mt,
                                     layout="frame_major")
    assert isinstance(H, torch.Tensor) and H.is_cuda
    close(H.cpu().numpy(), ref, fig, "non-contiguous tensors")
    Hb = evc().solve_activations_prox(A.T.copy(), y.T.copy(), alpha=1e-3, tol=0.0, iters=8, positive=False, mask=mask.T.copy())
    close(Hb.T, ref, fig, "numpy, bin_major, the default weights")


# ---- 4. a batch is its utterances, bitwise ----
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_batch_equals_per_utterance(dtype):
    d = load("proxm_m40_n130_t33_ista_pos")                         # its two utterances stop at different iterations
    offs, K = d["offs"].tolist(), int(d["maxiter"])
    kw = dict(d["kw"], dtype=dtype, layout="bin_major", pad=2)
    x, n_iter, tr = cabi(d["y"], d["A"], d["mask"], None, K, offs=offs, **kw)
    x2, n_iter2, tr2 = cabi(d["y"], d["A"], d["mask"], None, K, offs=offs, **kw)
    assert np.array_equal(x, x2) and np.array_equal(n_iter, n_iter2) and np.array_equal(tr, tr2, equal_nan=True)
    for u in range(len(offs) - 1):
        a, b = offs[u], offs[u + 1]
        xu, nu, tu = cabi(d["y"][a:b], d["A"], d["mask"][a:b], None, K, **kw)
        assert np.array_equal(x[a:b], xu) and nu[0] == n_iter[u] and np.array_equal(tr[u], tu[0], equal_nan=True)
    if dtype == np.float64:
        assert n_iter.tolist() == (d["it_split"] + 1).tolist() and len(set(n_iter.tolist())) > 1
        close(x, d["x_split"], float(d["perm64"]), "batch")
        for u in range(len(offs) - 1):                              # nothing is recorded after an utterance's stop
            c = (int(n_iter[u]) - 1) // 10
            assert np.isfinite(tr[u, :c + 1]).all() and np.isnan(tr[u, c + 1:]).all()
        # a stopped utterance's frames do not change afterwards: they hold the iterate of its last update
        u = int(np.argmin(n_iter))
        a, b = offs[u], offs[u + 1]
        xs, _, _ = cabi(d["y"][a:b], d["A"], d["mask"][a:b], None, int(n_iter[u]), stop_rule="none", **kw)
        assert np.array_equal(x[a:b], xs)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_batch_of_different_masks_equals_per_utterance(dtype):
    y, A, mask = (m.copy() for m in problem(25, 70, 150, seed=2))
    offs = [0, 64, 100, 150]                                        # the first utterance is one whole workgroup column
    mask[:64] = 1.0                                                 # all ones
    mask[70] = 0.0                                                  # a wholly masked frame: cnt_t = 0
    for lw in ("mean", "max"):
        kw = dict(dtype=dtype, lip_weights=lw, tol=1e-3, pad=1)
        x, n_iter, tr = cabi(y, A, mask, None, 40, offs=offs, **kw)
        assert np.isfinite(x).all() and not x[70].any()             # nothing observed, nothing activated
        for u in range(3):
            a, b = offs[u], offs[u + 1]
            xu, nu, tu = cabi(y[a:b], A, mask[a:b], None, 40, **kw)
            assert np.array_equal(x[a:b], xu) and nu[0] == n_iter[u] and np.array_equal(tr[u], tu[0], equal_nan=True)
        if dtype == np.float64:
            (ref, rn, _), fig = reference(y, A, mask, 40, tol=1e-3, lip_weights=lw, utt_offsets=offs)
            close(x, ref, fig, "three masks, " + lw)
            assert n_iter.tolist() == rn.tolist()


# ---- 5. an utterance whose mask is all zero ----
def test_an_all_zero_utterance_stays_inside_itself():
    y, A, mask = (m.copy() for m in problem(25, 70, 150, seed=2))
    offs = [0, 64, 100, 150]
    mask[64:100] = 0.0
    x, n_iter, tr = cabi(y, A, mask, None, 12, offs=offs, tol=1e-3)
    (ref, rn, rtr), fig = reference(y, A, mask, 12, tol=1e-3, utt_offsets=offs)
    assert np.isnan(ref[64:100]).all()                              # L = 0: deComP's arithmetic gives NaN
    close(x, ref, fig, "zero mask in the middle")
    assert n_iter.tolist() == rn.tolist() and np.array_equal(np.isnan(tr), np.isnan(rtr)) and np.isnan(tr[1, :2]).all()
    keep = np.r_[0:64, 100:150]
    xk, nk, trk = cabi(y[keep], A, mask[keep], None, 12, offs=[0, 64, 114], tol=1e-3)
    assert np.array_equal(x[keep], xk) and n_iter[[0, 2]].tolist() == nk.tolist() and np.array_equal(tr[[0, 2]], trk)


# ---- 6. no mask, a mask of ones and the Gram sweep ----
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_null_mask_is_a_mask_of_ones(dtype):
    y, A, _ = problem(25, 129, 130)
    offs = [0, 50, 130]
    for lw in ("mean", "max"):
        kw = dict(dtype=dtype, offs=offs, tol=1e-3, lip_weights=lw, layout="bin_major")
        a = cabi(y, A, None, None, 30, **kw)
        b = cabi(y, A, np.ones_like(y), None, 30, **kw)
        assert all(np.array_equal(u, v, equal_nan=True) for u, v in zip(a, b))
    if dtype == np.float64:
        (ref, rn, _), fig = reference(y, A, None, 30, tol=1e-3, utt_offsets=offs)       # prox_restatement itself
        close(a[0], ref, fig, "null mask against the restatement")
        g, gn = gram(y, A, None, 30, tol=1e-3, offs=offs)
        close(a[0], g, fig, "null mask against evc_prox_solve")
        assert a[1].tolist() == gn.tolist() == rn.tolist()


# ---- 7. independent of the restatement: a binary mask that is the same for every frame deletes those bins ----
def test_a_constant_binary_mask_deletes_bins():
    y, A, mask = problem(40, 129, 65, seed=3)
    keep = mask[0] > 0
    const = np.tile(mask[0], (65, 1))
    assert 0 < keep.sum() < 40
    kw = dict(normalize=False, lipschitz=900.0, tol=0.0)
    for positive in (True, False):
        x, _, _ = cabi(y, A, const, None, 25, positive=positive, **kw)
        g, _ = gram(y[:, keep], A[:, keep], None, 25, positive=positive, **kw)
        fig = pmr.permutation_figure(y, A, const, 25, np.float64, alpha=1e-3, positive=positive, **kw)
        assert g.any()
        close(x, g, fig, "bins deleted, positive=%s" % positive)


# ---- 8. the weights of the bound, and an explicit lipschitz ----
def test_lip_weights_and_an_explicit_lipschitz():
    y, A, mask = problem(25, 130, 65, kind="weights")
    out = {}
    for lw in ("mean", "max"):
        (ref, _, rtr), fig = reference(y, A, mask, 20, check_every=4, lip_weights=lw)
        x, _, tr = cabi(y, A, mask, None, 20, check_every=4, lip_weights=lw)
        close(x, ref, fig, "lip_weights " + lw)
        stat_close(tr, rtr, fig, ref, A)
        L = pmr.lipschitz_of(A, mask, lip_weights=lw)
        xl, _, _ = cabi(y, A, mask, None, 20, check_every=4, lipschitz=L, lip_weights="mean" if lw == "max" else "max")
        close(xl, ref, fig, "lipschitz = the restatement's L (" + lw + ")")
        out[lw] = x
    assert not np.array_equal(out["mean"], out["max"])
    # the override is honoured without the problem's own scaling too
    kw = dict(normalize=False, lipschitz=700.0)
    (ref, _, _), fig = reference(y, A, mask, 20, **kw)
    close(cabi(y, A, mask, None, 20, **kw)[0], ref, fig, "normalize=0 with lipschitz")
    (ref, _, _), fig = reference(y, A, mask, 20, normalize=False, lip_weights="max")
    close(cabi(y, A, mask, None, 20, normalize=False, lip_weights="max")[0], ref, fig, "normalize=0 with the bound")


# ---- 9. containment ----
def test_nan_in_a_frame_stays_in_its_frame():
    y, A, mask = problem(25, 129, 130)
    offs = [0, 65, 130]
    L = pmr.lipschitz_of(A, mask[:65], lip_weights="max")
    x, n, _ = cabi(y, A, mask, None, 12, offs=offs, layout="bin_major", tol=1e-3, lip_weights="max")
    yn = y.copy()
    yn[20, 7] = np.nan
    assert mask[20, 7] > 0
    xn, nn, trn = cabi(yn, A, mask, None, 12, offs=offs, layout="bin_major", tol=1e-3, lip_weights="max")
    keep = np.arange(130) != 20
    assert np.isnan(xn[20]).all() and np.array_equal(xn[keep], x[keep])
    assert n.tolist() == nn.tolist() == [12, 12] and np.isnan(trn[0]).all() and np.isfinite(trn[1]).all()
    # a NaN weight: with a given lipschitz it stays in its frame's column ...
    xl, _, _ = cabi(y, A, mask, None, 12, offs=offs, tol=1e-3, lipschitz=L)
    mn = mask.copy()
    mn[20, 7] = np.nan
    xm, _, _ = cabi(y, A, mn, None, 12, offs=offs, tol=1e-3, lipschitz=L)
    assert np.isnan(xm[20]).all() and np.array_equal(xm[keep], xl[keep])
    # ... and through the bound it reaches its utterance's step (deComP's wbar), and no other utterance
    for lw in ("mean", "max"):
        xb, _, _ = cabi(y, A, mask, None, 12, offs=offs, tol=1e-3, lip_weights=lw)
        xw, _, _ = cabi(y, A, mn, None, 12, offs=offs, tol=1e-3, lip_weights=lw)
        assert np.isnan(xw[:65]).all() and np.array_equal(xw[65:], xb[65:])


def test_nan_in_the_dictionary_reaches_every_activation():
    y, A, mask = (m.copy() for m in problem(25, 129, 65))
    A[40, 3] = np.nan
    for kw in (dict(), dict(lipschitz=50.0), dict(normalize=False, lipschitz=900.0)):
        x, n_iter, tr = cabi(y, A, mask, None, 11, tol=1e-3, **kw)
        assert np.isnan(x).all() and n_iter.tolist() == [11] and np.isnan(tr).all()


# ---- 10. the edges of the call, the Python surface, float32, the routed size ----
@pytest.mark.parametrize("layout", ["frame_major", "bin_major"])
def test_no_iterations_return_the_start(layout):
    y, A, mask = problem(25, 33, 70)
    x0 = np.random.default_rng(3).random((70, 33))
    x, n_iter, tr = cabi(y, A, mask, x0, 0, layout=layout, pad=5)
    assert np.array_equal(x, x0) and n_iter.tolist() == [0] and tr.shape == (1, 0)
    xc, _, _ = cabi(y, A, mask, None, 0, layout=layout, pad=5, init_value=0.25)
    assert np.array_equal(xc, np.full((70, 33), 0.25))
    # a constant start is the given start of that value
    x1, _, _ = cabi(y, A, mask, None, 4, layout=layout, pad=5, init_value=0.25, lip_weights="max")
    x2, _, _ = cabi(y, A, mask, np.full((70, 33), 0.25), 4, layout=layout, pad=5, lip_weights="max")
    assert np.array_equal(x1, x2)
    ref = pmr.solve(y, A, 1e-3, np.full((70, 33), 0.25), mask=mask, iters=4, tol=0.0, lip_weights="max")[0]
    close(x1, ref, pmr.permutation_figure(y, A, mask, 4, np.float64, x0=np.full((70, 33), 0.25), alpha=1e-3, tol=0.0,
                                          lip_weights="max"), "const start")


def test_no_frames_are_accepted():
    y, A, mask = problem(25, 33, 70)
    x, n_iter, tr = cabi(y[:0], A, mask[:0], None, 20, tol=1e-3)
    assert x.shape == (0, 33) and n_iter.tolist() == [20] and np.isnan(tr).all()
    x, n_iter, tr = cabi(y[:0], A, None, None, 20, tol=1e-3)
    assert x.shape == (0, 33) and n_iter.tolist() == [20]
    x, n_iter, tr = cabi(y, A, mask, None, 20, tol=0.0, offs=[0, 0, 70, 70], lip_weights="max")
    assert n_iter.tolist() == [20, 20, 20] and np.isnan(tr[[0, 2]]).all() and np.isfinite(tr[1]).all()
    (ref, _, _), fig = reference(y, A, mask, 20, lip_weights="max")
    close(x, ref, fig, "empty utterances around a full one")


def test_convert_prox_with_a_mask_is_solve_then_synthesize():
    import torch
    rng = np.random.default_rng(5)
    y, A, mask = problem(25, 64, 40)
    B = rng.random((201, 64))
    kw = dict(alpha=1e-3, iters=60, tol=1e-3, mask=mask.T.copy())
    Y, H, info = evc().convert_prox(A.T.copy(), B, y.T.copy(), info=True, **kw)
    H2, info2 = evc().solve_activations_prox(A.T.copy(), y.T.copy(), info=True, **kw)
    assert np.array_equal(H, H2) and np.array_equal(Y, evc().synthesize(B, H2))
    (ref, rn, rtr), fig = reference(y, A, mask, 60, tol=1e-3, lip_weights="max")
    close(H.T, ref, fig, "convert_prox")
    slots = pr.n_slots(60, 10)
    assert info["kernel"] == info2["kernel"] == "k_prox_resid+k_prox_back" and info["n_iter"].tolist() == rn.tolist()
    assert info["change"].shape == (1, slots) and info["launches"] == 2 * 60 + slots
    assert np.array_equal(np.isfinite(info["change"]), np.isfinite(rtr))
    # the factored sweep without a mask, and the Gram sweep as before
    Hf, inf_f = evc().solve_activations_prox(A.T.copy(), y.T.copy(), alpha=1e-3, iters=60, tol=1e-3, factored=True, info=True)
    Hg, inf_g = evc().solve_activations_prox(A.T.copy(), y.T.copy(), alpha=1e-3, iters=60, tol=1e-3, info=True)
    assert inf_f["kernel"] == "k_prox_resid+k_prox_back" and inf_g["kernel"] == "k_prox_sweep" and inf_g["launches"] == 60 + slots
    close(Hf, Hg, pmr.permutation_figure(y, A, None, 60, np.float64, alpha=1e-3, tol=1e-3), "factored against Gram")
    # device tensors in, device tensors out; utterances; a signed solve from a given start
    x0 = rng.random((40, 64)) * 0.05
    Yt, Ht = evc().convert_prox(torch.from_numpy(A).cuda(), torch.from_numpy(B.T.copy()).cuda(), torch.from_numpy(y).cuda(),
                                torch.from_numpy(x0).cuda(), layout="frame_major", positive=False, utt_offsets=[0, 15, 40],
                                alpha=1e-3, iters=60, tol=1e-3, mask=torch.from_numpy(mask).cuda(), lip_weights="mean")
    assert isinstance(Yt, torch.Tensor) and Yt.is_cuda and tuple(Yt.shape) == (40, 201)
    ref2 = pmr.solve(y, A, 1e-3, x0, mask=mask, iters=60, tol=1e-3, positive=False, utt_offsets=[0, 15, 40])[0]
    fig2 = max(pmr.permutation_figure(y[a:b], A, mask[a:b], 60, np.float64, x0=x0[a:b], alpha=1e-3, tol=1e-3, positive=False)
               for a, b in ((0, 15), (15, 40)))
    close(Ht.cpu().numpy(), ref2, fig2, "convert_prox frame_major")


@pytest.mark.parametrize("name", FIXTURES)
def test_float32_on_the_fixtures(name):
    d = load(name)
    K = int(d["maxiter"])
    kw = dict(alpha=d["kw"]["alpha"], positive=d["positive"], momentum=d["momentum"])
    ref = pmr.solve(d["y"], d["A"], x0=d.get("x0"), mask=d["mask"], iters=K, tol=0.0, stop=False, **kw)[0]
    for layout in ("frame_major", "bin_major"):
        x, n_iter, _ = cabi(d["y"], d["A"], d["mask"], d.get("x0"), K, dtype=np.float32, layout=layout, pad=3, tol=0.0,
                            stop_rule="none", **kw)
        assert x.dtype == np.float32 and n_iter.tolist() == [K]
        close(x, ref, float(d["perm32"]), "%s %s float32" % (name, layout))


def test_routed_size():
    y, A, mask = problem(25, 4096, 128)
    (ref, _, rtr), fig = reference(y, A, mask, 3, check_every=1, lip_weights="max")
    H, info = evc().solve_activations_prox(A, y, alpha=1e-3, iters=3, tol=0.0, check_every=1, layout="frame_major", mask=mask,
                                           info=True)
    close(H, ref, fig, "N 4096 T 128")
    stat_close(info["change"], rtr, fig, ref, A)
