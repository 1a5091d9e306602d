"""evc_mu_masked_solve and evc_mu_masked_learn on the GPU against recorded deComP runs (tests/golden/mum_*.npz: K calls of
deComP's update_x with a mask; mum_learn_*.npz: its nmf.solve) and the numpy restatement (tests/mu_masked_restatement.py), which reproduces every one of them bit for bit
(tests/test_mu_masked_host.py).

Everything here is in deComP's orientation: y is T x M, D is N x M (exemplars as rows), x is T x N, mask is T x M.

The bound is the project's own: max |x - ref| <= 100 figure max |ref|.  `figure` is the fixture's `perm64` / `perm32`: how far
the restatement's result moves when the exemplars AND the bins are permuted (the factored sweep sums over both), as
tools/make_golden_mu_masked.py records it, with a floor of K eps for K updates.  Shapes without a fixture get the same recipe
computed in the test (mmr.permutation_figure).  Zeros are exact where the reference's are and NaN appears where and only where
the reference has it.  float32: against the float64 reference within 100 perm32.
Measured on an MI355X (the table of DESIGN.md §5.22), worst error of max |ref| against its bound.  float64: solve fixtures
0 .. 2.1e-15 (4.4e-13 .. 9.2e-13), run to their stops 9.6e-16 .. 1.3e-15 (1.3e-12 .. 2.9e-12), M = 528 6.7e-15 (7.0e-13), no mask
4.1e-15 (4.4e-13), against evc_beta_solve 1.0e-15 (4.4e-13), a frame without data / a NaN frame / the batch of three 9.0e-16 ..
5.1e-15 (3.5e-13 .. 2.0e-12), convert_masked 6.5e-16 (4.2e-13); learn fixtures 1.8e-15 .. 4.4e-15 (2.7e-13 .. 2.6e-12), forced
frame ranges 8.0e-16 .. 3.6e-15 (2.7e-13 .. 3.9e-13).  float32: solve 7.9e-8 .. 5.6e-6 (2.4e-4 .. 6.4e-4), M = 528 4.1e-6
(3.8e-4), learn 8.0e-7 .. 2.2e-6 (1.5e-4 .. 1.4e-3)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mu_masked_restatement as mmr  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = ["m25_n64_t32", "m40_n130_t33", "m1_n5_t3", "m201_n300_t20"]
FIXTURES = ["mum_%s_%s" % (s, l) for l in mmr.LOSSES for s in SHAPES]
BATCHES = [f for f in FIXTURES if "m25" in f or "m40" in f]
_cache = {}


def evc():
    import exemplars_vc_amd
    return exemplars_vc_amd


def load(name):
    if name not in _cache:
        d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
        d["y"], d["D"], d["mask"] = d["y"].astype(np.float64), d["D"].astype(np.float64), d["mask"].astype(np.float64)
        d["loss"], d["K"] = str(d["loss"]), int(d["K"])
        d["x0"] = d["x0"].astype(np.float64) if "x0" in d else np.ones((d["y"].shape[0], d["D"].shape[0]))
        _cache[name] = d                                          # shared: the tests copy before they change one
    return _cache[name]


def problem(M, N, T, seed=0, kind="binary"):
    """y, D, mask - computed once per shape and left unchanged"""
    key = (M, N, T, seed, kind)
    if key not in _cache:
        s = 1000 * seed + 7 * M + 3 * N + T
        _cache[key] = mmr.problem(M, N, T, s) + (mmr.problem_mask(T, M, s, kind),)
    return _cache[key]


def reference(y, D, mask, K, loss, x0=None):
    """the restatement of K updates and its permutation figure (floored at K eps), computed once per case"""
    key = ("ref", id(y), id(D), id(mask), K, loss, None if x0 is None else id(x0))
    if key not in _cache:
        _cache[key] = (mmr.solve(y, D, x0, mask=mask, loss=loss, iters=K)[0],
                       mmr.permutation_figure(y, D, mask, K, np.float64, loss, x0=x0), y, D, mask, x0)
    return _cache[key][:2]


def close(x, ref, figure, what=""):
    """max |x - ref| <= 100 figure max |ref|; zeros exact where the reference's are; NaN where and only where it has NaN"""
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert x.shape == ref.shape and np.array_equal(np.isnan(x), np.isnan(ref))
    assert (x[ref == 0] == 0).all()
    good = ~np.isnan(ref)
    top = float(np.max(np.abs(ref[good]))) if good.any() else 0.0
    diff = float(np.max(np.abs(x[good] - ref[good]))) if good.any() else 0.0
    worst = diff / top if top > 0 else diff
    print("%s: max error %.3e of max |x| (allowed %.3e)" % (what, worst, 100 * figure))
    assert worst <= 100 * figure
    return worst


def cabi(y, D, mask, x0, iters, loss, *, check_every=0, tol=0.0, stop_rule="none", layout="frame_major", dtype=np.float64, pad=0,
         mpad=None, offs=None, init_value=1.0):
    """evc_mu_masked_solve through ctypes: every matrix is laid out as `layout` says inside a buffer whose leading dimension
    is `pad` longer than needed (the mask's: `mpad`, by default pad + 2, so ldm differs from ldx) and whose padding holds
    NaN, which must still be there afterwards.  mask None: a NULL pointer.  x0 None: EVC_INIT_CONST with init_value over a
    buffer full of NaN.  -> x (T x N), n_iter, trace"""
    import torch
    from exemplars_vc_amd import _lib
    L = _lib.lib()
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    fm = layout == "frame_major"
    (N, M), T = D.shape, y.shape[0]
    mpad = pad + 2 if mpad is None else mpad

    def stage(mat, extra):
        m = np.asarray(mat, dtype=dtype)
        m = m if fm else m.T
        buf = torch.full((m.shape[0], m.shape[1] + extra), float("nan"), dtype=tdt, device="cuda")
        buf[:, :m.shape[1]] = torch.from_numpy(np.ascontiguousarray(m))
        return buf, m.shape[1]
    (A_d, _), (X_d, _) = stage(D, pad), stage(y, pad)
    M_d = None if mask is None else stage(mask, mpad)[0]
    H_d, hcols = stage(np.full((T, N), np.nan) if x0 is None else x0, pad)
    o = _lib.MuMaskedOpts()
    o.struct_bytes = C.sizeof(o)
    o.dtype, o.layout, o.iters = (_lib.F64 if dtype == np.float64 else _lib.F32), (_lib.FRAME_MAJOR if fm else _lib.BIN_MAJOR), iters
    o.loss = {"l2": _lib.LOSS_FROBENIUS, "kl": _lib.LOSS_KL}[loss]
    o.check_every, o.stop_rule = check_every, {"none": _lib.STOP_NONE, "sklearn": _lib.STOP_SKLEARN}[stop_rule]
    o.init_mode = _lib.INIT_CONST if x0 is None else _lib.INIT_GIVEN
    o.tol, o.init_value = tol, init_value
    n_utt = 1 if offs is None else len(offs) - 1
    po = None if offs is None else (C.c_int * len(offs))(*offs)
    slots = mmr.n_slots(iters, check_every)
    n_iter, trace = np.zeros(n_utt, dtype=np.int32), np.full((n_utt, slots), -1.0)
    nbytes = int(L.evc_mu_masked_workspace_bytes(M, N, T, n_utt, o.dtype))
    assert nbytes > 0
    ws = torch.empty(nbytes + 8, dtype=torch.uint8, device="cuda")
    ld = lambda t: int(t.stride(0))      # noqa: E731
    st = L.evc_mu_masked_solve(A_d.data_ptr(), ld(A_d), X_d.data_ptr(), ld(X_d), None if M_d is None else M_d.data_ptr(),
                               0 if M_d is None else ld(M_d), H_d.data_ptr(), ld(H_d), M, N, T, po, n_utt, C.byref(o),
                               ws.data_ptr() + 8, nbytes, n_iter.ctypes.data_as(C.POINTER(C.c_int)),
                               trace.ctypes.data_as(C.POINTER(C.c_double)), None)
    assert st == 0, st
    torch.cuda.synchronize()
    out = H_d.cpu().numpy()
    if pad:
        assert np.isnan(out[:, hcols:]).all()                       # the padding of H was not written
    x = out[:, :hcols]
    return np.ascontiguousarray(x if fm else x.T), n_iter, trace


# ---- the recorded deComP runs ----
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_float64(name):
    d = load(name)
    fig = max(float(d["perm64"]), d["K"] * np.finfo(np.float64).eps)
    x, n_iter, trace = cabi(d["y"], d["D"], d["mask"], d["x0"], d["K"], d["loss"])
    close(x, d["x"], fig, name)
    assert n_iter.tolist() == [d["K"]] and np.isnan(trace).all()


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_float32(name):
    d = load(name)
    fig = max(float(d["perm32"]), d["K"] * float(np.finfo(np.float32).eps))
    x, _, _ = cabi(d["y"], d["D"], d["mask"], d["x0"], d["K"], d["loss"], dtype=np.float32, layout="bin_major", pad=3)
    assert x.dtype == np.float32
    close(x, d["x"], fig, name + " float32")


@pytest.mark.parametrize("name", BATCHES)
def test_fixture_stops_as_the_restatement(name):
    """the library's own stop rule on the recorded batch: the utterances stop at different checks, n_iter is the restatement's"""
    d = load(name)
    offs, iters, ce, tol = d["offs"].tolist(), int(d["iters"]), int(d["check_every"]), float(d["tol"])
    assert len(set(d["n_iter_stop"].tolist())) > 1 and (d["n_iter_stop"] < iters).all()
    x, n_iter, trace = cabi(d["y"], d["D"], d["mask"], d["x0"], iters, d["loss"], check_every=ce, tol=tol, stop_rule="sklearn",
                            offs=offs)
    assert n_iter.tolist() == d["n_iter_stop"].tolist()
    assert np.array_equal(np.isfinite(trace), np.isfinite(d["trace_stop"]))
    K = int(d["n_iter_stop"].max())
    x_stop, ns, ts = mmr.solve(d["y"], d["D"], d["x0"], mask=d["mask"], loss=d["loss"], iters=iters, check_every=ce, tol=tol,
                               utt_offsets=offs)                      # the fixture records its counts and errors
    assert ns.tolist() == d["n_iter_stop"].tolist()
    fig = max(mmr.permutation_figure(d["y"][a:b], d["D"], d["mask"][a:b], K, np.float64, d["loss"], x0=d["x0"][a:b])
              for a, b in zip(offs[:-1], offs[1:]))
    close(x, x_stop, fig, name + " stopped")
    if d["loss"] == "l2":
        # |err - err_ref| <= ||(x - x_ref) D||_F <= sqrt(T N) max|x - x_ref| ||D||_2: twice the activations' bound, scaled
        scale = np.sqrt(x.size) * np.linalg.norm(d["D"], 2) * np.max(np.abs(x_stop))
        good = np.isfinite(trace)
        assert np.max(np.abs(trace[good] - d["trace_stop"][good])) <= 2 * 100 * fig * scale
    # each utterance alone: the same bits, the same count
    for u, (a, b) in enumerate(zip(offs[:-1], offs[1:])):
        xu, nu, tu = cabi(d["y"][a:b], d["D"], d["mask"][a:b], d["x0"][a:b], iters, d["loss"], check_every=ce, tol=tol,
                          stop_rule="sklearn")
        assert np.array_equal(xu, x[a:b]) and nu[0] == n_iter[u] and np.array_equal(tu[0], trace[u], equal_nan=True)


@pytest.mark.parametrize("loss", mmr.LOSSES)
def test_the_limit_of_528_bins(loss):
    y, D, mask = problem(528, 16, 17)
    ref, fig = reference(y, D, mask, 6, loss)
    for dtype, f in ((np.float64, fig), (np.float32, mmr.permutation_figure(y, D, mask, 6, np.float32, loss))):
        x, _, _ = cabi(y, D, mask, None, 6, loss, dtype=dtype)
        close(x, ref, f, "M = 528 %s %s" % (loss, dtype.__name__))


# ---- mask handling ----
@pytest.mark.parametrize("loss", mmr.LOSSES)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_null_mask_is_a_mask_of_ones(loss, dtype):
    y, D, _ = problem(40, 130, 33)
    a = cabi(y, D, None, None, 12, loss, dtype=dtype, check_every=4)
    b = cabi(y, D, np.ones_like(y), None, 12, loss, dtype=dtype, check_every=4)
    assert all(np.array_equal(u, v) for u, v in zip(a, b)) and np.isfinite(a[0]).all() and a[0].any()
    ref = mmr.solve(y, D, None, loss=loss, iters=12)[0]
    close(a[0], ref, mmr.permutation_figure(y, D, None, 12, dtype, loss), "no mask %s %s" % (loss, dtype.__name__))


def test_l2_with_ones_agrees_with_evc_beta_solve():
    """strictly positive data: no maximum and no zero-replacement acts, h (Num / Den) and (h Num) / Den agree to rounding"""
    y, D, _ = problem(25, 64, 32, seed=1)
    assert (y > 0).all() and (D > 0).all()
    x0 = np.ones((32, 64))
    ref, fig = reference(y, D, None, 20, "l2")
    x, _, _ = cabi(y, D, np.ones_like(y), x0, 20, "l2")
    H = evc().solve_activations_beta(D, y, x0, beta=2.0, layout="frame_major", iters=20, init="given")
    close(x, ref, fig, "mask of ones")
    close(H, ref, fig, "evc_beta_solve beta = 2")
    close(x, H, fig, "mask of ones against evc_beta_solve")


@pytest.mark.parametrize("loss", mmr.LOSSES)
def test_a_frame_without_data_gets_zero_and_disturbs_nobody(loss):
    y, D, mask = problem(25, 64, 32, kind="weights")
    dead = mask.copy()
    dead[5] = 0.0
    x, _, _ = cabi(y, D, dead, None, 10, loss)
    assert (x[5] == 0).all() and np.isfinite(x).all()
    keep = np.arange(32) != 5
    rest, _, _ = cabi(y[keep], D, mask[keep], None, 10, loss)
    assert np.array_equal(x[keep], rest)
    close(x, mmr.solve(y, D, None, mask=dead, loss=loss, iters=10)[0], mmr.permutation_figure(y, D, dead, 10, np.float64, loss),
          "a frame without data " + loss)


@pytest.mark.parametrize("loss", mmr.LOSSES)
def test_a_nan_stays_in_its_frame(loss):
    y, D, mask = problem(25, 64, 32)
    bad = y.copy()
    bad[7, 3] = np.nan
    m = mask.copy()
    m[7, 3] = 1.0
    x, _, _ = cabi(bad, D, m, None, 8, loss)
    good, _, _ = cabi(y, D, m, None, 8, loss)
    keep = np.arange(32) != 7
    assert np.isnan(x[7]).all() and np.array_equal(x[keep], good[keep]) and np.isfinite(good).all()
    close(x, mmr.solve(bad, D, None, mask=m, loss=loss, iters=8)[0], mmr.permutation_figure(y, D, m, 8, np.float64, loss),
          "NaN frame " + loss)


# ---- batches and layouts ----
@pytest.mark.parametrize("loss", mmr.LOSSES)
def test_batch_of_three_is_the_per_utterance_calls(loss):
    y, D, mask = problem(25, 64, 34, kind="weights")
    offs = [0, 16, 33, 34]
    x0 = np.random.default_rng(3).random((34, 64)) + 0.1
    iters, ce, tol = 120, 2, {"l2": 1e-4, "kl": 3e-4}[loss]       # the three utterances stop at three different checks
    rx, rn, rt = mmr.solve(y, D, x0, mask=mask, loss=loss, iters=iters, check_every=ce, tol=tol, utt_offsets=offs)
    assert mmr.stop_margin(rt, tol) >= 1e-6 * tol and len(set(rn.tolist())) > 1
    x, n_iter, trace = cabi(y, D, mask, x0, iters, loss, check_every=ce, tol=tol, stop_rule="sklearn", offs=offs)
    assert n_iter.tolist() == rn.tolist()
    for u, (a, b) in enumerate(zip(offs[:-1], offs[1:])):
        xu, nu, tu = cabi(y[a:b], D, mask[a:b], x0[a:b], iters, loss, check_every=ce, tol=tol, stop_rule="sklearn")
        assert np.array_equal(xu, x[a:b]) and nu[0] == n_iter[u] and np.array_equal(tu[0], trace[u], equal_nan=True)
    fig = max(mmr.permutation_figure(y[a:b], D, mask[a:b], int(rn.max()), np.float64, loss, x0=x0[a:b])
              for a, b in zip(offs[:-1], offs[1:]))
    close(x, rx, fig, "batch of three " + loss)
    # an empty utterance in the middle: nothing happens to it
    x2, n2, t2 = cabi(y, D, mask, x0, 6, loss, check_every=2, offs=[0, 16, 16, 34])
    assert n2.tolist() == [6, 6, 6] and np.isnan(t2[1]).all() and np.isfinite(t2[0]).all() and np.isfinite(x2).all()


@pytest.mark.parametrize("loss", mmr.LOSSES)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_layouts_leading_dimensions_and_repeats(loss, dtype):
    y, D, mask = problem(40, 130, 33, kind="weights")
    base = cabi(y, D, mask, None, 9, loss, dtype=dtype, check_every=3)
    again = cabi(y, D, mask, None, 9, loss, dtype=dtype, check_every=3)
    assert all(np.array_equal(u, v) for u, v in zip(base, again))                     # the same call, the same bits
    for layout, pad, mpad in (("frame_major", 5, 0), ("bin_major", 0, 1), ("bin_major", 7, None)):
        other = cabi(y, D, mask, None, 9, loss, dtype=dtype, check_every=3, layout=layout, pad=pad, mpad=mpad)
        assert all(np.array_equal(u, v) for u, v in zip(base, other)), (layout, pad)  # addressing changes no arithmetic
    given = cabi(y, D, mask, np.ones((33, 130)), 9, loss, dtype=dtype, check_every=3)
    assert all(np.array_equal(u, v) for u, v in zip(base, given))                     # EVC_INIT_CONST 1 is a start of ones
    ref = mmr.solve(y, D, None, mask=mask, loss=loss, iters=9, check_every=3)
    close(base[0], ref[0], mmr.permutation_figure(y, D, mask, 9, dtype, loss), "layouts %s %s" % (loss, dtype.__name__))
    assert base[1].tolist() == [9] and np.isfinite(base[2]).all() and base[2].shape == (1, 4)
    np.testing.assert_allclose(base[2], ref[2], rtol=1e-4 if dtype == np.float32 else 1e-10)


def test_iters_zero_and_no_frames():
    y, D, mask = problem(25, 64, 32)
    x0 = np.random.default_rng(1).random((32, 64))
    x, n_iter, _ = cabi(y, D, mask, x0, 0, "l2")
    assert np.array_equal(x, x0) and n_iter.tolist() == [0]
    x, n_iter, _ = cabi(y[:0], D, mask[:0], x0[:0], 5, "kl")
    assert x.shape == (0, 64) and n_iter.tolist() == [5]


# ---- the Python wrappers ----
@pytest.mark.parametrize("loss", ["frobenius", "kl"])
def test_convert_masked_imputes_with_the_same_activations(loss):
    import torch
    y, D, mask = problem(25, 64, 32)
    short = {"frobenius": "l2", "kl": "kl"}[loss]
    ref, fig = reference(y, D, mask, 15, short)
    H, info = evc().solve_activations_masked(D, y, mask, loss=loss, iters=15, layout="frame_major", info=True)
    close(H, ref, fig, "solve_activations_masked " + loss)
    assert info["kernel"] == "k_mum_sweep" and info["n_iter"].tolist() == [15] and info["launches"] == 15
    Y, H2 = evc().convert_masked(D, D, y, mask, loss=loss, iters=15, layout="frame_major")
    assert np.array_equal(H, H2)
    close(Y, H @ D, fig, "convert_masked " + loss)
    # bin-major (the default), device tensors in -> device tensors out
    Hb, inf = evc().solve_activations_masked(torch.from_numpy(D.T.copy()).cuda(), torch.from_numpy(y.T.copy()).cuda(),
                                             torch.from_numpy(mask.T.copy()).cuda(), loss=loss, iters=15, check_every=5,
                                             info=True)
    assert isinstance(Hb, torch.Tensor) and np.array_equal(Hb.cpu().numpy().T, H) and inf["err"].shape == (1, 4)


# ---- evc_mu_masked_learn against deComP's nmf.solve (tests/golden/mum_learn_*.npz) ----
LEARN_FIXTURES = ["mum_learn_m25_r8_t48_l2", "mum_learn_m40_r19_t33_kl", "mum_learn_m201_r12_t40_kl_k12"]


def load_learn(name):
    if name not in _cache:
        d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
        for k in ("y", "D0", "mask"):
            d[k] = d[k].astype(np.float64)
        d["loss"], d["K"], d["tol"], d["maxiter"] = str(d["loss"]), int(d["n_iter"]), float(d["tol"]), int(d["maxiter"])
        d["x0"] = d["x0"].astype(np.float64) if "x0" in d else np.ones((d["y"].shape[0], d["D0"].shape[0]))
        _cache[name] = d
    return _cache[name]


def cabi_learn(y, D0, mask, x0, iters, loss, *, tol=0.0, check_every=1, layout="frame_major", dtype=np.float64, pad=0, splits=0):
    """evc_mu_masked_learn through ctypes, staged like cabi: -> D (R x M), x (T x R), n_iter, stats"""
    import torch
    from exemplars_vc_amd import _lib
    L = _lib.lib()
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    fm = layout == "frame_major"
    (R, M), T = D0.shape, y.shape[0]

    def stage(mat, extra):
        m = np.asarray(mat, dtype=dtype)
        m = m if fm else m.T
        buf = torch.full((m.shape[0], m.shape[1] + extra), float("nan"), dtype=tdt, device="cuda")
        buf[:, :m.shape[1]] = torch.from_numpy(np.ascontiguousarray(m))
        return buf, m.shape[1]
    (X_d, _), (W_d, wcols), (H_d, hcols) = stage(y, pad), stage(D0, pad), stage(x0, pad)
    M_d = None if mask is None else stage(mask, pad + 2)[0]
    o = _lib.MuMaskedLearnOpts()
    o.struct_bytes = C.sizeof(o)
    o.dtype, o.layout = (_lib.F64 if dtype == np.float64 else _lib.F32), (_lib.FRAME_MAJOR if fm else _lib.BIN_MAJOR)
    o.loss, o.iters, o.check_every, o.tol = {"l2": _lib.LOSS_FROBENIUS, "kl": _lib.LOSS_KL}[loss], iters, check_every, tol
    o.reserved = splits << 8
    n_iter, stats = C.c_int(-1), np.full(mmr.n_slots(iters, check_every), -1.0)
    nbytes = int(L.evc_mu_masked_learn_workspace_bytes(M, R, T, o.dtype))
    assert nbytes > 0
    ws = torch.empty(nbytes + 8, dtype=torch.uint8, device="cuda")
    ld = lambda t: int(t.stride(0))      # noqa: E731
    st = L.evc_mu_masked_learn(X_d.data_ptr(), ld(X_d), None if M_d is None else M_d.data_ptr(), 0 if M_d is None else ld(M_d),
                               W_d.data_ptr(), ld(W_d), H_d.data_ptr(), ld(H_d), M, R, T, C.byref(o), ws.data_ptr() + 8, nbytes,
                               C.byref(n_iter), stats.ctypes.data_as(C.POINTER(C.c_double)), None)
    assert st == 0, st
    torch.cuda.synchronize()
    W, H = W_d.cpu().numpy(), H_d.cpu().numpy()
    if pad:
        assert np.isnan(W[:, wcols:]).all() and np.isnan(H[:, hcols:]).all()
    W, H = W[:, :wcols], H[:, :hcols]
    return (np.ascontiguousarray(W if fm else W.T), np.ascontiguousarray(H if fm else H.T), int(n_iter.value), stats)


@pytest.mark.parametrize("name", LEARN_FIXTURES)
def test_learn_fixture(name):
    d = load_learn(name)
    fig = max(float(d["perm64"]), d["K"] * np.finfo(np.float64).eps)
    D, x, n_iter, stats = cabi_learn(d["y"], d["D0"], d["mask"], d["x0"], d["maxiter"] - 1, d["loss"], tol=d["tol"])
    assert n_iter == d["K"]                                            # and deComP's `it`: the stop, else maxiter
    stopped = d["tol"] > 0 and stats[n_iter] < d["tol"]
    assert (n_iter if stopped else d["maxiter"]) == int(d["it"])
    close(D, d["D"], fig, name + " D")
    close(x, d["x"], fig, name + " x")
    assert np.isnan(stats[0]) and np.isfinite(stats[1:n_iter + 1]).all() and np.isnan(stats[n_iter + 1:]).all()
    # the statistic is a difference of two dictionaries: twice the bound
    assert np.max(np.abs(stats[1:n_iter + 1] - d["stats"])) <= 2 * 100 * fig * np.max(d["D"])
    np.testing.assert_allclose(np.linalg.norm(D, axis=1), 1.0, rtol=0, atol=D.shape[1] * np.finfo(np.float64).eps)


@pytest.mark.parametrize("name", ["mum_learn_m25_r8_t48_l2", "mum_learn_m201_r12_t40_kl_k12"])
def test_learn_fixture_float32(name):
    d = load_learn(name)
    fig = max(float(d["perm32"]), d["K"] * float(np.finfo(np.float32).eps))
    D, x, n_iter, _ = cabi_learn(d["y"], d["D0"], d["mask"], d["x0"], d["K"], d["loss"], dtype=np.float32, layout="bin_major", pad=3)
    assert n_iter == d["K"] and D.dtype == np.float32
    close(D, d["D"], fig, name + " D float32")
    close(x, d["x"], fig, name + " x float32")
    np.testing.assert_allclose(np.linalg.norm(D.astype(np.float64), axis=1), 1.0, rtol=0, atol=D.shape[1] * np.finfo(np.float32).eps)


@pytest.mark.parametrize("loss", mmr.LOSSES)
def test_learn_frame_ranges_and_repeats(loss):
    M, R, T = 40, 19, 330
    y, _, mask = problem(M, R, T, kind="weights")
    rng = np.random.default_rng(11)
    D0, x0 = rng.random((R, M)) + 0.05, rng.random((T, R)) + 0.1
    _, Dr, xr, sr = mmr.learn(y, D0, x0, mask=mask, loss=loss, tol=0.0, maxiter=7)
    fig = mmr.learn_permutation_figure(y, D0, mask, 6, np.float64, loss, x0=x0)
    for S in (0, 1, 3, 7):
        a = cabi_learn(y, D0, mask, x0, 6, loss, splits=S)
        again = cabi_learn(y, D0, mask, x0, 6, loss, splits=S)
        assert all(np.array_equal(u, v, equal_nan=True) for u, v in zip(a, again)), S  # the same call, the same bits
        b = cabi_learn(y, D0, mask, x0, 6, loss, splits=S, layout="bin_major", pad=5)
        assert all(np.array_equal(u, v, equal_nan=True) for u, v in zip(a, b)), S      # addressing changes no arithmetic
        close(a[0], Dr, fig, "S = %d D %s" % (S, loss))
        close(a[1], xr, fig, "S = %d x %s" % (S, loss))
        assert a[2] == 6 and np.max(np.abs(a[3][1:] - sr)) <= 2 * 100 * fig * np.max(Dr)
    # no mask: deComP's unmasked nmf.solve; bitwise the mask of ones
    a, b = cabi_learn(y, D0, None, x0, 4, loss), cabi_learn(y, D0, np.ones_like(y), x0, 4, loss)
    assert all(np.array_equal(u, v, equal_nan=True) for u, v in zip(a, b))
    _, Dn, xn, _ = mmr.learn(y, D0, x0, loss=loss, tol=0.0, maxiter=5)
    close(a[0], Dn, fig, "no mask D " + loss)
    close(a[1], xn, fig, "no mask x " + loss)


@pytest.mark.parametrize("loss", mmr.LOSSES)
def test_learn_one_iteration_is_the_solve_on_the_normalised_start(loss):
    d = load_learn("mum_learn_m40_r19_t33_kl")
    Dn, x_same, n0, _ = cabi_learn(d["y"], d["D0"], d["mask"], d["x0"], 0, loss)       # iters = 0: the start, normalised
    assert n0 == 0 and np.array_equal(x_same, d["x0"])
    np.testing.assert_allclose(Dn, mmr.l2_strict(d["D0"]), rtol=4 * np.finfo(np.float64).eps)
    _, x1, n1, _ = cabi_learn(d["y"], d["D0"], d["mask"], d["x0"], 1, loss)
    xs, _, _ = cabi(d["y"], Dn, d["mask"], d["x0"], 1, loss)
    assert n1 == 1 and np.array_equal(x1, xs)


@pytest.mark.parametrize("name", ["mum_learn_m25_r8_t48_l2", "mum_learn_m201_r12_t40_kl_k12"])
def test_compat_nmf_solve(name):
    from exemplars_vc_amd.compat import decomp
    d = load_learn(name)
    fig = max(float(d["perm64"]), d["K"] * np.finfo(np.float64).eps)
    x0 = None if np.array_equal(d["x0"], np.ones_like(d["x0"])) else d["x0"]
    it, D, x = decomp.nmf.solve(d["y"], d["D0"], x0, tol=d["tol"], maxiter=d["maxiter"], likelihood=d["loss"], mask=d["mask"])
    assert it == int(d["it"])
    close(D, d["D"], fig, name + " compat D")
    close(x, d["x"], fig, name + " compat x")
    # the native wrapper, bin-major, device tensors
    import torch
    W, H, info = evc().learn_dictionary_masked(torch.from_numpy(d["y"].T.copy()).cuda(), torch.from_numpy(d["D0"].T.copy()).cuda(),
                                               torch.from_numpy(d["x0"].T.copy()).cuda(), torch.from_numpy(d["mask"].T.copy()).cuda(),
                                               loss={"l2": "frobenius", "kl": "kl"}[d["loss"]], layout="bin_major",
                                               iters=d["maxiter"] - 1, tol=d["tol"], info=True)
    assert isinstance(W, torch.Tensor) and info["n_iter"] == d["K"] and info["stopped"] == (int(d["it"]) < d["maxiter"])
    assert np.array_equal(W.cpu().numpy().T, D) and np.array_equal(H.cpu().numpy().T, x) and info["splits"] == 1
