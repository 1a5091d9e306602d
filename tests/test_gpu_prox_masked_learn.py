"""evc_prox_masked_learn on the GPU against recorded deComP runs (tests/golden/proxml_*.npz) and the numpy restatement
(tests/prox_masked_learn_restatement.py), which reproduces every one of them to rounding (tests/test_prox_masked_learn_host.py).

Everything here is in deComP's orientation: y and mask are T x M, D is N x M (atoms as rows), x is T x N.

float64 bound: tests/test_gpu_prox_learn.py's.  A GPU sum runs in another order than numpy's, so parity is not bitwise.
tools/make_golden_prox_masked_learn.py reruns the restatement with the ATOMS AND THE BINS permuted, the mask along with them -
another summation order of the lasso's contractions, the norms, G and a_k, the same algorithm - and records how far D moves
(absolute: atoms have norm <= 1) and x moves relative to max |x| (`perm64`).  Each fixture's bound is 100 times its own
figure, with a floor of eps steps (lasso_iters + 1) under the figure (M = 1 has nothing to permute).  Shapes without a fixture
get the same figure from the same recipe, computed in the test.  `it`, the step count and the trace are compared, and every
activation the reference's threshold cuts by more than 1e-6 thr is exactly 0.0.
float32 bound: the same scheme on the restatement's own float32 run (`perm32`), against the float64 restatement at fixed step
counts - the stop steps of float32 runs are not compared.
The measured errors are printed by every test; DESIGN.md §5.20 holds the table."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prox_masked_learn_restatement as pmlr  # noqa: E402
import prox_restatement as pr  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ["proxml_m5_n3_t101_fista", "proxml_m25_n40_t130_fista_pos_k4", "proxml_m12_n10_t64_ista_pos", "proxml_m1_n5_t12_k4",
            "proxml_m201_n48_t100_k3", "proxml_m25_n40_t130_weights_k3", "proxml_m12_n10_t64_holes_k3",
            "proxml_m8_n6_t40_unused_atom_k3", "proxml_m12_n10_t64_ones_k3"]
FIXED = [n for n in FIXTURES if n.endswith(("_k4", "_k3"))]          # tol = 0: fixed step counts
EPS = {np.float64: float(np.finfo(np.float64).eps), np.float32: float(np.finfo(np.float32).eps)}
LASSO_ITERS = 10
_cache = {}


def load(name):
    if name not in _cache:
        d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
        d["y"], d["D0"], d["mask"] = d["y"].astype(np.float64), d["D0"].astype(np.float64), d["mask"].astype(np.float64)
        d["positive"], d["momentum"] = pr.split_method(str(d["method"]))
        d["epochs"] = int(d["maxiter"]) - 1
        d["order"] = pmlr.decomp_order(d["y"].shape[0], d["epochs"], int(d["seed"]))
        d["kw"] = dict(alpha=float(d["alpha"]), batch_size=int(d["bs"]), epochs=d["epochs"], tol=float(d["tol"]),
                       positive=d["positive"], momentum=d["momentum"], order=d["order"])
        _cache[name] = d                                          # shared: the tests copy before they change one
    return _cache[name]


def floor(steps, dtype=np.float64):
    return EPS[dtype] * max(steps, 1) * (LASSO_ITERS + 1)


def moved(D, x, Dr, xr):
    """the figure of the bounds: max |D - D_ref| (absolute) and max |x - x_ref| / max |x_ref|, the larger"""
    D, x, Dr, xr = (np.asarray(a, dtype=np.float64) for a in (D, x, Dr, xr))
    top = float(np.max(np.abs(xr)))
    return max(float(np.max(np.abs(D - Dr))), float(np.max(np.abs(x - xr))) / (top if top > 0 else 1.0))


def problem(M, N, T, seed=0, kind="binary"):
    """y, D0 and a mask whose frame 3 has no valid bin"""
    key = ("p", M, N, T, seed, kind)
    if key not in _cache:
        s = 1000 * seed + 7 * M + 3 * N + T
        y, D0 = pmlr.problem(M, N, T, s)
        mask = np.ones((T, M)) if kind == "ones" else pmlr.problem_mask(T, M, s, kind=kind)
        if kind != "ones":
            mask[3] = 0.0
        _cache[key] = y, D0, mask
    return _cache[key]


def _key(kw):
    return tuple(sorted((k, v if not isinstance(v, np.ndarray) else v.tobytes()) for k, v in kw.items()))


def reference(M, N, T, seed=0, kind="binary", **kw):
    """the float64 restatement on problem(...), and its cuts"""
    key = ("ref", M, N, T, seed, kind, _key(kw))
    if key not in _cache:
        y, D0, mask = problem(M, N, T, seed, kind)
        cuts = {}
        _cache[key] = pmlr.solve(y, D0, mask=mask, cuts=cuts, **dict(dict(alpha=1e-3, tol=0.0), **kw)), cuts
    return _cache[key]


def figure(M, N, T, dtype=np.float64, seed=0, kind="binary", **kw):
    """tools/make_golden_prox_masked_learn.py's figure for reference(...)'s run: how far the restatement's result moves when
    the atoms and the bins (the mask's with them) are summed in another order - and at least the floor"""
    key = ("fig", M, N, T, dtype, seed, kind, _key(kw))
    if key not in _cache:
        y, D0, mask = problem(M, N, T, seed, kind)
        kw = dict(dict(alpha=1e-3, tol=0.0), **kw)
        x0 = kw.pop("x0", None)
        rng = np.random.default_rng(5)
        pn, pm = rng.permutation(N), rng.permutation(M)
        base = reference(M, N, T, seed, kind, **dict(kw, **({} if x0 is None else dict(x0=x0))))[0] if dtype == np.float64 \
            else pmlr.solve(y, D0, x0=x0, mask=mask, dtype=dtype, **kw)
        other = pmlr.solve(y[:, pm], D0[pn][:, pm], x0=None if x0 is None else x0[:, pn], mask=mask[:, pm], dtype=dtype, **kw)
        Db, xb = np.empty_like(other[0]), np.empty_like(other[1])
        Db[np.ix_(pn, pm)] = other[0]
        xb[:, pn] = other[1]
        _cache[key] = max(moved(Db, xb, base[0], base[1]), floor(base[3], dtype))
    return _cache[key]


def close(D, x, Dr, xr, figure, what=""):
    worst = moved(D, x, Dr, xr)
    print("%s: max error %.3e (allowed %.3e)" % (what, worst, 100 * figure))
    assert worst <= 100 * figure
    return worst


def zeros_where_cut(x, cuts, some=False):
    """every activation the reference cuts by more than 1e-6 thr is exactly 0.0 (some: and there are such)"""
    cut = cuts["pre"] < -1e-6 * cuts["thr"]
    assert (cut.any() or not some) and np.all(np.asarray(x)[cut] == 0.0)


def cabi(y, D0, mask, x0=None, *, alpha=1e-3, batch_size, epochs, tol=0.0, positive=True, momentum="fista", order=None,
         layout="frame_major", dtype=np.float64, pad=0, state=None, lasso_iters=LASSO_ITERS, lasso_tol=1e-5, want_trace=True):
    """evc_prox_masked_learn through ctypes: every matrix is laid out as `layout` says inside a buffer whose leading dimension
    is `pad` longer than needed and whose padding holds NaN, which must still be there afterwards.
    -> D (N x M), x (T x N), n_epochs, n_steps, trace, state = (stats_s [M * N rows] and stats_q with their padding, count)"""
    import torch
    from exemplars_vc_amd import _lib
    L = _lib.lib()
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    fm = layout == "frame_major"
    (N, M), T = D0.shape, y.shape[0]

    def stage(mat):
        m = np.asarray(mat, dtype=dtype)
        m = m if fm else m.T
        buf = torch.full((m.shape[0], m.shape[1] + pad), float("nan"), dtype=tdt, device="cuda")
        buf[:, :m.shape[1]] = torch.from_numpy(np.ascontiguousarray(m))
        return buf, m.shape[1]
    (D_d, dcols), (X_d, _), (W_d, wcols) = stage(D0), stage(y), stage(mask)
    H_d, hcols = stage(np.ones((T, N)) if x0 is None else x0)
    if state is None:
        S_d = torch.full((M * N, N + pad), float("nan"), dtype=tdt, device="cuda")
        Q_d, count = torch.full((N, M + pad), float("nan"), dtype=tdt, device="cuda"), C.c_longlong(-7)
    else:
        S_d, Q_d, count = state[0].clone(), state[1].clone(), C.c_longlong(state[2])
    o = _lib.ProxMaskedLearnOpts()
    o.struct_bytes = C.sizeof(o)
    o.dtype, o.layout = (_lib.F64 if dtype == np.float64 else _lib.F32), (_lib.FRAME_MAJOR if fm else _lib.BIN_MAJOR)
    o.batch_size, o.epochs, o.lasso_iters, o.lasso_check_every = batch_size, epochs, lasso_iters, 10
    o.mode = _lib.PROX_POSITIVE if positive else _lib.PROX_SIGNED
    o.momentum = {"ista": _lib.PROX_ISTA, "fista": _lib.PROX_FISTA, "nesterov": _lib.PROX_NESTEROV}[momentum]
    o.resume = 0 if state is None else 1
    o.alpha, o.tol, o.lasso_tol = alpha, tol, lasso_tol
    nbytes = int(L.evc_prox_masked_learn_workspace_bytes(M, N, T, batch_size, o.dtype))
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    n_ep, n_st = C.c_int(-1), C.c_int(-1)
    trace = np.full(epochs * (T // batch_size), -5.0)
    order_p = None
    if order is not None:
        order = np.ascontiguousarray(order, dtype=np.int32)
        order_p = order.ctypes.data_as(C.POINTER(C.c_int))
    st = L.evc_prox_masked_learn(X_d.data_ptr(), X_d.stride(0), W_d.data_ptr(), W_d.stride(0), D_d.data_ptr(), D_d.stride(0),
                                 H_d.data_ptr(), H_d.stride(0), S_d.data_ptr(), S_d.stride(0), Q_d.data_ptr(), Q_d.stride(0),
                                 C.byref(count), order_p, M, N, T, C.byref(o), ws.data_ptr(), nbytes, C.byref(n_ep), C.byref(n_st),
                                 trace.ctypes.data_as(C.POINTER(C.c_double)) if want_trace else None, None)
    torch.cuda.synchronize()
    assert st == 0, st
    for buf, cols in ((D_d, dcols), (H_d, hcols), (W_d, wcols), (S_d, N), (Q_d, M)):
        assert bool(torch.isnan(buf[:, cols:]).all())             # the padding is never written
    unstage = lambda buf, cols: (buf[:, :cols].cpu().numpy() if fm else buf[:, :cols].cpu().numpy().T)
    return unstage(D_d, dcols), unstage(H_d, hcols), n_ep.value, n_st.value, trace, (S_d, Q_d, int(count.value))


def planes(state, M, N):
    """the statistics as numpy: S [M][N][N], Q [N][M]"""
    return state[0][:, :N].cpu().numpy().reshape(M, N, N), state[1][:, :M].cpu().numpy()


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_cabi(name):
    d = load(name)
    D, x, n_ep, n_st, tr, state = cabi(d["y"], d["D0"], d["mask"], d.get("x0"), **d["kw"])
    steps = int(d["n_steps"])
    fig = max(float(d["perm64"]), floor(steps))
    close(D, x, d["D"], d["x"], fig, name)
    assert n_st == steps and state[2] == steps
    stopped = float(d["tol"]) > 0
    assert n_ep == (int(d["it"]) if stopped else d["epochs"])
    np.testing.assert_allclose(tr[:steps], d["trace"], rtol=0, atol=2 * 100 * fig)
    assert np.all(np.isnan(tr[steps:]))
    cuts = {}
    pmlr.solve(d["y"], d["D0"], x0=d.get("x0"), mask=d["mask"], cuts=cuts, **d["kw"])
    if d["positive"]:
        zeros_where_cut(x, cuts, some=name.endswith("_k4"))


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_python(name):
    import exemplars_vc_amd as evc
    d = load(name)
    kw = dict(d["kw"])
    kw.pop("order")
    D, x, info = evc.learn_dictionary_sparse(d["y"], d["D0"], d.get("x0"), layout="frame_major", mask=d["mask"],
                                             seed=int(d["seed"]), info=True, **kw)
    steps = int(d["n_steps"])
    assert D.dtype == np.float64 and D.shape == d["D"].shape and info["n_steps"] == steps and not info.get("block")
    assert info["n_epochs"] == (int(d["it"]) if float(d["tol"]) > 0 else d["epochs"])
    fig = max(float(d["perm64"]), floor(steps))
    close(D, x, d["D"], d["x"], fig, name)
    np.testing.assert_allclose(info["change"][:steps], d["trace"], rtol=0, atol=2 * 100 * fig)
    stats_s, stats_q, count = info["state"]
    M, N = d["y"].shape[1], d["D0"].shape[0]
    assert tuple(stats_s.shape) == (M, N, N) and tuple(stats_q.shape) == (N, M) and count == steps


@pytest.mark.parametrize("name", FIXED)
def test_fixture_float32(name):
    d = load(name)
    D, x, n_ep, n_st, _, _ = cabi(d["y"], d["D0"], d["mask"], d.get("x0"), dtype=np.float32, **d["kw"])
    assert D.dtype == np.float32 and n_st == int(d["n_steps"]) and n_ep == d["epochs"]
    close(D, x, d["D"], d["x"], max(float(d["perm32"]), floor(n_st, np.float32)), name)


GEOMETRY = [(M, N) for N in (1, 63, 64, 65, 130) for M in (1, 25, 201)]


@pytest.mark.parametrize("M,N", GEOMETRY)
def test_stats_geometry(M, N):
    """two steps, two frames left alone, at every tile geometry of k_pmlearn_stats: one atom, a panel short of, at and past
    64 rows, three panels with a short last one; one bin, one workgroup of bins per thread and nearly a whole one"""
    T, bs = 50, 24
    kw = dict(batch_size=bs, epochs=1)
    (Dr, xr, _, steps, trr, _), cuts = reference(M, N, T, **kw)
    fig = figure(M, N, T, **kw)
    y, D0, mask = problem(M, N, T)
    D, x, n_ep, n_st, tr, state = cabi(y, D0, mask, **kw)
    assert (n_ep, n_st, steps) == (1, 2, 2)
    close(D, x, Dr, xr, fig, "M=%d N=%d" % (M, N))
    np.testing.assert_allclose(tr, trr, rtol=0, atol=2 * 100 * fig)
    assert np.array_equal(x[48:], np.ones((2, N)))
    zeros_where_cut(x, cuts)


@pytest.mark.parametrize("bs", [1, 15, 16, 17, 33, 70])
def test_batch_sizes_and_skipped_frames(bs):
    """one frame, a slab short of, at and past 16 frames, three slabs with a short last one, the whole call in one batch"""
    M, N, T = 25, 40, 70
    y, D0, mask = problem(M, N, T, kind="weights")
    rng = np.random.default_rng(11)
    order = rng.permutation(T).astype(np.int32)[None]
    if bs == 1:                 # every batch needs a valid bin: L = 0 is test_restatement_options' and the NaN test's
        mask = mask.copy()
        mask[3] = 1.0
    x0 = rng.random((T, N)) * 0.05
    kw = dict(batch_size=bs, epochs=1, order=order)
    Dr, xr, _, steps, _, _ = pmlr.solve(y, D0, 1e-3, x0, mask=mask, **kw)
    D, x, _, n_st, _, _ = cabi(y, D0, mask, x0, **kw)
    assert n_st == steps == T // bs
    rng = np.random.default_rng(5)
    pn, pm = rng.permutation(N), rng.permutation(M)
    other = pmlr.solve(y[:, pm], D0[pn][:, pm], 1e-3, x0[:, pn], mask=mask[:, pm], **kw)
    Db, xb = np.empty_like(other[0]), np.empty_like(other[1])
    Db[np.ix_(pn, pm)] = other[0]
    xb[:, pn] = other[1]
    close(D, x, Dr, xr, max(moved(Db, xb, Dr, xr), floor(steps)), "bs=%d" % bs)
    never = order[0, (T // bs) * bs:]
    assert never.size == T % bs and np.array_equal(x[never], x0[never])      # bitwise: no step took these frames


@pytest.mark.parametrize("layout", ["frame_major", "bin_major"])
@pytest.mark.parametrize("bs", [31, 32, 33])
def test_float32_slab_boundary(bs, layout):
    """float32 stages slabs of 32 frames (float64: 16): a batch short of, at and past one slab, in both staging orders"""
    M, N, T = 25, 40, 70
    kw = dict(batch_size=bs, epochs=1)
    (Dr, xr, _, steps, _, _), _ = reference(M, N, T, **kw)
    y, D0, mask = problem(M, N, T)
    D, x, _, n_st, _, _ = cabi(y, D0, mask, dtype=np.float32, layout=layout, **kw)
    assert n_st == steps == 2
    close(D, x, Dr, xr, figure(M, N, T, np.float32, **kw), "float32 bs=%d %s" % (bs, layout))
    assert np.array_equal(x[2 * bs:], np.ones((T - 2 * bs, N), dtype=np.float32))


@pytest.mark.parametrize("layout", ["frame_major", "bin_major"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_layouts_with_padding(layout, dtype):
    M, N, T = 25, 33, 50
    kw = dict(batch_size=24, epochs=1)
    (Dr, xr, _, _, _, _), _ = reference(M, N, T, **kw)
    y, D0, mask = problem(M, N, T)
    D, x, _, _, _, _ = cabi(y, D0, mask, layout=layout, dtype=dtype, pad=3, **kw)
    close(D, x, Dr, xr, figure(M, N, T, dtype, **kw), "%s %s" % (layout, dtype.__name__))


def same_bits(a, b):
    import torch
    for u, v in zip(a[:2], b[:2]):
        assert np.array_equal(u, v, equal_nan=True)
    assert a[2:4] == b[2:4] and a[5][2] == b[5][2]
    for i in (0, 1):
        assert bool(torch.equal(torch.nan_to_num(a[5][i], nan=-1.0), torch.nan_to_num(b[5][i], nan=-1.0)))


def test_null_order_is_the_identity_and_repeatable():
    M, N, T = 25, 40, 70
    y, D0, mask = problem(M, N, T)
    kw = dict(batch_size=32, epochs=2)
    a = cabi(y, D0, mask, **kw)
    same_bits(a, cabi(y, D0, mask, order=np.tile(np.arange(T, dtype=np.int32), (2, 1)), **kw))
    b = cabi(y, D0, mask, **kw)
    same_bits(a, b)
    assert np.array_equal(a[4], b[4])


def test_resume_two_plus_one_is_three():
    M, N, T = 25, 40, 70
    y, D0, mask = problem(M, N, T)
    order = np.stack([np.random.default_rng(3 + e).permutation(T) for e in range(3)]).astype(np.int32)
    whole = cabi(y, D0, mask, batch_size=32, epochs=3, order=order)
    first = cabi(y, D0, mask, batch_size=32, epochs=2, order=order[:2])
    assert first[5][2] == 4
    second = cabi(y, first[0], mask, first[1], batch_size=32, epochs=1, order=order[2:], state=first[5])
    assert second[5][2] == 6 and whole[5][2] == 6
    same_bits((second[0], second[1], 0, 0, None, second[5]), (whole[0], whole[1], 0, 0, None, whole[5]))
    assert np.array_equal(np.concatenate([first[4], second[4]]), whole[4])


def test_no_trace_no_tol_is_an_enqueue_with_the_same_bits():
    M, N, T = 25, 40, 70
    y, D0, mask = problem(M, N, T)
    a = cabi(y, D0, mask, batch_size=32, epochs=2)
    b = cabi(y, D0, mask, batch_size=32, epochs=2, want_trace=False)
    same_bits(a, b)


def test_a_mask_of_ones_gives_equal_planes_and_not_the_unmasked_learner():
    import exemplars_vc_amd as evc
    M, N, T = 25, 40, 70
    y, D0, mask = problem(M, N, T, kind="ones")
    kw = dict(batch_size=32, epochs=2)
    (Dr, xr, _, _, _, _), _ = reference(M, N, T, kind="ones", **kw)
    D, x, _, _, _, state = cabi(y, D0, mask, **kw)
    close(D, x, Dr, xr, figure(M, N, T, kind="ones", **kw), "ones")
    S, _ = planes(state, M, N)
    assert np.any(S[0] != 0) and all(np.array_equal(S[m], S[0]) for m in range(1, M))
    Du, _ = evc.learn_dictionary_sparse(y, D0, alpha=1e-3, layout="frame_major", **kw)
    assert np.max(np.abs(Du - D)) > 1e-6


def test_unused_atom_comes_back_bitwise():
    d = load("proxml_m8_n6_t40_unused_atom_k3")
    N, M = d["D0"].shape
    for dtype in (np.float64, np.float32):
        D, x, _, _, _, state = cabi(d["y"], d["D0"], d["mask"], d["x0"], dtype=dtype, **d["kw"])
        assert np.array_equal(D[-1], d["D0"][-1].astype(dtype)) and np.all(x[:, -1] == 0.0)
        S, Q = planes(state, M, N)
        assert np.all(S[:, N - 1, N - 1] == 0.0) and np.all(S[:, N - 1, :] == 0.0) and np.all(Q[N - 1] == 0.0)


def test_nan_frame_poisons_the_dictionary_and_never_stops():
    M, N, T = 25, 33, 50
    y, D0, mask = problem(M, N, T)
    y, mask = y.copy(), mask.copy()
    y[7, 3], mask[7, 3] = np.nan, 1.0
    kw = dict(batch_size=24, epochs=2, tol=1e-3)
    with np.errstate(all="ignore"):
        Dr, xr, n_ep_r, steps_r, trr, _ = pmlr.solve(y, D0, 1e-3, mask=mask, **kw)
    assert np.all(np.isnan(Dr)) and np.all(np.isnan(trr)) and steps_r == 4
    D, x, n_ep, n_st, tr, _ = cabi(y, D0, mask, **kw)
    assert np.all(np.isnan(D)) and np.all(np.isnan(tr)) and (n_ep, n_st) == (2, 4)


def test_zero_epochs_prepares_only():
    M, N, T = 25, 33, 50
    y, D0, mask = problem(M, N, T)
    D, x, n_ep, n_st, tr, state = cabi(y, D0, mask, batch_size=24, epochs=0)
    assert (n_ep, n_st, state[2], tr.size) == (0, 0, 0, 0)
    np.testing.assert_allclose(D, pmlr.unit_atoms(D0), rtol=0, atol=4 * EPS[np.float64])
    S, Q = planes(state, M, N)
    assert np.array_equal(x, np.ones((T, N))) and np.all(S == 0) and np.all(Q == 0)


def test_routed_size():
    """M = 25, N = 256, T = 512, bs = 256: four row panels of four column tiles each, 25 planes, 16 slabs per tile"""
    M, N, T, bs = 25, 256, 512, 256
    kw = dict(batch_size=bs, epochs=1)
    (Dr, xr, _, steps, trr, _), cuts = reference(M, N, T, **kw)
    fig = figure(M, N, T, **kw)
    y, D0, mask = problem(M, N, T)
    D, x, _, n_st, tr, _ = cabi(y, D0, mask, **kw)
    assert n_st == steps == 2
    close(D, x, Dr, xr, fig, "routed")
    np.testing.assert_allclose(tr, trr, rtol=0, atol=2 * 100 * fig)
    zeros_where_cut(x, cuts, some=True)


def test_python_state_resumes():
    import exemplars_vc_amd as evc
    M, N, T = 25, 40, 70
    y, D0, mask = problem(M, N, T)
    order = np.stack([np.random.default_rng(3 + e).permutation(T) for e in range(3)]).astype(np.int32)
    kw = dict(alpha=1e-3, layout="frame_major", batch_size=32, mask=mask, info=True)
    Dw, xw, iw = evc.learn_dictionary_sparse(y, D0, epochs=3, order=order, **kw)
    D1, x1, i1 = evc.learn_dictionary_sparse(y, D0, epochs=2, order=order[:2], **kw)
    D2, x2, i2 = evc.learn_dictionary_sparse(y, D1, x1, epochs=1, order=order[2:], state=i1["state"], **kw)
    assert np.array_equal(D2, Dw) and np.array_equal(x2, xw) and i2["state"][2] == iw["state"][2] == 6
    with pytest.raises(ValueError, match="state"):
        evc.learn_dictionary_sparse(y, D1, x1, epochs=1, order=order[2:], state=i1["state"][1:], **kw)


def test_compact_dictionary_sparse_with_a_mask_beats_its_start():
    """50 + 50 bins, N = 300 exemplars, R = 32, the top third of A's bins missing: convert_prox(mask=...) with the learnt pair
    reconstructs B better than with the R evenly spaced start atoms (a sanity property, not a tolerance)"""
    import exemplars_vc_amd as evc
    rng = np.random.default_rng(21)
    Ma = Mb = 50
    N, R = 300, 32
    basis = rng.random((Ma + Mb, 12)) + 0.05
    act = rng.random((12, N)) * (rng.random((12, N)) < 0.25)
    stacked = basis @ act + 0.01 * rng.random((Ma + Mb, N))
    A, B = stacked[:Ma], stacked[Ma:]
    mask_a = np.ones((Ma, N))
    mask_a[Ma - Ma // 3:] = 0.0
    Wa, Wb, G, info = evc.compact_dictionary_sparse(A, B, R, alpha=1e-4, batch_size=100, epochs=15, mask_a=mask_a)
    assert Wa.shape == (Ma, R) and Wb.shape == (Mb, R) and G.shape == (R, N) and info["n_steps"] == 45
    assert len(info["state"]) == 3 and tuple(info["state"][0].shape) == (Ma + Mb, R, R)
    assert np.all(np.linalg.norm(np.concatenate([Wa, Wb]), axis=0) <= 1 + 1e-12)
    pick = (np.arange(R) * N) // R
    S0 = stacked[:, pick] / np.linalg.norm(stacked[:, pick], axis=0)

    def error(Da, Db):
        Y, _ = evc.convert_prox(Da, Db, A, alpha=1e-4, iters=200, tol=0.0, mask=mask_a)
        return float(np.mean((Y - B) ** 2))
    learnt, start = error(Wa, Wb), error(S0[:Ma], S0[Ma:])
    print("mean squared error of B: learnt %.4e, start atoms %.4e" % (learnt, start))
    assert learnt < start
