"""evc_prox_solve on the GPU against recorded deComP runs (tests/golden/prox_*.npz) and the numpy restatement
(tests/prox_restatement.py), which reproduces every one of them bit for bit (tests/test_prox_host.py).

Everything here is in deComP's orientation: y is T x M, A is N x M (exemplars as rows), x is T x N.

float64 bound.  A GPU sum runs in another order than numpy's, so parity is not bitwise.  tools/make_golden_prox.py reruns the
restatement with the exemplars permuted - another summation order - and records how far the result moves relative to max |x|
(`perm64`): 1.6e-15 .. 3.7e-14 on the non-negative fixtures, 4.3e-10 on the signed one.  Each fixture's bound is 100 times
its own figure, relative to max |x_ref| (all-zero frames occur, so no per-frame bound); the margin is there because another
MFMA order is not one permutation.  Shapes without a fixture get the same bound from the same recipe, computed in the test
(`permutation_figure`), with a floor of K eps under the figure for K updates: with N = 1 there is nothing to permute, yet
every update still rounds differently by about an ulp of max |x|.  n_iter equals the recorded `it` + 1 and every activation
that the reference's threshold cuts by more than 1e-6 thr is exactly 0.0.
float32 bound: the same scheme on the restatement's own float32 run (`perm32`, 1.5e-6 .. 1.8e-5, signed 3.2e-3), against the
float64 restatement, with fixed iteration counts - the stop iterations of a float32 run are not compared.
Measured on an MI355X, float64 (the table of DESIGN.md §5.17): 6.5e-15 .. 2.5e-13 on the non-negative fixtures, 1.2e-9 on the
signed one, at most 2.9e-15 over the geometry sweep and 8.0e-15 at N = 4096; float32: 1.9e-5 .. 2.0e-5 and 1.8e-4."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prox_restatement as pr  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ["prox_m25_n64_t32_fista_pos", "prox_m40_n130_t33_ista_pos", "prox_m25_n64_t32_fista", "prox_m1_n5_t3_fista_pos",
            "prox_m201_n300_t20_fista_pos", "prox_m25_n64_t32_fista_pos_k50", "prox_m25_n64_t32_fista_pos_k100",
            "prox_m25_n64_t32_nnls_ista", "prox_m25_n64_t32_fista_pos_start"]
EPS = {np.float64: float(np.finfo(np.float64).eps), np.float32: float(np.finfo(np.float32).eps)}
_cache = {}


def evc():
    import exemplars_vc_amd
    return exemplars_vc_amd


def load(name):
    if name not in _cache:
        d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
        d["y"], d["A"] = d["y"].astype(np.float64), d["A"].astype(np.float64)
        d["positive"], d["momentum"] = pr.split_method(str(d["method"]))
        d["kw"] = dict(alpha=float(d["alpha"]), tol=float(d["tol"]), positive=d["positive"], momentum=d["momentum"])
        _cache[name] = d                                          # shared: the tests copy before they change one
    return _cache[name]


def problem(M, N, T, seed=0, signed=False):
    key = (M, N, T, seed, signed)
    if key not in _cache:
        _cache[key] = pr.problem(M, N, T, 1000 * seed + 7 * M + 3 * N + T, signed=signed)
    return _cache[key]


def reference(M, N, T, K, seed=0, signed=False, **kw):
    """the restatement of K updates on problem(...): x, n_iter, trace"""
    key = ("ref", M, N, T, K, seed, signed, tuple(sorted(kw.items())))
    if key not in _cache:
        y, A = problem(M, N, T, seed, signed)
        _cache[key] = pr.solve(y, A, iters=K, **dict(dict(alpha=1e-3, tol=0.0, positive=not signed), **kw))
    return _cache[key]


def figure(M, N, T, K, dtype=np.float64, seed=0, signed=False, **kw):
    """the permutation figure of reference(...)'s run"""
    key = ("fig", M, N, T, K, dtype, seed, signed, tuple(sorted(kw.items())))
    if key not in _cache:
        y, A = problem(M, N, T, seed, signed)
        _cache[key] = permutation_figure(y, A, K, dtype, **dict(dict(alpha=1e-3, tol=0.0, positive=not signed), **kw))
    return _cache[key]


def permutation_figure(y, A, K, dtype, x0=None, **kw):
    """tools/make_golden_prox.py's figure: how far the restatement's result moves, relative to max |x|, when the exemplars
    are summed in another order - and at least K eps"""
    kw = dict(kw, iters=K, stop=False, dtype=dtype)
    kw.pop("utt_offsets", None)
    perm = np.random.default_rng(5).permutation(A.shape[0])
    base = pr.solve(y, A, x0=x0, **kw)[0].astype(np.float64)
    moved = pr.solve(y, A[perm], x0=None if x0 is None else x0[:, perm], **kw)[0].astype(np.float64)
    back = np.empty_like(moved)
    back[:, perm] = moved
    top = np.max(np.abs(base))
    return max(float(np.max(np.abs(back - base)) / top) if top > 0 else 0.0, K * EPS[dtype])


def close(x, ref, figure, what=""):
    """max |x - ref| <= 100 figure max |ref|"""
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert x.shape == ref.shape
    top = float(np.max(np.abs(ref))) if ref.size else 0.0
    worst = float(np.max(np.abs(x - ref))) / top if top > 0 else float(np.max(np.abs(x))) if x.size else 0.0
    print("%s: max error %.3e of max |x| (allowed %.3e)" % (what, worst, 100 * figure))
    assert worst <= 100 * figure
    return worst


def stat_close(tr, rtr, fig, ref, A, normalize=True):
    """the stop statistics: differences of activations in the solve's own scaling (x d, d the exemplars' norms), so twice
    the activations' bound times the largest norm"""
    d = float(np.max(np.linalg.norm(A, axis=1))) if normalize else 1.0
    assert np.array_equal(np.isfinite(tr), np.isfinite(rtr))
    np.testing.assert_allclose(tr, rtr, rtol=0, atol=2 * 100 * fig * float(np.max(np.abs(ref))) * d)


def cabi(y, A, x0, iters, *, alpha=1e-3, tol=0.0, positive=True, momentum="fista", normalize=True, check_every=10,
         stop_rule="decomp", lipschitz=0.0, layout="frame_major", dtype=np.float64, pad=0, offs=None, init_value=None):
    """evc_prox_solve through ctypes: every matrix is laid out as `layout` says inside a buffer whose leading dimension is
    `pad` longer than needed and whose padding holds NaN, which must still be there afterwards.  x0 None: EVC_INIT_CONST with
    init_value (default 0) over a buffer full of NaN.  -> x (T x N), n_iter, trace"""
    import torch
    from exemplars_vc_amd import _lib
    L = _lib.lib()
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    fm = layout == "frame_major"
    (N, M), T = A.shape, y.shape[0]

    def stage(mat):
        m = np.asarray(mat, dtype=dtype)
        m = m if fm else m.T
        buf = torch.full((m.shape[0], m.shape[1] + pad), float("nan"), dtype=tdt, device="cuda")
        buf[:, :m.shape[1]] = torch.from_numpy(np.ascontiguousarray(m))
        return buf, m.shape[1]
    (A_d, _), (X_d, _) = stage(A), stage(y)
    H_d, hcols = stage(np.full((T, N), np.nan) if x0 is None else x0)
    o = _lib.ProxOpts()
    o.struct_bytes = C.sizeof(o)
    o.dtype, o.layout, o.iters = (_lib.F64 if dtype == np.float64 else _lib.F32), (_lib.FRAME_MAJOR if fm else _lib.BIN_MAJOR), iters
    o.mode = _lib.PROX_POSITIVE if positive else _lib.PROX_SIGNED
    o.momentum = {"ista": _lib.PROX_ISTA, "fista": _lib.PROX_FISTA, "nesterov": _lib.PROX_NESTEROV}[momentum]
    o.normalize, o.check_every = int(normalize), check_every
    o.stop_rule = {"none": _lib.STOP_NONE, "decomp": _lib.STOP_DECOMP}[stop_rule]
    o.init_mode = _lib.INIT_CONST if x0 is None else _lib.INIT_GIVEN
    o.alpha, o.tol, o.init_value, o.lipschitz = alpha, tol, (0.0 if init_value is None else init_value), lipschitz
    n_utt = 1 if offs is None else len(offs) - 1
    po = None if offs is None else (C.c_int * len(offs))(*offs)
    slots = pr.n_slots(iters, check_every)
    n_iter, trace = np.zeros(n_utt, dtype=np.int32), np.full((n_utt, max(slots, 1)), -1.0)
    nbytes = int(L.evc_prox_workspace_bytes(M, N, T, n_utt, o.dtype))
    assert nbytes > 0
    ws = torch.empty(nbytes + 8, dtype=torch.uint8, device="cuda")
    ld = lambda t: int(t.stride(0))      # noqa: E731
    st = L.evc_prox_solve(A_d.data_ptr(), ld(A_d), X_d.data_ptr(), ld(X_d), H_d.data_ptr(), ld(H_d), M, N, T, po, n_utt,
                          C.byref(o), ws.data_ptr() + 8, nbytes, n_iter.ctypes.data_as(C.POINTER(C.c_int)),
                          trace.ctypes.data_as(C.POINTER(C.c_double)), None)
    assert st == 0, st
    torch.cuda.synchronize()
    out = H_d.cpu().numpy()
    if pad:
        assert np.isnan(out[:, hcols:]).all()                   # the padding of H was not overwritten
    out = out[:, :hcols]
    trace = trace.reshape(-1)[:n_utt * slots].reshape(n_utt, slots)
    return (out if fm else out.T).copy(), n_iter, trace


# ---- the fixtures, through the C ABI in both layouts and through compat.decomp ----
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_through_the_c_abi(name):
    d = load(name)
    K = int(d["maxiter"])
    _, _, rtr, pre, thr = pr.solve_one(d["y"], d["A"], d["kw"]["alpha"], np.zeros_like(d["x"]) if "x0" not in d else d["x0"],
                                       d["kw"]["tol"], K, positive=d["positive"], momentum=d["momentum"], want_pre=True)
    cut = pre < -1e-6 * thr
    assert cut.any()
    for layout in ("frame_major", "bin_major"):
        x, n_iter, tr = cabi(d["y"], d["A"], d.get("x0"), K, layout=layout, pad=3, **d["kw"])
        assert x.dtype == np.float64 and int(n_iter[0]) == int(d["it"]) + 1
        close(x, d["x"], float(d["perm64"]), name + " " + layout)
        assert not x[cut].any()                                     # exact zeros where the threshold cuts
        if d["positive"]:
            assert (x >= 0).all()
        stat_close(tr[0], rtr, float(d["perm64"]), d["x"], d["A"])


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_through_compat_decomp(name):
    from exemplars_vc_amd.compat import decomp
    d = load(name)
    x0 = None if "x0" not in d else d["x0"].copy()
    if bool(d["nnls"]):
        it, x = decomp.nnls.solve(d["y"], d["A"], d["kw"]["alpha"], x=x0, tol=d["kw"]["tol"], method=str(d["method"])[:-4],
                                  maxiter=int(d["maxiter"]))
    else:
        it, x = decomp.lasso.solve(d["y"], d["A"], d["kw"]["alpha"], x=x0, tol=d["kw"]["tol"], method=str(d["method"]),
                                   maxiter=int(d["maxiter"]))
    assert it == int(d["it"]) and x.dtype == np.float64
    close(x, d["x"], float(d["perm64"]), name)
    if x0 is not None:
        assert np.array_equal(x0, d["x0"])                          # the caller's start is not written


def test_compat_flattens_leading_dimensions():
    from exemplars_vc_amd.compat import decomp
    d = load("prox_m25_n64_t32_fista_pos_k50")
    it, x = decomp.lasso.solve(d["y"].reshape(4, 8, 25), d["A"], 1e-3, tol=0.0, method="fista_pos", maxiter=50)
    assert it == 49 and x.shape == (4, 8, 64)
    close(x.reshape(32, 64), d["x"], float(d["perm64"]), "3-D y")
    it32, x32 = decomp.lasso.solve(d["y"].astype(np.float32), d["A"].astype(np.float32), 1e-3, tol=0.0, method="fista_pos",
                                   maxiter=50)
    assert it32 == 49 and x32.dtype == np.float32
    close(x32, d["x"], float(d["perm32"]), "float32 y")


# ---- a batch is its utterances: the recorded per-utterance deComP runs, and bitwise one call per utterance ----
@pytest.mark.parametrize("name", ["prox_m25_n64_t32_fista_pos", "prox_m40_n130_t33_ista_pos", "prox_m201_n300_t20_fista_pos"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_batch_equals_per_utterance(name, dtype):
    d = load(name)
    offs, K = d["offs"].tolist(), int(d["maxiter"])
    kw = dict(d["kw"], dtype=dtype, layout="bin_major", pad=2)
    x, n_iter, tr = cabi(d["y"], d["A"], None, K, offs=offs, **kw)
    x2, n_iter2, tr2 = cabi(d["y"], d["A"], None, K, offs=offs, **kw)
    assert np.array_equal(x, x2) and np.array_equal(n_iter, n_iter2) and np.array_equal(tr, tr2, equal_nan=True)
    for u in range(len(offs) - 1):
        xu, nu, tu = cabi(d["y"][offs[u]:offs[u + 1]], d["A"], None, K, **kw)
        assert np.array_equal(x[offs[u]:offs[u + 1]], xu) and nu[0] == n_iter[u] and np.array_equal(tr[u], tu[0], equal_nan=True)
    if dtype == np.float64:
        assert n_iter.tolist() == (d["it_split"] + 1).tolist() and len(set(n_iter.tolist())) > 1
        close(x, d["x_split"], float(d["perm64"]), name + " batch")
        for u in range(len(offs) - 1):                              # nothing is recorded after an utterance's stop
            c = (int(n_iter[u]) - 1) // 10
            assert np.isfinite(tr[u, :c + 1]).all() and np.isnan(tr[u, c + 1:]).all()


# ---- the two workgroup widths, 8 and 4 wavefronts, chosen from the sizes alone (prox_waves), give the same bits ----
def test_every_workgroup_width_gives_the_same_bits():
    offs = [0, 5440, 10881]                     # N = 257: the batch runs 8 wavefronts (171 x 3 workgroups), its utterances alone 4
    y, A = problem(3, 257, 10881)
    x, n_iter, tr = cabi(y, A, None, 3, offs=offs, check_every=1, tol=0.0)
    ref, _, rtr = reference(3, 257, 10881, 3, check_every=1, utt_offsets=tuple(offs))
    p64 = figure(3, 257, 10881, 3)
    close(x, ref, p64, "8 wavefronts")
    stat_close(tr, rtr, p64, ref, A)
    for u in (0, 1):
        xu, _, tu = cabi(y[offs[u]:offs[u + 1]], A, None, 3, check_every=1, tol=0.0)
        assert np.array_equal(x[offs[u]:offs[u + 1]], xu) and np.array_equal(tr[u], tu[0])
    # one frame below the threshold the whole batch runs 4 wavefronts: the shared frames keep their bits
    xb, _, _ = cabi(y[:10880], A, None, 3, check_every=0)
    assert np.array_equal(xb[:5440], x[:5440])


# ---- geometry: exemplars around the k-slab (16) and the row blocks (64, 128), frames around 16 and the frame block (64) ----
NS, TS, MS = (1, 15, 16, 17, 127, 128, 129), (1, 63, 64, 65, 130), (1, 2, 25, 201)


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("T", TS)
def test_geometry(N, T):
    M = MS[(NS.index(N) + TS.index(T)) % 4]
    y, A = problem(M, N, T)
    (ref, _, rtr), p64 = reference(M, N, T, 5, check_every=2), figure(M, N, T, 5)
    for layout in ("frame_major", "bin_major"):
        x, n_iter, tr = cabi(y, A, None, 5, layout=layout, pad=7, check_every=2)
        assert n_iter.tolist() == [5] and tr.shape == (1, 3)
        close(x, ref, p64, "M %d N %d T %d %s" % (M, N, T, layout))
        stat_close(tr, rtr, p64, ref, A)
        assert (x >= 0).all()


@pytest.mark.parametrize("M", MS)
def test_every_bin_count_meets_both_layouts(M):
    y, A = problem(M, 129, 65, seed=1, signed=True)
    ref, p64 = reference(M, 129, 65, 5, seed=1, signed=True)[0], figure(M, 129, 65, 5, seed=1, signed=True)
    assert (ref < 0).any() and (ref == 0).any()
    for layout in ("frame_major", "bin_major"):
        close(cabi(y, A, None, 5, layout=layout, pad=1, positive=False)[0], ref, p64, "M %d %s" % (M, layout))


# ---- the stop: a stopped utterance of a whole frame block stays frozen while the other runs on ----
def test_a_stopped_utterance_stays_frozen():
    offs = [0, 64, 104]                          # the first utterance is one whole workgroup column: it only returns
    y, A = (m.copy() for m in pr.problem(25, 70, 104, 77))
    y[:64] *= 0.1
    kw = dict(alpha=1e-3, tol=1e-3)
    ref, rn, rtr = pr.solve(y, A, iters=200, utt_offsets=offs, **kw)
    assert rn.tolist() == [61, 200]
    x, n_iter, tr = cabi(y, A, None, 200, offs=offs, **kw)
    assert n_iter.tolist() == [61, 200] and np.isnan(tr[0, 7:]).all() and np.isfinite(tr[1]).all() and tr[0, 6] < 0
    close(x, ref, permutation_figure(y, A, 200, np.float64, **kw), "stopped + running")
    xa, na, ta = cabi(y[:64], A, None, 200, **kw)
    assert na.tolist() == [61] and np.array_equal(x[:64], xa) and np.array_equal(tr[0], ta[0], equal_nan=True)
    xb, nb, _ = cabi(y[64:], A, None, 200, **kw)
    assert nb.tolist() == [200] and np.array_equal(x[64:], xb)
    # stopped at its 61st update, the first utterance holds that iterate: 61 updates without a stop give the same bits
    xc, _, _ = cabi(y[:64], A, None, 61, stop_rule="none", **kw)
    assert np.array_equal(x[:64], xc)


# ---- containment ----
def test_nan_in_a_frame_stays_in_its_frame():
    y, A = problem(25, 129, 65)
    x, n, _ = cabi(y, A, None, 12, layout="bin_major", tol=1e-3)
    yn = y.copy()
    yn[20, 7] = np.nan
    xn, nn, trn = cabi(yn, A, None, 12, layout="bin_major", tol=1e-3)
    keep = np.arange(65) != 20
    assert np.isnan(xn[20]).all() and np.array_equal(xn[keep], x[keep])
    assert n.tolist() == nn.tolist() == [12] and np.isnan(trn).all()     # a NaN statistic compares false: it runs on


def test_nan_in_the_dictionary_reaches_every_activation():
    y, A = (m.copy() for m in problem(25, 129, 65))
    A[40, 3] = np.nan
    x, n_iter, tr = cabi(y, A, None, 11, tol=1e-3)
    assert np.isnan(x).all() and n_iter.tolist() == [11] and np.isnan(tr).all()


# ---- the edges of the call ----
@pytest.mark.parametrize("layout", ["frame_major", "bin_major"])
def test_no_iterations_return_the_start(layout):
    y, A = problem(25, 33, 70)
    x0 = np.random.default_rng(3).random((70, 33))
    x, n_iter, tr = cabi(y, A, x0, 0, layout=layout, pad=5)
    assert np.array_equal(x, x0) and n_iter.tolist() == [0] and tr.shape == (1, 0)
    xc, _, _ = cabi(y, A, None, 0, layout=layout, pad=5, init_value=0.25)
    assert np.array_equal(xc, np.full((70, 33), 0.25))
    # a constant start is the given start of that value
    x1, _, _ = cabi(y, A, None, 4, layout=layout, pad=5, init_value=0.25)
    x2, _, _ = cabi(y, A, np.full((70, 33), 0.25), 4, layout=layout, pad=5)
    assert np.array_equal(x1, x2)
    close(x1, pr.solve(y, A, 1e-3, np.full((70, 33), 0.25), iters=4, tol=0.0)[0],
          permutation_figure(y, A, 4, np.float64, x0=np.full((70, 33), 0.25), alpha=1e-3, tol=0.0), "const start")


def test_no_frames_are_accepted():
    y, A = problem(25, 33, 70)
    x, n_iter, tr = cabi(y[:0], A, None, 20, tol=1e-3)
    assert x.shape == (0, 33) and n_iter.tolist() == [20] and np.isnan(tr).all()
    x, n_iter, tr = cabi(y, A, None, 20, tol=0.0, offs=[0, 0, 70, 70])
    assert n_iter.tolist() == [20, 20, 20] and np.isnan(tr[[0, 2]]).all() and np.isfinite(tr[1]).all()
    close(x, reference(25, 33, 70, 20)[0], figure(25, 33, 70, 20), "empty utterances around a full one")


def test_options():
    y, A = problem(25, 33, 70)
    G = A / np.linalg.norm(A, axis=1, keepdims=True)
    L = float(np.max(np.sum(np.abs(G @ G.T), axis=0)))
    for kw in (dict(lipschitz=3 * L), dict(normalize=False), dict(normalize=False, lipschitz=800.0),
               dict(momentum="nesterov"), dict(momentum="ista"), dict(momentum="nesterov", positive=False)):
        rkw = dict(dict(alpha=1e-3, tol=0.0), **kw)
        ref = pr.solve(y, A, iters=25, **rkw)[0]
        x, n_iter, _ = cabi(y, A, None, 25, **rkw)
        assert n_iter.tolist() == [25] and ref.any()
        close(x, ref, permutation_figure(y, A, 25, np.float64, **rkw), str(kw))
    slow = cabi(y, A, None, 25, lipschitz=3 * L)[0]
    assert not np.array_equal(slow, cabi(y, A, None, 25)[0])               # the override is honoured
    # the Nesterov schedule with the stop, against the restatement
    ref, rn, rtr = pr.solve(y, A, 1e-3, iters=300, tol=1e-3, momentum="nesterov")
    x, n_iter, tr = cabi(y, A, None, 300, tol=1e-3, momentum="nesterov")
    print("nesterov stops after", rn, "margin", np.nanmin(np.abs(rtr)) / 1e-3)
    assert np.nanmin(np.abs(rtr)) >= 1e-6 * 1e-3 and n_iter.tolist() == rn.tolist()
    close(x, ref, permutation_figure(y, A, 300, np.float64, alpha=1e-3, tol=1e-3, momentum="nesterov"), "nesterov with stop")


# ---- the Python surface ----
def test_convert_prox_is_solve_then_synthesize():
    import torch
    rng = np.random.default_rng(5)
    y, A = problem(25, 64, 40)
    B = rng.random((201, 64))
    kw = dict(alpha=1e-3, iters=60, tol=1e-3)
    Y, H, info = evc().convert_prox(A.T.copy(), B, y.T.copy(), info=True, **kw)
    H2, info2 = evc().solve_activations_prox(A.T.copy(), y.T.copy(), info=True, **kw)
    assert np.array_equal(H, H2) and np.array_equal(Y, evc().synthesize(B, H2))
    ref, rn, rtr = pr.solve(y, A, 1e-3, iters=60, tol=1e-3)
    close(H.T, ref, permutation_figure(y, A, 60, np.float64, alpha=1e-3, tol=1e-3), "convert_prox")
    slots = pr.n_slots(60, 10)
    assert info["kernel"] == "k_prox_sweep" and info["n_iter"].tolist() == rn.tolist() and info["change"].shape == (1, slots)
    assert info["launches"] == 60 + slots and np.array_equal(np.isfinite(info["change"]), np.isfinite(rtr))
    assert Y.shape == (201, 40) and (Y >= 0).all() and (H == 0).any()
    np.testing.assert_allclose(Y, B @ H, rtol=1e-12, atol=1e-12 * np.abs(B @ H).max())
    # frame-major device tensors in, device tensors out; utterances; a signed solve from a given start
    x0 = rng.random((40, 64)) * 0.05
    Yt, Ht = evc().convert_prox(torch.from_numpy(A).cuda(), torch.from_numpy(B.T.copy()).cuda(), torch.from_numpy(y).cuda(),
                                torch.from_numpy(x0).cuda(), layout="frame_major", positive=False, utt_offsets=[0, 15, 40], **kw)
    assert isinstance(Yt, torch.Tensor) and Yt.is_cuda and tuple(Yt.shape) == (40, 201)
    ref2 = pr.solve(y, A, 1e-3, x0, iters=60, tol=1e-3, positive=False, utt_offsets=[0, 15, 40])[0]
    close(Ht.cpu().numpy(), ref2, permutation_figure(y, A, 60, np.float64, x0=x0, alpha=1e-3, tol=1e-3, positive=False),
          "convert_prox frame_major")


# ---- the routed size of the flagship: N = 4096, one utterance of 688 frames ----
def test_routed_size():
    y, A = problem(25, 4096, 688)
    (ref, _, rtr), p64 = reference(25, 4096, 688, 3, check_every=1), figure(25, 4096, 688, 3)
    H, info = evc().solve_activations_prox(A, y, alpha=1e-3, iters=3, tol=0.0, check_every=1, layout="frame_major", info=True)
    close(H, ref, p64, "N 4096 T 688")
    stat_close(info["change"], rtr, p64, ref, A)


# ---- float32: fixed iteration counts, against the float64 restatement ----
@pytest.mark.parametrize("case", ["prox_m25_n64_t32_fista_pos_k50", "prox_m25_n64_t32_fista_pos_k100", "prox_m25_n64_t32_fista",
                                  (25, 17, 63), (2, 129, 65), (201, 128, 130), (1, 127, 1)])
def test_float32(case):
    if isinstance(case, str):
        d = load(case)
        y, A, K = d["y"], d["A"], min(int(d["maxiter"]), 100)
        kw = dict(alpha=d["kw"]["alpha"], positive=d["positive"], momentum=d["momentum"])
        ref = pr.solve(y, A, iters=K, tol=0.0, **kw)[0]
        p32 = float(d["perm32"]) if K == int(d["maxiter"]) else permutation_figure(y, A, K, np.float32, tol=0.0, **kw)
    else:
        (y, A), K, kw = problem(*case), 5, dict(alpha=1e-3)
        ref, p32 = reference(*case, K)[0], figure(*case, K, dtype=np.float32)
    for layout in ("frame_major", "bin_major"):
        x, n_iter, _ = cabi(y, A, None, K, dtype=np.float32, layout=layout, pad=3, tol=0.0, **kw)
        assert x.dtype == np.float32 and n_iter.tolist() == [K]
        close(x, ref, p32, "%s %s float32" % (case, layout))
