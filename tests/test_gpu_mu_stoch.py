"""evc_mu_stoch_learn on the GPU against recorded deComP runs (tests/golden/mus_*.npz: nmf.solve(minibatch=bs) with its six
mini-batch methods) and the numpy restatement (tests/mu_stoch_restatement.py), which reproduces every one of them bit for bit
(tests/test_mu_stoch_host.py).

Everything here is in deComP's orientation: y is T x M, D is R x M (atoms as rows), x is T x R, mask is T x M.

The bound is the family's: max |. - ref| <= 100 figure max |ref|, for D, x and the statistics.  `figure` is the fixture's
`perm64` / `perm32`: how far the restatement's result moves when the atoms, the bins and the frames inside every batch are
permuted, as tools/make_golden_mu_stoch.py records it, with a floor of (dictionary updates) eps.  Shapes without a fixture get
the same recipe computed in the test (msr.permutation_figure).  Zeros are exact where the reference's are and NaN appears
where and only where the reference has it.  float32: against the float64 reference within 100 perm32.  The worst errors
measured on an MI355X are tabulated in DESIGN.md §5.23."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mu_masked_restatement as mmr  # noqa: E402
import mu_stoch_restatement as msr  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ["mus_asg_m25_r8_t50_bs16_l2_mask", "mus_gsg_m40_r19_t70_bs16_kl", "mus_asag_m201_r12_t40_bs16_kl_mask",
            "mus_asag_m40_r19_t70_bs16_l2_mid", "mus_gsag_m25_r8_t50_bs7_l2_last", "mus_svrmu_m40_r19_t70_bs16_l2_mask",
            "mus_svrmu_m25_r8_t48_bs16_kl_mask", "mus_svrmuacc_m25_r8_t50_bs16_kl", "mus_asg_m2_r3_t5_bs2_kl"]
METHOD_CODES = {"asg": 0, "asag": 1, "gsag": 2, "svrmu": 3}
ROUTES = {None: 0, "fused": 1, "unfused": 2}
_cache = {}


def load(name):
    if name not in _cache:
        d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
        for k in ("y", "D0", "mask", "x0"):
            if k in d:
                d[k] = d[k].astype(np.float64)
        d.setdefault("mask", None)
        d["x0"] = d["x0"] if "x0" in d else np.ones((d["y"].shape[0], d["D0"].shape[0]))
        for k in ("loss", "method"):
            d[k] = str(d[k])
        for k in ("it", "n_steps", "n_epochs", "maxiter", "bs", "inner_iters", "seed"):
            d[k] = int(d[k])
        for k in ("tol", "forget_rate", "alpha", "beta", "perm64", "perm32"):
            d[k] = float(d[k])
        d["native"] = msr.NATIVE[d["method"]]
        d["kw"] = dict(method=d["native"], loss=d["loss"], bs=d["bs"], epochs=d["maxiter"] - 1, tol=d["tol"],
                       forget_rate=d["forget_rate"], alpha=d["alpha"], inner_iters=d["inner_iters"])
        _cache[name] = d                                          # shared: the tests copy before they change one
    return _cache[name]


def close(x, ref, figure, what=""):
    """max |x - ref| <= 100 figure max |ref|; zeros exact where the reference's are; NaN where and only where it has NaN"""
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert x.shape == ref.shape and np.array_equal(np.isnan(x), np.isnan(ref)), what
    assert (x[ref == 0] == 0).all(), what
    good = ~np.isnan(ref)
    top = float(np.max(np.abs(ref[good]))) if good.any() else 0.0
    diff = float(np.max(np.abs(x[good] - ref[good]))) if good.any() else 0.0
    worst = diff / top if top > 0 else diff
    print("%s: max error %.3e of max |ref| (allowed %.3e)" % (what, worst, 100 * figure))
    assert worst <= 100 * figure, what
    return worst


def cabi(y, D0, mask, x0, order, *, method, loss, bs, epochs, tol=0.0, forget_rate=0.5, alpha=1.0, inner_iters=1, route=None,
         layout="frame_major", dtype=np.float64, pad=0, order_rows=None, expect=0):
    """evc_mu_stoch_learn through ctypes: every matrix is laid out as `layout` says inside a buffer whose leading dimension is
    `pad` longer than needed (the mask's: pad + 2) and whose padding holds NaN, which must still be there afterwards.  mask
    None: a NULL pointer; order None: a NULL pointer.  -> dict(D, x, n_epochs, n_steps, trace) or, where `expect` is a
    non-zero status, that status"""
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
    (W_d, wcols), (X_d, _), (H_d, hcols) = stage(D0, pad), stage(y, pad), stage(x0, pad)
    M_d = None if mask is None else stage(mask, pad + 2)[0]
    o = _lib.MuStochOpts()
    o.struct_bytes = C.sizeof(o)
    o.dtype, o.layout = (_lib.F64 if dtype == np.float64 else _lib.F32), (_lib.FRAME_MAJOR if fm else _lib.BIN_MAJOR)
    o.loss = {"l2": _lib.LOSS_FROBENIUS, "kl": _lib.LOSS_KL}[loss]
    o.method, o.batch_size, o.epochs, o.inner_iters, o.route = METHOD_CODES[method], bs, epochs, inner_iters, ROUTES[route]
    o.forget_rate, o.alpha, o.tol = forget_rate, alpha, tol
    po = None
    if order is not None:
        order = np.ascontiguousarray(order, dtype=np.int32)
        po = order.ctypes.data_as(C.POINTER(C.c_int))
    o.order_rows = (0 if order is None else order.shape[0]) if order_rows is None else order_rows
    n_upd = msr.n_updates(method, epochs, T, bs)
    n_epochs, n_steps, trace = C.c_int(-1), C.c_int(-1), np.full(max(n_upd, 1), -1.0)
    nbytes = int(L.evc_mu_stoch_learn_workspace_bytes(M, R, T, bs, o.method, o.dtype))
    assert nbytes > 0
    ws = torch.empty(nbytes + 8, dtype=torch.uint8, device="cuda")
    ld = lambda t: int(t.stride(0))      # noqa: E731
    st = L.evc_mu_stoch_learn(X_d.data_ptr(), ld(X_d), None if M_d is None else M_d.data_ptr(), 0 if M_d is None else ld(M_d),
                              W_d.data_ptr(), ld(W_d), H_d.data_ptr(), ld(H_d), po, M, R, T, C.byref(o), ws.data_ptr() + 8,
                              nbytes, C.byref(n_epochs), C.byref(n_steps), trace.ctypes.data_as(C.POINTER(C.c_double)), None)
    if expect:
        assert st == expect, st
        return st
    assert st == 0, st
    torch.cuda.synchronize()
    outs = []
    for buf, cols in ((W_d, wcols), (H_d, hcols)):
        out = buf.cpu().numpy()
        if pad:
            assert np.isnan(out[:, cols:]).all()                    # the padding was not written
        outs.append(np.ascontiguousarray(out[:, :cols] if fm else out[:, :cols].T))
    return dict(D=outs[0], x=outs[1], n_epochs=n_epochs.value, n_steps=n_steps.value, trace=trace[:n_upd])


def run_fixture(d, **over):
    kw = dict(d["kw"], **over)
    return cabi(d["y"], d["D0"], d["mask"], d["x0"], d["order"], **kw)


def check_fixture(d, r, fig, what):
    assert r["n_steps"] == d["n_steps"] and r["n_epochs"] == d["n_epochs"]
    assert (r["n_epochs"] if d["it"] < d["maxiter"] else d["maxiter"]) == d["it"]
    n = len(d["stats"])
    worst = max(close(r["D"], d["D"], fig, what + " D"), close(r["x"], d["x"], fig, what + " x"),
                close(r["trace"][:n], d["stats"], fig, what + " stat"))
    assert np.isnan(r["trace"][n:]).all()                           # NaN after the stop
    never = ~d["visited"]
    assert np.array_equal(r["x"][never], d["x0"][never].astype(r["x"].dtype))      # bitwise the start
    return worst


# ---- the recorded deComP runs ----
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_float64(name):
    d = load(name)
    fig = max(d["perm64"], len(d["stats"]) * np.finfo(np.float64).eps)
    check_fixture(d, run_fixture(d), fig, name)


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_float32(name):
    d = load(name)
    fig = max(d["perm32"], len(d["stats"]) * float(np.finfo(np.float32).eps))
    check_fixture(d, run_fixture(d, dtype=np.float32), fig, name + " f32")


@pytest.mark.parametrize("name", ["mus_asag_m40_r19_t70_bs16_l2_mid", "mus_svrmu_m25_r8_t48_bs16_kl_mask",
                                  "mus_gsag_m25_r8_t50_bs7_l2_last", "mus_gsg_m40_r19_t70_bs16_kl"])
def test_repeatable_and_routes_agree(name):
    d = load(name)
    fig = max(d["perm64"], len(d["stats"]) * np.finfo(np.float64).eps)
    runs = {}
    for route in ("fused", "unfused"):
        a, b = run_fixture(d, route=route), run_fixture(d, route=route)
        for k in ("D", "x", "trace"):
            assert np.array_equal(a[k], b[k], equal_nan=True), (route, k)           # the same call, the same bits
        assert (a["n_steps"], a["n_epochs"]) == (b["n_steps"], b["n_epochs"])
        runs[route] = a
        check_fixture(d, a, fig, name + " " + route)
    auto = run_fixture(d)                                                            # R <= 256: the fused route
    assert all(np.array_equal(auto[k], runs["fused"][k], equal_nan=True) for k in ("D", "x", "trace"))
    close(runs["fused"]["D"], runs["unfused"]["D"], fig, name + " fused vs unfused D")
    close(runs["fused"]["x"], runs["unfused"]["x"], fig, name + " fused vs unfused x")


# ---- identities that pin the method code ----
def same_bits(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("D", "x", "trace")) and a["n_steps"] == b["n_steps"]


def test_asag_with_rho_one_is_asg():
    d = load("mus_asg_m25_r8_t50_bs16_l2_mask")
    assert same_bits(run_fixture(d, method="asag", forget_rate=1.0), run_fixture(d, method="asg"))


def test_null_order_is_the_identity_and_one_row_is_repeated():
    d = load("mus_gsg_m40_r19_t70_bs16_kl")
    T, epochs = d["y"].shape[0], 3
    ident = np.tile(np.arange(T, dtype=np.int32), (epochs, 1))
    kw = dict(d["kw"], epochs=epochs)
    a = cabi(d["y"], d["D0"], d["mask"], d["x0"], None, **kw)
    assert same_bits(a, cabi(d["y"], d["D0"], d["mask"], d["x0"], ident, **kw))
    row = d["order"][:1]
    assert same_bits(cabi(d["y"], d["D0"], d["mask"], d["x0"], row, **kw),
                     cabi(d["y"], d["D0"], d["mask"], d["x0"], np.tile(row, (epochs, 1)), **kw))
    assert not same_bits(a, cabi(d["y"], d["D0"], d["mask"], d["x0"], row, **kw))


@pytest.mark.parametrize("name", ["mus_asg_m25_r8_t50_bs16_l2_mask", "mus_gsg_m40_r19_t70_bs16_kl"])
def test_first_step_is_the_masked_solve(name):
    """after one step H_F is bitwise evc_mu_masked_solve(iters = 1, EVC_INIT_GIVEN) on the gathered frames"""
    from test_gpu_mu_masked import cabi as mum_cabi
    d = load(name)
    T, bs = d["y"].shape[0], d["bs"]
    if T // bs != 1:                     # one step per epoch: keep bs, cut the frames
        T = bs + bs // 2
    y, x0 = d["y"][:T], d["x0"][:T]
    mask = None if d["mask"] is None else d["mask"][:T]
    order = np.random.default_rng(3).permutation(T).astype(np.int32)[None, :]
    r = cabi(y, d["D0"], mask, x0, order, **dict(d["kw"], epochs=1, tol=0.0))
    assert r["n_steps"] == 1
    F = order[0, :bs]
    # the ABI normalises W on entry: epochs = 0 returns exactly that dictionary
    ent = cabi(y, d["D0"], mask, x0, order, **dict(d["kw"], epochs=0))["D"]
    x1, _, _ = mum_cabi(y[F], ent, None if mask is None else mask[F], x0[F], 1, d["loss"])
    assert np.array_equal(r["x"][F], x1)
    rest = np.setdiff1d(np.arange(T), F)
    assert np.array_equal(r["x"][rest], x0[rest])


def test_null_mask_is_the_mask_of_ones():
    for name in ("mus_gsg_m40_r19_t70_bs16_kl", "mus_gsag_m25_r8_t50_bs7_l2_last", "mus_svrmuacc_m25_r8_t50_bs16_kl"):
        d = load(name)
        assert d["mask"] is None
        kw = dict(d["kw"], epochs=min(d["kw"]["epochs"], 4))
        order = d["order"][:kw["epochs"]] if d["order"].shape[0] > 1 else d["order"]
        assert same_bits(cabi(d["y"], d["D0"], None, d["x0"], order, **kw),
                         cabi(d["y"], d["D0"], np.ones_like(d["y"]), d["x0"], order, **kw))


# ---- the geometry of k_mus_dict_grad against the restatement ----
def problem(M, R, T, seed, kind):
    key = ("p", M, R, T, seed, kind)
    if key not in _cache:
        s = 1000 * seed + 7 * M + 3 * R + T
        y, _ = mmr.problem(M, R, T, s)
        rng = np.random.default_rng(s + 300)
        D0 = rng.random((R, M)) + 0.05
        x0 = rng.random((T, R)) + 0.125
        _cache[key] = (y, D0, x0, None if kind is None else mmr.problem_mask(T, M, s, kind))
    return _cache[key]


def reference(y, D0, x0, mask, order, **kw):
    """the restatement and its permutation figure (floored), computed once per case"""
    key = ("ref", id(y), id(mask), None if order is None else order.tobytes(), tuple(sorted(kw.items())))
    if key not in _cache:
        rk = dict(kw, batch_size=kw["bs"])
        del rk["bs"]
        _cache[key] = (msr.learn(y, D0, x0, mask=mask, order=order, **rk),
                       msr.permutation_figure(y, D0, mask, np.float64, x0=x0, order=order, **dict(rk, tol=0.0)), y, mask)
    return _cache[key][:2]


GEOMETRY = [  # M, R, T, bs, method, mask kind, layout, pad, route
    (1, 17, 37, 16, "asg", None, "frame_major", 0, None),
    (17, 1, 10, 3, "asag", "binary", "bin_major", 3, None),
    (528, 33, 40, 17, "gsag", "weights", "frame_major", 5, None),
    (25, 256, 140, 65, "svrmu", "binary", "bin_major", 0, "fused"),
    (17, 17, 5, 1, "svrmu", None, "frame_major", 1, None),
    (25, 17, 47, 15, "asg", "weights", "bin_major", 2, "fused"),
    (40, 33, 35, 16, "asag", "binary", "frame_major", 0, "unfused"),
    (25, 64, 150, 65, "gsag", None, "bin_major", 7, None),
]


@pytest.mark.parametrize("loss", mmr.LOSSES)
@pytest.mark.parametrize("case", GEOMETRY, ids=lambda c: "m%d_r%d_t%d_bs%d_%s" % c[:5])
def test_geometry_edges(case, loss):
    M, R, T, bs, method, kind, layout, pad, route = case
    y, D0, x0, mask = problem(M, R, T, 1, kind)
    order = msr.frame_orders(T, 2, 11 + M, method)
    kw = dict(method=method, loss=loss, bs=bs, epochs=2, forget_rate=0.4, alpha=0.9, inner_iters=2 if method == "svrmu" else 1)
    ref, fig = reference(y, D0, x0, mask, order, **kw)
    r = cabi(y, D0, mask, x0, order, layout=layout, pad=pad, route=route, **kw)
    what = "m%d r%d t%d bs%d %s %s" % (M, R, T, bs, method, loss)
    assert r["n_steps"] == ref["n_steps"] == 2 * (T // bs)
    close(r["D"], ref["D"], fig, what + " D")
    close(r["x"], ref["x"], fig, what + " x")
    close(r["trace"], ref["stats"], fig, what + " stat")
    assert np.array_equal(r["x"][~ref["visited"]], x0[~ref["visited"]])


def test_r_257_takes_the_unfused_route():
    from exemplars_vc_amd import _lib
    L = _lib.lib()
    assert L.evc_mu_stoch_learn_route(257, 0) == 2 and L.evc_mu_stoch_learn_route(257, 1) == 0
    assert L.evc_mu_stoch_learn_route(64, 0) == 1 and L.evc_mu_stoch_learn_route(256, 0) == 1 and L.evc_mu_stoch_learn_route(256, 1) == 1
    y, D0, x0, mask = problem(25, 257, 40, 2, "binary")
    kw = dict(method="asg", loss="l2", bs=16, epochs=2)
    ref, fig = reference(y, D0, x0, mask, None, **kw)
    r = cabi(y, D0, mask, x0, None, **kw)
    close(r["D"], ref["D"], fig, "r257 D")
    close(r["x"], ref["x"], fig, "r257 x")
    assert cabi(y, D0, mask, x0, None, route="fused", expect=-3, **kw) == -3


# ---- frames without data, and a NaN ----
@pytest.mark.parametrize("loss", mmr.LOSSES)
@pytest.mark.parametrize("route", ["fused", "unfused"])
def test_a_frame_without_data_and_a_nan_frame(loss, route):
    y, D0, x0, mask = problem(25, 17, 50, 3, "binary")
    mask = mask.copy()
    mask[5] = 0.0                                       # a frame whose mask is all zero: its activations become exactly 0
    kw = dict(method="asg", loss=loss, bs=16, epochs=2)
    ref, fig = reference(y, D0, x0, mask, None, **kw)
    r = cabi(y, D0, mask, x0, None, route=route, **kw)
    assert (ref["x"][5] == 0).all() and (r["x"][5] == 0).all()
    close(r["D"], ref["D"], fig, "zero frame D")
    close(r["x"], ref["x"], fig, "zero frame x")
    yn = y.copy()
    yn[20, 3] = np.nan                                  # in the second batch: the first update is finite, the second poisons W
    refn, _ = reference(yn, D0, x0, mask, None, **kw)
    rn = cabi(yn, D0, mask, x0, None, route=route, **kw)
    assert np.isfinite(refn["stats"][0]) and np.isnan(refn["stats"][1:]).all() and np.isnan(refn["D"]).all()
    close(rn["D"], refn["D"], fig, "nan frame D")
    close(rn["x"], refn["x"], fig, "nan frame x")
    close(rn["trace"], refn["stats"], fig, "nan frame stat")
    assert rn["n_steps"] == refn["n_steps"]


# ---- the compat layer end to end ----
@pytest.mark.parametrize("name", ["mus_asag_m40_r19_t70_bs16_l2_mid", "mus_svrmu_m40_r19_t70_bs16_l2_mask",
                                  "mus_svrmuacc_m25_r8_t50_bs16_kl"])
def test_compat_nmf_solve_minibatch(name):
    from exemplars_vc_amd.compat import decomp
    d = load(name)
    extra = dict(alpha=d["alpha"], beta=d["beta"]) if d["native"] == "svrmu" else dict(forget_rate=d["forget_rate"])
    it, D, x = decomp.nmf.solve(d["y"], d["D0"], d["x0"], tol=d["tol"], minibatch=d["bs"], maxiter=d["maxiter"], method=d["method"],
                                likelihood=d["loss"], mask=d["mask"], random_seed=d["seed"], **extra)
    fig = max(d["perm64"], len(d["stats"]) * np.finfo(np.float64).eps)
    assert it == d["it"] and D.shape == d["D"].shape and x.shape == d["x"].shape
    close(D, d["D"], fig, name + " compat D")
    close(x, d["x"], fig, name + " compat x")
