"""Mini-batch dictionary learning on the GPU (evc_online_learn) against scikit-learn's recorded MiniBatchNMF runs
(tests/golden/online_sk_*.npz) and the numpy restatement that reproduces them (online_restatement.py,
test_online_host.py).  `-m gpu`.

float64: W and H within rtol 1e-9 with zeros exact, n_steps and n_iter equal.  float32: ||delta|| / ||ref|| <= 1e-4.
The traces: see close_cost and close_change."""
import ctypes as C
import functools
import glob
import hashlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import online_restatement as onr  # noqa: E402
from beta_restatement import EPS  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "online_sk_*.npz")))
RTOL = 1e-9
FUSED_MAX_R = 256           # what the fused route holds when forced (include/evc.h)


def close(got, want, what, rtol=RTOL):
    """test_gpu_beta_learn.close"""
    got, want = np.asarray(got), np.asarray(want)
    if want.dtype == np.float32:
        r = np.linalg.norm(got.astype(float) - want) / np.linalg.norm(want)
        print(f"{what}: float32 norm-relative error {r:.3e}")
        assert got.dtype == np.float32 and r <= 1e-4, (what, r)
        return
    nz = want != 0
    r = float(np.max(np.abs(got[nz] - want[nz]) / np.abs(want[nz])))
    print(f"{what}: max relative error {r:.3e}, zeros {int((~nz).sum())}")
    assert r <= rtol and not got[~nz].any(), (what, r)


def _slack(X, W, H, beta):
    V = np.maximum(W @ H, EPS)
    return float(np.sum(V ** (beta - 1.0) * np.abs(V - X)))


def close_cost(got, want, slack_per_frame, held=1e-9):
    """the batch costs against the reference's, in test_gpu_beta_learn.close_err's form.  dD/dV = V^(beta-2) (V - X) per
    entry; W and H_b are held to a relative `held` each, so V = W H_b moves by at most 2 held relative and the batch's
    divergence by 2 held sum V^(beta-1) |V - X| (slack, taken at the factors the step's cost is evaluated on), which the
    cost divides by T_b.  The penalty terms are sums of positive terms held to 2 held relative: inside the relative term
    of 10 held."""
    got, want = np.asarray(got), np.asarray(want)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    atol = 2 * held * np.asarray(slack_per_frame)[:int(ok.sum())]
    err = np.abs(got[ok] - want[ok])
    print("cost", got[ok], "max error / bound", float(np.max(err / (atol + 10 * held * np.abs(want[ok])))))
    assert (err <= atol + 10 * held * np.abs(want[ok])).all()


def close_change(got, want, held=1e-9):
    """||W_new - W_old|| / ||W_new||: W_old and W_new are each held to `held` relative, so the ratio moves by at most
    about 2 held absolute: |got - want| <= 4 held + 10 held want"""
    got, want = np.asarray(got), np.asarray(want)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok])
    print("change", got[ok], "max error", float(err.max()) if err.size else 0.0)
    assert (err <= 4 * held + 10 * held * want[ok]).all()


def options(d):
    """the keyword arguments of learn_dictionary_online / online_restatement.learn a fixture was recorded with"""
    M = d["X"].shape[0]
    a, r = float(d["alpha"]), float(d["l1_ratio"])
    mni = int(d["max_no_improvement"])
    return dict(beta=float(d["beta"]), batch_size=int(d["batch_size"]), max_iter=int(d["max_iter"]),
                forget_factor=float(d["forget_factor"]), tol=float(d["tol"]), max_no_improvement=None if mni < 0 else mni,
                l1_h=M * a * r, l2_h=M * a * (1 - r), l1_w=a * r, l2_w=a * (1 - r))


def kernel_splits(M, R):
    from exemplars_vc_amd import _lib
    L = _lib.lib()
    return lambda Tb: int(L.evc_online_splits(M, R, Tb))


def restate(d, S=None, **over):
    """(W, H, n_iter, n_steps, cost, change, (A, B), slack per frame of every step) of the restatement, with the kernels'
    frame ranges unless S says otherwise"""
    M, R = d["W0"].shape
    kw = dict(options(d), **over)
    beta = kw.pop("beta")
    bs, K = kw.pop("batch_size"), kw.pop("max_iter")
    slack = []
    X = np.asarray(d["X"], dtype=np.float64)
    out = onr.learn(d["X"], d["W0"], d["H0"], beta, bs, K, S=S or kernel_splits(M, R), dtype=np.dtype(str(d["dtype"])),
                    on_step=lambda k, t0, t1, W, Hb: slack.append(
                        _slack(X[:, t0:t1], W.astype(float), Hb.astype(float), beta) / (t1 - t0)), **kw)
    return out + (np.array(slack),)


@functools.lru_cache(maxsize=None)
def restated(path):
    return restate(np.load(path))


def test_there_are_fixtures():
    assert len(FILES) == 18


def _check_fixture(path, route):
    import exemplars_vc_amd as evc
    d = np.load(path)
    M, R = d["W0"].shape
    T = d["X"].shape[1]
    kw = dict(options(d), layout="bin_major", info=True, route=route)
    if route == "fused" and R > FUSED_MAX_R:
        with pytest.raises(evc._lib.EvcError) as e:
            evc.learn_dictionary_online(d["X"], d["W0"], d["H0"], **kw)
        assert e.value.status == -3
        return
    W, H, info = evc.learn_dictionary_online(d["X"], d["W0"], d["H0"], **kw)
    assert info["n_steps"] == int(d["n_steps"]) and info["n_iter"] == int(d["n_iter"])
    assert info["route"] == (route or ("fused", "unfused")[evc._lib.lib().evc_beta_learn_route(M, R, T) - 1])
    close(W, d["W"], "W")
    close(H, d["H"], "H")
    n = info["n_steps"]
    per_pass = -(-T // min(int(d["batch_size"]), T))
    assert info["cost"].shape == info["change"].shape == (int(d["max_iter"]) * per_pass,)
    want_cost, want_change = np.full(info["cost"].shape, np.nan), np.full(info["cost"].shape, np.nan)
    want_cost[:n], want_change[:n] = d["cost"], d["change"]
    slack = restated(path)[7]
    held = 1e-9 if d["X"].dtype == np.float64 else 1e-4       # what the factors are held to
    close_cost(info["cost"], want_cost, slack, held)
    close_change(info["change"], want_change, held)
    if "_flush_" in path:
        assert (W == 0).sum() >= 10 or (H == 0).sum() >= 10


@pytest.mark.parametrize("path", FILES, ids=os.path.basename)
def test_fixture_through_learn_dictionary_online(path):
    _check_fixture(path, None)


@pytest.mark.parametrize("route", ["fused", "unfused"])
@pytest.mark.parametrize("path", FILES, ids=os.path.basename)
def test_fixture_with_the_route_forced(path, route):
    _check_fixture(path, route)


NO_STOP = os.path.join(GOLDEN, "online_sk_m25_r24_t330_bs100_k3_b1p5.npz")       # T = 330: a short last batch of 30
REG = os.path.join(GOLDEN, "online_sk_m25_r24_t300_bs100_k3_reg_b1p5.npz")


@pytest.mark.parametrize("route", ["fused", "unfused"])
@pytest.mark.parametrize("S", [1, 3, 7])
def test_forced_frame_ranges_agree_with_the_restatement(S, route):
    """batches of 100 and 30 frames in 7 ranges: 14 or 15 and 4 or 5 frames each, no multiple of the fused kernel's 16"""
    import exemplars_vc_amd as evc
    d = np.load(NO_STOP)
    W, H, info = evc.learn_dictionary_online(d["X"], d["W0"], d["H0"], layout="bin_major", info=True, route=route, splits=S,
                                             **options(d))
    Wr, Hr, n_iter, n_steps, cost, change, _, slack = restate(d, S=S)
    assert info["n_steps"] == n_steps == 12 and info["n_iter"] == n_iter == 3
    close(W, Wr, "W")
    close(H, Hr, "H")
    close_cost(info["cost"], cost, slack)
    close_change(info["change"], change)


SENTINEL = -12345.25


def _raw_call(d, layout, pad, route=0, **over):
    """evc_online_learn itself with every leading dimension at its minimum + pad: (W, H, A, B, trace, padding intact)"""
    import torch
    from exemplars_vc_amd import _lib
    L = _lib.lib()
    fm = layout == "frame_major"
    M, T = d["X"].shape
    R = d["W0"].shape[1]
    kw = dict(options(d), **over)

    def padded(a):
        a = np.ascontiguousarray(a.T) if fm else a
        b = np.full((a.shape[0], a.shape[1] + pad), SENTINEL)
        b[:, :a.shape[1]] = a
        return torch.from_numpy(b).cuda()
    Xb, Wb, Hb = padded(d["X"]), padded(d["W0"]), padded(d["H0"])
    Ab, Bb = padded(np.zeros_like(d["W0"])), padded(np.zeros_like(d["W0"]))
    o = _lib.OnlineOpts()
    o.struct_bytes = C.sizeof(_lib.OnlineOpts)
    o.dtype, o.layout = _lib.F64, _lib.FRAME_MAJOR if fm else _lib.BIN_MAJOR
    o.batch_size, o.max_iter, o.beta, o.forget_factor = kw["batch_size"], kw["max_iter"], kw["beta"], kw["forget_factor"]
    o.max_no_improvement = -1 if kw["max_no_improvement"] is None else kw["max_no_improvement"]
    o.tol, o.l1_h, o.l2_h, o.l1_w, o.l2_w = kw["tol"], kw["l1_h"], kw["l2_h"], kw["l1_w"], kw["l2_w"]
    o.reserved = route << 16
    nb = int(L.evc_online_workspace_bytes(M, R, T, o.batch_size, _lib.F64))
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    per_pass = -(-T // min(o.batch_size, T))
    trace = np.zeros((o.max_iter * per_pass, 2))
    n_iter, n_steps = C.c_int(-1), C.c_int(-1)
    st = L.evc_online_learn(Xb.data_ptr(), Xb.shape[1], Wb.data_ptr(), Wb.shape[1], Hb.data_ptr(), Hb.shape[1],
                            Ab.data_ptr(), Bb.data_ptr(), Ab.shape[1], M, R, T, C.byref(o), ws.data_ptr(), nb,
                            C.byref(n_iter), C.byref(n_steps), trace.ctypes.data_as(C.POINTER(C.c_double)),
                            C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == 0
    torch.cuda.synchronize()
    outs = [t.cpu().numpy() for t in (Wb, Hb, Ab, Bb)]
    intact = all((a[:, a.shape[1] - pad:] == SENTINEL).all() for a in outs) if pad else True
    outs = [a[:, :a.shape[1] - pad] for a in outs]
    return [np.ascontiguousarray(a.T) if fm else a for a in outs] + [trace, intact, n_steps.value]


@pytest.mark.parametrize("route", [1, 2])
def test_layouts_and_padded_leading_dimensions_give_the_same_bits(route):
    import exemplars_vc_amd as evc
    d = np.load(REG)
    runs = {(lay, pad): _raw_call(d, lay, pad, route) for lay in ("bin_major", "frame_major") for pad in (0, 3)}
    ref = runs[("bin_major", 0)]
    assert ref[6] == 9
    for key, run in runs.items():
        assert run[5], key                                 # the padding of W, H, A and B keeps its sentinels
        for a, b in zip(run[:4], ref[:4]):
            assert np.array_equal(a, b), key
    W, H, info = evc.learn_dictionary_online(d["X"], d["W0"], d["H0"], layout="bin_major", info=True,
                                             route=("fused", "unfused")[route - 1], **options(d))
    assert np.array_equal(W, ref[0]) and np.array_equal(H, ref[1])
    assert np.array_equal(info["state"][0].cpu().numpy(), ref[2]) and np.array_equal(info["state"][1].cpu().numpy(), ref[3])
    close(W, d["W"], "W")
    close(H, d["H"], "H")


@pytest.mark.parametrize("route", ["fused", "unfused"])
def test_the_same_call_twice_gives_the_same_bits(route):
    import exemplars_vc_amd as evc
    d = np.load(os.path.join(GOLDEN, "online_sk_m25_r24_t300_bs100_mni_b0.npz"))
    runs = [evc.learn_dictionary_online(d["X"], d["W0"], d["H0"], layout="bin_major", info=True, route=route, **options(d))
            for _ in range(2)]
    (W1, H1, i1), (W2, H2, i2) = runs
    assert i1["n_steps"] == i2["n_steps"] == 13
    assert np.array_equal(W1, W2) and np.array_equal(H1, H2)
    for a, b in zip(i1["state"], i2["state"]):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    assert np.array_equal(i1["cost"], i2["cost"], equal_nan=True) and np.array_equal(i1["change"], i2["change"], equal_nan=True)


@pytest.mark.parametrize("path", [NO_STOP, os.path.join(GOLDEN, "online_sk_m33_r272_t300_bs96_k3_b0p5.npz")],
                         ids=os.path.basename)
def test_resume_continues_bitwise(path):
    """2 passes, then 3 from the returned state = 5 passes, with the stop rules off"""
    import exemplars_vc_amd as evc
    d = np.load(path)
    kw = dict(options(d), layout="bin_major", info=True, tol=0.0, max_no_improvement=None)
    kw.pop("max_iter")
    W5, H5, i5 = evc.learn_dictionary_online(d["X"], d["W0"], d["H0"], max_iter=5, **kw)
    W2, H2, i2 = evc.learn_dictionary_online(d["X"], d["W0"], d["H0"], max_iter=2, **kw)
    W3, H3, i3 = evc.learn_dictionary_online(d["X"], W2, H2, max_iter=3, state=i2["state"], **kw)
    assert i3["state"][0] is i2["state"][0]                 # updated in place
    assert np.array_equal(W3, W5) and np.array_equal(H3, H5) and not np.array_equal(W2, W5)
    for a, b in zip(i3["state"], i5["state"]):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())


def test_pure_enqueue_equals_the_traced_call():
    import exemplars_vc_amd as evc
    d = np.load(NO_STOP)
    kw = dict(options(d), layout="bin_major", tol=0.0, max_no_improvement=None)
    W, H = evc.learn_dictionary_online(d["X"], d["W0"], d["H0"], **kw)
    Wt, Ht, info = evc.learn_dictionary_online(d["X"], d["W0"], d["H0"], info=True, **kw)
    assert info["n_steps"] == 12 and np.isfinite(info["cost"]).all()
    assert np.array_equal(W, Wt) and np.array_equal(H, Ht)
    close(W, d["W"], "W")


def test_zero_passes_return_the_start_and_a_fresh_state():
    import exemplars_vc_amd as evc
    d = np.load(NO_STOP)
    kw = dict(options(d), layout="bin_major", info=True)
    kw["max_iter"] = 0
    W, H, info = evc.learn_dictionary_online(d["X"], d["W0"], d["H0"], **kw)
    assert np.array_equal(W, d["W0"]) and np.array_equal(H, d["H0"])
    assert info["n_steps"] == info["n_iter"] == 0 and info["cost"].shape == (0,)
    assert np.array_equal(info["state"][0].cpu().numpy(), d["W0"]) and (info["state"][1].cpu().numpy() == 1.0).all()


@pytest.mark.parametrize("layout", ["bin_major", "frame_major"])
@pytest.mark.parametrize("beta,ff", [(1.5, 0.7), (3.0, 0.3), (1.0, 1.0)])
def test_one_step(beta, ff, layout):
    """one batch, one pass: the activations are bitwise one iteration of the fixed-dictionary solve; the dictionary is
    the closed form (rho W0 + Num W0^(1/gamma)) / (rho + Den), to the gamma - not the plain multiplicative step"""
    import exemplars_vc_amd as evc
    rng = np.random.default_rng(13)
    M, R, T = 50, 24, 150
    X, W0, H0 = rng.random((M, T)) + 0.01, rng.random((M, R)) + 1e-4, rng.random((R, T)) + 1e-4
    args = [np.ascontiguousarray(a.T) for a in (X, W0, H0)] if layout == "frame_major" else [X, W0, H0]
    W, H, info = evc.learn_dictionary_online(*args, beta=beta, layout=layout, batch_size=T + 7, max_iter=1,
                                             forget_factor=ff, tol=0.0, max_no_improvement=None, info=True)
    Hs = evc.solve_activations_beta(args[1], args[0], args[2], beta=beta, layout=layout, iters=1)
    assert info["n_steps"] == info["n_iter"] == 1
    assert np.array_equal(H, Hs)
    if layout == "frame_major":
        W, H = W.T, H.T
    num, den = onr.num_den(X, W0, H, beta, S=kernel_splits(M, R)(T))
    g = onr.gamma_of(beta)
    Wc = ((ff * W0 + num * W0 ** (1 / g)) / (ff + den)) ** g          # rho = ff ** (T / T)
    if beta <= 1:
        Wc[Wc < 2.0 ** -52] = 0.0
    close(W, Wc, "W against the closed form", rtol=1e-12)
    Wr = onr.learn(X, W0, H0, beta, T + 7, 1, ff, S=kernel_splits(M, R))[0]
    close(W, Wr, "W against the restatement", rtol=1e-12)


def test_a_nan_stays_in_its_frame_until_its_batch_is_visited():
    """the NaN sits in the last batch: the activations of the batches before it and of its own batch's other frames are
    formed from a finite dictionary; the dictionary update of its batch then carries it, by design"""
    import exemplars_vc_amd as evc
    d = np.load(NO_STOP)
    X = d["X"].copy()
    X[7, 310] = np.nan
    kw = dict(options(d), layout="bin_major", tol=0.0, max_no_improvement=None, info=True)
    kw["max_iter"] = 1
    W, H, info = evc.learn_dictionary_online(X, d["W0"], d["H0"], **kw)
    others = np.ones(X.shape[1], dtype=bool)
    others[310] = False
    assert np.isfinite(H[:, others]).all() and np.isnan(H[:, 310]).all()
    assert np.isnan(W).any()
    assert info["n_steps"] == 4 and np.isfinite(info["cost"][:3]).all() and np.isnan(info["cost"][3])
    # ... and the same run without the NaN, up to the visit: the first three batches' activations are bitwise the same
    _, Hc, _ = evc.learn_dictionary_online(d["X"], d["W0"], d["H0"], **kw)
    assert np.array_equal(H[:, :300], Hc[:, :300])


@pytest.mark.parametrize("name", ["online_sk_m25_r24_t300_bs100_mni_b3", "online_sk_m25_r24_t300_bs100_k3_reg_b1p5"])
def test_the_sklearn_mirror(name):
    from exemplars_vc_amd.compat.factorize import non_negative_factorization_minibatch
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    mni = int(d["max_no_improvement"])
    Wsk, Hsk, n_iter, n_steps = non_negative_factorization_minibatch(
        np.ascontiguousarray(d["X"].T), np.ascontiguousarray(d["H0"].T), np.ascontiguousarray(d["W0"].T),
        beta_loss=float(d["beta"]), batch_size=int(d["batch_size"]), max_iter=int(d["max_iter"]), tol=float(d["tol"]),
        max_no_improvement=None if mni < 0 else mni, forget_factor=float(d["forget_factor"]), alpha_W=float(d["alpha"]),
        l1_ratio=float(d["l1_ratio"]))
    assert (n_iter, n_steps) == (int(d["n_iter"]), int(d["n_steps"]))
    assert Wsk.shape == d["H"].T.shape and Hsk.shape == d["W"].T.shape
    close(Hsk.T, d["W"], "W")
    close(Wsk.T, d["H"], "H")


def _rank16(seed=3):
    """test_gpu_learn_kl._rank16"""
    rng = np.random.default_rng(seed)
    Wa, Wb = rng.random((25, 16)) + 0.05, rng.random((25, 16)) + 0.05
    G = rng.random((16, 300)) * (rng.random((16, 300)) < 0.4) + 1e-3
    return Wa @ G, Wb @ G


@pytest.mark.parametrize("beta", [None, 0])
@pytest.mark.parametrize("layout", ["bin_major", "frame_major"])
def test_compact_dictionary_online(layout, beta):
    import exemplars_vc_amd as evc
    A, B = _rank16()
    fm = layout == "frame_major"
    args = (np.ascontiguousarray(A.T), np.ascontiguousarray(B.T)) if fm else (A, B)
    Wa, Wb, G, info = evc.compact_dictionary(*args, 16, iters=3, layout=layout, batch_size=128, beta=beta)
    if fm:
        Wa, Wb, G = Wa.T, Wb.T, G.T
    assert Wa.shape == (25, 16) and Wb.shape == (25, 16) and G.shape == (16, 300)
    for F in (Wa, Wb, G):
        assert np.isfinite(F).all() and (F >= 0).all()
    assert info["n_iter"] == 3 and info["n_steps"] == 9
    D = np.vstack([A, B])
    W0 = np.maximum(D[:, (np.arange(16) * 300) // 16], 1e-6)
    G0 = np.full((16, 300), np.sqrt(D.mean() / 16))
    b = 2.0 if beta is None else float(beta)
    Wr, Gr = onr.learn(D, W0, G0, b, 128, 3, 0.7, S=kernel_splits(50, 16))[:2]
    close(np.vstack([Wa, Wb]), Wr, "W")
    close(G, Gr, "G")
    assert np.linalg.norm(D - np.vstack([Wa, Wb]) @ G) < np.linalg.norm(D - W0 @ G0)
    assert onr.raw_divergence(D, np.vstack([Wa, Wb]), G, b) < onr.raw_divergence(D, W0, G0, b)


# sha256 of (Wa, Wb, G) this call returned before compact_dictionary gained batch_size (float64, bin-major)
PARENT_DIGEST = "ea76d5dbf2c67742333ee69f868bcadca34b837a883f259ece9c38ff25d790ff"


def test_compact_dictionary_without_batch_size_is_bitwise_unchanged():
    import exemplars_vc_amd as evc
    A, B = _rank16()
    Wa, Wb, G, info = evc.compact_dictionary(A, B, 16, iters=20)
    h = hashlib.sha256()
    for F in (Wa, Wb, G):
        h.update(np.ascontiguousarray(F, dtype=np.float64).tobytes())
    print("digest", h.hexdigest())
    assert info["n_iter"] == 20 and h.hexdigest() == PARENT_DIGEST
