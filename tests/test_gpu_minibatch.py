"""The mini-batch estimator's activation solve (evc_online_transform: the change variant of k_beta_sweep and
k_beta_change_check), its fit with fresh restarts and partial_fit (evc_online_learn_fresh) and the MiniBatchNMF mirror on the
GPU against scikit-learn's recorded runs (tests/golden/mbnmf_{tr,fr,pf}_*.npz, tools/make_golden_minibatch.py) and the
numpy restatement (tests/minibatch_restatement.py).

Tolerances are the project's own: the activations under test_gpu_beta.py's predicates (float64 relative 1e-9 on the entries
the reference has non-zero, zeros exact; float32 norm-relative 1e-4), the ratios under test_gpu_online.close_change's (the
activations before and after an update are each held to `held` relative, so their ratio moves by at most 4 held + 10 held
ratio).  The counts are exact: every recorded decision is clear of tol by 1e-6 (float64) / 1e-2 (float32) relative."""
import functools
import glob
import hashlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import minibatch_restatement as mr  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "mbnmf_tr_*.npz")))
FR_FILES = sorted(glob.glob(os.path.join(GOLDEN, "mbnmf_fr_*.npz")))
PF_FILES = sorted(glob.glob(os.path.join(GOLDEN, "mbnmf_pf_*.npz")))

pytestmark = pytest.mark.gpu


def close(got, ref, what):
    """test_gpu_beta.close64 / its float32 bound; prints the figure before asserting"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    if ref.dtype == np.float32:
        r = float(np.linalg.norm(got.astype(np.float64) - ref) / np.linalg.norm(ref))
        print(f"{what}: float32 norm-relative error {r:.3e}")
        assert r <= 1e-4, (what, r)
        return
    nz = ref != 0
    worst = float(np.max(np.abs(got[nz] - ref[nz]) / np.abs(ref[nz]))) if nz.any() else 0.0
    print(f"{what}: worst relative deviation {worst:.3e}, zeros kept {bool((got[~nz] == 0).all())}")
    assert (got[~nz] == 0).all() and worst <= 1e-9, (what, worst)


def close_change(got, want, held):
    """test_gpu_online.close_change"""
    got, want = np.asarray(got), np.asarray(want)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok])
    print("change: max error", float(err.max()) if err.size else 0.0)
    assert (err <= 4 * held + 10 * held * want[ok]).all()


def _reg(d):
    M = d["X"].shape[0]
    a, r = float(d["alpha"]), float(d["l1_ratio"])
    return M * a * r, M * a * (1 - r)


def transform(W, X, **kw):
    import exemplars_vc_amd as evc
    kw.setdefault("layout", "bin_major")
    return evc.transform_online(W, X, info=True, **kw)


def test_there_are_fixtures():
    assert (len(FILES), len(FR_FILES), len(PF_FILES)) == (15, 6, 3)


@pytest.mark.parametrize("path", FILES, ids=os.path.basename)
def test_fixture(path):
    d = np.load(path)
    X, W, K, n_ref = d["X"], d["W"], int(d["max_iter"]), int(d["n_iter"])
    l1, l2 = _reg(d)
    H, info = transform(W, X, beta=float(d["beta"]), max_iter=K, tol=float(d["tol"]), l1=l1, l2=l2)
    assert info["kernel"] == "k_beta_sweep<change>" and info["n_iter"].tolist() == [n_ref]
    close(H, d["H"], "H")
    want = np.full((1, K), np.nan)
    want[0, :n_ref] = d["change"]
    close_change(info["change"], want, 1e-9 if X.dtype == np.float64 else 1e-4)
    Ht, it = transform(np.ascontiguousarray(W.T), np.ascontiguousarray(X.T), layout="frame_major", beta=float(d["beta"]),
                       max_iter=K, tol=float(d["tol"]), l1=l1, l2=l2)
    assert np.array_equal(Ht.T, H) and np.array_equal(it["change"], info["change"], equal_nan=True)     # the other layout
    # the mirror: the same call underneath
    from exemplars_vc_amd.compat.minibatch import MiniBatchNMF
    beta = float(d["beta"])
    est = MiniBatchNMF(W.shape[1], init="custom", beta_loss=beta if beta else "itakura-saito", tol=float(d["tol"]), max_iter=0,
                       transform_max_iter=K, alpha_W=float(d["alpha"]), l1_ratio=float(d["l1_ratio"]))
    est.fit(np.ascontiguousarray(X.T), W=np.ones((X.shape[1], W.shape[1]), dtype=X.dtype), H=np.ascontiguousarray(W.T))
    assert est.n_iter_ == 0 and np.array_equal(est.components_, W.T)       # no passes: the dictionary as given
    assert np.array_equal(est.transform(np.ascontiguousarray(X.T)).T, H)


@pytest.mark.parametrize("name,K", [("mbnmf_tr_m25_r24_t70_tol_b0p5", 7), ("mbnmf_tr_m33_r272_t50_tol_b2", 5),
                                    ("mbnmf_tr_m201_r32_t40_tol_b0", 4), ("mbnmf_tr_m25_r24_t70_tol_f32_b1p5", 7)])
def test_without_tol_bitwise_the_beta_solve(name, K):
    """tol = 0: the change variant stores what the plain sweep stores - both layouts, padded leading dimensions, twice"""
    import torch
    import exemplars_vc_amd as evc
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    X, W, beta = d["X"], d["W"], float(d["beta"])
    (M, T), R = X.shape, W.shape[1]
    ref = evc.solve_activations_beta(W, X, beta=beta, init="sklearn", iters=K, layout="bin_major")
    H, info = transform(W, X, beta=beta, max_iter=K, tol=0.0)
    assert np.array_equal(H, ref) and info["n_iter"].tolist() == [K] and np.isfinite(info["change"]).all()
    H2, info2 = transform(W, X, beta=beta, max_iter=K, tol=0.0)
    assert np.array_equal(H2, H) and np.array_equal(info2["change"], info["change"])
    dev = evc.require_device()

    def padded(a, extra):
        t = torch.full((a.shape[0], a.shape[1] + extra), -7.0, dtype=torch.from_numpy(a).dtype, device=dev)
        t[:, :a.shape[1]] = torch.from_numpy(a).to(dev)
        return t[:, :a.shape[1]], t
    for layout, Wl, Xl, hshape in (("bin_major", W, X, (R, T)), ("frame_major", W.T, X.T, (T, R))):
        Wl, Xl = np.ascontiguousarray(Wl), np.ascontiguousarray(Xl)
        out, base = padded(np.zeros(hshape, dtype=X.dtype), 5)
        Hd, infod = transform(padded(Wl, 3)[0], padded(Xl, 9)[0], beta=beta, max_iter=K, tol=0.0, layout=layout, out=out)
        Hd = Hd.cpu().numpy()
        assert np.array_equal(Hd if layout == "bin_major" else Hd.T, ref)
        assert np.array_equal(infod["change"], info["change"])
        assert (base[:, hshape[1]:] == -7.0).all()          # nothing written into the padding


@functools.lru_cache(maxsize=None)
def _ragged():
    """three utterances that stop at 40, 37 and 44 (margins >= 3e-3 at tol = 1e-2, the fixture's) and an empty one"""
    d = np.load(os.path.join(GOLDEN, "mbnmf_tr_m25_r24_t70_tol_b0p5.npz"))
    X, W = d["X"], d["W"]
    utts = [X[:, :30].copy(), X[:, 30:30].copy(), X[:, 30:50] * np.linspace(0.2, 5, 20)[None, :], X[:, 50:70] ** 2 + 0.3]
    offs = np.concatenate([[0], np.cumsum([u.shape[1] for u in utts])])
    kw = dict(beta=0.5, max_iter=60, tol=float(d["tol"]))
    return W, utts, offs, kw, mr.transform(np.concatenate(utts, axis=1), W, 0.5, 60, kw["tol"], utt_offsets=offs)


def test_ragged_batch_is_bitwise_the_solo_transforms():
    W, utts, offs, kw, (Hr, nr, cr) = _ragged()
    assert nr.tolist() == [40, 60, 37, 44]
    H, info = transform(W, np.concatenate(utts, axis=1), utt_offsets=offs, **kw)
    assert info["n_iter"].tolist() == nr.tolist() and np.isnan(info["change"][1]).all()      # the empty one: nothing ran
    close(H, Hr, "batch against the restatement")
    close_change(info["change"], cr, 1e-9)
    for u in (0, 2, 3):
        solo, si = transform(W, utts[u], **kw)
        assert np.array_equal(H[:, offs[u]:offs[u + 1]], solo)
        assert si["n_iter"][0] == info["n_iter"][u] and np.array_equal(si["change"][0], info["change"][u], equal_nan=True)


def test_a_nan_stays_in_its_utterance_which_runs_to_max_iter():
    W, utts, offs, kw, _ = _ragged()
    X = np.concatenate(utts, axis=1)
    H, info = transform(W, X, utt_offsets=offs, **kw)
    Xn = X.copy()
    Xn[3, offs[2] + 4] = np.nan
    Hn, infon = transform(W, Xn, utt_offsets=offs, **kw)
    assert infon["n_iter"].tolist() == [40, 60, 60, 44] and np.isnan(infon["change"][2]).all()
    keep = np.r_[0:offs[2], offs[3]:offs[4]]
    assert np.array_equal(Hn[:, keep], H[:, keep]) and np.isnan(Hn[:, offs[2]:offs[3]]).all()
    for u in (0, 3):
        assert np.array_equal(infon["change"][u], info["change"][u], equal_nan=True)
    # a given start keeps the NaN in its frame's column; the utterance's ratio is NaN and never stops it
    H0 = np.full((W.shape[1], X.shape[1]), 0.1)
    Hg, infog = transform(W, Xn, H0=H0, utt_offsets=offs, **kw)
    Hc, _ = transform(W, X, H0=H0, utt_offsets=offs, **dict(kw, tol=0.0))
    col = offs[2] + 4
    assert infog["n_iter"][2] == 60 and np.isnan(Hg[:, col]).all() and np.isfinite(np.delete(Hg, col, axis=1)).all()
    others = np.delete(np.arange(offs[2], offs[3]), 4)
    assert np.array_equal(Hg[:, others], Hc[:, others])


def test_pure_enqueue_equals_the_traced_call_and_no_iterations_return_the_start():
    import exemplars_vc_amd as evc
    W, utts, offs, kw, _ = _ragged()
    X = np.concatenate(utts, axis=1)
    H, _ = transform(W, X, utt_offsets=offs, **kw)
    assert np.array_equal(evc.transform_online(W, X, layout="bin_major", utt_offsets=offs, **kw), H)
    H0, info = transform(W, X, utt_offsets=offs, **dict(kw, max_iter=0))
    assert info["n_iter"].tolist() == [0, 0, 0, 0] and info["change"].shape == (4, 0)
    for u in (0, 2, 3):
        np.testing.assert_allclose(H0[:, offs[u]:offs[u + 1]], np.sqrt(utts[u].mean() / W.shape[1]), rtol=1e-13, atol=0)


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


# recorded with the library of the commit before evc_online_transform, through the same two calls
PARENT = {"beta_solve": "a7830be1aeae1646065cc098bc617649f0555adb8d68dc4c5be36e78f5c85f6c",
          "online_learn": "f5e537de12e1fa54c61afe1e1d5bf5b57750e4f7fbb8a4183fb01fff8d9adc8c"}


def existing_paths():
    import exemplars_vc_amd as evc
    d = np.load(os.path.join(GOLDEN, "betamu_m25_n64_t50_b0_tol2e-2.npz"))
    H, info = evc.solve_activations_beta(d["W_rows"], d["X_rows"], beta=0.0, layout="frame_major", iters=150, check_every=10,
                                         stop_rule="sklearn", tol=2e-2, info=True)
    out = {"beta_solve": _sha(H, info["n_iter"], np.nan_to_num(info["err"], nan=-1.0))}
    d = np.load(os.path.join(GOLDEN, "online_sk_m25_r24_t330_bs100_k3_b1p5.npz"))
    W, H, info = evc.learn_dictionary_online(d["X"], d["W0"], d["H0"], beta=1.5, layout="bin_major", batch_size=100,
                                             max_iter=3, tol=0.0, max_no_improvement=None, info=True)
    out["online_learn"] = _sha(W, H, np.nan_to_num(info["cost"], nan=-1.0), np.nan_to_num(info["change"], nan=-1.0),
                               info["state"][0].cpu().numpy(), info["state"][1].cpu().numpy())
    return out


def test_the_existing_paths_are_bitwise_what_the_parent_gave():
    assert existing_paths() == PARENT


# ---- the fit with fresh restarts, partial_fit and the estimator (evc_online_learn_fresh) ----
def fresh_options(d):
    import test_gpu_online as tgo
    return dict(tgo.options(d), fresh_restarts=True, fresh_restarts_max_iter=int(d["fresh_max_iter"]),
                transform_max_iter=int(d["final_max_iter"]))


@functools.lru_cache(maxsize=None)
def fresh_slack(path):
    """test_gpu_online.restate's slack per frame of every step, from the fresh-restart restatement"""
    import test_gpu_online as tgo
    d = np.load(path)
    kw = tgo.options(d)
    beta, slack = kw.pop("beta"), []
    X = np.asarray(d["X"], dtype=np.float64)
    mr.learn_fresh(d["X"], d["W0"], beta, kw.pop("batch_size"), kw.pop("max_iter"), fresh_max_iter=int(d["fresh_max_iter"]),
                   final_max_iter=0, dtype=np.dtype(str(d["dtype"])),
                   on_step=lambda k, t0, t1, W, Hb: slack.append(tgo._slack(X[:, t0:t1], W.astype(float), Hb.astype(float),
                                                                            beta) / (t1 - t0)), **kw)
    return np.array(slack)


@pytest.mark.parametrize("route", [None, "fused", "unfused"])
@pytest.mark.parametrize("path", FR_FILES, ids=os.path.basename)
def test_fresh_fixture(path, route):
    import exemplars_vc_amd as evc
    import test_gpu_online as tgo
    d = np.load(path)
    T = d["X"].shape[1]
    W, H, info = evc.learn_dictionary_online(d["X"], d["W0"], None, layout="bin_major", info=True, route=route,
                                             **fresh_options(d))
    assert info["n_steps"] == int(d["n_steps"]) and info["n_iter"] == int(d["n_iter"])
    tgo.close(W, d["W"], "W")
    tgo.close(H, d["H"], "H")
    n, per_pass = info["n_steps"], -(-T // min(int(d["batch_size"]), T))
    assert info["cost"].shape == info["change"].shape == (int(d["max_iter"]) * per_pass,)
    want_cost, want_change = np.full(info["cost"].shape, np.nan), np.full(info["cost"].shape, np.nan)
    want_cost[:n], want_change[:n] = d["cost"], d["change"]
    held = 1e-9 if d["X"].dtype == np.float64 else 1e-4
    tgo.close_cost(info["cost"], want_cost, fresh_slack(path), held)
    tgo.close_change(info["change"], want_change, held)
    if route is not None:
        return
    # the caller's H start is ignored, and the call repeats bitwise
    W2, H2, i2 = evc.learn_dictionary_online(d["X"], d["W0"], np.full(d["H"].shape, 7.0, dtype=d["X"].dtype), layout="bin_major",
                                             info=True, **fresh_options(d))
    assert np.array_equal(W2, W) and np.array_equal(H2, H) and np.array_equal(i2["cost"], info["cost"], equal_nan=True)
    # the mirror
    from exemplars_vc_amd.compat.minibatch import MiniBatchNMF
    beta, mni = float(d["beta"]), int(d["max_no_improvement"])
    est = MiniBatchNMF(W.shape[1], init="custom", batch_size=int(d["batch_size"]), beta_loss=beta if beta else "itakura-saito",
                       tol=float(d["tol"]), max_no_improvement=None if mni < 0 else mni, max_iter=int(d["max_iter"]),
                       forget_factor=float(d["forget_factor"]), fresh_restarts=True,
                       fresh_restarts_max_iter=int(d["fresh_max_iter"]), transform_max_iter=int(d["final_max_iter"]))
    Wsk = est.fit_transform(np.ascontiguousarray(d["X"].T), H=np.ascontiguousarray(d["W0"].T))
    assert (est.n_iter_, est.n_steps_, est.n_components_, est.n_features_in_) == (int(d["n_iter"]), n, W.shape[1], W.shape[0])
    frame_major = evc.learn_dictionary_online(np.ascontiguousarray(d["X"].T), np.ascontiguousarray(d["W0"].T), None,
                                              layout="frame_major", **fresh_options(d))
    assert np.array_equal(est.components_, frame_major[0]) and np.array_equal(Wsk, frame_major[1])
    tgo.close(est.components_.T, d["W"], "components_")
    tgo.close(Wsk.T, d["H"], "fit_transform")
    import beta_restatement as br
    want = br.beta_divergence(d["X"].T.astype(np.float64), d["H"].T.astype(np.float64), d["W"].T.astype(np.float64), beta)
    print("reconstruction_err_", est.reconstruction_err_, want)
    assert abs(est.reconstruction_err_ - want) <= (1e-7 if held == 1e-9 else 1e-3) * want
    np.testing.assert_allclose(est.inverse_transform(Wsk), Wsk @ est.components_)


def test_the_step_flushes_after_its_solve_not_during_it():
    """beta < 1 with silent frames: their activations fall below 2^-52 inside the solve and are stored as 0 afterwards; with
    final_max_iter = 0 the steps' activations are what the call returns (scikit-learn's own fit overwrites them, so no
    recorded run can show this)"""
    import exemplars_vc_amd as evc
    d = np.load(os.path.join(GOLDEN, "mbnmf_fr_m25_r24_t330_bs100_k2_b1p5.npz"))
    X = d["X"].copy()
    X[:, [5, 117, 118, 329]] = 1e-30
    kw = dict(beta=0.5, batch_size=100, max_iter=1, tol=0.0, max_no_improvement=None)
    Wr, Hr, _, _, _, _, _, _ = mr.learn_fresh(X, d["W0"], 0.5, 100, 1, fresh_max_iter=8, final_max_iter=0)
    W, H = evc.learn_dictionary_online(X, d["W0"], None, layout="bin_major", fresh_restarts=True, fresh_restarts_max_iter=8,
                                       transform_max_iter=0, **kw)
    assert (Hr[:, [5, 117, 118, 329]] == 0).all() and (Hr == 0).sum() == 4 * 24 and np.isfinite(Wr).all()
    close(H, Hr, "H with its flushed columns")
    close(W, Wr, "W")


@pytest.mark.parametrize("path", PF_FILES, ids=os.path.basename)
def test_partial_fit_sequence(path):
    from exemplars_vc_amd.compat.minibatch import MiniBatchNMF
    d = np.load(path)
    beta, o = float(d["beta"]), d["offsets"]
    chunks = [np.ascontiguousarray(d["X"][:, a:b].T) for a, b in zip(o[:-1], o[1:])]

    def estimator():
        return MiniBatchNMF(24, init="custom", batch_size=int(d["batch_size"]), beta_loss=beta, tol=float(d["tol"]),
                            forget_factor=float(d["forget_factor"]), fresh_restarts_max_iter=int(d["fresh_max_iter"]),
                            alpha_W=float(d["alpha"]), l1_ratio=float(d["l1_ratio"]))
    est = estimator()
    seen = []
    for c, X in enumerate(chunks):
        est.partial_fit(X, H=np.ascontiguousarray(d["W0"].T)) if c == 0 else est.partial_fit(X)
        assert est.n_steps_ == c + 1 and est._rho == float(d["rho"]) != float(d["forget_factor"])
        A, B = (t.cpu().numpy() for t in est._state)
        seen.append((est.components_, A, B))
        close(est.components_.T, d[f"W_{c}"], f"components_ after chunk {c}")
        close(A.T, d[f"A_{c}"], f"A after chunk {c}")
        close(B.T, d[f"B_{c}"], f"B after chunk {c}")
    again = estimator()                      # a fresh estimator given the same chunks: the same bits
    for c, X in enumerate(chunks[:2]):
        again.partial_fit(X, H=np.ascontiguousarray(d["W0"].T)) if c == 0 else again.partial_fit(X)
        assert np.array_equal(again.components_, seen[c][0])
        assert all(np.array_equal(t.cpu().numpy(), s) for t, s in zip(again._state, seen[c][1:]))


def test_one_partial_fit_is_one_fresh_step_bitwise():
    import exemplars_vc_amd as evc
    from exemplars_vc_amd.compat.minibatch import MiniBatchNMF
    d = np.load(PF_FILES[0])
    X, W0 = np.ascontiguousarray(d["X"].T), np.ascontiguousarray(d["W0"].T)
    est = MiniBatchNMF(24, init="custom", batch_size=1 << 20, beta_loss=float(d["beta"]), tol=float(d["tol"]),
                       fresh_restarts_max_iter=int(d["fresh_max_iter"])).partial_fit(X, H=W0)
    W, H, info = evc.learn_dictionary_online(X, W0, None, beta=float(d["beta"]), layout="frame_major", batch_size=X.shape[0],
                                             max_iter=1, tol=float(d["tol"]), max_no_improvement=None, fresh_restarts=True,
                                             fresh_restarts_max_iter=int(d["fresh_max_iter"]), transform_max_iter=0, info=True)
    assert info["n_steps"] == 1 and np.array_equal(est.components_, W)
    assert all(np.array_equal(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(est._state, info["state"]))


def test_fresh_pure_enqueue_equals_the_traced_call():
    import exemplars_vc_amd as evc
    d = np.load(os.path.join(GOLDEN, "mbnmf_fr_m25_r24_t330_bs100_k2_b1p5.npz"))
    kw = dict(beta=1.5, layout="bin_major", batch_size=100, max_iter=2, tol=0.0, max_no_improvement=None, fresh_restarts=True,
              fresh_restarts_max_iter=5, transform_max_iter=6)
    W, H, info = evc.learn_dictionary_online(d["X"], d["W0"], None, info=True, **kw)
    Wq, Hq = evc.learn_dictionary_online(d["X"], d["W0"], None, **kw)
    assert info["n_steps"] == 8 and np.array_equal(Wq, W) and np.array_equal(Hq, H)
