"""Golden vectors of the mini-batch estimator's activation solve (evc_online_transform), of its fit with fresh restarts
and of partial_fit (evc_online_learn_fresh).

scikit-learn 1.7.2, `MiniBatchNMF(n_components=R, init='custom', beta_loss=beta, tol=tol, transform_max_iter=K,
alpha_W=alpha, alpha_H='same', l1_ratio=l1_ratio).transform(X)` with `components_` set to the dictionary, through a
recording subclass that overrides `_solve_W` statement for statement and stores every iteration's
||W - W_buffer|| / ||W|| (scikit-learn's W is our H^T, its H is our W^T).  The fixtures store the bin-major orientation:
X (M, T), W (M, R), H (R, T), plus n_iter (the iteration the solve stopped at, or max_iter), change (one entry per iteration
carried out), max_iter, tol, beta, alpha, l1_ratio, dtype and margin.

X and W are make_golden_online.synth's X and W0.  Every case asserts, for scikit-learn alone, that every iteration's
decision (ratio <= tol) is away from its threshold by a relative make_golden_online.MARGIN[dtype] or more, and that no
positive entry of the result lies within a factor 1 +- 1e-3 of 2^-52.

mbnmf_fr_*: `MiniBatchNMF(..., fresh_restarts=True, fresh_restarts_max_iter=F, transform_max_iter=K2).fit_transform(X,
W=H0, H=W0)` through make_golden_online's recording subclass with the same `_solve_W` override: make_golden_online's keys
(W0, W, H, n_iter, n_steps, cost, change, batch_size, ...) plus fresh_max_iter and final_max_iter; no H0 (fresh restarts
ignore it).  The margin covers every ratio of every activation solve as well as every decision of the fit.
mbnmf_pf_*: three consecutive `partial_fit` chunks of unequal length, the first longer than batch_size so that rho =
forget_factor ** (batch_size / T_0) differs from forget_factor: X, W0, offsets (the chunks' frame ranges), rho, and per chunk c
W_c (components_), A_c, B_c (the statistics) after it.

Writes tests/golden/mbnmf_{tr,fr,pf}_*.npz; the prefix keeps them out of every other test's glob.

    python tools/make_golden_minibatch.py [--check] [name ...]     (--check: recompute and compare instead of writing)
"""
import os
import sys
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_online as mgo  # noqa: E402
from make_golden_online import E64, GOLDEN, MARGIN, synth  # noqa: E402


def recorder():
    from scipy import linalg
    from sklearn.decomposition._nmf import _multiplicative_update_w

    class Recording(mgo.recorder()):
        """_solve_W as scikit-learn has it, plus the list of the ratios it compares with tol (solve_changes_: the last solve's;
        solve_margins_: every solve's distances from tol)"""

        def _solve_W(self, X, H, max_iter):
            avg = np.sqrt(X.mean() / self._n_components)
            W = np.full((X.shape[0], self._n_components), avg, dtype=X.dtype)
            W_buffer = W.copy()
            l1_reg_W, _, l2_reg_W, _ = self._compute_regularization(X)
            self.solve_changes_ = []
            if not hasattr(self, "solve_margins_"):
                self.solve_margins_, self.solve_iters_ = [], []
            for _ in range(max_iter):
                W, *_ = _multiplicative_update_w(X, W, H, self._beta_loss, l1_reg_W, l2_reg_W, self._gamma)
                W_diff = linalg.norm(W - W_buffer) / linalg.norm(W)
                self.solve_changes_.append(float(W_diff))
                if self.tol > 0:
                    self.solve_margins_.append(abs(float(W_diff) - self.tol) / self.tol)
                if self.tol > 0 and W_diff <= self.tol:
                    break
                W_buffer[:] = W
            self.solve_iters_.append(len(self.solve_changes_))
            return W
    return Recording


def run_fresh(X, W0, beta, bs, K, tol, mni, ff, fresh, final, alpha=0.0, l1_ratio=0.0):
    """bin-major in, bin-major out: (W, H, n_iter, n_steps, cost, change, smallest margin, iterations of every solve)"""
    est = recorder()(n_components=W0.shape[1], init="custom", batch_size=bs, beta_loss=beta, tol=tol, max_iter=K,
                     max_no_improvement=mni, forget_factor=ff, alpha_W=alpha, alpha_H="same", l1_ratio=l1_ratio,
                     fresh_restarts=True, fresh_restarts_max_iter=fresh, transform_max_iter=final)
    H_any = np.full((X.shape[1], W0.shape[1]), 0.5, dtype=X.dtype)       # ignored by fresh restarts
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        Wsk = est.fit_transform(np.ascontiguousarray(X.T), W=H_any, H=np.ascontiguousarray(W0.T))
    n = int(est.n_steps_)
    margin = min(est.margins_ + est.solve_margins_) if est.margins_ + est.solve_margins_ else np.inf
    return (np.ascontiguousarray(est.components_.T), np.ascontiguousarray(Wsk.T), int(est.n_iter_), n,
            np.array(est.costs_), np.array(est.changes_), margin, np.array(est.solve_iters_))


def run_partial(X, W0, offsets, beta, bs, ff, tol, fresh, alpha=0.0, l1_ratio=0.0):
    """three partial_fit calls: per chunk (components_, A, B), plus rho, the margin and every solve's iterations"""
    est = recorder()(n_components=W0.shape[1], init="custom", batch_size=bs, beta_loss=beta, tol=tol, forget_factor=ff,
                     alpha_W=alpha, alpha_H="same", l1_ratio=l1_ratio, fresh_restarts_max_iter=fresh)
    Xs = np.ascontiguousarray(X.T)
    out = []
    for a, b in zip(offsets[:-1], offsets[1:]):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            if not out:         # init='custom' wants a W, which partial_fit then ignores
                est.partial_fit(Xs[a:b], W=np.full((b - a, W0.shape[1]), 0.5), H=np.ascontiguousarray(W0.T))
            else:
                est.partial_fit(Xs[a:b])
        out.append((np.ascontiguousarray(est.components_.T), np.ascontiguousarray(est._components_numerator.T),
                    np.ascontiguousarray(est._components_denominator.T)))
    margin = min(est.solve_margins_) if est.solve_margins_ else np.inf
    return out, float(est._rho), margin, np.array(est.solve_iters_)


def run_sklearn(X, W, beta, K, tol, alpha=0.0, l1_ratio=0.0):
    """bin-major in, bin-major out: (H, n_iter, change, smallest decision margin)"""
    Xs, comp = np.ascontiguousarray(X.T), np.ascontiguousarray(W.T)
    est = recorder()(n_components=W.shape[1], init="custom", beta_loss=beta, tol=tol, transform_max_iter=K, alpha_W=alpha,
                     alpha_H="same", l1_ratio=l1_ratio)
    est._check_params(Xs)
    est.components_, est.n_components_, est.n_features_in_ = comp, comp.shape[0], comp.shape[1]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        Hs = est.transform(Xs)
    change = np.array(est.solve_changes_)
    margin = float(np.min(np.abs(change - tol) / tol)) if tol > 0 else np.inf
    return np.ascontiguousarray(Hs.T), len(change), change, margin


def cases():
    """name -> dict(M, R, T, seed, K, beta, tol, dtype, alpha, l1_ratio, stop); stop: whether tol must end the solve"""
    def c(M, R, T, beta, K=200, tol=1e-2, dtype=np.float64, alpha=0.0, l1_ratio=0.0, stop=True, seed=801):
        return dict(M=M, R=R, T=T, seed=seed, K=K, beta=beta, tol=tol, dtype=dtype, alpha=alpha, l1_ratio=l1_ratio, stop=stop)
    d = {}
    # M, R and T no multiples of 16; every beta
    for tag, beta in (("b2", 2.0), ("b1", 1.0), ("b0", 0.0), ("b0p5", 0.5), ("b1p5", 1.5), ("b3", 3.0)):
        d[f"mbnmf_tr_m25_r24_t70_tol_{tag}"] = c(25, 24, 70, beta)
    # several exemplar tiles per wavefront
    d["mbnmf_tr_m33_r272_t50_tol_b0p5"] = c(33, 272, 50, 0.5)
    d["mbnmf_tr_m33_r272_t50_tol_b2"] = c(33, 272, 50, 2.0)
    # two passes of phase 1
    d["mbnmf_tr_m201_r32_t40_tol_b0"] = c(201, 32, 40, 0.0)
    d["mbnmf_tr_m201_r32_t40_tol_b1p5"] = c(201, 32, 40, 1.5)
    # tol never reached: every iteration's ratio is compared and the solve runs its full count
    d["mbnmf_tr_m25_r24_t70_k60_b2"] = c(25, 24, 70, 2.0, K=60, tol=1e-3, stop=False)
    d["mbnmf_tr_m201_r32_t40_k40_b0p5"] = c(201, 32, 40, 0.5, K=40, tol=1e-3, stop=False)
    d["mbnmf_tr_m25_r24_t70_tol_reg_b1p5"] = c(25, 24, 70, 1.5, alpha=1e-3, l1_ratio=0.5)
    d["mbnmf_tr_m25_r24_t70_tol_f32_b2"] = c(25, 24, 70, 2.0, dtype=np.float32)
    d["mbnmf_tr_m25_r24_t70_tol_f32_b1p5"] = c(25, 24, 70, 1.5, dtype=np.float32)
    return d


def cases_fresh():
    """name -> dict(M, R, T, bs, seed, K, beta, tol, mni, ff, fresh, final, dtype, flush, stop ("tol" | "mni" | None))"""
    def c(T, K, beta, tol=0.0, mni=None, fresh=8, final=10, seed=811, dtype=np.float64, flush=False, stop=None, ff=0.7):
        return dict(M=25, R=24, T=T, bs=100, seed=seed, K=K, beta=beta, tol=tol, mni=mni, ff=ff, fresh=fresh, final=final,
                    dtype=dtype, flush=flush, stop=stop)
    d = {}
    d["mbnmf_fr_m25_r24_t300_bs100_k2_b2"] = c(300, 2, 2.0)                              # every solve runs its full count
    d["mbnmf_fr_m25_r24_t330_bs100_k2_b1p5"] = c(330, 2, 1.5, tol=1e-4, fresh=12)         # short last batch, second tile table
    d["mbnmf_fr_m25_r24_t300_bs100_tol_b0p5"] = c(300, 20, 0.5, tol=3e-2, fresh=30, final=40, stop="tol")
    d["mbnmf_fr_m25_r24_t300_bs100_mni_b0"] = c(300, 20, 0.0, mni=1, stop="mni")
    # beta < 1 with ~4 % of W0 seeded at 1e-19.  The solve that ends scikit-learn's fit overwrites the steps' flushed
    # activations, and a flushed entry differs from its unflushed value by less than 2^-52 in every sum it enters, so what
    # scikit-learn returns here holds no zeros and the kernels must leave none either; the flush itself is checked against
    # the restatement with final_max_iter = 0 (tests/test_gpu_minibatch.py).
    d["mbnmf_fr_m25_r24_t330_bs100_k2_flush_b0p5"] = c(330, 2, 0.5, flush=True)
    d["mbnmf_fr_m25_r24_t300_bs100_k2_f32_b2"] = c(300, 2, 2.0, dtype=np.float32)
    return d


def make_fresh(name, s):
    X, W0, _ = synth(s["M"], s["R"], s["T"], s["seed"])
    if s["flush"]:      # ~4 % of W0 far below the flush threshold
        rng = np.random.default_rng(s["seed"] + 1000)
        W0[rng.random(W0.shape) < 0.04] = 1e-19
    dt = np.dtype(s["dtype"])
    X, W0 = X.astype(dt), W0.astype(dt)
    W, H, n_iter, n_steps, cost, change, margin, solves = run_fresh(X, W0, s["beta"], s["bs"], s["K"], s["tol"], s["mni"], s["ff"],
                                                                    s["fresh"], s["final"])
    per_pass = -(-s["T"] // s["bs"])
    assert margin >= MARGIN[dt.name], (name, margin)
    assert solves.max() <= 140 and len(solves) == n_steps + 1, (name, solves)
    if s["stop"] is None:
        assert n_steps == s["K"] * per_pass, (name, n_steps)
    else:
        assert 2 < n_steps < s["K"] * per_pass, (name, n_steps)
        assert (change[-1] <= s["tol"]) == (s["stop"] == "tol"), (name, change[-1])
    for F in (W, H):
        assert np.isfinite(F).all(), name
        pos = F[F > 0].astype(np.float64)
        assert not np.any((pos > E64 * (1 - 1e-3)) & (pos < E64 * (1 + 1e-3))), "an entry sits at the flush threshold"
    if s["flush"]:
        assert (W0 == dt.type(1e-19)).sum() >= 10, name
    return dict(X=X, W0=W0, W=W, H=H, n_iter=n_iter, n_steps=n_steps, cost=cost, change=change, batch_size=s["bs"],
                max_iter=s["K"], tol=s["tol"], max_no_improvement=-1 if s["mni"] is None else s["mni"],
                forget_factor=s["ff"], beta=s["beta"], alpha=0.0, l1_ratio=0.0, dtype=dt.name, margin=margin,
                fresh_max_iter=s["fresh"], final_max_iter=s["final"], solve_iters=solves)


def cases_partial():
    def c(beta, tol=1e-2, fresh=60, alpha=0.0, l1_ratio=0.0, seed=821):
        return dict(M=25, R=24, offsets=[0, 150, 220, 330], bs=100, seed=seed, beta=beta, tol=tol, ff=0.7, fresh=fresh,
                    alpha=alpha, l1_ratio=l1_ratio)
    return {"mbnmf_pf_m25_r24_t150_70_110_bs100_b2": c(2.0), "mbnmf_pf_m25_r24_t150_70_110_bs100_b0p5": c(0.5),
            "mbnmf_pf_m25_r24_t150_70_110_bs100_reg_b1p5": c(1.5, alpha=1e-3, l1_ratio=0.5)}


def make_partial(name, s):
    X, W0, _ = synth(s["M"], s["R"], s["offsets"][-1], s["seed"])
    out, rho, margin, solves = run_partial(X, W0, s["offsets"], s["beta"], s["bs"], s["ff"], s["tol"], s["fresh"], s["alpha"],
                                           s["l1_ratio"])
    assert margin >= MARGIN["float64"] and solves.max() <= 140 and len(solves) == 3, (name, margin, solves)
    assert rho == s["ff"] ** (s["bs"] / s["offsets"][1]) != s["ff"]
    d = dict(X=X, W0=W0, offsets=np.array(s["offsets"]), rho=rho, batch_size=s["bs"], forget_factor=s["ff"], beta=s["beta"],
             tol=s["tol"], fresh_max_iter=s["fresh"], alpha=s["alpha"], l1_ratio=s["l1_ratio"], margin=margin, solve_iters=solves)
    for c, (W, A, B) in enumerate(out):
        assert np.isfinite(W).all() and np.isfinite(A).all() and np.isfinite(B).all()
        d[f"W_{c}"], d[f"A_{c}"], d[f"B_{c}"] = W, A, B
    return d


def all_cases():
    """name -> (maker, spec) over the three kinds"""
    out = {n: (make, s) for n, s in cases().items()}
    out.update({n: (make_fresh, s) for n, s in cases_fresh().items()})
    out.update({n: (make_partial, s) for n, s in cases_partial().items()})
    return out


def make(name, s):
    X, W, _ = synth(s["M"], s["R"], s["T"], s["seed"])
    dt = np.dtype(s["dtype"])
    X, W = X.astype(dt), W.astype(dt)
    H, n_iter, change, margin = run_sklearn(X, W, s["beta"], s["K"], s["tol"], s["alpha"], s["l1_ratio"])
    assert H.dtype == dt and margin >= MARGIN[dt.name], (name, margin)
    if s["stop"]:
        assert 2 < n_iter <= 140 and change[-1] <= s["tol"], (name, n_iter)
    else:
        assert n_iter == s["K"] <= 140 and change[-1] > s["tol"], (name, n_iter)
    assert np.isfinite(H).all(), name
    pos = H[H > 0].astype(np.float64)
    assert not np.any((pos > E64 * (1 - 1e-3)) & (pos < E64 * (1 + 1e-3))), "an entry sits at 2^-52"
    return dict(X=X, W=W, H=H, n_iter=n_iter, change=change, max_iter=s["K"], tol=s["tol"], beta=s["beta"],
                alpha=s["alpha"], l1_ratio=s["l1_ratio"], dtype=dt.name, margin=margin)


def main():
    check = "--check" in sys.argv
    names = [a for a in sys.argv[1:] if not a.startswith("--")]
    bad = 0
    for name, (maker, spec) in all_cases().items():
        if names and name not in names:
            continue
        out = maker(name, spec)
        path = os.path.join(GOLDEN, name + ".npz")
        if check:
            ref = np.load(path)
            same = all(np.array_equal(np.asarray(ref[k]), np.asarray(v)) for k, v in out.items())
            print(name, "same" if same else "DIFFERENT")
            bad += not same
        else:
            np.savez_compressed(path, **out)
            print(name, "n_iter", out.get("n_iter"), "n_steps", out.get("n_steps"), "solves", out.get("solve_iters"),
                  "margin %.2e" % out["margin"], os.path.getsize(path), "bytes")
    return bad


if __name__ == "__main__":
    sys.exit(main())
