"""Golden vectors of mini-batch dictionary learning (evc_online_learn).

scikit-learn 1.7.2, `MiniBatchNMF(n_components=R, init='custom', batch_size=bs, beta_loss=beta, tol=tol, max_iter=K,
max_no_improvement=mni, forget_factor=ff, alpha_W=alpha, alpha_H='same', l1_ratio=l1_ratio, fresh_restarts=False)
.fit_transform(X, W=W0, H=H0)` through a recording subclass that stores every step's batch cost and
||H - H_buffer|| / ||H|| (scikit-learn's H is our dictionary W).  scikit-learn's X is T x M, its W is T x R (our H^T) and
its H is R x M (our W^T); the fixtures store the bin-major orientation: X (M, T), W0 / W (M, R), H0 / H (R, T), plus
n_iter, n_steps, cost, change (one entry per step carried out), batch_size, max_iter, tol, max_no_improvement (-1: off),
forget_factor, beta, alpha, l1_ratio, dtype.

X is a random low-rank product plus 5 % noise plus 1e-3, its frames scaled by a ramp 1 -> 3 so that the batch costs are
not monotone.  Every case asserts, for scikit-learn alone, that every decision of the run (H_diff <= tol, ewa < ewa_min)
that can end it is away from its threshold by a relative MARGIN[dtype] or more, and that no positive entry of either result lies within a
factor 1 +- 1e-3 of 2^-52 (the flush threshold).

Writes tests/golden/online_sk_*.npz; the prefix keeps them out of every other test's glob.

    python tools/make_golden_online.py [--check] [name ...]     (--check: recompute and compare instead of writing)
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
E64 = np.finfo(np.float64).eps
MARGIN = {"float64": 1e-6, "float32": 1e-2}     # float32 results are held to 1e-4: their decisions need that much more room


def synth(M, R, T, seed):
    rng = np.random.default_rng(seed)
    X = (rng.random((M, R)) ** 2) @ (rng.random((R, T)) * (rng.random((R, T)) < 0.5))
    X = X * (1 + 0.05 * rng.random((M, T))) + 1e-3
    X = X * np.linspace(1.0, 3.0, T)[None, :]
    W0 = rng.random((M, R)) + 1e-4
    H0 = rng.random((R, T)) + 1e-4
    return X, W0, H0


def recorder():
    from scipy import linalg
    from sklearn.decomposition import MiniBatchNMF

    class Recording(MiniBatchNMF):
        """records what _minibatch_convergence sees and how far each of its decisions is from its threshold"""

        def _minibatch_convergence(self, X, batch_cost, H, H_buffer, n_samples, step, n_steps):
            if step == 0:
                self.costs_, self.changes_, self.margins_ = [], [], []
            diff = float(linalg.norm(H - H_buffer) / linalg.norm(H))
            self.costs_.append(float(batch_cost))
            self.changes_.append(diff)
            ewa_min = self._ewa_cost_min if step > 0 else None
            stop = super()._minibatch_convergence(X, batch_cost, H, H_buffer, n_samples, step, n_steps)
            if step > 0:
                if self.tol > 0:
                    self.margins_.append(abs(diff - self.tol) / self.tol)
                if self.max_no_improvement is not None and not (self.tol > 0 and diff <= self.tol) and ewa_min is not None:
                    self.margins_.append(abs(float(self._ewa_cost) - float(ewa_min)) / abs(float(ewa_min)))
            return stop
    return Recording


def run_sklearn(X, W0, H0, beta, bs, K, tol, mni, ff, alpha=0.0, l1_ratio=0.0):
    """bin-major in, bin-major out: (W, H, n_iter, n_steps, cost, change, smallest decision margin)"""
    est = recorder()(n_components=W0.shape[1], init="custom", batch_size=bs, beta_loss=beta, tol=tol, max_iter=K,
                     max_no_improvement=mni, forget_factor=ff, alpha_W=alpha, alpha_H="same", l1_ratio=l1_ratio,
                     fresh_restarts=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        Wsk = est.fit_transform(np.ascontiguousarray(X.T), W=np.ascontiguousarray(H0.T), H=np.ascontiguousarray(W0.T))
    n = int(est.n_steps_)
    assert len(est.costs_) == n
    margin = min(est.margins_) if est.margins_ else np.inf
    return (np.ascontiguousarray(est.components_.T), np.ascontiguousarray(Wsk.T), int(est.n_iter_), n,
            np.array(est.costs_), np.array(est.changes_), margin)


def cases():
    """name -> dict(M, R, T, bs, seed, K, beta, tol, mni (None: off), ff, dtype, alpha, l1_ratio, flush, stop)
    stop: "mni" | "tol" | None - how the run must end"""
    def c(M, R, T, bs, seed, K, beta, tol=0.0, mni=None, ff=0.7, dtype=np.float64, alpha=0.0, l1_ratio=0.0, flush=False,
          stop=None):
        return dict(M=M, R=R, T=T, bs=bs, seed=seed, K=K, beta=beta, tol=tol, mni=mni, ff=ff, dtype=dtype, alpha=alpha,
                    l1_ratio=l1_ratio, flush=flush, stop=stop)
    d = {}
    # M, R no multiples of 16, a batch that is no multiple of the frame tile, a short last batch
    # (max_no_improvement 1 stops after 3 steps, at beta = 0 after 13; 2 at beta = 3 after 22)
    for tag, beta, mni in (("b2", 2.0, 1), ("b1", 1.0, 1), ("b0", 0.0, 1), ("b0p5", 0.5, 1), ("b3", 3.0, 2)):
        d[f"online_sk_m25_r24_t300_bs100_mni_{tag}"] = c(25, 24, 300, 100, 701, 20, beta, mni=mni, stop="mni")
    d["online_sk_m25_r24_t300_bs100_tol_b2"] = c(25, 24, 300, 100, 701, 20, 2.0, tol=1e-2, stop="tol")
    d["online_sk_m25_r24_t300_bs100_tol_b0p5"] = c(25, 24, 300, 100, 701, 20, 0.5, tol=3e-2, stop="tol")
    d["online_sk_m25_r24_t330_bs100_k3_b1p5"] = c(25, 24, 330, 100, 702, 3, 1.5)                    # no stop, short last batch
    d["online_sk_m40_r40_t330_bs128_k3_b0"] = c(40, 40, 330, 128, 703, 3, 0.0)                      # tile-aligned batches
    d["online_sk_m201_r32_t200_bs1024_k6_b1"] = c(201, 32, 200, 1024, 704, 6, 1.0)                  # one batch per pass
    d["online_sk_m33_r272_t300_bs96_k3_b0p5"] = c(33, 272, 300, 96, 705, 3, 0.5)                    # beyond the fused bound
    d["online_sk_m33_r272_t300_bs96_k3_b2"] = c(33, 272, 300, 96, 705, 3, 2.0)
    d["online_sk_m25_r24_t300_bs100_k3_reg_b1p5"] = c(25, 24, 300, 100, 706, 3, 1.5, alpha=1e-3, l1_ratio=0.5)
    d["online_sk_m25_r24_t300_bs100_k3_ff1_b3"] = c(25, 24, 300, 100, 707, 3, 3.0, ff=1.0)
    d["online_sk_m25_r24_t300_bs100_k3_f32_b2"] = c(25, 24, 300, 100, 708, 3, 2.0, dtype=np.float32)
    d["online_sk_m25_r24_t300_bs100_mni_f32_b2"] = c(25, 24, 300, 100, 708, 20, 2.0, mni=1, dtype=np.float32, stop="mni")
    d["online_sk_m25_r24_t300_bs100_k3_flush_b1"] = c(25, 24, 300, 100, 709, 3, 1.0, flush=True)
    d["online_sk_m25_r24_t300_bs100_k3_flush_b0p5"] = c(25, 24, 300, 100, 709, 3, 0.5, flush=True)
    return d


def make(name, s):
    X, W0, H0 = synth(s["M"], s["R"], s["T"], s["seed"])
    if s["flush"]:      # ~4 % of W0 and ~3 % of H0 far below the flush threshold
        rng = np.random.default_rng(s["seed"] + 1000)
        W0[rng.random(W0.shape) < 0.04] = 1e-19
        H0[rng.random(H0.shape) < 0.03] = 1e-19
    if s["R"] > 256:    # a constant start of the activations (compact_dictionary's): the file stays below 1 MiB
        H0[:] = np.sqrt(X.mean() / s["R"])
    dt = np.dtype(s["dtype"])
    X, W0, H0 = X.astype(dt), W0.astype(dt), H0.astype(dt)
    W, H, n_iter, n_steps, cost, change, margin = run_sklearn(X, W0, H0, s["beta"], s["bs"], s["K"], s["tol"], s["mni"],
                                                              s["ff"], s["alpha"], s["l1_ratio"])
    per_pass = -(-s["T"] // min(s["bs"], s["T"]))
    assert margin >= MARGIN[dt.name], (name, margin)
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
        assert (W == 0).sum() >= 10 or (H == 0).sum() >= 10, ((W == 0).sum(), (H == 0).sum())
    return dict(X=X, W0=W0, H0=H0, W=W, H=H, n_iter=n_iter, n_steps=n_steps, cost=cost, change=change, batch_size=s["bs"],
                max_iter=s["K"], tol=s["tol"], max_no_improvement=-1 if s["mni"] is None else s["mni"],
                forget_factor=s["ff"], beta=s["beta"], alpha=s["alpha"], l1_ratio=s["l1_ratio"], dtype=dt.name,
                margin=margin)


def main():
    check = "--check" in sys.argv
    names = [a for a in sys.argv[1:] if not a.startswith("--")]
    bad = 0
    for name, spec in cases().items():
        if names and name not in names:
            continue
        out = make(name, spec)
        path = os.path.join(GOLDEN, name + ".npz")
        if check:
            ref = np.load(path)
            same = all(np.array_equal(np.asarray(ref[k]), np.asarray(v)) for k, v in out.items())
            print(name, "same" if same else "DIFFERENT")
            bad += not same
        else:
            np.savez_compressed(path, **out)
            print(name, "n_iter", out["n_iter"], "n_steps", out["n_steps"], "margin %.2e" % out["margin"],
                  "zeros W/H", int((out["W"] == 0).sum()), int((out["H"] == 0).sum()), os.path.getsize(path), "bytes")
    return bad


if __name__ == "__main__":
    sys.exit(main())
