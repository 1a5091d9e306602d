#!/usr/bin/env python3
"""Generate tests/golden/mum_*.npz - runs ONLY where the vendored deComP lies (the build container).

tools/make_golden_prox_masked.py's recipe for the activation half of deComP's masked `nmf.solve(method='mu')`: the vectors are
produced by executing deComP's own code from where it lies, unmodified, behind the same placeholder `chainer` package - K
calls of `grads.get_likelihood(l).update_x` (decomp/nmf_methods/grads.py) from the recorded start.  Nothing of deComP's
source text is written into the fixtures: each .npz holds inputs, the mask, the start, the expected output and the options
(y, D, mask and a recorded start hold float32-representable values and are stored as float32; D and the start lie on a grid of
1/256, at 201 bins D on one of 1/16, so that they compress).

Per fixture the script
  * asserts that tests/mu_masked_restatement.py reproduces the K updates to the last bit, and records a fingerprint of this
    machine's BLAS on the fixture's products (`blas_crc`);
  * where `offs` splits the frames, runs the restatement with evc_mu_masked_solve's own stop rule (deComP has no
    fixed-dictionary surface) and records `n_iter_stop` and `trace_stop`; asserts that no stop decision sits within
    1e-6 tol of its threshold;
  * asserts that the mask has a zero and a non-zero, that x is finite and not all zero and that the permutation figures below
    are positive - else the next seed is tried;
  * reruns the restatement with the exemplars AND the bins permuted (the factored sweep sums over both) in float64 and
    float32 and records how far the result moves, relative to max |x| (`perm64`, `perm32`): 100 times that is the GPU tests'
    bound.
At least one batch fixture stops its utterances at different checks (asserted at the end).

The learn fixtures (mum_learn_*.npz) record deComP's `nmf.solve(method='mu')` itself - `it`, D, x - with the same assertions:
the restatement (mmr.learn) reproduces it to the last bit, no statistic max |D - D_new| sits within 1e-6 tol of tol, the
permutation figures (atoms, bins and frames permuted) are positive.  One of them stops before maxiter, one runs to the end.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import mu_masked_restatement as mmr  # noqa: E402
from make_golden_prox import import_decomp  # noqa: E402


def one_case(grads, c, seed):
    M, N, T = c["shape"]
    loss, K = c["loss"], c["K"]
    y, D = mmr.problem(M, N, T, seed)
    y = y.astype(np.float32).astype(np.float64)
    grid = 16.0 if M > 128 else 256.0
    D = np.round(D * grid) / grid
    mask = mmr.problem_mask(T, M, seed, c["kind"])
    assert np.array_equal(D, D.astype(np.float32)) and np.array_equal(mask, mask.astype(np.float32))
    assert (mask == 0).any() and (mask > 0).any() and (mask >= 0).all() and (y >= 0).all() and (D > 0).all()
    x0 = np.round((np.random.default_rng(seed + 500).random((T, N)) + 0.125) * 256.0) / 256.0 if c.get("start") else np.ones((T, N))

    lik = grads.get_likelihood(loss)
    x = x0.copy()
    for _ in range(K):
        x = lik.update_x(y.copy(), x, D.copy(), mask.copy())
    if not (np.isfinite(x).all() and x.any()):
        return None
    xr = mmr.solve(y, D, x0, mask=mask, loss=loss, iters=K)[0]
    assert np.array_equal(x, xr), (c["name"], "restatement differs from deComP")
    out = dict(y=y.astype(np.float32), D=D.astype(np.float32), mask=mask.astype(np.float32), x=x, K=K, loss=loss, seed=seed,
               kind=c["kind"])
    if c.get("start"):
        out["x0"] = x0.astype(np.float32)
    margin = np.inf
    if c.get("offs"):
        xs, ns, tr = mmr.solve(y, D, x0, mask=mask, loss=loss, iters=c["iters"], check_every=c["check_every"], tol=c["tol"],
                               utt_offsets=c["offs"])
        margin = mmr.stop_margin(tr, c["tol"]) / c["tol"]
        if margin < 1e-6 or len(set(ns.tolist())) == 1 or (ns == c["iters"]).all():
            return None
        out.update(offs=np.array(c["offs"]), iters=c["iters"], check_every=c["check_every"], tol=c["tol"],
                   n_iter_stop=ns, trace_stop=tr)
    out["blas_crc"] = np.array(mmr.blas_fingerprint(y, D, mask), dtype=np.int64)
    out["perm64"] = mmr.permutation_figure(y, D, mask, K, np.float64, loss, x0=x0, seed=seed + 1000, floor=False)
    out["perm32"] = mmr.permutation_figure(y, D, mask, K, np.float32, loss, x0=x0, seed=seed + 1000, floor=False)
    if not (out["perm64"] > 0 and out["perm32"] > 0):       # the permutation moved nothing: it measures nothing
        return None
    x32 = mmr.solve(y, D, x0, mask=mask, loss=loss, iters=K, dtype=np.float32)[0]
    out["d32"] = float(np.max(np.abs(x32 - x)) / np.max(np.abs(x)))
    np.savez_compressed(os.path.join(OUT, c["name"] + ".npz"), **out)
    print("%-24s K=%d stop=%s zero=%.2f margin=%.3g tol  perm64=%.2e perm32=%.2e d32=%.2e  max|x|=%.3g  %d bytes" % (
        c["name"], K, out.get("n_iter_stop"), float(np.mean(x == 0)), margin, out["perm64"], out["perm32"], out["d32"],
        float(np.max(np.abs(x))), os.path.getsize(os.path.join(OUT, c["name"] + ".npz"))))
    return out


def learn_case(nmf, c, seed):
    M, R, T = c["shape"]
    loss = c["loss"]
    y, _ = mmr.problem(M, R, T, seed)
    y = y.astype(np.float32).astype(np.float64)
    rng = np.random.default_rng(seed + 300)
    D0 = np.round((rng.random((R, M)) + 0.05) * 256.0) / 256.0
    x0 = np.round((rng.random((T, R)) + 0.125) * 256.0) / 256.0 if c.get("start") else None
    mask = mmr.problem_mask(T, M, seed, c["kind"])
    assert (mask == 0).any() and (mask > 0).any() and (mask >= 0).all() and (y >= 0).all() and (D0 > 0).all()
    it, D, x = nmf.solve(y.copy(), D0.copy(), None if x0 is None else x0.copy(), tol=c["tol"], maxiter=c["maxiter"], method="mu",
                         likelihood=loss, mask=mask.copy())
    if not (np.isfinite(D).all() and np.isfinite(x).all() and x.any()):
        return None
    itr, Dr, xr, stats = mmr.learn(y, D0, x0, mask=mask, loss=loss, tol=c["tol"], maxiter=c["maxiter"])
    assert int(it) == itr and np.array_equal(D, Dr) and np.array_equal(x, xr), (c["name"], "restatement differs from deComP")
    n_iter = len(stats)
    if c["tol"] > 0 and np.min(np.abs(stats - c["tol"])) < 1e-6 * c["tol"]:
        return None
    if c.get("stops") is not None and (int(it) < c["maxiter"]) != c["stops"]:
        return None
    out = dict(y=y.astype(np.float32), D0=D0.astype(np.float32), mask=mask.astype(np.float32), D=D, x=x, it=int(it), n_iter=n_iter,
               stats=stats, tol=c["tol"], maxiter=c["maxiter"], loss=loss, seed=seed, kind=c["kind"])
    if x0 is not None:
        out["x0"] = x0.astype(np.float32)
    out["blas_crc"] = np.array(mmr.blas_fingerprint(y, D0, mask), dtype=np.int64)
    out["perm64"] = mmr.learn_permutation_figure(y, D0, mask, n_iter, np.float64, loss, x0=x0, seed=seed + 1000, floor=False)
    out["perm32"] = mmr.learn_permutation_figure(y, D0, mask, n_iter, np.float32, loss, x0=x0, seed=seed + 1000, floor=False)
    if not (out["perm64"] > 0 and out["perm32"] > 0):
        return None
    np.savez_compressed(os.path.join(OUT, c["name"] + ".npz"), **out)
    print("%-28s it=%d n_iter=%d margin=%.3g tol  perm64=%.2e perm32=%.2e  max|x|=%.3g  %d bytes" % (
        c["name"], int(it), n_iter, (np.min(np.abs(stats - c["tol"])) / c["tol"]) if c["tol"] > 0 else np.inf, out["perm64"],
        out["perm32"], float(np.max(np.abs(x))), os.path.getsize(os.path.join(OUT, c["name"] + ".npz"))))
    return out


LEARN_CASES = [
    dict(name="mum_learn_m25_r8_t48_l2", shape=(25, 8, 48), loss="l2", kind="binary", tol=2e-3, maxiter=200, stops=True),
    dict(name="mum_learn_m40_r19_t33_kl", shape=(40, 19, 33), loss="kl", kind="weights", tol=2e-3, maxiter=200, stops=True,
         start=True),
    dict(name="mum_learn_m201_r12_t40_kl_k12", shape=(201, 12, 40), loss="kl", kind="binary", tol=1e-9, maxiter=13, stops=False),
]


def cases():
    out = []
    for loss in mmr.LOSSES:
        out += [
            dict(name="mum_m25_n64_t32_%s" % loss, shape=(25, 64, 32), loss=loss, kind="binary", K=40, offs=[0, 16, 32],
                 iters=200, check_every=2, tol=1e-4),
            dict(name="mum_m40_n130_t33_%s" % loss, shape=(40, 130, 33), loss=loss, kind="weights", K=40, offs=[0, 16, 33],
                 iters=200, check_every=2, tol=1e-4, start=True),
            dict(name="mum_m1_n5_t3_%s" % loss, shape=(1, 5, 3), loss=loss, kind="binary", K=20),
            dict(name="mum_m201_n300_t20_%s" % loss, shape=(201, 300, 20), loss=loss, kind="binary", K=25),
        ]
    return out


def main():
    import_decomp()
    from decomp.nmf_methods import grads
    different = 0
    for k, c in enumerate(cases()):
        seed = 100 + 50 * k
        while True:
            out = one_case(grads, c, seed)
            if out is not None:
                break
            print("%s: an all-zero or non-finite x, a permutation figure of 0, a stop decision within 1e-6 tol of its threshold, "
                  "or one stop for all utterances, at seed %d: trying the next" % (c["name"], seed))
            seed += 1
            assert seed < 100 + 50 * k + 50, c["name"]
        different += "n_iter_stop" in out and len(set(out["n_iter_stop"].tolist())) > 1
    assert different >= 1, "no batch fixture stops its utterances at different checks"
    from decomp import nmf
    outs = []
    for k, c in enumerate(LEARN_CASES):
        seed = 900 + 50 * k
        while True:
            out = learn_case(nmf, c, seed)
            if out is not None:
                break
            print("%s: rejected at seed %d: trying the next" % (c["name"], seed))
            seed += 1
            assert seed < 900 + 50 * k + 50, c["name"]
        outs.append(out)
    assert any(o["it"] < o["maxiter"] for o in outs) and any(o["it"] == o["maxiter"] for o in outs)


if __name__ == "__main__":
    main()
