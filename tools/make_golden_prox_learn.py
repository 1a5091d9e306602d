#!/usr/bin/env python3
"""Generate tests/golden/proxl_*.npz - runs ONLY where the vendored deComP lies (the build container).

The vectors are produced by executing deComP's own `dictionary_learning.solve` (decomp/dictionary_learning.py) from where it
lies, unmodified, behind the placeholder `chainer` package of tools/make_golden_prox.py.  Nothing of deComP's source text is
written into the fixtures: each .npz holds inputs (float32-representable, stored as float32), the start, the expected outputs
(`D`, `x`, `it`) and the options.

Per fixture the script
  * runs deComP once and asserts that tests/prox_learn_restatement.py - blocked, right-looking sweep, the frame orders by
    the shuffle rule - reproduces `it` exactly and D and x to 100 eps steps (`d_restated`, `x_restated` are recorded);
  * records the restatement's statistics (`trace`) and step count, and for a fixture that stops asserts that no statistic
    lies within 1000 `perm64` of `tol`;
  * reruns the restatement over the same steps with the BINS permuted - another summation order of the Gram matrix, the
    norms and Q, the same algorithm - in float64 and float32 and records how far D moves (absolute) and x moves (relative to
    max |x|): `perm64`, `perm32`, the larger of the two figures each.  100 times that is the GPU tests' bound;
  * records how far a float32 run over the same steps lies from the float64 one (`d32`).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import prox_learn_restatement as plr  # noqa: E402
import prox_restatement as pr  # noqa: E402
from make_golden_prox import import_decomp  # noqa: E402


def restated(y, D0, x0, c, order, dtype=np.float64, tol=None, max_steps=None):
    positive, momentum = pr.split_method(c["method"])
    return plr.solve(y, D0, c["alpha"], x0, batch_size=c["bs"], epochs=c["maxiter"] - 1, order=order,
                     tol=c["tol"] if tol is None else tol, lasso_iters=10, lasso_tol=1e-5, positive=positive,
                     momentum=momentum, dtype=dtype, max_steps=max_steps)


def moved(a, b):
    Da, xa, Db, xb = a[0].astype(np.float64), a[1].astype(np.float64), b[0].astype(np.float64), b[1].astype(np.float64)
    return float(max(np.max(np.abs(Da - Db)), np.max(np.abs(xa - xb)) / np.max(np.abs(xb))))


def perm_figure(y, D0, x0, c, order, steps, seed, dtype):
    perm = np.random.default_rng(seed + 1000).permutation(y.shape[1])
    base = restated(y, D0, x0, c, order, dtype=dtype, tol=0.0, max_steps=steps)
    other = restated(y[:, perm], D0[:, perm], x0, c, order, dtype=dtype, tol=0.0, max_steps=steps)
    back = np.empty_like(other[0])
    back[:, perm] = other[0]
    return moved((back, other[1]), base)


def inputs(c, seed):
    M, N, T = c["shape"]
    signed = not c["method"].endswith("_pos")
    y, D0 = plr.problem(M, N, T, seed, signed=signed, scale=c.get("scale", 1.0))
    x0 = None
    if c.get("unused_atom"):         # an atom no frame ever activates: alone on four bins that are silent in every frame
        y[:, -4:] = 0.0             # (exact unit norm, so that the first normalisation leaves it as it is)
        D0[:, -4:] = 0.0
        D0[-1] = 0.0
        D0[-1, -4:] = 0.5
        x0 = np.zeros((T, N))
    if c.get("x0_value"):            # a start far above the solution, which ten lasso updates do not bring down: atoms shrink
        x0 = np.full((T, N), float(c["x0_value"]))
    return y.astype(np.float32).astype(np.float64), D0.astype(np.float32).astype(np.float64), x0


def one_case(dl, c, seed):
    y, D0, x0 = inputs(c, seed)
    T = y.shape[0]
    epochs = c["maxiter"] - 1
    it, D, x = dl.solve(y.copy(), D0.copy(), c["alpha"], x=None if x0 is None else x0.copy(), tol=c["tol"], minibatch=c["bs"],
                        maxiter=c["maxiter"], method="block_cd", lasso_method=c["method"], lasso_iter=10, lasso_tol=1e-5,
                        random_seed=seed)
    order = plr.decomp_order(T, epochs, seed)
    Dr, xr, n_epochs, n_steps, trace, _ = restated(y, D0, x0, c, order)
    stopped = n_steps > 0 and trace[n_steps - 1] < c["tol"]
    assert int(it) == (n_epochs if stopped else c["maxiter"]), (c["name"], "it", it, n_epochs, n_steps)
    eps = np.finfo(np.float64).eps
    d_res, x_res = float(np.max(np.abs(D - Dr))), float(np.max(np.abs(x - xr)) / np.max(np.abs(x)))
    assert max(d_res, x_res) <= 100 * eps * max(n_steps, 1), (c["name"], "restatement differs from deComP", d_res, x_res)
    norms = np.sqrt(np.sum(D * D, axis=1))
    if c.get("inside") and not np.any(norms < 1.0 - 1e-6):
        return None
    if c.get("unused_atom"):
        assert np.all(x[:, -1] == 0.0) and np.array_equal(D[-1], D0[-1]), (c["name"], "the unused atom moved")
    p64 = perm_figure(y, D0, x0, c, order, n_steps, seed, np.float64)
    p32 = perm_figure(y, D0, x0, c, order, n_steps, seed, np.float32)
    if stopped:
        margin = float(np.min(np.abs(trace[:n_steps] - c["tol"])))
        if margin <= 1000 * p64:
            return None
    r32 = restated(y, D0, x0, c, order, dtype=np.float32, tol=0.0, max_steps=n_steps)
    r64 = restated(y, D0, x0, c, order, tol=0.0, max_steps=n_steps)
    out = dict(y=y.astype(np.float32), D0=D0.astype(np.float32), D=D, x=x, it=int(it), n_steps=n_steps, n_epochs=n_epochs,
               trace=trace[:n_steps], alpha=c["alpha"], tol=c["tol"], maxiter=c["maxiter"], bs=c["bs"], method=c["method"],
               seed=seed, perm64=p64, perm32=p32, d32=moved(r32, r64), d_restated=d_res, x_restated=x_res,
               min_norm=float(np.min(norms)))
    if x0 is not None:
        out["x0"] = x0
    path = os.path.join(OUT, c["name"] + ".npz")
    np.savez_compressed(path, **out)
    print("%-34s it=%d steps=%d stopped=%s nonzero=%.2f min|d|=%.3f restated=%.1e/%.1e perm64=%.2e perm32=%.2e d32=%.2e %d bytes"
          % (c["name"], int(it), n_steps, stopped, float(np.mean(x != 0)), out["min_norm"], d_res, x_res, p64, p32,
             out["d32"], os.path.getsize(path)))
    return out


CASES = [
    dict(name="proxl_m5_n3_t101_fista", shape=(5, 3, 101), bs=100, method="fista", alpha=0.1, tol=1e-4, maxiter=1000),
    dict(name="proxl_m25_n40_t130_fista_pos_k4", shape=(25, 40, 130), bs=32, method="fista_pos", alpha=1e-3, tol=0.0, maxiter=4),
    dict(name="proxl_m40_n70_t200_ista_pos_k3", shape=(40, 70, 200), bs=48, method="ista_pos", alpha=1e-3, tol=0.0, maxiter=3),
    dict(name="proxl_m201_n96_t150_fista_pos_k3", shape=(201, 96, 150), bs=64, method="fista_pos", alpha=1e-4, tol=0.0,
         maxiter=3),
    dict(name="proxl_m1_n5_t12_fista_pos", shape=(1, 5, 12), bs=4, method="fista_pos", alpha=1e-3, tol=1e-3, maxiter=10),
    dict(name="proxl_m25_n40_t130_fista_pos_stop", shape=(25, 40, 130), bs=32, method="fista_pos", alpha=1e-3, tol=1e-3,
         maxiter=1000),
    dict(name="proxl_m8_n6_t40_unused_atom", shape=(8, 6, 40), bs=16, method="fista_pos", alpha=1e-3, tol=0.0, maxiter=3,
         unused_atom=True),
    dict(name="proxl_m12_n10_t64_inside", shape=(12, 10, 64), bs=16, method="fista_pos", alpha=1e-3, tol=0.0, maxiter=3,
         inside=True, scales=(1.0, 0.3, 0.1, 0.03), x0_value=4.0),
]


def main():
    import_decomp()
    from decomp import dictionary_learning as dl
    only = set(sys.argv[1:])
    for k, c in enumerate(CASES):
        if only and c["name"] not in only:
            continue
        seed, tries = 300 + 10 * k, 0
        while True:
            cc = dict(c)
            if c.get("scales"):
                cc["scale"] = c["scales"][tries % len(c["scales"])]
            if one_case(dl, cc, seed + tries // max(len(c.get("scales", (1,))), 1)) is not None:
                break
            tries += 1
            assert tries < 200, (c["name"], "no seed or scale gives what the fixture is for")


if __name__ == "__main__":
    main()
