#!/usr/bin/env python3
"""Generate tests/golden/proxml_*.npz - runs ONLY where the vendored deComP lies (the build container).

The vectors are produced by executing deComP's own `dictionary_learning.solve(..., mask=)` (decomp/dictionary_learning.py,
solve_cd_mask) from where it lies, unmodified, behind the placeholder `chainer` package of tools/make_golden_prox.py.
Nothing of deComP's source text is written into the fixtures: each .npz holds inputs (float32-representable, stored as
float32), the mask, the start, the expected outputs (`D`, `x`, `it`) and the options.

Per fixture the script
  * runs deComP once and asserts that tests/prox_masked_learn_restatement.py - the Jacobi atom update, the frame orders by
    the shuffle rule - reproduces `it` exactly and D and x to 100 eps steps (`d_restated`, `x_restated` are recorded);
  * records the restatement's statistics (`trace`) and step count, and for a fixture that stops asserts that no statistic
    lies within 1000 `perm64` of `tol` (else the next seed is tried);
  * reruns the restatement over the same steps with the ATOMS AND THE BINS permuted, the mask along with them - another
    summation order of the lasso's two contractions, the norms, G and a_k, the same algorithm - in float64 and float32 and
    records how far D moves (absolute) and x moves (relative to max |x|): `perm64`, `perm32`, the larger of the two figures
    each.  100 times that is the GPU tests' bound;
  * records how far a float32 run over the same steps lies from the float64 one (`d32`);
  * asserts that every batch deComP takes holds a non-zero weight, so that deComP alone stays finite.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import prox_masked_learn_restatement as pmlr  # noqa: E402
import prox_restatement as pr  # noqa: E402
from make_golden_prox import import_decomp  # noqa: E402


def restated(y, D0, x0, mask, c, order, dtype=np.float64, tol=None, max_steps=None):
    positive, momentum = pr.split_method(c["method"])
    return pmlr.solve(y, D0, c["alpha"], x0, mask=mask, batch_size=c["bs"], epochs=c["maxiter"] - 1, order=order,
                      tol=c["tol"] if tol is None else tol, lasso_iters=10, lasso_tol=1e-5, positive=positive,
                      momentum=momentum, dtype=dtype, max_steps=max_steps)


def moved(a, b):
    Da, xa, Db, xb = a[0].astype(np.float64), a[1].astype(np.float64), b[0].astype(np.float64), b[1].astype(np.float64)
    return float(max(np.max(np.abs(Da - Db)), np.max(np.abs(xa - xb)) / np.max(np.abs(xb))))


def perm_figure(y, D0, x0, mask, c, order, steps, seed, dtype):
    rng = np.random.default_rng(seed + 1000)
    pn, pm = rng.permutation(D0.shape[0]), rng.permutation(y.shape[1])
    base = restated(y, D0, x0, mask, c, order, dtype=dtype, tol=0.0, max_steps=steps)
    other = restated(y[:, pm], D0[pn][:, pm], None if x0 is None else x0[:, pn], mask[:, pm], c, order, dtype=dtype, tol=0.0,
                     max_steps=steps)
    Db, xb = np.empty_like(other[0]), np.empty_like(other[1])
    Db[np.ix_(pn, pm)] = other[0]
    xb[:, pn] = other[1]
    return moved((Db, xb), base)


def inputs(c, seed, order):
    M, N, T = c["shape"]
    signed = not c["method"].endswith("_pos")
    y, D0 = pmlr.problem(M, N, T, seed, signed=signed)
    x0 = None
    if c.get("unused_atom"):         # an atom no frame ever activates: alone on four bins that are silent in every frame
        y[:, -4:] = 0.0             # (exact unit norm, so that the first normalisation leaves it as it is)
        D0[:, -4:] = 0.0
        D0[-1] = 0.0
        D0[-1, -4:] = 0.5
        x0 = np.zeros((T, N))
    kind = c.get("mask", "binary")
    mask = np.ones((T, M)) if kind == "ones" else pmlr.problem_mask(T, M, seed, kind=kind)
    if c.get("zero_frame"):
        mask[order[0, 3]] = 0.0     # a frame of the first batch without any valid bin
    if c.get("missing_bin"):
        mask[order[0, :c["bs"]], 2] = 0.0       # a bin that the whole first batch lacks
    return y.astype(np.float32).astype(np.float64), D0.astype(np.float32).astype(np.float64), x0, mask


def one_case(dl, c, seed):
    M, N, T = c["shape"]
    epochs = c["maxiter"] - 1
    order = pmlr.decomp_order(T, epochs, seed)
    y, D0, x0, mask = inputs(c, seed, order)
    assert np.array_equal(mask, mask.astype(np.float32)) and np.all(mask >= 0)
    for e in range(epochs):
        for b in range(T // c["bs"]):
            if not np.any(mask[order[e, b * c["bs"]:(b + 1) * c["bs"]]] > 0):
                return None
    kw = dict(x=None if x0 is None else x0.copy(), tol=c["tol"], minibatch=c["bs"], maxiter=c["maxiter"], method="block_cd",
              lasso_method=c["method"], lasso_iter=10, lasso_tol=1e-5, random_seed=seed)
    it, D, x = dl.solve(y.copy(), D0.copy(), c["alpha"], mask=mask.copy(), **kw)
    if not (np.all(np.isfinite(D)) and np.all(np.isfinite(x))):
        return None
    Dr, xr, n_epochs, n_steps, trace, _ = restated(y, D0, x0, mask, c, order)
    stopped = n_steps > 0 and trace[n_steps - 1] < c["tol"]
    assert int(it) == (n_epochs if stopped else c["maxiter"]), (c["name"], "it", it, n_epochs, n_steps)
    if c["tol"] > 0 and not stopped:
        return None
    eps = np.finfo(np.float64).eps
    d_res, x_res = float(np.max(np.abs(D - Dr))), float(np.max(np.abs(x - xr)) / np.max(np.abs(x)))
    assert max(d_res, x_res) <= 100 * eps * max(n_steps, 1), (c["name"], "restatement differs from deComP", d_res, x_res)
    if c.get("unused_atom"):
        assert np.all(x[:, -1] == 0.0) and np.array_equal(D[-1], D0[-1]), (c["name"], "the unused atom moved")
    unmasked = None
    if c.get("mask") == "ones":      # a mask of ones is NOT the unmasked learner: another atom update
        _, Du, xu = dl.solve(y.copy(), D0.copy(), c["alpha"], **kw)
        unmasked = float(np.max(np.abs(Du - D)))
        assert unmasked > 1e-6, (c["name"], "a mask of ones gave the unmasked learner's dictionary", unmasked)
    p64 = perm_figure(y, D0, x0, mask, c, order, n_steps, seed, np.float64)
    p32 = perm_figure(y, D0, x0, mask, c, order, n_steps, seed, np.float32)
    if stopped:
        margin = float(np.min(np.abs(trace[:n_steps] - c["tol"])))
        if margin <= 1000 * p64:
            return None
    r32 = restated(y, D0, x0, mask, c, order, dtype=np.float32, tol=0.0, max_steps=n_steps)
    r64 = restated(y, D0, x0, mask, c, order, tol=0.0, max_steps=n_steps)
    out = dict(y=y.astype(np.float32), D0=D0.astype(np.float32), mask=mask.astype(np.float32), D=D, x=x, it=int(it),
               n_steps=n_steps, n_epochs=n_epochs, trace=trace[:n_steps], alpha=c["alpha"], tol=c["tol"], maxiter=c["maxiter"],
               bs=c["bs"], method=c["method"], seed=seed, perm64=p64, perm32=p32, d32=moved(r32, r64), d_restated=d_res,
               x_restated=x_res)
    if x0 is not None:
        out["x0"] = x0
    if unmasked is not None:
        out["unmasked_differs"] = unmasked
    path = os.path.join(OUT, c["name"] + ".npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 512 * 1024
    print("%-36s it=%d steps=%d stopped=%s nonzero=%.2f valid=%.2f restated=%.1e/%.1e perm64=%.2e perm32=%.2e d32=%.2e %d bytes"
          % (c["name"], int(it), n_steps, stopped, float(np.mean(x != 0)), float(np.mean(mask > 0)), d_res, x_res, p64, p32,
             out["d32"], os.path.getsize(path)))
    return out


CASES = [
    dict(name="proxml_m5_n3_t101_fista", shape=(5, 3, 101), bs=50, method="fista", alpha=0.1, tol=1e-3, maxiter=1000,
         zero_frame=True),
    dict(name="proxml_m25_n40_t130_fista_pos_k4", shape=(25, 40, 130), bs=32, method="fista_pos", alpha=1e-3, tol=0.0, maxiter=4,
         zero_frame=True),
    dict(name="proxml_m12_n10_t64_ista_pos", shape=(12, 10, 64), bs=16, method="ista_pos", alpha=1e-3, tol=1e-3, maxiter=1000,
         zero_frame=True),
    dict(name="proxml_m1_n5_t12_k4", shape=(1, 5, 12), bs=4, method="fista_pos", alpha=1e-3, tol=0.0, maxiter=4),
    dict(name="proxml_m201_n48_t100_k3", shape=(201, 48, 100), bs=48, method="fista_pos", alpha=1e-4, tol=0.0, maxiter=3),
    dict(name="proxml_m25_n40_t130_weights_k3", shape=(25, 40, 130), bs=32, method="fista_pos", alpha=1e-3, tol=0.0, maxiter=3,
         mask="weights"),
    dict(name="proxml_m12_n10_t64_holes_k3", shape=(12, 10, 64), bs=16, method="fista_pos", alpha=1e-3, tol=0.0, maxiter=3,
         zero_frame=True, missing_bin=True),
    dict(name="proxml_m8_n6_t40_unused_atom_k3", shape=(8, 6, 40), bs=16, method="fista_pos", alpha=1e-3, tol=0.0, maxiter=3,
         unused_atom=True),
    dict(name="proxml_m12_n10_t64_ones_k3", shape=(12, 10, 64), bs=16, method="fista_pos", alpha=1e-3, tol=0.0, maxiter=3,
         mask="ones"),
]


def main():
    import_decomp()
    from decomp import dictionary_learning as dl
    only = set(sys.argv[1:])
    for k, c in enumerate(CASES):
        if only and c["name"] not in only:
            continue
        seed, tries = 500 + 10 * k, 0
        while one_case(dl, c, seed + tries) is None:
            tries += 1
            assert tries < 200, (c["name"], "no seed gives what the fixture is for")


if __name__ == "__main__":
    main()
