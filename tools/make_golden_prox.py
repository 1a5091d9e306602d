#!/usr/bin/env python3
"""Generate tests/golden/prox_*.npz - runs ONLY where the vendored deComP lies (the build container).

The vectors are produced by executing deComP's own `lasso.solve` / `nnls.solve` (decomp/lasso.py, decomp/nnls.py) from where
they lie, unmodified.  deComP imports `chainer` at the top of several modules that the lasso path never calls, so a
placeholder `chainer` package (chainer, chainer.cuda, chainer.utils with conv = conv_nd = None) stands in `sys.modules`.
Nothing of deComP's source text is written into the fixtures: each .npz holds inputs, the start, the expected outputs, `it`
and the options (y and A hold float32-representable values and are stored as float32).

Per fixture the script
  * runs deComP once over all frames (`x`, `it`) and, where `offs` splits the frames, once per utterance (`x_split`,
    `it_split`): deComP takes its stop statistic over the whole call, evc_prox_solve per utterance;
  * asserts that tests/prox_restatement.py reproduces every run to the last bit, and records a fingerprint of this
    machine's BLAS on the fixture's products (`blas_crc`): numpy's matrix products, deComP's and the restatement's alike,
    sum in an order that depends on the processor, so the tests demand the last bit where the fingerprint is met and the
    permutation bound below elsewhere;
  * asserts that no stop decision sits on its threshold: at every check |max(|dx| - tol_n)| >= 1e-6 tol, else the next seed
    is tried;
  * reruns the restatement with the exemplars permuted (another summation order) in float64 and float32 and records how far
    the result moves, relative to max |x| (`perm64`, `perm32`): 100 times that is the GPU tests' bound.
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
DECOMP = os.path.join(os.path.dirname(ROOT), "reference", "dependencies", "deComP-master")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import prox_restatement as pr  # noqa: E402


def import_decomp():
    if not os.path.isdir(DECOMP):
        raise SystemExit("the vendored deComP is not here: %s" % DECOMP)
    chainer = types.ModuleType("chainer")
    chainer.cuda = types.ModuleType("chainer.cuda")
    chainer.utils = types.ModuleType("chainer.utils")
    chainer.utils.conv = chainer.utils.conv_nd = None
    chainer.__path__ = []
    for name, mod in (("chainer", chainer), ("chainer.cuda", chainer.cuda), ("chainer.utils", chainer.utils)):
        sys.modules.setdefault(name, mod)
    sys.path.insert(0, DECOMP)
    from decomp import lasso, nnls
    return lasso, nnls


def restated(y, A, c, x0, offs=None, dtype=np.float64, stop=True):
    positive, momentum = pr.split_method(c["method"])
    return pr.solve(y, A, c["alpha"], x0, tol=c["tol"], iters=c["maxiter"], positive=positive, momentum=momentum,
                    utt_offsets=offs, dtype=dtype, stop=stop)


def perm_figure(y, A, c, x0, seed, dtype):
    """how far the restatement's result moves, relative to max |x|, when the exemplars are summed in another order"""
    perm = np.random.default_rng(seed + 1000).permutation(A.shape[0])
    base = restated(y, A, c, x0, dtype=dtype, stop=False)[0].astype(np.float64)
    moved = restated(y, A[perm], c, None if x0 is None else x0[:, perm], dtype=dtype, stop=False)[0].astype(np.float64)
    back = np.empty_like(moved)
    back[:, perm] = moved
    return float(np.max(np.abs(back - base)) / np.max(np.abs(base)))


def one_case(lasso, nnls, c, seed):
    M, N, T = c["shape"]
    signed = not c["method"].endswith("_pos")
    y, A = (m.astype(np.float32).astype(np.float64) for m in pr.problem(M, N, T, seed, signed=signed))   # stored as float32
    x0 = None
    if c.get("start"):
        x0 = np.random.default_rng(seed + 500).random((T, N)) * 0.05

    def run(ys, xs):
        xs = None if xs is None else xs.copy()
        if c.get("nnls"):
            return nnls.solve(ys.copy(), A.copy(), c["alpha"], x=xs, tol=c["tol"], method=c["method"][:-4],
                              maxiter=c["maxiter"])
        return lasso.solve(ys.copy(), A.copy(), c["alpha"], x=xs, tol=c["tol"], method=c["method"], maxiter=c["maxiter"])

    it, x = run(y, x0)
    xr, nr, tr = restated(y, A, c, x0)
    assert np.array_equal(x, xr) and int(it) + 1 == int(nr[0]), (c["name"], "restatement differs from deComP")
    traces = [tr]
    out = dict(y=y.astype(np.float32), A=A.astype(np.float32), x=x, it=int(it), alpha=c["alpha"], tol=c["tol"],
               maxiter=c["maxiter"], method=c["method"], seed=seed, nnls=bool(c.get("nnls")))
    if x0 is not None:
        out["x0"] = x0
    if c.get("offs"):
        offs = c["offs"]
        parts = [run(y[a:b], None if x0 is None else x0[a:b]) for a, b in zip(offs[:-1], offs[1:])]
        xs, its = np.concatenate([p[1] for p in parts]), np.array([int(p[0]) for p in parts])
        xr, nr, tr = restated(y, A, c, x0, offs)
        assert np.array_equal(xs, xr) and np.array_equal(its + 1, nr), (c["name"], "split restatement differs from deComP")
        traces.append(tr)
        if len(set(its.tolist())) == 1:            # the batch fixture is to stop its utterances at different iterations
            return None
        out.update(offs=np.array(offs), x_split=xs, it_split=its)
    margin = np.inf
    if c["tol"] > 0:
        stats = np.concatenate([t[np.isfinite(t)] for t in traces])
        margin = float(np.min(np.abs(stats)) / c["tol"])
        if margin < 1e-6:
            return None
    out["blas_crc"] = np.array(pr.blas_fingerprint(y, A), dtype=np.int64)
    out["perm64"] = perm_figure(y, A, c, x0, seed, np.float64)
    out["perm32"] = perm_figure(y, A, c, x0, seed, np.float32)
    x32 = restated(y, A, c, x0, dtype=np.float32, stop=False)[0]
    x64 = restated(y, A, c, x0, stop=False)[0]
    out["d32"] = float(np.max(np.abs(x32 - x64)) / np.max(np.abs(x64)))
    np.savez_compressed(os.path.join(OUT, c["name"] + ".npz"), **out)
    print("%-28s it=%s split=%s nonzero=%.2f margin=%.3g tol  perm64=%.2e perm32=%.2e d32=%.2e  max|x|=%.3g  %d bytes" % (
        c["name"], int(it), out.get("it_split"), float(np.mean(x != 0)), margin, out["perm64"], out["perm32"], out["d32"],
        float(np.max(np.abs(x))), os.path.getsize(os.path.join(OUT, c["name"] + ".npz"))))
    return out


CASES = [
    dict(name="prox_m25_n64_t32_fista_pos", shape=(25, 64, 32), method="fista_pos", alpha=1e-3, tol=1e-3, maxiter=300,
         offs=[0, 16, 32]),
    dict(name="prox_m40_n130_t33_ista_pos", shape=(40, 130, 33), method="ista_pos", alpha=1e-3, tol=1e-3, maxiter=300,
         offs=[0, 16, 33]),
    dict(name="prox_m25_n64_t32_fista", shape=(25, 64, 32), method="fista", alpha=1e-3, tol=1e-3, maxiter=300),
    dict(name="prox_m1_n5_t3_fista_pos", shape=(1, 5, 3), method="fista_pos", alpha=1e-3, tol=1e-6, maxiter=100),
    dict(name="prox_m201_n300_t20_fista_pos", shape=(201, 300, 20), method="fista_pos", alpha=1e-4, tol=1e-3, maxiter=400,
         offs=[0, 10, 20]),
    dict(name="prox_m25_n64_t32_fista_pos_k50", shape=(25, 64, 32), method="fista_pos", alpha=1e-3, tol=0.0, maxiter=50),
    dict(name="prox_m25_n64_t32_fista_pos_k100", shape=(25, 64, 32), method="fista_pos", alpha=1e-3, tol=0.0, maxiter=100),
    dict(name="prox_m25_n64_t32_nnls_ista", shape=(25, 64, 32), method="ista_pos", alpha=1e-3, tol=1e-3, maxiter=300,
         nnls=True),
    dict(name="prox_m25_n64_t32_fista_pos_start", shape=(25, 64, 32), method="fista_pos", alpha=1e-3, tol=1e-3, maxiter=300,
         start=True),
]


def main():
    lasso, nnls = import_decomp()
    for k, c in enumerate(CASES):
        seed = 100 + 10 * k
        while one_case(lasso, nnls, c, seed) is None:
            print("%s: a stop decision within 1e-6 tol of its threshold, or one stop for all utterances, at seed %d: trying "
                  "the next" % (c["name"], seed))
            seed += 1


if __name__ == "__main__":
    main()
