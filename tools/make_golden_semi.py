#!/usr/bin/env python3
"""Generate tests/golden/snmf*.npz - runs ONLY where the vendored pymf lies (the build container).

The vectors are produced by executing pymf's own SNMF (pymf/snmf.py, pymf/base.py) from where it lies, imported with the
two-symbol shim of tools/make_golden.py (`scipy.misc.factorial`, a placeholder `cvxopt`: neither is touched by SNMF).
`SNMF._update_h`, `SNMF._update_w`, `PyMFBase.factorize`, `_init_w`, `_init_h`, `_converged` and `frobenius_norm` run
unmodified.  Nothing of its source text is written into the fixtures: each .npz holds inputs, the start, the expected
outputs and a few scalars.

  snmf_<shape>_k<niter>    factorize(niter, compute_w=False) on a signed dictionary and signed frames
  snmf_doctest             the class's doctest data ([[1.5], [1.2]], W = I), niter = 20
  snmf_zero_collapse       H reaches exactly 0 after one update: ferr is constant and the stop fires with a difference of 0
  snmfw_m25_r8_t70_k30     the default call, compute_w=True, W and H drawn by pymf from the seeded global generator
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_golden  # noqa: E402
import semi_restatement as sr  # noqa: E402


def import_snmf():
    make_golden.import_pymf()
    from pymf.snmf import SNMF
    return SNMF


def applied(ferr, niter):
    """updates applied: pymf cuts ferr to ferr[:i] when it stops at update i + 1"""
    return niter if len(ferr) == niter else len(ferr) + 1


def fixed_case(SNMF, name, data, W, H0, niter):
    mdl = SNMF(data.copy(), num_bases=W.shape[1])
    mdl.W = W.copy()
    mdl.H = H0.copy()
    mdl.factorize(niter=niter, compute_w=False)
    ferr = np.asarray(mdl.ferr)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), surface="pymf_snmf", data=data, W=W, H0=H0, H=mdl.H, ferr=ferr,
                        niter=niter, n_iter=applied(ferr, niter), frobenius_norm=mdl.frobenius_norm(), residual=mdl.residual())
    print(f"{name}: M={data.shape[0]} T={data.shape[1]} N={W.shape[1]} len(ferr)={len(ferr)} "
          f"monotone={bool(np.all(np.diff(ferr) <= 0))}")


def default_case(SNMF, name, M, R, T, seed, niter):
    A, X, _ = sr.problem(M, R, T, seed, active=3)
    np.random.seed(seed)
    mdl = SNMF(X.copy(), num_bases=R)
    mdl.factorize(niter=niter)                      # compute_w=True: _init_w, then _init_h, from the global generator
    np.random.seed(seed)
    np.random.random((M, R))
    H0 = np.random.random((R, T)) + 10 ** -4          # what _init_h drew
    ferr = np.asarray(mdl.ferr)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), surface="pymf_snmf_full", data=X, seed=seed, H0=H0, W=mdl.W, H=mdl.H,
                        ferr=ferr, niter=niter, n_iter=applied(ferr, niter))
    print(f"{name}: M={M} T={T} R={R} len(ferr)={len(ferr)}")


def main():
    SNMF = import_snmf()
    for M, N, T, k, seed in ((25, 64, 32, 50, 11), (40, 130, 33, 100, 12), (1, 5, 3, 10, 13)):
        A, X, H0 = sr.problem(M, N, T, seed)
        fixed_case(SNMF, f"snmf_m{M}_n{N}_t{T}_k{k}", X, A, H0, k)
    rng = np.random.default_rng(14)
    fixed_case(SNMF, "snmf_doctest", np.array([[1.5], [1.2]]), np.eye(2), rng.random((2, 1)) + 1e-4, 20)
    fixed_case(SNMF, "snmf_zero_collapse", np.array([[-1.0], [0.0]]), np.array([[1.0, -1.0], [0.0, 0.0]]),
               np.array([[1.0], [0.0]]), 20)
    default_case(SNMF, "snmfw_m25_r8_t70_k30", 25, 8, 70, 15, 30)


if __name__ == "__main__":
    main()
