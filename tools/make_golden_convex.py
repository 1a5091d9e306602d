"""Record pymf's convex NMF (pymf/cnmf.py, class CNMF, run UNMODIFIED) as fixtures tests/golden/cnmf_*.npz and cnmfd_*.npz.

Runs only where the vendored pymf lies (tools/make_golden.py's PYMF_DIR and import shim).  Arrays and scalars only:
    data, G0, H0, niter, compute_w, compute_h   the call
    G, H, W, ferr, n_iter                       what the class left (n_iter: updates applied)
    seed (cnmfd_*)                              random.seed / np.random.seed before the class's own k-means start

cnmf_*: a cluster start as pymf builds it (cnmf.py:77-89) from labels t * R // T, handed to the class as attributes.
cnmfd_*: the default call - the start is the class's own (k-means on random.sample centres), recorded by calling its
_init_h() first, which is what factorize() does when H is missing.

    python tools/make_golden_convex.py
"""
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import convex_restatement as cr  # noqa: E402
from make_golden import OUT, import_pymf  # noqa: E402


def import_cnmf():
    import_pymf()
    if not hasattr(np, "bool"):          # pymf/kmeans.py:80 spells the builtin the way numpy < 1.24 exported it
        np.bool = bool
    from pymf.cnmf import CNMF
    return CNMF


def save(name, mdl, data, G0, H0, niter, compute_w, compute_h, **extra):
    n_ferr = len(mdl.ferr)
    n_iter = niter if n_ferr == niter else n_ferr + 1
    np.savez_compressed(os.path.join(OUT, name + ".npz"), data=data, G0=G0, H0=H0, niter=niter, compute_w=compute_w,
                        compute_h=compute_h, G=mdl.G, H=mdl.H, W=mdl.W, ferr=mdl.ferr, n_iter=n_iter, **extra)
    print(f"{name}: M={data.shape[0]} T={data.shape[1]} R={G0.shape[1]} niter={niter} n_iter={n_iter} "
          f"ferr {mdl.ferr[0]:.6g} -> {mdl.ferr[-1]:.6g} rises={int(np.sum(np.diff(mdl.ferr) > 0))}")


def given_case(CNMF, name, data, G0, H0, niter, compute_w=True, compute_h=True):
    mdl = CNMF(data.copy(), num_bases=G0.shape[1])
    mdl.G, mdl.H = G0.copy(), H0.copy()
    mdl.W = np.dot(data, mdl.G)
    mdl.factorize(niter=niter, compute_w=compute_w, compute_h=compute_h)
    save(name, mdl, data, G0, H0, niter, compute_w, compute_h)


def default_case(CNMF, name, data, R, niter, seed):
    random.seed(seed)
    np.random.seed(seed)
    mdl = CNMF(data.copy(), num_bases=R)
    mdl._init_h()
    G0, H0 = mdl.G.copy(), mdl.H.copy()
    mdl.factorize(niter=niter)
    save(name, mdl, data, G0, H0, niter, True, True, seed=seed)


def main():
    CNMF = import_cnmf()
    for M, T, R, niter, seed in ((25, 70, 8, 30, 2101), (40, 257, 17, 60, 2102), (3, 5, 2, 10, 2103), (25, 300, 33, 100, 2104)):
        X, assign = cr.problem(M, T, R, seed)
        G0, H0 = cr.cluster_start(assign, R)
        given_case(CNMF, f"cnmf_m{M}_t{T}_r{R}", X, G0, H0, niter)
    X, assign = cr.problem(25, 70, 8, 2101)
    G0, H0 = cr.cluster_start(assign, 8)
    Gz = np.where(G0 > 0.5 / 70, G0, 0.0)           # the one-hot part alone: exact zeros elsewhere
    given_case(CNMF, "cnmf_zeros", X, Gz, H0, 30)
    given_case(CNMF, "cnmf_honly", X, G0, H0, 30, compute_w=False)
    given_case(CNMF, "cnmf_gonly", X, G0, H0, 30, compute_h=False)
    default_case(CNMF, "cnmfd_doctest", np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]]), 2, 10, 2110)
    default_case(CNMF, "cnmfd_m25_t70_r8", X, 8, 30, 2111)
    default_case(CNMF, "cnmfd_m40_t257_r17", cr.problem(40, 257, 17, 2102)[0], 17, 20, 2112)


if __name__ == "__main__":
    main()
