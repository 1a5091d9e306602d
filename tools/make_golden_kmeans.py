"""Record pymf's k-means (pymf/kmeans.py, class Kmeans, run UNMODIFIED) as fixtures tests/golden/kmeans_*.npz.

Runs only where the vendored pymf lies (tools/make_golden.py's PYMF_DIR and import shim).  Arrays and scalars only:
    data, W0, niter, compute_w, seed   the call (W0: the centres the class started from - its own random.sample draw under
                                       random.seed(seed), recorded by calling its _init_w() first, or the ones handed to it)
    W, assigned, ferr, n_iter          what the class left (n_iter: rounds carried out)

    python tools/make_golden_kmeans.py
"""
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kmeans_restatement as kr  # noqa: E402
from make_golden import OUT, import_pymf  # noqa: E402


def import_kmeans():
    import_pymf()
    if not hasattr(np, "bool"):          # pymf/kmeans.py:80 spells the builtin the way numpy < 1.24 exported it
        np.bool = bool
    from pymf.kmeans import Kmeans
    return Kmeans


def case(Kmeans, name, data, R, niter, seed, W0=None, compute_w=True):
    random.seed(seed)
    np.random.seed(seed)
    mdl = Kmeans(data.copy(), num_bases=R)
    if W0 is None:
        mdl._init_w()
        W0 = mdl.W.copy()
    else:
        mdl.W = np.array(W0, dtype=np.float64)
    mdl.factorize(niter=niter, compute_w=compute_w)
    n_ferr = len(mdl.ferr)
    n_iter = niter if n_ferr == niter else n_ferr + 1
    np.savez_compressed(os.path.join(OUT, name + ".npz"), data=data, W0=W0, niter=niter, compute_w=compute_w, seed=seed, W=mdl.W,
                        assigned=np.asarray(mdl.assigned), ferr=mdl.ferr, n_iter=n_iter)
    counts = np.bincount(mdl.assigned, minlength=R)
    print(f"{name}: M={data.shape[0]} T={data.shape[1]} R={R} niter={niter} n_iter={n_iter} empty={int(np.sum(counts == 0))} "
          f"ferr {mdl.ferr[0] if n_ferr else float('nan'):.6g} -> {mdl.ferr[-1] if n_ferr else float('nan'):.6g}")


def main():
    Kmeans = import_kmeans()
    case(Kmeans, "kmeans_doctest", np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0]]), 2, 10, 2201)
    case(Kmeans, "kmeans_doctest_vq", np.array([[1.5], [1.2]]), 2, 1, 2202, W0=np.array([[1.0, 0.0], [0.0, 1.0]]), compute_w=False)
    d = np.load(os.path.join(OUT, "cnmfd_m25_t70_r8.npz"))
    case(Kmeans, "kmeans_m25_t70_r8", d["data"], 8, 10, 2111)                  # an empty cluster
    case(Kmeans, "kmeans_m40_t257_r17", kr.problem(40, 257, 17, 2204), 17, 30, 2204)
    case(Kmeans, "kmeans_m1_t64_r5", kr.problem(1, 64, 5, 2205), 5, 30, 2205)
    case(Kmeans, "kmeans_m513_t200_r17", kr.problem(513, 200, 17, 2206), 17, 30, 2206)      # more than one chunk of bins
    X = kr.problem(25, 70, 8, 2207)
    case(Kmeans, "kmeans_vq_m25_t70_r8", X, 8, 5, 2207, W0=kr.problem(25, 8, 8, 2208), compute_w=False)
    pick = np.array([3, 20, 20, 41, 41, 41, 60, 3])                             # duplicated start centres
    case(Kmeans, "kmeans_dup_m25_t70_r8", X, 8, 30, 2209, W0=X[:, pick])


if __name__ == "__main__":
    main()
