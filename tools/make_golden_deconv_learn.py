"""Golden vectors of the dictionary half of the convolutive dictionary learning (evc_deconv_learn).

scikit-learn 1.7.2 has no convolutive model, but one dictionary half IS its multiplicative update of the stacked
dictionary [W_0 ... W_{L-1}] (M x LR) under the stacked shifted activations [Hs_0; ...; Hs_{L-1}] (LR x T): the installed
`sklearn.decomposition._nmf._multiplicative_update_h(X^T, Hst^T, Wst^T, beta_loss, 0, 0, 1)`.  The shift itself (Hs_tau[r, t] =
H[r, t - tau] inside t's utterance, else 0) is written out here, independently of tests/deconv_learn_restatement.py.
Offsets [0, 37, 37, 40, 90]: an empty utterance and a 3-frame one, shorter than the 4 taps.

Writes tests/golden/deconvlearn_dicthalf_{fro,kl}_m25_r12_t90_l4.npz: X (M, T), W0 (L, M, R), H0 (R, T), offsets, W (L, M, R)
after one dictionary half, loss.  Run on the development machine only.

    python tools/make_golden_deconv_learn.py [--check]     (--check: recompute and compare instead of writing)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
M, R, T, L = 25, 12, 90, 4
OFFSETS = [0, 37, 37, 40, 90]


def stacked_shifted(H, offsets, taps):
    """(taps * R, T): block tau holds H moved tau frames to the right inside every utterance"""
    blocks = []
    for tau in range(taps):
        Hs = np.zeros_like(H)
        for t in range(H.shape[1]):
            u = max(i for i in range(len(offsets) - 1) if offsets[i] <= t)        # the last utterance that starts at or before t
            if t - tau >= offsets[u]:
                Hs[:, t] = H[:, t - tau]
        blocks.append(Hs)
    return np.concatenate(blocks, axis=0)


def inputs(seed):
    rng = np.random.default_rng(seed)
    Ws = rng.random((L, M, R)) + 1e-3
    Hs = rng.random((R, T)) * (rng.random((R, T)) < 0.4)
    X = np.concatenate(list(Ws), axis=1) @ stacked_shifted(Hs, OFFSETS, L) + 1e-6
    return X, rng.random((L, M, R)) + 0.1, rng.random((R, T)) + 0.1


def dict_half(X, W0, H0, beta):
    from sklearn.decomposition._nmf import _multiplicative_update_h
    Wst = np.concatenate(list(W0), axis=1)                       # (M, L R)
    Hst = stacked_shifted(H0, OFFSETS, L)                        # (L R, T)
    out = _multiplicative_update_h(np.ascontiguousarray(X.T), np.ascontiguousarray(Hst.T), np.ascontiguousarray(Wst.T), beta,
                                   0, 0, 1.0)
    return np.ascontiguousarray(out.T).reshape(M, L, R).transpose(1, 0, 2).copy()


def main():
    check = "--check" in sys.argv
    bad = 0
    for loss, beta, seed in (("fro", 2, 901), ("kl", 1, 902)):
        X, W0, H0 = inputs(seed)
        out = dict(X=X, W0=W0, H0=H0, offsets=np.array(OFFSETS, dtype=np.int32), W=dict_half(X, W0, H0, beta),
                   loss="frobenius" if beta == 2 else "kullback-leibler")
        path = os.path.join(GOLDEN, f"deconvlearn_dicthalf_{loss}_m{M}_r{R}_t{T}_l{L}.npz")
        if check:
            ref = np.load(path)
            same = all(np.array_equal(np.asarray(ref[k]), np.asarray(v)) for k, v in out.items())
            print(os.path.basename(path), "same" if same else "DIFFERENT")
            bad += not same
        else:
            np.savez_compressed(path, **out)
            print(os.path.basename(path), os.path.getsize(path), "bytes")
    return bad


if __name__ == "__main__":
    sys.exit(main())
