#!/usr/bin/env python3
"""Generate tests/golden/mus_*.npz - runs ONLY where the vendored deComP lies (the build container).

tools/make_golden_mu_masked.py's recipe for deComP's mini-batch NMF: the vectors are produced by executing deComP's own
`nmf.solve(minibatch=bs, method=...)` from where it lies, unmodified, behind the same placeholder `chainer` package.  Nothing
of deComP's source text is written into the fixtures: each .npz holds data only - the inputs (float32-representable values,
stored as float32), the mask, the order rows deComP's shuffles amount to, the options, and the recorded `it`, D, x and the
statistics of every dictionary update.

A case that names `want` ("mid": the call stops inside an epoch, "last": at an epoch's last step) gets its tol from a run
without a stop: the first update inside (at the end of) an epoch whose statistic lies below every earlier one, tol halfway
(geometrically) between the two.  Per fixture the script asserts
  * that tests/mu_stoch_restatement.py reproduces deComP's (it, D, x) to the last bit, and records a fingerprint of this
    machine's BLAS (`blas_crc`);
  * that no statistic lies within 1e-6 tol of tol; that the mask, where there is one, has a zero and a non-zero;
  * that the permutation figures (atoms, bins and the frames inside a batch permuted; `perm64`, `perm32`) are positive and
    100 perm64 <= 1e-9 - else the next seed is tried.  100 times the figure is the GPU tests' bound.
Over the set: every one of the six method names, both losses, mask and no mask, T mod bs != 0 in at least half the fixtures,
one stop inside an epoch, one at an epoch's last step, one run to maxiter, one svrmu-acc fixture with inner_iters >= 2."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import mu_masked_restatement as mmr  # noqa: E402
import mu_stoch_restatement as msr  # noqa: E402
from make_golden_prox import import_decomp  # noqa: E402

CASES = [
    dict(name="mus_asg_m25_r8_t50_bs16_l2_mask", method="asg-mu", shape=(25, 8, 50), bs=16, loss="l2", kind="binary",
         maxiter=13, tol=1e-9),
    dict(name="mus_gsg_m40_r19_t70_bs16_kl", method="gsg-mu", shape=(40, 19, 70), bs=16, loss="kl", kind=None, maxiter=13,
         tol=1e-9, start=True),
    dict(name="mus_asag_m201_r12_t40_bs16_kl_mask", method="asag-mu", shape=(201, 12, 40), bs=16, loss="kl", kind="weights",
         maxiter=13, tol=1e-9, forget_rate=0.3),
    dict(name="mus_asag_m40_r19_t70_bs16_l2_mid", method="asag-mu", shape=(40, 19, 70), bs=16, loss="l2", kind="binary",
         maxiter=31, want="mid"),
    dict(name="mus_gsag_m25_r8_t50_bs7_l2_last", method="gsag-mu", shape=(25, 8, 50), bs=7, loss="l2", kind=None, maxiter=41,
         want="last", start=True),
    dict(name="mus_svrmu_m40_r19_t70_bs16_l2_mask", method="svrmu", shape=(40, 19, 70), bs=16, loss="l2", kind="weights",
         maxiter=200, tol=2e-3),
    dict(name="mus_svrmu_m25_r8_t48_bs16_kl_mask", method="svrmu", shape=(25, 8, 48), bs=16, loss="kl", kind="binary",
         maxiter=9, tol=1e-9, alpha=0.75, start=True),
    dict(name="mus_svrmuacc_m25_r8_t50_bs16_kl", method="svrmu-acc", shape=(25, 8, 50), bs=16, loss="kl", kind=None,
         maxiter=13, tol=1e-9, beta=2.0),
    dict(name="mus_asg_m2_r3_t5_bs2_kl", method="asg-mu", shape=(2, 3, 5), bs=2, loss="kl", kind=None, maxiter=7, tol=1e-9),
]


def options(c):
    kasai = c["method"] in ("svrmu", "svrmu-acc")
    kw = dict(alpha=c.get("alpha", 1.0), beta=c.get("beta", 0.5)) if kasai else dict(forget_rate=c.get("forget_rate", 0.5))
    M, R, T = c["shape"]
    inner = msr.svrmu_acc_inner(R, M, T, kw["beta"]) if c["method"] == "svrmu-acc" else 1
    return kw, inner


def restated(c, y, D0, x0, mask, order, tol, dtype=np.float64):
    kw, inner = options(c)
    return msr.learn(y, D0, x0, mask=mask, method=msr.NATIVE[c["method"]], loss=c["loss"], batch_size=c["bs"],
                     epochs=c["maxiter"] - 1, tol=tol, forget_rate=kw.get("forget_rate", 0.5), alpha=kw.get("alpha", 1.0),
                     inner_iters=inner, order=order, dtype=dtype)


def pick_tol(stats, n_loop, want, gsag):
    """tol that stops the run at the first update of the wanted kind whose statistic lies below every earlier one"""
    for k in range(2 if gsag else n_loop + 1, len(stats)):      # not before the second epoch (gsag: the third)
        last = True if gsag else (k % n_loop == n_loop - 1)
        if (want == "last") != last or not stats[k] < np.min(stats[:k]):
            continue
        return float(np.sqrt(stats[k] * np.min(stats[:k])))
    return None


def one_case(nmf, c, seed):
    M, R, T = c["shape"]
    loss, bs, maxiter = c["loss"], c["bs"], c["maxiter"]
    y, _ = mmr.problem(M, R, T, seed)
    y = y.astype(np.float32).astype(np.float64)
    rng = np.random.default_rng(seed + 300)
    D0 = np.round((rng.random((R, M)) + 0.05) * 256.0) / 256.0
    x0 = np.round((rng.random((T, R)) + 0.125) * 256.0) / 256.0 if c.get("start") else None
    mask = None if c["kind"] is None else mmr.problem_mask(T, M, seed, c["kind"])
    assert (y >= 0).all() and (D0 > 0).all()
    if mask is not None:
        assert (mask == 0).any() and (mask > 0).any() and (mask >= 0).all()
    kw, inner = options(c)
    native = msr.NATIVE[c["method"]]
    order = msr.frame_orders(T, maxiter - 1, seed, native)
    n_loop = T // bs
    tol = c.get("tol")
    if c.get("want"):
        free = restated(c, y, D0, x0, mask, order, 0.0)
        tol = pick_tol(free["stats"], n_loop, c["want"], native == "gsag")
        if tol is None:
            return None
    it, D, x = nmf.solve(y.copy(), D0.copy(), None if x0 is None else x0.copy(), tol=tol, minibatch=bs, maxiter=maxiter,
                         method=c["method"], likelihood=loss, mask=None if mask is None else mask.copy(), random_seed=seed, **kw)
    if not (np.isfinite(D).all() and np.isfinite(x).all() and x.any()):
        return None
    r = restated(c, y, D0, x0, mask, order, tol)
    assert int(it) == r["it"] and np.array_equal(D, r["D"]) and np.array_equal(x, r["x"]), (c["name"], "restatement differs")
    stats = r["stats"]
    if np.min(np.abs(stats - tol)) < 1e-6 * tol:
        return None
    stopped = int(it) < maxiter
    where = "max" if not stopped else "last" if r["n_steps"] % n_loop == 0 else "mid"
    if c.get("want") and where != c["want"]:
        return None
    p64 = msr.permutation_figure(y, D0, mask, np.float64, x0=x0, seed=seed + 1000, floor=False, method=native, loss=loss,
                                 batch_size=bs, epochs=r["n_epochs"], forget_rate=kw.get("forget_rate", 0.5),
                                 alpha=kw.get("alpha", 1.0), inner_iters=inner, order=order)
    p32 = msr.permutation_figure(y, D0, mask, np.float32, x0=x0, seed=seed + 1000, floor=False, method=native, loss=loss,
                                 batch_size=bs, epochs=r["n_epochs"], forget_rate=kw.get("forget_rate", 0.5),
                                 alpha=kw.get("alpha", 1.0), inner_iters=inner, order=order)
    if not (p64 > 0 and p32 > 0 and 100 * p64 <= 1e-9):
        return None
    out = dict(y=y.astype(np.float32), D0=D0.astype(np.float32), order=order, D=D, x=x, it=int(it), stats=stats,
               n_steps=r["n_steps"], n_epochs=r["n_epochs"], visited=r["visited"], tol=tol, maxiter=maxiter, bs=bs, loss=loss,
               method=c["method"], inner_iters=inner, forget_rate=kw.get("forget_rate", 0.5), alpha=kw.get("alpha", 1.0),
               beta=kw.get("beta", 0.5), seed=seed, where=where, perm64=p64, perm32=p32,
               blas_crc=np.array(mmr.blas_fingerprint(y, D0, np.ones_like(y) if mask is None else mask), dtype=np.int64))
    if mask is not None:
        out["mask"] = mask.astype(np.float32)
    if x0 is not None:
        out["x0"] = x0.astype(np.float32)
    path = os.path.join(OUT, c["name"] + ".npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < (1 << 20)
    print("%-40s it=%d/%d steps=%d %s tol=%.3g inner=%d perm64=%.2e perm32=%.2e  %d bytes" % (
        c["name"], int(it), maxiter, r["n_steps"], where, tol, inner, p64, p32, os.path.getsize(path)))
    return out


def main():
    import_decomp()
    from decomp import nmf
    outs = []
    for k, c in enumerate(CASES):
        seed = 2100 + 50 * k
        while True:
            out = one_case(nmf, c, seed)
            if out is not None:
                break
            print("%s: rejected at seed %d: trying the next" % (c["name"], seed))
            seed += 1
            assert seed < 2100 + 50 * k + 50, c["name"]
        outs.append(out)
    assert {o["method"] for o in outs} == set(msr.NATIVE)
    assert {o["loss"] for o in outs} == {"l2", "kl"}
    assert any("mask" in o for o in outs) and any("mask" not in o for o in outs)
    assert 2 * sum(o["y"].shape[0] % o["bs"] != 0 for o in outs) >= len(outs)
    assert {"mid", "last", "max"} <= {o["where"] for o in outs}
    assert any(o["method"] == "svrmu-acc" and o["inner_iters"] >= 2 for o in outs)


if __name__ == "__main__":
    main()
