"""Benchmark of the mini-batch estimator's activation solve (evc_online_transform) against the plain beta-divergence solve
(evc_beta_solve): one JSON line per measurement, appended to profiles/online_transform_bench.jsonl.

  compaction  the shape of tools/bench_online.py (bench_learn.CONFIGS["compaction"]: 50 bins, 512 atoms, 65536 frames,
              float64), one utterance
  vc          one conversion-shaped call: 16 utterances of 688 frames, 201 bins, 512 exemplars, float32

Per shape, --iters iterations without a stop (tol = 0), timed by the HIP events around the iteration loop (ev_loop_start /
ev_loop_stop): `transform_online(tol=0, max_iter=K)` - K launches of the change variant of k_beta_sweep and K of
k_beta_change_check - against `solve_activations_beta(init="sklearn", iters=K, check_every=0)` - K launches of the plain
sweep.  The two are run alternately, --repeats times each after --warmup; reported are the medians, the spread (max - min)
of each, their ratio and the extra time per iteration.  With a package that has no transform_online (an earlier commit) only
the plain solve is measured: the baseline.

  fresh       for orientation, at the compaction shape: one pass of learn_dictionary_online(fresh_restarts=True,
              fresh_restarts_max_iter=F, transform_max_iter=0) against one plain pass at the same batch size, both as pure
              enqueues (tol = 0, stop rules off), timed by the events around the step loop

    python tools/bench_online_transform.py [--configs compaction,vc] [--beta 2] [--iters K] [--repeats R] [--warmup W]
                                           [--fresh-batch 1024] [--fresh-iters 30] [--tag NAME] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_learn import CONFIGS, problem  # noqa: E402

SHAPES = {"compaction": CONFIGS["compaction"][:4] + (1,), "vc": (201, 512, 16 * 688, np.float32, 16)}


def _events():
    import torch
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    ev[0].record()
    ev[1].record()          # force creation of the underlying hipEvent_t
    return ev


def run(name, beta, iters, repeats, warmup):
    import torch
    import exemplars_vc_amd as evc
    M, R, T, dt, n_utt = SHAPES[name]
    X, W, _ = problem(M, R, T, 17, dt)
    dev = torch.device("cuda", 0)
    Xd, Wd = torch.from_numpy(X).to(dev), torch.from_numpy(W).to(dev)
    offs = [u * (T // n_utt) for u in range(n_utt)] + [T]
    ev = _events()
    have = hasattr(evc, "transform_online")
    calls = {"beta_solve": lambda: evc.solve_activations_beta(Wd, Xd, beta=beta, layout="bin_major", init="sklearn", iters=iters,
                                                              check_every=0, utt_offsets=offs, loop_events=ev)}
    if have:
        calls["transform"] = lambda: evc.transform_online(Wd, Xd, beta=beta, layout="bin_major", max_iter=iters, tol=0.0,
                                                          utt_offsets=offs, loop_events=ev)
    times = {k: [] for k in calls}
    out = {}
    for r in range(warmup + repeats):
        for k, fn in calls.items():
            out[k] = fn()
            torch.cuda.synchronize()
            if r >= warmup:
                times[k].append(ev[0].elapsed_time(ev[1]) * 1e-3)
    rec = {"what": "online_transform", "config": name, "beta": beta, "M": M, "R": R, "T": T, "n_utt": n_utt,
           "dtype": np.dtype(dt).name, "iters": iters, "repeats": repeats}
    for k, v in times.items():
        rec[k + "_ms_per_iter"] = 1e3 * float(np.median(v)) / iters
        rec[k + "_spread_ms_per_iter"] = 1e3 * (max(v) - min(v)) / iters
    if have:
        assert bool(torch.equal(out["transform"], out["beta_solve"]))       # tol = 0: the same activations, bitwise
        rec["ratio"] = rec["transform_ms_per_iter"] / rec["beta_solve_ms_per_iter"]
        rec["extra_us_per_iter"] = 1e3 * (rec["transform_ms_per_iter"] - rec["beta_solve_ms_per_iter"])
    return rec


def run_fresh(beta, bs, fresh_iters, repeats, warmup):
    import torch
    import exemplars_vc_amd as evc
    M, R, T, dt, _ = SHAPES["compaction"]
    X, W0, H0 = problem(M, R, T, 17, dt)
    dev = torch.device("cuda", 0)
    Xd, Wd, Hd = (torch.from_numpy(a).to(dev) for a in (X, W0, H0))
    ev = _events()
    kw = dict(beta=beta, layout="bin_major", batch_size=bs, max_iter=1, tol=0.0, max_no_improvement=None, loop_events=ev)
    calls = {"plain": lambda: evc.learn_dictionary_online(Xd, Wd, Hd, **kw),
             "fresh": lambda: evc.learn_dictionary_online(Xd, Wd, None, fresh_restarts=True, fresh_restarts_max_iter=fresh_iters,
                                                          transform_max_iter=0, **kw)}
    times = {k: [] for k in calls}
    for r in range(warmup + repeats):
        for k, fn in calls.items():
            out = fn()
            torch.cuda.synchronize()
            assert bool(torch.isfinite(out[0]).all())
            if r >= warmup:
                times[k].append(ev[0].elapsed_time(ev[1]) * 1e-3)
    steps = -(-T // bs)
    rec = {"what": "fresh_pass", "config": "compaction", "beta": beta, "M": M, "R": R, "T": T, "dtype": np.dtype(dt).name,
           "batch_size": bs, "steps": steps, "fresh_max_iter": fresh_iters, "repeats": repeats}
    for k, v in times.items():
        rec[k + "_ms_per_pass"] = 1e3 * float(np.median(v))
        rec[k + "_spread_ms_per_pass"] = 1e3 * (max(v) - min(v))
    rec["ratio"] = rec["fresh_ms_per_pass"] / rec["plain_ms_per_pass"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="compaction,vc")
    ap.add_argument("--beta", type=float, default=2.0)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--fresh-batch", type=int, default=1024, help="batch size of the fresh-restart pass (0: skip it)")
    ap.add_argument("--fresh-iters", type=int, default=30)
    ap.add_argument("--tag", default="", help="copied into every record (which build was measured)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "online_transform_bench.jsonl"))
    a = ap.parse_args()
    with open(a.out, "a") as f:
        import exemplars_vc_amd as evc
        recs = [run(name, a.beta, a.iters, a.repeats, a.warmup) for name in a.configs.split(",")]
        if a.fresh_batch and hasattr(evc, "transform_online"):
            recs.append(run_fresh(a.beta, a.fresh_batch, a.fresh_iters, a.repeats, a.warmup))
        for rec in recs:
            if a.tag:
                rec["tag"] = a.tag
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()


if __name__ == "__main__":
    main()
