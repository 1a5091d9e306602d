"""Benchmark of mini-batch dictionary learning (evc_online_learn): one JSON line per measurement, appended to
profiles/online_bench.jsonl.  At the compaction shape of tools/bench_beta_learn.py (bench_learn.CONFIGS):

  online    per-step and per-pass time at each batch size, from the HIP events evc_online_opts.ev_loop_start /
            ev_loop_stop around --passes passes (median of --repeats calls after --warmup): once as a pure enqueue (stop
            rules off, nothing asked back) and once with the traces asked for (the host reads three doubles per step)
  full      one evc_beta_learn iteration at the same shape and beta (the full-batch learner: every frame between two
            dictionary updates)
  sklearn   wall time of MiniBatchNMF(init='custom', max_iter=1, tol=0, max_no_improvement=None).fit_transform on the
            CPU of the machine the tool runs on: one pass of the same call

    python tools/bench_online.py [--configs compaction] [--beta 2] [--batch-sizes 1024,4096] [--passes 2] [--repeats R]
                                 [--warmup W] [--no-sklearn] [--out FILE]
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_learn import CONFIGS, problem  # noqa: E402


def _events():
    import torch
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    ev[0].record()
    ev[1].record()          # force creation of the underlying hipEvent_t
    return ev


def run_online(name, M, R, T, dt, beta, bs, passes, repeats, warmup, traced):
    import torch
    from exemplars_vc_amd import _lib, learn_dictionary_online
    X, W0, H0 = problem(M, R, T, 17, dt)
    dev = torch.device("cuda", 0)
    Xd, Wd, Hd = (torch.from_numpy(a).to(dev) for a in (X, W0, H0))
    ev = _events()
    steps = passes * -(-T // min(bs, T))
    times, walls = [], []
    for r in range(warmup + repeats):
        t0 = time.perf_counter()
        out = learn_dictionary_online(Xd, Wd, Hd, beta=beta, layout="bin_major", batch_size=bs, max_iter=passes, tol=0.0,
                                      max_no_improvement=None, info=traced, loop_events=ev)
        torch.cuda.synchronize()
        if r >= warmup:
            walls.append(time.perf_counter() - t0)
            times.append(ev[0].elapsed_time(ev[1]) * 1e-3)
    assert bool(torch.isfinite(out[0]).all()) and bool(torch.isfinite(out[1]).all())
    L = _lib.lib()
    t = float(np.median(times))
    fused = int(L.evc_beta_learn_route(M, R, T)) == 1
    return {"what": "online", "config": name, "beta": beta, "M": M, "R": R, "T": T, "dtype": np.dtype(dt).name,
            "batch_size": bs, "passes": passes, "steps": steps, "traced": traced, "route": "fused" if fused else "unfused",
            "splits_per_batch": int(L.evc_online_splits(M, R, min(bs, T))),
            "launches_per_step": (6 if fused else 8) + (2 if traced else 0),
            "ms_per_step": 1e3 * t / steps, "s_per_pass": t / passes, "wall_s_per_pass": float(np.median(walls)) / passes,
            "spread_ms_per_step": 1e3 * (max(times) - min(times)) / steps, "repeats": repeats}


def run_full(name, M, R, T, dt, beta, iters, repeats, warmup):
    import torch
    from exemplars_vc_amd import learn_dictionary_beta
    X, W0, H0 = problem(M, R, T, 17, dt)
    dev = torch.device("cuda", 0)
    Xd, Wd, Hd = (torch.from_numpy(a).to(dev) for a in (X, W0, H0))
    ev = _events()
    times = []
    for r in range(warmup + repeats):
        _, _, info = learn_dictionary_beta(Xd, Wd, Hd, beta=beta, layout="bin_major", iters=iters, check_every=0, info=True,
                                           loop_events=ev)
        torch.cuda.synchronize()
        if r >= warmup:
            times.append(ev[0].elapsed_time(ev[1]) * 1e-3)
    return {"what": "full", "config": name, "beta": beta, "M": M, "R": R, "T": T, "dtype": np.dtype(dt).name,
            "iters": iters, "route": info["route"], "splits": info["splits"],
            "ms_per_iter": 1e3 * float(np.median(times)) / iters, "repeats": repeats}


def run_sklearn(name, M, R, T, dt, beta, bs):
    from sklearn.decomposition import MiniBatchNMF
    X, W0, H0 = problem(M, R, T, 17, dt)
    est = MiniBatchNMF(n_components=R, init="custom", batch_size=bs, beta_loss=beta, tol=0.0, max_iter=1,
                       max_no_improvement=None, fresh_restarts=False)
    Xs, Ws, Hs = np.ascontiguousarray(X.T), np.ascontiguousarray(H0.T), np.ascontiguousarray(W0.T)
    t0 = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        est.fit_transform(Xs, W=Ws, H=Hs)
    t = time.perf_counter() - t0
    return {"what": "sklearn", "config": name, "beta": beta, "M": M, "R": R, "T": T, "dtype": np.dtype(dt).name,
            "batch_size": bs, "steps": int(est.n_steps_), "cpu_s_per_pass": t, "cpu_ms_per_step": 1e3 * t / int(est.n_steps_),
            "cpus": len(os.sched_getaffinity(0))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="compaction")
    ap.add_argument("--beta", type=float, default=2.0)
    ap.add_argument("--batch-sizes", default="1024,4096")
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "online_bench.jsonl"))
    a = ap.parse_args()
    with open(a.out, "a") as f:
        def emit(r):
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        for name in a.configs.split(","):
            M, R, T, dt, _ = CONFIGS[name]
            for bs in (int(b) for b in a.batch_sizes.split(",")):
                for traced in (False, True):
                    emit(run_online(name, M, R, T, dt, a.beta, bs, a.passes, a.repeats, a.warmup, traced))
            emit(run_full(name, M, R, T, dt, a.beta, 5, a.repeats, a.warmup))
            if not a.no_sklearn:
                for bs in (int(b) for b in a.batch_sizes.split(",")):
                    emit(run_sklearn(name, M, R, T, dt, a.beta, bs))


if __name__ == "__main__":
    main()
