"""Benchmark of dictionary learning under a beta-divergence (evc_beta_learn): one JSON line per measurement, appended to
profiles/beta_learn_bench.jsonl.

  loop      per-iteration time of the whole loop from the HIP events evc_beta_learn_opts.ev_loop_start / ev_loop_stop
            (20 iterations, median of --repeats calls after --warmup), with the dictionary route forced to "fused" and to
            "unfused" (a shape the fused kernel does not hold is reported as such); beside it, from torch events, one
            activation step on its own (one evc_beta_solve call with iters = 1: packing and the sweep).  The dictionary
            half is the difference; it is priced at 6 M R T flop, the activation half at (6 M R + 3 R) T, against the
            dtype's matrix peak (78.6 TF float64, 157.3 TF float32)
  sweep     (--sweep) the same at R = 16 .. 256 on the two shapes' M and T: where the fused route stops paying
  yardstick tools/bench_learn.py run in the same session gives evc_nmf_learn (Frobenius and KL) at the same shapes: the
            only dictionary learning that existed before

    python tools/bench_beta_learn.py [--configs compaction,stft_pair] [--betas 0,0.5] [--iters K] [--repeats R]
                                     [--warmup W] [--sweep] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_learn import CONFIGS, PEAK, problem  # noqa: E402

SWEEP_R = (16, 32, 64, 128, 256)


def run_loop(name, M, R, T, dt, beta, route, iters, repeats, warmup):
    import torch
    from exemplars_vc_amd import _lib, learn_dictionary_beta, solve_activations_beta
    X, W0, H0 = problem(M, R, T, 17, dt)
    dev = torch.device("cuda", 0)
    Xd, Wd, Hd = (torch.from_numpy(a).to(dev) for a in (X, W0, H0))
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    ev[0].record()
    ev[1].record()          # force creation of the underlying hipEvent_t
    base = {"what": "loop", "config": name, "beta": beta, "route": route, "M": M, "R": R, "T": T,
            "dtype": np.dtype(dt).name, "iters": iters}
    times = []
    for r in range(warmup + repeats):
        try:
            W, H, info = learn_dictionary_beta(Xd, Wd, Hd, beta=beta, layout="bin_major", iters=iters, check_every=0,
                                               info=True, loop_events=ev, route=route)
        except _lib.EvcError as e:
            return dict(base, unsupported=e.status)
        torch.cuda.synchronize()
        if r >= warmup:
            times.append(ev[0].elapsed_time(ev[1]) * 1e-3)
    assert bool(torch.isfinite(W).all()) and bool(torch.isfinite(H).all())
    t = float(np.median(times))
    a0, a1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    solve_activations_beta(Wd, Xd, Hd, beta=beta, layout="bin_major", iters=1)
    a0.record()
    for _ in range(10):
        solve_activations_beta(Wd, Xd, Hd, beta=beta, layout="bin_major", iters=1)
    a1.record()
    torch.cuda.synchronize()
    act_ms = a0.elapsed_time(a1) / 10
    ms = 1e3 * t / iters
    dict_ms = max(ms - act_ms, 1e-9)
    return dict(base, splits=info["splits"], loop_s=t, ms_per_iter=ms, activation_step_ms=act_ms, dictionary_half_ms=dict_ms,
                dictionary_frac_peak=6.0 * M * R * T / (dict_ms * 1e-3) / PEAK[dt],
                activation_frac_peak=(6.0 * M * R + 3.0 * R) * T / (act_ms * 1e-3) / PEAK[dt],
                spread_ms_per_iter=1e3 * (max(times) - min(times)) / iters, repeats=repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--betas", default="0,0.5")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beta_learn_bench.jsonl"))
    a = ap.parse_args()
    betas = [float(b) for b in a.betas.split(",")]
    with open(a.out, "a") as f:
        def emit(r):
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        for name in a.configs.split(","):
            M, R, T, dt, _ = CONFIGS[name]
            for beta in betas:
                for route in ("fused", "unfused"):
                    emit(run_loop(name, M, R, T, dt, beta, route, a.iters, a.repeats, a.warmup))
            if a.sweep:
                for Rs in SWEEP_R:
                    for route in ("fused", "unfused"):
                        emit(dict(run_loop(name, M, Rs, T, dt, betas[0], route, a.iters, a.repeats, a.warmup), what="sweep"))


if __name__ == "__main__":
    main()
