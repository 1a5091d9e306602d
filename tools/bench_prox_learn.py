"""Benchmark of the sparse dictionary learner (evc_prox_learn): per-step times of the three halves of a step - lasso,
statistics, sweep - one JSON line per shape and element type, appended to profiles/prox_learn_bench.jsonl.

A half is timed by running the step loop with the other two left out (learn_dictionary_sparse(skip=...), measurement only)
between the HIP events ev_loop_start / ev_loop_stop of the entry, over `steps` steps: median of --repeats after --warmup calls,
tol = 0 and nothing asked back, so the call is a pure enqueue.  The statistics and the sweep are timed on the activations and
statistics a whole run of the same steps left behind (after zeros they would multiply nothing).  Reported:
  lasso_ms, stats_ms, sweep_ms, step_ms  per step; `lasso_ms` is evc_prox_solve on the same batch (10 FISTA updates) plus the
                         gather and scatter of the batch
  stats_over_lasso, sweep_over_lasso     the dictionary half's two parts as fractions of the lasso half of the same step
  addmm_ms, stats_over_addmm             torch.addmm(C, H_F, [H_F; X_F]^T, beta=...) on the same shapes, same process
  sweep_launches, sweep_us_per_launch    ceil(N / nb) launches of k_plearn_block (plus the contraction and the residual)

    python tools/bench_prox_learn.py [--configs m50_n512_f64,...] [--steps K] [--repeats R] [--warmup W] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# name -> (M, N, batch size, dtype)
CONFIGS = {
    "m50_n512_f64": (50, 512, 1024, np.float64),
    "m50_n512_f32": (50, 512, 1024, np.float32),
    "m402_n1024_f64": (402, 1024, 1024, np.float64),
    "m402_n1024_f32": (402, 1024, 1024, np.float32),
    "m25_n4096_f64": (25, 4096, 1024, np.float64),
    "m25_n4096_f32": (25, 4096, 1024, np.float32),
}


def median_of(fn, read, repeats, warmup):
    import torch
    times = []
    for r in range(warmup + repeats):
        fn()
        torch.cuda.synchronize()
        if r >= warmup:
            times.append(read())
    return float(np.median(times)), float(min(times)), float(max(times))


def run(name, steps, repeats, warmup):
    import torch
    from exemplars_vc_amd import _lib, learn_dictionary_sparse
    import prox_learn_restatement as plr
    M, N, bs, dt = CONFIGS[name]
    dev = torch.device("cuda", 0)
    tt = torch.float64 if dt == np.float64 else torch.float32
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    ev[0].record()
    ev[1].record()          # force creation of the underlying hipEvent_t
    T = 2 * bs
    epochs = max(steps // 2, 1)
    steps = 2 * epochs
    y, D0 = plr.problem(M, N, T, N + M)
    Xd, Dd = torch.from_numpy(y).to(dev, tt), torch.from_numpy(D0).to(dev, tt)
    kw = dict(alpha=1e-3, layout="frame_major", batch_size=bs, epochs=epochs, tol=0.0)
    # a whole run: the dictionary, activations and statistics the halves are then timed on
    D1, H1, info = learn_dictionary_sparse(Xd, Dd, None, info=True, **kw)
    state = info["state"]
    ms = lambda: ev[0].elapsed_time(ev[1]) / steps      # noqa: E731

    def half(*skip):
        def call():
            learn_dictionary_sparse(Xd, None, None, out_w=D1.clone(), out_h=H1.clone(), state=(state[0].clone(), state[1]),
                                    loop_events=ev, skip=skip, **kw)
        return median_of(call, ms, repeats, warmup)
    step = half()
    lasso = half("statistics", "sweep")
    stats = half("lasso", "sweep")
    sweep = half("lasso", "statistics")
    gather = half("lasso", "statistics", "sweep")       # what every variant carries: the gather and scatter of the batch
    # torch.addmm on the shapes of k_plearn_stats
    Hf = H1[:bs].contiguous()
    Zt = torch.cat([Hf, Xd[:bs]], dim=1).t().contiguous()
    Cm = state[0].clone()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def addmm():
        a.record()
        torch.addmm(Cm, Hf.t(), Zt.t(), beta=0.5, out=Cm)
        b.record()
    addmm_t = median_of(addmm, lambda: a.elapsed_time(b), 4 * repeats, 4 * warmup)
    nb = int(_lib.lib().evc_prox_learn_block(M, _lib.F64 if dt == np.float64 else _lib.F32))
    launches = -(-N // nb)
    own = lambda t: t[0] - gather[0]                    # noqa: E731
    return {"config": name, "M": M, "N": N, "batch": bs, "T": T, "dtype": np.dtype(dt).name, "steps": steps, "lasso_iters": 10,
            "step_ms": step[0], "step_ms_min": step[1], "step_ms_max": step[2],
            "lasso_ms": lasso[0], "lasso_ms_min": lasso[1], "lasso_ms_max": lasso[2],
            "stats_ms": own(stats), "stats_ms_with_gather": stats[0], "sweep_ms": own(sweep), "sweep_ms_with_gather": sweep[0],
            "gather_scatter_ms": gather[0],
            "stats_over_lasso": own(stats) / lasso[0], "sweep_over_lasso": own(sweep) / lasso[0],
            "addmm_ms": addmm_t[0], "addmm_ms_min": addmm_t[1], "stats_over_addmm": own(stats) / addmm_t[0],
            "stats_flop": 2.0 * N * (N + M) * bs, "stats_gflops": 2.0 * N * (N + M) * bs / (own(stats) * 1e-3) / 1e9,
            "block": nb, "sweep_launches": launches, "sweep_us_per_launch": 1e3 * own(sweep) / launches,
            "repeats": repeats, "warmup": warmup}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prox_learn_bench.jsonl"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_prox_learn.py needs a HIP device: a CPU run gives no time")
    with open(a.out, "a") as f:
        for name in a.configs.split(","):
            line = json.dumps(run(name, a.steps, a.repeats, a.warmup))
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
