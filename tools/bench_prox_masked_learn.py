"""Benchmark of the sparse dictionary learner with missing data (evc_prox_masked_learn): per-step times of the three halves of
a step - lasso, statistics, atoms - one JSON line per shape and element type, appended to
profiles/prox_masked_learn_bench.jsonl.

A half is timed as tools/bench_prox_learn.py times it: the step loop with the other two left out
(learn_dictionary_sparse(mask=..., skip=...), measurement only) between the HIP events ev_loop_start / ev_loop_stop of the
entry, over `steps` steps: median of --repeats after --warmup calls, tol = 0 and nothing asked back, so the call is a pure
enqueue; what every variant carries (the gathers and the scatter of the batch) is timed alone and taken off.  The statistics
and the atom update are timed on the activations and statistics a whole run of the same steps left behind.  Reported:
  lasso_ms, stats_ms, atoms_ms, step_ms   per step; `stats_ms` is k_pmlearn_stats and k_pmlearn_q together
  stats_flop, stats_tflops, stats_frac_peak    2 bs M N^2 flop per step against the fp64 / fp32 matrix peak (78.6 / 157.3 TF)
  stats_bytes, stats_tb_per_s             2 M N^2 es bytes per step: the tensor read once and written once
  unmasked_step_ms, step_over_unmasked    evc_prox_learn's whole step at the same shape, same process

    python tools/bench_prox_masked_learn.py [--configs m25_n256_b64_f64,...] [--steps K] [--repeats R] [--warmup W] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK = {np.float64: 78.6e12, np.float32: 157.3e12}
SHAPES = [(25, 256, 64), (25, 256, 256), (201, 256, 256), (25, 1024, 256)]
# name -> (M, N, batch size, dtype)
CONFIGS = {"m%d_n%d_b%d_%s" % (M, N, bs, tag): (M, N, bs, dt) for M, N, bs in SHAPES
           for tag, dt in (("f64", np.float64), ("f32", np.float32))}


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
    from exemplars_vc_amd import learn_dictionary_sparse
    import prox_masked_learn_restatement as pmlr
    M, N, bs, dt = CONFIGS[name]
    dev = torch.device("cuda", 0)
    tt = torch.float64 if dt == np.float64 else torch.float32
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    ev[0].record()
    ev[1].record()          # force creation of the underlying hipEvent_t
    T = 2 * bs
    epochs = max(steps // 2, 1)
    steps = 2 * epochs
    y, D0 = pmlr.problem(M, N, T, N + M)
    mask = pmlr.problem_mask(T, M, N + M)
    Xd, Dd, Wd = (torch.from_numpy(a).to(dev, tt) for a in (y, D0, mask))
    kw = dict(alpha=1e-3, layout="frame_major", batch_size=bs, epochs=epochs, tol=0.0)
    # a whole run: the dictionary, activations and statistics the halves are then timed on
    D1, H1, info = learn_dictionary_sparse(Xd, Dd, None, info=True, mask=Wd, **kw)
    state = info["state"]
    ms = lambda: ev[0].elapsed_time(ev[1]) / steps      # noqa: E731

    def half(*skip):
        def call():
            learn_dictionary_sparse(Xd, None, None, out_w=D1.clone(), out_h=H1.clone(), mask=Wd,
                                    state=(state[0].clone(), state[1].clone(), state[2]), loop_events=ev, skip=skip, **kw)
        return median_of(call, ms, repeats, warmup)
    step = half()
    lasso = half("statistics", "sweep")
    stats = half("lasso", "sweep")
    atoms = half("lasso", "statistics")
    gather = half("lasso", "statistics", "sweep")       # what every variant carries: the gathers and the scatter of the batch
    # evc_prox_learn's step at the same shape
    D2, H2, info2 = learn_dictionary_sparse(Xd, Dd, None, info=True, **kw)
    st2 = info2["state"]

    def unmasked():
        learn_dictionary_sparse(Xd, None, None, out_w=D2.clone(), out_h=H2.clone(), state=(st2[0].clone(), st2[1]), loop_events=ev,
                                **kw)
    plain = median_of(unmasked, ms, repeats, warmup)
    own = lambda t: t[0] - gather[0]                    # noqa: E731
    es = np.dtype(dt).itemsize
    flop, nbytes = 2.0 * bs * M * N * N, 2.0 * M * N * N * es
    t_stats = own(stats) * 1e-3
    return {"config": name, "M": M, "N": N, "batch": bs, "T": T, "dtype": np.dtype(dt).name, "steps": steps, "lasso_iters": 10,
            "step_ms": step[0], "step_ms_min": step[1], "step_ms_max": step[2],
            "lasso_ms": own(lasso), "lasso_ms_with_gather": lasso[0], "stats_ms": own(stats), "stats_ms_with_gather": stats[0],
            "stats_ms_min": stats[1] - gather[0], "stats_ms_max": stats[2] - gather[0],
            "atoms_ms": own(atoms), "atoms_ms_with_gather": atoms[0], "gather_scatter_ms": gather[0],
            "stats_flop": flop, "stats_tflops": flop / t_stats / 1e12, "stats_frac_peak": flop / t_stats / PEAK[dt],
            "stats_bytes": nbytes, "stats_tb_per_s": nbytes / t_stats / 1e12,
            "unmasked_step_ms": plain[0], "step_over_unmasked": step[0] / plain[0],
            "repeats": repeats, "warmup": warmup}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prox_masked_learn_bench.jsonl"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_prox_masked_learn.py needs a HIP device: a CPU run gives no time")
    with open(a.out, "a") as f:
        for name in a.configs.split(","):
            line = json.dumps(run(name, a.steps, a.repeats, a.warmup))
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
