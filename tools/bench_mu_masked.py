"""Benchmark of the missing-data multiplicative-update solve (evc_mu_masked_solve, k_mum_sweep): one JSON line per shape, loss
and mask, appended to profiles/mu_masked_bench.jsonl.

The iteration loop is timed with the HIP events evc_mu_masked_opts.ev_loop_start / ev_loop_stop (median of --repeats calls
after --warmup, no error checks inside the loop).  In the same run evc_beta_solve (k_beta_sweep, the untouched yardstick on
the same geometry) is timed at the same shape and iteration count with beta = 2 for the l2 rows and beta = 1 for the kl rows:
`ratio_to_beta` = loop time of the masked solve / loop time of the beta solve.  Both kernels do 6 M N flop per frame and
iteration, so arithmetic predicts a ratio near 1; no target is fixed.  Lines whose `variant` is not "current" were recorded with
a kernel variant that is no longer in the tree (DESIGN.md §5.22 says which).

    python tools/bench_mu_masked.py [--configs stft_f32_16utt,c2_batch] [--iters K] [--repeats R] [--warmup W]
                                    [--out profiles/mu_masked_bench.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# name -> (M, N, frames per utterance, utterances, dtype, iterations)
CONFIGS = {
    "stft_f32_16utt": (201, 4096, 688, 16, np.float32, 20),
    "c2_batch": (25, 4096, 688, 256, np.float64, 20),
}


def problem(M, N, T, seed):
    rng = np.random.default_rng(seed)
    W = rng.random((N, M)) ** 2 + 1e-3
    X = (rng.random((T, 64)) * (rng.random((T, 64)) < 0.2)) @ W[:64] + 1e-3 * rng.random((T, M)) + 1e-4
    mask = (rng.random((T, M)) < 0.7).astype(np.float64)
    return X, W, mask


def timed(fn, ev, repeats, warmup):
    import torch
    times = []
    for r in range(warmup + repeats):
        fn()
        torch.cuda.synchronize()
        if r >= warmup:
            times.append(ev[0].elapsed_time(ev[1]) * 1e-3)
    return float(np.median(times)), float(min(times)), float(max(times))


def run(name, iters_override, repeats, warmup):
    import torch
    from exemplars_vc_amd import solve_activations_beta, solve_activations_masked
    M, N, Tu, n_utt, dt, iters = CONFIGS[name]
    iters = iters_override or iters
    T = Tu * n_utt
    X, W, mask = problem(M, N, T, M * 7919 + N)
    dev = torch.device("cuda", 0)
    tt = torch.float64 if dt == np.float64 else torch.float32
    Wd, Xd, Md = (torch.from_numpy(m).to(dev, tt) for m in (W, X, mask))
    offs = np.arange(n_utt + 1, dtype=np.int32) * Tu
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    ev[0].record()
    ev[1].record()          # force creation of the underlying hipEvent_t
    out = []
    for loss, beta in (("frobenius", 2.0), ("kl", 1.0)):
        t_b, b_lo, b_hi = timed(lambda: solve_activations_beta(Wd, Xd, beta=beta, layout="frame_major", iters=iters, init="const",
                                                               init_value=1.0, utt_offsets=offs, loop_events=ev), ev, repeats, warmup)
        for masked in (False, True):
            def call():
                return solve_activations_masked(Wd, Xd, Md if masked else None, loss=loss, layout="frame_major", iters=iters,
                                                utt_offsets=offs, loop_events=ev)
            t, lo, hi = timed(call, ev, repeats, warmup)
            rec = {"variant": "current", "config": name, "loss": loss, "masked": masked, "M": M, "N": N, "T": T, "n_utt": n_utt,
                   "dtype": np.dtype(dt).name, "iters": iters, "loop_s": t, "loop_s_min": lo, "loop_s_max": hi,
                   "ms_per_iter": 1e3 * t / iters, "beta": beta, "beta_loop_s": t_b, "beta_loop_s_min": b_lo, "beta_loop_s_max": b_hi,
                   "beta_ms_per_iter": 1e3 * t_b / iters, "ratio_to_beta": t / t_b, "repeats": repeats, "warmup": warmup,
                   "kernel": "k_mum_sweep"}
            out.append(rec)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--iters", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mu_masked_bench.jsonl"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mu_masked.py needs a HIP device: a CPU run gives no time")
    with open(a.out, "a") as f:
        for name in a.configs.split(","):
            for rec in run(name, a.iters, a.repeats, a.warmup):
                line = json.dumps(rec)
                print(line, flush=True)
                f.write(line + "\n")


if __name__ == "__main__":
    main()
