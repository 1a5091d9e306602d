"""Benchmark of the missing-data / factored proximal-gradient solve (evc_prox_masked_solve: k_prox_resid + k_prox_back) against
the Gram sweep (evc_prox_solve: k_prox_sweep) timed in the same run on the same inputs: one JSON line per shape, element type
and variant, appended to profiles/prox_masked_bench.jsonl.

Variants: "null" (mask == NULL: the unmasked problem on the factored sweep) and "binary" (a binary mask that keeps 0.7 of the
bins).  The iteration loops are timed with the HIP events ev_loop_start / ev_loop_stop of both entries (median of --repeats
after --warmup calls; FISTA, tol = 0 so that nothing stops, the statistic evaluated every 10th iteration).  `ratio` = loop time
of the factored sweep / loop time of the Gram sweep.  `bytes_per_iter` is what the two launches must move at the least:
k_prox_resid reads W and the mask and writes R, k_prox_back reads R, W, P and X and writes X and W', each reads one dictionary
image - (6 N T + (2 | 3) M T + 2 M N) elements; `gbps` is that over the measured time.  `bound_ms` is the once-per-call cost of
the Gershgorin bound (k_pm_wbar, k_pm_bound, one per utterance with a mask): whole-call time with the bound minus whole-call
time with `lipschitz` given, both around one update.  Parity: 3 updates with a null mask against evc_prox_solve, relative to
max |x|.

    python tools/bench_prox_masked.py [--configs m25_16utt_f64,...] [--iters K] [--repeats R] [--warmup W] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# name -> (M, N, frames per utterance, utterances, dtype)
CONFIGS = {
    "m25_16utt_f64": (25, 4096, 688, 16, np.float64),
    "m25_16utt_f32": (25, 4096, 688, 16, np.float32),
    "m25_1utt_f64": (25, 4096, 688, 1, np.float64),
    "m25_1utt_f32": (25, 4096, 688, 1, np.float32),
    "m201_16utt_f64": (201, 4096, 688, 16, np.float64),
    "m201_16utt_f32": (201, 4096, 688, 16, np.float32),
    "m513_16utt_f64": (513, 4096, 688, 16, np.float64),      # towards the crossover with the Gram sweep
}


def timed(fn, ev, repeats, warmup):
    import torch
    times = []
    for r in range(warmup + repeats):
        fn()
        torch.cuda.synchronize()
        if r >= warmup:
            times.append(ev[0].elapsed_time(ev[1]) * 1e-3)
    return float(np.median(times)), float(min(times)), float(max(times))


def whole_call(fn, repeats, warmup):
    """median time of the whole call, between two events on the stream"""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for r in range(warmup + repeats):
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if r >= warmup:
            times.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(times))


def run(name, iters, repeats, warmup):
    import torch
    from exemplars_vc_amd import solve_activations_prox
    import prox_masked_restatement as pmr
    import prox_restatement as pr
    M, N, Tu, n_utt, dt = CONFIGS[name]
    dev = torch.device("cuda", 0)
    tt = torch.float64 if dt == np.float64 else torch.float32
    es = np.dtype(dt).itemsize
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    ev[0].record()
    ev[1].record()          # force creation of the underlying hipEvent_t
    T = Tu * n_utt
    offs = np.arange(n_utt + 1, dtype=np.int32) * Tu
    y, A = pr.problem(M, N, T, N + n_utt)
    Ad, Xd = (torch.from_numpy(a).to(dev, tt) for a in (A, y))
    Md = torch.from_numpy(pmr.problem_mask(T, M, 11, "binary", keep=0.7)).to(dev, tt)
    kw = dict(alpha=1e-3, tol=0.0, layout="frame_major", utt_offsets=offs)
    tg, tg_lo, tg_hi = timed(lambda: solve_activations_prox(Ad, Xd, iters=iters, loop_events=ev, **kw), ev, repeats, warmup)
    g3 = solve_activations_prox(Ad, Xd, iters=3, **kw).cpu().numpy().astype(np.float64)
    f3 = solve_activations_prox(Ad, Xd, iters=3, factored=True, **kw).cpu().numpy().astype(np.float64)
    parity = float(np.max(np.abs(f3 - g3)) / np.max(np.abs(g3)))
    out = []
    for variant, mkw in (("null", dict(factored=True)), ("binary", dict(mask=Md))):
        t, lo, hi = timed(lambda: solve_activations_prox(Ad, Xd, iters=iters, loop_events=ev, **mkw, **kw), ev, repeats, warmup)
        with_bound = whole_call(lambda: solve_activations_prox(Ad, Xd, iters=1, **mkw, **kw), repeats, warmup)
        without = whole_call(lambda: solve_activations_prox(Ad, Xd, iters=1, lipschitz=100.0, **mkw, **kw), repeats, warmup)
        nbytes = float(es) * (6.0 * N * T + (3.0 if variant == "binary" else 2.0) * M * T + 2.0 * M * N)
        out.append({"config": name, "variant": variant, "M": M, "N": N, "T": T, "n_utt": n_utt, "dtype": np.dtype(dt).name,
                    "iters": iters, "momentum": "fista", "check_every": 10,
                    "loop_s": t, "loop_s_min": lo, "loop_s_max": hi, "ms_per_iter": 1e3 * t / iters,
                    "gram_loop_s": tg, "gram_loop_s_min": tg_lo, "gram_loop_s_max": tg_hi, "gram_ms_per_iter": 1e3 * tg / iters,
                    "ratio": t / tg, "flop_per_iter": 4.0 * M * N * T, "gram_flop_per_iter": 2.0 * N * N * T,
                    "bytes_per_iter": nbytes, "gbps": nbytes * iters / t / 1e9,
                    "bound_ms": 1e3 * (with_bound - without), "bounds_per_call": n_utt if variant == "binary" else 1,
                    "parity_null_vs_gram_3it": parity, "repeats": repeats, "warmup": warmup,
                    "kernel": "k_prox_resid+k_prox_back", "baseline": "evc_prox_solve k_prox_sweep"})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prox_masked_bench.jsonl"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_prox_masked.py needs a HIP device: a CPU run gives no time")
    with open(a.out, "a") as f:
        for name in a.configs.split(","):
            for rec in run(name, a.iters, a.repeats, a.warmup):
                line = json.dumps(rec)
                print(line, flush=True)
                f.write(line + "\n")


if __name__ == "__main__":
    main()
