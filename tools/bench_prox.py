"""Benchmark of the proximal-gradient activation solve (evc_prox_solve: k_prox_sweep): one JSON line per shape and element
type, appended to profiles/prox_bench.jsonl.

The iteration loop is timed with the HIP events evc_prox_opts.ev_loop_start / ev_loop_stop (median of --repeats after
--warmup calls; FISTA, tol = 0 so that nothing stops, with the stop statistic evaluated every 10th iteration as deComP does
and, as `nocheck_*`, never).  flop = 2 N^2 T per iteration: one N x N contraction against W.  In the same run evc_semi_solve is
timed at the same N, frames and element type: its sweep (k_semi_sweep) issues exactly twice the MFMAs per output and writes
one array where this one writes two - `ratio_to_semi` = loop time of the prox sweep / loop time of the semi sweep (0.5 if
the matrix cores alone decided).  Parity: 3 iterations on the first 64 frames against the numpy restatement
(tests/prox_restatement.py).

    python tools/bench_prox.py [--configs n4096_f64,...] [--iters K] [--repeats R] [--warmup W] [--out profiles/prox_bench.jsonl]
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

# name -> (M, N, frames per utterance, utterance counts, dtype)
CONFIGS = {
    "n4096_f64": (25, 4096, 688, (16, 1), np.float64),
    "n4096_f32": (25, 4096, 688, (16, 1), np.float32),
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


def run(name, iters, repeats, warmup):
    import torch
    from exemplars_vc_amd import solve_activations_prox, solve_activations_semi
    import prox_restatement as pr
    M, N, Tu, utt_counts, dt = CONFIGS[name]
    dev = torch.device("cuda", 0)
    tt = torch.float64 if dt == np.float64 else torch.float32
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    ev[0].record()
    ev[1].record()          # force creation of the underlying hipEvent_t
    out = []
    for n_utt in utt_counts:
        T = Tu * n_utt
        offs = np.arange(n_utt + 1, dtype=np.int32) * Tu
        y, A = pr.problem(M, N, T, N + n_utt)
        Ad, Xd = (torch.from_numpy(a).to(dev, tt) for a in (A, y))
        Hd = torch.rand((T, N), dtype=tt, device=dev) + 1e-4
        kw = dict(alpha=1e-3, iters=iters, tol=0.0, layout="frame_major", utt_offsets=offs, loop_events=ev)
        ts, ts_lo, ts_hi = timed(lambda: solve_activations_semi(Ad, Xd, Hd, iters=iters, layout="frame_major", utt_offsets=offs,
                                                                loop_events=ev), ev, repeats, warmup)
        t, lo, hi = timed(lambda: solve_activations_prox(Ad, Xd, **kw), ev, repeats, warmup)
        tn, tn_lo, tn_hi = timed(lambda: solve_activations_prox(Ad, Xd, check_every=0, **kw), ev, repeats, warmup)
        act = solve_activations_prox(Ad, Xd[:64].contiguous(), alpha=1e-3, iters=3, tol=0.0, layout="frame_major")
        act = act.cpu().numpy().astype(np.float64)
        ref = pr.solve(y[:64], A, 1e-3, iters=3, tol=0.0)[0]
        flop = float(iters) * 2.0 * N * N * T
        out.append({"config": name, "M": M, "N": N, "T": T, "n_utt": n_utt, "dtype": np.dtype(dt).name, "iters": iters,
                    "momentum": "fista", "check_every": 10,
                    "loop_s": t, "loop_s_min": lo, "loop_s_max": hi, "ms_per_iter": 1e3 * t / iters, "flop": flop,
                    "tflops": flop / t / 1e12, "frac_flop": flop / t / PEAK[dt],
                    "nocheck_loop_s": tn, "nocheck_loop_s_min": tn_lo, "nocheck_loop_s_max": tn_hi,
                    "nocheck_ms_per_iter": 1e3 * tn / iters, "nocheck_frac_flop": flop / tn / PEAK[dt],
                    "semi_loop_s": ts, "semi_loop_s_min": ts_lo, "semi_loop_s_max": ts_hi, "semi_ms_per_iter": 1e3 * ts / iters,
                    "semi_frac_flop": 2.0 * flop / ts / PEAK[dt], "ratio_to_semi": t / ts,
                    "parity_max_3it": float(np.max(np.abs(act - ref)) / np.max(np.abs(ref))),
                    "repeats": repeats, "warmup": warmup, "kernel": "k_prox_sweep", "baseline": "evc_semi_solve k_semi_sweep"})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prox_bench.jsonl"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_prox.py needs a HIP device: a CPU run gives no time")
    with open(a.out, "a") as f:
        for name in a.configs.split(","):
            for rec in run(name, a.iters, a.repeats, a.warmup):
                line = json.dumps(rec)
                print(line, flush=True)
                f.write(line + "\n")


if __name__ == "__main__":
    main()
