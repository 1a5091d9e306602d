"""Benchmark of the semi-NMF activation solve (evc_semi_solve: k_semi_sweep): one JSON line per shape and element type,
appended to profiles/semi_bench.jsonl.

The iteration loop is timed with the HIP events evc_semi_opts.ev_loop_start / ev_loop_stop (median of --repeats after
--warmup calls, no error checks inside the loop).  flop = 4 N^2 T per iteration: two N x N contractions against H, the
positive and the negative part of the Gram matrix.  In the same run evc_nmf_solve with algo="gram" is timed at the same N,
frames and element type on non-negative data: one N x N contraction and update per iteration, of which the sweep issues
exactly twice the MFMAs - `ratio_to_gram` = loop time of the sweep / loop time of that baseline (the expectation to test:
about 2).  Parity: 3 iterations on the first 64 frames against the numpy restatement (tests/semi_restatement.py).

    python tools/bench_semi.py [--configs n1024_f64,...] [--iters K] [--repeats R] [--warmup W] [--out profiles/semi_bench.jsonl]
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
    "n1024_f64": (25, 1024, 688, (16, 1), np.float64),
    "n1024_f32": (25, 1024, 688, (16, 1), np.float32),
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
    from exemplars_vc_amd import solve_activations, solve_activations_semi
    import semi_restatement as sr
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
        A, X, H0 = sr.problem(M, N, T, N + n_utt)
        Ad, Xd, Hd = (torch.from_numpy(a).to(dev, tt) for a in (A, X, H0))
        An, Xn = Ad.abs() + 1e-3, Xd.abs() + 1e-3           # the baseline needs non-negative data; its time does not depend on the values
        tb, tb_lo, tb_hi = timed(lambda: solve_activations(An, Xn, Hd, algo="gram", iters=iters, utt_offsets=offs,
                                                           loop_events=ev), ev, repeats, warmup)
        t, lo, hi = timed(lambda: solve_activations_semi(Ad, Xd, Hd, iters=iters, utt_offsets=offs, loop_events=ev), ev,
                          repeats, warmup)
        act = solve_activations_semi(Ad, Xd[:, :64].contiguous(), Hd[:, :64].contiguous(), iters=3).cpu().numpy().astype(np.float64)
        ref = sr.solve(A, X[:, :64], H0[:, :64], 3)[0]
        flop = float(iters) * 4.0 * N * N * T
        out.append({"config": name, "M": M, "N": N, "T": T, "n_utt": n_utt, "dtype": np.dtype(dt).name, "iters": iters,
                    "loop_s": t, "loop_s_min": lo, "loop_s_max": hi, "ms_per_iter": 1e3 * t / iters, "flop": flop,
                    "tflops": flop / t / 1e12, "frac_flop": flop / t / PEAK[dt],
                    "gram_loop_s": tb, "gram_loop_s_min": tb_lo, "gram_loop_s_max": tb_hi, "gram_ms_per_iter": 1e3 * tb / iters,
                    "ratio_to_gram": t / tb, "parity_rel_3it": float(np.linalg.norm(act - ref) / np.linalg.norm(ref)),
                    "repeats": repeats, "warmup": warmup, "kernel": "k_semi_sweep", "baseline": "evc_nmf_solve algo=gram"})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "semi_bench.jsonl"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_semi.py needs a HIP device: a CPU run gives no time")
    with open(a.out, "a") as f:
        for name in a.configs.split(","):
            for rec in run(name, a.iters, a.repeats, a.warmup):
                line = json.dumps(rec)
                print(line, flush=True)
                f.write(line + "\n")


if __name__ == "__main__":
    main()
