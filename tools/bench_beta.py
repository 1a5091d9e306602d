"""Benchmark of the beta-divergence activation solve (evc_beta_solve, k_beta_sweep): one JSON line per shape and beta,
appended to profiles/beta_bench.jsonl.

The iteration loop is timed with the HIP events evc_beta_opts.ev_loop_start / ev_loop_stop (median of --repeats after
--warmup calls, no error checks inside the loop).  flop = K * (6 M N + 3 N) per frame: V = A H, Num and Den at 2 M N each,
the update at 3 N.  frac_flop = flop rate / the dtype's matrix peak (78.6 TF float64, 157.3 TF float32).  In the same
run the existing Kullback-Leibler solve (solve_activations(loss="kl"), 4 M N flop per frame-iteration) is timed at the
same shape and iteration count; `ratio_to_kl` = loop time of the beta solve / loop time of the KL solve (arithmetic alone
predicts 1.5).  Parity: 3 iterations on a sample of frames against the numpy restatement (tests/beta_restatement.py).

    python tools/bench_beta.py [--configs stft_f32_16utt,c2_batch,world_1utt] [--betas 0,0.5,0.7] [--iters K]
                               [--repeats R] [--warmup W] [--out profiles/beta_bench.jsonl]
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

# name -> (M, N, frames per utterance, utterances, dtype, iterations)
CONFIGS = {
    "stft_f32_16utt": (201, 4096, 688, 16, np.float32, 20),
    "c2_batch": (25, 4096, 688, 256, np.float64, 20),
    "world_1utt": (513, 4096, 688, 1, np.float64, 20),
}


def problem(M, N, T, seed):
    rng = np.random.default_rng(seed)
    W = rng.random((N, M)) ** 2 + 1e-3
    X = (rng.random((T, 64)) * (rng.random((T, 64)) < 0.2)) @ W[:64] + 1e-3 * rng.random((T, M)) + 1e-4
    return X, W


def timed(fn, ev, repeats, warmup):
    import torch
    times = []
    for r in range(warmup + repeats):
        fn()
        torch.cuda.synchronize()
        if r >= warmup:
            times.append(ev[0].elapsed_time(ev[1]) * 1e-3)
    return float(np.median(times)), float(min(times)), float(max(times))


def run(name, betas, iters_override, repeats, warmup):
    import torch
    from exemplars_vc_amd import solve_activations, solve_activations_beta
    import beta_restatement as br
    M, N, Tu, n_utt, dt, iters = CONFIGS[name]
    iters = iters_override or iters
    T = Tu * n_utt
    X, W = problem(M, N, T, M * 7919 + N)
    dev = torch.device("cuda", 0)
    tt = torch.float64 if dt == np.float64 else torch.float32
    Wd, Xd = torch.from_numpy(W).to(dev, tt), torch.from_numpy(X).to(dev, tt)
    offs = np.arange(n_utt + 1, dtype=np.int32) * Tu
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    ev[0].record()
    ev[1].record()          # force creation of the underlying hipEvent_t
    t_kl, kl_lo, kl_hi = timed(lambda: solve_activations(Wd, Xd, layout="frame_major", iters=iters, eps_mode="zero_replace",
                                                         init="sklearn", loss="kl", utt_offsets=offs, loop_events=ev),
                               ev, repeats, warmup)
    sample = np.arange(0, Tu, 43)
    out = []
    for beta in betas:
        t, lo, hi = timed(lambda: solve_activations_beta(Wd, Xd, beta=beta, layout="frame_major", iters=iters,
                                                         utt_offsets=offs, loop_events=ev), ev, repeats, warmup)
        flop = float(iters) * (6.0 * M * N + 3.0 * N) * T
        h0 = np.full((len(sample), N), np.sqrt(X[:Tu].astype(dt).mean(dtype=np.float64) / N))
        act = solve_activations_beta(Wd, Xd[:Tu], beta=beta, layout="frame_major", iters=3).cpu().numpy()
        ref = br.beta_solve(X[sample].astype(np.float64), W.astype(np.float64), beta, 3, W0=h0)[0]
        parity = float(np.linalg.norm(act[sample] - ref) / np.linalg.norm(ref))
        out.append({"config": name, "beta": beta, "M": M, "N": N, "T": T, "n_utt": n_utt, "dtype": np.dtype(dt).name,
                    "iters": iters, "loop_s": t, "loop_s_min": lo, "loop_s_max": hi, "ms_per_iter": 1e3 * t / iters,
                    "flop": flop, "tflops": flop / t / 1e12, "frac_flop": flop / t / PEAK[dt], "kl_loop_s": t_kl,
                    "kl_loop_s_min": kl_lo, "kl_loop_s_max": kl_hi, "kl_ms_per_iter": 1e3 * t_kl / iters,
                    "ratio_to_kl": t / t_kl, "parity_rel_3it": parity, "repeats": repeats, "warmup": warmup,
                    "kernel": "k_beta_sweep"})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--betas", default="0,0.5,0.7")
    ap.add_argument("--iters", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beta_bench.jsonl"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_beta.py needs a HIP device: a CPU run gives no time")
    with open(a.out, "a") as f:
        for name in a.configs.split(","):
            for rec in run(name, [float(b) for b in a.betas.split(",")], a.iters, a.repeats, a.warmup):
                line = json.dumps(rec)
                print(line, flush=True)
                f.write(line + "\n")


if __name__ == "__main__":
    main()
