"""Benchmark of the activation solve with multi-frame exemplars (evc_deconv_solve: k_deconv_v + k_deconv_update): one JSON
line per shape, tap count and loss, appended to profiles/deconv_bench.jsonl.

The iteration loop is timed with the HIP events evc_deconv_opts.ev_loop_start / ev_loop_stop (median of --repeats after
--warmup calls, no error checks inside the loop).  flop = K * L * (6 M N) + K * 3 N per frame: V, Num and Den at 2 L M N
each (the KL denominator runs the same contraction over ones).  In the same run evc_beta_solve (k_beta_sweep, beta = 2 for
Frobenius and beta = 1 for KL) is timed at the same M, N and frames: it is the one-frame baseline.  `ratio_to_beta` = loop
time of the deconvolution / loop time of the baseline, `per_tap_ratio` = that / L (the expectation was about 1).  Parity: 3
iterations on the first utterance against the numpy restatement (tests/deconv_restatement.py).

    python tools/bench_deconv.py [--configs c2_f64,stft_f32] [--iters K] [--repeats R] [--warmup W]
                                 [--out profiles/deconv_bench.jsonl]
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

# name -> (M, N, frames per utterance, utterances, dtype, tap counts, iterations)
CONFIGS = {
    "c2_f64": (25, 4096, 688, 16, np.float64, (1, 4, 8), 20),
    "stft_f32": (201, 4096, 688, 16, np.float32, (1, 4), 20),
}
LOSSES = (("frobenius", 2.0), ("kullback-leibler", 1.0))


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
    from exemplars_vc_amd import solve_activations_beta, solve_activations_deconv
    import deconv_restatement as dr
    M, N, Tu, n_utt, dt, tap_counts, iters = CONFIGS[name]
    iters = iters_override or iters
    T = Tu * n_utt
    offs = np.arange(n_utt + 1, dtype=np.int32) * Tu
    dev = torch.device("cuda", 0)
    tt = torch.float64 if dt == np.float64 else torch.float32
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    ev[0].record()
    ev[1].record()          # force creation of the underlying hipEvent_t
    Lmax = max(tap_counts)
    rng = np.random.default_rng(M * 7919 + N)
    D = rng.random((M, N + Lmax - 1)) ** 2 + 1e-3
    Hs = rng.random((N, T)) * (rng.random((N, T)) < 6.0 / N)
    out, base = [], {}
    for L in tap_counts:
        A = np.stack([D[:, tau:tau + N] for tau in range(L)])
        X = dr.synthesize(A, Hs, offs) + 1e-4
        Ad, Xd = torch.from_numpy(A).to(dev, tt), torch.from_numpy(X).to(dev, tt)
        for loss, beta in LOSSES:
            # the baseline sees the same X; its time does not depend on the values
            tb, tb_lo, tb_hi = timed(lambda: solve_activations_beta(Ad[0], Xd, beta=beta, iters=iters, utt_offsets=offs,
                                                                    loop_events=ev), ev, repeats, warmup)
            t, lo, hi = timed(lambda: solve_activations_deconv(Ad, Xd, loss=loss, iters=iters, utt_offsets=offs,
                                                               loop_events=ev), ev, repeats, warmup)
            act = solve_activations_deconv(Ad, Xd[:, :Tu], loss=loss, iters=3).cpu().numpy().astype(np.float64)
            ref = dr.solve(A, X[:, :Tu].astype(dt), loss="frobenius" if beta == 2.0 else "kl", iters=3)[0]
            flop = float(iters) * (6.0 * L * M * N + 3.0 * N) * T
            out.append({"config": name, "loss": loss, "taps": L, "M": M, "N": N, "T": T, "n_utt": n_utt,
                        "dtype": np.dtype(dt).name, "iters": iters, "loop_s": t, "loop_s_min": lo, "loop_s_max": hi,
                        "ms_per_iter": 1e3 * t / iters, "flop": flop, "tflops": flop / t / 1e12, "frac_flop": flop / t / PEAK[dt],
                        "beta_loop_s": tb, "beta_loop_s_min": tb_lo, "beta_loop_s_max": tb_hi, "beta_ms_per_iter": 1e3 * tb / iters,
                        "ratio_to_beta": t / tb, "per_tap_ratio": t / tb / L,
                        "parity_rel_3it": float(np.linalg.norm(act - ref) / np.linalg.norm(ref)), "repeats": repeats,
                        "warmup": warmup, "kernel": "k_deconv_v+k_deconv_update", "baseline": "k_beta_sweep"})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--iters", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deconv_bench.jsonl"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_deconv.py needs a HIP device: a CPU run gives no time")
    with open(a.out, "a") as f:
        for name in a.configs.split(","):
            for rec in run(name, a.iters, a.repeats, a.warmup):
                line = json.dumps(rec)
                print(line, flush=True)
                f.write(line + "\n")


if __name__ == "__main__":
    main()
