"""Benchmark of the coordinate-descent solve (evc_cd_solve, k_cd_sweep): one JSON line per configuration.

The iteration loop is timed with the HIP events evc_cd_opts.ev_loop_start / ev_loop_stop (median of --repeats after
--warmup calls).  flop = sum over utterances of n_iter_u * 4 M N T_u (the factored algebra: r . a_t and r += delta a_t
per component and frame; frames of a stopped utterance are not counted); bytes = H read and written once per
iteration plus X once.  frac = the larger of flop rate / peak (78.6 TF float64, 157.3 TF float32) and byte rate /
8 TB/s; `bound` says which.  Parity: a short run (3 iterations, tol = 0) of the same shapes against the numpy
restatement (tests/cd_restatement.py) on a sample of frames.

    python tools/bench_cd.py [--configs c2_batch,c2_1utt,c3_1utt,c3_16utt,stft_f32_16utt,script_default]
                             [--iters K] [--repeats R] [--warmup W]
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
BW = 8.0e12

# name -> (M, N, frames per utterance, utterances, dtype, tol, iterations)
CONFIGS = {
    "c2_batch": (25, 4096, 688, 256, np.float64, 0.0, 200),
    "c2_1utt": (25, 4096, 688, 1, np.float64, 0.0, 200),
    "c3_1utt": (513, 8192, 688, 1, np.float64, 0.0, 50),
    "c3_16utt": (513, 8192, 688, 16, np.float64, 0.0, 50),
    "stft_f32_16utt": (201, 4096, 688, 16, np.float32, 0.0, 50),
    "script_default": (201, 160, 40, 1, np.float64, 1e-4, 200),     # the real-audio fixture's shape, tol = 1e-4
}


def problem(M, N, T, seed):
    rng = np.random.default_rng(seed)
    W = rng.random((N, M)) ** 2
    X = (rng.random((T, N)) * (rng.random((T, N)) < 0.01)) @ W + 1e-3 * rng.random((T, M))
    return X, W


def run(name, iters_override, repeats, warmup):
    import torch
    from exemplars_vc_amd import solve_activations_cd
    from cd_restatement import cd_iterations
    M, N, Tu, n_utt, dt, tol, iters = CONFIGS[name]
    if iters_override:
        iters = iters_override
    T = Tu * n_utt
    if name == "script_default":
        d = np.load(os.path.join(ROOT, "tests", "golden", "cdnmf_m201_audio.npz"))
        X, W = d["X_rows"], d["W_rows"]
    else:
        X, W = problem(M, N, T, M * 7919 + N)
    dev = torch.device("cuda", 0)
    tt = torch.float64 if dt == np.float64 else torch.float32
    Wd = torch.from_numpy(W).to(dev, tt)
    Xd = torch.from_numpy(X).to(dev, tt)
    offs = np.arange(n_utt + 1, dtype=np.int32) * Tu
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    ev[0].record()
    ev[1].record()          # force creation of the underlying hipEvent_t
    times = []
    n_iter = None
    for r in range(warmup + repeats):
        _, info = solve_activations_cd(Wd, Xd, layout="frame_major", max_iter=iters, tol=tol, utt_offsets=offs,
                                       info=True, loop_events=ev)
        torch.cuda.synchronize()
        if r >= warmup:
            times.append(ev[0].elapsed_time(ev[1]) * 1e-3)
        n_iter = info["n_iter"]
    t = float(np.median(times))
    es = np.dtype(dt).itemsize
    frame_iters = float(np.sum(n_iter.astype(np.float64) * Tu))
    flop = 4.0 * M * N * frame_iters
    nbytes = 2.0 * N * es * frame_iters + T * M * es
    fr_f, fr_b = flop / t / PEAK[dt], nbytes / t / BW
    # parity: 3 iterations, tol = 0, on a sample of the first utterance's frames
    act = solve_activations_cd(Wd, Xd, layout="frame_major", max_iter=3, tol=0, utt_offsets=offs)
    act = act.cpu().numpy().astype(np.float64)
    sample = np.arange(0, min(Tu, 688), 43 if M > 32 else 11)
    ref, _ = cd_iterations(X[sample].astype(np.float64), W.astype(np.float64), 3)
    parity = float(np.linalg.norm(act[sample] - ref) / np.linalg.norm(ref))
    return {"config": name, "M": M, "N": N, "T": T, "n_utt": n_utt, "dtype": np.dtype(dt).name, "tol": tol,
            "max_iter": iters, "n_iter_max": int(n_iter.max()), "n_iter_min": int(n_iter.min()),
            "loop_s": t, "ms_per_iter": 1e3 * t / max(int(n_iter.max()), 1), "flop": flop, "bytes": nbytes,
            "tflops": flop / t / 1e12, "frac_flop": fr_f, "frac_bytes": fr_b, "frac": max(fr_f, fr_b),
            "bound": "flop" if fr_f >= fr_b else "bytes", "parity_rel_3it": parity, "repeats": repeats,
            "kernel": info["kernel"], "launches": info["launches"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--iters", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    for name in a.configs.split(","):
        print(json.dumps(run(name, a.iters, a.repeats, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
