"""Benchmark of dictionary learning (evc_nmf_learn): one JSON line per measurement, appended to profiles/learn_bench.jsonl.

  loop      per-iteration time of the whole loop from the HIP events evc_learn_opts.ev_loop_start / ev_loop_stop (median
            of --repeats calls after --warmup), and, from torch events, the time of one activation step on its own (one
            evc_nmf_solve call with iters = 1: import, packing and the update)
  kernels   (--kernels) a child run of the same configuration under `rocprofv3 --kernel-trace --stats`: total time of
            k_dict_grad, of k_dict_apply (+ k_dict_colnorm) and of every other kernel of the loop; k_dict_grad's share
            of the matrix peak priced at 4 M R T flop per iteration (78.6 TF float64, 157.3 TF float32) and of 8 TB/s
            priced at (2 M + R) T esize bytes; `bound` names the larger.  --loss kl: the one-operand contraction is
            priced at 2 M R T flop and (M + R) T esize bytes, and the quotient pass k_dict_quot is reported on its own
  --loss    frobenius (default) or kl: the same configurations and lines, with a `loss` field
  versus    (--versus) the pymf surface on the compaction shape, K = 5: compat.pymf.NMF(...).factorize() with the
            dictionary update in numpy on the host (the default) against dictionary_update="device", alternating, three
            runs each; ratio of the medians and whether the gain exceeds twice the run-to-run spread

    python tools/bench_learn.py [--configs compaction,stft_pair] [--iters K] [--repeats R] [--warmup W]
                                [--loss frobenius|kl] [--kernels] [--versus] [--out FILE]
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = {np.float64: 78.6e12, np.float32: 157.3e12}
BW = 8.0e12

# name -> (M, R, T, dtype, iterations)
CONFIGS = {
    "compaction": (50, 512, 65536, np.float64, 50),       # 25 + 25 stacked bins, every aligned frame
    "stft_pair": (402, 512, 32768, np.float32, 50),       # two stacked 201-bin STFT magnitudes
}


def problem(M, R, T, seed, dt):
    rng = np.random.default_rng(seed)
    A = rng.random((M, R)) ** 2 + 1e-3
    X = A @ (rng.random((R, T)) * (rng.random((R, T)) < 0.05)) + 1e-3 * rng.random((M, T))
    return X.astype(dt), (rng.random((M, R)) + 1e-4).astype(dt), (rng.random((R, T)) + 1e-4).astype(dt)


def run_loop(name, iters, repeats, warmup, loss):
    import torch
    from exemplars_vc_amd import learn_dictionary, solve_activations
    M, R, T, dt, k = CONFIGS[name]
    iters = iters or k
    X, W0, H0 = problem(M, R, T, 17, dt)
    dev = torch.device("cuda", 0)
    Xd, Wd, Hd = (torch.from_numpy(a).to(dev) for a in (X, W0, H0))
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    ev[0].record()
    ev[1].record()          # force creation of the underlying hipEvent_t
    times = []
    for r in range(warmup + repeats):
        W, H, info = learn_dictionary(Xd, Wd, Hd, layout="bin_major", iters=iters, check_every=0, info=True,
                                      loop_events=ev, loss=loss)
        torch.cuda.synchronize()
        if r >= warmup:
            times.append(ev[0].elapsed_time(ev[1]) * 1e-3)
    assert bool(torch.isfinite(W).all()) and bool(torch.isfinite(H).all())
    t = float(np.median(times))
    a0, a1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = torch.empty_like(Hd)
    kw = dict(layout="bin_major", iters=1, eps_mode="zero_replace", init="given", cooperative=False, out=out, loss=loss)
    solve_activations(Wd, Xd, Hd, **kw)
    a0.record()
    for _ in range(10):
        solve_activations(Wd, Xd, Hd, **kw)
    a1.record()
    torch.cuda.synchronize()
    act_ms = a0.elapsed_time(a1) / 10
    return {"what": "loop", "config": name, "loss": loss, "M": M, "R": R, "T": T, "dtype": np.dtype(dt).name, "iters": iters,
            "splits": info["splits"], "loop_s": t, "ms_per_iter": 1e3 * t / iters, "activation_step_ms": act_ms,
            "spread_ms_per_iter": 1e3 * (max(times) - min(times)) / iters, "repeats": repeats}


def run_kernels(name, iters, loss):
    M, R, T, dt, k = CONFIGS[name]
    iters = iters or k
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "learn", "--",
               sys.executable, os.path.abspath(__file__), "--child", "--configs", name, "--iters", str(iters),
               "--loss", loss]
        p = subprocess.run(cmd, capture_output=True, text=True)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if p.returncode != 0 or not files:
            found = [os.path.relpath(f, tmp) for f in glob.glob(os.path.join(tmp, "**", "*"), recursive=True)]
            return {"what": "kernels", "config": name, "loss": loss, "error": (p.stdout + p.stderr)[-300:], "files": found[:20]}
        rows = list(csv.DictReader(open(files[0])))
    key_n = next(c for c in rows[0] if "name" in c.lower())
    key_t = next(c for c in rows[0] if "total" in c.lower() and "ns" in c.lower())
    key_c = next(c for c in rows[0] if c.lower() in ("calls", "count"))
    tot = {"k_dict_grad": 0.0, "k_dict_apply": 0.0, "k_dict_quot": 0.0, "other": 0.0}
    calls = 0
    top = []
    for r in rows:
        ns = float(r[key_t])
        nm = r[key_n]
        top.append((ns, nm[:60]))
        if "k_dict_grad" in nm:
            tot["k_dict_grad"] += ns
            calls += int(r[key_c])
        elif "k_dict_apply" in nm or "k_dict_colnorm" in nm:
            tot["k_dict_apply"] += ns
        elif "k_dict_quot" in nm:
            tot["k_dict_quot"] += ns
        else:
            tot["other"] += ns
    es = np.dtype(dt).itemsize
    per_call = tot["k_dict_grad"] * 1e-9 / max(calls, 1)
    kl = loss == "kl"
    fr_f = (2.0 if kl else 4.0) * M * R * T / per_call / PEAK[dt]
    fr_b = ((1.0 if kl else 2.0) * M + R) * T * es / per_call / BW
    return {"what": "kernels", "config": name, "loss": loss, "iters": iters, "calls": calls,
            "k_dict_grad_ms_per_call": 1e3 * per_call,
            "k_dict_grad_ms": tot["k_dict_grad"] * 1e-6, "k_dict_apply_ms": tot["k_dict_apply"] * 1e-6,
            "k_dict_quot_ms_per_call": tot["k_dict_quot"] * 1e-6 / max(calls, 1),
            "other_kernels_ms": tot["other"] * 1e-6, "frac_flop": fr_f, "frac_bytes": fr_b,
            "bound": "flop" if fr_f >= fr_b else "bytes", "top": [[n, ns * 1e-6] for ns, n in sorted(top, reverse=True)[:8]]}


def run_child(name, iters, loss):
    """what the profiled child runs: one warm-up call, nothing printed"""
    import torch
    from exemplars_vc_amd import learn_dictionary
    M, R, T, dt, k = CONFIGS[name]
    X, W0, H0 = problem(M, R, T, 17, dt)
    dev = torch.device("cuda", 0)
    Xd, Wd, Hd = (torch.from_numpy(a).to(dev) for a in (X, W0, H0))
    learn_dictionary(Xd, Wd, Hd, layout="bin_major", iters=iters or k, check_every=0, loss=loss)
    torch.cuda.synchronize()


def run_versus(k=5):
    import warnings
    from exemplars_vc_amd.compat.pymf import NMF
    M, R, T, dt, _ = CONFIGS["compaction"]
    X, W0, H0 = problem(M, R, T, 17, np.float64)

    def once(mode):
        mdl = NMF(X, num_bases=R, dictionary_update=mode)
        mdl.W, mdl.H = W0.copy(), H0.copy()
        t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            mdl.factorize(niter=k, compute_err=False)
        return time.perf_counter() - t0, mdl.W
    once("device")                                  # warm-up: library load, workspace
    th, td = [], []
    for _ in range(3):
        t, Wh = once("host")
        th.append(t)
        t, Wd = once("device")
        td.append(t)
    spread = max(max(th) - min(th), max(td) - min(td))
    mh, md = float(np.median(th)), float(np.median(td))
    return {"what": "versus", "config": "compaction", "iters": k, "host_s": th, "device_s": td, "ratio": mh / md,
            "gain_s": mh - md, "spread_s": spread, "faster_by_more_than_twice_the_spread": bool(mh - md > 2 * spread),
            "max_rel_diff_W": float(np.max(np.abs(Wd - Wh) / np.abs(Wh)))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--iters", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--loss", choices=("frobenius", "kl"), default="frobenius")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--versus", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "learn_bench.jsonl"))
    a = ap.parse_args()
    names = a.configs.split(",")
    if a.child:
        return run_child(names[0], a.iters, a.loss)
    res = []
    if a.kernels:               # first: the profiled children run before this process opens the GPU
        res += [run_kernels(n, a.iters, a.loss) for n in names]
    res += [run_loop(n, a.iters, a.repeats, a.warmup, a.loss) for n in names]
    if a.versus:
        res.append(run_versus())
    with open(a.out, "a") as f:
        for r in res:
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
