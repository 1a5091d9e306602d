"""Benchmark of the coordinate descent that also learns the dictionary (evc_cd_learn): one JSON line per measurement,
appended to profiles/cd_learn_bench.jsonl.

  loop      per-iteration time of the whole loop from the HIP events evc_cd_learn_opts.ev_loop_start / ev_loop_stop (median
            of --repeats calls after --warmup; tol = 0 and nothing read back, so no stop checks), and beside it one
            evc_nmf_learn Frobenius iteration at the same shape, measured the same way
  kernels   (--kernels) a child run of the same configuration under `rocprofv3 --kernel-trace --stats`, a run of its own:
            per-iteration time of the activation sweep (k_cd_sweep), the residual start (k_cd_init_resid), the two
            contractions (k_dict_grad: the P call and the G call are told apart by their grids' sizes only in the trace, so
            their sum is reported and G's share is priced from the flop ratio R : M), the finish (k_cdl_finish), the
            dictionary sweep (k_cd_dict_sweep) and the rest; the G contraction's share of the matrix peak at 2 R^2 T flop
            (78.6 TF float64, 157.3 TF float32)
  sklearn   (--sklearn) scikit-learn's solver='cd' on the host for 3 iterations of the same problem, seconds per iteration

    python tools/bench_cd_learn.py [--configs compaction,stft_pair] [--iters K] [--repeats R] [--warmup W]
                                   [--kernels] [--sklearn] [--out FILE]
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
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = {np.float64: 78.6e12, np.float32: 157.3e12}

# name -> (M, R, T, dtype, iterations)
CONFIGS = {
    "compaction": (50, 512, 65536, np.float64, 10),       # 25 + 25 stacked bins, every aligned frame
    "stft_pair": (402, 512, 32768, np.float32, 10),       # two stacked 201-bin STFT magnitudes
}


def problem(M, R, T, seed, dt):
    rng = np.random.default_rng(seed)
    A = rng.random((M, R)) ** 2 + 1e-3
    X = A @ (rng.random((R, T)) * (rng.random((R, T)) < 0.05)) + 1e-3 * rng.random((M, T))
    return X.astype(dt), (rng.random((M, R)) + 1e-4).astype(dt), (rng.random((R, T)) + 1e-4).astype(dt)


def _device_problem(name):
    import torch
    M, R, T, dt, _ = CONFIGS[name]
    dev = torch.device("cuda", 0)
    return tuple(torch.from_numpy(a).to(dev) for a in problem(M, R, T, 17, dt))


def run_loop(name, iters, repeats, warmup):
    import torch
    from exemplars_vc_amd import learn_dictionary, learn_dictionary_cd
    M, R, T, dt, k = CONFIGS[name]
    iters = iters or k
    Xd, Wd, Hd = _device_problem(name)
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    ev[0].record()
    ev[1].record()          # force creation of the underlying hipEvent_t

    def timed(call):
        times = []
        for r in range(warmup + repeats):
            W, H = call()
            torch.cuda.synchronize()
            if r >= warmup:
                times.append(ev[0].elapsed_time(ev[1]) * 1e-3)
        assert bool(torch.isfinite(W).all()) and bool(torch.isfinite(H).all())
        return times
    cd = timed(lambda: learn_dictionary_cd(Xd, Wd, Hd, layout="bin_major", max_iter=iters, tol=0.0, loop_events=ev))
    mu = timed(lambda: learn_dictionary(Xd, Wd, Hd, layout="bin_major", iters=iters, check_every=0, loop_events=ev))
    from exemplars_vc_amd import _lib
    return {"what": "loop", "config": name, "M": M, "R": R, "T": T, "dtype": np.dtype(dt).name, "iters": iters,
            "splits": int(_lib.lib().evc_cd_learn_splits(M, R, T)), "ms_per_iter": 1e3 * float(np.median(cd)) / iters,
            "spread_ms_per_iter": 1e3 * (max(cd) - min(cd)) / iters,
            "nmf_learn_frobenius_ms_per_iter": 1e3 * float(np.median(mu)) / iters, "repeats": repeats}


GROUPS = (("k_cd_sweep", "activation_sweep"), ("k_cd_init_resid", "residual_start"), ("k_dict_grad", "contractions"),
          ("k_cdl_finish", "finish"), ("k_cd_dict_sweep", "dictionary_sweep"))


def run_kernels(name, iters):
    M, R, T, dt, k = CONFIGS[name]
    iters = iters or k
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "cdl", "--",
               sys.executable, os.path.abspath(__file__), "--child", "--configs", name, "--iters", str(iters)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if p.returncode != 0 or not files:
            return {"what": "kernels", "config": name, "error": (p.stdout + p.stderr)[-300:]}
        rows = list(csv.DictReader(open(files[0])))
    key_n = next(c for c in rows[0] if "name" in c.lower())
    key_t = next(c for c in rows[0] if "total" in c.lower() and "ns" in c.lower())
    ms = {g: 0.0 for _, g in GROUPS}
    ms["other"] = 0.0
    for r in rows:
        g = next((g for pat, g in GROUPS if pat in r[key_n]), "other")
        ms[g] += float(r[key_t]) * 1e-6 / iters
    g_ms = ms["contractions"] * R / (R + M)         # both calls run the same kernel at flop 2 R^2 T : 2 M R T
    out = {"what": "kernels", "config": name, "iters": iters, "M": M, "R": R, "T": T, "dtype": np.dtype(dt).name}
    out.update({g + "_ms_per_iter": v for g, v in ms.items()})
    out["kernels_ms_per_iter"] = sum(ms.values())
    out["G_contraction_ms_est"] = g_ms
    out["G_frac_of_matrix_peak"] = 2.0 * R * R * T / (g_ms * 1e-3) / PEAK[dt] if g_ms > 0 else None
    return out


def run_child(name, iters):
    """what the profiled child runs: one call, nothing printed"""
    import torch
    from exemplars_vc_amd import learn_dictionary_cd
    Xd, Wd, Hd = _device_problem(name)
    learn_dictionary_cd(Xd, Wd, Hd, layout="bin_major", max_iter=iters or CONFIGS[name][4], tol=0.0)
    torch.cuda.synchronize()


def run_sklearn(name, k=3):
    import sklearn.decomposition._nmf as nmf
    M, R, T, dt, _ = CONFIGS[name]
    X, W0, H0 = problem(M, R, T, 17, dt)
    t0 = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        nmf.non_negative_factorization(np.ascontiguousarray(X.T), W=np.ascontiguousarray(H0.T), H=np.ascontiguousarray(W0.T),
                                       init="custom", update_H=True, n_components=R, solver="cd", tol=0.0, max_iter=k)
    return {"what": "sklearn", "config": name, "iters": k, "s_per_iter": (time.perf_counter() - t0) / k,
            "cpus": len(os.sched_getaffinity(0))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--iters", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--sklearn", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cd_learn_bench.jsonl"))
    a = ap.parse_args()
    names = a.configs.split(",")
    if a.child:
        return run_child(names[0], a.iters)
    res = []
    if a.kernels:               # first: the profiled children run before this process opens the GPU
        res += [run_kernels(n, a.iters) for n in names]
    if a.sklearn:
        res += [run_sklearn(n) for n in names]
    res += [run_loop(n, a.iters, a.repeats, a.warmup) for n in names]
    with open(a.out, "a") as f:
        for r in res:
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
