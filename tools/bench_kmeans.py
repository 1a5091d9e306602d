"""Benchmark of the device k-means (evc_kmeans: k_km_assign and the round's other kernels): one JSON line per shape and
element type, appended to profiles/kmeans_bench.jsonl.

The round loop is timed with the HIP events evc_kmeans_opts.ev_loop_start / ev_loop_stop (median of --repeats after --warmup
calls, stop="none": every round runs).  A further call under torch.profiler gives the kernels' own times: `assign_ms` is
k_km_assign (+ k_km_merge where the centres are split) per assignment, `assign_frac_flop` its flop, 2 M R T, over that time
and the matrix peak; `bound` names the larger of the two floors of one assignment - the matrix cores at peak, or X and W once
through memory at `--hbm` bytes per second.  `redecided_share` is the share of samples whose two best expanded scores lie
within the guard, restated with torch from the start centres and from the final ones.
Two comparisons run in the same call, alternating with the k-means call in every repeat:
  synthesize(W^T, X)   the project's own contraction forming the same R x T product and WRITING it (`synth_ms`, events around
                       `--iters` calls); `assign_over_synth` is the fused assignment's time over it
  kmeans_assign        one assignment pass of compat/pymf.py's host loop in numpy, at the shapes of HOST only (`host_pass_s`)

    python tools/bench_kmeans.py [--configs m50_t4096_r64_f64,...] [--iters K] [--repeats R] [--warmup W] [--out ...]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK = {np.float64: 78.6e12, np.float32: 157.3e12}
SHAPES = ((50, 4096, 64), (50, 4096, 256), (50, 4096, 1024), (50, 16384, 1024), (402, 16384, 1024))
CONFIGS = {"m%d_t%d_r%d_%s" % (M, T, R, "f64" if dt == np.float64 else "f32"): (M, T, R, dt)
           for M, T, R in SHAPES for dt in (np.float64, np.float32)}
HOST = {(50, 4096, 256)}


def kernel_times(fn):
    """-> [(start, kernel name, seconds)] of one call, from torch.profiler; None where the profiler gives no device events"""
    import torch
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        rows = []
        for e in prof.events():
            dur = getattr(e, "device_time", None)
            if dur is None:
                dur = getattr(e, "cuda_time", 0.0)
            if dur and "Memcpy" not in e.name and "Memset" not in e.name:
                rows.append((e.time_range.start, e.name, dur * 1e-6))
        rows.sort()
        return rows or None
    except Exception as exc:  # noqa: BLE001 - the timing lines do not depend on the profiler
        print("profiler pass failed:", repr(exc), file=sys.stderr)
        return None


def redecided_share(X, W, M, dt):
    """the share of samples whose two best expanded scores lie closer than g_t = 4 (M + 4) u (||x_t||^2 + max_r ||w_r||^2)"""
    import torch
    xn, wn = (X * X).sum(0), (W * W).sum(0)
    two = torch.topk(wn[:, None] - 2.0 * (W.T @ X), 2, dim=0, largest=False).values
    g = 4.0 * (M + 4) * (np.finfo(dt).eps / 2) * (xn + wn.max())
    return float((~(two[1] - two[0] >= g)).double().mean())


def host_pass(X, W):
    """one assignment pass of compat/pymf.py's kmeans_assign"""
    t0 = time.perf_counter()
    d = np.zeros((W.shape[1], X.shape[1]))
    for a in range(W.shape[1]):
        d[a:a + 1, :] = np.sqrt(((X[:, :] - W[:, a:a + 1]) ** 2.0).sum(axis=0)).reshape((1, -1))
    np.argmin(d, axis=0)
    return time.perf_counter() - t0


def run(name, iters, repeats, warmup, hbm):
    import torch
    from exemplars_vc_amd import _lib, kmeans, synthesize
    import kmeans_restatement as kr
    M, T, R, dt = CONFIGS[name]
    dev = torch.device("cuda", 0)
    tt = torch.float64 if dt == np.float64 else torch.float32
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    es = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    for e in ev:
        e.record()          # force creation of the underlying hipEvent_t
    X = kr.problem(M, T, max(R // 4, 1), T + R)
    W0 = X[:, kr.spread_start(T, R)]
    Xd, W0d = torch.from_numpy(X).to(dev, tt), torch.from_numpy(W0).to(dev, tt).contiguous()
    WTd = W0d.T.contiguous()
    with_host = (M, T, R) in HOST and dt == np.float64
    res = {}

    def call(events=ev):
        res["W"], res["labels"] = kmeans(Xd, W0d, layout="bin_major", iters=iters, stop="none", loop_events=events)

    t_km, t_sy, t_host = [], [], []
    for r in range(warmup + repeats):
        call()
        torch.cuda.synchronize()
        es[0].record()
        for _ in range(iters):
            synthesize(WTd, Xd, layout="bin_major")
        es[1].record()
        torch.cuda.synchronize()
        if r >= warmup:
            t_km.append(ev[0].elapsed_time(ev[1]) * 1e-3 / iters)
            t_sy.append(es[0].elapsed_time(es[1]) * 1e-3 / iters)
            if with_host:
                t_host.append(host_pass(X, W0))
    flop = 2.0 * M * R * T
    esz = np.dtype(dt).itemsize
    floor_mm, floor_mem = flop / PEAK[dt], (M * T + M * R) * esz / hbm
    rec = {"config": name, "M": M, "T": T, "R": R, "dtype": np.dtype(dt).name, "iters": iters, "repeats": repeats, "warmup": warmup,
           "splits": int(_lib.lib().evc_kmeans_splits(R, T)), "round_ms": 1e3 * float(np.median(t_km)),
           "round_ms_min": 1e3 * min(t_km), "round_ms_max": 1e3 * max(t_km), "synth_ms": 1e3 * float(np.median(t_sy)),
           "synth_ms_min": 1e3 * min(t_sy), "synth_ms_max": 1e3 * max(t_sy), "flop_per_assign": flop,
           "floor_matrix_ms": 1e3 * floor_mm, "floor_bytes_ms": 1e3 * floor_mem, "bound": "matrix" if floor_mm >= floor_mem else "bytes",
           "redecided_share_first": redecided_share(Xd, W0d, M, dt), "redecided_share_last": redecided_share(Xd, res["W"], M, dt),
           "kernel": "k_km_assign", "yardstick": "synthesize(W^T, X)"}
    if with_host:
        rec.update({"host_pass_s": float(np.median(t_host)), "host_pass_s_min": min(t_host), "host_pass_s_max": max(t_host)})
    rows = kernel_times(lambda: call(None))
    if rows:
        n_assign = iters + 1
        per = {}
        for _, n, d in rows:
            key = next((k for k in ("k_km_assign", "k_km_merge", "k_km_refine", "k_km_centres", "k_km_err", "k_km_commit", "k_km_norms",
                                    "k_km_state") if k in n), None)
            if key:
                per[key] = per.get(key, 0.0) + d
        assign = (per.get("k_km_assign", 0.0) + per.get("k_km_merge", 0.0)) / n_assign
        rec.update({"assign_ms": 1e3 * assign, "assign_frac_flop": flop / assign / PEAK[dt], "assign_over_synth": assign / float(np.median(t_sy)),
                    "kernels_ms_per_round": {k: 1e3 * v / (iters if k == "k_km_centres" else n_assign) for k, v in sorted(per.items())}})
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--hbm", type=float, default=8.0e12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_bench.jsonl"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_kmeans.py needs a HIP device: a CPU run gives no time")
    with open(a.out, "a") as f:
        for name in a.configs.split(","):
            line = json.dumps(run(name, a.iters, a.repeats, a.warmup, a.hbm))
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
