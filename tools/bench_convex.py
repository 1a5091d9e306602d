"""Benchmark of the convex-NMF learner (evc_convex_learn: k_convex_sweep): one JSON line per shape, element type and sweep
geometry, appended to profiles/convex_bench.jsonl.

The iteration loop is timed with the HIP events evc_convex_opts.ev_loop_start / ev_loop_stop (median of --repeats after
--warmup calls, no error checks inside the loop).  flop = 8 T^2 R per iteration: two Gram sweeps, each the positive and the
negative part of the T x T Gram matrix against R columns.  A further call under torch.profiler gives the kernels' own
times: `sweep_share` is the share of k_convex_sweep (+ k_convex_reduce) in the loop's kernels, the rest being the small
products and the element-wise steps; `sweep_frac_flop` is the sweeps' flop over their own time and the matrix peak.
In the same run evc_semi_solve is timed with N = T exemplars and R frames as one utterance: one of its iterations issues
exactly one sweep's MFMAs - `ratio_to_semi` = the sweeps' time per iteration / (2 x semi's time per iteration).
--neighbours also times the plan's neighbouring geometries (forced through `reserved`), to check the plan's choice.

    python tools/bench_convex.py [--configs t4096_r64_f64,...] [--neighbours] [--iters K] [--repeats R] [--warmup W] [--out ...]
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
M = 50
CONFIGS = {"t%d_r%d_%s" % (T, R, "f64" if dt == np.float64 else "f32"): (T, R, dt)
           for T, R in ((4096, 64), (4096, 256), (4096, 1024), (16384, 512)) for dt in (np.float64, np.float32)}


def timed(fn, ev, repeats, warmup):
    import torch
    times = []
    for r in range(warmup + repeats):
        fn()
        torch.cuda.synchronize()
        if r >= warmup:
            times.append(ev[0].elapsed_time(ev[1]) * 1e-3)
    return float(np.median(times)), float(min(times)), float(max(times))


def kernel_times(fn):
    """-> {kernel name: seconds} of one call, from torch.profiler; None where the profiler gives no device events"""
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


def plan_of(T, R):
    """the library's plan: (wavefronts per workgroup, k-ranges) - convex_plan() of csrc/evc_convex_plan.h restated"""
    TP, cols, cap = -(-T // 128) * 128, -(-R // 64), max(1, min(16, -(-T // 16) // 4))
    for W in (8, 4, 2):
        S = -(-512 // (TP // (16 * W) * cols))
        if S <= cap:
            return W, S
    return 2, cap


def geometries(T, R, neighbours):
    W, S = plan_of(T, R)
    out = [(0, 0, W, S)]                     # as planned (nothing forced)
    if neighbours:
        cols, TP = -(-R // 64), -(-T // 128) * 128
        for w in (8, 4, 2):
            wgs = TP // (16 * w) * cols
            for s in sorted({1, max(1, min(16, -(-512 // wgs))), max(1, min(16, -(-1024 // wgs)))}):
                if (w, s) != (W, S):
                    out.append((w, s, w, s))
    return out


def run(name, iters, repeats, warmup, neighbours):
    import torch
    from exemplars_vc_amd import _lib, learn_dictionary_convex, solve_activations_semi
    import convex_restatement as cr
    T, R, dt = CONFIGS[name]
    dev = torch.device("cuda", 0)
    tt = torch.float64 if dt == np.float64 else torch.float32
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    ev[0].record()
    ev[1].record()          # force creation of the underlying hipEvent_t
    X, assign = cr.problem(M, T, R, T + R)
    G0, H0 = cr.cluster_start(assign, R)
    Xd, G0d, H0d = (torch.from_numpy(a).to(dev, tt) for a in (X, G0, H0))
    Gd, Hd = G0d.clone(), H0d.clone()
    assert int(_lib.lib().evc_convex_splits(R, T)) == plan_of(T, R)[1]

    # the yardstick: semi-NMF with the T exemplars as dictionary and R frames - one sweep's MFMAs per iteration
    Xs = torch.from_numpy(np.random.default_rng(1).standard_normal((M, R))).to(dev, tt)
    Hs = torch.rand((T, R), dtype=tt, device=dev) + 1e-4
    ts, ts_lo, ts_hi = timed(lambda: solve_activations_semi(Xd, Xs, Hs, iters=iters, loop_events=ev), ev, repeats, warmup)

    out = []
    for fw, fs, W, S in geometries(T, R, neighbours):
        def call(events=ev):
            Gd.copy_(G0d)
            Hd.copy_(H0d)
            learn_dictionary_convex(Xd, None, None, layout="bin_major", iters=iters, check_every=0, out_g=Gd, out_h=Hd,
                                    loop_events=events, splits=fs, waves=fw)
        t, lo, hi = timed(call, ev, repeats, warmup)
        flop = float(iters) * 8.0 * T * T * R
        rec = {"config": name, "M": M, "T": T, "R": R, "dtype": np.dtype(dt).name, "iters": iters, "waves": W, "splits": S,
               "forced": bool(fw or fs), "workgroups": -(-T // 128) * 128 // (16 * W) * -(-R // 64) * S,
               "loop_s": t, "loop_s_min": lo, "loop_s_max": hi, "ms_per_iter": 1e3 * t / iters, "flop": flop,
               "frac_flop_loop": flop / t / PEAK[dt], "semi_loop_s": ts, "semi_loop_s_min": ts_lo, "semi_loop_s_max": ts_hi,
               "semi_ms_per_iter": 1e3 * ts / iters, "repeats": repeats, "warmup": warmup, "kernel": "k_convex_sweep",
               "yardstick": "evc_semi_solve N=T, R frames"}
        rows = kernel_times(lambda: call(None))
        if rows:
            names = [n for _, n, _ in rows]
            first = next(i for i, n in enumerate(names) if "k_convex_sweep" in n)         # before it: state, K = X^T X
            last = max(i for i, n in enumerate(names) if "k_convex" in n)                 # after it: W = X G
            loop = rows[first:last + 1]
            sweep = sum(d for _, n, d in loop if "k_convex_sweep" in n or "k_convex_reduce" in n)
            total = sum(d for _, _, d in loop)
            rec.update({"kernels_s": total, "sweeps_s": sweep, "sweep_share": sweep / total,
                        "sweeps_ms_per_iter": 1e3 * sweep / iters, "sweep_frac_flop": flop / sweep / PEAK[dt],
                        "ratio_to_semi": (sweep / iters) / (2.0 * ts / iters)})
        out.append(rec)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--neighbours", action="store_true")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convex_bench.jsonl"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_convex.py needs a HIP device: a CPU run gives no time")
    with open(a.out, "a") as f:
        for name in a.configs.split(","):
            for rec in run(name, a.iters, a.repeats, a.warmup, a.neighbours):
                line = json.dumps(rec)
                print(line, flush=True)
                f.write(line + "\n")


if __name__ == "__main__":
    main()
