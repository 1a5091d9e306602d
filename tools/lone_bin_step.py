#!/usr/bin/env python3
"""One C2-shaped solve (M = 25, N = 4096, 100 iterations, 256 x 688 frames, float64) on k_fused_all's own unit or on
k_fused_lone's (--lone 0 is EVC_FLAG_NO_LONE_BIN) or, with --lone 1, on k_fused_quad's (the default; --quad 0 is
EVC_FLAG_NO_QUAD_ROWS: k_fused_lone), for A/B timing and for counter / kernel-trace runs of each kernel:

    python tools/lone_bin_step.py --lone 0 --reps 6
    rocprofv3 --pmc SQ_INSTS_MFMA -d out/pmc1 -o p --output-format csv -- python3 tools/lone_bin_step.py --lone 1 --reps 1
    rocprofv3 --kernel-trace --stats -d out/kt1 -o p --output-format csv -- python3 tools/lone_bin_step.py --lone 1

bench.py measures the default route and has no switch for this flag; the operands here stay on the device, as in its timed
loop.  Prints one JSON line: the calls' times (events around each call) and frames/s of the median."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lone", type=int, default=1)
    ap.add_argument("--quad", type=int, default=1)
    ap.add_argument("--exemplars", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=256 * 688)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    import torch
    import exemplars_vc_amd as evc
    from oracle import evc_oracle as o
    M, N, T = 25, a.exemplars, a.frames
    p = o.synth_problem(M, N, 688, seed=20190131)
    dev = torch.device("cuda", 0)
    A = torch.from_numpy(p["A"]).to(dev)
    X = torch.from_numpy(np.tile(p["X"], (1, (T + 687) // 688))[:, :T].copy()).to(dev)
    out = torch.empty((N, T), dtype=torch.float64, device=dev)
    kw = dict(iters=a.iters, eps_mode="zero_replace", init="sklearn", out=out, lone_bin=bool(a.lone), quad_rows=bool(a.quad))
    info = None
    ms = []
    for i in range(a.warmup + a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _, info = evc.solve_activations(A, X, info=True, **kw)
        e1.record()
        torch.cuda.synchronize()
        if i >= a.warmup:
            ms.append(e0.elapsed_time(e1))
    med = float(np.median(ms))
    print(json.dumps({"lone": a.lone, "quad": a.quad, "M": M, "N": N, "T": T, "iters": a.iters, "ms": ms, "median_ms": med,
                      "frames_per_s": T / med * 1e3, "kernel": info["kernel"], "members": info["members"],
                      "redo": info["redo"], "checksum": float(out.sum())}))


if __name__ == "__main__":
    main()
