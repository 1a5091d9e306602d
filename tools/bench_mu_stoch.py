"""Benchmark of the mini-batch multiplicative-update learning (evc_mu_stoch_learn): one JSON line per shape, method and route,
appended to profiles/mu_stoch_bench.jsonl.

The epoch loop is timed with the HIP events evc_mu_stoch_opts.ev_loop_start / ev_loop_stop (median of --repeats calls after
--warmup; tol = 0 and no outputs, so the call only enqueues and nothing waits inside the loop).  Every shape and method is
timed on both routes of the dictionary half in the same run: "unfused" is the yardstick - copy2d, gemm_nt, k_mum_dict_q and
k_dict_grad, the kernels evc_mu_masked_learn had before this entry existed - and "fused" is k_mus_dict_grad.  `ms_per_step`
is the loop time over epochs * (T // batch_size) steps (svrmu's full-gradient pass at every epoch's start is inside it),
`launches_per_step` the launches the driver enqueues per step on that route (gemm_nt counted as one), `fused_over_unfused` the
ratio of the two routes' times on the fused line.  No target is fixed.

    python tools/bench_mu_stoch.py [--configs f32_m201_r64,f64_m25_r64,...] [--epochs E] [--repeats R] [--warmup W]
                                   [--out profiles/mu_stoch_bench.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name -> (M, R, T, batch size, dtype)
CONFIGS = {
    "f32_m201_r64": (201, 64, 16 * 688, 256, np.float32),
    "f64_m25_r64": (25, 64, 64 * 688, 1024, np.float64),
    "f32_m201_r256": (201, 256, 16 * 688, 256, np.float32),
    "f64_m25_r256": (25, 256, 64 * 688, 1024, np.float64),
}
METHODS = ("asg", "asag", "gsag", "svrmu")


def problem(M, R, T, seed):
    rng = np.random.default_rng(seed)
    W = rng.random((R, M)) ** 2 + 1e-3
    k = min(R, 64)
    X = (rng.random((T, k)) * (rng.random((T, k)) < 0.2)) @ W[:k] + 1e-3 * rng.random((T, M)) + 1e-4
    mask = (rng.random((T, M)) < 0.7).astype(np.float64)
    return X, W, rng.random((T, R)) + 0.125, mask


def launches_per_step(method, route, n_loop):
    """gather, pack, sweep, scatter | the gradient slabs | apply, commit"""
    grads = 1 if route == "fused" else 4
    n = 4 + grads + 2.0
    if method == "gsag":
        n -= 1.0 - 1.0 / n_loop                 # one commit per epoch
    if method == "svrmu":
        n += 2 + grads                          # the full-gradient pass: gather, the slabs, apply
    return n


def timed(fn, ev, repeats, warmup):
    import torch
    times = []
    for r in range(warmup + repeats):
        fn()
        torch.cuda.synchronize()
        if r >= warmup:
            times.append(ev[0].elapsed_time(ev[1]))
    return float(np.median(times)), float(min(times)), float(max(times))


def run(name, epochs, repeats, warmup):
    import torch
    from exemplars_vc_amd import learn_dictionary_stochastic
    M, R, T, bs, dt = CONFIGS[name]
    X, W, H, mask = problem(M, R, T, M * 7919 + R)
    dev = torch.device("cuda", 0)
    tt = torch.float64 if dt == np.float64 else torch.float32
    Xd, Wd, Hd, Md = (torch.from_numpy(m).to(dev, tt) for m in (X, W, H, mask))
    order = np.stack([np.random.default_rng(e).permutation(T) for e in range(epochs)]).astype(np.int32)
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    ev[0].record()
    ev[1].record()          # force creation of the underlying hipEvent_t
    n_loop, out = T // bs, []
    for method in METHODS:
        recs = {}
        for route in ("unfused", "fused"):
            Wc, Hc = Wd.clone(), Hd.clone()

            def call():
                Wc.copy_(Wd)
                Hc.copy_(Hd)
                learn_dictionary_stochastic(Xd, None, None, Md, method=method, loss="kl", layout="frame_major", batch_size=bs,
                                            epochs=epochs, tol=0.0, order=order[:1] if method == "svrmu" else order, route=route,
                                            out_w=Wc, out_h=Hc, loop_events=ev)
            t, lo, hi = timed(call, ev, repeats, warmup)
            steps = epochs * n_loop
            recs[route] = {"config": name, "method": method, "route": route, "loss": "kl", "masked": True, "M": M, "R": R, "T": T,
                           "batch_size": bs, "dtype": np.dtype(dt).name, "epochs": epochs, "steps": steps, "loop_ms": t,
                           "loop_ms_min": lo, "loop_ms_max": hi, "ms_per_step": t / steps,
                           "launches_per_step": launches_per_step(method, route, n_loop), "repeats": repeats, "warmup": warmup}
        recs["fused"]["fused_over_unfused"] = recs["fused"]["loop_ms"] / recs["unfused"]["loop_ms"]
        out += [recs["unfused"], recs["fused"]]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mu_stoch_bench.jsonl"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mu_stoch.py needs a HIP device: a CPU run gives no time")
    with open(a.out, "a") as f:
        for name in a.configs.split(","):
            for rec in run(name, a.epochs, a.repeats, a.warmup):
                line = json.dumps(rec)
                print(line, flush=True)
                f.write(line + "\n")


if __name__ == "__main__":
    main()
