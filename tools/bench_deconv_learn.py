"""Benchmark of the convolutive dictionary learning (evc_deconv_learn: k_deconv_v + k_deconv_update + k_deconv_v +
k_deconv_dict_grad + k_deconv_dict_apply per iteration): one JSON line per shape, tap count and loss, appended to
profiles/deconv_learn_bench.jsonl.

The iteration loop is timed with the HIP events evc_deconv_learn_opts.ev_loop_start / ev_loop_stop (median of --repeats after
--warmup calls, no error checks inside the loop); the spread is recorded as loop_s_min / loop_s_max.  In the same run
evc_nmf_learn (learn_dictionary, scikit-learn surface) is timed at the same M, R and T: it is the one-frame baseline, and
`ratio_to_learn` = loop time of the convolutive learner / loop time of the baseline, `per_tap_ratio` = that / L.  Parity: 3
iterations on the first utterances against the numpy restatement (tests/deconv_learn_restatement.py).  --tag names the build
(A/B builds of the library are chosen with EVC_LIB); --layout frame_major times the transposed caller arrays (no parity run).

    python tools/bench_deconv_learn.py [--configs compact_f64,stft_f32] [--iters K] [--repeats R] [--warmup W] [--tag T]
                                       [--layout bin_major|frame_major] [--no-parity] [--out profiles/deconv_learn_bench.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# name -> (M, R, T, utterances, dtype, tap counts, iterations, utterances of the parity run)
CONFIGS = {
    "compact_f64": (50, 512, 65536, 96, np.float64, (1, 4, 8), 10, 2),
    "stft_f32": (201, 512, 32768, 48, np.float32, (1, 4), 10, 2),
}
LOSSES = ("frobenius", "kullback-leibler")


def timed(fn, ev, repeats, warmup):
    import torch
    times = []
    for r in range(warmup + repeats):
        fn()
        torch.cuda.synchronize()
        if r >= warmup:
            times.append(ev[0].elapsed_time(ev[1]) * 1e-3)
    return float(np.median(times)), float(min(times)), float(max(times))


def run(name, iters_override, repeats, warmup, tag, parity, layout):
    import torch
    from exemplars_vc_amd import _lib, learn_dictionary, learn_dictionary_deconv
    import deconv_learn_restatement as dlr
    M, R, T, n_utt, dt, tap_counts, iters, par_utts = CONFIGS[name]
    iters = iters_override or iters
    offs = (np.arange(n_utt + 1, dtype=np.int64) * T // n_utt).astype(np.int32)
    dev = torch.device("cuda", 0)
    tt = torch.float64 if dt == np.float64 else torch.float32
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    ev[0].record()
    ev[1].record()          # force creation of the underlying hipEvent_t
    rng = np.random.default_rng(M * 7919 + R)
    X = rng.random((M, T)) ** 2 + 1e-3
    H0 = rng.random((R, T)) + 0.1
    fm = layout == "frame_major"
    lay = (lambda t: t.transpose(-1, -2).contiguous()) if fm else (lambda t: t)
    Xd, Hd = lay(torch.from_numpy(X).to(dev, tt)), lay(torch.from_numpy(H0).to(dev, tt))
    out = []
    for L in tap_counts:
        W0 = rng.random((L, M, R)) + 0.1
        Wd = lay(torch.from_numpy(W0).to(dev, tt))
        for loss in LOSSES:
            # the baseline sees the same X and the first tap; its time does not depend on the values
            tb, tb_lo, tb_hi = timed(lambda: learn_dictionary(Xd, Wd[0], Hd, layout=layout, iters=iters, check_every=0,
                                                              loss=loss, loop_events=ev), ev, repeats, warmup)
            t, lo, hi = timed(lambda: learn_dictionary_deconv(Xd, Wd, Hd, loss=loss, layout=layout, iters=iters,
                                                              check_every=0, utt_offsets=offs, loop_events=ev), ev, repeats, warmup)
            rec = {"config": name, "tag": tag, "layout": layout, "loss": loss, "taps": L, "M": M, "R": R, "T": T, "n_utt": n_utt,
                   "dtype": np.dtype(dt).name, "iters": iters, "loop_s": t, "loop_s_min": lo, "loop_s_max": hi,
                   "ms_per_iter": 1e3 * t / iters, "learn_loop_s": tb, "learn_loop_s_min": tb_lo, "learn_loop_s_max": tb_hi,
                   "learn_ms_per_iter": 1e3 * tb / iters, "ratio_to_learn": t / tb, "per_tap_ratio": t / tb / L,
                   "splits": int(_lib.lib().evc_deconv_learn_splits(M, R, T, n_utt, L)),
                   "learn_splits": int(_lib.lib().evc_learn_splits(M, R, T)), "repeats": repeats, "warmup": warmup,
                   "baseline": "evc_nmf_learn"}
            if parity and not fm:
                Tp = int(offs[par_utts])
                po = offs[:par_utts + 1]
                Wg, Hg = learn_dictionary_deconv(Xd[:, :Tp], Wd, Hd[:, :Tp], loss=loss, layout="bin_major", iters=3,
                                                 check_every=0, utt_offsets=po)
                xr, wr, hr = (a.astype(dt).astype(np.float64) for a in (X[:, :Tp], W0, H0[:, :Tp]))
                Wr, Hr, _, _ = dlr.learn(wr, xr, hr, loss, 3, po)
                Wg, Hg = Wg.cpu().numpy().astype(np.float64), Hg.cpu().numpy().astype(np.float64)
                rec["parity_rel_w_3it"] = float(np.linalg.norm(Wg - Wr) / np.linalg.norm(Wr))
                rec["parity_rel_h_3it"] = float(np.linalg.norm(Hg - Hr) / np.linalg.norm(Hr))
            out.append(rec)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--iters", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tag", default="")
    ap.add_argument("--no-parity", action="store_true")
    ap.add_argument("--layout", default="bin_major", choices=("bin_major", "frame_major"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deconv_learn_bench.jsonl"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_deconv_learn.py needs a HIP device: a CPU run gives no time")
    with open(a.out, "a") as f:
        for name in a.configs.split(","):
            for rec in run(name, a.iters, a.repeats, a.warmup, a.tag, not a.no_parity, a.layout):
                line = json.dumps(rec)
                print(line, flush=True)
                f.write(line + "\n")


if __name__ == "__main__":
    main()
