#!/usr/bin/env python3
"""evc_mfcc timing on the GPU box: the MFCC alignment features of the dictionary build, sr 16000,
fft 400, hop 80, 128 mel bands, 20 coefficients, device-resident in and out.

  one     one utterance of 688 frames
  c4      the 162-utterance ragged set of BASELINE C4 for one speaker (lengths of the bundled audio, cycled)
Per shape (HIP events around REP calls after a warm-up, median of ROUNDS):
  (a) evc_mfcc without and with the STFT parts re / im
  (b) the way to the same STFT frames before evc_mfcc: one evc_stft call per utterance
  (c) the numpy restatement of the tests on this host (one round)
  (d) with --profile-loop N: only N calls of (a, with re / im) on the c4 shape, for a kernel trace taken around this
      program in a run of its own (the split between the DFT contraction and the two new kernels)
Writes one JSON line per measurement to stdout and, with --out FILE, appends them to FILE."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import exemplars_vc_amd as evc  # noqa: E402

C4_LENGTHS = [704, 216, 513, 494, 945, 640, 497, 1370, 688]     # frames, as bench.py's C4
F, HOP = 400, 80


def signals(frames, seed):
    rng = np.random.default_rng(seed)
    out = []
    for T in frames:
        n = (T - 1) * HOP
        t = np.arange(n) / 16000.0
        env = (0.55 + 0.45 * np.sin(2 * np.pi * 1.7 * t + rng.uniform(0, 6))) ** 2
        out.append(env * np.sin(2 * np.pi * rng.uniform(90, 240) * t) + 0.01 * rng.standard_normal(n))
    return out


def timed(fn, rep, rounds):
    """median over `rounds` of the mean time of `rep` calls, HIP events, in microseconds"""
    fn()
    torch.cuda.synchronize()
    res = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(rep):
            fn()
        e1.record()
        torch.cuda.synchronize()
        res.append(e0.elapsed_time(e1) * 1e3 / rep)
    return float(np.median(res)), float(np.min(res)), float(np.max(res))


class Native:
    """The C ABI called directly on buffers made once: no Python plumbing inside the timed loop."""

    def __init__(self, dev):
        import ctypes as C
        from exemplars_vc_amd import _lib
        self.C, self.L = C, _lib.lib()
        self.n = len(dev)
        self.x = torch.cat(dev)
        self.lens = [int(t.numel()) for t in dev]
        self.soff = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)
        self.foff = np.concatenate([[0], np.cumsum([1 + n // HOP for n in self.lens])])
        T = int(self.foff[-1])
        o = _lib.MfccOpts()
        o.struct_bytes = C.sizeof(_lib.MfccOpts)
        o.sr, o.fft_size, o.hop, o.n_mels, o.n_mfcc, o.center = 16000, F, HOP, 128, 20, 1
        o.fmin, o.fmax, o.amin, o.top_db = 0.0, 0.0, 1e-10, 80.0
        self.o = o
        self.sp = self.soff.ctypes.data_as(C.POINTER(C.c_long))
        nbytes = max(int(self.L.evc_mfcc_workspace_bytes(self.sp, self.n, C.byref(o))),
                     max(int(self.L.evc_stft_workspace_bytes(n, F, HOP, 1)) for n in self.lens))
        self.ws_bytes = nbytes
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        self.mf = torch.empty(T, 20, dtype=torch.float64, device="cuda")
        self.re = torch.empty(T, F // 2 + 1, dtype=torch.float64, device="cuda")
        self.im = torch.empty_like(self.re)
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def mfcc(self, want_stft):
        C, nb = self.C, F // 2 + 1
        st = self.L.evc_mfcc(self.x.data_ptr(), self.sp, self.n, C.byref(self.o), self.mf.data_ptr(), 20,
                             self.re.data_ptr() if want_stft else None, nb, self.im.data_ptr() if want_stft else None, nb,
                             self.ws.data_ptr(), self.ws.numel(), self.stream)
        assert st == 0, st

    def stft_each(self):
        nb = F // 2 + 1
        for u in range(self.n):
            st = self.L.evc_stft(self.x.data_ptr() + 8 * int(self.soff[u]), self.lens[u], F, HOP, 1,
                                 self.re.data_ptr() + 8 * nb * int(self.foff[u]), nb,
                                 self.im.data_ptr() + 8 * nb * int(self.foff[u]), nb, self.ws.data_ptr(), self.ws.numel(),
                                 self.stream)
            assert st == 0, st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--profile-loop", type=int, default=0)
    a = ap.parse_args()
    shapes = {"one": [688], "c4": [C4_LENGTHS[i % len(C4_LENGTHS)] for i in range(162)]}
    lines = []

    def emit(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    if a.profile_loop:
        nat = Native([torch.from_numpy(y).cuda() for y in signals(shapes["c4"], 1)])
        for _ in range(a.profile_loop):
            nat.mfcc(True)
        torch.cuda.synchronize()
        return
    import mfcc_restatement as mr
    for name, frames in shapes.items():
        host = signals(frames, 1)
        dev = [torch.from_numpy(y).cuda() for y in host]
        T = sum(frames)
        rep = 50 if name == "one" else 10
        got = evc.mfcc_batch(dev)
        assert sum(g.shape[0] for g in got) == T
        nat = Native(dev)
        for label, fn in (("evc_mfcc", lambda: nat.mfcc(False)),
                          ("evc_mfcc + re/im", lambda: nat.mfcc(True)),
                          ("evc_stft per utterance", nat.stft_each),
                          ("solver.mfcc_batch (Python plumbing included)", lambda: evc.mfcc_batch(dev))):
            med, lo, hi = timed(fn, rep, a.rounds)
            emit(shape=name, utterances=len(frames), frames=T, what=label, call_us=med, min_us=lo, max_us=hi,
                 frames_per_s=T / med * 1e6, rep=rep, rounds=a.rounds, workspace_mib=nat.ws_bytes / 2 ** 20)
        t0 = time.perf_counter()
        want = [mr.mfcc(y) for y in host]
        dt = time.perf_counter() - t0
        dev_max = max(float(np.abs(g.cpu().numpy() - w).max()) for g, w in zip(got, want))
        emit(shape=name, utterances=len(frames), frames=T, what="numpy restatement (host)", call_us=dt * 1e6,
             frames_per_s=T / dt, max_abs_deviation_of_evc_mfcc=dev_max)
    if a.out:
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
