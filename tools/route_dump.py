"""What the host layer of libevc_hip.so decides and delivers, one sorted line per case of a fixed, seeded list, so that the
outputs of two builds can be compared with `cmp`:

    python tools/route_dump.py --sizes              # no device needed: the three size queries over a grid
    python tools/route_dump.py --solves             # one solve per case: evc_solve_info, n_iter, sha256 of H (and Y)
    EVC_LIB=/path/to/other/libevc_hip.so python tools/route_dump.py --solves --out other.txt

A change that only moves host code (routing, carving, the drivers' shared steps) must leave both outputs byte-identical.
"""
import argparse
import hashlib
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

MS = [1, 16, 17, 25, 32, 33, 64, 144, 145, 176, 177, 201, 208, 209, 257, 513, 528, 529, 1025]
MBS = [0, 25, 40, 513]
NS = [15, 16, 512, 4096, 16384]
TS = [1, 90, 688, 11008, 70000]
UTTS = [1, 16]


def size_lines():
    """evc_workspace_bytes / evc_dict_bytes / evc_cd_workspace_bytes.  One line per shape; the values of a line run over
    n_utt x dtype x algo (workspace), dtype x loss (dict), n_utt x dtype (cd), in that nesting."""
    from exemplars_vc_amd import _lib
    L = _lib.lib()
    out = []
    for M, Mb, N, T in itertools.product(MS, MBS, NS, TS):
        v = [L.evc_workspace_bytes(M, Mb, N, T, U, dt, algo) for U in UTTS for dt in (0, 1) for algo in (0, 1, 2, 3)]
        out.append("ws M=%d Mb=%d N=%d T=%d : %s" % (M, Mb, N, T, " ".join(map(str, v))))
    for M, Mb, N in itertools.product(MS, MBS, NS):
        v = [L.evc_dict_bytes(M, Mb, N, dt, loss) for dt in (0, 1) for loss in (0, 1)]
        out.append("dict M=%d Mb=%d N=%d : %s" % (M, Mb, N, " ".join(map(str, v))))
    for M, N, T in itertools.product(MS, NS, TS):
        v = [L.evc_cd_workspace_bytes(M, N, T, U, dt) for U in UTTS for dt in (0, 1)]
        out.append("cd M=%d N=%d T=%d : %s" % (M, N, T, " ".join(map(str, v))))
    return out


def solve_cases():
    """(name, dict(dtype, M, N, utts, frames=688, Mb=0, prepared=False, given=False, want_h=True), solver keywords)."""
    cases = []

    def add(name, dtype, M, N, utts, frames=688, Mb=0, prepared=False, given=False, want_h=True, **kw):
        kw.setdefault("iters", 10)
        cases.append((name, dict(dtype=dtype, M=M, N=N, utts=utts, frames=frames, Mb=Mb, prepared=prepared, given=given,
                                 want_h=want_h), kw))

    # float64, M <= 32: k_fused_all with one and several members, k_fused_mu (N = 256), every batch size
    for N, U in itertools.product([256, 512, 4096, 16384], [1, 2, 16]):
        add("f64_m25_n%d_u%d" % (N, U), "f64", 25, N, U)
    for M, N in itertools.product([16, 32], [512, 4096]):
        add("f64_m%d_n%d_u1" % (M, N), "f64", M, N, 1)
    # the flags, at one and at sixteen utterances (k_fused_res cooperative and alone behind all_resident=False)
    for U in (1, 16):
        for key, val in (("fused", False), ("exact_div", True), ("cooperative", False), ("all_resident", False),
                         ("pair_tiles", True), ("fused_c", 1), ("fused_c", 2)):
            add("f64_m25_n4096_u%d_%s=%s" % (U, key, val), "f64", 25, 4096, U, **{key: val})
    add("f64_m25_n4096_u1_noexch_nores", "f64", 25, 4096, 1, cooperative=False, all_resident=False)
    for eps_mode, N in itertools.product(["add", "zero_replace", "clamp", "none"], [512, 4096]):
        add("f64_m25_n%d_u2_eps=%s" % (N, eps_mode), "f64", 25, N, 2, eps_mode=eps_mode)
    for N in (512, 4096, 16384):
        add("f64_m25_n%d_u2_kl" % N, "f64", 25, N, 2, loss="kl", eps_mode="zero_replace")
    for name, kw in (("stop_none", dict(check_every=10)), ("stop_sklearn", dict(check_every=10, stop_rule="sklearn", tol=1e-3)),
                     ("stop_pymf", dict(check_every=10, stop_rule="pymf", tol=1e-9))):
        add("f64_m25_n4096_u2_" + name, "f64", 25, 4096, 2, iters=30, **kw)
        add("f64_m25_n512_u16_" + name, "f64", 25, 512, 16, iters=30, **kw)
        add("f32_m201_n4096_u2_" + name, "f32", 201, 4096, 2, iters=30, **kw)
        add("f64_m513_n1024_u3_" + name, "f64", 513, 1024, 3, iters=30, **kw)
        add("f64_m201_n1024_u1_" + name, "f64", 201, 1024, 1, iters=30, **kw)
    for fam, (dtype, M, N, U) in (("all", ("f64", 25, 4096, 2)), ("wide", ("f32", 201, 4096, 2)),
                                  ("wide64", ("f64", 513, 1024, 3)), ("gemm", ("f64", 201, 1024, 1)),
                                  ("staged", ("f32", 25, 4096, 2))):
        add("init_const_" + fam, dtype, M, N, U, init="const", init_value=0.5)
        add("init_given_" + fam, dtype, M, N, U, given=True)
    # float32 riding the float64 kernels
    add("f32_m25_n4096_u1", "f32", 25, 4096, 1)
    add("f32_m25_n512_u16", "f32", 25, 512, 16)
    # k_fused_wide: tagged, static, ticket queue; the contractions below 43 frame tiles
    for M, U in itertools.product([64, 201], [1, 2, 8, 16]):
        add("f32_m%d_n4096_u%d" % (M, U), "f32", M, 4096, U)
    for M in (64, 201):
        add("f32_m%d_n4096_t90" % M, "f32", M, 4096, 1, frames=90)
    add("f32_m201_n4096_u2_fused_c=2", "f32", 201, 4096, 2, fused_c=2)
    add("f32_m201_n4096_u2_fused_w=4", "f32", 201, 4096, 2, fused_w=4)
    add("f32_m201_n4096_u2_fused_w=8", "f32", 201, 4096, 2, fused_w=8)
    add("f32_m201_n4096_t90_fused_c=1", "f32", 201, 4096, 1, frames=90, fused_c=1)
    for U in (2, 16):       # several stop checks per launch
        add("f32_m201_n4096_u%d_checks" % U, "f32", 201, 4096, U, iters=30, check_every=5, stop_rule="sklearn", tol=1e-3)
    add("f32_m201_n4096_u2_kl", "f32", 201, 4096, 2, loss="kl", eps_mode="zero_replace")
    # float64 wide spectra: both sides of every window of the routing
    for M, N, U in itertools.product([160, 201, 257, 513], [1024, 8192], [1, 2, 3, 16]):
        add("f64_m%d_n%d_u%d" % (M, N, U), "f64", M, N, U)
    add("f64_m513_n1024_u3_fused_w=8", "f64", 513, 1024, 3, fused_w=8)
    add("f64_m513_n1024_u3_exact_div", "f64", 513, 1024, 3, exact_div=True)
    for algo in ("gram", "literal"):
        add("f64_m25_n512_u2_" + algo, "f64", 25, 512, 2, algo=algo)
        add("f64_m201_n1024_u2_" + algo, "f64", 201, 1024, 2, algo=algo)
        add("f32_m201_n1024_u2_" + algo, "f32", 201, 1024, 2, algo=algo)
    # convert
    for Mb in (25, 40, 513):
        add("convert_f64_m25_mb%d" % Mb, "f64", 25, 4096, 2, Mb=Mb)
        add("convert_f64_m25_mb%d_noh" % Mb, "f64", 25, 4096, 2, Mb=Mb, want_h=False)
    add("convert_f32_m25_mb25", "f32", 25, 4096, 2, Mb=25)
    add("convert_f32_m201_mb40", "f32", 201, 4096, 2, Mb=40)
    add("convert_f32_m201_mb40_noh", "f32", 201, 4096, 2, Mb=40, want_h=False)
    add("convert_f64_m513_mb513", "f64", 513, 1024, 3, Mb=513)
    add("convert_f64_m201_mb25_gemm", "f64", 201, 1024, 1, Mb=25)
    # prepared dictionaries, every family
    add("prep_f64_m25", "f64", 25, 4096, 2, prepared=True)
    add("prep_f64_m25_mb25", "f64", 25, 4096, 2, Mb=25, prepared=True)
    add("prep_f64_m25_mb40_noh", "f64", 25, 4096, 2, Mb=40, prepared=True, want_h=False)
    add("prep_f64_m25_kl", "f64", 25, 4096, 2, prepared=True, loss="kl", eps_mode="zero_replace")
    add("prep_f64_m25_res", "f64", 25, 4096, 1, prepared=True, all_resident=False)
    add("prep_f32_m25_mb25", "f32", 25, 4096, 2, Mb=25, prepared=True)
    add("prep_f32_m201_mb40", "f32", 201, 4096, 2, Mb=40, prepared=True)
    add("prep_f32_m201_kl", "f32", 201, 4096, 2, prepared=True, loss="kl", eps_mode="zero_replace")
    add("prep_f64_m513", "f64", 513, 1024, 3, prepared=True)
    add("prep_f64_m201_gemm", "f64", 201, 1024, 1, prepared=True)
    add("prep_f32_m201_t90_gemm", "f32", 201, 4096, 1, frames=90, prepared=True)
    # the documented test hook: both redo paths, once per exchanging family
    for fake in (True, 2):
        kw = dict(iters=20, check_every=5, _fake_coop_timeout=fake)
        add("fake=%s_all" % fake, "f64", 25, 4096, 2, **kw)
        add("fake=%s_all_given" % fake, "f64", 25, 4096, 2, given=True, **kw)
        add("fake=%s_res_coop" % fake, "f64", 25, 4096, 1, all_resident=False, **kw)
        add("fake=%s_staged" % fake, "f32", 25, 4096, 2, **kw)
        add("fake=%s_wide" % fake, "f32", 201, 4096, 2, **kw)
        add("fake=%s_wide64" % fake, "f64", 513, 1024, 3, **kw)
        # a widened caller H0 that must survive the first attempt, and a prepared image reused by the second
        add("fake=%s_staged_given" % fake, "f32", 25, 4096, 2, given=True, **kw)
        add("fake=%s_prep_all" % fake, "f64", 25, 4096, 2, Mb=25, prepared=True, **kw)
    # k_fused_all, one utterance of 90 frames: every exchange body and both fragment sources.  2 and 4 members (direct,
    # dictionary in LDS), 3 members (ragged slices), M = 12 (ragged, fewer elements than threads), 8 members at M = 28
    # (whole slices, dictionary streamed), 16 members; KL with one member and with 16
    for M, N in ((25, 1024), (25, 2048), (25, 1536), (12, 1536), (28, 4096), (25, 8192)):
        add("f64_m%d_n%d_t90" % (M, N), "f64", M, N, 1, frames=90)
    for N in (512, 8192):
        add("f64_m25_n%d_t90_kl" % N, "f64", 25, N, 1, frames=90, loss="kl", eps_mode="zero_replace")
    return cases


def solve_lines():
    import torch
    import exemplars_vc_amd as evc
    dev = torch.device("cuda", 0)

    def sha(t):
        return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()[:32]

    out = []
    for idx, (name, c, kw) in enumerate(solve_cases()):
        rng = np.random.default_rng(1000 + idx)
        npdt = np.float64 if c["dtype"] == "f64" else np.float32
        M, N, U, Mb = c["M"], c["N"], c["utts"], c["Mb"]
        T = U * c["frames"]
        A = torch.from_numpy((rng.random((M, N)) + 0.01).astype(npdt)).to(dev)
        X = torch.from_numpy((rng.random((M, T)) + 0.01).astype(npdt)).to(dev)
        B = torch.from_numpy((rng.random((Mb, N)) + 0.01).astype(npdt)).to(dev) if Mb else None
        H0 = torch.from_numpy((rng.random((N, T)) + 0.01).astype(npdt)).to(dev) if c["given"] else None
        if U > 1:
            kw = dict(kw, utt_offsets=[u * c["frames"] for u in range(U + 1)])
        a_arg, b_arg = A, B
        if c["prepared"]:
            pkw = {k: kw[k] for k in ("loss",) if k in kw}
            a_arg, b_arg = evc.prepare_dictionary(A, B, dtype=c["dtype"], **pkw), None
        if Mb:
            res = evc.convert(a_arg, X, b_arg, H0, want_h=c["want_h"], dtype=c["dtype"], info=True, **kw)
        else:
            res = evc.solve_activations(a_arg, X, H0, dtype=c["dtype"], info=True, **kw)
        info = res[-1]
        mats = " ".join(sha(t) for t in res[:-1])
        var = info["variant"]
        # (the contraction kernels report blocks: (frames, rows) pairs, None where a solve forms no such product)
        fmt = lambda v: "-" if v is None else ("%dx%d" % v if isinstance(v, tuple) else "%d" % int(v))
        var = "-" if var is None else ",".join("%s=%s" % (k, fmt(v)) for k, v in sorted(var.items()))
        out.append("solve %s : kernel=%s members=%d launches=%d redo=%d exchange=%d prepared=%d variant=%s n_iter=%s : %s" % (
            name, info["kernel"], info["members"], info["launches"], info["redo"], info["exchange"], info["prepared"], var,
            ",".join(map(str, info["n_iter"].tolist())), mats))
        del A, X, B, H0, res, a_arg, b_arg
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", action="store_true", help="the size queries (no device needed)")
    ap.add_argument("--solves", action="store_true", help="one solve per case (needs a device)")
    ap.add_argument("--out", default=None, help="write the lines to this file instead of the standard output")
    a = ap.parse_args()
    if not (a.sizes or a.solves):
        ap.error("give --sizes, --solves or both")
    lines = (size_lines() if a.sizes else []) + (solve_lines() if a.solves else [])
    text = "\n".join(sorted(lines)) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
        print("%d lines, sha256 %s -> %s" % (len(lines), hashlib.sha256(text.encode()).hexdigest()[:16], a.out))
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
