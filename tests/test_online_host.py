"""Mini-batch dictionary learning (evc_online_learn), host side: the C ABI's declarations, struct mirror and argument
checks, the numpy restatement against scikit-learn's recorded MiniBatchNMF runs (tests/golden/online_sk_*.npz), the
fixture generator and the Python surfaces' validation.  No GPU needed."""
import ctypes as C
import glob
import inspect
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import online_restatement as onr  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "online_sk_*.npz")))
ZERO_MSG = "When beta_loss <= 0 and X contains zeros, the solver may diverge"
E64 = 2.0 ** -52
KEYS = {"X", "W0", "H0", "W", "H", "n_iter", "n_steps", "cost", "change", "batch_size", "max_iter", "tol",
        "max_no_improvement", "forget_factor", "beta", "alpha", "l1_ratio", "dtype", "margin"}


def lib():
    from exemplars_vc_amd import _lib
    return _lib, _lib.lib()


def options(d):
    """what a fixture was recorded with, as online_restatement.learn takes it (penalties as scikit-learn scales them: those
    of the activations by the bins, those of the dictionary per frame)"""
    M = d["X"].shape[0]
    a, r = float(d["alpha"]), float(d["l1_ratio"])
    mni = int(d["max_no_improvement"])
    return dict(beta=float(d["beta"]), batch_size=int(d["batch_size"]), max_iter=int(d["max_iter"]),
                forget_factor=float(d["forget_factor"]), tol=float(d["tol"]), max_no_improvement=None if mni < 0 else mni,
                l1_h=M * a * r, l2_h=M * a * (1 - r), l1_w=a * r, l2_w=a * (1 - r))


def test_symbols_declared_and_exported():
    _lib, L = lib()
    hdr = open(os.path.join(ROOT, "include", "evc.h")).read()
    declared = set(re.findall(r"\b(evc_[a-z_0-9]+)\s*\(", hdr))
    for sym in ("evc_online_learn", "evc_online_workspace_bytes", "evc_online_splits"):
        assert sym in declared and sym in _lib.SYMBOLS and hasattr(L, sym)
    assert "evc_online_learn " in hdr[:hdr.index("#ifndef EVC_H")]          # listed in the header comment
    sync = hdr[hdr.index("Host synchronisation"):hdr.index("No global mutable state")]
    assert "(10) evc_online_learn" in sync
    body = hdr[hdr.index("Mini-batch (online) dictionary learning"):]
    for out_of_scope in ("fresh_restarts=True", "partial_fit", "sparse X", "shuffled"):
        assert out_of_scope in body
    assert L.evc_version() == 100


def test_opts_mirror_matches_header():
    _lib, _ = lib()
    hdr = open(os.path.join(ROOT, "include", "evc.h")).read()
    body = hdr[hdr.index("typedef struct evc_online_opts {"):hdr.index("} evc_online_opts;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for grp in re.findall(r"\b(?:int|double|void\*)\s+([a-zA-Z_0-9, ]+);", body)
             for n in grp.replace(" ", "").split(",")]
    assert names == [f[0] for f in _lib.OnlineOpts._fields_]
    assert names == ["struct_bytes", "dtype", "layout", "batch_size", "max_iter", "max_no_improvement", "resume", "reserved",
                     "beta", "tol", "forget_factor", "l1_h", "l2_h", "l1_w", "l2_w", "ev_loop_start", "ev_loop_stop"]
    assert C.sizeof(_lib.OnlineOpts) == 8 * 4 + 7 * 8 + 2 * 8


def _opts(_lib, **kw):
    o = _lib.OnlineOpts()
    o.struct_bytes = C.sizeof(_lib.OnlineOpts)
    o.dtype, o.layout, o.batch_size, o.max_iter, o.max_no_improvement = _lib.F64, _lib.FRAME_MAJOR, 32, 5, 10
    o.beta, o.tol, o.forget_factor = 0.5, 1e-4, 0.7
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_bad_arguments_rejected_before_device_work():
    _lib, L = lib()
    one = C.c_void_p(8)              # never dereferenced: every case fails validation first

    def call(o, M=25, R=17, T=70, ldx=25, ldw=25, ldh=17, lda=25, ws=1 << 40, X=one, W=one, H=one, A=one, B=one, wsp=one):
        return L.evc_online_learn(X, ldx, W, ldw, H, ldh, A, B, lda, M, R, T, C.byref(o), wsp, ws, None, None, None, None)
    bad = _opts(_lib)
    bad.struct_bytes = 4
    assert call(bad) == -1
    assert L.evc_online_learn(one, 25, one, 25, one, 17, one, one, 25, 25, 17, 70, None, one, 1 << 40, None, None, None,
                              None) == -1
    assert call(_opts(_lib), M=0) == -1
    assert call(_opts(_lib), R=0) == -1
    assert call(_opts(_lib), T=0) == -1
    for ld in ("ldx", "ldw", "lda"):
        assert call(_opts(_lib), **{ld: 24}) == -1
    assert call(_opts(_lib), ldh=16) == -1
    for ld in (dict(ldx=69), dict(ldw=16), dict(ldh=69), dict(lda=16)):
        assert call(_opts(_lib, layout=_lib.BIN_MAJOR), **dict(dict(ldx=70, ldw=17, ldh=70, lda=17), **ld)) == -1
    assert call(_opts(_lib, layout=_lib.BIN_MAJOR), ldx=70, ldw=17, ldh=70, lda=17, ws=16) == -2
    for p in ("X", "W", "H", "A", "B", "wsp"):
        assert call(_opts(_lib), **{p: None}) == -1
    for v in (float("nan"), float("inf"), -float("inf")):
        assert call(_opts(_lib, beta=v)) == -1
    for f in ("tol", "l1_h", "l2_h", "l1_w", "l2_w"):
        assert call(_opts(_lib, **{f: -1e-4})) == -1
        assert call(_opts(_lib, **{f: float("nan")})) == -1
    for v in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        assert call(_opts(_lib, forget_factor=v)) == -1
    assert call(_opts(_lib, forget_factor=1.0), ws=16) == -2
    assert call(_opts(_lib, batch_size=0)) == -1
    assert call(_opts(_lib, batch_size=-3)) == -1
    assert call(_opts(_lib, max_iter=-1)) == -1
    assert call(_opts(_lib, max_iter=0), ws=16) == -2
    assert call(_opts(_lib, batch_size=1, max_iter=1 << 30)) == -1        # more steps than n_steps_out can count
    assert call(_opts(_lib, resume=2)) == -1
    assert call(_opts(_lib, resume=1), ws=16) == -2
    assert call(_opts(_lib, max_no_improvement=-1, tol=0.0), ws=16) == -2
    assert call(_opts(_lib, dtype=7)) == -1
    assert call(_opts(_lib, layout=5)) == -1
    for r in (1, 0x80, 65 << 8, 3 << 16, 1 << 18, -1):            # low bits, too many ranges, route 3, a bit beyond
        assert call(_opts(_lib, reserved=r)) == -1
    assert call(_opts(_lib, reserved=(64 << 8) | (2 << 16)), ws=16) == -2
    assert call(_opts(_lib), ws=16) == -2                         # workspace too small
    assert call(_opts(_lib), ws=int(L.evc_online_workspace_bytes(25, 17, 70, 32, _lib.F64)) - 1) == -2
    assert call(_opts(_lib), M=529, ldx=529, ldw=529, lda=529) == -3
    assert call(_opts(_lib), M=529, ldx=529, ldw=529, lda=529, ws=16) == -3
    assert call(_opts(_lib), R=4097, ldh=4097, ws=16) == -3
    assert call(_opts(_lib, reserved=1 << 16), R=257, ldh=257) == -3      # the fused route forced where it does not hold
    assert call(_opts(_lib, reserved=1 << 16), R=256, ldh=256, ws=16) == -2
    assert call(_opts(_lib, beta=float("nan")), M=529, ldx=529, ldw=529, lda=529) == -1        # -1 before -3


def test_workspace_and_splits_queries():
    _lib, L = lib()
    q = L.evc_online_workspace_bytes
    assert q(25, 16, 6880, 1024, _lib.F64) < q(25, 128, 6880, 1024, _lib.F64) < q(25, 128, 68800, 1024, _lib.F64)
    assert q(25, 16, 6880, 1024, _lib.F64) < q(25, 16, 6880, 4096, _lib.F64)        # one batch's scratch grows with it
    assert q(25, 16, 6880, 6880, _lib.F64) == q(25, 16, 6880, 1 << 30, _lib.F64)   # clipped to T
    assert q(201, 20, 688, 100, _lib.F32) < q(201, 20, 688, 100, _lib.F64)
    assert q(528, 4096, 1, 1, 0) > 0 and q(529, 1, 1, 1, 0) == 0 and q(25, 4097, 1, 1, 0) == 0
    assert q(0, 1, 1, 1, 0) == 0 and q(25, 0, 1, 1, 0) == 0 and q(25, 1, 0, 1, 0) == 0 and q(25, 1, 1, 1, 9) == 0
    assert q(25, 1, 1, 0, 0) == 0 and q(25, 1, 1, -1, 0) == 0
    for M, R, T in ((25, 17, 70), (50, 24, 150), (514, 16, 1024), (514, 16, 4096), (201, 300, 5000), (25, 24, 30)):
        assert L.evc_online_splits(M, R, T) == L.evc_beta_learn_splits(M, R, T) >= 1
    assert L.evc_online_splits(529, 1, 1) == 0 and L.evc_online_splits(25, 4097, 1) == 0
    assert L.evc_online_splits(25, 1, 0) == 0 and L.evc_online_splits(0, 1, 1) == 0


def test_fixture_table():
    names = [os.path.basename(p)[:-4] for p in FILES]
    assert len(FILES) == 18
    largest = max(os.path.getsize(p) for p in glob.glob(os.path.join(GOLDEN, "*.npz")) if p not in FILES)
    shapes, betas, stops = set(), set(), {"tol": 0, "mni": 0, "none": 0}
    for p in FILES:
        d = np.load(p)
        assert os.path.getsize(p) <= min(1 << 20, largest)
        assert set(d.files) == KEYS
        M, T = d["X"].shape
        shapes.add((M, d["W0"].shape[1], T, int(d["batch_size"])))
        betas.add(float(d["beta"]))
        assert d["W"].dtype == d["H"].dtype == d["X"].dtype == np.dtype(str(d["dtype"]))
        n, per_pass = int(d["n_steps"]), -(-T // min(int(d["batch_size"]), T))
        assert d["cost"].shape == d["change"].shape == (n,) and int(d["n_iter"]) == -(-n // per_pass)
        full = n == int(d["max_iter"]) * per_pass
        tol, mni = float(d["tol"]), int(d["max_no_improvement"])
        assert full == (tol == 0 and mni < 0)
        stops["none" if full else "tol" if d["change"][-1] <= tol else "mni"] += 1
        if tol > 0:         # every decision on the change of W is clear of its threshold
            assert (d["change"][1:-1] > tol * (1 + 1e-6)).all() and d["change"][-1] < tol * (1 - 1e-6)
        if not full:
            assert float(d["margin"]) >= (1e-6 if d["X"].dtype == np.float64 else 1e-2)
            assert n <= 30
        for F in (d["W"], d["H"]):
            pos = F[F > 0].astype(np.float64)
            assert not np.any((pos > E64 * (1 - 1e-3)) & (pos < E64 * (1 + 1e-3)))
        if "_flush_" in p:
            assert ((d["W0"] == 1e-19).sum() >= 10) and ((d["H0"] == 1e-19).sum() >= 10)
            assert (d["W"] == 0).sum() >= 10 or (d["H"] == 0).sum() >= 10
    assert {(25, 24, 300, 100), (25, 24, 330, 100), (40, 40, 330, 128), (201, 32, 200, 1024), (33, 272, 300, 96)} == shapes
    assert betas == {2.0, 1.0, 0.0, 0.5, 1.5, 3.0}
    assert stops["tol"] == 2 and stops["mni"] == 6 and stops["none"] == 10
    assert sum("_f32_" in n for n in names) == 2 and sum("_flush_" in n for n in names) == 2
    assert any(float(np.load(p)["forget_factor"]) == 1.0 for p in FILES)
    assert any(float(np.load(p)["alpha"]) == 1e-3 and float(np.load(p)["l1_ratio"]) == 0.5 for p in FILES)
    # costs that are not monotone: the stop by lack of improvement has something to see
    d = np.load(os.path.join(GOLDEN, "online_sk_m25_r24_t300_bs100_mni_b3.npz"))
    assert (np.diff(d["cost"]) > 0).any() and (np.diff(d["cost"]) < 0).any() and int(d["n_steps"]) == 22


def close_factor(got, ref, rtol=1e-9):
    """non-zero entries within rtol, zeros exact (test_beta_learn_host.close_factor)"""
    assert np.array_equal(got == 0, ref == 0)
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=0)


def _kernel_splits(M, R):
    _, L = lib()
    return lambda Tb: int(L.evc_online_splits(M, R, Tb))


@pytest.mark.parametrize("path", FILES, ids=os.path.basename)
def test_restatement_reproduces_sklearn_fixture(path):
    """float64 at S = 1: test_beta_learn_host's tolerance (rtol 1e-9, zeros exact, counts equal)"""
    d = np.load(path)
    dt = np.dtype(str(d["dtype"]))
    kw = options(d)
    args = (d["X"], d["W0"], d["H0"], kw.pop("beta"), kw.pop("batch_size"), kw.pop("max_iter"))
    W, H, n_iter, n_steps, cost, change, _ = onr.learn(*args, S=1, dtype=dt, **kw)
    assert W.dtype == H.dtype == dt
    assert (n_iter, n_steps) == (int(d["n_iter"]), int(d["n_steps"]))
    assert np.isnan(cost[n_steps:]).all() and np.isnan(change[n_steps:]).all()
    if dt == np.float64:
        close_factor(W, d["W"])
        close_factor(H, d["H"])
        np.testing.assert_allclose(cost[:n_steps], d["cost"], rtol=1e-9, atol=0)
        np.testing.assert_allclose(change[:n_steps], d["change"], rtol=1e-9, atol=1e-12)
    else:
        for got, ref in ((W, d["W"]), (H, d["H"])):
            assert np.linalg.norm(got.astype(np.float64) - ref) / np.linalg.norm(ref) <= 1e-4
        np.testing.assert_allclose(cost[:n_steps], d["cost"], rtol=1e-4, atol=0)
        np.testing.assert_allclose(change[:n_steps], d["change"], rtol=1e-3, atol=1e-6)


@pytest.mark.parametrize("path", FILES, ids=os.path.basename)
def test_restatement_with_the_kernels_frame_ranges_stays_within_a_quarter_of_the_gpu_bound(path):
    """the restatement the GPU tests compare against (the kernels' split counts; forced 3 and 7 ranges; the fixture's own
    element type) against the recorded results: measured, printed, and held to a quarter of the GPU bound (1e-9 / 1e-4)"""
    d = np.load(path)
    dt = np.dtype(str(d["dtype"]))
    M, R = d["W0"].shape
    quarter = 2.5e-10 if dt == np.float64 else 2.5e-5
    for S in (_kernel_splits(M, R), 3, 7):
        kw = options(d)
        args = (d["X"], d["W0"], d["H0"], kw.pop("beta"), kw.pop("batch_size"), kw.pop("max_iter"))
        W, H, n_iter, n_steps, cost, change, _ = onr.learn(*args, S=S, dtype=dt, **kw)
        assert (n_iter, n_steps) == (int(d["n_iter"]), int(d["n_steps"]))
        worst = 0.0
        for got, ref in ((W, d["W"]), (H, d["H"])):
            assert np.array_equal(got == 0, ref == 0)
            if dt == np.float64:
                nz = ref != 0
                worst = max(worst, float(np.max(np.abs(got[nz] - ref[nz]) / np.abs(ref[nz]))))
            else:
                worst = max(worst, float(np.linalg.norm(got.astype(np.float64) - ref) / np.linalg.norm(ref)))
        print(os.path.basename(path), "S", S if isinstance(S, int) else "kernel", "worst error %.3e" % worst)
        assert worst <= quarter


def test_restatement_resume_is_bitwise():
    d = np.load(os.path.join(GOLDEN, "online_sk_m25_r24_t330_bs100_k3_b1p5.npz"))
    run = lambda W, H, K, state=None: onr.learn(d["X"], W, H, 1.5, 100, K, 0.7, state=state)
    W5, H5, _, n5, _, _, (A5, B5) = run(d["W0"], d["H0"], 5)
    W2, H2, _, _, _, _, st = run(d["W0"], d["H0"], 2)
    W3, H3, _, n3, _, _, (A3, B3) = run(W2, H2, 3, st)
    assert n5 == 20 and n3 == 12
    for a, b in ((W3, W5), (H3, H5), (A3, A5), (B3, B5)):
        assert np.array_equal(a, b)


def test_generator_reproduces_the_fixtures():
    pytest.importorskip("sklearn")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_golden_online as g
    specs = g.cases()
    assert sorted(specs) == sorted(os.path.basename(p)[:-4] for p in FILES)
    for name in ("online_sk_m25_r24_t300_bs100_mni_b0", "online_sk_m25_r24_t300_bs100_tol_b0p5",
                 "online_sk_m25_r24_t300_bs100_k3_flush_b1"):
        out = g.make(name, specs[name])
        ref = np.load(os.path.join(GOLDEN, name + ".npz"))
        assert set(out) == set(ref.files)
        for k, v in out.items():
            v = np.asarray(v)
            assert np.asarray(ref[k]).dtype == v.dtype and np.asarray(ref[k]).tobytes() == v.tobytes(), (name, k)


# ---- the host pieces of the driver (csrc/evc_online_plan.h) in a program of their own, plainly and under the sanitizers ----
SRC = os.path.join(ROOT, "tests", "online_host_main.hip")
PKG = os.path.join(ROOT, "exemplars_vc_amd")
RULES = ((0.0, 1), (0.0, 2), (0.0, 4), (0.02, -1), (0.005, 3), (0.0, -1))


def _replay_cases():
    """(name, tol, max_no_improvement, T, frames, cost, change) over every fixture's recorded traces: the rules the fixture was
    recorded with, and a few others applied to the same figures"""
    out = []
    for p in FILES:
        d = np.load(p)
        T = d["X"].shape[1]
        bs = min(int(d["batch_size"]), T)
        per_pass = -(-T // bs)
        frames = [min(bs, T - (k % per_pass) * bs) for k in range(int(d["n_steps"]))]
        own = (float(d["tol"]), int(d["max_no_improvement"]))
        for i, (tol, mni) in enumerate((own,) + RULES):
            out.append((f"{os.path.basename(p)[:-4]}#{i}", tol, mni, T, frames, d["cost"], d["change"]))
    return out


def _program_lines(tmp, sanitize):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = os.path.join(tmp, "online_host_main" + ("_san" if sanitize else ""))
    cmd = [hipcc, "--offload-host-only", "-O1", "-std=c++17", SRC, "-o", exe, "-L" + PKG, "-levc_hip", "-Wl,-rpath," + PKG]
    if sanitize:
        cmd[1:1] = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-g"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    traces = os.path.join(tmp, "traces.txt")
    with open(traces, "w") as f:
        for name, tol, mni, T, frames, cost, change in _replay_cases():
            f.write(f"{name} {tol!r} {mni} {T} {len(frames)}\n")
            for fr, c, ch in zip(frames, cost, change):
                f.write(f"{fr} {float(c)!r} {float(ch)!r}\n")
    p = subprocess.run([exe, traces], capture_output=True, text=True)
    assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr)
    return p.stdout.split("\n")[:-1]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("online_host"))
    return _program_lines(tmp, False), tmp


def test_host_stop_rule_replays_every_recorded_trace(program):
    lines = [ln.split() for ln in program[0] if ln.startswith("stop ")]
    cases = _replay_cases()
    assert len(lines) == len(cases) == 18 * 7
    stopped = 0
    for (_, name, at), (cname, tol, mni, T, frames, cost, change) in zip(lines, cases):
        assert name == cname
        rule = onr.Stop(T, tol, None if mni < 0 else mni)
        want = next((k for k in range(1, len(frames) + 1) if rule.step(k, frames[k - 1], float(cost[k - 1]),
                                                                         float(change[k - 1]))), 0)
        assert int(at) == want, name
        if name.endswith("#0"):     # the fixture's own rules: the run ended where scikit-learn's did
            d = np.load(os.path.join(GOLDEN, name[:-2] + ".npz"))
            T_, bs = d["X"].shape[1], min(int(d["batch_size"]), d["X"].shape[1])
            full = int(d["n_steps"]) == int(d["max_iter"]) * -(-T_ // bs)
            assert int(at) == (0 if full else int(d["n_steps"])), name
        stopped += int(at) > 0
    assert stopped >= 40


def test_host_carving_and_argument_checks(program):
    _lib, L = lib()
    carves = [ln.split() for ln in program[0] if ln.startswith("carve ")]
    assert len(carves) == 14 and not any("BAD" in ln for ln in program[0])
    for c in carves:
        M, R, T, bs, esize, shift = int(c[1]), int(c[2]), int(c[3]), int(c[4]), int(c[5]), int(c[7])
        offs = [int(v) for v in c[9:18]]
        assert offs[0] == (256 - shift) % 256 and offs == sorted(offs)
        query = int(L.evc_online_workspace_bytes(M, R, T, bs, _lib.F64 if esize == 8 else _lib.F32))
        assert int(c[-1]) == query and int(c[-3]) <= query
    args = {ln.split()[1]: ln.split()[2:] for ln in program[0] if ln.startswith("args ")}
    want = dict(ok=0, ok_exact=0, short_by_one=-2, no_acc=-1, struct_bytes=-1, batch_size=-1, max_iter=-1, too_many_steps=-1,
                forget_0=-1, forget_1=0, forget_nan=-1, beta_inf=-1, l1_w=-1, resume=-1, forced_7_unfused=0, fused_257=-3,
                fused_256=0, R_65=0, M_529=-3, R_4097=-3, nan_before_limits=-1)
    assert {k: int(v[0]) for k, v in args.items()} == want
    assert args["ok"][1:] == ["forced", "0", "fused", "1"] and args["R_65"][1:] == ["forced", "0", "fused", "0"]
    assert args["forced_7_unfused"][1:] == ["forced", "7", "fused", "0"] and args["fused_256"][1:] == ["forced", "0", "fused", "1"]


def test_the_host_program_runs_clean_under_the_sanitizers(program):
    """a stand-alone program: address + undefined-behaviour sanitizers on the host code, nothing preloaded anywhere"""
    assert _program_lines(program[1], True) == program[0]


def _small():
    rng = np.random.default_rng(0)
    return rng.random((6, 4)) + 0.1, rng.random((5, 4)) + 0.1, rng.random((6, 5)) + 0.1      # X, dictionary, activations


def _runs_or_refuses(fn):
    """with a device the call answers; without one it refuses (there is no CPU fallback)"""
    import torch
    if torch.cuda.is_available():
        return fn()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fn()


def test_python_surface():
    import exemplars_vc_amd as evc
    from exemplars_vc_amd.compat import factorize as fz
    X, D, W0 = _small()
    assert "learn_dictionary_online" in evc.__all__
    sig = inspect.signature(evc.learn_dictionary_online).parameters
    assert list(sig)[:3] == ["X", "W0", "H0"]
    want = dict(beta=2.0, batch_size=1024, max_iter=200, forget_factor=0.7, tol=1e-4, max_no_improvement=10, l1_h=0.0,
                l2_h=0.0, l1_w=0.0, l2_w=0.0, state=None, dtype=None, device=None, info=False, route=None, splits=None)
    for k, v in want.items():
        assert sig[k].default == v and sig[k].kind is inspect.Parameter.KEYWORD_ONLY, k
    assert sig["layout"].default is inspect.Parameter.empty
    cd = inspect.signature(evc.compact_dictionary).parameters
    assert cd["batch_size"].default is None and cd["forget_factor"].default == 0.7
    mb = inspect.signature(fz.non_negative_factorization_minibatch).parameters
    assert list(mb)[:3] == ["X", "W", "H"]
    assert {k: mb[k].default for k in list(mb)[3:]} == dict(
        beta_loss="frobenius", batch_size=1024, max_iter=200, tol=1e-4, max_no_improvement=10, forget_factor=0.7,
        alpha_W=0.0, alpha_H="same", l1_ratio=0.0, device=None)
    for loss in ("itakura-saito", 0, 0.5, 1, "frobenius", np.float64(3.0)):
        _runs_or_refuses(lambda: fz.non_negative_factorization_minibatch(X, W0, D, beta_loss=loss, batch_size=4, max_iter=2))
    _runs_or_refuses(lambda: evc.learn_dictionary_online(X, D, W0, layout="frame_major", batch_size=4, max_iter=2))
    _runs_or_refuses(lambda: evc.compact_dictionary(X[:3], X[3:], 2, iters=2, batch_size=2))


def test_python_surface_refusals():
    import exemplars_vc_amd as evc
    from exemplars_vc_amd.compat import factorize as fz
    X, D, W0 = _small()
    Xz = X.copy()
    Xz[2, 1] = 0.0
    for loss in ("itakura-saito", 0, -0.5):                  # scikit-learn's refusal, before anything runs
        with pytest.raises(ValueError, match=ZERO_MSG):
            fz.non_negative_factorization_minibatch(Xz, W0, D, beta_loss=loss)
    for loss in ("bogus", float("nan"), True, None):
        with pytest.raises(ValueError, match="Invalid beta_loss parameter"):
            fz.non_negative_factorization_minibatch(X, W0, D, beta_loss=loss)
    with pytest.raises(ValueError, match="528"):
        evc.learn_dictionary_online(np.ones((3, 529)), np.ones((2, 529)), np.ones((3, 2)), layout="frame_major")
    with pytest.raises(ValueError, match="528"):
        evc.learn_dictionary_online(np.ones((529, 3)), np.ones((529, 2)), np.ones((2, 3)), layout="bin_major")
    with pytest.raises(ValueError, match="finite"):
        evc.learn_dictionary_online(X, D, W0, beta=float("nan"), layout="frame_major")
    with pytest.raises(ValueError, match="route"):
        evc.learn_dictionary_online(X, D, W0, layout="frame_major", route="both")
    with pytest.raises(ValueError, match="batch_size"):
        evc.learn_dictionary_online(X, D, W0, layout="frame_major", batch_size=0)
    for ff in (0.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="forget_factor"):
            evc.learn_dictionary_online(X, D, W0, layout="frame_major", forget_factor=ff)
    for kw in (dict(loss="kl"), dict(solver="cd")):
        with pytest.raises(ValueError, match="batch_size selects the online learner"):
            evc.compact_dictionary(X[:3], X[3:], 2, batch_size=2, **kw)
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            evc.learn_dictionary_online(X, D, W0, layout="frame_major", max_iter=1)
