"""Sparse dictionary learning (evc_prox_learn), host side: the C ABI's declarations and struct mirror, the statuses through the
library, the numpy restatement against every recorded deComP run, the shuffle rule, the Python surfaces' refusals and the
stand-alone host program (csrc/evc_prox_learn_plan.h), plainly and under the sanitizers.  No GPU needed."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prox_learn_restatement as plr  # noqa: E402
import prox_restatement as pr  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ["proxl_m5_n3_t101_fista", "proxl_m25_n40_t130_fista_pos_k4", "proxl_m40_n70_t200_ista_pos_k3",
            "proxl_m201_n96_t150_fista_pos_k3", "proxl_m1_n5_t12_fista_pos", "proxl_m25_n40_t130_fista_pos_stop",
            "proxl_m8_n6_t40_unused_atom", "proxl_m12_n10_t64_inside"]
EPS = float(np.finfo(np.float64).eps)


def lib():
    from exemplars_vc_amd import _lib
    return _lib, _lib.lib()


def load(name):
    d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    d["y"], d["D0"] = d["y"].astype(np.float64), d["D0"].astype(np.float64)
    d["positive"], d["momentum"] = pr.split_method(str(d["method"]))
    return d


def restate(d, order, **kw):
    return plr.solve(d["y"], d["D0"], float(d["alpha"]), d.get("x0"), batch_size=int(d["bs"]), epochs=int(d["maxiter"]) - 1,
                     order=order, tol=float(d["tol"]), positive=d["positive"], momentum=d["momentum"], **kw)


# ---- the C ABI's face ----
def test_symbols_declared_and_exported():
    _lib, L = lib()
    hdr = open(os.path.join(ROOT, "include", "evc.h")).read()
    declared = set(re.findall(r"\b(evc_[a-z_0-9]+)\s*\(", hdr))
    for sym in ("evc_prox_learn_workspace_bytes", "evc_prox_learn_block", "evc_prox_learn"):
        assert sym in declared and sym in _lib.SYMBOLS and hasattr(L, sym)
    assert "evc_prox_learn " in hdr[:hdr.index("#ifndef EVC_H")]
    assert (_lib.PROX_LEARN_MAX_M, _lib.PROX_LEARN_MAX_N) == (1056, 4096)


def test_opts_mirror_matches_header():
    _lib, _ = lib()
    hdr = open(os.path.join(ROOT, "include", "evc.h")).read()
    body = hdr[hdr.index("typedef struct evc_prox_learn_opts {"):hdr.index("} evc_prox_learn_opts;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for grp in re.findall(r"\b(?:int|double|void\*)\s+([a-zA-Z_0-9, ]+);", body) for n in grp.replace(" ", "").split(",")]
    assert names == [f[0] for f in _lib.ProxLearnOpts._fields_]
    assert names == ["struct_bytes", "dtype", "layout", "batch_size", "epochs", "lasso_iters", "lasso_check_every", "mode",
                     "momentum", "resume", "reserved", "reserved2", "alpha", "tol", "lasso_tol", "ev_loop_start", "ev_loop_stop"]
    assert C.sizeof(_lib.ProxLearnOpts) == 12 * 4 + 3 * 8 + 2 * 8
    assert C.sizeof(_lib.ProxOpts) == 12 * 4 + 4 * 8 + 2 * 8                        # the existing struct did not move


def test_statuses_through_the_library():
    """the same checks as the host program's, through the shared library: before any device work, in the statuses' order"""
    _lib, L = lib()
    one = C.c_void_p(8)              # never dereferenced: every case fails validation first
    count = C.c_longlong(0)

    def opts(**kw):
        o = _lib.ProxLearnOpts()
        o.struct_bytes = C.sizeof(o)
        o.dtype, o.layout, o.batch_size, o.epochs = _lib.F64, _lib.FRAME_MAJOR, 32, 3
        o.lasso_iters, o.lasso_check_every, o.mode, o.momentum = 10, 10, _lib.PROX_POSITIVE, _lib.PROX_FISTA
        o.alpha, o.lasso_tol = 1e-3, 1e-5
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def call(o, M=25, N=17, T=70, ldx=25, ldd=25, ldh=17, lds=42, ws=16, X=one, D=one, H=one, stats=one, cnt=count, order=None,
             wsp=one):
        return L.evc_prox_learn(X, ldx, D, ldd, H, ldh, stats, lds, None if cnt is None else C.byref(cnt), order, M, N, T,
                                None if o is None else C.byref(o), wsp, ws, None, None, None, None)
    assert call(opts()) == -2 and call(None) == -1 and call(opts(struct_bytes=8)) == -1
    for p in ("X", "D", "H", "stats", "cnt", "wsp"):
        assert call(opts(), **{p: None}) == -1
    assert call(opts(), ldx=24) == -1 and call(opts(), ldd=24) == -1 and call(opts(), ldh=16) == -1 and call(opts(), lds=41) == -1
    assert call(opts(layout=_lib.BIN_MAJOR), ldx=70, ldd=17, ldh=70) == -2
    assert call(opts(layout=_lib.BIN_MAJOR), ldx=69, ldd=17, ldh=70) == -1
    assert call(opts(batch_size=0)) == -1 and call(opts(batch_size=71)) == -1 and call(opts(batch_size=70)) == -2
    assert call(opts(epochs=-1)) == -1 and call(opts(epochs=0)) == -2 and call(opts(resume=2)) == -1
    assert call(opts(reserved=8)) == -1 and call(opts(reserved=7)) == -2 and call(opts(reserved2=1)) == -1 and call(opts(mode=2)) == -1
    assert call(opts(momentum=3)) == -1 and call(opts(alpha=float("nan"))) == -1 and call(opts(tol=-1.0)) == -1
    assert call(opts(lasso_tol=float("inf"))) == -1 and call(opts(lasso_iters=-1)) == -1
    assert call(opts(), M=1057, ldx=1057, ldd=1057, lds=1057 + 17) == -3 and call(opts(), N=4097, ldh=4097, lds=4097 + 25) == -3
    assert call(opts(alpha=-1.0), N=4097, ldh=4097, lds=4097 + 25) == -1
    good = (C.c_int * 140)(*(list(range(69, -1, -1)) + list(range(70))))
    bad = (C.c_int * 140)(*(list(range(70)) + [0] + list(range(69))))
    assert call(opts(epochs=2), order=good) == -2 and call(opts(epochs=2), order=bad) == -1
    assert call(opts(epochs=1), order=bad) == -2                       # only the rows of the call's epochs are looked at
    assert call(opts(), ws=int(L.evc_prox_learn_workspace_bytes(25, 17, 70, 32, _lib.F64)) - 1) == -2


def test_workspace_and_block_queries():
    _lib, L = lib()
    q, blk = L.evc_prox_learn_workspace_bytes, L.evc_prox_learn_block
    assert q(1057, 64, 100, 10, 0) == 0 and q(25, 4097, 100, 10, 0) == 0 and q(0, 64, 100, 10, 0) == 0
    assert q(25, 64, 0, 1, 0) == 0 and q(25, 64, 100, 0, 0) == 0 and q(25, 64, 100, 101, 0) == 0 and q(25, 64, 100, 10, 9) == 0
    assert q(1056, 4096, 100, 100, 0) > 0 and q(25, 64, 100, 100, 1) > 0
    assert q(25, 64, 688, 64, _lib.F32) < q(25, 64, 688, 64, _lib.F64) < q(25, 64, 688, 128, _lib.F64)
    for M, N, T, bs, dt, es in ((25, 64, 130, 32, _lib.F64, 8), (402, 1024, 2048, 1024, _lib.F32, 4)):
        own = ((N + M) * bs + 2 * N * M) * es + T * 4 + int(L.evc_prox_workspace_bytes(M, N, bs, 1, dt))
        assert own <= int(q(M, N, T, bs, dt)) <= own + N * 8 + 10 * 256
    assert blk(0, 0) == 0 and blk(1057, 0) == 0 and blk(25, 2) == 0
    for M in (1, 25, 160, 161, 201, 320, 321, 640, 641, 1056):
        for dt, npdt in ((_lib.F64, np.float64), (_lib.F32, np.float32)):
            assert blk(M, dt) == plr.plearn_block(M, npdt)
    assert [blk(M, _lib.F64) for M in (160, 161, 320, 321, 640, 641)] == [32, 16, 16, 8, 8, 4]
    assert [blk(M, _lib.F32) for M in (320, 321, 640, 641, 1056)] == [32, 16, 16, 8, 8]


# ---- the restatement against every recorded deComP run ----
@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_reproduces_decomp(name):
    """deComP's left-looking loop against the blocked, right-looking restatement with the frame orders of the shuffle rule:
    the same `it`, D and x to 100 eps steps (measured where the fixtures were recorded: 2.2e-16 .. 2.4e-14)"""
    d = load(name)
    epochs = int(d["maxiter"]) - 1
    order = plr.decomp_order(d["y"].shape[0], epochs, int(d["seed"]))
    D, x, n_epochs, n_steps, trace, (S, Q, count) = restate(d, order)
    stopped = n_steps > 0 and trace[n_steps - 1] < float(d["tol"])
    assert (n_epochs if stopped else int(d["maxiter"])) == int(d["it"]) and n_steps == int(d["n_steps"]) == count
    bound = 100 * EPS * n_steps
    worst_d, worst_x = float(np.max(np.abs(D - d["D"]))), float(np.max(np.abs(x - d["x"])) / np.max(np.abs(d["x"])))
    print("%s: D %.2e, x %.2e (allowed %.2e)" % (name, worst_d, worst_x, bound))
    assert worst_d <= bound and worst_x <= bound
    np.testing.assert_allclose(trace[:n_steps], d["trace"], rtol=0, atol=2 * bound)
    assert np.all(np.isnan(trace[n_steps:])) and np.all(np.linalg.norm(D, axis=1) <= 1 + 4 * EPS)
    if float(d["tol"]) > 0:                                         # no stop decision sits on its threshold
        assert np.min(np.abs(d["trace"] - float(d["tol"]))) > 1000 * float(d["perm64"])


def test_fixture_set_is_what_the_tests_need():
    kinds = {name: load(name) for name in FIXTURES}
    for name, d in kinds.items():
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 512 * 1024
        assert 0 <= float(d["perm64"]) < 1e-12 and 0 <= float(d["perm32"]) < 1e-3 and float(d["d32"]) < 100 * max(
            float(d["perm32"]), 1e-7)
    shapes = {name: d["y"].shape + d["D0"].shape[:1] + (int(d["bs"]),) for name, d in kinds.items()}
    assert shapes["proxl_m5_n3_t101_fista"] == (101, 5, 3, 100) and shapes["proxl_m1_n5_t12_fista_pos"] == (12, 1, 5, 4)
    assert all(T % bs for T, _, _, bs in list(shapes.values())[:4])                  # frames are left alone every epoch
    stops = {n: int(d["n_steps"]) for n, d in kinds.items() if float(d["tol"]) > 0}
    assert stops["proxl_m1_n5_t12_fista_pos"] == 1 and 10 < stops["proxl_m5_n3_t101_fista"] < 999
    assert stops["proxl_m25_n40_t130_fista_pos_stop"] > 50
    assert sum(1 for d in kinds.values() if int(d["maxiter"]) - 1 >= 3 and float(d["tol"]) == 0) >= 1   # the shuffle rule, 3 epochs
    signed = kinds["proxl_m5_n3_t101_fista"]
    assert not signed["positive"] and (signed["x"] < 0).any()
    unused = kinds["proxl_m8_n6_t40_unused_atom"]
    assert np.all(unused["x0"] == 0) and np.all(unused["x"][:, -1] == 0) and np.array_equal(unused["D"][-1], unused["D0"][-1])
    assert float(kinds["proxl_m12_n10_t64_inside"]["min_norm"]) < 1 - 1e-6           # the projection's other branch
    assert sum(1 for d in kinds.values() if float(d["min_norm"]) > 1 - 1e-9) >= 5


def test_the_shuffle_rule_and_a_wrong_one():
    """three epochs: the rule's rows reproduce deComP's run; rows shuffled afresh every epoch (not cumulatively) do not"""
    from exemplars_vc_amd.solver import decomp_frame_order
    d = load("proxl_m25_n40_t130_fista_pos_k4")
    T, seed = d["y"].shape[0], int(d["seed"])
    order = decomp_frame_order(T, 3, seed)
    assert order.dtype == np.int32 and order.shape == (3, T) and np.array_equal(order, plr.decomp_order(T, 3, seed))
    assert np.array_equal(np.sort(order, axis=1), np.tile(np.arange(T), (3, 1)))
    D = restate(d, order)[0]
    assert np.max(np.abs(D - d["D"])) <= 100 * EPS * 12
    rng = np.random.RandomState(seed)
    fresh = np.stack([rng.permutation(T) for _ in range(3)])
    assert np.max(np.abs(restate(d, fresh)[0] - d["D"])) > 1e-6
    assert np.array_equal(order[0], fresh[0]) and not np.array_equal(order[1], fresh[1])
    assert decomp_frame_order(7, 0, 1).shape == (0, 7)


def test_restatement_options():
    y, D0 = plr.problem(25, 40, 70, 3)
    order = plr.decomp_order(70, 3, 5)
    kw = dict(batch_size=32, order=order)
    whole = plr.solve(y, D0, 1e-3, epochs=3, **kw)
    first = plr.solve(y, D0, 1e-3, epochs=2, **kw)
    second = plr.solve(y, first[0], 1e-3, first[1], batch_size=32, epochs=1, order=order[2:], state=first[5])
    assert np.array_equal(second[0], whole[0]) and np.array_equal(second[1], whole[1]) and second[5][2] == whole[5][2] == 6
    # the block width moves roundings only; a left-looking sweep (one atom per block) is deComP's own loop
    for nb in (1, 4, 64):
        other = plr.solve(y, D0, 1e-3, epochs=3, nb=nb, **kw)
        assert 0 <= np.max(np.abs(other[0] - whole[0])) <= 100 * EPS * 6
    assert plr.solve(y, D0, 1e-3, epochs=0, **kw)[3] == 0
    x32 = plr.solve(y, D0, 1e-3, epochs=1, dtype=np.float32, **kw)
    assert x32[0].dtype == np.float32 and x32[1].dtype == np.float32


# ---- the Python surfaces refuse before any device is asked for ----
def test_compat_refusals():
    from exemplars_vc_amd.compat import decomp
    dl = decomp.dictionary_learning
    y, D = np.ones((12, 4)), np.ones((3, 4))
    with pytest.raises(NotImplementedError, match="minibatch is required"):
        dl.solve(y, D, 0.1)
    with pytest.raises(NotImplementedError, match="ista, fista, ista_pos"):
        dl.solve(y, D, 0.1, minibatch=4)                           # deComP's default lasso_method='cd'
    for method in ("cd", "parallel_cd", "admm", "acc_ista", "acc_ista_pos", "cd_pos"):
        with pytest.raises(NotImplementedError):
            dl.solve(y, D, 0.1, minibatch=4, lasso_method=method)
    with pytest.raises(NotImplementedError, match="mask"):
        dl.solve(y, D, 0.1, minibatch=4, lasso_method="fista", mask=np.ones_like(y))
    with pytest.raises(NotImplementedError, match="complex"):
        dl.solve(y.astype(complex), D, 0.1, minibatch=4, lasso_method="fista")
    with pytest.raises(NotImplementedError, match="block_cd"):
        dl.solve(y, D, 0.1, minibatch=4, lasso_method="fista", method="parallel_cd")
    with pytest.raises(ValueError, match="Minibatch size"):
        dl.solve(y, D, 0.1, minibatch=13, lasso_method="fista")
    with pytest.raises(ValueError, match="channels"):
        dl.solve(y, np.ones((3, 5)), 0.1, minibatch=4, lasso_method="fista")
    assert "dictionary_learning" in decomp.__doc__


def test_solver_refusals():
    import exemplars_vc_amd as evc
    X, D0 = np.ones((4, 12)), np.ones((4, 3))
    kw = dict(alpha=0.1, layout="bin_major", batch_size=4, epochs=1)
    for bad in (dict(batch_size=0), dict(batch_size=13), dict(epochs=-1), dict(alpha=-1.0), dict(tol=float("nan")),
                dict(momentum="cd"), dict(lasso_iters=-1), dict(order=np.zeros((1, 12), dtype=np.int32)),
                dict(order=np.arange(12)[None].repeat(2, 0))):
        with pytest.raises(ValueError):
            evc.learn_dictionary_sparse(X, D0, **dict(kw, **bad))
    assert "learn_dictionary_sparse" in evc.__all__ and "compact_dictionary_sparse" in evc.__all__


# ---- the host pieces of the driver (csrc/evc_prox_learn_plan.h) in a program of their own, plainly and under the sanitizers ----
SRC = os.path.join(ROOT, "tests", "prox_learn_host_main.hip")
PKG = os.path.join(ROOT, "exemplars_vc_amd")


def _program_lines(tmp, sanitize):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = os.path.join(tmp, "prox_learn_host_main" + ("_san" if sanitize else ""))
    cmd = [hipcc, "--offload-host-only", "-O1", "-std=c++17", SRC, "-o", exe, "-L" + PKG, "-levc_hip", "-Wl,-rpath," + PKG]
    if sanitize:
        cmd[1:1] = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-g"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr)
    return p.stdout.split("\n")[:-1]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("prox_learn_host"))
    return _program_lines(tmp, False), tmp


def test_host_carving_and_argument_checks(program):
    _lib, L = lib()
    carves = [ln.split() for ln in program[0] if ln.startswith("carve ")]
    assert len(carves) == 24 and not any("BAD" in ln for ln in program[0])
    for c in carves:
        M, N, T, bs, esize, shift = (int(v) for v in c[1:6] + [c[7]])
        offs = [int(v) for v in c[9:16]]
        assert len(offs) == 7 and c[16] == "bytes"
        assert offs[0] == (256 - shift) % 256 and offs == sorted(offs) and all((o + shift) % 256 == 0 for o in offs)
        query = int(L.evc_prox_learn_workspace_bytes(M, N, T, bs, _lib.F64 if esize == 8 else _lib.F32))
        assert int(c[-1]) == query and int(c[-3]) <= query <= int(c[-3]) + 512
    args = {ln.split()[1]: int(ln.split()[2]) for ln in program[0] if ln.startswith("args ")}
    want = dict(ok=0, ok_exact=0, short_by_one=-2, no_opts=-1, no_x=-1, struct_bytes=-1, dtype=-1, layout=-1, batch_0=-1,
                batch_T=0, batch_T_plus_1=-1, epochs_neg=-1, epochs_0=0, steps_beyond_int=-1, lasso_iters_neg=-1,
                lasso_iters_0=0, slots_4098=-1, slots_4097=0, check_every_neg=-1, mode=-1, mode_signed=0, momentum=-1,
                momentum_nesterov=0, resume_2=-1, resume_1=0, resume_count_neg=-1, fresh_count_neg=0, reserved=-1, reserved_halves_off=0,
                reserved2=-1, alpha_neg=-1, alpha_nan=-1, alpha_0=0, tol_neg=-1, tol_inf=-1, tol_set=0, lasso_tol_nan=-1,
                lasso_tol_0=0, ldx_short=-1, ldd_short=-1, ldh_short=-1, ld_stats_short=-1, padded=0, bin_major=0,
                bin_major_ldx_short=-1, bin_major_ldd_short=-1, M_0=-1, T_0=-1, M_1056=0, M_1057=-3, M_1057_small_ws=-3,
                N_4096=0, N_4096_small_ws=-2, N_4097=-3, nan_before_limits=-1)
    assert args == want
    blocks = [tuple(int(v) for v in ln.split()[1:]) for ln in program[0] if ln.startswith("block ")]
    assert len(blocks) == 22
    for M, es, nb, lds in blocks:
        assert nb == plr.plearn_block(M, np.float64 if es == 8 else np.float32) and nb in (4, 8, 16, 32)
        assert lds <= 64 * 1024 - 256 and (nb == 32 or 2 * nb * M * es > plr.LDS_BYTES)      # the widest block that fits
    betas = {(int(ln.split()[1]), int(ln.split()[2])): float(ln.split()[3]) for ln in program[0] if ln.startswith("beta ")}
    assert len(betas) == 15
    for (count, bs), beta in betas.items():
        theta = count * float(bs) + 1.0
        assert beta == (theta - bs) / theta
    assert betas[(0, 32)] == -31.0 and betas[(0, 1)] == 0.0 and 0 < betas[(217, 32)] < 1
    orders = {ln.split()[1]: int(ln.split()[2]) for ln in program[0] if ln.startswith("order ")}
    assert orders == dict(null=0, good=0, twice_in_second_row=-1, first_row_only=0, beyond=-1, negative=-1, no_epochs=0,
                          args_good=-2, args_twice=-1)


def test_the_epoch_loop_with_fake_callables(program):
    """plearn_loop (csrc/evc_prox_learn_plan.h), driven without a device: epochs x batches of 8 frames (the last case: 32),
    the k-th statistic read is 1 + 1 / k, or 0 where the case says so"""
    nan = float("nan")
    loops = {}
    for ln in program[0]:
        if ln.startswith("loop "):
            w = ln.split()
            cut = {k: w.index(k) for k in ("staged", "reads", "t0", "trace")}
            loops[w[1]] = dict(n_epochs=int(w[3]), n_steps=int(w[5]), count=int(w[7]),
                               staged=[int(v) for v in w[cut["staged"] + 1:cut["reads"]]], reads=int(w[cut["reads"] + 1]),
                               t0=[int(v) for v in w[cut["t0"] + 1:cut["trace"]]], trace=[float(v) for v in w[cut["trace"] + 1:]])
    stat = lambda k: 1.0 + 1.0 / k       # noqa: E731
    want = {
        # 4 epochs of 3 steps, tol 0.5, the 5th statistic is 0: the stop at step 1 of epoch 1, NaN after it
        "stop_at_step_2_of_epoch_1": dict(n_epochs=2, n_steps=5, count=5, staged=[0, 1], reads=5, t0=[0, 8, 16, 0, 8],
                                          trace=[stat(1), stat(2), stat(3), stat(4), 0.0] + [nan] * 7),
        # tol = 0 never stops, not even on a statistic of 0; no order: nothing staged
        "tol_0_with_a_trace": dict(n_epochs=2, n_steps=4, count=4, staged=[], reads=4, t0=[0, 8, 0, 8],
                                   trace=[stat(1), stat(2), 0.0, stat(4)]),
        # nobody reads the statistic: read_stat, the only synchronisation of a step, is never called
        "no_trace_no_tol": dict(n_epochs=2, n_steps=6, count=6, staged=[0, 1], reads=0, t0=[0, 8, 16] * 2, trace=[]),
        "tol_without_a_trace": dict(n_epochs=1, n_steps=2, count=2, staged=[], reads=2, t0=[0, 8], trace=[]),
        # a step that leaves no statistic (measurement only): nothing is read whatever tol and the trace ask for
        "no_statistic": dict(n_epochs=2, n_steps=4, count=4, staged=[0, 1], reads=0, t0=[0, 8, 0, 8], trace=[nan] * 4),
        "epochs_0": dict(n_epochs=0, n_steps=0, count=4, staged=[], reads=0, t0=[], trace=[]),
        "nbat_0": dict(n_epochs=3, n_steps=0, count=4, staged=[], reads=0, t0=[], trace=[]),
        # count_io = 7 on entry: the forgetting factors of steps 7 and 8 (checked in the program), 9 on return
        "resumed_count": dict(n_epochs=1, n_steps=2, count=9, staged=[0], reads=2, t0=[0, 32], trace=[stat(1), stat(2)]),
    }
    assert sorted(loops) == sorted(want)
    for name, w in want.items():
        got = loops[name]
        assert np.array_equal(got.pop("trace"), w.pop("trace"), equal_nan=True) and got == w, name


def test_the_host_program_runs_clean_under_the_sanitizers(program):
    """a stand-alone program: address + undefined-behaviour sanitizers on the host code, nothing preloaded anywhere"""
    assert _program_lines(program[1], True) == program[0]
