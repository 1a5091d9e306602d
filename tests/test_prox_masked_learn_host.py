"""Sparse dictionary learning with missing data (evc_prox_masked_learn), host side: the C ABI's declarations and struct mirror,
the statuses through the library, the numpy restatement against every recorded deComP run, the Python surfaces' refusals and
the stand-alone host program (csrc/evc_prox_masked_learn_plan.h), plainly and under the sanitizers.  No GPU needed."""
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
import prox_masked_learn_restatement as pmlr  # noqa: E402
import prox_restatement as pr  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ["proxml_m5_n3_t101_fista", "proxml_m25_n40_t130_fista_pos_k4", "proxml_m12_n10_t64_ista_pos", "proxml_m1_n5_t12_k4",
            "proxml_m201_n48_t100_k3", "proxml_m25_n40_t130_weights_k3", "proxml_m12_n10_t64_holes_k3",
            "proxml_m8_n6_t40_unused_atom_k3", "proxml_m12_n10_t64_ones_k3"]
EPS = float(np.finfo(np.float64).eps)


def lib():
    from exemplars_vc_amd import _lib
    return _lib, _lib.lib()


def load(name):
    d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    d["y"], d["D0"], d["mask"] = d["y"].astype(np.float64), d["D0"].astype(np.float64), d["mask"].astype(np.float64)
    d["positive"], d["momentum"] = pr.split_method(str(d["method"]))
    d["order"] = pmlr.decomp_order(d["y"].shape[0], int(d["maxiter"]) - 1, int(d["seed"]))
    return d


def restate(d, **kw):
    return pmlr.solve(d["y"], d["D0"], float(d["alpha"]), d.get("x0"), mask=d["mask"], batch_size=int(d["bs"]),
                      epochs=int(d["maxiter"]) - 1, order=d["order"], tol=float(d["tol"]), positive=d["positive"],
                      momentum=d["momentum"], **kw)


# ---- the C ABI's face ----
def test_symbols_declared_and_exported():
    _lib, L = lib()
    hdr = open(os.path.join(ROOT, "include", "evc.h")).read()
    declared = set(re.findall(r"\b(evc_[a-z_0-9]+)\s*\(", hdr))
    for sym in ("evc_prox_masked_learn_workspace_bytes", "evc_prox_masked_learn"):
        assert sym in declared and sym in _lib.SYMBOLS and hasattr(L, sym)
    assert "evc_prox_masked_learn " in hdr[:hdr.index("#ifndef EVC_H")]
    assert (_lib.PROX_MASKED_LEARN_MAX_M, _lib.PROX_MASKED_LEARN_MAX_N, _lib.PROX_MASKED_LEARN_MAX_S) == (1056, 1024, 1 << 28)


def test_opts_mirror_matches_header():
    _lib, _ = lib()
    hdr = open(os.path.join(ROOT, "include", "evc.h")).read()
    body = hdr[hdr.index("typedef struct evc_prox_masked_learn_opts {"):hdr.index("} evc_prox_masked_learn_opts;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for grp in re.findall(r"\b(?:int|double|void\*)\s+([a-zA-Z_0-9, ]+);", body) for n in grp.replace(" ", "").split(",")]
    assert names == [f[0] for f in _lib.ProxMaskedLearnOpts._fields_]
    assert names == ["struct_bytes", "dtype", "layout", "batch_size", "epochs", "lasso_iters", "lasso_check_every", "mode",
                     "momentum", "resume", "reserved", "reserved2", "alpha", "tol", "lasso_tol", "ev_loop_start", "ev_loop_stop"]
    assert C.sizeof(_lib.ProxMaskedLearnOpts) == 12 * 4 + 3 * 8 + 2 * 8
    assert C.sizeof(_lib.ProxLearnOpts) == 12 * 4 + 3 * 8 + 2 * 8                   # the existing structs did not move
    assert C.sizeof(_lib.ProxMaskedOpts) == 14 * 4 + 4 * 8 + 2 * 8


def test_statuses_through_the_library():
    """the same checks as the host program's, through the shared library: before any device work, in the statuses' order"""
    _lib, L = lib()
    one = C.c_void_p(8)              # never dereferenced: every case fails validation first
    count = C.c_longlong(0)

    def opts(**kw):
        o = _lib.ProxMaskedLearnOpts()
        o.struct_bytes = C.sizeof(o)
        o.dtype, o.layout, o.batch_size, o.epochs = _lib.F64, _lib.FRAME_MAJOR, 32, 3
        o.lasso_iters, o.lasso_check_every, o.mode, o.momentum = 10, 10, _lib.PROX_POSITIVE, _lib.PROX_FISTA
        o.alpha, o.lasso_tol = 1e-3, 1e-5
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def call(o, M=25, N=17, T=70, ldx=25, ldm=25, ldd=25, ldh=17, lds=17, ldq=25, ws=16, X=one, mask=one, D=one, H=one, S=one,
             Q=one, cnt=count, order=None, wsp=one):
        return L.evc_prox_masked_learn(X, ldx, mask, ldm, D, ldd, H, ldh, S, lds, Q, ldq, None if cnt is None else C.byref(cnt),
                                       order, M, N, T, None if o is None else C.byref(o), wsp, ws, None, None, None, None)
    assert call(opts()) == -2 and call(None) == -1 and call(opts(struct_bytes=8)) == -1
    for p in ("X", "mask", "D", "H", "S", "Q", "cnt", "wsp"):
        assert call(opts(), **{p: None}) == -1
    assert call(opts(), ldx=24) == -1 and call(opts(), ldm=24) == -1 and call(opts(), ldd=24) == -1 and call(opts(), ldh=16) == -1
    assert call(opts(), lds=16) == -1 and call(opts(), ldq=24) == -1 and call(opts(), lds=20, ldq=28) == -2
    assert call(opts(layout=_lib.BIN_MAJOR), ldx=70, ldm=70, ldd=17, ldh=70) == -2
    assert call(opts(layout=_lib.BIN_MAJOR), ldx=70, ldm=69, ldd=17, ldh=70) == -1
    assert call(opts(batch_size=0)) == -1 and call(opts(batch_size=71)) == -1 and call(opts(batch_size=70)) == -2
    assert call(opts(epochs=-1)) == -1 and call(opts(epochs=0)) == -2 and call(opts(resume=2)) == -1
    assert call(opts(reserved=8)) == -1 and call(opts(reserved=7)) == -2 and call(opts(reserved2=1)) == -1 and call(opts(mode=2)) == -1
    assert call(opts(momentum=3)) == -1 and call(opts(alpha=float("nan"))) == -1 and call(opts(tol=-1.0)) == -1
    assert call(opts(lasso_tol=float("inf"))) == -1 and call(opts(lasso_iters=-1)) == -1
    big = 1 << 40
    assert call(opts(), M=1057, ldx=1057, ldm=1057, ldd=1057, ldq=1057, ws=big) == -3
    assert call(opts(), N=1025, ldh=1025, lds=1025, ws=big) == -3
    assert call(opts(), N=1025, ldh=1025, lds=1025) == -3                        # -3 before the workspace is looked at
    assert call(opts(), N=1024, ldh=1024, lds=1024) == -2
    wide = dict(M=257, ldx=257, ldm=257, ldd=257, ldq=257, N=1024, ldh=1024, lds=1024)        # M N^2 = 2^28 + 2^20
    assert call(opts(), **wide) == -3 and call(opts(), **dict(wide, M=256)) == -2
    assert call(opts(alpha=-1.0), **wide) == -1 and call(opts(), **dict(wide, mask=None)) == -1  # -1 before -3
    good = (C.c_int * 140)(*(list(range(69, -1, -1)) + list(range(70))))
    bad = (C.c_int * 140)(*(list(range(70)) + [0] + list(range(69))))
    assert call(opts(epochs=2), order=good) == -2 and call(opts(epochs=2), order=bad) == -1
    assert call(opts(epochs=1), order=bad) == -2                       # only the rows of the call's epochs are looked at
    assert call(opts(), ws=int(L.evc_prox_masked_learn_workspace_bytes(25, 17, 70, 32, _lib.F64)) - 1) == -2


def test_workspace_query():
    _lib, L = lib()
    q = L.evc_prox_masked_learn_workspace_bytes
    assert q(1057, 64, 100, 10, 0) == 0 and q(25, 1025, 100, 10, 0) == 0 and q(257, 1024, 100, 10, 0) == 0 and q(0, 64, 100, 10, 0) == 0
    assert q(25, 64, 0, 1, 0) == 0 and q(25, 64, 100, 0, 0) == 0 and q(25, 64, 100, 101, 0) == 0 and q(25, 64, 100, 10, 9) == 0
    assert q(256, 1024, 100, 100, 0) > 0 and q(1056, 504, 100, 100, 1) > 0
    assert q(25, 64, 688, 64, _lib.F32) < q(25, 64, 688, 64, _lib.F64) < q(25, 64, 688, 128, _lib.F64)
    for M, N, T, bs, dt, es in ((25, 64, 130, 32, _lib.F64, 8), (201, 256, 2048, 256, _lib.F32, 4)):
        own = ((N + 2 * M) * bs + 3 * N * M) * es + N * 8 + T * 4 + int(L.evc_prox_masked_workspace_bytes(M, N, bs, 1, dt))
        assert own <= int(q(M, N, T, bs, dt)) <= own + 10 * 256


# ---- the restatement against every recorded deComP run ----
@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_reproduces_decomp(name):
    """deComP's solve_cd_mask against the restatement with the frame orders of the shuffle rule: the same `it`, D and x to
    100 eps steps (measured where the fixtures were recorded: 0 .. 5.0e-15)"""
    d = load(name)
    D, x, n_epochs, n_steps, trace, (S, Q, count) = restate(d)
    stopped = n_steps > 0 and trace[n_steps - 1] < float(d["tol"])
    assert (n_epochs if stopped else int(d["maxiter"])) == int(d["it"]) and n_steps == int(d["n_steps"]) == count
    assert S.shape == (d["y"].shape[1],) + 2 * d["D0"].shape[:1] and Q.shape == d["D0"].shape
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
        assert float(d["d_restated"]) <= 100 * EPS * int(d["n_steps"]) and float(d["x_restated"]) <= 100 * EPS * int(d["n_steps"])
        T, bs, mask = d["y"].shape[0], int(d["bs"]), d["mask"]
        assert mask.shape == d["y"].shape and np.all(mask >= 0) and np.all(np.isfinite(d["D"])) and np.all(np.isfinite(d["x"]))
        for row in d["order"]:                                      # every batch holds a non-zero weight
            assert all(np.any(mask[row[b * bs:(b + 1) * bs]] > 0) for b in range(T // bs))
    shapes = {name: d["y"].shape + d["D0"].shape[:1] + (int(d["bs"]),) for name, d in kinds.items()}
    assert list(shapes.values())[:5] == [(101, 5, 3, 50), (130, 25, 40, 32), (64, 12, 10, 16), (12, 1, 5, 4), (100, 201, 48, 48)]
    assert sum(1 for T, _, _, bs in shapes.values() if T % bs) >= 3                  # frames are left alone every epoch
    assert [str(kinds[n]["method"]) for n in FIXTURES[:3]] == ["fista", "fista_pos", "ista_pos"]
    stops = {n: int(d["n_steps"]) for n, d in kinds.items() if float(d["tol"]) > 0}
    assert set(stops) == {"proxml_m5_n3_t101_fista", "proxml_m12_n10_t64_ista_pos"} and all(5 < s < 999 for s in stops.values())
    assert int(kinds["proxml_m25_n40_t130_fista_pos_k4"]["n_steps"]) == 12 and int(kinds["proxml_m1_n5_t12_k4"]["maxiter"]) == 4
    assert int(kinds["proxml_m201_n48_t100_k3"]["maxiter"]) == 3
    signed = kinds["proxml_m5_n3_t101_fista"]
    assert not signed["positive"] and (signed["x"] < 0).any()
    for name in FIXTURES[:3]:                                       # binary, with a frame without any valid bin
        m = kinds[name]["mask"]
        assert set(np.unique(m)) == {0.0, 1.0} and np.sum(~np.any(m > 0, axis=1)) >= 1
    w = kinds["proxml_m25_n40_t130_weights_k3"]["mask"]
    assert np.any((w > 0) & (w < 1)) and np.any(w == 0) and np.array_equal(w, w.astype(np.float32))
    holes = kinds["proxml_m12_n10_t64_holes_k3"]
    first = holes["order"][0, :int(holes["bs"])]
    assert np.sum(~np.any(holes["mask"] > 0, axis=1)) >= 1 and np.any(~np.any(holes["mask"][first] > 0, axis=0))
    assert not np.any(~np.any(holes["mask"] > 0, axis=0))            # ... a bin the first batch lacks, not the whole call
    unused = kinds["proxml_m8_n6_t40_unused_atom_k3"]
    assert np.all(unused["x0"] == 0) and np.all(unused["x"][:, -1] == 0) and np.array_equal(unused["D"][-1], unused["D0"][-1])
    ones = kinds["proxml_m12_n10_t64_ones_k3"]
    assert np.all(ones["mask"] == 1) and float(ones["unmasked_differs"]) > 1e-6
    plain = plr.solve(ones["y"], ones["D0"], float(ones["alpha"]), batch_size=int(ones["bs"]), epochs=2, order=ones["order"])
    assert np.max(np.abs(plain[0] - ones["D"])) > 1e-6               # a mask of ones is not the unmasked learner


def test_restatement_options():
    y, D0 = pmlr.problem(25, 40, 70, 3)
    mask = pmlr.problem_mask(70, 25, 3)
    order = pmlr.decomp_order(70, 3, 5)
    kw = dict(mask=mask, batch_size=32, order=order)
    whole = pmlr.solve(y, D0, 1e-3, epochs=3, **kw)
    first = pmlr.solve(y, D0, 1e-3, epochs=2, **kw)
    second = pmlr.solve(y, first[0], 1e-3, first[1], mask=mask, batch_size=32, epochs=1, order=order[2:], state=first[5])
    assert np.array_equal(second[0], whole[0]) and np.array_equal(second[1], whole[1]) and second[5][2] == whole[5][2] == 6
    assert np.array_equal(second[5][0], whole[5][0]) and np.array_equal(second[5][1], whole[5][1])
    assert pmlr.solve(y, D0, 1e-3, epochs=0, **kw)[3] == 0 and pmlr.solve(y, D0, 1e-3, epochs=3, max_steps=4, **kw)[3] == 4
    x32 = pmlr.solve(y, D0, 1e-3, epochs=1, dtype=np.float32, **kw)
    assert x32[0].dtype == np.float32 and x32[1].dtype == np.float32 and x32[5][0].dtype == np.float32
    cuts = {}
    pmlr.solve(y, D0, 1e-3, epochs=1, cuts=cuts, **kw)
    assert cuts["pre"].shape == (70, 40) and np.all(np.isnan(cuts["pre"][order[0, 64:]])) and np.isfinite(cuts["thr"][order[0, 0]]).all()
    # a batch without any valid bin: L = 0, the activations and then the dictionary become NaN, and the call never stops
    dead = mask.copy()
    dead[order[0, :32]] = 0.0
    out = pmlr.solve(y, D0, 1e-3, epochs=1, tol=1e-3, **dict(kw, mask=dead))
    assert np.all(np.isnan(out[0])) and out[3] == 2 and np.all(np.isnan(out[4]))


# ---- the Python surfaces refuse before any device is asked for ----
def test_compat_refusal_names_the_native_call():
    from exemplars_vc_amd.compat import decomp
    y, D = np.ones((12, 4)), np.ones((3, 4))
    with pytest.raises(NotImplementedError, match="mask") as e:
        decomp.dictionary_learning.solve(y, D, 0.1, minibatch=4, lasso_method="fista", mask=np.ones_like(y))
    assert "learn_dictionary_sparse(mask=" in str(e.value) and "learn_dictionary_sparse(mask=" in decomp.__doc__


def test_solver_refuses_a_bad_mask(monkeypatch):
    import exemplars_vc_amd as evc
    from exemplars_vc_amd import solver

    def no_device(*a, **k):
        raise AssertionError("a device was asked for before the mask was refused")
    monkeypatch.setattr(solver, "require_device", no_device)
    X, D0 = np.ones((4, 12)), np.ones((4, 3))
    kw = dict(alpha=0.1, layout="bin_major", batch_size=4, epochs=1)
    nan, neg = np.ones((4, 12)), np.ones((4, 12))
    nan[1, 2], neg[3, 0] = np.nan, -0.5
    for bad in (np.ones((12, 4)), np.ones((4, 11)), np.ones(12), nan, neg, np.full((4, 12), np.inf), np.ones((4, 12), dtype=complex)):
        with pytest.raises(ValueError, match="mask"):
            evc.learn_dictionary_sparse(X, D0, mask=bad, **kw)
    A, B = np.ones((4, 12)), np.ones((5, 12))
    for side in (dict(mask_a=np.ones((5, 12))), dict(mask_b=np.ones((4, 12))), dict(mask_a=neg), dict(mask_b=np.full((5, 12), np.nan))):
        with pytest.raises(ValueError, match="mask"):
            evc.compact_dictionary_sparse(A, B, 3, alpha=0.1, batch_size=4, **side)
    with pytest.raises(AssertionError, match="a device was asked for"):             # a good mask goes on to the device
        evc.learn_dictionary_sparse(X, D0, mask=np.ones((4, 12)), **kw)


# ---- the host pieces of the driver (csrc/evc_prox_masked_learn_plan.h) in a program of their own ----
SRC = os.path.join(ROOT, "tests", "prox_masked_learn_host_main.hip")
PKG = os.path.join(ROOT, "exemplars_vc_amd")


def _program_lines(tmp, sanitize):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = os.path.join(tmp, "prox_masked_learn_host_main" + ("_san" if sanitize else ""))
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
    tmp = str(tmp_path_factory.mktemp("prox_masked_learn_host"))
    return _program_lines(tmp, False), tmp


def test_host_carving_and_argument_checks(program):
    _lib, L = lib()
    carves = [ln.split() for ln in program[0] if ln.startswith("carve ")]
    assert len(carves) == 24 and not any("BAD" in ln for ln in program[0])
    for c in carves:
        M, N, T, bs, esize, shift = (int(v) for v in c[1:6] + [c[7]])
        offs = [int(v) for v in c[9:17]]
        assert len(offs) == 8 and c[17] == "bytes"
        assert offs[0] == (256 - shift) % 256 and offs == sorted(offs) and all((o + shift) % 256 == 0 for o in offs)
        query = int(L.evc_prox_masked_learn_workspace_bytes(M, N, T, bs, _lib.F64 if esize == 8 else _lib.F32))
        assert int(c[-1]) == query and int(c[-3]) <= query <= int(c[-3]) + 512
    args = {ln.split()[1]: int(ln.split()[2]) for ln in program[0] if ln.startswith("args ")}
    want = dict(ok=0, ok_exact=0, short_by_one=-2, no_opts=-1, no_x=-1, no_mask=-1, no_d=-1, no_h=-1, no_stats_s=-1, no_stats_q=-1,
                no_workspace=-1, struct_bytes=-1, dtype=-1, layout=-1, batch_0=-1, batch_T=0, batch_T_plus_1=-1, epochs_neg=-1,
                epochs_0=0, steps_beyond_int=-1, lasso_iters_neg=-1, lasso_iters_0=0, slots_4098=-1, slots_4097=0,
                check_every_neg=-1, mode=-1, mode_signed=0, momentum=-1, momentum_nesterov=0, resume_2=-1, resume_1=0,
                resume_count_neg=-1, fresh_count_neg=0, reserved=-1, reserved_halves_off=0, reserved2=-1, alpha_neg=-1,
                alpha_nan=-1, alpha_0=0, tol_neg=-1, tol_inf=-1, tol_set=0, lasso_tol_nan=-1, lasso_tol_0=0, ldx_short=-1,
                ldm_short=-1, ldd_short=-1, ldh_short=-1, ld_s_short=-1, ld_q_short=-1, padded=0, bin_major=0,
                bin_major_ldm_short=-1, bin_major_ldd_short=-1, M_0=-1, T_0=-1, M_1056=0, M_1057=-3, M_1057_small_ws=-3, N_1024=0,
                N_1024_small_ws=-2, N_1025=-3, S_at_the_limit=0, S_beyond=-3, nan_before_limits=-1, order_good=-2, order_twice=-1,
                order_first_row_only=-2)
    assert args == want
    limits = {tuple(int(v) for v in ln.split()[1:3]): int(ln.split()[3]) for ln in program[0] if ln.startswith("limit ")}
    assert len(limits) == 9
    for (M, N), big in limits.items():
        assert big == int(M > 1056 or N > 1024 or M * N * N > 2 ** 28)
    lasso = {ln.split()[1]: ln.split()[2] for ln in program[0] if ln.startswith("lasso ")}
    assert lasso == dict(struct_bytes="1", layout=str(_lib.BIN_MAJOR), iters="7", mode=str(_lib.PROX_SIGNED),
                         momentum=str(_lib.PROX_ISTA), normalize="1", check_every="3", stop_rule=str(_lib.STOP_DECOMP),
                         init_mode=str(_lib.INIT_GIVEN), lip_weights=str(_lib.PROX_LIP_MEAN), reserved="0", alpha="0.001",
                         tol="1.0000000000000001e-05", lipschitz="0")


def test_the_host_program_runs_clean_under_the_sanitizers(program):
    """a stand-alone program: address + undefined-behaviour sanitizers on the host code, nothing preloaded anywhere"""
    assert _program_lines(program[1], True) == program[0]
