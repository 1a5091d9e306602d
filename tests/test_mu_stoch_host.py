"""deComP's mini-batch NMF (evc_mu_stoch_learn), host side: the C ABI's declarations and struct mirror, the numpy restatement
against every recorded deComP run (bit for bit), the frame orders of both families, the compat layer with the native call
replaced by the restatement, the Python surfaces' errors and the stand-alone host program (csrc/evc_mu_stoch_plan.h), plainly
and under the sanitizers.  No GPU needed."""
import ctypes as C
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
import mu_masked_restatement as mmr  # noqa: E402
import mu_stoch_restatement as msr  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ["mus_asg_m25_r8_t50_bs16_l2_mask", "mus_gsg_m40_r19_t70_bs16_kl", "mus_asag_m201_r12_t40_bs16_kl_mask",
            "mus_asag_m40_r19_t70_bs16_l2_mid", "mus_gsag_m25_r8_t50_bs7_l2_last", "mus_svrmu_m40_r19_t70_bs16_l2_mask",
            "mus_svrmu_m25_r8_t48_bs16_kl_mask", "mus_svrmuacc_m25_r8_t50_bs16_kl", "mus_asg_m2_r3_t5_bs2_kl"]


def lib():
    from exemplars_vc_amd import _lib
    return _lib, _lib.lib()


def load(name):
    d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    for k in ("y", "D0", "mask", "x0"):
        d[k] = d[k].astype(np.float64) if k in d else None
    for k in ("loss", "method", "where"):
        d[k] = str(d[k])
    for k in ("it", "n_steps", "n_epochs", "maxiter", "bs", "inner_iters", "seed"):
        d[k] = int(d[k])
    for k in ("tol", "forget_rate", "alpha", "beta", "perm64", "perm32"):
        d[k] = float(d[k])
    d["native"] = msr.NATIVE[d["method"]]
    return d


def restated(d, **over):
    kw = dict(mask=d["mask"], method=d["native"], loss=d["loss"], batch_size=d["bs"], epochs=d["maxiter"] - 1, tol=d["tol"],
              forget_rate=d["forget_rate"], alpha=d["alpha"], inner_iters=d["inner_iters"], order=d["order"])
    kw.update(over)
    return msr.learn(d["y"], d["D0"], d["x0"], **kw)


# ---- the C ABI's face ----
def test_symbols_declared_and_exported():
    _lib, L = lib()
    hdr = open(os.path.join(ROOT, "include", "evc.h")).read()
    declared = set(re.findall(r"\b(evc_[a-z_0-9]+)\s*\(", hdr))
    for sym in ("evc_mu_stoch_learn_workspace_bytes", "evc_mu_stoch_learn_route", "evc_mu_stoch_learn_splits", "evc_mu_stoch_learn"):
        assert sym in declared and sym in _lib.SYMBOLS and hasattr(L, sym)
    assert (_lib.STOCH_ASG, _lib.STOCH_ASAG, _lib.STOCH_GSAG, _lib.STOCH_SVRMU) == (0, 1, 2, 3)
    assert re.search(r"EVC_STOCH_ASG = 0, EVC_STOCH_ASAG = 1, EVC_STOCH_GSAG = 2, EVC_STOCH_SVRMU = 3", hdr)


def test_opts_mirror_matches_header():
    _lib, _ = lib()
    hdr = open(os.path.join(ROOT, "include", "evc.h")).read()
    body = hdr[hdr.index("typedef struct evc_mu_stoch_opts {"):hdr.index("} evc_mu_stoch_opts;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for grp in re.findall(r"\b(?:int|double|void\*)\s+([a-zA-Z_0-9, ]+);", body) for n in grp.replace(" ", "").split(",")]
    assert names == [f[0] for f in _lib.MuStochOpts._fields_]
    assert C.sizeof(_lib.MuStochOpts) == 12 * 4 + 3 * 8 + 2 * 8
    assert C.sizeof(_lib.MuMaskedLearnOpts) == 8 * 4 + 8 + 2 * 8                    # the existing struct did not move


def test_statuses_through_the_library():
    """the same checks as the host program's, through the shared library: before any device work, in the statuses' order"""
    _lib, L = lib()
    one = C.c_void_p(8)              # never dereferenced: every case fails validation first

    def opts(**kw):
        o = _lib.MuStochOpts()
        o.struct_bytes = C.sizeof(o)
        o.dtype, o.layout, o.loss, o.method = _lib.F64, _lib.FRAME_MAJOR, _lib.LOSS_KL, _lib.STOCH_ASAG
        o.batch_size, o.epochs, o.inner_iters, o.forget_rate, o.alpha, o.tol = 16, 3, 1, 0.5, 1.0, 1e-3
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def call(o, M=25, R=8, T=50, ldx=25, ldm=25, ldw=25, ldh=8, ws=16, X=one, mask=one, W=one, H=one, wsp=one, order=None):
        return L.evc_mu_stoch_learn(X, ldx, mask, ldm, W, ldw, H, ldh, order, M, R, T, None if o is None else C.byref(o), wsp, ws,
                                    None, None, None, None)
    assert call(opts()) == -2 and call(opts(), mask=None, ldm=0) == -2 and call(None) == -1 and call(opts(), ldm=24) == -1
    assert call(opts(reserved=1)) == -1 and call(opts(tol=-1.0)) == -1 and call(opts(loss=2)) == -1 and call(opts(), T=0) == -1
    assert call(opts(method=4)) == -1 and call(opts(batch_size=51)) == -1 and call(opts(batch_size=0)) == -1
    assert call(opts(inner_iters=2)) == -1 and call(opts(inner_iters=2, method=_lib.STOCH_SVRMU)) == -2
    assert call(opts(forget_rate=0.0)) == -1 and call(opts(forget_rate=1.0)) == -2 and call(opts(order_rows=3)) == -1
    assert call(opts(route=1), R=257, ldh=257) == -3 and call(opts(route=2), R=257, ldh=257) == -2 and call(opts(route=3)) == -1
    assert call(opts(), M=529, ldx=529, ldm=529, ldw=529) == -3 and call(opts(), R=4097, ldh=4097) == -3
    bad = (C.c_int * 150)(*([0] * 150))
    good = (C.c_int * 150)(*(list(range(50)) * 3))
    assert call(opts(order_rows=3), order=bad) == -1 and call(opts(order_rows=3), order=good) == -2
    assert call(opts(order_rows=3), order=bad, M=529, ldx=529, ldm=529, ldw=529) == -1          # -1 before -3
    q, sp, rt = L.evc_mu_stoch_learn_workspace_bytes, L.evc_mu_stoch_learn_splits, L.evc_mu_stoch_learn_route
    assert q(529, 8, 50, 16, 0, 0) == 0 and q(25, 4097, 50, 16, 0, 0) == 0 and q(25, 8, 50, 51, 0, 0) == 0 and q(25, 8, 50, 16, 4, 0) == 0
    assert 0 < q(25, 8, 50, 16, 0, 1) < q(25, 8, 50, 16, 0, 0) < q(25, 8, 50, 16, 3, 0)          # svrmu keeps prev+-
    assert call(opts(), ws=int(q(25, 8, 50, 16, 1, 0)) - 1) == -2
    assert (rt(64, 0), rt(256, 0), rt(256, 1), rt(257, 1), rt(257, 0), rt(8, 3)) == (1, 1, 1, 0, 2, 0)
    # S is a function of (M, R, bs) and the route alone; the unfused route's is evc_mu_masked_learn's of the batch
    assert sp(25, 64, 256, 2) == L.evc_mu_masked_learn_splits(25, 64, 256) and sp(25, 64, 256, 1) == 4 and sp(25, 64, 16, 1) == 1
    assert sp(25, 64, 1 << 20, 1) == 64 and sp(529, 64, 256, 1) == 0 and sp(25, 257, 256, 1) == 0


# ---- the restatement against every recorded deComP run, bit for bit ----
@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_reproduces_decomp(name):
    d = load(name)
    r = restated(d)
    assert r["it"] == d["it"] and r["n_steps"] == d["n_steps"] and r["n_epochs"] == d["n_epochs"]
    assert len(r["stats"]) == len(d["stats"]) and np.array_equal(r["visited"], d["visited"])
    ones = np.ones_like(d["y"]) if d["mask"] is None else d["mask"]
    if mmr.blas_fingerprint(d["y"], d["D0"], ones) == d["blas_crc"].tolist():
        assert np.array_equal(r["D"], d["D"]) and np.array_equal(r["x"], d["x"]) and np.array_equal(r["stats"], d["stats"])
    else:                           # another BLAS summation order here: the GPU tests' bound
        fig = max(d["perm64"], len(d["stats"]) * np.finfo(np.float64).eps)
        for a, b in ((r["D"], d["D"]), (r["x"], d["x"]), (r["stats"], d["stats"])):
            assert float(np.max(np.abs(a - b)) / np.max(np.abs(b))) <= 100 * fig
    assert np.array_equal(r["x"][~d["visited"]], (np.ones_like(d["x"]) if d["x0"] is None else d["x0"])[~d["visited"]])


def test_fixture_set_is_what_the_tests_need():
    ds = [load(n) for n in FIXTURES]
    assert {d["method"] for d in ds} == set(msr.NATIVE) and {d["loss"] for d in ds} == {"l2", "kl"}
    assert any(d["mask"] is None for d in ds) and any(d["mask"] is not None for d in ds)
    assert all((d["mask"] == 0).any() and (d["mask"] > 0).any() for d in ds if d["mask"] is not None)
    assert 2 * sum(d["y"].shape[0] % d["bs"] != 0 for d in ds) >= len(ds)
    assert {"mid", "last", "max"} <= {d["where"] for d in ds}
    for d in ds:
        n_loop = d["y"].shape[0] // d["bs"]
        stopped = d["it"] < d["maxiter"]
        assert d["where"] == ("max" if not stopped else "last" if d["n_steps"] % n_loop == 0 else "mid")
        assert stopped == bool(d["stats"][-1] < d["tol"]) and not (d["stats"][:-1] < d["tol"]).any()
        assert np.min(np.abs(d["stats"] - d["tol"])) >= 1e-6 * d["tol"]
        assert 0 < d["perm64"] <= 1e-11 and 0 < d["perm32"]
    assert any(d["method"] == "svrmu-acc" and d["inner_iters"] >= 2 for d in ds)
    assert any(not d["visited"].all() for d in ds)
    assert all(os.path.getsize(os.path.join(GOLDEN, n + ".npz")) < (1 << 20) for n in FIXTURES)


@pytest.mark.parametrize("name", FIXTURES)
def test_frame_orders_of_both_families(name):
    from exemplars_vc_amd import solver
    d = load(name)
    T, epochs = d["y"].shape[0], d["maxiter"] - 1
    rows = 1 if d["native"] == "svrmu" else epochs
    assert d["order"].shape == (rows, T)
    assert np.array_equal(solver.decomp_frame_order(T, rows, d["seed"]), d["order"])
    assert np.array_equal(msr.frame_orders(T, epochs, d["seed"], d["native"]), d["order"])
    assert d["inner_iters"] == (msr.svrmu_acc_inner(d["D0"].shape[0], d["D0"].shape[1], T, d["beta"]) if d["method"] == "svrmu-acc" else 1)


# ---- the compat layer with the native call replaced by the restatement ----
def fake_native(calls):
    def fake(X, W0, H0, mask=None, **kw):
        calls.append((X, W0, H0, mask, kw))
        r = msr.learn(X, W0, H0, mask=mask, method=kw["method"], loss={"frobenius": "l2", "kl": "kl"}[kw["loss"]],
                      batch_size=kw["batch_size"], epochs=kw["epochs"], tol=kw["tol"], forget_rate=kw["forget_rate"], alpha=kw["alpha"],
                      inner_iters=kw["inner_iters"], order=kw["order"], dtype=X.dtype)
        n_loop = X.shape[0] // kw["batch_size"]
        return r["D"], r["x"], {"n_epochs": r["n_epochs"], "n_steps": r["n_steps"], "stat": r["stats"],
                                "stopped": r["it"] <= kw["epochs"], "n_loop": n_loop}
    return fake


@pytest.mark.parametrize("name", FIXTURES)
def test_compat_reproduces_the_recorded_runs(name, monkeypatch):
    from exemplars_vc_amd import solver
    from exemplars_vc_amd.compat import decomp
    calls = []
    monkeypatch.setattr(solver, "learn_dictionary_stochastic", fake_native(calls))
    d = load(name)
    extra = dict(alpha=d["alpha"], beta=d["beta"]) if d["native"] == "svrmu" else dict(forget_rate=d["forget_rate"])
    it, D, x = decomp.nmf.solve(d["y"], d["D0"], d["x0"], tol=d["tol"], minibatch=d["bs"], maxiter=d["maxiter"], method=d["method"],
                                likelihood=d["loss"], mask=d["mask"], random_seed=d["seed"], **extra)
    kw = calls[-1][4]
    assert kw["method"] == d["native"] and kw["inner_iters"] == d["inner_iters"] and kw["layout"] == "frame_major"
    assert kw["epochs"] == d["maxiter"] - 1 and kw["batch_size"] == d["bs"] and np.array_equal(kw["order"], d["order"])
    assert it == d["it"] and D.shape == d["D"].shape and x.shape == d["x"].shape
    ones = np.ones_like(d["y"]) if d["mask"] is None else d["mask"]
    if mmr.blas_fingerprint(d["y"], d["D0"], ones) == d["blas_crc"].tolist():
        assert np.array_equal(D, d["D"]) and np.array_equal(x, d["x"])


def test_compat_argument_translation_and_errors(monkeypatch):
    from exemplars_vc_amd import solver
    from exemplars_vc_amd.compat import decomp
    calls = []
    monkeypatch.setattr(solver, "learn_dictionary_stochastic", fake_native(calls))
    monkeypatch.setattr(solver, "learn_dictionary_masked", lambda *a, **k: pytest.fail("the batch call was taken"))
    y, D = np.ones((6, 4)) + np.arange(4), np.ones((5, 4)) + np.arange(5)[:, None]
    it, Dn, x = decomp.nmf.solve(y, D, minibatch=2, maxiter=4, method='gsg-mu', tol=0.0, random_seed=3)
    X, W0, H0, m, kw = calls[-1]
    assert it == 4 and Dn.shape == (5, 4) and x.shape == (6, 5) and np.array_equal(H0, np.ones((6, 5))) and m is None
    assert kw["method"] == "asg" and kw["epochs"] == 3 and kw["order"].shape == (3, 6) and kw["forget_rate"] == 0.5 and kw["alpha"] == 1.0
    assert kw["loss"] == "frobenius" and kw["tol"] == 0.0
    decomp.nmf.solve(y, D, minibatch=3, maxiter=4, method='svrmu', likelihood='kl', alpha=0.5, mask=np.ones((6, 4)), random_seed=3)
    kw = calls[-1][4]
    assert kw["method"] == "svrmu" and kw["order"].shape == (1, 6) and kw["alpha"] == 0.5 and kw["inner_iters"] == 1 and kw["loss"] == "kl"
    assert calls[-1][3] is not None
    decomp.nmf.solve(y, D, minibatch=3, maxiter=4, method='svrmu-acc', beta=8.0)
    assert calls[-1][4]["inner_iters"] == int(max(8.0 * 5 * (3 * 4 + 2 * 6) / (3 * 5 * 6 + 2 * 4), 1)) >= 2
    assert decomp.nmf.solve(y, D, minibatch=3, maxiter=1, method='asag-mu', forget_rate=0.25)[0] == 1 and calls[-1][4]["epochs"] == 0
    assert calls[-1][4]["forget_rate"] == 0.25
    assert decomp.nmf.solve(y.astype(np.float32), D.astype(np.float32), minibatch=2, maxiter=3, method='gsag-mu')[1].dtype == np.float32
    n = len(calls)
    with pytest.raises(NotImplementedError):
        decomp.nmf.solve(y, D, minibatch=2)                                   # 'mu' has no mini-batch form, as in deComP
    with pytest.raises(NotImplementedError, match="Batch-NMF with asg-mu algorithm"):
        decomp.nmf.solve(y, D, method='asg-mu')
    with pytest.raises(NotImplementedError):
        decomp.nmf.solve(y, D, minibatch=2, method='sgd')
    with pytest.raises(ValueError, match="Minibatch size should be smaller than the total size. Given 6 < 7"):
        decomp.nmf.solve(y, D, minibatch=7, method='svrmu')
    with pytest.raises(NotImplementedError, match="unknown options"):
        decomp.nmf.solve(y, D, minibatch=2, method='svrmu', forget_rate=0.5)
    with pytest.raises(NotImplementedError, match="unknown options"):
        decomp.nmf.solve(y, D, minibatch=2, method='asg-mu', alpha=0.5)
    with pytest.raises(NotImplementedError, match="complex"):
        decomp.nmf.solve(y.astype(complex), D.astype(complex), minibatch=2, method='asg-mu')
    with pytest.raises(ValueError, match="identical"):
        decomp.nmf.solve(y, D, minibatch=2, method='asg-mu', mask=np.ones(4))  # a 1-D mask
    with pytest.raises(AssertionError):
        decomp.nmf.solve(y, -D, minibatch=2, method='asg-mu')
    assert len(calls) == n and "evc_mu_stoch_learn" in decomp.__doc__ and decomp.nmf.MINIBATCH_METHODS == list(msr.NATIVE)


# ---- the Python surface ----
def test_wrapper_rejects_bad_arguments_before_any_device(monkeypatch):
    import exemplars_vc_amd as evc
    from exemplars_vc_amd import solver
    assert "learn_dictionary_stochastic" in evc.__all__
    sig = inspect.signature(evc.learn_dictionary_stochastic).parameters
    assert list(sig)[:4] == ["X", "W0", "H0", "mask"] and sig["forget_rate"].default == 0.5 and sig["alpha"].default == 1.0
    assert sig["inner_iters"].default == 1 and sig["method"].default is inspect.Parameter.empty
    for k in ("method", "loss", "layout", "batch_size", "epochs", "tol", "order", "seed", "route", "info"):
        assert sig[k].kind is inspect.Parameter.KEYWORD_ONLY, k
    monkeypatch.setattr(solver, "require_device", lambda device=None: pytest.fail("a device was asked for"))
    Xb, W0, H0 = np.ones((4, 6)), np.ones((4, 2)), np.ones((2, 6))
    ok = dict(method="asg", layout="bin_major", batch_size=2, epochs=2)
    for bad, match in ((dict(method="mu"), "method"), (dict(loss="is"), "loss"), (dict(route="auto"), "route"), (dict(tol=-1.0), "tol"),
                       (dict(forget_rate=0.0), "forget_rate"), (dict(alpha=np.inf), "alpha"), (dict(batch_size=7), "batch_size"),
                       (dict(batch_size=0), "batch_size"), (dict(epochs=-1), "epochs"), (dict(inner_iters=2), "inner_iters"),
                       (dict(order=np.zeros((2, 6), dtype=int)), "permutation"), (dict(order=np.arange(6)), "permutation"),
                       (dict(order=np.tile(np.arange(6), (3, 1))), "permutation")):
        with pytest.raises(ValueError, match=match):
            evc.learn_dictionary_stochastic(Xb, W0, H0, **dict(ok, **bad))
    with pytest.raises(ValueError, match="mask has shape"):
        evc.learn_dictionary_stochastic(Xb, W0, H0, np.ones((6, 4)), **ok)
    with pytest.raises(ValueError, match="finite weights >= 0"):
        evc.learn_dictionary_stochastic(Xb, W0, H0, -np.ones((4, 6)), **ok)
    with pytest.raises(ValueError, match="at most 528"):
        evc.learn_dictionary_stochastic(np.ones((529, 6)), np.ones((529, 2)), H0, **ok)


def test_a_good_call_reaches_the_device_or_raises_without_one():
    import torch
    import exemplars_vc_amd as evc
    Xb, W0, H0 = np.ones((4, 6)), np.ones((4, 2)), np.ones((2, 6))
    if torch.cuda.is_available():
        W, H = evc.learn_dictionary_stochastic(Xb, W0, H0, method="svrmu", layout="bin_major", batch_size=2, epochs=2, seed=1)
        assert W.shape == (4, 2) and H.shape == (2, 6) and np.allclose(np.sum(W * W, axis=0), 1.0)
    else:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            evc.learn_dictionary_stochastic(Xb, W0, H0, method="svrmu", layout="bin_major", batch_size=2, epochs=2, seed=1)


# ---- the host pieces of the driver (csrc/evc_mu_stoch_plan.h) in a program of their own, plainly and under the sanitizers ----
SRC = os.path.join(ROOT, "tests", "mu_stoch_host_main.hip")
PKG = os.path.join(ROOT, "exemplars_vc_amd")


def _program_lines(tmp, sanitize):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = os.path.join(tmp, "mu_stoch_host_main" + ("_san" if sanitize else ""))
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
    tmp = str(tmp_path_factory.mktemp("mu_stoch_host"))
    return _program_lines(tmp, False), tmp


def test_host_carving_and_argument_checks(program):
    _lib, L = lib()
    carves = [ln.split() for ln in program[0] if ln.startswith("carve ")]
    assert len(carves) == 32 and not any("BAD" in ln for ln in program[0])
    for c in carves:
        M, R, T, bs, method, esize, shift = (int(v) for v in c[1:7] + [c[8]])
        offs = [int(v) for v in c[10:26]]
        assert len(offs) == 16 and c[26] == "bytes"
        # no overlap (the program checks every array's room), every start a multiple of 256 bytes, the total is the query
        assert offs[0] == (256 - shift) % 256 and offs == sorted(offs) and all((o + shift) % 256 == 0 for o in offs)
        query = int(L.evc_mu_stoch_learn_workspace_bytes(M, R, T, bs, method, _lib.F64 if esize == 8 else _lib.F32))
        assert int(c[-1]) == query and int(c[-3]) <= query <= int(c[-3]) + 512
        assert (offs[11] > offs[10]) == (method == _lib.STOCH_SVRMU)           # prev+- only where svrmu keeps them
    args = {ln.split()[1]: int(ln.split()[2]) for ln in program[0] if ln.startswith("args ")}
    want = dict(ok=0, ok_exact=0, short_by_one=-2, asag_ws_for_svrmu=-2, no_mask=0, ldm_short=-1, ldw_short=-1, no_w=-1,
                struct_bytes=-1, reserved=-1, reserved2=-1, loss=-1, loss_kl=0, method_4=-1, method_neg=-1, bs_0=-1, bs_T=0,
                bs_T_plus_1=-1, epochs_neg=-1, epochs_0=0, steps_overflow=-1, inner_0=-1, inner_2_asag=-1, inner_2_svrmu=0,
                route_3=-1, fused_256=0, fused_257=-3, unfused_257=0, auto_257=0, rho_0=-1, rho_1=0, rho_big=-1, rho_nan=-1,
                alpha_inf=-1, tol_neg=-1, tol_nan=-1, tol_0=0, dtype=-1, layout=-1, order_rows_no_order=-1, order_ok=0,
                order_one_row=0, order_rows_2_of_3=-1, order_rows_0_with_order=-1, order_twice=-1, order_twice_row_not_used=0,
                order_far=-1, order_bad_before_limits=-1, T_0=-1, M_528=0, M_529=-3, R_4096=0, R_4097=-3, tol_before_limits=-1,
                prev_too_large=-3, asag_same_sizes=0)
    assert args == want
    # the size query is 0 exactly where the call refuses with -1 or -3
    query = {ln.split()[1]: int(ln.split()[2]) for ln in program[0] if ln.startswith("query ")}
    assert query["ok"] > 0 and query["limits"] > 0 and len(query) == 12
    assert all(v == 0 for k, v in query.items() if k not in ("ok", "limits"))
    prev = {ln.split()[1]: (int(ln.split()[2]), int(ln.split()[3])) for ln in program[0] if ln.startswith("prev ")}
    assert prev == dict(at_limit=(1, 1 << 40), past_limit=(0, 0), int_max=(0, 0), not_svrmu=(1, 0), small=(1, 3 * 2 * 25 * 8 * 4))
    order = {ln.split()[1]: int(ln.split()[2]) for ln in program[0] if ln.startswith("order ")}
    assert order == dict(good=0, null=0, no_rows=0, dup=-1, dup_first_row_only=0, neg=-1, big=-1)
    routes = {(int(ln.split()[1]), int(ln.split()[2])): int(ln.split()[3]) for ln in program[0] if ln.startswith("route ")}
    assert len(routes) == 24
    for (R, route), r in routes.items():
        assert r == (0 if route == 3 else route if route else 1 if R <= 256 else 2)


def test_the_host_program_runs_clean_under_the_sanitizers(program):
    """a stand-alone program: address + undefined-behaviour sanitizers on the host code, nothing preloaded anywhere"""
    assert _program_lines(program[1], True) == program[0]
