"""The three fixed-dictionary entries (evc_nmf_solve / evc_nmf_convert, evc_cd_solve, evc_beta_solve) give bit for bit what
they gave before their host drivers came to share one skeleton: sha256 of the outputs, n_iter and the
error / violation trace of the calls below, recorded on the commit before that change by
`tools/make_learn_digests.py test_gpu_solve_digests`, which runs CASES as they stand here, twice each.  Every call reads
a fixture of tests/golden; together they take the paths the shared code has: both layouts, float32, several utterances
with an empty one (where the tile table's utt_tile0 and .w go wrong), a warm start, a violation trace longer than the
device ring (CD_TRACE_CAP = 256), both starts of the beta solve over an empty utterance, a workspace that does not start at
a multiple of 256 bytes, and for the Python wrapper of evc_nmf_solve / evc_nmf_convert: utterance offsets with the
sklearn stop rule, no H wanted, a prepared dictionary that holds B, `out=` and a caller's H0 on the device.

beta_reg_b0p5 is the call tests/test_gpu_beta_learn.py pinned earlier (the activations alone): the same digest."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def fixture(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def host(a):
    return np.ascontiguousarray(a if isinstance(a, np.ndarray) else a.cpu().numpy())


def digest(outs, info=None, trace=None):
    h = hashlib.sha256()
    for a in outs:
        h.update(host(a).tobytes())
    if info is not None:
        h.update(np.ascontiguousarray(info["n_iter"], dtype=np.int32).tobytes())
        h.update(np.ascontiguousarray(info[trace], dtype=np.float64).tobytes())
    return h.hexdigest()


def oriented(layout):
    """the fixtures hold frames (and exemplars) as rows: frame_major as they are, bin_major transposed"""
    return (lambda a: a) if layout == "frame_major" else (lambda a: np.ascontiguousarray(a.T))


def reg(d):
    M = d["X_rows"].shape[1]
    a, r = float(d["alpha_W"]), float(d["l1_ratio"])
    return dict(l1=M * a * r, l2=M * a * (1 - r))


def ragged(X):
    """three utterances, the middle one empty (tests/test_gpu_beta.py's batch)"""
    utts = [X[:23], X[:0], X[7:20] + 0.2]
    return np.concatenate(utts), np.concatenate([[0], np.cumsum([len(x) for x in utts])])


# ---- evc_cd_solve ----

def cd(name, layout="frame_major", H0=None, X=None, **kw):
    import exemplars_vc_amd as evc
    d = fixture(name)
    t = oriented(layout)
    kw.setdefault("max_iter", int(d["max_iter"]))
    kw.setdefault("tol", float(d["tol"]))
    H, info = evc.solve_activations_cd(t(d["W_rows"]), t(d["X_rows"] if X is None else X), None if H0 is None else t(H0),
                                       layout=layout, info=True, **reg(d), **kw)
    return digest([H], info, "violation"), info


def cd_empty_utterance():
    """M = 25: tiles of 32 frames.  Two tiles, the all-zero frames, no frames at all, one tile"""
    X, Z = fixture("cdnmf_m25_n64_t32")["X_rows"], fixture("cdnmf_m25_zero_utt")["X_rows"]
    utts = [np.concatenate([X, X[:7]]), Z, X[:0], X[5:]]
    offs = np.concatenate([[0], np.cumsum([len(x) for x in utts])])
    dg, info = cd("cdnmf_m25_zero_utt", X=np.concatenate(utts), utt_offsets=offs)
    assert list(info["n_iter"][1:3]) == [1, 1]
    return dg


def cd_warm_start():
    d = fixture("cdnmf_m6_n17_t70")
    return cd("cdnmf_m6_n17_t70", H0=0.5 * d["H"].T + 0.01, max_iter=20)[0]


def cd_trace_past_the_ring():
    dg, info = cd("cdnmf_m6_n17_t70", tol=0.0, max_iter=300)
    assert info["n_iter"][0] == 300 and np.isfinite(info["violation"]).all()
    return dg


# ---- evc_beta_solve ----

def beta(name, layout="bin_major", X=None, check_every=10, **kw):
    import exemplars_vc_amd as evc
    d = fixture(name)
    t = oriented(layout)
    tol = float(d["tol"])
    kw.setdefault("beta", float(d["beta"]))
    kw.setdefault("iters", int(d["max_iter"]))
    H, info = evc.solve_activations_beta(t(d["W_rows"]), t(d["X_rows"] if X is None else X), layout=layout,
                                         check_every=check_every, stop_rule="sklearn" if tol > 0 else "none", tol=tol,
                                         info=True, **reg(d), **kw)
    return digest([H], info, "err"), info


def beta_reg():
    """as tests/test_gpu_beta_learn.py makes the call and hashes it"""
    import exemplars_vc_amd as evc
    d = fixture("betamu_m25_n64_t50_reg_b0p5")
    H = evc.solve_activations_beta(d["W_rows"], d["X_rows"], beta=0.5, layout="frame_major", iters=int(d["max_iter"]),
                                   init="sklearn", **reg(d))
    return digest([np.ascontiguousarray(H, dtype=np.float64)])


def beta_early_stop():
    d = fixture("betamu_m25_n64_t50_b0_tol2e-2")
    dg, info = beta("betamu_m25_n64_t50_b0_tol2e-2")
    assert info["n_iter"][0] == int(d["n_iter"]) < int(d["max_iter"])
    return dg


def beta_empty_utterance(init):
    X, offs = ragged(fixture("betamu_m25_n64_t50_b0_tol2e-2")["X_rows"])
    return beta("betamu_m25_n64_t50_b0_tol2e-2", X=X, utt_offsets=offs, beta=0.5, iters=40, init=init, init_value=0.3)[0]


# ---- one raw call through the C ABI, float64, the workspace 8 bytes past a multiple of 256 ----

def raw_shifted(entry):
    import torch
    from exemplars_vc_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    cd_ = entry == "evc_cd_solve"
    d = fixture("cdnmf_m25_n64_t32" if cd_ else "betamu_m25_n64_t32_k50_b0p5")
    A, X = (torch.from_numpy(d[k]).to(dev) for k in ("W_rows", "X_rows"))
    (T, M), N = X.shape, A.shape[0]
    H = torch.empty((T, N), dtype=torch.float64, device=dev)
    if cd_:
        o = _lib.CdOpts()
        o.struct_bytes, o.layout, o.init_mode, o.max_iter, o.tol = C.sizeof(o), _lib.FRAME_MAJOR, _lib.INIT_SKLEARN, 12, 1e-4
        trace = np.zeros((1, 12))
        nbytes = int(L.evc_cd_workspace_bytes(M, N, T, 1, _lib.F64))
    else:
        o = _lib.BetaOpts()
        o.struct_bytes, o.layout, o.init_mode, o.iters, o.check_every, o.beta = (C.sizeof(o), _lib.FRAME_MAJOR,
                                                                                 _lib.INIT_SKLEARN, 12, 4, 0.5)
        trace = np.zeros((1, 4))
        nbytes = int(L.evc_beta_workspace_bytes(M, N, T, 1, _lib.F64))
    assert nbytes > 0
    buf = torch.empty(nbytes + 512, dtype=torch.uint8, device=dev)
    ws = (buf.data_ptr() + 255) // 256 * 256 + 8
    n_iter = np.zeros(1, dtype=np.int32)
    with torch.cuda.device(dev):
        st = getattr(L, entry)(A.data_ptr(), A.stride(0), X.data_ptr(), X.stride(0), H.data_ptr(), H.stride(0), M, N, T,
                               None, 1, C.byref(o), ws, nbytes, n_iter.ctypes.data_as(C.POINTER(C.c_int)),
                               trace.ctypes.data_as(C.POINTER(C.c_double)),
                               C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    _lib.check(st, entry)
    torch.cuda.synchronize()
    return digest([H], {"n_iter": n_iter, "t": trace}, "t")


# ---- evc_nmf_solve / evc_nmf_convert: the Python wrapper ----

SK = dict(layout="frame_major", eps_mode="zero_replace", init="sklearn")


def nmf_plain():
    import exemplars_vc_amd as evc
    d = fixture("sklearn_m25_n64_t32_k50")
    H, info = evc.solve_activations(d["W_rows"], d["X_rows"], iters=50, check_every=10, info=True, **SK)
    return digest([H], info, "err")


def nmf_utterances_sklearn_stop():
    import exemplars_vc_amd as evc
    d = fixture("sklearn_m25_n64_t50_tol5e-2")
    X, offs = ragged(d["X_rows"])
    H, info = evc.solve_activations(d["W_rows"], X, iters=int(d["max_iter"]), check_every=10, stop_rule="sklearn",
                                    tol=float(d["tol"]), utt_offsets=offs, info=True, **SK)
    return digest([H], info, "err")


def nmf_convert_no_h():
    import exemplars_vc_amd as evc
    d = fixture("sklearn_m25_n64_t32_k50")
    Y, info = evc.convert(d["W_rows"], d["X_rows"], d["B_rows"], want_h=False, iters=50, info=True, **SK)
    return digest([Y], info, "err")


def nmf_prepared_with_b():
    import exemplars_vc_amd as evc
    d = fixture("sklearn_m25_n64_t32_k50")
    pd = evc.prepare_dictionary(d["W_rows"], d["B_rows"], layout="frame_major")
    H, Y, info = evc.convert(pd, d["X_rows"], iters=50, check_every=10, info=True, **SK)
    return digest([H, Y], info, "err")


def nmf_out_given():
    import torch
    import exemplars_vc_amd as evc
    d = fixture("sklearn_m25_n64_t32_k50")
    out = torch.full((32, 64), -1.0, dtype=torch.float64, device="cuda:0")
    H, info = evc.solve_activations(d["W_rows"], d["X_rows"], iters=50, out=out, info=True, **SK)
    assert H is out
    return digest([out], info, "err")


def nmf_h0_on_the_device():
    import torch
    import exemplars_vc_amd as evc
    d = fixture("pymf_m25_n64_t32_k50_err")
    A, X, H0 = (torch.from_numpy(d[k]).to("cuda:0") for k in ("W", "data", "H0"))
    H, info = evc.solve_activations(A, X, H0, iters=50, info=True)
    assert H.data_ptr() != H0.data_ptr() and np.array_equal(H0.cpu().numpy(), d["H0"])     # the caller's start is intact
    return digest([H], info, "err")


CASES = {
    "cd_bin_major": lambda: cd("cdnmf_m25_n64_t32", "bin_major")[0],
    "cd_frame_major": lambda: cd("cdnmf_m25_n64_t32")[0],
    "cd_empty_utterance": cd_empty_utterance,
    "cd_m257_l1l2": lambda: cd("cdnmf_m257_n33_t9_l1l2")[0],
    "cd_f32": lambda: cd("cdnmf_m100_n47_t20_f32")[0],
    "cd_warm_start": cd_warm_start,
    "cd_trace_past_the_ring": cd_trace_past_the_ring,
    "cd_raw_workspace_plus_8": lambda: raw_shifted("evc_cd_solve"),
    "beta_reg_b0p5": beta_reg,
    "beta_early_stop": beta_early_stop,
    "beta_f32": lambda: beta("betamu_m25_n64_t32_b0_f32")[0],
    "beta_m513": lambda: beta("betamu_m513_n96_t21_b0")[0],
    "beta_m1": lambda: beta("betamu_m1_n48_t37_b0p5")[0],
    "beta_empty_utterance_sklearn": lambda: beta_empty_utterance("sklearn"),
    "beta_empty_utterance_const": lambda: beta_empty_utterance("const"),
    "beta_frame_major": lambda: beta("betamu_m25_n64_t32_k50_b0p5", "frame_major")[0],
    "beta_raw_workspace_plus_8": lambda: raw_shifted("evc_beta_solve"),
    "nmf_plain": nmf_plain,
    "nmf_utterances_sklearn_stop": nmf_utterances_sklearn_stop,
    "nmf_convert_no_h": nmf_convert_no_h,
    "nmf_prepared_with_b": nmf_prepared_with_b,
    "nmf_out_given": nmf_out_given,
    "nmf_h0_on_the_device": nmf_h0_on_the_device,
}

# printed by `tools/make_learn_digests.py test_gpu_solve_digests` on the commit before the drivers shared their skeleton
PARENT_DIGESTS = {
    "beta_early_stop": "2b387aa67d64bcb2867866ce3cd6167d7d79de189b315bfc85f1b4ec70e06e98",
    "beta_empty_utterance_const": "b40c508530228b5d7cf0097936a2e3dea350810daca381a71cd55f3a315e88e9",
    "beta_empty_utterance_sklearn": "c0e703d7ba239006bf0059e9bcb915a7e28211e62f01ab01ca023d74e276ab5a",
    "beta_f32": "852813e608aba5be6bfa1c9cd31aa63868e7903a9c07481ae01ce70167175add",
    "beta_frame_major": "7a69253e8091dd253fa3bed7067611ceb7d99b2c59bbd919fd5d5cf2c260c925",
    "beta_m1": "ba9fbcf0dfb1ee0374b99cfa059c3f2c85b346d9db10510697dbd400b3e5d3c9",
    "beta_m513": "e536cd3136bba4cccbb7059e8602c9a75907bc046db5792a7e95fe12672d154f",
    "beta_raw_workspace_plus_8": "ef5555295fcaf9d921ecbdc166e230f5b6168bbd14b121a46b1456fd93352180",
    "beta_reg_b0p5": "88510d8e5a3389e00aa07815c97f321344d920092a16dc2e5fe61d0ccbdb30b8",
    "cd_bin_major": "de94565388fa5252de747af7c5ebfc605402d309dc74c099b9d3a26370f7f362",
    "cd_empty_utterance": "d10ca30576763e927ac1aa79de8b08b4a6678dfd995bd962cd59a7ab222877f7",
    "cd_f32": "0fbe787712fb9fd82a4aea010b809730e5741f0b7282a1567a269d4d3ea61cee",
    "cd_frame_major": "c921f6c016cb005b2da82e3d20e0735785ef3187d0d927700b23835981cc9286",
    "cd_m257_l1l2": "ef9f35be1a84ba7602b9f5530b1ab6a80740873b09f13bcd50c2625d027edae2",
    "cd_raw_workspace_plus_8": "d67bba7d91ddb6b59eb0b9c98a2c6359a45005aa46fe464e945e105c4af42cbb",
    "cd_trace_past_the_ring": "30c1655fddba550d5fd421e97e85c5954b9bf304dfa20a05d4b0fc308d949147",
    "cd_warm_start": "497feab45d14f0df59e51f3b1bf60f9c8a135527ce636735660bc06eaf41211b",
    "nmf_convert_no_h": "47a994bed30bf112aa0e1c9f8f94113d9cf41d5308f5700adeebce7767530ce7",
    "nmf_h0_on_the_device": "48e32299b7117921bff4577bd081a20dde55528eabf8c23d31036b40f0b817cd",
    "nmf_out_given": "34cb460fdce4708fe56a562756af685b1f05274663ec675e0bea253bb463737e",
    "nmf_plain": "171b68771e53146b6a198778c852877e549dbb29d5b7f7428c909d1044007c52",
    "nmf_prepared_with_b": "31927187a7f818ac69e7247e41fb4adfae3e8b08cd3dfa8d2b4167213ed1a48f",
    "nmf_utterances_sklearn_stop": "41b9d4ba9d11900942306869530c2e5081e5f5539d297f44ccc767f6258ea740",
}


def test_every_case_is_pinned():
    assert sorted(PARENT_DIGESTS) == sorted(CASES)


def test_the_regularised_beta_case_is_the_digest_pinned_earlier():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_beta_learn
    assert PARENT_DIGESTS["beta_reg_b0p5"] == test_gpu_beta_learn.PARENT_DIGEST


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_bitwise_what_the_parent_gave(case):
    got = CASES[case]()
    print(case, got)
    assert got == PARENT_DIGESTS[case]
