"""The sparse family (evc_prox_solve, evc_prox_masked_solve, evc_prox_learn, evc_prox_masked_learn) and evc_semi_solve give
bit for bit what they gave before their host drivers came to share one skeleton: sha256 of the outputs,
n_iter (the learn entries: n_epochs, n_steps, the statistics and their count) and the whole trace, NaNs included, of the calls
below, recorded on the commit before that change by `tools/make_learn_digests.py test_gpu_prox_digests`, which runs CASES as
they stand here, twice each.  Every call reads a fixture of tests/golden; together they take the paths the shared code has.
The solves, without and with a mask: both layouts, float32, three utterances with the middle one empty of which one stops
early under the deComP rule while the other runs on, check_every = 0, no iterations from a constant and from a given start,
no frames, the Nesterov schedule, normalize off, the factored sweep without a mask, lip_weights "mean", an explicit
lipschitz, and through the C ABI a workspace that does not start at a multiple of 256 bytes.  The learn entries: both
layouts, float32, the order from a seed and none, an early stop, a batch size that does not divide T, a resume (2 epochs + 1
on the returned state: the digest of the 3-epoch call), nothing read back (info=False, tol = 0) and no epochs.  evc_semi_solve:
several utterances under the pymf stop rule, and check_every = 0."""
import hashlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def host(a):
    return np.ascontiguousarray(a if isinstance(a, np.ndarray) else a.cpu().numpy())


def digest(outs, counts=(), trace=None):
    h = hashlib.sha256()
    for a in outs:
        h.update(host(a).tobytes())
    h.update(np.ascontiguousarray(counts, dtype=np.int64).tobytes())
    if trace is not None:
        h.update(np.ascontiguousarray(trace, dtype=np.float64).tobytes())
    return h.hexdigest()


def oriented(layout):
    """the fixtures hold frames (and exemplars) as rows: frame_major as they are, bin_major transposed"""
    return (lambda a: a) if layout == "frame_major" else (lambda a: np.ascontiguousarray(a.T))


# ---- evc_prox_solve and evc_prox_masked_solve ----

def loaded(name):
    """the fixture as the family's own test modules load it (float64 operands, the method split into its options)"""
    if name.startswith("proxml_"):
        import test_gpu_prox_masked_learn as t
    elif name.startswith("proxl_"):
        import test_gpu_prox_learn as t
    elif name.startswith("proxm_"):
        import test_gpu_prox_masked as t
    else:
        import test_gpu_prox as t
    return t.load(name)


def prox(name, layout="frame_major", masked=None, x0=None, offs=None, **kw):
    """solve_activations_prox on the fixture (a proxm_ fixture: with its mask, unless masked=False) -> digest, info"""
    import exemplars_vc_amd as evc
    d = loaded(name)
    t = oriented(layout)
    masked = "mask" in d if masked is None else masked
    if masked:
        kw.setdefault("lip_weights", "mean")                      # deComP's choice, what the fixtures were recorded with
        kw["mask"] = t(d["mask"])
    kw.setdefault("iters", int(d["maxiter"]))
    H, info = evc.solve_activations_prox(t(d["A"]), t(d["y"]), None if x0 is None else t(x0), layout=layout,
                                         utt_offsets=offs, info=True, **dict(d["kw"], **kw))
    return digest([H], info["n_iter"], info["change"]), info


def prox_utterances(name):
    """three utterances, the middle one empty; the first stops early while the last runs on"""
    d = loaded(name)
    a, b = int(d["offs"][1]), int(d["offs"][2])
    dg, info = prox(name, "bin_major", offs=[0, a, a, b])
    n = info["n_iter"].tolist()
    assert n[0] < n[2] and n[0] < int(d["maxiter"]) and np.isnan(info["change"][1]).all()
    return dg


def prox_start(name, iters):
    d = loaded(name)
    x0 = np.random.default_rng(3).random(d["x"].shape) * 0.05
    return prox(name, x0=x0, iters=iters)[0]


def prox_cabi(name, frames=None, **kw):
    """the first `frames` frames through the C ABI as the entry's own test module calls it"""
    d = loaded(name)
    if "mask" in d:
        import test_gpu_prox_masked as t
        x, n_iter, tr = t.cabi(d["y"][:frames], d["A"], d["mask"][:frames], None, **kw)
    else:
        import test_gpu_prox as t
        x, n_iter, tr = t.cabi(d["y"][:frames], d["A"], None, **kw)
    return digest([x], n_iter, tr)


def raw_shifted(entry):
    """one raw call, float64, frame-major, the workspace 8 bytes past a multiple of 256"""
    import ctypes as C
    import torch
    from exemplars_vc_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    masked = entry == "evc_prox_masked_solve"
    d = loaded("proxm_m25_n64_t32_fista_pos_k50" if masked else "prox_m25_n64_t32_fista_pos_k50")
    A, X = (torch.from_numpy(d[k]).to(dev) for k in ("A", "y"))
    (T, M), N = X.shape, A.shape[0]
    H = torch.empty((T, N), dtype=torch.float64, device=dev)
    o = _lib.ProxMaskedOpts() if masked else _lib.ProxOpts()
    o.struct_bytes, o.dtype, o.layout, o.iters, o.check_every = C.sizeof(o), _lib.F64, _lib.FRAME_MAJOR, 12, 4
    o.mode, o.momentum, o.normalize, o.stop_rule, o.init_mode = (_lib.PROX_POSITIVE, _lib.PROX_FISTA, 1, _lib.STOP_DECOMP,
                                                                 _lib.INIT_CONST)
    o.alpha, o.tol, o.init_value = 1e-3, 0.0, 0.01
    mid = ()
    if masked:
        o.lip_weights = _lib.PROX_LIP_MAX
        mask = torch.from_numpy(d["mask"]).to(dev)
        mid = (mask.data_ptr(), mask.stride(0))
    nbytes = int(getattr(L, "evc_prox_masked_workspace_bytes" if masked else "evc_prox_workspace_bytes")(M, N, T, 1, _lib.F64))
    assert nbytes > 0
    buf = torch.empty(nbytes + 512, dtype=torch.uint8, device=dev)
    ws = (buf.data_ptr() + 255) // 256 * 256 + 8
    n_iter, trace = np.zeros(1, dtype=np.int32), np.zeros((1, 3))
    with torch.cuda.device(dev):
        st = getattr(L, entry)(A.data_ptr(), A.stride(0), X.data_ptr(), X.stride(0), *mid, H.data_ptr(), H.stride(0), M, N, T,
                               None, 1, C.byref(o), ws, nbytes, n_iter.ctypes.data_as(C.POINTER(C.c_int)),
                               trace.ctypes.data_as(C.POINTER(C.c_double)),
                               C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    _lib.check(st, entry)
    torch.cuda.synchronize()
    return digest([H], n_iter, trace)


P, PM = "prox_m25_n64_t32_fista_pos_k50", "proxm_m25_n64_t32_fista_pos_k50"


def solve_cases(tag, k50, m1, m201, stops):
    """the paths both solve drivers have; `stops`: a fixture with recorded utterances that stop at different iterations"""
    return {
        tag + "_frame_major": lambda: prox(k50)[0],
        tag + "_bin_major": lambda: prox(k50, "bin_major")[0],
        tag + "_m1": lambda: prox(m1)[0],
        tag + "_m201": lambda: prox(m201, "bin_major")[0],
        tag + "_m201_f32": lambda: prox(m201, dtype="f32", iters=60)[0],
        tag + "_utterances_one_stops": lambda: prox_utterances(stops),
        tag + "_check_every_0": lambda: prox(k50, check_every=0)[0],
        tag + "_iters_0_const": lambda: prox(k50, iters=0)[0],
        tag + "_iters_0_given": lambda: prox_start(k50, 0),
        tag + "_given_start": lambda: prox_start(k50, 23),
        tag + "_iters_0_const_value": lambda: prox_cabi(k50, iters=0, init_value=0.25, layout="bin_major", pad=3),
        tag + "_no_frames": lambda: prox_cabi(k50, frames=0, iters=20, tol=1e-3),
        tag + "_nesterov": lambda: prox(k50, momentum="nesterov", check_every=7)[0],
        tag + "_ista_signed": lambda: prox(k50, momentum="ista", positive=False, iters=30)[0],
        tag + "_no_normalize": lambda: prox(k50, normalize=False)[0],
        tag + "_lipschitz": lambda: prox(k50, lipschitz=40.0)[0],
        tag + "_raw_workspace_plus_8": lambda: raw_shifted("evc_prox_masked_solve" if tag == "pm" else "evc_prox_solve"),
    }


# ---- evc_prox_learn and evc_prox_masked_learn ----

def learn(name, layout="frame_major", state=None, start=None, epochs=None, info=True, **kw):
    """learn_dictionary_sparse on the fixture (a proxml_ fixture: with its mask) -> D, H, info (None without info)"""
    import exemplars_vc_amd as evc
    d = loaded(name)
    t = oriented(layout)
    kw = dict(d["kw"], **kw)
    if epochs is not None:
        kw["epochs"] = epochs
        if kw.get("order") is not None:
            kw["order"] = kw["order"][:epochs]
    if "mask" in d:
        kw["mask"] = t(d["mask"])
    D0, H0 = (t(d["D0"]), None if "x0" not in d else t(d["x0"])) if start is None else start
    out = evc.learn_dictionary_sparse(t(d["y"]), D0, H0, layout=layout, state=state, info=info, **kw)
    return out if info else (*out, None)


def learn_digest(D, H, info):
    state = info["state"]
    return digest([D, H, *state[:-1]], [info["n_epochs"], info["n_steps"], state[-1]], info["change"])


def learn_case(name, layout="frame_major", **kw):
    return learn_digest(*learn(name, layout, **kw))


def learn_stop(name):
    d = loaded(name)
    D, H, info = learn(name, epochs=int(d["it"]) + 3)
    assert info["n_epochs"] == int(d["it"]) and info["n_steps"] == int(d["n_steps"]) and np.isnan(info["change"][-1])
    return learn_digest(D, H, info)


def learn_resume(name):
    """2 epochs, then 1 on the returned dictionary, activations and state with the third row of the order, tol = 0: the
    call of 3 epochs"""
    order = loaded(name)["order"]
    D, H, first = learn(name, epochs=2, tol=0.0)
    D, H, second = learn(name, start=(D, H), state=first["state"], epochs=1, tol=0.0, order=order[2:3])
    whole = dict(second, n_epochs=first["n_epochs"] + second["n_epochs"], n_steps=first["n_steps"] + second["n_steps"],
                 change=np.concatenate([first["change"], second["change"]]))
    return learn_digest(D, H, whole)


def learn_nothing_read_back(name):
    D, H, info = learn(name, info=False)
    assert info is None
    return digest([D, H])


PL, PML = "proxl_m201_n96_t150_fista_pos_k3", "proxml_m25_n40_t130_fista_pos_k4"

CASES = {
    **solve_cases("p", P, "prox_m1_n5_t3_fista_pos", "prox_m201_n300_t20_fista_pos", "prox_m40_n130_t33_ista_pos"),
    **solve_cases("pm", PM, "proxm_m1_n5_t3_fista_pos", "proxm_m201_n300_t20_fista_pos", "proxm_m201_n300_t20_fista_pos"),
    "p_m40_ista": lambda: prox("prox_m40_n130_t33_ista_pos")[0],
    "pm_factored_no_mask": lambda: prox(PM, masked=False, factored=True)[0],
    "pm_factored_no_mask_bin_major": lambda: prox(P, "bin_major", factored=True)[0],
    "pm_lip_max": lambda: prox(PM, lip_weights="max")[0],
    "pm_lip_max_utterances": lambda: prox("proxm_m201_n300_t20_fista_pos", lip_weights="max", offs=[0, 10, 20], iters=60)[0],
    "pl_stops_early": lambda: learn_stop("proxl_m25_n40_t130_fista_pos_stop"),
    "pl_signed_bs_not_dividing": lambda: learn_case("proxl_m5_n3_t101_fista", epochs=5),
    "pl_m201": lambda: learn_case(PL),
    "pl_m201_bin_major": lambda: learn_case(PL, "bin_major"),
    "pl_m201_f32": lambda: learn_case(PL, dtype="f32"),
    "pl_order_none": lambda: learn_case(PL, order=None),
    "pl_order_from_seed": lambda: learn_case(PL, order=None, seed=330),
    "pl_three_epochs": lambda: learn_case("proxl_m25_n40_t130_fista_pos_stop", epochs=3, tol=0.0),
    "pl_resume_two_plus_one": lambda: learn_resume("proxl_m25_n40_t130_fista_pos_stop"),
    "pl_nothing_read_back": lambda: learn_nothing_read_back(PL),
    "pl_no_epochs": lambda: learn_case(PL, epochs=0),
    "pml_k4": lambda: learn_case(PML),
    "pml_k4_bin_major": lambda: learn_case(PML, "bin_major"),
    "pml_k4_f32": lambda: learn_case(PML, dtype="f32"),
    "pml_holes": lambda: learn_case("proxml_m12_n10_t64_holes_k3"),
    "pml_m1": lambda: learn_case("proxml_m1_n5_t12_k4"),
    "pml_order_none": lambda: learn_case(PML, order=None),
    "pml_order_from_seed": lambda: learn_case(PML, order=None, seed=510),
    "pml_stops_early": lambda: learn_case(PML, tol=0.05),
    "pml_resume_two_plus_one": lambda: learn_resume(PML),
    "pml_nothing_read_back": lambda: learn_nothing_read_back(PML),
    "pml_no_epochs": lambda: learn_case(PML, epochs=0),
}


# ---- evc_semi_solve ----

def semi(name, offs=None, **kw):
    import exemplars_vc_amd as evc
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    H, info = evc.solve_activations_semi(d["W"], d["data"], d["H0"], iters=int(d["niter"]), utt_offsets=offs, info=True, **kw)
    return digest([H], info["n_iter"], info["err"]), info


def semi_utterances_pymf_stop():
    """three utterances, the middle one empty, under the pymf rule at a tolerance the numpy restatement (tests/semi_restatement.py)
    passes after 50 and 51 updates, 0.3 % and 0.7 % away from the statistic"""
    dg, info = semi("snmf_m40_n130_t33_k100", offs=[0, 16, 16, 33], check_every=1, stop_rule="pymf", tol=1e-2)
    assert info["n_iter"].tolist() == [50, 100, 51]
    return dg


CASES["semi_utterances_pymf_stop"] = semi_utterances_pymf_stop
CASES["semi_check_every_0"] = lambda: semi("snmf_m25_n64_t32_k50")[0]

# printed by `tools/make_learn_digests.py test_gpu_prox_digests` on the commit before the drivers shared their skeleton
PARENT_DIGESTS = {
    "p_bin_major": "75fb204baac323ec46b46eaba5e2d8e6f0d272476e11e6ecef94c8d81e3ade8c",
    "p_check_every_0": "c0fb502e3ae61446c9fa7eaafbc2252f1a3df315bce9feea90d87343efead10a",
    "p_frame_major": "04bfffbc46e1b5b06beaabb2898c7d5f8c257b749a1826bb3130b8024ea516cf",
    "p_given_start": "1d4384511592e49fd4eede437db3d81dc914f00b30f00062f44f22b23586c071",
    "p_ista_signed": "9f8711b51a935bd6fb77c3e0afe13422c432511aad8e8dc36b2cb43e5ee64ac2",
    "p_iters_0_const": "f3e70dac36eb1b853d669f00f457c97c2f37cb5d8ae245305d05d661439365a7",
    "p_iters_0_const_value": "d1f8023a42b4f17decd8b1171a87bfa357700e3656a646a0bbb8988555decb2d",
    "p_iters_0_given": "0b4f7b5c07f6b174f7094fcdb8d1badddcb1a4b485ac111740ad5a1a0d7356da",
    "p_lipschitz": "f45c4e7efdc170a1a338b5e5cfda6e715fe332286f95887078680c9f951c9998",
    "p_m1": "020d3d6a24e25e9e63bdc1064c06d32df97ebe625de285455876fb6bc6be293f",
    "p_m201": "5f0ed0bac150d77cb7fac113fab5ad7d997d17838e159ed83d2a03c0cead16ad",
    "p_m201_f32": "63d48f735cdb7986e2a63dc34ee7c193ce853c008e9e2e62b8359fe8026a2c95",
    "p_m40_ista": "6cc745e9ae94e485d9274553e3d31c9f78be0250b20683046131d3fb65da2bf7",
    "p_nesterov": "34968ff6782ee538a145f3fc5dab2d2c532c09a17cfa2b42db7829be93bba9ac",
    "p_no_frames": "f089717fe4c8b256e4ee83ff8d1dcdaa2fe0ee5fbf20f9d693de90b7390d5caf",
    "p_no_normalize": "934f8ef58fb0ac623bc72fbacd077273d8e62603ccbb6a50d5445100fe33532a",
    "p_raw_workspace_plus_8": "3a029da5da16e3e44f78ba84242a2a99e740af05fa4f1510803dcd37a4107eeb",
    "p_utterances_one_stops": "5174106768b4c278de797ea51583a7e1e63928dc7dcdd7d94c839bc195a5b359",
    "pl_m201": "e724bdc85df84071fc32379d97f093c0dad9d49daa5fffc7ec7618ff0c6f842e",
    "pl_m201_bin_major": "1c42ba66f52f89a82331be51b3f4ca0f35f9e95f34efd2a103dc0910ebe8eaaa",
    "pl_m201_f32": "d9d94aee15b56ee67758351e68e6f7305ddc05f96e2cc94e6c7fba218297f250",
    "pl_no_epochs": "9b3986ada55bab9ae9c02ce76129b7ef6c8872f938aef3d103202c1a0bab2553",
    "pl_nothing_read_back": "9302b653c3a1e30af142fa0043cdc24762cc0510c604ad4168469cd4e60c8644",
    "pl_order_from_seed": "e724bdc85df84071fc32379d97f093c0dad9d49daa5fffc7ec7618ff0c6f842e",
    "pl_order_none": "1d368c608b0fff58789c98e5a13077ddcb84ea3c7804ae4a22c543cbfae057d1",
    "pl_resume_two_plus_one": "4f67165e2bd17b69d7885c2be5c4b43dd656a0e92d34836d1dab511632de2e3c",
    "pl_signed_bs_not_dividing": "0a9f4ace2a8d6e681c0d0a7dee8cd5c848b192bfd145d864dc647cd8ad3926a3",
    "pl_stops_early": "8281a1662c98dc7decae31d75476f686b90402f9867e8d06af9ce0e2d0e4c92e",
    "pl_three_epochs": "4f67165e2bd17b69d7885c2be5c4b43dd656a0e92d34836d1dab511632de2e3c",
    "pm_bin_major": "0b0249490bbe4ea75ede30c07141cef3596e8a1915e1a5d579b4efd0da456ee6",
    "pm_check_every_0": "2098c021040cf60f4f211c6654f328f34851a0b5a728193a7c4b00b181d5426c",
    "pm_factored_no_mask": "9116aa6a2ec3e35b72993036f9042ba3ab154669fd6eaa960208f2d11fd8d249",
    "pm_factored_no_mask_bin_major": "1c43373c72e310eaa79397a4b6c6e63184fbc88e5b314d0696c32f01d77b776a",
    "pm_frame_major": "7f4c29fdad06ae48364b5d7412fb22d4c98334556e7508e9323cf7fb75ea97c6",
    "pm_given_start": "bb58c0a4c79709bbdabfd85f113155d9863e3dfcafa9bb07dd272bbc8976f696",
    "pm_ista_signed": "0c3268c0716bfce49f9c3f17268bf6ad5a4a93606c330e6b157fda28eeb31b9d",
    "pm_iters_0_const": "f3e70dac36eb1b853d669f00f457c97c2f37cb5d8ae245305d05d661439365a7",
    "pm_iters_0_const_value": "d1f8023a42b4f17decd8b1171a87bfa357700e3656a646a0bbb8988555decb2d",
    "pm_iters_0_given": "0b4f7b5c07f6b174f7094fcdb8d1badddcb1a4b485ac111740ad5a1a0d7356da",
    "pm_lip_max": "0169207918499d2f0630186a477e0aab36f6295d8ff4d389d97cc57da8afde00",
    "pm_lip_max_utterances": "af94769662ae8fdabaf1f7081ce1c55b6e841b40c237e6544f7fb106636ca23c",
    "pm_lipschitz": "9256fa52dad9ebed286edee3fc51ec96d65b7f4f9bf85040583a32f81e19ce5f",
    "pm_m1": "300976096edff7d04b147471f555fa35381bc3b0b54aeae4dfb6527fb1a75d5e",
    "pm_m201": "2d029fd8a6b012629a7b84230e862b84fc32f30c75dfae9becf52b82686c29cb",
    "pm_m201_f32": "51c6c0aceea9321c2da2b5ac6e449754ac62f535b318f60b1becf082d7b05536",
    "pm_nesterov": "67014c93735b10b13305c80ee00035bb820e36f27de933e705131ca89db96763",
    "pm_no_frames": "f089717fe4c8b256e4ee83ff8d1dcdaa2fe0ee5fbf20f9d693de90b7390d5caf",
    "pm_no_normalize": "aa7406def7eb440834ac3b4be5b8a68ed62ce8c4fa17c6402ef1168af5138cf1",
    "pm_raw_workspace_plus_8": "085a1273d40c7293ec86e04babd7ff5cf923d3a5d39352e18f572ef341faf3c5",
    "pm_utterances_one_stops": "498492e52939fa9f317b761b387a0bfc6830d4c8b1a149197717d9ce54f67a85",
    "pml_holes": "8a2857e29bd0192d3a281da64da6a6c07d5a066b7206421a465140a28ebd1a34",
    "pml_k4": "72f5f4ce6db964a87208976599550f579a717f586abc14abdcab015b19bb7f9e",
    "pml_k4_bin_major": "dfd5bdc240fc582c5774a85220e867b4206c568cb7dc01d5e6f5b60411d85f2d",
    "pml_k4_f32": "6e805474f293493579c501aed43119bdf9ce05c57fa6ebb9a2e150bacd4e77b7",
    "pml_m1": "a4fcc36dc802291892aea1267e7861ce07253ced585fea5f57cbac95b982cd70",
    "pml_no_epochs": "a4754491f595e0523cd0a5deaa16f87400e5bdbe6ec3c874736ad3ce1f151ff2",
    "pml_nothing_read_back": "9cbda07ee62f6a7ebde8fe58713c002d75c7acd681b97a6a927265f6651dc5ac",
    "pml_order_from_seed": "72f5f4ce6db964a87208976599550f579a717f586abc14abdcab015b19bb7f9e",
    "pml_order_none": "82879a696c969466db7a7ba86c8da9f4fbfbf677ff4b3968618ca46098db378d",
    "pml_resume_two_plus_one": "72f5f4ce6db964a87208976599550f579a717f586abc14abdcab015b19bb7f9e",
    "pml_stops_early": "c38d7b1099b8d8b361e5a167c31ee6ff8d84ad287056f82625f0259a3df758fd",
    "semi_check_every_0": "6d242e82a2b4c4427436780a2384d1576bce61ad80b538e7bd82df0a67bf6a77",
    "semi_utterances_pymf_stop": "3922dd4f96e14b792c8bd2f74e55c60f0c25d9a9bd5a4c945e29e8eeeaeb039e",
}


def test_every_case_is_pinned():
    assert sorted(PARENT_DIGESTS) == sorted(CASES)


def test_a_resume_is_pinned_to_the_whole_calls_digest():
    assert PARENT_DIGESTS["pl_resume_two_plus_one"] == PARENT_DIGESTS["pl_three_epochs"]
    assert PARENT_DIGESTS["pml_resume_two_plus_one"] == PARENT_DIGESTS["pml_k4"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_bitwise_what_the_parent_gave(case):
    got = CASES[case]()
    print(case, got)
    assert got == PARENT_DIGESTS[case]
