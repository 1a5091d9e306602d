"""k_fused_wide (evc_wide.hip) step by step against the float64 oracle trajectory (oracle.mu_trajectory).

The other float32 tests compare after 20 to 150 iterations at rtol 2e-3 or more, where the multiplicative update has
damped a mid-solve error away: a solve in which every frame reads V one iteration late passes them.  Here K <= 20 and
the check is rtol 1e-4 with an absolute floor of 1e-6 max|H_K| (float32 against float64 stays below ~2e-5 at these K;
successive iterates differ by 1e-3 to 1e-1), and every case shows that the check can see one iteration of difference:
the oracle's H_{K-1} fails it.  A reader that used a partial sum one iteration old, a launch that restarted from the
wrong epoch or slot parity, or a stopped utterance that got the wrong snapshot back fails here.

Every case enters through evc.solve_activations / evc.convert on float32 inputs and asserts the kernel, the template
instance and schedule that ran (evc_solve_info.variant) and redo == 0 (a solve whose wait ran out is redone silently on
the two contractions).  The schedule follows from G = ceil(frame tiles / W) groups of W wavefronts, c exemplar ranges
(forced with fused_c, fused_w) and the CU count (evc_wide.hip, wide_layout / wide_variant):
    static        G c <= CUs, c <= 4           workgroup b runs task b of every iteration, counters
    tagged        G c <= CUs, c > 4            the same with reduce slices; the epoch bit rides in the data
    ticket        G c > CUs,  c <= 8           ticket queue, counters
    ticket_reduce G c > CUs,  c > 8            ticket queue with reduce tasks (c > 8 only for <= 256 frame tiles)
test_wide_instance_inventory (CPU) holds INSTANCES against the template instances in the built library."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
RTOL, AFLOOR = 1e-4, 1e-6
MT_SET = (4, 6, 8, 10, 13)
SK_EPS = float(np.finfo(np.float32).eps)
EPS = {"add": 1e-9, "zero_replace": SK_EPS, "none": 0.0, "clamp": 1e-15}


def oracle():
    from oracle import evc_oracle as o
    return o


def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def schedule(M, N, T, w, c, n_cus=256):
    """(schedule name, variant dict) that wide_layout / wide_variant give for forced c and w"""
    mt = next(v for v in MT_SET if 16 * v >= M)
    NB, TT = -(-N // 16), -(-T // 16)
    G = -(-TT // w)
    c = min(c, max(1, NB // 2), 64)
    static = G * c <= n_cus
    reduce = c > 8 or (c > 4 and static)
    name = ("tagged" if reduce else "static") if static else ("ticket_reduce" if reduce else "ticket")
    return name, c, {"static": static, "reduce": reduce, "tagged": reduce and static, "w": w, "mt": mt}


def launch_starts(K, ce, stop_rule, slots=4):
    """first iteration of every launch of a float32 wide solve (evc_api.hip, solve_wide: up to 1 + slots checks per
    launch, 1, 1, 2, 3 ... of them as the solve goes on; iteration 0 forms P and V = A H0)"""
    starts, nxt = [], 0

    def run_to(e):
        nonlocal nxt
        if e > nxt:
            starts.append(nxt)
            nxt = e
    if ce > 0 and stop_rule == "sklearn":
        run_to(1)
    done = 0
    while done < K:
        n = K - done
        if ce > 0 and n >= ce:
            n = min(1 + done // (2 * ce), 1 + slots, n // ce) * ce
        run_to(done + n + 1)
        done += n
    run_to(1)
    return starts


def score(got, want):
    """max |got - want| / max(|want|, 1e-6 max|want|) over the finite entries of want; inf when the NaN / inf patterns
    differ"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if not (np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))):
        return float("inf")
    fin = np.isfinite(want)
    if not fin.any():
        return 0.0
    floor = AFLOOR * float(np.abs(want[fin]).max())
    return float(np.max(np.abs(got[fin] - want[fin]) / np.maximum(np.abs(want[fin]), floor)))


def check_step(name, got, traj, K, extra=""):
    """got matches H_K at RTOL and (K >= 2) H_{K-1} does not: the check sees one iteration"""
    e = score(got, traj[K - 1])
    margin = score(traj[K - 2], traj[K - 1]) if K >= 2 else float("nan")
    print(f"STEPS {name} K={K} err={e:.3e} one_iteration={margin:.3e} {extra}")
    assert e <= RTOL, (name, e)
    if K >= 2:
        assert margin > RTOL, (name, margin)
    return e


def assert_ran(info, variant, members=None, launches=None):
    assert info["kernel"] == "k_fused_wide" and info["redo"] == 0, info
    assert info["variant"] == variant, (info["variant"], variant)
    if members is not None:
        assert info["members"] == members, info
    if launches is not None:
        assert info["launches"] == launches, info


def problem(M, N, T, seed, Mb=None):
    o = oracle()
    p = o.synth_problem(M, N, T, Mb=Mb, seed=seed)
    return (p["A"].astype(np.float32), p["X"].astype(np.float32), p["B"].astype(np.float32))


def solve(A, X, H0=None, B=None, layout="bin_major", **kw):
    """one call in either orientation (bins-as-rows arrays in, bins-as-rows float64 out): H, Y (or None), info"""
    import exemplars_vc_amd as evc
    tr = (lambda z: z) if layout == "bin_major" else (lambda z: None if z is None else np.ascontiguousarray(z.T))
    if B is None:
        H, info = evc.solve_activations(tr(A), tr(X), tr(H0), layout=layout, info=True, **kw)
        Y = None
    else:
        H, Y, info = evc.convert(tr(A), tr(X), tr(B), tr(H0), layout=layout, info=True, **kw)
    assert H.dtype == np.float32
    back = (lambda z: z) if layout == "bin_major" else (lambda z: None if z is None else z.T)
    return back(H).astype(np.float64), (None if Y is None else back(Y).astype(np.float64)), info


# ---------------------------------------------------------------------------------------------------------------------
# a. every instance (MT x W x tagged) at M on both sides of each bin-tile edge, the four schedules
# ---------------------------------------------------------------------------------------------------------------------
# (M, N, T, W, c, schedule, K, layout, start, l1, with Y = B H)
MATRIX = [
    (33, 256, 300, 4, 6, "tagged", 1, "bin_major", "const", 0.0, False),
    (33, 280, 4090, 8, 9, "ticket_reduce", 2, "frame_major", "given", 0.5, False),
    (64, 256, 300, 8, 5, "tagged", 3, "frame_major", "const", 0.0, True),
    (64, 200, 4090, 4, 5, "ticket", 4, "bin_major", "given", 0.0, False),
    (65, 300, 300, 4, 7, "tagged", 5, "bin_major", "given", 0.3, False),
    (65, 256, 300, 8, 2, "static", 9, "frame_major", "const", 0.0, False),
    (96, 256, 300, 8, 8, "tagged", 9, "bin_major", "const", 0.0, True),
    (96, 280, 4090, 4, 9, "ticket_reduce", 1, "frame_major", "given", 0.0, False),
    (97, 256, 300, 4, 6, "tagged", 2, "frame_major", "const", 0.0, False),
    (97, 160, 8190, 8, 5, "ticket", 3, "bin_major", "const", 0.0, False),
    (128, 400, 300, 8, 12, "tagged", 4, "bin_major", "given", 0.0, False),
    (128, 256, 300, 4, 3, "static", 5, "frame_major", "const", 0.2, True),
    (129, 256, 300, 4, 5, "tagged", 9, "bin_major", "const", 0.0, False),
    (129, 290, 4090, 8, 9, "ticket_reduce", 1, "bin_major", "given", 0.0, True),
    (160, 256, 300, 8, 6, "tagged", 2, "frame_major", "given", 0.0, False),
    (160, 256, 300, 4, 4, "static", 3, "bin_major", "const", 0.0, False),
    (161, 256, 300, 4, 8, "tagged", 4, "frame_major", "const", 0.0, False),
    (161, 300, 4090, 8, 9, "ticket_reduce", 5, "frame_major", "const", 0.4, False),
    (201, 256, 300, 8, 5, "tagged", 9, "bin_major", "given", 0.0, True),
    (201, 256, 4090, 4, 5, "ticket", 3, "frame_major", "const", 0.0, False),
    (201, 256, 300, 8, 1, "static", 2, "bin_major", "const", 0.0, False),
    (208, 288, 4090, 4, 9, "ticket_reduce", 9, "bin_major", "given", 0.0, False),
    (208, 256, 300, 8, 7, "tagged", 1, "frame_major", "const", 0.0, True),
    (208, 256, 300, 4, 2, "static", 5, "frame_major", "given", 0.1, False),
]
# k_fused_wide64<TPW> instances the non-finite cases run: (M, TPW), the narrowest instance that holds M (64 TPW + 16 >= M)
WIDE64_CASES = ((201, 3), (257, 4), (320, 5), (400, 7), (513, 8))


def _instances():
    out = set()
    for M, N, T, w, c, _, *_ in MATRIX:
        v = schedule(M, N, T, w, c)[2]
        out.add((v["mt"], w, v["tagged"]))
    return out


INSTANCES = {"k_fused_wide": _instances(), "k_fused_wide64": {(t,) for _, t in WIDE64_CASES}}


def _start(kind, N, T, seed):
    if kind == "const":
        return None, dict(init="const", init_value=0.0123), np.full((N, T), np.float64(np.float32(0.0123)))
    H0 = (np.random.default_rng(seed).random((N, T)) * 0.05 + 1e-4).astype(np.float32)
    return H0, dict(init="given"), H0.astype(np.float64)


@pytest.mark.parametrize("M,N,T,w,c,sched,K,layout,start,l1,conv", MATRIX,
                         ids=[f"M{m[0]}-W{m[3]}-c{m[4]}-{m[5]}-K{m[6]}" for m in MATRIX])
def test_wide_matrix_step_by_step(M, N, T, w, c, sched, K, layout, start, l1, conv):
    o = oracle()
    name, c_eff, variant = schedule(M, N, T, w, c, cus())
    assert name == sched, (name, sched)
    A, X, B = problem(M, N, T, seed=M * 7 + T)
    H0, kw, H0_64 = _start(start, N, T, seed=M)
    H, Y, info = solve(A, X, H0, B if conv else None, layout=layout, iters=K, eps_mode="zero_replace", l1=l1,
                       fused_c=c, fused_w=w, **kw)
    assert_ran(info, variant, members=c_eff, launches=1)
    traj, _ = o.mu_trajectory(A.astype(np.float64), X.astype(np.float64), H0_64, K, o.EPS_ZERO_REPLACE, SK_EPS, l1)
    check_step(f"a/{sched}/M{M}/W{w}", H, traj, K)
    if conv:
        e = score(Y, B.astype(np.float64) @ traj[K - 1])
        print(f"STEPS a/{sched}/M{M}/W{w}/Y err={e:.3e}")
        assert e <= RTOL, e


KL_CASES = [(201, 256, 300, 8, 6, 4), (150, 256, 4090, 4, 5, 3), (100, 280, 4090, 8, 9, 5), (201, 256, 300, 4, 3, 2)]


@pytest.mark.parametrize("M,N,T,w,c,K", KL_CASES)
def test_wide_kl_step_by_step(M, N, T, w, c, K):
    o = oracle()
    name, c_eff, variant = schedule(M, N, T, w, c, cus())
    A, X, _ = problem(M, N, T, seed=M + 2 * T)
    H, _, info = solve(A, X, layout="frame_major", iters=K, eps_mode="zero_replace", loss="kl", init="const",
                       init_value=0.02, fused_c=c, fused_w=w)
    assert_ran(info, variant, members=c_eff, launches=1)
    traj, _ = o.mu_trajectory(A.astype(np.float64), X.astype(np.float64),
                              np.full((N, T), np.float64(np.float32(0.02))), K, o.EPS_ZERO_REPLACE, SK_EPS, loss="kl")
    check_step(f"a/kl/{name}/M{M}", H, traj, K)


@pytest.mark.parametrize("eps_mode", ["add", "zero_replace", "none", "clamp"])
@pytest.mark.parametrize("T,w,c", [(300, 8, 6), (4090, 4, 5), (300, 4, 2)])
def test_wide_eps_modes_with_zero_frames(eps_mode, T, w, c):
    """frames of X that are all zero: P = 0, then H = 0 and a zero denominator from the second iteration on (NONE: 0/0)"""
    o = oracle()
    M, N, K = 150, 256, 5
    name, c_eff, variant = schedule(M, N, T, w, c, cus())
    A, X, _ = problem(M, N, T, seed=T + c)
    zero = [0, 3, 40, T - 1]
    X[:, zero] = 0.0
    H, _, info = solve(A, X, iters=K, eps_mode=eps_mode, eps=EPS[eps_mode], init="const", init_value=0.03,
                       fused_c=c, fused_w=w)
    assert_ran(info, variant, members=c_eff, launches=1)
    mode = {"add": o.EPS_ADD, "zero_replace": o.EPS_ZERO_REPLACE, "none": o.EPS_NONE, "clamp": o.EPS_CLAMP}[eps_mode]
    traj, _ = o.mu_trajectory(A.astype(np.float64), X.astype(np.float64), np.full((N, T), np.float64(np.float32(0.03))),
                              K, mode, EPS[eps_mode])
    want = traj[K - 1]
    assert (np.isnan(want[:, zero]).all() if eps_mode == "none" else (want[:, zero] == 0).all())
    check_step(f"a/eps-{eps_mode}/{name}", H, traj, K)


# ---------------------------------------------------------------------------------------------------------------------
# b. launch boundaries: checks that never stop anyone, so launches start at every iteration residue mod 4 (slot parity
#    it & 1, epoch bit (it >> 1) & 1) on the tagged static schedule and on a ticket schedule
# ---------------------------------------------------------------------------------------------------------------------
BOUNDARY = [("tagged", 201, 256, 300, 8, 6), ("ticket", 201, 256, 4090, 4, 5), ("ticket_reduce", 100, 300, 4090, 8, 9)]


@pytest.mark.parametrize("ce", [1, 2, 3])
@pytest.mark.parametrize("sched,M,N,T,w,c", BOUNDARY)
def test_wide_launch_boundaries(sched, M, N, T, w, c, ce):
    o = oracle()
    K = 20
    name, c_eff, variant = schedule(M, N, T, w, c, cus())
    assert name == sched
    A, X, _ = problem(M, N, T, seed=ce + T)
    h0 = 0.011
    H, _, info = solve(A, X, iters=K, eps_mode="zero_replace", init="const", init_value=h0, check_every=ce,
                       stop_rule="sklearn", tol=-1e300, fused_c=c, fused_w=w)
    starts = launch_starts(K, ce, "sklearn")
    if ce == 1:
        assert {s % 4 for s in starts} == {0, 1, 2, 3}, starts
    assert_ran(info, variant, members=c_eff, launches=len(starts))
    assert int(info["n_iter"][0]) == K
    A64, X64, H0 = A.astype(np.float64), X.astype(np.float64), np.full((N, T), np.float64(np.float32(h0)))
    traj, res = o.mu_trajectory(A64, X64, H0, K, o.EPS_ZERO_REPLACE, SK_EPS)
    check_step(f"b/{sched}/ce{ce}", H, traj, K, extra=f"starts={starts}")
    want_err = np.concatenate([[o.residual_fro(A64, X64, H0)], res[ce - 1::ce]])
    err = info["err"][0]
    assert err.shape == want_err.shape and np.isfinite(err).all(), (err, want_err)
    e = float(np.max(np.abs(err - want_err) / want_err))
    print(f"STEPS b/{sched}/ce{ce}/err err={e:.3e}")
    assert e <= RTOL, (err, want_err)


# ---------------------------------------------------------------------------------------------------------------------
# c. stops: one utterance stops at iteration 3, a check inside the launch [3, 5) (its snapshot is restored), while a
#    tile-mate and a third utterance go on; pymf's rule (|err - err_prev| / T_u < tol from the third check on) with the
#    first utterance's frames scaled by 1e-3 separates the two with a wide margin
# ---------------------------------------------------------------------------------------------------------------------
STOPS = [("tagged", 397, 8, 6, [0, 37, 149, 397]), ("tagged", 397, 8, 6, [0, 141, 300, 397]),
         ("ticket", 4090, 4, 5, [0, 37, 2100, 4090]), ("ticket", 4090, 4, 5, [0, 141, 2100, 4090])]


def pymf_stops(res_by_utt, sizes, tol, K):
    """n_iter per utterance under pymf's rule evaluated every iteration (evc_aux.hip k_utt_check, c >= 3)"""
    out = []
    for r, n in zip(res_by_utt, sizes):
        it = K
        for c in range(3, K + 1):
            if abs(r[c - 1] - r[c - 2]) / n < tol:
                it = c
                break
        out.append(it)
    return out


@pytest.mark.parametrize("sched,T,w,c,offs", STOPS, ids=[f"{s[0]}-{s[4][1]}" for s in STOPS])
def test_wide_stops_inside_a_launch(sched, T, w, c, offs):
    o = oracle()
    M, N, K = 201, 256, 12
    name, c_eff, variant = schedule(M, N, T, w, c, cus())
    assert name == sched
    A, X, _ = problem(M, N, T, seed=offs[1] + T)
    X[:, :offs[1]] *= np.float32(1e-3)
    n_utt = len(offs) - 1
    sizes = [offs[u + 1] - offs[u] for u in range(n_utt)]
    A64, X64 = A.astype(np.float64), X.astype(np.float64)
    H0 = np.concatenate([np.full((N, sizes[u]), np.float64(np.float32(np.sqrt(X64[:, offs[u]:offs[u + 1]].mean() / N))))
                         for u in range(n_utt)], axis=1)
    traj, _ = o.mu_trajectory(A64, X64, H0, K, o.EPS_ZERO_REPLACE, SK_EPS)
    res = [[o.residual_fro(A64, X64[:, offs[u]:offs[u + 1]], traj[k][:, offs[u]:offs[u + 1]]) for k in range(K)]
           for u in range(n_utt)]
    crit = [[abs(r[k] - r[k - 1]) / n for k in range(2, K)] for r, n in zip(res, sizes)]
    lo, hi = crit[0][0], min(min(cr) for cr in crit[1:])
    tol = float(np.sqrt(lo * hi))
    assert lo * 1.1 < tol < hi / 1.1, (lo, hi)          # 10 % margin on both sides
    want_n = pymf_stops(res, sizes, tol, K)
    assert want_n == [3] + [K] * (n_utt - 1), want_n
    H, _, info = solve(A, X, iters=K, eps_mode="zero_replace", init="sklearn", check_every=1, stop_rule="pymf", tol=tol,
                       utt_offsets=offs, fused_c=c, fused_w=w)
    starts = launch_starts(K, 1, "pymf")
    assert 3 in starts and 5 in starts                  # the stop at 3 is the first check of the launch [3, 5)
    assert_ran(info, variant, members=c_eff, launches=len(starts))
    assert list(info["n_iter"]) == want_n, (list(info["n_iter"]), want_n)
    s0 = slice(offs[0], offs[1])
    e = score(H[:, s0], traj[2][:, s0])
    print(f"STEPS c/{sched}/{offs[1]} stopped err={e:.3e} vs H2={score(traj[1][:, s0], traj[2][:, s0]):.3e} "
          f"vs H4={score(traj[3][:, s0], traj[2][:, s0]):.3e}")
    assert e <= RTOL, e
    assert score(traj[1][:, s0], traj[2][:, s0]) > RTOL and score(traj[3][:, s0], traj[2][:, s0]) > RTOL
    s1 = slice(offs[1], T)
    check_step(f"c/{sched}/{offs[1]}/live", H[:, s1], [t[:, s1] for t in traj], K)


# ---------------------------------------------------------------------------------------------------------------------
# d. non-finite frames: NaN (quiet and signalling payloads) and an infinity cross the hand-offs as NaN / inf and stay in
#    their frames' columns
# ---------------------------------------------------------------------------------------------------------------------
def _bad_frames(X, payloads, dtype):
    """X with frame 5 NaN, frames 17, 40, 41 (...) filled with the given bit patterns, bin 7 of frame 70 inf"""
    Xb = X.copy()
    Xb[:, 5] = np.nan
    itype = np.uint32 if dtype == np.float32 else np.uint64
    frames = [17, 40, 41][:len(payloads)]
    for t, bits in zip(frames, payloads):
        Xb[:, t] = np.array([bits], dtype=itype).view(dtype)[0]
    Xb[7, 70] = np.inf
    bad = [5, 70] + frames
    for t, bits in zip(frames, payloads):
        assert Xb.view(itype)[0, t] == bits
    return Xb, bad


def _nonfinite_check(name, got_bad, got_ref, want, bad, tile_mates_rtol=None):
    """the bad frames' NaN / inf pattern is the oracle's; every other frame is bitwise that of the call without them
    (tile_mates_rtol: k_fused_all - the frames sharing a frame tile of 16 with a bad one within that rtol instead: its
    update takes the IEEE division for the whole wavefront when a denominator is out of the shared reciprocal's range)"""
    assert np.array_equal(np.isnan(got_bad[:, bad]), np.isnan(want[:, bad])), name
    assert np.array_equal(np.isinf(got_bad[:, bad]), np.isinf(want[:, bad])), name
    assert np.isfinite(got_ref).all()
    frames = np.arange(got_bad.shape[1])
    mates = np.setdiff1d(frames[np.isin(frames // 16, np.asarray(bad) // 16)], bad) if tile_mates_rtol else []
    keep = np.setdiff1d(frames, np.concatenate([bad, mates]))
    assert np.array_equal(np.ascontiguousarray(got_bad[:, keep]).view(np.uint8),
                          np.ascontiguousarray(got_ref[:, keep]).view(np.uint8)), name
    if len(mates):
        np.testing.assert_allclose(got_bad[:, mates], got_ref[:, mates], rtol=tile_mates_rtol, atol=0)


F32_PAYLOADS = (0x7FFFFFFF, 0x7F800001, 0xFFC00003)
F64_PAYLOADS = (0x7FF0000000000001, 0x7FFFFFFFFFFFFFFF)
NONFINITE32 = [("tagged", 300, 8, 6), ("static", 300, 4, 3), ("ticket", 4090, 4, 5), ("ticket_reduce", 4090, 8, 9)]


@pytest.mark.parametrize("sched,T,w,c", NONFINITE32)
def test_wide_non_finite_frames(sched, T, w, c):
    import exemplars_vc_amd as evc
    o = oracle()
    M, N, K = 150, 300, 3
    name, c_eff, variant = schedule(M, N, T, w, c, cus())
    assert name == sched
    A, X, _ = problem(M, N, T, seed=T + w)
    Xb, bad = _bad_frames(X, F32_PAYLOADS, np.float32)
    kw = dict(iters=K, eps_mode="zero_replace", init="const", init_value=0.02, fused_c=c, fused_w=w, info=True)
    Hb, ib = evc.solve_activations(A, Xb, **kw)
    Hr, ir = evc.solve_activations(A, X, **kw)
    for i in (ib, ir):
        assert_ran(i, variant, members=c_eff, launches=1)
    with np.errstate(invalid="ignore", over="ignore"):
        want = o.mu_solve(A.astype(np.float64), Xb.astype(np.float64), np.full((N, T), 0.02), K, o.EPS_ZERO_REPLACE,
                          SK_EPS, algo="factored")
    assert not np.isfinite(want[:, bad]).any()
    _nonfinite_check(f"d/{sched}", Hb, Hr, want, bad)


@pytest.mark.parametrize("M,tpw", WIDE64_CASES)
def test_wide64_non_finite_frames(M, tpw):
    import exemplars_vc_amd as evc
    o = oracle()
    N, T, K = 300, 200, 3
    p = o.synth_problem(M, N, T, seed=tpw)
    Xb, bad = _bad_frames(p["X"], F64_PAYLOADS, np.float64)
    kw = dict(iters=K, eps_mode="zero_replace", init="const", init_value=0.02, fused_c=5, fused_w=tpw, info=True)
    Hb, ib = evc.solve_activations(p["A"], Xb, **kw)
    Hr, ir = evc.solve_activations(p["A"], p["X"], **kw)
    for i in (ib, ir):
        assert i["kernel"] == "k_fused_wide64" and i["redo"] == 0, i
        assert i["variant"] == {"static": True, "reduce": True, "tagged": False, "tpw": tpw, "tiles": 4 * tpw + 1}, i
    with np.errstate(invalid="ignore", over="ignore"):
        want = o.mu_solve(p["A"], Xb, np.full((N, T), 0.02), K, o.EPS_ZERO_REPLACE, SK_EPS, algo="factored")
    _nonfinite_check(f"d/wide64<{tpw}>", Hb, Hr, want, bad)


def test_fused_all_non_finite_frames():
    """k_fused_all's exchange (M <= 32, float64, several members per frame tile) tags every partial sum in bit 0"""
    import exemplars_vc_amd as evc
    o = oracle()
    M, N, T, K = 25, 4096, 688, 3
    p = o.synth_problem(M, N, T, seed=21)
    Xb, bad = _bad_frames(p["X"], F64_PAYLOADS, np.float64)
    kw = dict(iters=K, eps_mode="zero_replace", init="const", init_value=0.01, info=True)
    Hb, ib = evc.solve_activations(p["A"], Xb, **kw)
    Hr, ir = evc.solve_activations(p["A"], p["X"], **kw)
    for i in (ib, ir):
        assert i["kernel"] == "k_fused_all" and i["exchange"] == 1 and i["members"] > 1 and i["redo"] == 0, i
        assert i["variant"] is None, i
    with np.errstate(invalid="ignore", over="ignore"):
        want = o.mu_solve(p["A"], Xb, np.full((N, T), 0.01), K, o.EPS_ZERO_REPLACE, SK_EPS, algo="factored")
    _nonfinite_check("d/k_fused_all", Hb, Hr, want, bad, tile_mates_rtol=1e-14)
