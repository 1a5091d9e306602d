"""k_cd_sweep (evc_cd.hip) sweep by sweep against the float64 restatement (tests/cd_restatement.py), at every lane
geometry the kernel picks.

cd_geometry chooses the layout from M alone: L lanes per frame (the smallest power of two with ceil(M / L) <= 16),
mpl = ceil(M / L) residual slots per lane, F = 64 / L frames per wavefront tile and the instance k_cd_sweep<T, MPL>
with MPL = 1, 8 or 16.  Components go in blocks of 16; when N % 16 != 0 the last block is padded (hess = 0, clamped H
reads, guarded violation and stores).  The fixture tests (test_gpu_cd.py) run M = 1, 25, 201 and 513 with N % 16 == 0
and max_iter <= 200; this file runs every L and every MPL, padded blocks, partial tiles, zero-length utterances, leading
dimensions above the minimum, and violation traces longer than the device ring (CD_TRACE_CAP = 256).

Each step case runs max_iter = K sweeps with tol = 0 and checks
  - float64 H:  max|H - H_K| <= 1e-10 max|H_K|, and the restatement's H_{K-1} fails that bound (one sweep is visible);
  - float32 H:  |H - H_K| <= 1e-4 max(|H_K|, 1e-2 max|H_K|) against float64 on the float32-rounded inputs; H_{K-1}
    fails it as well.  The floor is 1e-2, not 1e-6: grad / hess amplifies the float32 rounding of the gradient's dot
    product in small entries, and the numpy restatement run in float32 is itself 2e-4 to 9e-4 off at a floor of 1e-6
    (<= 2e-5 at 1e-2) on these cases, while one sweep moves some entry by >= 0.3 max|H_K|;
  - the violation trace per sweep at rtol 1e-9 (float64) and n_iter == K.
test_cd_steps_host.py (CPU) proves the geometry mirror against evc_cd_workspace_bytes, holds INSTANCES against the
template instances in the built library, checks the restatement against scikit-learn at the matrix's (M, N), and shows
that h_err / v_err reject four wrong variants of the algebra."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cd_restatement import cd_iterations, cd_solve  # noqa: E402

pytestmark = pytest.mark.gpu

CD_B, CD_WAVE, CD_MAX_M, CD_TRACE_CAP = 16, 64, 1024, 256
H_BOUND, V_RTOL = 1e-10, 1e-9
F32_RTOL, F32_FLOOR = 1e-4, 1e-2


def geometry(M):
    """mirror of cd_geometry (evc_cd.hip): L, mpl, Mr, F and the MPL of the k_cd_sweep instance; None past 1024"""
    if not 1 <= M <= CD_MAX_M:
        return None
    L = 1
    while -(-M // L) > 16:
        L *= 2
    mpl = -(-M // L)
    return {"L": L, "mpl": mpl, "Mr": mpl * L, "F": CD_WAVE // L, "MPL": 1 if mpl <= 1 else 8 if mpl <= 8 else 16}


# ---------------------------------------------------------------------------------------------------------------------
# comparisons (test_cd_steps_host.py feeds them the mutants)
# ---------------------------------------------------------------------------------------------------------------------
def h_err(got, want):
    """max|got - want| / max|want| (the float64 bound); 0 when both are all zero"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    d = float(np.abs(got - want).max()) if want.size else 0.0
    s = float(np.abs(want).max()) if want.size else 0.0
    return d / s if s > 0 else (0.0 if d == 0 else math.inf)


def f32_err(got, want):
    """max |got - want| / max(|want|, 1e-6 max|want|) (the float32 bound)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    s = float(np.abs(want).max()) if want.size else 0.0
    if s == 0:
        return 0.0 if not np.any(got) else math.inf
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), F32_FLOOR * s)))


def v_err(got, want):
    """largest relative difference of two violation traces; inf when their NaN places differ or a 0 is not matched"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return math.inf
    fin = ~np.isnan(want)
    g, w = got[fin], want[fin]
    if np.any((w == 0) & (g != 0)):
        return math.inf
    nz = w != 0
    return float(np.max(np.abs(g[nz] - w[nz]) / np.abs(w[nz]))) if nz.any() else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# problems, the reference, one GPU call
# ---------------------------------------------------------------------------------------------------------------------
def problem(M, N, T, seed, zero_frames=False):
    """frames-as-rows X (T, M) and exemplar rows W (N, M); rows 1, 8, 15 ... of W are zero (hess = l2 there)"""
    rng = np.random.default_rng(seed)
    W = rng.random((N, M)) ** 2 + 0.05
    W[1::7] = 0.0
    X = (rng.random((T, N)) * (rng.random((T, N)) < 0.3)) @ W + 0.05 * rng.random((T, M))
    if zero_frames:
        X[::5] = 0.0
    return X, W


def reference(X, W, K, H0=None, l1=0.0, l2=0.0):
    """(H_K, H_{K-1}, violations of sweeps 1..K) of the float64 restatement"""
    HK, v = cd_iterations(X, W, K, H0=H0, l1=l1, l2=l2)
    if K == 1:
        HK1 = np.zeros_like(HK) if H0 is None else np.asarray(H0, np.float64)
    else:
        HK1, _ = cd_iterations(X, W, K - 1, H0=H0, l1=l1, l2=l2)
    return HK, HK1, v


def gpu(W, X, H0=None, layout="frame_major", dtype=np.float64, **kw):
    """one solve_activations_cd call on frames-as-rows inputs; returns H (T, N) as computed, and info"""
    from exemplars_vc_amd import solve_activations_cd
    W, X = W.astype(dtype), X.astype(dtype)
    H0 = None if H0 is None else np.asarray(H0).astype(dtype)
    if layout == "bin_major":
        W, X = np.ascontiguousarray(W.T), np.ascontiguousarray(X.T)
        H0 = None if H0 is None else np.ascontiguousarray(H0.T)
    H, info = solve_activations_cd(W, X, H0, layout=layout, info=True, **kw)
    assert H.dtype == dtype and info["kernel"] == "k_cd_sweep"
    return (H.T if layout == "bin_major" else H), info


def check_step(tag, M, H, info, ref, K, f32=False):
    """H is the restatement's H_K within the bound and H_{K-1} is not; the trace matches; n_iter == K"""
    HK, HK1, v = ref
    err, bound = (f32_err, F32_RTOL) if f32 else (h_err, H_BOUND)
    e, margin = err(H, HK), err(HK1, HK)
    ve = v_err(info["violation"][0], v)
    g = geometry(M)
    print(f"STEPS {tag} L={g['L']} MPL={g['MPL']} dtype={'f32' if f32 else 'f64'} K={K} err={e:.3e} "
          f"one_sweep={margin:.3e} viol={ve:.3e}")
    assert int(info["n_iter"][0]) == K, (tag, info["n_iter"])
    assert e <= bound, (tag, e)
    assert margin > bound, (tag, margin)
    if not f32:
        assert ve <= V_RTOL, (tag, ve)
    return e


# ---------------------------------------------------------------------------------------------------------------------
# a. the geometry matrix: M at and just past every L edge, N % 16 != 0 in most cases, T around the tile size F
# ---------------------------------------------------------------------------------------------------------------------
# (M, N, T, K); L / F in the comment.  At M = 1, or N = 1, the first sweep already reaches the fixed point (one bin:
# the first component with a negative gradient takes the whole frame), so those cases run one sweep.
MATRIX = [
    (1, 17, 63, 1),         # L 1, MPL 1, F 64: T = F - 1
    (1, 100, 197, 1),       #                   T = 3F + 5
    (2, 15, 65, 2),         # L 1, MPL 8:       T = F + 1
    (8, 33, 64, 3),         #                   T = F
    (9, 1, 197, 1),         # L 1, MPL 16
    (16, 16, 65, 1),
    (17, 100, 31, 2),       # L 2, F 32
    (32, 15, 101, 3),
    (33, 17, 15, 1),        # L 4, F 16
    (64, 100, 17, 3),
    (65, 33, 7, 2),         # L 8, F 8
    (128, 16, 29, 1),
    (129, 15, 5, 3),        # L 16, F 4
    (256, 100, 3, 2),
    (257, 17, 1, 1),        # L 32, F 2
    (512, 33, 11, 3),
    (513, 15, 2, 2),        # L 64, F 1
    (1000, 100, 1, 3),
    (1024, 17, 8, 1),
    (1024, 16, 1, 2),
]


@pytest.mark.parametrize("M,N,T,K", MATRIX, ids=[f"m{m}_n{n}_t{t}_k{k}" for m, n, t, k in MATRIX])
def test_geometry_matrix(M, N, T, K):
    X, W = problem(M, N, T, seed=M * 1000 + N)
    H, info = gpu(W, X, max_iter=K, tol=0.0)
    check_step(f"matrix m{M}_n{N}_t{T}", M, H, info, reference(X, W, K), K)


# ---------------------------------------------------------------------------------------------------------------------
# b. options, layout and warm start at every L (one M per L, a padded block and a partial tile)
# ---------------------------------------------------------------------------------------------------------------------
L_M = {1: 9, 2: 20, 4: 40, 8: 100, 16: 200, 32: 300, 64: 700}
L_IDS = [f"L{L}_m{M}" for L, M in L_M.items()]
OPTIONS = {"l1": (0.05, 0.0), "l2": (0.0, 0.1), "l1l2": (0.05, 0.1)}      # times M, as sklearn scales alpha_W


def l_problem(M, seed, zero_frames=False):
    g = geometry(M)
    return problem(M, 33, g["F"] + 1, seed, zero_frames)


@pytest.mark.parametrize("opt", sorted(OPTIONS))
@pytest.mark.parametrize("M", L_M.values(), ids=L_IDS)
def test_regularisation_at_every_L(M, opt):
    X, W = l_problem(M, seed=M + 7, zero_frames=True)
    l1, l2 = (M * a for a in OPTIONS[opt])
    K = 3
    H, info = gpu(W, X, max_iter=K, tol=0.0, l1=l1, l2=l2)
    check_step(f"{opt} m{M}", M, H, info, reference(X, W, K, l1=l1, l2=l2), K)
    assert not np.any(H[::5])                       # zero frames stay at 0


@pytest.mark.parametrize("M", L_M.values(), ids=L_IDS)
def test_all_zero_utterance_stops_at_one(M):
    g = geometry(M)
    _, W = l_problem(M, seed=M)
    H, info = gpu(W, np.zeros((g["F"] + 1, M)), max_iter=4, tol=0.0, l1=0.5)
    assert int(info["n_iter"][0]) == 1
    assert not np.any(H)
    assert info["violation"][0][0] == 0.0 and np.isnan(info["violation"][0][1:]).all()


@pytest.mark.parametrize("M", L_M.values(), ids=L_IDS)
def test_bin_major_is_bitwise_frame_major(M):
    X, W = l_problem(M, seed=M + 1)
    fm, ifm = gpu(W, X, layout="frame_major", max_iter=3, tol=0.0)
    bm, ibm = gpu(W, X, layout="bin_major", max_iter=3, tol=0.0)
    assert np.array_equal(fm, bm)
    np.testing.assert_array_equal(ifm["violation"], ibm["violation"])
    assert h_err(fm, reference(X, W, 3)[0]) <= H_BOUND


@pytest.mark.parametrize("M", L_M.values(), ids=L_IDS)
def test_warm_start_at_every_L(M):
    X, W = l_problem(M, seed=M + 2)
    rng = np.random.default_rng(M)
    H0 = rng.random((X.shape[0], W.shape[0])) * (rng.random((X.shape[0], W.shape[0])) < 0.5)
    K = 2
    H, info = gpu(W, X, H0, layout="bin_major" if M % 2 else "frame_major", max_iter=K, tol=0.0)
    check_step(f"warm m{M}", M, H, info, reference(X, W, K, H0=H0), K)
    H5, _ = gpu(W, X, max_iter=5, tol=0.0)
    H3, _ = gpu(W, X, max_iter=3, tol=0.0)
    H3_2, _ = gpu(W, X, H3, max_iter=2, tol=0.0)
    assert h_err(H3, H5) > 1e-6
    assert h_err(H3_2, H5) <= 1e-12, h_err(H3_2, H5)


# ---------------------------------------------------------------------------------------------------------------------
# c. float32 at every L and every MPL
# ---------------------------------------------------------------------------------------------------------------------
# (M, N, T, K)
F32_CASES = [(1, 1, 65, 1), (5, 33, 63, 3), (12, 16, 64, 1), (20, 100, 33, 2), (40, 17, 17, 3), (100, 15, 9, 2),
             (200, 33, 5, 3), (300, 100, 3, 2), (700, 17, 2, 3)]


@pytest.mark.parametrize("M,N,T,K", F32_CASES, ids=[f"m{m}_n{n}_t{t}_k{k}" for m, n, t, k in F32_CASES])
def test_float32_at_every_L_and_MPL(M, N, T, K):
    X, W = problem(M, N, T, seed=M * 31 + N)
    X32, W32 = X.astype(np.float32), W.astype(np.float32)
    H, info = gpu(W32, X32, dtype=np.float32, max_iter=K, tol=0.0)
    check_step(f"f32 m{M}_n{N}_t{T}", M, H, info, reference(X32.astype(np.float64), W32.astype(np.float64), K), K,
               f32=True)


# ---------------------------------------------------------------------------------------------------------------------
# d. leading dimensions above the minimum: one raw evc_cd_solve call per layout and start, sentinels in H's padding
# ---------------------------------------------------------------------------------------------------------------------
SENTINEL = -12345.25


def raw_cd_solve(W, X, H0, offs, layout, pad, max_iter):
    """evc_cd_solve through ctypes as solve_activations_cd makes it, but with lda / ldx / ldh = minimum + pad; returns
    (H buffer with its padding, frames-as-rows view of H, n_iter, violation)"""
    import torch
    from exemplars_vc_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    tr = (lambda z: z) if layout == "frame_major" else (lambda z: np.ascontiguousarray(z.T))

    def padded(a, fill):
        a = tr(a)
        buf = torch.full((a.shape[0], a.shape[1] + pad), fill, dtype=torch.float64, device=dev)
        buf[:, :a.shape[1]] = torch.from_numpy(a).to(dev)
        return buf
    T, N = X.shape[0], W.shape[0]
    A_b, X_b = padded(W, 7.5), padded(X, -3.5)
    H_b = padded(np.full((T, N), 3.25) if H0 is None else H0, SENTINEL)
    M = W.shape[1]
    o = _lib.CdOpts()
    o.struct_bytes = C.sizeof(_lib.CdOpts)
    o.dtype = _lib.F64
    o.layout = _lib.FRAME_MAJOR if layout == "frame_major" else _lib.BIN_MAJOR
    o.init_mode = _lib.INIT_SKLEARN if H0 is None else _lib.INIT_GIVEN
    o.max_iter, o.tol = max_iter, 0.0
    off = np.ascontiguousarray(offs, dtype=np.int32)
    n_utt = len(off) - 1
    ws = torch.empty(int(L.evc_cd_workspace_bytes(M, N, T, n_utt, _lib.F64)), dtype=torch.uint8, device=dev)
    n_iter = np.zeros(n_utt, dtype=np.int32)
    viol = np.full((n_utt, max_iter), np.nan)
    st = L.evc_cd_solve(A_b.data_ptr(), A_b.stride(0), X_b.data_ptr(), X_b.stride(0), H_b.data_ptr(), H_b.stride(0),
                        M, N, T, off.ctypes.data_as(C.POINTER(C.c_int)), n_utt, C.byref(o), ws.data_ptr(), ws.numel(),
                        n_iter.ctypes.data_as(C.POINTER(C.c_int)), viol.ctypes.data_as(C.POINTER(C.c_double)),
                        C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert st == 0, st
    Hb = H_b.cpu().numpy()
    view = Hb[:, :Hb.shape[1] - pad]
    return Hb, (view if layout == "frame_major" else view.T), n_iter, viol


@pytest.mark.parametrize("start", ["zero", "given"])
@pytest.mark.parametrize("layout", ["frame_major", "bin_major"])
def test_leading_dimensions_above_the_minimum(layout, start):
    M, N, pad = 40, 17, 3                             # L 4, F 16; utterances of 9 and 12 frames: partial tiles
    X, W = problem(M, N, 21, seed=5)
    offs = [0, 9, 21]
    H0 = None
    if start == "given":
        rng = np.random.default_rng(3)
        H0 = rng.random((21, N)) * (rng.random((21, N)) < 0.5)
    Hb, H, n_iter, viol = raw_cd_solve(W, X, H0, offs, layout, pad, max_iter=3)
    assert (Hb[:, Hb.shape[1] - pad:] == SENTINEL).all()
    packed, info = gpu(W, X, H0, layout=layout, max_iter=3, tol=0.0, utt_offsets=offs)
    assert np.array_equal(H, packed)
    assert np.array_equal(n_iter, info["n_iter"])
    np.testing.assert_array_equal(viol, info["violation"])
    assert h_err(H, reference(X, W, 3, H0=H0)[0]) <= H_BOUND


# ---------------------------------------------------------------------------------------------------------------------
# e. batches with zero-length utterances at L = 1, 4, 32; stops from the restatement's own ratios
# ---------------------------------------------------------------------------------------------------------------------
def stop_iteration(v, tol, max_iter):
    """sklearn's rule on a violation trace: the first it with v_1 == 0 or v_it / v_1 <= tol, else max_iter"""
    for it in range(1, max_iter + 1):
        if v[0] == 0 or v[it - 1] / v[0] <= tol:
            return it
    return max_iter


def pick_tol(traces, max_iter):
    """a tol at the log-midpoint of two consecutive ratios of one trace (a new minimum) that keeps every ratio of every
    trace at least 1e-6 (relative) away, and gives at least three different stops below max_iter"""
    for r in traces:
        r = r / r[0]
        for k in range(2, max_iter):
            lo, hi = r[k], r[:k].min()
            if not lo < hi:
                continue
            tol = math.sqrt(lo * hi)
            stops = [stop_iteration(t, tol, max_iter) for t in traces]
            clear = all(np.abs(np.log(t / t[0] / tol)).min() > 1e-6 for t in traces)
            if clear and len(set(s for s in stops if s < max_iter)) >= 3:
                return tol, stops
    raise AssertionError("no tol separates the stops")


@pytest.mark.parametrize("M", [10, 40, 300], ids=["L1", "L4", "L32"])
def test_batch_with_zero_length_utterances(M):
    g = geometry(M)
    F, N, max_iter = g["F"], 33, 40
    lens = [0, F - 1, F + 1, 0, 2 * F, 1, 0]
    W = problem(M, N, 1, seed=M)[1]
    utts = []
    for u, t in enumerate(lens):
        rng = np.random.default_rng(100 * M + u)
        Hs = rng.random((t, N)) ** (1 + 2 * u) * (rng.random((t, N)) < 0.2 + 0.1 * u)
        utts.append(Hs @ W + (0.01 + 0.05 * u) * rng.random((t, M)))
    traces = [cd_iterations(x, W, max_iter)[1] for x in utts if len(x)]
    tol, _ = pick_tol(traces, max_iter)
    offs = np.concatenate([[0], np.cumsum(lens)])
    act, info = gpu(W, np.concatenate(utts), max_iter=max_iter, tol=tol, utt_offsets=offs)
    stops = []
    for u, x in enumerate(utts):
        ni, v = int(info["n_iter"][u]), info["violation"][u]
        if len(x) == 0:
            assert ni == 1 and v[0] == 0.0 and np.isnan(v[1:]).all(), (u, ni, v[:3])
            continue
        _, ni_ref, v_ref = cd_solve(x, W, max_iter, tol)
        assert ni == ni_ref, (u, ni, ni_ref)
        assert v_err(v[:ni], v_ref) <= V_RTOL and np.isnan(v[ni:]).all()
        h, inf = gpu(W, x, max_iter=max_iter, tol=tol)
        assert np.array_equal(act[offs[u]:offs[u + 1]], h), u
        np.testing.assert_array_equal(v, inf["violation"][0])
        stops.append(ni)
    print(f"BATCH M={M} L={g['L']} tol={tol:.6e} stops={stops}")
    assert len(set(stops)) >= 3


# ---------------------------------------------------------------------------------------------------------------------
# f. the violation ring: traces longer than CD_TRACE_CAP are copied out in chunks; stale slots are masked
# ---------------------------------------------------------------------------------------------------------------------
RING_TOL = 5e-3


def ring_problem():
    """a dictionary of 20 strongly correlated exemplars (slow convergence, M = 6: L 1, MPL 8) and three two-frame
    utterances plus an empty one: the first stops before sweep 256, the third between 257 and 512, the last starts
    from its own 200th iterate and does not reach RING_TOL within 600 sweeps"""
    rng = np.random.default_rng(11)
    base = rng.random(6) + 0.5
    W = base + 0.15 * rng.random((20, 6))
    W[3] = 0.0
    r = np.random.default_rng(8)
    a = r.random((2, 6)) * 3
    r = np.random.default_rng(2)
    b = r.random((2, 20)) @ W * np.linspace(0.8, 1.2, 6)
    r = np.random.default_rng(1)
    c = (r.random((2, 20)) ** 8) @ W
    utts = [a, np.zeros((0, 6)), b, c]
    H0 = [np.zeros((2, 20)), np.zeros((0, 20)), np.zeros((2, 20)), cd_iterations(c, W, 200)[0]]
    return W, utts, H0


@pytest.fixture(scope="module")
def ring():
    W, utts, H0 = ring_problem()
    refs = [cd_iterations(x, W, 600, H0=h)[1] if len(x) else None for x, h in zip(utts, H0)]
    offs = np.concatenate([[0], np.cumsum([len(x) for x in utts])])
    X, H0c = np.concatenate(utts), np.concatenate(H0)
    short = gpu(W, X, H0c, max_iter=200, tol=RING_TOL, utt_offsets=offs)
    return W, utts, H0, refs, offs, X, H0c, short


@pytest.mark.parametrize("max_iter", [255, 256, 257, 600])
def test_violation_ring(ring, max_iter):
    W, utts, H0, refs, offs, X, H0c, (_, short) = ring
    act, info = gpu(W, X, H0c, max_iter=max_iter, tol=RING_TOL, utt_offsets=offs)
    ni = [int(n) for n in info["n_iter"]]
    want = [stop_iteration(v, RING_TOL, max_iter) if v is not None else 1 for v in refs]
    print(f"RING max_iter={max_iter} n_iter={ni} restatement={want}")
    assert ni == want
    assert ni[0] < 256 and ni[1] == 1 and ni[3] == max_iter
    assert (257 <= ni[2] <= 512) if max_iter == 600 else ni[2] == max_iter
    for u, (x, h0) in enumerate(zip(utts, H0)):
        v = info["violation"][u]
        assert not np.isnan(v[:ni[u]]).any() and np.isnan(v[ni[u]:]).all(), u
        np.testing.assert_array_equal(v[:200], short["violation"][u])
        if len(x) == 0:
            assert v[0] == 0.0
            continue
        ref = refs[u][:ni[u]]
        big = ref > 1e-8 * ref[0]
        assert v_err(v[:ni[u]][big], ref[big]) <= V_RTOL, u
        h, inf = gpu(W, x, h0, max_iter=max_iter, tol=RING_TOL)
        assert np.array_equal(act[offs[u]:offs[u + 1]], h), u
        np.testing.assert_array_equal(v, inf["violation"][0])


# every (element type, MPL) that a case above launches; test_cd_steps_host.py holds it against the library
INSTANCES = ({("double", geometry(m)["MPL"]) for m, *_ in MATRIX}
             | {("float", geometry(m)["MPL"]) for m, *_ in F32_CASES})
