"""k_gemm_nt (evc_gemm.hip) and k_gemm2 (evc_gemm2.hip) step by step against the float64 oracle, at every block shape.

The two contraction kernels carry every solve with more than 32 bins on small batches, every fused=False call and the
redo of a task-queue solve whose wait ran out; other GPU tests use them as the expected value.  They were compared with
the oracle only after 20 to 60 iterations (where one wrong mid-solve step is damped away) and at T <= 150, N <= 512 (where
the launchers always pick the smallest block).  Here K <= 4, every case enters through evc.solve_activations /
evc.convert with fused=False (or a forced redo), asserts the kernel and the block shapes that ran
(evc_solve_info.variant, against the restatement below of csrc/evc_gemm_plan.h evaluated with the device's CU count -
tests/test_gemm_plan_host.py holds that restatement against the C++ on a grid) and redo == 0, and compares H (and Y
where formed) with oracle.mu_trajectory / oracle.mu_solve in float64:
    float32  rtol 1e-4 with an absolute floor of 1e-6 max|H_K| (as tests/test_gpu_wide_steps.py)
    float64  rtol 1e-8, pure relative, exact zeros where the oracle has zeros
and every case with K >= 2 shows that the oracle's own H_{K-1} fails the same check.

Sizes that a rule makes depend on the CU count are derived from it (the values in the comments are those of 256 CUs).  A
case whose activations would pass 1 GiB on some CU count is skipped there; on 256 CUs none is (test_no_case_is_skipped_
on_256_cus)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
RTOL, AFLOOR, RTOL64 = 1e-4, 1e-6, 1e-8
SK_EPS = float(np.finfo(np.float32).eps)
EPS = {"add": 1e-9, "zero_replace": SK_EPS, "none": 0.0, "clamp": 1e-15}
GIB = 1 << 30


def oracle():
    from oracle import evc_oracle as o
    return o


def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---------------------------------------------------------------------------------------------------------------------
# csrc/evc_gemm_plan.h restated (tests/test_gemm_plan_host.py compares it with the C++ over the host program's grid)
# ---------------------------------------------------------------------------------------------------------------------
def ru(x, m):
    return -(-x // m) * m


def plan_nt(I, J, Kd, ldc, n_cus, have_scratch, scratch_elems):
    """gemm_nt on k_gemm_nt: (bf, br, splits)"""
    blocks = (I // 64) * (J // 64)
    if ((I + 127) // 128) * (J // 64) < 256:
        splits, slab = 1, I * ldc
        if have_scratch and ldc == J:
            n = n_cus if n_cus > 0 else 256
            eff = (1.0, 0.6, 0.8, 0.9, 0.95)
            nslabs, chunk = Kd // 16, (512 if Kd >= 1024 else 64)
            best = 1e30
            if Kd >= 1024:
                for sp in range(1, 9):
                    if blocks * sp > 4 * n or (sp > 1 and (nslabs // sp) * 16 < chunk) or sp * slab > scratch_elems:
                        continue
                    per_cu = (blocks * sp + n - 1) // n
                    cost = per_cu / sp / eff[per_cu]
                    if cost < best - 1e-9:
                        best, splits = cost, sp
            else:
                for sp in range(2, 9):
                    if nslabs % sp == 0 and blocks * sp <= 1024 and Kd // sp >= chunk and sp * slab <= scratch_elems:
                        splits = sp
        return 64, 64, splits
    if I % 128:
        return 64, (128 if J % 128 == 0 else 64), 1
    return 128, (128 if J % 128 == 0 else 64), 1


def plan_nt_mu(I, J):
    """gemm_nt_mu on k_gemm_nt: (bf, br)"""
    b128, b64 = ((I + 127) // 128) * (J // 128), (I // 64) * (J // 128)
    t128, t64 = 2 * ((b128 + 255) // 256), (b64 + 511) // 512
    return (64, 128) if (I % 128 or (I <= 2048 and t64 < t128)) else (128, 128)


G2_BLOCK = {0: (128, 128), 1: (128, 128), 2: (64, 128), 3: (64, 64)}


def _round_eff(wg, slots):
    return wg / float(-(-wg // slots) * slots)


def plan_g2(I, J, Kd, ldc, n_cus, have_scratch, scratch_elems):
    """gemm2 on k_gemm2: (shape, bf, br, splits)"""
    n = n_cus if n_cus > 0 else 256
    wide = J % 128 == 0 and (I // 64) * (J // 128) >= 3 * n
    shape = 2 if wide else 3
    blocks = (I // 64) * (J // (128 if wide else 64))
    slots = n * (3 if wide else 4)
    splits, slab = 1, I * ldc
    if have_scratch and ldc == J:
        best = _round_eff(blocks, slots)
        for sp in range(2, 33):
            if not best < 0.85:
                break
            if Kd % (sp * 16) or Kd // sp < 128 or sp * slab > scratch_elems:
                continue
            e = _round_eff(blocks * sp, slots)
            if e > best + 0.03:
                best, splits = e, sp
    return (shape,) + G2_BLOCK[shape] + (splits,)


def plan_g2_mu(esize, I, J, n_cus):
    """gemm2_mu on k_gemm2: (shape, bf, br)"""
    n = n_cus if n_cus > 0 else 256
    b128, b64 = (I // 128) * (J // 128), (I // 64) * (J // 128)
    shape = 1 if (esize == 4 and I % 128 == 0 and b128 >= 8 * n) else (2 if b64 >= 3 * n else 3)
    return (shape,) + G2_BLOCK[shape]


def dims(esize, M, N, T):
    """Mk, Mj, Np, Tp of csrc/evc_internal.h (make_dims, frame_pad) and the elements of the split-K scratch of V = H Am^T
    (csrc/evc_solve_plan.h, carve)"""
    Mk, Mj, Np = ru(M, 16), ru(M, 64), ru(N, 128)
    Tp = ru(T, 64 if (esize == 4 or T <= 2048) else 128)
    vslabs = 32 if Tp <= 2048 else (4 if Tp <= 16384 else (2 if Tp <= 65536 else 0))
    return Mk, Mj, Np, Tp, vslabs * Tp * Mj


def expected_variant(esize, M, N, T, n_cus, algo="factored", loss="frobenius"):
    """(kernel name, decoded evc_solve_info.variant) of a solve on the two contractions (csrc/evc_api.hip, solve_gemm):
    P = X A without scratch (k_gemm2 then counts 256 CUs whatever the device), V = H Am^T with the workspace's scratch,
    the update on Tp x Np"""
    Mk, Mj, Np, Tp, vse = dims(esize, M, N, T)
    g2 = esize == 4
    gram = algo in ("gram", "literal")
    if loss == "kl":
        p = None
    else:
        p = plan_g2(Tp, Np, Mk, Np, 0, False, 0)[1:3] if g2 else plan_nt(Tp, Np, Mk, Np, 256, False, 0)[:2]
    if gram:
        v, vs = None, 0
    elif g2:
        _, bf, br, vs = plan_g2(Tp, Mj, Np, Mj, n_cus if vse else 0, vse > 0, vse)
        v = (bf, br)
    else:
        bf, br, vs = plan_nt(Tp, Mj, Np, Mj, n_cus, vse > 0, vse)
        v = (bf, br)
    u = plan_g2_mu(esize, Tp, Np, n_cus)[1:] if g2 else plan_nt_mu(Tp, Np)
    return ("k_gemm2" if g2 else "k_gemm_nt"), {"update": u, "v": v, "v_splits": vs, "p": p, "deep": False}


# k_gemm_nt<BM, BN, MU> and k_gemm2 launch_shape(case, MU) instances the plans can name, and the case below that runs each
# with the oracle beside it (test_gemm_plan_host.py holds the names against the built library's symbols).  float64
# k_gemm2 and launch_shape case 0 (deep slabs) exist in the library but only diagnostic builds reach them: not tested.
INSTANCES = {
    "k_gemm_nt": {(64, 64, False): "A (split), D (large grid), E", (64, 128, False): "A", (128, 128, False): "B",
                  (128, 64, False): "C", (64, 128, True): "A", (128, 128, True): "B"},
    "k_gemm2": {(3, False): "F, J", (2, False): "G (P), I (V)", (3, True): "F", (2, True): "G", (1, True): "H"},
}
DIAGNOSTIC_ONLY = {"k_gemm2": {(0, False), (0, True), (1, False)}, "k_gemm2<double>": "every instance"}


# ---------------------------------------------------------------------------------------------------------------------
# scoring
# ---------------------------------------------------------------------------------------------------------------------
def score(got, want):
    """float32 cases: max |got - want| / max(|want|, 1e-6 max|want|) over the finite entries of want; inf when the NaN /
    inf patterns differ"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if not (np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))):
        return float("inf")
    fin = np.isfinite(want)
    if not fin.any():
        return 0.0
    floor = AFLOOR * float(np.abs(want[fin]).max())
    return float(np.max(np.abs(got[fin] - want[fin]) / np.maximum(np.abs(want[fin]), floor)))


def score64(got, want):
    """float64 cases: max |got - want| / |want| where want is finite and not zero; inf when the NaN / inf patterns differ
    or got is not exactly zero where want is"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if not (np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))):
        return float("inf")
    zero = want == 0
    if (got[zero] != 0).any():
        return float("inf")
    nz = np.isfinite(want) & ~zero
    if not nz.any():
        return 0.0
    return float(np.max(np.abs(got[nz] - want[nz]) / np.abs(want[nz])))


def check_step(name, esize, got, want, before=None):
    """got matches H_K at the dtype's tolerance and (K >= 2: `before` = H_{K-1}) H_{K-1} does not"""
    sc, tol = (score, RTOL) if esize == 4 else (score64, RTOL64)
    e = sc(got, want)
    margin = sc(before, want) if before is not None else float("nan")
    print(f"GEMMSTEPS {name} err={e:.3e} one_iteration={margin:.3e}")
    assert e <= tol, (name, e)
    if before is not None:
        assert margin > tol, (name, margin)
    return e


def problem(esize, M, N, T, seed, Mb=None):
    p = oracle().synth_problem(M, N, T, Mb=Mb, seed=seed)
    dt = np.float32 if esize == 4 else np.float64
    return p["A"].astype(dt), p["X"].astype(dt), p["B"].astype(dt)


def start(esize, N, T, seed):
    dt = np.float32 if esize == 4 else np.float64
    return (np.random.default_rng(seed).random((N, T)) * 0.05 + 1e-4).astype(dt)


def reference(A, X, H0, K, eps_mode="zero_replace", l1=0.0, algo="factored", loss="frobenius"):
    """(H_K, H_{K-1} or None) of the float64 oracle"""
    o = oracle()
    mode = {"add": o.EPS_ADD, "zero_replace": o.EPS_ZERO_REPLACE, "none": o.EPS_NONE, "clamp": o.EPS_CLAMP}[eps_mode]
    A, X, H0 = (np.asarray(z, np.float64) for z in (A, X, H0))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if algo == "factored":
            traj, _ = o.mu_trajectory(A, X, H0, K, mode, EPS[eps_mode], l1, loss=loss)
            return traj[K - 1], (traj[K - 2] if K >= 2 else None)
        before = o.mu_solve(A, X, H0, K - 1, mode, EPS[eps_mode], l1, algo=algo)
        return o.mu_solve(A, X, before, 1, mode, EPS[eps_mode], l1, algo=algo), (before if K >= 2 else None)


def run_case(name, esize, M, N, T, K, seed, eps_mode="zero_replace", l1=0.0, algo="factored", loss="frobenius", conv=False,
             zero_frames=(), expect=None, **kw):
    """one fused=False solve at (M, N, T): kernel, variant and redo asserted, H (and Y) against the oracle.  Returns the
    info record."""
    import exemplars_vc_amd as evc
    if N * T * esize > GIB:
        pytest.skip(f"{name}: {N} x {T} activations pass 1 GiB on {cus()} CUs")
    A, X, B = problem(esize, M, N, T, seed, Mb=(M if conv else None))
    X[:, list(zero_frames)] = 0
    H0 = start(esize, N, T, seed + 1)
    args = dict(iters=K, eps_mode=eps_mode, eps=EPS[eps_mode], l1=l1, algo=algo, loss=loss, fused=False, info=True, **kw)
    if conv:
        H, Y, info = evc.convert(A, X, B, H0, **args)
    else:
        H, info = evc.solve_activations(A, X, H0, **args)
        Y = None
    assert H.dtype == A.dtype
    kernel, variant = expected_variant(esize, M, N, T, cus(), algo, loss)
    assert info["kernel"] == kernel and info["redo"] == 0, info
    assert info["variant"] == variant, (info["variant"], variant)
    if expect is not None and cus() == 256:
        for k, v in expect.items():
            assert variant[k] == v, (name, k, variant[k], v)
    want, before = reference(A, X, H0, K, eps_mode, l1, algo, loss)
    check_step(name, esize, H, want, before)
    if conv:
        sc, tol = (score, RTOL) if esize == 4 else (score64, RTOL64)
        e = sc(Y, B.astype(np.float64) @ want)
        print(f"GEMMSTEPS {name}/Y err={e:.3e}")
        assert e <= tol, (name, e)
    return info


# sizes that the rules make depend on the CU count n (at 256 CUs: the values in the comments)
def frames_update_shape2(n):      # float32, N = 2048: (Tp / 64) 16 >= 3 n  ->  3072
    return 64 * -(-3 * n // 16)


def frames_update_shape1(n):      # float32, N = 4096: (Tp / 128) 32 >= 8 n  ->  8192
    return 128 * -(-8 * n // 32)


def frames_plain_wide(n, cols):   # float32 plain product with `cols` blocks of 128 rows: (Tp / 64) cols >= 3 n
    return 64 * -(-3 * n // cols)


# ---------------------------------------------------------------------------------------------------------------------
# float64, k_gemm_nt
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps_mode", ["add", "zero_replace", "none", "clamp"])
def test_a_nt_64x128_update_and_numerator_v_split_by_the_cost_model(eps_mode):
    """Tp = 1984 (not a multiple of 128), Np = 1024 with N = 1000: P <64,128>, V <64,64> split by the cost model
    (Kd = 1024), update <64,128,MU> with the last exemplar block reaching into the padding"""
    info = run_case(f"A/{eps_mode}", 8, 40, 1000, 1950, 3, seed=11, eps_mode=eps_mode, conv=eps_mode == "add",
                    expect={"update": (64, 128), "p": (64, 128), "v": (64, 64), "v_splits": 2})
    assert info["variant"]["v_splits"] > 1 or cus() != 256


@pytest.mark.parametrize("algo", ["factored", "gram"])
def test_b_nt_128x128_update_and_numerator(algo):
    """Tp = 2176 = 17 x 128 (> 2048 frames): P <128,128>, update <128,128,MU>; GRAM: the ping-pong pair of H buffers"""
    run_case(f"B/{algo}", 8, 40, 1000, 2100, 3, seed=12, algo=algo, l1=0.1 if algo == "gram" else 0.0,
             expect={"update": (128, 128), "p": (128, 128)})


def test_c_nt_128x64_v():
    """Mj = 192 bins, Tp = 11008 = 86 x 128: 258 tiles, V <128,64>"""
    run_case("C", 8, 150, 128, 11008, 2, seed=13, expect={"v": (128, 64), "v_splits": 1})


def test_d_nt_64x64_v_on_a_large_grid():
    """Mj = 1088 = 17 x 64 bins, Tp = 1984: 272 tiles of 64 x 64 without a split"""
    run_case("D", 8, 1030, 128, 1984, 2, seed=14, expect={"v": (64, 64), "v_splits": 1})


@pytest.mark.parametrize("N,splits", [(100, 2), (256, 4), (384, 6), (512, 8), (896, 8)])
def test_e_nt_v_split_by_the_divisor_rule(N, splits):
    """Kd = Np < 1024: the largest split <= 8 that divides the k-slabs and leaves 64 of k to each"""
    info = run_case(f"E/N{N}", 8, 40, N, 70, 3, seed=15 + N, conv=N == 384)
    assert info["variant"]["v"] == (64, 64) and info["variant"]["v_splits"] == splits, info["variant"]


# ---------------------------------------------------------------------------------------------------------------------
# float32, k_gemm2
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["frobenius", "kl"])
@pytest.mark.parametrize("M", [16, 20, 40, 65, 100, 130])
def test_f_g2_shape3_k_tails_and_slab_counts(M, loss):
    """the 64 x 64 shape with two slabs in flight: Mk / 32 = 0.5, 1, 1.5, 2.5, 3.5, 4.5 slabs in the update (one slab with a
    half tail up to five with a tail); V = H Am^T with 16-row groups 1+0, 2+0, 2+1 ... of Mj live (the jv skip)"""
    run_case(f"F/M{M}/{loss}", 4, M, 200, 100, 4, seed=20 + M, loss=loss, conv=(M == 65 and loss == "frobenius"),
             expect={"update": (64, 64), "v": (64, 64)})


@pytest.mark.parametrize("algo,K", [("factored", 3), ("gram", 2)])
def test_g_g2_shape2_update_and_numerator(algo, K):
    """N = 2048, Tp = 3072 on 256 CUs: 768 blocks of 64 x 128 = one round of three per CU: update shape 2, P shape 2 (the
    shapes a redo of a large batch lands on).  GRAM: a 2048-deep contraction, 64 slabs"""
    n = cus()
    run_case(f"G/{algo}", 4, 40, 2048, frames_update_shape2(n), K, seed=31, algo=algo,
             expect={"update": (64, 128), "p": (64, 128)})


def test_h_g2_shape1_update():
    """N = 4096, Tp = 8192 on 256 CUs: 2048 blocks of 128 x 128, eight per CU: update shape 1.
    (float32 against float64 over two steps, the update's sums 48 terms long and V's 4096: measured 1.4e-6 on the
    MI355X, 70 times below RTOL.)"""
    n = cus()
    run_case("H", 4, 40, 4096, frames_update_shape1(n), 2, seed=32, expect={"update": (128, 128), "p": (64, 128)})


@pytest.mark.parametrize("M,groups", [(201, 1), (215, 2), (230, 3), (250, 4)])
def test_i_g2_wide_plain_shape_with_every_live_group_count(M, groups):
    """V = H Am^T on the 64 x 128 plain shape (Mj = 256, Tp = 24576 on 256 CUs): wavefront 1 of the last block multiplies
    1, 2, 3 or all 4 of its 16-row groups (rows of Am from Mk on are padding)"""
    n = cus()
    assert (ru(M, 16) - 192) // 16 == groups
    run_case(f"I/M{M}", 4, M, 128, frames_plain_wide(n, 2), 2, seed=40 + M, expect={"v": (64, 128), "v_splits": 1})


def test_j_g2_block_counts_that_are_no_multiple_of_8():
    """the XCD renumbering of the plain products with 18 blocks (P: 3 x 6) and 3 blocks (V)"""
    Mk, Mj, Np, Tp, _ = dims(4, 40, 300, 150)
    assert ((Tp // 64) * (Np // 64)) % 8 and ((Tp // 64) * (Mj // 64)) % 8
    run_case("J", 4, 40, 300, 150, 3, seed=50, expect={"p": (64, 64), "v": (64, 64)})


@pytest.mark.parametrize("fake", [True, 2])
def test_k_redo_of_a_wide_solve_at_its_real_shape(fake):
    """M = 201, float32: the default route is k_fused_wide; its wait is made to run out (at the start; in front of the
    second launch) and the solve is redone on k_gemm2 at a size where the update takes shape 2"""
    import exemplars_vc_amd as evc
    o = oracle()
    n = cus()
    M, N, T, K = 201, 2048, frames_update_shape2(n), 3
    A, X, _ = problem(4, M, N, T, seed=60)
    h0 = 0.0123
    H, info = evc.solve_activations(A, X, iters=K, eps_mode="zero_replace", init="const", init_value=h0, check_every=1,
                                    stop_rule="sklearn", tol=-1e300, info=True, _fake_coop_timeout=fake)
    kernel, variant = expected_variant(4, M, N, T, n)
    assert info["redo"] == 1 and info["kernel"] == kernel == "k_gemm2", info
    assert info["variant"] == variant, (info["variant"], variant)
    if n == 256:
        assert variant["update"] == (64, 128)
    assert int(info["n_iter"][0]) == K
    traj, _ = o.mu_trajectory(A.astype(np.float64), X.astype(np.float64), np.full((N, T), np.float64(np.float32(h0))), K,
                              o.EPS_ZERO_REPLACE, SK_EPS)
    check_step(f"K/{fake}", 4, H, traj[K - 1], traj[K - 2])


# ---------------------------------------------------------------------------------------------------------------------
# stops: the all-stopped block copy, the per-row select in a straddling block, the gate
# ---------------------------------------------------------------------------------------------------------------------
def stops_problem(esize, T, seed=70):
    """Four utterances in T frames (T >= 2200) with boundaries that are no multiples of 64.  The second and the fourth stop
    at the second check: they are a scaled sum of all atoms, which the constant start fits after one iteration, times
    1 +- 0.5 %, so that their error then falls 20 times more slowly than an ordinary utterance's (criterion 1.4e-4 against
    3e-3 .. 5e-3) while their activations still move by 0.8 % from iteration 4 to 12 - a stopped frame that went on being
    updated fails the comparison.  (A scaled atom plus a little of another, as tests/test_gpu_wide.py uses at 120
    iterations, does not stop within 20 iterations at this size: its criterion stays at 3e-3 .. 1e-2.)  The second covers
    whole 64- and 128-row blocks ([192, 448)) and its start, frame 150, falls inside a block shared with the running
    first utterance.  Returns W_rows (N x M), X_rows (T x M), offsets."""
    o = oracle()
    M, N = 40, 128
    p = o.synth_problem(M, N, T, seed=seed)
    dt = np.float32 if esize == 4 else np.float64
    W_rows = np.ascontiguousarray(p["A"].T)
    X_rows = np.ascontiguousarray(p["X"].T)
    offs = [0, 150, 470, T - 700, T]
    rng = np.random.default_rng(seed + 1)
    for u in (1, 3):
        n = offs[u + 1] - offs[u]
        X_rows[offs[u]:offs[u + 1]] = (0.3 * W_rows.sum(axis=0))[None, :] * (1 + 0.01 * (rng.random((n, M)) - 0.5))
    return W_rows.astype(dt), X_rows.astype(dt), offs


STOP_ITERS, STOP_EVERY = 12, 2
# (stop rule's tol; who stops): the atoms stop early and the rest run on / everybody stops well before STOP_ITERS
STOP_TOLS = {"some": {"frobenius": 7e-4, "kl": 7e-4}, "all": {"frobenius": 0.2, "kl": 0.2}}


def stops_reference(W_rows, X_rows, offs, loss, tol):
    """per utterance (activations T_u x N, n_iter) of scikit-learn's fixed-dictionary solve in float64"""
    o = oracle()
    out = []
    W64 = W_rows.astype(np.float64)
    for u in range(len(offs) - 1):
        Xu = X_rows[offs[u]:offs[u + 1]].astype(np.float64)
        if loss == "kl":
            act, n, _ = o.sklearn_mu_fixed_dictionary_kl(Xu, W64, STOP_ITERS, tol, check_every=STOP_EVERY)
        else:
            act, n, _ = o.sklearn_mu_fixed_dictionary(Xu, W64, STOP_ITERS, tol, check_every=STOP_EVERY)
        out.append((act, n))
    return out


def stop_frames(esize, n_cus, big):
    """frames of a stops case: 2200 (float64: Tp = 2304 > 2048, the 128-row update block; float32: the 64 x 64 shape), or
    for float32 the smallest count at which the update takes the 64 x 128 shape with N = 128 (49152 - 40 on 256 CUs)"""
    return frames_plain_wide(n_cus, 1) - 40 if big else 2200


STOP_CASES = [(8, "factored", "frobenius", False), (8, "gram", "frobenius", False), (8, "factored", "kl", False),
              (4, "factored", "frobenius", False), (4, "gram", "frobenius", False), (4, "factored", "kl", False),
              (4, "factored", "frobenius", True), (4, "gram", "frobenius", True)]


@pytest.mark.parametrize("who", ["some", "all"])
@pytest.mark.parametrize("esize,algo,loss,big", STOP_CASES,
                         ids=[f"f{8 * c[0]}-{c[1]}-{c[2]}{'-big' if c[3] else ''}" for c in STOP_CASES])
def test_l_stopped_utterances(esize, algo, loss, big, who):
    """scikit-learn's stop rule every 2 iterations: GRAM copies an all-stopped block to the other H buffer, FACTORED and
    KL leave it in place and, once everybody has stopped, return at the gate; a block that straddles a stopped and a
    running utterance selects per row.  n_iter per utterance and H against sklearn_mu_fixed_dictionary / _kl in float64
    (tests/test_gemm_plan_host.py: the stop iterations do not move when tol is halved or doubled)"""
    import exemplars_vc_amd as evc
    n = cus()
    T = stop_frames(esize, n, big)
    W_rows, X_rows, offs = stops_problem(esize, T)
    tol = STOP_TOLS[who][loss]
    ref = stops_reference(W_rows, X_rows, offs, loss, tol)
    want_n = [r[1] for r in ref]
    if who == "some":
        assert want_n == [STOP_ITERS, 4, STOP_ITERS, 4], want_n
    else:
        assert max(want_n) <= STOP_ITERS // 2, want_n
    H, info = evc.solve_activations(W_rows, X_rows, layout="frame_major", iters=STOP_ITERS, eps_mode="zero_replace",
                                    eps=SK_EPS, init="sklearn", algo=algo, loss=loss, check_every=STOP_EVERY,
                                    stop_rule="sklearn", tol=tol, utt_offsets=offs, fused=False, info=True)
    kernel, variant = expected_variant(esize, 40, 128, T, n, algo, loss)
    assert info["kernel"] == kernel and info["redo"] == 0, info
    assert info["variant"] == variant, (info["variant"], variant)
    if n == 256:
        assert variant["update"] == ((128, 128) if esize == 8 else ((64, 128) if big else (64, 64)))
    assert list(info["n_iter"]) == want_n, (list(info["n_iter"]), want_n)
    sc, tl = (score, RTOL) if esize == 4 else (score64, RTOL64)
    for u, (act, _) in enumerate(ref):
        e = sc(H[offs[u]:offs[u + 1]], act)
        print(f"GEMMSTEPS L/{who}/f{8 * esize}/{algo}/{loss}/utt{u} n_iter={want_n[u]} err={e:.3e}")
        assert e <= tl, (u, e)


# ---------------------------------------------------------------------------------------------------------------------
# padding: the 0/0 mode keeps the columns >= N exactly zero
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("esize", [4, 8])
@pytest.mark.parametrize("algo", ["factored", "gram"])
def test_m_zero_padding_stays_exact_without_a_guard(esize, algo):
    """eps_mode='none', N = 200 (Np = 256), T = 100 (Tp = 128) and a zero frame: that frame is 0 after the first step and
    0/0 = NaN from the second on, as in the oracle, and nowhere else - padding columns that left exact zero would turn
    whole frames into NaN through V on the next step"""
    o = oracle()
    K = 4
    A, X, _ = problem(esize, 40, 200, 100, seed=80)
    X[:, 7] = 0
    H0 = start(esize, 200, 100, 81)
    want, _ = reference(A, X, H0, K, "none", algo=algo)
    assert np.isnan(want[:, 7]).all() and np.isfinite(np.delete(want, 7, axis=1)).all()
    run_case(f"M/f{8 * esize}/{algo}", esize, 40, 200, 100, K, seed=80, eps_mode="none", algo=algo, zero_frames=(7,))


def test_no_case_is_skipped_on_256_cus():
    """the largest activations of any case above on 256 CUs: H (4096 x 8192 float32, 128 MiB)"""
    sizes = [4096 * frames_update_shape1(256) * 4, 2048 * frames_update_shape2(256) * 4, 128 * frames_plain_wide(256, 2) * 4,
             128 * frames_plain_wide(256, 1) * 4, 1000 * 2100 * 8, 128 * 11008 * 8]
    assert max(sizes) <= GIB
    if cus() == 256:
        assert frames_update_shape1(256) == 8192 and frames_update_shape2(256) == 3072 and frames_plain_wide(256, 2) == 24576
