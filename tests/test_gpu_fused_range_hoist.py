"""The update's range test decided once per sweep (mu_tile_hoisted, evc_fused_common.h; `-m gpu`): k_fused_all and
k_fused_lone with 1, 2, 4 or 8 members against the same kernels with the test in front of every unit
(range_hoist=False, EVC_FLAG_NO_RANGE_HOIST).

The switch must not change one bit: with the flag set the fast quotients are the instructions the per-unit test would
have let through, and without it (a member that is not tame, a V with an element outside [2^-100, 2^100), a tile's first
sweep) the unit is the old code.  So every case asserts np.array_equal of H between switch on and switch off, and of H
and Y through convert(); the parity tests of the other files remain the yardstick against the oracle.

float64, T = 40 frames in two utterances of 23 and 17 (the frame tiles mix utterances and end in padding frames, whose V
is zero: those tiles keep the per-unit test), 30 iterations.  Cases, each taking the fall-back for its own reason:
plain positive data (the hoisted path); one utterance scaled by 2^-700 (V below the range, the exact path); an all-zero
frame; a NaN in X; N = 1000 and 4000 (padding exemplars in the last member); a dictionary with a zero column and one with
a negative entry (solve_activations hands the dictionary to the C entry as it is); CLAMP with eps = 1e-3 (not tame);
l1 = 0.25.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T, K, UTT = 40, 30, [0, 23, 40]

_problems = {}


def problem(M, N):
    if (M, N) not in _problems:
        rng = np.random.default_rng(9000 + 64 * M + N // 8)
        A = rng.random((M, N)) + 0.05
        A /= np.linalg.norm(A, axis=0)
        B = rng.random((M, N)) + 0.05
        Hs = np.where(rng.random((N, T)) < 8.0 / N, rng.random((N, T)), 0.0)
        X = A @ Hs + 1e-3 * rng.random((M, T))
        for v in (A, B, X):
            v.setflags(write=False)
        _problems[(M, N)] = (A, B, X)
    return _problems[(M, N)]


def plain(A, X):
    return A, X, {}


def tiny_utterance(A, X):
    X = X.copy()
    X[:, :23] *= 2.0 ** -700
    return A, X, {}


def zero_frame(A, X):
    X = X.copy()
    X[:, 5] = 0.0
    return A, X, {}


def nan_in_x(A, X):
    X = X.copy()
    X[3, 27] = np.nan
    return A, X, {}


def zero_column(A, X):
    A = A.copy()
    A[:, 17] = 0.0
    return A, X, {}


def negative_entry(A, X):
    A = A.copy()
    A[2, A.shape[1] - 100] = -0.01
    return A, X, {}


def clamp(A, X):
    return A, X, dict(eps_mode="clamp", eps=1e-3)


def l1(A, X):
    return A, X, dict(l1=0.25)


CASES = [plain, tiny_utterance, zero_frame, nan_in_x, zero_column, negative_entry, clamp, l1]


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def check(M, N, case):
    import exemplars_vc_amd as evc
    A, B, X = problem(M, N)
    A, X, more = case(A, X)
    kw = dict(iters=K, eps_mode="zero_replace", utt_offsets=UTT)
    kw.update(more)
    what = f"M={M} N={N} {case.__name__}"
    H_on, i_on = evc.solve_activations(A, X, range_hoist=True, info=True, **kw)
    H_off, i_off = evc.solve_activations(A, X, range_hoist=False, info=True, **kw)
    members = (N + 511) // 512
    for i in (i_on, i_off):
        assert (i["kernel"], i["members"], i["redo"]) == ("k_fused_all", members, 0), (what, i)
    assert same(H_on, H_off), what
    if case is plain:
        assert np.isfinite(H_on).all() and (H_on >= 0.0).all() and H_on.any(), what
    Hc_on, Y_on, j_on = evc.convert(A, X, B, range_hoist=True, info=True, **kw)
    Hc_off, Y_off, j_off = evc.convert(A, X, B, range_hoist=False, info=True, **kw)
    for i in (j_on, j_off):
        assert (i["kernel"], i["members"], i["redo"]) == ("k_fused_all", members, 0), (what, i)
    assert same(Hc_on, Hc_off) and same(Hc_on, H_on), what
    assert same(Y_on, Y_off), what


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.__name__)
@pytest.mark.parametrize("N", [512, 1024, 2048, 4096])
@pytest.mark.parametrize("M", [25, 20])
def test_the_switch_changes_no_bit(M, N, case):
    check(M, N, case)


@pytest.mark.parametrize("N", [1000, 4000])
@pytest.mark.parametrize("M", [25, 20])
def test_padding_exemplars_in_the_last_member(M, N):
    check(M, N, plain)
