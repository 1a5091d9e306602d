"""The lean direct exchange of k_fused_quad<7, 2 | 4 | 8> (evc_fused_all_body.inc, the QUAD branch; `-m gpu`).

That exchange keeps the protocol of k_fused_lone's - buffers, offsets, 16-byte words, one epoch bit per 8-byte half,
buffer parity, watch phase, the sums' orders - and drops vector instructions: every fetch round loads all C slots, the
thread's own included, and the tag test is one chain per epoch value.  k_fused_lone (quad_rows=False) still runs the
exchange as it was, and the two kernels' sweeps give the same bits (tests/test_gpu_fused_quad.py prints so for all its
cases), so here H and, through convert, Y of the two must be the same bit for bit.

M = 25, float64, eps_mode="zero_replace", init="sklearn".  Every case checks that evc_solve_info reports k_fused_all, the
member count and no redo.  Shapes are the smallest that reach what each case is about: see the cases.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M = 25
KW = dict(eps_mode="zero_replace", init="sklearn")

_problems = {}


def problem(N, frames):
    key = (N, frames)
    if key not in _problems:
        from oracle import evc_oracle
        p = evc_oracle.synth_problem(M, N, frames, seed=7300 + N // 512 + frames)
        for v in p.values():
            v.setflags(write=False)
        _problems[key] = p
    return _problems[key]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def routed(info, N, launches=1):
    return (info["kernel"], info["members"], info["redo"], info["exchange"], info["launches"]) == \
           ("k_fused_all", N // 512, 0, 1, launches)


def quad_and_lone(A, X, B, N, launches=1, **kw):
    """convert on k_fused_quad and on k_fused_lone: H and Y bit for bit the same, both routed as expected; returns
    k_fused_quad's"""
    import exemplars_vc_amd as evc
    H_on, Y_on, i_on = evc.convert(A, X, B, info=True, quad_rows=True, **KW, **kw)
    H_off, Y_off, i_off = evc.convert(A, X, B, info=True, quad_rows=False, **KW, **kw)
    assert routed(i_on, N, launches) and routed(i_off, N, launches), (i_on, i_off)
    dh, dy = int((bits(H_on) != bits(H_off)).sum()), int((bits(Y_on) != bits(Y_off)).sum())
    print(f"N={N} {kw}: {dh} of {H_on.size} words of H and {dy} of {Y_on.size} words of Y differ")
    assert dh == 0 and dy == 0
    assert np.isfinite(Y_on).all() and (H_on > 0).any()
    return H_on, Y_on


@pytest.mark.parametrize("l1", [0.0, 0.25])
@pytest.mark.parametrize("N", [1024, 2048, 4096])
def test_members_parities_and_epochs(N, l1):
    """2, 4, 8 members: every member index is the thread's own in one workgroup.  Two utterances of 24 and 19 frames: three
    frame tiles, the last ragged - one workgroup's halves both work, another's half works alone.  7 iterations: both
    buffer parities and, the epoch flipping every second exchange, both epoch values."""
    p = problem(N, 43)
    quad_and_lone(p["A"], p["X"], p["B"], N, iters=7, l1=l1, utt_offsets=[0, 24, 43])


def test_a_group_walks_a_second_frame_tile():
    """N = 4096, 16 x 65 + 5 frames in one utterance: 66 frame tiles on at most 64 groups (2 floor(256 / 8)) - `seq` runs
    on across the tiles of a group."""
    p = problem(4096, 16 * 65 + 5)
    quad_and_lone(p["A"], p["X"], p["B"], 4096, iters=5)


def test_three_launches_of_four_are_one_launch_of_twelve():
    """N = 2048: the exchange resumes across the launch boundary."""
    p = problem(2048, 43)
    H3, Y3 = quad_and_lone(p["A"], p["X"], p["B"], 2048, launches=3, iters=12, check_every=4)
    H1, Y1 = quad_and_lone(p["A"], p["X"], p["B"], 2048, launches=1, iters=12)
    assert np.array_equal(bits(H3), bits(H1)) and np.array_equal(bits(Y3), bits(Y1))


def test_the_exact_path_with_an_all_zero_frame():
    """N = 4096, l1 = 0 under zero_replace: the zero frame's activations are 0 after one update and its denominators 0 from
    then on - s_vok and the update's exact path, which sit beside the exchange's code."""
    p = problem(4096, 43)
    X = p["X"].copy()
    X[:, 5] = 0.0
    H, _ = quad_and_lone(p["A"], X, p["B"], 4096, iters=6, l1=0.0)
    assert (H[:, 5] == 0.0).all()
