"""The end of a frame tile in k_fused_all's last launch (evc_fused_all.hip, round 9; `-m gpu`): the members' shares of
Y = B H formed from the activations in registers and summed by k_unpack_y, the packed activations not stored when
nothing reads them, and the caller's frame-major H written with 16-byte stores.

Shapes: two utterances of 37 and 50 frames - six frame tiles, the third spanning both utterances, the last one with
padding frames - and 3 to 5 iterations: the tile's end runs once per tile whatever the iteration count.  Tolerance of Y:
RTOL64 of tests/test_gpu_parity.py's convert checks (float64, pure relative, against B @ H in float64 on the host; Y
differs from it in summation order only).  H must not change at all: it is compared bit for bit.
"""
import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu

RTOL64 = 1e-8
OFFS = [0, 37, 87]
T = OFFS[-1]
IN_KERNEL = {"y_in_kernel": True, "packed_h_stored": False}


def oracle():
    from oracle import evc_oracle
    return evc_oracle


def assert_close64(got, want, what, rtol=RTOL64):
    r, z = rel_err(got, want)
    print(f"{what}: max rel err {r:.3e}, max |got| where want==0 {z:.3e}")
    assert r <= rtol and z == 0.0, f"{what}: max rel err {r:.3e}, max |got| where want==0 {z:.3e}"


_problems = {}


def problem(M, N, Mb=None):
    key = (M, N, Mb)
    if key not in _problems:
        p = oracle().synth_problem(M, N, T, Mb=Mb, seed=900 + M + N + (Mb or 0))
        for v in p.values():
            v.setflags(write=False)
        _problems[key] = p
    return _problems[key]


KW = dict(iters=4, eps_mode="zero_replace", init="sklearn", utt_offsets=OFFS)


@pytest.mark.parametrize("M,Mb,N,members,in_kernel", [
    (25, 25, 512, 1, True),
    (25, 25, 1024, 2, True),
    (25, 25, 1536, 3, True),          # ragged slices
    (25, 25, 2048, 4, True),
    (25, 25, 4096, 8, True),
    (25, 25, 8192, 16, True),
    (12, 12, 2048, 4, True),          # one row tile
    (28, 28, 4096, 8, True),          # streamed dictionary, reduce-scatter
    (25, 1, 2048, 4, True),
    (25, 32, 2048, 4, True),          # B has one k-step more than A
    (12, 25, 2048, 4, False),         # Mb > 16 MT: B's bins do not fit the instance's row tiles - two passes
])
def test_y_of_convert_is_b_times_the_returned_h(M, Mb, N, members, in_kernel):
    import exemplars_vc_amd as evc
    p = problem(M, N, Mb)
    H, Y, info = evc.convert(p["A"], p["X"], p["B"], info=True, **KW)
    assert (info["kernel"], info["members"], info["redo"]) == ("k_fused_all", members, 0), info
    assert info["variant"] == (IN_KERNEL if in_kernel else None), info
    assert Y.shape == (Mb, T) and np.isfinite(Y).all() and (H >= 0).all()
    assert_close64(Y, p["B"] @ H, f"Y, M={M} Mb={Mb} N={N}")
    assert np.array_equal(H, evc.solve_activations(p["A"], p["X"], **KW))


@pytest.mark.parametrize("N", [1535, 2048, 4000, 4090])
@pytest.mark.parametrize("layout", ["bin_major", "frame_major"])
def test_h_of_convert_is_h_of_solve_bitwise(N, layout):
    """N = 1535: an odd leading dimension (frame-major: the 8-byte stores); 4000, 4090: the exemplars end inside a
    member, 4090 inside a lane's second pair.  `out` 8 bytes off a 16-byte boundary takes the 8-byte stores too: the
    same bits either way."""
    import torch
    import exemplars_vc_amd as evc
    p = problem(25, N)
    tr = (lambda a: np.ascontiguousarray(a.T)) if layout == "frame_major" else (lambda a: a)
    A, X, B = tr(p["A"]), tr(p["X"]), tr(p["B"])
    kw = dict(KW, layout=layout, iters=3)
    want = evc.solve_activations(A, X, **kw)
    H, Y, info = evc.convert(A, X, B, info=True, **kw)
    assert info["kernel"] == "k_fused_all" and info["variant"] == IN_KERNEL, info
    assert np.array_equal(H, want)
    assert_close64(Y, B @ H if layout == "bin_major" else H @ B, f"Y, N={N} {layout}")
    flat = torch.zeros(H.size + 3, dtype=torch.float64, device="cuda")
    for off in (1, 2):                               # 8 bytes off / on a 16-byte boundary
        out = flat[off:off + H.size].view(*H.shape)
        assert out.data_ptr() % 16 == 8 * (off % 2)
        out.fill_(-1.0)
        evc.convert(A, X, B, out=out, **kw)
        assert np.array_equal(out.cpu().numpy(), want), off
        out.fill_(-1.0)
        evc.solve_activations(A, X, out=out, **kw)
        assert np.array_equal(out.cpu().numpy(), want), off
    assert float(flat[0]) == 0.0 and float(flat[-1]) == 0.0          # nothing written around the view


@pytest.mark.parametrize("N", [512, 4096])
def test_convert_without_h(N):
    import exemplars_vc_amd as evc
    p = problem(25, N)
    si = {}
    Y = evc.convert(p["A"], p["X"], p["B"], want_h=False, solve_info=si, **KW)
    assert si["kernel"] == "k_fused_all" and si["variant"] == IN_KERNEL, si
    assert_close64(Y, p["B"] @ evc.solve_activations(p["A"], p["X"], **KW), f"Y only, N={N}")


def test_convert_with_given_start_values_keeps_the_packed_store():
    """caller-given start values: H leaves through the export pass behind the abort check, which reads the packed tiles"""
    import exemplars_vc_amd as evc
    p = problem(25, 2048)
    H0 = np.random.default_rng(3).random((2048, T)) + 1e-4
    kw = dict(KW, init="given")
    H, Y, info = evc.convert(p["A"], p["X"], p["B"], H0.copy(), info=True, **kw)
    assert info["variant"] == {"y_in_kernel": True, "packed_h_stored": True}, info
    assert np.array_equal(H, evc.solve_activations(p["A"], p["X"], H0.copy(), **kw))
    assert_close64(Y, p["B"] @ H, "Y, given start values")


def test_convert_under_a_stop_rule_takes_the_two_pass_path():
    """a stop rule with check_every: utterances may stop, later launches and the general kernel read the packed tiles"""
    import exemplars_vc_amd as evc
    p = problem(25, 4096)
    kw = dict(KW, iters=5, check_every=2, stop_rule="sklearn", tol=1e-12)
    H, Y, info = evc.convert(p["A"], p["X"], p["B"], info=True, **kw)
    assert info["kernel"] == "k_fused_all" and info["variant"] is None and info["launches"] == 3, info
    Hs, i2 = evc.solve_activations(p["A"], p["X"], info=True, **kw)
    assert np.array_equal(H, Hs) and np.array_equal(info["n_iter"], i2["n_iter"])
    assert_close64(Y, p["B"] @ H, "Y under a stop rule")
    # errors recorded but nothing can stop: three launches, the first two store the packed tiles, the last one forms Y
    kw = dict(KW, iters=5, check_every=2)
    H2, Y2, info = evc.convert(p["A"], p["X"], p["B"], info=True, **kw)
    assert info["variant"] == IN_KERNEL and info["launches"] == 3, info
    H1, Y1 = evc.convert(p["A"], p["X"], p["B"], **dict(KW, iters=5))
    assert np.array_equal(H2, H1) and np.array_equal(Y2, Y1)
    assert_close64(Y2, p["B"] @ H2, "Y with recorded errors")


@pytest.mark.parametrize("when,extra", [(True, {}), (1, {"check_every": 2})])
def test_convert_redone_after_a_voided_exchange(when, extra):
    """test_abort_at: a peer that does not arrive - from the start of the call, or (two launches of two iterations) in
    front of the second launch, the one whose tile ends form Y.  The redo runs without exchange and delivers what such
    a call does."""
    import exemplars_vc_amd as evc
    p = problem(25, 4096)
    kw = dict(KW, **extra)
    Hw, Yw, iw = evc.convert(p["A"], p["X"], p["B"], cooperative=False, info=True, **kw)
    H, Y, info = evc.convert(p["A"], p["X"], p["B"], _fake_coop_timeout=when, info=True, **kw)
    assert info["redo"] == 1 and info["exchange"] == 0 and iw["redo"] == 0, (info, iw)
    assert np.array_equal(H, Hw) and np.array_equal(Y, Yw)
    assert_close64(Y, p["B"] @ H, "Y after the redo")
