"""The four kernels of the dictionary build (csrc/evc_dtw.hip) at every geometry at which they take another path, through
the C ABI, against the plain restatement of tests/dtw_restatement.py.  `-m gpu`.

Every alignment is checked three ways (tests/dtw_cases.py; test_dtw_host.py shows on these inputs that the comparisons
reject wrong kernels): the paths with path_len and total; EVERY cell's local cost (bitwise) and direction byte, read
back from the test-owned workspace, not only the cells the optimal path happens to visit; and the path buffers around
the paths.  Each batch runs once with real-valued features and once with integers in {0, 1, 2}, which make exact ties
common, also across tile borders.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import dtw_cases as K
import dtw_restatement as R

pytestmark = pytest.mark.gpu


def _ip(a):
    return np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int))


def run_align(batch, lda=None, ldb=None, want_total=True):
    """evc_dtw_align on test-owned buffers; returns the image of the call (dtw_cases.emulate's keys)."""
    import torch
    from exemplars_vc_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    lda = batch.D if lda is None else lda
    ldb = batch.D if ldb is None else ldb
    A = torch.from_numpy(batch.packed("a", lda)).to(dev)
    B = torch.from_numpy(batch.packed("b", ldb)).to(dev)
    cap = max(int(batch.poff[-1]), 1)
    pa = torch.full((K.GUARD + cap + K.GUARD,), K.SENTINEL, dtype=torch.int32, device=dev)
    pb = pa.clone()
    plen = torch.full((batch.n,), K.SENTINEL, dtype=torch.int32, device=dev)
    tot = torch.full((batch.n,), K.TOTAL_SENTINEL, dtype=torch.float64, device=dev)
    need = int(L.evc_dtw_workspace_bytes(_ip(batch.aoff), _ip(batch.boff), batch.n))
    assert need == R.workspace_bytes(batch.aoff, batch.boff) > 0
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        st = L.evc_dtw_align(A.data_ptr(), lda, _ip(batch.aoff), B.data_ptr(), ldb, _ip(batch.boff), batch.D, batch.n,
                             pa.data_ptr() + 4 * K.GUARD, pb.data_ptr() + 4 * K.GUARD, plen.data_ptr(),
                             tot.data_ptr() if want_total else None, ws.data_ptr(), need, stream)
        assert st == 0, _lib.strerror(st)
        torch.cuda.synchronize(dev)
    return dict(pa=pa.cpu().numpy(), pb=pb.cpu().numpy(), plen=plen.cpu().numpy(), total=tot.cpu().numpy(),
                ws=ws.cpu().numpy())


def check(img, batch, total=True):
    rep, m = [], batch.models()
    ok = K.paths_equal(img, batch, m, total=total, report=rep)
    ok = K.cells_equal(img, batch, m, report=rep) and ok
    ok = K.buffers_intact(img, batch, m, report=rep) and ok
    assert ok, rep[:12]


# 1. partial tiles in each direction, the 256-column block edge of k_dtw_cost, a path through a tile corner, empty pairs
@pytest.mark.parametrize("kind", K.KINDS)
def test_tile_edges(kind):
    b = K.tile_edge_batch(kind)
    img = run_align(b)
    check(img, b)
    for p, (ta, tb) in enumerate(b.shapes):
        if ta == 0 or tb == 0:
            assert img["plen"][p] == 0 and img["total"][p] == 0.0
    assert [p for p, s in enumerate(b.shapes) if 0 in s] == [0, 10, b.n - 1]


# 2. more than 16 tiles on a tile diagonal: a wavefront takes a second tile
@pytest.mark.parametrize("kind", K.KINDS)
def test_two_tiles_per_wavefront(kind):
    b = K.two_tiles_batch(kind)
    assert min(R.tiles_on_longest_diagonal(*s) for s in b.shapes) > 16
    check(run_align(b), b)


# 3. the largest LDS allocation (raised limit) of k_dtw_accumulate: 120 + 120 tiles of borders
@pytest.mark.parametrize("kind", K.KINDS)
def test_longest_utterances(kind):
    b = K.longest_batch(kind)
    assert R.lds_accumulate(*np.max(b.shapes, axis=0)) > R.LDS_DEFAULT
    check(run_align(b), b)


# 4. feature widths on both sides of k_dtw_cost's raised LDS limit, leading dimensions above D, total = NULL
@pytest.mark.parametrize("kind", K.KINDS)
@pytest.mark.parametrize("D", K.WIDTHS)
def test_feature_widths_and_leading_dimensions(D, kind):
    b = K.width_batch(D, kind)
    check(run_align(b, lda=D + 3, ldb=D + 5), b)          # (the padding holds NaN)
    if D == 25:
        img = run_align(b, want_total=False)
        check(img, b, total=False)
        assert np.all(img["total"] == K.TOTAL_SENTINEL)


# 5. a pair's result does not depend on the batch around it
@pytest.mark.parametrize("kind", K.KINDS)
def test_pair_alone_and_inside_a_batch(kind):
    big, one = K.tile_edge_batch(kind), K.alone_batch(kind)
    p = K.ALONE
    ib, io = run_align(big), run_align(one)
    check(io, one)
    n = int(io["plen"][0])
    ob = K.GUARD + int(big.poff[p])
    assert ib["plen"][p] == n
    assert np.array_equal(ib["pa"][ob:ob + n], io["pa"][K.GUARD:K.GUARD + n])
    assert np.array_equal(ib["pb"][ob:ob + n], io["pb"][K.GUARD:K.GUARD + n])
    assert ib["total"][p:p + 1].view(np.uint64) == io["total"].view(np.uint64)
    lb, lo = R.workspace_layout(big.aoff, big.boff), R.workspace_layout(one.aoff, one.boff)
    s0, s1 = int(lb["doff"][p]), int(lb["doff"][p + 1])
    assert s1 - s0 == lo["cells"]
    # the pair's whole tiles: costs and direction bytes, and the slots no cell owns still hold the fill
    assert np.array_equal(ib["ws"][lb["cost_at"] + 8 * s0:lb["cost_at"] + 8 * s1],
                          io["ws"][lo["cost_at"]:lo["cost_at"] + 8 * lo["cells"]])
    assert np.array_equal(ib["ws"][lb["dir_at"] + s0:lb["dir_at"] + s1], io["ws"][lo["dir_at"]:lo["dir_at"] + lo["cells"]])


# 6. non-finite or overflowing features: unspecified but safe
def test_nonfinite_features_are_safe(tmp_path):
    """The call runs in a process of its own under a time limit: a walk that left the matrix would not come back."""
    out = str(tmp_path / "nonfinite.npz")
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dtw_nonfinite_child.py")
    r = subprocess.run([sys.executable, child, out], timeout=120, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out)
    base = K.three_batch()
    keys = ("pa", "pb", "plen", "total", "ws")
    fin = {k: z[f"finite_{k}"] for k in keys}
    check(fin, base)
    t_fin = float(z["finite_seconds"])
    lay = R.workspace_layout(base.aoff, base.boff)
    (ta, tb), o1, o2 = base.shapes[1], K.GUARD + int(base.poff[1]), K.GUARD + int(base.poff[2])
    for c, (side, frame, value) in enumerate(K.NONFINITE):
        img = {k: z[f"case{c}_{k}"] for k in keys}
        t = float(z[f"case{c}_seconds"])
        print(f"non-finite case {c} ({side}[{frame}] = {value}): {t * 1e3:.3f} ms, finite call {t_fin * 1e3:.3f} ms, "
              f"path_len {int(img['plen'][1])}")
        rep = []
        assert K.buffers_intact(img, base, None, report=rep), rep
        # the outer pairs: paths, totals, every cost and direction byte - and the whole of their path capacity, leftovers
        # of the backwards write included - are bitwise those of the call without the bad pair
        assert K.paths_equal(img, base, base.models(), report=rep, pairs=(0, 2)), rep
        assert K.cells_equal(img, base, base.models(), report=rep, pairs=(0, 2)), rep
        for name in ("pa", "pb"):
            assert np.array_equal(img[name][:o1], fin[name][:o1]) and np.array_equal(img[name][o2:], fin[name][o2:])
        for p in (0, 2):
            s0, s1 = int(lay["doff"][p]), int(lay["doff"][p + 1])
            assert np.array_equal(img["ws"][lay["dir_at"] + s0:lay["dir_at"] + s1], fin["ws"][lay["dir_at"] + s0:lay["dir_at"] + s1])
        # the bad pair: a valid warping path
        n = int(img["plen"][1])
        assert 1 <= n <= ta + tb - 1
        assert R.is_warping_path(img["pa"][o1:o1 + n], img["pb"][o1:o1 + n], ta, tb)
        # the guarded walk takes at most Ta + Tb - 2 steps like any other, so the call costs what the finite call costs;
        # at this size (tens of microseconds of kernel) the wall time is launch and synchronisation jitter, hence the
        # absolute allowance.  A walk without the guard runs on for 2^31 steps: seconds.
        assert t <= 3 * t_fin + 5e-3, (t, t_fin)


# 7. k_path_scan: one element per thread, and several (n_pairs > 1024)
@pytest.mark.parametrize("n_pairs", [1, 1023, 1024, 1025, 2500, 65535])
def test_path_rows(n_pairs):
    import torch
    from exemplars_vc_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(700 + n_pairs)
    lens = rng.integers(0, 3000, n_pairs).astype(np.int32)
    lens[rng.random(n_pairs) < 0.2] = 0
    assert int(lens.astype(np.int64).sum()) < 2 ** 31
    want = np.concatenate([[0], np.cumsum(lens.astype(np.int64))])
    dev = torch.device("cuda", 0)
    d_len = torch.from_numpy(lens).to(dev)
    for given in (True, False):
        rows = torch.full((n_pairs + 1 + 8,), K.SENTINEL, dtype=torch.int32, device=dev)
        n_rows = C.c_int(-1)
        with torch.cuda.device(dev):
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            st = L.evc_dtw_path_rows(d_len.data_ptr(), n_pairs, rows.data_ptr(), C.byref(n_rows) if given else None, stream)
            assert st == 0
            if given:
                assert n_rows.value == want[-1]       # (a given n_rows_out makes the call synchronous)
            torch.cuda.synchronize(dev)
        got = rows.cpu().numpy()
        assert np.array_equal(got[:n_pairs + 1], want) and np.all(got[n_pairs + 1:] == K.SENTINEL)
        assert given or n_rows.value == -1


# 8. k_gather_pairs on synthetic paths
GATHER_LENS = (0, 1, 64, 65, 200, 0, 3)
GATHER_COLS = (1, 255, 256, 257, 1024, 1025, 2100)


@pytest.mark.parametrize("op", [0, 1], ids=["copy", "abs"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_gather_rows(dtype, op):
    import torch
    from exemplars_vc_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    bits = np.uint64 if dtype == np.float64 else np.uint32
    rng = np.random.default_rng(800)
    n = len(GATHER_LENS)
    utt = rng.integers(20, 40, n)                                   # frames of every pair's utterance in src
    src_off = (7 + np.concatenate([[0], np.cumsum(utt)[:-1]])).astype(np.int32)     # non-zero; rows 0..6 belong to nobody
    n_src = 7 + int(utt.sum()) + 3
    pair_off = (11 + np.concatenate([[0], np.cumsum(np.array(GATHER_LENS) + 9)[:-1]])).astype(np.int32)   # with gaps
    path = np.full(int(pair_off[-1]) + GATHER_LENS[-1] + 9, 1 << 30, dtype=np.int32)   # (an index nobody may follow)
    for p, ln in enumerate(GATHER_LENS):
        path[pair_off[p]:pair_off[p] + ln] = rng.integers(0, utt[p], ln)
    lens = np.array(GATHER_LENS, dtype=np.int32)
    row_start = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    N = int(row_start[-1])
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_path, d_len, d_so, d_po = d(path), d(lens), d(src_off), d(pair_off)
    rows = torch.empty(n + 1, dtype=torch.int32, device=dev)
    assert L.evc_dtw_path_rows(d_len.data_ptr(), n, rows.data_ptr(), None, None) == 0
    torch.cuda.synchronize(dev)
    assert np.array_equal(rows.cpu().numpy(), row_start)
    special = np.array([-0.0, -np.inf, 0.0, np.inf], dtype=dtype)
    neg_nan = np.array([0xFFF8000000000123 if dtype == np.float64 else 0xFFC00123], dtype=bits).view(dtype)
    fill = dtype(-4242.5)
    for stride in (1, 2, 3):
        for cols in GATHER_COLS:
            ld_src = (cols - 1) * stride + 1 + 4
            ld_dst = cols + 5
            src = rng.standard_normal((n_src, ld_src)).astype(dtype)
            pick = rng.random(src.shape)
            src[pick < 0.12] = rng.choice(special, int((pick < 0.12).sum()))
            src[pick > 0.94] = neg_nan[0]
            rowsel = np.concatenate([src_off[p] + path[pair_off[p]:pair_off[p] + ln] for p, ln in enumerate(GATHER_LENS)])
            want = src[rowsel][:, 0:(cols - 1) * stride + 1:stride]
            if op == 1:
                want = np.abs(want)
                assert not np.any(np.signbit(want))
            assert want.shape == (N, cols)
            d_src = d(src)
            dst = torch.full((N + 2, ld_dst), float(fill), dtype=d_src.dtype, device=dev)
            with torch.cuda.device(dev):
                stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
                st = L.evc_dtw_gather_rows(d_src.data_ptr(), ld_src, stride, d_path.data_ptr(), d_len.data_ptr(),
                                           d_so.data_ptr(), d_po.data_ptr(), rows.data_ptr(), n, cols, op, dst.data_ptr(),
                                           ld_dst, _lib.F64 if dtype == np.float64 else _lib.F32, stream)
                assert st == 0
                torch.cuda.synchronize(dev)
            got = dst.cpu().numpy()
            where = f"stride {stride} cols {cols}"
            assert np.array_equal(got[:N, :cols].view(bits), np.ascontiguousarray(want).view(bits)), where
            assert np.all(got[:N, cols:] == fill) and np.all(got[N:] == fill), where
