"""Host side of the DTW tests (no GPU): the restatement the GPU tests compare with (dtw_restatement.py) against the
oracle, the workspace and tile geometry against the library, the status returns of the C ABI, the unsafe trace-back
shown on the model, and the proof that the comparisons of test_gpu_dtw_tiles.py reject wrong kernels.

Which comparison rejects which mutant, on the tile-edge batch of test_gpu_dtw_tiles.py (case 1):
  (a) lf tested before up          integer data: cells_equal (direction bytes) and paths_equal; real data: not visible
                                   (no exact ties)
  (b) <= instead of <              integer data: cells_equal and paths_equal; real data: not visible
  (c) costs summed downwards       real data: cells_equal (local costs) and paths_equal through `total` (the index paths
      square fused into the add    themselves stay); integer data: not visible (the sums are exact)
  (d) corner handed on as +inf     both: cells_equal and paths_equal (the identical pair's diagonal crosses the corner)
  (e) last row not handed down     both: cells_equal and paths_equal
"""
import ctypes as C

import numpy as np
import pytest

import dtw_cases as K
import dtw_restatement as R


def oracle():
    from oracle import evc_oracle
    return evc_oracle


def lib():
    from exemplars_vc_amd import _lib
    return _lib, _lib.lib()


def _ip(a):
    return np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int))


# ---- the restatement against the oracle ----------------------------------------------------------------------------
def _same_as_oracle(a, b):
    D1, (qa, qb) = oracle().dtw_align(a, b)
    m = R.align(a, b, guarded=True)
    assert m["left"] is None
    assert np.array_equal(m["pa"], qa) and np.array_equal(m["pb"], qb)
    assert np.array_equal(m["D1"].view(np.uint64), D1.view(np.uint64))
    assert R.is_warping_path(m["pa"], m["pb"], len(a), len(b))
    # on finite data the guard changes nothing
    ua, ub, left = R.traceback(m["dirs"], guarded=False)
    assert left is None and np.array_equal(ua, qa) and np.array_equal(ub, qb)


@pytest.mark.parametrize("kind", K.KINDS)
def test_restatement_is_the_oracle_on_tile_edge_shapes(kind):
    b = K.tile_edge_batch(kind)
    n = 0
    for (ta, tb), x, y in zip(b.shapes, b.As, b.Bs):
        if 0 < ta <= 130 and 0 < tb <= 130:
            _same_as_oracle(x, y)
            n += 1
    assert n >= 12


def test_restatement_is_the_oracle_on_the_shapes_of_the_first_dtw_test():
    rng = np.random.default_rng(5)
    for ta, tb in [(40, 25), (1, 1), (1, 17), (23, 1), (64, 64), (37, 90), (130, 97)]:
        for kind in K.KINDS:
            _same_as_oracle(*K._pair(rng, ta, tb, 25 if kind == "real" else 4, kind))
    a = rng.standard_normal((70, 6))
    _same_as_oracle(a, a.copy())                      # identical sequences: the pure diagonal
    assert np.array_equal(R.align(a, a)["pa"], np.arange(70))


def test_identical_pair_of_the_tile_edge_batch_walks_the_diagonal():
    for kind in K.KINDS:
        b = K.tile_edge_batch(kind)
        assert b.shapes[K.IDENT] == (128, 128) and b.shapes[K.ALONE] == (127, 129)
        m = b.models()[K.IDENT]
        if kind == "real":
            assert np.array_equal(m["pa"], np.arange(128)) and np.array_equal(m["pb"], np.arange(128))
        assert m["total"] == 0.0


# ---- geometry -------------------------------------------------------------------------------------------------------
def test_workspace_mirror_is_the_library_for_every_batch_of_the_gpu_tests():
    _, L = lib()
    for b in K.all_finite_batches():
        want = int(L.evc_dtw_workspace_bytes(_ip(b.aoff), _ip(b.boff), b.n))
        assert want == R.workspace_bytes(b.aoff, b.boff) > 0
        lay = R.workspace_layout(b.aoff, b.boff)
        assert lay["used"] <= want
        assert lay["cost_at"] % 256 == 0 and lay["dir_at"] % 16 == 0


def test_gpu_batches_reach_the_branches_they_are_meant_for():
    # two tiles per wavefront, the raised LDS limit of both kernels, and the threshold between D = 127 and 128
    assert [R.tiles_on_longest_diagonal(*s) for s in K.two_tiles_batch("real").shapes] == [18, 17]
    assert all(R.tiles_on_longest_diagonal(*s) <= 16 for s in K.tile_edge_batch("real").shapes)
    mx = np.max(K.longest_batch("real").shapes, axis=0)
    assert tuple(mx) == (R.MAX_FRAMES, R.MAX_FRAMES) and R.lds_accumulate(*mx) == (240 * 64 + 3 * 121) * 8 > R.LDS_DEFAULT
    mx = np.max(K.two_tiles_batch("real").shapes, axis=0)
    assert R.lds_accumulate(*mx) <= R.LDS_DEFAULT
    assert R.lds_accumulate(64 * 47, 64 * 46) <= R.LDS_DEFAULT < R.lds_accumulate(64 * 47, 64 * 47)   # (the corners count)
    assert R.lds_accumulate(1, 1) == R.DTW_TILE + 64
    assert R.lds_cost(127) == R.LDS_DEFAULT < R.lds_cost(128) and R.lds_cost(R.MAX_D) <= 160 * 1024
    assert R.lds_accumulate(R.MAX_FRAMES, R.MAX_FRAMES) <= 160 * 1024


@pytest.mark.parametrize("shape", [(1, 1), (63, 65), (64, 64), (65, 129), (130, 70), (1, 300), (300, 1)])
def test_tile_slot_is_injective_and_in_range(shape):
    ta, tb = shape
    ii, jj = np.indices(shape)
    s = R.tile_slot(ii, jj, ta, tb).ravel()
    assert s.min() >= 0 and s.max() < R.dtw_tiles(ta, tb) * R.DTW_TILE
    assert len(np.unique(s)) == ta * tb
    i, j = ta - 1, tb - 1
    ntj = (tb + 63) // 64
    assert R.tile_slot(i, j, ta, tb) == ((i // 64) * ntj + j // 64) * 127 * 64 + (i % 64 + j % 64) * 64 + i % 64


# ---- status returns, all before any device work --------------------------------------------------------------------
def test_dtw_workspace_query_rejects_bad_offsets():
    _, L = lib()
    q = lambda a, b: int(L.evc_dtw_workspace_bytes(_ip(a), _ip(b), len(a) - 1))
    assert q([0, 7680], [0, 10]) > 0
    assert q([0, 7681], [0, 10]) == 0 and q([0, 10], [0, 7681]) == 0
    assert q([0, 10, 5], [0, 10, 20]) == 0 and q([0, 10, 20], [0, 10, 5]) == 0
    assert q([1, 10], [0, 10]) == 0 and q([0, 10], [1, 10]) == 0
    assert int(L.evc_dtw_workspace_bytes(_ip([0, 10]), _ip([0, 10]), 0)) == 0
    assert R.workspace_bytes([0, 7681], [0, 10]) == 0 and R.workspace_bytes([1, 10], [0, 10]) == 0


def test_dtw_align_rejects_bad_arguments_before_any_device_work():
    _, L = lib()
    one = C.c_void_p(256)
    ao, bo = [0, 40], [0, 25]
    need = int(L.evc_dtw_workspace_bytes(_ip(ao), _ip(bo), 1))

    def call(A=one, lda=5, B=one, ldb=5, D=5, n=1, pa=one, pb=one, plen=one, ws=one, wsb=need, a=ao, b=bo):
        return L.evc_dtw_align(A, lda, _ip(a) if a is not None else None, B, ldb, _ip(b) if b is not None else None, D, n,
                               pa, pb, plen, None, ws, wsb, None)
    assert call(lda=4) == -1 and call(ldb=4) == -1
    assert call(D=0, lda=0, ldb=0) == -1 and call(n=0) == -1
    for k in ("A", "B", "pa", "pb", "plen", "ws", "a", "b"):
        assert call(**{k: None}) == -1, k
    assert call(D=513, lda=513, ldb=513) == -3
    big = np.zeros(65537, dtype=np.int32)
    assert call(n=65536, a=big, b=big) == -3
    assert call(wsb=need - 1) == -2
    assert call(a=[0, 7681]) == -1 and call(a=[1, 40]) == -1


def test_path_rows_and_gather_reject_bad_arguments():
    _lib, L = lib()
    one = C.c_void_p(256)
    assert L.evc_dtw_path_rows(None, 1, one, None, None) == -1
    assert L.evc_dtw_path_rows(one, 1, None, None, None) == -1
    assert L.evc_dtw_path_rows(one, 0, one, None, None) == -1
    assert L.evc_dtw_path_rows(one, 65536, one, None, None) == -1

    def g(src=one, ld_src=20, stride=1, path=one, plen=one, so=one, po=one, rs=one, n=1, cols=10, op=0, dst=one, ld_dst=10,
          dtype=_lib.F64):
        return L.evc_dtw_gather_rows(src, ld_src, stride, path, plen, so, po, rs, n, cols, op, dst, ld_dst, dtype, None)
    assert g(ld_dst=9) == -1
    assert g(stride=2, ld_src=18) == -1 and g(stride=3, ld_src=27) == -1 and g(ld_src=9) == -1
    assert g(op=2) == -1 and g(op=-1) == -1
    assert g(dtype=2) == -1 and g(dtype=-1) == -1
    assert g(cols=0) == -1 and g(stride=0) == -1 and g(n=0) == -1 and g(n=65536) == -1
    for k in ("src", "path", "plen", "so", "po", "rs", "dst"):
        assert g(**{k: None}) == -1, k


# ---- the unsafe trace-back, on the model only ----------------------------------------------------------------------
def _bad_pair(side, frame, value):
    rng = np.random.default_rng(44)
    a, b = rng.standard_normal((70, 5)), rng.standard_normal((50, 5))
    (a if side == "a" else b)[frame, 2] = value
    return a, b


@pytest.mark.parametrize("side", ["a", "b"])
@pytest.mark.parametrize("value", [np.nan, np.inf, 1e200])
def test_unguarded_traceback_leaves_the_matrix_and_the_guarded_one_does_not(side, value):
    a, b = _bad_pair(side, 0, value)
    m = R.align(a, b, guarded=False)
    assert m["left"] is not None and min(m["left"]) == -1, "the first frame's bad value must push the walk off the matrix"
    assert len(m["pa"]) < 70 + 50 - 1
    g = R.align(a, b, guarded=True)
    assert g["left"] is None and R.is_warping_path(g["pa"], g["pb"], 70, 50)
    assert len(g["pa"]) <= 70 + 50 - 1


def test_bad_value_in_a_middle_frame_stays_inside_either_way():
    a, b = _bad_pair("a", 30, np.nan)
    m = R.align(a, b, guarded=False)
    g = R.align(a, b, guarded=True)
    assert m["left"] is None and g["left"] is None
    assert R.is_warping_path(g["pa"], g["pb"], 70, 50)


def test_nonfinite_inputs_of_the_gpu_test_need_the_guard():
    b = K.three_batch()
    needs = []
    for side, frame, value in K.NONFINITE:
        p = K.poisoned(b, side, frame, value)
        m = R.align(p.As[1], p.Bs[1], guarded=False)
        needs.append(m["left"] is not None)
        g = R.align(p.As[1], p.Bs[1], guarded=True)
        assert R.is_warping_path(g["pa"], g["pb"], *p.shapes[1])
        assert p.shapes == b.shapes and all(np.array_equal(x, y) for x, y in zip(p.As[::2], b.As[::2]))
    assert needs == [True, True, True, False]


# ---- the comparisons can tell wrong kernels from right ones ------------------------------------------------------
MUTANTS = {                       # name: (cost mutant, accumulate mutant)
    "a_left_first": (None, "left_first"),
    "b_le": (None, "le"),
    "c_descending": ("descending", None),
    "c_fused": ("fused", None),
    "d_corner_inf": (None, "corner_inf"),
    "e_row_not_handed": (None, "row_not_handed"),
}
# (mutant, data kind) -> (rejected by paths_equal, rejected by cells_equal); every mutant is rejected on one kind at least
REJECTED_BY = {
    ("a_left_first", "real"): (False, False), ("a_left_first", "int"): (True, True),
    ("b_le", "real"): (False, False), ("b_le", "int"): (True, True),
    ("c_descending", "real"): (True, True), ("c_descending", "int"): (False, False),
    ("c_fused", "real"): (True, True), ("c_fused", "int"): (False, False),
    ("d_corner_inf", "real"): (True, True), ("d_corner_inf", "int"): (True, True),
    ("e_row_not_handed", "real"): (True, True), ("e_row_not_handed", "int"): (True, True),
}


def test_the_right_model_passes_every_comparison():
    for kind in K.KINDS:
        b = K.tile_edge_batch(kind)
        img = K.emulate(b, b.models())
        rep = []
        assert K.paths_equal(img, b, b.models(), report=rep) and K.cells_equal(img, b, b.models(), report=rep), rep
        assert K.buffers_intact(img, b, b.models(), report=rep), rep


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_every_mutant_is_rejected_on_the_tile_edge_batch(name):
    cm, am = MUTANTS[name]
    seen = {}
    for kind in K.KINDS:
        b = K.tile_edge_batch(kind)
        wrong = [R.align(x, y, cost_mutant=cm, acc_mutant=am) for x, y in zip(b.As, b.Bs)]
        img = K.emulate(b, wrong)
        seen[kind] = (not K.paths_equal(img, b, b.models()), not K.cells_equal(img, b, b.models()))
        assert seen[kind] == REJECTED_BY[(name, kind)], (name, kind, seen[kind])
    assert any(any(v) for v in seen.values()), f"mutant {name} survives: the inputs are too tame"


def test_buffers_intact_sees_a_write_outside_the_path():
    b = K.tile_edge_batch("int")
    img = K.emulate(b, b.models())
    for where in (K.GUARD - 1, len(img["pa"]) - K.GUARD):
        bad = dict(img, pa=img["pa"].copy())
        bad["pa"][where] = 3
        assert not K.buffers_intact(bad, b, b.models())
    # a path has at least max(Ta, Tb) entries, so it and its backwards copy cover a pair's capacity; the capacity of an
    # empty pair is never written: the one in the middle of the batch is a sentinel region between two pairs
    p = b.shapes.index((5, 0))
    assert img["plen"][p] == 0 and b.shapes[p - 1][0] > 0 and b.shapes[p + 1][0] > 0
    bad = dict(img, pb=img["pb"].copy())
    bad["pb"][K.GUARD + int(b.poff[p]) + 4] = 0
    assert not K.buffers_intact(bad, b, b.models())
