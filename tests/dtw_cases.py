"""Inputs and comparisons shared by test_dtw_host.py (CPU) and test_gpu_dtw_tiles.py (GPU).

A `Batch` is a list of utterance pairs as evc_dtw_align takes them.  An *image* is everything one call leaves behind:
the path buffers (with a guard region in front and behind), path_len, total and the raw workspace, which holds the local
costs and the direction bytes of every cell.  The GPU test reads an image back from the device; `emulate` builds the
image the restatement (or a mutant of it) would leave, so the very comparisons the GPU test asserts can be shown to
reject wrong kernels on the very inputs it uses.
"""
import functools

import numpy as np

import dtw_restatement as R

GUARD = 96                     # ints in front of and behind the path buffers
SENTINEL = -77777              # never a frame index
TOTAL_SENTINEL = -1.25e300     # never an accumulated cost


class Batch:
    def __init__(self, pairs):
        self.As = [np.ascontiguousarray(a, dtype=np.float64) for a, _ in pairs]
        self.Bs = [np.ascontiguousarray(b, dtype=np.float64) for _, b in pairs]
        self.n = len(pairs)
        self.D = self.As[0].shape[1]
        self.aoff = np.concatenate([[0], np.cumsum([len(a) for a in self.As])]).astype(np.int32)
        self.boff = np.concatenate([[0], np.cumsum([len(b) for b in self.Bs])]).astype(np.int32)
        self.poff = (self.aoff + self.boff).astype(np.int64)      # pair p's first path slot; capacity Ta + Tb
        self.shapes = [(len(a), len(b)) for a, b in zip(self.As, self.Bs)]

    def packed(self, side, ld=None, pad=np.nan):
        """All frames of one side as rows of stride ld >= D; the padding columns hold `pad`."""
        rows = np.concatenate(self.As if side == "a" else self.Bs, axis=0).reshape(-1, self.D)
        ld = self.D if ld is None else ld
        out = np.full((max(len(rows), 1), ld), pad, dtype=np.float64)
        out[:len(rows), :self.D] = rows
        return out

    @functools.lru_cache(maxsize=None)
    def models(self):
        """The restatement of every pair (computed once, shared, never modified)."""
        return tuple(R.align(a, b) for a, b in zip(self.As, self.Bs))


def _pair(rng, ta, tb, D, kind):
    if kind == "int":          # exact ties in the accumulated costs are common, also across tile borders
        return rng.integers(0, 3, (ta, D)).astype(np.float64), rng.integers(0, 3, (tb, D)).astype(np.float64)
    # two noisy resamplings of one random walk: the optimal path wanders off the diagonal
    base = np.cumsum(rng.standard_normal((max(ta, tb) + 8, D)), axis=0)
    ia = np.sort(rng.choice(len(base), ta, replace=True))
    ib = np.sort(rng.choice(len(base), tb, replace=True))
    return base[ia] + 0.05 * rng.standard_normal((ta, D)), base[ib] + 0.05 * rng.standard_normal((tb, D))


KINDS = ("real", "int")

# case 1: every partial-tile geometry, the 256-column block edge of k_dtw_cost, empty pairs first / middle / last and
# one pair of identical sequences (index IDENT) whose path is the pure diagonal through the tile corner
TILE_EDGE_SHAPES = [(0, 5), (63, 63), (64, 64), (64, 65), (65, 64), (65, 65), (127, 129), (128, 128), (129, 127),
                    (1, 64), (5, 0), (1, 65), (64, 1), (65, 1), (1, 300), (300, 1), (16, 257), (17, 256), (15, 513),
                    (128, 128), (0, 0)]
IDENT = 19
ALONE = 6                      # the pair of case 5 (127 x 129: four tiles, partial in both directions)


@functools.lru_cache(maxsize=None)
def tile_edge_batch(kind):
    rng = np.random.default_rng(101 if kind == "real" else 102)
    pairs = [_pair(rng, ta, tb, 3, kind) for ta, tb in TILE_EDGE_SHAPES]
    pairs[IDENT] = (pairs[IDENT][0], pairs[IDENT][0].copy())
    return Batch(pairs)


@functools.lru_cache(maxsize=None)
def alone_batch(kind):
    b = tile_edge_batch(kind)
    return Batch([(b.As[ALONE], b.Bs[ALONE])])


# case 2: 18 and 17 tiles on the longest tile diagonal: a wavefront of k_dtw_accumulate takes a second tile
@functools.lru_cache(maxsize=None)
def two_tiles_batch(kind):
    rng = np.random.default_rng(201 if kind == "real" else 202)
    return Batch([_pair(rng, 1100, 1100, 2, kind), _pair(rng, 1030, 2050, 2, kind)])


# case 3: the launch sizes LDS by the maxima over the batch: 120 + 120 tile borders without a 7680 x 7680 matrix
@functools.lru_cache(maxsize=None)
def longest_batch(kind):
    rng = np.random.default_rng(301 if kind == "real" else 302)
    return Batch([_pair(rng, 7680, 1, 3, kind), _pair(rng, 1, 7680, 3, kind), _pair(rng, 40, 25, 3, kind)])


# case 4: feature widths around the 48 KiB LDS threshold of k_dtw_cost (D = 127 | 128) and the supported maximum
WIDTHS = (1, 2, 25, 127, 128, 512)


@functools.lru_cache(maxsize=None)
def width_batch(D, kind):
    rng = np.random.default_rng(400 + D + (0 if kind == "real" else 1000))
    return Batch([_pair(rng, 70, 300, D, kind)])


# case 6: a batch of three; the middle pair is replaced by copies with one non-finite or overflowing feature
NONFINITE = (("a", 0, np.nan), ("b", 0, np.inf), ("a", 0, 1e200), ("a", 30, np.nan))


@functools.lru_cache(maxsize=None)
def three_batch():
    rng = np.random.default_rng(601)
    return Batch([_pair(rng, 40, 25, 5, "real"), _pair(rng, 70, 50, 5, "real"), _pair(rng, 65, 33, 5, "real")])


def poisoned(batch, side, frame, value, col=2):
    pairs = [(a.copy(), b.copy()) for a, b in zip(batch.As, batch.Bs)]
    (pairs[1][0] if side == "a" else pairs[1][1])[frame, col] = value
    return Batch(pairs)


def all_finite_batches():
    """Every batch whose image is compared with the restatement (the workspace-size check walks these too)."""
    out = []
    for kind in KINDS:
        out += [tile_edge_batch(kind), alone_batch(kind), two_tiles_batch(kind), longest_batch(kind)]
        out += [width_batch(D, kind) for D in WIDTHS]
    return out + [three_batch()]


# ---- the image of a call ---------------------------------------------------------------------------------------
def emulate(batch, models):
    """The image `models` (one R.align result per pair) would leave: paths written backwards into the end of the
    pair's capacity, then moved to its front; costs and direction bytes at their tile-diagonal-major slots."""
    cap_all = int(batch.poff[-1])
    pa = np.full(GUARD + max(cap_all, 1) + GUARD, SENTINEL, dtype=np.int32)
    pb = pa.copy()
    plen = np.zeros(batch.n, dtype=np.int32)
    total = np.full(batch.n, TOTAL_SENTINEL)
    lay = R.workspace_layout(batch.aoff, batch.boff)
    ws = np.full(R.workspace_bytes(batch.aoff, batch.boff), 0xA5, dtype=np.uint8)
    ws[lay["doff_at"]:lay["doff_at"] + 8 * (batch.n + 1)] = lay["doff"].view(np.uint8)
    cost = ws[lay["cost_at"]:lay["cost_at"] + 8 * lay["cells"]].view(np.float64)
    dirs = ws[lay["dir_at"]:lay["dir_at"] + lay["cells"]]
    for p, ((Ta, Tb), m) in enumerate(zip(batch.shapes, models)):
        n, cap, o = len(m["pa"]), Ta + Tb, GUARD + int(batch.poff[p])
        plen[p] = n
        total[p] = m["total"]
        for buf, path in ((pa, m["pa"]), (pb, m["pb"])):
            buf[o + cap - n:o + cap] = path
            buf[o:o + n] = path
        if Ta and Tb:
            ii, jj = np.indices((Ta, Tb))
            s = lay["doff"][p] + R.tile_slot(ii, jj, Ta, Tb)
            cost[s] = m["C"]
            dirs[s] = m["dirs"]
    return dict(pa=pa, pb=pb, plen=plen, total=total, ws=ws)


def _note(report, msg):
    if report is not None:
        report.append(msg)
    return False


def paths_equal(img, batch, models, total=True, report=None, pairs=None):
    """path_len and the first path_len entries of both paths are the models'; with total=True the accumulated cost of
    the last cell is bitwise the models' (0 for an empty pair)."""
    ok = True
    for p in (range(batch.n) if pairs is None else pairs):
        m, o = models[p], GUARD + int(batch.poff[p])
        n = int(img["plen"][p])
        if n != len(m["pa"]):
            ok = _note(report, f"pair {p} {batch.shapes[p]}: path_len {n}, want {len(m['pa'])}")
            continue
        if not (np.array_equal(img["pa"][o:o + n], m["pa"]) and np.array_equal(img["pb"][o:o + n], m["pb"])):
            ok = _note(report, f"pair {p} {batch.shapes[p]}: path differs")
        if total and np.float64(img["total"][p]).view(np.uint64) != np.float64(m["total"]).view(np.uint64):
            ok = _note(report, f"pair {p} {batch.shapes[p]}: total {img['total'][p]!r}, want {m['total']!r}")
    return ok


def cells_equal(img, batch, models, report=None, pairs=None):
    """Every valid cell of every pair: the local cost in the workspace is bitwise the models', the direction byte is
    the models'.  The slots of the layout no cell owns are not compared.  The per-pair slot offsets the device formed
    are the layout's."""
    lay = R.workspace_layout(batch.aoff, batch.boff)
    ws = img["ws"]
    ok = True
    doff = ws[lay["doff_at"]:lay["doff_at"] + 8 * (batch.n + 1)].view(np.int64)
    if not np.array_equal(doff, lay["doff"]):
        return _note(report, "slot offsets of the pairs differ from the layout")
    cost = ws[lay["cost_at"]:lay["cost_at"] + 8 * lay["cells"]].view(np.uint64)
    dirs = ws[lay["dir_at"]:lay["dir_at"] + lay["cells"]]
    for p in (range(batch.n) if pairs is None else pairs):
        Ta, Tb = batch.shapes[p]
        if not (Ta and Tb):
            continue
        ii, jj = np.indices((Ta, Tb))
        s = lay["doff"][p] + R.tile_slot(ii, jj, Ta, Tb)
        bad = cost[s] != np.ascontiguousarray(models[p]["C"]).view(np.uint64)
        if bad.any():
            i, j = np.argwhere(bad)[0]
            ok = _note(report, f"pair {p} {batch.shapes[p]}: {int(bad.sum())} local costs differ, first at ({i}, {j})")
        bad = dirs[s] != models[p]["dirs"]
        if bad.any():
            i, j = np.argwhere(bad)[0]
            ok = _note(report, f"pair {p} {batch.shapes[p]}: {int(bad.sum())} direction bytes differ, first at ({i}, {j}): "
                               f"{dirs[s][i, j]} for {models[p]['dirs'][i, j]}")
    return ok


def buffers_intact(img, batch, models=None, report=None):
    """The guards in front of and behind the path buffers are untouched.  Per pair of capacity Ta + Tb and length n:
    the slots [n, capacity - n) were never written (the walk writes the last n slots, the move the first n; what lies
    beyond is a leftover of the backwards write and is not asserted), the first n entries are frame indices of the
    pair and, given models, the models' path."""
    ok = True
    cap_all = int(batch.poff[-1])
    for name in ("pa", "pb"):
        buf = img[name]
        if not (np.all(buf[:GUARD] == SENTINEL) and np.all(buf[GUARD + max(cap_all, 1):] == SENTINEL)):
            ok = _note(report, f"{name}: guard region overwritten")
        for p, (Ta, Tb) in enumerate(batch.shapes):
            o, cap, n = GUARD + int(batch.poff[p]), Ta + Tb, int(img["plen"][p])
            if n < 0 or n > cap:
                ok = _note(report, f"pair {p}: path_len {n} outside its capacity {cap}")
                continue
            if not np.all(buf[o + n:o + max(cap - n, n)] == SENTINEL):
                ok = _note(report, f"{name} pair {p} {batch.shapes[p]}: a slot between the path and its backwards copy was written")
            head = buf[o:o + n]
            if n and not (head.min() >= 0 and head.max() < (Ta if name == "pa" else Tb)):
                ok = _note(report, f"{name} pair {p}: entries outside the utterance")
            if models is not None and not np.array_equal(head, models[p][name]):
                ok = _note(report, f"{name} pair {p} {batch.shapes[p]}: path differs")
    return ok
