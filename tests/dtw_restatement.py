"""numpy restatement of the DTW alignment that evc_dtw_align runs (csrc/evc_dtw.hip), without its tiling.

k_dtw_cost forms C[i][j] = sum_d (a[i][d] - b[j][d])^2, the D squares summed left to right with a separate multiply and
add.  k_dtw_accumulate forms D[i][j] = C[i][j] + min(D[i-1][j-1], D[i-1][j], D[i][j-1]) and keeps, per cell, WHICH
neighbour was the minimum: m = dg; if (up < m) take up; if (lf < m) take lf - the order (diagonal, i-1, j-1), a strict
`<`, the first minimum wins; a comparison with a NaN never holds.  Here the cells of one anti-diagonal are computed at
once (they only depend on the two anti-diagonals before).  The trace-back walks those bytes from the last cell.

Also the host-side geometry of the kernels: the tile-diagonal-major address of a cell, the carve-up of the workspace
(dtw_run), the dynamic LDS of the two kernels and evc_dtw_workspace_bytes.

`mutant` arguments build deliberately wrong variants; the tests use them to show that their comparisons can tell a
wrong kernel from a right one.
"""
import numpy as np

TILE = 64
DTW_TILE = 127 * 64          # slots of one 64 x 64 tile: 127 cell diagonals of 64 lanes
DTW_IC = 16                  # rows per workgroup of k_dtw_cost
MAX_FRAMES = 64 * 120        # per utterance
MAX_D = 512
MAX_PAIRS = 65535
LDS_DEFAULT = 48 * 1024      # above this a launch raises the kernel's dynamic LDS limit first


def local_costs(a, b, mutant=None):
    """C (Ta, Tb) float64.  mutant: None | 'descending' (d from D-1 down to 0) | 'fused' (the square fused into the
    add: one rounding per step instead of two)."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    Ta, Tb, D = len(a), len(b), a.shape[1] if a.ndim == 2 else 0
    acc = np.zeros((Ta, Tb))
    order = range(D - 1, -1, -1) if mutant == "descending" else range(D)
    with np.errstate(over="ignore", invalid="ignore"):
        for d in order:
            df = a[:, d][:, None] - b[:, d][None, :]
            if mutant == "fused":
                # fma(df, df, acc): exact product and sum, rounded once (longdouble holds the 106-bit product only
                # approximately; two-product splitting keeps it exact)
                acc = _fma(df, df, acc)
            else:
                sq = df * df
                acc = acc + sq
    return acc


def _fma(x, y, z):
    """round(x * y + z) with one rounding, for finite float64 arrays: Dekker's two-product gives x * y = p + e exactly;
    p + e + z is then summed in np.longdouble (64-bit mantissa: enough to decide the rounding in all but contrived
    cases) and rounded once."""
    split = 134217729.0                      # 2^27 + 1
    p = x * y
    xs = x * split; xh = xs - (xs - x); xl = x - xh
    ys = y * split; yh = ys - (ys - y); yl = y - yh
    e = ((xh * yh - p) + xh * yl + xl * yh) + xl * yl
    return (p.astype(np.longdouble) + z.astype(np.longdouble) + e.astype(np.longdouble)).astype(np.float64)


def accumulate(C, mutant=None):
    """(D1 (Ta, Tb) float64, dirs (Ta, Tb) uint8): accumulated costs and the trace-back byte of every cell
    (0 diagonal, 1 up = i-1, 2 left = j-1).
    mutant: None | 'left_first' (lf tested before up) | 'le' (<= instead of <) | 'corner_inf' (the corner value a tile
    hands to the tile down-right of it replaced by +inf) | 'row_not_handed' (the last row of a tile not handed to the
    tile below, which sees +inf)."""
    C = np.asarray(C, dtype=np.float64)
    Ta, Tb = C.shape
    D0 = np.full((Ta + 1, Tb + 1), np.inf)
    D0[0, 0] = 0.0
    dirs = np.zeros((Ta, Tb), dtype=np.uint8)
    less = np.less_equal if mutant == "le" else np.less
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(Ta + Tb - 1):
            i = np.arange(max(0, k - Tb + 1), min(Ta - 1, k) + 1)
            j = k - i
            dg, up, lf = D0[i, j], D0[i, j + 1], D0[i + 1, j]
            if mutant == "corner_inf":
                dg = np.where((i > 0) & (j > 0) & (i % TILE == 0) & (j % TILE == 0), np.inf, dg)
            elif mutant == "row_not_handed":
                # the kernel's lane 0 takes `up` from the row handed down, and the diagonal neighbour of its next cell
                # is that same value one step later; only the tile's first cell has its diagonal from the corner buffer
                top = (i > 0) & (i % TILE == 0)
                up = np.where(top, np.inf, up)
                dg = np.where(top & (j % TILE != 0), np.inf, dg)
            m = dg.copy()
            tb = np.zeros(len(i), dtype=np.uint8)
            first, second = ((lf, 2), (up, 1)) if mutant == "left_first" else ((up, 1), (lf, 2))
            for val, code in (first, second):
                take = less(val, m)
                m = np.where(take, val, m)
                tb = np.where(take, np.uint8(code), tb)
            D0[i + 1, j + 1] = C[i, j] + m
            dirs[i, j] = tb
    return D0[1:, 1:].copy(), dirs


def traceback(dirs, guarded=True):
    """Walk the direction bytes from the last cell.  Returns (path_a, path_b, left): int64 arrays in path order and
    `left` = None, or the (i, j) outside the matrix the walk stepped to (the path then ends at the last cell inside).
    guarded=False is the loop `while (i > 0 || j > 0)` with no lower bound; guarded=True moves left on row 0 and up on
    column 0 whatever the byte says, so every step lowers i or j and neither goes below 0."""
    Ta, Tb = dirs.shape
    if Ta == 0 or Tb == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), None
    i, j = Ta - 1, Tb - 1
    pa, pb = [i], [j]
    left = None
    while i > 0 or j > 0:
        t = int(dirs[i, j])
        if guarded:
            if i == 0:
                t = 2
            elif j == 0:
                t = 1
        if t == 0:
            i -= 1; j -= 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
        if i < 0 or j < 0:
            left = (i, j)
            break
        pa.append(i); pb.append(j)
    return np.array(pa[::-1], dtype=np.int64), np.array(pb[::-1], dtype=np.int64), left


def align(a, b, guarded=True, cost_mutant=None, acc_mutant=None):
    """One pair through the model.  Returns dict(C, D1, dirs, pa, pb, left, total)."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    if len(a) == 0 or len(b) == 0:
        z = np.zeros((len(a), len(b)))
        return dict(C=z, D1=z, dirs=z.astype(np.uint8), pa=np.zeros(0, np.int64), pb=np.zeros(0, np.int64), left=None,
                    total=0.0)
    C = local_costs(a, b, cost_mutant)
    D1, dirs = accumulate(C, acc_mutant)
    pa, pb, left = traceback(dirs, guarded)
    return dict(C=C, D1=D1, dirs=dirs, pa=pa, pb=pb, left=left, total=float(D1[-1, -1]))


def is_warping_path(pa, pb, Ta, Tb):
    """From (0, 0) to (Ta-1, Tb-1) in steps of (1, 1), (1, 0) or (0, 1); hence at most Ta + Tb - 1 entries."""
    pa, pb = np.asarray(pa), np.asarray(pb)
    if len(pa) != len(pb) or len(pa) < 1 or len(pa) > Ta + Tb - 1:
        return False
    if pa[0] != 0 or pb[0] != 0 or pa[-1] != Ta - 1 or pb[-1] != Tb - 1:
        return False
    da, db = np.diff(pa), np.diff(pb)
    return bool(np.all((da >= 0) & (da <= 1) & (db >= 0) & (db <= 1) & (da + db >= 1)))


# ---- geometry of the kernels -----------------------------------------------------------------------------------
def dtw_tiles(Ta, Tb):
    return ((Ta + 63) // 64) * ((Tb + 63) // 64)


def tile_slot(i, j, Ta, Tb):
    """Slot of cell (i, j) in the pair's tile-diagonal-major matrix (scalars or arrays)."""
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    ntj = (Tb + 63) // 64
    I, J, il, jl = i >> 6, j >> 6, i & 63, j & 63
    return (I * ntj + J) * DTW_TILE + (il + jl) * 64 + il


def _up256(n):
    return (n + 255) & ~255


def workspace_layout(aoff, boff):
    """dtw_run's carve-up.  Returns dict: byte positions `aoff_at`, `boff_at`, `doff_at`, `cost_at`, `dir_at`, the
    per-pair slot offsets `doff` (n + 1, int64), `cells` (slots of all pairs) and `used` (bytes up to the last one)."""
    aoff, boff = np.asarray(aoff, dtype=np.int64), np.asarray(boff, dtype=np.int64)
    n = len(aoff) - 1
    Ta, Tb = np.diff(aoff), np.diff(boff)
    doff = np.concatenate([[0], np.cumsum(dtw_tiles(Ta, Tb) * DTW_TILE)]).astype(np.int64)
    cells = int(doff[-1])
    boff_at = _up256(4 * (n + 1))
    doff_at = boff_at + _up256(4 * (n + 1))
    cost_at = doff_at + _up256(8 * (n + 1))
    dir_at = cost_at + 8 * cells
    return dict(aoff_at=0, boff_at=boff_at, doff_at=doff_at, cost_at=cost_at, dir_at=dir_at, doff=doff, cells=cells,
                used=dir_at + cells)


def offsets_ok(off):
    off = np.asarray(off, dtype=np.int64)
    d = np.diff(off)
    return bool(off[0] == 0 and np.all(d >= 0) and np.all(d <= MAX_FRAMES))


def workspace_bytes(aoff, boff):
    """evc_dtw_workspace_bytes: 0 for offsets it rejects."""
    n = len(aoff) - 1
    if n < 1 or not offsets_ok(aoff) or not offsets_ok(boff):
        return 0
    return workspace_layout(aoff, boff)["cells"] * 9 + (n + 1) * 16 + 2048


def lds_cost(D):
    """Dynamic LDS of k_dtw_cost: DTW_IC rows of a, then the block's DTW_IC x 257 costs on their way out."""
    return DTW_IC * (D + 257) * 8


def lds_accumulate(max_ta, max_tb):
    """Dynamic LDS of k_dtw_accumulate: the border rows and columns of the batch's longest utterances and three rows of
    corners; at least the tile of direction bytes the trace-back keeps there."""
    nti, ntj = (max_ta + 63) // 64, (max_tb + 63) // 64
    return max(((nti + ntj) * 64 + 3 * (ntj + 1)) * 8, DTW_TILE + 64)


def tiles_on_longest_diagonal(Ta, Tb):
    """Tiles on the longest tile diagonal: above 16 a wavefront of k_dtw_accumulate takes a second tile."""
    return min((Ta + 63) // 64, (Tb + 63) // 64)
