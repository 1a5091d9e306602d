"""The host pieces evc_cd_solve and evc_beta_solve share, without a device.

* The frame-tile table: tests/solve_common_host_main.hip, a program of its own built with the host half of hipcc alone,
  prints what evc::frame_tiles (evc_internal.h) builds; compared with the restatement below at every tile length the two
  entries use, with no offsets, one utterance, an empty first / middle / last utterance, no frames at all, and utterances
  of exactly F and of F + 1 frames.  The count never passes frame_tile_cap, which sizes the workspace.
* The size queries answer what they answered before the two carvers shared that bound:
  tests/golden/solve_workspace_bytes.json, recorded by tools/make_golden_solve_workspace.py on the commit before."""
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import make_golden_solve_workspace as g  # noqa: E402

SRC = os.path.join(ROOT, "tests", "solve_common_host_main.hip")
TILE_LENGTHS = (1, 4, 16, 64)


def cases(F):
    """(T, utt_offsets or None)"""
    T = 2 * F + 3
    return [(T, None), (T, [0, T]), (T, [0, 0, F + 2, T]), (T, [0, F + 2, F + 2, T]), (T, [0, F + 2, T, T]),
            (0, None), (0, [0, 0, 0]), (2 * F + 1, [0, F, 2 * F + 1]), (3 * F + 1, [0, F + 1, F + 1, 3 * F + 1])]


def restated(F, T, offs):
    """numpy-free restatement: (tiles as (utterance, first frame, frames, first tile of the utterance), utt_tile0, utt_frames)"""
    offs = [0, T] if offs is None else offs
    tiles, tile0, frames = [], [], []
    for u, (a, b) in enumerate(zip(offs[:-1], offs[1:])):
        tile0.append(len(tiles))
        frames.append(b - a)
        tiles += [(u, f, min(F, b - f), tile0[u]) for f in range(a, b, F)]
    return tiles, tile0 + [len(tiles)], frames


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc) and not shutil.which(hipcc):
        pytest.fail("hipcc not found: the package cannot be built without it either")
    exe = str(tmp_path_factory.mktemp("solve_common") / "solve_common_host_main")
    p = subprocess.run([hipcc, "--offload-host-only", "-O1", "-std=c++17", SRC, "-o", exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    args = [f"{F}:{T}:" + ("-" if offs is None else ",".join(map(str, offs))) for F in TILE_LENGTHS for T, offs in cases(F)]
    p = subprocess.run([exe] + args, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    lines = [[int(v) for v in ln.split()] for ln in p.stdout.split("\n")[:-1]]
    assert len(lines) == 4 * len(args)
    return {a: lines[4 * i:4 * i + 4] for i, a in enumerate(args)}


@pytest.mark.parametrize("F", TILE_LENGTHS)
def test_frame_tile_table(printed, F):
    for T, offs in cases(F):
        (n, cap, counted), flat, tile0, frames = printed[f"{F}:{T}:" + ("-" if offs is None else ",".join(map(str, offs)))]
        want_tiles, want_tile0, want_frames = restated(F, T, offs)
        print(F, T, offs, "tiles", n, "cap", cap)
        assert n == counted == len(want_tiles) <= cap
        assert [tuple(flat[4 * t:4 * t + 4]) for t in range(n)] == want_tiles
        assert tile0 == want_tile0 and frames == want_frames


with open(g.OUT) as f:
    GOLDEN = json.load(f)


def test_the_fixture_covers_the_grid():
    assert sorted(GOLDEN) == sorted(g.QUERIES)
    for q, limit in zip(g.QUERIES, (1024, 528)):
        rows = GOLDEN[q]
        assert [(r["M"], r["N"], r["T"], r["n_utt"]) for r in rows] == g.GRID
        assert any(r["T"] == 0 and r["f64"] > 0 for r in rows)
        for r in rows:
            assert (r["f64"] > 0) == (r["f32"] > 0) == (r["M"] <= limit), (q, r)


@pytest.mark.parametrize("query", g.QUERIES)
def test_size_queries_answer_what_the_parent_answered(query):
    for want, have in zip(GOLDEN[query], g.answers()[query]):
        print(query, have)
        assert have == want
