"""Records what evc_cd_solve and evc_beta_solve answer to their size queries: tests/golden/solve_workspace_bytes.json.

`evc_cd_workspace_bytes` and `evc_beta_workspace_bytes` over a grid of (M, N, T, n_utt) in float64 and float32: no frames,
bins up to each entry's limit and past it (CD_MAX_M = 1024, BETA_MAX_M = 528: the answer is 0), one to many utterances.
The queries need no device.  Run on the commit whose answers are to be pinned (a refactor of the host code: its parent);
tests/test_solve_common_host.py compares.

    python tools/make_golden_solve_workspace.py [--check]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "solve_workspace_bytes.json")

QUERIES = ("evc_cd_workspace_bytes", "evc_beta_workspace_bytes")
BINS = (1, 6, 25, 100, 257, 513, 528, 529, 1024, 1025)
GRID = [(M, N, T, n_utt) for M in BINS for N, T, n_utt in
        ((1, 0, 1), (17, 70, 1), (64, 37, 4), (96, 21, 21), (512, 65536, 1), (4096, 6880, 10))]


def answers():
    from exemplars_vc_amd import _lib
    L = _lib.lib()
    return {q: [{"M": M, "N": N, "T": T, "n_utt": U, "f64": int(getattr(L, q)(M, N, T, U, _lib.F64)),
                 "f32": int(getattr(L, q)(M, N, T, U, _lib.F32))} for M, N, T, U in GRID] for q in QUERIES}


if __name__ == "__main__":
    got = answers()
    if "--check" in sys.argv:
        with open(OUT) as f:
            sys.exit(0 if json.load(f) == got else "the library's answers differ from " + OUT)
    with open(OUT, "w") as f:
        json.dump(got, f)
        f.write("\n")
    print(json.dumps(got))
