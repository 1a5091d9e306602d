"""Records what the three dictionary-learning entries answer to their size queries: tests/golden/learn_workspace_bytes.json.

For evc_nmf_learn, evc_cd_learn and evc_beta_learn, in float64 and float32, at the shapes below: the bytes of
`*_learn_workspace_bytes`, the frame ranges of `*_learn_splits` and (beta) the route of `evc_beta_learn_route`.  The last
shape of each entry lies beyond its limits, where every query answers 0.  The queries need no device.  Run on the commit
whose answers are to be pinned (a refactor of the host code: its parent); tests/test_learn_common_host.py compares.

    python tools/make_golden_learn_workspace.py [--check]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "learn_workspace_bytes.json")

SHAPES = [(1, 1, 1), (25, 17, 70), (50, 24, 150), (50, 512, 65536), (201, 20, 6880), (513, 16, 40), (528, 4096, 40),
          (1024, 1024, 40), (1056, 16, 40)]
# entry -> (workspace query, splits query, route query or None, a shape beyond its limits)
ENTRIES = {
    "evc_nmf_learn": ("evc_learn_workspace_bytes", "evc_learn_splits", None, (1057, 16, 40)),
    "evc_cd_learn": ("evc_cd_learn_workspace_bytes", "evc_cd_learn_splits", None, (1025, 16, 40)),
    "evc_beta_learn": ("evc_beta_learn_workspace_bytes", "evc_beta_learn_splits", "evc_beta_learn_route", (529, 16, 40)),
}


def answers():
    from exemplars_vc_amd import _lib
    L = _lib.lib()
    out = {}
    for entry, (ws, splits, route, beyond) in ENTRIES.items():
        rows = []
        for M, R, T in SHAPES + [beyond]:
            row = {"M": M, "R": R, "T": T, "f64": int(getattr(L, ws)(M, R, T, _lib.F64)),
                   "f32": int(getattr(L, ws)(M, R, T, _lib.F32)), "splits": int(getattr(L, splits)(M, R, T))}
            if route:
                row["route"] = int(getattr(L, route)(M, R, T))
            rows.append(row)
        out[entry] = rows
    return out


if __name__ == "__main__":
    got = answers()
    if "--check" in sys.argv:
        with open(OUT) as f:
            sys.exit(0 if json.load(f) == got else "the library's answers differ from " + OUT)
    with open(OUT, "w") as f:
        json.dump(got, f, indent=1)
        f.write("\n")
    print(json.dumps(got))
