"""The size queries of the three dictionary-learning entries answer what they answered before their drivers shared one
workspace carver and one padding rule: tests/golden/learn_workspace_bytes.json, recorded by
tools/make_golden_learn_workspace.py on the commit before that change.  No device needed."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import make_golden_learn_workspace as g  # noqa: E402

with open(g.OUT) as f:
    GOLDEN = json.load(f)


def test_the_fixture_covers_every_entry_and_shape():
    assert sorted(GOLDEN) == sorted(g.ENTRIES)
    for entry, rows in GOLDEN.items():
        assert [(r["M"], r["R"], r["T"]) for r in rows] == g.SHAPES + [g.ENTRIES[entry][3]]
        assert rows[1]["f64"] > 0 and rows[1]["f32"] > 0 and rows[1]["splits"] == 1
        assert all(v == 0 for k, v in rows[-1].items() if k not in "MRT")      # beyond the entry's limits


@pytest.mark.parametrize("entry", sorted(g.ENTRIES))
def test_size_queries_answer_what_the_parent_answered(entry):
    got = g.answers()[entry]
    for want, have in zip(GOLDEN[entry], got):
        print(entry, have)
        assert have == want
