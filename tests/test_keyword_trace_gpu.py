"""A context's attributes hold what they held: the `state` cases of tests/golden/make_keyword_trace.py against tests/golden/keyword_trace.json,
recorded on an MI355X by the mirror of commit 6fd518c (see test_keyword_trace_cpu.py) and never regenerated from the restructured one.  Per kind
of context: the kind attributes, the attribute of every option keyword, the sizes (hess_nnz / hess_per, compact_nnz / compact_per, jac_nnz /
jac_per, n_rows) and the window after construction under every keyword state, after set_option(key, 1 / 0 / 1) of every gate option, and after
a one-member window and its reset -- or the error raised instead, code and text.  Contexts are created, options set and sizes asked: nothing is
launched."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_keyword_trace", os.path.join(GOLDEN, "make_keyword_trace.py"))
trace = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(trace)
with open(os.path.join(GOLDEN, "keyword_trace.json")) as f:
    TABLE = json.load(f)
ROWS = [row for row in TABLE["cases"] if row["group"] == "state"]


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=[row["id"] for row in ROWS])
def test_keyword_state(row):
    case = {k: v for k, v in row.items() if k != "expect"}
    want = trace.unpack(row["expect"], TABLE["texts"], TABLE["snaps"])
    got = json.loads(json.dumps(trace.run_case(case)))
    for part in ("construct", "options", "window"):  # name the row that differs
        assert list(got[part]) == list(want[part]), part
        for name in want[part]:
            assert got[part][name] == want[part][name], (part, name)
    assert got == want
