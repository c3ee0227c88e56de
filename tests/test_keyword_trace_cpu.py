"""The constructors of the Python mirror answer every combination of their service keywords as they did: the `checks` cases of
tests/golden/make_keyword_trace.py against tests/golden/keyword_trace.json.  That table was written by the mirror of commit 6fd518c -- the
commit BEFORE its per-keyword check functions and their three call ladders became the one table _SERVICES of integrators.py -- and is committed
unchanged with that restructuring: it is never regenerated from the restructured mirror.  Equality throughout: the ValueError's full text (so
which rule wins when two are broken at once), "reached" where the library would have been loaded, the class of any other exception."""
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
ROWS = [row for row in TABLE["cases"] if row["group"] == "checks"]


def test_table_is_of_these_cases():
    assert [{k: v for k, v in row.items() if k != "expect"} for row in TABLE["cases"]] == trace.CASES
    assert {k: TABLE[k] for k in trace.header()} == json.loads(json.dumps(trace.header()))
    for row in ROWS:
        assert len(row["expect"]) == len(trace.grid(row["ctor"]))
    for row in TABLE["cases"]:
        if row["group"] == "state":
            assert list(row["expect"]["construct"]) == TABLE["states"][row["kind"]] and list(row["expect"]["options"]) == trace.GATE_KEYS
            assert set(row["expect"]["window"]) <= set(row["expect"]["construct"]) and bool(row["expect"]["window"]) == (TABLE["kinds"][row["kind"]][6] > 1)


@pytest.mark.parametrize("row", ROWS, ids=[row["id"] for row in ROWS])
def test_keyword_checks(row):
    case = {k: v for k, v in row.items() if k != "expect"}
    want = trace.unpack(row["expect"], TABLE["texts"], TABLE["snaps"])
    got = trace.run_case(case)
    for cell, g, w in zip(trace.grid(row["ctor"]), got, want):  # name the combination that differs
        assert g == w, cell
    assert got == want
