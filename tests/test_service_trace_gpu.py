"""Every kind of context serves what it served and refuses the rest in the words it used: every case of tests/golden/make_service_trace.py
against tests/golden/service_trace.json.  That table was written by the library of commit 07bcae2 -- the commit BEFORE the refusal macros
became the one service table of pcl_host_service.hpp and the two option chains one table of keys -- and is committed unchanged with that
restructuring: it is never regenerated from the restructured library (a late case is recorded from a build of that commit).  Equality
throughout: the code and the pcl_last_error text of every call (which check fires first included), every option's code, text, read-back
code and read-back value for every value tried, the read-only keys, last_kernel behind the host route."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_service_trace", os.path.join(GOLDEN, "make_service_trace.py"))
trace = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(trace)
with open(os.path.join(GOLDEN, "service_trace.json")) as f:
    TABLE = json.load(f)


def test_table_is_of_these_cases():
    assert [{k: v for k, v in row.items() if k != "expect"} for row in TABLE["cases"]] == trace.CASES
    assert (TABLE["calls"], TABLE["values"], TABLE["keys"], TABLE["last"]) == (trace.CALLS, trace.VALUES, trace.KEYS, trace.LAST)
    for row in TABLE["cases"]:
        if row["group"] == "options":
            assert len(row["expect"]) == len(trace.KEYS)
        if row["group"] == "readonly":
            assert len(row["expect"]["fresh"]) == len(trace.KEYS) and len(row["expect"]["after"]) == len(trace.KEYS)


@pytest.mark.gpu
@pytest.mark.parametrize("row", TABLE["cases"], ids=[row["id"] for row in TABLE["cases"]])
def test_service_trace(row):
    case = {k: v for k, v in row.items() if k != "expect"}
    want = trace.unpack(row["expect"], row["group"], TABLE["texts"], TABLE["patterns"])
    got = json.loads(json.dumps(trace.run_case(case)))
    if row["group"] == "service" and want["calls"] is not None and got["calls"] is not None:  # name the call that differs
        assert dict(zip(trace.CALLS, got["calls"])) == dict(zip(trace.CALLS, want["calls"]))
    if row["group"] == "options":
        for key in trace.KEYS:
            assert got[key] == want[key], key
    assert got == want
