"""The launch ladders end where they did: every case of tests/golden/make_dispatch_trace.py (context, options, entry point) against the
table that script wrote at the commit before launch_fused and launch_hess were split into one launcher per kernel family
(tests/golden/dispatch_trace.json).  What the forced-option tests of the suite do not pin together is the fall-through: the rung that takes
a launch once the rungs before it have declined (jit = 0, a shape outside a family, a launch size on the other side of an auto rule), and
the exact text a forced option that cannot be served is refused with.  Equality throughout: returned code, error text, last_kernel,
last_n_stream, last_eval_coop, last_v4_ticket, last_hess_kernel, last_hess_split, last_hess_pair, last_hess_rpre."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_dispatch_trace", os.path.join(GOLDEN, "make_dispatch_trace.py"))
trace = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(trace)
with open(os.path.join(GOLDEN, "dispatch_trace.json")) as f:
    TABLE = json.load(f)


def test_table_is_of_these_cases():
    assert [{k: v for k, v in row.items() if k != "expect"} for row in TABLE["cases"]] == trace.CASES


@pytest.mark.gpu
@pytest.mark.parametrize("row", TABLE["cases"], ids=[row["id"] for row in TABLE["cases"]])
def test_dispatch_trace(row):
    got = trace.run_case({k: v for k, v in row.items() if k != "expect"})
    got.pop("n_cu")  # (recorded for information only)
    assert got == row["expect"]
