"""What tests/test_large_exp_reduce_gpu.py relies on, checked without a GPU (the cases are those of tests/large_exp_reduce_cases.py).

The plan: the restatement of large_exp_plan with its payload-only case (pcl_host_launch_pade.hpp) reproduces the committed table -- U, sx, nc, ngrp,
mg, npc and LDS bytes -- for every case and every split the GPU tests force; both launches stay within the 163,840 B a workgroup can have and within
NBW columns per buffer; the payload-only launch keeps the slices of the launch with values, has chain units alone and never counts more tile passes
x rounds than the launch with values.

The reference's floor: the payload formed from the float64 emulation of the kernel's recurrence (le.emulate) stays within 1e-13 -- the bound of
tests/test_large_reduce_cpu.py -- of the payload formed in longdouble from the scipy truth, per entry on the Cauchy-Schwarz scale, with lam = delta
and with the explicit multipliers, and entries of scale zero are exact: the 1e-11 of the GPU tests hides nothing of the reference.

Sensitivity: each of six faults moves an entry by 1e-7 of its scale or more: the last state column dropped, the last drive group dropped, a member's
weight ignored, the factor 1/2 dropped, lam of the wrong interval, the last substep dropped.

The compact layout: compact_of_full / expand_compact round trip at X1 and L7.  The keyword: large_exp_reduce=True raises ValueError before any device
call without large_exp=True and on a variational constructor."""
import numpy as np
import pytest

import large_exp_cases as le
import large_exp_reduce_cases as xc
import piccolo_jl_amd as pa

FLOOR = 1e-13
SEEN = 1e-7
K = xc.K


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------------------
def test_plan_table():
    rows = 0
    for name in xc.NAMES:
        kind, n, cols, m = xc.CASES[name]
        for cps, sl, dr in xc.splits(name):
            full = xc.plan(n, cols, m, False, cols_per_slice=cps, slices=sl, drives=dr)
            pay = xc.plan(n, cols, m, True, cols_per_slice=cps, slices=sl, drives=dr)
            assert (xc.row(full), xc.row(pay)) == xc.TABLE[(name, cps, sl, dr)], (name, cps, sl, dr, xc.row(full), xc.row(pay))
            rows += 1
            for p in (full, pay):  # the LDS bound, and what a buffer holds
                assert p["bytes"] <= le.LDS_BYTES and p["W"] <= p["NBW"] and p["W"] == p["nc"] * (1 + p["mg"]) + p["npc"], (name, cps, sl, dr)
                assert p["sx"] * p["nc"] >= cols > (p["sx"] - 1) * p["nc"] and p["ngrp"] * p["mg"] >= m > (p["ngrp"] - 1) * p["mg"], (name, cps, sl, dr)
                assert dr == 0 or p["mg"] <= dr
            # the payload-only launch: the slices of the Jacobian plan, chain units alone, no more tile passes x rounds
            assert (pay["sx"], pay["nc"]) == (full["sx"], full["nc"]) and pay["U"] == pay["sx"] * pay["ngrp"] and pay["npc"] == 0, (name, cps, sl, dr)
            assert pay["bytes"] == (pay["LD"] * n + le.SLACK + m + 8 + 3 * pay["LD"] * pay["nc"] * (1 + pay["mg"])) * 8
            assert xc.passes(pay) <= xc.passes(full) and pay["U"] <= full["U"], (name, cps, sl, dr)
    assert rows == len(xc.TABLE)
    # the launch with values is the plan as it was
    for name in le.NAMES:
        if name in xc.NAMES:
            assert xc.TABLE[(name, 0, 0, 0)][0] == le.TABLE[name], name
    # what the cases are for
    assert xc.TABLE[("L4", 0, 0, 0)][0][3:5] == (8, 3) and xc.TABLE[("L4", 0, 0, 0)][1][3:5] == (2, 12)  # eight groups of three; two of twelve
    assert xc.TABLE[("L6", 0, 0, 0)][1][:3] == (3, 3, 11)  # three slices
    x1 = xc.plan(128, 3, 2), xc.plan(128, 3, 2, True)
    assert x1[0]["NBW"] == 9 == 3 * (1 + 2) and (x1[0]["ngrp"], x1[0]["mg"]) == (2, 1) and (x1[1]["ngrp"], x1[1]["mg"], x1[1]["U"]) == (1, 2, 1)
    assert xc.plan(120, 1, 24, True, drives=2)["ngrp"] == 12 and xc.plan(96, 1, 4, True, items=99)["U"] == 1
    assert 128 * 128 // 2 == 8192  # ... and X1's tile is the expansion's largest


# ---- the reference's floor --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", xc.NAMES)
def test_emulated_payload_floor(name):
    d, j = xc.truth(name)
    ed, ej = xc.emulated(name)
    for lams in (None, [xc.lam(name)]):
        ref, scale = xc.payload(name, [d], [j], lams)
        got, _ = xc.payload(name, [ed], [ej], lams)
        w = xc.worst(got.astype(np.float64), ref, scale)
        print("%s, lam %s: %.1e of the scale" % (name, "= delta" if lams is None else "explicit", w))
        assert w <= FLOOR, (name, w)
    if name == "L1z":  # the zero step: exact zeros on the drive entries of interval 1
        kind, n, cols, m = xc.CASES[name]
        ref, scale = xc.payload(name, [d], [j], [xc.lam(name)])
        assert not scale[1 + m : 1 + 2 * m].any() and not ref[1 + m : 1 + 2 * m].any() and scale[1 + K * m + 1] > 0


# ---- sensitivity ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", xc.NAMES)
def test_payload_faults_are_seen(name):
    kind, n, cols, m = xc.CASES[name]
    members = [xc.truth(name, drift=b) for b in range(2)]  # two members with weights (0.25, 0.75): the second drift on the same knots
    deltas, vals, w = [t[0] for t in members], [t[1] for t in members], [0.25, 0.75]
    lams = [xc.lam(name, b) for b in range(2)]
    mg = xc.plan(n, cols, m)["mg"]
    good_l, good_d = xc.payload(name, deltas, vals, lams, w), xc.payload(name, deltas, vals, None, w)
    lay, G0, Gj, Z = xc.case(name)
    short = le.emulate(lay, G0, Gj, Z, drop_substep=True)
    one_l = xc.payload(name, [xc.emulated(name)[0]], [xc.emulated(name)[1]], [lams[0]])
    faults = {
        "last state column dropped": (good_l, xc.payload(name, deltas, vals, lams, w, drop_col=True)[0]),
        "last drive group dropped": (good_l, xc.payload(name, deltas, vals, lams, w, drop_group=mg)[0]),
        "member weights ignored": (good_l, xc.payload(name, deltas, vals, lams, w, ignore_weights=True)[0]),
        "factor 1/2 dropped": (good_d, xc.payload(name, deltas, vals, None, w, no_half=True)[0]),
        "lam of the wrong interval": (good_l, xc.payload(name, deltas, vals, lams, w, shift_lam=True)[0]),
        "last substep dropped": (one_l, xc.payload(name, [short[0]], [short[1]], [lams[0]])[0]),
    }
    for what, ((good, scale), bad) in faults.items():
        if what == "last state column dropped" and cols == 1:
            continue  # (one column: dropping it leaves nothing -- the multi-column cases carry this fault)
        moved = float((np.abs(bad - good)[scale > 0] / scale[scale > 0]).max())
        print("%s: %s moves an entry by %.1e of its scale" % (name, what, moved))
        assert moved >= SEEN, (name, what, moved)


# ---- the compact layout -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["X1", "L7"])
def test_compact_round_trip(name):
    kind, n, cols, m = xc.CASES[name]
    j = xc.truth(name)[1]
    c = xc.compact_of_full(j, n, cols, m)
    assert c.size == K * xc.compact_per(n, cols, m) == xc.compact_labels(n, cols, m).size and j.size == K * xc.full_per(n, cols, m)
    assert c.size < j.size  # (one column too: the ones are not part of the compact block)
    assert np.array_equal(xc.expand_compact(c, n, cols, m), j)
    assert np.array_equal(xc.compact_of_full(xc.expand_compact(c, n, cols, m), n, cols, m), c)


# ---- the keyword ------------------------------------------------------------------------------------------------------------------------------------
def _mk(d, **over):
    n = 2 * d
    kw = dict(d=d, m=1, N=3, z_dim=n + 3, u_off=n + 2, dt_off=n, x_offs=[0], G0=np.zeros((n, n)), Gj=np.zeros((1, n, n)), batch=1,
              batch_mode=pa._lib.PCL_BATCH_MEMBERS, state_cols=1, pade_order="exp", large_generator=True, large_exp=True, large_exp_reduce=True)  # fmt: skip
    kw.update(over)
    return kw


def test_keyword_value_errors_come_before_any_device_call():
    C = pa.integrators._PclContext
    with pytest.raises(ValueError, match="large_exp=True"):
        C(**_mk(33, large_exp=False))
    with pytest.raises(ValueError, match="large_exp=True"):
        C(**_mk(33, large_exp=False, pade_order=8))
    with pytest.raises(ValueError, match="large_generator=True"):
        C(**_mk(33, large_generator=False))
    for mode in (pa._lib.PCL_BATCH_VARIATIONAL, pa._lib.PCL_BATCH_VARIATIONAL_EXP):
        with pytest.raises(ValueError, match="variational"):
            C(**_mk(33, batch_mode=mode))
    with pytest.raises(ValueError, match="variational"):
        pa.integrators.HipVariationalIntegrator(None, None, "x", ["v"], "u", None, ket=True, large_exp_reduce=True)
    with pytest.raises(ValueError, match="large_exp=True"):
        pa.HipPadeIntegrator(np.zeros((4, 4)), np.zeros((1, 4, 4)), None, large_exp_reduce=True)
    pa.integrators._check_services(pa._lib.PCL_BATCH_VARIATIONAL, large_exp_reduce=False, large_exp=False)  # off: nothing to check
    pa.integrators._check_services(pa._lib.PCL_BATCH_MEMBERS, "exp", large_exp_reduce=True, large_exp=True, large_generator=True)  # (large_exp=True: with what it stands beside)
