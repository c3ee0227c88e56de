"""What tests/test_large_reduce_gpu.py relies on, checked without a GPU (the cases are those of tests/large_reduce_cases.py).

The plan: a restatement of large_plan with its payload-only case (pcl_host_launch_pade.hpp) reproduces the committed table -- U, sx, ngrp, mg, npc and
LDS bytes -- for every case and every split the GPU tests force, stays within the 163,840 B a workgroup can have, and the payload-only launch is the
chain units of the launch with values and nothing else.

The reference's floor: the payload formed from the float64 oracle (po.pade_residual, po.pade_jacobian_values) stays within 1e-13 per segment
(phi, g_u, g_dt; relative to the segment's largest magnitude) of the payload formed from the longdouble truth, with lam = delta and with the explicit
multipliers -- so the 1e-11 of the GPU tests hides nothing of the reference.

Sensitivity: each of five faults moves a payload segment by 1e-7 of its size or more: the last state column dropped, the last drive group dropped, a
member's weight ignored, the factor 1/2 dropped, lam of the wrong interval.

The keyword: large_reduce=True raises ValueError before any device call without large_generator, with pade_order="exp", on a variational constructor."""
import numpy as np
import pytest

import large_reduce_cases as rc
import large_shape_cases as lc
import piccolo_jl_amd as pa
from oracle import pade_oracle as po

FLOOR = 1e-13
SEEN = 1e-7
K = rc.N - 1


def seen(good, bad, labels):
    out = 0.0
    for s in np.unique(labels):
        sel = labels == s
        scale = np.abs(good[sel]).max()
        if scale > 0:
            out = max(out, float(np.abs(bad[sel] - good[sel]).max() / scale))
    return out


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------------------
def test_plan_table():
    rows = 0
    for name in rc.NAMES:
        kind, n, cols, m = rc.CASES[name]
        for cps, sl in rc.splits(name):
            full = rc.reduce_plan(n, cols, m, False, cols_per_slice=cps, slices=sl)
            pay = rc.reduce_plan(n, cols, m, True, cols_per_slice=cps, slices=sl)
            assert (rc.row(full), rc.row(pay)) == rc.TABLE[(name, cps, sl)], (name, cps, sl, rc.row(full), rc.row(pay))
            rows += 1
            for p in (full, pay):
                assert p["bytes"] <= lc.LDS_BYTES and p["chain_blocks"] + p["npc"] <= p["NB"], (name, cps, sl)
                assert sum(p["nce"]) == cols and p["ngrp"] * p["mg"] >= m > (p["ngrp"] - 1) * p["mg"], (name, cps, sl)
            # the payload-only launch: the same chain units, no panel, no P' block
            assert pay["U"] == full["sx"] * full["ngrp"] <= full["U"] and pay["npc"] == 0, (name, cps, sl)
            assert (pay["sx"], pay["nc"], pay["ngrp"], pay["mg"]) == (full["sx"], full["nc"], full["ngrp"], full["mg"])
            assert full["bytes"] - pay["bytes"] == 8 * full["LD"] * full["npc"]
    assert rows == len(rc.TABLE)
    # what the cases are for
    assert rc.TABLE[("L1", 0, 0)][0] == lc.TABLE["L1"] and rc.TABLE[("L6", 0, 0)][0] == lc.TABLE["L6"]  # the launch with values: the plan as it was
    assert rc.TABLE[("L4", 0, 0)][1][2] == 2 and rc.TABLE[("L6", 0, 0)][1][1] == 2  # two drive groups; two slices
    assert rc.reduce_plan(72, 5, 4, True, cols_per_slice=2)["nce"] == [2, 2, 1]
    r1 = rc.reduce_plan(128, 3, 2)
    assert r1["NB"] == 29 < 3 * (2 + 2 * (2 + 2)) and r1["ngrp"] == 2 and r1["mg"] == 1 and r1["chain_blocks"] == 24  # R1: the drives are split
    assert 128 * 128 // 2 == 8192  # ... and its tile is the expansion's largest


# ---- the reference's floor --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.NAMES)
def test_oracle_payload_floor(name):
    kind, n, cols, m = rc.CASES[name]
    lay, G0, Gj, Z, _ = rc.case(name)
    labels = rc.payload_labels(m)
    for order in rc.ORDERS_PAYLOAD:
        d, j = rc.truth_ld(name, order)
        od, oj = po.pade_residual(Z, lay, G0, Gj, order), po.pade_jacobian_values(Z, lay, G0, Gj, order)
        for lams in (None, [rc.lam(name)]):
            ref = rc.payload_ld(name, [d], [j], lams)
            got = rc.payload_ld(name, [od], [oj], lams)
            errs = rc.check_segments(got.astype(np.float64), ref.astype(np.float64), labels, FLOOR)
            print("%s order %d, lam %s: %s" % (name, order, "= delta" if lams is None else "explicit", {k: "%.1e" % v for k, v in errs.items()}))


# ---- sensitivity ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.NAMES)
def test_payload_faults_are_seen(name):
    kind, n, cols, m = rc.CASES[name]
    labels = rc.payload_labels(m)
    order = 4
    # two members with weights (0.25, 0.75): the second drift of the same system on the same knots
    members = [rc.truth_ld(name, order, drift=b) for b in range(2)]
    deltas, vals, w = [t[0] for t in members], [t[1] for t in members], [0.25, 0.75]
    lams = [rc.lam(name, b) for b in range(2)]
    mg = rc.reduce_plan(n, cols, m)["mg"]
    good_l, good_d = rc.payload_ld(name, deltas, vals, lams, w), rc.payload_ld(name, deltas, vals, None, w)
    faults = {
        "last state column dropped": (good_l, rc.payload_ld(name, deltas, vals, lams, w, drop_col=True)),
        "last drive group dropped": (good_l, rc.payload_ld(name, deltas, vals, lams, w, drop_group=mg)),
        "member weights ignored": (good_l, rc.payload_ld(name, deltas, vals, lams, w, ignore_weights=True)),
        "factor 1/2 dropped": (good_d, rc.payload_ld(name, deltas, vals, None, w, no_half=True)),
        "lam of the wrong interval": (good_l, rc.payload_ld(name, deltas, vals, lams, w, shift_lam=True)),
    }
    for what, (good, bad) in faults.items():
        if what == "last state column dropped" and cols == 1:
            continue  # (one column: dropping it leaves nothing -- the multi-column cases carry this fault)
        moved = seen(good.astype(np.float64), bad.astype(np.float64), labels)
        print("%s: %s moves a segment by %.1e" % (name, what, moved))
        assert moved >= SEEN, (name, what, moved)


def test_compact_truth_takes_each_tile_once():
    for name in ("L1", "L6", "R1"):
        kind, n, cols, m = rc.CASES[name]
        j = rc.truth(name, 2)[1]
        c = rc.compact_of(j, n, cols, m)
        assert c.size == K * rc.compact_per(n, cols, m) and rc.compact_labels(n, cols, m).size == c.size
        if cols == 1:
            assert np.array_equal(c, j)
        else:  # expanding it again gives the full values: every copy of a tile is the same numbers
            v = c.reshape(K, -1)
            nn = n * n
            back = np.concatenate([np.tile(v[:, :nn], cols), np.tile(v[:, nn : 2 * nn], cols), v[:, 2 * nn :]], axis=1).reshape(-1)
            assert np.array_equal(back, j)


# ---- the keyword ------------------------------------------------------------------------------------------------------------------------------------
def _mk(d, **over):
    n = 2 * d
    kw = dict(d=d, m=1, N=3, z_dim=n + 3, u_off=n + 2, dt_off=n, x_offs=[0], G0=np.zeros((n, n)), Gj=np.zeros((1, n, n)), batch=1,
              batch_mode=pa._lib.PCL_BATCH_MEMBERS, state_cols=1, pade_order=4, large_generator=True, large_reduce=True)  # fmt: skip
    kw.update(over)
    return kw


def test_keyword_value_errors_come_before_any_device_call():
    C = pa.integrators._PclContext
    with pytest.raises(ValueError, match="large_generator=True"):
        C(**_mk(33, large_generator=False))
    with pytest.raises(ValueError, match="exp"):
        C(**_mk(33, pade_order="exp"))
    for mode in (pa._lib.PCL_BATCH_VARIATIONAL, pa._lib.PCL_BATCH_VARIATIONAL_EXP):
        with pytest.raises(ValueError, match="variational"):
            C(**_mk(33, batch_mode=mode))
    with pytest.raises(ValueError, match="variational"):
        pa.integrators.HipVariationalIntegrator(None, None, "x", ["v"], "u", None, ket=True, large_reduce=True)
    with pytest.raises(ValueError, match="large_generator=True"):
        pa.HipPadeIntegrator(np.zeros((4, 4)), np.zeros((1, 4, 4)), None, large_reduce=True)
    pa.integrators._check_services(pa._lib.PCL_BATCH_VARIATIONAL, "exp", large_reduce=False, large_generator=False)  # off: nothing to check
    pa.integrators._check_services(pade_order=8, large_reduce=True, large_generator=True)
