"""The cases of tests/large_plan_cases.py (the launch plans of the large-generator Pade kernels, PCL_LARGE_N) before any GPU is involved: that every
number of the case table and of the long launches is what the restated plans (lc.large_plan, hc.hess_plan) give -- at 256 CUs, and at 304 and 128
wherever the rule reads n_cu -- that the forced splits of the GPU tests are what they claim and fit, that the float64 oracle is within 1e-13 of the
longdouble truth per segment, and that the truth sees the fault each case exists for at 1e-7 of a segment's size (1e4 x the GPU tolerance)."""
import numpy as np
import pytest

import large_plan_cases as pc
import large_shape_cases as lc
import vector_shape_cases as vc
from oracle import pade_oracle as po
from shape_cases import check_segments, hess_labels, jac_labels

FLOOR = 1e-13
CUS = (256, 304, 128)


def row(p):
    return (p["U"], p["sx"], p["ngrp"], p["mg"], p["npc"], p["bytes"])


def worst(errs):
    s = max(errs, key=errs.get)
    return errs[s], s


# ---- the case table ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.NAMES)
def test_jacobian_plan_of_the_table(name):
    kind, n, cols, m = pc.CASES[name]
    assert kind == "vec" or n % 2 == 0
    for n_cu in CUS:  # three items: n_cu / 3 never binds, so every CU count gives the table's row
        p = pc.jac_plan(name, n_cu=n_cu)
        assert row(p) == pc.TABLE[name], (name, n_cu, row(p))
        assert p["nce"] == pc.SPLIT[name][0] and p["npce"][-3:] == pc.SPLIT[name][1], (name, p["nce"], p["npce"])
        assert p["bytes"] <= pc.LDS_BYTES and p["chain_blocks"] + p["npc"] <= p["NB"], name
        assert sum(p["nce"]) == cols and sum(p["npce"]) == n and p["U"] == max(p["sx"] * p["ngrp"], -(-n // p["npc"])), name
        assert 1 <= p["pairs"] <= 2 and p["threads"] == 64 * p["row_tiles"] <= 512, name
        assert p["ngrp"] * p["mg"] >= m > (p["ngrp"] - 1) * p["mg"] if m else (p["ngrp"], p["mg"]) == (1, 0)
        e = lc.large_plan(n, cols, m, jac=False, n_cu=n_cu)
        assert ((e["U"], e["nc"], e["bytes"]), e["nce"]) == pc.EVAL_TABLE[name] and e["bytes"] <= pc.LDS_BYTES, (name, e)


def test_what_each_case_sits_on():
    P = {name: pc.jac_plan(name) for name in pc.NAMES}
    H = {name: pc.hess_plan(name) for name in pc.NAMES}
    # P1: 12 slices of 5 columns x 4 groups of one drive = 48 chain units; 120 / 3 = 40 panel units: eight units own no power column
    assert (P["P1"]["sx"], P["P1"]["nc"], P["P1"]["ngrp"]) == (12, 5, 4) and P["P1"]["npce"] == [3] * 40 + [0] * 8
    for name in lc.NAMES:  # ... which no case of large_shape_cases has: there the panel units outnumber the chain units
        q = lc.large_plan(*lc.CASES[name][1:])
        assert min(q["npce"]) > 0 and q["sx"] * q["ngrp"] < -(-lc.CASES[name][1] // q["npc"]), name
    # P2: x_dim 8192, 21 slices of 3 and one of 1; two panel columns in unit 42, none in unit 43
    assert pc.layout("P2").x_dim == 8192 and P["P2"]["nce"] == [3] * 21 + [1] and P["P2"]["npce"] == [3] * 42 + [2, 0]
    assert H["P2"]["nce"] == [2] * 32 and H["P1"]["nce"] == [3] * 20
    assert P["P3"]["npce"] == [6] * 16 and P["P3"]["U"] == P["P3"]["sx"] * P["P3"]["ngrp"] == 16  # chain units = panel units
    # seven waves: 448 threads (n = 97 .. 112), which none of L1 .. L9 has
    for name in ("P4", "P5", "P7"):
        assert P[name]["threads"] == 448 and P[name]["row_tiles"] == 7
    assert sorted({lc.large_plan(*lc.CASES[nm][1:])["threads"] for nm in lc.NAMES}) == [320, 384, 512]
    assert 100 % 16 == 4 and P["P4"]["npce"] == [15] * 6 + [10] and P["P5"]["npce"] == [15] * 6 + [14]
    # P5: no drive -- no group, two blocks per column in the chain (W | V), six chain blocks
    assert P["P5"]["mg"] == 0 and P["P5"]["chain_blocks"] == 6 and H["P5"]["mg"] == 0 and H["P5"]["mge"] == [0]
    # the Hessian's uneven groups and slices, chosen by the plan itself
    assert H["P6"]["mge"] == [3, 3, 1] and H["P8"]["mge"] == [6, 5] and H["P7"]["nce"] == [4, 4, 4, 1] and H["P7"]["mge"] == [1] * 5
    assert P["P7"]["nce"] == [7, 6] and P["P7"]["npce"] == [11] * 10 + [2] and P["P7"]["U"] == 2 * 5 + 1
    # P9: odd n, LD = n
    assert P["P9"]["LD"] == 67 and P["P9"]["npce"] == [14] * 4 + [11]


@pytest.mark.parametrize("name", pc.NAMES)
def test_hessian_plan_of_the_table(name):
    kind, n, cols, m = pc.CASES[name]
    h = pc.hess_plan(name)
    assert ((h["U"], h["sx"], h["nc"], h["ngrp"], h["mg"], h["bytes"]), h["nce"], h["mge"]) == pc.HESS_TABLE[name], (name, h)
    assert h["bytes"] <= pc.LDS_BYTES and sum(h["nce"]) == cols and sum(h["mge"]) == m and h["U"] == h["sx"] * h["ngrp"], name
    assert h["threads"] == 64 * ((n + 15) // 16)


# ---- long launches ------------------------------------------------------------------------------------------------------------------------------------
def test_long_launch_plans():
    for (name, items, n_cu), (U, npc, npce, pairs, nbytes) in pc.LONG.items():
        p = pc.jac_plan(name, items=items, n_cu=n_cu)
        assert (p["U"], p["npc"], p["npce"], p["pairs"], p["bytes"]) == (U, npc, npce, pairs, nbytes), (name, items, n_cu, p)
        assert p["bytes"] <= pc.LDS_BYTES and pairs <= lc.NP_PAIRS and sum(npce) == pc.shape(name)[1]
    for name in pc.LONG_NAMES:
        for items in pc.SEEDS:
            assert (name, items, 256) in pc.LONG
    assert 256 // 87 == 2 and 256 // 86 == 2 and 256 // 85 == 3 and 256 // 300 == 0 and 304 // 87 == 3 and 128 // 87 == 1
    # n = 96, one ket: U 2, npc 48, six pairs per thread; no case of the N = 4 tests runs more than two
    assert pc.LONG[("L2", 87, 256)][:2] == (2, 48) and pc.LONG[("L2", 87, 256)][3] == 6
    assert max(pc.jac_plan(name)["pairs"] for name in pc.NAMES) == 2 and max(lc.large_plan(*lc.CASES[nm][1:])["pairs"] for nm in lc.NAMES) == 2
    # n = 67 at 300 items: one unit holds the whole panel, 67 x 67 values = 2245 pairs on 320 threads: eight per thread, exactly PL_NP
    p = pc.jac_plan("P9", items=300)
    assert (p["U"], p["npc"], p["pairs"]) == (1, 67, 8) and lc.NP_PAIRS == 8 and (67 * 67 + 1) // 2 == 2245 <= 8 * 320 < 2245 + 320
    # where one panel does not fit beside the chain, the `fits` loop raises U again
    for name in ("L2", "P4", "P6", "P8"):
        q = pc.jac_plan(name, items=300)
        assert q["U"] == pc.LONG[(name, 300, 256)][0] >= 2
        one = pc.shape(name)[1]
        assert q["chain_blocks"] + one > q["NB"] or (one * one + 1) // 2 > lc.NP_PAIRS * q["threads"], name
    # P1: the plan does not move with the item count: 87 x 48 = 4,176 workgroups
    for items in (3, 87, 300):
        for n_cu in CUS:
            assert row(pc.jac_plan("P1", items=items, n_cu=n_cu)) == pc.TABLE["P1"]
    assert 87 * pc.TABLE["P1"][0] == 4176
    # the Hessian plan does not read the item count at all
    assert pc.hess_plan("P6")["U"] == 3


# ---- the forced splits of the GPU tests ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.NAMES + ["L2"])
def test_forced_splits_are_what_they_claim(name):
    kind, n, cols, m = pc.shape(name)
    jac, hess = pc.forced_splits(name)
    base = pc.jac_plan(name)
    seen_uneven = False
    for kw in jac:
        for items in (3, 87, 300):
            p = lc.large_plan(n, cols, m, items=items, cols_per_slice=kw.get("cols_per_slice", 0), slices=kw.get("general_slices", 0))
            assert p["bytes"] <= pc.LDS_BYTES and p["pairs"] <= lc.NP_PAIRS and sum(p["nce"]) == cols and sum(p["npce"]) == n, (name, kw, items)
        p = lc.large_plan(n, cols, m, cols_per_slice=kw.get("cols_per_slice", 0), slices=kw.get("general_slices", 0))
        if kw.get("general_slices") == n:
            assert p["npc"] == 1 and p["U"] == n
        elif "general_slices" in kw:
            assert kw["general_slices"] == base["U"] + 1 and p["U"] >= base["U"]
        else:
            e = lc.large_plan(n, cols, m, jac=False, cols_per_slice=kw["cols_per_slice"])
            assert max(p["nce"]) <= kw["cols_per_slice"] and max(e["nce"]) <= kw["cols_per_slice"] and e["bytes"] <= pc.LDS_BYTES
            seen_uneven |= p["nce"][-1] < p["nce"][0] or e["nce"][-1] < e["nce"][0]  # (in the Jacobian launch, or at least in the residual-only one)
    assert seen_uneven or cols == 1, name
    for items in pc.SEEDS:  # a long launch: one above ITS default U, which still fits
        above = [kw["general_slices"] for kw in pc.forced_splits(name, 256, items)[0] if kw.get("general_slices", n) != n]
        p = lc.large_plan(n, cols, m, items=items, slices=above[0])
        assert above == [pc.jac_plan(name, items=items)["U"] + 1] and p["U"] >= above[0] - 1 and p["bytes"] <= pc.LDS_BYTES and p["pairs"] <= lc.NP_PAIRS, (name, items)
    groups = []
    for kw in hess:
        h = pc.hess_plan(name, cols_per_slice=kw.get("cols_per_slice", 0), drives=kw.get("large_hess_drives", 0))
        assert h["bytes"] <= pc.LDS_BYTES and sum(h["nce"]) == cols and sum(h["mge"]) == m, (name, kw)
        if "large_hess_drives" in kw:
            assert max(h["mge"]) <= kw["large_hess_drives"]
            groups.append(h["mge"])
    if m > 1:
        assert [1] * m in groups, (name, groups)  # one drive per group
        forced = [kw["large_hess_drives"] for kw in hess if "large_hess_drives" in kw]
        assert m == 2 or any(m % g for g in forced), (name, forced)  # a cap that does not divide m
        # an uneven last group wherever any cap gives one: the plan evens the groups, so m = 2, 4, 6 never end in a narrower group, and beside P7's
        # four columns of n = 112 only one drive fits whatever the cap
        possible = any(pc.ragged_groups(pc.hess_plan(name, drives=g)) for g in range(1, m))
        assert any(g[-1] < g[0] for g in groups) == possible and possible == (m not in (2, 4, 6) and name != "P7"), (name, groups)


# ---- steps, the reference floor ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.NAMES)
def test_steps(name):
    lay, G0, Gj, Z, long_step = pc.case(name)
    th = [Z[k, lay.dt_off] * np.linalg.norm(vc.g_of(lay, Z, k, G0, Gj), 2) for k in range(lay.K)]
    assert np.allclose(th, [0.15, -0.3, long_step], rtol=1e-12)
    w = vc.top_term_weight(lay, G0, Gj, Z)
    assert w >= pc.SEEN
    print("%s: long step %.2f, c_5 moves the residual by %.1e" % (name, long_step, w))


@pytest.mark.parametrize("name", pc.NAMES[3:] + ["P3"])
def test_oracle_floor(name):
    """Every non-unitary case at its orders, and one unitary case (P3), Hessian included."""
    lay, G0, Gj, Z, _ = pc.case(name)
    mu = pc.rand_mu(name).reshape(lay.K, -1)
    for order in pc.ORDERS[name]:
        d, j = pc.truth(name, order)
        er = check_segments(po.pade_residual(Z, lay, G0, Gj, order), d, lc.residual_labels(lay), FLOOR)
        ej = check_segments(po.pade_jacobian_values(Z, lay, G0, Gj, order), j, jac_labels(lay), FLOOR)
        eh = check_segments(po.pade_hessian_values(Z, mu, lay, G0, Gj, order), pc.hess_truth(name, order), hess_labels(lay), FLOOR)
        print("%s order %d: residual %.1e (%s)  Jacobian %.1e (%s)  Hessian %.1e (%s)" % ((name, order) + worst(er) + worst(ej) + worst(eh)))


def test_the_sorted_check_is_check_segments():
    """pc.check (the labels sorted once per case) gives check_segments' numbers, accepts what it accepts and refuses what it refuses."""
    import large_reduce_cases as rc

    name, order = "P8", 6
    lay, G0, Gj, Z, _ = pc.case(name)
    d, j = pc.truth(name, order)
    h = pc.hess_truth(name, order)
    got = {"delta": po.pade_residual(Z, lay, G0, Gj, order).reshape(-1), "jac": po.pade_jacobian_values(Z, lay, G0, Gj, order).reshape(-1),
           "hess": po.pade_hessian_values(Z, pc.rand_mu(name).reshape(lay.K, -1), lay, G0, Gj, order).reshape(-1)}  # fmt: skip
    got["compact"] = pc.compact_of(got["jac"], name)
    ref = {"delta": d, "jac": j, "hess": h, "compact": pc.compact_of(j, name)}
    labels = {"delta": lc.residual_labels(lay), "jac": jac_labels(lay), "hess": hess_labels(lay), "compact": pc.compact_labels(name)}
    for which in ref:
        assert pc.check(got[which], ref[which], name, which, FLOOR) == check_segments(got[which], ref[which], labels[which], FLOOR), which
        bad = got[which].copy()
        bad[np.abs(bad).argmax()] *= 1 + 1e-9
        for fn in (lambda: pc.check(bad, ref[which], name, which, 1e-11), lambda: check_segments(bad, ref[which], labels[which], 1e-11)):
            with pytest.raises(AssertionError):
                fn()
    pay = pc.payload_truth(name, order, True)
    assert pc.check(pay, pay, name, "payload") == check_segments(pay, pay, rc.payload_labels(11), 1e-11)
    # a zero segment is held to exact zeros: (h, h) at order 2
    h2 = pc.hess_truth(name, 2)
    assert h2[pc.hess_labels(lay) == "hh@0"].max() == 0
    bad = h2.copy()
    bad[np.flatnonzero(pc.hess_labels(lay) == "hh@0")[0]] = 1e-300
    with pytest.raises(AssertionError):
        pc.check(bad, h2, name, "hess")


# ---- the truth sees the faults the cases exist for ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.MUTANT_NAMES)
def test_the_truth_sees_the_fault(name):
    lay = pc.layout(name)
    d, j = pc.truth_ld(name, pc.MUTANT_ORDER)
    muts = pc.mutants(name)
    assert muts
    for what, (bd, bj, bh) in muts.items():
        sd, sj = pc.moved(d, bd, lc.residual_labels(lay)), pc.moved(j, bj, jac_labels(lay))
        sh = pc.moved(pc.hess_truth_ld(name, pc.MUTANT_ORDER), bh, hess_labels(lay)) if bh is not None else 0.0
        print("%s, %s: residual moved by %.1e, Jacobian by %.1e, Hessian by %.1e" % (name, what, sd, sj, sh))
        assert max(sd, sj) >= pc.SEEN, (name, what, sd, sj)
        if bh is not None:
            assert sh >= pc.SEEN, (name, what, sh)
    if name in ("L2", "P9"):  # the slots exist: the 87-item plan gives a thread more than two pairs (and P9's 300-item plan all eight)
        assert pc.LONG[(name, 87, 256)][3] > 2 and (name != "P9" or pc.LONG[("P9", 300, 256)][3] == 8)


def test_a_drive_less_system_has_no_drive_column():
    """P5 (m = 0): the structure the GPU test holds pcl_jac_nnz / pcl_hess_nnz against."""
    lay = pc.layout("P5")
    n = 104
    assert lay.m == 0 and po.jac_nnz_per_interval(lay) == 2 * n * n + n and po.hess_nnz_per_interval(lay) == 1 + 2 * n
    assert not any(s.startswith("du") for s in jac_labels(lay)) and not any(s.startswith(("uu", "hu", "u0")) for s in hess_labels(lay))
    rows, cols = po.jac_structure(lay)
    assert rows.size == lay.K * (2 * n * n + n) and cols.max() < lay.N * lay.z_dim and lay.z_dim == n + 2
    hr, hc_ = po.hess_structure(lay)
    assert hr.size == lay.K * (1 + 2 * n)
    d, j = pc.truth("P5", 10)
    assert d.size == lay.K * n and j.size == rows.size and pc.hess_truth("P5", 10).size == hr.size
