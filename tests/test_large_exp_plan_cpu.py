"""The cases of tests/large_exp_plan_cases.py (the launch plans of the large exponential kernels, PCL_LARGE_N | PCL_LARGE_EXP) before any GPU is involved:
that every number of the committed tables is what the restated plans (le.plan, xc.plan, lh.plan) give at 3, 87 and 300 items on 256, 304 and 128 CUs;
that every regime the cases exist for is entered, each named by a predicate on the plan; that the forced splits of the GPU tests are what they claim
and fit; that the float64 emulations are within 1e-12 of the truths per segment (a tenth of the GPU tolerance -- the values read are in DESIGN.md
4.21.1); and that every mutant of le.emulate / lh.emulate_hess, both `mm` faults and the three mutants of the new regimes move a segment by 1e-7 on
every case they apply to."""
import numpy as np
import pytest

import large_exp_cases as le
import large_exp_hess_cases as lh
import large_exp_plan_cases as qc
import large_exp_reduce_cases as xc
from shape_cases import check_segments

K = qc.K


def worst(errs):
    s = max(errs, key=errs.get)
    return "%.1e (%s)" % (errs[s], s)


def payload_moved(good, bad, scale):
    sel = scale > 0
    return float((np.abs(bad - good)[sel] / scale[sel]).max())


# ---- the tables -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", qc.NAMES)
def test_every_number_of_the_tables(name):
    kind, n, cols, m = qc.CASES[name]
    assert kind == "vec" or n % 2 == 0
    for items in qc.ITEMS:
        for n_cu in qc.CUS:
            p = qc.jac_plan(name, items, n_cu)
            assert qc.jac_row(p) == qc.table_row(qc.JAC_TABLE, name, items, n_cu), (name, items, n_cu, qc.jac_row(p))
            assert p["bytes"] <= qc.LDS_BYTES and p["W"] == p["nc"] * (1 + p["mg"]) + p["npc"] <= p["NBW"] and p["threads"] == 64 * ((n + 15) // 16)
            assert sum(p["nce"]) == cols and sum(p["mge"]) == m and sum(p["npce"]) == n and min(p["nce"]) >= 1 and (m == 0 or min(p["mge"]) >= 1)
            assert p["U"] == max(p["chain_units"], -(-n // p["npc"])) and len(p["npce"]) == p["U"]
            q = qc.payload_plan(name, items, n_cu)
            assert qc.payload_row(q) == qc.table_row(qc.PAYLOAD_TABLE, name, items, n_cu), (name, items, n_cu, qc.payload_row(q))
            assert q["bytes"] <= qc.LDS_BYTES and q["W"] == q["nc"] * (1 + q["mg"]) <= q["NBW"] and q["npc"] == 0 and q["U"] == q["sx"] * q["ngrp"]
            assert q["nce"] == p["nce"] and sum(q["mge"]) == m  # the slices of the launch with values
        p = qc.jac_plan(name, items, 256)
        assert (p["nce"], p["mge"], p["npce"][-3:]) == qc.table_row(qc.JAC_SPLIT, name, items), (name, items, p["nce"], p["mge"], p["npce"])
    e = qc.eval_plan(name)
    assert (qc.eval_row(e), e["nce"]) == qc.EVAL_TABLE[name] and e["bytes"] <= qc.LDS_BYTES and sum(e["nce"]) == cols and e["mg"] == e["npc"] == 0
    h = qc.hess_plan(name)
    assert (qc.hess_row(h), h["nce"], h["mge"]) == qc.HESS_TABLE[name], (name, qc.hess_row(h), h["nce"], h["mge"])
    assert h["bytes"] <= qc.LDS_BYTES and h["W"] <= h["NBW"] and sum(h["nce"]) == cols and sum(h["mge"]) == m and h["U"] == h["sx"] * h["pairs"]
    assert h["W"] == h["nc"] * lh.unit_columns(h["mg"], h["ngrp"] == 1)


def test_the_table_has_a_row_for_every_launch():
    for name in qc.NAMES:
        for items in qc.ITEMS:
            for n_cu in qc.CUS:
                for table in (qc.JAC_TABLE, qc.PAYLOAD_TABLE):
                    assert len(qc.table_row(table, name, items, n_cu)) in (7, 9)
            assert len(qc.table_row(qc.JAC_SPLIT, name, items)) == 3
    assert set(qc.LONG_NAMES) <= set(qc.NAMES) and not set(qc.LONG_NAMES) & set(qc.UNITARY) and {87: 29, 300: 100} == qc.SEEDS
    assert 256 // 87 == 2 and 304 // 87 == 3 and 128 // 87 == 1 and 256 // 300 == 0


# ---- every regime, by a predicate on the plan -----------------------------------------------------------------------------------------------------------
def old_plans():
    """The plans of every launch the suite made before: L1 .. L9 (L1z is L1) and X1 at three items, with the splits those tests force."""
    out = []
    for name, (kind, n, cols, m) in xc.CASES.items():
        for cps, sl, dr in xc.splits(name) + [(2, 7, 0)]:
            out.append(qc._spell(le.plan(n, cols, m, cols_per_slice=cps, slices=sl, drives=dr), n, cols, m))
        for dr in (1, 2):
            out.append(qc._spell(le.plan(n, cols, m, drives=dr), n, cols, m))
    return out


def old_hess_plans():
    out = []
    for name, (kind, n, cols, m) in lh.CASES.items():
        for cps in (0, 1, 2, 3, 5, 7):
            for dr in (0, 1, 3, 4):
                out.append((name, cps, dr, qc._spell(lh.plan(n, cols, m, cols_per_slice=cps, drives=dr), n, cols, m)))
    return out


def test_every_regime_is_entered():
    J = {name: qc.jac_plan(name) for name in qc.NAMES}
    H = {name: qc.hess_plan(name) for name in qc.NAMES}
    P = {name: qc.payload_plan(name) for name in qc.NAMES}
    old, old_h = old_plans(), old_hess_plans()
    own = [qc._spell(le.plan(n, cols, m), n, cols, m) for kind, n, cols, m in xc.CASES.values()]  # ... those the plan chose itself
    # -- the unitary state, d = 48, 60, 64
    assert [(qc.CASES[nm][1] // 2, qc.CASES[nm][2]) for nm in qc.UNITARY] == [(60, 60), (64, 64), (48, 48)]
    assert max(c[2] for c in xc.CASES.values()) == 33 and xc.CASES["X1"][2] == 3 and min(qc.CASES[nm][2] for nm in qc.UNITARY) == 48  # copies of -E
    q = J["Q1"]
    assert (q["U"], q["sx"], q["ngrp"], q["npc"], q["chain_units"], q["bytes"]) == (60, 9, 4, 2, 36, 163744) and q["nce"] == [7] * 8 + [4]
    assert qc.LDS_BYTES - q["bytes"] == 96 and qc.uneven(q["nce"]) and not any(qc.uneven(p["nce"]) for p in own)
    q = J["Q2"]
    assert qc.layout("Q2").x_dim == 8192 and (q["U"], q["npc"], q["chain_units"], q["W"], q["NBW"]) == (128, 1, 32, 9, 9) and q["nce"] == [4] * 16
    q = J["Q3"]
    assert (q["nc"], q["W"], q["NBW"]) == (16, 37, 37) and qc.tiles(q) == 3 and max(p["nc"] for p in old) == 11
    # -- a Hessian plan with nc > 1 that the plan itself chose, at mg > 1; 60 and 64 slices of one column for the sum kernel to add
    assert (H["Q3"]["sx"], H["Q3"]["nc"], H["Q3"]["mg"]) == (24, 2, 4)
    assert not any(p["nc"] > 1 and p["mg"] > 1 for nm, cps, dr, p in old_h if (cps, dr) == (0, 0))
    assert (H["Q1"]["sx"], H["Q1"]["nc"], H["Q2"]["sx"], H["Q2"]["nc"]) == (60, 1, 64, 1) and max(lh.CASES[nm][2] for nm in lh.NAMES) == 33
    # -- off-diagonal Hessian units between uneven groups, crossed with state-column slices
    for name, groups, sx, pairs, U in (("Q7", [4, 4, 3], 3, 6, 18), ("Q10", [2, 2, 2, 1], 5, 10, 50)):
        h = H[name]
        assert qc.uneven(h["mge"]) and h["ngrp"] > 1 and h["sx"] > 1 and (h["mge"], h["sx"], h["pairs"], h["U"]) == (groups, sx, pairs, U)
    assert not any(qc.uneven(p["mge"]) and p["ngrp"] > 1 and p["sx"] > 1 for nm, cps, dr, p in old_h)
    assert not any(p["ngrp"] > 1 and p["sx"] > 1 for nm, cps, dr, p in old_h if (cps, dr) == (0, 0))
    # -- chain units beyond the panel units: some unit has u npc >= n
    q = J["Q11"]
    assert any(u * q["npc"] >= 128 for u in range(q["U"])) and (q["U"], q["chain_units"], q["npc"]) == (48, 48, 3) and q["npce"][42:] == [2, 0, 0, 0, 0, 0]
    assert all(min(p["npce"]) > 0 for p in old)
    # -- plans that move with the item count
    moves = {name: [qc.jac_row(qc.jac_plan(name, items)) for items in qc.ITEMS] for name in qc.NAMES}
    assert moves["Q4"][0] == moves["Q4"][1] != moves["Q4"][2] and moves["Q6"][0] != moves["Q6"][1] == moves["Q6"][2]
    assert moves["Q7"][0] == moves["Q7"][1] != moves["Q7"][2] and moves["Q8"][0] == moves["Q8"][2] != moves["Q8"][1]
    assert [r[4] for r in moves["Q12"]] == [1, 2, 3] and [r[0] for r in moves["Q8"]] == [6, 2, 6]
    assert [(r[0], r[4], r[5]) for r in moves["Q4"]] == [(8, 2, 13), (8, 2, 13), (4, 5, 25)]
    assert [(r[0], r[4], r[5]) for r in moves["Q6"]] == [(40, 1, 2), (4, 2, 20), (4, 2, 20)]
    assert [(r[0], r[4], r[5], r[6], r[7]) for r in moves["Q7"]][2] == (3, 4, 30, 45, 46)
    for name in qc.UNITARY + ("Q5", "Q10", "Q11"):
        assert len(set(moves[name])) == 1, name
    assert [qc.payload_plan("Q7", items)["mg"] for items in qc.ITEMS] == [4, 4, 4] and P["Q7"]["mge"] == [4, 4, 3] and J["Q7"]["mg"] == 1
    # -- a panel wider than 16 columns: the Horner loop runs two or three column tiles
    wide = {(name, items): qc.jac_plan(name, items) for name in qc.LONG_NAMES for items in qc.SEEDS}
    widths = sorted({p["npc"] for p in wide.values() if p["npc"] > 16})
    assert widths == [20, 24, 25, 30, 33, 34] and max(p["npc"] for p in old) <= 14
    assert sorted({qc.tiles(p) for p in wide.values()}) == [1, 2, 3] and max(qc.tiles(p) for p in old) <= 2
    for name in qc.LONG_NAMES:  # every long case has some launch with a wide panel
        assert any(wide[(name, items)]["npc"] > 16 for items in qc.SEEDS), name
    # -- seven waves; no drive at such an n; no drive with 33 columns; the first odd n with LD = n
    for name in ("Q4", "Q5"):
        assert J[name]["threads"] == H[name]["threads"] == 448 and 97 <= qc.CASES[name][1] <= 112
    assert sorted({p["threads"] for p in old}) == [320, 384, 512] and 100 % 16 == 4
    assert qc.CASES["Q5"][3] == 0 and J["Q5"]["mg"] == 0 and H["Q5"]["W"] == 2
    h = H["Q9"]
    assert qc.CASES["Q9"][2:] == (33, 0) and (h["sx"], h["nc"], h["W"]) == (3, 11, 22) and qc.tiles(h) == 2 and J["Q9"]["nce"] == [11] * 3
    assert (J["Q8"]["LD"], qc.CASES["Q8"][1]) == (67, 67) and min(c[1] for c in le.CASES.values() if c[1] % 2) == 81
    # -- Q9s stands where Q9 stands, at 17 columns: no drive, more than one slice, the Hessian's chain of two tiles -- and an uneven last slice
    assert (H["Q9s"]["nce"], H["Q9s"]["W"], qc.tiles(H["Q9s"])) == ([9, 8], 18, 2) and J["Q9s"]["nce"] == [9, 8]


# ---- the forced splits of the GPU tests ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", qc.NAMES)
def test_forced_splits_are_what_they_claim(name):
    kind, n, cols, m = qc.CASES[name]
    jac, hess = qc.forced_splits(name)
    seen = dict(one_col=False, ragged=False, one_unit_per_column=False, one_drive=False, all_drives=False, together=False)
    for kw in jac:
        for items in qc.ITEMS:
            for plan in (qc.jac_plan, qc.payload_plan):
                p = plan(name, items, **kw)
                assert p["bytes"] <= qc.LDS_BYTES and p["W"] <= p["NBW"] and sum(p["nce"]) == cols and sum(p["mge"]) == m, (name, kw, items)
        p = qc.jac_plan(name, **kw)
        e = qc.eval_plan(name, cols_per_slice=kw.get("cols_per_slice", 0))
        assert e["bytes"] <= qc.LDS_BYTES and sum(e["nce"]) == cols
        if kw is jac[-1]:  # the options at once
            assert kw["general_slices"] == 7 and set(kw) == {"general_slices"} | ({"cols_per_slice"} if cols > 1 else set()) | ({"large_exp_drives"} if m > 2 else set())
            seen["together"] = True
            continue
        if "cols_per_slice" in kw:
            assert max(p["nce"]) <= kw["cols_per_slice"] and max(e["nce"]) <= kw["cols_per_slice"]
            seen["one_col"] |= p["nce"] == [1] * cols
            seen["ragged"] |= qc.uneven(p["nce"])
        if kw.get("general_slices") == n:
            assert p["npc"] == 1 and p["U"] == n
            seen["one_unit_per_column"] = True
        if "large_exp_drives" in kw:
            assert max(p["mge"]) <= kw["large_exp_drives"] and max(qc.payload_plan(name, **kw)["mge"]) <= kw["large_exp_drives"]
            seen["one_drive"] |= p["mge"] == [1] * m
            seen["all_drives"] |= kw["large_exp_drives"] == m
    assert seen["one_unit_per_column"] and seen["together"]
    assert cols == 1 or (seen["one_col"] and seen["ragged"]), (name, seen)
    assert m <= 1 or (seen["one_drive"] and seen["all_drives"]), (name, seen)
    ragged_groups = [qc.uneven(plan(name, **kw)["mge"]) for kw in jac if list(kw) == ["large_exp_drives"] for plan in (qc.jac_plan, qc.payload_plan)]
    possible = any(qc.uneven(plan(name, large_exp_drives=g)["mge"]) for g in range(1, m + 1) for plan in (qc.jac_plan, qc.payload_plan))
    assert any(ragged_groups) == possible, (name, ragged_groups)
    hs = dict(one_col=False, ragged=False, one_drive=False, ragged_groups=False)
    for kw in hess:
        h = qc.hess_plan(name, **kw)
        assert h["bytes"] <= qc.LDS_BYTES and h["W"] <= h["NBW"] and sum(h["nce"]) == cols and sum(h["mge"]) == m, (name, kw)
        if "cols_per_slice" in kw:
            assert max(h["nce"]) <= kw["cols_per_slice"]
        if "large_exp_hess_drives" in kw:
            assert max(h["mge"]) <= kw["large_exp_hess_drives"]
        hs["one_col"] |= h["nce"] == [1] * cols
        hs["ragged"] |= qc.uneven(h["nce"])
        hs["one_drive"] |= h["mge"] == [1] * m
        hs["ragged_groups"] |= qc.uneven(h["mge"])
    assert cols == 1 or hs["one_col"]
    assert m <= 1 or hs["one_drive"]
    # an uneven last slice / last group wherever some cap gives one
    assert hs["ragged"] == any(qc.uneven(qc.hess_plan(name, cols_per_slice=c)["nce"]) for c in range(2, min(cols, 8))), name
    assert hs["ragged_groups"] == any(qc.uneven(qc.hess_plan(name, large_exp_hess_drives=g)["mge"]) for g in range(1, m)), name


# ---- steps --------------------------------------------------------------------------------------------------------------------------------------------
def test_steps_give_the_substep_counts():
    from vector_shape_cases import g_of

    for name in qc.NAMES:
        lay, G0, Gj, Z = qc.case(name)
        sp = [le.substeps(Z[k, lay.dt_off], g_of(lay, Z, k, G0, Gj)) for k in range(K)]
        assert sp[:2] == [1, 3] and sp[2] == int(np.ceil(qc.LONG_STEP[name])), (name, sp)
        assert (19 < sp[2] <= 21) if name in qc.UNITARY else (21 < sp[2] <= 51), (name, sp)
        for k in range(K):  # (no product near an integer: the device's norm may add in another order)
            x = abs(Z[k, lay.dt_off]) * le.norm1(g_of(lay, Z, k, G0, Gj))
            assert abs(x - round(x)) > 0.05, (name, k, x)
    seeds = {27000 + 17 * i + o for i in range(1, 14) for o in (0, 1, 77, 177, 77 + 1009)}
    assert not seeds & {25000 + 17 * i + s for i in range(0, 40) for s in range(0, 3)} and qc._seed("Q1") == 27017 and qc._seed("Q9s") == 27000 + 17 * 13


# ---- the emulations against the truths: a tenth of the GPU tolerance ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", qc.NAMES)
def test_emulation_meets_the_truth_per_segment(name):
    """Worst values read over the cases: delta 1.2e-15, Jacobian 3.2e-15, Hessian 1.6e-13 (Q2, (dt,dt) of interval 1), payload
    9.2e-16 of the scale."""
    d, j = qc.emulated(name)
    td, tj = qc.truth(name)
    ed, ej = qc.check(d, td, name, "delta", qc.FLOOR), qc.check(j, tj, name, "jac", qc.FLOOR)
    eh = qc.check(qc.emulated_hess(name), qc.hess_truth(name), name, "hess", qc.FLOOR)
    ep = []
    for explicit in (False, True):
        ref, scale = qc.payload_truth(name, explicit)
        ep.append(qc.worst(qc.payload(name, d, j, explicit)[0], ref, scale))
        assert ep[-1] <= qc.FLOOR, (name, explicit, ep)
    print("FLOOR %s: residual %s  Jacobian %s  Hessian %s  payload %.1e / %.1e" % (name, worst(ed), worst(ej), worst(eh), ep[0], ep[1]))
    assert qc.FLOOR == 1e-12 and qc.TOL == 1e-11


def test_the_sorted_check_is_check_segments():
    """qc.check (the labels sorted once per case) gives check_segments' numbers, accepts what it accepts and refuses what it refuses."""
    name = "Q8"
    got = dict(zip(("delta", "jac"), qc.emulated(name)), hess=qc.emulated_hess(name))
    ref = dict(zip(("delta", "jac"), qc.truth(name)), hess=qc.hess_truth(name))
    got["compact"], ref["compact"] = qc.compact_of(got["jac"], name), qc.compact_of(ref["jac"], name)
    for which in ref:
        assert qc.check(got[which], ref[which], name, which, qc.FLOOR) == check_segments(got[which], ref[which], qc.labels(name, which), qc.FLOOR), which
        bad = np.array(got[which])
        bad[np.abs(bad).argmax()] *= 1 + 1e-9
        assert qc.moved(got[which], bad, name, which) >= 9e-10
        for fn in (lambda: qc.check(bad, ref[which], name, which), lambda: check_segments(bad, ref[which], qc.labels(name, which), qc.TOL)):
            with pytest.raises(AssertionError):
                fn()


def test_the_per_drive_identity_on_nine_drives():
    """Q12 (m = 9, n = 72): lh.values_per_drive against the pairwise exp_hess_truth.values, per segment at the floor."""
    lay, G0, Gj, Z = qc.case("Q12")
    assert "Q12" not in qc.PER_DRIVE and set(qc.PER_DRIVE) == {"Q7", "Q10", "Q11"}
    er = qc.check(lh.values_per_drive(Z, qc.mu("Q12"), lay, G0, Gj), qc.hess_truth("Q12"), "Q12", "hess", qc.FLOOR)
    print("Q12: per-drive identity against the pairwise truth %s" % worst(er))


# ---- every case sees the faults -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", qc.NAMES)
def test_every_case_sees_the_faults_of_the_jacobian_emulation(name):
    kind, n, cols, m = qc.CASES[name]
    lay, G0, Gj, Z = qc.case(name)
    d, j = qc.emulated(name)
    faults = {"last substep": dict(drop_substep=True), "k beyond 64": dict(mm=qc.mm_drop_k_beyond_64(n)), "last row tile": dict(mm=qc.mm_zero_last_row_tile(n)),
              "last state column": dict(drop_col=True)}  # fmt: skip
    if m > 0:  # (no drive: nothing to drop, no G_l V)
        faults.update({"last drive": dict(drop_drive=True), "G_l V with the updated V": dict(updated_v=True)})
    for what, kw in faults.items():
        bd, bj = le.emulate(lay, G0, Gj, Z, **kw)
        sd, sj = qc.moved(d, bd, name, "delta"), qc.moved(j, bj, name, "jac")
        print("%s, %s: residual moved by %.1e, Jacobian by %.1e" % (name, what, sd, sj))
        assert max(sd, sj) >= qc.SEEN, (name, what, sd, sj)


@pytest.mark.parametrize("name", qc.NAMES)
def test_every_case_sees_the_faults_of_the_hessian_emulation(name):
    kind, n, cols, m = qc.CASES[name]
    lay, G0, Gj, Z = qc.case(name)
    good = qc.emulated_hess(name)
    faults = ["drop_substep", "drop_col"] + (["drop_cross", "updated_dw", "no_w_glx"] if m > 0 else [])
    for fault in faults:
        s = qc.moved(good, lh.emulate_hess(lay, G0, Gj, Z, qc.mu(name), **{fault: True}), name, "hess")
        print("%s, %s: Hessian moved by %.1e" % (name, fault, s))
        assert s >= qc.SEEN, (name, fault, s)


def uneven_slices(name):
    """(slices of a Jacobian-family plan, slices of a Hessian plan) whose last slice is narrower than the first: the plan's own where it is, else the
    one under the cap the GPU tests force; None where no cap gives one."""
    jac, hess = qc.forced_splits(name)
    j = [qc.jac_plan(name)["nce"]] + [qc.jac_plan(name, **kw)["nce"] for kw in jac if list(kw) == ["cols_per_slice"]]
    h = [qc.hess_plan(name)["nce"]] + [qc.hess_plan(name, **kw)["nce"] for kw in hess if list(kw) == ["cols_per_slice"]]
    return next((x for x in j if qc.uneven(x)), None), next((x for x in h if qc.uneven(x)), None)


def uneven_groups(name):
    jac, hess = qc.forced_splits(name)
    j = [plan(name, items)["mge"] for items in qc.ITEMS for plan in (qc.jac_plan, qc.payload_plan)]
    j += [qc.jac_plan(name, **kw)["mge"] for kw in jac if list(kw) == ["large_exp_drives"]]
    h = [qc.hess_plan(name)["mge"]] + [qc.hess_plan(name, **kw)["mge"] for kw in hess if list(kw) == ["large_exp_hess_drives"]]
    return next((x for x in j if qc.uneven(x)), None), next((x for x in h if qc.uneven(x)), None)


@pytest.mark.parametrize("name", qc.NAMES)
def test_the_mutants_of_the_new_regimes_are_seen(name):
    kind, n, cols, m = qc.CASES[name]
    d, j = qc.emulated(name)
    applied = []
    # the last slice's missing columns computed as if full
    sj, sh = uneven_slices(name)
    if sh is not None:
        s = qc.moved(qc.emulated_hess(name), qc.as_if_full_hess(name, sh), name, "hess")
        assert s >= qc.SEEN, (name, "as_if_full, Hessian", s)
        applied.append("as_if_full(H %s) %.1e" % (sh[-2:], s))
    if sj is not None:
        for explicit in (False, True):
            good, scale = qc.payload(name, d, j, explicit)
            s = payload_moved(good, qc.as_if_full_payload(name, sj, explicit), scale)
            assert s >= qc.SEEN, (name, "as_if_full, payload", explicit, s)
        applied.append("as_if_full(P %s) %.1e" % (sj[-2:], s))
    # the pair of uneven groups taken with the first group's size
    gj, gh = uneven_groups(name)
    if gh is not None:
        s = qc.moved(qc.emulated_hess(name), qc.first_group_size_hess(name, gh), name, "hess")
        assert s >= qc.SEEN, (name, "first_group_size, Hessian", s)
        applied.append("first_group_size(H %s) %.1e" % (gh, s))
    if gj is not None:
        for explicit in (False, True):
            good, scale = qc.payload(name, d, j, explicit)
            s = payload_moved(good, qc.first_group_size_payload(name, gj, explicit), scale)
            assert s >= qc.SEEN, (name, "first_group_size, payload", explicit, s)
        applied.append("first_group_size(P %s) %.1e" % (gj, s))
    # the second column tile of a wide buffer dropped: every launch of the case whose units have one
    for items in qc.ITEMS:
        p = qc.jac_plan(name, items)
        bad = qc.second_tile(name, p)
        assert (bad is None) == (p["W"] <= 16)
        if bad is not None:
            sd, sv = qc.moved(d, bad[0], name, "delta"), qc.moved(j, bad[1], name, "jac")
            assert sv >= qc.SEEN and (p["cx"] <= 16 or sd >= qc.SEEN or m > 0), (name, "second_tile", items, sd, sv)
            applied.append("second_tile(%d items, W %d, panel %d) %.1e" % (items, p["W"], p["npc"], sv))
    print("MUTANTS %s: %s" % (name, "; ".join(applied) or "none applies"))
    # which mutant applies where: the regimes' own cases by their own plans
    own_j, own_h = qc.uneven(qc.jac_plan(name)["nce"]), qc.uneven(qc.hess_plan(name)["nce"])
    assert own_j == (name in ("Q1", "Q11", "Q9s")) and own_h == (name == "Q9s")
    assert qc.uneven(qc.hess_plan(name)["mge"]) == (name in ("Q7", "Q10"))
    assert (cols > 1) == (sj is not None) and (gj is not None or name not in ("Q4", "Q6", "Q7", "Q12")) and (gh is not None or name not in ("Q7", "Q10"))
    assert any(qc.jac_plan(name, items)["W"] > 16 for items in qc.ITEMS) == (name in ["Q3", "Q9"] + qc.LONG_NAMES)


def test_the_payload_of_this_module_is_that_of_the_reduce_cases():
    """qc.payload runs xc.payload's code over this module's CASES and leaves xc's tables alone: on Q6 it gives what three float64 sums give."""
    assert not set(qc.CASES) & set(xc.CASES) and list(xc.CASES) == xc.NAMES
    name = "Q6"
    kind, n, cols, m = qc.CASES[name]
    d, j = qc.truth(name)
    lm = qc.lam(name)
    tails = j.reshape(K, xc.full_per(n, cols, m))[:, cols * n * n + cols * n :].reshape(K, cols, m + 1, n)
    g = np.einsum("kcli,kci->kl", tails, lm)
    want = np.concatenate([[np.sum(lm * d.reshape(K, cols, n))], g[:, :m].reshape(-1), g[:, m]])
    out, scale = qc.payload(name, d, j, True)
    assert out.dtype == np.longdouble and out.shape == scale.shape == (xc.payload_len(m),) and payload_moved(want, out, scale) <= 1e-14
    half = qc.payload(name, d, j, False)[0]
    assert abs(float(half[0]) - 0.5 * np.sum(d * d)) <= 1e-14 * np.sum(d * d)
