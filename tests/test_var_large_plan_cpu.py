"""The cases of tests/var_large_plan_cases.py (the launch plans of the large variational kernels, PCL_BATCH_VARIATIONAL | PCL_LARGE_N |
PCL_LARGE_VAR, and of their rollout under large_var_full) before any GPU is involved: that every number of the committed plan tables is what the
restated planners (vl.var_large_plan, vf.roll_plan) give at 256, 304 and 128 CUs and fits the LDS and the block budget; that the launches enter the
regimes they are there for; that the closed trajectory reproduces the case's own intervals and the library's value order; that the float64 lifted
oracle is within 1e-13 per segment of the truth (the longdouble values rounded once to float64: 1.1e-16 of a value at most) and the float64
restatement of the rollout within 1e-12 per knot and component of its longdouble truth on the 29- and 44-interval trajectories; and that the truths
see, at 1e-7 of a segment's size (1e4 x the GPU tolerance), the faults the cases exist for."""
import numpy as np
import pytest

import var_large_cases as vl
import var_large_full_cases as vf
import var_large_plan_cases as vp
import variational_shape_cases as vsc
import variational_truth as vt
from oracle import pade_oracle as po

FLOOR = 1e-13
ROLL_FLOOR = 1e-12  # a tenth of the GPU tolerance of the rollout
SEEN = vp.SEEN
MUTANT_ORDER = 4


def expand(width, count, last):
    return [width] * (count - 1) + [last]


# ---- the plan tables --------------------------------------------------------------------------------------------------------------------------------
def test_plan_tables():
    assert len(vp.PLAN) == 3 * len(vp.LAUNCHES) and set(vp.REGIME) == set(vp.LAUNCHES)
    for (name, K, n_cu), rows in vp.PLAN.items():
        n, C, v, m = vp.CASES[name]
        for jac, lit in zip((True, False), rows):
            row, sl, gr = vp.plan_row(name, K, n_cu, jac)
            assert row == lit, (name, K, n_cu, jac, row)
            sx, nc, last, ngrp, mg, lastg, U, blocks, nbytes = lit
            assert sl == expand(nc, sx, last) and sum(sl) == C and 1 <= last <= nc, (name, K, n_cu, sl)
            assert gr == expand(mg, ngrp, lastg) and sum(gr) == (m if jac else 0), (name, K, n_cu, gr)
            p = vp.plan(name, K, n_cu, jac)
            assert p["NB"] == vp.NB[name] and blocks <= vp.NB[name] and nbytes <= vp.LDS_BYTES, (name, K, n_cu, jac, lit)
            assert blocks == (1 + v) * nc * ((2 + 2 * (2 + mg)) if jac else 4) and p["panel_blocks"] <= vp.NB[name]
            assert U == sx * ngrp + ((1 + v) * p["pu"] if jac else 0) and p["threads"] == 64 * -(-n // 16)


def test_what_each_case_enters_on_256_cus():
    J = lambda name, K: vp.PLAN[(name, K, 256)][0]
    E = lambda name, K: vp.PLAN[(name, K, 256)][1]
    sl = lambda r: expand(r[1], r[0], r[2])
    gr = lambda r: expand(r[4], r[3], r[5])
    # R1: nc 2 (2, 2, 1), nc 3 (3, 2) at 84,720 B, nc 5 in one slice, 150 of 237 blocks, 116,880 B; the residual alone takes the same widths
    assert sl(J("R1", 28)) == [2, 2, 1] and sl(J("R1", 44)) == [3, 2] and J("R1", 44)[8] == 84720
    assert sl(J("R1", 88)) == [5] and J("R1", 88)[7:] == (150, 116880) and vp.NB["R1"] == 237
    assert all(sl(E("R1", K)) == sl(J("R1", K)) for K in (28, 44, 88))
    # R2: sx 5 x ngrp 2, drives 8 + 7, U 31 = 10 + 3 x 7, 66 of 101 blocks, 135,336 B, seven waves
    r = J("R2", 3)
    assert (r[0], r[3]) == (5, 2) and gr(r) == [8, 7] and r[6] == 31 == 10 + 3 * 7 and r[7:] == (66, 135336) and vp.NB["R2"] == 101
    assert vp.plan("R2", 3)["threads"] == 448 and 100 % 16 == 4 and vp.plan("R2", 3)["pu"] == 7
    # R3: sx 3 x ngrp 3, one drive per group, U 54 = 9 + 3 x 15, 24 of 29 blocks, 161,072 B
    r = J("R3", 3)
    assert (r[0], r[3]) == (3, 3) and gr(r) == [1, 1, 1] and r[6] == 54 == 9 + 3 * 15 and r[7:] == (24, 161072) and vp.NB["R3"] == 29
    # R4: the N = 100 plan of the bench -- sx 12, nc 4, 112 of 113 blocks, 162,528 B, U 24 -- from 10 intervals on; the residual alone nc 4, 100,448 B
    r = J("R4", 10)
    assert (r[0], r[1], r[6], r[7], r[8]) == (12, 4, 24, 112, 162528) and vp.NB["R4"] == 113 and (E("R4", 10)[1], E("R4", 10)[8]) == (4, 100448)
    assert vp.plan_row("R4", 100)[0] == r and vp.plan_row("R4", 8)[0][1] == 3 and vp.plan_row("R4", 3)[0][1] == 2
    # R5: 3 intervals, Jacobian: sx 60, nc 1, U 76, 160,840 B; 20 intervals, the residual alone: sx 10, nc 6, 48 of 48 blocks, 163,744 B
    r = J("R5", 3)
    assert (r[0], r[1], r[6], r[8]) == (60, 1, 76, 160840)
    r = E("R5", 20)
    assert (r[0], r[1], r[7], r[8]) == (10, 6, 48, 163744) and vp.NB["R5"] == 48 and vp.LDS_BYTES - r[8] == 96
    # R6: the residual alone -- sx 32, nc 2, 24 of 29 blocks, 157,960 B
    r = E("R6", 3)
    assert (r[0], r[1], r[7], r[8]) == (32, 2, 24, 157960) and vp.NB["R6"] == 29
    # R7: nc 2 (2, 2, 2, 1); nc 4 (4, 3), 160 of 171 blocks, 156,664 B at 44 and 88; the residual alone at 88: nc 7
    assert sl(J("R7", 20)) == [2, 2, 2, 1] and sl(J("R7", 44)) == sl(J("R7", 88)) == [4, 3] and J("R7", 44)[7:] == J("R7", 88)[7:] == (160, 156664)
    assert vp.NB["R7"] == 171 and sl(E("R7", 88)) == [7]
    # VL2: nc 3 in 11 slices; nc 6 (6, 6, 6, 6, 6, 3), 152,264 B; the residual alone at 20: nc 6, 75,080 B
    assert sl(J("VL2", 8)) == [3] * 11 and sl(J("VL2", 20)) == [6, 6, 6, 6, 6, 3] and J("VL2", 20)[8] == 152264 and (E("VL2", 20)[1], E("VL2", 20)[8]) == (6, 75080)
    # ... none of which the cases of var_large_cases enter at their own three or four intervals: nc <= 2, and slices never crossed with groups
    for name in vl.NAMES:
        n, C, v, m = vl.shape(name)
        for jac in (True, False):
            q = vl.var_large_plan(n, C, m, v, jac=jac, items=vl.knot(name)[0] - 1)
            assert q["nc"] <= 2 and (q["sx"] == 1 or q["ngrp"] == 1), name


def test_regimes_hold_on_256_cus_and_cover_the_list():
    seen_j, seen_e = set(), set()
    for (name, K), (ncj, nce, crossed, uneven) in vp.REGIME.items():
        n, C, v, m = vp.CASES[name]
        j, e = vp.plan(name, K, 256), vp.plan(name, K, 256, jac=False)
        assert e["nc"] == nce and (ncj is None or j["nc"] == ncj), (name, K)
        assert crossed == (j["sx"] > 1 and j["ngrp"] > 1) and uneven == (vp.groups(j, m)[-1] < j["mg"]), (name, K)
        seen_e.add(nce)
        if ncj is not None:
            seen_j.add(ncj)
    assert {3, 4, 5, 6} <= seen_j and {6, 7} <= seen_e
    assert any(c for _, _, c, _ in vp.REGIME.values()) and any(u for _, _, _, u in vp.REGIME.values())
    assert vp.plan("R5", 20, 256, jac=False)["chain_blocks"] == vp.NB["R5"]  # 48 of 48
    assert sorted({w for _, w in vp.ROLLS.values()}) == [20, 27, 33]


def test_rollout_plan_tables():
    assert {(name, K) for name, K, _ in vp.ROLL} == set(vp.ROLLS)
    for (name, K, n_cu), lit in vp.ROLL.items():
        n, C, v, m = vp.CASES[name]
        r = vp.roll_plan(name, K, n_cu)
        assert vp.roll_row(name, K, n_cu) == lit, (name, K, n_cu, vp.roll_row(name, K, n_cu))
        P, npc, last, be, S, nc, bc = lit
        assert r["npce"] == expand(npc, P, last) and sum(r["npce"]) == n and r["nce"] == expand(nc, S, C - (S - 1) * nc), (name, K, n_cu)
        assert be <= vp.LDS_BYTES and bc <= vp.LDS_BYTES and r["grid_e"] == K * (1 + v) * P
    for (name, K), (seed, width) in vp.ROLLS.items():
        assert vp.ROLL[(name, K, 256)][1] == width > 16, (name, K)
    assert vp.ROLL[("R1", 29, 256)][:4] == (2, 33, 33, 142608) and vp.ROLL[("R7", 29, 256)][:4] == (4, 20, 20, 130744)
    assert vp.ROLL[("R7", 44, 256)][:4] == (3, 27, 26, 157960)
    # the cases of var_large_full_cases at their own intervals: one panel per 16 columns
    for name in vf.NAMES:
        n, C, v, m = vl.shape(name)
        assert vf.roll_plan(n, C, m, v, K=vl.knot(name)[0] - 1)["npc"] <= 16, name
    # general_slices can only raise the panel count
    assert vp.roll_plan("R1", 29, slices=1)["npc"] == 33 and vp.roll_plan("R1", 29, slices=5)["npc"] == 14 and vp.roll_plan("R1", 29, slices=66)["npc"] == 1


# ---- what pcl_create decides about a count of kets ---------------------------------------------------------------------------------------------------
def test_a_large_variational_context_takes_any_count_of_kets():
    """R1, R2, R3 and R7 hold 5, 5, 3 and 7 kets: between one ket and the d columns of a unitary.  pcl_create takes such a count on a large variational
    context (the kernels are planned per slice of state columns) and nowhere else -- decided before the device is touched."""
    import torch

    import piccolo_jl_amd as pa

    pa.build_library()
    L = pa._lib

    def desc(d, cols, flags=L.PCL_LARGE_N | L.PCL_LARGE_VAR, v=2):
        n = 2 * d
        xdc = n * cols
        return dict(d=d, m=1, N=3, z_dim=(1 + v) * xdc + 3, u_off=(1 + v) * xdc + 2, dt_off=(1 + v) * xdc, x_offs=[b * xdc for b in range(1 + v)],
                    G0=np.zeros((1 + v, n, n)), Gj=np.zeros((1, n, n)), batch=1 + v, per_member_G0=True, state_cols=cols, pade_order=8,
                    batch_mode=L.PCL_BATCH_VARIATIONAL | flags)  # fmt: skip

    def refused(code, *words, **kw):
        with pytest.raises(pa.PclError) as ei:
            pa.integrators._PclContext(**kw)
        assert ei.value.code == code, str(ei.value)
        for w in words:
            assert w in str(ei.value), str(ei.value)

    for name in ("R1", "R2", "R3", "R7"):
        n, C, v, m = vp.CASES[name]
        assert 1 < C < n // 2
        if torch.cuda.is_available():
            pa.integrators._PclContext(**desc(n // 2, C, v=v)).close()
        else:
            refused(L.PCL_EHIP, "no CPU path", **desc(n // 2, C, v=v))
    words = ("state_cols=", "takes d (unitary, or 0) or 1 (ket)")
    refused(L.PCL_EINVAL, *words, **desc(33, 34))  # more than d
    refused(L.PCL_EINVAL, *words, **desc(33, -2))
    refused(L.PCL_EINVAL, *words, **desc(27, 5))  # the flags at n <= 64: the ordinary variational context
    refused(L.PCL_EINVAL, *words, **desc(33, 5, flags=0))  # without the flags
    refused(L.PCL_EINVAL, *words, **desc(8, 5, flags=0))


# ---- the closed trajectory ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", vp.NAMES)
def test_closed_trajectory(name):
    b, cs = vp.base(name), vp.case(name)
    P = vp.periods(name)
    assert P == (5 if name == "VL2" else 4) and cs.N == P + 1 and cs.K == P and (cs.n, cs.C, cs.v, cs.m) == vp.CASES[name]
    same = np.ones(b.Z.shape, bool)
    same[P - 1, b.dt_off] = False  # the wrap interval's step: the only entry that differs
    assert np.array_equal(cs.Z[:P][same], b.Z[same]) and np.array_equal(cs.Z[P], cs.Z[0])
    if name in ("R4", "VL2"):
        assert b is vl.case(vp.BORROWED[name])[0]
    th = [cs.Z[k, cs.dt_off] * vsc._lifted_norm(cs, k) for k in range(P)]
    want = [0.15, -0.3, vp.LONG[name]] + ([0.0] if name == "VL2" else []) + [vp.WRAP_STEP]
    assert np.allclose(th, want, rtol=1e-12, atol=0), (name, th)
    Zl = vp.long_knots(name, 11)
    assert Zl.shape == (12, cs.z_dim) and all(np.array_equal(Zl[k], cs.Z[k % P]) for k in range(12))
    lc = vp.long_case(name, 11)
    assert lc.K == 11 and lc.N == 12


def test_the_closed_trajectory_reproduces_the_cases_own_intervals_exactly():
    """The truth of the first P - 1 intervals of the closed trajectory is the truth of the case's own trajectory, bit for bit (R1; and VL2 against
    var_large_cases' own truth)."""
    for k in range(3):
        a = vp.lifted_interval("R1", 6, k)
        b = vp.lifted_interval("R1", 6, k, cs=vp.base("R1"))
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    d, j = vl.truth("VL2", 4)
    d2, j2 = vp.truth("VL2", 4)
    assert np.array_equal(d2[: d.size], d) and np.array_equal(j2[: j.size], j)


def test_value_order_is_the_lifted_structure_on_r2():
    cs = vp.case("R2")
    lay = vt.lifted(cs)[1]
    rows, cols = po.jac_structure(lay)
    rm, cm = vt._row_map(cs), vt._col_map(cs, lay)
    jr, jc = (rows // cs.xd) * cs.xd + rm[rows % cs.xd], cm[cols]
    perl = len(rows) // cs.K
    idx = (np.arange(cs.K)[:, None] * perl + vl.value_index(cs)[None]).reshape(-1)
    r, c = vl.lib_structure(cs)
    assert len(r) == cs.K * vl.values_per_interval(cs) and len(np.unique(idx)) == len(idx)
    assert np.array_equal(r, jr[idx]) and np.array_equal(c, jc[idx])


@pytest.mark.parametrize("name", vp.NAMES)
def test_long_step_is_the_smallest_that_shows_the_top_term(name):
    if name in ("R4", "VL2"):
        assert vp.LONG[name] == vl.LONG[vp.BORROWED[name]]
        return
    found, seen = vp.long_step_search(name)
    print("%s: %s" % (name, ", ".join("%.2f: %.1e" % kv for kv in seen.items())))
    assert found == vp.LONG[name] and all(w < SEEN for s, w in seen.items() if s < found), (name, found, seen)


def test_delta_truth_is_the_lifted_truth():
    """delta_truth_ld (R6's truth, block by block) against vector_shape_cases.truth_values on the lifted problem, both in longdouble, on R1."""
    cs = vp.case("R1")
    for order in (4, 10):
        d = vp.delta_truth_ld(cs, order)
        for k in range(cs.K):
            ref = vp.lifted_interval("R1", order, k)[0]
            assert np.abs(d[k] - ref).max() <= 1e-17 * np.abs(ref).max(), (order, k)


# ---- the reference floor ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", vp.NAMES)
def test_float64_oracle_meets_the_truth_at_the_floor(name):
    cs = vp.case(name)
    Zl, lay, G0l, Gjl = vt.lifted(cs)
    vi = vl.value_index(cs)
    worst = [0.0, 0.0]
    for order in vp.ORDERS[name]:
        d, j = vp.truth(name, order)
        wd = vp.assert_segments(vp.segment_errors(name, "delta", vt.residual(cs, order), d), FLOOR, "%s order %d residual" % (name, order))
        worst[0] = max(worst[0], wd[0])
        if j is not None:
            oj = po.pade_jacobian_values(Zl, lay, G0l, Gjl, order).reshape(cs.K, -1)[:, vi].reshape(-1)
            wj = vp.assert_segments(vp.segment_errors(name, "jac", oj, j), FLOOR, "%s order %d Jacobian" % (name, order))
            worst[1] = max(worst[1], wj[0])
    print("%s: float64 lifted oracle against the truth: residual %.1e, Jacobian %.1e" % (name, worst[0], worst[1]))


def test_the_sorted_check_is_vl_checks_rule():
    """vp.segment_errors / assert_segments (one interval's codes sorted once) give the numbers of vsc.segment_errors / assert_segments on the codes of
    the whole launch, accept what they accept and refuse what they refuse."""
    name, order = "R1", 6
    cs = vp.case(name)
    d, j = vp.truth(name, order)
    r, c = vl.lib_structure(cs)
    dc, jc = vsc.residual_codes(cs, np.arange(cs.K * cs.xd)), vsc.jac_codes(cs, r, c)
    Zl, lay, G0l, Gjl = vt.lifted(cs)
    od = vt.residual(cs, order)
    oj = po.pade_jacobian_values(Zl, lay, G0l, Gjl, order).reshape(cs.K, -1)[:, vl.value_index(cs)].reshape(-1)
    for which, codes, got, ref, name_of in (("delta", dc, od, d, vsc.residual_name), ("jac", jc, oj, j, vsc.jac_name)):
        theirs = {name_of(cs, s): es for s, es in vsc.segment_errors(codes, got, ref).items()}
        ours = vp.segment_errors(name, which, got, ref)
        assert ours.keys() == theirs.keys() and all(ours[s] == (float(theirs[s][0]), float(theirs[s][1])) for s in ours), which
        assert vp.assert_segments(ours, FLOOR, which)[0] == vsc.assert_segments(vsc.segment_errors(codes, got, ref), FLOOR, lambda s: name_of(cs, s), which)[0]
        bad = np.array(got)
        bad[np.abs(bad).argmax()] *= 1 + 1e-9
        with pytest.raises(AssertionError):
            vp.assert_segments(vp.segment_errors(name, which, bad, ref), 1e-11, which)
        bad = np.array(got)
        bad[5] = np.nan
        with pytest.raises(AssertionError):
            vp.assert_segments(vp.segment_errors(name, which, bad, ref), 1e-11, which)
    # an identically-zero segment is held to exact zeros: VL2's zero step
    d, j = vp.truth("VL2", 4)
    errs = vp.segment_errors("VL2", "jac", j, j)
    assert errs["r1.X0@0#3"] == (0.0, 0.0) and errs["r0.u@0#3"] == (0.0, 0.0) and errs["r1.X0@0#4"][1] > 0
    bad = np.array(j)
    one, uniq, order_, starts = vp.segments("VL2", "jac")
    per = order_.size
    zero_seg = np.flatnonzero(uniq == [s for s in uniq if vp.segment_name("VL2", "jac", s, 3) == "r0.u@0#3"][0])[0]
    bad[3 * per + order_[starts[zero_seg]]] = 1e-300
    with pytest.raises(AssertionError):
        vp.check("VL2", 4, d, bad)


# ---- the truth sees the faults the cases exist for ----------------------------------------------------------------------------------------------------
def _truth_interval(name, k=0):
    cs = vp.case(name)
    d, j = vp.truth(name, MUTANT_ORDER)
    return d.reshape(cs.K, -1)[k], j.reshape(cs.K, -1)[k]


@pytest.mark.parametrize("name", ["R2", "R3"])
def test_the_truth_sees_group_faults(name):
    """The last drive group ignored, the tails of two groups exchanged, the unit decode swapped (s = u / ngrp, g = u % ngrp)."""
    n, C, v, m = vp.CASES[name]
    p = vp.plan(name, 3)
    sl, gr = vp.slices(p, C), vp.groups(p, m)
    assert len(sl) > 1 and len(gr) > 1
    d, j = _truth_interval(name)
    kw = dict(drop_drive=True) if gr[-1] == 1 else dict(gj_zero_from=m - gr[-1])  # (R3: the last group is the last drive)
    bd, bj = vp.lifted_interval(name, MUTANT_ORDER, 0, **kw)
    seen = {"the last group ignored": max(vp.moved(name, "delta", d, bd), vp.moved(name, "jac", j, bj)),
            "two groups exchanged": vp.moved(name, "jac", j, vp.exchange_groups(name, j, gr)),
            "the unit decode swapped": vp.moved(name, "jac", j, vp.swapped_decode(name, j, sl, gr))}  # fmt: skip
    for what, s in seen.items():
        print("%s, %s: moved by %.1e" % (name, what, s))
        assert s >= SEEN, (name, what, s)
    # the swapped decode is a permutation of the tails and nothing else
    sw = vp.swapped_decode(name, j, sl, gr)
    nb = (2 + 4 * v) * C * n * n
    assert np.array_equal(sw[:nb], j[:nb]) and not np.array_equal(sw[nb:], j[nb:])


@pytest.mark.parametrize("name,K", [("R1", 44), ("R1", 88), ("R7", 88)])
def test_the_truth_sees_slice_faults(name, K):
    """At the widest slices: the last slice's columns dropped; a column c >= 2 of a slice reading column c - 2's additive term."""
    n, C, v, m = vp.CASES[name]
    sl = vp.slices(vp.plan(name, K), C)
    assert max(sl) >= 3
    d, j = _truth_interval(name)
    bd, bj = vp.lifted_interval(name, MUTANT_ORDER, 0, zero_cols=range(C - sl[-1], C))
    s1 = max(vp.moved(name, "delta", d, bd), vp.moved(name, "jac", j, bj))
    cd, cj = vp.column_reads_two_back(name, d, j, sl)
    s2 = max(vp.moved(name, "delta", d, cd), vp.moved(name, "jac", j, cj))
    print("%s at %d intervals, slices %s: the last slice dropped moves by %.1e, column c - 2's term by %.1e" % (name, K, sl, s1, s2))
    assert s1 >= SEEN and s2 >= SEEN, (name, s1, s2)


@pytest.mark.parametrize("name,K", list(vp.ROLLS))
def test_rollout_floor_and_faults(name, K):
    """The float64 restatement against the longdouble truth on the long trajectory; the steps walk every branch of the substep rule; the truth sees
    one substep in place of s', and the columns >= 16 of each panel of E, and of every L_i, read as zero."""
    cs, sp = vp.roll_case(name, K)
    seed, width = vp.ROLLS[(name, K)]
    assert cs.K == K and sp[1] == vp.LONG_SUB >= 20 and sp[2] == 0 and sp[3] == 3 and set(sp[4:]) == {1} and sp[0] == 1
    n1 = [np.abs(vf.g_of(cs, k)).sum(axis=0).max() * cs.Z[k, cs.dt_off] for k in range(K)]
    assert np.allclose(n1[4:], [(1 if seed else -1) * (-1) ** k * 0.8 for k in range(4, K)], rtol=1e-12) and abs(n1[3] + 2.5) < 1e-12
    sens = np.concatenate([cs.Z[0, o : o + cs.xdc] for o in cs.xo[1:]])
    assert sens.any() == bool(seed)
    truth = vp.rollout_truth_ld(name, K)
    full = vf.restatement(cs)
    e = vf.knot_errors(full, truth, cs)
    print("%s, %d intervals: float64 restatement against the truth %.1e" % (name, K, e.max()))
    assert e.max() <= ROLL_FLOOR, (name, K, e.max())
    npce = vp.roll_plan(name, K)["npce"]
    assert max(npce) == width
    seen = {"one substep": vf.knot_errors(vf.restatement(cs, mutant="one_substep"), truth, cs).max(),
            "E beyond column 16 of a panel": vf.knot_errors(vp.restatement_with_panels(cs, npce, "E"), truth, cs).max(),
            "L_i beyond column 16 of a panel": vf.knot_errors(vp.restatement_with_panels(cs, npce, "L"), truth, cs).max()}  # fmt: skip
    for what, s in seen.items():
        print("%s, %d intervals, %s: moved by %.1e" % (name, K, what, s))
        assert s >= SEEN, (name, K, what, s)
    assert np.array_equal(vp.restatement_with_panels(cs, [16] * -(-cs.n // 16), "E"), full)  # (panels of 16 columns: nothing to zero)
