"""The cases of tests/fused_batch_cases.py before any GPU is involved: that each can do its job in tests/test_fused_batch_gpu.py.

Case table: every claim is recomputed with the launch code's arithmetic restated in fused_batch_cases (launch, ticket_ok, ticket_grid, tick_cpi,
group_visits, ring_refills, ring_slot, hess_rpre_auto) at n_cu = 256, with the numbers written out here -- a restatement that drifts (a ring of 64 slots,
tick_cpi not raised at 32 slices, a grid that ignores the slices) fails this module -- and the rules that read n_cu also at 128 and 304.

Sensitivity: at every (case, order) the neighbouring order moves delta and the Jacobian values of every interval with a step by 1e4 x the GPU tolerance.

Fault visibility, on the truth alone (SEEN = 1e-7 of a segment's own size): B1 -- a visit that reads the controls and the step of the visit 128 earlier
(a ring slot read before its refill); B3, B5 -- a slice whose -B+ / B- columns come from the group's next interval."""
import numpy as np
import pytest

import fused_batch_cases as fc
import unitary4_cases as uc
from oracle import pade_oracle as po
from shape_cases import assert_sensitive, check_segments, lower_order

CASE_ORDERS = [(name, order) for name in fc.CASES for order in fc.CASES[name][1]]
L = fc.launch


def _bk(name, n_cu=256):
    B = fc.CASES[name][3] if name == "B7" else fc.seeds(name, n_cu)
    return B * (fc.CASES[name][2] - 1)


# ---- the restated arithmetic itself ---------------------------------------------------------------------------------------------------------------
def test_restated_arithmetic():
    assert (fc.UHR_SLOTS, fc.UHR_REFILL, fc.TICKET_RING_BYTES, fc.LDS_BYTES) == (128, 64, 8192, 163840)
    assert [fc.ring_slot(v) for v in (0, 63, 64, 127, 128, 191, 192, 259)] == [0, 63, 64, 127, 0, 63, 64, 3]
    assert [fc.ring_refills(v) for v in (0, 1, 64, 65, 128, 205, 260)] == [0, 1, 1, 2, 2, 4, 5]
    assert [fc.tick_cpi(d) for d in (9, 13, 32)] == [4, 4, 4] and fc.tick_cpi(3) == 3
    assert (fc.tick_cpi(32, 1), fc.tick_cpi(31, 1), fc.tick_cpi(32, 2), fc.tick_cpi(13, 27)) == (2, 1, 2, 13)  # (32 slices > 31: raised)
    assert fc.v4_lds_bytes(32, 2, 3) == 149952 and fc.v4_lds_bytes(31, 4, 2) == 156432 and fc.v4_lds_bytes(9, 1, 2) == 9768
    assert fc.v4_power_tiles(32, 2, 5) == 3 and fc.v4_power_tiles(31, 4, 5) == 2 and fc.v4_power_tiles(9, 1, 5) == 6 and fc.v4_power_tiles(9, 1, 1) == 2
    assert fc.v4_power_tiles(32, 6, 2) == 0  # (no LDS for kernel 4's tiles)
    assert fc.round_robin(260, 9, 256) == (9, 1, 260) and fc.round_robin(40, 13, 256) == (3, 5, 200) and fc.round_robin(125, 9, 256) == (5, 2, 250)
    assert fc.round_robin(40, 13, 256, cols_per_slice=5) == (5, 3, 120) and fc.round_robin(5, 9, 256) == (1, 9, 45)
    assert fc.contiguous_auto(552, 13, 256) and not fc.contiguous_auto(551, 13, 256) and not fc.contiguous_auto(552, 13, 256, compact=True)
    assert fc.group_values(256) == [1, 8, 16, 256] and fc.group_values(304) == [1, 8, 16, 304] and fc.group_values(120) == [1, 8, 15, 120]
    assert (fc.tick_group(256), fc.tick_group(256, 16), fc.tick_group(256, 1000), fc.tick_group(4)) == (8, 16, 256, 4)
    # ticket_ok, condition by condition
    ok = dict(d=13, m=2, q=2, bk=552, n_cu=256)
    assert fc.ticket_ok(**ok) and not fc.ticket_ok(**ok, grid=7) and not fc.ticket_ok(**ok, compact=True) and not fc.ticket_ok(**ok, v4_group=7)
    assert not fc.ticket_ok(**dict(ok, m=7)) and fc.ticket_ok(**dict(ok, m=6, d=9))  # m + 10 waves
    assert fc.ticket_ok(32, 2, 5, 40, 256) and not fc.ticket_ok(31, 4, 5, 20, 256)  # the tiles and the ring within the LDS
    assert fc.ticket_ok(13, 2, 2, 15, 256, v4_group=16) and not fc.ticket_ok(13, 2, 2, 1, 256, v4_group=16)  # a grid of 13 workgroups holds no group of 16
    assert fc.ticket_grid(1, 13, 256) == 13 and fc.ticket_grid(205, 9, 256) == 205 and fc.ticket_grid(260, 9, 256) == 256
    # the ring of power tiles
    assert L(9, 1, 5, 260, 256, v4_ticket=0)["v4_np"] == 4 and L(9, 1, 5, 5, 256)["v4_np"] == 5 and L(9, 1, 5, 260, 256, v4_ticket=1)["v4_np"] == 6
    assert L(9, 1, 1, 260, 256, v4_ticket=0)["v4_np"] == 1 and L(9, 1, 1, 5, 256)["v4_np"] == 1 and L(9, 1, 1, 260, 256, v4_ticket=1)["v4_np"] == 2
    assert L(9, 1, 5, 260, 256, v4_ticket=0, v4_power_tiles=2)["flags"] == 4 and L(9, 1, 5, 260, 256, v4_ticket=0, v4_power_tiles=4)["flags"] == 0
    assert L(9, 1, 2, 260, 256, v4_ticket=0, v4_power_tiles=1)["flags"] == 0  # (q >= 5 only)
    assert L(9, 1, 5, 260, 256, v4_ticket=0, v4_flags=16)["flags"] == 20 and L(9, 1, 5, 5, 256, v4_flags=8)["one_item"] == 0
    # visits
    assert fc.group_visits(260, 256, 256) == [260] and fc.group_visits(8, 216, 8) == [1] * 8 + [0] * 19
    assert fc.group_visits(250, 250, 8)[-1] == 8 and len(fc.group_visits(250, 250, 8)) == 32  # (the two workgroups past the last whole group walk 31, 62, ..)
    assert fc.hess_groups(13, 2) == (10, 2) and fc.hess_groups(27, 6) == (4, 7) and fc.rchain_blocks(1025) == 1032 and fc.rchain_blocks(1024) == 1024


# ---- the case table's claims ------------------------------------------------------------------------------------------------------------------------
def test_case_table_at_256_cus():
    n_cu = 256
    dm = {name: fc.dims(name) for name in fc.CASES}
    assert dm == {"B1": (9, 1), "B2": (13, 2), "B3": (13, 4), "B4": (20, 3), "B5": (32, 2), "B6": (31, 4), "B7": (20, 3), "H1": (13, 2)}
    assert {name: _bk(name) for name in fc.CASES} == {"B1": 260, "B2": 552, "B3": 40, "B4": 40, "B5": 40, "B6": 20, "B7": 15, "H1": 1025}
    assert fc.system("B7")[0].shape == (3, 40, 40) and fc.x_offs("B7") == [0, 800, 1600] and fc.layout("B7").u_off == 2402
    # B1: one group of all workgroups, the ring's refills, exhausted intervals, groups without an interval, the one-tile ring, the borrowed tile
    t = L(9, 1, 1, 260, n_cu, v4_ticket=1)
    assert (t["ticket"], t["grid"], t["groups"], t["slices"], t["v4_np"], t["tail"], t["lds"]) == (4, 256, 32, 3, 2, 0, 9768 + 8192)
    assert [min(4, 9 - 4 * s) for s in range(t["slices"])] == [4, 4, 1]
    one = L(9, 1, 1, 260, n_cu, v4_ticket=1, v4_group=n_cu)
    assert one["groups"] == 1 and fc.group_visits(260, 256, 256) == [260] and fc.ring_refills(260) == 5
    assert sorted({fc.ring_slot(v) for v in range(128, 260)}) == list(range(128))  # every slot is rewritten: refills 2 and 3, and refill 4 rewrites 0 .. 3 again
    assert 256 * 1 > 3  # (256 workgroups walk every interval, three find a slice)
    v8, v1 = fc.group_visits(260, 256, 8), fc.group_visits(260, 256, 1)
    assert v8 == [9] * 4 + [8] * 28 and v1 == [2] * 4 + [1] * 252
    r = L(9, 1, 1, 260, n_cu, v4_ticket=0, contiguous=0)
    assert (r["units"], r["grid"], r["v4_np"], r["one_item"], r["contig"]) == (260, 256, 1, 0, 0)  # four workgroups walk two items, a ring of one tile
    c = L(9, 1, 1, 260, n_cu, v4_ticket=0, contiguous=1)
    assert (c["units"], c["grid"], c["v4_np"]) == (2340, 256, 1) and 2340 % 256 != 0  # ranges begin and end inside an interval
    r10 = L(9, 1, 5, 260, n_cu, v4_ticket=0, contiguous=0)
    assert (r10["np"], r10["v4_np"], r10["borrowed"], r10["flags"]) == (6, 4, 1, 0) and r10["borrowed"] == dm["B1"][1]
    f10 = L(9, 1, 5, 260, n_cu, v4_ticket=0, contiguous=0, v4_power_tiles=2)
    assert (f10["v4_np"], f10["flags"], f10["borrowed"]) == (2, 4, 0)
    assert fc.windows("B1", n_cu) == [(1, 50), (1, 25)]
    w = L(9, 1, 1, 125, n_cu, v4_ticket=1, v4_group=1)
    assert (w["ticket"], w["grid"], w["groups"]) == (4, 250, 250) and fc.group_visits(125, 250, 1) == [1] * 125 + [0] * 125
    w = L(9, 1, 1, 250, n_cu, v4_ticket=1)
    assert (w["grid"], w["groups"]) == (250, 31) and fc.group_visits(250, 250, 8) == [9] * 2 + [8] * 29 + [8]
    assert L(9, 1, 1, 250, n_cu, v4_ticket=1, v4_group=n_cu)["ticket"] == 0  # no whole group: the static split
    # (the issue's 41 seeds: a grid of 205 workgroups, and no group under v4_group n_cu)
    assert fc.ticket_grid(205, 9, n_cu) == 205 and 205 // fc.tick_group(n_cu, n_cu) == 0 and L(9, 1, 1, 205, n_cu, v4_ticket=1, v4_group=n_cu)["ticket"] == 0
    # B2: both sides of bk d >= 28 n_cu
    assert fc.seeds("B2", n_cu) == 184 and fc.windows("B2", n_cu) == [(1, 182), (0, 183)]
    assert 552 * 13 == 7176 >= 28 * n_cu == 7168 > 549 * 13 == 7137 and 551 * 13 < 7168
    hi, lo = L(13, 2, 2, 552, n_cu, v4_ticket=0), L(13, 2, 2, 549, n_cu, v4_ticket=0)
    assert (hi["contig"], hi["units"], hi["grid"]) == (1, 7176, 256) and (lo["contig"], lo["S"], lo["units"], lo["grid"], lo["v4_np"]) == (0, 1, 549, 256, 1)
    # ranges of 28 or 29 columns: they begin mid-interval, and every one of the 183 trajectory boundaries (39 columns apart) lies inside one
    assert 7176 % 256 != 0 and 7176 // 256 == 28 and 28 % 13 != 0 and 28 < 3 * 13
    assert L(13, 2, 2, 552, n_cu, v4_ticket=-1, v4_tune=0)["ticket"] == 4 and L(13, 2, 2, 549, n_cu, v4_ticket=-1, v4_tune=0)["ticket"] == 0
    assert L(13, 2, 2, 552, n_cu, v4_ticket=-1, v4_tune=0, contiguous=1)["ticket"] == 0 and L(13, 2, 3, 552, n_cu, v4_ticket=-1, v4_tune=0)["ticket"] == 0
    # B3: the slice widths
    assert [L(13, 4, 3, 40, n_cu, v4_ticket=1, v4_ticket_cols=c)["slices"] for c in fc.TICKET_COLS["B3"]] == [13, 4, 3, 1]
    assert [L(13, 4, 3, 40, n_cu, v4_ticket=1, v4_ticket_cols=c)["ticket"] for c in fc.TICKET_COLS["B3"]] == [1, 4, 5, 13] and 13 - 3 * 4 == 1 and 4 + 10 <= 16
    t = L(13, 4, 3, 40, n_cu, v4_ticket=1)
    assert (t["grid"], t["groups"], t["v4_np"], t["np"]) == (200, 25, 4, 4) and L(13, 4, 3, 40, n_cu, v4_ticket=1, v4_group=n_cu)["ticket"] == 0
    # B4: streamed drift classes; tickets and both static splits
    t, r, c = (L(20, 3, 4, 40, n_cu, coop=False, **o) for o in (dict(v4_ticket=1), dict(v4_ticket=0, contiguous=0), dict(v4_ticket=0, contiguous=1)))
    assert (t["ticket"], t["slices"], t["lds"]) == (4, 5, 78912 + 8192) and (r["units"], r["one_item"]) == (200, 1) and (c["units"], c["v4_np"], c["borrowed"]) == (800, 3, 0)
    # B5: every lane of a half wave, more than 31 slices, the tightest ticket LDS, a ring of 3 with two borrowed tiles
    assert L(32, 2, 2, 40, n_cu, v4_ticket=1, v4_ticket_cols=1)["ticket"] == 2 and L(32, 2, 2, 40, n_cu, v4_ticket=1, v4_ticket_cols=1)["slices"] == 16
    t = L(32, 2, 5, 40, n_cu, v4_ticket=1, v4_group=16)
    assert (t["np"], t["v4_np"], t["lds"], t["grid"], t["groups"]) == (3, 3, 158144, 240, 15) and t["lds"] <= fc.LDS_BYTES
    assert fc.group_visits(40, 240, 16) == [3] * 10 + [2] * 5
    c = L(32, 2, 5, 40, n_cu, v4_ticket=0, contiguous=1)
    assert (c["units"], c["grid"], c["v4_np"], c["borrowed"], c["flags"]) == (1280, 256, 3, 2, 0) and c["borrowed"] == dm["B5"][1]
    assert 40 * po.jac_nnz_per_interval(fc.layout("B5")) * 8 < 200e6
    # B6: no LDS for the ring of controls
    assert all(fc.v4_power_tiles(31, 4, q) == 2 for q in range(1, 6))
    assert fc.v4_lds_bytes(31, 4, 2) + 8192 == 164624 > fc.LDS_BYTES and not fc.ticket_ok(31, 4, 5, 20, n_cu)
    t, c = L(31, 4, 5, 20, n_cu, v4_ticket=1), L(31, 4, 5, 20, n_cu, v4_ticket=0, contiguous=1)
    assert (t["ticket"], t["one_item"], t["lds"]) == (0, 1, 156432) and (c["units"], c["v4_np"], c["borrowed"], c["flags"]) == (620, 2, 3, 0) and 3 <= dm["B6"][1]
    # B7: an ensemble of 15 intervals
    t = L(20, 3, 2, 15, n_cu, v4_ticket=1, merit=True)
    assert (t["ticket"], t["grid"], t["groups"], t["slices"]) == (4, 150, 18, 5) and L(20, 3, 2, 15, n_cu, v4_ticket=-1, v4_tune=0, merit=True)["ticket"] == 0
    assert fc.windows("B7", n_cu) == [(1, 1)]
    # H1: the R-chain rule
    assert fc.seeds("H1", n_cu) == 205 and fc.hess_groups(13, 2) == (10, 2) and 13 - 10 == 3
    assert 1025 * 2 > 8 * n_cu >= 1020 * 2 and fc.hess_rpre_auto(1025, 13, 2, 4, n_cu) == 1 and fc.hess_rpre_auto(1020, 13, 2, 4, n_cu) == 0
    assert fc.hess_rpre_auto(1025, 13, 2, 3, n_cu) == 0 and 1025 % 8 and fc.rchain_blocks(1025) == 1032
    # every single-trajectory launch is the one-item module's
    for name, order in CASE_ORDERS:
        d, m = dm[name]
        assert L(d, m, order // 2, fc.CASES[name][2] - 1, n_cu)["one_item"] == 1, (name, order)


@pytest.mark.parametrize("n_cu", [128, 256, 304])
def test_counts_follow_n_cu(n_cu):
    """What the GPU module computes from the device's n_cu stays on the claimed side of each rule."""
    bk = _bk("B1", n_cu)
    assert n_cu < bk <= n_cu + 5 and fc.ticket_grid(bk, 9, n_cu) == n_cu
    t = L(9, 1, 1, bk, n_cu, v4_ticket=1, v4_group=n_cu)
    assert t["groups"] == 1 and fc.ring_refills(fc.group_visits(bk, n_cu, n_cu)[0]) >= 3  # the ring wraps
    assert L(9, 1, 1, bk, n_cu, v4_ticket=0, contiguous=0)["units"] > n_cu
    for first, count in fc.windows("B1", n_cu):
        assert 1 <= count and first + count <= fc.seeds("B1", n_cu) and L(9, 1, 1, count * 5, n_cu, v4_ticket=1, v4_group=n_cu)["ticket"] == 0
    B = fc.seeds("B2", n_cu)
    assert B * 3 * 13 >= 28 * n_cu > (B - 1) * 3 * 13 and fc.windows("B2", n_cu)[1] == (0, B - 1)
    B = fc.seeds("H1", n_cu)
    assert fc.hess_rpre_auto(5 * B, 13, 2, 4, n_cu) == 1 and (5 * B) % 8 != 0 and fc.hess_rpre_auto(5 * (B - 2), 13, 2, 4, n_cu) == 0
    for g in fc.group_values(n_cu):
        assert n_cu % g == 0
    for name, order in CASE_ORDERS:
        d, m = fc.dims(name)
        if name != "H1":  # a ticket launch has at least one whole group, or is refused
            for g in fc.group_values(n_cu):
                for bk_ in [_bk(name, n_cu)] + [c * (fc.CASES[name][2] - 1) for _, c in fc.windows(name, n_cu)]:
                    t = L(d, m, order // 2, bk_, n_cu, v4_ticket=1, v4_group=g)
                    assert (t["ticket"] > 0) == (t["groups"] >= 1), (name, order, g, bk_)


# ---- steps, zeros, sensitivity ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(fc.CASES))
def test_steps_and_exact_zeros(name):
    lay, Gj = fc.layout(name), fc.system(name)[1]
    order = fc.CASES[name][1][0]
    _, jl, _ = fc.labels(name)
    for s in range(1 if name == "B7" else 4):
        Z = fc.trajectory(name, s)
        th = [Z[k, lay.dt_off] * np.linalg.norm(uc.g_of(lay, Z, k, fc.member_G0(name), Gj), 2) for k in range(lay.K)]
        want = [fc.STEPS[(k + s) % 4] for k in range(lay.K)]
        assert np.allclose(th, want, rtol=1e-12, atol=0) and all((Z[k, lay.dt_off] == 0.0) == (want[k] == 0.0) for k in range(lay.K))
        j = fc.truth_one(name, order, s)[1].astype(np.float64)
        zero = sorted(str(x) for x in np.unique(jl) if not np.any(j[jl == x]))
        assert zero == sorted("du@%d" % k for k in range(lay.K) if want[k] == 0.0), (name, s, zero)
        for k in range(lay.K):
            if want[k] == 0.0:
                assert np.array_equal(j[jl == "B+@%d" % k], -np.tile(np.eye(lay.n).reshape(-1), lay.C)) and np.any(j[jl == "dh@%d" % k])
    if name != "B7":  # consecutive seeds, and a group's consecutive visits under 15 groups of B5, meet other steps
        assert {fc.step_class(2, s) for s in range(4)} == {0, 1, 2, 3} and fc.step_class(2, 0) != fc.step_class(2, 3)


@pytest.mark.parametrize("name,order", CASE_ORDERS)
def test_neighbouring_order_is_seen(name, order):
    """shape_cases.assert_sensitive at 1e4 x the tolerance, for delta and for the Jacobian values of every interval with a step."""
    lay = fc.layout(name)
    least = 1.0
    for s in range(1 if name == "B7" else 4):
        a, b = fc.truth_one(name, order, s), fc.truth_one(name, lower_order(order), s)
        for i in (0, 1):
            x, y = a[i].reshape(lay.K, -1), b[i].reshape(lay.K, -1)
            for k in range(lay.K):
                if fc.STEPS[fc.step_class(k, s)] != 0.0:
                    least = min(least, assert_sensitive(x[k], y[k], fc.TOL))
    print("%s, order %d: the neighbouring order moves every interval with a step by at least %.1e" % (name, order, least))


# ---- the payload's truth --------------------------------------------------------------------------------------------------------------------------------
def test_payload_truth_is_well_conditioned():
    """The payload formed in float64 from the rounded truth agrees with the longdouble one to 1e-13 per segment: no entry of it near-cancels, the GPU
    comparison at 1e-11 per segment has a factor 100 for the kernel's summation order; the entries of the h = 0 interval on u are exact zeros."""
    order = 4
    rows = [fc.truth_one("B7", order, member=i) for i in range(3)]
    pay = fc.payload_ld("B7", [r[0] for r in rows], [r[1] for r in rows])
    lab = fc.payload_labels("B7")
    lay = fc.layout("B7")
    assert pay.size == lab.size == 1 + lay.K * lay.m + lay.K
    lay1 = po.Layout(d=lay.d, m=lay.m, N=lay.N, z_dim=lay.z_dim, x_off=0, u_off=lay.u_off, dt_off=lay.dt_off)
    f64 = np.zeros(pay.size)
    for i in range(3):
        dl = po.pade_residual(fc.trajectory("B7"), lay1, fc.member_G0("B7", i), fc.system("B7")[1], order, fc.x_offs("B7")[i]).reshape(lay.K, lay.C, lay.n)
        tail = po.pade_jacobian_values(fc.trajectory("B7"), lay1, fc.member_G0("B7", i), fc.system("B7")[1], order, fc.x_offs("B7")[i])
        tail = tail.reshape(lay.K, -1)[:, 2 * lay.C * lay.n * lay.n :].reshape(lay.K, lay.C, lay.m + 1, lay.n)
        g = np.einsum("kcli,kci->kl", tail, dl)
        f64 += np.concatenate([[0.5 * np.sum(dl * dl)], g[:, : lay.m].reshape(-1), g[:, lay.m]])
    e = check_segments(f64, pay.astype(np.float64), lab, 1e-13)
    print("payload, float64 oracle against the truth: %.1e (%s)" % (max(e.values()), max(e, key=e.get)))
    zero = [k for k in range(lay.K) if fc.STEPS[fc.step_class(k, 0)] == 0.0]
    assert zero == [2] and not np.any(pay[lab == "gu@2"]) and np.all(pay[lab != "gu@2"] != 0)


# ---- faults, on the truth alone ---------------------------------------------------------------------------------------------------------------------------
def test_b1_stale_ring_slot_is_seen():
    """One group of all workgroups: visit v is interval v.  Every visit from 128 on, formed with the controls and the step the ring held before its refill
    (visit v - 128), moves a segment of its interval by SEEN or more."""
    n_cu, order = 256, 10
    B = fc.seeds("B1", n_cu)
    lay = fc.layout("B1")
    _, _, js, _, _ = fc.batch_truth("B1", order, B)
    js = js.reshape(B * lay.K, -1)
    lab = fc.labels("B1")[1][: js.shape[1]]
    n_vis = fc.group_visits(B * lay.K, n_cu, n_cu)[0]
    assert n_vis == 260 and fc.UHR_SLOTS == 128
    least = 1.0
    for v in range(fc.UHR_SLOTS, n_vis):
        assert fc.ring_slot(v) == fc.ring_slot(v - fc.UHR_SLOTS)
        least = min(least, uc.seen(js[v], fc.stale_ring_visit("B1", order, v), lab))
    print("B1: a stale ring slot moves a segment by at least %.1e" % least)
    assert least >= fc.SEEN


@pytest.mark.parametrize("name,order", [("B3", 6), ("B5", 4)])
def test_slice_from_the_groups_next_interval_is_seen(name, order):
    """A slice stored from the tiles of the group's NEXT visit (interval + groups): the -B+ or the B- block of the slice's columns moves by SEEN or more of
    the block's size, for every slice width the GPU module sets, under 16 and 8 workgroups per group -- except where both intervals have h = 0 (both are
    -I, I: nothing to see; the steps rotate with the seed, so that is at most the pairs of one step class in four: counted)."""
    n_cu = 256
    B, lay = fc.seeds(name, n_cu), fc.layout(name)
    d, m = fc.dims(name)
    n_int = B * lay.K
    js = fc.batch_truth(name, order, B)[2].reshape(n_int, -1)
    nn = lay.n * lay.n
    step = lambda iv: fc.STEPS[fc.step_class(iv % lay.K, iv // lay.K)]
    least, pairs, blind = 1.0, 0, 0
    for G in (16, 8):
        groups = L(d, m, order // 2, n_int, n_cu, v4_ticket=1, v4_group=G)["groups"]
        assert 1 <= groups < n_int
        for cols in fc.TICKET_COLS[name]:
            cpi = fc.tick_cpi(d, cols)
            for iv in range(n_int - groups):
                pairs += 1
                if step(iv) == 0.0 and step(iv + groups) == 0.0:
                    blind += 1
                    continue
                for c0 in range(0, d, cpi):
                    nce = min(cpi, d - c0)
                    bad = fc.swapped_slice(js, name, iv, iv + groups, c0, nce)
                    for blk in (0, lay.C * nn):
                        sel = slice(blk + c0 * nn, blk + (c0 + nce) * nn)
                        least = min(least, np.abs(bad[sel] - js[iv][sel]).max() / np.abs(js[iv][sel]).max())
    print("%s: a slice from the group's next interval moves its block by at least %.1e (%d pairs of visits, %d of them both h = 0)" % (name, least, pairs, blind))
    assert least >= fc.SEEN and 4 * blind <= pairs
