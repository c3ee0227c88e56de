"""The large variational kernels (contexts created with PCL_BATCH_VARIATIONAL | PCL_LARGE_N | PCL_LARGE_VAR) over the regimes of their launch
plans, at the cases of tests/var_large_plan_cases.py (the table and what each case enters are there), through the C ABI on device pointers into
NaN-filled arrays: pcl_eval_jac_dev (340 + q), pcl_eval_dev (350 + q), pcl_jac_dev, and under large_var_full pcl_rollout_dev (360).

Values: 1e-11 PER SEGMENT (row component x variable kind x relative knot x interval: the segments of var_large_cases.check), relative to the
segment's own maximum with no floor -- a segment that is identically zero must be exact zeros -- against the longdouble truth of the CLOSED
trajectory (the case's P knots and knot 0 again) rounded to float64; R6 (n = 128 unitary, v = 2) delta only.  The rollout: every knot and
component within 1e-11 of that knot's and component's largest entry in the longdouble truth, on trajectories of 29 and 44 intervals.
tests/test_var_large_plan_cpu.py holds the float64 oracle within 1e-13 (the rollout's restatement: 1e-12) of the same truths and shows that they see
the fault each case exists for.

Bit for bit: a long launch (the closed trajectory continued periodically) = the closed launch at interval k mod P, compared on the device -- delta and
the values of the fused launch, delta of the residual-only launch, fused delta = residual-only delta; every forced split (var_large_drives,
cols_per_slice, general_slices) = the automatic plan; component 0 = a plain PCL_LARGE_N context; the rollout's automatic panels = general_slices
n / 16 and n, its first four knots = a four-knot context, device = host pointers, launch = launch.

Before a long launch or a rollout is compared, the plan it takes is restated at the context's CU count and held to the regime the launch is there
for (vp.REGIME, vp.ROLLS): a box whose CU count puts the launch elsewhere FAILS there, with the plan in the message; where the count is 256, 304
or 128 the plan is also held to the committed tables.

ERR lines (pytest -s) carry the worst relative error per case and order; DESIGN.md 4.24.1 has what an MI355X gave.

69 tests; 50 s of wall time on an MI355X with the truths, the slowest (R5 at order 10: a truth of 21 million values, all compared on the host)
7.5 s; the truths are computed once per (case, order) and shared by every test of the case.
Without PCL_LARGE_VAR taking a count of kets between 1 and d, every test of R1, R2, R3 and R7 fails in pcl_create (PCL_EINVAL, state_cols)."""
import numpy as np
import pytest
import torch

import piccolo_jl_amd as pa
import var_large_cases as vl
import var_large_full_cases as vf
import var_large_plan_cases as vp

pytestmark = pytest.mark.gpu
TOL = vp.TOL
L = pa._lib
VAR, MEMBERS = L.PCL_BATCH_VARIATIONAL, L.PCL_BATCH_MEMBERS
NAN = float("nan")
CASE_ORDERS = [(name, order) for name in vp.NAMES for order in vp.ORDERS[name]]


def make_ctx(cs, order, **kw):
    c = pa.integrators._PclContext(**vp.context_args(cs, order, batch_mode=VAR, large_generator=True, large_variational=True, **kw))
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    assert c.x_dim == cs.xd and c.n_rows == cs.K * cs.xd and c.jac_per == vl.values_per_interval(cs) and c.jac_nnz == cs.K * c.jac_per
    return c


def plain_ctx(cs, order, **kw):
    """A plain PCL_LARGE_N context of the same drift and drives on component 0 of the same knots."""
    c = pa.integrators._PclContext(d=cs.n // 2, m=cs.m, N=cs.N, z_dim=cs.z_dim, u_off=cs.u_off, dt_off=cs.dt_off, x_offs=[cs.xo[0]], G0=cs.G0, Gj=cs.Gj,
                                   batch=1, batch_mode=MEMBERS, pade_order=order, state_cols=cs.C, large_generator=True, **kw)  # fmt: skip
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    return c


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float64).reshape(-1)).cuda()


def nans(k):
    return torch.full((k,), NAN, dtype=torch.float64, device="cuda")


def fused(c, Zd, q):
    dd, vd = nans(c.n_rows), nans(c.jac_nnz)
    c.eval_jac_dev(Zd, dd, vd)
    c.sync()
    assert c.get_option("last_kernel") == 340 + q
    assert not bool(torch.isnan(dd).any()) and not bool(torch.isnan(vd).any())
    return dd, vd


def residual(c, Zd, q):
    dd = nans(c.n_rows)
    c.eval_dev(Zd, dd)
    c.sync()
    assert c.get_option("last_kernel") == 350 + q and not bool(torch.isnan(dd).any())
    return dd


def jacobian(c, Zd):
    vd = nans(c.jac_nnz)
    c.jac_dev(Zd, vd)
    c.sync()
    return vd


def closed_launch(name, order, jac=True):
    """(delta, values | None) of the closed trajectory on the device, held to the truth."""
    cs = vp.case(name)
    c = make_ctx(cs, order)
    Zd = dev(cs.Z)
    if jac:
        dd, vd = fused(c, Zd, order // 2)
    else:
        dd, vd = residual(c, Zd, order // 2), None
    c.close()
    vp.check(name, order, dd.cpu().numpy(), None if vd is None else vd.cpu().numpy(), TOL, "the closed launch")
    return dd, vd


def periodic(long, short, K, P):
    """Interval k of the long array against interval k mod P of the short one, on the device."""
    idx = torch.arange(K, device=long.device) % P
    return torch.equal(long.view(K, -1), short.view(P, -1)[idx])


def held_plan(c, name, K):
    """The restated plans (Jacobian, residual only) of a launch of K intervals at the context's CU count, held to the regime of vp.REGIME and,
    at 256, 304 or 128 CUs, to the committed table."""
    n, C, v, m = vp.CASES[name]
    n_cu = c.get_option("n_cu")
    rows = [vp.plan_row(name, K, n_cu, jac) for jac in (True, False)]
    where = "%s at %d intervals on %d CUs: Jacobian %s slices %s groups %s | residual only %s slices %s" % (
        name, K, n_cu, rows[0][0], rows[0][1], rows[0][2], rows[1][0], rows[1][1])  # fmt: skip
    ncj, nce, crossed, uneven = vp.REGIME[(name, K)]
    for (row, sl, gr), jac in zip(rows, (True, False)):
        if jac and ncj is None:
            continue
        assert row[8] <= vp.LDS_BYTES and row[7] <= vp.NB[name] and sum(sl) == C and sum(gr) == (m if jac else 0), where
        assert row[1] == (ncj if jac else nce) and max(sl) == row[1], "outside the regime the launch is there for (nc %s): %s" % (ncj if jac else nce, where)
    if crossed:
        assert rows[0][0][0] > 1 and rows[0][0][3] > 1, "slices are not crossed with groups: " + where
    if uneven:
        assert rows[0][2][-1] < rows[0][2][0], "the groups are even: " + where
    if n_cu in vp.CUS:
        assert (rows[0][0], rows[1][0]) == vp.PLAN[(name, K, n_cu)], where
    print(where)
    return rows


def held_roll_plan(c, name, K):
    n_cu = c.get_option("n_cu")
    r = vp.roll_plan(name, K, n_cu)
    where = "%s rollout of %d intervals on %d CUs: panels %s, chain slices %s, %d B | %d B" % (name, K, n_cu, r["npce"], r["nce"], r["bytes_e"], r["bytes_c"])
    assert r["bytes_e"] <= vp.LDS_BYTES and r["bytes_c"] <= vp.LDS_BYTES, where
    assert max(r["npce"]) == vp.ROLLS[(name, K)][1] > 16, "outside the regime the rollout is there for (panels of %d columns): %s" % (vp.ROLLS[(name, K)][1], where)
    if n_cu in vp.CUS:
        assert vp.roll_row(name, K, n_cu) == vp.ROLL[(name, K, n_cu)], where
    print(where)
    return r


# ---- every case and order against the truth ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,order", CASE_ORDERS)
def test_values_per_segment(name, order):
    """The closed launch: pcl_eval_jac_dev, pcl_eval_dev and pcl_jac_dev against the truth per segment, and their bits against each other."""
    cs = vp.case(name)
    q = order // 2
    c = make_ctx(cs, order)
    assert c.get_option("large_variational") == 1 and c.get_option("variations") == cs.v
    Zd = dev(cs.Z)
    d2 = residual(c, Zd, q)
    if name in vp.RESIDUAL_ONLY:
        wd, wj = vp.check(name, order, d2.cpu().numpy(), None, TOL, "pcl_eval_dev")
        assert torch.equal(d2, residual(c, Zd, q)), "a second launch"
    else:
        dd, vd = fused(c, Zd, q)
        wd, wj = vp.check(name, order, dd.cpu().numpy(), vd.cpu().numpy(), TOL, "pcl_eval_jac_dev")
        vp.check(name, order, d2.cpu().numpy(), None, TOL, "pcl_eval_dev")
        assert torch.equal(d2, dd), "pcl_eval_dev alone"
        v2 = jacobian(c, Zd)
        vp.check(name, order, d2.cpu().numpy(), v2.cpu().numpy(), TOL, "pcl_jac_dev")
        assert torch.equal(v2, vd), "pcl_jac_dev alone"
        del v2
        d3, v3 = fused(c, Zd, q)
        assert torch.equal(d3, dd) and torch.equal(v3, vd), "a second launch"
    print("ERR %s order %d: residual %.1e (%s)  Jacobian %.1e (%s)" % (name, order, wd[0], wd[1], wj[0], wj[1]))
    c.close()


# ---- long launches ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,K", vp.LAUNCHES)
@pytest.mark.parametrize("order", [4, 10])
def test_long_launch_gives_the_bits_of_the_closed_launch(name, K, order):
    q, P = order // 2, vp.periods(name)
    with_jac = vp.REGIME[(name, K)][0] is not None
    ref_d, ref_v = closed_launch(name, order, jac=with_jac)
    cs = vp.long_case(name, K)
    c = make_ctx(cs, order)
    Zd = dev(cs.Z)
    held_plan(c, name, K)
    d_res = residual(c, Zd, q)
    assert periodic(d_res, ref_d, K, P), "delta of the residual-only launch"
    if with_jac:
        dd, vd = fused(c, Zd, q)
        assert periodic(dd, ref_d, K, P), "delta of the fused launch"
        assert periodic(vd, ref_v, K, P), "the Jacobian values of the fused launch"
        assert torch.equal(dd, d_res), "fused delta against residual-only delta"
        del vd
        d2, v2 = fused(c, Zd, q)
        assert torch.equal(d2, dd) and periodic(v2, ref_v, K, P), "a second launch"
    c.close()


# ---- forced splits ------------------------------------------------------------------------------------------------------------------------------------------
def _set(c, **kw):
    for key, val in kw.items():
        c.set_option(key, val)


@pytest.mark.parametrize("name", ["R2", "R3"])
@pytest.mark.parametrize("order", [4, 10])
def test_forced_groups_slices_and_panels_bitwise(name, order):
    """var_large_drives = 1, 3 and m crossed with cols_per_slice = 1 and 2 and general_slices = 1 and n: the automatic plan's bits."""
    cs = vp.case(name)
    n, C, v, m = vp.CASES[name]
    q = order // 2
    c = make_ctx(cs, order)
    Zd = dev(cs.Z)
    dd, vd = fused(c, Zd, q)
    vp.check(name, order, dd.cpu().numpy(), vd.cpu().numpy(), TOL)
    n_cu = c.get_option("n_cu")
    seen = set()
    for drives in (1, 3, m):
        for cols in (1, 2):
            for panels in (1, n):
                p = vp.plan(name, cs.K, n_cu, drives=drives, cols_per_slice=cols, slices=panels)
                assert p["bytes"] <= vp.LDS_BYTES and p["chain_blocks"] <= p["NB"] and p["mg"] <= drives and p["nc"] <= cols, (name, drives, cols, panels, p)
                seen.add((p["sx"], p["nc"], p["ngrp"], p["mg"], p["npc"]))
                _set(c, var_large_drives=drives, cols_per_slice=cols, general_slices=panels)
                d2, v2 = fused(c, Zd, q)
                assert torch.equal(d2, dd) and torch.equal(v2, vd), (name, drives, cols, panels)
                del v2
                assert torch.equal(residual(c, Zd, q), dd), ("pcl_eval_dev", name, drives, cols, panels)
    # the forced plans differ from each other (beside R3's tile only one column and one drive fit: the panels alone move)
    assert len(seen) >= (6 if name == "R2" else 2), seen
    _set(c, var_large_drives=0, cols_per_slice=0, general_slices=0)
    d2, v2 = fused(c, Zd, q)
    assert torch.equal(d2, dd) and torch.equal(v2, vd), "back to the automatic plan"
    c.close()


@pytest.mark.parametrize("name", ["R1", "R7"])
@pytest.mark.parametrize("order", [4, 10])
def test_forced_slices_of_the_88_interval_launch_bitwise(name, order):
    """cols_per_slice = 1, 2, 3 and C against the automatic plan's one or two wide slices."""
    K, q, P = 88, order // 2, vp.periods(name)
    n, C, v, m = vp.CASES[name]
    ref_d, ref_v = closed_launch(name, order)
    cs = vp.long_case(name, K)
    c = make_ctx(cs, order)
    Zd = dev(cs.Z)
    held_plan(c, name, K)
    dd, vd = fused(c, Zd, q)
    assert periodic(dd, ref_d, K, P) and periodic(vd, ref_v, K, P)
    n_cu = c.get_option("n_cu")
    for cols in (1, 2, 3, C):
        for jac in (True, False):
            p = vp.plan(name, K, n_cu, jac=jac, cols_per_slice=cols)
            assert p["nc"] <= cols and p["bytes"] <= vp.LDS_BYTES and p["chain_blocks"] <= p["NB"], (name, cols, jac, p)
        c.set_option("cols_per_slice", cols)
        d2, v2 = fused(c, Zd, q)
        assert torch.equal(d2, dd) and torch.equal(v2, vd), (name, "cols_per_slice", cols)
        del v2
        assert torch.equal(residual(c, Zd, q), dd), (name, "pcl_eval_dev, cols_per_slice", cols)
    c.close()


# ---- component 0 has the bits of a plain large context -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,K", [("R2", 4), ("R4", 10)])
@pytest.mark.parametrize("order", [4, 10])
def test_component_0_has_the_bits_of_a_plain_large_context(name, K, order):
    """delta_0, component 0's tails and the -B+ | B- copies of EVERY component against a PCL_LARGE_N context of the same drift and drives: R2's
    closed launch (slices crossed with uneven groups) and R4's 10-interval launch (the bench's plan)."""
    cs = vp.long_case(name, K)
    q = order // 2
    Zd = dev(cs.Z)
    c = make_ctx(cs, order)
    if (name, K) in vp.REGIME:
        held_plan(c, name, K)
    else:
        n_cu = c.get_option("n_cu")
        row, sl, gr = vp.plan_row(name, K, n_cu)
        assert row[0] > 1 and row[3] > 1 and gr[-1] < gr[0], "R2 outside its regime on %d CUs: %s %s %s" % (n_cu, row, sl, gr)
    dd, vd = fused(c, Zd, q)
    c.close()
    p = plain_ctx(cs, order)
    assert p.get_option("large_variational") == 0
    d0, v0 = nans(p.n_rows), nans(p.jac_nnz)
    p.eval_jac_dev(Zd, d0, v0)
    p.sync()
    assert p.get_option("last_kernel") == 290 + q
    p.close()
    dv, dp, jv, jp = vl.component0(cs)
    assert len(np.unique(dp)) == d0.numel() and len(np.unique(jp)) == v0.numel()
    d, v, d0, v0 = dd.cpu().numpy(), vd.cpu().numpy(), d0.cpu().numpy(), v0.cpu().numpy()
    assert not np.isnan(d0).any() and not np.isnan(v0).any()
    assert np.array_equal(d[dv], d0[dp]), "delta_0"
    assert np.array_equal(v[jv], v0[jp]), "the -B+ | B- copies and component 0's tails"


# ---- the rollout under large_var_full ------------------------------------------------------------------------------------------------------------------------
def rollout_dev(c, Zd):
    out = nans(c.N * c.x_dim)
    c.rollout_dev(Zd, out)
    c.sync()
    got = out.cpu().numpy()
    assert not np.isnan(got).any()
    return got


@pytest.mark.parametrize("name,K", list(vp.ROLLS))
def test_rollout_of_a_long_trajectory(name, K):
    cs, sp = vp.roll_case(name, K)
    n = cs.n
    c = make_ctx(cs, 8, large_var_full=True)
    assert c.get_option("large_var_full") == 1
    Zd = dev(cs.Z)
    held_roll_plan(c, name, K)
    got = rollout_dev(c, Zd)
    assert c.get_option("last_kernel") == 360
    e = vf.knot_errors(got, vp.rollout_truth(name, K), cs)
    k, b = np.unravel_index(int(e.argmax()), e.shape)
    print("ERR %s rollout of %d intervals: %.1e of the knot's and component's largest entry (knot %d, component %d)" % (name, K, e.max(), k, b))
    assert e.max() <= vf.TOL, (name, K, e)
    g = got.reshape(cs.N, cs.v + 1, cs.xdc)
    for b, o in enumerate(cs.xo):
        assert np.array_equal(g[0, b], cs.Z[0, o : o + cs.xdc]), "knot 0 is a copy"
    assert cs.Z[2, cs.dt_off] == 0.0 and np.array_equal(g[3], g[2]), "across the zero step: E = I and L_i = 0"
    assert np.array_equal(got, rollout_dev(c, Zd)), "a second launch"
    for panels in (-(-n // 16), n):
        c.set_option("general_slices", panels)
        assert np.array_equal(got, rollout_dev(c, Zd)), ("general_slices", panels)
    c.set_option("general_slices", 0)
    c.set_stream(None)
    assert np.array_equal(got, c.rollout(cs.Z.reshape(-1)).reshape(-1)), "pcl_rollout on host pointers"
    c.close()
    four = vp.first_knots(cs)
    c4 = make_ctx(four, 8, large_var_full=True)
    assert vp.roll_plan(name, 3, c4.get_option("n_cu"))["npc"] <= 16  # (one panel per 16 columns: the plan every earlier test takes)
    assert np.array_equal(rollout_dev(c4, dev(four.Z)).reshape(4, -1), got.reshape(cs.N, -1)[:4]), "knots 0 to 3 of a four-knot context"
    c4.close()
    p = plain_ctx(cs, 8, large_full=True)
    ref = rollout_dev(p, Zd).reshape(cs.N, cs.xdc)
    assert p.get_option("last_kernel") == 270 and np.array_equal(g[:, 0], ref), "component 0 against a plain large context"
    p.close()
