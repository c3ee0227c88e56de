"""The variational integrators at generator dimensions 66 .. 128 (PCL_BATCH_VARIATIONAL | PCL_LARGE_N | PCL_LARGE_VAR), without a GPU: the plan
of pcl_host_variational.hpp restated (tests/var_large_cases.py) against its table and its budgets, the value order against the lifted structure,
the float64 lifted oracle against the longdouble truth, the faults every case must see, what pcl_create decides before it touches a device,
and the mirror's keywords.

Without the feature these fail: test_constants_and_header and test_flag_table_without_a_device (AttributeError: the binding has no
PCL_LARGE_VAR), test_valid_descriptors_get_as_far_as_the_device and test_mirror_keywords (TypeError: the variational constructors and
_PclContext do not know large_generator / large_variational), test_mirror_never_sets_the_flags_by_itself (no such parameter)."""
import inspect

import numpy as np
import pytest

import piccolo_jl_amd as pa
import var_large_cases as vl
import variational_shape_cases as vsc
import variational_truth as vt
from oracle import pade_oracle as po

FLOOR = 1e-13  # the float64 lifted oracle against the truth, per segment (the floor tests/test_variational_sweep_cpu.py asserts)
SEEN = 1e-7  # what every fault must move some segment by


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------------------
def _intervals(name):
    return vl.knot(name)[0] - 1


@pytest.mark.parametrize("name", vl.NAMES)
def test_plan_table(name):
    n, C, v, m = vl.shape(name)
    P = vl.var_large_plan(n, C, m, v, items=_intervals(name))
    assert (P["sx"], P["nc"], P["ngrp"], P["mg"], P["pu"], P["npc"], P["U"], P["bytes"]) == vl.TABLE[name], (name, P)
    splits = [dict(), dict(jac=False), dict(cols_per_slice=1), dict(cols_per_slice=2), dict(cols_per_slice=C), dict(slices=1), dict(slices=n),
              dict(slices=10**6), dict(drives=1), dict(drives=5), dict(drives=max(m, 1)), dict(items=99), dict(items=99, n_cu=304)]  # fmt: skip
    for kw in splits:
        Q = vl.var_large_plan(n, C, m, v, **dict(dict(items=_intervals(name)), **kw))
        jac = kw.get("jac", True)
        assert Q["bytes"] <= vl.LDS_BYTES and Q["chain_blocks"] <= Q["NB"] and Q["panel_blocks"] <= Q["NB"], (name, kw, Q)
        assert Q["threads"] == 64 * -(-n // 16) <= 512 and Q["LD"] == n | 1, (name, kw, Q)
        assert Q["sx"] * Q["nc"] >= C > (Q["sx"] - 1) * Q["nc"] and Q["ngrp"] * Q["mg"] >= (m if jac else 0), (name, kw, Q)
        assert Q["chain_blocks"] == (1 + v) * Q["nc"] * ((2 + 2 * (2 + Q["mg"])) if jac else 4), (name, kw, Q)
        if jac:
            assert Q["pu"] * Q["npc"] >= n > (Q["pu"] - 1) * Q["npc"] and 1 <= Q["pairs"] <= vl.NP_PAIRS, (name, kw, Q)
            assert Q["U"] == Q["sx"] * Q["ngrp"] + (1 + v) * Q["pu"], (name, kw, Q)
        else:
            assert Q["pu"] == Q["npc"] == Q["mg"] == 0 and Q["U"] == Q["sx"], (name, kw, Q)
        if kw.get("cols_per_slice"):
            assert Q["nc"] <= kw["cols_per_slice"], (name, kw, Q)
        if kw.get("drives") and m:
            assert Q["mg"] <= kw["drives"], (name, kw, Q)
        if kw.get("slices"):
            assert Q["pu"] >= min(kw["slices"], n) or Q["npc"] == 1, (name, kw, Q)


def test_nothing_is_refused_up_to_the_abis_limits():
    """n <= 128, m <= 24, v <= 2, one or d state columns, any option: the chain unit of one column and one drive always fits."""
    for n in range(66, 130, 2):
        for v in (1, 2):
            for m in (0, 1, 24):
                for C in (1, n // 2):
                    for kw in (dict(), dict(jac=False), dict(drives=1), dict(cols_per_slice=1), dict(items=1), dict(items=1000)):
                        Q = vl.var_large_plan(n, C, m, v, **kw)
                        assert Q["bytes"] <= vl.LDS_BYTES and Q["chain_blocks"] <= Q["NB"] and Q["pairs"] <= vl.NP_PAIRS, (n, v, m, C, kw, Q)
    Q = vl.var_large_plan(128, 1, 1, 2)  # the tightest: 24 of 29 blocks, so the panel is not beside the chain
    assert (Q["NB"], Q["chain_blocks"], Q["nc"], Q["mg"], Q["npc"]) == (29, 24, 1, 1, 9)
    # the largest value count per interval: n = 128, C = 64, v = 2
    cs = vl.case_vl7()
    assert vl.values_per_interval(cs) == 10 * 64 * 128 * 128 + 3 * 128 * 64 * 2 == 10534912


def test_plan_sits_on_both_sides_of_its_splits():
    P = {name: vl.var_large_plan(*_shape_args(name), items=_intervals(name)) for name in vl.NAMES}
    assert P["VL5"]["ngrp"] == 3 and P["VL4"]["ngrp"] == 1 and P["VL6"]["mg"] == 0  # drive groups
    assert P["VL2"]["sx"] == 17 and P["VL3"]["sx"] == 24 and P["VL1"]["sx"] == 1  # column slices
    assert vl.var_large_plan(*_shape_args("VL2"), items=99)["sx"] == 6  # a long launch: the widest slices that take all drives (6 columns: 3 x 6 x 12 = 216 of 237 blocks)
    assert vl.var_large_plan(*_shape_args("VL5"), drives=1)["ngrp"] == 24 and vl.var_large_plan(*_shape_args("VL5"), drives=5)["ngrp"] == 5


def _shape_args(name):
    n, C, v, m = vl.shape(name)
    return n, C, m, v


# ---- the value order, the oracle's floor and the faults ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", vl.NAMES)
def test_value_order_is_the_lifted_structure(name):
    """lib_structure restates the header; value_index maps it into the lifted problem's values: position by position the two must name the same
    (row, variable), through variational_truth's maps of the oracle's structure."""
    cs, _ = vl.case(name)
    lay = vt.lifted(cs)[1]
    rows, cols = po.jac_structure(lay)
    rm, cm = vt._row_map(cs), vt._col_map(cs, lay)
    jr, jc = (rows // cs.xd) * cs.xd + rm[rows % cs.xd], cm[cols]
    perl = len(rows) // cs.K
    idx = (np.arange(cs.K)[:, None] * perl + vl.value_index(cs)[None]).reshape(-1)
    r, c = vl.lib_structure(cs)
    assert len(r) == cs.K * vl.values_per_interval(cs) and len(np.unique(idx)) == len(idx)
    assert np.array_equal(r, jr[idx]) and np.array_equal(c, jc[idx])
    assert len(np.unique(r * (cs.N * cs.z_dim) + c)) == len(r)  # every position once


@pytest.mark.parametrize("name", vl.NAMES)
def test_long_step_is_the_smallest_that_shows_the_top_term(name):
    """var_large_cases.LONG restates what the search of the variational sweep finds: the first candidate at which c_5 moves the order-10 residual by
    1e-7 of its size, every shorter one below that."""
    found, seen = vl.long_step_search(name)
    print("%s: %s" % (name, ", ".join("%.2f: %.1e" % kv for kv in seen.items())))
    assert found == vl.LONG[name] == vl.case(name)[1] and all(w < SEEN for s, w in seen.items() if s < found), (name, found, seen)
    assert abs(vl.vsc._lifted_norm(vl.case(name)[0], 2) * vl.case(name)[0].Z[2, vl.case(name)[0].dt_off] - found) < 1e-12


@pytest.mark.parametrize("name", vl.NAMES)
def test_float64_oracle_meets_the_truth_at_the_floor(name):
    cs, long_step = vl.case(name)
    Zl, lay, G0l, Gjl = vt.lifted(cs)
    dc, jc = vl.codes(name)
    vi = vl.value_index(cs)
    worst = [0.0, 0.0]
    for order in vl.ORDERS:
        d, j = vl.truth_ld(name, order)
        od = vt.residual(cs, order)
        oj = po.pade_jacobian_values(Zl, lay, G0l, Gjl, order).reshape(cs.K, -1)[:, vi].reshape(-1)
        wd = vsc.assert_segments(vsc.segment_errors(dc, od, d), FLOOR, lambda s: vsc.residual_name(cs, s), "%s order %d residual" % (name, order))
        wj = vsc.assert_segments(vsc.segment_errors(jc, oj, j), FLOOR, lambda s: vsc.jac_name(cs, s), "%s order %d Jacobian" % (name, order))
        worst = [max(worst[0], wd[0]), max(worst[1], wj[0])]
    print("%s (long step %.2f): float64 lifted oracle against the truth: residual %.1e, Jacobian %.1e" % (name, long_step, worst[0], worst[1]))


@pytest.mark.parametrize("name", vl.NAMES)
def test_every_case_sees_the_faults(name):
    """The truth alone: a zeroed c_q (orders 4 and 10, on the long step), and at order 10 an ignored last drive, an ignored last state column, a
    zeroed Gv_v and the Gv term restricted to k < 64 (on the first interval) each move a segment by 1e-7 of its size or more."""
    cs, _ = vl.case(name)
    dc, jc = vl.codes(name)

    def moved(order, k, **kw):
        d, j = vl.truth_ld(name, order)
        bd, bj, _ = vl.lifted_values(name, order, intervals=(k,), **kw)
        pick = lambda a: a.reshape(cs.K, -1)[k]
        return max(vsc.moved(pick(dc), pick(d), bd), vsc.moved(pick(jc), pick(j), bj.reshape(-1)))

    for order in (4, 10):
        c = vl.vs.coeffs(order)
        c[-1] = 0
        s = moved(order, 2, c=c)
        print("%s order %d, c_q zeroed: moved by %.1e" % (name, order, s))
        assert s >= SEEN, (name, order, s)
    faults = {"last state column": dict(drop_col=True), "Gv_v zeroed": dict(zero_last_variation=True), "Gv restricted to k < 64": dict(gv_k_below=64)}
    if cs.m:
        faults["last drive"] = dict(drop_drive=True)
    if cs.C == 1:
        del faults["last state column"]  # (a ket has one column: dropping it leaves nothing to compare)
    for what, kw in faults.items():
        s = moved(10, 0, **kw)
        print("%s, %s: moved by %.1e" % (name, what, s))
        assert s >= SEEN, (name, what, s)


def test_zero_step_segments_are_zero_in_the_truth():
    """VL2's interval of Delta t = 0: the L blocks and the d/du tails are identically zero (the GPU test asks for exact zeros there), the B blocks
    are -I | I and the d/dt tails are not zero."""
    cs, _ = vl.case("VL2")
    assert cs.Z[3, cs.dt_off] == 0.0
    d, j = vl.truth("VL2", 6)
    _, jc = vl.codes("VL2")
    seg = vsc.segment_max(jc, j)
    names = {vsc.jac_name(cs, s): mx for s, mx in seg.items()}
    for b in (1, 2):
        assert names["r%d.X0@0#3" % b] == 0.0 and names["r%d.X0@1#3" % b] == 0.0 and names["r%d.X0@0#2" % b] > 0.0
    for b in (0, 1, 2):
        assert names["r%d.u@0#3" % b] == 0.0 and names["r%d.h@0#3" % b] > 0.0 and names["r%d.X%d@0#3" % (b, b)] == 1.0


# ---- what pcl_create decides before it touches a device ----------------------------------------------------------------------------------------------
def _mk(d, large=True, large_var=True, mode=None, v=1, **over):
    L = pa._lib
    n = 2 * d
    kw = dict(d=d, m=1, N=3, z_dim=(1 + v) * n + 3, u_off=(1 + v) * n + 2, dt_off=(1 + v) * n, x_offs=[b * n for b in range(1 + v)], G0=np.zeros((1 + v, n, n)),
              Gj=np.zeros((1, n, n)), batch=1 + v, per_member_G0=True, state_cols=1, pade_order=8,
              batch_mode=(L.PCL_BATCH_VARIATIONAL if mode is None else mode) | (L.PCL_LARGE_N if large else 0) | (L.PCL_LARGE_VAR if large_var else 0))  # fmt: skip
    kw.update(over)
    return kw


def _refused(code, *words, **kw):
    with pytest.raises(pa.PclError) as ei:
        pa.integrators._PclContext(**kw)
    assert ei.value.code == code, str(ei.value)
    for w in words:
        assert w in str(ei.value), str(ei.value)


def test_constants_and_header():
    L = pa._lib
    text = open(L.INCLUDE + "/piccolo_hip.h").read()
    assert L.PCL_LARGE_VAR == 0x400 and "#define PCL_LARGE_VAR 0x400" in text
    assert L.PCL_LARGE_VAR & (L.PCL_LARGE_N | L.PCL_LARGE_EXP) == 0 and L.PCL_LARGE_VAR > L.PCL_BATCH_VARIATIONAL_EXP
    assert "#define PCL_MAX_D 32" in text and "#define PCL_LARGE_MAX_N 128" in text
    src = open(L.CSRC + "/pcl_kernel_variational.hpp").read()
    assert "#define PCL_VAR_MAXV 2 " in src
    large = open(L.CSRC + "/pcl_device_large.hpp").read()
    assert "#define PL_NP %d " % vl.NP_PAIRS in large and "#define PL_SLACK %d " % vl.SLACK in large


def test_flag_table_without_a_device():
    """Every row of the header's table that ends before the device (the flags go in through batch_mode, as a C caller sets them)."""
    pa.build_library()
    L = pa._lib
    single = dict(batch=1, per_member_G0=False, x_offs=[0], G0=np.zeros((66, 66)))
    _refused(L.PCL_EINVAL, "PCL_LARGE_VAR", "PCL_LARGE_N", **_mk(33, large=False))
    _refused(L.PCL_EINVAL, "PCL_LARGE_VAR", "PCL_LARGE_N", **_mk(8, large=False))
    for mode in (L.PCL_BATCH_MEMBERS, L.PCL_BATCH_TRAJ):
        _refused(L.PCL_EINVAL, "PCL_LARGE_VAR", "PCL_BATCH_VARIATIONAL", **_mk(33, mode=mode, **single))
    _refused(L.PCL_ENOTIMPL, "PCL_LARGE_VAR", "PCL_BATCH_VARIATIONAL_EXP", **_mk(33, mode=L.PCL_BATCH_VARIATIONAL_EXP, pade_order="exp"))
    _refused(L.PCL_ENOTIMPL, "PCL_LARGE_VAR", "PCL_BATCH_VARIATIONAL_EXP", **_mk(8, mode=L.PCL_BATCH_VARIATIONAL_EXP, pade_order="exp"))
    _refused(L.PCL_ENOTIMPL, "PCL_LARGE_VAR", "PCL_LARGE_EXP", **_mk(33, mode=L.PCL_BATCH_VARIATIONAL | L.PCL_LARGE_EXP))
    _refused(L.PCL_ENOTIMPL, "PCL_LARGE_VAR", "PCL_LARGE_EXP", **_mk(33, mode=L.PCL_BATCH_VARIATIONAL | L.PCL_LARGE_EXP, pade_order="exp"))
    # n > 128: the byte counts, as for PCL_LARGE_N
    _refused(L.PCL_ESHAPE, "generator dimension 130", "128", "163840", "132096", **_mk(65))
    _refused(L.PCL_ESHAPE, "generator dimension 130", "128", **_mk(65, v=2))
    # without the new flag: PCL_LARGE_N's refusal, in its words, with the new flag named behind them
    for mode, order in ((L.PCL_BATCH_VARIATIONAL, 8), (L.PCL_BATCH_VARIATIONAL_EXP, "exp")):
        for extra in (0, L.PCL_LARGE_EXP):
            _refused(L.PCL_ENOTIMPL, "PCL_LARGE_N is not implemented for the variational integrators (batch_mode PCL_BATCH_VARIATIONAL", "it goes with PCL_BATCH_MEMBERS or PCL_BATCH_TRAJ",
                     "PCL_LARGE_VAR", **_mk(33, large_var=False, mode=mode | extra, pade_order=order))  # fmt: skip
    # without any flag: as ever
    _refused(L.PCL_ESHAPE, "d=33 exceeds 32", **_mk(33, large=False, large_var=False))
    # the other checks of a variational descriptor come first, in their words
    _refused(L.PCL_ESHAPE, "3 variations", **_mk(33, v=3))
    _refused(L.PCL_ENOTIMPL, "pade_order=3", **_mk(33, pade_order=3))
    _refused(L.PCL_ESHAPE, "n_drives=25", **_mk(33, m=25, Gj=np.zeros((25, 66, 66)), z_dim=160, u_off=134))
    _refused(L.PCL_EINVAL, "PCL_STATE_VECTOR", **_mk(33, state_cols=L.PCL_STATE_VECTOR, G0=np.zeros((2, 33, 33)), Gj=np.zeros((1, 33, 33))))
    _refused(L.PCL_ENOTIMPL, "PCL_LARGE_VAR", "PCL_ORDER_EXP", **_mk(33, pade_order="exp"))  # (PCL_BATCH_VARIATIONAL with the exponential order)


def test_valid_descriptors_get_as_far_as_the_device():
    """The three flags on a valid descriptor: without a device PCL_EHIP "no CPU path", at 66 <= n <= 128 and at n <= 64, every order."""
    import torch

    pa.build_library()
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = pa._lib
    for order in (0, 2, 4, 6, 8, 10):
        _refused(L.PCL_EHIP, "no CPU path", **_mk(33, pade_order=order))
    _refused(L.PCL_EHIP, "no CPU path", **_mk(64, v=2))
    _refused(L.PCL_EHIP, "no CPU path", **_mk(27))  # the flags at n <= 64: the ordinary variational context's path
    unitary = dict(state_cols=33, z_dim=2 * 66 * 33 + 3, u_off=2 * 66 * 33 + 2, dt_off=2 * 66 * 33, x_offs=[0, 66 * 33])
    _refused(L.PCL_EHIP, "no CPU path", **_mk(33, **unitary))
    _refused(L.PCL_EHIP, "no CPU path", **_mk(33, m=24, Gj=np.zeros((24, 66, 66)), z_dim=160, u_off=134))
    # ... and by the keywords
    _refused(L.PCL_EHIP, "no CPU path", **dict(_mk(33, large=False, large_var=False), large_generator=True, large_variational=True))


# ---- the mirror ---------------------------------------------------------------------------------------------------------------------------------------
def test_mirror_keywords():
    """ValueErrors before any device call (a PclError would mean the library was reached)."""
    P, V = pa.integrators._PclContext, pa.integrators.HipVariationalIntegrator
    plain = _mk(33, large=False, large_var=False)
    with pytest.raises(ValueError, match="large_generator"):
        P(**dict(plain, large_variational=True))
    with pytest.raises(ValueError, match="exp"):
        P(**dict(plain, large_variational=True, large_generator=True, pade_order="exp"))
    with pytest.raises(ValueError, match="exp"):
        P(**dict(plain, large_variational=True, large_generator=True, batch_mode=pa._lib.PCL_BATCH_VARIATIONAL_EXP, pade_order="exp"))
    for mode in (pa._lib.PCL_BATCH_MEMBERS, pa._lib.PCL_BATCH_TRAJ):
        with pytest.raises(ValueError, match="variational"):
            P(**dict(plain, large_variational=True, large_generator=True, batch_mode=mode))
    # the public constructors: pade_order="exp" beside large_generator=True, and the other large keywords as ever
    with pytest.raises(ValueError, match="exp"):
        V(None, None, "x", ["v"], "u", [None], ket=True, large_generator=True, pade_order="exp")
    with pytest.raises(ValueError, match="exp"):
        V(None, None, "x", ["v"], "u", [None], ket=False, large_generator=True, pade_order=-1)
    for other in ("large_hessian", "large_full", "large_reduce", "large_exp", "large_exp_hessian", "large_exp_reduce"):
        for lg in (False, True):
            with pytest.raises(ValueError, match="variational"):
                V(None, None, "x", ["v"], "u", [None], ket=True, large_generator=lg, **{other: True})
    pa.integrators._check_services(pa._lib.PCL_BATCH_MEMBERS, "exp", large_variational=False, large_generator=False)  # off: nothing to check
    pa.integrators._check_services(pa._lib.PCL_BATCH_VARIATIONAL, 8, large_variational=True, large_generator=True)
    pa.integrators._check_services(pa._lib.PCL_BATCH_VARIATIONAL, 0, large_variational=True, large_generator=True)


def test_mirror_never_sets_the_flags_by_itself():
    for f, names in ((pa.integrators._PclContext.__init__, ("large_generator", "large_variational")), (pa.integrators.HipVariationalIntegrator.__init__, ("large_generator",))):
        sig = inspect.signature(f)
        for nm in names:
            assert sig.parameters[nm].default is False and sig.parameters[nm].kind is inspect.Parameter.KEYWORD_ONLY, (f, nm)
    src = inspect.getsource(pa.integrators)
    assert src.count("_lib.PCL_LARGE_VAR") == 1 and "_lib.PCL_LARGE_VAR if large_variational else 0" in src
    # the variational constructor passes ONE keyword on as both flags
    assert "large_generator=bool(large_generator), large_variational=bool(large_generator)" in src


def test_julia_glue_names_the_flag():
    text = open(pa._lib.CSRC + "/../julia/HipPadeIntegrator.jl").read()
    assert "const PCL_LARGE_VAR = 1024" in text and "large_generator ? PCL_LARGE_N | PCL_LARGE_VAR : 0" in text
