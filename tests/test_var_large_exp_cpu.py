"""The variational exponential constraint at generator dimensions 66 .. 128 (PCL_BATCH_VARIATIONAL_EXP | PCL_LARGE_N | PCL_LARGE_VAR |
PCL_LARGE_VAR_EXP, pade_order = PCL_ORDER_EXP), without a GPU: the plan of pcl_host_variational.hpp restated (tests/var_large_exp_cases.py) against
its table and its budgets, the kernel's recurrence emulated in float64 against scipy on the lifted generator, scipy's own floor against a
longdouble series, the mutants every case must see, the value order, what pcl_create decides before it touches a device, and the mirror's keyword.

Without the feature these fail: test_flag_value and test_descriptor_table (AttributeError: the binding has no PCL_LARGE_VAR_EXP),
test_valid_descriptors_get_as_far_as_the_device and test_mirror_keyword (TypeError: _PclContext and the variational constructors do not know
large_var_exp), test_julia_glue_names_the_flag."""
import inspect

import numpy as np
import pytest

import piccolo_jl_amd as pa
import var_exp_truth as vet
import var_large_cases as vl
import var_large_exp_cases as vx

# The float64 emulation of the kernel's recurrence against the scipy truth, per segment relative to the segment's own maximum.  Read on this
# suite's cases: VL1 1.4e-15, VL2 3.1e-15, VL3 6.6e-15, VL4 5.8e-15, VL5 2.7e-15, VL6 2.2e-15; the bound is ten times the worst reading and
# stays below 1e-12, so the GPU rule of 1e-11 keeps a decade.
EMU_BOUND = 7e-14
# scipy's expm / expm_frechet on the lifted generator against the longdouble series (VL1 1.4e-15, VL6 1.8e-15): at least a decade below 1e-11
SCIPY_FLOOR = 1e-12
SEEN = 1e-7  # what every mutant must move some segment by
# which cases see which mutant (every other pair is asserted to move NOTHING: a drift-only case has no drive terms)
MUTANTS = {
    "drop_gv_dv": ("VL1", "VL2", "VL3", "VL4", "VL5"), "drop_gl_vv": ("VL1", "VL2", "VL3", "VL4", "VL5"), "updated_v": vx.NAMES,
    "drop_substep": vx.NAMES, "drop_drive": ("VL1", "VL2", "VL3", "VL4", "VL5"), "dt_without_gv": vx.NAMES, "zero_last_row_tile": vx.NAMES,
}  # fmt: skip


def _worst(reads):
    return max((e / s for e, s in reads.values() if s > 0), default=0.0)


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------------------
def _check_plan(Q, n, C, m, v, jac, kw):
    comp = 1 + v
    assert Q["bytes"] <= vx.LDS_BYTES and 3 * Q["W"] <= Q["NB"], (kw, Q)
    assert Q["threads"] == 64 * -(-n // 16) <= 512 and Q["LD"] == n | 1, (kw, Q)
    assert Q["sx"] * Q["nc"] >= C > (Q["sx"] - 1) * Q["nc"] and Q["ngrp"] * Q["mg"] >= (m if jac else 0), (kw, Q)
    assert Q["chain_cols"] == comp * Q["nc"] * (1 + Q["mg"]) <= Q["W"] and Q["panel_cols"] <= Q["W"], (kw, Q)
    if jac:
        assert Q["pu"] * Q["npc"] >= n > (Q["pu"] - 1) * Q["npc"] and Q["panel_cols"] == comp * Q["npc"], (kw, Q)
        assert Q["U"] == Q["sx"] * Q["ngrp"] + Q["pu"], (kw, Q)
        assert Q["mg"] >= 1 or m == 0, (kw, Q)
    else:
        assert Q["pu"] == Q["npc"] == Q["mg"] == 0 and Q["U"] == Q["sx"], (kw, Q)


@pytest.mark.parametrize("name", vx.NAMES)
def test_plan_table(name):
    n, C, v, m = vl.shape(name)
    P = vx.var_large_exp_plan(n, C, m, v)
    assert (P["sx"], P["nc"], P["ngrp"], P["mg"], P["pu"], P["npc"], P["U"], P["W"], P["passes"], P["bytes"]) == vx.TABLE[name], (name, P)
    splits = [dict(), dict(jac=False), dict(cols_per_slice=1), dict(cols_per_slice=2), dict(cols_per_slice=C), dict(slices=1), dict(slices=n),
              dict(slices=10**6), dict(drives=1), dict(drives=2), dict(drives=max(m, 1))]  # fmt: skip
    for kw in splits:
        Q = vx.var_large_exp_plan(n, C, m, v, **kw)
        _check_plan(Q, n, C, m, v, kw.get("jac", True), (name, kw))
        if kw.get("cols_per_slice"):
            assert Q["nc"] <= kw["cols_per_slice"], (name, kw, Q)
        if kw.get("drives") and m:
            assert Q["mg"] <= kw["drives"], (name, kw, Q)
        if kw.get("slices"):
            assert Q["pu"] >= min(kw["slices"], n) or Q["npc"] == 1, (name, kw, Q)


def test_nothing_is_refused_up_to_the_abis_limits():
    """n <= 128, m <= 24, v <= 2, one or d state columns, any option: one column with one drive, and one panel column, always fit three buffers."""
    for n in range(66, 130, 2):
        for v in (1, 2):
            for m in (0, 1, 24):
                for C in (1, n // 2):
                    for kw in (dict(), dict(jac=False), dict(cols_per_slice=1), dict(slices=n), dict(drives=1), dict(drives=m)):
                        _check_plan(vx.var_large_exp_plan(n, C, m, v, **kw), n, C, m, v, kw.get("jac", True), (n, v, m, C, kw))
    P = vx.var_large_exp_plan(128, 64, 24, 2)  # the tightest: 29 blocks beside the tile, three buffers of 9 columns
    assert (P["NB"], P["NBW"], P["nc"], P["mg"], P["ngrp"], P["npc"], P["W"], P["bytes"]) == (29, 9, 1, 2, 12, 3, 9, 161240)


def test_plan_sits_on_both_sides_of_its_splits():
    # all drives in one unit | groups: VL5's 24 drives need four groups of six beside 15 columns per buffer; one column fewer per buffer would not
    P = vx.var_large_exp_plan(120, 1, 24, 1)
    assert (P["NBW"], P["mg"], P["ngrp"], P["chain_cols"]) == (15, 6, 4, 14)
    assert vx.var_large_exp_plan(96, 1, 4, 1)["ngrp"] == 1  # (the same system with room: one group)
    # one pass | two passes per chain unit: the fewest passes win, not the widest slice
    P = vx.var_large_exp_plan(96, 48, 4, 1)
    assert (P["nc"], P["mg"], P["chain_cols"]) == (3, 4, 30) and P["sx"] * P["ngrp"] * 2 == 32
    wide = 2 * 16 * 2  # sixteen columns of one drive: three slices x four groups x four passes
    assert 3 * 4 * -(-wide // 16) > 32
    # the panel: one 16-column pass where the buffer allows it (v = 1: 8 columns, v = 2: 5), the buffer's third at n = 128
    assert vx.var_large_exp_plan(66, 1, 2, 1)["npc"] == 8 and vx.var_large_exp_plan(72, 1, 0, 2)["npc"] == 5
    assert vx.var_large_exp_plan(128, 1, 1, 2)["npc"] == 3 and vx.var_large_exp_plan(128, 1, 1, 1)["npc"] == 4
    # general_slices on both sides of the auto count; cols_per_slice on both sides of the evened slice
    assert vx.var_large_exp_plan(66, 1, 2, 1, slices=9)["pu"] == 9 and vx.var_large_exp_plan(66, 1, 2, 1, slices=10)["pu"] == 10
    assert vx.var_large_exp_plan(66, 33, 3, 2, cols_per_slice=4)["nc"] == 4 and vx.var_large_exp_plan(66, 33, 3, 2, cols_per_slice=3)["nc"] == 3
    # the residual-only launch: value slots alone, no panel
    P = vx.var_large_exp_plan(128, 64, 24, 2, jac=False)
    assert (P["nc"], P["mg"], P["pu"], P["W"]) == (3, 0, 0, 9)


# ---- the value order --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", vx.NAMES)
def test_value_order_is_the_documented_structure(name):
    cs = vx.case(name)
    r, c = vet.structure(cs)
    per = vet.nnz_per_interval(cs)
    assert per == (1 + 2 * cs.v) * cs.C * cs.n**2 + cs.xd * (cs.m + 2) and r.size == c.size == cs.K * per
    key = r * (cs.N * cs.z_dim) + c
    assert np.unique(key).size == key.size  # no duplicates
    r1, c1 = vet.structure(cs, index_base=1)
    assert np.array_equal(r1, r + 1) and np.array_equal(c1, c + 1)
    assert r.min() == 0 and r.max() == cs.K * cs.xd - 1 and c.max() < cs.N * cs.z_dim
    # the -E copies of every component sit where component_vs_plain says a plain context has them
    dv, d0, jv, j0 = vx.component_vs_plain(cs)
    assert np.unique(d0).size == d0.size == cs.K * cs.xdc and np.unique(j0).size == cs.K * (cs.C * cs.n**2 + cs.xdc * (cs.m + 2))
    assert np.unique(jv).size == jv.size and np.all(c[jv] // cs.z_dim - r[jv] // cs.xd <= 1)


# ---- the recurrence, emulated -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", vx.NAMES)
def test_emulation_meets_the_truth(name):
    """A float64 numpy emulation of exactly the kernel's recurrence against scipy on the lifted generator, per segment.  Worst relative deviation
    read: 6.6e-15 (VL3, the Jacobian); asserted at ten times that, 7e-14, below the 1e-12 that leaves the GPU rule a decade."""
    cs = vx.case(name)
    assert [vx.substeps(cs, k) for k in range(3)][:2] == [1, 3] and vx.substeps(cs, 2) >= 20
    if cs.K == 4:
        assert vx.substeps(cs, 3) == 0
    d, j = vx.emulate(cs)
    wd, wj = vx.check(name, d, j, EMU_BOUND, "emulation")
    print("%s emulation: residual %.1e (%s)  Jacobian %.1e (%s)" % (name, wd[0], wd[1], wj[0], wj[1]))
    assert EMU_BOUND <= 1e-12


@pytest.mark.parametrize("name", ["VL1", "VL6"])
def test_scipy_meets_a_longdouble_series_at_its_floor(name):
    """The lifted generator is non-normal and the long step is long: scipy's own floor against an np.longdouble scaled Taylor series of the
    lifted matrix (read: VL1 7.2e-16 / 1.4e-15, VL6 1.0e-15 / 1.8e-15 for residual / Jacobian), and the emulation against that series."""
    ld = vx.truth_ld(name)
    t = vx.truth(name)
    ed, ej = vx.segment_reads(name, t[0], t[1], ref=ld)
    print("%s scipy floor: residual %.1e  Jacobian %.1e" % (name, _worst(ed), _worst(ej)))
    assert max(_worst(ed), _worst(ej)) <= SCIPY_FLOOR
    em = vx.emulate(vx.case(name))
    ed, ej = vx.segment_reads(name, em[0], em[1], ref=ld)
    print("%s emulation against the series: residual %.1e  Jacobian %.1e" % (name, _worst(ed), _worst(ej)))
    assert max(_worst(ed), _worst(ej)) <= EMU_BOUND


@pytest.mark.parametrize("name", vx.NAMES)
def test_every_case_sees_the_mutants(name):
    cs = vx.case(name)
    good = vx.emulate(cs)
    for fault, seen_by in MUTANTS.items():
        bad = vx.emulate(cs, mm=vx.mm_zero_last_row_tile(cs.n)) if fault == "zero_last_row_tile" else vx.emulate(cs, **{fault: True})
        mv = vx.moved(name, good, bad)
        if name in seen_by:
            assert mv >= SEEN, (name, fault, mv)
        else:
            assert mv == 0.0, (name, fault, mv)


def test_zero_step_in_the_truth_and_the_emulation():
    """VL2's interval of h = 0: -E = -I, L_i and the drive tails zeros, the dt tail -(Gv_i X + G Xv_i)."""
    cs = vx.case("VL2")
    n, C, v, m = cs.n, cs.C, cs.v, cs.m
    for vals in (vx.truth("VL2")[1], vx.emulate(cs)[1]):
        iv = vals.reshape(cs.K, -1)[3]
        blk = iv[: (1 + 2 * v) * C * n * n].reshape(1 + 2 * v, C, n * n)
        for b in range(1, v + 1):
            assert not blk[2 * b].any() and np.array_equal(blk[2 * b - 1], np.tile(-np.eye(n).reshape(-1), (C, 1)))
        assert np.array_equal(blk[0], np.tile(-np.eye(n).reshape(-1), (C, 1)))
        tails = iv[(1 + 2 * v) * C * n * n + cs.xd :].reshape(1 + v, C, m + 1, n)
        assert not tails[:, :, :m].any()
        G = vx.g_of(cs, 3)
        X = [cs.Z[3, o : o + cs.xdc].reshape(C, n) for o in cs.xo]
        for b in range(1 + v):
            want = -(X[b] @ G.T + (X[0] @ cs.Gv[b - 1].T if b else 0.0))
            assert np.abs(tails[b, :, m] - want).max() <= 1e-13 * np.abs(want).max()


# ---- what pcl_create decides before it touches a device ----------------------------------------------------------------------------------------------
def _mk(d, flags=None, mode=None, v=1, **over):
    L = pa._lib
    n = 2 * d
    flags = L.PCL_LARGE_N | L.PCL_LARGE_VAR | L.PCL_LARGE_VAR_EXP if flags is None else flags
    kw = dict(d=d, m=1, N=3, z_dim=(1 + v) * n + 3, u_off=(1 + v) * n + 2, dt_off=(1 + v) * n, x_offs=[b * n for b in range(1 + v)], G0=np.zeros((1 + v, n, n)),
              Gj=np.zeros((1, n, n)), batch=1 + v, per_member_G0=True, state_cols=1, pade_order="exp",
              batch_mode=(L.PCL_BATCH_VARIATIONAL_EXP if mode is None else mode) | flags)  # fmt: skip
    kw.update(over)
    return kw


def _refused(code, *words, **kw):
    with pytest.raises(pa.PclError) as ei:
        pa.integrators._PclContext(**kw)
    assert ei.value.code == code, str(ei.value)
    for w in words:
        assert w in str(ei.value), str(ei.value)


def test_flag_value():
    L = pa._lib
    text = open(L.INCLUDE + "/piccolo_hip.h").read()
    assert L.PCL_LARGE_VAR_EXP == 0x800 and "#define PCL_LARGE_VAR_EXP 0x800" in text
    assert L.PCL_LARGE_VAR_EXP & (L.PCL_LARGE_N | L.PCL_LARGE_EXP | L.PCL_LARGE_VAR) == 0
    assert L.PCL_LARGE_VAR_EXP > max(L.PCL_BATCH_MEMBERS, L.PCL_BATCH_TRAJ, L.PCL_BATCH_VARIATIONAL, L.PCL_BATCH_VARIATIONAL_EXP)
    src = open(L.CSRC + "/pcl_kernel_large_rollout.hpp").read()
    assert "#define LR_DEG %d" % vx.DEG in src and "#define LR_SMAX %d" % vx.SMAX in src


def test_descriptor_table():
    """Every combination with the new flag that ends before the device, and -- without it -- every refusal of today in its words."""
    pa.build_library()
    L = pa._lib
    N_, E_, V_, X_ = L.PCL_LARGE_N, L.PCL_LARGE_EXP, L.PCL_LARGE_VAR, L.PCL_LARGE_VAR_EXP
    single = dict(batch=1, per_member_G0=False, x_offs=[0], G0=np.zeros((66, 66)))
    for d in (33, 8):  # (decided from the flags alone, whatever the size)
        _refused(L.PCL_EINVAL, "PCL_LARGE_VAR_EXP goes with PCL_LARGE_N ", **_mk(d, flags=V_ | X_))
        _refused(L.PCL_EINVAL, "PCL_LARGE_VAR_EXP goes with PCL_LARGE_VAR ", **_mk(d, flags=N_ | X_))
        _refused(L.PCL_EINVAL, "PCL_LARGE_VAR_EXP goes with PCL_LARGE_N and PCL_LARGE_VAR ", **_mk(d, flags=X_))
    for mode, word in ((L.PCL_BATCH_MEMBERS, "PCL_BATCH_MEMBERS"), (L.PCL_BATCH_TRAJ, "PCL_BATCH_TRAJ")):
        _refused(L.PCL_EINVAL, "PCL_LARGE_VAR_EXP", "PCL_BATCH_VARIATIONAL_EXP, not " + word, **_mk(33, mode=mode, **single))
    _refused(L.PCL_EINVAL, "PCL_LARGE_VAR_EXP", "not PCL_BATCH_VARIATIONAL (", **_mk(33, mode=L.PCL_BATCH_VARIATIONAL))
    _refused(L.PCL_EINVAL, "PCL_LARGE_VAR_EXP", "not PCL_BATCH_VARIATIONAL (", **_mk(33, mode=L.PCL_BATCH_VARIATIONAL, pade_order=8))
    for order in (0, 2, 4, 10):
        _refused(L.PCL_EINVAL, "PCL_LARGE_VAR_EXP", "pade_order = PCL_ORDER_EXP, not a Pade order (got %d)" % order, **_mk(33, pade_order=order))
    _refused(L.PCL_EINVAL, "PCL_LARGE_VAR_EXP does not go with PCL_LARGE_EXP", "plain contexts", **_mk(33, flags=N_ | E_ | V_ | X_))
    # the checks of a variational descriptor, in their words; n > 128: the byte counts of the large kinds; n = 64: the ordinary context's PCL_ESHAPE
    _refused(L.PCL_ESHAPE, "generator dimension 130", "128", "163840", "132096", **_mk(65))
    _refused(L.PCL_ESHAPE, "generator dimension 130", "128", **_mk(65, v=2))
    _refused(L.PCL_ESHAPE, "3 variations", **_mk(33, v=3))
    _refused(L.PCL_ESHAPE, "n_drives=25", **_mk(33, m=25, Gj=np.zeros((25, 66, 66)), z_dim=160, u_off=134))
    _refused(L.PCL_EINVAL, "PCL_STATE_VECTOR", **_mk(33, state_cols=L.PCL_STATE_VECTOR, G0=np.zeros((2, 33, 33)), Gj=np.zeros((1, 33, 33))))
    # ---- without the new flag: exactly today's answers (tests/test_var_large_cpu.py, tests/test_large_exp_cpu.py pin the same words) ----
    VE, VA = L.PCL_BATCH_VARIATIONAL_EXP, L.PCL_BATCH_VARIATIONAL
    _refused(L.PCL_ENOTIMPL, "PCL_LARGE_VAR is not implemented for the exponential constraint (batch_mode PCL_BATCH_VARIATIONAL_EXP)", **_mk(33, flags=N_ | V_))
    _refused(L.PCL_ENOTIMPL, "PCL_LARGE_VAR is not implemented for the exponential constraint (batch_mode PCL_BATCH_VARIATIONAL_EXP)", **_mk(8, flags=N_ | V_))
    _refused(L.PCL_ENOTIMPL, "PCL_LARGE_VAR is not implemented for the exponential constraint (the flag PCL_LARGE_EXP)", **_mk(33, flags=N_ | V_ | E_, mode=VA))
    _refused(L.PCL_ENOTIMPL, "PCL_LARGE_VAR is not implemented for the exponential constraint (pade_order = PCL_ORDER_EXP)", **_mk(33, flags=N_ | V_, mode=VA))
    _refused(L.PCL_EINVAL, "PCL_LARGE_VAR goes with PCL_LARGE_N", **_mk(33, flags=V_))
    for mode in (L.PCL_BATCH_MEMBERS, L.PCL_BATCH_TRAJ):
        _refused(L.PCL_EINVAL, "PCL_LARGE_VAR is the variational integrators", "PCL_BATCH_VARIATIONAL", **_mk(33, flags=N_ | V_, mode=mode, pade_order=8, **single))
    for extra in (0, E_):
        _refused(L.PCL_ENOTIMPL, "PCL_LARGE_N is not implemented for the variational integrators (batch_mode PCL_BATCH_VARIATIONAL_EXP)", "PCL_LARGE_VAR",
                 **_mk(33, flags=N_ | extra))  # fmt: skip
    _refused(L.PCL_EINVAL, "PCL_LARGE_EXP goes with PCL_LARGE_N", **_mk(33, flags=E_, mode=L.PCL_BATCH_MEMBERS, **single))
    _refused(L.PCL_ESHAPE, "d=33 exceeds 32", **_mk(33, flags=0))


def test_valid_descriptors_get_as_far_as_the_device():
    """The four flags on a valid descriptor: without a device PCL_EHIP "no CPU path" -- validation has finished -- at 66 <= n <= 128 and n <= 64."""
    import torch

    pa.build_library()
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = pa._lib
    _refused(L.PCL_EHIP, "no CPU path", **_mk(33))
    _refused(L.PCL_EHIP, "no CPU path", **_mk(64, v=2))
    _refused(L.PCL_EHIP, "no CPU path", **_mk(27))  # the flags at n <= 64: the ordinary variational exponential context's path
    _refused(L.PCL_EHIP, "no CPU path", **_mk(32))  # (n = 64: its PCL_ESHAPE needs the device's LDS size)
    unitary = dict(state_cols=33, z_dim=2 * 66 * 33 + 3, u_off=2 * 66 * 33 + 2, dt_off=2 * 66 * 33, x_offs=[0, 66 * 33])
    _refused(L.PCL_EHIP, "no CPU path", **_mk(33, **unitary))
    kets = dict(state_cols=5, z_dim=2 * 66 * 5 + 3, u_off=2 * 66 * 5 + 2, dt_off=2 * 66 * 5, x_offs=[0, 66 * 5])
    _refused(L.PCL_EHIP, "no CPU path", **_mk(33, **kets))
    _refused(L.PCL_EHIP, "no CPU path", **_mk(33, m=24, Gj=np.zeros((24, 66, 66)), z_dim=160, u_off=134))
    # ... and by the keywords
    _refused(L.PCL_EHIP, "no CPU path", **dict(_mk(33, flags=0), large_generator=True, large_variational=True, large_var_exp=True))
    _refused(L.PCL_EHIP, "no CPU path", **dict(_mk(33, flags=0), large_generator=True, large_variational=True, large_var_exp=True, large_var_full=True))


# ---- the mirror ---------------------------------------------------------------------------------------------------------------------------------------
def test_mirror_keyword():
    """ValueErrors before any device call, each sentence (a PclError would mean the library was reached)."""
    L = pa._lib
    P, V, chk = pa.integrators._PclContext, pa.integrators.HipVariationalIntegrator, pa.integrators._check_services
    VE, VA = L.PCL_BATCH_VARIATIONAL_EXP, L.PCL_BATCH_VARIATIONAL
    on = dict(large_generator=True, large_variational=True, large_var_exp=True)
    chk(VE, "exp", **on)
    chk(VE, -1, **on)
    chk(VE, "exp", large_var_full=True, **on)
    chk(VE, "exp", large_generator=False, large_variational=False, large_var_exp=False)  # off: nothing to check
    for mode in (L.PCL_BATCH_MEMBERS, L.PCL_BATCH_TRAJ):
        with pytest.raises(ValueError, match="large_var_exp=True is the flag PCL_LARGE_VAR_EXP of a variational context .*: a plain context takes large_exp=True"):
            chk(mode, "exp", large_generator=True, large_var_exp=True)
    with pytest.raises(ValueError, match="large_var_exp=True is the exponential constraint of a variational context created with large_generator=True .*: it needs that keyword"):
        chk(VE, "exp", large_var_exp=True)
    for order in (0, 4, 10):
        with pytest.raises(ValueError, match=r"large_var_exp=True is the variational exponential constraint at generator dimensions 66 \.\. 128: it needs pade_order=\"exp\" \(got %d\)" % order):
            chk(VA, order, **on)
    for other in (dict(exp_hessian=True), dict(exp_hessian="workspace"), dict(var_compact=True), dict(large_var_hessian=True)):
        with pytest.raises(ValueError, match="large_var_exp=True serves residual and Jacobian, .*PCL_LARGE_VAR_EXP.*exp_hessian, var_compact and large_var_hessian stay off"):
            chk(VE, "exp", **dict(on, **other))
    # without the keyword: today's sentence
    with pytest.raises(ValueError, match="large_generator=True on a variational integrator serves the diagonal Pade orders 2 .. 10"):
        chk(VE, "exp", large_generator=True, large_variational=True)
    with pytest.raises(ValueError, match="large_var_full=True serves the diagonal Pade orders 2 .. 10"):
        chk(VE, "exp", large_generator=True, large_var_full=True)
    # the other large keywords beside it: the table's words
    for other in ("large_hessian", "large_full", "large_reduce", "large_exp", "large_exp_hessian", "large_exp_reduce"):
        with pytest.raises(ValueError, match="variational"):
            V(None, None, "x", ["v"], "u", [None], ket=True, large_generator=True, large_var_exp=True, pade_order="exp", **{other: True})
    # the constructors and the context
    with pytest.raises(ValueError, match="it needs that keyword"):
        V(None, None, "x", ["v"], "u", [None], ket=True, large_var_exp=True, pade_order="exp")
    with pytest.raises(ValueError, match="it needs pade_order"):
        V(None, None, "x", ["v"], "u", [None], ket=False, large_generator=True, large_var_exp=True, pade_order=4)
    with pytest.raises(ValueError, match="exp"):
        V(None, None, "x", ["v"], "u", [None], ket=True, large_generator=True, pade_order="exp")
    with pytest.raises(ValueError, match="plain context takes large_exp=True"):
        P(**dict(_mk(33, flags=0, mode=L.PCL_BATCH_MEMBERS), large_generator=True, large_var_exp=True))
    for f in (P.__init__, V.__init__):
        par = inspect.signature(f).parameters["large_var_exp"]
        assert par.default is False and par.kind is inspect.Parameter.KEYWORD_ONLY
    assert "large_var_exp" not in inspect.signature(pa.integrators.HipPadeIntegrator.__init__).parameters
    row = [r for r in pa.integrators._SERVICES if r.keyword == "large_var_exp"]
    assert len(row) == 1 and (row[0].flag, row[0].beside, row[0].constraint, row[0].family) == ("PCL_LARGE_VAR_EXP", "large_generator", "exp", "variational")
    assert list(row[0].refuse) == ["family", "beside", "constraint", "without"]


def test_julia_glue_names_the_flag():
    text = open(pa._lib.CSRC + "/../julia/HipPadeIntegrator.jl").read()
    assert "const PCL_LARGE_VAR_EXP = 2048" in text and "large_var_exp::Bool = false" in text
