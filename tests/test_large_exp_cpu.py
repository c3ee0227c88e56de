"""The exponential constraint at generator dimensions 66 .. 128 (PCL_LARGE_N | PCL_LARGE_EXP), without a GPU: the recurrence of
piccolo.jl_amd/csrc/pcl_kernel_large_exp.hpp emulated in float64 (tests/large_exp_cases.py) against scipy's expm / expm_frechet, the faults the
cases must see, the launch plan, what pcl_create decides before it touches a device, and the mirror's ValueErrors.

Without the feature the validation tests fail: the flag PCL_LARGE_EXP is an unknown batch mode."""
import numpy as np
import pytest

import large_exp_cases as le
import piccolo_jl_amd as pa
from shape_cases import check_segments

FLOOR = 1e-13  # the emulation against the truth, per segment (the floor the exponential sweep asserts)
SEEN = 1e-7  # what every fault must move some segment by


def worst(errs):
    s = max(errs, key=errs.get)
    return "%.1e (%s)" % (errs[s], s)


def seen(ref, bad, labels):
    """The largest relative move of a segment (a segment whose truth is zero counts by its absolute move)."""
    a, b, lab = np.asarray(bad), np.asarray(ref), np.asarray(labels).reshape(-1)
    out = 0.0
    for s in np.unique(lab):
        sel = lab == s
        scale = np.abs(b[sel]).max()
        err = np.abs(a[sel] - b[sel]).max()
        out = max(out, err / scale if scale > 0 else err)
    return out


# ---- the recurrence against the truth -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", le.NAMES + ["L1z"])
def test_emulation_meets_the_truth_per_segment(name):
    lay, G0, Gj, Z = le.case(name)
    d, j = le.emulate(lay, G0, Gj, Z)
    td, tj = le.truth(name)
    ed = check_segments(d, td, le.residual_labels(lay), FLOOR)
    ej = check_segments(j, tj, le.jac_labels(lay), FLOOR)
    print("%s: residual %s  Jacobian %s" % (name, worst(ed), worst(ej)))
    assert max(ed.values()) <= FLOOR and max(ej.values()) <= FLOOR, (name, ed, ej)


def test_steps_give_the_substep_counts_of_the_table():
    from vector_shape_cases import g_of

    for name in le.NAMES:
        lay, G0, Gj, Z = le.case(name)
        sp = [le.substeps(Z[k, lay.dt_off], g_of(lay, Z, k, G0, Gj)) for k in range(lay.K)]
        assert sp[:2] == [1, 3] and sp[2] == int(np.ceil(le.LONG[name])) and 20 < sp[2] <= 51, (name, sp)
        for k in range(lay.K):  # (no product near an integer: the device's norm may add in another order)
            x = abs(Z[k, lay.dt_off]) * le.norm1(g_of(lay, Z, k, G0, Gj))
            assert abs(x - round(x)) > 0.05, (name, k, x)
    lay, G0, Gj, Z = le.case("L1z")
    assert Z[1, lay.dt_off] == 0.0 and le.substeps(0.0, G0) == 0


def test_zero_step_of_the_emulation():
    """h = 0: E = I exactly, delta = X_{k+1} - X_k, zero drive tails, the dt tail -G X_k."""
    lay, G0, Gj, Z = le.case("L1z")
    n, m = lay.n, lay.m
    d, j = le.emulate(lay, G0, Gj, Z)
    per = lay.C * n * n + lay.x_dim * (m + 2)
    v = j[per : 2 * per]
    assert np.array_equal(v[: n * n], -np.eye(n).reshape(-1))
    assert np.array_equal(d[lay.x_dim : 2 * lay.x_dim], Z[2, : lay.x_dim] - Z[1, : lay.x_dim])
    tail = v[n * n + lay.x_dim :].reshape(m + 1, n)
    assert not tail[:m].any() and tail[m].any()


# ---- every case sees the faults ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", le.NAMES)
def test_every_case_sees_the_faults(name):
    kind, n, cols, m = le.CASES[name]
    lay, G0, Gj, Z = le.case(name)
    dl, jl = le.residual_labels(lay), le.jac_labels(lay)
    d, j = le.emulate(lay, G0, Gj, Z)
    faults = {"last substep": dict(drop_substep=True), "k beyond 64": dict(mm=le.mm_drop_k_beyond_64(n)), "last row tile": dict(mm=le.mm_zero_last_row_tile(n)),
              "last drive": dict(drop_drive=True), "last state column": dict(drop_col=True), "G_l V with the updated V": dict(updated_v=True)}  # fmt: skip
    for what, kw in faults.items():
        bd, bj = le.emulate(lay, G0, Gj, Z, **kw)
        sd, sj = seen(d, bd, dl), seen(j, bj, jl)
        print("%s, %s: residual moved by %.1e, Jacobian by %.1e" % (name, what, sd, sj))
        assert max(sd, sj) >= SEEN, (name, what, sd, sj)


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", le.NAMES)
def test_plan_table(name):
    kind, n, cols, m = le.CASES[name]
    P = le.plan(n, cols, m)
    assert (P["U"], P["sx"], P["nc"], P["ngrp"], P["mg"], P["npc"], P["bytes"]) == le.TABLE[name], (name, P)
    for kw in (dict(), dict(jac=False), dict(cols_per_slice=1), dict(cols_per_slice=2), dict(slices=n), dict(drives=1), dict(items=99)):
        Q = le.plan(n, cols, m, **kw)
        assert Q["bytes"] <= le.LDS_BYTES, (name, kw, Q)
        assert 3 * Q["W"] <= Q["NB"] and Q["sx"] * Q["nc"] >= cols and Q["ngrp"] * Q["mg"] >= (m if kw.get("jac", True) else 0), (name, kw, Q)
        if kw.get("jac", True):
            assert Q["U"] * Q["npc"] >= n and Q["U"] >= Q["sx"] * Q["ngrp"] and Q["npc"] >= 1, (name, kw, Q)
        else:
            assert Q["npc"] == 0 and Q["mg"] == 0 and Q["U"] == Q["sx"], (name, kw, Q)


def test_plan_sits_on_both_sides_of_its_splits():
    groups = {name: le.plan(*le.CASES[name][1:])["ngrp"] for name in le.NAMES}
    assert groups["L4"] == 8 and le.plan(*le.CASES["L4"][1:])["mg"] == 3 and groups["L9"] == 1  # the drive-group split
    P = le.plan(*le.CASES["L5"][1:], items=99)
    assert (P["ngrp"], P["mg"], P["U"]) == (1, 4, 2)  # ... and a long launch: one group of four drives
    slices = {name: le.plan(*le.CASES[name][1:])["sx"] for name in le.NAMES}
    assert slices["L6"] == 3 and slices["L5"] == 1  # the column-slice split
    P = le.plan(*le.CASES["L5"][1:], cols_per_slice=2)
    assert (P["sx"], P["nc"]) == (3, 2)
    assert le.plan(*le.CASES["L4"][1:], drives=1)["ngrp"] == 24 and le.plan(*le.CASES["L2"][1:], drives=1)["ngrp"] == 3


# ---- what pcl_create decides before it touches a device ----------------------------------------------------------------------------------------------
def _mk(d, large=True, large_exp=True, **over):
    n = 2 * d
    kw = dict(d=d, m=1, N=3, z_dim=n + 3, u_off=n + 2, dt_off=n, x_offs=[0], G0=np.zeros((n, n)), Gj=np.zeros((1, n, n)), batch=1,
              batch_mode=pa._lib.PCL_BATCH_MEMBERS | (pa._lib.PCL_LARGE_N if large else 0) | (pa._lib.PCL_LARGE_EXP if large_exp else 0),
              state_cols=1, pade_order="exp")  # fmt: skip
    kw.update(over)
    return kw


def _refused(code, *words, **kw):
    with pytest.raises(pa.PclError) as ei:
        pa.integrators._PclContext(**kw)
    assert ei.value.code == code, str(ei.value)
    for w in words:
        assert w in str(ei.value), str(ei.value)


def test_flag_validation_without_a_device():
    """Every row of the header's table that ends before the device (the flags go in through batch_mode, as a C caller sets them)."""
    pa.build_library()
    L = pa._lib
    assert L.PCL_LARGE_EXP == 0x200 and "#define PCL_LARGE_EXP 0x200" in open(L.INCLUDE + "/piccolo_hip.h").read()
    _refused(L.PCL_EINVAL, "PCL_LARGE_EXP", "PCL_LARGE_N", **_mk(33, large=False))
    _refused(L.PCL_EINVAL, "PCL_LARGE_EXP", "PCL_LARGE_N", **_mk(8, large=False))
    for order in (0, 2, 4, 10):
        _refused(L.PCL_EINVAL, "PCL_LARGE_EXP", "PCL_ORDER_EXP", **_mk(33, pade_order=order))
    var = dict(batch=2, per_member_G0=True, x_offs=[0, 0], G0=np.zeros((2, 66, 66)))
    flags = L.PCL_LARGE_N | L.PCL_LARGE_EXP
    _refused(L.PCL_ENOTIMPL, "PCL_LARGE_N", "PCL_BATCH_VARIATIONAL", **_mk(33, batch_mode=L.PCL_BATCH_VARIATIONAL | flags, **var))
    _refused(L.PCL_ENOTIMPL, "PCL_LARGE_N", "PCL_BATCH_VARIATIONAL_EXP", **_mk(33, batch_mode=L.PCL_BATCH_VARIATIONAL_EXP | flags, **var))
    # without the new flag: as before, in the same words, with a hint behind them
    _refused(L.PCL_ENOTIMPL, "PCL_LARGE_N is not implemented for the exponential constraint (pade_order = PCL_ORDER_EXP); it serves the diagonal Pade orders 2 .. 10",
             "PCL_LARGE_EXP", **_mk(33, large_exp=False))  # fmt: skip
    _refused(L.PCL_ENOTIMPL, "PCL_LARGE_N is not implemented for the exponential constraint", **_mk(8, large_exp=False))
    _refused(L.PCL_ESHAPE, "generator dimension 130", "128", "163840", **_mk(65))
    _refused(L.PCL_ESHAPE, "generator dimension 129", "128", **_mk(129, state_cols=L.PCL_STATE_VECTOR, G0=np.zeros((129, 129)), Gj=np.zeros((1, 129, 129))))


def test_valid_descriptors_get_as_far_as_the_device():
    """Both flags with PCL_ORDER_EXP: without a device PCL_EHIP "no CPU path", at 66 <= n <= 128 (even, or odd under PCL_STATE_VECTOR) and at n <= 64."""
    import torch

    pa.build_library()
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = pa._lib
    _refused(L.PCL_EHIP, "no CPU path", **_mk(33))
    _refused(L.PCL_EHIP, "no CPU path", **_mk(64, batch_mode=L.PCL_BATCH_TRAJ | L.PCL_LARGE_N | L.PCL_LARGE_EXP))
    _refused(L.PCL_EHIP, "no CPU path", **_mk(127, state_cols=L.PCL_STATE_VECTOR, G0=np.zeros((127, 127)), Gj=np.zeros((1, 127, 127)), z_dim=130, u_off=129, dt_off=127))
    _refused(L.PCL_EHIP, "no CPU path", **_mk(27))  # both flags at n <= 64: the ordinary exponential context's path
    _refused(L.PCL_EHIP, "no CPU path", **dict(_mk(33, batch_mode=L.PCL_BATCH_MEMBERS), large_generator=True, large_exp=True))  # ... and by the keywords


# ---- the mirror ---------------------------------------------------------------------------------------------------------------------------------------
def _kw(**over):
    kw = _mk(33, batch_mode=pa._lib.PCL_BATCH_MEMBERS)
    kw.update(over)
    return kw


def test_mirror_value_errors():
    """large_exp=True needs large_generator=True and pade_order="exp" on a plain context: a ValueError before any device call (a PclError would
    mean the library was reached).  large_full is allowed beside it; the other large options and the exponential ones are not."""
    P = pa.integrators._PclContext
    with pytest.raises(ValueError, match="large_generator"):
        P(**_kw(large_exp=True))
    for order in (0, 4, 10):
        with pytest.raises(ValueError, match="pade_order"):
            P(**_kw(large_exp=True, large_generator=True, pade_order=order))
    for mode in (pa._lib.PCL_BATCH_VARIATIONAL, pa._lib.PCL_BATCH_VARIATIONAL_EXP):
        with pytest.raises(ValueError, match="variational"):
            P(**_kw(large_exp=True, large_generator=True, batch_mode=mode))
    for other in ("large_hessian", "large_reduce"):
        with pytest.raises(ValueError, match="exp"):
            P(**_kw(large_exp=True, large_generator=True, **{other: True}))
    # every existing combination keeps its error: large_full on the exponential constraint WITHOUT the new keyword
    with pytest.raises(ValueError, match="has no large contexts"):
        P(**_kw(large_generator=True, large_full=True))
    with pytest.raises(ValueError, match="has no large contexts"):
        pa.integrators._check_services(pa._lib.PCL_BATCH_MEMBERS, "exp", large_full=True, large_generator=True)
    pa.integrators._check_services(pa._lib.PCL_BATCH_MEMBERS, "exp", large_full=True, large_generator=True, large_exp=True)  # ... and beside it: allowed
    pa.integrators._check_services(pade_order="exp", large_full=True, large_generator=True, large_exp=True)


def test_mirror_keyword_reaches_the_library():
    import torch

    pa.build_library()
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(pa.PclError) as ei:  # (large_full beside it passes the mirror's checks)
        pa.integrators._PclContext(**_kw(large_exp=True, large_generator=True, large_full=True))
    assert ei.value.code == pa._lib.PCL_EHIP and "no CPU path" in str(ei.value)


def test_integrator_constructors_take_the_keyword():
    """HipPadeIntegrator / BilinearIntegrator pass it on; the variational constructors refuse it."""
    import inspect

    for f in (pa.integrators._PclContext.__init__, pa.integrators.HipPadeIntegrator.__init__, pa.integrators.HipVariationalIntegrator.__init__):
        assert inspect.signature(f).parameters["large_exp"].default is False
    rng = np.random.default_rng(7)
    from vector_shape_cases import _herm

    s = pa.QuantumSystem(_herm(33, rng), [_herm(33, rng)], [1.0])
    psi = np.zeros(33, complex)
    psi[0] = 1
    t = pa.ket_trajectory(s, np.zeros((1, 4)), np.linspace(0, 0.1, 4), psi, psi)
    with pytest.raises(ValueError, match="large_generator"):
        pa.BilinearIntegrator(s, t, x_name=pa.trajectory.KET, pade_order="exp", large_exp=True)
    with pytest.raises(ValueError, match="pade_order"):
        pa.BilinearIntegrator(s, t, x_name=pa.trajectory.KET, pade_order=8, large_generator=True, large_exp=True)
