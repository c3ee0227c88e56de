"""The Hessian of the Lagrangian of the exponential constraint at generator dimensions 66 .. 128 without a device: the kernel's recurrence
(tests/large_exp_hess_cases.emulate_hess, float64 numpy) against scipy's expm / expm_frechet per segment, the faults the cases must see, the
per-drive identity that L4's truth takes its (u,u) block from, the launch plan, and the mirror's ValueErrors.

Without the feature the keyword tests fail with TypeError (an unexpected keyword argument)."""
import inspect

import numpy as np
import pytest

import exp_hess_truth as eht
import large_exp_cases as le
import large_exp_hess_cases as lh
import piccolo_jl_amd as pa
from shape_cases import check_segments

TOL = 1e-11  # the project's tolerance per segment, relative to the segment's own size
SEEN = 1e-7  # what a fault must move


def _rel(a, b, lab):
    """{segment: max|a - b| / max|b|}"""
    out = {}
    for s in np.unique(lab):
        sel = lab == s
        scale = np.abs(b[sel]).max()
        out[str(s)] = np.abs(a[sel] - b[sel]).max() / (scale if scale > 0 else 1.0)
    return out


# ---- the recurrence -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lh.NAMES + ["L1z"])
def test_emulation_meets_the_truth_per_segment(name):
    """Worst value read over the cases: 3.0e-13 (L2, (dt,dt) of the long step; 4.5e-14 elsewhere) -- DESIGN.md section 4.22."""
    lay, G0, Gj, Z = le.case(name)
    em = lh.emulate_hess(lay, G0, Gj, Z, lh.mu(name))
    er = check_segments(em, lh.truth(name), lh.labels(lay), TOL)
    print("%s: emulation against the truth %.1e (%s)" % (name, max(er.values()), max(er, key=er.get)))


def test_zero_step_of_the_emulation():
    """h = 0: segments 0 and 3 are exact zeros; 1 = -<M, G_l X>, 2 = -<G^T M, G X>, 4 = -G^T M."""
    lay, G0, Gj, Z = le.case("L1z")
    em = lh.emulate_hess(lay, G0, Gj, Z, lh.mu("L1z"))
    lab = lh.labels(lay)
    assert not em[lab == "seg0@1"].any() and not em[lab == "seg3@1"].any()
    G = G0 + np.tensordot(lay.u(Z, 1), Gj, axes=1)
    X, M = lay.X(Z, 1), lh.mu("L1z")[1].reshape(lay.C, lay.n).T
    assert np.array_equal(em[lab == "seg1@1"], np.array([-np.sum(M * (Gj[l] @ X)) for l in range(lay.m)]))
    assert np.array_equal(em[lab == "seg2@1"], np.array([-np.sum((G.T @ M) * (G @ X))]))
    assert np.array_equal(em[lab == "seg4@1"], (-(G.T @ M)).T.reshape(-1))


@pytest.mark.parametrize("name", ["L1", "L5", "L6", "L7"])
def test_every_fault_is_seen(name):
    lay, G0, Gj, Z = le.case(name)
    good = lh.emulate_hess(lay, G0, Gj, Z, lh.mu(name))
    lab = lh.labels(lay)
    for fault in ("drop_cross", "updated_dw", "drop_substep", "drop_col", "no_w_glx"):
        bad = lh.emulate_hess(lay, G0, Gj, Z, lh.mu(name), **{fault: True})
        moved = _rel(bad, good, lab)
        assert max(moved.values()) >= SEEN, (name, fault, max(moved.values()))


# ---- the identity behind L4's truth -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["L1", "L2"])
def test_per_drive_identity_meets_the_pairwise_truth(name):
    """(u_l,u_j) = -h <L2(A^T; M X^T, h G_l^T), G_j> against -<M, L2(A; h G_l, h G_j) X>, per segment at TOL."""
    lay, G0, Gj, Z = le.case(name)
    a = lh.values_per_drive(Z, lh.mu(name), lay, G0, Gj).reshape(-1)
    er = check_segments(a, lh.truth(name), lh.labels(lay), TOL)
    print("%s: per-drive identity against the pairwise truth %.1e" % (name, max(er.values())))


# ---- the plan -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lh.NAMES)
def test_plan_table(name):
    kind, n, cols, m = lh.CASES[name]
    P = lh.plan(n, cols, m)
    assert (P["U"], P["sx"], P["nc"], P["ngrp"], P["mg"], P["W"], P["NBW"], P["bytes"]) == lh.TABLE[name], (name, P)
    assert P["bytes"] <= lh.LDS_BYTES and P["W"] <= P["NBW"] and P["threads"] <= 512
    assert P["W"] == P["nc"] * lh.unit_columns(P["mg"], P["ngrp"] == 1) and P["U"] == P["sx"] * P["ngrp"] * (P["ngrp"] + 1) // 2


def test_plan_sits_on_both_sides_of_its_splits():
    P = lh.plan(120, 1, 24)  # fifteen columns: mg = 2 (9 off the diagonal); mg = 3 fits a diagonal unit (10) and not an off-diagonal one (16)
    assert P["NBW"] == 15 and P["mg"] == 2 and P["ngrp"] == 12 and P["U"] == 78 and P["W"] == 9
    assert lh.unit_columns(3, True) <= 15 < lh.unit_columns(3, False)
    P = lh.plan(128, 1, 24)  # nine columns: mg = 2 exactly
    assert P["NBW"] == 9 and P["mg"] == 2 and P["W"] == 9 and P["bytes"] <= lh.LDS_BYTES
    P = lh.plan(128, 1, 24, drives=1)
    assert P["W"] == 4 and P["U"] == 300
    P = lh.plan(128, 1, 3)  # one group of three would need 10 columns: two groups, sized off the diagonal
    assert (P["ngrp"], P["mg"], P["W"], P["U"]) == (2, 2, 9, 3)
    P = lh.plan(128, 1, 2, drives=1)  # L3 under large_exp_hess_drives = 1: the off-diagonal unit at n = 128
    assert (P["ngrp"], P["mg"], P["W"], P["U"]) == (2, 1, 4, 3)
    # one group is sized by its diagonal unit: a unitary state at n = 120 with four drives takes all four in one unit per column
    P = lh.plan(120, 60, 4)
    assert (P["sx"], P["nc"], P["ngrp"], P["mg"], P["W"], P["NBW"]) == (60, 1, 1, 4, 15, 16)
    # nothing is refused for m <= 24, n <= 128, 1 .. d columns
    for n in (66, 81, 96, 120, 127, 128):
        for m in (0, 1, 2, 3, 24):
            for cols in sorted({1, 2, n // 2} if n % 2 == 0 else {1}):
                for cps in (0, 1, 5):
                    for g in (0, 1, 3):
                        P = lh.plan(n, cols, m, cols_per_slice=cps, drives=g)
                        assert P["bytes"] <= lh.LDS_BYTES and P["W"] <= P["NBW"] and P["sx"] * P["nc"] >= cols and P["ngrp"] * P["mg"] >= m, (n, m, cols, cps, g, P)
                        assert P["W"] >= 2 * P["nc"] and (g == 0 or P["mg"] <= g) and (cps == 0 or P["nc"] <= cps)
    P = lh.plan(72, 5, 4, cols_per_slice=2)
    assert (P["sx"], P["nc"], P["mg"], P["ngrp"], P["U"]) == (3, 2, 4, 1, 3)
    P = lh.plan(72, 5, 4, cols_per_slice=5)
    assert (P["sx"], P["nc"], P["mg"], P["ngrp"], P["U"]) == (1, 5, 2, 2, 3)
    P = lh.plan(66, 33, 1, cols_per_slice=7)
    assert (P["sx"], P["nc"], P["U"]) == (5, 7, 5)


# ---- the mirror ---------------------------------------------------------------------------------------------------------------------------------------
def _kw(**over):
    n = 66
    kw = dict(d=33, m=1, N=3, z_dim=n + 3, u_off=n + 2, dt_off=n, x_offs=[0], G0=np.zeros((n, n)), Gj=np.zeros((1, n, n)), batch=1,
              batch_mode=pa._lib.PCL_BATCH_MEMBERS, state_cols=1, pade_order="exp")  # fmt: skip
    kw.update(over)
    return kw


def test_mirror_value_errors():
    """large_exp_hessian=True needs large_exp=True (and hence large_generator=True, pade_order="exp") on a plain context: a ValueError before any
    device call (a PclError would mean the library was reached)."""
    P = pa.integrators._PclContext
    with pytest.raises(ValueError, match="large_exp=True"):
        P(**_kw(large_exp_hessian=True))
    with pytest.raises(ValueError, match="large_exp=True"):
        P(**_kw(large_exp_hessian=True, large_generator=True))
    with pytest.raises(ValueError, match="large_generator"):
        P(**_kw(large_exp_hessian=True, large_exp=True))
    for order in (0, 4, 10):
        with pytest.raises(ValueError, match="pade_order"):
            P(**_kw(large_exp_hessian=True, large_exp=True, large_generator=True, pade_order=order))
    for mode in (pa._lib.PCL_BATCH_VARIATIONAL, pa._lib.PCL_BATCH_VARIATIONAL_EXP):
        with pytest.raises(ValueError, match="variational"):
            P(**_kw(large_exp_hessian=True, large_exp=True, large_generator=True, batch_mode=mode))
    # what stands beside large_exp=True keeps what it does today
    for other in ("large_hessian", "large_reduce"):
        with pytest.raises(ValueError, match="exp"):
            P(**_kw(large_exp_hessian=True, large_exp=True, large_generator=True, **{other: True}))


def test_integrator_constructors_take_the_keyword():
    """HipPadeIntegrator / BilinearIntegrator pass it on; the variational constructors refuse it."""
    for f in (pa.integrators._PclContext.__init__, pa.integrators.HipPadeIntegrator.__init__, pa.integrators.HipVariationalIntegrator.__init__):
        assert inspect.signature(f).parameters["large_exp_hessian"].default is False
    rng = np.random.default_rng(7)
    from vector_shape_cases import _herm

    s = pa.QuantumSystem(_herm(33, rng), [_herm(33, rng)], [1.0])
    psi = np.zeros(33, complex)
    psi[0] = 1
    t = pa.ket_trajectory(s, np.zeros((1, 4)), np.linspace(0, 0.1, 4), psi, psi)
    with pytest.raises(ValueError, match="large_exp=True"):
        pa.BilinearIntegrator(s, t, x_name=pa.trajectory.KET, pade_order="exp", large_generator=True, large_exp_hessian=True)
    with pytest.raises(ValueError, match="large_exp=True"):
        pa.BilinearIntegrator(s, t, x_name=pa.trajectory.KET, pade_order=8, large_exp_hessian=True)
    with pytest.raises(ValueError, match="variational"):
        pa.integrators.HipVariationalIntegrator(None, t, "x", ["y"], "u", [None], ket=True, pade_order="exp", large_exp_hessian=True, large_exp=True)
