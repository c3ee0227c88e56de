"""What tests/test_var_large_exp_hess_gpu.py stands on, without a GPU: the restated component-wise recurrence with its passes against the scipy
truth on the lifted generator per segment (the bound the GPU tolerance of 1e-11 keeps a decade above), the per-drive identity against the pairwise
truth, the decomposition into passes, what each case sees of the recurrence's faults, the plan of the launch per case and over the sizes (nothing
refused), the finite-difference yardstick of the device test, and the keyword."""
import inspect

import numpy as np
import pytest

import piccolo_jl_amd as pa
import var_large_exp_hess_cases as vc

L = pa._lib
FAULTS = ("drop_gv_d2w", "drop_gv_dw", "drop_cross", "updated_w", "drop_substep", "drop_pass", "seg1_without_gv", "drop_col")
DRIVE_FAULTS = ("drop_gv_d2w", "drop_gv_dw", "drop_cross")


@pytest.fixture(scope="module")
def emulated():
    """The emulation on the intervals that have a truth, once per case and process."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = vc.emulate_hess(vc.case(name), vc.rand_mu(name), ks=vc.intervals(name))
            cache[name].setflags(write=False)
        return cache[name]

    return get


# ---- the recurrence against the truth -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", vc.NAMES)
def test_emulation_against_the_truth(name, emulated):
    """Per segment of every interval that has a truth, relative to the segment's own maximum: what was read is vc.CPU_READ[name]; ten times the
    worst of them is the asserted CPU_BOUND, which stays below 1e-12."""
    errs = vc.segment_errors(name, emulated(name))
    w = vc.worst(errs)
    cs = vc.case(name)
    print("READ %s: %.1e (recorded %.1e), substeps %s" % (name, w, vc.CPU_READ[name], [vc.substeps(cs, k) for k in range(cs.K)]))
    assert 10 * max(vc.CPU_READ.values()) <= vc.CPU_BOUND <= 1e-12
    assert w <= vc.CPU_BOUND, (name, w)
    if name in ("VL1", "VL2", "VL3", "VL4", "VL5", "VL6"):
        assert vc.substeps(cs, 2) >= 20  # the long step
    # identically-zero segments are exact zeros in the emulation too
    for s, (e, scale) in errs.items():
        assert scale > 0 or e == 0.0, vc.segment_names(name)(s)


@pytest.mark.parametrize("name", ["VL1", "VL2"])
def test_per_drive_identity_against_the_pairwise_truth(name):
    """Segment 0 by (u_l,u_j) = -h <L2(Ahat^T; M' X'^T, h Ghat_l^T), Ghat_j> equals the pairwise second Frechet derivative, interval by interval."""
    cs = vc.case(name)
    ks = [0, 1] if name == "VL2" else list(range(cs.K))
    a = vc.truth_values(cs, vc.rand_mu(name), ks, per_drive=True)
    w = vc.worst(vc.segment_errors(name, a, vc.truth(name), ks))
    print("per-drive identity on %s: %.1e" % (name, w))
    assert w <= 1e-13


@pytest.mark.parametrize("name", ["VL1", "VL4", "VL6"])
def test_the_passes_add_up(name):
    """Pass 0 + .. + pass v = the lifted values, pass 0 knows no variation, and pass b alone is the Hessian under the multipliers of component b."""
    cs = vc.case(name)
    ks = [0, 1]
    parts = [vc.emulate_hess(cs, vc.rand_mu(name), passes=[b], ks=ks) for b in range(1 + cs.v)]
    assert vc.worst(vc.segment_errors(name, sum(parts), ks=ks)) <= vc.CPU_BOUND
    i0, ib, _ = vc.component_slices(cs)
    assert np.all(parts[0].reshape(-1)[ib] == 0.0)
    for b in range(1, 1 + cs.v):
        mu = np.zeros((cs.K, 1 + cs.v, cs.xdc))
        mu[:, b] = vc.rand_mu(name).reshape(cs.K, 1 + cs.v, cs.xdc)[:, b]
        alone = vc.truth_values(cs, mu.reshape(-1), ks)
        assert vc.worst(vc.segment_errors(name, parts[b], alone, ks)) <= vc.CPU_BOUND, (name, b)


# ---- faults ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["VL1", "VL2", "VL4", "VL6"])
def test_faults_are_seen(name, emulated):
    """Every fault of the recurrence moves some segment by 1e-7 of its size or more (interval 1: three substeps); on VL6 (m = 0) the drive faults
    move nothing."""
    cs = vc.case(name)
    ks = [1]
    good = emulated(name)
    seen = {}
    for fault in FAULTS:
        if fault == "drop_col" and cs.C == 1:
            continue
        seen[fault] = vc.moved(name, good, vc.emulate_hess(cs, vc.rand_mu(name), ks=ks, **{fault: True}), ks)
    print("SEEN %s: %s" % (name, "  ".join("%s %.1e" % kv for kv in seen.items())))
    for fault, x in seen.items():
        if cs.m == 0 and fault in DRIVE_FAULTS + ("seg1_without_gv",):
            assert x == 0.0, (name, fault, x)
        else:
            assert x >= vc.SEEN, (name, fault, x)


# ---- the plan -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", vc.NAMES)
def test_plan_table(name):
    n, C, v, m = vc.shape(name)
    p = vc.plan(n, C, m)
    assert (p["sx"], p["nc"], p["ngrp"], p["mg"], p["U"], p["W"], p["bytes"]) == vc.TABLE[name]
    assert p["bytes"] <= vc.LDS_BYTES and p["sx"] * p["nc"] >= C and p["ngrp"] * p["mg"] >= m and p["threads"] <= 512
    assert (p["sx"] - 1) * p["nc"] < C and (m == 0 or (p["ngrp"] - 1) * p["mg"] < m)  # no unit without work
    Tc = vc.unit_columns(p["mg"], p["ngrp"] == 1)
    assert p["W"] == 2 * p["nc"] * Tc and p["W"] >= 4 * p["nc"] and p["W"] <= p["NBW"]  # two components; [X' | Ghat X'] behind the chain fits


def test_both_sides_of_the_splits():
    """n = 128 leaves 9 columns per buffer: an off-diagonal two-component unit of one drive per group takes 8, two drives per group 18; a
    diagonal unit 6; all 1 + v = 3 components at once would take 12.  The knobs move the plan to the other side of each split."""
    assert vc.plan(128, 1, 24)["NBW"] == 9
    assert 2 * vc.unit_columns(1, False) == 8 and 2 * vc.unit_columns(1, True) == 6 and 3 * vc.unit_columns(1, False) == 12 and 2 * vc.unit_columns(2, False) == 18
    p = vc.plan(66, 33, 3)
    assert (p["ngrp"], p["mg"]) == (1, 3)
    p1, p2 = vc.plan(66, 33, 3, drives=1), vc.plan(66, 33, 3, drives=2)
    assert (p1["ngrp"], p1["mg"]) == (3, 1) and (p2["ngrp"], p2["mg"]) == (2, 2)
    assert p1["U"] == p1["sx"] * 6 and p2["U"] == p2["sx"] * 3
    for cap in (1, 2):
        pc = vc.plan(66, 33, 3, cols_per_slice=cap)
        assert pc["nc"] == cap and pc["sx"] == -(-33 // cap)
    assert vc.plan(120, 1, 24, drives=2)["mg"] == 1  # (two drives per group do not fit beside the n = 120 tile: 18 columns of 15)
    assert vc.plan(96, 48, 4, drives=2)["mg"] == 2 and vc.plan(96, 48, 4, drives=2)["ngrp"] == 2


def test_tightest_shape_fits():
    """n = 128 unitary, m = 24, v = 2: one column, one drive per group, 8 columns per buffer."""
    p = vc.plan(128, 64, 24)
    assert (p["sx"], p["nc"], p["ngrp"], p["mg"], p["W"]) == (64, 1, 24, 1, 8)
    assert p["bytes"] == (129 * 128 + 128 + 24 + 8 + 3 * 129 * 8) * 8 == 158144 <= 163840


def test_nothing_is_refused():
    """Every even n in 66 .. 128, m in {0, 1, 2, 24}, kets and unitaries, under every cap of the two knobs that the GPU tests use."""
    for n in range(66, 130, 2):
        for m in (0, 1, 2, 24):
            for C in (1, n // 2):
                for kw in ({}, dict(cols_per_slice=1), dict(cols_per_slice=2), dict(drives=1), dict(drives=2), dict(cols_per_slice=2, drives=2)):
                    p = vc.plan(n, C, m, **kw)
                    assert p["passes"] > 0 and p["bytes"] <= vc.LDS_BYTES, (n, m, C, kw, p)
                    assert p["U"] >= 1 and p["nc"] >= 1 and (p["mg"] >= 1) == (m > 0)


# ---- the finite-difference yardstick of the device test -----------------------------------------------------------------------------------------------------
def test_the_truth_against_its_own_central_difference():
    """The scipy truth's H v against (J(z + eps v)^T mu - J(z - eps v)^T mu) / (2 eps) with the truth's Jacobian, eps = 1e-5, on VL1.
    tests/test_var_large_exp_hess_gpu.py holds the device to 10 x FD_ORACLE."""
    err = vc.fd_oracle_error()
    print("the truth's H v against its central difference: %.2e of max |H v|" % err)
    assert 0.5 * vc.FD_ORACLE <= err <= vc.FD_ORACLE


# ---- the keyword ------------------------------------------------------------------------------------------------------------------------------------------
def test_keyword_validations():
    chk = pa.integrators._check_services
    V, VE, P = L.PCL_BATCH_VARIATIONAL, L.PCL_BATCH_VARIATIONAL_EXP, L.PCL_BATCH_MEMBERS
    assert chk(VE, "exp", large_generator=True, large_variational=True, large_var_exp=True, large_var_exp_hessian=True) is False
    assert chk(VE, "exp", large_generator=True, large_variational=True, large_var_exp=True, large_var_full=True, large_var_exp_hessian=True) is False
    with pytest.raises(ValueError, match="large_var_exp_hessian=True is the Hessian of the Lagrangian of a variational context created with large_var_exp=True .*: it needs that keyword"):
        chk(VE, "exp", large_var_exp_hessian=True)
    with pytest.raises(ValueError, match="large_var_exp_hessian=True .* it needs that keyword"):
        chk(V, 4, large_generator=True, large_variational=True, large_var_exp_hessian=True)
    with pytest.raises(ValueError, match="large_var_exp_hessian=True is the Hessian of the Lagrangian of a large variational exponential context .*: a plain context takes large_exp_hessian=True"):
        chk(P, "exp", large_generator=True, large_exp=True, large_var_exp_hessian=True)
    # the existing sentences keep their precedence and their words
    with pytest.raises(ValueError, match="so exp_hessian, var_compact and large_var_hessian stay off"):
        chk(VE, "exp", large_generator=True, large_variational=True, large_var_exp=True, large_var_hessian=True, large_var_exp_hessian=True)
    with pytest.raises(ValueError, match="large_var_exp=True is the variational exponential constraint at generator dimensions 66 .. 128: it needs pade_order"):
        chk(V, 4, large_generator=True, large_variational=True, large_var_exp=True, large_var_exp_hessian=True)
    row = pa.integrators._BY_OPTION["large_var_exp_hess"]
    assert (row.keyword, row.beside, row.family, row.constraint, row.sizes, row.at) == (
        "large_var_exp_hessian", "large_var_exp", "variational", None, "hess", "large_variational_exp")  # fmt: skip
    order = pa.integrators._OPTION_ORDER
    assert "large_var_exp_hess" in order and order.index("large_var_exp_hess") == order.index("large_var_hess") + 1
    keys = [r.keyword for r in pa.integrators._SERVICES]
    assert keys.index("large_var_exp_hessian") == keys.index("large_var_exp") + 1  # one row, beside large_var_exp
    for f in (pa.integrators._PclContext.__init__, pa.integrators.HipVariationalIntegrator.__init__):
        assert inspect.signature(f).parameters["large_var_exp_hessian"].default is False
    for ket in (True, False):  # both variational constructors' common body: before any device call
        with pytest.raises(ValueError, match="large_var_exp_hessian=True .* it needs that keyword"):
            pa.integrators.HipVariationalIntegrator(None, None, "x", ["xv"], "u", [None], ket=ket, pade_order="exp", large_var_exp_hessian=True)
    P = pa.PAULIS
    sysv = pa.VariationalQuantumSystem(P["Z"] / 2, [P["X"], P["Y"]], [P["Z"] / 2], [1.0, 1.0])
    for ctor in (pa.VariationalKetIntegrator, pa.VariationalUnitaryIntegrator):  # (the keyword is checked before the trajectory is looked at)
        with pytest.raises(ValueError, match="large_var_exp_hessian=True .* it needs that keyword"):
            ctor(sysv, None, "x", ["xv"], "u", pade_order="exp", large_generator=True, large_var_exp_hessian=True)
        with pytest.raises(ValueError, match="large_var_exp_hessian=True .* it needs that keyword"):
            ctor(sysv, None, "x", ["xv"], "u", pade_order="exp", large_var_exp_hessian=True)
    with pytest.raises(ValueError, match="a plain context takes large_exp_hessian=True"):  # a plain context, before the library is loaded
        pa.integrators._PclContext(d=2, m=2, N=4, z_dim=11, u_off=9, dt_off=8, x_offs=[0], G0=None, Gj=None, batch=1, batch_mode=P,
                                   large_var_exp_hessian=True)  # fmt: skip
    with pytest.raises(TypeError):  # (the plain integrator does not know the keyword)
        pa.HipPadeIntegrator(None, None, None, "x", large_var_exp_hessian=True)
