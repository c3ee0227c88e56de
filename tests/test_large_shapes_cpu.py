"""The cases of tests/large_shape_cases.py (generator dimensions 66 .. 128, PCL_LARGE_N) before any GPU is involved: that each can do its job in
tests/test_large_shapes_gpu.py, that the case table sits where the launch code's plan branches, and what pcl_create decides about the flag
before it touches a device.

Reference floor: for every case and order in (2, 4, 6, 8, 10) po.pade_residual and po.pade_jacobian_values agree with the longdouble truth per
segment to 1e-13 of the segment's own maximum, which leaves the GPU comparison at 1e-11 a factor 100 for the kernel's summation order over up
to 128 terms.

Sensitivity: every case sees, in at least one segment at 1e-7 relative or more (1e4 x the GPU tolerance), each of: every product's k range
beyond 64 dropped (what a kernel of 16 k-steps would do), the last 16-row tile of every product zeroed, the last drive dropped, the last state
column dropped."""
import numpy as np
import pytest

import large_shape_cases as lc
import piccolo_jl_amd as pa
import vector_shape_cases as vc
from oracle import pade_oracle as po
from shape_cases import check_segments, jac_labels

FLOOR = 1e-13
GPU_TOL = 1e-11
SEEN = 1e4 * GPU_TOL
NAMES = lc.NAMES


def worst(errs):
    s = max(errs, key=errs.get)
    return errs[s], s


def seen(good, bad, labels):
    """The largest relative change of a segment (against the segment's own maximum)."""
    out = 0.0
    for s in np.unique(labels):
        sel = labels == s
        scale = np.abs(good[sel]).max()
        if scale > 0:
            out = max(out, float(np.abs(bad[sel] - good[sel]).max() / scale))
    return out


# ---- the case table's claims ----------------------------------------------------------------------------------------------------------------------
def test_case_table_sits_where_the_plan_branches():
    plan = {name: lc.large_plan(n, cols, m) for name, (kind, n, cols, m) in lc.CASES.items()}
    for name, (kind, n, cols, m) in lc.CASES.items():
        p = plan[name]
        assert (p["U"], p["sx"], p["ngrp"], p["mg"], p["npc"], p["bytes"]) == lc.TABLE[name], (name, p)
        assert p["bytes"] <= lc.LDS_BYTES and p["chain_blocks"] + p["npc"] <= p["NB"], name
        assert 1 <= p["pairs"] <= lc.NP_PAIRS and p["threads"] == 64 * p["row_tiles"] <= 512, name
        assert sum(p["nce"]) == cols and sum(p["npce"]) == n and min(p["npce"]) > 0, name  # every column once, no unit without work
        assert p["ngrp"] * p["mg"] >= m > (p["ngrp"] - 1) * p["mg"] if m else p["ngrp"] == 1
        for jac in (False, True):  # and the residual-only launch
            assert lc.large_plan(n, cols, m, jac=jac)["bytes"] <= lc.LDS_BYTES, name
    # row tiles and k-steps
    assert plan["L1"]["row_tiles"] == 5 and 66 - 64 == 2 and plan["L1"]["k_steps"] == 17 and 66 % 4 == 2
    assert plan["L2"]["row_tiles"] == 6 and 96 % 16 == 0
    assert plan["L3"]["row_tiles"] == 8 and plan["L3"]["k_steps"] == 32 and plan["L3"]["NB"] == 29 and plan["L3"]["U"] == 8
    # L4: 2 (2 + 24) + 2 = 54 chain blocks do not fit beside the tile: two groups of 12 drives, 30 blocks each
    assert plan["L4"]["NB"] == 47 < 2 * (2 + 24) + 2 and plan["L4"]["ngrp"] == 2 and plan["L4"]["mg"] == 12 and plan["L4"]["chain_blocks"] == 30
    # L5: one chain unit of five columns; the forced slicings of the GPU test
    assert plan["L5"]["nce"] == [5] and plan["L5"]["npce"] == [15, 15, 15, 15, 12]
    assert lc.large_plan(72, 5, 4, cols_per_slice=2)["nce"] == [2, 2, 1] and lc.large_plan(72, 5, 4, cols_per_slice=1)["sx"] == 5
    assert lc.large_plan(72, 5, 4, slices=1)["U"] == 2 and lc.large_plan(72, 5, 4, slices=72)["npc"] == 1  # (one unit: 9 pairs per thread, refused)
    # L6: 33 columns of 8 blocks exceed the 237 beside the tile: slices of 17 and 16
    assert 33 * 8 > plan["L6"]["NB"] == 237 and plan["L6"]["nce"] == [17, 16]
    assert lc.large_plan(66, 33, 1, cols_per_slice=1)["U"] == 33 and lc.large_plan(66, 33, 1, slices=66)["npce"] == [1] * 66
    # odd n: LD = n, a pair may straddle two columns
    for name in ("L7", "L8", "L9"):
        assert plan[name]["LD"] == lc.CASES[name][1] and lc.CASES[name][1] % 2 == 1
    assert 81 % 16 == 1 and plan["L7"]["row_tiles"] == 6 and plan["L9"]["row_tiles"] == 8
    # the largest shape the flag admits with the most drives still fits: one drive at a time if need be
    p = lc.large_plan(128, 64, 24)
    assert p["bytes"] <= lc.LDS_BYTES and p["nc"] >= 1 and p["mg"] >= 1


@pytest.mark.parametrize("name", NAMES)
def test_steps(name):
    lay, G0, Gj, Z, long_step = lc.case(name)
    th = [Z[k, lay.dt_off] * np.linalg.norm(vc.g_of(lay, Z, k, G0, Gj), 2) for k in range(lay.K)]
    assert np.allclose(th, [0.15, -0.3, long_step], rtol=1e-12)
    assert long_step == (0.5 if lc.CASES[name][0] == "iso" else 0.65)
    w = vc.top_term_weight(lay, G0, Gj, Z)
    assert w >= SEEN
    print("%s: long step %.2f, c_5 moves the residual by %.1e" % (name, long_step, w))


# ---- the reference floor ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_oracle_floor(name):
    lay, G0, Gj, Z, _ = lc.case(name)
    for order in lc.ORDERS:
        d, j = lc.truth(name, order)
        er = check_segments(po.pade_residual(Z, lay, G0, Gj, order), d, lc.residual_labels(lay), FLOOR)
        ej = check_segments(po.pade_jacobian_values(Z, lay, G0, Gj, order), j, jac_labels(lay), FLOOR)
        print("%s order %d: residual %.1e (%s)  Jacobian %.1e (%s)" % ((name, order) + worst(er) + worst(ej)))


def test_oracle_floor_of_the_batched_members():
    """The other members of the batched cases of the GPU test: L1's second drift, L7's second seed."""
    for name, kw in (("L1", dict(drift=1)), ("L7", dict(seed=1))):
        lay, G0, Gj, Z, _ = lc.case(name, **kw)
        for order in (4, 8):
            d, j = lc.truth(name, order, **kw)
            check_segments(po.pade_residual(Z, lay, G0, Gj, order), d, lc.residual_labels(lay), FLOOR)
            check_segments(po.pade_jacobian_values(Z, lay, G0, Gj, order), j, jac_labels(lay), FLOOR)


# ---- sensitivity ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_every_case_sees_the_shape_faults(name):
    kind, n, cols, m = lc.CASES[name]
    lay, G0, Gj, Z, _ = lc.case(name)
    dl, jl = lc.residual_labels(lay), jac_labels(lay)
    faults = {"k beyond 64": dict(mm=lc.mm_drop_k_beyond_64(n)), "last row tile": dict(mm=lc.mm_zero_last_row_tile(n)), "last drive": dict(drop_drive=True),
              "last state column": dict(drop_col=True)}  # fmt: skip
    for order in (2, 10):
        d, j = lc.truth_ld(name, order)
        for what, kw in faults.items():
            bd, bj, _ = vc.truth_values(lay, G0, Gj, Z, None, order, hessian=False, **kw)
            sd, sj = seen(d, bd.reshape(-1), dl), seen(j, bj.reshape(-1), jl)
            print("%s order %d, %s: residual moved by %.1e, Jacobian by %.1e" % (name, order, what, sd, sj))
            assert max(sd, sj) >= SEEN, (name, order, what, sd, sj)
            if what == "k beyond 64":  # (the whole residual, not one corner of it)
                assert sd >= 2.3e-2, (name, order, sd)


# ---- what pcl_create decides before it touches a device -------------------------------------------------------------------------------------------
def _mk(d, flag=True, **over):
    n = 2 * d
    kw = dict(d=d, m=1, N=3, z_dim=n + 3, u_off=n + 2, dt_off=n, x_offs=[0], G0=np.zeros((n, n)), Gj=np.zeros((1, n, n)), batch=1,
              batch_mode=pa._lib.PCL_BATCH_MEMBERS, state_cols=1, pade_order=4, large_generator=flag)  # fmt: skip
    kw.update(over)
    return kw


def _refused(code, *words, **kw):
    with pytest.raises(pa.PclError) as ei:
        pa.integrators._PclContext(**kw)
    assert ei.value.code == code, str(ei.value)
    for w in words:
        assert w in str(ei.value), str(ei.value)


def test_flagged_generator_of_66_passes_validation():
    """d = 33 with the flag gets as far as the device: without one, PCL_EHIP "no CPU path" -- not the PCL_ESHAPE of an unflagged descriptor."""
    import torch

    pa.build_library()
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    _refused(pa._lib.PCL_EHIP, "no CPU path", **_mk(33))
    _refused(pa._lib.PCL_EHIP, "no CPU path", **_mk(64, batch_mode=pa._lib.PCL_BATCH_TRAJ))
    _refused(pa._lib.PCL_EHIP, "no CPU path", **_mk(127, state_cols=pa._lib.PCL_STATE_VECTOR, G0=np.zeros((127, 127)), Gj=np.zeros((1, 127, 127)), z_dim=130, u_off=129, dt_off=127))
    _refused(pa._lib.PCL_EHIP, "no CPU path", **_mk(27))  # the flag at n <= 64: the ordinary context's path


def test_flag_validation_without_a_device():
    pa.build_library()
    _refused(pa._lib.PCL_ESHAPE, "generator dimension 130", "128", "163840", **_mk(65))
    _refused(pa._lib.PCL_ESHAPE, "generator dimension 129", "128", **_mk(129, state_cols=pa._lib.PCL_STATE_VECTOR, G0=np.zeros((129, 129)), Gj=np.zeros((1, 129, 129))))
    _refused(pa._lib.PCL_ENOTIMPL, "PCL_LARGE_N", "PCL_ORDER_EXP", **_mk(33, pade_order="exp"))
    _refused(pa._lib.PCL_ENOTIMPL, "PCL_LARGE_N", "PCL_ORDER_EXP", **_mk(8, pade_order="exp"))
    var = dict(batch=2, per_member_G0=True, x_offs=[0, 0])
    _refused(pa._lib.PCL_ENOTIMPL, "PCL_LARGE_N", "PCL_BATCH_VARIATIONAL", **_mk(33, batch_mode=pa._lib.PCL_BATCH_VARIATIONAL, G0=np.zeros((2, 66, 66)), **var))
    _refused(pa._lib.PCL_ENOTIMPL, "PCL_LARGE_N", "PCL_BATCH_VARIATIONAL_EXP",
             **_mk(33, batch_mode=pa._lib.PCL_BATCH_VARIATIONAL_EXP, pade_order="exp", G0=np.zeros((2, 66, 66)), **var))
    # without the flag: as before, in the same words, with a hint behind them
    _refused(pa._lib.PCL_ESHAPE, "generator dimension 66 exceeds 64 (LDS-resident tiles; d <= 32)", "PCL_LARGE_N", **_mk(33, flag=False))
    _refused(pa._lib.PCL_EINVAL, "unknown batch_mode 7", **_mk(4, flag=False, batch_mode=7))


def test_the_mirror_never_sets_the_flag_by_itself():
    """BilinearIntegrator on a d = 33 ket system without the keyword is refused as before (PCL_ESHAPE); the constant is the header's."""
    pa.build_library()
    assert pa._lib.PCL_LARGE_N == 0x100
    hdr = open(pa._lib.INCLUDE + "/piccolo_hip.h").read()
    assert "#define PCL_LARGE_N 0x100" in hdr and "#define PCL_MAX_D 32 " in hdr
    rng = np.random.default_rng(5)
    H = vc._herm(33, rng)
    s = pa.QuantumSystem(H, [vc._herm(33, rng)], [1.0])
    psi = np.zeros(33, complex)
    psi[0] = 1
    t = pa.ket_trajectory(s, np.zeros((1, 4)), np.linspace(0, 0.1, 4), psi, psi)
    with pytest.raises(pa.PclError) as ei:
        pa.BilinearIntegrator(s, t, x_name=pa.trajectory.KET, pade_order=4)
    assert ei.value.code == pa._lib.PCL_ESHAPE and "generator dimension 66" in str(ei.value)
