"""The Hessian of the Lagrangian at generator dimensions 66 .. 128 (option large_hess on a context created with PCL_LARGE_N) before any GPU is
involved, at the cases of tests/large_hess_cases.py: the launch code's plan, the reference floor, what the cases can see, and the keyword
validation of the host mirror.

Reference floor: for every case and order in (2, 4, 6, 8, 10) po.pade_hessian_values agrees with the longdouble truth per segment
(shape_cases.hess_labels) to 1e-13 of the segment's own maximum -- worst segment 2.4e-14 over the nine cases -- which leaves the GPU comparison
at 1e-11 a factor 100 and more for the kernel's summation order.  The kernel's own formulation (no U_il blocks: forward Horner chain, backward
chains on G^T), restated in float64 numpy, is held to the same floor.

Sensitivity: every case sees, in at least one Hessian segment at 1e-7 relative or more (1e4 x the GPU tolerance), each of: every product's k
range beyond 64 dropped, the last 16-row tile of every product zeroed, the last drive dropped, the last state column dropped; and at order 10
zeroing c_5 moves interval 2's scalar entries by 1e-7 or more.

Without the feature the keyword tests fail: `large_hessian` is an unknown keyword (TypeError, not ValueError)."""
import numpy as np
import pytest

import large_hess_cases as hc
import large_shape_cases as lc
import piccolo_jl_amd as pa
import vector_shape_cases as vc
from oracle import pade_oracle as po
from shape_cases import check_segments, hess_labels

FLOOR = 1e-13
SEEN = 1e4 * hc.TOL
NAMES = hc.NAMES


def worst(errs):
    s = max(errs, key=errs.get)
    return errs[s], s


def seen(good, bad, labels, only=None):
    """The largest relative change of a segment (against the segment's own maximum); only: a predicate on the segment's name."""
    out = 0.0
    for s in np.unique(labels):
        if only is not None and not only(str(s)):
            continue
        sel = labels == s
        scale = np.abs(good[sel]).max()
        if scale > 0:
            out = max(out, float(np.abs(bad[sel] - good[sel]).max() / scale))
    return out


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------------
def test_plan_table():
    for name, (kind, n, cols, m) in hc.CASES.items():
        p = hc.hess_plan(n, cols, m)
        assert (p["U"], p["sx"], p["nc"], p["ngrp"], p["mg"], p["bytes"]) == hc.TABLE[name], (name, p)
        assert p["bytes"] <= hc.LDS_BYTES and p["threads"] == 64 * ((n + 15) // 16) <= 512 and p["LD"] == n | 1, name
        assert sum(p["nce"]) == cols and min(p["nce"]) > 0 and sum(p["mge"]) == m and min(p["mge"]) > 0, name  # every column and drive once, no idle unit
    # the splits the GPU test forces
    assert hc.hess_plan(72, 5, 4, cols_per_slice=2)["nce"] == [2, 2, 1] and hc.hess_plan(72, 5, 4, cols_per_slice=1)["sx"] == 5
    assert hc.hess_plan(66, 33, 1, cols_per_slice=7)["nce"] == [7, 7, 7, 7, 5] and hc.hess_plan(66, 33, 1)["nce"] == [11, 11, 11]
    assert hc.hess_plan(120, 1, 24, drives=1)["U"] == 24 and hc.hess_plan(120, 1, 24, drives=5)["mge"] == [5, 5, 5, 5, 4]
    assert hc.hess_plan(120, 1, 24)["mge"] == [8, 8, 8] and hc.hess_lds_bytes(120, 24, 1, 9) <= hc.LDS_BYTES < hc.hess_lds_bytes(120, 24, 1, 10)  # (auto: nine fit, three groups, evened)
    assert hc.hess_plan(66, 1, 2, drives=1)["mge"] == [1, 1] and hc.hess_plan(66, 1, 2, drives=2)["mge"] == [2]
    # nothing is refused for m <= 24, n <= 128: one column with one drive always fits, and no drive at all does
    for n in (66, 96, 120, 127, 128):
        for cols in (1, 5, n // 2):
            for m in (0, 1, 24):
                p = hc.hess_plan(n, cols, m)
                assert p["bytes"] <= hc.LDS_BYTES and p["nc"] >= 1 and (p["mg"] >= 1 if m else p["mg"] == 0), (n, cols, m, p)
    assert hc.hess_lds_bytes(128, 24, 1, 1) == 148032


# ---- the reference floor ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_oracle_floor(name):
    lay, G0, Gj, Z, _ = lc.case(name)
    mu = hc.rand_mu(name)
    labels = hess_labels(lay)
    for order in hc.ORDERS:
        ref = hc.truth(name, order)
        assert ref.size == po.hess_nnz_per_interval(lay) * lay.K
        eo = check_segments(po.pade_hessian_values(Z, mu.reshape(lay.K, -1), lay, G0, Gj, order), ref, labels, FLOOR)
        ef = check_segments(hc.formulation_values(lay, G0, Gj, Z, mu, order), ref, labels, FLOOR)
        print("%s order %d: oracle %.1e (%s)  the kernel's formulation %.1e (%s)" % ((name, order) + worst(eo) + worst(ef)))


def test_order_2_has_no_uu_and_no_hh():
    """At order 2 the (u, u) and (h, h) entries are identically zero: the truth says so, and check_segments holds a zero segment to zero."""
    lay = lc.layout("L5")
    ref, labels = hc.truth("L5", 2), hess_labels(lay)
    for k in range(lay.K):
        assert not ref[(labels == "uu@%d" % k) | (labels == "hh@%d" % k)].any() and ref[labels == "hu@%d" % k].all()


# ---- sensitivity --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_every_case_sees_the_shape_faults(name):
    kind, n, cols, m = hc.CASES[name]
    lay, G0, Gj, Z, _ = lc.case(name)
    labels, mu, order = hess_labels(lay), hc.rand_mu(name), 4
    good = hc.truth_ld(name, order)
    faults = {"k beyond 64": dict(mm=lc.mm_drop_k_beyond_64(n)), "last row tile": dict(mm=lc.mm_zero_last_row_tile(n)), "last drive": dict(drop_drive=True),
              "last state column": dict(drop_col=True)}  # fmt: skip
    for what, kw in faults.items():
        bad = vc.truth_values(lay, G0, Gj, Z, mu, order, hessian=True, **kw)[2].reshape(-1)
        s = seen(good, bad, labels)
        print("%s order %d, %s: a Hessian segment moved by %.1e" % (name, order, what, s))
        assert s >= SEEN, (name, what, s)


@pytest.mark.parametrize("name", NAMES)
def test_the_long_step_sees_the_top_coefficient(name):
    lay, G0, Gj, Z, _ = lc.case(name)
    labels, mu = hess_labels(lay), hc.rand_mu(name)
    c0 = vc.coeffs(10).copy()
    c0[-1] = 0
    bad = vc.truth_values(lay, G0, Gj, Z, mu, 10, c=c0, hessian=True)[2].reshape(-1)
    s = seen(hc.truth_ld(name, 10), bad, labels, only=lambda seg: seg in ("uu@2", "hu@2", "hh@2"))
    print("%s: zeroing c_5 moves interval 2's scalar entries by %.1e" % (name, s))
    assert s >= SEEN, (name, s)


# ---- the keyword, before any device call --------------------------------------------------------------------------------------------------------
def _mk(d, **over):
    n = 2 * d
    kw = dict(d=d, m=1, N=3, z_dim=n + 3, u_off=n + 2, dt_off=n, x_offs=[0], G0=np.zeros((n, n)), Gj=np.zeros((1, n, n)), batch=1,
              batch_mode=pa._lib.PCL_BATCH_MEMBERS, state_cols=1, pade_order=4)  # fmt: skip
    kw.update(over)
    return kw


def test_context_keyword_validation():
    with pytest.raises(ValueError, match="large_generator"):
        pa.integrators._PclContext(**_mk(33, large_hessian=True))
    with pytest.raises(ValueError, match="exp"):
        pa.integrators._PclContext(**_mk(33, large_generator=True, large_hessian=True, pade_order="exp"))
    for mode in (pa._lib.PCL_BATCH_VARIATIONAL, pa._lib.PCL_BATCH_VARIATIONAL_EXP):
        with pytest.raises(ValueError, match="variational"):
            pa.integrators._PclContext(**_mk(33, large_generator=True, large_hessian=True, batch_mode=mode))


def _ket_problem(d=33):
    rng = np.random.default_rng(5)
    s = pa.QuantumSystem(vc._herm(d, rng), [vc._herm(d, rng)], [1.0])
    psi = np.zeros(d, complex)
    psi[0] = 1
    return s, pa.ket_trajectory(s, np.zeros((1, 4)), np.linspace(0, 0.1, 4), psi, psi)


def test_integrator_keyword_validation():
    s, t = _ket_problem()
    KET = pa.trajectory.KET
    with pytest.raises(ValueError, match="large_generator"):
        pa.BilinearIntegrator(s, t, x_name=KET, pade_order=4, large_hessian=True)
    with pytest.raises(ValueError, match="exp"):
        pa.BilinearIntegrator(s, t, x_name=KET, pade_order="exp", large_generator=True, large_hessian=True)
    with pytest.raises(ValueError, match="large_generator"):
        pa.HipPadeIntegrator(s.G_drift, s.G_drives_array(), t, KET, large_hessian=True)


def test_variational_constructors_refuse_the_keyword():
    with pytest.raises(ValueError, match="variational"):
        pa.integrators.HipVariationalIntegrator(None, None, "x", ["xv"], "u", [None], ket=True, large_hessian=True)


# ---- the finite-difference yardstick of the public-interface test -------------------------------------------------------------------------------
def test_the_oracle_against_its_own_central_difference():
    """The float64 oracle's H v against (J(z + eps v)^T mu - J(z - eps v)^T mu) / (2 eps) with the oracle's Jacobian, eps = 1e-5, on the d = 33 ket
    problem: measured 1.76e-9 of max |H v|.  tests/test_large_hess_gpu.py holds the library to 10 x FD_ORACLE through pa.eval_jacobian."""
    s, traj, Z, lay = hc.ket33_problem()
    G0, Gj = s.G_drift, s.G_drives_array()
    mu, v = hc.fd_inputs(lay)
    H = po.hessian_dense(po.pade_hessian_values(Z, mu.reshape(lay.K, -1), lay, G0, Gj, hc.FD_ORDER), lay)
    jt_mu = lambda z: po.pade_jacobian_dense(z.reshape(lay.N, lay.z_dim), lay, G0, Gj, hc.FD_ORDER).T @ mu
    err = hc.fd_error(H @ v, jt_mu, Z.reshape(-1), v)
    print("the oracle's H v against its central difference: %.2e of max |H v|" % err)
    assert 0.5 * hc.FD_ORACLE <= err <= hc.FD_ORACLE
