"""The cases of tests/exp_shape_cases.py before any GPU is involved: that each can do its job in tests/test_exp_shapes_gpu.py.

Reference floor: for every case the numpy emulation of the kernels' recurrences agrees with the committed truths (po.exp_residual, exp_truth,
exp_hess_truth, var_exp_truth, var_exp_hess_truth, the product of scipy.linalg.expm for the rollouts) per segment to 1e-13 of the segment's own
maximum -- a condition on the inputs, which leaves the GPU comparison at 1e-11 a factor 100 for the matrix cores' summation order.  Largest
value read per mode (the segment and case it was read at):
    plain residual 1.8e-14 (delta@2, P12)          plain Jacobian 2.1e-14 (-E@2, P8)             plain Hessian 3.4e-14 (uu@1, P3)
    plain rollout 1.4e-14 (knot3, P6)              variational residual 7.3e-15 (delta.1@2, V5)  variational Jacobian 1.3e-14 (-E.1@2, V5)
    variational Hessian 6.5e-14 (hh@1, V4)         variational rollout 2.9e-15 (knot3, V2)
The second derivatives (uu, hu, hh) sit at up to 6.5e-14 where a scalar is a sum of a few thousand products of either sign; no third derivative
is compared alone (the variational Hessian's are inside its uu and hu scalars).

Sensitivity: every case sees each fault the kernels' shape handling could have, injected into the emulation, in at least one segment at 1e-7
relative or more (1e4 x the GPU tolerance), in the Jacobian values and, where the case has a Hessian, in the Hessian values as well.

Structure: the expected structure of every case names each position once."""
import numpy as np
import pytest

import exp_hess_truth
import exp_shape_cases as ec
import exp_truth
import var_exp_hess_truth
import var_exp_truth
from shape_cases import check_segments

FLOOR = 1e-13
GPU_TOL = 1e-11
SEEN = 1e4 * GPU_TOL
PLAIN = list(ec.PLAIN_CASES)
PLAIN_HESS = [c for c in PLAIN if c not in ec.HESS_REFUSED]
VAR = list(ec.VAR_CASES)
VAR_HESS = list(ec.VAR_HESS_LDS + ec.VAR_HESS_WS)
VAR_ROLLOUT = ["V1", "V2"]


def worst(errs):
    s = max(errs, key=errs.get)
    return "%.1e (%s)" % (errs[s], s)


# ---- the case table's byte counts -------------------------------------------------------------------------------------------------------------
def test_lds_arithmetic_places_every_boundary_pair():
    """The launch code's own arithmetic (restated in exp_shape_cases) puts each pair on the two sides of its boundary."""
    c = ec.PLAIN_CASES
    assert ec.jac_lds_bytes(*c["P9"][1:]) == (158992, True) and ec.jac_lds_bytes(*c["P10"][1:]) == (134688, False)
    assert (4 * 62 * 60 + 62 * 30 + 96 + 62 * 60) * 8 == 164448 > ec.LDS_BYTES
    assert ec.hess_lds_bytes(56) == (156032, True) and ec.hess_lds_bytes(58) == (143968, False)
    assert ec.hess_lds_bytes(61) == (161168, False) and ec.hess_lds_bytes(63)[0] == 166448 > ec.LDS_BYTES
    assert ec.var_lds_bytes(56) == (155904, True) and ec.var_lds_bytes(58) == (143840, False) and ec.var_lds_bytes(60)[0] <= ec.LDS_BYTES
    for name in ec.VAR_HESS_LDS:
        assert ec.var_lds_bytes(2 * ec.VAR_CASES[name][0], 9)[0] <= ec.LDS_BYTES
    for name in ec.VAR_HESS_WS:
        assert ec.var_lds_bytes(2 * ec.VAR_CASES[name][0], 9)[0] > ec.LDS_BYTES
    for name, (kind, n, cols, m) in c.items():  # every Jacobian fits; the thread count switches between P2 and P3
        assert ec.jac_lds_bytes(n, cols, m)[0] <= ec.LDS_BYTES, name
    for name, (d, ket, m, v) in ec.VAR_CASES.items():  # the last phase of the variational kernels: cols <= n / 2, at most two variations
        assert (1 if ket else d) <= d and v <= 2


# ---- the reference floor ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PLAIN)
def test_floor_plain(name):
    lay, G0, Gj, Z = ec.plain_case(name)
    d0, v0 = ec.plain_truth(name)
    d, v = ec.emu_plain(lay, G0, Gj, Z)
    ed = check_segments(d, d0, ec.residual_labels(lay.n, lay.C, lay.K), FLOOR)
    jl = ec.jac_labels(lay.n, lay.C, lay.m, lay.K)
    ev = check_segments(v, v0, jl, FLOOR)
    assert np.array_equal(v[np.char.startswith(jl, "ones")], np.ones(lay.K * lay.x_dim))
    er = check_segments(ec.emu_rollout(lay, G0, Gj, Z), ec.plain_rollout_truth(name), ec.rollout_labels(lay.x_dim, lay.N), FLOOR)
    print("%s: residual %s  Jacobian %s  rollout %s" % (name, worst(ed), worst(ev), worst(er)))


@pytest.mark.parametrize("name", PLAIN_HESS)
def test_floor_plain_hessian(name):
    lay, G0, Gj, Z = ec.plain_case(name)
    mu, h0 = ec.plain_hess_truth(name)
    eh = check_segments(ec.emu_plain_hess(lay, G0, Gj, Z, mu), h0, ec.hess_labels(lay.n, lay.C, lay.m, lay.K), FLOOR)
    print("%s: Hessian %s" % (name, worst(eh)))


@pytest.mark.parametrize("name, seed, drift", [("P4", 0, 1), ("P1", 1, 0)])
def test_floor_batched_members(name, seed, drift):
    """The second member of the two batched cases (the first is the plain case itself)."""
    lay, G0, Gj, Z = ec.plain_case(name, seed, drift)
    d0, v0 = ec.plain_truth(name, seed, drift)
    d, v = ec.emu_plain(lay, G0, Gj, Z)
    check_segments(d, d0, ec.residual_labels(lay.n, lay.C, lay.K), FLOOR)
    check_segments(v, v0, ec.jac_labels(lay.n, lay.C, lay.m, lay.K), FLOOR)
    mu, h0 = ec.plain_hess_truth(name, seed, drift)
    check_segments(ec.emu_plain_hess(lay, G0, Gj, Z, mu), h0, ec.hess_labels(lay.n, lay.C, lay.m, lay.K), FLOOR)


@pytest.mark.parametrize("name", VAR)
def test_floor_variational(name):
    case = ec.var_case(name)
    d0, v0 = ec.var_truth(name)
    d, v = ec.emu_var(case)
    ed = check_segments(d, d0, ec.residual_labels(case.n, case.C, case.K, case.v), FLOOR)
    ev = check_segments(v, v0, ec.jac_labels(case.n, case.C, case.m, case.K, case.v), FLOOR)
    print("%s: residual %s  Jacobian %s" % (name, worst(ed), worst(ev)))


@pytest.mark.parametrize("name", VAR_HESS)
def test_floor_variational_hessian(name):
    case = ec.var_case(name)
    mu, h0 = ec.var_hess_truth(name)
    eh = check_segments(ec.emu_var_hess(case, mu), h0, ec.hess_labels(case.n, case.C, case.m, case.K, case.v), FLOOR)
    print("%s: Hessian %s" % (name, worst(eh)))


@pytest.mark.parametrize("name", VAR_ROLLOUT)
def test_floor_variational_rollout(name):
    case = ec.var_case(name)
    er = check_segments(ec.emu_var_rollout(case), ec.var_rollout_truth(name), ec.rollout_labels(case.xd, case.N), FLOOR)
    print("%s: rollout %s" % (name, worst(er)))


# ---- sensitivity --------------------------------------------------------------------------------------------------------------------------------
def seen(good, bad, labels):
    """The largest relative change of a segment (against the segment's own maximum)."""
    out = 0.0
    for s in np.unique(labels):
        sel = labels == s
        scale = np.abs(good[sel]).max()
        if scale > 0:
            out = max(out, np.abs(bad[sel] - good[sel]).max() / scale)
    return out


def swap_drive_slices(vals, labels, stem):
    """Drive 0's slice (labels `stem`0..) taken from drive 1."""
    bad = vals.copy()
    for s in np.unique(labels):
        if s.startswith(stem % 0):
            bad[labels == s] = vals[labels == s.replace(stem % 0, stem % 1, 1)]
    return bad


def assert_sensitive(name, n, C, m, jac, hess, jl, hl):
    """jac(mm, fewer_on) -> values, hess the same or None.  The five faults of the issue."""
    good_j = jac(np.matmul, None)
    good_h = hess(np.matmul, None) if hess else None
    faults = {"last k step": (ec.mm_drop_last_k_step(n), None), "last row tile": (ec.mm_drop_last_row_tile(n), None), "one squaring fewer": (np.matmul, 2)}
    for what, (mm, fewer_on) in faults.items():
        sj = seen(good_j, jac(mm, fewer_on), jl)
        sh = seen(good_h, hess(mm, fewer_on), hl) if hess else None
        print("%s, %s: Jacobian moved by %.1e%s" % (name, what, sj, "" if sh is None else ", Hessian by %.1e" % sh))
        assert sj >= SEEN and (sh is None or sh >= SEEN), (name, what, sj, sh)
    if m >= 2:
        sj = seen(good_j, swap_drive_slices(good_j, jl, "du%d"), jl)
        sh = seen(good_h, swap_drive_slices(good_h, hl, "u%d.Xk"), hl) if hess else None
        assert sj >= SEEN and (sh is None or sh >= SEEN), (name, "drive slice", sj, sh)
    if C > 1:  # one state column's copy of -E left unwritten (at the NaN the outputs are prefilled with: here zero)
        bad = good_j.copy()
        per = len(good_j) // (ec.N - 1)
        bad[n * n : 2 * n * n] = 0.0
        bad[2 * per + (C - 1) * n * n : 2 * per + C * n * n] = 0.0
        assert seen(good_j, bad, jl) >= SEEN


@pytest.mark.parametrize("name", PLAIN)
def test_sensitive_plain(name):
    lay, G0, Gj, Z = ec.plain_case(name)
    mu = ec.rand_mu(lay.K * lay.x_dim, name)
    jac = lambda mm, f: ec.emu_plain(lay, G0, Gj, Z, mm=mm, fewer_on=f)[1]
    hess = (lambda mm, f: ec.emu_plain_hess(lay, G0, Gj, Z, mu, mm=mm, fewer_on=f)) if name in PLAIN_HESS else None
    assert_sensitive(name, lay.n, lay.C, lay.m, jac, hess, ec.jac_labels(lay.n, lay.C, lay.m, lay.K), ec.hess_labels(lay.n, lay.C, lay.m, lay.K))
    good = ec.emu_rollout(lay, G0, Gj, Z)  # the rollout: the two product faults
    for mm in (ec.mm_drop_last_k_step(lay.n), ec.mm_drop_last_row_tile(lay.n)):
        assert seen(good.reshape(-1), ec.emu_rollout(lay, G0, Gj, Z, mm=mm).reshape(-1), ec.rollout_labels(lay.x_dim, lay.N)) >= SEEN


@pytest.mark.parametrize("name", VAR)
def test_sensitive_variational(name):
    case = ec.var_case(name)
    mu = ec.rand_mu(case.K * case.xd, name)
    jac = lambda mm, f: ec.emu_var(case, mm=mm, fewer_on=f)[1]
    hess = (lambda mm, f: ec.emu_var_hess(case, mu, mm=mm, fewer_on=f)) if name in VAR_HESS else None
    assert_sensitive(name, case.n, case.C, case.m, jac, hess, ec.jac_labels(case.n, case.C, case.m, case.K, case.v),
                     ec.hess_labels(case.n, case.C, case.m, case.K, case.v))  # fmt: skip


# ---- structure ----------------------------------------------------------------------------------------------------------------------------------
def once(r, c, count):
    assert len(r) == len(c) == count == len(set(zip(r.tolist(), c.tolist())))


@pytest.mark.parametrize("name", PLAIN)
def test_structure_plain(name):
    """exp_truth.structure and exp_hess_truth.structure on the multi-ket and vector layouts: every position once, inside the matrix, the
    Hessian in the lower triangle; the labels count the same values."""
    lay = ec.plain_layout(name)
    r, c = exp_truth.structure(lay)
    once(r, c, lay.K * exp_truth.nnz_per_interval(lay))
    assert r.min() == 0 and r.max() == lay.K * lay.x_dim - 1 and c.min() >= 0 and c.max() < lay.N * lay.z_dim
    assert len(ec.jac_labels(lay.n, lay.C, lay.m, lay.K)) == len(r)
    r, c = exp_hess_truth.structure(lay)
    once(r, c, lay.K * exp_hess_truth.nnz_per_interval(lay))
    assert np.all(r >= c) and c.min() >= 0 and r.max() < lay.N * lay.z_dim
    assert len(ec.hess_labels(lay.n, lay.C, lay.m, lay.K)) == len(r)


@pytest.mark.parametrize("name", VAR)
def test_structure_variational(name):
    case = ec.var_case(name)
    r, c = var_exp_truth.structure(case)
    once(r, c, case.K * var_exp_truth.nnz_per_interval(case))
    assert r.min() == 0 and r.max() == case.K * case.xd - 1 and c.min() >= 0 and c.max() < case.N * case.z_dim
    assert len(ec.jac_labels(case.n, case.C, case.m, case.K, case.v)) == len(r)
    r, c = var_exp_hess_truth.structure(case)
    once(r, c, case.K * var_exp_hess_truth.nnz_per_interval(case))
    assert np.all(r >= c) and r.max() < case.N * case.z_dim
    assert len(ec.hess_labels(case.n, case.C, case.m, case.K, case.v)) == len(r)
