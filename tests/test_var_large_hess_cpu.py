"""What tests/test_var_large_hess_gpu.py stands on, without a GPU: the plan of the large variational Hessian launch per case and over the sizes
(nothing refused), the value order against the lifted structure, the float64 lifted oracle and the restated pass formulation against the
longdouble truth per segment (the floor the GPU tolerance of 1e-11 leaves decades above), the decomposition into passes, what each case sees of
five mutants, the finite-difference yardstick of the public-interface test, and the keyword."""
import inspect

import numpy as np
import pytest

import piccolo_jl_amd as pa
import var_large_hess_cases as vh
import variational_shape_cases as vsc
import variational_truth as vt
from oracle import pade_oracle as po

FLOOR = 1e-13
SEEN = vh.SEEN  # 1e-7: what a mutant must move, on the truth alone
L = pa._lib


def worst(errors):
    return max((e / s if s else (0.0 if e == 0 else np.inf)) for e, s in errors.values())


# ---- the plan -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", vh.NAMES)
def test_plan_table(name):
    n, C, v, m = vh.shape(name)
    p = vh.plan(n, C, m)
    assert (p["sx"], p["nc"], p["ngrp"], p["mg"], p["U"], p["bytes"]) == vh.TABLE[name]
    assert p["bytes"] <= vh.LDS_BYTES and p["sx"] * p["nc"] >= C and p["ngrp"] * p["mg"] >= m and p["threads"] <= 512
    assert (p["sx"] - 1) * p["nc"] < C and (m == 0 or (p["ngrp"] - 1) * p["mg"] < m)  # no unit without work


def test_tightest_units():
    """The arithmetic of the byte formula at n = 128: one column and one drive with m = 24, and VL4's m = 1."""
    assert vh.lds_bytes(128, 24, 1, 1) == (16512 + 3612 + 128 + 32 + 26) * 8 == 162480
    assert vh.lds_bytes(128, 1, 1, 1) == 162112


def test_nothing_is_refused():
    """Every even n in 66 .. 128, m in {0, 1, 24}, kets and unitaries (the plan does not depend on v: a unit holds component 0 and the running
    pass's), under every cap of the two knobs that the GPU tests use."""
    for n in range(66, 130, 2):
        for m in (0, 1, 24):
            for v in (1, 2):
                for C in (1, n // 2):
                    for kw in ({}, dict(cols_per_slice=1), dict(drives=1), dict(cols_per_slice=5, drives=5)):
                        p = vh.plan(n, C, m, **kw)
                        assert p["bytes"] <= vh.LDS_BYTES, (n, m, v, C, kw, p)
                        assert p["U"] >= 1 and p["nc"] >= 1 and (p["mg"] >= 1) == (m > 0)


# ---- the value order --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", vh.NAMES)
def test_value_order_against_the_lifted_structure(name):
    """value_index brings pade_oracle.hess_structure of the lifted layout, mapped through variational_truth._col_map, onto the restated
    structure of the library position by position."""
    cs = vh.case(name)
    lay = vt.lifted(cs)[1]
    cm = vt._col_map(cs, lay)
    a, b = po.hess_structure(lay)
    a, b = cm[a], cm[b]
    per, vi = vh.values_per_interval(cs), vh.value_index(cs)
    assert per == po.hess_nnz_per_interval(lay) and np.array_equal(np.sort(vi), np.arange(per))
    r, c = vh.lib_structure(cs)
    assert np.array_equal(np.maximum(a, b).reshape(cs.K, per)[:, vi].reshape(-1), r)
    assert np.array_equal(np.minimum(a, b).reshape(cs.K, per)[:, vi].reshape(-1), c)
    r1, c1 = vh.lib_structure(cs, 1)
    assert np.array_equal(r1, r + 1) and np.array_equal(c1, c + 1)


# ---- the floor ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", vh.NAMES)
def test_oracle_and_pass_formulation_against_the_truth(name):
    """Per segment, relative to the segment's own maximum, at every order.  Worst values read over the cases: the oracle 3.2e-14 (VL2, order 4),
    the pass formulation 1.4e-14 (VH1, order 4); the printed lines carry each case's."""
    cd = vh.codes(name)
    for order in vh.ORDERS:
        tr = vh.truth_ld(name, order)
        wo = worst(vsc.segment_errors(cd, vh.oracle_values(name, order), tr))
        pv = vh.pass_values(name, order).reshape(-1)
        wp = worst(vsc.segment_errors(cd, pv, tr))
        print("FLOOR %s order %d: oracle %.1e  pass formulation %.1e" % (name, order, wo, wp))
        assert wo <= FLOOR and wp <= FLOOR, (name, order, wo, wp)


@pytest.mark.parametrize("name", ["VL1", "VL2", "VL4"])
def test_the_passes_add_up(name):
    """Pass 0 + .. + pass v = the lifted Hessian (the oracle's), and pass b alone is the Hessian under the multipliers of component b alone."""
    cs = vh.case(name)
    cd = vh.codes(name)
    for order in (2, 6, 10):
        parts = [vh.pass_values(name, order, passes=[b]).reshape(-1) for b in range(1 + cs.v)]
        want = vh.oracle_values(name, order)
        assert worst(vsc.segment_errors(cd, sum(parts), want)) <= FLOOR
        for b in range(1 + cs.v):
            mu = np.zeros((cs.K, 1 + cs.v, cs.xdc))
            mu[:, b] = vh.rand_mu(name).reshape(cs.K, 1 + cs.v, cs.xdc)[:, b]
            alone = vh.oracle_values(name, order, mu.reshape(-1))
            scale = vsc.segment_max(cd, want)
            err = vsc.segment_max(cd, parts[b] - alone)
            assert all(err[s] <= FLOOR * scale[s] for s in err), (name, order, b)
        i0, ib, _ = vh.component_slices(cs)
        assert np.all(parts[0][ib] == 0.0)  # pass 0 knows no variation


# ---- mutants ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", vh.NAMES)
def test_mutants_are_seen(name):
    """A zeroed c_q, an ignored last drive, an ignored last state column, a zeroed Gv_v and a dropped pass v each move a Hessian segment by
    1e-7 of its own size or more, on the truth alone (order 10 for c_q: the long step is chosen for c_5; order 4 for the others)."""
    cs = vh.case(name)
    cd = vh.codes(name)
    import vector_shape_cases as vs

    c10 = np.array(vs.coeffs(10))
    c10[-1] = 0
    good10, good4 = vh.truth_ld(name, 10), vh.truth_ld(name, 4)
    seen = {"c_q": vsc.moved(cd, good10, vh.lifted_values(name, 10, c=c10).reshape(-1))}
    if cs.m:
        seen["last drive"] = vsc.moved(cd, good4, vh.lifted_values(name, 4, drop_drive=True).reshape(-1))
    if cs.C > 1:
        seen["last column"] = vsc.moved(cd, good4, vh.lifted_values(name, 4, drop_col=True).reshape(-1))
    seen["Gv_v"] = vsc.moved(cd, good4, vh.lifted_values(name, 4, zero_last_variation=True).reshape(-1))
    mu = np.array(vh.rand_mu(name)).reshape(cs.K, 1 + cs.v, cs.xdc)
    mu[:, cs.v] = 0
    seen["pass v"] = vsc.moved(cd, good4, vh.lifted_values(name, 4, mu=mu.reshape(-1)).reshape(-1))
    print("SEEN %s: %s" % (name, "  ".join("%s %.1e" % kv for kv in seen.items())))
    assert all(x >= SEEN for x in seen.values()), seen


# ---- the finite-difference yardstick of the public-interface test ------------------------------------------------------------------------------------------
def test_the_oracle_against_its_own_central_difference():
    """The float64 lifted oracle's H v against (J(z + eps v)^T mu - J(z - eps v)^T mu) / (2 eps) with the oracle's Jacobian, eps = 1e-5, order 8,
    on VL1: measured 2.78e-11 of max |H v|.  tests/test_var_large_hess_gpu.py holds the library to 10 x FD_ORACLE through pa.eval_jacobian."""
    err = vh.fd_oracle_error()
    print("the oracle's H v against its central difference: %.2e of max |H v|" % err)
    assert 0.5 * vh.FD_ORACLE <= err <= vh.FD_ORACLE


# ---- the keyword --------------------------------------------------------------------------------------------------------------------------------------------
def test_keyword_validations():
    chk = pa.integrators._check_services
    V, VE, P = L.PCL_BATCH_VARIATIONAL, L.PCL_BATCH_VARIATIONAL_EXP, L.PCL_BATCH_MEMBERS
    assert chk(V, 4, large_generator=True, large_variational=True, large_var_hessian=True) is False
    with pytest.raises(ValueError, match="large_var_hessian=True is the Hessian of the Lagrangian of a variational context created with large_generator=True: it needs that keyword"):
        chk(V, 4, large_var_hessian=True)
    with pytest.raises(ValueError, match="large_var_hessian=True is the Hessian of the Lagrangian of a large variational context .*: a plain context takes large_hessian=True"):
        chk(P, 4, large_generator=True, large_var_hessian=True)
    with pytest.raises(ValueError, match="has no large variational contexts"):
        chk(VE, "exp", large_generator=True, large_var_hessian=True)
    row = pa.integrators._BY_OPTION["large_var_hess"]
    assert (row.keyword, row.beside, row.family, row.constraint, row.sizes, row.at) == (
        "large_var_hessian", "large_generator", "variational", "pade context", "hess", "large_variational")  # fmt: skip
    assert "large_var_hess" in pa.integrators._OPTION_ORDER
    for f in (pa.integrators._PclContext.__init__, pa.integrators.HipVariationalIntegrator.__init__):
        assert inspect.signature(f).parameters["large_var_hessian"].default is False
    with pytest.raises(ValueError, match="large_var_hessian=True .* it needs that keyword"):
        pa.integrators.HipVariationalIntegrator(None, None, "x", ["xv"], "u", [None], ket=True, large_var_hessian=True)
    with pytest.raises(TypeError):  # (the plain integrator does not know the keyword)
        pa.HipPadeIntegrator(None, None, None, "x", large_var_hessian=True)
