"""GPU tests of the variational integrators (batch_mode PCL_BATCH_VARIATIONAL) on general shapes: n = 64 (every lane of a column wave, the
block role's pairs per thread exactly full), a ket, drift only (m = 0), many drives, a dense H_var outside G's pattern, components stored
out of order, a step of zero.  Every value against the lifted oracle (tests/variational_truth.py) per segment, every emitted position a
position of the truth's structure."""
import types

import numpy as np
import pytest
import scipy.sparse as sp

import piccolo_jl_amd as pa
from oracle import pade_oracle as po
from shape_cases import assert_sensitive, controlled_hermitians, lower_order
from variational_shape_cases import check_sparse_segments, hess_label, hess_plan, jac_label
from variational_truth import hessian, jacobian, make_case, residual

pytestmark = pytest.mark.gpu
TOL = 1e-11


def var_system(d, drive_mags, n_var, seed, dense_var=False):
    rng = np.random.default_rng(seed)
    H0, Hd = controlled_hermitians(d, drive_mags, rng) if drive_mags else (controlled_hermitians(d, [[0]], rng)[0], [])
    Hv = []
    for _ in range(n_var):
        if dense_var:
            A = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
            Hv.append((A + A.conj().T) / 2)
        else:
            Hv.append(controlled_hermitians(d, [], rng)[0])
    so = types.SimpleNamespace(levels=d, n_drives=len(Hd), G_drift=po.G_of_H(H0),
                               G_drives=[po.G_of_H(H) for H in Hd] if Hd else np.zeros((0, 2 * d, 2 * d)))  # fmt: skip
    return so, Hv


def var_ctx(so, case, order, ket=False, index_base=0):
    n = 2 * so.levels
    Gj = np.array(so.G_drives).reshape(so.n_drives, n, n)
    c = pa.integrators._PclContext(d=so.levels, m=so.n_drives, N=case.N, z_dim=case.z_dim, u_off=case.u_off, dt_off=case.dt_off, x_offs=case.xo,
                                   G0=np.concatenate([so.G_drift[None], np.array(case.Gv)]), Gj=Gj, batch=1 + case.v,
                                   batch_mode=pa._lib.PCL_BATCH_VARIATIONAL, per_member_G0=True, index_base=index_base, pade_order=order,
                                   state_cols=1 if ket else so.levels)  # fmt: skip
    assert c.get_option("variations") == case.v
    return c


def check_var(c, case, order, mu_seed=0, tol=TOL, hess=True, index_base=0):
    Z = case.Z.reshape(-1)
    delta, vals = c.eval_jac(Z)
    assert c.get_option("last_kernel") == 70
    ref = residual(case, order)
    assert np.abs(delta - ref).max() <= tol * np.abs(ref).max()
    J, pos = jacobian(case, order)
    rows, cols = c.jac_structure()
    rows, cols = rows - index_base, cols - index_base
    P = rows * J.shape[1] + cols
    assert len(np.unique(P)) == len(P) and np.isin(P, pos).all()
    check_sparse_segments(sp.csr_matrix((vals, (rows, cols)), shape=J.shape), J, lambda r, cc: jac_label(case, r, cc), tol)
    # the case sees a broken top term of the Jacobian (the B blocks move by >= 1e4 tol between neighbouring orders)
    Jl, _ = jacobian(case, lower_order(order))
    assert_sensitive(J.toarray() if J.shape[0] * J.shape[1] < 4e6 else J.data, Jl.toarray() if J.shape[0] * J.shape[1] < 4e6 else Jl.data, tol)
    if not hess:
        return delta, vals, None
    mu = np.random.default_rng(mu_seed).standard_normal(c.n_rows)
    H, hpos = hessian(case, order, mu)
    hv = c.hess(Z, mu)
    assert c.get_option("last_hess_kernel") == 70
    hr, hc = c.hess_structure()
    hr, hc = hr - index_base, hc - index_base
    nv = H.shape[0]
    assert np.all(hr >= hc) and len(np.unique(hr * nv + hc)) == len(hr) and np.isin(hr * nv + hc, hpos).all()
    check_sparse_segments(sp.csr_matrix((hv, (hr, hc)), shape=H.shape), H, lambda a, b: hess_label(case, a, b), tol)
    return delta, vals, hv


@pytest.mark.parametrize("order", [6, 10])
def test_v1_n64_unitary_two_variations(order):
    """d = 32 (n = 64), random sparse H, m = 2, v = 2, scales (3.0, 0.25), C = 32, one knot with Delta t = 0; work splits give the same bits."""
    so, Hv = var_system(32, [[0, 1], [2]], 2, seed=901)
    scales = (3.0, 0.25)
    case = make_case(so, [po.G_of_H(h) / s for h, s in zip(Hv, scales)], N=4, seed=31, u_scale=0.3)
    case.Z[1, case.dt_off] = 0.0
    assert np.all(np.isfinite(case.Z))
    c = var_ctx(so, case, order)
    d0, v0, h0 = check_var(c, case, order)
    for nb, ncw in ((1, 1), (3, 2), (2, 5), (7, 3)):
        c.set_option("var_block_wgs", nb)
        c.set_option("var_col_wgs", ncw)
        d1, v1 = c.eval_jac(case.Z.reshape(-1))
        assert np.array_equal(d1, d0) and np.array_equal(v1, v0), (nb, ncw)
        assert np.array_equal(c.eval(case.Z.reshape(-1)), d0)
    c.close()


def test_v2_n64_ket():
    so, Hv = var_system(32, [[0, 1], [2]], 2, seed=901)
    case = make_case(so, [po.G_of_H(h) / s for h, s in zip(Hv, (3.0, 0.25))], N=5, seed=32, ket=True, u_scale=0.3)
    c = var_ctx(so, case, 10, ket=True)
    check_var(c, case, 10)
    c.close()


@pytest.mark.parametrize("order", [2, 8])
def test_v3_drift_only(order):
    so, Hv = var_system(9, [], 1, seed=903)
    assert so.n_drives == 0
    case = make_case(so, [po.G_of_H(Hv[0])], N=4, seed=33, dt=0.3)
    c = var_ctx(so, case, order)
    check_var(c, case, order)
    c.close()


def test_v4_many_drives():
    """m = 12: delta, J and the Hessian match the truth.  The launch code's arithmetic (restated in tests/variational_shape_cases.py) serves this
    shape at order 10 with one wave per workgroup in 98,600 B of LDS: a refusal is a failure."""
    so, Hv = var_system(9, [[g % 5] for g in range(12)], 2, seed=904)
    case = make_case(so, [po.G_of_H(h) / 2 for h in Hv], N=4, seed=34, dt=0.15, u_scale=0.3)
    plan = hess_plan(case.n, case.C, case.m, case.v, 10)
    assert (case.n, case.C, case.m, case.v) == (18, 9, 12, 2) and plan["served"] and plan["w"] == 1 and plan["bytes"] == 98600
    c = var_ctx(so, case, 10)
    check_var(c, case, 10)
    c.close()


def test_v5_dense_variation_outside_the_pattern():
    so, Hv = var_system(12, [[0]], 1, seed=905, dense_var=True)
    case = make_case(so, [po.G_of_H(Hv[0]) / 4], N=4, seed=35, dt=0.2, u_scale=0.3)
    c = var_ctx(so, case, 8)
    check_var(c, case, 8)
    c.close()


@pytest.mark.parametrize("index_base", [0, 1])
def test_v6_components_out_of_order(index_base):
    """Knot [u, Delta t, t, U_var2, U, U_var1]: the x_offs do not increase."""
    so, Hv = var_system(9, [[0], [1, 2]], 2, seed=906)
    m, n, d = 2, 18, 9
    xdc = n * d
    xo = [m + 2 + xdc, m + 2 + 2 * xdc, m + 2]
    case = make_case(so, [po.G_of_H(h) / 2 for h in Hv], N=10, seed=36, dt=0.2, u_scale=0.3, xo=xo, u_off=0, dt_off=m, t_off=m + 1,
                     z_dim=m + 2 + 3 * xdc)  # fmt: skip
    c = var_ctx(so, case, 10, index_base=index_base)
    check_var(c, case, 10, index_base=index_base)
    c.close()
