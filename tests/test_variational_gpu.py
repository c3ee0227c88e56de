"""GPU tests of the variational (sensitivity) integrators (batch_mode PCL_BATCH_VARIATIONAL): every value against the lifted oracle
computation (tests/variational_truth.py), the reference's own test item rebuilt in Python, consistency with the plain integrator, a
finite-difference check of the Jacobian, bitwise equality of paths and work splits, the order policy on the lifted generator, refusals."""
import numpy as np
import pytest
import scipy.sparse as sp

import piccolo_jl_amd as pa
from oracle import pade_oracle as po
from variational_truth import VarCase, h_var_drift, hessian, jacobian, lifted, make_case, residual

pytestmark = pytest.mark.gpu
P = po.PAULIS


def _traj(case, ket=False):
    """Product-side NamedTrajectory over the case's knots: components x, x_var1.., dt, t, u."""
    comps = {}
    names = ["ψ̃" if ket else "Ũ⃗"] + [("ψ̃_var%d" if ket else "Ũ⃗_var%d") % (i + 1) for i in range(case.v)]
    for nm, o in zip(names, case.xo):
        comps[nm] = case.Z[:, o : o + case.xdc].T
    comps["Δt"] = case.Z[:, case.dt_off][None]
    comps["t"] = case.Z[:, case.dt_off + 1][None]
    comps["u"] = case.Z[:, case.u_off : case.u_off + case.m].T
    t = pa.NamedTrajectory(comps, controls=("u", "Δt"), timestep="Δt")
    assert np.array_equal(t.datavec, case.Z.reshape(-1))
    return t, names


def _vsys(sys_o, H_vars):
    return pa.VariationalQuantumSystem(sys_o.H_drift, list(sys_o.H_drives), H_vars, [1.0] * sys_o.n_drives)


def _integrator(sys_o, case, H_vars, scales, ket=False, **kw):
    traj, names = _traj(case, ket)
    vs = _vsys(sys_o, H_vars)
    if ket:
        B = pa.VariationalKetIntegrator(vs, traj, names[0], names[1:], "u", scale=scales, **kw)
    else:
        B = pa.VariationalUnitaryIntegrator(vs, traj, names[0], names[1:], "u", scales=scales, **kw)
    return B, traj


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


def _check_all(B, case, order, tol=1e-11):
    Z = case.Z.reshape(-1)
    delta, vals = B.ctx.eval_jac(Z)
    assert _rel(delta, residual(case, order)) < tol
    J, pos = jacobian(case, order)
    rows, cols = B.ctx.jac_structure()
    ours = sp.csr_matrix((vals, (rows, cols)), shape=J.shape)
    assert len(np.unique(rows * J.shape[1] + cols)) == len(rows)  # no position twice
    assert np.isin(rows * J.shape[1] + cols, pos).all()  # every emitted position is a position of the lifted structure
    D = (ours - J).tocoo()
    assert (np.abs(D.data).max() if D.nnz else 0.0) <= tol * np.abs(J.data).max()
    mu = np.random.default_rng(order).standard_normal(B.dim)
    H, hpos = hessian(case, order, mu)
    hv = B.ctx.hess(Z, mu)
    hr, hc = B.ctx.hess_structure()
    nv = H.shape[0]
    assert np.all(hr >= hc) and len(np.unique(hr * nv + hc)) == len(hr)
    assert np.isin(hr * nv + hc, hpos).all()
    Dh = (sp.csr_matrix((hv, (hr, hc)), shape=H.shape) - H).tocoo()
    assert (np.abs(Dh.data).max() if Dh.nnz else 0.0) <= tol * np.abs(H.data).max()
    return delta, vals


# ---- the reference's test item, in Python ------------------------------------------------------------------------------------------------
def test_reference_item_pauli():
    """[REF src/control/integrators.jl "VariationalKetIntegrator / VariationalUnitaryIntegrator construct and integrate"]"""
    sysv = pa.VariationalQuantumSystem(pa.PAULIS["Z"] / 2, [pa.PAULIS["X"], pa.PAULIS["Y"]], [pa.PAULIS["Z"] / 2], [1.0, 1.0])
    N = 5
    psi = np.zeros((4, N))
    psi[:, 0] = [1.0, 0, 0, 0]
    traj = pa.NamedTrajectory({"ψ̃": psi, "ψ̃_var": np.zeros((4, N)), "u": np.zeros((2, N)), "Δt": np.full((1, N), 0.1)},
                              controls=("u", "Δt"), timestep="Δt")  # fmt: skip
    U = np.zeros((8, N))
    U[:, 0] = pa.operator_to_iso_vec(np.eye(2))
    traj_U = pa.NamedTrajectory({"Ũ⃗": U, "Ũ⃗_var": np.zeros((8, N)), "u": np.zeros((2, N)), "Δt": np.full((1, N), 0.1)},
                                controls=("u", "Δt"), timestep="Δt")  # fmt: skip
    for ctor, t, names, xd in ((pa.VariationalKetIntegrator, traj, ["ψ̃", "ψ̃_var"], 8), (pa.VariationalUnitaryIntegrator, traj_U, ["Ũ⃗", "Ũ⃗_var"], 16)):
        B = ctor(sysv, t, names[0], names[1:], "u", pade_order=10)
        assert B.x_names == names and B.x_dim == xd and B.dim == xd * (N - 1)
        delta = np.zeros(B.dim)
        pa.evaluate_(delta, B, t)
        assert np.all(np.isfinite(delta)) and np.linalg.norm(delta) > 0
        # the exp constraint: on the exactly propagated trajectory (x_{k+1} = exp(h Ghat) x_k from the same knot 0) the order-10 residual
        # stays within 1e-10 of the exp constraint's, which is zero there
        Z = t.datavec.reshape(N, -1).copy()
        cols = 1 if xd == 8 else 2
        case = VarCase(Z=Z, z_dim=Z.shape[1], N=N, n=4, C=cols, m=2, xo=[t.components[nm].start for nm in names], u_off=t.components["u"].start,
                       dt_off=t.components["Δt"].start, G0=sysv.G_drift, Gv=[sysv.G_vars_array()[0]], Gj=sysv.G_drives_array())  # fmt: skip
        Zl, lay, G0l, Gjl = lifted(case)
        X = po.exact_rollout(Zl, lay, G0l, Gjl)  # [N, C n'] lifted order
        Ze = Z.copy()
        for k in range(N):
            S = X[k].reshape(cols, 2, 4)
            for b in range(2):
                Ze[k, case.xo[b] : case.xo[b] + case.xdc] = S[:, b, :].reshape(-1)
        assert np.abs(po.exp_residual(lifted(VarCase(**{**case.__dict__, "Z": Ze}))[0], lay, G0l, Gjl)).max() < 1e-13
        de = B.ctx.eval(Ze.reshape(-1))
        assert np.abs(de).max() < 1e-10
        assert np.abs(delta - residual(case, 10)).max() < 1e-13
        B.close()


def _config3_case(nv, N=4, seed=11, ket=False):
    s3 = po.config_system(3)
    Hv = [h_var_drift(3, 3), po.lift_operator(po.annihilate(3) + po.annihilate(3).conj().T, 2, [3, 3, 3])][:nv]
    scales = np.full(nv, 10.0)
    case = make_case(s3, [po.G_of_H(h) / s for h, s in zip(Hv, scales)], N=N, seed=seed, ket=ket)
    return s3, Hv, scales, case


@pytest.mark.parametrize("nv", [1, 2])
@pytest.mark.parametrize("order", [2, 4, 6, 8, 10])
def test_config3_unitary_values(nv, order):
    s3, Hv, scales, case = _config3_case(nv)
    B, traj = _integrator(s3, case, Hv, scales, pade_order=order)
    assert B.ctx.get_option("variations") == nv
    _check_all(B, case, order)
    assert B.ctx.get_option("last_kernel") == 70 and B.ctx.get_option("last_hess_kernel") == 70
    B.close()


@pytest.mark.parametrize("order", [2, 4, 6, 8, 10])
def test_d25_m4_values(order):
    s = po.multi_transmon_system([4.0, 4.1], [0.2, 0.21], [[0, 0.01], [0.01, 0]], levels_per_transmon=5, drive_bounds=0.1)
    assert s.levels == 25 and s.n_drives == 4
    Hv = [h_var_drift(5, 2)]
    case = make_case(s, [po.G_of_H(Hv[0]) / 10], N=4, seed=2)
    B, _ = _integrator(s, case, Hv, [10.0], pade_order=order)
    _check_all(B, case, order)
    B.close()


@pytest.mark.parametrize("nv", [1, 2])
@pytest.mark.parametrize("order", [2, 4, 6, 8, 10])
def test_config3_ket_values(nv, order):
    s3, Hv, scales, case = _config3_case(nv, ket=True, N=6)
    B, _ = _integrator(s3, case, Hv, 10.0, ket=True, pade_order=order)
    assert B.x_dim == (nv + 1) * 54
    _check_all(B, case, order)
    B.close()


# ---- consistency ----------------------------------------------------------------------------------------------------------------------------
def test_nominal_rows_equal_plain_context():
    s3, Hv, scales, case = _config3_case(1)
    B, traj = _integrator(s3, case, Hv, scales, pade_order=4)
    delta, vals = B.ctx.eval_jac(case.Z.reshape(-1))
    plain = pa.HipPadeIntegrator(s3.G_drift, np.array(s3.G_drives), traj, "Ũ⃗", "u", pade_order=4)
    plain.ctx.set_option("host_path", 1)
    dp, vp = plain.ctx.eval_jac(case.Z.reshape(-1))
    K, xd, xdc = case.K, B.x_dim, case.xdc
    assert np.abs(delta.reshape(K, xd)[:, :xdc] - dp.reshape(K, xdc)).max() <= 1e-13 * np.abs(dp).max()
    nb = 2 * case.C * case.n**2  # -B+ and B- of delta_0 are the plain blocks
    bv = vals.reshape(K, -1)[:, :nb]
    assert np.abs(bv - vp.reshape(K, -1)[:, :nb]).max() <= 1e-13 * np.abs(vp).max()
    B.close()
    plain.close()


def test_zero_variation_generator_gives_plain_residual_of_variations():
    s3 = po.config_system(3)
    n = 54
    case = make_case(s3, [np.zeros((n, n)), np.zeros((n, n))], N=4, seed=4)
    vs = pa.VariationalQuantumSystem(s3.H_drift, list(s3.H_drives), [0 * s3.H_drift, 0 * s3.H_drift], [1.0] * 6)
    traj, names = _traj(case)
    B = pa.VariationalUnitaryIntegrator(vs, traj, names[0], names[1:], "u", pade_order=6)
    delta = B.ctx.eval(case.Z.reshape(-1)).reshape(case.K, 3, case.xdc)
    for b in range(3):
        plain = pa.HipPadeIntegrator(s3.G_drift, np.array(s3.G_drives), traj, names[b], "u", pade_order=6)
        dp = plain.ctx.eval(case.Z.reshape(-1)).reshape(case.K, case.xdc)
        assert np.abs(delta[:, b] - dp).max() <= 1e-13 * max(np.abs(dp).max(), 1e-12)
        plain.close()
    B.close()


def test_jacobian_against_central_differences():
    """The check the reference's ForwardDiff Jacobian of this construction fails (its #307)."""
    s = po.config_system(2)
    Hv = [h_var_drift(2, 2), np.kron(P["X"], P["I"]).astype(complex)]
    case = make_case(s, [po.G_of_H(h) / 5 for h in Hv], N=4, seed=9, dt=0.3, u_scale=0.05)
    B, traj = _integrator(s, case, Hv, [5.0, 5.0], pade_order=4)
    Z = case.Z.reshape(-1).copy()
    delta, vals = B.ctx.eval_jac(Z)
    rows, cols = B.ctx.jac_structure()
    J = sp.csr_matrix((vals, (rows, cols)), shape=(B.dim, Z.size)).toarray()
    eps = 1e-6
    F = np.empty_like(J)
    for j in range(Z.size):
        zp, zm = Z.copy(), Z.copy()
        zp[j] += eps
        zm[j] -= eps
        F[:, j] = (B.ctx.eval(zp) - B.ctx.eval(zm)) / (2 * eps)
    assert np.abs(F - J).max() <= 1e-6 * max(1.0, np.abs(J).max())
    B.close()


# ---- paths and splits ---------------------------------------------------------------------------------------------------------------------------
def test_host_device_and_splits_bitwise():
    import torch

    s3, Hv, scales, case = _config3_case(2, N=5)
    B, _ = _integrator(s3, case, Hv, scales, pade_order=6)
    c = B.ctx
    Z = case.Z.reshape(-1)
    d0, v0 = c.eval_jac(Z)
    mu = np.random.default_rng(0).standard_normal(B.dim)
    h0 = c.hess(Z, mu)
    Zd = torch.from_numpy(Z).cuda()
    dd = torch.empty(c.n_rows, dtype=torch.float64, device="cuda")
    vd = torch.empty(c.jac_nnz, dtype=torch.float64, device="cuda")
    hd = torch.empty(c.hess_nnz, dtype=torch.float64, device="cuda")
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    c.eval_jac_dev(Zd, dd, vd)
    c.hess_dev(Zd, torch.from_numpy(mu).cuda(), hd)
    c.sync()
    assert np.array_equal(dd.cpu().numpy(), d0) and np.array_equal(vd.cpu().numpy(), v0) and np.array_equal(hd.cpu().numpy(), h0)
    vd2 = torch.zeros_like(vd)
    c.jac_dev(Zd, vd2)
    dd2 = torch.zeros_like(dd)
    c.eval_dev(Zd, dd2)
    c.sync()
    assert np.array_equal(vd2.cpu().numpy(), v0) and np.array_equal(dd2.cpu().numpy(), d0)
    c.set_stream(None)
    for nb, ncw in ((1, 1), (3, 2), (27, 4), (5, 27), (2, 7)):
        c.set_option("var_block_wgs", nb)
        c.set_option("var_col_wgs", ncw)
        d1, v1 = c.eval_jac(Z)
        assert np.array_equal(d1, d0) and np.array_equal(v1, v0), (nb, ncw)
        assert np.array_equal(c.eval(Z), d0)
    B.close()


# ---- order policy ------------------------------------------------------------------------------------------------------------------------------------
def test_order_policy_on_lifted_generator():
    s3 = po.config_system(3)
    Hv = [h_var_drift(3, 3)]
    for scale, met in ((10.0, True), (1.0, False)):
        case = make_case(s3, [po.G_of_H(Hv[0]) / scale], N=3, seed=1)
        B, traj = _integrator(s3, case, Hv, [scale], pade_order=4)
        order = B.ctx.set_order_policy(0.1, np.full(6, 0.1))
        assert B.ctx.order_tol_met == met
        if met:
            assert order == 10
        plain = pa.HipPadeIntegrator(s3.G_drift, np.array(s3.G_drives), traj, "Ũ⃗", "u", pade_order=4)
        assert order >= plain.ctx.set_order_policy(0.1, np.full(6, 0.1))
        o2 = B.ctx.set_order_from_trajectory(case.Z.reshape(-1))
        assert o2 >= plain.ctx.set_order_from_trajectory(case.Z.reshape(-1))
        plain.close()
        B.close()
    # pade_order = 0 at construction: decided over the trajectory, never below the plain system's
    case = make_case(s3, [po.G_of_H(Hv[0]) / 10], N=3, seed=1)
    B, _ = _integrator(s3, case, Hv, [10.0])
    assert B.pade_order in (2, 4, 6, 8, 10)
    B.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    import ctypes

    import torch

    s = po.config_system(2)
    Hv = [h_var_drift(2, 2)]
    case = make_case(s, [po.G_of_H(Hv[0])], N=3, seed=0)
    B, _ = _integrator(s, case, Hv, [1.0], pade_order=4)
    c = B.ctx
    L, h = c._L, c._h
    E = pa._lib.PCL_ENOTIMPL
    Z = case.Z.reshape(-1)
    Zd = torch.from_numpy(Z).cuda()
    buf = torch.zeros(max(c.jac_nnz, 16), dtype=torch.float64, device="cuda")
    i64 = ctypes.c_int64()
    vp = ctypes.c_void_p
    assert L.pcl_set_member_window(h, 0, 1) == E
    assert L.pcl_jac_compact_nnz(h, ctypes.byref(i64), ctypes.byref(i64)) == E
    assert L.pcl_rollout(h, vp(Z.ctypes.data), vp(buf.data_ptr())) == E
    assert L.pcl_rollout_dev(h, vp(Zd.data_ptr()), vp(buf.data_ptr())) == E
    assert L.pcl_eval_jac_compact_dev(h, vp(Zd.data_ptr()), vp(buf.data_ptr()), vp(buf.data_ptr())) == E
    assert L.pcl_jac_expand_dev(h, vp(buf.data_ptr()), vp(buf.data_ptr())) == E
    assert L.pcl_set_goal(h, vp(buf.data_ptr())) == E
    assert L.pcl_set_weights(h, None) == E
    assert L.pcl_merit_grad_len(h, ctypes.byref(i64), ctypes.byref(i64)) == E
    assert L.pcl_objective_hess_nnz(h, ctypes.byref(i64)) == E
    assert L.pcl_clear_regularizers(h) == E
    assert L.pcl_reduce_sum_dev(h, vp(buf.data_ptr()), ctypes.c_int64(4)) == E
    assert b"variational" in L.pcl_last_error(h)
    with pytest.raises(pa.PclError) as ei:
        c.eval_jac_merit_dev(Zd, None, buf, buf, buf)
    assert ei.value.code == E
    # derivative rows: as for a one-trajectory context
    assert c.deriv_dims(case.u_off, case.m) == (case.K * case.m, 4 * case.K * case.m)
    dlt, _ = c.deriv_eval_jac(case.dt_off + 1, -1, 1, Z)  # time consistency t_{k+1} - t_k - dt_k
    assert np.allclose(dlt, case.Z[1:, case.dt_off + 1] - case.Z[:-1, case.dt_off + 1] - case.Z[:-1, case.dt_off], atol=1e-15)
    B.close()
    # more variations than the kernels take
    Hv3 = [h_var_drift(2, 2)] * 3
    case3 = make_case(s, [po.G_of_H(g) for g in Hv3], N=3, seed=0)
    with pytest.raises(pa.PclError) as ei:
        _integrator(s, case3, Hv3, [1.0, 1.0, 1.0], pade_order=4)
    assert ei.value.code == pa._lib.PCL_ESHAPE
