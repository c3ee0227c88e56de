"""GPU tests of the variational integrators on the exponential constraint (batch_mode PCL_BATCH_VARIATIONAL_EXP): every delta and Jacobian
value against the lifted scipy truth (tests/var_exp_truth.py) at 1e-11, the special steps, consistency with a plain exponential context, the
context's own rollout, a finite-difference check on the device, bitwise equality of paths, the objective side against a Pade variational
context, refusals, and the Python constructors end to end."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import piccolo_jl_amd as pa
import var_exp_cases as cases
import var_exp_truth as truth
from oracle import pade_oracle as po
from test_parity_gpu import close

pytestmark = pytest.mark.gpu
EXP, VEXP = pa._lib.PCL_ORDER_EXP, pa._lib.PCL_BATCH_VARIATIONAL_EXP
E_INVAL, E_SHAPE, E_NOTIMPL = pa._lib.PCL_EINVAL, pa._lib.PCL_ESHAPE, pa._lib.PCL_ENOTIMPL


def vexp_ctx(case, batch_mode=VEXP, pade_order=EXP, index_base=0):
    c = pa.integrators._PclContext(d=case.n // 2, m=case.m, N=case.N, z_dim=case.z_dim, u_off=case.u_off, dt_off=case.dt_off, x_offs=case.xo,
                                   G0=np.concatenate([case.G0[None], np.array(case.Gv)]), Gj=case.Gj, batch=1 + case.v, batch_mode=batch_mode,
                                   per_member_G0=True, index_base=index_base, pade_order=pade_order, state_cols=case.C)  # fmt: skip
    assert c.get_option("variations") == case.v
    return c


def check_values(case, index_base=0):
    """Host-pointer delta and values against the truth at 1e-11, the structure against the documented one; returns (context, delta, values)."""
    c = vexp_ctx(case, index_base=index_base)
    assert c.get_option("pade_order") == -1
    assert c.x_dim == case.xd and c.n_rows == case.K * case.xd
    assert c.jac_per == truth.nnz_per_interval(case) and c.jac_nnz == case.K * c.jac_per
    Z = case.Z.reshape(-1)
    delta, vals = c.eval_jac(Z)
    assert c.get_option("last_kernel") == 110
    r, cc = c.jac_structure()
    tr, tc = truth.structure(case, index_base)
    assert np.array_equal(r, tr) and np.array_equal(cc, tc)
    r32, c32 = c.jac_structure(np.int32)
    assert np.array_equal(r32, tr) and np.array_equal(c32, tc)
    ed = close(delta, truth.residual(case), 1e-11)
    ev = close(vals, truth.values(case), 1e-11)
    print("delta %.2e  values %.2e" % (ed, ev))
    return c, delta, vals


# ---- shapes ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ket", [True, False])
def test_pauli_item(ket):
    check_values(cases.pauli(ket)[3])[0].close()


@pytest.mark.parametrize("nv", [1, 2])
def test_config2(nv):
    check_values(cases.config2(nv)[3])[0].close()


@pytest.mark.parametrize("nv", [1, 2])
def test_config3(nv):
    check_values(cases.config3(nv)[3])[0].close()


def test_d25_m4():
    check_values(cases.d25()[3])[0].close()


def test_config3_ket():
    check_values(cases.config3(2, ket=True)[3])[0].close()


def _no_drives(case):
    """The same knots read as a drift-only problem (the drive slots become idle variables)."""
    return dataclasses.replace(case, m=0, Gj=np.zeros((0, case.n, case.n)))


@pytest.mark.parametrize("ket", [True, False])
def test_no_drives(ket):
    check_values(_no_drives(cases.config2(2, ket=ket)[3]))[0].close()


def test_index_base_1():
    check_values(cases.config2(2, N=5)[3], index_base=1)[0].close()


def test_largest_served_n62_and_first_refused_n64():
    """d = 31 (n = 62, LD = 66): five tiles of 32 736 B, 163 680 of 163 840 B, G(u_k) read from the workspace.  d = 32: 168 960 B, refused by
    pcl_create with the byte counts."""
    check_values(cases.transmon(31)[3])[0].close()
    check_values(cases.transmon(31, ket=True)[3])[0].close()
    with pytest.raises(pa.PclError) as ei:
        vexp_ctx(cases.transmon(32, N=3)[3])
    assert ei.value.code == E_SHAPE
    msg = str(ei.value)
    assert "168960" in msg and "163840" in msg and "33792" in msg and "PCL_BATCH_VARIATIONAL_EXP" in msg


# ---- steps -----------------------------------------------------------------------------------------------------------------------------------
def test_zero_step():
    """dt = 0: the copies of E are exactly -I, L_i and L2 exactly 0, and component i's dt tail is -(Gv_i X + G Xv_i)."""
    _, _, _, case = cases.config2(2, N=4)
    case.Z[:, case.dt_off] = 0.0
    c, delta, vals = check_values(case)
    n, C, v, m, xdc = case.n, case.C, case.v, case.m, case.xdc
    per = c.jac_per
    V = vals.reshape(case.K, per)
    nb = C * n * n
    mI = np.tile(-np.eye(n).reshape(-1), C)
    for k in range(case.K):
        assert np.array_equal(V[k, :nb], mI)
        for i in range(1, v + 1):
            assert np.array_equal(V[k, (2 * i - 1) * nb : 2 * i * nb], mI)
            assert not V[k, 2 * i * nb : (2 * i + 1) * nb].any()
        tails = V[k, (1 + 2 * v) * nb + case.xd :].reshape(v + 1, C, m + 1, n)
        assert not tails[:, :, :m, :].any()
        z = case.Z[k]
        G = case.G0 + np.tensordot(z[case.u_off : case.u_off + m], case.Gj, axes=1)
        X = z[case.xo[0] : case.xo[0] + xdc].reshape(C, n).T
        close(tails[0, :, m, :], -(G @ X).T, 1e-13)
        for i in range(1, v + 1):
            Xv = z[case.xo[i] : case.xo[i] + xdc].reshape(C, n).T
            close(tails[i, :, m, :], -(case.Gv[i - 1] @ X + G @ Xv).T, 1e-13)
    c.close()


def test_negative_step():
    _, _, _, case = cases.config2(2, N=4)
    case.Z[:, case.dt_off] *= -1.0
    check_values(case)[0].close()
    _, _, _, case = cases.config3(1, N=3)
    case.Z[:, case.dt_off] *= -2.5
    check_values(case)[0].close()


@pytest.mark.parametrize("which", ["config2_dt4", "config3_dt1"])
def test_large_steps(which):
    """Several squarings: where a dropped cross term of the Tw squaring shows."""
    case = cases.config2(2, dt=4.0)[3] if which == "config2_dt4" else cases.config3(1, N=3, dt=1.0)[3]
    check_values(case)[0].close()


# ---- consistency -----------------------------------------------------------------------------------------------------------------------------
def test_zero_variation_generator_equals_a_plain_exponential_context():
    """Gv_i = 0: the -L_i block and the L2 contribution are exactly zero, and the rows of component i are a plain exponential context's on Xv_i."""
    _, _, _, case = cases.config2(1, N=4, dt=0.6)
    case = dataclasses.replace(case, Gv=[np.zeros_like(case.G0)])
    c, delta, vals = check_values(case)
    n, C, m, xdc = case.n, case.C, case.m, case.xdc
    nb = C * n * n
    V = vals.reshape(case.K, -1)
    assert not V[:, 2 * nb : 3 * nb].any()
    plain = pa.integrators._PclContext(d=n // 2, m=m, N=case.N, z_dim=case.z_dim, u_off=case.u_off, dt_off=case.dt_off, x_offs=[case.xo[1]], G0=case.G0,
                                       Gj=case.Gj, batch=1, batch_mode=pa._lib.PCL_BATCH_MEMBERS, pade_order=EXP, state_cols=C)  # fmt: skip
    pd, pv = plain.eval_jac(case.Z.reshape(-1))
    PV = pv.reshape(case.K, -1)
    close(delta.reshape(case.K, 2, xdc)[:, 1], pd.reshape(case.K, xdc), 1e-13)
    close(V[:, nb : 2 * nb], PV[:, :nb], 1e-13)
    tails = V[:, 3 * nb + 2 * xdc :].reshape(case.K, 2, C * (m + 1) * n)
    close(tails[:, 1], PV[:, nb + xdc :], 1e-13)
    plain.close()
    c.close()


@pytest.mark.parametrize("which", ["config2", "config3"])
def test_own_rollout_satisfies_the_constraint(which):
    """With var_full, the trajectory of the context's own pcl_rollout has |delta| <= 1e-12 max|X| over all components (N = 20)."""
    case = cases.config2(2, N=20, dt=0.3)[3] if which == "config2" else cases.config3(1, N=20)[3]
    c = vexp_ctx(case)
    c.set_option("var_full", 1)
    X = c.rollout(case.Z.reshape(-1))[0]  # [N, x_dim']
    Z = case.Z.copy()
    for b, o in enumerate(case.xo):
        Z[:, o : o + case.xdc] = X[:, b * case.xdc : (b + 1) * case.xdc]
    delta = c.eval(Z.reshape(-1))
    assert np.abs(delta).max() <= 1e-12 * np.abs(X).max(), np.abs(delta).max()
    c.close()


def test_jacobian_times_direction_against_differences_on_the_device():
    _, _, _, case = cases.config2(2, N=5, dt=0.4)
    c = vexp_ctx(case)
    c.set_stream(torch.cuda.current_stream().cuda_stream)  # the launches follow torch's own work on the perturbed points
    Z = torch.from_numpy(case.Z.reshape(-1).copy()).cuda()
    vals = torch.empty(c.jac_nnz, dtype=torch.float64, device="cuda")
    c.jac_dev(Z, vals)
    c.sync()
    r, cc = c.jac_structure()
    import scipy.sparse as sp

    J = sp.csr_matrix((vals.cpu().numpy(), (r, cc)), shape=(c.n_rows, c.n_cols))
    rng = np.random.default_rng(5)
    step = 1e-6
    for _ in range(3):
        w = rng.standard_normal(c.n_cols)
        wd = torch.from_numpy(w).cuda()
        dp, dm = torch.empty(c.n_rows, dtype=torch.float64, device="cuda"), torch.empty(c.n_rows, dtype=torch.float64, device="cuda")
        Zp, Zm = Z + step * wd, Z - step * wd
        c.eval_dev(Zp, dp)
        c.eval_dev(Zm, dm)
        c.sync()
        fd = ((dp - dm) / (2 * step)).cpu().numpy()
        err = np.abs(J @ w - fd).max()
        print("max|J w - fd| %.3e  max|fd| %.3e" % (err, np.abs(fd).max()))
        assert err <= 1e-6 * max(1.0, np.abs(fd).max())
    assert c.get_option("last_kernel") == 111
    c.close()


@pytest.mark.parametrize("which", ["config2_v2", "config3_v1", "pauli_ket"])
def test_bitwise_paths(which):
    """Fused delta = residual-only delta; host-pointer = device-pointer; launch = launch."""
    case = {"config2_v2": lambda: cases.config2(2, dt=0.7), "config3_v1": lambda: cases.config3(1), "pauli_ket": lambda: cases.pauli(True)}[which]()[3]
    c = vexp_ctx(case)
    Zh = case.Z.reshape(-1)
    hd, hv = c.eval_jac(Zh)
    assert c.get_option("last_kernel") == 110
    he = c.eval(Zh)
    assert c.get_option("last_kernel") == 111
    hj = c.jac(Zh)
    assert np.array_equal(hd, he) and np.array_equal(hv, hj)
    Z = torch.from_numpy(Zh.copy()).cuda()
    c.set_stream(torch.cuda.current_stream().cuda_stream)  # after torch's NaN fills of the outputs
    outs = []
    for _ in range(2):
        d1 = torch.full((c.n_rows,), np.nan, dtype=torch.float64, device="cuda")
        d2 = torch.full((c.n_rows,), np.nan, dtype=torch.float64, device="cuda")
        v1 = torch.full((c.jac_nnz,), np.nan, dtype=torch.float64, device="cuda")
        v2 = torch.full((c.jac_nnz,), np.nan, dtype=torch.float64, device="cuda")
        c.eval_jac_dev(Z, d1, v1)
        c.eval_dev(Z, d2)
        c.jac_dev(Z, v2)
        c.sync()
        outs.append((d1.cpu().numpy(), v1.cpu().numpy()))
        assert np.array_equal(outs[-1][0], d2.cpu().numpy()) and np.array_equal(outs[-1][1], v2.cpu().numpy())
        assert np.array_equal(outs[-1][0], hd) and np.array_equal(outs[-1][1], hv)
    c.set_stream(None)
    c.set_option("var_block_wgs", 3)  # no effect on this context
    c.set_option("var_col_wgs", 2)
    d3, v3 = c.eval_jac(Zh)
    assert np.array_equal(d3, hd) and np.array_equal(v3, hv)
    c.close()


def test_objective_side_has_the_bits_of_a_pade_variational_context():
    _, _, _, case = cases.config2(2, N=6, dt=0.3)
    rng = np.random.default_rng(9)
    goal = po.operator_to_iso_vec(np.linalg.qr(rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4)))[0])
    Z = case.Z.reshape(-1)
    got = []
    for mode, order in ((VEXP, EXP), (pa._lib.PCL_BATCH_VARIATIONAL, 4)):
        c = vexp_ctx(case, batch_mode=mode, pade_order=order)
        with pytest.raises(pa.PclError) as ei:  # refused until the option is on
            c.rollout(Z)
        assert ei.value.code == E_NOTIMPL
        c.set_option("var_full", 1)
        c.set_goal(goal)
        c.set_weights([1.0, 0.3, 0.2])
        c.add_regularizer(case.u_off, case.m, 0.1, 2)
        val, grad = c.objective(Z, 100.0)
        hr, hc = c.objective_hess_structure()
        hv = c.objective_hess(Z, 100.0, 0.7)
        got.append((val, grad, hr, hc, hv, c.rollout(Z)))
        c.close()
    for a, b in zip(*got):
        assert np.array_equal(a, b)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable():
    _, _, _, case = cases.config2(1, N=4)
    c = vexp_ctx(case)
    Zh = case.Z.reshape(-1)
    want = c.eval(Zh)
    L, h = c._L, c._h
    Z = torch.from_numpy(Zh.copy()).cuda()
    big = torch.zeros(max(c.jac_nnz, c.n_rows, 64), dtype=torch.float64, device="cuda")
    out = torch.zeros_like(big)
    hb = np.zeros(c.n_rows)
    a, b = ctypes.c_int64(), ctypes.c_int64()
    idx = np.zeros(16, dtype=np.int64)
    i32p, i64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    L.pcl_set_order_policy.argtypes = [ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p, ctypes.c_double, ctypes.POINTER(ctypes.c_int32)]
    L.pcl_set_order_from_trajectory.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.POINTER(ctypes.c_int32)]
    um = np.ones(case.m)
    o32 = ctypes.c_int32()
    hess_words = ("third Frechet", "quasi-Newton")
    calls = [
        ("pcl_hess", lambda: L.pcl_hess(h, Zh.ctypes.data, hb.ctypes.data, hb.ctypes.data), E_NOTIMPL, hess_words),
        ("pcl_hess_dev", lambda: L.pcl_hess_dev(h, Z.data_ptr(), big.data_ptr(), out.data_ptr()), E_NOTIMPL, hess_words),
        ("pcl_hess_nnz", lambda: L.pcl_hess_nnz(h, ctypes.byref(a), ctypes.byref(b)), E_NOTIMPL, hess_words),
        ("pcl_hess_structure", lambda: L.pcl_hess_structure(h, idx.ctypes.data_as(i32p), idx.ctypes.data_as(i32p)), E_NOTIMPL, hess_words),
        ("pcl_hess_structure_i64", lambda: L.pcl_hess_structure_i64(h, idx.ctypes.data_as(i64p), idx.ctypes.data_as(i64p)), E_NOTIMPL, hess_words),
        ("exp_hess", lambda: L.pcl_set_option(h, b"exp_hess", 1), E_NOTIMPL, hess_words),
        ("pcl_jac_compact_nnz", lambda: L.pcl_jac_compact_nnz(h, ctypes.byref(a), ctypes.byref(b)), E_NOTIMPL, ()),
        ("pcl_eval_jac_compact_dev", lambda: L.pcl_eval_jac_compact_dev(h, Z.data_ptr(), big.data_ptr(), out.data_ptr()), E_NOTIMPL, ()),
        ("pcl_jac_expand_dev", lambda: L.pcl_jac_expand_dev(h, big.data_ptr(), out.data_ptr()), E_NOTIMPL, ()),
        ("pcl_merit_grad_len", lambda: L.pcl_merit_grad_len(h, ctypes.byref(a), ctypes.byref(b)), E_NOTIMPL, ()),
        ("pcl_merit_grad_dev", lambda: L.pcl_merit_grad_dev(h, big.data_ptr(), None, big.data_ptr(), out.data_ptr()), E_NOTIMPL, ()),
        ("pcl_eval_jac_merit_dev", lambda: L.pcl_eval_jac_merit_dev(h, Z.data_ptr(), None, big.data_ptr(), big.data_ptr(), out.data_ptr()), E_NOTIMPL, ()),
        ("pcl_reduce_sum_dev", lambda: L.pcl_reduce_sum_dev(h, big.data_ptr(), 4), E_NOTIMPL, ()),
        ("pcl_set_member_window", lambda: L.pcl_set_member_window(h, 0, 1), E_NOTIMPL, ()),
        ("pcl_infidelity_dev", lambda: L.pcl_infidelity_dev(h, Z.data_ptr(), 1.0, out.data_ptr(), None), E_NOTIMPL, ()),
        ("pcl_set_order_policy", lambda: L.pcl_set_order_policy(h, 0.1, um.ctypes.data, 1e-10, ctypes.byref(o32)), E_INVAL, ("no order to choose",)),
        ("pcl_set_order_from_trajectory", lambda: L.pcl_set_order_from_trajectory(h, Zh.ctypes.data, 1e-10, ctypes.byref(o32)), E_INVAL, ("no order to choose",)),
    ]  # fmt: skip
    for on in (0, 1):  # the refusals do not depend on var_full
        c.set_option("var_full", on)
        for name, call, code, words in calls:
            rc = call()
            msg = L.pcl_last_error(h).decode()
            assert rc == code, (name, rc, msg)
            if code == E_NOTIMPL:
                assert "PCL_BATCH_VARIATIONAL_EXP" in msg and "is not implemented" in msg, (name, msg)
            for w in words:
                assert w in msg, (name, msg)
            assert np.array_equal(c.eval(Zh), want), name
    assert c.get_option("exp_hess") == 0 and c.hess_nnz == 0
    c.close()


# ---- the Python constructors -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ket", [True, False])
def test_constructors_end_to_end(ket):
    sysv = pa.VariationalQuantumSystem(pa.PAULIS["Z"] / 2, [pa.PAULIS["X"], pa.PAULIS["Y"]], [pa.PAULIS["Z"] / 2], [1.0, 1.0])
    _, _, _, case = cases.pauli(ket)
    names = ["ψ̃", "ψ̃_var"] if ket else ["Ũ⃗", "Ũ⃗_var"]
    comps = {nm: case.Z[:, o : o + case.xdc].T for nm, o in zip(names, case.xo)}
    comps["Δt"] = case.Z[:, case.dt_off][None]
    comps["t"] = case.Z[:, case.dt_off + 1][None]
    comps["u"] = case.Z[:, case.u_off : case.u_off + case.m].T
    traj = pa.NamedTrajectory(comps, controls=("u", "Δt"), timestep="Δt")
    assert np.array_equal(traj.datavec, case.Z.reshape(-1))
    ctor = pa.VariationalKetIntegrator if ket else pa.VariationalUnitaryIntegrator
    for order in ("exp", -1):
        B = ctor(sysv, traj, names[0], names[1:], "u", pade_order=order)
        assert B.pade_order == -1 and B.exponential and B.ctx.batch_mode == VEXP
        assert B.x_dim == case.xd and B.dim == case.xd * case.K
        delta = np.zeros(B.dim)
        pa.evaluate_(delta, B, traj)
        close(delta, truth.residual(case), 1e-11)
        J = pa.eval_jacobian(B, traj)
        r, cc = truth.structure(case)
        close(np.asarray(J[r, cc]).reshape(-1), truth.values(case), 1e-11)
        assert J.nnz <= len(r)
        for f in (lambda: pa.hessian_structure(B), lambda: pa.eval_hessian_of_lagrangian(B, traj, np.ones(B.dim))):
            with pytest.raises(pa.PclError) as ei:
                f()
            assert ei.value.code == E_NOTIMPL and "third Frechet" in str(ei.value)
        X = pa.variational_rollout(B, traj)
        assert X.shape == (case.xd, case.N) and np.array_equal(X[:, 0], np.concatenate([case.Z[0, o : o + case.xdc] for o in case.xo]))
        B.close()
