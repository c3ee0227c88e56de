"""The exponential mode (pcl_desc.pade_order = PCL_ORDER_EXP) on the device, through the C ABI:
    delta_k = X_{k+1} - exp(dt_k G(u_k)) X_k  and its Jacobian (Frechet pairs) against the committed oracle (po.exp_residual,
    po.exp_jacobian_values -- scipy.linalg.expm / expm_frechet) in the library's layout (tests/exp_truth.py).
Tolerance: close(a, b, 1e-11) of tests/test_parity_gpu.py -- the bound the rollout tests hold between the device's scaling and squaring
and scipy.linalg.expm; a numpy emulation of the recurrence (degree 14, theta <= 0.25, pair squaring) stays at 1e-15 .. 2e-14 of expm_frechet
on these systems, so the reference side is far inside it."""
import numpy as np
import pytest

import exp_truth
import piccolo_jl_amd as pa
from helpers import ref_case
from oracle import pade_oracle as po
from shape_cases import plain_case
from test_parity_gpu import close

pytestmark = pytest.mark.gpu
TOL = 1e-11
EXP = pa._lib.PCL_ORDER_EXP


def exp_ctx(lay, G0, Gj, **kw):
    args = dict(d=lay.d, m=lay.m, N=lay.N, z_dim=lay.z_dim, u_off=lay.u_off, dt_off=lay.dt_off, x_offs=[lay.x_off], G0=G0, Gj=Gj, batch=1,
                batch_mode=pa._lib.PCL_BATCH_MEMBERS, pade_order=EXP)  # fmt: skip
    if lay.gen is not None:
        args.update(d=lay.gen, state_cols=pa._lib.PCL_STATE_VECTOR)
    elif lay.cols is not None:
        args.update(state_cols=lay.cols)
    args.update(kw)
    return pa.integrators._PclContext(**args)


def truth(members, lay, traj_mode=False, index_base=0):
    """members: [(Z [N, z_dim], G0, Gj, x_off)] in row order.  (delta, values, rows, cols) of the launch."""
    ds, vs, rs, cs = [], [], [], []
    for b, (Z, G0, Gj, xo) in enumerate(members):
        ds.append(po.exp_residual(Z, lay, G0, Gj, x_off=xo).reshape(-1))
        vs.append(exp_truth.values(Z, lay, G0, Gj, x_off=xo).reshape(-1))
        r, c = exp_truth.structure(lay, x_off=xo, index_base=index_base, row0=b * lay.x_dim * lay.K, col0=b * lay.z_dim * lay.N if traj_mode else 0)
        rs.append(r)
        cs.append(c)
    return np.concatenate(ds), np.concatenate(vs), np.concatenate(rs), np.concatenate(cs)


def check(c, Zfull, members, lay, traj_mode=False, index_base=0, tol=TOL):
    """Every path of one context against the truth: host and device pointers, fused / residual only / Jacobian only; the structure entry
    for entry; the paths among themselves bitwise.  Returns (delta, values) of the fused device launch."""
    import torch

    d0, v0, r0, c0 = truth(members, lay, traj_mode, index_base)
    assert c.jac_per == exp_truth.nnz_per_interval(lay) and c.jac_nnz == v0.size and c.n_rows == d0.size
    assert c.get_option("pade_order") == -1
    rows, cols = c.jac_structure()
    assert np.array_equal(rows, r0) and np.array_equal(cols, c0)
    r32, c32 = c.jac_structure(np.int32)
    assert np.array_equal(r32, r0) and np.array_equal(c32, c0)
    Zh = np.ascontiguousarray(Zfull, dtype=np.float64).reshape(-1)
    # device pointers
    Zd = torch.from_numpy(Zh).cuda()
    dd = torch.full((c.n_rows,), float("nan"), dtype=torch.float64, device="cuda")
    vd = torch.full((c.jac_nnz,), float("nan"), dtype=torch.float64, device="cuda")
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    c.eval_jac_dev(Zd, dd, vd)
    c.sync()
    assert c.get_option("last_kernel") == 100
    delta, vals = dd.cpu().numpy(), vd.cpu().numpy()
    assert np.all(np.isfinite(delta)) and np.all(np.isfinite(vals))
    print("max|delta - oracle| %.3e  max|values - oracle| %.3e" % (np.abs(delta - d0).max(), np.abs(vals - v0).max()))
    close(delta, d0, tol)
    close(vals, v0, tol)
    d1 = torch.full_like(dd, float("nan"))
    c.eval_dev(Zd, d1)
    c.sync()
    assert c.get_option("last_kernel") == 101
    assert np.array_equal(d1.cpu().numpy(), delta)  # the residual-only launch: the fused launch's bits
    v1 = torch.full_like(vd, float("nan"))
    c.jac_dev(Zd, v1)
    c.sync()
    assert np.array_equal(v1.cpu().numpy(), vals)
    d2, v2 = torch.full_like(dd, float("nan")), torch.full_like(vd, float("nan"))
    c.eval_jac_dev(Zd, d2, v2)  # a second launch: the same bits
    c.sync()
    assert np.array_equal(d2.cpu().numpy(), delta) and np.array_equal(v2.cpu().numpy(), vals)
    c.set_stream(None)
    # host pointers (full values)
    hd, hv = c.eval_jac(Zh)
    assert np.array_equal(hd, delta) and np.array_equal(hv, vals)
    assert np.array_equal(c.eval(Zh), delta) and np.array_equal(c.jac(Zh), vals)
    return delta, vals


def config_case(cfg, N, seed, dt=None):
    so = po.config_system(cfg)
    Z, lay = po.synthetic_trajectory(so, N, seed=seed)
    if dt is not None:
        Z[:, lay.dt_off] = dt
    return lay, so.G_drift, np.array(so.G_drives), Z


# ---- 1. parity on the shapes and modes served -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg, N", [(1, 50), (2, 100), (3, 100)])
def test_configs_against_oracle(cfg, N):
    """BASELINE configs 1, 2 and 3 (synthetic trajectory, every interval: 99 x 6 workgroups at config 3)."""
    lay, G0, Gj, Z = config_case(cfg, N, seed=11 + cfg)
    c = exp_ctx(lay, G0, Gj)
    check(c, Z, [(Z, G0, Gj, lay.x_off)], lay)
    c.close()


def test_ket():
    rng = np.random.default_rng(105)
    d, m, N = 5, 2, 6
    n = 2 * d
    Hd = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
    Hs = [(lambda A: A + A.conj().T)((rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))) * (rng.random((d, d)) < 0.4)) for _ in range(m)]
    so = po.quantum_system(0.3 * (Hd + Hd.conj().T), Hs, [1.0] * m)
    lay = po.Layout(d=d, m=m, N=N, z_dim=n + 2 + 3 * m, x_off=0, u_off=n + 2, dt_off=n, cols=1)
    Z = 0.5 * rng.standard_normal((N, lay.z_dim))
    Z[:, lay.dt_off] = 0.05 + 0.05 * rng.random(N)
    G0, Gj = so.G_drift, np.array(so.G_drives)
    c = exp_ctx(lay, G0, Gj)
    check(c, Z, [(Z, G0, Gj, 0)], lay)
    c.close()


def test_compact_density_vector_odd_n():
    """PCL_STATE_VECTOR: a general real generator of odd dimension (levels = 3: n = 9) on one column."""
    rng = np.random.default_rng(34)
    lv, m, N = 3, 2, 7
    H = rng.standard_normal((lv, lv)) + 1j * rng.standard_normal((lv, lv))
    H = 0.5 * (H + H.conj().T)
    Hs = [(lambda A: A + A.conj().T)(rng.standard_normal((lv, lv)) + 1j * rng.standard_normal((lv, lv))) for _ in range(m)]
    a = po.annihilate(lv)
    G0, Gj = po.compact_lindbladian_generators(H, Hs, [0.3 * a, 0.1 * np.diag(np.arange(lv)).astype(complex)])
    Gj = np.array(Gj)
    n = lv * lv
    lay = po.Layout(d=0, m=m, N=N, z_dim=n + 2 + m, x_off=0, u_off=n + 2, dt_off=n, cols=1, gen=n)
    Z = 0.5 * rng.standard_normal((N, lay.z_dim))
    Z[:, lay.dt_off] = 0.05 + 0.05 * rng.random(N)
    c = exp_ctx(lay, G0, Gj)
    check(c, Z, [(Z, G0, Gj, 0)], lay)
    c.close()


def test_d32_six_drives_the_lds_limit():
    """n = 64 with 32 state columns and six drives: four n x n tiles and the X_k tile, G_l read from L2."""
    lay, G0, Gj, Z = plain_case("S6", N=4)
    assert lay.d == 32 and lay.m == 6
    c = exp_ctx(lay, G0, Gj)
    check(c, Z, [(Z, G0, Gj, 0)], lay)
    c.close()


def test_no_drives():
    so = po.config_system(2)
    G0 = so.G_drift
    d, N = 4, 9
    xd = 2 * d * d
    lay = po.Layout(d=d, m=0, N=N, z_dim=xd + 3, x_off=1, u_off=xd + 2, dt_off=xd + 1)
    rng = np.random.default_rng(8)
    Z = rng.standard_normal((N, lay.z_dim))
    Z[:, lay.dt_off] = 0.05 + 0.1 * rng.random(N)
    c = exp_ctx(lay, G0, np.zeros((0, 2 * d, 2 * d)))
    check(c, Z, [(Z, G0, np.zeros((0, 2 * d, 2 * d)), 1)], lay)
    c.close()


def test_ensemble_with_per_member_drifts_and_member_window(golden, golden_meta):
    """ref_sampling_robust: three members with their own drifts in one trajectory buffer; then a window of the last two, whose values are
    the slices of the full launch, bitwise."""
    systems, lay, x_offs = ref_case("sampling_robust", golden_meta)
    Z = golden("ref_sampling_robust")["Z"]
    M = len(systems)
    G0s, Gj = np.array([s.G_drift for s in systems]), np.array(systems[0].G_drives)
    c = exp_ctx(lay, G0s, Gj, x_offs=x_offs, batch=M, per_member_G0=True)
    members = [(Z, s.G_drift, Gj, xo) for s, xo in zip(systems, x_offs)]
    delta, vals = check(c, Z, members, lay)
    per_d, per_v = lay.x_dim * lay.K, exp_truth.nnz_per_interval(lay) * lay.K
    c.set_member_window(1, M - 1)
    wd, wv = c.eval_jac(Z)
    assert np.array_equal(wd, delta[per_d:]) and np.array_equal(wv, vals[per_v:])
    r, cc = c.jac_structure()
    r0 = np.concatenate([exp_truth.structure(lay, x_off=x_offs[1 + b], row0=b * per_d)[0] for b in range(M - 1)])
    c0 = np.concatenate([exp_truth.structure(lay, x_off=x_offs[1 + b], row0=b * per_d)[1] for b in range(M - 1)])
    assert np.array_equal(r, r0) and np.array_equal(cc, c0)
    assert np.array_equal(c.eval(Z), delta[per_d:])
    c.set_member_window(0, M)
    assert np.array_equal(c.eval(Z), delta)
    c.close()


def test_shared_drift_members():
    """PCL_BATCH_MEMBERS with one G0 for two members at different state offsets."""
    so = po.config_system(1)
    G0, Gj = so.G_drift, np.array(so.G_drives)
    d, m, N = 2, 2, 8
    xd = 2 * d * d
    lay = po.Layout(d=d, m=m, N=N, z_dim=2 * xd + 2 + m, x_off=0, u_off=2 * xd + 2, dt_off=2 * xd)
    rng = np.random.default_rng(21)
    Z = 0.4 * rng.standard_normal((N, lay.z_dim))
    Z[:, lay.dt_off] = 0.1 + 0.1 * rng.random(N)
    c = exp_ctx(lay, G0, Gj, x_offs=[0, xd], batch=2)
    check(c, Z, [(Z, G0, Gj, 0), (Z, G0, Gj, xd)], lay)
    c.close()


def test_batch_traj_three_seeds_and_window():
    lay, G0, Gj, _ = config_case(2, 12, seed=0)
    Zs = np.stack([config_case(2, 12, seed=40 + b)[3] for b in range(3)])
    c = exp_ctx(lay, G0, Gj, batch=3, batch_mode=pa._lib.PCL_BATCH_TRAJ)
    delta, vals = check(c, Zs, [(Zs[b], G0, Gj, lay.x_off) for b in range(3)], lay, traj_mode=True)
    per_d, per_v = lay.x_dim * lay.K, exp_truth.nnz_per_interval(lay) * lay.K
    c.set_member_window(2, 1)
    wd, wv = c.eval_jac(Zs)
    assert np.array_equal(wd, delta[2 * per_d :]) and np.array_equal(wv, vals[2 * per_v :])
    r, cc = c.jac_structure()
    r0, c0 = exp_truth.structure(lay, col0=2 * lay.z_dim * lay.N)
    assert np.array_equal(r, r0) and np.array_equal(cc, c0)
    c.close()


def test_index_base_one():
    lay, G0, Gj, Z = config_case(1, 6, seed=2)
    c = exp_ctx(lay, G0, Gj, index_base=1)
    check(c, Z, [(Z, G0, Gj, lay.x_off)], lay, index_base=1)
    c.close()


# ---- 2. steps ------------------------------------------------------------------------------------------------------------------------
def test_zero_and_negative_steps():
    """dt = 0 at one knot: E = I, L = 0, the dt tail is -G X_k and nothing is NaN; a negative dt at another."""
    lay, G0, Gj, Z = config_case(2, 8, seed=5)
    Z[3, lay.dt_off] = 0.0
    Z[5, lay.dt_off] = -0.13
    c = exp_ctx(lay, G0, Gj)
    delta, vals = check(c, Z, [(Z, G0, Gj, lay.x_off)], lay)
    per = exp_truth.nnz_per_interval(lay)
    C, n, m = lay.C, lay.n, lay.m
    v3 = vals[3 * per : 4 * per]
    assert np.array_equal(v3[: C * n * n], np.tile(-np.eye(n).reshape(-1), C))  # -E = -I exactly
    tail = v3[C * n * n + lay.x_dim :].reshape(C, m + 1, n)
    assert not tail[:, :m].any()  # L = 0
    G = G0 + np.tensordot(lay.u(Z, 3), Gj, axes=1)
    close(tail[:, m], -(G @ lay.X(Z, 3)).T, 1e-13)
    close(delta[3 * lay.x_dim : 4 * lay.x_dim], Z[4, : lay.x_dim] - Z[3, : lay.x_dim], 0.0)
    c.close()


@pytest.mark.parametrize("cfg, N, dt", [(2, 6, 4.0), (3, 4, 1.0)])
def test_large_steps_several_squarings(cfg, N, dt):
    """config 2 at dt = 4.0 and config 3 at dt = 1.0: several squarings of the pair (Hermitian systems)."""
    lay, G0, Gj, Z = config_case(cfg, N, seed=17, dt=dt)
    G = G0 + np.tensordot(lay.u(Z, 0), Gj, axes=1)
    assert dt * np.abs(G).sum(axis=0).max() > 2.0  # at least four squarings
    c = exp_ctx(lay, G0, Gj)
    check(c, Z, [(Z, G0, Gj, lay.x_off)], lay)
    c.close()


# ---- 3. the reference's own trajectories ----------------------------------------------------------------------------------------------
def test_reference_trajectories_are_feasible_in_this_mode_only(golden, golden_meta):
    """max|delta| on the reference's converged trajectories: below 1e-9 on ref_multilevel_transmon (max |dt G| = 1.64) and below 1e-11 on
    ref_two_qubit_zoh -- the bounds tests/test_oracle_pins.py holds the oracle to -- where an order-10 context reports more than 1e-8 on the
    first: what the mode is for."""
    out = {}
    for name, bound in (("multilevel_transmon", 1e-9), ("two_qubit_zoh", 1e-11)):
        systems, lay, _ = ref_case(name, golden_meta)
        Z = golden("ref_" + name)["Z"]
        G0, Gj = systems[0].G_drift, np.array(systems[0].G_drives)
        c = exp_ctx(lay, G0, Gj)
        delta = c.eval(Z)
        close(delta, po.exp_residual(Z, lay, G0, Gj), TOL)
        out[name] = np.abs(delta).max()
        print("%s: max|delta| %.3e" % (name, out[name]))
        assert out[name] < bound, out[name]
        c.close()
    systems, lay, _ = ref_case("multilevel_transmon", golden_meta)
    Z = golden("ref_multilevel_transmon")["Z"]
    c10 = exp_ctx(lay, systems[0].G_drift, np.array(systems[0].G_drives), pade_order=10)
    d10 = np.abs(c10.eval(Z)).max()
    print("multilevel_transmon, order 10: max|delta| %.3e" % d10)
    assert d10 > 1e-8, d10
    c10.close()


# ---- 4. consistency inside the library --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg, N, dt", [(2, 20, None), (3, 6, 1.0)])
def test_residual_of_the_rollout_vanishes(cfg, N, dt):
    lay, G0, Gj, Z = config_case(cfg, N, seed=23, dt=dt)
    c = exp_ctx(lay, G0, Gj)
    X = c.rollout(Z)[0]
    Zr = Z.copy()
    Zr[:, lay.x_off : lay.x_off + lay.x_dim] = X
    delta = c.eval(Zr)
    print("max|delta| on the rollout: %.3e" % np.abs(delta).max())
    assert np.abs(delta).max() < 1e-12
    c.close()


# ---- 5. what does not depend on the integrator ------------------------------------------------------------------------------------------
def test_objective_its_hessian_and_the_rollout_equal_an_order_4_context_bitwise():
    lay, G0, Gj, Z = config_case(2, 16, seed=31)
    goal = po.operator_to_iso_vec(np.linalg.qr(np.random.default_rng(1).standard_normal((4, 4)) + 1j * np.random.default_rng(2).standard_normal((4, 4)))[0])
    res = []
    for order in (EXP, 4):
        c = exp_ctx(lay, G0, Gj, pade_order=order)
        c.set_goal(goal)
        c.add_regularizer(lay.u_off, lay.m, 1e-2, 2)
        c.add_regularizer(lay.u_off + lay.m, lay.m, 1e-2, 0)
        val, grad = c.objective(Z, 100.0)
        hr, hc = c.objective_hess_structure()
        hv = c.objective_hess(Z, 100.0, 0.7)
        X = c.rollout(Z)
        dr, dv = c.deriv_eval_jac(lay.u_off, lay.u_off + lay.m, lay.m, Z)
        res.append((val, grad, hr, hc, hv, X, dr, dv))
        c.close()
    for a, b in zip(*res):
        assert np.array_equal(a, b)
    assert np.all(np.isfinite(res[0][1])) and res[0][4].size > 0
    close(res[0][5][0], po.exact_rollout(Z, lay, G0, Gj), TOL)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_mode_and_leave_the_context_usable():
    import ctypes

    import torch

    lay, G0, Gj, Z = config_case(2, 6, seed=3)
    c = exp_ctx(lay, G0, Gj)
    L, h = c._L, c._h
    want = c.eval(Z)
    Zd = torch.from_numpy(Z.reshape(-1)).cuda()
    buf = torch.zeros(c.jac_nnz + c.n_rows, dtype=torch.float64, device="cuda")
    hb = np.zeros(c.jac_nnz + c.n_rows)
    a, b = ctypes.c_int64(), ctypes.c_int64()
    idx = np.zeros(8, dtype=np.int64)
    i32p, i64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    E, NI = pa._lib.PCL_EINVAL, pa._lib.PCL_ENOTIMPL
    p, z = buf.data_ptr(), Zd.data_ptr()
    calls = [
        ("pcl_hess", NI, lambda: L.pcl_hess(h, Z.ctypes.data, hb.ctypes.data, hb.ctypes.data)),
        ("pcl_hess_dev", NI, lambda: L.pcl_hess_dev(h, z, p, p)),
        ("pcl_hess_nnz", NI, lambda: L.pcl_hess_nnz(h, ctypes.byref(a), ctypes.byref(b))),
        ("pcl_hess_structure", NI, lambda: L.pcl_hess_structure(h, idx.ctypes.data_as(i32p), idx.ctypes.data_as(i32p))),
        ("pcl_hess_structure_i64", NI, lambda: L.pcl_hess_structure_i64(h, idx.ctypes.data_as(i64p), idx.ctypes.data_as(i64p))),
        ("pcl_jac_compact_nnz", NI, lambda: L.pcl_jac_compact_nnz(h, ctypes.byref(a), ctypes.byref(b))),
        ("pcl_eval_jac_compact_dev", NI, lambda: L.pcl_eval_jac_compact_dev(h, z, p, p)),
        ("pcl_jac_expand_dev", NI, lambda: L.pcl_jac_expand_dev(h, p, p)),
        ("pcl_merit_grad_len", NI, lambda: L.pcl_merit_grad_len(h, ctypes.byref(a), ctypes.byref(b))),
        ("pcl_merit_grad_dev", NI, lambda: L.pcl_merit_grad_dev(h, p, None, p, p)),
        ("pcl_eval_jac_merit_dev", NI, lambda: L.pcl_eval_jac_merit_dev(h, z, None, p, p, p)),
        ("pcl_eval_jac_merit_objective_dev", NI, lambda: L.pcl_eval_jac_merit_objective_dev(h, z, None, p, p, p, 1.0, p, p)),
    ]
    for name, code, call in calls:
        rc = call()
        msg = L.pcl_last_error(h).decode()
        assert rc == code, (name, rc, msg)
        assert "exponential" in msg and "PCL_ORDER_EXP" in msg, (name, msg)
        assert np.array_equal(c.eval(Z), want), name
    for name, fn in (("pcl_set_order_policy", lambda: c.set_order_policy(0.2, [0.1] * lay.m)), ("pcl_set_order_from_trajectory", lambda: c.set_order_from_trajectory(Z))):
        with pytest.raises(pa.PclError) as ei:
            fn()
        assert ei.value.code == E and "exponential" in str(ei.value) and "no order to choose" in str(ei.value), name
        assert c.get_option("pade_order") == -1 and np.array_equal(c.eval(Z), want)
    with pytest.raises(pa.PclError) as ei:
        c.hess_structure()
    assert ei.value.code == NI and "exponential" in str(ei.value)
    c.close()


# ---- the reference-style objects ---------------------------------------------------------------------------------------------------------
def test_bilinear_integrator_with_pade_order_exp():
    from helpers import traj_from_Z
    from test_parity_gpu import product_system

    lay, G0, Gj, Z = config_case(2, 10, seed=13)
    traj = traj_from_Z(pa, Z, lay)
    B = pa.BilinearIntegrator(product_system(2), traj, pade_order="exp")
    assert B.pade_order == -1 and B.dim == lay.x_dim * lay.K
    d0, v0, r0, c0 = truth([(Z, G0, Gj, lay.x_off)], lay)
    close(pa.evaluate_(np.zeros(B.dim), B, traj), d0, TOL)
    r, c = pa.jacobian_structure(B)
    assert np.array_equal(r, r0) and np.array_equal(c, c0)
    close(pa.eval_jacobian(B, traj).toarray(), exp_truth.dense(Z, lay, G0, Gj), TOL)
    k = 3
    close(B.f(Z[k + 1, : lay.x_dim], Z[k, : lay.x_dim], Z[k, lay.u_off : lay.u_off + lay.m], Z[k, lay.dt_off]), d0[k * lay.x_dim : (k + 1) * lay.x_dim], TOL)
    for fn in (lambda: pa.hessian_structure(B), lambda: pa.eval_hessian_of_lagrangian(B, traj, np.zeros(B.dim))):
        with pytest.raises(pa.PclError) as ei:
            fn()
        assert "exponential" in str(ei.value)
    B.close()
