"""The variational exponential Hessian with four of the octuple chain's tiles in a device workspace (option ``var_exp_hess_tiles``;
pcl_kernel_var_exp_hess_tiles.hpp) on the device.  Where both plans run (n <= 44) the workspace plan must give the SAME BITS as the LDS plan:
the recurrence, the order of its terms and every product are the same, only the home of four tiles differs -- the cheapest complete check of the
tile bookkeeping.  At the newly served shapes (n = 46 .. 62, config 3 among them) every value is compared with the lifted truth of
tests/var_exp_hess_truth.py at ``close(..., 1e-11)``, the tolerance of this kernel family; a numpy run of the recurrence sits at 6e-16 .. 7e-15
of that truth there (tests/test_var_exp_hess_tiles_cpu.py)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import piccolo_jl_amd as pa
import var_exp_cases as cases
import var_exp_hess_truth as truth
from test_var_exp_hess_cpu import GPU_TOL, close
from test_var_exp_hess_gpu import no_drives, one_drive, plain_ctx, rand_mu, var_ctx

pytestmark = pytest.mark.gpu
EXP, VEXP = pa._lib.PCL_ORDER_EXP, pa._lib.PCL_BATCH_VARIATIONAL_EXP
E_INVAL, E_SHAPE, E_NOTIMPL = pa._lib.PCL_EINVAL, pa._lib.PCL_ESHAPE, pa._lib.PCL_ENOTIMPL
K_LDS, K_WS = 110, 112  # last_hess_kernel: nine LDS tiles | five, and four in the workspace


def hess_ctx(case, tiles, index_base=0):
    c = var_ctx(case, index_base=index_base)
    c.set_option("var_exp_hess_tiles", tiles)
    c.set_option("var_exp_hess", 1)
    assert c.get_option("var_exp_hess_tiles") == tiles and c.get_option("var_exp_hess") == 1
    return c


def launch(c, case, mu):
    Zd, mud = torch.from_numpy(np.ascontiguousarray(case.Z, dtype=np.float64).reshape(-1)).cuda(), torch.from_numpy(mu).cuda()
    vd = torch.full((c.hess_nnz,), float("nan"), dtype=torch.float64, device="cuda")
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    c.hess_dev(Zd, mud, vd)
    c.sync()
    c.set_stream(None)
    return vd.cpu().numpy()


def same_bits(case, seed=1, index_base=0):
    """var_exp_hess_tiles = 2 beside = 0 on two contexts: every value bitwise, last_hess_kernel 112 and 110."""
    mu = rand_mu(case, seed)
    a, b = hess_ctx(case, 0, index_base), hess_ctx(case, 2, index_base)
    va, vb = launch(a, case, mu), launch(b, case, mu)
    assert a.get_option("last_hess_kernel") == K_LDS and b.get_option("last_hess_kernel") == K_WS
    assert np.all(np.isfinite(va)) and va.any()
    assert np.array_equal(va, vb), np.abs(va - vb).max()
    for x, y in zip(a.hess_structure(), b.hess_structure()):
        assert np.array_equal(x, y)
    a.close()
    b.close()
    return va


@functools.lru_cache(maxsize=None)
def new_shape(which):
    """(case, mu, truth values): computed once, shared by the tests of one shape, never written to."""
    case = {"transmon23": lambda: cases.transmon(23, N=3)[3], "transmon27_ket": lambda: cases.transmon(27, N=3, ket=True)[3],
            "transmon31": lambda: cases.transmon(31, N=3)[3], "transmon31_ket": lambda: cases.transmon(31, N=3, ket=True)[3],
            "config3_v1": lambda: cases.config3(1, N=3)[3], "config3_v2_ket": lambda: cases.config3(2, N=3, ket=True)[3]}[which]()  # fmt: skip
    mu = rand_mu(case, 1)
    v0 = truth.values(case, mu).reshape(-1)
    v0.setflags(write=False)
    return case, mu, v0


def check(case, mu, v0, tiles, kernel, index_base=0):
    """``check`` of tests/test_var_exp_hess_gpu.py with the option and the expected last_hess_kernel as parameters: the structure entry for
    entry (int64 and int32), rows >= cols, the device-pointer launch value for value, a second launch and the host-pointer call bitwise."""
    c = hess_ctx(case, tiles, index_base)
    r0, c0 = truth.structure(case, index_base)
    assert c.get_option("exp_hess") == 0
    assert c.hess_per == truth.nnz_per_interval(case) and c.hess_nnz == v0.size
    rows, cols = c.hess_structure()
    assert np.array_equal(rows, r0) and np.array_equal(cols, c0)
    r32, c32 = c.hess_structure(np.int32)
    assert np.array_equal(r32, r0) and np.array_equal(c32, c0)
    assert np.all(rows >= cols)
    vals = launch(c, case, mu)
    assert c.get_option("last_hess_kernel") == kernel
    assert np.all(np.isfinite(vals))
    per, nsc = truth.nnz_per_interval(case), (case.m + 1) * (case.m + 2) // 2
    a, t = vals.reshape(-1, per), v0.reshape(-1, per)
    scale = max(1.0, np.abs(v0).max())
    print("max|values - truth| / max(1, |truth|): scalars %.3e  state slices %.3e   (|truth|_inf %.3e)"
          % (np.abs(a[:, :nsc] - t[:, :nsc]).max() / scale, np.abs(a[:, nsc:] - t[:, nsc:]).max() / scale, np.abs(v0).max()))  # fmt: skip
    close(vals, v0, GPU_TOL)
    assert np.array_equal(launch(c, case, mu), vals)  # a second launch: the same bits
    assert np.array_equal(c.hess(np.ascontiguousarray(case.Z).reshape(-1), mu), vals)  # host pointers
    return c, vals


# ---- 1. the same bits as the LDS plan ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ket", [True, False])
def test_same_bits_pauli(ket):
    same_bits(cases.pauli(ket)[3])


@pytest.mark.parametrize("nv, ket", [(1, False), (2, False), (1, True)])
def test_same_bits_config2(nv, ket):
    same_bits(cases.config2(nv, ket=ket)[3])


def test_same_bits_transmon3_n_not_a_multiple_of_four():
    same_bits(cases.transmon(3)[3])


def test_same_bits_transmon17_the_512_thread_variant():
    same_bits(cases.transmon(17, N=3)[3])


def test_same_bits_transmon22_the_largest_shape_of_both_plans():
    same_bits(cases.transmon(22, N=3)[3])


def test_same_bits_no_drives():
    """m = 0: the pair (T, Tb_i) alone -- no spilled tile is touched."""
    same_bits(no_drives(cases.config2(2)[3]))


def test_same_bits_one_drive():
    same_bits(one_drive(cases.config2(2)[3]))


def test_same_bits_index_base_one():
    same_bits(cases.config2(2, N=5)[3], index_base=1)


def test_same_bits_zero_step_on_one_interval():
    case = cases.config2(2, N=5)[3]
    case.Z[2, case.dt_off] = 0.0
    vals = same_bits(case)
    per, m = truth.nnz_per_interval(case), case.m
    assert not vals[2 * per : 2 * per + m * (m + 1) // 2].any()  # dt = 0: the (u, u) block of that interval is exactly zero


def test_same_bits_negative_steps():
    case = cases.config2(2, N=4)[3]
    case.Z[:, case.dt_off] *= -1.0
    same_bits(case)


def test_same_bits_large_step_five_squarings():
    """config 2 at dt = 4: the cross terms of the Tabc squaring read four spilled tiles, as left and as right operands."""
    case = cases.config2(1, dt=4.0)[3]
    G = case.G0 + np.tensordot(case.Z[0, case.u_off : case.u_off + case.m], case.Gj, axes=1)
    assert case.Z[0, case.dt_off] * np.abs(G).sum(axis=0).max() > 2.0  # at least four squarings
    same_bits(case)


# ---- 2. the newly served shapes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["transmon23", "transmon27_ket", "transmon31", "transmon31_ket", "config3_v1", "config3_v2_ket"])
def test_newly_served_shapes_against_the_truth(which):
    """transmon(23): n = 46, the first shape beyond nine tiles.  transmon(27) ket: n = 54 with one column.  transmon(31), unitary and ket:
    n = 62, five resident tiles of 32 736 B are 163 680 of 163 840 B and G(u_k) comes from the workspace; five squarings.  config 3, v = 1:
    cols = 27 = n / 2, the boundary of the last phase, m = 6.  config 3, v = 2, ket: two slots per interval in the finish kernel."""
    case, mu, v0 = new_shape(which)
    assert case.n >= 46
    check(case, mu, v0, 1, K_WS)[0].close()


# ---- 3. independent of the tile plan ---------------------------------------------------------------------------------------------------------
def test_directional_derivative_of_the_device_jacobian_config3():
    """H d against the central difference (step 1e-6) of the device's own J' mu at config 3, formed on the device from two pcl_jac_dev
    results.  Bound: 1e-6 max(1, |fd|_inf), the step and the figure of tests/test_var_exp_hess_gpu.py."""
    case = new_shape("config3_v1")[0]
    c = hess_ctx(case, 1)
    nv_ = case.z_dim * case.N
    rng = np.random.default_rng(12)
    mu = torch.from_numpy(rng.standard_normal(c.n_rows)).cuda()
    d = rng.standard_normal(nv_)
    d = torch.from_numpy(d / np.linalg.norm(d)).cuda()
    Zd = torch.from_numpy(case.Z.reshape(-1).copy()).cuda()
    jr, jc = (torch.from_numpy(a).cuda() for a in c.jac_structure())
    hr, hc = (torch.from_numpy(a).cuda() for a in c.hess_structure())
    c.set_stream(torch.cuda.current_stream().cuda_stream)

    def jt_mu(Zx):
        vals = torch.empty(c.jac_nnz, dtype=torch.float64, device="cuda")
        c.jac_dev(Zx, vals)
        return torch.zeros(nv_, dtype=torch.float64, device="cuda").index_add_(0, jc, vals * mu[jr])

    step = 1e-6
    fd = (jt_mu(Zd + step * d) - jt_mu(Zd - step * d)) / (2 * step)
    hv = torch.empty(c.hess_nnz, dtype=torch.float64, device="cuda")
    c.hess_dev(Zd, mu, hv)
    Hd = torch.zeros(nv_, dtype=torch.float64, device="cuda").index_add_(0, hr, hv * d[hc])
    off = hr != hc
    Hd.index_add_(0, hc[off], hv[off] * d[hr[off]])
    c.sync()
    c.set_stream(None)
    assert c.get_option("last_hess_kernel") == K_WS
    err, scale = (Hd - fd).abs().max().item(), max(1.0, fd.abs().max().item())
    print("|H d - fd|_inf %.3e   |fd|_inf %.3e" % (err, fd.abs().max().item()))
    assert err <= 1e-6 * scale, (err, scale)
    c.close()


# ---- 4. the option -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which, need, tile", [("transmon23", 165600, 18400), ("config3_v1", 225504, 25056)])
def test_default_zero_leaves_the_shapes_beyond_nine_tiles_refused(which, need, tile):
    case = new_shape(which)[0]
    c = var_ctx(case)
    assert c.get_option("var_exp_hess_tiles") == 0
    with pytest.raises(pa.PclError) as ei:
        c.set_option("var_exp_hess", 1)
    msg = str(ei.value)
    assert ei.value.code == E_SHAPE and "LDS" in msg and str(need) in msg and "163840" in msg and str(tile) in msg, msg
    assert "var_exp_hess_tiles" in msg, msg  # the message now names the option that serves the shape
    assert c.get_option("var_exp_hess") == 0 and c.get_option("var_exp_hess_tiles") == 0
    with pytest.raises(pa.PclError) as ei:
        c.hess_structure()
    assert ei.value.code == E_NOTIMPL
    c.close()


def test_option_needs_a_variational_exponential_context():
    case = cases.config2(1)[3]
    Zh = case.Z.reshape(-1)
    for make in (lambda: plain_ctx(case, case.xo[0]), lambda: plain_ctx(case, case.xo[0], pade_order=4),
                 lambda: var_ctx(case, batch_mode=pa._lib.PCL_BATCH_VARIATIONAL, pade_order=4)):  # fmt: skip
        c = make()
        want = c.eval(Zh)
        assert c.get_option("var_exp_hess_tiles") == 0  # readable on every context
        for v in (1, 2):
            with pytest.raises(pa.PclError) as ei:
                c.set_option("var_exp_hess_tiles", v)
            assert ei.value.code == E_INVAL and "PCL_BATCH_VARIATIONAL_EXP" in str(ei.value)
        c.set_option("var_exp_hess_tiles", 0)  # allowed everywhere
        assert c.get_option("var_exp_hess_tiles") == 0
        assert np.array_equal(c.eval(Zh), want)
        c.close()


@pytest.mark.parametrize("bad", [3, -1])
def test_unknown_value_is_einval(bad):
    c = var_ctx(cases.config2(1)[3])
    with pytest.raises(pa.PclError) as ei:
        c.set_option("var_exp_hess_tiles", bad)
    assert ei.value.code == E_INVAL and c.get_option("var_exp_hess_tiles") == 0
    c.close()


def test_a_change_while_the_hessian_is_on_is_refused():
    """The value is read when var_exp_hess is set to 1.  While that option is on, another value is PCL_EINVAL (the same value is accepted) and
    the plan in force stays; after var_exp_hess = 0 the value may change and holds from the next var_exp_hess = 1."""
    case = cases.config2(1, N=4)[3]
    mu = rand_mu(case, 5)
    c = hess_ctx(case, 0)
    ref = launch(c, case, mu)
    assert c.get_option("last_hess_kernel") == K_LDS
    for v in (1, 2):
        with pytest.raises(pa.PclError) as ei:
            c.set_option("var_exp_hess_tiles", v)
        assert ei.value.code == E_INVAL and "var_exp_hess = 0" in str(ei.value)
    c.set_option("var_exp_hess_tiles", 0)
    assert c.get_option("var_exp_hess_tiles") == 0 and c.get_option("var_exp_hess") == 1
    assert np.array_equal(launch(c, case, mu), ref) and c.get_option("last_hess_kernel") == K_LDS
    c.set_option("var_exp_hess", 0)
    c.set_option("var_exp_hess_tiles", 2)
    c.set_option("var_exp_hess", 1)
    assert np.array_equal(launch(c, case, mu), ref) and c.get_option("last_hess_kernel") == K_WS
    with pytest.raises(pa.PclError) as ei:
        c.set_option("var_exp_hess_tiles", 0)
    assert ei.value.code == E_INVAL and c.get_option("var_exp_hess_tiles") == 2
    assert np.array_equal(launch(c, case, mu), ref) and c.get_option("last_hess_kernel") == K_WS
    c.close()


def test_option_switches_the_five_entry_points_on_and_off():
    """var_exp_hess back to 0 restores the refusals of the five entry points in today's words, with the workspace plan as with the LDS plan."""
    case = cases.config2(1, N=4)[3]
    c = var_ctx(case)
    c.set_option("var_exp_hess_tiles", 2)
    assert c.get_option("var_exp_hess") == 0 and c.hess_nnz == 0
    Zh = case.Z.reshape(-1)
    want = c.eval(Zh)
    L, h = c._L, c._h
    n = truth.nnz_per_interval(case) * case.K
    Zd = torch.from_numpy(Zh.copy()).cuda()
    buf, out = torch.zeros(n, dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.float64, device="cuda")
    hb, hout = np.zeros(n), np.zeros(n)
    a, b = ctypes.c_int64(), ctypes.c_int64()
    idx = np.zeros(n, dtype=np.int64)
    i32p, i64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    calls = [
        ("pcl_hess", lambda: L.pcl_hess(h, Zh.ctypes.data, hb.ctypes.data, hout.ctypes.data)),
        ("pcl_hess_dev", lambda: L.pcl_hess_dev(h, Zd.data_ptr(), buf.data_ptr(), out.data_ptr())),
        ("pcl_hess_nnz", lambda: L.pcl_hess_nnz(h, ctypes.byref(a), ctypes.byref(b))),
        ("pcl_hess_structure", lambda: L.pcl_hess_structure(h, idx.ctypes.data_as(i32p), idx.ctypes.data_as(i32p))),
        ("pcl_hess_structure_i64", lambda: L.pcl_hess_structure_i64(h, idx.ctypes.data_as(i64p), idx.ctypes.data_as(i64p))),
    ]

    def refused():
        for name, call in calls:
            rc = call()
            msg = L.pcl_last_error(h).decode()
            assert rc == E_NOTIMPL, (name, rc, msg)
            for w in ("PCL_BATCH_VARIATIONAL_EXP", "is not implemented", "third Frechet", "quasi-Newton"):
                assert w in msg, (name, msg)
            assert np.array_equal(c.eval(Zh), want), name

    refused()
    c.set_option("var_exp_hess", 1)
    for name, call in calls:
        assert call() == 0, (name, L.pcl_last_error(h).decode())
    c.sync()
    assert c.get_option("last_hess_kernel") == K_WS
    assert a.value == n and b.value == truth.nnz_per_interval(case)
    assert c.hess_nnz == n and c.hess_per == truth.nnz_per_interval(case)
    c.set_option("var_exp_hess", 0)
    assert c.get_option("var_exp_hess") == 0 and c.get_option("var_exp_hess_tiles") == 2 and c.hess_nnz == 0 and c.hess_per == 0
    refused()
    c.close()


def test_other_results_are_bitwise_unchanged_by_the_option():
    """eval_jac and, with var_full, objective, objective Hessian and rollout: the same bits before the option, with it and after a launch."""
    from oracle import pade_oracle as po

    case = cases.config2(2, N=6, dt=0.3)[3]
    rng = np.random.default_rng(9)
    goal = po.operator_to_iso_vec(np.linalg.qr(rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4)))[0])
    Z = case.Z.reshape(-1)
    c = var_ctx(case)
    c.set_option("var_full", 1)
    c.set_goal(goal)
    c.set_weights([1.0, 0.3, 0.2])
    c.add_regularizer(case.u_off, case.m, 0.1, 2)

    def everything():
        d, v = c.eval_jac(Z)
        val, grad = c.objective(Z, 100.0)
        return [d, v, c.eval(Z), val, grad, c.objective_hess(Z, 100.0, 0.7), c.rollout(Z)]

    before = everything()
    c.set_option("var_exp_hess_tiles", 2)
    with_tiles = everything()
    c.set_option("var_exp_hess", 1)
    with_option = everything()
    assert np.all(np.isfinite(c.hess(Z, np.linspace(-1, 1, c.n_rows)))) and c.get_option("last_hess_kernel") == K_WS
    after = everything()
    for x, y, z, w in zip(before, with_tiles, with_option, after):
        assert np.array_equal(x, y) and np.array_equal(x, z) and np.array_equal(x, w)
    c.close()


def test_tiles_one_keeps_the_lds_plan_where_nine_tiles_fit():
    """var_exp_hess_tiles = 1 at n <= 44: today's kernel, today's bits, last_hess_kernel 110."""
    for case in (cases.config2(2)[3], cases.transmon(22, N=3)[3]):
        mu = rand_mu(case, 1)
        a, b = hess_ctx(case, 0), hess_ctx(case, 1)
        va, vb = launch(a, case, mu), launch(b, case, mu)
        assert a.get_option("last_hess_kernel") == K_LDS and b.get_option("last_hess_kernel") == K_LDS
        assert np.array_equal(va, vb)
        a.close()
        b.close()


# ---- 5. the Python constructors ----------------------------------------------------------------------------------------------------------------
def _config3_integrator():
    sys_o, Hv, scales, case = cases.config3(1, N=3)
    sysv = pa.VariationalQuantumSystem(sys_o.H_drift, list(sys_o.H_drives), Hv, [1.0] * sys_o.n_drives)
    names = ["Ũ⃗", "Ũ⃗_var"]
    comps = {nm: case.Z[:, o : o + case.xdc].T for nm, o in zip(names, case.xo)}
    comps["Δt"] = case.Z[:, case.dt_off][None]
    comps["t"] = case.Z[:, case.dt_off + 1][None]
    comps["u"] = case.Z[:, case.u_off : case.u_off + case.m].T
    traj = pa.NamedTrajectory(comps, controls=("u", "Δt"), timestep="Δt")
    assert np.array_equal(traj.datavec, case.Z.reshape(-1))
    return case, traj, lambda eh: pa.VariationalUnitaryIntegrator(sysv, traj, names[0], names[1:], "u", scales=scales, pade_order="exp", exp_hessian=eh)


def test_constructor_with_exp_hessian_workspace_serves_config3():
    case, mu, v0 = new_shape("config3_v1")
    case2, traj, make = _config3_integrator()
    assert np.array_equal(case2.Z, case.Z)
    with pytest.raises(pa.PclError) as ei:  # True keeps today's meaning: nine LDS tiles, which config 3 exceeds
        make(True)
    assert ei.value.code == E_SHAPE
    B = make("workspace")
    assert np.allclose(B.G_vars, np.array(case.Gv), rtol=0, atol=1e-13) and np.allclose(B.G_drift, case.G0, rtol=0, atol=1e-13)
    assert B.ctx.get_option("var_exp_hess") == 1 and B.ctx.get_option("var_exp_hess_tiles") == 1
    assert B.ctx.hess_nnz == v0.size and B.ctx.hess_per == truth.nnz_per_interval(case)
    r0, c0 = truth.structure(case)
    r, cc = pa.hessian_structure(B)
    assert np.array_equal(r, r0) and np.array_equal(cc, c0)
    close(B.ctx.hess(traj.datavec, mu), v0, GPU_TOL)
    assert B.ctx.get_option("last_hess_kernel") == K_WS
    B.ctx.set_option("var_exp_hess", 0)  # hess_nnz follows the option off and on
    assert B.ctx.hess_nnz == 0 and B.ctx.hess_per == 0 and not B.ctx.exp_hessian
    B.ctx.set_option("var_exp_hess", 1)
    assert B.ctx.hess_nnz == v0.size and B.ctx.exp_hessian
    B.close()
