"""Generator dimensions 66 .. 128 on the device (contexts created with PCL_LARGE_N; piccolo.jl_amd/csrc/pcl_kernel_pade_large.hpp), at the cases
of tests/large_shape_cases.py (the case table and the branch each case sits on are there), through the C ABI on device pointers.  Every value is
compared with the longdouble truth of tests/vector_shape_cases.py, rounded to float64, at TOL = 1e-11 PER SEGMENT, relative to the segment's own
maximum with no floor at 1 (shape_cases.check_segments) -- the project's tolerance for the Pade kernels (tests/test_vector_shapes_gpu.py).
tests/test_large_shapes_cpu.py shows that the reference formulation agrees with that truth to 1e-13 on these inputs and that each case sees a
dropped k range beyond 64, a zeroed last row tile, a dropped drive and a dropped state column at 1e-7.

Without the feature every test here fails at pcl_create (PCL_ESHAPE: the generator dimension exceeds 64; the flag itself is an unknown
batch mode)."""
import ctypes

import numpy as np
import pytest
import torch

import large_shape_cases as lc
import piccolo_jl_amd as pa
import vector_shape_cases as vc
from shape_cases import check_segments, jac_labels

pytestmark = pytest.mark.gpu
TOL = 1e-11
ENOTIMPL = pa._lib.PCL_ENOTIMPL
NAN = float("nan")


def make_ctx(lay, G0, Gj, order, flag=True, **kw):
    args = dict(d=lay.d, m=lay.m, N=lay.N, z_dim=lay.z_dim, u_off=lay.u_off, dt_off=lay.dt_off, x_offs=[lay.x_off], G0=G0, Gj=Gj, batch=1,
                batch_mode=pa._lib.PCL_BATCH_MEMBERS, pade_order=order, large_generator=flag)  # fmt: skip
    if lay.gen is not None:
        args.update(d=lay.gen, state_cols=pa._lib.PCL_STATE_VECTOR)
    else:
        args.update(state_cols=lay.cols)
    args.update(kw)
    c = pa.integrators._PclContext(**args)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    return c


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float64).reshape(-1)).cuda()


def nans(k):
    return torch.full((k,), NAN, dtype=torch.float64, device="cuda")


def eval_jac_dev(c, Zd):
    """(delta, values) of pcl_eval_jac_dev into NaN-filled arrays, as numpy."""
    dd, vd = nans(c.n_rows), nans(c.jac_nnz)
    c.eval_jac_dev(Zd, dd, vd)
    c.sync()
    return dd.cpu().numpy(), vd.cpu().numpy()


def worst(errs):
    s = max(errs, key=errs.get)
    return "%.1e (%s)" % (errs[s], s)


def check(lay, got, ref, what):
    """got, ref: (delta, values).  No NaN may remain; every segment within TOL of the truth."""
    assert not np.isnan(got[0]).any() and not np.isnan(got[1]).any(), what
    er = check_segments(got[0], ref[0], lc.residual_labels(lay), TOL)
    ej = check_segments(got[1], ref[1], jac_labels(lay), TOL)
    print("%s: residual %s  Jacobian %s" % (what, worst(er), worst(ej)))


def bitwise(a, b, what):
    for x, y in zip(a, b):
        assert np.array_equal(x, y), what


# ---- every case and order ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lc.NAMES)
@pytest.mark.parametrize("order", lc.ORDERS)
def test_eval_jac_per_segment(name, order):
    """pcl_eval_jac_dev against the truth; pcl_eval_dev alone and pcl_jac_dev alone give its bits; which kernel ran."""
    lay, G0, Gj, Z, _ = lc.case(name)
    ref = lc.truth(name, order)
    q = order // 2
    c = make_ctx(lay, G0, Gj, order)
    assert c.n_rows == ref[0].size and c.jac_nnz == ref[1].size and c.hess_nnz == 0 and c.compact_nnz == 0
    Zd = dev(Z)
    got = eval_jac_dev(c, Zd)
    assert c.get_option("last_kernel") == 290 + q
    check(lay, got, ref, "%s order %d" % (name, order))
    d2 = nans(c.n_rows)
    c.eval_dev(Zd, d2)
    c.sync()
    assert c.get_option("last_kernel") == 280 + q
    bitwise((got[0],), (d2.cpu().numpy(),), "pcl_eval_dev alone")
    v2 = nans(c.jac_nnz)
    c.jac_dev(Zd, v2)
    c.sync()
    assert c.get_option("last_kernel") == 290 + q
    bitwise((got[1],), (v2.cpu().numpy(),), "pcl_jac_dev alone")
    c.close()


# ---- two launches, every slicing -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["L5", "L6"])
@pytest.mark.parametrize("order", [4, 10])
def test_launches_and_slicings_bitwise(name, order):
    """Two launches give the same bits, and so does every split of the state columns (cols_per_slice) and of the power panels (general_slices)."""
    kind, n, cols, m = lc.CASES[name]
    lay, G0, Gj, Z, _ = lc.case(name)
    c = make_ctx(lay, G0, Gj, order)
    Zd = dev(Z)
    first = eval_jac_dev(c, Zd)
    check(lay, first, lc.truth(name, order), "%s order %d" % (name, order))
    bitwise(first, eval_jac_dev(c, Zd), "a second launch")
    for cp in sorted({1, 2, 3, cols - 1, cols}):
        c.set_option("cols_per_slice", cp)
        bitwise(first, eval_jac_dev(c, Zd), ("cols_per_slice", cp))
        d2 = nans(c.n_rows)
        c.eval_dev(Zd, d2)
        c.sync()
        bitwise((first[0],), (d2.cpu().numpy(),), ("pcl_eval_dev, cols_per_slice", cp))
    c.set_option("cols_per_slice", 0)
    for s in (1, 2, 7, cols, n):
        c.set_option("general_slices", s)
        bitwise(first, eval_jac_dev(c, Zd), ("general_slices", s))
    c.set_option("cols_per_slice", 2)  # both at once
    bitwise(first, eval_jac_dev(c, Zd), "general_slices with cols_per_slice")
    assert c.get_option("last_kernel") == 290 + order // 2
    c.close()


# ---- batched launches ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [4, 8])
def test_members_with_their_own_drifts_and_the_window(order):
    """L1 as two PCL_BATCH_MEMBERS members with per-member drifts: each member against its own truth, and the window on the second alone."""
    lay, _, Gj, Z, _ = lc.case("L1")
    G0s = [lc.case("L1", 0, b)[1] for b in range(2)]
    c = make_ctx(lay, np.array(G0s), Gj, order, x_offs=[0, 0], batch=2, per_member_G0=True)
    per_d, per_v = lay.x_dim * lay.K, lc.po.jac_nnz_per_interval(lay) * lay.K
    assert c.n_rows == 2 * per_d and c.jac_nnz == 2 * per_v
    Zd = dev(Z)
    delta, vals = eval_jac_dev(c, Zd)
    mine = [(delta[b * per_d : (b + 1) * per_d], vals[b * per_v : (b + 1) * per_v]) for b in range(2)]
    for b in range(2):
        check(lay, mine[b], lc.truth("L1", order, drift=b), "members, order %d, member %d" % (order, b))
    c.set_member_window(1, 1)
    assert c.n_rows == per_d and c.jac_nnz == per_v
    bitwise(mine[1], eval_jac_dev(c, Zd), "the window on member 1")
    d2 = nans(c.n_rows)
    c.eval_dev(Zd, d2)
    c.sync()
    bitwise((mine[1][0],), (d2.cpu().numpy(),), "pcl_eval_dev in the window")
    c.close()
    one = make_ctx(lay, G0s[1], Gj, order)  # ... and what a context of that member alone gives
    bitwise(mine[1], eval_jac_dev(one, Zd), "member 1 alone")
    one.close()


@pytest.mark.parametrize("order", [4, 8])
def test_trajectory_seeds(order):
    """L7 (odd n) as two PCL_BATCH_TRAJ seeds."""
    lay, G0, Gj, _, _ = lc.case("L7")
    Zs = [lc.case("L7", s)[3] for s in range(2)]
    c = make_ctx(lay, G0, Gj, order, batch=2, batch_mode=pa._lib.PCL_BATCH_TRAJ)
    per_d, per_v = lay.x_dim * lay.K, lc.po.jac_nnz_per_interval(lay) * lay.K
    delta, vals = eval_jac_dev(c, dev(np.stack(Zs)))
    for s in range(2):
        check(lay, (delta[s * per_d : (s + 1) * per_d], vals[s * per_v : (s + 1) * per_v]), lc.truth("L7", order, seed=s), "seeds, order %d, seed %d" % (order, s))
    c.close()


# ---- host pointers, the order policy ---------------------------------------------------------------------------------------------------------------
def test_host_pointer_calls_give_the_bits_of_the_device_call():
    lay, G0, Gj, Z, _ = lc.case("L2")
    c = make_ctx(lay, G0, Gj, 10)
    dev_call = eval_jac_dev(c, dev(Z))
    c.set_stream(None)
    bitwise(dev_call, c.eval_jac(Z), "pcl_eval_jac")
    bitwise((dev_call[0],), (c.eval(Z),), "pcl_eval")
    bitwise((dev_call[1],), (c.jac(Z),), "pcl_jac")
    c.close()
    lay, G0, Gj, Z, _ = lc.case("L5")  # several columns: full values all the same (no compact path on a large context)
    c = make_ctx(lay, G0, Gj, 6)
    dev_call = eval_jac_dev(c, dev(Z))
    c.set_stream(None)
    bitwise(dev_call, c.eval_jac(Z), "pcl_eval_jac, five columns")
    c.close()


def test_order_policy():
    """pade_order = 0: the device-pointer call is refused until pcl_set_order_policy decides, and decides what pcl_order_for_bounds gives."""
    lay, G0, Gj, Z, _ = lc.case("L2")
    c = make_ctx(lay, G0, Gj, 0)
    with pytest.raises(pa.PclError) as ei:
        eval_jac_dev(c, dev(Z))
    assert ei.value.code == pa._lib.PCL_EINVAL
    L = pa._lib.load()
    L.pcl_order_for_bounds.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p,
                                       ctypes.c_double, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]  # fmt: skip
    g0, gj = np.ascontiguousarray(G0.T), np.ascontiguousarray(np.stack([g.T for g in Gj]))
    um = np.full(lay.m, 0.5)
    for dt_max, tol in ((0.02, 1e-10), (0.004, 1e-8)):
        th, od, met = ctypes.c_double(), ctypes.c_int32(), ctypes.c_int32()
        assert L.pcl_order_for_bounds(lay.n, lay.m, g0.ctypes.data, 1, gj.ctypes.data, dt_max, um.ctypes.data, tol, ctypes.byref(th), ctypes.byref(od), ctypes.byref(met)) == 0
        assert c.set_order_policy(dt_max, um, tol) == od.value == c.get_option("pade_order")
        print("L2: dt_max %.3f, tol %.0e: theta %.3f, order %d" % (dt_max, tol, th.value, od.value))
        got = eval_jac_dev(c, dev(Z))
        assert c.get_option("last_kernel") == 290 + od.value // 2
        check(lay, got, lc.truth("L2", od.value), "L2 at the policy's order %d" % od.value)
    c2 = make_ctx(lay, G0, Gj, 0)  # ... and from a trajectory on the host
    order = c2.set_order_from_trajectory(Z)
    assert order in lc.ORDERS and c2.get_option("pade_order") == order
    c2.close()
    c.close()


# ---- what a large context refuses -----------------------------------------------------------------------------------------------------------------
def test_refused_entry_points_name_the_flag():
    lay, G0, Gj, Z, _ = lc.case("L1")
    c = make_ctx(lay, G0, Gj, 4)
    L, h = c._L, c._h
    buf = torch.zeros(64, dtype=torch.float64, device="cuda")
    hb = np.zeros(64)
    ib = np.zeros(64, dtype=np.int64)
    p, hp = buf.data_ptr(), hb.ctypes.data
    i64 = ib.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    i32 = ib.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    vp, f64, p64 = ctypes.c_void_p, ctypes.c_double, ctypes.POINTER(ctypes.c_int64)
    L.pcl_set_goal_form.argtypes = [vp, ctypes.c_int32, ctypes.c_int32, vp, vp]
    L.pcl_objective_hess_nnz.argtypes = [vp, p64]
    L.pcl_objective_hess_structure.argtypes = [vp, p64, p64]
    L.pcl_objective_hess_dev.argtypes = L.pcl_objective_hess.argtypes = [vp, vp, f64, f64, vp]
    calls = {
        "pcl_hess_nnz": lambda: L.pcl_hess_nnz(h, i64, i64),
        "pcl_hess_structure": lambda: L.pcl_hess_structure(h, i32, i32),
        "pcl_hess_structure_i64": lambda: L.pcl_hess_structure_i64(h, i64, i64),
        "pcl_hess": lambda: L.pcl_hess(h, hp, hp, hp),
        "pcl_hess_dev": lambda: L.pcl_hess_dev(h, p, p, p),
        "pcl_jac_compact_nnz": lambda: L.pcl_jac_compact_nnz(h, i64, i64),
        "pcl_eval_jac_compact_dev": lambda: L.pcl_eval_jac_compact_dev(h, p, p, p),
        "pcl_jac_expand_dev": lambda: L.pcl_jac_expand_dev(h, p, p),
        "pcl_merit_grad_len": lambda: L.pcl_merit_grad_len(h, i64, i64),
        "pcl_merit_grad_dev": lambda: L.pcl_merit_grad_dev(h, p, p, p, p),
        "pcl_eval_jac_merit_dev": lambda: L.pcl_eval_jac_merit_dev(h, p, p, p, p, p),
        "pcl_eval_jac_merit_objective_dev": lambda: L.pcl_eval_jac_merit_objective_dev(h, p, p, p, p, p, 1.0, p, p),
        "pcl_rollout": lambda: L.pcl_rollout(h, hp, hp),
        "pcl_rollout_dev": lambda: L.pcl_rollout_dev(h, p, p),
        "pcl_set_goal": lambda: L.pcl_set_goal(h, hp),
        "pcl_set_goal_subspace": lambda: L.pcl_set_goal_subspace(h, hp, i32, 1),
        "pcl_set_goal_form": lambda: L.pcl_set_goal_form(h, 0, 1, hp, hp),
        "pcl_set_weights": lambda: L.pcl_set_weights(h, hp),
        "pcl_add_regularizer": lambda: L.pcl_add_regularizer(h, 0, 1, hp, 2),
        "pcl_clear_regularizers": lambda: L.pcl_clear_regularizers(h),
        "pcl_infidelity_dev": lambda: L.pcl_infidelity_dev(h, p, 1.0, p, p),
        "pcl_objective_dev": lambda: L.pcl_objective_dev(h, p, 1.0, p, p),
        "pcl_objective": lambda: L.pcl_objective(h, hp, 1.0, hp, hp),
        "pcl_objective_hess_nnz": lambda: L.pcl_objective_hess_nnz(h, i64),
        "pcl_objective_hess_structure": lambda: L.pcl_objective_hess_structure(h, i64, i64),
        "pcl_objective_hess_dev": lambda: L.pcl_objective_hess_dev(h, p, 1.0, 1.0, p),
        "pcl_objective_hess": lambda: L.pcl_objective_hess(h, hp, 1.0, 1.0, hp),
    }  # fmt: skip
    for name, call in calls.items():
        rc = call()
        msg = (L.pcl_last_error(h) or b"").decode()
        assert rc == ENOTIMPL and "PCL_LARGE_N" in msg and name.replace("_i64", "") in msg, (name, rc, msg)
    # ... and the served ones still work afterwards
    check(lay, eval_jac_dev(c, dev(Z)), lc.truth("L1", 4), "L1 after the refusals")
    rows, cols = c.jac_structure(np.int32)
    r64, c64 = c.jac_structure(np.int64)
    er, ec = lc.po.jac_structure(lay)
    assert np.array_equal(rows, er) and np.array_equal(cols, ec) and np.array_equal(r64, er) and np.array_equal(c64, ec)
    c.close()


# ---- the flag at n <= 64 --------------------------------------------------------------------------------------------------------------------------
def test_flag_at_54_gives_the_ordinary_context():
    lay, G0, Gj, Z, _ = vc.case("K5")
    Zd = dev(Z)
    out = []
    for flag in (False, True):
        c = make_ctx(lay, G0, Gj, 8, flag=flag)
        out.append(eval_jac_dev(c, Zd) + (c.get_option("last_kernel"), c.hess_nnz))
        c.close()
    assert out[0][2] == out[1][2] == 194 and out[0][3] == out[1][3] > 0  # the lock-step kernel of n <= 64; the Hessian is served
    bitwise(out[0][:2], out[1][:2], "flagged against unflagged at n = 54")


# ---- the Python keyword ----------------------------------------------------------------------------------------------------------------------------
def test_bilinear_integrator_keyword():
    """BilinearIntegrator(..., large_generator=True) on a d = 33 ket system: residual and Jacobian against the truth; the Hessian raises."""
    d, m, N = 33, 2, 4
    rng = np.random.default_rng(15500)
    H = vc._herm(d, rng)
    Hs = [vc._herm(d, rng) for _ in range(m)]
    s = pa.QuantumSystem(H, Hs, [1.0] * m)
    psi = rng.standard_normal(d) + 1j * rng.standard_normal(d)
    psi /= np.linalg.norm(psi)
    times = np.cumsum(np.concatenate(([0.0], 0.005 + 0.005 * rng.random(N - 1))))
    traj = pa.ket_trajectory(s, 0.3 * rng.standard_normal((m, N)), times, psi, psi)
    Z = traj.datavec.reshape(N, traj.dim).copy()
    Z[1:, : 2 * d] += 0.05 * rng.standard_normal((N - 1, 2 * d))  # an infeasible iterate: residuals of the states' size
    traj.update(Z.reshape(-1))
    KET = pa.trajectory.KET
    B = pa.BilinearIntegrator(s, traj, x_name=KET, pade_order=8, large_generator=True)
    assert B.x_dim == 2 * d and B.dim == 2 * d * (N - 1) and B.ctx.large
    lay = lc.po.Layout(d=d, m=m, N=N, z_dim=traj.dim, x_off=traj.components[KET].start, u_off=traj.components["u"].start,
                       dt_off=traj.components[traj.timestep].start, cols=1)  # fmt: skip
    G0, Gj = s.G_drift, s.G_drives_array()
    ref = tuple(a.astype(np.float64).reshape(-1) for a in vc.truth_values(lay, G0, Gj, Z, None, 8, hessian=False)[:2])
    got = B.ctx.eval_jac(traj.datavec)
    assert B.ctx.get_option("last_kernel") == 294
    check(lay, got, ref, "BilinearIntegrator, d = 33 ket")
    J = pa.eval_jacobian(B, traj)
    assert J.shape == (B.dim, traj.dim * N + traj.global_dim)
    with pytest.raises(pa.PclError) as ei:
        pa.eval_hessian_of_lagrangian(B, traj, np.ones(B.dim))
    assert ei.value.code == ENOTIMPL and "PCL_LARGE_N" in str(ei.value)
    B.close()
