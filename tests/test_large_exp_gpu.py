"""The exponential constraint at generator dimensions 66 .. 128 on the device (contexts created with PCL_LARGE_N | PCL_LARGE_EXP and pade_order =
PCL_ORDER_EXP; piccolo.jl_amd/csrc/pcl_kernel_large_exp.hpp), at the cases of tests/large_exp_cases.py, through the C ABI on device pointers.
Every value is compared with scipy's expm / expm_frechet (the committed oracle, mapped by tests/exp_truth.py) at TOL = 1e-11 PER SEGMENT of every
interval, relative to the segment's own maximum with no floor at 1 (shape_cases.check_segments) -- the project's tolerance for every kernel
family.  tests/test_large_exp_cpu.py shows that the kernel's recurrence in float64 agrees with that truth to 1e-13 on these inputs and that each
case sees a dropped substep, a dropped k range beyond 64, a zeroed last row tile, a dropped drive, a dropped state column and G_l V taken with
the updated V at 1e-7.

Without the feature every test here fails at pcl_create (the flag is an unknown batch mode)."""
import ctypes

import numpy as np
import pytest
import torch

import exp_truth as xt
import large_exp_cases as le
import piccolo_jl_amd as pa
from shape_cases import check_segments

pytestmark = pytest.mark.gpu
TOL = 1e-11
ENOTIMPL, EINVAL = pa._lib.PCL_ENOTIMPL, pa._lib.PCL_EINVAL
MEMBERS, TRAJ = pa._lib.PCL_BATCH_MEMBERS, pa._lib.PCL_BATCH_TRAJ
NAN = float("nan")


def make_ctx(lay, G0, Gj, order="exp", **kw):
    args = dict(d=lay.d, m=lay.m, N=lay.N, z_dim=lay.z_dim, u_off=lay.u_off, dt_off=lay.dt_off, x_offs=[lay.x_off], G0=G0, Gj=Gj, batch=1,
                batch_mode=MEMBERS, pade_order=order, large_generator=True, large_exp=order == "exp")  # fmt: skip
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


def eval_dev(c, Zd):
    dd = nans(c.n_rows)
    c.eval_dev(Zd, dd)
    c.sync()
    return dd.cpu().numpy()


def worst(errs):
    s = max(errs, key=errs.get)
    return "%.1e (%s)" % (errs[s], s)


def check(lay, got, ref, what):
    """got, ref: (delta, values).  No NaN may remain; every segment of every interval within TOL of the truth."""
    assert not np.isnan(got[0]).any() and not np.isnan(got[1]).any(), what
    er = check_segments(got[0], ref[0], le.residual_labels(lay), TOL)
    ej = check_segments(got[1], ref[1], le.jac_labels(lay), TOL)
    print("%s: residual %s  Jacobian %s" % (what, worst(er), worst(ej)))
    assert max(er.values()) <= TOL and max(ej.values()) <= TOL, (what, er, ej)


def bitwise(a, b, what):
    for x, y in zip(a, b):
        assert np.array_equal(x, y), what


# ---- every case ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", le.NAMES)
def test_eval_jac_per_segment(name):
    """pcl_eval_jac_dev against the truth; the structure; pcl_eval_dev alone and pcl_jac_dev alone give its bits; two launches; which kernel ran."""
    lay, G0, Gj, Z = le.case(name)
    ref = le.truth(name)
    c = make_ctx(lay, G0, Gj)
    assert c.large and c.large_exp and c.exponential
    assert c.n_rows == ref[0].size and c.jac_nnz == ref[1].size and c.jac_per == xt.nnz_per_interval(lay) and c.hess_nnz == 0 and c.compact_nnz == 0
    assert c.get_option("pade_order") == -1
    Zd = dev(Z)
    got = eval_jac_dev(c, Zd)
    assert c.get_option("last_kernel") == 320
    check(lay, got, ref, name)
    d2 = eval_dev(c, Zd)
    assert c.get_option("last_kernel") == 321
    bitwise((got[0],), (d2,), "pcl_eval_dev alone")
    v2 = nans(c.jac_nnz)
    c.jac_dev(Zd, v2)
    c.sync()
    assert c.get_option("last_kernel") == 320
    bitwise((got[1],), (v2.cpu().numpy(),), "pcl_jac_dev alone")
    bitwise(got, eval_jac_dev(c, Zd), "a second launch")
    er, ec = xt.structure(lay)
    for dt in (np.int32, np.int64):
        rows, cols = c.jac_structure(dt)
        assert np.array_equal(rows, er) and np.array_equal(cols, ec), dt
    c.close()


# ---- every split gives the same bits ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["L4", "L5", "L6"])
def test_slicings_bitwise(name):
    """cols_per_slice in {1, 2, 0}, general_slices in {0, n}, a forced smaller drive group (large_exp_drives), and several at once."""
    kind, n, cols, m = le.CASES[name]
    lay, G0, Gj, Z = le.case(name)
    c = make_ctx(lay, G0, Gj)
    Zd = dev(Z)
    first = eval_jac_dev(c, Zd)
    check(lay, first, le.truth(name), name)
    for cp in (1, 2, 0):
        c.set_option("cols_per_slice", cp)
        bitwise(first, eval_jac_dev(c, Zd), ("cols_per_slice", cp))
        bitwise((first[0],), (eval_dev(c, Zd),), ("pcl_eval_dev, cols_per_slice", cp))
    for s in (n, 0):
        c.set_option("general_slices", s)
        bitwise(first, eval_jac_dev(c, Zd), ("general_slices", s))
    for g in sorted({1, 2, m}):
        c.set_option("large_exp_drives", g)
        assert c.get_option("large_exp_drives") == g
        bitwise(first, eval_jac_dev(c, Zd), ("large_exp_drives", g))
    c.set_option("cols_per_slice", 2)  # all at once
    c.set_option("general_slices", 7)
    bitwise(first, eval_jac_dev(c, Zd), "the three options at once")
    assert c.get_option("last_kernel") == 320
    with pytest.raises(pa.PclError) as ei:
        c.set_option("large_exp_drives", -1)
    assert ei.value.code == EINVAL
    c.close()


# ---- the zero step ----------------------------------------------------------------------------------------------------------------------------------
def test_zero_step():
    """L1 with h = 0 on interval 1: E = I and zero drive tails exactly, delta = X_{k+1} - X_k, the dt tail -G X_k; the other intervals as ever."""
    lay, G0, Gj, Z = le.case("L1z")
    n, m, xd = lay.n, lay.m, lay.x_dim
    c = make_ctx(lay, G0, Gj)
    got = eval_jac_dev(c, dev(Z))
    check(lay, got, le.truth("L1z"), "L1 with a zero step")
    per = xt.nnz_per_interval(lay)
    v = got[1][per : 2 * per]
    assert np.array_equal(v[: n * n], -np.eye(n).reshape(-1)), "E = I"
    assert np.array_equal(v[n * n : n * n + xd], np.ones(xd))
    tail = v[n * n + xd :].reshape(m + 1, n)
    assert not tail[:m].any(), "zero drive tails"
    assert tail[m].any()
    assert np.array_equal(got[0][xd : 2 * xd], Z[2, :xd] - Z[1, :xd])
    c.close()


# ---- batched launches -------------------------------------------------------------------------------------------------------------------------------
def test_members_with_their_own_drifts_and_the_window():
    """L5 as two PCL_BATCH_MEMBERS members with per-member drifts: each against its own truth; the window on the second alone gives its bits."""
    lay, _, Gj, Z = le.case("L5")
    G0s = [le.case("L5", 0, b)[1] for b in range(2)]
    c = make_ctx(lay, np.array(G0s), Gj, x_offs=[0, 0], batch=2, per_member_G0=True)
    per_d, per_v = lay.x_dim * lay.K, xt.nnz_per_interval(lay) * lay.K
    assert c.n_rows == 2 * per_d and c.jac_nnz == 2 * per_v
    Zd = dev(Z)
    delta, vals = eval_jac_dev(c, Zd)
    mine = [(delta[b * per_d : (b + 1) * per_d], vals[b * per_v : (b + 1) * per_v]) for b in range(2)]
    for b in range(2):
        check(lay, mine[b], le.truth("L5", drift=b), "members, member %d" % b)
    c.set_member_window(1, 1)
    assert c.n_rows == per_d and c.jac_nnz == per_v
    bitwise(mine[1], eval_jac_dev(c, Zd), "the window on member 1")
    bitwise((mine[1][0],), (eval_dev(c, Zd),), "pcl_eval_dev in the window")
    c.close()
    one = make_ctx(lay, G0s[1], Gj)  # ... and what a context of that member alone gives
    bitwise(mine[1], eval_jac_dev(one, Zd), "member 1 alone")
    one.close()


def test_trajectory_seeds():
    """L7 (odd n) as two PCL_BATCH_TRAJ seeds; the window on the second."""
    lay, G0, Gj, _ = le.case("L7")
    Zs = [le.case("L7", s)[3] for s in range(2)]
    c = make_ctx(lay, G0, Gj, batch=2, batch_mode=TRAJ)
    per_d, per_v = lay.x_dim * lay.K, xt.nnz_per_interval(lay) * lay.K
    Zd = dev(np.stack(Zs))
    delta, vals = eval_jac_dev(c, Zd)
    mine = [(delta[s * per_d : (s + 1) * per_d], vals[s * per_v : (s + 1) * per_v]) for s in range(2)]
    for s in range(2):
        check(lay, mine[s], le.truth("L7", seed=s), "seeds, seed %d" % s)
    c.set_member_window(1, 1)
    bitwise(mine[1], eval_jac_dev(c, Zd), "the window on seed 1")
    c.close()


# ---- host pointers ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["L2", "L5"])
def test_host_pointer_calls_give_the_bits_of_the_device_call(name):
    """(L5, several columns: full values all the same -- no compact path on such a context)"""
    lay, G0, Gj, Z = le.case(name)
    c = make_ctx(lay, G0, Gj)
    dev_call = eval_jac_dev(c, dev(Z))
    c.set_stream(None)
    bitwise(dev_call, c.eval_jac(Z), "pcl_eval_jac")
    bitwise((dev_call[0],), (c.eval(Z),), "pcl_eval")
    bitwise((dev_call[1],), (c.jac(Z),), "pcl_jac")
    c.close()


# ---- what such a context refuses ------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_flag():
    lay, G0, Gj, Z = le.case("L1")
    c = make_ctx(lay, G0, Gj)
    L, h = c._L, c._h
    buf = torch.zeros(64, dtype=torch.float64, device="cuda")
    hb = np.zeros(64)
    ib = np.zeros(64, dtype=np.int64)
    p, hp = buf.data_ptr(), hb.ctypes.data
    i64 = ib.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    i32 = ib.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
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
        "pcl_rollout_dev": lambda: L.pcl_rollout_dev(h, p, p),  # (without the option large_full)
        "pcl_objective_dev": lambda: L.pcl_objective_dev(h, p, 1.0, p, p),
    }  # fmt: skip
    for name, call in calls.items():
        rc = call()
        msg = (L.pcl_last_error(h) or b"").decode()
        assert rc == ENOTIMPL and "PCL_LARGE_EXP" in msg and name.replace("_i64", "") in msg, (name, rc, msg)
    for key in ("exp_hess", "large_hess", "exp_full", "large_reduce"):
        with pytest.raises(pa.PclError) as ei:
            c.set_option(key, 1)
        assert ei.value.code == ENOTIMPL and "PCL_LARGE_EXP" in str(ei.value) and key in str(ei.value), (key, str(ei.value))
        c.set_option(key, 0)
        assert c.get_option(key) == 0
    with pytest.raises(pa.PclError) as ei:
        c.set_order_policy(0.01, np.full(lay.m, 0.5), 1e-10)
    assert ei.value.code == EINVAL and "exponential" in str(ei.value)
    with pytest.raises(pa.PclError) as ei:
        c.set_order_from_trajectory(Z)
    assert ei.value.code == EINVAL and "exponential" in str(ei.value)
    c.set_option("large_full", 1)  # the fused call needs the reduce payload as well, which cannot be had: refused with large_full on, too
    rc = calls["pcl_eval_jac_merit_objective_dev"]()
    msg = (L.pcl_last_error(h) or b"").decode()
    assert rc == ENOTIMPL and "PCL_LARGE_EXP" in msg, (rc, msg)
    c.set_option("large_full", 0)
    # ... and the served ones still work afterwards
    check(lay, eval_jac_dev(c, dev(Z)), le.truth("L1"), "L1 after the refusals")
    c.close()


# ---- large_full: objective and rollout do not depend on the constraint -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["L1", "L6"])
def test_large_full_gives_the_bits_of_a_pade_context(name):
    """The rollout and the objective's value and gradient equal, bitwise, those of a large Pade context (pade_order 8, large_full) on the same
    system and trajectory; the rows are served beside them."""
    lay, G0, Gj, Z = le.case(name)
    rng = np.random.default_rng(31)
    goal = rng.standard_normal(lay.x_dim)
    goal /= np.linalg.norm(goal) / np.sqrt(lay.C)
    R = 0.5 + rng.random(lay.m)
    out = []
    for order in ("exp", 8):
        c = make_ctx(lay, G0, Gj, order, large_full=True)
        assert c.large and c.large_full and c.large_exp == (order == "exp")
        if lay.C == lay.d:  # a unitary state: a matrix goal; a ket: the form F = (a_1'x)^2 + (a_2'x)^2
            c.set_goal(goal)
        else:
            c.set_goal_form(0, np.stack([goal, np.roll(goal, lay.n // 2) * np.repeat([-1.0, 1.0], lay.n // 2)]), None)
        c.add_regularizer(lay.u_off, lay.m, R, 1)
        Zd = dev(Z)
        xo, vd, gd = nans(lay.N * lay.x_dim), nans(1), nans(Z.size)
        c.rollout_dev(Zd, xo)
        c.objective_dev(Zd, 100.0, vd, gd)
        c.sync()
        out.append((xo.cpu().numpy(), vd.cpu().numpy(), gd.cpu().numpy()))
        assert not any(np.isnan(a).any() for a in out[-1])
        if order == "exp":
            check(lay, eval_jac_dev(c, Zd), le.truth(name), "%s beside large_full" % name)
            assert c.get_option("last_kernel") == 320
        c.close()
    bitwise(out[0], out[1], "exponential against Pade context, %s" % name)
    assert np.abs(out[0][2]).max() > 0


# ---- both flags at n <= 64 --------------------------------------------------------------------------------------------------------------------------
def test_flags_at_54_give_the_ordinary_exponential_context():
    import vector_shape_cases as vc

    lay, G0, Gj, Z, _ = vc.case("K5")
    Zd = dev(Z)
    out = []
    for flags in (False, True):
        c = make_ctx(lay, G0, Gj, large_generator=flags, large_exp=flags)
        assert not c.large and not c.large_exp
        out.append(eval_jac_dev(c, Zd) + (c.get_option("last_kernel"),))
        c.close()
    assert out[0][2] == out[1][2] == 100  # the exponential kernel of n <= 64
    bitwise(out[0][:2], out[1][:2], "flagged against unflagged at n = 54")


# ---- the Python keyword -------------------------------------------------------------------------------------------------------------------------------
def test_bilinear_integrator_keyword():
    """BilinearIntegrator(..., pade_order="exp", large_generator=True, large_exp=True) on a d = 33 ket system: residual and Jacobian against
    the truth; the Hessian raises."""
    import vector_shape_cases as vc
    from oracle import pade_oracle as po

    d, m, N = 33, 2, 4
    rng = np.random.default_rng(25500)
    s = pa.QuantumSystem(vc._herm(d, rng), [vc._herm(d, rng) for _ in range(m)], [1.0] * m)
    psi = rng.standard_normal(d) + 1j * rng.standard_normal(d)
    psi /= np.linalg.norm(psi)
    times = np.cumsum(np.concatenate(([0.0], 0.05 + 0.05 * rng.random(N - 1))))
    traj = pa.ket_trajectory(s, 0.3 * rng.standard_normal((m, N)), times, psi, psi)
    Z = traj.datavec.reshape(N, traj.dim).copy()
    Z[1:, : 2 * d] += 0.05 * rng.standard_normal((N - 1, 2 * d))  # an infeasible iterate: residuals of the states' size
    traj.update(Z.reshape(-1))
    KET = pa.trajectory.KET
    B = pa.BilinearIntegrator(s, traj, x_name=KET, pade_order="exp", large_generator=True, large_exp=True)
    assert B.x_dim == 2 * d and B.dim == 2 * d * (N - 1) and B.ctx.large and B.ctx.large_exp
    lay = po.Layout(d=d, m=m, N=N, z_dim=traj.dim, x_off=traj.components[KET].start, u_off=traj.components["u"].start,
                    dt_off=traj.components[traj.timestep].start, cols=1)  # fmt: skip
    G0, Gj = s.G_drift, s.G_drives_array()
    ref = (po.exp_residual(Z, lay, G0, Gj).reshape(-1), xt.values(Z, lay, G0, Gj).reshape(-1))
    got = B.ctx.eval_jac(traj.datavec)
    assert B.ctx.get_option("last_kernel") == 320
    check(lay, got, ref, "BilinearIntegrator, d = 33 ket")
    J = pa.eval_jacobian(B, traj)
    assert J.shape == (B.dim, traj.dim * N + traj.global_dim)
    with pytest.raises(pa.PclError) as ei:
        pa.eval_hessian_of_lagrangian(B, traj, np.ones(B.dim))
    assert ei.value.code == ENOTIMPL and "PCL_LARGE_EXP" in str(ei.value)
    B.close()
