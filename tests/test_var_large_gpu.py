"""The variational integrators at generator dimensions 66 .. 128 on the device (contexts created with PCL_BATCH_VARIATIONAL | PCL_LARGE_N |
PCL_LARGE_VAR; piccolo.jl_amd/csrc/pcl_kernel_var_large.hpp), at the cases of tests/var_large_cases.py (the case table and the branch each case
sits on are there), through the C ABI on device pointers.  Every value is compared with the longdouble truth on the lifted problem, rounded to
float64, at TOL = 1e-11 PER SEGMENT (row component x variable kind x relative knot x interval), relative to the segment's own maximum -- the
project's tolerance for every kernel family -- and a segment whose truth is identically zero must be exact zeros.
tests/test_var_large_cpu.py shows that the float64 lifted oracle agrees with that truth to 1e-13 on these inputs and that each case sees a zeroed
c_q, a dropped drive, a dropped state column, a zeroed Gv_v and a Gv term cut at k = 64 at 1e-7.

Without the feature every test here fails before the device is reached: the binding has no PCL_LARGE_VAR and its constructors do not know the
keywords (AttributeError / TypeError)."""
import numpy as np
import pytest
import torch

import piccolo_jl_amd as pa
import var_large_cases as vl

pytestmark = pytest.mark.gpu
TOL = 1e-11
L = pa._lib
NAN = float("nan")


def make_ctx(cs, order, large=True, **kw):
    c = pa.integrators._PclContext(**vl.context_args(cs, order, batch_mode=L.PCL_BATCH_VARIATIONAL, large_generator=large, large_variational=large, **kw))
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    return c


def plain_ctx(cs, order):
    """A plain PCL_LARGE_N context of the same drift and drives on component 0 of the same knots."""
    c = pa.integrators._PclContext(d=cs.n // 2, m=cs.m, N=cs.N, z_dim=cs.z_dim, u_off=cs.u_off, dt_off=cs.dt_off, x_offs=[cs.xo[0]], G0=cs.G0, Gj=cs.Gj,
                                   batch=1, batch_mode=L.PCL_BATCH_MEMBERS, pade_order=order, state_cols=cs.C, large_generator=True)  # fmt: skip
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


def bitwise(a, b, what):
    for x, y in zip(a, b):
        assert np.array_equal(x, y), what


def refused(code, word, f, *args):
    with pytest.raises(pa.PclError) as ei:
        f(*args)
    assert ei.value.code == code and word in str(ei.value), str(ei.value)


# ---- every case and order ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", vl.NAMES)
@pytest.mark.parametrize("order", vl.ORDERS)
def test_eval_jac_per_segment(name, order):
    """pcl_eval_jac_dev against the truth; pcl_eval_dev alone and pcl_jac_dev alone give its bits; which kernel ran; the structure."""
    cs, _ = vl.case(name)
    ref = vl.truth(name, order)
    q = order // 2
    c = make_ctx(cs, order)
    assert c.x_dim == cs.xd and c.n_rows == ref[0].size and c.jac_nnz == ref[1].size and c.jac_per == vl.values_per_interval(cs)
    assert c.hess_nnz == 0 and c.compact_nnz == 0 and c.get_option("large_variational") == 1 and c.get_option("variations") == cs.v
    Zd = dev(cs.Z)
    got = eval_jac_dev(c, Zd)
    assert c.get_option("last_kernel") == 340 + q
    assert not np.isnan(got[0]).any() and not np.isnan(got[1]).any()
    wd, wj = vl.check(name, order, got[0], got[1], TOL)
    print("%s order %d: residual %.1e (%s)  Jacobian %.1e (%s)" % (name, order, wd[0], wd[1], wj[0], wj[1]))
    d2 = nans(c.n_rows)
    c.eval_dev(Zd, d2)
    c.sync()
    assert c.get_option("last_kernel") == 350 + q
    bitwise((got[0],), (d2.cpu().numpy(),), "pcl_eval_dev alone")
    v2 = nans(c.jac_nnz)
    c.jac_dev(Zd, v2)
    c.sync()
    bitwise((got[1],), (v2.cpu().numpy(),), "pcl_jac_dev alone")
    bitwise(got, eval_jac_dev(c, Zd), "a second launch")
    if order == 6:
        r, cc = c.jac_structure()
        er, ec = vl.lib_structure(cs)
        assert np.array_equal(r, er) and np.array_equal(cc, ec)
    c.close()


def test_zero_step_segments_are_exact_zeros():
    """VL2's interval of Delta t = 0: its L blocks and its d/du tails are zeros exactly, its B blocks -I | I (the segment check asks for this too;
    here by position)."""
    cs, _ = vl.case("VL2")
    c = make_ctx(cs, 8)
    _, vals = eval_jac_dev(c, dev(cs.Z))
    n, C, v, m = cs.n, cs.C, cs.v, cs.m
    blk = vals.reshape(cs.K, -1)[3, : (2 + 4 * v) * C * n * n].reshape(2 + 4 * v, C, n * n)
    eye = np.eye(n).reshape(-1)
    for b in range(1, v + 1):
        assert not blk[4 * b].any() and not blk[4 * b + 1].any()
    for s in [0] + [4 * b - 2 for b in range(1, v + 1)]:
        assert np.array_equal(blk[s], np.tile(-eye, (C, 1))) and np.array_equal(blk[s + 1], np.tile(eye, (C, 1)))
    tails = vals.reshape(cs.K, -1)[3, (2 + 4 * v) * C * n * n :].reshape((1 + v) * C, m + 1, n)
    assert not tails[:, :m].any() and tails[:, m].any()
    c.close()


# ---- host pointers ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["VL1", "VL2"])
def test_host_pointer_calls_deliver_the_same_bits(name):
    cs, _ = vl.case(name)
    c = make_ctx(cs, 6)
    first = eval_jac_dev(c, dev(cs.Z))
    Z = cs.Z.reshape(-1)
    d, v = c.eval_jac(Z, np.full(c.n_rows, NAN), np.full(c.jac_nnz, NAN))
    bitwise(first, (d, v), "pcl_eval_jac")
    bitwise((first[0],), (c.eval(Z, np.full(c.n_rows, NAN)),), "pcl_eval")
    bitwise((first[1],), (c.jac(Z, np.full(c.jac_nnz, NAN)),), "pcl_jac")
    c.close()


# ---- every split -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["VL2", "VL5"])
@pytest.mark.parametrize("order", [4, 10])
def test_every_split_bitwise(name, order):
    """cols_per_slice, general_slices and var_large_drives, one at a time and together; var_block_wgs / var_col_wgs change nothing."""
    cs, _ = vl.case(name)
    c = make_ctx(cs, order)
    Zd = dev(cs.Z)
    first = eval_jac_dev(c, Zd)
    vl.check(name, order, first[0], first[1], TOL)

    def same(what):
        bitwise(first, eval_jac_dev(c, Zd), what)
        d2 = nans(c.n_rows)
        c.eval_dev(Zd, d2)
        c.sync()
        bitwise((first[0],), (d2.cpu().numpy(),), ("pcl_eval_dev", what))

    for cp in (1, 2, cs.C, 0):
        c.set_option("cols_per_slice", cp)
        same(("cols_per_slice", cp))
    for s in (1, 10**6, 0):
        c.set_option("general_slices", s)
        same(("general_slices", s))
    for g in (1, 5, max(cs.m, 1), 0):
        c.set_option("var_large_drives", g)
        assert c.get_option("var_large_drives") == g
        same(("var_large_drives", g))
    c.set_option("cols_per_slice", 2)
    c.set_option("general_slices", 7)
    c.set_option("var_large_drives", 2)
    same("all three")
    c.set_option("var_block_wgs", 3)
    c.set_option("var_col_wgs", 5)
    same("var_block_wgs / var_col_wgs")
    assert c.get_option("last_kernel") == 350 + order // 2
    refused(L.PCL_EINVAL, "var_large_drives", c.set_option, "var_large_drives", -1)
    c.close()


# ---- component 0 has the bits of a plain large context -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["VL2", "VL3"])
@pytest.mark.parametrize("order", [4, 10])
def test_component_0_has_the_bits_of_a_plain_large_context(name, order):
    """delta_0, component 0's tails and the -B+ | B- copies of EVERY component against a PCL_LARGE_N context of the same drift and drives."""
    cs, _ = vl.case(name)
    Zd = dev(cs.Z)
    c = make_ctx(cs, order)
    d, v = eval_jac_dev(c, Zd)
    c.close()
    p = plain_ctx(cs, order)
    assert p.get_option("large_variational") == 0
    d0, v0 = eval_jac_dev(p, Zd)
    assert p.get_option("last_kernel") == 290 + order // 2
    p.close()
    dv, dp, jv, jp = vl.component0(cs)
    assert len(np.unique(dp)) == d0.size and len(np.unique(jp)) == v0.size
    assert np.array_equal(d[dv], d0[dp]), "delta_0"
    assert np.array_equal(v[jv], v0[jp]), "the -B+ | B- copies and component 0's tails"


def test_largest_value_count_is_written_everywhere():
    """n = 128 unitary, v = 2: 10.5 M values per interval, no truth (tests/var_large_cases.py): nothing stays NaN, and component 0 has the plain
    context's bits."""
    cs = vl.case_vl7()
    Zd = dev(cs.Z)
    c = make_ctx(cs, 4)
    assert c.jac_per == 10534912
    d, v = eval_jac_dev(c, Zd)
    c.close()
    assert not np.isnan(d).any() and not np.isnan(v).any()
    p = plain_ctx(cs, 4)
    d0, v0 = eval_jac_dev(p, Zd)
    p.close()
    dv, dp, jv, jp = vl.component0(cs)
    assert np.array_equal(d[dv], d0[dp]) and np.array_equal(v[jv], v0[jp])
    nn = cs.n * cs.n
    Lb = v[: 10 * cs.C * nn].reshape(10, cs.C, nn)
    for s in (4, 5, 8, 9):  # the L blocks: 64 equal copies, not zero
        assert Lb[s, 0].any() and np.array_equal(Lb[s], np.tile(Lb[s, 0], (cs.C, 1)))


# ---- the flags at n <= 64 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ket", [True, False])
def test_flags_at_n_54_change_nothing(ket):
    import variational_truth as vt

    rng = np.random.default_rng(54)
    d, v, m = 27, 2, 2
    n, C = 2 * d, (1 if ket else d)
    G = lambda: vl.po.G_of_H(vl.vsc._herm(d, rng))
    G0, Gj, Gv = G(), np.array([G() for _ in range(m)]), [G() / 3.0, G() / 0.25]
    xdc = n * C
    Z = 0.4 * rng.standard_normal((3, 3 * xdc + 2 + m))
    Z[:, 3 * xdc] = 0.05
    cs = vt.VarCase(Z=Z, z_dim=Z.shape[1], N=3, n=n, C=C, m=m, xo=[0, xdc, 2 * xdc], u_off=3 * xdc + 2, dt_off=3 * xdc, G0=G0, Gv=Gv, Gj=Gj)
    Zd = dev(Z)
    out = []
    for large in (False, True):
        c = make_ctx(cs, 8, large=large)
        assert c.get_option("large_variational") == 0
        out.append(eval_jac_dev(c, Zd) + (c.get_option("last_kernel"), c.hess(Z.reshape(-1), np.linspace(-1.0, 1.0, c.n_rows))))
        c.close()
    assert out[0][2] == out[1][2] == 70
    bitwise(out[0][:2] + out[0][3:], out[1][:2] + out[1][3:], "the three flags at n = 54")


# ---- the order policy ------------------------------------------------------------------------------------------------------------------------------------
def test_order_policy():
    """pade_order = 0: device-pointer calls are refused until a policy is set; the policy looks at the lifted generator; the host-pointer call decides
    from the trajectory."""
    cs, _ = vl.case("VL1")
    c = make_ctx(cs, 0)
    Zd = dev(cs.Z)
    refused(L.PCL_EINVAL, "pade_order = 0", c.eval_dev, Zd, nans(c.n_rows))
    u_max = np.abs(cs.Z[:, cs.u_off : cs.u_off + cs.m]).max(axis=0)
    order = c.set_order_policy(float(np.abs(cs.Z[:, cs.dt_off]).max()), u_max, 1e-9)
    assert order in (6, 8, 10) and c.pade_order == order
    got = eval_jac_dev(c, Zd)
    assert c.get_option("last_kernel") == 340 + order // 2
    vl.check("VL1", order, got[0], got[1], TOL)
    c.close()
    c = make_ctx(cs, 0)
    d = c.eval(cs.Z.reshape(-1))
    assert c.pade_order in (4, 6, 8, 10)
    bitwise((d,), (make_and_eval(cs, c.pade_order, Zd),), "the order the trajectory chose")
    c.close()


def make_and_eval(cs, order, Zd):
    c = make_ctx(cs, order)
    d = nans(c.n_rows)
    c.eval_dev(Zd, d)
    c.sync()
    out = d.cpu().numpy()
    c.close()
    return out


# ---- what stays refused ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_flag():
    cs, _ = vl.case("VL1")
    c = make_ctx(cs, 8)
    Zd, mu = dev(cs.Z), dev(np.ones(c.n_rows))
    buf = nans(16)
    E, W = L.PCL_ENOTIMPL, "PCL_LARGE_VAR"
    refused(E, W, c.hess, cs.Z.reshape(-1), np.ones(c.n_rows), np.zeros(16))
    refused(E, W, c.hess_dev, Zd, mu, buf)
    refused(E, W, c.hess_structure)
    import ctypes

    a, b = ctypes.c_int64(), ctypes.c_int64()
    for f in ("pcl_hess_nnz", "pcl_jac_compact_nnz", "pcl_merit_grad_len"):
        assert getattr(c._L, f)(c._h, ctypes.byref(a), ctypes.byref(b)) == E and W in c._L.pcl_last_error(c._h).decode(), f
    refused(E, W, c.set_option, "var_full", 1)
    refused(E, W, c.set_option, "var_compact", 1)
    assert c.get_option("var_full") == 0 and c.get_option("var_compact") == 0
    refused(E, W, c.rollout, cs.Z.reshape(-1))
    refused(E, W, c.set_member_window, 0, 1)
    refused(E, W, c.set_weights, np.ones(1 + cs.v))
    refused(E, W, c.set_goal, np.zeros(cs.xdc))
    for f, args in (("pcl_eval_jac_compact_dev", (Zd, buf, buf)), ("pcl_jac_expand_dev", (buf, buf)), ("pcl_merit_grad_dev", (Zd, buf, buf, buf)),
                    ("pcl_eval_jac_merit_dev", (Zd, buf, buf, buf, buf)), ("pcl_rollout_dev", (Zd, buf))):  # fmt: skip
        rc = getattr(c._L, f)(c._h, *[ctypes.c_void_p(t.data_ptr()) for t in args])
        assert rc == E and W in c._L.pcl_last_error(c._h).decode(), (f, rc, c._L.pcl_last_error(c._h))
    rc = c._L.pcl_infidelity_dev(c._h, ctypes.c_void_p(Zd.data_ptr()), ctypes.c_double(1.0), ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(buf.data_ptr()))
    assert rc == E and W in c._L.pcl_last_error(c._h).decode()
    # the other families' options: each with its own code for "not that kind of context"
    for key in ("large_hess", "large_full", "large_reduce", "large_exp_hess", "large_exp_reduce"):
        refused(L.PCL_EINVAL, key, c.set_option, key, 1)
        assert c.get_option(key) == 0
    # ... and the new option off such a context
    p = plain_ctx(cs, 8)
    refused(L.PCL_EINVAL, "var_large_drives", p.set_option, "var_large_drives", 1)
    p.close()
    got = eval_jac_dev(c, Zd)  # (nothing above left the context unusable)
    vl.check("VL1", 8, got[0], got[1], TOL)
    c.close()


# ---- the public constructors -----------------------------------------------------------------------------------------------------------------------------
def test_public_constructor_end_to_end():
    """VariationalKetIntegrator(..., large_generator=True, pade_order=8) on VL1's system (d = 33): residual and Jacobian through the mirror against
    the truth; the Hessian, the rollout and the objective switch raise the library's message."""
    cs, _ = vl.case("VL1")
    H0, Hd, Hv = vl.hamiltonians("VL1")
    sysv = pa.VariationalQuantumSystem(H0, list(Hd), list(Hv), [1.0] * cs.m)
    comps = {"ψ̃": cs.Z[:, cs.xo[0] : cs.xo[0] + cs.xdc].T, "ψ̃_var": cs.Z[:, cs.xo[1] : cs.xo[1] + cs.xdc].T, "Δt": cs.Z[:, cs.dt_off][None],
             "t": cs.Z[:, cs.dt_off + 1][None], "u": cs.Z[:, cs.u_off : cs.u_off + cs.m].T}  # fmt: skip
    traj = pa.NamedTrajectory(comps, controls=("u", "Δt"), timestep="Δt")
    assert np.array_equal(traj.datavec, cs.Z.reshape(-1))
    with pytest.raises(pa.PclError, match="exceeds 32"):  # without the keyword: as ever
        pa.VariationalKetIntegrator(sysv, traj, "ψ̃", ["ψ̃_var"], "u", scale=vl.SCALES[0], pade_order=8)
    B = pa.VariationalKetIntegrator(sysv, traj, "ψ̃", ["ψ̃_var"], "u", scale=vl.SCALES[0], pade_order=8, large_generator=True)
    assert B.ctx.large_variational and B.pade_order == 8 and B.dim == cs.K * cs.xd
    delta, vals = B.ctx.eval_jac(traj.datavec)
    wd, wj = vl.check("VL1", 8, delta, vals, TOL, "through the public constructor")
    print("VariationalKetIntegrator, large_generator=True: residual %.1e  Jacobian %.1e" % (wd[0], wj[0]))
    out = np.zeros(B.dim)
    pa.evaluate_(out, B, traj)
    assert np.array_equal(out, delta)
    for f, args in ((pa.hessian_structure, (B,)), (B.rollout, (traj,)), (B.enable_objective_and_rollout, ()), (B.ctx.hess, (traj.datavec, np.ones(B.dim), np.zeros(16)))):
        with pytest.raises(pa.PclError, match="PCL_LARGE_VAR") as ei:
            f(*args)
        assert ei.value.code == L.PCL_ENOTIMPL
    B.close()
