"""The Hessian of the Lagrangian of large variational contexts on the device (PCL_BATCH_VARIATIONAL | PCL_LARGE_N | PCL_LARGE_VAR with option
large_var_hess; piccolo.jl_amd/csrc/pcl_kernel_var_large_hess.hpp), at the cases of tests/var_large_hess_cases.py, through the C ABI on device
pointers.  Every value is compared with the longdouble truth on the lifted problem, rounded to float64, at TOL = 1e-11 PER SEGMENT (variable
kinds x relative knot x interval), relative to the segment's own maximum -- the project's tolerance for every kernel family -- and a segment
whose truth is identically zero must be exact zeros.  tests/test_var_large_hess_cpu.py shows that the float64 lifted oracle and the restated
pass formulation agree with that truth to 1e-13 on these inputs and that each case sees a zeroed c_q, a dropped drive, a dropped state
column, a zeroed Gv_v and a dropped pass v at 1e-7.

Without the feature every test here fails at set_option("large_var_hess", ..) (unknown option) or at the keyword (TypeError)."""
import ctypes

import numpy as np
import pytest
import torch

import piccolo_jl_amd as pa
import var_large_cases as vl
import var_large_hess_cases as vh
import variational_truth as vt

pytestmark = pytest.mark.gpu
TOL = 1e-11
L = pa._lib
NAN = float("nan")
REFUSAL = "residual and Jacobian only"


def make_ctx(cs, order, hess=True, **kw):
    c = pa.integrators._PclContext(**vl.context_args(cs, order, batch_mode=L.PCL_BATCH_VARIATIONAL, large_generator=True, large_variational=True,
                                                     large_var_hessian=hess, **kw))  # fmt: skip
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    return c


def plain_ctx(cs, order):
    """A plain PCL_LARGE_N context with large_hess of the same drift and drives on component 0 of the same knots."""
    c = pa.integrators._PclContext(d=cs.n // 2, m=cs.m, N=cs.N, z_dim=cs.z_dim, u_off=cs.u_off, dt_off=cs.dt_off, x_offs=[cs.xo[0]], G0=cs.G0, Gj=cs.Gj,
                                   batch=1, batch_mode=L.PCL_BATCH_MEMBERS, pade_order=order, state_cols=cs.C, large_generator=True, large_hessian=True)  # fmt: skip
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    return c


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float64).reshape(-1)).cuda()


def nans(k):
    return torch.full((k,), NAN, dtype=torch.float64, device="cuda")


def hess_dev(c, Zd, mud):
    """The values of pcl_hess_dev into a NaN-filled array, as numpy."""
    out = nans(c.hess_nnz)
    c.hess_dev(Zd, mud, out)
    c.sync()
    return out.cpu().numpy()


def refused(code, word, f, *args):
    with pytest.raises(pa.PclError) as ei:
        f(*args)
    assert ei.value.code == code and word in str(ei.value), str(ei.value)


# ---- every case and order ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", vh.NAMES)
@pytest.mark.parametrize("order", vh.ORDERS)
def test_hess_per_segment(name, order):
    """pcl_hess_dev against the truth; which kernel ran; a second launch and the host-pointer pcl_hess give its bits."""
    cs = vh.case(name)
    ref = vh.truth(name, order)
    c = make_ctx(cs, order)
    assert c.large_var_hessian and c.get_option("large_var_hess") == 1
    assert c.hess_per == vh.values_per_interval(cs) and c.hess_nnz == ref.size
    Zd, mud = dev(cs.Z), dev(vh.rand_mu(name))
    got = hess_dev(c, Zd, mud)
    assert c.get_option("last_hess_kernel") == 340 + order // 2
    assert not np.isnan(got).any()
    w = vh.check(name, order, got, TOL)
    print("%s order %d: Hessian %.1e (%s)" % (name, order, w[0], w[1]))
    assert np.array_equal(got, hess_dev(c, Zd, mud)), "a second launch"
    host = np.full(c.hess_nnz, NAN)
    c.hess(cs.Z.reshape(-1), vh.rand_mu(name), host)
    assert np.array_equal(got, host), "pcl_hess on host pointers"
    c.close()


def test_exact_zeros():
    """(u,u) and (h,h) at order 2, and every segment that is identically zero on VL2's Delta t = 0 interval."""
    for name in ("VL2", "VL5"):
        cs = vh.case(name)
        c = make_ctx(cs, 2)
        got = hess_dev(c, dev(cs.Z), dev(vh.rand_mu(name))).reshape(cs.K, -1)
        nscal, m = (cs.m + 1) * (cs.m + 2) // 2, cs.m
        assert np.all(got[:, : m * (m + 1) // 2] == 0.0) and np.all(got[:, nscal - 1] == 0.0)
        c.close()
    cs = vh.case("VL2")
    assert cs.Z[3, cs.dt_off] == 0.0
    for order in (4, 10):
        zero = vh.zero_segments("VL2", order)
        names = [vh.segment_names("VL2")(s) for s in zero]
        assert any(nm.endswith("#3") for nm in names), names
        c = make_ctx(cs, order)
        got = hess_dev(c, dev(cs.Z), dev(vh.rand_mu("VL2")))
        codes = vh.codes("VL2")
        for s in zero:
            assert np.all(got[codes == s] == 0.0), vh.segment_names("VL2")(s)
        c.close()


# ---- splits -----------------------------------------------------------------------------------------------------------------------------------------
def test_every_split_gives_the_same_bits():
    """cols_per_slice and large_var_hess_drives, alone and together, against auto."""
    for name, order, settings in (
        ("VL2", 6, [dict(cols_per_slice=1), dict(cols_per_slice=2), dict(cols_per_slice=5), dict(cols_per_slice=33), dict(large_var_hess_drives=1),
                    dict(large_var_hess_drives=2), dict(cols_per_slice=5, large_var_hess_drives=2), dict(cols_per_slice=2, large_var_hess_drives=1)]),
        ("VL5", 4, [dict(large_var_hess_drives=1), dict(large_var_hess_drives=5)]),
        ("VH1", 10, [dict(large_var_hess_drives=1), dict(large_var_hess_drives=5)]),
    ):  # fmt: skip
        cs = vh.case(name)
        c = make_ctx(cs, order)
        Zd, mud = dev(cs.Z), dev(vh.rand_mu(name))
        auto = hess_dev(c, Zd, mud)
        vh.check(name, order, auto, TOL)
        for opts in settings:
            for key, val in opts.items():
                c.set_option(key, val)
            assert np.array_equal(auto, hess_dev(c, Zd, mud)), (name, opts)
            for key in opts:
                c.set_option(key, 0)
        assert np.array_equal(auto, hess_dev(c, Zd, mud)), (name, "back to auto")
        c.close()


# ---- zero multipliers on the variations -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,order", [("VL2", 8), ("VL3", 10), ("VL3", 4)])
def test_zero_multipliers_on_the_variations_give_the_plain_bits(name, order):
    """Scalars and X_0 vectors bitwise a plain large context's with large_hess on (G0, Gj); X_b vectors exact zeros."""
    cs = vh.case(name)
    mu = vh.mu_without_variations(name)
    c = make_ctx(cs, order)
    Zd = dev(cs.Z)
    got = hess_dev(c, Zd, dev(mu))
    c.close()
    p = plain_ctx(cs, order)
    mu0 = mu.reshape(cs.K, 1 + cs.v, cs.xdc)[:, 0]
    want = hess_dev(p, Zd, dev(mu0))
    assert p.get_option("last_hess_kernel") == 290 + order // 2
    p.close()
    i0, ib, ip = vh.component_slices(cs)
    assert not np.isnan(got).any() and not np.isnan(want).any()
    assert np.array_equal(got[i0], want[ip]), "scalars and X_0 vectors"
    assert np.all(got[ib] == 0.0), "X_b vectors"


# ---- structure --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [0, 1])
def test_structure(base):
    cs = vh.case("VL2")
    c = make_ctx(cs, 4, index_base=base)
    er, ec = vh.lib_structure(cs, base)
    for dtype in (np.int32, np.int64):
        r, cc = c.hess_structure(dtype)
        assert r.dtype == dtype and np.array_equal(r, er) and np.array_equal(cc, ec)
    c.close()


def test_structure_is_the_small_context_rule():
    """The same descriptor at n <= 64 (W3 of the variational sweep: ket, v = 2): the library's structure there equals the restated rule."""
    import variational_shape_cases as vsc

    cs, _ = vsc.case("W3")
    c = pa.integrators._PclContext(**vl.context_args(cs, 4, batch_mode=L.PCL_BATCH_VARIATIONAL, large_generator=True, large_variational=True,
                                                     large_var_hessian=True))  # fmt: skip
    assert not c.large_variational and not c.large_var_hessian and c.get_option("large_var_hess") == 0  # (n <= 64: the keyword sets nothing)
    r, cc = c.hess_structure()
    er, ec = vh.lib_structure(cs)
    assert np.array_equal(r, er) and np.array_equal(cc, ec)
    c.close()


# ---- the option -------------------------------------------------------------------------------------------------------------------------------------
def test_the_option():
    cs = vh.case("VL1")
    c = make_ctx(cs, 8, hess=False)
    assert c.get_option("large_var_hess") == 0 and c.hess_nnz == 0 and not c.large_var_hessian
    Zd, mud = dev(cs.Z), dev(vh.rand_mu("VL1"))
    buf = nans(16)
    E = L.PCL_ENOTIMPL
    dd, vd = nans(c.n_rows), nans(c.jac_nnz)
    c.eval_jac_dev(Zd, dd, vd)
    c.sync()
    before = (dd.cpu().numpy(), vd.cpu().numpy())
    a, b = ctypes.c_int64(), ctypes.c_int64()

    def five_refusals():
        assert c._L.pcl_hess_nnz(c._h, ctypes.byref(a), ctypes.byref(b)) == E
        msg = c._L.pcl_last_error(c._h).decode()
        assert msg == "pcl_hess_nnz is not implemented for a large variational context (PCL_BATCH_VARIATIONAL | PCL_LARGE_N | PCL_LARGE_VAR, generator dimension 66 > 64): residual and Jacobian only", msg
        i32, i64 = np.zeros(4, np.int32), np.zeros(4, np.int64)
        p32, p64 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
        assert c._L.pcl_hess_structure(c._h, i32.ctypes.data_as(p32), i32.ctypes.data_as(p32)) == E
        assert c._L.pcl_last_error(c._h).decode().startswith("pcl_hess_structure is not implemented for a large variational context") and REFUSAL in c._L.pcl_last_error(c._h).decode()
        assert c._L.pcl_hess_structure_i64(c._h, i64.ctypes.data_as(p64), i64.ctypes.data_as(p64)) == E
        assert c._L.pcl_last_error(c._h).decode().startswith("pcl_hess_structure is not implemented for a large variational context")
        with pytest.raises(pa.PclError) as ei:
            c.hess(cs.Z.reshape(-1), np.ones(c.n_rows), np.zeros(16))
        assert ei.value.code == E and str(ei.value).count("pcl_hess is not implemented for a large variational context") and REFUSAL in str(ei.value)
        with pytest.raises(pa.PclError) as ei:
            c.hess_dev(Zd, mud, buf)
        assert ei.value.code == E and str(ei.value).count("pcl_hess_dev is not implemented for a large variational context") and REFUSAL in str(ei.value)

    def rest_refused():
        W = "PCL_LARGE_VAR"
        assert c._L.pcl_jac_compact_nnz(c._h, ctypes.byref(a), ctypes.byref(b)) == E and REFUSAL in c._L.pcl_last_error(c._h).decode()
        assert c._L.pcl_merit_grad_len(c._h, ctypes.byref(a), ctypes.byref(b)) == E and REFUSAL in c._L.pcl_last_error(c._h).decode()
        refused(E, W, c.rollout, cs.Z.reshape(-1))
        refused(E, W, c.set_member_window, 0, 1)
        refused(E, W, c.set_goal, np.zeros(cs.xdc))
        rc = c._L.pcl_infidelity_dev(c._h, ctypes.c_void_p(Zd.data_ptr()), ctypes.c_double(1.0), ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(buf.data_ptr()))
        assert rc == E and W in c._L.pcl_last_error(c._h).decode()
        for f, args in (("pcl_eval_jac_compact_dev", (Zd, buf, buf)), ("pcl_merit_grad_dev", (Zd, buf, buf, buf)), ("pcl_eval_jac_merit_dev", (Zd, buf, buf, buf, buf))):
            rc = getattr(c._L, f)(c._h, *[ctypes.c_void_p(t.data_ptr()) for t in args])
            assert rc == E and W in c._L.pcl_last_error(c._h).decode(), f

    five_refusals()
    rest_refused()
    for bad in (2, -1):
        refused(L.PCL_EINVAL, "large_var_hess must be 0 or 1", c.set_option, "large_var_hess", bad)
    refused(L.PCL_EINVAL, "large_var_hess_drives", c.set_option, "large_var_hess_drives", -1)
    refused(L.PCL_EINVAL, "large_hess", c.set_option, "large_hess", 1)
    c.set_option("large_var_hess", 1)
    assert c.get_option("large_var_hess") == 1 and c.large_var_hessian and c.hess_nnz == cs.K * vh.values_per_interval(cs)
    got = hess_dev(c, Zd, mud)
    vh.check("VL1", 8, got, TOL, "option switched on")
    assert np.array_equal(got, c.hess(cs.Z.reshape(-1), vh.rand_mu("VL1")))
    r, cc = c.hess_structure()
    er, ec = vh.lib_structure(cs)
    assert np.array_equal(r, er) and np.array_equal(cc, ec)
    r32, _ = c.hess_structure(np.int32)
    assert np.array_equal(r32, er)
    rest_refused()
    c.set_option("large_var_hess", 0)
    assert c.get_option("large_var_hess") == 0 and c.hess_nnz == 0
    five_refusals()
    c.eval_jac_dev(Zd, dd, vd)
    c.sync()
    assert np.array_equal(before[0], dd.cpu().numpy()) and np.array_equal(before[1], vd.cpu().numpy()), "residual + Jacobian before and after"
    c.set_option("large_var_hess", 1)
    assert np.array_equal(got, hess_dev(c, Zd, mud))
    c.close()


def test_the_option_on_other_kinds():
    """PCL_EINVAL with the `needs` sentence on a plain large, a small variational and a large exponential context."""
    import variational_shape_cases as vsc

    needs = "large_var_hess = 1 needs a large variational context (PCL_BATCH_VARIATIONAL | PCL_LARGE_N | PCL_LARGE_VAR at a generator dimension above 64)"
    cs = vh.case("VL1")
    ctxs = [pa.integrators._PclContext(d=cs.n // 2, m=cs.m, N=cs.N, z_dim=cs.z_dim, u_off=cs.u_off, dt_off=cs.dt_off, x_offs=[cs.xo[0]], G0=cs.G0, Gj=cs.Gj,
                                       batch=1, batch_mode=L.PCL_BATCH_MEMBERS, pade_order=o, state_cols=cs.C, large_generator=True, large_exp=e)
            for o, e in ((8, False), ("exp", True))]  # fmt: skip
    w3, _ = vsc.case("W3")
    ctxs.append(pa.integrators._PclContext(**vl.context_args(w3, 4, batch_mode=L.PCL_BATCH_VARIATIONAL)))
    for c in ctxs:
        refused(L.PCL_EINVAL, needs, c.set_option, "large_var_hess", 1)
        assert c.get_option("large_var_hess") == 0
        refused(L.PCL_EINVAL, "large_var_hess_drives", c.set_option, "large_var_hess_drives", 1)
        c.set_option("large_var_hess", 0)
        c.close()


def test_order_zero_without_a_decision():
    cs = vh.case("VL1")
    c = make_ctx(cs, 0)
    refused(L.PCL_EINVAL, "pcl_hess: the context was created with pade_order = 0; call pcl_set_order_policy (or a host-pointer entry point) first",
            c.hess_dev, dev(cs.Z), dev(vh.rand_mu("VL1")), nans(c.hess_nnz))  # fmt: skip
    c.close()


# ---- the public constructor ---------------------------------------------------------------------------------------------------------------------------
def test_public_constructor_end_to_end():
    """VariationalKetIntegrator(..., large_generator=True, large_var_hessian=True) on VL1's system: eval_hessian_of_lagrangian against the
    oracle's scattered values, and H v against the central difference of J(z +- eps v)^T mu through pa.eval_jacobian at eps = 1e-5, held to
    10 x what the float64 oracle shows against its own quotient (vh.FD_ORACLE; tests/test_var_large_hess_cpu.py measures it)."""
    cs = vh.case("VL1")
    order = vh.FD_ORDER
    H0, Hd, Hv = vl.hamiltonians("VL1")
    sysv = pa.VariationalQuantumSystem(H0, list(Hd), list(Hv), [1.0] * cs.m)
    comps = {"ψ̃": cs.Z[:, cs.xo[0] : cs.xo[0] + cs.xdc].T, "ψ̃_var": cs.Z[:, cs.xo[1] : cs.xo[1] + cs.xdc].T, "Δt": cs.Z[:, cs.dt_off][None],
             "t": cs.Z[:, cs.dt_off + 1][None], "u": cs.Z[:, cs.u_off : cs.u_off + cs.m].T}  # fmt: skip
    traj = pa.NamedTrajectory(comps, controls=("u", "Δt"), timestep="Δt")
    assert np.array_equal(traj.datavec, cs.Z.reshape(-1))
    B0 = pa.VariationalKetIntegrator(sysv, traj, "ψ̃", ["ψ̃_var"], "u", scale=vl.SCALES[0], pade_order=order, large_generator=True)
    with pytest.raises(pa.PclError, match="PCL_LARGE_VAR"):
        pa.hessian_structure(B0)
    B0.close()
    B = pa.VariationalKetIntegrator(sysv, traj, "ψ̃", ["ψ̃_var"], "u", scale=vl.SCALES[0], pade_order=order, large_generator=True, large_var_hessian=True)
    assert B.ctx.large_variational and B.ctx.large_var_hessian
    mu, v = vh.fd_inputs(cs)
    H = pa.eval_hessian_of_lagrangian(B, traj, mu)
    want, _ = vt.hessian(cs, order, mu)
    want = want + __import__("scipy.sparse").sparse.tril(want, -1).T
    r, c_ = pa.hessian_structure(B)
    er, ec = vh.lib_structure(cs)
    assert np.array_equal(r, er) and np.array_equal(c_, ec)
    scale = np.abs(want.data).max()
    err = np.abs((H - want).data).max() / scale if (H - want).nnz else 0.0
    print("eval_hessian_of_lagrangian against the oracle's scattered values: %.1e of the largest value" % err)
    assert err <= TOL
    z = traj.datavec.copy()

    def jt_mu(zz):
        traj.update(zz)
        return pa.eval_jacobian(B, traj).T @ mu

    fd = vh.fd_error(H @ v, jt_mu, z, v)
    traj.update(z)
    print("H v against the central difference through pa.eval_jacobian: %.2e of max |H v| (the oracle: %.2e)" % (fd, vh.FD_ORACLE))
    assert fd <= 10 * vh.FD_ORACLE
    B.close()
