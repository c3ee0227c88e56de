"""The option exp_full of the exponential constraint (pcl_desc.pade_order = PCL_ORDER_EXP) on the device, through the C ABI: the compact
Jacobian trio, the host-pointer calls' compact path and the merit / reduce payload by its three routes.  Cases, truth and tolerance:
tests/exp_full_cases.py (1e-11 per entry on |w lam_k|_2 |column|_2, the np.longdouble payload of exp_truth's Jacobian values)."""
import ctypes

import numpy as np
import pytest

import exp_full_cases as xc
import piccolo_jl_amd as pa
from exp_full_cases import TOL

pytestmark = pytest.mark.gpu
EXP = pa._lib.PCL_ORDER_EXP
NAMES = sorted(xc.CASES)


def make_ctx(name, exp_full=True, **kw):
    args = xc.ctx_args(name)
    args.update(pade_order=EXP, exp_full=exp_full)
    args.update(kw)
    c = pa.integrators._PclContext(**args)
    if name in xc.WEIGHTS:
        c.set_weights(xc.case(name).weights)
    return c


def nan(n):
    import torch

    t = torch.full((int(n),), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()  # (the contexts launch on streams of their own: the fill must have landed)
    return t


def dev(a):
    import torch

    t = torch.from_numpy(np.array(a, dtype=np.float64).reshape(-1)).cuda()  # (a copy: the cases are read-only)
    torch.cuda.synchronize()
    return t


def full_launch(c, Zd):
    d, v = nan(c.n_rows), nan(c.jac_nnz)
    c.eval_jac_dev(Zd, d, v)
    c.sync()
    assert c.get_option("last_kernel") == 100
    return d.cpu().numpy(), v.cpu().numpy()


# ---- the compact trio ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_compact_expands_to_the_full_values_bitwise(name):
    cs = xc.case(name)
    c = make_ctx(name)
    n, C, m, K = cs.n, cs.cols, cs.m, cs.lay.K
    assert c.exp_full and c.get_option("exp_full") == 1
    assert c.compact_per == xc.compact_per(n, C, m) and c.compact_nnz == c.compact_per * cs.batch * K
    Zd = dev(cs.Zfull)
    windows = [(0, cs.batch)] + ([xc.WINDOW[name]] if name in xc.WINDOW else [])
    whole = None
    for first, count in windows:
        c.set_member_window(first, count)
        assert c.compact_nnz == c.compact_per * count * K and c.jac_nnz == xc.full_per(n, C, m) * count * K
        delta, vals = full_launch(c, Zd)
        dc, comp = nan(c.n_rows), nan(c.compact_nnz)
        c.eval_jac_compact_dev(Zd, dc, comp)
        c.sync()
        assert c.get_option("last_kernel") == 102
        assert np.array_equal(dc.cpu().numpy(), delta)  # the residual of the compact launch: the full launch's bits
        assert np.array_equal(comp.cpu().numpy(), xc.compact_of_full(vals, n, C, m).reshape(-1))
        ve = nan(c.jac_nnz)
        c.jac_expand_dev(comp, ve)
        c.sync()
        assert np.array_equal(ve.cpu().numpy(), vals)
        assert np.array_equal(vals, xc.expand_compact(comp.cpu().numpy(), n, C, m).reshape(-1))
        if whole is None:
            whole = (delta, vals)
            ds, vs = xc.truth(name)
            assert np.abs(delta - ds.reshape(-1)).max() <= TOL * max(1.0, np.abs(ds).max())
            assert np.abs(vals - vs.reshape(-1)).max() <= TOL * max(1.0, np.abs(vs).max())
        else:  # the window's values are the slices of the whole launch
            pd, pv = K * n * C, K * xc.full_per(n, C, m)
            assert np.array_equal(delta, whole[0][first * pd : (first + count) * pd]) and np.array_equal(vals, whole[1][first * pv : (first + count) * pv])
    c.close()


@pytest.mark.parametrize("name", NAMES)
def test_host_pointer_paths_agree_bitwise(name):
    """pcl_eval_jac with host_path 0 (compact values over PCIe, expanded by the host's threads, when cols > 1) and host_path 1 (full values)."""
    cs = xc.case(name)
    c = make_ctx(name)
    Zh = np.ascontiguousarray(cs.Zfull).reshape(-1)
    c.set_option("host_threads", 4)
    c.set_option("host_path", 1)
    d1, v1 = c.eval_jac(Zh)
    assert c.get_option("last_kernel") == 100 and c.get_option("host_store_bytes") == 0
    c.set_option("host_path", 0)
    d0, v0 = c.eval_jac(Zh, np.full(c.n_rows, np.nan), np.full(c.jac_nnz, np.nan))
    took_compact = c.get_option("last_kernel") == 102
    assert took_compact == (cs.cols > 1)  # one state column: the path stays full
    assert (c.get_option("host_store_bytes") > 0) == took_compact
    assert np.array_equal(d0, d1) and np.array_equal(v0, v1)
    assert np.array_equal(c.jac(Zh), v1) and np.array_equal(c.eval(Zh), d1)
    if name in xc.WINDOW:
        first, count = xc.WINDOW[name]
        c.set_member_window(first, count)
        dw, vw = c.eval_jac(Zh)
        pd, pv = cs.lay.K * cs.n * cs.cols, cs.lay.K * xc.full_per(cs.n, cs.cols, cs.m)
        assert np.array_equal(dw, d1[first * pd : (first + count) * pd]) and np.array_equal(vw, v1[first * pv : (first + count) * pv])
    # with the option off the call is the parent's: full values
    c.set_member_window(0, cs.batch)
    c.set_option("exp_full", 0)
    d2, v2 = c.eval_jac(Zh)
    assert c.get_option("last_kernel") == 100 and np.array_equal(d2, d1) and np.array_equal(v2, v1)
    c.close()


# ---- the payload -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_lam", [True, False], ids=["lam", "merit"])
@pytest.mark.parametrize("name", NAMES)
def test_payload_three_routes_against_the_truth(name, with_lam):
    cs = xc.case(name)
    c = make_ctx(name)
    K, m = cs.lay.K, cs.m
    length, sets = c.merit_grad_len()
    assert (length, sets) == (1 + K * m + K, cs.sets)
    want, scale = xc.payload_truth(name, with_lam)
    Zd = dev(cs.Zfull)
    lam = dev(cs.lam) if with_lam else None
    delta, vals = full_launch(c, Zd)

    def check(label, out):
        w = xc.worst(out.cpu().numpy(), want, scale)
        print("%s %s: worst |payload - truth| / (|w lam| |column|) = %.2e" % (name, label, w))
        assert w <= TOL, (label, w)

    # 1. from the Jacobian values
    dd, vd = dev(delta), dev(vals)
    o1, o1b = nan(length * sets), nan(length * sets)
    c.merit_grad_dev(dd, lam, vd, o1)
    c.merit_grad_dev(dd, lam, vd, o1b)
    c.sync()
    check("from values", o1)
    assert np.array_equal(o1.cpu().numpy(), o1b.cpu().numpy())
    # 2. fused into the Jacobian launch
    outs = []
    for _ in range(2):
        d2, v2, o2 = nan(c.n_rows), nan(c.jac_nnz), nan(length * sets)
        c.eval_jac_merit_dev(Zd, lam, d2, v2, o2)
        c.sync()
        assert c.get_option("last_merit_fused") == 1 and c.get_option("last_kernel") == 100
        assert np.array_equal(d2.cpu().numpy(), delta) and np.array_equal(v2.cpu().numpy(), vals)
        outs.append(o2.cpu().numpy())
    check("fused", o2)
    assert np.array_equal(outs[0], outs[1])
    # 3. the adjoint launch: no Jacobian value
    outs = []
    for _ in range(2):
        d3, o3 = nan(c.n_rows), nan(length * sets)
        c.eval_jac_merit_dev(Zd, lam, d3, None, o3)
        c.sync()
        assert c.get_option("last_merit_fused") == 0 and c.get_option("last_kernel") == 103
        assert np.array_equal(d3.cpu().numpy(), delta)
        outs.append(o3.cpu().numpy())
    check("adjoint", o3)
    assert np.array_equal(outs[0], outs[1])
    if name in xc.WINDOW:  # the merit entry points cover every member, whatever the window says
        c.set_member_window(*xc.WINDOW[name])
        d4, o4 = nan(cs.n_rows), nan(length * sets)
        c.eval_jac_merit_dev(Zd, lam, d4, None, o4)
        c.sync()
        assert np.array_equal(o4.cpu().numpy(), outs[0]) and np.array_equal(d4.cpu().numpy(), delta)
    c.close()


def test_merit_objective_call_runs_the_two_calls():
    import torch

    cs = xc.case("a")
    c = make_ctx("a")
    goal = np.linalg.qr(np.random.default_rng(3).standard_normal((5, 5)) + 1j * np.random.default_rng(4).standard_normal((5, 5)))[0]
    from oracle import pade_oracle as po

    c.set_goal(po.operator_to_iso_vec(goal))
    c.add_regularizer(cs.lay.u_off, cs.m, 1e-2, 2)
    Zd, lam = dev(cs.Zfull), dev(cs.lam)
    length, sets = c.merit_grad_len()
    d1, v1, o1, val1, g1 = nan(c.n_rows), nan(c.jac_nnz), nan(length), nan(1), nan(c.z_len)
    c.eval_jac_merit_objective_dev(Zd, lam, d1, v1, o1, 100.0, val1, g1)
    c.sync()
    assert c.get_option("last_merit_fused") == 1
    d2, v2, o2, val2, g2 = nan(c.n_rows), nan(c.jac_nnz), nan(length), nan(1), nan(c.z_len)
    c.objective_dev(Zd, 100.0, val2, g2)
    c.eval_jac_merit_dev(Zd, lam, d2, v2, o2)
    c.sync()
    for a, b in ((d1, d2), (v1, v2), (o1, o2), (val1, val2), (g1, g2)):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    c.close()


# ---- gating ----------------------------------------------------------------------------------------------------------------------------------
def _gated_calls(c, Zd):
    """The compact trio and the merit / reduce family through the C ABI, every output in a buffer of its own."""
    L, h = c._L, c._h
    a, b = ctypes.c_int64(), ctypes.c_int64()
    nv = c.jac_nnz
    keep = [torch_zeros(c.n_rows), torch_zeros(nv), torch_zeros(nv), torch_zeros(2 + c.K * (c.m + 1)), torch_zeros(1), torch_zeros(c.z_len)]
    d, v, comp, out, val, grad = (t.data_ptr() for t in keep)
    z = Zd.data_ptr()
    return keep, [
        ("pcl_jac_compact_nnz", lambda: L.pcl_jac_compact_nnz(h, ctypes.byref(a), ctypes.byref(b))),
        ("pcl_eval_jac_compact_dev", lambda: L.pcl_eval_jac_compact_dev(h, z, d, comp)),
        ("pcl_jac_expand_dev", lambda: L.pcl_jac_expand_dev(h, comp, v)),
        ("pcl_merit_grad_len", lambda: L.pcl_merit_grad_len(h, ctypes.byref(a), ctypes.byref(b))),
        ("pcl_merit_grad_dev", lambda: L.pcl_merit_grad_dev(h, d, None, v, out)),
        ("pcl_eval_jac_merit_dev", lambda: L.pcl_eval_jac_merit_dev(h, z, None, d, v, out)),
        ("pcl_eval_jac_merit_objective_dev", lambda: L.pcl_eval_jac_merit_objective_dev(h, z, None, d, v, out, 1.0, val, grad)),
    ]


def torch_zeros(n):
    import torch

    t = torch.zeros(int(n), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    return t


def test_gating():
    cs = xc.case("a")
    E, NI = pa._lib.PCL_EINVAL, pa._lib.PCL_ENOTIMPL
    c = make_ctx("a", exp_full=False)
    assert c.get_option("exp_full") == 0 and not c.exp_full and c.compact_nnz == 0
    Zd = dev(cs.Zfull)
    keep, calls = _gated_calls(c, Zd)
    want = c.eval(cs.Zfull)

    def refused():
        for name, call in calls:
            rc = call()
            msg = c._L.pcl_last_error(c._h).decode()
            assert rc == NI and "exponential" in msg and "PCL_ORDER_EXP" in msg, (name, rc, msg)
        with pytest.raises(pa.PclError) as ei:  # the adjoint launch's signature: a NULL vals stays an invalid argument
            c.eval_jac_merit_dev(Zd, None, keep[0], None, keep[3])
        assert ei.value.code == E
        assert np.array_equal(c.eval(cs.Zfull), want)

    refused()
    c.set_option("exp_full", 1)
    assert c.get_option("exp_full") == 1 and c.compact_per == xc.compact_per(cs.n, cs.cols, cs.m)
    c.set_goal(np.eye(2 * 5, 5).T.reshape(-1))
    for name, call in calls:
        assert call() == 0, (name, c._L.pcl_last_error(c._h).decode())
    c.sync()
    c.set_option("exp_hess", 1)  # independent of exp_hess, both ways
    assert c.get_option("exp_full") == 1
    c.set_option("exp_hess", 0)
    c.set_option("exp_full", 0)
    assert c.get_option("exp_full") == 0 and c.compact_nnz == 0
    refused()
    with pytest.raises(pa.PclError) as ei:
        c.set_option("exp_full", 2)
    assert ei.value.code == E
    c.close()
    # any other context: PCL_EINVAL to set, 0 to read; a NULL vals is PCL_EINVAL
    args = xc.ctx_args("a")
    p4 = pa.integrators._PclContext(pade_order=4, **args)
    assert p4.get_option("exp_full") == 0
    with pytest.raises(pa.PclError) as ei:
        p4.set_option("exp_full", 1)
    assert ei.value.code == E and p4.get_option("exp_full") == 0
    p4.set_option("exp_full", 0)
    length, _ = p4.merit_grad_len()
    with pytest.raises(pa.PclError) as ei:
        p4.eval_jac_merit_dev(Zd, None, nan(p4.n_rows), None, nan(length))
    assert ei.value.code == E
    p4.close()
    from exp_shape_cases import var_case

    vc = var_case("V1")
    for mode, order in ((pa._lib.PCL_BATCH_VARIATIONAL_EXP, EXP), (pa._lib.PCL_BATCH_VARIATIONAL, 4)):
        v = pa.integrators._PclContext(d=vc.n // 2, m=vc.m, N=vc.N, z_dim=vc.z_dim, u_off=vc.u_off, dt_off=vc.dt_off, x_offs=vc.xo, G0=np.array([vc.G0] + list(vc.Gv)),
                                       Gj=vc.Gj, batch=1 + vc.v, batch_mode=mode, per_member_G0=True, pade_order=order, state_cols=vc.C)
        assert v.get_option("exp_full") == 0
        with pytest.raises(pa.PclError) as ei:
            v.set_option("exp_full", 1)
        assert ei.value.code == E and v.get_option("exp_full") == 0
        v.close()


def test_integrator_keyword():
    """HipPadeIntegrator(..., pade_order="exp", exp_full=True): the context serves the compact sizes and the host-pointer calls agree with a plain one."""
    from helpers import traj_from_Z

    cs = xc.case("a")
    traj = traj_from_Z(pa, cs.Zfull, cs.lay)
    B = pa.HipPadeIntegrator(cs.G0s[0], cs.Gj, traj, pade_order="exp", exp_full=True)
    B0 = pa.HipPadeIntegrator(cs.G0s[0], cs.Gj, traj, pade_order="exp")
    assert B.ctx.exp_full and B.ctx.compact_per == xc.compact_per(cs.n, cs.cols, cs.m) and not B0.ctx.exp_full and B0.ctx.compact_per == 0
    d1, v1 = B.ctx.eval_jac(traj.datavec)
    d0, v0 = B0.ctx.eval_jac(traj.datavec)
    assert B.ctx.get_option("last_kernel") == 102 and B0.ctx.get_option("last_kernel") == 100
    assert np.array_equal(d1, d0) and np.array_equal(v1, v0)
    B.close()
    B0.close()
