"""GPU tests of the option var_compact: the compact Jacobian of a variational context, either constraint kind (layouts, cases, truth and
comparison: tests/var_compact_cases.py).  N = 4 or 5 everywhere.

    mode         cases                                                        what they exercise
    Pade         Pauli d = 2, ket and unitary; config 2 (n = 8, m = 4), v = 1, 2  small shapes, both state kinds
    Pade         d = 16 and d = 17 (n = 32 / 34)                                one pass / two passes of the 512-thread pair loop (PCL_VAR_PPT)
    Pade         d = 32 (n = 64)                                                all four passes
    Pade         config 3 (n = 54, C = 27, m = 6), v = 1, 2, unitary and ket       the benchmark shape; a tail that crosses several expansion chunks
    Pade         each at order 4; config 2 and config 3 also at order 10        the fold differs by order, the store does not
    exponential  Pauli; config 2; d = 16 / 17                                  the 256 -> 512-thread switch at n > 32
    exponential  config 3, v = 1, 2, unitary and ket
    exponential  one transmon of 31 levels (n = 62)                             no LDS tile for G(u_k)

Column counts 4 and 17 are no multiples of the expansion's slice of 3 columns, 27 is one; kets have one column, where the compact layout still is
not the full one.  Every output buffer starts as NaN.  Every test here needs the option, which the parent commit does not know."""
import ctypes

import numpy as np
import pytest
import torch

import piccolo_jl_amd as pa
import var_compact_cases as vc

pytestmark = pytest.mark.gpu
EXP, VAR, VEXP = pa._lib.PCL_ORDER_EXP, pa._lib.PCL_BATCH_VARIATIONAL, pa._lib.PCL_BATCH_VARIATIONAL_EXP
E_INVAL, E_NOTIMPL = pa._lib.PCL_EINVAL, pa._lib.PCL_ENOTIMPL
IDS = [vc.case_id(p) for p in vc.ALL_CASES]


def make_ctx(case, order, **kw):
    expo = order == "exp"
    return pa.integrators._PclContext(d=case.n // 2, m=case.m, N=case.N, z_dim=case.z_dim, u_off=case.u_off, dt_off=case.dt_off, x_offs=case.xo,
                                      G0=np.concatenate([case.G0[None], np.array(case.Gv)]), Gj=case.Gj, batch=1 + case.v,
                                      batch_mode=VEXP if expo else VAR, per_member_G0=True, pade_order=EXP if expo else order, state_cols=case.C, **kw)  # fmt: skip


def kernels(order):
    """last_kernel after the full and after the compact launch"""
    return (110, 112) if order == "exp" else (70, 72)


def nan_dev(n):
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


def host(t):
    return t.cpu().numpy()


# ---- 1-3: the device launches ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, order", vc.ALL_CASES, ids=IDS)
def test_compact_launch_and_expansion(name, order):
    case = vc.built(name)[3]
    kw = vc.of_case(case, order == "exp")
    K = case.K
    c = make_ctx(case, order, var_compact=True)
    k_full, k_comp = kernels(order)
    assert c.get_option("var_compact") == 1 and c.var_compact
    assert c.compact_per == vc.compact_per(**kw) and c.compact_nnz == K * c.compact_per
    assert c.jac_per == vc.full_per(**kw) and c.jac_nnz == K * c.jac_per
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    Zd = torch.from_numpy(case.Z.reshape(-1).copy()).cuda()
    # 1. the full launch, then the compact launch
    d_full, v_full = nan_dev(c.n_rows), nan_dev(c.jac_nnz)
    c.eval_jac_dev(Zd, d_full, v_full)
    assert c.get_option("last_kernel") == k_full
    d_comp, v_comp = nan_dev(c.n_rows), nan_dev(c.compact_nnz)
    c.eval_jac_compact_dev(Zd, d_comp, v_comp)
    assert c.get_option("last_kernel") == k_comp
    v_exp = nan_dev(c.jac_nnz)
    c.jac_expand_dev(v_comp, v_exp)
    c.sync()
    full, comp, expd = host(v_full).reshape(K, -1), host(v_comp).reshape(K, -1), host(v_exp).reshape(K, -1)
    for what, a in (("delta", host(d_full)), ("compact delta", host(d_comp)), ("full values", full), ("compact values", comp), ("expanded values", expd)):
        assert not np.isnan(a).any(), what
    assert vc.same_bits(host(d_comp), host(d_full))
    assert vc.same_bits(comp, vc.compact_of_full(full, **kw))  # (raises if the full launch's own copies differ)
    assert vc.same_bits(expd, full)
    # 2. the truth: bit-equality with a wrong full launch does not pass
    ok, err = vc.matches(expd, name, order)
    print("%s: worst |expanded - truth| = %.2e (tolerance %.2e)" % (vc.case_id((name, order)), err, vc.TOL * vc.truth(name, order)[1]))
    assert ok, err
    # 3. the expansion's slices, and a second compact launch
    for cps in (1, 2, 0):
        c.set_option("cols_per_slice", cps)
        again = nan_dev(c.jac_nnz)
        c.jac_expand_dev(v_comp, again)
        c.sync()
        assert vc.same_bits(host(again).reshape(K, -1), full), cps
    d2, v2 = nan_dev(c.n_rows), nan_dev(c.compact_nnz)
    c.eval_jac_compact_dev(Zd, d2, v2)
    c.sync()
    assert c.get_option("last_kernel") == k_comp
    assert vc.same_bits(host(v2).reshape(K, -1), comp) and vc.same_bits(host(d2), host(d_full))
    # the Jacobian alone (no residual is written), and the block split that a compact launch has no use for
    c.set_option("var_block_wgs", 3)
    v3 = nan_dev(c.compact_nnz)
    c.eval_jac_compact_dev(Zd, None, v3)
    c.sync()
    assert vc.same_bits(host(v3).reshape(K, -1), comp)
    c.set_stream(None)
    c.close()


# ---- 4: the host-pointer path -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, order", vc.ALL_CASES, ids=IDS)
def test_host_pointer_path(name, order):
    case = vc.built(name)[3]
    c = make_ctx(case, order, var_compact=True)
    k_full, k_comp = kernels(order)
    Z = case.Z.reshape(-1).copy()
    c.set_option("host_threads", 4)
    c.set_option("host_path", 1)
    d1, v1 = c.eval_jac(Z, np.full(c.n_rows, np.nan), np.full(c.jac_nnz, np.nan))
    assert c.get_option("last_kernel") == k_full and c.get_option("host_store_bytes") == 0
    c.set_option("host_path", 0)
    d0, v0 = c.eval_jac(Z, np.full(c.n_rows, np.nan), np.full(c.jac_nnz, np.nan))
    took_compact = c.get_option("last_kernel") == k_comp
    assert took_compact == (case.C > 1)  # one state column: the route stays full
    assert took_compact or c.get_option("last_kernel") == k_full
    assert (c.get_option("host_store_bytes") > 0) == took_compact
    assert not np.isnan(d0).any() and not np.isnan(v0).any() and not np.isnan(d1).any() and not np.isnan(v1).any()
    assert vc.same_bits(d0, d1) and vc.same_bits(v0, v1)
    assert vc.same_bits(c.jac(Z, np.full(c.jac_nnz, np.nan)), v1) and vc.same_bits(c.eval(Z, np.full(c.n_rows, np.nan)), d1)
    ok, err = vc.matches(v0, name, order)
    assert ok, err
    # the option back to 0: the parent's call
    c.set_option("var_compact", 0)
    assert c.compact_nnz == 0 and c.compact_per == 0
    dp, vp = c.eval_jac(Z, np.full(c.n_rows, np.nan), np.full(c.jac_nnz, np.nan))
    assert c.get_option("last_kernel") == k_full
    assert vc.same_bits(dp, d1) and vc.same_bits(vp, v1)
    c.close()


# ---- 5: the option ------------------------------------------------------------------------------------------------------------------------------
def _trio(c, Zd, delta, comp, vals):
    """(code, message) of pcl_jac_compact_nnz, pcl_eval_jac_compact_dev, pcl_jac_expand_dev"""
    L, h, vp = c._L, c._h, ctypes.c_void_p
    i64 = ctypes.c_int64()
    out = []
    for call in (lambda: L.pcl_jac_compact_nnz(h, ctypes.byref(i64), ctypes.byref(i64)),
                 lambda: L.pcl_eval_jac_compact_dev(h, vp(Zd.data_ptr()), vp(delta.data_ptr()), vp(comp.data_ptr())),
                 lambda: L.pcl_jac_expand_dev(h, vp(comp.data_ptr()), vp(vals.data_ptr()))):  # fmt: skip
        rc = call()
        out.append((rc, (L.pcl_last_error(h) or b"").decode()))
    return out


@pytest.mark.parametrize("order", [4, "exp"])
def test_option_off_refuses_in_todays_words_and_on_serves(order):
    case = vc.built("config2_v1")[3]
    c = make_ctx(case, order)
    mode = "PCL_BATCH_VARIATIONAL_EXP" if order == "exp" else "PCL_BATCH_VARIATIONAL"
    Zd = torch.from_numpy(case.Z.reshape(-1).copy()).cuda()
    delta, comp, vals = nan_dev(c.n_rows), nan_dev(c.jac_nnz), nan_dev(c.jac_nnz)  # (the compact values are fewer than the full ones)
    words = ["pcl_jac_compact_nnz is not implemented for a variational context (%s)" % mode,
             "the compact Jacobian is not implemented for a variational context (%s)" % mode,
             "pcl_jac_expand_dev is not implemented for a variational context (%s)" % mode]  # fmt: skip
    assert c.get_option("var_compact") == 0 and c.compact_nnz == 0 and not c.var_compact
    for on in (1, 0):  # set back to 0: the refusals return
        assert [(E_NOTIMPL, w) for w in words] == _trio(c, Zd, delta, comp, vals)
        c.set_option("var_compact", 1)
        assert c.get_option("var_compact") == 1 and c.compact_per == vc.compact_per(**vc.of_case(case, order == "exp"))
        assert [rc for rc, _ in _trio(c, Zd, delta, comp, vals)] == [0, 0, 0]
        # still refused with the option on
        i64 = ctypes.c_int64()
        assert c._L.pcl_set_member_window(c._h, 0, 1) == E_NOTIMPL and b"variational" in c._L.pcl_last_error(c._h)
        assert c._L.pcl_merit_grad_len(c._h, ctypes.byref(i64), ctypes.byref(i64)) == E_NOTIMPL and b"variational" in c._L.pcl_last_error(c._h)
        c.sync()
        c.set_option("var_compact", 0)
        assert c.get_option("var_compact") == 0 and c.compact_nnz == 0
    for bad in (2, -1):
        with pytest.raises(pa.PclError) as ei:
            c.set_option("var_compact", bad)
        assert ei.value.code == E_INVAL and "var_compact must be 0 or 1" in str(ei.value)
    assert c.get_option("var_compact") == 0
    c.close()


@pytest.mark.parametrize("order", [4, "exp"])
def test_option_on_a_plain_context_is_einval(order):
    """A plain Pade context and a plain PCL_ORDER_EXP one: 1 is PCL_EINVAL, 0 is accepted, get reads 0."""
    s = pa.QuantumSystem(0.5 * pa.PAULIS["Z"], [pa.PAULIS["X"], pa.PAULIS["Y"]], [1.0, 1.0])
    c = pa.integrators._PclContext(d=2, m=2, N=4, z_dim=12, u_off=10, dt_off=8, x_offs=[0], G0=s.G_drift, Gj=s.G_drives_array(), batch=1,
                                   batch_mode=pa._lib.PCL_BATCH_MEMBERS, pade_order=order)  # fmt: skip
    with pytest.raises(pa.PclError) as ei:
        c.set_option("var_compact", 1)
    assert ei.value.code == E_INVAL and "var_compact = 1 needs a variational context" in str(ei.value)
    with pytest.raises(pa.PclError) as ei:
        c.set_option("var_compact", 2)
    assert ei.value.code == E_INVAL
    c.set_option("var_compact", 0)
    assert c.get_option("var_compact") == 0
    c.close()


def test_all_options_together_keep_the_other_results():
    """var_full, var_exp_hess (config 2: n = 8 <= 44) and var_compact on one context: the objective, its Hessian, the Hessian of the Lagrangian
    and the rollout have the bits they have without var_compact, and the compact trio is served beside them."""
    from oracle import pade_oracle as po

    case = vc.built("config2_v2")[3]
    kw = vc.of_case(case, True)
    Z = case.Z.reshape(-1).copy()
    rng = np.random.default_rng(9)
    goal = po.operator_to_iso_vec(np.linalg.qr(rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4)))[0])
    mu = rng.standard_normal(case.K * case.xd)
    got = []
    for on in (0, 1):
        c = make_ctx(case, "exp", exp_hessian=True)
        c.set_option("var_full", 1)
        c.set_option("var_compact", on)
        assert (c.get_option("var_full"), c.get_option("var_exp_hess"), c.get_option("var_compact")) == (1, 1, on)
        c.set_goal(goal)
        c.set_weights([1.0, 0.3, 0.2])
        c.add_regularizer(case.u_off, case.m, 0.1, 2)
        val, grad = c.objective(Z, 100.0)
        res = [np.asarray(val), grad, c.objective_hess(Z, 100.0, 0.7), c.hess(Z, mu), c.rollout(Z)]
        c.set_option("host_path", 1)
        res += list(c.eval_jac(Z))
        if on:
            c.set_option("host_path", 0)
            d0, v0 = c.eval_jac(Z)
            assert c.get_option("last_kernel") == 112
            assert vc.same_bits(d0, res[-2]) and vc.same_bits(v0, res[-1])
            vc.compact_of_full(v0.reshape(case.K, -1), **kw)
            # var_full and var_exp_hess off again: var_compact stays
            c.set_option("var_exp_hess", 0)
            c.set_option("var_full", 0)
            assert c.get_option("var_compact") == 1 and c.compact_per == vc.compact_per(**kw)
        got.append(res)
        c.close()
    for a, b in zip(*got):
        assert vc.same_bits(a, b)


def test_constructor_keyword_end_to_end():
    """VariationalUnitaryIntegrator / VariationalKetIntegrator(var_compact=True), a Pade order and "exp": the option is on, the sizes are set, and
    the host-pointer call takes the compact route where the blocks are replicated."""
    s, Hv, scales, case, _ = vc.built("config2_v1")
    for ket, order in ((False, 4), (False, "exp"), (True, 10)):
        cs = vc.built("pauli_ket")[3] if ket else case
        so, hv, sc = (vc.built("pauli_ket")[:3]) if ket else (s, Hv, scales)
        names = ["x"] + ["x_var%d" % (i + 1) for i in range(cs.v)]
        comps = {nm: cs.Z[:, o : o + cs.xdc].T for nm, o in zip(names, cs.xo)}
        comps["Δt"] = cs.Z[:, cs.dt_off][None]
        comps["t"] = cs.Z[:, cs.dt_off + 1][None]
        comps["u"] = cs.Z[:, cs.u_off : cs.u_off + cs.m].T
        traj = pa.NamedTrajectory(comps, controls=("u", "Δt"), timestep="Δt")
        vs = pa.VariationalQuantumSystem(so.H_drift, list(so.H_drives), hv, [1.0] * so.n_drives)
        if ket:
            B = pa.VariationalKetIntegrator(vs, traj, names[0], names[1:], "u", scale=float(sc[0]), pade_order=order, var_compact=True)
        else:
            B = pa.VariationalUnitaryIntegrator(vs, traj, names[0], names[1:], "u", scales=sc, pade_order=order, var_compact=True)
        kw = vc.of_case(cs, order == "exp")
        assert B.ctx.get_option("var_compact") == 1 and B.ctx.compact_per == vc.compact_per(**kw)
        B.ctx.set_option("host_threads", 4)
        J = pa.eval_jacobian(B, traj)
        assert B.ctx.get_option("last_kernel") == (kernels(order)[1] if cs.C > 1 else kernels(order)[0])
        B.ctx.set_option("var_compact", 0)
        J0 = pa.eval_jacobian(B, traj)
        assert (J != J0).nnz == 0
        B.close()
