"""GPU tests of the robust-control objective on a variational context (option var_full): terminal infidelity of the state, the reference's
UnitarySensitivityObjective on the variations at the terminal knot, regularisers on any component -- value, gradient and Hessian against the
closed forms restated in numpy (tests/robust_truth.py), finite differences, the switch, the structure, kets, bitwise equality of the paths, and
the host mirror.  Tolerances: 1e-12 max(1, |ref|) for the value, 1e-12 max|ref| for gradient and Hessian (the plain objective's in
tests/test_parity_gpu.py); 1e-6 max(1, |fd|) for the finite-difference checks (tests/test_plumbing_gpu.py)."""
import numpy as np
import pytest
import scipy.sparse as sp

import piccolo_jl_amd as pa
import robust_truth as rt
from oracle import pade_oracle as po
from variational_truth import h_var_drift, make_case

pytestmark = pytest.mark.gpu
Q = 100.0
ENOTIMPL, EINVAL = pa._lib.PCL_ENOTIMPL, pa._lib.PCL_EINVAL
REFUSAL = "is not implemented for a variational context (PCL_BATCH_VARIATIONAL)"


def _unitary(d, rng):
    return np.linalg.qr(rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d)))[0]


def _case(config, nv, N=5, seed=3, ket=False, **kw):
    """config 2 (two qubits) or 3 (three qutrits): variations along the drift frequencies and along a transmon's drive operator; the terminal
    state set near a unitary so that F is in the interesting range, the terminal variations of order 0.3."""
    s = po.config_system(config)
    lv, ns = (2, 2) if config == 2 else (3, 3)
    Hv = [h_var_drift(lv, ns), po.lift_operator(po.annihilate(lv) + po.annihilate(lv).conj().T, 2, [lv] * ns)][:nv]
    case = make_case(s, [po.G_of_H(h) / 10 for h in Hv], N=N, seed=seed, ket=ket, **kw)
    rng = np.random.default_rng(100 + seed)
    if not ket:
        case.Z[-1, case.xo[0] : case.xo[0] + case.xdc] = po.operator_to_iso_vec(_unitary(s.levels, rng)) + 0.02 * rng.standard_normal(case.xdc)
    for b in range(1, nv + 1):
        case.Z[-1, case.xo[b] : case.xo[b] + case.xdc] = 0.3 * rng.standard_normal(case.xdc)
    return s, case


def _regs(case):
    """all three dt_powers; the second one on a variation component"""
    return [(case.u_off, case.m, np.linspace(0.5, 2.0, case.m), 2), (case.xo[1], case.xdc, 0.1, 1), (case.dt_off + 1, 1, 3.0, 0)]


def _full(case, order=4, index_base=0):
    ctx = rt.var_context(pa, case, order, index_base)
    ctx.set_option("var_full", 1)
    return ctx


def _check_values(ctx, case, w, goal, subspace, regs, sigma=0.8):
    Z = case.Z.reshape(-1)
    val, grad = ctx.objective(Z, Q)
    v_ref, g_ref, H_ref = rt.objective(case, case.Z, w, Q, goal, subspace, regs, want_hess=True)
    e_v, e_g = abs(val[0] - v_ref), np.abs(grad - g_ref.reshape(-1)).max()
    print("value err %.2e (ref %.3e)  gradient err %.2e (max|ref| %.3e)" % (e_v, v_ref, e_g, np.abs(g_ref).max()))
    assert e_v <= 1e-12 * max(1.0, abs(v_ref))
    assert e_g <= 1e-12 * np.abs(g_ref).max()
    rows, cols = ctx.objective_hess_structure()
    hv = ctx.objective_hess(Z, Q, sigma)
    nv = Z.size
    assert np.all(rows >= cols) and len(np.unique(rows * nv + cols)) == len(rows)
    D = (sp.coo_matrix((hv, (rows, cols)), shape=(nv, nv)).tocsr() - sigma * sp.tril(H_ref)).tocoo()
    e_h = np.abs(D.data).max() if D.nnz else 0.0
    print("Hessian err %.2e (max|ref| %.3e, %d values)" % (e_h, sigma * np.abs(H_ref.data).max(), len(hv)))
    assert e_h <= 1e-12 * sigma * np.abs(H_ref.data).max()
    assert ctx.get_option("last_objective_launches") == 1
    return val, grad, hv


@pytest.mark.parametrize("config,nv", [(2, 1), (2, 2), (3, 1), (3, 2)])
def test_value_gradient_hessian_against_closed_forms(config, nv):
    s, case = _case(config, nv)
    ctx = _full(case)
    goal = _unitary(s.levels, np.random.default_rng(config))
    w = np.array([0.7, 0.3, 1.9])[: nv + 1]
    regs = _regs(case)
    ctx.set_goal(po.operator_to_iso_vec(goal))
    ctx.set_weights(w)
    for r in regs:
        ctx.add_regularizer(*r)
    _check_values(ctx, case, w, goal, None, regs)
    # without a goal the infidelity term is absent; without anything the call is refused
    ctx.set_option("var_full", 0)
    ctx.set_option("var_full", 1)
    with pytest.raises(pa.PclError) as ei:
        ctx.objective(case.Z.reshape(-1), Q)
    assert ei.value.code == EINVAL
    ctx.set_weights(w)
    _check_values(ctx, case, w, None, None, [])
    ctx.close()


def test_embedded_subspace_goal_and_regularisers():
    s, case = _case(2, 2, seed=5)
    ctx = _full(case)
    sub = [0, 1, 3]
    Gs = _unitary(3, np.random.default_rng(8))
    ctx.set_goal_subspace(po.operator_to_iso_vec(Gs), sub)
    w = np.array([1.0, 0.0, 2.5])
    ctx.set_weights(w)
    regs = _regs(case)
    for r in regs:
        ctx.add_regularizer(*r)
    _check_values(ctx, case, w, po.embed(Gs, sub, s.levels), sub, regs)
    ctx.close()


@pytest.mark.parametrize("config", [2, 3])
def test_gradient_and_hessian_against_finite_differences(config):
    s, case = _case(config, 2, N=4, seed=7)
    ctx = _full(case)
    goal = _unitary(s.levels, np.random.default_rng(1))
    w = np.array([0.9, 0.4, 1.3])
    regs = _regs(case)
    ctx.set_goal(po.operator_to_iso_vec(goal))
    ctx.set_weights(w)
    for r in regs:
        ctx.add_regularizer(*r)
    Z = case.Z.reshape(-1)
    rng = np.random.default_rng(2)
    if config == 2:  # the device's gradient against central differences of the numpy value
        fd = po.numerical_gradient(lambda z: rt.objective(case, z, w, Q, goal, None, regs)[0], Z)
        g = ctx.objective(Z, Q)[1]
        assert np.abs(g - fd).max() < 1e-6 * max(1.0, np.abs(fd).max())
    rows, cols = ctx.objective_hess_structure()
    L = sp.coo_matrix((ctx.objective_hess(Z, Q, 1.0), (rows, cols)), shape=(Z.size, Z.size)).tocsr()
    H = L + sp.tril(L, -1).T
    for _ in range(4):  # H e against central differences of the device's own gradient
        e = rng.standard_normal(Z.size)
        e /= np.linalg.norm(e)
        fd = (ctx.objective(Z + 1e-6 * e, Q)[1] - ctx.objective(Z - 1e-6 * e, Q)[1]) / 2e-6
        err = np.abs(H @ e - fd).max()
        print("H e vs fd: %.2e (max|fd| %.3e)" % (err, np.abs(fd).max()))
        assert err < 1e-6 * max(1.0, np.abs(fd).max())
    ctx.close()


def test_the_switch():
    s, case = _case(2, 1)
    ctx = rt.var_context(pa, case)
    Z = case.Z.reshape(-1)
    goal = po.operator_to_iso_vec(np.eye(4))

    def refused():
        for call in (lambda: ctx.set_goal(goal), lambda: ctx.set_weights(None), lambda: ctx.clear_regularizers(), lambda: ctx.rollout(Z),
                     lambda: ctx.objective(Z, Q), lambda: ctx.objective_hess_structure(), lambda: ctx.add_regularizer(case.u_off, case.m, 1.0, 2)):  # fmt: skip
            with pytest.raises(pa.PclError) as ei:
                call()
            assert ei.value.code == ENOTIMPL and REFUSAL in str(ei.value)

    assert ctx.get_option("var_full") == 0
    refused()
    ctx.set_option("var_full", 1)
    assert ctx.get_option("var_full") == 1
    ctx.set_goal(goal)
    ctx.add_regularizer(case.u_off, case.m, 1.0, 2)
    v1 = ctx.objective(Z, Q)[0][0]
    assert np.isfinite(v1)
    ctx.set_option("var_full", 0)
    refused()
    ctx.set_option("var_full", 1)  # goal, weights and regularisers were dropped
    with pytest.raises(pa.PclError) as ei:
        ctx.objective(Z, Q)
    assert ei.value.code == EINVAL
    with pytest.raises(pa.PclError) as ei:
        ctx.set_option("var_full", 2)
    assert ei.value.code == EINVAL
    # what stays refused whatever the option says
    import torch

    Zd = torch.from_numpy(Z).cuda()
    out = torch.zeros(4, dtype=torch.float64, device="cuda")
    for call in (lambda: ctx.infidelity_dev(Zd, Q, out, None), lambda: ctx.merit_grad_len(), lambda: ctx.set_member_window(0, 1)):
        with pytest.raises(pa.PclError) as ei:
            call()
        assert ei.value.code == ENOTIMPL
    ctx.close()
    plain = rt.plain_context(pa, case)
    assert plain.get_option("var_full") == 0
    plain.set_option("var_full", 0)
    with pytest.raises(pa.PclError) as ei:
        plain.set_option("var_full", 1)
    assert ei.value.code == EINVAL
    plain.close()


@pytest.mark.parametrize("index_base", [0, 1])
def test_structure(index_base):
    s, case = _case(2, 2)
    ctx = _full(case, index_base=index_base)
    ctx.set_goal(po.operator_to_iso_vec(np.eye(4)))
    regs = _regs(case)
    for r in regs:
        ctx.add_regularizer(*r)
    nv, L = case.Z.size, case.xdc
    tri, per_knot = L * (L + 1) // 2, (2 * case.m + 1) + 2 * L + 1
    counts = {}
    for w in ([1.0, 0.5, 0.25], [1.0, 0.0, 0.25], [1.0, 0.0, 0.0]):
        ctx.set_weights(w)
        rows, cols = ctx.objective_hess_structure()
        assert rows.min() >= index_base and rows.max() < nv + index_base and cols.min() >= index_base
        assert np.all(rows >= cols) and len(np.unique(rows * (nv + 1) + cols)) == len(rows)
        n_sens = sum(1 for x in w[1:] if x != 0)
        absorbed = L if w[1] != 0 else 0  # the regulariser on variation 1: its terminal-knot diagonal belongs to that variation's triangle
        assert len(rows) == (1 + n_sens) * tri + case.N * per_knot - absorbed
        counts[n_sens] = len(rows)
        # the values land where the structure says: against the truth, position by position
        hv = ctx.objective_hess(case.Z.reshape(-1), Q, 1.0)
        H_ref = rt.objective(case, case.Z, w, Q, np.eye(4), None, regs, want_hess=True)[2]
        D = (sp.coo_matrix((hv, (rows - index_base, cols - index_base)), shape=(nv, nv)).tocsr() - sp.tril(H_ref)).tocoo()
        assert (np.abs(D.data).max() if D.nnz else 0.0) <= 1e-12 * np.abs(H_ref.data).max()
    assert counts[2] > counts[1] > counts[0]
    ctx.close()


def test_ket_context():
    s, case = _case(3, 1, ket=True, N=6)
    ctx = _full(case)
    rng = np.random.default_rng(4)
    psi = rng.standard_normal(s.levels) + 1j * rng.standard_normal(s.levels)
    psi /= np.linalg.norm(psi)
    A = np.stack([np.concatenate([psi.real, psi.imag]), np.concatenate([-psi.imag, psi.real])])
    ctx.set_goal_form(0, A, None)
    regs = [(case.u_off, case.m, 0.5, 2), (case.xo[1], case.xdc, 0.1, 1), (case.xo[0], case.xdc, 0.2, 0)]
    for r in regs:
        ctx.add_regularizer(*r)
    ctx.set_weights([1.0, 0.0])
    Z = case.Z.reshape(-1)
    val, grad = ctx.objective(Z, Q)
    x = case.Z[-1, case.xo[0] : case.xo[0] + case.xdc]
    F = po.ket_fidelity_loss(x, psi)
    v_ref = Q * abs(1 - F)
    g_ref = np.zeros_like(case.Z)
    g_ref[-1, case.xo[0] : case.xo[0] + case.xdc] = -np.sign(1 - F) * Q * 2 * ((A[0] @ x) * A[0] + (A[1] @ x) * A[1])
    for r in regs:
        v_ref += po.quadratic_regularizer(case.Z, r[0], r[1], r[2], case.dt_off, r[3])
        g_ref += po.quadratic_regularizer_gradient(case.Z, r[0], r[1], r[2], case.dt_off, r[3])
    assert abs(val[0] - v_ref) <= 1e-12 * max(1.0, abs(v_ref))
    assert np.abs(grad - g_ref.reshape(-1)).max() <= 1e-12 * np.abs(g_ref).max()
    rows, cols = ctx.objective_hess_structure()
    # (the regulariser on the state itself: its terminal-knot diagonal belongs to the goal's triangle)
    assert np.all(rows >= cols) and len(rows) == case.xdc * (case.xdc + 1) // 2 + case.N * ((2 * case.m + 1) + 2 * case.xdc + case.xdc) - case.xdc
    assert len(np.unique(rows * Z.size + cols)) == len(rows)
    L_ = sp.coo_matrix((ctx.objective_hess(Z, Q, 1.0), (rows, cols)), shape=(Z.size, Z.size)).tocsr()
    H = L_ + sp.tril(L_, -1).T
    e = rng.standard_normal(Z.size)
    fd = (ctx.objective(Z + 1e-6 * e, Q)[1] - ctx.objective(Z - 1e-6 * e, Q)[1]) / 2e-6
    assert np.abs(H @ e - fd).max() < 1e-6 * max(1.0, np.abs(fd).max())
    with pytest.raises(pa.PclError) as ei:
        ctx.set_weights([1.0, 1.0])
    assert ei.value.code == ENOTIMPL
    with pytest.raises(pa.PclError) as ei:  # scope 1 stays refused (called on the library: the mirror has no joint form for this context)
        ctx._L.pcl_set_goal_form.argtypes = [pa.integrators.ctypes.c_void_p, pa.integrators.ctypes.c_int32, pa.integrators.ctypes.c_int32,
                                             pa.integrators.ctypes.c_void_p, pa.integrators.ctypes.c_void_p]  # fmt: skip
        ctx._chk(ctx._L.pcl_set_goal_form(ctx._h, 1, 2, A.ctypes.data, None))
    assert ei.value.code == ENOTIMPL
    with pytest.raises(pa.PclError) as ei:  # a unitary goal on a ket context
        ctx._chk(ctx._L.pcl_set_goal(ctx._h, pa.integrators._ptr(np.zeros(case.xdc))))
    assert ei.value.code == ENOTIMPL
    for bad, field in (([1.0, -0.5], "w[1]"), ([np.nan, 0.0], "w[0]"), ([np.inf, 0.0], "w[0]")):
        with pytest.raises(pa.PclError) as ei:
            ctx.set_weights(bad)
        assert ei.value.code == EINVAL and field in str(ei.value)
    assert ctx.objective(Z, Q)[0][0] == val[0]  # the refused weights changed nothing
    ctx.close()


def test_default_weights_and_pointer_paths_give_the_same_bits():
    import torch

    s, case = _case(3, 2)
    ctx = _full(case)
    ctx.set_goal(po.operator_to_iso_vec(_unitary(s.levels, np.random.default_rng(6))))
    for r in _regs(case):
        ctx.add_regularizer(*r)
    Z = case.Z.reshape(-1)
    ctx.set_weights(None)
    v0, g0 = ctx.objective(Z, Q)
    h0 = ctx.objective_hess(Z, Q, 1.0)
    ctx.set_weights([1.0, 0.0, 0.0])
    v1, g1 = ctx.objective(Z, Q)
    assert v0[0] == v1[0] and np.array_equal(g0, g1) and np.array_equal(h0, ctx.objective_hess(Z, Q, 1.0))
    ctx.set_weights([0.6, 0.2, 1.1])
    v, g = ctx.objective(Z, Q)
    h = ctx.objective_hess(Z, Q, 0.7)
    Zd = torch.from_numpy(Z).cuda()
    vd = torch.zeros(1, dtype=torch.float64, device="cuda")
    gd = torch.full((Z.size,), np.nan, dtype=torch.float64, device="cuda")
    hd = torch.full((h.size + 1,), np.nan, dtype=torch.float64, device="cuda")
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.objective_dev(Zd, Q, vd, gd)
    ctx.objective_hess_dev(Zd, Q, 0.7, hd[1:])  # (a values array that is not 16-byte aligned)
    vo = torch.zeros(1, dtype=torch.float64, device="cuda")
    ctx.objective_dev(Zd, Q, vo, None)  # value only
    torch.cuda.synchronize()
    assert vd.item() == v[0] and vo.item() == v[0] and np.array_equal(gd.cpu().numpy(), g) and np.array_equal(hd[1:].cpu().numpy(), h)
    assert ctx.get_option("last_objective_launches") == 1
    v2, g2 = ctx.objective(Z, Q)
    assert v2[0] == v[0] and np.array_equal(g2, g)
    ctx.close()


def _mirror_problem(nv=2):
    s, case = _case(2, nv, seed=9)
    names = ["Ũ⃗"] + ["Ũ⃗_var%d" % (i + 1) for i in range(nv)]
    comps = {nm: case.Z[:, o : o + case.xdc].T for nm, o in zip(names, case.xo)}
    comps["Δt"], comps["t"] = case.Z[:, case.dt_off][None], case.Z[:, case.dt_off + 1][None]
    comps["u"] = case.Z[:, case.u_off : case.u_off + case.m].T
    traj = pa.NamedTrajectory(comps, controls=("u", "Δt"), timestep="Δt")
    assert np.array_equal(traj.datavec, case.Z.reshape(-1))
    Hv = [h_var_drift(2, 2), po.lift_operator(po.annihilate(2) + po.annihilate(2).conj().T, 2, [2, 2])][:nv]
    vs = pa.VariationalQuantumSystem(s.H_drift, list(s.H_drives), Hv, [1.0] * s.n_drives)
    B = pa.VariationalUnitaryIntegrator(vs, traj, names[0], names[1:], "u", scales=[10.0] * nv, pade_order=4)
    return s, case, traj, names, B


def test_through_the_mirror():
    s, case, traj, names, B = _mirror_problem()
    goal = _unitary(4, np.random.default_rng(12))
    Qs, scale, R = 3.0, 1.7, 0.05
    J = (pa.UnitaryInfidelityObjective(goal, names[0], traj, Q=Q) + pa.UnitarySensitivityObjective(names[2], traj, [traj.N], Qs=[Qs], scale=scale)
         + pa.QuadraticRegularizer("u", traj, R) + pa.QuadraticRegularizer(names[1], traj, 0.3, dt_power=1))  # fmt: skip
    with pytest.raises(pa.PclError):  # a freshly constructed integrator refuses
        B.ctx.set_weights(None)
    val, grad = J.bind(B).value_and_gradient(traj)
    x0, x2 = (case.Z[-1, case.xo[b] : case.xo[b] + case.xdc] for b in (0, 2))
    v_ref = (po.unitary_infidelity(x0, goal, Q) + rt.sens_loss(x2, Qs * scale**4) + po.quadratic_regularizer(case.Z, case.u_off, case.m, R, case.dt_off, 2)
             + po.quadratic_regularizer(case.Z, case.xo[1], case.xdc, 0.3, case.dt_off, 1))  # fmt: skip
    w = [1.0, 0.0, Qs * scale**4]
    regs = [(case.u_off, case.m, R, 2), (case.xo[1], case.xdc, 0.3, 1)]
    v2, g_ref, H_ref = rt.objective(case, case.Z, w, Q, goal, None, regs, want_hess=True)
    assert abs(v_ref - v2) <= 1e-13 * abs(v_ref)
    assert abs(val - v_ref) <= 1e-12 * max(1.0, abs(v_ref))
    assert np.abs(grad - g_ref.reshape(-1)).max() <= 1e-12 * np.abs(g_ref).max()
    rows, cols = J.hessian_structure()
    nvar = case.Z.size
    D = (sp.coo_matrix((J.hessian(traj, 0.5), (rows, cols)), shape=(nvar, nvar)).tocsr() - 0.5 * sp.tril(H_ref)).tocoo()
    assert np.abs(D.data).max() <= 1e-12 * 0.5 * np.abs(H_ref.data).max()
    with pytest.raises(NotImplementedError):
        pa.UnitarySensitivityObjective(names[1], traj, [traj.N - 1, traj.N])
    with pytest.raises(ValueError, match="component 0"):
        pa.Objective([pa.UnitaryInfidelityObjective(goal, names[1], traj, Q=Q)]).bind(B)
    with pytest.raises(ValueError, match="variations"):
        pa.Objective([pa.UnitarySensitivityObjective(names[0], traj, [traj.N])]).bind(B)
    B.close()
