"""CPU tests of the robust-control objective: the host mirror's argument checks, and the truth helper (tests/robust_truth.py) checked against
itself -- closed-form gradient and Hessian against finite differences, the lifted rollout against the finite-difference construction."""
import dataclasses

import numpy as np
import pytest

import piccolo_jl_amd as pa
import robust_truth as rt
from oracle import pade_oracle as po
from variational_truth import h_var_drift, make_case


def _traj(N=5):
    U = np.zeros((8, N))
    U[:, 0] = pa.operator_to_iso_vec(np.eye(2))
    return pa.NamedTrajectory({"Ũ⃗": U, "Ũ⃗_var": np.zeros((8, N)), "u": np.zeros((2, N)), "Δt": np.full((1, N), 0.1)}, controls=("u", "Δt"), timestep="Δt")


def test_sensitivity_objective_arguments():
    traj = _traj()
    t = pa.UnitarySensitivityObjective("Ũ⃗_var", traj, [traj.N], Qs=[2.0], scale=3.0)
    assert t.weight == 2.0 * 81.0 and t.times == [traj.N]
    assert pa.UnitarySensitivityObjective("Ũ⃗_var", traj, traj.N).weight == 1.0
    for times in ([1], [traj.N - 1], [traj.N - 1, traj.N], []):
        with pytest.raises(NotImplementedError, match="terminal knot"):
            pa.UnitarySensitivityObjective("Ũ⃗_var", traj, times)
    with pytest.raises(KeyError):
        pa.UnitarySensitivityObjective("nope", traj, [traj.N])
    with pytest.raises(ValueError):
        pa.UnitarySensitivityObjective("Ũ⃗_var", traj, [traj.N], Qs=[1.0, 2.0])
    with pytest.raises(ValueError):
        pa.UnitarySensitivityObjective("Ũ⃗_var", traj, [traj.N], Qs=[-1.0])
    J = pa.UnitaryInfidelityObjective(np.eye(2), "Ũ⃗", traj) + t + pa.QuadraticRegularizer("u", traj, 1e-2)
    assert len(J.terms) == 3


def test_sensitivity_objective_needs_a_variational_integrator():
    class Plain:  # stands for an integrator with a plain context
        ctx = type("C", (), {"variational": False})()
        x_names = ["Ũ⃗"]

    traj = _traj()
    with pytest.raises(ValueError, match="variational integrator"):
        pa.Objective([pa.UnitarySensitivityObjective("Ũ⃗_var", traj, [traj.N])]).bind(Plain())
    with pytest.raises(TypeError):
        pa.variational_rollout(Plain(), traj)


def _case(nv=2):
    s = po.config_system(2)
    Hv = [h_var_drift(2, 2), po.lift_operator(po.annihilate(2) + po.annihilate(2).conj().T, 2, [2, 2])][:nv]
    case = make_case(s, [po.G_of_H(h) / 10 for h in Hv], N=4, seed=1)
    rng = np.random.default_rng(0)
    for b in range(1, nv + 1):
        case.Z[-1, case.xo[b] : case.xo[b] + case.xdc] = 0.3 * rng.standard_normal(case.xdc)
    return case


def test_sensitivity_closed_forms():
    rng = np.random.default_rng(3)
    x = rng.standard_normal(32)
    U = po.iso_vec_to_operator(x)
    assert abs(rt.sens_loss(x, 2.5) - 2.5 * (x @ x) ** 2 / 16) < 1e-12 * rt.sens_loss(x, 2.5)
    assert abs(np.trace(U.conj().T @ U) - x @ x) < 1e-12 * (x @ x)
    g = po.numerical_gradient(lambda y: rt.sens_loss(y, 2.5), x)
    assert np.abs(g - rt.sens_grad(x, 2.5)).max() < 1e-6 * np.abs(g).max()
    H = rt.sens_hess(x, 2.5)
    for _ in range(3):
        e = rng.standard_normal(32)
        fd = (rt.sens_grad(x + 1e-6 * e, 2.5) - rt.sens_grad(x - 1e-6 * e, 2.5)) / 2e-6
        assert np.abs(H @ e - fd).max() < 1e-6 * np.abs(fd).max()


@pytest.mark.parametrize("subspace", [None, [0, 1, 3]])
def test_objective_truth_against_finite_differences(subspace):
    case = _case()
    rng = np.random.default_rng(5)
    ns = 4 if subspace is None else len(subspace)
    G = np.linalg.qr(rng.standard_normal((ns, ns)) + 1j * rng.standard_normal((ns, ns)))[0]
    goal = G if subspace is None else po.embed(G, subspace, 4)
    w = [0.7, 0.3, 1.9]
    regs = [(case.u_off, case.m, 0.5, 2), (case.xo[1], case.xdc, 0.1, 1), (case.dt_off + 1, 1, 3.0, 0)]
    Z = case.Z.reshape(-1)
    val, g, H = rt.objective(case, Z, w, 100.0, goal, subspace, regs, want_hess=True)
    fd = po.numerical_gradient(lambda z: rt.objective(case, z, w, 100.0, goal, subspace, regs)[0], Z)
    assert np.abs(fd - g.reshape(-1)).max() < 1e-6 * max(1.0, np.abs(fd).max())
    assert abs(H - H.T).max() < 1e-12 * abs(H).max()
    for _ in range(3):
        e = rng.standard_normal(Z.size)
        fd = (rt.objective(case, Z + 1e-6 * e, w, 100.0, goal, subspace, regs)[1] - rt.objective(case, Z - 1e-6 * e, w, 100.0, goal, subspace, regs)[1]) / 2e-6
        assert np.abs(H @ e - fd.reshape(-1)).max() < 1e-6 * max(1.0, np.abs(fd).max())


def test_lifted_rollout_against_the_finite_difference_construction():
    s = po.config_system(2)
    case = make_case(s, [po.G_of_H(h_var_drift(2, 2)) / 10], N=6, seed=2, noise=0.0)
    Z = case.Z.copy()
    Z[0, case.xo[1] : case.xo[1] + case.xdc] = 0.0
    case = dataclasses.replace(case, Z=Z)
    X = rt.lifted_rollout(case)
    lay, Zp = rt.plain_layout(case)
    assert np.abs(X[:, : case.xdc] - po.exact_rollout(Zp, lay, case.G0, case.Gj)).max() < 1e-13
    fd = rt.fd_sensitivity_rollout(case, 1, 1e-4)
    assert np.abs(X[:, case.xdc :]).max() > 1e-3
    assert np.abs(X[:, case.xdc :] - fd).max() < 1e-6 * np.abs(fd).max()
