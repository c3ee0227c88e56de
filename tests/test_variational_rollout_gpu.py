"""GPU tests of the rollout of a variational context (option var_full): the stacked states [X; Xv_1; ..] at every knot against the oracle's
exact rollout of the lifted system (tests/robust_truth.py), relative to max|truth|: 1e-11 at default steps (the plain rollout's tolerance in
tests/test_parity_gpu.py), 1e-10 with the steps stretched up to 40-fold (the plain large-step test's).  Component 0 has the bits of a plain
context's rollout; the variations equal the central difference of two plain rollouts, a check that does not rest on lifting."""
import dataclasses
import types

import numpy as np
import pytest

import piccolo_jl_amd as pa
import robust_truth as rt
from oracle import pade_oracle as po
from shape_cases import controlled_hermitians, plain_system
from variational_truth import h_var_drift, make_case

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max()


def _config_case(config, nv, N=6, seed=3, **kw):
    s = po.config_system(config)
    lv, ns = (2, 2) if config == 2 else (3, 3)
    Hv = [h_var_drift(lv, ns), po.lift_operator(po.annihilate(lv) + po.annihilate(lv).conj().T, 2, [lv] * ns)][:nv]
    return make_case(s, [po.G_of_H(h) / 10 for h in Hv], N=N, seed=seed, **kw)


def _shape_case(d, drive_mags, nv, seed, N=4, **kw):
    """a general system of tests/shape_cases.py with nv variation generators of its drift's kind"""
    rng = np.random.default_rng(seed)
    H0, Hd = controlled_hermitians(d, drive_mags, rng) if drive_mags else (controlled_hermitians(d, [[0]], rng)[0], [])
    Hv = [controlled_hermitians(d, [], rng)[0] for _ in range(nv)]
    so = types.SimpleNamespace(levels=d, n_drives=len(Hd), G_drift=po.G_of_H(H0),
                               G_drives=[po.G_of_H(H) for H in Hd] if Hd else np.zeros((0, 2 * d, 2 * d)))  # fmt: skip
    return make_case(so, [po.G_of_H(h) for h in Hv], N=N, seed=seed, **kw)


def _s5_case(nv, N=4):
    """d = 32: the system S5 of tests/shape_cases.py"""
    G0, Gj = plain_system("S5")
    rng = np.random.default_rng(55)
    so = types.SimpleNamespace(levels=32, n_drives=len(Gj), G_drift=G0, G_drives=list(Gj))
    Hv = [controlled_hermitians(32, [], rng)[0] for _ in range(nv)]
    return make_case(so, [po.G_of_H(h) for h in Hv], N=N, seed=5)


def _rollout(case):
    ctx = rt.var_context(pa, case)
    ctx.set_option("var_full", 1)
    X = ctx.rollout(case.Z.reshape(-1))
    assert X.shape == (1, case.N, case.xd)
    ctx.close()
    return X[0]


def _check(case, tol):
    X, T = _rollout(case), rt.lifted_rollout(case)
    err = _rel(X, T)
    print("rollout: %.2e of max|truth| %.3e" % (err, np.abs(T).max()))
    assert np.array_equal(X[0], np.concatenate([case.Z[0, o : o + case.xdc] for o in case.xo]))  # knot 0 is the input
    assert err <= tol
    return X


CASES = {
    "config2-v1": lambda: _config_case(2, 1),
    "config2-v2": lambda: _config_case(2, 2),
    "config3-v1": lambda: _config_case(3, 1),
    "config3-v2": lambda: _config_case(3, 2),
    "config3-ket-v2": lambda: _config_case(3, 2, ket=True),
    "config2-ket-v1": lambda: _config_case(2, 1, ket=True),
    "drift-only-d12": lambda: _shape_case(12, [], 2, seed=21),
    "d25-v1": lambda: _shape_case(25, [[0, 1], [2], [0]], 1, seed=22),
    "d25-v2": lambda: _shape_case(25, [[0, 1], [2], [0]], 2, seed=23),
    "d31-v2": lambda: _shape_case(31, [[0], [1]], 2, seed=24),
    "d32-S5-v1": lambda: _s5_case(1),
    "d32-S5-v2": lambda: _s5_case(2),
    "d32-ket-v2": lambda: _shape_case(32, [[0, 1], [2]], 2, seed=25, ket=True),
    "N2": lambda: _config_case(3, 1, N=2),
    # components stored out of order, with gaps: [pad | Xv_2 | u | X | dt | t | Xv_1 | pad]
    "knot-layout": lambda: _config_case(2, 2, xo=[40, 80, 3], u_off=35, dt_off=72, t_off=73, z_dim=115),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_rollout_against_the_lifted_oracle(name):
    _check(CASES[name](), 1e-11)


@pytest.mark.parametrize("name,stretch", [("config2-v2", 40.0), ("config3-v2", 40.0), ("config3-v1", 7.0), ("d32-S5-v2", 12.0), ("config3-ket-v2", 40.0)])
def test_rollout_with_stretched_steps(name, stretch):
    case = CASES[name]()
    case.Z[:, case.dt_off] *= np.linspace(1.0, stretch, case.N)
    _check(case, 1e-10)


@pytest.mark.parametrize("name", ["config2-v2", "config3-v1", "config3-v2", "d32-S5-v2", "knot-layout", "config3-ket-v2"])
def test_component_0_has_the_bits_of_a_plain_rollout(name):
    """The T recurrence of the pair kernel is the plain kernel's, and so is the product X <- E X: the same bits."""
    case = CASES[name]()
    X = _rollout(case)
    plain = rt.plain_context(pa, case)
    Xp = plain.rollout(case.Z.reshape(-1))[0]
    plain.close()
    assert np.array_equal(X[:, : case.xdc], Xp)


@pytest.mark.parametrize("config", [2, 3])
def test_variation_equals_central_difference_of_plain_rollouts(config):
    """With Xv_1 = 0 at knot 0 the rolled-out Xv_1 is d/d eps of the plain rollout with drift G0 + eps Gv_1.  The device's two plain rollouts
    are differenced at eps = 1e-4; the bound is the truncation error of that difference, measured on the CPU with the oracle's exact rollout
    against the lifted truth, plus 2 * 1e-11 max|X| / (2 eps) for the plain rollout's tested accuracy."""
    eps = 1e-4
    case = _config_case(config, 1, N=8, noise=0.0)
    case.Z[0, case.xo[1] : case.xo[1] + case.xdc] = 0.0
    X = _rollout(case)
    Xv = X[:, case.xdc :]
    outs = []
    for sgn in (+1, -1):
        plain = rt.plain_context(pa, dataclasses.replace(case, G0=case.G0 + sgn * eps * case.Gv[0]))
        outs.append(plain.rollout(case.Z.reshape(-1))[0])
        plain.close()
    fd_dev = (outs[0] - outs[1]) / (2 * eps)
    truth = rt.lifted_rollout(case)
    trunc = np.abs(rt.fd_sensitivity_rollout(case, 1, eps) - truth[:, case.xdc :]).max()
    bound = trunc + 2 * 1e-11 * np.abs(truth[:, : case.xdc]).max() / (2 * eps)
    err = np.abs(Xv - fd_dev).max()
    print("config %d: |Xv - fd| %.2e, bound %.2e (truncation %.2e), max|Xv| %.3e" % (config, err, bound, trunc, np.abs(Xv).max()))
    assert np.abs(Xv).max() > 1e-3
    assert err <= bound


def test_pointer_paths_and_repeated_calls_give_the_same_bits():
    import torch

    case = CASES["config3-v2"]()
    ctx = rt.var_context(pa, case)
    ctx.set_option("var_full", 1)
    Z = case.Z.reshape(-1)
    X1 = ctx.rollout(Z).copy()
    X2 = ctx.rollout(Z)
    Zd = torch.from_numpy(Z).cuda()
    out = torch.full((case.N * case.xd,), np.nan, dtype=torch.float64, device="cuda")
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.rollout_dev(Zd, out)
    torch.cuda.synchronize()
    assert np.array_equal(X1, X2) and np.array_equal(out.cpu().numpy().reshape(X1.shape), X1)
    ctx.close()


def test_through_the_mirror():
    s = po.config_system(2)
    case = _config_case(2, 1)
    names = ["Ũ⃗", "Ũ⃗_var1"]
    comps = {nm: case.Z[:, o : o + case.xdc].T for nm, o in zip(names, case.xo)}
    comps["Δt"], comps["t"] = case.Z[:, case.dt_off][None], case.Z[:, case.dt_off + 1][None]
    comps["u"] = case.Z[:, case.u_off : case.u_off + case.m].T
    traj = pa.NamedTrajectory(comps, controls=("u", "Δt"), timestep="Δt")
    vs = pa.VariationalQuantumSystem(s.H_drift, list(s.H_drives), [h_var_drift(2, 2)], [1.0] * s.n_drives)
    B = pa.VariationalUnitaryIntegrator(vs, traj, names[0], names[1:], "u", scales=[10.0], pade_order=4)
    with pytest.raises(pa.PclError):  # a freshly constructed integrator refuses
        B.ctx.rollout(traj.datavec)
    X = pa.variational_rollout(B, traj)
    assert X.shape == (case.xd, case.N)
    assert _rel(X.T, rt.lifted_rollout(case)) <= 1e-11
    assert np.array_equal(B.rollout(traj), X.T)
    B.close()
