"""CPU tests of the variational exponential Hessian at generator dimensions 46 .. 62 (option ``var_exp_hess_tiles``: four of the octuple
chain's tiles in a device workspace, pcl_kernel_var_exp_hess_tiles.hpp): the numpy statement of the kernel's scaled recurrence
(tests/test_var_exp_hess_cpu.py) against the lifted truth of tests/var_exp_hess_truth.py at the newly served shapes, and the keyword
``exp_hessian`` of the constructors, which now takes ``False``, ``True`` or ``"workspace"``."""
import numpy as np
import pytest

import piccolo_jl_amd as pa
import var_exp_cases as cases
import var_exp_hess_truth as truth
from test_var_exp_hess_cpu import close, model, rand_mu, tiles_recurrence

NEW_SHAPES = {
    "transmon23": lambda: cases.transmon(23, N=3)[3],  # n = 46: the first shape beyond nine LDS tiles
    "transmon31": lambda: cases.transmon(31, N=3)[3],  # n = 62, theta = 5.97: five squarings
    "config3_v1": lambda: cases.config3(1, N=3)[3],  # n = 54, cols = 27 = n / 2, m = 6
    "config3_v2_ket": lambda: cases.config3(2, N=3, ket=True)[3],  # v = 2
}


@pytest.mark.parametrize("which", list(NEW_SHAPES))
def test_scaled_recurrence_equals_the_lifted_truth_at_the_new_shapes(which):
    """The reference alone stays far inside the GPU tolerance (1e-11) at these sizes.  Worst deviation read, relative to max(1, |truth|_inf):
    transmon(23) 4.3e-15, transmon(31) 6.4e-15, config 3 (v = 1) 5.9e-16, config 3 (v = 2, ket) 7.1e-16."""
    case = NEW_SHAPES[which]()
    mu = rand_mu(case, 2)
    t = truth.values(case, mu)
    err = close(model(case, mu, tiles=tiles_recurrence), t, 1e-12)
    print("%s: max|recurrence - truth| / max(1, |truth|) %.2e  (|truth|_inf %.2e)" % (which, err, np.abs(t).max()))


def test_transmon31_takes_five_squarings():
    case = NEW_SHAPES["transmon31"]()
    G = case.G0 + np.tensordot(case.Z[0, case.u_off : case.u_off + case.m], case.Gj, axes=1)
    theta = abs(case.Z[0, case.dt_off]) * np.abs(G).sum(axis=0).max()
    assert 4.0 < theta <= 8.0, theta  # theta 2^-5 <= 1/4 < theta 2^-4


def _pauli_traj(ket):
    sysv = pa.VariationalQuantumSystem(pa.PAULIS["Z"] / 2, [pa.PAULIS["X"], pa.PAULIS["Y"]], [pa.PAULIS["Z"] / 2], [1.0, 1.0])
    case = cases.pauli(ket)[3]
    names = ["ψ̃", "ψ̃_var"] if ket else ["Ũ⃗", "Ũ⃗_var"]
    comps = {nm: case.Z[:, o : o + case.xdc].T for nm, o in zip(names, case.xo)}
    comps["Δt"] = case.Z[:, case.dt_off][None]
    comps["t"] = case.Z[:, case.dt_off + 1][None]
    comps["u"] = case.Z[:, case.u_off : case.u_off + case.m].T
    return sysv, case, names, pa.NamedTrajectory(comps, controls=("u", "Δt"), timestep="Δt")


def _named(excinfo):
    msg = str(excinfo.value)
    assert "False" in msg and "True" in msg and '"workspace"' in msg, msg


@pytest.mark.parametrize("ket", [True, False])
@pytest.mark.parametrize("bad", ["anything-else", "Workspace", 2, None])
def test_exp_hessian_keyword_names_its_three_values(ket, bad):
    """Any value but False, True and "workspace": ValueError naming the three, before any device call (no device is present here)."""
    sysv, case, names, traj = _pauli_traj(ket)
    ctor = pa.VariationalKetIntegrator if ket else pa.VariationalUnitaryIntegrator
    with pytest.raises(ValueError) as ei:
        ctor(sysv, traj, names[0], names[1:], "u", pade_order="exp", exp_hessian=bad)
    _named(ei)
    with pytest.raises(ValueError) as ei:
        pa.integrators._PclContext(d=case.n // 2, m=case.m, N=case.N, z_dim=case.z_dim, u_off=case.u_off, dt_off=case.dt_off, x_offs=case.xo,
                                   G0=np.concatenate([case.G0[None], np.array(case.Gv)]), Gj=case.Gj, batch=1 + case.v,
                                   batch_mode=pa._lib.PCL_BATCH_VARIATIONAL_EXP, per_member_G0=True, pade_order=pa._lib.PCL_ORDER_EXP,
                                   state_cols=case.C, exp_hessian=bad)  # fmt: skip
    _named(ei)


@pytest.mark.parametrize("ket", [True, False])
def test_workspace_needs_the_exponential_constraint(ket):
    """``exp_hessian="workspace"`` with a Pade order: the existing ValueError of ``exp_hessian=True``."""
    sysv, case, names, traj = _pauli_traj(ket)
    ctor = pa.VariationalKetIntegrator if ket else pa.VariationalUnitaryIntegrator
    with pytest.raises(ValueError, match="exp_hessian=True is the Hessian of the Lagrangian of the exponential constraint"):
        ctor(sysv, traj, names[0], names[1:], "u", pade_order=4, exp_hessian="workspace")


def test_workspace_is_refused_on_plain_contexts():
    """A plain context or constructor of the exponential constraint: ValueError, before any device call."""
    case = cases.pauli(False)[3]
    with pytest.raises(ValueError, match="workspace"):
        pa.integrators._PclContext(d=case.n // 2, m=case.m, N=case.N, z_dim=case.z_dim, u_off=case.u_off, dt_off=case.dt_off, x_offs=[case.xo[0]],
                                   G0=case.G0, Gj=case.Gj, batch=1, batch_mode=pa._lib.PCL_BATCH_MEMBERS, pade_order=pa._lib.PCL_ORDER_EXP,
                                   state_cols=case.C, exp_hessian="workspace")  # fmt: skip
    sysv, case, names, traj = _pauli_traj(False)
    with pytest.raises(ValueError, match="workspace"):
        pa.HipPadeIntegrator(case.G0, case.Gj, traj, names[0], "u", pade_order="exp", exp_hessian="workspace")
