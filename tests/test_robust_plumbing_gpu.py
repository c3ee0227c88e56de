"""A robust single-qubit gate (the Pauli system of the reference's variational test item, H_var = Z/2, one variation) solved through scipy's
trust-constr with every callback on the device: variational residual, Jacobian and Hessian of the Lagrangian, and the objective
UnitaryInfidelityObjective + UnitarySensitivityObjective + regularisers with its gradient and Hessian.  Asserted: what must hold -- the
callbacks' dimensions, the outcome bounds of the plain plumbing test, an objective that went down, and the variational rollout of the solved
controls against the trajectory's own states.  How far the sensitivity dropped is printed, not asserted."""
import os
import sys

import numpy as np
import pytest

from oracle import pade_oracle as po
from variational_truth import VarCase, lifted

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))

pytestmark = pytest.mark.gpu


def test_robust_gate_plumbing_solve():
    import plumbing_robust

    N = 30
    r = plumbing_robust.solve(N=N, max_iter=300, seed=0)
    z_dim = 8 + 8 + 2 + 3 * 2
    n_vars, n_rows = z_dim * N, (16 + 2 + 2 + 1) * (N - 1)
    d = r["dims"]
    assert d == dict(n_vars=n_vars, n_rows=n_rows, obj_grad=n_vars, cons=n_rows, cons_jac=(n_rows, n_vars), cons_hess=(n_vars, n_vars), obj_hess=(n_vars, n_vars))
    print("fidelity %.6f  violation %.2e  iterations %d  objective %.4f -> %.4f  sensitivity %.4f -> %.4f" % (
        r["fidelity"], r["max_violation"], r["iterations"], r["objective_initial"], r["objective_final"], r["sensitivity_initial"], r["sensitivity_final"]))  # fmt: skip
    assert r["fidelity"] > 0.9, r["fidelity"]
    assert r["max_violation"] < 1e-2, r["max_violation"]
    assert r["objective_final"] < r["objective_initial"]
    # the rollout of the solved controls stays within 2 N max|exp residual| + 1e-12 of the trajectory's own states
    traj, sysv = r["traj"], r["system"]
    Z = traj.datavec.reshape(N, -1)
    names = ["Ũ⃗", "Ũ⃗_var"]
    case = VarCase(Z=Z, z_dim=Z.shape[1], N=N, n=4, C=2, m=2, xo=[traj.components[nm].start for nm in names], u_off=traj.components["u"].start,
                   dt_off=traj.components["Δt"].start, G0=sysv.G_drift, Gv=[sysv.G_vars_array()[0]], Gj=sysv.G_drives_array())  # fmt: skip
    Zl, lay, G0l, Gjl = lifted(case)
    res = np.abs(po.exp_residual(Zl, lay, G0l, Gjl)).max()
    own = np.concatenate([Z[:, o : o + case.xdc] for o in case.xo], axis=1)
    err = np.abs(r["rollout"].T - own).max()
    print("rollout vs the trajectory's states: %.2e (max|exp residual| %.2e)" % (err, res))
    assert err <= 2 * N * res + 1e-12
