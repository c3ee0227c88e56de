"""The robust two-qubit plumbing solve on the exponential constraint WITH its Hessian of the Lagrangian (scripts/plumbing_robust_exp_newton.py:
``VariationalUnitaryIntegrator(..., pade_order="exp", exp_hessian=True)`` on config 2, v = 1): GPU residual, Jacobian, the constraints' exact
second-order term (option var_exp_hess) and the objective's Hessian (var_full) behind a CPU NLP solver, next to the same solve with a
quasi-Newton model of the constraints.  The iteration counts are printed; there is no threshold on them (a short horizon and a short
iteration limit here: the test is about the plumbing, not about the optimum).  DESIGN.md section 4.13 records the script's own full-length run
(N = 20, 300 iterations allowed: 300 / 300 iterations, fidelity 0.9974 with the exact constraint Hessian, 0.0107 with the quasi-Newton model)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))

pytestmark = pytest.mark.gpu


def test_robust_solve_with_the_exact_constraint_hessian_beside_quasi_newton():
    import plumbing_robust_exp_newton as pl

    N = 10
    a = pl.solve(N=N, max_iter=40, seed=0, newton=True)
    b = pl.solve(N=N, max_iter=40, seed=0, newton=False)
    print(a)
    print(b)
    print("iterations: exact constraint Hessian %d (fidelity %.6f, violation %.2e) | quasi-Newton %d (fidelity %.6f, violation %.2e)"
          % (a["iterations"], a["fidelity"], a["max_violation"], b["iterations"], b["fidelity"], b["max_violation"]))  # fmt: skip
    for r in (a, b):
        assert r["n_vars"] == (2 * 32 + 2 + 3 * 4) * N and r["n_rows"] == (2 * 32 + 4 + 4 + 1) * (N - 1)
        assert np.isfinite([r["fidelity"], r["max_violation"], r["objective_final"], r["sensitivity_final"]]).all(), r
        assert 1 <= r["iterations"] <= 40


def test_hessian_of_the_lagrangian_is_complete_on_the_device():
    """tests/test_exp_hess_plumbing_gpu.py's check of the same name on this mode, with its numbers: sigma grad^2 f + sum_i mu_i grad^2 g_i from
    the device (pcl_objective_hess with var_full; pcl_hess with var_exp_hess + the derivative rows) is symmetric to 1e-12 relative, and along
    six random unit directions it equals the central difference (step 1e-6) of the device's own grad f + J' mu within 1e-6 max(1, |fd|_inf)."""
    import plumbing_robust_exp_newton as pl

    cb = pl.solve(N=6, callbacks_only=True)
    rng = np.random.default_rng(3)
    z = cb["z0"] + 0.05 * rng.standard_normal(cb["z0"].size)
    mu = rng.standard_normal(cb["n_rows"])
    gradL = lambda zz: cb["obj"](zz)[1] + cb["cons_jac"](zz).T @ mu
    H = (cb["obj_hess"](z) + cb["cons_hess"](z, mu)).toarray()
    assert np.abs(H - H.T).max() < 1e-12 * np.abs(H).max()
    for _ in range(6):
        e = rng.standard_normal(z.size)
        e /= np.linalg.norm(e)
        fd = (gradL(z + 1e-6 * e) - gradL(z - 1e-6 * e)) / 2e-6
        print("|H e - fd|_inf %.3e   |fd|_inf %.3e" % (np.abs(H @ e - fd).max(), np.abs(fd).max()))
        assert np.abs(H @ e - fd).max() < 1e-6 * max(1.0, np.abs(fd).max())
    cb["close"]()
