"""The X-gate plumbing solve on a context of the exponential constraint WITH its Hessian of the Lagrangian (scripts/plumbing_exp_newton.py:
``pade_order="exp", exp_hessian=True``): GPU residual, Jacobian and the constraints' exact second-order term behind a CPU NLP solver.
Outcome asserts are the reference's integration-test bounds, as tests/test_plumbing_gpu.py and tests/test_exp_plumbing_gpu.py:
`fidelity > 0.9`, `norm(delta, Inf) < 1e-2` [REF src/control/templates/smooth_pulse_problem.jl:745-785], and the rolled-out terminal state is
the trajectory's within the accumulated violation, 2 N max|delta| + 1e-12.  The iteration count is printed beside the quasi-Newton run's
(scripts/plumbing_exp.py) and recorded in DESIGN.md section 4.11; there is no threshold on it."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))

pytestmark = pytest.mark.gpu


def test_xgate_solve_with_the_exact_constraint_hessian():
    import plumbing_exp
    import plumbing_exp_newton

    N = 50
    r = plumbing_exp_newton.solve(N=N, max_iter=300, seed=0)
    print({k: v for k, v in r.items() if k != "traj"})
    assert r["n_vars"] == 16 * N and r["n_rows"] == (8 + 2 + 2 + 1) * (N - 1)
    assert r["fidelity"] > 0.9, r
    assert r["max_violation"] < 1e-2, r
    assert r["rollout_terminal_gap"] <= 2 * N * r["max_dynamics_violation"] + 1e-12, r
    q = plumbing_exp.solve(N=N, max_iter=300, seed=0)
    print("iterations: exact constraint Hessian %d (fidelity %.6f, violation %.2e) | quasi-Newton %d (fidelity %.6f, violation %.2e)"
          % (r["iterations"], r["fidelity"], r["max_violation"], q["iterations"], q["fidelity"], q["max_violation"]))  # fmt: skip


def test_hessian_of_the_lagrangian_is_complete_on_the_device():
    """tests/test_plumbing_gpu.py's check of the same name on this mode, with its numbers: sigma grad^2 f + sum_i mu_i grad^2 g_i from the device
    (pcl_objective_hess; pcl_hess on the exponential context + the derivative rows) is symmetric to 1e-12 relative, and along six random unit
    directions it equals the central difference (step 1e-6) of the device's own grad f + J' mu within 1e-6 max(1, |fd|_inf)."""
    import numpy as np

    import plumbing_exp_newton

    cb = plumbing_exp_newton.solve(N=12, callbacks_only=True)
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
