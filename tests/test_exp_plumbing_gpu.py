"""The X-gate plumbing solve on a context of the exponential constraint (scripts/plumbing_exp.py): GPU residual and Jacobian behind a CPU
NLP solver with quasi-Newton Hessians (the mode has no Hessian of the Lagrangian).  Outcome asserts are the reference's integration-test
bounds, as tests/test_plumbing_gpu.py: `fidelity > 0.9`, `norm(delta, Inf) < 1e-2` [REF src/control/templates/smooth_pulse_problem.jl:745-785];
and, since collocation and rollout are the same map in this mode, the rolled-out terminal state is the trajectory's within the accumulated
violation, 2 N max|delta| + 1e-12 (the bound tests/test_parity_gpu.py uses for rollouts of nearly feasible trajectories)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))

pytestmark = pytest.mark.gpu


def test_xgate_solve_on_the_exponential_constraint():
    import plumbing_exp

    N = 50
    r = plumbing_exp.solve(N=N, max_iter=300, seed=0)
    print({k: v for k, v in r.items() if k != "traj"})
    assert r["n_vars"] == 16 * N and r["n_rows"] == (8 + 2 + 2 + 1) * (N - 1)
    assert r["fidelity"] > 0.9, r
    assert r["max_violation"] < 1e-2, r
    assert r["rollout_terminal_gap"] <= 2 * N * r["max_dynamics_violation"] + 1e-12, r
