#!/usr/bin/env python3
"""A small solve on a LARGE context (generator dimension 66: a ket of 33 levels under a dense drift and two dense drives, N = 10 knots) with
everything from the device: ``BilinearIntegrator(..., large_generator=True, large_hessian=True, large_full=True)``.  GPU residual, sparse
Jacobian and the constraints' exact second-order term (``eval_hessian_of_lagrangian``; plus the derivative rows' (dt, dx) entries), the
objective -- KetInfidelityObjective + three QuadraticRegularizers -- with its gradient (and, on request, its exact Hessian: below), behind
scipy's trust-constr, as scripts/plumbing_exp_newton.py does on the exponential constraint.  The goal is the state that a known pulse reaches,
so a fidelity of 1 is attainable; the solve starts from another pulse.  Then the rollout (``unitary_rollout``: exact propagation from the
knot-0 state under the solution's controls) is compared with the objective: its terminal fidelity against the fidelity the objective sees at
the trajectory's terminal knot -- they differ by what the Pade constraint of the chosen order and the constraint violation leave.

The objective's second-order term is a BFGS model by default, as in that script: the exact Hessian of Q |1 - F| is -2 Q (a a' + b b') below the
kink, negative semidefinite, and scipy's trust-constr (no inertia correction) then shrinks its region at an infeasible point
(scripts/plumbing_xgate.py).  ``exact_hessian=True`` passes the device's objective Hessian instead -- both Hessians from the device; run as a
program, the script does one solve of each kind and prints both.  ``callbacks_only=True`` returns the callbacks (``obj_hess`` among them)
instead of solving."""
import os
import sys

import numpy as np
import scipy.linalg
import scipy.sparse as sp
from scipy.optimize import BFGS, Bounds, NonlinearConstraint, minimize

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import piccolo_jl_amd as pa


def _herm(d, rng):
    A = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
    return (A + A.conj().T) / 2


def solve(d=33, m=2, N=10, T=0.5, Q=100.0, R=1e-3, seed=0, pade_order=8, max_iter=1000, verbose=0, exact_hessian=False, callbacks_only=False):
    rng = np.random.default_rng(seed)
    system = pa.QuantumSystem(_herm(d, rng) / np.sqrt(d), [_herm(d, rng) / np.sqrt(d) for _ in range(m)], [1.0] * m)
    KET = pa.trajectory.KET
    times = np.linspace(0, T, N)
    psi0 = np.zeros(d, dtype=complex)
    psi0[0] = 1.0

    def propagate(u):
        states, psi = [], psi0
        for k in range(N):
            states.append(psi)
            if k + 1 < N:
                psi = scipy.linalg.expm(-1j * (times[k + 1] - times[k]) * system.H(u[:, k])) @ psi
        return states

    u_star = 0.5 * np.sin(np.outer(np.arange(1, m + 1), np.pi * times / T))  # the pulse that defines the goal: zero at both ends
    psi_goal = propagate(u_star)[-1]
    u0 = u_star + 0.3 * rng.standard_normal((m, N)) * np.sin(np.pi * times / T)
    traj = pa.ket_trajectory(system, u0, times, psi0, psi_goal, states=propagate(u0))
    B = pa.BilinearIntegrator(system, traj, x_name=KET, pade_order=pade_order, large_generator=True, large_hessian=True, large_full=True)
    assert B.ctx.large and B.ctx.large_hessian and B.ctx.large_full
    rows = [B, pa.DerivativeIntegrator("u", "du", traj, like=B), pa.DerivativeIntegrator("du", "ddu", traj, like=B),
            pa.DerivativeIntegrator("t", None, traj, like=B)]  # fmt: skip
    nv = traj.dim * traj.N
    structs = [pa.jacobian_structure(r) for r in rows]
    offs = np.cumsum([0] + [r.dim for r in rows])
    comp = traj.components

    def cons(z):
        traj.update(z)
        return np.concatenate([pa.evaluate_(np.zeros(r.dim), r, traj) for r in rows])

    def cons_jac(z):
        traj.update(z)
        return sp.vstack([sp.csr_matrix((r.ctx.jac(traj.datavec), (rr, cc)), shape=(r.dim, nv)) for r, (rr, cc) in zip(rows, structs)]).tocsr()

    def cons_hess(z, v):
        traj.update(z)
        H = pa.eval_hessian_of_lagrangian(B, traj, v[: B.dim])
        ii, jj, vv = [], [], []  # derivative rows: d^2/(d dt_k d dx_k[r]) = -1
        for r, o in zip(rows[1:3], offs[1:3]):
            mu = v[o : o + r.dim].reshape(N - 1, r.x_dim)
            for k in range(N - 1):
                a = k * traj.dim + comp[traj.timestep].start
                b = k * traj.dim + r.dx_off + np.arange(r.x_dim)
                ii += [np.full(r.x_dim, a), b]
                jj += [b, np.full(r.x_dim, a)]
                vv += [-mu[k], -mu[k]]
        return H + sp.csr_matrix((np.concatenate(vv), (np.concatenate(ii), np.concatenate(jj))), shape=(nv, nv))

    J = pa.Objective([pa.KetInfidelityObjective(psi_goal, KET, traj, Q=Q)])
    for c_ in ("u", "du", "ddu"):
        J = J + pa.QuadraticRegularizer(c_, traj, R, dt_power=0)
    J.bind(B)
    hr, hc = J.hessian_structure()

    def obj(z):
        return J.value_and_gradient(z)

    def obj_hess(z):  # sigma grad^2 f, lower triangle from the device -> symmetric sparse matrix
        L = sp.coo_matrix((J.hessian(z, 1.0), (hr, hc)), shape=(nv, nv)).tocsr()
        return L + sp.tril(L, -1).T

    if callbacks_only:
        return dict(z0=traj.datavec.copy(), obj=obj, obj_hess=obj_hess, cons=cons, cons_jac=cons_jac, cons_hess=cons_hess, n_rows=int(offs[-1]), close=B.close)
    lb, ub = np.full(nv, -np.inf), np.full(nv, np.inf)
    dt_i = comp[traj.timestep].start
    for k in range(N):
        o = k * traj.dim
        lb[o + comp["u"].start : o + comp["u"].stop], ub[o + comp["u"].start : o + comp["u"].stop] = -2.0, 2.0
        lb[o + dt_i] = ub[o + dt_i] = traj.datavec[o + dt_i]  # timesteps_all_equal
    z0 = traj.datavec.copy()
    x1 = slice(comp[KET].start, comp[KET].stop)
    lb[x1] = ub[x1] = z0[x1]  # initial condition
    for k in (0, N - 1):  # u(0) = u(T) = 0
        s = slice(k * traj.dim + comp["u"].start, k * traj.dim + comp["u"].stop)
        lb[s] = ub[s] = 0.0
    z0 = np.clip(z0, lb, ub)
    nc_rows = int(offs[-1])

    def fidelity_of(z):
        F = pa.Objective([pa.KetInfidelityObjective(psi_goal, KET, traj, Q=1.0)]).bind(B)
        return 1.0 - F.value_and_gradient(z, want_grad=False)[0]

    fid0 = fidelity_of(z0)
    J.bind(B)
    res = minimize(obj, z0, jac=True, method="trust-constr", hess=obj_hess if exact_hessian else BFGS(), bounds=Bounds(lb, ub, keep_feasible=False),
                   constraints=[NonlinearConstraint(cons, np.zeros(nc_rows), np.zeros(nc_rows), jac=cons_jac, hess=cons_hess)],
                   options=dict(maxiter=max_iter, gtol=1e-8, xtol=1e-12, verbose=verbose, sparse_jacobian=True))  # fmt: skip
    traj.update(res.x)
    viol = float(np.abs(cons(res.x)).max())
    dyn = float(np.abs(pa.evaluate_(np.zeros(B.dim), B, traj)).max())
    fid = fidelity_of(res.x)  # what the objective sees: the trajectory's terminal knot
    X = pa.unitary_rollout(B, traj)  # x_dim x N, from the trajectory's knot-0 state under the solution's controls
    psi_T = X[:d, -1] + 1j * X[d:, -1]
    fid_roll = float(abs(np.vdot(psi_goal, psi_T)) ** 2)
    gap = float(np.abs(X[:, -1] - traj.datavec.reshape(N, traj.dim)[-1, x1]).max())
    order = B.pade_order
    B.close()
    return dict(fidelity_start=float(fid0), fidelity=float(fid), rollout_fidelity=fid_roll, rollout_terminal_gap=gap, max_violation=viol,
                max_dynamics_violation=dyn, iterations=int(res.nit), n_vars=nv, n_rows=nc_rows, generator_dim=2 * d, pade_order=order, traj=traj)  # fmt: skip


if __name__ == "__main__":
    for exact in (False, True):
        r = solve(verbose=1, exact_hessian=exact)
        print("exact_hessian=%s:" % exact, {k: v for k, v in r.items() if k != "traj"})
