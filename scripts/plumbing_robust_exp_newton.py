#!/usr/bin/env python3
"""A robust two-qubit gate on the reference's own discretisation, solved with the exact constraint Hessian: BASELINE config 2 (two 2-level
transmons, d = 4, four drives), one variation (the drift-frequency direction 2 pi sum_q a_q' a_q / 10), a
``VariationalUnitaryIntegrator(..., pade_order="exp", exp_hessian=True)`` carrying U and dU/d(eps) under the exact exponential constraint, and the
objective UnitaryInfidelityObjective + UnitarySensitivityObjective(terminal knot) + regularisers.  Every callback is on the GPU: residual, sparse
Jacobian, the Hessian of the Lagrangian of the dynamics rows (``pcl_hess`` with option var_exp_hess: third Frechet derivatives of exp) and the
objective with its Hessian (``pcl_objective_hess`` with var_full).  The shape of scripts/plumbing_exp_newton.py and scripts/plumbing_robust.py:
scipy's trust-constr stands in for Ipopt; ``newton=False`` is the same solve with a quasi-Newton model in the constraints' place -- what this
mode could do before the option -- and ``__main__`` prints the iterations of both.  The objective keeps its BFGS model unless
``exact_hessian=True`` (scripts/plumbing_exp_newton.py: trust-constr has no inertia correction)."""
import os
import sys

import numpy as np
import scipy.linalg
import scipy.sparse as sp
from scipy.optimize import BFGS, Bounds, NonlinearConstraint, minimize

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import piccolo_jl_amd as pa

X_NAME, V_NAME = "Ũ⃗", "Ũ⃗_var"


def solve(N=20, T=10.0, Q=100.0, Qs=1e-2, R=1e-2, seed=0, max_iter=300, verbose=0, newton=True, exact_hessian=False, callbacks_only=False):
    base = pa.MultiTransmonSystem([4.0, 4.1], [0.2, 0.2], [[0, 0.1], [0.1, 0]], levels_per_transmon=2, drive_bounds=0.1)  # config 2
    d, m = base.levels, base.n_drives
    num = np.diag([0.0, 1.0])
    H_var = 2 * np.pi * (np.kron(num, np.eye(2)) + np.kron(np.eye(2), num)) / 10.0
    system = pa.VariationalQuantumSystem(base.H_drift, list(base.H_drives), [H_var], list(base.drive_bounds))
    U_goal = np.kron(pa.GATES["X"], np.eye(2))
    rng = np.random.default_rng(seed)
    times = np.linspace(0, T, N)
    dts = np.full(N, times[1] - times[0])
    u0 = 0.02 * rng.standard_normal((m, N))
    u0[:, 0] = u0[:, -1] = 0.0
    # initial states: exact propagation of [U; U_var] under the lifted generator, U_var(0) = 0
    n = 2 * d
    Gv = system.G_vars_array()[0]
    S = np.vstack([np.vstack([np.eye(d), np.zeros((d, d))]), np.zeros((n, d))])
    Xs, Vs = np.zeros((n * d, N)), np.zeros((n * d, N))
    for k in range(N):
        Xs[:, k], Vs[:, k] = S[:n].T.reshape(-1), S[n:].T.reshape(-1)
        G = system.G_drift + np.tensordot(u0[:, k], system.G_drives_array(), axes=1)
        S = scipy.linalg.expm(dts[k] * np.block([[G, np.zeros((n, n))], [Gv, G]])) @ S
    du = np.zeros((m, N))
    du[:, :-1] = np.diff(u0, axis=1) / dts[:-1]
    ddu = np.zeros((m, N))
    ddu[:, :-1] = np.diff(du, axis=1) / dts[:-1]
    traj = pa.NamedTrajectory({X_NAME: Xs, V_NAME: Vs, "Δt": dts[None], "t": times[None], "u": u0, "du": du, "ddu": ddu},
                              controls=("ddu", "Δt"), timestep="Δt")  # fmt: skip
    B = pa.VariationalUnitaryIntegrator(system, traj, X_NAME, [V_NAME], "u", pade_order="exp", exp_hessian=newton)
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
                a = k * traj.dim + comp["Δt"].start
                b = k * traj.dim + r.dx_off + np.arange(r.x_dim)
                ii += [np.full(r.x_dim, a), b]
                jj += [b, np.full(r.x_dim, a)]
                vv += [-mu[k], -mu[k]]
        return H + sp.csr_matrix((np.concatenate(vv), (np.concatenate(ii), np.concatenate(jj))), shape=(nv, nv))

    sens = pa.UnitarySensitivityObjective(V_NAME, traj, [traj.N], Qs=[Qs])
    J = pa.UnitaryInfidelityObjective(U_goal, X_NAME, traj, Q=Q) + sens
    for c_ in ("u", "du", "ddu"):
        J = J + pa.QuadraticRegularizer(c_, traj, R, dt_power=0)
    J.bind(B)

    def obj(z):
        return J.value_and_gradient(z)

    hr, hc = J.hessian_structure()

    def obj_hess(z):
        L = sp.csr_matrix((J.hessian(z, 1.0), (hr, hc)), shape=(nv, nv))
        return L + sp.tril(L, -1).T

    def sensitivity(z):  # |tr(U_var' U_var)|^2 / d^2 of the terminal knot, unweighted
        x = np.asarray(z).reshape(N, traj.dim)[-1, comp[V_NAME].start : comp[V_NAME].stop]
        return float((x @ x) ** 2 / d**2)

    if callbacks_only:
        return dict(z0=traj.datavec.copy(), obj=obj, obj_hess=obj_hess, cons=cons, cons_jac=cons_jac, cons_hess=cons_hess, n_rows=int(offs[-1]), close=B.close)
    lb, ub = np.full(nv, -np.inf), np.full(nv, np.inf)
    for k in range(N):
        o = k * traj.dim
        lb[o + comp[X_NAME].start : o + comp[X_NAME].stop], ub[o + comp[X_NAME].start : o + comp[X_NAME].stop] = -1.0, 1.0
        lb[o + comp["u"].start : o + comp["u"].stop], ub[o + comp["u"].start : o + comp["u"].stop] = -0.1, 0.1
        lb[o + comp["Δt"].start] = ub[o + comp["Δt"].start] = traj.datavec[o + comp["Δt"].start]  # timesteps_all_equal
    z0 = traj.datavec.copy()
    for nm in (X_NAME, V_NAME):  # initial condition
        s = slice(comp[nm].start, comp[nm].stop)
        lb[s] = ub[s] = z0[s]
    for k in (0, N - 1):  # u(0) = u(T) = 0
        s = slice(k * traj.dim + comp["u"].start, k * traj.dim + comp["u"].stop)
        lb[s] = ub[s] = 0.0
    z0 = np.clip(z0, lb, ub)
    nc_rows = int(offs[-1])
    J0, s0 = float(obj(z0)[0]), sensitivity(z0)
    res = minimize(obj, z0, jac=True, method="trust-constr", hess=obj_hess if exact_hessian else BFGS(), bounds=Bounds(lb, ub, keep_feasible=False),
                   constraints=[NonlinearConstraint(cons, np.zeros(nc_rows), np.zeros(nc_rows), jac=cons_jac, hess=cons_hess if newton else BFGS())],
                   options=dict(maxiter=max_iter, gtol=1e-8, xtol=1e-12, verbose=verbose, sparse_jacobian=True))  # fmt: skip
    traj.update(res.x)
    viol = float(np.abs(cons(res.x)).max())
    J1, s1 = float(obj(res.x)[0]), sensitivity(res.x)
    fid = 1.0 - pa.Objective([pa.UnitaryInfidelityObjective(U_goal, X_NAME, traj, Q=1.0)]).bind(B).value_and_gradient(res.x, want_grad=False)[0]
    B.close()
    return dict(fidelity=float(fid), max_violation=viol, iterations=int(res.nit), objective_initial=J0, objective_final=J1, sensitivity_initial=s0,
                sensitivity_final=s1, n_vars=nv, n_rows=nc_rows, newton=bool(newton))  # fmt: skip


if __name__ == "__main__":
    a = solve(verbose=1, newton=True)
    b = solve(verbose=1, newton=False)
    print(a)
    print(b)
    print("iterations: exact constraint Hessian %d (fidelity %.6f, violation %.2e) | quasi-Newton %d (fidelity %.6f, violation %.2e)"
          % (a["iterations"], a["fidelity"], a["max_violation"], b["iterations"], b["fidelity"], b["max_violation"]))  # fmt: skip
