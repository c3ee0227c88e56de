#!/usr/bin/env python3
"""A robust single-qubit gate driven through a CPU NLP solver with every callback on the GPU: the system of the reference's variational test
item (H_drift = Z/2, drives X and Y, H_var = Z/2: the sensitivity to the qubit frequency), a VariationalUnitaryIntegrator carrying
U and dU/d(eps), and the objective UnitaryInfidelityObjective + UnitarySensitivityObjective(terminal knot) + regularisers
[REF src/control/objectives.jl:437-453, src/specs/materialize.jl:306-307].  The shape of scripts/plumbing_xgate.py: scipy's trust-constr
stands in for Ipopt; constraints = [variational dynamics, DerivativeIntegrator(u, du), DerivativeIntegrator(du, ddu), time consistency]."""
import os
import sys

import numpy as np
import scipy.linalg
import scipy.sparse as sp
from scipy.optimize import BFGS, Bounds, NonlinearConstraint, minimize

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import piccolo_jl_amd as pa

X_NAME, V_NAME = "Ũ⃗", "Ũ⃗_var"


def solve(N=30, T=10.0, Q=100.0, Qs=1e-2, R=1e-2, seed=0, max_iter=300, verbose=0):
    Z2 = 0.5 * pa.PAULIS["Z"]
    system = pa.VariationalQuantumSystem(Z2, [pa.PAULIS["X"], pa.PAULIS["Y"]], [Z2], [1.0, 1.0])
    U_goal = pa.GATES["X"]
    rng = np.random.default_rng(seed)
    times = np.linspace(0, T, N)
    dts = np.full(N, times[1] - times[0])
    u0 = 0.1 * rng.standard_normal((2, N))
    u0[:, 0] = u0[:, -1] = 0.0
    # initial states: exact propagation of [U; U_var] under the lifted generator, U_var(0) = 0
    n = 4
    Gv = system.G_vars_array()[0]
    S = np.vstack([np.vstack([np.eye(2), np.zeros((2, 2))]), np.zeros((n, 2))])
    Xs, Vs = np.zeros((2 * n, N)), np.zeros((2 * n, N))
    for k in range(N):
        Xs[:, k], Vs[:, k] = S[:n].T.reshape(-1), S[n:].T.reshape(-1)
        G = system.G_drift + np.tensordot(u0[:, k], system.G_drives_array(), axes=1)
        S = scipy.linalg.expm(dts[k] * np.block([[G, np.zeros((n, n))], [Gv, G]])) @ S
    du = np.zeros((2, N))
    du[:, :-1] = np.diff(u0, axis=1) / dts[:-1]
    ddu = np.zeros((2, N))
    ddu[:, :-1] = np.diff(du, axis=1) / dts[:-1]
    traj = pa.NamedTrajectory({X_NAME: Xs, V_NAME: Vs, "Δt": dts[None], "t": times[None], "u": u0, "du": du, "ddu": ddu},
                              controls=("ddu", "Δt"), timestep="Δt")  # fmt: skip
    B = pa.VariationalUnitaryIntegrator(system, traj, X_NAME, [V_NAME], "u", pade_order=4)
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
        return float((x @ x) ** 2 / 4)

    lb, ub = np.full(nv, -np.inf), np.full(nv, np.inf)
    for k in range(N):
        o = k * traj.dim
        lb[o + comp[X_NAME].start : o + comp[X_NAME].stop], ub[o + comp[X_NAME].start : o + comp[X_NAME].stop] = -1.0, 1.0
        lb[o + comp["u"].start : o + comp["u"].stop], ub[o + comp["u"].start : o + comp["u"].stop] = -1.0, 1.0
        lb[o + comp["ddu"].start : o + comp["ddu"].stop], ub[o + comp["ddu"].start : o + comp["ddu"].stop] = -2.0, 2.0
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
    dims = dict(n_vars=nv, n_rows=nc_rows, obj_grad=int(obj(z0)[1].size), cons=int(cons(z0).size), cons_jac=tuple(cons_jac(z0).shape),
                cons_hess=tuple(cons_hess(z0, np.ones(nc_rows)).shape), obj_hess=tuple(obj_hess(z0).shape))  # fmt: skip
    J0, s0 = float(obj(z0)[0]), sensitivity(z0)
    res = minimize(obj, z0, jac=True, method="trust-constr", hess=BFGS(), bounds=Bounds(lb, ub, keep_feasible=False),
                   constraints=[NonlinearConstraint(cons, np.zeros(nc_rows), np.zeros(nc_rows), jac=cons_jac, hess=cons_hess)],
                   options=dict(maxiter=max_iter, gtol=1e-8, xtol=1e-12, verbose=verbose, sparse_jacobian=True))  # fmt: skip
    traj.update(res.x)
    viol = np.abs(cons(res.x)).max()
    J1, s1 = float(obj(res.x)[0]), sensitivity(res.x)
    rollout = pa.variational_rollout(B, traj)  # (switches nothing off: the objective stays bound)
    fid = 1.0 - pa.Objective([pa.UnitaryInfidelityObjective(U_goal, X_NAME, traj, Q=1.0)]).bind(B).value_and_gradient(res.x, want_grad=False)[0]
    B.close()
    return dict(fidelity=float(fid), max_violation=float(viol), iterations=int(res.nit), objective_initial=J0, objective_final=J1,
                sensitivity_initial=s0, sensitivity_final=s1, rollout=rollout, traj=traj, system=system, dims=dims)  # fmt: skip


if __name__ == "__main__":
    r = solve(verbose=1)
    print({k: v for k, v in r.items() if k not in ("traj", "rollout", "system")})
