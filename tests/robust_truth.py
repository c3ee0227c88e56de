"""Truth for the robust-control objective and the rollout of a variational context.

The sensitivity loss restates the reference's three lines (src/control/objectives.jl:437-453)

    U = iso_vec_to_operator(x);  loss = scale^4 * abs2(tr(U'U)) / n^2,   n = size(U, 1)

in numpy; its gradient and Hessian are the closed forms of that quartic.  The rollout is the oracle's exact rollout of the LIFTED system
(tests/variational_truth.py) mapped back to the stacked order with that helper's row map."""
import numpy as np
import scipy.sparse as sp

from oracle import pade_oracle as po
from variational_truth import _row_map, lifted


# ---- the sensitivity term -----------------------------------------------------------------------------------------------------------------
def sens_loss(x, w=1.0):
    """w |tr(U'U)|^2 / n^2 for the iso-vec x of U (w = Qs * scale^4)."""
    U = po.iso_vec_to_operator(np.asarray(x, dtype=float))
    return w * abs(np.trace(U.conj().T @ U)) ** 2 / U.shape[0] ** 2


def sens_grad(x, w=1.0):
    """tr(U'U) = |x|^2, so the loss is w (x'x)^2 / d^2 and its gradient 4 w (x'x) x / d^2."""
    x = np.asarray(x, dtype=float)
    d = int(round(np.sqrt(x.size / 2)))
    return 4.0 * w * (x @ x) * x / d**2


def sens_hess(x, w=1.0):
    x = np.asarray(x, dtype=float)
    d = int(round(np.sqrt(x.size / 2)))
    return w * (4.0 * (x @ x) * np.eye(x.size) + 8.0 * np.outer(x, x)) / d**2


# ---- the whole objective of a case ----------------------------------------------------------------------------------------------------------
def infidelity_terms(x, goal, Q, subspace=None):
    """(value, gradient, Hessian) of Q |1 - F(x)| for a unitary goal; the Hessian from the values of F, which is quadratic."""
    val = po.unitary_infidelity(x, goal, Q, subspace)
    g = po.unitary_infidelity_gradient(x, goal, Q, subspace)
    F = po.unitary_fidelity_loss(x, goal, subspace)
    sgn = 1.0 if 1.0 - F >= 0 else -1.0
    return val, g, -sgn * Q * fidelity_hessian(x.size, goal, subspace)


def fidelity_hessian(L, goal, subspace=None):
    """Hessian of F, which is quadratic in x.  Full-space goal: F = |tr(G'U)|^2 / d^2 = (a'x)^2 + (b'x)^2 with a = iso_vec(G) / d and
    b = iso_vec(iG) / d, so the Hessian is 2 (aa' + bb').  Embedded goal: from the values of F (small systems only)."""
    if subspace is not None:
        return po.quadratic_hessian(lambda y: po.unitary_fidelity_loss(y, goal, subspace), L)
    G = np.asarray(goal, dtype=complex)
    a, b = po.operator_to_iso_vec(G) / G.shape[0], po.operator_to_iso_vec(1j * G) / G.shape[0]
    return 2.0 * (np.outer(a, a) + np.outer(b, b))


def objective(case, Z, w, Q, goal=None, subspace=None, regs=(), want_hess=False):
    """J = Q w0 |1 - F(X_N)| + sum_i w_i sens(Xv_i,N) + regularisers (regs: (off, dim, R, dt_power)); returns (value, gradient [N, z_dim]) and,
    on request, the symmetric Hessian over the N z_dim variables (scipy CSR)."""
    Z = np.asarray(Z, dtype=float).reshape(case.N, case.z_dim)
    nv = Z.size
    val, g = 0.0, np.zeros_like(Z)
    blocks = []  # (rows, cols, values) of the Hessian, summed at the end

    def add(r, c, v):
        blocks.append((np.asarray(r).reshape(-1), np.asarray(c).reshape(-1), np.asarray(v, dtype=float).reshape(-1)))

    def add_dense(s0, M):
        i, j = np.meshgrid(np.arange(M.shape[0]), np.arange(M.shape[1]), indexing="ij")
        add(s0 + i, s0 + j, M)

    t0 = (case.N - 1) * case.z_dim
    if goal is not None:
        x = Z[-1, case.xo[0] : case.xo[0] + case.xdc]
        if want_hess:
            v0, g0, H0 = infidelity_terms(x, goal, Q, subspace)
            add_dense(t0 + case.xo[0], w[0] * H0)
        else:
            v0, g0 = po.unitary_infidelity(x, goal, Q, subspace), po.unitary_infidelity_gradient(x, goal, Q, subspace)
        val += w[0] * v0
        g[-1, case.xo[0] : case.xo[0] + case.xdc] += w[0] * g0
    for i in range(1, case.v + 1):
        if w[i] == 0:
            continue
        x = Z[-1, case.xo[i] : case.xo[i] + case.xdc]
        val += sens_loss(x, w[i])
        g[-1, case.xo[i] : case.xo[i] + case.xdc] += sens_grad(x, w[i])
        if want_hess:
            add_dense(t0 + case.xo[i], sens_hess(x, w[i]))
    for off, dim, R, pw in regs:
        val += po.quadratic_regularizer(Z, off, dim, R, case.dt_off, pw)
        g += po.quadratic_regularizer_gradient(Z, off, dim, R, case.dt_off, pw)
        if want_hess:
            Rv = np.broadcast_to(np.asarray(R, dtype=float), (dim,))
            for k in range(case.N):
                z0, h = k * case.z_dim, Z[k, case.dt_off]
                v = Z[k, off : off + dim]
                idx = z0 + off + np.arange(dim)
                hh = np.full(dim, z0 + case.dt_off)
                add(idx, idx, (h**pw if pw else 1.0) * Rv)
                if pw >= 1:
                    c = (1.0 if pw == 1 else 2.0 * h) * Rv * v
                    add(hh, idx, c)
                    add(idx, hh, c)
                if pw == 2:
                    add(hh[:1], hh[:1], [Rv @ (v * v)])
    if not want_hess:
        return val, g
    r, c, v = (np.concatenate(q) for q in zip(*blocks)) if blocks else (np.zeros(0, int), np.zeros(0, int), np.zeros(0))
    return val, g, sp.coo_matrix((v, (r, c)), shape=(nv, nv)).tocsr()


# ---- rollout ----------------------------------------------------------------------------------------------------------------------------
def lifted_rollout(case):
    """[N, x_dim'] stacked states: the oracle's exact rollout of the lifted system, rows mapped back to (component, column, row)."""
    X = po.exact_rollout(*lifted(case))
    out = np.empty_like(X)
    out[:, _row_map(case)] = X
    return out


def plain_layout(case):
    """Layout and trajectory [X | dt | u] of the case's nominal system alone (component 0)."""
    zl = case.xdc + 1 + case.m
    lay = po.Layout(d=case.n // 2, m=case.m, N=case.N, z_dim=zl, x_off=0, u_off=case.xdc + 1, dt_off=case.xdc, cols=case.C, gen=case.n)
    Zp = np.zeros((case.N, zl))
    Zp[:, : case.xdc] = case.Z[:, case.xo[0] : case.xo[0] + case.xdc]
    Zp[:, lay.dt_off] = case.Z[:, case.dt_off]
    Zp[:, lay.u_off : lay.u_off + case.m] = case.Z[:, case.u_off : case.u_off + case.m]
    return lay, Zp


def fd_sensitivity_rollout(case, i=1, eps=1e-4):
    """Central difference of two PLAIN exact rollouts with drift G0 +- eps Gv_i: the rolled-out Xv_i when Xv_i = 0 at knot 0, up to O(eps^2)."""
    lay, Zp = plain_layout(case)
    Xp = po.exact_rollout(Zp, lay, case.G0 + eps * case.Gv[i - 1], case.Gj)
    Xm = po.exact_rollout(Zp, lay, case.G0 - eps * case.Gv[i - 1], case.Gj)
    return (Xp - Xm) / (2 * eps)


# ---- a bare context of a case (every shape, no named trajectory) ----------------------------------------------------------------------------
def var_context(pa, case, order=4, index_base=0):
    d = case.n // 2
    return pa.integrators._PclContext(d=d, m=case.m, N=case.N, z_dim=case.z_dim, u_off=case.u_off, dt_off=case.dt_off, x_offs=case.xo,
                                      G0=np.concatenate([case.G0[None], np.array(case.Gv)]), Gj=np.asarray(case.Gj).reshape(case.m, case.n, case.n),
                                      batch=1 + case.v, batch_mode=pa._lib.PCL_BATCH_VARIATIONAL, per_member_G0=True, index_base=index_base,
                                      pade_order=order, state_cols=1 if case.C == 1 else d)  # fmt: skip


def plain_context(pa, case, order=4):
    """The nominal system alone on the case's own knots: a plain context reading component 0."""
    d = case.n // 2
    return pa.integrators._PclContext(d=d, m=case.m, N=case.N, z_dim=case.z_dim, u_off=case.u_off, dt_off=case.dt_off, x_offs=[case.xo[0]],
                                      G0=case.G0, Gj=np.asarray(case.Gj).reshape(case.m, case.n, case.n), batch=1,
                                      batch_mode=pa._lib.PCL_BATCH_MEMBERS, pade_order=order, state_cols=1 if case.C == 1 else d)  # fmt: skip
