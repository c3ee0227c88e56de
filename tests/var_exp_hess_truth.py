"""Truth of the Hessian of the Lagrangian of the variational integrators on the exponential constraint (option ``var_exp_hess`` on a
PCL_BATCH_VARIATIONAL_EXP context), by LIFTING: per state column the stack [X; Xv_1; ..; Xv_v] is one vector of the lifted generator
var_G(G, [Gv_i]), so ``exp_hess_truth.interval_values`` of the lifted system (block ``expm`` for the second Frechet derivative,
``expm_frechet`` for the first) gives every value.  The state slices come back from the lifted order (column c, component b, row i) to the
stacked, component-major order through the row map of ``variational_truth``.  Nothing here shares a path with the kernel's recurrence, nor
with its adjoint formulas.

The layout is the first five segments of the Pade variational one (nothing involves X'_{k+1}):

    (u_i, u_j), j <= i | (dt, u_j) | (dt, dt) | (u_l, X'_k[q]) l = 0 .. m-1 | (dt, X'_k[q])         q over the stacked state

Importable without a GPU."""
import numpy as np

import exp_hess_truth as eht
import variational_truth as vt


def nnz_per_interval(case):
    return (case.m + 1) * (case.m + 2) // 2 + case.xd * (case.m + 1)


def values(case, mu):
    """[K, nnz_per_interval]; mu in stacked order, [K * x_dim'] like delta."""
    Zl, lay, G0l, Gjl = vt.lifted(case)
    rm = vt._row_map(case)
    mul = np.asarray(mu, dtype=np.float64).reshape(case.K, case.xd)[:, rm]
    vl = eht.values(Zl, mul, lay, G0l, Gjl)
    nsc = (case.m + 1) * (case.m + 2) // 2
    out = vl.copy()
    S = vl[:, nsc:].reshape(case.K, case.m + 1, case.xd)
    O = np.empty_like(S)
    O[:, :, rm] = S
    out[:, nsc:] = O.reshape(case.K, -1)
    return out


def structure(case, index_base=0):
    """(rows, cols) of the K intervals in value order, lower triangle (rows >= cols)."""
    m, xd, xdc, zd = case.m, case.xd, case.xdc, case.z_dim
    q = np.arange(xd)
    xq = np.array(case.xo)[q // xdc] + q % xdc
    rows, cols = [], []
    for k in range(case.K):
        uk, hk = k * zd + case.u_off, k * zd + case.dt_off
        a, b = [], []
        for i in range(m):
            for j in range(i + 1):
                a.append(uk + i), b.append(uk + j)
        for j in range(m):
            a.append(hk), b.append(uk + j)
        a.append(hk), b.append(hk)
        a, b = [np.array(a, dtype=np.int64)], [np.array(b, dtype=np.int64)]
        for l in range(m):
            a.append(np.full(xd, uk + l)), b.append(k * zd + xq)
        a.append(np.full(xd, hk)), b.append(k * zd + xq)
        a, b = np.concatenate(a), np.concatenate(b)
        rows.append(np.maximum(a, b)), cols.append(np.minimum(a, b))
    return np.concatenate(rows).astype(np.int64) + index_base, np.concatenate(cols).astype(np.int64) + index_base


def dense(vals, case):
    """Symmetric (z_dim N) square matrix from the triplets (small cases)."""
    r, c = structure(case)
    nv = case.z_dim * case.N
    H = np.zeros((nv, nv))
    np.add.at(H, (r, c), np.asarray(vals).reshape(-1))
    return H + np.tril(H, -1).T
