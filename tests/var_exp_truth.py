"""Truth of the variational integrators on the exponential constraint (batch_mode PCL_BATCH_VARIATIONAL_EXP), by LIFTING: per state column the
stack [X; Xv_1; ..; Xv_v] is one vector of the lifted generator var_G(G, [Gv_i]) ((1 + v) n square), so the oracle's exponential residual
(``po.exp_residual``) and Jacobian (``exp_truth``: scipy ``expm`` / ``expm_frechet``) of the lifted problem give every value.  Rows and columns
go back through the maps of ``variational_truth``; the values are then gathered at the structure the library documents:

    -E (component 0, C copies) | per variation i: -E w.r.t. Xv_i,k, -L_i w.r.t. X_k | +1 for r < x_dim' (knot k+1) |
    tails, component-major, per state column: m drive slices of n, then the dt slice

Nothing here shares code with the kernel's recurrence.  The lifted Jacobian is kept sparse (config 3 would be 0.8 GB dense).
Importable without a GPU."""
import contextlib

import numpy as np
import scipy.linalg
import scipy.sparse as sp

import exp_truth
import variational_truth as vt
from oracle import pade_oracle as po


def nnz_per_interval(case):
    return (1 + 2 * case.v) * case.C * case.n**2 + case.xd * (case.m + 2)


def structure(case, index_base=0):
    """(rows, cols) of the K intervals in value order."""
    n, C, v, m, xdc, xd, zd = case.n, case.C, case.v, case.m, case.xdc, case.xd, case.z_dim
    c_, j_, i_ = np.meshgrid(np.arange(C), np.arange(n), np.arange(n), indexing="ij")
    br, bc = (c_ * n + i_).reshape(-1), (c_ * n + j_).reshape(-1)
    c_, l_, i_ = np.meshgrid(np.arange(C), np.arange(m + 1), np.arange(n), indexing="ij")
    tr = (c_ * n + i_).reshape(-1)
    tc = np.where(l_ < m, case.u_off + l_, case.dt_off).reshape(-1)
    q = np.arange(xd)
    ones_c = np.array(case.xo)[q // xdc] + q % xdc
    rows, cols = [], []
    for k in range(case.K):
        r0, c0 = k * xd, k * zd
        rows.append(r0 + br)
        cols.append(c0 + case.xo[0] + bc)
        for b in range(1, v + 1):
            rows += [r0 + b * xdc + br, r0 + b * xdc + br]
            cols += [c0 + case.xo[b] + bc, c0 + case.xo[0] + bc]
        rows.append(r0 + q)
        cols.append(c0 + zd + ones_c)
        for b in range(v + 1):
            rows.append(r0 + b * xdc + tr)
            cols.append(c0 + tc)
    rows, cols = np.concatenate(rows).astype(np.int64), np.concatenate(cols).astype(np.int64)
    return rows + index_base, cols + index_base


def residual(case):
    """delta in stacked order, [K * x_dim']"""
    Zl, lay, G0l, Gjl = vt.lifted(case)
    R = po.exp_residual(Zl, lay, G0l, Gjl)  # [K, C n']
    out = np.empty_like(R)
    out[:, vt._row_map(case)] = R
    return out.reshape(-1)


def jacobian(case):
    """scipy CSR of the Jacobian (K x_dim' rows, N z_dim columns), every position of the lifted problem's triplets."""
    Zl, lay, G0l, Gjl = vt.lifted(case)
    vals = exp_truth.values(Zl, lay, G0l, Gjl).reshape(-1)
    rows, cols = exp_truth.structure(lay)
    rm, cm = vt._row_map(case), vt._col_map(case, lay)
    xd = case.xd
    r = (rows // xd) * xd + rm[rows % xd]
    return sp.csr_matrix((vals, (r, cm[cols])), shape=(case.K * xd, case.N * case.z_dim))


def values(case, J=None):
    """[K * nnz_per_interval]: the truth at the library's structure.  What the lifted problem has outside it (the blocks of exp(h Ghat) above the
    diagonal and between variations) must vanish."""
    J = jacobian(case) if J is None else J
    r, c = structure(case)
    out = np.asarray(J[r, c]).reshape(-1)
    assert abs(np.abs(J).sum() - np.abs(out).sum()) <= 1e-12 * max(1.0, np.abs(out).sum())
    return out


@contextlib.contextmanager
def cached_expm():
    """Inside: scipy.linalg.expm remembers its results by argument -- a central difference in a state variable asks for the same propagator
    again and again."""
    real, memo = scipy.linalg.expm, {}

    def expm(A):
        key = np.ascontiguousarray(A).tobytes()
        if key not in memo:
            if len(memo) > 64:
                memo.clear()
            memo[key] = real(A)
        return memo[key]

    scipy.linalg.expm = expm
    try:
        yield
    finally:
        scipy.linalg.expm = real
