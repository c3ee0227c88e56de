"""Truth for the variational integrators, built from the oracle by LIFTING: per state column the stacked state [X; Xv_1; ...; Xv_v] is one
vector of the lifted generator var_G(G, [Gv_i]) ((1 + v) n x (1 + v) n), so the oracle's Pade residual, Jacobian and Hessian on a permuted copy
of the trajectory (Layout(gen=(1 + v) n, cols=C)) give every value.  The permutation maps the lifted order (column c, component b, row i) back to
the stacked order (component b, column c, row i) of the reference's vcat."""
import dataclasses

import numpy as np
import scipy.sparse as sp

from oracle import pade_oracle as po


@dataclasses.dataclass
class VarCase:
    Z: np.ndarray  # [N, z_dim]
    z_dim: int
    N: int
    n: int
    C: int
    m: int
    xo: list  # offsets of the 1 + v components
    u_off: int
    dt_off: int
    G0: np.ndarray
    Gv: list
    Gj: np.ndarray

    @property
    def v(self):
        return len(self.Gv)

    @property
    def xdc(self):
        return self.n * self.C

    @property
    def xd(self):
        return self.xdc * (self.v + 1)

    @property
    def K(self):
        return self.N - 1


def lifted(case: VarCase):
    """(Zl, layout, G0', Gj') of the lifted problem: knot = [lifted state (C x n') | dt | u]."""
    n, C, v, m = case.n, case.C, case.v, case.m
    nl = (v + 1) * n
    zl = C * nl + 1 + m
    lay = po.Layout(d=n // 2, m=m, N=case.N, z_dim=zl, x_off=0, u_off=C * nl + 1, dt_off=C * nl, cols=C, gen=nl)
    Zl = np.zeros((case.N, zl))
    for k in range(case.N):
        X = np.stack([case.Z[k, o : o + case.xdc].reshape(C, n) for o in case.xo], axis=1)  # [C, 1+v, n]
        Zl[k, : C * nl] = X.reshape(-1)
        Zl[k, lay.dt_off] = case.Z[k, case.dt_off]
        Zl[k, lay.u_off : lay.u_off + m] = case.Z[k, case.u_off : case.u_off + m]
    G0l = po.var_G(case.G0, list(case.Gv))
    Gjl = np.array([np.kron(np.eye(v + 1), g) for g in case.Gj]).reshape(m, nl, nl) if m else np.zeros((0, nl, nl))
    return Zl, lay, G0l, Gjl


def _row_map(case):
    """lifted row (within an interval) -> stacked row"""
    n, C, v = case.n, case.C, case.v
    c, b, i = np.meshgrid(np.arange(C), np.arange(v + 1), np.arange(n), indexing="ij")
    return (b * case.xdc + c * n + i).reshape(-1)


def _col_map(case, lay):
    """lifted variable index -> variable index of the case's trajectory"""
    n, C, v = case.n, case.C, case.v
    zl = lay.z_dim
    out = np.empty(case.N * zl, dtype=np.int64)
    c, b, i = np.meshgrid(np.arange(C), np.arange(v + 1), np.arange(n), indexing="ij")
    st = (np.array(case.xo)[b] + c * n + i).reshape(-1)
    for k in range(case.N):
        out[k * zl : k * zl + C * (v + 1) * n] = k * case.z_dim + st
        out[k * zl + lay.dt_off] = k * case.z_dim + case.dt_off
        out[k * zl + lay.u_off : k * zl + lay.u_off + case.m] = k * case.z_dim + case.u_off + np.arange(case.m)
    return out


def residual(case, order):
    """delta in stacked order, [K * x_dim']"""
    Zl, lay, G0l, Gjl = lifted(case)
    R = po.pade_residual(Zl, lay, G0l, Gjl, order)  # [K, C n']
    out = np.empty_like(R)
    out[:, _row_map(case)] = R
    return out.reshape(-1)


def jacobian(case, order):
    """scipy CSR of the Jacobian (K x_dim' rows, N z_dim columns) and the set of its structural positions (row * ncols + col)."""
    Zl, lay, G0l, Gjl = lifted(case)
    vals = po.pade_jacobian_values(Zl, lay, G0l, Gjl, order).reshape(-1)
    rows, cols = po.jac_structure(lay)
    rm, cm = _row_map(case), _col_map(case, lay)
    xd = case.xd
    r = (rows // xd) * xd + rm[rows % xd]
    c = cm[cols]
    shape = (case.K * xd, case.N * case.z_dim)
    return sp.csr_matrix((vals, (r, c)), shape=shape), r.astype(np.int64) * shape[1] + c


def hessian(case, order, mu):
    """scipy CSR (lower triangle, as emitted) of grad^2 mu' delta; mu in stacked order [K * x_dim']."""
    Zl, lay, G0l, Gjl = lifted(case)
    rm = _row_map(case)
    mul = mu.reshape(case.K, case.xd)[:, rm]
    vals = po.pade_hessian_values(Zl, mul, lay, G0l, Gjl, order).reshape(-1)
    rows, cols = po.hess_structure(lay)
    cm = _col_map(case, lay)
    a, b = cm[rows], cm[cols]
    nv = case.N * case.z_dim
    return sp.csr_matrix((vals, (np.maximum(a, b), np.minimum(a, b))), shape=(nv, nv)), np.maximum(a, b) * nv + np.minimum(a, b)


def literal_residual(case, order):
    """The reference's literal construction: Pade residual of var_G(I_C (x) G(u), [I_C (x) Gv_i]) on vcat(x, x_var_1, ...)
    (src/control/integrators.jl:247-264 with isomorphisms.jl:398-422)."""
    c = po.pade_coeffs(order)
    q = order // 2
    IC = np.eye(case.C)
    out = np.empty((case.K, case.xd))
    for k in range(case.K):
        u = case.Z[k, case.u_off : case.u_off + case.m]
        G = case.G0 + np.tensordot(u, case.Gj, axes=1) if case.m else case.G0
        Gh = po.var_G(np.kron(IC, G), [np.kron(IC, g) for g in case.Gv])
        h = case.Z[k, case.dt_off]
        s0 = np.concatenate([case.Z[k, o : o + case.xdc] for o in case.xo])
        s1 = np.concatenate([case.Z[k + 1, o : o + case.xdc] for o in case.xo])
        P = np.eye(Gh.shape[0])
        r = np.zeros(case.xd)
        for j in range(q + 1):
            r += c[j] * h**j * (P @ ((-1) ** j * s1 - s0))
            P = P @ Gh
        out[k] = r
    return out.reshape(-1)


def h_var_drift(levels_per, n_sub):
    """2 pi sum_q a_q^dag a_q: the drift-frequency direction (the direction config 4 samples)."""
    a = po.annihilate(levels_per)
    num = a.conj().T @ a
    H = 0
    for qb in range(n_sub):
        H = H + po.lift_operator(num, qb + 1, [levels_per] * n_sub)
    return 2 * np.pi * H


def make_case(sys_o, Gv, N, seed, ket=False, dt=0.1, u_scale=0.02, noise=1e-3, extra=0, xo=None, u_off=None, dt_off=None, t_off=None,
              z_dim=None):
    """A trajectory [X | Xv_1 .. Xv_v | dt | t | u | (extra zeros)] near the exact propagation of the lifted system (so delta is small
    but not zero).  Any other knot: the offsets of the 1 + v components (xo), of the controls, of dt and of t, and z_dim, all given;
    m = 0 (drift only) too."""
    import scipy.linalg

    rng = np.random.default_rng(seed)
    d, m = sys_o.levels, sys_o.n_drives
    n, C = 2 * d, (1 if ket else d)
    v = len(Gv)
    xdc = n * C
    if xo is None:
        xo = [b * xdc for b in range(v + 1)]
        dt_off = (v + 1) * xdc
        t_off = dt_off + 1
        u_off = dt_off + 2
        z_dim = u_off + m + extra
    assert len(xo) == v + 1 and None not in (u_off, dt_off, z_dim)
    Z = np.zeros((N, z_dim))
    u = np.clip(u_scale * rng.standard_normal((N, m)), -0.1, 0.1)
    Z[:, dt_off] = dt * (1 + 0.1 * rng.random(N))
    if t_off is not None:
        Z[:, t_off] = np.cumsum(Z[:, dt_off])
    Z[:, u_off : u_off + m] = u
    G0, Gj = np.asarray(sys_o.G_drift), np.array(sys_o.G_drives).reshape(m, n, n)
    xo = list(xo)
    X0 = np.vstack([np.eye(d), np.zeros((d, d))])[:, :C]
    S = np.concatenate([X0] + [0.01 * rng.standard_normal((n, C)) for _ in range(v)], axis=0)  # [n', C]
    for k in range(N):
        for b in range(v + 1):
            Z[k, xo[b] : xo[b] + xdc] = S[b * n : (b + 1) * n].T.reshape(-1)
        if k + 1 < N:
            Gh = po.var_G(G0 + np.tensordot(u[k], Gj, axes=1), list(Gv))
            S = scipy.linalg.expm(Z[k, dt_off] * Gh) @ S + noise * rng.standard_normal(S.shape)
    return VarCase(Z=Z, z_dim=z_dim, N=N, n=n, C=C, m=m, xo=xo, u_off=u_off, dt_off=dt_off, G0=G0, Gv=[np.asarray(g) for g in Gv], Gj=Gj)
