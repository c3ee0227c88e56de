"""Cases for the Hessian of the Lagrangian on large variational contexts (PCL_BATCH_VARIATIONAL | PCL_LARGE_N | PCL_LARGE_VAR with option
large_var_hess; piccolo.jl_amd/csrc/pcl_kernel_var_large_hess.hpp, planned by var_large_hess_plan in pcl_host_launch_hess.hpp, restated below);
numpy only, importable without a GPU.

Cases: VL1 .. VL6 of tests/var_large_cases.py (systems, knots, steps and seeds are that module's) and
    VH1  128 ket  v = 2  m = 24   the tightest LDS of the Hessian launch: one column and one drive per unit (28 blocks beside the tile,
                                  162,480 B), 24 groups of one drive; dense Hermitian generators, seed 16000 + 17 * 8, steps as the others
                                  (h |Ghat|_2 = 0.15, -0.3, and the long step 0.8: the smallest of LONG_STEPS that shows c_5 at 1e-7)
What var_large_hess_plan gives per case (sx slices of nc state columns x ngrp groups of mg drives, U workgroups per interval, LDS bytes) is
TABLE; tests/test_var_large_hess_cpu.py asserts it against the restatement.

Multipliers: default_rng(seed of the case + 77).standard_normal(K x_dim'), in the stacked order of the rows.

The truth is vector_shape_cases.truth_values(..., hessian=True) (np.longdouble) on the lifted problem of variational_truth.lifted, brought to
the library's value order by value_index -- within every vector segment the lifted order (column, component, row) against the stacked order
(component, column, row) -- which tests/test_var_large_hess_cpu.py checks position by position against oracle/pade_oracle.hess_structure
through variational_truth._col_map.  Segments are variational_shape_cases.hess_codes (variable kinds x relative knot x interval).

pass_values restates the kernel's formulation in float64 numpy: the chains of DESIGN 4.18 on the lifted generator without a lifted matrix, one
pass per component (pass 0: the plain Hessian of (M_0, X_0); pass b: the two-component problem (X_0, X_b) with the multipliers (0, M_b))."""
import functools

import numpy as np

import var_large_cases as vl
import variational_shape_cases as vsc
import variational_truth as vt
import vector_shape_cases as vs
from oracle import pade_oracle as po

LDS_BYTES = vl.LDS_BYTES
ORDERS = vs.ORDERS
SEEN = vs.SEEN
SLACK = vl.SLACK
LD_ = np.longdouble

VH1 = (64, True, 2, 24)
VH1_SEED, VH1_LONG = 16000 + 17 * 8, 0.8
NAMES = vl.NAMES + ["VH1"]
# what var_large_hess_plan gives on 163,840 B: (sx, nc, ngrp, mg, U, bytes)
TABLE = {
    "VL1": (1, 1, 1, 2, 1, 55832), "VL2": (5, 7, 3, 1, 15, 141824), "VL3": (12, 4, 4, 1, 48, 162720), "VL4": (1, 1, 1, 1, 1, 162112),
    "VL5": (1, 1, 8, 3, 8, 160640), "VL6": (1, 1, 1, 0, 1, 54824), "VH1": (1, 1, 24, 1, 24, 162480),
}  # fmt: skip


def shape(name):
    """(n, C, v, m)"""
    d, ket, v, m = VH1 if name == "VH1" else vl.CASES[name]
    return 2 * d, (1 if ket else d), v, m


# ---- the launch code's arithmetic (var_large_hess_plan, pcl_host_launch_hess.hpp) -----------------------------------------------------------------
def lds_bytes(n, m, nc, mg):
    """var_large_hess_lds_bytes: the tile, nc (20 + 8 mg) column blocks, the slack, the drives, the partial sums."""
    LD = n | 1
    return (LD * n + LD * nc * (20 + 8 * mg) + SLACK + m + 8 + nc * (mg * (m + 1) + 1)) * 8


def plan(n, cols, m, cols_per_slice=0, drives=0):
    nc_cap = min(cols_per_slice, cols) if cols_per_slice > 0 else cols
    mg_cap = (min(drives, m) if drives > 0 else m) if m > 0 else 0
    mg_min = 1 if m > 0 else 0
    nc = 1
    for c in range(nc_cap, 1, -1):
        if lds_bytes(n, m, c, mg_min) <= LDS_BYTES:
            nc = c
            break
    mg = mg_min
    for g in range(mg_cap, mg_min, -1):
        if lds_bytes(n, m, nc, g) <= LDS_BYTES:
            mg = g
            break
    ngrp = -(-m // mg) if m > 0 else 1
    if m > 0:
        mg = -(-m // ngrp)
    sx = -(-cols // nc)
    nc = -(-cols // sx)
    return dict(LD=n | 1, threads=64 * ((n + 15) // 16), sx=sx, nc=nc, ngrp=ngrp, mg=mg, U=sx * ngrp, bytes=lds_bytes(n, m, nc, mg))


# ---- systems, trajectories, multipliers ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(name):
    """The VarCase, read-only."""
    if name != "VH1":
        return vl.case(name)[0]
    d, ket, v, m = VH1
    n, C = 2 * d, 1
    rng = np.random.default_rng(VH1_SEED)
    H0 = vsc._herm(d, rng)
    Hd = [vsc._herm(d, rng) for _ in range(m)]
    Hv = [vsc._herm(d, rng) for _ in range(v)]
    G0 = po.G_of_H(H0)
    Gj = np.array([po.G_of_H(H) for H in Hd]).reshape(m, n, n)
    Gv = [po.G_of_H(H) / s for H, s in zip(Hv, vl.SCALES)]
    xdc = n * C
    N, z_dim, xo, dt_off, u_off = 4, (v + 1) * xdc + 2 + m, [b * xdc for b in range(v + 1)], (v + 1) * xdc, (v + 1) * xdc + 2
    Z = 0.4 * np.random.default_rng(VH1_SEED + 1).standard_normal((N, z_dim))
    cs = vt.VarCase(Z=Z, z_dim=z_dim, N=N, n=n, C=C, m=m, xo=xo, u_off=u_off, dt_off=dt_off, G0=G0, Gv=Gv, Gj=Gj)
    n2 = [vsc._lifted_norm(cs, k) for k in range(3)]
    Z[:, dt_off] = 0.1
    Z[0, dt_off], Z[1, dt_off], Z[2, dt_off] = 0.15 / n2[0], -0.3 / n2[1], VH1_LONG / n2[2]
    Z[:, dt_off + 1] = np.cumsum(Z[:, dt_off])
    for a in [Z, G0, Gj] + Gv:
        a.setflags(write=False)
    return cs


def seed(name):
    return VH1_SEED if name == "VH1" else vl._seed(name)


@functools.lru_cache(maxsize=None)
def rand_mu(name):
    cs = case(name)
    mu = np.random.default_rng(seed(name) + 77).standard_normal(cs.K * cs.xd)
    mu.setflags(write=False)
    return mu


def mu_without_variations(name):
    """The same multipliers with zeros on the rows of every variation component."""
    cs = case(name)
    mu = np.array(rand_mu(name)).reshape(cs.K, 1 + cs.v, cs.xdc)
    mu[:, 1:] = 0.0
    return mu.reshape(-1)


# ---- the library's structure and value order (pcl_hess_structure of PCL_BATCH_VARIATIONAL, include/piccolo_hip.h) --------------------------------------
def values_per_interval(cs):
    return (cs.m + 1) * (cs.m + 2) // 2 + 2 * cs.xd * (cs.m + 1)


def lib_structure(cs, base=0):
    """(rows, cols), rows >= cols, of every Hessian value in the library's order."""
    m, xd, xdc, zd = cs.m, cs.xd, cs.xdc, cs.z_dim
    q = np.arange(xd)
    xin = np.asarray(cs.xo)[q // xdc] + q % xdc
    A, B = [], []
    for k in range(cs.K):
        uk, hk = k * zd + cs.u_off, k * zd + cs.dt_off
        a = [np.array([uk + i for i in range(m) for j in range(i + 1)], dtype=np.int64), np.full(m, hk), np.array([hk])]
        b = [np.array([uk + j for i in range(m) for j in range(i + 1)], dtype=np.int64), uk + np.arange(m), np.array([hk])]
        for knot in (0, 1):
            for l in range(m + 1):
                a.append(np.full(xd, uk + l if l < m else hk))
                b.append((k + knot) * zd + xin)
        A.append(np.concatenate(a))
        B.append(np.concatenate(b))
    A, B = np.concatenate(A).astype(np.int64), np.concatenate(B).astype(np.int64)
    return np.maximum(A, B) + base, np.minimum(A, B) + base


def value_index(cs):
    """Index into ONE interval's lifted Hessian values (pade_oracle.hess_structure's order for variational_truth.lifted's layout) of every value
    of the library's order."""
    nscal = (cs.m + 1) * (cs.m + 2) // 2
    rm = vt._row_map(cs)  # lifted position -> stacked position
    inv = np.empty_like(rm)
    inv[rm] = np.arange(rm.size)
    return np.concatenate([np.arange(nscal)] + [nscal + s * cs.xd + inv for s in range(2 * (cs.m + 1))])


def lifted_mu(cs, mu):
    return np.asarray(mu).reshape(cs.K, cs.xd)[:, vt._row_map(cs)]


def lifted_values(name, order, mu=None, zero_last_variation=False, **kw):
    """vector_shape_cases.truth_values on the lifted problem, in longdouble: the Hessian values [K, per] in the library's order.  kw:
    truth_values' switches (c, drop_drive, drop_col); zero_last_variation: Gv_v read as zero."""
    cs = case(name)
    Zl, lay, G0l, Gjl = vt.lifted(cs)
    if zero_last_variation:
        G0l = np.array(G0l)
        G0l[cs.v * cs.n :, : cs.n] = 0
    mul = lifted_mu(cs, rand_mu(name) if mu is None else mu)
    h = vs.truth_values(lay, G0l, Gjl, Zl, mul, order, hessian=True, **kw)[2]
    return h[:, value_index(cs)]


@functools.lru_cache(maxsize=None)
def truth_ld(name, order):
    """The Hessian values in the library's order, flat, in longdouble; computed once and never written to."""
    h = lifted_values(name, order).reshape(-1)
    h.setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def truth(name, order):
    """The same rounded to float64: what the GPU tests compare with."""
    h = truth_ld(name, order).astype(np.float64)
    h.setflags(write=False)
    return h


def oracle_values(name, order, mu=None):
    """The float64 lifted oracle (pade_oracle.pade_hessian_values) in the library's order, flat."""
    cs = case(name)
    Zl, lay, G0l, Gjl = vt.lifted(cs)
    mul = lifted_mu(cs, rand_mu(name) if mu is None else mu)
    return po.pade_hessian_values(Zl, mul, lay, G0l, Gjl, order)[:, value_index(cs)].reshape(-1)


@functools.lru_cache(maxsize=None)
def codes(name):
    """Segment code of every Hessian value: variational_shape_cases.hess_codes."""
    cs = case(name)
    a, b = lib_structure(cs)
    c = vsc.hess_codes(cs, a, b)
    c.setflags(write=False)
    return c


def segment_names(name):
    cs = case(name)
    return lambda s: vsc.hess_name(cs, s)


def check(name, order, vals, tol, what="", want=None):
    """Every segment of the Hessian values within tol of its own size (identically-zero segments: exact zeros).  Returns the worst (relative
    error, segment)."""
    want = truth(name, order) if want is None else want
    return vsc.assert_segments(vsc.segment_errors(codes(name), vals, want), tol, segment_names(name), "%s order %d %s Hessian" % (name, order, what))


def zero_segments(name, order):
    """The codes of the segments whose truth is identically zero."""
    return [s for s, mx in vsc.segment_max(codes(name), truth(name, order)).items() if mx == 0.0]


def component_slices(cs):
    """(index of every scalar and X_0 vector value, index of every X_b vector value, b > 0) within the values of all intervals, and the index
    of the same X_0 values in a plain context's values on component 0."""
    m, xd, xdc, per = cs.m, cs.xd, cs.xdc, values_per_interval(cs)
    nscal = (m + 1) * (m + 2) // 2
    per0 = nscal + 2 * xdc * (m + 1)
    seg = np.arange(2 * (m + 1))[:, None]
    x0 = np.concatenate([np.arange(nscal), (nscal + seg * xd + np.arange(xdc)[None]).reshape(-1)])
    p0 = np.concatenate([np.arange(nscal), (nscal + seg * xdc + np.arange(xdc)[None]).reshape(-1)])
    xb = (nscal + seg * xd + np.arange(xdc, xd)[None]).reshape(-1)
    k = np.arange(cs.K)[:, None]
    return (k * per + x0[None]).reshape(-1), (k * per + xb[None]).reshape(-1), (k * per0 + p0[None]).reshape(-1)


# ---- the kernel's formulation, float64 ------------------------------------------------------------------------------------------------------------------
def pass_values(name, order, mu=None, passes=None):
    """The Hessian values [K, per] in the library's order by the pass formulation of pcl_kernel_var_large_hess.hpp; passes: the passes to run
    (None: all, 0 .. v)."""
    cs = case(name)
    n, C, v, m, K = cs.n, cs.C, cs.v, cs.m, cs.K
    q = order // 2
    c = po.pade_coeffs(order)
    mu = np.asarray(rand_mu(name) if mu is None else mu).reshape(K, 1 + v, C, n)
    out = np.zeros((K, values_per_interval(cs)))
    col = lambda a: np.array(a.reshape(C, n).T)
    for k in range(K):
        h = cs.Z[k, cs.dt_off]
        G = cs.G0 + (np.tensordot(cs.Z[k, cs.u_off : cs.u_off + m], cs.Gj, axes=1) if m else 0)
        Xc = [col(cs.Z[k, o : o + cs.xdc]) for o in cs.xo]
        Xn = [col(cs.Z[k + 1, o : o + cs.xdc]) for o in cs.xo]
        Y = [[(-1) ** j * Xn[b] - Xc[b] for j in range(q + 1)] for b in range(1 + v)]
        T = [c[j] * h**j for j in range(q + 1)]
        Z0 = [None] * q  # Z0[s] = sum_{j > s} T_j G^(j-s-1) Y_{0,j}
        Z0[q - 1] = T[q] * Y[0][q]
        for s in range(q - 1, 0, -1):
            Z0[s - 1] = G @ Z0[s] + T[s] * Y[0][s]
        F, hu, hh = np.zeros((m, m)), np.zeros(m), 0.0
        zeros = lambda: np.zeros((n, C))
        A3, A5 = [[zeros() for _ in range(1 + v)] for _ in range(m)], [[zeros() for _ in range(1 + v)] for _ in range(m)]
        A4, A6 = [zeros() for _ in range(1 + v)], [zeros() for _ in range(1 + v)]
        for b in range(1 + v) if passes is None else passes:
            comps = [0, b] if b else [0]
            M = col(mu[k, b].reshape(-1))
            if b:
                Gv = cs.Gv[b - 1]
                Zb = [None] * q
                Zb[q - 1] = T[q] * Y[b][q]
                for s in range(q - 1, 0, -1):
                    Zb[s - 1] = G @ Zb[s] + Gv @ Z0[s] + T[s] * Y[b][s]
                Zs = {0: Z0, b: Zb}
                W, V = {0: zeros(), b: M}, {0: [zeros() for _ in range(m)], b: [zeros() for _ in range(m)]}
            else:
                Zs = {0: Z0}
                W, V = {0: M}, {0: [zeros() for _ in range(m)]}
            for s in range(1, q + 1):
                Wn, Vn = {}, {}
                for cp in comps:
                    Wn[cp] = G.T @ W[cp]
                    Vn[cp] = [G.T @ V[cp][l] + cs.Gj[l].T @ W[cp] for l in range(m)]
                if b:
                    Wn[0] = Wn[0] + Gv.T @ W[b]
                    Vn[0] = [Vn[0][l] + Gv.T @ V[b][l] for l in range(m)]
                W, V = Wn, Vn
                T1, T1m = s * c[s] * h ** (s - 1), s * c[s] * (-h) ** (s - 1)
                for cp in comps:
                    A4[cp] += T1 * W[cp]
                    A6[cp] += T1m * W[cp]
                    for l in range(m):
                        A3[l][cp] += T[s] * V[cp][l]
                        A5[l][cp] += c[s] * (-h) ** s * V[cp][l]
                        hu[l] += T1 * np.sum(V[cp][l] * Y[cp][s])
                        if s < q:
                            for t in range(m):
                                F[l, t] += np.sum(V[cp][l] * (cs.Gj[t] @ Zs[cp][s]))
                    if s >= 2:
                        hh += s * (s - 1) * c[s] * h ** (s - 2) * np.sum(W[cp] * Y[cp][s])
        flat = lambda A: np.concatenate([a.T.reshape(-1) for a in A])
        vals = [np.array([F[i, l] + F[l, i] for i in range(m) for l in range(i + 1)] + list(hu) + [hh])]
        vals += [-flat(A3[l]) for l in range(m)] + [-flat(A4)] + [flat(A5[l]) for l in range(m)] + [-flat(A6)]
        out[k] = np.concatenate(vals)
    return out


# ---- the finite-difference yardstick of the public-interface test ---------------------------------------------------------------------------------------
FD_EPS = 1e-5
FD_ORDER = 8
FD_ORACLE = 2.8e-11  # (measured 2.78e-11) what the float64 oracle's Hessian shows against the central difference of the oracle's Jacobian on VL1


def fd_inputs(cs):
    """(mu, v): multipliers and a direction in the variables, seeded."""
    rng = np.random.default_rng(16500)
    return rng.standard_normal(cs.K * cs.xd), rng.standard_normal(cs.N * cs.z_dim)


def fd_error(Hv, jt_mu, z, v):
    """max |H v - (J(z + eps v)^T mu - J(z - eps v)^T mu) / (2 eps)| relative to max |H v|; jt_mu(z) -> J(z)^T mu."""
    quot = (jt_mu(z + FD_EPS * v) - jt_mu(z - FD_EPS * v)) / (2 * FD_EPS)
    return float(np.abs(Hv - quot).max() / np.abs(Hv).max())


def fd_oracle_error():
    """The float64 lifted oracle's H v against its own central difference on VL1 at FD_ORDER."""
    import dataclasses

    import scipy.sparse as sp

    cs = case("VL1")
    mu, v = fd_inputs(cs)
    L = vt.hessian(cs, FD_ORDER, mu)[0]
    H = L + sp.tril(L, -1).T
    jt_mu = lambda z: vt.jacobian(dataclasses.replace(cs, Z=z.reshape(cs.N, cs.z_dim)), FD_ORDER)[0].T @ mu
    return fd_error(H @ v, jt_mu, np.array(cs.Z).reshape(-1), v)
