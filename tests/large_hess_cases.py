"""Cases for the Hessian of the Lagrangian at generator dimensions 66 .. 128 (a context created with PCL_LARGE_N and its option large_hess;
piccolo.jl_amd/csrc/pcl_kernel_pade_large_hess.hpp); importable without a GPU.

The cases, N = 4, the knots and the three steps are those of tests/large_shape_cases.py (L1 .. L9, `case(name, seed, drift)`); the multipliers
are np.random.default_rng(15000 + 17 index + 77 + member).standard_normal (vector_shape_cases.rand_mu does not know the L names); the truth is
vector_shape_cases.truth_values(..., mu, order, hessian=True)[2] in np.longdouble, computed once per (case, order, seed, drift, member).

The launch code's plan (large_hess_plan in pcl_host_launch_hess.hpp, restated below as `hess_plan`): beside the one n x n tile (LD = n | 1) a unit of nc
state columns and mg drives holds nc (10 + 4 mg) column blocks of LD doubles and nc (mg (m + 1) + 1) partial sums; the widest nc that leaves
room for one drive, then the most drives that fit, slices and groups evened.  What it gives per case (U units = workgroups per interval,
sx slices of nc columns x ngrp groups of mg drives, LDS bytes):
    L1  iso  66  1  2    U 1   1 (1)  x 1 (2)    46,184 B
    L2  iso  96  1  3    U 1   1 (1)  x 1 (3)    92,784 B
    L3  iso 128  1  2    U 1   1 (1)  x 1 (2)   151,832 B
    L4  iso 120  1 24    U 3   1 (1)  x 3 (8)   159,704 B     10 + 4 * 24 = 106 blocks against 47: three groups of eight drives
    L5  iso  72  5  4    U 1   1 (5)  x 1 (4)   119,928 B
    L6  iso  66 33  1    U 3   3 (11) x 1 (1)   119,280 B     33 columns x 14 blocks = 462 > 237: slices of 11 columns
    L7  vec  81  1  3    U 1   1 (1)  x 1 (3)    67,960 B
    L8  vec 121  1  2    U 1   1 (1)  x 1 (2)   135,712 B
    L9  vec 127  1  1    U 1   1 (1)  x 1 (1)   144,376 B
tests/test_large_hess_cpu.py asserts every number of this table against `hess_plan`, and that one column with one drive fits at n = 128, m = 24.

`formulation_values` restates the kernel's formulation (forward Horner chain Z, backward chains W and V on G^T, F[i, l] = sum <V_i, G_l Z>) in
float64 numpy, per state column and added in column order as the second launch does; the CPU tests hold it to the truth."""
import functools

import numpy as np

import large_shape_cases as lc
import vector_shape_cases as vc
from shape_cases import check_segments, hess_labels  # noqa: F401  (re-exported for the two test files)

N = lc.N
LDS_BYTES = lc.LDS_BYTES
ORDERS = lc.ORDERS
NAMES = lc.NAMES
CASES = lc.CASES
SLACK = lc.SLACK
TOL = 1e-11  # the library's tolerance for the Pade kernels, per segment (400 x the float64 oracle's floor on these cases)
# what large_hess_plan gives: (U, sx, nc, ngrp, mg, bytes)
TABLE = {
    "L1": (1, 1, 1, 1, 2, 46184), "L2": (1, 1, 1, 1, 3, 92784), "L3": (1, 1, 1, 1, 2, 151832), "L4": (3, 1, 1, 3, 8, 159704),
    "L5": (1, 1, 5, 1, 4, 119928), "L6": (3, 3, 11, 1, 1, 119280), "L7": (1, 1, 1, 1, 3, 67960), "L8": (1, 1, 1, 1, 2, 135712),
    "L9": (1, 1, 1, 1, 1, 144376),
}  # fmt: skip


# ---- the launch code's arithmetic (large_hess_plan, pcl_host_launch_hess.hpp) -------------------------------------------------------------------------
def hess_lds_bytes(n, m, nc, mg):
    LD = n | 1
    return (LD * n + LD * nc * (10 + 4 * mg) + SLACK + m + 8 + nc * (mg * (m + 1) + 1)) * 8


def hess_plan(n, cols, m, cols_per_slice=0, drives=0):
    nc_cap = min(cols_per_slice, cols) if cols_per_slice > 0 else cols
    mg_cap = (min(drives, m) if drives > 0 else m) if m > 0 else 0
    mg_min = 1 if m > 0 else 0
    nc = next((c for c in range(nc_cap, 1, -1) if hess_lds_bytes(n, m, c, mg_min) <= LDS_BYTES), 1)
    mg = next((g for g in range(mg_cap, mg_min, -1) if hess_lds_bytes(n, m, nc, g) <= LDS_BYTES), mg_min)
    ngrp = -(-m // mg) if m > 0 else 1
    if m > 0:
        mg = -(-m // ngrp)
    sx = -(-cols // nc)
    nc = -(-cols // sx)
    return dict(LD=n | 1, threads=64 * ((n + 15) // 16), sx=sx, nc=nc, ngrp=ngrp, mg=mg, U=sx * ngrp, bytes=hess_lds_bytes(n, m, nc, mg),
                nce=[max(0, min(nc, cols - s * nc)) for s in range(sx)], mge=[max(0, min(mg, m - g * mg)) for g in range(ngrp)])  # fmt: skip


# ---- multipliers and the truth ---------------------------------------------------------------------------------------------------------------
def rand_mu(name, member=0):
    lay = lc.layout(name)
    mu = np.random.default_rng(15000 + 17 * int(name[1:]) + 77 + member).standard_normal(lay.K * lay.x_dim)
    mu.setflags(write=False)
    return mu


@functools.lru_cache(maxsize=None)
def truth_ld(name, order, seed=0, drift=0, member=0):
    """The Hessian values, flat, in longdouble."""
    lay, G0, Gj, Z, _ = lc.case(name, seed, drift)
    h = vc.truth_values(lay, G0, Gj, Z, rand_mu(name, member), order, hessian=True)[2].reshape(-1)
    h.setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def truth(name, order, seed=0, drift=0, member=0):
    """The same rounded to float64: what the GPU tests compare with."""
    h = truth_ld(name, order, seed, drift, member).astype(np.float64)
    h.setflags(write=False)
    return h


# ---- the kernel's formulation in float64 -----------------------------------------------------------------------------------------------------
def formulation_values(lay, G0, Gj, Z, mu, order):
    """[K, hess_per]: the values as pcl_pade_large_hess_kernel and its sum kernel form them (not bit for bit: numpy's products)."""
    n, C, m, q = lay.n, lay.C, lay.m, order // 2
    c = vc.coeffs(order).astype(np.float64)
    mu = np.asarray(mu).reshape(lay.K, lay.x_dim)
    out = []
    for k in range(lay.K):
        h = Z[k, lay.dt_off]
        G = vc.g_of(lay, Z, k, G0, Gj)
        col = lambda v: np.asarray(v).reshape(C, n).T
        Xc, Xn, M = col(Z[k, lay.x_off : lay.x_off + n * C]), col(Z[k + 1, lay.x_off : lay.x_off + n * C]), col(mu[k])
        Y = [(-1) ** j * Xn - Xc for j in range(q + 1)]
        Zs = {}
        if q >= 2:
            Zs[q - 1] = c[q] * h**q * Y[q]
            for s in range(q - 2, 0, -1):
                Zs[s] = G @ Zs[s + 1] + c[s + 1] * h ** (s + 1) * Y[s + 1]
        W, V = M, [np.zeros((n, C)) for _ in range(m)]
        part = np.zeros((C, m, m + 1))  # per column: F[i, .] | hu_i
        hh = np.zeros(C)
        A3, A5 = [np.zeros((n, C)) for _ in range(m)], [np.zeros((n, C)) for _ in range(m)]
        A4, A6 = np.zeros((n, C)), np.zeros((n, C))
        for s in range(1, q + 1):
            V = [G.T @ V[l] + Gj[l].T @ W for l in range(m)]
            W = G.T @ W
            A4 += s * c[s] * h ** (s - 1) * W
            A6 += s * c[s] * (-h) ** (s - 1) * W
            for l in range(m):
                A3[l] += c[s] * h**s * V[l]
                A5[l] += c[s] * (-h) ** s * V[l]
                part[:, l, m] += s * c[s] * h ** (s - 1) * np.sum(V[l] * Y[s], axis=0)
            if s < q:
                for l in range(m):
                    y = Gj[l] @ Zs[s]
                    for i in range(m):
                        part[:, i, l] += np.sum(V[i] * y, axis=0)
            if s >= 2:
                hh += s * (s - 1) * c[s] * h ** (s - 2) * np.sum(W * Y[s], axis=0)
        hu = np.zeros(m)
        uu = np.zeros(m * (m + 1) // 2)
        for cc in range(C):  # the second launch: the columns in order
            e = 0
            for i in range(m):
                for l in range(i + 1):
                    uu[e] += part[cc, i, l] + part[cc, l, i]
                    e += 1
            hu += part[cc, :, m]
        flat = lambda A: A.T.reshape(-1)
        out.append(np.concatenate([uu, hu, [hh.sum()]] + [flat(-A) for A in A3] + [flat(-A4)] + [flat(A) for A in A5] + [flat(-A6)]))
    return np.array(out)


# ---- the d = 33 ket problem of the public-interface tests (that of tests/test_large_shapes_gpu.py) ---------------------------------------------
FD_EPS = 1e-5
FD_ORDER = 8
FD_ORACLE = 1.8e-9  # what the float64 oracle's Hessian shows against the central difference of the oracle's Jacobian (measured 1.76e-9: the eps^2 term)


def ket33_problem():
    """(system, trajectory, Z [N, dim], layout) -- an infeasible iterate, so that residuals and multipliers are of the states' size."""
    import piccolo_jl_amd as pa
    from oracle import pade_oracle as po

    d, m, N_ = 33, 2, 4
    rng = np.random.default_rng(15500)
    H = vc._herm(d, rng)
    Hs = [vc._herm(d, rng) for _ in range(m)]
    s = pa.QuantumSystem(H, Hs, [1.0] * m)
    psi = rng.standard_normal(d) + 1j * rng.standard_normal(d)
    psi /= np.linalg.norm(psi)
    times = np.cumsum(np.concatenate(([0.0], 0.005 + 0.005 * rng.random(N_ - 1))))
    traj = pa.ket_trajectory(s, 0.3 * rng.standard_normal((m, N_)), times, psi, psi)
    Z = traj.datavec.reshape(N_, traj.dim).copy()
    Z[1:, : 2 * d] += 0.05 * rng.standard_normal((N_ - 1, 2 * d))
    traj.update(Z.reshape(-1))
    KET = pa.trajectory.KET
    lay = po.Layout(d=d, m=m, N=N_, z_dim=traj.dim, x_off=traj.components[KET].start, u_off=traj.components["u"].start,
                    dt_off=traj.components[traj.timestep].start, cols=1)  # fmt: skip
    return s, traj, Z, lay


def fd_inputs(lay):
    """(mu, v): multipliers and a direction in the variables, seeded."""
    rng = np.random.default_rng(15501)
    return rng.standard_normal(lay.K * lay.x_dim), rng.standard_normal(lay.N * lay.z_dim)


def fd_error(Hv, jt_mu, z, v):
    """max |H v - (J(z + eps v)^T mu - J(z - eps v)^T mu) / (2 eps)| relative to max |H v|; jt_mu(z) -> J(z)^T mu."""
    quot = (jt_mu(z + FD_EPS * v) - jt_mu(z - FD_EPS * v)) / (2 * FD_EPS)
    return float(np.abs(Hv - quot).max() / np.abs(Hv).max())
