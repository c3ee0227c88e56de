"""Cases for the Hessian of the Lagrangian of the exponential constraint at generator dimensions 66 .. 128 (option large_exp_hess on a context
created with PCL_LARGE_N | PCL_LARGE_EXP; piccolo.jl_amd/csrc/pcl_kernel_large_exp_hess.hpp); importable without a GPU.

Systems, trajectories and steps: those of tests/large_exp_cases.py (imported, never written to) -- L1 .. L7, L9 and "L1z", N = 4, s' = 1, 3,
21 .. 51 and 0.  Multipliers: standard normal, seeded per case and member (`mu`).

Values, order and structure are those of tests/exp_hess_truth.py: per interval the five segments
    0 (u_i,u_l), l <= i | 1 (dt,u_l) | 2 (dt,dt) | 3 (u_l, X_k) | 4 (dt, X_k).
Truth (`truth`): exp_hess_truth.values (scipy expm of the 4n x 4n block matrix, expm_frechet), cached.  For L4 (m = 24: 300 pairs of 480 x 480
block exponentials per interval) segment 0 comes from the per-drive identity  (u_l,u_j) = -h <L2(A^T; M X_k^T, h G_l^T), G_j>  (`values_per_drive`:
24 calls of exp_hess_truth.frechet2 per interval); tests/test_large_exp_hess_cpu.py holds that identity to the pairwise truth on L1 and L2.

Emulation (`emulate_hess`): the kernel's recurrence in float64 numpy; it shares no code with the truth.  Per substep, from Y (at first M), dY_l
(at first 0) and d2Y_il (l <= i, at first 0), Horner for j = DEG .. 1 with f = h_s / j, every right-hand side from before the level's update:
    d2W_il <- d2Y_il + f (G^T d2W_il + G_i^T dW_l + G_l^T dW_i)
    dW_l   <- dY_l   + f (G^T dW_l   + G_l^T W)
    W      <- Y      + f  G^T W
then Y <- W, ...; segment 0 = -sum <d2W_il, X_k>, 1 = -<dW_l, G X_k> - <W, G_l X_k>, 2 = -<G^T W, G X_k>, 3 = -dW_l, 4 = -G^T W.

`plan` restates large_exp_hess_plan (pcl_host_launch_hess.hpp): among the slice widths and group sizes that fit, the fewest 16-column tile passes
per interval.  What it gives (U units = workgroups per interval: sx state-column slices of nc columns x ngrp (ngrp + 1) / 2 pairs of drive groups
of mg drives; W columns per buffer of the NBW that fit -- the off-diagonal count wherever there is more than one group; LDS bytes, all <= 163,840):
    L1   iso  66  1  2   U 1    1 (1) x 1 pair   (mg 2)   W  6 of 79    46,128 B
    L2   iso  96  1  3   U 1    1 (1) x 1 pair   (mg 3)   W 10 of 37    98,888 B
    L3   iso 128  1  2   U 1    1 (1) x 1 pair   (mg 2)   W  6 of  9   151,776 B   (large_exp_hess_drives = 1: two groups, W 4, the off-diagonal unit)
    L4   iso 120  1 24   U 78   1 (1) x 78 pairs (mg 2)   W  9 of 15   143,576 B   mg = 3 would need 16 columns off the diagonal
    L5   iso  72  5  4   U 5    5 (1) x 1 pair   (mg 4)   W 15 of 68    69,448 B   (cols_per_slice = 2: 3 (2) x 1 pair, W 30; = 5: 1 (5) x 3 pairs of mg 2, W 45)
    L6   iso  66 33  1   U 7    7 (5) x 1 pair   (mg 1)   W 15 of 79    60,592 B   (cols_per_slice = 7: 5 (7), W 21: two tiles per unit)
    L7   vec  81  1  3   U 1    1 (1) x 1 pair   (mg 3)   W 10 of 56    73,040 B
    L9   vec 127  1  1   U 1    1 (1) x 1 pair   (mg 1)   W  3 of 11   139,272 B
tests/test_large_exp_hess_cpu.py asserts every number of this table against `plan`."""
import functools

import numpy as np

import exp_hess_truth as eht
import large_exp_cases as le

N = le.N
LDS_BYTES = le.LDS_BYTES
SLACK = le.SLACK
DEG = le.DEG
CASES = le.CASES
NAMES = le.NAMES
# (U, sx, nc, ngrp, mg, W, NBW, bytes)
TABLE = {
    "L1": (1, 1, 1, 1, 2, 6, 79, 46128), "L2": (1, 1, 1, 1, 3, 10, 37, 98888), "L3": (1, 1, 1, 1, 2, 6, 9, 151776),
    "L4": (78, 1, 1, 12, 2, 9, 15, 143576), "L5": (5, 5, 1, 1, 4, 15, 68, 69448), "L6": (7, 7, 5, 1, 1, 15, 79, 60592),
    "L7": (1, 1, 1, 1, 3, 10, 56, 73040), "L9": (1, 1, 1, 1, 1, 3, 11, 139272),
}  # fmt: skip


# ---- the launch code's arithmetic (large_exp_hess_plan, pcl_host_launch_hess.hpp) ---------------------------------------------------------------
def unit_columns(mg, diagonal):
    """Columns a unit carries per state column: W, the dW of its drives, the d2W of its pairs (no drives: W alone, and two behind the chain)."""
    if mg == 0:
        return 2
    return 1 + mg + mg * (mg + 1) // 2 if diagonal else 1 + 2 * mg + mg * mg


def plan(n, cols, m, cols_per_slice=0, drives=0):
    LD, threads = n | 1, 64 * ((n + 15) // 16)
    fixed = LD * n + SLACK + m + 8
    NB = (LDS_BYTES // 8 - fixed) // LD
    NBW = NB // 3
    t_min = 2 if m == 0 else (3 if m == 1 else 4)
    nc_hi = min(max(1, NBW // t_min), min(cols_per_slice, cols) if cols_per_slice > 0 else min(cols, 16))
    nc_lo = nc_hi if cols_per_slice > 0 else 1
    mg_cap = (min(drives, m) if drives > 0 else m) if m > 0 else 0
    best = None
    for nc0 in range(nc_hi, nc_lo - 1, -1):
        sx = -(-cols // nc0)
        nc = -(-cols // sx)
        for mg0 in range(mg_cap, (1 if m > 0 else 0) - 1, -1):
            ngrp = -(-m // mg0) if m > 0 else 1
            mg = -(-m // ngrp) if m > 0 else 0
            Td, To = unit_columns(mg, True), unit_columns(mg, False)
            W = nc * (To if ngrp > 1 else Td)
            if W > NBW:
                continue
            npo = ngrp * (ngrp - 1) // 2
            passes = sx * (ngrp * ((nc * (Td if m > 0 else 1) + 15) // 16) + npo * ((nc * To + 15) // 16))
            units = sx * (ngrp + npo)
            if best is None or (passes, units) < (best["passes"], best["U"]):
                best = dict(sx=sx, nc=nc, mg=mg, ngrp=ngrp, U=units, W=W, passes=passes)
    return dict(best, LD=LD, threads=threads, NB=NB, NBW=NBW, bytes=(fixed + 3 * LD * best["W"]) * 8)


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------------
case = le.case
layout = le.layout


@functools.lru_cache(maxsize=None)
def mu(name, seed=0, drift=0):
    """The multipliers of one member, [K, x_dim] like delta; read-only."""
    lay = le.layout(name)
    rng = np.random.default_rng(26000 + 17 * int(name[1:2]) + 101 * seed + 1009 * drift + (7 if name.endswith("z") else 0))
    a = rng.standard_normal((lay.K, lay.x_dim))
    a.setflags(write=False)
    return a


def labels(lay):
    """One label per value: the five segments, per interval."""
    m, xd = lay.m, lay.x_dim
    per = ["seg0"] * (m * (m + 1) // 2) + ["seg1"] * m + ["seg2"] + ["seg3"] * (m * xd) + ["seg4"] * xd
    return np.concatenate([np.char.add(np.array(per), "@%d" % k) for k in range(lay.K)])


# ---- the truth ------------------------------------------------------------------------------------------------------------------------------------
def values_per_drive(Z, mu_, lay, G0, Gj):
    """exp_hess_truth.values with segment 0 from the per-drive identity (u_l,u_j) = -h <L2(A^T; M X^T, h G_l^T), G_j>: m block exponentials per
    interval instead of m (m + 1) / 2."""
    import scipy.linalg

    m = lay.m
    out = []
    for k in range(lay.K):
        G = G0 + np.tensordot(lay.u(Z, k), Gj, axes=1) if m else G0
        h, X, M = lay.dt(Z, k), lay.X(Z, k), np.asarray(mu_)[k].reshape(lay.C, lay.n).T
        A = h * G
        E = scipy.linalg.expm(A)
        L = [scipy.linalg.expm_frechet(A, h * Gj[l], compute_expm=False) for l in range(m)]
        F = [eht.frechet2(A.T, M @ X.T, h * Gj[l].T) for l in range(m)]
        seg = [[-h * np.sum(F[i] * Gj[j])] for i in range(m) for j in range(i + 1)]
        seg += [[-np.sum(M * ((Gj[j] @ E + G @ L[j]) @ X))] for j in range(m)]
        seg.append([-np.sum(M * (G @ G @ E @ X))])
        seg += [(-(L[l].T @ M)).T.reshape(-1) for l in range(m)]
        seg.append((-((G @ E).T @ M)).T.reshape(-1))
        out.append(np.concatenate(seg))
    return np.array(out)


@functools.lru_cache(maxsize=None)
def truth(name, seed=0, drift=0):
    """The values of one member, flat, in the library's order; read-only."""
    lay, G0, Gj, Z = le.case(name, seed, drift)
    f = values_per_drive if lay.m > 6 else eht.values
    out = f(Z, mu(name, seed, drift), lay, G0, Gj).reshape(-1)
    out.setflags(write=False)
    return out


# ---- the kernel's recurrence in float64 numpy -------------------------------------------------------------------------------------------------------
def emulate_hess(lay, G0, Gj, Z, mu_, drop_cross=False, updated_dw=False, drop_substep=False, drop_col=False, no_w_glx=False):
    """The values, flat.  Faults: drop_cross leaves G_l^T dW_i out of the d2W update, updated_dw takes this level's dW there, drop_substep runs
    s' - 1 of the s' substeps, drop_col leaves the last state column out of the sums, no_w_glx leaves <W, G_l X_k> out of segment 1."""
    n, C, m, K = lay.n, lay.C, lay.m, lay.K
    pairs = [(i, l) for i in range(m) for l in range(i + 1)]
    GjT = np.array([Gj[l].T for l in range(m)]).reshape(m * n, n) if m else np.zeros((0, n))
    out = []
    for k in range(K):
        G = G0 + np.tensordot(lay.u(Z, k), Gj, axes=1) if m else np.array(G0)
        GT = G.T
        h = lay.dt(Z, k)
        sp = le.substeps(h, G)
        hs = h / sp if sp else 0.0
        X, M = lay.X(Z, k), np.asarray(mu_)[k].reshape(C, n).T
        Y, dY, d2Y = M.copy(), np.zeros((m, n, C)), np.zeros((len(pairs), n, C))
        for _ in range(sp - 1 if drop_substep else sp):
            W, dW, d2W = Y, dY, d2Y
            for j in range(DEG, 0, -1):
                f = hs / j
                Wn = Y + f * (GT @ W)
                dWn = np.array([dY[l] + f * (GT @ dW[l] + Gj[l].T @ W) for l in range(m)]).reshape(m, n, C)
                src = dWn if updated_dw else dW
                # S[i, l] = G_i^T dW_l
                S = (GjT @ src.transpose(1, 0, 2).reshape(n, m * C)).reshape(m, n, m, C).transpose(0, 2, 1, 3) if m else None
                d2W = np.array([d2Y[q] + f * (GT @ d2W[q] + S[i, l] + (0.0 if drop_cross else S[l, i])) for q, (i, l) in enumerate(pairs)]).reshape(len(pairs), n, C)
                W, dW = Wn, dWn
            Y, dY, d2Y = W, dW, d2W
        GX, GTW = G @ X, GT @ Y
        cs = slice(0, C - 1) if drop_col else slice(0, C)
        seg = [[-np.sum(d2Y[q][:, cs] * X[:, cs])] for q in range(len(pairs))]
        seg += [[-np.sum(dY[l][:, cs] * GX[:, cs]) - (0.0 if no_w_glx else np.sum(Y[:, cs] * (Gj[l] @ X)[:, cs]))] for l in range(m)]
        seg.append([-np.sum(GTW[:, cs] * GX[:, cs])])
        seg += [(-dY[l]).T.reshape(-1) for l in range(m)]
        seg.append((-GTW).T.reshape(-1))
        out.append(np.concatenate(seg))
    return np.concatenate(out)
