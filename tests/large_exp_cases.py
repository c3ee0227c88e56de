"""Cases for the exponential constraint at generator dimensions 66 .. 128 (contexts created with PCL_LARGE_N | PCL_LARGE_EXP and pade_order =
PCL_ORDER_EXP; piccolo.jl_amd/csrc/pcl_kernel_large_exp.hpp); importable without a GPU.

Systems: those of tests/large_shape_cases.py (imported, never written to) -- L1 .. L7 and L9.  The knot is [X | dt | t | u], N = 4, u ~ 0.4 N(0, 1).
Steps, per case from |G(u_k)|_1 (the norm the kernel takes its substep count s' = ceil(|h| |G|_1) from):
    interval 0   h |G|_1 =  0.8          s' = 1
    interval 1   h |G|_1 = -2.5          s' = 3     (a negative step is an ordinary step)
    interval 2   h |G|_1 = LONG[case]    s' = 21 .. 51
and one variant of L1 ("L1z") whose interval 1 has h = 0 (s' = 0: E = I exactly, zero drive tails).  None of the products h |G|_1 is near an
integer, so the s' of the device, of the emulation and of this table agree whatever the order of the norm's additions.

Truth: the committed oracle's po.exp_residual / po.exp_jacobian_values (scipy expm / expm_frechet), mapped to the library's layout by
tests/exp_truth.py.  Emulation (`emulate`): the kernel's recurrence in float64 numpy, every product through an `mm` hook; it shares no code
with the truth.  Per substep, from Y (at first X_k) and dY_l (at first 0), Horner for j = DEG .. 1 with f = h_s / j:
    dV_l <- dY_l + f (G dV_l + G_l V)    (the V before this level's update)
    V    <- Y + f G V
then Y <- V, dY_l <- dV_l; delta = X_{k+1} - Y, drive tails -dY_l, dt tail -G Y, and -E the V recurrence on the identity.

`plan` restates large_exp_plan (pcl_host_launch_pade.hpp).  What it gives for a Jacobian launch of the three intervals on 256 CUs
(U units = workgroups per interval, sx state-column slices of nc columns x ngrp drive groups of mg drives, npc columns of E per unit, LDS bytes):
    L1   iso  66  1  2   U 5    1 (1) x 2 (1)    npc 14    62,208 B
    L2   iso  96  1  3   U 7    1 (1) x 3 (1)    npc 14   112,856 B
    L3   iso 128  1  2   U 19   1 (1) x 2 (1)    npc  7   161,064 B   nine columns per buffer beside the tile
    L4   iso 120  1 24   U 11   1 (1) x 8 (3)    npc 11   161,000 B   fifteen columns per buffer: the drives in eight groups of three
    L5   iso  72  5  4   U 12   1 (5) x 4 (1)    npc  6    71,200 B   (cols_per_slice = 2: slices of 2, 2, 1)
    L6   iso  66 33  1   U 7    3 (11) x 1 (1)   npc 10    87,928 B   more than 16 columns: three slices; two column tiles per unit
    L7   vec  81  1  3   U 6    1 (1) x 3 (1)    npc 14    84,704 B
    L9   vec 127  1  1   U 15   1 (1) x 1 (1)    npc  9   163,656 B
(a launch of three intervals is one round of the CUs whatever the split, so the plan with the fewest tile passes wins: one drive per group
wherever a group's chain and the columns of E share one 16-column tile; a launch of 99 intervals of L5 takes 2 units of four drives each.)
tests/test_large_exp_cpu.py asserts every number of this table against `plan`."""
import functools

import numpy as np

import exp_shape_cases as xs
import exp_truth as xt
import large_shape_cases as lc
import vector_shape_cases as vc
from oracle import pade_oracle as po

N = lc.N
LDS_BYTES = lc.LDS_BYTES
SLACK = lc.SLACK
DEG = 18  # LE_DEG
SMAX = 1024  # LR_SMAX
CASES = {k: lc.CASES[k] for k in ("L1", "L2", "L3", "L4", "L5", "L6", "L7", "L9")}
NAMES = list(CASES)
LONG = {"L1": 20.5, "L2": 27.3, "L3": 33.7, "L4": 24.1, "L5": 38.9, "L6": 44.2, "L7": 50.6, "L9": 30.4}
STEPS = (0.8, -2.5)
# (U, sx, nc, ngrp, mg, npc, bytes)
TABLE = {
    "L1": (5, 1, 1, 2, 1, 14, 62208), "L2": (7, 1, 1, 3, 1, 14, 112856), "L3": (19, 1, 1, 2, 1, 7, 161064), "L4": (11, 1, 1, 8, 3, 11, 161000),
    "L5": (12, 1, 5, 4, 1, 6, 71200), "L6": (7, 3, 11, 1, 1, 10, 87928), "L7": (6, 1, 1, 3, 1, 14, 84704), "L9": (15, 1, 1, 1, 1, 9, 163656),
}  # fmt: skip


# ---- the launch code's arithmetic (large_exp_plan, pcl_host_launch_pade.hpp) ------------------------------------------------------------------------
def plan(n, cols, m, jac=True, items=N - 1, n_cu=256, cols_per_slice=0, slices=0, drives=0):
    LD, threads = n | 1, 64 * ((n + 15) // 16)
    fixed = LD * n + SLACK + m + 8
    NB = (LDS_BYTES // 8 - fixed) // LD
    NBW = NB // 3
    drv = jac and m > 0
    nc_cap = min(cols_per_slice, cols) if cols_per_slice > 0 else min(cols, 16)
    nc = max(1, min(nc_cap, (NBW - (1 if jac else 0)) // (2 if drv else 1)))
    sx = -(-cols // nc)
    nc = -(-cols // sx)
    mg, ngrp, U, npc = 0, 1, sx, 0
    if jac:
        mg_fit = max(1, min(m, (NBW - 1) // nc - 1)) if drv else 0
        if drv and drives > 0:
            mg_fit = min(mg_fit, drives)
        best_t = best_p = -1
        for mg0 in range(mg_fit, (1 if drv else 0) - 1, -1):
            g_ = -(-m // mg0) if drv else 1
            mg_ = -(-m // g_) if drv else 0
            cx = nc * (1 + mg_)
            npc_max = max(1, min(n, NBW - cx))
            for npc0 in (npc_max, min(npc_max, 16 * (cx // 16 + 1) - cx)):
                U_ = max(sx * g_, -(-n // npc0))
                tiles, rounds = (cx + -(-n // U_) + 15) // 16, -(-max(items, 1) * U_ // n_cu)
                t, passes = tiles * rounds, tiles * U_
                if best_t < 0 or t < best_t or (t == best_t and passes < best_p):
                    best_t, best_p, mg, ngrp, U = t, passes, mg_, g_, U_
            if not drv:
                break
        chain_units = sx * ngrp
        if slices > 0:
            U = max(U, min(slices, n))
        npc = -(-n // U)
        U = max(chain_units, -(-n // npc))
    W = nc * (1 + mg) + npc
    return dict(LD=LD, threads=threads, NB=NB, NBW=NBW, sx=sx, nc=nc, mg=mg, ngrp=ngrp, U=U, npc=npc, W=W, bytes=(fixed + 3 * LD * W) * 8)


# ---- trajectories -------------------------------------------------------------------------------------------------------------------------------------
def _base(name):
    return name[:2]


def layout(name):
    return lc.layout(_base(name))


def norm1(G):
    return float(np.abs(G).sum(axis=0).max())


def substeps(h, G):
    x = abs(h) * norm1(G)
    return 0 if x == 0 else (int(np.ceil(x)) if x <= SMAX else SMAX)


@functools.lru_cache(maxsize=None)
def case(name, seed=0, drift=0):
    """(layout, G0, Gj, Z), read-only.  name: a key of CASES, or "L1z" (L1 with h = 0 on interval 1).  seed: another trajectory of the same system;
    drift: the member's drift on the SAME trajectory (the steps are those of drift 0)."""
    base = _base(name)
    lay = lc.layout(base)
    G0, Gj = lc.system(base, 0)
    rng = np.random.default_rng(25000 + 17 * int(base[1:]) + seed)
    Z = 0.4 * rng.standard_normal((N, lay.z_dim))
    n1 = [norm1(vc.g_of(lay, Z, k, G0, Gj)) for k in range(N - 1)]
    Z[0, lay.dt_off], Z[1, lay.dt_off], Z[2, lay.dt_off], Z[N - 1, lay.dt_off] = STEPS[0] / n1[0], STEPS[1] / n1[1], LONG[base] / n1[2], 0.1
    if name.endswith("z"):
        Z[1, lay.dt_off] = 0.0
    Z[:, lay.dt_off + 1] = np.cumsum(Z[:, lay.dt_off])
    G0 = lc.system(base, drift)[0]
    for a in (G0, Gj, Z):
        a.setflags(write=False)
    return lay, G0, Gj, Z


def residual_labels(lay):
    return xs.residual_labels(lay.n, lay.C, lay.K)


def jac_labels(lay):
    return xs.jac_labels(lay.n, lay.C, lay.m, lay.K)


# ---- the truth: scipy expm / expm_frechet through the committed oracle, computed once and never written to ----------------------------------------
@functools.lru_cache(maxsize=None)
def truth(name, seed=0, drift=0):
    """(delta, Jacobian values), flat, in the library's order."""
    lay, G0, Gj, Z = case(name, seed, drift)
    out = (po.exp_residual(Z, lay, G0, Gj).reshape(-1), xt.values(Z, lay, G0, Gj).reshape(-1))
    for a in out:
        a.setflags(write=False)
    return out


# ---- the kernel's recurrence in float64 numpy -----------------------------------------------------------------------------------------------------
def emulate(lay, G0, Gj, Z, mm=np.matmul, drop_substep=False, updated_v=False, drop_drive=False, drop_col=False):
    """(delta, values), flat.  Faults: drop_substep runs s' - 1 of the s' substeps, updated_v takes G_l V with the V of THIS level, drop_drive
    leaves the last drive out of G(u) and of the tails, drop_col leaves the last state column at its initial value."""
    n, C, m, K = lay.n, lay.C, lay.m, lay.K
    delta, vals = [], []
    me = m - 1 if drop_drive else m
    for k in range(K):
        u = Z[k, lay.u_off : lay.u_off + m]
        G = G0 + np.tensordot(u[:me], Gj[:me], axes=1) if me else np.array(G0)
        h = Z[k, lay.dt_off]
        sp = substeps(h, G)
        hs = h / sp if sp else 0.0
        X = lay.X(Z, k)
        Y, dY, P = X.copy(), np.zeros((m, n, C)), np.eye(n)
        for _ in range(sp - 1 if drop_substep else sp):
            V, dV, Q = Y, dY, P
            for j in range(DEG, 0, -1):
                f = hs / j
                Vn = Y + f * mm(G, V)
                dV = np.array([dY[l] + f * (mm(G, dV[l]) + mm(Gj[l], Vn if updated_v else V)) if l < me else dY[l] for l in range(m)]).reshape(m, n, C)
                Q = P + f * mm(G, Q)
                V = Vn
            Y, dY, P = V, dV, Q
        if drop_col:
            Y, dY = Y.copy(), dY.copy()
            Y[:, C - 1], dY[:, :, C - 1] = X[:, C - 1], 0.0
        delta.append((lay.X(Z, k + 1) - Y).T.reshape(-1))
        GY = mm(G, Y)
        tails = np.stack([np.concatenate([-dY[l, :, c] for l in range(m)] + [-GY[:, c]]) for c in range(C)])
        vals.append(np.concatenate([np.tile(-P.T.reshape(-1), C), np.ones(n * C), tails.reshape(-1)]))
    return np.concatenate(delta), np.concatenate(vals)


# ---- faults of the products, through the `mm` hook (those of tests/large_shape_cases.py) ----------------------------------------------------------
mm_drop_k_beyond_64 = lc.mm_drop_k_beyond_64
mm_zero_last_row_tile = lc.mm_zero_last_row_tile
