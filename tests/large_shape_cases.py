"""Cases for generator dimensions 66 .. 128 (contexts created with PCL_LARGE_N; piccolo.jl_amd/csrc/pcl_kernel_pade_large.hpp), at the sizes at
which the launch code's plan (large_plan in pcl_host_launch_pade.hpp, restated below) and the kernel branch; importable without a GPU.

The knot, N = 4 and the three steps per case are those of tests/vector_shape_cases.py -- [X | dt | t | u], u ~ 0.4 N(0, 1); interval 0 at
h |G|_2 = 0.15, interval 1 at -0.3, interval 2 at the smallest of vc.LONG_STEPS at which zeroing c_5 of order 10 moves the residual by 1e-7 of
its size -- and so are the generators (iso: G(H) of a dense complex Hermitian H; vec: a general real n x n matrix / sqrt(n) under
PCL_STATE_VECTOR).  The truth, the coefficient vector and the `mm` hook are that module's (truth_values, coeffs, top_term_weight); nothing here
writes into its CASES.  Seeds: 15000 + 17 index.

Cases (kind, n, cols, m), the branch each sits on, and what the plan gives for the three intervals of a test launch (U units = workgroups per
interval, sx state-column slices x ngrp drive groups of mg drives, npc power columns per unit, LDS bytes):
    L1  iso  66  1  2   first n past 64: a fifth row tile of two rows, the 17th k-step half used           U 5   1 x 1 (2)   npc 14   49,344 B
    L2  iso  96  1  3   the 4 x 12 transmon-cavity size: six full row tiles                               U 6   1 x 1 (3)   npc 16   97,336 B
    L3  iso 128  1  2   largest: 32 full k-steps; the panel must be split (29 blocks beside the tile)     U 8   1 x 1 (2)   npc 16  160,032 B
    L4  iso 120  1 24   the 4 x 15 size with the ABI's most drives: 54 chain blocks against 47:           U 8   1 x 2 (12)  npc 15  161,000 B
                        two drive groups
    L5  iso  72  5  4   multi-ket: five columns in one chain unit; under cols_per_slice = 2 the slices    U 5   1 x 1 (4)   npc 15   92,808 B
                        hold 2, 2, 1
    L6  iso  66 33  1   unitary d = 33: 33 copies of each block; 33 columns x 8 blocks = 264 > 237:       U 5   2 x 1 (1)   npc 14  116,872 B
                        slices of 17 and 16 columns
    L7  vec  81  1  3   9-level density vector, n mod 16 = 1, odd: scalar block stores, straddling pairs  U 6   1 x 1 (3)   npc 14   70,448 B
    L8  vec 121  1  2   11-level density vector                                                           U 8   1 x 1 (2)   npc 16  143,400 B
    L9  vec 127  1  1   largest odd n                                                                     U 8   1 x 1 (1)   npc 16  154,512 B
tests/test_large_shapes_cpu.py asserts every number of this table against `large_plan`.

Checked there as well: every case finds its long step (0.5 for the iso cases, 0.65 for the vec cases); the reference formulation in float64
(oracle/pade_oracle.py) agrees with the longdouble truth per segment to 1e-13; and each of four faults -- every product's k range beyond 64
dropped, the last 16-row tile zeroed, the last drive dropped, the last state column dropped -- moves a segment by 1e-7 or more."""
import functools

import numpy as np

import vector_shape_cases as vc
from oracle import pade_oracle as po
from shape_cases import check_segments, jac_labels  # noqa: F401  (re-exported for the two test files)

N = vc.N
LDS_BYTES = vc.LDS_BYTES
ORDERS = vc.ORDERS
SEEN = vc.SEEN
NP_PAIRS = 8  # PL_NP
SLACK = 128  # PL_SLACK

# name: (kind, n, cols, m)
CASES = {
    "L1": ("iso", 66, 1, 2), "L2": ("iso", 96, 1, 3), "L3": ("iso", 128, 1, 2), "L4": ("iso", 120, 1, 24), "L5": ("iso", 72, 5, 4),
    "L6": ("iso", 66, 33, 1), "L7": ("vec", 81, 1, 3), "L8": ("vec", 121, 1, 2), "L9": ("vec", 127, 1, 1),
}  # fmt: skip
NAMES = list(CASES)
# what large_plan gives for a Jacobian launch of the three intervals on 256 CUs: (U, sx, ngrp, mg, npc, bytes)
TABLE = {
    "L1": (5, 1, 1, 2, 14, 49344), "L2": (6, 1, 1, 3, 16, 97336), "L3": (8, 1, 1, 2, 16, 160032), "L4": (8, 1, 2, 12, 15, 161000),
    "L5": (5, 1, 1, 4, 15, 92808), "L6": (5, 2, 1, 1, 14, 116872), "L7": (6, 1, 1, 3, 14, 70448), "L8": (8, 1, 1, 2, 16, 143400),
    "L9": (8, 1, 1, 1, 16, 154512),
}  # fmt: skip


# ---- the launch code's arithmetic (large_plan, pcl_host_launch_pade.hpp) -----------------------------------------------------------------------------
def large_plan(n, cols, m, jac=True, items=N - 1, n_cu=256, cols_per_slice=0, slices=0):
    LD, threads = n | 1, 64 * ((n + 15) // 16)
    fixed = LD * n + SLACK + m + 8
    NB = (LDS_BYTES // 8 - fixed) // LD
    nc_cap = min(cols_per_slice, cols) if cols_per_slice > 0 else cols
    nc_, mg = 1, (1 if jac and m > 0 else 0)
    for nc in range(nc_cap, 0, -1):
        if not jac:
            if 4 * nc > NB and nc > 1:
                continue
            nc_ = nc
            break
        mg_max = min(m, ((NB - 1) // nc - 6) // 2) if m > 0 else 0
        if (mg_max < 1 if m > 0 else 6 * nc + 1 > NB) and nc > 1:
            continue
        nc_, mg = nc, (max(mg_max, 1) if m > 0 else 0)
        break
    nc = nc_
    ngrp = -(-m // mg) if jac and m > 0 else 1
    if jac and m > 0:
        mg = -(-m // ngrp)
    sx = -(-cols // nc)
    nc = -(-cols // sx)
    chain_units, chain_blocks = sx * ngrp, nc * ((2 + 2 * (2 + mg)) if jac else 4)
    U, npc = chain_units, 0
    if jac:
        fits = lambda U: chain_blocks + -(-n // U) <= NB and (n * -(-n // U) + 1) // 2 <= NP_PAIRS * threads
        while U < n and not fits(U):
            U += 1
        want = slices if slices > 0 else min(max(chain_units, (n + 15) // 16), n_cu // max(items, 1))
        U = max(U, min(want, n))
        npc = -(-n // U)
        U = max(chain_units, -(-n // npc))
    pairs = -(-((n * npc + 1) // 2) // threads) if jac else 0
    return dict(LD=LD, threads=threads, NB=NB, nc=nc, mg=mg, ngrp=ngrp, sx=sx, U=U, npc=npc, chain_blocks=chain_blocks,
                bytes=(fixed + LD * (chain_blocks + npc)) * 8, row_tiles=(n + 15) // 16, k_steps=(n + 3) // 4, pairs=pairs,
                nce=[max(0, min(nc, cols - s * nc)) for s in range(sx)], npce=[max(0, min(npc, n - u * npc)) for u in range(U)])  # fmt: skip


# ---- systems and trajectories (vector_shape_cases.system / case, with this table and these seeds) ---------------------------------------------
def _seed(name):
    return 15000 + 17 * int(name[1:])


@functools.lru_cache(maxsize=None)
def system(name, drift=0):
    """(G0, Gj).  drift > 0: another drift for the same drives (a member of a PCL_BATCH_MEMBERS launch)."""
    kind, n, cols, m = CASES[name]
    rng = np.random.default_rng(_seed(name))
    if kind == "vec":
        G0s = [rng.standard_normal((n, n)) / np.sqrt(n) for _ in range(3)]
        Gj = rng.standard_normal((m, n, n)) / np.sqrt(n)
    else:
        G0s = [po.G_of_H(vc._herm(n // 2, rng)) for _ in range(3)]
        Gj = np.array([po.G_of_H(vc._herm(n // 2, rng)) for _ in range(m)])
    return G0s[drift], Gj


def layout(name):
    kind, n, cols, m = CASES[name]
    xs = n * cols
    if kind == "vec":
        return po.Layout(d=0, m=m, N=N, z_dim=xs + 2 + m, x_off=0, u_off=xs + 2, dt_off=xs, cols=1, gen=n)
    return po.Layout(d=n // 2, m=m, N=N, z_dim=xs + 2 + m, x_off=0, u_off=xs + 2, dt_off=xs, cols=cols)


@functools.lru_cache(maxsize=None)
def case(name, seed=0, drift=0):
    """(layout, G0, Gj, Z, long step), read-only.  seed: another trajectory of the same system (a seed of a PCL_BATCH_TRAJ launch).  drift: the
    member's drift on the SAME trajectory (the members of a PCL_BATCH_MEMBERS launch share the knots: the steps are those of drift 0)."""
    lay = layout(name)
    G0, Gj = system(name, 0)
    rng = np.random.default_rng(_seed(name) + 1 + seed)
    Z = 0.4 * rng.standard_normal((N, lay.z_dim))
    n2 = [np.linalg.norm(vc.g_of(lay, Z, k, G0, Gj), 2) for k in range(N - 1)]
    Z[0, lay.dt_off], Z[1, lay.dt_off], Z[N - 1, lay.dt_off] = 0.15 / n2[0], -0.3 / n2[1], 0.1
    long_step = None
    for s in vc.LONG_STEPS:
        Z[2, lay.dt_off] = s / n2[2]
        if vc.top_term_weight(lay, G0, Gj, Z) >= SEEN:
            long_step = s
            break
    assert long_step is not None, name
    Z[:, lay.dt_off + 1] = np.cumsum(Z[:, lay.dt_off])
    G0 = system(name, drift)[0]
    for a in (G0, Gj, Z):
        a.setflags(write=False)
    return lay, G0, Gj, Z, long_step


def residual_labels(lay):
    return vc.residual_labels(lay)


# ---- the truth (vector_shape_cases.truth_values), computed once per case and order and never written to ------------------------------------
@functools.lru_cache(maxsize=None)
def truth_ld(name, order, seed=0, drift=0):
    """(delta, Jacobian values), flat, in longdouble."""
    lay, G0, Gj, Z, _ = case(name, seed, drift)
    d, j, _ = vc.truth_values(lay, G0, Gj, Z, None, order, hessian=False)
    out = (d.reshape(-1), j.reshape(-1))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def truth(name, order, seed=0, drift=0):
    """The same rounded to float64: what the GPU tests compare with."""
    out = tuple(a.astype(np.float64) for a in truth_ld(name, order, seed, drift))
    for a in out:
        a.setflags(write=False)
    return out


# ---- faults, through the truth's `mm` hook ------------------------------------------------------------------------------------------------------
def mm_drop_k_beyond_64(n):
    """Every product with the left operand's columns from 64 on (per n x n block) read as zero: the k-steps the kernels of n <= 64 never had."""

    def mm(A, B):
        A = np.array(A)
        A[:, np.arange(A.shape[1]) % n >= 64] = 0
        return A @ B

    return mm


def mm_zero_last_row_tile(n):
    """Every product with the rows of the last 16-row tile of its output (per block of n rows) left at zero."""
    r0 = 16 * ((n - 1) // 16)

    def mm(A, B):
        Cm = A @ B
        Cm[np.arange(Cm.shape[0]) % n >= r0] = 0
        return Cm

    return mm
