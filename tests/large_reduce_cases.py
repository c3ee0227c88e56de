"""Cases for the option large_reduce of a large context (PCL_LARGE_N, generator dimensions 66 .. 128): the compact Jacobian, its device expansion, the
host-pointer calls' compact route and the merit / reduce payload (the modes of piccolo.jl_amd/csrc/pcl_kernel_pade_large.hpp, pcl_expand_large_kernel
in pcl_kernels_misc.hpp).  Importable without a GPU.

Systems, trajectories (N = 4, three intervals) and the longdouble truth are those of tests/large_shape_cases.py (lc.case, lc.truth_ld); nothing here
writes into its tables.  Cases (kind, n, cols, m) and what each is for:
    L1  iso  66  1  2   one column: the compact layout IS the full layout
    L4  iso 120  1 24   two drive groups: the payload's entries of one column come from two units
    L5  iso  72  5  4   multi-ket: cols_per_slice = 2 gives slices of 2, 2, 1
    L6  iso  66 33  1   unitary d = 33: two slices (17 and 16 columns), 33 copies of each tile in the expansion
    L7  vec  81  1  3   odd n under PCL_STATE_VECTOR
    R1  iso 128  3  2   NEW: the largest tile with replication -- 8192 element pairs per tile in the expansion, four workgroups of 2048 -- and
                        3 (2 + 2 (2 + 2)) = 30 chain blocks against NB = 29, so the plan splits the drives: two groups of one drive
R1 is built by the recipe of lc.system / lc.case with a seed of its own (15000 + 17 * 31).

The multipliers: lam = a standard normal of delta's shape, seed 77000 + the case's seed (and + 1000 per member / trajectory of a batched launch).

Truth.  compact_of(values) takes each tile of the longdouble Jacobian truth once.  payload_ld forms, in np.longdouble from the longdouble delta and tail
values,  phi = sum_b w_b c <lam_b, delta_b>  (c = 1/2 when lam = delta),  g[k, l] = sum_b w_b <d delta_bk / d u_l, lam_bk>,  g[k, m] likewise for dt;
one output set [phi | g_u (K m, k-major) | g_dt (K)] (PCL_BATCH_TRAJ: one per trajectory).  Its faults (payload_ld's keywords): the last state column
dropped, the last drive group dropped, a member's weight ignored, the factor 1/2 dropped, lam of the wrong interval.

TABLE: what the launch code's plan (large_plan in pcl_host_launch_pade.hpp, restated in reduce_plan below with its payload-only case: the same
chain units and nothing else, U = sx ngrp, npc = 0) gives for every case and every split the GPU tests force, as (U, sx, ngrp, mg, npc, bytes) for
the launch with values and for the payload-only launch.  tests/test_large_reduce_cpu.py asserts every row."""
import functools

import numpy as np

import large_shape_cases as lc
import vector_shape_cases as vc
from oracle import pade_oracle as po
from shape_cases import check_segments, jac_labels, per_interval  # noqa: F401  (re-exported for the two test files)

N = lc.N
ORDERS_COMPACT = (2, 6, 10)
ORDERS_PAYLOAD = (4, 10)
LD = np.longdouble

NEW = {"R1": ("iso", 128, 3, 2)}
NAMES = ["L1", "L4", "L5", "L6", "L7", "R1"]
CASES = {name: (lc.CASES[name] if name in lc.CASES else NEW[name]) for name in NAMES}


def _seed(name):
    return 15000 + 17 * (31 if name == "R1" else int(name[1:]))


# ---- R1, by the recipe of lc.system / lc.case ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _new_system(name, drift=0):
    kind, n, cols, m = NEW[name]
    rng = np.random.default_rng(_seed(name))
    G0s = [po.G_of_H(vc._herm(n // 2, rng)) for _ in range(3)]
    Gj = np.array([po.G_of_H(vc._herm(n // 2, rng)) for _ in range(m)])
    return G0s[drift], Gj


def layout(name):
    if name in lc.CASES:
        return lc.layout(name)
    kind, n, cols, m = NEW[name]
    xs = n * cols
    return po.Layout(d=n // 2, m=m, N=N, z_dim=xs + 2 + m, x_off=0, u_off=xs + 2, dt_off=xs, cols=cols)


@functools.lru_cache(maxsize=None)
def case(name, seed=0, drift=0):
    """(layout, G0, Gj, Z, long step), read-only: lc.case for its cases, the same recipe for R1."""
    if name in lc.CASES:
        return lc.case(name, seed, drift)
    lay = layout(name)
    G0, Gj = _new_system(name, 0)
    rng = np.random.default_rng(_seed(name) + 1 + seed)
    Z = 0.4 * rng.standard_normal((N, lay.z_dim))
    n2 = [np.linalg.norm(vc.g_of(lay, Z, k, G0, Gj), 2) for k in range(N - 1)]
    Z[0, lay.dt_off], Z[1, lay.dt_off], Z[N - 1, lay.dt_off] = 0.15 / n2[0], -0.3 / n2[1], 0.1
    long_step = None
    for s in vc.LONG_STEPS:
        Z[2, lay.dt_off] = s / n2[2]
        if vc.top_term_weight(lay, G0, Gj, Z) >= lc.SEEN:
            long_step = s
            break
    assert long_step is not None, name
    Z[:, lay.dt_off + 1] = np.cumsum(Z[:, lay.dt_off])
    G0 = _new_system(name, drift)[0]
    for a in (G0, Gj, Z):
        a.setflags(write=False)
    return lay, G0, Gj, Z, long_step


@functools.lru_cache(maxsize=None)
def truth_ld(name, order, seed=0, drift=0):
    """(delta, full Jacobian values), flat, in longdouble, read-only."""
    if name in lc.CASES:
        return lc.truth_ld(name, order, seed, drift)
    lay, G0, Gj, Z, _ = case(name, seed, drift)
    d, j, _ = vc.truth_values(lay, G0, Gj, Z, None, order, hessian=False)
    out = (d.reshape(-1), j.reshape(-1))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def truth(name, order, seed=0, drift=0):
    """The same rounded to float64."""
    out = tuple(a.astype(np.float64) for a in truth_ld(name, order, seed, drift))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def lam(name, member=0):
    """The multipliers of one member / trajectory: a standard normal of delta's shape [K, cols, n]."""
    kind, n, cols, m = CASES[name]
    a = np.random.default_rng(77000 + _seed(name) + 1000 * member).standard_normal((N - 1, cols, n))
    a.setflags(write=False)
    return a


# ---- sizes and the compact layout -----------------------------------------------------------------------------------------------------------------
def full_per(n, cols, m):
    return 2 * cols * n * n + n * cols * (m + 1)


def compact_per(n, cols, m):
    return 2 * n * n + n * cols * (m + 1)


def compact_of(vals, n, cols, m):
    """Each tile of the full values once: [-B+ (n n) | B- (n n) | tails] per interval."""
    nn = n * n
    v = np.asarray(vals).reshape(-1, full_per(n, cols, m))
    return np.concatenate([v[:, :nn], v[:, cols * nn : cols * nn + nn], v[:, 2 * cols * nn :]], axis=1).reshape(-1)


def compact_labels(n, cols, m, K=N - 1):
    tail = np.tile(np.repeat(np.array(["du"] * m + ["dh"]), n), cols)
    return per_interval(np.concatenate([np.full(n * n, "B+"), np.full(n * n, "B-"), tail]), K)


def payload_len(m, K=N - 1):
    return 1 + K * m + K


def payload_labels(m, K=N - 1):
    return np.array(["phi"] + ["gu"] * (K * m) + ["gdt"] * K)


# ---- the payload ----------------------------------------------------------------------------------------------------------------------------------
def payload_ld(name, deltas, vals, lams, weights=None, *, drop_col=False, drop_group=0, ignore_weights=False, no_half=False, shift_lam=False):
    """One output set [phi | g_u | g_dt] in longdouble from per-member (delta, full values, lam): lam None means lam = delta (c = 1/2).
    Faults: drop_col -- the last state column left out of every dot product; drop_group = mg -- the drives of the last group of mg left at zero;
    ignore_weights; no_half; shift_lam -- every interval reads the multipliers of the next one (cyclically)."""
    kind, n, cols, m = CASES[name] if isinstance(name, str) else name  # (or the sizes themselves: ("iso", n, cols, m))
    K = N - 1
    gu, gdt, phi = np.zeros((K, m), LD), np.zeros(K, LD), LD(0)
    for b, (dl, vl) in enumerate(zip(deltas, vals)):
        w = LD(1) if weights is None or ignore_weights else LD(weights[b])
        dl = np.asarray(dl, LD).reshape(K, cols, n)
        tail = np.asarray(vl, LD).reshape(K, full_per(n, cols, m))[:, 2 * cols * n * n :].reshape(K, cols, m + 1, n)
        lm = dl if lams is None else np.asarray(lams[b], LD).reshape(K, cols, n)
        if shift_lam:
            lm = np.roll(lm, -1, axis=0)
        ce = cols - 1 if drop_col else cols
        g = np.einsum("kcli,kci->kl", tail[:, :ce], lm[:, :ce])
        if drop_group:
            g[:, ((m - 1) // drop_group) * drop_group : m] = 0
        gu += w * g[:, :m]
        gdt += w * g[:, m]
        phi += w * (LD(1) if lams is not None or no_half else LD(0.5)) * np.einsum("kci,kci->", lm[:, :ce], dl[:, :ce])
    return np.concatenate([[phi], gu.reshape(-1), gdt])


# ---- the launch code's arithmetic (large_plan with its payload-only case) ---------------------------------------------------------------------------
def reduce_plan(n, cols, m, payload_only=False, items=N - 1, n_cu=256, cols_per_slice=0, slices=0):
    """lc.large_plan's statement of the Jacobian launch's plan; payload_only: the chain units alone -- U = sx ngrp, npc = 0, no P' block."""
    p = lc.large_plan(n, cols, m, jac=True, items=items, n_cu=n_cu, cols_per_slice=cols_per_slice, slices=slices)
    if payload_only:
        fixed = p["LD"] * n + lc.SLACK + m + 8
        p = dict(p, U=p["sx"] * p["ngrp"], npc=0, bytes=(fixed + p["LD"] * p["chain_blocks"]) * 8, pairs=0, npce=[])
    return p


def splits(name):
    """(cols_per_slice, general_slices) the GPU tests force on the case: the default first."""
    kind, n, cols, m = CASES[name]
    if cols == 1:
        return [(0, 0), (0, 7), (0, n)]
    return [(0, 0), (1, 0), (2, 0), (0, 7), (2, n)]


def row(p):
    return (p["U"], p["sx"], p["ngrp"], p["mg"], p["npc"], p["bytes"])


# (case, cols_per_slice, general_slices): (with values, payload-only), each (U, sx, ngrp, mg, npc, bytes), three intervals on 256 CUs
TABLE = {
    ("L1", 0, 0): ((5, 1, 1, 2, 14, 49344), (1, 1, 1, 2, 0, 41840)),
    ("L1", 0, 7): ((7, 1, 1, 2, 10, 47200), (1, 1, 1, 2, 0, 41840)),
    ("L1", 0, 66): ((66, 1, 1, 2, 1, 42376), (1, 1, 1, 2, 0, 41840)),
    ("L4", 0, 0): ((8, 1, 2, 12, 15, 161000), (2, 1, 2, 12, 0, 146480)),
    ("L4", 0, 7): ((8, 1, 2, 12, 15, 161000), (2, 1, 2, 12, 0, 146480)),
    ("L4", 0, 120): ((120, 1, 2, 12, 1, 147448), (2, 1, 2, 12, 0, 146480)),
    ("L5", 0, 0): ((5, 1, 1, 4, 15, 92808), (1, 1, 1, 4, 0, 84048)),
    ("L5", 1, 0): ((5, 5, 1, 4, 15, 60104), (5, 5, 1, 4, 0, 51344)),
    ("L5", 2, 0): ((5, 3, 1, 4, 15, 68280), (3, 3, 1, 4, 0, 59520)),
    ("L5", 0, 7): ((7, 1, 1, 4, 11, 90472), (1, 1, 1, 4, 0, 84048)),
    ("L5", 2, 72): ((72, 3, 1, 4, 1, 60104), (3, 3, 1, 4, 0, 59520)),
    ("L6", 0, 0): ((5, 2, 1, 1, 14, 116872), (2, 2, 1, 1, 0, 109368)),
    ("L6", 1, 0): ((33, 33, 1, 1, 2, 41832), (33, 33, 1, 1, 0, 40760)),
    ("L6", 2, 0): ((17, 17, 1, 1, 4, 47192), (17, 17, 1, 1, 0, 45048)),
    ("L6", 0, 7): ((7, 2, 1, 1, 10, 114728), (2, 2, 1, 1, 0, 109368)),
    ("L6", 2, 66): ((66, 17, 1, 1, 1, 45584), (17, 17, 1, 1, 0, 45048)),
    ("L7", 0, 0): ((6, 1, 1, 3, 14, 70448), (1, 1, 1, 3, 0, 61376)),
    ("L7", 0, 7): ((7, 1, 1, 3, 12, 69152), (1, 1, 1, 3, 0, 61376)),
    ("L7", 0, 81): ((81, 1, 1, 3, 1, 62024), (1, 1, 1, 3, 0, 61376)),
    ("R1", 0, 0): ((26, 1, 2, 1, 5, 163128), (2, 1, 2, 1, 0, 157968)),
    ("R1", 1, 0): ((8, 3, 1, 2, 16, 160032), (3, 3, 1, 2, 0, 143520)),
    ("R1", 2, 0): ((15, 2, 1, 2, 9, 163128), (2, 2, 1, 2, 0, 153840)),
    ("R1", 0, 7): ((26, 1, 2, 1, 5, 163128), (2, 1, 2, 1, 0, 157968)),
    ("R1", 2, 128): ((128, 2, 1, 2, 1, 154872), (2, 2, 1, 2, 0, 153840)),
}  # fmt: skip
