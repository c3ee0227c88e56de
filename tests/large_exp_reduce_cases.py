"""Cases for the option large_exp_reduce of a large exponential context (PCL_LARGE_N | PCL_LARGE_EXP, pade_order = PCL_ORDER_EXP, generator dimensions
66 .. 128): the compact Jacobian [-E (n n) | tails], its device expansion (pcl_exp_expand_large_kernel), the host-pointer calls' compact route and the
merit / reduce payload (the modes of piccolo.jl_amd/csrc/pcl_kernel_large_exp.hpp).  Importable without a GPU.

Systems, trajectories (N = 4; s' = 1, 3 and 21 .. 51 substeps per interval), the scipy truth and the float64 emulation are those of
tests/large_exp_cases.py (le.case, le.truth, le.emulate); nothing here writes into its tables.  Cases (kind, n, cols, m) and what each reaches:
    L1   iso  66  1  2   two parts per tile in the expansion; LE_MERIT with drive groups
    L1z  iso  66  1  2   L1 with h = 0 on interval 1: exact zero drive entries
    L3   iso 128  1  2   nine columns per buffer
    L4   iso 120  1 24   eight groups of three in the Jacobian plan, fewer in the payload-only plan
    L5   iso  72  5  4   members, weights, window
    L6   iso  66 33  1   three slices; a wave takes more than one job
    L7   vec  81  1  3   odd n: the expansion's scalar path; one column is not a copy (the ones lie between the tile and the tails)
    L9   vec 127  1  1   odd n, four parts
    X1   iso 128  3  2   NEW: the 8192-pair tile with replication; 3 (1 + 2) = 9 = NBW, so the payload-only plan takes both drives in one group
                         where the Jacobian plan, which keeps a column of E beside the chain, must split them
X1 takes the system of R1 in tests/large_reduce_cases.py (its drifts and drives, never written to) and a trajectory by large_exp_cases' rule: seed
25000 + 17 * 31 + the trajectory's seed, steps h |G|_1 = 0.8, -2.5 and 29.6.

The multipliers: lam = a standard normal of delta's shape [K, cols, n], seed 88000 + 17 * the case's number + 1000 per member / trajectory.

Truth.  compact_of_full takes each tile of the scipy truth once.  payload forms, in np.longdouble from per-member (delta, full values, lam):
    phi = sum_b w_b c <lam_b, delta_b>  (c = 1/2 when lam = delta),  g[k, l] = sum_b w_b <d delta_bk / d u_l, lam_bk>,  g[k, m] likewise for dt;
one output set [phi | g_u (K m, k-major) | g_dt (K)], and beside it the scale the tolerance multiplies, entry by entry: the Cauchy-Schwarz image
sum_b w_b |lam_bk|_2 |column_bk|_2 of "every segment within 1e-11 of its own size" (tests/exp_full_cases.py), and for phi
sum_bk w_b |lam_bk| |delta_bk| (half of it when lam = delta).  Entries whose scale is zero must be exact.  Its faults (keywords): the last state
column dropped, the last drive group dropped, a member's weight ignored, the factor 1/2 dropped, lam of the wrong interval.

`plan` restates large_exp_plan (pcl_host_launch_pade.hpp) with its payload-only case: the slices of the Jacobian plan; the drive-group size among
those with nc (1 + mg) <= NBW (large_exp_drives caps it) by tile passes x rounds of the grid, then the fewest passes, then the larger group;
U = sx ngrp, npc = 0, LDS = fixed + 3 LD nc (1 + mg) doubles.  TABLE: (U, sx, nc, ngrp, mg, npc, bytes) of the launch with values and of the
payload-only launch, three intervals on 256 CUs, for every case and every split the GPU tests force."""
import functools

import numpy as np

import exp_full_cases as xf
import exp_truth as xt
import large_exp_cases as le
import large_reduce_cases as rc
import vector_shape_cases as vc
from oracle import pade_oracle as po
from shape_cases import check_segments, per_interval  # noqa: F401  (re-exported for the two test files)

N = le.N
K = N - 1
LD = np.longdouble
TOL = 1e-11

NEW = {"X1": ("iso", 128, 3, 2)}
NAMES = ["L1", "L1z", "L3", "L4", "L5", "L6", "L7", "L9", "X1"]
LONG_X1 = 29.6


def _base(name):
    return name[:2]


CASES = {name: (NEW[name] if name in NEW else le.CASES[_base(name)]) for name in NAMES}


def _number(name):
    return 31 if name == "X1" else int(_base(name)[1:])


# ---- trajectories and the truth ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(name, seed=0, drift=0):
    """(layout, G0, Gj, Z), read-only: le.case for its cases; X1 by the same rule on the system of large_reduce_cases' R1."""
    if name not in NEW:
        return le.case(name, seed, drift)
    lay = rc.layout("R1")
    G0, Gj = rc._new_system("R1", 0)
    rng = np.random.default_rng(25000 + 17 * _number(name) + seed)
    Z = 0.4 * rng.standard_normal((N, lay.z_dim))
    n1 = [le.norm1(vc.g_of(lay, Z, k, G0, Gj)) for k in range(K)]
    Z[0, lay.dt_off], Z[1, lay.dt_off], Z[2, lay.dt_off], Z[N - 1, lay.dt_off] = le.STEPS[0] / n1[0], le.STEPS[1] / n1[1], LONG_X1 / n1[2], 0.1
    Z[:, lay.dt_off + 1] = np.cumsum(Z[:, lay.dt_off])
    G0 = rc._new_system("R1", drift)[0]
    Z.setflags(write=False)
    return lay, G0, Gj, Z


@functools.lru_cache(maxsize=None)
def truth(name, seed=0, drift=0):
    """(delta, full Jacobian values), flat, in the library's order: scipy expm / expm_frechet through the committed oracle."""
    if name not in NEW:
        return le.truth(name, seed, drift)
    lay, G0, Gj, Z = case(name, seed, drift)
    out = (po.exp_residual(Z, lay, G0, Gj).reshape(-1), xt.values(Z, lay, G0, Gj).reshape(-1))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def emulated(name, seed=0, drift=0):
    """(delta, full values) of the kernel's recurrence in float64 numpy (le.emulate), read-only."""
    out = le.emulate(*case(name, seed, drift))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def lam(name, member=0):
    kind, n, cols, m = CASES[name]
    a = np.random.default_rng(88000 + 17 * _number(name) + 1000 * member).standard_normal((K, cols, n))
    a.setflags(write=False)
    return a


# ---- sizes and the compact layout ----------------------------------------------------------------------------------------------------------------
full_per = xf.full_per
compact_per = xf.compact_per


def compact_of_full(vals, n, cols, m):
    """Flat: each interval's first copy of -E and its tails."""
    return xf.compact_of_full(vals, n, cols, m).reshape(-1)


def expand_compact(comp, n, cols, m):
    """Flat: cols copies of -E, x_dim ones, the tails."""
    return xf.expand_compact(comp, n, cols, m).reshape(-1)


def compact_labels(n, cols, m):
    tail = np.tile(np.repeat(np.array(["du%d" % l for l in range(m)] + ["dh"]), n), cols)
    return per_interval(np.concatenate([np.full(n * n, "-E"), tail]), K)


def payload_len(m):
    return 1 + K * m + K


# ---- the payload ---------------------------------------------------------------------------------------------------------------------------------
def payload(name, deltas, vals, lams, weights=None, *, drop_col=False, drop_group=0, ignore_weights=False, no_half=False, shift_lam=False):
    """(out, scale), each [1 + K m + K] in longdouble, from per-member (delta, full values, lam); lams None means lam = delta (c = 1/2).
    Faults: drop_col -- the last state column left out of every dot product; drop_group = mg -- the drives of the last group of mg left at zero;
    ignore_weights; no_half; shift_lam -- every interval reads the multipliers of the next one (cyclically)."""
    kind, n, cols, m = CASES[name]
    gu, gdt, phi = np.zeros((K, m), LD), np.zeros(K, LD), LD(0)
    su, sdt, sphi = np.zeros((K, m), LD), np.zeros(K, LD), LD(0)
    c = LD(1) if lams is not None or no_half else LD(0.5)
    for b, (dl, vl) in enumerate(zip(deltas, vals)):
        w = LD(1) if weights is None or ignore_weights else LD(weights[b])
        dl = np.asarray(dl, LD).reshape(K, cols, n)
        tail = np.asarray(vl, LD).reshape(K, full_per(n, cols, m))[:, cols * n * n + cols * n :].reshape(K, cols, m + 1, n)
        lm = dl if lams is None else np.asarray(lams[b], LD).reshape(K, cols, n)
        if shift_lam:
            lm = np.roll(lm, -1, axis=0)
        ce = cols - 1 if drop_col else cols
        g = np.einsum("kcli,kci->kl", tail[:, :ce], lm[:, :ce])
        if drop_group:
            g[:, ((m - 1) // drop_group) * drop_group : m] = 0
        s = np.sqrt((lm**2).sum(axis=(1, 2)))[:, None] * np.sqrt((tail**2).sum(axis=(1, 3)))
        gu += w * g[:, :m]
        gdt += w * g[:, m]
        su += w * s[:, :m]
        sdt += w * s[:, m]
        phi += w * c * np.einsum("kci,kci->", lm[:, :ce], dl[:, :ce])
        sphi += w * c * (np.sqrt((lm**2).sum(axis=(1, 2))) * np.sqrt((dl**2).sum(axis=(1, 2)))).sum()
    return np.concatenate([[phi], gu.reshape(-1), gdt]), np.concatenate([[sphi], su.reshape(-1), sdt])


def worst(out, want, scale):
    """max over the entries of |out - want| / scale; entries whose scale is zero must agree exactly."""
    err = np.abs(np.asarray(out, dtype=LD).reshape(want.shape) - want)
    assert not err[scale == 0].any(), "an entry of scale zero is not exact"
    return float((err[scale > 0] / scale[scale > 0]).max())


# ---- the launch code's arithmetic (large_exp_plan with its payload-only case) ------------------------------------------------------------------------
def plan(n, cols, m, payload_only=False, items=K, n_cu=256, cols_per_slice=0, slices=0, drives=0):
    p = le.plan(n, cols, m, jac=True, items=items, n_cu=n_cu, cols_per_slice=cols_per_slice, slices=slices, drives=drives)
    if not payload_only:
        return p
    nc, sx, NBW, ld = p["nc"], p["sx"], p["NBW"], p["LD"]
    fixed = ld * n + le.SLACK + m + 8
    mg, ngrp, U = 0, 1, sx
    if m > 0:
        mg_fit = max(1, min(m, NBW // nc - 1))
        if drives > 0:
            mg_fit = min(mg_fit, drives)
        best_t = best_p = -1
        for mg0 in range(mg_fit, 0, -1):
            g_ = -(-m // mg0)
            mg_ = -(-m // g_)
            U_ = sx * g_
            tiles, rounds = (nc * (1 + mg_) + 15) // 16, -(-max(items, 1) * U_ // n_cu)
            t, passes = tiles * rounds, tiles * U_
            if best_t < 0 or t < best_t or (t == best_t and passes < best_p):
                best_t, best_p, mg, ngrp, U = t, passes, mg_, g_, U_
    W = nc * (1 + mg)
    return dict(p, mg=mg, ngrp=ngrp, U=U, npc=0, W=W, bytes=(fixed + 3 * ld * W) * 8)


def passes(p, items=K, n_cu=256):
    """The plan's own count of a launch's time: 16-column tile passes per unit times the rounds of the grid over the CUs."""
    return ((p["W"] + 15) // 16) * -(-max(items, 1) * p["U"] // n_cu)


def splits(name):
    """(cols_per_slice, general_slices, large_exp_drives) the GPU tests force on the case: the default first."""
    kind, n, cols, m = CASES[name]
    out = [(0, 0, 0), (0, 7, 0)]
    if cols > 1:
        out += [(1, 0, 0), (2, n, 0)]
    if name in ("L4", "X1"):
        out += [(0, 0, g) for g in sorted({1, 2, m})]
    return out


def row(p):
    return (p["U"], p["sx"], p["nc"], p["ngrp"], p["mg"], p["npc"], p["bytes"])


# (case, cols_per_slice, general_slices, large_exp_drives): (with values, payload-only), each (U, sx, nc, ngrp, mg, npc, bytes)
TABLE = {
    ("L1", 0, 0, 0): ((5, 1, 1, 2, 1, 14, 62208), (1, 1, 1, 1, 2, 0, 41304)),
    ("L1", 0, 7, 0): ((7, 1, 1, 2, 1, 10, 55776), (1, 1, 1, 1, 2, 0, 41304)),
    ("L1z", 0, 0, 0): ((5, 1, 1, 2, 1, 14, 62208), (1, 1, 1, 1, 2, 0, 41304)),
    ("L1z", 0, 7, 0): ((7, 1, 1, 2, 1, 10, 55776), (1, 1, 1, 1, 2, 0, 41304)),
    ("L3", 0, 0, 0): ((19, 1, 1, 2, 1, 7, 161064), (1, 1, 1, 1, 2, 0, 142488)),
    ("L3", 0, 7, 0): ((19, 1, 1, 2, 1, 7, 161064), (1, 1, 1, 1, 2, 0, 142488)),
    ("L4", 0, 0, 0): ((11, 1, 1, 8, 3, 11, 161000), (2, 1, 1, 2, 12, 0, 155192)),
    ("L4", 0, 7, 0): ((11, 1, 1, 8, 3, 11, 161000), (2, 1, 1, 2, 12, 0, 155192)),
    ("L4", 0, 0, 1): ((24, 1, 1, 24, 1, 5, 137768), (24, 1, 1, 24, 1, 0, 123248)),
    ("L4", 0, 0, 2): ((12, 1, 1, 12, 2, 10, 155192), (12, 1, 1, 12, 2, 0, 126152)),
    ("L4", 0, 0, 24): ((11, 1, 1, 8, 3, 11, 161000), (2, 1, 1, 2, 12, 0, 155192)),
    ("L5", 0, 0, 0): ((12, 1, 5, 4, 1, 6, 71200), (2, 1, 5, 2, 2, 0, 69448)),
    ("L5", 0, 7, 0): ((12, 1, 5, 4, 1, 6, 71200), (2, 1, 5, 2, 2, 0, 69448)),
    ("L5", 1, 0, 0): ((7, 5, 1, 1, 4, 11, 71200), (5, 5, 1, 1, 4, 0, 51928)),
    ("L5", 2, 72, 0): ((72, 3, 2, 2, 2, 1, 55432), (3, 3, 2, 1, 4, 0, 60688)),
    ("L6", 0, 0, 0): ((7, 3, 11, 1, 1, 10, 87928), (3, 3, 11, 1, 1, 0, 71848)),
    ("L6", 0, 7, 0): ((7, 3, 11, 1, 1, 10, 87928), (3, 3, 11, 1, 1, 0, 71848)),
    ("L6", 1, 0, 0): ((33, 33, 1, 1, 1, 2, 42904), (33, 33, 1, 1, 1, 0, 39688)),
    ("L6", 2, 66, 0): ((66, 17, 2, 1, 1, 1, 44512), (17, 17, 2, 1, 1, 0, 42904)),
    ("L7", 0, 0, 0): ((6, 1, 1, 3, 1, 14, 84704), (1, 1, 1, 1, 3, 0, 61376)),
    ("L7", 0, 7, 0): ((7, 1, 1, 3, 1, 12, 80816), (1, 1, 1, 1, 3, 0, 61376)),
    ("L9", 0, 0, 0): ((15, 1, 1, 1, 1, 9, 163656), (1, 1, 1, 1, 1, 0, 136224)),
    ("L9", 0, 7, 0): ((15, 1, 1, 1, 1, 9, 163656), (1, 1, 1, 1, 1, 0, 136224)),
    ("X1", 0, 0, 0): ((43, 1, 3, 2, 1, 3, 161064), (1, 1, 3, 1, 2, 0, 161064)),
    ("X1", 0, 7, 0): ((43, 1, 3, 2, 1, 3, 161064), (1, 1, 3, 1, 2, 0, 161064)),
    ("X1", 1, 0, 0): ((19, 3, 1, 2, 1, 7, 161064), (3, 3, 1, 1, 2, 0, 142488)),
    ("X1", 2, 128, 0): ((128, 2, 2, 2, 1, 1, 148680), (2, 2, 2, 1, 2, 0, 151776)),
    ("X1", 0, 0, 1): ((43, 1, 3, 2, 1, 3, 161064), (2, 1, 3, 2, 1, 0, 151776)),
    ("X1", 0, 0, 2): ((43, 1, 3, 2, 1, 3, 161064), (1, 1, 3, 1, 2, 0, 161064)),
}  # fmt: skip
