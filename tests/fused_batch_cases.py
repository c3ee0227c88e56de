"""Cases that walk the pattern-compiled fused kernel (pcl_kernel_fused_sparse.hpp, last_kernel 40 + q) through its launches of SEVERAL trajectories
-- several items per workgroup with the rotating ring of power tiles, contiguous column ranges, groups of workgroups with slice tickets -- and the
column-group Hessian through its R-chain rule, at sizes other than BASELINE config 3; importable without a GPU.

Knot [X | dt | t | u] (the ensemble B7: [X_0 | X_1 | X_2 | dt | t | u], the members share the knots), u ~ 0.4 N(0, 1), X ~ 0.4 N(0, 1).  The step of
interval k of seed s is fixed from |G(u_k)|_2: h |G|_2 = STEPS[(k + s) % 4] with unitary4_cases.STEPS = 0.15, -0.3, 0 exactly, 0.5 -- so a group's
consecutive visits (interval + groups) meet different steps.  No step had to be widened: at every order the neighbouring order moves delta and the
Jacobian values of EVERY interval with a step by more than 1e4 x the tolerance (tests/test_fused_batch_cpu.py asserts it; the smallest read is 1.7e-4:
the orders differ from c_2 on).  At h = 0 the d/du tails are identically zero and must be read as exact zeros.

Systems: shape_cases.plain_system S1 .. S5, unitary4_cases.system("U17"), and the per-member-drift construction of
tests/test_general_shapes_gpu.py::test_per_member_drifts_streamed_classes -- what kernel 4 is known to take.

K = N - 1 intervals per trajectory, N = 6 (B2: N = 4).  `intervals` below is at 256 CUs; every count follows the device's n_cu (seeds(name, n_cu)).
case  system (d, m)            orders  seeds x K   what it straddles (every claim recomputed by the CPU module from the launch arithmetic restated below)
B1    S1 (9, 1)                2, 10   52 x 5      260 intervals, just above n_cu: the round-robin split walks two items in four workgroups; a ticket grid of n_cu
                                                   workgroups.  v4_group n_cu: ONE group of 260 visits -- refills 0 .. 4 of the controls ring, every slot rewritten
                                                   twice -- and 3 slices per interval (4, 4, 1 columns) for 256 workgroups: almost every visit finds its interval
                                                   exhausted.  v4_group 8: 32 groups of 9 or 8 visits.  v4_group 1: 256 groups of 2 or 1.  Window (1, 25): 125
                                                   intervals on 250 workgroups, v4_group 1: half the groups have no interval, their loaders still take chain tickets.
                                                   Order 2: np = 2 under tickets, a ONE-tile ring under the static multi-item splits.  Order 10: ring of 4 with
                                                   q - v4_np = m = 1 borrowed tile; v4_power_tiles 2 makes q - v4_np = 3 > m: the rule adds flag 4.
                                                   (moved from the issue's 41 seeds = 205 intervals: a launch of fewer slices than CUs has a grid of 205
                                                   workgroups, and v4_group n_cu then left the kernel with gridDim.x / tick_G = 0 groups -- see ticket_ok)
B2    U17 (13, 2)              4       184 x 3     both sides of bk d >= 28 n_cu: 552 intervals and, by the window (0, 183), 549 (K = 3 divides neither 551 nor the
                                                   threshold: the nearest counts either side).  v4_ticket 0: round-robin with S = 1 below, contiguous ranges above;
                                                   v4_ticket -1 with v4_tune 0: last_v4_ticket 0 below, 4 above.  Ranges begin mid-interval and cross trajectories.
B3    S2 (13, 4)               6       8 x 5       16 (drive, magnitude) pairs, 8 magnitudes.  v4_ticket_cols 1, 4, 5, 13: 13, 4, 3, 1 slices; a last slice of one column
B4    S3 (20, 3)               8       8 x 5       streamed drift classes: no cooperative first item in the module (SP4_COOP 0).  Tickets and both static splits
B5    S5 (32, 2)               4, 10   8 x 5       every lane of a half wave.  v4_ticket_cols 1: 32 slices > 31, tick_cpi raised to 2.  Order 10: np = 3 < q, ticket LDS
                                                   158,144 B of 163,840; static multi-item: ring of 3 with q - v4_np = m = 2 borrowed tiles.  v4_group 16 on a grid
                                                   of 240 workgroups: 15 groups of 3 or 2 visits (the issue's 16 groups need a grid of n_cu: 40 intervals give 240)
B6    S4 (31, 4)               10      4 x 5       np = 2.  ticket_ok false by LDS (156,432 + 8192 B): v4_ticket 1 runs the static split, last_v4_ticket 0.  Static
                                                   multi-item: ring of 2 with three borrowed tiles.  Odd d under contiguous ranges
B7    ensemble (20, 3), M = 3  4       3 x 5       PCL_BATCH_MEMBERS, per-member drifts (g0_batch_stride != 0) under tickets; the reduce payload by the writer wave of
                                                   whichever workgroup takes the chain ticket, for v4_ticket 0, 1, -1 (-1: static, 15 intervals are below the threshold)
H1    U17 (13, 2), Hessian     8       205 x 5     column-group Hessian (cpw = 10, ng = 2, last group 3 columns): 1025 intervals, items ng just above 8 n_cu: R-chain
                                                   waves (last_hess_rpre 1), 1025 not a multiple of 8: the R-chain block count is padded; window (0, 204): 1020, at the
                                                   threshold: none
B3 .. B7 have a ticket grid below n_cu at 256 CUs (B3, B4: 200 workgroups, B5: 240, B7: 150) and so has every window of B1 and B2 below n_cu intervals:
v4_group n_cu is refused there (ticket_ok: the grid holds no whole group) and the static split runs -- last_v4_ticket 0, the same bits.  Their reference
launch (round-robin, one slice per workgroup) is the one-item module's; the general module's several items per workgroup come with contiguous 1 and grid 7.

The truth is vector_shape_cases.truth_values (np.longdouble, general order, no code shared with oracle/pade_oracle.py), rounded to float64."""
import functools

import numpy as np

import shape_cases as sc
import unitary4_cases as uc
import vector_shape_cases as vc
from oracle import pade_oracle as po

TOL = 1e-11
SEEN = 1e-7
LD = np.longdouble
STEPS = uc.STEPS
LDS_BYTES = uc.LDS_BYTES
UHR_SLOTS = 128  # SP4_UHR: visits whose controls and step the dispatcher keeps in LDS
UHR_REFILL = 64  # visits per refill
TICKET_RING_BYTES = 8 * 8 * UHR_SLOTS

# name: (system, orders, knots, members)
CASES = {
    "B1": ("S1", (2, 10), 6, 1), "B2": ("U17", (4,), 4, 1), "B3": ("S2", (6,), 6, 1), "B4": ("S3", (8,), 6, 1), "B5": ("S5", (4, 10), 6, 1),
    "B6": ("S4", (10,), 6, 1), "B7": ("ensemble", (4,), 6, 3), "H1": ("U17", (8,), 6, 1),
}  # fmt: skip
FUSED = ("B1", "B2", "B3", "B4", "B5", "B6")  # the PCL_BATCH_TRAJ launches of the fused kernel
TICKET_COLS = {"B1": (4,), "B2": (3,), "B3": (1, 4, 5, 13), "B4": (7,), "B5": (1, 5), "B6": (1,), "B7": (3,)}
# member windows (first, count) beyond (1, B - 2); None: the count is computed from n_cu (windows())
EXTRA_WINDOWS = {"B1": ((1, 25),), "B2": ((0, None),)}


def dims(name):
    G0, Gj = system(name)
    return Gj.shape[1] // 2, len(Gj)


def hess_groups(d, m):
    """launch_hess_cols: (state columns per wave, column groups)."""
    cpw = 32 // (m + 1)
    return cpw, -(-d // cpw)


def seeds(name, n_cu):
    """Trajectories of the case's PCL_BATCH_TRAJ launch on a device of n_cu CUs."""
    d, m = dims(name)
    K = CASES[name][2] - 1
    if name == "B1":  # just above n_cu intervals
        return n_cu // K + 1
    if name == "B2":  # the first count at or above the contiguous threshold
        return -(-28 * n_cu // (d * K))
    if name == "H1":  # the first count with items ng > 8 n_cu -- and not a multiple of 8 intervals
        B = (8 * n_cu // hess_groups(d, m)[1]) // K + 1
        return B if (B * K) % 8 else B + 1
    return {"B3": 8, "B4": 8, "B5": 8, "B6": 4}[name]


def windows(name, n_cu):
    """The member windows the GPU module launches after the full one: (1, B - 2) and the case's own."""
    B = CASES[name][3] if name == "B7" else seeds(name, n_cu)
    out = [(1, B - 2)]
    for first, count in EXTRA_WINDOWS.get(name, ()):
        out.append((first, B - 1 if count is None else count))
    return out


# ---- systems, layouts, trajectories ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def system(name):
    """(G0, Gj), read-only; G0 is [M, n, n] for the ensemble."""
    s = CASES[name][0]
    if s == "U17":
        return uc.system("U17")
    if s == "ensemble":  # test_general_shapes_gpu.py::test_per_member_drifts_streamed_classes
        H0, Hd = sc.controlled_hermitians(20, [[0, 1], [2], [0, 3]], np.random.default_rng(7003), "continuous")
        Gj = np.array([po.G_of_H(H) for H in Hd])
        rng = np.random.default_rng(33)
        G0s = []
        for _ in range(3):
            R = 1 + 0.05 * rng.standard_normal(H0.shape)
            G0s.append(po.G_of_H(H0 * (R + R.T) / 2))  # the same pattern, every member's values its own
        G0 = np.array(G0s)
    else:
        G0, Gj = sc.plain_system(s)
    for a in (G0, Gj):
        a.setflags(write=False)
    return G0, Gj


def member_G0(name, member=0):
    G0 = system(name)[0]
    return G0[member] if G0.ndim == 3 else G0


def layout(name):
    d, m = dims(name)
    _, _, n_knots, M = CASES[name]
    xs = M * 2 * d * d
    return po.Layout(d=d, m=m, N=n_knots, z_dim=xs + 2 + m, x_off=0, u_off=xs + 2, dt_off=xs)


def x_offs(name):
    lay = layout(name)
    return [i * lay.x_dim for i in range(CASES[name][3])]


def _seed(name):
    return 52000 + 101 * list(CASES).index(name)


def step_class(k, seed):
    return (k + seed) % len(STEPS)


@functools.lru_cache(maxsize=None)
def trajectory(name, seed=0):
    """Z [N, z_dim], read-only: seed s of the case's launch."""
    lay = layout(name)
    Gj, G0 = system(name)[1], member_G0(name)
    Z = 0.4 * np.random.default_rng(_seed(name) + 7 * seed).standard_normal((lay.N, lay.z_dim))
    for k in range(lay.K):
        th = STEPS[step_class(k, seed)]
        Z[k, lay.dt_off] = th / np.linalg.norm(uc.g_of(lay, Z, k, G0, Gj), 2) if th else 0.0
    Z[lay.N - 1, lay.dt_off] = 0.1
    Z[:, lay.dt_off + 1] = np.cumsum(Z[:, lay.dt_off])
    Z.setflags(write=False)
    return Z


def rand_mu(name, seed=0):
    lay = layout(name)
    return np.random.default_rng(_seed(name) + 50000 + seed).standard_normal(lay.K * lay.x_dim)


def labels(name):
    lay = layout(name)
    return uc.residual_labels(lay), sc.jac_labels(lay), sc.hess_labels(lay)


def _ro(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


# ---- the truth --------------------------------------------------------------------------------------------------------------------------------------
def truth_one(name, order, seed=0, member=0, hessian=False, Z=None, intervals=None):
    """(delta, Jacobian values, mu | None, Hessian values | None) of one trajectory (one member) in longdouble, flat."""
    lay, Gj = layout(name), system(name)[1]
    mu = rand_mu(name, seed) if hessian else None
    Z = trajectory(name, seed) if Z is None else Z
    d, j, h = vc.truth_values(lay, member_G0(name, member), Gj, Z, mu, order, x_off=x_offs(name)[member], hessian=hessian, intervals=intervals)
    return d.reshape(-1), j.reshape(-1), mu, (None if h is None else h.reshape(-1))


@functools.lru_cache(maxsize=4)
def batch_truth(name, order, B, hessian=False):
    """(Z [B, N, z_dim], delta [B, ..], Jacobian values [B, ..], mu [B, ..] | None, Hessian values [B, ..] | None) of the first B seeds in float64,
    computed once and read-only.  The ensemble: Z [N, z_dim] and one row per member."""
    rows = []
    if name == "B7":
        Zs = trajectory(name)
        for i in range(CASES[name][3]):
            rows.append(truth_one(name, order, member=i))
    else:
        Zs = np.stack([trajectory(name, s) for s in range(B)])
        for s in range(B):
            rows.append(truth_one(name, order, s, hessian=hessian))
    f64 = lambda i: np.stack([r[i].astype(np.float64) for r in rows])
    return _ro(Zs, f64(0), f64(1), f64(2) if hessian else None, f64(3) if hessian else None)


def payload_ld(name, deltas, vals):
    """[phi | J' delta on u | on dt] of the ensemble in longdouble from the members' (delta, full Jacobian values): phi = 1/2 sum |delta|^2, the
    gradient entries the tail vectors' dot products with delta, summed over the state columns and the members."""
    lay = layout(name)
    K, C, n, m = lay.K, lay.C, lay.n, lay.m
    per = po.jac_nnz_per_interval(lay)
    gu, gdt, phi = np.zeros((K, m), LD), np.zeros(K, LD), LD(0)
    for dl, vl in zip(deltas, vals):
        dl = np.asarray(dl, LD).reshape(K, C, n)
        tail = np.asarray(vl, LD).reshape(K, per)[:, 2 * C * n * n :].reshape(K, C, m + 1, n)
        g = np.einsum("kcli,kci->kl", tail, dl)
        gu += g[:, :m]
        gdt += g[:, m]
        phi += LD(0.5) * np.einsum("kci,kci->", dl, dl)
    return np.concatenate([[phi], gu.reshape(-1), gdt])


def payload_labels(name):
    lay = layout(name)
    return np.array(["phi"] + ["gu@%d" % k for k in range(lay.K) for _ in range(lay.m)] + ["gdt@%d" % k for k in range(lay.K)])


# ---- the launch code's arithmetic (pcl_host_launch_pade.hpp launch_fused_v4; pcl_kernel_fused_sparse.hpp) -----------------------------------------------
v4_lds_bytes = uc.v4_lds_bytes
v4_power_tiles = uc.v4_power_tiles


def tick_group(n_cu, v4_group=0):
    return max(1, min(v4_group if v4_group > 0 else 8, n_cu))


def round_robin(bk, d, n_cu, cols_per_slice=0):
    """(state columns per slice, slices per interval, work items) of the round-robin split."""
    S0 = max(1, min(d, n_cu // max(bk, 1)))
    nc = min(cols_per_slice, d) if cols_per_slice > 0 else -(-d // S0)
    S = -(-d // nc)
    return nc, S, bk * S


def contiguous_auto(bk, d, n_cu, compact=False):
    return (not compact) and bk * d >= 28 * n_cu


def ticket_grid(bk, d, n_cu, cols_per_slice=0):
    """Workgroups of a ticket launch: the round-robin split's work items, at most one per CU."""
    return min(round_robin(bk, d, n_cu, cols_per_slice)[2], n_cu)


def ticket_ok(d, m, q, bk, n_cu, v4_group=0, grid=0, compact=False, cols_per_slice=0):
    """m + 10 waves, groups that divide n_cu, a grid that holds one whole group, the tiles and the dispatcher's ring within the LDS, no grid option, full values."""
    G = tick_group(n_cu, v4_group)
    return (grid <= 0 and not compact and m + 10 <= 16 and n_cu % G == 0 and ticket_grid(bk, d, n_cu, cols_per_slice) >= G
            and v4_lds_bytes(d, m, v4_power_tiles(d, m, q)) + TICKET_RING_BYTES <= LDS_BYTES)  # fmt: skip


def tick_cpi(d, v4_ticket_cols=0):
    """State columns per slice ticket: the slice index travels in five bits."""
    cpi = min(v4_ticket_cols, d) if v4_ticket_cols > 0 else min(4, d)
    while -(-d // cpi) > 31:
        cpi += 1
    return cpi


def launch(d, m, q, bk, n_cu, v4_ticket=-1, v4_tune=0, contiguous=-1, grid=0, cols_per_slice=0, v4_group=0, v4_ticket_cols=0, v4_power_tiles=0, v4_flags=0,
           v4_tail_mode=3, merit=False, coop=True, **ignored):  # fmt: skip
    """launch_fused_v4 for full values: what the launch reads back (ticket = last_v4_ticket, one_item = last_v4_one_item) and what decides its paths
    (contig, nc, S, units, grid, v4_np, flags, lds, groups, and the power tiles the cooperative first item borrows from the chains; coop: the module has
    a cooperative first item -- fully resident drift classes).  `auto` tickets are modelled under v4_tune 0 (with v4_tune 1 the context times both)."""
    np_ = uc.v4_power_tiles(d, m, q)
    assert np_ > 0
    contig = 0 if cols_per_slice > 0 else (contiguous if contiguous >= 0 else int(contiguous_auto(bk, d, n_cu)))
    ok = ticket_ok(d, m, q, bk, n_cu, v4_group, grid, False, cols_per_slice)
    auto = ok and v4_ticket < 0 and q <= 2 and contig and contiguous < 0 and cols_per_slice <= 0
    assert not (auto and v4_tune), "the timed choice is not a rule"
    ticket = ok and (v4_ticket == 1 or auto)
    if ticket:
        contig = 0
    nc, S, units = (d, 1, bk * d) if contig else round_robin(bk, d, n_cu, cols_per_slice)
    g = min(grid, units) if grid > 0 else min(units, n_cu)
    v4_np = min(v4_power_tiles, np_) if v4_power_tiles > 0 else np_ if ticket else max(1, min(np_, q - 1)) if units > g else min(np_, q)
    flags = v4_flags | (4 if q >= 5 and v4_np < q and (q - v4_np > m or v4_flags & 16) else 0)
    tail = 0 if ticket and v4_tail_mode == 3 else v4_tail_mode
    one_item = not ticket and not contig and units == g and grid <= 0 and not merit and tail == 3 and flags == 0
    G = tick_group(n_cu, v4_group)
    return dict(ticket=tick_cpi(d, v4_ticket_cols) if ticket else 0, contig=contig, nc=nc, S=S, units=units, grid=g, v4_np=v4_np, flags=flags, tail=tail,
                one_item=int(one_item), lds=v4_lds_bytes(d, m, np_) + (TICKET_RING_BYTES if ticket else 0), np=np_, groups=g // G if ticket else 0,
                slices=-(-d // tick_cpi(d, v4_ticket_cols)) if ticket else 0,
                borrowed=q - v4_np if coop and not ticket and not flags & (4 | 16) and 0 < q - v4_np <= m else 0)  # fmt: skip


def group_visits(n_int, grid, G):
    """Visits per group of workgroups: group g walks the intervals g, g + groups, ...; the workgroups beyond the last whole group form one more."""
    n_groups = grid // G
    return [(-(-(n_int - grp) // n_groups) if grp < n_int else 0) for grp in range(-(-grid // G))]


def ring_refills(n_vis):
    return -(-n_vis // UHR_REFILL)


def ring_slot(visit):
    return visit % UHR_SLOTS


def group_values(n_cu):
    """The issue's v4_group values 1, 8, 16, n_cu -- each moved to the nearest divisor of n_cu where it is none."""
    divs = [g for g in range(1, n_cu + 1) if n_cu % g == 0]
    return sorted({min(divs, key=lambda g: (abs(g - v), g)) for v in (1, 8, 16, n_cu)})


def hess_rpre_auto(items, d, m, q, n_cu):
    """launch_hess_cols, hess_rpre -1: R-chain waves for launches of more column-group waves than the device has wave slots, from order 8 on."""
    return int(items * hess_groups(d, m)[1] > 8 * n_cu and q >= 4)


def rchain_blocks(items):
    return (items + 7) // 8 * 8


# ---- faults, applied to the truth alone -------------------------------------------------------------------------------------------------------------
def stale_ring_visit(name, order, visit, groups=1, grp=0):
    """The Jacobian values of the interval of `visit` formed with the controls and the step of the visit UHR_SLOTS earlier (a ring slot read before its
    refill), in float64."""
    lay = layout(name)
    K = lay.K
    iv, old = grp + visit * groups, grp + (visit - UHR_SLOTS) * groups
    Z = np.array(trajectory(name, iv // K)[iv % K : iv % K + 2])
    Zo = trajectory(name, old // K)[old % K]
    Z[0, lay.u_off : lay.u_off + lay.m] = Zo[lay.u_off : lay.u_off + lay.m]
    Z[0, lay.dt_off] = Zo[lay.dt_off]
    return truth_one(name, order, Z=Z, intervals=(0,))[1].astype(np.float64)


def swapped_slice(js, name, iv, other, c0, nce):
    """Interval iv's Jacobian values (js: [intervals, per interval]) with the -B+ and B- blocks of the state columns c0 .. c0 + nce - 1 taken from interval `other`."""
    lay = layout(name)
    nn, C = lay.n * lay.n, lay.C
    out = np.array(js[iv])
    for blk in (0, C * nn):
        out[blk + c0 * nn : blk + (c0 + nce) * nn] = js[other][blk + c0 * nn : blk + (c0 + nce) * nn]
    return out
