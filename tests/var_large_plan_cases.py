"""Cases that walk the large variational kernels (contexts created with PCL_BATCH_VARIATIONAL | PCL_LARGE_N | PCL_LARGE_VAR, generator dimensions
66 .. 128) over the regimes of their launch plans that the three- and four-interval launches of tests/var_large_cases.py and
tests/var_large_full_cases.py never enter: the residual + Jacobian kernel (piccolo.jl_amd/csrc/pcl_kernel_var_large.hpp, planned by var_large_plan
in pcl_host_variational.hpp, restated as vl.var_large_plan) and the rollout kernels of option large_var_full (pcl_kernel_var_large_rollout.hpp,
var_large_roll_plan in pcl_host_robust.hpp, restated as vf.roll_plan).  Numpy only, importable without a GPU; nothing here writes to the modules it
imports.

Both planners read the interval count and the CU count, and a variational context has one trajectory: a launch of few intervals on 256 CUs takes
narrow slices (want_sx = n_cu / (2 K ngrp)) and one rollout panel per 16 columns (n_cu / (K (1 + v))), whatever the options say.  So the regimes
below are entered by LONG launches.

Systems by the recipe of var_large_cases: G(H) of a dense complex Hermitian H / sqrt(d) for the drift, the drives and the variation generators
(the latter divided by the scales 3.0, 0.25); state and variation components 0.4 N(0, 1), u ~ 0.4 N(0, 1); seeds 18000 + 17 index (the system)
and + 1 (the knots).  R4 is vl.system("VL3") on vl.case("VL3")'s knots, VL2 is vl.case("VL2") (N = 5, odd offsets), R6 is vl.system("VL7").
Steps, h |Ghat(u_k)|_2 of the LIFTED generator: 0.15, -0.3, the long step (LONG below: the smallest of vector_shape_cases.LONG_STEPS at which
zeroing c_5 at order 10 moves the interval's residual by 1e-7 of its size), VL2's zero step, and on the wrap interval 0.2.

Cases (n, state columns C, v, m) and what each enters; the plan numbers (PLAN / ROLL below, at 256, 304 and 128 CUs) are literals that
tests/test_var_large_plan_cpu.py holds against the restated planners:
    R1   66  5 2  2   wide slices on the smallest multi-ket: 28 intervals nc 2 (2, 2, 1); 44: nc 3 (3, 2), 84,720 B; 88: nc 5, one slice, 150 of
                      237 blocks, 116,880 B (the residual alone takes the same widths); rollout at K >= 29: 2 panels of 33 columns, 142,608 B
    R2  100  5 2 15   slices crossed with groups, uneven groups, seven waves (448 threads, n mod 16 = 4): 3 intervals sx 5 x ngrp 2, drives
                      8 + 7, U 31 = 10 + 3 x 7, 66 of 101 blocks, 135,336 B
    R3  128  3 2  3   the same crossing at the tightest LDS, one drive per group: sx 3 x ngrp 3, U 54 = 9 + 3 x 15, 24 of 29 blocks, 161,072 B
    R4   96 48 1  4   the N = 100 plan of bench/bench_var_large.py: 10 intervals sx 12, nc 4, 112 of 113 blocks, 162,528 B, U 24; the residual
                      alone nc 4, 100,448 B
    R5  120 60 1  4   the other bench shape; 3 intervals, Jacobian: sx 60, nc 1, U 76, 160,840 B; 20 intervals, the residual alone: sx 10,
                      nc 6, 48 of 48 blocks, 163,744 B of 163,840
    R6  128 64 2  1   the largest state (vl.VL7's shape), RESIDUAL ONLY: sx 32, nc 2, 24 of 29 blocks, 157,960 B; its truth is delta alone, formed
                      block by block (delta_truth_ld below: the lifted Jacobian of 19 M longdouble values per interval is never built)
    R7   80  7 1  7   uneven wide slices: 20 intervals nc 2 (2, 2, 2, 1); 44 and 88: nc 4 (4, 3), 160 of 171 blocks, 156,664 B; the residual
                      alone at 88: nc 7; rollout at K = 29: 4 panels of 20 columns, 130,744 B; at K >= 44: 3 panels 27, 27, 26, 157,960 B
    VL2  66 33 2  3   wide slices on the unitary state with its odd knot offsets: 8 intervals nc 3 (11 slices); 20: nc 6 (6, 6, 6, 6, 6, 3),
                      152,264 B; the residual alone at 20: nc 6, 75,080 B; rollout at K = 29: 2 panels of 33 columns
Orders: 2 .. 10 on R1, R2 and R7; 4 and 10 on R3, R4, R5, R6 and VL2, whose truths cost more (TRUTH_SECONDS; the whole of
tests/test_var_large_plan_cpu.py stays under two minutes on one core, so R3 kept its order 10).

Long launches.  A variational context has one trajectory, so a long launch is a long trajectory: the case's P knots (4; VL2: 5) are CLOSED --
knot 0 appended after knot P - 1, the wrap interval's step at h |Ghat|_2 = 0.2 -- and continued periodically (`long_knots`), the time entry
with them (the kernels do not read it).  The truth is computed once, on the closed trajectory of P intervals, interval by interval (never more
than one interval's lifted values in longdouble at a time), and interval k of a long launch must equal interval k mod P of the closed launch bit
for bit.

Rollouts (ROLLS below): trajectories of 29 and 44 intervals by the rule of var_large_full_cases with small s' = ceil(|h| |G|_1): h |G|_1 =
+-0.8 alternating, interval 1 the long step (s' = LONG_SUB - 0.5 over |G|_1, LONG_SUB >= 20), interval 2 h = 0, interval 3 h |G|_1 = -2.5 (three
substeps); knot-0 sensitivities zero (seed 0) or 0.4 N(0, 1) (seed 1).  Truth: vf.rollout_truth_values in longdouble, once per trajectory.

Segments are those of var_large_cases.check (variational_shape_cases.residual_codes / jac_codes on vl.lib_structure: row component x variable
kind x relative knot x interval); `check` sorts one interval's codes once per case and applies them interval by interval --
tests/test_var_large_plan_cpu.py shows that it gives vsc.assert_segments' numbers and refuses what that refuses."""
import functools

import numpy as np

import var_large_cases as vl
import var_large_full_cases as vf
import variational_shape_cases as vsc
import variational_truth as vt
import vector_shape_cases as vs

LD_ = np.longdouble
LDS_BYTES = vl.LDS_BYTES
TOL = 1e-11
SEEN = vs.SEEN
WRAP_STEP = 0.2
CUS = (256, 304, 128)

# name: (n, C, v, m)
CASES = {"R1": (66, 5, 2, 2), "R2": (100, 5, 2, 15), "R3": (128, 3, 2, 3), "R4": (96, 48, 1, 4), "R5": (120, 60, 1, 4), "R6": (128, 64, 2, 1),
         "R7": (80, 7, 1, 7), "VL2": (66, 33, 2, 3)}  # fmt: skip
NAMES = list(CASES)
BORROWED = {"R4": "VL3", "R6": "VL7", "VL2": "VL2"}  # the systems of var_large_cases
RESIDUAL_ONLY = ("R6",)
JAC_NAMES = [nm for nm in NAMES if nm not in RESIDUAL_ONLY]
ORDERS = {name: (vs.ORDERS if name in ("R1", "R2", "R7") else (4, 10)) for name in NAMES}
NB = {"R1": 237, "R2": 101, "R3": 29, "R4": 113, "R5": 48, "R6": 29, "R7": 171, "VL2": 237}  # column blocks beside the tile
# the long step of interval 2, h |Ghat|_2: what long_step_search finds (tests/test_var_large_plan_cpu.py holds the weight at this step and, on the
# cheap cases, runs the search)
LONG = {"R1": 1.25, "R2": 0.8, "R3": 1.25, "R4": 0.65, "R5": 0.5, "R6": 1.25, "R7": 0.5, "VL2": 1.5}

# (case, intervals, CUs): (Jacobian launch, residual-only launch), each (sx, nc, columns of the last slice, ngrp, mg, drives of the last group, U,
# chain blocks, bytes): slices nc, .., nc, last and groups mg, .., mg, last
PLAN = {
    ("R1", 28, 256): ((3, 2, 1, 1, 2, 2, 18, 60, 68640), (3, 2, 1, 1, 0, 0, 3, 24, 49344)), ("R1", 28, 304): ((5, 1, 1, 1, 2, 2, 20, 30, 58992), (5, 1, 1, 1, 0, 0, 5, 12, 42912)), ("R1", 28, 128): ((2, 3, 2, 1, 2, 2, 17, 90, 84720), (2, 3, 2, 1, 0, 0, 2, 36, 55776)),
    ("R1", 44, 256): ((2, 3, 2, 1, 2, 2, 17, 90, 84720), (2, 3, 2, 1, 0, 0, 2, 36, 55776)), ("R1", 44, 304): ((3, 2, 1, 1, 2, 2, 18, 60, 68640), (3, 2, 1, 1, 0, 0, 3, 24, 49344)), ("R1", 44, 128): ((1, 5, 5, 1, 2, 2, 16, 150, 116880), (1, 5, 5, 1, 0, 0, 1, 60, 68640)),
    ("R1", 88, 256): ((1, 5, 5, 1, 2, 2, 16, 150, 116880), (1, 5, 5, 1, 0, 0, 1, 60, 68640)), ("R1", 88, 304): ((1, 5, 5, 1, 2, 2, 16, 150, 116880), (1, 5, 5, 1, 0, 0, 1, 60, 68640)), ("R1", 88, 128): ((1, 5, 5, 1, 2, 2, 16, 150, 116880), (1, 5, 5, 1, 0, 0, 1, 60, 68640)),
    ("R2", 3, 256): ((5, 1, 1, 2, 8, 7, 31, 66, 135336), (5, 1, 1, 1, 0, 0, 5, 12, 91704)), ("R2", 3, 304): ((5, 1, 1, 2, 8, 7, 31, 66, 135336), (5, 1, 1, 1, 0, 0, 5, 12, 91704)), ("R2", 3, 128): ((5, 1, 1, 2, 8, 7, 31, 66, 135336), (5, 1, 1, 1, 0, 0, 5, 12, 91704)),
    ("R3", 3, 256): ((3, 1, 1, 3, 1, 1, 54, 24, 161072), (3, 1, 1, 1, 0, 0, 3, 12, 145592)), ("R3", 3, 304): ((3, 1, 1, 3, 1, 1, 54, 24, 161072), (3, 1, 1, 1, 0, 0, 3, 12, 145592)), ("R3", 3, 128): ((3, 1, 1, 3, 1, 1, 54, 24, 161072), (3, 1, 1, 1, 0, 0, 3, 12, 145592)),
    ("R4", 10, 256): ((12, 4, 4, 1, 4, 4, 24, 112, 162528), (12, 4, 4, 1, 0, 0, 12, 32, 100448)), ("R4", 10, 304): ((12, 4, 4, 1, 4, 4, 24, 112, 162528), (12, 4, 4, 1, 0, 0, 12, 32, 100448)), ("R4", 10, 128): ((12, 4, 4, 1, 4, 4, 24, 112, 162528), (6, 8, 8, 1, 0, 0, 6, 64, 125280)),
    ("R5", 3, 256): ((60, 1, 1, 1, 4, 4, 76, 28, 160840), (30, 2, 2, 1, 0, 0, 30, 16, 132768)), ("R5", 3, 304): ((60, 1, 1, 1, 4, 4, 76, 28, 160840), (30, 2, 2, 1, 0, 0, 30, 16, 132768)), ("R5", 3, 128): ((60, 1, 1, 1, 4, 4, 76, 28, 160840), (20, 3, 3, 1, 0, 0, 20, 24, 140512)),
    ("R5", 20, 256): ((60, 1, 1, 1, 4, 4, 76, 28, 160840), (10, 6, 6, 1, 0, 0, 10, 48, 163744)), ("R5", 20, 304): ((60, 1, 1, 1, 4, 4, 76, 28, 160840), (10, 6, 6, 1, 0, 0, 10, 48, 163744)), ("R5", 20, 128): ((60, 1, 1, 1, 4, 4, 76, 28, 160840), (10, 6, 6, 1, 0, 0, 10, 48, 163744)),
    ("R6", 3, 256): ((64, 1, 1, 1, 1, 1, 109, 24, 161056), (32, 2, 2, 1, 0, 0, 32, 24, 157960)), ("R6", 3, 304): ((64, 1, 1, 1, 1, 1, 109, 24, 161056), (32, 2, 2, 1, 0, 0, 32, 24, 157960)), ("R6", 3, 128): ((64, 1, 1, 1, 1, 1, 109, 24, 161056), (32, 2, 2, 1, 0, 0, 32, 24, 157960)),
    ("R7", 20, 256): ((4, 2, 1, 1, 7, 7, 14, 80, 104824), (4, 2, 1, 1, 0, 0, 4, 16, 63352)), ("R7", 20, 304): ((7, 1, 1, 1, 7, 7, 17, 40, 84088), (7, 1, 1, 1, 0, 0, 7, 8, 58168)), ("R7", 20, 128): ((3, 3, 1, 1, 7, 7, 13, 120, 130744), (3, 3, 1, 1, 0, 0, 3, 24, 68536)),
    ("R7", 44, 256): ((2, 4, 3, 1, 7, 7, 12, 160, 156664), (2, 4, 3, 1, 0, 0, 2, 32, 73720)), ("R7", 44, 304): ((3, 3, 1, 1, 7, 7, 13, 120, 130744), (3, 3, 1, 1, 0, 0, 3, 24, 68536)), ("R7", 44, 128): ((2, 4, 3, 1, 7, 7, 12, 160, 156664), (1, 7, 7, 1, 0, 0, 1, 56, 89272)),
    ("R7", 88, 256): ((2, 4, 3, 1, 7, 7, 12, 160, 156664), (1, 7, 7, 1, 0, 0, 1, 56, 89272)), ("R7", 88, 304): ((2, 4, 3, 1, 7, 7, 12, 160, 156664), (1, 7, 7, 1, 0, 0, 1, 56, 89272)), ("R7", 88, 128): ((2, 4, 3, 1, 7, 7, 12, 160, 156664), (1, 7, 7, 1, 0, 0, 1, 56, 89272)),
    ("VL2", 8, 256): ((11, 3, 3, 1, 3, 3, 26, 108, 94376), (11, 3, 3, 1, 0, 0, 11, 36, 55784)), ("VL2", 8, 304): ((17, 2, 1, 1, 3, 3, 32, 72, 75080), (17, 2, 1, 1, 0, 0, 17, 24, 49352)), ("VL2", 8, 128): ((7, 5, 3, 1, 3, 3, 22, 180, 132968), (7, 5, 3, 1, 0, 0, 7, 60, 68648)),
    ("VL2", 20, 256): ((6, 6, 3, 1, 3, 3, 21, 216, 152264), (6, 6, 3, 1, 0, 0, 6, 72, 75080)), ("VL2", 20, 304): ((7, 5, 3, 1, 3, 3, 22, 180, 132968), (7, 5, 3, 1, 0, 0, 7, 60, 68648)), ("VL2", 20, 128): ((6, 6, 3, 1, 3, 3, 21, 216, 152264), (3, 11, 11, 1, 0, 0, 3, 132, 107240)),
}  # fmt: skip
LAUNCHES = sorted({(name, K) for name, K, _ in PLAN}, key=lambda t: (NAMES.index(t[0]), t[1]))
# the regime each long launch is there for, asserted on the GPU from the restated plan at the box's CU count before anything is compared:
# (case, intervals): (nc of the fused launch | None where only the residual is launched, nc of the residual-only launch, sx x ngrp crossed, uneven groups)
REGIME = {
    ("R1", 28): (2, 2, False, False), ("R1", 44): (3, 3, False, False), ("R1", 88): (5, 5, False, False), ("R2", 3): (1, 1, True, True),
    ("R3", 3): (1, 1, True, False), ("R4", 10): (4, 4, False, False), ("R5", 3): (1, 2, False, False), ("R5", 20): (None, 6, False, False),
    ("R6", 3): (None, 2, False, False), ("R7", 20): (2, 2, False, False), ("R7", 44): (4, 4, False, False), ("R7", 88): (4, 7, False, False),
    ("VL2", 8): (3, 3, False, False), ("VL2", 20): (6, 6, False, False),
}  # fmt: skip
# rollouts, (case, intervals, CUs): (panels P, npc, columns of the last panel, bytes of the propagator launch, chain slices S, nc, bytes of the chain launch)
ROLL = {
    ("R1", 29, 256): (2, 33, 33, 142608, 1, 5, 11744), ("R1", 29, 304): (3, 22, 22, 107232, 1, 5, 11744), ("R1", 29, 128): (2, 33, 33, 142608, 1, 5, 11744),
    ("VL2", 29, 256): (2, 33, 33, 142616, 3, 16, 35328), ("VL2", 29, 304): (3, 22, 22, 107240, 3, 16, 35328), ("VL2", 29, 128): (2, 33, 33, 142616, 3, 16, 35328),
    ("R7", 29, 256): (4, 20, 20, 130744, 1, 7, 19168), ("R7", 29, 304): (5, 16, 16, 115192, 1, 7, 19168), ("R7", 29, 128): (3, 27, 26, 157960, 1, 7, 19168),
    ("R7", 44, 256): (3, 27, 26, 157960, 1, 7, 19168), ("R7", 44, 304): (3, 27, 26, 157960, 1, 7, 19168), ("R7", 44, 128): (3, 27, 26, 157960, 1, 7, 19168),
}  # fmt: skip
# (case, intervals): (seed convention of the knot-0 sensitivities, the panel width the launch is there for)
ROLLS = {("R1", 29): (0, 33), ("VL2", 29): (1, 33), ("R7", 29): (0, 20), ("R7", 44): (1, 27)}
LONG_SUB = 20  # s' of every rollout's long step
# seconds of one order-10 longdouble truth of the closed trajectory on one CPU core, measured; order 4 takes a quarter of it or less; a rollout
# truth: ROLL_SECONDS
TRUTH_SECONDS = {"R1": 1.0, "R2": 6.0, "R3": 6.0, "R4": 6.1, "R5": 12.4, "R6": 0.4, "R7": 1.1, "VL2": 4.1}
ROLL_SECONDS = {("R1", 29): 1.4, ("VL2", 29): 8.4, ("R7", 29): 0.7, ("R7", 44): 1.1}


def shape(name):
    """(n, C, v, m)"""
    return CASES[name]


def _seed(name):
    return 18000 + 17 * NAMES.index(name)


# ---- the plans -------------------------------------------------------------------------------------------------------------------------------
def plan(name, K, n_cu=256, jac=True, **kw):
    n, C, v, m = CASES[name]
    return vl.var_large_plan(n, C, m, v, jac=jac, items=K, n_cu=n_cu, **kw)


def slices(p, C):
    """The state columns of every slice."""
    return [min(p["nc"], C - s * p["nc"]) for s in range(p["sx"])]


def groups(p, m):
    """The drives of every group of a Jacobian launch."""
    return [min(p["mg"], m - g * p["mg"]) for g in range(p["ngrp"])] if p["mg"] else [0]


def plan_row(name, K, n_cu=256, jac=True):
    """PLAN's row of one launch from the restated planner, and the slice and group lists."""
    n, C, v, m = CASES[name]
    p = plan(name, K, n_cu, jac)
    sl, gr = slices(p, C), groups(p, m)
    return (p["sx"], p["nc"], sl[-1], p["ngrp"], p["mg"], gr[-1], p["U"], p["chain_blocks"], p["bytes"]), sl, gr


def roll_plan(name, K, n_cu=256, **kw):
    n, C, v, m = CASES[name]
    return vf.roll_plan(n, C, m, v, K=K, n_cu=n_cu, **kw)


def roll_row(name, K, n_cu=256):
    r = roll_plan(name, K, n_cu)
    return (r["P"], r["npc"], r["npce"][-1], r["bytes_e"], r["S"], r["nc"], r["bytes_c"])


# ---- systems and trajectories ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def system(name):
    """(G0, Gj [m, n, n], [Gv_i]) -- the variation generators already divided by their scales."""
    if name in BORROWED:
        return vl.system(BORROWED[name])
    n, C, v, m = CASES[name]
    d = n // 2
    rng = np.random.default_rng(_seed(name))
    H0 = vsc._herm(d, rng)
    Hd = [vsc._herm(d, rng) for _ in range(m)]
    Hv = [vsc._herm(d, rng) for _ in range(v)]
    G0 = vl.po.G_of_H(H0)
    Gj = np.array([vl.po.G_of_H(H) for H in Hd]).reshape(m, n, n)
    Gv = [vl.po.G_of_H(H) / s for H, s in zip(Hv, vl.SCALES)]
    for a in [G0, Gj] + Gv:
        a.setflags(write=False)
    return G0, Gj, Gv


@functools.lru_cache(maxsize=None)
def base(name):
    """The case's own P knots (VarCase of P - 1 intervals), read-only: vl.case for R4 (VL3) and VL2, the same recipe with this module's seeds
    for the others."""
    if name in ("R4", "VL2"):
        return vl.case(BORROWED[name])[0]
    n, C, v, m = CASES[name]
    G0, Gj, Gv = system(name)
    xdc = n * C
    z_dim, xo, dt_off, u_off = (v + 1) * xdc + 2 + m, [b * xdc for b in range(v + 1)], (v + 1) * xdc, (v + 1) * xdc + 2
    Z = 0.4 * np.random.default_rng(_seed(name) + 1).standard_normal((4, z_dim))
    cs = vt.VarCase(Z=Z, z_dim=z_dim, N=4, n=n, C=C, m=m, xo=xo, u_off=u_off, dt_off=dt_off, G0=G0, Gv=Gv, Gj=Gj)
    n2 = [vsc._lifted_norm(cs, k) for k in range(3)]
    Z[:, dt_off] = 0.1
    Z[0, dt_off], Z[1, dt_off], Z[2, dt_off] = 0.15 / n2[0], -0.3 / n2[1], LONG[name] / n2[2]
    Z[:, dt_off + 1] = np.cumsum(Z[:, dt_off])
    Z.setflags(write=False)
    return cs


def _with(cs, Z):
    Z.setflags(write=False)
    return vt.VarCase(**{**cs.__dict__, "Z": Z, "N": Z.shape[0]})


@functools.lru_cache(maxsize=None)
def case(name):
    """The CLOSED trajectory: the P knots, knot 0 again; P intervals, the wrap interval's step at h |Ghat|_2 = WRAP_STEP."""
    b = base(name)
    Z = np.concatenate([b.Z, b.Z[:1]])
    Z[b.N - 1, b.dt_off] = WRAP_STEP / vsc._lifted_norm(b, b.N - 1)
    return _with(b, Z)


def periods(name):
    return base(name).N


def long_knots(name, K):
    """[K + 1, z_dim]: the closed trajectory continued periodically; interval k is interval k mod P of `case`."""
    cs = case(name)
    return cs.Z[np.arange(K + 1) % cs.K]


def long_case(name, K):
    return _with(case(name), np.array(long_knots(name, K)))


def interval_case(cs, k):
    """Interval k alone: a VarCase of two knots."""
    return _with(cs, np.array(cs.Z[k : k + 2]))


def long_step_search(name):
    """The smallest of vector_shape_cases.LONG_STEPS at which zeroing c_5 at order 10 moves interval 2's residual by SEEN of its own size or more
    (None: no such step), and the weights read on the way."""
    b = base(name)
    Z = np.array(b.Z)
    norm = 1.0 / vsc._lifted_norm(b, 2)
    seen = {}
    for s in vs.LONG_STEPS:
        Z[2, b.dt_off] = s * norm
        seen[s] = top_term_weight(_with(b, np.array(Z)))
        if seen[s] >= SEEN:
            return s, seen
    return None, seen


def top_term_weight(cs, k=2, order=10):
    """By how much zeroing c_q moves interval k's residual, relative to the residual's own maximum (delta alone: delta_truth_ld)."""
    c = vs.coeffs(order)
    c0 = c.copy()
    c0[-1] = 0
    a, b = delta_truth_ld(cs, order, (k,), c), delta_truth_ld(cs, order, (k,), c0)
    return float(np.abs(a - b).max() / np.abs(a).max())


def context_args(cs, order, **kw):
    return vl.context_args(cs, order, **kw)


# ---- the truth ---------------------------------------------------------------------------------------------------------------------------------
def delta_truth_ld(cs, order, intervals=None, c=None):
    """delta [intervals, xd] in stacked order, in longdouble, through the block structure of the lifted generator -- [V; Vv_i] -> [G V; G Vv_i +
    Gv_i V], never a lifted matrix: delta = sum_j c_j Ghat^j Y_j with Y_j = (-h)^j X_k+1 - h^j X_k, in Horner form."""
    n, C, v, m = cs.n, cs.C, cs.v, cs.m
    c = vs.coeffs(order) if c is None else np.asarray(c, dtype=LD_)
    q = len(c) - 1
    G0l, Gl, Gvl = np.asarray(cs.G0, dtype=LD_), [np.asarray(g, dtype=LD_) for g in cs.Gj], [np.asarray(g, dtype=LD_) for g in cs.Gv]
    col = lambda z, o: np.array(np.asarray(z[o : o + cs.xdc], dtype=LD_).reshape(C, n).T)
    out = []
    for k in range(cs.K) if intervals is None else intervals:
        h = LD_(cs.Z[k, cs.dt_off])
        G = G0l.copy()
        for l in range(m):
            G = G + LD_(cs.Z[k, cs.u_off + l]) * Gl[l]
        Xc, Xn = [col(cs.Z[k], o) for o in cs.xo], [col(cs.Z[k + 1], o) for o in cs.xo]
        Y = lambda j: [(-h) ** j * Xn[b] - h**j * Xc[b] for b in range(v + 1)]
        A = [c[q] * y for y in Y(q)]
        for j in range(q - 1, -1, -1):
            GA = G @ np.concatenate(A, axis=1)
            A = [GA[:, :C]] + [GA[:, b * C : (b + 1) * C] + Gvl[b - 1] @ A[0] for b in range(1, v + 1)]
            A = [a + c[j] * y for a, y in zip(A, Y(j))]
        out.append(np.concatenate([a.T.reshape(-1) for a in A]))
    return np.array(out)


def lifted_interval(name, order, k, gj_zero_from=None, zero_cols=(), cs=None, **kw):
    """vector_shape_cases.truth_values on interval k of the lifted closed trajectory, in longdouble: (delta [xd] in stacked order, the Jacobian
    values [per] in the library's order).  kw: truth_values' switches (c, drop_drive, drop_col, mm).  gj_zero_from: the drives from that index on
    read as zero (a drive group ignored); zero_cols: those state columns of every component read as zero (a slice dropped)."""
    cs = case(name) if cs is None else cs
    Zl, lay, G0l, Gjl = vt.lifted(cs)
    if gj_zero_from is not None:
        Gjl = np.array(Gjl)
        Gjl[gj_zero_from:] = 0
    if len(zero_cols):
        Zl = np.array(Zl)
        X = Zl[:, : cs.C * lay.n].reshape(cs.N, cs.C, lay.n).copy()
        X[:, list(zero_cols)] = 0
        Zl[:, : cs.C * lay.n] = X.reshape(cs.N, -1)
    d, j, _ = vs.truth_values(lay, G0l, Gjl, Zl, None, order, hessian=False, intervals=(k,), **kw)
    ds = np.empty_like(d[0])
    ds[vt._row_map(cs)] = d[0]
    vi = vl.value_index(cs)
    rest = np.ones(j.shape[1], dtype=bool)
    rest[vi] = False
    assert not np.any(j[0][rest])  # the library's structure holds every non-zero of the lifted problem
    return ds, j[0][vi]


@functools.lru_cache(maxsize=None)
def truth(name, order):
    """(delta [P xd], the Jacobian values [P per] in the library's order | None on a residual-only case) of the closed trajectory, rounded from
    longdouble to float64: what the GPU tests compare with.  Computed once and never written to."""
    cs = case(name)
    if name in RESIDUAL_ONLY:
        out = (delta_truth_ld(cs, order).astype(np.float64).reshape(-1), None)
    else:
        per = [lifted_interval(name, order, k) for k in range(cs.K)]
        out = (np.concatenate([d.astype(np.float64) for d, _ in per]), np.concatenate([j.astype(np.float64) for _, j in per]))
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


# ---- the per-segment rule of vl.check, one interval's codes sorted once per case ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def segments(name, which):
    """(the one-interval case, segment codes, a permutation that sorts one interval's values by segment, each segment's start in it): `which` is
    "delta" (vsc.residual_codes) or "jac" (vsc.jac_codes on vl.lib_structure)."""
    one = interval_case(case(name), 0)
    if which == "delta":
        codes = vsc.residual_codes(one, np.arange(one.xd))
    else:
        r, c = vl.lib_structure(one)
        codes = vsc.jac_codes(one, r, c)
    uniq, inv = np.unique(codes, return_inverse=True)
    inv = inv.reshape(-1)
    order = np.argsort(inv, kind="stable")
    out = (uniq, order, np.searchsorted(inv[order], np.arange(uniq.size)))
    for a in out:
        a.setflags(write=False)
    return (one,) + out


def segment_name(name, which, code, k):
    one = segments(name, which)[0]
    return (vsc.residual_name(one, code) if which == "delta" else vsc.jac_name(one, code))[:-1] + str(k)


def segment_errors(name, which, got, ref):
    """{segment name: (max |got - ref|, max |ref|)} over the intervals of got (interval k against interval k of ref)."""
    one, uniq, order, starts = segments(name, which)
    a, b = np.asarray(got, dtype=np.float64).reshape(-1, order.size), np.asarray(ref, dtype=np.float64).reshape(-1, order.size)
    assert a.shape == b.shape, (a.shape, b.shape)
    out = {}
    for k in range(a.shape[0]):
        err = np.maximum.reduceat(np.abs(a[k] - b[k])[order], starts)
        scale = np.maximum.reduceat(np.abs(b[k])[order], starts)
        for s, e, sc in zip(uniq, err, scale):
            out[segment_name(name, which, s, k)] = (float(e), float(sc))
    return out


def assert_segments(errors, tol, what):
    """vsc.assert_segments' rule: every segment within tol of its own maximum, an identically-zero segment exactly zero (NaN fails).  Returns the
    worst (relative error, segment)."""
    worst = (0.0, None)
    for s, (e, scale) in errors.items():
        assert np.isfinite(e) and e <= tol * scale, "%s, segment %s: max err %.3e, max |truth| %.3e (rel %.3e > %.1e)" % (
            what, s, e, scale, e / scale if scale else np.inf, tol)  # fmt: skip
        if scale > 0 and e / scale > worst[0]:
            worst = (e / scale, s)
    return worst


def check(name, order, delta, vals, tol=TOL, what=""):
    """delta (and the Jacobian values, where not None) of the closed launch against the truth, per segment.  Returns the worst of each."""
    d, j = truth(name, order)
    wd = assert_segments(segment_errors(name, "delta", delta, d), tol, "%s order %d %s residual" % (name, order, what))
    wj = (0.0, None)
    if vals is not None:
        wj = assert_segments(segment_errors(name, "jac", vals, j), tol, "%s order %d %s Jacobian" % (name, order, what))
    return wd, wj


def moved(name, which, good, bad):
    """The largest relative change of a segment, against the segment's own maximum in `good`."""
    return max([e / sc for e, sc in segment_errors(name, which, bad, good).values() if sc > 0], default=0.0)


# ---- faults of the residual + Jacobian kernel, on one interval's values in the library's order ------------------------------------------------------
def tails_view(name, vals):
    """One interval's d/du | d/dt tails as [1 + v, C, m + 1, n], a view."""
    n, C, v, m = CASES[name]
    return vals[(2 + 4 * v) * C * n * n :].reshape(1 + v, C, m + 1, n)


def exchange_groups(name, vals, gr, a=0, b=None):
    """The tails of drive groups a and b (default: the last) exchanged, drive for drive, as far as the narrower group goes."""
    out = np.array(vals)
    t = tails_view(name, out)
    b = len(gr) - 1 if b is None else b
    oa, ob, w = sum(gr[:a]), sum(gr[:b]), min(gr[a], gr[b])
    t[:, :, oa : oa + w], t[:, :, ob : ob + w] = t[:, :, ob : ob + w].copy(), t[:, :, oa : oa + w].copy()
    return out


def swapped_decode(name, vals, sl, gr):
    """Chain unit u computes slice u % sx and group u / sx, but stores as a unit decoded s = u / ngrp, g = u % ngrp would: the (column, drive) tails
    of unit u land in the place of unit (u / ngrp) + sx (u % ngrp), column for column and drive for drive as far as the narrower goes."""
    src = np.asarray(vals)
    out = np.array(vals)
    t, ts = tails_view(name, out), tails_view(name, src)
    sx, ngrp = len(sl), len(gr)
    c0, g0 = np.concatenate([[0], np.cumsum(sl)]), np.concatenate([[0], np.cumsum(gr)])
    for u in range(sx * ngrp):
        s, g = u % sx, u // sx
        s2, g2 = u // ngrp, u % ngrp
        wc, wg = min(sl[s], sl[s2]), min(gr[g], gr[g2])
        t[:, c0[s2] : c0[s2] + wc, g0[g2] : g0[g2] + wg] = ts[:, c0[s] : c0[s] + wc, g0[g] : g0[g] + wg]
    return out


def column_reads_two_back(name, delta, vals, sl):
    """In every slice, a column c >= 2 of the slice takes column c - 2's additive term (its states): its delta and its tails are those of the
    column two before it (the B and L blocks do not depend on the column)."""
    n, C, v, m = CASES[name]
    d, j = np.array(delta), np.array(vals)
    dv, t = d.reshape(1 + v, C, n), tails_view(name, j)
    c0 = 0
    for w in sl:
        for c in range(2, w):
            dv[:, c0 + c] = np.asarray(delta).reshape(1 + v, C, n)[:, c0 + c - 2]
            t[:, c0 + c] = tails_view(name, np.asarray(vals))[:, c0 + c - 2]
        c0 += w
    return d, j


# ---- rollouts ----------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def roll_case(name, K):
    """(VarCase of K intervals, substeps per interval), read-only."""
    seed = ROLLS[(name, K)][0]
    b = base(name)
    rng = np.random.default_rng(_seed(name) + 500 + K + seed)
    Z = 0.4 * rng.standard_normal((K + 1, b.z_dim))
    if seed == 0:
        for o in b.xo[1:]:
            Z[0, o : o + b.xdc] = 0.0
    cs = vt.VarCase(**{**b.__dict__, "Z": Z, "N": K + 1})
    G = [vf.g_of(cs, k) for k in range(K)]
    n1 = [np.abs(g).sum(axis=0).max() for g in G]
    sign = 1.0 if seed else -1.0
    for k in range(K):
        Z[k, cs.dt_off] = sign * (-1.0) ** k * 0.8 / n1[k]
    Z[1, cs.dt_off] = (LONG_SUB - 0.5) / n1[1]
    Z[2, cs.dt_off] = 0.0
    Z[3, cs.dt_off] = -2.5 / n1[3]
    Z[K, cs.dt_off] = 0.0
    t_off = 0 if name == "VL2" else cs.dt_off + 1
    Z[:, t_off] = np.cumsum(Z[:, cs.dt_off])
    sp = tuple(vf.substeps(Z[k, cs.dt_off], G[k]) for k in range(K))
    Z.setflags(write=False)
    return cs, sp


@functools.lru_cache(maxsize=None)
def rollout_truth_ld(name, K):
    out = vf.rollout_truth_values(roll_case(name, K)[0])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def rollout_truth(name, K):
    """The same rounded to float64: what the GPU tests compare with."""
    out = rollout_truth_ld(name, K).astype(np.float64)
    out.setflags(write=False)
    return out


def first_knots(cs, N=4):
    """The first N knots as a trajectory of their own."""
    return _with(cs, np.array(cs.Z[:N]))


def restatement_with_panels(cs, npce, zero):
    """vf.restatement (the kernel's algorithm in float64) with the columns >= 16 of each panel (npce columns per panel) of E (zero = "E") or of
    every L_i (zero = "L") read as zero in the chain."""
    dead = np.zeros(cs.n, bool)
    c0 = 0
    for w in npce:
        dead[c0 + 16 : c0 + w] = True
        c0 += w
    X = [vf._cols(cs, cs.Z[0, o : o + cs.xdc], np.float64) for o in cs.xo]
    out = [vf._stack(X)]
    for k in range(cs.K):
        E, L = vf.propagators(cs, k)
        E, L = np.array(E), [np.array(l) for l in L]
        if zero == "E":
            E[:, dead] = 0
        else:
            for l in L:
                l[:, dead] = 0
        X = [E @ X[0]] + [E @ X[1 + i] + L[i] @ X[0] for i in range(cs.v)]
        out.append(vf._stack(X))
    return np.array(out)
