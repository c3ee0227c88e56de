"""Cases that walk the large exponential kernels (contexts created with PCL_LARGE_N | PCL_LARGE_EXP, pade_order = PCL_ORDER_EXP, generator dimensions
66 .. 128) over the regimes of their launch plans that L1 .. L9, L1z and X1 never enter: pcl_kernel_large_exp.hpp in its modes FULL, COMPACT, MERIT and
PAYLOAD and its residual-only launch (planned by large_exp_plan in pcl_host_launch_pade.hpp, restated as le.plan and, payload-only, xc.plan), the device
expansion pcl_exp_expand_large_kernel, and pcl_kernel_large_exp_hess.hpp with its sum kernel (large_exp_hess_plan in pcl_host_launch_hess.hpp, restated
as lh.plan).  Importable without a GPU.  The existing case modules are imported and never written to.

Generators follow the recipe of lc.system (three drifts, then the drives), knots (N = 4, 0.4 N(0, 1)) and steps the rule of le.case: h |G|_1 = 0.8
(s' = 1), -2.5 (s' = 3) and LONG_STEP[case] on interval 2, none near an integer; the unitary cases take a long step of s' = 20 or 21.  Seeds: 27000 +
17 index for the system, + 1 for the knots, + 77 for the Hessian's multipliers (+ 1009 per member), + 177 for the payload's explicit multipliers.

Truths, the committed ones, computed once per case and never written to: po.exp_residual and exp_truth.values (scipy expm / expm_frechet);
exp_hess_truth.values, or lh.values_per_drive where m >= 10 (Q7, Q11) and on Q10, whose pairwise truth took five seconds
(tests/test_large_exp_hess_cpu.py holds that identity to the pairwise truth; tests/test_large_exp_plan_cpu.py does so once more on Q12, m = 9);
the payload of large_exp_reduce_cases in np.longdouble with its Cauchy-Schwarz scale.  TRUTH_SECONDS has what each costs on one CPU core.

Cases (kind, n, cols, m), what each stands on, and what the plans give for the three intervals of a test launch on 256 CUs (J: residual + Jacobian,
H: Hessian of the Lagrangian; JAC_TABLE / EVAL_TABLE / PAYLOAD_TABLE / HESS_TABLE below hold every number at 3, 87 and 300 items and at 256, 304 and
128 CUs, and tests/test_large_exp_plan_cpu.py asserts them and, by predicates on the plans, that every regime named here is entered):
    Q1   iso 120 60  4   a bench shape (d = 60): 36 chain units, 60 panel units, the last slice of 4     J U 60 = 9 (7) x 4 (1), npc 2, 163,744 B
                                                                                                         H U 60 = 60 (1) x 1 pair (mg 4), W 15 of 16
    Q2   iso 128 64  2   x_dim 8192: one column of E per unit, 32 of 128 units run a chain, W = NBW      J U 128 = 16 (4) x 2 (1), npc 1, W 9 of 9
                                                                                                         H U 64 = 64 (1) x 1 pair (mg 2), W 6 of 9
    Q3   iso  96 48  4   the other bench shape (d = 48): a full column tile per slice, three tiles       J U 20 = 3 (16) x 4 (1), npc 5, W 37 of 37
                         per unit; the Hessian plan chooses nc 2 itself                                  H U 24 = 24 (2) x 1 pair (mg 4), W 30 of 37
    Q4   vec 100  1  5   448 threads (seven waves), n mod 16 = 4; the plan moves at 300 items            J U 8 = 1 x 3 (2, 2, 1), npc 13 (last 9)
                                                                                                         H U 1 (mg 5), W 21 of 33: two tiles
    Q5   iso 104  1  0   no drive at all, at 448 threads                                                 J U 7, mg 0, npc 15 (last 14)
                                                                                                         H U 1, mg 0, W 2
    Q6   iso  80  7  7   the plan moves at 87 items: four groups of 2, 2, 2, 1 and panels of 20          J U 40 = 1 (7) x 7 (1), npc 2
                                                                                                         H U 7 = 7 (1) x 1 pair (mg 7), W 36: three tiles
    Q7   iso  88  3 11   Hessian groups 4, 4, 3 crossed with 3 slices; the payload-only plan takes       J U 11 = 1 (3) x 11 (1), npc 8
                         mg 4; at 300 items panels of 30 at W 45 of 46                                   H U 18 = 3 (1) x 6 pairs (mg 4: 4, 4, 3), W 25
    Q8   vec  67  1  6   odd n, LD = n: U 6 -> 2 -> 6 with the item count, panels of 34 and 33           J U 6 = 1 x 2 (3), npc 12 (last 7)
                                                                                                         H U 1 (mg 6), W 28: two tiles
    Q9   iso  66 33  0   no drive, three slices of 11; the Hessian's [X_k | G X_k] pair behind a         J U 14 = 3 (11) x 1, npc 5 (last 1)
                         chain of two tiles                                                              H U 3 = 3 (11), mg 0, W 22
    Q10  iso 126  5  7   Hessian groups 2, 2, 2, 1 crossed with 5 slices; one column of E per unit       J U 126 = 1 (5) x 7 (1), npc 1
                                                                                                         H U 50 = 5 (1) x 10 pairs (mg 2: 2, 2, 2, 1), W 9 of 11
    Q11  iso 128  5 24   48 chain units against 43 panel units: units 43 .. 47 own nothing of E          J U 48 = 2 (3, 2) x 24 (1), npc 3 (unit 42: 2)
                                                                                                         H U 390 = 5 (1) x 78 pairs (mg 2), W 9 of 9
    Q12  iso  72  5  9   the drive group grows 1 -> 2 -> 3 with the item count                           J U 12 = 1 (5) x 9 (1), npc 6
                                                                                                         H U 5 = 5 (1) x 1 pair (mg 9), W 55 of 68: four tiles
    Q9s  iso  66 17  0   Q9 at 17 columns (slices 9 + 8), for the long launches: 300 items of Q9's 33 columns are 355 MB per array of values
Long launches (LONG_NAMES): the case's own four knots as 29 and as 100 seeds of one PCL_BATCH_TRAJ launch, 87 and 300 items, on Q4, Q6, Q7, Q8, Q9s
and Q12; no unitary case runs long.

Emulations: le.emulate and lh.emulate_hess (float64 numpy, sharing no code with the truths) with their mutants and the `mm` faults, and three
mutants of this module for the new regimes, each the value an index formula would give with its bound dropped:
    as_if_full         the last slice's missing columns computed as if the slice were full, each a clamped load of the last real column: the sums over
                       the columns (the Hessian's scalars, the payload) count the last column once more per missing column
    first_group_size   the pair of uneven drive groups taken with the first group's size: the short last group runs a drive m whose generator is
                       zero and whose output slot is the dt slot -- (u_m, u_l) lands on (dt, u_l) of the other groups' drives, <d delta / d u_m, lam> on
                       g_dt: those entries come out as zero
    second_tile        the second 16-column tile of a unit's buffer never run: its columns keep what they were loaded with -- the panel's columns of E the
                       identity, the chain's V columns X_k, its dV columns zero"""
import functools
import types

import numpy as np

import exp_hess_truth as eht
import exp_truth as xt
import large_exp_cases as le
import large_exp_hess_cases as lh
import large_exp_reduce_cases as xc
import vector_shape_cases as vc
from oracle import pade_oracle as po

N = le.N
K = N - 1
LDS_BYTES = le.LDS_BYTES
TOL = 1e-11
FLOOR = 1e-12  # the float64 emulation against the truth, per segment: a tenth of TOL, so that the truth does not eat the kernel's margin
SEEN = 1e-7
CUS = (256, 304, 128)
ITEMS = (3, 87, 300)

# name: (kind, n, cols, m)
CASES = {
    "Q1": ("iso", 120, 60, 4), "Q2": ("iso", 128, 64, 2), "Q3": ("iso", 96, 48, 4), "Q4": ("vec", 100, 1, 5), "Q5": ("iso", 104, 1, 0),
    "Q6": ("iso", 80, 7, 7), "Q7": ("iso", 88, 3, 11), "Q8": ("vec", 67, 1, 6), "Q9": ("iso", 66, 33, 0), "Q10": ("iso", 126, 5, 7),
    "Q11": ("iso", 128, 5, 24), "Q12": ("iso", 72, 5, 9), "Q9s": ("iso", 66, 17, 0),
}  # fmt: skip
NAMES = list(CASES)
UNITARY = ("Q1", "Q2", "Q3")
LONG_NAMES = ["Q4", "Q6", "Q7", "Q8", "Q9s", "Q12"]
SEEDS = {87: 29, 300: 100}  # items of a long launch: trajectories of three intervals
PER_DRIVE = ("Q7", "Q10", "Q11")  # the Hessian's truth by the per-drive identity: m >= 10, and Q10, whose 28 pairs of 504 x 504 exponentials took 5.0 s
# h |G|_1 on interval 2: s' = its ceiling
LONG_STEP = {"Q1": 19.6, "Q2": 20.4, "Q3": 19.3, "Q4": 23.4, "Q5": 31.7, "Q6": 26.6, "Q7": 35.3, "Q8": 41.6, "Q9": 22.7, "Q10": 28.4, "Q11": 24.6,
             "Q12": 47.3, "Q9s": 22.7}  # fmt: skip

# ---- the committed tables -----------------------------------------------------------------------------------------------------------------------
# The launch with values: (U, sx, nc, ngrp, mg, npc, W, NBW, bytes).  Plans that move neither with the items nor with the CUs, by case ...
_JAC_STILL = {
    "Q1": (60, 9, 7, 4, 1, 2, 16, 16, 163744), "Q2": (128, 16, 4, 2, 1, 1, 9, 9, 161064), "Q3": (20, 3, 16, 4, 1, 5, 37, 37, 161752),
    "Q5": (7, 1, 1, 1, 0, 15, 16, 29, 128768), "Q10": (126, 1, 5, 7, 1, 1, 11, 11, 162688), "Q11": (48, 2, 3, 24, 1, 3, 9, 9, 161240),
}  # fmt: skip
# ... and those that move, (case, items): the row, or {CUs: row} where the three CU counts differ
_A4, _B4 = (8, 1, 1, 3, 2, 13, 16, 33, 120712), (4, 1, 1, 1, 5, 25, 31, 33, 157072)
_A6, _B6, _C6 = (40, 1, 7, 7, 1, 2, 16, 57, 84088), (4, 1, 7, 4, 2, 20, 41, 57, 132688), (3, 1, 7, 3, 3, 27, 55, 57, 159904)
_A7, _B7 = (11, 1, 3, 11, 1, 8, 14, 46, 93736), (3, 1, 3, 3, 4, 30, 45, 46, 159952)
_A8, _B8, _C8 = (6, 1, 1, 2, 3, 12, 16, 78, 62776), (2, 1, 1, 2, 3, 34, 38, 78, 98152), (1, 1, 1, 1, 6, 67, 74, 78, 156040)
_A9, _B9 = (14, 3, 11, 1, 0, 5, 16, 79, 62192), (3, 3, 11, 1, 0, 22, 33, 79, 89528)
_A12, _B12, _C12 = (12, 1, 5, 9, 1, 6, 16, 68, 71240), (5, 1, 5, 5, 2, 15, 30, 68, 95768), (3, 1, 5, 3, 3, 24, 44, 68, 120296)
_A13, _B13 = (10, 2, 9, 1, 0, 7, 16, 79, 62192), (2, 2, 9, 1, 0, 33, 42, 79, 104000)
JAC_TABLE = {
    ("Q4", 3): _A4, ("Q4", 87): {256: _A4, 304: _A4, 128: _B4}, ("Q4", 300): {256: _B4, 304: _B4, 128: _A4},
    ("Q6", 3): _A6, ("Q6", 87): {256: _B6, 304: _C6, 128: _B6}, ("Q6", 300): {256: _B6, 304: _C6, 128: _B6},
    ("Q7", 3): _A7, ("Q7", 87): {256: _A7, 304: _B7, 128: _A7}, ("Q7", 300): _B7,
    ("Q8", 3): _A8, ("Q8", 87): {256: _B8, 304: _A8, 128: _C8}, ("Q8", 300): {256: _A8, 304: _C8, 128: _C8},
    ("Q9", 3): _A9, ("Q9", 87): {256: _A9, 304: _B9, 128: _B9}, ("Q9", 300): _B9,
    ("Q12", 3): _A12, ("Q12", 87): {256: _B12, 304: _C12, 128: _B12}, ("Q12", 300): _C12,
    ("Q9s", 3): _A13, ("Q9s", 87): _B13, ("Q9s", 300): _B13,
}  # fmt: skip
JAC_TABLE.update({(name, items): row for name, row in _JAC_STILL.items() for items in ITEMS})
# ... on 256 CUs the slices' columns, the groups' drives and the columns of E of the last three units (Q11: none -- units 43 .. 47 own nothing, and
# unit 42 two columns); by case where the plan stands still, by (case, items) where it moves
JAC_SPLIT = {
    "Q1": ([7] * 8 + [4], [1] * 4, [2, 2, 2]), "Q2": ([4] * 16, [1, 1], [1, 1, 1]), "Q3": ([16] * 3, [1] * 4, [5, 5, 1]),
    "Q5": ([1], [0], [15, 15, 14]), "Q10": ([5], [1] * 7, [1, 1, 1]), "Q11": ([3, 2], [1] * 24, [0, 0, 0]),
    ("Q4", 3): ([1], [2, 2, 1], [13, 13, 9]), ("Q4", 87): ([1], [2, 2, 1], [13, 13, 9]), ("Q4", 300): ([1], [5], [25, 25, 25]),
    ("Q6", 3): ([7], [1] * 7, [2, 2, 2]), ("Q6", 87): ([7], [2, 2, 2, 1], [20, 20, 20]), ("Q6", 300): ([7], [2, 2, 2, 1], [20, 20, 20]),
    ("Q7", 3): ([3], [1] * 11, [8, 8, 8]), ("Q7", 87): ([3], [1] * 11, [8, 8, 8]), ("Q7", 300): ([3], [4, 4, 3], [30, 30, 28]),
    ("Q8", 3): ([1], [3, 3], [12, 12, 7]), ("Q8", 87): ([1], [3, 3], [34, 33]), ("Q8", 300): ([1], [3, 3], [12, 12, 7]),
    ("Q9", 3): ([11] * 3, [0], [5, 5, 1]), ("Q9", 87): ([11] * 3, [0], [5, 5, 1]), ("Q9", 300): ([11] * 3, [0], [22, 22, 22]),
    ("Q12", 3): ([5], [1] * 9, [6, 6, 6]), ("Q12", 87): ([5], [2, 2, 2, 2, 1], [15, 15, 12]), ("Q12", 300): ([5], [3, 3, 3], [24, 24, 24]),
    ("Q9s", 3): ([9, 8], [0], [7, 7, 3]), ("Q9s", 87): ([9, 8], [0], [33, 33]), ("Q9s", 300): ([9, 8], [0], [33, 33]),
}  # fmt: skip
# The payload-only launch: (U, sx, nc, ngrp, mg, W, bytes), by case where it stands still, by (case, items) -- a row or {CUs: row} -- where it moves
_P6 = {7: (7, 1, 7, 7, 1, 14, 80200), 4: (2, 1, 7, 2, 4, 35, 121024), 3: (3, 1, 7, 3, 3, 28, 107416), 1: (1, 1, 7, 1, 7, 56, 161848)}
_P7 = {4: (3, 1, 3, 3, 4, 15, 95872), 11: (1, 1, 3, 1, 11, 36, 140728)}
_P12 = {2: (5, 1, 5, 5, 2, 15, 69488), 5: (2, 1, 5, 2, 5, 30, 95768), 9: (1, 1, 5, 1, 9, 50, 130808)}
PAYLOAD_TABLE = {
    "Q1": (36, 9, 7, 4, 1, 14, 157936), "Q2": (32, 16, 4, 2, 1, 8, 157968), "Q3": (12, 3, 16, 4, 1, 32, 150112), "Q4": (1, 1, 1, 1, 5, 6, 96472),
    "Q5": (1, 1, 1, 1, 0, 1, 90968), "Q8": (1, 1, 1, 1, 6, 7, 48304), "Q9": (3, 3, 11, 1, 0, 11, 54152), "Q10": (7, 1, 5, 7, 1, 10, 159640),
    "Q11": (24, 2, 3, 12, 2, 9, 161240), "Q9s": (2, 2, 9, 1, 0, 9, 50936),
    ("Q6", 3): _P6[7], ("Q6", 87): {256: _P6[4], 304: _P6[3], 128: _P6[1]}, ("Q6", 300): _P6[1],
    ("Q7", 3): _P7[4], ("Q7", 87): {256: _P7[4], 304: _P7[4], 128: _P7[11]}, ("Q7", 300): {256: _P7[4], 304: _P7[11], 128: _P7[4]},
    ("Q12", 3): _P12[2], ("Q12", 87): {256: _P12[5], 304: _P12[5], 128: _P12[9]}, ("Q12", 300): {256: _P12[5], 304: _P12[9], 128: _P12[5]},
}  # fmt: skip
# The residual-only launch (it reads neither the items nor the CUs): (U, nc, W, bytes), the slices' columns
EVAL_TABLE = {
    "Q1": ((4, 15, 15, 160840), [15] * 4), "Q2": ((8, 8, 8, 157968), [8] * 8), "Q3": ((3, 16, 16, 112864), [16] * 3), "Q4": ((1, 1, 1, 84352), [1]),
    "Q5": ((1, 1, 1, 90968), [1]), "Q6": ((1, 7, 7, 66592), [7]), "Q7": ((1, 3, 3, 70240), [3]), "Q8": ((1, 1, 1, 38656), [1]),
    "Q9": ((3, 11, 11, 54152), [11] * 3), "Q10": ((1, 5, 5, 144400), [5]), "Q11": ((1, 5, 5, 148856), [5]), "Q12": ((1, 5, 5, 51968), [5]),
    "Q9s": ((2, 9, 9, 50936), [9, 8]),
}  # fmt: skip
# The Hessian (neither): (U, sx, nc, ngrp, mg, W, NBW, bytes), the slices' columns, the groups' drives
HESS_TABLE = {
    "Q1": ((60, 60, 1, 1, 4, 15, 16, 160840), [1] * 60, [4]), "Q2": ((64, 64, 1, 1, 2, 6, 9, 151776), [1] * 64, [2]),
    "Q3": ((24, 24, 2, 1, 4, 30, 37, 145456), [2] * 24, [4]), "Q4": ((1, 1, 1, 1, 5, 21, 33, 132832), [1], [5]),
    "Q5": ((1, 1, 1, 1, 0, 2, 29, 93488), [1], [0]), "Q6": ((7, 7, 1, 1, 7, 36, 57, 122968), [1] * 7, [7]),
    "Q7": ((18, 3, 1, 3, 4, 25, 46, 117232), [1] * 3, [4, 4, 3]), "Q8": ((1, 1, 1, 1, 6, 28, 78, 82072), [1], [6]),
    "Q9": ((3, 3, 11, 1, 0, 22, 79, 71840), [11] * 3, [0]), "Q10": ((50, 5, 1, 4, 2, 9, 11, 156592), [1] * 5, [2, 2, 2, 1]),
    "Q11": ((390, 5, 1, 12, 2, 9, 9, 161240), [1] * 5, [2] * 12), "Q12": ((5, 5, 1, 1, 9, 55, 68, 139568), [1] * 5, [9]),
    "Q9s": ((2, 2, 9, 1, 0, 18, 79, 65408), [9, 8], [0]),
}  # fmt: skip
# seconds on one CPU core, measured: (residual + Jacobian truth, Hessian truth, both emulations); both payload truths take under 0.05 s everywhere.
# No truth takes more than four seconds, so no Hessian had to be cut to fewer intervals; Q10's pairwise Hessian truth took 5.0 s (hence PER_DRIVE), and
# Q11's long step is 24.6 rather than 50.6 for the sake of its emulation (300 pairs of drives), which the CPU tests run six times
TRUTH_SECONDS = {
    "Q1": (0.1, 1.1, 0.8), "Q2": (0.1, 0.4, 0.5), "Q3": (0.1, 0.7, 0.4), "Q4": (0.1, 1.0, 0.1), "Q5": (0.1, 0.1, 0.1), "Q6": (0.1, 1.2, 0.4),
    "Q7": (0.1, 0.7, 0.7), "Q8": (0.1, 0.6, 0.2), "Q9": (0.1, 0.1, 0.1), "Q10": (0.1, 1.3, 0.8), "Q11": (0.3, 3.7, 4.3), "Q12": (0.1, 1.5, 0.6),
    "Q9s": (0.1, 0.1, 0.1),
}  # fmt: skip


def _index(name):
    return 13 if name == "Q9s" else int(name[1:])


def _seed(name):
    return 27000 + 17 * _index(name)


# ---- systems and trajectories ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def system(name, drift=0):
    """(G0, Gj) by the recipe of lc.system.  drift > 0: another drift for the same drives (a member of a PCL_BATCH_MEMBERS launch)."""
    kind, n, cols, m = CASES[name]
    rng = np.random.default_rng(_seed(name))
    if kind == "vec":
        G0s = [rng.standard_normal((n, n)) / np.sqrt(n) for _ in range(3)]
        Gj = rng.standard_normal((m, n, n)) / np.sqrt(n)
    else:
        G0s = [po.G_of_H(vc._herm(n // 2, rng)) for _ in range(3)]
        Gj = np.array([po.G_of_H(vc._herm(n // 2, rng)) for _ in range(m)]).reshape(m, n, n)
    return _ro(G0s[drift], Gj)


def layout(name):
    kind, n, cols, m = CASES[name]
    xs = n * cols
    if kind == "vec":
        return po.Layout(d=0, m=m, N=N, z_dim=xs + 2 + m, x_off=0, u_off=xs + 2, dt_off=xs, cols=1, gen=n)
    return po.Layout(d=n // 2, m=m, N=N, z_dim=xs + 2 + m, x_off=0, u_off=xs + 2, dt_off=xs, cols=cols)


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def case(name, drift=0):
    """(layout, G0, Gj, Z), read-only, by the rule of le.case.  drift: the member's drift on the SAME trajectory (the steps are those of drift 0)."""
    lay = layout(name)
    G0, Gj = system(name, 0)
    rng = np.random.default_rng(_seed(name) + 1)
    Z = 0.4 * rng.standard_normal((N, lay.z_dim))
    n1 = [le.norm1(vc.g_of(lay, Z, k, G0, Gj)) for k in range(K)]
    Z[0, lay.dt_off], Z[1, lay.dt_off], Z[2, lay.dt_off], Z[N - 1, lay.dt_off] = le.STEPS[0] / n1[0], le.STEPS[1] / n1[1], LONG_STEP[name] / n1[2], 0.1
    Z[:, lay.dt_off + 1] = np.cumsum(Z[:, lay.dt_off])
    return (lay, system(name, drift)[0], Gj) + _ro(Z)


@functools.lru_cache(maxsize=None)
def mu(name, drift=0):
    """The Hessian's multipliers of one member, [K, x_dim] like delta."""
    lay = layout(name)
    return _ro(np.random.default_rng(_seed(name) + 77 + 1009 * drift).standard_normal((K, lay.x_dim)))[0]


@functools.lru_cache(maxsize=None)
def lam(name):
    """The payload's explicit multipliers: a standard normal of delta's shape [K, cols, n]."""
    kind, n, cols, m = CASES[name]
    return _ro(np.random.default_rng(_seed(name) + 177).standard_normal((K, cols, n)))[0]


# ---- the truths, computed once and never written to ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def truth(name, drift=0):
    """(delta, full Jacobian values), flat, in the library's order: scipy expm / expm_frechet through the committed oracle."""
    lay, G0, Gj, Z = case(name, drift)
    return _ro(po.exp_residual(Z, lay, G0, Gj).reshape(-1), xt.values(Z, lay, G0, Gj).reshape(-1))


@functools.lru_cache(maxsize=None)
def hess_truth(name, drift=0):
    """The Hessian's values of one member, flat: exp_hess_truth.values, with segment 0 from the per-drive identity where m >= 10."""
    lay, G0, Gj, Z = case(name, drift)
    f = lh.values_per_drive if name in PER_DRIVE else eht.values
    return _ro(f(Z, mu(name, drift), lay, G0, Gj).reshape(-1))[0]


# xc.payload reads its shape from xc.CASES: the same code over this module's CASES (a function of its own globals; nothing of xc is written to)
_payload = types.FunctionType(xc.payload.__code__, dict(vars(xc), CASES=CASES), "payload", xc.payload.__defaults__)
_payload.__kwdefaults__ = dict(xc.payload.__kwdefaults__)


def payload(name, delta, vals, explicit, **faults):
    """(out, scale) of xc.payload in longdouble, [1 + K m + K] each, from one member's (delta, full values): lam = delta or lam(name)."""
    return _payload(name, [delta], [vals], [lam(name)] if explicit else None, **faults)


@functools.lru_cache(maxsize=None)
def payload_truth(name, explicit):
    return _ro(*payload(name, *truth(name), explicit))


worst = xc.worst


# ---- the kernels' recurrences in float64 numpy ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def emulated(name):
    return _ro(*le.emulate(*case(name)))


@functools.lru_cache(maxsize=None)
def emulated_hess(name):
    return _ro(lh.emulate_hess(*case(name), mu(name)))[0]


# ---- labels, and check_segments with the labels sorted once per case ----------------------------------------------------------------------------
def labels(name, which):
    lay = layout(name)
    kind, n, cols, m = CASES[name]
    return {"delta": lambda: le.residual_labels(lay), "jac": lambda: le.jac_labels(lay), "hess": lambda: lh.labels(lay),
            "compact": lambda: xc.compact_labels(n, cols, m)}[which]()  # fmt: skip


@functools.lru_cache(maxsize=None)
def segments(name, which):
    """(segment names, a permutation that sorts the values by segment, each segment's start in it).  Q2's Jacobian has 3.2 million labels: sorted
    once, not per comparison."""
    uniq, inv = np.unique(labels(name, which), return_inverse=True)
    inv = inv.reshape(-1)
    order = np.argsort(inv, kind="stable")
    return _ro(uniq, order, np.searchsorted(inv[order], np.arange(uniq.size)))


def check(got, ref, name, which, tol=TOL):
    """shape_cases.check_segments(got, ref, labels(name, which), tol): max |got - ref| <= tol max |ref| per segment of every interval, relative to
    the segment's own maximum with no floor (a segment that is identically zero must be exact zeros).  Returns {segment: relative error}."""
    uniq, order, starts = segments(name, which)
    a, b = np.asarray(got).reshape(-1), np.asarray(ref).reshape(-1)
    assert a.shape == b.shape == order.shape, (a.shape, b.shape, order.shape)
    assert np.all(np.isfinite(a)), "non-finite values in %s of %s" % (which, name)
    err = np.maximum.reduceat(np.abs(a - b)[order], starts)
    scale = np.maximum.reduceat(np.abs(b)[order], starts)
    out = {}
    for s, e, sc in zip(uniq, err, scale):
        out[str(s)] = float(e / sc) if sc > 0 else float(e)
        assert e <= tol * sc, "%s %s, segment %s: max err %.3e, max |ref| %.3e (rel %.3e > %.1e)" % (name, which, s, e, sc, out[str(s)], tol)
    return out


def moved(good, bad, name, which):
    """The largest relative move of a segment (a segment whose truth is zero counts by its absolute move)."""
    uniq, order, starts = segments(name, which)
    a, b = np.asarray(bad, dtype=np.float64).reshape(-1), np.asarray(good, dtype=np.float64).reshape(-1)
    err = np.maximum.reduceat(np.abs(a - b)[order], starts)
    scale = np.maximum.reduceat(np.abs(b)[order], starts)
    return float(np.where(scale > 0, err / np.where(scale > 0, scale, 1.0), err).max())


def compact_of(vals, name):
    kind, n, cols, m = CASES[name]
    return xc.compact_of_full(vals, n, cols, m)


# ---- the plans: the restatements, with what the kernels make of them spelled out -------------------------------------------------------------------
def _split(total, width, count):
    """What `count` units of `width` own of `total`: the kernels' max(0, min(width, total - u width))."""
    return [max(0, min(width, total - u * width)) for u in range(count)]


def _spell(p, n, cols, m):
    p = dict(p)
    p["nce"] = _split(cols, p["nc"], p["sx"])
    p["mge"] = _split(m, p["mg"], p["ngrp"])
    if "npc" in p:
        p["chain_units"] = p["sx"] * p["ngrp"]
        p["npce"] = _split(n, p["npc"], p["U"]) if p["npc"] else []
        p["cx"] = p["W"] - p["npc"]  # the chain's columns of a buffer
    else:
        p["pairs"] = p["ngrp"] * (p["ngrp"] + 1) // 2
    return p


def jac_plan(name, items=K, n_cu=256, cols_per_slice=0, general_slices=0, large_exp_drives=0):
    """The launch with values (FULL, COMPACT, MERIT): le.plan, keyed by the options' names."""
    kind, n, cols, m = CASES[name]
    return _spell(le.plan(n, cols, m, items=items, n_cu=n_cu, cols_per_slice=cols_per_slice, slices=general_slices, drives=large_exp_drives), n, cols, m)


def eval_plan(name, cols_per_slice=0):
    kind, n, cols, m = CASES[name]
    return _spell(le.plan(n, cols, m, jac=False, cols_per_slice=cols_per_slice), n, cols, m)


def payload_plan(name, items=K, n_cu=256, cols_per_slice=0, general_slices=0, large_exp_drives=0):
    kind, n, cols, m = CASES[name]
    p = xc.plan(n, cols, m, payload_only=True, items=items, n_cu=n_cu, cols_per_slice=cols_per_slice, slices=general_slices, drives=large_exp_drives)
    return _spell(p, n, cols, m)


def hess_plan(name, cols_per_slice=0, large_exp_hess_drives=0):
    kind, n, cols, m = CASES[name]
    return _spell(lh.plan(n, cols, m, cols_per_slice=cols_per_slice, drives=large_exp_hess_drives), n, cols, m)


def jac_row(p):
    return (p["U"], p["sx"], p["nc"], p["ngrp"], p["mg"], p["npc"], p["W"], p["NBW"], p["bytes"])


def payload_row(p):
    return (p["U"], p["sx"], p["nc"], p["ngrp"], p["mg"], p["W"], p["bytes"])


def eval_row(p):
    return (p["U"], p["nc"], p["W"], p["bytes"])


def hess_row(p):
    return (p["U"], p["sx"], p["nc"], p["ngrp"], p["mg"], p["W"], p["NBW"], p["bytes"])


def table_row(table, name, items=K, n_cu=256):
    """The committed row of a launch of `items` items of the case on n_cu CUs."""
    r = table[name] if name in table else table[(name, items)]
    return r[n_cu] if isinstance(r, dict) else r


def uneven(widths):
    return len(widths) > 1 and widths[-1] < widths[0]


def tiles(p):
    """16-column tiles of the widest unit's buffer: what the Horner loop's ct_n comes to."""
    return (p["W"] + 15) // 16


def forced_splits(name):
    """What the GPU tests force on a case, (options of the Jacobian family, options of the Hessian), each a list of dicts: cols_per_slice 1 and the
    widest cap up to 7 that leaves the last slice narrower than the first; general_slices = n; the drive caps 1, the largest that leaves the last group
    narrower than the first (else the largest that does not divide m) and m; and the three kinds at once."""
    kind, n, cols, m = CASES[name]
    jac, hess = [], []
    cj = ch = gj = gh = None
    if cols > 1:
        tries = range(min(cols - 1, 7), 1, -1)
        cj = next((c for c in tries if uneven(jac_plan(name, cols_per_slice=c)["nce"])), None)
        ch = next((c for c in tries if uneven(hess_plan(name, cols_per_slice=c)["nce"])), None)
        jac += [dict(cols_per_slice=c) for c in sorted({1, cj} - {None})]
        hess += [dict(cols_per_slice=c) for c in sorted({1, ch} - {None})]
    jac.append(dict(general_slices=n))
    if m > 1:
        tries = range(m - 1, 1, -1)
        odd = [g for g in tries if m % g]
        gj = next((g for g in tries if uneven(jac_plan(name, large_exp_drives=g)["mge"])), odd[0] if odd else None)
        gh = next((g for g in tries if uneven(hess_plan(name, large_exp_hess_drives=g)["mge"])), odd[0] if odd else None)
        jac += [dict(large_exp_drives=g) for g in sorted({1, gj, m} - {None})]
        hess += [dict(large_exp_hess_drives=g) for g in sorted({1, gh, m} - {None})]
    both = dict(general_slices=7)
    if cj:
        both["cols_per_slice"] = cj
    if gj:
        both["large_exp_drives"] = gj
    jac.append(both)
    if ch and gh:
        hess.append(dict(cols_per_slice=ch, large_exp_hess_drives=gh))
    return jac, hess


# ---- the three mutants of the new regimes ---------------------------------------------------------------------------------------------------------
def hess_scalars(name):
    kind, n, cols, m = CASES[name]
    return (m + 1) * (m + 2) // 2


def as_if_full_hess(name, nce):
    """The Hessian's values with the last slice (nce: the slices' columns) computed as if full: the scalars count the last column once more per
    missing column.  None where no column is missing."""
    missing = nce[0] - nce[-1]
    if missing <= 0:
        return None
    lay, G0, Gj, Z = case(name)
    per = eht.nnz_per_interval(lay)
    good = np.array(emulated_hess(name)).reshape(K, per)
    less = lh.emulate_hess(lay, G0, Gj, Z, mu(name), drop_col=True).reshape(K, per)
    ns = hess_scalars(name)
    good[:, :ns] += missing * (good[:, :ns] - less[:, :ns])
    return good.reshape(-1)


def as_if_full_payload(name, nce, explicit):
    """The payload likewise, in longdouble from the emulated values."""
    missing = nce[0] - nce[-1]
    if missing <= 0:
        return None
    d, v = emulated(name)
    good, less = payload(name, d, v, explicit)[0], payload(name, d, v, explicit, drop_col=True)[0]
    return good + missing * (good - less)


def first_group_size_hess(name, mge):
    """The Hessian's values with the pairs of a short last group taken with the first group's size: (dt, u_l) of the drives of the other groups zero."""
    if not uneven(mge):
        return None
    kind, n, cols, m = CASES[name]
    lay = layout(name)
    out = np.array(emulated_hess(name)).reshape(K, eht.nnz_per_interval(lay))
    npair = m * (m + 1) // 2
    out[:, npair : npair + m - mge[-1]] = 0.0
    return out.reshape(-1)


def first_group_size_payload(name, mge, explicit):
    """The payload with a short last group run at the first group's size: drive m's slot is the dt slot, so g_dt is zero."""
    if not uneven(mge):
        return None
    kind, n, cols, m = CASES[name]
    out = np.array(payload(name, *emulated(name), explicit)[0])
    out[1 + K * m :] = 0
    return out


def second_tile(name, p):
    """(delta, full values) of the emulation with the buffer columns 16 .. 31 of every unit of the plan p never run, or None where no unit has them."""
    kind, n, cols, m = CASES[name]
    lay, G0, Gj, Z = case(name)
    if p["W"] <= 16:
        return None
    d, v = (np.array(a) for a in emulated(name))
    d, v = d.reshape(K, cols, n), v.reshape(K, xc.full_per(n, cols, m))
    nn, nc, mg, cx = n * n, p["nc"], p["mg"], p["cx"]
    for k in range(K):
        X, Xn = lay.X(Z, k), lay.X(Z, k + 1)
        E = v[k, : cols * nn].reshape(cols, n, n)  # [copy][column][row], a view
        tails = v[k, cols * nn + cols * n :].reshape(cols, m + 1, n)  # [column][l | dt][row], a view
        for u in range(p["U"]):
            chain = u < p["chain_units"]
            s, g = (u % p["sx"], u // p["sx"]) if chain else (0, 0)
            nce, mge, npce = (p["nce"][s], p["mge"][g], p["npce"][u]) if chain else (0, 0, p["npce"][u])
            ucx = cx if chain else 0
            for vcol in range(16, 32):
                if vcol >= ucx:
                    c = vcol - ucx
                    if c < npce:
                        j = u * p["npc"] + c
                        E[:, j, :] = 0.0
                        E[:, j, j] = -1.0
                    continue
                bl, c = divmod(vcol, nc)
                if c >= nce:
                    continue
                col = s * nc + c
                if bl == 0 and g == 0:  # V stays X_k: delta = X_{k+1} - X_k, the dt tail -G X_k
                    d[k, col] = Xn[:, col] - X[:, col]
                    tails[col, m] = -(vc.g_of(lay, Z, k, G0, Gj) @ X[:, col])
                elif bl >= 1 and bl - 1 < mge:
                    tails[col, g * mg + bl - 1] = 0.0
    return d.reshape(-1), v.reshape(-1)


# ---- faults of the products, through the `mm` hook ---------------------------------------------------------------------------------------------------
mm_drop_k_beyond_64 = le.mm_drop_k_beyond_64
mm_zero_last_row_tile = le.mm_zero_last_row_tile
