"""Cases that walk the large-generator Pade kernels (contexts created with PCL_LARGE_N, generator dimensions 66 .. 128) over the regimes of their launch
plans that the nine systems of tests/large_shape_cases.py never enter: the residual + Jacobian family with its compact, merit and payload modes
(piccolo.jl_amd/csrc/pcl_kernel_pade_large.hpp, planned by large_plan in pcl_host_launch_pade.hpp, restated as lc.large_plan) and the Hessian of the
Lagrangian (pcl_kernel_pade_large_hess.hpp, large_hess_plan in pcl_host_launch_hess.hpp, restated as hc.hess_plan).  Importable without a GPU.

Generators, knots (N = 4) and the three steps per interval follow the recipe of lc.system / lc.case -- h |G|_2 = 0.15, -0.3 and the long step of
vc.LONG_STEPS -- with seeds of their own (16000 + 17 index); multipliers: standard normals, seeds 16000 + 17 index + 77 (Hessian) and + 177 (payload).
The truth is vector_shape_cases.truth_values in np.longdouble, computed once per (case, order) and never written to; the payload's truth is
large_reduce_cases.payload_ld on that truth.

Cases (kind, n, cols, m), what each sits on, and what the plans give for the three intervals of a test launch on 256 CUs (TABLE / HESS_TABLE below;
tests/test_large_plan_cpu.py asserts every number, at 304 and 128 CUs as well):
    P1  iso 120 60  4   a bench shape (d = 60): 48 chain units against 40 panel units -- eight     J U 48 = 12 x 4, nc 5, mg 1, npc 3, 158,904 B
                        units own no power column                                                  H U 80 = 20 x 4, nc 3, mg 1, 158,080 B
    P2  iso 128 64  2   the largest state (x_dim 8192): slices 3, .., 3, 1; the residual alone     J U 44 = 22 x 2, nc 3, mg 1, npc 3, 161,064 B
                        takes slices 7, .., 7, 1                                                   H U 64 = 32 x 2, nc 2, mg 1, 162,160 B
    P3  iso  96 48  4   the other bench shape (d = 48)                                             J U 16 = 4 x 4, nc 12, mg 1, npc 6, 154,768 B
                                                                                                   H U 24 = 6 x 4, nc 8, mg 1, 162,912 B
    P4  vec 100  1  5   the ten-level density vector: 448 threads (seven waves), n mod 16 = 4      J U 7, mg 5, npc 15 (last 10), 106,976 B
                                                                                                   H U 1, mg 5, 106,416 B
    P5  iso 104  1  0   no drive at all, at 448 threads                                            J U 7, mg 0, npc 15 (last 14), 106,088 B
                                                                                                   H U 1, mg 0, 96,856 B
    P6  iso  80  7  7   Hessian drive groups 3, 3, 1 chosen by the plan                            J U 5, nc 7, mg 7, npc 16, 154,072 B
                                                                                                   H U 3, nc 7, mg 3 (3, 3, 1), 154,176 B
    P7  iso 112 13  5   slices 7 + 6, five groups of one drive, the last panel unit 2 columns;     J U 11 = 2 x 5 + 1, npc 11 (last 2), 162,944 B
                        Hessian slices 4, 4, 4, 1                                                  H U 20 = 4 x 5, nc 4, mg 1, 153,224 B
    P8  iso  88  3 11   Hessian drive groups 6 + 5                                                 J U 6, nc 3, mg 11, npc 15 (last 13), 134,320 B
                                                                                                   H U 2, nc 3, mg 6 (6, 5), 138,208 B
    P9  vec  67  1  6   odd n one past 66: LD = n, straddling pairs                                J U 5, mg 6, npc 14 (last 11), 54,200 B
                                                                                                   H U 1, mg 6, 55,616 B
Long launches (LONG below): the case's own four knots as 29 and as 100 seeds of one PCL_BATCH_TRAJ launch -- 87 and 300 items, so that
n_cu / items is 2 and 0 -- on P4, P6, P8, P9 and lc's L2 (n = 96, one ket), and P1 once at 87 items (the plan does not move: 4,176 workgroups).

Orders: 2 .. 10 on P4 .. P9; 4 and 10 on the three unitary cases, whose longdouble truths are the cost of the module (TRUTH_SECONDS, one CPU core:
none takes more than three seconds, so no case's Hessian had to be cut to order 4)."""
import functools

import numpy as np

import large_hess_cases as hc
import large_reduce_cases as rc
import large_shape_cases as lc
import vector_shape_cases as vc
from oracle import pade_oracle as po
from shape_cases import check_segments, hess_labels, jac_labels  # noqa: F401  (re-exported for the two test files)

N = lc.N
K = N - 1
LDS_BYTES = lc.LDS_BYTES
TOL = 1e-11
SEEN = 1e-7

# name: (kind, n, cols, m)
CASES = {
    "P1": ("iso", 120, 60, 4), "P2": ("iso", 128, 64, 2), "P3": ("iso", 96, 48, 4), "P4": ("vec", 100, 1, 5), "P5": ("iso", 104, 1, 0),
    "P6": ("iso", 80, 7, 7), "P7": ("iso", 112, 13, 5), "P8": ("iso", 88, 3, 11), "P9": ("vec", 67, 1, 6),
}  # fmt: skip
NAMES = list(CASES)
UNITARY = ("P1", "P2", "P3")
ORDERS = {name: ((4, 10) if name in UNITARY else lc.ORDERS) for name in NAMES}
LONG_NAMES = ["L2", "P4", "P6", "P8", "P9"]
SEEDS = {87: 29, 300: 100}  # items of a long launch: trajectories of three intervals

# what large_plan gives for a Jacobian launch of the three intervals: (U, sx, ngrp, mg, npc, bytes); it reads n_cu, and gives the same at 304 and 128 CUs
TABLE = {
    "P1": (48, 12, 4, 1, 3, 158904), "P2": (44, 22, 2, 1, 3, 161064), "P3": (16, 4, 4, 1, 6, 154768), "P4": (7, 1, 1, 5, 15, 106976),
    "P5": (7, 1, 1, 0, 15, 106088), "P6": (5, 1, 1, 7, 16, 154072), "P7": (11, 2, 5, 1, 11, 162944), "P8": (6, 1, 1, 11, 15, 134320),
    "P9": (5, 1, 1, 6, 14, 54200),
}  # fmt: skip
# ... the state columns of its slices and the power columns of its last three units
SPLIT = {
    "P1": ([5] * 12, [0, 0, 0]), "P2": ([3] * 21 + [1], [3, 2, 0]), "P3": ([12] * 4, [6, 6, 6]), "P4": ([1], [15, 15, 10]), "P5": ([1], [15, 15, 14]),
    "P6": ([7], [16, 16, 16]), "P7": ([7, 6], [11, 11, 2]), "P8": ([3], [15, 15, 13]), "P9": ([1], [14, 14, 11]),
}  # fmt: skip
# what large_hess_plan gives (it does not read n_cu): (U, sx, nc, ngrp, mg, bytes), the slices' columns, the groups' drives
HESS_TABLE = {
    "P1": ((80, 20, 3, 4, 1, 158080), [3] * 20, [1] * 4), "P2": ((64, 32, 2, 2, 1, 162160), [2] * 32, [1, 1]),
    "P3": ((24, 6, 8, 4, 1, 162912), [8] * 6, [1] * 4), "P4": ((1, 1, 1, 1, 5, 106416), [1], [5]), "P5": ((1, 1, 1, 1, 0, 96856), [1], [0]),
    "P6": ((3, 1, 7, 3, 3, 154176), [7], [3, 3, 1]), "P7": ((20, 4, 4, 5, 1, 153224), [4, 4, 4, 1], [1] * 5),
    "P8": ((2, 1, 3, 2, 6, 138208), [3], [6, 5]), "P9": ((1, 1, 1, 1, 6, 55616), [1], [6]),
}  # fmt: skip
# the residual-only launch: (U, nc, bytes) and the slices' columns
EVAL_TABLE = {
    "P1": ((5, 12, 163744), [12] * 5), "P2": ((10, 7, 162096), [7] * 9 + [1]), "P3": ((2, 24, 150112), [24, 24]), "P4": ((1, 1, 85160), [1]),
    "P5": ((1, 1, 91808), [1]), "P6": ((1, 7, 71128), [7]), "P7": ((1, 13, 149384), [13]), "P8": ((1, 3, 72376), [3]), "P9": ((1, 1, 39192), [1]),
}  # fmt: skip
# long launches, (system, items, CUs): (U, npc, power columns per unit, B+- pairs per thread, bytes)
LONG = {
    ("L2", 87, 256): (2, 48, [48, 48], 6, 122168), ("L2", 300, 256): (2, 48, [48, 48], 6, 122168),
    ("P4", 87, 256): (2, 50, [50, 50], 6, 135256), ("P4", 300, 256): (2, 50, [50, 50], 6, 135256),
    ("P6", 87, 256): (3, 27, [27, 27, 26], 4, 161200), ("P6", 300, 256): (3, 27, [27, 27, 26], 4, 161200),
    ("P8", 87, 256): (2, 44, [44, 44], 6, 154968), ("P8", 300, 256): (2, 44, [44, 44], 6, 154968),
    ("P9", 87, 256): (2, 34, [34, 33], 4, 64920), ("P9", 300, 256): (1, 67, [67], 8, 82608),
    # 304 CUs: 304 // 87 = 3 units;  128 CUs: 128 // 87 = 1, so the `fits` loop alone decides (one panel fits only at n = 67)
    ("L2", 87, 304): (3, 32, [32, 32, 32], 4, 109752), ("L2", 87, 128): (2, 48, [48, 48], 6, 122168),
    ("P4", 87, 304): (3, 34, [34, 34, 32], 4, 122328), ("P4", 87, 128): (2, 50, [50, 50], 6, 135256),
    ("P6", 87, 304): (3, 27, [27, 27, 26], 4, 161200), ("P6", 87, 128): (3, 27, [27, 27, 26], 4, 161200),
    ("P8", 87, 304): (3, 30, [30, 30, 28], 4, 145000), ("P8", 87, 128): (2, 44, [44, 44], 6, 154968),
    ("P9", 87, 304): (3, 23, [23, 23, 21], 3, 59024), ("P9", 87, 128): (1, 67, [67], 8, 82608),
    ("L2", 300, 304): (2, 48, [48, 48], 6, 122168), ("L2", 300, 128): (2, 48, [48, 48], 6, 122168),
    ("P9", 300, 304): (1, 67, [67], 8, 82608), ("P9", 300, 128): (1, 67, [67], 8, 82608),
}  # fmt: skip
# seconds of one longdouble truth on one CPU core, measured, (case, order): (residual + Jacobian, Hessian with both); building a unitary case (its
# long step: two order-10 residuals of one interval) takes 0.6 .. 1.1 s more.  No other case takes more than 0.8 s for anything
TRUTH_SECONDS = {
    ("P1", 4): (0.3, 0.5), ("P1", 10): (1.7, 2.9), ("P2", 4): (0.3, 0.4), ("P2", 10): (1.3, 2.1), ("P3", 4): (0.2, 0.3), ("P3", 10): (0.8, 1.5),
}  # fmt: skip


def shape(name):
    return CASES[name] if name in CASES else lc.CASES[name]


def _seed(name):
    return 16000 + 17 * int(name[1:])


# ---- systems and trajectories, by the recipe of lc.system / lc.case ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def system(name):
    kind, n, cols, m = CASES[name]
    rng = np.random.default_rng(_seed(name))
    if kind == "vec":
        G0 = rng.standard_normal((n, n)) / np.sqrt(n)
        Gj = rng.standard_normal((m, n, n)) / np.sqrt(n)
    else:
        G0 = po.G_of_H(vc._herm(n // 2, rng))
        Gj = np.array([po.G_of_H(vc._herm(n // 2, rng)) for _ in range(m)]).reshape(m, n, n)
    return G0, Gj


def layout(name):
    if name in lc.CASES:
        return lc.layout(name)
    kind, n, cols, m = CASES[name]
    xs = n * cols
    if kind == "vec":
        return po.Layout(d=0, m=m, N=N, z_dim=xs + 2 + m, x_off=0, u_off=xs + 2, dt_off=xs, cols=1, gen=n)
    return po.Layout(d=n // 2, m=m, N=N, z_dim=xs + 2 + m, x_off=0, u_off=xs + 2, dt_off=xs, cols=cols)


@functools.lru_cache(maxsize=None)
def case(name):
    """(layout, G0, Gj, Z, long step), read-only: lc.case for L2, the same recipe for P1 .. P9."""
    if name in lc.CASES:
        return lc.case(name)
    lay = layout(name)
    G0, Gj = system(name)
    rng = np.random.default_rng(_seed(name) + 1)
    Z = 0.4 * rng.standard_normal((N, lay.z_dim))
    n2 = [np.linalg.norm(vc.g_of(lay, Z, k, G0, Gj), 2) for k in range(K)]
    Z[0, lay.dt_off], Z[1, lay.dt_off], Z[N - 1, lay.dt_off] = 0.15 / n2[0], -0.3 / n2[1], 0.1
    long_step = None
    for s in vc.LONG_STEPS:
        Z[2, lay.dt_off] = s / n2[2]
        if vc.top_term_weight(lay, G0, Gj, Z) >= SEEN:
            long_step = s
            break
    assert long_step is not None, name
    Z[:, lay.dt_off + 1] = np.cumsum(Z[:, lay.dt_off])
    for a in (G0, Gj, Z):
        a.setflags(write=False)
    return lay, G0, Gj, Z, long_step


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def rand_mu(name):
    lay = layout(name)
    return _ro(np.random.default_rng((_seed(name) if name in CASES else 15000 + 17 * int(name[1:])) + 77).standard_normal(lay.K * lay.x_dim))[0]


@functools.lru_cache(maxsize=None)
def lam(name):
    """The payload's explicit multipliers: a standard normal of delta's shape [K, cols, n]."""
    kind, n, cols, m = shape(name)
    return _ro(np.random.default_rng((_seed(name) if name in CASES else 15000 + 17 * int(name[1:])) + 177).standard_normal((K, cols, n)))[0]


# ---- the truth, computed once per (case, order) and never written to ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def truth_ld(name, order):
    """(delta, Jacobian values), flat, in longdouble."""
    if name in lc.CASES:
        return lc.truth_ld(name, order)
    lay, G0, Gj, Z, _ = case(name)
    d, j, _ = vc.truth_values(lay, G0, Gj, Z, None, order, hessian=False)
    return _ro(d.reshape(-1), j.reshape(-1))


@functools.lru_cache(maxsize=None)
def truth(name, order):
    """The same rounded to float64: what the GPU tests compare with."""
    return _ro(*(a.astype(np.float64) for a in truth_ld(name, order)))


@functools.lru_cache(maxsize=None)
def hess_truth_ld(name, order):
    lay, G0, Gj, Z, _ = case(name)
    return _ro(vc.truth_values(lay, G0, Gj, Z, rand_mu(name), order, hessian=True)[2].reshape(-1))[0]


@functools.lru_cache(maxsize=None)
def hess_truth(name, order):
    return _ro(hess_truth_ld(name, order).astype(np.float64))[0]


@functools.lru_cache(maxsize=None)
def payload_truth(name, order, explicit):
    """[phi | g_u | g_dt] in float64 from the longdouble truth: lam = delta (explicit False) or lam(name)."""
    d, j = truth_ld(name, order)
    return _ro(rc.payload_ld(shape(name), [d], [j], [lam(name)] if explicit else None).astype(np.float64))[0]


def compact_of(vals, name):
    kind, n, cols, m = shape(name)
    return rc.compact_of(vals, n, cols, m)


def compact_labels(name):
    kind, n, cols, m = shape(name)
    return rc.compact_labels(n, cols, m)


# ---- the per-segment rule of shape_cases.check_segments, with the labels sorted once per case ----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def segments(name, which):
    """(segment names, a permutation that sorts the values by segment, each segment's start in it) for the labels of `which`: "delta", "jac"
    (shape_cases.jac_labels), "hess" (hess_labels), "compact", "payload".  P2's Jacobian has 6.3 million labels: sorted once, not per comparison."""
    lay = layout(name)
    kind, n, cols, m = shape(name)
    labels = {"delta": lambda: lc.residual_labels(lay), "jac": lambda: jac_labels(lay), "hess": lambda: hess_labels(lay),
              "compact": lambda: compact_labels(name), "payload": lambda: rc.payload_labels(m)}[which]()  # fmt: skip
    uniq, inv = np.unique(labels, return_inverse=True)
    inv = inv.reshape(-1)
    order = np.argsort(inv, kind="stable")
    return _ro(uniq, order, np.searchsorted(inv[order], np.arange(uniq.size)))


def check(got, ref, name, which, tol=TOL):
    """shape_cases.check_segments(got, ref, the labels of `which`, tol): max |got - ref| <= tol max |ref| per segment, relative to the segment's own
    maximum with no floor (a segment that is identically zero must be exact zeros).  Returns {segment: relative error}."""
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


# ---- the plans -------------------------------------------------------------------------------------------------------------------------------
def jac_plan(name, **kw):
    kind, n, cols, m = shape(name)
    return lc.large_plan(n, cols, m, **kw)


def hess_plan(name, **kw):
    kind, n, cols, m = shape(name)
    return hc.hess_plan(n, cols, m, **kw)


def ragged_groups(h):
    return h["mge"][-1] < h["mge"][0]


def forced_splits(name, n_cu=256, items=K):
    """What the GPU tests force on a case, each a dict of options: cols_per_slice 1, 2 and one that leaves an uneven last slice; general_slices = n
    (one power column per unit) and one above the default U of a launch of `items` items; large_hess_drives 1, 2 and one that does not divide m."""
    kind, n, cols, m = shape(name)
    jac, hess = [], []
    if cols > 1:
        # the widest cap up to 7 under which the plan's last slice is narrower than its first (the plan evens the slices, and what fits caps the cap):
        # in the Jacobian launch, else in the residual-only launch (P1, P2: 60 and 64 columns in slices of at most 5 and 3 come out even)
        tries = range(min(cols - 1, 7), 2, -1)
        ragged = lambda plan: plan["nce"][-1] < plan["nce"][0]
        uj = next((c for c in tries if ragged(lc.large_plan(n, cols, m, cols_per_slice=c))), None)
        ue = next((c for c in tries if ragged(lc.large_plan(n, cols, m, jac=False, cols_per_slice=c))), None)
        uh = next((c for c in tries if ragged(hc.hess_plan(n, cols, m, cols_per_slice=c))), None)
        jac += [dict(cols_per_slice=c) for c in sorted({1, 2, uj or ue} - {None})]
        hess += [dict(cols_per_slice=c) for c in sorted({1, 2, uh} - {None})]
    jac += [dict(general_slices=n), dict(general_slices=min(n, jac_plan(name, items=items, n_cu=n_cu)["U"] + 1))]
    if m > 1:
        # a cap that does not divide m: the largest under which the evened groups still end in a narrower one (m = 5: 2 -> 2, 2, 1), else the
        # largest at all (m = 4, 6: every cap comes out even -- 3 -> 2, 2 and 5 -> 3, 3)
        odd = [g for g in range(m - 1, 1, -1) if m % g]
        ug = next((g for g in odd if ragged_groups(hc.hess_plan(n, cols, m, drives=g))), odd[0] if odd else None)
        hess += [dict(large_hess_drives=g) for g in sorted({1, 2, ug} - {None}) if g < m]
    return jac, hess


# ---- faults -------------------------------------------------------------------------------------------------------------------------------------
def mm_zero_rows_from(n, r0):
    """Every product with the rows from r0 on (per block of n rows of its output) left at zero: the row tiles a workgroup of 384 threads never had."""

    def mm(A, B):
        Cm = A @ B
        Cm[np.arange(Cm.shape[0]) % n >= r0] = 0
        return Cm

    return mm


def zero_pair_slots(jac_vals, name, npce, first_slot):
    """A copy of the full Jacobian values in which, in every unit's panel of -B+ and B- (npce power columns per unit, n npce values contiguous from
    column u npc on), the flat positions from 2 threads first_slot on are zero: what a thread's B+- pair slots r >= first_slot hold (slot r of thread
    tid owns the positions 2 (tid + threads r) and the next one).  In columns of an even n: from index 2 threads first_slot / n of the panel on."""
    kind, n, cols, m = shape(name)
    threads = 64 * ((n + 15) // 16)
    v = np.array(jac_vals).reshape(-1, rc.full_per(n, cols, m))
    dead = np.zeros(n * n, bool)
    c0 = 0
    for w in npce:
        dead[c0 * n + 2 * threads * first_slot : (c0 + w) * n] = True
        c0 += w
    for k in range(v.shape[0]):
        v[k, : 2 * cols * n * n].reshape(2 * cols, n * n)[:, dead] = 0  # every copy of -B+ and of B-, a view
    return v.reshape(-1)


# the fault each of these cases exists for: (what, keywords of vc.truth_values | pair slots of the long launch's plan on 256 CUs)
MUTANT_NAMES = ["P2", "P7", "P6", "P8", "L2", "P9", "P4"]
MUTANT_ORDER = 4


@functools.lru_cache(maxsize=None)
def mutants(name, order=MUTANT_ORDER):
    """{what: (delta, Jacobian values, Hessian values | None)} in longdouble, flat: the truth with the fault the case exists for.
        P2, P7   the last state column dropped                      P6, P8   the last drive (of the last Hessian group) dropped
        L2, P9   the pair slots r >= 1 (the issue's column index 2 threads / n) and r >= 2 (a thread's third and later pairs) of the 87-item launch's
                 panels zeroed; P9 also the eighth slot of the 300-item launch's one panel
        P4       the rows beyond 96 of every product zeroed (the seventh wave)"""
    lay, G0, Gj, Z, _ = case(name)
    d, j = truth_ld(name, order)
    out = {}

    def run(what, **kw):
        r = vc.truth_values(lay, G0, Gj, Z, rand_mu(name), order, hessian=True, **kw)
        out[what] = _ro(*(a.reshape(-1) for a in r))

    if name in ("P2", "P7"):
        run("last state column", drop_col=True)
    elif name in ("P6", "P8"):
        run("last drive", drop_drive=True)
    elif name == "P4":
        run("rows beyond 96", mm=mm_zero_rows_from(100, 96))
    else:
        npce = LONG[(name, 87, 256)][2]
        for slot in (1, 2):
            out["pair slots from %d" % slot] = _ro(d, zero_pair_slots(j, name, npce, slot)) + (None,)
        if name == "P9":
            out["the eighth pair slot of one panel"] = _ro(d, zero_pair_slots(j, name, LONG[(name, 300, 256)][2], 7)) + (None,)
    return out


def moved(good, bad, labels):
    """The largest relative change of a segment (against the segment's own maximum)."""
    good, bad = np.asarray(good).reshape(-1), np.asarray(bad).reshape(-1)
    out = 0.0
    for s in np.unique(labels):
        sel = labels == s
        scale = np.abs(good[sel]).max()
        if scale > 0:
            out = max(out, float(np.abs(bad[sel] - good[sel]).max() / scale))
    return out
