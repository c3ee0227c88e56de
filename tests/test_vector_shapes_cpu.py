"""The cases of tests/vector_shape_cases.py before any GPU is involved: that each can do its job in tests/test_vector_shapes_gpu.py.

Reference floor: for every case and order in (2, 4, 6, 8, 10) po.pade_residual, po.pade_jacobian_values and po.pade_hessian_values agree with
the longdouble truth per segment to 1e-13 of the segment's own maximum -- a condition on the inputs, which leaves the GPU comparison at 1e-11
a factor 100 for the kernels' summation order.  Largest value read per output kind (segment, case, order):
    residual 4.4e-16 (delta@0, V5, order 10)    Jacobian 4.4e-16 (B+@0, V5, order 8)    Hessian 6.8e-15 (uu@1, K4, order 4)

Sensitivity: every case sees each fault its kernels' shape handling could have, applied to the truth alone, in at least one segment the fault
touches at 1e-7 relative or more (1e4 x the GPU tolerance): the top coefficient c_q zeroed (interval 2, every order); every product's last
k step of 4 and last 16-row tile dropped; the last state column, the last drive and (K7) the last drive pair ignored.

The case table's slice, pair, chunk and byte counts are recomputed with the launch code's arithmetic.

The structure through the C ABI (pcl_jac_structure, pcl_hess_structure on M2 and V5, index bases 0 and 1) needs a context, and a context needs
a device: that comparison is in tests/test_vector_shapes_gpu.py.  Here: po.jac_structure / po.hess_structure name every position once."""
import numpy as np
import pytest

import vector_shape_cases as vc
from exp_shape_cases import mm_drop_last_k_step, mm_drop_last_row_tile
from oracle import pade_oracle as po
from shape_cases import check_segments, hess_labels, jac_labels

FLOOR = 1e-13
GPU_TOL = 1e-11
SEEN = 1e4 * GPU_TOL
NAMES = list(vc.CASES)
_floors = {}


def worst(errs):
    s = max(errs, key=errs.get)
    return errs[s], s


def seen(good, bad, labels, only=None):
    """The largest relative change of a segment (against the segment's own maximum); only: a suffix the segment's label must have."""
    out = 0.0
    for s in np.unique(labels):
        if only and not s.endswith(only):
            continue
        sel = labels == s
        scale = np.abs(good[sel]).max()
        if scale > 0:
            out = max(out, float(np.abs(bad[sel] - good[sel]).max() / scale))
    return out


# ---- the case table's claims ----------------------------------------------------------------------------------------------------------------------
def test_case_table_sits_where_the_launch_code_branches():
    C = vc.CASES
    plan = {name: vc.lockstep_plan(n, cols, m) for name, (kind, n, cols, m) in C.items()}
    for name, (kind, n, cols, m) in C.items():  # the lock-step kernel takes every even n, within the LDS
        assert (plan[name] is not None) == (n % 2 == 0), name
        if plan[name]:
            assert plan[name]["bytes"] <= vc.LDS_BYTES, name
            assert plan[name]["S"] == cols and plan[name]["nc"] == 1  # three intervals: as many slices as state columns
    # row tiles, idle waves, B+- pairs
    assert plan["V2"]["row_tiles"] == 1 and plan["K1"]["row_tiles"] == 2 and plan["K2"]["row_tiles"] == 3 and plan["K6"]["row_tiles"] == 4
    assert plan["K2"]["idle_waves"] == 1 and 34 - 32 == 2 and plan["V4"]["idle_waves"] == 1 and plan["K6"]["idle_waves"] == 0
    assert plan["K3"]["pairs"] == 1 and 44 * 44 // 2 == 968 and plan["K4"]["pairs"] == 2 and plan["K4"]["last_pair_used"] == 34
    assert plan["K6"]["pairs"] == 2 and plan["K6"]["last_pair_used"] == 1024 and plan["V7"]["last_pair_used"] == 1024
    # slices
    assert plan["M1"]["npc"] == 3 and plan["M1"]["npce"] == [3, 3, 3, 3, 0] and plan["M1"]["nce"] == [1] * 5
    assert plan["M2"]["npc"] == 3 and plan["M2"]["npce"] == [3] * 6 + [2]
    assert plan["M3"]["npc"] == 9 and plan["M3"]["npce"] == [9] * 6 + [6]
    assert plan["M4"]["npc"] == 11 and plan["M4"]["npce"] == [11] * 4 + [10]
    for slices in (1, 2):  # the forced slice counts of the GPU test: more than one state column per slice, the last one short
        p = vc.lockstep_plan(20, 7, 2, slices=slices)
        assert p["S"] == slices and p["nc"] == (7, 4)[slices - 1] and p["nce"][-1] == (7, 3)[slices - 1]
    # the general Hessian's column chunks and rows
    assert vc.hess_general_chunk(60, 7, 6) == (2, [2, 2, 2, 1]) and vc.hess_general_bytes(60, 6, 4) > vc.LDS_BYTES >= vc.hess_general_bytes(60, 6, 2)
    assert vc.hess_general_chunk(20, 7, 2)[0] == 7 and vc.hess_general_chunk(12, 5, 4)[0] == 5
    assert 24 * 25 // 2 == 300 and 25 * 26 // 2 == 325 and vc.hess_general_bytes(10, 24, 1) <= vc.LDS_BYTES and 6 * 7 // 2 == 21
    for name, (kind, n, cols, m) in C.items():
        assert vc.hess_general_bytes(n, m, vc.hess_general_chunk(n, cols, m)[0]) <= vc.LDS_BYTES, name
        # the reference formulation holds every state column of every case in one workgroup, with the Jacobian as well but for M3's seventh
        assert vc.reference_cols(n, cols, m, 5, False) == cols and vc.reference_cols(n, cols, m, 5, True) == (6 if name == "M3" else cols), name
    # the order-4 kernels: kernel 10 up to d = 16, kernel 20 above; Hessian kernel 2 on K5's two-entry drives, kernel 1 on dense drives
    assert vc.drive_width(vc.system("K5")[1]) == 2 and vc.drive_width(vc.system("K2")[1]) > 2
    assert vc.hess2_lds_bytes(54, 6) <= vc.LDS_BYTES
    assert [vc.expected_family(c, 4)[0] for c in ("K1", "K2", "M1", "M2", "M3", "K7")] == [10, 20, 10, 10, 20, 10]
    assert vc.expected_family("K5", 4) == vc.expected_family("M4", 4) == (20, 20, 2) and vc.drive_width(vc.system("M4")[1]) == 2 and vc.expected_family("K2", 4) == (20, 20, 1)
    for name in ("K1", "K7", "M1", "M2"):
        n, cols, m = C[name][1:]
        assert vc.fused_lds_bytes(n, m, 1, True) <= vc.LDS_BYTES and vc.hess1_lds_bytes(n, m, cols) <= vc.LDS_BYTES // 2
    for name in ("K2", "K5", "K6", "M3"):
        n, cols, m = C[name][1:]
        assert vc.fused2_lds_bytes(n, m, 1, True, 2 if name == "K5" else 0) <= vc.LDS_BYTES  # (K5's two-entry drive rows are staged in LDS)
    assert vc.hess1_lds_bytes(60, 6, 7) > vc.LDS_BYTES // 2 >= vc.hess1_lds_bytes(60, 6, 4)  # M3 in kernel 1: chunks of 4 and 3 columns
    # the small kernel: n <= 16, cols <= 8, m <= 8 -- the residual alone above 8 rows
    assert [vc.expected_family(c, 10)[1] for c in ("M1", "V1", "V2", "V3", "K7", "K1")] == [55, 55, 55, 95, 95, 95]
    assert [vc.expected_family(c, 10)[0] for c in ("M1", "V1", "V2", "V3", "K7")] == [195, 95, 195, 95, 195]
    assert vc.expected_family("V2", 4) == (192, 52, 1) and vc.expected_family("V3", 4) == (92, 92, 1)


@pytest.mark.parametrize("name", NAMES)
def test_steps(name):
    lay, G0, Gj, Z, long_step = vc.case(name)
    th = [Z[k, lay.dt_off] * np.linalg.norm(vc.g_of(lay, Z, k, G0, Gj), 2) for k in range(lay.K)]
    assert np.allclose(th, [0.15, -0.3, long_step], rtol=1e-12)
    w = vc.top_term_weight(lay, G0, Gj, Z)
    assert w >= SEEN
    if long_step > vc.LONG_STEPS[0]:  # the smallest that does
        Zs = vc.with_step(lay, G0, Gj, Z, 2, vc.LONG_STEPS[vc.LONG_STEPS.index(long_step) - 1])
        assert vc.top_term_weight(lay, G0, Gj, Zs) < SEEN
    print("%s: long step %.2f, c_5 moves the residual by %.1e" % (name, long_step, w))


# ---- the reference floor ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_oracle_floor(name):
    lay, G0, Gj, Z, _ = vc.case(name)
    for order in vc.ORDERS:
        d, j, mu, h = vc.truth(name, order)
        er = check_segments(po.pade_residual(Z, lay, G0, Gj, order), d, vc.residual_labels(lay), FLOOR)
        ej = check_segments(po.pade_jacobian_values(Z, lay, G0, Gj, order), j, jac_labels(lay), FLOOR)
        eh = check_segments(po.pade_hessian_values(Z, mu.reshape(lay.K, -1), lay, G0, Gj, order), h, hess_labels(lay), FLOOR)
        for kind, e in (("residual", er), ("Jacobian", ej), ("Hessian", eh)):
            v, s = worst(e)
            if v > _floors.get(kind, (0.0,))[0]:
                _floors[kind] = (v, s, name, order)
        print("%s order %d: residual %.1e (%s)  Jacobian %.1e (%s)  Hessian %.1e (%s)" % ((name, order) + worst(er) + worst(ej) + worst(eh)))
    print("reference floor so far: " + "  ".join("%s %.1e (%s, %s, order %d)" % ((k,) + v) for k, v in _floors.items()))


def test_oracle_floor_of_the_batched_members():
    """The other members of the batched cases of the GPU test: K2's second drift, V5's second seed, M2's members 1 and 2 of a three-state knot."""
    for name, kw in (("K2", dict(drift=1)), ("V5", dict(seed=1)), ("M2", dict(members=3, member=1)), ("M2", dict(members=3, member=2))):
        lay, G0, Gj, Z, _ = vc.case(name, kw.get("seed", 0), kw.get("drift", 0), kw.get("members", 1))
        xo = kw.get("member", 0) * lay.x_dim
        for order in (4, 8):
            d, j, mu, h = vc.truth(name, order, **kw)
            check_segments(po.pade_residual(Z, lay, G0, Gj, order, x_off=xo), d, vc.residual_labels(lay), FLOOR)
            check_segments(po.pade_jacobian_values(Z, lay, G0, Gj, order, x_off=xo), j, jac_labels(lay), FLOOR)
            check_segments(po.pade_hessian_values(Z, mu.reshape(lay.K, -1), lay, G0, Gj, order, x_off=xo), h, hess_labels(lay), FLOOR)


# ---- sensitivity ----------------------------------------------------------------------------------------------------------------------------------
def _all(lay, G0, Gj, Z, mu, order, **kw):
    d, j, h = vc.truth_values(lay, G0, Gj, Z, mu, order, **kw)
    return d.reshape(-1), j.reshape(-1), h.reshape(-1)


@pytest.mark.parametrize("name", NAMES)
def test_every_case_sees_a_zeroed_top_coefficient(name):
    """Interval 2, every order: the residual, the Jacobian values and the Hessian values each move by 1e-7 of a segment's size or more."""
    lay, G0, Gj, Z, _ = vc.case(name)
    labels = (vc.residual_labels(lay), jac_labels(lay), hess_labels(lay))
    for order in vc.ORDERS:
        d, j, mu, h = vc.truth_ld(name, order)
        c0 = vc.coeffs(order)
        c0[-1] = 0
        bad = _all(lay, G0, Gj, Z, mu, order, c=c0)
        moved = [seen(g, b, l, "@2") for g, b, l in zip((d, j, h), bad, labels)]
        print("%s order %d, c_q = 0: residual %.1e  Jacobian %.1e  Hessian %.1e" % ((name, order) + tuple(moved)))
        assert min(moved) >= SEEN, (name, order, moved)


@pytest.mark.parametrize("name", NAMES)
def test_every_case_sees_the_shape_faults(name):
    kind, n, cols, m = vc.CASES[name]
    lay, G0, Gj, Z, _ = vc.case(name)
    jl, hl = jac_labels(lay), hess_labels(lay)
    for order in (4, 10):
        d, j, mu, h = vc.truth_ld(name, order)
        faults = {"last k step": dict(mm=mm_drop_last_k_step(n)), "last row tile": dict(mm=mm_drop_last_row_tile(n)), "last drive": dict(drop_drive=True)}
        if cols > 1:
            faults["last state column"] = dict(drop_col=True)
        for what, kw in faults.items():
            bd, bj, bh = _all(lay, G0, Gj, Z, mu, order, **kw)
            sj, sh = seen(j, bj, jl), seen(h, bh, hl)
            if what == "last state column":  # its own rows move by all they hold: ask the sums over the columns, the (u, u) entries
                sh = max(seen(h, bh, hl, "uu@%d" % k) for k in range(lay.K))
            print("%s order %d, %s: Jacobian moved by %.1e, Hessian by %.1e" % (name, order, what, sj, sh))
            assert sj >= SEEN and sh >= SEEN, (name, order, what, sj, sh)
        if name == "K7":  # the last of the 300 drive pairs: its (u, u) entry left unwritten
            per = po.hess_nnz_per_interval(lay)
            bad = np.array(h)
            for k in range(lay.K):
                assert hl[k * per + 299] == "uu@%d" % k and hl[k * per + 300] == "hu@%d" % k
                bad[k * per + 299] = 0
            assert seen(h, bad, hl) >= SEEN


# ---- structure --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["M2", "V5"])
def test_expected_structure_names_every_position_once(name):
    lay = vc.layout(name)
    r, c = po.jac_structure(lay)
    assert len(r) == lay.K * po.jac_nnz_per_interval(lay) == len(jac_labels(lay))
    tails = np.char.startswith(jac_labels(lay), "d")  # (the two blocks are replicated per state column, never summed: every position once)
    assert len(set(zip(r.tolist(), c.tolist()))) == len(r) and r.max() == lay.K * lay.x_dim - 1 and c.max() < lay.N * lay.z_dim and tails.sum() == lay.K * lay.x_dim * (lay.m + 1)
    r1, c1 = po.jac_structure(lay, index_base=1)
    assert np.array_equal(r1, r + 1) and np.array_equal(c1, c + 1)
    r, c = po.hess_structure(lay)
    assert len(r) == lay.K * po.hess_nnz_per_interval(lay) == len(hess_labels(lay)) == len(set(zip(r.tolist(), c.tolist())))
    assert np.all(r >= c) and c.min() >= 0 and r.max() < lay.N * lay.z_dim
