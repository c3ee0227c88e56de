"""What tests/test_large_full_gpu.py relies on, checked without a GPU: the cases of tests/large_full_cases.py walk every branch of the substep
rule; the kernel's algorithm restated in float64 (theta = 1, degree 18, s' from the column sums) agrees with the longdouble truth to 1e-13 of
max |X_k| per knot; three injected faults -- s' taken as 1 everywhere, the k-steps beyond 64 of every product dropped, the last 16-row tile of
every product zeroed -- move a knot by 1e-7 or more; the panel and slice plan of the two launches stays within the 163,840 B a workgroup can
have, for every case and every split the GPU tests ask for; and the Python keyword's ValueErrors are raised before any device call."""
import numpy as np
import pytest

import large_full_cases as fc
import large_shape_cases as lc
import piccolo_jl_amd as pa


@pytest.mark.parametrize("name", fc.NAMES)
def test_steps_walk_the_substep_rule(name):
    lay, G0, Gj, Z, sp = fc.case(name)
    h = Z[: fc.N - 1, lay.dt_off]
    assert h[0] < 0 and sp[0] == 1, (h, sp)
    assert h[1] > 0 and sp[1] >= 3, (h, sp)
    assert h[2] == 0 and sp[2] == 0, (h, sp)
    lay, G0, Gj, Z, sp = fc.case(name, 1)
    h = Z[: fc.N - 1, lay.dt_off]
    assert h[0] > 0 and sp[0] == 1 and h[1] < 0 and sp[1] == 3 and h[2] > 0 and sp[2] >= 1, (h, sp)
    print("%s: substeps %s (seed 0), %s (seed 1)" % (name, fc.case(name)[4], sp))


@pytest.mark.parametrize("name", fc.NAMES)
def test_restatement_and_faults(name):
    lay, G0, Gj, Z, _ = fc.case(name)
    ref = fc.rollout_truth_ld(name)
    e = fc.knot_errors(fc.restatement(lay, G0, Gj, Z), ref)
    print("%s: the restatement against the truth %.1e" % (name, e.max()))
    assert e[0] == 0 and e.max() <= 1e-13, e
    # (the truth's own hook: a fault there moves it as well -- the hook is live on both sides)
    assert fc.knot_errors(fc.rollout_truth_values(lay, G0, Gj, Z, mm=lc.mm_zero_last_row_tile(lay.n)), ref).max() >= fc.SEEN
    faults = {
        "one substep everywhere": dict(rule=lambda h, G: min(1, fc.substeps(h, G))),
        "k-steps beyond 64 dropped": dict(mm=lc.mm_drop_k_beyond_64(lay.n)),
        "last row tile zeroed": dict(mm=lc.mm_zero_last_row_tile(lay.n)),
    }
    for what, kw in faults.items():
        moved = fc.knot_errors(fc.restatement(lay, G0, Gj, Z, **kw), ref).max()
        print("%s: %s moves a knot by %.1e" % (name, what, moved))
        assert moved >= fc.SEEN, (name, what, moved)


def test_other_seed_and_drift():
    for kw in (dict(seed=1), dict(drift=1)):
        lay, G0, Gj, Z, _ = fc.case("L1", **kw)
        e = fc.knot_errors(fc.restatement(lay, G0, Gj, Z), fc.rollout_truth_ld("L1", **kw))
        assert e.max() <= 1e-13, (kw, e)


def test_the_rule_at_its_edges():
    G = np.array([[0.0, 2.0], [-2.0, 0.0]])
    assert fc.substeps(0.0, G) == 0 and fc.substeps(0.5, G) == 1 and fc.substeps(-0.5, G) == 1 and fc.substeps(0.5001, G) == 2
    assert fc.substeps(1e9, G) == fc.SMAX and fc.substeps(fc.SMAX / 2.0, G) == fc.SMAX


@pytest.mark.parametrize("name", fc.NAMES)
def test_plan_bytes(name):
    kind, n, cols, m = lc.CASES[name]
    splits = [dict()] + [dict(slices=s) for s in (1, 2, 5)] + [dict(cols_per_slice=c) for c in range(1, cols + 1)] + [dict(items=99), dict(items=5 * 99)]
    for kw in splits:
        P = fc.roll_plan(n, cols, m, **kw)
        assert P["bytes_e"] <= fc.LDS_BYTES and P["bytes_c"] <= fc.LDS_BYTES, (name, kw, P)
        assert sum(P["npce"]) == n and min(P["npce"]) >= 1 and sum(P["nce"]) == cols and min(P["nce"]) >= 1, (name, kw, P)
        assert P["LD"] * P["npc"] >= n  # the column sums pass through the product block
    P = fc.roll_plan(n, cols, m)
    print("%s: %d panels of %d columns (%d B), %d slices of %d columns (%d B)" % (name, P["P"], P["npc"], P["bytes_e"], P["S"], P["nc"], P["bytes_c"]))


def test_plan_at_the_largest_shape():
    """n = 128 with the ABI's most drives and every column count: one column always fits, and the widest panel is 9 columns."""
    for cols in (1, 5, 64):
        P = fc.roll_plan(128, cols, 24, items=1)
        assert P["bytes_e"] <= fc.LDS_BYTES and P["bytes_c"] <= fc.LDS_BYTES and P["npc"] <= 9 and P["nc"] <= 16, P
    assert fc.roll_plan(128, 1, 24, slices=128)["bytes_e"] == 136472 and fc.roll_plan(128, 1, 24)["bytes_c"] == 3088


def test_keyword_errors_without_a_device():
    from piccolo_jl_amd import integrators as pi

    args = dict(d=33, m=1, N=4, z_dim=70, u_off=68, dt_off=66, x_offs=[0], G0=np.zeros((66, 66)), Gj=np.zeros((1, 66, 66)), batch=1, state_cols=1)
    with pytest.raises(ValueError, match="large_generator=True"):
        pi._PclContext(batch_mode=pa._lib.PCL_BATCH_MEMBERS, pade_order=8, large_full=True, **args)
    with pytest.raises(ValueError, match="exp"):
        pi._PclContext(batch_mode=pa._lib.PCL_BATCH_MEMBERS, pade_order="exp", large_generator=True, large_full=True, **args)
    for mode in (pi.PCL_BATCH_VARIATIONAL, pi.PCL_BATCH_VARIATIONAL_EXP):
        with pytest.raises(ValueError, match="variational"):
            pi._PclContext(batch_mode=mode, pade_order=8, large_generator=True, large_full=True, **args)
    with pytest.raises(ValueError, match="large_generator=True"):
        pa.HipPadeIntegrator(np.zeros((66, 66)), np.zeros((1, 66, 66)), None, large_full=True)
    with pytest.raises(ValueError, match="exp"):
        pa.HipPadeIntegrator(np.zeros((66, 66)), np.zeros((1, 66, 66)), None, pade_order="exp", large_generator=True, large_full=True)
    with pytest.raises(ValueError, match="variational"):
        pi.HipVariationalIntegrator(None, None, "x", ["v"], "u", [None], ket=True, large_full=True)
    pi._check_services(pi.PCL_BATCH_VARIATIONAL, "exp", large_full=False, large_generator=False)  # (off: nothing to check)


def test_objective_cases_sit_on_both_sides_of_the_kink():
    import objective_cases as oc

    for name, case in fc.OBJ.items():
        sF = oc.objective_truth(case)[3]
        Fs = [float(F) for _, F in sF]
        print("%s: F = %s" % (name, ", ".join("%.3f" % F for F in Fs)))
        assert all(abs(1 - F) > 1e-3 for F in Fs), (name, Fs)
    for name in ("mat3", "den"):
        s = [float(s) for s, _ in oc.objective_truth(fc.OBJ[name])[3]]
        assert min(s) < 0 < max(s), (name, s)


def test_the_subspace_closed_form_is_the_rows_truth():
    import objective_cases as oc
    import objective_truth as ot

    case = fc.OBJ["sub4"]
    (A, c, x, w, idx, keep), = oc.terms(case)
    v, g, _, F = ot.form_loss(A, c, x, ot.LD(case["Q"]))
    v2, g2, F2 = fc.subspace_loss_ld(x, case["goal"][1], case["goal"][2], case["d"], ot.LD(case["Q"]))
    assert abs(float(F - F2)) <= 1e-17 and abs(float(v - v2)) <= 1e-15 and float(np.abs(g - g2).max()) <= 1e-15 * float(np.abs(g).max())
    assert abs(float(F2 - ot.subspace_fidelity(x, case["goal"][1], case["goal"][2], case["d"]))) <= 1e-17
