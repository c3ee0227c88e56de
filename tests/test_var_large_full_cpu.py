"""The cases of tests/var_large_full_cases.py without a GPU: the float64 restatement of the large variational rollout's algorithm against the
longdouble truth (1e-13 per knot and component), the four mutants of the restatement (each seen at >= 1e-7 = 1e4 x the GPU tolerance on at least
one case), the launch plan's bytes over every even n and every split the GPU tests ask for, and the keyword's ValueErrors.

Read: restatement against the truth 9.0e-16 at worst (VL4, seed 1); the mutants' largest distance over the cases 1.0 for the chain without
L_i X, the Horner level without Gv_i V and Yv reset per substep (a sensitivity component moves by its whole size), 8.2e-6 for s' taken as 1:
the smallest value read."""
import numpy as np
import pytest

import var_large_full_cases as fc
import piccolo_jl_amd as pa

CPU_CASES = ("VL1", "VL4", "VL6")  # the kets: a unitary's columns go through the same operations, one by one (the GPU tests hold VL2 and VL3)


@pytest.mark.parametrize("name", CPU_CASES)
@pytest.mark.parametrize("seed", fc.SEEDS)
def test_restatement_meets_the_truth(name, seed):
    cs, sp = fc.case(name, seed)
    e = fc.knot_errors(fc.restatement(cs), fc.rollout_truth_ld(name, seed), cs)
    print("%s seed %d substeps %s: restatement against the truth %.1e" % (name, seed, sp, e.max()))
    assert e.max() <= 1e-13, (name, seed, e)
    if seed == 0:
        assert sp[2] == 0 and sp[0] == 1 and 20 <= sp[1] <= 51, sp
        t = fc.rollout_truth(name, seed).reshape(cs.N, -1)
        assert np.array_equal(t[2], t[3])  # h = 0
    else:
        assert sp[0] == 1 and sp[1] == 3, sp


def test_unitary_cases_take_the_branches_of_their_rows():
    """VL2 and VL3 (the truths of 33 and 48 columns are the GPU tests'): the substeps, without a longdouble product."""
    for name in ("VL2", "VL3"):
        for seed in fc.SEEDS:
            cs, sp = fc.case(name, seed)
            assert (sp[0], sp[2]) == (1, 0) and 20 <= sp[1] <= 51 if seed == 0 else sp[:2] == (1, 3), (name, seed, sp)
            assert bool(np.any(cs.Z[0, cs.xo[1] : cs.xo[1] + cs.xdc])) == (seed == 1)
    assert fc.case("VL2", 0)[1][3] == 3 and fc.case("VL2", 1)[1][3] == 0


def test_mutants_of_the_restatement_are_seen():
    best = {m: 0.0 for m in fc.MUTANTS}
    for name in CPU_CASES:
        for seed in fc.SEEDS:
            cs, _ = fc.case(name, seed)
            ref = fc.rollout_truth(name, seed)
            for m in fc.MUTANTS:
                best[m] = max(best[m], fc.knot_errors(fc.restatement(cs, mutant=m), ref, cs).max())
    print("mutants, the largest distance over the cases: " + ", ".join("%s %.1e" % kv for kv in best.items()) + "; smallest %.1e" % min(best.values()))
    for m, e in best.items():
        assert e >= fc.SEEN, (m, e)


def test_plan_bytes_and_table():
    for n in range(66, 130, 2):
        for v in (1, 2):
            for cols in (1, n // 2):
                for m in (0, 3, 24):
                    for K in (1, 3, 4, 99):
                        splits = [dict()] + [dict(cols_per_slice=c) for c in range(1, 17)] + [dict(slices=s) for s in (1, 2, 5, n)]
                        for kw in splits:
                            P = fc.roll_plan(n, cols, m, v, K=K, **kw)
                            assert P["bytes_e"] <= fc.LDS_BYTES and P["bytes_c"] <= fc.LDS_BYTES, (n, v, cols, m, K, kw, P)
                            assert 1 <= P["nc"] <= 16 and sum(P["nce"]) == cols and sum(P["npce"]) == n and min(P["npce"]) >= 1 and min(P["nce"]) >= 1
                            if "slices" in kw:
                                assert P["P"] >= min(kw["slices"], n)
                            if not kw and K * (1 + v) * 8 <= 256:
                                assert P["grid_e"] <= 256 or P["npc"] == (fc.LDS_BYTES // 8 - (n | 1) * n - fc.SLACK - m - 8) // (n | 1) // 6
    # the cases: VL2 three chain slices of 16 + 16 + 1 columns; VL4 the smallest panel, six of the 29 blocks beside the tile per column
    assert fc.roll_plan(66, 33, 3, 2, K=4)["nce"] == [16, 16, 1]
    p4 = fc.roll_plan(128, 1, 1, 2, K=3)
    assert (fc.LDS_BYTES // 8 - 129 * 128 - fc.SLACK - 1 - 8) // 129 == 29 and p4["npc"] <= 4 and p4["bytes_e"] <= fc.LDS_BYTES
    assert fc.roll_plan(128, 64, 24, 2, K=99, slices=1)["npc"] == 4
    assert fc.roll_plan(128, 64, 24, 2, slices=128)["bytes_e"] == 139568 and fc.roll_plan(128, 1, 24, 2)["bytes_c"] == 5152


def test_keyword_errors_fire_without_a_device():
    VAR, VEXP = pa._lib.PCL_BATCH_VARIATIONAL, pa._lib.PCL_BATCH_VARIATIONAL_EXP
    chk = pa.integrators._check_services
    chk(VAR, 8, large_generator=True, large_variational=True, large_var_full=True)
    with pytest.raises(ValueError, match="large_var_full=True .* needs that keyword"):
        chk(VAR, 8, large_var_full=True)
    with pytest.raises(ValueError, match="exp"):
        chk(VEXP, "exp", large_generator=True, large_variational=True, large_var_full=True)
    with pytest.raises(ValueError, match="large_var_full=True .*pade_order"):
        chk(VAR, "exp", large_generator=True, large_var_full=True)
    with pytest.raises(ValueError, match="large_var_full=True .* plain context takes large_full"):
        chk(pa._lib.PCL_BATCH_MEMBERS, 8, large_generator=True, large_var_full=True)
    row = pa.integrators._BY_OPTION["large_var_full"]
    assert row.keyword == "large_var_full" and row.beside == "large_generator" and row.family == "variational" and row.at == "large_variational"
    assert "large_var_full" in pa.integrators._OPTION_ORDER
    import inspect

    assert "large_var_full" in inspect.signature(pa.integrators.HipVariationalIntegrator.__init__).parameters
    assert "large_var_full" not in inspect.signature(pa.integrators.HipPadeIntegrator.__init__).parameters
