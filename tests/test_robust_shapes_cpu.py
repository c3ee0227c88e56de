"""CPU side of the robust-control sweep (tests/robust_shape_cases.py): every case sits on the branch point the table names (the launch code's
formulas of pcl_host_robust.hpp restated there), the longdouble truths agree with the float64 oracles (tests/robust_truth.py: the closed forms
in numpy, scipy's expm of the lifted matrix), every mutant is seen by the case CATCHES names at >= 1e4 x the GPU tolerance, and every case and
mutant is one the GPU tests run."""
import numpy as np
import pytest
import scipy.sparse as sp

import robust_shape_cases as rc
import robust_truth as rt
from oracle import pade_oracle as po
from robust_shape_cases import LD, OBJ, ROLL

AGREE = 1e-11  # longdouble truth against the float64 closed forms


# ---- the objective cases sit where the table says -----------------------------------------------------------------------------------------------
def test_objective_cases_sit_on_their_branch_points():
    L = {name: rc.obj_case(name).vc.xdc for name in OBJ}
    assert L == {"Q1": 32, "Q2": 242, "Q3": 288, "Q4": 1058, "Q5": 1352, "Q6": 1458, "Q7": 2048, "Q8": 72, "Q9": 64, "Q10": 10, "Q11": 32, "Q12": 288}
    nT = {name: rc.tri_len(L[name]) for name in OBJ}
    assert (nT["Q1"], nT["Q2"], nT["Q3"]) == (528, 29403, 41616)
    assert [nT[q] % 2 for q in ("Q1", "Q2", "Q3", "Q6", "Q7")] == [0, 1, 0, 1, 0]  # even d: even nT (aligned, or head and tail together)
    assert L["Q2"] < 256 < L["Q3"]
    assert rc.hess_grids(L["Q1"]) == (2, 3, 3)  # one pass
    assert rc.hess_grids(L["Q4"])[0] == 1095 < rc.SENS_CAP
    assert rc.hess_grids(L["Q5"])[1] == 3573 < rc.GRAM_CAP
    assert rc.hess_grids(L["Q6"]) == (2078, 4155, 4155) and rc.SENS_CAP < 2078 < 2 * rc.SENS_CAP and rc.GRAM_CAP < 4155 < rc.SCALE_CAP
    assert rc.hess_grids(L["Q7"]) == (4098, 8196, 8196) and 4098 == 2 * rc.SENS_CAP + 2 and 8196 > rc.SCALE_CAP
    for name in rc.OFFSET_CASES:  # even nT: an array 8 bytes off peels the head AND the tail of every triangle
        assert nT[name] % 2 == 0 and (nT[name] - 1) % 2 == 1
    for name in OBJ:  # odd z_dim and a leading pad: the component rows of the odd knots are not 16-byte aligned
        vc = rc.obj_case(name).vc
        assert vc.z_dim % 2 == 1 and min(vc.xo) == 1
    assert rc.obj_case("Q6").vc.xo != sorted(rc.obj_case("Q6").vc.xo) and rc.roll_case("P3").xo != sorted(rc.roll_case("P3").xo)
    assert rc.obj_case("Q11").vc.N == 2 and rc.obj_case("Q12").exp


def test_the_kink_both_sides_and_near():
    F = {name: float(rc.objective_truth(name)[2]) for name in OBJ}
    for name in OBJ:
        assert (F[name] > 1 + 1e-3) == (name in rc.F_ABOVE), (name, F[name])
    assert all(F[name] < 1 for name in OBJ if name not in rc.F_ABOVE)
    assert 0 < 1 - F["Q11"] < 1e-3 and abs((1 - F["Q11"]) - 5e-4) < 1e-9
    print("F per case:", {k: round(v, 6) for k, v in F.items()})


def test_regulariser_sets_cover_what_the_table_says():
    q6, q7, q8, q3, q9, q10 = (rc.obj_case(n) for n in ("Q6", "Q7", "Q8", "Q3", "Q9", "Q10"))
    vc, L = q6.vc, q6.vc.xdc
    assert len(q6.regs) == 8 and sorted(p for o, _, _, p in q6.regs if o == vc.u_off) == [0, 1, 2]
    assert any(o <= vc.dt_off < o + dim and p >= 1 for o, dim, _, p in q6.regs)  # the x 2 rule
    part = [r for r in q6.regs if vc.xo[1] < r[0] < vc.xo[1] + L][0]
    assert part[0] + part[1] == vc.xo[1] + L + 2 and part[0] + part[1] <= vc.dt_off  # past the component's end, into the gap
    assert sorted(p for o, dim, _, p in q6.regs if o == vc.xo[0] and dim == L) == [0, 2]
    assert any(o == vc.xo[1] and dim == L for o, dim, _, _ in q6.regs)
    cover = [r for r in q7.regs if r[0] == q7.vc.xo[2] + 100]
    assert sorted(r[3] for r in cover) == [0, 1, 2] and len({r[1] for r in cover}) == 1
    h = q7.vc.Z[-1, q7.vc.dt_off]
    assert 0.04 < h < 0.2  # h and h^2 apart
    st = q8.regs[2]
    assert q8.vc.xo[1] < st[0] < q8.vc.xo[1] + 72 < st[0] + st[1] <= q8.vc.xo[2] + 72 and rc.triangles("Q8") == [0, 1, 2]
    assert q8.regs[1][0] == q8.vc.xo[0]
    assert rc.triangles("Q3") == [0, 2] and q3.regs[1][0] == q3.vc.xo[1] and q3.w[1] == 0  # the cover of the weightless variation stays whole
    assert rc.triangles("Q9") == [0] and len(q9.goal[1]) == 300 and q9.goal[2] is not None
    assert rc.triangles("Q10") == [] and q10.goal[1] is None and q10.goal[2] is not None
    for q in (q3, q6):
        assert [(o, dim, p) for o, dim, _, p in q.regs] == [(o, dim, p) for o, dim, _, p in q.regs2]
        assert all(np.abs(np.asarray(a[2]) - np.asarray(b[2])).min() > 0 for a, b in zip(q.regs, q.regs2))
    # the three rows of the absorbed diagonals are all non-zero on Q7 (h and h^2 both in use), and the ket's variation cover is kept
    assert hessian_kept("Q9") == hessian_kept("Q9", absorbed=False) - 64


def hessian_kept(name, absorbed=True):
    q = rc.obj_case(name)
    segs = rc.hessian_truth(name)[1]
    full = [b - a for lab, a, b in segs if lab == "knot@0"][0]
    return [b - a for lab, a, b in segs if lab == "knot@%d" % (q.vc.N - 1)][0] if absorbed else full


# ---- the truth against the float64 closed forms -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["Q1", "Q2", "Q3", "Q8", "Q11", "Q12"])
def test_objective_truth_agrees_with_the_float64_closed_forms(name):
    q = rc.obj_case(name)
    vc = q.vc
    goal, sub = (q.goal[1], None) if q.goal[0] == "unitary" else (po.embed(q.goal[1], q.goal[2], vc.n // 2), q.goal[2])
    v0, g0, H0 = rt.objective(vc, vc.Z, q.w, q.Q, goal, sub, q.regs, want_hess=True)
    value, grad, _ = rc.objective_truth(name)
    assert abs(float(value) - v0) <= AGREE * max(1.0, abs(v0))
    assert np.abs(grad.astype(float) - g0).max() <= AGREE * np.abs(g0).max()
    vals, segs, (rows, cols) = rc.hessian_truth(name, structure=True)
    nv = vc.Z.size
    assert np.all(rows >= cols) and len(rows) == len(vals) == segs[-1][2]
    keys, n_tri = rows * nv + cols, sum(b - a for lab, a, b in segs if lab.startswith("tri"))
    # each position once: no triangle position twice, none again in a knot's block (regularisers that overlap EACH OTHER emit their shared
    # positions once each, as on a plain context)
    assert len(np.unique(keys[:n_tri])) == n_tri and not np.isin(keys[n_tri:], keys[:n_tri]).any()
    D = (sp.coo_matrix((vals.astype(float), (rows, cols)), shape=(nv, nv)).tocsr() - q.sigma * sp.tril(H0)).tocoo()
    err = np.abs(D.data).max() if D.nnz else 0.0
    print("%s: float64 closed forms against the truth: value %.2e gradient %.2e Hessian %.2e (relative)" % (
        name, abs(float(value) - v0) / max(1.0, abs(v0)), np.abs(grad.astype(float) - g0).max() / np.abs(g0).max(), err / (q.sigma * np.abs(H0.data).max())))  # fmt: skip
    assert err <= AGREE * q.sigma * np.abs(H0.data).max()


def test_ket_truths_against_float64():
    for name in ("Q9", "Q10"):
        q = rc.obj_case(name)
        vc = q.vc
        A, c = q.goal[1], q.goal[2]
        x = vc.Z[-1, vc.xo[0] : vc.xo[0] + vc.xdc]
        p = A @ x if A is not None else np.zeros(0)
        F = c @ x + (p * p).sum()
        assert abs(F - 0.6) < 1e-12
        v0 = q.w[0] * q.Q * abs(1 - F) + sum(po.quadratic_regularizer(vc.Z, o, dim, R, vc.dt_off, pw) for o, dim, R, pw in q.regs)
        assert abs(float(rc.objective_truth(name)[0]) - v0) <= AGREE * max(1.0, abs(v0))


# ---- mutants ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mut", rc.MUTANTS)
def test_every_mutant_is_seen(mut):
    name, head = rc.CATCHES[mut]
    dist = rc.mutant_distance(name, mut, head)
    print("mutant %-15s seen by %s at %.2e (needs %.1e)" % (mut, name, dist, rc.SEEN * rc.TOL))
    assert dist >= rc.SEEN * rc.TOL


def test_the_peeling_mutants_need_the_offset_array():
    for mut in ("nohead", "notail"):
        assert rc.mutant_distance("Q1", mut, 0) == 0.0  # aligned and even: nothing is peeled


# ---- rollout cases ---------------------------------------------------------------------------------------------------------------------------
def test_rollout_cases_sit_on_their_branch_points():
    n = {name: rc.roll_case(name).n for name in ROLL}
    assert rc.roll_lds(n["P1"], 30, 5)[0] == 149568 <= rc.LDS_BYTES and rc.gv_in_lds(n["P1"])
    assert rc.roll_lds(n["P2"], 29, 5)[0] == 144608 and rc.gv_in_lds(n["P2"])
    assert rc.roll_lds(n["P9"], 31, 5)[0] == 164448 > rc.LDS_BYTES and not rc.gv_in_lds(n["P9"]) and rc.roll_lds(n["P9"], 31, 4)[0] <= rc.LDS_BYTES
    for name in ROLL:
        case = rc.roll_case(name)
        a, b, cc = rc.roll_lds(case.n, case.C, 5 if rc.gv_in_lds(case.n) else 4)
        assert a <= rc.LDS_BYTES and b <= rc.LDS_BYTES, name
    groups = lambda name: [min(16, rc.roll_case(name).C - c0) for c0 in range(0, rc.roll_case(name).C, 16)]
    assert groups("P3") == [16, 1] and groups("P4") == [16] and groups("P5") == [1] and groups("P1") == [16, 14]
    assert rc.roll_case("P6").m == 24 and rc.roll_case("P5").n == 10 and n["P9"] == 62 and ROLL["P9"][6]
    p7 = rc.roll_case("P7")
    assert [rc.squarings(p7.Z[k, p7.dt_off], rc.g_of(p7, k)) for k in range(3)] == [0, 1, 8]
    for k in range(3):  # the rule reads row or column sums alike: G(H) of a Hermitian H is antisymmetric up to its symmetric Im H blocks
        G = rc.g_of(p7, k)
        assert rc.squarings(p7.Z[k, p7.dt_off], G) == rc.squarings(p7.Z[k, p7.dt_off], G.T)
    p8 = rc.roll_case("P8")
    assert p8.Z[1, p8.dt_off] == 0.0 and p8.Z[2, p8.dt_off] < 0 < p8.Z[0, p8.dt_off]


@pytest.mark.parametrize("name", rc.ROLL_NAMES)
def test_rollout_truth_against_the_float64_lifted_oracle(name):
    """The distance printed here is the float64 oracle's floor.  A case keeps the per-component bound only where that floor is within a tenth
    of it on every knot and component."""
    case = rc.roll_case(name)
    T = rc.roll_truth_ld(name)
    O = rt.lifted_rollout(case)
    comp = rc.roll_errors(O, T, case)
    whole = float(np.abs(O - T).max() / np.abs(T).max())
    print("rollout %s: float64 lifted oracle against the truth: per component %.2e, whole array %.2e" % (name, comp.max(), whole))
    assert np.array_equal(T[0].astype(float), np.concatenate([case.Z[0, o : o + case.xdc] for o in case.xo]))
    assert np.abs(T).reshape(case.N, case.v + 1, -1).max(axis=2).min() > 0.1  # every component of every knot is O(1)
    assert whole <= rc.ROLL_TOL / 10
    assert (rc.ROLL_RULE[name] == "component") == (comp.max() <= rc.ROLL_TOL / 10), (name, comp.max())
    if name == "P8":
        assert np.array_equal(T[2], T[1])


# ---- coverage ----------------------------------------------------------------------------------------------------------------------------------
def test_every_case_and_mutant_is_run_on_the_gpu():
    import ast
    import os

    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_robust_shapes_gpu.py")).read()
    ast.parse(src)
    assert 'parametrize("name", rc.OBJ_NAMES)' in src and 'parametrize("name", rc.ROLL_NAMES)' in src
    assert set(rc.MUTANTS) == set(rc.CATCHES) and {c for c, _ in rc.CATCHES.values()} <= set(rc.OBJ_NAMES)
    assert {c for c, head in rc.CATCHES.values() if head} <= set(rc.OFFSET_CASES)  # the peeling mutants: a case that is run on an offset array
    assert set(rc.OFFSET_CASES) <= set(rc.OBJ_NAMES) and set(rc.REOPEN_CASES) <= set(rc.OBJ_NAMES)
    assert sorted(OBJ[q][0] for q in OBJ if not OBJ[q][1]) == [4, 4, 6, 11, 12, 12, 23, 26, 27, 32]
    assert sorted(ROLL[p][0] for p in ROLL) == [5, 9, 12, 12, 16, 17, 29, 30, 31]
