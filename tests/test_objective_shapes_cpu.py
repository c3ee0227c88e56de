"""CPU side of the objective-shape tests: the longdouble truth (tests/objective_truth.py) against the float64 oracle on every case of
tests/objective_cases.py, the conditions the cases must meet (every term at least 1e-3 from the kink of |1 - F|, both sides of the kink for
every loss kind), and the sensitivity of every case to the defects it is there for -- "mutant" truths (a sum that loses its elements beyond
the first 256 or one wave's partial, the wrong sign of 1 - F, ignored weights, an overlapping regulariser counted once, the last of eight
regularisers dropped, payload jobs l >= 8 dropped) must differ from the truth by at least 1e4 x the tolerance of the GPU test."""
import numpy as np
import pytest

import objective_cases as oc
import objective_truth as ot
import piccolo_jl_amd as pa
from objective_cases import CASES, LD, PAYLOAD_CASES, TOL
from oracle import pade_oracle as po

AGREE = 1e-11  # truth against the float64 oracle (sums of up to 2560 float64 products)


def rel(a, b):
    a, b = np.asarray(a, dtype=LD).reshape(-1), np.asarray(b, dtype=LD).reshape(-1)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), LD(1e-300)))


def oracle_objective(case):
    """value(s) and gradient of a case from the float64 oracle (po.sampling_objective for the unitary goals; the general form restated in float64
    numpy with po.quadratic_regularizer*)."""
    nbuf, N, zd = case["Z"].shape
    g = case["goal"]
    lay = po.Layout(d=case["d"], m=case["m"], N=N, z_dim=zd, x_off=case["x_offs"][0], u_off=case["u_off"], dt_off=case["dt_off"])
    vals, grads = [], []
    for b in range(nbuf):
        Z = case["Z"][b]
        members = [b] if case["traj"] else list(range(case["batch"]))
        w = [1.0 if case["weights"] is None else case["weights"][i] for i in members]
        xo = [case["x_offs"][0]] * len(members) if case["traj"] else case["x_offs"]
        if g[0] in ("unitary", "subspace"):
            goal = g[1] if g[0] == "unitary" else po.embed(g[1], g[2], case["d"])
            v, gr = po.sampling_objective(Z, lay, xo, goal, w, case["Q"], case["regs"], None if g[0] == "unitary" else g[2])
        else:
            v, gr = 0.0, np.zeros_like(Z)
            for off, dim, R, pw in case["regs"]:
                v += po.quadratic_regularizer(Z, off, dim, R, case["dt_off"], pw)
                gr += po.quadratic_regularizer_gradient(Z, off, dim, R, case["dt_off"], pw)
            _, A, c = g[1:]
            xs = [Z[-1, o : o + case["x_dim"]] for o in xo]
            for x, wi, idx in ([(np.concatenate(xs), 1.0, None)] if g[1] else zip(xs, w, range(len(xs)))):
                p = A @ x if A is not None else np.zeros(0)
                F = (c @ x if c is not None else 0.0) + (p * p).sum()
                s = 1.0 if 1.0 - F >= 0 else -1.0
                v += wi * case["Q"] * abs(1.0 - F)
                dF = (c if c is not None else 0.0) + (2.0 * p @ A if A is not None else 0.0)
                if g[1]:
                    for q, o in enumerate(xo):
                        gr[-1, o : o + case["x_dim"]] += -s * case["Q"] * dF[q * case["x_dim"] : (q + 1) * case["x_dim"]]
                else:
                    gr[-1, xo[idx] : xo[idx] + case["x_dim"]] += -s * wi * case["Q"] * dF
        vals.append(v), grads.append(gr)
    return np.array(vals), np.stack(grads)


@pytest.mark.parametrize("name", list(CASES))
def test_truth_agrees_with_the_oracle(name):
    case = CASES[name]
    value, grad, _, _ = oc.objective_truth(case)
    v0, g0 = oracle_objective(case)
    assert rel(value, v0) <= AGREE, rel(value, v0)
    lab = oc.grad_labels(case).reshape(-1)
    gt, gr = grad.reshape(-1), g0.reshape(-1)
    for s in np.unique(lab):
        sel = lab == s
        scale = np.abs(gt[sel]).max()
        assert float(np.abs(gt[sel] - gr[sel]).max()) <= AGREE * float(scale), (s, float(np.abs(gt[sel] - gr[sel]).max()), float(scale))


@pytest.mark.parametrize("name", [n for n in CASES if CASES[n]["goal"][0] in ("unitary", "subspace")])
def test_rows_of_the_unitary_losses_reproduce_the_direct_closed_forms(name):
    """F from the rows (a'x)^2 + (b'x)^2 [+ the row pairs of M] equals the direct |tr(G'U)|^2 / d^2 and (|M|^2 + |tr M|^2) / (ns (ns + 1)), in
    longdouble, and the oracle's po.unitary_fidelity_loss."""
    case = CASES[name]
    g = case["goal"]
    for A, c, x, w, idx, keep in oc.terms(case):
        F = ot.form_fidelity(A, c, x)[0]
        Fd = ot.unitary_fidelity(x, g[1]) if g[0] == "unitary" else ot.subspace_fidelity(x, g[1], g[2], case["d"])
        assert abs(F - Fd) <= 1e-17 * max(1, abs(Fd)), float(abs(F - Fd))
        Fo = po.unitary_fidelity_loss(x, g[1] if g[0] == "unitary" else po.embed(g[1], g[2], case["d"]), None if g[0] == "unitary" else g[2])
        assert abs(float(F) - Fo) <= 1e-13 * max(1, Fo)


def test_ket_rows_against_the_oracle_and_the_host_mirror():
    """The ket and coherent-ket rows of the truth give po.ket_fidelity_loss / po.coherent_ket_fidelity, equal the rows
    pa.KetInfidelityObjective / pa.CoherentKetInfidelityObjective hand to pcl_set_goal_form, and (L = 64) their Gram triangle is the exact
    second difference po.quadratic_hessian of the oracle's fidelity."""
    c = CASES["Cket"]
    for A, _, x, w, idx, _ in oc.terms(c):
        assert abs(float(ot.form_fidelity(A, None, x)[0]) - po.ket_fidelity_loss(x, c["ket_goal"])) <= 1e-14
    scope, Am, cm = pa.KetInfidelityObjective(c["ket_goal"], "psi").form(c["x_dim"], c["batch"])
    assert scope == 0 and cm is None and rel(Am, ot.ket_rows(c["ket_goal"])) <= 1e-16
    H = po.quadratic_hessian(lambda x: po.ket_fidelity_loss(x, c["ket_goal"]), c["x_dim"])
    assert rel(H[np.tril_indices(c["x_dim"])], ot.gram_tril(ot.ket_rows(c["ket_goal"]))) <= 1e-12
    for name in ("Ccoh5", "Ccoh5b", "Ccoh40"):
        c = CASES[name]
        goals, cw = c["coherent"]
        (A, _, x, w, idx, _), = oc.terms(c)
        Fo = po.coherent_ket_fidelity(x.reshape(c["batch"], -1), goals, cw)
        assert abs(float(ot.form_fidelity(A, None, x)[0]) - Fo) <= 1e-13
        scope, Am, cm = pa.CoherentKetInfidelityObjective(goals, ["k%d" % i for i in range(len(goals))], weights=cw).form(c["x_dim"], c["batch"])
        assert scope == 1 and cm is None and rel(Am, ot.coherent_ket_rows(goals, cw)) <= 1e-15


def loss_kind(case):
    g = case["goal"]
    return g[0] if g[0] != "form" else ("ket" if "ket_goal" in case else "coherent" if "coherent" in case else "form")


def test_every_term_is_away_from_the_kink_and_every_loss_kind_sees_both_sides():
    sides = {}
    for name, case in CASES.items():
        for s, F in oc.objective_truth(case)[3]:
            assert abs(1 - F) >= 1e-3, (name, float(F))
            sides.setdefault(loss_kind(case), set()).add(int(s))
    assert set(sides) == {"unitary", "subspace", "form", "ket", "coherent"}
    for kind, ss in sides.items():
        assert ss == {1, -1}, (kind, ss)


@pytest.mark.parametrize("name", list(CASES))
def test_every_case_sees_its_mutants(name):
    """As the GPU test compares: the value against max(1, |ref|), the gradient per segment against the segment's max|ref|.  A mutant is seen
    when the value, or some segment of the gradient, moves by 1e4 x the tolerance on that scale."""
    case = CASES[name]
    assert case["mutants"], name
    value, grad, _, _ = oc.objective_truth(case)
    lab = oc.grad_labels(case).reshape(-1)
    gt = grad.reshape(-1)
    segs = [lab == s for s in np.unique(lab)]
    segs = [(sel, np.abs(gt[sel]).max()) for sel in segs]
    for mut in case["mutants"]:
        v, g, _, _ = oc.objective_truth(case, mut)
        seen_v = float((np.abs(v - value) / np.maximum(1, np.abs(value))).max())
        gm = g.reshape(-1)
        seen_g = max(float(np.abs(gm[sel] - gt[sel]).max() / scale) for sel, scale in segs if scale > 0)
        assert max(seen_v, seen_g) >= 1e4 * TOL, "%s cannot see mutant %s: value %.2e, gradient segments %.2e" % (name, mut, seen_v, seen_g)
        if mut != "flip":  # (the wrong sign leaves the value |1 - F| as it is; every other mutant must move the value too)
            assert seen_v >= 1e4 * TOL, "%s: mutant %s does not move the value (%.2e)" % (name, mut, seen_v)
        linear = case["goal"][0] == "form" and case["goal"][2] is None  # (F = c'x: its gradient -s w Q c holds no sum to lose elements from)
        assert linear or seen_g >= 1e4 * TOL, "%s: mutant %s does not move any gradient segment (%.2e)" % (name, mut, seen_g)


def test_every_mutant_has_a_case():
    have = set(m for c in CASES.values() for m in c["mutants"])
    assert have == set(oc.MUTANTS), set(oc.MUTANTS) - have
    # the sums of more than 256 elements: every kernel's loop is covered by a case that lists the two element mutants
    for kind in ("unitary", "subspace", "form", "coherent"):
        assert any(loss_kind(c) == kind and {"drop256", "wave1"} <= set(c["mutants"]) for c in CASES.values()), kind


def test_regulariser_second_derivatives_are_the_differences_of_the_gradient():
    """The truth's regulariser Hessian (a regulariser covering dt_off included: its (dt, v_i = dt) cross term counts twice) against central
    differences of the truth's gradient in longdouble (step 1e-7: truncation zero for p <= 2 up to the cubic term, rounding 1e-19 / 1e-7)."""
    for name in ("Ddt", "Deight", "Doverlap"):
        case = CASES[name]
        Z = ot.ld(case["Z"][0][:1])
        _, _, (k, r, c, v) = ot.reg_terms(Z, case["regs"], case["dt_off"])
        zd = case["z_dim"]
        H = np.zeros((zd, zd), dtype=LD)
        np.add.at(H, (r, c), v)
        H = H + np.tril(H, -1).T
        cols = sorted(set(c.tolist()) | {case["dt_off"]})[-12:] + [case["dt_off"]]
        for j in cols:
            e = np.zeros((1, zd), dtype=LD)
            e[0, j] = LD(1e-7)
            fd = (ot.reg_terms(Z + e, case["regs"], case["dt_off"])[1] - ot.reg_terms(Z - e, case["regs"], case["dt_off"])[1])[0] / LD(2e-7)
            assert float(np.abs(fd - H[:, j]).max()) <= 1e-9 * max(1.0, float(np.abs(H[:, j]).max())), (name, j)


def test_hessian_truth_of_a_small_form_is_the_oracles_second_difference():
    c = CASES["Ccoh5"]
    goals, cw = c["coherent"]
    keys, vals, _ = oc.hessian_truth(c)
    nvar = c["Z"].size
    (A, _, x, w, idx, _), = oc.terms(c)
    H = np.zeros((nvar, nvar))
    H[keys // nvar, keys % nvar] = vals.astype(float)
    H = H + np.tril(H, -1).T
    s = 1.0 if po.coherent_ket_fidelity(x.reshape(c["batch"], -1), goals, cw) <= 1 else -1.0
    Ho = -s * c["Q"] * c["sigma"] * po.quadratic_hessian(lambda y: po.coherent_ket_fidelity(y.reshape(c["batch"], -1), goals, cw), len(idx))
    assert np.abs(H[np.ix_(idx, idx)] - Ho).max() <= 1e-11 * np.abs(Ho).max()


# ---- derivative rows and payload ----------------------------------------------------------------------------------------------------------------
def test_derivative_rows_truth_against_the_oracle():
    lay, G0, Gj, Z, x_offs, w, traj, sc = oc.payload_case("P24")
    for dx_off in (lay.u_off + lay.m, -1):
        for base in (0, 1):
            res, rows, cols, vals = ot.deriv_rows(Z[0], lay.u_off, dx_off, lay.m, lay.dt_off, index_base=base)
            r0, c0, v0 = po.derivative_jacobian(Z[0], lay.z_dim, lay.u_off, dx_off, lay.m, lay.dt_off, base)
            ref = po.derivative_residual(Z[0], lay.u_off, dx_off, lay.m, lay.dt_off) if dx_off >= 0 else (
                Z[0][1:, lay.u_off : lay.u_off + lay.m] - Z[0][:-1, lay.u_off : lay.u_off + lay.m] - Z[0][:-1, lay.dt_off : lay.dt_off + 1])
            assert rel(res, ref) <= 1e-15 and np.array_equal(rows, r0) and np.array_equal(cols, c0) and rel(vals, v0) <= 1e-16


def oracle_payload_inputs(name, order=4):
    lay, G0, Gj, Z, x_offs, w, traj, sc = oc.payload_case(name)
    J = [[po.pade_jacobian_dense(Z[s], lay, G0, Gj, order, x_off=o) for o in x_offs] for s in range(len(Z))]
    delta = [[po.pade_residual(Z[s], lay, G0, Gj, order, x_off=o).reshape(-1) for o in x_offs] for s in range(len(Z))]
    return lay, Z, w, traj, J, delta


@pytest.mark.parametrize("name", list(PAYLOAD_CASES))
def test_payload_truth_against_float64_and_its_mutant(name):
    lay, Z, w, traj, J, delta = oracle_payload_inputs(name)
    rng = np.random.default_rng(3)
    for s in range(len(Z)):
        lam = [rng.standard_normal(d.size) for d in delta[s]]
        ws = [w[s]] if traj else w
        for lm in (None, lam):
            t = ot.payload(J[s], lm, delta[s], ws, lay.N, lay.z_dim, lay.u_off, lay.m, lay.dt_off)
            g = sum(wi * (Ji.T @ (li if lm is not None else di)) for wi, Ji, li, di in zip(ws, J[s], lam, delta[s])).reshape(lay.N, lay.z_dim)
            phi = sum(wi * (1.0 if lm is not None else 0.5) * float((li if lm is not None else di) @ di) for wi, li, di in zip(ws, lam, delta[s]))
            ref = np.concatenate([[phi], g[: lay.K, lay.u_off : lay.u_off + lay.m].reshape(-1), g[: lay.K, lay.dt_off]])
            assert rel(t, ref) <= AGREE
            if lay.m + 2 > 8:  # the jobs of a wave's second pass: without them the payload is visibly another
                mut = ot.payload(J[s], lm, delta[s], ws, lay.N, lay.z_dim, lay.u_off, lay.m, lay.dt_off, max_job=8)
                assert rel(mut, t) >= 1e4 * TOL
    assert sum(1 for d, m, *_ in PAYLOAD_CASES.values() if m + 2 > 8) >= 3
