"""GPU tests of the robust-control sweep: the objective (value, gradient, Hessian, structure) and the rollout of a variational context with
option var_full at the cases of tests/robust_shape_cases.py, through piccolo_jl_amd.integrators._PclContext against the np.longdouble truths.

Tolerances (the project's own, per segment): value 1e-12 max(1, |ref|); gradient 1e-12 max|ref| per component row of the terminal knot and per
regulariser range; Hessian 1e-12 max|ref| per triangle and per knot block; rollout 1e-11 max|truth| per knot and per component (the float64
lifted oracle is within 1.8e-15 of the truth per knot and component on every case, so no case falls back to the whole-array rule).  Every test
prints the error it read."""
import numpy as np
import pytest

import piccolo_jl_amd as pa
import robust_shape_cases as rc
import robust_truth as rt
from shape_cases import check_segments

pytestmark = pytest.mark.gpu
VAR, VEXP = pa._lib.PCL_BATCH_VARIATIONAL, pa._lib.PCL_BATCH_VARIATIONAL_EXP


def context(case, exp=False):
    """A variational context of the case with var_full on: the Pade kind (robust_truth.var_context) or the exponential kind."""
    d = case.n // 2
    if exp:
        ctx = pa.integrators._PclContext(d=d, m=case.m, N=case.N, z_dim=case.z_dim, u_off=case.u_off, dt_off=case.dt_off, x_offs=case.xo,
                                         G0=np.concatenate([case.G0[None], np.array(case.Gv)]), Gj=np.asarray(case.Gj).reshape(case.m, case.n, case.n),
                                         batch=1 + case.v, batch_mode=VEXP, per_member_G0=True, pade_order="exp", state_cols=1 if case.C == 1 else d)  # fmt: skip
    else:
        ctx = rt.var_context(pa, case)
    ctx.set_option("var_full", 1)
    return ctx


def objective_context(q, exp=False):
    ctx = context(q.vc, exp)
    if q.goal[0] == "unitary":
        ctx.set_goal(rc._iso_vec(q.goal[1]))
    elif q.goal[0] == "subspace":
        ctx.set_goal_subspace(rc._iso_vec(q.goal[1]), q.goal[2])
    else:
        ctx.set_goal_form(0, q.goal[1], q.goal[2])
    ctx.set_weights(q.w)
    for r in q.regs:
        ctx.add_regularizer(*r)
    return ctx


def check_objective(ctx, q, regs, w, what, shifts=(0,)):
    """Value, gradient, structure and Hessian of the context against the truth of (regs, w); the Hessian through the host path and through a
    device array `shift` doubles off a 16-byte boundary, all to the same bits.  Returns (value, gradient, Hessian values)."""
    import torch

    name, vc = q.name, q.vc
    Z = vc.Z.reshape(-1)
    v_ref, g_ref, _ = rc.objective_truth(name, regs=regs, w=w)
    val, grad = ctx.objective(Z, q.Q)
    assert ctx.get_option("last_objective_launches") == 1
    e_v = rc.check_value(val[0], v_ref)
    e_g = max(check_segments(grad, g_ref, rc.grad_labels(name, regs, w), rc.TOL).values())
    h_ref, segs, struct = rc.hessian_truth(name, regs=regs, w=w, structure=True)
    rows, cols = ctx.objective_hess_structure()
    assert len(rows) == len(cols) == len(h_ref) and np.all(rows >= cols)
    if struct is None:
        assert len(rows) == 0
    else:  # position by position, in the library's order
        assert np.array_equal(rows, struct[0]) and np.array_equal(cols, struct[1])
    hv = ctx.objective_hess(Z, q.Q, q.sigma)
    assert np.all(np.isfinite(hv))
    errs = rc.segment_errors(hv, h_ref, segs)
    for lab, a, b in segs:
        scale = float(np.abs(h_ref[a:b]).max())
        assert errs[lab] <= (rc.TOL if scale > 0 else 0.0), "%s %s: segment %s rel %.3e (max|ref| %.3e)" % (name, what, lab, errs[lab], scale)
    e_h = max(errs.values()) if errs else 0.0
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    Zd = torch.from_numpy(np.array(Z)).cuda()
    for shift in shifts:
        hd = torch.full((hv.size + 2,), float("nan"), dtype=torch.float64, device="cuda")
        assert (hd.data_ptr() + 8 * shift) % 16 == 8 * shift
        ctx.objective_hess_dev(Zd, q.Q, q.sigma, hd[shift : shift + hv.size])
        torch.cuda.synchronize()
        out = hd.cpu().numpy()
        assert np.array_equal(out[shift : shift + hv.size], hv), (name, what, shift)
        assert np.isnan(out[:shift]).all() and np.isnan(out[shift + hv.size :]).all()  # nothing outside the values
    print("ROBUST objective %s %s: value %.2e gradient %.2e Hessian %.2e (%d values, F = %.6f)" % (name, what, e_v, e_g, e_h, hv.size,
                                                                                                  float(rc.objective_truth(name)[2])))  # fmt: skip
    return val, grad, hv


@pytest.mark.parametrize("name", rc.OBJ_NAMES)
def test_objective_value_gradient_hessian(name):
    """Q1 .. Q12: d = 32 on a variational context (Q7), the values array 8 bytes off a 16-byte boundary at even d (Q1, Q3, Q7: head and tail
    peeled together), F > 1 (Q2, Q7), the partial (Q3, Q6), straddling (Q8), three-power (Q7) and Gram-absorbed (Q6, Q8, Q9) covers, a cover
    that stays whole (Q3), the 300-row (Q9) and the linear-only (Q10) forms, N = 2 just before the kink (Q11), the exponential kind (Q12)."""
    q = rc.obj_case(name)
    ctx = objective_context(q, q.exp)
    shifts = (0, 1) if name in rc.OFFSET_CASES else (0,)
    val, grad, hv = check_objective(ctx, q, q.regs, q.w, "as set", shifts)
    if q.exp:  # the bits of the Pade context
        pade = objective_context(q)
        v2, g2 = pade.objective(q.vc.Z.reshape(-1), q.Q)
        assert v2[0] == val[0] and np.array_equal(g2, grad) and np.array_equal(pade.objective_hess(q.vc.Z.reshape(-1), q.Q, q.sigma), hv)
        pade.close()
    ctx.close()


@pytest.mark.parametrize("name", rc.REOPEN_CASES)
def test_a_change_of_R_and_of_a_weight_on_an_open_context(name):
    """The regularisers replaced by ones of the same offsets and sizes and another R (the plan's last_src stays, its diag changes), then a weight
    set to zero (a triangle leaves, its cover returns to the knot's block) and back: the values follow the truth each time."""
    q = rc.obj_case(name)
    ctx = objective_context(q)
    hv0 = ctx.objective_hess(q.vc.Z.reshape(-1), q.Q, q.sigma)  # the plan of (regs, w) is on the device
    ctx.clear_regularizers()
    for r in q.regs2:
        ctx.add_regularizer(*r)
    _, _, hv1 = check_objective(ctx, q, q.regs2, q.w, "R replaced")
    assert hv1.size == hv0.size and not np.array_equal(hv1, hv0)
    w = np.array(q.w)
    w[q.toggle] = 0.0
    ctx.set_weights(w)
    _, _, hv2 = check_objective(ctx, q, q.regs2, w, "w[%d] = 0" % q.toggle)
    assert hv2.size < hv1.size
    ctx.set_weights(q.w)
    _, _, hv3 = check_objective(ctx, q, q.regs2, q.w, "w back")
    assert np.array_equal(hv3, hv1)
    ctx.close()


@pytest.mark.parametrize("name", rc.ROLL_NAMES)
def test_rollout(name):
    """P1 .. P9: d = 29 / 30 / 31 (Gv_i in LDS and from L2), the 16 + 1 column split (P3), one group (P4), a ket (P5), 24 drives (P6), the
    sq = 0 / 1 pair beside sq = 8 (P7), the zero and the negative step (P8), the exponential kind at n = 62 (P9)."""
    import torch

    case = rc.roll_case(name)
    exp = rc.ROLL[name][6]
    ctx = context(case, exp)
    Z = case.Z.reshape(-1)
    X = ctx.rollout(Z).copy()
    assert X.shape == (1, case.N, case.xd)
    X = X[0]
    T = rc.roll_truth_ld(name)
    errs = rc.roll_errors(X, T, case)
    whole = float(np.abs(X - T).max() / np.abs(T).max())
    print("ROBUST rollout %s: per knot and component %.2e, whole array %.2e" % (name, errs.max(), whole))
    assert np.all(np.isfinite(X))
    assert np.array_equal(X[0], np.concatenate([case.Z[0, o : o + case.xdc] for o in case.xo]))  # knot 0 is the input's bits
    if rc.ROLL_RULE[name] == "component":
        assert errs.max() <= rc.ROLL_TOL, errs
    else:
        assert whole <= rc.ROLL_TOL
    if name == "P8":  # the zero step
        assert np.array_equal(X[2], X[1])
    # component 0 has the bits of a plain context's rollout
    plain = rt.plain_context(pa, case)
    Xp = plain.rollout(Z)[0]
    plain.close()
    assert np.array_equal(X[:, : case.xdc], Xp)
    # a repeated call and the device-pointer path: the same bits
    X2 = ctx.rollout(Z)[0]
    Zd = torch.from_numpy(np.array(Z)).cuda()
    out = torch.full((case.N * case.xd,), float("nan"), dtype=torch.float64, device="cuda")
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.rollout_dev(Zd, out)
    torch.cuda.synchronize()
    assert np.array_equal(X2, X) and np.array_equal(out.cpu().numpy().reshape(X.shape), X)
    if exp:  # the bits of the Pade context
        pade = context(case)
        assert np.array_equal(pade.rollout(Z)[0], X)
        pade.close()
    ctx.close()
