"""The robust-control objective and the rollout of the stacked state at generator dimensions 66 .. 128 on the device (option large_var_full on a
context created with PCL_BATCH_VARIATIONAL | PCL_LARGE_N | PCL_LARGE_VAR; piccolo.jl_amd/csrc/pcl_kernel_var_large_rollout.hpp, and the
objective kernels of n <= 64 behind the option's gate), at the cases of tests/var_large_full_cases.py, through the C ABI.

Rollout: every knot and component within 1e-11 of that knot's and component's largest entry in the longdouble truth (the project's rule for
the rollouts; tests/test_var_large_full_cpu.py holds the float64 restatement to 1e-13), written into NaN-filled arrays; knot 0 a bitwise copy,
the knot across a zero step equal as numbers; component 0 with the bits of a plain PCL_LARGE_N context's rollout, component 1 of a v = 2
context with the bits of the v = 1 context of Gv_1 alone; two launches, device and host pointers, every split and an output 8 bytes off a
16-byte boundary bit for bit; the rollout's states put back into Z leave an order-10 Pade residual of the same context below 1e-11 at steps
|h| |Ghat|_2 <= 0.3.
Objective: the 1e-12 rule of tests/test_objective_shapes_gpu.py (value 1e-12 max(1, |ref|); gradient and Hessian 1e-12 max |ref| per
segment); the Hessian as a COO matrix with duplicates summed; H p against central differences of the device's gradient at 1e-6.
The d = 64 unitary Hessian (268 MB per triangle) is not run.

Largest errors read on an MI355X: rollout 1.3e-15 of the knot's and component's largest entry (VL3, seed 1, knot 3, component 1; VL1 4.7e-16,
VL2 7.6e-16, VL4 9.0e-16, VL6 7.4e-16); order-10 residual of the rollout's states 3.7e-16; objective value 3.4e-16, gradient 2.6e-16, Hessian
2.7e-16 (VL2, 7,138,475 values), H p against the gradient's central difference 9.6e-9 at max |H p| = 23 (1e-6 max(1, |H p|) allowed); through the
public constructor value 2.4e-16, gradient 1.9e-16, rollout 9.2e-16.
Without the feature every test here fails: `large_var_full` is an unknown keyword and an unknown option."""
import ctypes

import numpy as np
import pytest
import torch

import piccolo_jl_amd as pa
import var_large_cases as vl
import var_large_full_cases as fc
import variational_truth as vt
from shape_cases import check_segments

pytestmark = pytest.mark.gpu
L = pa._lib
EINVAL, ENOTIMPL, ESHAPE = L.PCL_EINVAL, L.PCL_ENOTIMPL, L.PCL_ESHAPE
VAR, MEMBERS = L.PCL_BATCH_VARIATIONAL, L.PCL_BATCH_MEMBERS
NAN = float("nan")
KIND_WORDS = "%s is not implemented for a large variational context (PCL_BATCH_VARIATIONAL | PCL_LARGE_N | PCL_LARGE_VAR, generator dimension %d > 64): residual and Jacobian only"


def make_ctx(cs, order=8, full=True, **kw):
    c = pa.integrators._PclContext(**vl.context_args(cs, order, batch_mode=VAR, large_generator=True, large_variational=True, large_var_full=full, **kw))
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    return c


def plain_ctx(cs, order=8):
    """A plain PCL_LARGE_N context with large_full of the same drift and drives on component 0 of the same knots."""
    c = pa.integrators._PclContext(d=cs.n // 2, m=cs.m, N=cs.N, z_dim=cs.z_dim, u_off=cs.u_off, dt_off=cs.dt_off, x_offs=[cs.xo[0]], G0=cs.G0, Gj=cs.Gj,
                                   batch=1, batch_mode=MEMBERS, pade_order=order, state_cols=cs.C, large_generator=True, large_full=True)  # fmt: skip
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    return c


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float64).reshape(-1)).cuda()


def nans(k):
    return torch.full((k,), NAN, dtype=torch.float64, device="cuda")


def rollout_dev(c, Zd):
    out = nans(c.N * c.x_dim)
    c.rollout_dev(Zd, out)
    c.sync()
    got = out.cpu().numpy()
    assert not np.isnan(got).any()
    return got


def refused(call, code, *words):
    with pytest.raises(pa.PclError) as ei:
        call()
    assert ei.value.code == code, str(ei.value)
    for w in words:
        assert w in str(ei.value), str(ei.value)
    return str(ei.value)


def check_knots(cs, got, ref, what):
    e = fc.knot_errors(got, ref, cs)
    k, b = np.unravel_index(int(e.argmax()), e.shape)
    print("%s: rollout %.1e of the knot's and component's largest entry (knot %d, component %d)" % (what, e.max(), k, b))
    assert e.max() <= fc.TOL, (what, e)
    g = np.asarray(got).reshape(cs.N, cs.v + 1, cs.xdc)
    for b, o in enumerate(cs.xo):
        assert np.array_equal(g[0, b], cs.Z[0, o : o + cs.xdc]), "knot 0 is a copy"
    return e.max()


# ---- 1. rollout against the truth ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.NAMES)
@pytest.mark.parametrize("seed", fc.SEEDS)
def test_rollout_values(name, seed):
    cs, sp = fc.case(name, seed)
    c = make_ctx(cs)
    assert c.large_variational and c.large_var_full and c.get_option("large_var_full") == 1
    got = rollout_dev(c, dev(cs.Z))
    assert c.get_option("last_kernel") == 360
    check_knots(cs, got, fc.rollout_truth(name, seed), "%s seed %d substeps %s" % (name, seed, sp))
    g = got.reshape(cs.N, -1)
    for k in range(cs.K):
        if cs.Z[k, cs.dt_off] == 0.0:  # E = I and L_i = 0 exactly
            assert np.array_equal(g[k + 1], g[k]), (name, seed, k)
    c.close()


# ---- 2. bits ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["VL2", "VL3"])
def test_component_0_has_the_bits_of_a_plain_large_contexts_rollout(name):
    cs, _ = fc.case(name, 1)
    c, p = make_ctx(cs), plain_ctx(cs)
    Zd = dev(cs.Z)
    got = rollout_dev(c, Zd).reshape(cs.N, cs.v + 1, cs.xdc)
    ref = rollout_dev(p, Zd).reshape(cs.N, cs.xdc)
    assert p.get_option("last_kernel") == 270 and np.array_equal(got[:, 0], ref), name
    c.close()
    p.close()


def test_component_1_has_the_bits_of_the_context_of_its_variation_alone():
    cs, _ = fc.case("VL2", 1)
    one = vt.VarCase(**{**cs.__dict__, "xo": cs.xo[:2], "Gv": cs.Gv[:1]})
    c, c1 = make_ctx(cs), make_ctx(one)
    Zd = dev(cs.Z)
    got = rollout_dev(c, Zd).reshape(cs.N, 3, cs.xdc)
    got1 = rollout_dev(c1, Zd).reshape(cs.N, 2, cs.xdc)
    assert np.array_equal(got[:, :2], got1)
    c.close()
    c1.close()


@pytest.mark.parametrize("name", ["VL2", "VL4"])
def test_every_split_two_launches_and_both_pointer_paths_bitwise(name):
    cs, _ = fc.case(name, 1)
    c = make_ctx(cs)
    Zd = dev(cs.Z)
    first = rollout_dev(c, Zd)
    check_knots(cs, first, fc.rollout_truth(name, 1), name)
    assert np.array_equal(first, rollout_dev(c, Zd)), "a second launch"
    for v in range(1, 17):
        c.set_option("cols_per_slice", v)
        assert np.array_equal(first, rollout_dev(c, Zd)), ("cols_per_slice", v)
    c.set_option("cols_per_slice", 0)
    for v in (1, 2, 5, cs.n):
        c.set_option("general_slices", v)
        assert np.array_equal(first, rollout_dev(c, Zd)), ("general_slices", v)
    c.set_option("cols_per_slice", 3)
    assert np.array_equal(first, rollout_dev(c, Zd)), "both splits at once"
    c.set_option("general_slices", 0)
    c.set_option("cols_per_slice", 0)
    buf = nans(first.size + 1)  # 8 bytes off a 16-byte boundary: the scalar stores
    assert buf.data_ptr() % 16 == 0
    c.rollout_dev(Zd, buf[1:])
    c.sync()
    assert np.array_equal(first, buf[1:].cpu().numpy()) and np.isnan(buf[:1].cpu().numpy()).all()
    c.set_stream(None)
    assert np.array_equal(first, c.rollout(cs.Z.reshape(-1)).reshape(-1)), "pcl_rollout on host pointers"
    c.close()


# ---- 3. the rollout tied to the constraint ------------------------------------------------------------------------------------------------------
def test_pade_residual_of_the_rollouts_states():
    cs = fc.pade_case("VL1")
    c = make_ctx(cs, order=10)
    X = rollout_dev(c, dev(cs.Z)).reshape(cs.N, cs.v + 1, cs.xdc)
    Zr = np.array(cs.Z)
    for b, o in enumerate(cs.xo):
        Zr[:, o : o + cs.xdc] = X[:, b]
    dd = nans(c.n_rows)
    c.eval_dev(dev(Zr), dd)
    c.sync()
    res = np.abs(dd.cpu().numpy()).max()
    print("VL1: order-10 residual of the rollout's states %.1e (max |X| %.2f)" % (res, np.abs(X).max()))
    assert res < 1e-11
    c.close()


# ---- 4. objective -----------------------------------------------------------------------------------------------------------------------------------
def obj_ctx(q):
    c = make_ctx(q.vc)
    g = q.goal
    if g[0] == "unitary":
        c.set_goal(fc.rs._iso_vec(g[1]))
    elif g[0] == "subspace":
        c.set_goal_subspace(fc.rs._iso_vec(g[1]), g[2])
    else:
        c.set_goal_form(0, g[1], g[2])
    c.set_weights(q.w)
    for r in q.regs:
        c.add_regularizer(*r)
    return c


def check_objective(c, q, what):
    Zf = q.vc.Z.reshape(-1)
    tv, tg, F = fc.objective_truth(q)
    value, grad = c.objective(Zf, q.Q)
    assert c.get_option("last_objective_launches") == 1
    ev = fc.rs.check_value(value[0], tv)
    eg = max(check_segments(grad, tg, fc.grad_labels(q), fc.OTOL).values())
    print("%s: value %.1e, gradient %.1e (F = %.4f)" % (what, ev, eg, float(F)))
    Zd, gd, vd = dev(Zf), nans(Zf.size), nans(1)
    c.objective_dev(Zd, q.Q, vd, gd)
    c.sync()
    assert np.array_equal(vd.cpu().numpy(), value) and np.array_equal(gd.cpu().numpy(), grad), what
    return value, grad


@pytest.mark.parametrize("kind", ["mat2", "sub2", "ket1", "mat3"])
def test_objective_value_and_gradient(kind):
    q = fc.obj_case(kind)
    c = obj_ctx(q)
    check_objective(c, q, kind)
    c.close()


def test_objective_hessian():
    """VL2 (three triangles of 2,372,931 entries; the regulariser on variation 1 is absorbed into that variation's triangle at the terminal knot)
    as a COO matrix with duplicates summed against the closed form, and H p against central differences of the device's gradient."""
    q = fc.obj_case("mat2")
    c = obj_ctx(q)
    Zf = q.vc.Z.reshape(-1)
    nvar = Zf.size
    rows, cols = c.objective_hess_structure()
    vals = c.objective_hess(Zf, q.Q, q.sigma)
    assert rows.size == vals.size and (rows >= cols).all() and cols.min() >= 0 and rows.max() < nvar and np.all(np.isfinite(vals))
    keys = rows.astype(np.int64) * nvar + cols
    z1 = (q.vc.N - 1) * q.vc.z_dim + q.vc.xo[1]  # inside the terminal variation 1 each position once: the absorbed diagonal is the triangle's
    inside = keys[(cols >= z1) & (rows < z1 + q.vc.xdc)]
    assert inside.size == q.vc.xdc * (q.vc.xdc + 1) // 2 and np.unique(inside).size == inside.size, "the absorbed diagonal is emitted twice"
    dk, inv = np.unique(keys, return_inverse=True)
    dv = np.bincount(inv, weights=vals, minlength=dk.size)
    tk, tv, labels = fc.hessian_truth(q)
    assert np.isin(tk[tv != 0], dk).all(), "entries of the truth are missing from the structure"
    extra = ~np.isin(dk, tk)
    assert not np.any(dv[extra] != 0.0), "values at positions the truth does not hold"
    sel = np.isin(tk, dk)
    errs = check_segments(dv[~extra], tv[sel], labels[sel], fc.OTOL)
    print("mat2: Hessian %.1e over %d entries (%s)" % (max(errs.values()), vals.size, ", ".join("%s %.1e" % kv for kv in sorted(errs.items()))))
    p = np.random.default_rng(7).standard_normal(nvar)
    off = rows != cols
    Hp = (np.bincount(rows, weights=vals * p[cols], minlength=nvar) + np.bincount(cols[off], weights=vals[off] * p[rows[off]], minlength=nvar)) / q.sigma
    gp, gm = c.objective(Zf + 1e-6 * p, q.Q)[1], c.objective(Zf - 1e-6 * p, q.Q)[1]
    fd = np.abs((gp - gm) / 2e-6 - Hp).max()
    print("mat2: H p against the gradient's central difference %.1e (max |H p| %.1e)" % (fd, np.abs(Hp).max()))
    assert fd <= 1e-6 * max(1.0, np.abs(Hp).max())
    c.close()


def test_ket_sensitivity_weight_and_oversized_subspace_are_refused():
    q = fc.obj_case("ket1")
    c = obj_ctx(q)
    refused(lambda: c.set_weights(np.array([1.0, 0.5])), ENOTIMPL, "pcl_set_weights: w[1]=0.5 on a ket context; the sensitivity objective is defined for unitaries only")
    check_objective(c, q, "ket1 after the refused weights")
    c.close()
    q = fc.obj_case("mat3")  # d = 48: 46 levels need 4234 rows of the form against 4096
    c = obj_ctx(q)
    value, _ = c.objective(q.vc.Z.reshape(-1), q.Q)
    refused(lambda: c.set_goal_subspace(fc.rs._iso_vec(np.eye(46)), np.arange(46)), ESHAPE, "pcl_set_goal_subspace", "46 levels", "4234", "4096", "45 levels at most")
    assert np.array_equal(c.objective(q.vc.Z.reshape(-1), q.Q)[0], value), "the goal set before the refusal is still in force"
    c.close()


# ---- 5. the option ------------------------------------------------------------------------------------------------------------------------------------
def _calls(c):
    """(the entry points the option serves -- eleven, with their device and host variants fourteen calls --, the ones it leaves refused), on
    small dummy buffers: only for a context that refuses them."""
    Lb, h = c._L, c._h
    buf = torch.zeros(64, dtype=torch.float64, device="cuda")
    hb, ib = np.zeros(64), np.zeros(64, dtype=np.int64)
    p, hp = buf.data_ptr(), hb.ctypes.data
    i64 = ib.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    i32 = ib.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    vp, f64, p64 = ctypes.c_void_p, ctypes.c_double, ctypes.POINTER(ctypes.c_int64)
    Lb.pcl_set_goal_form.argtypes = [vp, ctypes.c_int32, ctypes.c_int32, vp, vp]
    Lb.pcl_objective_hess_nnz.argtypes = [vp, p64]
    Lb.pcl_objective_hess_structure.argtypes = [vp, p64, p64]
    Lb.pcl_objective_hess_dev.argtypes = Lb.pcl_objective_hess.argtypes = [vp, vp, f64, f64, vp]
    served = {
        "pcl_set_goal": lambda: Lb.pcl_set_goal(h, hp),
        "pcl_set_goal_subspace": lambda: Lb.pcl_set_goal_subspace(h, hp, i32, 1),
        "pcl_set_goal_form": lambda: Lb.pcl_set_goal_form(h, 0, 1, hp, hp),
        "pcl_set_weights": lambda: Lb.pcl_set_weights(h, hp),
        "pcl_add_regularizer": lambda: Lb.pcl_add_regularizer(h, 0, 1, hp, 2),
        "pcl_clear_regularizers": lambda: Lb.pcl_clear_regularizers(h),
        "pcl_objective_dev": lambda: Lb.pcl_objective_dev(h, p, 1.0, p, p),
        "pcl_objective": lambda: Lb.pcl_objective(h, hp, 1.0, hp, hp),
        "pcl_objective_hess_nnz": lambda: Lb.pcl_objective_hess_nnz(h, i64),
        "pcl_objective_hess_structure": lambda: Lb.pcl_objective_hess_structure(h, i64, i64),
        "pcl_objective_hess_dev": lambda: Lb.pcl_objective_hess_dev(h, p, 1.0, 1.0, p),
        "pcl_objective_hess": lambda: Lb.pcl_objective_hess(h, hp, 1.0, 1.0, hp),
        "pcl_rollout": lambda: Lb.pcl_rollout(h, hp, hp),
        "pcl_rollout_dev": lambda: Lb.pcl_rollout_dev(h, p, p),
    }  # fmt: skip
    kept = {
        "pcl_infidelity_dev": lambda: Lb.pcl_infidelity_dev(h, p, 1.0, p, p),
        "pcl_hess_nnz": lambda: Lb.pcl_hess_nnz(h, i64, i64),
        "pcl_hess_dev": lambda: Lb.pcl_hess_dev(h, p, p, p),
        "pcl_jac_compact_nnz": lambda: Lb.pcl_jac_compact_nnz(h, i64, i64),
        "pcl_eval_jac_compact_dev": lambda: Lb.pcl_eval_jac_compact_dev(h, p, p, p),
        "pcl_jac_expand_dev": lambda: Lb.pcl_jac_expand_dev(h, p, p),
        "pcl_merit_grad_len": lambda: Lb.pcl_merit_grad_len(h, i64, i64),
        "pcl_merit_grad_dev": lambda: Lb.pcl_merit_grad_dev(h, p, p, p, p),
        "pcl_eval_jac_merit_dev": lambda: Lb.pcl_eval_jac_merit_dev(h, p, p, p, p, p),
        "pcl_eval_jac_merit_objective_dev": lambda: Lb.pcl_eval_jac_merit_objective_dev(h, p, p, p, p, p, 1.0, p, p),
        "pcl_set_member_window": lambda: Lb.pcl_set_member_window(h, 0, 1),
    }  # fmt: skip
    return served, kept, (buf, hb, ib)


def _all_refused(c, calls, n, exact=True):
    for name, call in calls.items():
        rc = call()
        msg = (c._L.pcl_last_error(c._h) or b"").decode()
        assert rc == ENOTIMPL and "PCL_LARGE_VAR" in msg, (name, rc, msg)
        if exact:
            assert msg == KIND_WORDS % (name, n), (name, msg)


def test_the_option_switches_its_entry_points_and_nothing_else():
    q = fc.obj_case("ket1")
    cs = fc.case("VL1", 1)[0]
    c = make_ctx(cs, full=False)
    assert c.large_variational and not c.large_var_full and c.get_option("large_var_full") == 0
    served, kept, keep_alive = _calls(c)
    _all_refused(c, served, 66)
    _all_refused(c, kept, 66, exact=False)
    refused(lambda: c.set_option("var_full", 1), ENOTIMPL, "PCL_LARGE_VAR", "var_full = 1")
    for bad in (2, -1):
        refused(lambda: c.set_option("large_var_full", bad), EINVAL, "large_var_full must be 0 or 1")
    c.set_option("large_var_full", 1)
    assert c.get_option("large_var_full") == 1 and c.large_var_full
    _all_refused(c, kept, 66, exact=False)
    refused(lambda: c.set_option("var_full", 1), ENOTIMPL, "PCL_LARGE_VAR", "var_full = 1")
    refused(lambda: c.hess_structure(), ENOTIMPL, "PCL_LARGE_VAR")
    assert c.get_option("var_full") == 0
    # served: the goal form, the regulariser and the value of ket1 on its own knots, the Hessian's structure, and the rollout
    c.set_goal_form(0, q.goal[1], q.goal[2])
    c.set_weights(q.w)
    for r in q.regs:
        c.add_regularizer(*r)
    check_objective(c, q, "ket1 with the option on")
    rows, cols = c.objective_hess_structure()
    assert rows.size == 66 * 67 // 2 + cs.N * (2 * cs.m + 1)
    assert np.all(np.isfinite(c.objective_hess(q.vc.Z.reshape(-1), q.Q, 1.0)))
    c.clear_regularizers()
    c.set_stream(None)
    X = c.rollout(cs.Z.reshape(-1))
    check_knots(cs, X, fc.rollout_truth("VL1", 1), "VL1 with the option on")
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    # back at 0: refused in the same words, and the goal is gone
    c.set_option("large_var_full", 0)
    assert not c.large_var_full and c.get_option("large_var_full") == 0
    _all_refused(c, served, 66)
    _all_refused(c, kept, 66, exact=False)
    c.set_option("large_var_full", 1)
    refused(lambda: c.objective(q.vc.Z.reshape(-1), q.Q), EINVAL, "no goal, no sensitivity weight and no regulariser set")
    c.set_option("large_var_full", 0)
    # after all of it: residual + Jacobian of the context still meet the truth of tests/var_large_cases.py on its knots
    base, _ = vl.case("VL1")
    dd, vd = nans(c.n_rows), nans(c.jac_nnz)
    c.eval_jac_dev(dev(base.Z), dd, vd)
    c.sync()
    vl.check("VL1", 8, dd.cpu().numpy(), vd.cpu().numpy(), 1e-11)
    c.close()
    del keep_alive


def test_the_option_elsewhere_is_invalid():
    import vector_shape_cases as vc

    words = "large_var_full = 1 needs a large variational context (PCL_BATCH_VARIATIONAL | PCL_LARGE_N | PCL_LARGE_VAR at a generator dimension above 64)"

    def everywhere_invalid(c, what):
        assert c.get_option("large_var_full") == 0, what
        refused(lambda: c.set_option("large_var_full", 1), EINVAL, words)
        refused(lambda: c.set_option("large_var_full", 2), EINVAL, "large_var_full must be 0 or 1")
        c.set_option("large_var_full", 0)
        assert c.get_option("large_var_full") == 0, what
        c.close()

    from oracle import pade_oracle as po
    from variational_truth import h_var_drift, make_case

    small = make_case(po.config_system(3), [po.G_of_H(h_var_drift(3, 3)) / 10], N=4, seed=3)  # n = 54
    assert small.n == 54
    args = vl.context_args(small, 4, batch_mode=VAR)
    flags = pa.integrators._PclContext(**args, large_generator=True, large_variational=True, large_var_full=True)  # all three flags at n <= 64: nothing is set
    assert not flags.large_variational and not flags.large_var_full
    everywhere_invalid(flags, "a variational context with all three flags at n = 54")
    everywhere_invalid(pa.integrators._PclContext(**args), "a plain variational context")
    lay, G0, Gj, Z, _ = vc.case("K5")  # n = 54
    pargs = dict(d=lay.d, m=lay.m, N=lay.N, z_dim=lay.z_dim, u_off=lay.u_off, dt_off=lay.dt_off, x_offs=[lay.x_off], G0=G0, Gj=Gj, batch=1,
                 batch_mode=MEMBERS, state_cols=lay.cols)  # fmt: skip
    everywhere_invalid(pa.integrators._PclContext(**pargs, pade_order=8), "an ordinary context")
    everywhere_invalid(pa.integrators._PclContext(**pargs, pade_order="exp"), "an exponential context")
    cs, _ = fc.case("VL1", 1)
    everywhere_invalid(plain_ctx(cs), "a plain large context")
    le = pa.integrators._PclContext(d=cs.n // 2, m=cs.m, N=cs.N, z_dim=cs.z_dim, u_off=cs.u_off, dt_off=cs.dt_off, x_offs=[cs.xo[0]], G0=cs.G0, Gj=cs.Gj,
                                    batch=1, batch_mode=MEMBERS, pade_order="exp", state_cols=cs.C, large_generator=True, large_exp=True)  # fmt: skip
    assert le.large_exp
    everywhere_invalid(le, "a large exponential context")


# ---- 6. the public constructor -----------------------------------------------------------------------------------------------------------------------
def test_public_constructor_end_to_end():
    q = fc.obj_case("mat2")
    cs = q.vc
    H0, Hd, Hv = vl.hamiltonians("VL2")
    sysv = pa.VariationalQuantumSystem(H0, list(Hd), list(Hv), [1.0] * cs.m)
    names = ["Ũ⃗", "Ũ⃗_var1", "Ũ⃗_var2"]
    comps = {"t": cs.Z[:, 0][None]}
    for nm, o in zip(names, cs.xo):
        comps[nm] = cs.Z[:, o : o + cs.xdc].T
    comps["Δt"] = cs.Z[:, cs.dt_off][None]
    comps["u"] = cs.Z[:, cs.u_off : cs.u_off + cs.m].T
    traj = pa.NamedTrajectory(comps, controls=("u", "Δt"), timestep="Δt")
    assert np.array_equal(traj.datavec, cs.Z.reshape(-1))
    kw = dict(scales=list(vl.SCALES[: cs.v]), pade_order=8, large_generator=True)
    B = pa.VariationalUnitaryIntegrator(sysv, traj, names[0], names[1:], "u", large_var_full=True, **kw)
    assert B.ctx.large_variational and B.ctx.large_var_full
    Qs = 0.7
    J = pa.UnitaryInfidelityObjective(q.goal[1], names[0], traj, Q=q.Q) + pa.UnitarySensitivityObjective(names[2], traj, [traj.N], Qs=[Qs])
    val, grad = J.bind(B).value_and_gradient(traj)
    ref = fc.types.SimpleNamespace(vc=cs, goal=q.goal, w=np.array([1.0, 0.0, Qs]), Q=q.Q, regs=[])
    tv, tg, _ = fc.objective_truth(ref)
    ev = fc.rs.check_value(float(val), tv)
    eg = max(check_segments(grad, tg, fc.grad_labels(ref), fc.OTOL).values())
    X = pa.variational_rollout(B, traj)
    assert X.shape == (cs.xd, cs.N)
    e = fc.knot_errors(X.T, fc.rollout_truth_values(cs).astype(np.float64), cs).max()  # (the objective case's own knots: short steps, a few pieces)
    print("VariationalUnitaryIntegrator, large_var_full=True: value %.1e gradient %.1e rollout %.1e" % (ev, eg, e))
    assert e <= fc.TOL
    B.close()
    B = pa.VariationalUnitaryIntegrator(sysv, traj, names[0], names[1:], "u", **kw)
    assert B.ctx.large_variational and not B.ctx.large_var_full
    for f, args in ((B.enable_objective_and_rollout, ()), (B.rollout, (traj,))):
        with pytest.raises(pa.PclError, match="PCL_LARGE_VAR") as ei:
            f(*args)
        assert ei.value.code == ENOTIMPL
    B.close()
