"""The objective family and the rollout at generator dimensions 66 .. 128 on the device (option large_full on a context created with
PCL_LARGE_N; piccolo.jl_amd/csrc/pcl_kernel_large_rollout.hpp, and the objective kernels of n <= 64 behind the option's gate), at the cases of
tests/large_full_cases.py, through the C ABI.

Rollout: every knot within TOL = 1e-11 of max |X_k| of the longdouble truth (the project's standing tolerance; tests/test_large_full_cpu.py
holds the float64 restatement of the kernel's algorithm to 1e-13), written into NaN-filled arrays; two launches, device and host pointers and
every split bit for bit; members with their own drifts, the member window, trajectory seeds; and the rollout's states put back into Z leave an
order-10 Pade residual below 1e-11 at steps |h| |G|_2 <= 0.3 (the Pade error there is of order theta^11 1e-10 = 2e-16).
Objective: the 1e-12 rule of tests/test_objective_shapes_gpu.py (value 1e-12 max(1, |ref|); gradient and Hessian 1e-12 max |ref| per segment)
against the longdouble closed forms of tests/objective_truth.py; the Hessian times a direction against central differences of the device's
gradient at 1e-6.
The option: the fifteen entry points it serves are refused at 0 in today's words and served at 1, the seven that stay refused are refused at
both values, back at 0 the goal is gone, and the option on n = 54, on an exponential and on a variational context is PCL_EINVAL.

Largest errors read on an MI355X: rollout 6.0e-16 of max |X_k| (L5, seed 1, knot 3; every other case and seed 3.5e-16 .. 5.2e-16); order-10
residual of the rollout's states 2.4e-16; objective value 1.5e-15 (ket5), gradient 2.3e-16, Hessian 2.3e-16 (L6, 2,372,943 entries), H p against
the gradient's central difference 5.4e-9 of the 1e-6 allowed; 45 levels of a d = 64 unitary: value 1.1e-14, gradient 2.1e-16.
Without the feature every test here fails: `large_full` is an unknown keyword and an unknown option."""
import ctypes

import numpy as np
import pytest
import torch

import large_full_cases as fc
import objective_cases as oc
import piccolo_jl_amd as pa
import vector_shape_cases as vc
from shape_cases import check_segments

pytestmark = pytest.mark.gpu
TOL = fc.TOL
OTOL = oc.TOL
EINVAL, ENOTIMPL, ESHAPE = pa._lib.PCL_EINVAL, pa._lib.PCL_ENOTIMPL, pa._lib.PCL_ESHAPE
MEMBERS, TRAJ = pa._lib.PCL_BATCH_MEMBERS, pa._lib.PCL_BATCH_TRAJ
NAN = float("nan")
N = fc.N


def make_ctx(lay, G0, Gj, order=8, full=True, **kw):
    args = dict(d=lay.d, m=lay.m, N=lay.N, z_dim=lay.z_dim, u_off=lay.u_off, dt_off=lay.dt_off, x_offs=[lay.x_off], G0=G0, Gj=Gj, batch=1,
                batch_mode=MEMBERS, pade_order=order, large_generator=True, large_full=full)  # fmt: skip
    if lay.gen is not None:
        args.update(d=lay.gen, state_cols=pa._lib.PCL_STATE_VECTOR)
    else:
        args.update(state_cols=lay.cols)
    args.update(kw)
    c = pa.integrators._PclContext(**args)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    return c


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float64).reshape(-1)).cuda()


def nans(k):
    return torch.full((k,), NAN, dtype=torch.float64, device="cuda")


def rollout_dev(c, Zd, members=1):
    out = nans(members * c.N * c.x_dim)
    c.rollout_dev(Zd, out)
    c.sync()
    got = out.cpu().numpy()
    assert not np.isnan(got).any()
    return got


def check_knots(got, ref, what):
    e = fc.knot_errors(got, ref)
    print("%s: rollout %.1e of max |X_k| (knot %d)" % (what, e.max(), int(e.argmax())))
    assert e[0] == 0 and e.max() <= TOL, (what, e)
    return e.max()


def refused(call, code, *words):
    with pytest.raises(pa.PclError) as ei:
        call()
    assert ei.value.code == code, str(ei.value)
    for w in words:
        assert w in str(ei.value), str(ei.value)
    return str(ei.value)


# ---- rollout: values ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.NAMES)
def test_rollout_values(name):
    lay, G0, Gj, Z, sp = fc.case(name)
    c = make_ctx(lay, G0, Gj)
    assert c.get_option("large_full") == 1 and c.large_full
    got = rollout_dev(c, dev(Z))
    assert c.get_option("last_kernel") == 270
    check_knots(got, fc.rollout_truth(name), "%s substeps %s" % (name, sp))
    # h = 0 on the last interval: E = I exactly, the last knot repeats the one before it bit for bit
    assert np.array_equal(got.reshape(N, -1)[N - 1], got.reshape(N, -1)[N - 2])
    c.close()


# ---- rollout: bits ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["L5", "L6"])
def test_rollout_bits(name):
    lay, G0, Gj, Z, _ = fc.case(name)
    c = make_ctx(lay, G0, Gj)
    Zd = dev(Z)
    first = rollout_dev(c, Zd)
    check_knots(first, fc.rollout_truth(name), name)
    assert np.array_equal(first, rollout_dev(c, Zd)), "a second launch"
    for v in range(1, lay.C + 1):
        c.set_option("cols_per_slice", v)
        assert np.array_equal(first, rollout_dev(c, Zd)), ("cols_per_slice", v)
    c.set_option("cols_per_slice", 0)
    for v in (1, 2, 5):
        c.set_option("general_slices", v)
        assert np.array_equal(first, rollout_dev(c, Zd)), ("general_slices", v)
    c.set_option("general_slices", 0)
    c.set_option("cols_per_slice", 2)
    c.set_option("general_slices", lay.n)  # one column of E per panel
    assert np.array_equal(first, rollout_dev(c, Zd)), "both splits at once"
    c.set_option("general_slices", 0)
    c.set_option("cols_per_slice", 0)
    c.set_stream(None)
    assert np.array_equal(first, c.rollout(Z).reshape(-1)), "pcl_rollout on host pointers"
    c.close()


def test_rollout_odd_n_on_an_unaligned_output():
    """L8 (n = 121): knots are not 16-byte aligned in memory whatever the base is; and an even n (L1) into an array 8 bytes off a 16-byte boundary
    takes the scalar stores: the same bits."""
    for name in ("L8", "L1"):
        lay, G0, Gj, Z, _ = fc.case(name)
        c = make_ctx(lay, G0, Gj)
        Zd = dev(Z)
        first = rollout_dev(c, Zd)
        buf = nans(N * lay.x_dim + 1)
        c.rollout_dev(Zd, buf[1:])
        c.sync()
        assert np.array_equal(first, buf[1:].cpu().numpy()) and np.isnan(buf[:1].cpu().numpy()).all(), name
        c.close()


# ---- rollout: scope -------------------------------------------------------------------------------------------------------------------------
def test_rollout_members_with_their_own_drifts_and_the_window():
    lay, _, Gj, Z, _ = fc.case("L1")
    drifts = (1, 2)
    G0s = [fc.case("L1", 0, b)[1] for b in drifts]
    c = make_ctx(lay, np.array(G0s), Gj, x_offs=[0, 0], batch=2, per_member_G0=True)
    Zd = dev(Z)
    got = rollout_dev(c, Zd, 2).reshape(2, -1)
    for b in range(2):
        check_knots(got[b], fc.rollout_truth("L1", 0, drifts[b]), "members, member %d" % b)
    c.set_member_window(1, 1)
    assert np.array_equal(got[1], rollout_dev(c, Zd, 1)), "the window on member 1"
    c.set_stream(None)
    assert np.array_equal(got[1], c.rollout(Z).reshape(-1)), "the window on member 1, host pointers"
    c.close()
    one = make_ctx(lay, G0s[1], Gj)
    assert np.array_equal(got[1], rollout_dev(one, Zd)), "member 1 alone"
    one.close()


@pytest.mark.parametrize("name", ["L5", "L8"])
def test_rollout_trajectory_seeds(name):
    lay, G0, Gj, _, _ = fc.case(name)
    Zs = [fc.case(name, s)[3] for s in range(2)]
    c = make_ctx(lay, G0, Gj, batch=2, batch_mode=TRAJ)
    Zd = dev(np.stack(Zs))
    got = rollout_dev(c, Zd, 2).reshape(2, -1)
    for s in range(2):
        check_knots(got[s], fc.rollout_truth(name, s), "%s seed %d substeps %s" % (name, s, fc.case(name, s)[4]))
    c.set_member_window(1, 1)
    assert np.array_equal(got[1], rollout_dev(c, Zd, 1)), "the window on seed 1"
    c.close()


# ---- rollout against the Pade constraint of the same context ---------------------------------------------------------------------------------
def test_pade_residual_of_the_rollouts_states():
    lay, G0, Gj, Z = fc.pade_case("L1")
    c = make_ctx(lay, G0, Gj, order=10)
    X = rollout_dev(c, dev(Z)).reshape(N, lay.x_dim)
    Zr = np.array(Z)
    Zr[:, lay.x_off : lay.x_off + lay.x_dim] = X
    dd = nans(c.n_rows)
    c.eval_dev(dev(Zr), dd)
    c.sync()
    res = np.abs(dd.cpu().numpy()).max()
    print("L1: order-10 residual of the rollout's states %.1e (max |X| %.2f)" % (res, np.abs(X).max()))
    assert res < 1e-11
    c.close()


# ---- objective ------------------------------------------------------------------------------------------------------------------------------------
def obj_ctx(case, full=True):
    c = pa.integrators._PclContext(d=case["d"], m=case["m"], N=case["N"], z_dim=case["z_dim"], u_off=case["u_off"], dt_off=case["dt_off"], x_offs=case["x_offs"],
                                   G0=case["G0"], Gj=case["Gj"], batch=case["batch"], batch_mode=TRAJ if case["traj"] else MEMBERS, state_cols=case["state_cols"],
                                   pade_order=8, large_generator=True, large_full=full)  # fmt: skip
    if not full:
        return c
    g = case["goal"]
    if g[0] == "unitary":
        c.set_goal(oc._iso_vec(g[1]))
    elif g[0] == "subspace":
        c.set_goal_subspace(oc._iso_vec(g[1]), g[2])
    else:
        c.set_goal_form(g[1], g[2], g[3])
    if case["weights"] is not None:
        c.set_weights(case["weights"])
    for off, dim, R, pw in case["regs"]:
        c.add_regularizer(off, dim, R, pw)
    return c


def check_objective(case, value, grad, what):
    tv, tg = oc.objective_truth(case)[:2]
    value, tv = np.asarray(value, float).reshape(-1), np.asarray(tv).reshape(-1)
    ev = float((np.abs(value - tv) / np.maximum(1, np.abs(tv))).max())
    assert np.all(np.isfinite(value)) and ev <= OTOL, (what, value, tv.astype(float), ev)
    eg = check_segments(grad, tg, oc.grad_labels(case), OTOL)
    print("%s: value %.1e, gradient %.1e" % (what, ev, max(eg.values())))


@pytest.mark.parametrize("name", list(fc.OBJ))
def test_objective_value_and_gradient(name):
    case = fc.OBJ[name]
    c = obj_ctx(case)
    assert c.large and c.large_full
    Zf = case["Z"].reshape(-1)
    value, grad = c.objective(Zf, case["Q"])
    assert c.get_option("last_objective_launches") == case["launches"], (name, c.get_option("last_objective_launches"))
    check_objective(case, value, grad, name)
    v2, _ = c.objective(Zf, case["Q"], want_grad=False)
    assert np.array_equal(v2, value)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    Zd, gd, vd = dev(Zf), nans(Zf.size), nans(value.size)
    c.objective_dev(Zd, case["Q"], vd, gd)
    c.sync()
    assert np.array_equal(vd.cpu().numpy(), value) and np.array_equal(gd.cpu().numpy(), grad), name
    if case["launches"] == 1:  # the two-launch route: the same bits
        c.set_option("objective_launches", 2)
        v3, g3 = c.objective(Zf, case["Q"])
        assert c.get_option("last_objective_launches") == 2 and np.array_equal(v3, value) and np.array_equal(g3, grad)
    c.close()


@pytest.mark.parametrize("name", ["mat3", "sub4"])
def test_infidelity_terms(name):
    import objective_truth as ot

    case = fc.OBJ[name]
    c = obj_ctx(case)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    vd, gd = nans(case["batch"]), nans(case["batch"] * case["x_dim"])
    c.infidelity_dev(dev(case["Z"]), case["Q"], vd, gd)
    c.sync()
    ref = [ot.form_loss(A, cc, x, ot.LD(w) * ot.LD(case["Q"]))[:2] for A, cc, x, w, idx, keep in oc.terms(case)]
    rv, rg = np.array([r[0] for r in ref]), np.concatenate([r[1] for r in ref])
    got = vd.cpu().numpy()
    assert (np.abs(got - rv) / np.maximum(1, np.abs(rv))).max() <= OTOL
    check_segments(gd.cpu().numpy(), rg, np.repeat(np.arange(case["batch"]).astype(str), case["x_dim"]), OTOL)
    c.close()


def device_hessian(case, c, sigma):
    rows, cols = c.objective_hess_structure()
    vals = c.objective_hess(case["Z"].reshape(-1), case["Q"], sigma)
    nvar = case["Z"].size
    assert rows.size == vals.size and (rows >= cols).all() and cols.min() >= 0 and rows.max() < nvar and np.all(np.isfinite(vals))
    keys = rows * nvar + cols
    ukeys, inv = np.unique(keys, return_inverse=True)
    return ukeys, np.bincount(inv, weights=vals, minlength=ukeys.size), (rows, cols, vals)


@pytest.mark.parametrize("name", [n for n in fc.OBJ if fc.OBJ[n]["hess"]])
def test_objective_hessian(name):
    """L6 (mat1: a triangle of 2,372,931 entries; sub4) and L5 (coh5) as COO matrices with duplicates summed against the closed form, and H p
    against central differences of the device's gradient."""
    case = fc.OBJ[name]
    c = obj_ctx(case)
    tk, tv, labels = oc.hessian_truth(case)
    dk, dv, (r, cc, v) = device_hessian(case, c, case["sigma"])
    assert np.isin(tk[tv != 0], dk).all(), "entries of the truth are missing from the structure"
    extra = ~np.isin(dk, tk)
    assert not np.any(dv[extra] != 0.0), "values at positions the truth does not hold"
    errs = check_segments(dv[~extra], tv, labels, OTOL)
    print("%s: Hessian %.1e over %d entries" % (name, max(errs.values()), v.size))
    z0 = case["Z"].reshape(-1)
    p = np.random.default_rng(7).standard_normal(z0.size)
    off = r != cc
    Hp = (np.bincount(r, weights=v * p[cc], minlength=z0.size) + np.bincount(cc[off], weights=v[off] * p[r[off]], minlength=z0.size)) / case["sigma"]
    gp, gm = c.objective(z0 + 1e-6 * p, case["Q"])[1], c.objective(z0 - 1e-6 * p, case["Q"])[1]
    fd = np.abs((gp - gm) / 2e-6 - Hp).max()
    print("%s: H p against the gradient's central difference %.1e (max |H p| %.1e)" % (name, fd, np.abs(Hp).max()))
    assert fd <= 1e-6 * max(1.0, np.abs(Hp).max())
    c.close()


# ---- the option -------------------------------------------------------------------------------------------------------------------------------------
def _calls(c):
    """(the fifteen entry points the option serves, the seven it leaves refused), on small dummy buffers: only for a context that refuses them."""
    L, h = c._L, c._h
    buf = torch.zeros(64, dtype=torch.float64, device="cuda")
    hb, ib = np.zeros(64), np.zeros(64, dtype=np.int64)
    p, hp = buf.data_ptr(), hb.ctypes.data
    i64 = ib.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    i32 = ib.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    vp, f64, p64 = ctypes.c_void_p, ctypes.c_double, ctypes.POINTER(ctypes.c_int64)
    L.pcl_set_goal_form.argtypes = [vp, ctypes.c_int32, ctypes.c_int32, vp, vp]
    L.pcl_objective_hess_nnz.argtypes = [vp, p64]
    L.pcl_objective_hess_structure.argtypes = [vp, p64, p64]
    L.pcl_objective_hess_dev.argtypes = L.pcl_objective_hess.argtypes = [vp, vp, f64, f64, vp]
    served = {
        "pcl_set_goal": lambda: L.pcl_set_goal(h, hp),
        "pcl_set_goal_subspace": lambda: L.pcl_set_goal_subspace(h, hp, i32, 1),
        "pcl_set_goal_form": lambda: L.pcl_set_goal_form(h, 0, 1, hp, hp),
        "pcl_set_weights": lambda: L.pcl_set_weights(h, hp),
        "pcl_add_regularizer": lambda: L.pcl_add_regularizer(h, 0, 1, hp, 2),
        "pcl_clear_regularizers": lambda: L.pcl_clear_regularizers(h),
        "pcl_infidelity_dev": lambda: L.pcl_infidelity_dev(h, p, 1.0, p, p),
        "pcl_objective_dev": lambda: L.pcl_objective_dev(h, p, 1.0, p, p),
        "pcl_objective": lambda: L.pcl_objective(h, hp, 1.0, hp, hp),
        "pcl_objective_hess_nnz": lambda: L.pcl_objective_hess_nnz(h, i64),
        "pcl_objective_hess_structure": lambda: L.pcl_objective_hess_structure(h, i64, i64),
        "pcl_objective_hess_dev": lambda: L.pcl_objective_hess_dev(h, p, 1.0, 1.0, p),
        "pcl_objective_hess": lambda: L.pcl_objective_hess(h, hp, 1.0, 1.0, hp),
        "pcl_rollout": lambda: L.pcl_rollout(h, hp, hp),
        "pcl_rollout_dev": lambda: L.pcl_rollout_dev(h, p, p),
    }  # fmt: skip
    kept = {
        "pcl_jac_compact_nnz": lambda: L.pcl_jac_compact_nnz(h, i64, i64),
        "pcl_eval_jac_compact_dev": lambda: L.pcl_eval_jac_compact_dev(h, p, p, p),
        "pcl_jac_expand_dev": lambda: L.pcl_jac_expand_dev(h, p, p),
        "pcl_merit_grad_len": lambda: L.pcl_merit_grad_len(h, i64, i64),
        "pcl_merit_grad_dev": lambda: L.pcl_merit_grad_dev(h, p, p, p, p),
        "pcl_eval_jac_merit_dev": lambda: L.pcl_eval_jac_merit_dev(h, p, p, p, p, p),
        "pcl_eval_jac_merit_objective_dev": lambda: L.pcl_eval_jac_merit_objective_dev(h, p, p, p, p, p, 1.0, p, p),
    }  # fmt: skip
    assert len(served) == 15 and len(kept) == 7
    return served, kept, (buf, hb, ib)


def _all_refused(c, calls, n):
    for name, call in calls.items():
        rc = call()
        msg = (c._L.pcl_last_error(c._h) or b"").decode()
        assert rc == ENOTIMPL and msg == "%s is not implemented for a context created with PCL_LARGE_N (generator dimension %d > 64): residual and Jacobian only" % (name, n), (name, rc, msg)


def test_the_option_switches_its_entry_points_and_nothing_else():
    case = fc.OBJ["mat1"]
    c = obj_ctx(case, full=False)
    assert c.large and not c.large_full and c.get_option("large_full") == 0 and c.get_option("large_hess") == 0
    served, kept, keep_alive = _calls(c)
    _all_refused(c, served, 66)
    _all_refused(c, kept, 66)
    for bad in (2, -1):
        refused(lambda: c.set_option("large_full", bad), EINVAL, "large_full")
    c.set_option("large_full", 1)
    assert c.get_option("large_full") == 1 and c.large_full and c.get_option("large_hess") == 0
    _all_refused(c, kept, 66)
    # served: the goal, the regulariser and the value of the case, and the rollout
    Zf = case["Z"].reshape(-1)
    c.set_goal(oc._iso_vec(case["goal"][1]))
    for off, dim, R, pw in case["regs"]:
        c.add_regularizer(off, dim, R, pw)
    value, grad = c.objective(Zf, case["Q"])
    check_objective(case, value, grad, "mat1 with the option on")
    rows, cols = c.objective_hess_structure()
    assert rows.size == 2178 * 2179 // 2 + N * (2 * 1 + 1)
    X = c.rollout(Zf)
    assert X.shape == (1, N, 2178) and np.array_equal(X[0, 0], case["Z"][0, 0, :2178])
    # independent of large_hess: the Hessian of the Lagrangian stays refused until its own option is set, and setting that changes nothing here
    with pytest.raises(pa.PclError) as ei:
        c.hess_structure(np.int32)
    assert ei.value.code == ENOTIMPL
    c.set_option("large_hess", 1)
    assert c.get_option("large_full") == 1 and np.array_equal(c.objective(Zf, case["Q"])[0], value)
    c.set_option("large_hess", 0)
    # back at 0: refused in the same words, and the goal and the regulariser are gone
    c.set_option("large_full", 0)
    assert not c.large_full
    _all_refused(c, served, 66)
    _all_refused(c, kept, 66)
    c.set_option("large_full", 1)
    refused(lambda: c.objective(Zf, case["Q"]), EINVAL, "no goal and no regulariser set")
    c.set_goal(oc._iso_vec(case["goal"][1]))
    v2, _ = c.objective(Zf, case["Q"])  # (no regulariser any more: the infidelity alone)
    member = np.asarray(oc.objective_truth(case)[2], float)
    assert abs(v2[0] - member[0]) <= OTOL * max(1, abs(member[0]))
    c.close()
    del keep_alive


def test_the_option_elsewhere_is_invalid():
    lay, G0, Gj, Z, _ = vc.case("K5")  # n = 54: the flag gives the ordinary context
    args = dict(d=lay.d, m=lay.m, N=lay.N, z_dim=lay.z_dim, u_off=lay.u_off, dt_off=lay.dt_off, x_offs=[lay.x_off], G0=G0, Gj=Gj, batch=1,
                batch_mode=MEMBERS, state_cols=lay.cols)  # fmt: skip
    for kw in (dict(pade_order=8, large_generator=True), dict(pade_order=8), dict(pade_order="exp")):
        c = pa.integrators._PclContext(**args, **kw)
        assert c.get_option("large_full") == 0
        refused(lambda: c.set_option("large_full", 1), EINVAL, "large_full")
        refused(lambda: c.set_option("large_full", 7), EINVAL, "large_full")
        c.set_option("large_full", 0)
        c.close()
    # both keywords at n <= 64: the option is not set and the ordinary context serves the rollout as it does without them
    c = pa.integrators._PclContext(**args, pade_order=8, large_generator=True, large_full=True)
    assert not c.large and not c.large_full and c.get_option("large_full") == 0
    plain = pa.integrators._PclContext(**args, pade_order=8)
    assert np.array_equal(c.rollout(Z), plain.rollout(Z))
    c.close()
    plain.close()
    # a variational context (config 2 with one variation)
    import robust_truth as rt
    from oracle import pade_oracle as po
    from variational_truth import h_var_drift, make_case

    v = rt.var_context(pa, make_case(po.config_system(2), [po.G_of_H(h_var_drift(2, 2)) / 10], N=4, seed=3))
    assert v.get_option("large_full") == 0
    refused(lambda: v.set_option("large_full", 1), EINVAL, "large_full")
    v.set_option("large_full", 0)
    v.close()


# ---- subspace limits --------------------------------------------------------------------------------------------------------------------------------
def test_subspace_goals_beyond_the_form_and_the_lds_are_refused():
    """A unitary of d = 64 (n = 128): 46 levels need 4234 rows of the terminal form against 4096, 59 levels 167,088 B of LDS against 163,840; both
    are PCL_ESHAPE with their numbers at pcl_set_goal_subspace, before any launch; 45 levels (97,200 B, over the 64 KB a kernel has without
    asking) are served."""
    d, n = 64, 128
    rng = np.random.default_rng(16900)
    from oracle import pade_oracle as po

    G0, Gj = po.G_of_H(vc._herm(d, rng)), np.array([po.G_of_H(vc._herm(d, rng))])
    xd = n * d
    c = pa.integrators._PclContext(d=d, m=1, N=2, z_dim=xd + 3, u_off=xd + 2, dt_off=xd, x_offs=[0], G0=G0, Gj=Gj, batch=1, batch_mode=MEMBERS, pade_order=4,
                                   large_generator=True, large_full=True)  # fmt: skip
    for ns, words in ((46, ("4234", "4096", "rows")), (58, ("6730", "4096", "rows")), (59, ("167088", "163840", "LDS")), (64, ("196608", "163840", "LDS"))):
        sub = np.arange(ns)
        refused(lambda: c.set_goal_subspace(oc._iso_vec(np.eye(ns)), sub), ESHAPE, "pcl_set_goal_subspace", *words)
    refused(lambda: c.objective(np.zeros(2 * (xd + 3)), 1.0), EINVAL, "no goal")  # nothing was set by the refused calls
    ns = 45
    sub = rng.permutation(d)[:ns]
    Gs = oc._unitary(ns, rng)
    U = 0.3 * (rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d)))
    U[np.ix_(sub, sub)] = oc._near(Gs, 0.9, rng)
    c.set_goal_subspace(oc._iso_vec(Gs), sub)
    Z = 0.4 * rng.standard_normal((1, 2, xd + 3))
    Z[0, 1, :xd] = oc._iso_vec(U)
    import objective_truth as ot

    tv, tg, F = fc.subspace_loss_ld(Z[0, 1, :xd], Gs, sub, d, ot.LD(100.0))  # (the rows of the general form would take half a gigabyte here)
    ref_g = np.zeros(Z.shape, dtype=ot.LD)
    ref_g[0, 1, :xd] = tg
    labels = np.full(Z.shape, "k0", dtype="U4")
    labels[0, 1], labels[0, 1, :xd] = "k1", "x"
    for launches in (0, 2):  # the one-launch route and the two launches: more than 64 KB of dynamic LDS in either kernel
        c.set_option("objective_launches", launches)
        value, grad = c.objective(Z.reshape(-1), 100.0)
        assert c.get_option("last_objective_launches") == (launches or 1)
        assert abs(value[0] - float(tv)) <= OTOL * max(1, abs(float(tv))), (value, float(tv))
        e = check_segments(grad, ref_g, labels, OTOL)
        print("45 levels of 64 (F = %.3f), %d launch(es): value %.1e, gradient %.1e" % (float(F), launches or 1, abs(value[0] - float(tv)), max(e.values())))
    c.close()


# ---- the public interface ---------------------------------------------------------------------------------------------------------------------------
def test_bilinear_integrator_keyword():
    import large_hess_cases as hc
    from oracle import pade_oracle as po

    s, traj, Z, lay = hc.ket33_problem()
    KET = pa.trajectory.KET
    B = pa.BilinearIntegrator(s, traj, x_name=KET, pade_order=8, large_generator=True, large_full=True)
    assert B.ctx.large and B.ctx.large_full and not B.ctx.large_hessian
    X = B.ctx.rollout(traj.datavec)[0]
    ref = po.exact_rollout(Z, lay, s.G_drift, s.G_drives_array())
    e = fc.knot_errors(X, ref)
    print("d = 33 ket: rollout against scipy's expm %.1e" % e.max())
    assert e.max() <= TOL
    psi_goal = (X[-1, :33] + 1j * X[-1, 33:]) * np.exp(0.3j)
    obj = pa.Objective([pa.KetInfidelityObjective(psi_goal, KET, Q=100.0), pa.QuadraticRegularizer("u", traj, 0.1)]).bind(B)
    Zr = Z.copy()
    Zr[:, lay.x_off : lay.x_off + lay.x_dim] = X
    J, g = obj.value_and_gradient(Zr.reshape(-1))
    reg = 0.5 * 0.1 * float((Zr[:, lay.dt_off] ** 2 * (Zr[:, lay.u_off : lay.u_off + lay.m] ** 2).sum(axis=1)).sum())
    print("d = 33 ket: the objective at the rollout's terminal state %.3e (the regulariser alone %.3e)" % (J, reg))
    assert abs(J - reg) <= 1e-10 and g.shape == (Zr.size,)  # the goal is the rollout's own terminal state up to a phase: fidelity 1
    B.close()
