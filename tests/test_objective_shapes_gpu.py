"""GPU tests of the objective-side kernels -- terminal losses (pcl_infidelity_kernel, pcl_form_kernel), regularisers (pcl_regularizer_body), the
objective's Hessian (pcl_gram_kernel, pcl_scale_kernel, pcl_reg_hess_kernel), the derivative / time-consistency rows (pcl_deriv_kernel) and the
reduce payload (pcl_merit_part_kernel, pcl_merit_sum_kernel, pcl_merit_finish_body) -- at the sizes of tests/objective_cases.py: sums of more
than 256 elements (d = 17 .. 32, L up to 2560), d^2 = 256 exactly, subspaces of 1 .. 1024 entries, Gram triangles that wrap the 4096 x 256
and the 8192 x 256 grids (3.28 M entries), eight regularisers on N = 2, 65 and 100 knots, m = 7, 9 and 24 drives, an odd generator dimension
and six output sets; through pa.integrators._PclContext (the C ABI), against the longdouble truth of tests/objective_truth.py.

Tolerances (the project's own): value 1e-12 max(1, |ref|); gradient, Hessian and payload 1e-12 max|ref| per segment, no floor at 1
(shape_cases.check_segments).  The Hessian times a direction against central differences of the device's own gradient: 1e-6."""
import numpy as np
import pytest

import objective_cases as oc
import objective_truth as ot
import piccolo_jl_amd as pa
from objective_cases import CASES, PAYLOAD_CASES, TOL
from oracle import pade_oracle as po
from shape_cases import check_segments

pytestmark = pytest.mark.gpu
ESHAPE = pa._lib.PCL_ESHAPE
MEMBERS, TRAJ = pa._lib.PCL_BATCH_MEMBERS, pa._lib.PCL_BATCH_TRAJ


def show(part, name, errs):
    """Print the worst relative error of a check (pytest -s shows it)."""
    print("REL part %s case %s worst %.3e" % (part, name, max(errs.values()) if isinstance(errs, dict) else float(errs)))


def ctx_of(case, mirror_rows=False):
    c = pa.integrators._PclContext(d=case["d"], m=case["m"], N=case["N"], z_dim=case["z_dim"], u_off=case["u_off"], dt_off=case["dt_off"],
                                   x_offs=case["x_offs"], G0=case["G0"], Gj=case["Gj"], batch=case["batch"], batch_mode=TRAJ if case["traj"] else MEMBERS,
                                   index_base=case["index_base"], state_cols=case["state_cols"])  # fmt: skip
    g = case["goal"]
    if g[0] == "unitary":
        c.set_goal(oc._iso_vec(g[1]))
    elif g[0] == "subspace":
        c.set_goal_subspace(oc._iso_vec(g[1]), g[2])
    elif mirror_rows:  # the rows the host mirror builds (piccolo.jl_amd/objectives.py), held to the same truth
        if "ket_goal" in case:
            c.set_goal_form(*pa.KetInfidelityObjective(case["ket_goal"], "psi").form(case["x_dim"], case["batch"]))
        else:
            goals, cw = case["coherent"]
            c.set_goal_form(*pa.CoherentKetInfidelityObjective(goals, ["k%d" % i for i in range(len(goals))], weights=cw).form(case["x_dim"], case["batch"]))
    else:
        c.set_goal_form(g[1], g[2], g[3])
    if case["weights"] is not None:
        c.set_weights(case["weights"])
    for off, dim, R, pw in case["regs"]:
        c.add_regularizer(off, dim, R, pw)
    return c


def check_value(got, ref, what):
    got, ref = np.asarray(got, float).reshape(-1), np.asarray(ref).reshape(-1)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref) / np.maximum(1, np.abs(ref))
    assert np.all(np.isfinite(got)) and float(err.max()) <= TOL, "%s: %r against %r (rel %.3e)" % (what, got, ref.astype(float), float(err.max()))
    return float(err.max())


def check_objective(case, value, grad, truth, what):
    tv, tg = truth[0], truth[1]
    ev = check_value(value, tv, what + " value")
    eg = check_segments(grad, tg, oc.grad_labels(case), TOL)
    return max(ev, max(eg.values()))


# ---- A - D: value and gradient of the whole objective, both pointer paths ------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_objective_value_and_gradient(name):
    import torch

    case = CASES[name]
    truth = oc.objective_truth(case)
    c = ctx_of(case)
    Zf = case["Z"].reshape(-1)
    # host pointers
    value, grad = c.objective(Zf, case["Q"])
    if case["launches"] is not None:
        assert c.get_option("last_objective_launches") == case["launches"], (name, c.get_option("last_objective_launches"))
    worst = check_objective(case, value, grad, truth, name)
    # value alone (no gradient buffer: the launches that do not write one)
    v2, _ = c.objective(Zf, case["Q"], want_grad=False)
    assert np.array_equal(v2, value)
    # device pointers; the gradient buffer 8 bytes off a 16-byte boundary (with an odd z_dim both zeroing branches of a row run either way)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    Zd = torch.from_numpy(Zf).cuda()
    for shift in (0, 1):
        gd = torch.full((Zf.size + 1,), float("nan"), dtype=torch.float64, device="cuda")[shift : shift + Zf.size]
        vd = torch.empty(value.size, dtype=torch.float64, device="cuda")
        c.objective_dev(Zd, case["Q"], vd, gd)
        torch.cuda.synchronize()
        assert np.array_equal(vd.cpu().numpy(), value) and np.array_equal(gd.cpu().numpy(), grad), (name, shift)
    # the other launch arrangement where there is one (regulariser + infidelity launches): the same bits
    if case["launches"] == 1:
        c.set_option("objective_launches", 2)
        v3, g3 = c.objective(Zf, case["Q"])
        assert c.get_option("last_objective_launches") == 2 and np.array_equal(v3, value) and np.array_equal(g3, grad)
    show(name[0], name, worst)
    c.close()


@pytest.mark.parametrize("name", [n for n in CASES if CASES[n]["goal"][0] in ("unitary", "subspace")])
def test_infidelity_terms_and_member_gradients(name):
    """pcl_infidelity_dev: the terms w_b Q |1 - F_b| and every member's own x_dim gradient slot (overwritten, not added to)."""
    import torch

    case = CASES[name]
    c = ctx_of(case)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    Zd = torch.from_numpy(case["Z"].reshape(-1)).cuda()
    vd = torch.empty(case["batch"], dtype=torch.float64, device="cuda")
    gd = torch.full((case["batch"] * case["x_dim"],), float("nan"), dtype=torch.float64, device="cuda")
    c.infidelity_dev(Zd, case["Q"], vd, gd)
    torch.cuda.synchronize()
    ref_v, ref_g = [], []
    for A, cc, x, w, idx, keep in oc.terms(case):
        v, g, _, _ = ot.form_loss(A, cc, x, ot.LD(w) * ot.LD(case["Q"]))
        ref_v.append(v), ref_g.append(g)
    e = check_value(vd.cpu().numpy(), np.array(ref_v), name)
    eg = check_segments(gd.cpu().numpy(), np.concatenate(ref_g), np.repeat(np.arange(case["batch"]).astype(str), case["x_dim"]), TOL)
    show(name[0], name + " (terms)", max(e, max(eg.values())))
    c.close()


@pytest.mark.parametrize("name", ["Cket", "Ccoh5"])
def test_rows_of_the_host_mirror_on_the_device(name):
    case = CASES[name]
    c = ctx_of(case, mirror_rows=True)
    value, grad = c.objective(case["Z"].reshape(-1), case["Q"])
    assert c.get_option("last_objective_launches") == 3
    show("C", name + " (mirror rows)", check_objective(case, value, grad, oc.objective_truth(case), name))
    c.close()


def test_a_ninth_regulariser_is_refused():
    case = CASES["Deight"]
    c = ctx_of(case)
    with pytest.raises(pa.PclError) as ei:
        c.add_regularizer(case["dt_off"] + 2, 2, 1.0, 2)
    assert ei.value.code == ESHAPE
    value, grad = c.objective(case["Z"].reshape(-1), case["Q"])  # the eight stay as they were
    check_objective(case, value, grad, oc.objective_truth(case), "Deight")
    c.close()


# ---- E: Hessian of the objective ---------------------------------------------------------------------------------------------------------------------
def device_hessian(case, c, sigma):
    rows, cols = c.objective_hess_structure()
    vals = c.objective_hess(case["Z"].reshape(-1), case["Q"], sigma)
    base, nvar = case["index_base"], case["Z"].size
    assert rows.size == vals.size and (rows >= cols).all() and cols.min() >= base and rows.max() < nvar + base
    assert np.all(np.isfinite(vals))
    keys = (rows - base) * nvar + (cols - base)
    ukeys, inv = np.unique(keys, return_inverse=True)
    return ukeys, np.bincount(inv, weights=vals, minlength=ukeys.size), (rows - base, cols - base, vals)


@pytest.mark.parametrize("name", [n for n in CASES if CASES[n]["hess"]])
def test_objective_hessian_as_a_coo_matrix(name):
    case = CASES[name]
    c = ctx_of(case)
    tk, tv, labels = oc.hessian_truth(case)
    dk, dv, _ = device_hessian(case, c, case["sigma"])
    assert np.isin(tk[tv != 0], dk).all(), "entries of the truth are missing from the structure"
    extra = ~np.isin(dk, tk)
    assert not np.any(dv[extra] != 0.0), "values at positions the truth does not hold"
    errs = check_segments(dv[~extra], tv, labels, TOL)
    show("E", name, errs)
    c.close()


def test_hessian_times_directions_is_the_difference_of_the_device_gradient():
    case = CASES["Dstate"]
    c = ctx_of(case)
    _, _, (r, cc, v) = device_hessian(case, c, 1.0)
    z0 = case["Z"].reshape(-1)
    rng = np.random.default_rng(5)
    off = r != cc
    for _ in range(3):
        p = rng.standard_normal(z0.size)
        Hp = np.bincount(r, weights=v * p[cc], minlength=z0.size) + np.bincount(cc[off], weights=v[off] * p[r[off]], minlength=z0.size)
        gp, gm = c.objective(z0 + 1e-6 * p, case["Q"])[1], c.objective(z0 - 1e-6 * p, case["Q"])[1]
        assert np.abs((gp - gm) / 2e-6 - Hp).max() <= 1e-6 * max(1.0, np.abs(Hp).max()), np.abs((gp - gm) / 2e-6 - Hp).max()
    c.close()


# ---- F: derivative and time-consistency rows -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [0, 1])
def test_derivative_rows_of_24_components_on_three_buffers(base):
    import torch

    lay, G0, Gj, Z1, x_offs, w, _, sc = oc.payload_case("P24")
    S, dim = 3, lay.m
    Z = 0.4 * np.random.default_rng(8).standard_normal((S, lay.N, lay.z_dim))
    c = pa.integrators._PclContext(d=lay.d, m=lay.m, N=lay.N, z_dim=lay.z_dim, u_off=lay.u_off, dt_off=lay.dt_off, x_offs=x_offs[:1], G0=G0, Gj=Gj,
                                   batch=S, batch_mode=TRAJ, index_base=base)  # fmt: skip
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    for dx_off in (lay.u_off + dim, -1):
        ref = [ot.deriv_rows(Z[b], lay.u_off, dx_off, dim, lay.dt_off, z0=b * lay.N * lay.z_dim, r0=b * lay.K * dim, index_base=base) for b in range(S)]
        res, rows, cols, vals = (np.concatenate([r[i] for r in ref]) for i in range(4))
        r, cc = c.deriv_structure(lay.u_off, dx_off, dim)
        assert np.array_equal(r, rows) and np.array_equal(cc, cols)
        delta, v = c.deriv_eval_jac(lay.u_off, dx_off, dim, Z)
        e1 = check_segments(delta, res, np.repeat(np.arange(S * lay.K).astype(str), dim), TOL)
        seg = np.tile(np.repeat(np.array(["-1", "+1", "-h", "-dx"] if dx_off >= 0 else ["-1", "+1", "-one"]), dim), S * lay.K)
        e2 = check_segments(v, vals, seg, TOL)
        nr, nnz = c.deriv_dims(dx_off, dim)
        dd, vd = torch.empty(nr, dtype=torch.float64, device="cuda"), torch.empty(nnz, dtype=torch.float64, device="cuda")
        c.deriv_eval_jac_dev(lay.u_off, dx_off, dim, torch.from_numpy(Z.reshape(-1)).cuda(), dd, vd)
        torch.cuda.synchronize()
        assert np.array_equal(dd.cpu().numpy(), delta) and np.array_equal(vd.cpu().numpy(), v)
        show("F", "dx_off %d base %d" % (dx_off, base), max(max(e1.values()), max(e2.values())))
    c.close()


# ---- G: reduce payload ---------------------------------------------------------------------------------------------------------------------------------
FUSED_PAYLOAD = ("Ptraj6",)  # the cases whose payload pcl_eval_jac_merit_dev forms inside the Jacobian kernel; every other one: the separate kernels


@pytest.mark.parametrize("name", list(PAYLOAD_CASES))
def test_reduce_payload(name):
    """[phi | J' lam on (u_k, dt_k)] from the separate kernels (pcl_merit_grad_dev) and from pcl_eval_jac_merit_dev (fused into the Jacobian kernel
    where that applies: `last_merit_fused`, printed and asserted), lam = delta and a given lam, with weights; the reference takes the ORACLE's Jacobian and
    residual and forms the dot products in longdouble."""
    import torch

    lay, G0, Gj, Z, x_offs, w, traj, sc = oc.payload_case(name)
    nbuf, M = len(Z), len(x_offs)
    d = lay.n if sc else lay.d
    c = pa.integrators._PclContext(d=d, m=lay.m, N=lay.N, z_dim=lay.z_dim, u_off=lay.u_off, dt_off=lay.dt_off, x_offs=x_offs, G0=G0, Gj=Gj,
                                   batch=traj or M, batch_mode=TRAJ if traj else MEMBERS, state_cols=sc)  # fmt: skip
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    c.set_weights(w)
    order = c.pade_order
    J = [[po.pade_jacobian_dense(Z[s], lay, G0, Gj, order, x_off=o) for o in x_offs] for s in range(nbuf)]
    delta = [[po.pade_residual(Z[s], lay, G0, Gj, order, x_off=o).reshape(-1) for o in x_offs] for s in range(nbuf)]
    ln, sets = c.merit_grad_len()
    assert (ln, sets) == (1 + lay.K * lay.m + lay.K, nbuf)
    lam = np.random.default_rng(6).standard_normal((nbuf, M, lay.K * lay.x_dim))
    Zd = torch.from_numpy(Z.reshape(-1)).cuda()
    dd, vd = torch.empty(c.n_rows, dtype=torch.float64, device="cuda"), torch.empty(c.jac_nnz, dtype=torch.float64, device="cuda")
    labels = np.tile(np.array(["phi"] + ["gu"] * (lay.K * lay.m) + ["gdt"] * lay.K), nbuf)
    labels = np.char.add(labels, np.repeat(np.char.add("@", np.arange(nbuf).astype(str)), ln))
    for lm in (None, lam):
        ref = np.concatenate([ot.payload(J[s], None if lm is None else lm[s], delta[s], [w[s]] if traj else w, lay.N, lay.z_dim, lay.u_off, lay.m, lay.dt_off)
                              for s in range(nbuf)])  # fmt: skip
        lam_d = None if lm is None else torch.from_numpy(lm.reshape(-1)).cuda()
        out = torch.full((ln * sets,), float("nan"), dtype=torch.float64, device="cuda")
        c.eval_jac_dev(Zd, dd, vd)
        c.merit_grad_dev(dd, lam_d, vd, out)
        torch.cuda.synchronize()
        show("G", "%s separate kernels, lam %s" % (name, "delta" if lm is None else "given"), check_segments(out.cpu().numpy(), ref, labels, TOL))
        out2 = torch.full((ln * sets,), float("nan"), dtype=torch.float64, device="cuda")
        c.eval_jac_merit_dev(Zd, lam_d, dd, vd, out2)
        torch.cuda.synchronize()
        fused, kernel = c.get_option("last_merit_fused"), c.get_option("last_kernel")
        print("CARRIER %s lam %s: %s (last_kernel %d)" % (name, "delta" if lm is None else "given", "fused" if fused else "separate kernels", kernel))
        # the carrier each case is there for: the pattern-compiled kernel's writer wave (sparse iso generators, d >= 9, m <= 6) leaves the
        # dot products and the finish sums them per set -- six sets for Ptraj6; d = 4, m > 6 and the vector states take the separate kernels
        if name in FUSED_PAYLOAD:
            assert fused == 1 and kernel == 40 + order // 2, (name, fused, kernel)
        else:
            assert fused == 0, (name, fused, kernel)
        show("G", "%s pcl_eval_jac_merit_dev, lam %s" % (name, "delta" if lm is None else "given"), check_segments(out2.cpu().numpy(), ref, labels, TOL))
    c.close()
