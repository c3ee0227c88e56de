"""The exponential-constraint kernels on the device at the generator and column sizes of tests/exp_shape_cases.py (the case table, the branch
each case straddles and the LDS byte counts are there), through _PclContext / the C ABI.  Every value is compared with the committed truths
(scipy expm / expm_frechet / block expm) at TOL = 1e-11, the tolerance the mode already has -- here PER SEGMENT, relative to the segment's own
maximum with no floor at 1 (shape_cases.check_segments): the d/du tails of a short step and the Hessian's scalar entries are held to their own
size, not to the -E block's.  tests/test_exp_shapes_cpu.py shows that the truths are good to 1e-13 on these inputs and that each case sees a
dropped k step, a dropped row tile, a missing squaring, a swapped drive slice and an unwritten -E copy at 1e-7 or more."""

import numpy as np
import pytest
import torch

import exp_hess_truth
import exp_shape_cases as ec
import exp_truth
import piccolo_jl_amd as pa
import var_exp_hess_truth
import var_exp_truth
from shape_cases import check_segments
from test_exp_integrator_gpu import exp_ctx
from test_var_exp_hess_gpu import var_ctx

pytestmark = pytest.mark.gpu
TOL = 1e-11
E_SHAPE = pa._lib.PCL_ESHAPE
PLAIN = list(ec.PLAIN_CASES)
PLAIN_HESS = [c for c in PLAIN if c not in ec.HESS_REFUSED]
NAN = float("nan")


def worst(errs):
    s = max(errs, key=errs.get)
    return "%.1e (%s)" % (errs[s], s)


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float64).reshape(-1)).cuda()  # (a copy: the cases are read-only)


def nan_buf(size):
    return torch.full((size,), NAN, dtype=torch.float64, device="cuda")


def all_paths(c, Zh, kernels):
    """eval_jac_dev into NaN-prefilled outputs; eval_dev, jac_dev, a second launch and the host-pointer calls must give its bits.  Returns
    (delta, values) of the first launch."""
    Zd = dev(Zh)
    dd, vd = nan_buf(c.n_rows), nan_buf(c.jac_nnz)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    c.eval_jac_dev(Zd, dd, vd)
    c.sync()
    assert c.get_option("last_kernel") == kernels[0]
    delta, vals = dd.cpu().numpy(), vd.cpu().numpy()
    d1, v1 = nan_buf(c.n_rows), nan_buf(c.jac_nnz)
    c.eval_dev(Zd, d1)
    c.sync()
    assert c.get_option("last_kernel") == kernels[1]
    c.jac_dev(Zd, v1)
    c.sync()
    assert np.array_equal(d1.cpu().numpy(), delta, equal_nan=True) and np.array_equal(v1.cpu().numpy(), vals, equal_nan=True)
    d2, v2 = nan_buf(c.n_rows), nan_buf(c.jac_nnz)
    c.eval_jac_dev(Zd, d2, v2)
    c.sync()
    assert np.array_equal(d2.cpu().numpy(), delta, equal_nan=True) and np.array_equal(v2.cpu().numpy(), vals, equal_nan=True)
    c.set_stream(None)
    Zf = np.ascontiguousarray(Zh, dtype=np.float64).reshape(-1)
    hd, hv = c.eval_jac(Zf)
    assert np.array_equal(hd, delta, equal_nan=True) and np.array_equal(hv, vals, equal_nan=True)
    assert np.array_equal(c.eval(Zf), delta, equal_nan=True) and np.array_equal(c.jac(Zf), vals, equal_nan=True)
    return delta, vals


def hess_paths(c, Zh, mu, kernel):
    """hess_dev into a NaN-prefilled output; a second launch and the host-pointer call must give its bits."""
    Zd, mud = dev(Zh), dev(mu)
    vd = nan_buf(c.hess_nnz)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    c.hess_dev(Zd, mud, vd)
    c.sync()
    assert c.get_option("last_hess_kernel") == kernel
    vals = vd.cpu().numpy()
    v2 = nan_buf(c.hess_nnz)
    c.hess_dev(Zd, mud, v2)
    c.sync()
    c.set_stream(None)
    assert np.array_equal(v2.cpu().numpy(), vals, equal_nan=True)
    assert np.array_equal(c.hess(np.ascontiguousarray(Zh).reshape(-1), np.asarray(mu)), vals, equal_nan=True)
    return vals


def same_structure(got, want):
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


# ---- plain cases --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PLAIN)
def test_plain_residual_jacobian_rollout(name):
    lay, G0, Gj, Z = ec.plain_case(name)
    d0, v0 = ec.plain_truth(name)
    c = exp_ctx(lay, G0, Gj)
    assert c.jac_per == exp_truth.nnz_per_interval(lay) and c.jac_nnz == v0.size and c.n_rows == d0.size
    want = exp_truth.structure(lay)
    same_structure(c.jac_structure(), want)
    same_structure(c.jac_structure(np.int32), want)
    delta, vals = all_paths(c, Z, (100, 101))
    jl = ec.jac_labels(lay.n, lay.C, lay.m, lay.K)
    ed = check_segments(delta, d0, ec.residual_labels(lay.n, lay.C, lay.K), TOL)
    ev = check_segments(vals, v0, jl, TOL)
    assert np.array_equal(vals[np.char.startswith(jl, "ones")], np.ones(lay.K * lay.x_dim))  # exactly 1.0
    X = c.rollout(Z)[0]
    assert np.array_equal(X[0], Z[0, lay.x_off : lay.x_off + lay.x_dim])  # knot 0 is copied
    er = check_segments(X, ec.plain_rollout_truth(name), ec.rollout_labels(lay.x_dim, lay.N), TOL)
    print("%s: residual %s  Jacobian %s  rollout %s" % (name, worst(ed), worst(ev), worst(er)))
    c.close()


@pytest.mark.parametrize("name", PLAIN_HESS)
def test_plain_hessian(name):
    lay, G0, Gj, Z = ec.plain_case(name)
    mu, h0 = ec.plain_hess_truth(name)
    c = exp_ctx(lay, G0, Gj, exp_hessian=True)
    assert c.get_option("exp_hess") == 1 and c.hess_per == exp_hess_truth.nnz_per_interval(lay) and c.hess_nnz == h0.size
    want = exp_hess_truth.structure(lay)
    same_structure(c.hess_structure(), want)
    same_structure(c.hess_structure(np.int32), want)
    vals = hess_paths(c, Z, mu, 100)
    eh = check_segments(vals, h0, ec.hess_labels(lay.n, lay.C, lay.m, lay.K), TOL)
    print("%s: Hessian %s" % (name, worst(eh)))
    c.close()


def test_p12_hessian_is_refused_with_the_byte_counts_and_the_context_goes_on():
    """n = 63 (LD = 66): five tiles of 33 264 B and the reduction words are 166 448 B > 163 840 B."""
    lay, G0, Gj, Z = ec.plain_case("P12")
    c = exp_ctx(lay, G0, Gj)
    d0, v0 = c.eval_jac(Z)
    with pytest.raises(pa.PclError) as ei:
        c.set_option("exp_hess", 1)
    msg = str(ei.value)
    assert ei.value.code == E_SHAPE and "LDS" in msg and "166448" in msg and "163840" in msg and "33264" in msg, msg
    assert c.get_option("exp_hess") == 0 and c.hess_nnz == 0
    d1, v1 = c.eval_jac(Z)
    assert np.array_equal(d0, d1) and np.array_equal(v0, v1)
    check_segments(v1, ec.plain_truth("P12")[1], ec.jac_labels(lay.n, lay.C, lay.m, lay.K), TOL)
    c.close()
    with pytest.raises(pa.PclError) as ei:
        exp_ctx(lay, G0, Gj, exp_hessian=True)
    assert ei.value.code == E_SHAPE


def test_p4_values_buffer_aligned_to_8_bytes_only():
    """The values through base[1:] of a larger tensor: no 16-byte store is possible, so the -E copies take the scalar store path at an even n.
    The aligned launch's bits, and nothing written before or behind the view."""
    lay, G0, Gj, Z = ec.plain_case("P4")
    c = exp_ctx(lay, G0, Gj)
    Zd = dev(Z)
    dd, vd = nan_buf(c.n_rows), nan_buf(c.jac_nnz)
    base = nan_buf(c.jac_nnz + 2)
    view = base[1:-1]
    assert vd.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 8 and view.is_contiguous()
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    c.eval_jac_dev(Zd, dd, vd)
    d2 = nan_buf(c.n_rows)
    c.eval_jac_dev(Zd, d2, view)
    v3 = nan_buf(c.jac_nnz + 2)
    c.jac_dev(Zd, v3[1:-1])
    c.sync()
    c.set_stream(None)
    vals, b, b3 = vd.cpu().numpy(), base.cpu().numpy(), v3.cpu().numpy()
    assert np.all(np.isfinite(vals))
    assert np.array_equal(b[1:-1], vals) and np.array_equal(b3[1:-1], vals) and np.array_equal(d2.cpu().numpy(), dd.cpu().numpy())
    assert np.isnan(b[0]) and np.isnan(b[-1]) and np.isnan(b3[0]) and np.isnan(b3[-1])
    c.close()


# ---- batched cases ------------------------------------------------------------------------------------------------------------------------------
def batched(which):
    """(layout, context keywords, G0 for the context, Gj, Z of the launch, [(case key)] per member, traj_mode)"""
    if which == "members":  # P4's system, two members with their own drifts on one trajectory
        keys = [("P4", 0, 0), ("P4", 0, 1)]
        lay, _, Gj, Z = ec.plain_case(*keys[0])
        G0 = np.array([ec.plain_case(*k)[1] for k in keys])
        return lay, dict(x_offs=[lay.x_off, lay.x_off], batch=2, per_member_G0=True), G0, Gj, Z, keys, False
    keys = [("P1", 0, 0), ("P1", 1, 0)]  # P1's system, two seeds
    lay, G0, Gj, _ = ec.plain_case(*keys[0])
    Z = np.stack([ec.plain_case(*k)[3] for k in keys])
    return lay, dict(batch=2, batch_mode=pa._lib.PCL_BATCH_TRAJ), G0, Gj, Z, keys, True


@pytest.mark.parametrize("which", ["members", "traj"])
def test_batched(which):
    """Each member's slice against its own truth, per segment; a window on the second member gives the slices of the full launch bitwise."""
    lay, kw, G0, Gj, Z, keys, traj = batched(which)
    c = exp_ctx(lay, G0, Gj, exp_hessian=True, **kw)
    per_d, per_v, per_h = lay.x_dim * lay.K, exp_truth.nnz_per_interval(lay) * lay.K, exp_hess_truth.nnz_per_interval(lay) * lay.K
    assert c.n_rows == 2 * per_d and c.jac_nnz == 2 * per_v and c.hess_nnz == 2 * per_h
    r, cc = c.jac_structure()
    hr, hc = c.hess_structure()
    for b in range(2):
        col0 = b * lay.z_dim * lay.N if traj else 0
        same_structure((r[b * per_v : (b + 1) * per_v], cc[b * per_v : (b + 1) * per_v]), exp_truth.structure(lay, row0=b * per_d, col0=col0))
        same_structure((hr[b * per_h : (b + 1) * per_h], hc[b * per_h : (b + 1) * per_h]), exp_hess_truth.structure(lay, col0=col0))
    delta, vals = all_paths(c, Z, (100, 101))
    mus = [ec.plain_hess_truth(*k)[0] for k in keys]
    hv = hess_paths(c, Z, np.concatenate(mus), 100)
    jl, rl, hl = ec.jac_labels(lay.n, lay.C, lay.m, lay.K), ec.residual_labels(lay.n, lay.C, lay.K), ec.hess_labels(lay.n, lay.C, lay.m, lay.K)
    for b, k in enumerate(keys):
        d0, v0 = ec.plain_truth(*k)
        ed = check_segments(delta[b * per_d : (b + 1) * per_d], d0, rl, TOL)
        ev = check_segments(vals[b * per_v : (b + 1) * per_v], v0, jl, TOL)
        eh = check_segments(hv[b * per_h : (b + 1) * per_h], ec.plain_hess_truth(*k)[1], hl, TOL)
        print("%s member %d: residual %s  Jacobian %s  Hessian %s" % (which, b, worst(ed), worst(ev), worst(eh)))
    c.set_member_window(1, 1)
    wd, wv = c.eval_jac(Z)
    assert np.array_equal(wd, delta[per_d:]) and np.array_equal(wv, vals[per_v:])
    assert np.array_equal(c.hess(Z, mus[1]), hv[per_h:])
    c.set_member_window(0, 2)
    assert np.array_equal(c.eval(Z), delta)
    c.close()


# ---- variational cases --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ec.VAR_CASES))
def test_variational_residual_jacobian(name):
    case = ec.var_case(name)
    d0, v0 = ec.var_truth(name)
    c = var_ctx(case)
    assert c.jac_per == var_exp_truth.nnz_per_interval(case) and c.jac_nnz == v0.size and c.n_rows == d0.size
    want = var_exp_truth.structure(case)
    same_structure(c.jac_structure(), want)
    same_structure(c.jac_structure(np.int32), want)
    delta, vals = all_paths(c, case.Z, (110, 111))  # (the residual-only launch has the fused launch's bits)
    jl = ec.jac_labels(case.n, case.C, case.m, case.K, case.v)
    ed = check_segments(delta, d0, ec.residual_labels(case.n, case.C, case.K, case.v), TOL)
    ev = check_segments(vals, v0, jl, TOL)
    assert np.array_equal(vals[np.char.startswith(jl, "ones")], np.ones(case.K * case.xd))
    print("%s: residual %s  Jacobian %s" % (name, worst(ed), worst(ev)))
    c.close()


def var_hess_ctx(case, tiles):
    c = var_ctx(case)
    c.set_option("var_exp_hess_tiles", tiles)
    c.set_option("var_exp_hess", 1)
    return c


@pytest.mark.parametrize("name, tiles, kernel", [(n, 0, 110) for n in ec.VAR_HESS_LDS] + [(n, 1, 112) for n in ec.VAR_HESS_WS])
def test_variational_hessian(name, tiles, kernel):
    """V1, V2, V3: nine LDS tiles.  V4, V6: var_exp_hess_tiles = 1 serves what nine tiles exceed."""
    case = ec.var_case(name)
    mu, h0 = ec.var_hess_truth(name)
    c = var_hess_ctx(case, tiles)
    assert c.hess_per == var_exp_hess_truth.nnz_per_interval(case) and c.hess_nnz == h0.size
    want = var_exp_hess_truth.structure(case)
    same_structure(c.hess_structure(), want)
    same_structure(c.hess_structure(np.int32), want)
    vals = hess_paths(c, case.Z, mu, kernel)
    eh = check_segments(vals, h0, ec.hess_labels(case.n, case.C, case.m, case.K, case.v), TOL)
    print("%s: Hessian %s" % (name, worst(eh)))
    c.close()


@pytest.mark.parametrize("name", ["V1", "V2"])
def test_variational_hessian_workspace_plan_has_the_lds_plan_bits(name):
    case = ec.var_case(name)
    mu = ec.var_hess_truth(name)[0]
    a, b = var_hess_ctx(case, 0), var_hess_ctx(case, 2)
    va, vb = hess_paths(a, case.Z, mu, 110), hess_paths(b, case.Z, mu, 112)
    assert np.all(np.isfinite(va)) and np.array_equal(va, vb)
    a.close()
    b.close()


@pytest.mark.parametrize("name", ["V1", "V2"])
def test_variational_rollout(name):
    """With var_full: the stacked rollout against the product of expm of the lifted generator, per knot; knot 0 is copied."""
    case = ec.var_case(name)
    c = var_ctx(case)
    c.set_option("var_full", 1)
    X = c.rollout(case.Z.reshape(-1))[0]
    assert np.array_equal(X[0], np.concatenate([case.Z[0, o : o + case.xdc] for o in case.xo]))
    er = check_segments(X, ec.var_rollout_truth(name), ec.rollout_labels(case.xd, case.N), TOL)
    print("%s: rollout %s" % (name, worst(er)))
    c.close()
