"""GPU tests of the Pade variational kernels (batch_mode PCL_BATCH_VARIATIONAL) over the cases of tests/variational_shape_cases.py: the sizes
at which pcl_var_fused_kernel's block role changes its pair slot (n = 32, 34, 44, 46, 56, 64), dense and padded ELL tables in its column role, and
every wave count of pcl_var_hess_kernel with the refusal boundary (W7: served at order 8, refused at order 10).  Every case at orders 2 - 10:

    values          eval_jac is kernel 70; delta and every Jacobian segment (row component x variable kind x relative knot x interval) within
                    1e-11 of the longdouble truth, relative to the segment's own size; the emitted positions unique and those of the truth
    pointer paths   pcl_eval (71), pcl_jac_dev without delta, host pointers and device pointers: the same bits
    work splits     order 10: var_block_wgs in {1, 2, C} x var_col_wgs in {1, 3, C}: the same bits
    compact         orders 4, 10: the compact launch (72) expanded at cols_per_slice 0, 1, 2, C into NaN-prefilled arrays: the full launch's bits
    Hessian         where the restated plan serves it: kernel 70, every segment within 1e-11, lower-triangular unique positions of the truth,
                    two launches and both pointer paths the same bits
    W7, order 10    PCL_ESHAPE naming the LDS and 190728 bytes; eval_jac afterwards returns the earlier bits

Segments whose truth is identically zero (W2's Delta t = 0 interval: the L blocks, the d/du tails) must be zeros."""
import numpy as np
import pytest
import torch

import piccolo_jl_amd as pa
import variational_shape_cases as W
from var_compact_cases import same_bits

pytestmark = pytest.mark.gpu
TOL = 1e-11
VAR = pa._lib.PCL_BATCH_VARIATIONAL
NAMES = list(W.CASES)
ALL = [(nm, o) for nm in NAMES for o in W.ORDERS]
IDS = ["%s-%d" % p for p in ALL]
_worst = {}


def served(name, order):
    n, C, v, m = W.shape(name)
    return W.hess_plan(n, C, m, v, order)["served"]


def make_ctx(name, order, **kw):
    cs, _ = W.case(name)
    return pa.integrators._PclContext(d=cs.n // 2, m=cs.m, N=cs.N, z_dim=cs.z_dim, u_off=cs.u_off, dt_off=cs.dt_off, x_offs=cs.xo,
                                      G0=np.concatenate([cs.G0[None], np.array(cs.Gv)]), Gj=cs.Gj, batch=1 + cs.v, batch_mode=VAR,
                                      per_member_G0=True, pade_order=order, state_cols=cs.C, **kw)  # fmt: skip


def nan_host(n):
    return np.full(n, np.nan)


def nan_dev(n):
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


def host(t):
    return t.cpu().numpy()


def note(kind, name, order, worst):
    if worst[0] >= _worst.get(kind, (-1.0,))[0]:
        _worst[kind] = (worst[0], worst[1], name, order)
    print("%s order %d: worst %s segment %.2e (%s) | worst so far: %s" % (
        name, order, kind, worst[0], worst[1], "  ".join("%s %.2e (%s, %s, order %d)" % ((k,) + v) for k, v in sorted(_worst.items()))))  # fmt: skip


def check_delta(name, order, delta):
    cs, _ = W.case(name)
    st = W.structure(name)
    assert np.isfinite(delta).all()
    e = W.segment_errors(st["dcode"], delta, W.truth(name, order)[0])
    note("delta", name, order, W.assert_segments(e, TOL, lambda s: W.residual_name(cs, s), "%s order %d, delta" % (name, order)))


def check_jac(c, name, order, vals):
    cs, _ = W.case(name)
    st = W.structure(name)
    assert np.isfinite(vals).all()
    rows, cols = c.jac_structure()
    P = rows * st["ncols"] + cols
    i, ok = W.lookup(st["jkey"], P)
    assert ok.all() and len(np.unique(P)) == len(P)  # positions of the truth's structure, each once
    assert st["jstruct"][i].all() and len(P) == int(st["jstruct"].sum())  # ... and every one that can hold a value
    j = W.truth(name, order)[1]
    e = W.segment_errors(st["jcode"][i], vals, j[i], st["jcode"], j)
    note("Jacobian", name, order, W.assert_segments(e, TOL, lambda s: W.jac_name(cs, s), "%s order %d, Jacobian" % (name, order)))


def check_hess(c, name, order, hv):
    cs, _ = W.case(name)
    st = W.structure(name)
    assert np.isfinite(hv).all()
    hr, hc = c.hess_structure()
    assert np.all(hr >= hc)
    P = hr * st["ncols"] + hc
    i, ok = W.lookup(st["hkey"], P)
    assert ok.all() and len(np.unique(P)) == len(P) == len(st["hkey"])
    h = W.truth(name, order)[2]
    e = W.segment_errors(st["hcode"][i], hv, h[i], st["hcode"], h)
    note("Hessian", name, order, W.assert_segments(e, TOL, lambda s: W.hess_name(cs, s), "%s order %d, Hessian" % (name, order)))


# ---- values and pointer paths -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, order", ALL, ids=IDS)
def test_values_and_pointer_paths(name, order):
    cs, _ = W.case(name)
    Z = cs.Z.reshape(-1).copy()
    c = make_ctx(name, order)
    assert c.get_option("variations") == cs.v
    delta, vals = c.eval_jac(Z, nan_host(c.n_rows), nan_host(c.jac_nnz))
    assert c.get_option("last_kernel") == 70
    check_delta(name, order, delta)
    check_jac(c, name, order, vals)
    # the residual alone, the Jacobian alone, host and device pointers
    assert same_bits(c.eval(Z, nan_host(c.n_rows)), delta) and c.get_option("last_kernel") == 71
    assert same_bits(c.jac(Z, nan_host(c.jac_nnz)), vals) and c.get_option("last_kernel") == 70
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    Zd = torch.from_numpy(Z).cuda()
    dd, vd, v1, d1 = nan_dev(c.n_rows), nan_dev(c.jac_nnz), nan_dev(c.jac_nnz), nan_dev(c.n_rows)
    c.eval_jac_dev(Zd, dd, vd)
    assert c.get_option("last_kernel") == 70
    c.jac_dev(Zd, v1)
    c.eval_dev(Zd, d1)
    assert c.get_option("last_kernel") == 71
    c.sync()
    assert same_bits(host(dd), delta) and same_bits(host(vd), vals) and same_bits(host(v1), vals) and same_bits(host(d1), delta)
    c.set_stream(None)
    c.close()


# ---- work splits --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_every_work_split_gives_the_same_bits(name):
    cs, _ = W.case(name)
    Z = cs.Z.reshape(-1).copy()
    c = make_ctx(name, 10)
    d0, v0 = c.eval_jac(Z, nan_host(c.n_rows), nan_host(c.jac_nnz))
    check_jac(c, name, 10, v0)
    for nb in (1, 2, cs.C):
        for ncw in (1, 3, cs.C):
            assert (W.split_blocks(cs.C, nb), W.split_cols(cs.C, ncw)[0]) == (min(nb, cs.C), min(ncw, cs.C))
            c.set_option("var_block_wgs", nb)
            c.set_option("var_col_wgs", ncw)
            d1, v1 = c.eval_jac(Z, nan_host(c.n_rows), nan_host(c.jac_nnz))
            assert c.get_option("last_kernel") == 70
            assert same_bits(d1, d0) and same_bits(v1, v0), (nb, ncw)
            assert same_bits(c.eval(Z, nan_host(c.n_rows)), d0), (nb, ncw)
    c.close()


# ---- the compact Jacobian ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, order", [(nm, o) for nm in NAMES for o in (4, 10)], ids=["%s-%d" % (nm, o) for nm in NAMES for o in (4, 10)])
def test_compact_launch_expands_to_the_full_launch(name, order):
    cs, _ = W.case(name)
    c = make_ctx(name, order, var_compact=True)
    assert c.get_option("var_compact") == 1
    n, C, v, m = W.shape(name)
    assert c.compact_per == (2 + 2 * v) * n * n + cs.xd * (m + 1) and c.compact_nnz == cs.K * c.compact_per
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    Zd = torch.from_numpy(cs.Z.reshape(-1).copy()).cuda()
    d_full, v_full, d_comp, v_comp = nan_dev(c.n_rows), nan_dev(c.jac_nnz), nan_dev(c.n_rows), nan_dev(c.compact_nnz)
    c.eval_jac_dev(Zd, d_full, v_full)
    assert c.get_option("last_kernel") == 70
    c.eval_jac_compact_dev(Zd, d_comp, v_comp)
    assert c.get_option("last_kernel") == 72
    c.sync()
    full = host(v_full)
    check_delta(name, order, host(d_full))
    check_jac(c, name, order, full)
    assert same_bits(host(d_comp), host(d_full)) and not np.isnan(host(v_comp)).any()
    for cps in (0, 1, 2, C):
        c.set_option("cols_per_slice", cps)
        out = nan_dev(c.jac_nnz)
        c.jac_expand_dev(v_comp, out)
        c.sync()
        assert same_bits(host(out), full), cps
    c.set_stream(None)
    c.close()


# ---- the Hessian of the Lagrangian ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, order", [p for p in ALL if served(*p)], ids=["%s-%d" % p for p in ALL if served(*p)])
def test_hessian(name, order):
    cs, _ = W.case(name)
    Z, mu = cs.Z.reshape(-1).copy(), np.array(W.rand_mu(name))
    c = make_ctx(name, order)
    hv = c.hess(Z, mu, nan_host(c.hess_nnz))
    assert c.get_option("last_hess_kernel") == 70
    check_hess(c, name, order, hv)
    assert same_bits(c.hess(Z, mu, nan_host(c.hess_nnz)), hv)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    hd = nan_dev(c.hess_nnz)
    c.hess_dev(torch.from_numpy(Z).cuda(), torch.from_numpy(mu).cuda(), hd)
    c.sync()
    assert same_bits(host(hd), hv)
    c.set_stream(None)
    c.close()


def test_w7_hessian_is_refused_at_order_10_exactly_as_planned():
    n, C, v, m = W.shape("W7")
    plan = W.hess_plan(n, C, m, v, 10)
    assert not plan["served"] and plan["bytes"] == 190728
    cs, _ = W.case("W7")
    Z, mu = cs.Z.reshape(-1).copy(), np.array(W.rand_mu("W7"))
    c = make_ctx("W7", 10)
    d0, v0 = c.eval_jac(Z, nan_host(c.n_rows), nan_host(c.jac_nnz))
    check_jac(c, "W7", 10, v0)
    with pytest.raises(pa.PclError) as ei:
        c.hess(Z, mu)
    assert ei.value.code == pa._lib.PCL_ESHAPE and "LDS" in str(ei.value) and "190728" in str(ei.value), str(ei.value)
    d1, v1 = c.eval_jac(Z, nan_host(c.n_rows), nan_host(c.jac_nnz))
    assert c.get_option("last_kernel") == 70 and same_bits(d1, d0) and same_bits(v1, v0)
    c.close()
    # the same system one order lower: served, with one wave
    assert W.hess_plan(n, C, m, v, 8)["served"] and W.hess_plan(n, C, m, v, 8)["w"] == 1
    c = make_ctx("W7", 8)
    hv = c.hess(Z, mu, nan_host(c.hess_nnz))
    assert c.get_option("last_hess_kernel") == 70
    check_hess(c, "W7", 8, hv)
    c.close()
