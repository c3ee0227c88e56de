"""GPU tests of kernel 4's ONE-ITEM module (option v4_one_item; pcl_kernel_fused_sparse.hpp, SP4_ONE_ITEM): the fused kernel of launches in which
every workgroup has exactly one item, compiled with the launch's shape folded in as constants.  Every case runs the same inputs on one context
through the general module (v4_one_item 0) and through the one-item module (1); residual and every Jacobian value must have the same BITS
(torch.equal on the device: no tolerance).  The shapes are the smallest that reach every branch the module keeps: the three branches of `decode`
(S == 1, S == 2 with the balanced hand-over of the middle column's B- block, the general one), b > 0, `borrow` and `pingpong`, and the headline's
own launch (config 3, N = 100, order 4: two wide slices per interval).  Launches the module does not serve must not take it.
(The launch sizes assume what the library assumes: at most one workgroup per CU, so the cases need the 198 .. 234 CUs they ask for.)"""
import numpy as np
import pytest

import piccolo_jl_amd as pa
from oracle import pade_oracle as po
from piccolo_jl_amd import synthetic
from shape_cases import plain_case

pytestmark = pytest.mark.gpu
ESHAPE = pa._lib.PCL_ESHAPE


def make_ctx(lay, G0, Gj, order, batch=1):
    c = pa.integrators._PclContext(d=lay.d, m=lay.m, N=lay.N, z_dim=lay.z_dim, u_off=lay.u_off, dt_off=lay.dt_off, x_offs=[lay.x_off], G0=G0, Gj=Gj,
                                   batch=batch, batch_mode=pa._lib.PCL_BATCH_TRAJ if batch > 1 else pa._lib.PCL_BATCH_MEMBERS, pade_order=order)  # fmt: skip
    c.set_option("require_jit", 1)  # a module that cannot be built is an error, not a fallback
    return c


def run(c, Zd, one_item):
    """(residual, values) of one eval_jac_dev under v4_one_item = one_item, outputs NaN beforehand, and what the launch ran."""
    import torch

    c.set_option("v4_one_item", one_item)
    dd = torch.full((c.n_rows,), float("nan"), dtype=torch.float64, device="cuda")
    vd = torch.full((c.jac_nnz,), float("nan"), dtype=torch.float64, device="cuda")
    c.eval_jac_dev(Zd, dd, vd)
    c.sync()
    return dd, vd, c.get_option("last_kernel"), c.get_option("last_v4_one_item")


def both_modules(c, Z, order):
    import torch

    c.set_stream(torch.cuda.current_stream().cuda_stream)
    Zd = torch.from_numpy(np.array(Z, dtype=np.float64).reshape(-1)).cuda()
    d0, v0, k0, o0 = run(c, Zd, 0)
    d1, v1, k1, o1 = run(c, Zd, 1)
    assert k0 == k1 == 40 + order // 2 and (o0, o1) == (0, 1), (k0, k1, o0, o1)
    assert not torch.isnan(d0).any() and not torch.isnan(v0).any()
    assert torch.equal(d1, d0) and torch.equal(v1, v0)
    da, va, ka, oa = run(c, Zd, -1)  # auto: the module wherever it serves
    assert oa == 1 and torch.equal(da, d0) and torch.equal(va, v0)
    return d0, v0


_CONFIG3 = {}


def config3(N, seeds=(3,)):
    """Config 3's system (d = 27, m = 6) and near-feasible trajectories of N knots, computed once per (N, seeds) and never written to."""
    key = (N, tuple(seeds))
    if key not in _CONFIG3:
        so = po.config_system(3)
        Zs, lay = [], None
        for s in seeds:
            Z, lay = po.synthetic_trajectory(so, N, seed=s)
            Z[:, lay.dt_off] = 0.08 + 0.04 * np.random.default_rng(s).random(N)  # (steps that differ from interval to interval)
            Z.setflags(write=False)
            Zs.append(Z)
        system = synthetic.config_system(3)
        _CONFIG3[key] = (lay, system.G_drift, system.G_drives_array(), Zs)
    return _CONFIG3[key]


# ---- d = 9 (S1: the smallest system kernel 4 serves, odd d): every branch of decode ---------------------------------------------------------
@pytest.mark.parametrize("order", [2, 4, 6, 8, 10])
@pytest.mark.parametrize("N", [100, 200, 4])
def test_d9_every_split(N, order):
    """N = 100: two slices per interval of 5 and 4 columns (S == 2, the middle column's B- block handed over) | 200: one slice per interval
    (S == 1) | 4: nine slices of one column (the general branch)."""
    lay, G0, Gj, Z = plain_case("S1", N=N)
    c = make_ctx(lay, G0, Gj, order)
    both_modules(c, Z, order)
    c.close()


@pytest.mark.parametrize("order", [2, 4, 6, 8, 10])
def test_d9_two_trajectories(order):
    """Two trajectories of 40 knots in one launch: 78 intervals in three slices each, one item per workgroup, b > 0 in half of them."""
    lay, G0, Gj, Z0 = plain_case("S1", N=40, seed=0)
    Z1 = plain_case("S1", N=40, seed=1)[3]
    c = make_ctx(lay, G0, Gj, order, batch=2)
    both_modules(c, np.stack([Z0, Z1]), order)
    c.close()


# ---- config 3 (d = 27, m = 6) --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [4, 8, 10])
def test_config3_one_column_per_item(order):
    """N = 5: 27 slices of one column per interval.  Orders 8 and 10 have three power tiles for q = 4, 5 powers (`borrow`: the others stand in
    the chains' dW tiles) and run W through two tiles (`pingpong`, q >= 4)."""
    lay, G0, Gj, (Z,) = config3(5)
    c = make_ctx(lay, G0, Gj, order)
    d0, v0 = both_modules(c, Z, order)
    # (the values themselves, once per order: the oracle at 1e-12 as in the parity tests)
    so = po.config_system(3)
    j_ref = po.pade_jacobian_values(Z, lay, so.G_drift, np.array(so.G_drives), order).reshape(-1)
    assert np.abs(v0.cpu().numpy() - j_ref).max() <= 1e-12 * max(1.0, np.abs(j_ref).max())
    c.close()


def test_config3_headline_launch():
    """The headline's own launch: one trajectory of 100 knots at order 4, 198 workgroups, slices of 14 and 13 columns -- the only size at which
    both slices of an interval are wide."""
    lay, G0, Gj, (Z,) = config3(100)
    c = make_ctx(lay, G0, Gj, 4)
    both_modules(c, Z, 4)
    c.close()


# ---- launches the module does not serve -----------------------------------------------------------------------------------------------------
def test_several_items_per_workgroup_take_the_general_module():
    """8 trajectories of config 3 at N = 100: several items per workgroup.  auto runs what v4_one_item = 0 runs; requiring the module is refused
    before any launch."""
    import torch

    lay, G0, Gj, Zs = config3(100, seeds=tuple(range(8)))
    c = make_ctx(lay, G0, Gj, 4, batch=8)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    Zd = torch.from_numpy(np.stack(Zs).reshape(-1)).cuda()
    d0, v0, k0, o0 = run(c, Zd, 0)
    da, va, ka, oa = run(c, Zd, -1)
    assert k0 == ka == 42 and (o0, oa) == (0, 0)
    assert not torch.isnan(v0).any() and torch.equal(da, d0) and torch.equal(va, v0)
    c.set_option("v4_one_item", 1)
    with pytest.raises(pa.PclError) as ei:
        c.eval_jac_dev(Zd, da, va)
    assert ei.value.code == ESHAPE and "v4_one_item" in str(ei.value), str(ei.value)
    c.set_option("v4_one_item", -1)
    c.eval_jac_dev(Zd, da, va)  # (nothing launched: the context goes on)
    c.sync()
    assert torch.equal(va, v0)
    c.close()


def test_compact_merit_and_flag_launches_take_the_general_module():
    """One trajectory of config 3 at N = 5 (a launch the module serves as a plain eval_jac_dev): the compact launch, the payload-fused call and a
    context with v4_flags = 8 run the general module under auto, with the bits v4_one_item = 0 gives."""
    import torch

    lay, G0, Gj, (Z,) = config3(5)
    c = make_ctx(lay, G0, Gj, 4)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    Zd = torch.from_numpy(np.array(Z, dtype=np.float64).reshape(-1)).cuda()
    ln, _ = c.merit_grad_len()
    nan = lambda k: torch.full((k,), float("nan"), dtype=torch.float64, device="cuda")

    def compact():
        dd, cc = nan(c.n_rows), nan(c.compact_nnz)
        c.eval_jac_compact_dev(Zd, dd, cc)
        return dd, cc

    def merit():
        dd, vd, pay = nan(c.n_rows), nan(c.jac_nnz), nan(ln)
        c.eval_jac_merit_dev(Zd, None, dd, vd, pay)
        return dd, vd, pay

    def flagged():
        dd, vd = nan(c.n_rows), nan(c.jac_nnz)
        c.eval_jac_dev(Zd, dd, vd)
        return dd, vd

    plain = run(c, Zd, 0)
    for call, flags in ((compact, 0), (merit, 0), (flagged, 8)):
        c.set_option("v4_flags", flags)
        res = []
        for one_item in (0, -1):
            c.set_option("v4_one_item", one_item)
            out = call()
            c.sync()
            assert c.get_option("last_kernel") == 42 and c.get_option("last_v4_one_item") == 0, (call.__name__, one_item)
            res.append(out)
        for a, b in zip(*res):
            assert not torch.isnan(a).any() and torch.equal(a, b), call.__name__
        if call is not compact:  # ... and they are the plain launch's residual and values
            assert torch.equal(res[0][0], plain[0]) and torch.equal(res[0][1], plain[1]), call.__name__
    c.set_option("v4_flags", 0)
    assert run(c, Zd, -1)[3] == 1  # (the same context takes the module again)
    c.close()
