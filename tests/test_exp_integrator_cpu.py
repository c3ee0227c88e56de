"""The exponential mode (pcl_desc.pade_order = PCL_ORDER_EXP) without a device: the constant in the header and the mirror, the descriptor
validation of pcl_create, and the truth helper of the GPU tests (tests/exp_truth.py) against central differences of the oracle's residual."""
import ctypes
import os
import re

import numpy as np
import pytest

import exp_truth
import piccolo_jl_amd as pa
from oracle import pade_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return pa._lib.load()


def test_constant_in_header_and_mirror():
    with open(os.path.join(ROOT, "include", "piccolo_hip.h")) as f:
        header = f.read()
    mt = re.search(r"^#define\s+PCL_ORDER_EXP\s+\((-?\d+)\)", header, re.M)
    assert mt and int(mt.group(1)) == -1
    assert pa._lib.PCL_ORDER_EXP == -1
    assert pa._lib.order_code("exp") == pa._lib.PCL_ORDER_EXP == pa._lib.order_code(-1)
    assert pa._lib.order_code(0) == 0 and pa._lib.order_code(8) == 8
    with pytest.raises(ValueError):
        pa._lib.order_code("exponential-ish")


def _create(lib, **over):
    d, m, N = 2, 2, 5
    n, xd = 2 * d, 2 * d * d
    kw = dict(d=d, n_drives=m, N=N, z_dim=xd + 2 + m, u_off=xd + 2, dt_off=xd, batch=1, batch_mode=pa._lib.PCL_BATCH_MEMBERS, pade_order=4,
              device_id=0, index_base=0, per_member_G0=0, state_cols=d, global_dim=0)  # fmt: skip
    x_offs = over.pop("x_offs", [0])
    kw.update(over)
    G0 = np.zeros(n * n * max(kw["batch"], 1))
    Gj = np.zeros(n * n * m)
    xo = np.array(x_offs, dtype=np.int32)
    D = pa._lib.pcl_desc(struct_size=ctypes.sizeof(pa._lib.pcl_desc), G0=G0.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                         Gj=Gj.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), x_offs=xo.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), **kw)  # fmt: skip
    h = ctypes.c_void_p()
    rc = lib.pcl_create(ctypes.byref(D), ctypes.byref(h))
    msg = lib.pcl_last_error(None).decode()
    if rc == 0:
        lib.pcl_destroy(h)
    return rc, msg


def test_exponential_with_variational_is_refused_before_any_device_call(lib):
    """PCL_ENOTIMPL also on a box without a device, where a descriptor that passes validation ends in PCL_EHIP."""
    xd = 8
    rc, msg = _create(lib, pade_order=pa._lib.PCL_ORDER_EXP, batch_mode=pa._lib.PCL_BATCH_VARIATIONAL, batch=2, per_member_G0=1, x_offs=[0, xd],
                      z_dim=2 * xd + 4, u_off=2 * xd + 2, dt_off=2 * xd)  # fmt: skip
    assert rc == pa._lib.PCL_ENOTIMPL, (rc, msg)
    assert "pade_order" in msg and "batch_mode" in msg and "PCL_ORDER_EXP" in msg and "PCL_BATCH_VARIATIONAL" in msg


def test_orders_below_the_exponential_are_refused_before_any_device_call(lib):
    for order in (-2, -7):
        rc, msg = _create(lib, pade_order=order)
        assert rc == pa._lib.PCL_ENOTIMPL, (rc, msg)
        assert "PCL_ORDER_EXP" in msg and "pade_order=%d" % order in msg
    rc, msg = _create(lib, pade_order=3)  # the odd orders keep their message
    assert rc == pa._lib.PCL_ENOTIMPL and "diagonal Pade orders 2, 4, 6, 8, 10 are implemented" in msg


def test_exponential_descriptor_passes_validation(lib):
    import torch

    rc, msg = _create(lib, pade_order=pa._lib.PCL_ORDER_EXP)
    if torch.cuda.is_available():
        assert rc == pa._lib.PCL_OK, (rc, msg)
    else:  # past validation: only the missing device stops it
        assert rc == pa._lib.PCL_EHIP, (rc, msg)


def test_truth_helper_against_central_differences():
    """exp_truth.dense (the oracle's values in the library's layout, through the expected structure) equals central differences of
    po.exp_residual: config 2's system, N = 4, step 1e-6, 1e-7 relative -- every entry of the (x_dim K) x (z_dim N) matrix."""
    so = po.config_system(2)
    Z, lay = po.synthetic_trajectory(so, 4, seed=3)
    Z[:, lay.dt_off] = 0.1 + 0.05 * np.random.default_rng(0).random(lay.N)
    G0, Gj = so.G_drift, np.array(so.G_drives)
    J = exp_truth.dense(Z, lay, G0, Gj)
    assert J.shape == (lay.x_dim * lay.K, lay.z_dim * lay.N)
    step = 1e-6
    F = np.empty_like(J)
    for col in range(J.shape[1]):
        zp, zm = Z.reshape(-1).copy(), Z.reshape(-1).copy()
        zp[col] += step
        zm[col] -= step
        F[:, col] = (po.exp_residual(zp.reshape(Z.shape), lay, G0, Gj) - po.exp_residual(zm.reshape(Z.shape), lay, G0, Gj)).reshape(-1) / (2 * step)
    err = np.abs(J - F).max()
    assert err <= 1e-7 * max(1.0, np.abs(F).max()), err
    # the structure names every position once, and nothing outside it moves the residual
    r, c = exp_truth.structure(lay)
    assert len(r) == lay.K * exp_truth.nnz_per_interval(lay) == len(set(zip(r.tolist(), c.tolist())))
    mask = np.zeros_like(J, dtype=bool)
    mask[r, c] = True
    assert np.abs(F[~mask]).max() <= 1e-7
