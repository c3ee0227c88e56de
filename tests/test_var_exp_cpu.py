"""The variational integrators on the exponential constraint (batch_mode PCL_BATCH_VARIATIONAL_EXP) without a device: the constant, the
descriptor validation, the truth helper of the GPU tests (tests/var_exp_truth.py) against central differences of its own residual, the
structure, and a numpy restatement of exactly the kernel's recurrence (scaling, Taylor degree 14, squarings) against that truth."""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest

import piccolo_jl_amd as pa
import var_exp_cases as cases
import var_exp_truth as truth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (name, builder): the reference's Pauli item (ket and unitary), config 2 with v = 2, config 3 with v = 1 at dt = 0.1 and dt = 1
# (config 3: two knots, one interval -- 5 848 columns of central differences each)
CASES = [
    ("pauli_ket", lambda: cases.pauli(True)[3]),
    ("pauli_unitary", lambda: cases.pauli(False)[3]),
    ("config2_v2", lambda: cases.config2(2)[3]),
    ("config3_v1_dt0.1", lambda: cases.config3(1, N=2)[3]),
    ("config3_v1_dt1", lambda: cases.config3(1, N=2, dt=1.0)[3]),
]
_memo = {}


def case_of(name):
    if name not in _memo:
        _memo[name] = dict(CASES)[name]()
    return _memo[name]


@pytest.fixture(scope="module")
def lib():
    return pa._lib.load()


def test_constant_in_header_and_mirror():
    with open(os.path.join(ROOT, "include", "piccolo_hip.h")) as f:
        header = f.read()
    mt = re.search(r"^#define\s+PCL_BATCH_VARIATIONAL_EXP\s+(\d+)", header, re.M)
    assert mt and int(mt.group(1)) == 3
    assert pa._lib.PCL_BATCH_VARIATIONAL_EXP == 3


def _create(lib, **over):
    d, m, N = 2, 2, 5
    n, xd = 2 * d, 2 * d * d
    kw = dict(d=d, n_drives=m, N=N, z_dim=2 * xd + 2 + m, u_off=2 * xd + 2, dt_off=2 * xd, batch=2, batch_mode=pa._lib.PCL_BATCH_VARIATIONAL_EXP,
              pade_order=pa._lib.PCL_ORDER_EXP, device_id=0, index_base=0, per_member_G0=1, state_cols=d, global_dim=0)  # fmt: skip
    kw.update(over)
    G0 = np.zeros(n * n * 2)
    Gj = np.zeros(n * n * m)
    xo = np.array([0, xd], dtype=np.int32)
    D = pa._lib.pcl_desc(struct_size=ctypes.sizeof(pa._lib.pcl_desc), G0=G0.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                         Gj=Gj.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), x_offs=xo.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), **kw)  # fmt: skip
    h = ctypes.c_void_p()
    rc = lib.pcl_create(ctypes.byref(D), ctypes.byref(h))
    msg = lib.pcl_last_error(None).decode()
    if rc == 0:
        lib.pcl_destroy(h)
    return rc, msg


@pytest.mark.parametrize("order", [4, 0, 10])
def test_pade_order_with_the_mode_is_refused_before_any_device_call(lib, order):
    """PCL_EINVAL also on a box without a device, where a descriptor that passes validation ends in PCL_EHIP."""
    rc, msg = _create(lib, pade_order=order)
    assert rc == pa._lib.PCL_EINVAL, (rc, msg)
    assert "pade_order" in msg and "batch_mode" in msg and "PCL_BATCH_VARIATIONAL_EXP" in msg and "PCL_ORDER_EXP" in msg


def test_descriptor_passes_validation_and_the_old_pair_keeps_its_refusal(lib):
    import torch

    rc, msg = _create(lib)
    assert rc == (pa._lib.PCL_OK if torch.cuda.is_available() else pa._lib.PCL_EHIP), (rc, msg)
    rc, msg = _create(lib, batch_mode=pa._lib.PCL_BATCH_VARIATIONAL)
    assert rc == pa._lib.PCL_ENOTIMPL and "is not implemented" in msg and "PCL_BATCH_VARIATIONAL_EXP" in msg
    rc, msg = _create(lib, batch_mode=7)
    assert rc == pa._lib.PCL_EINVAL and "batch_mode" in msg
    rc, msg = _create(lib, batch=1)  # the conventions of PCL_BATCH_VARIATIONAL hold
    assert rc == pa._lib.PCL_EINVAL and "batch" in msg


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_structure_count_and_no_duplicates(name):
    case = case_of(name)
    r, c = truth.structure(case)
    per = (1 + 2 * case.v) * case.C * case.n**2 + case.xd * (case.m + 2)
    assert truth.nnz_per_interval(case) == per and len(r) == case.K * per
    assert len(np.unique(r * (case.N * case.z_dim) + c)) == len(r)
    r1, c1 = truth.structure(case, index_base=1)
    assert np.array_equal(r1, r + 1) and np.array_equal(c1, c + 1)


# Worst deviations measured here, |J - fd|_max / max(1, |J|_max): 5.9e-11 (pauli_ket), 9.2e-11 (pauli_unitary), 1.7e-10 (config2_v2: 2.1e-10 over
# 1.26), 5.9e-11 (config3_v1_dt0.1: 2.1e-10 over 3.6), 1.6e-10 (config3_v1_dt1: 4.4e-9 over 27.5) -- the rounding of a central difference with
# step 1e-6 (the residual is linear in the states, so there it is rounding alone).  The bound is 10 x the worst of them, 1.7e-10.
FD_BOUND = 1.7e-9


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_truth_jacobian_against_central_differences(name):
    """Every entry of the truth's Jacobian, and nothing outside the library's structure: column by column, step 1e-6."""
    case = case_of(name)
    J = truth.jacobian(case).tocsc()
    r, c = truth.structure(case)
    vals = truth.values(case, J.tocsr())  # (asserts that the lifted problem has nothing outside the structure)
    assert len(vals) == len(r)
    scale = max(1.0, np.abs(vals).max())
    step, worst = 1e-6, 0.0
    z0 = case.Z.reshape(-1)
    with truth.cached_expm():
        for col in range(J.shape[1]):
            zp, zm = z0.copy(), z0.copy()
            zp[col] += step
            zm[col] -= step
            f = (truth.residual(cases.with_Z(case, zp.reshape(case.Z.shape))) - truth.residual(cases.with_Z(case, zm.reshape(case.Z.shape)))) / (2 * step)
            worst = max(worst, np.abs(f - J[:, col].toarray().reshape(-1)).max())
    print("%s: worst |J - fd| = %.3e (scale %.3e)" % (name, worst, scale))
    assert worst <= FD_BOUND * scale, worst


# ---- the kernel's recurrence, restated in numpy ----------------------------------------------------------------------------------------------
def recurrence(case):
    """(delta, values) by pcl_var_exp_kernel's arithmetic: theta = |h| |G|_1 halved to <= 1/4, Horner of degree 14 on the quadruple
    (T, Tp, Tq, Tw), s squarings, then the products of the last phase -- in the library's value order."""
    n, C, v, m, xdc, xd = case.n, case.C, case.v, case.m, case.xdc, case.xd
    I = np.eye(n)
    per = truth.nnz_per_interval(case)
    delta, vals = np.empty((case.K, xd)), np.empty((case.K, per))
    seg1 = (1 + 2 * v) * C * n * n
    for k in range(case.K):
        z, zn = case.Z[k], case.Z[k + 1]
        h = z[case.dt_off]
        G = case.G0.copy()
        for l in range(m):
            G = G + z[case.u_off + l] * case.Gj[l]
        theta, s = abs(h) * np.abs(G).sum(axis=0).max(), 0
        while theta > 0.25 and s < 60:
            theta, s = theta / 2, s + 1
        hs = np.ldexp(h, -s)
        X = z[case.xo[0] : case.xo[0] + xdc].reshape(C, n).T
        tails = np.empty((v + 1, C, m + 1, n))
        blocks = []
        for i in range(1, v + 1):
            Gv = case.Gv[i - 1]
            Xv = z[case.xo[i] : case.xo[i] + xdc].reshape(C, n).T
            quad = {}
            for l in range(max(m, 1)):
                Gl = case.Gj[l] if m else None
                T, Tp, Tq, Tw = I.copy(), np.zeros((n, n)), np.zeros((n, n)), np.zeros((n, n))
                for j in range(14, 0, -1):
                    a = hs / j
                    if m:
                        Tw = a * (G @ Tw + Gv @ Tq + Gl @ Tp)
                    Tp = a * (G @ Tp + Gv @ T)
                    if m:
                        Tq = a * (G @ Tq + Gl @ T)
                    T = I + a * (G @ T)
                for _ in range(s):
                    if m:
                        Tw = T @ Tw + Tw @ T + Tp @ Tq + Tq @ Tp
                    Tp, Tq, T = T @ Tp + Tp @ T, T @ Tq + Tq @ T, T @ T
                quad[l] = (T, Tp, Tq, Tw)
                if m:
                    tails[i, :, l, :] = -(Tw @ X + Tq @ Xv).T
                    if i == 1:
                        tails[0, :, l, :] = -(Tq @ X).T
            E, L = quad[0][0], quad[0][1]
            Y0, Yi = E @ X, L @ X + E @ Xv
            if i == 1:
                delta[k, :xdc] = zn[case.xo[0] : case.xo[0] + xdc] - Y0.T.reshape(-1)
                tails[0, :, m, :] = -(G @ Y0).T
                blocks.append(np.tile((-E).T.reshape(-1), C))
            delta[k, i * xdc : (i + 1) * xdc] = zn[case.xo[i] : case.xo[i] + xdc] - Yi.T.reshape(-1)
            tails[i, :, m, :] = -(Gv @ Y0 + G @ Yi).T
            blocks += [np.tile((-E).T.reshape(-1), C), np.tile((-L).T.reshape(-1), C)]
        vals[k] = np.concatenate(blocks + [np.ones(xd), tails.reshape(-1)])
        assert len(np.concatenate(blocks)) == seg1
    return delta.reshape(-1), vals.reshape(-1)


# the step sizes of the GPU tests that take several squarings are here too
REC_CASES = [c[0] for c in CASES] + ["config2_v1_dt4", "config2_m0"]
CASES += [("config2_v1_dt4", lambda: cases.config2(1, dt=4.0)[3]), ("config2_m0", lambda: _no_drives(cases.config2(2)[3]))]


def _no_drives(case):
    """The same knots read as a drift-only problem (the drive slots become idle variables)."""
    return dataclasses.replace(case, m=0, Gj=np.zeros((0, case.n, case.n)))


@pytest.mark.parametrize("name", REC_CASES)
def test_kernel_recurrence_in_numpy_against_truth(name):
    """Worst relative deviation measured here: 4e-15; the GPU tests compare at 1e-11."""
    case = case_of(name)
    d, vals = recurrence(case)
    td, tv = truth.residual(case), truth.values(case)
    ed = np.abs(d - td).max() / max(1.0, np.abs(td).max())
    ev = np.abs(vals - tv).max() / max(1.0, np.abs(tv).max())
    print("%s: recurrence against truth: delta %.3e, values %.3e" % (name, ed, ev))
    assert ed <= 1e-12 and ev <= 1e-12, (ed, ev)


def test_python_constructors_map_the_keyword():
    """pade_order="exp" on the variational constructors asks for the new batch mode; the context mirror still hands
    (PCL_ORDER_EXP, PCL_BATCH_VARIATIONAL) to pcl_create, which refuses it."""
    import inspect

    src = inspect.getsource(pa.integrators.HipVariationalIntegrator.__init__)
    assert "PCL_BATCH_VARIATIONAL_EXP" in src
    with pytest.raises(pa.PclError) as ei:
        pa.integrators._PclContext(d=2, m=0, N=3, z_dim=18, u_off=17, dt_off=16, x_offs=[0, 8], G0=np.zeros((2, 4, 4)), Gj=np.zeros((0, 4, 4)), batch=2,
                                   batch_mode=pa._lib.PCL_BATCH_VARIATIONAL, per_member_G0=True, pade_order="exp", state_cols=2)  # fmt: skip
    assert ei.value.code == pa._lib.PCL_ENOTIMPL and "PCL_BATCH_VARIATIONAL_EXP" in str(ei.value)
