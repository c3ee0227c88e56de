"""CPU tests of the variational (sensitivity) integrators: the lifted truth against the reference's literal construction and against the
exp constraint, validation of PCL_BATCH_VARIATIONAL descriptors (before any device call), the host mirror's VariationalQuantumSystem, and a
resource check of the kernels' gfx950 code (no scratch)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.linalg

import piccolo_jl_amd as pa
from oracle import pade_oracle as po
from variational_truth import h_var_drift, lifted, literal_residual, make_case, residual

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = po.PAULIS


@pytest.fixture(scope="module")
def lib():
    pa.build_library()
    return pa._lib.load()


@pytest.mark.parametrize("ket", [False, True])
@pytest.mark.parametrize("nv", [1, 2])
def test_lifted_equals_literal_var_G(ket, nv):
    sys_o = po.config_system(2)  # d = 4, m = 4
    Gvs = [po.G_of_H(h_var_drift(2, 2)) / 10, po.G_of_H(np.kron(P["X"], P["I"])) / 3][:nv]
    case = make_case(sys_o, Gvs, N=5, seed=3, ket=ket)
    for order in (2, 4, 10):
        a, b = residual(case, order), literal_residual(case, order)
        assert np.abs(a - b).max() <= 1e-13 * max(1.0, np.abs(b).max()), order
        assert np.abs(b).max() > 1e-6  # (not a trivially zero residual)


def test_lifted_order10_matches_exp_constraint_config3():
    sys_o = po.config_system(3)
    Gv = po.G_of_H(h_var_drift(3, 3)) / 10
    case = make_case(sys_o, [Gv], N=3, seed=5, noise=0.0)  # exactly propagated: the exp constraint's residual is zero
    Zl, lay, G0l, Gjl = lifted(case)
    ex = po.exp_residual(Zl, lay, G0l, Gjl)
    assert np.abs(ex).max() < 1e-12
    r10 = residual(case, 10)
    assert np.abs(r10).max() < 1e-10
    assert np.abs(residual(case, 4)).max() > 1e-8  # order 4 is not (the policy's reason to go to 10)


def test_var_G_pin():
    G = np.arange(16.0).reshape(4, 4)
    Gv = -np.arange(16.0).reshape(4, 4).T
    L = po.var_G(G, [Gv])
    assert np.array_equal(L[:4, :4], G) and np.array_equal(L[4:, 4:], G) and np.array_equal(L[4:, :4], Gv) and not L[:4, 4:].any()


# ---- the C ABI: validation of a variational descriptor (no device here) ------------------------------------------------------------
def _desc(**over):
    d, m, N = 2, 2, 5
    n = 2 * d
    xd = n * d
    kw = dict(d=d, n_drives=m, N=N, z_dim=2 * xd + 2 + m, u_off=2 * xd + 2, dt_off=2 * xd, batch=2, batch_mode=2, pade_order=4, device_id=0,
              index_base=0, per_member_G0=1, state_cols=d, global_dim=0)  # fmt: skip
    x_offs = over.pop("x_offs", [0, xd])
    kw.update(over)
    nb, n = kw["batch"], 2 * kw["d"]
    G0 = np.zeros(n * n * max(nb, 1))
    Gj = np.zeros(n * n * max(m, 1))
    xo = np.array(x_offs + [0] * max(0, nb - len(x_offs)), dtype=np.int32)
    D = pa._lib.pcl_desc(struct_size=ctypes.sizeof(pa._lib.pcl_desc), G0=G0.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                         Gj=Gj.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), x_offs=xo.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), **kw)
    return D, (G0, Gj, xo)


def _create(lib, **over):
    D, keep = _desc(**over)
    h = ctypes.c_void_p()
    rc = lib.pcl_create(ctypes.byref(D), ctypes.byref(h))
    return rc, lib.pcl_last_error(None).decode()


@pytest.mark.parametrize("field, over, code", [
    ("batch", dict(batch=1, x_offs=[0]), pa._lib.PCL_EINVAL),
    ("per_member_G0", dict(per_member_G0=0), pa._lib.PCL_EINVAL),
    ("state_cols", dict(state_cols=pa._lib.PCL_STATE_VECTOR), pa._lib.PCL_EINVAL),
    ("state_cols", dict(state_cols=3, d=4, x_offs=[0, 24], z_dim=2 * 32 + 8 + 2, u_off=2 * 32 + 2 + 6, dt_off=2 * 32 + 6), pa._lib.PCL_EINVAL),
    ("x_offs[1]", dict(x_offs=[0, 40]), pa._lib.PCL_EINVAL),
    ("x_offs[1]", dict(x_offs=[0, 4]), pa._lib.PCL_EINVAL),  # overlaps the state
    ("x_offs[0]", dict(x_offs=[-1, 8]), pa._lib.PCL_EINVAL),
    ("u_off", dict(u_off=40), pa._lib.PCL_EINVAL),
    ("dt_off", dict(dt_off=-1), pa._lib.PCL_EINVAL),
    ("index_base", dict(index_base=2), pa._lib.PCL_EINVAL),
    ("N", dict(N=1), pa._lib.PCL_EINVAL),
    ("pade_order", dict(pade_order=3), pa._lib.PCL_ENOTIMPL),
    ("variations", dict(batch=4, x_offs=[0, 8, 16, 24], z_dim=4 * 8 + 4, u_off=34, dt_off=32), pa._lib.PCL_ESHAPE),
    ("d=33", dict(d=33, state_cols=0, x_offs=[0, 2178], z_dim=2 * 2178 + 4, dt_off=2 * 2178, u_off=2 * 2178 + 2), pa._lib.PCL_ESHAPE),
])  # fmt: skip
def test_variational_descriptor_validation(lib, field, over, code):
    rc, msg = _create(lib, **over)
    assert rc == code, (rc, msg)
    assert field.split("[")[0] in msg, msg


@pytest.mark.parametrize("state_cols, nv", [(2, 1), (1, 1), (0, 2), (2, 2)])
def test_valid_variational_descriptor_passes_validation(lib, state_cols, nv):
    d, m = 2, 2
    C = d if state_cols in (0, d) else 1
    xd = 2 * d * C
    z = (nv + 1) * xd
    rc, msg = _create(lib, state_cols=state_cols, batch=nv + 1, x_offs=[b * xd for b in range(nv + 1)], z_dim=z + 2 + m, u_off=z + 2, dt_off=z)
    assert rc == pa._lib.PCL_EHIP, (rc, msg)  # past validation: only the missing device stops it
    assert "no HIP device" in msg or "gfx950" in msg or "device" in msg


def test_mode_7_still_rejected(lib):
    rc, msg = _create(lib, batch_mode=7)
    assert rc == pa._lib.PCL_EINVAL and "batch_mode" in msg


# ---- host mirror --------------------------------------------------------------------------------------------------------------------
def test_variational_quantum_system_literals():
    """[REF src/quantum/systems/variational_quantum_systems.jl: "Variational system creation", "... drive_bounds conversion"]"""
    Pm = pa.PAULIS
    bounds = [(-1.0, 1.0), (-1.0, 1.0)]
    a = np.array([1.0, 2.0])
    GX, GY = pa.quantum.G(Pm["X"]), pa.quantum.G(Pm["Y"])
    Gref = a[0] * GX + a[1] * GY
    s1 = pa.VariationalQuantumSystem(0.0 * Pm["Z"], [Pm["X"], Pm["Y"]], [Pm["X"], Pm["Y"]], bounds)
    s2 = pa.VariationalQuantumSystem([Pm["X"], Pm["Y"]], [Pm["X"], Pm["Y"]], bounds)
    for s in (s1, s2):
        assert s.n_drives == 2 and len(s.G_vars) == 2 and s.drive_bounds == bounds
        assert np.allclose(s.G(a), Gref)
        assert np.allclose(s.G_vars[0](a), GX) and np.allclose(s.G_vars[1](a), GY)
    s3 = pa.VariationalQuantumSystem([Pm["X"], Pm["Y"]], [Pm["X"]], bounds)
    assert s3.n_drives == 2 and len(s3.G_vars) == 1 and np.allclose(s3.G(a), Gref) and np.allclose(s3.G_vars[0](a), GX)
    with pytest.raises(NotImplementedError):
        pa.VariationalQuantumSystem(lambda u: u[0] * Pm["X"] + u[1] * Pm["Y"], [lambda u: u[0] * Pm["X"], lambda u: Pm["Y"]], 2, bounds)
    assert pa.VariationalQuantumSystem(Pm["Z"], [Pm["X"], Pm["Y"]], [Pm["X"]], [1.0, 1.5]).drive_bounds == [(-1.0, 1.0), (-1.5, 1.5)]
    assert pa.VariationalQuantumSystem(Pm["Z"], [Pm["X"], Pm["Y"]], [Pm["X"]], [(-0.5, 1.0), (-1.5, 0.5)]).drive_bounds == [(-0.5, 1.0), (-1.5, 0.5)]
    with pytest.raises(AssertionError):
        pa.VariationalQuantumSystem(Pm["Z"], [Pm["X"]], [], [1.0])
    with pytest.raises(TypeError):  # the bounds left out: not re-read as the no-drift form with shifted arguments
        pa.VariationalQuantumSystem(Pm["Z"], [Pm["X"], Pm["Y"]], [Pm["X"]])


def test_constructors_exported_and_checked():
    assert callable(pa.VariationalUnitaryIntegrator) and callable(pa.VariationalKetIntegrator)
    sysv = pa.VariationalQuantumSystem(pa.PAULIS["Z"] / 2, [pa.PAULIS["X"], pa.PAULIS["Y"]], [pa.PAULIS["Z"] / 2], [1.0, 1.0])
    N = 5
    traj = pa.NamedTrajectory({"ψ̃": np.zeros((4, N)), "ψ̃_var": np.zeros((3, N)), "u": np.zeros((2, N)), "Δt": np.full((1, N), 0.1)},
                              controls=("u", "Δt"), timestep="Δt")
    with pytest.raises(ValueError, match="ψ̃_var"):  # component lengths are checked before any device is touched
        pa.VariationalKetIntegrator(sysv, traj, "ψ̃", ["ψ̃_var"], "u")
    with pytest.raises(ValueError):
        pa.VariationalKetIntegrator(sysv, traj, "ψ̃", [], "u")


# ---- the kernels' code ----------------------------------------------------------------------------------------------------------------
def test_variational_kernels_compile_without_scratch(tmp_path):
    """Every instance the library launches (v = 1, 2; orders 2 .. 10; residual + Jacobian, residual only, Hessian) compiles for gfx950 with no
    scratch; the VGPR and LDS figures are printed for the record."""
    csrc = os.path.join(ROOT, "piccolo.jl_amd", "csrc")
    lines = ["#include <hip/hip_runtime.h>", '#include "pcl_kernel_variational.hpp"']
    for v in (1, 2):
        for q in range(1, 6):
            lines += ["template __global__ void pcl_var_fused_kernel<%d, %d, true>(VarParams);" % (v, q),
                      "template __global__ void pcl_var_fused_kernel<%d, %d, false>(VarParams);" % (v, q),
                      "template __global__ void pcl_var_hess_kernel<%d, %d>(VarParams);" % (v, q)]  # fmt: skip
    src = tmp_path / "var_kernels.hip"
    src.write_text("\n".join(lines) + "\n")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", "-I", csrc, str(src), "-o", str(tmp_path / "k.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)  # fmt: skip
    assert r.returncode == 0, r.stderr[-4000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    vgprs = [int(x) for x in re.findall(r"VGPRs: (\d+)", r.stderr)]
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == 30 and len(vgprs) == 30 and len(scratch) == 30, r.stderr[-2000:]
    for nm, vg, sc in zip(names, vgprs, scratch):
        print("%-60s VGPRs %3d  scratch %d" % (nm, vg, sc))
        assert sc == 0, nm
        assert vg <= 256, nm  # 512-thread workgroups: two waves per SIMD
