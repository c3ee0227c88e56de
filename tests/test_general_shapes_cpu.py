"""CPU side of the general-shape tests (no GPU): the plain cases of tests/shape_cases.py keep straddling the limits they name -- the code
generator accepts or refuses each as the case table claims, the union-pattern rule of pcl_create admits or refuses F6 -- the generator's
term tables reproduce G(u) x and G(u)^T x for every pattern-compiled case, and the fused and column-group Hessian sources of the largest
orders compile for gfx950."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import piccolo_jl_amd as pa
from shape_cases import K_MAX_MAGS, KV4_MAX_CF, PLAIN_CASES, SP_MAX_NZ, cf_pairs, n_mags, plain_case, plain_system, sp_rule_admits, union_nz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "piccolo.jl_amd", "csrc")
# what pcl_codegen_source_v4 answers for the iso cases with m <= 6 (0: kernel 4 family; PCL_ESHAPE: refused)
KERNEL4 = {"S1": True, "S2": True, "S3": True, "S4": True, "S5": True, "S6": False, "F1": False, "F2": False, "F6": True}
PATTERN_COMPILED = ("S1", "S2", "S3", "S4", "S5")


@pytest.fixture(scope="module")
def lib():
    pa.build_library()
    return pa._lib.load()


def _cm(G0, Gj):
    return np.ascontiguousarray(G0.T).ravel(), np.ascontiguousarray(np.stack([g.T for g in Gj])).ravel()


def _source(lib, name, q, what):
    G0, Gj = plain_system(name)
    d, m = G0.shape[0] // 2, len(Gj)
    g0, gj = _cm(G0, Gj)
    need = ctypes.c_int64()
    rc = lib.pcl_codegen_source_v4(d, m, g0.ctypes.data, 1, gj.ctypes.data, q, what, None, 0, ctypes.byref(need))
    if rc != 0:
        return rc, None
    buf = ctypes.create_string_buffer(need.value)
    assert lib.pcl_codegen_source_v4(d, m, g0.ctypes.data, 1, gj.ctypes.data, q, what, buf, need.value, ctypes.byref(need)) == 0
    return 0, buf.value.decode()


@pytest.mark.parametrize("name", sorted(KERNEL4))
def test_classification_matches_the_case_table(lib, name):
    G0, Gj = plain_system(name)
    dm = PLAIN_CASES[name][1]
    # the limits each case claims to sit at or beyond
    if name == "S2":
        assert cf_pairs(dm) == KV4_MAX_CF and n_mags(dm) == K_MAX_MAGS
    if name == "F1":
        assert cf_pairs(dm) == KV4_MAX_CF + 1 and n_mags(dm) <= K_MAX_MAGS
    if name == "F2":
        assert n_mags(dm) == K_MAX_MAGS + 1 and cf_pairs(dm) <= KV4_MAX_CF
    for q in (1, 3, 4, 5):
        rc, _ = _source(lib, name, q, 0)
        assert rc == (0 if KERNEL4[name] else pa._lib.PCL_ESHAPE), (name, q, rc)
        # the column-group Hessian kernel: also at most kHcMaxMags = 7 drive magnitudes (S2 has 8)
        rc, _ = _source(lib, name, q, 5)
        assert rc == (0 if KERNEL4[name] and name != "S2" else pa._lib.PCL_ESHAPE), (name, q, rc)
    # the union-pattern rule of pcl_create (piccolo_hip.hip): F6 is too dense, every other case is not
    nz = union_nz(G0, Gj)
    d = G0.shape[0] // 2
    assert sp_rule_admits(G0, Gj) == (name != "F6"), nz
    if name == "F6":
        assert nz > SP_MAX_NZ


def test_drift_value_classes_resident_or_streamed(lib):
    """S3's drift has a value class per entry (more than the resident slots: streamed); S1's few classes are all resident."""
    for name, streamed in (("S3", True), ("S1", False), ("S5", False)):
        rc, src = _source(lib, name, 4, 0)
        assert rc == 0
        body = src[src.index("void sp4_product("):src.index("void sp4_product0(")]
        assert ("s_load" in body) == streamed, name
        assert ("#define SP4_COOP 1" in src) == (not streamed), name  # (the cooperative residual kernel needs every coefficient resident)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    """The host-only restatement of the generated products (pcl_codegen_v4.hpp) behind the lab header's signature, as
    tests/test_abi_cpu.py::test_pattern_compiled_fused_and_hessian_sources builds it."""
    tmp = tmp_path_factory.mktemp("shim")
    src = tmp / "apply_shim.cpp"
    src.write_text('#include "pcl_codegen_v4.hpp"\n'
                   'extern "C" int pcl_codegen_apply_v4(int d, int m, const double *G0, int n_g0, const double *Gj, const double *u, const double *x, double *y, int transposed) {\n'
                   '    const pcl_codegen::V4Plan plan = pcl_codegen::make_v4_plan(d, m, G0, n_g0, Gj);\n'
                   '    if (!plan.ok) return -5;\n'
                   '    if (transposed) pcl_codegen::v4_reference_apply_t(plan, G0, u, x, y); else pcl_codegen::v4_reference_apply(plan, G0, Gj, u, x, y);\n'
                   '    return 0;\n}\n')  # fmt: skip
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I", CSRC, "-o", str(tmp / "apply_shim.so"), str(src)])
    L = ctypes.CDLL(str(tmp / "apply_shim.so"))
    L.pcl_codegen_apply_v4.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_int]
    return L


@pytest.mark.parametrize("name", PATTERN_COMPILED)
def test_term_tables_reproduce_the_products(shim, name):
    lay, G0, Gj, Z = plain_case(name)
    d, m, n = lay.d, lay.m, lay.n
    g0, gj = _cm(G0, Gj)
    rng = np.random.default_rng(5)
    for tr in (0, 1):
        for k in range(lay.K):
            u, x, y = np.ascontiguousarray(Z[k, lay.u_off : lay.u_off + m]), rng.normal(size=n), np.zeros(n)
            assert shim.pcl_codegen_apply_v4(d, m, g0.ctypes.data, 1, gj.ctypes.data, u.ctypes.data, x.ctypes.data, y.ctypes.data, tr) == 0
            G = G0 + np.tensordot(u, Gj, axes=1)
            ref = (G.T if tr else G) @ x
            assert np.abs(ref - y).max() <= 1e-13 * max(1.0, np.abs(ref).max()), (name, tr)


@pytest.mark.parametrize("name", ["S3", "S5"])
def test_order_10_sources_compile_for_gfx950(lib, tmp_path, name):
    """The fused kernel (what 0) and the column-group Hessian kernel (what 5) at q = 5: S3 (streamed drift classes) and S5 (d = 32, every
    lane of a half wave; S6 is refused by the generator).  The fused kernels keep the scratch bound of the existing source test.  At d = 32
    the pair kernel's LDS outgrows its 16-bit offsets from q = 4 on: the module holds the one-wave column-group kernel alone."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    for what, kernels in ((0, ("pcl_fused_sparse_kernel", "pcl_eval_sparse4_kernel")), (5, ("pcl_hess_cols_kernel",))):
        rc, src = _source(lib, name, 5, what)
        assert rc == 0 and "#define SP4Q 5" in src
        f = tmp_path / ("%s_%d.hip" % (name, what))
        f.write_text(src)
        out = tmp_path / ("%s_%d.s" % (name, what))
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-include", "hip/hip_runtime.h", "-I", CSRC, "-S", "--cuda-device-only",
                            "-o", str(out), str(f)], capture_output=True, text=True)  # fmt: skip
        assert r.returncode == 0, r.stderr[-2000:]
        asm = out.read_text()
        for k in kernels:
            assert k in asm
        if what == 5:
            assert ("pcl_hess_cols_pair_kernel" in asm) == (name != "S5")
        if what == 0:
            scratch = [int(x) for x in re.findall(r"; ScratchSize: (\d+)", asm)]
            assert max(scratch) <= 64, scratch
