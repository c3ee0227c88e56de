"""The dispatch trace of the launch ladders (launch_fused, launch_hess): which kernel a context, its options and an entry point end on, and
the text a forced option that cannot be served is refused with.  tests/test_dispatch_trace_gpu.py runs `run_case` on every case of `CASES`
and compares with tests/golden/dispatch_trace.json for equality; this file run as a script (on an MI355X) writes that table:

    python tests/golden/make_dispatch_trace.py [out.json]

Everything goes through the host-pointer entry points of the Python mirror (eval, eval_jac with host_path 1, hess), a fresh context per case.
What the suite's forced-option tests do not pin together is the FALL-THROUGH: which rung takes a launch after the rungs before it declined.

Shapes: BASELINE config 2 (d = 4: the small-system kernel and kernel 1); a d = 9, m = 2 sparse exact-iso system (the smallest the
pattern-compiled kernels take) at orders 4 and 8, one trajectory of N = 6 (5 intervals: far below n_cu / 2) and BIG_BATCH trajectories of
BIG_N knots (batch x K x ng = 8316 column-group waves against the R-chain rule's 8 n_cu = 2048); a d = 12 dense-drift system whose drives
have one entry per row (versions 3 / 2 and the general-order kernels), as a unitary problem and as a ket.  Every n_cu-dependent rule is a
factor of four or more from its threshold at n_cu = 256; n_cu and max_lds are recorded for information only."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import piccolo_jl_amd as pa  # noqa: E402
from oracle import pade_oracle as po  # noqa: E402
from shape_cases import controlled_system  # noqa: E402

FIELDS = {"last_kernel": "last_kernel", "last_n_stream": "last_stream_workgroups", "last_eval_coop": "last_eval_coop", "last_v4_ticket": "last_v4_ticket",
          "last_hess_kernel": "last_hess_kernel", "last_hess_split": "last_hess_split", "last_hess_pair": "last_hess_pair", "last_hess_rpre": "last_hess_rpre"}  # fmt: skip
BIG_BATCH, BIG_N = 132, 64


def system(name):
    """(d, G0, Gj) of a named system, from fixed seeds."""
    if name == "config2":
        s = pa.synthetic.config_system(2)
        return s.levels, s.G_drift, s.G_drives_array()
    if name == "sparse9":
        G0, Gj = controlled_system(9, [(0,), (1,)], np.random.default_rng(9), drift="classes")
        return 9, G0, Gj
    if name == "dense12":  # a dense Hermitian drift; two drives with one entry per row and column (widths 1: versions 2 and 3 of the Hessian take them)
        rng = np.random.default_rng(12)
        A = rng.standard_normal((12, 12)) + 1j * rng.standard_normal((12, 12))
        H1, H2 = np.zeros((12, 12), dtype=complex), np.zeros((12, 12), dtype=complex)
        H1[0, 1] = H1[1, 0] = 1.0
        H2[2, 3], H2[3, 2] = 1j * np.sqrt(2.0), -1j * np.sqrt(2.0)
        return 12, po.G_of_H(A + A.conj().T), np.array([po.G_of_H(H1), po.G_of_H(H2)])
    raise ValueError(name)


def case(cid, sysname, entry, order=4, N=6, batch=1, ket=False, **options):
    return dict(id=cid, system=sysname, entry=entry, order=order, N=N, batch=batch, ket=ket, options=options)


S9, D12 = "sparse9", "dense12"
BIG = dict(N=BIG_N, batch=BIG_BATCH)
CASES = [
    # BASELINE config 2: kernel 5 by default, kernel 1 behind it
    case("config2-eval_jac", "config2", "eval_jac", N=12),
    case("config2-eval", "config2", "eval", N=12),
    case("config2-hess", "config2", "hess", N=12),
    case("config2-eval_jac-general", "config2", "eval_jac", N=12, general_pade_kernel=1),
    case("config2-eval_jac-k1", "config2", "eval_jac", N=12, kernel_version=1),
    case("config2-eval_jac-k2", "config2", "eval_jac", N=12, kernel_version=2),
    case("config2-eval_jac-o8", "config2", "eval_jac", N=12, order=8),
    # the sparse system, one trajectory of five intervals
    case("sparse9-o4-eval_jac", S9, "eval_jac"),
    case("sparse9-o4-eval", S9, "eval"),
    case("sparse9-o4-hess", S9, "hess"),
    case("sparse9-o8-eval_jac", S9, "eval_jac", order=8),
    case("sparse9-o8-eval", S9, "eval", order=8),
    case("sparse9-o8-hess", S9, "hess", order=8),
    case("sparse9-o4-eval-k2", S9, "eval", eval_kernel=2),
    case("sparse9-o4-eval-k1", S9, "eval", eval_kernel=1),
    case("sparse9-o4-eval_jac-k3", S9, "eval_jac", kernel_version=3),
    case("sparse9-o4-hess-k4", S9, "hess", hess_kernel=4),
    case("sparse9-o4-hess-k7", S9, "hess", hess_kernel=7),
    case("sparse9-o8-hess-k7", S9, "hess", order=8, hess_kernel=7),
    case("sparse9-o8-hess-general", S9, "hess", order=8, general_pade_kernel=1),
    # ... and many: the R-chain rule, the slice tickets, the order-4 pattern kernel
    case("sparse9-big-o4-eval_jac", S9, "eval_jac", **BIG),
    case("sparse9-big-o4-eval", S9, "eval", **BIG),
    case("sparse9-big-o4-hess", S9, "hess", **BIG),
    case("sparse9-big-o8-hess", S9, "hess", order=8, **BIG),
    case("sparse9-big-o8-eval", S9, "eval", order=8, **BIG),
    # jit = 0: the pattern rungs decline, the ladders land on the matrix-core kernels
    case("sparse9-o4-eval_jac-nojit", S9, "eval_jac", jit=0),
    case("sparse9-o4-eval-nojit", S9, "eval", jit=0),
    case("sparse9-o4-hess-nojit", S9, "hess", jit=0),
    case("sparse9-o8-eval_jac-nojit", S9, "eval_jac", order=8, jit=0),
    case("sparse9-o8-hess-nojit", S9, "hess", order=8, jit=0),
    case("sparse9-big-o4-eval_jac-nojit", S9, "eval_jac", jit=0, **BIG),
    case("sparse9-big-o4-eval-nojit", S9, "eval", jit=0, **BIG),
    # the dense system: versions 3 / 2 / 1 and the general-order kernels
    case("dense12-o4-eval_jac", D12, "eval_jac"),
    case("dense12-o4-eval_jac-k2", D12, "eval_jac", kernel_version=2),
    case("dense12-o4-eval_jac-k3", D12, "eval_jac", kernel_version=3),
    case("dense12-o4-eval", D12, "eval"),
    case("dense12-o4-hess", D12, "hess"),
    case("dense12-o4-hess-nojit", D12, "hess", jit=0),
    case("dense12-o4-hess-k2", D12, "hess", hess_kernel=2),
    case("dense12-o4-hess-k1", D12, "hess", hess_kernel=1),
    case("dense12-o8-eval_jac", D12, "eval_jac", order=8),
    case("dense12-o8-eval", D12, "eval", order=8),
    case("dense12-o8-hess", D12, "hess", order=8),
    # ... as a ket
    case("dense12-ket-o4-eval_jac", D12, "eval_jac", ket=True),
    case("dense12-ket-o4-eval", D12, "eval", ket=True),
    case("dense12-ket-o4-hess", D12, "hess", ket=True),
    case("dense12-ket-o8-eval_jac", D12, "eval_jac", order=8, ket=True),
    case("dense12-ket-o8-hess", D12, "hess", order=8, ket=True),
    # forced options that must be refused, with their texts
    case("refuse-hess8-dense", D12, "hess", hess_kernel=8),
    case("refuse-hess7-dense", D12, "hess", hess_kernel=7),
    case("refuse-hess4-dense", D12, "hess", hess_kernel=4),
    case("refuse-hess3-sparse9-nojit", S9, "hess", hess_kernel=3, jit=0),
    case("refuse-hess8-sparse9-nojit", S9, "hess", hess_kernel=8, jit=0),
    case("refuse-kernel4-dense", D12, "eval_jac", kernel_version=4),
    case("refuse-kernel4-config2", "config2", "eval_jac", N=12, kernel_version=4),
    case("refuse-kernel5-dense", D12, "eval_jac", kernel_version=5),
    case("refuse-kernel5-sparse9", S9, "eval_jac", kernel_version=5),
    case("refuse-eval2-dense", D12, "eval", eval_kernel=2),
    case("refuse-eval3-dense", D12, "eval", eval_kernel=3),
]


def run_case(c):
    """One fresh context, the case's options, one call: the returned code, the error text of a refusal and the context's last_* values."""
    d, G0, Gj = system(c["system"])
    m, N, batch = len(Gj), c["N"], c["batch"]
    x_dim = 2 * d * (1 if c["ket"] else d)
    z_dim = x_dim + 1 + m
    ctx = pa.integrators._PclContext(d=d, m=m, N=N, z_dim=z_dim, u_off=x_dim + 1, dt_off=x_dim, x_offs=[0], G0=G0, Gj=Gj, batch=batch,
                                     batch_mode=pa._lib.PCL_BATCH_TRAJ if batch > 1 else pa._lib.PCL_BATCH_MEMBERS, pade_order=c["order"],
                                     state_cols=1 if c["ket"] else 0)  # fmt: skip
    try:
        ctx.set_option("host_path", 1)  # full values: the launch under test is the one the device-pointer entry points make
        for key, value in c["options"].items():
            ctx.set_option(key, value)
        rng = np.random.default_rng(1)
        Z = 0.1 * rng.standard_normal((batch, N, z_dim))
        Z[:, :, x_dim] = 0.05 + 0.1 * rng.random((batch, N))
        out = dict(rc=0, error="")
        try:
            if c["entry"] == "eval":
                ctx.eval(Z)
            elif c["entry"] == "eval_jac":
                ctx.eval_jac(Z)
            else:
                ctx.hess(Z, rng.standard_normal(ctx.n_rows))
        except pa._lib.PclError as e:
            out = dict(rc=e.code, error=(ctx._L.pcl_last_error(ctx._h) or b"").decode())
        for name, key in FIELDS.items():
            out[name] = ctx.get_option(key)
        out["n_cu"] = ctx.get_option("n_cu")
        return out
    finally:
        ctx.close()


def main(path):
    rows, n_cu = [], None
    for c in CASES:
        r = run_case(c)
        n_cu = r.pop("n_cu")
        rows.append(dict(c, expect=r))
        print(c["id"], r, flush=True)
    max_lds = None
    try:  # (for information only: nothing in the table depends on it at these shapes)
        import ctypes

        v = ctypes.c_int()
        if ctypes.CDLL("libamdhip64.so").hipDeviceGetAttribute(ctypes.byref(v), 10002, 0) == 0:  # hipDeviceAttributeMaxSharedMemoryPerMultiprocessor
            max_lds = v.value
    except Exception:
        pass
    with open(path, "w") as f:
        json.dump(dict(n_cu=n_cu, max_lds=max_lds, cases=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "dispatch_trace.json"))
