"""Measurement of the large-generator kernel (contexts created with PCL_LARGE_N; pcl_kernel_pade_large.hpp) on a dispersive qubit-cavity system.

System, written from the physics (rotating frame of both modes, b the transmon's and a the cavity's lowering operator, hbar = 1, rad / ns):
    H0 = (alpha / 2) b'b'b b  +  chi a'a b'b  +  (kerr / 2) a'a'a a
    drives: b + b',  i (b' - b),  a + a',  i (a' - a)                      (four real controls)
with alpha = -2 pi 0.2, chi = -2 pi 0.002, kerr = -2 pi 1e-5; the transmon keeps 4 levels, the cavity 12 or 15: d = 48 and d = 60, generator
dimension n = 2 d = 96 and 120.  States: one ket and five kets (state_cols 1 and 5).  N = 100 knots, Pade orders 4 and 10.

Writes ONE JSON document (--out, default profiles/large_bench.json) and prints it as one line; per case:
  plan        what the launch code chose: workgroups per interval, threads, LDS bytes (read back through the Python restatement of large_plan in
              tests/large_shape_cases.py, the one the CPU tests hold against the table)
  launch_us   pcl_eval_jac_dev and pcl_eval_dev by HIP events: the median of --launches launches after --warmup warm-up launches
  bytes       stored per launch (residual and Jacobian values, 8 per value)
  flops       of the formulation, dense: per interval and level one product G [W | V | dW_1 .. dW_m | P] of 2 n^2 (cols (2 + m) + n) flops, the
              last level without the n columns of the powers (16 x 4 blocks of G without a nonzero are skipped by the kernel and still counted)
  cpu         the CPU comparators on --threads threads: the reference formulation in numpy (oracle/pade_oracle.py) for the SAME shape and order,
              and the C restatement (oracle/pade_ref.c) -- which has order 4 on d state columns only, so it is timed once per d, on that shape
There is no threshold: nothing at these sizes was measured before, and no earlier commit can run them.

    python bench/bench_large.py [--launches 50] [--warmup 5] [--threads 16] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TWO_PI = 2.0 * np.pi
ALPHA, CHI, KERR = -TWO_PI * 0.2, -TWO_PI * 0.002, -TWO_PI * 1e-5
QUBIT_LEVELS = 4


def lower(levels):
    return np.diag(np.sqrt(np.arange(1, levels)), 1).astype(complex)


def qubit_cavity(cavity_levels):
    """(H0, [four drive Hamiltonians]) on the qubit (x) cavity space, d = 4 cavity_levels."""
    b = np.kron(lower(QUBIT_LEVELS), np.eye(cavity_levels))
    a = np.kron(np.eye(QUBIT_LEVELS), lower(cavity_levels))
    bd, ad = b.conj().T, a.conj().T
    H0 = 0.5 * ALPHA * bd @ bd @ b @ b + CHI * (ad @ a) @ (bd @ b) + 0.5 * KERR * ad @ ad @ a @ a
    return H0, [b + bd, 1j * (bd - b), a + ad, 1j * (ad - a)]


def iso_generator(H):
    """G(H) = iso(-i H) = [[Im H, Re H], [-Re H, Im H]]"""
    return np.block([[H.imag, H.real], [-H.real, H.imag]])


def trajectory(d, cols, m, N, rng):
    """Knots [X | dt | t | u]: normalised random kets, dt = 0.05 ns, |u| ~ 2 pi 0.01."""
    n = 2 * d
    xd = n * cols
    Z = np.zeros((N, xd + 2 + m))
    X = rng.standard_normal((N, cols, n))
    Z[:, :xd] = (X / np.linalg.norm(X, axis=2, keepdims=True)).reshape(N, xd)
    Z[:, xd] = 0.05
    Z[:, xd + 1] = np.cumsum(Z[:, xd])
    Z[:, xd + 2 :] = TWO_PI * 0.01 * rng.standard_normal((N, m))
    return Z


def flops_dense(n, cols, m, q, K):
    chain = cols * (2 + m)
    return K * ((q - 1) * 2 * n * n * (chain + n) + 2 * n * n * chain)


def median_us(pairs):
    return round(float(np.median([e0.elapsed_time(e1) * 1e3 for e0, e1 in pairs])), 2)


def measure(torch, pa, po, lc, G0, Gj, d, cols, order, a, rng):
    n, m, N = 2 * d, len(Gj), a.N
    Z = trajectory(d, cols, m, N, rng)
    xd = n * cols
    lay = po.Layout(d=d, m=m, N=N, z_dim=xd + 2 + m, x_off=0, u_off=xd + 2, dt_off=xd, cols=cols)
    c = pa.integrators._PclContext(d=d, m=m, N=N, z_dim=lay.z_dim, u_off=lay.u_off, dt_off=lay.dt_off, x_offs=[0], G0=G0, Gj=Gj, batch=1,
                                   batch_mode=pa._lib.PCL_BATCH_MEMBERS, pade_order=order, state_cols=cols, large_generator=True)  # fmt: skip
    stream = torch.cuda.current_stream()
    c.set_stream(stream.cuda_stream)
    Zd = torch.from_numpy(Z.reshape(-1).copy()).cuda()
    dd = torch.empty(c.n_rows, dtype=torch.float64, device="cuda")
    vd = torch.empty(c.jac_nnz, dtype=torch.float64, device="cuda")
    jobs = {"eval_jac": lambda: c.eval_jac_dev(Zd, dd, vd), "eval": lambda: c.eval_dev(Zd, dd)}
    kern = {}
    for nm, j in jobs.items():
        j()
        kern[nm] = c.get_option("last_kernel")
    torch.cuda.synchronize()
    # against the reference formulation on the CPU (numpy with --threads BLAS threads), the same shape and order; timed
    t0 = time.perf_counter()
    d_ref = po.pade_residual(Z, lay, G0, Gj, order).reshape(-1)
    j_ref = po.pade_jacobian_values(Z, lay, G0, Gj, order).reshape(-1)
    t_np = time.perf_counter() - t0
    c.eval_jac_dev(Zd, dd, vd)
    torch.cuda.synchronize()
    err_d = float(np.abs(dd.cpu().numpy() - d_ref).max() / np.abs(d_ref).max())
    err_j = float(np.abs(vd.cpu().numpy() - j_ref).max() / np.abs(j_ref).max())
    for _ in range(a.warmup):
        for j in jobs.values():
            j()
    torch.cuda.synchronize()
    evs = {nm: [] for nm in jobs}
    for _ in range(a.launches):
        for nm, j in jobs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            j()
            e1.record(stream)
            evs[nm].append((e0, e1))
    torch.cuda.synchronize()
    us = {nm: median_us(v) for nm, v in evs.items()}
    K, q = N - 1, order // 2
    nbytes = {"eval_jac": 8 * (c.n_rows + c.jac_nnz), "eval": 8 * c.n_rows}
    fl = {"eval_jac": flops_dense(n, cols, m, q, K), "eval": K * q * 2 * n * n * cols}
    plan = {w: lc.large_plan(n, cols, m, jac=(w == "eval_jac"), items=K, n_cu=c.get_option("n_cu")) for w in jobs}
    out = {"d": d, "n": n, "state_cols": cols, "m": m, "N": N, "order": order, "max_rel_err_vs_numpy": {"residual": err_d, "jacobian": err_j}}
    for w in jobs:
        p = plan[w]
        out[w] = {"last_kernel": kern[w], "launch_us": us[w], "launches": a.launches, "warmup": a.warmup, "bytes_stored": nbytes[w], "flops_dense": fl[w],
                  "GB_per_s_stored": round(nbytes[w] / us[w] * 1e-3, 1), "GFLOP_per_s_dense": round(fl[w] / us[w] * 1e-3, 1),
                  "plan": {"workgroups_per_interval": p["U"], "threads": p["threads"], "lds_bytes": p["bytes"], "state_columns_per_workgroup": p["nc"],
                           "drive_groups": p["ngrp"], "power_columns_per_workgroup": p["npc"]}}  # fmt: skip
    out["cpu"] = {"threads": a.threads, "numpy_reference_formulation_ms": round(1e3 * t_np, 1),
                  "numpy_reference_formulation_what": "oracle/pade_oracle.py pade_residual + pade_jacobian_values, this shape and order, one call"}  # fmt: skip
    c.close()
    return out


def c_restatement(po, ref_lib, G0, Gj, d, a, rng):
    """oracle/pade_ref.c: Pade order 4 on d state columns (a unitary) -- the only shape it has.  Best of three on --threads threads."""
    m, N = len(Gj), a.N
    Z = trajectory(d, d, m, N, rng)
    xd = 2 * d * d
    lay = po.Layout(d=d, m=m, N=N, z_dim=xd + 2 + m, x_off=0, u_off=xd + 2, dt_off=xd)
    out = None
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        out = ref_lib.eval_jac(Z, lay, G0, Gj, nthreads=a.threads, out=out)
        ts.append(time.perf_counter() - t0)
    return {"what": "pade_ref_eval_jac: order 4, d = %d state columns (unitary), N = %d; the C restatement has no other order or column count" % (d, N),
            "threads": a.threads, "best_of_3_ms": round(1e3 * min(ts), 1), "bytes_stored": 8 * (N - 1) * (po.jac_nnz_per_interval(lay) + xd)}  # fmt: skip


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--N", type=int, default=100)
    ap.add_argument("--cavity-levels", default="12,15")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "large_bench.json"))
    a = ap.parse_args()
    for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
        os.environ[v] = str(a.threads)

    import torch

    import large_shape_cases as lc
    import piccolo_jl_amd as pa
    from oracle import pade_oracle as po
    from oracle import ref_lib

    torch.set_num_threads(a.threads)
    rng = np.random.default_rng(2026)
    out = {"system": "dispersive qubit-cavity, 4 transmon levels x cavity levels, four drives (see the module docstring)", "device": torch.cuda.get_device_name(0),
           "cases": [], "c_restatement": []}  # fmt: skip
    for cl in [int(s) for s in a.cavity_levels.split(",")]:
        d = QUBIT_LEVELS * cl
        H0, Hs = qubit_cavity(cl)
        G0, Gj = iso_generator(H0), np.array([iso_generator(H) for H in Hs])
        nz = float(np.mean((np.abs(G0) + np.abs(Gj).sum(axis=0)) != 0))
        for cols in (1, 5):
            for order in (4, 10):
                r = measure(torch, pa, po, lc, G0, Gj, d, cols, order, a, rng)
                r["generator_nonzero_fraction"] = round(nz, 4)
                out["cases"].append(r)
                print("d %d cols %d order %d: eval_jac %.1f us, eval %.1f us" % (d, cols, order, r["eval_jac"]["launch_us"], r["eval"]["launch_us"]), file=sys.stderr, flush=True)
        out["c_restatement"].append(dict(c_restatement(po, ref_lib, G0, Gj, d, a, rng), d=d, n=2 * d))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
