"""Measurement of the large exponential kernel (contexts created with PCL_LARGE_N | PCL_LARGE_EXP on pade_order = PCL_ORDER_EXP;
pcl_kernel_large_exp.hpp) on the dispersive qubit-cavity systems of bench/bench_large.py: 4 transmon levels x 12 or 15 cavity levels (generator
dimension n = 96 and 120), four drives, N = 100 knots, one ket and the unitary state (state_cols 1 and d).

Writes ONE JSON document (--out, default profiles/large_exp_bench.json) and prints it as one line; per case:
  substeps         s' = ceil(|dt| |G(u_k)|_1) over the intervals (min, max): the launch's cost is linear in it
  plan             what the launch code chose (the Python restatement of large_exp_plan in tests/large_exp_cases.py)
  launch_us        pcl_eval_jac_dev and pcl_eval_dev by HIP events: the median of --launches launches after --warmup warm-up launches
  comparators      pade10_jac_us      the same system's Pade order-10 residual + Jacobian launch on a large Pade context (context: the constraints differ)
                   rollout_expm_us    a large Pade context's rollout propagator launch (large_full, large_rollout_stage = 1): n columns of E per interval
                   predicted_us       rollout_expm_us (n + cols (1 + 2 m)) / n: the product count of this launch in propagator panel passes
                   measured_over_predicted
                   scipy_ms           scipy.linalg.expm + expm_frechet per drive over the same intervals on --threads threads, with the products that
                                      make the values of them
There is no threshold: nothing ran this launch before.

    python bench/bench_large_exp.py [--launches 30] [--warmup 3] [--threads 16] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "bench"))


def median_us(pairs):
    return round(float(np.median([e0.elapsed_time(e1) * 1e3 for e0, e1 in pairs])), 2)


def timed(torch, stream, job, a):
    for _ in range(a.warmup):
        job()
    torch.cuda.synchronize()
    evs = []
    for _ in range(a.launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        job()
        e1.record(stream)
        evs.append((e0, e1))
    torch.cuda.synchronize()
    return median_us(evs)


def scipy_values(Z, lay, G0, Gj):
    """delta and the Jacobian's distinct values by scipy: E, L_l X_k, G E X_k per interval (what the CPU would have to compute)."""
    import scipy.linalg

    acc = 0.0
    for k in range(lay.K):
        G = G0 + np.tensordot(lay.u(Z, k), Gj, axes=1)
        h = lay.dt(Z, k)
        X = lay.X(Z, k)
        E = scipy.linalg.expm(h * G)
        Y = E @ X
        acc += float((lay.X(Z, k + 1) - Y)[0, 0]) + float((G @ Y)[0, 0])
        for l in range(lay.m):
            acc += float((scipy.linalg.expm_frechet(h * G, h * Gj[l], compute_expm=False) @ X)[0, 0])
    return acc


def measure(torch, pa, po, le, bl, G0, Gj, d, cols, a, rng):
    n, m, N = 2 * d, len(Gj), a.N
    Z = bl.trajectory(d, cols, m, N, rng)
    xd = n * cols
    lay = po.Layout(d=d, m=m, N=N, z_dim=xd + 2 + m, x_off=0, u_off=xd + 2, dt_off=xd, cols=cols)
    base = dict(d=d, m=m, N=N, z_dim=lay.z_dim, u_off=lay.u_off, dt_off=lay.dt_off, x_offs=[0], G0=G0, Gj=Gj, batch=1, batch_mode=pa._lib.PCL_BATCH_MEMBERS,
                state_cols=cols, large_generator=True)  # fmt: skip
    stream = torch.cuda.current_stream()
    Zd = torch.from_numpy(Z.reshape(-1).copy()).cuda()
    sp = [le.substeps(lay.dt(Z, k), G0 + np.tensordot(lay.u(Z, k), Gj, axes=1)) for k in range(lay.K)]
    # the launch under measurement
    c = pa.integrators._PclContext(pade_order="exp", large_exp=True, **base)
    c.set_stream(stream.cuda_stream)
    dd = torch.empty(c.n_rows, dtype=torch.float64, device="cuda")
    vd = torch.empty(c.jac_nnz, dtype=torch.float64, device="cuda")
    us = {"eval_jac": timed(torch, stream, lambda: c.eval_jac_dev(Zd, dd, vd), a)}
    k_jac = c.get_option("last_kernel")
    us["eval"] = timed(torch, stream, lambda: c.eval_dev(Zd, dd), a)
    k_eval = c.get_option("last_kernel")
    n_cu = c.get_option("n_cu")
    nbytes = 8 * (c.n_rows + c.jac_nnz)
    c.close()
    del vd
    # comparator 1: the Pade order-10 launch of the same system
    c = pa.integrators._PclContext(pade_order=10, large_full=True, **base)
    c.set_stream(stream.cuda_stream)
    vp = torch.empty(c.jac_nnz, dtype=torch.float64, device="cuda")
    pade_us = timed(torch, stream, lambda: c.eval_jac_dev(Zd, dd, vp), a)
    del vp
    # comparator 2: the rollout's propagator launch on that context
    c.set_option("large_rollout_stage", 1)
    xo = torch.empty(N * xd, dtype=torch.float64, device="cuda")
    expm_us = timed(torch, stream, lambda: c.rollout_dev(Zd, xo), a)
    c.close()
    predicted = expm_us * (n + cols * (1 + 2 * m)) / n
    # comparator 3: scipy on the host
    t0 = time.perf_counter()
    scipy_values(Z, lay, G0, Gj)
    t_sp = time.perf_counter() - t0
    P = le.plan(n, cols, m, items=N - 1, n_cu=n_cu)
    ratio = us["eval_jac"] / predicted
    return {"d": d, "n": n, "state_cols": cols, "m": m, "N": N, "substeps_min_max": [int(min(sp)), int(max(sp))], "last_kernel": [k_jac, k_eval], "launch_us": us,
            "launches": a.launches, "warmup": a.warmup, "bytes_stored": nbytes, "GB_per_s_stored": round(nbytes / us["eval_jac"] * 1e-3, 1),
            "products_in_panel_passes": round(18 * max(sp) * (n + cols * (1 + 2 * m)) / n, 2),
            "plan": {"workgroups_per_interval": P["U"], "threads": P["threads"], "lds_bytes": P["bytes"], "state_columns_per_workgroup": P["nc"], "column_slices": P["sx"],
                     "drive_groups": P["ngrp"], "drives_per_group": P["mg"], "columns_of_E_per_workgroup": P["npc"]},
            "comparators": {"pade10_jac_us": pade_us, "rollout_expm_us": expm_us, "predicted_us": round(predicted, 2), "measured_over_predicted": round(ratio, 3),
                            "misses": "slower than predicted" if ratio > 1 else "faster than predicted", "scipy_ms": round(1e3 * t_sp, 1), "scipy_threads": a.threads}}  # fmt: skip


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--N", type=int, default=100)
    ap.add_argument("--cavity-levels", default="12,15")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "large_exp_bench.json"))
    a = ap.parse_args()
    for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
        os.environ[v] = str(a.threads)

    import torch

    import bench_large as bl
    import large_exp_cases as le
    import piccolo_jl_amd as pa
    from oracle import pade_oracle as po

    torch.set_num_threads(a.threads)
    rng = np.random.default_rng(2027)
    out = {"system": "dispersive qubit-cavity, 4 transmon levels x cavity levels, four drives (bench/bench_large.py)", "device": torch.cuda.get_device_name(0), "cases": []}
    for cl in [int(s) for s in a.cavity_levels.split(",")]:
        d = bl.QUBIT_LEVELS * cl
        H0, Hs = bl.qubit_cavity(cl)
        G0, Gj = bl.iso_generator(H0), np.array([bl.iso_generator(H) for H in Hs])
        for cols in (1, d):
            r = measure(torch, pa, po, le, bl, G0, Gj, d, cols, a, rng)
            out["cases"].append(r)
            print("d %d cols %d: eval_jac %.1f us (predicted %.1f), eval %.1f us, s' %s" % (d, cols, r["launch_us"]["eval_jac"], r["comparators"]["predicted_us"],
                                                                                            r["launch_us"]["eval"], r["substeps_min_max"]), file=sys.stderr, flush=True)  # fmt: skip
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
