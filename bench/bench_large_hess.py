"""Measurement of the Hessian of the Lagrangian on large contexts (PCL_LARGE_N with option large_hess; pcl_kernel_pade_large_hess.hpp) on the
dispersive qubit-cavity systems of bench/bench_large.py: 4 transmon levels x 12 or 15 cavity levels (d = 48 and 60, generator dimension n = 96
and 120), four drives, one ket and five kets, N = 100 knots, Pade orders 4 and 10.

Writes ONE JSON document (--out, default profiles/large_hess_bench.json) and prints it as one line; per case:
  plan            what the launch code chose: workgroups per interval, state columns and drives per workgroup, threads, LDS bytes (through the
                  Python restatement of large_hess_plan in tests/large_hess_cases.py, the one the CPU tests hold against the table)
  hess            pcl_hess_dev (the chain kernel and the sum kernel behind it) by HIP events: the median of --launches launches after --warmup
  eval_jac        pcl_eval_jac_dev of the SAME context in the same run, interleaved with the Hessian launches: the kernel this option does not
                  touch, the yardstick beside it
  ratio           hess launch_us / eval_jac launch_us
  bytes, flops    stored per launch; dense flops of the formulation: per interval and state column (q - 2) + q (1 + m) products of 2 n^2, times
                  the drive groups' repeats of Z and W (16 x 4 blocks of G without a nonzero are skipped by the kernel and still counted)
  max_rel_err_vs_numpy   the launch against oracle/pade_oracle.py pade_hessian_values, relative to the largest value
There is no threshold: nothing ran these shapes before, and no earlier commit can.

    python bench/bench_large_hess.py [--launches 50] [--warmup 5] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "bench"))


def median_us(pairs):
    return round(float(np.median([e0.elapsed_time(e1) * 1e3 for e0, e1 in pairs])), 2)


def measure(torch, pa, po, hc, bl, G0, Gj, d, cols, order, a, rng):
    n, m, N = 2 * d, len(Gj), a.N
    Z = bl.trajectory(d, cols, m, N, rng)
    xd = n * cols
    lay = po.Layout(d=d, m=m, N=N, z_dim=xd + 2 + m, x_off=0, u_off=xd + 2, dt_off=xd, cols=cols)
    c = pa.integrators._PclContext(d=d, m=m, N=N, z_dim=lay.z_dim, u_off=lay.u_off, dt_off=lay.dt_off, x_offs=[0], G0=G0, Gj=Gj, batch=1,
                                   batch_mode=pa._lib.PCL_BATCH_MEMBERS, pade_order=order, state_cols=cols, large_generator=True, large_hessian=True)  # fmt: skip
    stream = torch.cuda.current_stream()
    c.set_stream(stream.cuda_stream)
    mu = rng.standard_normal(c.n_rows)
    Zd, mud = torch.from_numpy(Z.reshape(-1).copy()).cuda(), torch.from_numpy(mu).cuda()
    dd = torch.empty(c.n_rows, dtype=torch.float64, device="cuda")
    vd = torch.empty(c.jac_nnz, dtype=torch.float64, device="cuda")
    hd = torch.full((c.hess_nnz,), float("nan"), dtype=torch.float64, device="cuda")
    jobs = {"hess": lambda: c.hess_dev(Zd, mud, hd), "eval_jac": lambda: c.eval_jac_dev(Zd, dd, vd)}
    c.hess_dev(Zd, mud, hd)
    torch.cuda.synchronize()
    h_ref = po.pade_hessian_values(Z, mu.reshape(lay.K, -1), lay, G0, Gj, order).reshape(-1)
    err = float(np.abs(hd.cpu().numpy() - h_ref).max() / np.abs(h_ref).max())
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
    p = hc.hess_plan(n, cols, m)
    flops = K * cols * 2 * n * n * (p["ngrp"] * (max(q - 2, 0) + q) + q * m)
    nbytes = 8 * c.hess_nnz
    out = {"d": d, "n": n, "state_cols": cols, "m": m, "N": N, "order": order, "max_rel_err_vs_numpy": err,
           "hess": {"last_hess_kernel": c.get_option("last_hess_kernel"), "launch_us": us["hess"], "launches": a.launches, "warmup": a.warmup,
                    "bytes_stored": nbytes, "flops_dense": flops, "GB_per_s_stored": round(nbytes / us["hess"] * 1e-3, 2),
                    "GFLOP_per_s_dense": round(flops / us["hess"] * 1e-3, 1),
                    "plan": {"workgroups_per_interval": p["U"], "threads": p["threads"], "lds_bytes": p["bytes"], "state_columns_per_workgroup": p["nc"],
                             "drive_groups": p["ngrp"], "drives_per_workgroup": p["mg"]}},
           "eval_jac": {"last_kernel": c.get_option("last_kernel"), "launch_us": us["eval_jac"], "bytes_stored": 8 * (c.n_rows + c.jac_nnz)},
           "ratio_hess_to_eval_jac": round(us["hess"] / us["eval_jac"], 2)}  # fmt: skip
    c.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--N", type=int, default=100)
    ap.add_argument("--cavity-levels", default="12,15")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "large_hess_bench.json"))
    a = ap.parse_args()

    import torch

    import bench_large as bl
    import large_hess_cases as hc
    import piccolo_jl_amd as pa
    from oracle import pade_oracle as po

    if not torch.cuda.is_available():
        raise SystemExit("bench_large_hess.py measures on a GPU; none is available")
    rng = np.random.default_rng(2027)
    out = {"system": "dispersive qubit-cavity, 4 transmon levels x cavity levels, four drives (bench/bench_large.py)", "device": torch.cuda.get_device_name(0),
           "cases": []}  # fmt: skip
    for cl in [int(s) for s in a.cavity_levels.split(",")]:
        d = bl.QUBIT_LEVELS * cl
        H0, Hs = bl.qubit_cavity(cl)
        G0, Gj = bl.iso_generator(H0), np.array([bl.iso_generator(H) for H in Hs])
        for cols in (1, 5):
            for order in (4, 10):
                r = measure(torch, pa, po, hc, bl, G0, Gj, d, cols, order, a, rng)
                out["cases"].append(r)
                print("d %d cols %d order %d: hess %.1f us, eval_jac %.1f us (%.2f x), err %.1e"
                      % (d, cols, order, r["hess"]["launch_us"], r["eval_jac"]["launch_us"], r["ratio_hess_to_eval_jac"], r["max_rel_err_vs_numpy"]), file=sys.stderr, flush=True)  # fmt: skip
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
