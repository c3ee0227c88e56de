"""Measurement of the Hessian of the Lagrangian of a large exponential context (option large_exp_hess; pcl_kernel_large_exp_hess.hpp) on the
dispersive qubit-cavity systems of bench/bench_large.py: 4 transmon levels x 12 or 15 cavity levels (generator dimension n = 96 and 120), four
drives, N = 100 knots, s' = 1, one ket and the unitary state (state_cols 1 and d).

Writes ONE JSON document (--out, default profiles/large_exp_hess_bench.json) and prints it as one line; per case:
  substeps         s' = ceil(|dt| |G(u_k)|_1) over the intervals (min, max)
  plan             what the launch code chose (the Python restatement of large_exp_hess_plan in tests/large_exp_hess_cases.py): units x threads, LDS bytes
  launch_us        pcl_hess_dev (the chain and the sum kernel) and pcl_eval_jac_dev of the SAME context, interleaved in one run, by HIP events:
                   the median of --launches launches after --warmup warm-up launches each
  column_products  18 s' cols (1 + m + m (m + 1) / 2) for the Hessian launch (and what its drive groups repeat: W per pair of groups, dW per
                   off-diagonal pair), 18 s' (n + cols (1 + m)) for the Jacobian launch; predicted_ratio is their quotient
  measured_ratio   hess_us / eval_jac_us
There is no threshold: nothing ran this launch before.  Not measured: other step counts (the cost is linear in s'), m = 24, batched launches, the
host-pointer call, and the two kernels of the Hessian launch apart.

    python bench/bench_large_exp_hess.py [--launches 50] [--warmup 5] [--out FILE]
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


def measure(torch, pa, po, le, lh, bl, G0, Gj, d, cols, a, rng):
    n, m, N = 2 * d, len(Gj), a.N
    Z = bl.trajectory(d, cols, m, N, rng)
    xd = n * cols
    lay = po.Layout(d=d, m=m, N=N, z_dim=xd + 2 + m, x_off=0, u_off=xd + 2, dt_off=xd, cols=cols)
    stream = torch.cuda.current_stream()
    Zd = torch.from_numpy(Z.reshape(-1).copy()).cuda()
    sp = [le.substeps(lay.dt(Z, k), G0 + np.tensordot(lay.u(Z, k), Gj, axes=1)) for k in range(lay.K)]
    c = pa.integrators._PclContext(d=d, m=m, N=N, z_dim=lay.z_dim, u_off=lay.u_off, dt_off=lay.dt_off, x_offs=[0], G0=G0, Gj=Gj, batch=1,
                                   batch_mode=pa._lib.PCL_BATCH_MEMBERS, state_cols=cols, large_generator=True, pade_order="exp", large_exp=True,
                                   large_exp_hessian=True)  # fmt: skip
    c.set_stream(stream.cuda_stream)
    mud = torch.from_numpy(rng.standard_normal(c.n_rows)).cuda()
    dd = torch.empty(c.n_rows, dtype=torch.float64, device="cuda")
    vd = torch.empty(c.jac_nnz, dtype=torch.float64, device="cuda")
    hd = torch.empty(c.hess_nnz, dtype=torch.float64, device="cuda")
    jobs = {"hess": lambda: c.hess_dev(Zd, mud, hd), "eval_jac": lambda: c.eval_jac_dev(Zd, dd, vd)}
    for _ in range(a.warmup):
        for job in jobs.values():
            job()
    torch.cuda.synchronize()
    evs = {k: [] for k in jobs}
    for _ in range(a.launches):  # interleaved: both launches see the same clocks and the same neighbours
        for k, job in jobs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            job()
            e1.record(stream)
            evs[k].append((e0, e1))
    torch.cuda.synchronize()
    us = {k: round(float(np.median([e0.elapsed_time(e1) * 1e3 for e0, e1 in v])), 2) for k, v in evs.items()}
    kernels = [c.get_option("last_hess_kernel"), c.get_option("last_kernel")]
    n_cu = c.get_option("n_cu")
    c.close()
    P, PJ = lh.plan(n, cols, m), le.plan(n, cols, m, items=N - 1, n_cu=n_cu)
    g, mg = P["ngrp"], P["mg"]
    s = max(sp)
    hess_cols = 18 * s * cols * (1 + m + m * (m + 1) // 2)
    launched = 18 * s * cols * (g * lh.unit_columns(mg, True) + g * (g - 1) // 2 * lh.unit_columns(mg, False))  # (even groups: an upper bound where the last group is short)
    jac_cols = 18 * s * (n + cols * (1 + m))
    return {"d": d, "n": n, "state_cols": cols, "m": m, "N": N, "substeps_min_max": [int(min(sp)), int(max(sp))], "last_hess_kernel_last_kernel": kernels,
            "launch_us": us, "launches": a.launches, "warmup": a.warmup,
            "plan": {"units_per_interval": P["U"], "threads": P["threads"], "lds_bytes": P["bytes"], "state_columns_per_unit": P["nc"], "column_slices": P["sx"],
                     "drive_groups": P["ngrp"], "drives_per_group": P["mg"], "columns_per_buffer": P["W"],
                     "jacobian_units_per_interval": PJ["U"], "jacobian_lds_bytes": PJ["bytes"]},
            "column_products": {"hess": hess_cols, "hess_with_what_groups_repeat": launched, "eval_jac": jac_cols},
            "predicted_ratio": round(hess_cols / jac_cols, 3), "predicted_ratio_with_repeats": round(launched / jac_cols, 3),
            "measured_ratio": round(us["hess"] / us["eval_jac"], 3)}  # fmt: skip


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--N", type=int, default=100)
    ap.add_argument("--cavity-levels", default="12,15")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "large_exp_hess_bench.json"))
    a = ap.parse_args()

    import torch

    import bench_large as bl
    import large_exp_cases as le
    import large_exp_hess_cases as lh
    import piccolo_jl_amd as pa
    from oracle import pade_oracle as po

    rng = np.random.default_rng(2028)
    out = {"system": "dispersive qubit-cavity, 4 transmon levels x cavity levels, four drives (bench/bench_large.py)", "device": torch.cuda.get_device_name(0),
           "not_measured": "other step counts (the cost is linear in s'), m = 24, batched launches, the host-pointer call, the chain and the sum kernel apart",
           "cases": []}  # fmt: skip
    for cl in [int(s) for s in a.cavity_levels.split(",")]:
        d = bl.QUBIT_LEVELS * cl
        H0, Hs = bl.qubit_cavity(cl)
        G0, Gj = bl.iso_generator(H0), np.array([bl.iso_generator(H) for H in Hs])
        for cols in (1, d):
            r = measure(torch, pa, po, le, lh, bl, G0, Gj, d, cols, a, rng)
            out["cases"].append(r)
            print("d %d cols %d: hess %.1f us, eval_jac %.1f us, ratio %.2f (by count %.2f, with repeats %.2f), s' %s"
                  % (d, cols, r["launch_us"]["hess"], r["launch_us"]["eval_jac"], r["measured_ratio"], r["predicted_ratio"], r["predicted_ratio_with_repeats"],
                     r["substeps_min_max"]), file=sys.stderr, flush=True)  # fmt: skip
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
