"""Measurement of the option exp_full of the exponential mode (pcl_desc.pade_order = PCL_ORDER_EXP) at BASELINE config 3 (d = 27, m = 6, N = 100).

Prints ONE JSON line:
  host       pcl_eval_jac into a pageable host array on ONE context with exp_full = 0 (full values over PCIe: the behaviour without the option) and
             exp_full = 1 (compact values over PCIe, expanded by the host's threads), timed alternately by the wall clock (the call is synchronous);
             evaluations per second from the median call, the bytes that cross PCIe (from shapes), and whether the two deliver the same bits.
  payload    HIP events, alternately in one run: pcl_eval_jac_dev alone, pcl_eval_jac_dev + pcl_merit_grad_dev, the fused pcl_eval_jac_merit_dev, and
             the adjoint launch (vals = NULL); medians in microseconds and each route's ratio to pcl_eval_jac_dev alone.
  untouched  pcl_eval_jac_dev and pcl_eval_dev with exp_full = 0 (what bench/bench_exp.py measures), for the comparison with the parent commit.

    python bench/bench_exp_full.py [--launches 100] [--warmup 10] [--host-calls 20] [--host-threads 0]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--host-calls", type=int, default=20)
    ap.add_argument("--host-threads", type=int, default=0)
    ap.add_argument("--N", type=int, default=100)
    a = ap.parse_args()

    import torch

    import piccolo_jl_amd as pa
    from oracle import pade_oracle as po

    so = po.config_system(3)
    Z, lay = po.synthetic_trajectory(so, a.N, seed=7)
    G0, Gj = so.G_drift, np.array(so.G_drives)
    stream = torch.cuda.current_stream()
    c = pa.integrators._PclContext(d=lay.d, m=lay.m, N=lay.N, z_dim=lay.z_dim, u_off=lay.u_off, dt_off=lay.dt_off, x_offs=[lay.x_off], G0=G0, Gj=Gj, batch=1,
                                   batch_mode=pa._lib.PCL_BATCH_MEMBERS, pade_order=pa._lib.PCL_ORDER_EXP, exp_full=True)  # fmt: skip
    out = {"config": 3, "d": lay.d, "m": lay.m, "N": lay.N, "launches": a.launches}

    # ---- host-delivered evaluations ------------------------------------------------------------------------------------------------------
    Zh = Z.reshape(-1).copy()
    c.set_option("host_threads", a.host_threads)
    res, ts = {}, {0: [], 1: []}
    for rep in range(a.host_calls + 3):
        for opt in (0, 1):
            c.set_option("exp_full", opt)
            d, v = np.empty(c.n_rows), np.empty(c.jac_nnz)
            t0 = time.perf_counter()
            c.eval_jac(Zh, d, v)
            t = time.perf_counter() - t0
            if rep >= 3:  # (the first calls allocate the staging buffers and start the thread pool)
                ts[opt].append(t)
            res[opt] = (d, v, c.get_option("last_kernel"))
    c.set_option("exp_full", 1)
    z8, r8 = 8 * c.z_len, 8 * c.n_rows
    host = {"host_threads": c.get_option("host_threads"), "calls": a.host_calls, "same_bits": bool(np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]))}
    for opt, nv in ((0, c.jac_nnz), (1, c.compact_nnz)):
        med = float(np.median(ts[opt]))
        host["exp_full_%d" % opt] = {"last_kernel": res[opt][2], "median_call_ms": round(1e3 * med, 3), "evaluations_per_s": round(1.0 / med, 1),
                                     "bytes_over_pcie": int(z8 + r8 + 8 * nv)}  # fmt: skip
    host["speedup"] = round(host["exp_full_1"]["evaluations_per_s"] / host["exp_full_0"]["evaluations_per_s"], 2)
    out["host"] = host

    # ---- payload routes -------------------------------------------------------------------------------------------------------------------
    c.set_stream(stream.cuda_stream)
    Zd = torch.from_numpy(Zh).cuda()
    lam = torch.from_numpy(np.random.default_rng(5).standard_normal(c.n_rows)).cuda()
    dd = torch.empty(c.n_rows, dtype=torch.float64, device="cuda")
    vd = torch.empty(c.jac_nnz, dtype=torch.float64, device="cuda")
    length, _ = c.merit_grad_len()
    od = torch.empty(length, dtype=torch.float64, device="cuda")

    def two_calls():
        c.eval_jac_dev(Zd, dd, vd)
        c.merit_grad_dev(dd, lam, vd, od)

    jobs = {
        "eval_jac_us": lambda: c.eval_jac_dev(Zd, dd, vd),
        "eval_jac_plus_merit_grad_us": two_calls,
        "fused_us": lambda: c.eval_jac_merit_dev(Zd, lam, dd, vd, od),
        "adjoint_us": lambda: c.eval_jac_merit_dev(Zd, lam, dd, None, od),
        "eval_us": lambda: c.eval_dev(Zd, dd),
    }
    outs = {}
    for nm, j in jobs.items():
        j()
        torch.cuda.synchronize()
        outs[nm] = od.cpu().numpy().copy()
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
    pay = {nm: round(float(np.median([e0.elapsed_time(e1) * 1e3 for e0, e1 in v])), 2) for nm, v in evs.items()}
    for nm in ("eval_jac_plus_merit_grad_us", "fused_us", "adjoint_us"):
        pay[nm.replace("_us", "_over_eval_jac")] = round(pay[nm] / pay["eval_jac_us"], 3)
    ref = outs["eval_jac_plus_merit_grad_us"]
    pay["routes_max_rel_dev"] = float(max(np.abs(outs[nm] - ref).max() for nm in ("fused_us", "adjoint_us")) / np.abs(ref).max())
    out["payload"] = pay

    # ---- the untouched path: the option off -------------------------------------------------------------------------------------------------
    c.set_option("exp_full", 0)
    evs = {"eval_jac_us": [], "eval_us": []}
    for _ in range(a.launches):
        for nm in evs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            jobs[nm]()
            e1.record(stream)
            evs[nm].append((e0, e1))
    torch.cuda.synchronize()
    out["untouched"] = {nm: round(float(np.median([e0.elapsed_time(e1) * 1e3 for e0, e1 in v])), 2) for nm, v in evs.items()}
    c.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
