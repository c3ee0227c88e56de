"""Measurement of the option var_compact of the variational contexts at BASELINE config 3 (d = 27, n = 54, C = 27, m = 6), N = 100, v = 1 (--v 2 for
two variations), at Pade orders 4 and 10 (PCL_BATCH_VARIATIONAL) and on the exponential constraint (PCL_BATCH_VARIATIONAL_EXP).

Writes ONE JSON document (--out, default profiles/var_compact_bench.json) and prints it as one line; per mode:
  bytes      per interval and per evaluation, computed HERE from the shapes: the full values, the compact values, what a host-pointer call moves over
             PCIe on either route (trajectory in, residual and values out) and what the device expansion reads and writes.
  launch     HIP events, alternately in one run after warm-up: the full launch (pcl_eval_jac_dev), the compact launch (pcl_eval_jac_compact_dev)
             and compact launch + device expansion (pcl_jac_expand_dev); medians in microseconds, the ratios to the full launch, and whether
             the expanded values have the bits of the full launch.
  host       pcl_eval_jac into a pageable array on ONE context with host_path 1 (full values over PCIe: the behaviour without the option) and
             host_path 0 (compact values over PCIe, expanded by the host's threads), timed alternately by the wall clock; evaluations per second
             from the median call, and whether the two deliver the same bits.

    python bench/bench_var_compact.py [--launches 50] [--warmup 5] [--host-calls 12] [--host-threads 16] [--out FILE]
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


def byte_counts(n, C, v, m, K, z_dim, expo):
    """Bytes from the shapes (8 per value).  x_dim' = (1 + v) n C; tails x_dim' (m + 1); Pade: (2 + 4 v) C tiles written, 2 + 2 v distinct;
    exponential: (1 + 2 v) C tiles and x_dim' ones written, 1 + v distinct tiles."""
    nn, xd = n * n, (1 + v) * n * C
    tail = xd * (m + 1)
    blocks_full = ((1 + 2 * v) if expo else (2 + 4 * v)) * C * nn
    blocks_comp = ((1 + v) if expo else (2 + 2 * v)) * nn
    full = blocks_full + (xd if expo else 0) + tail
    comp = blocks_comp + tail
    z, r = z_dim * (K + 1), xd * K
    return {
        "per_interval": {"full_blocks": 8 * blocks_full, "distinct_blocks": 8 * blocks_comp, "tails": 8 * tail, "full": 8 * full, "compact": 8 * comp},
        "per_evaluation": {"full": 8 * full * K, "compact": 8 * comp * K, "pcie_full_route": 8 * (z + r + full * K), "pcie_compact_route": 8 * (z + r + comp * K),
                           "device_expansion_read_plus_written": 8 * (comp + full) * K},
    }  # fmt: skip


def median_us(pairs):
    return round(float(np.median([e0.elapsed_time(e1) * 1e3 for e0, e1 in pairs])), 2)


def measure(torch, pa, case, order, a):
    expo = order == "exp"
    c = pa.integrators._PclContext(d=case.n // 2, m=case.m, N=case.N, z_dim=case.z_dim, u_off=case.u_off, dt_off=case.dt_off, x_offs=case.xo,
                                   G0=np.concatenate([case.G0[None], np.array(case.Gv)]), Gj=case.Gj, batch=1 + case.v,
                                   batch_mode=pa._lib.PCL_BATCH_VARIATIONAL_EXP if expo else pa._lib.PCL_BATCH_VARIATIONAL, per_member_G0=True,
                                   pade_order=pa._lib.PCL_ORDER_EXP if expo else order, state_cols=case.C, var_compact=True)  # fmt: skip
    out = {"bytes": byte_counts(case.n, case.C, case.v, case.m, case.K, case.z_dim, expo)}
    assert out["bytes"]["per_interval"]["full"] == 8 * c.jac_per and out["bytes"]["per_interval"]["compact"] == 8 * c.compact_per
    Zh = case.Z.reshape(-1).copy()

    # ---- launches ----------------------------------------------------------------------------------------------------------------------------
    stream = torch.cuda.current_stream()
    c.set_stream(stream.cuda_stream)
    Zd = torch.from_numpy(Zh).cuda()
    dd = torch.empty(c.n_rows, dtype=torch.float64, device="cuda")
    vd = torch.empty(c.jac_nnz, dtype=torch.float64, device="cuda")
    ve = torch.full((c.jac_nnz,), float("nan"), dtype=torch.float64, device="cuda")
    cd = torch.empty(c.compact_nnz, dtype=torch.float64, device="cuda")

    def compact_expand():
        c.eval_jac_compact_dev(Zd, dd, cd)
        c.jac_expand_dev(cd, ve)

    jobs = {"full_us": lambda: c.eval_jac_dev(Zd, dd, vd), "compact_us": lambda: c.eval_jac_compact_dev(Zd, dd, cd), "compact_plus_expand_us": compact_expand,
            "expand_us": lambda: c.jac_expand_dev(cd, ve)}  # fmt: skip
    kern = {}
    for nm, j in jobs.items():
        j()
        kern[nm] = c.get_option("last_kernel")
    torch.cuda.synchronize()
    same = bool(torch.equal(vd.view(torch.int64), ve.view(torch.int64)))
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
    launch = {nm: median_us(v) for nm, v in evs.items()}
    launch["compact_over_full"] = round(launch["compact_us"] / launch["full_us"], 3)
    launch["compact_plus_expand_over_full"] = round(launch["compact_plus_expand_us"] / launch["full_us"], 3)
    launch["last_kernel_full"], launch["last_kernel_compact"] = kern["full_us"], kern["compact_us"]
    launch["expanded_has_the_bits_of_full"] = same
    launch["launches"] = a.launches
    out["launch"] = launch
    c.set_stream(None)
    del vd, ve, cd

    # ---- host-delivered evaluations ------------------------------------------------------------------------------------------------------------
    c.set_option("host_threads", a.host_threads)
    res, ts = {}, {1: [], 0: []}
    d, v = {p: np.empty(c.n_rows) for p in (0, 1)}, {p: np.empty(c.jac_nnz) for p in (0, 1)}  # pageable
    for rep in range(a.host_calls + 2):
        for path in (1, 0):
            c.set_option("host_path", path)
            t0 = time.perf_counter()
            c.eval_jac(Zh, d[path], v[path])
            t = time.perf_counter() - t0
            if rep >= 2:  # (the first calls allocate the staging buffers and start the thread pool)
                ts[path].append(t)
            res[path] = c.get_option("last_kernel")
    host = {"host_threads": c.get_option("host_threads"), "calls": a.host_calls, "host_store_bytes": c.get_option("host_store_bytes"),
            "same_bits": bool(np.array_equal(d[0].view(np.int64), d[1].view(np.int64)) and np.array_equal(v[0].view(np.int64), v[1].view(np.int64)))}  # fmt: skip
    for path, key in ((1, "full_route"), (0, "compact_route")):
        med = float(np.median(ts[path]))
        host[key] = {"host_path": path, "last_kernel": res[path], "median_call_ms": round(1e3 * med, 3), "evaluations_per_s": round(1.0 / med, 2),
                     "bytes_over_pcie": out["bytes"]["per_evaluation"]["pcie_%s" % key]}  # fmt: skip
    host["speedup"] = round(host["compact_route"]["evaluations_per_s"] / host["full_route"]["evaluations_per_s"], 2)
    out["host"] = host
    c.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-calls", type=int, default=12)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--N", type=int, default=100)
    ap.add_argument("--v", type=int, default=1)
    ap.add_argument("--modes", default="4,10,exp")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "var_compact_bench.json"))
    a = ap.parse_args()

    import torch

    import piccolo_jl_amd as pa
    import var_exp_cases

    case = var_exp_cases.config3(a.v, N=a.N)[3]
    out = {"config": 3, "d": case.n // 2, "n": case.n, "C": case.C, "m": case.m, "N": case.N, "v": case.v, "device": torch.cuda.get_device_name(0), "modes": {}}
    # the byte counts at the other variation count too (shapes only: nothing is run for them)
    out["bytes_at_v"] = {str(v): {"pade": byte_counts(case.n, case.C, v, case.m, case.K, (1 + v) * case.n * case.C + 2 + case.m, False),
                                  "exp": byte_counts(case.n, case.C, v, case.m, case.K, (1 + v) * case.n * case.C + 2 + case.m, True)} for v in (1, 2)}  # fmt: skip
    for mode in a.modes.split(","):
        order = "exp" if mode == "exp" else int(mode)
        out["modes"]["exp" if mode == "exp" else "pade_%d" % order] = measure(torch, pa, case, order, a)
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
