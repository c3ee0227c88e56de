"""Measurement of the option large_exp_reduce of a large exponential context (PCL_LARGE_N | PCL_LARGE_EXP on pade_order = PCL_ORDER_EXP, generator
dimensions 66 .. 128): the compact Jacobian, its device expansion, the merit / reduce payload by its three routes and the host-pointer calls' compact
route, on the dispersive qubit-cavity systems of bench/bench_large.py -- 4 transmon levels x 12 and 15 cavity levels (n = 96 and 120), four drives,
N = 100 knots, s' = 1 substep per interval -- with one ket, five kets and the unitary state (d state columns).

Writes ONE JSON document (--out, default profiles/large_exp_reduce_bench.json) and prints it as one line; per case, by HIP events, the median of
--launches launches after --warmup:
  full_us                pcl_eval_jac_dev: the full-values launch -- the comparator: it is the code every commit before the option had
  full_again_us          the same launch timed once more at the end of the case (the spread of the comparator within the run)
  compact_us             pcl_eval_jac_compact_dev
  compact_expand_us      pcl_eval_jac_compact_dev + pcl_jac_expand_dev
  fused_payload_us       pcl_eval_jac_merit_dev with values (the full-values launch with the payload's partial sums, then the finish launch)
  full_plus_merit_us     pcl_eval_jac_dev + pcl_merit_grad_dev (the payload from the full values)
  payload_only_us        pcl_eval_jac_merit_dev with vals = NULL (chain units only, then the finish launch)
  plan                   what the launch code chose for the launch with values and for the payload-only launch (the Python restatement of
                         large_exp_plan in tests/large_exp_reduce_cases.py), with each plan's own count: 16-column tile passes x rounds of the grid
  predicted              beside compact_us and payload_only_us: full_us scaled by that count (the compact launch has the plan of the full launch:
                         ratio 1), and measured / predicted
  bytes                  what each launch stores, from the shapes
  host                   pcl_eval_jac into a pageable array with host_path at its default (the compact route where blocks are replicated) and with
                         host_path = 1 (full values over PCIe): evaluations per second over --host-calls calls by the host's clock around the
                         synchronous call, and the bytes that cross PCIe per evaluation
Every new path is compared with full_us of the same run.  There is no threshold: nothing measured these paths before.

    python bench/bench_large_exp_reduce.py [--launches 100] [--warmup 5] [--host-calls 10] [--cavity-levels 12,15] [--out FILE]
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
    return round(float(np.median([e0.elapsed_time(e1) * 1e3 for e0, e1 in evs])), 2)


def host_rate(c, Z, calls):
    c.eval_jac(Z)  # (staging buffers, the thread pool)
    t0 = time.perf_counter()
    for _ in range(calls):
        c.eval_jac(Z)
    return round(calls / (time.perf_counter() - t0), 2)


def plan_row(xc, P, items, n_cu):
    return {"workgroups_per_interval": P["U"], "lds_bytes": P["bytes"], "state_columns_per_workgroup": P["nc"], "column_slices": P["sx"], "drive_groups": P["ngrp"],
            "drives_per_group": P["mg"], "columns_of_E_per_workgroup": P["npc"], "columns_per_buffer": P["W"], "tile_passes_x_rounds": xc.passes(P, items, n_cu)}  # fmt: skip


def measure(torch, pa, po, le, xc, bl, G0, Gj, d, cols, a, rng):
    n, m, N = 2 * d, len(Gj), a.N
    K = N - 1
    Z = bl.trajectory(d, cols, m, N, rng)
    xd = n * cols
    lay = po.Layout(d=d, m=m, N=N, z_dim=xd + 2 + m, x_off=0, u_off=xd + 2, dt_off=xd, cols=cols)
    sp = [le.substeps(lay.dt(Z, k), G0 + np.tensordot(lay.u(Z, k), Gj, axes=1)) for k in range(K)]
    c = pa.integrators._PclContext(d=d, m=m, N=N, z_dim=xd + 2 + m, u_off=xd + 2, dt_off=xd, x_offs=[0], G0=G0, Gj=Gj, batch=1, batch_mode=pa._lib.PCL_BATCH_MEMBERS,
                                   pade_order="exp", state_cols=cols, large_generator=True, large_exp=True, large_exp_reduce=True)  # fmt: skip
    stream = torch.cuda.current_stream()
    c.set_stream(stream.cuda_stream)
    Zd = torch.from_numpy(Z.reshape(-1).copy()).cuda()
    dd = torch.empty(c.n_rows, dtype=torch.float64, device="cuda")
    vd = torch.empty(c.jac_nnz, dtype=torch.float64, device="cuda")
    cd = torch.empty(c.compact_nnz, dtype=torch.float64, device="cuda")
    length, _ = c.merit_grad_len()
    od = torch.empty(length, dtype=torch.float64, device="cuda")

    def compact_expand():
        c.eval_jac_compact_dev(Zd, dd, cd)
        c.jac_expand_dev(cd, vd)

    def full_merit():
        c.eval_jac_dev(Zd, dd, vd)
        c.merit_grad_dev(dd, None, vd, od)

    us = {"full_us": timed(torch, stream, lambda: c.eval_jac_dev(Zd, dd, vd), a)}
    us["compact_us"] = timed(torch, stream, lambda: c.eval_jac_compact_dev(Zd, dd, cd), a)
    kern = {"compact": c.get_option("last_kernel")}
    us["compact_expand_us"] = timed(torch, stream, compact_expand, a)
    us["fused_payload_us"] = timed(torch, stream, lambda: c.eval_jac_merit_dev(Zd, None, dd, vd, od), a)
    kern["fused_payload"] = c.get_option("last_kernel")
    us["full_plus_merit_us"] = timed(torch, stream, full_merit, a)
    us["payload_only_us"] = timed(torch, stream, lambda: c.eval_jac_merit_dev(Zd, None, dd, None, od), a)
    kern["payload_only"] = c.get_option("last_kernel")
    us["full_again_us"] = timed(torch, stream, lambda: c.eval_jac_dev(Zd, dd, vd), a)
    kern["full"] = c.get_option("last_kernel")
    n_cu = c.get_option("n_cu")
    Pf, Pp = xc.plan(n, cols, m, False, items=K, n_cu=n_cu), xc.plan(n, cols, m, True, items=K, n_cu=n_cu)
    out = {"d": d, "n": n, "state_cols": cols, "m": m, "N": N, "substeps_min_max": [int(min(sp)), int(max(sp))], "launches": a.launches, "warmup": a.warmup,
           "last_kernel": kern}  # fmt: skip
    out.update(us)
    out["ratio_to_full"] = {k[:-3]: round(us[k] / us["full_us"], 3) for k in us if k != "full_us"}
    out["plan"] = {"with_values": plan_row(xc, Pf, K, n_cu), "payload_only": plan_row(xc, Pp, K, n_cu)}
    scale = xc.passes(Pp, K, n_cu) / xc.passes(Pf, K, n_cu)
    out["predicted"] = {"compact_us": us["full_us"], "compact_measured_over_predicted": round(us["compact_us"] / us["full_us"], 3),
                        "payload_only_us": round(us["full_us"] * scale, 2), "payload_only_measured_over_predicted": round(us["payload_only_us"] / (us["full_us"] * scale), 3),
                        "chain_columns_of_all": [cols * (1 + m), n + cols * (1 + m)]}  # fmt: skip
    out["bytes"] = {"full_values": 8 * c.jac_nnz, "compact_values": 8 * c.compact_nnz, "delta": 8 * c.n_rows, "payload": 8 * length,
                    "payload_partial_sums": 8 * K * cols * (m + 2)}  # fmt: skip
    # host pointers, a pageable array
    c.set_stream(None)
    Zh = Z.reshape(-1).copy()
    host = {"calls": a.host_calls}
    host["default_evals_per_s"] = host_rate(c, Zh, a.host_calls)
    host["default_last_kernel"] = c.get_option("last_kernel")
    host["default_store_bytes"] = c.get_option("host_store_bytes")
    host["default_pcie_bytes"] = 8 * ((c.compact_nnz if cols > 1 else c.jac_nnz) + c.n_rows + Z.size)
    c.set_option("host_path", 1)
    host["full_evals_per_s"] = host_rate(c, Zh, a.host_calls)
    host["full_last_kernel"] = c.get_option("last_kernel")
    host["full_pcie_bytes"] = 8 * (c.jac_nnz + c.n_rows + Z.size)
    out["host"] = host
    c.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-calls", type=int, default=10)
    ap.add_argument("--N", type=int, default=100)
    ap.add_argument("--cavity-levels", default="12,15")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "large_exp_reduce_bench.json"))
    a = ap.parse_args()

    import torch

    import bench_large as bl
    import large_exp_cases as le
    import large_exp_reduce_cases as xc
    import piccolo_jl_amd as pa
    from oracle import pade_oracle as po

    if not torch.cuda.is_available():
        raise SystemExit("bench_large_exp_reduce.py measures on a GPU; none is available")
    rng = np.random.default_rng(2031)
    out = {"system": "dispersive qubit-cavity, 4 transmon levels x cavity levels, four drives (bench/bench_large.py)", "device": torch.cuda.get_device_name(0),
           "note": "one run, nothing earlier to compare with; every path against full_us of the same run", "cases": []}  # fmt: skip
    for cl in [int(s) for s in a.cavity_levels.split(",")]:
        d = bl.QUBIT_LEVELS * cl
        H0, Hs = bl.qubit_cavity(cl)
        G0, Gj = bl.iso_generator(H0), np.array([bl.iso_generator(H) for H in Hs])
        for cols in (1, 5, d):
            r = measure(torch, pa, po, le, xc, bl, G0, Gj, d, cols, a, rng)
            out["cases"].append(r)
            print("d %d cols %d: full %.1f (again %.1f) us, compact %.1f, + expansion %.1f, fused payload %.1f, full + merit %.1f, payload only %.1f (predicted %.1f); "
                  "host default %.1f /s, full %.1f /s" % (d, cols, r["full_us"], r["full_again_us"], r["compact_us"], r["compact_expand_us"], r["fused_payload_us"],
                                                          r["full_plus_merit_us"], r["payload_only_us"], r["predicted"]["payload_only_us"],
                                                          r["host"]["default_evals_per_s"], r["host"]["full_evals_per_s"]), file=sys.stderr, flush=True)  # fmt: skip
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
