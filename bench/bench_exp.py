"""Measurement of the exponential mode (pcl_desc.pade_order = PCL_ORDER_EXP) at BASELINE config 3 (d = 27, m = 6, N = 100) and config 2.

Prints ONE JSON line: per config the microseconds of pcl_eval_jac_dev and pcl_eval_dev on an exponential context (HIP events, warm-up, then
`--launches` launches), timed alternately in one process with an order-10 and an order-4 context of the same system; the bytes the launch writes
(from shapes) and the products per workgroup (14 x 3 + 3 s with the squaring count s the kernel took, recomputed here from theta = |h| |G|_1)
over the kernel's time, next to the f64 matrix peak; and the deviation of the timed run's outputs from the oracle.

    python bench/bench_exp.py [--launches 200] [--warmup 20] [--configs 3,2]
    python bench/bench_exp.py --only 3          the exponential launches of one config alone (for a kernel trace)
    python bench/bench_exp.py --cpu [--threads 16]   the CPU comparator: the reference's algorithm in C (oracle/expv_ref.c), no device
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

F64_MATRIX_PEAK = 78.6e12  # MI355X, flop/s


def case(cfg, N):
    from oracle import pade_oracle as po

    so = po.config_system(cfg)
    Z, lay = po.synthetic_trajectory(so, N, seed=7)
    return lay, so.G_drift, np.array(so.G_drives), Z


def squarings(lay, G0, Gj, Z):
    out = []
    for k in range(lay.K):
        G = G0 + np.tensordot(lay.u(Z, k), Gj, axes=1)
        theta, s = abs(lay.dt(Z, k)) * np.abs(G).sum(axis=0).max(), 0
        while theta > 0.25 and s < 60:
            theta *= 0.5
            s += 1
        out.append(s)
    return out


def cpu(a):
    from oracle import ref_lib

    out = {"cpu_comparator": "oracle/expv_ref.c (the reference's algorithm: forward-mode duals through expv)", "threads": a.threads, "entries": []}
    for cfg in a.configs:
        lay, G0, Gj, Z = case(cfg, a.N)
        ref_lib.expv_eval_jac(Z, lay, G0, Gj, nthreads=a.threads)
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            ref_lib.expv_eval_jac(Z, lay, G0, Gj, nthreads=a.threads)
            ts.append(time.perf_counter() - t0)
        out["entries"].append({"config": cfg, "N": a.N, "eval_jac_ms": round(1e3 * min(ts), 2)})
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--N", type=int, default=100)
    ap.add_argument("--configs", type=lambda s: [int(x) for x in s.split(",")], default=[3, 2])
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--only", type=int, default=0, help="config: the exponential launches alone (for a kernel trace)")
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    if a.cpu:
        return cpu(a)

    import torch

    import exp_truth
    import piccolo_jl_amd as pa
    from oracle import pade_oracle as po

    stream = torch.cuda.current_stream()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        return e0, e1

    us = lambda evs: float(np.median([e0.elapsed_time(e1) * 1e3 for e0, e1 in evs]))
    out = {"launches": a.launches, "library_bytes": os.path.getsize(pa._lib.SO_PATH), "entries": []}
    for cfg in ([a.only] if a.only else a.configs):
        lay, G0, Gj, Z = case(cfg, a.N)
        Zd = torch.from_numpy(Z.reshape(-1).copy()).cuda()
        ctxs, bufs = {}, {}
        t0 = time.perf_counter()
        for name, order in (("exp", pa._lib.PCL_ORDER_EXP), ("order10", 10), ("order4", 4)):
            if a.only and name != "exp":
                continue
            c = pa.integrators._PclContext(d=lay.d, m=lay.m, N=lay.N, z_dim=lay.z_dim, u_off=lay.u_off, dt_off=lay.dt_off, x_offs=[lay.x_off], G0=G0, Gj=Gj,
                                           batch=1, batch_mode=pa._lib.PCL_BATCH_MEMBERS, pade_order=order)  # fmt: skip
            c.set_stream(stream.cuda_stream)
            ctxs[name] = c
            bufs[name] = (torch.empty(c.n_rows, dtype=torch.float64, device="cuda"), torch.empty(c.jac_nnz, dtype=torch.float64, device="cuda"))
        jobs, names = [], []
        for name, c in ctxs.items():
            dd, vd = bufs[name]
            jobs += [lambda c=c, dd=dd, vd=vd: c.eval_jac_dev(Zd, dd, vd), lambda c=c, dd=dd: c.eval_dev(Zd, dd)]
            names += [name + "_eval_jac_us", name + "_eval_us"]
        for j in jobs:  # the first launch of every kernel: code objects loaded, pattern-compiled modules fetched
            j()
        torch.cuda.synchronize()
        first_s = time.perf_counter() - t0
        for _ in range(a.warmup):
            for j in jobs:
                j()
        torch.cuda.synchronize()
        if a.only:
            for _ in range(a.launches):
                for j in jobs:
                    j()
            torch.cuda.synchronize()
            for c in ctxs.values():
                c.close()
            continue
        ts = [[] for _ in jobs]
        for _ in range(a.launches):  # alternating: every exponential call next to its Pade counterparts
            for t, j in zip(ts, jobs):
                t.append(timed(j))
        torch.cuda.synchronize()
        e = {"config": cfg, "d": lay.d, "m": lay.m, "N": lay.N, "create_and_first_launches_s": round(first_s, 3)}
        for nm, t in zip(names, ts):
            e[nm] = round(us(t), 2)
        sq = squarings(lay, G0, Gj, Z)
        n, ml = lay.n, max(lay.m, 1)
        prods_wg = [14 * 3 + 3 * s + 3 for s in sq]  # + L X_k, E X_k, G E X_k (n x cols; counted as whole products: an upper bound)
        flop = float(sum(p * 2 * n**3 * ml for p in prods_wg))
        nbytes = 8.0 * (ctxs["exp"].jac_nnz + ctxs["exp"].n_rows)
        tj = e["exp_eval_jac_us"] * 1e-6
        e.update(squarings_min_max=[min(sq), max(sq)], products_per_workgroup_max=max(prods_wg), workgroups=lay.K * ml, jac_values=ctxs["exp"].jac_nnz,
                 pade_jac_values=ctxs["order10"].jac_nnz, bytes_written=nbytes, write_GBps=round(nbytes / tj / 1e9, 1), gflop=round(flop / 1e9, 2),
                 tflops=round(flop / tj / 1e12, 2), f64_matrix_peak_tflops=F64_MATRIX_PEAK / 1e12,
                 exp_over_order10_eval_jac=round(e["exp_eval_jac_us"] / e["order10_eval_jac_us"], 2))  # fmt: skip
        if not a.no_check:
            dd, vd = bufs["exp"]
            d0, v0 = po.exp_residual(Z, lay, G0, Gj).reshape(-1), exp_truth.values(Z, lay, G0, Gj).reshape(-1)
            e["delta_max_err"] = float(np.abs(dd.cpu().numpy() - d0).max())
            e["values_max_err"] = float(np.abs(vd.cpu().numpy() - v0).max())
        out["entries"].append(e)
        for c in ctxs.values():
            c.close()
    if not a.only:
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
