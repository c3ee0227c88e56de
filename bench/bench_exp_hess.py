"""Measurement of the Hessian of the Lagrangian in the exponential mode (PCL_ORDER_EXP with option exp_hess = 1) at BASELINE config 3
(d = 27, m = 6, N = 100) and config 2.

Prints ONE JSON line: per config the microseconds of pcl_hess_dev on an exponential context (the preparation launch and the chain kernel),
of pcl_jac_dev on the same context and of pcl_hess_dev on an order-10 context of the same system -- HIP events, warm-up, then `--launches`
launches, the three alternating in one process, medians; the products per workgroup (14 x 8 + 9 s with the squaring count s the kernel
took, recomputed here from theta = |h| |G|_1) over the launch's time next to the f64 matrix peak; and the deviation of the timed run's
output from tests/exp_hess_truth.py on the first `--check-intervals` intervals.

    python bench/bench_exp_hess.py [--launches 200] [--warmup 20] [--configs 3,2]
    python bench/bench_exp_hess.py --only 3      the exponential Hessian launches of one config alone (for a kernel trace)
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

from bench_exp import F64_MATRIX_PEAK, case, squarings  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--N", type=int, default=100)
    ap.add_argument("--configs", type=lambda s: [int(x) for x in s.split(",")], default=[3, 2])
    ap.add_argument("--check-intervals", type=int, default=4)
    ap.add_argument("--only", type=int, default=0, help="config: the exponential Hessian launches alone (for a kernel trace)")
    a = ap.parse_args()

    import torch

    import exp_hess_truth
    import piccolo_jl_amd as pa

    stream = torch.cuda.current_stream()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        return e0, e1

    us = lambda evs: float(np.median([e0.elapsed_time(e1) * 1e3 for e0, e1 in evs]))
    out = {"launches": a.launches, "library_bytes": os.path.getsize(pa._lib.SO_PATH), "entries": []}
    for cfg in [a.only] if a.only else a.configs:
        lay, G0, Gj, Z = case(cfg, a.N)
        Zd = torch.from_numpy(Z.reshape(-1).copy()).cuda()
        mu = np.random.default_rng(5).standard_normal(lay.K * lay.x_dim)
        mud = torch.from_numpy(mu).cuda()
        t0 = time.perf_counter()
        mk = lambda order, **kw: pa.integrators._PclContext(d=lay.d, m=lay.m, N=lay.N, z_dim=lay.z_dim, u_off=lay.u_off, dt_off=lay.dt_off, x_offs=[lay.x_off],
                                                            G0=G0, Gj=Gj, batch=1, batch_mode=pa._lib.PCL_BATCH_MEMBERS, pade_order=order, **kw)  # fmt: skip
        ce = mk("exp", exp_hessian=True)
        ce.set_stream(stream.cuda_stream)
        he = torch.empty(ce.hess_nnz, dtype=torch.float64, device="cuda")
        jobs, names, ctxs = [lambda: ce.hess_dev(Zd, mud, he)], ["exp_hess_us"], [ce]
        if not a.only:
            c10 = mk(10)
            c10.set_stream(stream.cuda_stream)
            ctxs.append(c10)
            je = torch.empty(ce.jac_nnz, dtype=torch.float64, device="cuda")
            h10 = torch.empty(c10.hess_nnz, dtype=torch.float64, device="cuda")
            jobs += [lambda: ce.jac_dev(Zd, je), lambda: c10.hess_dev(Zd, mud, h10)]
            names += ["exp_jac_us", "order10_hess_us"]
        for j in jobs:  # the first launch of every kernel: code objects loaded, pattern-compiled modules fetched
            j()
        torch.cuda.synchronize()
        first_s = time.perf_counter() - t0
        for _ in range(a.warmup):
            for j in jobs:
                j()
        torch.cuda.synchronize()
        ts = [[] for _ in jobs]
        for _ in range(a.launches):  # alternating: every exponential Hessian launch next to its two neighbours
            for t, j in zip(ts, jobs):
                t.append(timed(j))
        torch.cuda.synchronize()
        if not a.only:
            e = {"config": cfg, "d": lay.d, "m": lay.m, "N": lay.N, "create_and_first_launches_s": round(first_s, 3)}
            for nm, t in zip(names, ts):
                e[nm] = round(us(t), 2)
            sq = squarings(lay, G0, Gj, Z)
            n, ml = lay.n, max(lay.m, 1)
            prods_wg = [14 * 8 + 9 * s for s in sq]
            flop = float(sum(p * 2 * n**3 * ml for p in prods_wg))
            th = e["exp_hess_us"] * 1e-6
            e.update(squarings_min_max=[min(sq), max(sq)], products_per_workgroup_max=max(prods_wg), workgroups=lay.K * ml, hess_values=ce.hess_nnz,
                     order10_hess_values=c10.hess_nnz, gflop=round(flop / 1e9, 2), tflops=round(flop / th / 1e12, 2), f64_matrix_peak_tflops=F64_MATRIX_PEAK / 1e12,
                     us_per_product=round(e["exp_hess_us"] / max(prods_wg) / max(1, -(-lay.K * ml // ce.get_option("n_cu"))), 2),
                     exp_hess_over_exp_jac=round(e["exp_hess_us"] / e["exp_jac_us"], 2), exp_hess_over_order10_hess=round(e["exp_hess_us"] / e["order10_hess_us"], 2))  # fmt: skip
            if a.check_intervals:
                ks = list(range(min(a.check_intervals, lay.K)))
                per = exp_hess_truth.nnz_per_interval(lay)
                v0 = exp_hess_truth.values(Z, mu, lay, G0, Gj, intervals=ks).reshape(-1)
                e["values_max_err"] = float(np.abs(he.cpu().numpy()[: len(ks) * per] - v0).max())
                e["values_max_abs"] = float(np.abs(v0).max())
            out["entries"].append(e)
        for c in ctxs:
            c.close()
    if not a.only:
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
