"""Measurement of the variational integrators on the exponential constraint (batch_mode PCL_BATCH_VARIATIONAL_EXP) at BASELINE config 3
(d = 27, m = 6, N = 100) and config 2.

Prints ONE JSON line (and writes it to --out): per config the microseconds of pcl_eval_jac_dev (the fused launch: the preparation launch and
the chain kernel) and of pcl_eval_dev (residual only) at v = 1 and v = 2, next to three launches of the same system on the same trajectory
buffer: pcl_hess_dev and pcl_jac_dev of a plain exponential context over the state component (the yardstick: the same chain per workgroup), and
the order-10 fused launch of a Pade variational context (v = 1) -- HIP events, warm-up, then `--launches` launches, all alternating in one
process, medians; the two ratios to the yardstick; and the deviation of the timed run's output from tests/var_exp_truth.py on a short prefix
of the trajectory.

    python bench/bench_var_exp.py [--launches 200] [--warmup 20] [--configs 3,2] [--out profiles/var_exp_bench_line.json]
    python bench/bench_var_exp.py --only 3      the fused and residual launches of one config alone, v = 1 (for a kernel trace)
"""
import argparse
import dataclasses
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
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--N", type=int, default=100)
    ap.add_argument("--configs", type=lambda s: [int(x) for x in s.split(",")], default=[3, 2])
    ap.add_argument("--check-knots", type=int, default=3)
    ap.add_argument("--only", type=int, default=0, help="config: the new launches alone, v = 1 (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "var_exp_bench_line.json"))
    a = ap.parse_args()

    import torch

    import piccolo_jl_amd as pa
    import var_exp_cases as cases
    import var_exp_truth as truth

    L = pa._lib
    stream = torch.cuda.current_stream()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        return e0, e1

    us = lambda evs: float(np.median([e0.elapsed_time(e1) * 1e3 for e0, e1 in evs]))
    out = {"launches": a.launches, "library_bytes": os.path.getsize(L.SO_PATH), "entries": []}
    for cfg in [a.only] if a.only else a.configs:
        build = cases.config3 if cfg == 3 else cases.config2
        case2 = build(2, N=a.N, seed=7)[3]  # v = 2; its first variation and the same knots are the v = 1 problem
        case1 = dataclasses.replace(case2, Gv=case2.Gv[:1], xo=case2.xo[:1 + 1])
        Zd = torch.from_numpy(case2.Z.reshape(-1).copy()).cuda()
        n, C, m = case2.n, case2.C, case2.m

        def var_ctx(case, mode, order):
            c = pa.integrators._PclContext(d=n // 2, m=m, N=case.N, z_dim=case.z_dim, u_off=case.u_off, dt_off=case.dt_off, x_offs=case.xo,
                                           G0=np.concatenate([case.G0[None], np.array(case.Gv)]), Gj=case.Gj, batch=1 + case.v, batch_mode=mode,
                                           per_member_G0=True, pade_order=order, state_cols=C)  # fmt: skip
            c.set_stream(stream.cuda_stream)
            return c

        t0 = time.perf_counter()
        ctxs, jobs, names, keep = [], [], [], {}
        for v, case in ((1, case1), (2, case2)) if not a.only else ((1, case1),):
            c = var_ctx(case, L.PCL_BATCH_VARIATIONAL_EXP, "exp")
            dl = torch.empty(c.n_rows, dtype=torch.float64, device="cuda")
            vl = torch.empty(c.jac_nnz, dtype=torch.float64, device="cuda")
            d2 = torch.empty(c.n_rows, dtype=torch.float64, device="cuda")
            keep[v] = (c, dl, vl, d2)
            ctxs.append(c)
            jobs += [lambda c=c, dl=dl, vl=vl: c.eval_jac_dev(Zd, dl, vl), lambda c=c, d2=d2: c.eval_dev(Zd, d2)]
            names += ["var_exp_fused_v%d_us" % v, "var_exp_residual_v%d_us" % v]
        if not a.only:
            ce = pa.integrators._PclContext(d=n // 2, m=m, N=case2.N, z_dim=case2.z_dim, u_off=case2.u_off, dt_off=case2.dt_off, x_offs=[case2.xo[0]],
                                            G0=case2.G0, Gj=case2.Gj, batch=1, batch_mode=L.PCL_BATCH_MEMBERS, pade_order="exp", state_cols=C,
                                            exp_hessian=True)  # fmt: skip
            ce.set_stream(stream.cuda_stream)
            c10 = var_ctx(case1, L.PCL_BATCH_VARIATIONAL, 10)
            ctxs += [ce, c10]
            mud = torch.from_numpy(np.random.default_rng(5).standard_normal(ce.n_rows)).cuda()
            he = torch.empty(ce.hess_nnz, dtype=torch.float64, device="cuda")
            je = torch.empty(ce.jac_nnz, dtype=torch.float64, device="cuda")
            d10 = torch.empty(c10.n_rows, dtype=torch.float64, device="cuda")
            v10 = torch.empty(c10.jac_nnz, dtype=torch.float64, device="cuda")
            jobs += [lambda: ce.hess_dev(Zd, mud, he), lambda: ce.jac_dev(Zd, je), lambda: c10.eval_jac_dev(Zd, d10, v10)]
            names += ["exp_hess_us", "exp_jac_us", "order10_variational_v1_us"]
        for j in jobs:  # the first launch of every kernel
            j()
        torch.cuda.synchronize()
        first_s = time.perf_counter() - t0
        for _ in range(a.warmup):
            for j in jobs:
                j()
        torch.cuda.synchronize()
        ts = [[] for _ in jobs]
        for _ in range(a.launches):  # alternating: every launch next to its neighbours
            for t, j in zip(ts, jobs):
                t.append(timed(j))
        torch.cuda.synchronize()
        if not a.only:
            e = {"config": cfg, "d": n // 2, "m": m, "N": case2.N, "create_and_first_launches_s": round(first_s, 3)}
            for nm, t in zip(names, ts):
                e[nm] = round(us(t), 2)
            sq = []
            for k in range(case2.K):
                G = case2.G0 + np.tensordot(case2.Z[k, case2.u_off : case2.u_off + m], case2.Gj, axes=1)
                theta, s = abs(case2.Z[k, case2.dt_off]) * np.abs(G).sum(axis=0).max(), 0
                while theta > 0.25 and s < 60:
                    theta, s = theta / 2, s + 1
                sq.append(s)
            ml = max(m, 1)
            e.update(squarings_min_max=[min(sq), max(sq)], products_per_workgroup_max=14 * 8 + 9 * max(sq), workgroups_v1=case2.K * ml,
                     workgroups_v2=2 * case2.K * ml, n_cu=keep[1][0].get_option("n_cu"), values_v1=keep[1][0].jac_nnz, values_v2=keep[2][0].jac_nnz,
                     fused_v1_over_exp_hess=round(e["var_exp_fused_v1_us"] / e["exp_hess_us"], 3),
                     fused_v2_over_exp_hess=round(e["var_exp_fused_v2_us"] / e["exp_hess_us"], 3),
                     fused_v1_over_order10_variational=round(e["var_exp_fused_v1_us"] / e["order10_variational_v1_us"], 2))  # fmt: skip
            if a.check_knots > 1:
                for v, case in ((1, case1), (2, case2)):
                    c, dl, vl, d2 = keep[v]
                    short = dataclasses.replace(case, Z=case.Z[: a.check_knots], N=a.check_knots)
                    tv, td = truth.values(short), truth.residual(short)
                    e["values_max_err_v%d" % v] = float(np.abs(vl.cpu().numpy()[: len(tv)] - tv).max())
                    e["delta_max_err_v%d" % v] = float(np.abs(dl.cpu().numpy()[: len(td)] - td).max())
                    e["values_max_abs_v%d" % v] = float(np.abs(tv).max())
                    e["residual_launch_bitwise_v%d" % v] = bool(torch.equal(dl, d2))
            out["entries"].append(e)
        for c in ctxs:
            c.close()
    if not a.only:
        line = json.dumps(out)
        print(line, flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
