"""Measurement of the variational (sensitivity) integrators at BASELINE config 3 (d = 27, m = 6, N = 100, H_var = 2 pi sum_q n_q at scale 10).

Prints ONE JSON line: for v = 1, 2 and Pade orders 4, 10 the microseconds per fused residual + Jacobian evaluation (HIP events, warm-up, then
`--launches` launches), the algorithmic bytes (values, residual, trajectory), the fraction of the 8 TB/s HBM bound, the plain single-trajectory
fused launch timed in the same process alternately with the variational one and the ratio, the Hessian's time, and the largest deviation of
the timed run's outputs from the lifted oracle computation (residual: every interval; Jacobian and Hessian: three intervals).

    python bench/bench_variational.py [--launches 30] [--warmup 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_BPS = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--N", type=int, default=100)
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--only", default="", help="v,order: one case only, the fused launch alone (for counter passes)")
    a = ap.parse_args()

    import scipy.sparse as sp
    import torch

    import piccolo_jl_amd as pa
    from oracle import pade_oracle as po
    from variational_truth import VarCase, h_var_drift, hessian, jacobian, make_case, residual

    s3 = po.config_system(3)
    Hv_all = [h_var_drift(3, 3), po.lift_operator(po.annihilate(3) + po.annihilate(3).conj().T, 2, [3, 3, 3])]
    stream = torch.cuda.current_stream()
    out = {"config": 3, "d": 27, "m": 6, "N": a.N, "scale": 10.0, "launches": a.launches, "entries": []}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        return e0, e1

    only = tuple(int(x) for x in a.only.split(",")) if a.only else None
    for nv in ((only[0],) if only else (1, 2)):
        Hv = Hv_all[:nv]
        case = make_case(s3, [po.G_of_H(h) / 10.0 for h in Hv], N=a.N, seed=7)
        vs = pa.VariationalQuantumSystem(s3.H_drift, list(s3.H_drives), Hv, [0.1] * 6)
        comps = {"Ũ⃗": case.Z[:, : case.xdc].T}
        for i in range(nv):
            comps["Ũ⃗_var%d" % (i + 1)] = case.Z[:, case.xo[i + 1] : case.xo[i + 1] + case.xdc].T
        comps.update({"Δt": case.Z[:, case.dt_off][None], "t": case.Z[:, case.dt_off + 1][None], "u": case.Z[:, case.u_off : case.u_off + 6].T})
        traj = pa.NamedTrajectory(comps, controls=("u", "Δt"), timestep="Δt")
        names = ["Ũ⃗"] + ["Ũ⃗_var%d" % (i + 1) for i in range(nv)]
        for order in ((only[1],) if only else (4, 10)):
            B = pa.VariationalUnitaryIntegrator(vs, traj, names[0], names[1:], "u", scales=[10.0] * nv, pade_order=order)
            plain = pa.HipPadeIntegrator(s3.G_drift, np.array(s3.G_drives), traj, "Ũ⃗", "u", pade_order=order)
            c, cp = B.ctx, plain.ctx
            c.set_stream(stream.cuda_stream)
            cp.set_stream(stream.cuda_stream)
            Zd = torch.from_numpy(traj.datavec.copy()).cuda()
            dd = torch.empty(c.n_rows, dtype=torch.float64, device="cuda")
            vd = torch.empty(c.jac_nnz, dtype=torch.float64, device="cuda")
            ddp = torch.empty(cp.n_rows, dtype=torch.float64, device="cuda")
            vdp = torch.empty(cp.jac_nnz, dtype=torch.float64, device="cuda")
            mu = torch.from_numpy(np.random.default_rng(3).standard_normal(c.n_rows)).cuda()
            hd = torch.empty(c.hess_nnz, dtype=torch.float64, device="cuda")
            if only:  # counter passes: the variational fused launch and nothing else
                for _ in range(a.warmup + a.launches):
                    c.eval_jac_dev(Zd, dd, vd)
                torch.cuda.synchronize()
                B.close()
                plain.close()
                continue
            for _ in range(a.warmup):
                c.eval_jac_dev(Zd, dd, vd)
                cp.eval_jac_dev(Zd, ddp, vdp)
                c.hess_dev(Zd, mu, hd)
            torch.cuda.synchronize()
            tv, tp, th = [], [], []
            for _ in range(a.launches):  # alternating: the variational launch, the plain launch, the Hessian
                tv.append(timed(lambda: c.eval_jac_dev(Zd, dd, vd)))
                tp.append(timed(lambda: cp.eval_jac_dev(Zd, ddp, vdp)))
                th.append(timed(lambda: c.hess_dev(Zd, mu, hd)))
            torch.cuda.synchronize()
            us = lambda evs: float(np.median([e0.elapsed_time(e1) * 1e3 for e0, e1 in evs]))
            t_var, t_plain, t_hess = us(tv), us(tp), us(th)
            byt = 8.0 * (c.jac_nnz + c.n_rows + case.Z.size)
            byt_p = 8.0 * (cp.jac_nnz + cp.n_rows + case.Z.size)
            # the residual-only launch (column role alone, last_kernel 71) and the fused launch over block-workgroup splits
            tr = []
            for _ in range(a.launches):
                tr.append(timed(lambda: c.eval_dev(Zd, dd)))
            torch.cuda.synchronize()
            t_res = us(tr)
            splits = {}
            auto_nb = c.get_option("var_block_wgs")
            for nb in (1, 2, 4, 7, 14, 27):
                c.set_option("var_block_wgs", nb)
                for _ in range(3):
                    c.eval_jac_dev(Zd, dd, vd)
                ts = [timed(lambda: c.eval_jac_dev(Zd, dd, vd)) for _ in range(a.launches)]
                torch.cuda.synchronize()
                splits[str(nb)] = round(us(ts), 2)
            c.set_option("var_block_wgs", 0)
            c.eval_jac_dev(Zd, dd, vd)  # (the outputs checked below: the default split's)
            torch.cuda.synchronize()
            e = {"v": nv, "order": order, "residual_only_us": round(t_res, 2), "fused_us_by_block_wgs": splits, "auto_block_wgs": auto_nb, "us_per_eval": round(t_var, 2), "bytes": int(byt), "frac_of_8TBps": round(byt / (t_var * 1e-6) / HBM_BPS, 3),
                 "plain_us": round(t_plain, 2), "plain_bytes": int(byt_p), "ratio_to_plain": round(t_var / t_plain, 3), "byte_ratio": round(byt / byt_p, 3),
                 "hess_us": round(t_hess, 2), "kernel": c.get_option("last_kernel"), "block_wgs": c.get_option("var_block_wgs"),
                 "col_wgs": c.get_option("var_col_wgs")}  # fmt: skip
            if not a.no_check:  # the timed run's outputs against the lifted computation
                delta, vals, hv = dd.cpu().numpy(), vd.cpu().numpy(), hd.cpu().numpy()
                ref = residual(case, order)
                e["max_rel_err_delta"] = float(np.abs(delta - ref).max() / np.abs(ref).max())
                jper, hper = c.jac_per, c.hess_per
                rows, cols = c.jac_structure()
                hr, hc = c.hess_structure()
                ej = eh = 0.0
                for k in (0, case.K // 2, case.K - 1):
                    sub = VarCase(**{**case.__dict__, "Z": case.Z[k : k + 2], "N": 2})
                    J, _ = jacobian(sub, order)
                    sl = slice(k * jper, (k + 1) * jper)
                    r = rows[sl] - k * c.x_dim
                    cc = cols[sl] - k * case.z_dim
                    D = (sp.csr_matrix((vals[sl], (r, cc)), shape=J.shape) - J).tocoo()
                    ej = max(ej, (np.abs(D.data).max() if D.nnz else 0.0) / np.abs(J.data).max())
                    H, _ = hessian(sub, order, mu.cpu().numpy()[k * c.x_dim : (k + 1) * c.x_dim])
                    sh = slice(k * hper, (k + 1) * hper)
                    Dh = (sp.csr_matrix((hv[sh], (hr[sh] - k * case.z_dim, hc[sh] - k * case.z_dim)), shape=H.shape) - H).tocoo()
                    eh = max(eh, (np.abs(Dh.data).max() if Dh.nnz else 0.0) / np.abs(H.data).max())
                e["max_rel_err_jac_3_intervals"] = float(ej)
                e["max_rel_err_hess_3_intervals"] = float(eh)
            out["entries"].append(e)
            B.close()
            plain.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
