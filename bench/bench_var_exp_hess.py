"""Measurement of the Hessian of the Lagrangian of the variational integrators on the exponential constraint (option var_exp_hess on a
PCL_BATCH_VARIATIONAL_EXP context; pcl_kernel_var_exp_hess.hpp), v = 1, N = 100 knots, on

    two 3-level transmons (d = 9, n = 18, m = 4) | one transmon with 15 levels (n = 30, m = 2) | one with 22 levels (n = 44, the LDS boundary)

Prints ONE JSON line (and writes it to --out): per system the microseconds of pcl_hess_dev of the new launch (preparation, quadruple, octuple
and finishing kernels) on the ket problem and on the unitary problem, next to three launches of the same system on the same trajectory
buffer: (a) the context's own fused residual + Jacobian launch, (b) pcl_hess_dev of a plain exponential context (option exp_hess) over the
state component, and (c), where the lifted dimension 2n fits that kernel (<= 62), pcl_hess_dev of a plain PCL_STATE_VECTOR exponential
context on the LIFTED generator over the ket stack [psi; psi_var] -- the same values by the parent's means.  HIP events, warm-up, then
`--launches` launches, all alternating in one process, medians; and the deviation of (c)'s values from the new launch's.

    python bench/bench_var_exp_hess.py [--launches 200] [--warmup 20] [--N 100] [--out profiles/var_exp_hess_bench_line.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--N", type=int, default=100)
    ap.add_argument("--systems", type=lambda s: s.split(","), default=["transmons3x3", "transmon15", "transmon22"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "var_exp_hess_bench_line.json"))
    a = ap.parse_args()

    import torch

    import piccolo_jl_amd as pa
    import var_exp_cases as cases
    import variational_truth as vt
    from oracle import pade_oracle as po

    L = pa._lib
    stream = torch.cuda.current_stream()

    def two_transmons(ket):
        s = po.multi_transmon_system([4.0, 4.1], [0.2, 0.21], [[0, 0.01], [0.01, 0]], levels_per_transmon=3, drive_bounds=0.1)
        return vt.make_case(s, [po.G_of_H(vt.h_var_drift(3, 2)) / 10], N=a.N, seed=2, ket=ket)

    systems = {
        "transmons3x3": two_transmons,
        "transmon15": lambda ket: cases.transmon(15, N=a.N, ket=ket)[3],
        "transmon22": lambda ket: cases.transmon(22, N=a.N, ket=ket)[3],
    }

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        return e0, e1

    us = lambda evs: float(np.median([e0.elapsed_time(e1) * 1e3 for e0, e1 in evs]))

    def ctx(**kw):
        c = pa.integrators._PclContext(**kw)
        c.set_stream(stream.cuda_stream)
        return c

    def var_ctx(case):
        return ctx(d=case.n // 2, m=case.m, N=case.N, z_dim=case.z_dim, u_off=case.u_off, dt_off=case.dt_off, x_offs=case.xo,
                   G0=np.concatenate([case.G0[None], np.array(case.Gv)]), Gj=case.Gj, batch=1 + case.v, batch_mode=L.PCL_BATCH_VARIATIONAL_EXP,
                   per_member_G0=True, pade_order="exp", state_cols=case.C, exp_hessian=True)  # fmt: skip

    out = {"launches": a.launches, "warmup": a.warmup, "N": a.N, "library_bytes": os.path.getsize(L.SO_PATH), "entries": []}
    for name in a.systems:
        ck, cu = systems[name](True), systems[name](False)
        n, m = ck.n, ck.m
        Zk, Zu = torch.from_numpy(ck.Z.reshape(-1).copy()).cuda(), torch.from_numpy(cu.Z.reshape(-1).copy()).cuda()
        rng = np.random.default_rng(5)
        vk, vu = var_ctx(ck), var_ctx(cu)
        muk, muu = torch.from_numpy(rng.standard_normal(vk.n_rows)).cuda(), torch.from_numpy(rng.standard_normal(vu.n_rows)).cuda()
        hk = torch.empty(vk.hess_nnz, dtype=torch.float64, device="cuda")
        hu = torch.empty(vu.hess_nnz, dtype=torch.float64, device="cuda")
        dk, jk = torch.empty(vk.n_rows, dtype=torch.float64, device="cuda"), torch.empty(vk.jac_nnz, dtype=torch.float64, device="cuda")
        pe = ctx(d=n // 2, m=m, N=ck.N, z_dim=ck.z_dim, u_off=ck.u_off, dt_off=ck.dt_off, x_offs=[ck.xo[0]], G0=ck.G0, Gj=ck.Gj, batch=1,
                 batch_mode=L.PCL_BATCH_MEMBERS, pade_order="exp", state_cols=1, exp_hessian=True)  # fmt: skip
        mup = muk[: pe.n_rows].clone()
        hp = torch.empty(pe.hess_nnz, dtype=torch.float64, device="cuda")
        ctxs = [vk, vu, pe]
        jobs = [lambda: vk.hess_dev(Zk, muk, hk), lambda: vu.hess_dev(Zu, muu, hu), lambda: vk.eval_jac_dev(Zk, dk, jk), lambda: pe.hess_dev(Zk, mup, hp)]
        names = ["var_exp_hess_ket_us", "var_exp_hess_unitary_us", "var_exp_fused_ket_us", "plain_exp_hess_ket_us"]
        hl = None
        if 2 * n <= 62 and ck.xo[1] == ck.xo[0] + n:
            _, _, G0l, Gjl = vt.lifted(ck)
            pl = ctx(d=2 * n, m=m, N=ck.N, z_dim=ck.z_dim, u_off=ck.u_off, dt_off=ck.dt_off, x_offs=[ck.xo[0]], G0=G0l, Gj=Gjl, batch=1,
                     batch_mode=L.PCL_BATCH_MEMBERS, pade_order="exp", state_cols=L.PCL_STATE_VECTOR, exp_hessian=True)  # fmt: skip
            hl = torch.empty(pl.hess_nnz, dtype=torch.float64, device="cuda")
            ctxs.append(pl)
            jobs.append(lambda: pl.hess_dev(Zk, muk, hl))
            names.append("lifted_plain_exp_hess_ket_us")
        for j in jobs:  # the first launch of every kernel
            j()
        torch.cuda.synchronize()
        for _ in range(a.warmup):
            for j in jobs:
                j()
        torch.cuda.synchronize()
        ts = [[] for _ in jobs]
        for _ in range(a.launches):  # alternating: every launch next to its neighbours
            for t, j in zip(ts, jobs):
                t.append(timed(j))
        torch.cuda.synchronize()
        e = {"system": name, "n": n, "m": m, "v": 1, "N": ck.N, "n_cu": vk.get_option("n_cu")}
        for nm, t in zip(names, ts):
            e[nm] = round(us(t), 2)
        sq = []
        for k in range(ck.K):
            G = ck.G0 + np.tensordot(ck.Z[k, ck.u_off : ck.u_off + m], ck.Gj, axes=1)
            theta, s = abs(ck.Z[k, ck.dt_off]) * np.abs(G).sum(axis=0).max(), 0
            while theta > 0.25 and s < 60:
                theta, s = theta / 2, s + 1
            sq.append(s)
        e.update(squarings_min_max=[min(sq), max(sq)], octuple_workgroups=ck.K * max(m, 1), quadruple_workgroups=ck.K * max(m, 1),
                 octuple_products_max=14 * 20 + 27 * max(sq), hess_over_fused=round(e["var_exp_hess_ket_us"] / e["var_exp_fused_ket_us"], 2),
                 hess_over_plain_exp_hess=round(e["var_exp_hess_ket_us"] / e["plain_exp_hess_ket_us"], 2))  # fmt: skip
        if hl is not None:
            e["lifted_over_hess"] = round(e["lifted_plain_exp_hess_ket_us"] / e["var_exp_hess_ket_us"], 2)
            e["max_abs_diff_to_lifted"] = float((hk - hl).abs().max().item())
            e["max_abs_value"] = float(hl.abs().max().item())
        out["entries"].append(e)
        for c in ctxs:
            c.close()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
