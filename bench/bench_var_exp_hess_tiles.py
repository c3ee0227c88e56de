"""Measurement of the variational exponential Hessian with four of the octuple chain's tiles in a device workspace (option
var_exp_hess_tiles on a PCL_BATCH_VARIATIONAL_EXP context; pcl_kernel_var_exp_hess_tiles.hpp), v = 1, N = 100 knots:

    a   the cost of the workspace homes alone: one transmon with 22 levels (n = 44, where both plans run), var_exp_hess_tiles = 2 beside
        var_exp_hess_tiles = 0 on a second context -- the same arithmetic and the same bits (checked), the baseline is the nine-tile kernel
    b   config 3 (three 3-level transmons, d = 27, n = 54, m = 6) with var_exp_hess_tiles = 1, ket and unitary
    c   one transmon with 31 levels (n = 62, the smallest LDS margin), the same

Per part one process and one entry in --out (the file is read, the part's entry replaced, and written back, so the parts can run as separate
commands, each under a time limit of its own).  In b and c the new launch stands next to the context's own fused residual + Jacobian launch
and pcl_hess_dev of a plain exponential context (option exp_hess) over the state component, on the same trajectory buffer.  HIP events,
warm-up, then `--launches` launches, all alternating in one process, medians.

    python bench/bench_var_exp_hess_tiles.py --part a|b|c [--launches 200] [--warmup 20] [--N 100] [--out profiles/var_exp_hess_tiles_bench_line.json]
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
    ap.add_argument("--part", choices=["a", "b", "c"], required=True)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--N", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "var_exp_hess_tiles_bench_line.json"))
    a = ap.parse_args()

    import torch

    import piccolo_jl_amd as pa
    import var_exp_cases as cases

    L = pa._lib
    stream = torch.cuda.current_stream()

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

    def var_ctx(case, tiles):
        c = ctx(d=case.n // 2, m=case.m, N=case.N, z_dim=case.z_dim, u_off=case.u_off, dt_off=case.dt_off, x_offs=case.xo,
                G0=np.concatenate([case.G0[None], np.array(case.Gv)]), Gj=case.Gj, batch=1 + case.v, batch_mode=L.PCL_BATCH_VARIATIONAL_EXP,
                per_member_G0=True, pade_order="exp", state_cols=case.C)  # fmt: skip
        c.set_option("var_exp_hess_tiles", tiles)
        c.set_option("var_exp_hess", 1)
        return c

    def run(jobs):
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
        return [round(us(t), 2) for t in ts]

    def squarings(case):
        sq = []
        for k in range(case.K):
            G = case.G0 + np.tensordot(case.Z[k, case.u_off : case.u_off + case.m], case.Gj, axes=1)
            theta, s = abs(case.Z[k, case.dt_off]) * np.abs(G).sum(axis=0).max(), 0
            while theta > 0.25 and s < 60:
                theta, s = theta / 2, s + 1
            sq.append(s)
        return [min(sq), max(sq)]

    make = {"a": lambda ket: cases.transmon(22, N=a.N, ket=ket)[3], "b": lambda ket: cases.config3(1, N=a.N, ket=ket)[3],
            "c": lambda ket: cases.transmon(31, N=a.N, ket=ket)[3]}[a.part]  # fmt: skip
    ck, cu = make(True), make(False)
    n, m = ck.n, ck.m
    Zk, Zu = torch.from_numpy(ck.Z.reshape(-1).copy()).cuda(), torch.from_numpy(cu.Z.reshape(-1).copy()).cuda()
    rng = np.random.default_rng(5)
    e = {"part": a.part, "system": {"a": "transmon22", "b": "config3", "c": "transmon31"}[a.part], "n": n, "m": m, "v": 1, "N": ck.N,
         "squarings_min_max": squarings(ck), "octuple_workgroups": ck.K * max(m, 1), "workspace_homes_MB": round(ck.K * max(m, 1) * 4 * n * n * 8 / 1e6, 2)}  # fmt: skip
    buf = lambda k: torch.empty(k, dtype=torch.float64, device="cuda")
    if a.part == "a":
        k0, k2, u0, u2 = var_ctx(ck, 0), var_ctx(ck, 2), var_ctx(cu, 0), var_ctx(cu, 2)
        muk, muu = torch.from_numpy(rng.standard_normal(k0.n_rows)).cuda(), torch.from_numpy(rng.standard_normal(u0.n_rows)).cuda()
        hk0, hk2, hu0, hu2 = buf(k0.hess_nnz), buf(k2.hess_nnz), buf(u0.hess_nnz), buf(u2.hess_nnz)
        t = run([lambda: k0.hess_dev(Zk, muk, hk0), lambda: k2.hess_dev(Zk, muk, hk2), lambda: u0.hess_dev(Zu, muu, hu0), lambda: u2.hess_dev(Zu, muu, hu2)])
        e.update(n_cu=k0.get_option("n_cu"), lds_plan_ket_us=t[0], workspace_plan_ket_us=t[1], lds_plan_unitary_us=t[2], workspace_plan_unitary_us=t[3],
                 workspace_over_lds_ket=round(t[1] / t[0], 3), workspace_over_lds_unitary=round(t[3] / t[2], 3),
                 last_hess_kernel=[k0.get_option("last_hess_kernel"), k2.get_option("last_hess_kernel")],
                 same_bits=bool(torch.equal(hk0, hk2) and torch.equal(hu0, hu2)))  # fmt: skip
        ctxs = [k0, k2, u0, u2]
    else:
        vk, vu = var_ctx(ck, 1), var_ctx(cu, 1)
        muk, muu = torch.from_numpy(rng.standard_normal(vk.n_rows)).cuda(), torch.from_numpy(rng.standard_normal(vu.n_rows)).cuda()
        hk, hu, dk, jk = buf(vk.hess_nnz), buf(vu.hess_nnz), buf(vk.n_rows), buf(vk.jac_nnz)
        pe = ctx(d=n // 2, m=m, N=ck.N, z_dim=ck.z_dim, u_off=ck.u_off, dt_off=ck.dt_off, x_offs=[ck.xo[0]], G0=ck.G0, Gj=ck.Gj, batch=1,
                 batch_mode=L.PCL_BATCH_MEMBERS, pade_order="exp", state_cols=1, exp_hessian=True)  # fmt: skip
        mup, hp = muk[: pe.n_rows].clone(), buf(pe.hess_nnz)
        t = run([lambda: vk.hess_dev(Zk, muk, hk), lambda: vu.hess_dev(Zu, muu, hu), lambda: vk.eval_jac_dev(Zk, dk, jk), lambda: pe.hess_dev(Zk, mup, hp)])
        e.update(n_cu=vk.get_option("n_cu"), var_exp_hess_ket_us=t[0], var_exp_hess_unitary_us=t[1], var_exp_fused_ket_us=t[2], plain_exp_hess_ket_us=t[3],
                 hess_over_fused=round(t[0] / t[2], 2), hess_over_plain_exp_hess=round(t[0] / t[3], 2), last_hess_kernel=vk.get_option("last_hess_kernel"),
                 finite=bool(torch.isfinite(hk).all().item() and torch.isfinite(hu).all().item()))  # fmt: skip
        ctxs = [vk, vu, pe]
    for c in ctxs:
        c.close()
    out = {"launches": a.launches, "warmup": a.warmup, "N": a.N, "library_bytes": os.path.getsize(L.SO_PATH), "entries": []}
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            old = json.load(f)
        out["entries"] = [x for x in old.get("entries", []) if x.get("part") != a.part]
    out["entries"] = sorted(out["entries"] + [e], key=lambda x: x["part"])
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
