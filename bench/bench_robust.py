"""Measurement of the robust-control entry points of a variational context (option var_full) at BASELINE config 3 (d = 27, m = 6, N = 100,
variations along the drift frequencies and a transmon's drive operator at scale 10).

Prints ONE JSON line: for v = 1, 2 the microseconds of the variational rollout (HIP events, warm-up, then `--launches` launches), timed
alternately in one process with a plain context's pcl_rollout_dev, the ratio next to the gemm-count expectation 1 + 2 v, the objective value +
gradient and the objective Hessian of the variational context next to those of the plain one, and the deviation of the timed run's outputs from
the lifted oracle rollout and the closed-form objective.

    python bench/bench_robust.py [--launches 50] [--warmup 10] [--only-rollout V]
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
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--N", type=int, default=100)
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--only-rollout", type=int, default=0, help="v: the variational and the plain rollout alone (for a kernel trace)")
    a = ap.parse_args()

    import torch

    import piccolo_jl_amd as pa
    import robust_truth as rt
    from oracle import pade_oracle as po
    from variational_truth import h_var_drift, make_case

    s3 = po.config_system(3)
    Hv_all = [h_var_drift(3, 3), po.lift_operator(po.annihilate(3) + po.annihilate(3).conj().T, 2, [3, 3, 3])]
    stream = torch.cuda.current_stream()
    out = {"config": 3, "d": 27, "m": 6, "N": a.N, "scale": 10.0, "launches": a.launches, "entries": []}
    Q = 100.0

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        return e0, e1

    us = lambda evs: float(np.median([e0.elapsed_time(e1) * 1e3 for e0, e1 in evs]))
    rng = np.random.default_rng(5)
    goal = np.linalg.qr(rng.standard_normal((27, 27)) + 1j * rng.standard_normal((27, 27)))[0]
    for nv in ((a.only_rollout,) if a.only_rollout else (1, 2)):
        case = make_case(s3, [po.G_of_H(h) / 10.0 for h in Hv_all[:nv]], N=a.N, seed=7)
        c, cp = rt.var_context(pa, case), rt.plain_context(pa, case)
        c.set_option("var_full", 1)
        for x in (c, cp):
            x.set_stream(stream.cuda_stream)
            x.set_goal(po.operator_to_iso_vec(goal))
            x.add_regularizer(case.u_off, case.m, 1e-2, 2)
        w = np.array([1.0, 0.5, 0.25])[: nv + 1]
        c.set_weights(w)
        Z = case.Z.reshape(-1)
        Zd = torch.from_numpy(Z.copy()).cuda()
        Xv = torch.empty(case.N * case.xd, dtype=torch.float64, device="cuda")
        Xp = torch.empty(case.N * case.xdc, dtype=torch.float64, device="cuda")
        if a.only_rollout:
            for _ in range(a.warmup + a.launches):
                c.rollout_dev(Zd, Xv)
                cp.rollout_dev(Zd, Xp)
            torch.cuda.synchronize()
            c.close()
            cp.close()
            continue
        val, valp = torch.zeros(1, dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda")
        g, gp = torch.empty(Z.size, dtype=torch.float64, device="cuda"), torch.empty(Z.size, dtype=torch.float64, device="cuda")
        nh, nhp = len(c.objective_hess_structure()[0]), len(cp.objective_hess_structure()[0])
        h, hp = torch.empty(nh, dtype=torch.float64, device="cuda"), torch.empty(nhp, dtype=torch.float64, device="cuda")
        jobs = [lambda: c.rollout_dev(Zd, Xv), lambda: cp.rollout_dev(Zd, Xp), lambda: c.objective_dev(Zd, Q, val, g), lambda: cp.objective_dev(Zd, Q, valp, gp),
                lambda: c.objective_hess_dev(Zd, Q, 1.0, h), lambda: cp.objective_hess_dev(Zd, Q, 1.0, hp)]  # fmt: skip
        for _ in range(a.warmup):
            for j in jobs:
                j()
        torch.cuda.synchronize()
        ts = [[] for _ in jobs]
        for _ in range(a.launches):  # alternating: every variational call next to its plain counterpart
            for t, j in zip(ts, jobs):
                t.append(timed(j))
        torch.cuda.synchronize()
        t = [us(x) for x in ts]
        e = {"v": nv, "rollout_us": round(t[0], 2), "plain_rollout_us": round(t[1], 2), "rollout_ratio": round(t[0] / t[1], 3), "gemm_count_expectation": 1 + 2 * nv,
             "objective_us": round(t[2], 2), "plain_objective_us": round(t[3], 2), "objective_launches": c.get_option("last_objective_launches"),
             "plain_objective_launches": cp.get_option("last_objective_launches"), "objective_hess_us": round(t[4], 2), "plain_objective_hess_us": round(t[5], 2),
             "objective_hess_values": nh, "plain_objective_hess_values": nhp, "objective_hess_GBps": round(8.0 * nh / (t[4] * 1e-6) / 1e9, 1),
             "plain_objective_hess_GBps": round(8.0 * nhp / (t[5] * 1e-6) / 1e9, 1)}  # fmt: skip
        if not a.no_check:  # the timed run's outputs
            T = rt.lifted_rollout(case)
            X = Xv.cpu().numpy().reshape(case.N, case.xd)
            e["rollout_max_rel_err"] = float(np.abs(X - T).max() / np.abs(T).max())
            e["component_0_bitwise_plain"] = bool(np.array_equal(X[:, : case.xdc], Xp.cpu().numpy().reshape(case.N, case.xdc)))
            v_ref, g_ref = rt.objective(case, case.Z, w, Q, goal, None, [(case.u_off, case.m, 1e-2, 2)])
            e["objective_rel_err"] = float(abs(val.item() - v_ref) / max(1.0, abs(v_ref)))
            e["gradient_max_rel_err"] = float(np.abs(g.cpu().numpy() - g_ref.reshape(-1)).max() / np.abs(g_ref).max())
        out["entries"].append(e)
        c.close()
        cp.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
