"""Measurement of the Hessian of the Lagrangian of large variational contexts (PCL_BATCH_VARIATIONAL | PCL_LARGE_N | PCL_LARGE_VAR with option
large_var_hess; pcl_kernel_var_large_hess.hpp) on the dispersive qubit-cavity system of bench/bench_var_large.py (4 transmon levels x 12 or 15
cavity levels: generator dimension n = 96 and 120, four drives; H_var_1 = a'a, H_var_2 = b'b, scales 1).  States: one ket and the unitary
(d columns).  N = 100 knots, Pade orders 4 and 10, v = 1 and 2.

Per case three launches are timed ALTERNATELY in one process, by HIP events on the launch stream, the median of --launches launches after
--warmup:
  hessian      pcl_hess_dev of the variational context
  jacobian     the residual + Jacobian launch of the same context
  plain        pcl_hess_dev of a plain PCL_LARGE_N context with large_hess on the same drift and drives (component 0 of the same knots)
Writes ONE JSON document (--out, default profiles/var_large_hess_bench.json) and prints it as one line; per case:
  plan            the Python restatement of var_large_hess_plan (tests/var_large_hess_cases.py): workgroups per interval, slices, groups, LDS bytes
  launch_us       the three launches
  ratio_to_plain  hessian / plain, beside component_chains = 1 + 2 v -- the component chains the passes run against the plain launch's one: a
                  PREDICTION, not a gate
  ratio_to_jacobian
  max_rel_err     against the float64 lifted oracle (oracle/pade_oracle.py through tests/variational_truth.py), the ket cases
There is no threshold: nothing at these sizes was measured before, and no earlier commit can run them.

    python bench/bench_var_large_hess.py [--launches 50] [--warmup 5] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "bench"))


def median_us(pairs):
    return round(float(np.median([e0.elapsed_time(e1) * 1e3 for e0, e1 in pairs])), 2)


def measure(torch, pa, bv, vl, vh, vt, G0, Gj, Gv, d, cols, order, a, rng, check):
    L = pa._lib
    n, m, v, N = 2 * d, len(Gj), len(Gv), a.N
    xdc = n * cols
    Z = bv.trajectory(d, cols, m, v, N, rng)
    cs = vt.VarCase(Z=Z, z_dim=Z.shape[1], N=N, n=n, C=cols, m=m, xo=[b * xdc for b in range(1 + v)], u_off=(1 + v) * xdc + 2, dt_off=(1 + v) * xdc,
                    G0=G0, Gv=list(Gv), Gj=Gj)  # fmt: skip
    stream = torch.cuda.current_stream()
    cv = pa.integrators._PclContext(**vl.context_args(cs, order, batch_mode=L.PCL_BATCH_VARIATIONAL, large_generator=True, large_variational=True,
                                                      large_var_hessian=True))  # fmt: skip
    cp = pa.integrators._PclContext(d=d, m=m, N=N, z_dim=cs.z_dim, u_off=cs.u_off, dt_off=cs.dt_off, x_offs=[0], G0=G0, Gj=Gj, batch=1,
                                    batch_mode=L.PCL_BATCH_MEMBERS, pade_order=order, state_cols=cols, large_generator=True, large_hessian=True)  # fmt: skip
    for c in (cv, cp):
        c.set_stream(stream.cuda_stream)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64).reshape(-1)).cuda()
    empty = lambda k: torch.empty(k, dtype=torch.float64, device="cuda")
    mu = rng.standard_normal((cs.K, 1 + v, xdc))
    Zd, mud, mu0d = dev(Z), dev(mu), dev(mu[:, 0])
    hv, hp, dd, jv = empty(cv.hess_nnz), empty(cp.hess_nnz), empty(cv.n_rows), empty(cv.jac_nnz)
    jobs = {"hessian": lambda: cv.hess_dev(Zd, mud, hv), "jacobian": lambda: cv.eval_jac_dev(Zd, dd, jv), "plain": lambda: cp.hess_dev(Zd, mu0d, hp)}
    for j in jobs.values():
        j()
    torch.cuda.synchronize()
    out = {"d": d, "n": n, "state_cols": cols, "m": m, "v": v, "N": N, "order": order,
           "last_hess_kernel": {"variational": cv.get_option("last_hess_kernel"), "plain": cp.get_option("last_hess_kernel")}}  # fmt: skip
    if check:  # the float64 lifted oracle, this shape and order
        from oracle import pade_oracle as po

        Zl, lay, G0l, Gjl = vt.lifted(cs)
        ref = po.pade_hessian_values(Zl, vh.lifted_mu(cs, mu), lay, G0l, Gjl, order)[:, vh.value_index(cs)].reshape(-1)
        out["max_rel_err_vs_numpy"] = float(np.abs(hv.cpu().numpy() - ref).max() / np.abs(ref).max())
    for _ in range(a.warmup):
        for j in jobs.values():
            j()
    torch.cuda.synchronize()
    evs = {nm: [] for nm in jobs}
    for _ in range(a.launches):
        for nm, j in jobs.items():  # alternately
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            j()
            e1.record(stream)
            evs[nm].append((e0, e1))
    torch.cuda.synchronize()
    us = {nm: median_us(p) for nm, p in evs.items()}
    P = vh.plan(n, cols, m)
    out.update(launch_us=us, launches=a.launches, warmup=a.warmup, ratio_to_plain=round(us["hessian"] / us["plain"], 3), component_chains=1 + 2 * v,
               ratio_to_jacobian=round(us["hessian"] / us["jacobian"], 3), values={"hessian": cv.hess_nnz, "jacobian": cv.jac_nnz, "plain": cp.hess_nnz},
               plan={"workgroups_per_interval": P["U"], "threads": P["threads"], "lds_bytes": P["bytes"], "slices": P["sx"], "state_columns_per_unit": P["nc"],
                     "drive_groups": P["ngrp"], "drives_per_group": P["mg"], "passes": 1 + v})  # fmt: skip
    cv.close()
    cp.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--N", type=int, default=100)
    ap.add_argument("--cavity-levels", default="12,15")
    ap.add_argument("--orders", default="4,10")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "var_large_hess_bench.json"))
    a = ap.parse_args()
    import torch

    import bench_large as bl
    import bench_var_large as bv
    import piccolo_jl_amd as pa
    import var_large_cases as vl
    import var_large_hess_cases as vh
    import variational_truth as vt

    assert torch.cuda.is_available(), "bench_var_large_hess.py needs a GPU"
    pa.build_library()
    out = {"system": "dispersive qubit-cavity, 4 transmon levels x cavity levels, four drives (bench/bench_large.py); H_var_1 = a'a, H_var_2 = b'b",
           "device": torch.cuda.get_device_name(0),
           "timing": "HIP events on the launch stream, median; the variational Hessian, the same context's residual + Jacobian and a plain large context's Hessian alternate",
           "note": "a single run on one device; no threshold -- component_chains = 1 + 2 v is a prediction of ratio_to_plain, not a gate", "cases": []}  # fmt: skip
    rng = np.random.default_rng(2027)
    for cl in [int(s) for s in a.cavity_levels.split(",")]:
        d = bl.QUBIT_LEVELS * cl
        H0, Hs = bl.qubit_cavity(cl)
        b = np.kron(bl.lower(bl.QUBIT_LEVELS), np.eye(cl))
        c = np.kron(np.eye(bl.QUBIT_LEVELS), bl.lower(cl))
        Hv = [c.conj().T @ c, b.conj().T @ b]
        G0, Gj = bl.iso_generator(H0), np.array([bl.iso_generator(H) for H in Hs])
        for cols in (1, d):
            for v in (1, 2):
                Gv = [bl.iso_generator(H) for H in Hv[:v]]
                for order in [int(s) for s in a.orders.split(",")]:
                    r = measure(torch, pa, bv, vl, vh, vt, G0, Gj, Gv, d, cols, order, a, rng, check=cols == 1)
                    print("n=%d cols=%d v=%d order=%d: hessian %.1f us, jacobian %.1f us, plain hessian %.1f us, ratio %.2f (chains %d)" % (
                        2 * d, cols, v, order, r["launch_us"]["hessian"], r["launch_us"]["jacobian"], r["launch_us"]["plain"], r["ratio_to_plain"],
                        r["component_chains"]), file=sys.stderr)  # fmt: skip
                    out["cases"].append(r)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
