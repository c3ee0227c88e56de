"""Measurement of the Hessian of the Lagrangian of large variational exponential contexts (PCL_BATCH_VARIATIONAL_EXP | PCL_LARGE_N | PCL_LARGE_VAR |
PCL_LARGE_VAR_EXP with option large_var_exp_hess; pcl_kernel_var_large_exp_hess.hpp) on the dispersive qubit-cavity system of
bench/bench_var_large_exp.py (4 transmon levels x 12 or 15 cavity levels: generator dimension n = 96 and 120, four drives; H_var_1 = a'a,
H_var_2 = b'b, scales 1).  States: one ket and the unitary (d columns).  N = 100 knots, every step h_k |G(u_k)|_1 = 0.8: one substep (s' = 1),
v = 1 and 2.

Per case three launches are timed ALTERNATELY in one process, by HIP events on the launch stream, the median of --launches launches after
--warmup:
  hessian      pcl_hess_dev of the variational context (the pass launch and the sum launch behind it)
  jacobian     the residual + Jacobian launch of the same context
  plain        pcl_hess_dev of a plain PCL_LARGE_N | PCL_LARGE_EXP context with large_exp_hess on the same drift and drives (component 0 of the
               same knots)
Writes ONE JSON document (--out, default profiles/var_large_exp_hess_bench.json) and prints it as one line; per case:
  plan            the Python restatements of var_large_exp_hess_plan (tests/var_large_exp_hess_cases.py) and of the plain launch's
                  large_exp_hess_plan (tests/large_exp_hess_cases.py): units per interval (and pass), slices, groups, columns per buffer, LDS bytes
  launch_us       the three launches
  ratio_to_plain  hessian / plain, beside two PREDICTIONS stated before the run, neither a gate: component_chains = 1 + 2 v (the component
                  chains the passes run against the plain launch's one) and pass_ratio, the 16-column matrix-core passes per interval and level
                  of the two plans (pass 0 on one-component column counts, the passes b >= 1 on two-component ones)
  ratio_to_jacobian
  max_rel_err     against scipy on the lifted generator (tests/var_exp_hess_truth.py), the first three knots of the ket cases
There is no threshold: nothing at these sizes was measured on this launch before, and no earlier commit can run it.  One run.

    python bench/bench_var_large_exp_hess.py [--launches 50] [--warmup 5] [--out FILE]
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


def unit_passes(sx, ngrp, nc, Td, To, comps, drives):
    """16-column passes per interval and level of one pass of a plan: diagonal units of comps nc Td columns, off-diagonal ones of comps nc To."""
    npo = ngrp * (ngrp - 1) // 2
    return sx * (ngrp * -(-(comps * nc * (Td if drives else 1)) // 16) + npo * -(-(comps * nc * To) // 16))


def measure(torch, pa, bx, vc, leh, vt, G0, Gj, Gv, d, cols, a, rng, check):
    L = pa._lib
    n, m, v, N = 2 * d, len(Gj), len(Gv), a.N
    xdc = n * cols
    Z = bx.trajectory(G0, Gj, d, cols, v, N, rng)
    cs = vt.VarCase(Z=Z, z_dim=Z.shape[1], N=N, n=n, C=cols, m=m, xo=[b * xdc for b in range(1 + v)], u_off=(1 + v) * xdc + 2, dt_off=(1 + v) * xdc,
                    G0=G0, Gv=list(Gv), Gj=Gj)  # fmt: skip
    stream = torch.cuda.current_stream()
    cv = pa.integrators._PclContext(**vc.context_args(cs, batch_mode=L.PCL_BATCH_VARIATIONAL_EXP, large_generator=True, large_variational=True,
                                                      large_var_exp=True, large_var_exp_hessian=True))  # fmt: skip
    cp = pa.integrators._PclContext(d=d, m=m, N=N, z_dim=cs.z_dim, u_off=cs.u_off, dt_off=cs.dt_off, x_offs=[0], G0=G0, Gj=Gj, batch=1,
                                    batch_mode=L.PCL_BATCH_MEMBERS, pade_order="exp", state_cols=cols, large_generator=True, large_exp=True,
                                    large_exp_hessian=True)  # fmt: skip
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
    out = {"d": d, "n": n, "state_cols": cols, "m": m, "v": v, "N": N, "substeps": 1,
           "last_hess_kernel": {"variational": cv.get_option("last_hess_kernel"), "plain": cp.get_option("last_hess_kernel")}}  # fmt: skip
    if check:  # scipy on the lifted generator, the first three knots
        c3 = vt.VarCase(**{**cs.__dict__, "Z": Z[:3], "N": 3})
        ref = vc.truth_values(c3, mu[:2].reshape(-1)).reshape(-1)
        out["max_rel_err_vs_scipy"] = float(np.abs(hv.cpu().numpy()[: ref.size] - ref).max() / np.abs(ref).max())
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
    P, Q = vc.plan(n, cols, m), leh.plan(n, cols, m)
    Td, To = vc.unit_columns(P["mg"], True), vc.unit_columns(P["mg"], False)
    ours = unit_passes(P["sx"], P["ngrp"], P["nc"], Td, To, 1, m > 0) + v * unit_passes(P["sx"], P["ngrp"], P["nc"], Td, To, 2, m > 0)
    out.update(launch_us=us, launches=a.launches, warmup=a.warmup, ratio_to_plain=round(us["hessian"] / us["plain"], 3),
               predicted={"component_chains": 1 + 2 * v, "passes": ours, "plain_passes": Q["passes"], "pass_ratio": round(ours / Q["passes"], 3)},
               ratio_to_jacobian=round(us["hessian"] / us["jacobian"], 3), values={"hessian": cv.hess_nnz, "jacobian": cv.jac_nnz, "plain": cp.hess_nnz},
               plan={"units_per_interval_and_pass": P["U"], "passes": 1 + v, "threads": P["threads"], "lds_bytes": P["bytes"], "slices": P["sx"],
                     "state_columns_per_unit": P["nc"], "drive_groups": P["ngrp"], "drives_per_group": P["mg"], "columns_per_buffer": P["W"]},
               plain_plan={"units_per_interval": Q["U"], "lds_bytes": Q["bytes"], "slices": Q["sx"], "state_columns_per_unit": Q["nc"],
                           "drive_groups": Q["ngrp"], "drives_per_group": Q["mg"], "columns_per_buffer": Q["W"]})  # fmt: skip
    cv.close()
    cp.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--N", type=int, default=100)
    ap.add_argument("--cavity-levels", default="12,15")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "var_large_exp_hess_bench.json"))
    a = ap.parse_args()
    import torch

    import bench_large as bl
    import bench_var_large_exp as bx
    import large_exp_hess_cases as leh
    import piccolo_jl_amd as pa
    import var_large_exp_hess_cases as vc
    import variational_truth as vt

    assert torch.cuda.is_available(), "bench_var_large_exp_hess.py needs a GPU"
    pa.build_library()
    out = {"system": "dispersive qubit-cavity, 4 transmon levels x cavity levels, four drives (bench/bench_large.py); H_var_1 = a'a, H_var_2 = b'b; every step h |G|_1 = 0.8 (one substep)",
           "device": torch.cuda.get_device_name(0),
           "timing": "HIP events on the launch stream, median; the variational Hessian, the same context's residual + Jacobian and a plain large exponential context's Hessian alternate",
           "note": "a single run on one device; no threshold -- component_chains = 1 + 2 v and pass_ratio are predictions of ratio_to_plain, not gates", "cases": []}  # fmt: skip
    rng = np.random.default_rng(2028)
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
                r = measure(torch, pa, bx, vc, leh, vt, G0, Gj, Gv, d, cols, a, rng, check=cols == 1)
                print("n=%d cols=%d v=%d: hessian %.1f us, jacobian %.1f us, plain hessian %.1f us, ratio %.2f (chains %d, passes %.2f)" % (
                    2 * d, cols, v, r["launch_us"]["hessian"], r["launch_us"]["jacobian"], r["launch_us"]["plain"], r["ratio_to_plain"],
                    r["predicted"]["component_chains"], r["predicted"]["pass_ratio"]), file=sys.stderr)  # fmt: skip
                out["cases"].append(r)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
