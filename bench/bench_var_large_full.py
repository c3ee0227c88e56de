"""Measurement of the rollout of the stacked state and of the robust-control objective on a large variational context (option large_var_full on
PCL_BATCH_VARIATIONAL | PCL_LARGE_N | PCL_LARGE_VAR; pcl_kernel_var_large_rollout.hpp, pcl_host_robust.hpp) on the dispersive qubit-cavity
system of bench/bench_large.py and bench/bench_var_large.py (4 transmon levels x 12 or 15 cavity levels: generator dimension n = 96 and 120,
four drives; H_var_1 = a'a, H_var_2 = b'b, scales 1).  States: one ket and the unitary (d columns); v = 1 and 2; N = 100 knots; dt = 0.05 ns,
where every interval takes s' = 1 substep (asserted from the rule ceil(|h| |G|_1)).

Per case the rollout of the variational context and the rollout of a plain PCL_LARGE_N context with large_full of the same drift and drives
(component 0 of the same knots) are timed ALTERNATELY in one process, by HIP events on the launch stream: the median of --launches launches
after --warmup.  The ratio stands beside the product-count expectation 1 + 2 v: per Horner level and per chain step the plain rollout forms
one n x n x (columns) product, a variation adds G Vv and Gv_i V (E Xv and L_i X in the chain).  At the unitary sizes the objective (matrix
goal, every sensitivity weight on, one regulariser on the drives: value + gradient, one launch) and its Hessian (1 + v dense triangles) are
timed the same way.  Writes ONE JSON document (--out, default profiles/var_large_full_bench.json) and prints it as one line.
There is no threshold: nothing at these sizes was measured before, and no earlier commit can run them.  No kernel trace is taken: the split
between the propagator launch and the chain launch is not measured.

    python bench/bench_var_large_full.py [--launches 50] [--warmup 5] [--out FILE]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "bench"))


def median_us(pairs):
    return round(float(np.median([e0.elapsed_time(e1) * 1e3 for e0, e1 in pairs])), 2)


def timed(torch, stream, jobs, launches, warmup):
    """{name: median us} of the jobs launched alternately."""
    for _ in range(warmup):
        for j in jobs.values():
            j()
    torch.cuda.synchronize()
    evs = {nm: [] for nm in jobs}
    for _ in range(launches):
        for nm, j in jobs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            j()
            e1.record(stream)
            evs[nm].append((e0, e1))
    torch.cuda.synchronize()
    return {nm: median_us(p) for nm, p in evs.items()}


def measure(torch, pa, vl, vt, bv, G0, Gj, Gv, d, cols, a, rng):
    L = pa._lib
    n, m, v, N = 2 * d, len(Gj), len(Gv), a.N
    xdc = n * cols
    Z = bv.trajectory(d, cols, m, v, N, rng)
    cs = vt.VarCase(Z=Z, z_dim=Z.shape[1], N=N, n=n, C=cols, m=m, xo=[b * xdc for b in range(1 + v)], u_off=(1 + v) * xdc + 2, dt_off=(1 + v) * xdc,
                    G0=G0, Gv=list(Gv), Gj=Gj)  # fmt: skip
    sub = [int(math.ceil(abs(Z[k, cs.dt_off]) * np.abs(G0 + np.tensordot(Z[k, cs.u_off :], Gj, axes=1)).sum(axis=0).max())) for k in range(N - 1)]
    assert set(sub) == {1}, sorted(set(sub))
    stream = torch.cuda.current_stream()
    cv = pa.integrators._PclContext(**vl.context_args(cs, 4, batch_mode=L.PCL_BATCH_VARIATIONAL, large_generator=True, large_variational=True, large_var_full=True))
    cp = pa.integrators._PclContext(d=d, m=m, N=N, z_dim=cs.z_dim, u_off=cs.u_off, dt_off=cs.dt_off, x_offs=[0], G0=G0, Gj=Gj, batch=1,
                                    batch_mode=L.PCL_BATCH_MEMBERS, pade_order=4, state_cols=cols, large_generator=True, large_full=True)  # fmt: skip
    for c in (cv, cp):
        c.set_stream(stream.cuda_stream)
    Zd = torch.from_numpy(Z.reshape(-1).copy()).cuda()
    xv = torch.empty(N * cv.x_dim, dtype=torch.float64, device="cuda")
    xp = torch.empty(N * cp.x_dim, dtype=torch.float64, device="cuda")
    jobs = {"variational": lambda: cv.rollout_dev(Zd, xv), "plain": lambda: cp.rollout_dev(Zd, xp)}
    for j in jobs.values():
        j()
    torch.cuda.synchronize()
    got = xv.cpu().numpy().reshape(N, 1 + v, xdc)
    out = {"d": d, "n": n, "state_cols": cols, "m": m, "v": v, "N": N, "substeps_per_interval": 1,
           "last_kernel": {"variational": cv.get_option("last_kernel"), "plain": cp.get_option("last_kernel")},
           "component_0_bitwise_equal_to_plain": bool(np.array_equal(got[:, 0], xp.cpu().numpy().reshape(N, xdc)))}  # fmt: skip
    us = timed(torch, stream, jobs, a.launches, a.warmup)
    out.update(rollout_us=us, launches=a.launches, warmup=a.warmup, run="single run of this script: the medians were not repeated",
               ratio_to_plain=round(us["variational"] / us["plain"], 3), product_count_expectation=1 + 2 * v)
    if cols > 1:  # the objective at the unitary sizes: value + gradient, and the Hessian's 1 + v triangles
        Q, R = np.linalg.qr(rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d)))
        cv.set_goal(np.concatenate([np.concatenate([Q[:, c].real, Q[:, c].imag]) for c in range(d)]))
        cv.set_weights(np.array([1.0, 0.3, 0.7])[: 1 + v])
        cv.add_regularizer(cs.u_off, m, 0.1, 2)
        rows, _ = cv.objective_hess_structure()
        val = torch.empty(1, dtype=torch.float64, device="cuda")
        grad = torch.empty(Z.size, dtype=torch.float64, device="cuda")
        hv = torch.empty(rows.size, dtype=torch.float64, device="cuda")
        ojobs = {"value_and_gradient": lambda: cv.objective_dev(Zd, 100.0, val, grad), "hessian": lambda: cv.objective_hess_dev(Zd, 100.0, 1.0, hv)}
        for j in ojobs.values():
            j()
        torch.cuda.synchronize()
        ous = timed(torch, stream, ojobs, a.launches, a.warmup)
        out["objective_us"] = ous
        out["hessian_values"] = int(rows.size)
        out["hessian_stored_GB_per_second"] = round(8 * rows.size / ous["hessian"] * 1e-3, 1)
        del hv
    cv.close()
    cp.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--N", type=int, default=100)
    ap.add_argument("--cavity-levels", default="12,15")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "var_large_full_bench.json"))
    a = ap.parse_args()
    import torch

    import bench_large as bl
    import bench_var_large as bv
    import piccolo_jl_amd as pa
    import var_large_cases as vl
    import variational_truth as vt

    assert torch.cuda.is_available(), "bench_var_large_full.py needs a GPU"
    pa.build_library()
    out = {"system": "dispersive qubit-cavity, 4 transmon levels x cavity levels, four drives (bench/bench_large.py); H_var_1 = a'a, H_var_2 = b'b",
           "device": torch.cuda.get_device_name(0),
           "timing": "HIP events on the launch stream, median; the variational and the plain rollout alternate, so do the objective and its Hessian",
           "bounds": "ratio_to_plain is measured; 1 + 2 v is the count of matrix products per Horner level and chain step, supposed, not a measured bound; "
                     "the split between the propagator launch and the chain launch was not measured (no kernel trace)",
           "cases": []}  # fmt: skip
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
                r = measure(torch, pa, vl, vt, bv, G0, Gj, [bl.iso_generator(H) for H in Hv[:v]], d, cols, a, rng)
                print("n=%d cols=%d v=%d: rollout %.1f us, plain %.1f us, ratio %.2f (1 + 2v = %d)%s" % (
                    2 * d, cols, v, r["rollout_us"]["variational"], r["rollout_us"]["plain"], r["ratio_to_plain"], 1 + 2 * v,
                    "" if cols == 1 else "; objective %.1f us, Hessian %.1f us" % (r["objective_us"]["value_and_gradient"], r["objective_us"]["hessian"])), file=sys.stderr)  # fmt: skip
                out["cases"].append(r)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
