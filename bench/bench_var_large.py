"""Measurement of the large variational kernel (contexts created with PCL_BATCH_VARIATIONAL | PCL_LARGE_N | PCL_LARGE_VAR;
pcl_kernel_var_large.hpp) on the dispersive qubit-cavity system of bench/bench_large.py (4 transmon levels x 12 or 15 cavity levels: generator
dimension n = 96 and 120, four drives).  H_var_1 is the cavity number operator a'a (a cavity-frequency error), H_var_2 -- the cases with two
variations -- the transmon number operator b'b; scales 1.  States: one ket and the unitary (d columns).  N = 100 knots, Pade orders 4 and 10.

Per case the residual + Jacobian launch of the variational context and the launch of a plain PCL_LARGE_N context of the same system (component 0
of the same knots) are timed ALTERNATELY in one process, by HIP events on the launch stream: the median of --launches launches after --warmup.
Writes ONE JSON document (--out, default profiles/var_large_bench.json) and prints it as one line; per case:
  plan            what the launch code chose (the Python restatement of var_large_plan in tests/var_large_cases.py, held against the launch
                  code's table by tests/test_var_large_cpu.py): workgroups per interval, chain and panel units, LDS bytes
  launch_us       variational and plain, and their ratio
  bytes_stored    residual and Jacobian values, 8 bytes each; for the unitary cases the block stream (2 + 4v) C n^2 doubles per interval and its
                  share of the HBM bound: bytes / (launch time x 8.0 TB/s, the MI355X's specified peak)
  max_rel_err     against the float64 lifted oracle (oracle/pade_oracle.py through tests/variational_truth.py), one ket case per size
There is no threshold: nothing at these sizes was measured before, and no earlier commit can run them.

    python bench/bench_var_large.py [--launches 50] [--warmup 5] [--out FILE]
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

HBM_PEAK = 8.0e12  # bytes / s (specification)


def trajectory(d, cols, m, v, N, rng):
    """Knots [X | Xv_1 .. | dt | t | u]: normalised random columns, dt = 0.05 ns, |u| ~ 2 pi 0.01."""
    n = 2 * d
    xdc = n * cols
    Z = np.zeros((N, (1 + v) * xdc + 2 + m))
    X = rng.standard_normal((N, (1 + v) * cols, n))
    Z[:, : (1 + v) * xdc] = (X / np.linalg.norm(X, axis=2, keepdims=True)).reshape(N, -1)
    Z[:, (1 + v) * xdc] = 0.05
    Z[:, (1 + v) * xdc + 1] = np.cumsum(Z[:, (1 + v) * xdc])
    Z[:, (1 + v) * xdc + 2 :] = 2.0 * np.pi * 0.01 * rng.standard_normal((N, m))
    return Z


def median_us(pairs):
    return round(float(np.median([e0.elapsed_time(e1) * 1e3 for e0, e1 in pairs])), 2)


def measure(torch, pa, vl, vt, G0, Gj, Gv, d, cols, order, a, rng, check):
    L = pa._lib
    n, m, v, N = 2 * d, len(Gj), len(Gv), a.N
    xdc = n * cols
    Z = trajectory(d, cols, m, v, N, rng)
    cs = vt.VarCase(Z=Z, z_dim=Z.shape[1], N=N, n=n, C=cols, m=m, xo=[b * xdc for b in range(1 + v)], u_off=(1 + v) * xdc + 2, dt_off=(1 + v) * xdc,
                    G0=G0, Gv=list(Gv), Gj=Gj)  # fmt: skip
    stream = torch.cuda.current_stream()
    cv = pa.integrators._PclContext(**vl.context_args(cs, order, batch_mode=L.PCL_BATCH_VARIATIONAL, large_generator=True, large_variational=True))
    cp = pa.integrators._PclContext(d=d, m=m, N=N, z_dim=cs.z_dim, u_off=cs.u_off, dt_off=cs.dt_off, x_offs=[0], G0=G0, Gj=Gj, batch=1,
                                    batch_mode=L.PCL_BATCH_MEMBERS, pade_order=order, state_cols=cols, large_generator=True)  # fmt: skip
    for c in (cv, cp):
        c.set_stream(stream.cuda_stream)
    Zd = torch.from_numpy(Z.reshape(-1).copy()).cuda()
    bufs = {c: (torch.empty(c.n_rows, dtype=torch.float64, device="cuda"), torch.empty(c.jac_nnz, dtype=torch.float64, device="cuda")) for c in (cv, cp)}
    jobs = {"variational": lambda: cv.eval_jac_dev(Zd, *bufs[cv]), "plain": lambda: cp.eval_jac_dev(Zd, *bufs[cp])}
    kern = {}
    for nm, j in jobs.items():
        j()
        kern[nm] = (cv if nm == "variational" else cp).get_option("last_kernel")
    torch.cuda.synchronize()
    out = {"d": d, "n": n, "state_cols": cols, "m": m, "v": v, "N": N, "order": order, "last_kernel": kern}
    if check:  # the float64 lifted oracle, this shape and order
        Zl, lay, G0l, Gjl = vt.lifted(cs)
        from oracle import pade_oracle as po

        d_ref = vt.residual(cs, order)
        j_ref = po.pade_jacobian_values(Zl, lay, G0l, Gjl, order).reshape(cs.K, -1)[:, vl.value_index(cs)].reshape(-1)
        dd, vd = bufs[cv][0].cpu().numpy(), bufs[cv][1].cpu().numpy()
        out["max_rel_err_vs_numpy"] = {"residual": float(np.abs(dd - d_ref).max() / np.abs(d_ref).max()), "jacobian": float(np.abs(vd - j_ref).max() / np.abs(j_ref).max())}
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
    K = N - 1
    nbytes = {"variational": 8 * (cv.n_rows + cv.jac_nnz), "plain": 8 * (cp.n_rows + cp.jac_nnz)}
    P = vl.var_large_plan(n, cols, m, v, items=K, n_cu=cv.get_option("n_cu"))
    out.update(launch_us=us, launches=a.launches, warmup=a.warmup, ratio_to_plain=round(us["variational"] / us["plain"], 3), bytes_stored=nbytes,
               GB_per_s_stored={nm: round(nbytes[nm] / us[nm] * 1e-3, 1) for nm in us},
               plan={"workgroups_per_interval": P["U"], "threads": P["threads"], "lds_bytes": P["bytes"], "chain_units": P["chain_units"], "state_columns_per_chain_unit": P["nc"],
                     "drive_groups": P["ngrp"], "panel_units_per_role": P["pu"], "power_columns_per_panel_unit": P["npc"], "roles": 1 + v})  # fmt: skip
    if cols > 1:
        blocks = 8 * (2 + 4 * v) * cols * n * n * K
        out["block_stream"] = {"bytes": blocks, "share_of_hbm_bound": round(blocks / (us["variational"] * 1e-6) / HBM_PEAK, 3),
                               "hbm_bound": "8.0 TB/s, the specified peak"}  # fmt: skip
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "var_large_bench.json"))
    a = ap.parse_args()
    import torch

    import bench_large as bl
    import piccolo_jl_amd as pa
    import var_large_cases as vl
    import variational_truth as vt

    assert torch.cuda.is_available(), "bench_var_large.py needs a GPU"
    pa.build_library()
    out = {"system": "dispersive qubit-cavity, 4 transmon levels x cavity levels, four drives (bench/bench_large.py); H_var_1 = a'a, H_var_2 = b'b",
           "device": torch.cuda.get_device_name(0), "timing": "HIP events on the launch stream, median; variational and plain launches alternate", "cases": []}  # fmt: skip
    rng = np.random.default_rng(2026)
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
                    r = measure(torch, pa, vl, vt, G0, Gj, Gv, d, cols, order, a, rng, check=cols == 1)
                    print("n=%d cols=%d v=%d order=%d: variational %.1f us, plain %.1f us, ratio %.2f" % (2 * d, cols, v, order, r["launch_us"]["variational"],
                                                                                                         r["launch_us"]["plain"], r["ratio_to_plain"]), file=sys.stderr)  # fmt: skip
                    out["cases"].append(r)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
