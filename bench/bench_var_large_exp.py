"""Measurement of the large variational exponential kernel (contexts created with PCL_BATCH_VARIATIONAL_EXP | PCL_LARGE_N | PCL_LARGE_VAR |
PCL_LARGE_VAR_EXP, pade_order "exp"; pcl_kernel_var_large_exp.hpp) on the dispersive qubit-cavity system of bench/bench_large.py (4 transmon
levels x 12 or 15 cavity levels: generator dimension n = 96 and 120, four drives).  H_var_1 is the cavity number operator a'a, H_var_2 -- the
cases with two variations -- the transmon number operator b'b; scales 1.  States: one ket and the unitary (d columns).  N = 100 knots, every step
h_k |G(u_k)|_1 = 0.8: one substep (s' = 1).

Per case FOUR launches are timed ALTERNATELY in one process, by HIP events on the launch stream (the median of --launches launches after
--warmup): the fused residual + Jacobian launch and the residual-only launch of the variational context, and the same two of a plain
PCL_LARGE_N | PCL_LARGE_EXP context of the same system (component 0 of the same knots).  Writes ONE JSON document (--out, default
profiles/var_large_exp_bench.json) and prints it as one line; per case:
  plan            what the launch code chose (the Python restatement of var_large_exp_plan in tests/var_large_exp_cases.py, held against the
                  launch code's table by tests/test_var_large_exp_cpu.py) and the plain launch's plan (tests/large_exp_cases.py)
  launch_us       the four medians
  ratio_to_plain  fused / fused and residual / residual
  predicted       the ratio of 16-column matrix-core passes per interval the two plans run (DESIGN.md 4.29 states the count before the
                  measurement), and measured / predicted
  max_rel_err     against scipy's expm / expm_frechet on the lifted generator (tests/var_exp_truth.py), the first four knots of the v = 1 ket case
There is no threshold: nothing was measured at these sizes on this constraint before, and no earlier commit can run them.

    python bench/bench_var_large_exp.py [--launches 50] [--warmup 5] [--out FILE]
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


def trajectory(G0, Gj, d, cols, v, N, rng):
    """Knots [X | Xv_1 .. | dt | t | u]: normalised random columns, |u| ~ 2 pi 0.01, dt_k = 0.8 / |G(u_k)|_1."""
    n, m = 2 * d, len(Gj)
    xdc = n * cols
    Z = np.zeros((N, (1 + v) * xdc + 2 + m))
    X = rng.standard_normal((N, (1 + v) * cols, n))
    Z[:, : (1 + v) * xdc] = (X / np.linalg.norm(X, axis=2, keepdims=True)).reshape(N, -1)
    Z[:, (1 + v) * xdc + 2 :] = 2.0 * np.pi * 0.01 * rng.standard_normal((N, m))
    for k in range(N):
        G = G0 + np.tensordot(Z[k, (1 + v) * xdc + 2 :], Gj, axes=1)
        Z[k, (1 + v) * xdc] = 0.8 / np.abs(G).sum(axis=0).max()
    Z[:, (1 + v) * xdc + 1] = np.cumsum(Z[:, (1 + v) * xdc])
    return Z


def median_us(pairs):
    return round(float(np.median([e0.elapsed_time(e1) * 1e3 for e0, e1 in pairs])), 2)


def plain_passes(P, jac):
    return P["U"] * -(-P["W"] // 16) if jac else P["sx"] * -(-P["nc"] // 16)


def measure(torch, pa, vx, le, vt, G0, Gj, Gv, d, cols, a, rng, check):
    L = pa._lib
    n, m, v, N = 2 * d, len(Gj), len(Gv), a.N
    xdc = n * cols
    Z = trajectory(G0, Gj, d, cols, v, N, rng)
    cs = vt.VarCase(Z=Z, z_dim=Z.shape[1], N=N, n=n, C=cols, m=m, xo=[b * xdc for b in range(1 + v)], u_off=(1 + v) * xdc + 2, dt_off=(1 + v) * xdc,
                    G0=G0, Gv=list(Gv), Gj=Gj)  # fmt: skip
    stream = torch.cuda.current_stream()
    cv = pa.integrators._PclContext(**vx.context_args(cs, batch_mode=L.PCL_BATCH_VARIATIONAL_EXP, large_generator=True, large_variational=True,
                                                       large_var_exp=True))  # fmt: skip
    cp = pa.integrators._PclContext(d=d, m=m, N=N, z_dim=cs.z_dim, u_off=cs.u_off, dt_off=cs.dt_off, x_offs=[0], G0=G0, Gj=Gj, batch=1,
                                    batch_mode=L.PCL_BATCH_MEMBERS, pade_order="exp", state_cols=cols, large_generator=True, large_exp=True)  # fmt: skip
    for c in (cv, cp):
        c.set_stream(stream.cuda_stream)
    Zd = torch.from_numpy(Z.reshape(-1).copy()).cuda()
    bufs = {c: (torch.empty(c.n_rows, dtype=torch.float64, device="cuda"), torch.empty(c.jac_nnz, dtype=torch.float64, device="cuda")) for c in (cv, cp)}
    jobs = {"fused": lambda: cv.eval_jac_dev(Zd, *bufs[cv]), "residual": lambda: cv.eval_dev(Zd, bufs[cv][0]),
            "plain_fused": lambda: cp.eval_jac_dev(Zd, *bufs[cp]), "plain_residual": lambda: cp.eval_dev(Zd, bufs[cp][0])}  # fmt: skip
    kern = {}
    for nm, j in jobs.items():
        j()
        kern[nm] = (cp if nm.startswith("plain") else cv).get_option("last_kernel")
    torch.cuda.synchronize()
    out = {"d": d, "n": n, "state_cols": cols, "m": m, "v": v, "N": N, "substeps": 1, "last_kernel": kern}
    if check:  # scipy on the lifted generator, the first four knots
        import var_exp_truth as vet

        c4 = vt.VarCase(**{**cs.__dict__, "Z": Z[:4], "N": 4})
        d_ref, j_ref = vet.residual(c4), vet.values(c4)
        cv.eval_jac_dev(Zd, *bufs[cv])
        torch.cuda.synchronize()
        dd, vd = bufs[cv][0].cpu().numpy()[: d_ref.size], bufs[cv][1].cpu().numpy()[: j_ref.size]
        out["max_rel_err_vs_scipy"] = {"residual": float(np.abs(dd - d_ref).max() / np.abs(d_ref).max()), "jacobian": float(np.abs(vd - j_ref).max() / np.abs(j_ref).max())}
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
    P, Pe = vx.var_large_exp_plan(n, cols, m, v), vx.var_large_exp_plan(n, cols, m, v, jac=False)
    Q, Qe = le.plan(n, cols, m, items=N - 1, n_cu=cv.get_option("n_cu")), le.plan(n, cols, m, jac=False, items=N - 1, n_cu=cv.get_option("n_cu"))
    pred = {"fused": round(P["passes"] / plain_passes(Q, True), 3), "residual": round(Pe["passes"] / plain_passes(Qe, False), 3)}
    ratio = {"fused": round(us["fused"] / us["plain_fused"], 3), "residual": round(us["residual"] / us["plain_residual"], 3)}
    out.update(launch_us=us, launches=a.launches, warmup=a.warmup, ratio_to_plain=ratio,
               predicted={"passes": {"fused": P["passes"], "residual": Pe["passes"], "plain_fused": plain_passes(Q, True), "plain_residual": plain_passes(Qe, False)},
                          "ratio_to_plain": pred, "measured_over_predicted": {k: round(ratio[k] / pred[k], 3) for k in pred}},
               bytes_stored={"fused": 8 * (cv.n_rows + cv.jac_nnz), "plain_fused": 8 * (cp.n_rows + cp.jac_nnz)},
               plan={"workgroups_per_interval": P["U"], "threads": P["threads"], "lds_bytes": P["bytes"], "chain_units": P["chain_units"], "state_columns_per_chain_unit": P["nc"],
                     "drives_per_chain_unit": P["mg"], "drive_groups": P["ngrp"], "panel_units": P["pu"], "identity_columns_per_panel_unit": P["npc"], "buffer_columns": P["W"]},
               plain_plan={"workgroups_per_interval": Q["U"], "state_columns_per_unit": Q["nc"], "drives_per_unit": Q["mg"], "identity_columns_per_unit": Q["npc"], "buffer_columns": Q["W"]})  # fmt: skip
    cv.close()
    cp.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--N", type=int, default=100)
    ap.add_argument("--cavity-levels", default="12,15")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "var_large_exp_bench.json"))
    a = ap.parse_args()
    import torch

    import bench_large as bl
    import large_exp_cases as le
    import piccolo_jl_amd as pa
    import var_large_exp_cases as vx
    import variational_truth as vt

    assert torch.cuda.is_available(), "bench_var_large_exp.py needs a GPU"
    pa.build_library()
    out = {"system": "dispersive qubit-cavity, 4 transmon levels x cavity levels, four drives (bench/bench_large.py); H_var_1 = a'a, H_var_2 = b'b; every step h |G(u_k)|_1 = 0.8 (s' = 1)",
           "device": torch.cuda.get_device_name(0), "timing": "HIP events on the launch stream, median; the four launches alternate", "cases": []}  # fmt: skip
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
                r = measure(torch, pa, vx, le, vt, G0, Gj, Gv, d, cols, a, rng, check=cols == 1 and v == 1)
                print("n=%d cols=%d v=%d: fused %.1f us (plain %.1f, ratio %.2f, predicted %.2f), residual %.1f us (plain %.1f, ratio %.2f, predicted %.2f)" % (
                    2 * d, cols, v, r["launch_us"]["fused"], r["launch_us"]["plain_fused"], r["ratio_to_plain"]["fused"], r["predicted"]["ratio_to_plain"]["fused"],
                    r["launch_us"]["residual"], r["launch_us"]["plain_residual"], r["ratio_to_plain"]["residual"], r["predicted"]["ratio_to_plain"]["residual"]), file=sys.stderr)  # fmt: skip
                out["cases"].append(r)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
