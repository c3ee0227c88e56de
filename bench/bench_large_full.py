"""Measurement of the rollout and the objective family on large contexts (PCL_LARGE_N with option large_full; pcl_kernel_large_rollout.hpp and
the objective kernels behind the option's gate) on the dispersive qubit-cavity systems of bench/bench_large.py: 4 transmon levels x 12 or 15
cavity levels (d = 48 and 60, generator dimension n = 96 and 120), four drives, one ket and five kets, N = 100 knots.

Writes ONE JSON document (--out, default profiles/large_full_bench.json) and prints it as one line; per case:
  plan             what the launch code chose for the two launches: panels per interval and columns of E per panel, slices and state columns per
                   slice, threads, LDS bytes (through the Python restatement of large_roll_plan in tests/large_full_cases.py)
  rollout          pcl_rollout_dev by HIP events, the median of --launches launches after --warmup; `propagators` and `chain` are its two launches
                   alone (option large_rollout_stage 1 and 2), timed the same way; `substeps` the largest s' over the intervals
  objective        pcl_objective_dev, value and gradient: a ket goal (one ket) or a coherent-ket goal over the five kets, in the general form, and a
                   regulariser on the drives
  objective_hess   pcl_objective_hess_dev of the same objective (the Gram triangle is formed once per goal, before the timed launches)
  cpu_expm_chain   the same rollout with scipy.linalg.expm per interval on --threads threads and the chain of the knots in numpy, one run
  max_rel_err_vs_scipy   the device's rollout against that one, relative to the largest entry of each knot
There is no threshold: nothing ran these shapes before, and no earlier commit can.

    python bench/bench_large_full.py [--launches 50] [--warmup 5] [--threads 16] [--out FILE]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "bench"))


def median_us(pairs):
    return round(float(np.median([e0.elapsed_time(e1) * 1e3 for e0, e1 in pairs])), 2)


def timed(torch, stream, job, a):
    for _ in range(a.warmup):
        job()
    torch.cuda.synchronize()
    evs = []
    for _ in range(a.launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        job()
        e1.record(stream)
        evs.append((e0, e1))
    torch.cuda.synchronize()
    return median_us(evs)


def cpu_chain(Z, G0, Gj, n, cols, m, threads):
    from scipy.linalg import expm

    N, xd = Z.shape[0], n * cols
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        E = list(ex.map(lambda k: expm(Z[k, xd] * (G0 + np.tensordot(Z[k, xd + 2 : xd + 2 + m], Gj, axes=1))), range(N - 1)))
    X = Z[0, :xd].reshape(cols, n).T
    out = [X.T.reshape(-1)]
    for k in range(N - 1):
        X = E[k] @ X
        out.append(X.T.reshape(-1))
    return np.array(out), time.perf_counter() - t0


def measure(torch, pa, fc, ot, bl, G0, Gj, d, cols, a, rng):
    n, m, N = 2 * d, len(Gj), a.N
    Z = bl.trajectory(d, cols, m, N, rng)
    xd = n * cols
    z_dim, dt_off, u_off = xd + 2 + m, xd, xd + 2
    c = pa.integrators._PclContext(d=d, m=m, N=N, z_dim=z_dim, u_off=u_off, dt_off=dt_off, x_offs=[0], G0=G0, Gj=Gj, batch=1,
                                   batch_mode=pa._lib.PCL_BATCH_MEMBERS, pade_order=8, state_cols=cols, large_generator=True, large_full=True)  # fmt: skip
    stream = torch.cuda.current_stream()
    c.set_stream(stream.cuda_stream)
    goals = [(lambda v: v / np.linalg.norm(v))(rng.standard_normal(d) + 1j * rng.standard_normal(d)) for _ in range(cols)]
    rows = ot.ket_rows(goals[0]) if cols == 1 else ot.coherent_ket_rows(goals)
    c.set_goal_form(0, np.asarray(rows, float), None)
    c.add_regularizer(u_off, m, 1e-2, 2)
    Zd = torch.from_numpy(Z.reshape(-1).copy()).cuda()
    xo = torch.full((N * xd,), float("nan"), dtype=torch.float64, device="cuda")
    gd = torch.empty(Z.size, dtype=torch.float64, device="cuda")
    vd = torch.empty(1, dtype=torch.float64, device="cuda")
    nh = c.objective_hess_structure()[0].size
    hd = torch.empty(nh, dtype=torch.float64, device="cuda")
    c.rollout_dev(Zd, xo)
    c.objective_hess_dev(Zd, 100.0, 1.0, hd)
    torch.cuda.synchronize()
    ref, cpu_s = cpu_chain(Z, G0, Gj, n, cols, m, a.threads)
    err = float(fc.knot_errors(xo.cpu().numpy(), ref, N).max())
    us = {"rollout": timed(torch, stream, lambda: c.rollout_dev(Zd, xo), a)}
    for stage, nm in ((1, "propagators"), (2, "chain")):
        c.set_option("large_rollout_stage", stage)
        us[nm] = timed(torch, stream, lambda: c.rollout_dev(Zd, xo), a)
    c.set_option("large_rollout_stage", 0)
    us["objective"] = timed(torch, stream, lambda: c.objective_dev(Zd, 100.0, vd, gd), a)
    us["objective_hess"] = timed(torch, stream, lambda: c.objective_hess_dev(Zd, 100.0, 1.0, hd), a)
    p = fc.roll_plan(n, cols, m, items=N - 1)
    sp = max(fc.substeps(Z[k, dt_off], G0 + np.tensordot(Z[k, u_off : u_off + m], Gj, axes=1)) for k in range(N - 1))
    out = {"d": d, "n": n, "state_cols": cols, "m": m, "N": N, "max_rel_err_vs_scipy": err,
           "rollout": {"last_kernel": c.get_option("last_kernel"), "launch_us": us["rollout"], "propagators_us": us["propagators"], "chain_us": us["chain"],
                       "launches": a.launches, "warmup": a.warmup, "substeps": sp, "degree": fc.DEG,
                       "plan": {"panels_per_interval": p["P"], "columns_per_panel": p["npc"], "lds_bytes_propagators": p["bytes_e"], "slices": p["S"],
                                "state_columns_per_slice": p["nc"], "lds_bytes_chain": p["bytes_c"], "threads": p["threads"]}},
           "objective": {"launch_us": us["objective"], "form_rows": 2, "form_L": xd, "launches_per_call": c.get_option("last_objective_launches")},
           "objective_hess": {"launch_us": us["objective_hess"], "values": int(nh), "bytes_stored": 8 * int(nh)},
           "cpu_expm_chain": {"seconds": round(cpu_s, 4), "threads": a.threads, "ratio_to_rollout": round(cpu_s * 1e6 / us["rollout"], 1)}}  # fmt: skip
    c.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--N", type=int, default=100)
    ap.add_argument("--cavity-levels", default="12,15")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "large_full_bench.json"))
    a = ap.parse_args()

    import torch

    import bench_large as bl
    import large_full_cases as fc
    import objective_truth as ot
    import piccolo_jl_amd as pa

    if not torch.cuda.is_available():
        raise SystemExit("bench_large_full.py measures on a GPU; none is available")
    rng = np.random.default_rng(2028)
    out = {"system": "dispersive qubit-cavity, 4 transmon levels x cavity levels, four drives (bench/bench_large.py)", "device": torch.cuda.get_device_name(0),
           "cases": []}  # fmt: skip
    for cl in [int(s) for s in a.cavity_levels.split(",")]:
        d = bl.QUBIT_LEVELS * cl
        H0, Hs = bl.qubit_cavity(cl)
        G0, Gj = bl.iso_generator(H0), np.array([bl.iso_generator(H) for H in Hs])
        for cols in (1, 5):
            r = measure(torch, pa, fc, ot, bl, G0, Gj, d, cols, a, rng)
            out["cases"].append(r)
            print("d %d cols %d: rollout %.1f us (propagators %.1f, chain %.1f), objective %.1f us, its Hessian %.1f us, scipy %.3f s, err %.1e"
                  % (d, cols, r["rollout"]["launch_us"], r["rollout"]["propagators_us"], r["rollout"]["chain_us"], r["objective"]["launch_us"],
                     r["objective_hess"]["launch_us"], r["cpu_expm_chain"]["seconds"], r["max_rel_err_vs_scipy"]), file=sys.stderr, flush=True)  # fmt: skip
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
