"""bench.py's plain run and its --dump-outputs: what the timed path computed in its last step, written so that two builds can be compared."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_dump_outputs_budget_and_fixed_sample(tmp_path):
    """Small arrays whole, large ones as a sorted, seeded sample that shares the budget; the same arrays give the same files."""
    import torch

    bench = _bench_module()
    rng = np.random.default_rng(3)
    arrays = {"small": torch.from_numpy(rng.standard_normal(1000)), "scalar": torch.from_numpy(rng.standard_normal(1)),
              "large": torch.from_numpy(rng.standard_normal(bench.DUMP_WHOLE + 12345)),
              "larger": torch.from_numpy(rng.standard_normal(8 * bench.DUMP_WHOLE).astype(np.float32))}  # fmt: skip
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), arrays)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["large_sample.npy", "larger_sample.npy", "scalar.npy", "small.npy"]
    total = 0
    for nm in names:
        a, b = np.load(tmp_path / "a" / nm), np.load(tmp_path / "b" / nm)
        assert a.dtype == np.float64 and np.array_equal(a, b), nm
        total += os.path.getsize(tmp_path / "a" / nm)
    assert total <= 64 << 20
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), arrays["small"].numpy())
    assert np.array_equal(np.load(tmp_path / "a" / "large_sample.npy"), arrays["large"].numpy())  # within its share of the budget: every value, in order
    full = arrays["larger"].numpy().astype(np.float64)
    smp = np.load(tmp_path / "a" / "larger_sample.npy")
    assert 0 < smp.size < full.size
    idx = np.sort(np.random.default_rng(full.size).choice(full.size, size=smp.size, replace=False))  # distinct positions, increasing
    assert np.array_equal(smp, full[idx])


@pytest.mark.gpu
def test_plain_bench_run_dumps_the_timed_outputs(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR`: the headline alone (no extras), K timed steps, and in DIR the residual and a sample
    of the Jacobian values of the timed launch -- equal to the C oracle's on the same seeded trajectory."""
    from oracle import pade_oracle as po
    from oracle import ref_lib
    from piccolo_jl_amd import synthetic

    out_dir = tmp_path / "out"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    pr = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--dump-outputs", str(out_dir)],
                        stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)  # fmt: skip
    assert pr.returncode == 0, pr.stderr.decode()[-2000:]
    lines = [ln for ln in pr.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    out = json.loads(lines[0])
    assert out["steps"] == 7 and out["warmup"] == 2 and out["ms_per_step"] > 0 and out["value"] > 0 and out["config"]["workload_id"] == "single"
    assert abs(out["value"] * out["ms_per_step"] * 1e-3 - 1.0) < 1e-9  # one evaluation per step
    for key in ("other_rates", "cpu_baseline", "multistart_share", "ensemble_share", "value_reference_order", "multistart_64"):
        assert key not in out, key  # --full only
    assert sorted(os.listdir(out_dir)) == ["jacobian_values_sample.npy", "residual.npy"]
    assert sum(os.path.getsize(out_dir / f) for f in os.listdir(out_dir)) <= 64 << 20
    delta, vals = np.load(out_dir / "residual.npy"), np.load(out_dir / "jacobian_values_sample.npy")
    system = synthetic.config_system(3)
    tr = synthetic.synthetic_trajectory(system, 100, seed=1000)
    lay = po.Layout.smooth_pulse(system.levels, system.n_drives, 100)
    d_ref, j_ref = ref_lib.eval_jac(tr.datavec.reshape(100, -1), lay, system.G_drift, system.G_drives_array())
    d_ref, j_ref = d_ref.reshape(-1), j_ref.reshape(-1)
    idx = np.sort(np.random.default_rng(j_ref.size).choice(j_ref.size, size=vals.size, replace=False))
    assert delta.dtype == np.float64 and delta.shape == d_ref.shape
    assert np.abs(delta - d_ref).max() <= 1e-12 * max(1.0, np.abs(d_ref).max())
    assert np.abs(vals - j_ref[idx]).max() <= 1e-12 * max(1.0, np.abs(j_ref).max())
