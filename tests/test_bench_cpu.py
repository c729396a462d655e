"""bench.py pieces that run without a GPU: the CPU-baseline leg (oracle env + fp64 numpy policy in forked workers) for
every workload, and the refusal to run the timed path without an MI355X (no CPU fallback)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@pytest.mark.parametrize("workload", ["pp_easy", "pp_hard", "tj_medium", "tj_hard"])
def test_cpu_baseline_leg(workload):
    import bench
    out = bench.cpu_baseline(workload, envs_per_proc=2, episodes=1, budget_s=0.3)
    pp = bench.WORKLOADS[workload][0] == 'predator_prey'
    assert set(out) == {"value", "unit", "cores", "kind", "sample", "reference_probe"} | ({"reference_shaped"} if pp else set())
    if pp:      # leg (ii): the reference-shaped numpy env (dense one-hot grid copy per step)
        assert out["reference_shaped"]["value"] > 0 and out["reference_shaped"]["unit"] == "agent-steps/s"
    assert out["reference_probe"]["rollout_1proc"] > 0 and "build container" in out["reference_probe"]["host"]
    assert out["unit"] == "agent-steps/s" and out["kind"] == "port" and out["cores"] >= 1
    assert out["value"] > 0
    N, T = bench.WORKLOADS[workload][1]['nagents'], bench.WORKLOADS[workload][1]['max_steps']
    steps = int(out["sample"].split("policy + C oracle env: ")[1].split(" env-steps")[0])
    assert steps >= out["cores"]                       # every worker played at least one step of one episode
    assert steps <= out["cores"] * 2 * T * 50          # and stopped near its budget
    assert N > 0


def test_bench_refuses_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("needs a machine without a GPU")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--no-cpu-baseline", "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "no CPU fallback" in (p.stderr + p.stdout)


def test_dump_outputs_stays_within_its_budget_and_repeats(tmp_path):
    """--dump-outputs: float32 / float64 arrays named after what the step returns, a fixed row sample of whatever exceeds
    its share, 64 MB at most in all — the same files from the same tensors."""
    import numpy as np
    import torch
    import bench
    g = torch.Generator().manual_seed(0)
    items = (bench._dump_items('logp', [torch.randn(81920, 5, generator=g), torch.randn(81920, 2, generator=g)]) +
             bench._dump_items('hidden', (torch.randn(8192, 10, 128, generator=g), torch.randn(8192, 10, 128, generator=g))) +
             bench._dump_items('next_obs', torch.randn(8192, 10, 3627, generator=g)) +
             bench._dump_items('action', torch.randint(0, 5, (2, 8192, 10), generator=g, dtype=torch.int32)) +
             bench._dump_items('stat', {'n': torch.as_tensor(7), 'r': torch.as_tensor(np.ones(3))}))
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), items)
    names = sorted(os.listdir(tmp_path / 'a'))
    assert names == sorted(n + '.npy' for n, _ in items)
    total = 0
    for n in names:
        x, y = np.load(tmp_path / 'a' / n), np.load(tmp_path / 'b' / n)
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y)
        total += x.nbytes
    assert total <= 64 << 20
    assert np.load(tmp_path / 'a' / 'stat_r.npy').dtype == np.float64
    obs = dict(items)['next_obs']
    got = np.load(tmp_path / 'a' / 'next_obs.npy')
    assert 0 < got.shape[0] < obs.shape[0] and got.shape[1:] == tuple(obs.shape[1:])
    rows = np.sort(np.random.RandomState(0).choice(obs.shape[0], size=got.shape[0], replace=False))
    assert np.array_equal(got, obs[torch.from_numpy(rows)].numpy())


def test_bench_options():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "--full" in p.stdout and "--dump-outputs" in p.stdout
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode != 0 and "--steps must be >= 1" in p.stderr
