"""GPU: a plain `bench.py` run times exactly --steps steps once and nothing else, and --dump-outputs writes what its last
timed step computed — the same arrays from two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1"] + list(args), cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_and_its_output_dump(tmp_path):
    E, K = 256, 5
    runs = []
    for name in ("a", "b"):
        d = _bench("--steps", str(K), "--warmup", "2", "--nenvs", str(E), "--dump-outputs", str(tmp_path / name))
        assert d["steps"] == K and d["warmup"] == 2 and d["ms_per_step"] > 0
        assert d["value"] == pytest.approx(10 * E * K / (d["ms_per_step"] * K * 1e-3), rel=1e-3)
        assert d["unit"] == "agent-steps/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
        assert d["cpu_baseline"] is None and d["value_episode_graph"] is None and len(d["timing"]["attempts"]) == 1
        runs.append(tmp_path / name)
    names = sorted(os.listdir(runs[0]))
    assert {"action.npy", "reward.npy", "done.npy", "value.npy", "next_obs.npy", "hidden0.npy", "hidden1.npy"} <= set(names)
    assert names == sorted(os.listdir(runs[1]))
    total = 0
    for n in names:
        x, y = np.load(runs[0] / n), np.load(runs[1] / n)
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y), n
        total += x.nbytes
    assert total <= 64 << 20
    assert np.load(runs[0] / "action.npy").shape == (2, E, 10)       # movement + communication gate, E envs x 10 agents
    assert np.load(runs[0] / "reward.npy").shape == (E, 10)
