"""bench.py's plain run and `--dump-outputs` on the GPU, at a small size: the line reports exactly `--steps` timed update steps
and their `ms_per_step`, the secondary legs stay behind `--full`, and the dump holds what the last timed step computed --
the same arrays from two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
ARGS = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--spin-up", "2", "--n-steps", "20", "--batch", "5000"]
DUMPED = {"stats", "actor_ft_grads", "critic_grads", "actor_ft_params", "critic_params"}


def run(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, BENCH] + ARGS + ["--dump-outputs", str(out_dir)], env=env, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.lstrip().startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_reports_its_steps_and_dumps_the_last_step(tmp_path):
    lines = [run(tmp_path / "a"), run(tmp_path / "b")]
    for r in lines:
        assert r["steps"] == 3 and r["warmup"] == 1 and r["passes"]["n"] == 1 and r["passes"]["steps_each"] == 3
        assert r["ms_per_step"] > 0 and r["value"] == pytest.approx(5000 / (r["ms_per_step"] * 1e-3), rel=1e-9)
        assert r["unit"] == "samples/s" and r["higher_is_better"] is True and r["dtype"] == "bf16"
        assert not {"env_steps_per_sec", "fp32", "configs", "pixel", "cpu_baseline"} & set(r)
    assert {f[:-len(".npy")] for f in os.listdir(tmp_path / "a")} == DUMPED
    total = 0
    for name in sorted(DUMPED):
        x, y = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert x.dtype in (np.float32, np.float64) and x.size > 0 and np.isfinite(x).all(), name
        np.testing.assert_array_equal(x, y, err_msg=name)
        total += x.nbytes
    assert total <= 64 << 20
    stats = np.load(tmp_path / "a" / "stats.npy")
    last = lines[0]["last_stats"]
    assert (stats[0], stats[1], stats[2], stats[4]) == (last["pg_loss"], last["v_loss"], last["approx_kl"], last["ratio"])
    assert np.abs(np.load(tmp_path / "a" / "actor_ft_grads.npy")).sum() > 0
