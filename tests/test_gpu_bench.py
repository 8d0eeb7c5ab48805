"""-m gpu: bench.py's plain run (the headline figure only) and --dump-outputs (what the last timed step computed, the same from
run to run: the timed steps start from the state the warm-up steps left, however many untimed steps the run took in between)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra or {})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, env=env,
                       cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_reports_the_headline_and_dumps_the_same_outputs_every_time(tmp_path):
    args = ["--gpus", "1", "--config", "c1", "--steps", "3", "--warmup", "2"]
    # the second run settles three times as long: more untimed steps between the warm-up and the timed region
    lines = [_bench(args + ["--dump-outputs", str(tmp_path / run)], {"AVF_BENCH_SETTLE_S": settle})
             for run, settle in (("a", "0.3"), ("b", "0.9"))]
    assert lines[1]["untimed_steps_beyond_warmup"] > lines[0]["untimed_steps_beyond_warmup"]
    for d in lines:
        assert d["steps"] == 3 and d["warmup"] == 2 and d["ms_per_step"] > 0 and d["value"] > 0
        assert d["dtype"] == "bf16" and d["unit"] == "clips/s" and d["higher_is_better"] is True
        for k in ("roofline", "cpu_baseline", "north_star_shape", "kernel_classes", "fwd_bwd_ms_per_step", "clock_power"):
            assert k not in d, k  # --full only
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["grads.npy", "logits.npy", "loss.npy", "params.npy"]
    assert sorted(os.listdir(tmp_path / "b")) == names
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        total += a.nbytes
        assert a.dtype == np.float32 and a.shape == b.shape and np.isfinite(a).all(), n
        err = float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-30))
        assert err <= 1e-6, (n, err)
    assert total <= 64 << 20
    assert np.load(tmp_path / "a" / "logits.npy").shape == (4, 21)  # c1: B = 4, the [B, 21] rows
    loss = np.load(tmp_path / "a" / "loss.npy").item()  # the line's loss is the last timed step's
    assert abs(loss - lines[0]["config"]["loss"]) <= 1e-6 * max(1.0, abs(loss))
