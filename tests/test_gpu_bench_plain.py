"""GPU: a plain ``bench.py`` run (no ``--full``) on a small geometry: exactly ``--steps`` timed steps, the headline fields and
nothing of what ``--full`` adds, and ``--dump-outputs`` writing the last timed step's loss, gradient and updated weights."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_line_and_dumped_outputs(dev, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--arch", "vit_tiny_test", "--size", "224", "--batch", "2", "--dump-outputs", str(tmp_path)],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    j = json.loads(lines[0])
    assert j["steps"] == 3 and j["warmup"] == 1 and j["ms_per_step"] > 0 and j["value"] > 0
    assert j["unit"] == "img/s" and j["higher_is_better"] is True and j["dtype"] == "f16"
    assert not set(j) & {"secondary", "roofline", "cpu_baseline", "host_enqueue_ms_per_step"}
    names = sorted(os.listdir(tmp_path))
    assert names == ["decoder_grad.npy", "decoder_weights.npy", "loss.npy"], names
    for n in names:
        x = np.load(tmp_path / n)
        assert x.dtype == np.float32 and x.size > 0 and np.isfinite(x).all(), n
    assert abs(float(np.load(tmp_path / "loss.npy")[0]) - j["config"]["loss"]) < 1e-6
