"""bench.py's own options, without a GPU (--dry-run replaces the GPU work by a sleep, everything around it is the real
code): --steps is the number of timed steps, a plain run carries no CPU baseline, --dump-outputs writes float .npy."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*extra):
    e = dict(os.environ, OMP_NUM_THREADS="1")
    e.pop("WORLD_SIZE", None); e.pop("RANK", None); e.pop("LOCAL_RANK", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *extra], env=e,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_plain_run_line_and_dumped_outputs(tmp_path):
    out = _bench("--gpus", "1", "--steps", "4", "--warmup", "1", "--dry-run", "--frames", "1000",
                 "--dump-outputs", str(tmp_path / "dump"))
    assert out["steps"] == 4 and out["warmup"] == 1 and out["dry_run"]
    assert out["metric"] == "HE-AAC frames/s (batched)" and out["unit"] == "frames/s" and out["higher_is_better"]
    assert out["dtype"] == "f32" and out["ms_per_step"] > 0
    assert "cpu_baseline" not in out
    files = sorted(os.listdir(tmp_path / "dump"))
    assert "pcm.npy" in files and "frame_index.npy" in files
    total = 0
    for f in files:
        a = np.load(tmp_path / "dump" / f)
        assert a.dtype in (np.float32, np.float64), (f, a.dtype)
        total += a.nbytes
    assert total <= 64 << 20
    idx = np.load(tmp_path / "dump" / "frame_index.npy")
    assert len(idx) == np.load(tmp_path / "dump" / "pcm.npy").shape[0]


def test_full_is_an_option():
    out = _bench("--gpus", "1", "--steps", "2", "--warmup", "0", "--dry-run", "--frames", "64", "--full")
    assert out["steps"] == 2 and "roofline" in out
