"""GPU: a plain `bench.py` run -- the headline line alone, exactly --steps timed steps, and --dump-outputs (the state the last timed
step left, float32 / float64, 64 MB at most)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


@pytest.mark.gpu
def test_plain_bench_run_times_exactly_the_steps_and_dumps_the_last_step(cuda, tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT, PYTHONDONTWRITEBYTECODE="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--workload", "er",
                        "--dump-outputs", str(out)], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 7 and d["warmup"] == 2 and len(d["ms_per_step_repeats"]) == 1           # one timed region of exactly --steps
    assert abs(d["value"] - 7 * 10 / (d["ms_per_step"] * 7 * 1e-3)) < 1e-5 * d["value"]
    assert not {"roofline", "cpu_baseline", "also", "accuracy"} & set(d)                             # the --full legs
    files = sorted(os.listdir(out))
    arrs = {f[:-4]: np.load(os.path.join(out, f)) for f in files}
    assert all(f.endswith(".npy") for f in files)
    assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
    assert any(k.startswith("model.") and k.endswith(".weight") for k in arrs)
    lab = arrs["buffer_label"]
    assert lab.shape == (1000,) and np.array_equal(lab, np.round(lab)) and lab.min() >= 0 and lab.max() < 10
    rows = arrs["buffer_img_sample_rows"].astype(np.int64)
    assert arrs["buffer_img_sample"].shape == (len(rows), 3, 32, 32) and arrs["buffer_img_row_sum"].shape == (1000,)
    assert np.allclose(arrs["buffer_img_sample"].reshape(len(rows), -1).sum(1, dtype=np.float64), arrs["buffer_img_row_sum"][rows])
    assert all(np.isfinite(a).all() for a in arrs.values())
