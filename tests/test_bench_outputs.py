"""bench.py's plain run (headline only) and --dump-outputs: the timed path's last result lands on disk, identical from run
to run with the same arguments, so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent


def test_dump_outputs_writes_float32_and_samples_above_the_limit(tmp_path, monkeypatch):
    import bench
    small = torch.arange(24, dtype=torch.float64).reshape(2, 3, 4)
    bench.dump_outputs(tmp_path / "a", {"small": small})
    v = np.load(tmp_path / "a" / "small.npy")
    assert v.dtype == np.float32 and v.shape == (2, 3, 4) and np.array_equal(v, small.float().numpy())
    # above the limit: a fixed, seeded sample of the flattened elements, in order, the same every time
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 400)
    big = torch.arange(1000, dtype=torch.float32)
    bench.dump_outputs(tmp_path / "b", {"big": big})
    bench.dump_outputs(tmp_path / "c", {"big": big})
    vb, vc = np.load(tmp_path / "b" / "big.npy"), np.load(tmp_path / "c" / "big.npy")
    assert vb.dtype == np.float32 and vb.nbytes <= 400 and vb.size == 100
    assert np.array_equal(vb, vc) and np.all(np.diff(vb) > 0)


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    outs = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--small", "--objects", "4",
                            "--steps", "3", "--warmup", "1", "--dump-outputs", str(d)],
                           capture_output=True, text=True, timeout=600, env=env, cwd=str(ROOT))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith('{"metric"')]
        assert len(lines) == 1
        res = json.loads(lines[0])
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in res, k
        assert res["steps"] == 3 and res["warmup"] == 1 and res["finite"] is True
        assert abs(res["value"] - 1e3 / res["ms_per_step"]) < 1e-6 * res["value"]
        # nothing beyond the headline without --full
        assert res["roofline"] is None and res["decode"] is None and "cpu_baseline" not in res
        lat = np.load(d / "latents.npy")
        assert lat.dtype == np.float32 and lat.shape == (4, 3, 16, 16, 16) and np.isfinite(lat).all()
        outs.append(lat)
    assert np.array_equal(outs[0], outs[1]), "same arguments, same inputs: the dumped outputs must be identical"
