"""tools/eval_walkthrough.py --object-views: one 256x256 RGBA view per shaped object of every scene, named by the reference's
rule (helpers/visualize_scene.py:29-40) under DIR/render_object_imgs/<scan>/; without the flag the tool's output keeps the
keys it had before the flag existed."""
import json
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu

TOP_KEYS = {"scenes", "world", "attention", "width", "ddim_steps", "mini_B", "total_s", "box_std_mean", "angle_std_mean",
            "chamfer_diversity_mean", "chamfer_diversity_n"}
SCENE_KEYS = {"scan", "nodes", "shapes", "triples", "sample_s", "verts", "finite", "angle_range", "export"}
EXPORT_KEYS = {"obj", "image", "verts", "faces", "dropped", "covered", "apply_bytes", "first_call_s", "device_s", "assemble_s",
               "render_s", "numpy_fit_s"}


def _run(extra):
    env = dict(os.environ, CS_ONE_DEVICE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, str(ROOT / "tools" / "eval_walkthrough.py"), "--scenes", "2", "--samples", "2", "--points", "500"]
    r = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=600, env=env, cwd=str(ROOT))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("EVAL_WALKTHROUGH ")]
    assert len(lines) == 1
    return json.loads(lines[0].split(" ", 1)[1])


def test_object_views_are_written_per_shaped_object(tmp_path):
    from PIL import Image
    d = _run(["--export-scenes", str(tmp_path), "--object-views"])
    assert set(d) == TOP_KEYS | {"object_views"}
    ov = d["object_views"]
    assert ov["images"] == sum(s["shapes"] for s in d["scenes"]) == 9 and ov["render_s"] > 0 and ov["write_s"] > 0
    for s in d["scenes"]:
        files = sorted((tmp_path / "render_object_imgs" / s["scan"]).iterdir())
        assert len(files) == s["shapes"]
        inst = set()
        for f in files:
            m = re.fullmatch(r"obj(\d+)_(\d+)_(\d+)\.png", f.name)          # <label>_<cat>_<instance>, label = obj<cat>
            assert m and m.group(1) == m.group(2) and 0 < int(m.group(2)) < 34      # never _scene_ (0) or floor (34)
            inst.add(int(m.group(3)))
            img = Image.open(f)
            assert img.mode == "RGBA" and img.size == (256, 256)
            a = np.asarray(img)
            assert set(np.unique(a[..., 3]).tolist()) == {127, 255}          # tensor2im: alpha 0 -> 127, 1 -> 255; mask not empty
            assert (a[..., :3][a[..., 3] == 127] == 255).all()               # white background
        assert inst == set(range(1, s["shapes"] + 1))


def test_output_without_the_flag_keeps_its_keys(tmp_path):
    d = _run(["--export-scenes", str(tmp_path)])
    assert set(d) == TOP_KEYS
    for s in d["scenes"]:
        assert set(s) == SCENE_KEYS and set(s["export"]) == EXPORT_KEYS
    assert not (tmp_path / "render_object_imgs").exists()


def test_flag_needs_an_export_directory():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "eval_walkthrough.py"), "--object-views"], capture_output=True,
                       text=True, timeout=120, cwd=str(ROOT))
    assert r.returncode == 2 and "--export-scenes" in r.stderr
