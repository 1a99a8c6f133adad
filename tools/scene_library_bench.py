#!/usr/bin/env python
"""Report-only timings of the scenes from a mesh library (commonscenes_amd/scene_library.py, csrc/cs_scene_lib.hip):

  retrieve   FurnitureLibrary.retrieve_many on --scenes scenes x ~10 boxes against one --rows-row category, next to the
             reference's host loop (helpers/util.py:71-83: one numpy argmin per box) over the same queries;
  markers    assemble_scene_from_library('onlybox') over --boxes boxes (12 tubes each);
  scene      one retrieval scene of --objects objects with markers and floor, up to its 256x256 top-down PNG bytes.

    python tools/scene_library_bench.py [--scenes 4096] [--rows 5000] [--boxes 4096] [--objects 10] [--repeats 5]
prints one `SCENE_LIBRARY {...}` JSON line.  Nothing here is a gate."""
import argparse
import io
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def timed(fn, repeats):
    fn()                                                      # first call: code objects, allocator
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return float(np.median(out)), [float(x) for x in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=5000)
    ap.add_argument("--boxes", type=int, default=4096)
    ap.add_argument("--objects", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    from commonscenes_amd import scene_mesh as S, synth
    from commonscenes_amd.scene_library import FurnitureLibrary
    rng = np.random.default_rng(48)
    res = dict(scenes=a.scenes, rows=a.rows, repeats=a.repeats)

    # --- retrieve
    sizes = rng.uniform(0.05, 3.0, (a.rows, 3))
    lib = FurnitureLibrary({"sofa": [(f"m{i}", sizes[i].tolist()) for i in range(a.rows)]})
    classes = ["sofa\n"]
    scenes = []
    for s in range(a.scenes):
        n = 8 + s % 5                                         # ~10 boxes per scene
        scenes.append((torch.from_numpy(rng.uniform(0.05, 3.0, (n, 7)).astype(np.float32)).cuda(), [0] * n))
    nq = sum(b.shape[0] for b, _ in scenes)
    got = lib.retrieve_many(scenes, classes)
    t_dev, all_dev = timed(lambda: lib.retrieve_many(scenes, classes), a.repeats)
    allq = torch.cat([b[:, :3] for b, _ in scenes]).contiguous()
    cats = [0] * nq
    t_kernel, _ = timed(lambda: lib.retrieve_rows(allq, cats), a.repeats)      # the launch with its small upload, no lists
    host_q = allq.cpu().numpy()
    t0 = time.perf_counter()
    want = [int(np.argmin(np.sum((sizes - q) ** 2, axis=-1))) for q in host_q]
    t_host = time.perf_counter() - t0
    flat = [r for _, _, rows in got for r in rows]
    res["retrieve"] = dict(queries=nq, retrieve_many_s=t_dev, retrieve_many_all_s=all_dev, retrieve_rows_s=t_kernel,
                           numpy_loop_s=t_host, equal=flat == want,
                           pairs_per_s=nq * a.rows / t_kernel,
                           note="retrieve_many includes the per-scene host lists and one read-back; numpy_loop is one argmin "
                                "per box over the same fp64 rows (util.py:74-77) without the JSON reload the reference adds")

    # --- markers
    nb = a.boxes
    boxes = np.concatenate([rng.uniform(0.3, 2.5, (nb, 3)), rng.uniform(-3, 3, (nb, 3)), rng.uniform(-180, 180, (nb, 1))],
                           axis=1).astype(np.float32)
    boxes[:, 4] = 0
    bt = torch.from_numpy(boxes).cuda()
    mc = ["chair\n"]
    t_mark, _ = timed(lambda: S.assemble_scene_from_library("onlybox", bt, [0] * nb, mc), a.repeats)
    res["markers"] = dict(boxes=nb, tubes=12 * nb, verts=120 * nb, faces=192 * nb, onlybox_scene_s=t_mark,
                          bytes_written=nb * (120 * 24 + 192 * 28), note="host planning of the per-box bases included")

    # --- one retrieval scene to its PNG
    labels = ["chair\n", "table\n", "sofa\n"]
    flib = synth.furniture_library(labels, per_category=32)
    cls = ["_scene_\n", "floor\n"] + labels
    n = a.objects + 2
    sb = np.concatenate([rng.uniform(0.4, 2.0, (n, 3)), rng.uniform(-3, 3, (n, 3)), rng.uniform(-180, 180, (n, 1))],
                        axis=1).astype(np.float32)
    sb[:, 4] = 0
    sc = [0, 1] + [2 + i % 3 for i in range(a.objects)]
    st = torch.from_numpy(sb).cuda()

    def whole():
        scene = S.assemble_scene_from_library("retrieval", st, sc, cls, library=flib, render_boxes=True, floor=True)
        img = S.render_topdown(scene, 256)
        rgb = img["rgb"].cpu().numpy()
        try:
            from PIL import Image
            buf = io.BytesIO()
            Image.fromarray(rgb).save(buf, format="PNG")
            return scene, img, buf.tell()
        except ImportError:
            return scene, img, rgb.nbytes
    scene, img, nbytes = whole()
    t_scene, _ = timed(whole, a.repeats)
    res["scene"] = dict(objects=a.objects, verts=int(scene.verts.shape[0]), faces=int(scene.faces.shape[0]),
                        covered=int((img["object_id"] >= 0).sum()), dropped=img["dropped"], png_bytes=nbytes,
                        retrieval_scene_to_png_s=t_scene)
    print("SCENE_LIBRARY " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
