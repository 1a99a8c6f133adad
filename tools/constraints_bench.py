#!/usr/bin/env python
"""Time the scene-graph constraint accuracy (commonscenes_amd/constraints.py) on the device: the 48-scene fixture
tests/golden/constraints.npz and that fixture tiled to 4096 scenes.  Report only, no gate.

  call     constraints.validate_constrains_many: host packing of the scene list, uploads, the launch, ONE read-back
  launch   cs_scene_constraints alone on pre-packed device buffers (device events around `reps` back-to-back launches)

    python tools/constraints_bench.py [--out profiles/constraints.txt]
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from commonscenes_amd import constraints as CN, lib as L
    from commonscenes_amd.ops import _stream
    if not torch.cuda.is_available():
        raise SystemExit("constraints_bench: needs the HIP device")
    g = np.load(ROOT / "tests" / "golden" / "constraints.npz")
    vocab = {"pred_idx_to_name": [str(n) + "\n" for n in g["pred_names"]]}
    bp, tp = g["box_ptr"], g["triple_ptr"]
    boxes, tri = torch.from_numpy(g["boxes"]).cuda(), torch.from_numpy(g["triples"]).cuda()
    base = [(tri[tp[s]:tp[s + 1]], boxes[bp[s]:bp[s + 1]]) for s in range(len(bp) - 1)]
    prop = torch.cuda.get_device_properties(0)
    lines = [f"device: {prop.name} ({getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} CUs)"]
    for tile, reps in ((1, 200), (4096 // len(base) + 1, 10)):
        scenes = (base * tile)[:4096] if tile > 1 else base
        S, T = len(scenes), sum(int(s[0].shape[0]) for s in scenes)
        want = CN.validate_constrains_many(scenes, vocab)                      # warm-up; also the expected totals
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            got = CN.validate_constrains_many(scenes, vocab)                   # ends in its read-back
        call = (time.perf_counter() - t0) / reps
        assert got["total"] == want["total"]
        # the launch alone, on buffers packed once
        box_ptr = np.concatenate([[0], np.cumsum([s[1].shape[0] for s in scenes])]).astype(np.int64)
        tri_ptr = np.concatenate([[0], np.cumsum([s[0].shape[0] for s in scenes])]).astype(np.int64)
        pb = torch.cat([s[1] for s in scenes]).contiguous()
        pt = torch.cat([s[0] for s in scenes]).contiguous()
        meta = torch.from_numpy(np.concatenate([box_ptr, tri_ptr])).cuda()
        codes = torch.tensor(CN.predicate_codes(vocab), dtype=torch.int32).cuda()
        norm = torch.from_numpy(CN._norm_rows(None, 6)).cuda()
        verdict = torch.empty(T, dtype=torch.int8, device="cuda")
        counts = torch.empty((S, 11, 2), dtype=torch.int32, device="cuda")
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        dll = L.load()

        def launch():
            L.check(dll.cs_scene_constraints(pb.data_ptr(), pb.shape[0], 6, 6, pt.data_ptr(), T, meta.data_ptr(),
                                             meta[S + 1:].data_ptr(), S, codes.data_ptr(), codes.numel(), None, 0,
                                             norm.data_ptr(), 3.0, 1, 0.3, verdict.data_ptr(), counts.data_ptr(),
                                             status.data_ptr(), _stream()), "cs_scene_constraints")
        launch()
        torch.cuda.synchronize()
        n = 500
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            launch()
        e1.record()
        torch.cuda.synchronize()
        dev = e0.elapsed_time(e1) / n * 1e-3
        assert int(status.cpu()) == 0 and int(counts[:, :, 1].sum().cpu()) == want["total"][1]
        lines.append(f"{S} scenes, {T} triples ({want['total'][1]} evaluated, {want['total'][0]} satisfied): "
                     f"validate_constrains_many {call * 1e3:.3f} ms per call (mean of {reps}; host packing + uploads + launch + "
                     f"one read-back); cs_scene_constraints alone {dev * 1e6:.1f} us per launch (device events, {n} "
                     f"back-to-back launches incl. the counts reset)")
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
