#!/usr/bin/env python
"""Triangle meshes -> SDF grids on the MI355X (commonscenes_amd.mesh_sdf.mesh_to_sdf): the input every shape entry of the
project takes -- VQVAE.encode, shape_comp / tools/complete_shape.py --sdf, tools/eval_checkpoint.py --sdfs.

    python tools/mesh_to_sdf.py --obj a.obj b.obj --out shapes.npy [--res 64] [--trunc 0.2] [--bound 1.0] [--no-normalize]
    python tools/mesh_to_sdf.py --synthetic 10000 [--batch 32]        # a generated sphere mesh of about that many faces

Writes [N,1,res,res,res] fp32 and prints one JSON line (`MESH_TO_SDF {...}`): shapes, face counts, slices, centroid / scale,
inside share and device time per mesh (device events around synchronised work, second call of the process; report only).
--against FILE.npy adds the max / mean absolute difference to an existing grid: how an operator who has the original
`ori_sample_grid.h5` data can pin the convention, which is unpinned here.  --compare-host adds the time
of a numpy brute force on the first mesh at a reduced resolution (report only).
"""
import argparse
import json
import math
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import numpy as np  # noqa: E402
import torch  # noqa: E402


def uv_sphere(faces: int, radius: float = 0.8):
    """a closed latitude / longitude sphere of about `faces` triangles (2 nu (nv - 1)), outward normals"""
    nv = max(3, int(round(math.sqrt(faces / 4.0))))
    nu = max(3, int(round(faces / (2.0 * (nv - 1)))))
    th = np.arange(1, nv) * (np.pi / nv)
    ph = np.arange(nu) * (2 * np.pi / nu)
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)),
                     np.outer(np.cos(th), np.ones(nu))], -1).reshape(-1, 3)
    v = np.concatenate([[[0, 0, 1.0]], ring, [[0, 0, -1.0]]]) * radius
    rid = lambda i, j: 1 + i * nu + (j % nu)
    f = []
    for j in range(nu):
        f.append((0, rid(0, j), rid(0, j + 1)))
        f.append((len(v) - 1, rid(nv - 2, j + 1), rid(nv - 2, j)))
    for i in range(nv - 2):
        for j in range(nu):
            f += [(rid(i, j), rid(i + 1, j), rid(i + 1, j + 1)), (rid(i, j), rid(i + 1, j + 1), rid(i, j + 1))]
    return torch.from_numpy(v.astype(np.float32)), torch.tensor(f, dtype=torch.int64)


def host_brute_force(v, f, n, bound):
    """numpy fp64: distance to the closest point of every triangle (closest point, then the norm) and the winding sign"""
    sys.path.insert(0, str(ROOT / "tests"))
    import _mesh_sdf_ref as R
    t0 = time.perf_counter()
    R.sdf(R.grid_points(n, bound), v.double().numpy()[f.numpy()])
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obj", nargs="+", help=".obj files (v / f lines; polygons are fanned)")
    ap.add_argument("--synthetic", type=int, metavar="F", help="a generated sphere of about F faces instead of files")
    ap.add_argument("--batch", type=int, default=1, help="--synthetic: copies in the batch")
    ap.add_argument("--out", help="output .npy")
    ap.add_argument("--res", type=int, default=64)
    ap.add_argument("--trunc", type=float, default=None, help="clamp to +-TRUNC (the dataset loader uses 0.2)")
    ap.add_argument("--bound", type=float, default=1.0)
    ap.add_argument("--no-normalize", action="store_true", help="take the vertices as given")
    ap.add_argument("--against", help=".npy of grids of the same shape to compare with")
    ap.add_argument("--compare-host", action="store_true", help="time a numpy brute force on the first mesh at res 8")
    a = ap.parse_args()
    if (a.obj is None) == (a.synthetic is None):
        ap.error("give --obj FILE [FILE ...] or --synthetic F")
    if a.obj and not a.out:
        ap.error("--obj needs --out FILE.npy")
    assert torch.cuda.is_available(), "needs the MI355X (no CPU path)"
    from commonscenes_amd.mesh_sdf import mesh_to_sdf, read_obj

    torch.cuda.set_device(0)
    if a.obj:
        pairs = [read_obj(p) for p in a.obj]
        src = list(a.obj)
    else:
        v, f = uv_sphere(a.synthetic)
        pairs = [(v * (1.0 - 0.01 * i), f) for i in range(max(1, a.batch))]
        src = f"uv_sphere({a.synthetic}) x {len(pairs)}"
    vs, fs = [v.cuda() for v, _ in pairs], [f.cuda() for _, f in pairs]
    kw = dict(res=a.res, bound=a.bound, normalize=not a.no_normalize, trunc=a.trunc, return_winding=True, return_meta=True)
    mesh_to_sdf(vs, fs, **kw)                      # first call: library load, allocator
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    sdf, w, meta = mesh_to_sdf(vs, fs, **kw)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    pairs_eval = float(sum(meta["faces"])) * a.res ** 3
    rec = {
        "source": src, "shape": list(sdf.shape), "faces": meta["faces"], "slices": meta["slices"],
        "centroid": [[round(x, 6) for x in c] for c in meta["centroid"].cpu().tolist()],
        "scale": [round(x, 6) for x in meta["scale"].cpu().tolist()],
        "inside_share": [round(float((s < 0).float().mean()), 5) for s in sdf],
        "winding_range": [round(float(w.min()), 4), round(float(w.max()), 4)],
        "device_ms": round(ms, 3), "device_ms_per_mesh": round(ms / len(vs), 3),
        "pair_evals_per_s": round(pairs_eval / (ms * 1e-3), 0),
        "trunc": a.trunc, "bound": a.bound, "normalize": not a.no_normalize,
    }
    if a.against:
        other = torch.from_numpy(np.asarray(np.load(a.against), np.float32)).reshape(sdf.shape).cuda()
        d = (sdf - other).abs()
        rec["against"] = {"file": a.against, "max_abs": float(d.max()), "mean_abs": float(d.mean())}
    if a.compare_host:
        vn = pairs[0][0]
        if not a.no_normalize:
            from commonscenes_amd.mesh_sdf import get_normalize_mesh
            vn = get_normalize_mesh(pairs[0][0], pairs[0][1])[0].cpu()
        sec = host_brute_force(vn, pairs[0][1], 8, a.bound)
        rec["host_brute_force"] = {"res": 8, "faces": int(pairs[0][1].shape[0]), "seconds": round(sec, 3),
                                   "pair_evals_per_s": round(pairs[0][1].shape[0] * 512 / sec, 0)}
    if a.out:
        np.save(a.out, sdf.cpu().numpy())
        rec["out"] = a.out
    print("MESH_TO_SDF " + json.dumps(rec))


if __name__ == "__main__":
    main()
