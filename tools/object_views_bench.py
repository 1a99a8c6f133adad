#!/usr/bin/env python
"""Report-only timing of the per-object views (commonscenes_amd/object_views.py, csrc/cs_view.hip): `render_meshes` for 32
marching-cubes meshes (synth.sdf_volume at 64^3, level 0.02) at 256 x 256, whole and split per stage (the stages with the
normalisation get_current_visuals_v2 asks for).  No gate: no reference renderer can run next to it.

    python tools/object_views_bench.py [--out profiles/object_views.txt] [--meshes 32] [--size 256] [--iters 20]
"""
import argparse
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[len(ts) // 2] * 1e3, ts[0] * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "object_views.txt"))
    ap.add_argument("--meshes", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    from commonscenes_amd import object_views as OV, synth
    from commonscenes_amd.mesh import sdf_to_mesh
    sdf = torch.cat([synth.sdf_volume(k % 2, 64).roll(k // 2, dims=2 + k % 3) for k in range(a.meshes)]).cuda()
    meshes = sdf_to_mesh(sdf, render_all=True)
    r = OV.init_mesh_renderer(image_size=a.size, dist=1.7, elev=20, azim=20, device="cuda")
    dev = torch.device("cuda", torch.cuda.current_device())
    pk = OV._Packed(meshes, dev)
    pr = r.project(pk, True)
    nrm = OV.vertex_normals(pk, pr["world"])
    keys, _ = r.raster(pk, pr["screen"], pr["zview"])
    rows = [
        ("render_meshes (pack + all stages)", lambda: OV.render_meshes(r, meshes)),
        ("  pack (torch: cat, face offsets)", lambda: OV._Packed(meshes, dev)),
        ("  normalise + project", lambda: r.project(pk, True)),
        ("  vertex normals", lambda: OV.vertex_normals(pk, pr["world"])),
        ("  rasterise", lambda: r.raster(pk, pr["screen"], pr["zview"])),
        ("  resolve + shade", lambda: r.shade(pk, keys, pr["world"], nrm, pr["screen"], pr["zview"])),
        ("normalize_meshes alone", lambda: OV.normalize_meshes(meshes)),
    ]
    out = r.render_all(pk, True)
    covered = int((out["pix_to_face"] >= 0).sum())
    lines = [f"object views: {a.meshes} marching-cubes meshes (64^3), {pk.V} vertices, {pk.F} faces, {a.size} x {a.size}, "
             f"{covered} covered pixels, dropped {int(out['dropped'].sum())}",
             f"device: {torch.cuda.get_device_name(0)}; wall-clock per call incl. launch and allocation, median / best of "
             f"{a.iters} (ms)"]
    for name, fn in rows:
        med, best = timed(fn, a.iters)
        lines.append(f"{name:<36s} {med:9.3f} {best:9.3f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
