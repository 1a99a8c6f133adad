"""Deterministic synthetic weights and inputs (no checkpoints or datasets are reachable offline).

Values come from a counter-based integer hash (FNV-1a of the tensor name -> SplitMix64 per
element) mapped to uniform [-1, 1) with exact integer->float arithmetic, so the same tensors are
regenerated bit-identically in the build container (golden generation against the reference) and on
the GPU box (parity tests, bench) without shipping 1.65 GB of weights.  Zero-initialised reference
tensors are randomised like every other tensor, otherwise parity would be vacuous.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, Iterable, Tuple

import numpy as np
import torch

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _fnv1a(name: str) -> int:
    h = 0xCBF29CE484222325
    for b in name.encode():
        h ^= b
        h = (h * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def hash_uniform(name: str, n: int, seed: int = 111) -> np.ndarray:
    """n values in [-1, 1), float64, each exactly representable in fp32."""
    base = np.uint64((_fnv1a(name) ^ (seed * 0x9E3779B97F4A7C15)) & 0xFFFFFFFFFFFFFFFF)
    out = np.empty(n, dtype=np.float64)
    CH = 1 << 22
    with np.errstate(over="ignore"):
        for s in range(0, n, CH):
            e = min(n, s + CH)
            z = np.arange(s, e, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + base
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            z = z ^ (z >> np.uint64(31))
            k = (z >> np.uint64(40)).astype(np.int64)          # 24 bits
            out[s:e] = (2 * k - (1 << 24)).astype(np.float64) / float(1 << 24)
    return out


def tensor(name: str, shape: Tuple[int, ...], scale: float = 1.0, offset: float = 0.0, seed: int = 111) -> torch.Tensor:
    n = int(np.prod(shape)) if len(shape) else 1
    v = hash_uniform(name, n, seed) * scale + offset
    return torch.from_numpy(v.astype(np.float32).reshape(shape))


def _fan_in(shape: Tuple[int, ...]) -> int:
    f = 1
    for s in shape[1:]:
        f *= s
    return max(f, 1)


def _entry_params(name: str, shape, shapes, gain: float):
    """(scale, offset) of the uniform law for one state_dict entry; None for integer bookkeeping entries."""
    leaf = name.rsplit(".", 1)[-1]
    if leaf == "num_batches_tracked":
        return None
    if leaf == "running_mean":
        return 0.2, 0.0
    if leaf == "running_var":
        return 0.5, 1.0
    if "embedding" in name and leaf == "weight" and len(shape) == 2 and "quantize" in name:
        return 1.5, 0.0                                   # VQ codebook spread over the latent range
    if "embeddings" in name and leaf == "weight":
        return 1.0, 0.0
    if leaf == "weight" and len(shape) == 1:
        return 0.2, 1.0                                   # norm scale
    if leaf == "bias" and (".norm" in name or "in_layers.0" in name or "out_layers.0" in name
                           or name.endswith("out.0.bias") or _is_bn(name, shapes)):
        return 0.1, 0.0                                   # norm shift
    if leaf == "weight":
        return float(gain / np.sqrt(_fan_in(shape))), 0.0
    if leaf == "bias":
        wshape = shapes.get(name[:-4] + "weight", (shape[0], 1))
        return float(1.0 / np.sqrt(_fan_in(wshape))), 0.0
    return 1.0, 0.0


def tensor_device(name: str, shape: Tuple[int, ...], scale: float = 1.0, offset: float = 0.0, seed: int = 111,
                  device="cuda") -> torch.Tensor:
    """Same values as `tensor`, generated on the HIP device by cs_synth_fill (bit-identical)."""
    import ctypes as C
    from . import lib as L
    n = int(np.prod(shape)) if len(shape) else 1
    out = torch.empty(shape, dtype=torch.float32, device=device)
    base = (_fnv1a(name) ^ (seed * 0x9E3779B97F4A7C15)) & 0xFFFFFFFFFFFFFFFF
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(L.load().cs_synth_fill(out.data_ptr(), n, base, float(scale), float(offset), stream), "cs_synth_fill")
    return out


def synth_state_dict(shapes: "Dict[str, Tuple[int, ...]]", seed: int = 111, gain: float = 3.0 ** 0.5,
                     device: str = "cpu") -> "OrderedDict[str, torch.Tensor]":
    """Weights for a {name: shape} table.  Conv/Linear weights ~ U(-a, a) with a = gain/sqrt(fan_in)
    (variance preserving), biases ~ U(-1, 1)/sqrt(fan_in) of their layer, norm scales 1 + 0.2u,
    norm biases 0.1u, BatchNorm running_mean 0.2u, running_var 1 + 0.5u, embeddings U(-1, 1).
    device='cuda' generates the identical values with the cs_synth_fill kernel."""
    sd: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    on_dev = str(device).startswith("cuda")
    for name, shape in shapes.items():
        pr = _entry_params(name, shape, shapes, gain)
        if pr is None:
            sd[name] = torch.tensor(1, dtype=torch.long)
        elif on_dev:
            sd[name] = tensor_device(name, tuple(shape), pr[0], pr[1], seed, device)
        else:
            sd[name] = tensor(name, tuple(shape), pr[0], pr[1], seed)
    return sd


def _is_bn(name: str, shapes) -> bool:
    return (name[:-4] + "running_mean") in shapes


def gaussian_like(name: str, shape: Tuple[int, ...], seed: int = 111, scale: float = 1.0) -> torch.Tensor:
    """Approximately N(0, scale^2) samples (sum of 12 hash uniforms; every float64 operation below is
    exact or a single correctly-rounded IEEE op, so the result is platform independent)."""
    n = int(np.prod(shape))
    acc = np.zeros(n, dtype=np.float64)
    for k in range(12):
        acc += hash_uniform(f"{name}#{k}", n, seed)
    # each term is uniform[-1,1): variance 1/3, sum variance 4 -> divide by 2
    return torch.from_numpy((acc / 2.0 * float(scale)).astype(np.float32).reshape(shape))


def random_scene_graph(n_objects: int, seed: int = 111, n_obj_classes: int = 35, n_pred_classes: int = 16):
    """Synthetic SG-FRONT-like graph: O = n_objects + 2 nodes (last two: floor, _scene_),
    an `in` edge (predicate 0 here) from every node to `_scene_`, plus 2-6 typed edges per object.
    Returns objs (O,), triples (T,3) [s,p,o] int64, text_feats (O,512), rel_feats (T,512), z (O,64)."""
    O = n_objects + 2
    u = lambda tag, n: hash_uniform(f"graph:{tag}", n, seed)
    objs = ((u("objs", O) * 0.5 + 0.5) * (n_obj_classes - 2)).astype(np.int64) + 1
    objs[-2] = n_obj_classes - 1          # floor
    objs[-1] = 0                          # _scene_
    triples = []
    ne = ((u("nedges", n_objects) * 0.5 + 0.5) * 5).astype(np.int64) + 2
    tgt = u("targets", int(ne.sum()) + 1)
    prd = u("preds", int(ne.sum()) + 1)
    k = 0
    for i in range(n_objects):
        for _ in range(int(ne[i])):
            j = int((tgt[k] * 0.5 + 0.5) * (O - 1)) % (O - 1)
            if j == i:
                j = (j + 1) % (O - 1)
            p = int((prd[k] * 0.5 + 0.5) * (n_pred_classes - 1)) % (n_pred_classes - 1) + 1
            triples.append((i, p, j))
            k += 1
    for i in range(O - 1):
        triples.append((i, 0, O - 1))
    triples = np.asarray(triples, dtype=np.int64)
    T = triples.shape[0]

    def clip_like(tag, n):       # CLIP-like scale: ||f|| ~ 10 (no data-dependent normalisation:
        return gaussian_like(f"graph:{tag}", (n, 512), seed, scale=10.0 / float(np.sqrt(512.0)))  # keeps it exact)

    return dict(objs=torch.from_numpy(objs), triples=torch.from_numpy(triples),
                text_feats=clip_like("text", O), rel_feats=clip_like("rel", T),
                z=gaussian_like("graph:z", (O, 64), seed))


def sdf_volume(variant: int = 0, res: int = 64) -> torch.Tensor:
    """An analytic SDF-like volume [1, 1, res, res, res] (fp32): the signed distance to the union of a sphere and a box
    on the cube [-1, 1]^3, clipped to +-0.2 like the truncated SDFs SDFusion encodes.  Every float64 operation is exact
    or a single correctly-rounded IEEE op, so the result is platform independent."""
    c = (np.arange(res, dtype=np.float64) + 0.5) * (2.0 / res) - 1.0
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    (sc, sr), (bc, bh) = [(((0.1, -0.05, 0.0), 0.5), ((-0.2, 0.1, 0.1), (0.3, 0.2, 0.4))),
                          (((-0.15, 0.2, 0.05), 0.35), ((0.15, -0.1, -0.05), (0.45, 0.15, 0.3)))][variant % 2]
    ds = np.sqrt((x - sc[0]) ** 2 + (y - sc[1]) ** 2 + (z - sc[2]) ** 2) - sr
    q = [np.abs(v - o) - h for v, o, h in zip((x, y, z), bc, bh)]
    outside = np.sqrt(np.maximum(q[0], 0.0) ** 2 + np.maximum(q[1], 0.0) ** 2 + np.maximum(q[2], 0.0) ** 2)
    db = outside + np.minimum(np.maximum(q[0], np.maximum(q[1], q[2])), 0.0)
    d = np.clip(np.minimum(ds, db), -0.2, 0.2)
    return torch.from_numpy(d.astype(np.float32).reshape(1, 1, res, res, res))


def iou_case(thres: float):
    """Two batches of three 64^3 volumes for the IoU counts (tests/golden/eval_losses.npz, fixture (c)): sample 0 =
    sdf_volume(0) against sdf_volume(1) with one NaN voxel and one voxel exactly at fp32(thres); sample 1 = the two volumes
    swapped; sample 2 = two all-free volumes (empty union)."""
    v0, v1 = sdf_volume(0), sdf_volume(1)
    a = torch.cat([v0, v1, torch.full_like(v0, 0.2)], dim=0)
    b = torch.cat([v1, v0, torch.full_like(v0, 0.15)], dim=0).clone()
    b[0, 0, 10, 20, 30] = float("nan")
    b[0, 0, 40, 41, 42] = float(np.float32(thres))
    b[2] += float(np.float32(max(thres, 0.0)))          # stays free for every threshold
    return a, b


def _box_mesh(size):
    """an axis-aligned box of (l, h, w) standing on y = 0, centred in x / z: 8 vertices, 12 outward triangles"""
    l, h, w = [float(s) for s in size]
    v = np.asarray([[l / 2 * i, h * j, w / 2 * k] for i in (-1, 1) for j in (0, 1) for k in (-1, 1)], dtype=np.float32)
    f = np.asarray([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                    [1, 5, 7], [1, 7, 3]], dtype=np.int64)
    return torch.from_numpy(v), torch.from_numpy(f)


def _ellipsoid_mesh(size, rings: int = 6, segments: int = 8):
    """an ellipsoid inscribed in the same box: a latitude / longitude mesh, poles on the y axis"""
    l, h, w = [float(s) for s in size]
    vs = [[0.0, 0.0, 0.0]]
    for r in range(1, rings):
        th = np.pi * r / rings
        for s in range(segments):
            ph = 2 * np.pi * s / segments
            vs.append([l / 2 * np.sin(th) * np.cos(ph), h / 2 - h / 2 * np.cos(th), w / 2 * np.sin(th) * np.sin(ph)])
    vs.append([0.0, h, 0.0])
    top = len(vs) - 1
    ring = lambda r, s: 1 + (r - 1) * segments + s % segments
    fs = []
    for s in range(segments):
        fs.append([0, ring(1, s), ring(1, s + 1)])
        fs.append([top, ring(rings - 1, s + 1), ring(rings - 1, s)])
        for r in range(1, rings - 1):
            fs.append([ring(r, s), ring(r + 1, s), ring(r + 1, s + 1)])
            fs.append([ring(r, s), ring(r + 1, s + 1), ring(r, s + 1)])
    return torch.from_numpy(np.asarray(vs, dtype=np.float32)), torch.from_numpy(np.asarray(fs, dtype=np.int64))


def furniture_table(labels, per_category: int = 8, seed: int = 111):
    """A small synthetic furniture library (3D-FUTURE is not reachable offline): per label `per_category` models,
    alternately boxes and ellipsoids, sizes hash-uniform in [0.2, 2.2) -> {label: [(id, (l, h, w), verts, faces), ...]}, the
    argument of scene_library.FurnitureLibrary.from_meshes."""
    table = OrderedDict()
    for lab in labels:
        lab = lab.strip("\n")
        sz = hash_uniform(f"furniture:{lab}", per_category * 3, seed).reshape(per_category, 3) + 1.2
        table[lab] = []
        for k in range(per_category):
            size = [float(np.float32(x)) for x in sz[k]]
            v, f = _box_mesh(size) if k % 2 == 0 else _ellipsoid_mesh(size)
            table[lab].append((f"{lab}-{k:03d}", size, v, f))
    return table


def furniture_library(labels, per_category: int = 8, seed: int = 111):
    from .scene_library import FurnitureLibrary
    return FurnitureLibrary.from_meshes(furniture_table(labels, per_category, seed))


def write_shape_library(root, labels, per_category: int = 4, seed: int = 111) -> None:
    """the same models as `root/<label>/<id>.ply`: the folder layout scene_library.ShapeLibrary reads"""
    import os
    from .scene_library import write_ply
    for lab, entries in furniture_table(labels, per_category, seed).items():
        os.makedirs(os.path.join(root, lab), exist_ok=True)
        for mid, _, v, f in entries:
            write_ply(os.path.join(root, lab, mid + ".ply"), v, f, binary=True)
