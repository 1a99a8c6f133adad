"""The diversity table of scripts/eval_3dfront.py (--evaluate_diversity, :577-762) and the two tables of
scripts/consistency_check.py (Chamfer :68-101; CLIP :82-90 over clip.py's image features) behind the reference's names.

Both tables are the same three device steps -- resample a ragged set of vertex clouds (`sample_points`,
helpers/util.py:31-44), normalise them (`normalize`, eval_3dfront.py:783-796), take the Chamfer distance of a list of pairs --
and here each step is one launch over ALL clouds / pairs (csrc/cs_diversity.hip: cs_cloud_resample, csrc/cs_pairwise.hip:
cs_chamfer_pairlist).  The random rows are drawn on the CPU with the reference's own calls in the reference's order, so
`torch.manual_seed(k)` selects the rows the reference selects.  The small statistics (standard deviation of the
denormalised boxes, circular standard deviation of the angles, the per-category means) are float64 numpy on the host after one
read-back each.

Import swap for the scripts:
    from helpers.util import sample_points                      -> from commonscenes_amd.diversity import sample_points
    from helpers.metrics_3dfront import estimate_angular_std    -> from commonscenes_amd.diversity import estimate_angular_std
    the inline `normalize` of eval_3dfront.py                   -> from commonscenes_amd.diversity import normalize

The marching-cubes vertex order is unpinned against PyMCubes (mesh.py): on the same SDF the sampled ROWS differ from the
reference's, so a table agrees with the reference's statistically, not per digit.
"""
from __future__ import annotations

from cmath import phase, rect
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import ops

Tensor = torch.Tensor

CATEGORIES = ("bed", "nightstand", "wardrobe", "chair", "table", "cabinet", "lamp", "sofa", "shelf", "tv_stand")
# helpers/util.py:570-571: the statistics batch_torch_denormalize_box_params falls back to without a file
BOX_MEAN = (1.3827214, 1.309359, 0.9488993, -0.12464812, 0.6188591, -0.54847)
BOX_STD = (1.7797655, 1.657638, 0.8501885, 1.9160025, 2.0038228, 0.70099753)


def _device() -> torch.device:
    return torch.device("cuda", torch.cuda.current_device())


# ----------------------------------------------------------------------------------------------------------------------
# sample_points / normalize
# ----------------------------------------------------------------------------------------------------------------------
def _counts(points_list) -> List[int]:
    counts = []
    for i, pc in enumerate(points_list):
        if not isinstance(pc, torch.Tensor) or pc.dim() != 2 or pc.shape[1] != 3:
            raise ValueError(f"cloud {i} must be an [n, 3] tensor")
        if pc.shape[0] == 0:
            raise ValueError(f"cloud {i} is empty: nothing to sample from")
        counts.append(int(pc.shape[0]))
    return counts


def draw_indices(counts: Sequence[int], num: int, generator: Optional[torch.Generator] = None) -> Tensor:
    """The rows helpers/util.py:31-44 selects, [N, num] int64 on the CPU: per cloud, in list order, randperm(n)[:num] when
    n >= num, else randint(n, size=(num,)) -- from the global CPU generator, or from `generator`."""
    kw = {} if generator is None else {"generator": generator}
    rows = []
    for i, n in enumerate(counts):
        if n < 1:
            raise ValueError(f"cloud {i} is empty: nothing to sample from")
        rows.append(torch.randperm(n, **kw)[:num] if n >= num else torch.randint(n, size=(num,), **kw))
    return torch.stack(rows) if rows else torch.zeros((0, num), dtype=torch.int64)


def _packed(points_list, counts):
    """(verts [V, 3] on the device, first row of every cloud).  A list that is the split of ONE packed float32 device buffer
    (what marching_cubes / sdf_to_mesh return) is read in place; anything else is packed once."""
    p0 = points_list[0]
    if all(pc.is_cuda and pc.dtype == torch.float32 and pc.is_contiguous() and pc.device == p0.device
           and pc.untyped_storage().data_ptr() == p0.untyped_storage().data_ptr() for pc in points_list):
        offs = [int(pc.storage_offset()) for pc in points_list]
        base = min(offs)
        if all((o - base) % 3 == 0 for o in offs):
            first = [(o - base) // 3 for o in offs]
            rows = max(f + n for f, n in zip(first, counts))
            verts = torch.empty(0, dtype=torch.float32, device=p0.device).set_(p0.untyped_storage(), base, (rows, 3), (3, 1))
            return verts, first
    dev = p0.device if p0.is_cuda else _device()
    verts = torch.cat([pc.to(torch.float32) for pc in points_list]).to(dev)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]]).tolist()
    return verts, first


def _indices_for(counts, num, generator, indices):
    if num < 1:
        raise ValueError("num must be at least 1")
    if indices is None:
        return draw_indices(counts, num, generator)
    if not isinstance(indices, torch.Tensor) or not indices.is_cuda:
        indices = torch.as_tensor(np.asarray(indices) if not isinstance(indices, torch.Tensor) else indices)
        if tuple(indices.shape) != (len(counts), num):
            raise ValueError(f"indices must be [{len(counts)}, {num}], got {tuple(indices.shape)}")
    return indices


def sample_points_packed(verts: Tensor, counts: Sequence[int], num: int, generator: Optional[torch.Generator] = None,
                         indices=None, normalize: bool = False, first: Optional[Sequence[int]] = None) -> Tensor:
    """`sample_points` over clouds packed in verts [V, 3] (cloud i = counts[i] rows, consecutive unless `first` says where each
    starts) -> ONE [N, num, 3] device tensor, one upload of the [N, num] int32 rows and one launch.  `indices` supplies the
    rows and draws nothing; `normalize` applies eval_3dfront.py:783-796 to every sampled cloud in the same launch."""
    counts = [int(c) for c in counts]
    for i, n in enumerate(counts):
        if n < 1:
            raise ValueError(f"cloud {i} is empty: nothing to sample from")
    idx = _indices_for(counts, int(num), generator, indices)
    if first is None:
        first = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64).tolist() if counts else []
    return ops.cloud_resample(verts, first, counts, int(num), idx=idx, normalize=normalize)


def _sample(points_list, num, generator, indices, normalize) -> Tensor:
    points_list = list(points_list)
    counts = _counts(points_list)
    idx = _indices_for(counts, int(num), generator, indices)      # (drawn before anything touches the device)
    if not points_list:
        return torch.empty((0, int(num), 3), dtype=torch.float32, device=_device())
    verts, first = _packed(points_list, counts)
    return ops.cloud_resample(verts, first, counts, int(num), idx=idx, normalize=normalize)


def sample_points(points_list, num: int, generator: Optional[torch.Generator] = None, indices=None) -> List[Tensor]:
    """helpers/util.py:31-44: every cloud of the list resampled to `num` rows (a random subset when it has at least `num`, rows
    drawn with replacement otherwise).  Returns a list of [num, 3] views of one [N, num, 3] device tensor."""
    return list(_sample(points_list, num, generator, indices, False).unbind(0))


def sample_and_normalize(points_list, num: int, generator: Optional[torch.Generator] = None, indices=None) -> Tensor:
    """normalize(sample_points(...)) in one launch -> [N, num, 3] (what the tables use)."""
    return _sample(points_list, num, generator, indices, True)


def normalize(vertices: Tensor, scale=1) -> Tensor:
    """eval_3dfront.py:783-796 on a [P, 3] cloud or a batch [N, P, 3] of them (each normalised on its own): every axis
    centred on the middle of its extent and divided by its maximum.  A new tensor of the same shape (the reference also
    shifts its argument in place; nobody reads it afterwards)."""
    if not isinstance(vertices, torch.Tensor) or vertices.dim() not in (2, 3) or vertices.shape[-1] != 3 \
            or vertices.shape[-2] < 1:
        raise ValueError("normalize takes a [P, 3] or [N, P, 3] tensor with P >= 1")
    n = 1 if vertices.dim() == 2 else int(vertices.shape[0])
    p = int(vertices.shape[-2])
    flat = vertices.reshape(n * p, 3)
    out = ops.cloud_resample(flat, [i * p for i in range(n)], [p] * n, p, idx=None, normalize=True).reshape(vertices.shape)
    return out if scale == 1 else out * scale


# ----------------------------------------------------------------------------------------------------------------------
# the three diversity figures
# ----------------------------------------------------------------------------------------------------------------------
def chamfer_pairs(clouds: Tensor, pairs) -> Tensor:
    """[npairs] fp32: mean_k min_l |a_k - b_l|^2 + mean_l min_k |a_k - b_l|^2 of clouds[i], clouds[j] for every listed (i, j);
    one launch, bit-equal to shape_metrics.pairwise_cd(clouds, clouds)[i, j]."""
    return ops.chamfer_pairlist(clouds, pairs)


def shape_diversity(shapes_sample: Tensor) -> np.ndarray:
    """shapes_sample [O, K, P, 3] (object, run) -> [O] float64: the mean over k of chamfer(run k, run k + 1), as
    eval_3dfront.py:688-699.  One launch for all O * (K - 1) pairs, one read-back."""
    if not isinstance(shapes_sample, torch.Tensor) or shapes_sample.dim() != 4 or shapes_sample.shape[-1] != 3:
        raise ValueError("shape_diversity takes [O, K, P, 3]")
    O, K, P = (int(s) for s in shapes_sample.shape[:3])
    if K < 2:
        raise ValueError("diversity needs at least two runs per object")          # eval_3dfront.py:448-449
    if O == 0:
        return np.zeros((0,), np.float64)
    base = np.arange(O, dtype=np.int64)[:, None] * K + np.arange(K - 1, dtype=np.int64)[None, :]
    pairs = np.stack([base, base + 1], axis=-1).reshape(-1, 2)
    d = chamfer_pairs(shapes_sample.reshape(O * K, P, 3), pairs)
    return d.cpu().numpy().astype(np.float64).reshape(O, K - 1).mean(axis=1)


def angular_std(degs) -> np.ndarray:
    """`estimate_angular_std` (helpers/metrics_3dfront.py:40-47) for every row of degs [O, K] -> [O] float64: the root mean
    square angular distance to the row's circular mean.  The mean is taken with the reference's own complex sum (its order
    is part of the result); the distances are numpy float64 over all rows at once."""
    d = np.asarray(degs, np.float64)
    if d.ndim != 2 or d.shape[1] < 1:
        raise ValueError("angular_std takes [O, K] with K >= 1")
    O, K = d.shape
    m = np.empty((O,), np.float64)
    for o in range(O):
        m[o] = np.rad2deg(phase(sum(rect(1, np.deg2rad(x)) for x in d[o]) / K)) % 360.
    a, b = np.deg2rad(d % 360.), np.deg2rad(m % 360.)[:, None]
    dot = np.cos(a) * np.cos(b) + np.sin(a) * np.sin(b)
    dist = np.rad2deg(np.arccos(np.clip(dot, -1, 1))) % 360.
    return np.sqrt(np.sum(dist ** 2, axis=1) / K)


def estimate_angular_std(degs) -> float:
    """helpers/metrics_3dfront.py:44-47 for one set of angles."""
    return float(angular_std(np.asarray(degs, np.float64).reshape(1, -1))[0])


def box_stats(file=None):
    """(mean [6], std [6]) float64: the constants of helpers/util.py:570-571, or the first six columns of the two rows of a
    statistics file (np.loadtxt layout)."""
    if file is None:
        return np.array(BOX_MEAN, np.float64), np.array(BOX_STD, np.float64)
    stats = np.loadtxt(file)
    return stats[0][:6].astype(np.float64), stats[1][:6].astype(np.float64)


def box_std(boxes_runs, file=None, scale=3) -> np.ndarray:
    """boxes_runs [O, K, 6] normalised box parameters of K runs -> [O, 6] float64: the unbiased standard deviation over the
    runs of the boxes denormalised as batch_torch_denormalize_box_params does (eval_3dfront.py:665-668).  One read-back."""
    b = boxes_runs.detach().cpu().numpy() if isinstance(boxes_runs, torch.Tensor) else np.asarray(boxes_runs)
    if b.ndim != 3 or b.shape[2] != 6:
        raise ValueError("box_std takes [O, K, 6]")
    if b.shape[1] < 2:
        raise ValueError("diversity needs at least two runs per object")
    mean, std = box_stats(file)
    den = (b.astype(np.float64) * std[None, None, :]) / scale + mean[None, None, :]
    return den.std(axis=1, ddof=1)


# ----------------------------------------------------------------------------------------------------------------------
# the table
# ----------------------------------------------------------------------------------------------------------------------
def _verts_of(run) -> List[Tensor]:
    if hasattr(run, "verts_list"):
        return list(run.verts_list())
    return list(run)


class DiversityMeter:
    """Accumulates what eval_3dfront.py:577-719 accumulates over the scenes and reports what :735-762 prints.

    classes: name -> class id (the dataset's `classes`).  Nodes of class 0 and `floor` carry no shape and are skipped
    (:636).  A shape's category is that of the node's OWN index; the reference compares the position among the kept nodes
    with the unfiltered node index (:700-719) -- the two agree whenever the skipped nodes trail the list, as they do in
    SG-FRONT.  Box and angle deviations are taken over all nodes, as the reference takes them."""

    def __init__(self, classes: Dict[str, int], categories: Sequence[str] = CATEGORIES, points: int = 5000, file=None):
        self.classes = {str(k).strip(): int(v) for k, v in classes.items()}
        self.classes_r = {v: k for k, v in self.classes.items()}
        self.categories = tuple(categories)
        self.points, self.file = int(points), file
        self.shape: List[float] = []
        self.by_category: Dict[str, List[float]] = {c: [] for c in self.categories}
        self.boxes: List[np.ndarray] = []
        self.angles: List[float] = []

    def kept_nodes(self, dec_objs) -> List[int]:
        objs = [int(c) for c in (dec_objs.tolist() if hasattr(dec_objs, "tolist") else dec_objs)]
        return [i for i, c in enumerate(objs) if c != 0 and self.classes_r.get(c) != "floor"]

    def add_numbers(self, dec_objs, shape_div=None, box_std_rows=None, angle_stds=None) -> None:
        """The meter's arithmetic on ready per-object numbers: shape_div holds one figure per KEPT node, in node order;
        box_std_rows [O, 6] and angle_stds [O] one per node."""
        objs = [int(c) for c in (dec_objs.tolist() if hasattr(dec_objs, "tolist") else dec_objs)]
        keep = self.kept_nodes(objs)
        if shape_div is not None:
            shape_div = np.asarray(shape_div, np.float64).reshape(-1)
            if len(shape_div) != len(keep):
                raise ValueError(f"{len(shape_div)} shape figures for {len(keep)} shaped nodes")
            for node, v in zip(keep, shape_div):
                self.shape.append(float(v))
                for cat in self.categories:
                    if cat in self.classes and self.classes[cat] == objs[node]:
                        self.by_category[cat].append(float(v))
        if box_std_rows is not None:
            rows = np.asarray(box_std_rows, np.float64)
            if rows.ndim != 2 or rows.shape[1] != 6:
                raise ValueError("box_std_rows must be [O, 6]")
            self.boxes += list(rows)
        if angle_stds is not None:
            self.angles += [float(v) for v in np.asarray(angle_stds, np.float64).reshape(-1)]

    def shapes_tensor(self, dec_objs, shapes_runs, shape_nodes=None, generator=None) -> Tensor:
        """[kept nodes, K, points, 3]: `shapes_runs` as it is when it is that tensor already; otherwise K Meshes / vertex
        lists / SDF batches [S, 1, n, n, n] (meshed here, all runs in one call, render_all=True), resampled and normalised in
        one launch with the rows drawn run by run over the whole list, as :592 draws them.  shape_nodes[r] is the node of
        shape r (default: r, as the reference indexes them)."""
        keep = self.kept_nodes(dec_objs)
        if isinstance(shapes_runs, torch.Tensor) and shapes_runs.dim() == 4:
            if shapes_runs.shape[0] != len(keep) or shapes_runs.shape[-1] != 3:
                raise ValueError(f"a ready shapes tensor must be [{len(keep)}, K, P, 3], got {tuple(shapes_runs.shape)}")
            if shapes_runs.shape[1] < 2:
                raise ValueError("diversity needs at least two runs per object")
            return shapes_runs
        runs = list(shapes_runs)
        K = len(runs)
        if K < 2:
            raise ValueError("diversity needs at least two runs per object")
        if all(isinstance(r, torch.Tensor) and r.dim() == 5 for r in runs):
            from .mesh import sdf_to_mesh
            S = int(runs[0].shape[0])
            if any(int(r.shape[0]) != S for r in runs):
                raise ValueError("every run must hold the same objects")
            verts = _verts_of(sdf_to_mesh(torch.cat([r.to(_device()) for r in runs]), render_all=True))
        else:
            per = [_verts_of(r) for r in runs]
            S = len(per[0])
            if any(len(v) != S for v in per):
                raise ValueError("every run must hold the same objects")
            verts = [v for run in per for v in run]
        nodes = list(range(S)) if shape_nodes is None else [int(i) for i in shape_nodes]
        if len(nodes) != S:
            raise ValueError(f"shape_nodes names {len(nodes)} nodes for {S} shapes")
        row_of = {node: r for r, node in enumerate(nodes)}
        missing = [i for i in keep if i not in row_of]
        if missing:
            raise ValueError(f"nodes {missing} carry a shape class but no shape was given for them")
        pts = sample_and_normalize(verts, self.points, generator=generator).reshape(K, S, self.points, 3)
        sel = torch.as_tensor([row_of[i] for i in keep], dtype=torch.int64, device=pts.device)
        return pts.index_select(1, sel).permute(1, 0, 2, 3).contiguous()

    def add_scene(self, dec_objs, boxes_runs, angles_runs, shapes_runs, shape_nodes=None, generator=None) -> dict:
        """One scene's K runs.  boxes_runs: K [O, 6] tensors (or [O, K, 6]); angles_runs: the K [O, 24] score tensors
        (angle = argmax / 24 * 360, :655) or None; shapes_runs: see shapes_tensor.  Returns the scene's own numbers."""
        out = {"nodes": self.kept_nodes(dec_objs)}
        shape = box = ang = None
        if shapes_runs is not None:
            ss = self.shapes_tensor(dec_objs, shapes_runs, shape_nodes, generator)
            shape = shape_diversity(ss) if ss.shape[0] else np.zeros((0,), np.float64)
        if boxes_runs is not None:
            b = boxes_runs if isinstance(boxes_runs, torch.Tensor) and boxes_runs.dim() == 3 \
                else torch.stack([torch.as_tensor(x) for x in boxes_runs], 1)
            box = box_std(b, file=self.file)
        if angles_runs is not None:
            scores = torch.stack([torch.as_tensor(x) for x in angles_runs], 1)          # [O, K, 24]
            if scores.shape[1] < 2:
                raise ValueError("diversity needs at least two runs per object")
            degs = torch.argmax(scores, dim=2).cpu().numpy() / 24. * 360.
            ang = angular_std(degs)
        self.add_numbers(dec_objs, shape, box, ang)
        out.update(shape=shape, box_std=box, angle_std=ang)
        return out

    def summary(self) -> dict:
        mean = lambda v: float(np.mean(v)) if len(v) else None
        box = np.mean(np.stack(self.boxes), axis=0) if self.boxes else None
        return {
            "objects": len(self.shape), "shape": mean(self.shape),
            "categories": {c: {"n": len(v), "shape": mean(v)} for c, v in self.by_category.items()},
            "box_size": None if box is None else float(np.mean(box[:3])),
            "box_location": None if box is None else float(np.mean(box[3:])),
            "angle": mean(self.angles),
        }


@torch.no_grad()
def scene_diversity(model, scene: dict, num_samples: int = 3, ddim_steps: int = 100, points: int = 5000, zs=None, x_Ts=None,
                    meter: Optional[DiversityMeter] = None, generator=None) -> dict:
    """The diversity block for one scene: its `num_samples` runs go out as ONE VAE.sample_box_and_shape_many call (K copies of
    the scene, run k with zs[k] / x_Ts[k] when given), one sdf_to_mesh over all K * S shaped objects, one resample launch
    and one Chamfer launch.  `scene` holds sample_box_and_shape's arguments by name (dec_objs, dec_triplets, dec_sdfs,
    encoded_dec_text_feat, encoded_dec_rel_feat[, attributes]).  Returns {'shape' [S], 'box_std' [O, 6], 'angle_std' [O] |
    None, 'shape_nodes'} as float64 numpy; with a `meter`, 'shape' covers the nodes the meter keeps and the meter is fed."""
    from .mesh import sdf_to_mesh
    K = int(num_samples)
    if K < 2:
        raise ValueError("diversity needs at least two runs per object")
    for name, v in (("zs", zs), ("x_Ts", x_Ts)):
        if v is not None and len(v) != K:
            raise ValueError(f"{name} must hold one entry per run ({K})")
    scs = []
    for k in range(K):
        sc = dict(scene)
        if zs is not None:
            sc["z"] = zs[k]
        if x_Ts is not None:
            sc["x_T"] = x_Ts[k]
        scs.append(sc)
    outs = model.sample_box_and_shape_many(scs, gen_shape=True, ddim_steps=ddim_steps)
    with_angles = isinstance(outs[0][0], (tuple, list))
    boxes = [o[0][0] if with_angles else o[0] for o in outs]
    angles = [o[0][1] for o in outs] if with_angles else None
    sdfs = torch.cat([o[1] for o in outs])
    S = int(outs[0][1].shape[0])
    # the shaped nodes, as the model picks them: those whose ground-truth SDF is not all zero
    dec_sdfs = scene["dec_sdfs"]
    shape_nodes = torch.unique(torch.where(torch.ne(dec_sdfs, torch.zeros_like(dec_sdfs[0])))[0]).tolist()
    verts = _verts_of(sdf_to_mesh(sdfs, render_all=True))
    runs = [verts[k * S:(k + 1) * S] for k in range(K)]
    if meter is not None:
        res = meter.add_scene(scene["dec_objs"], boxes, angles, runs, shape_nodes=shape_nodes, generator=generator)
        res["shape_nodes"] = res.pop("nodes")
        return res
    pts = sample_and_normalize(verts, points, generator=generator).reshape(K, S, points, 3)
    res = {"shape": shape_diversity(pts.permute(1, 0, 2, 3).contiguous()), "box_std": box_std(torch.stack(boxes, 1)),
           "angle_std": None, "shape_nodes": shape_nodes}
    if angles is not None:
        res["angle_std"] = angular_std(torch.argmax(torch.stack(angles, 1), dim=2).cpu().numpy() / 24. * 360.)
    return res


# ----------------------------------------------------------------------------------------------------------------------
# consistency
# ----------------------------------------------------------------------------------------------------------------------
def _group(dist: np.ndarray, categories, key: str = "chamfer") -> dict:
    table: Dict[str, List[float]] = {}
    for c, v in zip(categories, dist):
        table.setdefault(str(c), []).append(float(v))
    out = {c: {"pairs": len(v), key: float(np.mean(np.array(v, np.float64)))} for c, v in table.items()}
    n = len(dist)
    out["total"] = {"pairs": n, key: float(np.sum(np.asarray(dist, np.float64)) / n) if n else None}
    return out


def consistency_table(clouds: Tensor, pairs, categories: Sequence[str]) -> dict:
    """consistency_check.py:78-101 without its CLIP half: the Chamfer distance of every listed pair of the sampled clouds
    [M, P, 3] (one launch), averaged per category (categories[k] names pair k) and in total, in float64."""
    pairs = np.asarray(pairs.cpu() if isinstance(pairs, torch.Tensor) else pairs, np.int64).reshape(-1, 2)
    if len(categories) != len(pairs):
        raise ValueError(f"{len(categories)} category names for {len(pairs)} pairs")
    if "total" in [str(c) for c in categories]:
        raise ValueError("'total' is the table's own row")
    dist = chamfer_pairs(clouds, pairs).cpu().numpy().astype(np.float64) if len(pairs) else np.zeros((0,), np.float64)
    return _group(dist, categories)


def clip_consistency_table(features: Tensor, pairs, categories: Sequence[str]) -> dict:
    """consistency_check.py:82-90, the `CLIP AVG` table: torch.norm(feature_a - feature_b) of every listed pair of the
    image features [N, E] (clip.CLIP.encode_image of the rendered object views) in one launch (cs_feature_pair_l2), averaged
    per category (categories[k] names pair k) and in total as sum / count, in float64."""
    from .clip import feature_pair_l2
    pairs = np.asarray(pairs.cpu() if isinstance(pairs, torch.Tensor) else pairs, np.int64).reshape(-1, 2)
    if len(categories) != len(pairs):
        raise ValueError(f"{len(categories)} category names for {len(pairs)} pairs")
    if "total" in [str(c) for c in categories]:
        raise ValueError("'total' is the table's own row")
    dist = feature_pair_l2(features, pairs).cpu().numpy().astype(np.float64) if len(pairs) else np.zeros((0,), np.float64)
    return _group(dist, categories, key="clip")


def consistency_from_meshes(verts_list, pairs, categories: Sequence[str], points: int = 5000, seed: int = 47) -> dict:
    """The table from the meshes' vertex lists: every cloud is resampled to `points` rows from a fresh CPU generator seeded
    `seed` (the script reseeds 47 before each cloud, :70 / :75), all clouds in one launch; no normalisation, as in the
    script."""
    verts_list = list(verts_list)
    counts = _counts(verts_list)
    idx = torch.stack([draw_indices([n], points, torch.Generator().manual_seed(seed))[0] for n in counts]) if counts \
        else torch.zeros((0, points), dtype=torch.int64)
    pairs_h = np.asarray(pairs, np.int64).reshape(-1, 2)
    if len(categories) != len(pairs_h):
        raise ValueError(f"{len(categories)} category names for {len(pairs_h)} pairs")
    if len(pairs_h) and (pairs_h.min() < 0 or pairs_h.max() >= len(counts)):
        raise ValueError(f"a pair names a mesh outside [0, {len(counts)})")
    clouds = _sample(verts_list, points, None, idx, False)
    return consistency_table(clouds, pairs_h, categories)


def read_obj_vertices(path) -> Tensor:
    """The `v x y z` lines of a Wavefront OBJ file as a float32 [n, 3] tensor, in file order.  (trimesh.load, which the
    script uses, also merges duplicate vertices; this reader does not.)"""
    rows = []
    with open(path) as fh:
        for line in fh:
            t = line.split()
            if len(t) >= 4 and t[0] == "v":
                rows.append([float(t[1]), float(t[2]), float(t[3])])
    return torch.tensor(rows, dtype=torch.float32).reshape(-1, 3)
