"""Generated objects -> one scene mesh -> the 256x256 top-down view, on the MI355X.

The reference does this on the host right after sampling (helpers/visualize_scene.py:378-461 `render_v2_full`):
`get_generated_models_v2` (helpers/util.py:298-332) meshes the SDFs, inverts each mesh (`pytorch3d_to_trimesh`, :260-267),
colours it and fits it into its box (`fit_shapes_to_box_v2`, :158-189); `create_floor` (visualize_scene.py:57-81) adds the
floor quad; `render_img` (:85-116) renders the top-down image its FID / KID script consumes.  It needs trimesh and pyrender,
neither of which is in this image.  Here the meshes stay on the device: csrc/cs_scene.hip fits all boxes in one launch,
writes the scene buffers in one pass and rasterises them (exact integer coverage, one 64-bit atomic min per pixel).

The names mirror the reference's so that a script swaps the import.  What differs, on purpose:
  * meshes are `TriMesh` records of device tensors (vertices, faces, vertex_colors), not trimesh objects;
  * `render_boxes=True` draws this package's own tube markers (csrc/cs_scene_lib.hip: trimesh.creation.cylinder's vertex order
    cannot be pinned without trimesh); `get_generated_models_v2` still raises on it, `assemble_scene` is the marker path;
  * export is plain-text OBJ with vertex colours (no glb);
  * the shading of `render_topdown` is this package's (base colour x (0.3 + 0.7 max(0, n_y))): pyrender's lights cannot be
    pinned without pyrender.  Coverage, depth and object ids follow the reference's camera exactly.
Like the reference, colours are consumed with `next()` by the non-skipped objects: the k-th shaped object takes `colors[k]`.
"""
from __future__ import annotations

import colorsys
import os
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import lib as L
from .mesh import Meshes, sdf_to_mesh
from .ops import _stream

Tensor = torch.Tensor
ZNEAR = 0.05                       # pyrender.PerspectiveCamera's default znear
FLOOR_RGB = (0.4, 0.4, 0.4)        # trimesh's default face colour (102, 102, 102)


@dataclass
class TriMesh:
    """what the reference's consumers read from a trimesh.Trimesh: vertices [V,3] fp32, faces [F,3] int64 (local ids),
    vertex_colors [V,3] fp32 in [0, 1] (or None)."""
    vertices: Tensor
    faces: Tensor
    vertex_colors: Optional[Tensor] = None

    def export(self, path) -> None:
        _write_obj(path, self.vertices, self.faces, self.vertex_colors)


@dataclass
class SceneMesh:
    """One scene: verts [V,3] fp32, faces [F,3] int64 (scene-global ids), vert_rgb [V,3] fp32, face_object [F] int32 (the
    object's index in the input order; the floor, if any, is index N = len(boxes)), box_points [N,8,3] fp32 (every node's
    box corners) and kept (input indices of the objects in the buffers, in order)."""
    verts: Tensor
    faces: Tensor
    vert_rgb: Tensor
    face_object: Tensor
    box_points: Tensor
    kept: List[int]
    vert_counts: List[int] = field(default_factory=list)
    face_counts: List[int] = field(default_factory=list)
    sources: List[str] = field(default_factory=list)       # assemble_scene_from_library: model id / file per kept object

    def per_object(self) -> List[TriMesh]:
        out, v0, f0 = [], 0, 0
        for nv, nf in zip(self.vert_counts, self.face_counts):
            out.append(TriMesh(self.verts[v0:v0 + nv], self.faces[f0:f0 + nf] - v0, self.vert_rgb[v0:v0 + nv]))
            v0, f0 = v0 + nv, f0 + nf
        return out

    def export_obj(self, path) -> None:
        _write_obj(path, self.verts, self.faces, self.vert_rgb)


def _write_obj(path, verts: Tensor, faces: Tensor, rgb: Optional[Tensor]) -> None:
    v = verts.detach().cpu().numpy().astype(np.float64)
    f = faces.detach().cpu().numpy().astype(np.int64) + 1
    with open(path, "w") as fh:
        if rgb is not None:
            np.savetxt(fh, np.concatenate([v, rgb.detach().cpu().numpy().astype(np.float64)], axis=1),
                       fmt="v %.8g %.8g %.8g %.4f %.4f %.4f")
        else:
            np.savetxt(fh, v, fmt="v %.8g %.8g %.8g")
        np.savetxt(fh, f, fmt="f %d %d %d")


def _device() -> torch.device:
    if not torch.cuda.is_available():
        raise L.CsError("scene_mesh: needs the HIP device (the HIP path has no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _label(classes, cat) -> str:
    return classes[int(cat)].strip("\n")


def _skipped(label: str) -> bool:
    return label == "_scene_" or label == "floor"          # helpers/util.py:307-311


def hls_palette(n: int) -> np.ndarray:
    """seaborn's color_palette('hls', n) (visualize_scene.py:390), restated: n hues from 0.01, lightness .6, saturation .65"""
    hues = (np.linspace(0, 1, n + 1)[:-1] + 0.01) % 1.0
    return np.asarray([colorsys.hls_to_rgb(float(h), 0.6, 0.65) for h in hues], dtype=np.float64)


def _check_inputs(n_boxes: int, box_shape, cat_ids, classes) -> List[int]:
    if len(box_shape) != 2 or box_shape[1] != 7:
        raise L.CsError(f"scene_mesh: boxes must be [N, 7] (l, h, w, px, py, pz, angle), got {tuple(box_shape)}")
    cats = [int(c) for c in (cat_ids.tolist() if hasattr(cat_ids, "tolist") else cat_ids)]
    if len(cats) != n_boxes:
        raise L.CsError(f"scene_mesh: {n_boxes} boxes but {len(cats)} category ids")
    for c in cats:
        if c < 0 or c >= len(classes):
            raise L.CsError(f"scene_mesh: category id {c} outside the {len(classes)} classes")
    return cats


def _as_meshes(shapes) -> Meshes:
    """the SDF batch (B,1,n,n,n) -> Meshes (sdf_to_mesh, render_all as helpers/util.py:300), or a Meshes as is"""
    if isinstance(shapes, Meshes):
        return shapes
    if not isinstance(shapes, torch.Tensor) or shapes.dim() != 5 or shapes.shape[1] != 1 or \
            shapes.shape[2] != shapes.shape[3] or shapes.shape[3] != shapes.shape[4]:
        got = tuple(shapes.shape) if isinstance(shapes, torch.Tensor) else type(shapes).__name__
        raise L.CsError(f"scene_mesh: shapes must be a Meshes or a cubic SDF batch (B, 1, n, n, n), got {got}")
    return sdf_to_mesh(shapes, render_all=True)


def _ragged(tensors: Sequence[Tensor], dtype, dev):
    """[k_i, 3] tensors -> (pointer, rows, bases, counts, owner) of one [rows, 3] device buffer.  The views
    `marching_cubes` hands out (torch.split of one buffer) are used in place; anything else is uploaded / concatenated."""
    for t in tensors:
        if t.dim() != 2 or t.shape[1] != 3:
            raise L.CsError(f"scene_mesh: expected [k, 3] vertex / face arrays, got {tuple(t.shape)}")
    counts = [int(t.shape[0]) for t in tensors]
    live = [t for t in tensors if t.shape[0] > 0]
    if live and all(t.is_cuda and t.device == dev and t.dtype == dtype and t.is_contiguous() and
                    t.untyped_storage().data_ptr() == live[0].untyped_storage().data_ptr() and t.storage_offset() % 3 == 0
                    for t in live):
        st = live[0].untyped_storage()
        rows = st.nbytes() // (3 * live[0].element_size())
        return st.data_ptr(), rows, [t.storage_offset() // 3 if t.shape[0] else 0 for t in tensors], counts, live
    if live:
        buf = torch.cat([t.to(device=dev, dtype=dtype) for t in live]).contiguous()
    else:
        buf = torch.zeros((1, 3), dtype=dtype, device=dev)
    bases, b = [], 0
    for c in counts:
        bases.append(b)
        b += c
    return buf.data_ptr(), buf.shape[0], bases, counts, buf


def _i64(vals, dev) -> Tensor:
    return torch.tensor([int(v) for v in vals], dtype=torch.int64).to(dev)


def _fit(vptr: int, vrows: int, vbase: Tensor, vcount: Tensor, box7: Tensor, degrees: bool) -> Tuple[Tensor, Tensor]:
    n = box7.shape[0]
    xform = torch.empty((n, 12), dtype=torch.float32, device=box7.device)
    pts = torch.empty((n, 8, 3), dtype=torch.float32, device=box7.device)
    L.check(L.load().cs_scene_fit_boxes(vptr, vrows, vbase.data_ptr(), vcount.data_ptr(), box7.data_ptr(),
                                        n, int(bool(degrees)), xform.data_ptr(), pts.data_ptr(), _stream()),
            "cs_scene_fit_boxes")
    return xform, pts


def _assemble(verts_list, faces_list, node_of_mesh: List[int], box7: Tensor, keep_nodes: List[bool], colors: np.ndarray,
              degrees: bool, flip: bool, extra_verts: int = 0, extra_faces: int = 0, placed: bool = False,
              mark_nodes: Optional[List[bool]] = None, sections: int = 4, radius: float = 0.006):
    """fit + apply over N nodes; mesh k belongs to node node_of_mesh[k]; the other nodes own no vertices.
    -> (out_verts, out_rgb, out_faces, face_object, box_points, xform, kept nodes, vert counts, face counts); the outputs have
    `extra_*` spare rows at the end (the floor).  placed: retrieval's placement (cs_scene_place_boxes) instead of the fit.
    mark_nodes: the nodes whose box gets tube markers, written after all objects, in input order (cs_scene_box_markers);
    they are appended to kept / counts."""
    dev = box7.device
    n = box7.shape[0]
    vptr, vrows, vb, vc, vown = _ragged(verts_list, torch.float32, dev)
    fptr, frows, fb, fc, fown = _ragged(faces_list, torch.int64, dev)
    nvb, nvc, nfb, nfc = [0] * n, [0] * n, [0] * n, [0] * n
    for k, j in enumerate(node_of_mesh):
        nvb[j], nvc[j], nfb[j], nfc[j] = vb[k], vc[k], fb[k], fc[k]
    ovb, ofb, kept, v0, f0 = [0] * n, [0] * n, [], 0, 0
    for j in range(n):
        ovb[j], ofb[j] = v0, f0
        if keep_nodes[j]:
            kept.append(j)
            v0, f0 = v0 + nvc[j], f0 + nfc[j]
    meta = _i64(nvb + nvc + nfb + nfc + ovb + ofb, dev).view(6, n)          # one small upload
    keep = torch.tensor(keep_nodes, dtype=torch.bool).to(dev)
    col = torch.from_numpy(np.ascontiguousarray(colors, dtype=np.float32)).to(dev)
    xform, pts = _place(box7, degrees) if placed else _fit(vptr, vrows, meta[0], meta[1], box7, degrees)
    marked = [j for j in range(n) if mark_nodes is not None and mark_nodes[j]]
    mv, mf = 12 * (2 * sections + 2), 48 * sections
    tv, tf = v0 + len(marked) * mv + extra_verts, f0 + len(marked) * mf + extra_faces
    out_v = torch.empty((max(tv, 1), 3), dtype=torch.float32, device=dev)     # (never a NULL pointer for an empty scene)
    out_c = torch.empty((max(tv, 1), 3), dtype=torch.float32, device=dev)
    out_f = torch.empty((max(tf, 1), 3), dtype=torch.int64, device=dev)
    out_o = torch.empty((max(tf, 1),), dtype=torch.int32, device=dev)
    L.check(L.load().cs_scene_apply(vptr, vrows, fptr, frows, meta[0].data_ptr(), meta[1].data_ptr(), meta[2].data_ptr(),
                                    meta[3].data_ptr(), xform.data_ptr(), keep.data_ptr(), meta[4].data_ptr(),
                                    meta[5].data_ptr(), col.data_ptr(), n, int(bool(flip)), out_v.data_ptr(),
                                    out_c.data_ptr(), v0, out_f.data_ptr(), out_o.data_ptr(), f0, _stream()),
            "cs_scene_apply")
    del vown, fown
    nv_kept, nf_kept = [nvc[j] for j in kept], [nfc[j] for j in kept]
    if marked:
        mvb, mfb = [0] * n, [0] * n
        for k, j in enumerate(marked):
            mvb[j], mfb[j] = v0 + k * mv, f0 + k * mf
        mmeta = _i64(mvb + mfb, dev).view(2, n)
        mkeep = torch.tensor([bool(mark_nodes[j]) for j in range(n)], dtype=torch.bool).to(dev)
        L.check(L.load().cs_scene_box_markers(pts.data_ptr(), n, mkeep.data_ptr(), mmeta[0].data_ptr(), mmeta[1].data_ptr(),
                                              col.data_ptr(), sections, float(radius), out_v.data_ptr(), out_c.data_ptr(),
                                              v0 + len(marked) * mv, out_f.data_ptr(), out_o.data_ptr(), f0 + len(marked) * mf,
                                              _stream()), "cs_scene_box_markers")
        kept, nv_kept, nf_kept = kept + marked, nv_kept + [mv] * len(marked), nf_kept + [mf] * len(marked)
    return out_v[:tv], out_c[:tv], out_f[:tf], out_o[:tf], pts, xform, kept, nv_kept, nf_kept


def _place(box7: Tensor, degrees: bool) -> Tuple[Tensor, Tensor]:
    n = box7.shape[0]
    xform = torch.empty((n, 12), dtype=torch.float32, device=box7.device)
    pts = torch.empty((n, 8, 3), dtype=torch.float32, device=box7.device)
    L.check(L.load().cs_scene_place_boxes(box7.data_ptr(), n, int(bool(degrees)), xform.data_ptr(), pts.data_ptr(), _stream()),
            "cs_scene_place_boxes")
    return xform, pts


def _check_marker(sections, radius) -> Tuple[int, float]:
    if isinstance(sections, bool) or not isinstance(sections, (int, np.integer)) or \
            not L.MARKER_MIN_SECTIONS <= int(sections) <= L.MARKER_MAX_SECTIONS:
        raise L.CsError(f"scene_mesh: marker sections must be an integer in {L.MARKER_MIN_SECTIONS}..{L.MARKER_MAX_SECTIONS}, "
                        f"got {sections!r}")
    try:
        r = float(np.float32(radius))                      # the kernel takes the fp32 value
    except (TypeError, ValueError):
        raise L.CsError(f"scene_mesh: marker radius must be a number, got {radius!r}") from None
    if not (r > 0.0) or not np.isfinite(r):
        raise L.CsError(f"scene_mesh: marker radius must be positive and finite, got {radius!r}")
    return int(sections), r


def _box7(box, dev) -> Tensor:
    b = torch.as_tensor(box)
    return b.detach().to(device=dev, dtype=torch.float32).contiguous()


def fit_shapes_to_box_v2(verts: Tensor, faces: Tensor, box, degrees: bool = False) -> Tuple[Tensor, Tensor]:
    """helpers/util.py:158-189 for ONE object: -> (box_points [8,3], verts [V,3] fitted into the box), device tensors.
    box: the 7 parameters l, h, w, px, py, pz, angle.  Faces are not changed by the fit (the reference inverts earlier)."""
    dev = _device()
    b = _box7(box, dev).reshape(1, -1)
    if b.shape[1] != 7:
        raise L.CsError(f"fit_shapes_to_box_v2: box must hold 7 parameters, got {b.shape[1]}")
    verts, faces = torch.as_tensor(verts), torch.as_tensor(faces)
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise L.CsError(f"fit_shapes_to_box_v2: expected verts [V,3] and faces [F,3], got {tuple(verts.shape)}, "
                        f"{tuple(faces.shape)}")
    out = _assemble([verts], [faces], [0], b, [True], np.ones((1, 3)), degrees, flip=False)
    return out[4][0], out[0]


def _plan(boxes, meshes: Meshes, cat_ids, classes, colors, without_lamp: bool):
    """the reference's loop (:307-328) as index lists: which node each mesh belongs to, which nodes are kept, colours"""
    return _plan_nodes(boxes, len(meshes), cat_ids, classes, colors, without_lamp)


def _plan_nodes(boxes, n_meshes: Optional[int], cat_ids, classes, colors, without_lamp: bool):
    """`_plan` without the meshes (n_meshes None: the caller chooses them afterwards, one per shaped node)"""
    shape = tuple(torch.as_tensor(boxes).shape)
    cats = _check_inputs(shape[0] if shape else 0, shape, cat_ids, classes)
    labels = [_label(classes, c) for c in cats]
    shaped = [j for j, lab in enumerate(labels) if not _skipped(lab)]
    if n_meshes is not None and n_meshes != len(shaped):
        raise L.CsError(f"scene_mesh: {len(shaped)} shaped objects (boxes that are neither _scene_ nor floor) but "
                        f"{n_meshes} shapes")
    if colors is None:
        colors = hls_palette(len(classes))[cats]
    colors = np.asarray(colors.detach().cpu() if isinstance(colors, torch.Tensor) else colors, dtype=np.float64)
    if colors.ndim != 2 or colors.shape[1] < 3 or colors.shape[0] < len(shaped):
        raise L.CsError(f"scene_mesh: colors must be [>= {len(shaped)}, 3], got {colors.shape}")
    node_col = np.ones((len(cats), 3))
    for k, j in enumerate(shaped):
        node_col[j] = colors[k, :3]                        # next(colors): consumed by the non-skipped objects only
    lamps = [j for j in shaped if labels[j] == "lamp" and without_lamp]
    box7 = _box7(boxes, _device())                         # arguments are checked before the device is touched
    return box7, cats, labels, shaped, node_col, lamps


def get_generated_models_v2(boxes, shapes, cat_ids, classes, mesh_dir=None, render_boxes: bool = False, colors=None,
                            without_lamp: bool = False):
    """helpers/util.py:298-332 -> (lamp_mesh_list, obj_list, raw_obj_list) of TriMesh: the fitted objects (lamps apart when
    without_lamp) and the raw, inverted, coloured meshes.  `shapes`: the SDF batch of the non-skipped objects in order, or
    a Meshes.  Boxes carry their angle in degrees, as at :320.  Writes <label>_<cat>_<instance>.obj per object into mesh_dir
    when given (:317)."""
    if render_boxes:
        raise NotImplementedError("render_boxes needs trimesh.creation.cylinder tube markers: not built")
    meshes = _as_meshes(shapes)
    box7, cats, labels, shaped, node_col, lamps = _plan(boxes, meshes, cat_ids, classes, colors, without_lamp)
    keep = [j in shaped for j in range(len(cats))]
    v, c, f, _, _, _, kept, nv, nf = _assemble(meshes.verts_list(), meshes.faces_list(), shaped, box7, keep, node_col,
                                               degrees=True, flip=True)
    fitted = SceneMesh(v, f, c, None, None, kept, nv, nf).per_object()
    lamp_list, obj_list, raw_list = [], [], []
    if mesh_dir is not None:
        os.makedirs(mesh_dir, exist_ok=True)
    for k, (j, m) in enumerate(zip(shaped, fitted)):
        raw = TriMesh(meshes.verts_list()[k], torch.flip(meshes.faces_list()[k], dims=[1]), m.vertex_colors)
        raw_list.append(raw)
        if mesh_dir is not None:
            raw.export(os.path.join(mesh_dir, f"{labels[j]}_{cats[j]}_{k + 1}.obj"))
        (lamp_list if j in lamps else obj_list).append(m)
    return lamp_list, obj_list, raw_list


def params_to_8points_3dfront(box, degrees: bool = False) -> np.ndarray:
    """helpers/util.py:379-391 on the host, fp64"""
    l, h, w, px, py, pz, angle = [float(x) for x in box]
    pts = np.asarray([[l / 2 * i, h * j, w / 2 * k] for i in (-1, 1) for j in (0, 1) for k in (-1, 1)])
    y = np.deg2rad(angle) if degrees else angle
    rot = np.array([[np.cos(y), 0, -np.sin(y)], [0, 1, 0], [np.sin(y), 0, np.cos(y)]])
    return pts.dot(rot) + np.array([[px, py, pz]])


def create_floor(box_and_angle, cat_ids, classes) -> TriMesh:
    """visualize_scene.py:57-81: the quad at y = 0 spanning the x / z range of the four bottom corners (rows 0, 1, 4, 5) of
    every box but `_scene_`'s (angles in degrees).  A host restatement on host tensors; `assemble_scene(floor=True)` takes
    the same quad from the device box corners."""
    b = torch.as_tensor(box_and_angle).detach().cpu().double()
    cats = _check_inputs(b.shape[0], b.shape, cat_ids, classes)
    xs, zs = [], []
    for j in range(b.shape[0]):
        if _label(classes, cats[j]) == "_scene_":
            continue
        p = params_to_8points_3dfront(b[j].tolist(), degrees=True)
        xs += [p[0:2, 0], p[4:6, 0]]
        zs += [p[0:2, 2], p[4:6, 2]]
    if not xs:
        raise L.CsError("create_floor: no box besides _scene_")
    xs, zs = np.concatenate(xs), np.concatenate(zs)
    v = np.array([[xs.min(), 0, zs.min()], [xs.min(), 0, zs.max()], [xs.max(), 0, zs.max()], [xs.max(), 0, zs.min()]],
                 dtype=np.float32)
    return TriMesh(torch.from_numpy(v), torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int64))


def _floor_rows(labels: List[str], what: str) -> List[int]:
    rows = [j for j in range(len(labels)) if labels[j] != "_scene_"]
    if not rows:
        raise L.CsError(f"{what}: no box besides _scene_ to span the floor")
    return rows


def _add_floor(v, c, f, o, pts, rows: List[int], n: int):
    """the floor quad into the last 4 vertex / 2 face rows, from the device box corners (create_floor's rows 0, 1, 4, 5)"""
    bottom = pts[torch.tensor(rows, dtype=torch.int64).to(v.device)][:, [0, 1, 4, 5]]
    x0, x1, z0, z1 = bottom[..., 0].min(), bottom[..., 0].max(), bottom[..., 2].min(), bottom[..., 2].max()
    zero = torch.zeros((), dtype=torch.float32, device=v.device)
    nv0, nf0 = v.shape[0] - 4, f.shape[0] - 2
    v[nv0:] = torch.stack([torch.stack([x0, zero, z0]), torch.stack([x0, zero, z1]), torch.stack([x1, zero, z1]),
                           torch.stack([x1, zero, z0])])
    c[nv0:] = torch.tensor(FLOOR_RGB, dtype=torch.float32, device=v.device)
    f[nf0:] = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int64, device=v.device) + nv0
    o[nf0:] = n


def assemble_scene(meshes, box_and_angle, cat_ids, classes, colors=None, without_lamp: bool = False, floor: bool = False,
                   degrees: bool = True, flip: bool = True, render_boxes: bool = False,
                   tube_radius: float = 0.006) -> SceneMesh:
    """What render_v2_full hands to trimesh.Scene (visualize_scene.py:401, 433-436), as ONE mesh on the device: the shaped
    objects (neither `_scene_` nor `floor`; lamps left out when without_lamp) fitted into their boxes, in input order, then
    the floor quad when `floor` (the reference's `demo`).  meshes: a Meshes or the SDF batch of the shaped objects.
    flip reverses the winding like pytorch3d_to_trimesh's invert(); degrees as get_generated_models_v2 (:320).
    render_boxes: the tube markers of util.py:330-331 (radius 0.006, four sections) for EVERY shaped object -- a lamp's marker
    stays in the scene under without_lamp, as there -- after all objects and before the floor."""
    meshes = _as_meshes(meshes)
    sections, radius = _check_marker(4, tube_radius) if render_boxes else (4, 0.006)
    box7, cats, labels, shaped, node_col, lamps = _plan(box_and_angle, meshes, cat_ids, classes, colors, without_lamp)
    n = len(cats)
    keep = [(j in shaped) and (j not in lamps) for j in range(n)]
    rows = _floor_rows(labels, "assemble_scene") if floor else None
    mark = [j in shaped for j in range(n)] if render_boxes else None
    v, c, f, o, pts, _, kept, nv, nf = _assemble(meshes.verts_list(), meshes.faces_list(), shaped, box7, keep, node_col,
                                                 degrees, flip, extra_verts=4 if floor else 0,
                                                 extra_faces=2 if floor else 0, mark_nodes=mark, sections=sections,
                                                 radius=radius)
    if floor:
        _add_floor(v, c, f, o, pts, rows, n)
        kept, nv, nf = kept + [n], nv + [4], nf + [2]
    return SceneMesh(v, f, c, o, pts, kept, nv, nf)


# ---------------------------------------------------------------- scenes from a mesh library (csrc/cs_scene_lib.hip)
RENDER_TYPES = ("retrieval", "library", "onlybox")
# the marker radii of the reference: util.py:135 (retrieval), :374 (get_sdfusion_models: create_bbox_marker's default), :149
MARKER_RADIUS = {"retrieval": 0.006, "library": 0.002, "onlybox": 0.02}


def get_closest_furniture_to_box(box_dict, query_size) -> str:
    """helpers/util.py:71-83 for ONE query through cs_scene_retrieve: box_dict {model id: (l, h, w)} in its own order, query_size
    three numbers (a tensor row, rounded to fp32 like the box tensor it comes from) -> the id of the first closest model"""
    from .scene_library import FurnitureLibrary
    if not hasattr(box_dict, "items") or len(box_dict) == 0:
        raise L.CsError("get_closest_furniture_to_box: box_dict must be a non-empty {id: (l, h, w)}")
    q = torch.as_tensor(query_size).detach().reshape(-1)
    if q.numel() != 3:
        raise L.CsError(f"get_closest_furniture_to_box: query_size must hold (l, h, w), got {q.numel()} numbers")
    lib = FurnitureLibrary({"_": list(box_dict.items())}, what="get_closest_furniture_to_box")
    rows, _, status = lib.retrieve_rows(q.reshape(1, 3), [0])
    lib._raise_refused(rows.cpu().tolist(), status.cpu().tolist(), ["query"], "get_closest_furniture_to_box")
    return lib.ids[int(rows.item())]


def choose_shape_files(labels: Sequence[str], library, no_stool: bool = False, rng=None) -> List[str]:
    """The draws of get_sdfusion_models (util.py:351-358) for the shaped objects `labels`, in its order: a = randint(0, 100);
    seed(a); choice(files of the label); for a chair under no_stool: choice(stool files), then choice of the two.  Draws on
    Python's `random` module, or on the random.Random passed as rng.  Host work only.  `library.category(label)` is the sorted
    file list (the reference's is in glob order)."""
    import random as _random
    r = _random if rng is None else rng
    files = {lab: library.category(lab) for lab in set(labels)}          # a missing folder raises before any draw
    if no_stool and "chair" in files:
        files["stool"] = library.category("stool")
    out = []
    for lab in labels:
        a = r.randint(0, 100)
        r.seed(a)
        path = r.choice(files[lab])
        if no_stool and lab == "chair":
            path2 = r.choice(files["stool"])
            path = r.choice([path, path2])
        out.append(path)
    return out


def _library_plan(render_type: str, boxes, cat_ids, classes, library, sections, radius, no_stool: bool, rng):
    """every argument check of the library scenes, then the host-side choices that need no device (the library type's draws)"""
    from .scene_library import FurnitureLibrary, ShapeLibrary
    if render_type not in RENDER_TYPES:
        raise L.CsError(f"scene_mesh: render_type must be one of {RENDER_TYPES}, got {render_type!r}")
    sections, radius = _check_marker(sections, MARKER_RADIUS[render_type] if radius is None else radius)
    shape = tuple(torch.as_tensor(boxes).shape)
    cats = _check_inputs(shape[0] if shape else 0, shape, cat_ids, classes)
    labels = [_label(classes, c) for c in cats]
    shaped = [j for j, lab in enumerate(labels) if not _skipped(lab)]
    files = None
    if render_type == "retrieval":
        if not isinstance(library, FurnitureLibrary):
            raise L.CsError("scene_mesh: render_type 'retrieval' needs a scene_library.FurnitureLibrary as `library`")
        for j in shaped:
            if labels[j] not in library.label_index:
                raise L.CsError(f"scene_mesh: box {j} ({labels[j]!r}): the library has no such category")
    elif render_type == "library":
        if not isinstance(library, ShapeLibrary):
            raise L.CsError("scene_mesh: render_type 'library' needs a scene_library.ShapeLibrary as `library`")
        files = choose_shape_files([labels[j] for j in shaped], library, no_stool, rng)
    return sections, radius, cats, labels, shaped, files


def _library_scene(render_type: str, boxes, cat_ids, classes, library, colors, without_lamp: bool, render_boxes: bool,
                   radius, sections, floor: bool, no_stool: bool, rng):
    """-> (SceneMesh, plan): the one device path behind the list-returning functions and assemble_scene_from_library"""
    sections, radius, cats, labels, shaped, files = _library_plan(render_type, boxes, cat_ids, classes, library, sections,
                                                                  radius, no_stool, rng)
    rows = _floor_rows(labels, "assemble_scene_from_library") if floor else None
    box7, cats, labels, shaped, node_col, lamps = _plan_nodes(boxes, None, cat_ids, classes, colors, without_lamp)
    n = len(cats)
    verts, faces, sources = [], [], []
    if render_type == "retrieval" and shaped:
        idx = torch.tensor(shaped, dtype=torch.int64).to(box7.device)
        lib_rows, _, status = library.retrieve_rows(box7[idx], [library.label_index[labels[j]] for j in shaped])
        lib_rows, status = lib_rows.cpu().tolist(), status.cpu().tolist()      # the one read-back: which meshes to place
        library._raise_refused(lib_rows, status, [labels[j] for j in shaped], "scene_mesh", numbers=shaped)
        for r in lib_rows:
            v, f = library.mesh(r)
            verts.append(v)
            faces.append(f)
            sources.append(library.ids[r])
    elif render_type == "library":
        for path in files:
            v, f = library.mesh(path)
            verts.append(v)
            faces.append(f)
            sources.append(path)
    marks_on = render_boxes or render_type == "onlybox"
    if render_type == "onlybox":
        keep = [False] * n                                  # get_bbox: a lamp's marker itself leaves the scene (:152-153)
        mark = [(j in shaped) and (j not in lamps) for j in range(n)]
        node_of_mesh = []
    else:
        keep = [(j in shaped) and (j not in lamps) for j in range(n)]
        mark = [j in shaped for j in range(n)] if marks_on else None     # (:131-135, :370-374: a lamp's marker stays)
        node_of_mesh = shaped
    # retrieval places (no scale, no inversion); the library type inverts and fits like the generated shapes (:361, :368)
    v, c, f, o, pts, _, kept, nv, nf = _assemble(verts, faces, node_of_mesh, box7, keep, node_col, degrees=True,
                                                 flip=render_type == "library", extra_verts=4 if floor else 0,
                                                 extra_faces=2 if floor else 0, placed=render_type != "library",
                                                 mark_nodes=mark, sections=sections, radius=radius)
    if floor:
        _add_floor(v, c, f, o, pts, rows, n)
        kept, nv, nf = kept + [n], nv + [4], nf + [2]
    kept_src = [sources[shaped.index(j)] for j in kept[:sum(keep)]] if sources else []
    scene = SceneMesh(v, f, c, o, pts, kept, nv, nf, kept_src)
    return scene, dict(cats=cats, labels=labels, shaped=shaped, lamps=lamps, verts=verts, faces=faces, sources=sources,
                       n_objects=sum(keep), node_col=node_col, keep=keep, mark=mark)


def assemble_scene_from_library(render_type: str, box_and_angle, cat_ids, classes, library=None, colors=None,
                                without_lamp: bool = False, render_boxes: bool = False, tube_radius: Optional[float] = None,
                                sections: int = 4, floor: bool = False, no_stool: bool = False, rng=None) -> SceneMesh:
    """The layout-only scenes of visualize_scene.py:208-461 as ONE mesh on the device.  render_type:
      retrieval  per box the closest model of a FurnitureLibrary, placed (util.py:86-138);
      library    per box a drawn shape of a ShapeLibrary, inverted and fitted (get_sdfusion_models, :335-376);
      onlybox    tube markers only (get_bbox, :140-156; render_boxes is implied).
    Content: the kept objects in input order, then the markers in input order, then the floor when asked.  tube_radius
    defaults to the reference's per type (0.006 / 0.002 / 0.02).  `scene.sources` names the model / file of each kept object.
    without_lamp: a lamp's mesh leaves the scene; its marker stays for retrieval / library and leaves for onlybox."""
    return _library_scene(render_type, box_and_angle, cat_ids, classes, library, colors, without_lamp, render_boxes,
                          tube_radius, sections, floor, no_stool, rng)[0]


def _lists_from_scene(scene: SceneMesh, plan: dict):
    """the reference's return lists from one assembled scene: objects and markers interleaved per box, lamps apart"""
    parts = scene.per_object()
    nobj = plan["n_objects"]
    obj_of = {j: parts[k] for k, j in enumerate(scene.kept[:nobj])}
    mark_of = {j: parts[nobj + k] for k, j in enumerate(scene.kept[nobj:])}
    lamp_list, out = [], []
    for j in plan["shaped"]:
        if j in obj_of:
            (lamp_list if j in plan["lamps"] else out).append(obj_of[j])
        if j in mark_of:
            out.append(mark_of[j])
    return lamp_list, out


def _raw_meshes(plan: dict, flip: bool, mesh_dir) -> List[TriMesh]:
    raw = []
    if mesh_dir is not None:
        os.makedirs(mesh_dir, exist_ok=True)
    for k, j in enumerate(plan["shaped"]):
        v, f = plan["verts"][k], plan["faces"][k]
        col = torch.from_numpy(plan["node_col"][j].astype(np.float32)).to(v.device).expand(v.shape[0], 3)
        raw.append(TriMesh(v, torch.flip(f, dims=[1]) if flip else f, col))
        if mesh_dir is not None:
            raw[-1].export(os.path.join(mesh_dir, f"{plan['labels'][j]}_{plan['cats'][j]}_{k + 1}.obj"))
    return raw


def get_textured_objects_v2(boxes, library, cat_ids, classes, mesh_dir=None, render_boxes: bool = False, colors=None,
                            without_lamp: bool = False):
    """helpers/util.py:86-138 -> (lamp_mesh_list, trimesh_meshes, raw_meshes) of TriMesh.  `library` (a FurnitureLibrary)
    replaces the reference's `datasize`, which selects two hard-coded paths.  The placed models in input order, each followed
    by its marker (radius 0.006) when render_boxes; a lamp's model goes to the lamp list under without_lamp, its marker stays."""
    scene, plan = _library_scene("retrieval", boxes, cat_ids, classes, library, colors, False, render_boxes, None, 4,
                                 False, False, None)
    plan["lamps"] = [j for j in plan["shaped"] if plan["labels"][j] == "lamp" and without_lamp]
    lamp_list, out = _lists_from_scene(scene, plan)
    return lamp_list, out, _raw_meshes(plan, False, mesh_dir)


def get_bbox(boxes, cat_ids, classes, colors=None, without_lamp: bool = False):
    """helpers/util.py:140-156 -> (lamp_mesh_list, trimesh_meshes): one marker (radius 0.02) per shaped box; under without_lamp a
    lamp's marker goes to the lamp list"""
    scene, plan = _library_scene("onlybox", boxes, cat_ids, classes, None, colors, False, True, None, 4, False, False, None)
    lamp_list, out = [], []
    for j, m in zip(scene.kept, scene.per_object()):
        (lamp_list if (plan["labels"][j] == "lamp" and without_lamp) else out).append(m)
    return lamp_list, out


def get_sdfusion_models(boxes, library, cat_ids, classes, mesh_dir=None, render_boxes: bool = False, colors=None,
                        no_stool: bool = False, without_lamp: bool = False, rng=None):
    """helpers/util.py:335-376 -> (lamp_mesh_list, obj_list, raw_obj_list).  `library` (a ShapeLibrary) replaces the hard-coded
    folder.  Per shaped object the reference's own draws in its order (`choose_shape_files`), then invert and fit: the
    cs_scene_fit_boxes / cs_scene_apply path with flip, as for generated shapes.  Markers have radius 0.002 (:374)."""
    scene, plan = _library_scene("library", boxes, cat_ids, classes, library, colors, False, render_boxes, None, 4, False,
                                 no_stool, rng)
    plan["lamps"] = [j for j in plan["shaped"] if plan["labels"][j] == "lamp" and without_lamp]
    lamp_list, out = _lists_from_scene(scene, plan)
    return lamp_list, out, _raw_meshes(plan, True, mesh_dir)


def create_bbox_marker(corner_points, color=(0, 0, 255), tube_radius: float = 0.002, sections: int = 4) -> TriMesh:
    """helpers/util.py:393-421: twelve tubes along the edges of the box with corners corner_points [8,3] (in
    params_to_8points_3dfront's order) -> TriMesh of 12 (2 sections + 2) vertices and 48 sections faces, closed and wound
    outward per tube (the layout is documented in include/commonscenes_hip.h).  color: 0..255 integers or 0..1 floats."""
    sections, radius = _check_marker(sections, tube_radius)
    pts = torch.as_tensor(corner_points)
    if tuple(pts.shape) != (8, 3):
        raise L.CsError(f"create_bbox_marker: corner_points must be [8, 3], got {tuple(pts.shape)}")
    col = np.asarray(color)
    if col.size < 3:
        raise L.CsError(f"create_bbox_marker: color must hold r, g, b, got {color!r}")
    col = (col.astype(np.float64) / 255.0 if np.issubdtype(col.dtype, np.integer) else col.astype(np.float64)).reshape(-1)[:3]
    dev = _device()
    pts = pts.detach().to(device=dev, dtype=torch.float32).contiguous().view(1, 8, 3)
    nv, nf = 12 * (2 * sections + 2), 48 * sections
    out_v = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    out_c = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    out_f = torch.empty((nf, 3), dtype=torch.int64, device=dev)
    out_o = torch.empty((nf,), dtype=torch.int32, device=dev)
    zero = torch.zeros((1,), dtype=torch.int64, device=dev)
    keep = torch.ones((1,), dtype=torch.bool, device=dev)
    c = torch.from_numpy(col.astype(np.float32)).to(dev).view(1, 3)
    L.check(L.load().cs_scene_box_markers(pts.data_ptr(), 1, keep.data_ptr(), zero.data_ptr(), zero.data_ptr(), c.data_ptr(),
                                          sections, radius, out_v.data_ptr(), out_c.data_ptr(), nv, out_f.data_ptr(),
                                          out_o.data_ptr(), nf, _stream()), "cs_scene_box_markers")
    return TriMesh(out_v, out_f, out_c)


def render_topdown(scene: SceneMesh, size: int = 256) -> dict:
    """render_img's camera (visualize_scene.py:85-108) -> dict(depth [size,size] fp32 (+inf where empty), object_id int32
    (-1 where empty), rgb [size,size,3] uint8, dropped: triangles left out whole for a vertex nearer than znear)."""
    size = int(size)
    if size <= 0 or size > 8192:
        raise L.CsError(f"render_topdown: size {size} outside 1..8192")
    dev = _device()
    verts = torch.as_tensor(scene.verts).to(device=dev, dtype=torch.float32).contiguous()
    faces = torch.as_tensor(scene.faces).to(device=dev, dtype=torch.int64).contiguous()
    rgb_in = torch.as_tensor(scene.vert_rgb).to(device=dev, dtype=torch.float32).contiguous()
    fobj = torch.as_tensor(scene.face_object).to(device=dev, dtype=torch.int32).contiguous()
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3 or \
            rgb_in.shape != verts.shape or fobj.shape != (faces.shape[0],):
        raise L.CsError(f"render_topdown: malformed scene: verts {tuple(verts.shape)}, faces {tuple(faces.shape)}, "
                        f"vert_rgb {tuple(rgb_in.shape)}, face_object {tuple(fobj.shape)}")
    depth = torch.full((size, size), float("inf"), dtype=torch.float32, device=dev)
    oid = torch.full((size, size), -1, dtype=torch.int32, device=dev)
    rgb = torch.full((size, size, 3), 255, dtype=torch.uint8, device=dev)
    if verts.shape[0] == 0 or faces.shape[0] == 0:
        return dict(depth=depth, object_id=oid, rgb=rgb, dropped=0)
    keys = torch.empty((size, size), dtype=torch.int64, device=dev)
    dropped = torch.empty((1,), dtype=torch.int32, device=dev)
    lib = L.load()
    L.check(lib.cs_scene_raster_topdown(verts.data_ptr(), verts.shape[0], faces.data_ptr(), faces.shape[0], size, ZNEAR,
                                        keys.data_ptr(), dropped.data_ptr(), _stream()), "cs_scene_raster_topdown")
    L.check(lib.cs_scene_resolve(keys.data_ptr(), verts.data_ptr(), verts.shape[0], faces.data_ptr(), faces.shape[0],
                                 rgb_in.data_ptr(), fobj.data_ptr(), size, depth.data_ptr(), oid.data_ptr(), rgb.data_ptr(),
                                 _stream()), "cs_scene_resolve")
    return dict(depth=depth, object_id=oid, rgb=rgb, dropped=int(dropped.item()))
