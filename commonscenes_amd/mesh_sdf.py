"""Triangle meshes -> 64^3 SDF grids on the MI355X: the input side of every entry that takes a shape.

The reference READS its SDFs from `3D-FUTURE-SDF/.../ori_sample_grid.h5` (dataset/threedfront_dataset.py:383-392,
model/diff_utils/util_3d.py:50-56); the preprocessing binary that wrote those files is not part of it.  Only the mesh
normalisation survives, as `get_normalize_mesh` (util_3d.py:481-512).  `mesh_to_sdf` makes the grids here from what people
have -- 3D-FUTURE `.obj` files, `sdf_to_mesh` output, scene exports -- with csrc/cs_sdf.hip (moments, pack, grid, finish).

Convention (parity with the original `.h5` grids is UNPINNED: their recipe is not in the reference; it is chosen to agree with
what the reference does with the grids):
  * array index [i, j, k] is (x, y, z); the grid spans [-bound, bound]^3 and node i of an axis sits at
    -bound + i * 2 bound / (n - 1) (`get_partial_shape`, demo_util.py:187-201, reads the grid exactly so);
  * normalize=True puts the mesh in the unit sphere: subtract the surface centroid, divide by the largest distance from it.
    The reference estimates both from 16384 area-weighted random surface samples; this module uses their LIMITS -- the exact
    area-weighted centroid of the triangles and the largest vertex distance from it (the maximum over a triangulated surface
    is reached at a vertex) -- so the result is deterministic;
  * distance: exact Euclidean distance to the closest point of any triangle; a zero-area triangle is a segment or a point;
  * sign: generalised winding number w = sum Omega_i / 4 pi (Van Oosterom-Strackee solid angles); a node is inside when
    |w| >= wind_level.  The absolute value is deliberate: `sdf_to_mesh`'s default table orients normals towards decreasing
    value, so the project's own meshes have w = -1 inside, and a globally flipped mesh must still get an inside;
  * value: negative inside; trunc=0.2 clamps to +-0.2 as the dataset loader does (threedfront_dataset.py:391).
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import torch

from . import lib as L
from .mesh import Meshes
from .ops import _stream

Tensor = torch.Tensor


def plan(face_count: int, n: int) -> Tuple[int, int]:
    """cs_mesh_sdf_plan: (slices, workspace bytes) of one mesh -- a function of its own face count and n only.  Host only."""
    s, b = C.c_int32(0), C.c_int64(0)
    rc = L.load().cs_mesh_sdf_plan(int(face_count), int(n), C.byref(s), C.byref(b))
    if rc != L.CS_OK:
        raise ValueError(f"mesh_to_sdf: no plan for face_count={face_count}, res={n}")
    return s.value, b.value


def display_to_grid(verts: Tensor, n: int, bound: float = 1.0) -> Tensor:
    """`sdf_to_mesh`'s display coordinates (v = idx / n - 0.5) -> this module's frame, where node idx sits at
    -bound + idx * 2 bound / (n - 1)."""
    idx = verts * float(n) + 0.5 * float(n)
    return idx * (2.0 * float(bound) / float(n - 1)) - float(bound)


def read_obj(path) -> Tuple[Tensor, Tensor]:
    """Wavefront .obj -> (verts [V,3] fp32, faces [F,3] int64), `v` / `f` lines only.  Polygons are fanned from their first
    corner; `a/b/c` corners keep the vertex id; negative ids count back from the vertices read so far."""
    verts: List[List[float]] = []
    faces: List[List[int]] = []
    with open(path, "r", errors="replace") as fh:
        for line in fh:
            tok = line.split()
            if not tok:
                continue
            if tok[0] == "v" and len(tok) >= 4:
                verts.append([float(tok[1]), float(tok[2]), float(tok[3])])
            elif tok[0] == "f" and len(tok) >= 4:
                ids = []
                for t in tok[1:]:
                    i = int(t.split("/")[0])
                    ids.append(i - 1 if i > 0 else len(verts) + i)
                for k in range(1, len(ids) - 1):
                    faces.append([ids[0], ids[k], ids[k + 1]])
    v = torch.tensor(verts, dtype=torch.float32).reshape(-1, 3)
    f = torch.tensor(faces, dtype=torch.int64).reshape(-1, 3)
    return v, f


def _device() -> torch.device:
    return torch.device("cuda", torch.cuda.current_device())


class _Batch:
    """a ragged batch packed for the C ABI: verts fp32 [sum V, 3], faces int64 [sum F, 3] (mesh-local ids), host counts"""

    def __init__(self, verts_list: Sequence[Tensor], faces_list: Sequence[Tensor]):
        if len(verts_list) == 0 or len(verts_list) != len(faces_list):
            raise ValueError("mesh_to_sdf: need as many face tensors as vertex tensors, and at least one mesh")
        for i, (v, f) in enumerate(zip(verts_list, faces_list)):      # host-side checks first: they need no device
            if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3:
                raise ValueError(f"mesh_to_sdf: mesh {i}: expected verts [V,3] and faces [F,3], got {tuple(v.shape)}, "
                                 f"{tuple(f.shape)}")
            if v.shape[0] == 0 or f.shape[0] == 0:
                raise ValueError(f"mesh_to_sdf: mesh {i} is empty ({v.shape[0]} vertices, {f.shape[0]} faces)")
            if f.dtype not in (torch.int32, torch.int64):
                raise ValueError(f"mesh_to_sdf: mesh {i}: faces must be int32 or int64, got {f.dtype}")
        dev = _device()
        # CPU tensors are uploaded, as sdf_to_mesh does with a host SDF: the work is on the device
        vs = [v.to(device=dev, dtype=torch.float32) for v in verts_list]
        fs = [f.to(device=dev, dtype=torch.int64) for f in faces_list]
        self.nv = [int(v.shape[0]) for v in vs]
        self.nf = [int(f.shape[0]) for f in fs]
        self.verts = torch.cat(vs).contiguous()
        self.faces = torch.cat(fs).contiguous()
        self.nb = len(vs)

    def meta(self, n: int):
        rows, vb, fb, wo, slices = [], 0, 0, 0, []
        for v, f in zip(self.nv, self.nf):
            s, b = plan(f, n)
            rows.append([vb, v, fb, f, s, wo])
            slices.append(s)
            vb, fb, wo = vb + v, fb + f, wo + b
        return torch.tensor(rows, dtype=torch.int64).to(_device()), slices, wo


_STATUS_TEXT = ((L.SDF_STATUS_INDEX, "a face index outside its vertex range"),
                (L.SDF_STATUS_NONFINITE, "a non-finite vertex"),
                (L.SDF_STATUS_RANGE, "a range outside its buffer (internal)"),
                (L.SDF_STATUS_EMPTY, "no surface area to normalise by"))


def _raise_status(status: Tensor, what: str) -> None:
    st = status.cpu().tolist()             # the one read-back of the batch
    bad = [(i, s) for i, s in enumerate(st) if s]
    if bad:
        msg = "; ".join(f"mesh {i}: " + ", ".join(t for b, t in _STATUS_TEXT if s & b) for i, s in bad)
        raise L.CsError(f"{what}: {msg}")


def _moments(b: _Batch, meta: Tensor, status: Tensor) -> Tensor:
    lib = L.load()
    dev = b.verts.device
    partial = torch.empty((b.nb, L.SDF_MOMENT_BLOCKS, 4), dtype=torch.float64, device=dev)
    norm = torch.empty((b.nb, 4), dtype=torch.float64, device=dev)
    L.check(lib.cs_mesh_sdf_moments(b.verts.data_ptr(), b.verts.shape[0], b.faces.data_ptr(), b.faces.shape[0],
                                    meta.data_ptr(), b.nb, partial.data_ptr(), norm.data_ptr(), status.data_ptr(),
                                    _stream()), "cs_mesh_sdf_moments")
    return norm


def get_normalize_mesh(verts: Tensor, faces: Tensor):
    """util_3d.py:481-512 under the reference's name: (verts_normalised, centroid, m) with verts_normalised =
    (verts - centroid) / m inside the unit sphere.  centroid and m are the limits of the reference's 16384-sample estimates
    (module docstring), computed in fp64 on the device; centroid is fp64 [3], m a fp64 scalar tensor."""
    b = _Batch([verts], [faces])
    meta, _, _ = b.meta(2)
    status = torch.zeros((1,), dtype=torch.int32, device=b.verts.device)
    norm = _moments(b, meta, status)
    _raise_status(status, "get_normalize_mesh")
    c, m = norm[0, :3], norm[0, 3]
    out = ((b.verts.double() - c) / m).to(torch.float32)
    return out, c, m


def mesh_to_sdf(meshes_or_verts_list, faces_list=None, res: int = 64, bound: float = 1.0, normalize: bool = True,
                sign: str = "winding", wind_level: float = 0.5, trunc: Optional[float] = None,
                return_winding: bool = False, return_meta: bool = False):
    """A ragged batch of triangle meshes -> [B,1,res,res,res] fp32 SDF grids on the device (convention: module docstring).

    meshes_or_verts_list: a `mesh.Meshes`, or a list of [V,3] tensors with faces_list a list of [F,3] int32 / int64 tensors
    (CPU tensors are uploaded).  normalize=True applies `get_normalize_mesh` (deterministic: exact area-weighted centroid,
    largest vertex distance); normalize=False takes the vertices as given.  sign="unsigned" returns the distance alone.
    Returns sdf, then the winding field [B,1,res,res,res] if return_winding, then a dict if return_meta: `centroid` fp64 [B,3]
    and `scale` fp64 [B] on the device, `faces` and `slices` (lists).  The result is bit-identical from run to run and a
    mesh's grid does not depend on the rest of the batch.  ValueError for empty meshes, res < 2, bound <= 0, a bad `sign`;
    CsError, naming the mesh, for a face index out of range or a non-finite vertex."""
    if isinstance(meshes_or_verts_list, Meshes):
        if faces_list is not None:
            raise ValueError("mesh_to_sdf: faces_list goes with a list of vertex tensors, not with Meshes")
        verts_list, faces_list = meshes_or_verts_list.verts_list(), meshes_or_verts_list.faces_list()
    else:
        verts_list = list(meshes_or_verts_list)
        if faces_list is None:
            raise ValueError("mesh_to_sdf: faces_list is required with a list of vertex tensors")
    n = int(res)
    if n < 2 or n > 1024:
        raise ValueError(f"mesh_to_sdf: res must be in 2..1024, got {res}")
    if not (float(bound) > 0.0) or float(bound) == float("inf"):
        raise ValueError(f"mesh_to_sdf: bound must be positive and finite, got {bound}")
    if sign not in ("winding", "unsigned"):
        raise ValueError(f"mesh_to_sdf: sign must be 'winding' or 'unsigned', got {sign!r}")
    if not (float(wind_level) > 0.0):
        raise ValueError(f"mesh_to_sdf: wind_level must be positive, got {wind_level}")
    if trunc is not None and not (float(trunc) > 0.0):
        raise ValueError(f"mesh_to_sdf: trunc must be positive or None, got {trunc}")
    b = _Batch(verts_list, list(faces_list))
    lib = L.load()
    dev = b.verts.device
    meta, slices, ws_bytes = b.meta(n)
    status = torch.zeros((b.nb,), dtype=torch.int32, device=dev)
    if normalize:
        norm = _moments(b, meta, status)
    else:
        norm = torch.tensor([[0.0, 0.0, 0.0, 1.0]] * b.nb, dtype=torch.float64).to(dev)
    tf = b.faces.shape[0]
    tris = torch.empty((tf, 12), dtype=torch.float32, device=dev)
    L.check(lib.cs_mesh_sdf_pack(b.verts.data_ptr(), b.verts.shape[0], b.faces.data_ptr(), tf, meta.data_ptr(), b.nb,
                                 norm.data_ptr(), tris.data_ptr(), status.data_ptr(), _stream()), "cs_mesh_sdf_pack")
    ws = torch.empty((ws_bytes // 8,), dtype=torch.float64, device=dev)
    L.check(lib.cs_mesh_sdf_grid(tris.data_ptr(), tf, meta.data_ptr(), b.nb, n, float(bound), max(slices), ws.data_ptr(),
                                 ws_bytes, status.data_ptr(), _stream()), "cs_mesh_sdf_grid")
    out = torch.empty((b.nb, 1, n, n, n), dtype=torch.float32, device=dev)
    wout = torch.empty_like(out) if return_winding else None
    L.check(lib.cs_mesh_sdf_finish(ws.data_ptr(), ws_bytes, meta.data_ptr(), b.nb, n, 1 if sign == "winding" else 0,
                                   float(wind_level), float(trunc) if trunc is not None else 0.0, out.data_ptr(),
                                   wout.data_ptr() if wout is not None else None, _stream()), "cs_mesh_sdf_finish")
    _raise_status(status, "mesh_to_sdf")
    ret = [out]
    if return_winding:
        ret.append(wout)
    if return_meta:
        ret.append({"centroid": norm[:, :3], "scale": norm[:, 3], "faces": list(b.nf), "slices": list(slices)})
    return ret[0] if len(ret) == 1 else tuple(ret)
