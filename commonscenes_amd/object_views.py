"""Per-object views on the MI355X: the reference's object renderer behind its own names.

  look_at_view_transform / init_mesh_renderer / render_sdf / render_meshes   model/diff_utils/util_3d.py:135-189, 350-393
  trimeshes_to_meshes / normalize_meshes                                     helpers/util.py:222-258
  tensor2im                                                                  model/diff_utils/util.py:21-41
  get_current_visuals_v2 / store_current_imgs                                helpers/visualize_scene.py:29-55

The reference renders with pytorch3d (FoVPerspectiveCameras, MeshRasterizer, HardPhongShader with the default lights) and
tiles images with torchvision; neither is in this image.  csrc/cs_view.hip does the work on the device: normalise, project,
vertex normals in 64-bit fixed point, the exact-coverage rasteriser of the top-down view with one key image per mesh, and
per-pixel Phong shading.  pytorch3d's conventions are restated from its documented behaviour, so parity with it is NOT
pinned (like marching cubes and the top-down shading); the tests check known answers and an fp64 restatement.

Stated differences: coverage follows the top-left rule on the 1/256-pixel grid (pytorch3d lets both triangles own a shared
edge), and a triangle with a vertex nearer than znear / 2 = 0.5 is dropped whole where pytorch3d clips it (counted in
`Fragments.dropped`; it cannot happen for normalised meshes or render_sdf's, which stay within distance 1 of the origin).
The orthographic camera (`camera != '0'`) is not built.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from collections import OrderedDict
from dataclasses import dataclass
from typing import Callable, List, Optional

import numpy as np
import torch

from . import lib as L
from .mesh import Meshes, Textures, sdf_to_mesh

Tensor = torch.Tensor
FOCAL = 1.0 / math.tan(math.radians(30.0))        # FoVPerspectiveCameras' default fov = 60 degrees
ZMIN = 0.5                                        # znear / 2 of the default znear = 1
LIGHT = (0.0, 1.0, 0.0)                           # PointLights' default location
MAX_SIZE = 8192


def look_at_view_transform(dist=1.0, elev=0.0, azim=0.0):
    """pytorch3d's look_at_view_transform (degrees, at = origin, up = +y) -> (R [3,3], T [3]) numpy fp64 with
    X_view = X_world @ R + T.  Raises ValueError where up x z degenerates (elev = +-90)."""
    e, a = math.radians(float(elev)), math.radians(float(azim))
    c = float(dist) * np.array([math.cos(e) * math.sin(a), math.sin(e), math.cos(e) * math.cos(a)], dtype=np.float64)
    n = np.linalg.norm(c)
    if not n > 0:
        raise ValueError("look_at_view_transform: the camera sits on the point it looks at")
    z = -c / n
    x = np.cross(np.array([0.0, 1.0, 0.0]), z)
    if np.linalg.norm(x) < 1e-6:
        raise ValueError(f"look_at_view_transform: up x view direction degenerates at elev = {elev}")
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    y /= np.linalg.norm(y)
    R = np.stack([x, y, z], axis=1)
    return R, -c @ R


def camera_position(R: np.ndarray, T: np.ndarray) -> np.ndarray:
    return -R @ T


@dataclass
class Fragments:
    """pix_to_face [B,S,S] int64 (face id in the packed batch, -1 empty), zbuf [B,S,S] fp32 (view depth, -1 empty),
    bary_coords [B,S,S,3] fp32 (perspective-correct), dropped [B] int32 (triangles left out whole at the near plane)."""
    pix_to_face: Tensor
    zbuf: Tensor
    bary_coords: Tensor
    dropped: Tensor


def _device(device=None) -> torch.device:
    if not torch.cuda.is_available():
        raise L.CsError("object_views: needs the HIP device (the HIP path has no CPU fallback)")
    d = torch.device(device) if device is not None else torch.device("cuda")
    if d.type != "cuda":
        raise L.CsError("object_views: renders on the HIP device only")
    return torch.device("cuda", d.index if d.index is not None else torch.cuda.current_device())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class _Packed:
    """a Meshes as one packed batch on the device: verts [V,3], faces [F,3] with packed ids, rgb [V,3], meta [4,B] int64"""

    def __init__(self, meshes: Meshes, dev: torch.device):
        vl, fl = list(meshes.verts_list()), list(meshes.faces_list())
        tx = meshes.textures.verts_features_list() if meshes.textures is not None else None
        self.n = len(vl)
        self.nv = [int(v.shape[0]) for v in vl]
        self.nf = [int(f.shape[0]) for f in fl]
        for v, f in zip(vl, fl):
            if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3:
                raise L.CsError(f"object_views: expected verts [V,3] and faces [F,3], got {tuple(v.shape)}, {tuple(f.shape)}")
        if tx is not None:
            for v, t in zip(vl, tx):
                if tuple(t.shape) != tuple(v.shape):
                    raise L.CsError(f"object_views: vertex colours {tuple(t.shape)} for vertices {tuple(v.shape)}")
        vb = np.concatenate([[0], np.cumsum(self.nv)]).astype(np.int64)
        fb = np.concatenate([[0], np.cumsum(self.nf)]).astype(np.int64)
        self.V, self.F = int(vb[-1]), int(fb[-1])
        f32 = lambda ts: torch.cat([t.to(device=dev, dtype=torch.float32) for t in ts]).contiguous()
        self.verts = f32(vl) if self.V else torch.zeros((0, 3), dtype=torch.float32, device=dev)
        self.rgb = f32(tx) if (tx is not None and self.V) else torch.ones_like(self.verts)
        self.meta = torch.from_numpy(np.stack([vb[:-1], np.asarray(self.nv, dtype=np.int64), fb[:-1],
                                               np.asarray(self.nf, dtype=np.int64)]).reshape(4, -1)).to(dev)
        if self.F:
            off = torch.repeat_interleave(self.meta[0], self.meta[3])
            self.faces = (torch.cat([f.to(device=dev, dtype=torch.int64) for f in fl]) + off[:, None]).contiguous()
        else:
            self.faces = torch.zeros((0, 3), dtype=torch.int64, device=dev)

    def ranges(self):
        return tuple(self.meta[k].data_ptr() for k in range(4))


def _empty(shape, dtype, dev) -> Tensor:
    return torch.empty(shape, dtype=dtype, device=dev)


class MeshRenderer:
    """What the reference's `MeshRenderer(MeshRasterizer(FoVPerspectiveCameras(R, T), image_size), HardPhongShader)` does:
    `renderer(meshes)` -> [B,S,S,4] fp32 RGBA on a white background (alpha 0 / 1); `renderer.rasterize(meshes)` ->
    Fragments.  `normalize=True` runs normalize_meshes' stage inside the same pass."""

    def __init__(self, image_size: int, R: np.ndarray, T: np.ndarray, device=None):
        image_size = int(image_size)
        if image_size < 1 or image_size > MAX_SIZE:
            raise ValueError(f"image_size {image_size} outside 1..{MAX_SIZE}")
        self.image_size, self.R, self.T, self.device = image_size, np.asarray(R, np.float64), np.asarray(T, np.float64), device
        self.cam12 = (C.c_float * 12)(*np.concatenate([self.R.T, self.T[:, None]], axis=1).reshape(-1).tolist())
        self.eye = camera_position(self.R, self.T)
        self.eye3 = (C.c_float * 3)(*self.eye.tolist())

    # the stages, one entry each; `alloc(shape, dtype, device)` lets a test put guard bands around every output
    def project(self, pk: _Packed, normalize: bool = False, alloc: Callable = _empty):
        dev = pk.verts.device
        centre = alloc((3,), torch.float32, dev)
        world = alloc((pk.V, 3), torch.float32, dev)
        screen = alloc((pk.V, 2), torch.int32, dev)
        zview = alloc((pk.V,), torch.float32, dev)
        vb, vc, _, _ = pk.ranges()
        L.check(L.load().cs_view_project(pk.verts.data_ptr(), pk.V, vb, vc, pk.n, int(bool(normalize)), self.cam12, FOCAL,
                                         self.image_size, centre.data_ptr(), world.data_ptr(), screen.data_ptr(),
                                         zview.data_ptr(), _stream()), "cs_view_project")
        return dict(centre=centre, world=world, screen=screen, zview=zview)

    def raster(self, pk: _Packed, screen: Tensor, zview: Tensor, alloc: Callable = _empty):
        dev, s = pk.verts.device, self.image_size
        keys = alloc((pk.n, s, s), torch.int64, dev)
        dropped = alloc((pk.n,), torch.int32, dev)
        L.check(L.load().cs_view_raster(screen.data_ptr(), zview.data_ptr(), pk.V, pk.faces.data_ptr(), pk.F, *pk.ranges(),
                                        pk.n, s, ZMIN, keys.data_ptr(), dropped.data_ptr(), _stream()), "cs_view_raster")
        return keys, dropped

    def shade(self, pk: _Packed, keys: Tensor, world: Tensor, normals: Tensor, screen: Tensor, zview: Tensor,
              alloc: Callable = _empty):
        dev, s = pk.verts.device, self.image_size
        image = alloc((pk.n, s, s, 4), torch.float32, dev)
        p2f = alloc((pk.n, s, s), torch.int64, dev)
        zbuf = alloc((pk.n, s, s), torch.float32, dev)
        bary = alloc((pk.n, s, s, 3), torch.float32, dev)
        L.check(L.load().cs_view_shade(keys.data_ptr(), world.data_ptr(), normals.data_ptr(), pk.rgb.data_ptr(),
                                       screen.data_ptr(), zview.data_ptr(), pk.V, pk.faces.data_ptr(), pk.F, *pk.ranges(), pk.n,
                                       s, self.eye3, image.data_ptr(), p2f.data_ptr(), zbuf.data_ptr(), bary.data_ptr(),
                                       _stream()), "cs_view_shade")
        return image, p2f, zbuf, bary

    def render_all(self, meshes: Meshes, normalize: bool = False, alloc: Callable = _empty) -> dict:
        """every stage's outputs: image, pix_to_face, zbuf, bary, dropped, and (when the batch has faces) world, normals,
        screen, zview, keys and the packed batch `pk`"""
        dev = _device(self.device)
        pk = meshes if isinstance(meshes, _Packed) else _Packed(meshes, dev)
        s = self.image_size
        if pk.n == 0 or pk.F == 0 or pk.V == 0:                 # nothing to draw: background
            image = torch.ones((pk.n, s, s, 4), dtype=torch.float32, device=dev)
            image[..., 3] = 0
            return dict(image=image, pix_to_face=torch.full((pk.n, s, s), -1, dtype=torch.int64, device=dev),
                        zbuf=torch.full((pk.n, s, s), -1.0, dtype=torch.float32, device=dev),
                        bary=torch.zeros((pk.n, s, s, 3), dtype=torch.float32, device=dev),
                        dropped=torch.zeros((pk.n,), dtype=torch.int32, device=dev), pk=pk)
        pr = self.project(pk, normalize, alloc)
        normals = vertex_normals(pk, pr["world"], alloc)
        keys, dropped = self.raster(pk, pr["screen"], pr["zview"], alloc)
        image, p2f, zbuf, bary = self.shade(pk, keys, pr["world"], normals, pr["screen"], pr["zview"], alloc)
        return dict(image=image, pix_to_face=p2f, zbuf=zbuf, bary=bary, dropped=dropped, normals=normals, keys=keys, pk=pk,
                    **pr)

    def rasterize(self, meshes: Meshes, normalize: bool = False) -> Fragments:
        o = self.render_all(meshes, normalize)
        return Fragments(o["pix_to_face"], o["zbuf"], o["bary"], o["dropped"])

    def __call__(self, meshes: Meshes, normalize: bool = False) -> Tensor:
        return self.render_all(meshes, normalize)["image"]


def vertex_normals(pk: _Packed, world: Optional[Tensor] = None, alloc: Callable = _empty) -> Tensor:
    """pytorch3d's verts_normals_packed of the packed batch -> [V,3] fp32, bit-reproducible"""
    dev = pk.verts.device
    world = pk.verts if world is None else world
    accum = alloc((pk.V, 3), torch.int64, dev)
    scale = alloc((pk.n,), torch.float32, dev)
    normals = alloc((pk.V, 3), torch.float32, dev)
    L.check(L.load().cs_view_vertex_normals(world.data_ptr(), pk.V, pk.faces.data_ptr(), pk.F, *pk.ranges(), pk.n,
                                            accum.data_ptr(), scale.data_ptr(), normals.data_ptr(), _stream()),
            "cs_view_vertex_normals")
    return normals


def init_mesh_renderer(image_size=512, dist=3.5, elev=90, azim=90, camera="0", device="cuda:0") -> MeshRenderer:
    """util_3d.py:135-189.  Only the perspective camera ('0') is built.  The reference's default elev = 90 looks straight
    down, where the look-at basis degenerates: every caller of the reference passes its own angles (1.7, 20, 20)."""
    if camera != "0":
        raise NotImplementedError("the orthographic camera (camera != '0') is not built")
    R, T = look_at_view_transform(dist, elev, azim)
    return MeshRenderer(image_size, R, T, device)


def trimeshes_to_meshes(meshes) -> Meshes:
    """helpers/util.py:222-240 for this package's TriMesh records (vertex_colors already in [0, 1]; none = white)"""
    vl = [torch.as_tensor(m.vertices, dtype=torch.float32) for m in meshes]
    fl = [torch.as_tensor(m.faces, dtype=torch.int64) for m in meshes]
    tx = [torch.as_tensor(m.vertex_colors, dtype=torch.float32)[:, :3] if m.vertex_colors is not None else torch.ones_like(v)
          for m, v in zip(meshes, vl)]
    return Meshes(vl, fl, Textures(tx))


def normalize_meshes(meshes: Meshes) -> Meshes:
    """helpers/util.py:242-258: ONE centre, the mean over all packed vertices of the batch, and one scale per mesh,
    1 / (its largest distance from that centre).  A mesh of extent 0 (or with a non-finite vertex) collapses to the origin."""
    dev = _device()
    pk = _Packed(meshes, dev)
    if pk.n == 0 or pk.V == 0:
        return meshes
    centre = torch.empty((3,), dtype=torch.float32, device=dev)
    out = torch.empty_like(pk.verts)
    vb, vc, _, _ = pk.ranges()
    L.check(L.load().cs_view_normalize(pk.verts.data_ptr(), pk.V, vb, vc, pk.n, centre.data_ptr(), out.data_ptr(),
                                       _stream()), "cs_view_normalize")
    return Meshes(list(torch.split(out, pk.nv)), list(meshes.faces_list()), meshes.textures)


def _chw(images: Tensor) -> Tensor:
    return images.permute(0, 3, 1, 2).contiguous()


def render_sdf(mesh_renderer: MeshRenderer, sdf: Tensor, level=0.02, color=None, render_imsize=256, render_all=False):
    """util_3d.py:350-375: (B,1,n,n,n) SDF -> [B',4,S,S] (B' = min(B, 16) unless render_all); zeros
    [B',4,render_imsize,render_imsize] when marching cubes finds no surface at all."""
    mesh = sdf_to_mesh(sdf, level=level, color=color, render_all=render_all)
    if len(mesh) == 0 or all(int(v.shape[0]) == 0 for v in mesh.verts_list()):
        nimg = sdf.shape[0] if render_all else min(sdf.shape[0], 16)
        return torch.zeros((nimg, 4, render_imsize, render_imsize), dtype=torch.float32, device=_device())
    return _chw(mesh_renderer(mesh))


def render_meshes(mesh_renderer: MeshRenderer, meshes: Optional[Meshes], level=0.02, color=None, render_imsize=256,
                  render_all=False):
    """util_3d.py:378-393 -> [B,4,S,S]"""
    if meshes is None:
        return torch.zeros((0, 4, render_imsize, render_imsize), dtype=torch.float32, device=_device())
    return _chw(mesh_renderer(meshes))


def make_grid(t: Tensor, nrow: int = 4, padding: int = 2, pad_value: float = 0.0) -> Tensor:
    """torchvision.utils.make_grid(nrow, padding, pad_value) restated (no normalisation)"""
    if t.dim() == 3:
        if t.shape[0] == 1:
            t = torch.cat((t, t, t), 0)
        t = t.unsqueeze(0)
    if t.dim() != 4:
        raise ValueError(f"make_grid: expected [C,H,W] or [N,C,H,W], got {tuple(t.shape)}")
    if t.shape[1] == 1:
        t = torch.cat((t, t, t), 1)
    if t.shape[0] == 1:
        return t.squeeze(0)
    n = t.shape[0]
    xmaps = min(nrow, n)
    ymaps = int(math.ceil(n / xmaps))
    h, w = t.shape[2] + padding, t.shape[3] + padding
    grid = t.new_full((t.shape[1], h * ymaps + padding, w * xmaps + padding), pad_value)
    for k in range(n):
        y, x = divmod(k, xmaps)
        grid[:, y * h + padding:y * h + h, x * w + padding:x * w + w] = t[k]
    return grid


def tensor2im(image_tensor: Tensor, imtype=np.uint8) -> np.ndarray:
    """diff_utils/util.py:21-41: at most 16 images tiled 4 per row, then ((x + 1) / 2 * 255).astype(uint8), which truncates
    and maps white to 255, alpha 1 to 255 and alpha 0 to 127.  A [4,H,W] input is one RGBA image: -> [H,W,4]."""
    image_tensor = image_tensor[:min(image_tensor.shape[0], 16)]
    if image_tensor.dim() == 4 and image_tensor.shape[1] == 1:
        image_tensor = image_tensor.repeat(1, 3, 1, 1)
    grid = make_grid(image_tensor, nrow=4)
    image_numpy = grid.detach().cpu().float().numpy()
    image_numpy = (np.transpose(image_numpy, (1, 2, 0)) + 1) / 2.0 * 255.0
    return image_numpy.astype(imtype)


def get_current_visuals_v2(vocab, renderer: MeshRenderer, meshes, obj_ids) -> "OrderedDict[int, np.ndarray]":
    """visualize_scene.py:42-55: the objects of one scene (TriMesh records, or a Meshes), normalised together, one view each
    -> OrderedDict {1..N: uint8 [S,S,4]}"""
    m = meshes if isinstance(meshes, Meshes) else trimeshes_to_meshes(meshes)
    with torch.no_grad():
        img = _chw(renderer(m, normalize=True)).detach().cpu()
    return OrderedDict((k + 1, tensor2im(img[k])) for k in range(img.shape[0]))


def store_current_imgs(visuals, img_dir, classes, cat_ids) -> List[str]:
    """visualize_scene.py:29-40: <label>_<cat>_<instance>.png per image; a `_scene_` or `floor` category is stepped over
    (once, as in the reference).  Returns the paths written."""
    from PIL import Image
    cat_ids = iter(cat_ids)
    paths = []
    for instance_id, image_numpy in visuals.items():
        cat_id = next(cat_ids)
        query_label = classes[int(cat_id)].strip("\n")
        if query_label == "_scene_" or query_label == "floor":
            cat_id = next(cat_ids)
            query_label = classes[int(cat_id)].strip("\n")
        path = os.path.join(img_dir, f"{query_label}_{int(cat_id)}_{instance_id}.png")
        Image.fromarray(image_numpy).save(path)
        paths.append(path)
    return paths
