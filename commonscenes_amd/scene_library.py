"""Mesh libraries for the layout-only scenes: the 3D-FUTURE retrieval library and the folder of pre-generated shapes.

The reference turns a sampled layout into a scene without generating shapes in two ways (helpers/visualize_scene.py:208-461):
`retrieval` takes, per box, the 3D-FUTURE model of the box's category whose (l, h, w) is closest to the box's
(`get_closest_furniture_to_box`, helpers/util.py:71-83, called from `get_textured_objects_v2`, :86-138, which reopens
`cat_jid_trainval*.json` and loads `<model root>/<jid>/raw_model.obj` per box); `txt2shape` takes a random pre-generated
`*.ply` of the category (`get_sdfusion_models`, :335-376).  Both need trimesh, which is not in this image.

`FurnitureLibrary` holds the JSON's sizes on the device as fp64 in the file's insertion order -- the order np.argmin's "first
minimum" refers to -- and answers all boxes of all scenes in one launch (csrc/cs_scene_lib.hip: cs_scene_retrieve); meshes are
read on first use and cached on the device.  `ShapeLibrary` lists `root/<label>/*.ply|*.obj` SORTED: the reference takes
`glob` order, which depends on the file system, so its draws cannot be pinned across machines; ours can.
`read_ply` is the companion of `mesh_sdf.read_obj`.
"""
from __future__ import annotations

import json
import math
import os
import struct
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import lib as L
from .mesh_sdf import read_obj
from .ops import _stream

Tensor = torch.Tensor

_PLY_TYPES = {"char": "b", "int8": "b", "uchar": "B", "uint8": "B", "short": "h", "int16": "h", "ushort": "H", "uint16": "H",
              "int": "i", "int32": "i", "uint": "I", "uint32": "I", "float": "f", "float32": "f", "double": "d",
              "float64": "d"}


def read_ply(path) -> Tuple[Tensor, Tensor]:
    """Stanford .ply -> (verts [V,3] fp32, faces [F,3] int64): `ascii` and `binary_little_endian`, vertex x / y / z as float
    or double (other vertex properties are skipped), faces as a `vertex_indices` / `vertex_index` list.  Triangles only: a
    quad is refused by name (the pre-generated shapes are marching-cubes output), as is a file cut short."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise L.CsError(f"read_ply: {path}: not a ply file (no `ply` ... `end_header`)")
    nl = data.find(b"\n", end)
    if nl < 0:
        raise L.CsError(f"read_ply: {path}: truncated after the header")
    fmt, elements = None, []                                  # elements: [name, count, [(prop name, type | (cnt, item))]]
    for line in data[:end].decode("ascii", errors="replace").splitlines()[1:]:
        tok = line.split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append([tok[1], int(tok[2]), []])
        elif tok[0] == "property":
            if not elements:
                raise L.CsError(f"read_ply: {path}: property before any element")
            if tok[1] == "list":
                elements[-1][2].append((tok[4], (tok[2], tok[3])))
            else:
                elements[-1][2].append((tok[2], tok[1]))
    if fmt not in ("ascii", "binary_little_endian"):
        raise L.CsError(f"read_ply: {path}: format {fmt!r} is not read (ascii and binary_little_endian are)")
    for _, _, props in elements:
        for pname, ptype in props:
            for t in (ptype if isinstance(ptype, tuple) else (ptype,)):
                if t not in _PLY_TYPES:
                    raise L.CsError(f"read_ply: {path}: unknown property type {t!r} of {pname!r}")
    body = data[nl + 1:]
    verts: Optional[np.ndarray] = None
    faces: Optional[np.ndarray] = None
    if fmt == "ascii":
        lines = body.decode("ascii", errors="replace").split("\n")
        lines = [ln for ln in lines if ln.strip()]
        at = 0
    else:
        at = 0
    for name, count, props in elements:
        names = [p[0] for p in props]
        if name == "vertex":
            if not all(a in names for a in "xyz") or any(isinstance(p[1], tuple) for p in props):
                raise L.CsError(f"read_ply: {path}: vertex needs scalar x, y, z properties, has {names}")
            for a in "xyz":
                if _PLY_TYPES[props[names.index(a)][1]] not in "fd":
                    raise L.CsError(f"read_ply: {path}: vertex {a} must be float or double")
            cols = [names.index(a) for a in "xyz"]
            if fmt == "ascii":
                if at + count > len(lines):
                    raise L.CsError(f"read_ply: {path}: truncated: {count} vertices declared, {len(lines) - at} lines left")
                try:
                    rows = [[float(t) for t in lines[at + i].split()] for i in range(count)]
                except ValueError as e:
                    raise L.CsError(f"read_ply: {path}: malformed vertex line: {e}") from None
                if any(len(r) < len(names) for r in rows):
                    raise L.CsError(f"read_ply: {path}: truncated vertex line")
                verts = np.asarray([[r[c] for c in cols] for r in rows], dtype=np.float64).reshape(-1, 3)
                at += count
            else:
                dt = np.dtype([(f"p{i}", "<" + _PLY_TYPES[p[1]]) for i, p in enumerate(props)])
                need = dt.itemsize * count
                if at + need > len(body):
                    raise L.CsError(f"read_ply: {path}: truncated: {count} vertices declared, "
                                    f"{(len(body) - at) // max(dt.itemsize, 1)} present")
                rec = np.frombuffer(body, dtype=dt, count=count, offset=at)
                verts = np.stack([rec[f"p{c}"].astype(np.float64) for c in cols], axis=1).reshape(-1, 3)
                at += need
        elif name == "face":
            lists = [i for i, p in enumerate(props) if isinstance(p[1], tuple)]
            if len(lists) != 1 or props[lists[0]][0] not in ("vertex_indices", "vertex_index"):
                raise L.CsError(f"read_ply: {path}: face needs one vertex_indices list, has {names}")
            li = lists[0]
            out = np.empty((count, 3), dtype=np.int64)
            if fmt == "ascii":
                if li != 0:
                    raise L.CsError(f"read_ply: {path}: ascii faces must start with the vertex_indices list")
                if at + count > len(lines):
                    raise L.CsError(f"read_ply: {path}: truncated: {count} faces declared, {len(lines) - at} lines left")
                for i in range(count):
                    tok = lines[at + i].split()
                    try:
                        k = int(tok[0])
                        ids = [int(t) for t in tok[1:1 + k]]
                    except (ValueError, IndexError) as e:
                        raise L.CsError(f"read_ply: {path}: malformed face line {i}: {e}") from None
                    if k != 3:
                        raise L.CsError(f"read_ply: {path}: face {i} has {k} corners" + (" (a quad)" if k == 4 else "") +
                                        ": triangles only")
                    if len(ids) != 3:
                        raise L.CsError(f"read_ply: {path}: truncated face line {i}")
                    out[i] = ids
                at += count
            else:
                ctype, itype = props[li][1]
                csz, isz = struct.calcsize(_PLY_TYPES[ctype]), struct.calcsize(_PLY_TYPES[itype])
                pre = sum(struct.calcsize(_PLY_TYPES[p[1]]) for p in props[:li])
                post = sum(struct.calcsize(_PLY_TYPES[p[1]]) for p in props[li + 1:])
                # all-triangle files have a fixed record: check the counts in one pass, fall back to naming the culprit
                rec = pre + csz + 3 * isz + post
                if at + rec * count <= len(body):
                    fields = [("k", "<" + _PLY_TYPES[ctype]), ("ids", "<" + _PLY_TYPES[itype], (3,))]
                    if pre:
                        fields.insert(0, ("pre", "V%d" % pre))
                    if post:
                        fields.append(("post", "V%d" % post))
                    arr = np.frombuffer(body, dtype=np.dtype(fields), count=count, offset=at)
                    if count == 0 or (arr["k"] == 3).all():
                        out[:] = arr["ids"]
                        at += rec * count
                        faces = out
                        continue
                for i in range(count):                       # a record that is not a triangle, or a short file
                    if at + pre + csz > len(body):
                        raise L.CsError(f"read_ply: {path}: truncated: {count} faces declared, {i} present")
                    k = struct.unpack_from("<" + _PLY_TYPES[ctype], body, at + pre)[0]
                    if k != 3:
                        raise L.CsError(f"read_ply: {path}: face {i} has {k} corners" + (" (a quad)" if k == 4 else "") +
                                        ": triangles only")
                    if at + rec > len(body):
                        raise L.CsError(f"read_ply: {path}: truncated: {count} faces declared, {i} present")
                    out[i] = struct.unpack_from("<3" + _PLY_TYPES[itype], body, at + pre + csz)
                    at += rec
            faces = out
        else:                                                 # another element: skipped where its size is known
            if fmt == "ascii":
                at += count
            else:
                if any(isinstance(p[1], tuple) for p in props):
                    raise L.CsError(f"read_ply: {path}: element {name!r} with a list property cannot be skipped")
                at += count * sum(struct.calcsize(_PLY_TYPES[p[1]]) for p in props)
    if verts is None or faces is None:
        raise L.CsError(f"read_ply: {path}: needs a vertex and a face element")
    if faces.size and (faces.min() < 0 or faces.max() >= verts.shape[0]):
        raise L.CsError(f"read_ply: {path}: face index outside the {verts.shape[0]} vertices")
    return torch.from_numpy(verts.astype(np.float32)), torch.from_numpy(faces)


def write_ply(path, verts, faces, binary: bool = True) -> None:
    """(verts [V,3], faces [F,3]) -> a triangle .ply (float x y z; uchar-counted int lists), what `read_ply` reads back"""
    v = np.ascontiguousarray(torch.as_tensor(verts).detach().cpu().numpy(), dtype="<f4").reshape(-1, 3)
    f = np.ascontiguousarray(torch.as_tensor(faces).detach().cpu().numpy(), dtype="<i4").reshape(-1, 3)
    head = ("ply\nformat %s 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
            "element face %d\nproperty list uchar int vertex_indices\nend_header\n") % (
        "binary_little_endian" if binary else "ascii", v.shape[0], f.shape[0])
    with open(path, "wb") as fh:
        fh.write(head.encode("ascii"))
        if binary:
            fh.write(v.tobytes())
            rec = np.empty(f.shape[0], dtype=[("k", "u1"), ("ids", "<i4", (3,))])
            rec["k"], rec["ids"] = 3, f
            fh.write(rec.tobytes())
        else:
            for r in v:
                fh.write(("%.9g %.9g %.9g\n" % tuple(float(x) for x in r)).encode("ascii"))
            for r in f:
                fh.write(("3 %d %d %d\n" % tuple(int(x) for x in r)).encode("ascii"))


def read_mesh(path) -> Tuple[Tensor, Tensor]:
    return read_ply(path) if str(path).lower().endswith(".ply") else read_obj(path)


def _device() -> torch.device:
    if not torch.cuda.is_available():
        raise L.CsError("scene_library: needs the HIP device (the HIP path has no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _check_mesh(what: str, v: Tensor, f: Tensor) -> Tuple[Tensor, Tensor]:
    v, f = torch.as_tensor(v), torch.as_tensor(f)
    if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3:
        raise L.CsError(f"{what}: expected verts [V,3] and faces [F,3], got {tuple(v.shape)}, {tuple(f.shape)}")
    return v, f


class FurnitureLibrary:
    """The retrieval library: per category label an ordered list of (model id, (l, h, w)), with the models' meshes.

    rows are numbered over all categories in insertion order; `cat_base` is the CSR of the categories over the rows;
    `labels[c]` names category c.  Sizes stay Python floats (fp64) as json.load delivers them."""

    def __init__(self, table: "Dict[str, Sequence[Tuple[str, Sequence[float]]]]", loader=None, what: str = "FurnitureLibrary"):
        self.labels: List[str] = []
        self.ids: List[str] = []
        self.cat_base: List[int] = [0]
        sizes: List[List[float]] = []
        for label, entries in table.items():
            self.labels.append(str(label))
            for mid, size in entries:
                try:
                    s = [float(x) for x in size]
                except (TypeError, ValueError):
                    raise L.CsError(f"{what}: {label}/{mid}: size {size!r} is not three numbers") from None
                if len(s) != 3:
                    raise L.CsError(f"{what}: {label}/{mid}: size must be (l, h, w), got {len(s)} numbers")
                if not all(math.isfinite(x) for x in s):
                    raise L.CsError(f"{what}: {label}/{mid}: size {s} is not finite")
                self.ids.append(str(mid))
                sizes.append(s)
            self.cat_base.append(len(self.ids))
        if not self.labels:
            raise L.CsError(f"{what}: no category")
        self.label_index = {lab: c for c, lab in enumerate(self.labels)}
        self.sizes = np.asarray(sizes, dtype=np.float64).reshape(-1, 3)
        self._loader = loader
        self._meshes: Dict[int, Tuple[Tensor, Tensor]] = {}
        self._dev = None                                     # (sizes fp64 [M,3], cat_base int64 [C+1]) on the device

    @classmethod
    def from_json(cls, bbox_file, model_root=None) -> "FurnitureLibrary":
        """`cat_jid_trainval*.json`: {label: {jid: [l, h, w]}} (util.py:88-91); meshes from model_root/<jid>/raw_model.obj"""
        with open(bbox_file, "r") as fh:
            data = json.load(fh)
        if not isinstance(data, dict) or not all(isinstance(v, dict) for v in data.values()):
            raise L.CsError(f"FurnitureLibrary.from_json: {bbox_file}: expected {{label: {{jid: [l, h, w]}}}}")
        root = None if model_root is None else Path(model_root)

        def load(mid: str):
            if root is None:
                raise L.CsError(f"FurnitureLibrary: model {mid}: the library was opened without a model root")
            p = root / mid / "raw_model.obj"
            if not p.exists():
                raise L.CsError(f"FurnitureLibrary: {p} not found")
            return read_obj(p)
        return cls({lab: list(models.items()) for lab, models in data.items()}, loader=load,
                   what=f"FurnitureLibrary.from_json({os.fspath(bbox_file)})")

    @classmethod
    def from_meshes(cls, table: "Dict[str, Sequence[Tuple[str, Sequence[float], Tensor, Tensor]]]") -> "FurnitureLibrary":
        """{label: [(id, (l, h, w), verts [V,3], faces [F,3]), ...]}: a library held in memory (tests, synthetic runs)"""
        meshes, plain = {}, {}
        for label, entries in table.items():
            plain[label] = []
            for mid, size, v, f in entries:
                meshes[(str(label), str(mid))] = _check_mesh(f"FurnitureLibrary.from_meshes: {label}/{mid}", v, f)
                plain[label].append((mid, size))
        out = cls(plain, what="FurnitureLibrary.from_meshes")
        for c, label in enumerate(out.labels):
            for r in range(out.cat_base[c], out.cat_base[c + 1]):
                out._meshes[r] = meshes[(label, out.ids[r])]
        return out

    def __len__(self) -> int:
        return len(self.ids)

    def category(self, label: str) -> "Dict[str, List[float]]":
        """the reference's `box_data[label]`: {model id: [l, h, w]} in insertion order"""
        c = self.label_index[label]
        return {self.ids[r]: self.sizes[r].tolist() for r in range(self.cat_base[c], self.cat_base[c + 1])}

    def mesh(self, row: int) -> Tuple[Tensor, Tensor]:
        """the model of library row `row` as device tensors (verts fp32, faces int64), read on first use"""
        row = int(row)
        if row < 0 or row >= len(self.ids):
            raise L.CsError(f"FurnitureLibrary: row {row} outside the {len(self.ids)} models")
        dev = _device()
        got = self._meshes.get(row)
        if got is None:
            if self._loader is None:
                raise L.CsError(f"FurnitureLibrary: model {self.ids[row]} has no mesh")
            got = _check_mesh(f"FurnitureLibrary: model {self.ids[row]}", *self._loader(self.ids[row]))
        if got[0].device != dev or got[0].dtype != torch.float32 or got[1].dtype != torch.int64:
            got = (got[0].to(device=dev, dtype=torch.float32).contiguous(), got[1].to(device=dev, dtype=torch.int64).contiguous())
        self._meshes[row] = got
        return got

    def _device_tables(self, dev):
        if self._dev is None or self._dev[0].device != dev:
            self._dev = (torch.from_numpy(self.sizes).to(dev), torch.tensor(self.cat_base, dtype=torch.int64).to(dev))
        return self._dev

    def query_categories(self, cat_ids, classes) -> Tuple[List[str], List[int]]:
        """per box its label and the library's category index (-1: the library has no such label)"""
        cats = [int(c) for c in (cat_ids.tolist() if hasattr(cat_ids, "tolist") else cat_ids)]
        for c in cats:
            if c < 0 or c >= len(classes):
                raise L.CsError(f"scene_library: category id {c} outside the {len(classes)} classes")
        labels = [classes[c].strip("\n") for c in cats]
        return labels, [self.label_index.get(lab, -1) for lab in labels]

    def retrieve_rows(self, boxes: Tensor, lib_cats: Sequence[int]) -> Tuple[Tensor, Tensor, Tensor]:
        """cs_scene_retrieve over the rows of `boxes` ([Q, >= 3], size = columns 0..2) with the LIBRARY's category index per
        row -> (row int64 [Q], d2 fp64 [Q], status int32 [Q]) on the device.  Nothing is raised for a refused query."""
        boxes = torch.as_tensor(boxes)
        if boxes.dim() != 2 or boxes.shape[1] < 3:
            raise L.CsError(f"scene_library: boxes must be [Q, >= 3] (l, h, w first), got {tuple(boxes.shape)}")
        if len(lib_cats) != boxes.shape[0]:
            raise L.CsError(f"scene_library: {boxes.shape[0]} boxes but {len(lib_cats)} category ids")
        if boxes.shape[0] == 0:
            raise L.CsError("scene_library: no box to retrieve for")
        dev = _device()
        b = boxes.detach().to(device=dev, dtype=torch.float32)
        if b.stride(1) != 1 or b.stride(0) < b.shape[1]:
            b = b.contiguous()
        sizes, base = self._device_tables(dev)
        qc = torch.tensor([int(c) for c in lib_cats], dtype=torch.int32).to(dev)
        q = b.shape[0]
        index = torch.empty((q,), dtype=torch.int64, device=dev)
        d2 = torch.empty((q,), dtype=torch.float64, device=dev)
        status = torch.empty((q,), dtype=torch.int32, device=dev)
        L.check(L.load().cs_scene_retrieve(sizes.data_ptr(), sizes.shape[0], base.data_ptr(), len(self.labels), b.data_ptr(),
                                           max(b.stride(0), 3), qc.data_ptr(), q,
                                           index.data_ptr(), d2.data_ptr(), status.data_ptr(), _stream()),
                "cs_scene_retrieve")
        return index, d2, status

    def _raise_refused(self, rows, status, labels, where: str, numbers=None):
        for j, (r, st) in enumerate(zip(rows, status)):
            if st:
                why = [w for bit, w in ((L.RETRIEVE_STATUS_NONFINITE, "its size is not finite"),
                                        (L.RETRIEVE_STATUS_CATEGORY, "the library has no such category"),
                                        (L.RETRIEVE_STATUS_EMPTY, "the library's category is empty"),
                                        (L.RETRIEVE_STATUS_NODISTANCE, "no distance to the category is finite")) if st & bit]
                raise L.CsError(f"{where}: box {j if numbers is None else numbers[j]} ({labels[j]!r}): " + ", ".join(why))

    def retrieve(self, boxes, cat_ids, classes) -> Tuple[List[str], Tensor]:
        """every row of `boxes` ([Q, >= 3]) against its category `classes[cat_ids[j]]` -> (model ids, d2 fp64 [Q] on the
        device).  Raises CsError naming the box and label for a non-finite size, a label the library lacks or an empty
        category (the reference raises KeyError / ValueError there)."""
        ids, d2, _ = self.retrieve_many([(boxes, cat_ids)], classes)[0]
        return ids, d2

    def retrieve_many(self, scenes: "Sequence[Tuple[Tensor, Sequence[int]]]", classes) -> "List[Tuple[List[str], Tensor, List[int]]]":
        """[(boxes, cat_ids), ...] -> per scene (model ids, d2, library rows): all scenes' boxes in ONE launch"""
        labels, lib_cats, parts = [], [], []
        for boxes, cat_ids in scenes:
            boxes = torch.as_tensor(boxes)
            if boxes.dim() != 2 or boxes.shape[1] < 3:
                raise L.CsError(f"scene_library: boxes must be [Q, >= 3] (l, h, w first), got {tuple(boxes.shape)}")
            lab, lc = self.query_categories(cat_ids, classes)
            if len(lab) != boxes.shape[0]:
                raise L.CsError(f"scene_library: {boxes.shape[0]} boxes but {len(lab)} category ids")
            labels += lab
            lib_cats += lc
            parts.append(boxes[:, :3])
        if not parts:
            return []
        dev = _device()
        allb = torch.cat([p.detach().to(device=dev, dtype=torch.float32) for p in parts])
        rows, d2, status = self.retrieve_rows(allb, lib_cats)
        rows_h, st_h = rows.cpu().tolist(), status.cpu().tolist()
        self._raise_refused(rows_h, st_h, labels, "FurnitureLibrary.retrieve")
        out, at = [], 0
        for p in parts:
            n = p.shape[0]
            out.append(([self.ids[r] for r in rows_h[at:at + n]], d2[at:at + n], rows_h[at:at + n]))
            at += n
        return out


class ShapeLibrary:
    """The folder of pre-generated shapes of get_sdfusion_models (util.py:337, :349-354): label -> the SORTED list of
    `root/<label>/*.ply` and `*.obj`.  (The reference takes glob order, which the file system decides.)"""

    def __init__(self, root):
        self.root = Path(root)
        if not self.root.is_dir():
            raise L.CsError(f"ShapeLibrary: {self.root} is not a directory")
        self.files: Dict[str, List[str]] = {}
        for d in sorted(p for p in self.root.iterdir() if p.is_dir()):
            got = sorted(str(p) for p in d.iterdir() if p.suffix.lower() in (".ply", ".obj"))
            if got:
                self.files[d.name] = got
        self._meshes: Dict[str, Tuple[Tensor, Tensor]] = {}

    def category(self, label: str) -> List[str]:
        if label not in self.files:
            raise L.CsError(f"ShapeLibrary: {self.root} has no shapes for {label!r}")
        return self.files[label]

    def mesh(self, path: str) -> Tuple[Tensor, Tensor]:
        dev = _device()
        got = self._meshes.get(path)
        if got is None:
            v, f = read_mesh(path)
            got = (v.to(dev), f.to(dev))
            self._meshes[path] = got
        return got
