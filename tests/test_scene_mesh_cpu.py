"""CPU suite of the scene assembly / top-down view (commonscenes_amd/scene_mesh.py, csrc/cs_scene.hip): the C ABI is declared,
exported and described; arguments are validated before the device is touched; create_floor equals the fp64 numpy restatement
of helpers/visualize_scene.py:57-81."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ("cs_scene_fit_boxes", "cs_scene_apply", "cs_scene_raster_topdown", "cs_scene_resolve")
CLASSES = ["_scene_\n", "floor\n", "chair\n", "lamp\n", "table\n"]


def test_scene_entries_are_declared_exported_and_described():
    from commonscenes_amd import build, lib
    txt = (ROOT / "include" / "commonscenes_hip.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    dll = lib.load()
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), f"{name} not declared (with a status) in the header"
        assert hasattr(dll, name), f"{name} not exported"
        assert name in lib.SIGNATURES and lib.SIGNATURES[name][0] is lib._i
    assert "cs_scene.hip" in build.SOURCES
    assert dll.cs_abi_version() == 18


def _meshes(counts):
    from commonscenes_amd.mesh import Meshes
    return Meshes([torch.zeros(c, 3) for c in counts], [torch.zeros(1, 3, dtype=torch.int64) for _ in counts])


def test_argument_validation_raises_before_any_device_work():
    from commonscenes_amd import lib, scene_mesh as S
    cats = [2, 0, 4]
    with pytest.raises(lib.CsError, match=r"\[N, 7\]"):          # a wrong box width
        S.assemble_scene(_meshes([3, 3]), torch.zeros(3, 6), cats, CLASSES)
    with pytest.raises(lib.CsError, match="category ids"):       # boxes / category ids mismatch
        S.assemble_scene(_meshes([3, 3]), torch.zeros(4, 7), cats, CLASSES)
    with pytest.raises(lib.CsError, match="2 shaped objects"):   # shapes / shaped objects mismatch
        S.assemble_scene(_meshes([3, 3, 3]), torch.zeros(3, 7), cats, CLASSES)
    with pytest.raises(lib.CsError, match="cubic SDF"):          # non-cubic SDFs
        S.assemble_scene(torch.zeros(2, 1, 8, 8, 4), torch.zeros(3, 7), cats, CLASSES)
    with pytest.raises(lib.CsError, match="cubic SDF"):
        S.get_generated_models_v2(torch.zeros(3, 7), torch.zeros(2, 8, 8, 8), cats, CLASSES)
    with pytest.raises(lib.CsError, match="outside the 5 classes"):
        S.assemble_scene(_meshes([3, 3]), torch.zeros(3, 7), [2, 0, 9], CLASSES)
    with pytest.raises(lib.CsError, match=r"\[N, 7\]"):
        S.create_floor(torch.zeros(3, 8), cats, CLASSES)
    with pytest.raises(NotImplementedError):
        S.get_generated_models_v2(torch.zeros(3, 7), _meshes([3, 3]), cats, CLASSES, render_boxes=True)


def _ref_rotation_3dfront(y, degree=True):                       # helpers/util.py:510-516
    if degree:
        y = np.deg2rad(y)
    return np.array([[np.cos(y), 0, -np.sin(y)], [0, 1, 0], [np.sin(y), 0, np.cos(y)]])


def _ref_8points(box, degrees):                                  # helpers/util.py:379-391
    l, h, w, px, py, pz, angle = [float(v) for v in box]
    pts = []
    for i in [-1, 1]:
        for j in [0, 1]:
            for k in [-1, 1]:
                pts.append([l / 2 * i, h * j, w / 2 * k])
    pts = np.asarray(pts).dot(_ref_rotation_3dfront(angle, degree=degrees))
    return pts + np.expand_dims(np.array([px, py, pz]), 0)


def _ref_floor(boxes, cats, classes):                            # helpers/visualize_scene.py:57-81
    xs, zs = [], []
    for j in range(boxes.shape[0]):
        if classes[cats[j]].strip("\n") == "_scene_":
            continue
        p = _ref_8points(boxes[j], True)
        xs += [p[0:2, 0], p[4:6, 0]]
        zs += [p[0:2, 2], p[4:6, 2]]
    px = np.array(xs).reshape(-1, 1)
    pz = np.array(zs).reshape(-1, 1)
    pts = np.concatenate((px, np.zeros(px.shape), pz), axis=1)
    (x0, _, z0), (x1, _, z1) = np.min(pts, axis=0), np.max(pts, axis=0)
    return np.array([[x0, 0, z0], [x0, 0, z1], [x1, 0, z1], [x1, 0, z0]], dtype=np.float32)


def test_create_floor_equals_the_numpy_restatement():
    from commonscenes_amd import scene_mesh as S
    rng = np.random.default_rng(5)
    boxes = np.concatenate([rng.uniform(0.3, 2.0, (5, 3)), rng.uniform(-4, 4, (5, 3)),
                            np.array([[0.0], [90.0], [33.3], [-270.0], [15.0]])], axis=1).astype(np.float32)
    boxes[2, 3:6] = [100.0, 0.0, -100.0]                         # the _scene_ node: far away, must not widen the floor
    cats = [2, 4, 0, 1, 3]                                       # chair, table, _scene_, floor, lamp
    m = S.create_floor(torch.from_numpy(boxes), cats, CLASSES)
    want = _ref_floor(boxes, cats, CLASSES)
    assert m.vertices.dtype == torch.float32 and m.faces.tolist() == [[0, 1, 2], [0, 2, 3]]
    assert np.array_equal(m.vertices.numpy(), want)
    assert abs(want).max() < 10                                  # (the _scene_ box was left out)
    assert np.array_equal(S.params_to_8points_3dfront(boxes[3], degrees=True), _ref_8points(boxes[3], True))


def test_default_palette_and_obj_export(tmp_path):
    from commonscenes_amd import scene_mesh as S
    pal = S.hls_palette(5)
    assert pal.shape == (5, 3) and pal.min() >= 0 and pal.max() <= 1 and len({tuple(p) for p in pal}) == 5
    m = S.TriMesh(torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0.5]]), torch.tensor([[0, 1, 2]]),
                  torch.tensor([[1.0, 0, 0]] * 3))
    m.export(tmp_path / "t.obj")
    lines = (tmp_path / "t.obj").read_text().split("\n")
    assert lines[0] == "v 0 0 0 1.0000 0.0000 0.0000" and lines[2] == "v 0 1 0.5 1.0000 0.0000 0.0000"
    assert lines[3] == "f 1 2 3"
