"""CPU suite of the scene-library feature: the three C entries are declared and exported, the readers and libraries behave,
every argument is checked before the device is touched, and get_sdfusion_models' file choices equal the restated draws."""
import json
import random
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import _scene_library_ref as R

ROOT = Path(__file__).resolve().parent.parent
CLASSES = ["_scene_\n", "floor\n", "chair\n", "lamp\n", "table\n", "stool\n"]
ENTRIES = ("cs_scene_retrieve", "cs_scene_place_boxes", "cs_scene_box_markers")


def test_entries_are_declared_exported_and_abi_is_still_18():
    import ctypes as C
    from commonscenes_amd import build, lib
    assert "cs_scene_lib.hip" in build.SOURCES and (build.CSRC / "cs_scene_lib.hip").exists()
    txt = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "commonscenes_hip.h").read_text(), flags=re.S)
    dll = lib.load()
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), f"{name} is not declared with an int status"
        assert name in lib.SIGNATURES and lib.SIGNATURES[name][0] is C.c_int
        assert hasattr(dll, name)
    assert dll.cs_abi_version() == lib.ABI_VERSION == 18
    # the status bits and the section range of the header are the ones the host uses
    for k, v in (("CS_RETRIEVE_STATUS_NONFINITE", lib.RETRIEVE_STATUS_NONFINITE),
                 ("CS_RETRIEVE_STATUS_CATEGORY", lib.RETRIEVE_STATUS_CATEGORY),
                 ("CS_RETRIEVE_STATUS_EMPTY", lib.RETRIEVE_STATUS_EMPTY),
                 ("CS_RETRIEVE_STATUS_NODISTANCE", lib.RETRIEVE_STATUS_NODISTANCE),
                 ("CS_MARKER_MIN_SECTIONS", lib.MARKER_MIN_SECTIONS), ("CS_MARKER_MAX_SECTIONS", lib.MARKER_MAX_SECTIONS)):
        assert re.search(r"#define\s+%s\s+%d\b" % (k, v), txt), k


def test_entries_refuse_bad_arguments_before_any_launch():
    """beyond the all-zero call of test_abi_cpu: valid pointers with one bad scalar each (host memory: never dereferenced)"""
    import ctypes as C
    from commonscenes_amd import lib
    dll = lib.load()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    ok_r = [p, 5, p, 1, p, 7, p, 1, p, p, p, None]
    for i, bad in ((1, 0), (3, 0), (5, 2), (7, 0), (0, None), (8, None)):
        a = list(ok_r)
        a[i] = bad
        assert dll.cs_scene_retrieve(*a) == lib.CS_EINVAL, (i, bad)
    assert dll.cs_scene_place_boxes(p, 0, 1, p, p, None) == lib.CS_EINVAL
    assert dll.cs_scene_place_boxes(p, 1, 1, None, p, None) == lib.CS_EINVAL
    ok_m = [p, 1, p, p, p, p, 4, 0.02, p, p, 120, p, p, 192, None]
    for i, bad in ((6, 2), (6, 65), (7, 0.0), (7, -1.0), (7, float("inf")), (7, float("nan")), (1, 0), (10, -1), (2, None)):
        a = list(ok_m)
        a[i] = bad
        assert dll.cs_scene_box_markers(*a) == lib.CS_EINVAL, (i, bad)


@pytest.mark.parametrize("binary,double,index_type", [(False, False, "int"), (True, False, "int"), (True, True, "uchar"),
                                                      (False, True, "int")])
def test_read_ply_round_trips(tmp_path, binary, double, index_type):
    from commonscenes_amd.scene_library import read_ply
    v, f = R.box_mesh((1.25, 0.5, 2.0))
    v = v + np.float32(0.1)
    R.write_ply(tmp_path / "a.ply", v, f, binary, double, index_type)
    gv, gf = read_ply(tmp_path / "a.ply")
    assert gv.dtype == torch.float32 and gf.dtype == torch.int64
    assert np.array_equal(gv.numpy(), v) and np.array_equal(gf.numpy(), f)


def test_package_writer_is_read_back(tmp_path):
    from commonscenes_amd.scene_library import read_ply, write_ply
    v, f = R.box_mesh((0.3, 0.7, 1.1))
    for binary in (False, True):
        write_ply(tmp_path / "w.ply", v, f, binary=binary)
        gv, gf = read_ply(tmp_path / "w.ply")
        assert np.array_equal(gv.numpy(), v) and np.array_equal(gf.numpy(), f)


@pytest.mark.parametrize("binary", [False, True])
def test_read_ply_refuses_a_quad_and_a_truncated_file(tmp_path, binary):
    from commonscenes_amd import lib
    from commonscenes_amd.scene_library import read_ply
    v, f = R.box_mesh((1, 1, 1))
    R.write_ply(tmp_path / "q.ply", v, [[0, 1, 3], [0, 1, 3, 2]], binary)
    with pytest.raises(lib.CsError, match="quad"):
        read_ply(tmp_path / "q.ply")
    R.write_ply(tmp_path / "t.ply", v, f, binary)
    data = (tmp_path / "t.ply").read_bytes()
    for cut in (30, len(data) - 1 - (0 if binary else 8), data.index(b"end_header") + 20):
        (tmp_path / "c.ply").write_bytes(data[:cut])
        with pytest.raises(lib.CsError):
            read_ply(tmp_path / "c.ply")
    (tmp_path / "n.ply").write_bytes(b"not a ply\n")
    with pytest.raises(lib.CsError):
        read_ply(tmp_path / "n.ply")


def test_from_json_keeps_insertion_order_and_refuses_non_finite_sizes(tmp_path):
    from commonscenes_amd import lib
    from commonscenes_amd.scene_library import FurnitureLibrary
    data = {"table": {"zz": [1.0, 0.5, 2.0], "aa": [0.1, 0.2, 0.3], "mm": [1.0, 0.5, 2.0]}, "empty": {},
            "chair": {"c9": [0.4, 0.9, 0.4], "c1": [0.45, 1.0, 0.5]}}
    (tmp_path / "lib.json").write_text(json.dumps(data))
    lib_ = FurnitureLibrary.from_json(tmp_path / "lib.json", tmp_path)
    assert lib_.labels == ["table", "empty", "chair"] and lib_.ids == ["zz", "aa", "mm", "c9", "c1"]
    assert lib_.cat_base == [0, 3, 3, 5] and len(lib_) == 5
    assert lib_.sizes.dtype == np.float64 and lib_.sizes.tolist()[1] == [0.1, 0.2, 0.3]       # the Python floats, not fp32
    assert list(lib_.category("chair")) == ["c9", "c1"]
    for bad in ("NaN", "Infinity", "-Infinity"):
        (tmp_path / "bad.json").write_text('{"table": {"a": [1.0, %s, 2.0]}}' % bad)
        with pytest.raises(lib.CsError, match="finite"):
            FurnitureLibrary.from_json(tmp_path / "bad.json", tmp_path)
    (tmp_path / "bad.json").write_text('{"table": {"a": [1.0, 2.0]}}')
    with pytest.raises(lib.CsError):
        FurnitureLibrary.from_json(tmp_path / "bad.json", tmp_path)
    (tmp_path / "bad.json").write_text('{"table": [1.0, 2.0, 3.0]}')
    with pytest.raises(lib.CsError):
        FurnitureLibrary.from_json(tmp_path / "bad.json", tmp_path)


def test_shape_library_lists_sorted_files(tmp_path):
    from commonscenes_amd import lib
    from commonscenes_amd.scene_library import ShapeLibrary
    for lab, names in (("chair", ["b.ply", "a.obj", "c.PLY", "notes.txt"]), ("table", ["t.ply"]), ("void", ["x.txt"])):
        (tmp_path / lab).mkdir()
        for n in names:
            (tmp_path / lab / n).write_text("")
    sl = ShapeLibrary(tmp_path)
    assert [Path(p).name for p in sl.category("chair")] == ["a.obj", "b.ply", "c.PLY"]
    assert set(sl.files) == {"chair", "table"}
    with pytest.raises(lib.CsError, match="void"):
        sl.category("void")
    with pytest.raises(lib.CsError):
        ShapeLibrary(tmp_path / "missing")


def _shape_library(tmp_path, counts):
    from commonscenes_amd.scene_library import ShapeLibrary
    v, f = R.box_mesh((1, 1, 1))
    for lab, n in counts.items():
        (tmp_path / lab).mkdir()
        for k in range(n):
            R.write_ply(tmp_path / lab / f"{lab}{k:02d}.ply", v * np.float32(1 + k), f, True)
    return ShapeLibrary(tmp_path)


@pytest.mark.parametrize("no_stool", [False, True])
def test_file_choices_equal_the_restated_draws(tmp_path, no_stool):
    from commonscenes_amd import scene_mesh as S
    sl = _shape_library(tmp_path, {"chair": 7, "table": 5, "lamp": 3, "stool": 4})
    labels = ["chair", "table", "chair", "lamp", "chair", "table", "chair"]
    for seed in (0, 48, 12345):
        want = R.ref_choices(labels, sl.files, no_stool, seed)
        assert S.choose_shape_files(labels, sl, no_stool, random.Random(seed)) == want
        random.seed(seed)                                   # rng None: Python's module-level generator
        assert S.choose_shape_files(labels, sl, no_stool) == want
    assert len(set(R.ref_choices(labels, sl.files, no_stool, 48))) > 2
    if no_stool:
        assert any("stool" in p for s in range(20) for p in R.ref_choices(labels, sl.files, True, s))


def test_arguments_are_checked_before_the_device(tmp_path, monkeypatch):
    from commonscenes_amd import lib, scene_mesh as S, synth
    touched = []
    monkeypatch.setattr(S, "_device", lambda: touched.append(1) or (_ for _ in ()).throw(AssertionError("device touched")))
    flib = synth.furniture_library(["chair\n", "table\n", "lamp\n"], per_category=3)
    sl = _shape_library(tmp_path, {"chair": 2, "table": 2})
    boxes = torch.ones(3, 7)
    cats = [2, 4, 0]
    call = lambda *a, **k: S.assemble_scene_from_library(*a, **k)
    with pytest.raises(lib.CsError, match="render_type"):
        call("txt2shape", boxes, cats, CLASSES, library=flib)
    with pytest.raises(lib.CsError, match=r"\[N, 7\]"):
        call("retrieval", torch.ones(3, 6), cats, CLASSES, library=flib)
    with pytest.raises(lib.CsError, match="category id"):
        call("retrieval", boxes, [2, 4, 6], CLASSES, library=flib)
    with pytest.raises(lib.CsError, match="category ids"):
        call("onlybox", boxes, [2, 4], CLASSES)
    with pytest.raises(lib.CsError, match="FurnitureLibrary"):
        call("retrieval", boxes, cats, CLASSES)
    with pytest.raises(lib.CsError, match="FurnitureLibrary"):
        call("retrieval", boxes, cats, CLASSES, library=sl)
    with pytest.raises(lib.CsError, match="ShapeLibrary"):
        call("library", boxes, cats, CLASSES, library=flib)
    with pytest.raises(lib.CsError, match="stool"):         # a label without a folder / a library category
        call("retrieval", boxes, [2, 5, 0], CLASSES, library=flib)
    with pytest.raises(lib.CsError, match="lamp"):
        call("library", boxes, [2, 3, 0], CLASSES, library=sl)
    for sections in (2, 65, 4.0, True):
        with pytest.raises(lib.CsError, match="sections"):
            call("onlybox", boxes, cats, CLASSES, sections=sections)
        with pytest.raises(lib.CsError, match="sections"):
            S.create_bbox_marker(np.zeros((8, 3)), sections=sections)
    for radius in (0.0, -0.01, float("inf"), float("nan"), 1e-60):
        with pytest.raises(lib.CsError, match="radius"):
            call("onlybox", boxes, cats, CLASSES, tube_radius=radius)
        with pytest.raises(lib.CsError, match="radius"):
            S.create_bbox_marker(np.zeros((8, 3)), tube_radius=radius)
    with pytest.raises(lib.CsError, match="radius"):
        S.assemble_scene(_empty_meshes(), torch.ones(1, 7), [0], CLASSES, render_boxes=True, tube_radius=0.0)
    with pytest.raises(lib.CsError, match=r"\[8, 3\]"):
        S.create_bbox_marker(np.zeros((7, 3)))
    with pytest.raises(lib.CsError):
        S.get_textured_objects_v2(torch.ones(3, 6), flib, cats, CLASSES)
    with pytest.raises(lib.CsError):
        S.get_bbox(boxes, [2, 4, 9], CLASSES)
    with pytest.raises(lib.CsError):
        S.get_sdfusion_models(boxes, None, cats, CLASSES)
    with pytest.raises(lib.CsError):
        S.get_closest_furniture_to_box({}, torch.ones(3))
    with pytest.raises(lib.CsError):
        S.get_closest_furniture_to_box({"a": [1.0, 2.0, 3.0]}, torch.ones(4))
    with pytest.raises(lib.CsError, match="finite"):
        S.get_closest_furniture_to_box({"a": [1.0, float("nan"), 3.0]}, torch.ones(3))
    assert not touched
    # generated shapes: the marker path is assemble_scene; get_generated_models_v2 keeps refusing
    with pytest.raises(NotImplementedError):
        S.get_generated_models_v2(boxes, None, cats, CLASSES, render_boxes=True)


def _empty_meshes():
    from commonscenes_amd.mesh import Meshes
    return Meshes([], [])


def test_synthetic_library_is_closed_and_varied():
    from commonscenes_amd import synth
    table = synth.furniture_table(["chair\n", "table\n"], per_category=4)
    assert list(table) == ["chair", "table"]
    sizes = set()
    for entries in table.values():
        for mid, size, v, f in entries:
            v, f = v.double().numpy(), f.numpy()
            assert np.allclose(v.max(0) - v.min(0), size, rtol=1e-6) and v[:, 1].min() == 0
            edges = {}
            for t in f:
                for i in range(3):
                    edges[(t[i], t[(i + 1) % 3])] = edges.get((t[i], t[(i + 1) % 3]), 0) + 1
            assert all(n == 1 and edges.get((b, a)) == 1 for (a, b), n in edges.items())
            assert (v[f[:, 0]] * np.cross(v[f[:, 1]], v[f[:, 2]])).sum() > 0          # wound outward
            sizes.add(tuple(size))
    assert len(sizes) == 8
