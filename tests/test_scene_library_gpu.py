"""GPU suite of the scenes from a mesh library (commonscenes_amd/scene_library.py, scene_mesh.py, csrc/cs_scene_lib.hip).

Retrieval is gated bit for bit against the numpy restatement of helpers/util.py:74-77 (tests/_scene_library_ref.py), the
placement against fp64 `v.dot(R) + t` within the bound of tests/test_scene_mesh_gpu.py, 8 * 2^-24 * (sum |A_ij| |v_j| + |t_i|),
the box corners bit for bit against cs_scene_fit_boxes, and the tube markers -- this package's own construction, parity with
trimesh.creation.cylinder unpinned -- against the fp64 restatement of that construction within 2 * 2^-24 * max(1, |coordinate|)
(one rounding to fp32 plus the last-bit difference of device and host sin / cos)."""
import json
import os
import random
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import _scene_library_ref as R
from test_scene_mesh_gpu import CLASSES, make_boxes, make_objects, oracle_raster, to_meshes

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24
CAT_SIZES = [1, 63, 64, 65, 257, 5000]
LABELS = ["c1", "c63", "c64", "c65", "c257", "c5000"]


# ---------------------------------------------------------------- retrieval
@pytest.fixture(scope="module")
def big_library():
    """categories of 1, 63, 64, 65, 257 and 5000 rows and an empty one; in c257 rows 67 and 128 repeat rows 3 and 64, whose
    sizes are fp32 numbers (so a query can equal them)"""
    from commonscenes_amd.scene_library import FurnitureLibrary
    rng = np.random.default_rng(71)
    table = {}
    for lab, m in zip(LABELS, CAT_SIZES):
        s = rng.uniform(0.05, 3.0, (m, 3))
        if m == 257:
            s[3] = s[3].astype(np.float32)
            s[64] = s[64].astype(np.float32)
            s[67], s[128] = s[3], s[64]
        table[lab] = [(f"{lab}-{i}", s[i].tolist()) for i in range(m)]
        if m == 64:
            table["none"] = []
    return FurnitureLibrary(table)


def _queries(lib, q, seed):
    """q queries over the six populated categories (each at least once when q allows), some of them rows of the library
    rounded to fp32, the rest free"""
    rng = np.random.default_rng(seed)
    cats = [lib.label_index[LABELS[i % 6]] for i in range(q)] if q > 1 else [lib.label_index["c257"]]
    boxes = rng.uniform(0.05, 3.0, (q, 7)).astype(np.float32)
    for i in range(0, q, 3):
        lo, hi = lib.cat_base[cats[i]], lib.cat_base[cats[i] + 1]
        boxes[i, :3] = lib.sizes[rng.integers(lo, hi)].astype(np.float32)
    return boxes, cats


def _want(lib, boxes, cats):
    idx, d2 = [], []
    for b, c in zip(boxes, cats):
        lo, hi = lib.cat_base[c], lib.cat_base[c + 1]
        i, m = R.ref_retrieve(lib.sizes[lo:hi], b[:3])
        idx.append(lo + i)
        d2.append(m)
    return np.asarray(idx, dtype=np.int64), np.asarray(d2, dtype=np.float64)


@pytest.mark.parametrize("q", [1, 5, 257])
def test_retrieve_is_numpys_argmin_bit_for_bit(big_library, q):
    lib = big_library
    boxes, cats = _queries(lib, q, 100 + q)
    rows, d2, status = lib.retrieve_rows(torch.from_numpy(boxes), cats)          # the [Q,7] box tensor itself: row stride 7
    want_i, want_d = _want(lib, boxes, cats)
    assert (status.cpu().numpy() == 0).all()
    assert np.array_equal(rows.cpu().numpy(), want_i)
    assert np.array_equal(d2.cpu().numpy().view(np.uint64), want_d.view(np.uint64))
    if q >= 5:
        assert {c for c in cats} == {lib.label_index[l] for l in LABELS[:min(q, 6)]}


def test_retrieve_ties_go_to_the_lower_row_and_an_equal_query_has_distance_zero(big_library):
    lib = big_library
    c = lib.label_index["c257"]
    lo = lib.cat_base[c]
    q = np.stack([lib.sizes[lo + 3], lib.sizes[lo + 64], lib.sizes[lo + 67], lib.sizes[lo + 128]]).astype(np.float32)
    rows, d2, status = lib.retrieve_rows(torch.from_numpy(q), [c] * 4)
    assert rows.cpu().tolist() == [lo + 3, lo + 64, lo + 3, lo + 64] and (status.cpu().numpy() == 0).all()
    assert (d2.cpu().numpy() == 0).all()
    assert np.array_equal(rows.cpu().numpy(), _want(lib, q, [c] * 4)[0])          # np.argmin's first minimum
    # a one-row category answers that row whatever the query
    one = lib.label_index["c1"]
    rows, _, _ = lib.retrieve_rows(torch.tensor([[9.0, 9.0, 9.0]]), [one])
    assert rows.cpu().tolist() == [lib.cat_base[one]]


def test_retrieve_does_not_depend_on_the_batch_or_the_position(big_library):
    lib = big_library
    boxes, cats = _queries(lib, 257, 7)
    rows, d2, _ = lib.retrieve_rows(torch.from_numpy(boxes), cats)
    for k in (0, 1, 3, 4, 5, 130, 255, 256):                 # every wave slot of a workgroup, first and last workgroup
        r1, d1, _ = lib.retrieve_rows(torch.from_numpy(boxes[k:k + 1]), [cats[k]])
        assert r1.item() == rows[k].item()
        assert d1.cpu().numpy().view(np.uint64)[0] == d2[k:k + 1].cpu().numpy().view(np.uint64)[0]
    again = lib.retrieve_rows(torch.from_numpy(boxes[::-1].copy()), cats[::-1])
    assert torch.equal(again[0].flip(0), rows) and torch.equal(again[1].flip(0), d2)


def test_refused_queries_are_reported_one_by_one(big_library):
    from commonscenes_amd import lib as L
    lib = big_library
    boxes, cats = _queries(lib, 9, 13)
    boxes[1, 1] = np.nan
    boxes[6, 0] = np.inf
    cats[2] = lib.label_index["none"]
    cats[4], cats[7] = len(lib.labels), -1
    rows, d2, status = lib.retrieve_rows(torch.from_numpy(boxes), cats)
    rows, d2, status = rows.cpu().numpy(), d2.cpu().numpy(), status.cpu().numpy()
    assert status.tolist() == [0, L.RETRIEVE_STATUS_NONFINITE, L.RETRIEVE_STATUS_EMPTY, 0, L.RETRIEVE_STATUS_CATEGORY, 0,
                               L.RETRIEVE_STATUS_NONFINITE, L.RETRIEVE_STATUS_CATEGORY, 0]
    bad = status != 0
    assert (rows[bad] == -1).all() and np.isinf(d2[bad]).all()
    good = np.flatnonzero(~bad)
    want_i, want_d = _want(lib, boxes[good], [cats[i] for i in good])
    assert np.array_equal(rows[good], want_i) and np.array_equal(d2[good].view(np.uint64), want_d.view(np.uint64))
    # the public calls raise, naming the box and its label
    classes = [l + "\n" for l in lib.labels] + ["sofa\n"]
    b = torch.from_numpy(boxes)
    with pytest.raises(L.CsError, match=r"box 1 \('c63'\).*finite"):
        lib.retrieve(b[:2], [lib.label_index["c1"], lib.label_index["c63"]], classes)
    with pytest.raises(L.CsError, match=r"box 0 \('none'\).*empty"):
        lib.retrieve(b[:1], [lib.label_index["none"]], classes)
    with pytest.raises(L.CsError, match=r"box 0 \('sofa'\).*no such category"):
        lib.retrieve(b[:1], [len(classes) - 1], classes)


def test_public_retrieval_calls(big_library):
    from commonscenes_amd import scene_mesh as S
    lib = big_library
    classes = [l + "\n" for l in lib.labels]
    scenes = []
    for s, n in enumerate((3, 11, 1)):
        boxes, cats = _queries(lib, n, 40 + s)
        scenes.append((torch.from_numpy(boxes), cats))
    many = lib.retrieve_many(scenes, classes)
    for (boxes, cats), (ids, d2, rows) in zip(scenes, many):
        want_i, want_d = _want(lib, boxes.numpy(), cats)
        assert rows == want_i.tolist() and ids == [lib.ids[r] for r in want_i]
        assert np.array_equal(d2.cpu().numpy().view(np.uint64), want_d.view(np.uint64))
        ids1, d21 = lib.retrieve(boxes, cats, classes)
        assert ids1 == ids and torch.equal(d21, d2)
    # one query through get_closest_furniture_to_box, on the reference's own argument (box_data[label])
    boxes, cats = scenes[1]
    for j in (0, 4, 7):
        label = lib.labels[cats[j]]
        assert S.get_closest_furniture_to_box(lib.category(label), boxes[j, 0:3]) == many[1][0][j]


# ---------------------------------------------------------------- placement
def _entries():
    from commonscenes_amd import lib as L
    from commonscenes_amd.ops import _stream
    return L, L.load(), _stream()


@pytest.mark.parametrize("degrees", [True, False])
def test_box_corners_equal_the_fit_kernels_bit_for_bit(degrees):
    L, dll, stream = _entries()
    n = 37                                                   # angles 0, 90, 33.3, -270 in turn (make_boxes)
    boxes = torch.from_numpy(make_boxes(n, 5, degrees)).cuda()
    verts = torch.rand(4, 3, device="cuda")
    zero = torch.zeros(n, dtype=torch.int64, device="cuda")
    xf_fit, pts_fit = torch.empty(n, 12, device="cuda"), torch.empty(n, 8, 3, device="cuda")
    xf, pts = torch.full((n + 3, 12), -7.0, device="cuda"), torch.full((n + 3, 8, 3), -7.0, device="cuda")
    L.check(dll.cs_scene_fit_boxes(verts.data_ptr(), 4, zero.data_ptr(), zero.data_ptr(), boxes.data_ptr(), n, int(degrees),
                                   xf_fit.data_ptr(), pts_fit.data_ptr(), stream), "fit")
    L.check(dll.cs_scene_place_boxes(boxes.data_ptr(), n, int(degrees), xf.data_ptr(), pts.data_ptr(), stream), "place")
    assert torch.equal(pts[:n].view(torch.int32), pts_fit.view(torch.int32))
    assert (xf[n:] == -7).all() and (pts[n:] == -7).all()    # nothing past the n boxes
    b = boxes.cpu().numpy().astype(np.float64)
    got = xf[:n].cpu().numpy().astype(np.float64).reshape(n, 3, 4)
    for j in range(n):
        Rm = R.ref_rotation(b[j, 6], degrees)
        assert np.abs(got[j, :, :3] - Rm.T).max() <= 2 * EPS and np.array_equal(got[j, :, 3], b[j, 3:6])
        assert np.array_equal(got[j, 1], [0, 1, 0, b[j, 4]])


def _library_and_scene(n, seed, lamp_at=()):
    """a synthetic furniture library over chair / table / lamp and n boxes (with a _scene_ and a floor node among them)"""
    from commonscenes_amd import synth
    lib = synth.furniture_library(["chair\n", "lamp\n", "table\n"], per_category=6, seed=seed)
    boxes = make_boxes(n, seed)
    cats = [[2, 4][i % 2] for i in range(n)]
    for i in lamp_at:
        cats[i] = 3
    if n > 4:
        cats[1], cats[3] = 0, 1                              # _scene_, floor
    return lib, boxes, cats


def _expected_rows(lib, boxes, cats):
    rows = {}
    for j, c in enumerate(cats):
        label = CLASSES[c].strip()
        if label in ("_scene_", "floor"):
            continue
        k = lib.label_index[label]
        lo, hi = lib.cat_base[k], lib.cat_base[k + 1]
        rows[j] = lo + R.ref_retrieve(lib.sizes[lo:hi], boxes[j, :3])[0]
    return rows


def test_retrieval_scene_places_the_closest_models():
    from commonscenes_amd import scene_mesh as S
    lib, boxes, cats = _library_and_scene(9, 21, lamp_at=(6,))
    shaped = [j for j, c in enumerate(cats) if c not in (0, 1)]
    cols = np.random.default_rng(2).uniform(0, 1, (len(shaped), 3))
    scene = S.assemble_scene_from_library("retrieval", torch.from_numpy(boxes), cats, CLASSES, library=lib, colors=cols)
    rows = _expected_rows(lib, boxes, cats)
    assert scene.kept == shaped and scene.sources == [lib.ids[rows[j]] for j in shaped]
    got_v, got_f = scene.verts.cpu().numpy(), scene.faces.cpu().numpy()
    got_o, got_c = scene.face_object.cpu().numpy(), scene.vert_rgb.cpu().numpy()
    v0 = f0 = 0
    for k, j in enumerate(shaped):
        v, f = [t.cpu().numpy() for t in lib.mesh(rows[j])]
        want, mag = R.ref_place(v, boxes[j])
        err = np.abs(got_v[v0:v0 + len(v)].astype(np.float64) - want)
        assert (err <= 8 * EPS * mag).all(), f"box {j}: worst {err.max():.3e}"
        assert np.array_equal(got_f[f0:f0 + len(f)], f + v0)                  # not reversed: retrieval does not invert
        assert (got_o[f0:f0 + len(f)] == j).all()
        assert (got_c[v0:v0 + len(v)] == cols[k].astype(np.float32)[None]).all()   # colours: non-skipped nodes only
        assert scene.vert_counts[k] == len(v) and scene.face_counts[k] == len(f)
        v0, f0 = v0 + len(v), f0 + len(f)
    assert got_v.shape[0] == v0 and got_f.shape[0] == f0
    # the mesh is neither scaled nor inverted: its extent is the model's, its volume positive
    j = shaped[0]
    v, f = [t.cpu().numpy() for t in lib.mesh(rows[j])]
    p = got_v[:len(v)].astype(np.float64)
    a, b, c = p[f[:, 0]] - p[0], p[f[:, 1]] - p[0], p[f[:, 2]] - p[0]
    assert (a * np.cross(b, c)).sum() > 0
    assert abs((p[:, 1].max() - p[:, 1].min()) - (v[:, 1].max() - v[:, 1].min())) <= 16 * EPS * np.abs(p).max()


def test_lamps_and_markers_follow_the_reference_lists():
    from commonscenes_amd import scene_mesh as S
    lib, boxes, cats = _library_and_scene(8, 22, lamp_at=(2, 6))
    b = torch.from_numpy(boxes)
    shaped = [j for j, c in enumerate(cats) if c not in (0, 1)]
    cols = np.random.default_rng(3).uniform(0, 1, (len(shaped), 3))
    mv, mf = 12 * 10, 48 * 4
    # get_textured_objects_v2: the lamp's model leaves, its marker stays (util.py:131-135)
    full = S.assemble_scene_from_library("retrieval", b, cats, CLASSES, library=lib, colors=cols, render_boxes=True)
    lamps, objs, raws = S.get_textured_objects_v2(b, lib, cats, CLASSES, render_boxes=True, colors=cols, without_lamp=True)
    assert len(lamps) == 2 and len(raws) == len(shaped) and len(objs) == 2 * len(shaped) - 2
    parts = full.per_object()
    nobj = len(shaped)
    assert full.kept == shaped + shaped
    it = iter(objs)
    for k, j in enumerate(shaped):
        if cats[j] == 3:
            assert torch.equal(lamps[[2, 6].index(j)].vertices, parts[k].vertices)
        else:
            assert torch.equal(next(it).vertices, parts[k].vertices)
        m = next(it)                                         # the marker right after its object, lamp or not
        assert m.vertices.shape[0] == mv and m.faces.shape[0] == mf
        assert torch.equal(m.vertices, parts[nobj + k].vertices) and torch.equal(m.faces, parts[nobj + k].faces)
        assert (m.vertex_colors.cpu().numpy() == cols[k].astype(np.float32)[None]).all()
    rows = _expected_rows(lib, boxes, cats)
    for k, j in enumerate(shaped):                           # raw: the model as stored, coloured
        assert torch.equal(raws[k].vertices, lib.mesh(rows[j])[0]) and torch.equal(raws[k].faces, lib.mesh(rows[j])[1])
    nolamp = S.assemble_scene_from_library("retrieval", b, cats, CLASSES, library=lib, colors=cols, render_boxes=True,
                                           without_lamp=True)
    keep = [j for j in shaped if cats[j] != 3]
    assert nolamp.kept == keep + shaped
    # get_bbox: the lamp's marker itself goes to the lamp list (util.py:152-153)
    lamps, marks = S.get_bbox(b, cats, CLASSES, cols, without_lamp=True)
    assert len(lamps) == 2 and len(marks) == len(shaped) - 2
    only = S.assemble_scene_from_library("onlybox", b, cats, CLASSES, colors=cols, without_lamp=True)
    assert only.kept == keep and only.verts.shape[0] == len(keep) * mv
    for m, p in zip(marks, only.per_object()):
        assert torch.equal(m.vertices, p.vertices)
    assert np.array_equal(np.unique(only.face_object.cpu().numpy()), keep)
    lamps, marks = S.get_bbox(b, cats, CLASSES, cols)
    assert lamps == [] and len(marks) == len(shaped)


def test_one_object_alone_equals_the_same_object_among_33():
    from commonscenes_amd import scene_mesh as S
    lib, boxes, cats = _library_and_scene(35, 23)
    b = torch.from_numpy(boxes)
    shaped = [j for j, c in enumerate(cats) if c not in (0, 1)]
    assert len(shaped) == 33
    scene = S.assemble_scene_from_library("retrieval", b, cats, CLASSES, library=lib, render_boxes=True)
    parts = scene.per_object()
    for k in (0, 19, 32):
        j = shaped[k]
        alone = S.assemble_scene_from_library("retrieval", b[j:j + 1], [cats[j]], CLASSES, library=lib, render_boxes=True)
        one = alone.per_object()
        assert torch.equal(one[0].vertices, parts[k].vertices) and torch.equal(one[0].faces, parts[k].faces)
        assert torch.equal(one[1].vertices, parts[33 + k].vertices) and torch.equal(one[1].faces, parts[33 + k].faces)
        assert torch.equal(alone.box_points[0], scene.box_points[j]) and alone.sources == [scene.sources[k]]


# ---------------------------------------------------------------- markers
def _tube_checks(v, f, S, r, lens):
    """per tube: closed and consistently wound, signed volume (S/2) sin(2 pi / S) r^2 len within the fp32 rounding of the
    vertices (every coordinate moved by at most 2^-24 |coordinate|: |dV| <= surface area * sqrt(3) * that, doubled)"""
    tv, tf = 2 * S + 2, 4 * S
    r = float(np.float32(r))
    for e in range(12):
        ff = f[e * tf:(e + 1) * tf]
        assert ff.min() == e * tv and ff.max() == (e + 1) * tv - 1
        edges = {}
        for t in ff:
            for i in range(3):
                k = (int(t[i]), int(t[(i + 1) % 3]))
                edges[k] = edges.get(k, 0) + 1
        assert all(n == 1 and edges.get((b, a)) == 1 for (a, b), n in edges.items())
        p = v[e * tv:(e + 1) * tv].astype(np.float64)
        o = p[0]
        a, b, c = v[ff[:, 0]] - o, v[ff[:, 1]] - o, v[ff[:, 2]] - o
        vol = (a.astype(np.float64) * np.cross(b.astype(np.float64), c.astype(np.float64))).sum() / 6
        want = S / 2 * np.sin(2 * np.pi / S) * r * r * lens[e]
        area = S * 2 * r * np.sin(np.pi / S) * lens[e] + S * np.sin(2 * np.pi / S) * r * r
        tol = 2 * area * np.sqrt(3) * EPS * max(1.0, np.abs(p).max()) + 1e-12 * want
        assert abs(vol - want) <= tol, (e, vol, want, tol)
        assert lens[e] == 0 or vol > 0


@pytest.mark.parametrize("sections", [3, 4, 8])
@pytest.mark.parametrize("radius", [0.02, 0.006])
def test_markers_match_the_fp64_restatement(sections, radius):
    from commonscenes_amd import scene_mesh as S
    n = 6
    boxes = make_boxes(n, 31)                                # angles 0, 90, 33.3, -270, 0, 90
    boxes[4, 6] = 12.5
    cats = [2, 0, 4, 2, 1, 4]
    cols = np.random.default_rng(5).uniform(0, 1, (4, 3))
    scene = S.assemble_scene_from_library("onlybox", torch.from_numpy(boxes), cats, CLASSES, colors=cols,
                                          tube_radius=radius, sections=sections)
    kept = [0, 2, 3, 5]
    mv, mf = 12 * (2 * sections + 2), 48 * sections
    assert scene.kept == kept and scene.vert_counts == [mv] * 4 and scene.face_counts == [mf] * 4
    assert scene.verts.shape == (4 * mv, 3) and scene.faces.shape == (4 * mf, 3)
    pts = scene.box_points.cpu().numpy()
    got_v, got_f, got_o = scene.verts.cpu().numpy(), scene.faces.cpu().numpy(), scene.face_object.cpu().numpy()
    got_c = scene.vert_rgb.cpu().numpy()
    for k, j in enumerate(kept):
        V, F, lens = R.ref_marker(pts[j], radius, sections)
        g = got_v[k * mv:(k + 1) * mv]
        err = np.abs(g.astype(np.float64) - V)
        assert (err <= 2 * EPS * np.maximum(1.0, np.abs(V))).all(), f"box {j}: worst {err.max():.3e}"
        assert np.array_equal(got_f[k * mf:(k + 1) * mf], F + k * mv)
        assert (got_o[k * mf:(k + 1) * mf] == j).all()
        assert (got_c[k * mv:(k + 1) * mv] == cols[k].astype(np.float32)[None]).all()
        _tube_checks(g, F, sections, radius, lens)
        # the same box through create_bbox_marker: the same bits, local ids
        m = S.create_bbox_marker(scene.box_points[j], color=cols[k], tube_radius=radius, sections=sections)
        assert torch.equal(m.vertices, scene.verts[k * mv:(k + 1) * mv])
        assert np.array_equal(m.faces.cpu().numpy(), F)
    assert S.create_bbox_marker(pts[0]).vertex_colors[0].tolist() == [0.0, 0.0, 1.0]     # the reference's default: 0..255


def test_flat_box_gives_zero_area_tubes_and_the_scene_still_renders():
    from commonscenes_amd import scene_mesh as S
    boxes = make_boxes(3, 33)
    boxes[:, 3:6] = [[-2, 0, -2], [2, 0, 1], [0, 0, 2.5]]
    boxes[1, 1] = 0.0                                        # h = 0: the four vertical edges have no length
    cats = [2, 4, 2]
    scene = S.assemble_scene_from_library("onlybox", torch.from_numpy(boxes), cats, CLASSES)
    mv, mf = 120, 192
    v = scene.verts.cpu().numpy()[mv:2 * mv].astype(np.float64)
    f = scene.faces.cpu().numpy()[mf:2 * mf] - mv
    pts = scene.box_points.cpu().numpy()[1]
    assert torch.isfinite(scene.verts).all()
    for e, (ia, ib) in enumerate(R.EDGES):
        ff = f[e * 16:(e + 1) * 16]
        area = np.linalg.norm(np.cross(v[ff[:, 1]] - v[ff[:, 0]], v[ff[:, 2]] - v[ff[:, 0]]), axis=1)
        if (pts[ia] == pts[ib]).all():
            assert e in (1, 3, 9, 10)
            assert (v[e * 10:(e + 1) * 10] == pts[ia].astype(np.float64)[None]).all() and (area == 0).all()
        else:
            assert (area > 0).any()
    assert [e for e, (ia, ib) in enumerate(R.EDGES) if (pts[ia] == pts[ib]).all()] == [1, 3, 9, 10]
    out = S.render_topdown(scene, 512)
    others = S.assemble_scene_from_library("onlybox", torch.from_numpy(boxes[[0, 2]]), [2, 2], CLASSES)
    assert out["dropped"] == S.render_topdown(others, 512)["dropped"] == 0
    assert set(np.unique(out["object_id"].cpu().numpy())) == {-1, 0, 1, 2}


def test_onlybox_scene_matches_the_integer_rasteriser_pixel_for_pixel():
    """one rotated box near the camera (depth 2.07 .. 3.55) at 512 pixels: a side of the 0.02 tube's square section, 0.0283,
    spans 512 * 0.0283 / (2 * 3.55) = 2.04 pixels at the far end.  The oracle projects in fp64, the kernel in fp32; the box
    is chosen so that both snap every vertex to the same 1/256 pixel, which the test checks first."""
    from commonscenes_amd import scene_mesh as S
    size = 512
    boxes = np.asarray([[0.1, 0.1, 0.1, 0, 0, 0, 0], [1.671875, 1.4375, 1.328125, -0.515625, 4.46875, 0.21875, 30.0]],
                       dtype=np.float32)
    scene = S.assemble_scene_from_library("onlybox", torch.from_numpy(boxes), [0, 2], CLASSES)
    v32, f, o = scene.verts.cpu().numpy(), scene.faces.cpu().numpy(), scene.face_object.cpu().numpy()
    assert v32.shape == (120, 3) and (o == 1).all()
    d32 = np.float32(8.0) - v32[:, 1]
    assert d32.max() <= 3.56 and size * 0.02 * np.sqrt(2) / (2 * d32.max()) >= 2.0
    for a in (0, 2):                                         # tri_setup / snap of csrc/cs_scene.hip, cs_raster.h in fp32
        pix = ((np.float32(1.0) + v32[:, a] / d32) * np.float32(0.5)) * np.float32(size)
        got = np.floor(pix * np.float32(256) + np.float32(0.5)).astype(np.int64)
        want = np.floor((1 + v32[:, a].astype(np.float64) / (8.0 - v32[:, 1].astype(np.float64))) / 2 * size * 256 + 0.5)
        assert np.array_equal(got, want.astype(np.int64)), "the test's box no longer projects alike in fp32 and fp64"
    out = S.render_topdown(scene, size)
    oid = out["object_id"].cpu().numpy()
    best, win, _, dropped = oracle_raster(v32, f, size)
    assert out["dropped"] == dropped == 0
    assert np.array_equal(oid, np.where(win >= 0, 1, -1))
    assert 2000 < (oid == 1).sum() < 0.2 * size * size       # twelve thin lines, not a filled box


# ---------------------------------------------------------------- the library type, assemble_scene, the tools
def _shape_folder(tmp_path):
    from commonscenes_amd.scene_library import ShapeLibrary
    rng = np.random.default_rng(9)
    for lab, n in (("chair", 5), ("table", 4), ("lamp", 2), ("stool", 3)):
        (tmp_path / lab).mkdir()
        for k in range(n):
            v, f = R.box_mesh(rng.uniform(0.3, 1.5, 3))
            v = v + rng.uniform(-0.2, 0.2, (1, 3)).astype(np.float32)
            R.write_ply(tmp_path / lab / f"{lab}_{k}.ply", v, f, binary=bool(k % 2))
    return ShapeLibrary(tmp_path)


@pytest.mark.parametrize("no_stool", [False, True])
def test_library_type_equals_assemble_scene_on_the_drawn_meshes(tmp_path, no_stool):
    from commonscenes_amd import scene_mesh as S
    from commonscenes_amd.scene_library import read_ply
    sl = _shape_folder(tmp_path)
    n = 8
    boxes = torch.from_numpy(make_boxes(n, 51))
    cats = [2, 0, 4, 2, 1, 3, 2, 4]
    shaped = [j for j, c in enumerate(cats) if c not in (0, 1)]
    labels = [CLASSES[cats[j]].strip() for j in shaped]
    cols = np.random.default_rng(6).uniform(0, 1, (len(shaped), 3))
    paths = R.ref_choices(labels, sl.files, no_stool, 48)
    meshes = [read_ply(p) for p in paths]
    want = S.assemble_scene(to_meshes([m[0].numpy() for m in meshes], [m[1].numpy() for m in meshes]), boxes, cats, CLASSES,
                            colors=cols, without_lamp=True)
    got = S.assemble_scene_from_library("library", boxes, cats, CLASSES, library=sl, colors=cols, without_lamp=True,
                                        no_stool=no_stool, rng=random.Random(48))
    assert got.sources == [p for p, l in zip(paths, labels) if l != "lamp"] and got.kept == want.kept
    for x, y in ((got.verts, want.verts), (got.faces, want.faces), (got.vert_rgb, want.vert_rgb),
                 (got.face_object, want.face_object), (got.box_points, want.box_points)):
        assert torch.equal(x, y)
    f0 = meshes[0][1].numpy()
    assert np.array_equal(got.faces.cpu().numpy()[:len(f0)], f0[:, ::-1])           # inverted (util.py:361)
    lamps, objs, raws = S.get_sdfusion_models(boxes, sl, cats, CLASSES, mesh_dir=tmp_path / "out", render_boxes=True,
                                              colors=cols, no_stool=no_stool, without_lamp=True, rng=random.Random(48))
    assert len(lamps) == 1 and len(raws) == len(shaped) and len(objs) == 2 * len(shaped) - 1
    kept_parts = want.per_object()
    objs_only = [m for m in objs if m.vertices.shape[0] != 120] + []
    assert len(objs_only) == len(kept_parts) and all(torch.equal(a.vertices, b.vertices) for a, b in zip(objs_only, kept_parts))
    assert sum(m.vertices.shape[0] == 120 for m in objs) == len(shaped)            # a marker per shaped box, the lamp's too
    assert np.array_equal(raws[0].faces.cpu().numpy(), f0[:, ::-1]) and torch.equal(raws[0].vertices.cpu(), meshes[0][0])
    assert sorted(os.listdir(tmp_path / "out")) == sorted(f"{l}_{cats[j]}_{k + 1}.obj" for k, (j, l) in
                                                           enumerate(zip(shaped, labels)))


def test_assemble_scene_without_markers_is_unchanged_and_with_markers_appends_them():
    from commonscenes_amd import scene_mesh as S
    cats = [2, 0, 4, 1, 3, 2]
    vs, fs = make_objects([40, 70, 9, 130], 31)
    boxes = torch.from_numpy(make_boxes(6, 32))
    m = to_meshes(vs, fs)
    base = S.assemble_scene(m, boxes, cats, CLASSES, floor=True, without_lamp=True)
    plain = S.assemble_scene(m, boxes, cats, CLASSES, floor=True, without_lamp=True, render_boxes=False)
    marked = S.assemble_scene(m, boxes, cats, CLASSES, floor=True, without_lamp=True, render_boxes=True)
    for name in ("verts", "faces", "vert_rgb", "face_object", "box_points"):
        assert torch.equal(getattr(base, name), getattr(plain, name))
    assert base.kept == plain.kept == [0, 2, 5, 6] and marked.kept == [0, 2, 5, 0, 2, 4, 5, 6]      # the lamp's marker stays
    nv, nf = sum(base.vert_counts[:3]), sum(base.face_counts[:3])
    assert torch.equal(marked.verts[:nv], base.verts[:nv]) and torch.equal(marked.faces[:nf], base.faces[:nf])
    assert torch.equal(marked.verts[-4:], base.verts[-4:])                                        # then the floor
    assert torch.equal(marked.faces[-2:] - marked.verts.shape[0], base.faces[-2:] - base.verts.shape[0])
    assert marked.verts.shape[0] == base.verts.shape[0] + 4 * 120
    pts = marked.box_points.cpu().numpy()
    for k, j in enumerate([0, 2, 4, 5]):                     # radius 0.006 (util.py:331), four sections
        V, F, _ = R.ref_marker(pts[j], 0.006, 4)
        g = marked.verts[nv + k * 120:nv + (k + 1) * 120].cpu().numpy().astype(np.float64)
        assert (np.abs(g - V) <= 2 * EPS * np.maximum(1.0, np.abs(V))).all()
        assert np.array_equal(marked.faces[nf + k * 192:nf + (k + 1) * 192].cpu().numpy(), F + nv + k * 120)
        assert (marked.face_object[nf + k * 192:nf + (k + 1) * 192] == j).all()


@pytest.mark.parametrize("render_type", ["retrieval", "onlybox"])
def test_walkthrough_exports_layout_scenes_without_sampling(tmp_path, render_type):
    env = dict(os.environ, CS_ONE_DEVICE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, str(ROOT / "tools" / "eval_walkthrough.py"), "--scenes", "2", "--export-scenes", str(tmp_path),
           "--render-type", render_type, "--library", "synthetic", "--render-boxes"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=str(ROOT))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("EVAL_WALKTHROUGH ")]
    assert len(lines) == 1
    d = json.loads(lines[0].split(" ", 1)[1])
    assert d["render_type"] == render_type and d["sampler_calls"] == 0 and len(d["scenes"]) == 2
    for s, nobj in zip(d["scenes"], (4, 5)):
        e = s["export"]
        assert (tmp_path / f"{s['scan']}.obj").stat().st_size > 0 and (tmp_path / f"{s['scan']}.png").stat().st_size > 0
        assert e["render_boxes"] is True and s["shapes"] == 0 and s["finite"]
        assert len(e["sources"]) == (nobj if render_type == "retrieval" else 0)
        assert e["faces"] >= nobj * 192 + 2
