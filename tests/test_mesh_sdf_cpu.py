"""mesh_to_sdf without a GPU: known answers of the fp64 restatement (tests/_mesh_sdf_ref.py) that do not lean on the kernels,
the host-side slice plan, the .obj reader and the host-side argument checks."""
import ctypes as C

import numpy as np
import pytest
import torch

import _mesh_sdf_ref as R


def test_octant_triangle_seen_from_the_origin_is_one_eighth():
    tri = np.array([[[1, 0, 0], [0, 1, 0], [0, 0, 1.0]]])
    w = R.winding(np.zeros((1, 3)), tri)
    assert abs(abs(w[0]) - 0.125) <= 1e-15


def test_box_against_the_closed_form():
    v, f = R.box()
    p = R.grid_points(12)
    sd, d, w = R.sdf(p, v[f])
    err = np.abs(sd - R.box_sdf(p)).max()
    print(f"box n=12: max |sdf - closed form| {err:.2e}, min d {d.min():.3e}")
    assert err <= 1e-14
    assert np.abs(w - np.round(w)).max() <= 1e-12 and set(np.round(w).astype(int)) <= {0, 1, -1}


def test_closed_mesh_has_integer_winding_off_the_surface():
    for sub, n in ((1, 16), (2, 17)):
        v, f = R.icosphere(sub)
        assert len(f) == 20 * 4 ** sub
        p = R.grid_points(n)
        w = R.winding(p, v[f])
        assert np.abs(w - np.round(w)).max() <= 1e-11
        r = np.linalg.norm(p - R.OFF, axis=1)
        inner = R.ICO_RADIUS * np.cos(np.pi / 5)        # inside every face's plane of the coarsest sphere
        assert np.all(np.abs(np.round(w[r < 0.5 * inner])) == 1) and np.all(np.round(w[r > R.ICO_RADIUS]) == 0)


def test_hemisphere_is_open_with_fractional_winding():
    v, f = R.hemisphere(2)
    assert len(f) == 168
    w = R.winding(R.grid_points(16), v[f])
    assert np.abs(w - np.round(w)).max() > 0.1
    assert np.abs(np.abs(w) - 0.5).min() >= 1e-4        # what lets the GPU test compare the sign at every node


def test_degenerate_triangles_are_segments_and_contribute_no_winding():
    p = R.grid_points(5)
    a, b = np.array([0.1, 0.2, -0.3]), np.array([0.7, -0.4, 0.2])
    seg = R._segment_dist(p, a, b)
    for tri in ([a, b, b], [a, a, b], [a, 0.5 * (a + b), b]):
        t = np.array([tri])
        assert np.abs(R.distance(p, t) - seg).max() <= 1e-15
        assert np.all(R.winding(p, t) == 0)
    assert np.abs(R.distance(p, np.array([[a, a, a]])) - np.linalg.norm(p - a, axis=1)).max() <= 1e-15


def test_get_normalize_mesh_of_a_box():
    v, f = R.box()
    out, cen, m = R.get_normalize_mesh(v * 3.0 + 2.0, f)
    assert np.abs(cen - (R.OFF * 3.0 + 2.0)).max() <= 1e-14
    assert abs(m - 3.0 * np.linalg.norm(R.BOX_HALF)) <= 1e-14
    assert abs(np.linalg.norm(out, axis=1).max() - 1.0) <= 1e-15


def test_plan_is_a_function_of_faces_and_n_only():
    from commonscenes_amd import lib as L, mesh_sdf
    dll = L.load()
    s, b = C.c_int32(-1), C.c_int64(-1)
    for bad in ((0, 64), (-3, 64), (100, 0), (100, 1), (100, 1025)):
        assert dll.cs_mesh_sdf_plan(bad[0], bad[1], C.byref(s), C.byref(b)) == L.CS_EINVAL
    assert dll.cs_mesh_sdf_plan(100, 64, None, C.byref(b)) == L.CS_EINVAL
    assert dll.cs_mesh_sdf_plan(100, 64, C.byref(s), None) == L.CS_EINVAL
    seen = {}
    for n in (2, 5, 16, 33, 64):
        for faces in (1, 255, 256, 257, 512, 513, 1280, 10_000, 100_000, 5_000_000):
            got = mesh_sdf.plan(faces, n)
            assert got == mesh_sdf.plan(faces, n)
            slices, ws = got
            chunks = -(-faces // L.SDF_CHUNK)
            assert 1 <= slices <= min(L.SDF_MAX_SLICES, chunks)
            assert ws % 16 == 0 and ws >= slices * n ** 3 * 12
            seen[(faces, n)] = slices
    # a slice is at least two chunks long; one 64^3 grid is 256 workgroups, so long meshes get four slices there
    assert seen[(512, 16)] == 1 and seen[(513, 16)] == 2 and seen[(1280, 16)] == 3
    assert seen[(1, 64)] == 1 and seen[(10_000, 64)] == 4 and seen[(100_000, 64)] == 4
    with pytest.raises(ValueError):
        mesh_sdf.plan(0, 64)


def test_read_obj_quads_negative_and_slashed_indices(tmp_path):
    from commonscenes_amd.mesh_sdf import read_obj
    p = tmp_path / "m.obj"
    p.write_text("# a comment\nmtllib x.mtl\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0 0.5\nvn 0 0 1\nvt 0.5 0.5\n"
                 "f 1 2 3 4\nv 0 0 1\nf -1 1/1/1 2/1/1\nf 3//1 4//1 5//1\nusemtl m\nf 1 2 3 4 5\n")
    v, f = read_obj(p)
    assert v.dtype == torch.float32 and tuple(v.shape) == (5, 3) and v[4].tolist() == [0.0, 0.0, 1.0]
    assert f.dtype == torch.int64
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [4, 0, 1], [2, 3, 4], [0, 1, 2], [0, 2, 3], [0, 3, 4]]


def test_display_to_grid_maps_node_indices_to_node_positions():
    from commonscenes_amd.mesh_sdf import display_to_grid
    n, bound = 32, 1.0
    idx = torch.tensor([[0.0, 15.5, 31.0]], dtype=torch.float64)
    got = display_to_grid(idx / n - 0.5, n, bound)
    want = -bound + idx * (2 * bound / (n - 1))
    assert torch.allclose(got, want, atol=1e-14) and got[0, 0] == -1.0 and abs(float(got[0, 2]) - 1.0) <= 1e-15


def test_host_side_value_errors():
    from commonscenes_amd.mesh_sdf import mesh_to_sdf
    v = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=torch.float32)
    f = torch.tensor([[0, 1, 2]])
    for kw in (dict(res=1), dict(res=0), dict(bound=0.0), dict(bound=-1.0), dict(sign="flood"), dict(wind_level=0.0),
               dict(trunc=0.0)):
        with pytest.raises(ValueError):
            mesh_to_sdf([v], [f], **kw)
    for vv, ff in (([], []), ([v], [f, f]), ([v[:0]], [f]), ([v], [f[:0]]), ([v], [f.float()]), ([v[:, :2]], [f])):
        with pytest.raises(ValueError):
            mesh_to_sdf(vv, ff)
    with pytest.raises(ValueError):
        mesh_to_sdf([v])


def test_lib_constants_mirror_the_header():
    import re
    from pathlib import Path
    from commonscenes_amd import lib as L
    txt = (Path(__file__).resolve().parent.parent / "include" / "commonscenes_hip.h").read_text()
    defs = {k: int(v) for k, v in re.findall(r"#define (CS_SDF_[A-Z_]+) (\d+)", txt)}
    assert defs == {"CS_SDF_CHUNK": L.SDF_CHUNK, "CS_SDF_MAX_SLICES": L.SDF_MAX_SLICES,
                    "CS_SDF_MOMENT_BLOCKS": L.SDF_MOMENT_BLOCKS, "CS_SDF_STATUS_INDEX": L.SDF_STATUS_INDEX,
                    "CS_SDF_STATUS_NONFINITE": L.SDF_STATUS_NONFINITE, "CS_SDF_STATUS_RANGE": L.SDF_STATUS_RANGE,
                    "CS_SDF_STATUS_EMPTY": L.SDF_STATUS_EMPTY}
