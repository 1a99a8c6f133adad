"""GPU suite of the scene assembly and the top-down view (commonscenes_amd/scene_mesh.py, csrc/cs_scene.hip).

Fit / apply are gated against an fp64 numpy restatement of helpers/util.py:158-189 kept in this file:
    |got - want| <= 8 * 2^-24 * (sum_j |A_ij| |v_j| + |t_i|)
(eight roundings: one each for A and t, three multiplies, three adds; the build has -ffp-contract=off).  The rasteriser is
gated against an integer-math numpy rasteriser kept in this file, on inputs whose projection is exact in fp32 (heights in
{0, 4, 6} -> depths 8, 4, 2; x / z multiples of 2^-6; 64 pixels)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
CLASSES = ["_scene_\n", "floor\n", "chair\n", "lamp\n", "table\n"]
ANGLES = [0.0, 90.0, 33.3, -270.0]


# ---------------------------------------------------------------- fp64 restatement of the reference's fit
def ref_rotation_3dfront(y, degree):                             # helpers/util.py:510-516
    if degree:
        y = np.deg2rad(y)
    return np.array([[np.cos(y), 0, -np.sin(y)], [0, 1, 0], [np.sin(y), 0, np.cos(y)]])


def ref_fit_map(v, box, degrees):
    """helpers/util.py:158-189 as (A [3,3], t [3], box_points [8,3], R, degenerate) in fp64; v: [V,3] fp32 array.  An axis of
    zero extent maps to 0 before the translation (the reference divides by zero there)."""
    l, h, w, px, py, pz, angle = [float(x) for x in box]
    corners = np.asarray([[l / 2 * i, h * j, w / 2 * k] for i in [-1, 1] for j in [0, 1] for k in [-1, 1]])
    R = ref_rotation_3dfront(angle, degrees)
    t = np.array([px, py, pz])
    box_points = corners.dot(R) + t[None]
    if v.shape[0] == 0:
        return np.eye(3), np.zeros(3), box_points, R, True
    v = v.astype(np.float64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    c = lo + (hi - lo) / 2
    c[1] = lo[1]
    P = np.array([[0.0, 0, -1], [0, 1, 0], [1, 0, 0]])           # rotation_matrix(-pi/2, [0,1,0]), exact permutation
    v1 = v.dot(P.T) - c[None]
    s = v1.max(axis=0) - v1.min(axis=0)
    k = np.where(s > 0, np.array([l, h, w]) / np.where(s > 0, s, 1.0), 0.0)
    Rinv = np.linalg.inv(R)
    A = Rinv @ np.diag(k) @ P
    tt = -(Rinv @ np.diag(k)) @ c + t
    return A, tt, box_points, R, bool((s <= 0).any())


def bound(A, t, v):
    return 8 * EPS * (np.abs(v.astype(np.float64)).dot(np.abs(A).T) + np.abs(t)[None])


def make_objects(counts, seed):
    rng = np.random.default_rng(seed)
    vs, fs = [], []
    for i, c in enumerate(counts):
        v = rng.uniform(-0.5, 0.5, (c, 3)).astype(np.float32)
        if i % 2 == 1 and c >= 2:                 # every other object: x / z bounds symmetric about 0, like a meshed SDF
            v[0, 0], v[1, 0], v[0, 2], v[1, 2] = -0.5, 0.5, 0.5, -0.5
        vs.append(v)
        nf = 0 if c == 0 else max(1, 2 * c - 4)
        fs.append(rng.integers(0, max(c, 1), (nf, 3)).astype(np.int64))
    return vs, fs


def make_boxes(n, seed, degrees=True):
    rng = np.random.default_rng(seed)
    ang = np.array([ANGLES[i % 4] for i in range(n)])
    if not degrees:
        ang = np.deg2rad(ang)
    b = np.concatenate([rng.uniform(0.3, 2.5, (n, 3)), rng.uniform(-10, 10, (n, 3)), ang[:, None]], axis=1)
    return b.astype(np.float32)


def to_meshes(vs, fs):
    from commonscenes_amd.mesh import Meshes
    return Meshes([torch.from_numpy(v) for v in vs], [torch.from_numpy(f) for f in fs])


def check_scene(scene, vs, fs, boxes, kept, degrees, flip=True):
    """every coordinate, box corner, face id and face_object of `scene` against the restatement; kept: node index per mesh"""
    got_v, got_f = scene.verts.cpu().numpy(), scene.faces.cpu().numpy()
    got_o, got_p = scene.face_object.cpu().numpy(), scene.box_points.cpu().numpy()
    assert scene.kept == list(kept)
    v0 = f0 = 0
    for k, j in enumerate(kept):
        A, t, pts, R, degenerate = ref_fit_map(vs[k], boxes[j], degrees)
        nv, nf = vs[k].shape[0], fs[k].shape[0]
        want = vs[k].astype(np.float64).dot(A.T) + t[None]
        err = np.abs(got_v[v0:v0 + nv].astype(np.float64) - want)
        assert (err <= bound(A, t, vs[k])).all(), f"object {k}: worst {err.max():.3e}"
        corners = np.asarray([[boxes[j][0] / 2 * a, boxes[j][1] * b, boxes[j][2] / 2 * c]
                              for a in [-1, 1] for b in [0, 1] for c in [-1, 1]], dtype=np.float64)
        perr = np.abs(got_p[j].astype(np.float64) - pts)
        assert (perr <= 8 * EPS * (np.abs(corners).dot(np.abs(R)) + np.abs(boxes[j][3:6].astype(np.float64))[None])).all()
        wf = fs[k][:, ::-1] if flip else fs[k]
        assert np.array_equal(got_f[f0:f0 + nf], wf + v0)
        assert (got_o[f0:f0 + nf] == j).all()
        lo, hi = (vs[k].min(axis=0), vs[k].max(axis=0)) if nv else (np.zeros(3), np.ones(3))
        # the reference takes the centre from the UNROTATED bounds and subtracts it after the (x,y,z) -> (-z,y,x) turn (a quirk
        # the port keeps), so an object sits centred in its box exactly when its x / z bounds are symmetric about 0
        if not degenerate and nv > 1 and lo[0] == -hi[0] and lo[2] == -hi[2]:
            # back in the box frame u = R (v3 - t) the object spans [-l/2, l/2] x [0, h] x [-w/2, w/2]; R mixes x and z with
            # |cos| + |sin| <= sqrt 2, so the bound of a coordinate is sqrt 2 times the worst bound of the object
            u = (got_v[v0:v0 + nv].astype(np.float64) - boxes[j][3:6].astype(np.float64)[None]).dot(R.T)
            tol = np.sqrt(2) * bound(A, t, vs[k]).max()
            l, h, w = [float(x) for x in boxes[j][:3]]
            assert np.abs(u.min(axis=0) - [-l / 2, 0, -w / 2]).max() <= tol
            assert np.abs(u.max(axis=0) - [l / 2, h, w / 2]).max() <= tol
        v0, f0 = v0 + nv, f0 + nf
    assert got_v.shape[0] == v0 and got_f.shape[0] == f0


def test_ragged_call_matches_the_fp64_restatement():
    from commonscenes_amd import scene_mesh as S
    counts = [0, 1, 3, 63, 64, 65, 257, 4097]     # below a wave, at its edge, past one workgroup pass
    vs, fs = make_objects(counts, 1)
    boxes = make_boxes(len(counts), 2)
    scene = S.assemble_scene(to_meshes(vs, fs), torch.from_numpy(boxes), [2] * len(counts), CLASSES)
    check_scene(scene, vs, fs, boxes, range(len(counts)), degrees=True)
    assert torch.isfinite(scene.verts).all()
    rgb = scene.vert_rgb.cpu().numpy()
    assert np.array_equal(rgb, np.repeat(S.hls_palette(5)[[2]].astype(np.float32), rgb.shape[0], axis=0))
    parts = scene.per_object()
    assert [p.vertices.shape[0] for p in parts] == counts
    assert np.array_equal(parts[7].faces.cpu().numpy(), fs[7][:, ::-1])


@pytest.mark.parametrize("n,degrees", [(1, True), (7, True), (33, True), (7, False)])
def test_calls_of_1_7_33_objects(n, degrees):
    from commonscenes_amd import scene_mesh as S
    counts = [(17 + 131 * i) % 300 + 2 for i in range(n)]
    vs, fs = make_objects(counts, 10 + n)
    boxes = make_boxes(n, 20 + n, degrees)
    cols = np.random.default_rng(3).uniform(0, 1, (n, 3))
    scene = S.assemble_scene(to_meshes(vs, fs), torch.from_numpy(boxes).cuda(), torch.full((n,), 4), CLASSES, colors=cols,
                             degrees=degrees, flip=False)
    check_scene(scene, vs, fs, boxes, range(n), degrees, flip=False)
    rgb, v0 = scene.vert_rgb.cpu().numpy(), 0
    for k, c in enumerate(counts):
        assert (rgb[v0:v0 + c] == cols[k].astype(np.float32)[None]).all()
        v0 += c


def test_filtered_classes_shift_nothing_else():
    from commonscenes_amd import scene_mesh as S
    cats = [2, 0, 4, 1, 3, 2]                     # chair, _scene_, table, floor, lamp, chair
    shaped = [0, 2, 4, 5]
    vs, fs = make_objects([40, 70, 9, 130], 31)
    boxes = make_boxes(6, 32)
    cols = np.random.default_rng(4).uniform(0, 1, (4, 3))
    m = to_meshes(vs, fs)
    full = S.assemble_scene(m, torch.from_numpy(boxes), cats, CLASSES, colors=cols)
    check_scene(full, vs, fs, boxes, shaped, True)
    nolamp = S.assemble_scene(m, torch.from_numpy(boxes), cats, CLASSES, colors=cols, without_lamp=True)
    keep = [0, 1, 3]
    check_scene(nolamp, [vs[k] for k in keep], [fs[k] for k in keep], boxes, [0, 2, 5], True)
    # each kept object: the same bits as alone, and the k-th SHAPED object took colors[k] (next(colors), util.py:313)
    parts = nolamp.per_object()
    for p, k in zip(parts, keep):
        alone = S.assemble_scene(to_meshes([vs[k]], [fs[k]]), torch.from_numpy(boxes[shaped[k]:shaped[k] + 1]), [2], CLASSES)
        assert torch.equal(p.vertices, alone.verts) and torch.equal(p.faces, alone.faces)
        assert (p.vertex_colors.cpu().numpy() == cols[k].astype(np.float32)[None]).all()
    lamps, objs, raws = S.get_generated_models_v2(torch.from_numpy(boxes), m, cats, CLASSES, colors=cols, without_lamp=True)
    assert len(lamps) == 1 and len(objs) == 3 and len(raws) == 4
    assert torch.equal(lamps[0].vertices, full.per_object()[2].vertices)
    assert all(torch.equal(o.vertices, p.vertices) for o, p in zip(objs, parts))
    assert np.array_equal(raws[1].faces.cpu().numpy(), fs[1][:, ::-1]) and np.array_equal(raws[1].vertices.numpy(), vs[1])


def test_alone_equals_batched_and_runs_repeat_bit_for_bit():
    from commonscenes_amd import scene_mesh as S
    n = 33
    counts = [(29 + 97 * i) % 500 + 3 for i in range(n)]
    vs, fs = make_objects(counts, 41)
    boxes = make_boxes(n, 42)
    a = S.assemble_scene(to_meshes(vs, fs), torch.from_numpy(boxes), [2] * n, CLASSES)
    b = S.assemble_scene(to_meshes(vs, fs), torch.from_numpy(boxes), [2] * n, CLASSES)
    for x, y in ((a.verts, b.verts), (a.faces, b.faces), (a.face_object, b.face_object), (a.box_points, b.box_points)):
        assert torch.equal(x, y)
    k = 19
    pts, v = S.fit_shapes_to_box_v2(torch.from_numpy(vs[k]), torch.from_numpy(fs[k]), torch.from_numpy(boxes[k]), degrees=True)
    assert torch.equal(v, a.per_object()[k].vertices) and torch.equal(pts, a.box_points[k])


def test_zero_extent_axis_gives_finite_output():
    from commonscenes_amd import scene_mesh as S
    vs, fs = make_objects([50, 1], 51)
    vs[0][:, 1] = 0.25                            # a flat object: zero extent along y
    boxes = make_boxes(2, 52)
    scene = S.assemble_scene(to_meshes(vs, fs), torch.from_numpy(boxes), [2, 2], CLASSES)
    assert torch.isfinite(scene.verts).all()
    check_scene(scene, vs, fs, boxes, [0, 1], True)
    got = scene.verts.cpu().numpy()
    assert (got[:50, 1] == boxes[0][4]).all() and (got[50] == boxes[1][3:6]).all()


def test_sentinel_past_the_outputs_survives():
    from commonscenes_amd import lib as L
    from commonscenes_amd.ops import _stream
    dll = L.load()
    counts = [65, 0, 300]
    vs, fs = make_objects(counts, 61)
    V, F, n, pad = sum(counts), sum(f.shape[0] for f in fs), 3, 7
    verts = torch.from_numpy(np.concatenate(vs)).cuda()
    faces = torch.from_numpy(np.concatenate(fs)).cuda()
    fc = [f.shape[0] for f in fs]
    i64 = lambda a: torch.tensor(a, dtype=torch.int64).cuda()
    vb, vc, fb, fcn = i64([0, 65, 65]), i64(counts), i64([0, fc[0], fc[0]]), i64(fc)
    boxes = torch.from_numpy(make_boxes(n, 62)).cuda()
    xform = torch.full((n + pad, 12), -7.0, device="cuda")
    pts = torch.full((n + pad, 8, 3), -7.0, device="cuda")
    L.check(dll.cs_scene_fit_boxes(verts.data_ptr(), V, vb.data_ptr(), vc.data_ptr(), boxes.data_ptr(), n, 1,
                                   xform.data_ptr(), pts.data_ptr(), _stream()), "fit")
    assert (xform[n:] == -7).all() and (pts[n:] == -7).all() and (xform[:n] != -7).any(dim=1).all()
    assert xform[1].tolist() == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]          # no vertices: identity
    ov = torch.full((V + pad, 3), -7.0, device="cuda")
    oc = torch.full((V + pad, 3), -7.0, device="cuda")
    of = torch.full((F + pad, 3), -7, dtype=torch.int64, device="cuda")
    oo = torch.full((F + pad,), -7, dtype=torch.int32, device="cuda")
    keep = torch.ones(n, dtype=torch.bool, device="cuda")
    col = torch.rand(n, 3, device="cuda")
    args = lambda nv, nf: (verts.data_ptr(), V, faces.data_ptr(), F, vb.data_ptr(), vc.data_ptr(), fb.data_ptr(),
                           fcn.data_ptr(), xform.data_ptr(), keep.data_ptr(), vb.data_ptr(), fb.data_ptr(), col.data_ptr(), n,
                           0, ov.data_ptr(), oc.data_ptr(), nv, of.data_ptr(), oo.data_ptr(), nf, _stream())
    L.check(dll.cs_scene_apply(*args(V, F)), "apply")
    torch.cuda.synchronize()
    assert (ov[V:] == -7).all() and (oc[V:] == -7).all() and (of[F:] == -7).all() and (oo[F:] == -7).all()
    assert (oo[:F] >= 0).all() and (of[:F] >= 0).all() and (oc[:V] >= 0).all()
    # an output declared too small for the last object: that object is left out whole, nothing past the end is written
    ov.fill_(-7.0); of.fill_(-7); oo.fill_(-7)
    L.check(dll.cs_scene_apply(*args(V - 1, F - 1)), "apply")
    torch.cuda.synchronize()
    assert (ov[65:] == -7).all() and (of[fc[0]:] == -7).all() and (oo[:fc[0]] == 0).all()


def sphere_sdf(n, radius, centre=(0.0, 0.0, 0.0)):
    g = (torch.arange(n, dtype=torch.float32) + 0.5) / n - 0.5
    x, y, z = torch.meshgrid(g, g, g, indexing="ij")
    return torch.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius


def test_end_to_end_sphere_sdf_to_scene():
    from commonscenes_amd import scene_mesh as S
    from commonscenes_amd.mesh import sdf_to_mesh
    sdf = sphere_sdf(16, 0.3)[None, None].cuda()
    box = torch.tensor([[1.0, 2.0, 0.5, 1.5, 0.0, -2.0, 30.0]])
    scene = S.assemble_scene(sdf, box, [2], CLASSES)                       # the SDF batch itself
    m = sdf_to_mesh(sdf, render_all=True)
    vs, fs = [m.verts_list()[0].cpu().numpy()], [m.faces_list()[0].cpu().numpy()]
    assert vs[0].shape[0] > 100
    check_scene(scene, vs, fs, box.numpy(), [0], True)
    via = S.assemble_scene(m, box, [2], CLASSES)                           # marching_cubes' views, used in place
    assert torch.equal(via.verts, scene.verts) and torch.equal(via.faces, scene.faces)
    # outward normals after the flip: the signed volume is positive
    v, f = scene.verts.double().cpu(), scene.faces.cpu()
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    ctr = v.mean(dim=0)
    vol = ((a - ctr) * torch.cross(b - ctr, c - ctr, dim=1)).sum() / 6
    assert vol > 0.1 * (1.0 * 2.0 * 0.5)


# ---------------------------------------------------------------- integer-math oracle of the rasteriser
def oracle_raster(verts, faces, size, znear=0.05):
    """-> depth [size,size] fp64 (inf where empty), winner face (-1), second nearest depth (inf), dropped.  Integer
    coverage (1/256 pixel snap, int64 edge functions, top-left rule), fp64 perspective-correct depth, ties to the lower id."""
    v = verts.astype(np.float64)
    d = 8.0 - v[:, 1]
    X = np.floor((1 + v[:, 0] / np.where(d > 0, d, 1)) / 2 * size * 256 + 0.5).astype(np.int64)
    Y = np.floor((1 + v[:, 2] / np.where(d > 0, d, 1)) / 2 * size * 256 + 0.5).astype(np.int64)
    best = np.full((size, size), np.inf)
    second = np.full((size, size), np.inf)
    win = np.full((size, size), -1, dtype=np.int64)
    dropped = 0
    py, px = np.meshgrid(np.arange(size, dtype=np.int64), np.arange(size, dtype=np.int64), indexing="ij")
    cx, cy = px * 256 + 128, py * 256 + 128
    edge = lambda ax, ay, bx, by, qx, qy: (bx - ax) * (qy - ay) - (by - ay) * (qx - ax)
    for fid, (i0, i1, i2) in enumerate(faces):
        if min(d[i0], d[i1], d[i2]) < znear:
            dropped += 1
            continue
        area = edge(X[i0], Y[i0], X[i1], Y[i1], X[i2], Y[i2])
        if area == 0:
            continue
        if area < 0:
            i1, i2, area = i2, i1, -area
        idx = (i0, i1, i2)
        inside = np.ones((size, size), dtype=bool)
        es = []
        for a, b in ((1, 2), (2, 0), (0, 1)):
            ax, ay, bx, by = X[idx[a]], Y[idx[a]], X[idx[b]], Y[idx[b]]
            e = edge(ax, ay, bx, by, cx, cy)
            dx, dy = bx - ax, by - ay
            tl = (dy == 0 and dx > 0) or dy < 0
            inside &= (e > 0) | ((e == 0) & tl)
            es.append(e.astype(np.float64))
        with np.errstate(divide="ignore", invalid="ignore"):
            dep = 1.0 / sum(es[k] / float(area) / d[idx[k]] for k in range(3))
        dep = np.where(inside, dep, np.inf)
        closer = dep < best                                    # strict: equal depths stay with the lower face id
        second = np.where(closer, best, np.minimum(second, dep))
        win = np.where(closer, fid, win)
        best = np.where(closer, dep, best)
    return best, win, second, dropped


def make_scene(verts, faces, face_object):
    from commonscenes_amd.scene_mesh import SceneMesh
    # (contiguous copies: a reversed view such as F[::-1] has a negative stride, which torch.from_numpy refuses)
    v = torch.from_numpy(np.ascontiguousarray(verts, dtype=np.float32)).cuda()
    f = torch.from_numpy(np.ascontiguousarray(faces, dtype=np.int64)).cuda()
    o = torch.from_numpy(np.ascontiguousarray(face_object, dtype=np.int32)).cuda()
    return SceneMesh(v, f, torch.full_like(v, 0.5), o, None, [])


def render(verts, faces, face_object, size=64):
    from commonscenes_amd.scene_mesh import render_topdown
    out = render_topdown(make_scene(verts, faces, face_object), size)
    return out["depth"].cpu().numpy(), out["object_id"].cpu().numpy(), out["rgb"].cpu().numpy(), out["dropped"]


def quad(x0, x1, z0, z1, y, base):
    return [[x0, y, z0], [x0, y, z1], [x1, y, z1], [x1, y, z0]], [[base, base + 1, base + 2], [base, base + 2, base + 3]]


def layers():
    """three flat layers at heights 0, 4, 6 (depths 8, 4, 2), x / z multiples of 2^-6, some corners on pixel centres"""
    V, F, O = [], [], []
    for k, (x0, x1, z0, z1, y) in enumerate([(-6.375, 5.25, -7.0, 6.625, 0.0), (-2.140625, 1.5, -1.0, 2.515625, 4.0),
                                            (-0.546875, 0.96875, -0.75, 0.265625, 6.0)]):
        v, f = quad(x0, x1, z0, z1, y, len(V))
        V += v
        F += f
        O += [k, k]
    V += [[-3.0, 4.0, -3.5], [-1.0, 4.0, -3.25], [-2.5, 4.0, -1.015625]]     # a lone triangle, wound to face down
    F += [[12, 13, 14]]
    O += [3]
    return np.asarray(V, dtype=np.float32), np.asarray(F, dtype=np.int64), np.asarray(O, dtype=np.int32)


def test_flat_layers_match_the_oracle_at_every_pixel():
    V, F, O = layers()
    depth, oid, rgb, dropped = render(V, F, O)
    best, win, _, odrop = oracle_raster(V, F, 64)
    want = np.where(win >= 0, O[np.maximum(win, 0)], -1)
    assert dropped == odrop == 0
    assert np.array_equal(oid, want)
    assert set(np.unique(oid)) == {-1, 0, 1, 2, 3}
    hit = win >= 0
    assert np.isinf(depth[~hit]).all() and (np.abs(depth[hit] - best[hit]) <= 4 * EPS * best[hit]).all()
    assert (rgb[~hit] == 255).all()
    up = oid != 3                                   # facing the camera: 0.5 * (0.3 + 0.7) * 255 = 127.5 -> 128
    assert (rgb[hit & up] == 128).all() and (rgb[oid == 3] == round(0.5 * 0.3 * 255)).all()     # turned away: ambient


def test_shared_edge_covers_every_pixel_exactly_once():
    # depth 4: pixel = 32 + 8 x; the corners sit on pixel centres (8.5, 50.5), so the shared diagonal runs through centres
    V, F = quad(-2.9375, 2.3125, -2.9375, 2.3125, 4.0, 0)
    V, F = np.asarray(V, dtype=np.float32), np.asarray(F)
    both = render(V, F, [0, 1])[1]
    first, second = render(V, F[:1], [0])[1], render(V, F[1:], [1])[1]
    covered = (first >= 0).astype(int) + (second >= 0).astype(int)
    _, win, _, _ = oracle_raster(V, F, 64)
    assert np.array_equal(both >= 0, win >= 0) and (covered[both >= 0] == 1).all() and (covered[both < 0] == 0).all()
    assert np.array_equal(both, win)
    assert (both >= 0).sum() > 300


def test_off_screen_half_off_screen_and_zero_area():
    base_v, base_f = quad(-1.0, 1.0, -1.0, 1.0, 0.0, 0)
    V = np.asarray(base_v + [[20.0, 0, 20.0], [24.0, 0, 20.5], [21.0, 0, 25.0],          # wholly off-screen
                             [-12.0, 4.0, -1.0], [-3.0, 4.0, 0.5], [-12.0, 4.0, 2.0],      # half off-screen (left)
                             [1.0, 6.0, 1.0], [1.5, 6.0, 1.5], [2.0, 6.0, 2.0],            # zero area (collinear)
                             [0.5, 6.0, -0.5]], dtype=np.float32)
    F = np.asarray(base_f + [[4, 5, 6], [7, 8, 9], [10, 11, 12], [13, 13, 10]])
    O = [0, 0, 1, 2, 3, 3]
    depth, oid, _, dropped = render(V, F, O)
    best, win, _, _ = oracle_raster(V, F, 64)
    assert dropped == 0
    assert np.array_equal(oid, np.where(win >= 0, np.asarray(O)[np.maximum(win, 0)], -1))
    assert set(np.unique(oid)) == {-1, 0, 2} and (oid[:, 0] == 2).any()
    assert (np.abs(depth[win >= 0] - best[win >= 0]) <= 4 * EPS * best[win >= 0]).all()


def test_triangle_behind_znear_is_dropped_whole():
    V, F, O = layers()
    ref = render(V, F, O)
    V2 = np.concatenate([V, np.asarray([[-1.0, 7.96875, -1.0], [1.0, 4.0, -1.0], [0.0, 4.0, 1.0]], dtype=np.float32)])
    F2 = np.concatenate([F, [[15, 16, 17]]])
    got = render(V2, F2, np.concatenate([O, [9]]))
    assert got[3] == 1 and ref[3] == 0
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])


def test_coplanar_overlap_goes_to_the_lower_face_id_and_face_order_does_not_matter():
    V = np.asarray([[-4.0, 4.0, -4.0], [3.5, 4.0, -3.0], [-1.0, 4.0, 3.515625],
                    [-3.0, 4.0, 3.0], [3.0, 4.0, 2.5], [0.5, 4.0, -3.765625]], dtype=np.float32)
    F = np.asarray([[0, 1, 2], [3, 4, 5]])
    d01, o01 = render(V, F, [0, 1])[:2]
    d10, o10 = render(V, F[::-1], [1, 0])[:2]
    only0, only1 = render(V, F[:1], [0])[1] >= 0, render(V, F[1:], [1])[1] >= 0
    overlap = only0 & only1
    assert overlap.sum() > 100
    assert (o01[overlap] == 0).all() and (o10[overlap] == 1).all()          # face id 0 wins either way
    assert np.array_equal(d01, d10) and np.array_equal(o01[~overlap], o10[~overlap])
    # a permutation of a scene without ties: depth bit-equal, ids equal
    V3, F3, O3 = layers()
    perm = np.random.default_rng(7).permutation(len(F3))
    a, b = render(V3, F3, O3), render(V3, F3[perm], O3[perm])
    best, win, second, _ = oracle_raster(V3, F3, 64)
    differ = ~((win >= 0) & (best == second))
    assert differ.all()                              # (this scene has no tie at all)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1][differ], b[1][differ])


def sloped():
    """three sloped triangles stacked over a floor quad, heights in {0, 4, 6}; the upper ones stay strictly above the lower
    ones wherever they overlap, so the oracle has no pixel whose two nearest depths are within the tolerance"""
    fv, ff = quad(-7.0, 7.0, -7.0, 7.0, 0.0, 0)
    V = fv + [[-5.0, 0.0, -4.0], [4.0, 4.0, -3.5], [-1.0, 4.0, 5.015625],
              [-2.0, 4.0, -2.0], [1.5, 6.0, -1.0], [-0.5, 6.0, 1.515625],
              [2.0, 0.0, 1.0], [6.0, 4.0, 2.0], [3.0, 6.0, 5.25]]
    F = ff + [[4, 5, 6], [7, 8, 9], [12, 11, 10]]
    return np.asarray(V, dtype=np.float32), np.asarray(F), np.asarray([0, 0, 1, 2, 3])


def test_sloped_triangles_depth_and_ids():
    V, F, O = sloped()
    tol = 8 * EPS
    best, win, second, _ = oracle_raster(V, F, 64)
    hit = win >= 0
    close = hit & np.isfinite(second) & (second - best <= tol * second)
    assert close.sum() == 0                          # chosen so: the oracle alone has no ambiguous pixel
    depth, oid, _, dropped = render(V, F, O)
    assert dropped == 0 and np.array_equal(oid >= 0, hit)
    assert (np.abs(depth[hit] - best[hit]) <= tol * best[hit]).all()
    want = np.where(hit, O[np.maximum(win, 0)], -1)
    bad = oid != want
    assert not (bad & ~close).any() and bad.sum() <= 0.01 * hit.sum()
    assert set(np.unique(oid)) == {0, 1, 2, 3} | ({-1} if (~hit).any() else set())
    assert len(np.unique(depth[oid == 1])) > 50      # really sloped


@pytest.fixture(scope="module")
def seven_object_scene():
    from commonscenes_amd import scene_mesh as S
    sdf = torch.stack([sphere_sdf(16, 0.2 + 0.03 * i)[None] for i in range(7)]).cuda()
    cats = [2, 4, 0, 3, 2, 1, 4, 2, 3]                                      # 7 shaped + _scene_ + floor
    rng = np.random.default_rng(9)
    boxes = np.zeros((9, 7), dtype=np.float32)
    boxes[:, :3] = rng.uniform(0.8, 2.0, (9, 3))
    grid = [(-3, -3), (0, -3), (9, 9), (3, -3), (-3, 0), (9, 9), (3, 0), (-2, 3), (2, 3)]
    boxes[:, 3], boxes[:, 5] = [g[0] for g in grid], [g[1] for g in grid]
    boxes[:, 6] = [0, 15, 0, 30, 45, 0, 60, 75, 90]
    boxes[2] = [0.1, 0.1, 0.1, 0, 0, 0, 0]                                  # _scene_
    boxes[5] = [9.0, 0.01, 9.0, 0, 0, 0, 0]                                 # the floor node
    return S.assemble_scene(sdf, torch.from_numpy(boxes), cats, CLASSES, floor=True), boxes, cats


def test_seven_object_scene_with_floor_at_256(seven_object_scene, tmp_path):
    from commonscenes_amd import scene_mesh as S
    scene, boxes, cats = seven_object_scene
    assert scene.kept == [0, 1, 3, 4, 6, 7, 8, 9]
    want = S.create_floor(torch.from_numpy(boxes), cats, CLASSES).vertices
    assert torch.equal(scene.verts[-4:].cpu(), want)                        # the device floor = the host restatement
    out = S.render_topdown(scene, 256)
    oid = out["object_id"].cpu().numpy()
    assert out["dropped"] == 0
    assert set(np.unique(oid)) == {-1, 0, 1, 3, 4, 6, 7, 8, 9}
    assert (oid == 9).sum() > 0.1 * 256 * 256                                # the floor is visible
    depth = out["depth"].cpu().numpy()
    obj = (oid >= 0) & (oid < 9)
    assert (depth[oid == 9] == 8.0).all() and (depth[obj] <= 8.0).all() and (depth[obj] < 8.0).mean() > 0.99
    again = S.render_topdown(scene, 256)
    assert torch.equal(again["depth"], out["depth"]) and torch.equal(again["object_id"], out["object_id"])
    assert torch.equal(again["rgb"], out["rgb"])
    scene.export_obj(tmp_path / "scene.obj")
    txt = (tmp_path / "scene.obj").read_text().split("\n")
    assert sum(l.startswith("v ") for l in txt) == scene.verts.shape[0]
    assert sum(l.startswith("f ") for l in txt) == scene.faces.shape[0]
