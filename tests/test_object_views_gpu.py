"""Per-object views on the device (csrc/cs_view.hip behind commonscenes_amd/object_views.py), stage by stage against the
fp64 / integer restatement of tests/_object_view_ref.py, and against known answers that do not lean on it.  pytorch3d is not
in the image: what is pinned here is the documented convention, not its output."""
import numpy as np
import pytest
import torch

import _object_view_ref as REF

pytestmark = pytest.mark.gpu
CAM = (1.7, 20, 20)


def renderer(size, cam=CAM):
    from commonscenes_amd.object_views import init_mesh_renderer
    return init_mesh_renderer(image_size=size, dist=cam[0], elev=cam[1], azim=cam[2], device="cuda")


def front_renderer(size):
    """camera on the +z axis at distance 2: R = diag(-1, 1, -1) exactly, so z_view = 2 - z_world with no rounding"""
    from commonscenes_amd.object_views import MeshRenderer
    return MeshRenderer(size, np.diag([-1.0, 1.0, -1.0]), np.array([0.0, 0.0, 2.0]), "cuda")


def meshes_of(verts_list, faces_list, rgb_list=None):
    from commonscenes_amd.mesh import Meshes, Textures
    v = [torch.as_tensor(np.asarray(x, dtype=np.float32).reshape(-1, 3)).cuda() for x in verts_list]
    f = [torch.as_tensor(np.asarray(x, dtype=np.int64).reshape(-1, 3)).cuda() for x in faces_list]
    tx = None if rgb_list is None else Textures([torch.as_tensor(np.asarray(x, dtype=np.float32).reshape(-1, 3)).cuda()
                                                 for x in rgb_list])
    return Meshes(v, f, tx)


def pack(m):
    from commonscenes_amd.object_views import _Packed
    return _Packed(m, torch.device("cuda", torch.cuda.current_device()))


def unit_ball(n, seed):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (d * rng.uniform(0, 1, (n, 1)) ** (1 / 3)).astype(np.float32)


def at(r, col, row, z):
    """world point that lands at continuous pixel (col, row) at view depth z for renderer r"""
    s = r.image_size
    view = np.array([(1 - 2 * col / s) * z / REF.FOCAL, (1 - 2 * row / s) * z / REF.FOCAL, z])
    return (view - r.T) @ r.R.T


def sphere_mesh(n, radius=0.3):
    """marching-cubes sphere of the n^3 grid: verts [V,3], faces [F,3] numpy"""
    from commonscenes_amd.mesh import sdf_to_mesh
    g = (torch.arange(n, dtype=torch.float32) + 0.5) / n - 0.5
    x, y, z = torch.meshgrid(g, g, g, indexing="ij")
    m = sdf_to_mesh((torch.sqrt(x * x + y * y + z * z) - radius)[None, None].cuda(), render_all=True)
    return m.verts_list()[0].cpu().numpy(), m.faces_list()[0].cpu().numpy()


# ------------------------------------------------------------------------------------------------------------ projection
@pytest.mark.parametrize("n,size", [(1, 16), (63, 17), (64, 32), (65, 64), (1000, 64)])
def test_projection_against_fp64(n, size):
    v = unit_ball(n, n)
    r = renderer(size)
    out = r.project(pack(meshes_of([v], [np.zeros((0, 3))])))
    sub, z = REF.project(v, r.R, r.T, size)
    scr = out["screen"].cpu().numpy().astype(np.int64)
    assert np.abs(scr - np.floor(sub + 0.5)).max() <= 1                      # 1/256-pixel units
    assert np.abs(out["zview"].cpu().numpy() / z - 1).max() <= 1e-6
    assert torch.equal(out["world"].cpu(), torch.from_numpy(v))               # no normalisation: the vertices as given


def test_projection_with_normalisation_pins_common_centre_and_per_mesh_scale():
    from commonscenes_amd.object_views import normalize_meshes
    a = unit_ball(200, 1) * 0.2 + np.array([2.0, -1.0, 0.5], dtype=np.float32)     # small, far off
    b = unit_ball(77, 2) * 3.0 + np.array([-1.0, 0.5, 0.0], dtype=np.float32)      # large
    m = meshes_of([a, b], [np.zeros((0, 3))] * 2)
    r = renderer(32)
    out = r.project(pack(m), normalize=True)
    want, centre = REF.normalize([a, b])
    world = out["world"].cpu().numpy()
    assert np.abs(out["centre"].cpu().numpy() - centre).max() <= 1e-6 * np.abs(centre).max()
    # fp32: v - centre carries ~2.4e-7 (|v| ~ 2) and the small mesh divides it by r = 0.2; r itself carries as much again
    assert np.abs(world - np.concatenate(want)).max() <= 5e-6
    # the quirk: ONE centre (the mean of all 277 vertices, so neither mesh is centred on its own) and one scale per mesh
    for lo, hi in ((0, 200), (200, 277)):
        assert abs(np.linalg.norm(world[lo:hi], axis=1).max() - 1.0) <= 1e-6
        assert np.linalg.norm(world[lo:hi].mean(axis=0)) > 0.1
    sub, z = REF.project(np.concatenate(want), r.R, r.T, 32)
    # (fp32 normalisation: 5e-6 of a unit-size vertex is 5e-6 * 32 * 256 * FOCAL / z < 0.1 grid units on top of the snap)
    assert np.abs(out["screen"].cpu().numpy() - np.floor(sub + 0.5)).max() <= 1
    assert np.abs(out["zview"].cpu().numpy() / z - 1).max() <= 3e-6
    alone = normalize_meshes(m)                                              # the stage on its own: the same numbers
    assert torch.equal(torch.cat(alone.verts_list()), out["world"])


# -------------------------------------------------------------------------------------------------------- vertex normals
def _tetra():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32) * 0.7 - 0.2
    return v, np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])


def _fan(k=65):
    ang = np.linspace(0, 2 * np.pi, k + 1)
    rim = np.stack([np.cos(ang), 0.3 * np.sin(3 * ang), np.sin(ang)], axis=1) * 0.8
    v = np.concatenate([[[0.0, 0.25, 0.0]], rim]).astype(np.float32)
    return v, np.array([[0, i + 1, i + 2] for i in range(k)])


@pytest.mark.parametrize("case", ["tetra", "fan65", "sphere16"])
def test_vertex_normals_against_fp64_and_bit_reproducible(case):
    from commonscenes_amd.object_views import vertex_normals
    v, f = {"tetra": _tetra, "fan65": _fan, "sphere16": lambda: sphere_mesh(16)}[case]()
    got = vertex_normals(pack(meshes_of([v], [f])))
    want = REF.vertex_normals(v, f)
    err = np.abs(got.cpu().numpy() - want).max()
    print(f"vertex normals {case}: {len(v)} vertices, {len(f)} faces, max |err| {err:.2e}")
    assert err <= 1e-6
    assert torch.equal(vertex_normals(pack(meshes_of([v], [f]))), got)                       # two runs
    perm = np.random.default_rng(5).permutation(len(f))
    assert torch.equal(vertex_normals(pack(meshes_of([v], [f[perm]]))), got)                 # any face order
    assert torch.equal(vertex_normals(pack(meshes_of([v], [f[::-1].copy()]))), got)


# ---------------------------------------------------------------------------------------------------- coverage and depth
def check_against_oracle(r, verts_list, faces_list, zero_near_ties=False):
    """render the batch; the oracle gets the GPU's own snapped coordinates and fp32 depths; pix_to_face and zbuf must be
    equal at every pixel.  -> (out, per-mesh (win, best, second))"""
    out = r.render_all(meshes_of(verts_list, faces_list))
    pk, s = out["pk"], r.image_size
    scr, zv = out["screen"].cpu().numpy(), out["zview"].cpu().numpy()
    faces = pk.faces.cpu().numpy()
    vb, fb = np.concatenate([[0], np.cumsum(pk.nv)]), np.concatenate([[0], np.cumsum(pk.nf)])
    res, drops = [], []
    for b in range(pk.n):
        best, win, second, dropped = REF.oracle_raster(scr, zv, faces[fb[b]:fb[b + 1]], s, nverts_range=(vb[b], vb[b + 1]))
        if zero_near_ties:
            hit = np.isfinite(second)
            assert int((second[hit] - best[hit] <= 1e-6 * best[hit]).sum()) == 0
        p2f = out["pix_to_face"][b].cpu().numpy()
        assert np.array_equal(p2f, np.where(win >= 0, win + fb[b], -1)), f"mesh {b}: pix_to_face"
        assert np.array_equal(out["zbuf"][b].cpu().numpy(), np.where(win >= 0, best, np.float32(-1.0))), f"mesh {b}: zbuf"
        res.append((win, best, second))
        drops.append(dropped)
    assert out["dropped"].tolist() == drops
    return out, res


def test_one_triangle():
    for size in (16, 17, 32, 64):
        r = renderer(size)
        q = size / 16.0
        v = [at(r, 3.3 * q, 2.1 * q, 1.5), at(r, 12.7 * q, 4.2 * q, 1.7), at(r, 6.5 * q, 13.9 * q, 2.0)]
        out, res = check_against_oracle(r, [v], [[[0, 1, 2]]])
        assert (res[0][0] >= 0).sum() > 20 * q * q
        out2, res2 = check_against_oracle(r, [v], [[[0, 2, 1]]])                     # both windings are drawn
        assert np.array_equal(res2[0][0], res[0][0])
        assert torch.equal(out2["zbuf"], out["zbuf"])


def test_two_triangles_sharing_an_edge_cover_every_pixel_once():
    r = renderer(32)
    v = [at(r, 4.2, 5.1, 1.6), at(r, 27.3, 3.4, 1.7), at(r, 25.8, 28.6, 1.9), at(r, 2.9, 24.7, 1.8)]
    f = [[0, 1, 2], [0, 2, 3]]
    out, res = check_against_oracle(r, [v], [f])
    # each triangle alone, as its own mesh of one batch: the two masks are disjoint and their union is the quad's
    solo, _ = check_against_oracle(r, [v, v], [[f[0]], [f[1]]])
    m0, m1 = (solo["pix_to_face"][k].cpu().numpy() >= 0 for k in (0, 1))
    both = out["pix_to_face"][0].cpu().numpy()
    assert not (m0 & m1).any() and np.array_equal(m0 | m1, both >= 0)
    assert np.array_equal(both == 0, m0) and np.array_equal(both == 1, m1)
    # an axis-aligned quad on pixel-centre lines: the top-left rule decides the boundary, still exactly once
    v = [at(r, 4.5, 6.5, 1.7), at(r, 20.5, 6.5, 1.7), at(r, 20.5, 18.5, 1.7), at(r, 4.5, 18.5, 1.7)]
    out, _ = check_against_oracle(r, [v], [f])
    solo, _ = check_against_oracle(r, [v, v], [[f[0]], [f[1]]])
    m0, m1 = (solo["pix_to_face"][k].cpu().numpy() >= 0 for k in (0, 1))
    assert not (m0 & m1).any() and np.array_equal(m0 | m1, out["pix_to_face"][0].cpu().numpy() >= 0)


def test_coplanar_overlap_goes_to_the_lower_face_id_whatever_the_order():
    r = front_renderer(32)
    z = 0.25                                                   # world z: every vertex at view depth 1.75 exactly
    a = [[-0.6, -0.5, z], [0.5, -0.4, z], [-0.1, 0.6, z]]
    b = [[-0.3, -0.6, z], [0.7, 0.1, z], [-0.2, 0.5, z]]
    v = a + b
    out, res = check_against_oracle(r, [v], [[[0, 1, 2], [3, 4, 5]]])
    outr, resr = check_against_oracle(r, [v], [[[3, 4, 5], [0, 1, 2]]])
    zb = out["zbuf"][0].cpu().numpy()
    assert set(np.unique(zb).tolist()) == {-1.0, 1.75}
    ma = check_against_oracle(r, [a], [[[0, 1, 2]]])[1][0][0] >= 0
    mb = check_against_oracle(r, [b], [[[0, 1, 2]]])[1][0][0] >= 0
    assert (ma & mb).sum() > 50
    assert (res[0][0][ma & mb] == 0).all() and (resr[0][0][ma & mb] == 0).all()      # face 0 wins: a first, then b first
    assert torch.equal(out["zbuf"], outr["zbuf"])


def test_sloped_interpenetrating_triangles():
    r = renderer(64)
    a = [at(r, 5.3, 8.2, 1.3), at(r, 58.1, 11.7, 2.1), at(r, 30.4, 57.9, 1.7)]
    b = [at(r, 7.9, 50.3, 2.0), at(r, 55.2, 52.8, 1.35), at(r, 33.6, 6.1, 1.75)]
    out, res = check_against_oracle(r, [a + b], [[[0, 1, 2], [3, 4, 5]]], zero_near_ties=True)
    win = res[0][0]
    assert (win == 0).sum() > 200 and (win == 1).sum() > 200                        # each is in front somewhere
    assert np.isfinite(res[0][2]).sum() > 200                                       # and they do overlap
    outr, _ = check_against_oracle(r, [a + b], [[[3, 4, 5], [0, 1, 2]]], zero_near_ties=True)
    assert torch.equal(out["zbuf"], outr["zbuf"])


def test_large_triangle_next_to_129_small_ones():
    """both paths of the rasteriser (own-lane walk up to 8 pixel centres, whole-wave walk above) and the wave edges: 130
    faces = two full waves and two lanes; the large triangle sits at a wave boundary in one order and mid-wave in another"""
    r = renderer(64)
    v, f = [], []
    rng = np.random.default_rng(11)
    for k in range(129):
        c, rw = 4 + (k % 13) * 4.5 + rng.uniform(-0.4, 0.4), 4 + (k // 13) * 5.7 + rng.uniform(-0.4, 0.4)
        zz = 1.4 + 0.002 * k
        v += [at(r, c, rw, zz), at(r, c + 2.3, rw + 0.3, zz + 0.01), at(r, c + 0.4, rw + 2.5, zz + 0.02)]
        f.append([3 * k, 3 * k + 1, 3 * k + 2])
    v += [at(r, 2.2, 3.1, 2.0), at(r, 61.7, 6.3, 2.2), at(r, 28.4, 62.5, 1.9)]
    big = [387, 388, 389]
    for pos in (0, 64, 100, 129):
        ff = f[:pos] + [big] + f[pos:]
        out, res = check_against_oracle(r, [v], [ff])
        win = res[0][0]
        assert (win == pos).sum() > 800 and len(np.unique(win)) > 100


def test_offscreen_zero_area_and_malformed_faces():
    r = renderer(17)
    v = [at(r, -30, -20, 1.7), at(r, -10, -25, 1.7), at(r, -20, -5, 1.7),          # all outside
         at(r, -6.3, 4.2, 1.6), at(r, 9.1, 2.7, 1.8), at(r, 3.3, 22.4, 1.7),        # half outside (left and bottom)
         at(r, 10.2, 8.8, 1.7), at(r, 14.1, 12.3, 1.7)]
    f = [[0, 1, 2], [3, 4, 5], [6, 6, 7], [6, 7, 7], [3, 4, 8], [-1, 4, 5], [4, 5, 2 ** 40]]
    out, res = check_against_oracle(r, [v], [f])
    assert set(np.unique(res[0][0]).tolist()) == {-1, 1}                            # only the half-visible one draws
    # in a batch a malformed id may point into ANOTHER mesh's vertices: still nothing is drawn for it
    tri = [at(r, 3.3, 2.1, 1.5), at(r, 12.7, 4.2, 1.7), at(r, 6.5, 13.9, 2.0)]
    out, res = check_against_oracle(r, [tri, tri], [[[0, 1, 3]], [[0, 1, 2], [0, 1, -2]]])
    assert (res[0][0] == -1).all() and (res[1][0] == 0).sum() > 20 and not (res[1][0] == 1).any()
    img = out["image"].cpu().numpy()
    assert np.array_equal(img[0], np.broadcast_to(np.array([1, 1, 1, 0], dtype=np.float32), img[0].shape))


def test_near_plane_drop_is_per_mesh():
    r = renderer(32)
    tri = [at(r, 6.6, 4.2, 1.5), at(r, 25.4, 8.4, 1.7), at(r, 13.0, 27.8, 2.0)]
    near = [at(r, 6.6, 4.2, 1.5), at(r, 25.4, 8.4, 0.4), at(r, 13.0, 27.8, 2.0)]      # one vertex at z_view = 0.4 < 0.5
    out, res = check_against_oracle(r, [tri, near], [[[0, 1, 2]], [[0, 1, 2]]])
    assert abs(float(out["zview"][4]) - 0.4) < 1e-5
    assert out["dropped"].tolist() == [0, 1]
    alone = r.render_all(meshes_of([tri], [[[0, 1, 2]]]))
    assert torch.equal(out["image"][0], alone["image"][0]) and torch.equal(out["zbuf"][0], alone["zbuf"][0])
    assert (out["pix_to_face"][1] == -1).all() and (out["image"][1, ..., 3] == 0).all()
    frag = r.rasterize(meshes_of([tri, near], [[[0, 1, 2]], [[0, 1, 2]]]))
    assert frag.dropped.tolist() == [0, 1] and torch.equal(frag.pix_to_face, out["pix_to_face"])
    assert frag.bary_coords.shape == (2, 32, 32, 3) and frag.zbuf.shape == (2, 32, 32)


# --------------------------------------------------------------------------------------------------------- batch isolation
def _ragged_batch():
    fv, ff = _fan(65)
    tv, tf = _tetra()
    one = np.array([[-0.5, -0.3, 0.1], [0.6, -0.2, 0.0], [0.0, 0.5, -0.1]], dtype=np.float32)
    point = np.tile(np.array([[0.2, 0.1, -0.3]], dtype=np.float32), (4, 1))
    empty = np.array([[0.1, 0.2, 0.3], [0.3, 0.2, 0.1], [0.0, 0.0, 0.1]], dtype=np.float32)
    verts = [fv * 0.6, empty, point, one, tv]
    faces = [ff, np.zeros((0, 3), dtype=np.int64), np.array([[0, 1, 2], [1, 2, 3], [0, 2, 3]]), np.array([[0, 1, 2]]), tf]
    rng = np.random.default_rng(3)
    rgb = [rng.uniform(0, 1, v.shape).astype(np.float32) for v in verts]
    return verts, faces, rgb


@pytest.mark.parametrize("size", [16, 17, 32, 64])
def test_batch_isolation_each_mesh_as_if_alone(size):
    verts, faces, rgb = _ragged_batch()
    r = renderer(size)
    out = r.render_all(meshes_of(verts, faces, rgb))
    assert out["image"].shape == (5, size, size, 4) and out["dropped"].tolist() == [0] * 5
    fb = np.concatenate([[0], np.cumsum([len(f) for f in faces])])
    for b in range(5):
        alone = r.render_all(meshes_of([verts[b]], [faces[b]], [rgb[b]]))
        p2f = out["pix_to_face"][b]
        assert torch.equal(torch.where(p2f >= 0, p2f - int(fb[b]), p2f), alone["pix_to_face"][0]), b
        for k in ("image", "zbuf", "bary"):
            assert torch.equal(out[k][b], alone[k][0]), (b, k)
    for b in (1, 2):                                            # no faces / all vertices equal: pure background, finite
        img = out["image"][b].cpu().numpy()
        assert np.isfinite(img).all() and (img[..., :3] == 1).all() and (img[..., 3] == 0).all()
    assert (out["pix_to_face"][0] >= 0).sum() > 0 and (out["pix_to_face"][4] >= 0).sum() > 0


def test_batch_with_normalisation_against_fp64():
    verts, faces, rgb = _ragged_batch()
    verts = [v + np.float32(0.1 * k) for k, v in enumerate(verts)]      # the common centre couples the meshes
    r = renderer(32)
    out = r.render_all(meshes_of(verts, faces, rgb), normalize=True)
    want, _ = REF.normalize(verts)
    world = np.concatenate(want)
    assert np.abs(out["world"].cpu().numpy() - world).max() <= 5e-6
    pk = out["pk"]
    fp = pk.faces.cpu().numpy()
    vb = np.concatenate([[0], np.cumsum(pk.nv)])
    nrm = np.concatenate([REF.vertex_normals(w, f) for w, f in zip(want, faces)])
    assert np.abs(out["normals"].cpu().numpy() - nrm).max() <= 1e-5      # (normals of fp32-normalised vertices)
    img, _ = REF.shade(out["pix_to_face"].cpu().numpy(), out["bary"].cpu().numpy(), world, fp, nrm, np.concatenate(rgb), r.eye)
    err = np.abs(out["image"].cpu().numpy() - img).max()
    print(f"normalised batch: max |rgba - fp64| {err:.2e}")
    assert err <= 1e-4
    for b in (1, 2):
        i = out["image"][b].cpu().numpy()
        assert np.isfinite(i).all() and (i[..., :3] == 1).all() and (i[..., 3] == 0).all()
    # coverage against the restatement's own pipeline: the same silhouette up to the pixels a 1-unit snap difference moves
    ref_img, ref_p2f, _, _ = REF.render(verts, faces, rgb, *CAM, 32, normalized=True)
    diff = (ref_p2f >= 0) != (out["pix_to_face"].cpu().numpy() >= 0)
    assert diff.sum() <= 2
    assert vb[-1] == world.shape[0]


# ------------------------------------------------------------------------------------------------------------------ shading
def _box_mesh():
    v = np.array([[x, y, z] for x in (-0.4, 0.4) for y in (-0.3, 0.3) for z in (-0.2, 0.2)], dtype=np.float32)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                  [1, 5, 7], [1, 7, 3]])
    rgb = np.where(v[:, :1] < 0, np.array([[0.9, 0.2, 0.1]]), np.array([[0.1, 0.3, 0.8]])).astype(np.float32)
    return v, f, rgb


def _shading_case(name):
    if name in ("sphere16", "sphere32"):
        v, f = sphere_mesh(int(name[-2:]))
        rgb = (0.5 + 0.5 * np.sin(7 * v + np.array([0.0, 1.0, 2.0]))).astype(np.float32)
        return v, f[:, ::-1].copy(), rgb                        # (flipped: outward normals, as get_generated_models_v2 does)
    if name in ("synth16", "synth32"):                           # synth's analytic sphere-and-box volumes
        from commonscenes_amd import synth
        from commonscenes_amd.mesh import sdf_to_mesh
        m = sdf_to_mesh(synth.sdf_volume(int(name[-2:]) // 32, int(name[-2:])).cuda(), render_all=True)
        v, f = m.verts_list()[0].cpu().numpy(), m.faces_list()[0].cpu().numpy()
        return v, f[:, ::-1].copy(), (0.5 + 0.5 * np.cos(5 * v + np.array([2.0, 1.0, 0.0]))).astype(np.float32)
    if name == "box":
        return _box_mesh()
    v, f, rgb = _box_mesh()
    return v, f[:, ::-1].copy(), rgb                            # "inverted"


@pytest.mark.parametrize("name,size", [("sphere16", 17), ("sphere32", 64), ("synth16", 32), ("synth32", 64), ("box", 32),
                                       ("inverted", 16), ("inverted", 64)])
def test_shading_against_fp64_given_the_gpu_fragments(name, size):
    v, f, rgb = _shading_case(name)
    r = renderer(size)
    out = r.render_all(meshes_of([v], [f], [rgb]))
    p2f, bary = out["pix_to_face"].cpu().numpy(), out["bary"].cpu().numpy()
    assert (p2f >= 0).sum() > size * size / 20
    nrm = REF.vertex_normals(v, f)
    assert np.abs(out["normals"].cpu().numpy() - nrm).max() <= 1e-6
    want, info = REF.shade(p2f, bary, v, f, nrm, rgb, r.eye)
    got = out["image"].cpu().numpy()
    err = np.abs(got - want).max()                              # every pixel, background included
    print(f"shading {name} S={size}: {(p2f >= 0).sum()} covered pixels, max |rgba - fp64| {err:.2e}")
    assert err <= 1e-4
    assert np.abs(bary[p2f >= 0].sum(-1) - 1).max() <= 1e-6 and (bary[p2f < 0] == 0).all()
    lit = info["cos"] > 0
    assert lit.any() and (~lit).any()                           # both sides of the terminator are in view
    # where the light is behind the surface (by a margin fp32 cannot cross): ambient only, 0.5 * texel EXACTLY, with the
    # texel as the kernel forms it (fp32, (b0 c0 + b1 c1) + b2 c2)
    dark = np.zeros(p2f.shape, dtype=bool)
    dark[info["hit"]] = info["cos"] <= -1e-4
    assert dark.sum() > 0
    ids = f[p2f[dark]]
    b32, c32 = bary[dark].astype(np.float32), rgb.astype(np.float32)
    tex = (b32[:, 0:1] * c32[ids[:, 0]] + b32[:, 1:2] * c32[ids[:, 1]]) + b32[:, 2:3] * c32[ids[:, 2]]
    assert np.array_equal(got[dark][:, :3], np.float32(0.5) * tex)
    if name == "inverted":                                      # normals point inwards: every face seen from outside is dark
        box = r.render_all(meshes_of([v], [f[:, ::-1].copy()], [rgb]))
        assert torch.equal(box["pix_to_face"] >= 0, out["pix_to_face"] >= 0)


# ------------------------------------------------------------------------------- known answers, independent of the restatement
def test_sphere_silhouette_is_the_circle_perspective_predicts():
    """A radius-0.5 sphere on the SDF cube [-1, 1]^3 (SDFusion's convention; the mesh lives in [-0.5, 0.5), so its radius is
    0.25 plus the level's shift) centred on the grid point that sdf_to_mesh maps to the origin.  A sphere on the optical
    axis projects to a circle of angular radius asin(r / dist)."""
    from commonscenes_amd.mesh import sdf_to_mesh
    from commonscenes_amd.object_views import render_sdf
    n, S = 32, 64
    g = (torch.arange(n, dtype=torch.float32) / n - 0.5) * 2.0
    x, y, z = torch.meshgrid(g, g, g, indexing="ij")
    sdf = (torch.sqrt(x * x + y * y + z * z) - 0.5)[None, None].cuda()
    rad = float(sdf_to_mesh(sdf).verts_list()[0].norm(dim=1).max())
    assert 0.25 < rad < 0.27
    img = render_sdf(renderer(S), sdf)
    assert img.shape == (1, 4, S, S)
    alpha = img[0, 3].cpu().numpy()
    assert set(np.unique(alpha).tolist()) == {0.0, 1.0}
    radius = S / 2 * np.tan(np.arcsin(rad / 1.7)) / np.tan(np.deg2rad(30))
    area = alpha.sum()
    rows, cols = np.nonzero(alpha)
    cen = np.array([cols.mean() + 0.5, rows.mean() + 0.5])
    print(f"sphere silhouette: radius {radius:.3f} px, area {area:.0f} vs {np.pi * radius ** 2:.1f} "
          f"({area / (np.pi * radius ** 2) - 1:+.2%}), centroid {cen - S / 2}")
    assert abs(area / (np.pi * radius ** 2) - 1) <= 0.03
    assert np.abs(cen - S / 2).max() <= 0.5
    # a white sphere: ambient 0.5 at least, 0.5 + 0.3 + 0.2 at most
    rgb = img[0, :3].cpu().numpy()
    assert rgb.max() <= 1.0 + 1e-6 and rgb[:, alpha > 0].min() >= 0.5 - 1e-6 and rgb[:, alpha > 0].max() > 0.6
    # no surface at all: zeros, like the reference
    none = render_sdf(renderer(S), torch.ones(3, 1, 8, 8, 8).cuda(), render_imsize=48)
    assert none.shape == (3, 4, 48, 48) and float(none.abs().max()) == 0.0


def _mask_centroid(img_b):
    a = img_b[..., 3].cpu().numpy()
    rows, cols = np.nonzero(a)
    assert len(rows) > 0
    return cols.mean() + 0.5, rows.mean() + 0.5


def test_directions_and_depth_order_known_answers():
    from commonscenes_amd.object_views import render_meshes
    S = 64
    r = renderer(S)
    small = np.array([[-0.1, -0.1, 0.0], [0.1, -0.1, 0.0], [0.0, 0.2, 0.0]], dtype=np.float32)     # centroid at the origin
    right = small + np.array([0.5, 0, 0], dtype=np.float32)
    above = small + np.array([0, 0.5, 0], dtype=np.float32)
    img = render_meshes(r, meshes_of([small, right, above], [[[0, 1, 2]]] * 3))
    assert img.shape == (3, 4, S, S)
    chw = img.permute(0, 2, 3, 1)
    c0, cr, ca = (_mask_centroid(chw[k]) for k in range(3))
    assert abs(c0[0] - S / 2) < 1 and abs(c0[1] - S / 2) < 1       # the origin is the image centre
    assert cr[0] > S / 2 + 3                                       # world +x: right of centre
    assert ca[1] < S / 2 - 3                                       # world +y: above centre (row 0 is the top)
    # two stacked triangles along the view axis: the nearer one (towards the camera) wins, in either face order
    toward = (r.eye / np.linalg.norm(r.eye)).astype(np.float32)
    big = small * 4
    v = np.concatenate([big, big + 0.3 * toward])
    red, blue = np.tile([[1.0, 0, 0]], (3, 1)), np.tile([[0, 0, 1.0]], (3, 1))
    for faces, want in (([[0, 1, 2], [3, 4, 5]], 1), ([[3, 4, 5], [0, 1, 2]], 0)):
        out = r.render_all(meshes_of([v], [faces], [np.concatenate([red, blue])]))
        c = S // 2
        assert int(out["pix_to_face"][0, c, c]) == want
        px = out["image"][0, c, c].cpu().numpy()
        assert px[2] > px[0] and px[3] == 1.0                      # the blue one
        assert abs(float(out["zbuf"][0, c, c]) - (1.7 - 0.3)) < 0.05     # (pixel centre half a pixel off the axis)


# ---------------------------------------------------------------------------------------------------------- other checks
def test_sentinel_bands_past_every_output_survive():
    verts, faces, rgb = _ragged_batch()
    r = renderer(17)
    held = []
    PAD = 64

    def alloc(shape, dtype, dev):
        n = int(np.prod(shape))
        buf = torch.full((n + 2 * PAD,), 77, dtype=dtype, device=dev)
        held.append((buf, n))
        return buf[PAD:PAD + n].view(shape)

    ref = r.render_all(meshes_of(verts, faces, rgb), normalize=True)
    out = r.render_all(meshes_of(verts, faces, rgb), normalize=True, alloc=alloc)
    assert len(held) == 13                                         # every output and workspace of the five entries
    for buf, n in held:
        assert (buf[:PAD] == 77).all() and (buf[PAD + n:] == 77).all()
    for k in ("image", "pix_to_face", "zbuf", "bary", "normals", "world", "screen", "zview", "keys", "dropped"):
        assert torch.equal(out[k], ref[k]), k


def test_empty_batches_return_background():
    r = renderer(16)
    img = r(meshes_of([np.zeros((3, 3)), np.zeros((0, 3))], [np.zeros((0, 3)), np.zeros((0, 3))]))
    assert img.shape == (2, 16, 16, 4) and (img[..., :3] == 1).all() and (img[..., 3] == 0).all()
    frag = r.rasterize(meshes_of([np.zeros((3, 3))], [np.zeros((0, 3))]))
    assert (frag.pix_to_face == -1).all() and (frag.zbuf == -1).all() and frag.dropped.tolist() == [0]
    # a missing texture is white: ambient + diffuse + specular of 1
    tri = np.array([[-0.5, -0.3, 0.1], [0.6, -0.2, 0.0], [0.0, 0.5, -0.1]])
    a = r(meshes_of([tri], [[[0, 1, 2]]]))
    b = r(meshes_of([tri], [[[0, 1, 2]]], [np.ones((3, 3))]))
    assert torch.equal(a, b) and (a[..., 3] == 1).any()


def test_visuals_of_one_scene():
    from commonscenes_amd.object_views import get_current_visuals_v2
    from commonscenes_amd.scene_mesh import TriMesh
    verts, faces, rgb = _ragged_batch()
    ms = [TriMesh(torch.from_numpy(v), torch.from_numpy(np.asarray(f, dtype=np.int64)), torch.from_numpy(c))
          for v, f, c in zip(verts, faces, rgb)]
    vis = get_current_visuals_v2({}, renderer(32), ms, [0] * 5)
    assert list(vis.keys()) == [1, 2, 3, 4, 5]
    for k, im in vis.items():
        assert im.shape == (32, 32, 4) and im.dtype == np.uint8
        assert set(np.unique(im[..., 3]).tolist()) <= {127, 255}
    assert (vis[2][..., 3] == 127).all() and (vis[2][..., :3] == 255).all()
    assert (vis[1][..., 3] == 255).any()


def test_vqvae_model_renders_input_and_reconstruction():
    from collections import OrderedDict
    from commonscenes_amd import synth
    from commonscenes_amd.vqvae import VQVAE, vqvae_encoder_param_shapes, vqvae_param_shapes
    from commonscenes_amd.vqvae_model import VQVAEModel
    from oracle.ref_torch import VQ_FULL
    dd = dict(VQ_FULL, in_channels=1, double_z=False)
    table = OrderedDict(list(vqvae_encoder_param_shapes(dd, 8192, 3).items()) + list(vqvae_param_shapes(dd, 8192, 3).items()))
    vq = VQVAE(dd, 8192, 3, device="cuda").load_state_dict(synth.synth_state_dict(table, device="cuda"))
    vm = VQVAEModel(vqvae=vq)
    x = torch.cat([synth.sdf_volume(0), synth.sdf_volume(1)], dim=0)
    vm.inference({"sdf": x}, should_render=True)
    for img in (vm.image, vm.image_recon):
        assert img.shape == (2, 4, 256, 256) and img.dtype == torch.float32
        assert set(torch.unique(img[:, 3]).tolist()) <= {0.0, 1.0}
    assert (vm.image[:, 3] == 1).flatten(1).sum(1).min() > 1000          # the analytic volumes have a surface
    vis = vm.get_current_visuals()
    assert list(vis.keys()) == ["image", "image_recon"]
    for im in vis.values():
        assert im.dtype == np.uint8 and im.shape == (256 + 4, 2 * 256 + 6, 4)


def test_sdfusion_model_visual_panels():
    """SDFusionText2ShapeModel.get_current_visuals: img_gt and img_gen_df grids (the text panel is not built)"""
    from commonscenes_amd import synth
    from commonscenes_amd.sdfusion import SDFusionText2ShapeModel
    m = object.__new__(SDFusionText2ShapeModel)                     # the method reads only x, gen_df and the renderer
    m.x = torch.cat([synth.sdf_volume(0, 32), synth.sdf_volume(1, 32), synth.sdf_volume(0, 32)])
    m.gen_df = m.x[:2].cuda()
    vis = m.get_current_visuals({3: "chair", 5: "bed", 7: "lamp"}, [3, 5, 7], num_obj=2)
    assert list(vis.keys()) == ["img_gt", "img_gen_df"] and m.text_obj == ["chair", "bed"]
    for im in vis.values():
        assert im.dtype == np.uint8 and im.shape == (256 + 4, 2 * 256 + 6, 4)
    assert np.array_equal(vis["img_gt"], vis["img_gen_df"])         # the same two volumes
    assert (vis["img_gt"][..., 3] == 255).sum() > 2000 and m.img_gt.shape == (2, 4, 256, 256) and not m.img_gt.is_cuda
