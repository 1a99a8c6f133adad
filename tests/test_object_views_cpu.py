"""Per-object views, host side (no GPU): the look-at camera, tensor2im's tiling and conversion, the PNG name rule, and the
fp64 restatement the GPU tests lean on (tests/_object_view_ref.py) against a closed form."""
import numpy as np
import pytest
import torch

import _object_view_ref as REF


def test_look_at_view_transform_matches_pytorch3d_conventions():
    from commonscenes_amd import object_views as OV
    R, T = OV.look_at_view_transform(1.7, 20, 20)
    assert R.dtype == np.float64 and T.dtype == np.float64 and R.shape == (3, 3) and T.shape == (3,)
    C = OV.camera_position(R, T)
    assert np.abs(C - np.array([0.5463695, 0.5814342, 1.5011378])).max() < 1e-6
    assert np.abs(R.T @ R - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1.0) < 1e-12
    assert np.abs(np.zeros(3) @ R + T - np.array([0.0, 0.0, 1.7])).max() < 1e-12          # the origin sits at depth dist
    up = np.array([0.0, 1.0, 0.0]) @ R                        # directions: no translation
    assert up[1] > 0.9 and abs(up[0]) < 1e-12                  # world +y is view +y (up in the image)
    right = np.array([1.0, 0.0, 0.0]) @ R
    assert right[0] < -0.9                                     # world +x is view -x: +X is LEFT in NDC, so right in the image
    R2, T2, C2 = REF.camera(1.7, 20, 20)                       # the tests' own restatement agrees
    assert np.abs(R - R2).max() < 1e-15 and np.abs(T - T2).max() < 1e-15 and np.abs(C - C2).max() < 1e-15
    for elev in (90, -90):
        with pytest.raises(ValueError):
            OV.look_at_view_transform(3.5, elev, 90)
    with pytest.raises(ValueError):
        OV.init_mesh_renderer()                                # the reference's default elev = 90
    with pytest.raises(NotImplementedError):
        OV.init_mesh_renderer(image_size=64, dist=1.7, elev=20, azim=20, camera="1")
    for bad in (0, 8193):
        with pytest.raises(ValueError):
            OV.init_mesh_renderer(image_size=bad, dist=1.7, elev=20, azim=20)


def test_tensor2im_single_rgba_image():
    from commonscenes_amd.object_views import tensor2im
    t = torch.zeros(4, 5, 7)
    t[:3] = 1.0                       # white
    t[3, :, :3] = 1.0                 # alpha 1 on the left, 0 on the right
    t[0, 0, 0] = 0.5                  # (0.5 + 1) / 2 * 255 = 191.25 -> 191
    t[1, 0, 0] = 0.004                # (1.004) / 2 * 255 = 128.01 -> 128
    t[2, 0, 0] = 0.0117               # 128.99... -> 128: truncation, not rounding
    im = tensor2im(t)
    assert im.shape == (5, 7, 4) and im.dtype == np.uint8
    assert (im[1:, :, :3] == 255).all()
    assert (im[:, :3, 3] == 255).all() and (im[:, 3:, 3] == 127).all()
    assert tuple(im[0, 0, :3]) == (191, 128, 128)
    assert (1.0117 / 2.0 * 255.0) % 1 > 0.9                    # the case above really sits just under the next integer


def test_tensor2im_grid_of_five():
    from commonscenes_amd.object_views import tensor2im
    t = torch.stack([torch.full((4, 8, 8), v) for v in (1.0, 0.5, 0.0, -0.5, -1.0)])
    im = tensor2im(t)
    assert im.shape == (2 * 8 + 3 * 2, 4 * 8 + 5 * 2, 4)
    want = {0: 255, 1: 191, 2: 127, 3: 63, 4: 0}
    tile = np.zeros(im.shape[:2], dtype=bool)
    for k, val in want.items():
        r, c = divmod(k, 4)
        blk = im[2 + r * 10:2 + r * 10 + 8, 2 + c * 10:2 + c * 10 + 8]
        assert (blk == val).all(), k
        tile[2 + r * 10:2 + r * 10 + 8, 2 + c * 10:2 + c * 10 + 8] = True
    assert (im[~tile] == 127).all()                            # padding value 0 -> 127, the empty cells of row 2 included
    # more than 16 images: only the first 16, 4 rows of 4
    assert tensor2im(torch.zeros(20, 4, 8, 8)).shape == (4 * 8 + 5 * 2, 4 * 8 + 5 * 2, 4)
    # one channel is repeated to three
    assert tensor2im(torch.zeros(2, 1, 8, 8)).shape == (8 + 4, 2 * 8 + 3 * 2, 3)


def test_store_current_imgs_name_rule(tmp_path):
    from collections import OrderedDict
    from PIL import Image
    from commonscenes_amd.object_views import store_current_imgs
    classes = ["_scene_\n", "bed\n", "floor\n", "chair\n", "lamp\n"]
    rng = np.random.default_rng(0)
    visuals = OrderedDict((k, rng.integers(0, 256, (6, 6, 4), dtype=np.uint8)) for k in (1, 2, 3))
    cat_ids = [1, 2, 3, 0, 4]          # bed, (floor ->) chair, (_scene_ ->) lamp
    paths = store_current_imgs(visuals, str(tmp_path), classes, cat_ids)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["bed_1_1.png", "chair_3_2.png", "lamp_4_3.png"]
    assert len(paths) == 3
    for k, name in ((1, "bed_1_1.png"), (2, "chair_3_2.png"), (3, "lamp_4_3.png")):
        img = Image.open(tmp_path / name)
        assert img.mode == "RGBA"
        assert np.array_equal(np.asarray(img), visuals[k])


def test_restatement_against_the_phong_formula_by_hand():
    """one triangle facing the camera's side of the light, its three vertex normals equal (one face: they all are the face
    normal): the centre pixel's colour is the Phong formula at the point the centre ray meets the triangle's plane."""
    S = 17
    R, T, C = REF.camera(1.7, 20, 20)
    v = np.array([[-0.6, 0.1, -0.5], [0.7, 0.1, -0.5], [0.1, 0.1, 0.8]])       # in the plane y = 0.1; normal +y after winding
    f = np.array([[0, 2, 1]])
    rgb = np.array([[0.2, 0.5, 0.9]] * 3)
    n = REF.vertex_normals(v, f)
    assert np.abs(n - np.array([0.0, 1.0, 0.0])).max() < 1e-12
    img, p2f, zbuf, bary = REF.render([v], [f], [rgb], 1.7, 20, 20, S)
    c = S // 2
    assert p2f[0, c, c] == 0
    # centre pixel: NDC (0, 0), the ray from C along the view axis z = -C/|C|, met with the plane y = 0.1
    zaxis = -C / np.linalg.norm(C)
    t = (0.1 - C[1]) / zaxis[1]
    p = C + t * zaxis
    assert abs(zbuf[0, c, c] - t) < 2e-3                         # (the snapped grid moves the vertices by <= 1/512 pixel)
    nrm = np.array([0.0, 1.0, 0.0])
    l = (REF.LIGHT - p) / np.linalg.norm(REF.LIGHT - p)
    cosa = nrm @ l
    vdir = (C - p) / np.linalg.norm(C - p)
    refl = -l + 2 * cosa * nrm
    want = (0.5 + 0.3 * max(cosa, 0)) * rgb[0] + 0.2 * (max(vdir @ refl, 0) * (cosa > 0)) ** 64
    assert cosa > 0.5
    assert np.abs(img[0, c, c, :3] - want).max() < 5e-3 and img[0, c, c, 3] == 1.0
    # tighter: at the restatement's own interpolated point the formula is met to rounding
    ids = f[0]
    pp = (bary[0, c, c][:, None] * v[ids]).sum(0)
    l = (REF.LIGHT - pp) / np.linalg.norm(REF.LIGHT - pp)
    cosa = nrm @ l
    vdir = (C - pp) / np.linalg.norm(C - pp)
    want = (0.5 + 0.3 * cosa) * rgb[0] + 0.2 * max(vdir @ (-l + 2 * cosa * nrm), 0) ** 64
    assert np.abs(img[0, c, c, :3] - want).max() < 1e-12
    assert np.abs(pp - p).max() < 2e-3
    # the other winding: the normal points away from the light -> ambient only
    img2, _, _, _ = REF.render([v], [f[:, ::-1]], [rgb], 1.7, 20, 20, S)
    assert np.abs(img2[0, c, c, :3] - 0.5 * rgb[0]).max() < 1e-12
    # background
    assert tuple(img[0, 0, 0]) == (1.0, 1.0, 1.0, 0.0) and p2f[0, 0, 0] == -1 and zbuf[0, 0, 0] == -1.0
