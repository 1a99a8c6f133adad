"""fp64 / integer restatement of the per-object view pipeline (commonscenes_amd/object_views.py, csrc/cs_view.hip) for the
tests: pytorch3d's look-at camera, normalize_py3d_meshes, verts_normals_packed, the exact-coverage rasteriser and
HardPhongShader with the default lights, written from their documented behaviour.  numpy only."""
import numpy as np

FOCAL = 1.0 / np.tan(np.deg2rad(30.0))
LIGHT = np.array([0.0, 1.0, 0.0])
ZMIN = 0.5


def camera(dist, elev, azim):
    """-> R [3,3], T [3] (X_view = X_world @ R + T), C [3]"""
    e, a = np.deg2rad(elev), np.deg2rad(azim)
    C = dist * np.array([np.cos(e) * np.sin(a), np.sin(e), np.cos(e) * np.cos(a)])
    z = -C / np.linalg.norm(C)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    y /= np.linalg.norm(y)
    R = np.stack([x, y, z], axis=1)
    return R, -C @ R, C


def normalize(verts_list):
    """one centre (mean over all packed vertices), one scale per mesh; extent 0 -> the origin"""
    vs = [np.asarray(v, dtype=np.float64) for v in verts_list]
    centre = np.concatenate(vs).mean(axis=0)
    out = []
    for v in vs:
        c = v - centre
        r = np.sqrt((c * c).sum(axis=1)).max() if len(c) else 0.0
        out.append(c / r if (r > 0 and np.isfinite(r)) else np.zeros_like(c))
    return out, centre


def project(verts, R, T, size):
    """-> continuous (col, row) pixel coordinates in 1/256 units (not rounded) and z_view, fp64"""
    v = np.asarray(verts, dtype=np.float64) @ R + T
    z = v[:, 2]
    px = (1.0 - FOCAL * v[:, 0] / z) * 0.5 * size * 256.0
    py = (1.0 - FOCAL * v[:, 1] / z) * 0.5 * size * 256.0
    return np.stack([px, py], axis=1), z


def snap(sub):
    return np.floor(sub + 0.5).astype(np.int64)


def vertex_normals(verts, faces):
    v = np.asarray(verts, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    n = np.zeros_like(v)
    if len(f):
        cr = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
        for k in range(3):
            np.add.at(n, f[:, k], cr)
    return n / np.maximum(np.sqrt((n * n).sum(axis=1, keepdims=True)), 1e-6)


def oracle_raster(screen, zview, faces, size, zmin=ZMIN, nverts_range=None):
    """Integer coverage (int64 edge functions on the snapped grid, top-left rule, both windings), perspective-correct depth
    in fp32 in the rasteriser's operation order, ties to the lower face id.  screen [V,2] int (col, row), zview [V] fp32.
    nverts_range = (lo, hi): ids outside are malformed (the face draws nothing).
    -> depth [size,size] fp32 (inf empty), winner (-1), second-nearest depth (inf), dropped"""
    X, Y = np.asarray(screen)[:, 0].astype(np.int64), np.asarray(screen)[:, 1].astype(np.int64)
    d = np.asarray(zview, dtype=np.float32)
    lo, hi = nverts_range if nverts_range is not None else (0, len(d))
    best = np.full((size, size), np.inf, dtype=np.float32)
    second = np.full((size, size), np.inf, dtype=np.float32)
    win = np.full((size, size), -1, dtype=np.int64)
    dropped = 0
    py, px = np.meshgrid(np.arange(size, dtype=np.int64), np.arange(size, dtype=np.int64), indexing="ij")
    cx, cy = px * 256 + 128, py * 256 + 128
    edge = lambda ax, ay, bx, by, qx, qy: (bx - ax) * (qy - ay) - (by - ay) * (qx - ax)
    for fid, (i0, i1, i2) in enumerate(np.asarray(faces, dtype=np.int64)):
        if min(i0, i1, i2) < lo or max(i0, i1, i2) >= hi:
            continue
        dd = d[[i0, i1, i2]]
        if not np.all(np.isfinite(dd)) or dd.min() < zmin:
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
            es.append(e.astype(np.float32))
        d0, d1, d2 = d[idx[0]], d[idx[1]], d[idx[2]]
        if d0 == d1 and d1 == d2:
            dep = np.full((size, size), d0, dtype=np.float32)
        else:
            a32 = np.float32(area)
            with np.errstate(divide="ignore", invalid="ignore"):
                inv = ((es[0] / a32) / d0 + (es[1] / a32) / d1) + (es[2] / a32) / d2
                dep = (np.float32(1.0) / inv).astype(np.float32)
        dep = np.where(inside, dep, np.float32(np.inf)).astype(np.float32)
        closer = dep < best                                    # strict: equal depths stay with the lower face id
        second = np.where(closer, best, np.minimum(second, dep))
        win = np.where(closer, fid, win)
        best = np.where(closer, dep, best)
    return best, win, second, dropped


def barycentrics(screen, zview, faces, pix_to_face):
    """perspective-correct barycentrics of the winning faces from the integer edge functions, fp64: [S,S,3] (0 empty)"""
    size = pix_to_face.shape[0]
    X, Y = np.asarray(screen)[:, 0].astype(np.int64), np.asarray(screen)[:, 1].astype(np.int64)
    z = np.asarray(zview, dtype=np.float64)
    out = np.zeros((size, size, 3))
    for r, c in zip(*np.nonzero(pix_to_face >= 0)):
        i = np.asarray(faces)[pix_to_face[r, c]]
        cx, cy = c * 256 + 128, r * 256 + 128
        e = np.array([(X[i[b]] - X[i[a]]) * (cy - Y[i[a]]) - (Y[i[b]] - Y[i[a]]) * (cx - X[i[a]])
                      for a, b in ((1, 2), (2, 0), (0, 1))], dtype=np.float64)
        w = e / e.sum() / z[i]
        out[r, c] = w / w.sum()
    return out


def shade(pix_to_face, bary, verts, faces, normals, rgb, eye):
    """HardPhongShader, default PointLights / Materials, hard blend on white: [..., 4] fp64 RGBA.  pix_to_face / bary may carry
    any leading shape; faces hold ids into verts / normals / rgb."""
    p2f = np.asarray(pix_to_face)
    b = np.asarray(bary, dtype=np.float64)
    v, n, c = (np.asarray(a, dtype=np.float64) for a in (verts, normals, rgb))
    f = np.asarray(faces, dtype=np.int64)
    out = np.ones(p2f.shape + (4,))
    out[..., 3] = 0.0
    hit = p2f >= 0
    ids = f[p2f[hit]]                                        # [K,3]
    w = b[hit][:, :, None]                                   # [K,3,1]
    tex, nn, pp = (w * c[ids]).sum(1), (w * n[ids]).sum(1), (w * v[ids]).sum(1)
    unit = lambda a: a / np.maximum(np.sqrt((a * a).sum(1, keepdims=True)), 1e-6)
    nn = unit(nn)
    l = unit(LIGHT[None] - pp)
    cosa = (nn * l).sum(1, keepdims=True)
    diffuse = 0.3 * np.maximum(cosa, 0.0)
    vv = unit(np.asarray(eye, dtype=np.float64)[None] - pp)
    refl = -l + 2.0 * cosa * nn
    alpha = np.maximum((vv * refl).sum(1, keepdims=True), 0.0) * (cosa > 0)
    col = (0.5 + diffuse) * tex + 0.2 * alpha ** 64
    out[hit] = np.concatenate([col, np.ones((len(col), 1))], axis=1)
    return out, dict(cos=cosa[:, 0], texel=tex, hit=hit)


def render(verts_list, faces_list, rgb_list, dist, elev, azim, size, normalized=False):
    """the whole pipeline in fp64 (faces local to each mesh) -> image [B,S,S,4], pix_to_face (packed ids), zbuf, bary"""
    R, T, C = camera(dist, elev, azim)
    vs = [np.asarray(v, dtype=np.float64) for v in verts_list]
    if normalized:
        vs, _ = normalize(vs)
    imgs, p2fs, zs, bs = [], [], [], []
    foff = 0
    for v, f, c in zip(vs, faces_list, rgb_list):
        f = np.asarray(f, dtype=np.int64).reshape(-1, 3)
        if len(v) == 0 or len(f) == 0:
            win = np.full((size, size), -1, dtype=np.int64)
            img, _ = shade(win, np.zeros((size, size, 3)), np.zeros((1, 3)), np.zeros((1, 3), dtype=np.int64),
                           np.zeros((1, 3)), np.zeros((1, 3)), C)
            imgs.append(img), p2fs.append(win), zs.append(np.full((size, size), -1.0)), bs.append(np.zeros((size, size, 3)))
            foff += len(f)
            continue
        sub, z = project(v, R, T, size)
        scr = snap(sub)
        best, win, _, _ = oracle_raster(scr, z.astype(np.float32), f, size)
        bary = barycentrics(scr, z, f, win)
        img, _ = shade(win, bary, v, f, vertex_normals(v, f), c, C)
        imgs.append(img), bs.append(bary)
        p2fs.append(np.where(win >= 0, win + foff, -1))
        zs.append(np.where(win >= 0, best.astype(np.float64), -1.0))
        foff += len(f)
    return np.stack(imgs), np.stack(p2fs), np.stack(zs), np.stack(bs)
