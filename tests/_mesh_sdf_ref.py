"""fp64 numpy brute force of commonscenes_amd.mesh_sdf's definitions, and the meshes its tests are built from.

Same definitions, independent code: the closest point of every triangle (Ericson's regions, masks instead of selects) and
then |p - q|; the Van Oosterom-Strackee solid angle from the corner vectors themselves (a . (b x c), no precomputed normal);
inside where |w| >= level; the exact area-weighted centroid and the largest used-vertex distance from it.  A triangle
without area is the union of its three edges for the distance and contributes 0 to the winding number.
"""
import numpy as np

OFF = np.array([0.0137, -0.0291, 0.0073])
BOX_HALF = np.array([0.31, 0.47, 0.53])
ICO_RADIUS = 0.61803


# ------------------------------------------------------------------------------------------------------------------ geometry
def grid_points(n, bound=1.0):
    """[n^3, 3] node positions, index (i, j, k) = (x, y, z), node i at -bound + i * 2 bound / (n - 1)"""
    g = -bound + np.arange(n, dtype=np.float64) * (2.0 * bound / (n - 1))
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def _segment_dist(p, a, b):
    ab = b - a
    l2 = float(ab @ ab)
    t = np.zeros(len(p)) if l2 == 0.0 else np.clip(((p - a) @ ab) / l2, 0.0, 1.0)
    return np.linalg.norm(p - (a + t[:, None] * ab), axis=1)


def _is_degenerate(a, b, c):
    n = np.cross(b - a, c - a)
    l2 = max(float((b - a) @ (b - a)), float((c - b) @ (c - b)), float((a - c) @ (a - c)))
    return float(n @ n) <= 1e-24 * l2 * l2


def _triangle_dist(p, a, b, c):
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = ap @ ab, ap @ ac
    bp = p - b
    d3, d4 = bp @ ab, bp @ ac
    cp = p - c
    d5, d6 = cp @ ab, cp @ ac
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    q = np.empty_like(p)
    done = np.zeros(len(p), bool)

    def put(mask, val):
        mask = mask & ~done
        q[mask] = val[mask] if val.ndim == 2 else val
        done[mask] = True

    with np.errstate(all="ignore"):
        put((d1 <= 0) & (d2 <= 0), a)
        put((d3 >= 0) & (d4 <= d3), b)
        put((vc <= 0) & (d1 >= 0) & (d3 <= 0), a + (d1 / (d1 - d3))[:, None] * ab)
        put((d6 >= 0) & (d5 <= d6), c)
        put((vb <= 0) & (d2 >= 0) & (d6 <= 0), a + (d2 / (d2 - d6))[:, None] * ac)
        put((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), b + ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[:, None] * (c - b))
        den = 1.0 / (va + vb + vc)
        put(np.ones(len(p), bool), a + ab * (vb * den)[:, None] + ac * (vc * den)[:, None])
    return np.linalg.norm(p - q, axis=1)


def distance(p, tri):
    """p [P,3], tri [F,3,3] -> [P] distance to the nearest point of any triangle"""
    p = np.asarray(p, np.float64)
    best = np.full(len(p), np.inf)
    for a, b, c in np.asarray(tri, np.float64):
        if _is_degenerate(a, b, c):
            d = np.minimum(np.minimum(_segment_dist(p, a, b), _segment_dist(p, b, c)), _segment_dist(p, c, a))
        else:
            d = _triangle_dist(p, a, b, c)
        best = np.minimum(best, d)
    return best


def winding(p, tri):
    """p [P,3], tri [F,3,3] -> [P] generalised winding number sum Omega / 4 pi"""
    p = np.asarray(p, np.float64)
    w = np.zeros(len(p))
    for ta, tb, tc in np.asarray(tri, np.float64):
        if _is_degenerate(ta, tb, tc):
            continue
        a, b, c = ta - p, tb - p, tc - p
        la, lb, lc = np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1), np.linalg.norm(c, axis=1)
        num = (a * np.cross(b, c)).sum(1)
        den = la * lb * lc + (a * b).sum(1) * lc + (b * c).sum(1) * la + (c * a).sum(1) * lb
        w += 2.0 * np.arctan2(num, den)
    return w / (4.0 * np.pi)


def sdf(p, tri, level=0.5):
    """(signed distance, unsigned distance, winding number): negative where |w| >= level"""
    d, w = distance(p, tri), winding(p, tri)
    return np.where(np.abs(w) >= level, -d, d), d, w


def centroid_scale(verts, faces):
    """exact area-weighted centroid of the triangles, largest distance of a used vertex from it"""
    v = np.asarray(verts, np.float64)
    t = v[np.asarray(faces)]
    area = 0.5 * np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1)
    cen = (area[:, None] * t.mean(1)).sum(0) / area.sum()
    m = np.linalg.norm(t.reshape(-1, 3) - cen, axis=1).max()
    return cen, m


def get_normalize_mesh(verts, faces):
    cen, m = centroid_scale(verts, faces)
    return (np.asarray(verts, np.float64) - cen) / m, cen, m


def box_sdf(p, half=BOX_HALF, centre=OFF):
    q = np.abs(np.asarray(p, np.float64) - centre) - half
    return np.linalg.norm(np.maximum(q, 0.0), axis=1) + np.minimum(q.max(1), 0.0)


# -------------------------------------------------------------------------------------------------------------------- meshes
def icosphere(sub, radius=ICO_RADIUS, centre=OFF):
    """20 * 4^sub faces, outward normals; (verts fp64 [V,3], faces int64 [F,3])"""
    t = (1 + 5 ** .5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, float) / np.linalg.norm(x) for x in v]
    for _ in range(sub):
        cache, nf = {}, []

        def mid(i, j):
            k = (min(i, j), max(i, j))
            if k not in cache:
                m = v[i] + v[j]
                v.append(m / np.linalg.norm(m))
                cache[k] = len(v) - 1
            return cache[k]

        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v) * radius + centre, np.array(f, dtype=np.int64)


def hemisphere(sub=2):
    """the open upper half of icosphere(sub): the faces whose centroid lies above the centre"""
    v, f = icosphere(sub)
    keep = v[f].mean(1)[:, 2] > OFF[2]
    return v, f[keep]


def box(half=BOX_HALF, centre=OFF):
    c = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], float) * half + centre
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = np.array([t for a, b, cc, d in quads for t in ((a, b, cc), (a, cc, d))], dtype=np.int64)
    return c, f


def torus(nu=24, nv=12, big=0.55, small=0.21, centre=OFF):
    """closed torus around the z axis, 2 nu nv faces"""
    u = np.arange(nu) * (2 * np.pi / nu)
    w = np.arange(nv) * (2 * np.pi / nv)
    uu, ww = np.meshgrid(u, w, indexing="ij")
    v = np.stack([(big + small * np.cos(ww)) * np.cos(uu), (big + small * np.cos(ww)) * np.sin(uu), small * np.sin(ww)], -1)
    idx = lambda i, j: (i % nu) * nv + (j % nv)
    f = []
    for i in range(nu):
        for j in range(nv):
            f += [(idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1))]
    return v.reshape(-1, 3) + centre, np.array(f, dtype=np.int64)


def random_soup(nf, seed, extent=0.7, size=0.25):
    """nf small independent triangles (an open, self-overlapping mesh): any face count, fractional winding numbers"""
    rs = np.random.RandomState(seed)
    c = rs.uniform(-extent, extent, (nf, 1, 3))
    v = (c + rs.uniform(-size, size, (nf, 3, 3))).reshape(-1, 3)
    return v, np.arange(3 * nf, dtype=np.int64).reshape(nf, 3)
