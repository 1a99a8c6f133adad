"""Host restatements for the scene-library tests (commonscenes_amd/scene_library.py, csrc/cs_scene_lib.hip).

helpers/util.py cannot be imported here (it needs trimesh), so retrieval is pinned by a restatement of its three numpy lines
(:74-77), the placement by :121-129, and the draws of get_sdfusion_models by :351-358.  The tube markers are this package's own
construction (include/commonscenes_hip.h): `ref_marker` restates it in fp64 numpy; parity with trimesh.creation.cylinder is
unpinned."""
import random

import numpy as np

EDGES = [[0, 1], [0, 2], [0, 4], [1, 3], [1, 5], [2, 3], [2, 6], [3, 7], [4, 5], [4, 6], [5, 7], [6, 7]]      # util.py:405


def ref_retrieve(lhw, query32):
    """helpers/util.py:74-77: lhw fp64 [M,3], query fp32 [3] -> (argmin, min) of np.sum((lhw - q) ** 2, axis=-1)"""
    lhw = np.asarray(lhw, dtype=np.float64)
    q = np.asarray(query32, dtype=np.float32)
    mses = np.sum((lhw - q) ** 2, axis=-1)
    i = int(np.argmin(mses))
    return i, mses[i]


def ref_rotation(angle, degrees=True):                            # util.py:121-127 / :510-516
    th = angle * (np.pi / 180) if degrees else angle
    R = np.zeros((3, 3))
    R[0, 0], R[0, 2], R[2, 0], R[2, 2], R[1, 1] = np.cos(th), -np.sin(th), np.sin(th), np.cos(th), 1.0
    return R


def ref_place(verts32, box32, degrees=True):
    """util.py:121-129 in fp64 from the fp32 box row -> (placed vertices, |A| |v| + |t| for the error bound)"""
    b = np.asarray(box32, dtype=np.float32).astype(np.float64)
    R, t = ref_rotation(b[6], degrees), b[3:6]
    v = np.asarray(verts32, dtype=np.float32).astype(np.float64)
    return v.dot(R) + t, np.abs(v).dot(np.abs(R)) + np.abs(t)


def ref_marker(box_points32, radius, sections):
    """the tubes of one box from its fp32 corners [8,3] -> (verts fp64 [12 (2S+2), 3], faces int64 [48 S, 3], tube lengths)"""
    S = int(sections)
    r = float(np.float32(radius))
    P = np.asarray(box_points32, dtype=np.float32).astype(np.float64)
    V, F, lens = [], [], []
    for e, (ia, ib) in enumerate(EDGES):
        a, b = P[ia], P[ib]
        d = b - a
        ln = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        lens.append(ln)
        base = e * (2 * S + 2)
        if not (ln > 0) or not np.isfinite(ln):
            V += [a.copy() for _ in range(2 * S + 2)]
        else:
            m = 0
            if abs(d[1]) < abs(d[m]):
                m = 1
            if abs(d[2]) < abs(d[m]):
                m = 2
            em = np.zeros(3)
            em[m] = 1.0
            u = np.cross(d, em)
            u = u / np.sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2])
            w = np.cross(d / ln, u)
            for p in (a, b):
                for k in range(S):
                    ang = 2.0 * np.pi * k / S
                    V.append(p + r * (np.cos(ang) * u + np.sin(ang) * w))
            V += [a.copy(), b.copy()]
        tri = []
        for k in range(S):
            tri.append([k, (k + 1) % S, S + (k + 1) % S])
        for k in range(S):
            tri.append([k, S + (k + 1) % S, S + k])
        for k in range(S):
            tri.append([2 * S, (k + 1) % S, k])
        for k in range(S):
            tri.append([2 * S + 1, S + k, S + (k + 1) % S])
        F += [[base + i for i in t] for t in tri]
    return np.asarray(V, dtype=np.float64), np.asarray(F, dtype=np.int64), np.asarray(lens)


def ref_choices(labels, files_of, no_stool, seed):
    """util.py:351-358 per shaped object, on a random.Random(seed): a = randint(0, 100); seed(a); choice(files);
    for a chair under no_stool two more choices"""
    r = random.Random(seed)
    out = []
    for lab in labels:
        a = r.randint(0, 100)
        r.seed(a)
        path = r.choice(files_of[lab])
        if no_stool and lab == "chair":
            path2 = r.choice(files_of["stool"])
            path = r.choice([path, path2])
        out.append(path)
    return out


def box_mesh(size):
    """a closed box of (l, h, w) standing on y = 0: 8 vertices, 12 outward triangles"""
    l, h, w = [float(s) for s in size]
    v = np.asarray([[l / 2 * i, h * j, w / 2 * k] for i in (-1, 1) for j in (0, 1) for k in (-1, 1)], dtype=np.float32)
    f = np.asarray([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                    [1, 5, 7], [1, 7, 3]], dtype=np.int64)
    return v, f


def write_ply(path, v, f, binary, double=False, index_type="int"):
    """a minimal writer of the test's own (the package's is not trusted to check its reader)"""
    import struct
    vt = "double" if double else "float"
    with open(path, "wb") as fh:
        fh.write(("ply\nformat %s 1.0\ncomment test\nelement vertex %d\nproperty %s x\nproperty %s y\nproperty %s z\n"
                  "element face %d\nproperty list uchar %s vertex_indices\nend_header\n" % (
                      "binary_little_endian" if binary else "ascii", len(v), vt, vt, vt, len(f), index_type)).encode())
        if binary:
            for p in v:
                fh.write(struct.pack("<3d" if double else "<3f", *[float(x) for x in p]))
            for t in f:
                fh.write(struct.pack("<B", len(t)))
                fh.write(struct.pack("<%d%s" % (len(t), {"int": "i", "uchar": "B"}[index_type]), *[int(x) for x in t]))
        else:
            for p in v:
                fh.write(("%r %r %r\n" % tuple(float(x) for x in p)).encode())
            for t in f:
                fh.write((" ".join(str(int(x)) for x in [len(t), *t]) + "\n").encode())
