"""FID / KID of the rendered scenes (scripts/compute_fid_scores_3dfront.py: cleanfid's `compute_fid`, `compute_fid(...,
model_name="clip_vit_b_32")` and `compute_kid`) behind cleanfid's names, with the statistics in fp64 on the device
(csrc/cs_fid.hip: cs_fid_moments, cs_fid_widen, cs_fid_gram on the fp64 MFMA, cs_fid_subset_sums).

    frechet_distance(feats1, feats2)   |mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrt(S1 S2), S the unbiased covariances (np.cov)
    kernel_distance(feats1, feats2)    cleanfid's KID: `num_subsets` random subsets of m rows, polynomial kernel (u.v / d + 1)^3
    image_features(images, model)      clip.preprocess + CLIP.encode_image, as encode_image returns them (no L2 normalisation),
                                       or inception.InceptionV3.encode_image (pool3, 2048 columns; mode= clean | legacy_pytorch)
    compute_fid / compute_kid          directories of .png (with a clip.CLIP or an inception.InceptionV3) or ready features
                                       (tensors, arrays, .npy paths)
    select_room(names, room)           the script's file filter

tr sqrt(S1 S2) takes one of two routes.  "gram" (min(N1, N2) <= d): with A, B the centred feature matrices,
tr sqrt(S1 S2) = ||A B^T||_* / sqrt((N1 - 1)(N2 - 1)) -- one N1 x N2 product on the device and the singular values of that small
matrix on the host; no d x d matrix and no matrix square root is formed, and the result is exact when the covariances are
singular (N <= d: the normal case for one room type of SG-FRONT's test split).  "cov" (otherwise): S = A^T A / (N - 1) from the
same kernel on the transposed operands, R = S1^(1/2) from numpy.linalg.eigh, and the sum of the square roots of the
eigenvalues of R S2 R, negative ones clipped to 0.  tr S is ss / (N - 1) from cs_fid_moments on both routes.

KID computes the three kernel matrices (N2 x N2, N1 x N1, N2 x N1) once and turns every subset into a gather-sum.  The subsets
are drawn on the CPU with cleanfid's own calls in cleanfid's order on numpy's legacy global generator, so `np.random.seed(s)`
before the call selects the subsets cleanfid selects.

Import swap for the script:
    from cleanfid import fid            ->  from commonscenes_amd import fid
    fid.compute_fid(real, fake)                                            ->  fid.compute_fid(real, fake, model=inception_model)
    fid.compute_fid(real, fake, mode="clean", model_name="clip_vit_b_32")  ->  fid.compute_fid(real, fake, model=clip_model)
    fid.compute_kid(real, fake)                                            ->  fid.compute_kid(real, fake, model=inception_model)

cleanfid is not part of the build image: its definitions are restated here from its published formulas and parity with it is
NOT pinned; whether its CLIP mode normalises the features could not be checked.  The InceptionV3 network (cleanfid's default
feature extractor) is commonscenes_amd/inception.py with the resize modes "clean" and "legacy_pytorch" ("legacy_tensorflow" is
out of scope); pool3 features computed elsewhere still enter as tensors / .npy.
"""
from __future__ import annotations

import math
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import lib as L
from . import ops

Tensor = torch.Tensor

# scripts/compute_fid_scores_3dfront.py:68
ROOM_DICT = {"bedroom": ["Bedroom", "MasterBedroom", "SecondBedroom"], "livingroom": ["LivingDiningRoom", "LivingRoom"],
             "diningroom": ["LivingDiningRoom", "DiningRoom"]}
MOMENT_COLS = 64        # CS_FID_MOMENT_COLS


def select_room(names: Sequence[str], room: str = "all") -> List[str]:
    """compute_fid_scores_3dfront.py:96-100: the names that end in .png and whose part before the first '-' is one of the
    room's types; "all" keeps every .png.  Order is kept."""
    if room == "all":
        return [oi for oi in names if oi.endswith(".png")]
    if room not in ROOM_DICT:
        raise ValueError(f"room must be one of {sorted(ROOM_DICT)} or 'all', got {room!r}")
    return [oi for oi in names if oi.endswith(".png") and oi.split('-')[0] in ROOM_DICT[room]]


def pick_route(n1: int, n2: int, d: int) -> str:
    """"gram" when min(N1, N2) <= d (a covariance is then singular and the N1 x N2 product is the smaller one), else "cov"."""
    return "gram" if min(int(n1), int(n2)) <= int(d) else "cov"


def kid_subsets(n1: int, n2: int, num_subsets: int, m: int) -> Tuple[np.ndarray, np.ndarray]:
    """(idx2 [num_subsets, m], idx1 [num_subsets, m]) int32: per subset np.random.choice(n2, m, replace=False) then
    np.random.choice(n1, m, replace=False), cleanfid's order, on numpy's legacy global generator.  Host only."""
    n1, n2, num_subsets, m = int(n1), int(n2), int(num_subsets), int(m)
    if num_subsets < 1 or m < 1 or m > min(n1, n2):
        raise ValueError(f"kid_subsets: {num_subsets} subsets of {m} rows out of {n1} / {n2}")
    i2 = np.empty((num_subsets, m), np.int32)
    i1 = np.empty((num_subsets, m), np.int32)
    for s in range(num_subsets):
        i2[s] = np.random.choice(n2, m, replace=False)
        i1[s] = np.random.choice(n1, m, replace=False)
    return i2, i1


# ----------------------------------------------------------------------------------------------------------------------
# the four entries
# ----------------------------------------------------------------------------------------------------------------------
def _check_shape(t, name: str) -> None:
    if not isinstance(t, torch.Tensor):
        raise L.CsError(f"{name}: expected a float32 HIP device tensor, got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise L.CsError(f"{name}: expected torch.float32, got {t.dtype}")
    if t.dim() != 2 or t.shape[1] < 1:
        raise L.CsError(f"{name}: expected [N, d], got {tuple(t.shape)}")


def _check_feats(t, name: str) -> None:
    _check_shape(t, name)
    if not t.is_cuda:
        raise L.CsError(f"{name}: expected a HIP device tensor (the HIP path has no CPU fallback)")


def _check_pair(feats1, feats2, what: str) -> Tuple[int, int, int]:
    """every refusal of frechet_distance / kernel_distance that needs no launch, in one place"""
    _check_shape(feats1, f"{what}: feats1")
    _check_shape(feats2, f"{what}: feats2")
    if feats1.shape[1] != feats2.shape[1]:
        raise L.CsError(f"{what}: the feature widths differ ({feats1.shape[1]} and {feats2.shape[1]})")
    n1, n2 = int(feats1.shape[0]), int(feats2.shape[0])
    if n1 < 2 or n2 < 2:
        raise ValueError(f"{what}: a covariance needs at least two rows per set, got {n1} and {n2}")
    if not feats1.is_cuda or not feats2.is_cuda:
        raise L.CsError(f"{what}: expected HIP device tensors (the HIP path has no CPU fallback)")
    if feats1.device != feats2.device:
        raise L.CsError(f"{what}: the feature sets live on different devices")
    return n1, n2, int(feats1.shape[1])


def _rows(t: Tensor) -> Tensor:
    return t if t.stride(1) == 1 and t.stride(0) >= t.shape[1] else t.contiguous()


def moments(x: Tensor) -> Tuple[Tensor, Tensor]:
    """cs_fid_moments: (mu fp64 [d], ss fp64 [1 + chunks]) on the device; ss[0] = sum_i |x_i - mu|^2."""
    _check_feats(x, "moments")
    x = _rows(x)
    n, d = int(x.shape[0]), int(x.shape[1])
    if n < 1:
        raise L.CsError("moments: no rows")
    mu = torch.empty((d,), dtype=torch.float64, device=x.device)
    ss = torch.empty((1 + (d + MOMENT_COLS - 1) // MOMENT_COLS,), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        L.check(L.load().cs_fid_moments(x.data_ptr(), n, d, int(x.stride(0)), mu.data_ptr(), ss.data_ptr(), ops._stream()),
                "cs_fid_moments")
    return mu, ss


def widen(x: Tensor, mu: Optional[Tensor] = None, transpose: bool = False, out: Optional[Tensor] = None) -> Tensor:
    """cs_fid_widen: (double)x - mu as fp64 [n, d], or [d, n] with `transpose`; `out` may be a wider view (its row stride is
    the leading dimension)."""
    _check_feats(x, "widen")
    x = _rows(x)
    n, d = int(x.shape[0]), int(x.shape[1])
    if n < 1:
        raise L.CsError("widen: no rows")
    if mu is not None and (not mu.is_cuda or mu.dtype != torch.float64 or tuple(mu.shape) != (d,) or not mu.is_contiguous()):
        raise L.CsError(f"widen: mu must be a dense float64 device tensor [{d}]")
    shape = (d, n) if transpose else (n, d)
    if out is None:
        out = torch.empty(shape, dtype=torch.float64, device=x.device)
    elif not out.is_cuda or out.dtype != torch.float64 or tuple(out.shape) != shape or out.stride(1) != 1 \
            or out.stride(0) < shape[1]:
        raise L.CsError(f"widen: out must be a float64 device view {shape} with unit column stride")
    with torch.cuda.device(x.device):
        L.check(L.load().cs_fid_widen(x.data_ptr(), n, d, int(x.stride(0)), ops._ptr(mu), out.data_ptr(), int(out.stride(0)),
                                      1 if transpose else 0, ops._stream()), "cs_fid_widen")
    return out


def _check_f64(t, name: str) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float64 or t.dim() != 2 or t.stride(1) != 1 \
            or t.stride(0) < t.shape[1] or t.shape[0] < 1 or t.shape[1] < 1:
        raise L.CsError(f"{name}: expected a non-empty float64 device matrix with unit column stride")


def gram(a: Tensor, b: Tensor, mode: int = 0, gamma: float = 1.0, coef0: float = 0.0, out: Optional[Tensor] = None) -> Tensor:
    """cs_fid_gram: g[i, j] = post(a[i] . b[j]) for a [n1, k], b [n2, k] float64 (row strides are the leading dimensions);
    mode 0: identity, mode 1: (s * gamma + coef0)^3."""
    _check_f64(a, "gram: a")
    _check_f64(b, "gram: b")
    if a.shape[1] != b.shape[1] or a.device != b.device:
        raise L.CsError(f"gram: operands of widths {a.shape[1]} and {b.shape[1]}")
    n1, n2, k = int(a.shape[0]), int(b.shape[0]), int(a.shape[1])
    if out is None:
        out = torch.empty((n1, n2), dtype=torch.float64, device=a.device)
    else:
        _check_f64(out, "gram: out")
        if tuple(out.shape) != (n1, n2):
            raise L.CsError(f"gram: out must be [{n1}, {n2}]")
    with torch.cuda.device(a.device):
        L.check(L.load().cs_fid_gram(a.data_ptr(), b.data_ptr(), out.data_ptr(), n1, n2, k, int(a.stride(0)), int(b.stride(0)),
                                     int(out.stride(0)), int(mode), float(gamma), float(coef0), ops._stream()), "cs_fid_gram")
    return out


def subset_sums(kmat: Tensor, ri, ci, skip_diag: bool, out: Optional[Tensor] = None) -> Tensor:
    """cs_fid_subset_sums: out[s] = sum_{p, q (p != q when skip_diag)} kmat[ri[s, p], ci[s, q]] -> float64 [nsub].  ri / ci:
    [nsub, m] integer tables (uploaded as int32) or int32 device tensors.  An index outside the matrix gives a NaN subset and
    sets ops.index_err_word; ops.check_index_errors raises for it."""
    _check_f64(kmat, "subset_sums: kmat")
    dev = kmat.device

    def table(v, name):
        t = v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))
        if t.is_floating_point() or t.dim() != 2:
            raise L.CsError(f"subset_sums: {name} must be an integer table [nsub, m]")
        return t.to(device=dev, dtype=torch.int32).contiguous()
    ri, ci = table(ri, "ri"), table(ci, "ci")
    if ri.shape != ci.shape or ri.shape[0] < 1 or ri.shape[1] < 1:
        raise L.CsError(f"subset_sums: ri {tuple(ri.shape)} and ci {tuple(ci.shape)} must be equal, non-empty [nsub, m]")
    nsub, m = int(ri.shape[0]), int(ri.shape[1])
    if out is None:
        out = torch.empty((nsub,), dtype=torch.float64, device=dev)
    elif not out.is_cuda or out.dtype != torch.float64 or tuple(out.shape) != (nsub,) or not out.is_contiguous():
        raise L.CsError(f"subset_sums: out must be a dense float64 device tensor [{nsub}]")
    with torch.cuda.device(dev):
        L.check(L.load().cs_fid_subset_sums(kmat.data_ptr(), int(kmat.shape[0]), int(kmat.shape[1]), int(kmat.stride(0)),
                                            ri.data_ptr(), ci.data_ptr(), nsub, m, 1 if skip_diag else 0, out.data_ptr(),
                                            ops.index_err_word(dev).data_ptr(), ops._stream()), "cs_fid_subset_sums")
    return out


# ----------------------------------------------------------------------------------------------------------------------
# FID
# ----------------------------------------------------------------------------------------------------------------------
def _sym_psd_eigs(m: np.ndarray) -> np.ndarray:
    return np.clip(np.linalg.eigvalsh((m + m.T) * 0.5), 0.0, None)


def trace_sqrt_from_gram(g: np.ndarray, n1: int, n2: int) -> float:
    """tr sqrt(S1 S2) from G = A B^T [N1, N2] (A, B centred): the nuclear norm of G over sqrt((N1 - 1)(N2 - 1))."""
    s = np.linalg.svd(np.asarray(g, np.float64), compute_uv=False)
    return float(s.sum() / math.sqrt(float(n1 - 1) * float(n2 - 1)))


def trace_sqrt_from_cov(s1: np.ndarray, s2: np.ndarray) -> float:
    """tr sqrt(S1 S2) from the two covariances: R = S1^(1/2) by eigh (negative eigenvalues clipped to 0), then the sum of
    the square roots of the clipped eigenvalues of R S2 R."""
    s1, s2 = np.asarray(s1, np.float64), np.asarray(s2, np.float64)
    w, v = np.linalg.eigh((s1 + s1.T) * 0.5)
    r = (v * np.sqrt(np.clip(w, 0.0, None))[None, :]) @ v.T
    return float(np.sqrt(_sym_psd_eigs(r @ s2 @ r)).sum())


def fid_from_parts(mu1, mu2, ss1: float, ss2: float, n1: int, n2: int, tr_sqrt: float) -> float:
    """|mu1 - mu2|^2 + ss1 / (N1 - 1) + ss2 / (N2 - 1) - 2 tr sqrt(S1 S2), float64 on the host."""
    diff = np.asarray(mu1, np.float64) - np.asarray(mu2, np.float64)
    return float(diff.dot(diff) + float(ss1) / (n1 - 1) + float(ss2) / (n2 - 1) - 2.0 * float(tr_sqrt))


def frechet_distance(feats1: Tensor, feats2: Tensor, route: Optional[str] = None) -> float:
    """cleanfid's frechet_distance over the two feature sets (fp32 [N, d] device tensors) -> a Python float.  route: "gram",
    "cov" or None = pick_route.  Read-backs: the moments (one copy), then the N1 x N2 product (gram) or the two covariances
    (cov, one copy)."""
    if route not in (None, "gram", "cov"):
        raise ValueError(f"frechet_distance: route must be 'gram', 'cov' or None, got {route!r}")
    n1, n2, d = _check_pair(feats1, feats2, "frechet_distance")
    route = pick_route(n1, n2, d) if route is None else route
    dev = feats1.device
    mu1, ss1 = moments(feats1)
    mu2, ss2 = moments(feats2)
    head = torch.cat([mu1, mu2, ss1[:1], ss2[:1]]).cpu().numpy()
    if not np.isfinite(head).all():
        raise ValueError("frechet_distance: a feature is not finite")
    m1, m2, s1, s2 = head[:d], head[d:2 * d], float(head[2 * d]), float(head[2 * d + 1])
    if route == "gram":
        g = gram(widen(feats1, mu1), widen(feats2, mu2)).cpu().numpy()
        tr = trace_sqrt_from_gram(g, n1, n2)
    else:
        cov = torch.empty((2, d, d), dtype=torch.float64, device=dev)
        for f, mu, c in ((feats1, mu1, cov[0]), (feats2, mu2, cov[1])):
            at = widen(f, mu, transpose=True)
            gram(at, at, out=c)
        cov = cov.cpu().numpy()
        tr = trace_sqrt_from_cov(cov[0] / (n1 - 1), cov[1] / (n2 - 1))
    return fid_from_parts(m1, m2, s1, s2, n1, n2, tr)


# ----------------------------------------------------------------------------------------------------------------------
# KID
# ----------------------------------------------------------------------------------------------------------------------
def kid_from_sums(sxx, syy, sxy, m: int) -> float:
    """cleanfid's accumulation over the subsets from the three gathered sums per subset (off-diagonal k(x, x), off-diagonal
    k(y, y), full k(x, y)), float64 on the host, in subset order."""
    t = 0.0
    for a, b, c in zip(np.asarray(sxx, np.float64), np.asarray(syy, np.float64), np.asarray(sxy, np.float64)):
        t += (a + b) / (m - 1) - c * 2 / m
    return float(t / len(sxx) / m)


def kernel_distance(feats1: Tensor, feats2: Tensor, num_subsets: int = 100, max_subset_size: int = 1000,
                    seed: Optional[int] = None) -> float:
    """cleanfid's kernel_distance (KID) -> a Python float.  m = min(N1, N2, max_subset_size); per subset x = feats2[choice],
    y = feats1[choice]; k(u, v) = (u.v / d + 1)^3.  seed: np.random.seed(seed) before the draw; None leaves numpy's global
    generator as it is (the caller's np.random.seed then selects the subsets, as for cleanfid)."""
    n1, n2, d = _check_pair(feats1, feats2, "kernel_distance")
    num_subsets, m = int(num_subsets), min(n1, n2, int(max_subset_size))
    if num_subsets < 1:
        raise ValueError("kernel_distance: num_subsets must be at least 1")
    if m < 2:
        raise ValueError("kernel_distance: subsets of fewer than two rows (KID divides by m - 1)")
    if seed is not None:
        np.random.seed(int(seed))
    i2, i1 = kid_subsets(n1, n2, num_subsets, m)        # drawn before anything touches the device
    dev = feats1.device
    x, y = widen(feats2), widen(feats1)
    gamma = 1.0 / d
    sums = torch.empty((3, num_subsets), dtype=torch.float64, device=dev)
    r2, r1 = torch.from_numpy(i2).to(dev), torch.from_numpy(i1).to(dev)
    subset_sums(gram(x, x, 1, gamma, 1.0), r2, r2, True, out=sums[0])
    subset_sums(gram(y, y, 1, gamma, 1.0), r1, r1, True, out=sums[1])
    subset_sums(gram(x, y, 1, gamma, 1.0), r2, r1, False, out=sums[2])
    s = sums.cpu().numpy()
    if not np.isfinite(s).all():
        ops.check_index_errors(dev, what="kernel_distance subsets")       # (host-drawn rows are in range: never raises)
        raise ValueError("kernel_distance: a feature is not finite")
    return kid_from_sums(s[0], s[1], s[2], m)


# ----------------------------------------------------------------------------------------------------------------------
# images -> features -> numbers
# ----------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def image_features(images, model, batch: int = 64, mode: Optional[str] = None) -> Tensor:
    """paths / PIL images (through clip.preprocess) or uint8 [B, S, S, 3] -> CLIP.encode_image features fp32 [N, E] on the
    device, `batch` images per call, exactly as encode_image returns them.  With an inception.InceptionV3: its encode_image
    (paths / PIL images or uint8 [B, H, W, 3]; `mode` = "clean", the default, or "legacy_pytorch") -> pool3 features [N, 2048]."""
    from . import clip as K
    from . import inception as I
    incep = isinstance(model, I.InceptionV3)
    if not incep and (not isinstance(model, K.CLIP) or model.vision is None):
        raise L.CsError("image_features: model must be a clip.CLIP with a vision tower")
    if mode is not None and not incep:
        raise L.CsError("image_features: mode= selects an InceptionV3 resize; a clip.CLIP has one preprocess")
    batch = max(1, int(batch))
    size = None if incep else model.vision.resolution
    tensor_in = isinstance(images, (torch.Tensor, np.ndarray))
    if not tensor_in:
        from PIL import Image
        single = isinstance(images, (str, bytes, Image.Image)) or hasattr(images, "__fspath__")
        images = [images] if single else list(images)
    n = len(images)
    if n < 1:
        raise ValueError("image_features: no images")
    out = []
    for i in range(0, n, batch):
        chunk = images[i:i + batch]
        if incep:
            out.append(model.encode_image(torch.as_tensor(chunk) if tensor_in else chunk, mode=mode or "clean"))
        else:
            out.append(model.encode_image(torch.as_tensor(chunk) if tensor_in else K.preprocess(chunk, size)))
    return torch.cat(out) if len(out) > 1 else out[0]


def list_images(directory, room: str = "all") -> List[str]:
    """the .png files of `directory` that pass select_room, as full paths in sorted name order (os.listdir's order is the file
    system's: sorting makes KID's subsets reproducible)"""
    return [os.path.join(str(directory), oi) for oi in select_room(sorted(os.listdir(str(directory))), room)]


def features_of(src, model, room: str, batch: int, what: str, mode: Optional[str] = None) -> Tensor:
    if isinstance(src, torch.Tensor):
        return src
    if isinstance(src, np.ndarray):
        arr = src
    elif isinstance(src, (str, bytes)) or hasattr(src, "__fspath__"):
        path = os.fspath(src)
        if os.path.isdir(path):
            if model is None:
                raise L.CsError(f"{what}: a directory of images needs model=<clip.CLIP>")
            files = list_images(path, room)
            if len(files) < 2:
                raise ValueError(f"{what}: {len(files)} images of room {room!r} in {path}: a covariance needs two")
            return image_features(files, model, batch, mode=mode)
        arr = np.load(path)
    else:
        raise L.CsError(f"{what}: expected a directory, a .npy path, an array or a device tensor, got {type(src).__name__}")
    if arr.ndim != 2 or arr.dtype != np.float32:
        raise L.CsError(f"{what}: features must be float32 [N, d], got {arr.dtype} {arr.shape}")
    dev = model.device if model is not None else torch.device("cuda", torch.cuda.current_device())
    return torch.from_numpy(np.ascontiguousarray(arr)).to(dev)


def compute_fid(real, fake, model=None, room: str = "all", batch: int = 64, route: Optional[str] = None,
                mode: Optional[str] = None) -> float:
    """cleanfid's compute_fid(fdir1, fdir2): `real` / `fake` are directories of .png (then `model` is a clip.CLIP or an
    inception.InceptionV3 -- with `mode` its resize, "clean" by default -- and `room` the script's filter) or features: fp32
    device tensors, float32 arrays or .npy paths (how features computed elsewhere enter)."""
    f1 = features_of(real, model, room, batch, "compute_fid", mode)
    f2 = features_of(fake, model, room, batch, "compute_fid", mode)
    return frechet_distance(f1, f2, route=route)


def compute_kid(real, fake, model=None, room: str = "all", batch: int = 64, num_subsets: int = 100,
                max_subset_size: int = 1000, seed: Optional[int] = None, mode: Optional[str] = None) -> float:
    """cleanfid's compute_kid(fdir1, fdir2) over the same inputs as compute_fid."""
    f1 = features_of(real, model, room, batch, "compute_kid", mode)
    f2 = features_of(fake, model, room, batch, "compute_kid", mode)
    return kernel_distance(f1, f2, num_subsets=num_subsets, max_subset_size=max_subset_size, seed=seed)
