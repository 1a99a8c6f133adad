"""Shape-quality table of the paper's shape branch behind the call surface of the reference's
scripts/compute_mmd_cov_1nn.py: MMD / COV / 1-NNA under Chamfer and approximate EMD (`compute_all_metrics`) and the JSD of
occupancy grids (`jsd_between_point_cloud_sets`).

The hot path is three HIP entries (csrc/cs_pairwise.hip): the all-pairs Chamfer matrix, the all-pairs approximate-EMD
cost without a match matrix, and the nearest-cell histogram.  Everything that acts on an N x N matrix or on the grid's
counters (`lgan_mmd_cov`, `knn`, the entropy formulas) is plumbing: one copy to the host, float64 numpy, results back as
tensors on the input's device, as the script returns them.

Point clouds are float32 [N, P, 3] tensors on the HIP device.  Which EMD route runs is decided by one rule: clouds of up
to `EMD_FUSED_MAX_POINTS` points take the fused entry, larger ones the per-pass entries of emd.py pair by pair.
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np
import torch

from . import lib as L
from .chamfer import nm_distance
from .emd import ApproxMatch, MatchCost

Tensor = torch.Tensor

EMD_FUSED_MAX_POINTS = 8192      # CS_EMD_PAIRWISE_MAX_POINTS
CHAMFER_MAX_Q = 32768            # CS_CHAMFER_PAIRWISE_MAX_Q
_BATCHED_MATCH_BYTES = 8 << 30   # match matrices one batched EMD call of the per-pass route may hold


def _check(t, name: str) -> Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 3 or t.shape[-1] != 3 \
            or t.shape[0] < 1 or t.shape[1] < 1:
        raise L.CsError(f"{name} must be a non-empty float32 [N, P, 3] tensor on the HIP device")
    return t.contiguous()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ----------------------------------------------------------------------------------------------------------------------
# all-pairs matrices
# ----------------------------------------------------------------------------------------------------------------------
def pairwise_cd(a: Tensor, b: Tensor, symmetric: bool = False) -> Tensor:
    """cd[i, j] = mean_k min_l |a_ik - b_jl|^2 + mean_l min_k |a_ik - b_jl|^2, [na, nb] fp32 (compute_mmd_cov_1nn.py:131-134).
    `symmetric=True` (b must be a) computes i <= j and mirrors; the result is bit-equal to the full matrix."""
    same = b is a
    a = _check(a, "a")
    b = a if same else _check(b, "b")
    if symmetric and not (b.data_ptr() == a.data_ptr() and b.shape == a.shape):
        raise L.CsError("symmetric=True needs b to be a")
    if b.shape[1] > CHAMFER_MAX_Q:
        raise L.CsError(f"pairwise_cd holds one minimum per point of b in LDS: at most {CHAMFER_MAX_Q} points")
    out = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
    L.check(L.load().cs_chamfer_pairwise(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.shape[0], b.shape[0], a.shape[1],
                                         b.shape[1], 1 if symmetric else 0, _stream()), "cs_chamfer_pairwise")
    return out


def pairwise_emd_cost(a: Tensor, b: Tensor) -> Tensor:
    """cost[i, j] = match_cost(a_i, b_j), un-normalised, [na, nb] fp32.  The point counts may differ (integer multiplicity,
    approxmatch.cu:6-12)."""
    a, b = _check(a, "a"), _check(b, "b")
    if max(a.shape[1], b.shape[1]) > EMD_FUSED_MAX_POINTS:
        return pairwise_emd_cost_batched(a, b)
    out = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
    L.check(L.load().cs_emd_pairwise_cost(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.shape[0], b.shape[0], a.shape[1],
                                          b.shape[1], _stream()), "cs_emd_pairwise_cost")
    return out


def pairwise_emd(a: Tensor, b: Tensor) -> Tensor:
    """emd[i, j] = match_cost(a_i, b_j) / N (emd_approx_cuda, :56-62); equal point counts, as the script asserts."""
    a, b = _check(a, "a"), _check(b, "b")
    if a.shape[1] != b.shape[1]:
        raise L.CsError("EMD needs clouds of equal point counts")
    return pairwise_emd_cost(a, b) / float(a.shape[1])


# the script's own way of driving the per-pair kernels (one cloud expanded to a batch, host loops): what the all-pairs
# entries replace.  Kept for clouds beyond the fused kernel's size and as the yardstick of tools/shape_metrics.py.
def pairwise_cd_batched(a: Tensor, b: Tensor, batch_size: int = 50) -> Tensor:
    a, b = _check(a, "a"), _check(b, "b")
    rows = []
    for i in range(a.shape[0]):
        row = []
        for j0 in range(0, b.shape[0], batch_size):
            bb = b[j0:j0 + batch_size]
            ae = a[i].view(1, -1, 3).expand(bb.shape[0], -1, -1).contiguous()
            dl, _ = nm_distance(ae, bb)
            dr, _ = nm_distance(bb, ae)
            row.append((dl.mean(dim=1) + dr.mean(dim=1)).view(1, -1))
        rows.append(torch.cat(row, dim=1))
    return torch.cat(rows, dim=0)


def pairwise_emd_cost_batched(a: Tensor, b: Tensor, batch_size: int = 50) -> Tensor:
    a, b = _check(a, "a"), _check(b, "b")
    batch_size = max(1, min(batch_size, _BATCHED_MATCH_BYTES // (4 * a.shape[1] * b.shape[1])))
    rows = []
    for i in range(a.shape[0]):
        row = []
        for j0 in range(0, b.shape[0], batch_size):
            bb = b[j0:j0 + batch_size]
            ae = a[i].view(1, -1, 3).expand(bb.shape[0], -1, -1).contiguous()
            match, _ = ApproxMatch(ae, bb)
            row.append(MatchCost(ae, bb, match).view(1, -1))
            del match
        rows.append(torch.cat(row, dim=1))
    return torch.cat(rows, dim=0)


def _pairwise_EMD_CD_(sample_pcs: Tensor, ref_pcs: Tensor, batch_size: int = 50, accelerated_cd: bool = True,
                      accelerated_emd: bool = True, symmetric: bool = False) -> Tuple[Tensor, Tensor]:
    """(all_cd, all_emd), both [N_sample, N_ref] (:110-150).  `batch_size` and the two switches are accepted for the
    script's callers and ignored: there is one route and it has no batches."""
    return pairwise_cd(sample_pcs, ref_pcs, symmetric=symmetric), pairwise_emd(sample_pcs, ref_pcs)


def EMD_CD(sample_pcs: Tensor, ref_pcs: Tensor, batch_size: int = 50, accelerated_cd: bool = True, reduced: bool = True,
           accelerated_emd: bool = True) -> Dict[str, Tensor]:
    """The diagonal pairing sample_i <-> ref_i (:69-107): {'MMD-CD', 'MMD-EMD'}, means when `reduced`."""
    sample_pcs, ref_pcs = _check(sample_pcs, "sample_pcs"), _check(ref_pcs, "ref_pcs")
    if sample_pcs.shape[0] != ref_pcs.shape[0]:
        raise L.CsError(f"REF:{ref_pcs.shape[0]} SMP:{sample_pcs.shape[0]}")
    if sample_pcs.shape[1] != ref_pcs.shape[1]:
        raise L.CsError("EMD needs clouds of equal point counts")
    from .emd import match_cost
    cds, emds = [], []
    for s in range(0, sample_pcs.shape[0], max(1, int(batch_size))):
        sb, rb = sample_pcs[s:s + batch_size], ref_pcs[s:s + batch_size]
        dl, _ = nm_distance(sb, rb)
        dr, _ = nm_distance(rb, sb)
        cds.append(dl.mean(dim=1) + dr.mean(dim=1))
        emds.append(match_cost(sb, rb) / float(sb.shape[1]))
    cd, emd = torch.cat(cds), torch.cat(emds)
    return {"MMD-CD": cd.mean() if reduced else cd, "MMD-EMD": emd.mean() if reduced else emd}


# ----------------------------------------------------------------------------------------------------------------------
# statistics of the matrices: host, float64
# ----------------------------------------------------------------------------------------------------------------------
def _host(t) -> np.ndarray:
    return t.detach().cpu().numpy().astype(np.float64) if isinstance(t, torch.Tensor) else np.asarray(t, np.float64)


def _like(v, ref) -> Tensor:
    if isinstance(ref, torch.Tensor):
        return torch.tensor(v, dtype=ref.dtype, device=ref.device)
    return torch.tensor(v, dtype=torch.float64)


def lgan_mmd_cov(all_dist) -> Dict[str, Tensor]:
    """all_dist [N_sample, N_ref] (:186-198): MMD = mean over refs of the nearest sample's distance, MMD-smp the other way
    round, COV = share of refs that are some sample's nearest."""
    d = _host(all_dist)
    n_ref = d.shape[1]
    return {
        "lgan_mmd": _like(d.min(axis=0).mean(), all_dist),
        # (the script rounds this one ratio to float32 on its way into a tensor, whatever the matrix's type)
        "lgan_cov": _like(float(np.float32(len(np.unique(d.argmin(axis=1))) / float(n_ref))), all_dist),
        "lgan_mmd_smp": _like(d.min(axis=1).mean(), all_dist),
    }


def knn(Mxx, Mxy, Myy, k: int, sqrt: bool = False) -> Dict[str, Tensor]:
    """Leave-one-out k-NN classifier over the joint distance matrix (:154-183): label 1 for the n0 clouds of Mxx, 0 for the
    n1 of Myy; a point is predicted 1 when at least k / 2 of its k nearest others are."""
    xx, xy, yy = _host(Mxx), _host(Mxy), _host(Myy)
    n0, n1 = xx.shape[0], yy.shape[0]
    label = np.concatenate([np.ones(n0), np.zeros(n1)])
    m = np.block([[xx, xy], [xy.T, yy]])
    if sqrt:
        m = np.sqrt(np.abs(m))
    m = m + np.diag(np.full(n0 + n1, np.inf))
    idx = np.argsort(m, axis=0, kind="stable")[:k]               # the k smallest of every column
    count = label[idx].sum(axis=0)
    pred = (count >= k / 2.0).astype(np.float64)
    tp, fp = (pred * label).sum(), (pred * (1 - label)).sum()
    fn, tn = ((1 - pred) * label).sum(), ((1 - pred) * (1 - label)).sum()
    s = {
        "tp": tp, "fp": fp, "fn": fn, "tn": tn,
        "precision": tp / (tp + fp + 1e-10),
        "recall": tp / (tp + fn + 1e-10),
        "acc_t": tp / (tp + fn + 1e-10),
        "acc_f": tn / (tn + fp + 1e-10),
        # (the script takes this one mean in float32, whatever the matrices' type)
        "acc": float(np.float32((label == pred).sum()) / np.float32(n0 + n1)),
    }
    return {key: _like(v, Mxx) for key, v in s.items()}


def compute_all_metrics(sample_pcs: Tensor, ref_pcs: Tensor, batch_size: int = 50, accelerated_cd: bool = True
                        ) -> Dict[str, Tensor]:
    """The twelve numbers of the table (:201-229): lgan_mmd / lgan_cov / lgan_mmd_smp and 1-NN acc_t / acc_f / acc, each
    under CD and EMD.  The script builds the ref x sample matrix and hands its transpose to lgan_mmd_cov; so does this."""
    sample_pcs, ref_pcs = _check(sample_pcs, "sample_pcs"), _check(ref_pcs, "ref_pcs")
    if sample_pcs.shape[1] != ref_pcs.shape[1]:
        raise L.CsError("EMD needs clouds of equal point counts")
    results = {}
    m_rs_cd, m_rs_emd = _pairwise_EMD_CD_(ref_pcs, sample_pcs, batch_size)
    results.update({f"{k}-CD": v for k, v in lgan_mmd_cov(m_rs_cd.t()).items()})
    results.update({f"{k}-EMD": v for k, v in lgan_mmd_cov(m_rs_emd.t()).items()})
    m_rr_cd, m_rr_emd = _pairwise_EMD_CD_(ref_pcs, ref_pcs, batch_size, symmetric=True)
    m_ss_cd, m_ss_emd = _pairwise_EMD_CD_(sample_pcs, sample_pcs, batch_size, symmetric=True)
    results.update({f"1-NN-CD-{k}": v for k, v in knn(m_rr_cd, m_rs_cd, m_ss_cd, 1).items() if "acc" in k})
    results.update({f"1-NN-EMD-{k}": v for k, v in knn(m_rr_emd, m_rs_emd, m_ss_emd, 1).items() if "acc" in k})
    return results


# ----------------------------------------------------------------------------------------------------------------------
# JSD of occupancy grids
# ----------------------------------------------------------------------------------------------------------------------
def unit_cube_grid_point_cloud(resolution: int, clip_sphere: bool = False) -> Tuple[np.ndarray, float]:
    """Cell centres of a resolution^3 grid over the unit cube, float32, x slowest (:235-253); with `clip_sphere` only the
    cells inside the sphere of radius 0.5, as an [g, 3] array."""
    spacing = 1.0 / float(resolution - 1)
    axis = (np.arange(resolution, dtype=np.float64) * spacing - 0.5).astype(np.float32)
    grid = np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), axis=-1)
    if clip_sphere:
        grid = grid.reshape(-1, 3)
        grid = grid[np.linalg.norm(grid, axis=1) <= 0.5]
    return grid, spacing


def occupancy_histogram(pcs: Tensor, grid) -> Tuple[Tensor, Tensor]:
    """(grid_counters [g], grid_bernoulli [g]) int32: hits per cell, and clouds with at least one hit per cell, of every
    point's nearest cell (ties: lowest index) in ONE shared grid [g, 3]."""
    pcs = _check(pcs, "pcs")
    g = torch.as_tensor(np.ascontiguousarray(grid, dtype=np.float32).reshape(-1, 3)) if not isinstance(grid, torch.Tensor) \
        else grid.reshape(-1, 3)
    g = g.to(device=pcs.device, dtype=torch.float32).contiguous()
    idx = torch.empty(pcs.shape[:2], dtype=torch.int32, device=pcs.device)
    counters = torch.empty((g.shape[0],), dtype=torch.int32, device=pcs.device)
    bern = torch.empty_like(counters)
    L.check(L.load().cs_occupancy_histogram(pcs.data_ptr(), g.data_ptr(), idx.data_ptr(), counters.data_ptr(),
                                            bern.data_ptr(), pcs.shape[0], pcs.shape[1], g.shape[0], _stream()),
            "cs_occupancy_histogram")
    return counters, bern


def _entropy(p: np.ndarray, base: float = np.e) -> float:
    p = np.asarray(p, np.float64)
    p = p / p.sum()
    nz = p[p > 0]
    return float(-(nz * np.log(nz)).sum() / np.log(base))


def occupancy_entropy(grid_bernoulli, n_clouds: int) -> float:
    """Mean over ALL cells of the entropy of each hit cell's Bernoulli variable (:302-309)."""
    b = np.asarray(grid_bernoulli, np.float64)
    acc = 0.0
    for g in b[b > 0]:
        p = g / float(n_clouds)
        acc += _entropy(np.array([p, 1.0 - p]))
    return acc / len(b)


def entropy_of_occupancy_grid(pclouds: Tensor, grid_resolution: int, in_sphere: bool = False) -> Tuple[float, np.ndarray]:
    """(entropy, grid_counters as float64 numpy) like the script's function of the same name (:270-309)."""
    grid, _ = unit_cube_grid_point_cloud(grid_resolution, in_sphere)
    counters, bern = occupancy_histogram(pclouds, grid)
    return occupancy_entropy(bern.cpu().numpy(), pclouds.shape[0]), counters.cpu().numpy().astype(np.float64)


def jensen_shannon_divergence(P, Q) -> float:
    """JSD in bits of two non-negative vectors, each normalised to a distribution first (:312-331)."""
    P, Q = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    if np.any(P < 0) or np.any(Q < 0):
        raise ValueError("Negative values.")
    if len(P) != len(Q):
        raise ValueError("Non equal size.")
    p, q = P / P.sum(), Q / Q.sum()
    return _entropy((p + q) / 2.0, 2) - (_entropy(p, 2) + _entropy(q, 2)) / 2.0


def jsd_between_point_cloud_sets(sample_pcs: Tensor, ref_pcs: Tensor, resolution: int = 28) -> float:
    """JSD between the occupancy distributions of two cloud sets over the resolution^3 grid clipped to the unit sphere
    (:256-267)."""
    s = entropy_of_occupancy_grid(sample_pcs, resolution, True)[1]
    r = entropy_of_occupancy_grid(ref_pcs, resolution, True)[1]
    return jensen_shannon_divergence(s, r)
