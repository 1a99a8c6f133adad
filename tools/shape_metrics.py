#!/usr/bin/env python
"""Shape-quality table (MMD / COV / 1-NNA under CD and EMD, JSD) of two point-cloud sets, as JSON.

    python tools/shape_metrics.py SAMPLE.npy REF.npy            ([N, P, 3] arrays; .npz: the first array, or --key)
    python tools/shape_metrics.py --synthetic 116 5000 --compare-batched

--compare-batched also times the ref x sample Chamfer and EMD matrices on the route the reference's script takes with the
per-pair kernels (one cloud expanded to a batch of 50, host loops: nm_distance x 2, ApproxMatch + MatchCost) against the
all-pairs entries, interleaved in this process, and reports min / median / max of each and the matrices' differences.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from commonscenes_amd import shape_metrics as SM      # noqa: E402


def _load(path, key):
    d = np.load(path)
    if isinstance(d, np.lib.npyio.NpzFile):
        d = d[key or d.files[0]]
    return torch.from_numpy(np.ascontiguousarray(d, dtype=np.float32))


def _synthetic(n, p, seed):
    """noisy ellipsoid surfaces with per-cloud axes, centred and scaled to max |coordinate| 1 like the script's loader"""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn((n, p, 3), generator=g)
    v = v / v.norm(dim=-1, keepdim=True) * (0.25 + 0.75 * torch.rand((n, 1, 3), generator=g))
    v = v + 0.01 * torch.randn((n, p, 3), generator=g)
    v = v - v.mean(dim=1, keepdim=True)
    return v / v.abs().amax(dim=(1, 2), keepdim=True)


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def _stats(ts):
    return {"min_s": min(ts), "median_s": statistics.median(ts), "max_s": max(ts), "runs": len(ts)}


def compare(ref, smp, repeats, batch_size):
    out = {}
    for name, new, old in (("cd", lambda: SM.pairwise_cd(ref, smp), lambda: SM.pairwise_cd_batched(ref, smp, batch_size)),
                           ("emd", lambda: SM.pairwise_emd_cost(ref, smp),
                            lambda: SM.pairwise_emd_cost_batched(ref, smp, batch_size))):
        new(), torch.cuda.synchronize()                     # one untimed pass of each: code objects, allocator
        t_new, t_old = [], []
        for _ in range(repeats):
            t, m_old = _timed(old)
            t_old.append(t)
            t, m_new = _timed(new)
            t_new.append(t)
        diff = (m_new.double() - m_old.double()).abs()
        out[name] = {"all_pairs": _stats(t_new), "batched": _stats(t_old),
                     "speedup_median": statistics.median(t_old) / statistics.median(t_new),
                     "max_abs_diff": float(diff.max()), "max_rel_diff": float((diff / m_old.double().abs().clamp_min(1e-30)).max())}
    n, p = ref.shape[0] * smp.shape[0], ref.shape[1]
    # three passes of nine levels, one exponential per point pair each
    out["emd"]["exponentials_per_s"] = 27.0 * n * p * smp.shape[1] / out["emd"]["all_pairs"]["median_s"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("sets", nargs="*", help="SAMPLE REF (.npy / .npz)")
    ap.add_argument("--key", default=None)
    ap.add_argument("--synthetic", nargs=2, type=int, metavar=("N", "P"))
    ap.add_argument("--compare-batched", action="store_true")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch-size", type=int, default=50)
    ap.add_argument("--no-table", action="store_true", help="with --compare-batched: timings only")
    a = ap.parse_args()
    if a.synthetic:
        smp, ref = _synthetic(a.synthetic[0], a.synthetic[1], 1), _synthetic(a.synthetic[0], a.synthetic[1], 2)
    elif len(a.sets) == 2:
        smp, ref = _load(a.sets[0], a.key), _load(a.sets[1], a.key)
    else:
        ap.error("give SAMPLE and REF, or --synthetic N P")
    smp, ref = smp.cuda(), ref.cuda()
    res = {"clouds": [int(smp.shape[0]), int(ref.shape[0])], "points": int(smp.shape[1]),
           "device": torch.cuda.get_device_name(0)}
    if not a.no_table:
        t, table = _timed(lambda: SM.compute_all_metrics(smp, ref, a.batch_size))
        res["metrics"] = {k: float(v) for k, v in table.items()}
        res["metrics_s"] = t
        res["jsd"] = SM.jsd_between_point_cloud_sets(smp * 0.5, ref * 0.5)      # (the grid spans [-0.5, 0.5])
    if a.compare_batched:
        res["compare"] = compare(ref, smp, max(3, a.repeats), a.batch_size)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
