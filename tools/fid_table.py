#!/usr/bin/env python
"""The FID / KID table of scripts/compute_fid_scores_3dfront.py through commonscenes_amd.fid.

    python tools/fid_table.py --real DIR --fake DIR [--clip {MODEL.pt | synthetic}]
        [--inception {MODEL.pth | synthetic} [--inception-mode clean|legacy_pytorch]] [--room bedroom|livingroom|diningroom|all]
    python tools/fid_table.py --features REAL.npy FAKE.npy
    python tools/fid_table.py --synthetic N1 N2 D
        [--kid-subsets 100] [--kid-subset-size 1000] [--seed S] [--batch 64] [--compare-host]

prints one `FID_TABLE {...}` JSON line: fid, kid, n_real, n_fake, d, route, kid_subsets, kid_subset_size, seed.  The
directories are what `tools/eval_walkthrough.py --export-scenes DIR` writes (256 x 256 top-down PNGs named <RoomType>-...png).
`--clip synthetic` runs the ViT-B/32 vision tower on synthetic weights (the numbers mean nothing; the path is the real one).
--inception adds (or, without --clip, gives alone) the InceptionV3 pool3 numbers -- the reference prints both -- as an
`inception` block: fid, kid, n_real, n_fake, d, route, mode, images_per_second (both directories through decode, resize and
the network, one timed pass; report only).  MODEL.pth holds a state dict in torchvision's Inception3 names.
--features takes float32 [N, d] arrays computed elsewhere (e.g. InceptionV3 pool3).  --compare-host adds the same two numbers
from the numpy float64 formulas on the same features, with both wall times (report only; the device times follow one untimed
pass)."""
import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")


def synthetic_features(n1, n2, d, seed=2024):
    """two float32 feature sets with different means and per-column spreads, from numpy's default_rng(seed)"""
    rng = np.random.default_rng(seed)
    scale = rng.uniform(0.5, 2.0, size=d)
    f1 = (rng.standard_normal((n1, d)) * scale + rng.standard_normal(d)).astype(np.float32)
    f2 = (rng.standard_normal((n2, d)) * scale * 1.1 + 0.5 * rng.standard_normal(d)).astype(np.float32)
    return f1, f2


def host_fid(f1, f2, route):
    """the numpy float64 formulas of commonscenes_amd.fid, features to number, on the host"""
    from commonscenes_amd import fid
    f1, f2 = f1.astype(np.float64), f2.astype(np.float64)
    n1, n2 = len(f1), len(f2)
    mu1, mu2 = f1.mean(axis=0), f2.mean(axis=0)
    a, b = f1 - mu1, f2 - mu2
    if route == "gram":
        tr = fid.trace_sqrt_from_gram(a @ b.T, n1, n2)
    else:
        tr = fid.trace_sqrt_from_cov(a.T @ a / (n1 - 1), b.T @ b / (n2 - 1))
    return fid.fid_from_parts(mu1, mu2, float((a * a).sum()), float((b * b).sum()), n1, n2, tr)


def host_kid(f1, f2, num_subsets, max_subset_size):
    """cleanfid's loop as published, numpy float64, on numpy's global generator"""
    f1, f2 = f1.astype(np.float64), f2.astype(np.float64)
    n = f1.shape[1]
    m = min(min(f1.shape[0], f2.shape[0]), max_subset_size)
    t = 0
    for _ in range(num_subsets):
        x = f2[np.random.choice(f2.shape[0], m, replace=False)]
        y = f1[np.random.choice(f1.shape[0], m, replace=False)]
        a = (x @ x.T / n + 1) ** 3 + (y @ y.T / n + 1) ** 3
        b = (x @ y.T / n + 1) ** 3
        t += (a.sum() - np.diag(a).sum()) / (m - 1) - b.sum() * 2 / m
    return float(t / num_subsets / m)


def inception_block(args, dev, kid_kw):
    """the `inception` block of the FID_TABLE line: InceptionV3 pool3 features of both directories, then the same statistics"""
    from commonscenes_amd import fid, inception as I
    if args.inception == "synthetic":
        model = I.InceptionV3(dev).load_state_dict(I.synth_inception_state_dict(7))
    else:
        model = I.load_checkpoint(args.inception, dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    g1 = fid.features_of(args.real, model, args.room, args.batch, "fid_table", args.inception_mode)
    g2 = fid.features_of(args.fake, model, args.room, args.batch, "fid_table", args.inception_mode)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    n1, n2, d = int(g1.shape[0]), int(g2.shape[0]), int(g1.shape[1])
    return dict(fid=fid.frechet_distance(g1, g2), kid=fid.kernel_distance(g1, g2, **kid_kw), n_real=n1, n_fake=n2, d=d,
                route=fid.pick_route(n1, n2, d), mode=args.inception_mode, images_per_second=(n1 + n2) / dt)


def parse_args(argv=None):
    """the command line with every check that needs no device"""
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--real")
    ap.add_argument("--fake")
    ap.add_argument("--clip", help="MODEL.pt (OpenAI's ViT-B-32.pt) or 'synthetic'")
    ap.add_argument("--inception", help="MODEL.pth (a state dict in torchvision's Inception3 names) or 'synthetic'")
    ap.add_argument("--inception-mode", default="clean", choices=["clean", "legacy_pytorch"])
    ap.add_argument("--room", default="all", choices=["bedroom", "livingroom", "diningroom", "all"])
    ap.add_argument("--features", nargs=2, metavar=("REAL.npy", "FAKE.npy"))
    ap.add_argument("--synthetic", nargs=3, type=int, metavar=("N1", "N2", "D"))
    ap.add_argument("--kid-subsets", type=int, default=100)
    ap.add_argument("--kid-subset-size", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--compare-host", action="store_true")
    args = ap.parse_args(argv)
    modes = [args.synthetic is not None, args.features is not None, args.real is not None or args.fake is not None]
    if sum(modes) != 1:
        ap.error("give exactly one of --synthetic, --features, --real/--fake")
    images = args.real is not None or args.fake is not None
    if args.inception and not images:
        ap.error("--inception reads images: it goes with --real / --fake")
    if images and not (args.real and args.fake and (args.clip or args.inception)):
        ap.error("--real and --fake go together, with --clip and / or --inception")
    if args.compare_host and images and not args.clip:
        ap.error("--compare-host compares the top-level numbers: give --clip, --features or --synthetic")
    return args


def main(argv=None):
    args = parse_args(argv)
    from commonscenes_amd import clip as K, fid
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    kid_kw = dict(num_subsets=args.kid_subsets, max_subset_size=args.kid_subset_size, seed=args.seed)
    f1 = f2 = incep = None
    if args.synthetic is not None:
        f1, f2 = (torch.from_numpy(f).to(dev) for f in synthetic_features(*args.synthetic))
    elif args.features is not None:
        f1, f2 = (fid.features_of(p, None, "all", args.batch, "fid_table") for p in args.features)
    else:
        if args.clip:
            if args.clip == "synthetic":
                model = K.CLIP(dev).load_state_dict(K.synth_clip_state_dict({"vision": K.VIT_B_32["vision"]}, 7))
            else:
                model = K.load_checkpoint(args.clip, dev)
            f1 = fid.features_of(args.real, model, args.room, args.batch, "fid_table")
            f2 = fid.features_of(args.fake, model, args.room, args.batch, "fid_table")
        if args.inception:
            incep = inception_block(args, dev, kid_kw)
    rec = dict(kid_subsets=args.kid_subsets, seed=args.seed)
    if f1 is not None:
        n1, n2, d = int(f1.shape[0]), int(f2.shape[0]), int(f1.shape[1])
        route = fid.pick_route(n1, n2, d)
        rec = dict(fid=fid.frechet_distance(f1, f2), kid=fid.kernel_distance(f1, f2, **kid_kw), n_real=n1, n_fake=n2, d=d,
                   route=route, kid_subsets=args.kid_subsets, kid_subset_size=min(n1, n2, args.kid_subset_size), seed=args.seed)
    if incep is not None:
        rec["inception"] = incep
    if args.compare_host:
        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            v = fn()
            torch.cuda.synchronize()
            return v, time.perf_counter() - t0
        _, t_fid = timed(lambda: fid.frechet_distance(f1, f2))
        _, t_kid = timed(lambda: fid.kernel_distance(f1, f2, **kid_kw))
        h1, h2 = f1.cpu().numpy(), f2.cpu().numpy()
        hf, th_fid = timed(lambda: host_fid(h1, h2, route))
        if args.seed is not None:
            np.random.seed(args.seed)
        hk, th_kid = timed(lambda: host_kid(h1, h2, args.kid_subsets, args.kid_subset_size))
        rec.update(host_fid=hf, host_kid=hk, device_fid_seconds=t_fid, device_kid_seconds=t_kid, host_fid_seconds=th_fid,
                   host_kid_seconds=th_kid, host_threads=torch.get_num_threads())
    print("FID_TABLE " + json.dumps(rec))
    return rec


if __name__ == "__main__":
    main()
