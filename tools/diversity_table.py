#!/usr/bin/env python
"""The two evaluation tables of commonscenes_amd/diversity.py from the command line.

    python tools/diversity_table.py --synthetic [--scenes 2] [--samples 3] [--width 32] [--ddim-steps 2] [--objects N]
                                    [--points 5000] [--compare-host]
        the diversity block of scripts/eval_3dfront.py (--evaluate_diversity, :577-762) on the synthetic experiment of
        tools/eval_walkthrough.py: every scene's K runs as one coalesced sampler call, then DiversityMeter.  Prints one
        `DIVERSITY_TABLE {...}` JSON line.  --compare-host also pushes the SAME SDFs through the host route -- the functions
        tools/eval_walkthrough.py:47-60 uses: clouds copied to the CPU, normalised in numpy, one Chamfer call per pair -- and
        prints its numbers and both wall times (second call each), plus the two device launches' own times.

    python tools/diversity_table.py --consistency FILE.json --meshes DIR [--mapping FILE.json] [--points 5000] [--seed 47]
                                    [--images DIR --clip {MODEL.pt | synthetic} [--time-batch N]]
        scripts/consistency_check.py: its Chamfer half (:68-101) and, with --images, its CLIP half (:58-66, :82-90).  FILE.json is what
        scripts/collect_consistency.py:284-300 writes: {"scans": [{"scan": name, "objects": {id: class name},
        "consistency": [[id, id, ...], ...]}]}; --mapping maps the fine class names to the coarse ones, as the script does
        for the small vocabulary.  Meshes are DIR/<scan>/<name>_<classid>_<id>.obj; the class id is whatever the exporter
        wrote (the file is found by name and instance id).  Vertices are read from the `v` lines as they stand:
        trimesh.load, which the script uses, also merges duplicate vertices, this reader does not.  Prints one
        `CONSISTENCY_TABLE {...}` JSON line.
        --images DIR adds a `clip` block to that line: the rendered views DIR/<scan>/<name>_<classid>_<id>.png
        (object_views.py writes them; found by name and instance id like the meshes) go through CLIP's preprocess and
        commonscenes_amd.clip.CLIP.encode_image, and every pair's ||f_a - f_b|| is averaged per category and in total
        (diversity.clip_consistency_table).  --clip MODEL.pt is OpenAI's ViT-B-32.pt (torch.jit.load, else torch.load);
        --clip synthetic takes ViT-B/32 shapes with clip.synth_clip_state_dict weights, vision tower only (the figures then
        mean nothing; the route is the same).  The reference runs CLIP in fp16, this is an fp32 forward: tables agree to the
        low digits, not per bit.  --time-batch N also reports (never gates on) the time of one encode_image call on N
        random images, second call, device events.  Without --images the output is what it was.
"""
import argparse
import json
import os
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")


def synthetic_classes():
    """the walkthrough's synthetic vocabulary read as SG-FRONT's: class 0 is `_scene_`, the last one `floor`
    (synth.random_scene_graph), and the ten table categories are classes 1..10"""
    from commonscenes_amd.diversity import CATEGORIES
    return {"_scene_": 0, "floor": 34, **{n: i for i, n in enumerate(CATEGORIES, start=1)}}


def sample_runs(model, data, samples, ddim_steps):
    """one scene's K runs as ONE coalesced call -> (scene arguments, K box tensors, K angle score tensors, K SDF batches)"""
    d = data["decoder"]
    scene = dict(dec_objs=d["objs"].cuda(), dec_triplets=d["tripltes"].cuda(), dec_sdfs=d["sdfs"],
                 encoded_dec_text_feat=d["text_feats"].cuda(), encoded_dec_rel_feat=d["rel_feats"].cuda())
    with torch.no_grad():
        outs = model.sample_box_and_shape_many([dict(scene) for _ in range(samples)], gen_shape=True, ddim_steps=ddim_steps)
    nodes = torch.unique(torch.where(torch.ne(d["sdfs"], torch.zeros_like(d["sdfs"][0])))[0]).tolist()
    return scene, [o[0][0] for o in outs], [o[0][1] for o in outs], [o[1] for o in outs], nodes


def device_route(runs, points, seed):
    from commonscenes_amd.diversity import DiversityMeter
    meter = DiversityMeter(synthetic_classes(), points=points)
    torch.manual_seed(seed)
    for scene, boxes, angles, sdfs, nodes in runs:
        meter.add_scene(scene["dec_objs"], boxes, angles, sdfs, shape_nodes=nodes)
    return meter.summary()


def host_route(runs, points, seed):
    """tools/eval_walkthrough.py:311-343 on the same SDFs (its figures: plain std of normalised boxes and of the angles)"""
    import eval_walkthrough as W
    from commonscenes_amd.chamfer import chamferDist
    from commonscenes_amd.mesh import sdf_to_mesh
    chamfer = chamferDist()
    torch.manual_seed(seed)
    all_boxes, all_angles, all_chamfer = [], [], []
    for scene, boxes, angles, sdfs, _ in runs:
        shapes_sample, angle_div = [], []
        for k, sdf in enumerate(sdfs):
            pts = W.sample_points(sdf_to_mesh(sdf, render_all=True).verts_list(), points)
            shapes_sample.append(torch.stack([torch.from_numpy(W.normalize(p.cpu().numpy())).cuda() for p in pts]))
            angle_div.append(np.expand_dims(np.argmax(angles[k].cpu().numpy(), 1), 1) / 24.0 * 360.0)
        all_boxes += torch.std(torch.stack(boxes, 1), dim=1).cpu().numpy().tolist()
        all_angles += np.stack(angle_div, 1).std(axis=1).reshape(-1).tolist()
        ss = torch.stack(shapes_sample, 1)
        for sid in range(len(ss)):
            seq = []
            for k in range(ss.shape[1] - 1):
                d1, d2 = chamfer(ss[sid, k:k + 1].float(), ss[sid, k + 1:k + 2].float())
                seq.append(float((torch.mean(d1) + torch.mean(d2)).cpu()))
            all_chamfer.append(float(np.mean(seq)))
    return dict(objects=len(all_chamfer), shape=float(np.mean(all_chamfer)), box_std_mean=float(np.mean(all_boxes)),
                angle_std_mean=float(np.mean(all_angles)))


def launch_times(runs, points):
    """the two launches on their own (device events, second call): all clouds of the first scene"""
    from commonscenes_amd import diversity as D, ops
    from commonscenes_amd.mesh import sdf_to_mesh
    _, _, _, sdfs, _ = runs[0]
    K, S = len(sdfs), int(sdfs[0].shape[0])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    verts = sdf_to_mesh(torch.cat(sdfs), render_all=True).verts_list()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    counts = [int(v.shape[0]) for v in verts]
    packed, first = D._packed(verts, counts)
    idx = D.draw_indices(counts, points)                         # the reference's draws, on the CPU: both routes pay them
    t2 = time.perf_counter()
    shared = dict(mesh_ms=(t1 - t0) * 1e3, draw_indices_ms=(t2 - t1) * 1e3, mean_vertices=float(np.mean(counts)))
    idx = idx.to(torch.int32).cuda()
    base = np.arange(S)[:, None] + S * np.arange(K - 1)[None, :]
    pairs = torch.as_tensor(np.stack([base, base + S], -1).reshape(-1, 2), dtype=torch.int32).cuda()
    out = {}
    for _ in range(2):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        clouds = ops.cloud_resample(packed, first, counts, points, idx=idx, normalize=True, check_indices=False)
        ev[1].record()
        ops.chamfer_pairlist(clouds, pairs, check_indices=False)
        ev[2].record()
        torch.cuda.synchronize()
        out = dict(clouds=len(counts), pairs=int(pairs.shape[0]), resample_ms=ev[0].elapsed_time(ev[1]),
                   chamfer_ms=ev[1].elapsed_time(ev[2]), **shared)
    return out


def run_synthetic(a):
    import eval_walkthrough as W
    from commonscenes_amd.vae import VAE
    torch.cuda.set_device(0)
    torch.manual_seed(48)
    np.random.seed(48)
    res = dict(width=a.width, ddim_steps=a.ddim_steps, scenes=a.scenes, samples=a.samples, points=a.points)
    with tempfile.TemporaryDirectory() as td:
        tmp = Path(td)
        opt = W.build_experiment(tmp, a.width)
        model = VAE(type="v2_full", diff_opt=opt, vocab=W.VOCAB, replace_latent=True, with_changes=True, residual=True,
                    with_angles=True, clip=True, with_E2=True)
        model.load_networks(str(tmp), 100)
        model.compute_statistics(str(tmp), 100, W.synthetic_loader(3, seed=900))
        model.eval()
        t0 = time.perf_counter()
        runs = [sample_runs(model, data, a.samples, a.ddim_steps)
                for data in W.synthetic_loader(a.scenes, seed=500, objects=a.objects)]
        torch.cuda.synchronize()
        res["sample_s"] = time.perf_counter() - t0
        res["launch_sizes"] = list(model.vae_v2.Diff.last_launch_sizes)
    res["nodes"] = [int(r[0]["dec_objs"].shape[0]) for r in runs]
    routes = [("device", device_route)] + ([("host", host_route)] if a.compare_host else [])
    for name, fn in routes:
        for tag in ("first_call_s", "wall_s"):                   # the second call is the figure: the first loads code objects
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            table = fn(runs, a.points, 47)
            torch.cuda.synchronize()
            res[f"{name}_{tag}"] = time.perf_counter() - t0
        if name == "device":
            res["table"] = table
        else:
            res["host_table"] = table
    if a.compare_host:
        res["launches"] = launch_times(runs, a.points)
    print("DIVERSITY_TABLE " + json.dumps(res), flush=True)


_CLIP_MODELS = {}


def clip_model(spec):
    """--clip: 'synthetic' (ViT-B/32 shapes, synthetic weights, vision tower only) or a checkpoint path; built once"""
    from commonscenes_amd import clip as K
    if spec not in _CLIP_MODELS:
        if spec == "synthetic":
            sd = K.synth_clip_state_dict({"vision": K.VIT_B_32["vision"]}, 0)
            _CLIP_MODELS[spec] = K.CLIP("cuda").load_state_dict(sd)
        else:
            _CLIP_MODELS[spec] = K.load_checkpoint(spec, "cuda")
    return _CLIP_MODELS[spec]


def clip_block(a, image_files, pairs, cats):
    from commonscenes_amd import clip as K
    from commonscenes_amd.diversity import clip_consistency_table
    model = clip_model(a.clip)
    if model.vision is None:
        raise SystemExit(f"--clip {a.clip}: no vision tower in the checkpoint")
    size = model.vision.resolution
    feats = [model.encode_image(K.preprocess(image_files[i:i + 64], size)) for i in range(0, len(image_files), 64)]
    feats = torch.cat(feats) if feats else torch.zeros((1, 1), device="cuda")          # (no pairs: only the empty total row)
    block = dict(model=a.clip, images=len(image_files), resolution=size, table=clip_consistency_table(feats, pairs, cats))
    if a.time_batch:
        batch = torch.from_numpy(np.random.default_rng(0).integers(0, 256, size=(a.time_batch, size, size, 3), dtype=np.uint8))
        batch = batch.cuda()
        for _ in range(2):                                       # the second call is the figure
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            model.encode_image(batch)
            e1.record()
            torch.cuda.synchronize()
            block["encode_image_ms"], block["time_batch"] = e0.elapsed_time(e1), a.time_batch
    return block


def run_consistency(a):
    from commonscenes_amd.diversity import consistency_from_meshes, read_obj_vertices
    with open(a.consistency) as fh:
        cons = json.load(fh)
    mapping = None
    if a.mapping:
        with open(a.mapping) as fh:
            mapping = json.load(fh)
    name_of = lambda n: mapping[n] if mapping is not None else n
    verts, where, pairs, cats, image_files = [], {}, [], [], []

    def cloud(scan, name, oid):
        key = (scan, str(oid))
        if key not in where:
            found = sorted((Path(a.meshes) / scan).glob(f"{name}_*_{oid}.obj"))
            if len(found) != 1:
                raise SystemExit(f"{scan}: expected one mesh {name}_<classid>_{oid}.obj, found {len(found)}")
            if a.images:                                         # consistency_check.py:58-59: the same stem, .png
                img = sorted((Path(a.images) / scan).glob(f"{name}_*_{oid}.png"))
                if len(img) != 1:
                    raise SystemExit(f"{scan}: expected one image {name}_<classid>_{oid}.png, found {len(img)}")
                image_files.append(img[0])
            where[key] = len(verts)
            verts.append(read_obj_vertices(found[0]))
        return where[key]

    for scan in cons["scans"]:
        for triplet in scan.get("consistency") or []:
            sub_id, obj_id = triplet[0], triplet[1]
            sub, obj = name_of(scan["objects"][str(sub_id)]), name_of(scan["objects"][str(obj_id)])
            if sub != obj:
                raise SystemExit(f"{scan['scan']}: objects {sub_id} ({sub}) and {obj_id} ({obj}) are marked the same")
            pairs.append((cloud(scan["scan"], sub, sub_id), cloud(scan["scan"], obj, obj_id)))
            cats.append(sub)
    table = consistency_from_meshes(verts, pairs, cats, points=a.points, seed=a.seed)
    res = dict(meshes=len(verts), points=a.points, seed=a.seed, table=table)
    if a.images:
        res["clip"] = clip_block(a, image_files, pairs, cats)
    print("CONSISTENCY_TABLE " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--synthetic", action="store_true", help="the diversity table on the walkthrough's synthetic experiment")
    ap.add_argument("--scenes", type=int, default=2)
    ap.add_argument("--samples", type=int, default=3, help="runs per scene (eval_3dfront.py num_samples)")
    ap.add_argument("--width", type=int, default=32, help="UNet model_channels (224 = the shipped network)")
    ap.add_argument("--ddim-steps", type=int, default=2)
    ap.add_argument("--objects", type=int, default=None, help="shaped objects per scene (default 4, 5, ...)")
    ap.add_argument("--points", type=int, default=5000)
    ap.add_argument("--compare-host", action="store_true",
                    help="also run the host route (numpy normalisation, one Chamfer call per pair) on the same SDFs")
    ap.add_argument("--consistency", metavar="FILE.json", help="the ground truth's `same as` pairs (collect_consistency.py)")
    ap.add_argument("--meshes", metavar="DIR", help="DIR/<scan>/<name>_<classid>_<id>.obj; only the `v` lines are read -- "
                    "trimesh.load merges duplicate vertices, this reader does not")
    ap.add_argument("--mapping", metavar="FILE.json", default=None, help="fine -> coarse class names (mapping_no_stool.json)")
    ap.add_argument("--seed", type=int, default=47)
    ap.add_argument("--images", metavar="DIR", default=None, help="DIR/<scan>/<name>_<classid>_<id>.png: adds the CLIP half "
                    "(consistency_check.py:58-66, :82-90) as a `clip` block; needs --clip")
    ap.add_argument("--clip", metavar="MODEL.pt|synthetic", default=None, help="OpenAI's ViT-B-32.pt, or `synthetic`: ViT-B/32 "
                    "shapes with synthetic weights (vision tower only)")
    ap.add_argument("--time-batch", type=int, default=0, help="also report the time of encode_image on N random images")
    a = ap.parse_args()
    if a.synthetic == bool(a.consistency):
        ap.error("give --synthetic or --consistency FILE.json")
    if a.consistency and not a.meshes:
        ap.error("--consistency needs --meshes DIR")
    if bool(a.images) != bool(a.clip) or (a.images and not a.consistency):
        ap.error("--images DIR and --clip MODEL go together, with --consistency")
    if a.synthetic and a.samples < 2:
        ap.error("diversity needs at least two runs per object")
    run_synthetic(a) if a.synthetic else run_consistency(a)


if __name__ == "__main__":
    main()
