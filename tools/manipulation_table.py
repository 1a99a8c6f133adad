#!/usr/bin/env python
"""The scene-manipulation experiment (scripts/eval_3dfront.py:206-441, `validate_constrains_loop_w_changes`) on a synthetic
SG-FRONT-like dataset through this package only: graph edits (commonscenes_amd.manipulation.make_edit), the 1 + K decodes per
scene, the three accuracy tables and the changed-node diversity block.

    python tools/manipulation_table.py --synthetic --mode {relationship,addition} [--scenes 3] [--samples 3] [--width 32]
        [--ddim-steps 2] [--batch-scenes 1] [--shape-nodes all|changed] [--points 5000] [--export-scenes DIR]
        [--compare-sequential]

prints one `MANIPULATION_TABLE {...}` JSON line.  --export-scenes additionally runs the before / after editing workflow
(scripts/eval_3dfront_manivis.py:298-380, manipulation.edit_scene) per scene and writes <scan>_before.obj / .png and
<scan>_after_<label>.obj / .png.  --compare-sequential times the coalesced loop (--batch-scenes, default all scenes) against
the scene-by-scene loop, interleaved in one process, three repeats after an untimed pass; timings are report-only."""
import argparse
import importlib.util
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
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")


def _walkthrough():
    spec = importlib.util.spec_from_file_location("eval_walkthrough", ROOT / "tools" / "eval_walkthrough.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def synthetic_names(W):
    """the synthetic vocabulary read as SG-FRONT's: class 0 `_scene_`, the last class `floor`, the ten diversity categories
    1..10; predicate 0 the `in` edge, 1..15 SG-FRONT's relationship list"""
    from commonscenes_amd.diversity import CATEGORIES
    from commonscenes_amd.manipulation import SGFRONT_RELATIONSHIPS
    n = len(W.VOCAB["object_idx_to_name"])
    classes = {"_scene_": 0, "floor": n - 1, **{c: i for i, c in enumerate(CATEGORIES, start=1)}}
    for i in range(len(CATEGORIES) + 1, n - 1):
        classes[f"obj{i}"] = i
    names = [None] * n
    for k, v in classes.items():
        names[v] = k + "\n"
    rels = list(SGFRONT_RELATIONSHIPS)
    eval_vocab = dict(pred_idx_to_name=["in\n"] + [r + "\n" for r in rels])
    return classes, names, rels, eval_vocab


def synthetic_edits(W, n_scenes, mode, classes, rels, seed=500, objects=None, edit_seed=48):
    """one make_edit per synthetic scene (None where the edit found nothing to change), numpy's RNG seeded once"""
    from commonscenes_amd import synth
    from commonscenes_amd.manipulation import graph_lists, make_edit
    classes_r = {v: k for k, v in classes.items()}
    feat = lambda words: synth.gaussian_like(f"mt:{words}", (512,), scale=10.0 / float(np.sqrt(512.0)))
    np.random.seed(edit_seed)
    torch.manual_seed(edit_seed)                       # the synthetic loader draws its box angles from torch's RNG
    out = []
    for data in W.synthetic_loader(n_scenes, seed=seed, objects=objects):
        d = data["decoder"]
        scene = graph_lists(d["objs"], d["tripltes"], d["boxes"], d["text_feats"], d["rel_feats"], classes_r, rels,
                            sdfs=d["sdfs"], scan_id=data["scan_id"][0])
        out.append(make_edit(scene, mode, classes, rels, rel_feat_fn=feat))
    return out


def build_model(W, tmp: Path, width: int):
    from commonscenes_amd.vae import VAE
    opt = W.build_experiment(tmp, width)
    model = VAE(type="v2_full", diff_opt=opt, vocab=W.VOCAB, replace_latent=True, with_changes=True, residual=True,
                with_angles=True, clip=True, with_E2=True)
    model.load_networks(str(tmp), 100)
    model.compute_statistics(str(tmp), 100, W.synthetic_loader(3, seed=900))
    return model.eval()


def export_edit(out_dir, model, edit, names, ddim_steps, shape_nodes, seed, render_type="generated", render_boxes=False,
                library=None):
    """<scan>_before.obj / .png and <scan>_after_<label>.obj / .png (.npy without PIL).  render_type retrieval / library /
    onlybox fills the edited layout from the mesh library instead of the generated shapes (scene_mesh.
    assemble_scene_from_library); render_boxes adds the tube markers."""
    import random
    from commonscenes_amd import manipulation as MP, scene_mesh as S
    out = Path(out_dir)
    out.mkdir(parents=True, exist_ok=True)
    g = torch.Generator().manual_seed(seed)
    noise = lambda: torch.randn((1, 3, 16, 16, 16), generator=g)
    np.random.seed(seed)
    res = MP.edit_scene(model, None, edit, ddim_steps=ddim_steps, shape_nodes=shape_nodes, x_T_before=noise(),
                        x_T_after=noise())
    scan = edit["scan_id"][0]
    label = names[res["after"][2][res["changed"][0]]].strip() if res["changed"] else "none"
    files = []
    for tag, (meshes, boxes, cats) in (("before", res["before"]), (f"after_{label}", res["after"])):
        if render_type == "generated":
            scene = S.assemble_scene(meshes, boxes, cats, names, floor=True, render_boxes=render_boxes)
        else:
            scene = S.assemble_scene_from_library(render_type, boxes, cats, names, library=library, render_boxes=render_boxes,
                                                  floor=True, rng=random.Random(seed))
        img = S.render_topdown(scene, 256)
        scene.export_obj(out / f"{scan}_{tag}.obj")
        rgb = img["rgb"].cpu().numpy()
        try:
            from PIL import Image
            Image.fromarray(rgb).save(out / f"{scan}_{tag}.png")
            image = f"{scan}_{tag}.png"
        except ImportError:
            np.save(out / f"{scan}_{tag}.npy", rgb)
            image = f"{scan}_{tag}.npy"
        files += [f"{scan}_{tag}.obj", image]
    return dict(scan=scan, label=label, changed=res["changed"], files=files)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--synthetic", action="store_true", help="the synthetic dataset (the only one reachable offline)")
    ap.add_argument("--mode", choices=["relationship", "addition"], required=True)
    ap.add_argument("--scenes", type=int, default=3)
    ap.add_argument("--samples", type=int, default=3, help="diversity decodes per scene (eval_3dfront.py num_samples)")
    ap.add_argument("--width", type=int, default=32, help="UNet model_channels (224 = the shipped network)")
    ap.add_argument("--ddim-steps", type=int, default=2)
    ap.add_argument("--batch-scenes", type=int, default=1)
    ap.add_argument("--shape-nodes", choices=["all", "changed"], default="all")
    ap.add_argument("--points", type=int, default=5000)
    ap.add_argument("--objects", type=int, default=None, help="shaped objects per scene (default 4, 5, ...)")
    ap.add_argument("--export-scenes", metavar="DIR", default=None)
    ap.add_argument("--render-type", choices=["generated", "retrieval", "library", "onlybox"], default="generated",
                    help="with --export-scenes: what fills the boxes of the before / after scenes (default: the generated shapes)")
    ap.add_argument("--render-boxes", action="store_true", help="with --export-scenes: add tube markers along the box edges")
    ap.add_argument("--library", nargs="+", metavar="SPEC", default=None,
                    help="the mesh library of --render-type retrieval / library: `synthetic`, `JSON MODEL_ROOT` or `DIR`")
    ap.add_argument("--compare-sequential", action="store_true")
    a = ap.parse_args()
    if not a.synthetic:
        ap.error("only --synthetic is available: the real dataset and its CLIP features are not reachable offline")
    if (a.render_type != "generated" or a.render_boxes) and not a.export_scenes:
        ap.error("--render-type / --render-boxes need --export-scenes DIR")
    torch.cuda.set_device(0)
    from commonscenes_amd import manipulation as MP
    W = _walkthrough()
    classes, names, rels, eval_vocab = synthetic_names(W)
    res = dict(mode=a.mode, scenes=a.scenes, samples=a.samples, width=a.width, ddim_steps=a.ddim_steps,
               batch_scenes=a.batch_scenes, shape_nodes=a.shape_nodes, points=a.points)
    with tempfile.TemporaryDirectory() as td:
        model = build_model(W, Path(td), a.width)
        edits = synthetic_edits(W, a.scenes, a.mode, classes, rels, objects=a.objects)

        def loop(batch_scenes):
            np.random.seed(48)                                                     # eval_3dfront.py:62-63
            meter = MP.ManipulationMeter(eval_vocab, classes, points=a.points)
            out = MP.manipulation_loop(model, edits, a.mode, num_samples=a.samples, gen_shape=True, ddim_steps=a.ddim_steps,
                                       batch_scenes=batch_scenes, shape_nodes=a.shape_nodes, meter=meter,
                                       noise_generator=torch.Generator().manual_seed(48),
                                       points_generator=torch.Generator().manual_seed(48))
            torch.cuda.synchronize()
            return out, list(model.vae_v2.Diff.last_launch_sizes)

        t0 = time.perf_counter()
        out, launches = loop(a.batch_scenes)
        res.update(out, loop_s=time.perf_counter() - t0, last_launch_sizes=launches)
        if a.compare_sequential:
            wide = a.batch_scenes if a.batch_scenes > 1 else max(a.scenes, 2)
            loop(wide), loop(1)                                                    # untimed pass
            t_c, t_s = [], []
            for _ in range(3):
                t0 = time.perf_counter(); oc, lc = loop(wide); t_c.append(time.perf_counter() - t0)
                t0 = time.perf_counter(); os_, _ = loop(1); t_s.append(time.perf_counter() - t0)
            res["compare_sequential"] = dict(
                batch_scenes=wide, coalesced_s=t_c, sequential_s=t_s, coalesced_median_s=float(np.median(t_c)),
                sequential_median_s=float(np.median(t_s)), speedup=float(np.median(t_s) / np.median(t_c)),
                launch_sizes_coalesced=lc, tables_equal=oc["tables"] == os_["tables"],
                note="whole loop (encode, 1 + K decodes per scene, meshing, resampling, Chamfer, tables): one `_many` call "
                     "per batch of scenes vs one facade call per decode; report-only")
        if a.export_scenes:
            library = W.open_library(a.library, a.render_type, names, Path(td))
            res["export"] = [export_edit(a.export_scenes, model, e, names, a.ddim_steps, a.shape_nodes, 48 + i,
                                         a.render_type, a.render_boxes, library)
                             for i, e in enumerate(edits) if e is not None]
            if a.render_type != "generated" or a.render_boxes:
                res["export_render"] = dict(render_type=a.render_type, render_boxes=a.render_boxes)
    print("MANIPULATION_TABLE " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
