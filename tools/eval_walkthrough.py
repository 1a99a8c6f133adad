#!/usr/bin/env python
"""BASELINE configs[4] (C5) exerciser: the call sequence of scripts/eval_3dfront.py:484-722 for the v2_full model with
--gen_shape True --visualize / --evaluate_diversity, on a synthetic SG-FRONT-like dataset (the real dataset, CLIP
features and trained checkpoints are not reachable offline), through this package only:

    VAE(type='v2_full', ...).load_networks / compute_statistics           scripts/eval_3dfront.py:150-175
    for each scene of the test loader                                      :484-510
        boxes, shapes = model.sample_box_and_shape(..., gen_shape=True)    :513
        angles = -180 + (argmax + 1) * 15                                  :514-516
        meshes  = sdf_to_mesh(shapes, render_all=True)                     helpers/util.py:298 (--visualize)
        diversity: num_samples x [sample_box_and_shape -> sdf_to_mesh -> verts_list -> sample_points(5000)
                   -> normalize]; chamfer(shape_k, shape_k+1)              :577-690
    box / angle / shape diversity summaries                                :660-690

Under `torch.distributed.run` (one process per GPU) every rank runs the same script and rel2shape shards the objects
over the ranks (one broadcast in, one all-gather out) -- the 8xMI355X form of C5.  `--attention f16` selects the opt-in
"fp16 MFMA attention" C5 names (reduced precision; the default is the fp32-grade F16X3 attention).

    python tools/eval_walkthrough.py [--scenes 2] [--samples 3] [--width 32] [--ddim-steps 2] [--attention f16]
prints one JSON line (rank 0)."""
import argparse
import json
import os
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch
import yaml

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

VOCAB = dict(object_idx_to_name=[f"obj{i}\n" for i in range(35)], pred_idx_to_name=[f"pred{i}\n" for i in range(16)],
             object_idx_to_name_grained=[f"objg{i}\n" for i in range(35)])
# --constraints: what the synthetic predicates stand for in the evaluation ONLY (the model keeps pred0..pred15): predicate 0 is
# synth.random_scene_graph's `in` edge, 1..11 the eleven relations helpers/metrics_3dfront.py:74-165 evaluates, the rest are
# relations it does not evaluate
EVAL_PREDICATES = ["in", "left", "right", "front", "behind", "bigger than", "smaller than", "taller than", "shorter than",
                   "standing on", "close by", "symmetrical to", "inside", "attached to", "part of", "cover"]
EVAL_VOCAB = dict(pred_idx_to_name=[p + "\n" for p in EVAL_PREDICATES])


def sample_points(points_list, num):                         # helpers/util.py:31-44
    out = []
    for pc in points_list:
        n = pc.size(0)
        idx = torch.randperm(n)[:num] if n >= num else torch.randint(n, size=(num,))
        out.append(pc[idx.to(pc.device)])
    return out


def normalize(vertices, scale=1):                            # scripts/eval_3dfront.py:783-796
    for a in range(3):
        lo, hi = np.amin(vertices[:, a]), np.amax(vertices[:, a])
        vertices[:, a] += -lo - (hi - lo) * 0.5
    return vertices / np.max(vertices, axis=0) * scale


def synthetic_loader(n_scenes, seed, objects=None):
    """`objects`: shaped objects per scene (default 4, 5, ...).  32 gives an SG-FRONT-livingroom-sized graph: 34 nodes
    (objects + floor + _scene_) and ~160 triples (dataset/threedfront_dataset.py:448-452: an `in` edge from every node
    to `_scene_` plus the typed relations)."""
    from commonscenes_amd import synth
    out = []
    for s in range(n_scenes):
        nobj = (4 + s) if objects is None else objects
        g = synth.random_scene_graph(nobj, seed=seed + s)
        O = g["objs"].shape[0]
        sdfs = torch.zeros(O, 1, 4, 4, 4)
        sdfs[:nobj] = 1.0                                     # floor / _scene_ carry all-zero SDFs
        boxes = torch.cat([synth.gaussian_like(f"ev:{s}", (O, 6)), torch.randint(0, 24, (O, 1)).float()], dim=1)
        out.append({"scan_id": [f"Synthetic-{s}"], "instance_id": [list(range(O))],
                    "decoder": {"objs": g["objs"], "tripltes": g["triples"], "boxes": boxes, "sdfs": sdfs,
                                "text_feats": g["text_feats"], "rel_feats": g["rel_feats"]}})
    return out


def build_experiment(tmp: Path, width: int):
    """an experiment directory in the reference's layout: checkpoint/model{epoch}.pth with synthetic weights."""
    from commonscenes_amd import configs as K
    from commonscenes_amd import synth
    from commonscenes_amd.scene import scene_param_shapes
    from commonscenes_amd.unet import unet_param_shapes
    from commonscenes_amd.vqvae import vqvae_param_shapes
    ucfg = K.reduced(K.UNET_CROSSATTN, width) if width != 224 else dict(K.UNET_CROSSATTN)
    gen = "cuda" if torch.cuda.is_available() else "cpu"      # same values either way (synth.py); the device is faster
    df_yaml = dict(model=dict(params=dict(conditioning_key="crossattn", **K.DIFFUSION)),
                   unet=dict(params={k: (list(v) if isinstance(v, tuple) else v) for k, v in ucfg.items()}))
    vq_yaml = dict(model=dict(params=dict(embed_dim=K.VQVAE_EMBED_DIM, n_embed=K.VQVAE_N_EMBED,
                                          ddconfig={k: (list(v) if isinstance(v, tuple) else v)
                                                    for k, v in K.VQVAE_DDCONFIG.items()})))
    (tmp / "df.yaml").write_text(yaml.safe_dump(df_yaml))
    (tmp / "vq.yaml").write_text(yaml.safe_dump(vq_yaml))
    opt = dict(hyper=dict(device="cuda", batch_size=4),
               network=dict(df_cfg=str(tmp / "df.yaml"), vq_cfg=str(tmp / "vq.yaml"), vq_ckpt=None), misc=dict(seed=111))
    cpu = lambda sd: {k: v.cpu() for k, v in sd.items()}
    ck = dict(synth.synth_state_dict(scene_param_shapes(35, 16)))
    ck["vqvae"] = synth.synth_state_dict(vqvae_param_shapes(K.VQVAE_DDCONFIG, K.VQVAE_N_EMBED, K.VQVAE_EMBED_DIM))
    ck["df"] = cpu(synth.synth_state_dict(unet_param_shapes(ucfg), device=gen))
    ck.update(opt={}, epoch=100, counter=0)
    (tmp / "checkpoint").mkdir(exist_ok=True)
    torch.save(ck, tmp / "checkpoint" / "model100.pth")
    return opt


def open_library(spec, render_type, classes, tmp):
    """--library: `synthetic` (commonscenes_amd.synth: boxes and ellipsoids per class, nothing on disk but a temporary folder
    for the `library` type), `JSON MODEL_ROOT` (cat_jid_trainval*.json + the 3D-FUTURE model folder) or `DIR` (label folders of
    *.ply / *.obj) -> the FurnitureLibrary (retrieval) or ShapeLibrary (library) the render type needs; None for onlybox"""
    from commonscenes_amd import scene_library as SL, synth
    if render_type in ("generated", "onlybox"):
        return None
    if not spec:
        raise SystemExit(f"--render-type {render_type} needs --library")
    labels = [c for c in classes if c.strip() not in ("_scene_", "floor")]
    if render_type == "retrieval":
        if spec == ["synthetic"]:
            return synth.furniture_library(labels)
        if len(spec) != 2:
            raise SystemExit("--render-type retrieval needs --library synthetic or --library JSON MODEL_ROOT")
        return SL.FurnitureLibrary.from_json(spec[0], spec[1])
    if spec == ["synthetic"]:
        synth.write_shape_library(str(tmp / "shape_library"), labels)
        return SL.ShapeLibrary(tmp / "shape_library")
    if len(spec) != 1:
        raise SystemExit("--render-type library needs --library synthetic or --library DIR")
    return SL.ShapeLibrary(spec[0])


def export_layout_scene(out_dir, scan, render_type, render_boxes, library, boxes_pred, angles_pred, dec_objs):
    """--export-scenes with --render-type retrieval | library | onlybox: the scene from the mesh library (no generated
    shapes: the v2_box use) and its top-down view -> DIR/<scan>.obj, DIR/<scan>.png"""
    import random
    from commonscenes_amd import scene_mesh as S
    out = Path(out_dir)
    out.mkdir(parents=True, exist_ok=True)
    classes = list(VOCAB["object_idx_to_name"])
    classes[0], classes[-1] = "_scene_\n", "floor\n"
    box_and_angle = torch.cat([boxes_pred.float(), angles_pred.float()], dim=1)
    cats = dec_objs.cpu().tolist()
    times = {}
    for tag in ("first_call_s", "device_s"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        scene = S.assemble_scene_from_library(render_type, box_and_angle, cats, classes, library=library,
                                              render_boxes=render_boxes, floor=True, rng=random.Random(48))
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        img = S.render_topdown(scene, 256)
        torch.cuda.synchronize()
        times[tag] = time.perf_counter() - t0
        times["assemble_s"], times["render_s"] = t1 - t0, time.perf_counter() - t1
    scene.export_obj(out / f"{scan}.obj")
    image = _save_image(out, scan, img["rgb"].cpu().numpy())
    return dict(obj=f"{scan}.obj", image=image, verts=int(scene.verts.shape[0]), faces=int(scene.faces.shape[0]),
                dropped=img["dropped"], covered=int((img["object_id"] >= 0).sum()), render_type=render_type,
                render_boxes=bool(render_boxes or render_type == "onlybox"),
                sources=[os.path.basename(str(x)) for x in scene.sources], **times)


def _save_image(out, scan, rgb):
    try:
        from PIL import Image
        Image.fromarray(rgb).save(out / f"{scan}.png")
        return f"{scan}.png"
    except ImportError:
        np.save(out / f"{scan}.npy", rgb)
        return f"{scan}.npy"


def export_scene(out_dir, scan, meshes, boxes_pred, angles_pred, dec_objs, render_boxes=False):
    """--export-scenes: the scene mesh and its top-down view, timed on the device (second call: the first loads the code
    objects), and the host numpy restatement of fit_shapes_to_box_v2 over the same meshes for context."""
    from commonscenes_amd import scene_mesh as S
    out = Path(out_dir)
    out.mkdir(parents=True, exist_ok=True)
    classes = list(VOCAB["object_idx_to_name"])
    classes[0], classes[-1] = "_scene_\n", "floor\n"           # synth.random_scene_graph: class 0 / the last class
    box_and_angle = torch.cat([boxes_pred.float(), angles_pred.float()], dim=1)
    cats = dec_objs.cpu().tolist()
    times = {}
    for tag in ("first_call_s", "device_s"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        scene = S.assemble_scene(meshes, box_and_angle, cats, classes, floor=True, render_boxes=render_boxes)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        img = S.render_topdown(scene, 256)
        torch.cuda.synchronize()
        times[tag] = time.perf_counter() - t0
        times["assemble_s"], times["render_s"] = t1 - t0, time.perf_counter() - t1
    t0 = time.perf_counter()                                     # the reference's host path: copy out, fit per object in fp64
    boxes_h = box_and_angle.cpu().numpy()
    shaped = [j for j, c in enumerate(cats) if classes[c].strip() not in ("_scene_", "floor")]
    for j, v in zip(shaped, meshes.verts_list()):
        v = v.cpu().numpy().astype(np.float64)
        if v.shape[0] == 0:
            continue
        l, h, w, px, py, pz, ang = [float(x) for x in boxes_h[j]]
        lo, hi = v.min(axis=0), v.max(axis=0)
        c = lo + (hi - lo) / 2
        c[1] = lo[1]
        v1 = np.stack([-v[:, 2], v[:, 1], v[:, 0]], axis=1) - c[None]
        size = v1.max(axis=0) - v1.min(axis=0)
        y = np.deg2rad(ang)
        rot = np.array([[np.cos(y), 0, -np.sin(y)], [0, 1, 0], [np.sin(y), 0, np.cos(y)]])
        with np.errstate(divide="ignore", invalid="ignore"):
            (v1 / size * np.array([l, h, w])).dot(np.linalg.inv(rot).T) + np.array([px, py, pz])
    times["numpy_fit_s"] = time.perf_counter() - t0
    scene.export_obj(out / f"{scan}.obj")
    image = _save_image(out, scan, img["rgb"].cpu().numpy())
    nv, nf = int(scene.verts.shape[0]), int(scene.faces.shape[0])
    # cs_scene_apply reads 12 B per vertex and 24 B per face, writes 24 B per vertex (position + colour) and 28 B per face
    return dict(obj=f"{scan}.obj", image=image, verts=nv, faces=nf, dropped=img["dropped"],
                covered=int((img["object_id"] >= 0).sum()), apply_bytes=36 * nv + 52 * nf, **times)


def export_object_views(out_dir, scan, meshes, boxes_pred, angles_pred, dec_objs, renderer):
    """--object-views: one normalised 256x256 RGBA view per shaped object -- the raw, inverted, coloured meshes of
    get_generated_models_v2 through helpers/visualize_scene.py:42-55 get_current_visuals_v2 and :29-40 store_current_imgs
    -> DIR/render_object_imgs/<scan>/<label>_<cat>_<instance>.png"""
    from commonscenes_amd import object_views as OV, scene_mesh as S
    img_dir = Path(out_dir) / "render_object_imgs" / str(scan)
    img_dir.mkdir(parents=True, exist_ok=True)
    classes = list(VOCAB["object_idx_to_name"])
    classes[0], classes[-1] = "_scene_\n", "floor\n"
    cats = dec_objs.cpu().tolist()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    raw = S.get_generated_models_v2(torch.cat([boxes_pred.float(), angles_pred.float()], dim=1), meshes, cats, classes)[2]
    visuals = OV.get_current_visuals_v2(VOCAB, renderer, raw, cats)
    t1 = time.perf_counter()
    paths = OV.store_current_imgs(visuals, str(img_dir), classes, cats)
    return len(paths), t1 - t0, time.perf_counter() - t1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=2)
    ap.add_argument("--samples", type=int, default=3, help="diversity runs per scene (eval_3dfront.py num_samples)")
    ap.add_argument("--width", type=int, default=32, help="UNet model_channels (224 = the shipped network)")
    ap.add_argument("--ddim-steps", type=int, default=2)
    ap.add_argument("--attention", choices=["same", "f16"], default="same")
    ap.add_argument("--points", type=int, default=5000)
    ap.add_argument("--objects", type=int, default=None,
                    help="shaped objects per scene (default 4, 5, ...; 32 = a livingroom-sized SG-FRONT graph: 34 nodes)")
    ap.add_argument("--mini-b", type=int, default=None,
                    help="sampler mini-batch (default: the reference's 7, sdfusion_txt2shape_model.py:493)")
    ap.add_argument("--compare-attention", action="store_true",
                    help="additionally sample the first scene once with the default (fp32-grade F16X3) attention and once "
                         "with the fp16 MFMA attention from the SAME z / x_T and report the latent / SDF deviation "
                         "(SURVEY 8d: fp16-attention mode is report-only)")
    ap.add_argument("--batch-scenes", action="store_true",
                    help="additionally time the shape sampling of ALL scenes scene by scene (the reference's loop, "
                         "scripts/eval_3dfront.py:484-513) against ONE coalesced call (VAE.sample_box_and_shape_many: each "
                         "scene's graph and shared x_T kept, one sampler + decode over all scenes' objects), same z / x_T, "
                         "and report the wall times and the per-object latent deviation")
    ap.add_argument("--export-scenes", metavar="DIR", default=None,
                    help="additionally assemble every scene (scene_mesh.assemble_scene with the floor: what render_v2_full "
                         "hands to trimesh.Scene, helpers/visualize_scene.py:401-436) and render its 256x256 top-down view "
                         "(render_img, :85-116); writes DIR/<scan>.obj and DIR/<scan>.png (.npy without PIL) and reports the "
                         "device time next to a host numpy restatement of the fit (helpers/util.py:158-189)")
    ap.add_argument("--render-type", choices=["generated", "retrieval", "library", "onlybox"], default="generated",
                    help="with --export-scenes DIR: what fills the boxes (helpers/visualize_scene.py:208-461): the generated shapes "
                         "(default), the closest model of a furniture library, a drawn shape of a shape library, or tube "
                         "markers only.  With retrieval / library / onlybox the shape branch is not sampled (the v2_box use) "
                         "and only the layout scenes are exported")
    ap.add_argument("--render-boxes", action="store_true",
                    help="with --export-scenes DIR: add tube markers along the box edges (helpers/util.py:393-421)")
    ap.add_argument("--library", nargs="+", metavar="SPEC", default=None,
                    help="the mesh library of --render-type retrieval / library: `synthetic`, `JSON MODEL_ROOT` "
                         "(cat_jid_trainval*.json and the model folder; retrieval) or `DIR` (label folders of *.ply; library)")
    ap.add_argument("--object-views", action="store_true",
                    help="with --export-scenes DIR: additionally render every shaped object on its own (object_views: the "
                         "reference's init_mesh_renderer(256, 1.7, 20, 20) + get_current_visuals_v2) and write "
                         "DIR/render_object_imgs/<scan>/<label>_<cat>_<instance>.png; reports the image count and time")
    ap.add_argument("--constraints", action="store_true",
                    help="additionally evaluate every scene's sampled boxes against its graph (constraints.validate_constrains: "
                         "scripts/eval_3dfront.py:722 -> helpers/metrics_3dfront.py:57-179) and report the accuracy table")
    ap.add_argument("--diversity-gpu", action="store_true",
                    help="additionally feed every scene's diversity runs to commonscenes_amd.diversity.DiversityMeter (the "
                         "reference's figures: denormalised boxes, circular angle deviation, per-category table; resampling, "
                         "normalisation and all Chamfer pairs on the device) and report its summary as `diversity`")
    a = ap.parse_args()
    if a.object_views and not a.export_scenes:
        ap.error("--object-views needs --export-scenes DIR")
    if (a.render_type != "generated" or a.render_boxes) and not a.export_scenes:
        ap.error("--render-type / --render-boxes need --export-scenes DIR")
    if a.render_type != "generated" and a.object_views:
        ap.error("--object-views renders generated shapes: not with --render-type " + a.render_type)
    if a.diversity_gpu and a.samples < 2:
        ap.error("--diversity-gpu needs at least two runs per object (--samples)")

    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    one = os.environ.get("CS_ONE_DEVICE") == "1"
    torch.cuda.set_device(0 if one else int(os.environ.get("LOCAL_RANK", "0")))
    if world > 1:
        torch.distributed.init_process_group(os.environ.get("CS_DIST_BACKEND", "gloo" if one else "nccl"))
    torch.manual_seed(48)                                     # eval_3dfront.py:62-63
    np.random.seed(48)

    from commonscenes_amd.chamfer import chamferDist
    from commonscenes_amd.mesh import sdf_to_mesh
    from commonscenes_amd.vae import VAE
    chamfer = chamferDist()
    res = dict(scenes=[], world=world, attention=a.attention, width=a.width, ddim_steps=a.ddim_steps,
               mini_B=a.mini_b or 7)
    with tempfile.TemporaryDirectory() as td:
        tmp = Path(td)
        opt = build_experiment(tmp, a.width)
        model = VAE(type="v2_full", diff_opt=opt, vocab=VOCAB, replace_latent=True, with_changes=True, residual=True,
                    with_angles=True, clip=True, with_E2=True)
        model.load_networks(str(tmp), 100)
        if a.mini_b:
            model.vae_v2.Diff.mini_B = a.mini_b
        if a.attention == "f16":
            model.vae_v2.Diff.df.set_attention_math("f16")
        model.compute_statistics(str(tmp), 100, synthetic_loader(3, seed=900))
        model.eval()
        loader = synthetic_loader(a.scenes, seed=500, objects=a.objects)
        if a.render_type != "generated":                      # layout only: boxes and angles, no sampler step
            classes = list(VOCAB["object_idx_to_name"])
            classes[0], classes[-1] = "_scene_\n", "floor\n"
            library = open_library(a.library, a.render_type, classes, tmp)
            calls = [0]
            rel2shape = model.vae_v2.Diff.rel2shape

            def counted(*args, **kw):
                calls[0] += 1
                return rel2shape(*args, **kw)
            model.vae_v2.Diff.rel2shape = counted
            t_all = time.perf_counter()
            for data in loader:
                d = data["decoder"]
                dec_objs = d["objs"].cuda()
                with torch.no_grad():
                    (boxes_pred, angles_pred), shapes = model.sample_box_and_shape(
                        None, dec_objs, d["tripltes"].cuda(), d["sdfs"], d["text_feats"].cuda(), d["rel_feats"].cuda(),
                        attributes=None, gen_shape=False)
                angles_pred = -180 + (torch.argmax(angles_pred, dim=1, keepdim=True) + 1) * 15.0
                assert shapes is None
                export = export_layout_scene(a.export_scenes, data["scan_id"][0], a.render_type, a.render_boxes, library,
                                             boxes_pred, angles_pred, dec_objs) if rank == 0 else None
                res["scenes"].append(dict(scan=data["scan_id"][0], nodes=int(dec_objs.shape[0]), shapes=0,
                                          finite=bool(torch.isfinite(boxes_pred).all()), export=export))
            torch.cuda.synchronize()
            res.update(total_s=time.perf_counter() - t_all, render_type=a.render_type, sampler_calls=calls[0])
            if rank == 0:
                print("EVAL_WALKTHROUGH " + json.dumps(res), flush=True)
            if world > 1:
                torch.distributed.barrier()
                torch.distributed.destroy_process_group()
            return
        if a.compare_attention:
            from commonscenes_amd import synth
            d = loader[0]["decoder"]
            O = d["objs"].shape[0]
            z = synth.gaussian_like("ev:cmp:z", (O, 64))
            x_T = synth.gaussian_like("ev:cmp:xT", (1, 3, 16, 16, 16))
            got = {}
            for mode in ("same", "f16"):
                model.vae_v2.Diff.df.set_attention_math(mode)
                t0 = time.perf_counter()
                with torch.no_grad():
                    _, sdf = model.sample_box_and_shape(None, d["objs"].cuda(), d["tripltes"].cuda(), d["sdfs"],
                                                        d["text_feats"].cuda(), d["rel_feats"].cuda(), attributes=None,
                                                        gen_shape=True, ddim_steps=a.ddim_steps, z=z, x_T=x_T)
                torch.cuda.synchronize()
                got[mode] = (sdf.double(), model.vae_v2.Diff.last_latents.double(), time.perf_counter() - t0)
            rl2 = lambda x, y: float((x - y).norm() / y.norm().clamp_min(1e-30))
            per_obj = [(rl2(got["f16"][1][i], got["same"][1][i])) for i in range(got["same"][1].shape[0])]
            res["attention_compare"] = dict(
                objects=int(got["same"][0].shape[0]), ddim_steps=a.ddim_steps,
                latent_rel_l2=rl2(got["f16"][1], got["same"][1]), latent_rel_l2_worst_object=max(per_obj),
                sdf_rel_l2=rl2(got["f16"][0], got["same"][0]),
                sdf_sign_flips=int(((got["f16"][0] > 0.02) != (got["same"][0] > 0.02)).sum()),
                sdf_voxels=int(got["same"][0].numel()), sample_s_default=got["same"][2], sample_s_f16=got["f16"][2],
                note="fp16 MFMA attention (one fp16 pass, fp32 softmax/accumulate) vs the default fp32-grade F16X3 "
                     "attention, same z / x_T / weights; report-only (SURVEY 8d)")
            model.vae_v2.Diff.df.set_attention_math("f16" if a.attention == "f16" else "same")
        if a.batch_scenes:
            from commonscenes_amd import synth
            scs = []
            for si, data in enumerate(loader):
                d = data["decoder"]
                O = d["objs"].shape[0]
                scs.append(dict(dec_objs=d["objs"].cuda(), dec_triplets=d["tripltes"].cuda(), dec_sdfs=d["sdfs"],
                                encoded_dec_text_feat=d["text_feats"].cuda(), encoded_dec_rel_feat=d["rel_feats"].cuda(),
                                z=synth.gaussian_like(f"ev:bs:z{si}", (O, 64)),
                                x_T=synth.gaussian_like(f"ev:bs:x{si}", (1, 3, 16, 16, 16))))

            def per_scene():
                outs, lats = [], []
                for sc in scs:
                    outs.append(model.sample_box_and_shape(None, sc["dec_objs"], sc["dec_triplets"], sc["dec_sdfs"],
                                                           sc["encoded_dec_text_feat"], sc["encoded_dec_rel_feat"],
                                                           gen_shape=True, ddim_steps=a.ddim_steps, z=sc["z"], x_T=sc["x_T"]))
                    lats.append(model.vae_v2.Diff.last_latents)
                return outs, torch.cat(lats)

            def batched():
                outs = model.sample_box_and_shape_many(scs, gen_shape=True, ddim_steps=a.ddim_steps)
                return outs, model.vae_v2.Diff.last_latents

            with torch.no_grad():
                per_scene(); batched()                        # warm-up (weight packing, allocator)
                torch.cuda.synchronize()
                t0 = time.perf_counter(); o1, l1 = per_scene(); torch.cuda.synchronize(); t_ps = time.perf_counter() - t0
                t0 = time.perf_counter(); o2, l2 = batched(); torch.cuda.synchronize(); t_b = time.perf_counter() - t0
            dev = float((l2.double() - l1.double()).norm() / l1.double().norm())
            res["batch_scenes"] = dict(scenes=len(scs), objects=[int(o[1].shape[0]) for o in o1], ddim_steps=a.ddim_steps,
                                       scene_by_scene_s=t_ps, coalesced_s=t_b, speedup=t_ps / t_b,
                                       launch_sizes=list(model.vae_v2.Diff.last_launch_sizes), latent_rel_l2=dev,
                                       boxes_equal=all(bool(torch.equal(x[0][0], y[0][0])) for x, y in zip(o1, o2)),
                                       note="shape sampling + decode of all scenes: one sample_box_and_shape call per scene "
                                            "(eval_3dfront.py:484-513) vs VAE.sample_box_and_shape_many")
        if a.constraints:
            from commonscenes_amd import constraints as CN
            accuracy, mapped = CN.new_accuracy(), 0
        if a.diversity_gpu:
            from commonscenes_amd.diversity import CATEGORIES, DiversityMeter
            # the synthetic vocabulary read as SG-FRONT's: class 0 `_scene_`, the last class `floor`, the ten categories 1..10
            meter = DiversityMeter({"_scene_": 0, "floor": 34, **{n: i for i, n in enumerate(CATEGORIES, start=1)}},
                                   points=a.points)
            meter_gen = torch.Generator().manual_seed(48)      # its own generator: the keys below draw what they always drew
        if a.object_views:
            from commonscenes_amd.object_views import init_mesh_renderer
            view_renderer = init_mesh_renderer(image_size=256, dist=1.7, elev=20, azim=20, device="cuda")   # eval_3dfront.py:476-478
            views = dict(images=0, render_s=0.0, write_s=0.0)
        x_T = None                                            # like the reference: fresh noise per call
        all_div_boxes, all_div_angles, all_div_chamfer = [], [], []
        t_all = time.perf_counter()
        for data in loader:
            d = data["decoder"]
            dec_objs, dec_triples = d["objs"].cuda(), d["tripltes"].cuda()
            text, rel, dec_sdfs = d["text_feats"].cuda(), d["rel_feats"].cuda(), d["sdfs"]
            t0 = time.perf_counter()
            with torch.no_grad():
                boxes_pred, shapes_pred = model.sample_box_and_shape(None, dec_objs, dec_triples, dec_sdfs, text, rel,
                                                                     attributes=None, gen_shape=True,
                                                                     ddim_steps=a.ddim_steps)
                boxes_pred, angles_pred = boxes_pred
                angles_pred = -180 + (torch.argmax(angles_pred, dim=1, keepdim=True) + 1) * 15.0
            if a.constraints:                                                  # eval_3dfront.py:722
                CN.validate_constrains(dec_triples, boxes_pred, None, None, EVAL_VOCAB, accuracy)
                mapped += sum(1 for p in d["tripltes"][:, 1].tolist() if 1 <= p <= 11)
            meshes = sdf_to_mesh(shapes_pred, render_all=True)                 # --visualize (helpers/util.py:298)
            torch.cuda.synchronize()
            t_scene = time.perf_counter() - t0
            nshape = shapes_pred.shape[0]
            export = export_scene(a.export_scenes, data["scan_id"][0], meshes, boxes_pred, angles_pred, dec_objs,
                                  a.render_boxes) if a.export_scenes and rank == 0 else None
            if a.object_views and rank == 0:
                n_img, t_r, t_w = export_object_views(a.export_scenes, data["scan_id"][0], meshes, boxes_pred, angles_pred,
                                                       dec_objs, view_renderer)
                views = dict(images=views["images"] + n_img, render_s=views["render_s"] + t_r,
                             write_s=views["write_s"] + t_w)
            # --evaluate_diversity
            boxes_div, angle_div, shapes_sample = [], [], []
            div_angles, div_sdfs = [], []
            for _ in range(a.samples):
                with torch.no_grad():
                    dboxes, dsdf = model.sample_box_and_shape(None, dec_objs, dec_triples, dec_sdfs, text, rel,
                                                              attributes=None, gen_shape=True, ddim_steps=a.ddim_steps)
                pts = sample_points(sdf_to_mesh(dsdf, render_all=True).verts_list(), a.points)
                dboxes, dangles = dboxes
                div_angles.append(dangles)
                div_sdfs.append(dsdf)
                norm = [torch.from_numpy(normalize(p.cpu().numpy())).cuda() for p in pts]
                boxes_div.append(dboxes)
                angle_div.append(np.expand_dims(np.argmax(dangles.cpu().numpy(), 1), 1) / 24.0 * 360.0)
                shapes_sample.append(torch.stack(norm))
            if a.diversity_gpu:
                shaped = torch.unique(torch.where(torch.ne(dec_sdfs, torch.zeros_like(dec_sdfs[0])))[0]).tolist()
                meter.add_scene(dec_objs, boxes_div, div_angles, div_sdfs, shape_nodes=shaped, generator=meter_gen)
            bd = torch.stack(boxes_div, 1)
            all_div_boxes += torch.std(bd, dim=1).cpu().numpy().tolist()
            all_div_angles += np.stack(angle_div, 1).std(axis=1).reshape(-1).tolist()
            ss = torch.stack(shapes_sample, 1)                                  # [objects, samples, points, 3]
            for sid in range(len(ss)):
                seq = []
                for k in range(ss.shape[1] - 1):
                    d1, d2 = chamfer(ss[sid, k:k + 1].float(), ss[sid, k + 1:k + 2].float())
                    seq.append(float((torch.mean(d1) + torch.mean(d2)).cpu()))
                all_div_chamfer.append(float(np.mean(seq)))
            res["scenes"].append(dict(scan=data["scan_id"][0], nodes=int(dec_objs.shape[0]), shapes=int(nshape),
                                      triples=int(dec_triples.shape[0]),
                                      sample_s=t_scene, verts=[int(v.shape[0]) for v in meshes.verts_list()],
                                      finite=bool(torch.isfinite(shapes_pred).all() and torch.isfinite(boxes_pred).all()),
                                      angle_range=[float(angles_pred.min()), float(angles_pred.max())]))
            if export is not None:
                res["scenes"][-1]["export"] = export
        torch.cuda.synchronize()
        res.update(total_s=time.perf_counter() - t_all, box_std_mean=float(np.mean(all_div_boxes)),
                   angle_std_mean=float(np.mean(all_div_angles)), chamfer_diversity_mean=float(np.mean(all_div_chamfer)),
                   chamfer_diversity_n=len(all_div_chamfer))
        if a.object_views:
            res["object_views"] = views
        if a.diversity_gpu:
            res["diversity"] = meter.summary()
        if a.constraints:
            res["accuracy"] = dict({k: dict(satisfied=int(sum(v)), evaluated=len(v)) for k, v in accuracy.items()},
                                   mapped_triples=mapped)
    if rank == 0:
        print("EVAL_WALKTHROUGH " + json.dumps(res), flush=True)
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
