#!/usr/bin/env python
"""Shape completion on the MI355X path: keep what lies inside a box of a partial SDF, generate the rest.

    python tools/complete_shape.py model.pth --sdf FILE.npy --range x0 x1 y0 y1 z0 z1 [--ngen K] [--obj DIR] [--cond FILE.npy]
    python tools/complete_shape.py --synthetic [--width 32] [--step-rows 32]

  * model.pth: the layout VAEGAN_V2FULL.py:687-699 writes ('df' + 'vqvae'; the VQ-VAE needs its encoder.* entries).
  * --sdf: a .npy of [N, 1, 64, 64, 64] (or [N, 64, 64, 64] / [64, 64, 64]) fp32 SDFs; --range: the KNOWN box in [-1, 1]^3
    (tensor axes 2, 3, 4 of the SDF take the x, y, z ranges, as diff_utils/demo_util.py:172-254 has it).
  * --mesh FILE.obj in place of --sdf: the mesh is normalised into the unit sphere and sampled to a 64^3 SDF truncated at 0.2
    on the device (commonscenes_amd/mesh_sdf.py; also with --synthetic weights).
  * --cond: [N, 1, 1280] conditions (the scene-graph embedding rel2shape would pass); a zero context otherwise.  The
    unconditional embedding is a zero context.
  * --obj DIR: the completed shapes as DIR/obj{n}_gen{k}.obj through sdf_to_mesh (marching cubes on the device).
  * --synthetic: synthetic weights and synth.sdf_volume inputs; also times ONE masked sampler step against one unmasked step
    at --step-rows rows (device events around synchronised work).
Prints one JSON line (`COMPLETE_SHAPE {...}`): shapes, steps, fell_back, the mean |completed - input| over the known region
(non-zero by construction: the known region is re-noised before every step and denoised by the last one, never copied back),
and the wall time per completion.
"""
import argparse
import json
import os
import sys
import tempfile
from collections import OrderedDict
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _timed(fn):
    """milliseconds of fn() between two device events, after a synchronise"""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1)


def _step_cost(model, rows, ctx, n_steps=4, repeats=3):
    """ms per sampler step at `rows` rows, masked against unmasked (S = 50, the first n_steps steps, alternated, the fastest of
    `repeats`): the masked step adds one randn and one cs_ddim_masked_blend launch."""
    from commonscenes_amd.ddim import DDIMSampler
    C_, D, H, W = model.z_shape
    g = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda *s: torch.randn(s, generator=g, device="cuda", dtype=torch.float32)
    c, uc, x_T, x0 = rnd(rows, 1, ctx), rnd(rows, 1, ctx), rnd(rows, C_, D, H, W), rnd(1, C_, D, H, W) * 0.8
    mask = torch.zeros(1, 1, D, H, W, device="cuda")
    mask[:, :, : D // 2] = 1.0

    def run(masked):
        if hasattr(model.df, "reset_run_cache"):
            model.df.reset_run_cache()
        kw = dict(x0=x0, mask=mask) if masked else {}
        return DDIMSampler(model).sample(S=50, batch_size=rows, shape=model.z_shape, conditioning=c, x_T=x_T, verbose=False,
                                         unconditional_guidance_scale=3.0, unconditional_conditioning=uc, eta=0.0,
                                         max_steps=n_steps, **kw)[0]
    run(True), run(False)                                   # warm-up: packing, workspaces, plans
    best = {True: float("inf"), False: float("inf")}
    for _ in range(repeats):
        for masked in (False, True):
            best[masked] = min(best[masked], _timed(lambda: run(masked))[1] / n_steps)
    return best[False], best[True]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("checkpoint", nargs="?", help="model{epoch}.pth in the reference's layout ('df' + 'vqvae')")
    ap.add_argument("--synthetic", action="store_true", help="synthetic weights and inputs instead of files")
    ap.add_argument("--sdf", help=".npy of [N,1,64,64,64] fp32 SDFs")
    ap.add_argument("--mesh", help=".obj instead of --sdf: normalised into the unit sphere and sampled to a 64^3 SDF truncated at "
                                   "0.2 (commonscenes_amd.mesh_sdf.mesh_to_sdf)")
    ap.add_argument("--range", type=float, nargs=6, metavar=("x0", "x1", "y0", "y1", "z0", "z1"),
                    help="the known box inside [-1, 1]^3")
    ap.add_argument("--cond", help=".npy of [N,1,1280] conditions (default: a zero context)")
    ap.add_argument("--ngen", type=int, default=1, help="completions per shape")
    ap.add_argument("--steps", type=int, default=100, help="ddim_steps (S; S = 100 runs 100 steps, S = 6 runs 7)")
    ap.add_argument("--scale", type=float, default=3.0, help="classifier-free guidance scale")
    ap.add_argument("--seed", type=int, default=0, help="torch.manual_seed before sampling (x_T and the q_sample noise)")
    ap.add_argument("--width", type=int, default=224, help="UNet model_channels of the checkpoint (224 = the shipped config)")
    ap.add_argument("--obj", help="directory for the completed meshes")
    ap.add_argument("--step-rows", type=int, default=32, help="--synthetic: rows of the masked / unmasked step timing (0: skip)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X (no CPU path)"
    if a.sdf and a.mesh:
        ap.error("--sdf and --mesh are alternatives")
    if not a.synthetic and not (a.checkpoint and (a.sdf or a.mesh) and a.range):
        ap.error("give model.pth --sdf FILE.npy (or --mesh FILE.obj) --range x0 x1 y0 y1 z0 z1, or --synthetic")
    from commonscenes_amd import configs as K, synth
    from commonscenes_amd.sdfusion import SDFusionText2ShapeModel
    from commonscenes_amd.unet import unet_param_shapes
    from commonscenes_amd.vqvae import vqvae_encoder_param_shapes, vqvae_param_shapes

    torch.cuda.set_device(0)
    cfg = dict(K.UNET_CROSSATTN) if a.width == 224 else K.reduced(K.UNET_CROSSATTN, a.width)
    with tempfile.TemporaryDirectory() as td:
        model = SDFusionText2ShapeModel(K.write_yaml_configs(td, unet=cfg))
    if a.synthetic:
        dd = dict(K.VQVAE_DDCONFIG)
        vq_shapes = OrderedDict(list(vqvae_encoder_param_shapes(dd, K.VQVAE_N_EMBED, K.VQVAE_EMBED_DIM).items()) +
                                list(vqvae_param_shapes(dd, K.VQVAE_N_EMBED, K.VQVAE_EMBED_DIM).items()))
        model.load_state_dict({"df": synth.synth_state_dict(unet_param_shapes(cfg), device="cuda"),
                               "vqvae": synth.synth_state_dict(vq_shapes, device="cuda")})
        src = "synthetic (commonscenes_amd/synth.py)"
    else:
        ck = torch.load(a.checkpoint, map_location="cpu")
        if not (isinstance(ck, dict) and "df" in ck and "vqvae" in ck):
            raise SystemExit("the checkpoint must hold 'df' and 'vqvae' state dicts (VAEGAN_V2FULL.py:687-699)")
        model.load_state_dict(ck)
        src = a.checkpoint
    if not model.vqvae.has_encoder:
        raise SystemExit("the checkpoint's 'vqvae' entry has no encoder.* / quant_conv.* tensors: a partial SDF cannot be encoded")
    if a.sdf:
        x = torch.from_numpy(np.asarray(np.load(a.sdf), np.float32)).reshape(-1, 1, 64, 64, 64)
        sdf_src = a.sdf
    elif a.mesh:
        from commonscenes_amd.mesh_sdf import mesh_to_sdf, read_obj
        mv, mf = read_obj(a.mesh)
        x = mesh_to_sdf([mv], [mf], res=64, trunc=0.2).cpu()
        sdf_src = f"{a.mesh} ({mf.shape[0]} faces) through mesh_to_sdf"
    else:
        x = torch.cat([synth.sdf_volume(0), synth.sdf_volume(1)], dim=0)
        sdf_src = "synth.sdf_volume(0), (1)"
    r = a.range or [-1.0, 0.1, -0.55, 1.0, -1.0, 1.0]
    xyz = {"x": (r[0], r[1]), "y": (r[2], r[3]), "z": (r[4], r[5])}
    N = int(x.shape[0])
    ctx = int(cfg["context_dim"])
    cond = torch.from_numpy(np.asarray(np.load(a.cond), np.float32)).reshape(N, 1, ctx) if a.cond else torch.zeros(N, 1, ctx)
    uc = torch.zeros(N, 1, ctx)
    x = x.cuda()

    def run():
        torch.manual_seed(a.seed)
        return model.shape_comp(x, xyz, cond, uc=uc, ngen=a.ngen, ddim_steps=a.steps, uc_scale=a.scale, return_meta=True)
    if a.synthetic:
        run()                                               # warm-up (packing, workspaces): the timing below is of a second call
    (gen, meta), ms = _timed(run)
    rows = N * a.ngen
    from commonscenes_amd.demo_util import get_partial_shape
    known = get_partial_shape(x, xyz)["shape_mask"].repeat_interleave(a.ngen, dim=0)
    ref = x.repeat_interleave(a.ngen, dim=0)
    diff = (gen - ref).abs()
    n_known = int(known.sum())
    known_diff = float(diff[known].double().mean()) if n_known else float("nan")
    rest_diff = float(diff[~known].double().mean()) if n_known < known.numel() else float("nan")
    finite = bool(torch.isfinite(gen).all())
    rep = dict(source=src, sdfs=sdf_src, shapes=N, ngen=a.ngen, completions=rows, out_shape=list(gen.shape), width=a.width,
               ddim_steps=a.steps, steps=meta["masked_steps"], scale=a.scale, range=r, known_fraction=n_known / known.numel(),
               known_mean_abs_diff=known_diff, generated_mean_abs_diff=rest_diff, launch_sizes=meta["launch_sizes"],
               fell_back=meta["fell_back"], ms_per_completion=ms / rows, finite=finite, ok=finite)
    if a.synthetic and a.step_rows > 0:
        plain, masked = _step_cost(model, a.step_rows, ctx)
        rep.update(step_rows=a.step_rows, plain_step_ms=plain, masked_step_ms=masked)
        rep["fell_back"] = dict(model.fell_back)
    if a.obj:
        from commonscenes_amd.mesh import sdf_to_mesh
        out = Path(a.obj)
        out.mkdir(parents=True, exist_ok=True)
        meshes = sdf_to_mesh(gen, render_all=True)
        for k, (v, f) in enumerate(zip(meshes.verts_list(), meshes.faces_list())):
            v, f = v.cpu().numpy(), f.cpu().numpy() + 1
            with open(out / f"obj{k // a.ngen}_gen{k % a.ngen}.obj", "w") as fh:
                fh.writelines(f"v {p[0]:.6f} {p[1]:.6f} {p[2]:.6f}\n" for p in v)
                fh.writelines(f"f {t[0]} {t[1]} {t[2]}\n" for t in f)
        rep["obj_dir"] = str(out)
    print(f"checkpoint: {src}\nSDFs: {sdf_src} ({N} shapes x {a.ngen} completions), known box {xyz}\n"
          f"{meta['masked_steps']} masked DDIM steps, {ms / rows:.1f} ms per completion; mean |completed - input|: "
          f"{known_diff:.5f} over the known region, {rest_diff:.5f} over the generated one")
    print("COMPLETE_SHAPE " + json.dumps(rep))
    sys.exit(0 if finite else 1)


if __name__ == "__main__":
    main()
