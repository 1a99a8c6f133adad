#!/usr/bin/env python
"""Held-out evaluation of a CommonScenes checkpoint on the MI355X path: the two numbers an operator knows from the training
logs, computed forward-only on held-out SDFs.

    python tools/eval_checkpoint.py /path/to/model100.pth --sdfs held_out.npy [--timesteps 1,100,500,999] [--width 224]
    python tools/eval_checkpoint.py --synthetic [--width 32]          # synthetic weights and synth.sdf_volume variants

  * the diffusion model's loss_simple / loss_vlb per timestep (SDFusionText2ShapeModel.p_losses,
    sdfusion_txt2shape_model.py:311-345) over every given shape -- denoising_loss_table, unconditioned rows use a zero context
    unless the .npz brings `cond`;
  * the VQ-VAE's reconstruction iou / iou_std at threshold 0 and its L1 (VQVAEModel.eval_metrics, vqvae_model.py:138-168).
The checkpoint is the layout VAEGAN_V2FULL.py:687-699 writes ('df' + 'vqvae'; the VQ-VAE needs its encoder.* entries).
--sdfs: a .npy of [N, 1, 64, 64, 64] (or [N, 64, 64, 64]) fp32 SDFs, or a .npz with `sdf` and optionally `cond` [N, 1, 1280].
--meshes DIR in place of --sdfs: every DIR/*.obj, normalised into the unit sphere and sampled to a 64^3 SDF truncated at 0.2 on the
device (commonscenes_amd/mesh_sdf.py).
Prints a table and one JSON line (`EVAL_CHECKPOINT {...}`); shapes per second are for the record only.
"""
import argparse
import json
import os
import sys
import tempfile
import time
from collections import OrderedDict
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("checkpoint", nargs="?", help="model{epoch}.pth in the reference's layout ('df' + 'vqvae')")
    ap.add_argument("--synthetic", action="store_true", help="synthetic weights instead of a checkpoint file")
    ap.add_argument("--sdfs", help=".npy [N,1,64,64,64] or .npz with 'sdf' (and optionally 'cond')")
    ap.add_argument("--meshes", help="directory of .obj files instead of --sdfs: each is normalised into the unit sphere and sampled "
                                     "to a 64^3 SDF truncated at 0.2 (commonscenes_amd.mesh_sdf.mesh_to_sdf)")
    ap.add_argument("--timesteps", default="1,100,250,500,750,999")
    ap.add_argument("--width", type=int, default=224, help="UNet model_channels of the checkpoint (224 = the shipped config)")
    ap.add_argument("--seed", type=int, default=0, help="seed of the device generator that draws the noise")
    ap.add_argument("--batch", type=int, default=64, help="rows per UNet launch")
    ap.add_argument("--vq-batch", type=int, default=8, help="SDFs per VQ-VAE batch")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X (no CPU path)"
    if not a.synthetic and not a.checkpoint:
        ap.error("give a checkpoint file or --synthetic")
    if a.sdfs and a.meshes:
        ap.error("--sdfs and --meshes are alternatives")
    from commonscenes_amd import configs as K, synth
    from commonscenes_amd.sdfusion import SDFusionText2ShapeModel
    from commonscenes_amd.unet import unet_param_shapes
    from commonscenes_amd.vqvae import vqvae_encoder_param_shapes, vqvae_param_shapes
    from commonscenes_amd.vqvae_model import VQVAEModel

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
        raise SystemExit("the checkpoint's 'vqvae' entry has no encoder.* / quant_conv.* tensors: nothing can be encoded")
    cond = None
    if a.sdfs:
        blob = np.load(a.sdfs)
        sdf = blob if isinstance(blob, np.ndarray) else blob["sdf"]
        if not isinstance(blob, np.ndarray) and "cond" in blob:
            cond = torch.from_numpy(np.asarray(blob["cond"], np.float32))
        x = torch.from_numpy(np.asarray(sdf, np.float32)).reshape(-1, 1, 64, 64, 64)
        sdf_src = a.sdfs
    elif a.meshes:
        from commonscenes_amd.mesh_sdf import mesh_to_sdf, read_obj
        files = sorted(Path(a.meshes).glob("*.obj"))
        if not files:
            ap.error(f"no .obj file in {a.meshes}")
        parts = []
        for i in range(0, len(files), 8):
            vf = [read_obj(f) for f in files[i:i + 8]]
            parts.append(mesh_to_sdf([v for v, _ in vf], [f for _, f in vf], res=64, trunc=0.2).cpu())
        x = torch.cat(parts, dim=0)
        sdf_src = f"{len(files)} meshes of {a.meshes} through mesh_to_sdf"
    else:
        if not a.synthetic:
            ap.error("--sdfs or --meshes is required with a checkpoint file")
        v0, v1 = synth.sdf_volume(0), synth.sdf_volume(1)
        x = torch.cat([v0, v1, v0.flip(2), v1.flip(3)], dim=0)
        sdf_src = "synth.sdf_volume variants"
    N = int(x.shape[0])
    if cond is None:
        cond = torch.zeros((N, 1, int(cfg["context_dim"])), dtype=torch.float32)
    ts = [int(v) for v in a.timesteps.split(",") if v != ""]
    x = x.cuda()

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    table = model.denoising_loss_table(x, cond, ts, seed=a.seed, batch=a.batch)
    torch.cuda.synchronize()
    dt_df = time.perf_counter() - t0
    vm = VQVAEModel(vqvae=model.vqvae)
    loader = [{"sdf": x[i:i + a.vq_batch]} for i in range(0, N, a.vq_batch)]
    t0 = time.perf_counter()
    met = vm.eval_metrics(loader, thres=0.0)
    torch.cuda.synchronize()
    dt_vq = time.perf_counter() - t0

    print(f"checkpoint: {src}\nSDFs: {sdf_src} ({N} shapes)\nUNet width {a.width}\n")
    print(f"denoising losses over {N} shapes (noise seed {a.seed}):")
    print(f"  {'t':>5s} {'loss_simple':>12s} {'loss_vlb':>12s} {'min':>12s} {'max':>12s}")
    for k, t in enumerate(ts):
        col = table["per_sample"][:, k]
        print(f"  {t:5d} {float(table['loss_simple'][k]):12.6f} {float(table['loss_vlb'][k]):12.6f} {float(col.min()):12.6f} "
              f"{float(col.max()):12.6f}")
    print(f"\nVQ-VAE reconstruction: iou {float(met['iou']):.6f} (std {float(met['iou_std']):.6f}), "
          f"L1 {float(met['loss_rec']):.6f}, codebook loss {float(met['loss_codebook']):.6f}")
    print(f"throughput (for the record): {N * len(ts) / dt_df:.1f} shape-timesteps/s, {N / dt_vq:.1f} reconstructions/s")
    finite = bool(torch.isfinite(table["per_sample"]).all()) and all(bool(torch.isfinite(v)) for k, v in met.items()
                                                                      if k != "iou_std" or N > 1)
    rep = dict(source=src, sdfs=sdf_src, shapes=N, width=a.width, timesteps=ts, seed=a.seed,
               loss_simple=[float(v) for v in table["loss_simple"]], loss_vlb=[float(v) for v in table["loss_vlb"]],
               per_sample=[[float(v) for v in row] for row in table["per_sample"]],
               iou=float(met["iou"]), iou_std=float(met["iou_std"]), loss_rec=float(met["loss_rec"]),
               loss_codebook=float(met["loss_codebook"]), fell_back=table["fell_back"],
               shape_timesteps_per_s=N * len(ts) / dt_df, reconstructions_per_s=N / dt_vq, finite=finite, ok=finite)
    print("EVAL_CHECKPOINT " + json.dumps(rep))
    sys.exit(0 if finite else 1)


if __name__ == "__main__":
    main()
