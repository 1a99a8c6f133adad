"""VQ-VAE evaluation behind the reference's `VQVAEModel` interface (model/vqvae_model.py), forward only.

  iou(x_gt, x, thres)        model/diff_utils/util.py:111-130 -- one cs_pair_stats launch instead of two mask volumes
  VQLoss(codebook_weight)    model/losses.py:63-83, forward value and log dict (no autograd graph)
  VQVAEModel                 set_input / forward / inference / test_iou / eval_metrics / get_current_visuals
                             (vqvae_model.py:97-168, 204-218); the views come from object_views (256^2, camera 1.7, 20, 20,
                             vqvae_model.py:70-71)

Not built: `best_iou` / `save`, the optimiser and everything that needs a backward pass (`backward`,
`optimize_parameters`): they raise NotImplementedError.
"""
from __future__ import annotations

from collections import OrderedDict
from pathlib import Path
from typing import Optional

import torch

from . import ops
from .vqvae import VQVAE

Tensor = torch.Tensor


def iou_from_counts(counts: Tensor) -> Tensor:
    """util.py:129 from the int64 {inter, union} rows: float32(inter) / (float32(union) + 1e-12), in that order -- the sum
    `union + 1e-12` is an fp32 one, so it only matters for an empty union, where the quotient is 0."""
    inter = counts[:, 0].to(torch.float32)
    union = counts[:, 1].to(torch.float32)
    return inter / (union + 1e-12)


@torch.no_grad()
def iou(x_gt: Tensor, x: Tensor, thres: float) -> Tensor:
    """util.py:111-130: per-sample IoU of the occupied sets {x_gt <= 0} and {x <= thres} (> 0 is free space).  The masks
    are built there as "1 unless v > threshold", so a NaN voxel counts as occupied; cs_pair_stats counts the same sets."""
    _, counts = ops.pair_stats(x_gt, x, 0.0, float(thres), want_sums=False)
    return iou_from_counts(counts)


class VQLoss:
    """losses.py:63-83, value only: (loss, log) with log = {loss_total, loss_codebook, loss_nll, loss_rec}."""

    def __init__(self, codebook_weight: float = 1.0):
        self.codebook_weight = codebook_weight

    def to(self, device):
        return self

    def from_sums(self, codebook_loss: Tensor, l1_sum, numel: int):
        """the arithmetic behind forward(): `l1_sum` = the fp64 sum of |inputs - reconstructions| over `numel` elements"""
        dev = codebook_loss.device
        nll_loss = (torch.as_tensor(l1_sum, dtype=torch.float64, device=dev).sum() / float(numel)).to(torch.float32)
        cb = codebook_loss.detach().to(torch.float32).mean()
        loss = nll_loss + self.codebook_weight * cb
        log = {"loss_total": loss.clone().detach().mean(), "loss_codebook": cb, "loss_nll": nll_loss.detach().mean(),
               "loss_rec": nll_loss.detach().mean()}
        return loss, log

    @torch.no_grad()
    def forward(self, codebook_loss: Tensor, inputs: Tensor, reconstructions: Tensor, split: str = "train"):
        sums, _ = ops.pair_stats(inputs, reconstructions)
        return self.from_sums(codebook_loss, sums[:, 1], inputs.numel())

    __call__ = forward


class VQVAEModel:
    """The reference's VQVAEModel over this package's VQVAE (which needs its encoder: a decode-only checkpoint raises on the
    first encode).  Build it from an `opt` mapping like the reference (opt.network.vq_cfg / opt.network.ckpt, opt.hyper.device)
    or hand it a loaded VQVAE."""

    def __init__(self, opt=None, vqvae: Optional[VQVAE] = None, resolve_dir: Optional[Path] = None,
                 codebook_weight: float = 1.0):
        self.isTrain = False
        self.model_name = self.name()
        if vqvae is None:
            from .sdfusion import AttrDict, load_yaml, to_attr
            self.opt = opt if isinstance(opt, AttrDict) else to_attr(opt)
            self.device = torch.device(self.opt.hyper.device)
            if self.device.type != "cuda":
                raise RuntimeError("commonscenes_amd runs on the HIP device only (hyper.device must be 'cuda')")
            base = Path(resolve_dir) if resolve_dir else Path.cwd()
            rp = lambda p: str(p) if Path(p).is_absolute() else str(base / p)
            assert self.opt.network.vq_cfg is not None
            configs = load_yaml(rp(self.opt.network.vq_cfg))
            mp = configs.model.params
            vqvae = VQVAE(mp.ddconfig, mp.n_embed, mp.embed_dim, device=self.device)
            lc = configs.get("lossconfig")
            if lc is not None:
                codebook_weight = lc.params.codebook_weight
            self.vqvae = vqvae
            if self.opt.network.get("ckpt") is not None:
                self.load_ckpt(rp(self.opt.network.ckpt))
        else:
            self.opt = opt
            self.vqvae = vqvae
            self.device = torch.device(vqvae.device)
        self.vqvae_module = self.vqvae
        self.loss_vq = VQLoss(codebook_weight=codebook_weight)

    def name(self):
        return "VQVAE-Model"

    def switch_eval(self):
        self.vqvae.eval()

    def switch_train(self):
        raise NotImplementedError("training is out of scope (SURVEY 3.4)")

    def set_input(self, input):
        self.x = input["sdf"].to(device=self.device, dtype=torch.float32)
        self.cur_bs = self.x.shape[0]

    @torch.no_grad()
    def forward(self):
        """:107-108: reconstruction through the quantiser and the codebook loss."""
        self.x_recon, self.qloss = self.vqvae(self.x, verbose=False)

    @torch.no_grad()
    def inference(self, data, should_render=False, verbose=False):
        """:110-124: encode without quantising, then decode_no_quant (which quantises to the nearest code first)."""
        self.switch_eval()
        self.set_input(data)
        self.z = self.vqvae(self.x, forward_no_quant=True, encode_only=True)
        self.x_recon = self.vqvae_module.decode_no_quant(self.z)
        if should_render:
            self._render()

    @property
    def renderer(self):
        """:70-71: init_mesh_renderer(image_size=256, dist=1.7, elev=20, azim=20), built on first use"""
        if getattr(self, "_renderer", None) is None:
            from .object_views import init_mesh_renderer
            self._renderer = init_mesh_renderer(image_size=256, dist=1.7, elev=20, azim=20, device=self.device)
        return self._renderer

    def _render(self):
        from .object_views import render_sdf
        self.image = render_sdf(self.renderer, self.x)
        self.image_recon = render_sdf(self.renderer, self.x_recon)

    @torch.no_grad()
    def get_current_visuals(self):
        """:204-218: OrderedDict(image, image_recon) of uint8 grids (tensor2im) of the last input and its reconstruction"""
        from .object_views import tensor2im
        self._render()
        return OrderedDict((name, tensor2im(getattr(self, name))) for name in ("image", "image_recon"))

    @torch.no_grad()
    def test_iou(self, data, thres=0.0):
        """:126-136.  thres: threshold to consider a voxel to be free space or occupied space."""
        self.inference(data, should_render=False)
        return iou(self.x, self.x_recon, thres)

    @torch.no_grad()
    def eval_metrics(self, dataloader, thres=0.0, global_step=0):
        """:138-168: OrderedDict(iou, iou_std) over all samples of the loader (unbiased std).  Extension: `loss_rec` and
        `loss_codebook`, VQLoss's log values of forward() accumulated over the set (every voxel / every sample weighs the
        same, whatever the batch sizes).  The reference's best-checkpoint bookkeeping is not built."""
        self.switch_eval()
        iou_list = []
        l1_sum, numel, cb_sum, count = 0.0, 0, 0.0, 0
        for test_data in dataloader:
            iou_list.append(self.test_iou(test_data, thres=thres).detach())
            self.forward()
            sums, _ = ops.pair_stats(self.x, self.x_recon)
            l1_sum += float(sums[:, 1].sum())
            numel += self.x.numel()
            cb_sum += float(self.qloss) * self.cur_bs
            count += self.cur_bs
        v = torch.cat(iou_list)
        return OrderedDict([
            ("iou", v.mean().data),
            ("iou_std", v.std().data),
            ("loss_rec", torch.tensor(l1_sum / max(numel, 1), dtype=torch.float32, device=self.device)),
            ("loss_codebook", torch.tensor(cb_sum / max(count, 1), dtype=torch.float32, device=self.device)),
        ])

    def backward(self):
        raise NotImplementedError("training is out of scope (SURVEY 3.4)")

    def optimize_parameters(self, total_steps):
        raise NotImplementedError("training is out of scope (SURVEY 3.4)")

    def save(self, label, global_step=0, save_opt=False):
        raise NotImplementedError("checkpoint writing is not built")

    def load_ckpt(self, ckpt, load_opt=False):
        """:241-257: a path or a state dict, raw or under 'vqvae'."""
        sd = torch.load(ckpt, map_location="cpu") if isinstance(ckpt, (str, Path)) else ckpt
        self.vqvae.load_state_dict(sd["vqvae"] if "vqvae" in sd else sd)
