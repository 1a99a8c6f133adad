"""MI355X-native VQ-VAE decode side behind the reference's `VQVAE` interface.

Mirrors  model/networks/vqvae_networks/network.py:48-103   VQVAE.decode / decode_no_quant
         model/networks/vqvae_networks/quantizer.py:68-119 VectorQuantizer.forward (nearest code)
         model/networks/vqvae_networks/vqvae_modules.py:292-409 Decoder3D (+ ResnetBlock, AttnBlock, Upsample)
         model/model_utils.py:7-31 load_vqvae
Channels-last throughout; nearest x2 upsampling is folded into the following conv's address
arithmetic (no 8x larger intermediate), swish/GELU are fused into the GroupNorm apply pass, the
single-head N=4096 attention is the flash kernel (no 64 MiB score matrix), and the codebook search
runs out of LDS (no 134 MB distance matrix).
The encode side (network.py:78-88, 123-140: encode / encode_no_quant / forward; Encoder3D vqvae_modules.py:181-290)
runs when the state_dict brings the encoder: the same ResnetBlock / AttnBlock / GroupNorm building blocks on the
decoder's kernels, the 1-channel conv_in and the quantiser's straight-through outputs on their own kernels
(csrc/cs_vqenc.hip), and the Downsample's F.pad(0,1) + stride-2 conv as one conv with explicit pads.
"""
from __future__ import annotations

import os
from collections import OrderedDict
from typing import Dict, Optional, Tuple

import torch

from . import lib as L
from . import ops

Tensor = torch.Tensor


def _vq_groups(c: int) -> int:          # vqvae_modules.py:13-21
    if c <= 32:
        return c // 4
    if c % 32 != 0:
        return 30
    return 32


def _dd(ddconfig) -> dict:
    g = (lambda k, d=None: ddconfig.get(k, d)) if isinstance(ddconfig, dict) else (
        lambda k, d=None: getattr(ddconfig, k, d))
    cfg = dict(ch=int(g("ch")), out_ch=int(g("out_ch")), ch_mult=tuple(g("ch_mult")),
               num_res_blocks=int(g("num_res_blocks")), z_channels=int(g("z_channels")),
               resolution=int(g("resolution")), attn_resolutions=tuple(g("attn_resolutions", ()) or ()))
    if cfg["attn_resolutions"]:
        raise NotImplementedError("attn_resolutions is empty in config/vqvae_snet.yaml; per-level attention "
                                  "is not on the path")
    return cfg


def vqvae_param_shapes(ddconfig, n_embed: int, embed_dim: int) -> "OrderedDict[str, Tuple[int, ...]]":
    """Decode-side state_dict entries of the reference VQVAE."""
    cfg = _dd(ddconfig)
    S: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()

    def conv(p, o, i, k):
        S[p + ".weight"] = (o, i, k, k, k)
        S[p + ".bias"] = (o,)

    def norm(p, c):
        S[p + ".weight"] = (c,)
        S[p + ".bias"] = (c,)

    def res(p, cin, cout):
        norm(p + ".norm1", cin)
        conv(p + ".conv1", cout, cin, 3)
        norm(p + ".norm2", cout)
        conv(p + ".conv2", cout, cout, 3)
        if cin != cout:
            conv(p + ".nin_shortcut", cout, cin, 1)

    ch, mult = cfg["ch"], cfg["ch_mult"]
    nres = len(mult)
    block_in = ch * mult[-1]
    D = "decoder."
    conv(D + "conv_in", block_in, cfg["z_channels"], 3)
    res(D + "mid.block_1", block_in, block_in)
    norm(D + "mid.attn_1.norm", block_in)
    for n in ("q", "k", "v", "proj_out"):
        conv(D + f"mid.attn_1.{n}", block_in, block_in, 1)
    res(D + "mid.block_2", block_in, block_in)
    for i_level in reversed(range(nres)):
        block_out = ch * mult[i_level]
        for i_block in range(cfg["num_res_blocks"]):
            res(f"{D}up.{i_level}.block.{i_block}", block_in, block_out)
            block_in = block_out
        if i_level != 0:
            conv(f"{D}up.{i_level}.upsample.conv", block_in, block_in, 3)
    norm(D + "norm_out", block_in)
    conv(D + "conv_out", cfg["out_ch"], block_in, 3)
    S["quantize.embedding.weight"] = (n_embed, embed_dim)
    conv("post_quant_conv", cfg["z_channels"], embed_dim, 1)
    return S


def vqvae_encoder_param_shapes(ddconfig, n_embed: int, embed_dim: int) -> "OrderedDict[str, Tuple[int, ...]]":
    """Encode-side state_dict entries of the reference VQVAE (encoder.* and quant_conv.*), in its state_dict order."""
    cfg = _dd(ddconfig)
    g = (lambda k, d=None: ddconfig.get(k, d)) if isinstance(ddconfig, dict) else (
        lambda k, d=None: getattr(ddconfig, k, d))
    in_ch, double_z = int(g("in_channels", 1)), bool(g("double_z", True))
    S: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()

    def conv(p, o, i, k):
        S[p + ".weight"] = (o, i, k, k, k)
        S[p + ".bias"] = (o,)

    def norm(p, c):
        S[p + ".weight"] = (c,)
        S[p + ".bias"] = (c,)

    def res(p, cin, cout):
        norm(p + ".norm1", cin)
        conv(p + ".conv1", cout, cin, 3)
        norm(p + ".norm2", cout)
        conv(p + ".conv2", cout, cout, 3)
        if cin != cout:
            conv(p + ".nin_shortcut", cout, cin, 1)

    ch, mult = cfg["ch"], cfg["ch_mult"]
    nres = len(mult)
    in_mult = (1,) + tuple(mult)
    E = "encoder."
    conv(E + "conv_in", ch, in_ch, 3)
    block_in = ch
    for i_level in range(nres):                             # vqvae_modules.py:215-235
        block_in = ch * in_mult[i_level]
        block_out = ch * mult[i_level]
        for i_block in range(cfg["num_res_blocks"]):
            res(f"{E}down.{i_level}.block.{i_block}", block_in, block_out)
            block_in = block_out
        if i_level != nres - 1:
            conv(f"{E}down.{i_level}.downsample.conv", block_in, block_in, 3)
    res(E + "mid.block_1", block_in, block_in)
    norm(E + "mid.attn_1.norm", block_in)
    for n in ("q", "k", "v", "proj_out"):
        conv(E + f"mid.attn_1.{n}", block_in, block_in, 1)
    res(E + "mid.block_2", block_in, block_in)
    norm(E + "norm_out", block_in)
    z = cfg["z_channels"]
    conv(E + "conv_out", 2 * z if double_z else z, block_in, 3)
    conv("quant_conv", embed_dim, z, 1)                     # network.py:69
    return S


# Downsample (vqvae_modules.py:42-60): F.pad(x, (0, 1, 0, 1, 0, 1)) then Conv3d(k 3, stride 2, pad 0) -- one conv with
# pads (low 0, high 1) per dim; the generic gather reads the high pad's taps as zero
_DOWN_PAD = ((0, 1), (0, 1), (0, 1))


class _Tables:
    """One side's weights as the building blocks read them: raw tensors, packs, numerics, Normalize bounds and the
    attention block's static-bound statistics."""

    def __init__(self, sd, pk, math, ngb, attn_stat):
        self.sd, self.pk, self.math, self.ngb, self.attn_stat = sd, pk, math, ngb, attn_stat


class VQVAE:
    """Drop-in for reference `VQVAE` (network.py:48-140): decode side always, encode side when the encoder is loaded."""

    # what an F16X3 encode does when an activation leaves the fp16 range: 'fp32' re-runs that call on fp32-packed
    # encoder weights (with a warning), 'raise' propagates CsOverflowError (as SDFusionText2ShapeModel.overflow_policy)
    overflow_policy = os.environ.get("CS_OVERFLOW_POLICY", "fp32")

    def __init__(self, ddconfig, n_embed: int, embed_dim: int, device: str | torch.device = "cuda"):
        self.cfg = _dd(ddconfig)
        self.ddconfig = ddconfig
        self.n_embed, self.embed_dim = int(n_embed), int(embed_dim)
        self.device = torch.device(device)
        self.shapes = vqvae_param_shapes(ddconfig, n_embed, embed_dim)
        self._sd: Dict[str, Tensor] = {}
        self._packed = None
        self.math = L.DEFAULT_MATH      # F16X3 unless CS_MATH=fp32
        self.last_indices: Optional[Tensor] = None
        self.enc_shapes = vqvae_encoder_param_shapes(ddconfig, n_embed, embed_dim)
        self._esd: Dict[str, Tensor] = {}       # encoder.* / quant_conv.*: kept only when a state_dict brings the whole set
        self._epk: Dict[int, _Tables] = {}      # encoder packs by numerics mode

    # ---- nn.Module-like surface ----
    def state_dict(self):
        if not self._esd:
            return OrderedDict((k, self._sd[k]) for k in self.shapes if k in self._sd)
        # the reference's order: encoder, decoder, quantize, quant_conv, post_quant_conv
        enc = [k for k in self.enc_shapes if k.startswith("encoder.")]
        dec = [k for k in self.shapes if not k.startswith("post_quant_conv.")]
        qc = [k for k in self.enc_shapes if k.startswith("quant_conv.")]
        pq = [k for k in self.shapes if k.startswith("post_quant_conv.")]
        out = OrderedDict()
        for k in enc + dec + qc + pq:
            t = self._esd.get(k, self._sd.get(k))
            if t is not None:
                out[k] = t
        return out

    @property
    def has_encoder(self) -> bool:
        return bool(self._esd)

    def load_state_dict(self, sd, strict: bool = True):
        """Accepts a decode-only or a full reference VQVAE state_dict.  encoder.* / quant_conv.* are kept (and enable
        encode) when the COMPLETE encoder set is present -- a shape mismatch in it raises; a partial set is ignored."""
        missing = [k for k in self.shapes if k not in sd]
        unexpected = [k for k in sd if k not in self.shapes and not k.startswith(("encoder.", "quant_conv."))]
        if strict and (missing or unexpected):
            raise RuntimeError(f"VQVAE.load_state_dict: missing {missing[:5]} unexpected {unexpected[:5]}")
        with_enc = all(k in sd for k in self.enc_shapes)
        if with_enc:
            for k, shp in self.enc_shapes.items():
                if tuple(sd[k].shape) != tuple(shp):
                    raise RuntimeError(f"size mismatch for {k}: {tuple(sd[k].shape)} vs {shp}")
        for k, shp in self.shapes.items():
            if k in sd:
                if tuple(sd[k].shape) != tuple(shp):
                    raise RuntimeError(f"size mismatch for {k}: {tuple(sd[k].shape)} vs {shp}")
                self._sd[k] = sd[k].detach().to(device=self.device, dtype=torch.float32).contiguous()
        if with_enc:
            self._esd = {k: sd[k].detach().to(device=self.device, dtype=torch.float32).contiguous()
                         for k in self.enc_shapes}
        self._packed = None
        self._epk = {}
        return self

    def parameters(self):
        return iter([*self._sd.values(), *self._esd.values()])

    def to(self, device):
        self.device = torch.device(device)
        self._sd = {k: v.to(self.device) for k, v in self._sd.items()}
        self._esd = {k: v.to(self.device) for k, v in self._esd.items()}
        self._packed = None
        self._epk = {}
        return self

    def cuda(self):
        return self.to("cuda")

    def eval(self):
        return self

    def set_math(self, mode) -> "VQVAE":
        """'fp32' or 'f16x3' GEMM numerics (see DiffusionUNet.set_math)."""
        m = {"fp32": L.MATH_FP32, "f16x3": L.MATH_F16X3}.get(mode, mode)
        if m not in (L.MATH_FP32, L.MATH_F16X3):
            raise ValueError(f"unknown math mode {mode!r}")
        if m != self.math:
            self.math = m
            self._packed = None
        return self

    # ---- packing ----
    def _pack(self):
        sd = self._sd
        missing = [k for k in self.shapes if k not in sd]
        if missing:
            raise RuntimeError(f"VQVAE: weights not loaded ({len(missing)} tensors missing)")
        pk = {}
        for k in self.shapes:
            if k.endswith(".weight") and sd[k].dim() == 5:
                p = k[:-7]
                if p.startswith("decoder.mid.attn_1.") and p.split(".")[-1] in ("q", "k", "v"):
                    continue
                if p == "post_quant_conv":
                    # emit a zero 4th channel so the decoder's conv_in reads float4-aligned rows
                    wz, bz = sd[k], sd[p + ".bias"]
                    pad = (-wz.shape[0]) % 4
                    wz = torch.cat([wz, wz.new_zeros((pad, *wz.shape[1:]))], dim=0)
                    bz = torch.cat([bz, bz.new_zeros(pad)], dim=0)
                    pk[p] = ops.pack_weight(wz, bz, cin_pad=(wz.shape[1] + 3) // 4 * 4, math=self.math)
                    continue
                cin = sd[k].shape[1]
                if p == "decoder.conv_out" and ops.tapcol_ok(sd[k], self.math):
                    # vqvae_modules.py:473 (3x3x3 conv to out_ch = 1): taps as columns, see ops.py
                    pk[p] = ops.pack_weight_tapcol(sd[k], sd.get(p + ".bias"))
                    continue
                # Upsample's conv (vqvae_modules.py:35-39: nearest x2 in D, H, W) runs on the source grid
                fold = (1, 1, 1) if p.endswith(".upsample.conv") else None
                pk[p] = ops.pack_weight(sd[k], sd.get(p + ".bias"), cin_pad=(cin + 3) // 4 * 4, math=self.math,
                                        fold_up=fold)
                if fold is None and self.math == L.MATH_F16X3:      # r5: + the Winograd-W pack where the geometry allows
                    ops.pack_weight_wino(pk[p], sd[k])
        a = "decoder.mid.attn_1."
        wqkv = torch.cat([sd[a + "q.weight"], sd[a + "k.weight"], sd[a + "v.weight"]], dim=0)
        bqkv = torch.cat([sd[a + "q.bias"], sd[a + "k.bias"], sd[a + "v.bias"]], dim=0)
        pk[a + "qkv"] = ops.pack_weight(wqkv, bqkv, math=self.math)
        # r6: what bounds the attention block's q / k / v (ops.attnblock_static_scales; cs_vqvae_pack takes the same statistics)
        self._attn_stat = None
        if self.math == L.MATH_F16X3:
            c_ = int(sd[a + "q.weight"].shape[0])
            l2, _ = ops.weight_rowstats([sd[a + f"{n}.weight"].reshape(c_, -1) for n in ("q", "k", "v")])
            _, bm = ops.weight_rowstats([sd[a + f"{n}.bias"].reshape(1, -1) for n in ("q", "k", "v")])
            self._attn_stat = (l2, bm)
        # |gamma|, |beta| maxima of the Normalize layers: norm-fed GEMMs take their F16X3 operand scale from the
        # producer's bound (ops.norm_a_scale), one read-back at load time
        norms = [k[:-7] for k in sd if k.startswith("decoder.") and k.endswith(".weight") and sd[k].dim() == 1]
        if self.math == L.MATH_F16X3 and norms:
            mx = torch.stack([torch.stack([sd[n + ".weight"].abs().max(), sd[n + ".bias"].abs().max()]) for n in norms]).cpu()
            self._ngb = {n: (float(mx[i, 0]), float(mx[i, 1])) for i, n in enumerate(norms)}
        else:
            self._ngb = {}
        self._packed = pk

    # ---- building blocks ----
    def _nas(self, norm: str, n: int, T: Optional[_Tables] = None):
        gb = (getattr(self, "_ngb", {}) if T is None else T.ngb).get(norm)
        return ops.norm_a_scale(gb[0], gb[1], n) if gb is not None else None

    def _res(self, p: str, x: Tensor, T: Optional[_Tables] = None) -> Tensor:
        sd, pk = (self._sd, self._packed) if T is None else (T.sd, T.pk)
        math = self.math if T is None else T.math
        c = x.shape[-1]
        m = x.shape[0] * x.shape[1] * x.shape[2] * x.shape[3]
        rows = m // x.shape[0]
        s1 = self._nas(p + ".norm1", rows * (c // _vq_groups(c)), T)
        vol = tuple(int(v) for v in x.shape[:4])
        # (r5: the Winograd-W operand where the conv takes that route -- decided per sample geometry, never by the batch)
        h = ops.groupnorm(x, sd[p + ".norm1.weight"], sd[p + ".norm1.bias"], _vq_groups(c), 1e-6, L.ACT_SILU,
                          split16=ops.wants_split16(m, pk[p + ".conv1"]), a_scale=s1,
                          wino=ops.wants_wino(*vol, pk[p + ".conv1"]))
        # (stats="invariant", r5: the conv's epilogue leaves the partial sums norm2 takes its statistics from -- only where
        # the statistics tiles are the same for one object and for a slice of sixteen, see ops._epilogue_extras)
        h = ops.conv_gemm(h, pk[p + ".conv1"], math=math, a_scale=s1, stats="invariant")
        co = h.shape[-1]
        s2 = self._nas(p + ".norm2", rows * (co // _vq_groups(co)), T)
        h = ops.groupnorm(h, sd[p + ".norm2.weight"], sd[p + ".norm2.bias"], _vq_groups(co), 1e-6, L.ACT_SILU,
                          split16=ops.wants_split16(m, pk[p + ".conv2"]), a_scale=s2,
                          wino=ops.wants_wino(*vol, pk[p + ".conv2"]))
        skip = x if (p + ".nin_shortcut") not in pk else ops.conv_gemm(x, pk[p + ".nin_shortcut"], math=math)
        return ops.conv_gemm(h, pk[p + ".conv2"], res=skip, math=math, a_scale=s2, stats="invariant")

    def _attn(self, p: str, x: Tensor, T: Optional[_Tables] = None) -> Tensor:
        sd, pk = (self._sd, self._packed) if T is None else (T.sd, T.pk)
        math = self.math if T is None else T.math
        nb, d, h, w, c = x.shape
        n = d * h * w
        hn = ops.groupnorm(x, sd[p + ".norm.weight"], sd[p + ".norm.bias"], _vq_groups(c), 1e-6, L.ACT_NONE)
        qkv = ops.linear(hn.view(nb, n, c), pk[p + ".qkv"], math=math,
                         a_scale=self._nas(p + ".norm", n * (c // _vq_groups(c)), T))
        # r6: q / k / v = Conv1x1(Normalize(x)) + bias are bounded by the weights and the norm's affine parameters alone: static
        # operand scales (no input can leave the fp16 range; the attention output is a convex combination of v rows)
        ss = None
        gb = (getattr(self, "_ngb", {}) if T is None else T.ngb).get(p + ".norm")
        st = getattr(self, "_attn_stat", None) if T is None else T.attn_stat
        if math == L.MATH_F16X3 and gb is not None and st is not None:
            ss = ops.attnblock_static_scales(gb[0], gb[1], n * (c // _vq_groups(c)), c, st[0], st[1], int(c) ** (-0.5))
        a = ops.attention(qkv[..., 0:c], qkv[..., c:2 * c], qkv[..., 2 * c:], 1, int(c) ** (-0.5), math=math,
                          scales=ss[:3] if ss is not None else None)
        out = ops.linear(a, pk[p + ".proj_out"], res=x.view(nb, n, c), math=math,
                         a_scale=ss[3] if ss is not None else None)
        return out.view(nb, d, h, w, c)

    @torch.no_grad()
    def decoder_ndhwc(self, z: Tensor) -> Tensor:
        """Decoder3D.forward (vqvae_modules.py:376-409) on [nb,d,h,w,4] -> [nb,4d,4h,4w,out_ch]."""
        sd, pk = self._sd, self._packed
        D = "decoder."
        nres = len(self.cfg["ch_mult"])
        h = ops.conv_gemm(z, pk[D + "conv_in"], math=self.math, stats="invariant")
        h = self._res(D + "mid.block_1", h)
        h = self._attn(D + "mid.attn_1", h)
        h = self._res(D + "mid.block_2", h)
        for i_level in reversed(range(nres)):
            for i_block in range(self.cfg["num_res_blocks"]):
                h = self._res(f"{D}up.{i_level}.block.{i_block}", h)
            if i_level != 0:
                h = ops.conv_gemm(h, pk[f"{D}up.{i_level}.upsample.conv"], up=(1, 1, 1), math=self.math)
        c = h.shape[-1]
        so = self._nas(D + "norm_out", h.shape[1] * h.shape[2] * h.shape[3] * (c // _vq_groups(c)))
        h = ops.groupnorm(h, sd[D + "norm_out.weight"], sd[D + "norm_out.bias"], _vq_groups(c), 1e-6, L.ACT_GELU,
                          split16=ops.wants_split16(h.shape[0] * h.shape[1] * h.shape[2] * h.shape[3], pk[D + "conv_out"]),
                          a_scale=so)
        return ops.conv_gemm(h, pk[D + "conv_out"], math=self.math, a_scale=so)

    # ---- reference API ----
    @torch.no_grad()
    def quantize(self, h: Tensor) -> Tuple[Tensor, Tensor]:
        """VectorQuantizer.forward(is_voxel=True) value path: (quant NCDHW, indices)."""
        zl = ops.nchw_to_ndhwc(h.to(torch.float32), cpad=4)
        idx, zq = ops.vq_lookup(zl, self._sd["quantize.embedding.weight"])
        return ops.ndhwc_to_nchw(zq, c=self.embed_dim), idx

    # Objects decode independently; a 64^3 x 128-channel activation is 134 MB per object (4.3 GB at 32), so large
    # batches are decoded in slices of this many, which bounds the workspace.
    MAX_DECODE_BATCH = 16

    @torch.no_grad()
    def decode(self, quant: Tensor) -> Tensor:
        """network.py:90-93: post_quant_conv + decoder on an already-quantised latent (NCDHW)."""
        if self._packed is None:
            self._pack()
        if quant.shape[0] > self.MAX_DECODE_BATCH:
            return torch.cat([self.decode(quant[i:i + self.MAX_DECODE_BATCH])
                              for i in range(0, quant.shape[0], self.MAX_DECODE_BATCH)], dim=0)
        zl = ops.nchw_to_ndhwc(quant.to(torch.float32), cpad=4)
        return self._decode_cl(zl)

    def _decode_cl(self, zl: Tensor) -> Tensor:
        q4 = ops.conv_gemm(zl, self._packed["post_quant_conv"], math=self.math)   # [nb,d,h,w,4], channel 3 == 0
        return ops.ndhwc_to_nchw(self.decoder_ndhwc(q4))

    @torch.no_grad()
    def decode_no_quant(self, h: Tensor, force_not_quantize: bool = False) -> Tensor:
        """network.py:95-103: (despite the name) quantise to the nearest code, then decode."""
        if self._packed is None:
            self._pack()
        if h.shape[0] > self.MAX_DECODE_BATCH:
            outs, idxs = [], []
            for i in range(0, h.shape[0], self.MAX_DECODE_BATCH):
                outs.append(self.decode_no_quant(h[i:i + self.MAX_DECODE_BATCH], force_not_quantize))
                if not force_not_quantize:
                    idxs.append(self.last_indices)
            if idxs:
                self.last_indices = torch.cat(idxs)
            return torch.cat(outs, dim=0)
        zl = ops.nchw_to_ndhwc(h.to(torch.float32), cpad=4)
        if not force_not_quantize:
            idx, zl = ops.vq_lookup(zl, self._sd["quantize.embedding.weight"])
            self.last_indices = idx
        return self._decode_cl(zl)

    # ---- encode side ----
    def _enc_tables(self, math: int) -> _Tables:
        T = self._epk.get(math)
        if T is not None:
            return T
        esd = self._esd
        if not esd:
            raise RuntimeError("VQVAE: no encoder weights -- encode needs a state_dict with the complete encoder.* and "
                               "quant_conv.* set (a decode-only checkpoint cannot encode)")
        g = (lambda k, d=None: self.ddconfig.get(k, d)) if isinstance(self.ddconfig, dict) else (
            lambda k, d=None: getattr(self.ddconfig, k, d))
        if bool(g("double_z", True)):
            raise NotImplementedError("double_z=True: conv_out emits 2 * z_channels, which quant_conv cannot take "
                                      "(config/vqvae_snet.yaml sets double_z: False)")
        pk = {}
        E = "encoder."
        for k in self.enc_shapes:
            if not (k.endswith(".weight") and esd[k].dim() == 5):
                continue
            p = k[:-7]
            w, b = esd[k], esd[p + ".bias"]
            if p.startswith(E + "mid.attn_1.") and p.split(".")[-1] in ("q", "k", "v"):
                continue
            if p == E + "conv_in" and w.shape[1] == 1 and w.shape[0] % 4 == 0 and w.shape[0] <= 256:
                pk[p] = (w, b)              # raw: cs_vqenc_conv_in, the same kernel in both modes
                continue
            if p in (E + "conv_out", "quant_conv"):
                # a zero 4th output channel (and input channel): quant_conv and the quantiser read float4-aligned rows
                pad = (-w.shape[0]) % 4
                w = torch.cat([w, w.new_zeros((pad, *w.shape[1:]))], dim=0)
                b = torch.cat([b, b.new_zeros(pad)], dim=0)
                if p == "quant_conv":
                    pk[p] = ops.pack_weight(w, b, cin_pad=(w.shape[1] + 3) // 4 * 4, math=math)
                    continue
                if ops.tapcol_ok(w, math):
                    pk[p] = ops.pack_weight_tapcol(w, b)
                    continue
            cin = w.shape[1]
            pk[p] = ops.pack_weight(w, b, cin_pad=(cin + 3) // 4 * 4, math=math)
            if math == L.MATH_F16X3 and not p.endswith(".downsample.conv") and tuple(w.shape[2:]) == (3, 3, 3):
                ops.pack_weight_wino(pk[p], w)
        a = E + "mid.attn_1."
        wqkv = torch.cat([esd[a + "q.weight"], esd[a + "k.weight"], esd[a + "v.weight"]], dim=0)
        bqkv = torch.cat([esd[a + "q.bias"], esd[a + "k.bias"], esd[a + "v.bias"]], dim=0)
        pk[a + "qkv"] = ops.pack_weight(wqkv, bqkv, math=math)
        attn_stat, ngb = None, {}
        if math == L.MATH_F16X3:
            c_ = int(esd[a + "q.weight"].shape[0])
            l2, _ = ops.weight_rowstats([esd[a + f"{n}.weight"].reshape(c_, -1) for n in ("q", "k", "v")])
            _, bm = ops.weight_rowstats([esd[a + f"{n}.bias"].reshape(1, -1) for n in ("q", "k", "v")])
            attn_stat = (l2, bm)
            norms = [k[:-7] for k in esd if k.startswith(E) and k.endswith(".weight") and esd[k].dim() == 1]
            mx = torch.stack([torch.stack([esd[n + ".weight"].abs().max(), esd[n + ".bias"].abs().max()])
                              for n in norms]).cpu()
            ngb = {n: (float(mx[i, 0]), float(mx[i, 1])) for i, n in enumerate(norms)}
        T = self._epk[math] = _Tables(esd, pk, math, ngb, attn_stat)
        return T

    @torch.no_grad()
    def encoder_ndhwc(self, x: Tensor, math: Optional[int] = None) -> Tensor:
        """Encoder3D.forward (vqvae_modules.py:263-290) + quant_conv on NCDHW [nb,1,D,H,W] -> [nb,D/4,H/4,W/4,4] (channel
        3 zero)."""
        T = self._enc_tables(self.math if math is None else math)
        sd, pk = T.sd, T.pk
        E = "encoder."
        nres = len(self.cfg["ch_mult"])
        ci = pk[E + "conv_in"]
        if isinstance(ci, tuple):
            h = ops.vqenc_conv_in(x, ci[0], ci[1])
        else:
            h = ops.conv_gemm(ops.nchw_to_ndhwc(x, cpad=ci.cin_pad), ci, math=T.math)
        for i_level in range(nres):
            for i_block in range(self.cfg["num_res_blocks"]):
                h = self._res(f"{E}down.{i_level}.block.{i_block}", h, T)
            if i_level != nres - 1:
                h = ops.conv_gemm(h, pk[f"{E}down.{i_level}.downsample.conv"], stride=(2, 2, 2), pad=_DOWN_PAD,
                                  math=T.math)
        h = self._res(E + "mid.block_1", h, T)
        h = self._attn(E + "mid.attn_1", h, T)
        h = self._res(E + "mid.block_2", h, T)
        c = h.shape[-1]
        so = self._nas(E + "norm_out", h.shape[1] * h.shape[2] * h.shape[3] * (c // _vq_groups(c)), T)
        h = ops.groupnorm(h, sd[E + "norm_out.weight"], sd[E + "norm_out.bias"], _vq_groups(c), 1e-6, L.ACT_GELU,
                          split16=ops.wants_split16(h.shape[0] * h.shape[1] * h.shape[2] * h.shape[3], pk[E + "conv_out"]),
                          a_scale=so)
        h = ops.conv_gemm(h, pk[E + "conv_out"], math=T.math, a_scale=so)
        return ops.conv_gemm(h, pk["quant_conv"], math=T.math)

    # Objects encode independently; one 64^3 x 64-channel activation is 67 MB per object, so large batches run in slices
    # of this many (as decode)
    MAX_ENCODE_BATCH = 16

    def _encode_cl(self, x: Tensor, quantize: bool):
        """One call's encode under the F16X3 range rule: status cleared, run, read back once; on overflow re-run on
        fp32-packed encoder weights (overflow_policy 'fp32', with a warning) or raise CsOverflowError ('raise')."""
        if x.dim() != 5 or x.shape[1] != int(self.enc_shapes["encoder.conv_in.weight"][1]):
            raise ValueError(f"encode expects NCDHW [nb, {self.enc_shapes['encoder.conv_in.weight'][1]}, D, H, W], "
                             f"got {tuple(x.shape)}")
        self._enc_tables(self.math)                 # (raises without encoder weights)
        x = x.to(device=self.device, dtype=torch.float32).contiguous()

        def run(math):
            outs = []
            for i in range(0, x.shape[0], self.MAX_ENCODE_BATCH):
                xs = x[i:i + self.MAX_ENCODE_BATCH]
                z = self.encoder_ndhwc(xs, math)
                if quantize:
                    idx, zst, part = ops.vq_quantize_st(z, self._sd["quantize.embedding.weight"], xs.shape[0])
                    outs.append((ops.ndhwc_to_nchw(zst, c=self.embed_dim), idx, part))
                else:
                    outs.append((ops.ndhwc_to_nchw(z, c=self.embed_dim),))
            return [torch.cat(t, dim=0) if len(t) > 1 else t[0] for t in zip(*outs)]

        ops.clear_status(self.device)
        res = run(self.math)
        if self.math == L.MATH_F16X3:
            try:
                ops.check_overflow(self.device, "VQ-VAE encode")
            except L.CsOverflowError:
                if self.overflow_policy != "fp32":
                    raise
                import warnings
                warnings.warn("F16X3 activation overflow in the VQ-VAE encoder: re-running this call on fp32-packed "
                              "encoder weights")
                res = run(L.MATH_FP32)
        return res

    @torch.no_grad()
    def encode_no_quant(self, x: Tensor) -> Tensor:
        """network.py:84-88: encoder + quant_conv -> h NCDHW [nb, embed_dim, D/4, H/4, W/4]."""
        return self._encode_cl(x, quantize=False)[0]

    @torch.no_grad()
    def encode(self, x: Tensor):
        """network.py:78-82: (quant, emb_loss, (None, None, indices)) -- quant = z + (z_q - z) (straight-through value),
        emb_loss = beta * mean + mean of (z_q - z)^2 with beta = 1 (quantizer.py:89-95, legacy=False), indices int64
        [nb * D/4 * H/4 * W/4]."""
        quant, idx, part = self._encode_cl(x, quantize=True)
        mean = float(part.sum()) / float(idx.numel() * self.embed_dim)
        emb_loss = torch.tensor(1.0 * mean + mean, dtype=torch.float32, device=self.device)
        self.last_indices = idx
        return quant, emb_loss, (None, None, idx)

    @torch.no_grad()
    def forward(self, input: Tensor, verbose: bool = False, forward_no_quant: bool = False, encode_only: bool = False):
        """network.py:123-140."""
        if forward_no_quant:
            z = self.encode_no_quant(input)
            if encode_only:
                return z
            dec = self.decode_no_quant(z)
            return dec, z
        quant, diff, info = self.encode(input)
        dec = self.decode(quant)
        if verbose:
            return dec, quant, diff, info
        return dec, diff

    __call__ = forward


def load_vqvae(vq_conf, vq_ckpt: str, opt=None, device: Optional[str] = None) -> VQVAE:
    """model/model_utils.py:7-31.  Accepts a raw state_dict or {'vqvae': state_dict}."""
    mp = vq_conf["model"]["params"] if isinstance(vq_conf, dict) else vq_conf.model.params
    g = (lambda o, k: o[k]) if isinstance(mp, dict) else getattr
    dev = device or (opt.hyper.device if opt is not None else "cuda")
    vq = VQVAE(g(mp, "ddconfig"), g(mp, "n_embed"), g(mp, "embed_dim"), device=dev)
    sd = torch.load(vq_ckpt, map_location="cpu")
    vq.load_state_dict(sd["vqvae"] if "vqvae" in sd else sd)     # (keeps the encoder when the checkpoint has it)
    return vq.eval()
