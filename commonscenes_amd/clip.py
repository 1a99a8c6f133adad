"""OpenAI CLIP ViT-B/32 (clip/model.py) on the HIP library: `encode_image` for the CLIP half of
scripts/consistency_check.py (:58-66, :82-90) and `encode_text` for the 512-wide class-name / relation-word rows the dataset
computes when a scene's CLIP_*.pkl is missing or a relationship is edited (dataset/threedfront_dataset.py:462-490, :758-763).

Both towers share one residual block, x + out_proj(attn(in_proj(ln_1 x))) then x + c_proj(quick_gelu(c_fc(ln_2 x))).  The
linear layers are the fp32-input MFMA GEMM (ops.pack_weight / ops.linear on MATH_FP32, the residual in its epilogue), the
norms ops.layernorm, the vision tower's attention ops.attention on MATH_FP32 over views of the fused q|k|v output; the front
ends, QuickGELU, the text tower's causal attention and the pooling are csrc/cs_clip.hip.  There is no PyTorch fallback.

What is NOT here: a tokenizer.  `clip.tokenize` / `transformers.CLIPTokenizer` need vocabulary files this package does not
ship; `encode_text` takes token ids and `text_feature_fn` takes the caller's tokenizer.  No real CLIP checkpoint has been
loaded by this code's tests: the key layout and the size inference follow clip/model.py (build_model) and are pinned to
`transformers`' CLIP through tools/make_clip_goldens.py on synthetic weights.  The reference runs CLIP in fp16 on the GPU;
this is an fp32 forward, so a table differs from the reference's in the low digits.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

from . import lib as L
from . import ops

Tensor = torch.Tensor

# clip/clip.py:_transform: Normalize((0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)), as the fp32
# values the kernel receives
CLIP_MEAN = tuple(float(np.float32(v)) for v in (0.48145466, 0.4578275, 0.40821073))
CLIP_STD = tuple(float(np.float32(v)) for v in (0.26862954, 0.26130258, 0.27577711))
LN_EPS = 1e-5
HEAD_DIM = 64                     # build_model: heads = width // 64 in both towers


# ----------------------------------------------------------------------------------------------------------------------
# sizes from shapes (clip/model.py:build_model)
# ----------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class VisionConfig:
    width: int
    layers: int
    heads: int
    patch: int
    grid: int
    embed: int

    @property
    def resolution(self) -> int:
        return self.patch * self.grid


@dataclass(frozen=True)
class TextConfig:
    width: int
    layers: int
    heads: int
    embed: int
    context: int
    vocab: int


def _shape(sd, key) -> tuple:
    if key not in sd:
        raise KeyError(f"CLIP state dict: missing key {key!r}")
    return tuple(int(v) for v in sd[key].shape)


def _layers(sd, prefix: str) -> int:
    ids = {int(k[len(prefix):].split(".")[0]) for k in sd if k.startswith(prefix)}
    if not ids:
        raise KeyError(f"CLIP state dict: missing key {prefix + '0.ln_1.weight'!r}")
    if ids != set(range(len(ids))):
        raise KeyError(f"CLIP state dict: missing key {prefix + str(min(set(range(max(ids) + 1)) - ids)) + '.ln_1.weight'!r}")
    return len(ids)


def _block_shapes(prefix: str, width: int) -> Dict[str, tuple]:
    w = width
    return {f"{prefix}ln_1.weight": (w,), f"{prefix}ln_1.bias": (w,),
            f"{prefix}attn.in_proj_weight": (3 * w, w), f"{prefix}attn.in_proj_bias": (3 * w,),
            f"{prefix}attn.out_proj.weight": (w, w), f"{prefix}attn.out_proj.bias": (w,),
            f"{prefix}ln_2.weight": (w,), f"{prefix}ln_2.bias": (w,),
            f"{prefix}mlp.c_fc.weight": (4 * w, w), f"{prefix}mlp.c_fc.bias": (4 * w,),
            f"{prefix}mlp.c_proj.weight": (w, 4 * w), f"{prefix}mlp.c_proj.bias": (w,)}


def vision_shapes(cfg: VisionConfig) -> Dict[str, tuple]:
    """every vision-tower key of OpenAI's layout with its shape"""
    w = cfg.width
    out = {"visual.conv1.weight": (w, 3, cfg.patch, cfg.patch), "visual.class_embedding": (w,),
           "visual.positional_embedding": (cfg.grid * cfg.grid + 1, w),
           "visual.ln_pre.weight": (w,), "visual.ln_pre.bias": (w,)}
    for i in range(cfg.layers):
        out.update(_block_shapes(f"visual.transformer.resblocks.{i}.", w))
    out.update({"visual.ln_post.weight": (w,), "visual.ln_post.bias": (w,), "visual.proj": (w, cfg.embed)})
    return out


def text_shapes(cfg: TextConfig) -> Dict[str, tuple]:
    """every text-tower key of OpenAI's layout with its shape"""
    w = cfg.width
    out = {"token_embedding.weight": (cfg.vocab, w), "positional_embedding": (cfg.context, w)}
    for i in range(cfg.layers):
        out.update(_block_shapes(f"transformer.resblocks.{i}.", w))
    out.update({"ln_final.weight": (w,), "ln_final.bias": (w,), "text_projection": (w, cfg.embed)})
    return out


def _validate(sd, shapes: Dict[str, tuple]) -> None:
    for key, want in shapes.items():
        got = _shape(sd, key)
        if got != want:
            raise ValueError(f"CLIP state dict: {key!r} has shape {got}, expected {want}")


def infer_config(sd) -> tuple:
    """(VisionConfig | None, TextConfig | None) from the shapes of a state dict in OpenAI's key layout -- what
    clip/model.py:build_model does: width from conv1 / ln_final, layers from the keys, patch from conv1, grid from the
    positional table, heads = width // 64.  Only shapes are read (meta tensors will do).  A tower none of whose keys are
    present is None; a tower that is partly there raises, naming the key."""
    vis = txt = None
    if any(k.startswith("visual.") for k in sd):
        s = _shape(sd, "visual.conv1.weight")
        if len(s) != 4 or s[1] != 3 or s[2] != s[3]:
            raise ValueError(f"CLIP state dict: 'visual.conv1.weight' has shape {s}, expected (width, 3, patch, patch)")
        width, patch = s[0], s[3]
        pos = _shape(sd, "visual.positional_embedding")
        grid = int(round((pos[0] - 1) ** 0.5))
        if len(pos) != 2 or grid < 1 or grid * grid + 1 != pos[0]:
            raise ValueError(f"CLIP state dict: 'visual.positional_embedding' has shape {pos}, expected (grid^2 + 1, {width})")
        proj = _shape(sd, "visual.proj")
        if len(proj) != 2:
            raise ValueError(f"CLIP state dict: 'visual.proj' has shape {proj}, expected ({width}, embed)")
        if width % HEAD_DIM:
            raise ValueError(f"CLIP state dict: 'visual.conv1.weight' gives width {width}, not a multiple of {HEAD_DIM}")
        vis = VisionConfig(width, _layers(sd, "visual.transformer.resblocks."), width // HEAD_DIM, patch, grid, proj[1])
        _validate(sd, vision_shapes(vis))
    text_keys = ("token_embedding.weight", "positional_embedding", "ln_final.weight", "ln_final.bias", "text_projection")
    if any(k in sd for k in text_keys) or any(k.startswith("transformer.resblocks.") for k in sd):
        s = _shape(sd, "ln_final.weight")
        width = s[0]
        tok, pos, proj = _shape(sd, "token_embedding.weight"), _shape(sd, "positional_embedding"), _shape(sd, "text_projection")
        if len(tok) != 2 or len(pos) != 2:
            raise ValueError(f"CLIP state dict: 'token_embedding.weight' has shape {tok}, expected (vocab, {width})")
        if len(proj) != 2:
            raise ValueError(f"CLIP state dict: 'text_projection' has shape {proj}, expected ({width}, embed)")
        if width % HEAD_DIM:
            raise ValueError(f"CLIP state dict: 'ln_final.weight' gives width {width}, not a multiple of {HEAD_DIM}")
        txt = TextConfig(width, _layers(sd, "transformer.resblocks."), width // HEAD_DIM, proj[1], pos[0], tok[0])
        _validate(sd, text_shapes(txt))
    if vis is None and txt is None:
        raise KeyError("CLIP state dict: missing key 'visual.conv1.weight' (and no text tower either)")
    return vis, txt


# ----------------------------------------------------------------------------------------------------------------------
# kernel front ends (csrc/cs_clip.hip)
# ----------------------------------------------------------------------------------------------------------------------
def patchify(images: Tensor, patch: int) -> Tensor:
    """uint8 [B, S, S, 3] -> fp32 patch rows [B * G * G, 3 * P * P], normalised as CLIP's preprocess does"""
    ops._chk(images, "images", torch.uint8)
    if images.dim() != 4 or images.shape[3] != 3 or images.shape[1] != images.shape[2]:
        raise L.CsError(f"images must be uint8 [B, S, S, 3], got {tuple(images.shape)}")
    b, s = int(images.shape[0]), int(images.shape[1])
    if patch < 1 or s % patch:
        raise L.CsError(f"cs_clip_patchify failed: invalid argument (image size {s} is no multiple of the patch {patch})")
    g = s // patch
    images = images.contiguous()
    out = torch.empty((b * g * g, 3 * patch * patch), dtype=torch.float32, device=images.device)
    L.check(L.load().cs_clip_patchify(images.data_ptr(), out.data_ptr(), b, s, patch, out.shape[1], *CLIP_MEAN,
                                      *CLIP_STD, ops._stream()), "cs_clip_patchify")
    return out


def assemble_image_tokens(patch_out: Tensor, class_embedding: Tensor, pos: Tensor, nb: int) -> Tensor:
    """patch_out [B * G * G, W], class_embedding [W], pos [G * G + 1, W] -> x [B, G * G + 1, W]"""
    for t, n in ((patch_out, "patch_out"), (class_embedding, "class_embedding"), (pos, "pos")):
        ops._chk(t, n)
    m, w, ldp = ops.rows_ld(patch_out, "patch_out")
    ntok = int(pos.shape[0]) - 1
    if m != nb * ntok or tuple(pos.shape) != (ntok + 1, w) or tuple(class_embedding.shape) != (w,):
        raise L.CsError("assemble_image_tokens: shape mismatch")
    class_embedding, pos = class_embedding.contiguous(), pos.contiguous()
    x = torch.empty((nb, ntok + 1, w), dtype=torch.float32, device=patch_out.device)
    L.check(L.load().cs_clip_assemble_image_tokens(patch_out.data_ptr(), class_embedding.data_ptr(),
                                                   pos.data_ptr(), x.data_ptr(), nb, ntok, w, ldp, w,
                                                   ops._stream()), "cs_clip_assemble_image_tokens")
    return x


def _ids32(ids, device) -> Tensor:
    t = ids if isinstance(ids, torch.Tensor) else torch.as_tensor(np.asarray(ids))
    if t.is_floating_point() or t.dtype == torch.bool or t.dim() != 2:
        raise L.CsError(f"token ids must be an integer [B, T] table, got {t.dtype} {tuple(t.shape)}")
    return t.to(device=device, dtype=torch.int32).contiguous()


def embed_text(token_embedding: Tensor, ids: Tensor, pos: Tensor) -> Tensor:
    """x[b, t] = token_embedding[ids[b, t]] + pos[t]; ids int32 [B, T] on the device.  An id outside the vocabulary gives a
    NaN row and sets ops.index_err_word() (ops.check_index_errors raises for it); nothing is read through it."""
    ops._chk(token_embedding, "token_embedding")
    ops._chk(pos, "pos")
    ops._chk(ids, "ids", torch.int32)
    vocab, w = (int(v) for v in token_embedding.shape)
    b, t = (int(v) for v in ids.shape)
    if pos.dim() != 2 or pos.shape[0] < t or pos.shape[1] != w:
        raise L.CsError(f"embed_text: {t} tokens but the positional table is {tuple(pos.shape)}")
    token_embedding, ids, pos = token_embedding.contiguous(), ids.contiguous(), pos.contiguous()
    x = torch.empty((b, t, w), dtype=torch.float32, device=token_embedding.device)
    L.check(L.load().cs_clip_embed_text(token_embedding.data_ptr(), ids.data_ptr(),
                                        pos.data_ptr(), x.data_ptr(), b, t, w, vocab, w,
                                        ops.index_err_word(x.device).data_ptr(), ops._stream()), "cs_clip_embed_text")
    return x


def quick_gelu(x: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """x * sigmoid(1.702 x); `out` may be `x`"""
    ops._chk(x, "x")
    m, c, ldx = ops.rows_ld(x, "x")
    if out is None:
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    ops._chk(out, "out")
    om, oc, ldy = ops.rows_ld(out, "out")
    if (om, oc) != (m, c):
        raise L.CsError("quick_gelu: out shape mismatch")
    L.check(L.load().cs_clip_quick_gelu(x.data_ptr(), out.data_ptr(), m, c, ldx, ldy, ops._stream()), "cs_clip_quick_gelu")
    return out


def attn_causal(q: Tensor, k: Tensor, v: Tensor, heads: int, scale: float, out: Optional[Tensor] = None) -> Tensor:
    """q, k, v: [B, T, heads * dh] (views with a wider row stride allowed): query i attends to keys j <= i"""
    for t, n in ((q, "q"), (k, "k"), (v, "v")):
        ops._chk(t, n)
        if t.dim() != 3 or t.shape != q.shape:
            raise L.CsError(f"{n} must be [B, T, heads * dh] like q")
    nb, t_len, c = (int(s) for s in q.shape)
    if heads < 1 or c % heads:
        raise L.CsError(f"attn_causal: {c} columns do not split into {heads} heads")
    _, _, ldq = ops.rows_ld(q, "q")
    _, _, ldk = ops.rows_ld(k, "k")
    _, _, ldv = ops.rows_ld(v, "v")
    if out is None:
        out = torch.empty((nb, t_len, c), dtype=torch.float32, device=q.device)
    _, _, ldo = ops.rows_ld(out, "out")
    L.check(L.load().cs_clip_attn_causal(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), nb, t_len, heads, c // heads,
                                         ldq, ldk, ldv, ldo, float(scale), ops._stream()), "cs_clip_attn_causal")
    return out


def pool_eot(x: Tensor, ids: Tensor) -> Tensor:
    """x [B, T, W], ids int32 [B, T] -> [B, W]: the row at the first maximum of ids[b, :] (the end-of-text token)"""
    ops._chk(x, "x")
    ops._chk(ids, "ids", torch.int32)
    b, t, w = (int(s) for s in x.shape)
    if tuple(ids.shape) != (b, t):
        raise L.CsError("pool_eot: ids must be [B, T] like x")
    _, _, ldx = ops.rows_ld(x, "x")
    ids = ids.contiguous()
    out = torch.empty((b, w), dtype=torch.float32, device=x.device)
    L.check(L.load().cs_clip_pool_eot(x.data_ptr(), ids.data_ptr(), out.data_ptr(), b, t, w, ldx, w, ops._stream()),
            "cs_clip_pool_eot")
    return out


def feature_pair_l2(features: Tensor, pairs, check_indices: bool = True) -> Tensor:
    """dist[k] = ||features[pairs[k, 0]] - features[pairs[k, 1]]||_2 in one launch (torch.norm(a - b),
    consistency_check.py:65).  pairs [P, 2]: a host-side integer table (range-checked here) or an int32 device tensor
    (`check_indices` then costs one read-back; without it a bad entry gives NaN and sets ops.index_err_word())."""
    what = "feature_pair_l2"
    ops._chk(features, "features")
    if features.dim() != 2 or features.shape[0] < 1 or features.shape[1] < 1:
        raise L.CsError(f"{what}: features must be a non-empty [N, E] tensor")
    n, e, ld = ops.rows_ld(features, "features")
    on_dev = isinstance(pairs, torch.Tensor) and pairs.is_cuda
    if not on_dev:
        pairs_h = ops._host_ints(pairs, "pairs", what)
        if pairs_h.numel() == 0:
            pairs_h = pairs_h.reshape(0, 2)
        if pairs_h.dim() != 2 or pairs_h.shape[1] != 2:
            raise L.CsError(f"{what}: pairs must be [npairs, 2], got {tuple(pairs_h.shape)}")
        if pairs_h.numel() and (int(pairs_h.min()) < 0 or int(pairs_h.max()) >= n):
            raise L.CsError(f"{what} failed: invalid argument (a pair outside [0, {n}))")
        pairs = pairs_h.to(torch.int32).to(features.device)
    else:
        if pairs.dtype != torch.int32 or pairs.dim() != 2 or pairs.shape[1] != 2:
            raise L.CsError(f"{what}: device pairs must be int32 [npairs, 2], got {pairs.dtype} {tuple(pairs.shape)}")
        pairs = pairs.contiguous()
        if check_indices and pairs.numel() and not ops._index_range_ok(pairs, n):
            raise L.CsError(f"{what} failed: invalid argument (a pair outside [0, {n}))")
    npairs = int(pairs.shape[0])
    out = torch.empty((npairs,), dtype=torch.float32, device=features.device)
    if npairs == 0:
        return out
    L.check(L.load().cs_feature_pair_l2(features.data_ptr(), pairs.data_ptr(), out.data_ptr(), n, e, npairs, ld,
                                        ops.index_err_word(features.device).data_ptr(), ops._stream()), "cs_feature_pair_l2")
    return out


# ----------------------------------------------------------------------------------------------------------------------
# the model
# ----------------------------------------------------------------------------------------------------------------------
@dataclass
class _Block:
    ln1: tuple
    in_proj: ops.PackedWeight
    out_proj: ops.PackedWeight
    ln2: tuple
    c_fc: ops.PackedWeight
    c_proj: ops.PackedWeight


class CLIP:
    """Both towers of CLIP over the HIP library, fp32.  `load_state_dict` takes OpenAI's key layout -- what
    `torch.jit.load("ViT-B-32.pt").state_dict()` or `clip.load(...)[0].state_dict()` give; fp16 tensors are upcast -- and
    infers every size from the shapes.  Either tower may be absent; calling its encoder then raises."""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        self.vision: Optional[VisionConfig] = None
        self.text: Optional[TextConfig] = None
        self._v: dict = {}
        self._t: dict = {}

    # -- weights ---------------------------------------------------------------------------------------------------------
    def _blocks(self, get, prefix: str, layers: int) -> List[_Block]:
        out = []
        for i in range(layers):
            p = f"{prefix}{i}."
            lin = lambda w, b: ops.pack_weight(get(p + w), get(p + b), math=L.MATH_FP32)
            out.append(_Block((get(p + "ln_1.weight"), get(p + "ln_1.bias")),
                              lin("attn.in_proj_weight", "attn.in_proj_bias"),
                              lin("attn.out_proj.weight", "attn.out_proj.bias"),
                              (get(p + "ln_2.weight"), get(p + "ln_2.bias")),
                              lin("mlp.c_fc.weight", "mlp.c_fc.bias"), lin("mlp.c_proj.weight", "mlp.c_proj.bias")))
        return out

    def load_state_dict(self, sd) -> "CLIP":
        vis, txt = infer_config(sd)              # raises KeyError / ValueError naming the key
        get = lambda k: sd[k].detach().to(device=self.device, dtype=torch.float32).contiguous()
        self._v, self._t = {}, {}
        if vis is not None:
            if vis.width % 4 or vis.embed % 4:
                raise ValueError(f"CLIP state dict: 'visual.proj' {vis.width} x {vis.embed}: the GEMM needs multiples of 4")
            self._v = dict(
                conv1=ops.pack_weight(get("visual.conv1.weight").reshape(vis.width, -1), None, math=L.MATH_FP32),
                cls=get("visual.class_embedding"), pos=get("visual.positional_embedding"),
                ln_pre=(get("visual.ln_pre.weight"), get("visual.ln_pre.bias")),
                blocks=self._blocks(get, "visual.transformer.resblocks.", vis.layers),
                ln_post=(get("visual.ln_post.weight"), get("visual.ln_post.bias")),
                proj=ops.pack_weight(get("visual.proj").t().contiguous(), None, math=L.MATH_FP32))
        if txt is not None:
            if txt.embed % 4:
                raise ValueError(f"CLIP state dict: 'text_projection' {txt.width} x {txt.embed}: the GEMM needs multiples of 4")
            self._t = dict(
                tok=get("token_embedding.weight"), pos=get("positional_embedding"),
                blocks=self._blocks(get, "transformer.resblocks.", txt.layers),
                ln_final=(get("ln_final.weight"), get("ln_final.bias")),
                proj=ops.pack_weight(get("text_projection").t().contiguous(), None, math=L.MATH_FP32))
        self.vision, self.text = vis, txt
        return self

    # -- the shared block ------------------------------------------------------------------------------------------------
    @staticmethod
    def _block(x: Tensor, blk: _Block, heads: int, causal: bool) -> Tensor:
        w = int(x.shape[-1])
        scale = float(w // heads) ** -0.5
        qkv = ops.linear(ops.layernorm(x, *blk.ln1, eps=LN_EPS), blk.in_proj)
        q, k, v = qkv[..., :w], qkv[..., w:2 * w], qkv[..., 2 * w:]
        a = attn_causal(q, k, v, heads, scale) if causal else ops.attention(q, k, v, heads, scale, math=L.MATH_FP32)
        x = ops.linear(a, blk.out_proj, res=x)
        h = ops.linear(ops.layernorm(x, *blk.ln2, eps=LN_EPS), blk.c_fc)
        return ops.linear(quick_gelu(h, out=h), blk.c_proj, res=x)

    # -- encoders --------------------------------------------------------------------------------------------------------
    def encode_image(self, images) -> Tensor:
        """uint8 [B, S, S, 3] (HWC: what PIL, `preprocess` and tensor2im give) -> features [B, E]"""
        if self.vision is None:
            raise L.CsError("encode_image: no vision tower was loaded")
        cfg, p = self.vision, self._v
        images = images if isinstance(images, torch.Tensor) else torch.as_tensor(np.asarray(images))
        images = images.to(self.device)
        if images.dim() != 4 or tuple(images.shape[1:]) != (cfg.resolution, cfg.resolution, 3):
            raise L.CsError(f"encode_image: expected uint8 [B, {cfg.resolution}, {cfg.resolution}, 3], got {tuple(images.shape)}")
        nb = int(images.shape[0])
        x = assemble_image_tokens(ops.linear(patchify(images, cfg.patch), p["conv1"]), p["cls"], p["pos"], nb)
        x = ops.layernorm(x, *p["ln_pre"], eps=LN_EPS)
        for blk in p["blocks"]:
            x = self._block(x, blk, cfg.heads, causal=False)
        return ops.linear(ops.layernorm(x[:, 0, :], *p["ln_post"], eps=LN_EPS), p["proj"])

    def encode_text(self, ids, return_hidden: bool = False):
        """token ids [B, T] (T <= the context length; what the caller's tokenizer gives) -> features [B, E]: the hidden row
        at the end-of-text token (the first maximum of each id row) through ln_final and text_projection.
        return_hidden=True: (features, ln_final(hidden) [B, T, W])."""
        if self.text is None:
            raise L.CsError("encode_text: no text tower was loaded")
        cfg, p = self.text, self._t
        ids = _ids32(ids, self.device)
        if ids.shape[1] > cfg.context or ids.shape[0] < 1:
            raise L.CsError(f"encode_text: {tuple(ids.shape)} ids, the context length is {cfg.context}")
        x = embed_text(p["tok"], ids, p["pos"])
        for blk in p["blocks"]:
            x = self._block(x, blk, cfg.heads, causal=True)
        feats = ops.linear(ops.layernorm(pool_eot(x, ids), *p["ln_final"], eps=LN_EPS), p["proj"])
        hidden = ops.layernorm(x, *p["ln_final"], eps=LN_EPS) if return_hidden else None
        ops.check_index_errors(self.device, what="CLIP token ids")       # one read-back per call
        return (feats, hidden) if return_hidden else feats


# ----------------------------------------------------------------------------------------------------------------------
# host side
# ----------------------------------------------------------------------------------------------------------------------
def preprocess(images, size: int) -> Tensor:
    """PIL images (or paths) -> uint8 [B, S, S, 3]: clip/clip.py:_transform up to ToTensor with its own PIL calls in its own
    order -- Resize(S, BICUBIC) of the shorter side, CenterCrop(S), convert("RGB") -- so the pixels are the reference's; the
    division by 255 and the normalisation are cs_clip_patchify's."""
    from PIL import Image
    if isinstance(images, (str, bytes)) or hasattr(images, "__fspath__") or isinstance(images, Image.Image):
        images = [images]
    out = []
    for im in images:
        if not isinstance(im, Image.Image):
            with Image.open(im) as fh:
                im = fh.copy()
        w, h = im.size
        # torchvision.transforms.functional.resize with an int size: the shorter side becomes `size`, the longer one
        # int(size * long / short); an image that already fits is left alone
        short, long = (w, h) if w <= h else (h, w)
        if short != size:
            new_short, new_long = size, int(size * long / short)
            nw, nh = (new_short, new_long) if w <= h else (new_long, new_short)
            im = im.resize((nw, nh), Image.BICUBIC)
            w, h = nw, nh
        # torchvision center_crop
        top, left = int(round((h - size) / 2.0)), int(round((w - size) / 2.0))
        im = im.crop((left, top, left + size, top + size)).convert("RGB")
        out.append(torch.from_numpy(np.array(im, dtype=np.uint8)))
    return torch.stack(out)


def text_feature_fn(model: CLIP, tokenize: Callable) -> Callable:
    """The `rel_feat_fn` of manipulation.make_edit, and the encoder of threedfront_dataset.py:468-478: fn(words) with
    words a string -> fp32 CPU [E]; with a list of strings -> [n, E].  `tokenize` is the caller's: clip.tokenize (a [n, 77]
    tensor) or a transformers.CLIPTokenizer call (anything with `input_ids`).  No tokenizer is built here."""
    def fn(words):
        single = isinstance(words, str)
        tok = tokenize([words] if single else list(words))
        if not isinstance(tok, torch.Tensor) and hasattr(tok, "keys") and "input_ids" in tok.keys():
            tok = tok["input_ids"]
        feats = model.encode_text(torch.as_tensor(np.asarray(tok)) if not isinstance(tok, torch.Tensor) else tok).cpu()
        return feats[0] if single else feats
    return fn


def scene_text_features(fn: Callable, class_names: Sequence[str], words: Sequence[str]) -> dict:
    """threedfront_dataset.py:468-478 with `fn = text_feature_fn(...)`: the class-name rows (the caller appends 'room' for
    the scene node, as the reference does) and one row per relation sentence, in the layout of a scene's CLIP_*.pkl."""
    inst = fn(list(class_names)).numpy()
    rel = fn(list(words)).numpy() if len(words) else np.zeros((0, inst.shape[1]), np.float32)
    return {"instance_feats": inst, "rel_feats": {w: rel[i] for i, w in enumerate(words)}}


def _rs(x) -> float:
    return 1.0 / math.sqrt(float(x))          # correctly rounded operations only (no pow)


def _uniform(rng, shape, std: float) -> np.ndarray:
    """zero-mean uniform draws of standard deviation `std` from integers alone (exact on every machine: no libm)"""
    u = rng.integers(0, 1 << 24, size=shape, dtype=np.int64).astype(np.float64)
    return (((u + 0.5) / float(1 << 24) - 0.5) * (math.sqrt(12.0) * std)).astype(np.float32)


def synth_clip_state_dict(cfg: dict, seed: int) -> Dict[str, Tensor]:
    """Weights in OpenAI's key layout from numpy.random.default_rng(seed), scaled as clip/model.py initialises them
    (CLIP.initialize_parameters, VisionTransformer.__init__) so activations stay O(1) through 12 layers; the draws are
    uniform with those standard deviations and built from integers only, hence identical on every machine.  Biases and norm
    parameters, which CLIP starts at 0 / 1, are drawn too (std 0.02 around them) so that no term is trivially absent.
    cfg: {"vision": {width, layers, patch, grid, embed}, "text": {width, layers, context, vocab, embed}}, either optional.
    CPU fp32 tensors."""
    rng = np.random.default_rng(int(seed))
    sd: Dict[str, np.ndarray] = {}

    def blocks(prefix, width, layers):
        attn_std, proj_std, fc_std = _rs(width), _rs(width) * _rs(2 * layers), _rs(2 * width)
        for i in range(layers):
            p = f"{prefix}{i}."
            for ln in ("ln_1", "ln_2"):
                sd[p + ln + ".weight"] = 1.0 + _uniform(rng, (width,), 0.02)
                sd[p + ln + ".bias"] = _uniform(rng, (width,), 0.02)
            sd[p + "attn.in_proj_weight"] = _uniform(rng, (3 * width, width), attn_std)
            sd[p + "attn.in_proj_bias"] = _uniform(rng, (3 * width,), 0.02)
            sd[p + "attn.out_proj.weight"] = _uniform(rng, (width, width), proj_std)
            sd[p + "attn.out_proj.bias"] = _uniform(rng, (width,), 0.02)
            sd[p + "mlp.c_fc.weight"] = _uniform(rng, (4 * width, width), fc_std)
            sd[p + "mlp.c_fc.bias"] = _uniform(rng, (4 * width,), 0.02)
            sd[p + "mlp.c_proj.weight"] = _uniform(rng, (width, 4 * width), proj_std)
            sd[p + "mlp.c_proj.bias"] = _uniform(rng, (width,), 0.02)

    v = cfg.get("vision")
    if v:
        w, pt, g = int(v["width"]), int(v["patch"]), int(v["grid"])
        scale = _rs(w)
        sd["visual.conv1.weight"] = _uniform(rng, (w, 3, pt, pt), _rs(3 * pt * pt))
        sd["visual.class_embedding"] = _uniform(rng, (w,), scale)
        sd["visual.positional_embedding"] = _uniform(rng, (g * g + 1, w), scale)
        sd["visual.ln_pre.weight"] = 1.0 + _uniform(rng, (w,), 0.02)
        sd["visual.ln_pre.bias"] = _uniform(rng, (w,), 0.02)
        blocks("visual.transformer.resblocks.", w, int(v["layers"]))
        sd["visual.ln_post.weight"] = 1.0 + _uniform(rng, (w,), 0.02)
        sd["visual.ln_post.bias"] = _uniform(rng, (w,), 0.02)
        sd["visual.proj"] = _uniform(rng, (w, int(v["embed"])), scale)
    t = cfg.get("text")
    if t:
        w = int(t["width"])
        sd["token_embedding.weight"] = _uniform(rng, (int(t["vocab"]), w), 0.02)
        sd["positional_embedding"] = _uniform(rng, (int(t["context"]), w), 0.01)
        blocks("transformer.resblocks.", w, int(t["layers"]))
        sd["ln_final.weight"] = 1.0 + _uniform(rng, (w,), 0.02)
        sd["ln_final.bias"] = _uniform(rng, (w,), 0.02)
        sd["text_projection"] = _uniform(rng, (w, int(t["embed"])), _rs(w))
    return {k: torch.from_numpy(np.ascontiguousarray(a.astype(np.float32))) for k, a in sd.items()}


VIT_B_32 = {"vision": dict(width=768, layers=12, patch=32, grid=7, embed=512),
            "text": dict(width=512, layers=12, context=77, vocab=49408, embed=512)}


def load_checkpoint(path, device="cuda") -> CLIP:
    """MODEL.pt as OpenAI ships it (a TorchScript archive) or a pickled module / state dict -> CLIP"""
    try:
        sd = torch.jit.load(str(path), map_location="cpu").state_dict()
    except RuntimeError:
        obj = torch.load(str(path), map_location="cpu", weights_only=False)
        sd = obj.state_dict() if hasattr(obj, "state_dict") else obj.get("state_dict", obj)
    return CLIP(device).load_state_dict(sd)
