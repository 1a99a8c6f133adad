"""InceptionV3 pool3 features (2048 columns) on the HIP library: the default extractor of cleanfid's `compute_fid` /
`compute_kid`, i.e. the FID / KID columns scripts/compute_fid_scores_3dfront.py prints per room type.

This is the FID variant of the network (pytorch-fid's `FIDInceptionA / C / E_1 / E_2`): the average pools of the Mixed blocks
leave the padding out of the divisor and Mixed_7c pools with a maximum.  Every layer is BasicConv2d = conv without bias,
BatchNorm(eps 1e-3, eval mode) and ReLU; the architecture is the tables `STEM` and `BLOCKS` below.

How it runs: activations are NHWC fp32 carried as [B, 1, H, W, C]; every conv is ops.conv_gemm on an F16X3-packed weight with
kernel (1, kh, kw), the BatchNorm as the epilogue's scale / shift terms (the weights are packed as they are) and CS_ACT_RELU;
a branch's last conv writes straight into its channel range of the block's output buffer (out_fn), so no concatenation copy
exists.  The operand scale of every conv follows the tensor it reads: cs_absmax leaves max |x| in a device slot and the kernel
takes the scale from it (conv_gemm(x_bound=)), so no activation magnitude can leave the fp16 range; `features` still reads the
status word once at the end.  K is sliced by a rule of the layer alone (`k_slices`: at most 32 chunks of 16 channels per
slice, summed in slice order), never by the library's batch-dependent plan: the order of a conv's sum is the same in every
call and no fp32 accumulation chain is longer than 512 products.  The image front end and the pools are csrc/cs_incep.hip.
There is no PyTorch fallback.

State dict: torchvision's `Inception3` names as in pytorch-fid's pt_inception-2015-12-05 file -- `<layer>.conv.weight`
[cout, cin, kh, kw] and `<layer>.bn.{weight, bias, running_mean, running_var}`; `num_batches_tracked`, `fc.*` and
`AuxLogits.*` are ignored.

What is NOT here: the fc / logits head, cleanfid's `legacy_tensorflow` resize, a reader for the TorchScript
inception-2015-12-05.pt archive.  No real Inception weights have been loaded by this code's tests, cleanfid / pytorch-fid /
torchvision are not part of the build image, and parity with them is NOT pinned: the layer table, the two normalisation
constants and the resize rules are restated from those packages' published sources.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import lib as L
from . import ops

Tensor = torch.Tensor

BN_EPS = 1e-3            # BasicConv2d: nn.BatchNorm2d(eps=0.001)
SIZE = 299               # CS_INCEP_SIZE
CPAD = 4                 # channels of the front end's output: RGB + one zero (cs_conv_gemm wants cin % 4 == 0)
MIN_SIZE = 75            # the smallest input every stride-2 stage still maps to an extent >= 1
MODES = ("clean", "legacy_pytorch")


# ----------------------------------------------------------------------------------------------------------------------
# the architecture as data
# ----------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Conv:
    name: str
    cin: int
    cout: int
    k: Tuple[int, int] = (1, 1)          # (kh, kw)
    stride: int = 1
    pad: Tuple[int, int] = (0, 0)        # (ph, pw)


@dataclass(frozen=True)
class Pool:
    kind: str                            # "max" | "avg" (3 x 3; avg: stride 1, pad 1, padding left out of the divisor)
    stride: int = 1
    pad: int = 0


@dataclass(frozen=True)
class Fork:
    """two convs on the same input whose outputs are concatenated (Mixed_7b / 7c: 1x3 and 3x1)"""
    a: Conv
    b: Conv


def _block_a(n: str, cin: int, pf: int):
    return [[Conv(f"{n}.branch1x1", cin, 64)],
            [Conv(f"{n}.branch5x5_1", cin, 48), Conv(f"{n}.branch5x5_2", 48, 64, (5, 5), 1, (2, 2))],
            [Conv(f"{n}.branch3x3dbl_1", cin, 64), Conv(f"{n}.branch3x3dbl_2", 64, 96, (3, 3), 1, (1, 1)),
             Conv(f"{n}.branch3x3dbl_3", 96, 96, (3, 3), 1, (1, 1))],
            [Pool("avg", 1, 1), Conv(f"{n}.branch_pool", cin, pf)]]


def _block_b(n: str, cin: int):
    return [[Conv(f"{n}.branch3x3", cin, 384, (3, 3), 2)],
            [Conv(f"{n}.branch3x3dbl_1", cin, 64), Conv(f"{n}.branch3x3dbl_2", 64, 96, (3, 3), 1, (1, 1)),
             Conv(f"{n}.branch3x3dbl_3", 96, 96, (3, 3), 2)],
            [Pool("max", 2, 0)]]


def _block_c(n: str, cin: int, c7: int):
    row, col = dict(k=(1, 7), pad=(0, 3)), dict(k=(7, 1), pad=(3, 0))
    return [[Conv(f"{n}.branch1x1", cin, 192)],
            [Conv(f"{n}.branch7x7_1", cin, c7), Conv(f"{n}.branch7x7_2", c7, c7, **row), Conv(f"{n}.branch7x7_3", c7, 192, **col)],
            [Conv(f"{n}.branch7x7dbl_1", cin, c7), Conv(f"{n}.branch7x7dbl_2", c7, c7, **col),
             Conv(f"{n}.branch7x7dbl_3", c7, c7, **row), Conv(f"{n}.branch7x7dbl_4", c7, c7, **col),
             Conv(f"{n}.branch7x7dbl_5", c7, 192, **row)],
            [Pool("avg", 1, 1), Conv(f"{n}.branch_pool", cin, 192)]]


def _block_d(n: str, cin: int):
    return [[Conv(f"{n}.branch3x3_1", cin, 192), Conv(f"{n}.branch3x3_2", 192, 320, (3, 3), 2)],
            [Conv(f"{n}.branch7x7x3_1", cin, 192), Conv(f"{n}.branch7x7x3_2", 192, 192, (1, 7), 1, (0, 3)),
             Conv(f"{n}.branch7x7x3_3", 192, 192, (7, 1), 1, (3, 0)), Conv(f"{n}.branch7x7x3_4", 192, 192, (3, 3), 2)],
            [Pool("max", 2, 0)]]


def _block_e(n: str, cin: int, pool: str):
    fork = lambda p: Fork(Conv(f"{n}.{p}a", 384, 384, (1, 3), 1, (0, 1)), Conv(f"{n}.{p}b", 384, 384, (3, 1), 1, (1, 0)))
    return [[Conv(f"{n}.branch1x1", cin, 320)],
            [Conv(f"{n}.branch3x3_1", cin, 384), fork("branch3x3_2")],
            [Conv(f"{n}.branch3x3dbl_1", cin, 448), Conv(f"{n}.branch3x3dbl_2", 448, 384, (3, 3), 1, (1, 1)),
             fork("branch3x3dbl_3")],
            [Pool(pool, 1, 1), Conv(f"{n}.branch_pool", cin, 192)]]


# the stem: a plain sequence; then (name, branches) per Mixed block, each branch a sequence whose outputs are concatenated
STEM = [Conv("Conv2d_1a_3x3", 3, 32, (3, 3), 2), Conv("Conv2d_2a_3x3", 32, 32, (3, 3)),
        Conv("Conv2d_2b_3x3", 32, 64, (3, 3), 1, (1, 1)), Pool("max", 2, 0),
        Conv("Conv2d_3b_1x1", 64, 80), Conv("Conv2d_4a_3x3", 80, 192, (3, 3)), Pool("max", 2, 0)]
BLOCKS = [("Mixed_5b", _block_a("Mixed_5b", 192, 32)), ("Mixed_5c", _block_a("Mixed_5c", 256, 64)),
          ("Mixed_5d", _block_a("Mixed_5d", 288, 64)), ("Mixed_6a", _block_b("Mixed_6a", 288)),
          ("Mixed_6b", _block_c("Mixed_6b", 768, 128)), ("Mixed_6c", _block_c("Mixed_6c", 768, 160)),
          ("Mixed_6d", _block_c("Mixed_6d", 768, 160)), ("Mixed_6e", _block_c("Mixed_6e", 768, 192)),
          ("Mixed_7a", _block_d("Mixed_7a", 768)), ("Mixed_7b", _block_e("Mixed_7b", 1280, "avg")),
          ("Mixed_7c", _block_e("Mixed_7c", 2048, "max"))]


def _convs_of(seq) -> List[Conv]:
    out = []
    for op in seq:
        if isinstance(op, Conv):
            out.append(op)
        elif isinstance(op, Fork):
            out += [op.a, op.b]
    return out


def conv_layers() -> List[Conv]:
    """every conv layer of the network, in execution order"""
    out = _convs_of(STEM)
    for _, branches in BLOCKS:
        for br in branches:
            out += _convs_of(br)
    return out


def block_input_width(branches) -> int:
    first = branches[0][0]
    return first.cin


def branch_width(branch, cin: int) -> int:
    """output channels of one branch of a block whose input has `cin` channels (a pool keeps its input's)"""
    c = cin
    for op in branch:
        c = op.cout if isinstance(op, Conv) else op.a.cout + op.b.cout if isinstance(op, Fork) else c
    return c


def block_widths() -> Dict[str, List[int]]:
    """block name -> the widths of its branches in concatenation order"""
    return {name: [branch_width(br, block_input_width(branches)) for br in branches] for name, branches in BLOCKS}


def inception_shapes() -> Dict[str, tuple]:
    """every key the loader reads with its shape (torchvision's Inception3 names)"""
    out: Dict[str, tuple] = {}
    for c in conv_layers():
        out[f"{c.name}.conv.weight"] = (c.cout, c.cin, c.k[0], c.k[1])
        for p in ("weight", "bias", "running_mean", "running_var"):
            out[f"{c.name}.bn.{p}"] = (c.cout,)
    return out


def _validate(sd) -> None:
    for key, want in inception_shapes().items():
        if key not in sd:
            raise KeyError(f"Inception state dict: missing key {key!r}")
        got = tuple(int(v) for v in sd[key].shape)
        if got != want:
            raise ValueError(f"Inception state dict: {key!r} has shape {got}, expected {want}")


def fold_bn(weight: Tensor, bias: Tensor, mean: Tensor, var: Tensor, eps: float = BN_EPS) -> Tuple[Tensor, Tensor]:
    """eval-mode BatchNorm as y = x * scale + shift: scale = gamma / sqrt(var + eps), shift = beta - mean * scale, formed
    in fp64 (the caller rounds)."""
    scale = weight.double() / torch.sqrt(var.double() + float(eps))
    return scale, bias.double() - mean.double() * scale


# ----------------------------------------------------------------------------------------------------------------------
# kernel front ends (csrc/cs_incep.hip)
# ----------------------------------------------------------------------------------------------------------------------
def _nhwc(t: Tensor, name: str) -> Tuple[int, int, int, int, int]:
    """(nb, h, w, c, ld) of an fp32 device view [B, H, W, C] or [B, 1, H, W, C] whose rows are pixels"""
    ops._chk(t, name)
    if t.dim() == 5 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() != 4:
        raise L.CsError(f"{name}: expected [B, H, W, C] (or [B, 1, H, W, C]), got {tuple(t.shape)}")
    nb, h, w, c = (int(v) for v in t.shape)
    if min(nb, h, w, c) < 1:
        raise L.CsError(f"{name}: empty tensor {tuple(t.shape)}")
    m, _, ld = ops.rows_ld(t, name)
    if m != nb * h * w:
        raise L.CsError(f"{name}: not a row-strided layout {tuple(t.shape)} {t.stride()}")
    return nb, h, w, c, ld


def _pool_out(x: Tensor, oshape, out: Optional[Tensor], out_fn, name: str) -> Tensor:
    if out is None:
        out = out_fn(oshape) if out_fn is not None else torch.empty(oshape, dtype=torch.float32, device=x.device)
    if tuple(out.shape) != tuple(oshape):
        raise L.CsError(f"{name}: out has shape {tuple(out.shape)}, expected {tuple(oshape)}")
    return out


def _like(x: Tensor, nb: int, ho: int, wo: int, c: int) -> tuple:
    return (nb, 1, ho, wo, c) if x.dim() == 5 else (nb, ho, wo, c)


def max_pool3(x: Tensor, stride: int = 2, pad: int = 0, out: Optional[Tensor] = None, out_fn=None) -> Tensor:
    """F.max_pool2d(kernel 3, stride 1 | 2, padding 0 | 1) on NHWC; `out` / `out_fn` may place a channel slice"""
    nb, h, w, c, ldx = _nhwc(x, "x")
    if stride not in (1, 2) or pad not in (0, 1):
        raise L.CsError(f"cs_pool2d_max3 failed: invalid argument (stride {stride}, pad {pad})")
    ho, wo = (h + 2 * pad - 3) // stride + 1, (w + 2 * pad - 3) // stride + 1
    if h + 2 * pad < 3 or w + 2 * pad < 3:
        raise L.CsError(f"cs_pool2d_max3 failed: invalid argument ({h} x {w} input, pad {pad}: no output)")
    out = _pool_out(x, _like(x, nb, ho, wo, c), out, out_fn, "max_pool3")
    _, _, _, _, ldo = _nhwc(out, "out")
    L.check(L.load().cs_pool2d_max3(x.data_ptr(), out.data_ptr(), nb, h, w, c, ldx, ldo, int(stride), int(pad), ops._stream()),
            "cs_pool2d_max3")
    return out


def avg_pool3(x: Tensor, count_include_pad: bool = False, out: Optional[Tensor] = None, out_fn=None) -> Tensor:
    """F.avg_pool2d(kernel 3, stride 1, padding 1, count_include_pad=...) on NHWC"""
    nb, h, w, c, ldx = _nhwc(x, "x")
    out = _pool_out(x, _like(x, nb, h, w, c), out, out_fn, "avg_pool3")
    _, _, _, _, ldo = _nhwc(out, "out")
    L.check(L.load().cs_pool2d_avg3(x.data_ptr(), out.data_ptr(), nb, h, w, c, ldx, ldo, 1 if count_include_pad else 0,
                                    ops._stream()), "cs_pool2d_avg3")
    return out


def global_avg(x: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """[B, H, W, C] -> [B, C]: the mean over H x W (fp64 accumulation, one rounding); `out` may be a wider view"""
    nb, h, w, c, ldx = _nhwc(x, "x")
    if out is None:
        out = torch.empty((nb, c), dtype=torch.float32, device=x.device)
    ops._chk(out, "out")
    if tuple(out.shape) != (nb, c):
        raise L.CsError(f"global_avg: out has shape {tuple(out.shape)}, expected {(nb, c)}")
    _, _, ldo = ops.rows_ld(out, "out")
    L.check(L.load().cs_pool2d_global_avg(x.data_ptr(), out.data_ptr(), nb, h, w, c, ldx, ldo, ops._stream()),
            "cs_pool2d_global_avg")
    return out


def front_end(images: Tensor, norm: int, resize: bool = True, cpad: int = CPAD) -> Tensor:
    """uint8 [B, H, W, 3] (bilinear resize to 299 x 299 on the device when `resize`, else H = W = 299) or float32
    [B, 299, 299, 3] holding 0..255 values -> normalised fp32 [B, 299, 299, cpad], channels 3.. zero.
    norm 0: 2 (v / 255) - 1; norm 1: (v - 128) / 128."""
    if not isinstance(images, torch.Tensor) or not images.is_cuda:
        raise L.CsError("front_end: expected a HIP device tensor (the HIP path has no CPU fallback)")
    if images.dtype not in (torch.uint8, torch.float32):
        raise L.CsError(f"front_end: expected torch.uint8 or torch.float32, got {images.dtype}")
    if images.dim() != 4 or images.shape[3] != 3 or images.shape[0] < 1:
        raise L.CsError(f"front_end: images must be [B, H, W, 3], got {tuple(images.shape)}")
    is_float = images.dtype == torch.float32
    nb, h, w = (int(v) for v in images.shape[:3])
    if is_float:
        resize = False
    images = images.contiguous()
    out = torch.empty((nb, SIZE, SIZE, int(cpad)), dtype=torch.float32, device=images.device)
    L.check(L.load().cs_incep_input(images.data_ptr(), 1 if is_float else 0, nb, h, w, 1 if resize else 0, int(norm),
                                    out.data_ptr(), int(cpad), ops._stream()), "cs_incep_input")
    return out


# ----------------------------------------------------------------------------------------------------------------------
# the model
# ----------------------------------------------------------------------------------------------------------------------
@dataclass
class _Layer:
    spec: Conv
    w: ops.PackedWeight
    scale: Tensor
    shift: Tensor


# One accumulator of the F16X3 kernel takes a layer's whole K loop as ONE sequential fp32 chain (three MFMAs per 16-channel
# chunk): at K = 448 * 9 that chain's rounding alone put the network at 2.2x the error of a blocked fp32 convolution on the
# CPU.  So K is cut into slices of at most K_CHUNKS_PER_SLICE chunks (512 products per chain) that are summed in slice order
# (CsConvGemm.splitk): measured on the 299 x 299 input, rel-L2 against fp64 5.0e-7 unsliced, 4.1e-7 / 3.3e-7 / 2.9e-7 / 3.0e-7
# at 64 / 32 / 16 / 8 chunks per slice for 4.4 -> 5.0 / 5.1 / 5.3 / 6.2 ms per batch of 16 (profiles/inception.txt).  0: never.
K_CHUNKS_PER_SLICE = 32
SLICED_TILE = 6          # the 256 x 128 tile: K-sliced launches of any cout % 4 == 0 run on an explicit narrow tile


def k_slices(spec: Conv) -> int:
    """K slices of a layer's GEMM: a function of the layer alone (never of the batch or the image size), so the order of
    every sum is the same in every call -- the library's own split-K plan follows the row count and is not asked"""
    if K_CHUNKS_PER_SLICE <= 0:
        return 1
    nk = spec.k[0] * spec.k[1] * ((spec.cin + 15) // 16)
    return max(1, min(16, -(-nk // K_CHUNKS_PER_SLICE)))


def pack_layer(spec: Conv, sd, device) -> _Layer:
    """one BasicConv2d of a state dict (keys `<spec.name>.conv.weight`, `<spec.name>.bn.*`) ready for the device: the conv
    weight F16X3-packed as it is, the BatchNorm folded (fp64, rounded once) into the epilogue's scale / shift"""
    dev = torch.device(device)
    w = sd[f"{spec.name}.conv.weight"].detach().to(device=dev, dtype=torch.float32)
    if tuple(w.shape) != (spec.cout, spec.cin, *spec.k):
        raise ValueError(f"Inception state dict: '{spec.name}.conv.weight' has shape {tuple(w.shape)}, expected "
                         f"{(spec.cout, spec.cin, *spec.k)}")
    bn = [sd[f"{spec.name}.bn.{p}"].detach().to("cpu") for p in ("weight", "bias", "running_mean", "running_var")]
    scale, shift = fold_bn(*bn)
    pw = ops.pack_weight(w.unsqueeze(2).contiguous(), None, cin_pad=(spec.cin + 3) // 4 * 4, math=L.MATH_F16X3)
    return _Layer(spec, pw, scale.to(device=dev, dtype=torch.float32).contiguous(),
                  shift.to(device=dev, dtype=torch.float32).contiguous())


class InceptionV3:
    """The FID InceptionV3 up to pool3 over the HIP library (F16X3 GEMMs, fp32-grade).  `load_state_dict` takes
    torchvision's `Inception3` key layout; fp16 / fp64 tensors are converted."""

    SLOTS = 256          # absmax slots per block of them: one per tensor a conv reads (94 convs, fewer distinct inputs)

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        self._layers: Dict[str, _Layer] = {}
        self._slots: Optional[Tensor] = None
        self._next_slot = 0

    # -- weights ---------------------------------------------------------------------------------------------------------
    def load_state_dict(self, sd) -> "InceptionV3":
        _validate(sd)                             # raises KeyError / ValueError naming the key
        self._layers = {c.name: pack_layer(c, sd, self.device) for c in conv_layers()}
        return self

    # -- pieces ----------------------------------------------------------------------------------------------------------
    def _bound(self, x: Tensor) -> Optional[Tensor]:
        """max |x| of a dense tensor in a zeroed slot of its own (once per tensor: every conv that reads x shares it)"""
        b = getattr(x, "cs_bound", None)
        if b is not None:
            return b
        if self._slots is None or self._next_slot >= self.SLOTS or self._slots.device != x.device:
            self._slots = torch.zeros((self.SLOTS,), dtype=torch.float32, device=x.device)
            self._next_slot = 0
        slot = self._slots[self._next_slot:self._next_slot + 1]
        self._next_slot += 1
        return ops.absmax_bound(x, slot)

    def run_layer(self, x: Tensor, ly: _Layer, out_fn=None) -> Tensor:
        """one BasicConv2d on x [B, 1, H, W, cin] (dense): conv, folded BatchNorm and ReLU in one cs_conv_gemm launch whose
        operand scale follows max |x|"""
        c = ly.spec
        slices = k_slices(c)
        return ops.conv_gemm(x, ly.w, stride=(1, c.stride, c.stride), pad=(0, c.pad[0], c.pad[1]), act=L.ACT_RELU,
                             scale=ly.scale, shift=ly.shift, out_fn=out_fn, math=L.MATH_F16X3, splitk=slices,
                             tile=SLICED_TILE if slices > 1 else 0, x_bound=self._bound(x))

    def conv(self, x: Tensor, name: str, out_fn=None) -> Tensor:
        if name not in self._layers:
            raise L.CsError(f"InceptionV3: no weights loaded for {name!r}")
        return self.run_layer(x, self._layers[name], out_fn)

    @staticmethod
    def _pool(x: Tensor, op: Pool, out_fn=None) -> Tensor:
        if op.kind == "max":
            return max_pool3(x, op.stride, op.pad, out_fn=out_fn)
        return avg_pool3(x, count_include_pad=False, out_fn=out_fn)

    def block(self, x: Tensor, name: str) -> Tensor:
        """one Mixed block on x [B, 1, H, W, cin] (dense): the last layer of every branch (both convs of a Fork) stores into
        its channel range of the block's output buffer"""
        branches = dict(BLOCKS)[name]
        cin = int(x.shape[-1])
        if cin != block_input_width(branches):
            raise L.CsError(f"{name}: input has {cin} channels, expected {block_input_width(branches)}")
        total = sum(branch_width(br, cin) for br in branches)
        buf: List[Optional[Tensor]] = [None]

        def place(lo: int, width: int):
            def out_fn(oshape):
                if buf[0] is None:
                    buf[0] = torch.empty((*oshape[:-1], total), dtype=torch.float32, device=x.device)
                return buf[0][..., lo:lo + width]
            return out_fn

        c0 = 0
        for br in branches:
            h = x
            for op in br[:-1]:
                h = self.conv(h, op.name) if isinstance(op, Conv) else self._pool(h, op)
            op = br[-1]
            if isinstance(op, Fork):
                self.conv(h, op.a.name, out_fn=place(c0, op.a.cout))
                self.conv(h, op.b.name, out_fn=place(c0 + op.a.cout, op.b.cout))
            elif isinstance(op, Conv):
                self.conv(h, op.name, out_fn=place(c0, op.cout))
            else:
                self._pool(h, op, out_fn=place(c0, cin))
            c0 += branch_width(br, cin)
        return buf[0]

    # -- the network -----------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def features(self, x: Tensor, trace: Optional[list] = None) -> Tensor:
        """x: the front end's output [B, H, W, 4] at any H, W >= 75 -> pool3 features [B, 2048].  `trace`, a list, receives
        (stage name, H, W, C) after every stem layer and block."""
        if not self._layers:
            raise L.CsError("InceptionV3.features: no weights were loaded")
        ops._chk(x, "x")
        if x.dim() != 4 or x.shape[3] != CPAD or x.shape[0] < 1 or min(x.shape[1], x.shape[2]) < MIN_SIZE:
            raise L.CsError(f"InceptionV3.features: expected [B, H, W, {CPAD}] with H, W >= {MIN_SIZE}, got {tuple(x.shape)}")
        with torch.cuda.device(x.device):
            self._slots = None                    # a fresh block of zeroed slots per call
            h = x.contiguous().unsqueeze(1)
            note = (lambda n, t: trace.append((n, int(t.shape[2]), int(t.shape[3]), int(t.shape[4])))) if trace is not None \
                else (lambda n, t: None)
            for op in STEM:
                h = self.conv(h, op.name) if isinstance(op, Conv) else self._pool(h, op)
                note(op.name if isinstance(op, Conv) else "maxpool", h)
            for name, _ in BLOCKS:
                h = self.block(h, name)
                note(name, h)
            out = global_avg(h)
            ops.check_overflow(x.device, what="InceptionV3.features")        # one read-back per call
        return out

    def encode_image(self, images, mode: str = "clean") -> Tensor:
        """paths / PIL images or a uint8 [B, H, W, 3] tensor -> pool3 features [B, 2048] (see `preprocess` for the modes)"""
        pre = preprocess(images, mode)
        norm = 1 if mode == "clean" else 0
        if isinstance(pre, torch.Tensor):
            return self.features(front_end(pre.to(self.device), norm))
        x = torch.cat([front_end(p.to(self.device), norm) for p in pre])      # images of different sizes: one resize each
        return self.features(x)


# ----------------------------------------------------------------------------------------------------------------------
# host side
# ----------------------------------------------------------------------------------------------------------------------
def _rgb_arrays(images) -> List[np.ndarray]:
    from PIL import Image
    if isinstance(images, torch.Tensor):
        images = images.detach().cpu().numpy()
    if isinstance(images, np.ndarray):
        if images.dtype != np.uint8 or images.ndim != 4 or images.shape[3] != 3:
            raise L.CsError(f"images must be uint8 [B, H, W, 3], got {images.dtype} {images.shape}")
        return [np.ascontiguousarray(a) for a in images]
    if isinstance(images, (str, bytes, Image.Image)) or hasattr(images, "__fspath__"):
        images = [images]
    out = []
    for im in images:
        if not isinstance(im, Image.Image):
            with Image.open(im) as fh:
                im = fh.convert("RGB")
        out.append(np.array(im.convert("RGB"), dtype=np.uint8))
    return out


def resize_clean(arr: np.ndarray) -> np.ndarray:
    """uint8 [H, W, 3] -> float32 [299, 299, 3]: each channel as a float32 "F" image through PIL's BICUBIC resize (no
    rounding back to bytes)"""
    from PIL import Image
    chans = [np.asarray(Image.fromarray(arr[:, :, c].astype(np.float32), mode="F").resize((SIZE, SIZE), resample=Image.BICUBIC),
                        dtype=np.float32) for c in range(3)]
    return np.stack(chans, axis=2)


def preprocess(images, mode: str = "clean"):
    """The host half of `encode_image`.  mode "legacy_pytorch": convert to RGB and leave the bytes alone -> uint8
    [B, H, W, 3] (a list of [1, H, W, 3] when the sizes differ); the device resizes (bilinear) and normalises with
    2 (v / 255) - 1.  mode "clean" (cleanfid's default): resize on the host with PIL -> float32 [B, 299, 299, 3] holding
    0..255-range values; the device normalises with (v - 128) / 128."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
    arrs = _rgb_arrays(images)
    if not arrs:
        raise ValueError("preprocess: no images")
    if mode == "clean":
        return torch.from_numpy(np.stack([resize_clean(a) for a in arrs]))
    if all(a.shape == arrs[0].shape for a in arrs):
        return torch.from_numpy(np.stack(arrs))
    return [torch.from_numpy(a[None]) for a in arrs]


def _uniform(rng, shape, std: float) -> np.ndarray:
    """zero-mean uniform draws of standard deviation `std` from integers alone (exact on every machine: no libm)"""
    u = rng.integers(0, 1 << 24, size=shape, dtype=np.int64).astype(np.float64)
    return (((u + 0.5) / float(1 << 24) - 0.5) * (math.sqrt(12.0) * std)).astype(np.float32)


def synth_inception_state_dict(seed: int, gain: float = 1.0) -> Dict[str, Tensor]:
    """Weights in torchvision's key layout from numpy.random.default_rng(seed): conv weights He-scaled (std sqrt(2 / fan_in)),
    BatchNorm gamma around `gain`, beta around 0.1 `gain`, and running statistics that match what the conv produces from
    the previous layer's outputs (mean around 0, variance around gain^2; 1 for the image's own conv), so every activation is
    O(gain) through the 94 layers.  The draws are uniform and built from integers only, hence identical on every machine.
    `gain` = 1e3 puts every activation three decades up -- beyond what the fixed operand scale 16 of the F16X3 kernels
    carries (65504 / 16): the stress case of the scale rule.  CPU fp32 tensors."""
    rng = np.random.default_rng(int(seed))
    g = float(gain)
    sd: Dict[str, np.ndarray] = {}
    for c in conv_layers():
        fan_in = c.cin * c.k[0] * c.k[1]
        gin = 1.0 if c.cin == 3 else g            # the magnitude of this conv's input
        sd[f"{c.name}.conv.weight"] = _uniform(rng, (c.cout, c.cin, c.k[0], c.k[1]), math.sqrt(2.0 / fan_in))
        sd[f"{c.name}.bn.weight"] = (1.0 + _uniform(rng, (c.cout,), 0.1)) * g
        sd[f"{c.name}.bn.bias"] = (0.1 + _uniform(rng, (c.cout,), 0.1)) * g
        sd[f"{c.name}.bn.running_mean"] = _uniform(rng, (c.cout,), 0.1) * gin
        sd[f"{c.name}.bn.running_var"] = (1.0 + _uniform(rng, (c.cout,), 0.1)) * (gin * gin)
    return {k: torch.from_numpy(np.ascontiguousarray(a.astype(np.float32))) for k, a in sd.items()}


def load_checkpoint(path, device="cuda") -> InceptionV3:
    """MODEL.pth: a pickled state dict (pytorch-fid's pt_inception-2015-12-05 file) or module -> InceptionV3"""
    obj = torch.load(str(path), map_location="cpu", weights_only=False)
    sd = obj.state_dict() if hasattr(obj, "state_dict") else obj.get("state_dict", obj)
    return InceptionV3(device).load_state_dict(sd)
