"""Partial shapes for shape completion: the reference's `get_partial_shape` (diff_utils/demo_util.py:172-254).

A user marks an axis-aligned box of the unit cube [-1, 1]^3; what lies inside is the KNOWN part of the shape, the rest is to
be generated.  The box becomes two masks: a bool one over the SDF grid and a float one over the latent grid, which the masked
DDIM sampler blends with (ddim.py `sample(mask=..., x0=...)`).  Off the sampling path: the index arithmetic is host Python
(the reference's own expressions, truncation included), the masks are assembled on the host and uploaded once.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

Tensor = torch.Tensor
TSDF_FILL = 0.2          # the truncation value the reference writes outside / inside the box (demo_util.py:220-221)


def _index_range(lo: float, hi: float, n: int) -> Tuple[int, int]:
    """[-1, 1] -> grid indices as demo_util.py:188-201 does it: clamp, then int() of (v + 1) / 2 * n, which truncates."""
    lo, hi = max(-1, lo), min(1, hi)
    return int((lo - (-1)) / 2 * n), int((hi - (-1)) / 2 * n)


def _box_mask(shape5, ranges, dtype) -> Tensor:
    """ones inside the box, zeros outside, on the host; tensor axis 2 takes the x range, axis 3 the y range, axis 4 the z
    range.  Slicing semantics are Python's ([:st] and [ed:] are cleared), so an empty or inverted range clears everything."""
    B, _, n2, n3, n4 = shape5
    m = torch.ones((B, 1, n2, n3, n4), dtype=dtype)
    for axis, ((lo, hi), n) in enumerate(zip(ranges, (n2, n3, n4)), start=2):
        st, ed = _index_range(lo, hi, n)
        head = [slice(None)] * 5
        tail = [slice(None)] * 5
        head[axis], tail[axis] = slice(None, st), slice(ed, None)
        m[tuple(head)] = 0
        m[tuple(tail)] = 0
    return m


def get_partial_shape(shape: Tensor, xyz_dict: Dict[str, Tuple[float, float]], z: Optional[Tensor] = None) -> Dict[str, Tensor]:
    """shape: SDFs [B, 1, H, W, D]; xyz_dict: {'x': (min, max), 'y': ..., 'z': ...} inside [-1, 1] (clamped to it).
    Returns, on the device of `shape`: 'shape_part' (the SDF with 0.2 outside the box), 'shape_missing' (0.2 inside it),
    'shape_mask' (bool [B, 1, H, W, D], True inside) and, when the latent `z` [B, C, h, w, d] is given, 'z_mask' (float32
    [B, 1, h, w, d], 1 inside): the same box at the latent's resolution, its bounds truncated at THAT resolution."""
    if shape.dim() != 5:
        raise ValueError(f"get_partial_shape: shape must be [B, 1, H, W, D], got {tuple(shape.shape)}")
    ranges = (xyz_dict["x"], xyz_dict["y"], xyz_dict["z"])
    device = shape.device
    B = shape.shape[0]
    x_mask = _box_mask((B, 1, *shape.shape[2:]), ranges, torch.bool).to(device)
    fill = torch.full((), TSDF_FILL, dtype=shape.dtype, device=device)
    ret = {"shape_part": torch.where(x_mask, shape, fill), "shape_missing": torch.where(x_mask, fill, shape),
           "shape_mask": x_mask}
    if z is not None:
        if z.dim() != 5:
            raise ValueError(f"get_partial_shape: z must be [B, C, h, w, d], got {tuple(z.shape)}")
        ret["z_mask"] = _box_mask((z.shape[0], 1, *z.shape[2:]), ranges, torch.float32).to(device)
    return ret
