"""Scene-graph constraint accuracy on the MI355X: the layout table of the reference's evaluation script
(scripts/eval_3dfront.py:411-415,722 -> helpers/metrics_3dfront.py:57-311): left / right / front / behind / bigger / smaller /
taller / shorter / standing on / close by / symmetrical to / total.

The reference walks the triples on the host and reads two boxes back per triple (two `.cpu().detach().numpy()` each); here
csrc/cs_constraints.hip evaluates every triple of every scene in one launch and nothing is read back until the caller wants
the numbers:

    validate_constrains / validate_constrains_changes   the reference's call surface: same arguments, same `accuracy` dict of
                                                        lists, appended in triple order (one read-back of the verdicts)
    validate_constrains_many                            several scenes, one launch, one read-back of the counts
    evaluate                                            the launch alone: device tensors, no read-back
    box3d_iou                                           metrics_3dfront.py:337-370 over a batch of box pairs

Inputs are HIP device tensors; there is no CPU path.  Argument errors raise `lib.CsError` before any device work.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import lib as L
from .ops import _stream

Tensor = torch.Tensor

# the script's twelve keys (scripts/eval_3dfront.py:411-415); the first eleven are the kernel's categories 0..10
CATEGORIES = ("left", "right", "front", "behind", "bigger", "smaller", "taller", "shorter", "standing on", "close by",
              "symmetrical to")
KEYS = CATEGORIES + ("total",)
# predicate name (vocab entry without its last character) -> category (metrics_3dfront.py:74-165)
PREDICATE_CATEGORY = {"left": 0, "right": 1, "front": 2, "behind": 3, "bigger than": 4, "smaller than": 5, "taller than": 6,
                      "shorter than": 7, "standing on": 8, "close by": 9, "symmetrical to": 10}
# helpers/util.py:546-550: the default statistics of denormalize_box_params
DEFAULT_MEAN = (1.3827214, 1.309359, 0.9488993, -0.12464812, 0.6188591, -0.54847, 0.73127955)
DEFAULT_STD = (1.7797655, 1.657638, 0.8501885, 1.9160025, 2.0038228, 0.70099753, 0.50347435)
SCALE = 3.0
MODE_ALL, MODE_KEPT, MODE_CHANGED = 0, 1, 2


def new_accuracy() -> Dict[str, List[int]]:
    """the dict of lists the script hands to validate_constrains (scripts/eval_3dfront.py:411-415)"""
    return {k: [] for k in KEYS}


def predicate_codes(vocab) -> List[int]:
    """predicate index -> category 0..10, -1 = not evaluated.  The reference compares `name[:-1]` (it strips the newline its
    vocabulary files end every entry with), so a name is matched WITHOUT its last character, whatever that is."""
    return [PREDICATE_CATEGORY.get(str(name)[:-1], -1) for name in vocab["pred_idx_to_name"]]


def _norm_rows(file_dist, params: int) -> np.ndarray:
    """[2][7] fp64 mean / std: the defaults, or `np.loadtxt(file_dist)` (helpers/util.py:554-558)"""
    out = np.zeros((2, 7), np.float64)
    if file_dist is None:
        out[0], out[1] = DEFAULT_MEAN, DEFAULT_STD
        return out
    stats = np.atleast_2d(np.loadtxt(file_dist)).astype(np.float64)
    if stats.shape[0] < 2 or stats.shape[1] < params:
        raise L.CsError(f"constraints: {file_dist} holds {stats.shape} values, need mean and std rows of {params} parameters")
    out[:, :min(7, stats.shape[1])] = stats[:2, :7]
    return out


def _check_scene(i: int, triples, boxes, keep, mode: int) -> Tuple[int, int, int]:
    """shape checks of one scene -> (objects, triples, box width).  Needs no device."""
    if not isinstance(boxes, torch.Tensor) or boxes.dim() != 2 or boxes.shape[1] not in (6, 7):
        got = tuple(boxes.shape) if isinstance(boxes, torch.Tensor) else type(boxes).__name__
        raise L.CsError(f"constraints: scene {i}: boxes must be [N, 6] or [N, 7] (l, h, w, px, py, pz[, angle]), got {got}")
    if boxes.shape[0] == 0:
        raise L.CsError(f"constraints: scene {i}: no boxes")
    if not isinstance(triples, torch.Tensor) or triples.dim() != 2 or triples.shape[1] != 3 or \
            triples.dtype not in (torch.int64, torch.int32):
        got = (tuple(triples.shape), triples.dtype) if isinstance(triples, torch.Tensor) else type(triples).__name__
        raise L.CsError(f"constraints: scene {i}: triples must be an integer tensor [T, 3] (s, p, o), got {got}")
    if mode == MODE_CHANGED and boxes.shape[1] == 7:
        raise L.CsError("constraints: validate_constrains_changes takes 6-parameter boxes: the reference calls box3d_iou with "
                        "its 6-parameter default there and cannot unpack seven values")
    if keep is not None:
        if not isinstance(keep, torch.Tensor) or keep.numel() != boxes.shape[0]:
            got = keep.numel() if isinstance(keep, torch.Tensor) else type(keep).__name__
            raise L.CsError(f"constraints: scene {i}: keep has {got} entries for {boxes.shape[0]} boxes")
    return int(boxes.shape[0]), int(triples.shape[0]), int(boxes.shape[1])


def _check_ids_host(i: int, triples: Tensor, n_boxes: int, n_preds: int) -> None:
    """ids of a HOST triple tensor (a device tensor's ids are checked by the kernel and reported through the status word)"""
    if triples.is_cuda or triples.shape[0] == 0:
        return
    t = triples.to(torch.int64)
    so = torch.stack([t[:, 0], t[:, 2]])
    if int(so.min()) < 0 or int(so.max()) >= n_boxes or int(t[:, 1].min()) < 0 or int(t[:, 1].max()) >= n_preds:
        raise L.CsError(f"constraints: scene {i}: a triple's ids are out of range ({n_boxes} boxes, {n_preds} predicates)")


def _require_device(ts: Sequence[Optional[Tensor]]) -> torch.device:
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise L.CsError("constraints: expected HIP device tensors (the HIP path has no CPU fallback)")
        if dev is not None and t.device != dev:
            raise L.CsError("constraints: all tensors must live on one device")
        dev = t.device
    return dev


def _keep_u8(keep: Tensor) -> Tensor:
    """0 / 1 as the reference tests them (`== 1`, `== 0`); any other value matches neither"""
    k = keep.reshape(-1)
    return torch.where(k == 1, 1, torch.where(k == 0, 0, 2)).to(torch.uint8)


class Launch:
    """what `evaluate` leaves on the device: verdict [T] int8 (-1 skipped, 0 violated, 1 satisfied), counts [S][11][2] int32
    (satisfied, evaluated), status [1] int32 (lib.STATUS_CONSTRAINT_RANGE), and the host-side CSR offsets of the scenes"""

    def __init__(self, verdict, counts, status, packed, triple_ptr, box_ptr, category):
        self.verdict, self.counts, self.status, self._packed = verdict, counts, status, packed
        self.triple_ptr, self.box_ptr, self._category = triple_ptr, box_ptr, category

    def read_verdict(self, with_category: bool = False):
        """ONE read-back: the status word and the verdicts share a buffer (with_category: each triple's category 0..10 / -1
        rides along).  Raises on a range error."""
        T = self.verdict.numel()
        buf = torch.cat([self._packed, self._category().view(torch.uint8)]) if with_category else self._packed
        host = buf.cpu().numpy()
        if int(host[:4].view(np.int32)[0]) & L.STATUS_CONSTRAINT_RANGE:
            raise L.CsError("constraints: a triple's ids are out of range for its scene (verdict -1)")
        verdict = host[4:4 + T].view(np.int8)
        return (verdict, host[4 + T:].view(np.int8)) if with_category else verdict


def evaluate(scenes, vocab, mode: int = MODE_ALL, file_dist=None, with_norm: bool = True, strict: bool = True,
             overlap_threshold: float = 0.3) -> Launch:
    """One launch over `scenes` = [(triples [T,3] int, boxes [N,6|7] fp32[, keep [N])), ...]; nothing is read back."""
    if mode not in (MODE_ALL, MODE_KEPT, MODE_CHANGED):
        raise L.CsError(f"constraints: mode must be 0, 1 or 2, got {mode}")
    scenes = [tuple(sc) for sc in scenes]
    if not scenes:
        raise L.CsError("constraints: no scenes")
    codes = predicate_codes(vocab)
    if not codes:
        raise L.CsError("constraints: the vocabulary lists no predicates")
    widths, n_box, n_tri = set(), [], []
    for i, sc in enumerate(scenes):
        if len(sc) not in (2, 3):
            raise L.CsError(f"constraints: scene {i}: expected (triples, boxes[, keep])")
        keep = sc[2] if len(sc) == 3 else None
        if mode != MODE_ALL and keep is None:
            raise L.CsError(f"constraints: scene {i}: mode {mode} needs a keep mask")
        nb, nt, w = _check_scene(i, sc[0], sc[1], keep, mode)
        _check_ids_host(i, sc[0], nb, len(codes))
        widths.add(w)
        n_box.append(nb)
        n_tri.append(nt)
    if len(widths) != 1:
        raise L.CsError("constraints: every scene of one launch must have the same box width (6 or 7)")
    params = widths.pop()
    norm_host = _norm_rows(file_dist, params) if with_norm else None
    dev = _require_device([t for sc in scenes for t in sc])
    box_ptr = np.concatenate([[0], np.cumsum(n_box)]).astype(np.int64)
    triple_ptr = np.concatenate([[0], np.cumsum(n_tri)]).astype(np.int64)
    S, T = len(scenes), int(triple_ptr[-1])
    boxes = torch.cat([sc[1].detach().to(torch.float32) for sc in scenes]).contiguous()
    triples = torch.cat([sc[0].to(torch.int64) for sc in scenes]).contiguous() if T else \
        torch.zeros((1, 3), dtype=torch.int64, device=dev)
    keep = torch.cat([_keep_u8(sc[2]) for sc in scenes]).contiguous() if mode != MODE_ALL else None
    # small uploads: CSR offsets, predicate codes and the statistics
    meta_i = torch.from_numpy(np.concatenate([box_ptr, triple_ptr])).to(dev)
    code_t = torch.tensor(codes, dtype=torch.int32).to(dev)
    norm_t = torch.from_numpy(norm_host).to(dev) if norm_host is not None else None
    packed = torch.zeros(4 + max(T, 1), dtype=torch.uint8, device=dev)       # [status word | verdicts]
    status, verdict = packed[:4].view(torch.int32), packed[4:4 + T].view(torch.int8)
    counts = torch.empty((S, len(CATEGORIES), 2), dtype=torch.int32, device=dev)
    L.check(L.load().cs_scene_constraints(
        boxes.data_ptr(), boxes.shape[0], boxes.stride(0), params, triples.data_ptr(), T, meta_i.data_ptr(),
        meta_i[S + 1:].data_ptr(), S, code_t.data_ptr(), len(codes), None if keep is None else keep.data_ptr(), mode,
        None if norm_t is None else norm_t.data_ptr(), SCALE, int(bool(strict)), float(overlap_threshold),
        packed[4:].data_ptr(), counts.data_ptr(), status.data_ptr(), _stream()), "cs_scene_constraints")
    category = lambda: code_t[triples[:T, 1].clamp(0, len(codes) - 1)].to(torch.int8)      # (host bookkeeping, not a rule)
    return Launch(verdict, counts, status, packed[:4 + T], triple_ptr, box_ptr, category)


def _validate(mode, triples, pred_boxes, keep, vocab, accuracy, file_dist, with_norm, strict, overlap_threshold):
    if mode == MODE_CHANGED:
        _check_scene(0, triples, pred_boxes, keep, mode)    # 7-parameter boxes: refused with or without a keep mask
    if keep is None:
        mode = MODE_ALL                                     # both reference functions evaluate every triple then
    scene = (triples, pred_boxes) if keep is None else (triples, pred_boxes, keep)
    launch = evaluate([scene], vocab, mode, file_dist, with_norm, strict, overlap_threshold)
    if launch.verdict.numel() == 0:
        return accuracy
    verdict, category = launch.read_verdict(with_category=True)             # the call's one read-back
    for c, v in zip(category.tolist(), verdict.tolist()):
        if v >= 0:
            accuracy[CATEGORIES[c]].append(v)
            accuracy["total"].append(v)
    return accuracy


def validate_constrains(triples, pred_boxes, gt_boxes, keep, vocab, accuracy, file_dist=None, with_norm=True, strict=True,
                        overlap_threshold=0.3):
    """helpers/metrics_3dfront.py:57-179: every triple (`keep is None`) or the triples whose two nodes are both kept; appends
    0 / 1 to `accuracy[category]` and `accuracy['total']` in triple order.  `gt_boxes` is unused, as in the reference."""
    return _validate(MODE_KEPT, triples, pred_boxes, keep, vocab, accuracy, file_dist, with_norm, strict, overlap_threshold)


def validate_constrains_changes(triples, pred_boxes, gt_boxes, keep, vocab, accuracy, file_dist=None, with_norm=True,
                                strict=True, overlap_threshold=0.3):
    """helpers/metrics_3dfront.py:182-311: the triples with a changed node (keep == 0 on either side).  6-parameter boxes
    only: the reference cannot run this function on 7-parameter boxes."""
    return _validate(MODE_CHANGED, triples, pred_boxes, keep, vocab, accuracy, file_dist, with_norm, strict,
                     overlap_threshold)


def validate_constrains_many(scenes, vocab, mode: int = MODE_ALL, file_dist=None, with_norm: bool = True,
                             strict: bool = True, overlap_threshold: float = 0.3) -> dict:
    """Several scenes (triples, boxes[, keep]) in one launch and ONE read-back.  -> dict(counts = [S][11][2] int32 numpy
    (satisfied, evaluated), summary = {category: (satisfied, evaluated)}, total = (satisfied, evaluated))."""
    launch = evaluate(scenes, vocab, mode, file_dist, with_norm, strict, overlap_threshold)
    host = torch.cat([launch.counts.reshape(-1), launch.status]).cpu().numpy()
    if int(host[-1]) & L.STATUS_CONSTRAINT_RANGE:
        raise L.CsError("constraints: a triple's ids are out of range for its scene")
    counts = host[:-1].reshape(len(launch.triple_ptr) - 1, len(CATEGORIES), 2)
    per_cat = counts.sum(axis=0, dtype=np.int64)
    summary = {c: (int(per_cat[k, 0]), int(per_cat[k, 1])) for k, c in enumerate(CATEGORIES)}
    return dict(counts=counts, summary=summary, total=(int(per_cat[:, 0].sum()), int(per_cat[:, 1].sum())))


def box3d_iou(boxes1: Tensor, boxes2: Tensor, param6: bool = True, with_translation: bool = False) -> Tuple[Tensor, Tensor]:
    """helpers/metrics_3dfront.py:337-370 over M pairs of (denormalised) boxes [M, 6] (param6) or [M, 7]: -> (iou, iou_2d),
    fp64 device tensors [M].  The angle is ignored and iou divides by the smaller volume, as the reference does."""
    width = 6 if param6 else 7
    for name, b in (("boxes1", boxes1), ("boxes2", boxes2)):
        if not isinstance(b, torch.Tensor) or b.dim() != 2 or b.shape[1] != width:
            got = tuple(b.shape) if isinstance(b, torch.Tensor) else type(b).__name__
            raise L.CsError(f"box3d_iou: {name} must be [M, {width}], got {got}")
    if boxes1.shape[0] != boxes2.shape[0] or boxes1.shape[0] == 0:
        raise L.CsError(f"box3d_iou: {boxes1.shape[0]} and {boxes2.shape[0]} boxes do not pair up")
    dev = _require_device([boxes1, boxes2])
    b1 = boxes1.detach().to(torch.float32).contiguous()
    b2 = boxes2.detach().to(torch.float32).contiguous()
    m = b1.shape[0]
    out = torch.empty((2, m), dtype=torch.float64, device=dev)
    L.check(L.load().cs_box3d_iou_pairs(b1.data_ptr(), b2.data_ptr(), m, width, width, int(bool(with_translation)),
                                        out[0].data_ptr(), out[1].data_ptr(), _stream()), "cs_box3d_iou_pairs")
    return out[0], out[1]
