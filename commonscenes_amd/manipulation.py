"""The scene-manipulation experiment of scripts/eval_3dfront.py (`validate_constrains_loop_w_changes`, :206-441) and the
before / after editing workflow of scripts/eval_3dfront_manivis.py (:223-420) over this package's models and kernels.

Call map (reference -> here)
  dataset/threedfront_dataset.py:582-628  remove_node_and_relationship   -> remove_node_and_relationship
  dataset/threedfront_dataset.py:630-684  modify_relship                 -> modify_relship
  :536-550 (`eval=True` branch of __getitem__) + :705-723 (collate)      -> make_edit
  eval_3dfront.py:228-416  the per-scene body                            -> manipulation_loop
  eval_3dfront.py:335-400  diversity over the changed nodes              -> ManipulationMeter.add_scene(runs=...)
  eval_3dfront.py:411-416  the three validate_constrains* calls          -> ManipulationMeter.add_scene
  eval_3dfront.py:418-441  the printed rows                              -> ManipulationMeter.summary
  eval_3dfront_manivis.py:298-380 + render_v2_full(mani=2)               -> edit_scene

No new kernel: the hot path is the sampler (Diff.rel2shape_many through the `_many` decodes of scene.py / vae.py) plus the
constraint, mesh, resample and Chamfer entries that exist.  The three tables are three `constraints.evaluate` launches over
ALL queued scenes in summary(), with one read-back of their counts.

Quirks of the reference that are kept:
  * the first two tables pass `file_dist=normalized_file`, the third passes none and so falls to the default statistics
    (eval_3dfront.py:411-416);
  * `remove_node_and_relationship` draws from `len(objs) - 1`: the last node is never removed;
  * the collated key is spelled `tripltes`.
One quirk is NOT kept: the reference's loop calls `sdf_to_mesh` without `render_all` and so meshes only the first 16 objects
(util_3d.py:204-208), which breaks on larger scenes; here every shape is meshed (`render_all=True`).

The graph edits draw from numpy's global RNG with the reference's calls in the reference's order: `np.random.seed(k)`
reproduces its pick.
"""
from __future__ import annotations

import copy
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import constraints as CN
from . import diversity as DV

Tensor = torch.Tensor

# dataset/threedfront_dataset.py:23-39: which relation a relationship edit turns each relation into (names: data)
CHANGED_RELATIONSHIPS = {
    "left": "right", "right": "left", "front": "behind", "behind": "front",
    "bigger than": "smaller than", "smaller than": "bigger than", "taller than": "shorter than",
    "shorter than": "taller than", "close by": "close by", "same style as": "same style as",
    "same super category as": "same super category as", "same material as": "same material as",
    "symmetrical to": "symmetrical to", "standing on": "standing on", "above": "above",
}
# :643 the relations a geometric rule can check (ids are 1-based positions in the relationship list)
INTERPRETABLE_RELS = (1, 2, 3, 4, 8, 9, 10, 11)
# SG-FRONT's relationships.txt (predicate id = position + 1; id 0 is the `in` edge to `_scene_`), :639-641
SGFRONT_RELATIONSHIPS = ("left", "right", "front", "behind", "close by", "above", "standing on", "bigger than", "smaller than",
                         "taller than", "shorter than", "symmetrical to", "same style as", "same super category as",
                         "same material as")
TABLES = ("changed nodes", "unchanged nodes", "changed nodes placed in original graph")


def _rel_dicts(relationships):
    fwd = dict(zip(relationships, range(1, len(relationships) + 1)))          # :95-96
    return fwd, {v: k for k, v in fwd.items()}


# ----------------------------------------------------------------------------------------------------------------------
# graph edits
# ----------------------------------------------------------------------------------------------------------------------
def remove_node_and_relationship(graph, classes, with_feats: bool = False, with_CLIP: bool = True) -> int:
    """dataset/threedfront_dataset.py:582-628 on a graph of lists (objs, boxes, triples[, text_feats, rel_feats, words,
    feats]), in place.  Draws np.random.randint(len(objs) - 1) until the node is not `floor`; gives up with -1 after 100
    trials.  Returns the removed node's id."""
    floor = classes["floor"]
    node_id, trials = -1, 0
    while node_id < 0 or graph["objs"][node_id] == floor:
        if trials > 100:
            return -1
        trials += 1
        node_id = np.random.randint(len(graph["objs"]) - 1)
    graph["objs"].pop(node_id)
    if with_feats:
        graph["feats"].pop(node_id)
    if with_CLIP:
        graph["text_feats"].pop(node_id)
    graph["boxes"].pop(node_id)
    gone = [i for i, t in enumerate(graph["triples"]) if t[0] == node_id or t[2] == node_id]
    if with_CLIP:
        for i in reversed(gone):                     # the reference pops these rows from the back (:610-616)
            graph["rel_feats"].pop(i)
            graph["words"].pop(i)
    # :618-619 removes the incident triples by value from the front: every triple equal to an incident one is incident
    # itself, so what is left is the other triples in their order
    graph["triples"][:] = [t for i, t in enumerate(graph["triples"]) if i not in set(gone)]
    for t in graph["triples"]:
        if t[0] > node_id:
            t[0] -= 1
        if t[2] > node_id:
            t[2] -= 1
    return node_id


def modify_relship(graph, classes, relationships, interpretable: bool = False):
    """dataset/threedfront_dataset.py:630-684, in place -> (idx, (sub, obj), did_change).  Up to 1000 draws of
    np.random.randint(len(triples)); `in` edges (predicate 0) and triples touching `floor` are skipped.  interpretable: only
    relations 1, 2, 3, 4, 8, 9, 10, 11, each turned into its opposite; otherwise a self-mapped relation redraws
    np.random.randint(1, 12) and tries again when that is the same relation."""
    rel_id, rel_name = _rel_dicts(relationships)
    floor = classes["floor"]
    did_change, trials = False, 0
    idx = sub = obj = None
    while not did_change and trials < 1000:
        idx = np.random.randint(len(graph["triples"]))
        sub, pred, obj = graph["triples"][idx]
        trials += 1
        if pred == 0:
            continue
        if graph["objs"][obj] == floor or graph["objs"][sub] == floor:
            continue
        name = rel_name[pred]
        if interpretable:
            if pred not in INTERPRETABLE_RELS:
                continue
            new_pred = rel_id[CHANGED_RELATIONSHIPS[name]]
        elif name == CHANGED_RELATIONSHIPS[name]:
            new_pred = np.random.randint(1, 12)
            if new_pred == pred:
                continue
        else:
            new_pred = rel_id[CHANGED_RELATIONSHIPS[name]]
        graph["words"][idx] = graph["words"][idx].replace(name, rel_name[new_pred])
        graph["changed_id"] = idx
        graph["triples"][idx][1] = new_pred
        did_change = True
    return idx, (sub, obj), did_change


_NODE_KEYS = ("objs", "objs_grained", "boxes", "text_feats", "feats")
_EDGE_KEYS = ("triples", "rel_feats", "words")


def graph_lists(objs, triples, boxes, text_feats, rel_feats, classes_r=None, relationships=None, sdfs=None,
                scan_id="scene") -> dict:
    """A scene as the dataset holds it before an edit (lists, one entry per node / triple) from its tensors.  `words` are
    '<subject> <relation> <object>' with the names of classes_r / relationships where given."""
    o = [int(c) for c in torch.as_tensor(objs).tolist()]
    t = [[int(v) for v in row] for row in torch.as_tensor(triples).tolist()]
    _, rel_name = _rel_dicts(relationships or ())
    cname = lambda c: (classes_r or {}).get(c, f"obj{c}")
    words = [f"{cname(o[s])} {rel_name.get(p, 'in' if p == 0 else f'pred{p}')} {cname(o[q])}" for s, p, q in t]
    scene = dict(objs=o, objs_grained=list(o), triples=t, boxes=[list(map(float, b)) for b in torch.as_tensor(boxes).tolist()],
                 text_feats=[np.asarray(r, np.float32) for r in torch.as_tensor(text_feats).cpu().numpy()],
                 rel_feats=[np.asarray(r, np.float32) for r in torch.as_tensor(rel_feats).cpu().numpy()], words=words,
                 scan_id=scan_id)
    if sdfs is not None:
        scene["sdfs"] = sdfs
    return scene


def _torchify(g: dict) -> dict:
    out = {"objs": torch.from_numpy(np.array(g["objs"], dtype=np.int64)),
           "tripltes": torch.from_numpy(np.array(g["triples"], dtype=np.int64).reshape(-1, 3)),
           "boxes": torch.from_numpy(np.array(g["boxes"], dtype=np.float32)), "words": list(g["words"])}
    if "objs_grained" in g:
        out["objs_grained"] = torch.from_numpy(np.array(g["objs_grained"], dtype=np.int64))
    for k in ("text_feats", "rel_feats", "feats"):
        if k in g:
            out[k] = torch.from_numpy(np.array([np.asarray(r) for r in g[k]], dtype=np.float32))
    if "changed_id" in g:
        out["changed_id"] = int(g["changed_id"])
    return out


def make_edit(scene: dict, eval_type: str, classes, relationships, rel_feat_fn=None, with_feats: bool = False,
              with_CLIP: bool = True) -> Optional[dict]:
    """The `eval=True` branch of the dataset's __getitem__ (:536-550) and the bookkeeping of its collate (:705-723) for ONE
    scene of lists (graph_lists): `decoder` is a deep copy of `encoder`; 'addition' removes a node from the ENCODER graph
    (missing_nodes = [node_id]); 'relationship' edits the DECODER graph with interpretable=True (manipulated_nodes =
    [sub, obj]).  None where the reference returns -1.  The scene itself is left as it was.  The collate re-encodes the
    edited triple's words with CLIP (:758-763); `rel_feat_fn(words) -> [512]` stands in for it, and without one the row
    keeps the feature of the unedited words."""
    if eval_type not in ("addition", "relationship", "none"):
        raise ValueError(f"eval_type must be 'addition', 'relationship' or 'none', got {eval_type!r}")
    lists = {k: copy.deepcopy(scene[k]) for k in _NODE_KEYS + _EDGE_KEYS if k in scene}
    encoder = lists
    decoder = copy.deepcopy(encoder)
    manipulate = {"type": eval_type}
    missing, missing_dec, manipulated = [], [], []
    if eval_type == "addition":
        node_id = remove_node_and_relationship(encoder, classes, with_feats=with_feats, with_CLIP=with_CLIP)
        if node_id < 0:
            return None
        manipulate["added"] = node_id
        missing, missing_dec = [node_id], [node_id]
    elif eval_type == "relationship":
        rel, pair, ok = modify_relship(decoder, classes, relationships, interpretable=True)
        if not ok:
            return None
        manipulate["relship"] = (rel, pair)
        manipulated = [pair[0], pair[1]]
    out = {"encoder": _torchify(encoder), "decoder": _torchify(decoder), "manipulate": manipulate,
           "missing_nodes": missing, "missing_nodes_decoder": missing_dec, "manipulated_nodes": manipulated,
           "scan_id": [scene.get("scan_id", "scene")]}
    if "changed_id" in decoder and rel_feat_fn is not None and "rel_feats" in out["decoder"]:
        i = decoder["changed_id"]
        out["decoder"]["rel_feats"][i] = torch.as_tensor(rel_feat_fn(decoder["words"][i]), dtype=torch.float32).reshape(-1)
    if "sdfs" in scene:
        out["decoder"]["sdfs"] = scene["sdfs"]
    return out


# ----------------------------------------------------------------------------------------------------------------------
# the meter
# ----------------------------------------------------------------------------------------------------------------------
def table_rows(sat_eval: Dict[str, Sequence[int]]) -> dict:
    """eval_3dfront.py:432-441 from {key: (satisfied, evaluated)} over the twelve keys: the printed figures, None where the
    reference prints nan (a mean over no verdicts)."""
    m = {k: (sat_eval[k][0] / sat_eval[k][1] if sat_eval[k][1] else float("nan")) for k in CN.KEYS}
    pair = lambda a, b: float(np.mean([m[a], m[b]]))
    row = {"L/R": pair("left", "right"), "F/B": pair("front", "behind"), "Bi/Sm": pair("bigger", "smaller"),
           "Ta/Sh": pair("taller", "shorter"), "Stand": m["standing on"], "Close": m["close by"],
           "Symm": m["symmetrical to"], "Total": m["total"]}
    row["means of mean"] = float(np.mean([row[k] for k in ("L/R", "F/B", "Bi/Sm", "Ta/Sh", "Stand", "Close", "Symm")]))
    return {k: (None if np.isnan(v) else float(v)) for k, v in row.items()}


def format_row(name: str, row: dict) -> str:
    """the two lines eval_3dfront.py:432-441 prints for one table"""
    f = lambda v: "nan" if v is None else f"{v:.2f}"
    return ("{} & L/R: {} & F/B: {} & Bi/Sm: {} & Ta/Sh: {} & Stand: {} & Close: {} & Symm: {}. Total: &{}\nmeans of mean: {}"
            .format(name, *[f(row[k]) for k in ("L/R", "F/B", "Bi/Sm", "Ta/Sh", "Stand", "Close", "Symm", "Total",
                                                "means of mean")]))


def _mean_or_none(v):
    return float(np.mean(v)) if len(v) else None


def diversity_block(chamfer: Sequence[float], box_rows, angles: Sequence[float]) -> dict:
    """eval_3dfront.py:418-424 from the accumulated lists; None (not NaN) for a figure nothing was accumulated for"""
    box = np.mean(np.asarray(box_rows, np.float64).reshape(-1, 6), axis=0) if len(box_rows) else None
    return {"shape": _mean_or_none(chamfer), "box_size": None if box is None else float(np.mean(box[:3])),
            "box_location": None if box is None else float(np.mean(box[3:])), "angle": _mean_or_none(angles),
            "shapes": len(chamfer), "boxes": len(box_rows), "angles": len(angles)}


class ManipulationMeter:
    """Accumulates what eval_3dfront.py:335-416 accumulates over the scenes and reports what :418-441 prints.

    vocab: the evaluation vocabulary (`pred_idx_to_name`); classes: name -> class id; file: the statistics file the
    reference calls `normalized_file` (first two tables and the box deviation; the third table ALWAYS uses the default
    statistics, as :415-416 passes no file).  add_scene only queues device tensors; the three tables are three launches over
    all queued scenes in summary(), whose counts come back in one read-back.  Shapes are meshed with render_all=True: the
    reference's loop omits it and meshes only 16 objects per call (util_3d.py:204-208), which breaks on larger scenes."""

    def __init__(self, vocab, classes: Dict[str, int], file=None, points: int = 5000):
        self.vocab, self.file, self.points = vocab, file, int(points)
        self.classes = {str(k).strip(): int(v) for k, v in classes.items()}
        self.classes_r = {v: k for k, v in self.classes.items()}
        self._queued = ([], [], [])                 # changed / unchanged / changed in the original graph
        self._boxes: List[Tensor] = []              # [C, K, 6] per scene, changed rows
        self._angles: List[Tensor] = []             # [C, K] argmax bins
        self._chamfer: List[Tensor] = []            # [C', K - 1] per scene
        self.scenes = 0

    # -- the three tables --
    def add_scene(self, dec_triples, boxes_pred, dec_tight_boxes, keep, runs=None, dec_objs=None, changed=None,
                  shape_nodes=None, generator=None) -> None:
        """One scene: the main decode's boxes [O, 6], the ground truth [O, >= 6], keep [O, 1]; `runs`: K tuples (boxes,
        angle scores | None, SDFs [S, 1, n, n, n] | Meshes | vertex list | None, keep) of the diversity decodes (:301-362).
        dec_objs is needed with shapes (class 0 and `floor` carry none); shape_nodes[r] is the node of shape row r
        (default r); `changed` is the host's list of nodes with keep == 0 -- without it the list is read from the runs' keep
        (a small read-back)."""
        boxes_pred = boxes_pred.detach()
        k = keep.reshape(-1)
        gt = dec_tight_boxes[:, :6].to(device=boxes_pred.device, dtype=boxes_pred.dtype)
        bp = torch.where((k == 0).unsqueeze(1), boxes_pred, gt)                     # :401-406
        tri = dec_triples.to(boxes_pred.device)
        self._queued[0].append((tri, boxes_pred, k))
        self._queued[1].append((tri, boxes_pred, k))
        self._queued[2].append((tri, bp, k))
        self.scenes += 1
        if runs:
            self._add_runs(list(runs), dec_objs, changed, shape_nodes, generator)

    def _add_runs(self, runs, dec_objs, changed, shape_nodes, generator):
        K = len(runs)
        if K < 2:
            raise ValueError("diversity needs at least two runs per object")          # eval_3dfront.py:207-208
        dev = runs[0][0].device
        if changed is None:
            changed = torch.nonzero(runs[0][3].reshape(-1) == 0).reshape(-1).cpu().tolist()
        changed = sorted(int(c) for c in changed)
        if not changed:
            return
        rows = torch.tensor(changed, dtype=torch.int64).to(dev)
        self._boxes.append(torch.stack([r[0].detach() for r in runs], 1).index_select(0, rows))           # :355, :366
        if runs[0][1] is not None:
            scores = torch.stack([r[1].detach() for r in runs], 1).index_select(0, rows)                 # :359
            self._angles.append(torch.argmax(scores, dim=2))
        if runs[0][2] is None:
            return
        if dec_objs is None:
            raise ValueError("shape diversity needs dec_objs: nodes of class 0 and `floor` carry no shape")
        objs = [int(c) for c in (dec_objs.tolist() if hasattr(dec_objs, "tolist") else dec_objs)]
        per = [r[2] for r in runs]
        as_sdf = all(isinstance(p, torch.Tensor) and p.dim() == 5 for p in per)
        if not as_sdf:
            per = [DV._verts_of(p) for p in per]
        S = int(per[0].shape[0]) if as_sdf else len(per[0])
        nodes = list(range(S)) if shape_nodes is None else [int(n) for n in shape_nodes]
        if len(nodes) != S or any((int(p.shape[0]) if as_sdf else len(p)) != S for p in per):
            raise ValueError(f"every run must hold the same {len(nodes)} shapes")
        sel = [r for r, n in enumerate(nodes)                                                             # :338-343
               if n in changed and objs[n] != 0 and self.classes_r.get(objs[n]) != "floor"]
        if not sel:
            return
        if as_sdf:
            from .mesh import sdf_to_mesh
            pick = torch.tensor(sel, dtype=torch.int64)
            sdfs = torch.cat([p.index_select(0, pick.to(p.device)) for p in per])
            verts = DV._verts_of(sdf_to_mesh(sdfs.to(DV._device()), render_all=True))
        else:
            verts = [p[r] for p in per for r in sel]
        C = len(sel)
        pts = DV.sample_and_normalize(verts, self.points, generator=generator).reshape(K, C, self.points, 3)
        clouds = pts.permute(1, 0, 2, 3).contiguous().reshape(C * K, self.points, 3)
        # diversity.shape_diversity's pair list (run k against run k + 1 of the same object, :393-400); its distances stay
        # on the device until summary()
        base = np.arange(C, dtype=np.int64)[:, None] * K + np.arange(K - 1, dtype=np.int64)[None, :]
        pairs = np.stack([base, base + 1], axis=-1).reshape(-1, 2)
        self._chamfer.append(DV.chamfer_pairs(clouds, pairs).reshape(C, K - 1))

    # -- read-out --
    def _launches(self):
        files = (self.file, None, self.file)                      # the third call of :411-416 passes no file_dist
        modes = (CN.MODE_CHANGED, CN.MODE_KEPT, CN.MODE_CHANGED)
        order = (0, 1, 2)
        return [CN.evaluate(self._queued[i], self.vocab, modes[i], file_dist=files[i], with_norm=True) for i in order]

    def _counts(self):
        """[3][S][11][2] int64 (satisfied, evaluated) in TABLES order: one read-back of the three launches"""
        if not self.scenes:
            return np.zeros((3, 0, len(CN.CATEGORIES), 2), np.int64)
        ls = self._launches()
        host = torch.cat([t for l in ls for t in (l.counts.reshape(-1), l.status)]).cpu().numpy()
        n = self.scenes * len(CN.CATEGORIES) * 2
        out = []
        for i in range(3):
            blk = host[i * (n + 1):(i + 1) * (n + 1)]
            if int(blk[-1]) & CN.L.STATUS_CONSTRAINT_RANGE:
                raise CN.L.CsError("constraints: a triple's ids are out of range for its scene")
            out.append(blk[:-1].reshape(self.scenes, len(CN.CATEGORIES), 2).astype(np.int64))
        # _queued is (changed, unchanged, in original graph); TABLES has the same order
        return np.stack(out)

    def lists(self) -> List[Dict[str, List[int]]]:
        """The reference's three accuracy dicts of lists (appended scene by scene in triple order), in TABLES order: a
        read-back of every verdict, for comparisons; summary() needs the counts only."""
        out = []
        for l in (self._launches() if self.scenes else []):
            acc = CN.new_accuracy()
            verdict, category = l.read_verdict(with_category=True)
            for c, v in zip(category.tolist(), verdict.tolist()):
                if v >= 0:
                    acc[CN.CATEGORIES[c]].append(v)
                    acc["total"].append(v)
            out.append(acc)
        return out or [CN.new_accuracy() for _ in range(3)]

    def diversity(self) -> dict:
        chamfer, box_rows, angles = [], [], []
        if self._chamfer:
            d = torch.cat([c.reshape(-1) for c in self._chamfer]).cpu().numpy().astype(np.float64)
            at = 0
            for c in self._chamfer:
                n = c.numel()
                chamfer += d[at:at + n].reshape(c.shape).mean(axis=1).tolist()
                at += n
        if self._boxes:
            b = torch.cat([x.reshape(-1) for x in self._boxes]).cpu().numpy()
            at = 0
            for x in self._boxes:
                n = x.numel()
                box_rows += list(DV.box_std(b[at:at + n].reshape(x.shape), file=self.file))
                at += n
        if self._angles:
            a = torch.cat([x.reshape(-1) for x in self._angles]).cpu().numpy()
            at = 0
            for x in self._angles:
                n = x.numel()
                angles += DV.angular_std(a[at:at + n].reshape(x.shape) / 24. * 360.).tolist()
                at += n
        return diversity_block(chamfer, box_rows, angles)

    def summary(self) -> dict:
        counts = self._counts()
        tables = {}
        for name, c in zip(TABLES, counts):
            per = c.sum(axis=0)
            se = {k: (int(per[i, 0]), int(per[i, 1])) for i, k in enumerate(CN.CATEGORIES)}
            se["total"] = (int(per[:, 0].sum()), int(per[:, 1].sum()))
            tables[name] = dict(table_rows(se), counts={k: list(v) for k, v in se.items()})
        return {"scenes": self.scenes, "tables": tables, "diversity": self.diversity(),
                "text": "\n".join(format_row(n, tables[n]) for n in ("changed nodes", "unchanged nodes",
                                                                       "changed nodes placed in original graph"))}


# ----------------------------------------------------------------------------------------------------------------------
# the loop
# ----------------------------------------------------------------------------------------------------------------------
def classes_of(vocab) -> Dict[str, int]:
    """dataset/threedfront_dataset.py:157-158: class name -> id from the vocabulary"""
    names = sorted(set(str(v).strip("\n") for v in vocab["object_idx_to_name"]))
    return dict(zip(names, range(len(names))))


def _noise(model, generator):
    if generator is None:
        return None                                   # the sampler's own draw, time-seeded as in the reference
    shape = tuple(model.vae_v2.Diff.z_shape) if getattr(model, "type_", "") == "v2_full" else (3, 16, 16, 16)
    return torch.randn((1,) + shape, generator=generator)


def _entries_of(model, data, num_samples, gen_shape, distribution, noise_generator):
    """one scene of the loader -> (context, its 1 + K decode entries); :255-291"""
    dev = "cuda"
    enc, dec = data["encoder"], data["decoder"]
    enc_objs, enc_triples, enc_tight = enc["objs"].to(dev), enc["tripltes"].to(dev), enc["boxes"].to(dev)
    dec_objs, dec_triples, dec_tight = dec["objs"].to(dev), dec["tripltes"].to(dev), dec["boxes"].to(dev)
    enc_boxes = enc_tight[:, :6]
    enc_angles = enc_tight[:, 6].long() - 1                                            # :267-270
    enc_angles = torch.where(enc_angles > 0, enc_angles, torch.zeros_like(enc_angles))
    enc_angles = torch.where(enc_angles < 24, enc_angles, torch.zeros_like(enc_angles))
    (z_box, _), _ = model.encode_box_and_shape(enc_objs, enc_triples, enc["text_feats"].to(dev), enc["rel_feats"].to(dev),
                                               None, enc_boxes, enc_angles, None)
    missing, manipulated = list(data["missing_nodes"]), list(data["manipulated_nodes"])
    base = dict(z_box=z_box, z=z_box, objs=dec_objs, triples=dec_triples, encoded_dec_text_feat=dec["text_feats"].to(dev),
                encoded_dec_rel_feat=dec["rel_feats"].to(dev), dec_sdfs=dec.get("sdfs"), attributes=None,
                missing_nodes=missing, manipulated_nodes=manipulated, distribution=distribution)
    K = int(num_samples) if (missing or manipulated) else 0                            # :297
    entries = [dict(base, x_T=_noise(model, noise_generator) if gen_shape else None) for _ in range(1 + K)]
    changed = sorted(set(m + i for i, m in enumerate(missing)) | set(manipulated))
    ctx = dict(dec_objs=dec["objs"].tolist(), dec_triples=dec_triples, dec_tight=dec_tight, changed=changed, K=K)
    return ctx, entries


def _split(pred):
    return (pred[0], pred[1]) if isinstance(pred, (tuple, list)) else (pred, None)


def _shaped_nodes(dec_sdfs) -> List[int]:
    return torch.unique(torch.where(torch.ne(dec_sdfs, torch.zeros_like(dec_sdfs[0])))[0]).tolist()


@torch.no_grad()
def manipulation_loop(model, loader, mode: str, num_samples: int = 3, gen_shape: bool = True, ddim_steps: int = 100,
                      batch_scenes: int = 1, shape_nodes: str = "all", meter: Optional[ManipulationMeter] = None,
                      distribution=None, noise_generator: Optional[torch.Generator] = None,
                      points_generator: Optional[torch.Generator] = None, file=None, points: int = 5000) -> dict:
    """eval_3dfront.py:206-441 over `loader` (what make_edit returns per scene; None / -1 entries are skipped and counted).

    mode 'relationship' decodes through decoder_with_changes_* (the reference's args.manipulate=True), 'addition' through
    decoder_with_additions_*.  Per scene: enc_angles clamped as :267-270, z_box = the encoder mean, one main decode (its
    boxes feed the three tables; its shapes are never read at :401-416 and are not sampled), and -- only when a node was
    added or manipulated -- K = num_samples diversity decodes, then the meter.  batch_scenes = 1 is the reference's regime:
    one per-scene facade call per decode.  batch_scenes > 1 sends that many scenes' 1 + K decodes through ONE call of the
    facade's `_many` route (one coalesced sampler); numpy's draws keep the scene-by-scene order (the RNG contract of
    Sg2ScVAEModel._manipulation_many).  shape_nodes='changed' samples only the changed nodes' shapes -- all the meter reads.
    `noise_generator` draws every decode's x_T (None: the sampler's time-seeded draw, as in the reference);
    `points_generator` draws the meter's rows.  Returns the meter's summary plus 'skipped' and 'decodes'."""
    if mode not in ("relationship", "addition"):
        raise ValueError(f"mode must be 'relationship' or 'addition', got {mode!r}")
    if num_samples == 1:
        raise ValueError("Diversity requires at least two runs (i.e. num_samples > 1).")      # :207-208
    if batch_scenes < 1:
        raise ValueError("batch_scenes must be at least 1")
    if meter is None:
        meter = ManipulationMeter(model.vocab, classes_of(model.vocab), file=file, points=points)
    changes = mode == "relationship"
    one = model.decoder_with_changes_boxes_and_shape if changes else model.decoder_with_additions_boxes_and_shape
    many = model.decoder_with_changes_boxes_and_shape_many if changes else model.decoder_with_additions_boxes_and_shape_many
    skipped = decodes = 0

    def run_entries(entries, flags):
        """flags[i]: sample entry i's shapes"""
        outs = [None] * len(entries)
        if batch_scenes == 1 and shape_nodes == "all":
            for i, e in enumerate(entries):
                kw = dict(gen_shape=flags[i], ddim_steps=ddim_steps, x_T=e["x_T"])
                if e["distribution"] is not None:
                    kw["distribution"] = e["distribution"]
                outs[i] = one(e["z_box"], None, e["objs"], e["triples"], e["encoded_dec_text_feat"],
                              e["encoded_dec_rel_feat"], e["dec_sdfs"], None, e["missing_nodes"], e["manipulated_nodes"], **kw)
            return outs
        if batch_scenes == 1:
            for i, e in enumerate(entries):
                outs[i] = many([e], gen_shape=flags[i], ddim_steps=ddim_steps, shape_nodes=shape_nodes)[0]
            return outs
        # coalesced: ONE `_many` call builds every entry's latent in entry order (numpy's draws) and samples the flagged
        # entries' shapes together; the main decodes ride along without shapes
        if all(flags) or not any(flags):
            return many(entries, gen_shape=bool(flags and flags[0]), ddim_steps=ddim_steps, shape_nodes=shape_nodes)
        return _ordered_many(model, changes, entries, flags, ddim_steps, shape_nodes)

    def flush(batch):
        nonlocal decodes
        entries, flags = [], []
        for ctx, es in batch:
            entries += es
            flags += [False] + [bool(gen_shape)] * ctx["K"]
        outs = run_entries(entries, flags)
        decodes += len(entries)
        at = 0
        for ctx, es in batch:
            mine = outs[at:at + len(es)]
            at += len(es)
            boxes_pred, _ = _split(mine[0][0])
            runs = []
            for pred, shapes, keep in mine[1:]:
                b, a = _split(pred)
                nodes = None
                if isinstance(shapes, tuple):
                    shapes, nodes = shapes
                runs.append((b, a, shapes, keep, nodes))
            nodes = None
            if runs and runs[0][2] is not None:
                nodes = runs[0][4] if runs[0][4] is not None else _shaped_nodes(es[0]["dec_sdfs"])
            meter.add_scene(ctx["dec_triples"], boxes_pred, ctx["dec_tight"], mine[0][2], runs=[r[:4] for r in runs] or None,
                            dec_objs=ctx["dec_objs"], changed=ctx["changed"], shape_nodes=nodes,
                            generator=points_generator)

    batch = []
    for data in loader:
        if data is None or (not isinstance(data, dict) and data == -1):
            skipped += 1
            continue
        batch.append(_entries_of(model, data, num_samples, gen_shape, distribution, noise_generator))
        if len(batch) >= batch_scenes:
            flush(batch)
            batch = []
    if batch:
        flush(batch)
    out = meter.summary()
    out.update(skipped=skipped, decodes=decodes, mode=mode, batch_scenes=int(batch_scenes), shape_nodes=shape_nodes)
    return out


def _ordered_many(model, changes, entries, flags, ddim_steps, shape_nodes):
    """`_many` over entries of which only some sample shapes, latents built in ENTRY order.  The model's `_many` builds
    every entry's latent in order before sampling; an entry without a flag is given an all-zero dec_sdfs, so it contributes
    no object to the sampler and answers with an empty shape batch, which is dropped here."""
    es = []
    for e, f in zip(entries, flags):
        if f or e["dec_sdfs"] is None:
            es.append(e)
        else:
            es.append(dict(e, dec_sdfs=torch.zeros_like(e["dec_sdfs"])))
    many = model.decoder_with_changes_boxes_and_shape_many if changes else model.decoder_with_additions_boxes_and_shape_many
    outs = many(es, gen_shape=True, ddim_steps=ddim_steps, shape_nodes=shape_nodes)
    return [o if f else (o[0], None, o[2]) for o, f in zip(outs, flags)]


# ----------------------------------------------------------------------------------------------------------------------
# before / after
# ----------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def edit_scene(model, scene: dict, edit: dict, mode: Optional[str] = None, ddim_steps: int = 100, shape_nodes: str = "all",
               file=None, z=None, x_T_before=None, x_T_after=None, distribution=None) -> dict:
    """eval_3dfront_manivis.py:298-380 for one edit (what make_edit returned for `scene`): sample the ORIGINAL graph (the
    encoder graph), encode the GENERATED boxes and argmax angles, decode the edited graph, and build the "after" scene as
    render_v2_full(mani=2) does -- unchanged objects keep their "before" meshes and boxes, the added / manipulated nodes get
    new ones.  `scene` (the unedited scene) is not read: `edit` carries both graphs.  Returns dict(before=(Meshes, box_and_angle [O_enc, 7], cats), after=(Meshes, box_and_angle [O_dec, 7], cats),
    changed=[decoder nodes], before_of=[encoder node of each decoder node | None]); the mesh lists are in node order over
    the shaped nodes, as scene_mesh.assemble_scene / render_topdown take them.  shape_nodes='changed': the second sampler
    run covers only the changed nodes.  z / x_T_*: injected latents and noise (default: the reference's draws)."""
    from .mesh import Meshes, sdf_to_mesh
    dev = "cuda"
    enc, dec = edit["encoder"], edit["decoder"]
    missing, manipulated = list(edit["missing_nodes"]), list(edit["manipulated_nodes"])
    if mode is None:
        mode = "addition" if missing else "relationship"
    enc_objs, enc_triples = enc["objs"].to(dev), enc["tripltes"].to(dev)
    enc_text, enc_rel = enc["text_feats"].to(dev), enc["rel_feats"].to(dev)
    dec_objs, dec_triples = dec["objs"].to(dev), dec["tripltes"].to(dev)
    dec_sdfs = dec["sdfs"]
    # the encoder graph's SDF rows: the decoder's without the added nodes (the reference's data['encoder']['sdfs'])
    enc_rows = [i for i in range(dec_sdfs.shape[0]) if i not in missing]
    enc_sdfs = dec_sdfs[enc_rows]
    inject = {k: v for k, v in (("z", z), ("x_T", x_T_before)) if v is not None}
    (boxes0, angles0), shapes0 = model.sample_box_and_shape(None, enc_objs, enc_triples, enc_sdfs, enc_text, enc_rel,
                                                             attributes=None, gen_shape=True, ddim_steps=ddim_steps,
                                                             **inject)
    bins0 = torch.argmax(angles0, dim=1)                                                # :305
    deg0 = -180 + (bins0.unsqueeze(1) + 1) * 15.0                                       # :306-307
    den = lambda b: _denormalize(b, file)
    before_boxes = torch.cat([den(boxes0), deg0.float()], dim=1)
    meshes0 = sdf_to_mesh(shapes0, render_all=True)
    (z_box, _), _ = model.encode_box_and_shape(enc_objs, enc_triples, enc_text, enc_rel, None, boxes0, bins0, None)    # :346
    entry = dict(z_box=z_box, z=z_box, objs=dec_objs, triples=dec_triples, encoded_dec_text_feat=dec["text_feats"].to(dev),
                 encoded_dec_rel_feat=dec["rel_feats"].to(dev), dec_sdfs=dec_sdfs, attributes=None, missing_nodes=missing,
                 manipulated_nodes=manipulated, distribution=distribution, x_T=x_T_after)
    many = model.decoder_with_changes_boxes_and_shape_many if mode == "relationship" \
        else model.decoder_with_additions_boxes_and_shape_many
    (boxes1, angles1), shapes1, keep = many([entry], gen_shape=True, ddim_steps=ddim_steps, shape_nodes=shape_nodes)[0]
    shaped_dec = _shaped_nodes(dec_sdfs)
    if isinstance(shapes1, tuple):
        shapes1, new_nodes = shapes1
    else:
        new_nodes = shaped_dec
    deg1 = -180 + (torch.argmax(angles1, dim=1, keepdim=True) + 1) * 15.0               # :353-354
    after_new = torch.cat([den(boxes1), deg1.float()], dim=1)
    meshes1 = sdf_to_mesh(shapes1, render_all=True)
    changed = sorted(set(m + i for i, m in enumerate(missing)) | set(manipulated))
    added = set(m + i for i, m in enumerate(missing))
    before_of, e = [], 0
    for n in range(dec_objs.shape[0]):
        if n in added:
            before_of.append(None)
        else:
            before_of.append(e)
            e += 1
    shaped_enc = _shaped_nodes(enc_sdfs)
    row0 = {n: r for r, n in enumerate(shaped_enc)}
    row1 = {n: r for r, n in enumerate(new_nodes)}
    v0, f0, v1, f1 = meshes0.verts_list(), meshes0.faces_list(), meshes1.verts_list(), meshes1.faces_list()
    verts, faces, rows = [], [], []
    for n in range(dec_objs.shape[0]):
        fresh = n in changed or before_of[n] is None
        rows.append(after_new[n] if fresh else before_boxes[before_of[n]])
        if n not in shaped_dec:
            continue
        if fresh or before_of[n] not in row0:
            verts.append(v1[row1[n]])
            faces.append(f1[row1[n]])
        else:
            verts.append(v0[row0[before_of[n]]])
            faces.append(f0[row0[before_of[n]]])
    return dict(before=(meshes0, before_boxes, enc_objs.tolist()),
                after=(Meshes(verts, faces), torch.stack(rows), dec_objs.tolist()), changed=changed, before_of=before_of,
                keep=keep)


def _denormalize(boxes: Tensor, file=None) -> Tensor:
    """batch_torch_denormalize_box_params (helpers/util.py:566-580) on [O, 6] device boxes: x * std / 3 + mean, elementwise"""
    mean, std = DV.box_stats(file)
    m = torch.tensor(mean, dtype=torch.float32).to(boxes.device)
    s = torch.tensor(std, dtype=torch.float32).to(boxes.device)
    return boxes.float() * s / 3 + m
