"""Scene manipulation on the MI355X (commonscenes_amd/manipulation.py, the `_many` decodes of scene.py / vae.py,
tools/manipulation_table.py): the three accuracy tables against the reference's own lists (tests/golden/manipulation.npz),
the coalesced decodes against the per-scene calls, the loop against a scene-by-scene restatement, the before / after scenes
and the tool.  UNet width 32, 2 DDIM steps, at most 8 objects per scene, 256 points.  Every figure is printed before it is
asserted."""
import importlib.util
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rel_l2

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
LATENT_GATE = 1e-5          # tests/test_vae_facade_gpu.py:186: coalesced sampling against the per-scene call
DIVERSITY_GATE = 1e-6       # tests/test_diversity_gpu.py (test_shape_diversity): device route against the host route
P = 256


def _tool():
    spec = importlib.util.spec_from_file_location("manipulation_table", ROOT / "tools" / "manipulation_table.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN / "manipulation.npz")


@pytest.fixture(scope="module")
def rig(tmp_path_factory):
    """the width-32 v2_full VAE on synthetic weights and the synthetic names, built once"""
    T = _tool()
    W = T._walkthrough()
    model = T.build_model(W, tmp_path_factory.mktemp("exp"), 32)
    classes, names, rels, eval_vocab = T.synthetic_names(W)
    return dict(T=T, W=W, model=model, classes=classes, names=names, rels=rels, eval_vocab=eval_vocab)


def _close(a, b):
    """max |a - b| / max |b| over the figures both hold; None must match None"""
    worst = 0.0
    for x, y in zip(a, b):
        assert (x is None) == (y is None), (a, b)
        if x is not None:
            worst = max(worst, abs(x - y) / max(abs(y), 1e-30) if y != 0 else abs(x))
    return worst


DIV_KEYS = ("shape", "box_size", "box_location", "angle")


# 4 ------------------------------------------------------------------------------------------------------------------
def _gold_lists(gold, tag):
    keys = [str(k) for k in gold["keys"].tolist()]
    flat, at, out = gold[f"acc_{tag}"], 0, {}
    for k, n in zip(keys, gold[f"len_{tag}"].tolist()):
        out[k] = flat[at:at + n].tolist()
        at += n
    return out, keys


def test_three_tables_equal_the_reference_lists(gold, tmp_path):
    from commonscenes_amd import manipulation as MP
    vocab = {"pred_idx_to_name": [str(p) + "\n" for p in gold["pred_names"].tolist()]}
    stats = tmp_path / "boxes_stats.txt"
    np.savetxt(stats, gold["t_stats"])
    bp, tp = gold["t_box_ptr"].tolist(), gold["t_triple_ptr"].tolist()
    scenes = []
    for s in range(len(bp) - 1):
        scenes.append((torch.from_numpy(gold["t_triples"][tp[s]:tp[s + 1]]).cuda(),
                       torch.from_numpy(gold["t_boxes"][bp[s]:bp[s + 1]]).cuda(),
                       torch.from_numpy(gold["t_gt"][bp[s]:bp[s + 1]]).cuda(),
                       torch.from_numpy(gold["t_keep"][bp[s]:bp[s + 1]].astype(np.float32)).reshape(-1, 1).cuda()))
    assert len(scenes) == 12
    tags = ("changed", "unchanged", "orig")                      # MP.TABLES order
    want = [_gold_lists(gold, t)[0] for t in tags]
    keys = _gold_lists(gold, "changed")[1]
    whole = MP.ManipulationMeter(vocab, {"floor": 1}, file=str(stats))
    for sc in scenes:
        whole.add_scene(*sc)
    got = whole.lists()
    for t, g, w in zip(tags, got, want):
        print(f"table {t}: {len(g['total'])} verdicts, {sum(g['total'])} satisfied (reference {len(w['total'])}, "
              f"{sum(w['total'])})")
        assert g == w, t
    summary = whole.summary()
    for t, name, w in zip(tags, MP.TABLES, want):
        counts = summary["tables"][name]["counts"]
        assert {k: tuple(v) for k, v in counts.items()} == {k: (sum(w[k]), len(w[k])) for k in keys}
        assert summary["tables"][name]["Total"] == sum(w["total"]) / len(w["total"])
    # the third call passes no file: with the default statistics everywhere the "unchanged" table is the same, the others move
    plain = MP.ManipulationMeter(vocab, {"floor": 1}, file=None)
    for sc in scenes:
        plain.add_scene(*sc)
    pl = plain.lists()
    assert pl[1] == got[1] and pl[0] != got[0]
    # scene by scene
    for s, sc in enumerate(scenes):
        one = MP.ManipulationMeter(vocab, {"floor": 1}, file=str(stats))
        one.add_scene(*sc)
        ls = one.lists()
        for t, g, w in zip(tags, ls, want):
            lens = gold[f"scene_len_{t}"]
            for j, k in enumerate(keys):
                at = int(lens[:s, j].sum())
                assert g[k] == w[k][at:at + int(lens[s, j])], (t, s, k)


# 5 ------------------------------------------------------------------------------------------------------------------
def _entries(seed=60, n=6):
    """an addition with a distribution, a relationship change, and the second again"""
    from commonscenes_amd import synth
    g = synth.random_scene_graph(n, seed=seed)
    O = g["objs"].shape[0]
    dec_sdfs = torch.zeros(O, 1, 4, 4, 4)
    dec_sdfs[:n] = 1.0
    z = synth.gaussian_like(f"mp:z{seed}", (O, 64))
    common = dict(dec_objs=g["objs"], dec_triples=g["triples"], encoded_dec_text_feat=g["text_feats"],
                  encoded_dec_rel_feat=g["rel_feats"], dec_sdfs=dec_sdfs, attributes=None)
    x = lambda i: synth.gaussian_like(f"mp:x{seed}:{i}", (1, 3, 16, 16, 16))
    add = dict(common, z=torch.cat([z[:2], z[3:]]), missing_nodes=[2], manipulated_nodes=[],
               distribution=(np.zeros(64), np.eye(64)), x_T=x(0))
    rel = dict(common, z=z, missing_nodes=[], manipulated_nodes=[1, 4], x_T=x(1))
    return [add, rel, dict(rel, x_T=x(2))], n


def _sequential(m, entries, changes):
    out = []
    for e in entries:
        fn = m.decoder_with_changes if changes else m.decoder_with_additions
        pred, sdf, keep = fn(e["z"], e["dec_objs"], e["dec_triples"], e["encoded_dec_text_feat"], e["encoded_dec_rel_feat"],
                             e["dec_sdfs"], None, e["missing_nodes"], e["manipulated_nodes"],
                             distribution=e.get("distribution"), gen_shape=True, x_T=e["x_T"], ddim_steps=2)
        out.append((pred, sdf, keep, m.Diff.last_latents.clone()))
    return out


@pytest.mark.parametrize("changes", [True, False])
def test_many_against_sequential_calls(rig, changes):
    m = rig["model"].vae_v2
    entries, n = _entries()
    np.random.seed(11)
    seq = _sequential(m, entries, changes)
    np.random.seed(11)
    many = (m.decoder_with_changes_many if changes else m.decoder_with_additions_many)(entries, gen_shape=True, ddim_steps=2)
    lat = m.Diff.last_latents
    torch.cuda.synchronize()
    assert len(many) == 3 and lat.shape[0] == 3 * n and sum(m.Diff.last_launch_sizes) == 3 * n
    for i, ((pred, sdf, keep), (rpred, rsdf, rkeep, rlat)) in enumerate(zip(many, seq)):
        err = rel_l2(lat[i * n:(i + 1) * n], rlat)
        print(f"changes={changes} entry {i}: latents rel-L2 vs the per-scene call {err:.3e}; SDF rel-L2 {rel_l2(sdf, rsdf):.3e}")
        assert torch.equal(pred[0], rpred[0]) and torch.equal(pred[1], rpred[1]) and torch.equal(keep, rkeep)
        assert sdf.shape == (n, 1, 64, 64, 64) and err < LATENT_GATE
    assert many[0][2].reshape(-1).tolist() == [1, 1, 0, 1, 1, 1, 1, 1]
    assert many[1][2].reshape(-1).tolist() == ([1, 0, 1, 1, 0, 1, 1, 1] if changes else [1, 0, 1, 1, 0, 1, 1, 1])
    if changes:                     # the repeat drew other change rows: its changed boxes differ, the RNG moved on
        assert not torch.equal(many[1][0][0], many[2][0][0])
    # the facade answers with the model's answers
    np.random.seed(11)
    fac = rig["model"]
    f = (fac.decoder_with_changes_boxes_and_shape_many if changes else fac.decoder_with_additions_boxes_and_shape_many)(
        [dict(e, z_box=e["z"], objs=e["dec_objs"], triples=e["dec_triples"]) for e in entries], gen_shape=False, ddim_steps=2)
    assert all(o[1] is None for o in f) and all(torch.equal(a[0][0], b[0][0]) for a, b in zip(f, many))
    with pytest.raises(ValueError):
        m.decoder_with_changes_many(entries, shape_nodes="some")


def test_one_entry_many_meets_the_reference_gates(tmp_path):
    """the gates of tests/test_model_gpu.py::test_v2full_manipulation_surface_vs_reference_golden, on the `_many` route"""
    from test_model_gpu import _g, _record_latents, _scene, _sdf_gates
    g = _g("full_manip_small")
    m = _scene(tmp_path)
    t = lambda k: torch.from_numpy(np.ascontiguousarray(g[k]))
    O = t("objs").shape[0]
    dec_sdfs = torch.zeros(O, 1, 4, 4, 4)
    dec_sdfs[t("dec_sdfs_nonzero")] = 1.0
    lat = _record_latents(m)
    np.random.seed(1234)
    [((d3c, angc), gen, keepc)] = m.decoder_with_changes_many(
        [dict(z=t("z_in"), dec_objs=t("objs"), dec_triples=t("triples"), encoded_dec_text_feat=t("text_feats"),
              encoded_dec_rel_feat=t("rel_feats"), dec_sdfs=dec_sdfs, attributes=None, missing_nodes=[2],
              manipulated_nodes=[4], x_T=t("x_T"))], gen_shape=True, ddim_steps=2)
    torch.cuda.synchronize()
    assert gen.shape == (6, 1, 64, 64, 64)
    for mine, key in ((d3c, "d3_changes"), (angc, "angles_changes")):
        err = rel_l2(mine, t(key))
        print(f"one-entry _many {key}: rel-L2 vs the reference {err:.3e}")
        assert err < 3e-6, key
    assert torch.equal(keepc.cpu(), t("keep_changes"))
    _sdf_gates(m, g, gen, lat, "full_manip_small through decoder_with_changes_many")


# 6 ------------------------------------------------------------------------------------------------------------------
def test_shape_nodes_changed_samples_fewer_objects(rig):
    m = rig["model"].vae_v2
    entries, n = _entries(seed=61)
    entries[1] = dict(entries[1], manipulated_nodes=[1, n])            # node n is the floor: changed, but it has no shape
    np.random.seed(12)
    full = m.decoder_with_changes_many(entries, gen_shape=True, ddim_steps=2, shape_nodes="all")
    lat_all = m.Diff.last_latents.clone()
    np.random.seed(12)
    part = m.decoder_with_changes_many(entries, gen_shape=True, ddim_steps=2, shape_nodes="changed")
    lat = m.Diff.last_latents
    torch.cuda.synchronize()
    want_nodes = [[2], [1], [1, 4]]
    at = 0
    for i, ((pred, (sdf, nodes), keep), (rpred, rsdf, rkeep)) in enumerate(zip(part, full)):
        k = keep.reshape(-1).tolist()
        assert nodes == [j for j in range(n) if k[j] == 0] == want_nodes[i]
        assert torch.equal(pred[0], rpred[0]) and torch.equal(keep, rkeep) and sdf.shape[0] == len(nodes)
        rows = [i * n + j for j in nodes]
        err = rel_l2(lat[at:at + len(nodes)], lat_all[rows])
        print(f"entry {i}: nodes {nodes}; latents vs the same rows of the 'all' run rel-L2 {err:.3e}")
        assert err < LATENT_GATE
        at += len(nodes)
    assert lat.shape[0] == at == 4 and lat_all.shape[0] == 3 * n and sum(m.Diff.last_launch_sizes) == 4


# 7 ------------------------------------------------------------------------------------------------------------------
def _run_loop(rig, edits, mode, batch_scenes, shape_nodes="all"):
    from commonscenes_amd import manipulation as MP
    model = rig["model"]
    np.random.seed(21)
    meter = MP.ManipulationMeter(rig["eval_vocab"], rig["classes"], points=P)
    dist = (model.mean_est, model.cov_est) if mode == "addition" else None
    return MP.manipulation_loop(model, edits, mode, num_samples=2, gen_shape=True, ddim_steps=2, batch_scenes=batch_scenes,
                                shape_nodes=shape_nodes, meter=meter, distribution=dist,
                                noise_generator=torch.Generator().manual_seed(5),
                                points_generator=torch.Generator().manual_seed(6))


def _local_loop(rig, edits, mode):
    """eval_3dfront.py:228-416 scene by scene from the per-scene facade calls, validate_constrains* and the host Chamfer"""
    from commonscenes_amd import constraints as CN, diversity as D
    from commonscenes_amd.chamfer import chamferDist
    from commonscenes_amd.mesh import sdf_to_mesh
    model, vocab, classes = rig["model"], rig["eval_vocab"], rig["classes"]
    floor = classes["floor"]
    np.random.seed(21)
    noise, rows = torch.Generator().manual_seed(5), torch.Generator().manual_seed(6)
    draw = lambda: torch.randn((1, 3, 16, 16, 16), generator=noise)
    acc = [CN.new_accuracy() for _ in range(3)]
    chamfer, all_boxes, all_angles, dist_fn = [], [], [], chamferDist()
    kw = dict(distribution=(model.mean_est, model.cov_est)) if mode == "addition" else {}
    call = model.decoder_with_changes_boxes_and_shape if mode == "relationship" else model.decoder_with_additions_boxes_and_shape
    for data in edits:
        if data is None:
            continue
        enc, dec = data["encoder"], data["decoder"]
        tight = enc["boxes"].cuda()
        ang = tight[:, 6].long() - 1
        ang = torch.where(ang > 0, ang, torch.zeros_like(ang))
        ang = torch.where(ang < 24, ang, torch.zeros_like(ang))
        (z_box, _), _ = model.encode_box_and_shape(enc["objs"].cuda(), enc["tripltes"].cuda(), enc["text_feats"].cuda(),
                                                   enc["rel_feats"].cuda(), None, tight[:, :6], ang, None)
        args = (z_box, None, dec["objs"].cuda(), dec["tripltes"].cuda(), dec["text_feats"].cuda(), dec["rel_feats"].cuda(),
                dec["sdfs"], None, data["missing_nodes"], data["manipulated_nodes"])
        (boxes, _), _, keep = call(*args, gen_shape=False, ddim_steps=2, x_T=draw(), **kw)
        runs = []
        for _ in range(2):
            (b, a), sdf, k = call(*args, gen_shape=True, ddim_steps=2, x_T=draw(), **kw)
            runs.append((b, a, sdf, k))
        k0 = runs[0][3].reshape(-1).cpu().tolist()
        objs = dec["objs"].tolist()
        changed = [i for i, v in enumerate(k0) if v == 0]
        shaped = [i for i in range(len(objs)) if bool((dec["sdfs"][i] != 0).any())]
        sel = [r for r, node in enumerate(shaped) if node in changed and objs[node] != 0 and objs[node] != floor]
        if sel:
            verts = sdf_to_mesh(torch.cat([r[2][sel] for r in runs]), render_all=True).verts_list()
            pts = D.sample_and_normalize(verts, P, generator=rows).reshape(2, len(sel), P, 3)
            for c in range(len(sel)):                                               # eval_3dfront.py:393-400
                d1, d2 = dist_fn(pts[0, c:c + 1].float(), pts[1, c:c + 1].float())
                chamfer.append(float(d1.double().mean() + d2.double().mean()))
        bx = torch.stack([r[0][changed] for r in runs], 1).cpu().numpy().astype(np.float64)
        den = bx * np.array(D.BOX_STD)[None, None] / 3 + np.array(D.BOX_MEAN)[None, None]
        all_boxes += den.std(axis=1, ddof=1).tolist()
        degs = np.stack([np.argmax(r[1][changed].cpu().numpy(), 1) for r in runs], 1) / 24. * 360.
        all_angles += [D.estimate_angular_std(d) for d in degs]
        gt = dec["boxes"].cuda()
        bp = torch.stack([boxes[i] if k0[i] == 0 else gt[i, :6] for i in range(len(k0))], 0)
        tri = dec["tripltes"].cuda()
        CN.validate_constrains_changes(tri, boxes, gt, keep, vocab, acc[0], with_norm=True)
        CN.validate_constrains(tri, boxes, gt, keep, vocab, acc[1], with_norm=True)
        CN.validate_constrains_changes(tri, bp, gt, keep, vocab, acc[2], with_norm=True)
    box = np.mean(np.asarray(all_boxes), axis=0)
    div = dict(shape=float(np.mean(chamfer)) if chamfer else None, box_size=float(np.mean(box[:3])),
               box_location=float(np.mean(box[3:])), angle=float(np.mean(all_angles)), shapes=len(chamfer))
    return acc, div


@pytest.mark.parametrize("mode", ["relationship", "addition"])
def test_loop_batched_sequential_and_local(rig, mode):
    from commonscenes_amd import manipulation as MP
    edits = rig["T"].synthetic_edits(rig["W"], 3, mode, rig["classes"], rig["rels"])
    assert all(e is not None for e in edits)
    edits = edits[:1] + [None] + edits[1:]                            # a scene whose edit found nothing: skipped, counted
    seq = _run_loop(rig, edits, mode, 1)
    bat = _run_loop(rig, edits, mode, 3)
    launches = list(rig["model"].vae_v2.Diff.last_launch_sizes)
    acc, div = _local_loop(rig, edits, mode)
    print(f"[{mode}] tables (batch_scenes=1):\n{seq['text']}\n[{mode}] diversity 1: {seq['diversity']}\n"
          f"[{mode}] diversity 3: {bat['diversity']}\n[{mode}] diversity local: {div}; last coalesced launch sizes {launches}")
    assert seq["skipped"] == bat["skipped"] == 1 and seq["scenes"] == bat["scenes"] == 3 and seq["decodes"] == 9
    assert seq["tables"] == bat["tables"]
    for name, a in zip(MP.TABLES, acc):
        want = {k: [int(sum(v)), len(v)] for k, v in a.items()}
        assert seq["tables"][name]["counts"] == want, name
    assert seq["tables"]["changed nodes"]["counts"]["total"][1] > 0
    d_bat = _close([bat["diversity"][k] for k in DIV_KEYS], [seq["diversity"][k] for k in DIV_KEYS])
    d_loc = _close([seq["diversity"][k] for k in DIV_KEYS], [div[k] for k in DIV_KEYS])
    print(f"[{mode}] diversity: batch_scenes=3 vs 1 worst relative difference {d_bat:.3e}; batch_scenes=1 vs the local "
          f"scene-by-scene run {d_loc:.3e}")
    assert seq["diversity"]["shapes"] == bat["diversity"]["shapes"] == div["shapes"] > 0
    assert d_bat < DIVERSITY_GATE and d_loc < DIVERSITY_GATE
    # shape_nodes='changed' feeds the meter the same clouds' worth of shapes from fewer sampled objects
    part = _run_loop(rig, edits, mode, 3, shape_nodes="changed")
    assert part["tables"] == seq["tables"] and part["diversity"]["shapes"] == seq["diversity"]["shapes"]
    assert sum(rig["model"].vae_v2.Diff.last_launch_sizes) < sum(launches)


# 8 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["relationship", "addition"])
def test_edit_scene_before_and_after(rig, mode):
    from commonscenes_amd import manipulation as MP, scene_mesh as S
    edit = rig["T"].synthetic_edits(rig["W"], 1, mode, rig["classes"], rig["rels"])[0]
    x = lambda s: torch.randn((1, 3, 16, 16, 16), generator=torch.Generator().manual_seed(s))
    np.random.seed(3)
    res = MP.edit_scene(rig["model"], None, edit, ddim_steps=2, x_T_before=x(1), x_T_after=x(2))
    nodes_all = rig["model"].vae_v2.Diff.last_latents.shape[0]
    before = S.assemble_scene(*res["before"], rig["names"], floor=False)
    after = S.assemble_scene(*res["after"], rig["names"], floor=False)
    torch.cuda.synchronize()
    b_objs, a_objs = dict(zip(before.kept, before.per_object())), dict(zip(after.kept, after.per_object()))
    n_dec = len(res["after"][2])
    shaped = [n for n in range(n_dec) if rig["names"][res["after"][2][n]].strip() not in ("_scene_", "floor")]
    assert after.kept == shaped and res["changed"] and set(res["changed"]) <= set(range(n_dec))
    # face_object ids follow node order
    ids = after.face_object.cpu().tolist()
    assert ids == sorted(ids) and sorted(set(ids)) == [n for n in shaped if a_objs[n].faces.shape[0] > 0]
    same = differ = 0
    for n in shaped:
        e = res["before_of"][n]
        if n in res["changed"]:
            differ += 1
            assert e is None or not (a_objs[n].vertices.shape == b_objs[e].vertices.shape and
                                     torch.equal(a_objs[n].vertices, b_objs[e].vertices))
        else:
            same += 1
            assert torch.equal(a_objs[n].vertices, b_objs[e].vertices) and torch.equal(a_objs[n].faces, b_objs[e].faces)
    print(f"[{mode}] after scene: {same} objects bit-equal to before, {differ} changed; changed nodes {res['changed']}")
    assert same > 0 and differ > 0
    if mode == "addition":
        assert len(after.kept) == len(before.kept) + 1 and res["before_of"].count(None) == 1
    else:
        assert len(after.kept) == len(before.kept)
    # shape_nodes='changed': the second sampler run covers the changed nodes only
    np.random.seed(3)
    part = MP.edit_scene(rig["model"], None, edit, ddim_steps=2, x_T_before=x(1), x_T_after=x(2), shape_nodes="changed")
    n_part = rig["model"].vae_v2.Diff.last_latents.shape[0]
    assert n_part == len([n for n in res["changed"] if n in shaped]) < nodes_all
    again = S.assemble_scene(*part["after"], rig["names"], floor=False)
    for n, (p, q) in enumerate(zip(again.per_object(), after.per_object())):
        if after.kept[n] not in res["changed"]:
            assert torch.equal(p.vertices, q.vertices)


# 9 ------------------------------------------------------------------------------------------------------------------
def test_tool_prints_the_table_and_exports(tmp_path):
    from PIL import Image
    out = tmp_path / "scenes"
    cmd = ["timeout", "-k", "10", "600", sys.executable, str(ROOT / "tools" / "manipulation_table.py"), "--synthetic",
           "--mode", "relationship", "--scenes", "2", "--samples", "2", "--points", str(P), "--batch-scenes", "2",
           "--export-scenes", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(ROOT))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("MANIPULATION_TABLE ")]
    assert len(lines) == 1
    d = json.loads(lines[0].split(" ", 1)[1])
    assert set(d["tables"]) == {"changed nodes", "unchanged nodes", "changed nodes placed in original graph"}
    for row in d["tables"].values():
        assert {"L/R", "F/B", "Bi/Sm", "Ta/Sh", "Stand", "Close", "Symm", "Total", "means of mean", "counts"} <= set(row)
    assert {"shape", "box_size", "box_location", "angle", "shapes", "boxes", "angles"} <= set(d["diversity"])
    assert d["scenes"] == 2 and d["diversity"]["shape"] is not None and d["diversity"]["shape"] >= 0
    assert len(d["export"]) == 2
    for e in d["export"]:
        assert len(e["files"]) == 4 and e["files"][0] == f"{e['scan']}_before.obj"
        assert e["files"][2] == f"{e['scan']}_after_{e['label']}.obj"
        for f in e["files"]:
            assert (out / f).is_file() and (out / f).stat().st_size > 0
            if f.endswith(".png"):
                assert Image.open(out / f).size == (256, 256)
