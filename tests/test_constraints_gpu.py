"""Scene-graph constraint accuracy on the device (csrc/cs_constraints.hip through commonscenes_amd/constraints.py) against
tests/golden/constraints.npz: what helpers/metrics_3dfront.py:57-311 (validate_constrains, validate_constrains_changes) and
:337-370 (box3d_iou) answered for the same scenes on the CPU (tools/make_goldens.py g_constraints)."""
import importlib.util
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu
KEYS = ["left", "right", "front", "behind", "bigger", "smaller", "taller", "shorter", "standing on", "close by",
        "symmetrical to", "total"]


@pytest.fixture(scope="module")
def G():
    g = np.load(ROOT / "tests" / "golden" / "constraints.npz")
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def vocab(G):
    return {"pred_idx_to_name": [str(n) + "\n" for n in G["pred_names"]]}


def _scenes(G, tag, with_keep=True):
    """[(triples, boxes, keep)] on the device, uploaded once per scene"""
    bp, tp = G[tag + "box_ptr"], G[tag + "triple_ptr"]
    boxes, tri, keep = (torch.from_numpy(G[tag + k]).cuda() for k in ("boxes", "triples", "keep"))
    out = []
    for s in range(len(bp) - 1):
        sc = (tri[tp[s]:tp[s + 1]], boxes[bp[s]:bp[s + 1]], keep[bp[s]:bp[s + 1]])
        out.append(sc if with_keep else sc[:2])
    return out


@pytest.fixture(scope="module")
def main_scenes(G):
    return _scenes(G, "")


def _lists(G, tag):
    off = np.concatenate([[0], np.cumsum(G["len_" + tag])])
    return {k: G["acc_" + tag][off[i]:off[i + 1]].tolist() for i, k in enumerate(KEYS)}


def _per_scene(scenes, vocab, changes, use_keep, **kw):
    from commonscenes_amd import constraints as CN
    acc = CN.new_accuracy()
    fn = CN.validate_constrains_changes if changes else CN.validate_constrains
    for t, b, k in scenes:
        assert fn(t, b, None, k if use_keep else None, vocab, acc, **kw) is acc
    return acc


def _check_many(scenes, vocab, want, mode, **kw):
    from commonscenes_amd import constraints as CN
    sc = scenes if mode else [s[:2] for s in scenes]
    res = CN.validate_constrains_many(sc, vocab, mode=mode, **kw)
    assert res["counts"].shape == (len(scenes), 11, 2)
    for i, k in enumerate(KEYS[:11]):
        assert res["summary"][k] == (sum(want[k]), len(want[k])), k
        assert (int(res["counts"][:, i, 0].sum()), int(res["counts"][:, i, 1].sum())) == res["summary"][k]
    assert res["total"] == (sum(want["total"]), len(want["total"]))


# mode 0 strict / non-strict, mode 1 (validate_constrains with keep), mode 2 (validate_constrains_changes)
CASES = {"m0s": (0, dict(strict=True)), "m0n": (0, dict(strict=False)), "m1": (1, {}), "m2": (2, {})}


@pytest.mark.parametrize("tag", list(CASES))
def test_twelve_lists_equal_the_reference_exactly(G, vocab, main_scenes, tag):
    mode, kw = CASES[tag]
    want = _lists(G, tag)
    got = _per_scene(main_scenes, vocab, changes=mode == 2, use_keep=mode != 0, **kw)
    for k in KEYS:
        assert got[k] == want[k], f"{tag}: list {k!r} differs"
    _check_many(main_scenes, vocab, want, mode, **kw)        # all 48 scenes in one launch: the sums of those lists


@pytest.mark.parametrize("tag,mode,kw", [("p7_m0", 0, {}), ("p7_m1", 1, {}), ("nn_m0", 0, dict(with_norm=False)),
                                         ("nn_m2", 2, dict(with_norm=False))])
def test_seven_parameter_and_unnormalised_sets(G, vocab, tag, mode, kw):
    scenes = _scenes(G, tag[:3])
    want = _lists(G, tag)
    got = _per_scene(scenes, vocab, changes=mode == 2, use_keep=mode != 0, **kw)
    for k in KEYS:
        assert got[k] == want[k], f"{tag}: list {k!r} differs"
    _check_many(scenes, vocab, want, mode, **kw)


def test_default_statistics_equal_a_statistics_file(G, vocab, main_scenes, tmp_path):
    """file_dist (np.loadtxt on the host, helpers/util.py:554-558) with the default numbers gives the default's verdicts"""
    from commonscenes_amd import constraints as CN
    np.savetxt(tmp_path / "dist.txt", np.stack([CN.DEFAULT_MEAN, CN.DEFAULT_STD]), fmt="%.17g")
    sc = [s[:2] for s in main_scenes[:6]]
    a = CN.evaluate(sc, vocab).verdict.cpu()
    b = CN.evaluate(sc, vocab, file_dist=str(tmp_path / "dist.txt")).verdict.cpu()
    assert torch.equal(a, b) and int((a >= 0).sum()) > 100


def test_batch_independence_and_empty_scenes(vocab, main_scenes):
    from commonscenes_amd import constraints as CN
    sc = [s[:2] for s in main_scenes]
    whole = CN.evaluate(sc, vocab)
    v, tp = whole.verdict.cpu().numpy(), whole.triple_ptr
    counts = whole.counts.cpu().numpy()
    assert int(whole.status.cpu()) == 0
    for i in (0, 23, 47):                                   # front, middle, end of the 48-scene launch
        alone = CN.evaluate([sc[i]], vocab)
        assert alone.verdict.cpu().numpy().tobytes() == v[tp[i]:tp[i + 1]].tobytes()
        assert np.array_equal(alone.counts.cpu().numpy()[0], counts[i])
    # empty scenes (0 triples) at the front, inside and at the end of a batch change nothing
    empty = (sc[0][0][:0], sc[0][1])
    mixed = CN.evaluate([empty, sc[1], empty, empty, sc[2], empty], vocab)
    mv, mc = mixed.verdict.cpu().numpy(), mixed.counts.cpu().numpy()
    assert mv.tobytes() == v[tp[1]:tp[3]].tobytes() and int(mixed.status.cpu()) == 0
    assert np.array_equal(mc[[1, 4]], counts[[1, 2]]) and not mc[[0, 2, 3, 5]].any()
    only = CN.evaluate([empty], vocab)                      # nothing to launch: counts are still reset
    assert only.verdict.numel() == 0 and not only.counts.cpu().numpy().any()
    acc = CN.new_accuracy()
    assert CN.validate_constrains(empty[0], empty[1], None, None, vocab, acc) is acc and acc == CN.new_accuracy()


def test_box3d_iou_pairs_against_the_reference(G):
    """|delta| <= 1e-9 on both outputs.  Derived, not measured: box3d_iou is fewer than 100 fp64 operations on magnitudes
    <= 1e2, which bounds the rounding error near 100 * 1e2 * 2^-53 ~ 2e-12; the gate leaves three orders for Qhull's different
    summation of the clipped polygon's area."""
    from commonscenes_amd import constraints as CN
    b1, b2 = torch.from_numpy(G["pair_box1"]).cuda(), torch.from_numpy(G["pair_box2"]).cuda()
    worst = 0.0
    for wt, key in ((True, "pair_iou_t"), (False, "pair_iou_0")):
        iou, iou2 = CN.box3d_iou(b1, b2, param6=True, with_translation=wt)
        assert iou.dtype == torch.float64 and iou.shape == (200,)
        d = np.abs(torch.stack([iou, iou2], 1).cpu().numpy() - G[key]).max()
        print(f"box3d_iou with_translation={wt}: max |delta| = {d:.3e}")
        worst = max(worst, d)
    assert worst <= 1e-9
    # seven columns, param6=False: the angle is ignored (metrics_3dfront.py:328 rotates by the identity)
    ang = torch.linspace(-180, 180, 200, device="cuda")[:, None]
    i7, j7 = CN.box3d_iou(torch.cat([b1, ang], 1), torch.cat([b2, -ang], 1), param6=False, with_translation=True)
    i6, j6 = CN.box3d_iou(b1, b2, with_translation=True)
    assert torch.equal(i7, i6) and torch.equal(j7, j6)


def test_box3d_iou_known_answers():
    """values measured with the reference (with_translation=True).  The boxes reach the device as fp32, so 0.2 and 0.3 are
    off by 3e-9 / 1.2e-8: the decimal answers hold to 1e-7, and the reference's own answers for the fp32 boxes to 1e-12."""
    from commonscenes_amd import constraints as CN
    a, b, c = (1, 1, 1, 0, 0, 0), (.5, .5, .5, .1, .2, .1), (1, 1, 1, 1, 0, 0)
    d, e = (-1, 1, 1, .2, 0, .2), (1, 1, 1, .3, 2, .3)
    pairs = [(a, b), (b, a), (a, c), (a, a), (a, d), (d, a), (a, e)]
    want = [(1.0, 0.25), (1.0, 0.25), (0.0, 0.0), (1.0, 1.0), (0.0, 0.0), (0.64, 8 / 17), (0.0, 0.3245033112582781)]
    want32 = {5: (0.6399999952316284, 0.47058823013800655), 6: (0.0, 0.32450329661918315)}
    x = torch.tensor([p[0] for p in pairs], dtype=torch.float32).cuda()
    y = torch.tensor([p[1] for p in pairs], dtype=torch.float32).cuda()
    iou, iou2 = (t.cpu().numpy() for t in CN.box3d_iou(x, y, with_translation=True))
    for k, (wi, w2) in enumerate(want):
        print(f"pair {k}: iou {iou[k]!r} iou_2d {iou2[k]!r}")
        assert abs(iou[k] - wi) <= 1e-7 and abs(iou2[k] - w2) <= 1e-7, (k, iou[k], iou2[k])
    for k in (2, 4):                                        # no overlap at all: exactly 0
        assert (iou[k], iou2[k]) == want[k]
    for k in (0, 1, 3):
        assert abs(iou[k] - want[k][0]) <= 1e-12 and abs(iou2[k] - want[k][1]) <= 1e-12
    for k, (wi, w2) in want32.items():
        assert abs(iou[k] - wi) <= 1e-12 and abs(iou2[k] - w2) <= 1e-12


def test_out_of_range_ids_are_reported_not_dereferenced(vocab, main_scenes):
    from commonscenes_amd import constraints as CN, lib
    sc = [s[:2] for s in main_scenes[:3]]
    good = CN.evaluate(sc, vocab)
    v0 = good.verdict.cpu().numpy().copy()
    tp, n1 = good.triple_ptr, sc[1][1].shape[0]
    tri = sc[1][0].clone()
    assert tri.shape[0] >= 6
    tri[0, 0] = n1                    # one past the scene's last object (it would read the NEXT scene's box)
    tri[1, 2] = -1
    tri[2, 1] = 12                    # one past the vocabulary
    tri[3, 1] = -5
    tri[4, 0] = 2 ** 40
    bad = CN.evaluate([sc[0], (tri, sc[1][1]), sc[2]], vocab)
    v1 = bad.verdict.cpu().numpy()
    assert int(bad.status.cpu()) == lib.STATUS_CONSTRAINT_RANGE
    hit = np.arange(tp[1], tp[1] + 5)
    assert (v1[hit] == -1).all()
    rest = np.setdiff1d(np.arange(len(v0)), hit)
    assert np.array_equal(v1[rest], v0[rest]) and int(good.status.cpu()) == 0
    want = good.counts.cpu().numpy().copy()
    got = bad.counts.cpu().numpy()
    assert np.array_equal(got[[0, 2]], want[[0, 2]]) and got[1].sum() <= want[1].sum()
    # the host API turns the status bit into an error
    with pytest.raises(lib.CsError, match="out of range"):
        CN.validate_constrains(tri, sc[1][1], None, None, vocab, CN.new_accuracy())
    with pytest.raises(lib.CsError, match="out of range"):
        CN.validate_constrains_many([sc[0], (tri, sc[1][1])], vocab)


def _walkthrough(args, timeout=600):
    env = dict(os.environ, CS_ONE_DEVICE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "eval_walkthrough.py"), *args], capture_output=True, text=True,
                       timeout=timeout, env=env, cwd=str(ROOT))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("EVAL_WALKTHROUGH ")]
    assert len(lines) == 1
    return json.loads(lines[0].split(" ", 1)[1])


def test_walkthrough_reports_the_accuracy_table():
    spec = importlib.util.spec_from_file_location("eval_walkthrough", ROOT / "tools" / "eval_walkthrough.py")
    W = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(W)
    assert [f"pred{i}\n" for i in range(16)] == W.VOCAB["pred_idx_to_name"]      # the model's vocabulary stays as it is
    # the triples the flag's mapping evaluates, counted from the synthetic graphs themselves
    cat = {"left": "left", "right": "right", "front": "front", "behind": "behind", "bigger than": "bigger",
           "smaller than": "smaller", "taller than": "taller", "shorter than": "shorter", "standing on": "standing on",
           "close by": "close by", "symmetrical to": "symmetrical to"}
    want = {k: 0 for k in KEYS}
    for data in W.synthetic_loader(2, seed=500):
        for p in data["decoder"]["tripltes"][:, 1].tolist():
            name = W.EVAL_PREDICATES[p]
            if name in cat:
                want[cat[name]] += 1
                want["total"] += 1
    assert want["total"] > 0
    d = _walkthrough(["--scenes", "2", "--width", "32", "--ddim-steps", "2", "--constraints"])
    acc = d["accuracy"]
    assert acc["mapped_triples"] == want["total"]
    for k in KEYS:
        assert acc[k]["evaluated"] == want[k] and 0 <= acc[k]["satisfied"] <= acc[k]["evaluated"], k
    assert sum(acc[k]["satisfied"] for k in KEYS[:11]) == acc["total"]["satisfied"]
    # without the flag the JSON line has the parent commit's keys
    plain = _walkthrough(["--scenes", "1", "--samples", "2", "--points", "500", "--width", "32", "--ddim-steps", "2"])
    parent = {"scenes", "world", "attention", "width", "ddim_steps", "mini_B", "total_s", "box_std_mean", "angle_std_mean",
              "chamfer_diversity_mean", "chamfer_diversity_n"}
    assert set(plain) == parent and set(d) == parent | {"accuracy"}
    assert set(plain["scenes"][0]) == set(d["scenes"][0]) == {"scan", "nodes", "shapes", "triples", "sample_s", "verts",
                                                               "finite", "angle_range"}
