"""Scene-graph constraint accuracy (commonscenes_amd/constraints.py, csrc/cs_constraints.hip), the part that needs no GPU:
the ABI, the predicate mapping, the argument checks and the fixture's own conditions."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ("cs_scene_constraints", "cs_box3d_iou_pairs")
KEYS = ["left", "right", "front", "behind", "bigger", "smaller", "taller", "shorter", "standing on", "close by",
        "symmetrical to", "total"]


def _vocab(names):
    return {"pred_idx_to_name": list(names)}


def test_entries_are_declared_exported_and_bound():
    from commonscenes_amd import build, lib
    txt = (ROOT / "include" / "commonscenes_hip.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    dll = lib.load()
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), f"{name} is not declared with a status return"
        assert hasattr(dll, name) and name in lib.SIGNATURES
        assert lib.SIGNATURES[name][0] is lib.C.c_int
    assert "cs_constraints.hip" in build.SOURCES and (build.CSRC / "cs_constraints.hip").exists()
    assert dll.cs_abi_version() == lib.ABI_VERSION == 18
    # the comments cite the reference's lines, as the scene entries' do
    assert "metrics_3dfront.py:57-179" in txt and "metrics_3dfront.py" in txt and ":337-370" in txt
    assert re.search(r"#define\s+CS_STATUS_CONSTRAINT_RANGE\s+8\b", txt) and lib.STATUS_CONSTRAINT_RANGE == 8


def test_entries_reject_null_and_malformed_arguments_before_the_device():
    import ctypes as C
    from commonscenes_amd import lib
    dll = lib.load()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)

    def constraints(**kw):
        a = dict(boxes=p, n_boxes=4, ld=6, params=6, triples=p, n_triples=2, box_ptr=p, triple_ptr=p, n_scenes=1, pred_code=p,
                 n_preds=3, keep=p, mode=0, norm=p, scale=3.0, strict=1, thr=0.3, verdict=p, counts=p, status=p, stream=None)
        a.update(kw)
        return dll.cs_scene_constraints(*a.values())

    for bad in (dict(boxes=None), dict(triples=None), dict(box_ptr=None), dict(triple_ptr=None), dict(pred_code=None),
                dict(verdict=None), dict(counts=None), dict(n_boxes=0), dict(n_triples=-1), dict(n_scenes=0), dict(n_preds=0),
                dict(params=5), dict(params=8), dict(ld=5), dict(params=7, ld=6), dict(mode=3), dict(mode=-1),
                dict(mode=1, keep=None), dict(mode=2, keep=None), dict(mode=2, params=7, ld=7), dict(scale=0.0)):
        assert constraints(**bad) == lib.CS_EINVAL, bad
    for bad in ((None, p, 4, 6, 6), (p, None, 4, 6, 6), (p, p, 0, 6, 6), (p, p, 4, 5, 6), (p, p, 4, 6, 5), (p, p, 4, 8, 8)):
        assert dll.cs_box3d_iou_pairs(*bad, 1, p, p, None) == lib.CS_EINVAL, bad
    assert dll.cs_box3d_iou_pairs(p, p, 4, 6, 6, 1, None, p, None) == lib.CS_EINVAL
    assert dll.cs_box3d_iou_pairs(p, p, 4, 6, 6, 1, p, None, None) == lib.CS_EINVAL


def test_predicate_names_map_like_the_reference_slice():
    """metrics_3dfront.py:74 compares `vocab["pred_idx_to_name"][p][:-1]`: the LAST character goes, whatever it is."""
    from commonscenes_amd import constraints as CN
    names = ["left", "right", "front", "behind", "bigger than", "smaller than", "taller than", "shorter than", "standing on",
             "close by", "symmetrical to"]
    assert CN.predicate_codes(_vocab(n + "\n" for n in names)) == list(range(11))
    # without the trailing newline the slice eats the last letter: nothing matches, exactly as in the reference
    assert CN.predicate_codes(_vocab(names)) == [-1] * 11
    assert CN.predicate_codes(_vocab(["leftX", "left", "lef\n", "left\n\n", "Left\n", "none\n", "in\n", "bigger\n", "\n", ""])) == \
        [0, -1, -1, -1, -1, -1, -1, -1, -1, -1]
    assert CN.predicate_codes(_vocab(["close by\n", "pred3\n", "standing on\n", "bigger than\n"])) == [9, -1, 8, 4]
    assert list(CN.CATEGORIES) == KEYS[:11] and list(CN.KEYS) == KEYS


def test_new_accuracy_has_the_scripts_twelve_keys():
    from commonscenes_amd import constraints as CN
    acc = CN.new_accuracy()
    assert list(acc) == KEYS and all(v == [] for v in acc.values())
    acc["left"].append(1)
    assert CN.new_accuracy()["left"] == []                 # fresh lists every time


def test_argument_errors_raise_before_any_device_work():
    from commonscenes_amd import constraints as CN, lib
    vocab = _vocab(["none\n", "left\n", "close by\n"])
    tri = torch.tensor([[0, 1, 1], [1, 2, 0]])
    box6, box7, keep = torch.zeros(3, 6), torch.zeros(3, 7), torch.ones(3)
    acc = CN.new_accuracy()

    def raises(match, fn, *a, **k):
        with pytest.raises(lib.CsError, match=match):
            fn(*a, **k)

    # CPU tensors: no fallback
    raises("no CPU fallback", CN.validate_constrains, tri, box6, None, None, vocab, acc)
    raises("no CPU fallback", CN.validate_constrains, tri, box7, None, keep, vocab, acc)
    raises("no CPU fallback", CN.validate_constrains_changes, tri, box6, None, keep, vocab, acc)
    raises("no CPU fallback", CN.validate_constrains_many, [(tri, box6), (tri, box6, keep)], vocab)
    raises("no CPU fallback", CN.box3d_iou, box6, box6)
    # box width
    for bad in (torch.zeros(3, 5), torch.zeros(3, 8), torch.zeros(6), torch.zeros(0, 6)):
        raises("boxes", CN.validate_constrains, tri, bad, None, None, vocab, acc)
    raises(r"\[M, 6\]", CN.box3d_iou, box7, box7)
    raises(r"\[M, 7\]", CN.box3d_iou, box6, box6, param6=False)
    raises("pair up", CN.box3d_iou, box6, torch.zeros(2, 6))
    # mode 2 with seven parameters, with and without a keep mask
    raises("6-parameter", CN.validate_constrains_changes, tri, box7, None, keep, vocab, acc)
    raises("6-parameter", CN.validate_constrains_changes, tri, box7, None, None, vocab, acc)
    raises("6-parameter", CN.validate_constrains_many, [(tri, box7, keep)], vocab, mode=2)
    # ids out of range
    for bad in ([[0, 1, 3]], [[3, 1, 0]], [[-1, 1, 0]], [[0, 3, 1]], [[0, -1, 1]]):
        raises("out of range", CN.validate_constrains, torch.tensor(bad), box6, None, None, vocab, acc)
    raises("out of range", CN.validate_constrains_many, [(tri, box6), (torch.tensor([[0, 1, 3]]), box6)], vocab)
    # keep length, triples shape, scene lists
    raises("keep has 2 entries", CN.validate_constrains, tri, box6, None, torch.ones(2), vocab, acc)
    raises("triples", CN.validate_constrains, torch.zeros(2, 2, dtype=torch.int64), box6, None, None, vocab, acc)
    raises("triples", CN.validate_constrains, torch.zeros(2, 3), box6, None, None, vocab, acc)
    raises("keep mask", CN.validate_constrains_many, [(tri, box6)], vocab, mode=1)
    raises("same box width", CN.validate_constrains_many, [(tri, box6), (tri, box7)], vocab)
    raises("no scenes", CN.validate_constrains_many, [], vocab)
    raises("mode", CN.validate_constrains_many, [(tri, box6)], vocab, mode=3)
    assert all(v == [] for v in acc.values())              # nothing was appended on the way


def test_file_dist_is_read_on_the_host(tmp_path):
    from commonscenes_amd import constraints as CN, lib
    stats = np.stack([np.arange(1, 8) * 0.5, np.arange(1, 8) * 0.25])
    np.savetxt(tmp_path / "dist.txt", stats)
    assert np.array_equal(CN._norm_rows(str(tmp_path / "dist.txt"), 7), stats)
    assert np.array_equal(CN._norm_rows(str(tmp_path / "dist.txt"), 6)[:, :6], stats[:, :6])
    d = CN._norm_rows(None, 6)
    assert d[0, 0] == 1.3827214 and d[1, 5] == 0.70099753 and d.dtype == np.float64
    np.savetxt(tmp_path / "short.txt", stats[:, :5])
    with pytest.raises(lib.CsError):
        CN._norm_rows(str(tmp_path / "short.txt"), 6)


def test_fixture_holds_its_conditions():
    """tests/golden/constraints.npz (tools/make_goldens.py g_constraints): the reference's verdicts are those of triples that
    sit away from every threshold, every category has both verdicts, `strict` matters, and the lists are consistent."""
    g = np.load(ROOT / "tests" / "golden" / "constraints.npz")
    assert list(g["keys"]) == KEYS and list(g["pred_names"][1:]) == ["left", "right", "front", "behind", "bigger than",
                                                                      "smaller than", "taller than", "shorter than",
                                                                      "standing on", "close by", "symmetrical to"]
    assert int(g["cond_min_per_verdict"]) >= 20 and int(g["cond_strict_flips"]) >= 20
    assert float(g["cond_dropped_fraction"]) <= 0.02 and float(g["cond_noise"]) == 1e-5 and int(g["cond_noise_draws"]) == 2
    assert len(g["box_ptr"]) == 49 and g["boxes"].shape[1] == 6 and g["boxes"].dtype == np.float32
    assert g["p7_boxes"].shape[1] == 7 and g["nn_boxes"].shape[1] == 6
    for tag in ("", "p7_", "nn_"):
        bp, tp, tri = g[tag + "box_ptr"], g[tag + "triple_ptr"], g[tag + "triples"]
        assert bp[0] == 0 and bp[-1] == len(g[tag + "boxes"]) == len(g[tag + "keep"]) and tp[0] == 0 and tp[-1] == len(tri)
        for s in range(len(bp) - 1):
            t = tri[tp[s]:tp[s + 1]]
            assert t[:, [0, 2]].min() >= 0 and t[:, [0, 2]].max() < bp[s + 1] - bp[s] and t[:, 1].min() >= 0 and t[:, 1].max() < 12
    # the stored conditions restated from the stored lists
    lens = g["len_m0s"]
    off = np.concatenate([[0], np.cumsum(lens)])
    assert lens[:11].sum() == lens[11] == int((g["triples"][:, 1] != 0).sum()) and list(g["len_m0n"]) == list(lens)
    for k in range(11):
        part = g["acc_m0s"][off[k]:off[k + 1]]
        assert min(int((part == 0).sum()), int((part == 1).sum())) >= 20, KEYS[k]
    tot_s, tot_n = g["acc_m0s"][off[11]:], g["acc_m0n"][off[11]:]
    assert int((tot_s != tot_n).sum()) == int(g["cond_strict_flips"]) and np.all(tot_s <= tot_n)
    assert 0 < g["len_m1"][11] < lens[11] and 0 < g["len_m2"][11] < lens[11] and g["len_m1"][11] + g["len_m2"][11] == lens[11]
    # 200 box pairs in metres, no tiny denominator, a good share of them overlapping
    assert g["pair_box1"].shape == g["pair_box2"].shape == (200, 6) and g["pair_iou_t"].shape == (200, 2)
    assert min(g["pair_box1"][:, :3].min(), g["pair_box2"][:, :3].min()) >= 0.05
    assert np.isfinite(g["pair_iou_t"]).all() and np.isfinite(g["pair_iou_0"]).all() and int((g["pair_iou_t"][:, 0] > 0).sum()) >= 50
    assert (ROOT / "tests" / "golden" / "constraints.npz").stat().st_size < 200 * 1024
