"""commonscenes_amd.manipulation without a GPU: the graph edits against what the reference's dataset methods did
(tests/golden/manipulation.npz, dataset/threedfront_dataset.py:582-684), make_edit's bookkeeping against the collate's
(:705-723), and the meter's arithmetic against scripts/eval_3dfront.py:432-441 restated here."""
import copy

import numpy as np
import pytest
import torch

from conftest import GOLDEN


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN / "manipulation.npz")


def _names(gold):
    classes = {str(n): i for i, n in enumerate(gold["classes"].tolist())}
    return classes, {i: n for n, i in classes.items()}, [str(r) for r in gold["relationships"].tolist()]


def _graph(gold, gi):
    from commonscenes_amd.manipulation import graph_lists
    classes, classes_r, rels = _names(gold)
    O, T = (int(v) for v in gold["in_n"][gi])
    objs, tri = gold["in_objs"][gi, :O].tolist(), gold["in_triples"][gi, :T].tolist()
    g = graph_lists(objs, tri, [[float(i)] * 7 for i in range(O)], np.arange(O, dtype=np.float32).reshape(O, 1),
                    np.arange(T, dtype=np.float32).reshape(T, 1), classes_r, rels, scan_id=f"g{gi}")
    return g, classes, rels


def _valid(row):
    return row[row >= 0] if row.ndim == 1 else row[(row >= 0).all(axis=-1)]


# 1 ------------------------------------------------------------------------------------------------------------------
def test_remove_node_and_relationship_reproduces_the_reference(gold):
    from commonscenes_amd.manipulation import remove_node_and_relationship
    G, S = gold["rm_node"].shape
    for gi in range(G):
        base, classes, _ = _graph(gold, gi)
        tagged = [f"{i}|{w}" for i, w in enumerate(base["words"])]
        for k in range(S):
            g = copy.deepcopy(base)
            g["words"] = list(tagged)
            np.random.seed(k)
            node = remove_node_and_relationship(g, classes)
            assert node == int(gold["rm_node"][gi, k]), (gi, k)
            assert g["objs"] == _valid(gold["rm_objs"][gi, k]).tolist()
            rows = _valid(gold["rm_obj_rows"][gi, k]).tolist()
            assert [int(b[0]) for b in g["boxes"]] == rows and [int(f[0]) for f in g["text_feats"]] == rows
            assert g["triples"] == _valid(gold["rm_triples"][gi, k]).tolist()
            assert [int(f[0]) for f in g["rel_feats"]] == _valid(gold["rm_tri_rows"][gi, k]).tolist()
            assert [int(w.split("|")[0]) for w in g["words"]] == _valid(gold["rm_word_rows"][gi, k]).tolist()
            if node < 0:                                             # gave up: the graph is as it was
                assert g["objs"] == base["objs"] and g["triples"] == base["triples"]
    assert (gold["rm_node"][6] == -1).all()                           # the all-floor graph is in the fixture


@pytest.mark.parametrize("interpretable", [False, True])
def test_modify_relship_reproduces_the_reference(gold, interpretable):
    from commonscenes_amd.manipulation import modify_relship
    tag = "mod1" if interpretable else "mod0"
    G, S = gold[f"{tag}_idx"].shape
    for gi in range(G):
        base, classes, rels = _graph(gold, gi)
        T = len(base["triples"])
        for k in range(S):
            g = copy.deepcopy(base)
            np.random.seed(k)
            idx, pair, did = modify_relship(g, classes, rels, interpretable=interpretable)
            assert (int(idx), tuple(int(p) for p in pair), bool(did)) == \
                (int(gold[f"{tag}_idx"][gi, k]), tuple(gold[f"{tag}_pair"][gi, k].tolist()), bool(gold[f"{tag}_did"][gi, k]))
            assert g["triples"] == gold[f"{tag}_triples"][gi, k, :T].tolist()
            assert g["triples"][idx][1] == int(gold[f"{tag}_new_pred"][gi, k])
            assert "\n".join(g["words"]) == str(gold[f"{tag}_words"][gi, k])
            assert (g.get("changed_id") == idx) if did else ("changed_id" not in g)
            # nothing but the predicate and the words entry moves
            assert g["objs"] == base["objs"] and g["boxes"] == base["boxes"]
            assert all(np.array_equal(a, b) for a, b in zip(g["rel_feats"], base["rel_feats"]))
    assert not gold[f"{tag}_did"][7].any() and gold[f"{tag}_did"][:6].any()      # the graph with nothing to edit


# 2 ------------------------------------------------------------------------------------------------------------------
def test_make_edit_bookkeeping(gold):
    from commonscenes_amd.manipulation import make_edit
    G, S = gold["rm_node"].shape
    for gi in range(G):
        base, classes, rels = _graph(gold, gi)
        base["sdfs"] = torch.zeros(len(base["objs"]), 1, 2, 2, 2)
        keep_objs, keep_tri = list(base["objs"]), copy.deepcopy(base["triples"])
        for k in range(S):
            np.random.seed(k)
            add = make_edit(base, "addition", classes, rels)
            node = int(gold["rm_node"][gi, k])
            if node < 0:
                assert add is None
            else:
                assert add["missing_nodes"] == [node] and add["missing_nodes_decoder"] == [node]
                assert add["manipulated_nodes"] == [] and add["manipulate"] == {"type": "addition", "added": node}
                assert add["encoder"]["objs"].shape[0] == add["decoder"]["objs"].shape[0] - 1
                assert add["encoder"]["objs"].tolist() == _valid(gold["rm_objs"][gi, k]).tolist()
                assert add["encoder"]["tripltes"].tolist() == _valid(gold["rm_triples"][gi, k]).tolist()
                assert add["decoder"]["objs"].tolist() == keep_objs and add["decoder"]["tripltes"].tolist() == keep_tri
                assert add["encoder"]["text_feats"].shape == (len(keep_objs) - 1, 1)
                assert add["encoder"]["rel_feats"].shape[0] == add["encoder"]["tripltes"].shape[0]
                assert add["encoder"]["objs"].dtype == torch.int64 and add["encoder"]["boxes"].dtype == torch.float32
                assert add["decoder"]["sdfs"] is base["sdfs"] and "tripltes" in add["encoder"]
            np.random.seed(k)
            rel = make_edit(base, "relationship", classes, rels, rel_feat_fn=lambda words: np.full(1, -7.0, np.float32))
            if not bool(gold["mod1_did"][gi, k]):
                assert rel is None
            else:
                sub, obj = gold["mod1_pair"][gi, k].tolist()
                idx = int(gold["mod1_idx"][gi, k])
                assert rel["manipulated_nodes"] == [sub, obj] and rel["missing_nodes"] == []
                assert rel["manipulate"]["relship"] == (idx, (sub, obj))
                enc_t, dec_t = rel["encoder"]["tripltes"], rel["decoder"]["tripltes"]
                differ = (enc_t != dec_t).any(dim=1).nonzero().reshape(-1).tolist()
                assert differ == [idx] and bool((enc_t[idx, [0, 2]] == dec_t[idx, [0, 2]]).all())
                assert int(dec_t[idx, 1]) == int(gold["mod1_new_pred"][gi, k])
                assert enc_t.tolist() == keep_tri and rel["decoder"]["changed_id"] == idx
                assert float(rel["decoder"]["rel_feats"][idx, 0]) == -7.0            # the edited words were re-encoded
                assert float(rel["encoder"]["rel_feats"][idx, 0]) == float(idx)
            # the caller's scene is never touched
            assert base["objs"] == keep_objs and base["triples"] == keep_tri
    with pytest.raises(ValueError):
        make_edit(_graph(gold, 0)[0], "removal", *_names(gold)[::2])


# 3 ------------------------------------------------------------------------------------------------------------------
def _lists(gold, tag):
    keys = [str(k) for k in gold["keys"].tolist()]
    flat, lens = gold[f"acc_{tag}"], gold[f"len_{tag}"]
    at, out = 0, {}
    for k, n in zip(keys, lens.tolist()):
        out[k] = flat[at:at + n].tolist()
        at += n
    return out


def _reference_rows(dic):
    """scripts/eval_3dfront.py:432-441 on the reference's key order (:214)"""
    order = ["left", "right", "front", "behind", "smaller", "bigger", "shorter", "taller", "standing on", "close by",
             "symmetrical to", "total"]
    m = [np.mean(dic[k]) if len(dic[k]) else float("nan") for k in order]
    row = [np.mean([m[0], m[1]]), np.mean([m[2], m[3]]), np.mean([m[4], m[5]]), np.mean([m[6], m[7]]), m[8], m[9], m[10]]
    return row + [m[11], np.mean(row)]


def test_meter_arithmetic(gold):
    from commonscenes_amd import manipulation as MP
    names = ("L/R", "F/B", "Bi/Sm", "Ta/Sh", "Stand", "Close", "Symm", "Total", "means of mean")
    for tag in ("changed", "unchanged", "orig"):
        dic = _lists(gold, tag)
        row = MP.table_rows({k: (int(sum(v)), len(v)) for k, v in dic.items()})
        want = _reference_rows(dic)
        assert [row[n] for n in names] == pytest.approx(want, rel=1e-12, abs=0)
        text = MP.format_row("changed nodes", row)
        assert text.startswith("changed nodes & L/R: {:.2f} & F/B: {:.2f}".format(want[0], want[1]))
        assert text.endswith("means of mean: {:.2f}".format(want[8]))
    # a category nobody evaluated: None where the reference prints nan, and it spreads as nan does
    dic = dict(_lists(gold, "changed"), **{"standing on": []})
    row = MP.table_rows({k: (int(sum(v)), len(v)) for k, v in dic.items()})
    assert row["Stand"] is None and row["means of mean"] is None and row["L/R"] is not None
    # the diversity block: None, not NaN, when nothing was accumulated
    empty = MP.diversity_block([], [], [])
    assert empty == {"shape": None, "box_size": None, "box_location": None, "angle": None, "shapes": 0, "boxes": 0,
                     "angles": 0}
    blk = MP.diversity_block([0.5, 1.5], [np.arange(6.0), np.arange(6.0) + 2], [10.0])
    assert blk["shape"] == 1.0 and blk["box_size"] == 2.0 and blk["box_location"] == 5.0 and blk["angle"] == 10.0
    m = MP.ManipulationMeter({"pred_idx_to_name": ["in\n"]}, {"floor": 1})
    s = m.summary()                                                  # nothing queued: no device needed
    assert s["scenes"] == 0 and s["diversity"]["shape"] is None and s["tables"]["changed nodes"]["Total"] is None
