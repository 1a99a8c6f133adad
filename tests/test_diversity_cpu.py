"""commonscenes_amd/diversity.py without a device: the host half of the diversity and consistency tables against what the
reference's own functions gave on the CPU (tests/golden/diversity.npz, tools/make_goldens.py --only diversity), the order of
the random draws, the meter's arithmetic on injected numbers, and every argument error, which must come before any launch.
Every figure is printed before it is asserted."""
from pathlib import Path

import numpy as np
import pytest
import torch

GOLD = Path(__file__).resolve().parent / "golden" / "diversity.npz"
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def test_entries_are_declared_exported_and_reject_bad_arguments():
    from commonscenes_amd import build, lib
    dll = lib.load()
    txt = (ROOT / "include" / "commonscenes_hip.h").read_text()
    for name in ("cs_cloud_resample", "cs_chamfer_pairlist"):
        assert name in lib.SIGNATURES and hasattr(dll, name) and f"int {name}(" in txt
    assert "cs_diversity.hip" in build.SOURCES and dll.cs_abi_version() == 18
    one = 1                                        # any non-NULL address: the checks below all fail before a launch
    assert dll.cs_cloud_resample(one, one, one, None, one, -1, 4, 0, one, None) == lib.CS_EINVAL
    assert dll.cs_cloud_resample(one, one, one, None, one, 2, 0, 0, one, None) == lib.CS_EINVAL
    assert dll.cs_cloud_resample(one, one, one, None, one, 2, 4, 0, None, None) == lib.CS_EINVAL
    assert dll.cs_cloud_resample(None, one, one, None, one, 2, 4, 0, one, None) == lib.CS_EINVAL
    assert dll.cs_cloud_resample(one, one, one, None, one, 0, 4, 1, one, None) == lib.CS_OK          # no cloud: no launch
    assert dll.cs_chamfer_pairlist(one, one, one, 0, 8, 1, one, None) == lib.CS_EINVAL
    assert dll.cs_chamfer_pairlist(one, one, one, 2, 32769, 1, one, None) == lib.CS_EINVAL
    assert dll.cs_chamfer_pairlist(one, one, one, 2, 8, 0, one, None) == lib.CS_EINVAL
    assert dll.cs_chamfer_pairlist(one, None, one, 2, 8, 1, one, None) == lib.CS_EINVAL
    assert dll.cs_chamfer_pairlist(one, one, one, 2, 8, 1, None, None) == lib.CS_EINVAL


def test_draw_indices_makes_the_references_calls_in_the_references_order():
    """helpers/util.py:31-44 restated: per cloud, in list order, randperm(n)[:num] or randint(n, (num,)) from the global
    generator.  A check of call order under one seed, so it holds on any torch build."""
    from commonscenes_amd import diversity as D
    counts = [1, 3, 17, 64, 65, 257, 3000, 5, 64]
    for num in (64, 257):
        torch.manual_seed(47)
        want = [torch.randperm(n)[:num] if n >= num else torch.randint(n, size=(num,)) for n in counts]
        after = torch.rand(1)
        torch.manual_seed(47)
        got = D.draw_indices(counts, num)
        assert torch.equal(torch.rand(1), after)                 # the generator was advanced by exactly those draws
        assert got.shape == (len(counts), num) and got.dtype == torch.int64
        for w, g in zip(want, got):
            assert torch.equal(w, g)
        # an explicit generator leaves the global one alone and gives the same rows for the same seed
        torch.manual_seed(5)
        mark = torch.rand(1)
        torch.manual_seed(5)
        got2 = D.draw_indices(counts, num, generator=torch.Generator().manual_seed(47))
        assert torch.equal(torch.rand(1), mark) and torch.equal(got2, got)


def test_angular_std_matches_the_reference(gold):
    from commonscenes_amd import diversity as D
    for K in (2, 3, 5):
        got, want = D.angular_std(gold[f"angles_{K}"]), gold[f"angular_std_{K}"]
        plain = gold[f"angles_{K}"].std(axis=1)
        print(f"angular_std K={K}: worst |diff| {np.abs(got - want).max():.3e} deg; plain std differs by up to "
              f"{np.abs(plain - want).max():.1f} deg")
        assert got.dtype == np.float64 and got.shape == (6,)
        assert np.abs(got - want).max() <= 1e-9
        assert D.estimate_angular_std(list(gold[f"angles_{K}"][1])) == got[1]
        assert np.abs(plain - want).max() > 1.0                  # the sets straddling 0 / 360 tell the two apart
    with pytest.raises(ValueError):
        D.angular_std(np.zeros((3,)))


def test_box_std_matches_the_reference(gold, tmp_path):
    """tolerance per entry: 1e-6 * max |denormalised value of that column|.  (The reference multiplies the float32 boxes by
    float64 statistics, so its figure is a float64 one too; the fixture says so.  The bound stays as set.)"""
    from commonscenes_amd import diversity as D
    f = tmp_path / "stats.txt"
    np.savetxt(f, gold["box_stats"])
    boxes = torch.from_numpy(gold["boxes"])
    for tag, file in (("none", None), ("file", str(f))):
        got, want = D.box_std(boxes, file=file), gold[f"box_std_{tag}"].astype(np.float64)
        tol = 1e-6 * gold[f"box_den_absmax_{tag}"][None, :]
        ratio = float((np.abs(got - want) / tol).max())
        print(f"box_std ({tag}): worst |diff| / tolerance = {ratio:.3e}")
        assert got.shape == (6, 6) and got.dtype == np.float64 and ratio <= 1.0
    normalised = boxes.double().std(dim=1).numpy()
    assert np.abs(normalised - gold["box_std_none"]).max() > 1e-2            # the std of normalised boxes is another figure
    with pytest.raises(ValueError):
        D.box_std(boxes[:, :1])
    with pytest.raises(ValueError):
        D.box_std(torch.zeros(4, 3, 5))


CLASSES = {"_scene_": 0, "bed": 1, "chair": 2, "lamp": 3, "floor": 4, "sofa": 5, "plant": 6}


def test_meter_arithmetic_on_injected_numbers():
    from commonscenes_amd import diversity as D
    m = D.DiversityMeter(CLASSES)
    assert m.categories == ("bed", "nightstand", "wardrobe", "chair", "table", "cabinet", "lamp", "sofa", "shelf", "tv_stand")
    s0 = m.summary()
    assert s0["objects"] == 0 and s0["shape"] is None and s0["box_size"] is None and s0["angle"] is None
    # scene 1: bed, chair, chair, plant (no category of its own), floor, _scene_
    objs1 = torch.tensor([1, 2, 2, 6, 4, 0])
    assert m.kept_nodes(objs1) == [0, 1, 2, 3]
    box1 = np.arange(36, dtype=np.float64).reshape(6, 6)
    m.add_numbers(objs1, [0.1, 0.2, 0.4, 0.8], box1, [1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    # scene 2: a skipped node in the MIDDLE -- the category follows the node's own index
    objs2 = [3, 4, 1]
    assert m.kept_nodes(objs2) == [0, 2]
    box2 = np.ones((3, 6)) * np.array([1, 1, 1, 7, 7, 7.0])
    m.add_numbers(objs2, [1.6, 3.2], box2, [10.0, 20.0, 30.0])
    s = m.summary()
    print(s)
    assert s["objects"] == 6 and s["shape"] == pytest.approx(np.mean([0.1, 0.2, 0.4, 0.8, 1.6, 3.2]), abs=1e-15)
    cats = s["categories"]
    assert cats["bed"] == {"n": 2, "shape": pytest.approx((0.1 + 3.2) / 2, abs=1e-15)}
    assert cats["chair"] == {"n": 2, "shape": pytest.approx(0.3, abs=1e-15)}
    assert cats["lamp"] == {"n": 1, "shape": 1.6}
    assert cats["sofa"] == {"n": 0, "shape": None} and cats["tv_stand"] == {"n": 0, "shape": None}   # empty: no warning
    assert set(cats) == set(m.categories)
    rows = np.concatenate([box1, box2])
    assert s["box_size"] == pytest.approx(rows.mean(axis=0)[:3].mean(), abs=1e-12)
    assert s["box_location"] == pytest.approx(rows.mean(axis=0)[3:].mean(), abs=1e-12)
    assert s["box_size"] != s["box_location"]
    assert s["angle"] == pytest.approx(np.mean([1, 2, 3, 4, 5, 6, 10, 20, 30]), abs=1e-12)
    with pytest.raises(ValueError):
        m.add_numbers(objs2, [1.0, 2.0, 3.0])                    # three figures for two shaped nodes
    with pytest.raises(ValueError):
        m.add_numbers(objs2, None, np.zeros((3, 5)))


def test_meter_angles_and_boxes_from_runs(gold):
    """add_scene without shapes touches no device: argmax / 24 * 360 of the score tensors, then the circular deviation; boxes
    denormalised, then the unbiased deviation over the runs."""
    from commonscenes_amd import diversity as D
    m = D.DiversityMeter(CLASSES)
    degs = gold["angles_3"]                                        # [6, 3] on the 15-degree grid
    scores = []
    for k in range(3):
        s = torch.zeros(6, 24)
        s[torch.arange(6), torch.from_numpy((degs[:, k] / 15.0).astype(np.int64))] = 1.0
        scores.append(s)
    boxes = torch.from_numpy(gold["boxes"])
    res = m.add_scene([1, 2, 2, 3, 4, 0], [boxes[:, k] for k in range(3)], scores, None)
    assert np.abs(res["angle_std"] - gold["angular_std_3"]).max() <= 1e-9
    assert np.array_equal(res["box_std"], D.box_std(boxes)) and res["shape"] is None and res["nodes"] == [0, 1, 2, 3]
    s = m.summary()
    assert s["objects"] == 0 and s["angle"] == pytest.approx(gold["angular_std_3"].mean(), abs=1e-9)
    with pytest.raises(ValueError):
        m.add_scene([1, 2], None, [torch.zeros(2, 24)], None)    # one run


def test_consistency_grouping():
    from commonscenes_amd.diversity import _group
    t = _group(np.array([1.0, 2.0, 4.0, 8.0, 16.0]), ["chair", "bed", "chair", "lamp", "chair"])
    print(t)
    assert list(t) == ["chair", "bed", "lamp", "total"]
    assert t["chair"] == {"pairs": 3, "chamfer": 7.0} and t["bed"] == {"pairs": 1, "chamfer": 2.0}
    assert t["lamp"] == {"pairs": 1, "chamfer": 8.0} and t["total"] == {"pairs": 5, "chamfer": 31.0 / 5}
    assert _group(np.zeros((0,)), []) == {"total": {"pairs": 0, "chamfer": None}}


def test_obj_vertex_reader(tmp_path):
    from commonscenes_amd.diversity import read_obj_vertices
    f = tmp_path / "chair_2_7.obj"
    f.write_text("# a comment\nmtllib x.mtl\nv 0 0.5 -1\nvn 0 0 1\nv 1e-3 2 3 0.5 0.5 0.5\n\nvt 0 0\nv  -4.25\t5 6\nf 1 2 3\n"
                 "v 0 0.5 -1\n")
    v = read_obj_vertices(f)
    assert v.dtype == torch.float32 and v.shape == (4, 3)
    assert torch.equal(v, torch.tensor([[0, 0.5, -1], [1e-3, 2, 3], [-4.25, 5, 6], [0, 0.5, -1]]))    # duplicates stay
    (tmp_path / "empty.obj").write_text("f 1 2 3\n")
    assert read_obj_vertices(tmp_path / "empty.obj").shape == (0, 3)


def test_argument_errors_come_before_any_launch():
    """all on CPU tensors, on a machine without a device: whatever is wrong with shapes and values is reported first."""
    from commonscenes_amd import diversity as D, lib, ops
    c = lambda n: torch.zeros(n, 3)
    with pytest.raises(ValueError, match="cloud 1 is empty"):
        D.sample_points([c(4), c(0), c(2)], 8)
    with pytest.raises(ValueError, match="cloud 2 is empty"):
        D.sample_and_normalize([c(4), c(1), c(0)], 8)
    with pytest.raises(ValueError, match="cloud 0 is empty"):
        D.sample_points_packed(c(4), [0, 4], 8)
    with pytest.raises(ValueError, match="cloud 1"):
        D.consistency_from_meshes([c(4), c(0)], [[0, 1]], ["chair"])
    with pytest.raises(ValueError):
        D.sample_points([torch.zeros(4, 2)], 8)
    with pytest.raises(ValueError):
        D.sample_points([c(4)], 0)
    with pytest.raises(ValueError):
        D.sample_points([c(4), c(5)], 8, indices=torch.zeros(3, 8, dtype=torch.int64))
    for bad in (torch.zeros(3, 1, 16, 3), torch.zeros(3, 0, 16, 3)):
        with pytest.raises(ValueError, match="two runs"):
            D.shape_diversity(bad)                               # K < 2
    with pytest.raises(ValueError):
        D.shape_diversity(torch.zeros(3, 2, 16))
    with pytest.raises(ValueError):
        D.normalize(torch.zeros(4, 2))
    with pytest.raises(ValueError):
        D.normalize(torch.zeros(0, 3))
    with pytest.raises(ValueError):
        D.consistency_table(torch.zeros(3, 8, 3), [[0, 1], [1, 2]], ["chair"])
    with pytest.raises(ValueError):
        D.consistency_from_meshes([c(4), c(3)], [[0, 2]], ["chair"])
    m = D.DiversityMeter(CLASSES)
    with pytest.raises(ValueError):
        m.add_scene([1, 2, 0], None, None, torch.zeros(3, 2, 8, 3))          # two shaped nodes, three rows
    with pytest.raises(ValueError, match="two runs"):
        m.add_scene([1, 2, 0], None, None, torch.zeros(2, 1, 8, 3))
    with pytest.raises(ValueError, match="two runs"):
        m.add_scene([1, 2, 0], None, None, [[c(4), c(4)]])
    with pytest.raises(ValueError):
        D.scene_diversity(None, {}, num_samples=1)
    # the wrappers: indices and pairs that live on the host are range-checked here
    v = torch.zeros(10, 3)
    for kw in (dict(idx=[[0, 4], [1, 5]]), dict(idx=[[0, -1], [1, 2]]), dict(idx=torch.tensor([[0, 1]])),
               dict(idx=torch.tensor([[0.0, 1.0], [1.0, 2.0]]))):
        with pytest.raises(lib.CsError):
            ops.cloud_resample(v, [0, 4], [4, 5], 2, **kw)
    for first, count in (([0, 4], [4, 7]), ([0, 4], [4, 0]), ([-1, 4], [4, 5]), ([0], [4, 5])):
        with pytest.raises(lib.CsError):
            ops.cloud_resample(v, first, count, 2, idx=[[0, 1], [0, 1]][:len(first)])
    with pytest.raises(lib.CsError):
        ops.cloud_resample(v, [0, 4], [4, 5], 4)                 # no idx: every cloud must hold exactly num rows
    with pytest.raises(lib.CsError):
        ops.cloud_resample(torch.zeros(10, 2), [0], [4], 2, idx=[[0, 1]])
    with pytest.raises(lib.CsError):
        ops.cloud_resample(v, [0], [4], 0, idx=[[]])
    cl = torch.zeros(3, 8, 3)
    for pairs in ([[0, 3]], [[-1, 0]], [[0, 1, 2]], torch.tensor([[0.0, 1.0]])):
        with pytest.raises(lib.CsError):
            ops.chamfer_pairlist(cl, pairs)
    with pytest.raises(lib.CsError):
        ops.chamfer_pairlist(torch.zeros(3, 8, 2), [[0, 1]])
    with pytest.raises(lib.CsError):
        ops.chamfer_pairlist(torch.zeros(2, 32769, 3), [[0, 1]])
    # what is right reaches the device check, and only that
    with pytest.raises(lib.CsError, match="HIP device"):
        ops.cloud_resample(v, [0, 4], [4, 5], 2, idx=[[0, 3], [1, 4]])
    with pytest.raises(lib.CsError, match="HIP device"):
        ops.chamfer_pairlist(cl, [[0, 2], [1, 1]])
