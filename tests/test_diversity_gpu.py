"""The diversity and consistency tables on the MI355X (commonscenes_amd/diversity.py over cs_cloud_resample and
cs_chamfer_pairlist) against
  * what the reference's own sample_points / normalize gave on the CPU (tests/golden/diversity.npz),
  * the reference's formulas restated in numpy float32 / float64 here,
  * the project's all-pairs Chamfer matrix, whose bits the pair list must carry.
No test hands a kernel an out-of-range index: the host checks are tested on the CPU.  Every figure is printed before it is
asserted."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden" / "diversity.npz"


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _bits(t):
    t = t.detach().cpu().contiguous() if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    return t.view(torch.int32)


def _same_bits_or_both_nan(got, want, what):
    """the same NaN mask, bit-equal elsewhere"""
    got = got.detach().cpu() if isinstance(got, torch.Tensor) else torch.from_numpy(got)
    want = want.detach().cpu() if isinstance(want, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(want))
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, what
    gn, wn = torch.isnan(got), torch.isnan(want)
    differ = int((_bits(got)[~wn] != _bits(want)[~wn]).sum()) if bool((gn == wn).all()) else -1
    print(f"{what}: NaN {int(gn.sum())} / {int(wn.sum())}, entries that differ elsewhere {differ}")
    assert bool((gn == wn).all()) and differ == 0, what


def _first(counts):
    return np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64).tolist()


def _np_normalize(v):
    """scripts/eval_3dfront.py:783-796 restated on float32 data"""
    v = np.array(v, np.float32, copy=True)
    for a in range(3):
        lo, hi = np.amin(v[:, a]), np.amax(v[:, a])
        v[:, a] += -lo - (hi - lo) * np.float32(0.5)
    with np.errstate(divide="ignore", invalid="ignore"):
        return v / np.max(v, axis=0)


def _brute_cd(a, b):
    """float64 Chamfer distance of two [p, 3] clouds"""
    d = ((a.double()[:, None, :] - b.double()[None, :, :]) ** 2).sum(-1)
    return float(d.min(dim=1).values.mean() + d.min(dim=0).values.mean())


# 1 ------------------------------------------------------------------------------------------------------------------
def test_resample_against_the_reference(gold):
    from commonscenes_amd import diversity as D, ops
    counts = gold["counts"].tolist()
    verts = torch.from_numpy(gold["verts"]).cuda()
    first = _first(counts)
    for num in gold["nums"].tolist():
        idx = torch.from_numpy(gold[f"idx_{num}"])
        got = ops.cloud_resample(verts, first, counts, num, idx=idx)
        assert got.shape == (len(counts), num, 3) and got.is_cuda
        differ = int((_bits(got) != _bits(gold[f"sampled_{num}"])).sum())
        print(f"sampled num={num}: entries that differ {differ}")
        assert differ == 0
        nrm = ops.cloud_resample(verts, first, counts, num, idx=idx, normalize=True)
        _same_bits_or_both_nan(nrm, gold[f"normalized_{num}"], f"normalized num={num}")
        assert bool(torch.isnan(nrm[0]).all()) and not bool(torch.isnan(nrm[1:]).any())      # the one-vertex cloud
        # every cloud alone: no dependence on n or on the cloud's place in the launch
        for i in range(len(counts)):
            one = ops.cloud_resample(verts, [first[i]], [counts[i]], num, idx=idx[i:i + 1], normalize=True)
            assert torch.equal(_bits(one[0]), _bits(nrm[i])), (num, i)
        # a device-side index tensor, and the public functions over the split of the packed buffer (read in place)
        dev = ops.cloud_resample(verts, first, counts, num, idx=idx.to(torch.int32).cuda(), normalize=True)
        assert torch.equal(_bits(dev), _bits(nrm))
        views = list(torch.split(verts, counts))
        packed, where = D._packed(views, counts)
        assert packed.data_ptr() == verts.data_ptr() and where == first
        pts = D.sample_points(views, num, indices=idx)
        assert len(pts) == len(counts) and torch.equal(torch.stack(pts), got)
        assert pts[1].untyped_storage().data_ptr() == pts[0].untyped_storage().data_ptr()
        assert torch.equal(D.sample_points_packed(verts, counts, num, indices=idx), got)
        # clouds that do not share a buffer (and live on the host) are packed once: the same rows
        loose = [v.cpu().clone() for v in views]
        assert torch.equal(torch.stack(D.sample_points(loose, num, indices=idx)), got)
        # drawn here under the seed: the rows the reference drew
        torch.manual_seed(47)
        assert torch.equal(torch.stack(D.sample_points(views, num)), got)
    for i in range(3):
        _same_bits_or_both_nan(D.normalize(torch.from_numpy(gold[f"hand_{i}"]).cuda()), gold[f"hand_normalized_{i}"],
                               f"hand-made cloud {i}")
    assert int(ops.index_error_word().item()) == 0


# 2 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 255, 256, 257, 1030])
def test_normalize_at_the_shape_boundaries(P, N):
    from commonscenes_amd import diversity as D
    rng = np.random.default_rng(100 * P + N)
    v = ((rng.random((N, P, 3)) - 0.3) * np.array([2.0, 0.7, 11.0])).astype(np.float32)
    want = np.stack([_np_normalize(c) for c in v])
    got = D.normalize(torch.from_numpy(v).cuda())
    _same_bits_or_both_nan(got, want, f"normalize P={P} N={N}")
    assert bool(torch.isnan(got).all()) == (P == 1)
    one = D.normalize(torch.from_numpy(v[N - 1]).cuda())
    assert one.shape == (P, 3)
    _same_bits_or_both_nan(one, want[N - 1], f"normalize P={P}, the last cloud alone")
    if P > 1:
        assert torch.equal(D.normalize(torch.from_numpy(v).cuda(), scale=2), got * 2)


# 3 ------------------------------------------------------------------------------------------------------------------
def test_ragged_unaligned_clouds(gold):
    """every cloud behind a pad so that every first[i] is odd: a cloud starts 12 bytes past a 24-byte boundary, never on a
    16-byte one by construction of the index"""
    from commonscenes_amd import ops
    counts = gold["counts"].tolist()
    src = torch.from_numpy(gold["verts"])
    chunks, first, at = [], [], 0
    for c in torch.split(src, counts):
        pad = 1 if at % 2 == 0 else 2
        chunks += [torch.full((pad, 3), 7e8), c]
        first.append(at + pad)
        at += pad + c.shape[0]
    assert all(f % 2 == 1 for f in first)
    verts = torch.cat(chunks).cuda()
    for num in gold["nums"].tolist():
        idx = torch.from_numpy(gold[f"idx_{num}"])
        got = ops.cloud_resample(verts, first, counts, num, idx=idx)
        assert int((_bits(got) != _bits(gold[f"sampled_{num}"])).sum()) == 0
        _same_bits_or_both_nan(ops.cloud_resample(verts, first, counts, num, idx=idx, normalize=True),
                               gold[f"normalized_{num}"], f"odd first rows, num={num}")


# 4 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 65, 300, 2900])
def test_chamfer_pairs(p):
    """slabs of 256 rows: p = 1 and 65 take the one-slab step, 300 the two-slab step, 2900 (twelve slabs, the last one ragged)
    a step of eight and a step of four"""
    from commonscenes_amd import diversity as D, shape_metrics as SM
    g = torch.Generator().manual_seed(p)
    c = (torch.rand((5, p, 3), generator=g) - 0.5).cuda()
    full = SM.pairwise_cd(c, c.clone())
    pairs = [(0, 1), (1, 0), (2, 2), (0, 4), (3, 1), (0, 1), (4, 0), (4, 4), (2, 3), (0, 1)]
    got = D.chamfer_pairs(c, pairs)
    assert got.shape == (len(pairs),) and got.dtype == torch.float32 and got.is_cuda
    want = torch.stack([full[i, j] for i, j in pairs])
    differ = int((_bits(got) != _bits(want)).sum())
    brute = torch.tensor([_brute_cd(c[i], c[j]) for i, j in pairs], dtype=torch.float64)
    err = rel_l2(got, brute)
    print(f"chamfer_pairs p={p}: entries that differ from pairwise_cd {differ}; rel-L2 vs float64 = {err:.3e}")
    assert differ == 0
    assert err < 1e-6
    assert float(got[2]) == 0.0 and float(got[7]) == 0.0                     # (i, i)
    assert torch.equal(_bits(got[0]), _bits(got[1])) and torch.equal(_bits(got[3]), _bits(got[6]))      # (i, j), (j, i)
    assert torch.equal(_bits(got[5]), _bits(got[0])) and torch.equal(_bits(got[9]), _bits(got[0]))      # repeated
    assert torch.equal(_bits(D.chamfer_pairs(c, [(0, 1)])), _bits(got[:1]))                             # a one-pair list
    dev_pairs = torch.tensor(pairs, dtype=torch.int32).cuda()
    assert torch.equal(_bits(D.chamfer_pairs(c, dev_pairs)), _bits(got))
    assert torch.equal(_bits(D.chamfer_pairs(c[1:4], [(2, 0)])), _bits(got[4:5]))                       # no dependence on m
    assert D.chamfer_pairs(c, []).shape == (0,)


# 5 ------------------------------------------------------------------------------------------------------------------
def test_shape_diversity():
    from commonscenes_amd import diversity as D
    from commonscenes_amd.chamfer import chamferDist
    g = torch.Generator().manual_seed(5)
    ss = (torch.rand((3, 3, 128, 3), generator=g) - 0.5).cuda()
    got = D.shape_diversity(ss)
    assert got.shape == (3,) and got.dtype == np.float64
    pairs = [(o * 3 + k, o * 3 + k + 1) for o in range(3) for k in range(2)]
    comp = D.chamfer_pairs(ss.reshape(9, 128, 3), pairs).cpu().numpy().astype(np.float64).reshape(3, 2).mean(axis=1)
    chamfer = chamferDist()
    host = []
    for o in range(3):                                                        # eval_3dfront.py:688-699
        seq = []
        for k in range(2):
            d1, d2 = chamfer(ss[o, k:k + 1].float(), ss[o, k + 1:k + 2].float())
            seq.append(float(d1.double().mean() + d2.double().mean()))
        host.append(np.mean(seq))
    err = float(np.abs(got - np.array(host)).max() / np.abs(host).max())
    print(f"shape_diversity {got.tolist()}: vs composition {np.abs(got - comp).max():.1e}, vs host route {err:.3e}")
    assert np.array_equal(got, comp)
    assert err < 1e-6
    assert np.array_equal(D.shape_diversity(ss[1:2]), got[1:2])


# 6 ------------------------------------------------------------------------------------------------------------------
def test_sample_and_normalize_is_normalize_of_sample_points(gold):
    from commonscenes_amd import diversity as D
    counts = gold["counts"].tolist()
    views = list(torch.split(torch.from_numpy(gold["verts"]).cuda(), counts))
    for num in (64, 100):
        torch.manual_seed(3)
        both = D.sample_and_normalize(views, num)
        torch.manual_seed(3)
        two = D.normalize(torch.stack(D.sample_points(views, num)))
        _same_bits_or_both_nan(both, two, f"sample_and_normalize num={num}")
        g = torch.Generator().manual_seed(3)
        _same_bits_or_both_nan(D.sample_and_normalize(views, num, generator=g), two, "  from an explicit generator")


# 7 ------------------------------------------------------------------------------------------------------------------
CLASSES = {"_scene_": 0, "bed": 1, "chair": 2, "lamp": 3, "floor": 34}


def _analytic_sdfs(n, q, bump):
    """[4, 1, n, n, n] over [-0.5, 0.5]^3: a sphere, a box, and the same two again.  Only the first two depend on the run:
    the sphere's exponent q (2 = a sphere, larger = towards a cube) and the radius of a bump on the box's corner -- changes
    that survive the per-axis normalisation, which a change of size would not."""
    ax = (torch.arange(n, dtype=torch.float32) + 0.5) / n - 0.5
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    ball = lambda e: (x.abs() ** e + y.abs() ** e + z.abs() ** e) ** (1.0 / e) - 0.3
    box = torch.stack([x.abs() - 0.25, y.abs() - 0.2, z.abs() - 0.125]).max(dim=0).values
    bumped = torch.minimum(box, torch.sqrt((x - 0.25) ** 2 + (y - 0.2) ** 2 + (z - 0.125) ** 2) - bump)
    return torch.stack([ball(q), bumped, ball(2.0), box]).unsqueeze(1)


def test_diversity_meter_on_synthetic_sdfs():
    from commonscenes_amd import diversity as D
    objs = torch.tensor([1, 2, 2, 3, 34, 0])                                  # four shaped nodes, floor, _scene_
    runs = [_analytic_sdfs(32, 2.0 + 1.5 * k, 0.08 + 0.05 * k).cuda() for k in range(3)]
    boxes = [torch.randn(6, 6, generator=torch.Generator().manual_seed(k)) for k in range(3)]
    scores = [torch.randn(6, 24, generator=torch.Generator().manual_seed(10 + k)) for k in range(3)]
    P = 500
    m1 = D.DiversityMeter(CLASSES, points=P)
    torch.manual_seed(47)
    r1 = m1.add_scene(objs, boxes, scores, runs)
    torch.manual_seed(47)
    ready = D.DiversityMeter(CLASSES, points=P).shapes_tensor(objs, runs)
    assert ready.shape == (4, 3, P, 3) and not bool(torch.isnan(ready).any())
    m2 = D.DiversityMeter(CLASSES, points=P)
    r2 = m2.add_scene(objs, boxes, scores, ready)
    s1, s2 = m1.summary(), m2.summary()
    print("summary from SDF batches:", s1)
    assert s1 == s2 and np.array_equal(r1["shape"], r2["shape"])
    assert s1["objects"] == 4 and s1["shape"] > 0 and bool((r1["shape"] > 0).all())
    assert s1["categories"]["bed"]["n"] == 1 and s1["categories"]["chair"]["n"] == 2 and s1["categories"]["lamp"]["n"] == 1
    assert s1["categories"]["sofa"] == {"n": 0, "shape": None}
    assert s1["categories"]["bed"]["shape"] == r1["shape"][0] and s1["categories"]["lamp"]["shape"] == r1["shape"][3]
    assert s1["categories"]["chair"]["shape"] == float(np.mean(r1["shape"][1:3]))
    assert np.isfinite([s1["box_size"], s1["box_location"], s1["angle"]]).all()
    # a normalised cloud reaches exactly 1 on every axis (m / m) and about -1 on the other side
    assert float(ready.amax(dim=2).min()) == 1.0 and float(ready.amin(dim=2).max()) < -0.999
    # the K runs also arrive as Meshes / vertex lists from separate calls (packed once): the same table
    from commonscenes_amd.mesh import sdf_to_mesh
    m3 = D.DiversityMeter(CLASSES, points=P)
    torch.manual_seed(47)
    m3.add_scene(objs, boxes, scores, [sdf_to_mesh(r, render_all=True) for r in runs])
    assert m3.summary() == s1
    # objects whose K runs are the same cloud have diversity exactly 0 (their rows differ run by run when they are drawn, so
    # the runs are made identical here, after the draw)
    same = ready.clone()
    same[2:] = same[2:, :1]
    m4 = D.DiversityMeter(CLASSES, points=P)
    r4 = m4.add_scene(objs, None, None, same)
    print("identical runs for objects 2, 3:", r4["shape"].tolist())
    assert r4["shape"][2] == 0.0 and r4["shape"][3] == 0.0 and np.array_equal(r4["shape"][:2], r1["shape"][:2])


# 8 ------------------------------------------------------------------------------------------------------------------
def test_consistency_from_meshes():
    from commonscenes_amd import diversity as D
    P = 64
    sizes = [10, 37, 300, 64, 5, 120]                                         # some with fewer than P vertices
    g = torch.Generator().manual_seed(8)
    verts = [torch.rand((n, 3), generator=g) * 2 - 1 for n in sizes]
    pairs = [(0, 1), (2, 3), (4, 5), (1, 2), (3, 3)]
    cats = ["chair", "table", "chair", "lamp", "table"]
    got = D.consistency_from_meshes(verts, pairs, cats, points=P, seed=47)
    clouds = []
    for v in verts:                                                           # consistency_check.py:69-77 restated
        gen = torch.Generator().manual_seed(47)
        n = v.shape[0]
        clouds.append(v[torch.randperm(n, generator=gen)[:P] if n >= P else torch.randint(n, size=(P,), generator=gen)])
    brute = np.array([_brute_cd(clouds[i], clouds[j]) for i, j in pairs])
    print("consistency table:", got)
    assert list(got) == ["chair", "table", "lamp", "total"]
    assert [got[c]["pairs"] for c in ("chair", "table", "lamp", "total")] == [2, 2, 1, 5]
    want = np.array([brute[[0, 2]].mean(), brute[[1, 4]].mean(), brute[3], brute.sum() / 5])
    have = np.array([got[c]["chamfer"] for c in ("chair", "table", "lamp", "total")])
    err = float(np.linalg.norm(have - want) / np.linalg.norm(want))
    print(f"consistency means: rel-L2 vs float64 brute force over the same rows = {err:.3e}")
    assert err < 1e-6
    # the same table from clouds sampled by the caller
    tab = D.consistency_table(torch.stack(clouds).cuda(), pairs, cats)
    assert tab == got


# 9 ------------------------------------------------------------------------------------------------------------------
def test_scene_diversity_smoke(tmp_path):
    """width 32, 2 DDIM steps, one 4-object scene, K = 2: finite numbers of the right shapes, and the K runs went out as ONE
    coalesced sampler launch.  No parity claim: the marching-cubes vertex order is unpinned against the reference's."""
    from commonscenes_amd import diversity as D, synth
    from commonscenes_amd.vae import VAE
    spec = importlib.util.spec_from_file_location("eval_walkthrough", ROOT / "tools" / "eval_walkthrough.py")
    W = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(W)
    opt = W.build_experiment(tmp_path, 32)
    model = VAE(type="v2_full", diff_opt=opt, vocab=W.VOCAB, replace_latent=True, with_changes=True, residual=True,
                with_angles=True, clip=True, with_E2=True)
    model.load_networks(str(tmp_path), 100)
    model.compute_statistics(str(tmp_path), 100, W.synthetic_loader(3, seed=900))
    model.eval()
    d = W.synthetic_loader(1, seed=500, objects=4)[0]["decoder"]
    O = int(d["objs"].shape[0])
    scene = dict(dec_objs=d["objs"].cuda(), dec_triplets=d["tripltes"].cuda(), dec_sdfs=d["sdfs"],
                 encoded_dec_text_feat=d["text_feats"].cuda(), encoded_dec_rel_feat=d["rel_feats"].cuda())
    zs = [synth.gaussian_like(f"dv:z{k}", (O, 64)) for k in range(2)]
    x_Ts = [synth.gaussian_like(f"dv:x{k}", (1, 3, 16, 16, 16)) for k in range(2)]
    classes = {"_scene_": 0, "floor": 34, **{n: i for i, n in enumerate(D.CATEGORIES, start=1)}}
    meter = D.DiversityMeter(classes, points=500)
    torch.manual_seed(1)
    res = D.scene_diversity(model, scene, num_samples=2, ddim_steps=2, points=500, zs=zs, x_Ts=x_Ts, meter=meter)
    sizes = list(model.vae_v2.Diff.last_launch_sizes)
    print("scene_diversity:", {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in res.items()}, "launches", sizes)
    assert sizes == [8]                                                       # 2 runs x 4 shaped objects: one launch
    assert res["shape"].shape == (4,) and np.isfinite(res["shape"]).all() and (res["shape"] >= 0).all()
    assert res["box_std"].shape == (O, 6) and np.isfinite(res["box_std"]).all()
    assert res["angle_std"].shape == (O,) and np.isfinite(res["angle_std"]).all()
    assert res["shape_nodes"] == [0, 1, 2, 3]
    s = meter.summary()
    assert s["objects"] == 4 and np.isfinite(s["shape"]) and sum(c["n"] for c in s["categories"].values()) <= 4
    torch.manual_seed(1)
    bare = D.scene_diversity(model, scene, num_samples=2, ddim_steps=2, points=500, zs=zs, x_Ts=x_Ts)
    assert np.array_equal(bare["shape"], res["shape"]) and np.array_equal(bare["box_std"], res["box_std"])
