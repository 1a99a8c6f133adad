"""CPU suite of commonscenes_amd/fid.py: the subset draw, the room filter, the route rule, the refusals and the two host
finishing steps of frechet_distance on host-built float64 Gram / covariance matrices (no launch anywhere)."""
import numpy as np
import pytest
import torch

import _fid_ref as ref


def _feats(n1, n2, d, seed):
    rng = np.random.default_rng(seed)
    f1 = (rng.standard_normal((n1, d)) * rng.uniform(0.5, 2.0, size=d) + rng.standard_normal(d)).astype(np.float32)
    f2 = (rng.standard_normal((n2, d)) * rng.uniform(0.5, 2.0, size=d) + 0.3 * rng.standard_normal(d)).astype(np.float32)
    return f1, f2


def test_entries_are_built_exported_and_refuse_bad_arguments():
    import ctypes as C
    from commonscenes_amd import build, lib
    assert "cs_fid.hip" in build.SOURCES and (build.CSRC / "cs_fid.hip").exists()
    dll = lib.load()
    assert dll.cs_abi_version() == 18
    for name in ("cs_fid_moments", "cs_fid_widen", "cs_fid_gram", "cs_fid_subset_sums"):
        assert name in lib.SIGNATURES and hasattr(dll, name)
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    E = lib.CS_EINVAL
    assert dll.cs_fid_moments(p, 4, 3, 2, p, p, None) == E                           # ldx < d
    assert dll.cs_fid_moments(p, 0, 3, 3, p, p, None) == E
    assert dll.cs_fid_widen(p, 4, 3, 3, None, p, 2, 0, None) == E                    # ldo < d
    assert dll.cs_fid_widen(p, 4, 3, 3, None, p, 3, 1, None) == E                    # transposed: ldo < n
    assert dll.cs_fid_gram(p, p, p, 2, 2, 3, 2, 3, 2, 0, 1.0, 0.0, None) == E        # lda < k
    assert dll.cs_fid_gram(p, p, p, 2, 2, 3, 3, 3, 1, 0, 1.0, 0.0, None) == E        # ldg < n2
    assert dll.cs_fid_gram(p, p, p, 2, 2, 3, 3, 3, 2, 2, 1.0, 0.0, None) == E        # mode
    assert dll.cs_fid_subset_sums(p, 2, 2, 1, p, p, 1, 2, 0, p, p, None) == E        # ldk < n_c
    assert dll.cs_fid_subset_sums(p, 2, 2, 2, p, p, 1, 2, 0, p, None, None) == E     # no index word


def test_kid_subsets_are_cleanfids_interleaved_draws():
    from commonscenes_amd import fid
    np.random.seed(7)
    i2, i1 = fid.kid_subsets(37, 29, 5, 23)
    np.random.seed(7)
    for s in range(5):
        assert np.array_equal(i2[s], np.random.choice(29, 23, replace=False))
        assert np.array_equal(i1[s], np.random.choice(37, 23, replace=False))
    assert i2.dtype == i1.dtype == np.int32 and i2.shape == i1.shape == (5, 23)
    assert all(len(set(r.tolist())) == 23 for r in i2) and i2.max() < 29 and i1.max() < 37
    for bad in ((37, 29, 0, 23), (37, 29, 5, 30), (37, 29, 5, 0)):
        with pytest.raises(ValueError):
            fid.kid_subsets(*bad)


def test_select_room_is_the_scripts_filter():
    from commonscenes_amd import fid
    names = ["Bedroom-1.png", "MasterBedroom-22.png", "SecondBedroom-3.png", "LivingDiningRoom-4.png", "LivingRoom-5.png",
             "DiningRoom-6.png", "Bedroom-7.obj", "KidsRoom-8.png", "LivingRoom.png", "Bedroom-9-extra.png", "notes.txt"]
    assert fid.select_room(names, "bedroom") == ["Bedroom-1.png", "MasterBedroom-22.png", "SecondBedroom-3.png",
                                                 "Bedroom-9-extra.png"]
    assert fid.select_room(names, "livingroom") == ["LivingDiningRoom-4.png", "LivingRoom-5.png"]
    assert fid.select_room(names, "diningroom") == ["LivingDiningRoom-4.png", "DiningRoom-6.png"]      # in both rooms
    assert fid.select_room(names, "all") == [n for n in names if n.endswith(".png")]
    with pytest.raises(ValueError):
        fid.select_room(names, "kitchen")
    assert fid.ROOM_DICT == {'bedroom': ["Bedroom", "MasterBedroom", "SecondBedroom"],
                             'livingroom': ['LivingDiningRoom', 'LivingRoom'], 'diningroom': ['LivingDiningRoom', 'DiningRoom']}


def test_route_rule():
    from commonscenes_amd import fid
    assert fid.pick_route(20, 30, 48) == "gram" and fid.pick_route(33, 17, 70) == "gram"
    assert fid.pick_route(64, 48, 16) == "cov" and fid.pick_route(200, 150, 64) == "cov"
    assert fid.pick_route(512, 5000, 512) == "gram" and fid.pick_route(513, 5000, 512) == "cov"
    assert fid.pick_route(5000, 300, 512) == "gram"


@pytest.mark.parametrize("fn", ["frechet_distance", "kernel_distance"])
def test_refusals_come_before_any_launch(fn):
    from commonscenes_amd import fid, lib
    f = getattr(fid, fn)
    a, b = torch.zeros(8, 6), torch.zeros(5, 6)
    with pytest.raises(lib.CsError):
        f(a, b)                                             # CPU tensors
    with pytest.raises(lib.CsError):
        f(a.double(), b.double())                           # not float32
    with pytest.raises(lib.CsError):
        f(a.half(), b)
    with pytest.raises(lib.CsError):
        f(a, torch.zeros(5, 7))                             # width mismatch
    with pytest.raises(lib.CsError):
        f(a.numpy(), b)                                     # not a tensor
    with pytest.raises(lib.CsError):
        f(torch.zeros(8), b)                                # not [N, d]
    with pytest.raises(ValueError):
        f(a, torch.zeros(1, 6))                             # N < 2
    with pytest.raises(ValueError):
        f(torch.zeros(1, 6), b)


def test_more_refusals():
    from commonscenes_amd import fid, lib
    with pytest.raises(ValueError):
        fid.frechet_distance(torch.zeros(4, 3), torch.zeros(4, 3), route="sqrtm")
    with pytest.raises(lib.CsError):
        fid.moments(torch.zeros(4, 3))
    with pytest.raises(lib.CsError):
        fid.widen(torch.zeros(4, 3))
    with pytest.raises(lib.CsError):
        fid.gram(torch.zeros(4, 3, dtype=torch.float64), torch.zeros(4, 3, dtype=torch.float64))
    with pytest.raises(lib.CsError):
        fid.subset_sums(torch.zeros(4, 4, dtype=torch.float64), [[0, 1]], [[0, 1]], True)
    with pytest.raises(lib.CsError):
        fid.compute_fid(np.zeros((4, 3), np.float64), np.zeros((4, 3), np.float64))      # float64 features
    with pytest.raises(lib.CsError):
        fid.image_features(["a.png"], model=None)


def _host_parts(f1, f2):
    f1, f2 = f1.astype(np.float64), f2.astype(np.float64)
    mu1, mu2 = f1.mean(axis=0), f2.mean(axis=0)
    a, b = f1 - mu1, f2 - mu2
    return mu1, mu2, a, b, float((a * a).sum()), float((b * b).sum())


@pytest.mark.parametrize("shape", [(64, 48, 16), (200, 150, 64)])
def test_both_finishing_steps_agree_on_full_rank_covariances(shape):
    from commonscenes_amd import fid
    n1, n2, d = shape
    f1, f2 = _feats(n1, n2, d, seed=n1)
    mu1, mu2, a, b, ss1, ss2 = _host_parts(f1, f2)
    tr_g = fid.trace_sqrt_from_gram(a @ b.T, n1, n2)
    tr_c = fid.trace_sqrt_from_cov(a.T @ a / (n1 - 1), b.T @ b / (n2 - 1))
    via_gram = fid.fid_from_parts(mu1, mu2, ss1, ss2, n1, n2, tr_g)
    via_cov = fid.fid_from_parts(mu1, mu2, ss1, ss2, n1, n2, tr_c)
    want = ref.frechet_distance(f1, f2, form="eigh")
    print(f"{shape}: gram {via_gram!r} cov {via_cov!r} ref {want!r}")
    assert abs(via_gram - via_cov) <= 1e-12 * abs(want)
    assert abs(via_gram - want) <= 1e-12 * abs(want) and abs(via_cov - want) <= 1e-12 * abs(want)


@pytest.mark.parametrize("shape", [(20, 30, 48), (33, 17, 70)])
def test_gram_finishing_step_on_singular_covariances(shape):
    from commonscenes_amd import fid
    n1, n2, d = shape
    f1, f2 = _feats(n1, n2, d, seed=n1)
    mu1, mu2, a, b, ss1, ss2 = _host_parts(f1, f2)
    got = fid.fid_from_parts(mu1, mu2, ss1, ss2, n1, n2, fid.trace_sqrt_from_gram(a @ b.T, n1, n2))
    want = ref.frechet_distance(f1, f2, form="svd")
    print(f"{shape}: gram {got!r} ref {want!r}")
    assert abs(got - want) <= 1e-12 * abs(want)


def test_kid_accumulation_is_cleanfids():
    """kid_from_sums on host-gathered sums against the reference loop"""
    from commonscenes_amd import fid
    f1, f2 = _feats(37, 29, 19, seed=3)
    np.random.seed(11)
    want, _ = ref.kernel_distance(f1, f2, num_subsets=5, max_subset_size=23)
    np.random.seed(11)
    i2, i1 = fid.kid_subsets(37, 29, 5, 23)
    x, y = f2.astype(np.float64), f1.astype(np.float64)
    kxx, kyy, kxy = (x @ x.T / 19 + 1) ** 3, (y @ y.T / 19 + 1) ** 3, (x @ y.T / 19 + 1) ** 3
    off = lambda k, r: k[np.ix_(r, r)].sum() - np.diag(k[np.ix_(r, r)]).sum()
    got = fid.kid_from_sums([off(kxx, r) for r in i2], [off(kyy, r) for r in i1],
                            [kxy[np.ix_(a, b)].sum() for a, b in zip(i2, i1)], 23)
    assert abs(got - want) <= 1e-12 * max(1.0, abs(want))
