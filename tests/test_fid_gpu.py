"""GPU suite of the FID / KID statistics: the four entries of csrc/cs_fid.hip against numpy float64 with bounds evaluated from
the operands, then frechet_distance / kernel_distance, the directory-to-number path through a tiny CLIP, and the tool."""
import json
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import _fid_ref as ref

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
U = 2.0 ** -53
SENTINEL = -12345.678


def _feats(n1, n2, d, seed):
    rng = np.random.default_rng(seed)
    f1 = (rng.standard_normal((n1, d)) * rng.uniform(0.5, 2.0, size=d) + rng.standard_normal(d)).astype(np.float32)
    f2 = (rng.standard_normal((n2, d)) * rng.uniform(0.5, 2.0, size=d) + 0.3 * rng.standard_normal(d)).astype(np.float32)
    return f1, f2


# ---- cs_fid_gram ----------------------------------------------------------------------------------------------------------
GRAM_SHAPES = [(1, 1, 1), (16, 16, 4), (17, 15, 5), (65, 33, 19), (130, 70, 515)]


def _gram_operands(n1, n2, k, seed):
    """operands inside wider NaN-filled buffers, and a sentinel-filled output"""
    rng = np.random.default_rng(seed)
    a, b = rng.standard_normal((n1, k)), rng.standard_normal((n2, k))
    abuf = np.full((n1, k + 3), np.nan)
    bbuf = np.full((n2, k + 5), np.nan)
    abuf[:, :k], bbuf[:, :k] = a, b
    return a, b, torch.from_numpy(abuf).cuda(), torch.from_numpy(bbuf).cuda()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", GRAM_SHAPES)
def test_gram_against_float64_with_the_operand_bound(shape, mode):
    from commonscenes_amd import fid
    n1, n2, k = shape
    a, b, abuf, bbuf = _gram_operands(n1, n2, k, seed=n1 + n2)
    gbuf = torch.full((n1, n2 + 7), SENTINEL, dtype=torch.float64, device="cuda")
    gamma, coef0 = 1.0 / k, 1.0
    fid.gram(abuf[:, :k], bbuf[:, :k], mode, gamma, coef0, out=gbuf[:, :n2])
    got = gbuf.cpu().numpy()
    assert (got[:, n2:] == SENTINEL).all(), "padding columns of the output were written"
    got = got[:, :n2]
    assert np.isfinite(got).all(), "NaN padding of an operand reached the output"
    s = a @ b.T
    e = k * 2.0 ** -52 * (np.abs(a) @ np.abs(b).T)
    if mode == 0:
        want, bound = s, e
    else:
        p = s * gamma + coef0
        want = p * p * p
        bound = 3 * p * p * gamma * e + 8 * U * np.abs(p) ** 3
    worst = float((np.abs(got - want) / bound).max())
    print(f"gram {shape} mode {mode}: worst error / bound = {worst:.3e}")
    assert worst <= 1.0


def test_gram_rows_alone_carry_the_bits_of_the_full_matrix():
    from commonscenes_amd import fid
    n1, n2, k = 65, 33, 19
    _, _, abuf, bbuf = _gram_operands(n1, n2, k, seed=5)
    for mode in (0, 1):
        full = fid.gram(abuf[:, :k], bbuf[:, :k], mode, 1.0 / k, 1.0)
        part = fid.gram(abuf[3:20, :k], bbuf[:, :k], mode, 1.0 / k, 1.0)
        assert torch.equal(full[3:20], part)
        cols = fid.gram(abuf[:, :k], bbuf[7:30, :k], mode, 1.0 / k, 1.0)
        assert torch.equal(full[:, 7:30], cols)


def test_gram_refuses_bad_arguments():
    from commonscenes_amd import fid, lib
    a = torch.zeros(4, 3, dtype=torch.float64, device="cuda")
    with pytest.raises(lib.CsError):
        fid.gram(a, torch.zeros(4, 5, dtype=torch.float64, device="cuda"))
    with pytest.raises(lib.CsError):
        fid.gram(a, a, mode=2)
    with pytest.raises(lib.CsError):
        fid.gram(a.float(), a.float())


# ---- cs_fid_moments / cs_fid_widen ----------------------------------------------------------------------------------------
MOMENT_SHAPES = [(2, 1), (37, 19), (300, 70)]


def _offset_data(n, d, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, d)) + 100.0).astype(np.float32)
    buf = torch.full((n, d + 5), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :d] = torch.from_numpy(x).cuda()
    return x, buf[:, :d]


@pytest.mark.parametrize("shape", MOMENT_SHAPES)
def test_moments_second_pass_holds_where_the_one_pass_form_fails(shape):
    from commonscenes_amd import fid
    n, d = shape
    x, view = _offset_data(n, d, seed=n)
    mu, ss = fid.moments(view)
    mu, ss = mu.cpu().numpy(), float(ss[0].cpu())
    x64 = x.astype(np.float64)
    mu_ref = np.array([math.fsum(x64[:, c]) / n for c in range(d)])
    ss_ref = float(((x64 - x64.mean(axis=0)) ** 2).sum())
    mu_bound = n * 2.0 ** -52 * np.abs(x64).mean(axis=0)
    ss_bound = n * d * 2.0 ** -50 * ss_ref
    print(f"moments {shape}: mu err / bound {float((np.abs(mu - mu_ref) / mu_bound).max()):.3e}, "
          f"ss err / bound {abs(ss - ss_ref) / ss_bound:.3e}")
    assert (np.abs(mu - mu_ref) <= mu_bound).all()
    assert abs(ss - ss_ref) <= ss_bound
    # the one-pass form sum x^2 - n mu^2, emulated in the features' own precision (products and running sums rounded to
    # float32, what a single pass over the fp32 rows does): it misses the same bound at every shape.  Carried in float64 it
    # is printed only: x^2 of an fp32 value is exact in float64, so at (2, 1) that form is exact, at (37, 19) it lands at
    # 0.3 - 0.8 of the bound and only at (300, 70) beyond it (1.6) -- no assertion can hold for it at all three shapes.
    sq = np.cumsum(x * x, axis=0, dtype=np.float32)[-1]
    mean32 = (np.cumsum(x, axis=0, dtype=np.float32)[-1] / np.float32(n)).astype(np.float32)
    one_pass = float((sq - np.float32(n) * mean32 * mean32).astype(np.float64).sum())
    one_pass64 = float(((x64 * x64).sum(axis=0) - n * mu_ref * mu_ref).sum())
    print(f"    one-pass form: err / bound {abs(one_pass - ss_ref) / ss_bound:.3e} in float32, "
          f"{abs(one_pass64 - ss_ref) / ss_bound:.3e} in float64")
    assert abs(one_pass - ss_ref) > ss_bound


@pytest.mark.parametrize("shape", MOMENT_SHAPES)
def test_widen_is_one_exact_subtraction_in_both_orientations(shape):
    from commonscenes_amd import fid
    n, d = shape
    x, view = _offset_data(n, d, seed=n + 1)
    mu, _ = fid.moments(view)
    for m in (None, mu):
        want = view.double() if m is None else view.double() - m
        assert torch.equal(fid.widen(view, m), want)
        assert torch.equal(fid.widen(view, m, transpose=True), want.t().contiguous())
        wide = torch.full((d, n + 3), SENTINEL, dtype=torch.float64, device="cuda")
        fid.widen(view, m, transpose=True, out=wide[:, :n])
        assert torch.equal(wide[:, :n], want.t()) and bool((wide[:, n:] == SENTINEL).all())
        wide = torch.full((n, d + 2), SENTINEL, dtype=torch.float64, device="cuda")
        fid.widen(view, m, out=wide[:, :d])
        assert torch.equal(wide[:, :d], want) and bool((wide[:, d:] == SENTINEL).all())


# ---- cs_fid_subset_sums ---------------------------------------------------------------------------------------------------
SUBSET_CASES = [(41, 37, 1, 2), (41, 37, 7, 23), (41, 37, 3, 37), (70, 70, 2, 67)]


def _subset_case(nr, nc, nsub, m, seed):
    rng = np.random.default_rng(seed)
    k = rng.standard_normal((nr, nc)) * 3.0
    ri = np.stack([rng.permutation(nr)[:m] for _ in range(nsub)]).astype(np.int32)
    ci = np.stack([rng.permutation(nc)[:m] for _ in range(nsub)]).astype(np.int32)
    kbuf = torch.full((nr, nc + 4), float("nan"), dtype=torch.float64, device="cuda")
    kbuf[:, :nc] = torch.from_numpy(k).cuda()
    return k, kbuf[:, :nc], ri, ci


def _subset_ref(k, ri, ci, skip):
    out = []
    for r, c in zip(ri, ci):
        blk = k[np.ix_(r, c)]
        out.append(blk.sum() - (np.trace(blk) if skip else 0.0))
    return np.array(out)


@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("case", SUBSET_CASES)
def test_subset_sums_against_numpy_and_bit_stable(case, skip):
    from commonscenes_amd import fid, ops
    nr, nc, nsub, m = case
    k, kview, ri, ci = _subset_case(nr, nc, nsub, m, seed=nsub * 100 + m)
    got = fid.subset_sums(kview, ri, ci, skip)
    again = fid.subset_sums(kview, torch.from_numpy(ri).cuda(), torch.from_numpy(ci).cuda(), skip)
    assert torch.equal(got, again)
    ops.check_index_errors(kview.device)
    bound = m ** 2 * 2.0 ** -52 * float(np.abs(k).max()) * m ** 2
    err = np.abs(got.cpu().numpy() - _subset_ref(k, ri, ci, skip))
    print(f"subset sums {case} skip_diag={skip}: worst error {err.max():.3e}, bound {bound:.3e}")
    assert (err <= bound).all()


def test_subset_sums_bad_index_gives_nan_and_raises():
    from commonscenes_amd import fid, ops
    nr, nc, nsub, m = 41, 37, 7, 23
    k, kview, ri, ci = _subset_case(nr, nc, nsub, m, seed=9)
    ops.check_index_errors(kview.device)              # start from a clean word
    want = _subset_ref(k, ri, ci, True)
    bad_r, bad_c = ri.copy(), ci.copy()
    bad_r[2, 5] = nr                                  # one past the last row
    bad_c[4, 0] = -1
    got = fid.subset_sums(kview, bad_r, bad_c, True).cpu().numpy()
    assert np.isnan(got[2]) and np.isnan(got[4])
    keep = [s for s in range(nsub) if s not in (2, 4)]
    bound = m ** 2 * 2.0 ** -52 * float(np.abs(k).max()) * m ** 2
    assert (np.abs(got[keep] - want[keep]) <= bound).all()
    with pytest.raises(IndexError):
        ops.check_index_errors(kview.device, what="subset rows")
    ops.check_index_errors(kview.device)              # the word was cleared by the raise


# ---- frechet_distance -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,route", [((20, 30, 48), "gram"), ((33, 17, 70), "gram"), ((64, 48, 16), "cov"),
                                         ((200, 150, 64), "cov")])
def test_frechet_distance_both_routes(shape, route):
    from commonscenes_amd import fid
    n1, n2, d = shape
    f1, f2 = _feats(n1, n2, d, seed=n1)
    assert fid.pick_route(n1, n2, d) == route
    got = fid.frechet_distance(torch.from_numpy(f1).cuda(), torch.from_numpy(f2).cuda())
    want = ref.frechet_distance(f1, f2, form="svd" if route == "gram" else "eigh")
    print(f"frechet_distance {shape} ({route}): {got!r} vs {want!r}, rel {abs(got - want) / abs(want):.3e}")
    assert isinstance(got, float) and abs(got - want) <= 1e-9 * abs(want)
    assert fid.frechet_distance(torch.from_numpy(f1).cuda(), torch.from_numpy(f2).cuda(), route=route) == got


@pytest.mark.parametrize("shape", [(20, 30, 48), (64, 48, 16)])
def test_frechet_distance_of_a_set_with_itself(shape):
    from commonscenes_amd import fid
    f1, _ = _feats(*shape, seed=2)
    x = torch.from_numpy(f1).cuda()
    tr_s = float(np.trace(np.atleast_2d(np.cov(f1.astype(np.float64), rowvar=False))))
    got = fid.frechet_distance(x, x)
    print(f"frechet_distance(x, x) {shape}: {got:.3e} (tr S = {tr_s:.3e})")
    assert abs(got) <= 1e-9 * tr_s


def test_forced_cov_route_on_a_singular_case_is_the_less_exact_one():
    from commonscenes_amd import fid
    f1, f2 = _feats(20, 30, 48, seed=20)
    x1, x2 = torch.from_numpy(f1).cuda(), torch.from_numpy(f2).cuda()
    want = ref.frechet_distance(f1, f2, form="svd")
    e_gram = abs(fid.frechet_distance(x1, x2, route="gram") - want) / abs(want)
    e_cov = abs(fid.frechet_distance(x1, x2, route="cov") - want) / abs(want)
    print(f"singular (20, 30, 48): gram route rel {e_gram:.3e}, forced cov route rel {e_cov:.3e}")
    assert e_cov <= 1e-6 and e_gram <= 1e-9 and e_cov >= e_gram


def test_non_finite_features_are_refused_after_the_moments():
    from commonscenes_amd import fid
    f1, f2 = _feats(20, 30, 8, seed=4)
    for bad in (float("nan"), float("inf")):
        g = f2.copy()
        g[3, 2] = bad
        with pytest.raises(ValueError):
            fid.frechet_distance(torch.from_numpy(f1).cuda(), torch.from_numpy(g).cuda())
        with pytest.raises(ValueError):
            fid.kernel_distance(torch.from_numpy(f1).cuda(), torch.from_numpy(g).cuda(), num_subsets=2, seed=0)


# ---- kernel_distance ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(37, 29, 19, 5, 23), (29, 37, 19, 3, 1000), (130, 70, 515, 4, 64)])
def test_kernel_distance_against_cleanfids_loop(case):
    from commonscenes_amd import fid
    n1, n2, d, subsets, cap = case
    f1, f2 = _feats(n1, n2, d, seed=n1 + d)
    x1, x2 = torch.from_numpy(f1).cuda(), torch.from_numpy(f2).cuda()
    np.random.seed(123)
    got = fid.kernel_distance(x1, x2, num_subsets=subsets, max_subset_size=cap)
    np.random.seed(123)
    want, kmax = ref.kernel_distance(f1, f2, num_subsets=subsets, max_subset_size=cap)
    print(f"kernel_distance {case}: {got!r} vs {want!r}, |diff| {abs(got - want):.3e}, max|k| {kmax:.3e}")
    assert isinstance(got, float) and abs(got - want) <= 1e-11 * max(1.0, kmax)
    a = fid.kernel_distance(x1, x2, num_subsets=subsets, max_subset_size=cap, seed=5)
    state = np.random.get_state()[1].copy()
    b = fid.kernel_distance(x1, x2, num_subsets=subsets, max_subset_size=cap, seed=5)
    assert a == b
    np.random.seed(5)
    assert fid.kernel_distance(x1, x2, num_subsets=subsets, max_subset_size=cap) == a      # seed= is np.random.seed
    assert np.array_equal(np.random.get_state()[1], state)


# ---- end to end -----------------------------------------------------------------------------------------------------------
TINY_VISION = dict(width=128, layers=2, patch=32, grid=2, embed=32)       # the fixture's v0: 64 x 64 images, 5 tokens, 2 heads


def test_directories_to_numbers_through_a_tiny_clip(tmp_path):
    from PIL import Image
    from commonscenes_amd import clip as K, fid
    model = K.CLIP("cuda").load_state_dict(K.synth_clip_state_dict({"vision": TINY_VISION}, 41))
    size = model.vision.resolution
    rng = np.random.default_rng(8)
    rooms = ["Bedroom", "MasterBedroom", "LivingRoom", "SecondBedroom", "DiningRoom"]
    dirs = {}
    for name, count in (("real", 12), ("fake", 9)):
        (tmp_path / name).mkdir()
        for i in range(count):
            img = rng.integers(0, 256, size=(size, size, 3), dtype=np.uint8)
            Image.fromarray(img).save(tmp_path / name / f"{rooms[i % len(rooms)]}-{i:03d}.png")
        (tmp_path / name / "Bedroom-notes.txt").write_text("not an image")
        dirs[name] = tmp_path / name
    for room in ("bedroom", "all"):
        files = {k: fid.list_images(v, room) for k, v in dirs.items()}
        assert all(Path(f).name.split("-")[0] in fid.ROOM_DICT["bedroom"] for f in files["real"]) or room == "all"
        assert len(files["real"]) == (8 if room == "bedroom" else 12) and len(files["fake"]) == (6 if room == "bedroom" else 9)
        f1, f2 = fid.image_features(files["real"], model, batch=5), fid.image_features(files["fake"], model)
        assert f1.dtype == torch.float32 and tuple(f1.shape) == (len(files["real"]), 32) and f1.is_cuda
        got_fid = fid.compute_fid(dirs["real"], dirs["fake"], model=model, room=room, batch=5)
        got_kid = fid.compute_kid(str(dirs["real"]), str(dirs["fake"]), model=model, room=room, num_subsets=4, seed=3,
                                  batch=5)
        f1b = fid.image_features(files["real"], model, batch=5)
        assert got_fid == fid.frechet_distance(f1b, f2)
        assert got_kid == fid.kernel_distance(f1b, f2, num_subsets=4, seed=3)
        h1, h2 = f1b.cpu().numpy(), f2.cpu().numpy()
        form = "svd" if fid.pick_route(len(h1), len(h2), 32) == "gram" else "eigh"
        want_fid = ref.frechet_distance(h1, h2, form=form)
        np.random.seed(3)
        want_kid, kmax = ref.kernel_distance(h1, h2, num_subsets=4)
        print(f"room {room}: fid {got_fid!r} vs {want_fid!r}; kid {got_kid!r} vs {want_kid!r}")
        assert abs(got_fid - want_fid) <= 1e-9 * abs(want_fid)
        assert abs(got_kid - want_kid) <= 1e-11 * max(1.0, kmax)
    # features from outside: arrays and .npy paths take the same route as tensors
    np.save(tmp_path / "real.npy", h1)
    np.save(tmp_path / "fake.npy", h2)
    assert fid.compute_fid(tmp_path / "real.npy", h2) == fid.frechet_distance(f1b, f2)


# ---- the tool -------------------------------------------------------------------------------------------------------------
def test_fid_table_tool_prints_the_in_process_numbers():
    from commonscenes_amd import fid
    out = subprocess.run([sys.executable, str(ROOT / "tools" / "fid_table.py"), "--synthetic", "40", "30", "24", "--seed", "1"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("FID_TABLE ")]
    assert len(lines) == 1
    rec = json.loads(lines[0][len("FID_TABLE "):])
    assert set(rec) >= {"fid", "kid", "n_real", "n_fake", "d", "route", "kid_subsets", "kid_subset_size", "seed"}
    assert (rec["n_real"], rec["n_fake"], rec["d"], rec["route"], rec["seed"]) == (40, 30, 24, "cov", 1)
    spec = __import__("importlib.util").util.spec_from_file_location("fid_table", ROOT / "tools" / "fid_table.py")
    tool = __import__("importlib.util").util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    f1, f2 = tool.synthetic_features(40, 30, 24)
    x1, x2 = torch.from_numpy(f1).cuda(), torch.from_numpy(f2).cuda()
    assert rec["fid"] == fid.frechet_distance(x1, x2)
    assert rec["kid"] == fid.kernel_distance(x1, x2, num_subsets=rec["kid_subsets"], max_subset_size=rec["kid_subset_size"],
                                             seed=1)
