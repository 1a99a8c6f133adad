"""Host side of commonscenes_amd/shape_metrics.py against what the reference's scripts/compute_mmd_cov_1nn.py computed on the
CPU in float64 (tests/golden/shape_metrics.npz, written by tools/make_goldens.py --only shape_metrics): `lgan_mmd_cov`, `knn`
and the entropy / JSD formulas.  The fixture's minima are separated from their runners-up by >= 1e-3 (asserted by the
generator, re-checked here), so the discrete outputs are well defined and must match exactly.  No GPU."""
from pathlib import Path

import numpy as np
import pytest
import torch

GOLD = Path(__file__).resolve().parent / "golden" / "shape_metrics.npz"


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def test_fixture_holds_the_conditions_the_tests_lean_on(gold):
    assert gold["sample"].shape == gold["ref"].shape == (24, 256, 3) and gold["sample"].dtype == np.float32
    assert float(gold["cond_min_gap"]) >= 1e-3 and float(gold["cond_cell_gap"]) >= 1e-4
    assert 1 - 1e-6 <= float(gold["cond_auction_lo"]) and float(gold["cond_auction_hi"]) <= 1.5
    assert GOLD.stat().st_size < 1 << 20


def test_knn_matches_the_reference_on_stored_matrices(gold):
    from commonscenes_amd import shape_metrics as SM
    got = SM.knn(torch.from_numpy(gold["knn_xx"]), torch.from_numpy(gold["knn_xy"]), torch.from_numpy(gold["knn_yy"]), 1)
    want = dict(zip([str(k) for k in gold["knn_keys"]], gold["knn_vals"]))
    assert sorted(got) == sorted(want) == sorted(["tp", "fp", "fn", "tn", "precision", "recall", "acc_t", "acc_f", "acc"])
    for k, v in want.items():
        assert got[k].dtype == torch.float64
        assert float(got[k]) == float(v), (k, float(got[k]), float(v))        # counts and accuracies: exactly
    # numpy inputs work too, and sqrt=True changes no neighbour (monotone), so no count
    got2 = SM.knn(gold["knn_xx"], gold["knn_xy"], gold["knn_yy"], 1, sqrt=True)
    assert all(float(got2[k]) == float(want[k]) for k in ("tp", "fp", "fn", "tn", "acc"))


def test_lgan_mmd_cov_matches_the_reference_square_and_rectangular(gold):
    from commonscenes_amd import shape_metrics as SM
    keys = [str(k) for k in gold["lgan_keys"]]
    for mat, vals in ((gold["knn_xy"], gold["lgan_vals_xy"]), (gold["lgan_rect"], gold["lgan_vals_rect"])):
        got = SM.lgan_mmd_cov(torch.from_numpy(mat))
        want = dict(zip(keys, vals))
        assert sorted(got) == sorted(keys) == ["lgan_cov", "lgan_mmd", "lgan_mmd_smp"]
        assert float(got["lgan_cov"]) == float(want["lgan_cov"])
        for k in ("lgan_mmd", "lgan_mmd_smp"):
            assert abs(float(got[k]) - float(want[k])) <= 1e-12, k
    # [N_sample, N_ref]: the coverage counts refs
    d = torch.tensor([[1.0, 5.0, 9.0], [2.0, 6.0, 9.5]], dtype=torch.float64)
    r = SM.lgan_mmd_cov(d)
    assert float(r["lgan_cov"]) == float(np.float32(1.0 / 3.0)) and float(r["lgan_mmd"]) == (1.0 + 5.0 + 9.0) / 3 and float(r["lgan_mmd_smp"]) == 1.5


def test_table_statistics_on_the_reference_matrices_reproduce_its_twelve_keys(gold):
    """the plumbing of compute_all_metrics (the transposition included) fed with the REFERENCE's own float64 matrices gives
    the reference's numbers: CD keys from the CD matrices, EMD keys from the exact-assignment matrices"""
    from commonscenes_amd import shape_metrics as SM
    want = dict(zip([str(k) for k in gold["metrics_keys"]], gold["metrics_vals"]))
    assert len(want) == 12
    for tag, rs, rr, ss in (("CD", gold["cd_rs"], gold["cd_rr"], gold["cd_ss"]),
                            ("EMD", gold["emd_rs_exact"], gold["emd_rr_exact"], gold["emd_ss_exact"])):
        lg = SM.lgan_mmd_cov(torch.from_numpy(rs).t())
        nn = SM.knn(torch.from_numpy(rr), torch.from_numpy(rs), torch.from_numpy(ss), 1)
        assert float(lg["lgan_cov"]) == want[f"lgan_cov-{tag}"]
        for k in ("lgan_mmd", "lgan_mmd_smp"):
            assert abs(float(lg[k]) - want[f"{k}-{tag}"]) <= 1e-12
        for k in ("acc_t", "acc_f", "acc"):
            assert float(nn[k]) == want[f"1-NN-{tag}-{k}"], (tag, k)


def test_entropy_and_jsd_formulas_on_the_stored_counters(gold):
    from commonscenes_amd import shape_metrics as SM
    jsd = SM.jensen_shannon_divergence(gold["counters_smp"], gold["counters_ref"])
    assert abs(jsd - float(gold["jsd"])) <= 1e-12
    assert 0.0 < jsd < 1.0
    for tag in ("smp", "ref"):
        assert abs(SM.occupancy_entropy(gold[f"bernoulli_{tag}"], 24) - float(gold[f"entropy_{tag}"])) <= 1e-12
        assert int(gold[f"counters_{tag}"].sum()) == 24 * 256
        assert np.array_equal(gold[f"bernoulli_{tag}"] > 0, gold[f"counters_{tag}"] > 0)
    assert SM.jensen_shannon_divergence([1, 2, 3], [1, 2, 3]) == 0.0
    assert abs(SM.jensen_shannon_divergence([1, 0], [0, 1]) - 1.0) <= 1e-15
    with pytest.raises(ValueError):
        SM.jensen_shannon_divergence([1, -1], [1, 1])
    with pytest.raises(ValueError):
        SM.jensen_shannon_divergence([1, 1], [1, 1, 1])


def test_unit_cube_grid():
    from commonscenes_amd import shape_metrics as SM
    grid, spacing = SM.unit_cube_grid_point_cloud(28, True)
    assert grid.dtype == np.float32 and grid.ndim == 2 and grid.shape[1] == 3 and spacing == 1.0 / 27.0
    assert grid.shape[0] == len(np.load(GOLD)["counters_ref"])
    assert float(np.linalg.norm(grid, axis=1).max()) <= 0.5
    full, _ = SM.unit_cube_grid_point_cloud(4, False)
    assert full.shape == (4, 4, 4, 3) and full[1, 2, 3].tolist() == [np.float32(1 / 3 - 0.5), np.float32(2 / 3 - 0.5), 0.5]


def test_cpu_tensors_are_refused_and_the_entries_are_in_the_abi():
    from commonscenes_amd import lib, shape_metrics as SM
    c = torch.zeros(2, 8, 3)
    for call in (lambda: SM.pairwise_cd(c, c), lambda: SM.pairwise_emd(c, c), lambda: SM.compute_all_metrics(c, c, 50),
                 lambda: SM.jsd_between_point_cloud_sets(c, c), lambda: SM.EMD_CD(c, c, 50)):
        with pytest.raises(lib.CsError):
            call()
    dll = lib.load()
    for name in ("cs_chamfer_pairwise", "cs_emd_pairwise_cost", "cs_occupancy_histogram"):
        assert name in lib.SIGNATURES and hasattr(dll, name)
    # argument checks come before any device work
    assert dll.cs_emd_pairwise_cost(1, 1, 1, 1, 1, 8193, 8193, None) == lib.CS_EINVAL
    assert dll.cs_chamfer_pairwise(1, 2, 1, 2, 2, 8, 8, 1, None) == lib.CS_EINVAL       # symmetric needs a == b
    assert dll.cs_chamfer_pairwise(1, 1, 1, 1, 1, 8, 32769, 0, None) == lib.CS_EINVAL
