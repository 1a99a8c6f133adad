"""Held-out checkpoint evaluation, host side (no GPU): the schedule tables of SDFusionText2ShapeModel.register_schedule
against the reference's (tests/golden/eval_losses.npz, tools/make_goldens.py --only eval_losses), the constants of
init_diffusion_params, the two C entries' argument checks, and the iou / VQLoss arithmetic on hand-made counts."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import GOLDEN

NEW_TABLES = ("log_one_minus_alphas_cumprod", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod",
              "posterior_variance", "posterior_log_variance_clipped", "posterior_mean_coef1", "posterior_mean_coef2",
              "lvlb_weights")
OLD_TABLES = ("betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod")


def _bare_model():
    """the schedule needs none of the networks: run init_diffusion_params on an instance that skipped __init__"""
    from commonscenes_amd.sdfusion import SDFusionText2ShapeModel
    from oracle.ref_torch import DIFFUSION
    m = SDFusionText2ShapeModel.__new__(SDFusionText2ShapeModel)
    m.init_diffusion_params(uc_scale=3., df_model_params=SimpleNamespace(**DIFFUSION))
    return m


def test_schedule_tables_equal_the_reference_bit_for_bit():
    g = np.load(GOLDEN / "eval_losses.npz")
    m = _bare_model()
    for k in NEW_TABLES + OLD_TABLES + ("logvar",):
        mine, ref = getattr(m, k), torch.from_numpy(g["tab_" + k])
        assert mine.dtype == torch.float32 and mine.shape == (1000,), k
        assert torch.equal(mine, ref), f"{k}: {int((mine != ref).sum())} entries differ"
    assert float(m.lvlb_weights[0]) == float(m.lvlb_weights[1])
    assert float(m.posterior_variance[0]) == 0.0 and float(m.posterior_log_variance_clipped[0]) == float(np.float32(np.log(1e-20)))


def test_init_diffusion_params_sets_the_constants():
    g = np.load(GOLDEN / "eval_losses.npz")
    m = _bare_model()
    assert m.learn_logvar is False and m.v_posterior == 0. and m.original_elbo_weight == 0. and m.l_simple_weight == 1.
    assert [float(m.learn_logvar), m.v_posterior, m.original_elbo_weight, m.l_simple_weight] == list(g["consts"])
    assert m.parameterization == "eps" and m.num_timesteps == 1000
    assert m.logvar.shape == (1000,) and not m.logvar.any()


def test_x0_parameterisation_is_not_shipped():
    m = _bare_model()
    m.parameterization = "x0"
    with pytest.raises(NotImplementedError):
        m.p_losses(torch.zeros(1, 3, 16, 16, 16), torch.zeros(1, 1, 1280), torch.zeros(1, dtype=torch.long))
    with pytest.raises(NotImplementedError):
        m.denoising_loss_table(torch.zeros(1, 3, 16, 16, 16), torch.zeros(1, 1, 1280), [1], encoded=True)
    with pytest.raises(NotImplementedError):
        m.register_schedule()
    with pytest.raises(NotImplementedError):
        m.switch_train()


def _aligned(n_floats):
    buf = (C.c_float * (n_floats + 16))()
    base = C.addressof(buf)
    return buf, base + (-base) % 64


def test_library_exports_the_two_entries_and_rejects_bad_arguments_without_a_device_call():
    from commonscenes_amd import lib
    dll = lib.load()
    assert "cs_q_sample" in lib.SIGNATURES and "cs_pair_stats" in lib.SIGNATURES
    assert hasattr(dll, "cs_q_sample") and hasattr(dll, "cs_pair_stats")
    keep, p = _aligned(64)            # a host address: every call below must return before any launch
    E = lib.CS_EINVAL
    q = lambda **kw: dll.cs_q_sample(*[{**dict(x0=p, noise=p, out=p, t=p, sa=p, s1=p, src=None, nsrc=None, rows=2, per=8, T=10,
                                               x0_rows=2, noise_rows=2, stream=None), **kw}[k]
                                       for k in ("x0", "noise", "out", "t", "sa", "s1", "src", "nsrc", "rows", "per", "T",
                                                 "x0_rows", "noise_rows", "stream")])
    for bad in (dict(x0=None), dict(noise=None), dict(out=None), dict(t=None), dict(sa=None), dict(s1=None), dict(rows=0),
                dict(per=0), dict(per=-4), dict(T=0), dict(T=-1), dict(x0_rows=0), dict(noise_rows=0),
                dict(x0_rows=1), dict(noise_rows=1)):          # (the last two: an identity map over too few source rows)
        assert q(**bad) == E, bad
    s = lambda **kw: dll.cs_pair_stats(*[{**dict(a=p, b=p, nb=2, per=8, lda=8, ldb=8, sums=p, counts=p, thr_a=0.0, thr_b=0.0,
                                                 ws=p, ws_bytes=64, stream=None), **kw}[k]
                                         for k in ("a", "b", "nb", "per", "lda", "ldb", "sums", "counts", "thr_a", "thr_b", "ws",
                                                   "ws_bytes", "stream")])
    for bad in (dict(a=None), dict(b=None), dict(ws=None), dict(sums=None, counts=None), dict(nb=0), dict(per=0), dict(per=-1),
                dict(lda=7), dict(ldb=4), dict(a=p + 2)):
        assert s(**bad) == E, bad
    assert s(ws_bytes=63) == lib.CS_ENOMEM and s(per=lib.PAIR_CHUNK + 1, lda=4096, ldb=4096, ws_bytes=127) == lib.CS_ENOMEM
    assert (lib.PAIR_CHUNK, lib.PAIR_PARTIAL_BYTES) == (2048, 32)
    txt = (GOLDEN.parent.parent / "include" / "commonscenes_hip.h").read_text()
    assert "#define CS_PAIR_CHUNK 2048" in txt and "#define CS_PAIR_PARTIAL_BYTES 32" in txt
    del keep


def test_ops_wrappers_refuse_cpu_tensors():
    from commonscenes_amd import lib, ops
    z = torch.zeros(2, 8)
    with pytest.raises(lib.CsError):
        ops.q_sample(z, z, torch.zeros(2, dtype=torch.long), torch.ones(4), torch.ones(4))
    with pytest.raises(lib.CsError):
        ops.pair_stats(z, z)


def test_iou_arithmetic_on_hand_made_counts():
    from commonscenes_amd.vqvae_model import iou_from_counts
    counts = torch.tensor([[4248, 122160], [0, 0], [5, 5], [0, 7], [16777217, 16777219]], dtype=torch.int64)
    v = iou_from_counts(counts)
    assert v.dtype == torch.float32 and v.shape == (5,)
    want = [np.float32(4248) / np.float32(122160), np.float32(0), np.float32(1), np.float32(0),
            np.float32(16777217) / np.float32(16777219)]
    assert [float(x) for x in v] == [float(w) for w in want]
    # the reference's expression on the same counts (int64 / (int64 + python float)): the same values
    ref = counts[:, 0] / (counts[:, 1] + 1e-12)
    assert torch.equal(v, ref)
    g = np.load(GOLDEN / "eval_losses.npz")
    for k in range(3):          # fixture (c): the reference's own counts give the reference's own values, empty union included
        assert torch.equal(iou_from_counts(torch.from_numpy(g["case_counts"][k])), torch.from_numpy(g["case_iou"][k]))
    assert torch.equal(iou_from_counts(torch.stack([torch.from_numpy(g["vq_inter"][0]), torch.from_numpy(g["vq_union"][0])], 1)),
                       torch.from_numpy(g["vq_iou"][0]))


def test_vqloss_arithmetic():
    from commonscenes_amd.vqvae_model import VQLoss
    cb = torch.tensor(0.375, dtype=torch.float32)
    loss, log = VQLoss(codebook_weight=0.5).from_sums(cb, torch.tensor([3.0, 5.0], dtype=torch.float64), 64)
    assert sorted(log) == ["loss_codebook", "loss_nll", "loss_rec", "loss_total"]
    assert all(v.dtype == torch.float32 and v.dim() == 0 for v in log.values()) and loss.dtype == torch.float32
    assert float(log["loss_rec"]) == float(log["loss_nll"]) == 0.125
    assert float(log["loss_codebook"]) == 0.375 and float(loss) == float(log["loss_total"]) == 0.125 + 0.5 * 0.375
