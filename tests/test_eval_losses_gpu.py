"""Held-out checkpoint evaluation on the MI355X: cs_q_sample and cs_pair_stats piecewise (bit-exact against torch's three
ATen ops, <= 1e-12 against fp64 sums, exact counts, batch / position / layout independence), then p_losses,
denoising_loss_table, VQVAEModel.test_iou / eval_metrics and tools/eval_checkpoint.py against the reference's values
(tests/golden/eval_losses.npz, tools/make_goldens.py --only eval_losses)."""
import json
import os
import subprocess
import sys
from collections import OrderedDict
from pathlib import Path

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rel_l2, vq_flip_report

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
MODES = ["fp32", "f16x3"]
RHO = 1e-5          # the project's UNet-forward gate (rel-L2)
_CACHE = {}


def _g():
    if "g" not in _CACHE:
        _CACHE["g"] = dict(np.load(GOLDEN / "eval_losses.npz"))
    return _CACHE["g"]


def _chk_ok(v, want):
    """the input rebuilt here is the one the fixture was made from ({sum, sum of magnitudes} in fp64; the summation order is
    the host's own, hence not to the last bit)"""
    got = np.array([float(v.double().sum()), float(v.double().abs().sum())])
    return bool((np.abs(got - want) <= 1e-12 * np.abs(want[1])).all())


def _inputs_a():
    """golden (a)'s inputs, rebuilt and checked against the checksums in the file"""
    if "a" not in _CACHE:
        from commonscenes_amd import synth
        g = _g()
        x0 = synth.gaussian_like("eval:x0", (4, 3, 16, 16, 16), scale=0.8)
        noise = synth.gaussian_like("eval:noise", (4, 3, 16, 16, 16))
        cond = synth.gaussian_like("eval:c", (4, 1, 1280))
        assert _chk_ok(x0, g["x0_chk"]) and _chk_ok(noise, g["noise_chk"]) and _chk_ok(cond, g["cond_chk"])
        _CACHE["a"] = (x0.cuda(), noise.cuda(), cond.cuda(), torch.from_numpy(g["t"]).cuda())
    return _CACHE["a"]


def _tables():
    """sqrt_alphas_cumprod / sqrt_one_minus_alphas_cumprod on the device (== the golden's, tests/test_eval_losses_cpu.py)"""
    if "tab" not in _CACHE:
        g = _g()
        _CACHE["tab"] = (torch.from_numpy(g["tab_sqrt_alphas_cumprod"]).cuda(),
                         torch.from_numpy(g["tab_sqrt_one_minus_alphas_cumprod"]).cuda())
    return _CACHE["tab"]


def _rand(shape, seed, scale=1.0):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    return torch.randn(shape, generator=gen, device="cuda", dtype=torch.float32) * scale


# ---------------------------------------------------------------------------------------------------------------------
# cs_q_sample
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per", [1, 3, 12288, 12289])
@pytest.mark.parametrize("rows", [1, 5])
def test_q_sample_equals_torchs_three_ops_bit_for_bit(per, rows):
    from commonscenes_amd import ops
    sa, s1 = _tables()
    t = torch.tensor([0, 999, 500, 1, 731][:rows], dtype=torch.int64, device="cuda")
    x0, noise = _rand((rows, per), 1, 0.8), _rand((rows, per), 2)
    out = ops.q_sample(x0, noise, t, sa, s1)
    ref = sa[t][:, None] * x0 + s1[t][:, None] * noise
    assert out.shape == (rows, per) and torch.equal(out, ref)
    # row maps: three sources, repeated and permuted; the noise through another map
    x3, n2 = _rand((3, per), 3, 0.8), _rand((2, per), 4)
    src = torch.tensor([2, 0, 2, 1, 0][:rows], dtype=torch.int32, device="cuda")
    nsrc = torch.tensor([1, 1, 0, 1, 0][:rows], dtype=torch.int32, device="cuda")
    out = ops.q_sample(x3, n2, t, sa, s1, src=src, nsrc=nsrc)
    ref = sa[t][:, None] * x3[src.long()] + s1[t][:, None] * n2[nsrc.long()]
    assert torch.equal(out, ref)
    out = ops.q_sample(x3, noise, t, sa, s1, src=src)          # one map only
    assert torch.equal(out, sa[t][:, None] * x3[src.long()] + s1[t][:, None] * noise)


def test_q_sample_equals_the_reference_and_rejects_bad_indices_on_the_host():
    from commonscenes_amd import lib, ops
    g = _g()
    x0, noise, _, t = _inputs_a()
    sa, s1 = _tables()
    out = ops.q_sample(x0, noise, t, sa, s1)
    assert out.shape == x0.shape and torch.equal(out.cpu(), torch.from_numpy(g["x_noisy"]))
    ident = torch.arange(4, dtype=torch.int32, device="cuda")
    for bad in (dict(t=torch.tensor([0, 1, 2, 1000], device="cuda")), dict(t=torch.tensor([0, -1, 2, 3], device="cuda")),
                dict(src=torch.tensor([0, 1, 2, 4], dtype=torch.int32, device="cuda")),
                dict(nsrc=torch.tensor([0, -1, 2, 3], dtype=torch.int32, device="cuda")),
                dict(src=ident[:3]), dict(src=ident.long())):
        with pytest.raises(lib.CsError):
            ops.q_sample(x0, noise, bad.get("t", t), sa, s1, src=bad.get("src"), nsrc=bad.get("nsrc"))
    with pytest.raises(lib.CsError):          # five rows from four sources without a map
        ops.q_sample(x0, noise, torch.zeros(5, dtype=torch.int64, device="cuda"), sa, s1)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# cs_pair_stats
# ---------------------------------------------------------------------------------------------------------------------
def _pair_ref(a, b, thr_a, thr_b):
    d = (a - b).double()                                  # the fp32 difference, widened
    sums = torch.stack([(d * d).sum(1), d.abs().sum(1)], 1)
    oa, ob = ~(a > thr_a), ~(b > thr_b)
    counts = torch.stack([(oa & ob).sum(1), (oa | ob).sum(1)], 1)
    return sums, counts


@pytest.mark.parametrize("per", [1, 63, 64, 65, 12288, 262144, 262145])
def test_pair_stats_sums_and_counts(per):
    from commonscenes_amd import ops
    for nb in (1, 2, 7):
        a, b = _rand((nb, per), 10 + nb, 0.2), _rand((nb, per), 20 + nb, 0.2)
        sums, counts = ops.pair_stats(a, b, 0.0, 0.02)
        rs, rc = _pair_ref(a, b, 0.0, float(np.float32(0.02)))
        assert sums.dtype == torch.float64 and sums.shape == (nb, 2) and counts.dtype == torch.int64 and counts.shape == (nb, 2)
        err = float(((sums - rs).abs() / rs).max())
        assert err <= 1e-12, (nb, per, err)
        assert torch.equal(counts, rc), (nb, per)
        # either block alone, and twice: the same bits
        s_only, none = ops.pair_stats(a, b)
        none2, c_only = ops.pair_stats(a, b, 0.0, 0.02, want_sums=False)
        assert none is None and none2 is None and torch.equal(s_only, sums) and torch.equal(c_only, counts)
        sums2, counts2 = ops.pair_stats(a, b, 0.0, 0.02)
        assert torch.equal(sums2, sums) and torch.equal(counts2, counts)


@pytest.mark.parametrize("per", [65, 12288, 262145])
def test_pair_stats_does_not_depend_on_batch_position_or_layout(per):
    from commonscenes_amd import ops
    a, b = _rand((7, per), 31, 0.2), _rand((7, per), 32, 0.2)
    sums, counts = ops.pair_stats(a, b, 0.0, -0.05)
    for k in (0, 3, 6):                                  # alone
        s1, c1 = ops.pair_stats(a[k:k + 1].clone(), b[k:k + 1].clone(), 0.0, -0.05)
        assert torch.equal(s1[0], sums[k]) and torch.equal(c1[0], counts[k])
    # at another position of a larger batch
    a9 = torch.cat([_rand((2, per), 33, 0.2), a.flip(0)])
    b9 = torch.cat([_rand((2, per), 34, 0.2), b.flip(0)])
    s9, c9 = ops.pair_stats(a9, b9, 0.0, -0.05)
    assert torch.equal(s9[2:].flip(0), sums) and torch.equal(c9[2:].flip(0), counts)
    # ld views: rows of a wider buffer whose padding columns are poisoned -- a 16-byte-aligned stride and an odd one
    for pad in ((-per) % 4 + 4, (-per) % 4 + 3):
        wa = torch.full((7, per + pad), float("nan"), device="cuda")
        wb = torch.full((7, per + pad), -1e30, device="cuda")
        wa[:, :per], wb[:, :per] = a, b
        sv, cv = ops.pair_stats(wa[:, :per], wb[:, :per], 0.0, -0.05)
        assert torch.equal(sv, sums) and torch.equal(cv, counts), pad
        sv, cv = ops.pair_stats(wa[:, :per], b, 0.0, -0.05)          # mixed strides
        assert torch.equal(sv, sums) and torch.equal(cv, counts), pad


def test_pair_stats_counts_and_iou_on_the_reference_fixture():
    """fixture (c): a NaN voxel, a voxel exactly at the threshold, an empty union -- the counts equal torch's masks and the
    reference's, iou equals the reference's values bit for bit"""
    from commonscenes_amd import ops, synth
    from commonscenes_amd.vqvae_model import iou
    g = _g()
    for k, thr in enumerate(g["vq_thres"]):
        a, b = (v.cuda() for v in synth.iou_case(float(thr)))
        assert bool(torch.isnan(b[0]).sum() == 1) and float(b[0, 0, 40, 41, 42]) == float(np.float32(thr))
        _, counts = ops.pair_stats(a, b, 0.0, float(thr), want_sums=False)
        x_gt_mask, x_mask = a.clone(), b.clone()               # util.py:116-122, spelled out
        x_gt_mask[a > 0.0] = 0.
        x_gt_mask[a <= 0.0] = 1.
        x_mask[b > float(thr)] = 0.
        x_mask[b <= float(thr)] = 1.
        inter = torch.logical_and(x_gt_mask, x_mask).flatten(1).sum(1)
        union = torch.logical_or(x_gt_mask, x_mask).flatten(1).sum(1)
        assert torch.equal(counts, torch.stack([inter, union], 1))
        assert torch.equal(counts.cpu(), torch.from_numpy(g["case_counts"][k]))
        assert int(counts[2, 1]) == 0
        v = iou(a, b, float(thr))
        assert v.dtype == torch.float32 and torch.equal(v.cpu(), torch.from_numpy(g["case_iou"][k])) and float(v[2]) == 0.0
        sums, _ = ops.pair_stats(a, b)
        assert bool(torch.isnan(sums[0]).all()) and bool(torch.isfinite(sums[1:]).all())      # the NaN stays in its own sample


# ---------------------------------------------------------------------------------------------------------------------
# p_losses / denoising_loss_table on the reduced-width UNet
# ---------------------------------------------------------------------------------------------------------------------
def _model(tmp_path, mode, with_encoder=False):
    from commonscenes_amd import configs as K, synth
    from commonscenes_amd.sdfusion import SDFusionText2ShapeModel
    from commonscenes_amd.unet import unet_param_shapes
    from commonscenes_amd.vqvae import vqvae_encoder_param_shapes, vqvae_param_shapes
    cfg = K.reduced(K.UNET_CROSSATTN, 32)
    m = SDFusionText2ShapeModel(K.write_yaml_configs(tmp_path, unet=cfg))
    dd = dict(K.VQVAE_DDCONFIG)
    table = OrderedDict(vqvae_param_shapes(dd, 8192, 3))
    if with_encoder:
        table = OrderedDict(list(vqvae_encoder_param_shapes(dd, 8192, 3).items()) + list(table.items()))
    m.load_state_dict({"df": synth.synth_state_dict(unet_param_shapes(cfg), device="cuda"),
                       "vqvae": synth.synth_state_dict(table, device="cuda")})
    m.df.set_math(mode)
    m.vqvae.set_math(mode)
    return m


@pytest.mark.parametrize("mode", MODES)
def test_p_losses_against_the_reference(tmp_path, mode):
    """Measured on the MI355X (fp32 / f16x3): model output rel-L2 2.3e-6 / 2.0e-6, per-sample loss_simple within 9.3e-8 of the
    reference (bound 9.4e-6 .. 9.6e-6), loss_vlb 9.1e-8 / 1.8e-7.  The bounds: the UNet-forward gate
    rho = 1e-5 on the model output, and what it implies for a per-sample loss: ||eps' - n|| lies within (1 +- rho r) ||eps - n||
    with r = ||eps|| / ||eps - n||, so the mean square moves by at most 2 rho r + (rho r)^2 of itself."""
    g = _g()
    m = _model(tmp_path, mode)
    x0, noise, cond, t = _inputs_a()
    x_noisy, target, loss, ld = m.p_losses(x0, cond, t, noise=noise)
    torch.cuda.synchronize()
    assert torch.equal(x_noisy.cpu(), torch.from_numpy(g["x_noisy"])) and torch.equal(target, noise)
    e_out = rel_l2(m.last_model_output, torch.from_numpy(g["eps"]))
    r = g["r"]
    bound = 2 * RHO * r + (RHO * r) ** 2
    mine = m.get_loss(m.last_model_output, target, mean=False)
    ref = g["loss_simple_per_sample"]
    e_ls = np.abs(mine.cpu().numpy().astype(np.float64) - ref) / ref
    print(f"[{mode}] model output rel-L2 {e_out:.2e}; per-sample loss_simple rel err {e_ls} bound {bound} (r {r})")
    assert mine.dtype == torch.float32 and mine.shape == (4,)
    assert e_out <= RHO
    assert (e_ls <= bound).all()
    # the reduction alone: the reference's own model output through get_loss, against its fp32 value
    fed = m.get_loss(torch.from_numpy(g["eps"]).cuda(), target, mean=False).cpu().numpy().astype(np.float64)
    e_fed = np.abs(fed - ref) / ref
    print(f"[{mode}] get_loss on the reference's model output: rel err {e_fed}")
    assert (e_fed <= 1e-6).all()
    # the dict: the reference's keys, fp32 0-dim, the same bound (positive weights: a weighted mean moves by no more than
    # its worst term)
    assert sorted(ld) == list(g["loss_keys"]) == ["loss_simple", "loss_total", "loss_vlb"]
    for k, want in zip(g["loss_keys"], g["loss_vals"]):
        v = ld[str(k)]
        assert v.dtype == torch.float32 and v.dim() == 0
        e = abs(float(v) - float(want)) / float(want)
        print(f"[{mode}] {k}: {float(v):.8f} vs {float(want):.8f} rel err {e:.2e}")
        assert e <= bound.max()
    assert loss.dtype == torch.float32 and loss.dim() == 0 and float(loss) == float(ld["loss_total"])
    assert abs(float(loss) - float(g["loss"][0])) / float(g["loss"][0]) <= bound.max()
    # scalar forms of get_loss
    for lt in ("l2", "l1"):
        got = float(m.get_loss(m.last_model_output, target, loss_type=lt))
        d = (target - m.last_model_output).double()
        want = float((d * d).mean() if lt == "l2" else d.abs().mean())
        assert abs(got - want) <= 1e-6 * want
    with pytest.raises(NotImplementedError):
        m.get_loss(target, target, loss_type="huber")
    m.parameterization = "x0"
    with pytest.raises(NotImplementedError):
        m.p_losses(x0, cond, t, noise=noise)


@pytest.mark.parametrize("mode", MODES)
def test_denoising_loss_table_equals_separate_p_losses_calls(tmp_path, mode):
    m = _model(tmp_path, mode)
    x0, noise, cond, _ = _inputs_a()
    z, nz, c = x0[:2], noise[:2], cond[:2]
    ts = [1, 500, 999]
    want_ps, want_ls, want_vlb = [], [], []
    for tk in ts:
        _, target, _, ld = m.p_losses(z, c, torch.full((2,), tk, dtype=torch.int64, device="cuda"), noise=nz)
        want_ps.append(m.get_loss(m.last_model_output, target, mean=False).cpu())
        want_ls.append(ld["loss_simple"].cpu())
        want_vlb.append(ld["loss_vlb"].cpu())
    for batch in (4, 64):          # 4: rows 0-3 and 4-5 in two launches; 64: one launch of six
        tab, meta = m.denoising_loss_table(z, c, ts, noise=nz, batch=batch, encoded=True, return_meta=True)
        assert meta["launch_sizes"] == ([4, 2] if batch == 4 else [6]) and tab["fell_back"] == meta["fell_back"]
        assert not meta["any_fell_back"]
        ps = tab["per_sample"]
        assert ps.dtype == torch.float64 and ps.shape == (2, 3) and tab["timesteps"].tolist() == ts
        diff = [float((ps[:, k].to(torch.float32) - want_ps[k]).abs().max() / want_ps[k].abs().max()) for k in range(3)]
        print(f"[{mode}] batch {batch}: per-sample rel diff to separate p_losses calls {diff}")
        for k in range(3):
            assert torch.equal(ps[:, k].to(torch.float32), want_ps[k]), (batch, k)
            assert torch.equal(tab["loss_simple"][k], want_ls[k]) and torch.equal(tab["loss_vlb"][k], want_vlb[k])
    # noise per cell, and drawn from the seeded device generator: reproducible
    nk = torch.stack([nz, nz.flip(0), nz * 0.5], dim=1)
    t1 = m.denoising_loss_table(z, c, ts, noise=nk, batch=64, encoded=True)
    assert torch.equal(t1["per_sample"][:, 0], ps[:, 0]) and not torch.equal(t1["per_sample"][:, 1], ps[:, 1])
    s1, s2 = (m.denoising_loss_table(z, c, ts, seed=5, encoded=True)["per_sample"] for _ in range(2))
    assert torch.equal(s1, s2) and bool(torch.isfinite(s1).all())
    with pytest.raises(RuntimeError):          # SDFs need the encoder, and this checkpoint has none
        m.denoising_loss_table(torch.zeros(1, 1, 64, 64, 64, device="cuda"), c[:1], ts)
    with pytest.raises(ValueError):
        m.denoising_loss_table(z, c, [1000], noise=nz, encoded=True)


# ---------------------------------------------------------------------------------------------------------------------
# VQVAEModel
# ---------------------------------------------------------------------------------------------------------------------
def _vq(mode):
    from commonscenes_amd import synth
    from commonscenes_amd.vqvae import VQVAE, vqvae_encoder_param_shapes, vqvae_param_shapes
    from oracle.ref_torch import VQ_FULL
    dd = dict(VQ_FULL, in_channels=1, double_z=False)
    table = OrderedDict(list(vqvae_encoder_param_shapes(dd, 8192, 3).items()) + list(vqvae_param_shapes(dd, 8192, 3).items()))
    return VQVAE(dd, 8192, 3, device="cuda").load_state_dict(synth.synth_state_dict(table, device="cuda")).set_math(mode)


def _torch_iou(x, xr, thr):
    og, orr = ~(x > 0.0), ~(xr > thr)
    inter, union = (og & orr).flatten(1).sum(1), (og | orr).flatten(1).sum(1)
    return inter / (union + 1e-12), inter, union


@pytest.mark.parametrize("mode", MODES)
def test_vqvae_model_iou_and_losses_against_the_reference(mode):
    from commonscenes_amd import synth
    from commonscenes_amd.vqvae_model import VQLoss, VQVAEModel
    g = _g()
    ge = np.load(GOLDEN / "vq_encode.npz")
    vm = VQVAEModel(vqvae=_vq(mode), codebook_weight=float(g["vq_codebook_weight"]))
    x = torch.cat([synth.sdf_volume(0), synth.sdf_volume(1)], dim=0)
    assert _chk_ok(x, g["vq_x_chk"])
    data = {"sdf": x}
    for k, thr in enumerate(g["vq_thres"]):
        v = vm.test_iou(data, thres=float(thr))
        idx = vm.vqvae.last_indices
        want, inter, union = _torch_iou(vm.x, vm.x_recon, float(thr))
        assert v.dtype == torch.float32 and v.shape == (2,) and torch.equal(v, want)          # its own volumes: bit for bit
        same = torch.equal(idx.cpu(), torch.from_numpy(g["vq_indices"]))
        if k == 0:
            assert vm.x.is_cuda and vm.cur_bs == 2 and vm.z.shape == (2, 3, 16, 16, 16) and vm.x_recon.shape == x.shape
            flips, unexplained = vq_flip_report(vm.z, torch.from_numpy(ge["h"]), idx, torch.from_numpy(g["vq_indices"]),
                                                vm.vqvae.state_dict()["quantize.embedding.weight"])
            print(f"[{mode}] decode_no_quant index flips {flips} (unexplained {unexplained})")
            assert unexplained == 0
        di = (inter.cpu() - torch.from_numpy(g["vq_inter"][k])).abs()
        du = (union.cpu() - torch.from_numpy(g["vq_union"][k])).abs()
        print(f"[{mode}] thres {thr}: iou {v.tolist()} (reference {g['vq_iou'][k].tolist()}), |inter - ref| {di.tolist()}, "
              f"|union - ref| {du.tolist()}, n_near {g['vq_n_near'][k].tolist()}, same codes {same}")
        if same:
            n_near = torch.from_numpy(g["vq_n_near"][k])
            assert bool((di <= n_near).all()) and bool((du <= n_near).all())
    # forward() + VQLoss against the reference's log
    vm.set_input(data)
    vm.forward()
    _, log = vm.loss_vq(vm.qloss, vm.x, vm.x_recon)
    ref = {str(k): float(v) for k, v in zip(g["vq_log_keys"], g["vq_log_vals"])}
    assert sorted(log) == sorted(ref) and all(v.dtype == torch.float32 and v.dim() == 0 for v in log.values())
    same = torch.equal(vm.vqvae.last_indices.cpu(), torch.from_numpy(ge["indices"]))
    # dec's gate is rel-L2 <= 1e-4 (test_vq_encode_gpu.py): mean |x - dec| then moves by at most 1e-4 ||dec|| / sqrt(n);
    # emb_loss's gate is 1e-5 relative
    n = x.numel()
    rec_gate = 1e-4 * float(ge["dec_norm"]) / n ** 0.5
    e_rec = abs(float(log["loss_rec"]) - ref["loss_rec"])
    e_cb = abs(float(log["loss_codebook"]) - ref["loss_codebook"]) / ref["loss_codebook"]
    print(f"[{mode}] loss_rec {float(log['loss_rec']):.8f} (reference {ref['loss_rec']:.8f}, |diff| {e_rec:.2e}, gate "
          f"{rec_gate:.2e}); loss_codebook rel err {e_cb:.2e}; same codes {same}")
    if same:
        assert e_rec <= rec_gate and e_cb <= 1e-5
        assert abs(float(log["loss_total"]) - ref["loss_total"]) <= rec_gate + 1e-5 * ref["loss_codebook"] * vm.loss_vq.codebook_weight
    assert float(log["loss_nll"]) == float(log["loss_rec"])
    d = (vm.x - vm.x_recon).double().abs().mean()
    assert abs(float(log["loss_rec"]) - float(d)) <= 1e-6 * float(d)
    assert isinstance(vm.loss_vq, VQLoss)
    with pytest.raises(NotImplementedError):
        vm.switch_train()


def test_eval_metrics_over_a_two_batch_loader():
    from commonscenes_amd import synth
    from commonscenes_amd.vqvae_model import VQVAEModel
    vm = VQVAEModel(vqvae=_vq("f16x3"))
    v0, v1 = synth.sdf_volume(0), synth.sdf_volume(1)
    loader = [{"sdf": torch.cat([v0, v1])}, {"sdf": v0.flip(2)}]
    per, l1, cb = [], 0.0, 0.0
    for d in loader:
        per.append(vm.test_iou(d, thres=0.02))
        vm.forward()
        l1 += float((vm.x - vm.x_recon).double().abs().sum())
        cb += float(vm.qloss) * vm.cur_bs
    allv = torch.cat(per)
    met = vm.eval_metrics(loader, thres=0.02)
    assert list(met) == ["iou", "iou_std", "loss_rec", "loss_codebook"]
    assert all(v.dtype == torch.float32 and v.dim() == 0 for v in met.values())
    assert torch.equal(met["iou"], allv.mean()) and torch.equal(met["iou_std"], allv.std())
    v64 = allv.double().cpu().numpy()
    assert abs(float(met["iou"]) - v64.mean()) <= 1e-6 * v64.mean()
    assert abs(float(met["iou_std"]) - v64.std(ddof=1)) <= 1e-5 * v64.std(ddof=1)          # unbiased, over all three samples
    assert abs(float(met["loss_rec"]) - l1 / (3 * 64 ** 3)) <= 1e-6 * l1 / (3 * 64 ** 3)
    assert abs(float(met["loss_codebook"]) - cb / 3) <= 1e-6 * cb / 3


# ---------------------------------------------------------------------------------------------------------------------
# the operator's tool
# ---------------------------------------------------------------------------------------------------------------------
def test_eval_checkpoint_tool_on_synthetic_weights():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "eval_checkpoint.py"), "--synthetic", "--width", "32",
                        "--timesteps", "1,500,999"], capture_output=True, text=True, env=env, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("EVAL_CHECKPOINT ")]
    assert r.returncode == 0 and lines, r.stdout[-2000:] + r.stderr[-2000:]
    rep = json.loads(lines[-1][len("EVAL_CHECKPOINT "):])
    assert rep["ok"] and rep["finite"] and rep["shapes"] == 4 and rep["width"] == 32 and rep["timesteps"] == [1, 500, 999]
    assert len(rep["loss_simple"]) == 3 and len(rep["loss_vlb"]) == 3 and all(v > 0 for v in rep["loss_simple"])
    assert len(rep["per_sample"]) == 4 and len(rep["per_sample"][0]) == 3
    assert 0.0 <= rep["iou"] <= 1.0 and rep["iou_std"] >= 0.0 and rep["loss_rec"] > 0 and rep["loss_codebook"] > 0
    assert rep["shape_timesteps_per_s"] > 0 and rep["reconstructions_per_s"] > 0
    assert not any(rep["fell_back"].values())
