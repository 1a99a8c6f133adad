"""Shape completion on the MI355X: cs_ddim_masked_blend bit for bit against torch's CPU ops, the masked DDIM trajectory and
SDFusionText2ShapeModel.shape_comp against the reference's values (tests/golden/shape_comp*.npz, tools/make_goldens.py --only
shape_comp), and the invariants of the masked sampler on the reduced-width model."""
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
MODES = ["f16x3", "fp32"]          # the default math mode first
GATE = 1e-4          # the project's k-step DDIM latent gate and its SDF gate (tests/test_model_gpu.py)
_CACHE = {}


def _g(name="shape_comp"):
    if name not in _CACHE:
        _CACHE[name] = dict(np.load(GOLDEN / f"{name}.npz"))
    return _CACHE[name]


def _volume_chk(v):
    d = v.detach().double().cpu().flatten()
    w = (torch.arange(d.numel(), dtype=torch.float64) % 251.0) + 1.0
    return np.array([float(d.sum()), float(d.abs().sum()), float((d * w).sum())], np.float64)


def _chk_ok(v, want):
    """the input rebuilt here is the one the fixture was made from (fp64 sums; the summation order is the host's own)"""
    tol = 1e-12 * abs(want[1]) * np.array([1.0, 1.0, 251.0])
    return bool((np.abs(_volume_chk(v) - want) <= tol).all())


def _tables():
    """sqrt_alphas_cumprod / sqrt_one_minus_alphas_cumprod of the shipped schedule (the reference's own, from eval_losses.npz)"""
    if "tab" not in _CACHE:
        g = np.load(GOLDEN / "eval_losses.npz")
        _CACHE["tab"] = (torch.from_numpy(g["tab_sqrt_alphas_cumprod"]), torch.from_numpy(g["tab_sqrt_one_minus_alphas_cumprod"]))
    return _CACHE["tab"]


def _rand(shape, seed, scale=1.0):
    gen = torch.Generator()
    gen.manual_seed(seed)
    return torch.randn(shape, generator=gen, dtype=torch.float32) * scale


# ---------------------------------------------------------------------------------------------------------------------
# cs_ddim_masked_blend
# ---------------------------------------------------------------------------------------------------------------------
def _blend_ref(img, x0, mask, noise, t, sa, s1, src=None, msrc=None):
    """torch's CPU ops, one rounding each: q_sample's three (sdfusion_txt2shape_model.py:271-272), then ddim.py:161's four"""
    bc = (-1,) + (1,) * (img.dim() - 1)
    xs = x0 if src is None else x0[src.long()]
    ms = mask if msrc is None else mask[msrc.long()]
    q = sa[t].view(bc) * xs + s1[t].view(bc) * noise
    return q * ms + (1. - ms) * img


def _off(v, k):
    """the same values at a base address k floats past a 16-byte boundary"""
    buf = torch.empty(v.numel() + 4, dtype=v.dtype, device=v.device)
    out = buf[k:k + v.numel()].view(v.shape)
    out.copy_(v)
    assert out.data_ptr() % 16 == 4 * k
    return out


@pytest.mark.parametrize("rows,C_,inner", [(1, 3, 1), (3, 3, 5), (2, 3, 85), (5, 1, 257), (2, 3, 4096)])
def test_masked_blend_equals_torchs_cpu_ops_bit_for_bit(rows, C_, inner):
    from commonscenes_amd import ops
    sa, s1 = _tables()
    sad, s1d = sa.cuda(), s1.cuda()
    T = sa.numel()
    t = torch.tensor([T - 1, 0, 500, 1, 731][:rows], dtype=torch.int64)
    img, noise = _rand((rows, C_, inner), 1), _rand((rows, C_, inner), 2)
    x0 = _rand((rows, C_, inner), 3, 0.8)
    x3 = _rand((3, C_, inner), 4, 0.8)                     # three source rows, repeated and permuted through the maps
    src = torch.tensor([2, 0, 2, 1, 0][:rows], dtype=torch.int32)
    msrc = torch.tensor([1, 1, 0, 1, 0][:rows], dtype=torch.int32)
    n = 0
    for MC in sorted({1, C_}):
        pattern = (torch.arange(inner) % 3 == 0).float().expand(rows, MC, inner).contiguous()
        masks = {"zero": torch.zeros(rows, MC, inner), "one": torch.ones(rows, MC, inner),
                 "quarter": torch.full((rows, MC, inner), 0.25), "random": torch.rand((rows, MC, inner), generator=torch.Generator().manual_seed(5)),
                 "binary": pattern}
        for name, m in masks.items():
            ref = _blend_ref(img, x0, m, noise, t, sa, s1)
            out = ops.masked_blend(img.cuda(), x0.cuda(), m.cuda(), noise.cuda(), t.cuda(), sad, s1d)
            assert out.shape == img.shape and torch.equal(out.cpu(), ref), (MC, name)
            if name == "zero":
                assert torch.equal(out.cpu(), img), MC                                  # mask == 0 returns img exactly
            if name == "one":                                                           # mask == 1 returns q_sample exactly
                q = ops.q_sample(x0.cuda(), noise.cuda(), t.cuda(), sad, s1d)
                assert torch.equal(out, q), MC
            # in place: out aliases img
            buf = img.cuda()
            res = ops.masked_blend(buf, x0.cuda(), m.cuda(), noise.cuda(), t.cuda(), sad, s1d, out=buf)
            assert res.data_ptr() == buf.data_ptr() and torch.equal(buf.cpu(), ref), (MC, name, "in place")
            # through the row maps (two mask rows, three x0 rows), in place as the sampler runs it
            m2 = torch.stack([m[0], m[-1].flip(-1)])
            ref = _blend_ref(img, x3, m2, noise, t, sa, s1, src, msrc)
            buf = img.cuda()
            ops.masked_blend(buf, x3.cuda(), m2.cuda(), noise.cuda(), t.cuda(), sad, s1d, src=src.cuda(), msrc=msrc.cuda(),
                             out=buf)
            assert torch.equal(buf.cpu(), ref), (MC, name, "maps")
            out = ops.masked_blend(img.cuda(), x3.cuda(), m.cuda(), noise.cuda(), t.cuda(), sad, s1d, src=src.cuda())
            assert torch.equal(out.cpu(), _blend_ref(img, x3, m, noise, t, sa, s1, src)), (MC, name, "one map")
            n += 1
        # bases that are not 16-byte aligned (one array at a time, then all): the scalar route, the same bits
        m = masks["random"]
        ref = _blend_ref(img, x0, m, noise, t, sa, s1)
        for k in range(6):
            args = [img.cuda(), x0.cuda(), m.cuda(), noise.cuda()]
            for j in range(4):
                if k == j or k == 4:
                    args[j] = _off(args[j], 1 + j % 3)
            o = _off(torch.empty_like(args[0]), 3) if k >= 4 else None
            out = ops.masked_blend(*args, t.cuda(), sad, s1d, out=o)
            assert torch.equal(out.cpu(), ref), (MC, "unaligned", k)
    assert n == 5 * len({1, C_})
    torch.cuda.synchronize()


def test_masked_blend_rejects_bad_indices_on_the_host_with_device_tensors():
    from commonscenes_amd import lib, ops
    sa, s1 = (v.cuda() for v in _tables())
    img, noise, x0 = (_rand((4, 3, 8), s).cuda() for s in (1, 2, 3))
    m = torch.ones(4, 1, 8, device="cuda")
    t = torch.tensor([0, 1, 2, 999], device="cuda")
    ident = torch.arange(4, dtype=torch.int32, device="cuda")
    for bad in (dict(t=torch.tensor([0, 1, 2, 1000], device="cuda")), dict(t=torch.tensor([0, -1, 2, 3], device="cuda")),
                dict(src=torch.tensor([0, 1, 2, 4], dtype=torch.int32, device="cuda")),
                dict(msrc=torch.tensor([0, -1, 2, 3], dtype=torch.int32, device="cuda")),
                dict(src=ident[:3]), dict(msrc=ident.long())):
        with pytest.raises(lib.CsError):
            ops.masked_blend(img, x0, m, noise, bad.get("t", t), sa, s1, src=bad.get("src"), msrc=bad.get("msrc"))
    with pytest.raises(lib.CsError):                      # the output may alias img only
        ops.masked_blend(img, x0, m, noise, t, sa, s1, out=noise)
    with pytest.raises(lib.CsError):
        ops.masked_blend(img, x0, m, noise, t, sa, s1, out=x0)
    assert torch.equal(ops.masked_blend(img, x0, m, noise, t, sa, s1, src=ident, msrc=ident),
                       ops.masked_blend(img, x0, m, noise, t, sa, s1))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# the reduced-width model (UNet + the VQ-VAE with its encoder), one per module
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(tmp_path_factory):
    from commonscenes_amd import configs as K, synth
    from commonscenes_amd.sdfusion import SDFusionText2ShapeModel
    from commonscenes_amd.unet import unet_param_shapes
    from commonscenes_amd.vqvae import vqvae_encoder_param_shapes, vqvae_param_shapes
    cfg = K.reduced(K.UNET_CROSSATTN, 32)
    m = SDFusionText2ShapeModel(K.write_yaml_configs(tmp_path_factory.mktemp("shape_comp"), unet=cfg))
    dd = dict(K.VQVAE_DDCONFIG)
    table = OrderedDict(list(vqvae_encoder_param_shapes(dd, 8192, 3).items()) + list(vqvae_param_shapes(dd, 8192, 3).items()))
    m.load_state_dict({"df": synth.synth_state_dict(unet_param_shapes(cfg), device="cuda"),
                       "vqvae": synth.synth_state_dict(table, device="cuda")})
    return m


def _set_math(m, mode):
    m.df.set_math(mode)
    m.vqvae.set_math(mode)
    return m


def _traj_inputs():
    """fixture (b)'s inputs, rebuilt and checked against the checksums in the file"""
    if "traj" not in _CACHE:
        from commonscenes_amd import synth
        from commonscenes_amd.demo_util import get_partial_shape
        g, ga = _g("shape_comp_traj_x"), _g()
        x0 = synth.gaussian_like("shape_comp:x0", (2, 3, 16, 16, 16), scale=0.8)
        c = synth.gaussian_like("shape_comp:c", (2, 1, 1280))
        uc = synth.gaussian_like("shape_comp:uc", (2, 1, 1280))
        x_T = synth.gaussian_like("shape_comp:xT", (2, 3, 16, 16, 16))
        q = torch.stack([synth.gaussian_like(f"shape_comp:q{i}", (2, 3, 16, 16, 16)) for i in range(int(g["steps"]))])
        assert _chk_ok(x0, g["x0_chk"]) and _chk_ok(c, g["c_chk"]) and _chk_ok(uc, g["uc_chk"]) and _chk_ok(x_T, g["xT_chk"])
        assert all(_chk_ok(q[i], g["q_chk"][i]) for i in range(q.shape[0]))
        b = ga["boxes"][int(g["box"])]
        z_mask = get_partial_shape(torch.zeros(2, 1, 64, 64, 64), {"x": tuple(b[0]), "y": tuple(b[1]), "z": tuple(b[2])},
                                   z=x0)["z_mask"]
        assert float(z_mask.mean()) == 0.46875 and torch.equal(z_mask, torch.from_numpy(ga[f"z_mask_{int(g['box'])}"]))
        _CACHE["traj"] = dict(x0=x0, c=c.cuda(), uc=uc.cuda(), x_T=x_T, q=q, z_mask=z_mask)
    return _CACHE["traj"]


def _sample(m, i, S=6, **kw):
    from commonscenes_amd.ddim import DDIMSampler
    args = dict(S=S, batch_size=2, shape=(3, 16, 16, 16), conditioning=i["c"], x_T=i["x_T"], verbose=False,
                unconditional_guidance_scale=3.0, unconditional_conditioning=i["uc"], eta=0.0, log_every_t=1)
    args.update(kw)
    if hasattr(m.df, "reset_run_cache"):
        m.df.reset_run_cache()
    out = DDIMSampler(m).sample(**args)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("mode", MODES)
def test_masked_trajectory_against_the_reference(model, mode):
    """B = 2, S = 6 (7 steps), scale 3, eta 0, mean(mask) = 0.46875: every step's x and pred_x0 within the k-step DDIM latent
    gate (rel-L2 1e-4) of the reference's.  Measured on the MI355X (f16x3 / fp32): x 1.6e-6 .. 1.7e-6 / 1.8e-6 .. 2.0e-6,
    pred_x0 1.6e-6 .. 2.4e-6 / 1.9e-6 .. 2.8e-6 -- where the unmasked trajectories sit."""
    g, gp = _g("shape_comp_traj_x"), _g("shape_comp_traj_pred_x0")
    i = _traj_inputs()
    m = _set_math(model, mode)
    x0_before, q_before, mask_before = i["x0"].clone(), i["q"].clone(), i["z_mask"].clone()
    x, inter = _sample(m, i, x0=i["x0"], mask=i["z_mask"], q_noise=i["q"])
    xs, ps = inter["x_inter"], inter["pred_x0"]
    assert len(xs) == 8 and len(ps) == 8 and torch.equal(xs[-1], x)
    ex = [rel_l2(xs[k + 1], torch.from_numpy(g["x"][k])) for k in range(7)]
    ep = [rel_l2(ps[k + 1], torch.from_numpy(gp["pred_x0"][k])) for k in range(7)]
    print(f"[{mode}] masked trajectory rel-L2 per step: x {['%.2e' % v for v in ex]} pred_x0 {['%.2e' % v for v in ep]}")
    assert max(ex) <= GATE and max(ep) <= GATE
    # the inputs are the caller's: untouched (x_T is the first intermediate, not a buffer the loop blends into)
    assert torch.equal(i["x0"], x0_before) and torch.equal(i["q"], q_before) and torch.equal(i["z_mask"], mask_before)
    assert torch.equal(xs[0].cpu(), i["x_T"])
    # the known region is what the last step made of q_sample(x0, t_min): near x0, not x0 (the reference's own distance)
    known = float((x.cpu() - i["x0"]).abs()[i["z_mask"].expand(2, 3, 16, 16, 16) > 0].max())
    print(f"[{mode}] max |x - x0| over the known region {known:.4f} (reference {float(g['known_max_diff']):.4f})")
    assert abs(known - float(g["known_max_diff"])) <= 1e-3
    assert not any(m.fell_back.values())


def test_masked_sampler_invariants(model):
    m = _set_math(model, "f16x3")
    i = _traj_inputs()
    zeros, ones = torch.zeros_like(i["z_mask"]), torch.ones_like(i["z_mask"])
    # mask == 0: the unmasked run from the same x_T, bit for bit, at every step
    plain, pi = _sample(m, i)
    blank, bi = _sample(m, i, x0=i["x0"], mask=zeros, q_noise=i["q"])
    assert torch.equal(blank, plain)
    assert all(torch.equal(a, b) for a, b in zip(bi["x_inter"], pi["x_inter"]))
    assert all(torch.equal(a, b) for a, b in zip(bi["pred_x0"], pi["pred_x0"]))
    # mask == 1: nothing of x_T survives the first blend
    a, _ = _sample(m, i, x0=i["x0"], mask=ones, q_noise=i["q"])
    b, _ = _sample(m, i, x0=i["x0"], mask=ones, q_noise=i["q"], x_T=i["x_T"].flip(0) * 1.5)
    assert torch.equal(a, b) and not torch.equal(a, plain)
    # one shared x0 / mask row (the reference's broadcast) and explicit row maps address the same rows
    x1, m1 = i["x0"][:1], i["z_mask"][:1]
    c, _ = _sample(m, i, x0=x1, mask=m1, q_noise=i["q"])
    d, _ = _sample(m, i, x0=i["x0"].flip(0), mask=torch.cat([zeros[:1], m1]), q_noise=i["q"],
                   x0_src=torch.tensor([1, 1]), mask_src=torch.tensor([1, 1], dtype=torch.int32))
    assert torch.equal(c, d)
    # q_noise = None: drawn on the device, reproducible under torch.manual_seed, different under another seed
    torch.manual_seed(7)
    e, _ = _sample(m, i, S=2, x0=i["x0"], mask=i["z_mask"])
    torch.manual_seed(7)
    f, _ = _sample(m, i, S=2, x0=i["x0"], mask=i["z_mask"])
    torch.manual_seed(8)
    h, _ = _sample(m, i, S=2, x0=i["x0"], mask=i["z_mask"])
    assert torch.equal(e, f) and not torch.equal(e, h)
    # the graph-replay option is not taken with a mask: the same bits as the eager loop
    from commonscenes_amd.ddim import DDIMSampler
    s = DDIMSampler(m)
    s.use_graph = True
    k, _ = s.sample(S=6, batch_size=2, shape=(3, 16, 16, 16), conditioning=i["c"], x_T=i["x_T"], verbose=False,
                    unconditional_guidance_scale=3.0, unconditional_conditioning=i["uc"], eta=0.0, x0=i["x0"],
                    mask=i["z_mask"], q_noise=i["q"])
    ref, _ = _sample(m, i, x0=i["x0"], mask=i["z_mask"], q_noise=i["q"], log_every_t=100)
    assert torch.equal(k, ref)
    # ... and blending in place (steps whose x is not kept as an intermediate) gives the bits of the all-logged run
    full, fi = _sample(m, i, x0=i["x0"], mask=i["z_mask"], q_noise=i["q"])
    assert torch.equal(ref, full) and len(fi["x_inter"]) == 8
    with pytest.raises(AssertionError):
        _sample(m, i, mask=ones)


# ---------------------------------------------------------------------------------------------------------------------
# shape_comp
# ---------------------------------------------------------------------------------------------------------------------
def _e2e_inputs():
    if "e2e" not in _CACHE:
        from commonscenes_amd import synth
        g = _g()
        vol = torch.cat([synth.sdf_volume(0), synth.sdf_volume(1)], dim=0)
        c = synth.gaussian_like("shape_comp:e2e:c", (2, 1, 1280))
        uc = synth.gaussian_like("shape_comp:e2e:uc", (2, 1, 1280))
        x_T = synth.gaussian_like("shape_comp:e2e:xT", (4, 3, 16, 16, 16))
        q = torch.stack([synth.gaussian_like(f"shape_comp:e2e:q{i}", (4, 3, 16, 16, 16)) for i in range(int(g["e2e_steps"]))])
        assert _chk_ok(vol, g["vol_chk"]) and _chk_ok(c, g["e2e_c_chk"]) and _chk_ok(uc, g["e2e_uc_chk"])
        assert _chk_ok(x_T, g["e2e_xT_chk"]) and all(_chk_ok(q[i], g["e2e_q_chk"][i]) for i in range(q.shape[0]))
        b = g["e2e_box"]
        _CACHE["e2e"] = dict(vol=vol, c=c, uc=uc, x_T=x_T, q=q, box={"x": tuple(b[0]), "y": tuple(b[1]), "z": tuple(b[2])},
                             S=int(g["e2e_S"]), scale=float(g["e2e_scale"]))
    return _CACHE["e2e"]


def _comp(m, i, rows=None, ngen=2, **kw):
    """shape_comp on fixture (c)'s inputs; `rows`: the (object-major) output rows of the full call this call reproduces"""
    x_T, q = (i["x_T"], i["q"]) if rows is None else (i["x_T"][rows], i["q"][:, rows])
    out = m.shape_comp(kw.pop("vol", i["vol"]), i["box"], kw.pop("c", i["c"]), uc=kw.pop("uc", i["uc"]), ngen=ngen,
                       ddim_steps=i["S"], uc_scale=i["scale"], x_T=x_T, q_noise=q, return_latents=True, return_meta=True, **kw)
    torch.cuda.synchronize()
    return out


def _codes(m, lat):
    return m.vqvae.quantize(lat)[1].reshape(lat.shape[0], -1)


def _sdf_rows_agree(m, gen_a, lat_a, gen_b, idx_b):
    """the SDF gate between two of our own runs: rows decoded from the same code indices agree within 1e-4 (decode_no_quant
    quantises, so a latent that moved by fp32 summation order may sit on the other side of a codebook near-tie: such a row is
    reported, and its latent is gated by the caller)"""
    idx_a = _codes(m, lat_a)
    flipped = [r for r in range(gen_a.shape[0]) if not torch.equal(idx_a[r], idx_b[r])]
    if flipped:
        print(f"rows whose code indices differ between the two runs: {flipped}")
    assert len(flipped) <= 1
    for r in range(gen_a.shape[0]):
        if r not in flipped:
            assert rel_l2(gen_a[r], gen_b[r]) <= GATE, r


@pytest.mark.parametrize("mode", MODES)
def test_shape_comp_against_the_reference(model, mode):
    """Two analytic volumes x two completions, 4 masked steps, decode: latents within 1e-4 of the reference's, every SDF within
    1e-4 given equal code indices (decode_no_quant quantises: flips are accounted voxel by voxel as in tests/test_model_gpu.py,
    and an object with a flip is decoded from the reference's indices instead).  Measured on the MI355X (f16x3 / fp32): encoder
    latent 2.2e-6 / 3.3e-6, sampled latents 1.8e-6 / 2.1e-6, no flips, SDFs 2.5e-6 / 3.0e-6."""
    g, i = _g(), _e2e_inputs()
    m = _set_math(model, mode)
    m.launch_B = 32
    gen, lat, meta = _comp(m, i)
    assert gen.shape == (4, 1, 64, 64, 64) and lat.shape == (4, 3, 16, 16, 16) and gen.dtype == torch.float32
    assert meta["launch_sizes"] == [4] and meta["ngen"] == 2 and meta["masked_steps"] == 4 and not meta["any_fell_back"]
    assert m.gen_df is gen and m.last_latents is lat
    # the encoder's latent and the masks the sampler was given
    z = m.vqvae.encode_no_quant(i["vol"].cuda())
    e_z = rel_l2(z, torch.from_numpy(g["e2e_z"]))
    assert _chk_ok(m.x_part, g["e2e_part_chk"]) and _chk_ok(m.x_missing, g["e2e_missing_chk"])
    assert m.x_part.is_cuda and m.x_part.shape == (2, 1, 64, 64, 64)
    lat_ref = torch.from_numpy(g["e2e_latents"])
    e_lat = [rel_l2(lat[r], lat_ref[r]) for r in range(4)]
    print(f"[{mode}] shape_comp: encoder latent rel-L2 {e_z:.2e}; sampled latents rel-L2 per row {['%.2e' % v for v in e_lat]}")
    assert e_z <= 1e-5                                     # the encoder's own gate (tests/test_vq_encode_gpu.py)
    assert rel_l2(lat, lat_ref) <= GATE and max(e_lat) <= GATE
    vq = m.vqvae
    _, idx = vq.quantize(lat)
    cb = vq.state_dict()["quantize.embedding.weight"]
    idx_ref = torch.from_numpy(g["e2e_indices"])
    flips, unexplained = vq_flip_report(lat, lat_ref, idx.view(4, 16, 16, 16), idx_ref, cb)
    print(f"[{mode}] shape_comp: VQ code flips per row {flips} (of 4096 voxels each); unexplained {unexplained}")
    assert unexplained == 0 and sum(flips) <= 8
    sub, ref = gen[:, :, ::2, ::2, ::2], torch.from_numpy(g["e2e_gen_sdf_sub"])
    forced = None
    e_sdf = []
    for r in range(4):
        if flips[r] == 0:
            e_sdf.append(rel_l2(sub[r], ref[r]))
        else:
            if forced is None:
                quant = cb[idx_ref.reshape(-1).cuda()].view(4, 16, 16, 16, 3).permute(0, 4, 1, 2, 3).contiguous()
                forced = vq.decode(quant)
            e_sdf.append(rel_l2(forced[r, :, ::2, ::2, ::2], ref[r]))
    print(f"[{mode}] shape_comp: SDF rel-L2 per row {['%.2e' % v for v in e_sdf]}")
    assert max(e_sdf) <= GATE
    # object-major: rows 0-1 complete volume 0, rows 2-3 volume 1 -- swapping the objects swaps the row pairs
    order = [2, 3, 0, 1]
    idx_all = idx.reshape(4, -1)
    part = m.x_part.clone()
    gen_s, lat_s, _ = _comp(m, dict(i, x_T=i["x_T"][order], q=i["q"][:, order]), vol=i["vol"].flip(0), c=i["c"].flip(0),
                            uc=i["uc"].flip(0))
    same = torch.equal(lat_s, lat[order])
    print(f"[{mode}] objects swapped: latents rel-L2 to the swapped rows {rel_l2(lat_s, lat[order]):.2e} (bit-identical: {same})")
    assert rel_l2(lat_s, lat[order]) <= 1e-5 and rel_l2(lat_s, lat) > 1e-2
    _sdf_rows_agree(m, gen_s, lat_s, gen[order], idx_all[order])
    assert torch.equal(m.x_part, part.flip(0))


def test_shape_comp_rows_do_not_depend_on_ngen_or_on_the_slicing(model):
    i = _e2e_inputs()
    m = _set_math(model, "f16x3")
    m.launch_B = 32
    gen, lat, _ = _comp(m, i)
    idx = _codes(m, lat)
    # ngen = 2 rows of one object == two ngen = 1 calls given the matching q_noise / x_T rows
    for g_ in range(2):
        rows = [g_, 2 + g_]                                # completion g_ of object 0 and of object 1
        gen1, lat1, meta1 = _comp(m, i, rows=rows, ngen=1)
        d = [rel_l2(lat1[k], lat[rows[k]]) for k in range(2)]
        same = torch.equal(lat1, lat[rows])
        print(f"ngen=1 call {g_}: latents rel-L2 to the ngen=2 rows {['%.2e' % v for v in d]} (bit-identical: {same})")
        assert max(d) <= 1e-5
        _sdf_rows_agree(m, gen1, lat1, gen[rows], idx[rows])
        assert meta1["launch_sizes"] == [2] and meta1["ngen"] == 1
    # launch_B = 2: two slices of two rows; within 1e-5 of the single slice (the bound INTEGRATION states for a changed GEMM
    # plan), bit-identical where the plan is the same
    m.launch_B = 2
    try:
        gen2, lat2, meta2 = _comp(m, i)
    finally:
        m.launch_B = 32
    assert meta2["launch_sizes"] == [2, 2]
    d = rel_l2(lat2, lat)
    same = torch.equal(lat2, lat)
    print(f"launch_B = 2 (two slices) vs one slice: latents rel-L2 {d:.2e}; "
          f"{'same GEMM plan: bit-identical' if same else 'another GEMM plan: fp32 summation order'}")
    assert d <= 1e-5
    _sdf_rows_agree(m, gen2, lat2, gen, idx)
    # a 4-d input gains a batch axis; uc=None takes the embedding of the last set_input
    m.set_input({"sdf": i["vol"][:1], "rel": i["c"][:1], "uc": i["uc"][:1]})
    gen4, lat4 = m.shape_comp(i["vol"][0], i["box"], i["c"][:1], ngen=2, ddim_steps=i["S"], uc_scale=i["scale"],
                              x_T=i["x_T"][:2], q_noise=i["q"][:, :2], return_latents=True)
    assert gen4.shape == (2, 1, 64, 64, 64) and rel_l2(lat4, lat[:2]) <= 1e-5
    with pytest.raises(ValueError):
        m.shape_comp(i["vol"], i["box"], i["c"][:1], uc=i["uc"][:1])
    with pytest.raises(ValueError):
        m.shape_comp(i["vol"], i["box"], i["c"], uc=i["uc"], ddim_steps=i["S"], x_T=i["x_T"][:1])


def test_shape_comp_needs_the_encoder(tmp_path):
    """a decode-only checkpoint cannot complete shapes: the error encode_no_quant raises"""
    from commonscenes_amd import configs as K, synth
    from commonscenes_amd.sdfusion import SDFusionText2ShapeModel
    from commonscenes_amd.unet import unet_param_shapes
    from commonscenes_amd.vqvae import vqvae_param_shapes
    cfg = K.reduced(K.UNET_CROSSATTN, 32)
    m = SDFusionText2ShapeModel(K.write_yaml_configs(tmp_path, unet=cfg))
    m.load_state_dict({"df": synth.synth_state_dict(unet_param_shapes(cfg), device="cuda"),
                       "vqvae": synth.synth_state_dict(vqvae_param_shapes(dict(K.VQVAE_DDCONFIG), 8192, 3), device="cuda")})
    i = _e2e_inputs()
    with pytest.raises(RuntimeError, match="no encoder"):
        m.shape_comp(i["vol"], i["box"], i["c"], uc=i["uc"], ddim_steps=i["S"])


# ---------------------------------------------------------------------------------------------------------------------
# the operator's tool
# ---------------------------------------------------------------------------------------------------------------------
def test_complete_shape_tool_on_synthetic_weights(tmp_path):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "complete_shape.py"), "--synthetic", "--width", "32", "--steps", "6",
                        "--ngen", "2", "--step-rows", "2", "--obj", str(tmp_path / "obj")], capture_output=True, text=True,
                       env=env, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("COMPLETE_SHAPE ")]
    assert r.returncode == 0 and lines, r.stdout[-2000:] + r.stderr[-2000:]
    rep = json.loads(lines[-1][len("COMPLETE_SHAPE "):])
    assert rep["ok"] and rep["finite"] and rep["shapes"] == 2 and rep["ngen"] == 2 and rep["completions"] == 4
    assert rep["out_shape"] == [4, 1, 64, 64, 64] and rep["ddim_steps"] == 6 and rep["steps"] == 7 and rep["launch_sizes"] == [4]
    assert 0.0 < rep["known_fraction"] < 1.0
    assert rep["known_mean_abs_diff"] > 0.0 and rep["generated_mean_abs_diff"] > 0.0      # the known region is not copied back
    assert rep["ms_per_completion"] > 0 and rep["plain_step_ms"] > 0 and rep["masked_step_ms"] > 0 and rep["step_rows"] == 2
    assert not any(rep["fell_back"].values())
    assert sorted(p.name for p in (tmp_path / "obj").iterdir()) == ["obj0_gen0.obj", "obj0_gen1.obj", "obj1_gen0.obj",
                                                                    "obj1_gen1.obj"]
