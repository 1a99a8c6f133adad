"""VQ-VAE encode side on the MI355X: VQVAE.encode_no_quant / encode / forward against the reference's outputs
(tests/golden/vq_encode.npz, tools/make_goldens.py --only vq_encode), the new kernels and the stride-2 Downsample route
against fp64 at full size (batch 16), batch invariance, and the F16X3 range rule."""
import warnings
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, rel_l2, vq_flip_report

pytestmark = pytest.mark.gpu

MODES = ["fp32", "f16x3"]
_CACHE = {}


def _sd():
    from commonscenes_amd import synth
    from commonscenes_amd.vqvae import vqvae_encoder_param_shapes, vqvae_param_shapes
    from oracle.ref_torch import VQ_FULL
    dd = dict(VQ_FULL, in_channels=1, double_z=False)
    table = OrderedDict(list(vqvae_encoder_param_shapes(dd, 8192, 3).items()) +
                        list(vqvae_param_shapes(dd, 8192, 3).items()))
    return synth.synth_state_dict(table, device="cuda"), dd


def _vq(mode="f16x3", sd=None):
    from commonscenes_amd.vqvae import VQVAE
    sd0, dd = _sd()
    return VQVAE(dd, 8192, 3, device="cuda").load_state_dict(sd if sd is not None else sd0).set_math(mode)


def _x():
    from commonscenes_amd import synth
    return torch.cat([synth.sdf_volume(0), synth.sdf_volume(1)], dim=0).cuda()


@pytest.mark.parametrize("mode", MODES)
def test_encode_matches_the_reference(mode):
    g = np.load(GOLDEN / "vq_encode.npz")
    vq = _vq(mode)
    x = _x()
    h = vq.encode_no_quant(x)
    quant, emb_loss, info = vq.encode(x)
    idx = info[2]
    torch.cuda.synchronize()
    h_ref, q_ref, i_ref = (torch.from_numpy(g[k]) for k in ("h", "quant", "indices"))
    e_h = rel_l2(h, h_ref)
    assert idx.dtype == torch.int64 and tuple(idx.shape) == (2 * 4096,) and info[0] is None and info[1] is None
    flips, unexplained = vq_flip_report(h, h_ref, idx, i_ref, vq.state_dict()["quantize.embedding.weight"])
    print(f"[{mode}] encode_no_quant rel-L2 {e_h:.2e}, index flips {flips} (unexplained {unexplained})")
    assert e_h <= 1e-5
    assert unexplained == 0
    same = bool(torch.equal(idx.cpu(), i_ref))
    if same:
        assert rel_l2(quant, q_ref) <= 1e-5
        assert abs(float(emb_loss) - float(g["emb_loss"][0])) <= 1e-5 * abs(float(g["emb_loss"][0]))
    assert emb_loss.dtype == torch.float32 and emb_loss.dim() == 0
    # forward: all four branches of network.py:123-140
    z = vq(x, forward_no_quant=True, encode_only=True)
    assert torch.equal(z, h)
    dec_nq, z2 = vq(x, forward_no_quant=True)
    assert torch.equal(z2, h) and dec_nq.shape == (2, 1, 64, 64, 64)
    dec, diff = vq(x)
    assert torch.equal(diff, emb_loss)
    if same:
        e_d = rel_l2(dec[:, :, :32, :32, :32], torch.from_numpy(g["dec_crop"]))
        e_n = abs(float(dec.double().norm()) - float(g["dec_norm"])) / float(g["dec_norm"])
        print(f"[{mode}] forward(x) reconstruction crop rel-L2 {e_d:.2e}, norm {e_n:.2e}")
        assert e_d <= 1e-4 and e_n <= 1e-4
        assert torch.equal(dec_nq, dec) or rel_l2(dec_nq, dec) <= 1e-5       # nearest code vs straight-through value
    dv, qv, lv, iv = vq(x, verbose=True)
    assert torch.equal(dv, dec) and torch.equal(qv, quant) and torch.equal(lv, emb_loss) and torch.equal(iv[2], idx)


def _pick(rs, dims, n=4096):
    return np.stack([rs.randint(0, d, n) for d in dims], 1)


def _conv_points_fp64(x64, w64, b64, pick, stride, pad_lo):
    """fp64 Conv3d(3) at the picked points [n, d, h, w, co] of x64 [nb, D, H, W, C] zero-padded by (pad_lo, 1 + ...):
    plain torch gathers + an einsum, no kernel of this package."""
    nb, D, H, W, C = x64.shape
    xp = torch.zeros((nb, D + 2, H + 2, W + 2, C), dtype=torch.float64, device=x64.device)
    xp[:, pad_lo:pad_lo + D, pad_lo:pad_lo + H, pad_lo:pad_lo + W] = x64
    p = torch.from_numpy(pick).to(x64.device)
    k = torch.arange(3, device=x64.device)
    n = p[:, 0][:, None, None, None]
    d = (p[:, 1] * stride)[:, None, None, None] + k[None, :, None, None]
    h = (p[:, 2] * stride)[:, None, None, None] + k[None, None, :, None]
    w = (p[:, 3] * stride)[:, None, None, None] + k[None, None, None, :]
    patch = xp[n, d, h, w]                                           # [P, 3, 3, 3, C]
    wsel = w64[p[:, 4]]                                              # [P, C, 3, 3, 3]
    return (torch.einsum("pdhwc,pcdhw->p", patch, wsel) + b64[p[:, 4]]).cpu().numpy()


def _at(out, pick):
    return out[tuple(torch.from_numpy(pick[:, j]).cuda() for j in range(pick.shape[1]))].double().cpu().numpy()


def _err(got, ref):
    return float(np.linalg.norm(got - ref) / np.linalg.norm(ref))


def test_conv_in_kernel_at_full_size_against_fp64():
    """cs_vqenc_conv_in at batch 16 (64^3, 1 -> 64): sampled outputs and one whole object against fp64; one kernel for
    both math modes."""
    from commonscenes_amd import ops, synth
    sd, _ = _sd()
    w, b = sd["encoder.conv_in.weight"], sd["encoder.conv_in.bias"]
    x = (synth.gaussian_like("enc:x", (16, 1, 64, 64, 64), scale=0.2)).cuda()
    y = ops.vqenc_conv_in(x, w, b)
    torch.cuda.synchronize()
    assert y.shape == (16, 64, 64, 64, 64)
    pick = _pick(np.random.RandomState(3), (16, 64, 64, 64, 64))
    ref = _conv_points_fp64(x.double().permute(0, 2, 3, 4, 1), w.double(), b.double(), pick, 1, 1)
    e = _err(_at(y, pick), ref)
    ref0 = F.conv3d(x[5:6].double().cpu(), w.double().cpu(), b.double().cpu(), padding=1).permute(0, 2, 3, 4, 1)
    e0 = rel_l2(y[5:6], ref0)
    print(f"conv_in batch 16: sampled rel-L2 {e:.2e}, object 5 whole {e0:.2e}")
    assert e <= 1e-6 and e0 <= 1e-6


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("level", [0, 1])
def test_downsample_conv_route_at_full_size_against_fp64(mode, level):
    """Downsample (F.pad(0, 1) + Conv3d stride 2, pad 0) as conv_gemm(pad=((0, 1),) * 3, stride 2) -- the generic gather
    (the slab / Winograd routes demand pad 1) -- at batch 16 on both encoder levels."""
    from commonscenes_amd import lib as L, ops, synth
    from commonscenes_amd.vqvae import _DOWN_PAD
    sd, _ = _sd()
    c, r = (64, 64) if level == 0 else (128, 32)
    wn = f"encoder.down.{level}.downsample.conv"
    w, b = sd[wn + ".weight"], sd[wn + ".bias"]
    x = synth.gaussian_like(f"enc:ds{level}", (16, r, r, r, c)).cuda()
    pw = ops.pack_weight(w, b, cin_pad=c, math=L.MATH_F16X3 if mode == "f16x3" else L.MATH_FP32)
    y = ops.conv_gemm(x, pw, stride=(2, 2, 2), pad=_DOWN_PAD)
    torch.cuda.synchronize()
    assert y.shape == (16, r // 2, r // 2, r // 2, c)
    pick = _pick(np.random.RandomState(7 + level), (16, r // 2, r // 2, r // 2, c))
    ref = _conv_points_fp64(x.double(), w.double(), b.double(), pick, 2, 0)
    e = _err(_at(y, pick), ref)
    # one whole object the reference's way: F.pad + F.conv3d (fp64, CPU)
    x1 = x[9:10].double().cpu().permute(0, 4, 1, 2, 3)
    ref1 = F.conv3d(F.pad(x1, (0, 1, 0, 1, 0, 1)), w.double().cpu(), b.double().cpu(), stride=2).permute(0, 2, 3, 4, 1)
    e1 = rel_l2(y[9:10], ref1)
    print(f"Downsample level {level} ({mode}) batch 16: sampled rel-L2 {e:.2e}, object 9 whole {e1:.2e}")
    # (level 1: K = 27 * 128 = 3456-term fp32 fma chains over zero-mean operands sit at ~1e-6 on rounding alone -- measured
    # 1.02e-6 in fp32 mode, the level-0 conv (K = 1728) at 7.7e-7; the gate follows the chain length)
    gate = 1e-6 if level == 0 else 1.5e-6
    assert e <= gate and e1 <= gate


def test_quantize_st_kernel():
    """cs_vq_quantize_st at batch 16 x 4096 rows: indices == cs_vq_argmin_lookup's bit for bit, the straight-through value
    z + (z_q - z) as torch forms it in fp32, per-object loss sums == an fp64 sum, bit-reproducible, batch invariant."""
    from commonscenes_amd import ops, synth
    sd, _ = _sd()
    cb = sd["quantize.embedding.weight"]
    z = torch.zeros((16, 16, 16, 16, 4), device="cuda")
    z[..., :3] = synth.gaussian_like("enc:z", (16, 16, 16, 16, 3), scale=0.8).cuda()
    idx, zst, loss = ops.vq_quantize_st(z, cb, 16)
    idx_l, zq_l = ops.vq_lookup(z, cb)
    torch.cuda.synchronize()
    assert torch.equal(idx, idx_l)
    zq = cb[idx].view(16, 16, 16, 16, 3)
    z3 = z[..., :3]
    assert torch.equal(zst[..., :3], z3 + (zq - z3)) and torch.equal(zst[..., 3], torch.zeros_like(zst[..., 3]))
    ref = ((zq - z3).double() ** 2).reshape(16, -1).sum(1)
    assert loss.dtype == torch.float64 and float(((loss - ref).abs() / ref).max()) <= 1e-12
    _, _, loss2 = ops.vq_quantize_st(z, cb, 16)
    _, _, loss1 = ops.vq_quantize_st(z[3:4].contiguous(), cb, 1)
    assert torch.equal(loss, loss2) and torch.equal(loss1[0], loss[3])


@pytest.mark.parametrize("mode", MODES)
def test_encode_batch_invariance(mode):
    """object 1 of a batch of 3 == the same object alone; a batch of 17 (> MAX_ENCODE_BATCH) == its slices -- bitwise."""
    from commonscenes_amd import synth
    vq = _vq(mode)
    x = _x()
    x3 = torch.cat([x, synth.sdf_volume(0).cuda().flip(2)], dim=0)
    q3, _, i3 = vq.encode(x3)
    q1, _, i1 = vq.encode(x3[1:2])
    assert torch.equal(q3[1], q1[0]) and torch.equal(i3[2][4096:8192], i1[2])
    assert torch.equal(vq.encode_no_quant(x3)[1], vq.encode_no_quant(x3[1:2])[0])
    x17 = x3.repeat(6, 1, 1, 1, 1)[:17]
    assert vq.MAX_ENCODE_BATCH == 16
    h17 = vq.encode_no_quant(x17)
    h16, h1 = vq.encode_no_quant(x17[:16]), vq.encode_no_quant(x17[16:])
    assert torch.equal(h17, torch.cat([h16, h1]))
    q17, l17, i17 = vq.encode(x17)
    assert torch.equal(i17[2][:16 * 4096], vq.encode(x17[:16])[2][2])


def test_overflow_policy():
    """A stress checkpoint (conv_in bias x 1e5: the raw residual stream the nin_shortcut and Downsample read leaves the
    F16X3 operand range): policy 'fp32' re-runs on fp32-packed weights == the fp32-mode encode bit for bit; 'raise'
    raises CsOverflowError."""
    from commonscenes_amd import lib as L
    sd, _ = _sd()
    sd["encoder.conv_in.bias"] = sd["encoder.conv_in.bias"] * 1e5
    x = _x()
    ref = _vq("fp32", sd).encode_no_quant(x)
    vq = _vq("f16x3", sd)
    vq.overflow_policy = "fp32"
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        h = vq.encode_no_quant(x)
    assert any("overflow" in str(r.message) for r in rec)
    assert torch.equal(h, ref)
    assert vq.math == L.MATH_F16X3          # the model itself stays on F16X3
    vq.overflow_policy = "raise"
    with pytest.raises(L.CsOverflowError):
        vq.encode_no_quant(x)
