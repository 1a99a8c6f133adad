"""VQ-VAE encode side, host-only parts: the encoder's state_dict table, what load_state_dict keeps, the C entries' argument
checks and the encode fixture (tests/test_vq_encode_gpu.py runs the encoder itself)."""
import ctypes as C
from collections import OrderedDict

import numpy as np
import pytest
import torch

from conftest import GOLDEN

from oracle.ref_torch import VQ_FULL


def _shapes():
    from commonscenes_amd.vqvae import vqvae_encoder_param_shapes, vqvae_param_shapes
    dd = dict(VQ_FULL, in_channels=1, double_z=False)
    return vqvae_encoder_param_shapes(dd, 8192, 3), vqvae_param_shapes(dd, 8192, 3), dd


def test_encoder_param_shapes_follow_encoder3d():
    enc, dec, _ = _shapes()
    keys = list(enc)
    assert keys[:2] == ["encoder.conv_in.weight", "encoder.conv_in.bias"]
    assert keys[-2:] == ["quant_conv.weight", "quant_conv.bias"]
    assert enc["encoder.conv_in.weight"] == (64, 1, 3, 3, 3)
    assert enc["encoder.down.0.block.0.conv1.weight"] == (64, 64, 3, 3, 3)
    assert "encoder.down.0.block.0.nin_shortcut.weight" not in enc
    assert enc["encoder.down.0.downsample.conv.weight"] == (64, 64, 3, 3, 3)
    assert enc["encoder.down.1.block.0.nin_shortcut.weight"] == (128, 64, 1, 1, 1)
    assert enc["encoder.down.1.downsample.conv.weight"] == (128, 128, 3, 3, 3)
    assert "encoder.down.2.downsample.conv.weight" not in enc
    assert enc["encoder.mid.attn_1.q.weight"] == (256, 256, 1, 1, 1)
    assert enc["encoder.norm_out.weight"] == (256,)
    assert enc["encoder.conv_out.weight"] == (3, 256, 3, 3, 3)
    assert enc["quant_conv.weight"] == (3, 3, 1, 1, 1)
    assert not set(enc) & set(dec)
    assert not any(k.startswith(("encoder.", "quant_conv.")) for k in dec)
    # every conv / norm is weight + bias: conv_in, 3 ResnetBlocks (4 each, +1 nin_shortcut in the two that widen),
    # 2 Downsample convs, 2 mid ResnetBlocks, the AttnBlock (norm + 4 convs), norm_out, conv_out, quant_conv
    assert len(enc) == 2 * (1 + 3 * 4 + 2 + 2 + 2 * 4 + 5 + 1 + 1 + 1)


def _sd(with_encoder=True):
    from commonscenes_amd import synth
    enc, dec, _ = _shapes()
    table = OrderedDict(list(enc.items()) + list(dec.items())) if with_encoder else dec
    return synth.synth_state_dict(table)


def _vq():
    from commonscenes_amd.vqvae import VQVAE
    _, _, dd = _shapes()
    return VQVAE(dd, 8192, 3, device="cpu")


def test_decode_only_dict_loads_strict_and_cannot_encode():
    vq = _vq()
    sd = _sd(with_encoder=False)
    vq.load_state_dict(sd, strict=True)
    assert list(vq.state_dict()) == list(sd)
    assert not vq.has_encoder
    x = torch.zeros(1, 1, 64, 64, 64)
    for call in (vq.encode_no_quant, vq.encode, vq, lambda t: vq(t, forward_no_quant=True, encode_only=True)):
        with pytest.raises(RuntimeError, match="encoder"):
            call(x)


def test_full_dict_keeps_the_encoder_and_round_trips():
    vq = _vq()
    sd = _sd(with_encoder=True)
    vq.load_state_dict(sd, strict=True)
    assert vq.has_encoder
    out = vq.state_dict()
    assert set(out) == set(sd)
    # the reference's order: encoder, decoder, quantize, quant_conv, post_quant_conv
    ks = list(out)
    assert ks[0].startswith("encoder.") and ks[-4:] == ["quant_conv.weight", "quant_conv.bias",
                                                         "post_quant_conv.weight", "post_quant_conv.bias"]
    for k in sd:
        assert torch.equal(out[k], sd[k]), k
    vq2 = _vq().load_state_dict(out, strict=True)
    assert vq2.has_encoder and list(vq2.state_dict()) == ks


def test_partial_encoder_set_is_ignored():
    vq = _vq()
    sd = _sd(with_encoder=False)
    sd["encoder.conv_in.weight"] = torch.zeros(64, 1, 3, 3, 3)
    vq.load_state_dict(sd, strict=True)
    assert not vq.has_encoder
    assert "encoder.conv_in.weight" not in vq.state_dict()


def test_wrong_encoder_shape_raises():
    vq = _vq()
    sd = _sd(with_encoder=True)
    sd["encoder.down.1.downsample.conv.weight"] = torch.zeros(128, 128, 3, 3, 1)
    with pytest.raises(RuntimeError, match="size mismatch"):
        vq.load_state_dict(sd, strict=True)
    assert not vq.has_encoder and not vq.state_dict()      # nothing half-loaded


def test_new_entries_check_arguments_first():
    from commonscenes_amd import lib
    dll = lib.load()
    assert dll.cs_vq_quantize_st(*([None] * 6), 0, 0, 0, 0, 0, 0, None) == lib.CS_EINVAL
    assert dll.cs_vqenc_conv_in(None, None, None, None, 0, 0, 0, 0, 0, 0, None) == lib.CS_EINVAL
    buf = (C.c_float * 64)()
    p = C.addressof(buf) + (-C.addressof(buf)) % 16
    # cout not a multiple of 4 / too wide, ldo short, edim 4: refused before any launch
    assert dll.cs_vqenc_conv_in(p, p, None, p, 1, 1, 1, 1, 6, 8, None) == lib.CS_EINVAL
    assert dll.cs_vqenc_conv_in(p, p, None, p, 1, 1, 1, 1, 512, 512, None) == lib.CS_EINVAL
    assert dll.cs_vqenc_conv_in(p, p, None, p, 1, 1, 1, 1, 8, 4, None) == lib.CS_EINVAL
    assert dll.cs_vq_quantize_st(p, p, p, p, p, p, 1, 1, 8, 4, 4, 4, None) == lib.CS_EINVAL
    assert dll.cs_vq_quantize_st(p, p, p, p, p, p, 1, 1, 16384, 3, 4, 4, None) == lib.CS_EINVAL   # codebook > LDS
    assert lib.VQ_ST_ROWS == 256


def test_conv_gemm_pad_keyword_is_refused_where_it_cannot_apply():
    from commonscenes_amd import lib, ops
    with pytest.raises(lib.CsError):
        ops.conv_gemm(torch.zeros(1, 4, 4, 4, 4), ops.PackedWeight(None, None, 4, 4, 4, 4, (3, 3, 3)),
                      pad=((0, 1), (0, 1), (0, 1)), stride=(2, 2, 2))      # (a CPU tensor: refused like every op)


def test_encode_fixture_is_small_and_its_input_is_rebuilt_exactly():
    from commonscenes_amd import synth
    f = GOLDEN / "vq_encode.npz"
    assert f.stat().st_size <= 1 << 20
    g = np.load(f)
    x = torch.cat([synth.sdf_volume(0), synth.sdf_volume(1)], dim=0)
    assert x.shape == (2, 1, 64, 64, 64) and float(x.abs().max()) <= 0.2 + 1e-6
    assert float(x.double().sum()) == float(g["x_sum"]) and float(x.double().abs().sum()) == float(g["x_abs_sum"])
    assert g["h"].shape == (2, 3, 16, 16, 16) and g["indices"].shape == (2 * 4096,)
    assert g["quant"].shape == g["h"].shape and g["emb_loss"].shape == (1,)
