#!/usr/bin/env python
"""VQ-VAE encode: ms per object of encode_no_quant and of the forward(x) round trip (encode + decode) at 1 / 7 / 16 / 32
objects in both math modes, with FLOP/s from the layer table (encoder 271 GFLOP, decoder 723 GFLOP per object); then a
same-box A/B of conv_in: cs_vqenc_conv_in against the generic route (nchw_to_ndhwc(cpad=4) + cs_conv_gemm).
    python tools/encode_bench.py [--batches 1 7 16 32] [--iters 3]"""
import argparse, os, sys, time
from collections import OrderedDict
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from commonscenes_amd import configs as K, lib as L, ops, synth
from commonscenes_amd.vqvae import VQVAE, vqvae_encoder_param_shapes, vqvae_param_shapes

ENC_GFLOP, DEC_GFLOP = 271.0, 723.0

ap = argparse.ArgumentParser()
ap.add_argument("--batches", type=int, nargs="*", default=[1, 7, 16, 32])
ap.add_argument("--iters", type=int, default=3)
a = ap.parse_args()
dd = dict(K.VQVAE_DDCONFIG) if isinstance(K.VQVAE_DDCONFIG, dict) else K.VQVAE_DDCONFIG
dd = dict(dd, in_channels=1, double_z=False)
table = OrderedDict(list(vqvae_encoder_param_shapes(dd, K.VQVAE_N_EMBED, K.VQVAE_EMBED_DIM).items()) +
                    list(vqvae_param_shapes(dd, K.VQVAE_N_EMBED, K.VQVAE_EMBED_DIM).items()))
sd = synth.synth_state_dict(table, device="cuda")
vol = torch.cat([synth.sdf_volume(0), synth.sdf_volume(1)], dim=0).cuda()


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


for mode in ("f16x3", "fp32"):
    vq = VQVAE(dd, K.VQVAE_N_EMBED, K.VQVAE_EMBED_DIM, device="cuda").load_state_dict(sd).set_math(mode)
    for nb in a.batches:
        x = vol.repeat((nb + 1) // 2, 1, 1, 1, 1)[:nb].contiguous()
        te = timed(lambda: vq.encode_no_quant(x), a.iters)
        tf = timed(lambda: vq(x), a.iters)
        print(f"{mode:5s} {nb:3d} objects: encode_no_quant {te * 1e3 / nb:7.3f} ms/object "
              f"({ENC_GFLOP * nb / te / 1e3:6.1f} TFLOP/s); forward(x) {tf * 1e3 / nb:7.3f} ms/object "
              f"({(ENC_GFLOP + DEC_GFLOP) * nb / tf / 1e3:6.1f} TFLOP/s)", flush=True)
    del vq
    torch.cuda.empty_cache()

# conv_in A/B (16 objects): the same layer on the two routes, HIP events around each
w, b = sd["encoder.conv_in.weight"], sd["encoder.conv_in.bias"]
x = vol.repeat(8, 1, 1, 1, 1).contiguous()
for mode, m in (("f16x3", L.MATH_F16X3), ("fp32", L.MATH_FP32)):
    pw = ops.pack_weight(w, b, cin_pad=4, math=m)
    routes = {"cs_vqenc_conv_in": lambda: ops.vqenc_conv_in(x, w, b),
              "generic (layout + cs_conv_gemm)": lambda: ops.conv_gemm(ops.nchw_to_ndhwc(x, cpad=4), pw)}
    y0 = routes["cs_vqenc_conv_in"]()
    y1 = routes["generic (layout + cs_conv_gemm)"]()
    d = float((y0 - y1).double().norm() / y1.double().norm())
    for name, fn in routes.items():
        t = []
        for rep in range(2):          # best of two runs of 20 launches
            t.append(timed(fn, 20))
        print(f"conv_in 16 objects [{mode}] {name}: {min(t) * 1e6 / 16:7.1f} us/object "
              f"(output {64 ** 3 * 64 * 4 * 16 / min(t) / 1e12:5.2f} TB/s written)", flush=True)
    print(f"conv_in routes agree to rel-L2 {d:.1e}")
