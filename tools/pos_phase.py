#!/usr/bin/env python
"""Phase budget of the Winograd-W position GEMMs (tools/tok_phase.py's sibling): the three conv shapes that carry the step's
position time, each run PP_N times in a row through GroupNorm (transformed operand) -> ops.conv_gemm, to be read from a
rocprofv3 kernel trace with tools/rocpd_by_grid.py (the position kernel's dispatches by grid size; the output transform is
another kernel).  Against the product library and the -DCS_ABLATE=2048 (no K loop) / 18432 (no K loop, no stores) builds:
    CS_LIB_PATH=commonscenes_amd/alt/libcommonscenes_hip_<name>.so rocprofv3 --kernel-trace -d DIR -o pos -- python tools/pos_phase.py
position launch of each shape (rows = positions x M / R):  196608 x 2016 -> 224,  98304 x 4032 -> 448,  24576 x 6048 -> 672"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from commonscenes_amd import lib as L
from commonscenes_amd import ops, synth

N = int(os.environ.get("PP_N", "12"))
SHAPES = [(32, (16, 16, 16), 224, 224), (64, (16, 8, 8), 448, 448), (64, (16, 4, 4), 672, 672)]
for nb, sp, cin, cout in SHAPES:
    rows = sp[0] * sp[1] * sp[2]
    x = synth.tensor_device(f"x{sp}{cin}", (nb, *sp, cin), 1.0)
    g = synth.tensor_device(f"g{cin}", (cin,), 1.0)
    b = synth.tensor_device(f"b{cin}", (cin,), 0.1)
    w = synth.tensor_device(f"w{cin}{cout}", (cout, cin, 3, 3, 3), (3.0 / (cin * 27)) ** 0.5)
    pw = ops.pack_weight_wino(ops.pack_weight(w, synth.tensor_device(f"c{cout}", (cout,), 0.1), math=L.MATH_F16X3), w)
    emb = synth.tensor_device(f"e{cout}", (nb, cout), 1.0)
    wv = ops.wants_wino(nb, *sp, pw)
    if not wv:
        print(f"{sp} {cin}->{cout} batch {nb}: not eligible", flush=True)
        continue
    v = ops.groupnorm(x, g, b, 32, 1e-5, L.ACT_SILU, wino=wv)
    for _ in range(N):
        ops.conv_gemm(v, pw, rowvec=emb, rv_rows=rows, stats=True)
    torch.cuda.synchronize()
    print(f"positions F({wv},3): {(wv + 2) * nb * rows // wv} x {9 * cin} -> {cout}", flush=True)
