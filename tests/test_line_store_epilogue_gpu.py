"""Whole-line stores of the register-direct epilogues (cs_gemm_f16x3.hip; cs_epilogue.h::cs_quad_transpose4): before it
stores, a TR kernel transposes the four float4s of each 32x32 block inside its lane quads, so that slot s of lane q holds
row r0 + s, columns 8 q + 4 h + 0..3.  Row validity is then per slot, column validity per lane, the residual is loaded at
the transposed addresses, and the Winograd-W position GEMMs (three-tap slab kernel) store that way into the workspace.
tests/test_gemm_variants_gpu.py, test_pw_reg_epilogue_gpu.py and test_wino_variants_gpu.py cover the kernels as they stand;
this file adds the shapes at which the transposition itself can go wrong.  (The kernel's LINE rule decides which tiles
exchange: the position GEMMs and the 256x224 pointwise tile in the product, every pointwise tile in a -DCS_LINE_PW=2 build.
The cases below hold for either epilogue, so every tile with a register-direct path meets them.)

One-tap GEMMs, tiles 1, 2, 3, 4, 6, 7 (fp32 operand; the interleaved pair operand on 1 - 4 in every second case):
  rows     one whole tile + 35 (the last quad holds 3 valid rows, in a second tile), + 33 and + 34 (M = 1, 2 mod 4)
  columns  BN + 36 (the edge tile's second block holds ONE valid float4; BN + 48 where the output is a pair: 16-column
           chunks) and 28 (16 for a pair: lanes q >= 2 of the only block are masked)
  K        64 and 448
  strides  ldo != ldr, neither a multiple of 32 floats, the views 16 bytes (pair: 64) into their rows: no row of the
           residual or of an fp32 output starts on a 128-byte line (a pair output: every second row does not).  The same
           case into 128-byte aligned rows must give the same bits.
  forms    plain | bias + row vector + SiLU | residual | residual to pair | GEGLU | GEGLU to pair, every tile every form
           (GEGLU: cout = 448 on the 224-wide tiles, 256 elsewhere -- whole [x | gate] groups of the wave, and no row
           narrower than 128 outputs: a row is judged by its own norm, and over the 32 outputs that two groups of the 64x64
           tile give, the flat 1e-6 row gate measures how GELU's conditioning happens to fall on a few dozen values -- first
           run, f0-t3-geglu_pair K = 448 cout = 64: worst row 1.27e-6 while bit-equal to the untransposed kernel and to the
           aligned launch, which is what the transposition could break)
Each case: bit-equal to the launch under CsDebug.no_pw (the untransposed kernel and its staged epilogue), fp64 under
test_gemm_variants_gpu.py's gates (whole tensor gate(K), worst row / column 1e-6), every word outside the output view still
the sentinel (guard rows before and after, ldo wider than the row), operands inside NaN-filled allocations, status 0.

Positions (cs_conv_wino_positions): F(2,3) and F(4,3) at the smallest volumes the entry accepts, cout 224 and 448, unsliced
and with 2 and 3 K slices, against _wino_cases.positions64 under test_wino_variants_gpu.py's gates; no word outside the
[slices, P, M / R, cout] view is written (sentinel bands), nothing reaches the output."""
import ctypes as C
from collections import namedtuple

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2
from test_f16x3_gpu import gate
from test_gemm_variants_gpu import PRE_ROWS, ROW_GATE, SENTINEL, TILES, X_SCALE, _place, _rand, _rowcol, _untouched_outside
from test_pw_reg_epilogue_gpu import A_PAIR_SCALE, _pair_decode, _pair_encode
from test_wino_variants_gpu import _assert_grant, _check_positions, _desc, _pack, _run_positions, _unused_output, _wscale

import _wino_cases as W

pytestmark = pytest.mark.gpu

FORMS = ("plain", "brv", "res", "res_pair", "geglu", "geglu_pair")
PAIR_OUT = {"res_pair": 16.0, "geglu_pair": 16.0}
TILE_CODES = (1, 2, 3, 4, 6, 7)
ROWS_PAST = (35, 33, 34)

Case = namedtuple("Case", "fmt tile form m cin cout")


def _dims(tile):
    wmb, wnb, wm, wn = TILES[tile]
    return 32 * wmb * wm, 32 * wnb * wn, 32 * wnb          # BM, BN, columns per wave


def _case(ti, f, tile, form):
    bm, bn, wcols = _dims(tile)
    k = ti + f
    m = bm + ROWS_PAST[k % 3]
    cin = (64, 448)[(k // 2) % 2]
    if form in ("geglu", "geglu_pair"):
        cout = 448 if bn == 224 else max(2 * wcols, 256)    # whole [x | gate] groups, at least 128 outputs per row
    elif form in PAIR_OUT:
        cout = 16 if tile in (2, 3, 6) else bn + 48         # (every tile width meets the edge tile once)
    else:
        cout = (bn + 36, 28)[k % 2]
    fmt = 2 if (tile <= 4 and k % 2 == 0) else 0
    return Case(fmt, tile, form, m, cin, cout)


CASES = [_case(ti, f, tile, form) for ti, tile in enumerate(TILE_CODES) for f, form in enumerate(FORMS)]


def _id(c):
    return f"f{c.fmt}-t{c.tile}-{c.form}-{c.m}-{c.cin}-{c.cout}"


def _mods():
    from commonscenes_amd import lib as L, ops
    from oracle import ref_ops as R
    return L, ops, R


def test_cases_cover_every_tile_form_row_count_width_and_depth():
    assert {(c.tile, c.form) for c in CASES} == {(t, e) for t in TILE_CODES for e in FORMS}
    for tile in TILE_CODES:
        bm, bn, _ = _dims(tile)
        mine = [c for c in CASES if c.tile == tile]
        assert {c.m - bm for c in mine} == {33, 34, 35} and {c.m % 4 for c in mine} == {1, 2, 3}
        assert {c.cin for c in mine} == {64, 448}
        plain = [c for c in mine if c.form in ("plain", "brv", "res")]
        assert {c.cout for c in plain} == {bn + 36, 28}, "one valid float4 in the edge tile's second block; a 28-column tile"
        assert {c.cout for c in mine if c.form == "res_pair"} <= {bn + 48, 16}
    assert {c.cout for c in CASES if c.form == "res_pair"} == {b + 48 for b in (64, 128, 224)} | {16}
    assert {c.fmt for c in CASES} == {0, 2} and all(c.tile <= 4 for c in CASES if c.fmt == 2)


def _ocols(c):
    return c.cout // 2 if c.form in ("geglu", "geglu_pair") else c.cout


def _ld(cols, step, avoid=()):
    """the smallest row stride >= cols + step floats that is a multiple of `step`, no multiple of 32, and not in `avoid`"""
    ld = (cols + step + step - 1) // step * step
    while ld % 32 == 0 or ld in avoid:
        ld += step
    return ld


def _strides(c, aligned):
    """(ldo, column offset of the output view, ldr, column offset of the residual view) in floats"""
    oc = _ocols(c)
    if aligned:
        return (oc + 31) // 32 * 32, 0, (c.cout + 31) // 32 * 32 + 32, 0
    # fp32 rows: stride % 8 == 0 and the view 4 floats in -- (row * stride + 4) % 32 != 0 for EVERY row; a pair output needs
    # ldo % 16 == 0 and a 64-byte aligned view, so there every second row starts on a line and the others in its middle
    pair = c.form in PAIR_OUT
    ldo = _ld(oc, 16 if pair else 8)
    return ldo, (16 if pair else 4), _ld(c.cout, 8, avoid=(ldo,)), 4


def test_unaligned_strides_are_what_the_docstring_says():
    for c in CASES:
        ldo, oo, ldr, ro = _strides(c, False)
        assert ldo % 32 and ldr % 32 and ldo != ldr and ldo >= _ocols(c) + oo and ldr >= c.cout + ro
        for ld, o in ((ldr, ro),) + (() if c.form in PAIR_OUT else ((ldo, oo),)):
            assert all((r * ld + o) % 32 for r in range(32)), "a row of the view starts on a 128-byte line"
        assert ldo % (16 if c.form in PAIR_OUT else 8) == 0 and ldr % 8 == 0
        lda, oa, _, _ = _strides(c, True)
        assert lda % 32 == 0 and oa == 0


def _rv_rows(c):
    return _dims(c.tile)[0]                                  # one sample per row tile


_DATA = {}


def _data(c):
    """CPU inputs and the fp64 result of a case: computed once, never modified"""
    if c in _DATA:
        return _DATA[c]
    _, _, R = _mods()
    seed = 6100 + 16 * CASES.index(c)
    t = {}
    x = (_rand(c.m, c.cin, seed=seed) * X_SCALE).double()
    if c.fmt == 2:
        t["xw"], x = _pair_encode(x, A_PAIR_SCALE)
    else:
        x = x.float().double()
    t["x"] = x
    t["wt"] = _rand(c.cout, c.cin, seed=seed + 3, scale=c.cin ** -0.5)
    t["bias"] = _rand(c.cout, seed=seed + 4) if c.form in ("brv", "geglu", "geglu_pair") else None
    if c.form in ("geglu", "geglu_pair"):
        t["bias"] = t["bias"] * 0.1                          # (test_pw_reg_epilogue_gpu.py::_data says why: GELU's tail)
    t["rv"] = _rand(-(-c.m // _rv_rows(c)), c.cout, seed=seed + 5) if c.form == "brv" else None
    t["res"] = _rand(c.m, c.cout, seed=seed + 6) if c.form in ("res", "res_pair") else None
    y = R.conv_ndhwc(x.view(1, 1, 1, c.m, c.cin), t["wt"].double(), None if t["bias"] is None else t["bias"].double())
    y = y.view(c.m, c.cout)
    if t["rv"] is not None:
        y = F.silu(y + t["rv"].double()[torch.arange(c.m) // _rv_rows(c)])
    if c.form in ("geglu", "geglu_pair"):
        wcols = _dims(c.tile)[2]
        g = y.view(c.m, c.cout // wcols, 2, wcols // 2)
        y = (g[:, :, 0] * F.gelu(g[:, :, 1])).reshape(c.m, c.cout // 2)
    if t["res"] is not None:
        y = y + t["res"].double()
    t["ref"] = y.contiguous()
    _DATA[c] = t
    return t


def _device(c):
    """the operands that do not depend on the strides under test, each inside a NaN-filled allocation (lda > cin)"""
    L, ops, _ = _mods()
    t = _data(c)
    d = {}
    if c.fmt == 2:
        d["x"] = _place(t["xw"].cuda().view(torch.float32), c.cin + 48, 16, bits=True)
    else:
        d["x"] = _place(t["x"].float().cuda(), c.cin + 12, 4)
    bias = None if t["bias"] is None else t["bias"].cuda()
    d["pk"] = ops.pack_weight(t["wt"].cuda(), bias, cin_pad=c.cin, math=L.MATH_F16X3)
    d["bias"] = bias is not None
    if t["rv"] is not None:
        d["rv"] = _place(t["rv"].cuda(), c.cout + 4, 4)
    return d


def _launch(c, dev, aligned=False, **switches):
    """one cs_conv_gemm of the case into a fresh sentinel-filled allocation -> the output view"""
    L, ops, _ = _mods()
    t = _data(c)
    ocols = _ocols(c)
    ldo, off, ldr, roff = _strides(c, aligned)
    buf = torch.empty((PRE_ROWS + c.m + 5, ldo), dtype=torch.float32, device="cuda")
    buf.view(torch.int32).fill_(SENTINEL)
    out = buf[PRE_ROWS:PRE_ROWS + c.m, off:off + ocols]
    x, pk = dev["x"], dev["pk"]
    p = L.CsConvGemm()
    p.x, p.out = x.data_ptr(), out.data_ptr()
    p.lda, p.ldo, p.ldw = x.stride(0), ldo, pk.ldw
    p.nb, p.din, p.hin, p.win = 1, 1, 1, c.m
    p.dout, p.hout, p.wout = 1, 1, c.m
    p.cin, p.cout = c.cin, c.cout
    p.kd = p.kh = p.kw = p.sd = p.sh = p.sw = 1
    p.math, p.tile, p.rv_rows = L.MATH_F16X3, c.tile, 1
    p.w, p.w_lo = pk.wh.data_ptr(), pk.wl.data_ptr()
    a_sc = A_PAIR_SCALE if c.fmt == 2 else ops.A_SCALE
    p.a_scale, p.acc_scale, p.a_format = a_sc, pk.acc_scale * (ops.A_SCALE / a_sc), c.fmt
    p.status = ops.status_word(x.device).data_ptr()
    if dev["bias"]:
        p.bias = pk.bias.data_ptr()
    if "rv" in dev:
        p.rowvec, p.ldrv, p.rv_rows, p.act = dev["rv"].data_ptr(), dev["rv"].stride(0), _rv_rows(c), L.ACT_SILU
    if c.form in ("geglu", "geglu_pair"):
        p.act = L.ACT_GEGLU
    res = None
    if t["res"] is not None:
        res = _place(t["res"].cuda(), ldr, roff)
        p.res, p.ldr = res.data_ptr(), ldr
    if c.form in PAIR_OUT:
        p.out_format, p.out_scale = 2, PAIR_OUT[c.form]
    with L.debug_override(**switches):
        tl, sl = C.c_int32(-1), C.c_int32(-1)
        L.check(L.load().cs_conv_gemm_launch_info(C.byref(p), C.byref(tl), C.byref(sl)), "cs_conv_gemm_launch_info")
        assert (tl.value, sl.value) == (c.tile, 0)
        L.check(L.load().cs_conv_gemm(C.byref(p), None), "cs_conv_gemm")
        torch.cuda.synchronize()
    assert _untouched_outside(buf, out), "a word outside the output view was written"
    return out


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_one_tap_line_stores(c):
    L, ops, _ = _mods()
    t = _data(c)
    dev = _device(c)
    ops.read_status()
    out = _launch(c, dev)
    twin = _launch(c, dev, no_pw=1)
    flat = _launch(c, dev, aligned=True)
    assert ops.read_status() == 0
    assert torch.equal(out.view(torch.int32), twin.view(torch.int32)), "pointwise != table-driven (CsDebug.no_pw)"
    assert torch.equal(out.view(torch.int32), flat.view(torch.int32)), "unaligned strides != 128-byte aligned rows"
    val = _pair_decode(out.cpu().view(torch.int32), PAIR_OUT[c.form]) if c.form in PAIR_OUT else out.double().cpu()
    ref = t["ref"]
    whole = rel_l2(val, ref)
    row, col = _rowcol(val, ref)
    print(f"line_store {_id(c)}: whole {whole:.3e} (gate {gate(c.cin):.0e}) row {row:.3e} col {col:.3e} (gate {ROW_GATE:.0e})")
    assert torch.isfinite(val).all()
    assert whole < gate(c.cin), (whole, gate(c.cin))
    assert row < ROW_GATE and col < ROW_GATE, (row, col)


def test_rows_land_on_their_own_lines_on_known_values():
    """out[m][n] = m * 1000 + n, exact in every format on the way, on the 64x64 tile with M = 99 and cout = 100 (a second row
    and column tile, the last quad with 3 rows, the last block with one float4): a slot stored to another row of its quad, or
    a lane to another lane's columns, shows as a wrong integer"""
    L, ops, _ = _mods()
    m, n = 99, 100
    x = torch.zeros(m, 4)
    x[:, 0], x[:, 1] = torch.arange(m, dtype=torch.float32), 1.0
    w = torch.zeros(n, 4)
    w[:, 0], w[:, 1] = 1000.0, torch.arange(n, dtype=torch.float32)
    pk = ops.pack_weight(w.cuda(), torch.zeros(n).cuda(), cin_pad=4, math=L.MATH_F16X3)
    xd = x.cuda()
    ldo = 116
    buf = torch.empty((PRE_ROWS + m + 5, ldo), dtype=torch.float32, device="cuda")
    buf.view(torch.int32).fill_(SENTINEL)
    out = buf[PRE_ROWS:PRE_ROWS + m, 4:4 + n]
    p = L.CsConvGemm()
    p.x, p.out, p.bias = xd.data_ptr(), out.data_ptr(), pk.bias.data_ptr()
    p.lda, p.ldo, p.ldw = 4, ldo, pk.ldw
    p.nb, p.din, p.hin, p.win, p.dout, p.hout, p.wout = 1, 1, 1, m, 1, 1, m
    p.cin, p.cout = 4, n
    p.kd = p.kh = p.kw = p.sd = p.sh = p.sw = 1
    p.math, p.tile, p.rv_rows = L.MATH_F16X3, 3, 1
    p.w, p.w_lo = pk.wh.data_ptr(), pk.wl.data_ptr()
    p.a_scale, p.acc_scale = ops.A_SCALE, pk.acc_scale
    p.status = ops.status_word(xd.device).data_ptr()
    ops.read_status()
    L.check(L.load().cs_conv_gemm(C.byref(p), None), "cs_conv_gemm")
    torch.cuda.synchronize()
    assert ops.read_status() == 0
    assert _untouched_outside(buf, out)
    want = torch.arange(m).double()[:, None] * 1000.0 + torch.arange(n).double()[None, :]
    assert torch.equal(out.double().cpu(), want), (out.double().cpu() - want).abs().max()


# ---- the position GEMMs ---------------------------------------------------------------------------------------------------------
# the smallest volume of each variant the entry accepts (_wino_cases.GEOM "W4": one sample of 32 x 4 x 4 for F(2,3), two for
# F(4,3)), both widths each; view: lda = cin + 8
POS = [W.Conv(2, "W4", 24, 224, True), W.Conv(2, "W4", 72, 448, False), W.Conv(4, "W4", 24, 224, True), W.Conv(4, "W4", 72, 448, False)]
# cin 24 = 6 super-chunks (one kd x 16 channels): 3 + 3 and 2 + 2 + 2; cin 72 = 15: 8 + 7 and 5 + 5 + 5
SLICES = (1, 2, 3)


def test_position_cases_are_the_smallest_volumes_and_whole_super_chunks():
    for c in POS:
        vol = W.GEOM[c.variant][c.geom]
        assert W.rows_of(vol) == min(W.rows_of(v) for v in W.GEOM[c.variant].values())
        nsc = 3 * ((c.cin + 15) // 16)
        for s in SLICES:
            assert s == 1 or -(-nsc // s) * s * 10 <= nsc * 11
    assert {(c.variant, c.cout) for c in POS} == {(2, 224), (2, 448), (4, 224), (4, 448)}


_POS = {}


def _pos_data(c):
    """host inputs of a position case, computed once (as test_wino_variants_gpu.py::_conv_data, which serves its own table only):
    the operand images as fp16 hi / lo of B^T d a_scale, the weights, the fp64 position results of exactly those operands"""
    if c not in _POS:
        vol = W.GEOM[c.variant][c.geom]
        seed = 6900 + 16 * POS.index(c)
        y = W.rand(*vol, c.cin, seed=seed) * X_SCALE
        wt = W.rand(c.cout, c.cin, 3, 3, 3, seed=seed + 1) * (27 * c.cin) ** -0.5
        a_scale = 8.0 if c.variant == 2 else 1.0               # the producers': 16 / 2 resp. 16 / 16
        hi, lo, val = W.split16(W.images64(y.double(), c.variant), a_scale)
        assert float(hi.float().abs().max()) < 65504.0
        _POS[c] = dict(vol=vol, wt=wt, hi=hi, lo=lo, a_scale=a_scale, ref=W.positions64(val, W.weights64(wt.double(), c.variant)))
    return _POS[c]


def _pos_setup(c):
    """the descriptor of a case with its operand images and packed weights on the device (view: lda = cin + 8, NaN in the gap)"""
    _, ops, _ = _mods()
    t = _pos_data(c)
    p = _desc(t["vol"], c.cin, c.cout, c.variant)
    mt = W.rows_of(t["vol"]) // c.variant
    rows = (c.variant + 2) * mt
    lda = c.cin + 8 if c.view else c.cin
    keep = [W.place(t[k].reshape(rows, c.cin), lda, 0, "cuda") for k in ("hi", "lo")]
    scale = _wscale(t["wt"], c.variant)
    keep.append(_pack(t["wt"].cuda(), c.cin, c.variant, scale))
    p.x, p.x_lo, p.lda = keep[0][1].data_ptr(), keep[1][1].data_ptr(), lda
    p.w, p.w_lo = keep[2][0][1].data_ptr(), keep[2][1][1].data_ptr()
    p.a_scale, p.acc_scale = t["a_scale"], 1.0 / (scale * t["a_scale"])
    p.status = ops.status_word(torch.device("cuda", 0)).data_ptr()
    _unused_output(p, W.rows_of(t["vol"]), c.cout, keep)
    return p, keep, mt


@pytest.mark.parametrize("slices", SLICES, ids=[f"k{s}" for s in SLICES])
@pytest.mark.parametrize("c", POS, ids=W.conv_id)
def test_positions_store_whole_lines_into_the_workspace(c, slices):
    t = _pos_data(c)
    p, keep, mt = _pos_setup(c)
    plan = _assert_grant(c, p)
    ws = _run_positions(p, slices, mt, c.cout, keep[-1])     # (asserts: status 0, bands hold, the output untouched)
    _check_positions(W.conv_id(c) + f" k{slices} line stores", ws, t["ref"], c.cin, plan)
    if slices > 1:
        assert all(float(ws[s].abs().max()) > 0.0 for s in range(slices))
