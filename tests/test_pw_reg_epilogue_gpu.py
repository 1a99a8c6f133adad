"""The pointwise (TR) instantiations of conv_gemm_f16x3_kernel accumulate the transposed product and store from registers
(cs_gemm_f16x3.hip, "register-direct epilogue"); every other epilogue of those kernels first puts the accumulators back
into the untransposed layout.  Every TR instantiation -- tiles 1, 2, 3, 4, 6, 7 on the fp32 operand, 1 - 4 on the
interleaved pair -- meets every epilogue form here, at the smallest shapes that can still go wrong: one valid row in the
second row tile (or two tiles and 37 rows), a ragged last column tile with cout % 4 == 0 (cout % 16 == 0 for pair output),
whole [x | gate] groups for GEGLU at K = 48, and -- every second case -- all operands as views (lda > cin, ldo > cout).

Checks per case.  (1) Bit for bit against the same launch under CsDebug.no_pw: the table-driven, untransposed kernel and
its staged epilogue, untouched by the transposition (GroupNorm partials included where they are asked for).  (2) Against
fp64 (oracle/ref_ops.py) under test_gemm_variants_gpu.py's gates: whole tensor under gate(K), worst row and worst column
under the flat 1e-6; a pair output is decoded on the host first (hi + lo, 22 mantissa bits: 2.4e-7 per element at worst,
inside the same gates).  (3) The output allocation is filled with a sentinel word and every operand sits in a NaN-filled
allocation: afterwards every word outside the output view is still the sentinel, the result is finite, status 0.

One more case writes a 32x32 block of known values m * 1000 + n through the pair output and decodes it on the host: exact,
so a swapped operand order in the half exchange of cs_pair16_half32 (cs_epilogue.h) shows."""
import ctypes as C
from collections import namedtuple

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2
from test_f16x3_gpu import gate
from test_gemm_variants_gpu import PRE_ROWS, ROW_GATE, SENTINEL, TILES, X_SCALE, _place, _rand, _rowcol, _untouched_outside

pytestmark = pytest.mark.gpu

FORMS = ("plain", "bias", "rowvec", "rowvec2", "res", "to_out", "geglu", "geglu_pair", "res_pair", "gnpart")
PAIR_OUT = {"geglu_pair": 16.0, "res_pair": 16.0}
INSTS = [(0, t) for t in (1, 2, 3, 4, 6, 7)] + [(2, t) for t in (1, 2, 3, 4)]      # (a_format, tile): the TR kernels
A_PAIR_SCALE = 16.0

Case = namedtuple("Case", "fmt tile form m cin cout view")


def _dims(tile):
    wmb, wnb, wm, wn = TILES[tile]
    return 32 * wmb * wm, 32 * wnb * wn, 32 * wnb          # BM, BN, columns per wave


def _case(i, f, fmt, tile, form):
    """case f of instantiation i: views on every second case, the row counts alternating at half that rate"""
    bm, bn, wcols = _dims(tile)
    k = i + f // 2
    if form == "gnpart":
        m = 2 * bm                                          # two samples of one tile each: rows per sample % BM == 0
    elif bm == 256:
        m = 257
    elif bm == 128:
        m = (129, 2 * 128 + 37)[k % 2]
    else:
        m = (65, 2 * 64 + 37)[k % 2]
    if form in ("geglu", "geglu_pair"):
        cout, cin = (448 if bn == 224 else 2 * wcols), 48   # two whole [x | gate] groups
    else:
        pair = form in PAIR_OUT
        cout = {224: 240 if pair else 236, 128: 144 if pair else 132, 64: 80 if pair else 68}[bn]
        cin = 48 if fmt == 2 else 44
    return Case(fmt, tile, form, m, cin, cout, (i + f) % 2 == 1)


CASES = [_case(i, f, fmt, tile, form) for i, (fmt, tile) in enumerate(INSTS) for f, form in enumerate(FORMS)]


def _id(c):
    return f"f{c.fmt}-t{c.tile}-{c.form}-{c.m}-{c.cin}-{c.cout}" + ("-view" if c.view else "")


def _mods():
    from commonscenes_amd import lib as L, ops
    from oracle import ref_ops as R
    return L, ops, R


def test_cases_cover_every_tr_instantiation_and_form():
    assert {(c.fmt, c.tile, c.form) for c in CASES} == {(f, t, e) for f, t in INSTS for e in FORMS}
    for c in CASES:
        bm, bn, wcols = _dims(c.tile)
        assert c.m > bm and c.cout % 4 == 0
        if c.form in ("geglu", "geglu_pair"):
            assert c.cout == 2 * (224 if bn == 224 else wcols) and c.cout % wcols == 0 and c.cin == 48
        else:
            assert c.cout > bn and c.cout % bn
        if c.form in PAIR_OUT:
            assert (c.cout // (2 if c.form == "geglu_pair" else 1)) % 16 == 0
    assert abs(sum(c.view for c in CASES) - len(CASES) / 2) <= 1
    assert any(c.m % _dims(c.tile)[0] == 1 for c in CASES) and any(c.m % _dims(c.tile)[0] == 37 for c in CASES)


def _rv_rows(c):
    bm = _dims(c.tile)[0]
    return {"rowvec": bm, "to_out": bm, "rowvec2": bm // 2 + 11}.get(c.form, 1)


def _pair_encode(v, scale):
    """fp64 [rows, cols] (cols % 16 == 0) -> (the interleaved pair as int32 words [rows, cols], the value it holds)"""
    s = (v * scale).float()
    hi = s.half()
    lo = (s - hi.float()).half()
    rows, cols = v.shape
    h = torch.stack([hi.view(rows, cols // 16, 2, 8), lo.view(rows, cols // 16, 2, 8)], dim=3)   # [r, chunk, c8, hi|lo, 8]
    words = h.reshape(rows, cols * 2).contiguous().view(torch.int32)
    return words, (hi.double() + lo.double()) / scale


def _pair_decode(words, scale):
    """int32 words [rows, cols] of an interleaved pair -> fp64 values [rows, cols]"""
    rows, cols = words.shape
    h = words.contiguous().view(torch.float16).view(rows, cols // 16, 2, 2, 8).double()
    return ((h[:, :, :, 0] + h[:, :, :, 1]) / scale).reshape(rows, cols)


_DATA = {}


def _data(c):
    """CPU inputs and the fp64 result of a case: computed once, never modified"""
    if c in _DATA:
        return _DATA[c]
    _, _, R = _mods()
    seed = 5000 + 16 * CASES.index(c)
    t = {}
    x = (_rand(c.m, c.cin, seed=seed) * X_SCALE).double()
    if c.fmt == 2:
        t["xw"], x = _pair_encode(x, A_PAIR_SCALE)
    else:
        x = x.float().double()
    t["x"] = x
    t["wt"] = _rand(c.cout, c.cin, seed=seed + 3, scale=c.cin ** -0.5)
    t["bias"] = None if c.form in ("plain", "res") else _rand(c.cout, seed=seed + 4)
    if c.form in ("geglu", "geglu_pair"):
        # A unit bias on a gate column can sit near -2.5, and then the WHOLE output column is x * gelu(g) around g = -2.5, where
        # |g gelu'(g) / gelu(g)| ~ 6: the fp32 rounding of g alone (6e-8) already costs 3.7e-7 of the column, before the GEMM's
        # own error -- a column gate of 1e-6 then measures the conditioning of GELU, not the kernel (first run, unit bias:
        # worst column 1.10e-6 on f0-t1-geglu, bit-equal to the untransposed kernel).  GEGLU.proj's bias at a tenth, as in
        # test_epilogue_outputs_gpu.py's GEGLU cases: the gate stays N(0, 0.5) and no column lives in GELU's tail.
        t["bias"] = t["bias"] * 0.1
    rvr = _rv_rows(c)
    t["rv"] = _rand(-(-c.m // rvr), c.cout, seed=seed + 5) if c.form in ("rowvec", "rowvec2", "to_out") else None
    t["res"] = _rand(c.m, c.cout, seed=seed + 6) if c.form in ("res", "to_out", "res_pair") else None
    y = R.conv_ndhwc(x.view(1, 1, 1, c.m, c.cin), t["wt"].double(), None if t["bias"] is None else t["bias"].double())
    y = y.view(c.m, c.cout)
    if t["rv"] is not None:
        y = y + t["rv"].double()[torch.arange(c.m) // rvr]
    if c.form in ("rowvec", "rowvec2"):
        y = F.silu(y)
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
    """the operands on the device, each inside a NaN-filled allocation (view cases: lda > cin; ldr / ldrv > cout always)"""
    L, ops, _ = _mods()
    t = _data(c)
    d = {}
    if c.fmt == 2:
        xw = t["xw"].cuda().view(torch.float32)
        d["x"] = _place(xw, *((c.cin + 48, 16) if c.view else (c.cin, 0)), bits=True)
    else:
        d["x"] = _place(t["x"].float().cuda(), *((c.cin + 12, 4) if c.view else (c.cin, 0)))
    bias = None if t["bias"] is None else t["bias"].cuda()
    d["pk"] = ops.pack_weight(t["wt"].cuda(), bias, cin_pad=c.cin, math=L.MATH_F16X3)
    d["bias"] = bias is not None
    if t["rv"] is not None:
        d["rv"] = _place(t["rv"].cuda(), c.cout + 4, 4)
    if t["res"] is not None:
        d["res"] = _place(t["res"].cuda(), c.cout + 8, 4)
    return d


def _launch(c, dev, **switches):
    """one cs_conv_gemm of the case into a fresh sentinel-filled allocation -> (output view, gn_part | None)"""
    L, ops, _ = _mods()
    ocols = c.cout // 2 if c.form in ("geglu", "geglu_pair") else c.cout
    ldo, off = (ocols + 32, 16) if c.view else (ocols, 0)
    buf = torch.empty((PRE_ROWS + c.m + 5, ldo), dtype=torch.float32, device="cuda")
    buf.view(torch.int32).fill_(SENTINEL)
    out = buf[PRE_ROWS:PRE_ROWS + c.m, off:off + ocols]
    x, pk = dev["x"], dev["pk"]
    bm = _dims(c.tile)[0]
    p = L.CsConvGemm()
    p.x, p.out = x.data_ptr(), out.data_ptr()
    p.lda, p.ldo, p.ldw = x.stride(0), ldo, pk.ldw
    nb = 2 if c.form == "gnpart" else 1
    p.nb, p.din, p.hin, p.win = nb, 1, 1, c.m // nb
    p.dout, p.hout, p.wout = 1, 1, c.m // nb
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
        p.rowvec, p.ldrv, p.rv_rows = dev["rv"].data_ptr(), dev["rv"].stride(0), _rv_rows(c)
    if c.form in ("rowvec", "rowvec2"):
        p.act = L.ACT_SILU
    if c.form in ("geglu", "geglu_pair"):
        p.act = L.ACT_GEGLU
    if "res" in dev:
        p.res, p.ldr = dev["res"].data_ptr(), dev["res"].stride(0)
    if c.form in PAIR_OUT:
        p.out_format, p.out_scale = 2, PAIR_OUT[c.form]
    part = None
    if c.form == "gnpart":
        part = torch.full((c.m // bm, c.cout, 2), float("nan"), dtype=torch.float64, device="cuda")
        p.gn_part, p.gn_ld, p.gn_rows = part.data_ptr(), c.cout, bm
    with L.debug_override(**switches):
        tl, sl = C.c_int32(-1), C.c_int32(-1)
        L.check(L.load().cs_conv_gemm_launch_info(C.byref(p), C.byref(tl), C.byref(sl)), "cs_conv_gemm_launch_info")
        assert (tl.value, sl.value) == (c.tile, 0)
        L.check(L.load().cs_conv_gemm(C.byref(p), None), "cs_conv_gemm")
        torch.cuda.synchronize()
    assert _untouched_outside(buf, out), "a word outside the output view was written"
    return out, part


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_tr_epilogue_forms(c):
    L, ops, _ = _mods()
    t = _data(c)
    dev = _device(c)
    ops.read_status()
    out, part = _launch(c, dev)
    twin, tpart = _launch(c, dev, no_pw=1)
    assert ops.read_status() == 0
    assert torch.equal(out.view(torch.int32), twin.view(torch.int32)), "pointwise != table-driven (CsDebug.no_pw)"
    if part is not None:
        assert torch.equal(part.view(torch.int64), tpart.view(torch.int64)), "GroupNorm partials differ from the no_pw launch"
        assert torch.isfinite(part).all()
    val = _pair_decode(out.cpu().view(torch.int32), PAIR_OUT[c.form]) if c.form in PAIR_OUT else out.double().cpu()
    ref = t["ref"]
    whole = rel_l2(val, ref)
    row, col = _rowcol(val, ref)
    print(f"pw_reg_epilogue {_id(c)}: whole {whole:.3e} row {row:.3e} col {col:.3e}")
    assert torch.isfinite(val).all()
    assert whole < gate(c.cin), (whole, gate(c.cin))
    assert row < ROW_GATE and col < ROW_GATE, (row, col)


def test_pair_half_exchange_on_known_values():
    """out[m][n] = m * 1000 + n (exact in every format on the way), pair output at scale 1/2, decoded on the host"""
    L, ops, _ = _mods()
    m = n = 32
    x = torch.zeros(m, 4)
    x[:, 0], x[:, 1] = torch.arange(m, dtype=torch.float32), 1.0
    w = torch.zeros(n, 4)
    w[:, 0], w[:, 1] = 1000.0, torch.arange(n, dtype=torch.float32)
    pk = ops.pack_weight(w.cuda(), torch.zeros(n).cuda(), cin_pad=4, math=L.MATH_F16X3)
    xd = x.cuda()
    buf = torch.empty((PRE_ROWS + m + 5, n), dtype=torch.float32, device="cuda")
    buf.view(torch.int32).fill_(SENTINEL)
    out = buf[PRE_ROWS:PRE_ROWS + m]
    p = L.CsConvGemm()
    p.x, p.out, p.bias = xd.data_ptr(), out.data_ptr(), pk.bias.data_ptr()
    p.lda, p.ldo, p.ldw = 4, n, pk.ldw
    p.nb, p.din, p.hin, p.win, p.dout, p.hout, p.wout = 1, 1, 1, m, 1, 1, m
    p.cin, p.cout = 4, n
    p.kd = p.kh = p.kw = p.sd = p.sh = p.sw = 1
    p.math, p.tile, p.rv_rows = L.MATH_F16X3, 3, 1
    p.w, p.w_lo = pk.wh.data_ptr(), pk.wl.data_ptr()
    p.a_scale, p.acc_scale = ops.A_SCALE, pk.acc_scale
    p.status = ops.status_word(xd.device).data_ptr()
    p.out_format, p.out_scale = 2, 0.5
    ops.read_status()
    L.check(L.load().cs_conv_gemm(C.byref(p), None), "cs_conv_gemm")
    torch.cuda.synchronize()
    assert ops.read_status() == 0
    assert _untouched_outside(buf, out)
    got = _pair_decode(out.cpu().view(torch.int32), 1.0)
    want = (torch.arange(m).double()[:, None] * 1000.0 + torch.arange(n).double()[None, :]) * 0.5
    assert torch.equal(got, want), (got - want).abs().max()
