"""The Winograd-W conv route and the split-K reduce pair, piecewise against fp64 (cs_gemm.hip: pack_f16x3_wino_kernel, conv_wino's
stacked position GEMMs -- launch16<..., TPK = 3> of cs_gemm_f16x3.hip with omap_p positions --, wino_out_kernel<2> / <4>,
splitk_reduce_kernel, splitk_reduce_epi_kernel), at the smallest geometries at which each edge exists (tests/_wino_cases.py: D = 1,
H = 1, W = 4 / 6 / 12 / 64, an odd batch, cin 16 / 24 / 40 / 72, cout 64 / 128 / 224 / 256 / 448 = tiles 7 / 6 / 4), every
second case with all operands as views of wider buffers (lda = cin + 8, ldo = cout + 12, own ldr / ldrv, gn_ld = cout + 4).  The
descriptors are built directly (CsConvGemm), the thresholds opened with CsDebug.wino_min_rows / wino43_min_rows = 1, and every case
first asserts through cs_conv_wino_ok / cs_conv_wino_plan_info that the library grants the variant and plan it is meant for.

1. cs_pack_weight_f16x3_wino_v: (hi + lo) / scale against G g in fp64, both variants, whole-tensor and channel-slice form
   (src_cin, c0), |error| <= 2^-21 |u| + 2^-24 2^-14 / scale; the channels cin .. 16 ceil(cin / 16) exactly zero.
2. cs_conv_wino_positions alone on operand images built on the host (B^T d in fp64, split into fp16 hi / lo; NaN in the lda gaps
   and in bands of rows around them): status 0, every workspace word outside [slices][P][M / R][cout] still the sentinel, the
   slice sum against the fp64 3x3x1 conv -- whole tensor under gate(9 cin), worst row / column (relative to the RMS row / column
   norm of the whole reference) under a flat 1e-6 -- at the plan's slice count and at explicit 1, 2 and ragged counts.
3. cs_conv_wino_output alone on a synthetic workspace (random fp32, NaN bands, NaN in every slice it must not read): elementwise
   inside the derived bound E = (a + 4) 2^-24 T of _wino_cases.py, bit for bit equal to the fp32 CPU restatement where the epilogue
   is additive only; rv_rows that cut through a tile; scale / shift, SiLU, GELU; gn_part (fp64 sums of the kernel's own output
   rows, (16 R + 16) 2^-53; gn_ld gap untouched -- with cout = 224 the columns 224 .. 255 of the last block); out_format = 2
   decoded and compared bit for bit with the fp32 launch, and the overflow status.
4. The tail plan at the smallest shape cs_conv_wino_plan_info grants it: the positions launch leaves slices 1 .. of the main
   units untouched, the output transform reads one slice for them (NaN elsewhere), the whole conv against fp64 and no_wino_tail.
5. ops.groupnorm(wino=variant) -> ops.conv_gemm as the hosts call it, on the geometry table with bias + rowvec + res and
   stats=True, against fp64 (whole 1e-6 and (2 | 3.5) x the direct form + 2e-7: test_wino_gpu.py's gates; worst row / column
   1e-6 for F(2,3), 2e-6 for F(4,3)).
6. splitk_reduce_kernel / splitk_reduce_epi_kernel (cs_conv_gemm with explicit splitk under CsDebug.no_fused_reduce) against the
   partial tiles the call left in the test's own workspace: bound, bit equality, gn_part, pair output as in 3.
7. Refusals: CS_EINVAL with the output untouched, host only.

Not covered here: the fused in-kernel reduce (test_fused_splitk_gpu.py), up2_reduce_scatter_kernel (test_up2_variants_gpu.py: slice
counts 2 / 9 / 10 / 17, read back from the workspace footprint), the K-wave
kernel (test_kwave_gpu.py), the GroupNorm producer of the operand images (test_norm_variants_gpu.py), the workload's own shapes
(test_wino_gpu.py).  Measured values: profiles/wino_variants_parity.txt (nothing here reads them)."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2
from test_f16x3_gpu import gate
from test_gemm_variants_gpu import ROW_GATE, SENTINEL, X_SCALE, _rowcol

import _wino_cases as W

pytestmark = pytest.mark.gpu

OPEN = dict(wino_min_rows=1, wino43_min_rows=1)
BAND = 4096                    # floats of band before / after a workspace
NAN = float("nan")
assert SENTINEL == W.SENTINEL


def _mods():
    from commonscenes_amd import lib as L, ops
    return L, ops


def _desc(vol, cin, cout, variant):
    """the 3x3x3 stride-1 conv over vol = (nb, D, H, W) as a Winograd-W descriptor (a_format 3 / 4), no pointers yet"""
    L, _ = _mods()
    p = L.CsConvGemm()
    p.nb, p.din, p.hin, p.win = vol
    p.dout, p.hout, p.wout = vol[1:]
    p.cin, p.cout, p.lda, p.ldo, p.ldw = cin, cout, cin, cout, cout
    p.kd = p.kh = p.kw = 3
    p.sd = p.sh = p.sw = p.pd = p.ph = p.pw = 1
    p.math, p.rv_rows, p.a_format = L.MATH_F16X3, 1, (4 if variant == 4 else 3)
    p.a_scale = p.acc_scale = 1.0
    return p


def _granted(p):
    L, _ = _mods()
    return int(L.load().cs_conv_wino_ok(C.byref(p)))


def _plan(p):
    """(slices, units_main, units) of cs_conv_wino_plan_info"""
    L, _ = _mods()
    sl, um, ut = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    L.check(L.load().cs_conv_wino_plan_info(C.byref(p), C.byref(sl), C.byref(um), C.byref(ut)), "cs_conv_wino_plan_info")
    return sl.value, um.value, ut.value


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _wscale(wt, variant):
    """ops.pack_weight_wino's power-of-two scale: max |u_q| <= 1.5 max |w| (F(2,3)), <= max |w| (F(4,3))"""
    am = (1.5 if variant == 2 else 1.0) * float(wt.abs().max())
    return 2.0 ** (14 - math.frexp(am)[1])


def _pack(wt, cin, variant, scale, src_cin=0, c0=0):
    """cs_pack_weight_f16x3_wino_v of wt [cout, src_cin or cin, 3, 3, 3] (cuda, fp32) into NaN-banded allocations ->
    ((alloc, image), (alloc, image)) for hi and lo, images [P, 9, cin16 / 8, cout, 8] fp16"""
    L, _ = _mods()
    cout = wt.shape[0]
    shape = (variant + 2, 9, (cin + 15) // 16 * 2, cout, 8)
    n = math.prod(shape)
    out = []
    for _ in range(2):
        alloc = torch.full((n + 128,), NAN, dtype=torch.float16, device="cuda")
        out.append((alloc, alloc[64:64 + n].view(shape)))
    L.check(L.load().cs_pack_weight_f16x3_wino_v(wt.data_ptr(), out[0][1].data_ptr(), out[1][1].data_ptr(), cout, cin, scale, variant,
                                                 src_cin, c0, None), "cs_pack_weight_f16x3_wino_v")
    torch.cuda.synchronize()
    for alloc, _ in out:
        assert bool(torch.isnan(alloc[:64]).all()) and bool(torch.isnan(alloc[64 + n:]).all()), "the pack wrote outside its images"
    return out


def _workspace(n, fill):
    """n floats inside an allocation with BAND floats before and after: fill = SENTINEL (bit pattern) or NaN"""
    alloc = torch.empty((n + 2 * BAND,), dtype=torch.float32, device="cuda")
    if fill == SENTINEL:
        alloc.view(torch.int32).fill_(SENTINEL)
    else:
        alloc.fill_(fill)
    return alloc, alloc[BAND:BAND + n]


def _bands_hold(alloc, n, fill):
    b = torch.cat([alloc[:BAND], alloc[BAND + n:]])
    return bool((b.view(torch.int32) == SENTINEL).all()) if fill == SENTINEL else bool(torch.isnan(b).all())


def _report(line):
    print("wino_variants " + line)


# ---- 1. the weight pack --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [2, 4], ids=["F(2,3)", "F(4,3)"])
@pytest.mark.parametrize("form", list(W.PACK_FORMS))
def test_weight_pack_against_fp64(variant, form):
    cin, src_cin, c0 = W.PACK_FORMS[form]
    wt, scale, u64 = W.pack_case(form, variant)
    assert scale == _wscale(wt, variant)
    (_, wh), (_, wl) = _pack(wt.cuda(), cin, variant, scale, src_cin, c0)
    u = W.pack_order(u64)
    got = (wh.double().cpu() + wl.double().cpu()) / scale
    assert got.shape == u.shape
    err = (got - u).abs()
    bound = W.pack_bound(u, scale)
    _report(f"pack F{variant} {form}: worst |error| / gate {float((err / bound).max()):.3f}, scale 2^{int(math.log2(scale))}")
    assert bool((err <= bound).all())
    # channels cin .. 16 ceil(cin / 16): exactly zero in both images ([P, tap, cin16 / 8, cout, 8]: channel = kg 8 + j)
    kg0 = cin // 8
    assert (cin % 16 == 0) == (kg0 == wh.shape[2])
    assert bool((wh[:, :, kg0:] == 0).all()) and bool((wl[:, :, kg0:] == 0).all())
    assert float(wh.float().abs().max()) >= 2.0 ** 12              # the scale uses the fp16 range


# ---- 2. the position GEMMs alone -----------------------------------------------------------------------------------------------
_CONV = {}


def _conv_data(c):
    """host inputs of a Conv case, computed once: the operand images (fp16 hi / lo of B^T d a_scale and the value they carry), the
    weights, the fp64 position results of exactly those operands"""
    if c not in _CONV:
        vol = W.GEOM[c.variant][c.geom]
        seed = 3000 + 16 * W.CONVS.index(c)
        y = W.rand(*vol, c.cin, seed=seed) * X_SCALE
        wt = W.rand(c.cout, c.cin, 3, 3, 3, seed=seed + 1) * (27 * c.cin) ** -0.5
        a_scale = 8.0 if c.variant == 2 else 1.0                   # the producers': 16 / 2 resp. 16 / 16
        hi, lo, val = W.split16(W.images64(y.double(), c.variant), a_scale)
        assert float(hi.float().abs().max()) < 65504.0
        ref = W.positions64(val, W.weights64(wt.double(), c.variant))
        _CONV[c] = dict(vol=vol, wt=wt, hi=hi, lo=lo, a_scale=a_scale, ref=ref)
    return _CONV[c]


def _positions_setup(c):
    """the descriptor of a Conv case with its operand images and packed weights on the device; view cases: lda = cin + 8 with NaN
    in the gap, NaN rows before and after"""
    L, ops = _mods()
    t = _conv_data(c)
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


def _unused_output(p, m, cout, keep):
    """the output of a positions-only launch: required by the descriptor's checks, never written (keep[-1]: its allocation)"""
    buf, out = W.sentinel_buffer(m, cout, cout, 0, "cuda")
    p.out, p.ldo = out.data_ptr(), cout
    keep.append(buf)


def _run_positions(p, slices, mt, cout, outbuf, fill=SENTINEL):
    """cs_conv_wino_positions into a pre-filled workspace with bands -> the [slices, P, mt, cout] view (device)"""
    L, ops = _mods()
    npos = (4 if p.a_format == 4 else 2) + 2
    n = slices * npos * mt * cout
    alloc, ws = _workspace(n, fill)
    p.splitk, p.splitk_ws = slices, ws.data_ptr()
    ops.read_status()
    with L.debug_override(**OPEN):
        L.check(L.load().cs_conv_wino_positions(C.byref(p), None), "cs_conv_wino_positions")
        torch.cuda.synchronize()
    assert ops.read_status() == 0
    assert _bands_hold(alloc, n, fill), "a word outside [slices][P][M / R][cout] was written"
    assert bool((outbuf.view(torch.int32) == SENTINEL).all()), "the positions launch wrote to the output"
    return ws.view(slices, npos, mt, cout)


def _check_positions(tag, ws, ref, cin, plan):
    got = ws.double().sum(0).cpu().reshape(-1, ref.shape[-1])
    assert bool(torch.isfinite(got).all()), tag
    r = ref.reshape(-1, ref.shape[-1])
    whole = float((got - r).norm() / r.norm())
    row, col = W.rms_rowcol(got, r)
    _report(f"positions {tag}: plan (slices, units_main, units) {plan} run with {ws.shape[0]} slices on {_cus()} CUs: whole "
            f"{whole:.3e} (gate {gate(9 * cin):.0e}) row {row:.3e} col {col:.3e} (gate {ROW_GATE:.0e})")
    assert whole < gate(9 * cin), (tag, whole)
    assert row < ROW_GATE and col < ROW_GATE, (tag, row, col)


def _assert_grant(c, p):
    """the library grants the variant the case is meant for (F(2,3) stays valid where it would pick F(4,3))"""
    L, _ = _mods()
    with L.debug_override(**OPEN):
        best = _granted(p)
        assert best >= c.variant, (W.conv_id(c), best)
        if c.geom == "W6":
            q = _desc(W.GEOM[2]["W6"], c.cin, c.cout, 4)
            assert best == 2 and _granted(q) == 2                  # W % 4 != 0: the rule answers F(2,3), whatever is asked
        return _plan(p)


@pytest.mark.parametrize("c", W.CONVS, ids=W.conv_id)
def test_position_gemms_alone_at_the_plans_slice_count(c):
    p, keep, mt = _positions_setup(c)
    plan = _assert_grant(c, p)
    assert plan[1] == 0 and plan[2] == (c.variant + 2) * ((c.cout + 223) // 224)       # no tail plan at these sizes
    assert plan[0] == 1 or c.cout % 224 == 0
    ws = _run_positions(p, plan[0], mt, c.cout, keep[-1])
    _check_positions(W.conv_id(c), ws, _conv_data(c)["ref"], c.cin, plan)


# (case, slices): 15 super-chunks of cin = 72 over 4 -> 4 4 4 3; 6 of cin = 24 over 2; 9 of cin = 40 over 3; one slice everywhere
EXPLICIT = [(3, 4), (3, 2), (3, 1), (1, 2), (7, 2), (7, 1), (12, 4), (11, 2), (13, 3), (2, 1)]


@pytest.mark.parametrize("idx,slices", EXPLICIT, ids=[f"{W.conv_id(W.CONVS[i])}-k{s}" for i, s in EXPLICIT])
def test_position_gemms_alone_at_explicit_slice_counts(idx, slices):
    c = W.CONVS[idx]
    nsc = 3 * ((c.cin + 15) // 16)
    per = -(-nsc // slices)
    assert slices == 1 or per * slices * 10 <= nsc * 11          # whole super-chunks, padded by at most a tenth
    p, keep, mt = _positions_setup(c)
    plan = _assert_grant(c, p)
    ws = _run_positions(p, slices, mt, c.cout, keep[-1])
    _check_positions(W.conv_id(c) + f" k{slices}", ws, _conv_data(c)["ref"], c.cin, plan)
    if slices > 1:                                                 # every slice carries a share of the sum
        assert all(float(ws[s].abs().max()) > 0.0 for s in range(slices))


def test_table_of_explicit_slice_counts():
    assert {s for _, s in EXPLICIT} >= {1, 2, 3, 4} and {W.CONVS[i].variant for i, _ in EXPLICIT} == {2, 4}
    assert any(W.CONVS[i].cin == 72 and s == 4 for i, s in EXPLICIT) and any(W.CONVS[i].view for i, _ in EXPLICIT)


# ---- 3. the output transform alone ----------------------------------------------------------------------------------------------
_DUMMY = {}


def _dummy():
    """operand / weight pointers of an output-transform-only launch: required non-null and 16-byte aligned, never read"""
    if not _DUMMY:
        _DUMMY["t"] = torch.zeros(256, dtype=torch.float16, device="cuda")
    return _DUMMY["t"].data_ptr()


def _epilogue_on_device(p, e, cout, view, keep):
    """the epilogue terms of `e` into the descriptor: bias / scale / shift contiguous, row vector and residual in NaN-gapped views
    with their own leading dimensions where `view`"""
    if e.bias is not None:
        keep.append(e.bias.cuda())
        p.bias = keep[-1].data_ptr()
    if e.scale is not None:
        keep += [e.scale.cuda(), e.shift.cuda()]
        p.scale, p.shift = keep[-2].data_ptr(), keep[-1].data_ptr()
    if e.rv is not None:
        keep.append(W.place(e.rv, cout + 4 if view else cout, 4 if view else 0, "cuda"))
        p.rowvec, p.ldrv, p.rv_rows = keep[-1][1].data_ptr(), keep[-1][1].stride(0), e.rv_rows
    if e.res is not None:
        keep.append(W.place(e.res, cout + 8 if view else cout, 4 if view else 0, "cuda"))
        p.res, p.ldr = keep[-1][1].data_ptr(), keep[-1][1].stride(0)
    p.act = e.act


def _out_buffer(m, cout, view, pair=False):
    """sentinel-filled output allocation + view; view cases ldo = cout + 12 at column 4 (pair output: ldo = 16 ceil(cout / 16) + 16 at
    column 16, so that ldo % 16 == 0 and the view starts on 64 bytes)"""
    if pair:
        buf, out = W.sentinel_buffer(m, cout, (cout + 15) // 16 * 16 + 16, 16, "cuda")
        assert out.data_ptr() % 64 == 0
        return buf, out
    return W.sentinel_buffer(m, cout, cout + 12 if view else cout, 4 if view else 0, "cuda")


def _gn_buffer(p, m, cout, rows_per_tile):
    """sentinel-filled fp64 allocation for the partials [tiles][gn_ld = cout + 4][2]"""
    tiles = m // rows_per_tile
    buf, part = W.sentinel_buffer(tiles, 2 * cout, 2 * (cout + 4), 0, "cuda", torch.float64)
    p.gn_part, p.gn_ld, p.gn_rows = part.data_ptr(), cout + 4, rows_per_tile
    return buf, part


def _check_gn(tag, buf, part, out, rows_per_tile):
    """each (tile, column) pair of fp64 sums == the fp64 sum / sum of squares of the kernel's own fp32 output rows of that tile,
    within (rows + 16) 2^-53 of sum |v| resp. sum v^2; the gn_ld gap and the bands untouched"""
    assert W.untouched_outside(buf, part), (tag, "a word outside the partials was written")
    o = out.double().cpu().reshape(-1, rows_per_tile, out.shape[1])
    g = part.cpu().reshape(o.shape[0], out.shape[1], 2)
    tol = (rows_per_tile + 16) * 2.0 ** -53
    assert bool(((g[..., 0] - o.sum(1)).abs() <= tol * o.abs().sum(1)).all()), (tag, "sums")
    assert bool(((g[..., 1] - (o * o).sum(1)).abs() <= tol * (o * o).sum(1)).all()), (tag, "sums of squares")


def _run_output(variant, vol, cout, ws_host, slices, e, view, gn=False, pair_scale=None, expect_status=0, cin=16):
    """cs_conv_wino_output on the workspace ws_host [S, P, Mt, cout] (copied between NaN bands) -> the output view (device).
    cin enters the plan only (which units a slice count cuts): nothing of the operand or the weights is read"""
    L, ops = _mods()
    m = W.rows_of(vol)
    p = _desc(vol, cin, cout, variant)
    p.x = p.x_lo = p.w = p.w_lo = _dummy()
    p.status = ops.status_word(torch.device("cuda", 0)).data_ptr()
    keep = []
    alloc, ws = _workspace(ws_host.numel(), NAN)
    ws.copy_(ws_host.reshape(-1))
    p.splitk, p.splitk_ws = slices, ws.data_ptr()
    _epilogue_on_device(p, e, cout, view, keep)
    buf, out = _out_buffer(m, cout, view, pair_scale is not None)
    p.out, p.ldo = out.data_ptr(), out.stride(0)
    if pair_scale is not None:
        p.out_format, p.out_scale = 2, pair_scale
    gnb = _gn_buffer(p, m, cout, 16 * variant) if gn else None
    ops.read_status()
    with L.debug_override(**OPEN):
        assert _granted(p) >= variant
        L.check(L.load().cs_conv_wino_output(C.byref(p), None), "cs_conv_wino_output")
        torch.cuda.synchronize()
    assert ops.read_status() == expect_status
    assert W.untouched_outside(buf, out), "a word outside the output view was written"
    return out, gnb


def _check_output(tag, out, ref, bound, exact):
    got = out.cpu()
    assert bool(torch.isfinite(got).all()), tag
    ratio = float(((got.double() - ref).abs() / bound).max())
    same = exact is not None and torch.equal(got, exact)
    _report(f"{tag}: worst |error| / E {ratio:.3f}" + ("" if exact is None else f", bit-equal to the fp32 restatement: {same}"))
    assert ratio <= 1.0, (tag, ratio)
    if exact is not None:
        assert same, (tag, "differs from the fp32 restatement in the source's order",
                      int((got != exact).sum()), float((got - exact).abs().max()))


@pytest.mark.parametrize("c", W.OUTS, ids=W.out_id)
def test_output_transform_alone_on_a_synthetic_workspace(c):
    vol = W.GEOM[c.variant][c.geom]
    ws, nsl, e = W.out_case(c)
    ref, bound = W.reference64(ws, nsl, c.variant, e)
    exact = W.kernel32(ws, nsl, c.variant, e) if W.additive_only(e) else None
    out, gnb = _run_output(c.variant, vol, c.cout, ws, c.slices, e, c.view, c.gn)
    _check_output("output " + W.out_id(c), out, ref, bound, exact)
    if c.gn:
        _check_gn(W.out_id(c), gnb[0], gnb[1], out, 16 * c.variant)


@pytest.mark.parametrize("variant", [2, 4], ids=["F(2,3)", "F(4,3)"])
@pytest.mark.parametrize("cout", [64, 224])
def test_output_transform_pair_output_is_the_split_of_the_fp32_result(variant, cout):
    L, _ = _mods()
    vol = W.GEOM[variant]["W4"] if cout == 224 else W.GEOM[variant]["odd-nb"]
    m = W.rows_of(vol)
    ws = W.rand(3, variant + 2, m // variant, cout, seed=500 + cout + variant)
    e = W.epilogue_terms("brr", 6, m, m // vol[0], cout, 600 + cout + variant)
    scale = 16.0
    caps = _desc(vol, 16, cout, variant)
    caps.ldo, caps.out = cout + 16, 64
    pair = C.c_int32(0)
    L.check(L.load().cs_conv_gemm_epilogue_caps(C.byref(caps), None, C.byref(pair)), "cs_conv_gemm_epilogue_caps")
    assert pair.value == 1                                         # the route offers the pair output
    o32, _ = _run_output(variant, vol, cout, ws, 3, e, True)
    words, _ = _run_output(variant, vol, cout, ws, 3, e, True, pair_scale=scale)
    hi, lo = W.pair_decode(words.cpu(), cout)
    ehi, elo = W.pair_expected(o32.cpu(), scale)
    _report(f"output pair F{variant} cout {cout}: hi equal {torch.equal(hi, ehi)}, lo equal {torch.equal(lo, elo)}")
    assert torch.equal(hi, ehi) and torch.equal(lo, elo)
    # a residual of +5000 at out_scale 16 leaves the fp16 range: the launch must say so
    over = e._replace(res=e.res + 5000.0)
    _run_output(variant, vol, cout, ws, 3, over, True, pair_scale=scale, expect_status=L.STATUS_F16X3_OVERFLOW)


# ---- 4. the tail plan at its smallest shape ---------------------------------------------------------------------------------------
# candidates around the two shapes a hand restatement of wino_plan for 256 CUs grants first: (variant, (nb, D, H, W)), cin 32, cout 672
TAIL_CANDIDATES = [(2, (22, 8, 8, 8)), (4, (15, 16, 8, 8)), (2, (23, 8, 8, 8)), (4, (14, 16, 8, 8)), (2, (22, 16, 4, 8)), (4, (16, 16, 8, 8))]
TAIL_CIN, TAIL_COUT = 32, 672
_TAIL = {}


def _tail():
    """the first candidate with units_main > 0, and its plan: asked of the library, not re-derived"""
    if not _TAIL:
        L, _ = _mods()
        seen = []
        with L.debug_override(**OPEN):
            for variant, vol in TAIL_CANDIDATES:
                p = _desc(vol, TAIL_CIN, TAIL_COUT, variant)
                if _granted(p) < variant:
                    seen.append((variant, vol, "not granted"))
                    continue
                plan = _plan(p)
                seen.append((variant, vol, plan))
                if plan[1] > 0:
                    _TAIL.update(variant=variant, vol=vol, plan=plan)
                    break
        _TAIL["seen"] = seen
    print(f"wino_variants tail plan candidates on {_cus()} CUs: {_TAIL['seen']}")
    if "plan" not in _TAIL:
        assert _cus() != 256, f"no candidate takes the tail plan on 256 CUs: {_TAIL['seen']}"
        pytest.skip(f"no candidate takes the tail plan on {_cus()} CUs: {_TAIL['seen']}")
    return _TAIL


def test_tail_plan_positions_leave_the_main_units_later_slices_untouched():
    t = _tail()
    variant, vol, (slices, um, units) = t["variant"], t["vol"], t["plan"]
    y = W.rand(*vol, TAIL_CIN, seed=41) * X_SCALE
    wt = W.rand(TAIL_COUT, TAIL_CIN, 3, 3, 3, seed=42) * (27 * TAIL_CIN) ** -0.5
    a_scale = 8.0 if variant == 2 else 1.0
    hi, lo, val = W.split16(W.images64(y.double(), variant), a_scale)
    L, ops = _mods()
    p = _desc(vol, TAIL_CIN, TAIL_COUT, variant)
    mt = W.rows_of(vol) // variant
    keep = [hi.reshape(-1, TAIL_CIN).cuda(), lo.reshape(-1, TAIL_CIN).cuda()]
    scale = _wscale(wt, variant)
    keep.append(_pack(wt.cuda(), TAIL_CIN, variant, scale))
    p.x, p.x_lo, p.w, p.w_lo = keep[0].data_ptr(), keep[1].data_ptr(), keep[2][0][1].data_ptr(), keep[2][1][1].data_ptr()
    p.a_scale, p.acc_scale = a_scale, 1.0 / (scale * a_scale)
    p.status = ops.status_word(torch.device("cuda", 0)).data_ptr()
    _unused_output(p, W.rows_of(vol), TAIL_COUT, keep)
    ws = _run_positions(p, slices, mt, TAIL_COUT, keep[-1], fill=NAN)
    nsl = W.tail_nsl(variant, TAIL_COUT, slices, um)
    live = (torch.arange(slices)[:, None, None] < nsl[None]).cuda()                   # [S, P, cout]
    fin = torch.isfinite(ws)
    assert bool((fin.all(dim=2) == live).all()) and bool((fin.any(dim=2) == live).all()), \
        "the main units' slices 1 .. must stay untouched, every other word written"
    ref = W.positions64(val, W.weights64(wt.double(), variant))
    got = torch.where(live[:, :, None, :], ws, torch.zeros((), device="cuda"))
    _check_positions(f"tail F{variant} " + "x".join(map(str, vol)), got, ref, TAIL_CIN, t["plan"])


def test_tail_plan_output_transform_reads_one_slice_for_the_main_units():
    t = _tail()
    variant, vol, (slices, um, units) = t["variant"], t["vol"], t["plan"]
    m = W.rows_of(vol)
    nsl = W.tail_nsl(variant, TAIL_COUT, slices, um)
    ws = W.rand(slices, variant + 2, m // variant, TAIL_COUT, seed=43)
    live = torch.arange(slices)[:, None, None, None] < nsl[None, :, None, :]
    ws = torch.where(live, ws, torch.full((), NAN))                # NaN in slices 1 .. of the main units
    e = W.epilogue_terms("brr", "sample", m, m // vol[0], TAIL_COUT, 44)
    ref, bound = W.reference64(ws, nsl, variant, e)
    out, _ = _run_output(variant, vol, TAIL_COUT, ws, slices, e, False, cin=TAIL_CIN)
    _check_output(f"output tail F{variant} plan {t['plan']}", out, ref, bound, W.kernel32(ws, nsl, variant, e))


def test_tail_plan_whole_conv_against_fp64_and_the_uniform_plan():
    """the gates of test_wino_gpu.py::test_tail_plan_of_a_position_launch_that_is_not_whole_rounds at the smallest shape"""
    L, ops = _mods()
    t = _tail()
    variant, vol = t["variant"], t["vol"]
    nb, sp = vol[0], vol[1:]
    rows = sp[0] * sp[1] * sp[2]
    cin, cout = TAIL_CIN, TAIL_COUT
    x = (W.rand(nb, *sp, cin, seed=51) * 1.5 + 0.2).cuda()
    g, b = (W.rand(cin, seed=52) * 0.2 + 1.0).cuda(), (W.rand(cin, seed=53) * 0.2).cuda()
    wt = (W.rand(cout, cin, 3, 3, 3, seed=54) * (cin * 27) ** -0.5).cuda()
    bias, emb, res = W.rand(cout, seed=55).cuda(), W.rand(nb, cout, seed=56).cuda(), W.rand(nb, *sp, cout, seed=57).cuda()
    x[-1], emb[-1], res[-1] = x[0], emb[0], res[0]
    pw = ops.pack_weight_wino(ops.pack_weight(wt, bias, math=L.MATH_F16X3), wt)
    s1 = ops.norm_a_scale(float(g.abs().max()), float(b.abs().max()), rows * (cin // 8))
    outs, plans = {}, {}
    for tail in (1, 0):
        with L.debug_override(no_wino_tail=int(not tail), **OPEN):
            assert ops.wants_wino(nb, *sp, pw) >= variant
            v = ops.groupnorm(x, g, b, 8, 1e-5, L.ACT_SILU, a_scale=s1, wino=variant)
            outs[tail] = ops.conv_gemm(v, pw, rowvec=emb, rv_rows=rows, res=res, stats=True)
            p = ops._wino_desc(nb, *sp, pw)
            p.a_format = 4 if variant == 4 else 3
            plans[tail] = _plan(p)
    torch.cuda.synchronize()
    ops.check_overflow()
    assert plans[1] == t["plan"] and plans[0][1] == 0
    a = F.silu(F.group_norm(x.double().cpu().permute(0, 4, 1, 2, 3), 8, g.double().cpu(), b.double().cpu(), 1e-5))
    ref = F.conv3d(a, wt.double().cpu(), bias.double().cpu(), padding=1).permute(0, 2, 3, 4, 1)
    ref = ref + emb.double().cpu()[:, None, None, None, :] + res.double().cpu()
    e1, e0, e10 = rel_l2(outs[1], ref), rel_l2(outs[0], ref), rel_l2(outs[1], outs[0])
    _report(f"tail whole conv F{variant} " + "x".join(map(str, vol)) + f": tail plan {plans[1]} {e1:.3e}, uniform {plans[0]} {e0:.3e}, "
            f"tail vs uniform {e10:.3e} (gates 1e-6, 1e-6, 1.5e-6) on {_cus()} CUs")
    assert e1 < 1e-6 and e0 < 1e-6 and e10 < 1.5e-6
    for o in outs.values():
        assert torch.equal(o[-1], o[0])                            # the batch position does not enter the arithmetic
        st = ops.groupnorm_stats_from_parts([(0, o.cs_stats)], nb, rows, cout, 32, 1e-5, o.device)
        tt = o.double().reshape(nb, rows, 32, cout // 32)
        mean, var = tt.mean(dim=(1, 3)), tt.var(dim=(1, 3), unbiased=False)
        assert rel_l2(st[..., 0], mean) < 1e-5 and rel_l2(st[..., 1], (var + 1e-5).rsqrt()) < 1e-5


# ---- 5. the whole route as the hosts call it ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", W.CONVS, ids=W.conv_id)
def test_whole_route_against_fp64_and_the_direct_form(c):
    L, ops = _mods()
    vol = W.GEOM[c.variant][c.geom]
    nb, sp = vol[0], vol[1:]
    rows, m = sp[0] * sp[1] * sp[2], W.rows_of(vol)
    seed = 5000 + 16 * W.CONVS.index(c)
    # activations at half scale (gamma) against unit epilogue terms, as test_gemm_variants_gpu.py
    x = (W.rand(nb, *sp, c.cin, seed=seed) * X_SCALE * 3.0 + 0.3).cuda()
    g, b = ((W.rand(c.cin, seed=seed + 1) * 0.2 + 1.0) * X_SCALE).cuda(), (W.rand(c.cin, seed=seed + 2) * 0.1).cuda()
    wt = (W.rand(c.cout, c.cin, 3, 3, 3, seed=seed + 3) * (27 * c.cin) ** -0.5).cuda()
    bias, emb, res = W.rand(c.cout, seed=seed + 4), W.rand(nb, c.cout, seed=seed + 5), W.rand(m, c.cout, seed=seed + 6)
    pw = ops.pack_weight_wino(ops.pack_weight(wt, bias.cuda(), math=L.MATH_F16X3), wt)
    assert pw.wino is not None
    keep = [W.place(emb, c.cout + 4 if c.view else c.cout, 4 if c.view else 0, "cuda"),
            W.place(res, c.cout + 8 if c.view else c.cout, 4 if c.view else 0, "cuda")]
    embv, resv = keep[0][1], keep[1][1].unflatten(0, (nb, *sp))
    buf, out = _out_buffer(m, c.cout, c.view)
    with L.debug_override(no_wino43=int(c.variant == 2), **OPEN):
        got = ops.wants_wino(nb, *sp, pw)
        assert got == c.variant, (W.conv_id(c), got)
        p = ops._wino_desc(nb, *sp, pw)
        p.a_format = 4 if c.variant == 4 else 3
        plan = _plan(p)
        s1 = ops.norm_a_scale(float(g.abs().max()), float(b.abs().max()), rows * (c.cin // 8))
        v = ops.groupnorm(x, g, b, 8, 1e-5, L.ACT_SILU, a_scale=s1, wino=c.variant)
        assert isinstance(v, ops.Wino16) and v.variant == c.variant
        hn = ops.groupnorm(x, g, b, 8, 1e-5, L.ACT_SILU, a_scale=s1, split16=True)
        yw = ops.conv_gemm(v, pw, rowvec=embv, rv_rows=rows, res=resv, stats=True, out=out.unflatten(0, (nb, *sp)))
        yd = ops.conv_gemm(hn, pw, rowvec=embv, rv_rows=rows, res=resv)
        torch.cuda.synchronize()
    ops.check_overflow()
    assert W.untouched_outside(buf, out), "a word outside the output view was written"
    a = F.silu(F.group_norm(x.double().cpu().permute(0, 4, 1, 2, 3), 8, g.double().cpu(), b.double().cpu(), 1e-5))
    ref = F.conv3d(a, wt.double().cpu(), bias.double(), padding=1).permute(0, 2, 3, 4, 1).reshape(m, c.cout)
    ref = ref + emb.double().repeat_interleave(rows, dim=0) + res.double()
    ew, ed = rel_l2(out, ref), rel_l2(yd.reshape(m, c.cout), ref)
    row, col = _rowcol(out, ref)
    rgate = ROW_GATE if c.variant == 2 else 2 * ROW_GATE
    _report(f"route {W.conv_id(c)}: plan (slices, units_main, units) {plan} on {_cus()} CUs: whole {ew:.3e} (direct form {ed:.3e}; "
            f"gates 1e-6 and {2 if c.variant == 2 else 3.5} x direct + 2e-7) row {row:.3e} col {col:.3e} (gate {rgate:.0e})"
            + ("   ** F(4,3) row / column above 1e-6 **" if c.variant == 4 and max(row, col) > 1e-6 else ""))
    assert bool(torch.isfinite(out).all())
    assert ew < 1e-6 and ew < (2 if c.variant == 2 else 3.5) * ed + 2e-7, (ew, ed)
    assert row < rgate and col < rgate, (row, col)
    st = getattr(yw, "cs_stats", None)
    assert st is not None, "the route's epilogue left no GroupNorm partials"
    part = st.part.reshape(-1, 2 * c.cout)
    o = out.double().cpu().reshape(part.shape[0], -1, c.cout)
    gsum = part.cpu().reshape(part.shape[0], c.cout, 2)
    tol = (o.shape[1] + 16) * 2.0 ** -53
    assert o.shape[1] == 16 * c.variant
    assert bool(((gsum[..., 0] - o.sum(1)).abs() <= tol * o.abs().sum(1)).all())
    assert bool(((gsum[..., 1] - (o * o).sum(1)).abs() <= tol * (o * o).sum(1)).all())


# ---- 6. the split-K reduce pair ------------------------------------------------------------------------------------------------------
def _run_reduce(c, e, t, pair_scale=None, gn=None, expect_status=0):
    """cs_conv_gemm with explicit splitk under no_fused_reduce into the test's own NaN workspace -> (out view, ws [S, 1, M, cout]
    (device), gn buffers)"""
    L, ops = _mods()
    m, s = W.rows_of(c.vol), W.red_slices(c)
    gn = c.gn if gn is None else gn
    p = L.CsConvGemm()
    p.nb, p.din, p.hin, p.win = c.vol
    p.dout, p.hout, p.wout = c.vol[1:]
    p.cin, p.cout, p.lda = c.cin, c.cout, c.cin
    p.kd = p.kh = p.kw = 3
    p.sd = p.sh = p.sw = p.pd = p.ph = p.pw = 1
    p.math, p.tile, p.rv_rows = L.MATH_F16X3, c.tile, 1
    pk = t["pk"]
    p.x, p.w, p.w_lo, p.ldw = t["x"].data_ptr(), pk.wh.data_ptr(), pk.wl.data_ptr(), pk.ldw
    p.a_scale, p.acc_scale, p.a_format = ops.A_SCALE, pk.acc_scale, 0
    p.status = ops.status_word(torch.device("cuda", 0)).data_ptr()
    keep = []
    _epilogue_on_device(p, e, c.cout, c.view, keep)
    buf, out = _out_buffer(m, c.cout, c.view, pair_scale is not None)
    p.out, p.ldo = out.data_ptr(), out.stride(0)
    if pair_scale is not None:
        p.out_format, p.out_scale = 2, pair_scale
    gnb = _gn_buffer(p, m, c.cout, 16) if gn else None
    n = s * m * c.cout
    alloc, ws = _workspace(n, NAN)
    p.splitk, p.splitk_ws = s, ws.data_ptr()
    ops.read_status()
    with L.debug_override(no_fused_reduce=1):
        L.check(L.load().cs_conv_gemm(C.byref(p), None), "cs_conv_gemm")
        torch.cuda.synchronize()
    assert ops.read_status() == expect_status
    assert _bands_hold(alloc, n, NAN), "a word outside [slices][M][cout] of the workspace was written"
    assert W.untouched_outside(buf, out), "a word outside the output view was written"
    return out, ws.view(s, 1, m, c.cout), gnb


_RED = {}


def _red_inputs(c):
    L, ops = _mods()
    if c not in _RED:
        seed = 9000 + 16 * W.REDS.index(c)
        x = W.rand(W.rows_of(c.vol), c.cin, seed=seed + 8) * X_SCALE
        wt = W.rand(c.cout, c.cin, 3, 3, 3, seed=seed + 9) * (27 * c.cin) ** -0.5
        conv = F.conv3d(x.double().reshape(*c.vol, c.cin).permute(0, 4, 1, 2, 3), wt.double(), padding=1)
        _RED[c] = dict(x=x.cuda(), wt=wt, conv=conv.permute(0, 2, 3, 4, 1).reshape(-1, c.cout),
                       pk=ops.pack_weight(wt.cuda(), None, cin_pad=c.cin, math=L.MATH_F16X3))
    return _RED[c]


@pytest.mark.parametrize("c", W.REDS, ids=W.red_id)
def test_splitk_reduce_against_the_partial_tiles_the_call_left(c):
    L, _ = _mods()
    t = _red_inputs(c)
    _, _, e = W.red_case(c)
    out, ws_dev, gnb = _run_reduce(c, e, t)
    ws = ws_dev.cpu()
    assert bool(torch.isfinite(ws).all()), "a partial tile was not written"
    part_err = float((ws.double().sum(0)[0] - t["conv"]).norm() / t["conv"].norm())
    assert part_err < gate(27 * c.cin), part_err                  # the slices do sum to the conv
    _, nsl, _ = W.red_case(c, ws)
    ref, bound = W.reference64(ws, nsl, None, e)
    exact = W.kernel32(ws, nsl, None, e) if W.additive_only(e) else None
    kernel = "splitk_reduce_epi_kernel" if c.gn else "splitk_reduce_kernel"
    _check_output(f"reduce {W.red_id(c)} ({kernel}, {ws.shape[0]} slices; slice sum vs fp64 conv {part_err:.2e})", out, ref, bound, exact)
    if c.gn:
        _check_gn(W.red_id(c), gnb[0], gnb[1], out, 16)
    if c.pair:
        scale = 16.0
        words, ws2, gnb2 = _run_reduce(c, e, t, pair_scale=scale)
        assert torch.equal(ws2, ws_dev)
        hi, lo = W.pair_decode(words.cpu(), c.cout)
        ehi, elo = W.pair_expected(out.cpu(), scale)
        _report(f"reduce pair {W.red_id(c)}: hi equal {torch.equal(hi, ehi)}, lo equal {torch.equal(lo, elo)}")
        assert torch.equal(hi, ehi) and torch.equal(lo, elo)
        if c.gn:                                                    # the partials beside the pair output: of the fp32 values
            _check_gn(W.red_id(c) + " pair", gnb2[0], gnb2[1], out, 16)
        if e.res is not None:
            _run_reduce(c, e._replace(res=e.res + 5000.0), t, pair_scale=scale, expect_status=L.STATUS_F16X3_OVERFLOW)


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------
def _refusal_base(c, keep):
    """a complete, valid cs_conv_gemm descriptor of a Conv case (every buffer real and large enough for whatever is asked)"""
    L, ops = _mods()
    p, k, mt = _positions_setup(c)
    keep += k
    m = W.rows_of(W.GEOM[c.variant][c.geom])
    alloc, ws = _workspace(17 * (c.variant + 2) * mt * c.cout, SENTINEL)
    buf, out = W.sentinel_buffer(m, c.cout, c.cout + 12, 4, "cuda")
    keep += [alloc, buf]
    p.out, p.ldo, p.splitk, p.splitk_ws = out.data_ptr(), out.stride(0), 1, ws.data_ptr()
    return p, buf, out, ws


REFUSALS = ["valid", "lda % 8", "splitk 17", "a_bound", "workspace off 16 bytes", "gn_rows", "a_format 4 at W = 6", "ldo % 4",
            "slices padded by more than a tenth"]


@pytest.mark.parametrize("what", REFUSALS)
def test_refusals_leave_the_output_untouched(what):
    L, ops = _mods()
    keep = []
    c = W.CONVS[4] if what == "a_format 4 at W = 6" else W.CONVS[5] if what == "slices padded by more than a tenth" else W.CONVS[1]
    p, buf, out, ws = _refusal_base(c, keep)
    m = out.shape[0]
    if what == "lda % 8":
        assert c.view
        p.lda = c.cin + 4
    elif what == "splitk 17":
        p.splitk = 17
    elif what == "a_bound":
        keep.append(torch.zeros(4, device="cuda"))
        p.a_bound = keep[-1].data_ptr()
    elif what == "workspace off 16 bytes":
        p.splitk_ws = ws.data_ptr() + 4
    elif what == "gn_rows":
        keep.append(W.sentinel_buffer(m // 16, 2 * c.cout, 2 * (c.cout + 4), 0, "cuda", torch.float64))
        p.gn_part, p.gn_ld, p.gn_rows = keep[-1][1].data_ptr(), c.cout + 4, 16          # the F(2,3) statistics tile is 32 rows
    elif what == "a_format 4 at W = 6":
        p.a_format = 4
    elif what == "ldo % 4":
        p.ldo = c.cout + 10
    elif what == "slices padded by more than a tenth":
        # 9 super-chunks (cin = 40) over 2 slices run 5 + 5: the three-tap slab kernel -- the only one that selects a position's
        # weight image -- does not take that count (cs_f16x3_slab_width), so the launch is refused, not run on the gather path
        assert c.cin == 40
        p.splitk = 2
    ops.read_status()
    with L.debug_override(**OPEN):
        rc = L.load().cs_conv_gemm(C.byref(p), None)
        torch.cuda.synchronize()
    if what == "valid":                                            # the base descriptor itself runs
        assert rc == 0 and ops.read_status() == 0 and bool(torch.isfinite(out).all()) and W.untouched_outside(buf, out)
        return
    assert rc == L.CS_EINVAL, (what, rc)
    assert bool((buf.view(torch.int32) == SENTINEL).all()), "a refused launch wrote to the output"
    assert bool((ws.view(torch.int32) == SENTINEL).all()), "a refused launch wrote to the workspace"
    assert ops.read_status() == 0
