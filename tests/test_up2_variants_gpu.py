"""Every route of the folded Upsample conv (cs_conv_gemm_up2, cs_gemm.hip: nearest x2 of the flagged dims + 3x3x3 conv as one
conv per output parity class on the source grid) at ragged shapes against fp64; the table, the restated fold and the way a row
asserts its route are in tests/_up2_cases.py.  The descriptors are built directly (CsConvGemm through ctypes), so that a row can
pass lda > cin, a sentinel-filled workspace and the pre-split operand as views; the routes are selected in-process with
lib.debug_override(no_slab4 / no_up2_direct / no_up2_batch).

1. cs_fold_upsample_weight, all seven doubling patterns, bit for bit against the fp32 sum of the same taps in the kernel's order
   (x, y, z ascending from 0.f), at 5 x 3 channels and at a size beyond one sweep of the capped grid (256 * 32 workgroups of 256).
2. One row per (route, pattern, operand form): against conv_ndhwc in fp64 -- whole tensor under test_f16x3_gpu.py::gate(K) with K
   the executed terms cin kd' kh' kw', the worst output row and column under test_gemm_variants_gpu.py's flat ROW_GATE where
   K < 2000, e_folded < 3 e_direct + 3e-7 against the unfolded 27-tap GPU form -- with the fp32 CPU oracle's own figures printed
   beside the kernel's.  Every row asserts the workspace prefix its route writes (for the sliced class batch: its slice count),
   the untouched band behind cs_conv_gemm_up2_ws_bytes, status 0 and a second run's bits; every second row has its operands as
   views between NaN guard bands (lda > cin at a column offset, ldo > cout inside a sentinel-filled allocation).
3. The sliced class batch against the per-class route at test_k_slices_at_ragged_chunk_counts's 1.5e-6.
4. The bit identities the source claims, on rows d, e and a small one: slab == per-tap gather (no_slab4), scattered store ==
   scratch + interleave (no_up2_direct), one launch over all classes == one per class (no_up2_batch).
5. A NaN sample stays confined on routes 1 (sliced), 2 (one-launch batch) and 4 (scratch).
6. GroupNorm partials of the one-launch route against fp64 column statistics of the kernel's own output, at
   test_kwave_gpu.py::test_kwave_epilogue_outputs_partials_and_pairs's 2e-7.
7. A negative control: with two classes' packed weights exchanged the whole-tensor and worst-row gates fail by > 100 x.
Pre-split operands (a_format = 1): no route refuses them -- the slab kernel reads fp32 only, so both rows run per class on the
per-tap gather into scratch, which their footprint asserts; the reference is fp64 over the fp32 producer output.
Measured values: profiles/up2_variants_parity.txt (nothing here reads them) -- over the table the folded op's worst whole tensor /
row / column were 1.8e-7 / 3.9e-7 / 2.5e-7 in F16X3 and 2.7e-7 / 4.8e-7 / 3.3e-7 in fp32-MFMA, every row on the route and at the
slice count the table states."""
import ctypes as C
from collections import namedtuple

import pytest
import torch

from conftest import rel_l2
from test_f16x3_gpu import gate
from test_gemm_variants_gpu import (POST_ROWS, PRE_ROWS, ROW_GATE, SENTINEL, X_SCALE, _gates, _out_buffer, _place, _rowcol,
                                    _untouched_outside)

import _up2_cases as U

pytestmark = pytest.mark.gpu

BAND = 4096          # words behind cs_conv_gemm_up2_ws_bytes that must stay untouched
Shim = namedtuple("Shim", "vol stride cout view")          # what test_gemm_variants_gpu.py::_out_buffer reads of a case
assert X_SCALE == U.X_SCALE and PRE_ROWS > 0 and POST_ROWS > 0


def _mods():
    from commonscenes_amd import lib as L, ops
    from oracle import ref_ops as R
    return L, ops, R


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.randn(*shape, generator=g) * scale


def _errs(out, ref):
    return (rel_l2(out, ref),) + _rowcol(out, ref)


_DATA = {}


def _data(r):
    """CPU inputs of a row's case, its fp64 result and the fp32 oracle's own errors: computed once, shared by the rows and tests
    of the same case, never modified.  (pre-split rows: the reference follows the producer, see _device)"""
    case = lambda q: (q.up, q.vol, q.cin, q.cout, q.bias, q.act, q.fmt)
    key = case(r)
    if key not in _DATA:
        _, _, R = _mods()
        seed = 2000 + 16 * next(i for i, q in enumerate(U.ROWS) if case(q) == key)      # (the same inputs in any test order)
        t = dict(x=_rand(*r.vol, r.cin, seed=seed) * X_SCALE, g=None, b=None)
        if r.fmt:
            t["x"] = t["x"] * 3.0 + 0.3
            t["g"], t["b"] = (_rand(r.cin, seed=seed + 1) * 0.2 + 1.0) * X_SCALE, _rand(r.cin, seed=seed + 2) * 0.1
        t["wt"] = _rand(r.cout, r.cin, 3, 3, 3, seed=seed + 3, scale=(r.cin * 27) ** -0.5)
        t["bias"] = _rand(r.cout, seed=seed + 4) if r.bias else None
        if not r.fmt:
            _reference(r, t, t["x"], R)
        _DATA[key] = t
    return _DATA[key]


def _reference(r, t, a, R):
    act = "silu" if r.act == "silu" else None
    dbl = lambda v: None if v is None else v.double()
    t["ref"] = R.conv_ndhwc(a.double(), t["wt"].double(), dbl(t["bias"]), (1, 1, 1), r.up, act=act)
    t["oracle"] = _errs(R.conv_ndhwc(a, t["wt"], t["bias"], (1, 1, 1), r.up, act=act), t["ref"])


def _device(r):
    """the row's operands on the device: the activation as the [m1, cin] view the GEMM reads (view rows: at a column offset of
    4 floats / 8 halves inside a NaN-filled allocation with rows before and after), folded and unfolded packed weights"""
    L, ops, R = _mods()
    t = _data(r)
    m1 = U.m1(r)
    x0 = t["x"].cuda()
    gap = lambda unit: (r.cin + 3 * unit, unit) if r.view else (r.cin, 0)
    math = L.MATH_F16X3 if r.math == "f16x3" else L.MATH_FP32
    if r.fmt == 0:
        a, x32 = (_place(x0.view(m1, r.cin), *gap(4)), None), x0
    else:
        ops.SPLIT16_PRODUCERS = True          # (a module-global shadow of the switch: conftest drops it after the test)
        g, b = t["g"].cuda(), t["b"].cuda()
        h16 = ops.groupnorm(x0, g, b, 8, 1e-5, L.ACT_SILU, split16=True, a_scale=ops.A_SCALE)
        assert isinstance(h16, ops.Split16) and h16.hi.dtype == torch.float16 and float(h16.a_scale) == ops.A_SCALE
        x32 = ops.groupnorm(x0, g, b, 8, 1e-5, L.ACT_SILU)
        a = (_place(h16.hi.view(m1, r.cin), *gap(8)), _place(h16.lo.view(m1, r.cin), *gap(8)))
        if "ref" not in t:
            _reference(r, t, x32.cpu(), R)
    wt = t["wt"].cuda()
    bias = t["bias"].cuda() if r.bias else None
    pk = ops.pack_weight(wt, bias, cin_pad=r.cin, math=math, fold_up=r.up)
    assert pk.classes is not None and len(pk.classes) == U.ncls(r) and tuple(pk.up) == r.up
    return dict(a=a, x32=x32, pk=pk, pkd=ops.pack_weight(wt, bias, cin_pad=r.cin, math=math), math=math)


Run = namedtuple("Run", "out prefix part")


def _run(r, dev, sw=None, a=None, order=None):
    """one cs_conv_gemm_up2 of the row's descriptor under the row's (or the given) CsDebug switches, into a fresh sentinel-filled
    output allocation and a fresh sentinel-filled workspace of cs_conv_gemm_up2_ws_bytes + BAND words.  Asserts the return code,
    that no word outside the output view changed, and that the workspace words written are exactly a prefix (so the band is
    untouched); returns the output view, the prefix length and the GroupNorm partials (gn rows)."""
    L, ops, _ = _mods()
    lib = L.load()
    buf, out = _out_buffer(Shim(U.out_vol(r), (1, 1, 1), r.cout, r.view))
    xa, lo = a or dev["a"]
    pk = dev["pk"]
    f16 = dev["math"] == L.MATH_F16X3
    p = U.descriptor(L, r, lda=xa.stride(0), ldo=out.stride(0), ldw=pk.ldw)
    p.x, p.out = xa.data_ptr(), out.data_ptr()
    if r.bias:
        p.bias = pk.bias.data_ptr()
    if f16:
        p.a_scale, p.status = ops.A_SCALE, ops.status_word(xa.device).data_ptr()
        if lo is not None:
            p.x_lo = lo.data_ptr()
    n = U.ncls(r)
    cls = [pk.classes[i] for i in (order or range(n))]          # (order: the negative control's permuted class weights)
    w_arr = (C.c_void_p * n)(*[(c.wh if f16 else c.wt).data_ptr() for c in cls])
    lo_arr = (C.c_void_p * n)(*[(c.wl.data_ptr() if f16 else 0) for c in cls])
    sc_arr = (C.c_float * n)(*[c.acc_scale for c in cls])
    part = None
    with L.debug_override(**({k: 1 for k in r.sw} if sw is None else sw)):
        if r.gn:
            rows, pair = C.c_int32(0), C.c_int32(0)
            L.check(lib.cs_conv_gemm_epilogue_caps(C.byref(p), C.byref(rows), C.byref(pair)), "cs_conv_gemm_epilogue_caps")
            assert (rows.value, pair.value) == (256, 0)
            part = torch.full((n * (U.m1(r) // 256), r.cout, 2), float("nan"), dtype=torch.float64, device="cuda")
            p.gn_part, p.gn_ld, p.gn_rows = part.data_ptr(), r.cout, 256
        wsb = lib.cs_conv_gemm_up2_ws_bytes(C.byref(p))
        assert wsb >= n * U.m1(r) * r.cout * 4 and wsb % 16 == 0, wsb
        ws = torch.empty((wsb // 4 + BAND,), dtype=torch.int32, device="cuda")
        ws.fill_(SENTINEL)
        rc = lib.cs_conv_gemm_up2(C.byref(p), w_arr, lo_arr, sc_arr, ws.data_ptr(), None)
        torch.cuda.synchronize()
    assert rc == 0, rc
    assert _untouched_outside(buf, out), "a word outside the output view was written"
    written = ws != SENTINEL
    prefix = int(written.sum())
    assert prefix <= wsb // 4 and bool(written[:prefix].all()), "the workspace words written are not a prefix inside ws_bytes"
    return Run(out, prefix, part)


def _direct(r, dev):
    """the unfolded 27-tap GPU form of the same op (upsampling as addressing), same math mode"""
    L, ops, _ = _mods()
    out = ops.conv_gemm(dev["x32"], dev["pkd"], up=r.up, act=L.ACT_SILU if r.act == "silu" else L.ACT_NONE)
    torch.cuda.synchronize()
    return out.view(-1, r.cout)


def _report(r, name, out, ref, oracle):
    e = _errs(out, ref)
    print(f"up2_variants {U.row_id(r)} {name}: whole {e[0]:.3e} row {e[1]:.3e} col {e[2]:.3e}   "
          f"(fp32 oracle {oracle[0]:.3e} {oracle[1]:.3e} {oracle[2]:.3e})")
    return e


def _route_name(r, prefix):
    unit = U.m1(r) * r.cout
    return f"prefix {prefix} words = {prefix / unit:g} x m1 cout ({U.ncls(r)} classes)"


# ---- 1. the fold ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("up", U.PATTERNS, ids=lambda u: "".join(map(str, u)))
def test_fold_kernel_is_the_fp32_tap_sum_bit_for_bit(up):
    L, ops, _ = _mods()
    lib = L.load()
    rc, n, kd, kh, kw = U.up2_info(L, up)
    assert rc == 0 and n == 1 << sum(up) and (kd, kh, kw) == tuple(2 if u else 3 for u in up)
    sizes = [(5, 3)] + ([(224, 224)] if up == (1, 1, 1) else [])
    for cout, cin in sizes:
        w = _rand(cout, cin, 3, 3, 3, seed=70 + cout)
        wd = w.cuda()
        wf = torch.full((n, cout, cin, kd, kh, kw), float("nan"), device="cuda")
        L.check(lib.cs_fold_upsample_weight(wd.data_ptr(), wf.data_ptr(), cout, cin, *up, None), "cs_fold_upsample_weight")
        torch.cuda.synchronize()
        want = torch.stack(U.fold(w, up))
        assert wf.numel() > 256 * 32 * 256 or (cout, cin) == (5, 3)
        assert torch.equal(wf.cpu().view(torch.int32), want.view(torch.int32)), (up, cout, cin)
    for bad in ((0, 0, 0), (2, 1, 1), (1, -1, 0)):
        wf = torch.zeros(8 * 15 * 27, device="cuda")
        assert lib.cs_fold_upsample_weight(wf.data_ptr(), wf.data_ptr(), 5, 3, *bad, None) == L.CS_EINVAL


# ---- 2. the table --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", U.ROWS, ids=U.row_id)
def test_route_matrix(r):
    L, ops, _ = _mods()
    dev = _device(r)
    t = _data(r)
    ref, oracle = t["ref"], t["oracle"]
    ops.read_status()
    run = _run(r, dev)
    assert ops.read_status() == 0
    print(f"up2_variants {U.row_id(r)} route {r.route}: {_route_name(r, run.prefix)}")
    e = _report(r, r.math, run.out, ref, oracle)
    direct = _direct(r, dev)
    ed = _report(r, "direct-27", direct, ref, oracle)
    # the route: the workspace prefix the row states (sliced: its slice count, read back from the footprint)
    assert run.prefix == U.prefix_words(r), (r.route, _route_name(r, run.prefix))
    if r.route == "sliced":
        assert run.prefix // (U.ncls(r) * U.m1(r) * r.cout) == r.slices >= 2
    # fp64
    K = U.k_exec(r)
    assert torch.isfinite(run.out).all()
    if K < 2000:
        _gates(U.row_id(r), run.out, e, oracle, gate(K))
    else:
        assert e[0] < gate(K), (e, gate(K))
    assert e[0] < 3 * ed[0] + 3e-7, (e, ed)
    # a second run; status
    again = _run(r, dev)
    assert torch.equal(again.out, run.out) and again.prefix == run.prefix, "a second run differs"
    assert ops.read_status() == 0
    if r.gn:
        _check_partials(r, run)
        assert torch.equal(again.part, run.part)


def _check_partials(r, run):
    """the partials the one-launch route left ([class][sample][256-row tile] x column: fp64 sum and sum of squares), finalised
    by cs_groupnorm_finalize_parts, against the fp64 statistics of the kernel's own output over the doubled grid"""
    L, ops, _ = _mods()
    nb, groups, eps = r.vol[0], 32, 1e-6
    rows_out = U.ncls(r) * (U.m1(r) // nb)
    assert torch.isfinite(run.part).all()
    st = ops.ColStats(run.part, r.cout, nb, (U.m1(r) // nb) // 256, U.ncls(r))
    a = ops.groupnorm_stats_from_parts([(0, st)], nb, rows_out, r.cout, groups, eps, run.out.device)
    torch.cuda.synchronize()
    y = run.out.double().reshape(nb, rows_out, groups, r.cout // groups)
    mean, var = y.mean(dim=(1, 3)), y.var(dim=(1, 3), unbiased=False)
    refst = torch.stack([mean, 1.0 / (var + eps).sqrt()], dim=-1)
    dm = float(((a[..., 0].double() - refst[..., 0]).abs() * refst[..., 1]).max())
    dr = float(((a[..., 1].double() - refst[..., 1]).abs() / refst[..., 1]).max())
    print(f"up2_variants {U.row_id(r)} partials: mean {dm:.3e} rstd {dr:.3e}")
    assert dm < 2e-7 and dr < 2e-7, (dm, dr)


# ---- 3. sliced against per class -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [r for r in U.ROWS if r.route == "sliced"], ids=U.row_id)
def test_sliced_class_batch_against_the_per_class_route(r):
    L, ops, _ = _mods()
    dev = _device(r)
    ops.read_status()
    sliced = _run(r, dev)
    per = _run(r, dev, sw=dict(no_up2_batch=1))
    assert ops.read_status() == 0
    unit = U.m1(r) * r.cout
    assert sliced.prefix == U.ncls(r) * r.slices * unit
    # per class: scratch + interleave, each class cut by plan_splitk or not -- whole class results and whole partial slices
    assert per.prefix % unit == 0 and per.prefix // unit >= U.ncls(r) and per.prefix // unit != U.ncls(r) + 1
    e = rel_l2(sliced.out, per.out)
    print(f"up2_variants {U.row_id(r)} sliced vs per class ({_route_name(r, per.prefix)}): {e:.3e}")
    assert e < 1.5e-6


# ---- 4. bit identities ---------------------------------------------------------------------------------------------------
IDENT = [U.ROWS[0]] + [r for r in U.ROWS if r.piece in ("d", "e") and not r.gn]


@pytest.mark.parametrize("r", IDENT, ids=U.row_id)
def test_bit_identities_between_routes(r):
    """(claim, switches, the footprint the switched launch must show): each gives the row's bits.  Rows d / e run the slab
    kernel with the scattered store; switched off one at a time they fall back to scratch + interleave on the per-tap gather
    (no_slab4), on the slab kernel where a class alone still takes a 256-row tile (no_up2_direct on row e), or to one launch per
    class (no_up2_batch: row d's classes alone are 35 / 16 row tiles -- the 64x64 tile, into scratch)."""
    L, ops, _ = _mods()
    dev = _device(r)
    scratch = U.ncls(r) * U.m1(r) * r.cout
    base = _run(r, dev)
    assert base.prefix == U.prefix_words(r)
    plain = _run(r, dev, sw={})
    claims = [("slab == per-tap gather", dict(no_slab4=1), scratch),
              ("scattered store == scratch + interleave", dict(no_up2_direct=1), scratch),
              ("one launch over all classes == one per class", dict(no_up2_batch=1), 0 if r.piece == "e" else scratch)]
    if r.piece in ("d", "e"):
        assert plain.prefix == 0, "the one-launch batch leaves the workspace untouched"
    assert torch.equal(plain.out, base.out), "row's own switches"
    for claim, sw, want in claims:
        got = _run(r, dev, sw=sw)
        assert got.prefix == want, (claim, _route_name(r, got.prefix))
        assert torch.equal(got.out, base.out), claim
    assert ops.read_status() == 0


# ---- 5. a NaN sample stays confined --------------------------------------------------------------------------------------
CONFINE = [U.ROWS[0], next(r for r in U.ROWS if r.route == "sliced" and r.slices == 9),
           next(r for r in U.ROWS if r.route == "batch" and r.vol[0] == 3)]


@pytest.mark.parametrize("r", CONFINE, ids=U.row_id)
def test_nan_sample_is_confined(r):
    """tiles span samples (315 / 3861 source rows over three samples): the taps a sample's border voxels do not have are masked,
    not read from the neighbouring sample -- with sample 1 all NaN the other samples keep their bits, on routes 4, 1 and 2"""
    L, ops, _ = _mods()
    dev = _device(r)
    clean = _run(r, dev)
    xn = _data(r)["x"].clone()
    xn[1] = float("nan")
    gap = (r.cin + 12, 4) if r.view else (r.cin, 0)
    dirty = _run(r, dev, a=(_place(xn.cuda().view(U.m1(r), r.cin), *gap), None))
    assert dirty.prefix == clean.prefix == U.prefix_words(r)
    nb = r.vol[0]
    c, d = clean.out.reshape(nb, -1), dirty.out.reshape(nb, -1)
    keep = [i for i in range(nb) if i != 1]
    assert torch.equal(d[keep], c[keep]) and bool(torch.isfinite(c).all())
    assert bool(torch.isnan(d[1]).all())
    ops.read_status()


# ---- 6. negative control: the gates see a class that reads another class's weights ---------------------------------------
@pytest.mark.parametrize("r", CONFINE, ids=U.row_id)
def test_gates_flag_swapped_class_weights(r):
    """the last two classes' packed weights exchanged (W parity 0 <-> 1 of the last (pd, ph)): the same launches, the same
    footprint, and a quarter (an eighth) of the output voxels convolved with the neighbouring parity's pre-summed taps -- the
    whole-tensor gate and the worst-row gate must both fail, on routes 4, 1 and 2"""
    L, ops, _ = _mods()
    dev = _device(r)
    t = _data(r)
    n = U.ncls(r)
    bad = _run(r, dev, order=list(range(n - 2)) + [n - 1, n - 2])
    assert bad.prefix == U.prefix_words(r)
    e = _errs(bad.out, t["ref"])
    print(f"up2_variants {U.row_id(r)} swapped class weights: whole {e[0]:.3e} row {e[1]:.3e} col {e[2]:.3e}")
    assert e[0] > 100 * gate(U.k_exec(r)) and e[1] > 100 * ROW_GATE
    ops.read_status()
