"""Every kernel of commonscenes_amd/csrc/cs_norm.hip and every template instantiation behind its extern "C" entries (10 kernels,
16 instantiations at 12 launch sites: gn_finalize_parts_kernel<1|4>, gn_apply_wino_kernel<2,4|4,4>,
and ln_kernel<2|4|8>, ln_pair_kernel<2|4|8> behind one CS_LN_LAUNCH site each, recounted from the source by
test_norm_variants_cpu.py), each at the smallest shape that reaches the geometry branch it is in the table
for (tests/_norm_cases.py: the table, the fp64 references, the bounds).  The entries are called through ctypes so that ld*,
col0, nb_src and ncls are explicit.

Checks per case.  (1) The output against fp64 ELEMENTWISE: |out - ref| <= E with E the bound of _norm_cases.py, built from the
fp64 quantities alone -- no whole-tensor norm, no factor.  (2) stats against fp64: |mean - mu| <= 2u |mu| + 1e-12,
|rstd / rho - 1| <= 2u (u = 2^-24).  (3) bound >= max |x| and equal to the fp64 max(|mu| + sqrt(var (n - 1))) rounded up, within
2 fp32 ulps; a zero tensor leaves the slot at 0.  (4) |lo| <= half an fp16 ulp of hi.  (5) CS_STATUS_F16X3_OVERFLOW set exactly
when the fp64 reference times a_scale reaches 65504.  (6) The bit identities the source claims: cs_groupnorm_parts on the split
route == finalize_parts + apply, _stats_bound == _stats, apply_range over [0, ks) and [ks, c) == apply, split16 == the fp32 apply
output times a_scale split on the host, pair16 == the cs_layernorm output times a_scale split and interleaved on the host,
<4> == <1> under no_gn_fold, a second run == the first.  (7) One-launch against split-route stats within one fp32 ulp.
(8) Every second case of every group has all tensors as views of wider buffers (ldx != ldy, both > c); every output allocation
is pre-filled with 0x5A5AA5A5 including 3 rows before and 5 after the view and must keep it outside the view; inputs carry NaN
in the ld gaps and the bands; the view ends finite; status 0.

c % 4 != 0: cs_groupnorm and cs_groupnorm_parts take their one-launch kernels (scalar accesses) without a c % 4 check, while
their split route (float4) rejects such c -- (2, 9, 21, 3) passes (1)-(2) on the one-launch route and the same call under
gn_small_group = 0 returns CS_EINVAL and writes nothing.  cs_groupnorm_parts used to launch the finalize kernel (stats, bound
written) BEFORE cs_groupnorm_apply turned the call down; it now checks the apply's conditions first.

The min_rows 16 / 4 rule of the apply entries: its 16-row side needs nb ceil(rows / (16 rowlanes)) >= 1024 and differs from the
4-row side in the rows per block only when rows > 4 rowlanes, i.e. from nb rows c 4 >= 16 MB; the table reaches the side
(1024 x 5 x 8), where both give one block per sample.

Measured (profiles/norm_variants_parity.txt): the worst err / E of any output over the table is 0.47 (apply, 1024 x 5 x 8); the
fp32 CPU emulation of the same expression gives 0.47 on the same case.  Statistics: at most 0.98 u; every bound slot exactly the
fp64 value rounded up."""
import ctypes as C

import numpy as np
import pytest
import torch

import _norm_cases as N

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5AA5A5          # bit pattern of untouched output words
PRE, POST = 3, 5               # bands of rows before / after every view
U = N.U


def _mods():
    from commonscenes_amd import lib as L, ops
    return L, L.load(), ops


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- buffers -----------------------------------------------------------------------------------------------------------
def _in(t, view, unit=4):
    """2-D CPU tensor -> its copy as a view of a NaN-filled allocation: bands of rows before and after, and (view) a row
    stride of cols + 3 units at a column offset of one unit"""
    rows, cols = t.shape
    ld, off = (cols + 3 * unit, unit) if view else (cols, 0)
    buf = torch.full((PRE + rows + POST, ld), float("nan"), dtype=t.dtype, device="cuda")
    v = buf[PRE:PRE + rows, off:off + cols]
    v.copy_(t)
    return v


def _out(rows, cols, view, unit=4, dtype=torch.float32):
    """(allocation, [rows, cols] view): every word of the allocation holds the sentinel; (view) row stride cols + 5 units at a
    column offset of two units"""
    ld, off = (cols + 5 * unit, 2 * unit) if view else (cols, 0)
    buf = torch.empty((PRE + rows + POST) * ld, dtype=dtype, device="cuda")
    buf.view(torch.int32).fill_(SENTINEL)
    buf = buf.view(PRE + rows + POST, ld)
    return buf, buf[PRE:PRE + rows, off:off + cols]


def _words(t):
    return t.reshape(-1).view(torch.int32)


def _untouched(buf, v):
    """every word of the allocation outside the view still holds the sentinel"""
    pat = torch.empty_like(buf)
    _words(pat).fill_(SENTINEL)
    chk = buf.clone()
    off = v.storage_offset() - PRE * buf.shape[1]
    chk[PRE:PRE + v.shape[0], off:off + v.shape[1]] = pat[PRE:PRE + v.shape[0], off:off + v.shape[1]]
    return torch.equal(_words(chk), _words(pat))


def _pristine(buf):
    return bool((_words(buf) == SENTINEL).all())


def _slot(dtype=torch.float32):
    """a zeroed word (bound slot / status word) in the middle of a sentinel-filled allocation"""
    buf, v = _out(1, 1, False, dtype=dtype)
    v.zero_()
    return buf, v


def _stats_out(nb, groups):
    buf, v = _out(1, nb * groups * 2, False)
    return buf, v


def _ws(lib, nb, groups):
    return torch.empty(max(1, lib.cs_groupnorm_ws_bytes(nb, groups) // 8), dtype=torch.float64, device="cuda")


def _vec(t):
    return t.cuda().contiguous()


def _ok(rc, what):
    assert rc == 0, (what, rc)


# ---- checks ------------------------------------------------------------------------------------------------------------
_EMU = {}


def _emu(c):
    key = N.case_id(c)
    if key not in _EMU:
        _EMU[key] = N.worst_ratio(N.emulate(c), c)
    return _EMU[key]


def _check_out(c, val, what="out"):
    """(1): elementwise against fp64 under E"""
    r = N.reference(c)
    val = val.detach().double().cpu().reshape(r["ref"].shape)
    assert torch.isfinite(val).all(), (N.case_id(c), what)
    ratio = float(((val - r["ref"]).abs() / r["E"]).max())
    print(f"norm_variants {N.case_id(c)} {what}: err/E {ratio:.3f}   (cpu emulation {_emu(c):.3f})")
    assert ratio <= 1.0, (N.case_id(c), what, ratio)


def _check_stats(c, stats, what="stats"):
    """(2)"""
    r = N.reference(c)
    st = stats.detach().double().cpu().reshape(r["mu"].shape + (2,))
    dm = (st[..., 0] - r["mu"]).abs()
    dr = (st[..., 1] / r["rho"] - 1.0).abs()
    print(f"norm_variants {N.case_id(c)} {what}: mean {float((dm / (U * r['mu'].abs()).clamp_min(1e-300)).max()):.2f} u "
          f"rstd {float(dr.max() / U):.2f} u   (gate 2 u each)")
    assert bool((dm <= 2.0 * U * r["mu"].abs() + 1e-12).all()), (N.case_id(c), what, "mean")
    assert bool((dr <= 2.0 * U).all()), (N.case_id(c), what, "rstd")


def _check_bound(c, slot, what="bound"):
    """(3)"""
    b = np.float32(float(slot.item()))
    ref = N.reference(c)["bound"]
    up = np.float32(ref)
    if float(up) < ref:
        up = np.nextafter(up, np.float32(np.inf))
    xmax = float(N.data(c)["x"].abs().max())
    ulps = (float(b) - float(up)) / float(np.spacing(up))
    print(f"norm_variants {N.case_id(c)} {what}: {float(b):.6f} = {float(b) / xmax:.2f} max|x|, {ulps:+.0f} ulp from the fp64 value rounded up")
    assert float(b) >= xmax and abs(ulps) <= 2, (N.case_id(c), what, float(b), ref, xmax)


def _ulp_equal(a, b):
    """(7): within one fp32 ulp"""
    a, b = a.reshape(-1), b.reshape(-1)
    ulp = torch.nextafter(b.abs(), torch.full_like(b, float("inf"))) - b.abs()
    return bool(((a - b).abs() <= ulp).all())


def _check_pair(hi, lo, what):
    """(4): |lo| <= half an fp16 ulp of hi"""
    h, l = hi.detach().cpu().double().abs(), lo.detach().cpu().double().abs()
    expo = torch.frexp(h.clamp_min(2.0 ** -14))[1]               # h = m 2^expo, m in [0.5, 1): exact, unlike log2
    ulp = torch.ldexp(torch.ones_like(h), expo - 11)              # 2^-24 from the smallest normal down
    assert bool((l <= 0.5 * ulp).all()), what


def _bits16(t):
    return t.contiguous().view(torch.int16)


# ---- case plumbing -----------------------------------------------------------------------------------------------------
def _gn_operands(c):
    """x view [nb * rows, ctot] (NaN gaps and bands), gamma, beta on the device"""
    t = N.data(c)
    nb, rows, ch = N.dims(c)
    return _in(t["x"].reshape(nb * rows, ch), c.view), _vec(t["g"]), _vec(t["b"])


def _ref_stats(c):
    """the fp64 statistics rounded to fp32, as the [nb][groups][2] input of an apply entry"""
    r = N.reference(c)
    return torch.stack([r["mu"].float(), r["rho"].float()], dim=-1).contiguous().cuda()


def _segs(c, L):
    """CsGnSeg array of the case's host-built fp64 partials (NaN in the ld gaps and in bands around each array)"""
    keep, arr, k0 = [], (L.CsGnSeg * len(c.o["segs"]))(), 0
    for i, ((nch, tps, ncls, nb_src, col0, pad), p) in enumerate(zip(c.o["segs"], N.partials(c))):
        buf = torch.full((16 + p.numel() + 16,), float("nan"), dtype=torch.float64, device="cuda")
        buf[16:16 + p.numel()].copy_(p.reshape(-1))
        keep.append(buf)
        arr[i] = L.CsGnSeg(buf[16:].data_ptr(), col0 + nch + pad, col0, k0, nch, tps, ncls, nb_src, 0)
        k0 += nch
    return arr, keep


def _ids(group):
    return dict(argvalues=N.BY_GROUP[group], ids=[N.case_id(c) for c in N.BY_GROUP[group]])


# ---- stats: gn_partial_kernel + gn_finalize_kernel ------------------------------------------------------------------------
@pytest.mark.parametrize("c", **_ids("stats"))
def test_stats(c):
    L, lib, _ = _mods()
    nb, rows, ch = c.shape
    x, _, _ = _gn_operands(c)
    ws = _ws(lib, nb, c.groups)
    runs = []
    for _ in range(2):
        sb, st = _stats_out(nb, c.groups)
        _ok(lib.cs_groupnorm_stats(x.data_ptr(), nb, rows, ch, x.stride(0), c.groups, N.EPS, ws.data_ptr(), st.data_ptr(), _stream()),
            "stats")
        runs.append((sb, st))
    sb2, st2 = _stats_out(nb, c.groups)
    bb, slot = _slot()
    _ok(lib.cs_groupnorm_stats_bound(x.data_ptr(), nb, rows, ch, x.stride(0), c.groups, N.EPS, ws.data_ptr(), st2.data_ptr(),
                                     slot.data_ptr(), _stream()), "stats_bound")
    torch.cuda.synchronize()
    _check_stats(c, runs[0][1])
    _check_bound(c, slot)
    assert torch.equal(runs[0][1], runs[1][1]), "a second run differs"
    assert torch.equal(runs[0][1], st2), "_stats_bound != _stats"
    assert all(_untouched(b, v) for b, v in runs + [(sb2, st2), (bb, slot)])


# ---- finalize_parts: gn_finalize_parts_kernel<1> / <4> --------------------------------------------------------------------
def _finalize(c, L, lib, segs, stats=True, bound=True):
    nb, rows, ch = c.shape
    sb, st = _stats_out(nb, c.groups)
    bb, slot = _slot()
    _ok(lib.cs_groupnorm_finalize_parts(segs, len(segs), nb, rows, ch, c.groups, N.EPS, st.data_ptr() if stats else None,
                                        slot.data_ptr() if bound else None, _stream()), "finalize_parts")
    return sb, st, bb, slot


@pytest.mark.parametrize("c", **_ids("finalize_parts"))
def test_finalize_parts(c):
    L, lib, _ = _mods()
    segs, keep = _segs(c, L)
    sb, st, bb, slot = _finalize(c, L, lib, segs)
    sb2, st2, bb2, slot2 = _finalize(c, L, lib, segs)
    sb3, st3, bb3, slot3 = _finalize(c, L, lib, segs, bound=False)
    sb4, st4, bb4, slot4 = _finalize(c, L, lib, segs, stats=False)
    torch.cuda.synchronize()
    _check_stats(c, st)
    _check_bound(c, slot)
    assert torch.equal(st, st2) and torch.equal(slot, slot2), "a second run differs"
    assert torch.equal(st, st3) and float(slot3.item()) == 0.0 and torch.equal(slot, slot4) and _pristine(sb4)
    if "gn_finalize_parts_kernel<4>" in c.kernels:
        with L.debug_override(no_gn_fold=1):
            sb5, st5, bb5, slot5 = _finalize(c, L, lib, segs)
            torch.cuda.synchronize()
        assert torch.equal(st, st5) and torch.equal(slot, slot5), "<4> != <1>"
        assert _untouched(sb5, st5) and _untouched(bb5, slot5)
    for b, v in ((sb, st), (sb2, st2), (sb3, st3), (bb, slot), (bb2, slot2), (bb3, slot3), (bb4, slot4)):
        assert _untouched(b, v)


# ---- parts: gn_small_parts_kernel, and the split route ----------------------------------------------------------------------
def _parts(c, L, lib, x, g, b, segs, gsg=None):
    nb, rows, ch = c.shape
    yb, y = _out(nb * rows, ch, c.view)
    sb, st = _stats_out(nb, c.groups)
    bb, slot = _slot()
    call = lambda: lib.cs_groupnorm_parts(x.data_ptr(), segs, len(segs), g.data_ptr(), b.data_ptr(), y.data_ptr(), nb, rows, ch,
                                          x.stride(0), y.stride(0), c.groups, N.EPS, c.act, st.data_ptr(), slot.data_ptr(), _stream())
    if gsg is None:
        rc = call()
    else:
        with L.debug_override(gn_small_group=gsg):
            rc = call()
    return rc, (yb, y), (sb, st), (bb, slot)


@pytest.mark.parametrize("c", **_ids("parts"))
def test_parts_one_launch(c):
    L, lib, _ = _mods()
    nb, rows, ch = c.shape
    assert N.rsplit_rule(nb, rows, ch, c.groups) == c.o["rsplit"] and rows * (ch // c.groups) <= L.debug().gn_small_group
    x, g, b = _gn_operands(c)
    segs, keep = _segs(c, L)
    rc, Y, S, B = _parts(c, L, lib, x, g, b, segs)
    rc2, Y2, S2, B2 = _parts(c, L, lib, x, g, b, segs)
    rc3, Y3, S3, B3 = _parts(c, L, lib, x, g, b, segs, gsg=0)
    torch.cuda.synchronize()
    assert rc == 0 and rc2 == 0
    _check_out(c, Y[1])
    _check_stats(c, S[1])
    _check_bound(c, B[1])
    assert torch.equal(Y[1], Y2[1]) and torch.equal(S[1], S2[1]) and torch.equal(B[1], B2[1]), "a second run differs"
    for buf, v in (Y, S, B, Y2, S2, B2):
        assert _untouched(buf, v)
    if ch % 4:
        # the split route is float4: it turns the call down, before any launch
        assert rc3 == L.CS_EINVAL and _pristine(Y3[0]) and _pristine(S3[0]) and float(B3[1].item()) == 0.0 and _untouched(*B3)
    else:
        assert rc3 == 0
        _check_out(c, Y3[1], "out (split route)")
        assert _ulp_equal(S[1], S3[1]), "one-launch vs split-route stats"
        assert torch.equal(B[1], B3[1]) and _untouched(*Y3) and _untouched(*S3)


@pytest.mark.parametrize("c", **_ids("parts_split"))
def test_parts_split_route(c):
    L, lib, _ = _mods()
    nb, rows, ch = c.shape
    x, g, b = _gn_operands(c)
    segs, keep = _segs(c, L)
    rc, Y, S, B = _parts(c, L, lib, x, g, b, segs, gsg=c.o["gsg"])
    rc2, Y2, S2, B2 = _parts(c, L, lib, x, g, b, segs, gsg=c.o["gsg"])
    sb, st, bb, slot = _finalize(c, L, lib, segs)
    yb, y = _out(nb * rows, ch, c.view)
    _ok(lib.cs_groupnorm_apply(x.data_ptr(), st.data_ptr(), g.data_ptr(), b.data_ptr(), y.data_ptr(), nb, rows, ch, x.stride(0),
                               y.stride(0), c.groups, c.act, _stream()), "apply")
    torch.cuda.synchronize()
    assert rc == 0 and rc2 == 0
    _check_out(c, Y[1])
    _check_stats(c, S[1])
    _check_bound(c, B[1])
    assert torch.equal(Y[1], y) and torch.equal(S[1], st) and torch.equal(B[1], slot), "parts != finalize_parts + apply"
    assert torch.equal(Y[1], Y2[1]) and torch.equal(S[1], S2[1]), "a second run differs"
    for buf, v in (Y, S, B, Y2, S2, B2, (yb, y), (sb, st)):
        assert _untouched(buf, v)


# ---- small: gn_small_kernel ---------------------------------------------------------------------------------------------
def _groupnorm(c, L, lib, x, g, b, ws, gsg=None):
    nb, rows, ch = c.shape
    yb, y = _out(nb * rows, ch, c.view)
    sb, st = _stats_out(nb, c.groups)
    call = lambda: lib.cs_groupnorm(x.data_ptr(), g.data_ptr(), b.data_ptr(), y.data_ptr(), nb, rows, ch, x.stride(0), y.stride(0),
                                    c.groups, N.EPS, c.act, ws.data_ptr(), st.data_ptr(), _stream())
    if gsg is None:
        rc = call()
    else:
        with L.debug_override(gn_small_group=gsg):
            rc = call()
    return rc, (yb, y), (sb, st)


@pytest.mark.parametrize("c", **_ids("small"))
def test_small(c):
    L, lib, _ = _mods()
    nb, rows, ch = c.shape
    x, g, b = _gn_operands(c)
    ws = _ws(lib, nb, c.groups)
    rc, Y, S = _groupnorm(c, L, lib, x, g, b, ws)
    rc2, Y2, S2 = _groupnorm(c, L, lib, x, g, b, ws)
    rc3, Y3, S3 = _groupnorm(c, L, lib, x, g, b, ws, gsg=0)
    torch.cuda.synchronize()
    assert rc == 0 and rc2 == 0
    _check_out(c, Y[1])
    _check_stats(c, S[1])
    assert torch.equal(Y[1], Y2[1]) and torch.equal(S[1], S2[1]), "a second run differs"
    assert all(_untouched(buf, v) for buf, v in (Y, S, Y2, S2))
    if ch % 4:
        assert rc3 == L.CS_EINVAL and _pristine(Y3[0]) and _pristine(S3[0])
    elif c.o.get("route") == "split":
        # cpg > 256: the default call already ran statistics + apply -- the same launches as under gn_small_group = 0
        assert ch // c.groups > 256 and rc3 == 0 and torch.equal(S[1], S3[1]) and torch.equal(Y[1], Y3[1])
    else:
        assert rc3 == 0 and _ulp_equal(S[1], S3[1]), "one-launch vs split-route stats"
        _check_out(c, Y3[1], "out (split route)")
        assert _untouched(*Y3) and _untouched(*S3)


# ---- apply: gn_apply_kernel ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", **_ids("apply"))
def test_apply(c):
    L, lib, _ = _mods()
    nb, rows, ctot = c.shape
    ch0, nc = N.chan_range(c)
    cpg = ctot // c.groups
    x, g, b = _gn_operands(c)
    st = _ref_stats(c)
    xr = x[:, ch0:ch0 + nc]
    rng = lambda xx, yy, k0, n: lib.cs_groupnorm_apply_range(xx.data_ptr(), st.data_ptr(), g[k0:].data_ptr(), b[k0:].data_ptr(),
                                                             yy.data_ptr(), nb, rows, n, x.stride(0), yy.stride(0), c.groups, cpg, k0,
                                                             c.act, _stream())
    outs = []
    for _ in range(2):
        yb, y = _out(nb * rows, nc, c.view)
        if "ch0" in c.o:
            _ok(rng(xr, y, ch0, nc), "apply_range")
        else:
            _ok(lib.cs_groupnorm_apply(x.data_ptr(), st.data_ptr(), g.data_ptr(), b.data_ptr(), y.data_ptr(), nb, rows, nc,
                                       x.stride(0), y.stride(0), c.groups, c.act, _stream()), "apply")
        outs.append((yb, y))
    # the two ranges [ch0, ch0 + ks) and [ch0 + ks, ch0 + nc) into one output
    ks = 4 * max(1, nc // 8)
    yb2, y2 = _out(nb * rows, nc, c.view)
    _ok(rng(xr[:, :ks], y2[:, :ks], ch0, ks), "range 1")
    if nc > ks:
        _ok(rng(xr[:, ks:], y2[:, ks:], ch0 + ks, nc - ks), "range 2")
    torch.cuda.synchronize()
    _check_out(c, outs[0][1])
    assert torch.equal(outs[0][1], outs[1][1]), "a second run differs"
    assert torch.equal(outs[0][1], y2), "the two channel ranges != the whole"
    assert all(_untouched(buf, v) for buf, v in outs + [(yb2, y2)])


# ---- split16: gn_apply_split16_kernel -------------------------------------------------------------------------------------
def _split16(c, lib, x, g, b, st, s, status):
    nb, rows, ctot = c.shape
    ch0, nc = N.chan_range(c)
    H, Lo = _out(nb * rows, nc, c.view, 8, torch.float16), _out(nb * rows, nc, c.view, 8, torch.float16)
    xr = x[:, ch0:ch0 + nc]
    if "ch0" in c.o:
        rc = lib.cs_groupnorm_apply_split16_range(xr.data_ptr(), st.data_ptr(), g[ch0:].data_ptr(), b[ch0:].data_ptr(), H[1].data_ptr(),
                                                  Lo[1].data_ptr(), nb, rows, nc, x.stride(0), H[1].stride(0), c.groups,
                                                  ctot // c.groups, ch0, c.act, s, status.data_ptr(), _stream())
    else:
        rc = lib.cs_groupnorm_apply_split16(x.data_ptr(), st.data_ptr(), g.data_ptr(), b.data_ptr(), H[1].data_ptr(), Lo[1].data_ptr(),
                                            nb, rows, nc, x.stride(0), H[1].stride(0), c.groups, c.act, s, status.data_ptr(), _stream())
    _ok(rc, "split16")
    return H, Lo


@pytest.mark.parametrize("c", **_ids("split16"))
def test_split16(c):
    L, lib, _ = _mods()
    nb, rows, ctot = c.shape
    ch0, nc = N.chan_range(c)
    s = c.o["s"]
    x, g, b = _gn_operands(c)
    st = _ref_stats(c)
    stb, status = _slot(torch.int32)
    H, Lo = _split16(c, lib, x, g, b, st, s, status)
    H2, Lo2 = _split16(c, lib, x, g, b, st, s, status)
    yb, y = _out(nb * rows, nc, c.view)
    _ok(lib.cs_groupnorm_apply_range(x[:, ch0:].data_ptr(), st.data_ptr(), g[ch0:].data_ptr(), b[ch0:].data_ptr(), y.data_ptr(), nb, rows,
                                     nc, x.stride(0), y.stride(0), c.groups, ctot // c.groups, ch0, c.act, _stream()), "apply_range")
    torch.cuda.synchronize()
    hi, lo = H[1], Lo[1]
    assert torch.isfinite(hi).all() and torch.isfinite(lo).all()
    _check_out(c, (hi.double() + lo.double()) / s, "(hi + lo) / s")
    _check_pair(hi, lo, N.case_id(c))
    o = y * s
    hh = o.half()
    assert torch.equal(_bits16(hi), _bits16(hh)) and torch.equal(_bits16(lo), _bits16((o - hh.float()).half())), \
        "split16 != the fp32 apply output x a_scale, split on the host"
    assert torch.equal(_bits16(hi), _bits16(H2[1])) and torch.equal(_bits16(lo), _bits16(Lo2[1])), "a second run differs"
    assert int(status.item()) == 0 and _untouched(stb, status)
    assert all(_untouched(buf, v) for buf, v in (H, Lo, H2, Lo2, (yb, y)))


# ---- wino: gn_apply_wino_kernel<2, 4>, gn_apply_wino_kernel<4, 4> ----------------------------------------------------------------
def _wino(c, lib, x, g, b, st, s, status, entry="range"):
    nb, d, h, w, ctot = c.shape
    ch0, nc = N.chan_range(c)
    var = c.o["variant"]
    q, r = len(N.BT[var]), nb * d * h * (w // var)
    H, Lo = _out(q * r, nc, c.view, 8, torch.float16), _out(q * r, nc, c.view, 8, torch.float16)
    xr = x[:, ch0:ch0 + nc]
    head = (xr.data_ptr(), st.data_ptr(), g[ch0:].data_ptr(), b[ch0:].data_ptr(), H[1].data_ptr(), Lo[1].data_ptr(), nb, d, h, w, nc,
            x.stride(0), H[1].stride(0), c.groups)
    cpg = ctot // c.groups
    if entry == "range":
        rc = lib.cs_groupnorm_apply_wino_range(*head, cpg, ch0, c.act, s, var, status.data_ptr(), _stream())
    elif entry == "wino16_range":
        rc = lib.cs_groupnorm_apply_wino16_range(*head, cpg, ch0, c.act, s, status.data_ptr(), _stream())
    else:
        rc = lib.cs_groupnorm_apply_wino16(*head, c.act, s, status.data_ptr(), _stream())
    _ok(rc, entry)
    return H, Lo


def _wino_case(c):
    L, lib, _ = _mods()
    s = c.o["s"]
    x, g, b = _gn_operands(c)
    st = _ref_stats(c)
    stb, status = _slot(torch.int32)
    H, Lo = _wino(c, lib, x, g, b, st, s, status)
    runs = [_wino(c, lib, x, g, b, st, s, status)]
    if c.o["variant"] == 2:                 # the F(2,3) entries of the earlier ABI are the same launch
        runs.append(_wino(c, lib, x, g, b, st, s, status, "wino16_range" if "ch0" in c.o else "wino16"))
    torch.cuda.synchronize()
    hi, lo = H[1], Lo[1]
    assert torch.isfinite(hi).all() and torch.isfinite(lo).all()
    _check_out(c, (hi.double() + lo.double()) / s, "images (hi + lo) / s")
    _check_pair(hi, lo, N.case_id(c))
    for H2, Lo2 in runs:
        assert torch.equal(_bits16(hi), _bits16(H2[1])) and torch.equal(_bits16(lo), _bits16(Lo2[1])), "a second run differs"
        assert _untouched(*H2) and _untouched(*Lo2)
    assert int(status.item()) == 0 and _untouched(stb, status) and _untouched(*H) and _untouched(*Lo)


@pytest.mark.parametrize("c", **_ids("wino23"))
def test_wino23(c):
    _wino_case(c)


@pytest.mark.parametrize("c", **_ids("wino43"))
def test_wino43(c):
    _wino_case(c)


# ---- layernorm: ln_kernel<2|4|8>, ln_pair_kernel<2|4|8> -------------------------------------------------------------------
def _layernorm(c, lib, x, g, b):
    m, ch = c.shape
    yb, y = _out(m, ch, c.view)
    _ok(lib.cs_layernorm(x.data_ptr(), g.data_ptr(), b.data_ptr(), y.data_ptr(), m, ch, x.stride(0), y.stride(0), N.EPS, _stream()),
        "layernorm")
    return yb, y


@pytest.mark.parametrize("c", **_ids("layernorm"))
def test_layernorm(c):
    L, lib, _ = _mods()
    t = N.data(c)
    x, g, b = _in(t["x"][0], c.view), _vec(t["g"]), _vec(t["b"])
    Y, Y2 = _layernorm(c, lib, x, g, b), _layernorm(c, lib, x, g, b)
    torch.cuda.synchronize()
    _check_out(c, Y[1])
    assert torch.equal(Y[1], Y2[1]), "a second run differs"
    assert _untouched(*Y) and _untouched(*Y2)


def _pair16(c, lib, x, g, b, s, status):
    """the output as halves: [m, 2 c] inside an allocation whose row stride is 2 ldy halves (ldy floats)"""
    m, ch = c.shape
    yb, y = _out(m, 2 * ch, c.view, 32, torch.float16)
    _ok(lib.cs_layernorm_pair16(x.data_ptr(), g.data_ptr(), b.data_ptr(), y.data_ptr(), m, ch, x.stride(0), y.stride(0) // 2, N.EPS, s,
                                status.data_ptr(), _stream()), "pair16")
    return yb, y


def _decode_pair(y, m, ch):
    """[hi c0-7 | lo c0-7 | hi c8-15 | lo c8-15] per row and 16-channel chunk -> hi, lo [m, c]"""
    v = y.reshape(m, ch // 16, 2, 2, 8)
    return v[:, :, :, 0, :].reshape(m, ch), v[:, :, :, 1, :].reshape(m, ch)


@pytest.mark.parametrize("c", **_ids("pair16"))
def test_pair16(c):
    L, lib, _ = _mods()
    m, ch = c.shape
    s = c.o["s"]
    t = N.data(c)
    x, g, b = _in(t["x"][0], c.view), _vec(t["g"]), _vec(t["b"])
    stb, status = _slot(torch.int32)
    Y, Y2 = _pair16(c, lib, x, g, b, s, status), _pair16(c, lib, x, g, b, s, status)
    Y32 = _layernorm(c, lib, x, g, b)
    torch.cuda.synchronize()
    hi, lo = _decode_pair(Y[1], m, ch)
    assert torch.isfinite(Y[1]).all()
    _check_out(c, (hi.double() + lo.double()) / s, "(hi + lo) / s")
    _check_pair(hi, lo, N.case_id(c))
    o = Y32[1] * s
    hh = o.half()
    ll = (o - hh.float()).half()
    host = torch.stack([hh.reshape(m, ch // 16, 2, 8), ll.reshape(m, ch // 16, 2, 8)], dim=3).reshape(m, 2 * ch)
    assert torch.equal(_bits16(Y[1]), _bits16(host)), "pair16 != the cs_layernorm output x a_scale, split and interleaved on the host"
    assert torch.equal(_bits16(Y[1]), _bits16(Y2[1])), "a second run differs"
    assert int(status.item()) == 0 and _untouched(stb, status) and _untouched(*Y) and _untouched(*Y2) and _untouched(*Y32)


# ---- (5) the overflow flag ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["split16", "wino23", "wino43", "pair16"])
def test_overflow_flag_exactly_when_the_reference_reaches_65504(kind):
    """a_scale = 65504 / max |ref| times (1 +- 2^-10): fp32 evaluates the expression to a few 2^-24, so the fp64 reference times
    a_scale is clear of 65504 on either side"""
    L, lib, _ = _mods()
    c = N.BY_GROUP[kind][0]
    top = float(N.reference(c)["ref"].abs().max())
    t = N.data(c)
    for over in (True, False):
        s = 65504.0 / top * (1.0 + (1 if over else -1) * 2.0 ** -10)
        assert (top * float(np.float32(s)) >= 65504.0) == over
        stb, status = _slot(torch.int32)
        if kind == "pair16":
            x, g, b = _in(t["x"][0], c.view), _vec(t["g"]), _vec(t["b"])
            outs = [_pair16(c, lib, x, g, b, s, status)]
        else:
            x, g, b = _gn_operands(c)
            outs = list((_split16 if kind == "split16" else _wino)(c, lib, x, g, b, _ref_stats(c), s, status))
        torch.cuda.synchronize()
        assert int(status.item()) == (L.STATUS_F16X3_OVERFLOW if over else 0), (kind, over, int(status.item()))
        assert _untouched(stb, status) and all(_untouched(buf, v) for buf, v in outs)


# ---- (3) a zero tensor leaves the bound slot at 0 ---------------------------------------------------------------------------
def test_zero_tensor_leaves_the_bound_at_zero():
    L, lib, _ = _mods()
    nb, rows, ch, groups = 2, 37, 24, 3
    x = _in(torch.zeros(nb * rows, ch), True)
    g, b = _vec(torch.ones(ch)), _vec(torch.zeros(ch))
    ws = _ws(lib, nb, groups)
    slots = [_slot() for _ in range(3)]
    sb, st = _stats_out(nb, groups)
    _ok(lib.cs_groupnorm_stats_bound(x.data_ptr(), nb, rows, ch, x.stride(0), groups, N.EPS, ws.data_ptr(), st.data_ptr(),
                                     slots[0][1].data_ptr(), _stream()), "stats_bound")
    part = torch.zeros(1, nb, 4, ch, 2, dtype=torch.float64, device="cuda")
    segs = (L.CsGnSeg * 1)(L.CsGnSeg(part.data_ptr(), ch, 0, 0, ch, 4, 1, nb, 0))
    _ok(lib.cs_groupnorm_finalize_parts(segs, 1, nb, rows, ch, groups, N.EPS, st.data_ptr(), slots[1][1].data_ptr(), _stream()), "finalize")
    yb, y = _out(nb * rows, ch, True)
    _ok(lib.cs_groupnorm_parts(x.data_ptr(), segs, 1, g.data_ptr(), b.data_ptr(), y.data_ptr(), nb, rows, ch, x.stride(0), y.stride(0),
                               groups, N.EPS, N.ACT_SILU, st.data_ptr(), slots[2][1].data_ptr(), _stream()), "parts")
    torch.cuda.synchronize()
    for buf, v in slots:
        assert int(_words(v).item()) == 0 and _untouched(buf, v)
    assert bool((y == 0).all()) and _untouched(yb, y) and _untouched(sb, st)
    assert bool((st.reshape(-1, 2)[:, 0] == 0).all())


# ---- rejections: CS_EINVAL with no launch -----------------------------------------------------------------------------------
def test_rejections_return_einval_and_write_nothing():
    L, lib, _ = _mods()
    big = lambda dtype=torch.float32: _out(256, 256, False, dtype=dtype)          # 256 KB of sentinel: nothing may land in it
    xin = torch.randn(256 * 300, device="cuda")                                    # generous: no geometry below could leave it
    g, b = torch.ones(4096, device="cuda"), torch.zeros(4096, device="cuda")
    ws = _ws(lib, 4, 257)
    (yb, y), (sb, st), (hb, hi), (lb, lo) = big(), big(), big(torch.float16), big(torch.float16)
    bb, slot = _slot()
    stb, status = _slot(torch.int32)
    stats_in = torch.zeros(4 * 257 * 2, device="cuda")
    stats_in[1::2] = 1.0
    part = torch.zeros(2 * 4 * 8 * 40 * 2 + 2, dtype=torch.float64, device="cuda")
    S = _stream()
    X, G, B, Y, ST, HI, LO, WS = (v.data_ptr() for v in (xin, g, b, y, st, hi, lo, ws))
    SLOT, STATUS, SI, P = slot.data_ptr(), status.data_ptr(), stats_in.data_ptr(), part.data_ptr()

    def seg(ch0, nch, ld=40, col0=0, tps=8, ncls=1, nb_src=2, ptr=P):
        return L.CsGnSeg(ptr, ld, col0, ch0, nch, tps, ncls, nb_src, 0)

    def fin(segs, nb=2, c=24, groups=3):
        arr = (L.CsGnSeg * max(1, len(segs)))(*segs)
        return lib.cs_groupnorm_finalize_parts(arr, len(segs), nb, 37, c, groups, N.EPS, ST, SLOT, S)

    def parts(segs, nb=2, c=24, groups=3):
        arr = (L.CsGnSeg * max(1, len(segs)))(*segs)
        return lib.cs_groupnorm_parts(X, arr, len(segs), G, B, Y, nb, 37, c, c, c, groups, N.EPS, 0, ST, SLOT, S)

    wino = lambda w, c, var, ldx=None: lib.cs_groupnorm_apply_wino_range(X, SI, G, B, HI, LO, 2, 1, 3, w, c, ldx or c, c, 2, c // 2, 0, 2,
                                                                         16.0, var, STATUS, S)
    calls = {
        "stats c % 4": lambda: lib.cs_groupnorm_stats(X, 2, 37, 6, 8, 2, N.EPS, WS, ST, S),
        "stats_bound c % 4": lambda: lib.cs_groupnorm_stats_bound(X, 2, 37, 6, 8, 2, N.EPS, WS, ST, SLOT, S),
        "stats ldx < c": lambda: lib.cs_groupnorm_stats(X, 2, 37, 16, 8, 2, N.EPS, WS, ST, S),
        "stats groups > 256": lambda: lib.cs_groupnorm_stats(X, 2, 5, 1028, 1028, 257, N.EPS, WS, ST, S),
        "stats misaligned x": lambda: lib.cs_groupnorm_stats(X + 4, 2, 37, 8, 8, 2, N.EPS, WS, ST, S),
        "apply c % 4": lambda: lib.cs_groupnorm_apply(X, SI, G, B, Y, 2, 37, 6, 8, 8, 2, 0, S),
        "apply ldx < c": lambda: lib.cs_groupnorm_apply(X, SI, G, B, Y, 2, 37, 16, 8, 16, 2, 0, S),
        "apply ldy < c": lambda: lib.cs_groupnorm_apply(X, SI, G, B, Y, 2, 37, 16, 16, 8, 2, 0, S),
        "apply misaligned y": lambda: lib.cs_groupnorm_apply(X, SI, G, B, Y + 4, 2, 37, 8, 8, 8, 2, 0, S),
        "apply_range past the groups": lambda: lib.cs_groupnorm_apply_range(X, SI, G, B, Y, 2, 37, 16, 16, 16, 2, 12, 12, 0, S),
        "split16 c % 8": lambda: lib.cs_groupnorm_apply_split16(X, SI, G, B, HI, LO, 2, 37, 12, 12, 16, 2, 0, 16.0, STATUS, S),
        "split16 ldx < c": lambda: lib.cs_groupnorm_apply_split16(X, SI, G, B, HI, LO, 2, 37, 16, 8, 16, 2, 0, 16.0, STATUS, S),
        "split16 a_scale 0": lambda: lib.cs_groupnorm_apply_split16(X, SI, G, B, HI, LO, 2, 37, 16, 16, 16, 2, 0, 0.0, STATUS, S),
        "wino c % 8": lambda: wino(4, 12, 2),
        "wino ldx < c": lambda: wino(4, 16, 2, ldx=8),
        "wino w % 4": lambda: wino(6, 16, 4),
        "wino w % 2": lambda: wino(3, 16, 2),
        "wino w < 2": lambda: wino(1, 16, 2),
        "wino variant 3": lambda: wino(6, 16, 3),
        "layernorm c 2052": lambda: lib.cs_layernorm(X, G, B, Y, 5, 2052, 2052, 2052, N.EPS, S),
        "layernorm c % 4": lambda: lib.cs_layernorm(X, G, B, Y, 5, 6, 8, 8, N.EPS, S),
        "layernorm ldx < c": lambda: lib.cs_layernorm(X, G, B, Y, 5, 16, 8, 16, N.EPS, S),
        "pair16 c % 16": lambda: lib.cs_layernorm_pair16(X, G, B, Y, 5, 24, 24, 32, N.EPS, 16.0, STATUS, S),
        "pair16 ldy % 16": lambda: lib.cs_layernorm_pair16(X, G, B, Y, 5, 16, 16, 24, N.EPS, 16.0, STATUS, S),
        "pair16 c 2064": lambda: lib.cs_layernorm_pair16(X, G, B, Y, 5, 2064, 2064, 2064, N.EPS, 16.0, STATUS, S),
        "pair16 ldx < c": lambda: lib.cs_layernorm_pair16(X, G, B, Y, 5, 32, 16, 32, N.EPS, 16.0, STATUS, S),
        "finalize nseg 0": lambda: fin([]),
        "finalize nseg 5": lambda: fin([seg(0, 4), seg(4, 4), seg(8, 4), seg(12, 4), seg(16, 8)]),
        "finalize hole": lambda: fin([seg(0, 8), seg(12, 12)]),
        "finalize overlap": lambda: fin([seg(0, 16), seg(12, 12)]),
        "finalize short cover": lambda: fin([seg(0, 8), seg(8, 8)]),
        "finalize nb % nb_src": lambda: fin([seg(0, 24)], nb=3),
        "finalize col0 + nch > ld": lambda: fin([seg(0, 24, ld=26, col0=3)]),
        "finalize misaligned part": lambda: fin([seg(0, 24, ptr=P + 8)]),
        "finalize c % groups": lambda: fin([seg(0, 24)], groups=5),
        "parts nseg 0": lambda: parts([]),
        "parts hole": lambda: parts([seg(0, 8), seg(12, 12)]),
        "parts nb % nb_src": lambda: parts([seg(0, 24)], nb=3),
        "parts misaligned part": lambda: parts([seg(0, 24, ptr=P + 8)]),
        "groupnorm ldy < c": lambda: lib.cs_groupnorm(X, G, B, Y, 2, 37, 24, 24, 16, 3, N.EPS, 0, WS, ST, S),
        "groupnorm c % groups": lambda: lib.cs_groupnorm(X, G, B, Y, 2, 37, 24, 24, 24, 5, N.EPS, 0, WS, ST, S),
    }
    got = {k: f() for k, f in calls.items()}
    torch.cuda.synchronize()
    assert got == {k: L.CS_EINVAL for k in calls}, {k: v for k, v in got.items() if v != L.CS_EINVAL}
    assert all(_pristine(buf) for buf in (yb, sb, hb, lb))
    assert float(slot.item()) == 0.0 and int(status.item()) == 0 and _untouched(bb, slot) and _untouched(stb, status)
