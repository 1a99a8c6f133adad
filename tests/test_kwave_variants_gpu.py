"""The K-wave GEMM (csrc/cs_gemm_kw.hip, tile code 10, kw_gemm_f16x3_kernel<PAIR>) on both operand forms at ragged shapes, with
the machinery and the gates of test_gemm_variants_gpu.py over the table of tests/_kwave_cases.py: waves with an empty K range, a
ring that wraps into every tail length, partial K chunks beside NaN-filled lda gaps, one-row and one-float4 edge tiles, grids of
fewer than eight workgroups and ragged ones for the XCD tile map, operands and output as views of wider buffers.

Checks per case (test_kwave_variant_matrix).  cs_conv_gemm_launch_info reports tile 10.  Against fp64 (oracle/ref_ops.py::
conv_ndhwc, behind F.layer_norm for the pair): whole tensor under test_f16x3_gpu.py::gate(K), e16 < 4 e32 + 3e-7 against the
fp32-MFMA path on the same operands, worst row and worst column under the flat ROW_GATE -- the row gate where a row has at least
32 values, the column gate where a column has at least 63: below that the figure is single elements, and cancellation in one
element puts an fp32 evaluation of the same expression at 1.8e-5 (worst column, M = 1), 7.7e-7 (M = 2) and 9.1e-7 (worst row,
cout = 4) with this input recipe, against 1.0e-7 .. 2.0e-7 / 1.7e-7 .. 5.7e-7 on the other cases; the fp32 CPU oracle's own
figures are printed beside the kernel's, never read by a gate.  The output is finite (no NaN from a gap or a band of rows), every
word of its allocation outside the view still holds the sentinel, the status word stays 0.  Identities: a second run gives the
same bits; the one-chain 64x64 tile on the same descriptor agrees within rel-L2 1e-6 (not bit for bit: the K sum is cut in
four); pair cases give the bits of their fp32 twin at the same a_scale.

Further: rows [64, M) launched alone equal those rows of the full launch bit for bit (a row's sum does not depend on m0, the
grid or its slot in the XCD map); the operand scale CsConvGemm.a_bound selects, at both exponent clamps, the 2^40 default and
the overflow flag it must raise for an unbounded operand; every refusal of cs_kw_gemm_f16x3_launch returns before anything is
written, and auto-selection never picks the kernel for a descriptor its launch refuses.
Measured values: profiles/kwave_variants_parity.txt."""
import ctypes as C

import pytest
import torch

import _kwave_cases as K
from conftest import rel_l2
from test_f16x3_gpu import gate
from test_gemm_variants_gpu import (ROW_GATE, SENTINEL, _data, _desc, _device, _k_terms, _launch, _launch_info, _mods,
                                    _out_buffer, _place, _rand, _reference, _report, _rowcol, _rows, _untouched_outside)

pytestmark = pytest.mark.gpu


def _gates(c, tag, out, errs, whole_gate):
    """errs = (whole, worst row, worst column) of out; a direction is gated where _kwave_cases says its figure is a norm"""
    whole, row, col = errs
    assert torch.isfinite(out).all(), tag
    assert whole < whole_gate, (tag, whole, whole_gate)
    if K.row_gated(c):
        assert row < ROW_GATE, (tag, "worst row", row, ROW_GATE)
    if K.col_gated(c):
        assert col < ROW_GATE, (tag, "worst column", col, ROW_GATE)


def _build(c, dev, tile, edit=None, out_case=None):
    """the case's F16X3 descriptor on its fp32 operand slot (a pair case: its own), `edit`ed, over a fresh sentinel-filled
    allocation: (descriptor, allocation, output view, what edit wants kept alive)"""
    L, _, _ = _mods()
    buf, out = _out_buffer(out_case or c)
    p = _desc(c, dev, out, c.fmt, tile, L.MATH_F16X3)
    keep = edit(p) if edit else None
    return p, buf, out, keep


def _run(c, dev, tile=10, edit=None, out_case=None):
    """one cs_conv_gemm of _build's descriptor: (return code, allocation, output view)"""
    L, _, _ = _mods()
    p, buf, out, keep = _build(c, dev, tile, edit, out_case)
    rc = L.load().cs_conv_gemm(C.byref(p), None)
    torch.cuda.synchronize()
    del keep
    return rc, buf, out


# ---- the matrix --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", K.KW_CASES, ids=K.case_id)
def test_kwave_variant_matrix(c):
    L, ops, _ = _mods()
    t = _data(c)
    ref, oracle = t["ref"], t["oracle"]
    dev = _device(c)
    tag = "kwave " + K.case_id(c)
    ops.read_status()
    o16 = _launch(c, dev, expect=(10, None))
    assert ops.read_status() == 0
    o32 = _launch(c, dev, fmt=0, tile=3, math=L.MATH_FP32)          # (the fp32-MFMA path has no tile 10: its 64x64 tile)
    r16 = _report(tag, "f16x3", o16, ref, oracle)
    r32 = _report(tag, "fp32-mfma", o32, ref, oracle)
    _gates(c, tag, o16, r16, gate(_k_terms(c)))
    assert torch.isfinite(o32).all() and r32[0] < gate(_k_terms(c)), r32
    assert r16[0] < 4 * r32[0] + 3e-7, (r16, r32)
    assert torch.equal(_launch(c, dev), o16), "a second run differs"
    o3 = _launch(c, dev, tile=3, expect=(3, 0))
    e3 = rel_l2(o16, o3)
    print(f"gemm_variants {tag} K-wave vs one-chain 64x64 tile: {e3:.3e}")
    assert e3 < 1e-6, e3
    if c.fmt == 2:
        assert torch.equal(_launch(c, dev, fmt=0, expect=(10, None)), o16), "producer split == in-loop split"
    assert ops.read_status() == 0


# ---- a row's sum does not depend on the launch ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A4", "A9"])
def test_rows_do_not_depend_on_the_launch(name):
    """bias / bn epilogues: no per-row operand to shift.  A4: 3 x 2 tiles against 2 x 2; A9: 4 x 3 against 3 x 3"""
    L, ops, _ = _mods()
    c = K.BY_NAME[name]
    assert c.epi in ("bias", "bn") and _rows(c) > 128
    dev = _device(c)
    m = _rows(c)
    ops.read_status()
    full = _launch(c, dev, expect=(10, None))
    rest = c._replace(vol=(1, 1, 1, m - 64))

    def edit(p):
        p.x = p.x + 64 * p.lda * 4
        p.nb, p.win, p.wout = 1, m - 64, m - 64
        assert _launch_info(p)[0] == 10

    rc, buf, out = _run(c, dev, edit=edit, out_case=rest)
    assert rc == 0 and _untouched_outside(buf, out)
    assert out.shape == (m - 64, c.cout) and torch.equal(out, full[64:])
    assert ops.read_status() == 0


# ---- the operand scale from a magnitude bound -----------------------------------------------------------------------------
def _bound_id(v):
    return f"mb={v:g}"


@pytest.mark.parametrize("mb", [2.0, 5000.0, 65000.0, 1e-30, 3.0e7, 0.0, float("inf"), float("nan")], ids=_bound_id)
def test_operand_scale_from_a_bound(mb):
    L, ops, R = _mods()
    c = K.BY_NAME["A7"]
    t = _data(c)
    dev = _device(c)
    xv = dev["a"][0][0]
    s2 = K.bound_scale(mb)
    keep = [torch.tensor([mb], dtype=torch.float32, device="cuda")]
    tag = f"kwave {K.case_id(c)} a_bound {mb:g}"

    def with_x(x):
        return dict(dev, a={0: (_place(x.cuda().view(-1, c.cin), xv.stride(0), 4), None, ops.A_SCALE)})

    def bound(p):
        p.a_bound = keep[0].data_ptr()

    ops.read_status()
    if mb == 0.0:
        # an all-zero tensor under its bound: 2^40, and the output is the epilogue terms alone
        assert s2 == 2.0 ** 40
        rc, buf, out = _run(c, with_x(torch.zeros_like(t["x0"])), edit=bound)
        assert rc == 0 and _untouched_outside(buf, out)
        assert torch.equal(out, t["bias"].cuda()[None, :] + dev["res"])
        assert ops.read_status() == 0
        return
    if not mb < 3.0e38:
        # no bound at all: 2^40 again -- 16 x 2^40 cannot be split into fp16 and must not pass silently
        assert s2 == 2.0 ** 40
        rc, buf, out = _run(c, dev, edit=bound)
        assert rc == 0 and _untouched_outside(buf, out)
        with pytest.raises(L.CsOverflowError):
            ops.check_overflow()
        ops.clear_status()
        assert ops.read_status() == 0
        return
    # finite bounds: x under the bound (3e7: at its own scale -- the exponent clamp at -8 is what is asked)
    x = t["x0"] if mb == 3.0e7 else t["x0"] * (0.99 * mb / float(t["x0"].abs().max()))
    assert float(x.abs().max()) <= mb
    d2 = with_x(x)
    rc, buf, out = _run(c, d2, edit=bound)
    assert rc == 0 and _untouched_outside(buf, out) and ops.read_status() == 0

    def explicit(p):
        a0 = p.a_scale
        assert a0 == ops.A_SCALE
        p.acc_scale = p.acc_scale * (a0 / s2)              # powers of two: exact, as the kernel's acc_scale * (a_scale / s2)
        p.a_scale = s2

    rc, buf_e, out_e = _run(c, d2, edit=explicit)
    assert rc == 0 and _untouched_outside(buf_e, out_e) and ops.read_status() == 0
    assert torch.equal(out, out_e), f"a_bound {mb:g} did not select a_scale {s2:g}"
    if mb in (2.0, 5000.0):
        ref = _reference(c, dict(t, x0=x), torch.float64, R)
        o32 = _reference(c, dict(t, x0=x), torch.float32, R)
        oracle = (rel_l2(o32, ref),) + _rowcol(o32, ref)
        _gates(c, tag, out, _report(tag, "f16x3", out, ref, oracle), gate(_k_terms(c)))
        rc, buf3, out3 = _run(c, d2, tile=3, edit=bound)
        assert rc == 0 and _untouched_outside(buf3, out3) and ops.read_status() == 0
        assert rel_l2(out, out3) < 1e-6


# ---- what the launch refuses ------------------------------------------------------------------------------------------------
REFUSALS = ["base", "a_format 1", "pair cin 136", "pair lda % 16", "3x3x3", "stride 2", "GEGLU", "ldo % 4", "ldr % 4", "ldrv % 4",
            "res off 4 bytes", "rv_rows 0", "scale without shift", "gn_rows 32", "pair out cout 228", "pair out out_scale 0",
            "acc_scale 0"]
# what cs_kw_gemm_applicable sees (operand form, geometry, alignment, leading dimensions, epilogue operands): auto-selection
# must not report the kernel either.  The rest is seen by the launch alone (cs_kw_gemm_f16x3_launch / cs_conv_gemm's own checks)
SEEN = set(REFUSALS[1:13])
# ... and the changed descriptor is still a GEMM another tile runs
VALID = {"3x3x3", "ldr % 4", "ldrv % 4", "res off 4 bytes"}


@pytest.mark.parametrize("what", REFUSALS)
def test_launch_refuses_what_the_kernel_does_not_cover(what):
    """every refusal is a host check that returns before any launch (cs_kw_gemm_geometry_ok, kw_operands_ok, the scale / pair /
    gn_part checks of cs_kw_gemm_f16x3_launch, cs_conv_gemm's argument checks): nothing here runs a kernel on a bad descriptor"""
    L, ops, _ = _mods()
    c = {"pair cin 136": K.R_CIN136, "pair lda % 16": K.R_CIN144, "3x3x3": K.R_K333, "pair out cout 228": K.R_COUT228}.get(
        what, K.R_BASE)
    t = _data(c)
    ref = t["ref"]
    dev = dict(_device(c))
    m = _rows(c)
    assert m == 150 and c.fmt == 0
    x2d = lambda: t["x0"].cuda().view(m, c.cin)
    res2d = lambda: t["res"].cuda().view(m, c.cout)
    rv = _rand(c.vol[0], c.cout, seed=77)
    edit = None
    if what == "a_format 1":
        def edit(p):
            p.a_format, p.x_lo = 1, p.x
    elif what in ("pair cin 136", "pair lda % 16"):
        # the pair operand at cin = 144, lda = 144 is what the kernel takes: auto-selection reports it
        d0 = _device(K.R_CIN144)
        p0 = _build(K.R_CIN144, d0, 0)[0]
        p0.a_format = 2
        assert p0.lda == 144 and _launch_info(p0)[0] == 10
        dev["a"] = {0: (_place(x2d(), 144 if what == "pair cin 136" else 148, 0), None, ops.A_SCALE)}

        def edit(p):
            p.a_format = 2
            assert (p.cin, p.lda) == ((136, 144) if what == "pair cin 136" else (144, 148))
    elif what == "stride 2":
        def edit(p):
            p.sw, p.wout = 2, 38
    elif what == "GEGLU":
        def edit(p):
            p.act = L.ACT_GEGLU
    elif what == "ldo % 4":
        def edit(p):
            p.ldo = c.cout + 2
    elif what == "ldr % 4":
        dev["res"] = _place(res2d(), c.cout + 6, 2)             # (3 x 230 + 2 floats in: the pointer itself stays 16-byte aligned)
        assert dev["res"].data_ptr() % 16 == 0 and dev["res"].stride(0) % 4 == 2
    elif what == "res off 4 bytes":
        dev["res"] = _place(res2d(), c.cout + 4, 1)
        assert dev["res"].data_ptr() % 16 == 4 and dev["res"].stride(0) % 4 == 0
    elif what in ("ldrv % 4", "rv_rows 0"):
        rvd = _place(rv.cuda(), *((c.cout + 6, 2) if what == "ldrv % 4" else (c.cout, 0)))
        assert rvd.data_ptr() % 16 == 0
        if what == "ldrv % 4":
            ref = ref + rv.double()[:, None, None, None, :]

        def edit(p):
            p.rowvec, p.ldrv, p.rv_rows = rvd.data_ptr(), rvd.stride(0), (75 if what == "ldrv % 4" else 0)
            return rvd
    elif what == "scale without shift":
        def edit(p):
            sc = torch.ones(c.cout, device="cuda")
            p.scale, p.shift = sc.data_ptr(), None
            return sc
    elif what == "gn_rows 32":
        def edit(p):
            g = torch.zeros((m // 32 + 2) * 2 * c.cout, dtype=torch.float64, device="cuda")
            p.gn_part, p.gn_ld, p.gn_rows = g.data_ptr(), c.cout, 32
            return g
    elif what == "pair out cout 228":
        def edit(p):
            p.out_format, p.out_scale = 2, 16.0
    elif what == "pair out out_scale 0":
        def edit(p):
            p.out_format, p.out_scale = 2, 0.0
    elif what == "acc_scale 0":
        def edit(p):
            p.acc_scale = 0.0
    else:
        assert what in ("base", "3x3x3")

    def holds_fp64(buf, out, name):
        tag = f"kwave refusal [{what}] {name}"
        assert _untouched_outside(buf, out) and ops.read_status() == 0
        errs = (rel_l2(out, ref),) + _rowcol(out, ref)
        print(f"gemm_variants {tag} f16x3: whole {errs[0]:.3e} row {errs[1]:.3e} col {errs[2]:.3e}")
        assert torch.isfinite(out).all() and errs[0] < gate(_k_terms(c)), (tag, errs)
        return errs

    ops.read_status()
    rc, buf, out = _run(c, dev, tile=10, edit=edit)
    if what == "base":
        assert rc == 0
        errs = holds_fp64(buf, out, "tile 10")
        assert errs[1] < ROW_GATE and errs[2] < ROW_GATE, errs
        assert _launch_info(_build(c, dev, 0)[0])[0] == 10, "auto-selection does not take the K-wave kernel for the base"
        rc, buf0, out0 = _run(c, dev, tile=0)
        assert rc == 0 and torch.equal(out0, out)
        return
    assert rc != 0, (what, rc)
    assert bool((buf.view(torch.int32) == SENTINEL).all()), "a refused launch wrote to the output"
    assert ops.read_status() == 0
    if what in SEEN:
        p, _, _, keep = _build(c, dev, 0, edit)
        assert _launch_info(p)[0] != 10, "auto-selection picks the kernel for a descriptor its launch refuses"
    if what in VALID:
        rc, buf0, out0 = _run(c, dev, tile=0, edit=edit)
        assert rc == 0, (what, rc)
        holds_fp64(buf0, out0, "tile 0")
