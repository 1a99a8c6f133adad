"""The host side of tests/test_gemm_variants_gpu.py, without a device: for every row of its CASES and every (case, slices) of
its SLICED, cs_conv_gemm_launch_info -- a reader of the one variant rule of cs_gemm_f16x3.hip (cs_f16x3_variant) -- reports the
(tile, slab) the row is meant for, and under the CsDebug switches the values its bit-identity twins expect.  The descriptors
are built from the rows' geometry alone: the pointers are aligned dummy integers, nothing is launched or dereferenced."""
import ctypes as C

import pytest

from test_gemm_variants_gpu import CASES, SLICED, SLICES, _id, _out_vol, _twins

BASE = 1 << 28          # a 16-byte aligned address nobody reads


def _desc(c, fmt=None, tile=None, splitk=0):
    from commonscenes_amd import lib as L
    p = L.CsConvGemm()
    p.x = p.w = p.w_lo = p.out = p.bias = BASE
    p.nb, p.din, p.hin, p.win = c.vol
    p.dout, p.hout, p.wout = _out_vol(c)
    p.cin, p.cout = c.cin, c.cout
    p.lda, p.ldo, p.ldw = c.cin, c.cout, c.cout
    p.kd, p.kh, p.kw = c.k
    p.sd, p.sh, p.sw = c.stride
    p.pd, p.ph, p.pw = c.pad
    p.math, p.rv_rows, p.acc_scale = L.MATH_F16X3, 1, 1.0
    p.a_format = c.fmt if fmt is None else fmt
    p.tile = c.tile if tile is None else tile
    if p.a_format == 1:
        p.x_lo = BASE
    if splitk > 1:
        p.splitk, p.splitk_ws = splitk, BASE
    return p


def _info(p):
    from commonscenes_amd import lib as L
    tl, sl = C.c_int32(-1), C.c_int32(-1)
    assert L.load().cs_conv_gemm_launch_info(C.byref(p), C.byref(tl), C.byref(sl)) == 0
    return tl.value, sl.value


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_launch_info_names_the_rows_variant_and_its_twins(c):
    from commonscenes_amd import lib as L
    assert _info(_desc(c)) == (c.tile, c.slab)
    for claim, over, expect in _twins(c):
        over = dict(over)
        p = _desc(c, fmt=over.pop("fmt", None), tile=over.pop("tile", None))
        with L.debug_override(**over):
            info = _info(p)
        assert info[0] == expect[0] and (expect[1] is None or info[1] == expect[1]), (claim, info, expect)


@pytest.mark.parametrize("c,slices", list(zip(SLICED, SLICES)), ids=lambda v: _id(v) if hasattr(v, "route") else f"k{v}")
def test_launch_info_of_the_sliced_rows(c, slices):
    """rows 4 and 5 (slab 0): slice counts that pad the super-chunks by more than a tenth go back to the per-tap gather"""
    nsc = 3 * ((c.cin + 15) // 16)
    assert (-(-nsc // slices) * slices * 10 <= nsc * 11) == (c.slab != 0)
    assert _info(_desc(c, splitk=slices)) == (c.tile or 4, c.slab)
