"""The parts of test_up2_variants_gpu.py that need no device (tests/_up2_cases.py): (1) the fold restated in torch -- tap sets
per doubled dim and parity, extent 2 and low pad 1 - parity, class index (pd * nh + ph) * nw + pw, interleaved outputs -- equals
oracle/ref_ops.py::conv_ndhwc(up=...) in fp64 for all seven doubling patterns on a 2 x 3 x 5 x 7 grid, inside a per-element bound
on the reassociation of the same products (measured: 2.5e-14 at most, the bound's smallest element 1.4e-13); (2) the comparison helper flags every mutant of the
restatement -- parity pads swapped, a tap dropped from a two-tap sum, H and W parity swapped in the row map, the classes in
pw-major order -- wherever the pattern does not turn the mutant into the restatement itself; (3) cs_conv_up2_info on all eight
flag combinations and flags outside 0 / 1; (4) the host rules cs_conv_gemm_up2_ws_bytes (-1 for every descriptor up2_ok refuses,
at least the class results for every row of the table) and cs_conv_gemm_epilogue_caps on Upsample descriptors (never the pair;
256-row partials exactly on the one-launch route with a bias, no scale / shift and whole tiles per sample); (5) the table's
self-checks.

Without a device device_cus() is 0, so up2_sliced_plan grants no slices here: the slice counts and the sliced launch's
workspace are CU-dependent and are asserted by the GPU file alone (its footprint check).  up2_direct_batched, plan_splitk and the
tile rule do not look at the CU count; what this file asserts about them holds on the device as it does here."""
import ctypes as C

import pytest
import torch

import _up2_cases as U

GRID = (2, 3, 5, 7)
CIN, COUT = 3, 4


def _inputs():
    g = torch.Generator().manual_seed(20)
    x = torch.randn(*GRID, CIN, generator=g, dtype=torch.float64)
    w = torch.randn(COUT, CIN, 3, 3, 3, generator=g, dtype=torch.float64)
    return x, w


@pytest.mark.parametrize("up", U.PATTERNS, ids=lambda u: "".join(map(str, u)))
def test_class_convs_interleave_to_the_upsampled_conv_and_every_mutant_does_not(up):
    from oracle import ref_ops as R
    x, w = _inputs()
    ref = R.conv_ndhwc(x, w, None, (1, 1, 1), up)
    gate = U.fold_gate(x, w, up)
    out = U.folded_conv(x, w, up)
    assert out.shape == ref.shape
    line = f"up2_variants_cpu {up}: restatement max abs {float((out - ref).abs().max()):.2e} (gate min {float(gate.min()):.2e})"
    assert not U.differs(out, ref, gate)
    for m in U.MUTANTS:
        if not U.mutant_applies(m, up):
            line += f"  {m} n/a"
            continue
        bad = U.folded_conv(x, w, up, m)
        line += f"  {m} {float((bad - ref).abs().max()):.2e}"
        assert U.differs(bad, ref, gate), (up, m)
    print(line)
    assert U.differs(out + torch.where(torch.arange(out.numel()).reshape(out.shape) == 17, float("nan"), 0.0), ref, gate)


def test_every_mutant_is_applied_and_the_restated_class_order_is_pd_major():
    applied = {m: sum(U.mutant_applies(m, up) for up in U.PATTERNS) for m in U.MUTANTS}
    assert applied == {"pads_swapped": 7, "tap_dropped": 7, "hw_swapped": 2, "class_order": 4}
    assert U.classes((1, 1, 1))[:3] == [(0, 0, 0), (0, 0, 1), (0, 1, 0)] and U.classes((0, 1, 1))[1] == (0, 0, 1)
    assert U.classes((1, 1, 0))[1] == (0, 1, 0)
    for up in U.PATTERNS:
        assert [(pd * (2 if up[1] else 1) + ph) * (2 if up[2] else 1) + pw for pd, ph, pw in U.classes(up)] == \
            list(range(1 << sum(up)))
    assert U.src_taps(1, 0, 0) == [0] and U.src_taps(1, 0, 1) == [1, 2] and U.src_taps(1, 1, 0) == [0, 1]
    assert U.src_taps(1, 1, 1) == [2] and [U.src_taps(0, 0, k) for k in range(3)] == [[0], [1], [2]]


def test_up2_info_on_every_flag_combination():
    from commonscenes_amd import lib as L
    for ud in (0, 1):
        for uh in (0, 1):
            for uw in (0, 1):
                got = U.up2_info(L, (ud, uh, uw))
                if not (ud | uh | uw):
                    assert got[0] == L.CS_EINVAL
                else:
                    assert got == (0, 1 << (ud + uh + uw), 2 if ud else 3, 2 if uh else 3, 2 if uw else 3)
    for bad in ((2, 0, 0), (0, -1, 1), (1, 1, 2), (0, 3, 0), (-1, -1, -1)):
        assert U.up2_info(L, bad)[0] == L.CS_EINVAL, bad
    assert L.load().cs_conv_up2_info(1, 1, 1, None, None, None, None) == 0          # every output is optional


def _base():
    return next(r for r in U.ROWS if r.route == "batch" and r.gn)


def test_ws_bytes_refuses_what_up2_ok_refuses():
    from commonscenes_amd import lib as L
    lib = L.load()
    r = _base()
    fake = 4096          # a non-null pointer no host rule dereferences
    ok = U.descriptor(L, r)
    assert lib.cs_conv_gemm_up2_ws_bytes(C.byref(ok)) >= U.ncls(r) * U.m1(r) * r.cout * 4
    assert lib.cs_conv_gemm_up2_ws_bytes(None) == -1
    edits = {
        "residual": dict(res=fake), "row vector": dict(rowvec=fake), "scale / shift": dict(scale=fake, shift=fake),
        "GEGLU": dict(act=L.ACT_GEGLU), "cout % 4": dict(cout=r.cout + 2, ldo=r.cout + 4), "ldo % 4": dict(ldo=r.cout + 2),
        "splitk": dict(splitk=2), "flag 2 (D)": dict(ud=2, dout=r.vol[1] << 2), "flag 2 (W)": dict(uw=2, wout=r.vol[3] << 2),
        "flag -1": dict(uh=-1), "no flag": dict(ud=0, uh=0, uw=0, dout=r.vol[1], hout=r.vol[2], wout=r.vol[3]),
        "dout != din << ud": dict(dout=r.vol[1]), "hout": dict(hout=(r.vol[2] << 1) + 1), "wout": dict(wout=r.vol[3]),
        "1x1x1": dict(kd=1, kh=1, kw=1), "3x3x1": dict(kw=1), "stride 2": dict(sh=2), "pad 0": dict(pd=0), "pad 0 (W)": dict(pw=0),
    }
    for what, e in edits.items():
        p = U.descriptor(L, r)
        for k, v in e.items():
            assert hasattr(p, k)
            setattr(p, k, v)
        assert lib.cs_conv_gemm_up2_ws_bytes(C.byref(p)) == -1, what
    # ... and the terms it admits stay admitted: bias, SiLU, a wider output row, GroupNorm partials
    p = U.descriptor(L, r, ldo=r.cout + 12)
    p.bias, p.act = fake, L.ACT_SILU
    assert lib.cs_conv_gemm_up2_ws_bytes(C.byref(p)) > 0


@pytest.mark.parametrize("r", U.ROWS, ids=U.row_id)
def test_ws_bytes_holds_the_class_results_of_every_row(r):
    from commonscenes_amd import lib as L
    got = L.load().cs_conv_gemm_up2_ws_bytes(C.byref(U.descriptor(L, r)))
    assert got >= U.ncls(r) * U.m1(r) * r.cout * 4, (got, U.row_id(r))
    if r.route == "scratch":          # (plan_splitk does not look at the CU count: the per-class slices are already in)
        assert got >= U.prefix_words(r) * 4


def _caps(L, p):
    rows, pair = C.c_int32(-1), C.c_int32(-1)
    assert L.load().cs_conv_gemm_epilogue_caps(C.byref(p), C.byref(rows), C.byref(pair)) == 0
    return rows.value, pair.value


def test_epilogue_caps_of_upsample_descriptors():
    from commonscenes_amd import lib as L
    r = _base()
    fake = 4096

    def desc(row=r, bias=True, **e):
        p = U.descriptor(L, row, ldo=e.pop("ldo", None))
        p.out = 1 << 20          # 64-byte aligned: with ldo % 16 == 0 and cout % 8 == 0 the pair's geometry would do
        p.bias = fake if bias else None
        for k, v in e.items():
            setattr(p, k, v)
        return p

    assert r.cout % 8 == 0 and r.cout % 16 == 0
    assert _caps(L, desc()) == (256, 0)                                    # granted; never the pair
    assert _caps(L, desc(ldo=r.cout + 16)) == (256, 0)
    assert _caps(L, desc(act=L.ACT_SILU)) == (256, 0)
    assert _caps(L, desc(bias=False)) == (0, 0)                            # the piped epilogue needs a bias
    assert _caps(L, desc(scale=fake, shift=fake)) == (0, 0)                # (up2_ok refuses it anyway)
    assert _caps(L, desc(math=L.MATH_FP32)) == (0, 0)
    assert _caps(L, desc(a_format=1)) == (0, 0)                            # pre-split: off the slab kernel, off the route
    assert _caps(L, desc(splitk=2)) == (0, 0)
    # the `fills` rule: classes x 256-row tiles x column tiles >= 128 -- 8 x 16 x 1 here, one sample fewer is 8 x 15
    assert U.ncls(r) * (U.m1(r) // 256) * (r.cout // 128) == 128
    assert _caps(L, desc(nb=r.vol[0] - 1)) == (0, 0)
    assert _caps(L, desc(nb=r.vol[0] + 1)) == (256, 0)
    # rps % 256: 4 x 8 x 8 source rows per sample -> 4 x 8 x 7 (still >= 128 tiles at 19 samples)
    assert _caps(L, desc(win=7, wout=14, nb=19)) == (0, 0) and 8 * ((19 * 224 + 255) // 256) >= 128
    with L.debug_override(no_up2_batch=1):
        assert _caps(L, desc()) == (0, 0)
    with L.debug_override(no_up2_direct=1):
        assert _caps(L, desc()) == (0, 0)
    with L.debug_override(no_slab4=1):
        assert _caps(L, desc()) == (0, 0)
    # every row of the table: partials exactly on the row that asks for them, the pair nowhere
    for row in U.ROWS:
        sw = {k: 1 for k in row.sw}
        with L.debug_override(**sw):
            got = _caps(L, desc(row=row, bias=row.bias))
        assert got == ((256, 0) if row.gn else (0, 0)), (U.row_id(row), got)


def test_table_has_every_route_pattern_and_edge():
    rows = U.ROWS
    assert {r.route for r in rows} == {"scratch", "sliced", "batch", "perclass"}
    assert {r.up for r in rows} == set(U.PATTERNS)
    for route in ("sliced", "batch"):
        assert {r.up for r in rows if r.route == route} == set(U.SLAB_PATTERNS), route
    assert {r.up for r in rows if r.piece == "a"} == set(U.SLAB_PATTERNS)
    assert {(r.up, r.math) for r in rows if r.piece == "b"} == \
        {(u, m) for u in U.PATTERNS if u not in U.SLAB_PATTERNS for m in ("f16x3", "fp32")}
    assert {(r.math, r.cout) for r in rows if r.piece == "a"} == {(m, c) for m in ("f16x3", "fp32") for c in (236, 132)}
    assert {(r.bias, r.act) for r in rows if r.piece == "a"} == {(b, a) for b in (True, False) for a in ("none", "silu")}
    assert any("no_slab4" in r.sw for r in rows if r.piece == "a")
    assert sorted(r.slices for r in rows if r.route == "sliced") == [2, 9, 10, 17]
    assert any(r.route == "scratch" and r.slices > 1 for r in rows)
    assert [r.view for r in rows] == [i % 2 == 1 for i in range(len(rows))]
    for route in ("scratch", "sliced", "batch"):
        assert {r.view for r in rows if r.route == route} == {True, False}, route
    for r in rows:
        assert r.vol[0] >= 2 and r.cout % 4 == 0 and r.cin % (8 if r.fmt else 4) == 0, U.row_id(r)
        if r.gn:          # whole statistics tiles per sample: the one row that cannot have a ragged last row tile
            assert (r.vol[1] * r.vol[2] * r.vol[3]) % 256 == 0 and r.bias
            continue
        assert all(v % 2 for v in r.vol[1:]), U.row_id(r)
        for bm in (64, 128, 256):
            assert U.m1(r) % bm not in (0, bm - 1), U.row_id(r)
        assert r.cin % 16 or r.cin in (96, 272), U.row_id(r)          # (whole K chunks: two of the sliced shapes only)
    assert {r.slices for r in rows if r.route == "sliced" and r.cin % 16} == {2, 10}
    # K bounds where the worst-row / worst-column gates apply; the rows beyond are whole-tensor only
    assert [U.row_id(r) for r in rows if U.k_exec(r) >= 2000] == [U.row_id(r) for r in rows if r.slices == 17]
    assert all(r.cin * 27 < 10000 for r in rows)
    # the routes' size rules, as far as they do not depend on the CU count
    for r in rows:
        tiles = U.ncls(r) * ((U.m1(r) + 255) // 256) * (r.cout // (224 if r.cout % 224 == 0 else 128))
        if r.route == "batch":
            assert tiles >= 128 and r.cout % (224 if r.cout % 224 == 0 else 128) == 0
        if r.route == "perclass":
            assert (U.m1(r) + 255) // 256 >= 192 and "no_up2_batch" in r.sw and len(set(r.vol[1:])) == 3
        if r.route == "sliced":
            assert 2 * tiles <= 256 and r.fmt == 0 and not r.sw
    assert sum(r.fmt == 1 for r in rows) == 2 and all(r.route == "scratch" for r in rows if r.fmt)
