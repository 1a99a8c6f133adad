"""What test_wino_variants_gpu.py relies on, checked without a GPU: (1) the fp64 B^T / G / A^T restatement of both Winograd-W
variants in tests/_wino_cases.py composes to F.conv3d in fp64 (1e-12) on three of the table's geometries, and the packed-weight
index order is the one pack_f16x3_wino_kernel decodes; (2) the derived bound E = (a + 4) u T of the output transform and of the
split-K reduce holds for an fp32 CPU evaluation in the kernels' order on every case of the two tables -- the inputs stay inside
the gate by the reference alone -- while a per-tile row vector, a slice too many / too few and a dropped term leave it; (3) the
guard-band, sentinel and pair-decode helpers notice a planted out-of-view write and a planted wrong half; (4) the tables hold
what the module docstrings claim (every second case a view, every epilogue set per variant, nothing above 3072 x 448)."""
import pytest
import torch
import torch.nn.functional as F

import _wino_cases as W


@pytest.mark.parametrize("variant,geom", [(2, "W4"), (2, "W6"), (4, "W4"), (4, "W12"), (4, "D1-W64"), (2, "H1")])
def test_transform_identity_equals_conv3d_in_fp64(variant, geom):
    nb, d, h, w = W.GEOM[variant][geom]
    nb, d = min(nb, 2), min(d, 5)                   # (the identity is per line; fewer planes keep this quick)
    cin, cout = 5, 7
    y = W.rand(nb, d, h, w, cin, seed=1).double()
    wt = W.rand(cout, cin, 3, 3, 3, seed=2).double()
    got = W.transform64(W.positions64(W.images64(y, variant), W.weights64(wt, variant)), variant)
    ref = F.conv3d(y.permute(0, 4, 1, 2, 3), wt, padding=1).permute(0, 2, 3, 4, 1).reshape(-1, cout)
    assert got.shape == ref.shape
    assert float((got - ref).abs().max()) <= 1e-12


def test_pack_order_is_the_kernels_index_decode():
    """element i of the packed image, decoded as pack_f16x3_wino_kernel does: j = i & 7, n, kg, tap, q"""
    u = W.rand(4, 3, 24, 3, 3, seed=3).double()
    pk = W.pack_order(u).flatten()
    cout, kgpt = 3, 4
    per = 9 * kgpt * cout * 8
    for i in (0, 7, 8, 95, 96, per - 1, per, 3 * per + 517, 4 * per - 1):
        q, t = divmod(i, per)
        j, t = t & 7, t >> 3
        n, t = t % cout, t // cout
        kg, tap = t % kgpt, t // kgpt
        c = kg * 8 + j
        want = float(u[q, n, c, tap // 3, tap % 3]) if c < 24 else 0.0
        assert float(pk[i]) == want, i


@pytest.mark.parametrize("variant", [2, 4])
@pytest.mark.parametrize("form", list(W.PACK_FORMS))
def test_pack_inputs_stay_inside_the_gate_under_the_exact_split(form, variant):
    """(hi + lo) / scale of the fp64 value's own fp16 split against the gate of the GPU test: the inputs leave the kernel room"""
    wt, scale, u = W.pack_case(form, variant)
    _, _, val = W.split16(u, scale)
    r = float(((val - u).abs() / W.pack_bound(u, scale)).max())
    print(f"wino_variants_cpu pack F{variant} {form}: exact split at {r:.3f} of the gate")
    assert r <= 0.5 and float(u.abs().max()) * scale < 65504.0


def _worst(val, ref, e):
    return float(((val.double() - ref).abs() / e).max())


@pytest.mark.parametrize("c", W.OUTS, ids=W.out_id)
def test_bound_holds_for_the_fp32_restatement_of_the_output_transform(c):
    ws, nsl, e = W.out_case(c)
    ref, bound = W.reference64(ws, nsl, c.variant, e)
    assert torch.isfinite(ref).all() and torch.isfinite(bound).all() and float(bound.min()) > 0.0
    r = _worst(W.kernel32(ws, nsl, c.variant, e), ref, bound)
    print(f"wino_variants_cpu out {W.out_id(c)}: fp32 restatement at {r:.3f} E")
    assert r <= 1.0
    # the slices the kernel must not read may hold anything: NaN there changes neither the reference nor the restatement
    if c.slices > 1:
        n1 = nsl.clone()
        n1[1:] = 1
        poisoned = ws.clone()
        poisoned[1:, 1:] = float("nan")
        ref1, b1 = W.reference64(poisoned, n1, c.variant, e)
        assert torch.isfinite(ref1).all() and _worst(W.kernel32(poisoned, n1, c.variant, e), ref1, b1) <= 1.0
        assert _worst(W.kernel32(ws, n1, c.variant, e), ref, bound) > 1.0                 # a slice too few


@pytest.mark.parametrize("c", W.REDS, ids=W.red_id)
def test_bound_holds_for_the_fp32_restatement_of_the_reduce(c):
    ws, nsl, e = W.red_case(c)
    ref, bound = W.reference64(ws, nsl, None, e)
    assert torch.isfinite(ref).all() and float(bound.min()) > 0.0
    r = _worst(W.kernel32(ws, nsl, None, e), ref, bound)
    print(f"wino_variants_cpu reduce {W.red_id(c)}: fp32 restatement at {r:.3f} E")
    assert r <= 1.0
    assert _worst(W.kernel32(ws, nsl - 1, None, e), ref, bound) > 1.0                      # the last slice left out


def test_mutants_of_the_restatement_leave_the_bound():
    """what a subtly wrong wino_out_kernel would compute: the row vector taken per TILE (m / rv_rows of the tile's first row),
    the epilogue's residual of the neighbouring row, a dropped bias"""
    seen = 0
    for c in W.OUTS:
        ws, nsl, e = W.out_case(c)
        ref, bound = W.reference64(ws, nsl, c.variant, e)
        if c.rv not in (None, "sample") and c.rv % c.variant:
            m = ref.shape[0]
            first = (torch.arange(m) // c.variant * c.variant) // c.rv
            per_tile = e._replace(rv=e.rv[first], rv_rows=1)
            assert _worst(W.kernel32(ws, nsl, c.variant, per_tile), ref, bound) > 1.0, W.out_id(c)
            seen += 1
        if e.res is not None:
            assert _worst(W.kernel32(ws, nsl, c.variant, e._replace(res=torch.roll(e.res, 1, 0))), ref, bound) > 1.0
        if e.bias is not None:
            assert _worst(W.kernel32(ws, nsl, c.variant, e._replace(bias=None)), ref, bound) > 1.0
    assert seen >= 3 and {c.variant for c in W.OUTS if c.rv not in (None, 'sample') and c.rv % c.variant} == {2, 4}


def test_tail_plan_slice_map():
    """one slice for the (position, 224-column tile) units before units_main, `slices` from there on: q tiles_n + n / 224"""
    nsl = W.tail_nsl(2, 672, 3, 11)
    assert nsl.shape == (4, 672) and int((nsl == 1).sum()) == 11 * 224 and int((nsl == 3).sum()) == 224
    assert int(nsl[3, 447]) == 1 and int(nsl[3, 448]) == 3
    nsl = W.tail_nsl(4, 672, 3, 17)
    assert int((nsl == 3).sum()) == 224 and int(nsl[5, 448]) == 3 and int(nsl[5, 447]) == 1


def test_guard_band_and_sentinel_helpers_notice_a_planted_write():
    t = W.rand(6, 8, seed=4)
    buf, view = W.place(t, 12, 4)
    assert torch.equal(view, t) and W.nan_outside(buf, view)
    for r, col in ((W.PRE_ROWS - 1, 5), (W.PRE_ROWS + 6, 4), (W.PRE_ROWS + 2, 3), (W.PRE_ROWS + 5, 0), (0, 0)):
        b2 = buf.clone()
        b2[r, col] = 1.0
        assert not W.nan_outside(b2, b2[W.PRE_ROWS:W.PRE_ROWS + 6, 4:12]), (r, col)
    for dtype in (torch.float32, torch.float64):
        sb, sv = W.sentinel_buffer(6, 8, 12, 4, dtype=dtype)
        assert W.untouched_outside(sb, sv)
        sv.copy_(t)
        assert W.untouched_outside(sb, sv)
        for r, col in ((W.PRE_ROWS - 1, 11), (W.PRE_ROWS + 6, 4), (W.PRE_ROWS + 3, 3), (W.PRE_ROWS + 3, 0), (sb.shape[0] - 1, 11)):
            b2 = sb.clone()
            b2[r, col] = 0.0
            assert not W.untouched_outside(b2, b2[W.PRE_ROWS:W.PRE_ROWS + 6, 4:12]), (dtype, r, col)
    # the sentinel as a float is finite and nothing a kernel here produces
    f = torch.tensor([W.SENTINEL], dtype=torch.int32).view(torch.float32)
    assert torch.isfinite(f).all() and float(f.abs()) > 1e15


def test_pair_decode_notices_a_wrong_half():
    o = W.rand(5, 24, seed=5) * 3.0
    s = 16.0
    hi, lo = W.pair_expected(o, s)
    words = torch.full((5, 32), float("nan"))
    h = words.view(torch.float16).reshape(5, 4, 2, 8)            # 16 halves per 8 columns: hi then lo
    h[:, :3, 0] = hi.reshape(5, 3, 8)
    h[:, :3, 1] = lo.reshape(5, 3, 8)
    dh, dl = W.pair_decode(words, 24)
    assert torch.equal(dh, hi) and torch.equal(dl, lo)
    assert float(((dh.double() + dl.double()) / s - o.double()).abs().max()) <= 2.0 ** -21 * float(o.abs().max())
    swapped = words.clone()
    sh = swapped.view(torch.float16).reshape(5, 4, 2, 8)
    sh[2, 1, 0], sh[2, 1, 1] = h[2, 1, 1].clone(), h[2, 1, 0].clone()           # one group's halves exchanged
    dh, dl = W.pair_decode(swapped, 24)
    assert not torch.equal(dh, hi) and not torch.equal(dl, lo)
    off = words.clone()
    off.view(torch.float16).reshape(5, 4, 2, 8)[4, 2, 1, 7] += 2.0 ** -10       # one lo half an ulp-ish off
    assert not torch.equal(W.pair_decode(off, 24)[1], lo)


def test_tables_hold_what_they_claim():
    for v in (2, 4):
        assert set(W.GEOM[v]) >= {"D1-W64", "W4", "H1", "odd-nb", "W12"}
        for vol in W.GEOM[v].values():
            assert W.rows_of(vol) % (256 * v) == 0 and W.rows_of(vol) <= 3072 and vol[3] % 2 == 0 and 2 <= vol[3] // 2 <= 32
    assert "W6" in W.GEOM[2] and "W6" not in W.GEOM[4]
    tile = lambda cout: 4 if cout % 224 == 0 else 6 if cout % 128 == 0 else 7
    for v in (2, 4):
        cs = [c for c in W.CONVS if c.variant == v]
        assert {c.geom for c in cs} == set(W.GEOM[v])
        assert {c.cin for c in cs} == {16, 24, 40, 72}
        for t in (4, 6, 7):
            assert sum(tile(c.cout) == t for c in cs) >= 2, (v, t)
        for c in cs:                                  # F(4,3) off the 224-column widths: whole 1024-row samples only
            vol = W.GEOM[v][c.geom]
            assert v == 2 or c.cout % 224 == 0 or (W.rows_of(vol) // vol[0]) % 1024 == 0, W.conv_id(c)
        os_ = [c for c in W.OUTS if c.variant == v]
        assert {c.epi for c in os_} == {"bias", "brr", "bn", "rg"} and {c.cout for c in os_} == {64, 224, 448}
        assert {c.slices for c in os_} == {1, 3, 16} and {c.rv for c in os_} >= {"sample", 6}
        assert any(c.gn and c.cout == 224 for c in os_)
    assert {c.cout for c in W.CONVS} == {64, 128, 224, 256, 448}
    for table in (W.CONVS, W.OUTS, W.REDS):
        views = sum(c.view for c in table)
        assert abs(views - len(table) / 2) <= 1
    assert {W.rows_of(c.vol) for c in W.REDS} == {750, 210, 160}
    assert {c.cin for c in W.REDS} == {24, 40} and {c.cout for c in W.REDS} == {224, 68, 132, 72}
    assert {2, 5, "max"} == {c.slices for c in W.REDS}
    assert all((W.rows_of(c.vol) // c.vol[0]) % 16 == 0 for c in W.REDS if c.gn)
    assert max(W.rows_of(W.GEOM[c.variant][c.geom]) * c.cout for c in W.CONVS) <= 3072 * 448
