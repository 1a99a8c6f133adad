"""Every instantiation attn16_dispatch can pick (cs_attention_f16x3.hip), and the fp32 kernel next to it (cs_attention.hip),
at ragged shapes against softmax(q k^T / sqrt(d)) v in fp64: ragged last query / key tiles on the four- and eight-wave
kernels, dh below the padded width 32*DB, nk < KT on the prefetch pipeline, (sample, head) counts that are no multiple of
the grid's groups of eight, nq != nk on the tile-image path -- and the claims the source makes in comments: masked keys
contribute nothing, nothing outside the ld* views is read or written, the overflow report looks at operands inside the view
only, four waves == eight waves and image path == in-kernel split bit for bit.

Gates.  Whole tensor: F16X3 at the per-op gate 1e-6 (test_f16x3_gpu.py), the fp32 kernel at test_ops_gpu.py's TOL.  Worst
(sample, head, query) row of dh values: max(4 x the fp32 CPU oracle's worst row on the same inputs, 1e-6) -- F16X3 operands
carry 22 mantissa bits against fp32's 24, and at nk = 1 the oracle is exact while the hi + lo split is not, hence the floor.
Measured values: profiles/attn_variants_parity.txt; the kernels each case launches: profiles/attn_variants_kernel_trace.txt."""
from collections import namedtuple

import pytest
import torch

from conftest import rel_l2
from test_ops_gpu import TOL

pytestmark = pytest.mark.gpu

GATE16 = 1e-6          # the per-op F16X3 gate of test_f16x3_attention_is_fp32_grade
ROW_FLOOR = 1e-6
SENTINEL = 0x5A5AA5A5  # bit pattern of untouched output words (a finite float no kernel here produces)

Case = namedtuple("Case", "nb nq nk heads dh route")      # route: "" | "nw8" (the debug switch) | "natural" (the fill rule)

CASES = [
    Case(1, 1, 1, 1, 4, ""),            # <1,64,4>  one query, one key: output = v
    Case(3, 67, 65, 3, 20, ""),         # <1,64,4>  9 (sample, head)s: 7 surplus workgroups; key tile of 1
    Case(1, 40, 5, 1, 48, ""),          # <2,64,4>  nk < KT on the prefetch pipeline; dh < DP
    Case(1, 129, 65, 3, 36, ""),        # <2,64,4>  second tile holds one key: the prefetch of a 1-key tile
    Case(2, 64, 64, 2, 64, ""),         # <2,64,4>  exact tiles, dh = DP (control)
    Case(1, 520, 70, 3, 40, "nw8"),     # <2,64,8>  3 query tiles of 256, last with 8 rows; ragged keys
    Case(16, 512, 64, 8, 36, "natural"),  # <2,64,8>  fill rule 16*8*2 = 256 >= 128
    Case(2, 100, 200, 2, 68, ""),       # <3,64,4>  28 padded channels, ragged both ways
    Case(1, 300, 90, 3, 84, "nw8"),     # <3,64,8>  ragged second query tile, 3 heads
    Case(16, 256, 64, 8, 84, "natural"),  # <3,64,8>  fill rule 16*8*1 = 128
    Case(1, 130, 130, 2, 100, ""),      # <4,64,4>  DB 4; dh < DP
    Case(2, 64, 192, 1, 128, ""),       # <4,64,4>  dh = DP, nq < nk
    Case(1, 70, 33, 1, 132, ""),        # <8,32,4>  32-key tile + 1, dh < DP
    Case(1, 200, 100, 2, 256, ""),      # <8,32,4>  dh = DP, 4 ragged keys
    Case(1, 1025, 129, 1, 140, ""),     # image path: nq != nk, both ragged, zero-padded image
]
IMG_CASE = CASES[-1]
NW8_CASES = [CASES[5], CASES[8]]
# On unit-variance q the fp32 CPU oracle's own worst row passes 1e-6 in these four (1.4e-6 .. 1.8e-6: long rows, many of
# them), which would move the worst-row gate with the oracle; they keep their shapes and take q / 2 (oracle 3.5e-7 .. 6.7e-7).
HALF_Q = {CASES[8], CASES[9], CASES[13], CASES[14]}


def _id(c):
    return "x".join(str(x) for x in c[:5]) + ("-" + c.route if c.route else "")


def _mods():
    from commonscenes_amd import lib as L, ops
    from oracle import ref_ops as R
    return L, ops, R


def _rand(*shape, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.randn(*shape, generator=g)


def _inputs(case, seed=900):
    c = case.heads * case.dh
    return (_rand(case.nb, case.nq, c, seed=seed) * (0.5 if case in HALF_Q else 1.0), _rand(case.nb, case.nk, c, seed=seed + 1),
            _rand(case.nb, case.nk, c, seed=seed + 2))


def _rows(out, ref, heads):
    """rel-L2 of every (sample, query, head) row of dh values, in fp64: [nb, nq, heads]"""
    o = out.detach().double().cpu()
    nb, nq, c = ref.shape
    d = (o - ref).reshape(nb, nq, heads, c // heads).norm(dim=-1)
    return d / ref.reshape(nb, nq, heads, c // heads).norm(dim=-1).clamp_min(1e-30)


def _oracle(q, k, v, heads):
    """(fp64 result, whole-tensor rel-L2 and worst-row rel-L2 of the fp32 CPU oracle against it) for fp32 inputs"""
    _, _, R = _mods()
    scale = (q.shape[-1] // heads) ** -0.5
    ref = R.attention(q.double(), k.double(), v.double(), heads, scale)
    o32 = R.attention(q, k, v, heads, scale)
    whole = float((o32.double() - ref).norm() / ref.norm())
    return ref, whole, float(_rows(o32, ref, heads).max())


_DATA = {}


def _data(case):
    """inputs, fp64 result and the fp32 oracle's own errors of a table case: computed once, shared, never modified"""
    if case not in _DATA:
        q, k, v = _inputs(case)
        _DATA[case] = (q, k, v) + _oracle(q, k, v, case.heads)
    return _DATA[case]


def _place(t, ld=None, off=0, extra_rows=0, fill=0.0):
    """CPU [nb, n, c] -> (device buffer [nb*n + extra_rows, ld] filled with `fill`, its [nb, n, c] view at column `off`)"""
    nb, n, c = t.shape
    ld = ld or c
    buf = torch.full((nb * n + extra_rows, ld), fill, dtype=torch.float32, device="cuda")
    view = buf[:nb * n].view(nb, n, ld)[..., off:off + c]
    view.copy_(t)
    return buf, view


def _fused(q, k, v):
    """q | k | v as column slices of [nb, n, 3c] buffers, as the hosts pass them (one buffer when nq == nk)"""
    c = q.shape[-1]
    if q.shape[1] == k.shape[1]:
        buf = torch.cat([q, k, v], dim=-1).cuda()
        return buf[..., 0:c], buf[..., c:2 * c], buf[..., 2 * c:]
    return (_place(q, 3 * c, 0)[1], _place(k, 3 * c, c)[1], _place(v, 3 * c, 2 * c)[1])


def _operands(case, q, k, v):
    """half the table on fused buffers (row stride 3c), the rest contiguous; every third case writes a wider output"""
    i = CASES.index(case)
    qd, kd, vd = _fused(q, k, v) if i % 2 == 0 else (q.cuda(), k.cuda(), v.cuda())
    out = None
    if i % 3 == 0:
        c = q.shape[-1]
        out = torch.zeros((case.nb, case.nq, c + 12), device="cuda")[..., 4:4 + c]
    return qd, kd, vd, out


def _run(case, q, k, v, math, out=None, scales=None, route=None, **switches):
    L, ops, _ = _mods()
    if (case.route if route is None else route) == "nw8":
        switches["attn_nw8"] = 1
    with L.debug_override(**switches):
        o = ops.attention(q, k, v, case.heads, case.dh ** -0.5, out=out, math=math, scales=scales)
        torch.cuda.synchronize()
    return o


def _gates(tag, out, ref, heads, whole_gate, oracle_whole, oracle_row):
    whole = rel_l2(out, ref)
    row = float(_rows(out, ref, heads).max())
    row_gate = max(4.0 * oracle_row, ROW_FLOOR)
    print(f"attn_variants {tag}: whole {whole:.3e} (gate {whole_gate:.1e}, fp32 oracle {oracle_whole:.3e})  "
          f"worst row {row:.3e} (gate {row_gate:.3e}, fp32 oracle {oracle_row:.3e})")
    assert torch.isfinite(out).all(), tag
    assert whole < whole_gate, (tag, whole, whole_gate)
    assert row < row_gate, (tag, row, row_gate)


def _maths():
    L, _, _ = _mods()
    return {"f16x3": L.MATH_F16X3, "fp32": L.MATH_FP32, "f16": L.MATH_F16}


# ---- 1. variant matrix against fp64 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_variant_matrix_against_fp64(case):
    L, ops, _ = _mods()
    q, k, v, ref, o_whole, o_row = _data(case)
    if case is IMG_CASE:
        assert L.load().cs_attn_f16x3_ws_bytes(case.nb, case.nq, case.nk, case.heads, case.dh) > 0
    ops.read_status()
    for name, gate in (("f16x3", GATE16), ("fp32", TOL)):
        qd, kd, vd, out = _operands(case, q, k, v)
        o = _run(case, qd, kd, vd, _maths()[name], out=out)
        assert ops.read_status() == 0
        _gates(f"{_id(case)} {name}", o, ref, case.heads, gate, o_whole, o_row)
        if out is not None:         # the pad columns of the wider output stay as allocated
            assert float(out._base[..., :4].abs().max()) == 0.0 and float(out._base[..., 4 + q.shape[-1]:].abs().max()) == 0.0
    if case.nq == 1 and case.nk == 1:
        assert rel_l2(o, v) < GATE16        # one key: softmax = 1, output = v


# ---- 2. softmax paths ------------------------------------------------------------------------------------------------
SOFTMAX_CASES = [Case(1, 200, 200, 2, 40, ""), Case(1, 520, 200, 2, 40, "nw8"), Case(1, 200, 200, 2, 84, "")]


def _aligned(case, seed):
    """q_i = u + noise with scale * |u|^2 = 1 per head: the logit of key k_j = s u is s * (1 + small) for every query"""
    u = _rand(1, 1, case.heads, case.dh, seed=seed)
    u = u / u.norm(dim=-1, keepdim=True) * case.dh ** 0.25
    q = u + 0.1 * _rand(case.nb, case.nq, case.heads, case.dh, seed=seed + 1)
    return u, q.reshape(case.nb, case.nq, -1).contiguous()


def _check_softmax(case, tag, q, k, v):
    ref, o_whole, o_row = _oracle(q, k, v, case.heads)
    for name, gate in (("f16x3", GATE16), ("fp32", TOL)):
        o = _run(case, q.cuda(), k.cuda(), v.cuda(), _maths()[name])
        _gates(f"{_id(case)} {tag} {name}", o, ref, case.heads, max(4.0 * o_whole, gate), o_whole, o_row)


@pytest.mark.parametrize("order", ["rising", "falling"])
@pytest.mark.parametrize("case", SOFTMAX_CASES, ids=_id)
def test_running_max_moves_in_every_tile(case, order):
    """logits that rise with the key index for every query (ramp over +-30): the running maximum moves and the alpha rescale
    is live in every key tile; reversed, the first tile holds the maximum and every later tile is rescaled against it.
    Whole-tensor gate: max(4 x the fp32 CPU oracle, the per-op gate) -- logits of magnitude 30 cost fp32 itself
    30 * 2^-24 in every exponent."""
    u, q = _aligned(case, 910)
    s = torch.linspace(-30.0, 30.0, case.nk)
    if order == "falling":
        s = s.flip(0)
    k = (s.view(1, -1, 1, 1) * u).reshape(1, case.nk, -1).contiguous()
    v = _rand(case.nb, case.nk, case.heads * case.dh, seed=912)
    sim = torch.einsum("bihd,bjhd->bhij", q.double().reshape(1, case.nq, case.heads, -1),
                       k.double().reshape(1, case.nk, case.heads, -1))
    d = sim[..., 1:] - sim[..., :-1]
    assert bool((d > 0).all() if order == "rising" else (d < 0).all())
    _check_softmax(case, order, q, k, v)


@pytest.mark.parametrize("case", SOFTMAX_CASES, ids=_id)
def test_zero_queries_average_the_values(case):
    _, k, v = _inputs(case, seed=920)
    q = torch.zeros(case.nb, case.nq, case.heads * case.dh)
    mean = v.double().mean(dim=1, keepdim=True).expand(-1, case.nq, -1)
    for name, gate in (("f16x3", GATE16), ("fp32", TOL)):
        o = _run(case, q.cuda(), k.cuda(), v.cuda(), _maths()[name])
        e = rel_l2(o, mean)
        print(f"attn_variants {_id(case)} q=0 {name}: {e:.3e}")
        assert e < gate


@pytest.mark.parametrize("case", SOFTMAX_CASES, ids=_id)
def test_only_key_of_the_ragged_tile_dominates(case):
    """nk = 3 * 64 + 1: the last key tile holds one valid key, and that key takes (nearly) all the weight of every query"""
    nk = 193
    u, q = _aligned(case, 930)
    k = _rand(case.nb, nk, case.heads * case.dh, seed=931)
    v = _rand(case.nb, nk, case.heads * case.dh, seed=932)
    k[:, nk - 1] = (30.0 * u).reshape(1, -1)
    _check_softmax(case, "spike-at-last-key", q, k, v)
    ref = _oracle(q, k, v, case.heads)[0]
    assert rel_l2(ref, v[:, nk - 1:nk].double().expand(-1, case.nq, -1)) < 1e-3     # the spike does dominate


# ---- 3. what lies outside the view must not matter -------------------------------------------------------------------
READ_CASES = [CASES[1], CASES[3], CASES[5], CASES[7], CASES[10], CASES[12], IMG_CASE]
MATHS = ["f16x3", "fp32", "f16"]


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("case", READ_CASES, ids=_id)
def test_nothing_outside_the_views_is_read(case, math):
    """rows >= nk of the K / V allocations and the pad columns of every operand hold 0, NaN or 1e30: same bits out, status 0.
    Fails if a tail is loaded and then multiplied by zero, or if the overflow report looks at masked operands."""
    _, ops, _ = _mods()
    q, k, v = _data(case)[:3]
    c = q.shape[-1]
    outs = []
    ops.read_status()
    for fill in (0.0, float("nan"), 1e30):
        qd = _place(q, c + 8, 4, 3, fill)[1]
        kd = _place(k, c + 16, 8, 70, fill)[1]
        vd = _place(v, c + 12, 4, 70, fill)[1]
        outs.append(_run(case, qd, kd, vd, _maths()[math]))
        assert ops.read_status() == 0, fill
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("case", NW8_CASES + [CASES[10], IMG_CASE], ids=_id)
def test_nothing_outside_the_output_view_is_written(case, math):
    q, k, v = _data(case)[:3]
    c = q.shape[-1]
    rows = case.nb * case.nq
    buf = torch.empty((rows + 5, c + 12), dtype=torch.float32, device="cuda")
    bits = buf.view(torch.int32)
    bits.fill_(SENTINEL)
    out = buf[:rows].view(case.nb, case.nq, c + 12)[..., 4:4 + c]
    plain = _run(case, q.cuda(), k.cuda(), v.cuda(), _maths()[math])
    _run(case, q.cuda(), k.cuda(), v.cuda(), _maths()[math], out=out)
    assert torch.equal(out, plain)
    assert bool((bits[:, :4] == SENTINEL).all()) and bool((bits[:, 4 + c:] == SENTINEL).all())
    assert bool((bits[rows:] == SENTINEL).all())


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("case,b,h", [(CASES[5], 0, 1), (CASES[7], 1, 0), (CASES[13], 0, 1)],
                         ids=lambda x: _id(x) if isinstance(x, Case) else str(x))
def test_a_nan_key_stays_inside_its_sample_and_head(case, b, h, math):
    q, k, v = _data(case)[:3]
    dh = case.dh
    clean = _run(case, q.cuda(), k.cuda(), v.cuda(), _maths()[math])
    k2 = k.clone()
    k2[b, case.nk - 1, h * dh + dh - 1] = float("nan")        # last valid key (ragged tile), last channel of the head
    bad = _run(case, q.cuda(), k2.cuda(), v.cuda(), _maths()[math])
    nan = torch.isnan(bad)
    want = torch.zeros_like(nan)
    want[b, :, h * dh:(h + 1) * dh] = True
    assert torch.equal(nan, want)
    assert torch.equal(bad[~want], clean[~want])


# ---- 4. bit-identities the source promises ---------------------------------------------------------------------------
@pytest.mark.parametrize("math", ["f16x3", "f16"])
@pytest.mark.parametrize("case", NW8_CASES, ids=_id)
def test_four_waves_equal_eight_waves(case, math):
    """attn16_dispatch: "Same per-query arithmetic either way: bit-identical" """
    q, k, v = (t.cuda() for t in _data(case)[:3])
    four = _run(case, q, k, v, _maths()[math], route="")
    eight = _run(case, q, k, v, _maths()[math], route="nw8")
    assert torch.isfinite(four).all()
    assert torch.equal(four, eight)


def test_image_path_equals_in_kernel_split_when_nq_differs_from_nk():
    L, ops, _ = _mods()
    case = IMG_CASE
    lib = L.load()
    c = case.heads * case.dh
    assert lib.cs_attn_f16x3_ws_bytes(case.nb, case.nq, case.nk, case.heads, case.dh) > 0
    q, k, v = _fused(*_data(case)[:3])
    ops.read_status()
    new = _run(case, q, k, v, L.MATH_F16X3)
    old = torch.empty_like(new)
    L.check(lib.cs_attn_selfattn_f16x3(q.data_ptr(), k.data_ptr(), v.data_ptr(), old.data_ptr(), case.nb, case.nq, case.nk,
                                       case.heads, case.dh, 3 * c, 3 * c, 3 * c, c, case.dh ** -0.5,
                                       ops.status_word().data_ptr(), None), "cs_attn_selfattn_f16x3")
    torch.cuda.synchronize()
    off = _run(case, q, k, v, L.MATH_F16X3, no_attn_img=1)
    assert ops.read_status() == 0
    assert torch.isfinite(new).all()
    assert torch.equal(new, old) and torch.equal(new, off)


# one shape per DB, nb * heads no multiple of 8, and the two eight-wave kernels
IDENT_CASES = [Case(3, 67, 65, 3, 20, ""), Case(3, 129, 65, 3, 36, ""), Case(3, 100, 200, 2, 68, ""),
               Case(3, 130, 130, 2, 100, ""), Case(3, 70, 33, 2, 132, ""), Case(3, 520, 70, 3, 40, "nw8"),
               Case(3, 300, 90, 3, 84, "nw8")]


@pytest.mark.parametrize("math", ["f16x3", "f16"])
@pytest.mark.parametrize("case", IDENT_CASES, ids=_id)
def test_samples_and_heads_are_independent(case, math):
    """sample b of a batch of three == that sample run alone; permuting the heads of q, k and v permutes the output's
    heads -- both bit for bit"""
    m = _maths()[math]
    q, k, v = (t.cuda() for t in _inputs(case, seed=940))
    full = _run(case, q, k, v, m)
    assert torch.isfinite(full).all()
    for b in range(case.nb):
        one = _run(case, q[b:b + 1].contiguous(), k[b:b + 1].contiguous(), v[b:b + 1].contiguous(), m)
        assert torch.equal(one[0], full[b]), b
    perm = list(range(1, case.heads)) + [0]
    ph = lambda t: t.reshape(*t.shape[:2], case.heads, case.dh)[:, :, perm].reshape(t.shape).contiguous()
    assert torch.equal(_run(case, ph(q), ph(k), ph(v), m), ph(full))


@pytest.mark.parametrize("math", ["f16x3", "f16"])
def test_eight_wave_kernel_is_reproducible_run_to_run(math):
    case = NW8_CASES[0]
    q, k, v = (t.cuda() for t in _data(case)[:3])
    a = _run(case, q, k, v, _maths()[math])
    b = _run(case, q, k, v, _maths()[math])
    assert torch.equal(a, b)


# ---- 5. the overflow report, per variant -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_overflow_report_per_variant(case):
    """|operand| * QK_SCALE (16, ops.py) >= 65504 raises CS_STATUS_F16X3_OVERFLOW when the operand is inside the view -- here
    5000 at the last valid key, in the ragged tile -- and only then: the same value one row past the view raises nothing.
    With the operand scales the hosts' own rule gives for these tensors (ops.bound_a_scale of max |q| * scale, max |k|, max |v|:
    the largest powers of two that keep each inside the fp16 range -- 8 for the tensor that holds 5000) the same inputs run
    unflagged, at the matrix gates against fp64.  Measured and not used: scales of (1, 1, 1) and of (16, 8, 8) run unflagged
    too, but a q entry of ~1e-3 then has its lo half among the fp16 subnormals (absolute 2^-25 / q_scale on the operand, times
    5000): the rows in which the 5000-key competes for weight measured 8.2e-5 and 5.9e-6 at worst (fp32 oracle 4e-7 .. 8e-7).
    That floor is the F16X3 format's, the same in every variant, and the reason operands ride the largest scale they can."""
    L, ops, _ = _mods()
    q, k, v = _data(case)[:3]
    c = q.shape[-1]
    big = 5000.0
    qd = q.cuda()
    (kb, kd), (vb, vd) = _place(k, c + 8, 4, 1), _place(v, c + 8, 4, 1)
    ops.read_status()
    clean = _run(case, qd, kd, vd, L.MATH_F16X3)
    assert ops.read_status() == 0
    for name, view, ch in (("k", kd, c - 1), ("v", vd, 0)):
        keep = float(view[-1, -1, ch])
        view[-1, -1, ch] = big
        _run(case, qd, kd, vd, L.MATH_F16X3)
        assert ops.read_status() & L.STATUS_F16X3_OVERFLOW, name
        # the same inputs under scales that keep 5000 inside the fp16 range
        kc, vc = kd.cpu().contiguous(), vd.cpu().contiguous()
        ref, o_whole, o_row = _oracle(q, kc, vc, case.heads)
        sc = (ops.bound_a_scale(float(q.abs().max()) * case.dh ** -0.5), ops.bound_a_scale(float(kc.abs().max())),
              ops.bound_a_scale(float(vc.abs().max())))
        assert 5000.0 * sc["qkv".index(name)] < 65504.0
        o = _run(case, qd, kd, vd, L.MATH_F16X3, scales=sc)
        assert ops.read_status() == 0, name
        _gates(f"{_id(case)} {name}=5000 scales={sc}", o, ref, case.heads, GATE16, o_whole, o_row)
        view[-1, -1, ch] = keep
    kb[-1, 4 + c - 1] = big          # row nk of the last sample: one past the view
    vb[-1, 4] = big
    past = _run(case, qd, kd, vd, L.MATH_F16X3)
    assert ops.read_status() == 0
    assert torch.equal(past, clean)


# ---- 6. plain fp16 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_plain_fp16_matrix_is_finite_and_its_tail_no_worse_than_its_body(case):
    """MATH_F16 is reported, not gated (test_plain_fp16_attention_option_is_reported_not_gated): finite, status 0, and the rows
    of a ragged last query tile no worse than twice the worst row of the whole tiles of the same launch."""
    L, ops, _ = _mods()
    q, k, v, ref = _data(case)[:4]
    ops.read_status()
    qd, kd, vd, out = _operands(case, q, k, v)
    o = _run(case, qd, kd, vd, L.MATH_F16, out=out)
    assert ops.read_status() == 0
    assert torch.isfinite(o).all()
    rows = _rows(o, ref, case.heads)
    tile = 256 if case.route else 128         # queries per workgroup of the kernel the case reaches (32 * NW)
    whole = (case.nq // tile) * tile
    print(f"attn_variants {_id(case)} f16: whole {rel_l2(o, ref):.3e} worst row {float(rows.max()):.3e}", end="")
    if 0 < whole < case.nq:
        body, tail = float(rows[:, :whole].max()), float(rows[:, whole:].max())
        print(f"  body {body:.3e} tail ({case.nq - whole} queries) {tail:.3e}")
        assert tail <= 2.0 * body, (tail, body)
    else:
        print()
