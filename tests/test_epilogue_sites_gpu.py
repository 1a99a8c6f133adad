"""Every site that applies csrc/cs_epilogue.h -- the epilogue terms, the interleaved pair, the fp64 column sums -- gives the
same bits from the same accumulators, and those bits are right against an oracle that is not the library.

Inputs are integers: activations and weights in -4 .. 4 (times the power-of-two operand scales: exact fp16 `hi`, `lo` = 0),
K <= 27 * 32 terms (|sum| < 2^14), an integer bias, `scale` = +-2^k per column with an integer `shift`, an integer row
vector with rv_rows = 11 (cuts through every tile, divides no row count here; the launches meant for the piped epilogue, which
takes one row-vector row per tile and is granted its extras only for rv_rows % tile rows == 0, use rv_rows = the tile's rows,
64 or 256: above 1, and no divisor of the ragged row counts 130 and 210), NONE / RELU, an integer residual at its own ldr.
Every route's accumulation is then exact whatever its K partition, and the expected output is an int64 computation in
numpy with no rounding anywhere: the comparison is torch.equal -- on the fp32 output, on the decoded pair (whose `lo` half
must be all zero: the pair cases keep |out| < 2048, asserted on the oracle) and on the GroupNorm partials (fp64 sums of
integers and of their squares).  Each launch asks for exactly the extras cs_conv_gemm_epilogue_caps grants it (ops.conv_gemm
asks: stats=True / out_pair=), the tile it ran is read back from cs_conv_gemm_launch_info (ops.GEMM_PROFILE), and the test
states per site which extras that rule grants and asserts that they came back (a Pair16, partials): a site whose extras were
silently dropped fails.

Sites: the 64x64 one-tap tile at M = 130, cin = 32, cout = 72 (float4 paths: piped without scale / shift, plain with) and
cout = 70 (scalar tail), and at M = 2 x 64 -- ragged columns only -- where the statistics tiles fit the samples and the
launches are granted the partials; the K-wave kernel and its one-chain twin; the fp32-input kernel; a 3x3x3 conv (2x3x5x7, the
smallest slab geometry of test_gemm_variants_gpu.py, and 2x4x4x4 where the reduce is granted the partials) on the 256x64 tile
unsliced and in two K slices with the two-kernel reduce (splitk_reduce_kernel without extras, splitk_reduce_epi_kernel with);
the FUSED reduce at cout = 224 on the 256x224 slice tile, 2x4x4x4 -- that site cannot have a ragged column tile (the host rule
fused_reduce_plan admits whole 224-column tiles on slice tiles 2 / 4 only), and no ABI entry reports which form a launch
took, so the test asserts every condition of that rule on the launch it makes and runs the two-kernel form beside it;
cs_conv_wino_output<2 / 4> on a hand-written integer workspace of three slices (its factors 2, 4, 8 keep integers exact),
cout = 224: a ragged last 64-column block.  (The ragged slice counts of the Winograd tail plan need a 22 x 8^3 volume at
672 columns: they stay with test_wino_variants_gpu.py's tail-plan tests.)

test_transcendental_activations_agree_across_sites is a CONSISTENCY check, not an oracle test: with SiLU / GELU nothing exact
exists, so it asserts that all sites that ran the same case agree bit for bit and lie within the per-op gate (1e-6 rel-L2)
of an fp64 evaluation."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import rel_l2

import _wino_cases as W
import test_wino_variants_gpu as WV

pytestmark = pytest.mark.gpu

RV_CUT = 11                      # rv_rows that cuts through every tile and divides none of 128, 130, 210, 512, 1024
PAIR_SCALE = 0.5                 # a power of two: |out| < 2048 (eleven bits) is then exact in the fp16 hi half


def _mods():
    from commonscenes_amd import lib as L, ops
    return L, ops


def _ints(rng, *shape, lim=4):
    return rng.integers(-lim, lim + 1, size=shape).astype(np.int64)


def _case(m, cin, cout, k, seed, with_scale, act, rv_rows=RV_CUT):
    """int64 operands and epilogue terms of a GEMM with m output rows; x is [m, cin] (k = 1) or a volume"""
    rng = np.random.default_rng(seed)
    t = dict(wt=_ints(rng, cout, cin, *([k] * 3 if k > 1 else [])), bias=_ints(rng, cout, lim=9), rv_rows=rv_rows,
             rv=_ints(rng, -(-m // rv_rows), cout, lim=9), res=_ints(rng, m, cout, lim=9), act=act, scale=None, shift=None)
    if with_scale:
        t["scale"] = rng.choice([-2, -1, 1, 2], size=cout).astype(np.int64)
        t["shift"] = _ints(rng, cout, lim=9)
    return rng, t


def _epilogue64(acc, t):
    """bias, scale / shift, row vector (row m / rv_rows), activation, residual -- in int64"""
    v = acc + t["bias"]
    if t["scale"] is not None:
        v = v * t["scale"] + t["shift"]
    v = v + t["rv"][np.arange(v.shape[0]) // t["rv_rows"]]
    if t["act"] == 1:
        v = np.maximum(v, 0)
    return v + t["res"]


def _f(a):
    return torch.from_numpy(np.ascontiguousarray(a)).float().cuda()


def _view(rows, cols, ld):
    buf = torch.zeros((rows, ld), dtype=torch.float32, device="cuda")
    return buf[:, :cols]


def _run(x, pk, t, m, cout, *, pair=False, stats=True, **kw):
    """one ops.conv_gemm with the case's terms -> (fp32 output or Pair16, partials or None, the tile it ran)"""
    L, ops = _mods()
    switches = kw.pop("switches", {})
    res = _view(m, cout, cout + 8)
    res.copy_(_f(t["res"]))
    out = _view(m, cout, (cout + 15) // 16 * 16 + 16)         # ldo % 16 == 0, rows on 64 bytes: the pair's geometry
    args = dict(act=t["act"], rowvec=_f(t["rv"]), rv_rows=t["rv_rows"], res=res, out=out, stats=stats,
                scale=None if t["scale"] is None else _f(t["scale"]), shift=None if t["shift"] is None else _f(t["shift"]))
    if pair:
        args["out_pair"] = PAIR_SCALE
    ops.read_status()
    ops.GEMM_PROFILE = prof = []
    try:
        with L.debug_override(**switches):
            y = ops.conv_gemm(x, pk, **args, **kw)
        torch.cuda.synchronize()
    finally:
        ops.GEMM_PROFILE = None
    assert ops.read_status() == 0
    st = getattr(y, "cs_stats", None)
    return y, st, prof[-1]["tile"]


def _check(tag, y, st, exp, cout, pair=None, stats=None):
    """fp32 output / pair / partials of one launch against the int64 result `exp` [m, cout]; pair / stats (not None): whether
    the caps rule grants this launch the pair it asked for / the partials -- what came back must say the same"""
    L, ops = _mods()
    want = torch.from_numpy(exp).float()
    assert float(np.abs(exp).max()) < 2 ** 24
    if pair is not None:
        assert isinstance(y, ops.Pair16) == pair, (tag, "pair output", type(y), pair)
    if stats is not None and not isinstance(y, ops.Pair16):          # (a Pair16 carries no partials)
        assert (st is not None) == stats, (tag, "partials", st is not None, stats)
    if isinstance(y, ops.Pair16):
        assert float(np.abs(exp).max()) < 2048, "the pair cases must stay exactly representable in fp16"
        hi, lo = W.pair_decode(y.t.reshape(-1, y.t.shape[-1]).cpu(), cout)
        assert torch.equal(hi.float(), want * PAIR_SCALE), (tag, "pair hi")
        assert int((lo != 0).sum()) == 0, (tag, "pair lo")
    else:
        got = y.reshape(-1, cout).cpu()
        assert torch.equal(got, want), (tag, int((got != want).sum()), float((got - want).abs().max()))
    if st is not None:
        assert st.part.shape[0] == st.nb * st.tps and exp.shape[0] % (st.nb * st.tps) == 0, (tag, st.part.shape, st.nb, st.tps)
        rows = exp.shape[0] // (st.nb * st.tps)
        e = exp.reshape(-1, rows, cout)
        part = st.part.cpu()[:, :cout]
        assert torch.equal(part[..., 0], torch.from_numpy(e.sum(1)).double()), (tag, "partial sums")
        assert torch.equal(part[..., 1], torch.from_numpy((e * e).sum(1)).double()), (tag, "partial sums of squares")


# ---- the one-tap sites at M = 130 ----------------------------------------------------------------------------------------------
CIN1 = 32
SPATIAL = {130: None, 128: (2, 64, 1, 1)}


def _one_tap_sites(m, cout, t, x64):
    """[(site, output, partials, pair asked)] of every one-tap site that takes the case, each without and with the pair asked"""
    L, ops = _mods()
    x, wt, bias = _f(x64), _f(t["wt"]), _f(t["bias"])
    pk16 = ops.pack_weight(wt, bias, cin_pad=CIN1, math=L.MATH_F16X3)
    pk32 = ops.pack_weight(wt, bias, cin_pad=CIN1)
    runs, sp = [], dict(spatial=SPATIAL[m])
    for pair in (False, True):
        y, st, tile = _run(x, pk16, t, m, cout, pair=pair, tile=3, **sp)
        assert tile == 3
        runs.append((f"64x64 tile pair={pair}", y, st, pair))
        if cout % 4 == 0:
            y, st, tile = _run(x, pk16, t, m, cout, pair=pair, tile=10, **sp)
            assert tile == 10
            runs.append((f"K-wave pair={pair}", y, st, pair))
        y, st, tile = _run(x, pk16, t, m, cout, pair=pair, switches=dict(no_kwave=1), **sp)
        assert tile == 3
        runs.append((f"one-chain twin pair={pair}", y, st, pair))
    y, st, _ = _run(x, pk32, t, m, cout, **sp)
    runs.append(("fp32-input kernel", y, st, False))
    return runs


@pytest.mark.parametrize("act", [0, 1], ids=["none", "relu"])
@pytest.mark.parametrize("with_scale", [False, True], ids=["piped", "scale-shift"])
@pytest.mark.parametrize("cout", [72, 70], ids=["float4", "scalar-tail"])
@pytest.mark.parametrize("m", [130, 128], ids=["M130", "M2x64"])
def test_one_tap_sites_against_the_integer_oracle(m, cout, with_scale, act):
    rng, t = _case(m, CIN1, cout, 1, 100 + m + cout + 2 * with_scale + act, with_scale, act, RV_CUT if with_scale else 64)
    x64 = _ints(rng, m, CIN1)
    exp = _epilogue64(x64 @ t["wt"].T, t)
    # cs_conv_gemm_epilogue_caps: the K-wave kernel emits both extras whatever the terms; the 64x64 tile only from its piped
    # epilogue (float4 rows, no scale / shift, rv_rows % 64 == 0); the pair needs cout % 8 == 0, the partials 64-row samples
    for site, y, st, asked in _one_tap_sites(m, cout, t, x64):
        emits = cout % 4 == 0 and (site.startswith("K-wave") or (not with_scale and not site.startswith("fp32")))
        _check(site, y, st, exp, cout, pair=asked and emits and cout % 8 == 0, stats=emits and m == 128)


# ---- the 3x3x3 conv: unsliced, two-kernel reduce, fused reduce -------------------------------------------------------------------
CIN3, COUT3 = 32, 72


def _conv64(x64, wt):
    """3x3x3, stride 1, pad 1, in int64 -> [rows, cout]"""
    vol = x64.shape[:4]
    xp = np.pad(x64, ((0, 0), (1, 1), (1, 1), (1, 1), (0, 0)))
    acc = np.zeros((*vol, wt.shape[0]), dtype=np.int64)
    for a in range(3):
        for b in range(3):
            for c in range(3):
                acc += xp[:, a:a + vol[1], b:b + vol[2], c:c + vol[3]] @ wt[:, :, a, b, c].T
    return acc.reshape(-1, wt.shape[0])


@pytest.mark.parametrize("act", [0, 1], ids=["none", "relu"])
@pytest.mark.parametrize("with_scale", [False, True], ids=["plain", "scale-shift"])
@pytest.mark.parametrize("VOL", [(2, 3, 5, 7), (2, 4, 4, 4)], ids=["2x3x5x7", "2x4x4x4"])
def test_sliced_conv_sites_against_the_integer_oracle(VOL, with_scale, act):
    """2 x 3 x 5 x 7: ragged rows and columns; 2 x 4 x 4 x 4: 64-row samples, where the reduce kernel is granted the partials.
    The 256x64 tile never takes the fused reduce (fused_reduce_plan): the sliced launches here are the two-kernel form."""
    L, ops = _mods()
    m = VOL[0] * VOL[1] * VOL[2] * VOL[3]
    rng, t = _case(m, CIN3, COUT3, 3, 300 + m + 2 * with_scale + act, with_scale, act, RV_CUT if with_scale else 256)
    x64 = _ints(rng, *VOL, CIN3, lim=2)
    exp = _epilogue64(_conv64(x64, t["wt"]), t)
    x = _f(x64)
    pk = ops.pack_weight(_f(t["wt"]), _f(t["bias"]), cin_pad=CIN3, math=L.MATH_F16X3)
    rps = m // VOL[0]
    for pair in (False, True):
        # caps: unsliced = the piped epilogue (no scale / shift, rv_rows % 256 == 0), partials only for rps % 256 == 0; the
        # reduce kernel emits the pair whatever the terms and the partials of its 16-row blocks for rps % 16 == 0
        for site, kw, emits, st_ok in (
                ("unsliced", dict(splitk=1), not with_scale, False),
                ("two-kernel reduce, no extras asked", dict(splitk=2, stats=False, switches=dict(no_fused_reduce=1)), True, False),
                ("two-kernel reduce", dict(splitk=2, switches=dict(no_fused_reduce=1)), True, rps % 16 == 0)):
            if pair and kw.get("stats") is False:
                continue
            y, st, tile = _run(x, pk, t, m, COUT3, pair=pair, tile=7, **kw)
            assert tile == 7
            _check(f"{site} pair={pair}", y, st, exp, COUT3, pair=pair and emits, stats=st_ok)


@pytest.mark.parametrize("act", [0, 1], ids=["none", "relu"])
@pytest.mark.parametrize("with_scale", [False, True], ids=["plain", "scale-shift"])
def test_fused_reduce_site_against_the_integer_oracle(with_scale, act):
    """fused_splitk_reduce, the one site that keeps a written-out copy of the pair conversion and the 16-row column sum: two K
    slices of a 2 x 4 x 4 x 4 conv with 224 columns on the 256x224 slice tile, beside the two-kernel form of the same launch"""
    L, ops = _mods()
    vol, cout, slices = (2, 4, 4, 4), 224, 2
    m = vol[0] * vol[1] * vol[2] * vol[3]
    rng, t = _case(m, CIN3, cout, 3, 400 + 2 * with_scale + act, with_scale, act)
    x64 = _ints(rng, *vol, CIN3, lim=2)
    exp = _epilogue64(_conv64(x64, t["wt"]), t)
    x = _f(x64)
    pk = ops.pack_weight(_f(t["wt"]), _f(t["bias"]), cin_pad=CIN3, math=L.MATH_F16X3)
    # fused_reduce_plan (cs_gemm.hip), condition by condition: arrival counters passed (ops.conv_gemm does for every sliced
    # F16X3 launch), the switch off, slice tile 2 or 4 (asserted below from launch_info), whole 224-column tiles, every
    # workgroup resident at once (one per CU on the 256-row tile), two counter words per tile
    tiles = -(-m // 256) * (cout // 224)
    assert cout % 224 == 0 and tiles * slices <= torch.cuda.get_device_properties(0).multi_processor_count
    assert 2 * tiles <= ops.SYNC_WORDS
    for pair in (False, True):
        for site, fused in (("two-kernel reduce", 0), ("fused reduce", 1)):
            y, st, tile = _run(x, pk, t, m, cout, pair=pair, splitk=slices, switches=dict(no_fused_reduce=1 - fused))
            assert tile == 4
            _check(f"{site} pair={pair}", y, st, exp, cout, pair=pair, stats=True)
    assert int(ops.sync_words().abs().sum().item()) == 0, "arrival counters must return to zero"


# ---- the Winograd output transform on an integer workspace -------------------------------------------------------------------------
@pytest.mark.parametrize("act", [0, 1], ids=["none", "relu"])
@pytest.mark.parametrize("variant", [2, 4], ids=["F(2,3)", "F(4,3)"])
def test_wino_output_against_the_integer_oracle(variant, act):
    L, _ = _mods()
    vol, cout, slices = W.GEOM[variant]["W4"], 224, 3
    m = W.rows_of(vol)
    rng, t = _case(m, 1, cout, 1, 500 + variant + act, True, act)
    ws = torch.from_numpy(_ints(rng, slices, variant + 2, m // variant, cout, lim=4)).float()
    e = W.Epi(*(torch.from_numpy(t[k]).float() for k in ("bias", "scale", "shift", "rv")), RV_CUT, act,
              torch.from_numpy(t["res"]).float())
    at = np.array(W.AT[variant], dtype=np.int64)
    y64 = np.einsum("eq,qtc->tec", at, ws.numpy().astype(np.int64).sum(0)).reshape(m, cout)
    exp = _epilogue64(y64, t)
    caps = WV._desc(vol, 16, cout, variant)
    caps.ldo, caps.out = cout + 16, 64
    rows, pair = C.c_int32(0), C.c_int32(0)
    L.check(L.load().cs_conv_gemm_epilogue_caps(C.byref(caps), C.byref(rows), C.byref(pair)), "cs_conv_gemm_epilogue_caps")
    assert rows.value == 16 * variant and pair.value == 1          # the route offers both extras at this geometry
    want = torch.from_numpy(exp).float()
    out, gnb = WV._run_output(variant, vol, cout, ws, slices, e, True, gn=True)
    assert torch.equal(out.cpu(), want)
    ex = exp.reshape(-1, 16 * variant, cout)
    part = gnb[1].cpu().reshape(ex.shape[0], cout, 2)
    assert torch.equal(part[..., 0], torch.from_numpy(ex.sum(1)).double())
    assert torch.equal(part[..., 1], torch.from_numpy((ex * ex).sum(1)).double())
    assert float(np.abs(exp).max()) < 2048
    words, _ = WV._run_output(variant, vol, cout, ws, slices, e, True, gn=True, pair_scale=PAIR_SCALE)
    hi, lo = W.pair_decode(words.cpu(), cout)
    assert torch.equal(hi.float(), want * PAIR_SCALE) and int((lo != 0).sum()) == 0


# ---- SiLU / GELU: consistency only ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [2, 3], ids=["silu", "gelu"])
@pytest.mark.parametrize("cout", [72, 70], ids=["float4", "scalar-tail"])
def test_transcendental_activations_agree_across_sites(cout, act):
    """CONSISTENCY check (no exact oracle exists for expf / erff): every site that ran the case gives the same bits, and they
    lie within the per-op gate of the fp64 evaluation"""
    m = 130
    rng, t = _case(m, CIN1, cout, 1, 700 + cout + act, False, act)
    x64 = _ints(rng, m, CIN1)
    # activations, bias and row vector carry a factor 1 / 64 (exact in every format on the way): the sums land in the curved
    # range of the activation, and the pre-activation value is still the same exact number at every site
    pre = torch.from_numpy(_epilogue64(x64 @ t["wt"].T, dict(t, act=0, res=np.zeros_like(t["res"])))).double() / 64.0
    ref = W.act64(pre, act) + torch.from_numpy(t["res"]).double()
    L, ops = _mods()
    x = _f(x64) / 64.0
    wt, bias = _f(t["wt"]), _f(t["bias"]) / 64.0
    tt = dict(t, rv=t["rv"] / 64.0)
    pk16 = ops.pack_weight(wt, bias, cin_pad=CIN1, math=L.MATH_F16X3)
    pk32 = ops.pack_weight(wt, bias, cin_pad=CIN1)
    outs = [("64x64 tile", _run(x, pk16, tt, m, cout, tile=3)[0]),
            ("one-chain twin", _run(x, pk16, tt, m, cout, switches=dict(no_kwave=1))[0]),
            ("fp32-input kernel", _run(x, pk32, tt, m, cout)[0])]
    if cout % 4 == 0:
        outs.append(("K-wave", _run(x, pk16, tt, m, cout, tile=10)[0]))
    for site, y in outs:
        err = rel_l2(y.reshape(-1, cout), ref)
        print(f"epilogue_sites act {act} cout {cout} {site}: rel-L2 vs fp64 {err:.3e}")
        assert err < 1e-6, (site, err)
        assert torch.equal(y, outs[0][1]), (site, "differs from " + outs[0][0])
