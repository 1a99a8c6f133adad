"""The case tables, fp64 references and bounds of test_wino_variants_{cpu,gpu}.py: the Winograd-W conv route (cs_gemm.hip:
pack_f16x3_wino_kernel, the stacked position GEMMs of conv_wino, wino_out_kernel<2> / <4>) and the split-K reduce pair
(splitk_reduce_kernel, splitk_reduce_epi_kernel), piecewise.  No test functions here.

The transforms, written out (F(R,3) along W, P = R + 2 positions, tile t of a line covers outputs R t .. R t + R - 1):
  image q   = sum_j BT[q][j] d[R t - 1 + j]        (zero outside the line; gn_apply_wino_kernel, tests/_norm_cases.py::BT)
  weight q  = sum_k G[q][k] g[.., k]               (pack_f16x3_wino_kernel)
  m_q       = the 3x3x1 conv (pads 1 / 1 / 0) of image q with weight q over (D, H, W / R)      (the position GEMMs)
  output e  = sum_q AT[e][q] m_q                   (wino_out_kernel)
test_wino_variants_cpu.py checks that their composition is F.conv3d in fp64.

Workspace of a position launch: fp32 [slices][P][M / R][cout]; the output transform sums the slices of a (position, column) in
slice order -- `nsl` [P, cout] slices each, uniform except under the tail plan -- then forms A^T m in the order the kernel
writes it, then the epilogue: bias, scale / shift, row vector (row m / rv_rows), activation, residual.  The split-K reduce
kernels are the same with P = 1 and no transform.

The bound of an output element, u = 2^-24:  E = (a + 4) u T,  a = its slices + the non-zero coefficients of its transform row
+ its epilogue terms (the fp32 additions / multiplications on its path), T = the same expression in fp64 with every term
replaced by its absolute value (the coefficients 2, 4, 8 included).  With SiLU / GELU: the pre-activation part of T times 1.13
(the largest slope) and + 4 u |ref| for expf / erff / the division.  Derived, never measured; test_wino_variants_cpu.py shows
that an fp32 CPU evaluation in the kernel's order stays inside it on every case of the two tables."""
from collections import namedtuple

import torch
import torch.nn.functional as F

from _norm_cases import ACT_GELU, ACT_NONE, ACT_SILU, BT, LIPSCHITZ, U, act32, act64, pair_value      # noqa: F401

SENTINEL = 0x5A5AA5A5          # test_gemm_variants_gpu.py's: the bit pattern of untouched output / workspace words
PRE_ROWS, POST_ROWS = 3, 5     # bands of rows before / after every view

G = {2: [[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]],
     4: [[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]]}
AT = {2: [[1, 1, 1, 0], [0, 1, -1, -1]],
      4: [[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]],
      None: [[1]]}               # None: the split-K reduce (one "position", no transform)


def _t(m):
    return torch.tensor(m, dtype=torch.float64)


def rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ---- the transforms in fp64 --------------------------------------------------------------------------------------------------
def images64(y, variant):
    """B^T d along W of y [nb, D, H, W, C] (fp64), zeros outside the line -> [P, nb, D, H, W / R, C]"""
    z = torch.zeros_like(y[:, :, :, :1])
    taps = torch.cat([z, y, z], dim=3).unfold(3, variant + 2, variant)               # [nb, D, H, W / R, C, R + 2]
    return torch.einsum("qj,ndhtcj->qndhtc", _t(BT[variant]), taps)


def weights64(w, variant):
    """G g over the kw taps of w [cout, cin, 3, 3, 3] (fp64) -> [P, cout, cin, 3, 3]"""
    return torch.einsum("qk,oidhk->qoidh", _t(G[variant]), w)


def positions64(img, u):
    """the position results [P, nb D H (W / R), cout]: per position the 3x3x1 conv, pads 1 / 1 / 0, of its image with its weight"""
    out = []
    for q in range(img.shape[0]):
        o = F.conv3d(img[q].permute(0, 4, 1, 2, 3), u[q][..., None], padding=(1, 1, 0))
        out.append(o.permute(0, 2, 3, 4, 1).reshape(-1, u.shape[1]))
    return torch.stack(out)


def transform64(m, variant):
    """A^T m of m [P, Mt, cout] -> [Mt R, cout]: row t R + e = output e of tile t (the NDHWC row order)"""
    at = _t(AT[variant])
    return torch.einsum("eq,qtc->tec", at, m).reshape(m.shape[1] * at.shape[0], m.shape[2])


def split16(v64, a_scale):
    """fp16 hi / lo of v a_scale, split on the host from fp64, and the value the pair carries: (hi + lo) / a_scale"""
    s = v64 * a_scale
    hi = s.half()
    lo = (s - hi.double()).half()
    return hi, lo, (hi.double() + lo.double()) / a_scale


def pack_order(u):
    """u [P, cout, cin, 3, 3] -> the packed layout [P][tap = kd 3 + kh][cin16 / 8][cout][8] with zeros from cin up"""
    p, cout, cin = u.shape[:3]
    cp = (cin + 15) // 16 * 16
    v = torch.zeros(p, cout, cp, 9, dtype=u.dtype)
    v[:, :, :cin] = u.reshape(p, cout, cin, 9)
    return v.reshape(p, cout, cp // 8, 8, 9).permute(0, 4, 2, 1, 3).contiguous()


# part 1: the weight pack.  form -> (cin, src_cin, c0): the whole tensor, or the channel slice c0 .. c0 + cin of src_cin channels
PACK_FORMS = {"whole-16": (16, 0, 0), "whole-24": (24, 0, 0), "slice-24-of-40": (24, 40, 16)}
PACK_COUT = 12


def pack_case(form, variant):
    """(weights [12, src_cin or cin, 3, 3, 3] fp32, the power-of-two scale ops.pack_weight_wino takes, G g of the slice in fp64)
    The gate 2^-21 |u| + 2^-24 2^-14 / scale has no room for a lo half that is an fp16 subnormal (spacing 2^-24 in scaled units,
    i.e. values below 2^-4 of them whose lo half does not vanish): about one weight in 10^5 of a normal draw.  The seed is one at
    which the EXACT split stays inside the gate (test_wino_variants_cpu.py asserts it), so the gate judges the kernel alone."""
    import math
    cin, src_cin, c0 = PACK_FORMS[form]
    wt = rand(PACK_COUT, src_cin or cin, 3, 3, 3, seed=101) * 0.05
    am = (1.5 if variant == 2 else 1.0) * float(wt.abs().max())           # max |u_q| <= 1.5 max |w| (F(2,3)), <= max |w| (F(4,3))
    return wt, 2.0 ** (14 - math.frexp(am)[1]), weights64(wt.double()[:, c0:c0 + cin], variant)


def pack_bound(u, scale):
    return 2.0 ** -21 * u.abs() + 2.0 ** -24 * 2.0 ** -14 / scale


# ---- epilogue, bound, fp32 restatement ---------------------------------------------------------------------------------------
Epi = namedtuple("Epi", "bias scale shift rv rv_rows act res", defaults=(None, None, None, None, 1, ACT_NONE, None))


def _rv_rows(e, m):
    return e.rv[torch.arange(m) // e.rv_rows]


def _masked(ws, nsl):
    """ws [S, P, Mt, cout] with every slice a (position, column) does not have replaced by 0 (it may hold NaN)"""
    live = torch.arange(ws.shape[0])[:, None, None, None] < nsl[None, :, None, :]
    return torch.where(live, ws, torch.zeros((), dtype=ws.dtype))


def reference64(ws, nsl, variant, e):
    """(ref, E) [M, cout] in fp64 of the output transform (variant 2 / 4) or the split-K reduce (None) + epilogue `e` on the
    fp32 workspace ws [S, P, Mt, cout], nsl [P, cout] slices per (position, column)"""
    w = _masked(ws.double(), nsl)
    at = _t(AT[variant])
    cv = lambda t: None if t is None else t.double()
    m = transform64(w.sum(0), variant)
    t = torch.einsum("eq,qtc->tec", at.abs(), w.abs().sum(0)).reshape(m.shape)
    # fp32 operations on the element's path: its slices (the most of its row's positions), the transform row, the terms
    nz = (at != 0)
    sl = torch.stack([nsl[nz[i]].max(0).values for i in range(at.shape[0])]).double()              # [R, cout]
    a = sl + (nz.sum(1).double()[:, None] if variant else 0.0)
    a = a.repeat(m.shape[0] // at.shape[0], 1)
    if e.bias is not None:
        m, t, a = m + cv(e.bias), t + cv(e.bias).abs(), a + 1
    if e.scale is not None:
        m, t, a = m * cv(e.scale) + cv(e.shift), t * cv(e.scale).abs() + cv(e.shift).abs(), a + 2
    if e.rv is not None:
        rv = cv(_rv_rows(e, m.shape[0]))
        m, t, a = m + rv, t + rv.abs(), a + 1
    extra = 0.0
    if e.act != ACT_NONE:
        m = act64(m, e.act)
        t, extra = LIPSCHITZ * t, 4.0 * U * m.abs()
    if e.res is not None:
        m, t, a = m + cv(e.res), t + cv(e.res).abs(), a + 1
        extra = extra + (4.0 * U * cv(e.res).abs() if e.act != ACT_NONE else 0.0)
    return m, (a + 4.0) * U * t + extra


def kernel32(ws, nsl, variant, e):
    """the kernels' expression in torch fp32 on the CPU, in the source's stated order: slice-order sums, the transform rows as
    wino_out_kernel writes them, then bias, scale / shift, row vector, activation, residual -> [M, cout] fp32.  No operation is
    contracted (the library is built with -ffp-contract=off; the products by 2, 4, 8 are exact either way)."""
    assert ws.dtype == torch.float32
    s_all, p, mt, cout = ws.shape
    mq = []
    for q in range(p):
        acc = ws[0, q].clone()
        for s in range(1, s_all):
            acc = torch.where((nsl[q] > s)[None, :], acc + ws[s, q], acc)
        mq.append(acc)
    if variant == 4:
        y0 = (((mq[0] + mq[1]) + mq[2]) + mq[3]) + mq[4]
        y1 = (mq[1] - mq[2]) + 2.0 * (mq[3] - mq[4])
        y2 = (mq[1] + mq[2]) + 4.0 * (mq[3] + mq[4])
        y3 = ((mq[1] - mq[2]) + 8.0 * (mq[3] - mq[4])) + mq[5]
        y = [y0, y1, y2, y3]
    elif variant == 2:
        y = [(mq[0] + mq[1]) + mq[2], (mq[1] - mq[2]) - mq[3]]
    else:
        y = [mq[0]]
    v = torch.stack(y, dim=1).reshape(mt * len(y), cout)
    if e.bias is not None:
        v = v + e.bias
    if e.scale is not None:
        v = v * e.scale
        v = v + e.shift
    if e.rv is not None:
        v = v + _rv_rows(e, v.shape[0])
    v = act32(v, e.act)
    if e.res is not None:
        v = v + e.res
    return v


def additive_only(e):
    return e.scale is None and e.act == ACT_NONE


# ---- guard bands, sentinel, pair decode ---------------------------------------------------------------------------------------
def place(t, ld, off, device="cpu", fill=float("nan"), bits=False):
    """2-D tensor -> (allocation, view): its copy as the [rows, cols] view at column `off` of a [PRE_ROWS + rows + POST_ROWS, ld]
    buffer of `fill` (bits: `fill` is a 32-bit pattern written over the whole float32 allocation first)"""
    rows, cols = t.shape
    assert off + cols <= ld
    buf = torch.empty((PRE_ROWS + rows + POST_ROWS, ld), dtype=t.dtype, device=device)
    if bits:
        buf.view(torch.int32).fill_(fill)
    else:
        buf.fill_(fill)
    view = buf[PRE_ROWS:PRE_ROWS + rows, off:off + cols]
    view.copy_(t)
    return buf, view


def sentinel_buffer(rows, cols, ld, off, device="cpu", dtype=torch.float32):
    """(allocation, view): a [PRE_ROWS + rows + POST_ROWS, ld] buffer whose every 32-bit word is SENTINEL, view included"""
    buf = torch.empty((PRE_ROWS + rows + POST_ROWS, ld), dtype=dtype, device=device)
    buf.view(torch.int32).fill_(SENTINEL)
    return buf, buf[PRE_ROWS:PRE_ROWS + rows, off:off + cols]


def _inside(buf, view):
    r0, off = divmod(view.storage_offset() - buf.storage_offset(), buf.shape[1])
    inside = torch.zeros(buf.shape, dtype=torch.bool, device=buf.device)
    inside[r0:r0 + view.shape[0], off:off + view.shape[1]] = True
    return inside


def untouched_outside(buf, view):
    """every 32-bit word of the allocation outside the view still holds SENTINEL"""
    words = buf.element_size() // 4
    ok = (buf.view(torch.int32).reshape(buf.shape[0], buf.shape[1], words) == SENTINEL).all(dim=2)
    return bool((ok | _inside(buf, view)).all())


def nan_outside(buf, view):
    """every element of the allocation outside the view is still NaN"""
    return bool((torch.isnan(buf) | _inside(buf, view)).all())


def pair_decode(words, cout):
    """the interleaved operand pair a kernel wrote over the first cout 32-bit words of each row of `words` [M, >= cout]
    (float32-tagged): per 8 columns 8 fp16 hi then 8 fp16 lo -> (hi, lo) [M, cout] fp16"""
    assert cout % 8 == 0
    h = words[:, :cout].contiguous().view(torch.float16).reshape(words.shape[0], cout // 8, 2, 8)
    return h[:, :, 0].reshape(-1, cout), h[:, :, 1].reshape(-1, cout)


def pair_expected(out32, out_scale):
    """(hi, lo) as the epilogues form them from the fp32 result: o = out out_scale; hi = half(o); lo = half(o - float(hi))"""
    hi, lo, _ = pair_value(out32 * out_scale, out_scale)
    return hi, lo


# ---- tables ------------------------------------------------------------------------------------------------------------------
# The smallest geometries (nb, D, H, W) at which each edge exists; the route needs M % 512 == 0 (F(2,3)), M % 1024 == 0 and W % 4
# == 0 (F(4,3)), W even, 2 <= W / 2 <= 32 and -- cout % 224 != 0, F(4,3) -- D H W % 1024 == 0 per sample.
GEOM = {2: {"D1-W64": (1, 1, 8, 64), "W4": (1, 32, 4, 4), "H1": (1, 64, 1, 8), "odd-nb": (3, 4, 8, 16), "W6": (4, 8, 8, 6),
            "W12": (2, 8, 8, 12)},
        4: {"D1-W64": (2, 1, 8, 64), "W4": (2, 32, 4, 4), "H1": (2, 64, 1, 8), "odd-nb": (3, 8, 8, 16), "W12": (4, 8, 8, 12)}}

# parts 2 and 5: positions alone and the whole route.  view: lda = cin + 8, ldo = cout + 12, own ldr / ldrv / gn_ld.
Conv = namedtuple("Conv", "variant geom cin cout view")
CONVS = [
    Conv(2, "D1-W64", 16, 64, False), Conv(2, "W4", 24, 224, True), Conv(2, "H1", 40, 128, False), Conv(2, "odd-nb", 72, 448, True),
    Conv(2, "W6", 24, 256, False), Conv(2, "W12", 40, 224, True), Conv(2, "odd-nb", 16, 64, False),
    Conv(4, "D1-W64", 24, 224, True), Conv(4, "W4", 40, 448, False), Conv(4, "H1", 16, 224, True), Conv(4, "odd-nb", 24, 128, False),
    Conv(4, "odd-nb", 72, 64, True), Conv(4, "W12", 72, 224, False), Conv(4, "odd-nb", 40, 256, True), Conv(4, "odd-nb", 16, 64, False),
]


def conv_id(c):
    return f"F{c.variant}-{c.geom}-" + "x".join(map(str, GEOM[c.variant][c.geom])) + f"-{c.cin}-{c.cout}" + ("-view" if c.view else "")


def rows_of(vol):
    return vol[0] * vol[1] * vol[2] * vol[3]


# part 3: the output transform on a synthetic workspace.  epi: bias | brr (bias + rowvec + res) | bn (bias, scale / shift, SiLU) |
# rg (res + GELU); rv: "sample" (rv_rows = the sample's rows) | 6 (cuts through the tiles of four rows) | 3 (of two); gn: GroupNorm partials.
Out = namedtuple("Out", "variant geom cout slices epi rv view gn")
OUTS = [
    Out(2, "W4", 64, 1, "bias", None, False, False), Out(2, "W4", 224, 3, "brr", "sample", True, True),
    Out(2, "H1", 448, 16, "brr", 6, False, False), Out(2, "H1", 224, 3, "bn", None, True, False),
    Out(2, "D1-W64", 64, 16, "rg", None, False, False), Out(2, "odd-nb", 448, 1, "brr", 6, True, True),
    Out(2, "W12", 224, 3, "brr", 3, False, False),     # (6 is whole F(2,3) tiles: 3 is what cuts through a tile of two rows)
    Out(4, "odd-nb", 64, 3, "bias", None, False, False), Out(4, "W4", 224, 1, "brr", "sample", True, True),
    Out(4, "H1", 448, 3, "brr", 6, False, False), Out(4, "D1-W64", 224, 16, "bn", None, True, False),
    Out(4, "odd-nb", 64, 16, "rg", None, False, True), Out(4, "W4", 448, 1, "brr", 6, True, True),
]


def out_id(c):
    return (f"F{c.variant}-{c.geom}-{c.cout}-s{c.slices}-{c.epi}" + (f"-rv{c.rv}" if c.rv else "") + ("-gn" if c.gn else "")
            + ("-view" if c.view else ""))


# part 6: the split-K reduce pair.  vol: (nb, D, H, W) of a 3x3x3 stride-1 conv; tile 0 = the default sliced tile (cout % 224 ==
# 0), 6 / 7 explicit; slices "max" = the most the K loop allows (27 ceil(cin / 16) chunks, at most 64); pair: out_format = 2.
Red = namedtuple("Red", "vol cin cout tile slices epi rv view gn pair")
V750, V210, V160 = (3, 10, 5, 5), (2, 3, 5, 7), (2, 4, 4, 5)
REDS = [
    Red(V750, 24, 224, 0, 2, "brr", "sample", True, False, False), Red(V210, 40, 68, 7, 5, "bias", None, False, False, False),
    Red(V750, 40, 132, 6, "max", "rg", None, True, False, False), Red(V210, 24, 224, 0, "max", "bn", None, False, False, False),
    Red(V210, 40, 132, 6, 2, "brr", 6, True, False, False), Red(V160, 24, 224, 0, 5, "brr", "sample", True, True, False),
    Red(V160, 40, 68, 7, 2, "bias", None, False, True, False), Red(V750, 24, 72, 7, 5, "bias", None, False, False, True),
    Red(V160, 24, 72, 7, "max", "brr", 6, True, True, True),
]


def red_slices(c):
    return min(27 * ((c.cin + 15) // 16), 64) if c.slices == "max" else c.slices


def red_id(c):
    return ("x".join(map(str, c.vol)) + f"-{c.cin}-{c.cout}-t{c.tile}-s{c.slices}-{c.epi}" + (f"-rv{c.rv}" if c.rv else "")
            + ("-gn" if c.gn else "") + ("-pair" if c.pair else "") + ("-view" if c.view else ""))


def epilogue_terms(epi, rv, m, rps, cout, seed):
    """the unit-scale epilogue terms of a case, contiguous fp32 CPU tensors (the GPU file copies them into its views)"""
    rv_rows = rps if rv == "sample" else (rv or 1)
    bias = rand(cout, seed=seed + 1) if epi in ("bias", "brr", "bn") else None
    scale = rand(cout, seed=seed + 2) * 0.2 + 1.0 if epi == "bn" else None
    shift = rand(cout, seed=seed + 3) * 0.1 + 0.5 if epi == "bn" else None
    rvt = rand(-(-m // rv_rows), cout, seed=seed + 4) if epi == "brr" else None
    res = rand(m, cout, seed=seed + 5) if epi in ("brr", "rg") else None
    act = {"bn": ACT_SILU, "rg": ACT_GELU}.get(epi, ACT_NONE)
    return Epi(bias, scale, shift, rvt, rv_rows, act, res)


def out_case(c):
    """part 3's inputs of a case: the synthetic workspace [S, P, Mt, cout] (random, seeded), nsl, the epilogue terms"""
    vol = GEOM[c.variant][c.geom]
    m, p = rows_of(vol), c.variant + 2
    seed = 7000 + 16 * OUTS.index(c)
    ws = rand(c.slices, p, m // c.variant, c.cout, seed=seed)
    nsl = torch.full((p, c.cout), c.slices, dtype=torch.int64)
    return ws, nsl, epilogue_terms(c.epi, c.rv, m, m // vol[0], c.cout, seed)


def red_case(c, ws=None):
    """part 6's epilogue terms (and, for the CPU file, a synthetic workspace in place of the partial tiles a launch leaves)"""
    m, s = rows_of(c.vol), red_slices(c)
    seed = 9000 + 16 * REDS.index(c)
    if ws is None:
        ws = rand(s, 1, m, c.cout, seed=seed) * s ** -0.5
    nsl = torch.full((1, c.cout), s, dtype=torch.int64)
    return ws, nsl, epilogue_terms(c.epi, c.rv, m, m // c.vol[0], c.cout, seed)


def tail_nsl(variant, cout, slices, units_main):
    """slices per (position, column) under the tail plan: one for the (position, 224-column tile) units before units_main"""
    tiles_n = cout // 224
    unit = torch.arange(variant + 2)[:, None] * tiles_n + (torch.arange(cout) // 224)[None, :]
    return torch.where(unit >= units_main, slices, 1)


def rms_rowcol(out, ref):
    """worst row and worst column error of out against ref, each relative to the RMS row / column norm of the WHOLE reference
    (not to its own norm: a row that is mostly padding neither inflates nor excuses anything)"""
    d = out.double() - ref
    return (float(d.norm(dim=1).max() / ref.norm(dim=1).pow(2).mean().sqrt()),
            float(d.norm(dim=0).max() / ref.norm(dim=0).pow(2).mean().sqrt()))
