"""The folded Upsample conv (cs_conv_gemm_up2, cs_gemm.hip) for test_up2_variants_cpu.py / test_up2_variants_gpu.py: the case
table, a restatement of the fold in torch, its mutants, and the descriptor both files build.

The fold.  Nearest x2 upsampling of a dim followed by a three-tap conv with pad 1: output 2 s + p reads upsampled positions
2 s + p - 1 .. 2 s + p + 1, i.e. source positions {s - 1, s, s} (p = 0) or {s, s, s + 1} (p = 1) -- per output parity p TWO source
taps, weights [w0, w1 + w2] at offsets {-1, 0} (low pad 1) resp. [w0 + w1, w2] at {0, +1} (low pad 0): extent 2, low pad 1 - p.
A dim that is not doubled keeps its three taps and pad 1.  The op is one conv per parity class on the SOURCE grid, class index
(pd * nh + ph) * nw + pw over the doubled dims, whose outputs interleave: class (pd, ph, pw) owns the output voxels
(2 d + pd, 2 h + ph, 2 w + pw).  fold_upsample_kernel sums the source taps of a folded tap in x, y, z ascending order from 0.f.

The routes of cs_conv_gemm_up2 and how a row of the table asserts the one it ran: the test hands the call a workspace of
cs_conv_gemm_up2_ws_bytes plus a band, filled with a sentinel; the prefix the call wrote names the route --
  nothing                                   scattered store: one launch over all classes ("batch") / one per class ("perclass");
                                            told apart only by CsDebug.no_up2_batch
  ncls m1 cout (+ s m1 cout) words          per-class GEMMs into scratch + up2_interleave_kernel ("scratch"); s > 1: each class
                                            K-sliced by plan_splitk, the partial tiles behind the class results
  ncls S m1 cout words, S >= 2              all classes x S K slices in one launch + up2_reduce_scatter_kernel ("sliced")
Each row states the route and the slice count it expects on the MI355X (256 CUs)."""
import ctypes as C
from collections import namedtuple

import torch
import torch.nn.functional as F

X_SCALE = 0.5          # test_gemm_variants_gpu.py's: activations at half scale against unit bias
PATTERNS = [(ud, uh, uw) for ud in (0, 1) for uh in (0, 1) for uw in (0, 1) if ud | uh | uw]
SLAB_PATTERNS = ((0, 1, 1), (1, 1, 1))          # kh' = kw' = 2: the four-tap slab kernel's
MUTANTS = ("pads_swapped", "tap_dropped", "hw_swapped", "class_order")


# ---- the fold, restated ----------------------------------------------------------------------------------------------------
def src_taps(u, p, k, mutant=None):
    """the taps of the three a folded tap k sums at output parity p (u = 0: the dim is not doubled, tap k itself)"""
    if not u:
        return [k]
    t = ([0], [1, 2])[k] if p == 0 else ([0, 1], [2])[k]
    if mutant == "tap_dropped" and len(t) == 2:
        t = t[:1]
    return t


def classes(up, mutant=None):
    """[(pd, ph, pw)] in class order: index (pd * nh + ph) * nw + pw (mutant class_order: pw-major, (pw * nh + ph) * nd + pd)"""
    nd, nh, nw = (2 if u else 1 for u in up)
    if mutant == "class_order":
        return [(pd, ph, pw) for pw in range(nw) for ph in range(nh) for pd in range(nd)]
    return [(pd, ph, pw) for pd in range(nd) for ph in range(nh) for pw in range(nw)]


def fold(w, up, mutant=None):
    """w [cout, cin, 3, 3, 3] -> [ncls][cout, cin, kd', kh', kw'] in w's dtype: every folded tap the sum of its source taps in
    x, then y, then z ascending order, starting from zero (fp32: the kernel's adds, bit for bit)"""
    ext = [2 if u else 3 for u in up]
    out = []
    for par in classes(up, mutant):
        wf = torch.zeros(*w.shape[:2], *ext, dtype=w.dtype)
        for a in range(ext[0]):
            for b in range(ext[1]):
                for c in range(ext[2]):
                    acc = torch.zeros(w.shape[:2], dtype=w.dtype)
                    for x in src_taps(up[0], par[0], a, mutant):
                        for y in src_taps(up[1], par[1], b, mutant):
                            for z in src_taps(up[2], par[2], c, mutant):
                                acc = acc + w[:, :, x, y, z]
                    wf[:, :, a, b, c] = acc
        out.append(wf)
    return out


def class_conv(x, wc, up, par, mutant=None):
    """one parity class on the source grid: x [nb, d, h, w, cin], extent 2 and low pad 1 - parity on the doubled dims (mutant
    pads_swapped: low pad = parity), extent 3 and pad 1 elsewhere; taps past the input read zero, the output keeps x's extents"""
    pads = []
    for u, p in zip(up, par):
        lo = 1 if not u else (p if mutant == "pads_swapped" else 1 - p)
        pads.append((lo, (2 if u else 3) - 1 - lo))
    xn = F.pad(x.permute(0, 4, 1, 2, 3), (*pads[2], *pads[1], *pads[0]))
    return F.conv3d(xn, wc).permute(0, 2, 3, 4, 1)


def folded_conv(x, w, up, mutant=None):
    """nearest x2 of the flagged dims + 3x3x3 conv, evaluated as the interleaved class convs (no bias, no activation)"""
    nb, d, h, wd, _ = x.shape
    out = torch.zeros(nb, d << up[0], h << up[1], wd << up[2], w.shape[0], dtype=x.dtype)
    true_order = classes(up)
    wf = fold(w, up, mutant)
    for i, par in enumerate(classes(up, mutant)):
        # (class_order: the class that sits at the kernel's index i gets the weights the mutated order put at i)
        own = true_order[i] if mutant == "class_order" else par
        y = class_conv(x, wf[i], up, own, mutant)
        pd, ph, pw = own
        if mutant == "hw_swapped":
            ph, pw = (pw if up[1] else 0), (ph if up[2] else 0)
        out[:, pd::1 << up[0], ph::1 << up[1], pw::1 << up[2]] = y
    return out


def mutant_applies(m, up):
    """a mutant the pattern turns into the restatement itself is not applied: H / W swap needs both doubled, the class order at
    least two doubled dims"""
    if m == "hw_swapped":
        return bool(up[1] and up[2])
    if m == "class_order":
        return sum(up) >= 2
    return True


def fold_gate(x, w, up):
    """per element: both evaluations are fp64 sums of the same cin * 27 products (the fold pre-sums two or four weights), so each
    is within (K + 2) 2^-53 of sum |x| |w| over its terms; twice that, and a factor two of slack"""
    from oracle import ref_ops as R
    K = w.shape[1] * 27
    return 4.0 * (K + 2) * 2.0 ** -53 * R.conv_ndhwc(x.abs(), w.abs(), None, (1, 1, 1), up)


def differs(out, ref, gate):
    """the comparison helper: True where `out` is NOT the op `ref` evaluates (any element beyond its gate, or not finite)"""
    return bool((~torch.isfinite(out)).any() or ((out - ref).abs() > gate).any())


# ---- the table -------------------------------------------------------------------------------------------------------------
# route: what the footprint must show (module docstring).  vol = (nb, d, h, w) of the SOURCE grid.  math f16x3 | fp32.
# fmt = CsConvGemm.a_format (1: the GroupNorm + SiLU producer's fp16 hi / lo images at ops.A_SCALE).  sw: CsDebug switches of the
# launch.  slices: sliced -> S, scratch -> s of plan_splitk (0: unsliced).  gn: GroupNorm partials asked (and granted).
# piece: the row family of the issue (a small ragged scratch, b non-slab patterns, c sliced, d one-launch batch, e per class,
# f pre-split).  view: operands as views between guard bands (every second row).
Row = namedtuple("Row", "piece route up vol cin cout math fmt bias act sw slices gn view")

G315, G210 = (3, 3, 5, 7), (2, 3, 5, 7)


def _rows():
    r = []
    add = lambda piece, route, up, vol, cin, cout, math="f16x3", fmt=0, bias=True, act="none", sw=(), slices=0, gn=False: \
        r.append(Row(piece, route, up, vol, cin, cout, math, fmt, bias, act, tuple(sw), slices, gn, len(r) % 2 == 1))
    # a. 315 source rows: 64- / 128-row tiles span the three samples, the last tile is partly filled; ragged column tiles
    add("a", "scratch", (0, 1, 1), G315, 20, 236, act="silu")
    add("a", "scratch", (0, 1, 1), G315, 20, 236, math="fp32", bias=False)
    add("a", "scratch", (1, 1, 1), G315, 20, 132, bias=False, act="silu", sw=("no_slab4",))
    add("a", "scratch", (1, 1, 1), G315, 20, 132, math="fp32")
    add("a", "scratch", (0, 1, 1), G315, 20, 132, sw=("no_slab4",))
    add("a", "scratch", (1, 1, 1), G315, 20, 236, math="fp32", act="silu")
    add("a", "scratch", (1, 1, 1), G315, 20, 236, bias=False)
    add("a", "scratch", (0, 1, 1), G315, 20, 132, math="fp32", bias=False, act="silu")
    # b. the five patterns with a three-tap H or W: never on the slab kernel
    for i, up in enumerate(p for p in PATTERNS if p not in SLAB_PATTERNS):
        add("b", "scratch", up, G210, 12, 36, act="silu" if i % 2 else "none", bias=i % 3 != 0)
        add("b", "scratch", up, G210, 12, 36, math="fp32", act="none" if i % 2 else "silu", bias=i % 3 != 1)
    # c. all classes x S slices in one launch; S = 2 / 9 / 10 / 17: a partial first group of eight of the reduce's loop, a first
    # group exactly full (1 + 8), one slice into the second, a third group.  up2_sliced_plan at 256 CUs: S' = min(256 / tiles,
    # 32, nsc / 2) with nsc = kd' ceil(cin / 16) super-chunks, then the fewest slices of ceil(nsc / S') super-chunks --
    #   8 classes x 1 row tile, nsc = 4:  S' = 2                       -> 2
    #   4 classes x 2 row tiles, nsc = 18: S' = 9, 2 per slice          -> 9
    #   8 classes x 1 row tile, nsc = 20: S' = 10, 2 per slice          -> 10
    #   4 classes x 3 row tiles, nsc = 51: S' = 21, 3 per slice         -> 17
    add("c", "sliced", (1, 1, 1), G210, 20, 128, slices=2, act="silu")
    add("c", "sliced", (0, 1, 1), G315, 96, 224, slices=9)
    add("c", "sliced", (1, 1, 1), G210, 148, 128, slices=10, bias=False)
    add("c", "sliced", (0, 1, 1), (2, 7, 7, 7), 272, 224, slices=17, act="silu")
    # ... and row c's second case per class: plan_splitk cuts each class's 72 K chunks into 8 (a power of two, >= 8 chunks
    # each, 3 tiles x 8 <= 512), the partial tiles behind the four class results
    add("c", "scratch", (0, 1, 1), G315, 96, 224, sw=("no_up2_batch",), slices=8)
    # d. one launch over all classes, scattered store: 4 x 35 and 8 x 16 row tiles (>= 128: `fills`), the last one ragged
    add("d", "batch", (0, 1, 1), (5, 9, 13, 15), 20, 224, act="silu")
    add("d", "batch", (1, 1, 1), (3, 11, 9, 13), 20, 128)
    # ... with GroupNorm partials: 256 source rows per sample, so whole tiles (the one row without a ragged last row tile)
    add("d", "batch", (1, 1, 1), (16, 4, 8, 8), 20, 128, gn=True)
    # e. one scattered-store launch per class: 201 row tiles of 256 (>= 192: the class alone takes the 256-row tile)
    add("e", "perclass", (0, 1, 1), (3, 19, 29, 31), 20, 224, sw=("no_up2_batch",))
    # f. pre-split operand: the slab kernel reads fp32 only, so these run per class on the per-tap gather into scratch -- at row
    # a's grid and at the first sliced row's (no route refuses the form; none of the one-launch routes takes it)
    add("f", "scratch", (0, 1, 1), G315, 24, 236, fmt=1, act="silu")
    add("f", "scratch", (1, 1, 1), G210, 24, 128, fmt=1)
    return r


ROWS = _rows()


def row_id(r):
    s = f"{r.piece}-{r.route}" + (f"{r.slices}" if r.slices else "") + "-" + "".join(str(u) for u in r.up)
    s += "-" + "x".join(str(v) for v in r.vol) + f"-{r.cin}-{r.cout}-{r.math}" + (f"-f{r.fmt}" if r.fmt else "")
    s += ("-bias" if r.bias else "") + (f"-{r.act}" if r.act != "none" else "") + "".join(f"-{k}" for k in r.sw)
    return s + ("-gn" if r.gn else "") + ("-view" if r.view else "")


def ncls(r):
    return 1 << sum(r.up)


def m1(r):
    return r.vol[0] * r.vol[1] * r.vol[2] * r.vol[3]


def out_vol(r):
    return (r.vol[0], r.vol[1] << r.up[0], r.vol[2] << r.up[1], r.vol[3] << r.up[2])


def k_exec(r):
    """executed terms per output: cin * kd' * kh' * kw'"""
    k = r.cin
    for u in r.up:
        k *= 2 if u else 3
    return k


def prefix_words(r):
    """words of the workspace the row's route writes, from its first word on"""
    if r.route == "scratch":
        return (ncls(r) + (r.slices if r.slices > 1 else 0)) * m1(r) * r.cout
    if r.route == "sliced":
        return ncls(r) * r.slices * m1(r) * r.cout
    return 0


def descriptor(L, r, lda=None, ldo=None, ldw=None):
    """the CsConvGemm of a row, no pointers: what the host rules look at (the GPU file adds operands, status and scales)"""
    p = L.CsConvGemm()
    p.nb, p.din, p.hin, p.win = r.vol
    _, p.dout, p.hout, p.wout = out_vol(r)
    p.cin, p.cout = r.cin, r.cout
    p.lda, p.ldo, p.ldw = lda or r.cin, ldo or r.cout, ldw or r.cout
    p.kd = p.kh = p.kw = 3
    p.sd = p.sh = p.sw = 1
    p.pd = p.ph = p.pw = 1
    p.ud, p.uh, p.uw = r.up
    p.math = L.MATH_F16X3 if r.math == "f16x3" else L.MATH_FP32
    p.act = L.ACT_SILU if r.act == "silu" else L.ACT_NONE
    p.rv_rows, p.a_format = 1, r.fmt
    if r.math == "f16x3":
        p.a_scale = 16.0
    return p


def up2_info(L, up):
    """(rc, ncls, kd', kh', kw') of cs_conv_up2_info"""
    v = [C.c_int32(-1) for _ in range(4)]
    rc = L.load().cs_conv_up2_info(*up, *(C.byref(x) for x in v))
    return (rc,) + tuple(x.value for x in v)
