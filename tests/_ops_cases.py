"""The case table, inputs, CPU oracles, fp32 emulations, mutants and gates of the small-op variant suite: every extern "C" entry
of commonscenes_amd/csrc/cs_ops.hip at the smallest shapes that reach its edges -- a tail workgroup, a row stride wider than the
row, the second pass of a grid-stride loop under the launch's block cap.  test_ops_variants_cpu.py proves the gates here are
neither vacuous nor tighter than fp32; test_ops_variants_gpu.py runs the kernels through them.  Nothing here imports
commonscenes_amd.

Gates.  `exact`: the bits of the output equal the oracle's (data movement, fp32 operation sequences the source pins down).
`E`: |out - fp64| <= E elementwise with E = k 2^-24 S, S the sum of the magnitudes of the expression's terms and k the number of
roundings on its longest path, counted from the source (ddim / plms: K_DDIM, K_PLMS below) or, for the three ops whose error is
the device library's erff / expf / sinf / cosf / logf, set from the fp32 evaluation of the same expression by torch on the CPU:
four times its worst ratio over the case inputs, rounded up to a power of two (K_GEGLU, K_TSEMB, K_LSM; the measured ratios
stand beside them).  `norm`: N <= out <= N (1 + 2^-22) with N the fp64 row norm -- one rounding and at most one bump up; where N is an fp32 number
whose square is the sum of squares exactly (the 3, 4 rows: 5; a single entry) the band would let a bump that was not due pass
(one ulp of 5 is 0.8 of it), so there the gate is `exact`.
`vq`: the indices equal the fp64 argmin except on at most 2 provable fp32 near-ties per case (the bound of conftest.vq_flip_
report at equal latents: 8 eps32 (|z|^2 + |e|^2)); rows that equal a duplicated code are exact (first index).

Shapes.  One sweep of a capped grid is 256 threads x the cap: 256 * 8192 work items under cs_grid_for(.., 256 * 32), 256 * 4096
under the default cap, 256 * 1024 rows for the VQ lookup, 256 * 256 threads for absmax.  The layout kernels' wrap case is one sweep
and three elements (256 * 8192 + 3 = 5 * 419431); 256 such sweeps (2 GiB per tensor) run as an identity copy in the GPU test
alone.  log_softmax carries a row of +-80 and a row of +-100: exp(80) = 5.5e34 is still an fp32 number, exp(100) is not, so the
second row is the one on which the max subtraction decides between a finite result and inf.

A mutant returns None where the case's shape turns it into a no-op."""
import math
import zlib
from dataclasses import dataclass
from functools import lru_cache

import numpy as np
import torch

U = 2.0 ** -24
NAN = float("nan")
INF = float("inf")
SWEEP32 = 256 * 256 * 32        # work items of one sweep of a grid capped at 256 * 32 workgroups (cs_grid_for(.., 256 * 32))
SWEEP16 = 256 * 256 * 16        # the default cap
SWEEP_VQ = 256 * 1024
SWEEP_ABSMAX = 256 * 256

# k of the transcendental ops: 4 x (worst |torch CPU fp32 - fp64| / (2^-24 S) over the table's inputs), rounded up to a power of 2.
# Measured ratios: geglu 2.04, timestep_embedding 7.40, log_softmax 1.51 (test_ops_variants_cpu.py prints them).
K_GEGLU = 16
K_TSEMB = 32
K_LSM = 8

# roundings on the longest path, -ffp-contract=off.  e = eu + s (ec - eu): sub, mul, add = 3 (0 without cfg).
# p0 = (x - c e) / sa: mul, sub, div = 3 more.  xp = sp p0 + dc e [+ sigma noise]: mul, add [, add] = 2 [3] more.
K_CFG = 3
K_DDIM = {"p0": 3, "xp": 5, "xp_noise": 6}
# the multistep forms (plms.py:221-230) between e and p0: AB2 (3e - h1) / 2: mul, sub, div; AB3: mul, sub, add, div;
# AB4: mul, sub, add, sub, div; the Euler average (h1 + e) / 2: add, div
K_PLMS = {0: 0, 1: 3, 2: 4, 3: 5, 4: 2}
PLMS_COEF = {0: ((1.0,), 1.0), 1: ((3.0, -1.0), 2.0), 2: ((23.0, -16.0, 5.0), 12.0), 3: ((55.0, -59.0, 37.0, -9.0), 24.0),
             4: ((1.0, 1.0), 2.0)}
PLMS_NEED = {0: 0, 1: 1, 2: 2, 3: 3, 4: 1}

A_T, A_PREV, SIGMA, CFG_SCALE = 0.512, 0.624, 0.1, 3.0

MUTANTS = ("drop_tail", "c_for_ld", "sweep_untouched", "sweep_twice", "row_mod", "uncond_both", "tapsum_mask", "lsm_nomax",
           "rowstats_nearest", "rowstats_always_bump", "fold_overwrite", "csr_order", "vq_last", "nan_dropped")


@dataclass(frozen=True)
class Case:
    op: str
    name: str
    entries: tuple
    p: tuple

    def __getitem__(self, k):
        return dict(self.p)[k]

    def get(self, k, d=None):
        return dict(self.p).get(k, d)


def _c(op, name, entries, **p):
    return Case(op, name, tuple(entries), tuple(sorted(p.items())))


def case_id(c):
    return f"{c.op}-{c.name}"


def _gen(c, salt=0):
    return torch.Generator().manual_seed(zlib.crc32(case_id(c).encode()) + salt)


def _randn(c, *shape, salt=0):
    return torch.randn(*shape, generator=_gen(c, salt), dtype=torch.float32)


# ---- views and visits ----------------------------------------------------------------------------------------------------
def misread(t, ld):
    """what a kernel reads of the [m, c] view with row stride ld (NaN in the gaps) when it steps rows by c"""
    m, c = t.shape
    flat = torch.full((m * ld + c,), NAN, dtype=t.dtype)
    torch.as_strided(flat, (m, c), (ld, 1)).copy_(t)
    return torch.as_strided(flat, (m, c), (c, 1)).clone()


def miswrite(v, ld):
    """what lands in the [m, c] view with row stride ld (NaN = untouched) when a kernel steps its output rows by c"""
    m, c = v.shape
    flat = torch.full((m * ld + c,), NAN, dtype=v.dtype)
    torch.as_strided(flat, (m, c), (c, 1)).copy_(v)
    return torch.as_strided(flat, (m, c), (ld, 1)).clone()


def visited(total, mutant, sweep, block=256):
    """mask of the work items a mutant still processes; None where that is all of them"""
    if mutant == "drop_tail":
        keep = (total // block) * block
    elif mutant in ("sweep_untouched", "sweep_twice"):
        keep = sweep
    else:
        return None
    if keep >= total:
        return None
    return torch.arange(total) < keep


def _units(mask, m, c4n):
    return mask.view(m, c4n).repeat_interleave(4, dim=1)


# ---- the table -----------------------------------------------------------------------------------------------------------
WRAP_ROWS = SWEEP32 + 5          # rows of 4 floats: m h / 4 = 256 * 8192 + 5 units


def _build_cases():
    C = []
    for m, h, px, po, nm in ((1, 4, 0, 0, "1x4"), (3, 12, 8, 4, "3x12-view"), (77, 448, 0, 0, "77x448"), (WRAP_ROWS, 4, 0, 0, "wrap")):
        C.append(_c("geglu", nm, ["cs_geglu"], m=m, h=h, ldx=2 * h + px, ldo=h + po))
    for m, c, nm in ((1, 4, "1x4-view"), (3, 12, "3x12-view"), (77, 448, "77x448-view"), (WRAP_ROWS, 4, "wrap")):
        v = 0 if nm == "wrap" else 1
        C.append(_c("copy_rows", nm, ["cs_copy_rows"], m=m, c=c, lds=c + 8 * v, ldd=c + 4 * v))
        C.append(_c("add_rowvec", nm, ["cs_add_rowvec"], m=m, c=c, ldx=c + 4 * v, ldv=c + 8 * v, rows={1: 1, 3: 2, 77: 11}.get(m, 1000)))
    C.append(_c("add_rowvec", "50x8-rows7-view", ["cs_add_rowvec"], m=50, c=8, ldx=12, ldv=16, rows=7))
    for nb, rows, ca, cb, v, share, nm in ((1, 1, 4, 4, 1, 1, "1x4-view"), (2, 3, 12, 4, 1, 1, "3x12-view"), (2, 77, 448, 12, 1, 1, "77x448-view"),
                                           (4, 5, 8, 12, 1, 2, "shared-b-view"), (1, WRAP_ROWS, 4, 4, 0, 1, "wrap")):
        C.append(_c("concat", nm, ["cs_copy_rows"], nb=nb, rows=rows, ca=ca, cb=cb, lda=ca + 4 * v, ldb=cb + 8 * v, share=share))
    for c in (1, 3, 5):
        for pad in (0, 3):
            C.append(_c("to_ndhwc", f"c{c}-cpad{c + pad}", ["cs_nchw_to_ndhwc"], nb=2, c=c, sp=(7, 5, 3), cpad=c + pad))
            C.append(_c("to_nchw", f"c{c}-ld{c + pad}", ["cs_ndhwc_to_nchw"], nb=2, c=c, sp=(7, 5, 3), ldx=c + pad))
    # 256 * 8192 + 3 = 5 * 419431 elements: one sweep of the capped grid and three elements of the second
    C.append(_c("to_ndhwc", "wrap", ["cs_nchw_to_ndhwc"], nb=1, c=5, sp=(419431, 1, 1), cpad=5))
    C.append(_c("to_nchw", "wrap", ["cs_ndhwc_to_nchw"], nb=1, c=5, sp=(419431, 1, 1), ldx=5))
    for dim in (2, 3, 33, 224):
        for mp in (10000.0, 100.0):
            C.append(_c("ts_embedding", f"dim{dim}-p{int(mp)}", ["cs_timestep_embedding"], dim=dim, mp=mp))
    # n = nb * per: 1, 255 = 5 * 51, 257, the default-cap wrap 256 * 4096 + 77 as one sample, and 7 * 149807 = 256 * 4096 + 73
    # (256 * 4096 + 77 = 27 * 38839 has no factor 7: the nearest odd per above one sweep)
    for nb, per, nm in ((1, 1, "n1"), (5, 51, "n255"), (1, 257, "n257"), (1, SWEEP16 + 77, "wrap-nb1"), (7, 149807, "wrap-nb7")):
        for cfg, noise in ((1, 1), (0, 0), (1, 0)):
            C.append(_c("ddim", f"{nm}-cfg{cfg}-noise{noise}", ["cs_ddim_cfg_update", "cs_ddim_cfg_update_dev", "cs_ddim_coefficients"],
                        nb=nb, per=per, cfg=cfg, noise=noise))
        for mode in range(5):
            C.append(_c("plms", f"{nm}-mode{mode}-cfg{(mode + nb) % 2}", ["cs_plms_update"], nb=nb, per=per, cfg=(mode + nb) % 2, mode=mode))
    for m, ncode, edim, ldz, dup in ((1, 1, 1, 1, 0), (300, 7, 1, 4, 1), (300, 4097, 2, 2, 1), (1, 8192, 2, 4, 0), (SWEEP_VQ + 3, 7, 3, 3, 1),
                                     (300, 4097, 3, 4, 1), (300, 8192, 3, 4, 0), (300, 1, 3, 3, 0), (300, 7, 2, 4, 0), (300, 7, 1, 1, 1)):
        C.append(_c("vq", f"m{m}-n{ncode}-e{edim}-ld{ldz}" + ("-dup" if dup else ""), ["cs_vq_argmin_lookup"], m=m, ncode=ncode, edim=edim,
                    ldz=ldz, dup=dup))
    for n_obj, n_tri, h, pad, kind in ((1, 1, 1, 0, "self"), (1, 65, 33, 3, "self"), (5, 63, 33, 0, "hub"), (5, 64, 1, 3, "hub"),
                                       (6, 65, 33, 0, "rand"), (7, 128, 33, 3, "rand"), (9, 129, 1, 0, "rand"), (4, 129, 33, 3, "hub")):
        C.append(_c("gcn", f"o{n_obj}-t{n_tri}-h{h}-{kind}" + ("-view" if pad else ""),
                    ["cs_gcn_gather_cat", "cs_gcn_segment_mean", "cs_gcn_csr_ints", "cs_gcn_csr_build", "cs_gcn_segment_mean_csr"],
                    n_obj=n_obj, n_tri=n_tri, h=h, pad=pad, kind=kind))
    for dim, n, pad, nm in ((1, 1, 0, "d1-n1"), (33, 7, 0, "d33-n7"), (33, 300, 7, "d33-n300-view"), (1, 300, 3, "d1-n300-view"),
                            (33, 31776, 0, "wrap")):        # 31776 * 33 = 256 * 4096 + 32 elements
        C.append(_c("embedding", nm, ["cs_embedding"], n_rows=10, dim=dim, n=n, ldo=dim + pad))
    for i, (cc, m) in enumerate((cc, m) for cc in (1, 24, 63, 64, 65, 130) for m in (1, 4, 5)):
        C.append(_c("log_softmax", f"{m}x{cc}" + ("-view" if i % 2 else ""), ["cs_log_softmax"], m=m, c=cc, pad=5 * (i % 2)))
    for mats, kind in ((((1, 1),), "last"), (((3, 63),), "last"), (((4, 64),), "last"), (((5, 65),), "last"), (((1, 200),), "last"),
                       (((3, 1),), "last"), (((4, 65),), "last"), (((5, 200),), "last"), (((5, 64),), "last"), (((4, 63),), "last"),
                       (((3, 64), (5, 65)), "last"), (((4, 200), (1, 63), (5, 1)), "last"), (((3, 65),), "squares"),
                       (((1, 64), (4, 2)), "squares"), (((5, 65), (3, 64)), "first"), (((4, 63), (5, 200), (1, 1)), "first"),
                       (((3, 65), (4, 64)), "squares-first")):
        C.append(_c("rowstats", "+".join(f"{r}x{cl}" for r, cl in mats) + f"-{kind}", ["cs_weight_rowstats"], mats=mats, kind=kind))
    big = SWEEP_ABSMAX * 8 + 3
    for n, kind in ((1, "last"), (big, "last"), (big, "idx65537"), (big, "neg"), (1000, "zeros"), (big, "fold"), (big, "inf"), (1, "nan"),
                    (big, "nan"), (big, "nan-idx65537")):
        C.append(_c("absmax", f"n{n}-{kind}", ["cs_absmax"], n=n, kind=kind))
    i = 0
    for vol in ((1, 1, 1), (1, 1, 5), (3, 1, 1), (2, 3, 4)):
        for ints in (1, 0):
            C.append(_c("tapsum27", f"{'x'.join(map(str, vol))}-nb{1 + i % 2}-co{(1, 4)[(i // 2 + ints) % 2]}-{'int' if ints else 'f32'}"
                        + ("-view" if i % 3 else ""), ["cs_tapsum27"], nb=1 + i % 2, vol=vol, cout=(1, 4)[(i // 2 + ints) % 2],
                        ypad=5 * (i % 3 != 0), opad=3 * (i % 3 != 0) + 1, bias=(i + 1) % 2 if i < 6 else i % 2, ints=ints, axis=i % 3))
            i += 1
    for cout, cin, ncolp, scale in ((1, 3, 28, 1.0), (1, 16, 84, 0.125), (3, 20, 84, 1.0), (3, 3, 84, 0.125), (1, 20, 28, 0.125),
                                    (3, 16, 84, 1.0)):
        C.append(_c("pack_tapcol", f"co{cout}-ci{cin}-n{ncolp}-s{scale:g}", ["cs_pack_weight_f16x3_tapcol"], cout=cout, cin=cin,
                    ncolp=ncolp, scale=scale))
    for b, n, m in ((1, 1, 1), (2, 300, 1030), (1, 257, 1024)):
        C.append(_c("chamfer", f"b{b}-n{n}-m{m}", ["cs_chamfer_nm_distance"], b=b, n=n, m=m))
    for n, nm in ((1, "n1"), (333, "n333"), (SWEEP32 + 3, "wrap")):
        C.append(_c("synth_fill", nm, ["cs_synth_fill"], n=n, base=0x1234567 + n, scale=0.75, offset=-0.25))
    return C


CASES = _build_cases()
BY_OP = {}
for _x in CASES:
    BY_OP.setdefault(_x.op, []).append(_x)


# ---- per-op inputs, oracle, emulation ------------------------------------------------------------------------------------
# data(c) -> dict of CPU tensors;  reference(c) -> list of (name, kind, ref, E);  emulate(c, mutant) -> list of tensors | None
def _geglu32(x, h):
    a, g = x[:, :h], x[:, h:]
    return a * ((0.5 * g) * (1.0 + torch.erf(g * 0.70710678118654752440)))


def _d_geglu(c):
    x = _randn(c, c["m"], 2 * c["h"])
    x[:, c["h"]:] *= 2.0
    return {"x": x}


def _r_geglu(c, d):
    h = c["h"]
    a, g = d["x"][:, :h].double(), d["x"][:, h:].double()
    return [("out", "E", a * (0.5 * g * (1.0 + torch.erf(g / math.sqrt(2.0)))), K_GEGLU * U * a.abs() * (g.abs() + 1.0))]


def _e_geglu(c, d, mut):
    m, h = c["m"], c["h"]
    x = d["x"]
    if mut == "c_for_ld":
        x = misread(x, c["ldx"])
    out = _geglu32(x, h)
    mask = visited(m * h // 4, mut, SWEEP32)
    if mut in ("drop_tail", "sweep_untouched"):
        if mask is None:
            return None
        out[~_units(mask, m, h // 4)] = NAN
    return [out]


def _m_geglu(c):
    return ["drop_tail"] + ["c_for_ld"] * (c["ldx"] > 2 * c["h"]) + ["sweep_untouched"] * (c["m"] * c["h"] // 4 > SWEEP32)


def _copy_emu(src, lds, ldd, mut):
    m, c = src.shape
    s = misread(src, lds) if (mut == "c_for_ld" and lds > c) else src
    out = s.clone()
    mask = visited(m * c // 4, mut, SWEEP32)
    if mask is not None:
        out[~_units(mask, m, c // 4)] = NAN
    if mut == "c_for_ld" and ldd > c:
        out = miswrite(out, ldd)
    return out


def _d_copy(c):
    return {"src": _randn(c, c["m"], c["c"])}


def _r_copy(c, d):
    return [("dst", "exact", d["src"], None)]


def _e_copy(c, d, mut):
    if mut in ("drop_tail", "sweep_untouched") and visited(c["m"] * c["c"] // 4, mut, SWEEP32) is None:
        return None
    return [_copy_emu(d["src"], c["lds"], c["ldd"], mut)]


def _m_copy(c):
    return ["drop_tail"] + ["c_for_ld"] * (c["lds"] > c["c"] and c["m"] > 1) + ["sweep_untouched"] * (c["m"] * c["c"] // 4 > SWEEP32)


def _d_addrv(c):
    nv = (c["m"] + c["rows"] - 1) // c["rows"]
    return {"x": _randn(c, c["m"], c["c"]), "v": _randn(c, nv, c["c"], salt=1)}


def _r_addrv(c, d):
    g = torch.arange(c["m"]) // c["rows"]
    return [("x", "exact", d["x"] + d["v"][g], None)]


def _e_addrv(c, d, mut):
    m, cc, rows = c["m"], c["c"], c["rows"]
    x, v = d["x"], d["v"]
    if mut == "c_for_ld":
        v = misread(v, c["ldv"])
    row = torch.arange(m)
    g = row % rows if mut == "row_mod" else row // rows
    if int(g.max()) >= v.shape[0]:                      # rows of v that are not there: whatever lies behind it
        v = torch.cat([v, torch.full((int(g.max()) + 1 - v.shape[0], cc), NAN)])
    out = x + v[g]
    mask = visited(m * cc // 4, mut, SWEEP32)
    if mut in ("drop_tail", "sweep_untouched", "sweep_twice"):
        if mask is None:
            return None
        um = ~_units(mask, m, cc // 4)
        out = torch.where(um, x if mut != "sweep_twice" else out + v[g], out)
    return [out]


def _m_addrv(c):
    wrap = c["m"] * c["c"] // 4 > SWEEP32
    return (["drop_tail"] + ["c_for_ld"] * (c["ldv"] > c["c"] and c["m"] > c["rows"]) + ["row_mod"] * (c["m"] > 1)
            + ["sweep_untouched", "sweep_twice"] * wrap)


def _d_concat(c):
    na = c["nb"]
    return {"a": _randn(c, na, c["rows"], c["ca"]), "b": _randn(c, na // c["share"], c["rows"], c["cb"], salt=1)}


def _r_concat(c, d):
    return [("out", "exact", torch.cat([d["a"], d["b"].repeat(c["share"], 1, 1)], dim=-1), None)]


def _e_concat(c, d, mut):
    ca, cb = c["ca"], c["cb"]
    a2, b2 = d["a"].reshape(-1, ca), d["b"].repeat(c["share"], 1, 1).reshape(-1, cb)
    if mut in ("drop_tail", "sweep_untouched") and visited(b2.shape[0] * cb // 4, mut, SWEEP32) is None:
        return None
    ldd = ca + cb
    if mut == "c_for_ld":       # the source strides (the destination's is always wider than either half)
        oa, ob = _copy_emu(a2, c["lda"], ca, mut), _copy_emu(b2, c["ldb"], cb, mut)
    else:
        oa, ob = a2.clone(), _copy_emu(b2, cb, cb, mut)
    return [torch.cat([oa, ob], dim=1).reshape(*d["a"].shape[:-1], ldd)]


def _m_concat(c):
    return ["drop_tail"] + ["c_for_ld"] * (c["lda"] > c["ca"] and c["rows"] * c["nb"] > 1) + \
        ["sweep_untouched"] * (c["nb"] * c["rows"] * c["cb"] // 4 > SWEEP32)


def _s_of(c):
    return c["sp"][0] * c["sp"][1] * c["sp"][2]


def _d_ndhwc(c):
    return {"x": _randn(c, c["nb"], c["c"], _s_of(c))}


def _r_ndhwc(c, d):
    y = torch.zeros(c["nb"], _s_of(c), c["cpad"])
    y[..., :c["c"]] = d["x"].permute(0, 2, 1)
    return [("y", "exact", y, None)]


def _e_ndhwc(c, d, mut):
    y = _r_ndhwc(c, d)[0][2].clone()
    if mut == "c_for_ld":
        flat = torch.full((y.numel(),), NAN)
        flat[:c["nb"] * _s_of(c) * c["c"]] = d["x"].permute(0, 2, 1).reshape(-1)
        return [flat.view_as(y)]
    mask = visited(y.numel(), mut, SWEEP32)
    if mut is not None:
        if mask is None:
            return None
        y.view(-1)[~mask] = NAN
    return [y]


def _m_ndhwc(c):
    tot = c["nb"] * _s_of(c) * c["cpad"]
    return ["drop_tail"] * (tot % 256 != 0) + ["c_for_ld"] * (c["cpad"] > c["c"]) + ["sweep_untouched"] * (tot > SWEEP32)


def _d_nchw(c):
    return {"x": _randn(c, c["nb"], _s_of(c), c["c"])}


def _r_nchw(c, d):
    return [("y", "exact", d["x"].permute(0, 2, 1).clone(memory_format=torch.contiguous_format), None)]


def _e_nchw(c, d, mut):
    x = d["x"]
    if mut == "c_for_ld":
        x = misread(x.reshape(-1, c["c"]), c["ldx"]).view_as(x)
    y = x.permute(0, 2, 1).clone(memory_format=torch.contiguous_format)
    mask = visited(y.numel(), mut, SWEEP32)
    if mut in ("drop_tail", "sweep_untouched"):
        if mask is None:
            return None
        y.view(-1)[~mask] = NAN
    return [y]


def _m_nchw(c):
    tot = c["nb"] * _s_of(c) * c["c"]
    return ["drop_tail"] * (tot % 256 != 0) + ["c_for_ld"] * (c["ldx"] > c["c"]) + ["sweep_untouched"] * (tot > SWEEP32)


TS = (0, 1, 999)


def _d_ts(c):
    return {"t": torch.tensor(TS, dtype=torch.int64)}


def _r_ts(c, d):
    dim, half = c["dim"], c["dim"] // 2
    f = torch.exp(-math.log(c["mp"]) * torch.arange(half, dtype=torch.float64) / half)
    a = d["t"].double()[:, None] * f
    z = torch.zeros(len(TS), dim - 2 * half, dtype=torch.float64)
    s = a.abs() + 1.0
    return [("emb", "E", torch.cat([a.cos(), a.sin(), z], 1), K_TSEMB * U * torch.cat([s, s, torch.ones_like(z)], 1))]


def _e_ts(c, d, mut):
    dim, half = c["dim"], c["dim"] // 2
    f = torch.exp(-math.log(c["mp"]) * torch.arange(half, dtype=torch.float32) / half)
    a = d["t"].float()[:, None] * f
    out = torch.cat([a.cos(), a.sin(), torch.zeros(len(TS), dim - 2 * half)], 1)
    if mut == "drop_tail":
        out.view(-1)[~visited(out.numel(), mut, 0)] = NAN
    return [out]


def _m_ts(c):
    return ["drop_tail"]


def ddim_coefs(sigma, plms=False):
    """the five fp32 step coefficients as cs_ddim_coefficients / cs_plms_update derive them (sqrtf is correctly rounded)"""
    one, at, ap, sg = np.float32(1.0), np.float32(A_T), np.float32(A_PREV), np.float32(0.0 if plms else sigma)
    s1 = np.float32(math.sqrt(1.0 - A_T))
    return np.sqrt(at), np.sqrt(ap), np.sqrt(one - ap - sg * sg), sg, s1


def _d_step(c):
    n = c["nb"] * c["per"]
    d = {"x": _randn(c, n), "eps": _randn(c, (2 if c["cfg"] else 1) * n, salt=1)}
    if c.op == "ddim":
        if c["noise"]:
            d["noise"] = _randn(c, n, salt=2)
    else:
        for j in range(PLMS_NEED[c["mode"]]):
            d[f"h{j + 1}"] = _randn(c, n, salt=3 + j)
    return d


def _step(c, d, dt, x=None, uncond=False):
    """(e, e magnitude, ep, ep magnitude, p0, p0 mag, xp, xp mag) of one update in numpy dtype dt; the magnitudes are fp64 sums"""
    n = c["nb"] * c["per"]
    A = lambda t: t.numpy().astype(dt)
    x = A(d["x"]) if x is None else x.astype(dt)
    plms = c.op == "plms"
    sa, sp, dc, sg, s1 = (dt(v) for v in ddim_coefs(SIGMA if c.get("noise") else 0.0, plms))
    eps = A(d["eps"])
    if c["cfg"]:
        eu, ec = eps[:n], (eps[:n] if uncond else eps[n:])
        e = eu + dt(CFG_SCALE) * (ec - eu)
        em = np.abs(eu).astype(np.float64) + CFG_SCALE * (np.abs(ec).astype(np.float64) + np.abs(eu))
    else:
        e, em = eps, np.abs(eps).astype(np.float64)
    ep, epm = e, em
    if plms and c["mode"]:
        cf, den = PLMS_COEF[c["mode"]]
        hs = [A(d[f"h{j + 1}"]) for j in range(PLMS_NEED[c["mode"]])]
        terms = [hs[0], e] if c["mode"] == 4 else [e] + hs
        ep = (terms[0] if cf[0] == 1.0 else dt(cf[0]) * terms[0])
        epm = abs(cf[0]) * (em if terms[0] is e else np.abs(terms[0]).astype(np.float64))
        for k, t in zip(cf[1:], terms[1:]):
            term = t if abs(k) == 1.0 else dt(abs(k)) * t
            ep = ep + term if k > 0 else ep - term
            epm = epm + abs(k) * (em if t is e else np.abs(t).astype(np.float64))
        ep, epm = ep / dt(den), epm / den
    p0 = (x - s1 * ep) / sa
    p0m = (np.abs(x).astype(np.float64) + float(s1) * epm) / float(sa)
    xp = sp * p0 + dc * ep
    xpm = float(sp) * p0m + float(dc) * epm
    if "noise" in d:
        xp = xp + sg * A(d["noise"])
        xpm = xpm + float(sg) * np.abs(A(d["noise"])).astype(np.float64)
    return e, em, p0, p0m, xp, xpm


def _r_step(c, d):
    e, em, p0, p0m, xp, xpm = _step(c, d, np.float64)
    kc = K_CFG * c["cfg"]
    km = K_PLMS[c["mode"]] if c.op == "plms" else 0
    kx = K_DDIM["xp_noise" if "noise" in d else "xp"]
    T = torch.from_numpy
    out = [("x_prev", "E", T(xp), (kc + km + kx) * U * T(xpm)), ("pred_x0", "E", T(p0), (kc + km + K_DDIM["p0"]) * U * T(p0m))]
    if c.op == "plms":
        out.append(("e_t", "E", T(e), kc * U * T(em)))
    return out


def _e_step(c, d, mut):
    n = c["nb"] * c["per"]
    e, _, p0, _, xp, _ = _step(c, d, np.float32, uncond=mut == "uncond_both")
    mask = visited(n, mut, SWEEP16)
    if mut in ("drop_tail", "sweep_untouched", "sweep_twice"):
        if mask is None:
            return None
        um = ~mask.numpy()
        if mut == "sweep_twice":                      # x_prev aliases x: the second visit reads what the first wrote
            _, _, p2, _, x2, _ = _step(c, d, np.float32, x=xp)
            xp, p0 = np.where(um, x2, xp), np.where(um, p2, p0)
        else:
            xp, p0, e = (np.where(um, np.float32(NAN), v) for v in (xp, p0, e))
    T = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))
    return [T(xp), T(p0)] + ([T(e)] if c.op == "plms" else [])


def _m_step(c):
    n = c["nb"] * c["per"]
    return (["drop_tail"] * (n % 256 != 0) + ["uncond_both"] * c["cfg"]
            + (["sweep_untouched"] + ["sweep_twice"] * (c.op == "ddim")) * (n > SWEEP16))


def _d_vq(c):
    m, ncode, edim = c["m"], c["ncode"], c["edim"]
    cb = _randn(c, ncode, edim)
    z = _randn(c, m, edim, salt=1)
    if c["dup"]:                       # codes 0 and 1 again further back: a row equal to either must return the FIRST index
        cb[ncode - 1] = cb[0]
        cb[ncode // 2] = cb[1]
        z[0], z[1], z[m - 1] = cb[0], cb[1], cb[1]
    return {"z": z, "cb": cb}


def vq_flips(z, cb, idx):
    """(flips against the fp64 argmin, flips that are not provable fp32 near-ties) -- the bound of conftest.vq_flip_report"""
    zd, cd = z.double(), cb.double()
    d = (zd * zd).sum(1)[:, None] + (cd * cd).sum(1)[None, :] - 2.0 * zd @ cd.t() if cb.shape[0] > 64 else \
        ((zd[:, None, :] - cd[None]) ** 2).sum(-1)
    ref = d.argmin(1)
    bad = (idx != ref).nonzero().flatten()
    if bad.numel() == 0:
        return 0, 0
    em, er = cd[idx[bad]], cd[ref[bad]]
    gap = ((zd[bad] - em) ** 2).sum(1) - ((zd[bad] - er) ** 2).sum(1)
    bound = 8 * 2.0 ** -23 * ((zd[bad] ** 2).sum(1) + torch.maximum((em ** 2).sum(1), (er ** 2).sum(1)))
    return int(bad.numel()), int((gap > bound).sum())


def _r_vq(c, d):
    return [("idx", "vq", None, None), ("zq", "vq", None, None)]


def _e_vq(c, d, mut):
    m, ncode, edim = c["m"], c["ncode"], c["edim"]
    z, cb = d["z"], d["cb"].numpy()
    if mut == "c_for_ld":
        z = misread(z, c["ldz"])
    z = z.numpy()
    z2, ee = np.zeros(m, np.float32), np.zeros(ncode, np.float32)
    for k in range(edim):
        z2 = z2 + z[:, k] * z[:, k]
        ee = ee + cb[:, k] * cb[:, k]
    with np.errstate(invalid="ignore"):
        dot = z[:, :1] * cb[None, :, 0]
        for k in range(1, edim):         # fmaf: the product is exact in fp64
            dot = (z[:, k:k + 1].astype(np.float64) * cb[None, :, k].astype(np.float64) + dot).astype(np.float32)
        dist = (z2[:, None] + ee[None, :]) - np.float32(2.0) * dot
    dist = np.where(np.isnan(dist), np.inf, dist)        # `d < best` is false for NaN: index 0 stands
    idx = ncode - 1 - np.argmin(dist[:, ::-1], axis=1) if mut == "vq_last" else np.argmin(dist, axis=1)
    idx = torch.from_numpy(idx.astype(np.int64))
    zq = d["cb"][idx]
    mask = visited(m, mut, SWEEP_VQ)
    if mut in ("drop_tail", "sweep_untouched"):
        if mask is None:
            return None
        idx = torch.where(mask, idx, torch.full_like(idx, -1))
    if mut == "vq_last" and bool((idx == torch.from_numpy(np.argmin(dist, axis=1))).all()):
        return None
    return [idx, zq]


def _m_vq(c):
    return (["drop_tail"] * (c["m"] % 256 != 0) + ["c_for_ld"] * (c["ldz"] > c["edim"] and c["m"] > 1 and c["ncode"] > 1)
            + ["sweep_untouched"] * (c["m"] > SWEEP_VQ) + ["vq_last"] * c["dup"])


def _d_gcn(c):
    n_obj, n_tri, h, kind = c["n_obj"], c["n_tri"], c["h"], c["kind"]
    g = _gen(c, 9)
    if kind == "self":
        edges = torch.zeros(n_tri, 2, dtype=torch.int64)
    else:                               # the last node appears nowhere
        edges = torch.randint(0, n_obj - 1, (n_tri, 2), generator=g)
        if kind == "hub":               # node 0 is an endpoint of every edge
            edges[0::2, 0] = 0
            edges[1::2, 1] = 0
    off_o = h + 1
    ld_t = off_o + h + c["pad"]
    nt = torch.full((n_tri, ld_t), NAN)
    nt[:, :h] = _randn(c, n_tri, h)
    nt[:, off_o:off_o + h] = _randn(c, n_tri, h, salt=1)
    return {"edges": edges, "obj": _randn(c, n_obj, h, salt=2), "pred": _randn(c, n_tri, h + 1, salt=3), "nt": nt}


def gcn_lists(edges, n_obj, n_tri_seen=None):
    e = edges.numpy()[:n_tri_seen]
    return [([t for t in range(len(e)) if e[t, 0] == o], [t for t in range(len(e)) if e[t, 1] == o]) for o in range(n_obj)]


def gcn_canon(lists, cursor=None, cover=True):
    """counts, cursor, the per-node entry lists (subject edges then object edges) and the cover flag as one int64 vector"""
    cs, co = [len(a) for a, _ in lists], [len(b) for _, b in lists]
    ent = [t for a, b in lists for t in a + b]
    return torch.tensor(cs + co + [sum(cs) + sum(co) if cursor is None else cursor, int(cover)] + ent, dtype=torch.int64)


def gcn_canon_from_csr(csr, n_obj, n_tri):
    """the device's CSR block (start | count_s | count_o | cursor | entries) in the canonical form of gcn_canon"""
    v = csr.cpu().numpy().astype(np.int64)
    st, cs, co, cur, ent = v[:n_obj], v[n_obj:2 * n_obj], v[2 * n_obj:3 * n_obj], int(v[3 * n_obj]), v[3 * n_obj + 1:]
    segs = sorted((int(s), int(s + a + b)) for s, a, b in zip(st, cs, co))
    cover = segs[0][0] == 0 and segs[-1][1] == 2 * n_tri == len(ent) and all(p[1] == q[0] for p, q in zip(segs, segs[1:]))
    ok = cover and bool((st >= 0).all()) and bool((cs >= 0).all()) and bool((co >= 0).all())
    lists = [([int(t) for t in ent[s:s + a]], [int(t) for t in ent[s + a:s + a + b]]) for s, a, b in zip(st, cs, co)] if ok else \
        [([], []) for _ in range(n_obj)]
    return gcn_canon(lists, cur, ok)


def gcn_pool_lists(nt, lists, h, off_o, ld_read=None):
    """the mean over each node's list in list order, fp32, one add per entry (gcn_segment_mean_csr_kernel)"""
    src = nt if ld_read is None else ld_read
    out = np.zeros((len(lists), h), np.float32)
    a = src.numpy()
    for o, (ls, lo) in enumerate(lists):
        acc = np.zeros(h, np.float32)
        for t in ls:
            acc = acc + a[t, :h]
        for t in lo:
            acc = acc + a[t, off_o:off_o + h]
        out[o] = acc / np.float32(max(len(ls) + len(lo), 1))
    return torch.from_numpy(out)


def _r_gcn(c, d):
    n_obj, h = c["n_obj"], c["h"]
    e = d["edges"]
    gather = torch.cat([d["obj"][e[:, 0]], d["pred"], d["obj"][e[:, 1]]], dim=1)
    lists = gcn_lists(e, n_obj)
    pooled = gcn_pool_lists(d["nt"], lists, h, h + 1)
    return [("gather", "exact", gather, None), ("pooled", "exact", pooled, None), ("csr", "exact", gcn_canon(lists), None),
            ("pooled_csr", "exact", pooled, None)]


def _e_gcn(c, d, mut):
    n_obj, n_tri, h = c["n_obj"], c["n_tri"], c["h"]
    ref = _r_gcn(c, d)
    gather, pooled = ref[0][2].clone(), ref[1][2]
    lists = gcn_lists(d["edges"], n_obj)
    nt = d["nt"]
    if mut == "drop_tail":               # the gather's last partial workgroup, the CSR build's last partial 64-lane chunk
        mask = visited(gather.numel(), mut, SWEEP16)
        if mask is not None:
            gather.view(-1)[~mask] = NAN
        if n_tri % 64 == 0 and mask is None:
            return None
        lists = gcn_lists(d["edges"], n_obj, (n_tri // 64) * 64)
    elif mut == "csr_order":
        if all(len(a) < 2 for a, _ in lists):
            return None
        lists = [(a[::-1], b) for a, b in lists]
    elif mut == "c_for_ld":
        w = 2 * h + 1
        nt = torch.as_strided(torch.cat([nt.reshape(-1), torch.full((w,), NAN)]), (n_tri, w), (w, 1))
        pooled = gcn_pool_lists(nt, lists, h, h + 1)
    return [gather, pooled, gcn_canon(lists), gcn_pool_lists(nt, lists, h, h + 1)]


def _m_gcn(c):
    return ["drop_tail", "csr_order"] + ["c_for_ld"] * (c["pad"] > 0 and c["n_tri"] > 1)


def _d_emb(c):
    idx = torch.randint(0, c["n_rows"], (c["n"],), generator=_gen(c, 1))
    idx[0], idx[-1] = 0, c["n_rows"] - 1
    return {"table": _randn(c, c["n_rows"], c["dim"]), "idx": idx}


def _r_emb(c, d):
    return [("out", "exact", d["table"][d["idx"]], None)]


def _e_emb(c, d, mut):
    out = d["table"][d["idx"]]
    mask = visited(out.numel(), mut, SWEEP16)
    if mut in ("drop_tail", "sweep_untouched"):
        if mask is None:
            return None
        out.view(-1)[~mask] = NAN
    if mut == "c_for_ld":
        out = miswrite(out, c["ldo"])
    return [out]


def _m_emb(c):
    tot = c["n"] * c["dim"]
    return ["drop_tail"] * (tot % 256 != 0) + ["c_for_ld"] * (c["ldo"] > c["dim"] and c["n"] > 1) + ["sweep_untouched"] * (tot > SWEEP16)


def _d_lsm(c):
    m, cc = c["m"], c["c"]
    x = 3.0 * _randn(c, m, cc)
    if m >= 4:
        x[0] = 1.5                                        # a row of equal values
        if cc >= 2:
            sign = torch.where(torch.arange(cc) % 2 == 0, 1.0, -1.0)
            x[1] = 80.0 * sign
            x[2, cc // 2] = -INF                          # its output is -inf there and finite elsewhere
            x[3] = 100.0 * sign                           # exp(100) is beyond fp32: the max subtraction is what keeps it finite
    return {"x": x}


def _r_lsm(c, d):
    x = d["x"].double()
    sh = x - x.max(1, keepdim=True).values
    ls = sh.exp().sum(1, keepdim=True).log()
    return [("y", "E", sh - ls, K_LSM * U * (sh.abs() + ls.abs() + 1.0))]


def _e_lsm(c, d, mut):
    m, cc = c["m"], c["c"]
    x = d["x"]
    if mut == "c_for_ld":
        x = misread(x, cc + c["pad"])
    keep_c, keep_r = cc, m
    if mut == "drop_tail":
        if cc % 64:
            keep_c = 64 * (cc // 64)
        elif m % 4:
            keep_r = m - m % 4
        else:
            return None
    xs = x[:, :keep_c]
    y = torch.full((m, cc), NAN)
    if keep_c:
        if mut == "lsm_nomax":
            y[:, :keep_c] = xs - xs.exp().sum(1, keepdim=True).log()
        else:
            sh = xs - xs.max(1, keepdim=True).values
            y[:, :keep_c] = sh - sh.exp().sum(1, keepdim=True).log()
    y[keep_r:] = NAN
    return [y]


def _m_lsm(c):
    return ["drop_tail"] + ["c_for_ld"] * (c["pad"] > 0 and c["m"] > 1) + ["lsm_nomax"] * (c["m"] >= 4 and c["c"] >= 2)


def _rownorm(row, mut=None):
    ss = float((row.double() ** 2).sum())
    n = np.float32(math.sqrt(ss))
    sq = float(n) * float(n)
    if (mut != "rowstats_nearest" and sq < ss) or (mut == "rowstats_always_bump" and sq <= ss):
        n = np.nextafter(n, np.float32(np.inf))
    return float(n)


def _rowstats_exact(d):
    """the largest row norm is an fp32 number whose square is the row's sum of squares exactly: the kernel must return it as it
    is, one ulp above is a bump that was not due"""
    ss = max(float(m.double().pow(2).sum(1).max()) for m in d["mats"])
    n = np.float32(math.sqrt(ss))
    return float(n) * float(n) == ss


def _d_rowstats(c):
    mats = [_randn(c, r, cl, salt=i) for i, (r, cl) in enumerate(c["mats"])]
    w = mats[0] if c["kind"].endswith("first") else mats[-1]   # first: a later call must keep what an earlier one left
    if c["kind"].startswith("squares"):           # the largest row is 3, 4, 0, ...: its norm is 5 exactly and must not be bumped
        for m in mats:
            m.mul_(0.01)
        w[-1] = 0.0
        w[-1, -2], w[-1, -1] = 3.0, -4.0
    else:                                # the largest entry, and the largest row, last; a norm that rounds DOWN to fp32 where one can
        w[-1, -1] = -50.0
        if w.shape[1] > 1:
            for j in range(256):
                w[-1, 0] = 1.0 + j / 256.0
                ss = float((w[-1].double() ** 2).sum())
                if float(np.float32(math.sqrt(ss))) < math.sqrt(ss) and float(np.float32(math.sqrt(ss))) ** 2 < ss:
                    break
    return {"mats": mats}


def _r_rowstats(c, d):
    n = max(float(m.double().pow(2).sum(1).sqrt().max()) for m in d["mats"])
    a = max(float(m.abs().max()) for m in d["mats"])
    norm = ("norm", "exact", torch.tensor([n], dtype=torch.float32), None) if _rowstats_exact(d) else \
        ("norm", "norm", torch.tensor([n], dtype=torch.float64), None)
    return [norm, ("amax", "exact", torch.tensor([a], dtype=torch.float32), None)]


def _e_rowstats(c, d, mut):
    n, a, changed = 0.0, 0.0, False
    for m in d["mats"]:
        rows, cols = m.shape
        if mut == "fold_overwrite":          # a call that stores its result instead of folding it into the slot
            n, a = 0.0, 0.0
        if mut == "drop_tail":
            if cols % 64:
                m, changed = m[:, :64 * (cols // 64)], True
            elif rows % 4:
                m, changed = m[:rows - rows % 4], True
        for r in m:
            if r.numel():
                n, a = max(n, _rownorm(r, mut)), max(a, float(r.abs().max()))
    if mut == "drop_tail" and not changed:
        return None
    if mut == "fold_overwrite" and [n, a] == [v.item() for v in _e_rowstats(c, d, None)]:
        return None
    if mut in ("rowstats_nearest", "rowstats_always_bump") and n == _e_rowstats(c, d, None)[0].item():
        return None
    return [torch.tensor([n], dtype=torch.float32), torch.tensor([a], dtype=torch.float32)]


def _m_rowstats(c):
    exact = _rowstats_exact(data(c))
    return ["drop_tail"] + (["rowstats_always_bump"] if exact else ["rowstats_nearest"]) + ["fold_overwrite"] * c["kind"].endswith("first")


CLAMP = float(np.float32(3.0e38))


def _d_absmax(c):
    n, kind = c["n"], c["kind"]
    x = _randn(c, n).clamp_(-4.0, 4.0)
    d = {"slot0": 0.0}
    if kind == "last":
        x[-1] = 10.0
    elif kind == "idx65537":
        x[65537 % n] = 10.0
    elif kind == "neg":
        x[n // 3] = -10.0
    elif kind == "zeros":
        x.zero_()
        x[1::2] = -0.0
    elif kind == "fold":                  # a second call into the slot the first left non-zero: once below, once above it
        d["x2"] = 0.5 * x.flip(0)
        d["x3"] = 3.0 * x.flip(0)
        x[5] = 10.0
    elif kind == "inf":
        x[n - 2] = -INF
    elif kind == "nan":
        x[n // 2] = NAN
    elif kind == "nan-idx65537":
        x[65537] = NAN
    d["x"] = x
    return d


def _absmax_one(x, slot, mut):
    a = x.abs().numpy()
    mask = visited(a.size, mut, SWEEP_ABSMAX)
    if mask is not None:
        a = a[mask.numpy()]
    if mut == "nan_dropped":              # fmaxf returns its non-NaN operand
        a = a[~np.isnan(a)]
    m = float(np.max(a)) if a.size else 0.0
    if not m < CLAMP:
        m = CLAMP
    return max(slot, m)


def _r_absmax(c, d):
    return [("slot", "exact", _e_absmax(c, d, None)[0], None)]


def _e_absmax(c, d, mut):
    if mut in ("drop_tail", "sweep_untouched") and visited(c["n"], mut, SWEEP_ABSMAX) is None:
        return None
    s = d["slot0"]
    for k in ("x", "x2", "x3"):
        if k in d:
            s = _absmax_one(d[k], s, mut)
    return [torch.tensor([s], dtype=torch.float32)]


def _m_absmax(c):
    n, kind = c["n"], c["kind"]
    return (["drop_tail"] * (kind == "last") + ["sweep_untouched"] * (n > SWEEP_ABSMAX and kind in ("last", "idx65537", "nan-idx65537"))
            + ["nan_dropped"] * kind.startswith("nan"))


def _tap_geom(c):
    nb = c["nb"]
    D, H, W = c["vol"]
    M = nb * D * H * W
    m = torch.arange(M)
    return nb, D, H, W, M, (m // (H * W)) % D, (m // W) % H, m % W


def _d_tapsum(c):
    nb, D, H, W, M, dd, hh, ww = _tap_geom(c)
    cout = c["cout"]
    g = _gen(c, 4)
    if c["ints"]:
        y = torch.randint(-8, 9, (M, cout, 27), generator=g).float()
        bias = torch.randint(-8, 9, (cout,), generator=g).float()
    else:
        y, bias = _randn(c, M, cout, 27), _randn(c, cout, salt=1)
    # Y[m'][o 27 + t] is read by the output at m' - off_t alone: NaN wherever that output is outside the volume (or in the
    # neighbouring sample), so a tap taken without its mask shows as NaN
    for t in range(27):
        kd, kh, kw = t // 9 - 1, (t // 3) % 3 - 1, t % 3 - 1
        ok = (dd - kd >= 0) & (dd - kd < D) & (hh - kh >= 0) & (hh - kh < H) & (ww - kw >= 0) & (ww - kw < W)
        y[~ok, :, t] = NAN
    return {"y": y.reshape(M, cout * 27), "bias": bias if c["bias"] else None}


def _e_tapsum(c, d, mut):
    nb, D, H, W, M, dd, hh, ww = _tap_geom(c)
    cout = c["cout"]
    P = H * W + W + 1
    y = torch.cat([torch.full((P, cout * 27), NAN), d["y"], torch.full((P, cout * 27), NAN)]).numpy()
    out = np.zeros((M, cout), np.float32)
    skip = c["axis"] if mut == "tapsum_mask" else -1
    rows = np.arange(M)
    for o in range(cout):
        acc = np.zeros(M, np.float32)
        for t in range(27):
            kd, kh, kw = t // 9 - 1, (t // 3) % 3 - 1, t % 3 - 1
            ok = torch.ones(M, dtype=torch.bool)
            for ax, (p, k, n) in enumerate(((dd, kd, D), (hh, kh, H), (ww, kw, W))):
                if ax != skip:
                    ok &= (p + k >= 0) & (p + k < n)
            v = y[P + rows + (kd * H + kh) * W + kw, o * 27 + t]
            acc = acc + np.where(ok.numpy(), v, np.float32(0.0))
        out[:, o] = acc + d["bias"].numpy()[o] if d["bias"] is not None else acc
    out = torch.from_numpy(out)
    if mut == "drop_tail":
        out[(M // 256) * 256:] = NAN
    return [out]


def _r_tapsum(c, d):
    return [("out", "exact", _e_tapsum(c, d, None)[0], None)]


def _m_tapsum(c):
    return ["drop_tail", "tapsum_mask"]


def _d_pack(c):
    return {"w": _randn(c, c["cout"], c["cin"], 27)}


def _e_pack(c, d, mut):
    cout, cin, ncolp = c["cout"], c["cin"], c["ncolp"]
    kg = ((cin + 15) // 16) * 2
    V = np.zeros((kg * 8, ncolp), np.float32)
    V[:cin, :27 * cout] = (d["w"].numpy() * np.float32(c["scale"])).transpose(1, 0, 2).reshape(cin, cout * 27)
    V = np.ascontiguousarray(V.reshape(kg, 8, ncolp).transpose(0, 2, 1))
    hi = V.astype(np.float16)
    lo = (V - hi.astype(np.float32)).astype(np.float16)
    hi, lo = torch.from_numpy(hi), torch.from_numpy(lo)
    if mut == "drop_tail":
        keep = (hi.numel() // 256) * 256
        if keep == hi.numel():
            return None
        hi.view(-1)[keep:] = NAN
        lo.view(-1)[keep:] = NAN
    return [hi, lo]


def _r_pack(c, d):
    hi, lo = _e_pack(c, d, None)
    return [("hi", "exact", hi, None), ("lo", "exact", lo, None)]


def _m_pack(c):
    return ["drop_tail"]


def _d_chamfer(c):
    return {"a": _randn(c, c["b"], c["n"], 3), "b": _randn(c, c["b"], c["m"], 3, salt=1)}


def _e_chamfer(c, d, mut):
    a, b = d["a"].numpy(), d["b"].numpy()
    dx, dy, dz = (b[:, None, :, k] - a[:, :, None, k] for k in range(3))
    dist = (dx * dx + dy * dy) + dz * dz
    idx = dist.argmin(-1)
    best = torch.from_numpy(np.take_along_axis(dist, idx[..., None], -1)[..., 0].copy())
    idx = torch.from_numpy(idx.astype(np.int32))
    if mut == "drop_tail":
        best[:, (c["n"] // 256) * 256:] = NAN
    return [best, idx]


def _r_chamfer(c, d):
    best, idx = _e_chamfer(c, d, None)
    return [("dist", "exact", best, None), ("idx", "exact", idx, None)]


def _m_chamfer(c):
    return ["drop_tail"]


def _d_synth(c):
    return {}


def _e_synth(c, d, mut):
    n = c["n"]
    with np.errstate(over="ignore"):
        z = np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(c["base"])
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    k = (z >> np.uint64(40)).astype(np.int64)
    u = (2 * k - (1 << 24)).astype(np.float64) / 16777216.0
    out = torch.from_numpy((u * c["scale"] + c["offset"]).astype(np.float32))
    mask = visited(n, mut, SWEEP32)
    if mut is not None:
        if mask is None:
            return None
        out[~mask] = NAN
    return [out]


def _r_synth(c, d):
    return [("out", "exact", _e_synth(c, d, None)[0], None)]


def _m_synth(c):
    return ["drop_tail"] * (c["n"] % 256 != 0) + ["sweep_untouched"] * (c["n"] > SWEEP32)


OPS = {
    "geglu": (_d_geglu, _r_geglu, _e_geglu, _m_geglu), "copy_rows": (_d_copy, _r_copy, _e_copy, _m_copy),
    "add_rowvec": (_d_addrv, _r_addrv, _e_addrv, _m_addrv), "concat": (_d_concat, _r_concat, _e_concat, _m_concat),
    "to_ndhwc": (_d_ndhwc, _r_ndhwc, _e_ndhwc, _m_ndhwc), "to_nchw": (_d_nchw, _r_nchw, _e_nchw, _m_nchw),
    "ts_embedding": (_d_ts, _r_ts, _e_ts, _m_ts), "ddim": (_d_step, _r_step, _e_step, _m_step),
    "plms": (_d_step, _r_step, _e_step, _m_step), "vq": (_d_vq, _r_vq, _e_vq, _m_vq), "gcn": (_d_gcn, _r_gcn, _e_gcn, _m_gcn),
    "embedding": (_d_emb, _r_emb, _e_emb, _m_emb), "log_softmax": (_d_lsm, _r_lsm, _e_lsm, _m_lsm),
    "rowstats": (_d_rowstats, _r_rowstats, _e_rowstats, _m_rowstats), "absmax": (_d_absmax, _r_absmax, _e_absmax, _m_absmax),
    "tapsum27": (_d_tapsum, _r_tapsum, _e_tapsum, _m_tapsum), "pack_tapcol": (_d_pack, _r_pack, _e_pack, _m_pack),
    "chamfer": (_d_chamfer, _r_chamfer, _e_chamfer, _m_chamfer), "synth_fill": (_d_synth, _r_synth, _e_synth, _m_synth),
}


@lru_cache(maxsize=2)
def data(c):
    return OPS[c.op][0](c)


@lru_cache(maxsize=2)
def reference(c):
    return OPS[c.op][1](c, data(c))


def emulate(c, mutant=None):
    return OPS[c.op][2](c, data(c), mutant)


def mutants_of(c):
    return OPS[c.op][3](c)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


def ratio_one(val, kind, ref, E):
    val = val.detach().cpu()
    if kind == "exact":
        return 0.0 if val.shape == ref.shape and val.dtype == ref.dtype and torch.equal(_bits(val), _bits(ref)) else INF
    if kind == "norm":
        r = (float(val.double()) - float(ref)) / (float(ref) * 2.0 ** -22)
        return r if r >= 0.0 else INF
    val = val.double().reshape(ref.shape)
    fin = torch.isfinite(ref)
    if bool((~fin & (val != ref)).any()) or not bool(torch.isfinite(val[fin]).all()):
        return INF
    diff = (val - ref).abs()[fin]
    e = E[fin]
    if bool(((e == 0) & (diff != 0)).any()):
        return INF
    return float((diff / e.clamp_min(1e-300)).max()) if diff.numel() else 0.0


def vq_report(c, idx, zq):
    """(flips, unexplained flips, duplicate rows exact, zq == codebook[idx] and idx in range)"""
    d = data(c)
    idx = idx.detach().cpu()
    if idx.dtype != torch.int64 or bool(((idx < 0) | (idx >= c["ncode"])).any()):
        return None
    flips, bad = vq_flips(d["z"], d["cb"], idx)
    dup_ok = (not c["dup"]) or (int(idx[0]) == 0 and int(idx[1]) == 1 and int(idx[-1]) == 1)
    return flips, bad, dup_ok, torch.equal(_bits(zq.detach().cpu()), _bits(d["cb"][idx]))


def worst_ratio(outs, c):
    """the worst element of any output in units of its gate (<= 1 passes); inf for a broken identity, NaN, or a flipped index"""
    if c.op == "vq":
        r = vq_report(c, outs[0], outs[1])
        return 0.0 if r is not None and r[0] <= 2 and r[1] == 0 and r[2] and r[3] else INF
    ref = reference(c)
    assert len(outs) == len(ref), (case_id(c), len(outs), len(ref))
    return max(ratio_one(v, kind, r, E) for v, (_, kind, r, E) in zip(outs, ref))


def measured_k(op):
    """worst |fp32 - fp64| / (2^-24 S) of the torch CPU evaluation over the op's cases: what K_GEGLU / K_TSEMB / K_LSM are set from"""
    k = {"geglu": K_GEGLU, "ts_embedding": K_TSEMB, "log_softmax": K_LSM}[op]
    return k * max(worst_ratio(emulate(c), c) for c in BY_OP[op])
