"""The K-wave GEMM (csrc/cs_gemm_kw.hip, tile code 10, kw_gemm_f16x3_kernel<PAIR>) for test_kwave_variants_cpu.py /
test_kwave_variants_gpu.py: the case table, what the table is for (check_table), and the cases of the refusal test.

The kernel.  One workgroup of four waves per 64x64 output tile; nk = ceil(cin / 16) K chunks, wave w owns chunks
[w per, min(nk, (w + 1) per)) with per = ceil(nk / 4) -- for nk in {1, 2, 3, 5, 6, 9} one or more waves own nothing and only
issue zero-fill DMA.  Each wave runs a four-stage LDS ring, three chunks of DMA ahead of the MFMAs: per > 4 wraps the ring, and
the unrolled loop ends in a tail of per % 4 stages.  cin % 16 in {4, 8, 12} (fp32 operand) leaves a partial last chunk whose
16-byte pieces at c >= cin must read zero, not the lda gap; rows m >= M and columns n >= cout of edge tiles are zero-filled the
same way and kept out of memory by the epilogue's mask.  Workgroup b takes tile (b % 8 < r ? ... ) + b / 8 with
q, r = divmod(nblk, 8): a bijection for every nblk, including nblk < 8 and nblk % 8 != 0.

A row is test_gemm_variants_gpu.py's Case -- _c("pw", fmt, 10, 0, (nb, 1, 1, W), cin, cout, epi, view) -- so that file's _data /
_device / _out_buffer / _desc / _launch serve it unchanged (fmt 0: fp32 operand split in the loop; fmt 2: LayerNorm's interleaved
pair; view: lda > cin at a column offset, ldo = cout + 12 at offset 4, own ldr / ldrv, NaN around every operand, the sentinel
around the output).  Its seeds come from this file (FOREIGN_SEEDS), never from an index into that file's tables."""
from test_gemm_variants_gpu import FOREIGN_SEEDS, _c, _id, _rows

NAMES = ["A1", "A2", "A3", "A4", "A5", "A6", "A7", "A8", "A9", "A10", "A11", "P1", "P2", "P3", "P4", "P5", "P6"]
KW_CASES = [
    # fp32 operand                                                   M    chunks per wave     tiles m x n
    _c("pw", 0, 10, 0, (1, 1, 1, 1), 12, 68, "bias", False),       # 1    12 -> 1 0 0 0        1 x 2
    _c("pw", 0, 10, 0, (2, 1, 1, 1), 20, 132, "rowvec", True),     # 2    20 -> 1 1 0 0        1 x 3
    _c("pw", 0, 10, 0, (1, 1, 1, 65), 44, 36, "res", True),        # 65   44 -> 1 1 1 0        2 x 1   one row in the last tile
    _c("pw", 0, 10, 0, (2, 1, 1, 75), 72, 124, "bn", False),       # 150  72 -> 2 2 1 0        3 x 2   cin % 16 = 8, cout % 64 = 60
    _c("pw", 0, 10, 0, (3, 1, 1, 43), 100, 4, "bias", True),       # 129  100 -> 2 2 2 1       3 x 1   one float4 of columns
    _c("pw", 0, 10, 0, (1, 1, 1, 257), 132, 196, "rowvec", False),  # 257  132 -> 3 3 3 0       5 x 4   20 workgroups
    _c("pw", 0, 10, 0, (4, 1, 1, 75), 196, 68, "res", True),       # 300  196 -> 4 4 4 1       5 x 2   10 workgroups
    _c("pw", 0, 10, 0, (1, 1, 1, 63), 260, 228, "bn", False),      # 63   260 -> 5 5 5 2       1 x 4   ring wraps, tail 1 / 2
    _c("pw", 0, 10, 0, (2, 1, 1, 100), 324, 132, "bias", True),    # 200  324 -> 6 6 6 3       4 x 3   tail 2 / 3, 12 workgroups
    _c("pw", 0, 10, 0, (2, 1, 1, 65), 404, 72, "rowvec", True),    # 130  404 -> 7 7 7 5       3 x 2   tail 3 / 1
    _c("pw", 0, 10, 0, (8, 1, 1, 64), 64, 64, "res", False),       # 512  64 -> 1 1 1 1        8 x 1   no edge at all, 8 workgroups
    # interleaved pair
    _c("pw", 2, 10, 0, (2, 1, 1, 75), 16, 68, "res", False),       # 150  16 -> 1 0 0 0        3 x 2
    _c("pw", 2, 10, 0, (1, 1, 1, 65), 48, 132, "bn", True),        # 65   48 -> 1 1 1 0        2 x 3
    _c("pw", 2, 10, 0, (3, 1, 1, 43), 80, 40, "rowvec", False),    # 129  80 -> 2 2 1 0        3 x 1
    _c("pw", 2, 10, 0, (1, 1, 1, 257), 144, 200, "bias", True),    # 257  144 -> 3 3 3 0       5 x 4
    _c("pw", 2, 10, 0, (4, 1, 1, 25), 272, 72, "res", True),       # 100  272 -> 5 5 5 2       2 x 2
    _c("pw", 2, 10, 0, (2, 1, 1, 1), 112, 224, "bias", False),     # 2    112 -> 2 2 2 1       1 x 4
]
BY_NAME = dict(zip(NAMES, KW_CASES))

# the refusal test's descriptors: M = 150, cin = 132 (nine chunks), cout = 224, fp32 operand, bias + residual -- what auto-selection
# gives the K-wave kernel on the GPU -- and the geometries its rows change to (the pair rows reuse fp32-sized buffers: a pair word
# is 32 bits, and a refused launch reads nothing)
R_BASE = _c("pw", 0, 10, 0, (2, 1, 1, 75), 132, 224, "res", False)
R_CIN136 = R_BASE._replace(cin=136)
R_CIN144 = R_BASE._replace(cin=144)
R_COUT228 = R_BASE._replace(cout=228)
R_K333 = _c("gather", 0, 0, 0, (2, 1, 1, 75), 132, 224, "res", False)
R_CASES = [R_BASE, R_CIN136, R_CIN144, R_COUT228, R_K333]

FOREIGN_SEEDS.update({c: 5000 + 16 * i for i, c in enumerate(KW_CASES)})
FOREIGN_SEEDS.update({c: 9000 + 16 * i for i, c in enumerate(R_CASES)})


def case_id(c):
    return (NAMES[KW_CASES.index(c)] + "-" if c in KW_CASES else "") + _id(c)


def nk(c):
    return (c.cin + 15) // 16


def per_wave(c):
    """K chunks of waves 0 .. 3: [w per, min(nk, (w + 1) per))"""
    n = nk(c)
    per = (n + 3) // 4
    return [max(0, min(n, (w + 1) * per) - w * per) for w in range(4)]


def tiles(c):
    return (_rows(c) + 63) // 64, (c.cout + 63) // 64


def nblk(c):
    tm, tn = tiles(c)
    return tm * tn


def row_gated(c):
    """a worst-row figure over fewer than 32 values is single elements: the fp64 reference alone does not hold 1e-6 there"""
    return c.cout >= 32


def col_gated(c):
    return _rows(c) >= 63


def tile_map(n):
    """the kernel's XCD-aware map, workgroup -> tile, restated: workgroup b runs on XCD b % 8, each XCD owns a run of tiles"""
    q, r = divmod(n, 8)
    out = []
    for b in range(n):
        xcd, within = b % 8, b // 8
        out.append((xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + within)
    return out


def bound_scale(mb):
    """the operand scale CsConvGemm.a_bound asks for, from the documented rule: the largest power of two <= 65000 / mb (fp32
    arithmetic), exponent clamped to [-8, 40]; 2^40 for a bound that is zero, negative, >= 3e38 or NaN (nothing to scale by)"""
    import math
    import numpy as np
    f = np.float32(mb)
    if not (f > np.float32(0.0) and f < np.float32(3.0e38)):
        return 2.0 ** 40
    q = float(np.float32(65000.0) / f)
    e = math.frexp(q)[1] - 1                   # q = m 2^(e + 1), 0.5 <= m < 1: 2^e <= q < 2^(e + 1)
    return 2.0 ** min(max(e, -8), 40)


def check_table(cases):
    """what the table is for: an edit that thins it out fails here"""
    assert all(c.route == "pw" and c.tile == 10 and c.slab == 0 and c.fmt in (0, 2) for c in cases)
    assert all(c.vol[1] == c.vol[2] == 1 and c.cin < 2000 and c.cout % 4 == 0 for c in cases)
    assert all(c.cin % (16 if c.fmt == 2 else 4) == 0 for c in cases)
    forms = [[c for c in cases if c.fmt == f] for f in (0, 2)]
    # chunks per wave: 1, 2, 3, 4 and three values above 4 with three different residues mod 4 (the ring wraps, every tail)
    pers = {max(per_wave(c)) for c in cases}
    assert {1, 2, 3, 4} <= pers, pers
    assert len({p % 4 for p in pers if p > 4}) >= 3 and len([p for p in pers if p > 4]) >= 3, pers
    # empty waves: at least five cases, on both operand forms
    empty = [c for c in cases if 0 in per_wave(c)]
    assert len(empty) >= 5 and {c.fmt for c in empty} == {0, 2}
    assert all(sum(per_wave(c)) == nk(c) for c in cases)
    # partial last chunk (fp32 operand): one, two and three 16-byte pieces
    assert {4, 8, 12} <= {c.cin % 16 for c in forms[0]}
    # row tiles: one valid row in the last of several tiles, a full and an all-but-full last tile, a single row
    ms = [_rows(c) for c in cases]
    assert any(m % 64 == 1 and m > 64 for m in ms) and any(m % 64 == 0 for m in ms) and any(m % 64 == 63 for m in ms)
    assert 1 in ms
    # column tiles
    assert {4, 60, 0} <= {c.cout % 64 for c in cases}
    assert any(c.cout < 64 for c in cases) and any(c.cout == 4 for c in cases)
    # grid sizes for the XCD map: below 8, a multiple of 8, above 8 and ragged
    grids = {nblk(c) for c in cases}
    assert len([g for g in grids if g < 8]) >= 3, grids
    assert any(g % 8 == 0 for g in grids), grids
    assert len([g for g in grids if g > 8 and g % 8]) >= 2, grids
    for f in forms:
        assert {c.epi for c in f} == {"bias", "rowvec", "res", "bn"}
        assert 0.4 <= sum(c.view for c in f) / len(f) <= 0.6
    # every case keeps at least one of the two directional gates
    assert all(row_gated(c) or col_gated(c) for c in cases)
