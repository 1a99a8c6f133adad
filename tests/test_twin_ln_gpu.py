"""cs_twin_layernorm_pair16 (twin_ln_pair_kernel<2|4>, csrc/cs_twin_ln.hip) on its own: the hand-over of the late guidance split
(cs_unet.hip::attn_block, twin).  For replica g in {0, 1} and row r < M
    t1[g M + r] = (y[r] + rowvec[(g M + r) / rv_rows]) + res[r],    pair[g M + r] = layernorm_pair16(t1[g M + r])
must be, bit for bit, what the GEMM epilogue's two fp32 adds and today's ln_pair kernel give on the duplicated tensors.

Shapes, the smallest at which it can go wrong: C = 448 and 672 (ln_pair_kernel<2> / <4>'s widths in the shipped UNet) and 64 (the
reduced UNet's); B = 3 samples of rv_rows = 5 tokens (M = 15: the four rows of a workgroup straddle samples, and M % 4 != 0 puts
the replica boundary inside the last workgroup's rows) and of 40 tokens (M = 120); the row vectors at a row stride > C; both
outputs as views (row stride > C) inside sentinel-filled allocations.

The fp64 gate is the one tests/test_norm_variants_gpu.py applies to ln_pair (tests/_norm_cases.py::reference, kind "pair16"):
err <= E elementwise, E = u [rho |gamma| (L a + 4 |x - mu|) + L |t - beta| + 2 |t|] + 2^-22 |t| + 2^-25 / s, u = 2^-24,
L = log2(c) + 4, a = the row mean of |x| -- with x = the kernel's own fp32 t1, the LayerNorm's input."""
import ctypes as C
import math

import pytest
import torch

import _norm_cases as N

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5AA5A5
PRE, POST = 3, 5
B = 3
SCALE = 16.0


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _out(rows, cols, ld, off):
    """(allocation, [rows, cols] view at column `off` of rows of `ld` floats, bands of rows around it): every word = sentinel"""
    buf = torch.empty((PRE + rows + POST) * ld, dtype=torch.float32, device="cuda")
    buf.view(torch.int32).fill_(SENTINEL)
    buf = buf.view(PRE + rows + POST, ld)
    return buf, buf[PRE:PRE + rows, off:off + cols]


def _untouched(buf, v):
    chk = buf.clone().view(torch.int32)
    off = v.storage_offset() - PRE * buf.shape[1]
    chk[PRE:PRE + v.shape[0], off:off + v.shape[1]] = SENTINEL
    return bool((chk == SENTINEL).all())


def _inputs(c, rv_rows, gamma_scale=1.0):
    g = torch.Generator().manual_seed(1000 * c + rv_rows)
    m = B * rv_rows
    y = (torch.randn(m, c, generator=g) * 2.0 + 0.7).cuda()
    res = (torch.randn(m, c, generator=g) * 1.5 - 0.3).cuda()
    # the 2 B halves' row vectors as a column slice of a wider tensor: ldrv = c + 32
    wide = torch.full((2 * B, c + 32), float("nan"), device="cuda")
    rv = wide[:, 16:16 + c]
    rv.copy_(torch.randn(2 * B, c, generator=g))
    gam = ((torch.randn(c, generator=g) * 0.2 + 1.0) * gamma_scale).cuda()
    bet = (torch.randn(c, generator=g) * 0.1).cuda()
    return y, res, rv, gam, bet


def _twin(lib, y, res, rv, gam, bet, rv_rows, s, status):
    m, c = y.shape
    T, P = _out(2 * m, c, c + 20, 8), _out(2 * m, c, c + 32, 16)
    rc = lib.cs_twin_layernorm_pair16(y.data_ptr(), rv.data_ptr(), res.data_ptr(), gam.data_ptr(), bet.data_ptr(), T[1].data_ptr(),
                                      P[1].data_ptr(), m, c, y.stride(0), rv.stride(0), rv_rows, res.stride(0), T[1].stride(0),
                                      P[1].stride(0), N.EPS, s, status.data_ptr(), _stream())
    assert rc == 0, rc
    return T, P


def _t1_ref(y, res, rv, rv_rows):
    """the GEMM epilogue's order on the duplicated tensors: += rowvec, then += res (two fp32 adds per element)"""
    m = y.shape[0]
    return (torch.cat([y, y]) + rv.repeat_interleave(rv_rows, dim=0)[:2 * m]) + torch.cat([res, res])


def _decode_pair(p, m, c):
    """fp32-tagged pair rows -> hi, lo [m, c] (per 16-channel chunk [hi c0-7 | lo c0-7 | hi c8-15 | lo c8-15])"""
    v = p.contiguous().view(torch.float16).reshape(m, c // 16, 2, 2, 8)
    return v[:, :, :, 0, :].reshape(m, c), v[:, :, :, 1, :].reshape(m, c)


@pytest.mark.parametrize("rv_rows", [5, 40])
@pytest.mark.parametrize("c", [448, 672, 64])
def test_twin_equals_epilogue_adds_then_ln_pair(c, rv_rows):
    from commonscenes_amd import lib as L, ops
    lib = L.load()
    y, res, rv, gam, bet = _inputs(c, rv_rows)
    m = B * rv_rows
    ops.clear_status()
    status = ops.status_word()
    T, P = _twin(lib, y, res, rv, gam, bet, rv_rows, SCALE, status)
    T2, P2 = _twin(lib, y, res, rv, gam, bet, rv_rows, SCALE, status)
    ref = _t1_ref(y, res, rv, rv_rows)
    pref = ops.layernorm(ref, gam, bet, eps=N.EPS, pair_scale=SCALE)
    torch.cuda.synchronize()
    assert isinstance(pref, ops.Pair16)
    assert torch.equal(T[1].contiguous().view(torch.int32), ref.view(torch.int32)), "t1 != (y + rowvec) + res"
    assert torch.equal(P[1].contiguous().view(torch.int32), pref.t.view(torch.int32)), "pair != ln_pair(t1)"
    assert torch.equal(T[0].view(torch.int32), T2[0].view(torch.int32)) and torch.equal(P[0].view(torch.int32), P2[0].view(torch.int32))
    assert _untouched(*T) and _untouched(*P), "wrote outside its views"
    assert ops.read_status() == 0
    # fp64 LayerNorm of the kernel's input t1 under ln_pair's gate (tests/_norm_cases.py::reference, "pair16")
    hi, lo = _decode_pair(P[1], 2 * m, c)
    val = ((hi.double() + lo.double()) / SCALE).cpu()
    x, g, b = ref.double().cpu(), gam.double().cpu(), bet.double().cpu()
    mu = x.mean(dim=1, keepdim=True)
    var = (x * x).mean(dim=1, keepdim=True) - mu * mu
    rho = 1.0 / torch.sqrt(var + N.EPS)
    tt = (x - mu) * rho * g + b
    lg = math.log2(c) + 4.0
    a = x.abs().mean(dim=1, keepdim=True)
    e = N.U * (rho * g.abs() * (lg * a + 4.0 * (x - mu).abs()) + lg * (tt - b).abs() + 2.0 * tt.abs())
    e = e + 2.0 ** -22 * tt.abs() + 2.0 ** -25 / SCALE
    ratio = float(((val - tt).abs() / e).max())
    print(f"twin_ln c={c} M={m}: err/E {ratio:.3f}")
    assert torch.isfinite(val).all() and ratio <= 1.0, ratio


def test_twin_raises_the_overflow_flag_as_ln_pair_does():
    """gamma x 1e4: |LayerNorm| x 16 leaves the fp16 range -- the status word gets CS_STATUS_F16X3_OVERFLOW, as from ln_pair on
    the same t1; the same inputs with the plain gamma leave it clear"""
    from commonscenes_amd import lib as L, ops
    lib = L.load()
    for gscale, want in ((1e4, L.STATUS_F16X3_OVERFLOW), (1.0, 0)):
        y, res, rv, gam, bet = _inputs(448, 5, gscale)
        st = torch.zeros(2, dtype=torch.int32, device="cuda")
        _twin(lib, y, res, rv, gam, bet, 5, SCALE, st[0:1])
        ref = _t1_ref(y, res, rv, 5)
        out = torch.empty_like(ref)
        rc = lib.cs_layernorm_pair16(ref.data_ptr(), gam.data_ptr(), bet.data_ptr(), out.data_ptr(), ref.shape[0], 448, 448, 448,
                                     N.EPS, SCALE, st[1:2].data_ptr(), _stream())
        torch.cuda.synchronize()
        assert rc == 0 and st.tolist() == [want, want], (gscale, st.tolist())


def test_twin_rejects_malformed_arguments():
    from commonscenes_amd import lib as L
    lib = L.load()
    buf = torch.zeros(4096, device="cuda")
    X, S, st = buf.data_ptr(), _stream(), None
    ok = dict(m=4, c=32, ldy=32, ldrv=32, rv_rows=2, ldr=32, ldt=32, ldp=32)
    bad = [dict(c=24), dict(ldp=40), dict(ldt=28), dict(ldy=16), dict(rv_rows=0), dict(m=0), dict(ldrv=34)]
    for d in bad:
        k = dict(ok, **d)
        rc = lib.cs_twin_layernorm_pair16(X, X, X, X, X, X, X, k["m"], k["c"], k["ldy"], k["ldrv"], k["rv_rows"], k["ldr"], k["ldt"],
                                          k["ldp"], N.EPS, SCALE, st, S)
        assert rc == L.CS_EINVAL, d
    assert lib.cs_twin_layernorm_pair16(X, X + 4, X, X, X, X, X, 4, 32, 32, 32, 2, 32, 32, 32, N.EPS, SCALE, st, S) == L.CS_EINVAL
    assert lib.cs_twin_layernorm_pair16(X, X, X, X, X, X, X, 4, 32, 32, 32, 2, 32, 32, 32, N.EPS, 0.0, st, S) == L.CS_EINVAL
