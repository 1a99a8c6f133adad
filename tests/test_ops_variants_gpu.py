"""Every extern "C" entry of commonscenes_amd/csrc/cs_ops.hip (24, recounted from the source by test_ops_variants_cpu.py) at the
cases of tests/_ops_cases.py: a single element, a tail workgroup, row strides wider than the rows, groups that do not divide the
rows, and one shape per kernel that is larger than one sweep of its capped grid, so that the second pass of the grid-stride loop
runs (and, for the in-place add_rowvec and the aliased x_prev == x of the update kernels, an element visited twice would show).
The entries are called through ops.*, or through ctypes where ops has no wrapper with explicit ld (cs_copy_rows, cs_absmax,
cs_log_softmax, cs_tapsum27, cs_pack_weight_f16x3_tapcol, cs_chamfer_nm_distance, cs_synth_fill).

Checks per case.  (1) The gate of _ops_cases.py: bit equality for data movement and the fp32 sequences the source pins down,
|out - fp64| <= E elementwise otherwise, N <= norm <= N (1 + 2^-22), VQ indices against the fp64 argmin.  (2) The identities the
source claims: cs_ddim_cfg_update_dev == the scalar entry, out = x == out of place, null pred_x0 / e_out leave x_prev unchanged,
cs_ddim_coefficients == the numpy fp32 coefficients, a second run == the first.  (3) Every case with a view: operands inside
wider allocations with bands of rows before and after, NaN in the input gaps and bands, 0x5A5AA5A5 in every word of the output
allocation, which must survive outside the view.  (4) The argument rules as rejections: CS_EINVAL / CsError, nothing written.
(5) The index guards of cs_gcn_gather_cat, cs_gcn_segment_mean and cs_embedding.

cs_absmax with a NaN in the tensor: the reduction was built from fmaxf, which returns its non-NaN operand, so the slot held the
max of the finite values and nothing was flagged; the kernel now carries the NaN to its 3.0e38 clamp (the parent commit fails
absmax-n1-nan, -n524291-nan and -nan-idx65537; figures in profiles/ops_variants_parity.txt).

A row norm that is exact in fp32 (the 3, 4 rows: 5.0; a single entry) is gated by bit equality, not by the band: one ulp of 5 is
0.8 of 5 * 2^-22, so the band would pass a bump that was not due.  The multi-matrix cases carry the maximum in the last and in
the first call.

Measured (profiles/ops_variants_parity.txt): 87 cases bit-exact; the worst ratio to a gate is 0.83 (plms, 10^6 elements, equal to
the numpy fp32 evaluation bit for bit); geglu 0.13, timestep_embedding 0.23, log_softmax 0.22, the row norm 0.31 of its one-bump
band; no VQ flip in any case."""
import ctypes as C

import numpy as np
import pytest
import torch

import _ops_cases as N

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5AA5A5
PRE, POST = 3, 5


def _mods():
    from commonscenes_amd import lib as L, ops
    return L, L.load(), ops


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _in(t, ld=None):
    """2-D CPU tensor -> its copy as a [rows, cols] view (row stride ld) of a NaN-filled allocation with bands of rows around it"""
    rows, cols = t.shape
    ld = cols if ld is None else ld
    buf = torch.full((PRE + rows + POST, ld), float("nan"), dtype=t.dtype, device="cuda")
    v = buf[PRE:PRE + rows, :cols]
    v.copy_(t)
    return v


def _out(rows, cols, ld=None, dtype=torch.float32):
    """(allocation, [rows, cols] view with row stride ld): every word of the allocation holds the sentinel"""
    ld = cols if ld is None else ld
    buf = torch.empty((PRE + rows + POST) * ld, dtype=dtype, device="cuda")
    buf.view(torch.int32).fill_(SENTINEL)
    buf = buf.view(PRE + rows + POST, ld)
    return buf, buf[PRE:PRE + rows, :cols]


def _words(t):
    return t.reshape(-1).view(torch.int32)


def _untouched(buf, v):
    """every word of the allocation outside the view still holds the sentinel"""
    pat = torch.empty_like(buf)
    _words(pat).fill_(SENTINEL)
    chk = buf.clone()
    chk[PRE:PRE + v.shape[0], :v.shape[1]] = pat[PRE:PRE + v.shape[0], :v.shape[1]]
    return torch.equal(_words(chk), _words(pat))


def _pristine(buf):
    return bool((_words(buf) == SENTINEL).all())


def _ok(rc, what):
    assert rc == 0, (what, rc)


# ---- one runner per op: (outputs in the order of N.reference, guarded (allocation, view) pairs) ---------------------------
def _run_geglu(c, L, lib, ops):
    x = _in(N.data(c)["x"], c["ldx"])
    buf, o = _out(c["m"], c["h"], c["ldo"])
    ops.geglu(x, out=o)
    return [o], [(buf, o)]


def _run_copy_rows(c, L, lib, ops):
    s = _in(N.data(c)["src"], c["lds"])
    buf, o = _out(c["m"], c["c"], c["ldd"])
    _ok(lib.cs_copy_rows(s.data_ptr(), o.data_ptr(), c["m"], c["c"], c["lds"], c["ldd"], _stream()), "cs_copy_rows")
    return [o], [(buf, o)]


def _run_add_rowvec(c, L, lib, ops):
    d = N.data(c)
    buf, x = _out(c["m"], c["c"], c["ldx"])
    x.copy_(d["x"])
    ops.add_rowvec_(x, _in(d["v"], c["ldv"]), c["rows"])
    return [x], [(buf, x)]


def _run_concat(c, L, lib, ops):
    d = N.data(c)
    a = _in(d["a"].reshape(-1, c["ca"]), c["lda"]).view(*d["a"].shape)
    b = _in(d["b"].reshape(-1, c["cb"]), c["ldb"]).view(*d["b"].shape)
    return [ops.concat_channels(a, b)], []


def _run_to_ndhwc(c, L, lib, ops):
    x = N.data(c)["x"].cuda().reshape(c["nb"], c["c"], *c["sp"])
    return [ops.nchw_to_ndhwc(x, c["cpad"]).reshape(c["nb"], -1, c["cpad"])], []


def _run_to_nchw(c, L, lib, ops):
    x = _in(N.data(c)["x"].reshape(-1, c["c"]), c["ldx"]).view(c["nb"], *c["sp"], c["c"])
    return [ops.ndhwc_to_nchw(x).reshape(c["nb"], c["c"], -1)], []


def _run_ts_embedding(c, L, lib, ops):
    out = ops.timestep_embedding(N.data(c)["t"].cuda(), c["dim"], c["mp"])
    if c["dim"] % 2:
        assert bool((_words(out[:, -1].contiguous()) == 0).all()), "the last column of an odd dim is an exact zero"
    return [out], []


def _step_args(c):
    d = N.data(c)
    n = c["nb"] * c["per"]
    x = d["x"].cuda().reshape(c["nb"], c["per"])
    eps = d["eps"].cuda().reshape(-1, c["per"])
    s1 = float(np.float32(np.sqrt(1.0 - N.A_T)))
    return d, n, x, eps, s1


def _run_ddim(c, L, lib, ops):
    d, n, x, eps, s1 = _step_args(c)
    noise = d["noise"].cuda().reshape_as(x) if "noise" in d else None
    sigma, cfg = (N.SIGMA if noise is not None else 0.0), bool(c["cfg"])
    coefs = tuple(float(v) for v in N.ddim_coefs(sigma))
    assert ops.ddim_coefficients(N.A_T, N.A_PREV, sigma, s1) == coefs, "cs_ddim_coefficients != the numpy fp32 coefficients"
    call = lambda xx, **kw: ops.ddim_cfg_update(xx, eps, N.A_T, N.A_PREV, sigma, s1, N.CFG_SCALE, cfg, noise=noise, **kw)
    xp, p0 = call(x)
    xp2, p02 = call(x)
    xp3, none = call(x, want_pred_x0=False)
    xa = x.clone()
    xa2, p0a = call(xa, out=xa)
    cd = torch.tensor(coefs, dtype=torch.float32, device="cuda")
    p0d = torch.empty_like(x)
    xpd = ops.ddim_cfg_update_dev(x, eps, cd, N.CFG_SCALE, cfg, noise=noise, pred_x0=p0d)
    xpd2 = ops.ddim_cfg_update_dev(x, eps, cd, N.CFG_SCALE, cfg, noise=noise)
    xb = x.clone()
    ops.ddim_cfg_update_dev(xb, eps, cd, N.CFG_SCALE, cfg, noise=noise, out=xb)
    torch.cuda.synchronize()
    assert torch.equal(xp, xp2) and torch.equal(p0, p02), "a second run differs"
    assert none is None and torch.equal(xp, xp3) and torch.equal(xp, xpd2), "x_prev depends on pred_x0 being asked for"
    assert xa2.data_ptr() == xa.data_ptr() and torch.equal(xa, xp) and torch.equal(p0a, p0), "out = x != out of place"
    assert torch.equal(xpd, xp) and torch.equal(p0d, p0) and torch.equal(xb, xp), "_dev != the scalar entry"
    return [xp.reshape(-1), p0.reshape(-1)], []


def _run_plms(c, L, lib, ops):
    d, n, x, eps, s1 = _step_args(c)
    hist = [d[f"h{j + 1}"].cuda().reshape_as(x) for j in range(N.PLMS_NEED[c["mode"]])]
    call = lambda **kw: ops.plms_update(x, eps, hist, c["mode"], N.A_T, N.A_PREV, s1, N.CFG_SCALE, bool(c["cfg"]), **kw)
    xp, p0, e = call()
    xp2, p02, e2 = call()
    xp3, n1, n2 = call(want_e=False, want_pred_x0=False)
    torch.cuda.synchronize()
    assert torch.equal(xp, xp2) and torch.equal(p0, p02) and torch.equal(e, e2), "a second run differs"
    assert n1 is None and n2 is None and torch.equal(xp, xp3), "x_prev depends on the optional outputs"
    return [xp.reshape(-1), p0.reshape(-1), e.reshape(-1)], []


def _run_vq(c, L, lib, ops):
    d = N.data(c)
    m, edim, ldz = c["m"], c["edim"], c["ldz"]
    zc = torch.full((m, ldz), float("nan"))
    zc[:, :edim] = d["z"]
    z = _in(zc)                                              # NaN in the ld gap and in bands of rows around the operand
    idx, zq = ops.vq_lookup(z, d["cb"].cuda())
    idx2, zq2 = ops.vq_lookup(z, d["cb"].cuda())
    torch.cuda.synchronize()
    assert torch.equal(idx, idx2) and torch.equal(zq, zq2), "a second run differs"
    assert zq.shape == (m, ldz) and bool((_words(zq[:, edim:].contiguous()) == 0).all()), "columns of zq past edim stay zero"
    r = N.vq_report(c, idx, zq[:, :edim].contiguous())
    print(f"ops_variants {N.case_id(c)}: flips against fp64 {r[0] if r else '?'} (not near-ties: {r[1] if r else '?'}; gate 2 / 0)")
    return [idx, zq[:, :edim].contiguous()], []


def _run_gcn(c, L, lib, ops):
    d = N.data(c)
    n_obj, n_tri, h = c["n_obj"], c["n_tri"], c["h"]
    obj, pred, edges = d["obj"].cuda(), d["pred"].cuda(), d["edges"].cuda()
    # ld_t = off_o + h + pad: NaN in the skipped column, the gap and bands of rows around the operand
    nt = _in(d["nt"][:, :2 * h + 1], d["nt"].shape[1])
    ops.check_index_errors()
    gather = ops.gcn_gather_cat(obj, pred, edges)
    pooled = ops.gcn_segment_mean(nt, edges, n_obj, h, h + 1)
    csr = ops.gcn_csr(edges, n_obj)
    csr2 = ops.gcn_csr(edges, n_obj)
    pooled_csr = ops.gcn_segment_mean_csr(nt, csr, n_obj, h, h + 1)
    torch.cuda.synchronize()
    ops.check_index_errors()
    assert csr.numel() == 3 * n_obj + 1 + 2 * n_tri == lib.cs_gcn_csr_ints(n_obj, n_tri) and lib.cs_gcn_csr_ints(0, n_tri) == 0
    canon = N.gcn_canon_from_csr(csr, n_obj, n_tri)
    assert torch.equal(canon, N.gcn_canon_from_csr(csr2, n_obj, n_tri)), "a second build differs in content"
    return [gather, pooled, canon, pooled_csr], []


def _run_embedding(c, L, lib, ops):
    d = N.data(c)
    buf, o = _out(c["n"], c["dim"], c["ldo"])
    ops.embedding(d["table"].cuda(), d["idx"].cuda(), out=o)
    torch.cuda.synchronize()
    ops.check_index_errors()
    return [o], [(buf, o)]


def _run_log_softmax(c, L, lib, ops):
    m, cc = c["m"], c["c"]
    ldx, ldy = cc + c["pad"], cc + (c["pad"] + 2 if c["pad"] else 0)
    x = _in(N.data(c)["x"], ldx)
    buf, y = _out(m, cc, ldy)
    _ok(lib.cs_log_softmax(x.data_ptr(), y.data_ptr(), m, cc, ldx, ldy, _stream()), "cs_log_softmax")
    if c["pad"] == 0:
        assert torch.equal(_words(ops.log_softmax(x)), _words(y.contiguous())), "ops.log_softmax != the entry"
    return [y], [(buf, y)]


def _run_rowstats(c, L, lib, ops):
    n, a = ops.weight_rowstats([m.cuda() for m in N.data(c)["mats"]])
    return [torch.tensor([n], dtype=torch.float32), torch.tensor([a], dtype=torch.float32)], []


def _run_absmax(c, L, lib, ops):
    d = N.data(c)
    buf, slot = _out(1, 1)
    slot.fill_(d["slot0"])
    keep = []
    for k in ("x", "x2", "x3"):
        if k in d:
            x = torch.full((64 + c["n"] + 64,), float("nan"), device="cuda")     # NaN around the tensor: a read outside it shows
            x[64:64 + c["n"]] = d[k].cuda()
            keep.append(x)
            _ok(lib.cs_absmax(x[64:].data_ptr(), c["n"], slot.data_ptr(), _stream()), "cs_absmax")
    torch.cuda.synchronize()
    return [slot.reshape(1)], [(buf, slot)]


def _run_tapsum27(c, L, lib, ops):
    d = N.data(c)
    D, H, W = c["vol"]
    cout, M = c["cout"], c["nb"] * D * H * W
    ldy, ldo = 27 * cout + c["ypad"], cout + c["opad"]
    y = _in(d["y"], ldy)
    bias = d["bias"].cuda() if d["bias"] is not None else None
    runs = []
    for _ in range(2):
        buf, o = _out(M, cout, ldo)
        _ok(lib.cs_tapsum27(y.data_ptr(), bias.data_ptr() if bias is not None else None, o.data_ptr(), c["nb"], D, H, W, cout, ldy, ldo,
                            _stream()), "cs_tapsum27")
        runs.append((buf, o))
    torch.cuda.synchronize()
    assert torch.equal(_words(runs[0][1].contiguous()), _words(runs[1][1].contiguous())), "a second run differs"
    return [runs[0][1]], runs


def _run_pack_tapcol(c, L, lib, ops):
    cout, cin, ncolp = c["cout"], c["cin"], c["ncolp"]
    kg = ((cin + 15) // 16) * 2
    w = N.data(c)["w"].cuda().reshape(cout, cin, 3, 3, 3).contiguous()
    (hb, hi), (lb, lo) = _out(1, kg * ncolp * 8, dtype=torch.float16), _out(1, kg * ncolp * 8, dtype=torch.float16)
    _ok(lib.cs_pack_weight_f16x3_tapcol(w.data_ptr(), hi.data_ptr(), lo.data_ptr(), cout, cin, ncolp, c["scale"], _stream()), "tapcol")
    return [hi.reshape(kg, ncolp, 8), lo.reshape(kg, ncolp, 8)], [(hb, hi), (lb, lo)]


def _run_chamfer(c, L, lib, ops):
    d = N.data(c)
    b, n, m = c["b"], c["n"], c["m"]
    a, t = _in(d["a"].reshape(1, -1)), _in(d["b"].reshape(1, -1))
    (db, dist), (ib, idx) = _out(b, n), _out(b, n, dtype=torch.int32)
    _ok(lib.cs_chamfer_nm_distance(a.data_ptr(), t.data_ptr(), dist.data_ptr(), idx.data_ptr(), b, n, m, _stream()), "chamfer")
    return [dist, idx], [(db, dist), (ib, idx)]


def _run_synth_fill(c, L, lib, ops):
    buf, o = _out(1, c["n"])
    _ok(lib.cs_synth_fill(o.data_ptr(), c["n"], c["base"], c["scale"], c["offset"], _stream()), "cs_synth_fill")
    return [o.reshape(-1)], [(buf, o)]


@pytest.mark.parametrize("c", N.CASES, ids=N.case_id)
def test_case(c):
    L, lib, ops = _mods()
    outs, guards = globals()["_run_" + c.op](c, L, lib, ops)
    torch.cuda.synchronize()
    ratio = N.worst_ratio(outs, c)
    kinds = {k for _, k, _, _ in N.reference(c)}
    if kinds & {"E", "norm"}:
        emu = N.worst_ratio(N.emulate(c), c)
        print(f"ops_variants {N.case_id(c)}: worst ratio to the gate {ratio:.3f}   (cpu fp32 {emu:.3f})")
    else:
        print(f"ops_variants {N.case_id(c)}: {'exact' if ratio == 0.0 else 'DIFFERS'}")
    assert ratio <= 1.0, (N.case_id(c), ratio)
    if c.op in ("ddim", "plms"):
        # IEEE operations only, no contraction: the numpy fp32 evaluation of the source's expression is the kernel's, bit for bit
        for got, emu_t in zip(outs, N.emulate(c)):
            assert torch.equal(_words(got.cpu()), _words(emu_t)), (N.case_id(c), "differs from the fp32 operation sequence")
    for buf, v in guards:
        assert _untouched(buf, v), N.case_id(c)


def test_measured_k_of_the_transcendental_ops():
    """the kernel's own worst |out - fp64| / (2^-24 S) over each op's cases, beside the k its gate was set to from the CPU's fp32
    evaluation: printed and recorded, never used to set the gate"""
    L, lib, ops = _mods()
    for op, k in (("geglu", N.K_GEGLU), ("ts_embedding", N.K_TSEMB), ("log_softmax", N.K_LSM)):
        worst = 0.0
        for c in N.BY_OP[op]:
            outs, _ = globals()["_run_" + op](c, L, lib, ops)
            torch.cuda.synchronize()
            worst = max(worst, k * N.worst_ratio(outs, c))
        print(f"ops_variants {op}: kernel worst ratio {worst:.2f} x 2^-24 S, cpu fp32 {N.measured_k(op):.2f}, k = {k}")
        assert worst <= k


def test_layout_copy_of_256_sweeps():
    """256 * 8192 * 256 + 3 elements through both layout kernels with c = cpad = ldx = 1, where each is the identity: every
    thread of the capped grid makes 256 passes and three make one more.  An identity copy shows only that the loop covers every
    element once, at every pass; it cannot show an error in how a large flat index is split into sample, position and channel --
    that split is checked by the table's cases (c = 1, 3, 5, prime extents, one sweep and three elements), whose indices stay
    below 2^22.  Two tensors of 2 GiB: the one test here beyond the 70 MB of the table."""
    L, lib, ops = _mods()
    n = 256 * 8192 * 256 + 3
    x = torch.arange(n, dtype=torch.int32, device="cuda").view(torch.float32)
    for fn in (lib.cs_nchw_to_ndhwc, lib.cs_ndhwc_to_nchw):
        y = torch.zeros(n, dtype=torch.float32, device="cuda")
        _ok(fn(x.data_ptr(), y.data_ptr(), 1, 1, n, 1, _stream()), "layout")
        torch.cuda.synchronize()
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
        del y


# ---- (4) the argument rules ------------------------------------------------------------------------------------------------
def test_rejections_return_einval_and_write_nothing():
    L, lib, ops = _mods()
    buf, o = _out(64, 64)
    x = torch.randn(64 * 64 + 8, device="cuda")
    X, O, S = x.data_ptr(), o.data_ptr(), _stream()
    calls = {
        "geglu h % 4": lambda: lib.cs_geglu(X, O, 3, 6, 12, 8, S),
        "geglu ldx < 2h": lambda: lib.cs_geglu(X, O, 3, 8, 12, 8, S),
        "geglu ldo < h": lambda: lib.cs_geglu(X, O, 3, 8, 16, 4, S),
        "geglu ldx % 4": lambda: lib.cs_geglu(X, O, 3, 8, 18, 8, S),
        "geglu misaligned x": lambda: lib.cs_geglu(X + 4, O, 3, 8, 16, 8, S),
        "geglu misaligned out": lambda: lib.cs_geglu(X, O + 4, 3, 8, 16, 8, S),
        "copy_rows c % 4": lambda: lib.cs_copy_rows(X, O, 3, 6, 8, 8, S),
        "copy_rows lds < c": lambda: lib.cs_copy_rows(X, O, 3, 8, 4, 8, S),
        "copy_rows ldd < c": lambda: lib.cs_copy_rows(X, O, 3, 8, 8, 4, S),
        "copy_rows ldd % 4": lambda: lib.cs_copy_rows(X, O, 3, 8, 8, 10, S),
        "copy_rows misaligned src": lambda: lib.cs_copy_rows(X + 4, O, 3, 8, 8, 8, S),
        "copy_rows misaligned dst": lambda: lib.cs_copy_rows(X, O + 4, 3, 8, 8, 8, S),
        "add_rowvec c % 4": lambda: lib.cs_add_rowvec(O, X, 3, 6, 8, 8, 1, S),
        "add_rowvec ldx < c": lambda: lib.cs_add_rowvec(O, X, 3, 8, 4, 8, 1, S),
        "add_rowvec ldv < c": lambda: lib.cs_add_rowvec(O, X, 3, 8, 8, 4, 1, S),
        "add_rowvec rows 0": lambda: lib.cs_add_rowvec(O, X, 3, 8, 8, 8, 0, S),
        "add_rowvec misaligned x": lambda: lib.cs_add_rowvec(O + 4, X, 3, 8, 8, 8, 1, S),
        "add_rowvec misaligned v": lambda: lib.cs_add_rowvec(O, X + 4, 3, 8, 8, 8, 1, S),
        "nchw_to_ndhwc cpad < c": lambda: lib.cs_nchw_to_ndhwc(X, O, 2, 3, 5, 2, S),
        "ndhwc_to_nchw ldx < c": lambda: lib.cs_ndhwc_to_nchw(X, O, 2, 3, 5, 2, S),
        "log_softmax ldx < c": lambda: lib.cs_log_softmax(X, O, 3, 8, 4, 8, S),
        "log_softmax ldy < c": lambda: lib.cs_log_softmax(X, O, 3, 8, 8, 4, S),
        "embedding ldo < dim": lambda: lib.cs_embedding(X, X, O, 3, 8, 4, 4, None, S),
        "vq edim 4": lambda: lib.cs_vq_argmin_lookup(X, X, O, O, 3, 7, 4, 4, 4, S),
        "vq ldz < edim": lambda: lib.cs_vq_argmin_lookup(X, X, O, O, 3, 7, 3, 2, 4, S),
        "vq 10241 codes": lambda: lib.cs_vq_argmin_lookup(X, X, O, O, 3, 10241, 3, 4, 4, S),
        "segment_mean ld_t < off_o + h": lambda: lib.cs_gcn_segment_mean(X, X, O, 2, 3, 4, 5, 8, None, S),
        "tapsum27 cout 5": lambda: lib.cs_tapsum27(X, None, O, 1, 2, 2, 2, 5, 135, 5, S),
        "tapsum27 ldy < 27 cout": lambda: lib.cs_tapsum27(X, None, O, 1, 2, 2, 2, 2, 53, 2, S),
        "tapsum27 ldo < cout": lambda: lib.cs_tapsum27(X, None, O, 1, 2, 2, 2, 2, 54, 1, S),
        "tapcol ncolp < 27 cout": lambda: lib.cs_pack_weight_f16x3_tapcol(X, O, O, 2, 3, 28, 1.0, S),
        "tapcol ncolp % 4": lambda: lib.cs_pack_weight_f16x3_tapcol(X, O, O, 1, 3, 30, 1.0, S),
        "tapcol scale 0": lambda: lib.cs_pack_weight_f16x3_tapcol(X, O, O, 1, 3, 28, 0.0, S),
        "ts_embedding dim 1": lambda: lib.cs_timestep_embedding(X, O, 3, 1, 10000.0, S),
        "ddim a_t 0": lambda: lib.cs_ddim_cfg_update(X, X, None, O, None, 1, 8, 0.0, 0.5, 0.0, 1.0, 1.0, 0, S),
        "plms mode 5": lambda: lib.cs_plms_update(X, X, X, X, X, None, O, None, 1, 8, 5, 0.5, 0.5, 0.7, 1.0, 0, S),
        "plms AB3 without h2": lambda: lib.cs_plms_update(X, X, X, None, None, None, O, None, 1, 8, 2, 0.5, 0.5, 0.7, 1.0, 0, S),
        "absmax n 0": lambda: lib.cs_absmax(X, 0, O, S),
    }
    got = {k: f() for k, f in calls.items()}
    torch.cuda.synchronize()
    assert got == {k: L.CS_EINVAL for k in calls}, {k: v for k, v in got.items() if v != L.CS_EINVAL}
    assert _pristine(buf)
    xv = x[:64 * 12].view(64, 12)
    for what, f in (("geglu h % 4", lambda: ops.geglu(xv, out=o[:, :6])), ("geglu x offset by a float", lambda: ops.geglu(x[1:193].view(12, 16), out=o[:12, :8])),
                    ("add_rowvec c % 4", lambda: ops.add_rowvec_(o[:, :6], xv[:, :6], 1)),
                    ("add_rowvec x offset by a float", lambda: ops.add_rowvec_(o[:, 1:9], xv[:, :8], 1))):
        with pytest.raises(L.CsError):
            f()
    torch.cuda.synchronize()
    assert _pristine(buf)


# ---- (5) the index guards in the kernel source -------------------------------------------------------------------------------
def test_index_guards_zero_or_skip_and_raise_once():
    L, lib, ops = _mods()
    g = torch.Generator().manual_seed(11)
    n_obj, n_tri, h, n_rows = 5, 9, 6, 7
    obj, pred = torch.randn(n_obj, h, generator=g), torch.randn(n_tri, h + 1, generator=g)
    nt = torch.randn(n_tri, 2 * h, generator=g)
    table = torch.randn(n_rows, h, generator=g)
    edges = torch.randint(0, n_obj, (n_tri, 2), generator=g)
    bad = edges.clone()
    bad[2, 0], bad[6, 1] = n_obj, -1
    idx, bad_idx = torch.tensor([0, 3, 6, 3, 1]), torch.tensor([0, n_rows, 6, -1, 1])
    word = ops.index_err_word()
    try:
        ops.check_index_errors()
        good = (ops.gcn_gather_cat(obj.cuda(), pred.cuda(), edges.cuda()), ops.gcn_segment_mean(nt.cuda(), edges.cuda(), n_obj, h, h),
                ops.embedding(table.cuda(), idx.cuda()))
        ops.check_index_errors()                           # nothing to report
        # gather: the columns of the bad endpoint are zero, everything else is unchanged
        got = ops.gcn_gather_cat(obj.cuda(), pred.cuda(), bad.cuda())
        with pytest.raises(IndexError):
            ops.check_index_errors()
        assert int(word.item()) == 0
        ops.check_index_errors()                           # raised once
        want = good[0].clone()
        want[2, :h] = 0.0
        want[6, h + h + 1:] = 0.0
        assert torch.equal(got, want)
        # segment mean: the bad endpoint is skipped (sum and count), its edge's other endpoint still counts
        got = ops.gcn_segment_mean(nt.cuda(), bad.cuda(), n_obj, h, h)
        with pytest.raises(IndexError):
            ops.check_index_errors()
        lists = [([t for t in range(n_tri) if int(bad[t, 0]) == o], [t for t in range(n_tri) if int(bad[t, 1]) == o]) for o in range(n_obj)]
        assert torch.equal(got.cpu(), N.gcn_pool_lists(nt, lists, h, h))
        assert torch.equal(good[1].cpu(), N.gcn_pool_lists(nt, N.gcn_lists(edges, n_obj), h, h))
        # embedding: the rows of the bad indices are zero
        got = ops.embedding(table.cuda(), bad_idx.cuda())
        with pytest.raises(IndexError):
            ops.check_index_errors()
        want = good[2].clone()
        want[1] = 0.0
        want[3] = 0.0
        assert torch.equal(got, want) and int(word.item()) == 0
    finally:
        word.zero_()
        torch.cuda.synchronize()


# ---- the consumer of the absmax slot ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_a_nan_or_inf_in_the_bounded_operand_raises_the_overflow_flag(poison):
    """cs_absmax leaves 3.0e38 for a tensor with a NaN or an inf -- a bound no operand scale can honour -- so the F16X3 GEMM
    that reads the slot reports the operand through the overflow flag and the host falls back to fp32"""
    L, lib, ops = _mods()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(512, 448, generator=g).cuda()
    w = (torch.randn(448, 448, generator=g) * 448 ** -0.5).cuda()
    pw = ops.pack_weight(w, None, math=L.MATH_F16X3)
    ops.clear_status()
    try:
        slot = torch.zeros(1, device="cuda")
        y = ops.conv_gemm(x, pw, math=L.MATH_F16X3, x_bound=ops.absmax_bound(x, slot))
        torch.cuda.synchronize()
        ops.check_overflow()
        assert float(slot.item()) == float(x.abs().max()) and torch.isfinite(y).all()
        x[300, 17] = poison
        slot = torch.zeros(1, device="cuda")
        ops.conv_gemm(x, pw, math=L.MATH_F16X3, x_bound=ops.absmax_bound(x, slot))
        torch.cuda.synchronize()
        assert float(slot.item()) == N.CLAMP
        with pytest.raises(L.CsOverflowError):
            ops.check_overflow()
    finally:
        ops.clear_status()
        torch.cuda.synchronize()
