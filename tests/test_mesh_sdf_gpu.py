"""mesh_to_sdf on the MI355X against the fp64 brute force of tests/_mesh_sdf_ref.py: closed and open meshes, the winding field,
the shapes at which the kernels change path (chunk and slice boundaries, register-blocking tails, ragged batches),
bit-equality, degenerate and hostile input, orientation, the round trip through sdf_to_mesh, normalisation and truncation,
and the chain into the VQ-VAE.

Gates: 4 x the largest error measured on the MI355X against the fp64 brute force, rounded up to one digit (DESIGN.md
section 8m lists the figures per case).
  DIST_GATE       max |d - d_ref| over every case of this file: 1.49e-7 (the box at n = 16; the others 3.8e-8 .. 1.3e-7)
                  -> 5.97e-7 -> 6e-7
  WIND_GATE       max |w - w_ref| over the closed meshes and the open hemisphere, all nodes: 1.40e-6 (the box at n = 16;
                  the icospheres 1.2e-7 .. 1.3e-6) -> 5.6e-6 -> 6e-6
  WIND_GATE_SOUP  the same over the random triangle soups of the shape tests, all nodes: 1.28e-5 (257 faces at n = 33)
                  -> 5.1e-5 -> 6e-5.  Their triangles are up to 0.5 long and nodes come within 1e-3 of one: the denominator
                  of the solid-angle formula is then a sum of terms of size D^3 that cancels to about d L^2, and fp32 leaves
                  eps D / d ~ 1.5e-5 in w.  The sign only needs |w| against 0.5.
"""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import _mesh_sdf_ref as R

pytestmark = pytest.mark.gpu

DIST_GATE = 6e-7
WIND_GATE = 6e-6
WIND_GATE_SOUP = 6e-5
NEAR = 1e-3            # nodes nearer the surface than this are compared by magnitude only

_REF = {}
_GOT = {}


def _t(v, f, idt=torch.int64):
    return torch.from_numpy(np.asarray(v, np.float32)), torch.from_numpy(np.asarray(f)).to(idt)


def _mesh(name):
    if name.startswith("ico"):
        return R.icosphere(int(name[3:]))
    if name.startswith("soup"):
        return R.random_soup(int(name[4:]), seed=int(name[4:]))
    return {"box": R.box, "torus": R.torus, "hemi": R.hemisphere}[name]()


def _ref(name, n):
    """(signed, distance, winding) of the fp32-rounded mesh in fp64, computed once per (mesh, n)"""
    if (name, n) not in _REF:
        v, f = _mesh(name)
        _REF[(name, n)] = R.sdf(R.grid_points(n), np.asarray(v, np.float32).astype(np.float64)[f])
    return _REF[(name, n)]


def _got(name, n):
    """(sdf, winding) of the device, flattened fp64 numpy, computed once per (mesh, n)"""
    from commonscenes_amd.mesh_sdf import mesh_to_sdf
    if (name, n) not in _GOT:
        v, f = _t(*_mesh(name))
        s, w = mesh_to_sdf([v], [f], res=n, normalize=False, return_winding=True)
        assert tuple(s.shape) == (1, 1, n, n, n) and s.dtype == torch.float32 and s.is_cuda and w.shape == s.shape
        _GOT[(name, n)] = (s.cpu().double().numpy().ravel(), w.cpu().double().numpy().ravel())
    return _GOT[(name, n)]


def _check(tag, got_sdf, got_w, ref, closed, near_cap=None, wind_gate=WIND_GATE):
    sd_ref, d_ref, w_ref = ref
    e_d = np.abs(np.abs(got_sdf) - d_ref).max()
    e_w = np.abs(got_w - w_ref).max()
    far = d_ref >= NEAR
    if not closed:      # an open mesh has no sign where |w| sits on the level: leave out what the gate cannot tell apart
        far = far & (np.abs(np.abs(w_ref) - 0.5) > wind_gate)
    flips = int(((got_sdf < 0) != (sd_ref < 0))[far].sum())
    print(f"[{tag}] max |d - d_ref| {e_d:.3e}, max |w - w_ref| {e_w:.3e}, sign flips {flips} of {int(far.sum())}, "
          f"left out {int((~far).sum())} of {far.size}")
    assert e_d <= DIST_GATE
    assert e_w <= wind_gate
    assert flips == 0
    if near_cap is not None:
        assert (~far).sum() < near_cap * far.size


CLOSED = [("ico1", 16), ("ico2", 17), ("ico3", 9), ("box", 12), ("torus", 13)]


@pytest.mark.parametrize("name,n", CLOSED)
def test_closed_meshes_against_fp64(name, n):
    s, w = _got(name, n)
    _check(f"{name} n={n}", s, w, _ref(name, n), closed=True, near_cap=0.01)
    w_ref = _ref(name, n)[2]
    assert np.abs(w_ref - np.round(w_ref)).max() < 1e-9          # closed: the reference's own w is an integer


def test_unsigned_is_the_magnitude_of_signed():
    from commonscenes_amd.mesh_sdf import mesh_to_sdf
    v, f = _t(*_mesh("ico1"))
    u = mesh_to_sdf([v], [f], res=16, normalize=False, sign="unsigned")
    s = mesh_to_sdf([v], [f], res=16, normalize=False)
    assert torch.equal(u, s.abs()) and bool((s < 0).any()) and bool((u >= 0).all())


def test_open_hemisphere_winding_field():
    s, w = _got("hemi", 16)
    ref = _ref("hemi", 16)
    assert np.abs(np.abs(ref[2]) - 0.5).min() >= 1e-4 and np.abs(ref[2] - np.round(ref[2])).max() > 0.1
    sd_ref, d_ref, w_ref = ref
    far = d_ref >= NEAR
    assert np.array_equal((s < 0)[far], (sd_ref < 0)[far])        # every node off the surface: none is near the level
    _check("hemisphere n=16", s, w, ref, closed=False)


# chunk = 256 triangles; the plan cuts 513 faces (three chunks) in two slices and 512 in one
@pytest.mark.parametrize("faces", [1, 255, 256, 257, 512, 513])
def test_face_counts_either_side_of_chunk_and_slice_sizes(faces):
    from commonscenes_amd import mesh_sdf
    assert mesh_sdf.plan(512, 5)[0] == 1 and mesh_sdf.plan(513, 5)[0] == 2
    name = f"soup{faces}"
    s, w = _got(name, 5)
    _check(f"{name} n=5", s, w, _ref(name, 5), closed=False, wind_gate=WIND_GATE_SOUP)


@pytest.mark.parametrize("n", [2, 5, 33])
def test_grid_sizes_that_leave_a_register_blocking_tail(n):
    s, w = _got("soup257", n)
    _check(f"soup257 n={n}", s, w, _ref("soup257", n), closed=False, wind_gate=WIND_GATE_SOUP)


def _batch3():
    a, b, c = _t(*_mesh("ico1"), idt=torch.int32), _t(*_mesh("soup300")), _t(*_mesh("box"), idt=torch.int32)
    return [a[0], b[0], c[0]], [a[1], b[1], c[1]]


def test_ragged_batch_of_three():
    from commonscenes_amd.mesh_sdf import mesh_to_sdf
    vs, fs = _batch3()
    s, w, meta = mesh_to_sdf(vs, fs, res=16, normalize=False, return_winding=True, return_meta=True)
    assert tuple(s.shape) == (3, 1, 16, 16, 16) and meta["faces"] == [80, 300, 12]
    for i, (name, closed) in enumerate((("ico1", True), ("soup300", False), ("box", True))):
        _check(f"batch[{i}] {name}", s[i].cpu().double().numpy().ravel(), w[i].cpu().double().numpy().ravel(),
               _ref(name, 16), closed=closed, wind_gate=WIND_GATE if closed else WIND_GATE_SOUP)


def test_bit_equality_across_batch_position_and_runs():
    from commonscenes_amd.mesh_sdf import mesh_to_sdf
    vs, fs = _batch3()
    big = _t(*_mesh("ico3"))
    kw = dict(res=16, normalize=True, return_winding=True)
    alone = mesh_to_sdf([big[0]], [big[1]], **kw)
    first = mesh_to_sdf([big[0]] + vs, [big[1]] + fs, **kw)
    last = mesh_to_sdf(vs + [big[0]], fs + [big[1]], **kw)
    again = mesh_to_sdf(vs + [big[0]], fs + [big[1]], **kw)
    for k in range(2):
        assert torch.equal(alone[k][0], first[k][0]) and torch.equal(alone[k][0], last[k][3])
        assert torch.equal(last[k], again[k])
        for i in range(3):           # a batch against one call per mesh
            one = mesh_to_sdf([vs[i]], [fs[i]], **kw)
            assert torch.equal(one[k][0], last[k][i]) and torch.equal(one[k][0], first[k][1 + i])


def test_zero_area_triangles_change_nothing():
    from commonscenes_amd.mesh_sdf import mesh_to_sdf
    v, f = _mesh("ico2")
    v32 = np.asarray(v, np.float32)
    mids = 0.5 * (v32[f[:8, 0]].astype(np.float64) + v32[f[:8, 1]])            # on an edge: collinear with its ends
    v2 = np.concatenate([v32, mids.astype(np.float32)])
    extra = [[f[i, 0], len(v32) + i, f[i, 1]] for i in range(8)]              # collinear
    extra += [[f[i, 0], f[i, 0], f[i, 1]] for i in range(8, 16)]              # repeated vertex
    extra += [[f[i, 2], f[i, 2], f[i, 2]] for i in range(16, 20)]             # a point
    f2 = np.concatenate([f[:100], np.array(extra, dtype=np.int64), f[100:]])
    s, w = mesh_to_sdf(*[[x] for x in _t(v2, f2)], res=17, normalize=False, return_winding=True)
    clean_s, clean_w = _got("ico2", 17)
    s, w = s.cpu().double().numpy().ravel(), w.cpu().double().numpy().ravel()
    e = np.abs(s - clean_s).max()
    print(f"[degenerate] max |sdf - clean| {e:.3e}, max |w - clean| {np.abs(w - clean_w).max():.3e}")
    assert e <= DIST_GATE and np.abs(w - clean_w).max() <= WIND_GATE
    _check("ico2 + 20 zero-area n=17", s, w, _ref("ico2", 17), closed=True)


def test_doubled_mesh_has_winding_two_and_the_same_sdf():
    from commonscenes_amd.mesh_sdf import mesh_to_sdf
    v, f = _mesh("ico2")
    s, w = mesh_to_sdf(*[[x] for x in _t(v, np.concatenate([f, f]))], res=17, normalize=False, return_winding=True)
    clean_s, clean_w = _got("ico2", 17)
    assert np.array_equal(s.cpu().double().numpy().ravel(), clean_s)
    w = w.cpu().double().numpy().ravel()
    assert np.abs(w - 2 * clean_w).max() <= 2 * WIND_GATE and np.abs(np.round(w)).max() == 2


def test_bad_face_index_raises_and_names_the_mesh():
    from commonscenes_amd import lib as L
    from commonscenes_amd.mesh_sdf import mesh_to_sdf
    v, f = _t(*_mesh("ico1"))
    nv = v.shape[0]
    # the vertex buffer ends where its allocation ends: an id of nv or beyond has nothing behind it
    buf = torch.empty((4096 + nv) * 3, dtype=torch.float32, device="cuda")
    vt = buf[-nv * 3:].view(nv, 3)
    vt.copy_(v)
    for bad in (nv, -1, 2 ** 40, 2 ** 31):
        fb = f.clone()
        fb[7, 1] = bad
        with pytest.raises(L.CsError, match="mesh 1.*face index"):
            mesh_to_sdf([v, vt], [f, fb.cuda()], res=5, normalize=True)
        with pytest.raises(L.CsError, match="mesh 0.*face index"):
            mesh_to_sdf([vt], [fb.to(torch.int32) if abs(bad) < 2 ** 31 else fb], res=5, normalize=False)
    ok = mesh_to_sdf([v, vt], [f, f], res=5, normalize=False)          # the device still answers, and the same for both
    assert torch.equal(ok[0], ok[1]) and bool(torch.isfinite(ok).all())


def test_nan_vertex_raises():
    from commonscenes_amd import lib as L
    from commonscenes_amd.mesh_sdf import mesh_to_sdf
    v, f = _t(*_mesh("ico1"))
    for bad in (float("nan"), float("inf")):
        for normalize in (False, True):
            vb = v.clone()
            vb[5, 2] = bad
            with pytest.raises(L.CsError, match="mesh 0.*non-finite"):
                mesh_to_sdf([vb], [f], res=5, normalize=normalize)


def test_reversed_faces_give_the_same_grid():
    from commonscenes_amd.mesh_sdf import mesh_to_sdf
    for name, n in (("ico2", 17), ("torus", 13), ("hemi", 16)):
        v, f = _t(*_mesh(name))
        s, w = mesh_to_sdf([v], [f], res=n, normalize=False, return_winding=True)
        sr, wr = mesh_to_sdf([v], [f[:, [0, 2, 1]].contiguous()], res=n, normalize=False, return_winding=True)
        assert torch.equal(s, sr)                  # distance bit for bit, and the same signs
        assert torch.equal(w, -wr)


def _analytic(kind, p):
    if kind == "sphere":
        return np.linalg.norm(p - R.OFF, axis=1) - 0.62
    q = p - R.OFF
    return np.sqrt((np.sqrt(q[:, 0] ** 2 + q[:, 1] ** 2) - 0.6) ** 2 + q[:, 2] ** 2) - 0.3


@pytest.mark.parametrize("table", ["classic", "watertight"])
@pytest.mark.parametrize("kind", ["sphere", "torus"])
def test_round_trip_through_sdf_to_mesh(kind, table):
    """A marching-cubes triangle lies inside a cell the true surface crosses (diameter sqrt(3) h) and an SDF is 1-Lipschitz:
    the distance to the mesh differs from the analytic one by at most 2 sqrt(3) h at every node.  Derived, not measured."""
    from commonscenes_amd.mesh import sdf_to_mesh
    from commonscenes_amd.mesh_sdf import display_to_grid, mesh_to_sdf
    n = 32
    h = 2.0 / (n - 1)
    ana = _analytic(kind, R.grid_points(n))
    vol = torch.from_numpy(ana.astype(np.float32)).view(1, 1, n, n, n).cuda()
    m = sdf_to_mesh(vol, level=0.0, table=table)
    verts = display_to_grid(m.verts_list()[0], n, 1.0)
    s, w = mesh_to_sdf([verts], [m.faces_list()[0]], res=n, normalize=False, return_winding=True)
    s = s.cpu().double().numpy().ravel()
    err = np.abs(s - ana).max()
    bound = 2.0 * np.sqrt(3.0) * h
    clear = np.abs(ana) > bound
    inside = float(np.round(w.cpu().double().numpy().ravel()[ana < -bound]).mean())
    print(f"[round trip {kind}/{table}] F {m.faces_list()[0].shape[0]}, max |sdf - analytic| {err:.4f} (bound {bound:.4f}), "
          f"w inside {inside:+.0f}")
    assert err <= bound
    assert np.array_equal((s < 0)[clear], (ana < 0)[clear]) and (ana < -bound).any()


def test_normalize_recovers_shift_and_scale():
    from commonscenes_amd.mesh_sdf import get_normalize_mesh, mesh_to_sdf
    v, f = _mesh("ico2")
    unit, _, _ = R.get_normalize_mesh(np.asarray(v, np.float32).astype(np.float64), f)
    shift, scale = np.array([0.5, -0.25, 0.75]), 2.0
    uv, ff = _t(unit, f)
    cv = torch.from_numpy((unit * scale + shift).astype(np.float32))
    base = mesh_to_sdf([uv], [ff], res=16, normalize=False)
    got, meta = mesh_to_sdf([cv], [ff], res=16, normalize=True, return_meta=True)
    cen, m = meta["centroid"][0].cpu().numpy(), float(meta["scale"][0])
    cen_ref, m_ref = R.centroid_scale(cv.double().numpy(), f)
    e = float((got - base).abs().max())
    print(f"[normalize] max |sdf - unit copy| {e:.3e}, centroid err {np.abs(cen - cen_ref).max():.2e}, scale err "
          f"{abs(m - m_ref):.2e}")
    assert e <= DIST_GATE
    assert np.abs(cen - cen_ref).max() <= 1e-12 and abs(m - m_ref) <= 1e-12        # fp64 sums of a few hundred terms
    assert np.abs(cen - shift).max() <= 1e-6 and abs(m - scale) <= 1e-6            # the copy's fp32 rounding
    nv, c2, m2 = get_normalize_mesh(cv, ff)
    assert np.abs(c2.cpu().numpy() - cen_ref).max() <= 1e-12 and abs(float(m2) - m_ref) <= 1e-12
    assert abs(float(nv.double().norm(dim=1).max()) - 1.0) <= 1e-6
    bv, bf = _t(*R.box())
    _, cb, mb = get_normalize_mesh(bv * 3.0 + 2.0, bf)
    assert np.abs(cb.cpu().numpy() - (R.OFF * 3.0 + 2.0)).max() <= 1e-6
    assert abs(float(mb) - 3.0 * np.linalg.norm(R.BOX_HALF)) <= 1e-6


def test_trunc_is_a_clamp_bit_for_bit():
    from commonscenes_amd.mesh_sdf import mesh_to_sdf
    v, f = _t(*_mesh("ico2"))
    full = mesh_to_sdf([v], [f], res=17)
    cut = mesh_to_sdf([v], [f], res=17, trunc=0.2)
    assert torch.equal(cut, full.clamp(-0.2, 0.2)) and float(cut.max()) == float(np.float32(0.2))
    assert float(cut.min()) == -float(np.float32(0.2))


def test_accepts_meshes_and_cpu_tensors():
    from commonscenes_amd.mesh import Meshes
    from commonscenes_amd.mesh_sdf import mesh_to_sdf
    v, f = _t(*_mesh("ico1"))
    a = mesh_to_sdf([v], [f], res=9)
    b = mesh_to_sdf(Meshes([v.cuda()], [f.cuda()]), res=9)
    assert torch.equal(a, b)


def test_chain_into_the_vqvae():
    """plumbing only: synthetic weights carry no quality claim"""
    from commonscenes_amd import synth
    from commonscenes_amd.mesh_sdf import mesh_to_sdf
    from commonscenes_amd.vqvae import VQVAE, vqvae_encoder_param_shapes, vqvae_param_shapes
    from oracle.ref_torch import VQ_FULL
    dd = dict(VQ_FULL, in_channels=1, double_z=False)
    table = OrderedDict(list(vqvae_encoder_param_shapes(dd, 8192, 3).items()) +
                        list(vqvae_param_shapes(dd, 8192, 3).items()))
    vq = VQVAE(dd, 8192, 3, device="cuda").load_state_dict(synth.synth_state_dict(table, device="cuda")).set_math("f16x3")
    v, f = _t(*R.box())
    x = mesh_to_sdf([v], [f], res=64, trunc=0.2)
    assert tuple(x.shape) == (1, 1, 64, 64, 64) and bool((x < 0).any())
    h = vq.encode_no_quant(x)
    out = vq.decode_no_quant(h)
    out = out[0] if isinstance(out, (tuple, list)) else out
    assert tuple(out.shape) == (1, 1, 64, 64, 64) and bool(torch.isfinite(out).all()) and bool(torch.isfinite(h).all())
