"""Shape completion, host side (no GPU): get_partial_shape against the reference's masks (tests/golden/shape_comp.npz,
tools/make_goldens.py --only shape_comp), the C entry's export and argument checks, what ops.masked_blend refuses before it
touches a device, and the sampler options that stay unbuilt."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import GOLDEN


def _volume_chk(v):
    """{sum, sum of magnitudes, position-weighted sum} in fp64, as the fixture's generator takes them"""
    d = v.detach().double().cpu().flatten()
    w = (torch.arange(d.numel(), dtype=torch.float64) % 251.0) + 1.0
    return np.array([float(d.sum()), float(d.abs().sum()), float((d * w).sum())], np.float64)


def _chk_ok(v, want):
    """the summation order is the host's own: 1e-12 of the sum of magnitudes (x 251 for the weighted sum)"""
    got = _volume_chk(v)
    tol = 1e-12 * abs(want[1]) * np.array([1.0, 1.0, 251.0])
    return bool((np.abs(got - want) <= tol).all())


def test_get_partial_shape_equals_the_reference_exactly():
    from commonscenes_amd import synth
    from commonscenes_amd.demo_util import get_partial_shape
    g = np.load(GOLDEN / "shape_comp.npz")
    vol = torch.cat([synth.sdf_volume(0), synth.sdf_volume(1)], dim=0)
    assert _chk_ok(vol, g["vol_chk"])
    z = torch.zeros(2, 3, 16, 16, 16)
    boxes = g["boxes"]
    assert len(boxes) >= 6
    empties = 0
    for i, b in enumerate(boxes):
        xyz = {"x": tuple(b[0]), "y": tuple(b[1]), "z": tuple(b[2])}
        ret = get_partial_shape(vol, xyz, z=z)
        assert sorted(ret) == ["shape_mask", "shape_missing", "shape_part", "z_mask"]
        sm, zm = ret["shape_mask"], ret["z_mask"]
        assert sm.dtype == torch.bool and sm.shape == (2, 1, 64, 64, 64)
        assert zm.dtype == torch.float32 and zm.shape == (2, 1, 16, 16, 16)
        assert g[f"shape_mask_{i}"].dtype == np.bool_ and g[f"z_mask_{i}"].dtype == np.float32
        assert torch.equal(sm, torch.from_numpy(g[f"shape_mask_{i}"])), i
        assert torch.equal(zm, torch.from_numpy(g[f"z_mask_{i}"])), i
        part, missing = ret["shape_part"], ret["shape_missing"]
        assert part.dtype == torch.float32 and part.shape == vol.shape and missing.shape == vol.shape
        assert _chk_ok(part, g[f"part_chk_{i}"]) and _chk_ok(missing, g[f"missing_chk_{i}"]), i
        # what the two volumes are: the input inside / outside the box, 0.2 elsewhere
        assert torch.equal(part[sm], vol[sm]) and bool((part[~sm] == np.float32(0.2)).all())
        assert torch.equal(missing[~sm], vol[~sm]) and bool((missing[sm] == np.float32(0.2)).all())
        empties += int(not sm.any())
    assert empties >= 2                                   # the empty and the inverted range
    # the ranges are truncated at each grid's own resolution: 0.3 -> 41 of 64 but 10 of 16
    sm, zm = torch.from_numpy(g["shape_mask_2"]), torch.from_numpy(g["z_mask_2"])
    assert bool(sm[0, 0, 41:, 14:41, :14].all()) and not bool(sm[0, 0, :41].any()) and not bool(sm[0, 0, :, :14].any())
    assert bool((zm[0, 0, 10:, 3:10, :3] == 1).all()) and float(zm.sum()) == 2 * 6 * 7 * 3
    # without a latent there is no z_mask; the input is left alone
    before = vol.clone()
    ret = get_partial_shape(vol, {"x": (-1, 0), "y": (-1, 1), "z": (-1, 1)})
    assert "z_mask" not in ret and torch.equal(vol, before)
    assert float(ret["shape_mask"].float().mean()) == 0.5
    with pytest.raises(ValueError):
        get_partial_shape(vol[0], {"x": (-1, 0), "y": (-1, 1), "z": (-1, 1)})


def _aligned(n_floats):
    buf = (C.c_float * (n_floats + 16))()
    base = C.addressof(buf)
    return buf, base + (-base) % 64


def test_library_exports_the_blend_entry_and_rejects_bad_arguments_without_a_device_call():
    from commonscenes_amd import build, lib
    assert "cs_complete.hip" in build.SOURCES
    dll = lib.load()
    assert "cs_ddim_masked_blend" in lib.SIGNATURES and hasattr(dll, "cs_ddim_masked_blend")
    keep, p = _aligned(64)            # a host address: every call below must return before any launch
    names = ("x0", "noise", "mask", "img", "out", "t", "sa", "s1", "src", "msrc", "rows", "channels", "inner",
             "mask_channels", "T", "x0_rows", "mask_rows", "stream")
    good = dict(x0=p, noise=p, mask=p, img=p, out=p, t=p, sa=p, s1=p, src=None, msrc=None, rows=2, channels=3, inner=8,
                mask_channels=1, T=10, x0_rows=2, mask_rows=2, stream=None)
    call = lambda **kw: dll.cs_ddim_masked_blend(*[{**good, **kw}[k] for k in names])
    for bad in (dict(x0=None), dict(noise=None), dict(mask=None), dict(img=None), dict(out=None), dict(t=None), dict(sa=None),
                dict(s1=None), dict(rows=0), dict(rows=-1), dict(channels=0), dict(inner=0), dict(inner=-8), dict(T=0),
                dict(x0_rows=0), dict(mask_rows=0), dict(mask_channels=2), dict(mask_channels=0),
                dict(x0_rows=1), dict(mask_rows=1),          # an identity map over too few source rows
                dict(rows=2 ** 31, x0_rows=2 ** 31, mask_rows=2 ** 31)):          # more workgroups than a grid holds
        assert call(**bad) == lib.CS_EINVAL, bad
    txt = (GOLDEN.parent.parent / "include" / "commonscenes_hip.h").read_text()
    assert "int cs_ddim_masked_blend(" in txt
    del keep


def test_ops_masked_blend_rejects_on_the_host():
    from commonscenes_amd import lib, ops
    img, noise = torch.zeros(2, 3, 2, 2, 2), torch.zeros(2, 3, 2, 2, 2)
    x0, m1 = torch.zeros(2, 3, 2, 2, 2), torch.ones(2, 1, 2, 2, 2)
    t = torch.tensor([0, 3], dtype=torch.long)
    sa, s1 = torch.ones(4), torch.ones(4)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    with pytest.raises(lib.CsError, match="HIP device"):                      # well-formed, but CPU tensors
        ops.masked_blend(img, x0, m1, noise, t, sa, s1)
    with pytest.raises(lib.CsError, match="HIP device"):
        ops.masked_blend(img, x0[:1], m1[:1], noise, t, sa, s1, src=i32(0, 0), msrc=i32(0, 0))
    for tt in (torch.tensor([0, 4]), torch.tensor([-1, 0])):                  # a timestep outside [0, T)
        with pytest.raises(lib.CsError, match="timestep outside"):
            ops.masked_blend(img, x0, m1, noise, tt, sa, s1)
    for kw, what in ((dict(src=i32(0, 2)), "src outside"), (dict(msrc=i32(-1, 0)), "msrc outside"),
                     (dict(src=i32(0)), "one int32 per output row"), (dict(msrc=torch.tensor([0, 1])), "msrc: expected")):
        with pytest.raises(lib.CsError, match=what):
            ops.masked_blend(img, x0, m1, noise, t, sa, s1, **kw)
    with pytest.raises(lib.CsError, match="neither 1 nor 3"):                 # a 2-channel mask for 3 channels
        ops.masked_blend(img, x0, torch.ones(2, 2, 2, 2, 2), noise, t, sa, s1)
    # rows that do not match
    with pytest.raises(lib.CsError, match="one .* row per timestep"):
        ops.masked_blend(img, x0, m1, noise, torch.tensor([0, 1, 2]), sa, s1)
    with pytest.raises(lib.CsError, match="one .* row per timestep"):
        ops.masked_blend(img, x0, m1, noise[:1], t, sa, s1)
    with pytest.raises(lib.CsError, match="without a src map"):
        ops.masked_blend(img, x0[:1], m1, noise, t, sa, s1)
    with pytest.raises(lib.CsError, match="without a msrc map"):
        ops.masked_blend(img, x0, m1[:1], noise, t, sa, s1)
    with pytest.raises(lib.CsError, match="row shape"):
        ops.masked_blend(img, torch.zeros(2, 3, 2, 2, 3), m1, noise, t, sa, s1)
    with pytest.raises(lib.CsError, match="voxel shape"):
        ops.masked_blend(img, x0, torch.ones(2, 1, 2, 2, 3), noise, t, sa, s1)
    with pytest.raises(lib.CsError, match="empty rows"):
        e = torch.zeros(2, 3, 0)
        ops.masked_blend(e, e, torch.zeros(2, 1, 0), e, t, sa, s1)
    with pytest.raises(lib.CsError, match="t: expected"):
        ops.masked_blend(img, x0, m1, noise, t.int(), sa, s1)


class _HostModel:
    """what a sampler reads from its model before any device work"""
    num_timesteps = 1000
    device = torch.device("cpu")
    alphas_cumprod = torch.linspace(0.999, 0.01, 1000)


def test_mask_without_x0_fails_like_the_reference_and_the_open_options_still_raise():
    from commonscenes_amd.ddim import DDIMSampler
    from commonscenes_amd.plms import PLMSSampler
    m = torch.ones(1, 1, 16, 16, 16)
    z = torch.zeros(1, 3, 16, 16, 16)
    kw = dict(S=6, batch_size=1, shape=(3, 16, 16, 16), verbose=False)
    with pytest.raises(AssertionError):                                       # ddim.py:159 `assert x0 is not None`
        DDIMSampler(_HostModel()).sample(mask=m, **kw)
    for bad in (dict(quantize_x0=True), dict(temperature=0.5), dict(noise_dropout=0.1), dict(mm_cls_free=True),
                dict(score_corrector=object())):
        with pytest.raises(NotImplementedError):
            DDIMSampler(_HostModel()).sample(mask=m, x0=z, **kw, **bad)
        with pytest.raises(NotImplementedError):
            DDIMSampler(_HostModel()).sample(**kw, **bad)
    with pytest.raises(NotImplementedError):
        PLMSSampler(_HostModel()).sample(mask=m, x0=z, **kw)
    with pytest.raises(NotImplementedError):
        PLMSSampler(_HostModel()).sample(x0=z, **kw)
    # the sampler's own checks of a mask it cannot use come before any device work too
    from commonscenes_amd import lib
    with pytest.raises(lib.CsError, match="mask"):
        DDIMSampler(_HostModel()).sample(mask=torch.ones(1, 2, 16, 16, 16), x0=z, **kw)
    with pytest.raises(lib.CsError, match="x0_src"):
        DDIMSampler(_HostModel()).sample(mask=m, x0=z, x0_src=torch.tensor([1]), **kw)
    with pytest.raises(lib.CsError, match="rows for a batch"):
        DDIMSampler(_HostModel()).sample(mask=m.repeat(2, 1, 1, 1, 1), x0=z, **{**kw, "batch_size": 3})


def test_shape_comp_is_single_rank_and_checks_its_arguments_first(monkeypatch):
    from commonscenes_amd import dist
    from commonscenes_amd.sdfusion import SDFusionText2ShapeModel
    m = SDFusionText2ShapeModel.__new__(SDFusionText2ShapeModel)
    monkeypatch.setattr(dist, "world", lambda: (0, 2))
    with pytest.raises(RuntimeError, match="single-rank"):
        m.shape_comp(torch.zeros(1, 1, 64, 64, 64), {"x": (-1, 0), "y": (-1, 1), "z": (-1, 1)}, torch.zeros(1, 1, 1280))
    monkeypatch.setattr(dist, "world", lambda: (0, 1))
    with pytest.raises(ValueError, match="ngen"):
        m.shape_comp(torch.zeros(1, 1, 64, 64, 64), {"x": (-1, 0), "y": (-1, 1), "z": (-1, 1)}, torch.zeros(1, 1, 1280), ngen=0)
