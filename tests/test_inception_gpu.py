"""GPU suite of the InceptionV3 pool3 extractor: the kernels of csrc/cs_incep.hip, cs_conv_gemm at the network's 2-D kernel
forms, the six block types, the whole network and the FID / KID surface, all against the independent fp64 oracle
tests/_inception_ref.py.

Measured on the MI355X (one run; rel-L2 against the fp64 oracle, beside the yardstick = the oracle's own fp32 evaluation on
the same input; the gate is 2 x the yardstick): features B = 3 at 91 x 123 5.16e-7 vs 4.54e-7, B = 1 at 299 x 299 3.32e-7 vs
2.30e-7, gain 1e3 4.97e-7 vs 4.33e-7, encode_image clean 2.95e-7 vs 2.02e-7, legacy_pytorch 2.94e-7 vs 2.70e-7.  Without the
per-layer K slices (inception.k_slices) the 299 x 299 case measured 4.99e-7, 2.16 x its yardstick.  profiles/inception.txt and
DESIGN 8l hold the rest."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import _inception_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
SEED = 7


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.fixture(scope="module")
def sd():
    from commonscenes_amd import inception as I
    return I.synth_inception_state_dict(SEED)


@pytest.fixture(scope="module")
def model(sd):
    from commonscenes_amd import inception as I
    return I.InceptionV3("cuda").load_state_dict(sd)


def _net_input(shape, seed):
    """what the front end emits: values in [-1, 1], the pad channel zero"""
    x = torch.rand(shape, generator=_gen(seed)) * 2 - 1
    x[..., 3:] = 0
    return x


# ----------------------------------------------------------------------------------------------------------------------
# pools
# ----------------------------------------------------------------------------------------------------------------------
POOL_SHAPES = [(2, 7, 9, 5), (1, 3, 3, 16), (3, 1, 4, 80), (2, 2, 2, 7), (2, 35, 35, 288), (1, 8, 8, 2048)]
SENTINEL = -777.0


def _layouts(shape, seed, layout):
    """x on the device as asked -- "dense", "slice" (a channel range at offset 5 of a buffer 9 channels wider: never the
    float4 path) or "slice4" (offset 4 of a buffer 8 wider: the float4 path with ld > C where C % 4 == 0) -- and its CPU copy"""
    b, h, w, c = shape
    xc = torch.randn(shape, generator=_gen(seed))
    if layout == "dense":
        return xc.cuda(), xc
    off, extra = (5, 9) if layout == "slice" else (4, 8)
    big = torch.full((b, h, w, c + extra), SENTINEL, device="cuda")
    big[..., off:off + c] = xc.cuda()
    return big[..., off:off + c], xc


def _out_view(oshape, layout):
    """an output placed like the input; returns (view, whole buffer)"""
    if layout == "dense":
        t = torch.full(oshape, SENTINEL, device="cuda")
        return t, t
    off, extra = (3, 6) if layout == "slice" else (8, 12)
    big = torch.full((*oshape[:-1], oshape[-1] + extra), SENTINEL, device="cuda")
    return big[..., off:off + oshape[-1]], big


def _guard_ok(view, big):
    """nothing outside the view was written"""
    mask = torch.ones_like(big, dtype=torch.bool)
    if view.data_ptr() != big.data_ptr() or view.shape != big.shape:
        off = (view.data_ptr() - big.data_ptr()) // 4
        mask[..., off:off + view.shape[-1]] = False
        return bool((big[mask] == SENTINEL).all())
    return True


def _nchw64(x):
    return x.double().permute(0, 3, 1, 2)


def _nhwc(y):
    return y.permute(0, 2, 3, 1)


@pytest.mark.parametrize("layout", ["dense", "slice", "slice4"])
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_max_pool_is_exact(shape, layout):
    from commonscenes_amd import inception as I, lib
    b, h, w, c = shape
    x, xc = _layouts(shape, 11, layout)
    ran = 0
    for stride in (1, 2):
        for pad in (0, 1):
            if h + 2 * pad < 3 or w + 2 * pad < 3:
                with pytest.raises(lib.CsError):
                    I.max_pool3(x, stride, pad)
                continue
            ho, wo = (h + 2 * pad - 3) // stride + 1, (w + 2 * pad - 3) // stride + 1
            out, big = _out_view((b, ho, wo, c), layout)
            I.max_pool3(x, stride, pad, out=out)
            want = _nhwc(F.max_pool2d(_nchw64(xc), 3, stride, pad))
            assert tuple(want.shape) == (b, ho, wo, c)
            assert torch.equal(out.cpu().double(), want), (stride, pad)
            assert _guard_ok(out, big)
            # the last sample alone carries the bits it has at the end of the batch
            alone = I.max_pool3(x[b - 1:].contiguous() if layout == "dense" else x[b - 1:], stride, pad)
            assert torch.equal(alone[0], out[b - 1])
            ran += 1
    assert ran >= 2


@pytest.mark.parametrize("layout", ["dense", "slice", "slice4"])
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_avg_pool_within_nine_roundings_of_the_window_mean(shape, layout):
    from commonscenes_amd import inception as I
    b, h, w, c = shape
    x, xc = _layouts(shape, 12, layout)
    for cip in (False, True):
        out, big = _out_view(shape, layout)
        I.avg_pool3(x, count_include_pad=cip, out=out)
        want = _nhwc(F.avg_pool2d(_nchw64(xc), 3, 1, 1, count_include_pad=cip))
        mean_abs = _nhwc(F.avg_pool2d(_nchw64(xc).abs(), 3, 1, 1, count_include_pad=cip))
        err = (out.cpu().double() - want).abs()
        worst = float((err / (9 * U * mean_abs)).max())
        print(f"avg3 {shape} {layout} include_pad={cip}: max err / bound = {worst:.3f}")
        assert bool((err <= 9 * U * mean_abs).all())
        assert _guard_ok(out, big)
        xx = torch.cat([x[b - 1:], x])                 # the last sample again, now at index 0 of a longer batch
        assert torch.equal(I.avg_pool3(xx, count_include_pad=cip)[0], out[b - 1])


@pytest.mark.parametrize("layout", ["dense", "slice", "slice4"])
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_global_average_is_the_fp64_mean_rounded_once(shape, layout):
    from commonscenes_amd import inception as I
    b, h, w, c = shape
    x, xc = _layouts(shape, 13, layout)
    out, big = _out_view((b, c), layout)
    I.global_avg(x, out=out)
    want = xc.double().mean(dim=(1, 2))
    mean_abs = xc.double().abs().mean(dim=(1, 2))
    err = (out.cpu().double() - want).abs()
    print(f"global_avg {shape} {layout}: max err / bound = {float((err / (2 * U * mean_abs)).max()):.3f}")
    assert bool((err <= 2 * U * mean_abs).all())
    assert _guard_ok(out, big)
    xx = torch.cat([x[b - 1:], x])
    assert torch.equal(I.global_avg(xx)[0], out[b - 1])


# ----------------------------------------------------------------------------------------------------------------------
# front end
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", [0, 1])
@pytest.mark.parametrize("size", [(256, 256), (299, 299), (64, 48), (1, 1), (300, 600)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_front_end_bilinear_against_interpolate_in_fp64(size, norm):
    from commonscenes_amd import inception as I
    img = torch.randint(0, 256, (2, size[0], size[1], 3), generator=_gen(size[0] + norm), dtype=torch.uint8)
    out = I.front_end(img.cuda(), norm)
    assert tuple(out.shape) == (2, 299, 299, I.CPAD)
    want = R.front_end(img, norm)
    err = float((out[..., :3].cpu().double() - want).abs().max())
    print(f"front end {size} norm {norm}: max abs err {err:.3e} = {err / U:.2f} x 2^-24")
    assert err <= 8 * U
    assert bool((out[..., 3:] == 0).all())
    for cpad in (5, 16):                               # the scalar store path; more than one float4 of padding
        o2 = I.front_end(img.cuda(), norm, cpad=cpad)
        assert torch.equal(o2[..., :3], out[..., :3]) and bool((o2[..., 3:] == 0).all())
    alone = I.front_end(img[1:].cuda(), norm)
    assert torch.equal(alone[0], out[1])


@pytest.mark.parametrize("norm", [0, 1])
def test_front_end_identity_and_float_form_are_the_normalisation_alone(norm):
    """resize = 0 and the float form: the result is exactly the normalisation's two fp32 roundings of the input"""
    from commonscenes_amd import inception as I, lib
    one, two, c255, c128 = (np.float32(v) for v in (1, 2, 255, 128))          # numpy: IEEE fp32 operations, one rounding each

    def f(t):
        v = t.numpy().astype(np.float32)
        return torch.from_numpy(two * (v / c255) - one if norm == 0 else (v - c128) / c128)
    img = torch.randint(0, 256, (2, 299, 299, 3), generator=_gen(3), dtype=torch.uint8)
    out = I.front_end(img.cuda(), norm, resize=False)
    assert torch.equal(out[..., :3].cpu(), f(img.float())) and bool((out[..., 3:] == 0).all())
    # the resampling grid of a 299 x 299 image is the image: the same bits with resize = 1
    assert torch.equal(I.front_end(img.cuda(), norm, resize=True), out)
    fl = torch.rand((2, 299, 299, 3), generator=_gen(4)) * 300.0 - 20.0         # bicubic overshoot leaves [0, 255]
    outf = I.front_end(fl.cuda(), norm)
    assert torch.equal(outf[..., :3].cpu(), f(fl)) and bool((outf[..., 3:] == 0).all())
    with pytest.raises(lib.CsError):
        I.front_end(img[:, :100].cuda(), norm, resize=False)
    with pytest.raises(lib.CsError):
        I.front_end(fl[:, :100].cuda(), norm)


# ----------------------------------------------------------------------------------------------------------------------
# conv forms
# ----------------------------------------------------------------------------------------------------------------------
FORMS = {"1x1": ((1, 1), 1, (0, 0)), "3x3s2": ((3, 3), 2, (0, 0)), "3x3": ((3, 3), 1, (0, 0)), "3x3p1": ((3, 3), 1, (1, 1)),
         "5x5p2": ((5, 5), 1, (2, 2)), "1x7": ((1, 7), 1, (0, 3)), "7x1": ((7, 1), 1, (3, 0)), "1x3": ((1, 3), 1, (0, 1)),
         "3x1": ((3, 1), 1, (1, 0))}


@pytest.mark.parametrize("chans", [(3, 32), (48, 64), (80, 192), (160, 160)], ids=lambda c: f"{c[0]}to{c[1]}")
@pytest.mark.parametrize("form", list(FORMS))
def test_basic_conv2d_forms_against_fp64(form, chans):
    from commonscenes_amd import inception as I
    k, stride, pad = FORMS[form]
    cin, cout = chans
    g = _gen(cin * 100 + k[0] * 10 + k[1] + stride)
    fan = cin * k[0] * k[1]
    lsd = {"L.conv.weight": torch.randn((cout, cin, *k), generator=g) * (2.0 / fan) ** 0.5,
           "L.bn.weight": torch.rand(cout, generator=g) + 0.5, "L.bn.bias": torch.randn(cout, generator=g) * 0.3,
           "L.bn.running_mean": torch.randn(cout, generator=g) * 0.3, "L.bn.running_var": torch.rand(cout, generator=g) + 0.3}
    cp = (cin + 3) // 4 * 4
    x = torch.zeros(2, 9, 11, cp)
    x[..., :cin] = torch.randn((2, 9, 11, cin), generator=g)
    ly = I.pack_layer(I.Conv("L", cin, cout, k, stride, pad), lsd, "cuda")
    out = I.InceptionV3("cuda").run_layer(x.cuda().unsqueeze(1), ly)
    want = R.basic_conv(lsd, "L", _nchw64(x[..., :cin]), stride=stride, padding=pad)
    assert tuple(out.shape) == (2, 1, want.shape[2], want.shape[3], cout)
    err = rel_l2(out[:, 0], _nhwc(want))
    print(f"BasicConv2d {form} {cin}->{cout}: rel-L2 {err:.3e}")
    assert err <= 1e-6


# ----------------------------------------------------------------------------------------------------------------------
# block types
# ----------------------------------------------------------------------------------------------------------------------
BLOCK_CASES = {"A": ("Mixed_5b", "A", (5, 7), 3), "B": ("Mixed_6a", "B", (7, 9), 3), "C": ("Mixed_6b", "C", (5, 7), 5),
               "D": ("Mixed_7a", "D", (7, 9), 4), "E_avg": ("Mixed_7b", "E_avg", (5, 7), 3),
               "E_max": ("Mixed_7c", "E_max", (5, 7), 3)}


@pytest.mark.parametrize("case", list(BLOCK_CASES))
def test_block_types_branch_by_branch(case, sd, model):
    from commonscenes_amd import inception as I
    name, kind, (h, w), depth = BLOCK_CASES[case]
    cin = I.block_input_width(dict(I.BLOCKS)[name])
    x = torch.randn((2, h, w, cin), generator=_gen(len(name) + cin)).abs()          # what a ReLU hands a block
    out = model.block(x.cuda().unsqueeze(1), name)[:, 0]
    branches = R.block(sd, name, kind, _nchw64(x))
    assert out.shape[-1] == sum(b.shape[1] for b in branches) == sum(I.block_widths()[name])
    c0 = 0
    for i, br in enumerate(branches):
        c1 = c0 + br.shape[1]
        err = rel_l2(out[..., c0:c1], _nhwc(br))
        print(f"{name} branch {i} channels [{c0}, {c1}): rel-L2 {err:.3e}")
        assert err <= 1e-6 * depth, f"{name}: branch {i} (channels {c0}..{c1}) is off"
        c0 = c1


# ----------------------------------------------------------------------------------------------------------------------
# the network
# ----------------------------------------------------------------------------------------------------------------------
def _gate(sd_, x, dev_feats, what):
    """device rel-L2 against the fp64 oracle <= 2 x the oracle's own fp32-vs-fp64 rel-L2 on the same input"""
    f64 = R.features(sd_, x, torch.float64)
    yard = rel_l2(R.features(sd_, x, torch.float32), f64)
    err = rel_l2(dev_feats, f64)
    print(f"{what}: device rel-L2 {err:.3e}, fp32 oracle rel-L2 {yard:.3e}, ratio {err / yard:.2f}")
    assert err <= 2 * yard, f"{what}: device {err:.3e} > 2 x yardstick {yard:.3e}"
    return err, yard


def test_features_nonsquare_small_input(sd, model):
    x = _net_input((3, 91, 123, 4), 21)
    trace = []
    out = model.features(x.cuda(), trace=trace)
    assert tuple(out.shape) == (3, 2048) and trace[-1][1:] == (1, 2, 2048)
    _gate(sd, x, out, "features B=3 91x123")


def test_features_full_size_and_stage_extents(sd, model):
    x = _net_input((1, 299, 299, 4), 22)
    trace = []
    out = model.features(x.cuda(), trace=trace)
    assert tuple(out.shape) == (1, 2048)
    got = {n: (h, w, c) for n, h, w, c in trace if n != "maxpool"}
    pools = [(h, w, c) for n, h, w, c in trace if n == "maxpool"]
    assert got["Conv2d_1a_3x3"] == (149, 149, 32) and got["Conv2d_2a_3x3"] == (147, 147, 32)
    assert got["Conv2d_2b_3x3"] == (147, 147, 64) and pools[0] == (73, 73, 64)
    assert got["Conv2d_3b_1x1"] == (73, 73, 80) and got["Conv2d_4a_3x3"] == (71, 71, 192) and pools[1] == (35, 35, 192)
    assert [got[n] for n in ("Mixed_5b", "Mixed_5c", "Mixed_5d")] == [(35, 35, 256), (35, 35, 288), (35, 35, 288)]
    assert all(got[n] == (17, 17, 768) for n in ("Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"))
    assert got["Mixed_7a"] == (8, 8, 1280) and got["Mixed_7b"] == got["Mixed_7c"] == (8, 8, 2048)
    _gate(sd, x, out, "features B=1 299x299")


def test_gain_1e3_stress_keeps_the_gate_and_a_clear_status_word():
    """every activation is O(1e3): beyond 65504 / 16, what the fixed operand scale would carry"""
    from commonscenes_amd import inception as I, ops
    big = I.synth_inception_state_dict(SEED, gain=1e3)
    m = I.InceptionV3("cuda").load_state_dict(big)
    x = _net_input((3, 91, 123, 4), 23)
    ops.read_status()                                   # start from a clear word
    out = m.features(x.cuda())
    assert ops.read_status(reset=False) == 0
    assert float(out.abs().max()) > 4094.0              # the stress is real: these magnitudes overflow at scale 16
    _gate(big, x, out, "features gain=1e3 B=3 91x123")


def test_batch_in_chunks_is_bit_equal_to_one_call(model):
    x = _net_input((5, 75, 91, 4), 24).cuda()
    whole = model.features(x)
    parts = torch.cat([model.features(x[i:i + 2]) for i in range(0, 5, 2)])
    assert torch.equal(whole, parts)


# ----------------------------------------------------------------------------------------------------------------------
# end to end
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def png_dirs(tmp_path_factory):
    from PIL import Image
    rng = np.random.default_rng(5)
    out = []
    for tag, base in (("real", 90), ("fake", 140)):
        d = tmp_path_factory.mktemp(tag)
        for i in range(6):
            h, w = (64, 48) if i % 2 else (80, 80)
            a = np.clip(rng.normal(base, 60, size=(h, w, 3)), 0, 255).astype(np.uint8)
            Image.fromarray(a).save(d / f"Bedroom-{i}.png")
        out.append(d)
    return out


@pytest.mark.parametrize("mode", ["clean", "legacy_pytorch"])
def test_compute_fid_and_kid_from_png_directories(mode, png_dirs, sd, model):
    from PIL import Image
    from commonscenes_amd import fid, inception as I
    real, fake = png_dirs
    f1 = fid.features_of(str(real), model, "all", 4, "test", mode)
    f2 = fid.features_of(str(fake), model, "all", 4, "test", mode)
    assert tuple(f1.shape) == tuple(f2.shape) == (6, 2048)
    # the same images in the same chunks give the same features, so the same numbers
    assert fid.compute_fid(str(real), str(fake), model=model, mode=mode, batch=4) == fid.frechet_distance(f1, f2)
    assert fid.compute_kid(str(real), str(fake), model=model, mode=mode, batch=4, seed=3) == fid.kernel_distance(f1, f2, seed=3)
    # the oracle's features of the first two images of `real`, from its own front end
    files = fid.list_images(str(real))[:2]
    xs64, xs32 = [], []
    for p in files:
        a = np.array(Image.open(p).convert("RGB"), dtype=np.uint8)
        if mode == "clean":
            chans = [np.asarray(Image.fromarray(a[:, :, c].astype(np.float32), mode="F").resize((299, 299), resample=Image.BICUBIC))
                     for c in range(3)]
            v = torch.from_numpy(np.stack(chans, 2))[None]
            assert torch.equal(I.preprocess(p, "clean"), v)           # the pixels of a direct PIL call
            xs64.append((v.double() - 128) / 128)
            xs32.append((v - 128) / 128)
        else:
            u = torch.from_numpy(a)[None]
            xs64.append(R.front_end(u, 0, dtype=torch.float64))
            xs32.append(R.front_end(u, 0, dtype=torch.float32))
    x64, x32 = torch.cat(xs64), torch.cat(xs32)
    f64 = R.features(sd, x64, torch.float64)
    yard = rel_l2(R.features(sd, x32, torch.float32), f64)
    err = rel_l2(f1[:2], f64)
    print(f"encode_image {mode}: device rel-L2 {err:.3e}, fp32 oracle rel-L2 {yard:.3e}, ratio {err / yard:.2f}")
    assert err <= 2 * yard


def test_fid_table_tool_prints_the_inception_block(png_dirs, capsys):
    sys.path.insert(0, str(ROOT / "tools"))
    import fid_table as T
    d = str(png_dirs[0])
    T.main(["--real", d, "--fake", d, "--inception", "synthetic", "--seed", "1"])
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("FID_TABLE ")][-1]
    rec = json.loads(line[len("FID_TABLE "):])
    blk = rec["inception"]
    assert blk["n_real"] == blk["n_fake"] == 6 and blk["d"] == 2048 and blk["mode"] == "clean"
    assert abs(blk["fid"]) < 1e-6 and np.isfinite(blk["kid"]) and blk["images_per_second"] > 0
