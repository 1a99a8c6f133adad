"""CPU suite of the InceptionV3 pool3 extractor (commonscenes_amd/inception.py, csrc/cs_incep.hip): the layer table, the
loader, the BatchNorm fold, the synthetic weights, the C entries' presence and refusals, and the public surface.  Nothing
here launches a kernel."""
import ctypes as C
import re
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ("cs_incep_input", "cs_pool2d_max3", "cs_pool2d_avg3", "cs_pool2d_global_avg")


def test_layer_table_has_94_convs_and_the_stated_block_widths():
    from commonscenes_amd import inception as I
    shapes = I.inception_shapes()
    convs = [k for k in shapes if k.endswith(".conv.weight")]
    assert len(convs) == 94 and len(shapes) == 94 * 5
    assert all(len(shapes[k]) == 4 for k in convs)
    widths = I.block_widths()
    assert list(widths) == ["Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e",
                            "Mixed_7a", "Mixed_7b", "Mixed_7c"]
    assert [sum(w) for w in widths.values()] == [256, 288, 288, 768, 768, 768, 768, 768, 1280, 2048, 2048]
    # a block's output width is the next block's input width, and every channel count but the image's is a multiple of 16
    blocks = I.BLOCKS
    for (_, a), (_, b) in zip(blocks[:-1], blocks[1:]):
        assert sum(I.branch_width(br, I.block_input_width(a)) for br in a) == I.block_input_width(b)
    assert all(c.cout % 16 == 0 and (c.cin % 16 == 0 or c.cin == 3) for c in I.conv_layers())
    assert shapes["Mixed_6c.branch7x7dbl_2.conv.weight"] == (160, 160, 7, 1)
    assert shapes["Mixed_6c.branch7x7dbl_3.conv.weight"] == (160, 160, 1, 7)
    assert shapes["Mixed_7c.branch3x3_2b.conv.weight"] == (384, 384, 3, 1)
    assert shapes["Conv2d_1a_3x3.conv.weight"] == (32, 3, 3, 3)


def test_oracle_and_table_name_the_same_layers():
    """the independent oracle reads exactly the keys the loader validates: it runs on a state dict cut down to them"""
    sys.path.insert(0, str(ROOT / "tests"))
    import _inception_ref as R
    from commonscenes_amd import inception as I
    used = set()

    class Spy(dict):
        def __getitem__(self, k):
            used.add(k)
            return super().__getitem__(k)
    sd = Spy({k: (torch.ones(s) if k.endswith("running_var") else torch.zeros(s)) for k, s in I.inception_shapes().items()})
    out = R.features(sd, torch.zeros(1, 75, 75, 3), torch.float32)
    assert tuple(out.shape) == (1, 2048) and used == set(I.inception_shapes())


def test_loader_names_a_missing_or_misshapen_key_and_ignores_the_head():
    from commonscenes_amd import inception as I
    sd = {k: torch.zeros(s) for k, s in I.inception_shapes().items()}
    sd.update({"fc.weight": torch.zeros(1008, 2048), "fc.bias": torch.zeros(1008), "AuxLogits.conv0.conv.weight": torch.zeros(1),
               "Mixed_5b.branch1x1.bn.num_batches_tracked": torch.zeros((), dtype=torch.long)})
    I._validate(sd)                                    # the head, the auxiliary classifier and the counters are not read
    bad = dict(sd)
    del bad["Mixed_6a.branch3x3dbl_3.bn.running_var"]
    with pytest.raises(KeyError, match="Mixed_6a.branch3x3dbl_3.bn.running_var"):
        I.InceptionV3("cpu").load_state_dict(bad)
    bad = dict(sd)
    bad["Mixed_7b.branch3x3_2a.conv.weight"] = torch.zeros(384, 384, 3, 1)
    with pytest.raises(ValueError, match="Mixed_7b.branch3x3_2a.conv.weight"):
        I.InceptionV3("cpu").load_state_dict(bad)


def test_bn_fold_matches_batch_norm_in_fp64():
    from commonscenes_amd import inception as I
    g = torch.Generator().manual_seed(5)
    c = 48
    x = torch.randn(3, c, 5, 7, generator=g, dtype=torch.float64) * 3
    w, b = torch.rand(c, generator=g, dtype=torch.float64) + 0.5, torch.randn(c, generator=g, dtype=torch.float64)
    m, v = torch.randn(c, generator=g, dtype=torch.float64), torch.rand(c, generator=g, dtype=torch.float64) * 1e-2
    scale, shift = I.fold_bn(w, b, m, v)
    assert scale.dtype == torch.float64 and I.BN_EPS == 1e-3
    want = F.batch_norm(x, m, v, w, b, training=False, eps=1e-3)
    got = x * scale[None, :, None, None] + shift[None, :, None, None]
    assert float((got - want).abs().max()) <= 1e-13 * float(want.abs().max())
    # eps matters at these variances: the default 1e-5 would be far outside that bound
    off = F.batch_norm(x, m, v, w, b, training=False, eps=1e-5)
    assert float((off - want).abs().max()) > 1e-3


def test_synthetic_state_dict_is_deterministic_per_seed():
    from commonscenes_amd import inception as I
    a, b, c = I.synth_inception_state_dict(11), I.synth_inception_state_dict(11), I.synth_inception_state_dict(12)
    assert {k: tuple(v.shape) for k, v in a.items()} == I.inception_shapes()
    assert all(torch.equal(a[k], b[k]) for k in a) and all(v.dtype == torch.float32 for v in a.values())
    assert any(not torch.equal(a[k], c[k]) for k in a)
    assert all(float(v.min()) > 0 for k, v in a.items() if k.endswith("running_var"))
    # gain scales the BatchNorm outputs and the statistics of the layers that read them; the conv weights stay
    s = I.synth_inception_state_dict(11, gain=1e3)
    k = "Mixed_5b.branch1x1"
    assert torch.equal(s[k + ".conv.weight"], a[k + ".conv.weight"])
    assert torch.allclose(s[k + ".bn.weight"], a[k + ".bn.weight"] * 1e3) and torch.allclose(s[k + ".bn.running_var"],
                                                                                           a[k + ".bn.running_var"] * 1e6)
    assert torch.equal(s["Conv2d_1a_3x3.bn.running_var"], a["Conv2d_1a_3x3.bn.running_var"])


def test_entries_are_declared_built_and_exported_with_abi_18():
    from commonscenes_amd import build, lib
    assert "cs_incep.hip" in build.SOURCES and (build.CSRC / "cs_incep.hip").exists()
    txt = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "commonscenes_hip.h").read_text(), flags=re.S)
    dll = lib.load()
    for name in ENTRIES:
        assert re.search(rf"\bint {name}\s*\(", txt), f"{name} is not declared in the header"
        assert name in lib.SIGNATURES and hasattr(dll, name)
    assert lib.ABI_VERSION == 18 and dll.cs_abi_version() == 18


def test_entries_refuse_bad_arguments_before_any_launch():
    """every refusal returns CS_EINVAL from the host-side checks: no device is needed (or touched)"""
    from commonscenes_amd import lib
    dll = lib.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    p += (-p) % 16
    E = lib.CS_EINVAL
    ok_pool = dict(x=p, out=p, nb=1, h=5, w=5, c=8, ldx=8, ldo=8)

    def mx(stride=2, pad=0, **kw):
        a = {**ok_pool, **kw}
        return dll.cs_pool2d_max3(a["x"], a["out"], a["nb"], a["h"], a["w"], a["c"], a["ldx"], a["ldo"], stride, pad, None)

    def av(cip=0, **kw):
        a = {**ok_pool, **kw}
        return dll.cs_pool2d_avg3(a["x"], a["out"], a["nb"], a["h"], a["w"], a["c"], a["ldx"], a["ldo"], cip, None)

    def ga(**kw):
        a = {**ok_pool, **kw}
        return dll.cs_pool2d_global_avg(a["x"], a["out"], a["nb"], a["h"], a["w"], a["c"], a["ldx"], a["ldo"], None)

    for fn in (mx, av, ga):
        for bad in (dict(x=None), dict(out=None), dict(x=p + 2), dict(out=p + 1), dict(nb=0), dict(h=0), dict(w=0), dict(c=0),
                    dict(ldx=7), dict(ldo=7), dict(nb=1 << 20, h=1 << 6, w=1 << 6)):
            assert fn(**bad) == E, (fn.__name__, bad)
    assert mx(stride=3) == E and mx(stride=0) == E and mx(pad=2) == E and mx(pad=-1) == E
    assert mx(h=2) == E and mx(w=2, stride=1) == E            # no output row / column without padding
    assert av(cip=2) == E and av(cip=-1) == E

    def inp(img=p, is_float=0, nb=1, h=10, w=10, resize=1, norm=0, out=p, cpad=4):
        return dll.cs_incep_input(img, is_float, nb, h, w, resize, norm, out, cpad, None)
    for bad in (dict(img=None), dict(out=None), dict(out=p + 2), dict(nb=0), dict(h=0), dict(w=0), dict(cpad=2), dict(norm=2),
                dict(resize=2), dict(is_float=2), dict(resize=0), dict(resize=0, h=299, w=298),
                dict(is_float=1, h=299, w=299, resize=1), dict(is_float=1, h=299, w=299, resize=0, img=p + 2),
                dict(nb=1 << 15)):
        assert inp(**bad) == E, bad


def test_python_front_ends_refuse_cpu_tensors():
    from commonscenes_amd import inception as I, lib
    x = torch.zeros(1, 5, 5, 8)
    for fn in (lambda: I.max_pool3(x), lambda: I.avg_pool3(x), lambda: I.global_avg(x),
               lambda: I.front_end(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), 0),
               lambda: I.InceptionV3("cpu").features(torch.zeros(1, 75, 75, 4))):
        with pytest.raises(lib.CsError):
            fn()


def test_preprocess_modes_on_the_host():
    import numpy as np
    from PIL import Image
    from commonscenes_amd import inception as I
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, size=(2, 20, 31, 3), dtype=np.uint8)
    leg = I.preprocess(torch.from_numpy(a), "legacy_pytorch")
    assert leg.dtype == torch.uint8 and torch.equal(leg, torch.from_numpy(a))
    mixed = I.preprocess([Image.fromarray(a[0]), Image.fromarray(a[1, :10])], "legacy_pytorch")
    assert isinstance(mixed, list) and [tuple(m.shape) for m in mixed] == [(1, 20, 31, 3), (1, 10, 31, 3)]
    grey = I.preprocess(Image.fromarray(a[0, :, :, 0]), "legacy_pytorch")           # converted to RGB
    assert tuple(grey.shape) == (1, 20, 31, 3) and torch.equal(grey[..., 0], grey[..., 2])
    clean = I.preprocess(a, "clean")
    assert clean.dtype == torch.float32 and tuple(clean.shape) == (2, 299, 299, 3)
    want = np.asarray(Image.fromarray(a[1, :, :, 2].astype(np.float32), mode="F").resize((299, 299), resample=Image.BICUBIC))
    assert np.array_equal(clean[1, :, :, 2].numpy(), want)
    with pytest.raises(ValueError):
        I.preprocess(a, "legacy_tensorflow")


def test_fid_surface_still_refuses_a_missing_or_foreign_model(tmp_path):
    from commonscenes_amd import fid, lib
    with pytest.raises(lib.CsError):
        fid.image_features(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), None)
    with pytest.raises(lib.CsError):
        fid.image_features(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), object())
    with pytest.raises(lib.CsError, match="needs model="):
        fid.compute_fid(str(tmp_path), str(tmp_path))
    import inspect
    for fn in (fid.image_features, fid.features_of, fid.compute_fid, fid.compute_kid):
        assert "mode" in inspect.signature(fn).parameters


def test_fid_table_argument_surface():
    sys.path.insert(0, str(ROOT / "tools"))
    import fid_table as T
    a = T.parse_args(["--real", "R", "--fake", "F", "--inception", "synthetic"])
    assert (a.inception, a.inception_mode, a.clip) == ("synthetic", "clean", None)
    a = T.parse_args(["--real", "R", "--fake", "F", "--inception", "m.pth", "--inception-mode", "legacy_pytorch", "--clip", "synthetic"])
    assert (a.inception, a.inception_mode, a.clip) == ("m.pth", "legacy_pytorch", "synthetic")
    assert T.parse_args(["--real", "R", "--fake", "F", "--clip", "synthetic"]).inception is None
    for bad in (["--real", "R", "--fake", "F"], ["--real", "R", "--inception", "synthetic"],
                ["--synthetic", "8", "8", "4", "--inception", "synthetic"],
                ["--features", "a.npy", "b.npy", "--inception", "synthetic"],
                ["--real", "R", "--fake", "F", "--inception", "synthetic", "--inception-mode", "legacy_tensorflow"],
                ["--real", "R", "--fake", "F", "--inception", "synthetic", "--compare-host"]):
        with pytest.raises(SystemExit):
            T.parse_args(bad)
