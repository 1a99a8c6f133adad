"""CLIP on the MI355X (commonscenes_amd/clip.py over csrc/cs_clip.hip and the GEMM / LayerNorm / attention entries):
  * every new kernel against the torch expression it replaces (bit-equal where it is a copy or a fixed sequence of IEEE
    operations, against fp64 within the project's per-op 1e-6 elsewhere),
  * both towers against `transformers`' CLIP (tests/golden/clip_tiny.npz, fp64) and, at the shipped widths, against the
    plain-torch restatement in tests/test_clip_cpu.py (which that file pins to the fixture), within the project's 1e-4,
  * invariances that must hold bit for bit: padding after the end-of-text token, a sample's place in the batch.
The two tests that hand a kernel a bad index rely on the kernels comparing it before reading through it (cs_clip.hip) and
clear the sticky index word again.  Every figure is printed before it is asserted."""
import contextlib
import importlib.util
import io
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import test_clip_cpu as ref
from conftest import rel_l2

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden" / "clip_tiny.npz"


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(got, want, what):
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, what
    differ = int((_bits(got) != _bits(want)).sum())
    print(f"{what}: {differ} of {got.numel()} entries differ in bits")
    assert differ == 0, what


def _randn(seed, *shape):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32))


# ---- kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,s,p", [(3, 64, 32), (2, 40, 8)])
def test_patchify_is_bit_equal_to_the_torch_expression(b, s, p):
    from commonscenes_amd import clip as K, lib
    u = torch.from_numpy(np.random.default_rng(s).integers(0, 256, size=(b, s, s, 3), dtype=np.uint8))
    pix = ((u.float() / 255) - torch.tensor(K.CLIP_MEAN)) / torch.tensor(K.CLIP_STD)           # fp32 on the CPU: IEEE
    g = s // p
    want = pix.view(b, g, p, g, p, 3).permute(0, 1, 3, 5, 2, 4).reshape(b * g * g, 3 * p * p)   # columns (c, py, px)
    got = K.patchify(u.cuda(), p)
    _same_bits(got, want.contiguous(), f"patchify B={b} S={s} P={p}")
    with pytest.raises(lib.CsError):
        K.patchify(u.cuda(), p - 1 if s % (p - 1) else p + 1)


def test_assemble_image_tokens_is_bit_equal_to_torch():
    from commonscenes_amd import clip as K
    b, ntok, w = 3, 25, 192
    patch, cls, pos = _randn(1, b * ntok, w), _randn(2, w), _randn(3, ntok + 1, w)
    want = torch.cat([cls.expand(b, 1, w), patch.view(b, ntok, w)], dim=1) + pos
    _same_bits(K.assemble_image_tokens(patch.cuda(), cls.cuda(), pos.cuda(), b), want, "assemble")
    # a patch matrix that is a column slice of a wider buffer
    wide = _randn(4, b * ntok, w + 64)
    want = torch.cat([cls.expand(b, 1, w), wide[:, 32:32 + w].reshape(b, ntok, w)], dim=1) + pos
    _same_bits(K.assemble_image_tokens(wide.cuda()[:, 32:32 + w], cls.cuda(), pos.cuda(), b), want, "assemble (view)")


def test_embed_text_is_bit_equal_and_flags_a_bad_id():
    from commonscenes_amd import clip as K, ops
    vocab, w, b, t = 100, 128, 3, 16
    table, pos = _randn(5, vocab, w), _randn(6, t, w)
    ids = torch.from_numpy(np.random.default_rng(7).integers(0, vocab, size=(b, t)).astype(np.int32))
    ids[0, 0], ids[2, t - 1] = 0, vocab - 1
    want = table[ids.long()] + pos
    word = ops.index_err_word()
    word.zero_()
    _same_bits(K.embed_text(table.cuda(), ids.cuda(), pos.cuda()), want, "embed_text")
    assert int(word.item()) == 0
    # a shorter text than the positional table
    _same_bits(K.embed_text(table.cuda(), ids[:, :5].contiguous().cuda(), pos.cuda()), want[:, :5].contiguous(), "embed_text T=5")
    bad = ids.clone()
    bad[1, 4] = vocab                     # one past the table: compared before anything is read through it
    got = K.embed_text(table.cuda(), bad.cuda(), pos.cuda()).cpu()
    flag = int(word.item())
    word.zero_()
    print(f"bad id: index word {flag}, NaNs in the row {int(torch.isnan(got[1, 4]).sum())} / {w}")
    assert flag != 0 and bool(torch.isnan(got[1, 4]).all())
    keep = torch.ones(b, t, dtype=torch.bool)
    keep[1, 4] = False
    _same_bits(got[keep], want[keep], "embed_text rows beside the bad id")
    with pytest.raises(IndexError):
        K.embed_text(table.cuda(), bad.cuda(), pos.cuda())
        ops.check_index_errors(what="CLIP token ids")
    assert int(word.item()) == 0


def test_quick_gelu_against_fp64():
    from commonscenes_amd import clip as K
    x = torch.cat([torch.tensor([0.0, -0.0, 1e-30, -1e-30, 20.0, -20.0, 19.999, -19.999]), torch.linspace(-20, 20, 200000),
                   _randn(8, 4096) * 3]).view(-1, 8).contiguous()
    want = x.double() * torch.sigmoid(1.702 * x.double())
    got = K.quick_gelu(x.cuda()).cpu()
    rel = ((got.double() - want).abs() / want.abs().clamp_min(1e-300))[want != 0]
    print(f"quick_gelu over [-20, 20]: max relative error {float(rel.max()):.3e} (at x = {float(x[want != 0][rel.argmax()]):.4f})")
    assert float(rel.max()) <= 1e-6
    assert bool((got[want == 0] == 0).all())
    # in place, and on a column slice of a wider buffer: the same bits
    y = x.cuda().clone()
    assert K.quick_gelu(y, out=y) is y
    _same_bits(y, got, "quick_gelu in place")
    wide = torch.zeros(x.shape[0], 24)
    wide[:, 8:16] = x
    wd = wide.cuda()
    K.quick_gelu(wd[:, 8:16], out=wd[:, 8:16])
    _same_bits(wd[:, 8:16].contiguous(), got, "quick_gelu on a view")
    assert float(wd[:, :8].abs().max()) == 0 and float(wd[:, 16:].abs().max()) == 0
    edge = torch.tensor([[1e4, -1e4, 3e38, -3e38, float("nan"), 88.0, -88.0, 60.0]])
    e = K.quick_gelu(edge.cuda()).cpu()[0]
    print(f"quick_gelu edges: {e.tolist()}")
    assert bool(torch.isfinite(e[[0, 1, 2, 3, 5, 6, 7]]).all()) and bool(torch.isnan(e[4]))
    assert float(e[0]) == 1e4 and float(e[1]) == 0.0 and float(e[5]) == 88.0 and float(e[6]) == 0.0


def _causal_ref(q, k, v, heads):
    b, t, c = q.shape
    dh = c // heads
    q, k, v = (u.double().reshape(b, t, heads, dh).transpose(1, 2) for u in (q, k, v))
    s = (q @ k.transpose(-1, -2)) * dh ** -0.5
    s = s.masked_fill(torch.ones(t, t, dtype=torch.bool).triu(1), float("-inf"))
    return (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(b, t, c)


@pytest.mark.parametrize("b,t,heads,dh", [(2, 77, 8, 64), (1, 1, 2, 64), (3, 5, 2, 64), (1, 64, 2, 64), (1, 65, 3, 64),
                                          (1, 128, 2, 32), (1, 128, 1, 64)])      # the last: over 64 KB of LDS
def test_attn_causal_against_fp64_on_strided_views(b, t, heads, dh):
    from commonscenes_amd import clip as K
    w = heads * dh
    buf = _randn(100 + t, b, t, 3 * w)                    # the fused in_proj output: q | k | v
    dev = buf.cuda()
    q, k, v = dev[..., :w], dev[..., w:2 * w], dev[..., 2 * w:]
    got = K.attn_causal(q, k, v, heads, dh ** -0.5)
    want = _causal_ref(buf[..., :w], buf[..., w:2 * w], buf[..., 2 * w:], heads)
    err = rel_l2(got, want)
    print(f"attn_causal B={b} T={t} heads={heads} dh={dh}: rel-L2 vs fp64 {err:.3e}")
    assert err <= 1e-6
    # causality: other finite K / V rows after i0 leave the output rows up to i0 bit-identical
    if t > 1:
        i0 = t // 2
        dev2 = dev.clone()
        dev2[:, i0 + 1:, w:] = (_randn(200 + t, b, t - i0 - 1, 2 * w) * 50.0).cuda()
        got2 = K.attn_causal(dev2[..., :w], dev2[..., w:2 * w], dev2[..., 2 * w:], heads, dh ** -0.5)
        _same_bits(got2[:, :i0 + 1].contiguous(), got[:, :i0 + 1].contiguous(), f"rows <= {i0} after editing K / V rows > {i0}")
        assert not torch.equal(got2[:, i0 + 1:], got[:, i0 + 1:])


def test_attn_causal_rejects_what_it_does_not_cover():
    from commonscenes_amd import clip as K, lib
    for t, heads, dh in ((129, 2, 64), (8, 2, 68), (8, 1, 128), (8, 2, 6)):
        x = torch.zeros(1, t, 3 * heads * dh, device="cuda")
        w = heads * dh
        with pytest.raises(lib.CsError, match="invalid argument"):
            K.attn_causal(x[..., :w], x[..., w:2 * w], x[..., 2 * w:], heads, 1.0)


def test_pool_eot_takes_the_first_maximum():
    from commonscenes_amd import clip as K
    b, t, w = 3, 16, 128
    x = _randn(9, b, t, w)
    ids = torch.from_numpy(np.random.default_rng(10).integers(1, 90, size=(b, t)).astype(np.int32))
    ids[0, 3] = 99                         # the end-of-text token early, zeros after it
    ids[0, 4:] = 0
    ids[1, t - 1] = 99                     # in the last position
    ids[2, 2] = ids[2, 5] = 99             # the maximum twice: the first position wins
    want = x[torch.arange(b), torch.tensor([3, t - 1, 2])]
    assert torch.equal(ids.long().argmax(dim=1), torch.tensor([3, t - 1, 2]))
    _same_bits(K.pool_eot(x.cuda(), ids.cuda()), want, "pool_eot")
    wide = _randn(11, b, t, w + 32)
    _same_bits(K.pool_eot(wide.cuda()[..., 16:16 + w], ids.cuda()), wide[torch.arange(b), torch.tensor([3, t - 1, 2]), 16:16 + w],
               "pool_eot (view)")


@pytest.mark.parametrize("e", [32, 512])
def test_feature_pair_l2_against_fp64(e):
    from commonscenes_amd import clip as K, ops
    n = 9
    f = _randn(20 + e, n, e) * 3
    pairs = torch.tensor([[0, 1], [2, 3], [0, 1], [4, 4], [8, 0], [1, 0], [7, 7]])
    got = K.feature_pair_l2(f.cuda(), pairs).cpu()
    want = (f.double()[pairs[:, 0]] - f.double()[pairs[:, 1]]).norm(dim=1)
    nz = want > 0
    rel = float(((got.double() - want).abs()[nz] / want[nz]).max())
    print(f"feature_pair_l2 E={e}: max relative error vs fp64 {rel:.3e}; (a, a) -> {got[3].item()}, {got[6].item()}")
    assert rel <= 1e-6
    assert got[3].item() == 0.0 and got[6].item() == 0.0                       # (a, a): exactly zero
    assert _bits(got)[0] == _bits(got)[2] == _bits(got)[5]                     # a repeated pair, and (b, a)
    # a device pair list with a bad entry: NaN there, the index word set, the other entries as before
    word = ops.index_err_word()
    word.zero_()
    bad = pairs.clone().to(torch.int32)
    bad[1, 1] = n
    got_bad = K.feature_pair_l2(f.cuda(), bad.cuda(), check_indices=False).cpu()
    flag = int(word.item())
    word.zero_()
    print(f"bad pair: index word {flag}, entry {got_bad[1].item()}")
    assert flag != 0 and bool(torch.isnan(got_bad[1]))
    keep = torch.arange(len(pairs)) != 1
    _same_bits(got_bad[keep], got[keep], "the entries beside the bad pair")
    from commonscenes_amd import lib
    with pytest.raises(lib.CsError):
        K.feature_pair_l2(f.cuda(), bad.cuda())               # the wrapper's own check (one read-back)
    with pytest.raises(lib.CsError):
        K.feature_pair_l2(f.cuda(), [[0, n]])


# ---- towers -------------------------------------------------------------------------------------------------------------
def _model(cfg_by_tower, seed):
    from commonscenes_amd import clip as K
    sd = K.synth_clip_state_dict(cfg_by_tower, seed)
    return K.CLIP("cuda").load_state_dict(sd), sd


@pytest.mark.parametrize("name", ref.VISION_CASES + ref.TEXT_CASES)
def test_towers_against_the_transformers_fixture(gold, name):
    cfg, inp, out64, out32 = ref.fixture_case(gold, name)
    tower = "vision" if name in ref.VISION_CASES else "text"
    model, _ = _model({tower: cfg}, cfg["seed"])
    got = model.encode_image(torch.from_numpy(inp)) if tower == "vision" else model.encode_text(torch.from_numpy(inp))
    err = rel_l2(got, torch.from_numpy(out64))
    cpu32 = rel_l2(torch.from_numpy(out32), torch.from_numpy(out64))
    print(f"{name} ({tower}, {cfg}): rel-L2 vs transformers fp64 {err:.3e}; transformers' own CPU fp32 {cpu32:.3e}")
    assert tuple(got.shape) == out64.shape and err <= 1e-4


SHIPPED_VISION = dict(width=768, layers=2, patch=32, grid=7, embed=512)           # 12 heads, 50 tokens
# (the vocabulary only sizes the table cs_clip_embed_text gathers from: 512 rows keep the weight generation quick)
SHIPPED_TEXT = dict(width=512, layers=2, context=77, vocab=512, embed=512)        # 8 heads, 77 tokens


def _text_ids(rng, b, t, vocab):
    ids = np.zeros((b, t), np.int32)
    for r in range(b):
        e = int(rng.integers(2, t))
        ids[r, 0] = vocab - 2
        ids[r, 1:e] = rng.integers(1, vocab - 2, size=e - 1)
        ids[r, e] = vocab - 1
    return ids


def test_vision_tower_at_the_shipped_width():
    model, sd = _model({"vision": SHIPPED_VISION}, 31)
    assert (model.vision.heads, model.vision.grid ** 2 + 1, model.vision.resolution) == (12, 50, 224)
    img = torch.from_numpy(np.random.default_rng(32).integers(0, 256, size=(2, 224, 224, 3), dtype=np.uint8))
    want = ref.ref_encode_image(sd, img, torch.float64)
    err = rel_l2(model.encode_image(img), want)
    cpu32 = rel_l2(ref.ref_encode_image(sd, img, torch.float32), want)
    print(f"vision width 768, 12 heads, 50 tokens, B=2, 2 layers: rel-L2 vs fp64 {err:.3e}; CPU fp32 restatement {cpu32:.3e}")
    assert err <= 1e-4


def test_text_tower_at_the_shipped_width():
    model, sd = _model({"text": SHIPPED_TEXT}, 33)
    assert (model.text.heads, model.text.context) == (8, 77)
    ids = _text_ids(np.random.default_rng(34), 3, 77, SHIPPED_TEXT["vocab"])
    ids[0, :] = 0
    ids[0, :76] = np.arange(1, 77)
    ids[0, 76] = SHIPPED_TEXT["vocab"] - 1                   # a text that fills the context: the last row pools
    want = ref.ref_encode_text(sd, ids, torch.float64)
    got, hidden = model.encode_text(torch.from_numpy(ids), return_hidden=True)
    err = rel_l2(got, want)
    cpu32 = rel_l2(ref.ref_encode_text(sd, ids, torch.float32), want)
    print(f"text width 512, 8 heads, 77 tokens, B=3, 2 layers: rel-L2 vs fp64 {err:.3e}; CPU fp32 restatement {cpu32:.3e}")
    assert err <= 1e-4 and tuple(hidden.shape) == (3, 77, 512)
    _same_bits(model.encode_text(ids), got, "encode_text with and without return_hidden (numpy ids)")


def test_padding_after_the_end_of_text_does_not_reach_the_features(gold):
    cfg, inp, _, _ = ref.fixture_case(gold, "t0")
    model, _ = _model({"text": cfg}, cfg["seed"])
    ids = np.repeat(inp[:1], 2, axis=0).copy()                # EOT at position 3, zeros after it
    assert ids[0].argmax() == 3
    ids[1, 4:] = np.random.default_rng(40).integers(1, cfg["vocab"] - 1, size=ids.shape[1] - 4)
    got = model.encode_text(ids)
    _same_bits(got[1:2], got[0:1], "features of two texts that differ only after the end-of-text token")


@pytest.mark.parametrize("tower", ["vision", "text"])
def test_a_sample_does_not_know_its_place_in_the_batch(gold, tower):
    name = "v1" if tower == "vision" else "t1"
    cfg, inp, _, _ = ref.fixture_case(gold, name)
    model, _ = _model({tower: cfg}, cfg["seed"])
    rng = np.random.default_rng(41)
    if tower == "vision":
        s = cfg["patch"] * cfg["grid"]
        x = rng.integers(0, 256, size=(5, s, s, 3), dtype=np.uint8)
        enc = lambda a: model.encode_image(torch.from_numpy(a))
    else:
        x = _text_ids(rng, 5, cfg["context"], cfg["vocab"])
        enc = lambda a: model.encode_text(torch.from_numpy(a))
    perm = np.array([3, 0, 4, 1, 2])
    base = enc(x)
    _same_bits(enc(np.ascontiguousarray(x[perm])), base[torch.from_numpy(perm).cuda()], f"{tower}: permuted batch of 5")
    _same_bits(enc(np.ascontiguousarray(x[2:3])), base[2:3], f"{tower}: sample 2 alone")


# ---- the tool -----------------------------------------------------------------------------------------------------------
def _tool():
    spec = importlib.util.spec_from_file_location("diversity_table", ROOT / "tools" / "diversity_table.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run(tool, argv):
    import sys
    old, out = sys.argv, io.StringIO()
    sys.argv = ["diversity_table.py", *argv]
    try:
        with contextlib.redirect_stdout(out):
            tool.main()
    finally:
        sys.argv = old
    line = [l for l in out.getvalue().splitlines() if l.startswith("CONSISTENCY_TABLE ")]
    assert len(line) == 1
    return json.loads(line[0][len("CONSISTENCY_TABLE "):])


def test_tool_adds_the_clip_block(tmp_path):
    """tools/diversity_table.py --consistency ... --images DIR --clip synthetic: the clip block's per-category means are
    clip_consistency_table on encode_image of the same files; the Chamfer block is what a run without --images prints"""
    from PIL import Image
    from commonscenes_amd import clip as K, diversity as D
    rng = np.random.default_rng(50)
    scans = [{"scan": "roomA", "objects": {"1": "chair", "2": "chair", "3": "table", "4": "table", "5": "lamp"},
              "consistency": [[1, 2, "same as"], [3, 4, "same as"]]},
             {"scan": "roomB", "objects": {"7": "chair", "9": "chair"}, "consistency": [[9, 7, "same as"]]},
             {"scan": "roomC", "objects": {"1": "bed"}, "consistency": []}]
    classes = {"chair": 4, "table": 5}
    files = []
    for sc in scans:
        for pair in sc["consistency"]:
            for oid in pair[:2]:
                name = sc["objects"][str(oid)]
                stem = f"{name}_{classes[name]}_{oid}"
                (tmp_path / "meshes" / sc["scan"]).mkdir(parents=True, exist_ok=True)
                (tmp_path / "imgs" / sc["scan"]).mkdir(parents=True, exist_ok=True)
                v = rng.standard_normal((12, 3))
                (tmp_path / "meshes" / sc["scan"] / f"{stem}.obj").write_text(
                    "".join(f"v {a:.6f} {b:.6f} {c:.6f}\n" for a, b, c in v) + "f 1 2 3\n")
                img = tmp_path / "imgs" / sc["scan"] / f"{stem}.png"
                Image.fromarray(rng.integers(0, 256, size=(64, 64, 3), dtype=np.uint8)).save(img)
                files.append(img)
    assert len(files) == 6 and len(set(files)) == 6
    cons = tmp_path / "cons.json"
    cons.write_text(json.dumps({"scans": scans}))
    tool = _tool()
    base = ["--consistency", str(cons), "--meshes", str(tmp_path / "meshes"), "--points", "64"]
    plain = _run(tool, base)
    with_clip = _run(tool, base + ["--images", str(tmp_path / "imgs"), "--clip", "synthetic"])
    assert "clip" not in plain and with_clip["table"] == plain["table"] and with_clip["meshes"] == plain["meshes"] == 6
    model = tool.clip_model("synthetic")               # the tool's own (cached) synthetic ViT-B/32 vision tower
    assert (model.vision.width, model.vision.layers, model.vision.resolution) == (768, 12, 224) and model.text is None
    feats = model.encode_image(K.preprocess(files, 224))
    want = D.clip_consistency_table(feats, [(0, 1), (2, 3), (4, 5)], ["chair", "table", "chair"])
    print(f"clip block {with_clip['clip']}\nexpected table {want}")
    assert with_clip["clip"]["table"] == want and with_clip["clip"]["images"] == 6
    assert want["chair"]["pairs"] == 2 and want["table"]["pairs"] == 1 and want["total"]["pairs"] == 3
    assert all(np.isfinite(want[c]["clip"]) and want[c]["clip"] > 0 for c in want)
