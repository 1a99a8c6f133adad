#!/usr/bin/env python
"""tests/golden/clip_tiny.npz: both CLIP towers at four tiny configurations, computed by `transformers`' CLIP on the CPU.

Build machine only (like tools/make_goldens.py): needs `transformers`; the tests read the file and never import it.

    python tools/make_clip_goldens.py [--out tests/golden/clip_tiny.npz]

The weights are commonscenes_amd.clip.synth_clip_state_dict(cfg, seed) -- OpenAI's key layout, deterministic on every
machine -- converted HERE to the transformers layout (in_proj split into q / k / v, the two projections transposed) and loaded
into CLIPVisionModelWithProjection / CLIPTextModelWithProjection with hidden_act="quick_gelu".  Each tower runs in fp64 and in
fp32 (attention through torch's scaled_dot_product_attention: the "eager" route takes its softmax in fp32 whatever the model's
precision, which would cap the fp64 run at 1e-8).  The file holds the configs, the seeds, the inputs and both outputs -- no weights: a test regenerates them from the seed.
That the key layout and the size inference of clip.py are OpenAI's is pinned by this conversion: transformers'
convert_clip_original_pytorch_to_hf.py maps the same keys the same way.
"""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

E = 32
VISION = {"v0": dict(width=128, layers=2, patch=32, grid=2, embed=E, batch=3, seed=101),        # S = 64: 5 tokens
          "v1": dict(width=192, layers=2, patch=8, grid=5, embed=E, batch=2, seed=102)}         # S = 40: 26 tokens
TEXT = {"t0": dict(width=128, layers=2, context=16, vocab=100, embed=E, batch=4, seed=103),
        "t1": dict(width=128, layers=2, context=77, vocab=100, embed=E, batch=3, seed=104)}


def _layer(sd, src, dst, out):
    w = sd[src + "attn.in_proj_weight"].shape[1]
    for i, n in enumerate(("q_proj", "k_proj", "v_proj")):
        out[f"{dst}self_attn.{n}.weight"] = sd[src + "attn.in_proj_weight"][i * w:(i + 1) * w]
        out[f"{dst}self_attn.{n}.bias"] = sd[src + "attn.in_proj_bias"][i * w:(i + 1) * w]
    for a, b in (("attn.out_proj", "self_attn.out_proj"), ("ln_1", "layer_norm1"), ("ln_2", "layer_norm2"),
                 ("mlp.c_fc", "mlp.fc1"), ("mlp.c_proj", "mlp.fc2")):
        out[f"{dst}{b}.weight"], out[f"{dst}{b}.bias"] = sd[f"{src}{a}.weight"], sd[f"{src}{a}.bias"]


def to_hf_vision(sd, layers):
    out = {"vision_model.embeddings.class_embedding": sd["visual.class_embedding"],
           "vision_model.embeddings.patch_embedding.weight": sd["visual.conv1.weight"],
           "vision_model.embeddings.position_embedding.weight": sd["visual.positional_embedding"],
           "vision_model.pre_layrnorm.weight": sd["visual.ln_pre.weight"],
           "vision_model.pre_layrnorm.bias": sd["visual.ln_pre.bias"],
           "vision_model.post_layernorm.weight": sd["visual.ln_post.weight"],
           "vision_model.post_layernorm.bias": sd["visual.ln_post.bias"],
           "visual_projection.weight": sd["visual.proj"].t().contiguous()}
    for i in range(layers):
        _layer(sd, f"visual.transformer.resblocks.{i}.", f"vision_model.encoder.layers.{i}.", out)
    return out


def to_hf_text(sd, layers):
    out = {"text_model.embeddings.token_embedding.weight": sd["token_embedding.weight"],
           "text_model.embeddings.position_embedding.weight": sd["positional_embedding"],
           "text_model.final_layer_norm.weight": sd["ln_final.weight"],
           "text_model.final_layer_norm.bias": sd["ln_final.bias"],
           "text_projection.weight": sd["text_projection"].t().contiguous()}
    for i in range(layers):
        _layer(sd, f"transformer.resblocks.{i}.", f"text_model.encoder.layers.{i}.", out)
    return out


def _load(model, hf_sd):
    own = model.state_dict()
    extra = {k: v for k, v in own.items() if k not in hf_sd}
    assert all(k.endswith("position_ids") for k in extra), sorted(extra)         # buffers only
    assert set(hf_sd) <= set(own), sorted(set(hf_sd) - set(own))
    model.load_state_dict({**extra, **hf_sd}, strict=True)
    return model.eval()


def run_vision(c):
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    from commonscenes_amd import clip as K
    sd = K.synth_clip_state_dict({"vision": c}, c["seed"])
    s = c["patch"] * c["grid"]
    cfg = CLIPVisionConfig(hidden_size=c["width"], intermediate_size=4 * c["width"], projection_dim=c["embed"],
                           num_hidden_layers=c["layers"], num_attention_heads=c["width"] // 64, image_size=s,
                           patch_size=c["patch"], hidden_act="quick_gelu", layer_norm_eps=1e-5, attn_implementation="sdpa")
    images = np.random.default_rng(c["seed"] + 1000).integers(0, 256, size=(c["batch"], s, s, 3), dtype=np.uint8)
    outs = {}
    for name, dt in (("out64", torch.float64), ("out32", torch.float32)):
        model = _load(CLIPVisionModelWithProjection(cfg), to_hf_vision(sd, c["layers"])).to(dt)
        mean, std = torch.tensor(K.CLIP_MEAN, dtype=dt), torch.tensor(K.CLIP_STD, dtype=dt)
        pix = ((torch.from_numpy(images).to(dt) / 255) - mean) / std          # ToTensor + Normalize in the run's precision
        with torch.no_grad():
            outs[name] = model(pixel_values=pix.permute(0, 3, 1, 2).contiguous()).image_embeds.numpy()
    return images, outs


def run_text(c):
    from transformers import CLIPTextConfig, CLIPTextModelWithProjection
    from commonscenes_amd import clip as K
    sd = K.synth_clip_state_dict({"text": c}, c["seed"])
    eot = c["vocab"] - 1
    cfg = CLIPTextConfig(vocab_size=c["vocab"], hidden_size=c["width"], intermediate_size=4 * c["width"],
                         projection_dim=c["embed"], num_hidden_layers=c["layers"], num_attention_heads=c["width"] // 64,
                         max_position_embeddings=c["context"], hidden_act="quick_gelu", layer_norm_eps=1e-5,
                         bos_token_id=eot - 1, eos_token_id=eot, pad_token_id=0, attn_implementation="sdpa")
    # as clip.tokenize lays a text out: <start> words <end> then zeros; <end> has the largest id
    rng = np.random.default_rng(c["seed"] + 1000)
    t = c["context"]
    ids = np.zeros((c["batch"], t), np.int32)
    ends = [3, t - 1] + [int(v) for v in rng.integers(2, t - 1, size=c["batch"] - 2)]
    for b, e in enumerate(ends):
        ids[b, 0] = eot - 1
        ids[b, 1:e] = rng.integers(1, eot - 1, size=e - 1)
        ids[b, e] = eot
    outs = {}
    for name, dt in (("out64", torch.float64), ("out32", torch.float32)):
        model = _load(CLIPTextModelWithProjection(cfg), to_hf_text(sd, c["layers"])).to(dt)
        with torch.no_grad():
            outs[name] = model(input_ids=torch.from_numpy(ids).long()).text_embeds.numpy()
    return ids, outs


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "clip_tiny.npz"))
    a = ap.parse_args()
    blob = {}
    for name, c in {**VISION, **TEXT}.items():
        inp, outs = (run_vision if name in VISION else run_text)(c)
        keys = sorted(c)
        blob[f"{name}.cfg_keys"] = np.array(keys)
        blob[f"{name}.cfg"] = np.array([c[k] for k in keys], np.int64)
        blob[f"{name}.input"] = inp
        blob[f"{name}.out64"] = outs["out64"].astype(np.float64)
        blob[f"{name}.out32"] = outs["out32"].astype(np.float32)
        d = outs["out64"] - outs["out32"].astype(np.float64)
        print(f"{name}: {c}  input {inp.shape}  out {outs['out64'].shape}  |out| {np.linalg.norm(outs['out64']):.4f}  "
              f"CPU-fp32 rel-L2 {np.linalg.norm(d) / np.linalg.norm(outs['out64']):.3e}")
    np.savez_compressed(a.out, **blob)
    print(f"wrote {a.out}: {Path(a.out).stat().st_size} bytes")


if __name__ == "__main__":
    main()
