// cs_unet_*: the whole UNet forward of the shape-branch denoiser as ONE native call over a packed weight arena
// (SURVEY 8b "cs_unet_step").  Host-side C++ only sequences the library's own kernels (cs_conv_gemm,
// cs_groupnorm_*, cs_layernorm, cs_attn_selfattn*, cs_copy_rows, ...) -- the same launches, in the same order,
// with the same arguments as commonscenes_amd/unet.py::DiffusionUNet.forward_ndhwc, so both drivers produce
// identical bits -- and owns nothing on the device: the caller passes the raw parameters, the arena, the
// workspace and the stream.
//
// Reference being replaced:
//   model/networks/diffusion_networks/openai_model_3d.py:452-789   UNet3DModel.__init__ / forward
//   model/networks/diffusion_networks/attention.py:154-351         CrossAttention / BasicTransformerBlock /
//                                                                  SpatialTransformer3D
//   model/networks/diffusion_networks/network.py:20-42             DiffusionUNet.forward (crossattn branch)
// Scope: the shipped config family (dims=3 i.e. H,W-only resampling, use_spatial_transformer, one transformer
// block per SpatialTransformer3D, ONE context token -- SURVEY F4: cross-attention over a single key is the
// per-sample row vector to_out(to_v(ctx)), computed once per sampling run by cs_unet_context).
#include "cs_driver.h"

namespace {

enum Kind { CONV_IN, RES, ATTN, ATTNBLOCK, DOWN, UP };

struct Layer {
  Kind kind;
  int cin, cout;
  int g[8];
  int n[4];
  int emb_lo = 0;      // RES: column offset into the batched emb_layers projection
  // RES of an output block whose skip half is shared by the guidance halves (unet.py::_pack "channel-split ResBlocks"):
  // split channel ks (> 0), channels of h, and in_layers.2 as two GEMMs {over channels [0, ks), over channels [ks, C)}; the
  // 1x1x1 skip_connection stays whole
  int ks = 0, ch_h = 0;
  int gsp[2] = {-1, -1};
  int ctx_off = 0;     // ATTN: column offset into the context-vector block
  bool fused_geglu = false;
  // ATTN / ATTNBLOCK, F16X3: first of this block's float slots (34 / 4) behind the plan's |w| maxima, where cs_unet_pack
  // leaves the statistics of the raw weights that bound the operands born inside the block
  int stat_slot = -1;
  // ATTN: those statistics (cs_transformer_static_scales); ctx_max = the largest |entry| of the block's cross-attention
  // row vector of the current run (cs_unet_set_context_bounds), 0 until the host sets it
  CsTransformerStats ts;
  bool has_ts = false;
  float ctx_max = 0.f;
  // ATTNBLOCK: max row 2-norm of the fused qkv weight and max |bias| (cs_attnblock_static_scales); ab_w / ab_b = the raw
  // parameters they are taken from
  int ab_w = -1, ab_b = -1;
  float ab_l2max = 0.f, ab_bmax = 0.f;
};

}  // namespace

struct cs_unet : Plan {
  CsUnetConfig cfg;
  std::vector<std::vector<Layer>> inp, out;
  std::vector<Layer> mid;
  int g_te0 = -1, g_te2 = -1, g_emb_all = -1, g_out = -1, n_out = -1;
  int emb_total = 0, ctx_total = 0, cpad_in = 4, ch_final = 0;
  int64_t split_min_rows = 65536;      // channel-split ResBlocks only from this many rows (unet.py: split_min_rows)
};

namespace {

// every layer in block order: input blocks, middle, output blocks (U = cs_unet or const cs_unet)
template <class U, class F>
void for_each_layer(U& u, F&& fn) {
  for (auto& layers : u.inp)
    for (auto& l : layers) fn(l);
  for (auto& l : u.mid) fn(l);
  for (auto& layers : u.out)
    for (auto& l : layers) fn(l);
}

bool has_attn(const std::vector<Layer>& layers) {
  for (const Layer& l : layers)
    if (l.kind == ATTN || l.kind == ATTNBLOCK) return true;
  return false;
}

// ---------------------------------------------------------------------------------------------------------
// plan construction (mirrors unet.py::unet_blocks / unet_param_shapes / DiffusionUNet._pack)
// ---------------------------------------------------------------------------------------------------------
struct EmbAcc {
  std::vector<Piece> w, b;
  int total = 0;
};

Layer make_res(cs_unet& u, const std::string& p, int cin, int cout, int ted, EmbAcc& emb) {
  Layer l{};
  l.kind = RES;
  l.cin = cin;
  l.cout = cout;
  l.n[0] = add_norm(u, p + ".in_layers.0", cin);
  l.g[0] = add_layer_gemm(u, p + ".in_layers.2", cout, cin, 3);
  int wp, bp;
  add_wb(u, p + ".emb_layers.1", cout, ted, 0, true, wp, bp);
  emb.w.push_back({wp, 0, cout});
  emb.b.push_back({bp, 0, cout});
  l.emb_lo = emb.total;
  emb.total += cout;
  l.n[1] = add_norm(u, p + ".out_layers.0", cout);
  l.g[1] = add_layer_gemm(u, p + ".out_layers.3", cout, cout, 3);
  l.g[2] = (cin != cout) ? add_layer_gemm(u, p + ".skip_connection", cout, cin, 1) : -1;
  return l;
}

Layer make_attn(cs_unet& u, const std::string& p, int c, int ctx_dim, bool f16x3) {
  Layer l{};
  l.kind = ATTN;
  l.cin = l.cout = c;
  l.n[0] = add_norm(u, p + ".norm", c);
  l.g[0] = add_layer_gemm(u, p + ".proj_in", c, c, 1);
  const std::string t = p + ".transformer_blocks.0";
  int q, k, v, dummy;
  add_wb(u, t + ".attn1.to_q", c, c, 0, false, q, dummy);
  add_wb(u, t + ".attn1.to_k", c, c, 0, false, k, dummy);
  add_wb(u, t + ".attn1.to_v", c, c, 0, false, v, dummy);
  l.g[1] = add_gemm(u, {{q, 0, c}, {k, 0, c}, {v, 0, c}}, {}, 3 * c, c, 0);      // fused q|k|v projection
  l.g[2] = add_layer_gemm(u, t + ".attn1.to_out.0", c, c, 0);
  // attn2.to_q / to_k are parameters of the reference module but unused with one context token (softmax == 1)
  add_wb(u, t + ".attn2.to_q", c, c, 0, false, q, dummy);
  add_wb(u, t + ".attn2.to_k", c, ctx_dim, 0, false, k, dummy);
  l.g[3] = add_layer_gemm(u, t + ".attn2.to_v", c, ctx_dim, 0, false);
  l.g[4] = add_layer_gemm(u, t + ".attn2.to_out.0", c, c, 0);
  int wp, bp;
  add_wb(u, t + ".ff.net.0.proj", 8 * c, c, 0, true, wp, bp);
  const int hdim = 4 * c;
  l.fused_geglu = f16x3 && (hdim % 112 == 0);
  if (l.fused_geglu) {
    // output columns interleaved per 224-column tile as [x (112) | gate (112)]  (ops.pack_geglu_weight)
    std::vector<Piece> w, b;
    for (int blk = 0; blk < hdim / 112; ++blk) {
      w.push_back({wp, blk * 112, 112});
      w.push_back({wp, hdim + blk * 112, 112});
      b.push_back({bp, blk * 112, 112});
      b.push_back({bp, hdim + blk * 112, 112});
    }
    l.g[5] = add_gemm(u, w, b, 8 * c, c, 0);
  } else {
    l.g[5] = add_gemm(u, {{wp, 0, 8 * c}}, {{bp, 0, 8 * c}}, 8 * c, c, 0);
  }
  l.g[6] = add_layer_gemm(u, t + ".ff.net.2", c, 4 * c, 0);
  l.n[1] = add_norm(u, t + ".norm1", c);
  l.n[2] = add_norm(u, t + ".norm2", c);
  l.n[3] = add_norm(u, t + ".norm3", c);
  l.g[7] = add_layer_gemm(u, p + ".proj_out", c, c, 1);
  l.ctx_off = u.ctx_total;
  u.ctx_total += c;
  return l;
}

// AttentionBlock (openai_model_3d.py:316-366; the concat family, use_spatial_transformer=False): GroupNorm ->
// Conv1d(k=1) qkv -> QKVAttentionLegacy -> Conv1d(k=1) proj_out + x.  The legacy module reads the 3C qkv channels
// as [head][q|k|v][ch]; the packed weight's rows are gathered as [q|k|v][head][ch] instead, so q, k, v are plain
// column slices for the flash kernel (same permutation as unet.py::_pack).
Layer make_attnblock(cs_unet& u, const std::string& p, int c, int heads) {
  Layer l{};
  l.kind = ATTNBLOCK;
  l.cin = l.cout = c;
  l.n[0] = add_norm(u, p + ".norm", c);
  const int wq = add_param(u, p + ".qkv.weight", {3 * c, c, 1});
  const int bq = add_param(u, p + ".qkv.bias", {3 * c});
  const int ch = c / heads;
  std::vector<Piece> w, b;
  for (int j = 0; j < 3; ++j)
    for (int h = 0; h < heads; ++h) {
      w.push_back({wq, h * 3 * ch + j * ch, ch});
      b.push_back({bq, h * 3 * ch + j * ch, ch});
    }
  l.g[0] = add_gemm(u, w, b, 3 * c, c, 0);
  l.ab_w = wq;
  l.ab_b = bq;
  const int wo = add_param(u, p + ".proj_out.weight", {c, c, 1});
  const int bo = add_param(u, p + ".proj_out.bias", {c});
  l.g[1] = add_gemm(u, {{wo, 0, c}}, {{bo, 0, c}}, c, c, 0);
  return l;
}

bool in_list(const int32_t* v, int n, int x) {
  for (int i = 0; i < n; ++i)
    if (v[i] == x) return true;
  return false;
}

int build(cs_unet& u) {
  const CsUnetConfig& c = u.cfg;
  if (c.model_channels <= 0 || c.model_channels % 32 || c.num_res_blocks <= 0 || c.n_mult <= 0 || c.n_mult > 8 ||
      c.n_attn_res < 0 || c.n_attn_res > 8 || c.num_heads <= 0 || c.in_channels <= 0 ||
      (c.use_spatial_transformer && c.context_dim <= 0) || (c.dims != 3 && c.dims != 4) ||
      c.out_channels <= 0 || c.d <= 0 || c.h <= 0 || c.w <= 0)
    return CS_EINVAL;
  if (c.math != CS_MATH_FP32 && c.math != CS_MATH_F16X3) return CS_EINVAL;
  if ((c.h >> (c.n_mult - 1)) << (c.n_mult - 1) != c.h || (c.w >> (c.n_mult - 1)) << (c.n_mult - 1) != c.w)
    return CS_EINVAL;
  if (c.dims == 4 && (c.d >> (c.n_mult - 1)) << (c.n_mult - 1) != c.d) return CS_EINVAL;
  auto attn_layer = [&](const std::string& q, int chn) {
    return c.use_spatial_transformer ? make_attn(u, q, chn, c.context_dim, c.math == CS_MATH_F16X3)
                                     : make_attnblock(u, q, chn, c.num_heads);
  };
  const int mc = c.model_channels, ted = 4 * mc, nres = c.num_res_blocks;
  const std::string P = "diffusion_net.";
  u.cpad_in = (c.in_channels + 3) / 4 * 4;
  u.g_te0 = add_layer_gemm(u, P + "time_embed.0", ted, mc, 0);
  u.g_te2 = add_layer_gemm(u, P + "time_embed.2", ted, ted, 0);
  EmbAcc emb;
  std::vector<int> chans;
  int ch = mc, ds = 1, bi = 0;
  {
    Layer l{};
    l.kind = CONV_IN;
    l.cin = c.in_channels;
    l.cout = mc;
    l.g[0] = add_layer_gemm(u, P + "input_blocks.0.0", mc, c.in_channels, 3, true, u.cpad_in);
    u.inp.push_back({l});
    chans.push_back(mc);
    bi = 1;
  }
  for (int level = 0; level < c.n_mult; ++level) {
    const int m = c.channel_mult[level];
    if (m <= 0) return CS_EINVAL;
    for (int r = 0; r < nres; ++r) {
      const std::string bp = P + "input_blocks." + std::to_string(bi++);
      std::vector<Layer> layers;
      layers.push_back(make_res(u, bp + ".0", ch, m * mc, ted, emb));
      ch = m * mc;
      if (ch % c.num_heads) return CS_EINVAL;
      if (in_list(c.attention_resolutions, c.n_attn_res, ds))
        layers.push_back(attn_layer(bp + ".1", ch));
      u.inp.push_back(layers);
      chans.push_back(ch);
    }
    if (level != c.n_mult - 1) {
      const std::string bp = P + "input_blocks." + std::to_string(bi++);
      Layer l{};
      l.kind = DOWN;
      l.cin = l.cout = ch;
      l.g[0] = add_layer_gemm(u, bp + ".0.op", ch, ch, 3);
      u.inp.push_back({l});
      chans.push_back(ch);
      ds *= 2;
    }
  }
  u.mid.push_back(make_res(u, P + "middle_block.0", ch, ch, ted, emb));
  u.mid.push_back(attn_layer(P + "middle_block.1", ch));
  u.mid.push_back(make_res(u, P + "middle_block.2", ch, ch, ted, emb));
  int oi = 0;
  for (int level = c.n_mult - 1; level >= 0; --level) {
    const int m = c.channel_mult[level];
    for (int i = 0; i <= nres; ++i) {
      const int ich = chans.back();
      chans.pop_back();
      const std::string bp = P + "output_blocks." + std::to_string(oi++);
      std::vector<Layer> layers;
      layers.push_back(make_res(u, bp + ".0", ch + ich, mc * m, ted, emb));
      ch = mc * m;
      if (in_list(c.attention_resolutions, c.n_attn_res, ds))
        layers.push_back(attn_layer(bp + ".1", ch));
      if (level && i == nres) {
        Layer l{};
        l.kind = UP;
        l.cin = l.cout = ch;
        l.g[0] = add_layer_gemm(u, bp + "." + std::to_string(layers.size()) + ".conv", ch, ch, 3, true, 0,
                                c.dims == 3 ? 3 : 7);      // Upsample: H, W doubled (dims = 3) or D, H, W
        layers.push_back(l);
        ds /= 2;
      }
      u.out.push_back(layers);
    }
  }
  // channel-split ResBlocks: output block j reads the skip of input block (n_in - 1 - j); the ones from the context-free
  // prefix of the input path (before the first attention block) are shared by the guidance halves.  Same rule and same
  // split point as unet.py::_pack.
  if (c.use_spatial_transformer && !cs_debug()->no_cfg_split) {
    size_t n_prefix = 0;
    while (n_prefix < u.inp.size() && !has_attn(u.inp[n_prefix])) ++n_prefix;
    for (size_t j = 0; j < u.out.size(); ++j) {
      const size_t src = u.inp.size() - 1 - j;
      Layer& l = u.out[j][0];
      if (src >= n_prefix || l.kind != RES || l.g[2] < 0) continue;
      const int ch_s = u.inp[src].back().cout, C = l.cin, ch_h = C - ch_s, cpg = C / 32;
      if (C % 32) continue;
      int ks = 0;
      for (int k = (ch_h + 15) / 16 * 16; k < C; k += 16)
        if ((k / cpg) * cpg >= ch_h) {
          ks = k;
          break;
        }
      if (!ks || (C - ks) % 16) continue;
      // in_layers.2 (3x3x3) as two GEMMs; the unsplit one stays packed: small batches take it, see split_min_rows
      const int gi = l.g[0];
      const int wp = u.gemms[gi].w[0].param, bp = u.gemms[gi].b.empty() ? -1 : u.gemms[gi].b[0].param;
      const int k = u.gemms[gi].k;
      l.gsp[0] = add_gemm_cin_range(u, wp, bp, l.cout, C, k, 0, ks);
      l.gsp[1] = add_gemm_cin_range(u, wp, -1, l.cout, C, k, ks, C);
      l.ks = ks;
      l.ch_h = ch_h;
    }
  }
  u.split_min_rows = cs_debug()->cfg_split_min_rows;
  u.ch_final = ch;
  u.n_out = add_norm(u, P + "out.0", ch);
  u.g_out = add_layer_gemm(u, P + "out.2", c.out_channels, mc, 3, true, 0, 0, /*tapcol=*/true);
  // all ResBlock emb_layers Linears read the same SiLU(emb): one GEMM [nb, 4mc] x [4mc, sum(cout)]
  u.g_emb_all = add_gemm(u, emb.w, emb.b, emb.total, ted, 0);
  u.emb_total = emb.total;

  // F16X3: 34 float slots per transformer block for the static-bound statistics (cs_unet_pack), then 4 per AttentionBlock
  int nblk = 0, nab = 0;
  for_each_layer(u, [&](const Layer& l) {
    nblk += l.kind == ATTN;
    nab += l.kind == ATTNBLOCK;
  });
  u.extra_slots = (c.math == CS_MATH_F16X3) ? 34 * nblk + 4 * nab : 0;
  layout_arena(u);
  if (u.extra_slots) {
    int k = 0, k2 = 0;
    for_each_layer(u, [&](Layer& l) {
      if (l.kind == ATTN) l.stat_slot = u.extra_slot0 + 34 * k++;
      if (l.kind == ATTNBLOCK) l.stat_slot = u.extra_slot0 + 34 * nblk + 4 * k2++;
    });
  }
  return CS_OK;
}

struct Exec : ExecBase {
  const cs_unet& u;
  Exec(const cs_unet& u_, const void* arena_, void* ws_, int64_t ws_bytes_, bool dry_, hipStream_t st_)
      : ExecBase(u_, arena_, ws_, ws_bytes_, dry_, st_), u(u_) {}
  int64_t in_bound_off = -1;      // bound slot of the latent (conv_in's operand), set by forward()

  // unet.py::_res
  Act res_block(const Layer& l, const Act& x, const Buf& semb) {
    const int rows = x.d * x.h * x.w;
    const bool own_skip = l.g[2] >= 0;
    // xb: the skip conv below reads x RAW -- the GroupNorm's finalize kernel leaves x's magnitude bound on the way.
    // x.d, x.h, x.w: where the conv takes the Winograd-W route the GroupNorm emits that operand
    int64_t xb = -1;
    Buf hn = groupnorm(x.b, l.n[0], x.nb, 1e-5f, CS_ACT_SILU, 32, l.g[0], own_skip ? &xb : nullptr, x.d, x.h, x.w);
    // stats(): the conv's epilogue leaves the partial sums the next GroupNorm takes its statistics from
    Buf h1 = gemm(hn, l.g[0], x.nb, x.d, x.h, x.w, GemmOpts().row_vector(at(semb, l.emb_lo), semb.c, rows).stats());
    release(hn);
    Buf hn2 = groupnorm(h1, l.n[1], x.nb, 1e-5f, CS_ACT_SILU, 32, l.g[1], nullptr, x.d, x.h, x.w);
    release(h1);
    // the skip conv reads the RAW residual stream: operand scale from the tensor's actual range (x_bound=)
    Buf skip;
    if (own_skip) skip = gemm(x.b, l.g[2], x.nb, x.d, x.h, x.w, GemmOpts().bound(xb));
    Act o = x;
    const Buf& sk = own_skip ? skip : x.b;
    o.b = gemm(hn2, l.g[1], x.nb, x.d, x.h, x.w, GemmOpts().residual(sk, sk.c).stats());
    release(hn2);
    release(skip);
    return o;
  }

  // ResBlock whose input is the concatenation x = [h | skip] with the skip half shared by nb / sk.nb groups of samples
  // (the guidance halves): in_layers' conv is evaluated as a GEMM over channels [0, ks) at the full batch plus a GEMM
  // over channels [ks, C) -- whole GroupNorm groups of skip channels -- at batch sk.nb, which enters the first one's
  // epilogue as a residual (the 1x1x1 skip_connection stays whole).  Same launches, in the same order, as
  // unet.py::_res_split.
  Act res_block_split(const Layer& l, const Act& x, const Act& sk, const Buf& semb) {
    const int rows = x.d * x.h * x.w, C = x.b.c, ks = l.ks, cs = C - ks, off = ks - l.ch_h, cpg = C / 32;
    const int nb = x.nb, nbs = sk.nb, ch_s = sk.b.c, cout = l.cout;
    Act o = x;
    if (nbs <= 0 || nb % nbs || ch_s != C - l.ch_h) {
      chk(CS_EINVAL);
      return o;
    }
    // GroupNorm ranges: the statistics of the whole concatenation once (+ its magnitude bound for the skip conv), then
    // channels [ch0, ch0 + c) of nbr samples from sample0 on, read at xp with row stride ldx, in the form conv_gi wants
    // for a launch over nbs samples (wn: wants_wino's answer)
    const Norm& n0 = pl.norms[l.n[0]];
    GnStats s = gn_stats_alloc(x.b, nb, 32, true);
    gn_stats_run(x.b, nb, 1e-5f, 32, s);
    release(s.wsb);
    auto gn_range = [&](const float* xp, int ldx, int nbr, int64_t sample0, int ch0, int c, int conv_gi, int wn) {
      Buf y = gn_out(n0, (int64_t)nbr * rows, c, nbr, cpg, wn, conv_gi, (int64_t)nbs * rows);
      gn_emit(xp, ldx, at(s.stats, sample0 * 32 * 2), n0, y, nbr, rows, x.d, x.h, x.w, 32, cpg, ch0, CS_ACT_SILU);
      return y;
    };
    const int wn_h = wants_wino(l.gsp[0], nbs, x.d, x.h, x.w), wn_s = wants_wino(l.gsp[1], nbs, x.d, x.h, x.w);
    // the h channels [0, ks): one operand for the whole batch -- the Winograd-W form is emitted per guidance half instead
    Buf a_h;
    if (!wn_h) a_h = gn_range(at(x.b), C, nb, 0, 0, ks, l.gsp[0], 0);
    // shared half: the skip channels [ks, C), read from the skip tensor itself, through their GEMM at batch nbs
    Buf a_s = gn_range(at(sk.b, off), ch_s, nbs, 0, ks, cs, l.gsp[1], wn_s);
    Buf y_s = alloc(sk.b.rows, cout);
    if (ok()) gemm_view(view(a_s), l.gsp[1], nbs, x.d, x.h, x.w, at(y_s), cout);
    release(a_s);
    // per-guidance-half GEMMs over the h channels: + the half's emb row vectors, + the shared half as the residual
    Buf h1 = alloc(x.b.rows, cout);
    for (int g = 0; g < nb / nbs && ok(); ++g) {
      const int64_t s0 = (int64_t)g * nbs, r0 = s0 * rows;
      GemmOpts opt;
      opt.row_vector(at(semb, s0 * semb.c + l.emb_lo), semb.c, rows).residual(y_s, cout);
      if (wn_h) {
        Buf a_g = gn_range(at(x.b, r0 * C), C, nbs, s0, 0, ks, l.gsp[0], wn_h);
        if (ok()) gemm_view(view(a_g), l.gsp[0], nbs, x.d, x.h, x.w, at(h1, r0 * cout), cout, opt);
        release(a_g);
      } else {
        gemm_view(view(a_h, r0), l.gsp[0], nbs, x.d, x.h, x.w, at(h1, r0 * cout), cout, opt);
      }
    }
    release(s.stats);
    release(a_h);
    release(y_s);
    Buf skc = gemm(x.b, l.g[2], nb, x.d, x.h, x.w, GemmOpts().bound(s.bound));
    Buf hn2 = groupnorm(h1, l.n[1], nb, 1e-5f, CS_ACT_SILU, 32, l.g[1], nullptr, x.d, x.h, x.w);
    release(h1);
    o.b = gemm(hn2, l.g[1], nb, x.d, x.h, x.w, GemmOpts().residual(skc, cout).stats());
    release(hn2);
    release(skc);
    return o;
  }

  // twin (forward: the late guidance split): x holds ONE copy per (x, t) pair and everything up to the attn1.to_out product
  // runs on it; the cross-attention row vector -- the first term that differs between the guidance halves -- enters in
  // cs_twin_layernorm_pair16, which writes t1 and norm3's operand pair for both halves; the rest runs at 2 x.nb samples
  Act attn_block(const Layer& l, const Act& x, const float* ctxvec, bool twin = false) {
    const int c = l.cin, heads = u.cfg.num_heads, dh = c / heads;
    const int n = x.d * x.h * x.w;
    const int nbo = twin ? 2 * x.nb : x.nb;
    const int64_t rows = (int64_t)nbo * n;
    Buf xn = groupnorm(x.b, l.n[0], x.nb, 1e-6f, CS_ACT_NONE);
    Buf t0 = linear(xn, l.g[0]);
    release(xn);
    Buf n1 = layernorm(t0, l.n[1]);
    Buf qkv = linear(n1, l.g[1]);
    release(n1);
    Buf a = alloc(t0.rows, c);
    // static bounds of the operands born inside the block (unet.py::_static_scales; the ONE rule in cs_plan.hip)
    float ss[12];
    const Norm& gnn = pl.norms[l.n[0]];
    const bool stat = l.has_ts && u.cfg.math == CS_MATH_F16X3 && !cs_debug()->no_static_scales && ctxvec &&
                      cs_transformer_static_scales(&l.ts, c, n, heads, gnn.gmax, gnn.bmax, l.ctx_max, ss) == CS_OK;
    self_attention(qkv, a, x.nb, n, heads, dh, c, (float)std::pow((double)dh, -0.5), stat ? ss : nullptr);
    if (stat) a.a_scale = ss[3];
    release(qkv);
    // one context token: attn2(x) == to_out(to_v(ctx)) for every query row -> a row vector in this epilogue
    const float* rv = ctxvec ? ctxvec + l.ctx_off : nullptr;
    Buf t1, n3;
    if (twin) {
      Buf y = linear(a, l.g[2]);
      cs_conv_plan_copies(1);      // (forward set 2: the launches up to here stand for both guidance halves)
      release(a);
      const Norm& nm = pl.norms[l.n[3]];
      t1 = alloc(rows, c);
      n3 = alloc(rows, c);
      n3.pair = true;
      n3.a_scale = norm_a_scale(nm.gmax, nm.bmax, c);
      if (ok() && !dry)
        chk(cs_twin_layernorm_pair16(p(y), rv, p(t0), wf(nm.g_off), wf(nm.b_off), p(t1), p(n3), (int)y.rows, c, c, u.ctx_total, n, c,
                                     c, c, 1e-5f, n3.a_scale, status, st));
      release(y);
      release(t0);
    } else {
      t1 = linear(a, l.g[2], GemmOpts().row_vector(rv, u.ctx_total, n).residual(t0, c));
      release(a);
      release(t0);
      n3 = layernorm(t1, l.n[3]);
    }
    Buf gg;
    // gg's only reader is ff.net.2, t2's only reader proj_out: both producers write the operand pair where they can
    // (unet.py::_attn, out_pair=)
    const float pairs = u.cfg.math == CS_MATH_F16X3 ? 16.f : 0.f;
    const float pair_gg = (pairs > 0.f && stat) ? ss[4] : pairs, pair_t2 = (pairs > 0.f && stat) ? ss[5] : pairs;
    if (l.fused_geglu) {
      gg = linear(n3, l.g[5], GemmOpts().activation(CS_ACT_GEGLU).pair(pair_gg));   // tile 0: a 224-column tile for the gate
    } else {
      Buf ff = linear(n3, l.g[5]);
      gg = alloc(rows, 4 * c);
      if (ok() && !dry) chk(cs_geglu(p(ff), p(gg), (int)rows, 4 * c, 8 * c, 4 * c, st));
      release(ff);
    }
    if (stat && !gg.pair) gg.a_scale = ss[4];      // (a producer that could not emit the pair hands over fp32)
    release(n3);
    Buf t2 = linear(gg, l.g[6], GemmOpts().residual(t1, c).pair(pair_t2));
    if (stat && !t2.pair) t2.a_scale = ss[5];
    release(gg);
    release(t1);
    Act o = x;
    o.nb = nbo;
    // proj_out's residual is the block's input: one copy per guidance half
    Buf x2;
    if (twin) {
      x2 = alloc(rows, c);
      for (int g = 0; g < 2 && ok() && !dry; ++g)
        chk(cs_copy_rows(p(x.b), p(x2) + (int64_t)g * x.b.rows * c, x.b.rows, c, c, c, st));
    }
    // (nbo samples of n tokens: what the epilogue's GroupNorm partial sums are tiled by -- unet.py::_attn, spatial=)
    o.b = gemm(t2, l.g[7], nbo, n, 1, 1, GemmOpts().residual(twin ? x2 : x.b, c).stats());
    release(t2);
    release(x2);
    return o;
  }

  Act attnblock(const Layer& l, const Act& x) {
    const int c = l.cin, heads = u.cfg.num_heads, dh = c / heads;
    const int n = x.d * x.h * x.w;
    const int64_t rows = (int64_t)x.nb * n;
    Buf xn = groupnorm(x.b, l.n[0], x.nb, 1e-5f, CS_ACT_NONE);
    Buf qkv = linear(xn, l.g[0]);
    release(xn);
    Buf a = alloc(rows, c);
    // static operand scales of q / k / v and of the attention output (unet.py::_attnblock: the same rule and statistics)
    float ss[4];
    const float qks = (float)std::pow((double)dh, -0.5);
    const bool stat = attnblock_scales(l.n[0], (int64_t)n * (c / 32), c, l.ab_l2max, l.ab_bmax, qks, ss);
    self_attention(qkv, a, x.nb, n, heads, dh, c, qks, stat ? ss : nullptr);
    if (stat) a.a_scale = ss[3];
    release(qkv);
    Act o = x;
    o.b = gemm(a, l.g[1], x.nb, n, 1, 1, GemmOpts().residual(x.b, c).stats());
    release(a);
    return o;
  }

  // runs the layers of one block; `keep_in` says whether the caller still needs the input buffer
  // twin: h holds one copy per guidance pair and the block's last layer is the transformer block that splits (attn_block)
  Act run(const std::vector<Layer>& layers, Act h, const Buf& semb, const float* ctxvec, bool keep_in,
          const Act* split_skip = nullptr, bool twin = false) {
    bool owned = !keep_in;
    if (twin) cs_conv_plan_copies(2);      // shared launches take the duplicated batch's launch rules: the same bits
    for (const Layer& l : layers) {
      Act o;
      if (l.kind == RES && l.ks > 0 && split_skip && &l == &layers[0]) {
        o = res_block_split(l, h, *split_skip, semb);
        if (owned) release(h.b);
        h = o;
        owned = true;
        continue;
      }
      switch (l.kind) {
        case CONV_IN:
          o = h;
          o.b = gemm(h.b, l.g[0], h.nb, h.d, h.h, h.w, GemmOpts().stats().bound(in_bound_off));
          break;
        case RES:
          o = res_block(l, h, semb);
          break;
        case ATTN:
          o = attn_block(l, h, ctxvec, twin && &l == &layers.back());
          break;
        case ATTNBLOCK:
          o = attnblock(l, h);
          break;
        case DOWN: {   // dims == 3: inner two dims only (openai_model_3d.py:188); dims == 4: all three
          const int sd = u.cfg.dims == 3 ? 1 : 2;
          o = h;
          // (Down / Upsample read the RAW stream with no GroupNorm in front: its bound from the producers' partials)
          o.b = gemm(h.b, l.g[0], h.nb, h.d, h.h, h.w, GemmOpts().stride(2, sd).stats().bound(range_bound(h.b, h.nb)));
          o.d = h.d / sd;
          o.h = h.h / 2;
          o.w = h.w / 2;
          break;
        }
        case UP: {     // nearest x2 folded into the conv's addressing (openai_model_3d.py:148-157)
          const int ud = u.cfg.dims == 3 ? 0 : 1;
          o = h;
          o.b = gemm(h.b, l.g[0], h.nb, h.d, h.h, h.w, GemmOpts().upsample(1, ud).stats().bound(range_bound(h.b, h.nb)));
          o.d = h.d << ud;
          o.h = h.h * 2;
          o.w = h.w * 2;
          break;
        }
      }
      if (owned) release(h.b);
      h = o;
      owned = true;
    }
    if (twin) cs_conv_plan_copies(1);
    return h;
  }

  // may this block split the guidance halves INSIDE its transformer block (ResBlocks, then one transformer block on the
  // one-token row-vector route whose norm3 writes the operand pair)?  unet.py::forward_ndhwc asks the same
  bool late_split(const std::vector<Layer>& layers) const {
    if (u.cfg.math != CS_MATH_F16X3 || cs_debug()->no_cfg_late_split || cs_debug()->no_pair16) return false;
    if (layers.size() < 2 || layers.back().kind != ATTN || layers.back().cin % 16) return false;
    for (size_t i = 0; i + 1 < layers.size(); ++i)
      if (layers[i].kind != RES) return false;
    return true;
  }

  Buf duplicate(const Buf& a) {   // torch.cat([a, a], dim=0); the copy gets its own copy of the producer's partials
    Buf o = alloc(2 * a.rows, a.c);
    if (a.nseg == 1 && a.seg[0].valid()) {
      o.seg[0] = dup_stat(a.seg[0]);
      o.nseg = o.seg[0].valid() ? 1 : 0;
    }
    if (ok() && !dry) {
      const size_t bytes = (size_t)a.rows * a.c * 4;
      if (hipMemcpyAsync(p(o), p(a), bytes, hipMemcpyDeviceToDevice, st) != hipSuccess ||
          hipMemcpyAsync((char*)p(o) + bytes, p(a), bytes, hipMemcpyDeviceToDevice, st) != hipSuccess)
        chk(CS_EINVAL);
    }
    return o;
  }
};

int forward(Exec& e, const float* x_ncdhw, const int64_t* t, const float* ctxvec, float* eps_ncdhw, int nbx,
            int cfg_pairs) {
  const cs_unet& u = e.u;
  const CsUnetConfig& c = u.cfg;
  const int S = c.d * c.h * c.w;
  e.sync_begin();         // split-K arrival counters (CsConvGemm.splitk_sync)
  e.amax_begin(64);       // magnitude-bound slots of this forward (unet.py::forward_ndhwc: self._amax)
  Buf temb = e.alloc(nbx, c.model_channels);
  if (e.ok() && !e.dry) e.chk(cs_timestep_embedding(t, e.p(temb), nbx, c.model_channels, 10000.0f, e.st));
  Buf e1 = e.linear(temb, u.g_te0, GemmOpts().activation(CS_ACT_SILU));
  e.release(temb);
  // every consumer of `emb` is emb_layers = SiLU -> Linear (openai_model_3d.py:257-263): keep SiLU(emb)
  Buf e2 = e.linear(e1, u.g_te2, GemmOpts().activation(CS_ACT_SILU));
  e.release(e1);
  Buf semb = e.linear(e2, u.g_emb_all);
  e.release(e2);
  Act h;
  h.nb = nbx; h.d = c.d; h.h = c.h; h.w = c.w;
  h.b = e.alloc((int64_t)nbx * S, u.cpad_in);
  if (e.ok() && !e.dry) e.chk(cs_nchw_to_ndhwc(x_ncdhw, e.p(h.b), nbx, c.in_channels, S, u.cpad_in, e.st));
  // conv_in reads the RAW latent -- its exact max |.| goes to a bound slot (unet.py::forward_ndhwc: ops.absmax_bound)
  e.in_bound_off = e.amax_slot();
  if (e.in_bound_off >= 0 && e.ok() && !e.dry)
    e.chk(cs_absmax(e.p(h.b), (int64_t)nbx * S * u.cpad_in, e.bound_ptr(e.in_bound_off), e.st));
  bool shared = cfg_pairs != 0;
  auto split = [&](bool h_retained) {   // first context-dependent block: one copy per guidance half, [uc; c]
    Buf h2 = e.duplicate(h.b);
    if (!h_retained) e.release(h.b);     // otherwise it lives on in `hs` as a (shared) skip tensor
    h.b = h2;
    h.nb *= 2;
    Buf s2 = e.duplicate(semb);
    e.release(semb);
    semb = s2;
    shared = false;
  };
  std::vector<Act> hs;
  bool first = true;
  for (const auto& layers : u.inp) {
    bool keep = !first;           // the block input is the previous block's output, retained in `hs`
    bool twin = false;
    if (shared && has_attn(layers)) {
      twin = e.late_split(layers);
      if (!twin) {
        split(!first);            // the duplicate is a fresh buffer this block may consume
        keep = false;
      }
    }
    h = e.run(layers, h, semb, ctxvec, keep, nullptr, twin);
    if (twin) {                   // the block's output holds both halves; the later blocks want their emb rows too
      Buf s2 = e.duplicate(semb);
      e.release(semb);
      semb = s2;
      shared = false;
    }
    hs.push_back(h);
    first = false;
    if (!e.ok()) return e.rc;
  }
  bool keep_mid = true;           // h is hs.back()
  if (shared) {
    split(true);
    keep_mid = false;
  }
  h = e.run(u.mid, h, semb, ctxvec, keep_mid);
  for (const auto& layers : u.out) {
    Act sk = hs.back();
    hs.pop_back();
    // torch.cat([h, skip], channel); a shared (nbx-sized) skip tensor feeds both guidance halves
    Act cat = h;
    cat.b = e.alloc(h.b.rows, h.b.c + sk.b.c);
    if (e.ok() && !e.dry) {
      e.chk(cs_copy_rows(e.p(h.b), e.p(cat.b), h.b.rows, h.b.c, h.b.c, cat.b.c, e.st));
      const int groups = h.nb / sk.nb;
      if (groups * sk.nb != h.nb) e.chk(CS_EINVAL);
      for (int g = 0; g < groups && e.ok(); ++g)
        e.chk(cs_copy_rows(e.p(sk.b), e.p(cat.b) + (int64_t)g * sk.b.rows * cat.b.c + h.b.c, sk.b.rows, sk.b.c,
                           sk.b.c, cat.b.c, e.st));
    }
    // the concatenation's GroupNorm takes its statistics from both halves' producers (unet.py: cs_segs): their partials
    // move to the concatenation buffer and are released with it
    cat.b.nseg = 0;
    if (h.b.nseg == 1 && sk.b.nseg == 1 && h.b.seg[0].valid() && sk.b.seg[0].valid()) {
      cat.b.seg[0] = h.b.seg[0];
      cat.b.seg[1] = sk.b.seg[0];
      cat.b.nseg = 2;
      h.b.seg[0] = Stat();
      sk.b.seg[0] = Stat();
      h.b.nseg = sk.b.nseg = 0;
    }
    e.release(h.b);
    if (layers[0].kind == RES && layers[0].ks > 0 && cat.b.rows >= u.split_min_rows) {
      h = e.run(layers, cat, semb, ctxvec, false, &sk);      // the skip tensor itself feeds the shared GEMMs
      e.release(sk.b);
    } else {
      e.release(sk.b);
      h = e.run(layers, cat, semb, ctxvec, false);
    }
    if (!e.ok()) return e.rc;
  }
  Buf hn = e.groupnorm(h.b, u.n_out, h.nb, 1e-5f, CS_ACT_SILU, 32, u.g_out);
  e.release(h.b);
  Buf eps = e.gemm(hn, u.g_out, h.nb, h.d, h.h, h.w);
  e.release(hn);
  if (e.ok() && !e.dry) e.chk(cs_ndhwc_to_nchw(e.p(eps), eps_ncdhw, h.nb, c.out_channels, S, eps.c, e.st));
  e.release(eps);
  e.release(semb);
  e.release(e.amax_arena);
  return e.rc;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------
extern "C" int cs_unet_create(const CsUnetConfig* cfg, cs_unet** out) {
  if (!cfg || !out) return CS_EINVAL;
  cs_unet* u = new (std::nothrow) cs_unet();
  if (!u) return CS_ENOMEM;
  u->cfg = *cfg;
  u->math = cfg->math;
  const int rc = build(*u);
  if (rc != CS_OK) {
    delete u;
    return rc;
  }
  *out = u;
  return CS_OK;
}

extern "C" void cs_unet_destroy(cs_unet* u) { delete u; }

extern "C" int cs_unet_param_count(const cs_unet* u) { return u ? (int)u->params.size() : 0; }

extern "C" int cs_unet_param_info(const cs_unet* u, int i, const char** name, int64_t shape5[5], int* ndim,
                                  int64_t* raw_offset_bytes) {
  return plan_param_info(u, i, name, shape5, ndim, raw_offset_bytes);
}

extern "C" int64_t cs_unet_raw_bytes(const cs_unet* u) { return u ? u->raw_bytes : 0; }
extern "C" int64_t cs_unet_arena_bytes(const cs_unet* u) { return u ? u->arena_bytes : 0; }
extern "C" int64_t cs_unet_context_floats(const cs_unet* u) { return u ? u->ctx_total : 0; }

extern "C" int cs_unet_pack(cs_unet* u, const void* raw_dev, void* arena_dev, cs_stream_t stream) {
  const int rc = pack_plan(u, raw_dev, arena_dev, stream);
  if (rc != CS_OK || !u || u->math != CS_MATH_F16X3) return rc;
  // The static-bound statistics of every AttentionBlock, then of every transformer block (unet.py::_pack: the same kernel
  // on the same tensors, the same values): cs_weight_rowstats leaves {max row 2-norm, max |.|} of one raw tensor per job
  // in two of the block's float slots behind the plan's |w| maxima (zeroed by pack_plan).  ONE read-back per block kind at
  // load time; a model has one kind
  hipStream_t st = (hipStream_t)stream;
  const char* raw = reinterpret_cast<const char*>(raw_dev);
  float* d_amax = reinterpret_cast<float*>(reinterpret_cast<char*>(arena_dev) + u->amax_off);
  auto src = [&](int param) { return reinterpret_cast<const float*>(raw + u->params[param].raw_off); };
  struct Job {
    const float* w;
    int rows, cols;
  };
  for (Kind kind : {ATTNBLOCK, ATTN}) {
    std::vector<Layer*> blocks;
    for_each_layer(*u, [&](Layer& l) {
      if (l.kind == kind && l.stat_slot >= 0) blocks.push_back(&l);
    });
    if (blocks.empty()) continue;
    const int njobs = kind == ATTN ? 17 : 2;      // two float slots each
    for (const Layer* lp : blocks) {
      const Layer& l = *lp;
      const int c = l.cin;
      std::vector<Job> jobs;
      if (kind == ATTNBLOCK) {      // the fused qkv weight [3c][c] and its bias
        jobs = {{src(l.ab_w), 3 * c, c}, {src(l.ab_b), 1, 3 * c}};
      } else {      // the block's Linears and LayerNorm parameters
        const Gemm& qkv = u->gemms[l.g[1]];
        const Gemm& to = u->gemms[l.g[2]];
        const Gemm& ff = u->gemms[l.g[5]];
        const Gemm& f2 = u->gemms[l.g[6]];
        const Gemm& pi = u->gemms[l.g[0]];
        const Norm& n1 = u->norms[l.n[1]];
        const Norm& n3 = u->norms[l.n[3]];
        if (qkv.w.size() != 3 || to.w.empty() || to.b.empty() || ff.w.empty() || ff.b.empty() || f2.w.empty() || f2.b.empty() ||
            pi.w.empty() || pi.b.empty())
          return CS_EINVAL;
        const float* wff = src(ff.w[0].param);
        const float* bff = src(ff.b[0].param);
        jobs = {
            {src(qkv.w[0].param), c, c}, {src(qkv.w[1].param), c, c}, {src(qkv.w[2].param), c, c},        // rq rk rv
            {src(to.w[0].param), c, c}, {src(to.b[0].param), 1, c},                                          // ro bo
            {wff, 4 * c, c}, {bff, 1, 4 * c}, {wff + (int64_t)4 * c * c, 4 * c, c}, {bff + 4 * c, 1, 4 * c},  // rx bx rg bg
            {src(f2.w[0].param), c, 4 * c}, {src(f2.b[0].param), 1, c},                                      // r2 b2
            {src(pi.w[0].param), c, c}, {src(pi.b[0].param), 1, c},                                          // rpi bpi
            {src(n1.gp), 1, c}, {src(n1.bp), 1, c}, {src(n3.gp), 1, c}, {src(n3.bp), 1, c}};                 // g1 be1 g3 be3
      }
      if ((int)jobs.size() != njobs) return CS_EINVAL;
      for (int j = 0; j < njobs; ++j) {
        const int r2 = cs_weight_rowstats(jobs[j].w, jobs[j].rows, jobs[j].cols, d_amax + l.stat_slot + 2 * j, stream);
        if (r2 != CS_OK) return r2;
      }
    }
    // (the blocks' slots are contiguous: they were reserved one after the other)
    std::vector<float> host((size_t)2 * njobs * blocks.size());
    if (hipMemcpyAsync(host.data(), d_amax + blocks[0]->stat_slot, host.size() * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
      return CS_EINVAL;
    for (size_t b = 0; b < blocks.size(); ++b) {
      const float* h = host.data() + 2 * njobs * b;
      if (kind == ATTNBLOCK) {
        blocks[b]->ab_l2max = h[0];      // the weight's row norm, the bias's abs max
        blocks[b]->ab_bmax = h[3];
        continue;
      }
      // which of {row norm, abs max} each field takes (unet.py::_pack)
      static const int which[17] = {0, 0, 0, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 1, 0, 1, 0};
      float v[17];
      for (int j = 0; j < 17; ++j) v[j] = h[2 * j + which[j]];
      CsTransformerStats& t = blocks[b]->ts;
      t.rq = v[0]; t.rk = v[1]; t.rv = v[2]; t.ro = v[3]; t.bo = v[4]; t.rx = v[5]; t.bx = v[6]; t.rg = v[7]; t.bg = v[8];
      t.r2 = v[9]; t.b2 = v[10]; t.rpi = v[11]; t.bpi = v[12]; t.g1 = v[13]; t.be1 = v[14]; t.g3 = v[15]; t.be3 = v[16];
      blocks[b]->has_ts = true;
    }
  }
  return CS_OK;
}

// the largest |entry| of every transformer block's cross-attention row vector of the CURRENT run, in block order (input
// blocks, middle, output blocks) -- host data the caller reads back once per run after cs_unet_context (it enters t1's
// static bound, cs_transformer_static_scales).  n must equal the number of transformer blocks; never called: 0 is assumed.
extern "C" int cs_unet_set_context_bounds(cs_unet* u, const float* ctx_max, int n) {
  if (!u || !ctx_max || n < 0) return CS_EINVAL;
  int nblk = 0;
  for_each_layer(*u, [&](const Layer& l) { nblk += l.kind == ATTN; });
  if (nblk != n) return CS_EINVAL;
  int i = 0;
  for_each_layer(*u, [&](Layer& l) {
    if (l.kind != ATTN) return;
    l.ctx_max = ctx_max[i] > 0.f ? ctx_max[i] : 0.f;
    ++i;
  });
  return CS_OK;
}

extern "C" int64_t cs_unet_workspace_bytes(const cs_unet* u, int nb_x, int cfg_pairs) {
  if (!u || nb_x <= 0) return CS_EINVAL;
  Exec e(*u, nullptr, nullptr, 0, true, nullptr);
  const int rc = forward(e, nullptr, nullptr, nullptr, nullptr, nb_x, cfg_pairs);
  if (rc != CS_OK) return rc;
  // the context pass needs one [nb_ctx][max c] temporary
  int maxc = 0;
  for (const Gemm& g : u->gemms) maxc = g.cout > maxc && g.cin == u->cfg.context_dim ? g.cout : maxc;
  const int64_t ctx_ws = align_up((int64_t)(cfg_pairs ? 2 : 1) * nb_x * maxc * 4) + 3 * ALIGN;      // (+ the bound slots)
  return e.peak > ctx_ws ? e.peak : ctx_ws;
}

extern "C" int cs_unet_context(const cs_unet* u, const void* arena, const float* ctx, int nb_ctx, float* ctxvec,
                               int32_t* status, void* workspace, int64_t workspace_bytes, cs_stream_t stream) {
  if (!u || !u->packed || !arena || !ctx || !ctxvec || !workspace || nb_ctx <= 0) return CS_EINVAL;
  if (!u->cfg.use_spatial_transformer) return CS_EINVAL;      // the concat family has no context
  Exec e(*u, arena, workspace, workspace_bytes, false, (hipStream_t)stream);
  e.status = status;
  const bool dyn = u->cfg.math == CS_MATH_F16X3 && !cs_debug()->no_dyn_scale && !cs_debug()->no_static_scales;
  Buf slots = e.alloc(64, 1);              // slot 0: max |ctx|; slot 1 + k: max |to_v(ctx)| of transformer block k
  int nslot = 0;
  if (dyn && e.ok() && hipMemsetAsync(e.p(slots), 0, 64 * 4, e.st) != hipSuccess) e.chk(CS_EINVAL);
  for_each_layer(*u, [&](const Layer& l) {
    if (l.kind != ATTN || !e.ok()) return;
    const Gemm& gv = u->gemms[l.g[3]];
    const Gemm& go = u->gemms[l.g[4]];
    Buf v2 = e.alloc(nb_ctx, gv.cout);
    if (!e.ok()) return;
    for (int pass = 0; pass < 2 && e.ok(); ++pass) {      // to_v over the context rows (read in place), then to_out
      const Gemm& g = pass == 0 ? gv : go;
      View a;
      a.x = pass == 0 ? ctx : e.p(v2);
      a.lda = g.cin_pad;
      GemmOpts opt;
      // unet.py::_context_vectors: the context and to_v's output are raw operands -- their scale follows a device-side
      // magnitude bound (max |.| into a workspace slot, CsConvGemm.a_bound) instead of the constant 16
      if (dyn) {
        const int64_t nel = (int64_t)nb_ctx * (pass == 0 ? u->cfg.context_dim : gv.cout);
        const int slot = pass == 0 ? 0 : 1 + nslot;
        if (pass == 1 || nslot == 0) {
          CS_LAUNCH(absmax_kernel, dim3(cs_grid_for(nel, 256, 256)), dim3(256), 0, e.st, a.x, nel, e.p(slots) + slot);
          if (hipGetLastError() != hipSuccess) e.chk(CS_EINVAL);
        }
        opt.bound(slots.off + 4 * slot);
        if (pass == 1) ++nslot;
      }
      CsConvGemm q;
      e.describe(q, g, a, pass == 0 ? e.p(v2) : ctxvec + l.ctx_off, pass == 0 ? g.cout : u->ctx_total, nb_ctx, 1, 1, 1, opt);
      e.chk(cs_conv_gemm(&q, e.st));
    }
    e.release(v2);
  });
  return e.rc;
}

extern "C" int cs_unet_step(const cs_unet* u, const void* arena, const float* x_ncdhw, const int64_t* t,
                            const float* ctxvec, float* eps_ncdhw, int nb_x, int cfg_pairs, int32_t* status,
                            void* workspace, int64_t workspace_bytes, cs_stream_t stream) {
  if (!u || !u->packed || !arena || !x_ncdhw || !t || !eps_ncdhw || !workspace || nb_x <= 0) return CS_EINVAL;
  // crossattn family: ctxvec (cs_unet_context) is required.  concat family (no transformer blocks): there is no
  // context, x carries the condition volume as its last channel(s) (network.py:25-27) and the guidance halves
  // share nothing, so cfg_pairs must be 0 and the caller passes the duplicated batch.
  if (u->cfg.use_spatial_transformer ? !ctxvec : (ctxvec != nullptr || cfg_pairs != 0)) return CS_EINVAL;
  if (((uintptr_t)workspace & 15) || ((uintptr_t)arena & 15) || ((uintptr_t)ctxvec & 15)) return CS_EINVAL;
  Exec e(*u, arena, workspace, workspace_bytes, false, (hipStream_t)stream);
  e.status = status;
  return forward(e, x_ncdhw, t, ctxvec, eps_ncdhw, nb_x, cfg_pairs);
}
