// Shared machinery of the native whole-forward drivers (cs_unet.hip, cs_vqvae.hip): the host-side plan (reference
// parameter table, packed-GEMM recipes, arena layout), the raw -> arena packing pass, and an executor that
// sequences the library's own C entries over a caller-owned workspace (first-fit allocator, dry-run sizing).
// Internal header: everything lives in an anonymous namespace of the including translation unit.
#pragma once
#include "cs_common.h"

#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

namespace {

constexpr int64_t ALIGN = 256;
inline int64_t align_up(int64_t v) { return (v + ALIGN - 1) / ALIGN * ALIGN; }

struct Param {
  std::string name;
  int64_t shape[5];
  int ndim;
  int64_t numel;
  int64_t raw_off;   // bytes into the caller's raw parameter buffer
};

struct Piece {       // rows [row0, row0 + rows) of parameter `param` seen as a [rows_total][cols] matrix;
                     // param < 0: `rows` all-zero rows (channel padding)
  int param;
  int row0;
  int rows;
};

struct Gemm {        // one packed GEMM weight (possibly several reference tensors concatenated along cout)
  std::vector<Piece> w, b;
  int cout = 0, cin = 0, cin_pad = 0, k = 1, taps = 1, ldw = 0;
  // input-channel range [c0, c0 + cin) of source tensors that have src_cin input channels (0 = all of them): the two
  // halves of a channel-split conv (cs_unet.hip: res_block_split); the operand scale is the WHOLE tensor's either way
  int c0 = 0, src_cin = 0;
  // > 0: a thin-output 3x3x3 conv (tap_cout <= 4 output channels) run as "taps as columns": the packed weight is the
  // POINTWISE one with cout = 27 * tap_cout (+ pad) columns (cs_pack_weight_f16x3_tapcol; k = 1 here), and cs_tapsum27
  // adds the 27 shifted columns of every output channel and the bias (ops.py::pack_weight_tapcol)
  int tap_cout = 0;
  int64_t w_off = 0, wlo_off = 0, b_off = -1;
  float acc_scale = 1.f;
  // Upsample's conv folded onto the source grid (cs_conv_gemm_up2): bit 2 / 1 / 0 = D / H / W doubled.  The packed
  // weights are then one image (pair) per output parity class, built from the folded fp32 taps kept at fold_off.
  int up_mask = 0, ncls = 0, fkd = 3, fkh = 3, fkw = 3, amax_slot = -1;
  int64_t fold_off = 0, cls_w_off[8] = {0}, cls_wlo_off[8] = {0};
  float cls_acc_scale[8] = {0};
  // the Winograd-W pack of a 3x3x3 conv beside the direct one (CsConvGemm.a_format = 3, ops.py::pack_weight_wino): four
  // position images, one power-of-two scale; -1 = the geometry can never take that route
  int64_t wino_off = -1, wino_lo_off = -1;
  float wino_acc = 1.f;
  // ... and its F(4,3) sibling (six images): CsConvGemm.a_format = 4
  int64_t wino4_off = -1, wino4_lo_off = -1;
  float wino4_acc = 1.f;

  // the pack a launch reads: hi / lo image offsets and 1 / (weight scale * 16).  variant 0 = direct, 2 = F(2,3), 4 = F(4,3)
  struct Pack {
    int64_t w, lo;
    float acc;
  };
  Pack pack(int variant) const {
    if (variant == 4) return {wino4_off, wino4_lo_off, wino4_acc};
    if (variant == 2) return {wino_off, wino_lo_off, wino_acc};
    return {w_off, wlo_off, acc_scale};
  }
  // F16X3 images: 8-channel K groups per tap (cin rounded up to 16), bytes of one hi or lo image of ntaps taps
  int kg() const { return (cin + 15) / 16 * 2; }
  int64_t img_bytes(int64_t ntaps) const { return ntaps * kg() * cout * 16; }
  // fp32 layout [tap][cin_pad][ldw]
  int64_t f32_bytes(int64_t ntaps) const { return ntaps * cin_pad * ldw * 4; }
};

// power-of-two F16X3 weight scale of a tensor whose largest |entry| is m (2^14 / 2^ex: the scaled maximum lands in
// [2^13, 2^14)) and the matching accumulator scale 1 / (scale * 16)
struct WeightScale {
  float scale, acc;
};
inline WeightScale weight_scale(double m) {
  int ex = 0;
  if (m > 0.0 && std::isfinite(m)) (void)std::frexp(m, &ex);
  const float scale = (float)std::ldexp(1.0, 14 - ex);
  return {scale, 1.0f / (scale * 16.0f)};
}

struct Norm {
  int gp, bp, c;
  int64_t g_off, b_off;
  float gmax = 1.f, bmax = 0.f;   // max |gamma|, max |beta| (filled by pack_plan in F16X3 mode): norm_a_scale
};

// F16X3 operand scale of a GEMM fed by a normalisation over n elements per statistic: cs_norm_a_scale (csrc/cs_plan.hip),
// the one rule both hosts call
inline float norm_a_scale(float gmax, float bmax, int64_t n) { return cs_norm_a_scale(gmax, bmax, n); }

struct RawCopy {     // a parameter copied verbatim into the arena (e.g. the VQ codebook)
  int param;
  int64_t arena_off;
};

struct FreeBlock {
  int64_t off, size;
};

struct Plan {
  int math = CS_MATH_FP32;
  std::vector<Param> params;
  std::vector<Gemm> gemms;
  std::vector<Norm> norms;
  std::vector<RawCopy> copies;
  int64_t raw_bytes = 0, arena_bytes = 0, amax_off = 0;
  int amax_slots = 0;      // per-parameter |w| maxima, then one per parity class of every folded upsample conv
  int extra_slots = 0;     // ... then this many more floats reserved by the model (cs_unet: 34 per transformer block)
  int extra_slot0 = 0;     // index of the first of them (set by layout_arena)
  bool packed = false;
};

// ---------------------------------------------------------------------------------------------------------
// plan construction
// ---------------------------------------------------------------------------------------------------------
int add_param(Plan& u, const std::string& name, std::initializer_list<int64_t> shape) {
  Param p;
  p.name = name;
  p.ndim = (int)shape.size();
  p.numel = 1;
  int i = 0;
  for (int64_t s : shape) {
    p.shape[i++] = s;
    p.numel *= s;
  }
  for (; i < 5; ++i) p.shape[i] = 1;
  p.raw_off = u.raw_bytes;
  u.raw_bytes += align_up(p.numel * 4);
  u.params.push_back(p);
  return (int)u.params.size() - 1;
}

int add_norm(Plan& u, const std::string& p, int c) {
  Norm n;
  n.gp = add_param(u, p + ".weight", {c});
  n.bp = add_param(u, p + ".bias", {c});
  n.c = c;
  n.g_off = n.b_off = 0;
  u.norms.push_back(n);
  return (int)u.norms.size() - 1;
}

// registers <p>.weight (+ .bias); returns the parameter indices
void add_wb(Plan& u, const std::string& p, int o, int i, int k, bool bias, int& wp, int& bp) {
  if (k > 1)
    wp = add_param(u, p + ".weight", {o, i, k, k, k});
  else if (k == 1)
    wp = add_param(u, p + ".weight", {o, i, 1, 1, 1});
  else
    wp = add_param(u, p + ".weight", {o, i});   // Linear
  bp = bias ? add_param(u, p + ".bias", {o}) : -1;
}

int add_gemm(Plan& u, std::vector<Piece> w, std::vector<Piece> b, int cout, int cin, int k, int cin_pad = 0) {
  Gemm g;
  g.w = std::move(w);
  g.b = std::move(b);
  g.cout = cout;
  g.cin = cin;
  g.k = k < 1 ? 1 : k;
  g.taps = g.k * g.k * g.k;
  g.cin_pad = cin_pad ? cin_pad : (cin + 3) / 4 * 4;
  u.gemms.push_back(g);
  return (int)u.gemms.size() - 1;
}

// conv (k = 3 or 1) or Linear (k = 0) as a single-tensor GEMM
// tapcol: the caller names this layer as a thin-output conv to run as "taps as columns" -- exactly the layers the Python
// hosts name (unet.py: `out.2`, vqvae.py: `decoder.conv_out`); whether it is then taken is ops.py::tapcol_ok's rule.  (r3
// applied the rule to ANY thin 3x3x3 conv here: a config with another one would have made the two hosts sum in a
// different order -- ADVICE r3.)
int add_layer_gemm(Plan& u, const std::string& p, int o, int i, int k, bool bias = true, int cin_pad = 0,
                   int up_mask = 0, bool tapcol = false) {
  int wp, bp;
  add_wb(u, p, o, i, k, bias, wp, bp);
  std::vector<Piece> b;
  if (bp >= 0) b.push_back({bp, 0, o});
  if (tapcol) {
    // cs_tapcol_ok: the one rule (csrc/cs_plan.hip) both hosts ask
    if (!up_mask && cin_pad == 0 && cs_tapcol_ok(o, i, k, u.math)) {
      const int gi = add_gemm(u, {{wp, 0, o}}, b, (27 * o + 3) / 4 * 4, i, 1);
      u.gemms[gi].tap_cout = o;
      return gi;
    }
  }
  const int gi = add_gemm(u, {{wp, 0, o}}, b, o, i, k, cin_pad);
  if (up_mask && k == 3) {      // the conv of an Upsample: folded per output parity class (cs_fold_upsample_weight)
    Gemm& g = u.gemms[gi];
    int32_t n, a, bb, c;
    if (cs_conv_up2_info((up_mask >> 2) & 1, (up_mask >> 1) & 1, up_mask & 1, &n, &a, &bb, &c) == CS_OK) {
      g.up_mask = up_mask;
      g.ncls = n;
      g.fkd = a; g.fkh = bb; g.fkw = c;
    }
  }
  return gi;
}

// input channels [c0, c1) of an already registered conv / linear weight (wp; bias bp or -1) as a GEMM of its own
int add_gemm_cin_range(Plan& u, int wp, int bp, int o, int i_total, int k, int c0, int c1) {
  std::vector<Piece> b;
  if (bp >= 0) b.push_back({bp, 0, o});
  const int gi = add_gemm(u, {{wp, 0, o}}, b, o, c1 - c0, k);
  u.gemms[gi].c0 = c0;
  u.gemms[gi].src_cin = i_total;
  return gi;
}

int add_copy(Plan& u, int param) {
  u.copies.push_back({param, 0});
  return (int)u.copies.size() - 1;
}

void layout_arena(Plan& u) {
  const bool f16 = u.math == CS_MATH_F16X3;
  int64_t off = 0;
  int slots = (int)u.params.size();
  for (Gemm& g : u.gemms) {
    if (g.up_mask) {
      const int ftaps = g.fkd * g.fkh * g.fkw;
      g.ldw = f16 ? g.cout : (g.cout + 3) / 4 * 4;
      g.fold_off = off;
      off += align_up((int64_t)g.ncls * g.cout * g.cin * ftaps * 4);
      for (int c = 0; c < g.ncls; ++c) {
        g.cls_w_off[c] = off;
        off += align_up(f16 ? g.img_bytes(ftaps) : g.f32_bytes(ftaps));
        if (f16) {
          g.cls_wlo_off[c] = off;
          off += align_up(g.img_bytes(ftaps));
        }
      }
      g.amax_slot = slots;
      slots += g.ncls;
      if (!g.b.empty()) {
        g.b_off = off;
        off += align_up((int64_t)g.cout * 4);
      }
      continue;
    }
    if (f16) {
      g.ldw = g.cout;
      g.w_off = off;
      off += align_up(g.img_bytes(g.taps));
      g.wlo_off = off;
      off += align_up(g.img_bytes(g.taps));
      // the Winograd-W packs beside the direct one (four resp. six position images of nine taps) -- also for the
      // input-channel halves of a channel-split conv, scaled by the whole tensor's maximum like their direct packs:
      // ops.py::pack_weight_wino
      if (g.k == 3 && !g.tap_cout && g.w.size() == 1 && g.w[0].param >= 0 && g.w[0].row0 == 0 && g.w[0].rows == g.cout &&
          (g.cout % 224 == 0 || g.cout % 128 == 0 || g.cout == 64) && g.cin % 8 == 0 && g.cin >= 16 && g.cin_pad == g.cin) {
        g.wino_off = off;
        off += align_up(g.img_bytes(4 * 9));
        g.wino_lo_off = off;
        off += align_up(g.img_bytes(4 * 9));
        g.wino4_off = off;
        off += align_up(g.img_bytes(6 * 9));
        g.wino4_lo_off = off;
        off += align_up(g.img_bytes(6 * 9));
      }
    } else {
      g.ldw = (g.cout + 3) / 4 * 4;
      g.w_off = off;
      off += align_up(g.f32_bytes(g.taps));
    }
    if (!g.b.empty()) {
      g.b_off = off;
      off += align_up((int64_t)g.cout * 4);
    }
  }
  for (Norm& n : u.norms) {
    n.g_off = off;
    off += align_up((int64_t)n.c * 4);
    n.b_off = off;
    off += align_up((int64_t)n.c * 4);
  }
  for (RawCopy& rc : u.copies) {
    rc.arena_off = off;
    off += align_up(u.params[rc.param].numel * 4);
  }
  u.extra_slot0 = slots;
  slots += u.extra_slots;
  u.amax_off = off;
  u.amax_slots = slots;
  off += align_up((int64_t)slots * 4);
  u.arena_bytes = off;
}

int plan_param_info(const Plan* u, int i, const char** name, int64_t shape5[5], int* ndim, int64_t* raw_offset_bytes) {
  if (!u || i < 0 || i >= (int)u->params.size()) return CS_EINVAL;
  const Param& p = u->params[i];
  if (name) *name = p.name.c_str();
  if (shape5) memcpy(shape5, p.shape, sizeof(p.shape));
  if (ndim) *ndim = p.ndim;
  if (raw_offset_bytes) *raw_offset_bytes = p.raw_off;
  return CS_OK;
}

// ---------------------------------------------------------------------------------------------------------
// weight packing kernels (piece-wise versions of cs_pack_weight_f16x3 / cs_relayout_weight: a piece is a row
// range of a reference tensor landing at a column offset of a possibly fused GEMM weight)
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void absmax_kernel(const float* __restrict__ w, int64_t n, float* __restrict__ out) {
  __shared__ float red[4];
  float m = 0.f;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    m = fmaxf(m, fabsf(w[i]));
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    // non-negative floats order like their bit patterns
    atomicMax(reinterpret_cast<unsigned int*>(out), __float_as_uint(m));
  }
}

__global__ __launch_bounds__(256) void pack_part_f16x3_kernel(const float* __restrict__ w, _Float16* __restrict__ wh,
                                                              _Float16* __restrict__ wl, int rows, int n_off,
                                                              int cout_total, int cin, int taps, int kg_per_tap,
                                                              float scale, int src_cin = 0, int c0 = 0) {
  if (src_cin == 0) src_cin = cin;
  const int64_t total = (int64_t)taps * kg_per_tap * rows * 8;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int j = (int)(i & 7);
    int64_t t = i >> 3;
    const int n = (int)(t % rows);
    t /= rows;
    const int kg = (int)(t % kg_per_tap);
    const int tap = (int)(t / kg_per_tap);
    const int c = kg * 8 + j;
    float v = 0.f;
    if (c < cin) v = w[((int64_t)n * src_cin + c0 + c) * taps + tap] * scale;
    const _Float16 h = (_Float16)v;
    const int64_t o = (((int64_t)tap * kg_per_tap + kg) * cout_total + n_off + n) * 8 + j;
    wh[o] = h;
    wl[o] = (_Float16)(v - (float)h);
  }
}

// the Winograd-W pack of a 3x3x3 conv (or of an input-channel range [c0, c0 + cin) of one): cs_pack_weight_f16x3_wino's
// arithmetic -- u_q over the kw taps formed and split in fp64 -- on a (cout, src_cin, 27) source tensor
__global__ __launch_bounds__(256) void pack_part_f16x3_wino_kernel(const float* __restrict__ w, _Float16* __restrict__ wh,
                                                                   _Float16* __restrict__ wl, int cout, int cin,
                                                                   int kg_per_tap, float scale, int src_cin, int c0,
                                                                   int variant) {
  if (src_cin == 0) src_cin = cin;
  const int64_t per = 9LL * kg_per_tap * cout * 8;
  const int np = variant + 2;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < np * per; i += (int64_t)gridDim.x * blockDim.x) {
    const int q = (int)(i / per);
    int64_t t = i - q * per;
    const int j = (int)(t & 7);
    t >>= 3;
    const int n = (int)(t % cout);
    t /= cout;
    const int kg = (int)(t % kg_per_tap);
    const int tap = (int)(t / kg_per_tap);
    const int c = kg * 8 + j;
    double u = 0.0;
    if (c < cin) {
      const float* g = w + ((int64_t)n * src_cin + c0 + c) * 27 + tap * 3;
      const double g0 = g[0], g1 = g[1], g2 = g[2];
      if (variant == 4)
        u = q == 0 ? g0 / 4.0 : q == 1 ? -(g0 + g1 + g2) / 6.0 : q == 2 ? (-g0 + g1 - g2) / 6.0
            : q == 3 ? g0 / 24.0 + g1 / 12.0 + g2 / 6.0 : q == 4 ? g0 / 24.0 - g1 / 12.0 + g2 / 6.0 : g2;
      else
        u = q == 0 ? g0 : q == 1 ? 0.5 * (g0 + g1 + g2) : q == 2 ? 0.5 * (g0 - g1 + g2) : g2;
    }
    const double v = u * (double)scale;
    const _Float16 h = (_Float16)v;
    wh[i] = h;
    wl[i] = (_Float16)(v - (double)h);
  }
}

__global__ __launch_bounds__(256) void pack_part_f32_kernel(const float* __restrict__ w, float* __restrict__ o,
                                                            int rows, int n_off, int cin, int taps, int cin_pad,
                                                            int ldw, int src_cin = 0, int c0 = 0) {
  if (src_cin == 0) src_cin = cin;
  // w: rows of a (cout, cin, taps) torch tensor; o: [tap][cin_pad][ldw], columns n_off .. n_off + rows
  const int64_t total = (int64_t)taps * cin_pad * rows;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int n = (int)(i % rows);
    const int64_t t = i / rows;
    const int c = (int)(t % cin_pad);
    const int tap = (int)(t / cin_pad);
    float v = 0.f;
    if (c < cin) v = w[((int64_t)n * src_cin + c0 + c) * taps + tap];
    o[((int64_t)tap * cin_pad + c) * ldw + n_off + n] = v;
  }
}

// raw parameters -> arena: GEMM weights in the layout of the plan's math mode (pieces gathered into fused weights),
// biases, norm affine parameters, verbatim copies.  One stream sync in F16X3 mode (per-tensor |w| maxima).
int pack_plan(Plan* u, const void* raw_dev, void* arena_dev, cs_stream_t stream) {
  if (!u || !raw_dev || !arena_dev) return CS_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const char* raw = (const char*)raw_dev;
  char* arena = (char*)arena_dev;
  const bool f16 = u->math == CS_MATH_F16X3;
  auto src = [&](int param) { return reinterpret_cast<const float*>(raw + u->params[param].raw_off); };
  std::vector<float> amax((size_t)u->amax_slots, 0.f);
  // Upsample convs: fold the 27 taps into the per-parity-class taps first (their maxima are taken over the folded values)
  for (const Gemm& g : u->gemms) {
    if (!g.up_mask) continue;
    if (g.w.size() != 1 || g.w[0].param < 0 || g.w[0].row0 != 0 || g.w[0].rows != g.cout) return CS_EINVAL;
    const int rc = cs_fold_upsample_weight(src(g.w[0].param), reinterpret_cast<float*>(arena + g.fold_off), g.cout, g.cin,
                                           (g.up_mask >> 2) & 1, (g.up_mask >> 1) & 1, g.up_mask & 1, stream);
    if (rc != CS_OK) return rc;
  }
  if (f16) {
    // per-tensor |w| maxima for the power-of-two operand scales: one device pass, ONE host sync (load time)
    float* d_amax = reinterpret_cast<float*>(arena + u->amax_off);
    if (hipMemsetAsync(d_amax, 0, (size_t)u->amax_slots * 4, st) != hipSuccess) return CS_EINVAL;
    for (const Gemm& g : u->gemms) {
        if (g.up_mask) {
        const int64_t n = (int64_t)g.cout * g.cin * g.fkd * g.fkh * g.fkw;
        for (int c = 0; c < g.ncls; ++c) {
          CS_LAUNCH(absmax_kernel, dim3(cs_grid_for(n, 256, 256)), dim3(256), 0, st,
                    reinterpret_cast<const float*>(arena + g.fold_off) + c * n, n, d_amax + g.amax_slot + c);
          CS_CHECK_LAUNCH();
        }
        continue;
      }
      for (const Piece& pc : g.w) {
        if (pc.param < 0) continue;
        const Param& p = u->params[pc.param];
        CS_LAUNCH(absmax_kernel, dim3(cs_grid_for(p.numel, 256, 256)), dim3(256), 0, st, src(pc.param), p.numel,
                  d_amax + pc.param);
        CS_CHECK_LAUNCH();
      }
    }
    for (const Norm& n : u->norms) {
      CS_LAUNCH(absmax_kernel, dim3(1), dim3(256), 0, st, src(n.gp), (int64_t)n.c, d_amax + n.gp);
      CS_CHECK_LAUNCH();
      CS_LAUNCH(absmax_kernel, dim3(1), dim3(256), 0, st, src(n.bp), (int64_t)n.c, d_amax + n.bp);
      CS_CHECK_LAUNCH();
    }
    if (hipMemcpyAsync(amax.data(), d_amax, amax.size() * 4, hipMemcpyDeviceToHost, st) != hipSuccess)
      return CS_EINVAL;
    if (hipStreamSynchronize(st) != hipSuccess) return CS_EINVAL;
    for (Norm& n : u->norms) {
      n.gmax = amax[(size_t)n.gp];
      n.bmax = amax[(size_t)n.bp];
    }
  }
  auto copy_bias = [&](const Gemm& g) -> int {
    int n_off = 0;
    for (const Piece& pc : g.b) {
      if (pc.param < 0) {
        if (hipMemsetAsync(arena + g.b_off + (int64_t)n_off * 4, 0, (size_t)pc.rows * 4, st) != hipSuccess)
          return CS_EINVAL;
      } else if (hipMemcpyAsync(arena + g.b_off + (int64_t)n_off * 4, src(pc.param) + pc.row0, (size_t)pc.rows * 4,
                                hipMemcpyDeviceToDevice, st) != hipSuccess)
        return CS_EINVAL;
      n_off += pc.rows;
    }
    return CS_OK;
  };
  for (Gemm& g : u->gemms) {
    const int kg = g.kg();
    if (g.up_mask) {      // one packed image (pair) per parity class, each with its own power-of-two scale
      const int ftaps = g.fkd * g.fkh * g.fkw;
      const int64_t n = (int64_t)g.cout * g.cin * ftaps;
      for (int c = 0; c < g.ncls; ++c) {
        const float* w = reinterpret_cast<const float*>(arena + g.fold_off) + c * n;
        if (f16) {
          const WeightScale s = weight_scale(amax[(size_t)g.amax_slot + c]);
          g.cls_acc_scale[c] = s.acc;
          const int64_t total = (int64_t)ftaps * kg * g.cout * 8;
          CS_LAUNCH(pack_part_f16x3_kernel, dim3(cs_grid_for(total, 256, 256 * 32)), dim3(256), 0, st, w,
                    (_Float16*)(arena + g.cls_w_off[c]), (_Float16*)(arena + g.cls_wlo_off[c]), g.cout, 0, g.cout,
                    g.cin, ftaps, kg, s.scale, 0, 0);
        } else {
          if (hipMemsetAsync(arena + g.cls_w_off[c], 0, (size_t)g.f32_bytes(ftaps), st) != hipSuccess) return CS_EINVAL;
          const int64_t total = (int64_t)ftaps * g.cin_pad * g.cout;
          CS_LAUNCH(pack_part_f32_kernel, dim3(cs_grid_for(total, 256)), dim3(256), 0, st, w,
                    (float*)(arena + g.cls_w_off[c]), g.cout, 0, g.cin, ftaps, g.cin_pad, g.ldw, 0, 0);
        }
        CS_CHECK_LAUNCH();
      }
      const int rc = copy_bias(g);
      if (rc != CS_OK) return rc;
      continue;
    }
    if (g.tap_cout) {     // taps as columns: the whole (tap_cout, cin, 3, 3, 3) tensor -> one pointwise image pair
      if (!f16 || g.w.size() != 1 || g.w[0].param < 0 || g.w[0].row0 != 0 || g.w[0].rows != g.tap_cout) return CS_EINVAL;
      const WeightScale s = weight_scale(amax[(size_t)g.w[0].param]);
      g.acc_scale = s.acc;
      int rc = cs_pack_weight_f16x3_tapcol(src(g.w[0].param), arena + g.w_off, arena + g.wlo_off, g.tap_cout, g.cin,
                                           g.cout, s.scale, stream);
      if (rc == CS_OK) rc = copy_bias(g);
      if (rc != CS_OK) return rc;
      continue;
    }
    const int cols = (g.src_cin ? g.src_cin : g.cin) * g.taps;    // row length of the reference tensor seen as [cout][cin * taps]
    float scale = 1.f;
    if (f16) {
      // scale by the whole tensor's maximum even when only a row range is used (GEGLU pieces): what
      // ops._pack_weight_f16x3 sees is the permuted full tensor, whose maximum is the same
      float m = 0.f;
      bool zero_rows = false;
      for (const Piece& pc : g.w) {
        if (pc.param >= 0) m = fmaxf(m, amax[pc.param]);
        zero_rows |= pc.param < 0;
      }
      const WeightScale s = weight_scale(m);
      scale = s.scale;
      g.acc_scale = s.acc;
      if (zero_rows && (hipMemsetAsync(arena + g.w_off, 0, (size_t)g.img_bytes(g.taps), st) != hipSuccess ||
                        hipMemsetAsync(arena + g.wlo_off, 0, (size_t)g.img_bytes(g.taps), st) != hipSuccess))
        return CS_EINVAL;
    } else {
      if (hipMemsetAsync(arena + g.w_off, 0, (size_t)g.f32_bytes(g.taps), st) != hipSuccess) return CS_EINVAL;
    }
    int n_off = 0;
    for (const Piece& pc : g.w) {
      if (pc.param < 0) {     // zero rows: the images were cleared above
        n_off += pc.rows;
        continue;
      }
      const float* w = src(pc.param) + (int64_t)pc.row0 * cols;
      if (f16) {
        const int64_t total = (int64_t)g.taps * kg * pc.rows * 8;
        CS_LAUNCH(pack_part_f16x3_kernel, dim3(cs_grid_for(total, 256, 256 * 32)), dim3(256), 0, st, w,
                  (_Float16*)(arena + g.w_off), (_Float16*)(arena + g.wlo_off), pc.rows, n_off, g.cout, g.cin,
                  g.taps, kg, scale, g.src_cin, g.c0);
      } else {
        const int64_t total = (int64_t)g.taps * g.cin_pad * pc.rows;
        CS_LAUNCH(pack_part_f32_kernel, dim3(cs_grid_for(total, 256)), dim3(256), 0, st, w,
                  (float*)(arena + g.w_off), pc.rows, n_off, g.cin, g.taps, g.cin_pad, g.ldw, g.src_cin, g.c0);
      }
      CS_CHECK_LAUNCH();
      n_off += pc.rows;
    }
    if (n_off != g.cout) return CS_EINVAL;
    // the Winograd-W packs (max |u_q| <= 1.5 max |w| for F(2,3), <= max |w| for F(4,3): ops.py::pack_weight_wino)
    for (int variant = 2; f16 && variant <= 4 && g.pack(variant).w >= 0; variant += 2) {
      const WeightScale s = weight_scale((variant == 2 ? 1.5 : 1.0) * (double)amax[(size_t)g.w[0].param]);
      (variant == 2 ? g.wino_acc : g.wino4_acc) = s.acc;
      const Gemm::Pack pk = g.pack(variant);
      CS_LAUNCH(pack_part_f16x3_wino_kernel, dim3(cs_grid_for((variant + 2LL) * 9 * kg * g.cout * 8, 256, 256 * 32)), dim3(256),
                0, st, src(g.w[0].param), (_Float16*)(arena + pk.w), (_Float16*)(arena + pk.lo), g.cout, g.cin, kg, s.scale,
                g.src_cin, g.c0, variant);
      CS_CHECK_LAUNCH();
    }
    const int rc = copy_bias(g);
    if (rc != CS_OK) return rc;
  }
  for (const Norm& n : u->norms) {
    if (hipMemcpyAsync(arena + n.g_off, src(n.gp), (size_t)n.c * 4, hipMemcpyDeviceToDevice, st) != hipSuccess ||
        hipMemcpyAsync(arena + n.b_off, src(n.bp), (size_t)n.c * 4, hipMemcpyDeviceToDevice, st) != hipSuccess)
      return CS_EINVAL;
  }
  for (const RawCopy& rc : u->copies) {
    if (hipMemcpyAsync(arena + rc.arena_off, src(rc.param), (size_t)u->params[rc.param].numel * 4,
                       hipMemcpyDeviceToDevice, st) != hipSuccess)
      return CS_EINVAL;
  }
  u->packed = true;
  return CS_OK;
}

// ---------------------------------------------------------------------------------------------------------
// execution
// ---------------------------------------------------------------------------------------------------------
// per-(row tile, column) GroupNorm partial sums a producing GEMM left in the workspace (CsConvGemm.gn_part; ops.ColStats)
struct Stat {
  int64_t off = -1, bytes = 0;
  int nch = 0, nb = 0, tps = 0, ncls = 1;      // columns, samples the producer ran, tiles per sample (per class), classes
  bool valid() const { return off >= 0; }
};

struct Buf {
  int64_t off = -1, bytes = 0;
  int64_t rows = 0;
  int c = 0;
  // the producers' partials covering this tensor's channels in order -- one segment (a GEMM output) or two (a channel
  // concatenation [h | skip]: seg[1] starts at channel seg[0].nch); released with the buffer
  Stat seg[2];
  int nseg = 0;
  bool half = false;   // fp16 hi image [rows][c] followed by the lo image (the F16X3 GEMMs' pre-split A operand);
                       // same footprint as fp32 [rows][c]
  bool pair = false;   // the INTERLEAVED operand pair (CsConvGemm.a_format = 2): bytes / row stride of fp32 [rows][c],
                       // written by cs_layernorm_pair16
  int wino = 0;        // the Winograd-W operand (CsConvGemm.a_format = 3 / 4), the variant (2 = F(2,3), 4 = F(4,3)): fp16 hi
                       // images [variant + 2][voxels / variant][c] followed by the lo images -- `rows` = (variant + 2) /
                       // variant x the volume's voxels
  float a_scale = 16.f;   // F16X3 operand scale a GEMM reading this buffer uses: the default for activations of unknown
                          // range, the producer's bound for normalisation outputs (norm_a_scale)
};

struct Act {   // an activation volume, channels-last
  Buf b;
  int nb = 0, d = 0, h = 0, w = 0;
};

// a GEMM's A operand as the kernel reads it: x (+ x_lo: the lo image of a pre-split pair / of a Winograd-W operand), row
// stride lda, the F16X3 operand scale and CsConvGemm.a_format (0 fp32, 1 pre-split, 2 interleaved pair, 3 / 4 Winograd-W
// F(2,3) / F(4,3)).  The sizing pass carries no pointers but the same format: the plan and tile rules look at it
struct View {
  const float* x = nullptr;
  const void* x_lo = nullptr;
  int lda = 0;
  float a_scale = 16.f;
  int format = 0;
  int wino() const { return format == 4 ? 4 : format == 3 ? 2 : 0; }      // the Winograd-W variant (Gemm::pack), 0 = none
};

// what a GEMM launch sets beyond operand, weight and geometry, by name: `gemm(x, gi, nb, d, h, w,
// GemmOpts().stats().residual(skip, skip.c))`.  The defaults are a plain stride-1 launch
struct GemmOpts {
  int s_hw = 1, s_d = 1;          // stride along (H, W) and along D
  int up_hw = 0, up_d = 0;        // log2 nearest-upsample factor applied to the operand first
  int act = CS_ACT_NONE;
  const float* rowvec = nullptr;  // epilogue row vector: entry [row / rv_rows][ldrv] (a launch argument: NULL in the sizing
  int ldrv = 0, rv_rows = 1;      // pass, where ldrv > 0 says that the real pass will bring one)
  int64_t res_off = -1;           // epilogue residual [M][ldr]: the workspace offset of its buffer
  int ldr = 0;
  int tile = 0;                   // CsConvGemm.tile, 0 = auto
  bool want_stats = false;        // the result feeds a GroupNorm: leave its partial sums where the launch can
  float out_pair = 0.f;           // > 0: the only reader is the next F16X3 GEMM -- write the operand pair at this scale
  int64_t a_bound_off = -1;       // >= 0: the operand is RAW, its magnitude bound sits in this workspace slot

  GemmOpts& stride(int hw, int d) { s_hw = hw; s_d = d; return *this; }
  GemmOpts& upsample(int hw, int d) { up_hw = hw; up_d = d; return *this; }
  GemmOpts& activation(int a) { act = a; return *this; }
  GemmOpts& row_vector(const float* rv, int ld, int rows) { rowvec = rv; ldrv = ld; rv_rows = rows; return *this; }
  GemmOpts& residual(const Buf& b, int ld) { res_off = b.off; ldr = ld; return *this; }
  GemmOpts& stats() { want_stats = true; return *this; }
  GemmOpts& pair(float scale) { out_pair = scale; return *this; }
  GemmOpts& bound(int64_t slot_off) { a_bound_off = slot_off; return *this; }
};

struct ExecBase {
  const Plan& pl;
  const char* arena;
  char* ws;
  int64_t ws_bytes;
  bool dry;
  hipStream_t st;
  int rc = CS_OK;
  int64_t peak = 0;
  int32_t* status = nullptr;     // caller's sticky CS_STATUS_* word (device) handed to every F16X3 kernel
  bool stats_invariant_only = false;   // (the VQ-VAE decoder) GroupNorm partials only from batch-independent statistics tiles
  // magnitude-bound slots of this forward (CsConvGemm.a_bound; unet.py::_slot / ops.range_bound): one small zeroed region
  Buf amax_arena;
  int amax_next = 0, amax_cap = 0;
  std::vector<FreeBlock> fl;

  ExecBase(const Plan& pl_, const void* arena_, void* ws_, int64_t ws_bytes_, bool dry_, hipStream_t st_)
      : pl(pl_), arena((const char*)arena_), ws((char*)ws_), ws_bytes(ws_bytes_), dry(dry_), st(st_) {
    fl.push_back({0, dry ? (int64_t)1 << 60 : ws_bytes});
  }
  bool ok() const { return rc == CS_OK; }
  void chk(int r) {
    if (rc == CS_OK && r != CS_OK) rc = r;
  }
  float* p(const Buf& b) const { return reinterpret_cast<float*>(ws + b.off); }
  const float* wf(int64_t off) const { return reinterpret_cast<const float*>(arena + off); }

  Buf alloc(int64_t rows, int c) {
    Buf b;
    b.rows = rows;
    b.c = c;
    b.bytes = align_up(rows * c * 4);
    for (size_t i = 0; i < fl.size(); ++i) {
      if (fl[i].size >= b.bytes) {
        b.off = fl[i].off;
        fl[i].off += b.bytes;
        fl[i].size -= b.bytes;
        if (fl[i].size == 0) fl.erase(fl.begin() + i);
        if (b.off + b.bytes > peak) peak = b.off + b.bytes;
        return b;
      }
    }
    chk(CS_ENOMEM);
    b.off = 0;
    return b;
  }
  void release_region(int64_t off, int64_t bytes) {
    Buf t;
    t.off = off;
    t.bytes = bytes;
    release_data(t);
  }
  void amax_begin(int slots) {
    if (pl.math != CS_MATH_F16X3 || cs_debug()->no_dyn_scale || cs_debug()->no_gn_parts) return;
    amax_arena = alloc(slots, 1);
    amax_cap = ok() ? slots : 0;
    amax_next = 0;
    if (ok() && !dry && hipMemsetAsync(ws + amax_arena.off, 0, (size_t)slots * 4, st) != hipSuccess) chk(CS_EINVAL);
  }
  // split-K arrival counters of this forward (CsConvGemm.splitk_sync, ops.py::sync_words): zeroed with the bound slots'
  // region (one memset), returned to zero by the kernels that use them
  Buf sync_arena;
  static constexpr int SYNC_WORDS = 8192;
  void sync_begin() {
    if (pl.math != CS_MATH_F16X3) return;
    sync_arena = alloc(SYNC_WORDS, 1);
    if (ok() && !dry && hipMemsetAsync(ws + sync_arena.off, 0, (size_t)SYNC_WORDS * 4, st) != hipSuccess) chk(CS_EINVAL);
  }
  int64_t amax_slot() {       // a fresh slot's workspace offset, or -1 (feature off / arena exhausted)
    if (amax_next >= amax_cap) return -1;
    return amax_arena.off + 4 * (int64_t)amax_next++;
  }
  Stat alloc_stat(int64_t tiles, int nch, int nb, int tps, int ncls) {
    Buf t = alloc(tiles * nch * 4, 1);          // [tiles][nch][2] doubles = 16 bytes per (tile, column)
    Stat st;
    st.off = t.off;
    st.bytes = t.bytes;
    st.nch = nch; st.nb = nb; st.tps = tps; st.ncls = ncls;
    return st;
  }
  // a private copy of a producer's partials (the guidance split: the shared tensor lives on as a skip, its duplicate feeds
  // the next GroupNorm; each copy is released with its buffer)
  Stat dup_stat(const Stat& a) {
    if (!a.valid()) return Stat();
    Stat st = alloc_stat(a.bytes / ((int64_t)a.nch * 16), a.nch, a.nb, a.tps, a.ncls);
    if (ok() && !dry && hipMemcpyAsync(ws + st.off, ws + a.off, (size_t)a.bytes, hipMemcpyDeviceToDevice, this->st) != hipSuccess)
      chk(CS_EINVAL);
    return st;
  }
  void release(Buf& b) {
    for (int i = 0; i < 2; ++i)
      if (b.seg[i].valid()) {
        release_region(b.seg[i].off, b.seg[i].bytes);
        b.seg[i] = Stat();
      }
    b.nseg = 0;
    release_data(b);
  }
  void release_data(Buf& b) {
    if (b.off < 0 || b.bytes == 0) return;
    size_t i = 0;
    while (i < fl.size() && fl[i].off < b.off) ++i;
    fl.insert(fl.begin() + i, {b.off, b.bytes});
    if (i + 1 < fl.size() && fl[i].off + fl[i].size == fl[i + 1].off) {
      fl[i].size += fl[i + 1].size;
      fl.erase(fl.begin() + i + 1);
    }
    if (i > 0 && fl[i - 1].off + fl[i - 1].size == fl[i].off) {
      fl[i - 1].size += fl[i].size;
      fl.erase(fl.begin() + i);
    }
    b.off = -1;
    b.bytes = 0;
  }

  // launch-argument pointer into a buffer (+ an offset in floats); the sizing pass carries none
  float* at(const Buf& b, int64_t off = 0) const { return dry ? nullptr : p(b) + off; }

  // the operand view of b from row `row0` on (a row range: fp32 and pre-split buffers only).  The lo image of a pre-split
  // pair / of a Winograd-W operand follows the hi image's rows x c halves
  View view(const Buf& b, int64_t row0 = 0) const {
    View a;
    a.lda = b.c;
    a.a_scale = b.a_scale;
    a.format = b.wino == 4 ? 4 : b.wino ? 3 : b.half ? 1 : b.pair ? 2 : 0;
    if (dry) return a;
    const bool halves = b.half || b.wino;
    const char* base = reinterpret_cast<const char*>(p(b));
    a.x = reinterpret_cast<const float*>(base + row0 * b.c * (halves ? 2 : 4));
    if (halves) a.x_lo = base + (b.rows + row0) * b.c * 2;
    return a;
  }

  // output extent of a k-tap "same"-padded conv with stride s over an extent upsampled by 2^up
  static int conv_out(int in, int up, int k, int s) { return ((in << up) + 2 * (k / 2) - k) / s + 1; }

  // THE descriptor of plan GEMM g reading operand view a of an [nb, d, h, w] volume and writing [.][ldo] rows at `out`:
  // the weight pack that goes with the operand format, geometry, epilogue terms.  The operand format is part of what the
  // plan and tile rules look at: it is set in the sizing pass too, so that both passes ask them about the same launch
  void describe(CsConvGemm& q, const Gemm& g, const View& a, float* out, int ldo, int nb, int d, int h, int w,
                const GemmOpts& o) const {
    memset(&q, 0, sizeof(q));
    q.a_format = a.format;
    if (!dry) {
      const Gemm::Pack pk = g.pack(a.wino());
      q.x = a.x;
      q.x_lo = a.x_lo;
      q.out = out;
      q.w = wf(pk.w);
      if (pl.math == CS_MATH_F16X3) {
        q.w_lo = arena + pk.lo;
        q.acc_scale = pk.acc * (16.0f / a.a_scale);      // pk.acc = 1 / (weight scale * 16); powers of two
        q.a_scale = a.a_scale;
        // a RAW activation whose magnitude bound sits in a workspace slot (range_bound / the GroupNorm over it): the kernel
        // derives the operand scale from it instead of the fixed one (ops.py: x_bound=)
        if (o.a_bound_off >= 0 && a.format == 0) q.a_bound = reinterpret_cast<const float*>(ws + o.a_bound_off);
      }
      q.bias = (g.b_off >= 0 && !g.tap_cout) ? wf(g.b_off) : nullptr;      // (taps as columns: cs_tapsum27 adds it)
      q.rowvec = o.rowvec;
      q.res = o.res_off >= 0 ? reinterpret_cast<const float*>(ws + o.res_off) : nullptr;
      q.status = status;
    }
    q.nb = nb; q.din = d; q.hin = h; q.win = w;
    q.dout = conv_out(d, o.up_d, g.k, o.s_d);
    q.hout = conv_out(h, o.up_hw, g.k, o.s_hw);
    q.wout = conv_out(w, o.up_hw, g.k, o.s_hw);
    q.cin = g.cin_pad; q.cout = g.cout;
    q.lda = a.lda; q.ldw = g.ldw; q.ldo = ldo; q.ldr = q.res ? o.ldr : 0; q.ldrv = q.rowvec ? o.ldrv : 0;
    q.kd = q.kh = q.kw = g.k;
    q.sd = o.s_d; q.sh = q.sw = o.s_hw;
    q.pd = q.ph = q.pw = g.k / 2;
    q.ud = o.up_d; q.uh = q.uw = o.up_hw;
    q.act = o.act; q.rv_rows = o.rv_rows; q.math = pl.math; q.tile = o.tile;
  }

  // small batches: few output tiles -> the K loop cut into slices (cs_conv_gemm_plan, the plan function the Python host
  // calls); Winograd-W: the position results (x K slices) live in the workspace, output transform + epilogue in the reduce
  // kernel (cs_conv_wino_plan).  skws: the region, released by the caller after the launch.  The sizing pass allocates it too
  bool plan_splitk(CsConvGemm& q, Buf& skws) {
    const bool wino = q.a_format >= 3;
    int32_t sk = 1;
    int64_t wsb = 0;
    if (wino) {
      if (cs_conv_wino_plan(&q, &sk, &wsb) != CS_OK) chk(CS_EINVAL);
    } else if (q.tile != 0 || cs_conv_gemm_plan(&q, &sk, &wsb) != CS_OK || sk <= 1) {
      return true;
    }
    if (ok()) skws = alloc(wsb / 4, 1);
    if (!ok()) return false;
    q.splitk = sk;
    q.splitk_ws = at(skws);
    if (!wino && sync_arena.off >= 0 && !dry) {
      q.splitk_sync = reinterpret_cast<int32_t*>(ws + sync_arena.off);
      q.splitk_sync_words = SYNC_WORDS;
    }
    return true;
  }

  // the one GEMM path: descriptor, plan and workspace, epilogue extras, launch.  dst (optional): the Buf behind `out`, which
  // takes the GroupNorm partials (want_stats) and the pair format (out_pair) where the launch can leave them
  void launch_gemm(const Gemm& g, const View& a, float* out, int ldo, int nb, int d, int h, int w, const GemmOpts& o,
                   Buf* dst = nullptr) {
    if (a.wino() && (g.pack(a.wino()).w < 0 || g.k != 3 || pl.math != CS_MATH_F16X3 || o.s_hw != 1 || o.s_d != 1 || o.up_hw ||
                     o.up_d || o.tile || o.a_bound_off >= 0)) {
      chk(CS_EINVAL);
      return;
    }
    CsConvGemm q;
    describe(q, g, a, out, ldo, nb, d, h, w, o);
    const bool extras = dst && !g.tap_cout;
    if (g.up_mask) {
      // Upsample's conv on the source grid: one GEMM per output parity class + interleave (cs_conv_gemm_up2)
      if (g.up_mask != ((o.up_d << 2) | (o.up_hw << 1) | o.up_hw) || o.s_hw != 1 || o.s_d != 1 || o.res_off >= 0 || o.rowvec ||
          o.tile || a.a_scale != 16.f) {
        chk(CS_EINVAL);
        return;
      }
      const int64_t ub = cs_conv_gemm_up2_ws_bytes(&q);
      if (ub <= 0) {
        chk(CS_EINVAL);
        return;
      }
      Buf uws = alloc(ub / 4, 1);
      if (!ok()) return;
      if (o.want_stats && extras) stats_for(q, g, o, *dst, (int64_t)d * h * w, g.ncls);
      if (!dry) {
        const void* wc[8];
        const void* wl[8];
        for (int c = 0; c < g.ncls; ++c) {
          wc[c] = arena + g.cls_w_off[c];
          wl[c] = arena + g.cls_wlo_off[c];
        }
        chk(cs_conv_gemm_up2(&q, wc, wl, g.cls_acc_scale, p(uws), st));
      }
      release(uws);
      return;
    }
    Buf skws;
    if (!plan_splitk(q, skws)) return;
    if (o.want_stats && extras) stats_for(q, g, o, *dst, (int64_t)q.dout * q.hout * q.wout, 1);
    if (o.out_pair > 0.f && extras && pl.math == CS_MATH_F16X3) {
      // the result's only reader is the next F16X3 GEMM: written as the interleaved operand pair where the launch can
      // (ops.py::conv_gemm out_pair=).  Asked in the sizing pass too -- same bytes either way, but the consumer's tile rule
      // looks at its operand format
      int32_t pair = 0;
      CsConvGemm probe = q;
      if (dry) dry_operands(probe, g, o);
      if (!cs_debug()->no_pair_epilogue && cs_conv_gemm_epilogue_caps(&probe, nullptr, &pair) == CS_OK && pair) {
        q.out_format = 2;
        q.out_scale = o.out_pair;
        dst->pair = true;
        dst->a_scale = o.out_pair;
      }
    }
    if (!dry) chk(cs_conv_gemm(&q, st));
    release(skws);      // stream-ordered: later kernels that reuse the region run after the reduce
  }

  // conv (k^3 taps, stride (s_d,s_hw,s_hw), nearest upsample (up_d,up_hw,up_hw)) or pointwise/linear GEMM with the fused
  // epilogue, into a fresh buffer.  want_stats: the result feeds a GroupNorm -- where the launch can
  // (cs_conv_gemm_epilogue_caps: the one rule both hosts ask), its epilogue leaves the per-(row tile, column) partial sums
  // and the returned buffer carries them (seg[0])
  Buf gemm(const Buf& x, int gi, int nb, int d, int h, int w, const GemmOpts& o = GemmOpts()) {
    const Gemm& g = pl.gemms[gi];
    const int64_t voxels = (int64_t)nb * d * h * w;
    if (g.tap_cout) {      // taps as columns: the pointwise GEMM, then cs_tapsum27
      if (o.s_hw != 1 || o.s_d != 1 || o.up_hw || o.up_d || o.act != CS_ACT_NONE || o.rowvec || o.res_off >= 0 || o.tile ||
          x.half) {
        chk(CS_EINVAL);
        return Buf();
      }
      GemmOpts ot = o;
      ot.tile = cs_tapcol_tile(voxels, g.cout);
      Buf cols = gemm_fresh(x, g, nb, d, h, w, ot);
      if (!ok()) return cols;
      Buf out = alloc(voxels, g.tap_cout);
      if (ok() && !dry)
        chk(cs_tapsum27(p(cols), g.b_off >= 0 ? wf(g.b_off) : nullptr, p(out), nb, d, h, w, g.tap_cout, g.cout, g.tap_cout, st));
      release(cols);
      return out;
    }
    return gemm_fresh(x, g, nb, d, h, w, o);
  }
  Buf gemm_fresh(const Buf& x, const Gemm& g, int nb, int d, int h, int w, const GemmOpts& o) {
    const int64_t voxels = (int64_t)nb * d * h * w;
    const int64_t mo =
        (int64_t)nb * conv_out(d, o.up_d, g.k, o.s_d) * conv_out(h, o.up_hw, g.k, o.s_hw) * conv_out(w, o.up_hw, g.k, o.s_hw);
    Buf out = alloc(mo, o.act == CS_ACT_GEGLU ? g.cout / 2 : g.cout);
    if (!ok()) return out;
    if (x.c != g.cin_pad || x.rows != (x.wino ? wino_rows(x.wino, voxels) : voxels)) {
      chk(CS_EINVAL);
      return out;
    }
    launch_gemm(g, view(x), at(out), out.c, nb, d, h, w, o, &out);
    return out;
  }
  Buf linear(const Buf& x, int gi, const GemmOpts& o = GemmOpts()) { return gemm(x, gi, (int)x.rows, 1, 1, 1, o); }
  // the same path on explicit views -- channel ranges of wider buffers, sample ranges of a batch (res_block_split): a
  // stride-1 conv / pointwise GEMM of operand view a into rows of stride ldo at `out`
  void gemm_view(const View& a, int gi, int nb, int d, int h, int w, float* out, int ldo, const GemmOpts& o = GemmOpts()) {
    launch_gemm(pl.gemms[gi], a, out, ldo, nb, d, h, w, o);
  }

  // ops.py::_epilogue_extras: ask the library what the launch's epilogue can emit and point the descriptor at a fresh
  // partials region (rps = rows per sample -- per class -- the statistics tiles run over).
  // The sizing pass carries no pointers, but cs_conv_gemm_epilogue_caps looks at which epilogue terms exist (and at their
  // alignment): aligned stand-ins for exactly the operands the real pass will set, so both passes get the same answer
  static void dry_operands(CsConvGemm& probe, const Gemm& g, const GemmOpts& o) {
    const float* some = reinterpret_cast<const float*>((uintptr_t)256);
    probe.out = const_cast<float*>(some);
    probe.bias = g.b_off >= 0 ? some : nullptr;
    probe.res = o.ldr > 0 ? some : nullptr;
    probe.ldr = o.ldr;
    probe.rowvec = o.ldrv > 0 ? some : nullptr;
    probe.ldrv = o.ldrv;
  }
  void stats_for(CsConvGemm& q, const Gemm& g, const GemmOpts& o, Buf& out, int64_t rps, int ncls) {
    if (cs_debug()->no_gn_parts || pl.math != CS_MATH_F16X3) return;
    CsConvGemm probe = q;
    if (dry) dry_operands(probe, g, o);
    int32_t rows = 0;
    if (cs_conv_gemm_epilogue_caps(&probe, &rows, nullptr) != CS_OK || rows <= 0) return;
    if (stats_invariant_only) {
      // only where ONE sample's launch picks the same statistics tiles (ops.py::_epilogue_extras, stats="invariant": the VQ
      // decoder's bit-exact batch invariance) -- the SAME kernel variant (tile code, slab width, statistics rows) at one
      // sample, at the decode slice limit of sixteen and at this batch
      int32_t t0 = 0, s0 = 0;
      if (q.nb > 16 || cs_conv_gemm_launch_info(&probe, &t0, &s0) != CS_OK) return;
      for (int nbp : {1, 16}) {
        CsConvGemm one = probe;
        one.nb = nbp;
        int32_t r1 = 0, t1 = 0, s1 = 0;
        if (cs_conv_gemm_epilogue_caps(&one, &r1, nullptr) != CS_OK || cs_conv_gemm_launch_info(&one, &t1, &s1) != CS_OK ||
            r1 != rows || t1 != t0 || s1 != s0)
          return;
      }
    }
    const int64_t tiles = (q.nb * rps + rows - 1) / rows;
    Stat sx = alloc_stat((int64_t)ncls * tiles, q.cout, q.nb, (int)(rps / rows), ncls);
    if (!ok()) return;
    out.seg[0] = sx;
    out.nseg = 1;
    q.gn_part = dry ? nullptr : reinterpret_cast<double*>(ws + sx.off);
    q.gn_ld = q.cout;
    q.gn_rows = rows;
  }
  // do x's segments cover its channels?  (ops.py::stats_segments)
  bool has_parts(const Buf& x) const {
    if (cs_debug()->no_gn_parts || x.nseg < 1) return false;
    int n = 0;
    for (int i = 0; i < x.nseg; ++i) {
      if (!x.seg[i].valid()) return false;
      n += x.seg[i].nch;
    }
    return n == x.c;
  }
  float* bound_ptr(int64_t off) const { return off >= 0 ? reinterpret_cast<float*>(ws + off) : nullptr; }
  // (mean, rstd) -> stats (may be NULL) and the magnitude bound -> slot boff (may be -1) from the producers' partials:
  // ops.py::groupnorm_stats_from_parts
  void finalize_parts(const Buf& x, int nb, float eps, int groups, float* stats, int64_t boff) {
    if (!ok() || dry) return;
    CsGnSeg sg[2];
    seg_array(x, sg);
    chk(cs_groupnorm_finalize_parts(sg, x.nseg, nb, (int)(x.rows / nb), x.c, groups, eps, stats, bound_ptr(boff), st));
  }
  void seg_array(const Buf& x, CsGnSeg* sg) const {
    int ch0 = 0;
    for (int i = 0; i < x.nseg; ++i) {
      const Stat& a = x.seg[i];
      sg[i].part = reinterpret_cast<const double*>(ws + a.off);
      sg[i].ld = a.nch; sg[i].col0 = 0; sg[i].ch0 = ch0; sg[i].nch = a.nch;
      sg[i].tiles_per_sample = a.tps; sg[i].ncls = a.ncls; sg[i].nb_src = a.nb; sg[i].reserved = 0;
      ch0 += a.nch;
    }
  }
  // GroupNorm, step one: the statistics of x and (want_bound: a consumer will read x RAW, ops.py::groupnorm bound=) its
  // magnitude bound in a fresh slot (-1: feature off / arena exhausted).  The source is the producers' partials -- the
  // tensor is then read once -- or a statistics pass, which needs scratch.  alloc / run / release are separate because the
  // single-launch forms of groupnorm() compute the statistics themselves
  struct GnStats {
    Buf stats, wsb;
    int64_t bound = -1;
    bool parts = false;
  };
  GnStats gn_stats_alloc(const Buf& x, int nb, int groups, bool want_bound) {
    GnStats s;
    s.parts = has_parts(x);
    if (!s.parts) s.wsb = alloc((cs_groupnorm_ws_bytes(nb, groups) + 3) / 4, 1);
    s.stats = alloc((int64_t)nb * groups * 2, 1);
    if (want_bound) s.bound = amax_slot();
    return s;
  }
  void gn_stats_run(const Buf& x, int nb, float eps, int groups, const GnStats& s) {
    if (s.parts) return finalize_parts(x, nb, eps, groups, at(s.stats), s.bound);
    if (!ok() || dry) return;
    const int rows = (int)(x.rows / nb);
    chk(s.bound >= 0
            ? cs_groupnorm_stats_bound(p(x), nb, rows, x.c, x.c, groups, eps, p(s.wsb), p(s.stats), bound_ptr(s.bound), st)
            : cs_groupnorm_stats(p(x), nb, rows, x.c, x.c, groups, eps, p(s.wsb), p(s.stats), st));
  }
  void gn_stats_release(GnStats& s) {
    release(s.wsb);
    release(s.stats);
  }

  // ops.py::range_bound: the magnitude bound of a RAW tensor that no GroupNorm follows, from its producers' partials, into
  // a fresh slot; -1 when x carries none (the consumer then keeps the fixed scale)
  int64_t range_bound(const Buf& x, int nb, int groups = 32) {
    if (x.c % groups) return -1;
    const int64_t off = amax_slot();
    if (off < 0) return -1;
    if (has_parts(x)) {
      finalize_parts(x, nb, 1e-5f, groups, nullptr, off);
      return off;
    }
    // no partials (e.g. a folded Upsample conv at a small batch): one statistics pass over the (small) tensor
    GnStats s;
    s.wsb = alloc((cs_groupnorm_ws_bytes(nb, groups) + 3) / 4, 1);
    s.stats = alloc((int64_t)nb * groups * 2, 1);
    s.bound = off;
    gn_stats_run(x, nb, 1e-5f, groups, s);
    gn_stats_release(s);
    return off;
  }

  // GroupNorm, step two: the buffer for c normalised channels of rows_total rows in the operand format the consuming conv
  // `conv_gi` (-1: none) wants -- wn > 0: the Winograd-W operand, variant wn (what wants_wino answered), at 1/2 resp. 1/16 of
  // the normalisation's operand scale (|transformed| <= 2 x resp. 10 x the activation's bound; ops.py::groupnorm wino=);
  // else the pre-split pair where wants_split16 says so for m_launch rows per launch of that conv; else fp32 -- ...
  Buf gn_out(const Norm& n, int64_t rows_total, int c, int nb, int cpg, int wn, int conv_gi, int64_t m_launch) {
    Buf y = alloc(wn ? wino_rows(wn, rows_total) : rows_total, c);
    if (pl.math == CS_MATH_F16X3) y.a_scale = norm_a_scale(n.gmax, n.bmax, rows_total / nb * cpg);
    if (wn) {
      y.wino = wn;
      y.a_scale *= wn == 2 ? 0.5f : 0.0625f;
    } else {
      y.half = wants_split16(m_launch, conv_gi);
    }
    return y;
  }
  // ... and the apply (+ activation) that fills it with channels [ch0, ch0 + y.c) of the normalised tensor: x points at
  // channel ch0 of the first row, row stride ldx; nb samples of `rows` rows (the Winograd-W operand: of the d x h x w
  // volume); stats = their (mean, rstd) pairs
  void gn_emit(const float* x, int ldx, const float* stats, const Norm& n, const Buf& y, int nb, int rows, int d, int h, int w,
               int groups, int cpg, int ch0, int act) {
    if (!ok() || dry) return;
    const float *gamma = wf(n.g_off) + ch0, *beta = wf(n.b_off) + ch0;
    const int c = y.c;
    char* hi = reinterpret_cast<char*>(p(y));
    if (y.wino)
      chk(cs_groupnorm_apply_wino_range(x, stats, gamma, beta, hi, hi + y.rows * c * 2, nb, d, h, w, c, ldx, c, groups, cpg, ch0,
                                        act, y.a_scale, y.wino, status, st));
    else if (y.half)
      chk(cs_groupnorm_apply_split16_range(x, stats, gamma, beta, hi, hi + y.rows * c * 2, nb, rows, c, ldx, c, groups, cpg, ch0,
                                           act, y.a_scale, status, st));
    else
      chk(cs_groupnorm_apply_range(x, stats, gamma, beta, p(y), nb, rows, c, ldx, c, groups, cpg, ch0, act, st));
  }

  // GroupNorm (+ activation) of x, nb samples.  conv_gi: the 3x3x3 conv that consumes the result (decides the output
  // format), or -1; d, h, w: the volume's extents where that conv may take the Winograd-W route (the ResBlocks), else 0;
  // bound_off (out, optional): wanted when a consumer will read x RAW (the ResBlock's skip conv) -- the slot x's magnitude
  // bound went to, -1 if none.  ops.py::groupnorm
  Buf groupnorm(const Buf& x, int ni, int nb, float eps, int act, int groups = 32, int conv_gi = -1,
                int64_t* bound_off = nullptr, int d = 0, int h = 0, int w = 0) {
    const Norm& n = pl.norms[ni];
    const int rows = (int)(x.rows / nb), cpg = x.c / groups;
    Buf y = gn_out(n, x.rows, x.c, nb, cpg, wants_wino(conv_gi, nb, d, h, w), conv_gi, x.rows);
    GnStats s = gn_stats_alloc(x, nb, groups, bound_off != nullptr);
    if (bound_off) *bound_off = s.bound;
    if (y.wino || y.half || (!s.parts && s.bound >= 0)) {
      gn_stats_run(x, nb, eps, groups, s);
      gn_emit(at(x), x.c, at(s.stats), n, y, nb, rows, d, h, w, groups, cpg, 0, act);
    } else if (ok() && !dry) {
      // fp32 result: ONE call each -- from partials a single launch for small tensors, finalize + apply otherwise
      // (cs_groupnorm_parts decides); without partials and without a bound cs_groupnorm (one launch while the tensor is small)
      if (s.parts) {
        CsGnSeg sg[2];
        seg_array(x, sg);
        chk(cs_groupnorm_parts(p(x), sg, x.nseg, wf(n.g_off), wf(n.b_off), p(y), nb, rows, x.c, x.c, x.c, groups, eps, act,
                               p(s.stats), bound_ptr(s.bound), st));
      } else {
        chk(cs_groupnorm(p(x), wf(n.g_off), wf(n.b_off), p(y), nb, rows, x.c, x.c, x.c, groups, eps, act, p(s.wsb), p(s.stats),
                         st));
      }
    }
    gn_stats_release(s);
    return y;
  }
  Buf layernorm(const Buf& x, int ni) {
    const Norm& n = pl.norms[ni];
    Buf y = alloc(x.rows, x.c);
    if (pl.math == CS_MATH_F16X3) y.a_scale = norm_a_scale(n.gmax, n.bmax, x.c);
    // LayerNorm outputs only ever feed GEMMs: in F16X3 mode they are written as the interleaved operand pair
    // (ops.py::layernorm pair_scale; CS_NO_PAIR16=1 keeps fp32 for A/B runs)
    y.pair = pl.math == CS_MATH_F16X3 && !cs_debug()->no_pair16 && x.c % 16 == 0;
    if (!ok() || dry) return y;
    chk(y.pair ? cs_layernorm_pair16(p(x), wf(n.g_off), wf(n.b_off), p(y), (int)x.rows, x.c, x.c, x.c, 1e-5f, y.a_scale, status, st)
               : cs_layernorm(p(x), wf(n.g_off), wf(n.b_off), p(y), (int)x.rows, x.c, x.c, x.c, 1e-5f, st));
    return y;
  }

  // does the GroupNorm feeding conv `gi` over m output rows emit the pre-split operand pair?  (cs_conv_wants_split16: the
  // one rule, csrc/cs_plan.hip; bit-identical to the fp32 route either way)
  bool wants_split16(int64_t m, int gi) const {
    if (gi < 0) return false;
    const Gemm& g = pl.gemms[gi];
    return cs_conv_wants_split16(m, g.cin, g.cout, g.k, !g.up_mask && !g.tap_cout && g.cin_pad == g.cin, pl.math) != 0;
  }
  // does the GroupNorm feeding the 3x3x3 conv `gi` over an [nb, d, h, w] volume emit the Winograd-W operand, and which
  // variant (0 = direct form, 2 = F(2,3), 4 = F(4,3))?  (cs_conv_wino_ok: the one rule; ops.py::wants_wino)
  int wants_wino(int gi, int nb, int d, int h, int w) const {
    if (gi < 0 || d <= 0 || pl.math != CS_MATH_F16X3 || cs_debug()->no_split16) return 0;
    const Gemm& g = pl.gemms[gi];
    if (g.wino_off < 0) return 0;
    CsConvGemm q;
    memset(&q, 0, sizeof(q));
    q.nb = nb; q.din = q.dout = d; q.hin = q.hout = h; q.win = q.wout = w;
    q.cin = g.cin_pad; q.cout = g.cout; q.lda = g.cin_pad; q.ldo = g.cout; q.ldw = g.ldw;
    q.kd = q.kh = q.kw = 3;
    q.sd = q.sh = q.sw = q.pd = q.ph = q.pw = 1;
    q.math = pl.math; q.rv_rows = 1;
    const int v = cs_conv_wino_ok(&q);
    return v == 4 ? (g.wino4_off >= 0 ? 4 : 2) : v;
  }
  // rows of the Buf that holds variant v's operand of a volume of `voxels` rows
  static int64_t wino_rows(int v, int64_t voxels) { return voxels / v * (v + 2); }

  // the F16X3 operand scales of an attention block fed by a GroupNorm (cs_attnblock_static_scales: the one rule; vqvae.py /
  // unet.py call it with the same statistics) -- false: feature off / not F16X3 / no statistics, the constant 16 then
  bool attnblock_scales(int norm, int64_t n_per_group, int c, float w_l2max, float b_absmax, float qk_scale, float out4[4]) const {
    if (pl.math != CS_MATH_F16X3 || cs_debug()->no_static_scales || !(w_l2max > 0.f)) return false;
    const Norm& nm = pl.norms[norm];
    return cs_attnblock_static_scales(nm.gmax, nm.bmax, n_per_group, c, w_l2max, b_absmax, qk_scale, out4) == CS_OK;
  }

  // self-attention over a fused [rows][3c] q | k | v buffer -> a [rows][c]; F16X3: K / V tile images in a scratch buffer
  // where the library has that path (cs_attn_f16x3_ws_bytes > 0; ops.py::attention does the same)
  // qkv_scales: the static-bound operand scales of q * scale, k, v (cs_transformer_static_scales), or nullptr = 16
  void self_attention(const Buf& qkv, const Buf& a, int nb, int n, int heads, int dh, int c, float scale,
                      const float* qkv_scales = nullptr) {
    const bool f16 = pl.math == CS_MATH_F16X3;
    const int64_t wsb = f16 ? cs_attn_f16x3_ws_bytes(nb, n, n, heads, dh) : 0;
    Buf img;
    if (wsb > 0) img = alloc(wsb / 4, 1);
    if (ok() && !dry) {
      const float *q = p(qkv), *k = q + c, *v = q + 2 * c, *s = qkv_scales;
      const int ld = 3 * c;
      void* iw = wsb > 0 ? (void*)p(img) : nullptr;
      chk(!f16 ? cs_attn_selfattn(q, k, v, p(a), nb, n, n, heads, dh, ld, ld, ld, c, scale, st)
          : !s ? cs_attn_selfattn_f16x3_ws(q, k, v, p(a), nb, n, n, heads, dh, ld, ld, ld, c, scale, status, iw, st)
          : iw ? cs_attn_selfattn_f16x3_ws_scaled(q, k, v, p(a), nb, n, n, heads, dh, ld, ld, ld, c, scale, s[0], s[1], s[2],
                                                  status, iw, st)
               : cs_attn_selfattn_f16x3_scaled(q, k, v, p(a), nb, n, n, heads, dh, ld, ld, ld, c, scale, s[0], s[1], s[2], status,
                                               st));
    }
    release(img);
  }
};

}  // namespace
