// The pieces of OpenAI CLIP ViT-B/32 (clip/model.py) that the GEMM, LayerNorm and unmasked-attention kernels do not cover:
//   * cs_clip_patchify               uint8 HWC image -> normalised fp32 patch rows (the A operand of conv1 as a GEMM)
//   * cs_clip_assemble_image_tokens  [class_embedding | patch rows] + positional_embedding
//   * cs_clip_embed_text             token_embedding[ids] + positional_embedding
//   * cs_clip_quick_gelu             x * sigmoid(1.702 x)
//   * cs_clip_attn_causal            the text tower's attention: query i sees keys j <= i
//   * cs_clip_pool_eot               the hidden row at the first maximum of ids[b, :]
//   * cs_feature_pair_l2             ||f_a - f_b||_2 for a list of pairs (consistency_check.py:65)
// All math is fp32.  Every entry only launches; none synchronises.
#include "cs_common.h"

namespace {

constexpr int EL_T = 256;

// ---- front ends -------------------------------------------------------------------------------------------------------
// one thread per pixel (x fastest): three byte reads, three stores that are contiguous along px inside a patch row
__global__ __launch_bounds__(EL_T) void clip_patchify_kernel(const uint8_t* __restrict__ img, float* __restrict__ out,
                                                             int64_t npix, int s, int p, int ldo, float m0, float m1,
                                                             float m2, float s0, float s1, float s2) {
  const int g = s / p;
  const float mean[3] = {m0, m1, m2}, sd[3] = {s0, s1, s2};
  for (int64_t i = blockIdx.x * (int64_t)EL_T + threadIdx.x; i < npix; i += (int64_t)gridDim.x * EL_T) {
    const int x = (int)(i % s), y = (int)((i / s) % s);
    const int64_t b = i / ((int64_t)s * s);
    const int gx = x / p, px = x - gx * p, gy = y / p, py = y - gy * p;
    float* row = out + ((b * g + gy) * g + gx) * (int64_t)ldo + py * p + px;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float u = (float)img[3 * i + c];
      row[c * p * p] = ((u / 255.0f) - mean[c]) / sd[c];       // torchvision ToTensor + Normalize: two IEEE divisions
    }
  }
}

// x[b][0] = cls + pos[0];  x[b][1 + t] = patch[b][t] + pos[1 + t]
__global__ __launch_bounds__(EL_T) void clip_assemble_kernel(const float* __restrict__ patch, const float* __restrict__ cls,
                                                             const float* __restrict__ pos, float* __restrict__ x,
                                                             int ntok, int w, int ldp, int ldx) {
  const int64_t r = blockIdx.x;                 // output row: b * (ntok + 1) + t
  const int t = (int)(r % (ntok + 1));
  const int64_t b = r / (ntok + 1);
  const float* src = t == 0 ? cls : patch + (b * ntok + (t - 1)) * (int64_t)ldp;
  const float* pr = pos + (int64_t)t * w;
  float* dst = x + r * ldx;
  for (int c = threadIdx.x; c < w; c += EL_T) dst[c] = src[c] + pr[c];
}

// x[b][t] = table[ids[b][t]] + pos[t]; an id outside [0, vocab) writes a NaN row and flags *err, nothing is read through it
__global__ __launch_bounds__(EL_T) void clip_embed_text_kernel(const float* __restrict__ table,
                                                               const int32_t* __restrict__ ids,
                                                               const float* __restrict__ pos, float* __restrict__ x, int t,
                                                               int w, int vocab, int ldx, int32_t* __restrict__ err) {
  const int64_t r = blockIdx.x;
  const int id = ids[r];
  float* dst = x + r * ldx;
  if (id < 0 || id >= vocab) {                  // compared BEFORE anything is read through it
    for (int c = threadIdx.x; c < w; c += EL_T) dst[c] = __builtin_nanf("");
    if (threadIdx.x == 0) atomicOr(err, 1);
    return;
  }
  const float* src = table + (int64_t)id * w;
  const float* pr = pos + (r % t) * w;
  for (int c = threadIdx.x; c < w; c += EL_T) dst[c] = src[c] + pr[c];
}

// ---- QuickGELU --------------------------------------------------------------------------------------------------------
// x * sigmoid(1.702 x) = x / (1 + exp(-1.702 x)).  At x = -20 the exponent is 34: rounding the product 1.702f * x to fp32
// (half an ulp of 34 = 1.9e-6) and 1.702f - 1.702 (2e-8 * 34) would each show as a RELATIVE error of that size in the result,
// so the product is carried as hi + lo and exp(-(hi + lo)) = exp(-hi) * (1 - lo) to first order (|lo| < 4e-6).
__device__ __forceinline__ float quick_gelu(float x) {
  constexpr float C = 1.702f;
  constexpr float C_LO = (float)(1.702 - (double)1.702f);
  const float hi = C * x;
  float e = expf(-hi);
  if (fabsf(hi) < __builtin_inff() && e < __builtin_inff()) {
    const float lo = fmaf(C, x, -hi) + C_LO * x;
    e = fmaf(-e, lo, e);
  }
  return x / (1.0f + e);          // e = inf: x / inf = -0 (x < 0); e = 0: x; NaN stays NaN
}

// (no __restrict__: y may be x -- every element is read and written by the same thread)
__global__ __launch_bounds__(EL_T) void clip_quick_gelu_kernel(const float* x, float* y, int64_t m, int c, int ldx, int ldy) {
  const int64_t n = m * c;
  for (int64_t i = blockIdx.x * (int64_t)EL_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * EL_T) {
    const int64_t r = i / c;
    const int col = (int)(i - r * c);
    y[r * ldy + col] = quick_gelu(x[r * ldx + col]);
  }
}

// ---- causal attention -------------------------------------------------------------------------------------------------
// One workgroup of four waves per (batch, head).  K and V of the head are staged once in LDS; wave w then owns the query
// rows w, w + 4, ...: lane j scores keys j and j + 64 (t <= 128), the wave reduces the maximum and the sum, and lane d
// accumulates output column d over the keys j <= i in key order.  A key j > i is never scored and never enters the
// sum: row i does not depend on its K / V values.  Each row's arithmetic depends on (i, dh) only, not on the launch.
//
// LDS layout: K rows are read as float4 by 64 lanes at 64 different rows, so the row stride is dh + 4 floats (one access
// width of padding): the 16 lanes of a ds_read_b128 group then fall on 16 different 16-byte slots.  V is read one dword
// per lane at consecutive columns of ONE row (conflict-free at any stride) and keeps the same stride for one index rule.
constexpr int AC_T = 256, AC_W = AC_T / 64, AC_MAX_T = 128, AC_MAX_DH = 64;

__global__ __launch_bounds__(AC_T) void clip_attn_causal_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                const float* __restrict__ v, float* __restrict__ out, int t,
                                                                int heads, int dh, int ldq, int ldk, int ldv, int ldo,
                                                                float scale) {
  extern __shared__ __attribute__((aligned(16))) float ac_smem[];
  const int lds = dh + 4;
  float* ks = ac_smem;                          // [t][lds]
  float* vs = ks + t * lds;                     // [t][lds]
  float* qs = vs + t * lds;                     // [AC_W][AC_MAX_DH]
  float* ps = qs + AC_W * AC_MAX_DH;            // [AC_W][AC_MAX_T]
  const int b = blockIdx.x / heads, h = blockIdx.x - b * heads;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row0 = (int64_t)b * t;
  const int d4n = dh >> 2;
  for (int i = tid; i < t * d4n; i += AC_T) {
    const int r = i / d4n, c = (i - r * d4n) << 2;
    *(float4*)(ks + r * lds + c) = *(const float4*)(k + (row0 + r) * ldk + h * dh + c);
    *(float4*)(vs + r * lds + c) = *(const float4*)(v + (row0 + r) * ldv + h * dh + c);
  }
  float* qw = qs + wave * AC_MAX_DH;
  float* pw = ps + wave * AC_MAX_T;
  // every wave runs the same number of rounds, so the barriers are met by all four (a round past t does no work)
  for (int i0 = 0; i0 < t; i0 += AC_W) {
    const int i = i0 + wave;
    const bool live = i < t;
    if (live && lane < dh) qw[lane] = q[(row0 + i) * ldq + h * dh + lane];
    __syncthreads();                            // K / V staged (first round); this round's q row visible
    float s[2] = {-__builtin_inff(), -__builtin_inff()};
    if (live) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int j = lane + 64 * u;
        if (j <= i) {
          const float* kr = ks + j * lds;
          float acc = 0.f;
          for (int c = 0; c < dh; c += 4) {
            const float4 kv = *(const float4*)(kr + c);
            const float4 qv = *(const float4*)(qw + c);
            acc = fmaf(qv.x, kv.x, acc);
            acc = fmaf(qv.y, kv.y, acc);
            acc = fmaf(qv.z, kv.z, acc);
            acc = fmaf(qv.w, kv.w, acc);
          }
          s[u] = acc * scale;
        }
      }
    }
    const float mx = wave_max(fmaxf(s[0], s[1]));           // key 0 is always seen: finite for finite inputs
    float p[2], sum = 0.f;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      p[u] = (live && lane + 64 * u <= i) ? expf(s[u] - mx) : 0.f;
      sum += p[u];
    }
    sum = wave_sum(sum);
    if (live) {
#pragma unroll
      for (int u = 0; u < 2; ++u)
        if (lane + 64 * u <= i) pw[lane + 64 * u] = p[u];
    }
    __syncthreads();                            // the wave's probabilities visible to its lanes
    if (live && lane < dh) {
      float acc = 0.f;
      for (int j = 0; j <= i; ++j) acc = fmaf(pw[j], vs[j * lds + lane], acc);
      out[(row0 + i) * ldo + h * dh + lane] = acc / sum;
    }
  }
}

// ---- pooling ----------------------------------------------------------------------------------------------------------
// out[b] = x[b][argmax_t ids[b][t]] with torch.argmax's tie rule for a tokenised text: the FIRST maximum
__global__ __launch_bounds__(EL_T) void clip_pool_eot_kernel(const float* __restrict__ x, const int32_t* __restrict__ ids,
                                                             float* __restrict__ out, int t, int w, int ldx, int ldo) {
  const int64_t b = blockIdx.x;
  const int32_t* mine = ids + b * t;
  int best = 0, bv = mine[0];
  for (int j = 1; j < t; ++j) {                 // the same scan in every thread: t is a context length (77)
    const int vj = mine[j];
    if (vj > bv) bv = vj, best = j;
  }
  const float* src = x + (b * t + best) * (int64_t)ldx;
  float* dst = out + b * ldo;
  for (int c = threadIdx.x; c < w; c += EL_T) dst[c] = src[c];
}

// ---- pair distance ----------------------------------------------------------------------------------------------------
// one wave per pair; lane l sums columns l, l + 64, ... in order, then the butterfly: out[k] depends on the two rows only
__global__ __launch_bounds__(EL_T) void feature_pair_l2_kernel(const float* __restrict__ f, const int32_t* __restrict__ pairs,
                                                               float* __restrict__ out, int n, int e, int npairs, int ld,
                                                               int32_t* __restrict__ err) {
  const int kk = blockIdx.x * (EL_T / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (kk >= npairs) return;
  const int a = pairs[2 * kk], b = pairs[2 * kk + 1];
  if (a < 0 || a >= n || b < 0 || b >= n) {     // compared BEFORE anything is read through them
    if (lane == 0) {
      out[kk] = __builtin_nanf("");
      atomicOr(err, 1);
    }
    return;
  }
  const float* fa = f + (int64_t)a * ld;
  const float* fb = f + (int64_t)b * ld;
  float acc = 0.f;
  for (int c = lane; c < e; c += 64) {
    const float d = fa[c] - fb[c];
    acc = fmaf(d, d, acc);
  }
  acc = wave_sum(acc);
  if (lane == 0) out[kk] = sqrtf(acc);
}

}  // namespace

extern "C" int cs_clip_patchify(const uint8_t* img, float* out, int nb, int s, int p, int ldo, float mean0, float mean1,
                                float mean2, float std0, float std1, float std2, cs_stream_t stream) {
  if (!img || !out || nb < 1 || s < 1 || p < 1 || s % p || ldo < 3 * p * p) return CS_EINVAL;
  if ((int64_t)nb * (s / p) * (s / p) > 0x7fffffffLL) return CS_EINVAL;
  const int64_t npix = (int64_t)nb * s * s;
  CS_LAUNCH(clip_patchify_kernel, dim3(cs_grid_for(npix, EL_T)), dim3(EL_T), 0, (hipStream_t)stream, img, out, npix, s, p,
            ldo, mean0, mean1, mean2, std0, std1, std2);
  CS_CHECK_LAUNCH();
  return CS_OK;
}

extern "C" int cs_clip_assemble_image_tokens(const float* patch_out, const float* class_embedding, const float* pos, float* x,
                                             int nb, int ntok, int w, int ldp, int ldx, cs_stream_t stream) {
  if (!patch_out || !class_embedding || !pos || !x || nb < 1 || ntok < 1 || w < 1 || ldp < w || ldx < w) return CS_EINVAL;
  const int64_t rows = (int64_t)nb * (ntok + 1);
  if (rows > 0x7fffffffLL) return CS_EINVAL;
  CS_LAUNCH(clip_assemble_kernel, dim3((unsigned)rows), dim3(EL_T), 0, (hipStream_t)stream, patch_out, class_embedding, pos,
            x, ntok, w, ldp, ldx);
  CS_CHECK_LAUNCH();
  return CS_OK;
}

extern "C" int cs_clip_embed_text(const float* token_embedding, const int32_t* ids, const float* pos, float* x, int nb, int t,
                                  int w, int vocab, int ldx, int32_t* err, cs_stream_t stream) {
  if (!token_embedding || !ids || !pos || !x || !err || nb < 1 || t < 1 || w < 1 || vocab < 1 || ldx < w) return CS_EINVAL;
  const int64_t rows = (int64_t)nb * t;
  if (rows > 0x7fffffffLL) return CS_EINVAL;
  CS_LAUNCH(clip_embed_text_kernel, dim3((unsigned)rows), dim3(EL_T), 0, (hipStream_t)stream, token_embedding, ids, pos, x, t,
            w, vocab, ldx, err);
  CS_CHECK_LAUNCH();
  return CS_OK;
}

extern "C" int cs_clip_quick_gelu(const float* x, float* y, int64_t m, int c, int ldx, int ldy, cs_stream_t stream) {
  if (!x || !y || m < 1 || c < 1 || ldx < c || ldy < c) return CS_EINVAL;
  CS_LAUNCH(clip_quick_gelu_kernel, dim3(cs_grid_for(m * c, EL_T)), dim3(EL_T), 0, (hipStream_t)stream, x, y, m, c, ldx, ldy);
  CS_CHECK_LAUNCH();
  return CS_OK;
}

extern "C" int cs_clip_attn_causal(const float* q, const float* k, const float* v, float* out, int nb, int t, int heads,
                                   int dh, int ldq, int ldk, int ldv, int ldo, float scale, cs_stream_t stream) {
  if (!q || !k || !v || !out || nb < 1 || t < 1 || heads < 1 || dh < 1) return CS_EINVAL;
  if (t > AC_MAX_T || dh > AC_MAX_DH || (dh & 3)) return CS_EINVAL;
  if ((ldq & 3) || (ldk & 3) || (ldv & 3) || (ldo & 3)) return CS_EINVAL;
  if (ldq < heads * dh || ldk < heads * dh || ldv < heads * dh || ldo < heads * dh) return CS_EINVAL;
  if (((uintptr_t)q & 15) || ((uintptr_t)k & 15) || ((uintptr_t)v & 15) || ((uintptr_t)out & 15)) return CS_EINVAL;
  const int64_t grid = (int64_t)nb * heads;
  if (grid > 0x7fffffffLL) return CS_EINVAL;
  const size_t smem = ((size_t)2 * t * (dh + 4) + AC_W * AC_MAX_DH + AC_W * AC_MAX_T) * sizeof(float);
  if (smem > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)clip_attn_causal_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)smem);
    if (e != hipSuccess) return (int)e;
  }
  CS_LAUNCH(clip_attn_causal_kernel, dim3((unsigned)grid), dim3(AC_T), smem, (hipStream_t)stream, q, k, v, out, t, heads, dh,
            ldq, ldk, ldv, ldo, scale);
  CS_CHECK_LAUNCH();
  return CS_OK;
}

extern "C" int cs_clip_pool_eot(const float* x, const int32_t* ids, float* out, int nb, int t, int w, int ldx, int ldo,
                                cs_stream_t stream) {
  if (!x || !ids || !out || nb < 1 || t < 1 || w < 1 || ldx < w || ldo < w) return CS_EINVAL;
  CS_LAUNCH(clip_pool_eot_kernel, dim3((unsigned)nb), dim3(EL_T), 0, (hipStream_t)stream, x, ids, out, t, w, ldx, ldo);
  CS_CHECK_LAUNCH();
  return CS_OK;
}

extern "C" int cs_feature_pair_l2(const float* f, const int32_t* pairs, float* out, int n, int e, int npairs, int ld,
                                  int32_t* err, cs_stream_t stream) {
  if (!f || !pairs || !out || !err || n < 1 || e < 1 || npairs < 1 || ld < e) return CS_EINVAL;
  const int per = EL_T / 64;
  CS_LAUNCH(feature_pair_l2_kernel, dim3((unsigned)((npairs + per - 1) / per)), dim3(EL_T), 0, (hipStream_t)stream, f, pairs,
            out, n, e, npairs, ld, err);
  CS_CHECK_LAUNCH();
  return CS_OK;
}
