// What the norm kernels that emit an F16X3 operand share (cs_norm.hip, cs_twin_ln.hip): the fp32 -> fp16 hi / lo split with its
// overflow flag, and the LayerNorm row routines -- load, statistics, and the row of the interleaved pair (CsConvGemm.a_format =
// 2; ln_pair_kernel in cs_norm.hip, twin_ln_pair_kernel in cs_twin_ln.hip).  ONE source each, so every kernel runs the same
// arithmetic in the same order and gives the same bits.
#pragma once
#include "cs_common.h"

template <int V>
using cs_hv = _Float16 __attribute__((ext_vector_type(V)));

// fp16 hi / lo of o[0 .. V) (already at operand scale); amax = the thread's running max |o|
template <int V>
__device__ __forceinline__ void cs_pair_split(const float (&o)[V], cs_hv<V>& hi, cs_hv<V>& lo, float& amax) {
#pragma unroll
  for (int k = 0; k < V; ++k) {
    amax = fmaxf(amax, fabsf(o[k]));
    const _Float16 h = (_Float16)o[k];
    hi[k] = h;
    lo[k] = (_Float16)(o[k] - (float)h);
  }
}

// a value at or past the largest finite fp16 went into a pair: tell the status word
__device__ __forceinline__ void cs_pair_amax_flag(int32_t* __restrict__ status, float amax) {
  if (status && amax >= 65504.f) atomicOr(status, CS_STATUS_F16X3_OVERFLOW);
}

// One wave per row; each lane owns up to MAXV float4 chunks (c <= 64*4*MAXV): chunks lane + 64 k of row `row` of x into v,
// zeros past the row's end; returns the lane's sum over them
template <int MAXV>
__device__ __forceinline__ float cs_ln_load_row(const float* __restrict__ x, int64_t row, int ldx, int lane, int ch4, float4 (&v)[MAXV]) {
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < MAXV; ++k) {
    const int c4 = lane + 64 * k;
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c4 < ch4) t = *reinterpret_cast<const float4*>(x + row * ldx + c4 * 4);
    s += (t.x + t.y) + (t.z + t.w);
    v[k] = t;
  }
  return s;
}

// (mean, 1 / std) of the row a wave holds in v (s = the lane's sum): two passes in fp32
template <int MAXV>
__device__ __forceinline__ void cs_ln_row_stats(const float4 (&v)[MAXV], float s, int lane, int ch4, int c, float eps,
                                                float& mean, float& rstd) {
  mean = wave_sum(s) / (float)c;
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < MAXV; ++k) {
    const int c4 = lane + 64 * k;
    if (c4 < ch4) {
      const float a = v[k].x - mean, b = v[k].y - mean, cc = v[k].z - mean, d = v[k].w - mean;
      q += (a * a + b * b) + (cc * cc + d * d);
    }
  }
  const float var = wave_sum(q) / (float)c;
  rstd = 1.0f / sqrtf(var + eps);
}

// One row: the wave's lanes hold the row in v (cs_ln_load_row's layout) and s = the lane's sum over them; returns the lane's
// max |scaled output| joined with amax
template <int MAXV>
__device__ __forceinline__ float cs_ln_pair_row(const float4 (&v)[MAXV], float s, int lane, int ch4, int c,
                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                _Float16* __restrict__ yrow, float eps, float a_scale, float amax) {
  float mean, rstd;
  cs_ln_row_stats<MAXV>(v, s, lane, ch4, c, eps, mean, rstd);
#pragma unroll
  for (int k = 0; k < MAXV; ++k) {
    const int c4 = lane + 64 * k;
    if (c4 < ch4) {
      const float4 g = *reinterpret_cast<const float4*>(gamma + c4 * 4);
      const float4 b = *reinterpret_cast<const float4*>(beta + c4 * 4);
      // the fp32 LayerNorm's expression, then the operand scale (a power of two: exact)
      const float o[4] = {((v[k].x - mean) * rstd * g.x + b.x) * a_scale, ((v[k].y - mean) * rstd * g.y + b.y) * a_scale,
                          ((v[k].z - mean) * rstd * g.z + b.z) * a_scale, ((v[k].w - mean) * rstd * g.w + b.w) * a_scale};
      cs_hv<4> hi, lo;
      cs_pair_split<4>(o, hi, lo, amax);
      // channel 4*c4 + e sits in chunk (4*c4) / 16 at j = (4*c4) % 16: hi at halves (j < 8 ? 0 : 16) + j % 8, lo 8 further
      const int cch = c4 >> 2, j = (c4 & 3) * 4;
      _Float16* dst = yrow + cch * 32 + (j < 8 ? 0 : 16) + (j & 7);
      *reinterpret_cast<cs_hv<4>*>(dst) = hi;
      *reinterpret_cast<cs_hv<4>*>(dst + 8) = lo;
    }
  }
  return amax;
}

// The MAXV instantiation of a LayerNorm row kernel for rows of ch4 float4 chunks; CS_EINVAL (returned from the calling entry)
// past 64 * 8 chunks
#define CS_LN_LAUNCH(kernel, ch4, ...)                                  \
  do {                                                                  \
    if ((ch4) <= 64 * 2) CS_LAUNCH(kernel<2>, __VA_ARGS__);             \
    else if ((ch4) <= 64 * 4) CS_LAUNCH(kernel<4>, __VA_ARGS__);        \
    else if ((ch4) <= 64 * 8) CS_LAUNCH(kernel<8>, __VA_ARGS__);        \
    else return CS_EINVAL;                                              \
  } while (0)
