// The row routine of the LayerNorm that emits the interleaved F16X3 operand pair (CsConvGemm.a_format = 2; ln_pair_kernel in
// cs_norm.hip, twin_ln_pair_kernel in cs_twin_ln.hip): ONE source, so both kernels run the same arithmetic in the same order
// and give the same bits.
#pragma once
#include "cs_common.h"

typedef _Float16 cs_h4v __attribute__((ext_vector_type(4)));

// One row: the wave's lanes hold the row in v (lane owns float4 chunks lane + 64 k, zeros past the row's end) and
// s = the lane's sum over them; returns the lane's max |scaled output| joined with amax
template <int MAXV>
__device__ __forceinline__ float cs_ln_pair_row(const float4 (&v)[MAXV], float s, int lane, int ch4, int c,
                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                _Float16* __restrict__ yrow, float eps, float a_scale, float amax) {
  const float mean = wave_sum(s) / (float)c;
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
  const float rstd = 1.0f / sqrtf(var + eps);
#pragma unroll
  for (int k = 0; k < MAXV; ++k) {
    const int c4 = lane + 64 * k;
    if (c4 < ch4) {
      const float4 g = *reinterpret_cast<const float4*>(gamma + c4 * 4);
      const float4 b = *reinterpret_cast<const float4*>(beta + c4 * 4);
      // the fp32 LayerNorm's expression, then the operand scale (a power of two: exact)
      const float o[4] = {((v[k].x - mean) * rstd * g.x + b.x) * a_scale, ((v[k].y - mean) * rstd * g.y + b.y) * a_scale,
                          ((v[k].z - mean) * rstd * g.z + b.z) * a_scale, ((v[k].w - mean) * rstd * g.w + b.w) * a_scale};
      cs_h4v hi, lo;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        amax = fmaxf(amax, fabsf(o[e]));
        const _Float16 h = (_Float16)o[e];
        hi[e] = h;
        lo[e] = (_Float16)(o[e] - (float)h);
      }
      // channel 4*c4 + e sits in chunk (4*c4) / 16 at j = (4*c4) % 16: hi at halves (j < 8 ? 0 : 16) + j % 8, lo 8 further
      const int cch = c4 >> 2, j = (c4 & 3) * 4;
      _Float16* dst = yrow + cch * 32 + (j < 8 ? 0 : 16) + (j & 7);
      *reinterpret_cast<cs_h4v*>(dst) = hi;
      *reinterpret_cast<cs_h4v*>(dst + 8) = lo;
    }
  }
  return amax;
}
