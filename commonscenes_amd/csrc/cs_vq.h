// The VQ nearest-code search (quantizer.py:76-84), shared by cs_vq_argmin_lookup (cs_ops.hip) and cs_vq_quantize_st
// (cs_vqenc.hip): one distance expression and one tie rule, so both entries return the same indices bit for bit.
#pragma once
#include "cs_common.h"

// codebook [ncode][edim] -> sm [ncode][4] = e0, e1, e2 | 0, sum(e^2); the whole workgroup stages, the caller syncs
__device__ __forceinline__ void cs_vq_stage_codebook(const float* __restrict__ cb, float* __restrict__ sm, int ncode,
                                                     int edim) {
  for (int i = threadIdx.x; i < ncode; i += blockDim.x) {
    float e[3] = {0.f, 0.f, 0.f};
    float ee = 0.f;
    for (int d = 0; d < edim && d < 3; ++d) e[d] = cb[(int64_t)i * edim + d];
    // torch.sum(w**2, dim=1): sequential fp32 sum over edim entries
    for (int d = 0; d < edim; ++d) {
      const float w = cb[(int64_t)i * edim + d];
      ee += w * w;
    }
    sm[4 * i + 0] = e[0];
    sm[4 * i + 1] = e[1];
    sm[4 * i + 2] = e[2];
    sm[4 * i + 3] = ee;
  }
}

// index of the nearest code to the row zr[0:edim] (the FIRST minimum, as torch.argmin returns); zz receives the row
__device__ __forceinline__ int cs_vq_argmin(const float* __restrict__ zr, const float* __restrict__ sm, int ncode,
                                            int edim, float zz[3]) {
  float z2 = 0.f;
  for (int d = 0; d < edim; ++d) {
    zz[d] = zr[d];
    z2 += zz[d] * zz[d];
  }
  float best = INFINITY;
  int bi = 0;
  for (int i = 0; i < ncode; ++i) {
    const float4 c = *reinterpret_cast<const float4*>(sm + 4 * i);
    // z.e as the K=3 dot product of the reference einsum: ((z0*e0) + z1*e1) + z2*e2 via fma chain
    float dot = zz[0] * c.x;
    dot = fmaf(zz[1], c.y, dot);
    dot = fmaf(zz[2], c.z, dot);
    const float d = (z2 + c.w) - 2.0f * dot;
    if (d < best) {
      best = d;
      bi = i;
    }
  }
  return bi;
}
