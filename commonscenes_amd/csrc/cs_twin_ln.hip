// cs_twin_layernorm_pair16: the LayerNorm hand-over of the late guidance split (cs_unet.hip::attn_block, twin).
#include "cs_common.h"
#include "cs_ln_pair.h"

namespace {

// The guidance hand-over of the first context-dependent transformer block (cs_unet.hip::attn_block, twin): y = the
// attn1.to_out product + bias and res = its t0 residual are the same for both guidance halves (m rows each); the halves
// differ in the cross-attention row vector.  For replica g in {0, 1} and row r < m:
//   v = (y[r] + rowvec[(g m + r) / rv_rows]) + res[r]      -- the GEMM epilogue's add order (+= rowvec, then += res)
//   t1[g m + r] = v;   pair[g m + r] = ln_pair_kernel's LayerNorm of v
// One wave per row: y and res are read once, both replicas are written.
template <int MAXV>
__global__ __launch_bounds__(256) void twin_ln_pair_kernel(const float* __restrict__ y, const float* __restrict__ rowvec,
                                                           const float* __restrict__ res, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float* __restrict__ t1,
                                                           _Float16* __restrict__ pair, int m, int c, int ldy, int ldrv,
                                                           int rv_rows, int ldr, int ldt, int ldp, float eps, float a_scale,
                                                           int32_t* __restrict__ status) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int ch4 = c >> 2;
  float amax = 0.f;
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < m; row += (int64_t)gridDim.x * 4) {
    float4 a[MAXV], r[MAXV];
#pragma unroll
    for (int k = 0; k < MAXV; ++k) {
      const int c4 = lane + 64 * k;
      a[k] = r[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c4 < ch4) {
        a[k] = *reinterpret_cast<const float4*>(y + row * ldy + c4 * 4);
        r[k] = *reinterpret_cast<const float4*>(res + row * ldr + c4 * 4);
      }
    }
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const int64_t orow = (int64_t)g * m + row;
      const float* rv = rowvec + orow / rv_rows * ldrv;
      float4 v[MAXV];
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < MAXV; ++k) {
        const int c4 = lane + 64 * k;
        v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c4 < ch4) {
          const float4 w = *reinterpret_cast<const float4*>(rv + c4 * 4);
          v[k].x = (a[k].x + w.x) + r[k].x;
          v[k].y = (a[k].y + w.y) + r[k].y;
          v[k].z = (a[k].z + w.z) + r[k].z;
          v[k].w = (a[k].w + w.w) + r[k].w;
          *reinterpret_cast<float4*>(t1 + orow * ldt + c4 * 4) = v[k];
        }
        s += (v[k].x + v[k].y) + (v[k].z + v[k].w);
      }
      amax = cs_ln_pair_row<MAXV>(v, s, lane, ch4, c, gamma, beta, pair + orow * (int64_t)ldp * 2, eps, a_scale, amax);
    }
  }
  cs_pair_amax_flag(status, amax);
}

}  // namespace

// LayerNorm hand-over shared by two guidance halves (see twin_ln_pair_kernel): for g in {0, 1}, r < m
//   t1[g m + r] = (y[r] + rowvec[(g m + r) / rv_rows]) + res[r],   pair[g m + r] = cs_layernorm_pair16 of that row.
// y [m][ldy], res [m][ldr], rowvec [ceil(2 m / rv_rows)][ldrv], t1 [2m][ldt] fp32; pair: the bytes of an fp32 [2m][ldp]
// tensor; c, ldp multiples of 16, the other strides multiples of 4; every pointer 16-byte aligned.
extern "C" int cs_twin_layernorm_pair16(const float* y, const float* rowvec, const float* res, const float* gamma,
                                        const float* beta, float* t1, void* pair, int m, int c, int ldy, int ldrv, int rv_rows,
                                        int ldr, int ldt, int ldp, float eps, float a_scale, int32_t* status,
                                        cs_stream_t stream) {
  if (!y || !rowvec || !res || !gamma || !beta || !t1 || !pair || m <= 0 || c <= 0 || rv_rows <= 0 || !(a_scale > 0.f))
    return CS_EINVAL;
  if ((c & 15) || (ldy & 3) || (ldrv & 3) || (ldr & 3) || (ldt & 3) || (ldp & 15) || ldy < c || ldrv < c || ldr < c || ldt < c ||
      ldp < c)
    return CS_EINVAL;
  if (((uintptr_t)y & 15) || ((uintptr_t)rowvec & 15) || ((uintptr_t)res & 15) || ((uintptr_t)gamma & 15) ||
      ((uintptr_t)beta & 15) || ((uintptr_t)t1 & 15) || ((uintptr_t)pair & 15))
    return CS_EINVAL;
  const int grid = cs_grid_for(((int64_t)m + 3) / 4, 1, 256 * 32);
  CS_LN_LAUNCH(twin_ln_pair_kernel, c >> 2, dim3(grid), dim3(256), 0, (hipStream_t)stream, y, rowvec, res, gamma, beta, t1,
               (_Float16*)pair, m, c, ldy, ldrv, rv_rows, ldr, ldt, ldp, eps, a_scale, status);
  CS_CHECK_LAUNCH();
  return CS_OK;
}
