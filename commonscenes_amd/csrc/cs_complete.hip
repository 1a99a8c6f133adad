// Shape completion (gfx950): the masked step of the DDIM loop, samplers/ddim.py:158-161
//   img_orig = model.q_sample(x0, ts);  img = img_orig * mask + (1. - mask) * img
// as one launch.  The reference evaluates it as seven ATen ops, each rounding to fp32: two multiplies and an add for q_sample,
// then mul, rsub, mul, add.  Every product and sum below is therefore an explicit _rn intrinsic -- never one fma.
// Bandwidth-trivial (five 48 KB streams per latent row); what matters is the arithmetic and the tails.
// One workgroup owns up to CS_MB_BLOCK_FLOATS voxels of ONE (row, channel) run, so the mask channel, the row maps and the
// 16-byte decision are uniform per workgroup.
#include "cs_common.h"

#define CS_MB_THREADS 256
#define CS_MB_BLOCK_FLOATS 4096      // 256 threads x 4 groups of 4

__device__ __forceinline__ float mb_one(float a, float x, float b, float n, float m, float g) {
  const float q = __fadd_rn(__fmul_rn(a, x), __fmul_rn(b, n));                   // q_sample: three roundings
  return __fadd_rn(__fmul_rn(q, m), __fmul_rn(__fsub_rn(1.f, m), g));           // the blend: four more
}

// `img` and `out` may be the same buffer: no __restrict__ on either, and a thread writes only what it has read itself
__global__ __launch_bounds__(CS_MB_THREADS) void masked_blend_kernel(
    const float* __restrict__ x0, const float* __restrict__ noise, const float* __restrict__ mask, const float* img, float* out,
    const int64_t* __restrict__ t, const float* __restrict__ sa, const float* __restrict__ s1, const int32_t* __restrict__ src,
    const int32_t* __restrict__ msrc, int channels, int64_t inner, int mask_channels, int blocks_per_run, int T,
    int64_t x0_rows, int64_t mask_rows, int bases_aligned) {
  const int64_t run = blockIdx.x / blocks_per_run;               // (row, channel)
  const int64_t e0 = (int64_t)(blockIdx.x % blocks_per_run) * CS_MB_BLOCK_FLOATS;
  const int64_t r = run / channels;
  const int c = (int)(run % channels);
  const int64_t tt = t[r];
  const int64_t xr = src ? (int64_t)src[r] : r;
  const int64_t mr = msrc ? (int64_t)msrc[r] : r;
  // the host wrapper rejects out-of-range indices before the launch; a caller of the C entry that did not gets a row of NaNs,
  // never an out-of-bounds read
  const bool ok = tt >= 0 && tt < T && xr >= 0 && xr < x0_rows && mr >= 0 && mr < mask_rows;
  const float a = ok ? sa[tt] : 0.f, b = ok ? s1[tt] : 0.f;
  const int mc = mask_channels == 1 ? 0 : c;
  const int64_t ox = ((ok ? xr : 0) * channels + c) * inner;     // element offsets of this run in x0 / mask / the row arrays
  const int64_t om = ((ok ? mr : 0) * mask_channels + mc) * inner;
  const int64_t oo = run * inner;
  const float* xp = x0 + ox;
  const float* mp = mask + om;
  const float* np_ = noise + oo;
  const float* gp = img + oo;
  float* op = out + oo;
  const float bad = __builtin_nanf("");
  const bool vec = bases_aligned && ((ox | om | oo) & 3) == 0;   // e0 is a multiple of 4: a group's offset is 4-float aligned
#pragma unroll
  for (int j = 0; j < CS_MB_BLOCK_FLOATS / CS_MB_THREADS / 4; ++j) {
    const int64_t e = e0 + ((int64_t)j * CS_MB_THREADS + threadIdx.x) * 4;
    if (e >= inner) continue;
    if (vec && e + 4 <= inner) {
      const f32x4 xv = *(const f32x4*)(xp + e), nv = *(const f32x4*)(np_ + e), mv = *(const f32x4*)(mp + e),
                  gv = *(const f32x4*)(gp + e);
      f32x4 o;
      o.x = mb_one(a, xv.x, b, nv.x, mv.x, gv.x);
      o.y = mb_one(a, xv.y, b, nv.y, mv.y, gv.y);
      o.z = mb_one(a, xv.z, b, nv.z, mv.z, gv.z);
      o.w = mb_one(a, xv.w, b, nv.w, mv.w, gv.w);
      if (!ok) o.x = o.y = o.z = o.w = bad;
      *(f32x4*)(op + e) = o;
    } else {                                                     // an unaligned run, or the last inner % 4 voxels of a run
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (e + k < inner) {
          const float v = mb_one(a, xp[e + k], b, np_[e + k], mp[e + k], gp[e + k]);
          op[e + k] = ok ? v : bad;
        }
      }
    }
  }
}

extern "C" int cs_ddim_masked_blend(const float* x0, const float* noise, const float* mask, const float* img, float* out,
                                    const int64_t* t, const float* sa, const float* s1, const int32_t* src,
                                    const int32_t* msrc, int64_t rows, int channels, int64_t inner, int mask_channels, int T,
                                    int64_t x0_rows, int64_t mask_rows, hipStream_t stream) {
  if (!x0 || !noise || !mask || !img || !out || !t || !sa || !s1) return CS_EINVAL;
  if (rows <= 0 || channels <= 0 || inner <= 0 || T <= 0 || x0_rows <= 0 || mask_rows <= 0) return CS_EINVAL;
  if (mask_channels != 1 && mask_channels != channels) return CS_EINVAL;
  if ((!src && x0_rows < rows) || (!msrc && mask_rows < rows)) return CS_EINVAL;      // the identity map would leave the tensor
  const int64_t bpr = (inner + CS_MB_BLOCK_FLOATS - 1) / CS_MB_BLOCK_FLOATS;
  if (rows > 0x7fffffffLL / channels || bpr > 0x7fffffffLL / (rows * channels)) return CS_EINVAL;
  const int aligned =
      (((uintptr_t)x0 | (uintptr_t)noise | (uintptr_t)mask | (uintptr_t)img | (uintptr_t)out) & 15) == 0 ? 1 : 0;
  const dim3 grid((unsigned)(bpr * rows * channels)), block(CS_MB_THREADS);
  CS_LAUNCH(masked_blend_kernel, grid, block, 0, stream, x0, noise, mask, img, out, t, sa, s1, src, msrc, channels, inner,
            mask_channels, (int)bpr, T, x0_rows, mask_rows, aligned);
  CS_CHECK_LAUNCH();
  return CS_OK;
}
