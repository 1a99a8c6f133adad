// The VQ-VAE encode side's own kernels (vqvae_networks/network.py:78-88 VQVAE.encode / encode_no_quant).  Everything
// between conv_in and the quantiser -- ResnetBlocks, the stride-2 Downsample convs, the mid attention, norm_out, conv_out,
// quant_conv -- runs on the decoder's GEMM / GroupNorm / attention kernels (commonscenes_amd/vqvae.py::encoder_ndhwc);
// what is here are the two edges those kernels do not fit:
//   cs_vqenc_conv_in   Encoder3D.conv_in (vqvae_modules.py:201-205): Conv3d(1 -> cout, 3x3x3, pad 1) on the raw SDF.
//                      One input channel: the implicit GEMM would pad K from 27 to 27 x 16 and still need a layout pass;
//                      here the 27 taps are fp32 FMAs on the VALU and the kernel is bound by its output write.
//   cs_vq_quantize_st  VectorQuantizer.forward (quantizer.py:68-119, legacy=False): nearest code (cs_vq_argmin, the
//                      search cs_vq_argmin_lookup runs), the straight-through value z + (z_q - z), and per-object fp64
//                      sums of (z_q - z)^2 for the embedding loss -- fixed order, no float atomics.
#include "cs_common.h"
#include "cs_vq.h"

namespace {

// One thread per (voxel, 4 output channels): 16 lanes of a 64-channel voxel read the same 27 input words (broadcast,
// L1-resident) and together write its 256-byte row, so every wave stores 1 KB of contiguous output.  Weights are
// staged in LDS as [27][cout] (float4 per lane and tap) with the bias behind them.  Per output channel:
// acc = sum over taps in (kd, kh, kw) order of x * w as an fma chain, then + bias.
__global__ __launch_bounds__(256) void vqenc_conv_in_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                            const float* __restrict__ b, float* __restrict__ out,
                                                            int nb, int d, int h, int wd, int cout, int ldo) {
  extern __shared__ __attribute__((aligned(16))) float sw[];     // [27][cout] weights, then [cout] bias
  for (int i = threadIdx.x; i < 27 * cout; i += blockDim.x) {
    const int t = i / cout, o = i - t * cout;
    sw[i] = w[o * 27 + t];
  }
  for (int i = threadIdx.x; i < cout; i += blockDim.x) sw[27 * cout + i] = b ? b[i] : 0.f;
  __syncthreads();
  const int q4 = cout >> 2;
  const int64_t vol = (int64_t)d * h * wd;
  const int64_t total = (int64_t)nb * vol * q4;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int q = (int)(i % q4);
    const int64_t v = i / q4;
    const int64_t n = v / vol;
    int r = (int)(v - n * vol);
    const int ow = r % wd;
    r /= wd;
    const int oh = r % h;
    const int od = r / h;
    const float* xb = x + n * vol;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    int t = 0;
#pragma unroll
    for (int kd = 0; kd < 3; ++kd) {
      const int id = od + kd - 1;
#pragma unroll
      for (int kh = 0; kh < 3; ++kh) {
        const int ih = oh + kh - 1;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw, ++t) {
          const int iw = ow + kw - 1;
          const bool ok = (unsigned)id < (unsigned)d && (unsigned)ih < (unsigned)h && (unsigned)iw < (unsigned)wd;
          const float xv = ok ? xb[((int64_t)id * h + ih) * wd + iw] : 0.f;
          const float4 wv = *reinterpret_cast<const float4*>(sw + t * cout + 4 * q);
          acc.x = fmaf(xv, wv.x, acc.x);
          acc.y = fmaf(xv, wv.y, acc.y);
          acc.z = fmaf(xv, wv.z, acc.z);
          acc.w = fmaf(xv, wv.w, acc.w);
        }
      }
    }
    const float4 bv = *reinterpret_cast<const float4*>(sw + 27 * cout + 4 * q);
    acc.x += bv.x;
    acc.y += bv.y;
    acc.z += bv.z;
    acc.w += bv.w;
    *reinterpret_cast<float4*>(out + v * ldo + 4 * q) = acc;
  }
}

// grid (row tiles of CS_VQ_ST_ROWS, objects): one row per lane.  Each workgroup leaves the fp64 sum of its rows'
// (z_q - z)^2 in part[n][tile] (lane sums, then a fixed LDS tree); vq_st_sum_kernel adds an object's tiles in order.
__global__ __launch_bounds__(CS_VQ_ST_ROWS) void vq_st_kernel(const float* __restrict__ z, const float* __restrict__ cb,
                                                              int64_t* __restrict__ idx, float* __restrict__ zst,
                                                              double* __restrict__ part, int64_t rows, int ncode,
                                                              int edim, int ldz, int ldq) {
  extern __shared__ __attribute__((aligned(16))) float sm[];     // [ncode][4] : e0,e1,e2|0,ee
  __shared__ double red[CS_VQ_ST_ROWS];
  cs_vq_stage_codebook(cb, sm, ncode, edim);
  __syncthreads();
  const int64_t n = blockIdx.y;
  const int64_t rl = (int64_t)blockIdx.x * CS_VQ_ST_ROWS + threadIdx.x;
  double s = 0.0;
  if (rl < rows) {
    const int64_t r = n * rows + rl;
    float zz[3] = {0.f, 0.f, 0.f};
    const int bi = cs_vq_argmin(z + r * ldz, sm, ncode, edim, zz);
    idx[r] = bi;
    for (int e = 0; e < edim; ++e) {
      const float q = cb[(int64_t)bi * edim + e];
      const float df = q - zz[e];                 // (z_q - z) in fp32, as torch forms it
      zst[r * ldq + e] = zz[e] + df;              // quantizer.py:96-97: z + (z_q - z).detach()
      s += (double)df * (double)df;
    }
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = CS_VQ_ST_ROWS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[n * gridDim.x + blockIdx.x] = red[0];
}

__global__ __launch_bounds__(64) void vq_st_sum_kernel(const double* __restrict__ part, double* __restrict__ loss,
                                                       int nb, int tiles) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= nb) return;
  double s = 0.0;
  for (int t = 0; t < tiles; ++t) s += part[(int64_t)n * tiles + t];
  loss[n] = s;
}

}  // namespace

extern "C" int cs_vqenc_conv_in(const float* x, const float* w, const float* bias, float* out, int nb, int d, int h,
                                int wd, int cout, int ldo, cs_stream_t stream) {
  if (!x || !w || !out || nb <= 0 || d <= 0 || h <= 0 || wd <= 0 || cout <= 0 || (cout & 3) || cout > 256 ||
      ldo < cout || (ldo & 3) || ((uintptr_t)out & 15))
    return CS_EINVAL;
  const int64_t total = (int64_t)nb * d * h * wd * (cout / 4);
  const size_t smem = (size_t)28 * cout * sizeof(float);     // <= 28 KB
  CS_LAUNCH(vqenc_conv_in_kernel, dim3(cs_grid_for(total, 256, 256 * 64)), dim3(256), smem, (hipStream_t)stream, x,
            w, bias, out, nb, d, h, wd, cout, ldo);
  CS_CHECK_LAUNCH();
  return CS_OK;
}

extern "C" int cs_vq_quantize_st(const float* z, const float* codebook, int64_t* idx, float* zst, double* part,
                                 double* loss, int64_t rows, int nb, int ncode, int edim, int ldz, int ldq,
                                 cs_stream_t stream) {
  if (!z || !codebook || !idx || !zst || !part || !loss || rows <= 0 || nb <= 0 || ncode <= 0 || edim <= 0 ||
      edim > 3 || ldz < edim || ldq < edim)
    return CS_EINVAL;
  const int64_t tiles = (rows + CS_VQ_ST_ROWS - 1) / CS_VQ_ST_ROWS;
  if (tiles > 0x7fffffffLL || nb > 65535) return CS_EINVAL;
  const size_t smem = (size_t)ncode * 4 * sizeof(float);
  if (smem + CS_VQ_ST_ROWS * sizeof(double) > 160 * 1024) return CS_EINVAL;
  if (smem > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)vq_st_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)smem);
    if (e != hipSuccess) return (int)e;
  }
  CS_LAUNCH(vq_st_kernel, dim3((unsigned)tiles, nb), dim3(CS_VQ_ST_ROWS), smem, (hipStream_t)stream, z, codebook, idx,
            zst, part, rows, ncode, edim, ldz, ldq);
  CS_CHECK_LAUNCH();
  CS_LAUNCH(vq_st_sum_kernel, dim3((nb + 63) / 64), dim3(64), 0, (hipStream_t)stream, part, loss, nb, (int)tiles);
  CS_CHECK_LAUNCH();
  return CS_OK;
}
