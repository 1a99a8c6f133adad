// What InceptionV3's pool3 features (commonscenes_amd/inception.py: the FID / KID extractor of
// scripts/compute_fid_scores_3dfront.py) need beside cs_conv_gemm:
//   * cs_incep_input        uint8 / float HWC image -> normalised fp32 [nb][299][299][cpad], bilinear resize on the way
//   * cs_pool2d_max3        3 x 3 max pool, stride 1 / 2, pad 0 / 1
//   * cs_pool2d_avg3        3 x 3 average, stride 1, pad 1, with or without the padding in the divisor
//   * cs_pool2d_global_avg  mean over H x W, fp64 accumulation
// NHWC fp32, rows are pixels with a leading dimension, so operands may be channel slices of wider buffers.  Every kernel is one
// pass over its input with no atomics and a fixed order of operations per output element: a sample's bits do not depend on its
// place in the batch.  The pools come in two instantiations, V = 4 (float4 along C: c, ldx, ldo and both pointers multiples of
// 4 floats) and V = 1 (anything else); a lane's arithmetic per channel is the same in both.
// The two normalisations -- 2 * (v / 255) - 1 (pytorch-fid; cleanfid's "legacy_pytorch") and (v - 128) / 128 (cleanfid's
// "clean" wrapper) -- are restated from those packages' published sources: neither is part of the build image.
#include "cs_common.h"

namespace {

constexpr int IN_T = 256;
constexpr int OUT_S = CS_INCEP_SIZE;

template <int V>
struct Vec;
template <>
struct Vec<1> {
  float v[1];
  __device__ __forceinline__ void load(const float* p) { v[0] = *p; }
  __device__ __forceinline__ void store(float* p) const { *p = v[0]; }
};
template <>
struct Vec<4> {
  float v[4];
  __device__ __forceinline__ void load(const float* p) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  }
  __device__ __forceinline__ void store(float* p) const { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
};

// ---- front end --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float incep_norm(float v, int norm) {
  return norm == 0 ? 2.0f * (v / 255.0f) - 1.0f : (v - 128.0f) / 128.0f;
}

// F.interpolate(bilinear, align_corners=False) along one axis: src = (dst + 0.5) * in / out - 0.5 = n / (2 out) with
// n = (2 dst + 1) in - out, clamped below at 0.  Kept as the exact rational: i0 = n div 2 out, and the weights of i0 / i1 are
// (2 out - r) / 2 out and r / 2 out with r = n mod 2 out.  (src itself reaches 600 for a 300 x 600 image: rounded to fp32 its
// fraction would be off by 3e-5, a hundred times the tolerance of the blend.)
__device__ __forceinline__ void incep_axis(int dst, int in, int& i0, int& i1, int& r) {
  constexpr int D = 2 * OUT_S;
  int64_t n = (int64_t)(2 * dst + 1) * in - OUT_S;
  if (n < 0) n = 0;
  i0 = (int)(n / D);
  r = (int)(n - (int64_t)i0 * D);
  i1 = i0 + 1 < in ? i0 + 1 : in - 1;
}

// one thread per output pixel.  The four weights times the 0..255 samples are integers below 255 * 598^2 < 2^27: the blend's
// numerator is exact, one division rounds it to fp32, the normalisation adds its own two roundings.
__global__ __launch_bounds__(IN_T) void incep_input_u8_kernel(const uint8_t* __restrict__ img, float* __restrict__ out,
                                                              int64_t npix, int h, int w, int resize, int norm, int cpad,
                                                              int vec) {
  constexpr int D = 2 * OUT_S;
  for (int64_t i = blockIdx.x * (int64_t)IN_T + threadIdx.x; i < npix; i += (int64_t)gridDim.x * IN_T) {
    const int ox = (int)(i % OUT_S), oy = (int)((i / OUT_S) % OUT_S);
    const int64_t b = i / ((int64_t)OUT_S * OUT_S);
    const uint8_t* src = img + b * (int64_t)h * w * 3;
    float val[3];
    if (resize) {
      int y0, y1, ry, x0, x1, rx;
      incep_axis(oy, h, y0, y1, ry);
      incep_axis(ox, w, x0, x1, rx);
      const uint8_t* p00 = src + ((int64_t)y0 * w + x0) * 3;
      const uint8_t* p01 = src + ((int64_t)y0 * w + x1) * 3;
      const uint8_t* p10 = src + ((int64_t)y1 * w + x0) * 3;
      const uint8_t* p11 = src + ((int64_t)y1 * w + x1) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int top = (D - rx) * (int)p00[c] + rx * (int)p01[c];
        const int bot = (D - rx) * (int)p10[c] + rx * (int)p11[c];
        const int num = (D - ry) * top + ry * bot;
        val[c] = (float)((double)num / (double)(D * D));
      }
    } else {
      const uint8_t* p = src + ((int64_t)oy * w + ox) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) val[c] = (float)p[c];
    }
    float* row = out + i * cpad;
    if (vec) {
      *reinterpret_cast<float4*>(row) = make_float4(incep_norm(val[0], norm), incep_norm(val[1], norm), incep_norm(val[2], norm), 0.f);
      for (int c = 4; c < cpad; c += 4) *reinterpret_cast<float4*>(row + c) = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) row[c] = incep_norm(val[c], norm);
      for (int c = 3; c < cpad; ++c) row[c] = 0.f;
    }
  }
}

__global__ __launch_bounds__(IN_T) void incep_input_f32_kernel(const float* __restrict__ img, float* __restrict__ out,
                                                               int64_t npix, int norm, int cpad, int vec) {
  for (int64_t i = blockIdx.x * (int64_t)IN_T + threadIdx.x; i < npix; i += (int64_t)gridDim.x * IN_T) {
    const float* p = img + i * 3;
    float* row = out + i * cpad;
    const float a = incep_norm(p[0], norm), b = incep_norm(p[1], norm), c2 = incep_norm(p[2], norm);
    if (vec) {
      *reinterpret_cast<float4*>(row) = make_float4(a, b, c2, 0.f);
      for (int c = 4; c < cpad; c += 4) *reinterpret_cast<float4*>(row + c) = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      row[0] = a, row[1] = b, row[2] = c2;
      for (int c = 3; c < cpad; ++c) row[c] = 0.f;
    }
  }
}

// ---- 3 x 3 pools ------------------------------------------------------------------------------------------------------------
// one thread per (output pixel, V channels), channels fastest: a wave reads 64 V consecutive floats of each tap's row
template <int V, bool AVG>
__global__ __launch_bounds__(IN_T) void pool3_kernel(const float* __restrict__ x, float* __restrict__ out, int64_t n, int h, int w,
                                                     int ho, int wo, int cv, int ldx, int ldo, int stride, int pad,
                                                     int include_pad) {
  for (int64_t i = blockIdx.x * (int64_t)IN_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * IN_T) {
    const int c = (int)(i % cv) * V;
    const int64_t pix = i / cv;                       // (b * ho + oy) * wo + ox
    const int ox = (int)(pix % wo), oy = (int)((pix / wo) % ho);
    const int64_t b = pix / ((int64_t)wo * ho);
    const float* xb = x + b * (int64_t)h * w * ldx + c;
    Vec<V> acc;
    int taps = 0;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const int y = oy * stride - pad + kh;
      if (y < 0 || y >= h) continue;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int xx = ox * stride - pad + kw;
        if (xx < 0 || xx >= w) continue;
        Vec<V> t;
        t.load(xb + ((int64_t)y * w + xx) * ldx);
        if (taps == 0) {
          acc = t;
        } else {
#pragma unroll
          for (int e = 0; e < V; ++e) {
            if (AVG) acc.v[e] += t.v[e];
            else acc.v[e] = (t.v[e] > acc.v[e] || t.v[e] != t.v[e]) ? t.v[e] : acc.v[e];      // NaN wins, as in torch
          }
        }
        ++taps;
      }
    }
    if (AVG) {
      const float div = include_pad ? 9.0f : (float)taps;
#pragma unroll
      for (int e = 0; e < V; ++e) acc.v[e] = acc.v[e] / div;
    }
    acc.store(out + pix * ldo + c);
  }
}

// one thread per (sample, V channels): the h * w pixels in index order into fp64, one rounding at the end
template <int V>
__global__ __launch_bounds__(IN_T) void global_avg_kernel(const float* __restrict__ x, float* __restrict__ out, int64_t n, int hw,
                                                          int cv, int ldx, int ldo) {
  for (int64_t i = blockIdx.x * (int64_t)IN_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * IN_T) {
    const int c = (int)(i % cv) * V;
    const int64_t b = i / cv;
    const float* xb = x + b * (int64_t)hw * ldx + c;
    double acc[V];
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = 0.0;
    for (int p = 0; p < hw; ++p) {
      Vec<V> t;
      t.load(xb + (int64_t)p * ldx);
#pragma unroll
      for (int e = 0; e < V; ++e) acc[e] += (double)t.v[e];
    }
    Vec<V> r;
#pragma unroll
    for (int e = 0; e < V; ++e) r.v[e] = (float)(acc[e] / (double)hw);
    r.store(out + b * ldo + c);
  }
}

inline bool al(const void* p, int bytes) { return ((uintptr_t)p & (uintptr_t)(bytes - 1)) == 0; }

// the float4 path: c, both leading dimensions and both pointers are whole float4s
inline bool vec4_ok(const float* x, const float* out, int c, int ldx, int ldo) {
  return !(c & 3) && !(ldx & 3) && !(ldo & 3) && al(x, 16) && al(out, 16);
}

// every refusal the three pools share; the row counts must fit int32 (what cs_conv_gemm, their neighbour, indexes with)
inline bool pool_args_ok(const float* x, const float* out, int nb, int h, int w, int c, int ldx, int ldo, int64_t ho,
                         int64_t wo) {
  if (!x || !out || !al(x, 4) || !al(out, 4)) return false;
  if (nb < 1 || h < 1 || w < 1 || c < 1 || ldx < c || ldo < c || ho < 1 || wo < 1) return false;
  return (int64_t)nb * h * w <= 0x7fffffffLL && (int64_t)nb * ho * wo <= 0x7fffffffLL;
}

template <bool AVG>
int launch_pool3(const float* x, float* out, int nb, int h, int w, int c, int ldx, int ldo, int stride, int pad, int include_pad,
                 hipStream_t s) {
  const int ho = (h + 2 * pad - 3) / stride + 1, wo = (w + 2 * pad - 3) / stride + 1;
  const bool vec = vec4_ok(x, out, c, ldx, ldo);
  const int cv = vec ? c >> 2 : c;
  const int64_t n = (int64_t)nb * ho * wo * cv;
  if (vec)
    CS_LAUNCH((pool3_kernel<4, AVG>), dim3(cs_grid_for(n, IN_T)), dim3(IN_T), 0, s, x, out, n, h, w, ho, wo, cv, ldx, ldo, stride,
              pad, include_pad);
  else
    CS_LAUNCH((pool3_kernel<1, AVG>), dim3(cs_grid_for(n, IN_T)), dim3(IN_T), 0, s, x, out, n, h, w, ho, wo, cv, ldx, ldo, stride,
              pad, include_pad);
  CS_CHECK_LAUNCH();
  return CS_OK;
}

}  // namespace

extern "C" int cs_incep_input(const void* img, int is_float, int nb, int h, int w, int resize, int norm, float* out, int cpad,
                              cs_stream_t stream) {
  if (!img || !out || !al(out, 4) || nb < 1 || h < 1 || w < 1 || cpad < 3) return CS_EINVAL;
  if ((is_float != 0 && is_float != 1) || (resize != 0 && resize != 1) || (norm != 0 && norm != 1)) return CS_EINVAL;
  if (is_float && (resize || !al(img, 4))) return CS_EINVAL;
  if (!resize && (h != OUT_S || w != OUT_S)) return CS_EINVAL;
  const int64_t npix = (int64_t)nb * OUT_S * OUT_S;
  if (npix > 0x7fffffffLL || (int64_t)nb * h * w > 0x7fffffffLL) return CS_EINVAL;
  const int vec = !(cpad & 3) && al(out, 16);
  hipStream_t s = (hipStream_t)stream;
  if (is_float)
    CS_LAUNCH(incep_input_f32_kernel, dim3(cs_grid_for(npix, IN_T)), dim3(IN_T), 0, s, reinterpret_cast<const float*>(img), out,
              npix, norm, cpad, vec);
  else
    CS_LAUNCH(incep_input_u8_kernel, dim3(cs_grid_for(npix, IN_T)), dim3(IN_T), 0, s, reinterpret_cast<const uint8_t*>(img), out,
              npix, h, w, resize, norm, cpad, vec);
  CS_CHECK_LAUNCH();
  return CS_OK;
}

extern "C" int cs_pool2d_max3(const float* x, float* out, int nb, int h, int w, int c, int ldx, int ldo, int stride, int pad,
                              cs_stream_t stream) {
  if ((stride != 1 && stride != 2) || (pad != 0 && pad != 1)) return CS_EINVAL;
  if (h + 2 * pad < 3 || w + 2 * pad < 3) return CS_EINVAL;                 // an output extent below 1
  if (!pool_args_ok(x, out, nb, h, w, c, ldx, ldo, (h + 2 * pad - 3) / stride + 1, (w + 2 * pad - 3) / stride + 1))
    return CS_EINVAL;
  return launch_pool3<false>(x, out, nb, h, w, c, ldx, ldo, stride, pad, 0, (hipStream_t)stream);
}

extern "C" int cs_pool2d_avg3(const float* x, float* out, int nb, int h, int w, int c, int ldx, int ldo, int count_include_pad,
                              cs_stream_t stream) {
  if (count_include_pad != 0 && count_include_pad != 1) return CS_EINVAL;
  if (!pool_args_ok(x, out, nb, h, w, c, ldx, ldo, h, w)) return CS_EINVAL;
  return launch_pool3<true>(x, out, nb, h, w, c, ldx, ldo, 1, 1, count_include_pad, (hipStream_t)stream);
}

extern "C" int cs_pool2d_global_avg(const float* x, float* out, int nb, int h, int w, int c, int ldx, int ldo,
                                    cs_stream_t stream) {
  if (!pool_args_ok(x, out, nb, h, w, c, ldx, ldo, 1, 1)) return CS_EINVAL;
  const bool vec = vec4_ok(x, out, c, ldx, ldo);
  const int cv = vec ? c >> 2 : c;
  const int64_t n = (int64_t)nb * cv;
  hipStream_t s = (hipStream_t)stream;
  if (vec)
    CS_LAUNCH(global_avg_kernel<4>, dim3(cs_grid_for(n, IN_T)), dim3(IN_T), 0, s, x, out, n, h * w, cv, ldx, ldo);
  else
    CS_LAUNCH(global_avg_kernel<1>, dim3(cs_grid_for(n, IN_T)), dim3(IN_T), 0, s, x, out, n, h * w, cv, ldx, ldo);
  CS_CHECK_LAUNCH();
  return CS_OK;
}
