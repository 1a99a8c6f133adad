// Resampling and normalisation of a ragged set of vertex clouds: the device half of the diversity block of
// scripts/eval_3dfront.py (:592 sample_points -> helpers/util.py:31-44, :643 normalize -> :783-796) and of
// scripts/consistency_check.py:68-77.
//   * cs_cloud_resample   out[i][e] = cloud_i[idx[i][e]], optionally normalised per axis as `normalize` does
// One workgroup per cloud.  Pass 1 gathers the p rows and reduces the per-axis minimum and maximum (order-free: the result
// does not depend on the launch); pass 2 gathers again and writes.  Rows are 12 bytes and a cloud starts at an arbitrary
// row of the packed buffer, so every access is a 4-byte one.
#include "cs_common.h"

namespace {

constexpr int RS_T = 256;

__device__ __forceinline__ float wave_fmin(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}

__global__ __launch_bounds__(RS_T) void cloud_resample_kernel(const float* __restrict__ verts,
                                                              const int64_t* __restrict__ first,
                                                              const int32_t* __restrict__ count,
                                                              const int32_t* __restrict__ idx, float* __restrict__ out, int p,
                                                              int normalize, int32_t* __restrict__ err) {
  __shared__ float red[6][RS_T / 64];
  const int i = blockIdx.x, tid = threadIdx.x;
  const float* cloud = verts + 3 * first[i];
  const int cnt = count[i];
  const int32_t* mine = idx ? idx + (int64_t)i * p : nullptr;
  float* dst = out + (int64_t)i * p * 3;
  float shift[3] = {0.f, 0.f, 0.f}, top[3] = {1.f, 1.f, 1.f};
  if (normalize) {
    float lo[3], hi[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) lo[a] = __builtin_inff(), hi[a] = -__builtin_inff();
    for (int e = tid; e < p; e += RS_T) {
      const int row = mine ? mine[e] : e;
      if (row < 0 || row >= cnt) continue;              // compared BEFORE anything is read through it
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float v = cloud[3 * (int64_t)row + a];
        lo[a] = fminf(lo[a], v), hi[a] = fmaxf(hi[a], v);
      }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      lo[a] = wave_fmin(lo[a]), hi[a] = wave_max(hi[a]);
      if ((tid & 63) == 0) red[a][tid >> 6] = lo[a], red[3 + a][tid >> 6] = hi[a];
    }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      float l = red[a][0], h = red[3 + a][0];
#pragma unroll
      for (int w = 1; w < RS_T / 64; ++w) l = fminf(l, red[a][w]), h = fmaxf(h, red[3 + a][w]);
      // vertices[:, a] += -min - (max - min) * 0.5;  scalars = max(vertices): adding a constant is monotone, so the
      // maximum of the shifted column is the shifted maximum
      shift[a] = (-l) - ((h - l) * 0.5f);
      top[a] = h + shift[a];
    }
  }
  bool bad = false;
  for (int e = tid; e < p; e += RS_T) {
    const int row = mine ? mine[e] : e;
    float v[3];
    if (row < 0 || row >= cnt) {
      bad = true;
      v[0] = v[1] = v[2] = __builtin_nanf("");
    } else {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        v[a] = cloud[3 * (int64_t)row + a];
        if (normalize) v[a] = (v[a] + shift[a]) / top[a];        // IEEE division; a zero extent gives 0 / 0 = NaN
      }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) dst[3 * (int64_t)e + a] = v[a];
  }
  if (bad) atomicOr(err, 1);
}

}  // namespace

extern "C" int cs_cloud_resample(const float* verts, const int64_t* first, const int32_t* count, const int32_t* idx,
                                 float* out, int n, int p, int normalize, int32_t* err, cs_stream_t stream) {
  if (!verts || !first || !count || !out || !err || n < 0 || p < 1) return CS_EINVAL;
  if (n == 0) return CS_OK;
  CS_LAUNCH(cloud_resample_kernel, dim3(n), dim3(RS_T), 0, (hipStream_t)stream, verts, first, count, idx, out, p,
            normalize ? 1 : 0, err);
  CS_CHECK_LAUNCH();
  return CS_OK;
}
