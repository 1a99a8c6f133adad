// Held-out checkpoint evaluation glue (gfx950): the forward-diffusion noising with a per-sample timestep and one-pass
// per-sample error sums / occupancy counts over pairs of volumes.
//   cs_q_sample   sdfusion_txt2shape_model.py:268-272 (q_sample): two rounded fp32 multiplies and one rounded add per element,
//                 as the reference's three ATen ops; optional row maps so a shapes x timesteps sweep never copies the latents
//   cs_pair_stats sdfusion_txt2shape_model.py:293-306,328 (get_loss + per-sample mean), losses.py:69-72 (L1),
//                 diff_utils/util.py:111-130 (iou): fp64 {sum d^2, sum |d|} and int64 {inter, union} per sample
// Determinism rule of cs_pair_stats: a sample is cut into chunks of CS_PAIR_CHUNK floats, one workgroup per (sample, chunk);
// every thread owns FIXED elements of its chunk, threads are folded by a fixed shuffle tree, waves in wave order, chunks in
// chunk order by a second kernel.  No atomics of any kind: a sample's result depends on its own floats only -- not on nb, not on
// its position in the batch, not on whether the 16-byte path was taken -- and two runs are bit-identical.
#include "cs_common.h"

#define CS_EVAL_THREADS 256

// ---------------------------------------------------------------------------------------------------------------------
// q_sample
// ---------------------------------------------------------------------------------------------------------------------
#define CS_QS_BLOCK_FLOATS 4096      // floats of one row per workgroup: 256 threads x 4 groups of 4

__device__ __forceinline__ float qs_one(float a, float x, float b, float n) {
  return __fadd_rn(__fmul_rn(a, x), __fmul_rn(b, n));        // never one fma: the reference rounds three times
}

template <bool VEC>
__global__ __launch_bounds__(CS_EVAL_THREADS) void q_sample_kernel(
    const float* __restrict__ x0, const float* __restrict__ noise, float* __restrict__ out, const int64_t* __restrict__ t,
    const float* __restrict__ sa, const float* __restrict__ s1, const int32_t* __restrict__ src,
    const int32_t* __restrict__ nsrc, int64_t per, int blocks_per_row, int T, int64_t x0_rows, int64_t noise_rows) {
  const int64_t r = blockIdx.x / blocks_per_row;
  const int64_t e0 = (int64_t)(blockIdx.x % blocks_per_row) * CS_QS_BLOCK_FLOATS;
  const int64_t tt = t[r];
  const int64_t xr = src ? (int64_t)src[r] : r;
  const int64_t nr = nsrc ? (int64_t)nsrc[r] : r;
  // the host wrapper rejects out-of-range indices before the launch; a caller of the C entry that did not gets a row of NaNs,
  // never an out-of-bounds read
  const bool ok = tt >= 0 && tt < T && xr >= 0 && xr < x0_rows && nr >= 0 && nr < noise_rows;
  const float a = ok ? sa[tt] : 0.f, b = ok ? s1[tt] : 0.f;
  const float* xp = x0 + (ok ? xr : 0) * per;
  const float* np_ = noise + (ok ? nr : 0) * per;
  float* op = out + r * per;
  const float bad = __builtin_nanf("");
  if (VEC) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t e = e0 + ((int64_t)j * CS_EVAL_THREADS + threadIdx.x) * 4;
      if (e < per) {                                           // per % 4 == 0: the whole group is inside the row
        const f32x4 xv = *(const f32x4*)(xp + e), nv = *(const f32x4*)(np_ + e);
        f32x4 o;
        o.x = qs_one(a, xv.x, b, nv.x);
        o.y = qs_one(a, xv.y, b, nv.y);
        o.z = qs_one(a, xv.z, b, nv.z);
        o.w = qs_one(a, xv.w, b, nv.w);
        if (!ok) o.x = o.y = o.z = o.w = bad;
        *(f32x4*)(op + e) = o;
      }
    }
  } else {
#pragma unroll 4
    for (int j = 0; j < CS_QS_BLOCK_FLOATS / CS_EVAL_THREADS; ++j) {
      const int64_t e = e0 + (int64_t)j * CS_EVAL_THREADS + threadIdx.x;
      if (e < per) op[e] = ok ? qs_one(a, xp[e], b, np_[e]) : bad;
    }
  }
}

extern "C" int cs_q_sample(const float* x0, const float* noise, float* out, const int64_t* t, const float* sa, const float* s1,
                           const int32_t* src, const int32_t* nsrc, int64_t rows, int64_t per, int T, int64_t x0_rows,
                           int64_t noise_rows, hipStream_t stream) {
  if (!x0 || !noise || !out || !t || !sa || !s1) return CS_EINVAL;
  if (rows <= 0 || per <= 0 || T <= 0 || x0_rows <= 0 || noise_rows <= 0) return CS_EINVAL;
  if ((!src && x0_rows < rows) || (!nsrc && noise_rows < rows)) return CS_EINVAL;      // the identity map would leave the tensor
  const int64_t bpr = (per + CS_QS_BLOCK_FLOATS - 1) / CS_QS_BLOCK_FLOATS;
  if (bpr * rows > 0x7fffffffLL) return CS_EINVAL;
  const bool vec = per % 4 == 0 && (((uintptr_t)x0 | (uintptr_t)noise | (uintptr_t)out) & 15) == 0;
  const dim3 grid((unsigned)(bpr * rows)), block(CS_EVAL_THREADS);
  if (vec)
    CS_LAUNCH(q_sample_kernel<true>, grid, block, 0, stream, x0, noise, out, t, sa, s1, src, nsrc, per, (int)bpr, T, x0_rows,
              noise_rows);
  else
    CS_LAUNCH(q_sample_kernel<false>, grid, block, 0, stream, x0, noise, out, t, sa, s1, src, nsrc, per, (int)bpr, T, x0_rows,
              noise_rows);
  CS_CHECK_LAUNCH();
  return CS_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// pair statistics
// ---------------------------------------------------------------------------------------------------------------------
// One partial per (sample, chunk): {sum d^2, sum |d|} as doubles, then {inter, union} as int64 -- 32 bytes.
struct PairPartial {
  double s2, s1;
  int64_t inter, uni;
};
static_assert(sizeof(PairPartial) == CS_PAIR_PARTIAL_BYTES, "CS_PAIR_PARTIAL_BYTES");
#define CS_PAIR_GROUPS (CS_PAIR_CHUNK / 4 / CS_EVAL_THREADS)      // groups of 4 floats per thread
static_assert(CS_PAIR_GROUPS * 4 * CS_EVAL_THREADS == CS_PAIR_CHUNK, "CS_PAIR_CHUNK");

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <bool VEC>
__global__ __launch_bounds__(CS_EVAL_THREADS) void pair_partials_kernel(
    const float* __restrict__ a, const float* __restrict__ b, PairPartial* __restrict__ part, int64_t per, int64_t lda,
    int64_t ldb, int chunks, float thr_a, float thr_b) {
  const int64_t s = blockIdx.x / chunks;
  const int ch = blockIdx.x % chunks;
  const float* ap = a + s * lda;
  const float* bp = b + s * ldb;
  const int64_t c0 = (int64_t)ch * CS_PAIR_CHUNK;
  float av[CS_PAIR_GROUPS][4], bv[CS_PAIR_GROUPS][4];
  int n[CS_PAIR_GROUPS];
  // loads first (all in flight together), arithmetic after: thread t owns floats c0 + 4 (j * 256 + t) .. + 3 of the chunk
#pragma unroll
  for (int j = 0; j < CS_PAIR_GROUPS; ++j) {
    const int64_t e = c0 + ((int64_t)j * CS_EVAL_THREADS + threadIdx.x) * 4;
    const int64_t left = per - e;
    n[j] = left >= 4 ? 4 : (left > 0 ? (int)left : 0);
    if (VEC && n[j] == 4) {
      const f32x4 x = *(const f32x4*)(ap + e), y = *(const f32x4*)(bp + e);
      av[j][0] = x.x; av[j][1] = x.y; av[j][2] = x.z; av[j][3] = x.w;
      bv[j][0] = y.x; bv[j][1] = y.y; bv[j][2] = y.z; bv[j][3] = y.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        av[j][k] = k < n[j] ? ap[e + k] : 0.f;
        bv[j][k] = k < n[j] ? bp[e + k] : 0.f;
      }
    }
  }
  double s2 = 0.0, s1 = 0.0;
  int inter = 0, uni = 0;
#pragma unroll
  for (int j = 0; j < CS_PAIR_GROUPS; ++j) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < n[j]) {
        const double d = (double)__fsub_rn(av[j][k], bv[j][k]);      // the difference is the reference's fp32 one
        s2 += d * d;                                                 // (exact in fp64: 24-bit x 24-bit)
        s1 += fabs(d);
        const bool oa = !(av[j][k] > thr_a), ob = !(bv[j][k] > thr_b);      // a NaN voxel counts as occupied, as in the masks
        inter += (oa && ob) ? 1 : 0;
        uni += (oa || ob) ? 1 : 0;
      }
    }
  }
  s2 = wave_sum_f64(s2);
  s1 = wave_sum_f64(s1);
  inter = wave_sum_i32(inter);
  uni = wave_sum_i32(uni);
  __shared__ double l2[CS_EVAL_THREADS / 64], l1[CS_EVAL_THREADS / 64];
  __shared__ int li[CS_EVAL_THREADS / 64], lu[CS_EVAL_THREADS / 64];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    l2[w] = s2; l1[w] = s1; li[w] = inter; lu[w] = uni;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    PairPartial p = {0.0, 0.0, 0, 0};
#pragma unroll
    for (int i = 0; i < CS_EVAL_THREADS / 64; ++i) {
      p.s2 += l2[i]; p.s1 += l1[i]; p.inter += li[i]; p.uni += lu[i];
    }
    part[blockIdx.x] = p;
  }
}

// one wave per sample: lane l folds chunks l, l + 64, ... in order, then the fixed shuffle tree
__global__ __launch_bounds__(64) void pair_finish_kernel(const PairPartial* __restrict__ part, double* __restrict__ sums,
                                                         int64_t* __restrict__ counts, int chunks) {
  const int s = blockIdx.x;
  const PairPartial* p = part + (int64_t)s * chunks;
  double s2 = 0.0, s1 = 0.0;
  int64_t inter = 0, uni = 0;
  for (int c = threadIdx.x; c < chunks; c += 64) {
    s2 += p[c].s2; s1 += p[c].s1; inter += p[c].inter; uni += p[c].uni;
  }
  s2 = wave_sum_f64(s2);
  s1 = wave_sum_f64(s1);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    inter += __shfl_xor(inter, o, 64);
    uni += __shfl_xor(uni, o, 64);
  }
  if (threadIdx.x == 0) {
    if (sums) { sums[2 * s] = s2; sums[2 * s + 1] = s1; }
    if (counts) { counts[2 * s] = inter; counts[2 * s + 1] = uni; }
  }
}

extern "C" int cs_pair_stats(const float* a, const float* b, int nb, int64_t per, int64_t lda, int64_t ldb, double* sums,
                             int64_t* counts, float thr_a, float thr_b, void* workspace, int64_t workspace_bytes,
                             hipStream_t stream) {
  if (!a || !b || !workspace || (!sums && !counts)) return CS_EINVAL;
  if (nb <= 0 || per <= 0 || lda < per || ldb < per) return CS_EINVAL;
  if ((((uintptr_t)a | (uintptr_t)b) & 3) || ((uintptr_t)workspace & 7)) return CS_EINVAL;
  const int64_t chunks = (per + CS_PAIR_CHUNK - 1) / CS_PAIR_CHUNK;
  if (chunks * nb > 0x7fffffffLL) return CS_EINVAL;
  if (workspace_bytes < chunks * nb * (int64_t)sizeof(PairPartial)) return CS_ENOMEM;
  const bool vec = (((uintptr_t)a | (uintptr_t)b) & 15) == 0 && lda % 4 == 0 && ldb % 4 == 0;
  PairPartial* part = (PairPartial*)workspace;
  const dim3 grid((unsigned)(chunks * nb)), block(CS_EVAL_THREADS);
  if (vec)
    CS_LAUNCH(pair_partials_kernel<true>, grid, block, 0, stream, a, b, part, per, lda, ldb, (int)chunks, thr_a, thr_b);
  else
    CS_LAUNCH(pair_partials_kernel<false>, grid, block, 0, stream, a, b, part, per, lda, ldb, (int)chunks, thr_a, thr_b);
  CS_CHECK_LAUNCH();
  CS_LAUNCH(pair_finish_kernel, dim3((unsigned)nb), dim3(64), 0, stream, part, sums, counts, (int)chunks);
  CS_CHECK_LAUNCH();
  return CS_OK;
}
