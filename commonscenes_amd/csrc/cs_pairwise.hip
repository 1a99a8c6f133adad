// All-pairs shape-quality kernels (the layer scripts/compute_mmd_cov_1nn.py builds over the per-pair metric kernels):
//   * cs_chamfer_pairwise     the Chamfer matrix of _pairwise_EMD_CD_ (:110-150), set A x set B, one workgroup per pair
//   * cs_chamfer_pairlist     the same distance for a list of pairs of ONE set (eval_3dfront.py:688-699, consistency_check.py:78-80)
//   * cs_emd_pairwise_cost    match_cost of every pair (approxmatch.cu:3-182 + matchcostkernel :184-224) with the whole
//                             nine-level auction inside one workgroup and NO match matrix
//   * cs_occupancy_histogram  the nearest-cell counters of entropy_of_occupancy_grid (:270-309)
// The reference feeds its batched kernels by copying one cloud `batch_size` times and looping on the host; here a pair is
// a workgroup, indexed along x (the pair count passes gridDim.y's 65535), and no cloud is ever copied.
#include "cs_common.h"

namespace {

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}

// sum of 256 per-thread partials, fixed tree (the order never depends on the launch)
__device__ __forceinline__ float block_sum_256(float v, float* part) {
  __syncthreads();
  part[threadIdx.x] = v;
  for (int s = 128; s > 0; s >>= 1) {
    __syncthreads();
    if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
  }
  __syncthreads();
  return part[0];
}

// ---------------------------------------------------------------------------------------------------------------------
// Chamfer.  Thread t keeps R points of cloud A in registers (rows row0 + r * 256 + t) and walks cloud B, staged through LDS
// in 1024-point tiles (every lane reads the same 16 bytes per step: a broadcast).  Each distance ((dx*dx + dy*dy) + dz*dz,
// dx = b - a, the expression of cs_chamfer_nm_distance) is formed ONCE: it updates the row's running minimum in a
// register and, through a wave-wide minimum and one LDS atomic per wave, the column's minimum in colmin[q].  Minima are
// exact and order-free (non-negative floats order like their bit patterns), so the atomics do not touch determinism.
// The two means are then summed in ONE pattern -- thread t adds elements t, t + 256, ... in ascending order, then a
// fixed tree -- for rows and columns alike: pair (i, j) and pair (j, i) of a symmetric matrix are the same bits.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int CD_T = 256, CD_TILE = 1024;

template <int R>
__device__ __forceinline__ float cd_rows(const float* __restrict__ A, int p, int row0, const float* __restrict__ B, int q,
                                         float4* tile, unsigned* colmin, float acc) {
  const int tid = threadIdx.x, lane = tid & 63;
  float x[R], y[R], z[R], best[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int row = row0 + r * CD_T + tid;
    // a row past the cloud's end sits at 1e30: its distances overflow to +inf and never win a minimum
    x[r] = y[r] = z[r] = 1e30f;
    if (row < p) x[r] = A[3 * (int64_t)row], y[r] = A[3 * (int64_t)row + 1], z[r] = A[3 * (int64_t)row + 2];
    best[r] = __builtin_inff();
  }
  for (int l0 = 0; l0 < q; l0 += CD_TILE) {
    const int cnt = min(CD_TILE, q - l0);
    __syncthreads();
    for (int e = tid; e < cnt; e += CD_T)
      tile[e] = make_float4(B[3 * (int64_t)(l0 + e)], B[3 * (int64_t)(l0 + e) + 1], B[3 * (int64_t)(l0 + e) + 2], 0.f);
    __syncthreads();
    for (int l = 0; l < cnt; ++l) {
      const float4 b = tile[l];
      float cm = __builtin_inff();
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float dx = b.x - x[r], dy = b.y - y[r], dz = b.z - z[r];
        const float d = (dx * dx + dy * dy) + dz * dz;
        best[r] = fminf(best[r], d);
        cm = fminf(cm, d);
      }
      cm = wave_min(cm);
      if (lane == 0) atomicMin(&colmin[l0 + l], __float_as_uint(cm));
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (row0 + r * CD_T + tid < p) acc += best[r];
  return acc;
}

__global__ __launch_bounds__(CD_T) void chamfer_pair_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                            float* __restrict__ out, int nb, int p, int q, int symmetric) {
  extern __shared__ float4 cd_smem[];
  float4* tile = cd_smem;                                       // [CD_TILE]
  unsigned* colmin = (unsigned*)(cd_smem + CD_TILE);            // [q]
  float* part = (float*)(colmin + q);                           // [CD_T]
  const int i = blockIdx.x / nb, j = blockIdx.x % nb, tid = threadIdx.x;
  if (symmetric && i > j) return;                               // written by pair (j, i)
  const float* A = a + (int64_t)i * p * 3;
  const float* B = b + (int64_t)j * q * 3;
  for (int e = tid; e < q; e += CD_T) colmin[e] = 0x7f800000u;  // +inf
  float acc = 0.f;
  int row0 = 0;
  // slabs of 256 rows, taken eight, four, two, one at a time: no register set is spent on rows the cloud does not have
  for (int slabs = (p + CD_T - 1) / CD_T; slabs > 0;) {
    if (slabs >= 8) acc = cd_rows<8>(A, p, row0, B, q, tile, colmin, acc), row0 += 8 * CD_T, slabs -= 8;
    else if (slabs >= 4) acc = cd_rows<4>(A, p, row0, B, q, tile, colmin, acc), row0 += 4 * CD_T, slabs -= 4;
    else if (slabs >= 2) acc = cd_rows<2>(A, p, row0, B, q, tile, colmin, acc), row0 += 2 * CD_T, slabs -= 2;
    else acc = cd_rows<1>(A, p, row0, B, q, tile, colmin, acc), row0 += CD_T, slabs -= 1;
  }
  const float srow = block_sum_256(acc, part);                  // (its first barrier also orders the last LDS atomics)
  float cacc = 0.f;
  for (int e = tid; e < q; e += CD_T) cacc += __uint_as_float(colmin[e]);
  const float scol = block_sum_256(cacc, part);
  if (tid == 0) {
    const float v = srow / (float)p + scol / (float)q;
    out[(int64_t)i * nb + j] = v;
    if (symmetric) out[(int64_t)j * nb + i] = v;
  }
}

// The Chamfer distance of a LIST of pairs of one cloud set (the diversity and consistency tables: consecutive runs of an
// object, objects the ground truth marks "same as").  chamfer_pair_kernel's schedule with A = cloud pairs[k][0] and
// B = cloud pairs[k][1]: the same slabs, the same summation pattern, the same final expression, so out[k] carries the bits
// of cs_chamfer_pairwise(clouds, clouds)[i][j] whatever the list's length, the pair's place in it or m.
__global__ __launch_bounds__(CD_T) void chamfer_pairlist_kernel(const float* __restrict__ clouds,
                                                                const int32_t* __restrict__ pairs, float* __restrict__ out,
                                                                int m, int p, int32_t* __restrict__ err) {
  extern __shared__ float4 cd_smem[];
  float4* tile = cd_smem;                                       // [CD_TILE]
  unsigned* colmin = (unsigned*)(cd_smem + CD_TILE);            // [p]
  float* part = (float*)(colmin + p);                           // [CD_T]
  const int tid = threadIdx.x;
  const int i = pairs[2 * (int64_t)blockIdx.x], j = pairs[2 * (int64_t)blockIdx.x + 1];
  if (i < 0 || i >= m || j < 0 || j >= m) {                     // (the whole workgroup leaves, before any barrier)
    if (tid == 0) out[blockIdx.x] = __builtin_nanf(""), atomicOr(err, 1);
    return;
  }
  const float* A = clouds + (int64_t)i * p * 3;
  const float* B = clouds + (int64_t)j * p * 3;
  for (int e = tid; e < p; e += CD_T) colmin[e] = 0x7f800000u;  // +inf
  float acc = 0.f;
  int row0 = 0;
  for (int slabs = (p + CD_T - 1) / CD_T; slabs > 0;) {
    if (slabs >= 8) acc = cd_rows<8>(A, p, row0, B, p, tile, colmin, acc), row0 += 8 * CD_T, slabs -= 8;
    else if (slabs >= 4) acc = cd_rows<4>(A, p, row0, B, p, tile, colmin, acc), row0 += 4 * CD_T, slabs -= 4;
    else if (slabs >= 2) acc = cd_rows<2>(A, p, row0, B, p, tile, colmin, acc), row0 += 2 * CD_T, slabs -= 2;
    else acc = cd_rows<1>(A, p, row0, B, p, tile, colmin, acc), row0 += CD_T, slabs -= 1;
  }
  const float srow = block_sum_256(acc, part);
  float cacc = 0.f;
  for (int e = tid; e < p; e += CD_T) cacc += __uint_as_float(colmin[e]);
  const float scol = block_sum_256(cacc, part);
  if (tid == 0) out[blockIdx.x] = srow / (float)p + scol / (float)p;
}

// ---------------------------------------------------------------------------------------------------------------------
// Approximate EMD.  One workgroup per pair, the nine levels and their three passes inside it, ordered by workgroup
// barriers.  Thread t OWNS rows t, t + T, ... of both clouds: point, remain and ratio live in registers for the whole
// auction.  A pass walks the other cloud in tiles of T points that their owners write into LDS as {x, y, z, w} (w =
// remainR, ratioL or ratioR: what that pass multiplies by) -- no global traffic after the first load -- and every lane
// reads the same 16 bytes per step.  Two tile buffers, one barrier per tile: a buffer is rewritten only after the barrier
// of the tile in between, which every thread passes after it has finished reading.
// Per element the arithmetic is that of emd_ratio_l / emd_ratio_r / emd_match_kernel (cs_metrics.hip), sums over the other
// cloud in index order; pass 3 adds w * |d| to the row's running cost instead of storing w, so nothing of size n * m exists.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int EMD_T = 1024;

__device__ __forceinline__ float sqd(float x1, float y1, float z1, float x2, float y2, float z2) {
  return (x2 - x1) * (x2 - x1) + (y2 - y1) * (y2 - y1) + (z2 - z1) * (z2 - z1);
}

template <int ROWS>
__global__ __launch_bounds__(EMD_T) void emd_pair_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                         float* __restrict__ cost, int nb, int n, int m, float multiL,
                                                         float multiR) {
  __shared__ float4 buf[2][EMD_T];
  __shared__ float part[EMD_T];
  const int T = blockDim.x, tid = threadIdx.x;
  const int i = blockIdx.x / nb, j = blockIdx.x % nb;
  const float* p1 = a + (int64_t)i * n * 3;
  const float* p2 = b + (int64_t)j * m * 3;
  float x1[ROWS], y1[ROWS], z1[ROWS], remL[ROWS], ratL[ROWS], cst[ROWS];
  float x2[ROWS], y2[ROWS], z2[ROWS], remR[ROWS], ratR[ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    const int k = r * T + tid;
    x1[r] = y1[r] = z1[r] = x2[r] = y2[r] = z2[r] = 0.f;
    if (k < n) x1[r] = p1[3 * k], y1[r] = p1[3 * k + 1], z1[r] = p1[3 * k + 2];
    if (k < m) x2[r] = p2[3 * k], y2[r] = p2[3 * k + 1], z2[r] = p2[3 * k + 2];
    remL[r] = k < n ? multiL : 0.f;                              // rows past a cloud's end carry no mass and are never
    remR[r] = k < m ? multiR : 0.f;                              // read as the other side (tiles stop at the count)
    ratL[r] = ratR[r] = cst[r] = 0.f;
  }
  int ph = 0;
  float level = -16384.0f;                                       // -4^7, then / 4 per level down to -4^-1 (:24-29), exact
  for (int lv = 0; lv < 9; ++lv, level *= 0.25f) {
    float sum[ROWS];
    // pass 1 (:31-62): ratioL[k] = remainL[k] / (1e-9 + sum_l exp(level d(k,l)) remainR[l])
#pragma unroll
    for (int r = 0; r < ROWS; ++r) sum[r] = 1e-9f;
#pragma unroll
    for (int t = 0; t < ROWS; ++t) {
      const int cnt = min(T, m - t * T);
      if (cnt <= 0) break;
      buf[ph][tid] = make_float4(x2[t], y2[t], z2[t], remR[t]);
      __syncthreads();
      for (int l = 0; l < cnt; ++l) {
        const float4 q = buf[ph][l];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) sum[r] += __expf(level * sqd(x1[r], y1[r], z1[r], q.x, q.y, q.z)) * q.w;
      }
      ph ^= 1;
    }
#pragma unroll
    for (int r = 0; r < ROWS; ++r) ratL[r] = remL[r] / sum[r];
    // pass 2 (:79-113): sumr = remainR[l] sum_k exp(level d) ratioL[k]; ratioR = min(remainR / (sumr + 1e-9), 1) remainR;
    // remainR = max(0, remainR - sumr)
#pragma unroll
    for (int r = 0; r < ROWS; ++r) sum[r] = 0.f;
#pragma unroll
    for (int t = 0; t < ROWS; ++t) {
      const int cnt = min(T, n - t * T);
      if (cnt <= 0) break;
      buf[ph][tid] = make_float4(x1[t], y1[t], z1[t], ratL[t]);
      __syncthreads();
      for (int k = 0; k < cnt; ++k) {
        const float4 q = buf[ph][k];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) sum[r] += __expf(level * sqd(q.x, q.y, q.z, x2[r], y2[r], z2[r])) * q.w;
      }
      ph ^= 1;
    }
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      const float rr = remR[r];
      const float sumr = sum[r] * rr;
      const float consumption = fminf(rr / (sumr + 1e-9f), 1.0f);
      ratR[r] = consumption * rr;
      remR[r] = fmaxf(0.0f, rr - sumr);
    }
    // pass 3 (:131-160 and matchcostkernel :184-224): w = exp(level d) ratioL[k] ratioR[l]; cost[k] += w |d|;
    // remainL[k] = max(0, remainL[k] - sum_l w)
#pragma unroll
    for (int r = 0; r < ROWS; ++r) sum[r] = 0.f;
#pragma unroll
    for (int t = 0; t < ROWS; ++t) {
      const int cnt = min(T, m - t * T);
      if (cnt <= 0) break;
      buf[ph][tid] = make_float4(x2[t], y2[t], z2[t], ratR[t]);
      __syncthreads();
      for (int l = 0; l < cnt; ++l) {
        const float4 q = buf[ph][l];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
          const float d2 = sqd(x1[r], y1[r], z1[r], q.x, q.y, q.z);
          const float w = __expf(level * d2) * ratL[r] * q.w;
          cst[r] += w * __builtin_amdgcn_sqrtf(d2);
          sum[r] += w;
        }
      }
      ph ^= 1;
    }
#pragma unroll
    for (int r = 0; r < ROWS; ++r) remL[r] = fmaxf(0.0f, remL[r] - sum[r]);
  }
  // rows of a thread in ascending order, then a fixed tree over the (power-of-two padded) threads
  float acc = 0.f;
#pragma unroll
  for (int r = 0; r < ROWS; ++r)
    if (r * T + tid < n) acc += cst[r];
  __syncthreads();
  part[tid] = acc;
  for (int e = T + tid; e < EMD_T; e += T) part[e] = 0.f;
  for (int s = EMD_T / 2; s > 0; s >>= 1) {
    __syncthreads();
    if (tid < s) part[tid] += part[tid + s];
  }
  if (tid == 0) cost[blockIdx.x] = part[0];
}

// ---------------------------------------------------------------------------------------------------------------------
// Occupancy histogram.  hist_nearest_kernel: the lowest-index nearest grid cell of every point (the scan of
// chamfer_nm_kernel, the grid read once per 256 points through LDS).  hist_count_kernel: one workgroup per cloud;
// grid_counters takes every hit, grid_bernoulli one hit per cloud and cell -- the thread that sets the cell's bit in
// the cloud's LDS bitmap first.  Integer atomics: exact whatever the order.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hist_nearest_kernel(const float* __restrict__ pts, const float* __restrict__ grid,
                                                           int32_t* __restrict__ idx, int64_t total, int g) {
  constexpr int TILE = 1024;
  __shared__ float4 tile[TILE];
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const float* q = pts + (j < total ? j : 0) * 3;
  const float x1 = q[0], y1 = q[1], z1 = q[2];
  float best = 0.f;
  int best_i = 0;
  for (int k0 = 0; k0 < g; k0 += TILE) {
    const int cnt = min(TILE, g - k0);
    __syncthreads();
    for (int e = threadIdx.x; e < cnt; e += blockDim.x)
      tile[e] = make_float4(grid[3 * (k0 + e)], grid[3 * (k0 + e) + 1], grid[3 * (k0 + e) + 2], 0.f);
    __syncthreads();
    for (int k = 0; k < cnt; ++k) {
      const float4 c = tile[k];
      const float dx = c.x - x1, dy = c.y - y1, dz = c.z - z1;
      const float d = (dx * dx + dy * dy) + dz * dz;
      if ((k0 + k) == 0 || d < best) best = d, best_i = k0 + k;
    }
  }
  if (j < total) idx[j] = best_i;
}

__global__ __launch_bounds__(256) void hist_count_kernel(const int32_t* __restrict__ idx, int32_t* __restrict__ counters,
                                                         int32_t* __restrict__ bernoulli, int p, int g) {
  extern __shared__ unsigned seen[];                            // [(g + 31) / 32]
  const int words = (g + 31) / 32;
  for (int e = threadIdx.x; e < words; e += blockDim.x) seen[e] = 0u;
  __syncthreads();
  const int32_t* mine = idx + (int64_t)blockIdx.x * p;
  for (int e = threadIdx.x; e < p; e += blockDim.x) {
    const int c = mine[e];
    const unsigned bit = 1u << (c & 31);
    atomicAdd(&counters[c], 1);
    if (!(atomicOr(&seen[c >> 5], bit) & bit)) atomicAdd(&bernoulli[c], 1);
  }
}

template <int ROWS>
int launch_emd(const float* a, const float* b, float* cost, int na, int nb, int n, int m, int threads, float multiL,
               float multiR, hipStream_t s) {
  CS_LAUNCH(emd_pair_kernel<ROWS>, dim3(na * nb), dim3(threads), 0, s, a, b, cost, nb, n, m, multiL, multiR);
  CS_CHECK_LAUNCH();
  return CS_OK;
}

}  // namespace

extern "C" int cs_chamfer_pairwise(const float* a, const float* b, float* out, int na, int nb, int p, int q, int symmetric,
                                   cs_stream_t stream) {
  if (!a || !b || !out || na <= 0 || nb <= 0 || p <= 0 || q <= 0 || q > CS_CHAMFER_PAIRWISE_MAX_Q ||
      (int64_t)na * nb > 0x7fffffff)
    return CS_EINVAL;
  if (symmetric && (a != b || na != nb || p != q)) return CS_EINVAL;
  const size_t smem = CD_TILE * sizeof(float4) + (size_t)q * sizeof(unsigned) + CD_T * sizeof(float);
  if (smem > 64 * 1024) {
    (void)hipGetLastError();
    hipError_t e = hipFuncSetAttribute((const void*)chamfer_pair_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) return (int)e;
  }
  CS_LAUNCH(chamfer_pair_kernel, dim3(na * nb), dim3(CD_T), smem, (hipStream_t)stream, a, b, out, nb, p, q,
            symmetric ? 1 : 0);
  CS_CHECK_LAUNCH();
  return CS_OK;
}

extern "C" int cs_chamfer_pairlist(const float* clouds, const int32_t* pairs, float* out, int m, int p, int npairs,
                                   int32_t* err, cs_stream_t stream) {
  if (!clouds || !pairs || !out || !err || m <= 0 || p <= 0 || npairs <= 0 || p > CS_CHAMFER_PAIRWISE_MAX_Q)
    return CS_EINVAL;
  const size_t smem = CD_TILE * sizeof(float4) + (size_t)p * sizeof(unsigned) + CD_T * sizeof(float);
  if (smem > 64 * 1024) {
    (void)hipGetLastError();
    hipError_t e = hipFuncSetAttribute((const void*)chamfer_pairlist_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)smem);
    if (e != hipSuccess) return (int)e;
  }
  CS_LAUNCH(chamfer_pairlist_kernel, dim3(npairs), dim3(CD_T), smem, (hipStream_t)stream, clouds, pairs, out, m, p, err);
  CS_CHECK_LAUNCH();
  return CS_OK;
}

extern "C" int cs_emd_pairwise_cost(const float* a, const float* b, float* cost, int na, int nb, int n, int m,
                                    cs_stream_t stream) {
  if (!a || !b || !cost || na <= 0 || nb <= 0 || n <= 0 || m <= 0 || n > CS_EMD_PAIRWISE_MAX_POINTS ||
      m > CS_EMD_PAIRWISE_MAX_POINTS || (int64_t)na * nb > 0x7fffffff)
    return CS_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const float multiL = n >= m ? 1.f : (float)(m / n);           // integer ratios, approxmatch.cu:6-12
  const float multiR = n >= m ? (float)(n / m) : 1.f;
  const int big = n > m ? n : m;
  // up to 1024 points a thread owns one row of each cloud (whole waves); beyond, 1024 threads own ceil(big / 1024) rows
  const int threads = big >= EMD_T ? EMD_T : (big + 63) / 64 * 64;
  switch ((big + EMD_T - 1) / EMD_T) {
    case 1: return launch_emd<1>(a, b, cost, na, nb, n, m, threads, multiL, multiR, s);
    case 2: return launch_emd<2>(a, b, cost, na, nb, n, m, threads, multiL, multiR, s);
    case 3: return launch_emd<3>(a, b, cost, na, nb, n, m, threads, multiL, multiR, s);
    case 4: return launch_emd<4>(a, b, cost, na, nb, n, m, threads, multiL, multiR, s);
    case 5: return launch_emd<5>(a, b, cost, na, nb, n, m, threads, multiL, multiR, s);
    case 6: return launch_emd<6>(a, b, cost, na, nb, n, m, threads, multiL, multiR, s);
    case 7: return launch_emd<7>(a, b, cost, na, nb, n, m, threads, multiL, multiR, s);
    default: return launch_emd<8>(a, b, cost, na, nb, n, m, threads, multiL, multiR, s);
  }
}

extern "C" int cs_occupancy_histogram(const float* clouds, const float* grid, int32_t* idx, int32_t* counters,
                                      int32_t* bernoulli, int s, int p, int g, cs_stream_t stream) {
  if (!clouds || !grid || !idx || !counters || !bernoulli || s <= 0 || p <= 0 || g <= 0 ||
      g > CS_OCCUPANCY_MAX_CELLS || (int64_t)s * p > (int64_t)0x7fffffff * 256)
    return CS_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  (void)hipGetLastError();
  hipError_t e = hipMemsetAsync(counters, 0, (size_t)g * sizeof(int32_t), st);
  if (e == hipSuccess) e = hipMemsetAsync(bernoulli, 0, (size_t)g * sizeof(int32_t), st);
  if (e != hipSuccess) return (int)e;
  const int64_t total = (int64_t)s * p;
  CS_LAUNCH(hist_nearest_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, clouds, grid, idx, total, g);
  CS_CHECK_LAUNCH();
  CS_LAUNCH(hist_count_kernel, dim3(s), dim3(256), (size_t)((g + 31) / 32) * sizeof(unsigned), st, idx, counters, bernoulli,
            p, g);
  CS_CHECK_LAUNCH();
  return CS_OK;
}
