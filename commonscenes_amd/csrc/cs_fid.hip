// FID / KID statistics in fp64 (scripts/compute_fid_scores_3dfront.py -> cleanfid's frechet_distance / kernel_distance): the
// device half of commonscenes_amd/fid.py.
//   * cs_fid_moments      column means and the centred sum of squares of an fp32 feature matrix, fp64, two passes
//   * cs_fid_widen        fp32 -> fp64, optionally centred, optionally transposed (LDS tile transpose)
//   * cs_fid_gram         G = post(A B^T) on v_mfma_f64_16x16x4_f64, both operands K-contiguous
//   * cs_fid_subset_sums  sum of a gathered m x m sub-block of a kernel matrix, one workgroup per subset
// Every reduction has a fixed partition and a fixed order; the only atomic is the integer OR into the sticky index word.
//
// cs_fid_gram: a workgroup of four waves owns a 64 x 64 output tile, each wave a 32 x 32 quarter = 2 x 2 MFMA tiles (16
// accumulator doubles per lane).  K runs in slabs of 16: both 64 x 16 operand slabs are loaded from global memory with one
// 8-byte load per lane, 16 lanes covering the 128 contiguous bytes of one row (any lda / ldb / base alignment; rows and
// columns past the matrix and the K tail are zero-filled, never read), held in registers while the previous slab is
// multiplied, and written to LDS rows of 17 doubles.  The MFMA operand of a lane is the double at
// [row = lane & 15][k = 4 step + (lane >> 4)].  hipcc pairs the reads of two steps into one ds_read2_b64 (read in the
// assembly: 8 of them per slab and wave), which serves each of its two accesses in four 16-lane groups over 32 dword banks:
// a group is the 16 rows at one k, and with an odd row stride (17 doubles = 34 dwords) they fall on 16 distinct even dword
// banks -- conflict-free; a stride of 16 puts all 16 rows on one bank, 18 is two-way.  Should a compiler emit plain
// ds_read_b64 instead (32-lane halves over 64 dword banks), 17 costs one two-way collision per half (row 15 / k + 1 on row
// 0 / k).  The slab writes are 16 consecutive doubles per 16-lane group: conflict-free at any stride.  A wave reads 32 bytes
// per lane for every four f64 MFMAs (each operand is used twice).  17 KiB of LDS and 116 registers per
// lane (32 of them accumulators) admit four workgroups per CU; the matrices of this module have at most a few thousand rows,
// so there are few tiles and the tile is kept small rather than register-blocked further.
// The K order of an output element is k = 0, 1, 2, ... in MFMA steps of four from a zero accumulator, whichever tile or
// wave it falls into: a sub-block computed alone carries the bits of the same block inside the full matrix.
#include "cs_common.h"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------------------------------------
// moments
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int MO_COLS = 64;      // columns per workgroup (CS_FID_MOMENT_COLS)
constexpr int MO_ROWS = 16;      // row groups per workgroup: thread (g, c) owns rows g, g + 16, ... of column c
constexpr int MO_T = MO_COLS * MO_ROWS;

__global__ __launch_bounds__(MO_T) void fid_moments_kernel(const float* __restrict__ x, int n, int d, int64_t ldx,
                                                           double* __restrict__ mu, double* __restrict__ ss) {
  __shared__ double red[MO_ROWS][MO_COLS];
  __shared__ double col[MO_COLS];
  const int c = threadIdx.x % MO_COLS, g = threadIdx.x / MO_COLS;
  const int j = blockIdx.x * MO_COLS + c;
  const bool live = j < d;
  double s = 0.0;
  if (live)
    for (int i = g; i < n; i += MO_ROWS) s += (double)x[i * ldx + j];
  red[g][c] = s;
  __syncthreads();
  if (g == 0) {
    double t = red[0][c];
    for (int k = 1; k < MO_ROWS; ++k) t += red[k][c];
    t = t / (double)n;
    col[c] = t;
    if (live) mu[j] = t;
  }
  __syncthreads();
  const double m = col[c];
  __syncthreads();
  // second pass over the centred values (never sum x^2 - n mu^2: at a mean of 100 and a spread of 1 that form loses 8 digits)
  s = 0.0;
  if (live)
    for (int i = g; i < n; i += MO_ROWS) {
      const double v = (double)x[i * ldx + j] - m;
      s += v * v;
    }
  red[g][c] = s;
  __syncthreads();
  if (g == 0) {
    double t = red[0][c];
    for (int k = 1; k < MO_ROWS; ++k) t += red[k][c];
    col[c] = t;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = col[0];
    for (int k = 1; k < MO_COLS; ++k) t += col[k];
    ss[1 + blockIdx.x] = t;
  }
}

__global__ void fid_moments_fold_kernel(double* __restrict__ ss, int chunks) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    double t = ss[1];
    for (int k = 1; k < chunks; ++k) t += ss[1 + k];
    ss[0] = t;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// widen
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int WD_TILE = 32;
constexpr int WD_T = 256;

__global__ __launch_bounds__(WD_T) void fid_widen_kernel(const float* __restrict__ x, int n, int d, int64_t ldx,
                                                         const double* __restrict__ mu, double* __restrict__ out, int64_t ldo,
                                                         int transpose) {
  __shared__ double tile[WD_TILE][WD_TILE + 1];
  const int tx = threadIdx.x % WD_TILE, ty = threadIdx.x / WD_TILE;
  const int r0 = blockIdx.y * WD_TILE, c0 = blockIdx.x * WD_TILE;
  const int cj = c0 + tx;
  const double m = (mu && cj < d) ? mu[cj] : 0.0;
  if (!transpose) {
    for (int r = ty; r < WD_TILE; r += WD_T / WD_TILE) {
      const int i = r0 + r;
      if (i < n && cj < d) {
        const double v = (double)x[i * ldx + cj];
        out[i * ldo + cj] = mu ? v - m : v;
      }
    }
    return;
  }
  for (int r = ty; r < WD_TILE; r += WD_T / WD_TILE) {
    const int i = r0 + r;
    double v = 0.0;
    if (i < n && cj < d) {
      v = (double)x[i * ldx + cj];
      if (mu) v = v - m;
    }
    tile[r][tx] = v;
  }
  __syncthreads();
  // out[column][row]: lanes run along the rows of x, which are contiguous in the transposed image
  for (int r = ty; r < WD_TILE; r += WD_T / WD_TILE) {
    const int j = c0 + r, i = r0 + tx;
    if (j < d && i < n) out[j * ldo + i] = tile[tx][r];
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// gram
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int GR_TILE = 64;      // output rows and columns per workgroup
constexpr int GR_K = 16;         // K per slab
constexpr int GR_LD = 17;        // LDS row stride in doubles (see the file comment)
constexpr int GR_T = 256;
constexpr int GR_PER = GR_TILE * GR_K / GR_T;      // slab elements per lane and operand: 4

__device__ __forceinline__ void gram_fetch(const double* __restrict__ p, int rows, int k, int64_t ld, int row0, int k0,
                                           double (&v)[GR_PER]) {
  const int kk = threadIdx.x % GR_K, r = threadIdx.x / GR_K;
#pragma unroll
  for (int e = 0; e < GR_PER; ++e) {
    const int row = row0 + r + e * (GR_T / GR_K);
    v[e] = (row < rows && k0 + kk < k) ? p[row * ld + (k0 + kk)] : 0.0;
  }
}

__global__ __launch_bounds__(GR_T) void fid_gram_kernel(const double* __restrict__ a, const double* __restrict__ b,
                                                        double* __restrict__ g, int n1, int n2, int k, int64_t lda,
                                                        int64_t ldb, int64_t ldg, int mode, double gamma, double coef0) {
  __shared__ double sa[GR_TILE][GR_LD];
  __shared__ double sb[GR_TILE][GR_LD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
  const int row0 = blockIdx.y * GR_TILE, col0 = blockIdx.x * GR_TILE;
  const int fk = threadIdx.x % GR_K, fr = threadIdx.x / GR_K;
  f64x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (f64x4){0.0, 0.0, 0.0, 0.0};
  double va[GR_PER], vb[GR_PER];
  gram_fetch(a, n1, k, lda, row0, 0, va);
  gram_fetch(b, n2, k, ldb, col0, 0, vb);
  for (int k0 = 0; k0 < k; k0 += GR_K) {
    __syncthreads();            // the previous slab has been read by every wave
#pragma unroll
    for (int e = 0; e < GR_PER; ++e) {
      sa[fr + e * (GR_T / GR_K)][fk] = va[e];
      sb[fr + e * (GR_T / GR_K)][fk] = vb[e];
    }
    __syncthreads();
    if (k0 + GR_K < k) {        // the next slab travels while this one is multiplied
      gram_fetch(a, n1, k, lda, row0, k0 + GR_K, va);
      gram_fetch(b, n2, k, ldb, col0, k0 + GR_K, vb);
    }
#pragma unroll
    for (int s = 0; s < GR_K / 4; ++s) {
      const int kk = 4 * s + (lane >> 4);
      const double a0 = sa[wr + (lane & 15)][kk], a1 = sa[wr + 16 + (lane & 15)][kk];
      const double b0 = sb[wc + (lane & 15)][kk], b1 = sb[wc + 16 + (lane & 15)][kk];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
  }
  // f64 C/D map: col = lane & 15, row = (lane >> 4) + 4 * reg
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row0 + wr + 16 * i + (lane >> 4) + 4 * r;
        const int col = col0 + wc + 16 * j + (lane & 15);
        if (row < n1 && col < n2) {
          double s = acc[i][j][r];
          if (mode == 1) {
            const double p = s * gamma + coef0;        // two roundings: the build has -ffp-contract=off
            s = p * p * p;
          }
          g[row * ldg + col] = s;
        }
      }
}

// ---------------------------------------------------------------------------------------------------------------------------
// subset sums
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int SS_T = 1024;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(SS_T) void fid_subset_sums_kernel(const double* __restrict__ kmat, int n_r, int n_c, int64_t ldk,
                                                               const int32_t* __restrict__ ri, const int32_t* __restrict__ ci,
                                                               int m, int skip_diag, double* __restrict__ out,
                                                               int32_t* __restrict__ err) {
  __shared__ double red[SS_T / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int32_t* rows = ri + (int64_t)blockIdx.x * m;
  const int32_t* cols = ci + (int64_t)blockIdx.x * m;
  // wave w owns positions p = w, w + 16, ...; lane l the positions q = l, l + 64, ...: p outer, q inner
  double s = 0.0;
  bool bad = false;
  for (int p = wave; p < m; p += SS_T / 64) {
    const int r = rows[p];
    const bool rbad = r < 0 || r >= n_r;                 // compared BEFORE anything is read through it
    for (int q = lane; q < m; q += 64) {
      if (skip_diag && q == p) continue;
      const int c = cols[q];
      if (rbad || c < 0 || c >= n_c) {
        bad = true;
        s += __builtin_nan("");
      } else {
        s += kmat[r * ldk + c];
      }
    }
  }
  s = wave_sum_f64(s);
  if (lane == 0) red[wave] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = red[0];
    for (int w = 1; w < SS_T / 64; ++w) t += red[w];
    out[blockIdx.x] = t;
  }
  if (bad) atomicOr(err, 1);
}

}  // namespace

extern "C" int cs_fid_moments(const float* x, int n, int d, int ldx, double* mu, double* ss, cs_stream_t stream) {
  if (!x || !mu || !ss || n < 1 || d < 1 || ldx < d) return CS_EINVAL;
  const int chunks = (d + MO_COLS - 1) / MO_COLS;
  CS_LAUNCH(fid_moments_kernel, dim3(chunks), dim3(MO_T), 0, (hipStream_t)stream, x, n, d, (int64_t)ldx, mu, ss);
  CS_CHECK_LAUNCH();
  CS_LAUNCH(fid_moments_fold_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, ss, chunks);
  CS_CHECK_LAUNCH();
  return CS_OK;
}

extern "C" int cs_fid_widen(const float* x, int n, int d, int ldx, const double* mu, double* out, int ldo, int transpose,
                            cs_stream_t stream) {
  if (!x || !out || n < 1 || d < 1 || ldx < d || ldo < (transpose ? n : d)) return CS_EINVAL;
  const int gx = (d + WD_TILE - 1) / WD_TILE, gy = (n + WD_TILE - 1) / WD_TILE;
  if (gy > 65535) return CS_EINVAL;
  CS_LAUNCH(fid_widen_kernel, dim3(gx, gy), dim3(WD_T), 0, (hipStream_t)stream, x, n, d, (int64_t)ldx, mu, out, (int64_t)ldo,
            transpose ? 1 : 0);
  CS_CHECK_LAUNCH();
  return CS_OK;
}

extern "C" int cs_fid_gram(const double* a, const double* b, double* g, int n1, int n2, int k, int lda, int ldb, int ldg,
                           int mode, double gamma, double coef0, cs_stream_t stream) {
  if (!a || !b || !g || n1 < 1 || n2 < 1 || k < 1 || lda < k || ldb < k || ldg < n2 || (mode != 0 && mode != 1))
    return CS_EINVAL;
  const int gx = (n2 + GR_TILE - 1) / GR_TILE, gy = (n1 + GR_TILE - 1) / GR_TILE;
  if (gy > 65535) return CS_EINVAL;
  CS_LAUNCH(fid_gram_kernel, dim3(gx, gy), dim3(GR_T), 0, (hipStream_t)stream, a, b, g, n1, n2, k, (int64_t)lda, (int64_t)ldb,
            (int64_t)ldg, mode, gamma, coef0);
  CS_CHECK_LAUNCH();
  return CS_OK;
}

extern "C" int cs_fid_subset_sums(const double* kmat, int n_r, int n_c, int ldk, const int32_t* ri, const int32_t* ci,
                                  int nsub, int m, int skip_diag, double* out, int32_t* err_word, cs_stream_t stream) {
  if (!kmat || !ri || !ci || !out || !err_word || n_r < 1 || n_c < 1 || ldk < n_c || nsub < 1 || m < 1) return CS_EINVAL;
  CS_LAUNCH(fid_subset_sums_kernel, dim3(nsub), dim3(SS_T), 0, (hipStream_t)stream, kmat, n_r, n_c, (int64_t)ldk, ri, ci, m,
            skip_diag ? 1 : 0, out, err_word);
  CS_CHECK_LAUNCH();
  return CS_OK;
}
