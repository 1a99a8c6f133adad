// GroupNorm (NDHWC) and LayerNorm for gfx950.  Both are HBM-bound streaming kernels:
// float4 coalesced loads, fp64 accumulation for GroupNorm statistics (a group spans up to
// 4096*42 elements), wave64 shuffles for LayerNorm rows.
#include <cstdlib>

#include "cs_common.h"
#include "cs_ln_pair.h"

namespace {

constexpr int GN_MIN_SPLIT_ROWS = 16;  // minimum rows handled by one statistics block
constexpr int GN_MAX_SPLITS = 256;
constexpr int64_t GN_SMALL_BYTES = 16 << 20;   // single-launch path: whole tensor at most this (L2 / MALL resident)
constexpr int64_t GN_SMALL_GROUP = 11264;      // ... and at most this many elements per (sample, group) workgroup
                                               // (16x4x4 voxels x 42 channels: 14.5 vs 18.0 / 25.4 vs 30.2 us, tools/gn_bench.py)

// The thread map of the row and line kernels: a thread keeps a column of V channels; a workgroup of 256 puts `tpr` threads on
// a row (line) of cv = c / V columns and walks `lanes` rows (lines) side by side.  Threads past tpr * lanes idle.
struct GnMap {
  int tpr, lanes;
};
__host__ __device__ __forceinline__ GnMap gn_map(int cv) {
  const int tpr = cv < 256 ? cv : 256;
  return {tpr, 256 / tpr};
}

// (mean, variance clamped at 0, 1 / std) of a group from its fp64 (sum, sum of squares)
__device__ __forceinline__ void gn_moments(double s, double q, double count, float eps, double& mean, double& var,
                                           float& rstd) {
  mean = s / count;
  var = q / count - mean * mean;
  if (var < 0) var = 0;
  rstd = (float)(1.0 / sqrt(var + (double)eps));
}

// |mean| + std * sqrt(n - 1) >= max |x| over the group (Samuelson's inequality), rounded UP to fp32; the maximum over all
// (sample, group)s bounds the tensor: what CsConvGemm.a_bound reads.  atomicMax of the bits: order-independent.
__device__ __forceinline__ float gn_bound_value(double mean, double var, double count) {
  const double b = fabs(mean) + sqrt(var * (count > 1.0 ? count - 1.0 : 1.0));
  float bf = (float)b;
  if ((double)bf < b) bf = __uint_as_float(__float_as_uint(bf) + 1u);
  return (bf == bf && bf > 0.f) ? bf : 0.f;
}
__device__ __forceinline__ void gn_bound_commit(float* bound, float bf) {
  if (bf > 0.f) atomicMax(reinterpret_cast<unsigned int*>(bound), __float_as_uint(bf));
}
__device__ __forceinline__ void gn_bound_max(float* bound, double mean, double var, double count) {
  gn_bound_commit(bound, gn_bound_value(mean, var, count));
}

// Pass 1: partial[n][split][g] = (sum, sumsq) in fp64.  Each thread owns fixed channel chunks so
// its accumulation order is fixed; the cross-thread reduction runs in a fixed order too, so the
// statistics are bit-reproducible run to run.
__global__ __launch_bounds__(256) void gn_partial_kernel(const float* __restrict__ x, int rows, int c,
                                                         int ldx, int groups, int nsplit, int rps,
                                                         double* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) double sm[];  // [rowlanes][c][2]
  const int n = blockIdx.x / nsplit;
  const int split = blockIdx.x % nsplit;
  const int ch4 = c >> 2;
  const int tpr = gn_map(ch4).tpr, rowlanes = gn_map(ch4).lanes;
  const int tid = threadIdx.x;
  const int rl = tid / tpr;
  const int cl = tid - rl * tpr;
  const int r0 = split * rps;
  const int r1 = min(rows, r0 + rps);
  const float* xb = x + (int64_t)n * rows * ldx;
  if (rl < rowlanes) {
    for (int c4 = cl; c4 < ch4; c4 += tpr) {
      double s0 = 0, s1 = 0, s2 = 0, s3 = 0, q0 = 0, q1 = 0, q2 = 0, q3 = 0;
      // four rows' loads in flight per thread (one 16-byte load per iteration left the kernel at ~45 % of the HBM
      // rate: too few bytes in flight per CU); the accumulation order is unchanged
      for (int r = r0 + rl; r < r1; r += 4 * rowlanes) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int rr = r + u * rowlanes;
          v[u] = rr < r1 ? *reinterpret_cast<const float4*>(xb + (int64_t)rr * ldx + c4 * 4)
                         : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (r + u * rowlanes < r1) {
            s0 += v[u].x; q0 += (double)v[u].x * v[u].x;
            s1 += v[u].y; q1 += (double)v[u].y * v[u].y;
            s2 += v[u].z; q2 += (double)v[u].z * v[u].z;
            s3 += v[u].w; q3 += (double)v[u].w * v[u].w;
          }
        }
      }
      double* d = sm + ((int64_t)rl * c + c4 * 4) * 2;
      d[0] = s0; d[1] = q0; d[2] = s1; d[3] = q1; d[4] = s2; d[5] = q2; d[6] = s3; d[7] = q3;
    }
  }
  __syncthreads();
  if (tid < groups) {
    const int cpg = c / groups;
    double s = 0, q = 0;
    for (int l = 0; l < rowlanes; ++l)
      for (int k = 0; k < cpg; ++k) {
        const double* d = sm + ((int64_t)l * c + tid * cpg + k) * 2;
        s += d[0];
        q += d[1];
      }
    double* o = partial + (((int64_t)n * nsplit + split) * groups + tid) * 2;
    o[0] = s;
    o[1] = q;
  }
}

// One wave per (sample, group): lanes take the row-slice partials in a strided fashion and a fixed butterfly
// combines them, so the result does not depend on scheduling (the serial version walked up to 256 dependent
// loads per thread: 17-27 us for what is a few KB of data).
__global__ __launch_bounds__(256) void gn_finalize_kernel(const double* __restrict__ partial, int nsplit, int groups,
                                                          double count, float eps, float* __restrict__ stats,
                                                          int total, float* __restrict__ bound = nullptr) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);  // n*groups + g
  if (i >= total) return;
  const int n = i / groups, g = i - n * groups;
  double s = 0, q = 0;
  for (int k = lane; k < nsplit; k += 64) {
    const double* d = partial + (((int64_t)n * nsplit + k) * groups + g) * 2;
    s += d[0];
    q += d[1];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o, 64);
    q += __shfl_xor(q, o, 64);
  }
  if (lane == 0) {
    double mean, var;
    float rstd;
    gn_moments(s, q, count, eps, mean, var, rstd);
    stats[2 * i] = (float)mean;
    stats[2 * i + 1] = rstd;
    if (bound) gn_bound_max(bound, mean, var, count);
  }
}

// Statistics from the producers' per-(row tile, column) partials (CsConvGemm.gn_part) instead of a pass over the tensor.
// One wave per (sample, group): for each channel of the group in turn the lanes stride over that channel's tiles, then a
// fixed butterfly -- the result does not depend on scheduling or on how many samples share the launch.
struct GnSegs {
  CsGnSeg s[4];
  int n;
};
// the (sum, sum of squares) of group g of sample n from the segments' partials: the lanes of one wave stride over the
// (channel, tile) pairs of each segment's share of the group -- independent loads, all in flight together (a first version
// walked the channels one after the other: up to 42 dependent load latencies per group) -- in a fixed order
__device__ __forceinline__ void gn_group_parts(const GnSegs& sg, int n, int g, int cpg, int lane, int nlanes, double& s,
                                               double& q) {
  s = 0;
  q = 0;
  const int c_lo = g * cpg, c_hi = c_lo + cpg;
#pragma unroll
  for (int si = 0; si < 4; ++si) {
    if (si >= sg.n) break;
    const CsGnSeg& sp = sg.s[si];
    const int lo = max(c_lo, sp.ch0), hi = min(c_hi, sp.ch0 + sp.nch);
    if (hi <= lo) continue;
    const int tps = sp.tiles_per_sample, nt = sp.ncls * tps, items = (hi - lo) * nt;
    const int64_t cls_stride = (int64_t)sp.nb_src * tps;
    const int64_t t0 = (int64_t)(n % sp.nb_src) * tps;
    // four items' loads in flight per lane (the plain loop waited out one load latency per item: 28 items a lane at the
    // 16-row partials of the split-K reduce = 9.6 us for a kernel that moves 30 KB); added in the same order as before
    for (int j = lane; j < items; j += 4 * nlanes) {
      double2 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int ju = j + u * nlanes;
        v[u] = make_double2(0.0, 0.0);
        if (ju < items) {
          const int k = ju / nt, r = ju - k * nt;           // channel lo + k, tile r = cls * tps + t
          const int cls = r / tps, t = r - cls * tps;
          v[u] = *reinterpret_cast<const double2*>(sp.part +
                                                   ((cls * cls_stride + t0 + t) * sp.ld + sp.col0 + (lo + k - sp.ch0)) * 2);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (j + u * nlanes < items) {
          s += v[u].x;
          q += v[u].y;
        }
    }
  }
}

// One word per tensor: the 2048 (sample, group)s of a 32-object launch each hitting it with an atomic serialise in L2
// (measured: 30 us for a kernel that otherwise takes 5), so a workgroup is SIXTEEN waves = sixteen (sample, group)s and
// commits one maximum.
constexpr int GN_FIN_WAVES = 16;
// WPG = waves per (sample, group).  r5: at one or two objects a group of the 16^3 level is 1792 (channel, tile) pairs of
// 16-row partials -- 28 dependent-latency rounds for ONE wave (15.9 us per launch, 27 launches per one-object step); with
// four waves per group the same kernel takes a third of that.  WPG is chosen from the pairs per group alone (a property of
// the sample's own partials, cs_groupnorm_finalize_parts), never from the batch: the summation tree of a sample does not
// depend on what else shares the launch.
template <int WPG>
__global__ __launch_bounds__(64 * GN_FIN_WAVES) void gn_finalize_parts_kernel(const GnSegs sg, int groups, int cpg,
                                                                              double count, float eps,
                                                                              float* __restrict__ stats,
                                                                              float* __restrict__ bound, int total) {
  constexpr int GPB = GN_FIN_WAVES / WPG;           // (sample, group)s per workgroup
  __shared__ float bmax[GN_FIN_WAVES];
  __shared__ double wsum[GN_FIN_WAVES][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slot = wave / WPG, sub = wave - slot * WPG;
  const int i = blockIdx.x * GPB + slot;  // n * groups + g
  float bf = 0.f;
  double s = 0, q = 0;
  if (i < total) {
    const int n = i / groups, g = i - n * groups;
    gn_group_parts(sg, n, g, cpg, sub * 64 + lane, 64 * WPG, s, q);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      s += __shfl_xor(s, o, 64);
      q += __shfl_xor(q, o, 64);
    }
  }
  if constexpr (WPG > 1) {
    if (lane == 0) {
      wsum[wave][0] = s;
      wsum[wave][1] = q;
    }
    __syncthreads();
    s = 0;
    q = 0;
#pragma unroll
    for (int w = 0; w < WPG; ++w) {               // fixed order over the group's waves
      s += wsum[slot * WPG + w][0];
      q += wsum[slot * WPG + w][1];
    }
  }
  if (i < total && sub == 0) {
    double mean, var;
    float rstd;
    gn_moments(s, q, count, eps, mean, var, rstd);
    if (lane == 0 && stats) {
      stats[2 * i] = (float)mean;
      stats[2 * i + 1] = rstd;
    }
    if (bound) bf = gn_bound_value(mean, var, count);
  }
  if (!bound) return;                  // (kernel-uniform)
  if (lane == 0) bmax[wave] = bf;
  __syncthreads();
  if (threadIdx.x == 0) {
    float m = bmax[0];
#pragma unroll
    for (int w = 1; w < GN_FIN_WAVES; ++w) m = fmaxf(m, bmax[w]);
    gn_bound_commit(bound, m);
  }
}

// What a thread of the apply kernels keeps for its V channels, loaded once: the affine parameters and the statistics of each
// channel's group.  The c channels handled are channels ch0 .. ch0 + c of the normalised tensor -- x, gamma and beta already
// point at channel ch0 -- so the thread's channel col + k belongs to group (ch0 + col + k) / cpg; `st` = the sample's
// [groups][2] (mean, rstd).
template <int V>
struct GnCols {
  float g[V], b[V], mean[V], rstd[V];
  __device__ __forceinline__ GnCols(const float* __restrict__ gamma, const float* __restrict__ beta,
                                    const float* __restrict__ st, int ch0, int cpg, int col) {
#pragma unroll
    for (int k4 = 0; k4 < V / 4; ++k4) {
      const float4 gv = *reinterpret_cast<const float4*>(gamma + col + 4 * k4);
      const float4 bv = *reinterpret_cast<const float4*>(beta + col + 4 * k4);
      g[4 * k4] = gv.x; g[4 * k4 + 1] = gv.y; g[4 * k4 + 2] = gv.z; g[4 * k4 + 3] = gv.w;
      b[4 * k4] = bv.x; b[4 * k4 + 1] = bv.y; b[4 * k4 + 2] = bv.z; b[4 * k4 + 3] = bv.w;
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const int grp = (ch0 + col + k) / cpg;
      mean[k] = st[grp * 2];
      rstd[k] = st[grp * 2 + 1];
    }
  }
  // THE expression of every GroupNorm apply: channel k of the thread's column
  __device__ __forceinline__ float norm(float in, int k, int act) const {
    return cs_act((in - mean[k]) * rstd[k] * g[k] + b[k], act);
  }
  // the V channels at px, normalised and scaled (the operand scale is applied after the activation)
  __device__ __forceinline__ void norm_scaled(const float* __restrict__ px, int act, float a_scale, float (&o)[V]) const {
#pragma unroll
    for (int k4 = 0; k4 < V / 4; ++k4) {
      const float4 v = *reinterpret_cast<const float4*>(px + 4 * k4);
      const float iv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) o[4 * k4 + k] = norm(iv[k], 4 * k4 + k, act) * a_scale;
    }
  }
};

// One workgroup = a run of rows of ONE sample; a thread keeps its float4 column for the whole run, so the group
// statistics and the affine parameters of its four channels are loaded once and the row loop has no index
// arithmetic beyond a pointer bump (the previous flat element loop -- in both output forms, two 64-bit divisions per
// float4 -- ran at ~45 % of the HBM rate).  Four rows' loads are in flight per thread.
// (`groups` = row length of `stats`.)  put(off, o) stores the four normalised channels o of the sample's output element
// at off = row ldy + column: the ONE difference between the two kernels below.
template <class Put>
__device__ __forceinline__ void gn_apply_rows(const float* __restrict__ x, const float* __restrict__ stats,
                                              const float* __restrict__ gamma, const float* __restrict__ beta, int rows,
                                              int c, int ldx, int ldy, int groups, int act, int rows_per_block, int cpg,
                                              int ch0, Put put) {
  const int ch4 = c >> 2;
  const int tpr = gn_map(ch4).tpr, rowlanes = gn_map(ch4).lanes;
  const int tid = threadIdx.x;
  const int rl = tid / tpr;
  const int cl = tid - rl * tpr;
  if (rl >= rowlanes) return;
  const int n = blockIdx.y;
  const int r0 = blockIdx.x * rows_per_block;
  const int r1 = min(rows, r0 + rows_per_block);
  const float* xb = x + (int64_t)n * rows * ldx;
  const float* st = stats + (int64_t)n * groups * 2;
  for (int c4 = cl; c4 < ch4; c4 += tpr) {
    const GnCols<4> cols(gamma, beta, st, ch0, cpg, c4 * 4);
    for (int r = r0 + rl; r < r1; r += 4 * rowlanes) {
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int rr = r + u * rowlanes;
        if (rr < r1) v[u] = *reinterpret_cast<const float4*>(xb + (int64_t)rr * ldx + c4 * 4);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int rr = r + u * rowlanes;
        if (rr < r1) {
          const float in[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
          float o[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) o[k] = cols.norm(in[k], k, act);
          put((int64_t)rr * ldy + c4 * 4, o);
        }
      }
    }
  }
}

// fp32 output
__global__ __launch_bounds__(256) void gn_apply_kernel(const float* __restrict__ x,
                                                       const float* __restrict__ stats,
                                                       const float* __restrict__ gamma,
                                                       const float* __restrict__ beta,
                                                       float* __restrict__ y, int rows, int c, int ldx, int ldy,
                                                       int groups, int act, int rows_per_block, int cpg, int ch0) {
  float* yb = y + (int64_t)blockIdx.y * rows * ldy;
  gn_apply_rows(x, stats, gamma, beta, rows, c, ldx, ldy, groups, act, rows_per_block, cpg, ch0,
                [&](int64_t off, const float (&o)[4]) {
                  *reinterpret_cast<float4*>(yb + off) = make_float4(o[0], o[1], o[2], o[3]);
                });
}

// GroupNorm apply emitting the fp16 hi / lo pair of y * a_scale (A operand of the F16X3 GEMMs): the fp32 -> pair
// split costs nothing here (this kernel is HBM-bound) and is then done once per element instead of once per
// conv tap inside the GEMM.  Output bytes equal the fp32 version (2 + 2 per element).
__global__ __launch_bounds__(256) void gn_apply_split16_kernel(const float* __restrict__ x,
                                                               const float* __restrict__ stats,
                                                               const float* __restrict__ gamma,
                                                               const float* __restrict__ beta,
                                                               _Float16* __restrict__ yh, _Float16* __restrict__ yl,
                                                               int rows, int c, int ldx, int ldy, int groups,
                                                               int act, float a_scale, int rows_per_block,
                                                               int32_t* __restrict__ status, int cpg, int ch0) {
  _Float16* hb = yh + (int64_t)blockIdx.y * rows * ldy;
  _Float16* lb = yl + (int64_t)blockIdx.y * rows * ldy;
  float amax = 0.f;
  gn_apply_rows(x, stats, gamma, beta, rows, c, ldx, ldy, groups, act, rows_per_block, cpg, ch0,
                [&](int64_t off, const float (&o)[4]) {
                  const float os[4] = {o[0] * a_scale, o[1] * a_scale, o[2] * a_scale, o[3] * a_scale};
                  cs_hv<4> hi, lo;
                  cs_pair_split<4>(os, hi, lo, amax);
                  *reinterpret_cast<cs_hv<4>*>(hb + off) = hi;
                  *reinterpret_cast<cs_hv<4>*>(lb + off) = lo;
                });
  cs_pair_amax_flag(status, amax);
}

// Image q of the Winograd transform B^T d along W, channel k of the thread's column; d_j = y[VAR t - 1 + j] of tile t (0
// outside the line).  F(2,3): [d0 - d2, d1 + d2, d2 - d1, d1 - d3].
template <int VAR, int V>
__device__ __forceinline__ float gn_wino_bt(const float (&d)[VAR + 2][V], int q, int k) {
  if constexpr (VAR == 2) {
    return q == 0 ? d[0][k] - d[2][k] : q == 1 ? d[1][k] + d[2][k] : q == 2 ? d[2][k] - d[1][k] : d[1][k] - d[3][k];
  } else {
    if (q == 0) return 4.f * d[0][k] - 5.f * d[2][k] + d[4][k];
    if (q == 1) return (d[4][k] + d[3][k]) - 4.f * (d[1][k] + d[2][k]);
    if (q == 2) return 4.f * (d[1][k] - d[2][k]) + (d[4][k] - d[3][k]);
    if (q == 3) return 2.f * (d[3][k] - d[1][k]) + (d[4][k] - d[2][k]);
    if (q == 4) return 2.f * (d[1][k] - d[3][k]) + (d[4][k] - d[2][k]);
    return 4.f * d[1][k] - 5.f * d[3][k] + d[5][k];
  }
}

// r5: GroupNorm + activation emitted in the WINOGRAD-W form of the 3x3x3 conv that follows: per W line of a sample and tile of
// VAR voxels (w = VAR t .. VAR t + VAR - 1) the VAR + 2 transformed values B^T d (gn_wino_bt), split into fp16 hi / lo of
// value * a_scale -- images [VAR + 2][nb][lines][W / VAR][ldv].  VAR = 2: F(2,3), CsConvGemm.a_format = 3; VAR = 4: F(4,3),
// a_format = 4.  A thread keeps its column of V channels and walks whole lines: every activation is evaluated once (a tile's
// last two d are the next tile's d0, d1).  w % VAR == 0 (the entry checks it), so only the LAST d of a tile can lie past the
// line.
// (V = channels per thread.  r6 measured V = 8 for F(4,3) -- two float4 loads, ONE 16-byte store per image and position
// instead of two 8-byte ones -- and it LOST: 80.7 vs 61.3 us per launch, 64.63 vs 64.00 ms per 32-object step same box
// (profiles/r06_j_gn_wino_v8_whatif_ab.txt): half the threads in flight cost more than the wider stores gain.  V = 4 stays;
// -DCS_GN_WINO_V8 is the what-if build.  Same arithmetic per element either way.)
template <int VAR, int V>
__global__ __launch_bounds__(256) void gn_apply_wino_kernel(const float* __restrict__ x, const float* __restrict__ stats,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            _Float16* __restrict__ vh, _Float16* __restrict__ vl, int lines,
                                                            int w, int c, int ldx, int ldv, int groups, int act,
                                                            float a_scale, int lines_per_block, int64_t pos_stride,
                                                            int32_t* __restrict__ status, int cpg, int ch0) {
  const int chv = c / V;
  const int tpr = gn_map(chv).tpr, linelanes = gn_map(chv).lanes;
  const int tid = threadIdx.x;
  const int ll = tid / tpr;
  const int cl = tid - ll * tpr;
  if (ll >= linelanes) return;
  const int n = blockIdx.y;
  const int l0 = blockIdx.x * lines_per_block;
  const int l1 = min(lines, l0 + lines_per_block);
  const int wtn = (int)((unsigned)w / VAR);      // tiles per line (w > 0: a shift)
  const float* xb = x + (int64_t)n * lines * w * ldx;
  const int64_t vrow0 = (int64_t)n * lines * wtn;
  const float* st = stats + (int64_t)n * groups * 2;
  float amax = 0.f;
  for (int cv = cl; cv < chv; cv += tpr) {
    const GnCols<V> cols(gamma, beta, st, ch0, cpg, cv * V);
    for (int line = l0 + ll; line < l1; line += linelanes) {
      const float* xl = xb + (int64_t)line * w * ldx + cv * V;
      float d[VAR + 2][V];
#pragma unroll
      for (int k = 0; k < V; ++k) d[0][k] = 0.f;
      cols.norm_scaled(xl, act, a_scale, d[1]);
      for (int t = 0; t < wtn; ++t) {
#pragma unroll
        for (int j = 2; j < VAR + 2; ++j) {
          const int wi = VAR * t - 1 + j;
          if (j <= VAR || wi < w) {
            cols.norm_scaled(xl + (int64_t)wi * ldx, act, a_scale, d[j]);
          } else {
#pragma unroll
            for (int k = 0; k < V; ++k) d[j][k] = 0.f;
          }
        }
        const int64_t off = (vrow0 + (int64_t)line * wtn + t) * ldv + cv * V;
#pragma unroll
        for (int q = 0; q < VAR + 2; ++q) {
          float o[V];
#pragma unroll
          for (int k = 0; k < V; ++k) o[k] = gn_wino_bt<VAR, V>(d, q, k);
          cs_hv<V> hi, lo;
          cs_pair_split<V>(o, hi, lo, amax);
          *reinterpret_cast<cs_hv<V>*>(vh + q * pos_stride + off) = hi;
          *reinterpret_cast<cs_hv<V>*>(vl + q * pos_stride + off) = lo;
        }
#pragma unroll
        for (int k = 0; k < V; ++k) {
          d[0][k] = d[VAR][k];
          d[1][k] = d[VAR + 1][k];
        }
      }
    }
  }
  cs_pair_amax_flag(status, amax);
}

// LayerNorm: one wave per row; each lane owns up to MAXV float4 chunks (c <= 64*4*MAXV).
template <int MAXV>
__global__ __launch_bounds__(256) void ln_kernel(const float* __restrict__ x,
                                                 const float* __restrict__ gamma,
                                                 const float* __restrict__ beta,
                                                 float* __restrict__ y, int m, int c, int ldx,
                                                 int ldy, float eps) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int ch4 = c >> 2;
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < m; row += (int64_t)gridDim.x * 4) {
    float4 v[MAXV];
    const float s = cs_ln_load_row<MAXV>(x, row, ldx, lane, ch4, v);
    float mean, rstd;
    cs_ln_row_stats<MAXV>(v, s, lane, ch4, c, eps, mean, rstd);
#pragma unroll
    for (int k = 0; k < MAXV; ++k) {
      const int c4 = lane + 64 * k;
      if (c4 < ch4) {
        const float4 g = *reinterpret_cast<const float4*>(gamma + c4 * 4);
        const float4 b = *reinterpret_cast<const float4*>(beta + c4 * 4);
        float4 o;
        o.x = (v[k].x - mean) * rstd * g.x + b.x;
        o.y = (v[k].y - mean) * rstd * g.y + b.y;
        o.z = (v[k].z - mean) * rstd * g.z + b.z;
        o.w = (v[k].w - mean) * rstd * g.w + b.w;
        *reinterpret_cast<float4*>(y + row * ldy + c4 * 4) = o;
      }
    }
  }
}

// LayerNorm emitting the interleaved F16X3 operand pair (CsConvGemm.a_format = 2): per row and 16-channel chunk the 64
// bytes [hi c0-7 | lo c0-7 | hi c8-15 | lo c8-15], halves of y * a_scale -- same bytes and row stride as the fp32 output
// it replaces, so the consuming GEMM gathers the same 64-byte pieces and its K loop carries no conversion.
template <int MAXV>
__global__ __launch_bounds__(256) void ln_pair_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, _Float16* __restrict__ y, int m,
                                                      int c, int ldx, int ldy, float eps, float a_scale,
                                                      int32_t* __restrict__ status) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int ch4 = c >> 2;
  float amax = 0.f;
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < m; row += (int64_t)gridDim.x * 4) {
    float4 v[MAXV];
    const float s = cs_ln_load_row<MAXV>(x, row, ldx, lane, ch4, v);
    amax = cs_ln_pair_row<MAXV>(v, s, lane, ch4, c, gamma, beta, y + row * (int64_t)ldy * 2, eps, a_scale, amax);
  }
  cs_pair_amax_flag(status, amax);
}

// What the two one-launch kernels share: a workgroup of 256 per (sample, group), or per row share of one.
// The fixed LDS tree over the workgroup's 256 (s, q): every thread leaves with the totals, so they are reproducible.
__device__ __forceinline__ void gn_block_sum(double& s, double& q) {
  __shared__ double red[2][256];
  const int tid = threadIdx.x;
  red[0][tid] = s;
  red[1][tid] = q;
  __syncthreads();
#pragma unroll
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      red[0][tid] += red[0][tid + o];
      red[1][tid] += red[1][tid + o];
    }
    __syncthreads();
  }
  s = red[0][0];
  q = red[1][0];
}
// The walk over a group's rows x cpg elements, 256 apart: element index + 256  ->  (row + dr, k + dk) with carry
struct GnWalk {
  int cpg, dr, dk;
  __device__ __forceinline__ explicit GnWalk(int cpg_) : cpg(cpg_), dr(256 / cpg_), dk(256 - dr * cpg_) {}
  __device__ __forceinline__ void next(int& r, int& k) const {
    r += dr;
    k += dk;
    if (k >= cpg) {
      k -= cpg;
      ++r;
    }
  }
};
// The apply sweep over rows [rbeg, rend) of the group at xb / yb (gamma, beta at the group's first channel): four loads in
// flight, the same expression as gn_apply_kernel
__device__ __forceinline__ void gn_small_apply(const float* __restrict__ xb, float* __restrict__ yb,
                                               const float* __restrict__ gamma, const float* __restrict__ beta, int rbeg,
                                               int rend, const GnWalk wk, int ldx, int ldy, float mean, float rstd, int act) {
  const int tid = threadIdx.x;
  int r = rbeg + tid / wk.cpg, k = tid - (tid / wk.cpg) * wk.cpg;
  while (r < rend) {
    float v[4], ga[4], be[4];
    int rr[4], kk[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      rr[u] = r;
      kk[u] = k;
      if (r < rend) {
        v[u] = xb[(int64_t)r * ldx + k];
        ga[u] = gamma[k];
        be[u] = beta[k];
      }
      wk.next(r, k);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (rr[u] < rend) yb[(int64_t)rr[u] * ldy + kk[u]] = cs_act((v[u] - mean) * rstd * ga[u] + be[u], act);
  }
}

// Small tensors (one or two objects: a few MB, L2-resident): statistics and normalisation in ONE launch, one workgroup
// per (sample, group).  The three-launch path costs ~23 us per GroupNorm there (6.8 + 4.6 + 11.5 us, each at its launch
// floor), 61 times a step.  Threads walk the group's rows x cpg elements in a fixed stride, accumulate in fp64, and a
// fixed LDS tree adds the 256 partials, so the statistics are reproducible; the second sweep re-reads the group from
// L2 and applies the same expression as gn_apply_kernel.
__global__ __launch_bounds__(256) void gn_small_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, float* __restrict__ y,
                                                       float* __restrict__ stats, int rows, int c, int ldx, int ldy,
                                                       int groups, float eps, int act) {
  const int n = blockIdx.x / groups, g = blockIdx.x - n * groups;
  const int cpg = c / groups;
  const int tid = threadIdx.x;
  const float* xb = x + (int64_t)n * rows * ldx + g * cpg;
  float* yb = y + (int64_t)n * rows * ldy + g * cpg;
  const GnWalk wk(cpg);
  double s = 0, q = 0;
  {
    int r = tid / cpg, k = tid - r * cpg;
    while (r < rows) {                                      // four loads in flight, accumulated in element order
      float v[4];
      int rr[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        rr[u] = r;
        v[u] = r < rows ? xb[(int64_t)r * ldx + k] : 0.f;
        wk.next(r, k);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (rr[u] < rows) {
          s += v[u];
          q += (double)v[u] * v[u];
        }
    }
  }
  gn_block_sum(s, q);
  double mean_d, var;
  float rstd;
  gn_moments(s, q, (double)rows * cpg, eps, mean_d, var, rstd);
  const float mean = (float)mean_d;
  if (tid == 0 && stats) {
    stats[2 * blockIdx.x] = mean;
    stats[2 * blockIdx.x + 1] = rstd;
  }
  gn_small_apply(xb, yb, gamma + g * cpg, beta + g * cpg, 0, rows, wk, ldx, ldy, mean, rstd, act);
}

// gn_small_kernel with the statistics taken from the producers' partials (r4): one workgroup per (sample, group) adds the
// group's partial sums (256 threads over the (channel, tile) pairs, fixed LDS tree) and makes ONE sweep over the group.
// Small tensors only (the gn_small rule): one launch per GroupNorm where the two-launch form would sit at its launch floors.
__global__ __launch_bounds__(256) void gn_small_parts_kernel(const float* __restrict__ x, const GnSegs sg,
                                                             const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float* __restrict__ y,
                                                             float* __restrict__ stats, float* __restrict__ bound, int rows,
                                                             int c, int ldx, int ldy, int groups, float eps, int act,
                                                             int rsplit) {
  // r5: `rsplit` workgroups per (sample, group), each deriving the SAME statistics from the partials (a few hundred pairs)
  // and sweeping its share of the rows -- one or two objects are 64 (sample, group)s, a quarter of the CUs
  const int sgi = blockIdx.x / rsplit, rs = blockIdx.x - sgi * rsplit;
  const int n = sgi / groups, g = sgi - n * groups;
  const int cpg = c / groups;
  const int tid = threadIdx.x;
  double s, q;
  gn_group_parts(sg, n, g, cpg, tid, 256, s, q);
  gn_block_sum(s, q);
  const double count = (double)rows * cpg;
  double mean_d, var;
  float rstd;
  gn_moments(s, q, count, eps, mean_d, var, rstd);
  const float mean = (float)mean_d;
  if (tid == 0 && stats && rs == 0) {
    stats[2 * sgi] = mean;
    stats[2 * sgi + 1] = rstd;
  }
  if (tid == 0 && bound && rs == 0) gn_bound_max(bound, mean_d, var, count);
  const int rper = (rows + rsplit - 1) / rsplit;
  const int rbeg = rs * rper, rend = min(rows, rbeg + rper);
  gn_small_apply(x + (int64_t)n * rows * ldx + g * cpg, y + (int64_t)n * rows * ldy + g * cpg, gamma + g * cpg,
                 beta + g * cpg, rbeg, rend, GnWalk(cpg), ldx, ldy, mean, rstd, act);
}

// row slices per sample: enough workgroups to fill the chip (~2048 in total) but no slice shorter than
// GN_MIN_SPLIT_ROWS rows (each workgroup ends in a serial LDS reduction that longer slices amortise)
int gn_nsplit(int rows, int nb) {
  int n = (2048 + nb - 1) / nb;
  const int cap = (rows + GN_MIN_SPLIT_ROWS - 1) / GN_MIN_SPLIT_ROWS;
  if (n > cap) n = cap;
  if (n < 1) n = 1;
  return n < GN_MAX_SPLITS ? n : GN_MAX_SPLITS;
}

// rows per workgroup of gn_apply_kernel / gn_apply_split16_kernel: enough workgroups to fill the chip (>= ~2048 in total), each with at least 16 rows
// per row-lane
int gn_rows_per_block(int nb, int rows, int rowlanes) {
  int blocks_per_sample = (2048 + nb - 1) / nb;
  // (r5: down to four rows per row-lane -- one round of the kernel's four loads in flight -- where sixteen would leave
  // most of the chip idle: 8192 x 224 at one object ran 128 workgroups x 4 dependent rounds, 12 us for 14 MB)
  const int min_rows = (int64_t)nb * ((rows + 16 * rowlanes - 1) / (16 * rowlanes)) >= 1024 ? 16 : 4;
  const int max_blocks = (rows + min_rows * rowlanes - 1) / (min_rows * rowlanes);
  if (blocks_per_sample > max_blocks) blocks_per_sample = max_blocks;
  if (blocks_per_sample < 1) blocks_per_sample = 1;
  return (rows + blocks_per_sample - 1) / blocks_per_sample;
}

// one launch (gn_small_kernel / gn_small_parts_kernel) while the tensor is a few MB (it stays in L2 between the two sweeps)
// and a group is a handful of elements per thread; otherwise statistics + apply
bool gn_one_launch(int nb, int rows, int c, int groups) {
  const int cpg = c / groups;
  const int64_t small_group = cs_debug()->gn_small_group;      // (CS_GN_SMALL_GROUP: tuning override, tools/gn_bench.py)
  return (int64_t)nb * rows * c * 4 <= GN_SMALL_BYTES && cpg <= 256 && (int64_t)rows * cpg <= small_group &&
         (int64_t)nb * groups <= 65535;
}

// What the three channel-range apply entries ask of their arguments (`rows` = any of the row-count arguments already folded
// by the caller: all must be positive).  The fp32 form has float4 accesses only (cgran = ldgran = 4, y1 = y0, no scale); the
// pair forms store eight-byte halves of 8-channel operand rows (8, 8) and scale by a_scale > 0.
bool gn_apply_args_ok(const void* x, const void* stats, const void* gamma, const void* beta, const void* y0,
                      const void* y1, int nb, int c, int ldx, int ldy, int groups, int cpg, int ch0, int cgran,
                      int ldgran, bool scaled, float a_scale) {
  if (!x || !stats || !gamma || !beta || !y0 || !y1 || nb <= 0 || nb > 65535 || c <= 0 || groups <= 0 || cpg <= 0 ||
      ch0 < 0)
    return false;
  if ((c & (cgran - 1)) || (ldx & 3) || (ldy & (ldgran - 1)) || ldx < c || ldy < c ||
      (int64_t)ch0 + c > (int64_t)groups * cpg || (scaled && !(a_scale > 0.f)))
    return false;
  return !(((uintptr_t)x & 15) || ((uintptr_t)y0 & 15) || ((uintptr_t)y1 & 15) || ((uintptr_t)gamma & 15) ||
           ((uintptr_t)beta & 15));
}

}  // namespace

extern "C" int64_t cs_groupnorm_ws_bytes(int nb, int groups) {
  return (int64_t)nb * GN_MAX_SPLITS * groups * 2 * (int64_t)sizeof(double);
}

static int gn_pack_segs(const CsGnSeg* segs, int nseg, int nb, int c, GnSegs& sg) {
  if (!segs || nseg < 1 || nseg > 4) return CS_EINVAL;
  sg.n = nseg;
  int next = 0;
  for (int i = 0; i < nseg; ++i) {
    const CsGnSeg& s = segs[i];
    // contiguous cover of [0, c) in channel order; every tile index the kernel forms must exist
    if (!s.part || ((uintptr_t)s.part & 15) || s.ch0 != next || s.nch <= 0 || s.col0 < 0 || s.col0 + s.nch > s.ld ||
        s.tiles_per_sample <= 0 || s.ncls <= 0 || s.nb_src <= 0 || (nb % s.nb_src) != 0)
      return CS_EINVAL;
    next += s.nch;
    sg.s[i] = s;
  }
  if (next != c) return CS_EINVAL;
  for (int i = nseg; i < 4; ++i) sg.s[i] = segs[0];
  return CS_OK;
}

extern "C" int cs_groupnorm_finalize_parts(const CsGnSeg* segs, int nseg, int nb, int rows, int c, int groups, float eps,
                                           float* stats, float* bound, cs_stream_t stream) {
  if ((!stats && !bound) || ((uintptr_t)bound & 3) || nb <= 0 || rows <= 0 || c <= 0 || groups <= 0 || c % groups) return CS_EINVAL;
  GnSegs sg;
  const int rc = gn_pack_segs(segs, nseg, nb, c, sg);
  if (rc != CS_OK) return rc;
  const int total = nb * groups;
  // (channel, tile) pairs of the largest group share: four waves per group from 512 pairs (see the kernel)
  int64_t pairs = 0;
  for (int i = 0; i < nseg; ++i) {
    const int64_t nt = (int64_t)segs[i].ncls * segs[i].tiles_per_sample;
    const int64_t chs = segs[i].nch < c / groups ? segs[i].nch : c / groups;
    if (nt * chs > pairs) pairs = nt * chs;
  }
  if (pairs >= 512 && !cs_debug()->no_gn_fold) {
    CS_LAUNCH(gn_finalize_parts_kernel<4>, dim3((total + 3) / 4), dim3(64 * GN_FIN_WAVES), 0, (hipStream_t)stream, sg, groups,
              c / groups, (double)rows * (c / groups), eps, stats, bound, total);
  } else {
    CS_LAUNCH(gn_finalize_parts_kernel<1>, dim3((total + GN_FIN_WAVES - 1) / GN_FIN_WAVES), dim3(64 * GN_FIN_WAVES), 0,
              (hipStream_t)stream, sg, groups, c / groups, (double)rows * (c / groups), eps, stats, bound, total);
  }
  CS_CHECK_LAUNCH();
  return CS_OK;
}

// GroupNorm of a tensor whose statistics come from its producers' partials, in ONE call: a single launch for small
// tensors (the cs_groupnorm rule: <= 16 MB, <= 11264 elements per (sample, group)), cs_groupnorm_finalize_parts +
// cs_groupnorm_apply otherwise.  `stats` [nb][groups][2] is written either way.
extern "C" int cs_groupnorm_parts(const float* x, const CsGnSeg* segs, int nseg, const float* gamma, const float* beta,
                                  float* y, int nb, int rows, int c, int ldx, int ldy, int groups, float eps, int act,
                                  float* stats, float* bound, cs_stream_t stream) {
  if (!x || !gamma || !beta || !y || !stats || ((uintptr_t)bound & 3) || nb <= 0 || rows <= 0 || c <= 0 || groups <= 0 || c % groups || ldx < c ||
      ldy < c)
    return CS_EINVAL;
  GnSegs sg;
  const int rc0 = gn_pack_segs(segs, nseg, nb, c, sg);
  if (rc0 != CS_OK) return rc0;
  const int cpg = c / groups;
  if (gn_one_launch(nb, rows, c, groups)) {
    // (row shares per (sample, group): up to four while the launch stays under ~512 workgroups and a share keeps >= 4
    // elements per thread; depends on the sample's own shape and on nb only through the workgroup budget -- the
    // arithmetic per element does not depend on it)
    int rsplit = 1;
    while (rsplit < 4 && (int64_t)nb * groups * rsplit * 2 <= 512 && (int64_t)rows * cpg >= 2048LL * rsplit) rsplit *= 2;
    if (cs_debug()->no_gn_fold) rsplit = 1;
    CS_LAUNCH(gn_small_parts_kernel, dim3((unsigned)(nb * groups * rsplit)), dim3(256), 0, (hipStream_t)stream, x, sg, gamma,
              beta, y, stats, bound, rows, c, ldx, ldy, groups, eps, act, rsplit);
    CS_CHECK_LAUNCH();
    return CS_OK;
  }
  // what cs_groupnorm_apply (float4 accesses) will ask for, checked BEFORE the finalize launch: a call that is turned down
  // has written nothing (c % 4 != 0 used to leave stats and bound behind and then return CS_EINVAL)
  if (!gn_apply_args_ok(x, stats, gamma, beta, y, y, nb, c, ldx, ldy, groups, cpg, 0, 4, 4, false, 0.f)) return CS_EINVAL;
  const int rc = cs_groupnorm_finalize_parts(segs, nseg, nb, rows, c, groups, eps, stats, bound, stream);
  if (rc) return rc;
  return cs_groupnorm_apply(x, stats, gamma, beta, y, nb, rows, c, ldx, ldy, groups, act, stream);
}

static int gn_stats_impl(const float* x, int nb, int rows, int c, int ldx, int groups, float eps, void* ws, float* stats,
                         float* bound, cs_stream_t stream) {
  if (!x || !ws || !stats || nb <= 0 || rows <= 0 || c <= 0 || groups <= 0) return CS_EINVAL;
  if ((c & 3) || (ldx & 3) || ldx < c || c % groups || groups > 256) return CS_EINVAL;
  if (((uintptr_t)x & 15) || ((uintptr_t)ws & 7)) return CS_EINVAL;
  const int nsplit = gn_nsplit(rows, nb);
  const int rps = (rows + nsplit - 1) / nsplit;
  const size_t smem = (size_t)gn_map(c >> 2).lanes * c * 2 * sizeof(double);
  if (smem > 64 * 1024) return CS_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  CS_LAUNCH(gn_partial_kernel, dim3((unsigned)(nb * nsplit)), dim3(256), smem, s, x, rows,
                     c, ldx, groups, nsplit, rps, (double*)ws);
  CS_CHECK_LAUNCH();
  const int total = nb * groups;
  CS_LAUNCH(gn_finalize_kernel, dim3((total + 3) / 4), dim3(256), 0, s,
                     (const double*)ws, nsplit, groups, (double)rows * (c / groups), eps, stats,
                     total, bound);
  CS_CHECK_LAUNCH();
  return CS_OK;
}

extern "C" int cs_groupnorm_stats(const float* x, int nb, int rows, int c, int ldx, int groups,
                                  float eps, void* ws, float* stats, cs_stream_t stream) {
  return gn_stats_impl(x, nb, rows, c, ldx, groups, eps, ws, stats, nullptr, stream);
}

// cs_groupnorm_stats that also leaves the tensor's magnitude bound (max over (sample, group) of |mean| + std sqrt(n - 1),
// see cs_groupnorm_finalize_parts) in `bound`: for a tensor whose producers left no partial sums (r4)
extern "C" int cs_groupnorm_stats_bound(const float* x, int nb, int rows, int c, int ldx, int groups, float eps, void* ws,
                                        float* stats, float* bound, cs_stream_t stream) {
  if (!bound || ((uintptr_t)bound & 3)) return CS_EINVAL;
  return gn_stats_impl(x, nb, rows, c, ldx, groups, eps, ws, stats, bound, stream);
}

// Channel-range form of the apply entries: the c channels handled are channels ch0 .. ch0 + c of a tensor that was
// normalised over `groups` groups of `cpg` channels each (stats: [nb][groups][2]); x, gamma, beta and y point AT channel
// ch0.  Lets one statistics pass over a concatenated tensor [h | skip] feed two separate operand tensors (the channel
// split of the classifier-free-guidance output blocks, unet.py::_res_split).
extern "C" int cs_groupnorm_apply_range(const float* x, const float* stats, const float* gamma, const float* beta,
                                        float* y, int nb, int rows, int c, int ldx, int ldy, int groups, int cpg,
                                        int ch0, int act, cs_stream_t stream) {
  if (rows <= 0 || !gn_apply_args_ok(x, stats, gamma, beta, y, y, nb, c, ldx, ldy, groups, cpg, ch0, 4, 4, false, 0.f))
    return CS_EINVAL;
  const int rpb = gn_rows_per_block(nb, rows, gn_map(c >> 2).lanes);
  CS_LAUNCH(gn_apply_kernel, dim3((unsigned)((rows + rpb - 1) / rpb), (unsigned)nb), dim3(256), 0,
            (hipStream_t)stream, x, stats, gamma, beta, y, rows, c, ldx, ldy, groups, act, rpb, cpg, ch0);
  CS_CHECK_LAUNCH();
  return CS_OK;
}

extern "C" int cs_groupnorm_apply(const float* x, const float* stats, const float* gamma,
                                  const float* beta, float* y, int nb, int rows, int c, int ldx,
                                  int ldy, int groups, int act, cs_stream_t stream) {
  if (groups <= 0 || c <= 0 || c % groups) return CS_EINVAL;
  return cs_groupnorm_apply_range(x, stats, gamma, beta, y, nb, rows, c, ldx, ldy, groups, c / groups, 0, act, stream);
}

extern "C" int cs_groupnorm_apply_split16_range(const float* x, const float* stats, const float* gamma,
                                                const float* beta, void* y_hi, void* y_lo, int nb, int rows, int c,
                                                int ldx, int ldy, int groups, int cpg, int ch0, int act, float a_scale,
                                                int32_t* status, cs_stream_t stream) {
  if (rows <= 0 ||
      !gn_apply_args_ok(x, stats, gamma, beta, y_hi, y_lo, nb, c, ldx, ldy, groups, cpg, ch0, 8, 8, true, a_scale))
    return CS_EINVAL;
  const int rpb = gn_rows_per_block(nb, rows, gn_map(c >> 2).lanes);
  CS_LAUNCH(gn_apply_split16_kernel, dim3((unsigned)((rows + rpb - 1) / rpb), (unsigned)nb), dim3(256), 0,
            (hipStream_t)stream, x, stats, gamma, beta, (_Float16*)y_hi, (_Float16*)y_lo, rows, c, ldx, ldy, groups, act,
            a_scale, rpb, status, cpg, ch0);
  CS_CHECK_LAUNCH();
  return CS_OK;
}

extern "C" int cs_groupnorm_apply_wino_range(const float* x, const float* stats, const float* gamma, const float* beta,
                                             void* v_hi, void* v_lo, int nb, int d, int h, int w, int c, int ldx, int ldv,
                                             int groups, int cpg, int ch0, int act, float a_scale, int variant,
                                             int32_t* status, cs_stream_t stream) {
  if (d <= 0 || h <= 0 || w < 2 || (variant != 2 && variant != 4) || (w % variant) ||
      !gn_apply_args_ok(x, stats, gamma, beta, v_hi, v_lo, nb, c, ldx, ldv, groups, cpg, ch0, 8, 8, true, a_scale))
    return CS_EINVAL;
  const int64_t lines64 = (int64_t)d * h;
  if (lines64 * w > 0x7fffffffLL) return CS_EINVAL;
  const int lines = (int)lines64;
#ifdef CS_GN_WINO_V8           // what-if build: eight channels per thread (one 16-byte store per image and position)
  constexpr int WV = 8;
#else
  constexpr int WV = 4;            // channels per thread of the F(4,3) kernel
#endif
  const int linelanes = gn_map(variant == 4 ? c / WV : c >> 2).lanes;
  // ~2048 workgroups in all, at least one line per line-lane
  int blocks_per_sample = (2048 + nb - 1) / nb;
  const int max_blocks = (lines + linelanes - 1) / linelanes;
  if (blocks_per_sample > max_blocks) blocks_per_sample = max_blocks;
  if (blocks_per_sample < 1) blocks_per_sample = 1;
  const int lpb = (lines + blocks_per_sample - 1) / blocks_per_sample;
  const int64_t pos_stride = (int64_t)nb * lines * (w / variant) * ldv;
  if (variant == 4) {
    CS_LAUNCH((gn_apply_wino_kernel<4, WV>), dim3((unsigned)((lines + lpb - 1) / lpb), (unsigned)nb), dim3(256), 0,
              (hipStream_t)stream, x, stats, gamma, beta, (_Float16*)v_hi, (_Float16*)v_lo, lines, w, c, ldx, ldv, groups, act,
              a_scale, lpb, pos_stride, status, cpg, ch0);
  } else {
    CS_LAUNCH((gn_apply_wino_kernel<2, 4>), dim3((unsigned)((lines + lpb - 1) / lpb), (unsigned)nb), dim3(256), 0,
              (hipStream_t)stream, x, stats, gamma, beta, (_Float16*)v_hi, (_Float16*)v_lo, lines, w, c, ldx, ldv, groups, act,
              a_scale, lpb, pos_stride, status, cpg, ch0);
  }
  CS_CHECK_LAUNCH();
  return CS_OK;
}

extern "C" int cs_groupnorm_apply_wino16_range(const float* x, const float* stats, const float* gamma, const float* beta,
                                               void* v_hi, void* v_lo, int nb, int d, int h, int w, int c, int ldx, int ldv,
                                               int groups, int cpg, int ch0, int act, float a_scale, int32_t* status,
                                               cs_stream_t stream) {
  return cs_groupnorm_apply_wino_range(x, stats, gamma, beta, v_hi, v_lo, nb, d, h, w, c, ldx, ldv, groups, cpg, ch0, act,
                                       a_scale, 2, status, stream);
}

extern "C" int cs_groupnorm_apply_wino16(const float* x, const float* stats, const float* gamma, const float* beta,
                                         void* v_hi, void* v_lo, int nb, int d, int h, int w, int c, int ldx, int ldv,
                                         int groups, int act, float a_scale, int32_t* status, cs_stream_t stream) {
  if (groups <= 0 || c <= 0 || c % groups) return CS_EINVAL;
  return cs_groupnorm_apply_wino16_range(x, stats, gamma, beta, v_hi, v_lo, nb, d, h, w, c, ldx, ldv, groups, c / groups, 0,
                                         act, a_scale, status, stream);
}

extern "C" int cs_groupnorm_apply_split16(const float* x, const float* stats, const float* gamma,
                                          const float* beta, void* y_hi, void* y_lo, int nb, int rows, int c,
                                          int ldx, int ldy, int groups, int act, float a_scale,
                                          int32_t* status, cs_stream_t stream) {
  if (groups <= 0 || c <= 0 || c % groups) return CS_EINVAL;
  return cs_groupnorm_apply_split16_range(x, stats, gamma, beta, y_hi, y_lo, nb, rows, c, ldx, ldy, groups, c / groups, 0,
                                          act, a_scale, status, stream);
}

extern "C" int cs_groupnorm(const float* x, const float* gamma, const float* beta, float* y, int nb, int rows, int c,
                            int ldx, int ldy, int groups, float eps, int act, void* ws, float* stats,
                            cs_stream_t stream) {
  if (!x || !gamma || !beta || !y || !stats || nb <= 0 || rows <= 0 || c <= 0 || groups <= 0) return CS_EINVAL;
  if (c % groups || ldx < c || ldy < c) return CS_EINVAL;
  if (gn_one_launch(nb, rows, c, groups)) {
    CS_LAUNCH(gn_small_kernel, dim3((unsigned)(nb * groups)), dim3(256), 0, (hipStream_t)stream, x, gamma, beta, y,
              stats, rows, c, ldx, ldy, groups, eps, act);
    CS_CHECK_LAUNCH();
    return CS_OK;
  }
  if (!ws) return CS_EINVAL;
  int rc = cs_groupnorm_stats(x, nb, rows, c, ldx, groups, eps, ws, stats, stream);
  if (rc) return rc;
  return cs_groupnorm_apply(x, stats, gamma, beta, y, nb, rows, c, ldx, ldy, groups, act, stream);
}

extern "C" int cs_groupnorm_silu_ndhwc(const float* x, const float* gamma, const float* beta,
                                       float* y, int nb, int rows, int c, int groups, float eps,
                                       void* ws, float* stats, cs_stream_t stream) {
  return cs_groupnorm(x, gamma, beta, y, nb, rows, c, c, c, groups, eps, CS_ACT_SILU, ws, stats, stream);
}

extern "C" int cs_layernorm(const float* x, const float* gamma, const float* beta, float* y, int m,
                            int c, int ldx, int ldy, float eps, cs_stream_t stream) {
  if (!x || !gamma || !beta || !y || m <= 0 || c <= 0) return CS_EINVAL;
  if ((c & 3) || (ldx & 3) || (ldy & 3) || ldx < c || ldy < c) return CS_EINVAL;
  if (((uintptr_t)x & 15) || ((uintptr_t)y & 15) || ((uintptr_t)gamma & 15) ||
      ((uintptr_t)beta & 15))
    return CS_EINVAL;
  const int grid = cs_grid_for(((int64_t)m + 3) / 4, 1, 256 * 32);
  CS_LN_LAUNCH(ln_kernel, c >> 2, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, gamma, beta, y, m, c, ldx, ldy, eps);
  CS_CHECK_LAUNCH();
  return CS_OK;
}

// LayerNorm whose output is the interleaved F16X3 operand pair of y * a_scale (see ln_pair_kernel): y has the bytes of an
// fp32 [m][ldy] tensor (ldy in floats, c and ldy multiples of 16).  Feeds cs_conv_gemm with a_format = 2.
extern "C" int cs_layernorm_pair16(const float* x, const float* gamma, const float* beta, void* y, int m, int c, int ldx,
                                   int ldy, float eps, float a_scale, int32_t* status, cs_stream_t stream) {
  if (!x || !gamma || !beta || !y || m <= 0 || c <= 0 || !(a_scale > 0.f)) return CS_EINVAL;
  if ((c & 15) || (ldx & 3) || (ldy & 15) || ldx < c || ldy < c) return CS_EINVAL;
  if (((uintptr_t)x & 15) || ((uintptr_t)y & 15) || ((uintptr_t)gamma & 15) || ((uintptr_t)beta & 15)) return CS_EINVAL;
  const int grid = cs_grid_for(((int64_t)m + 3) / 4, 1, 256 * 32);
  CS_LN_LAUNCH(ln_pair_kernel, c >> 2, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, gamma, beta, (_Float16*)y, m, c, ldx,
               ldy, eps, a_scale, status);
  CS_CHECK_LAUNCH();
  return CS_OK;
}
