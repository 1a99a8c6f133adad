// What follows a GEMM's accumulation, for every kernel of the GEMM family (cs_gemm.hip, cs_gemm_f16x3.hip, cs_gemm_kw.hip):
// the epilogue terms, the interleaved fp16 operand pair of the result, and the fp64 column sums for the GroupNorm that
// follows.  ONE source, so every site runs the same arithmetic in the same order and gives the same bits -- the split-K
// reduce in its fused and two-kernel forms, the K-wave kernel and its one-chain twin, the Winograd output transform, the
// float4 and scalar epilogues of the tile kernels, the register-direct epilogues of the transposed-accumulator (TR) kernels
// (cs_gemm_f16x3.hip: stores by row per lane or -- after cs_quad_transpose4 -- by whole lines).  Device code only,
// no state.  (One written-out copy remains: the pair conversion and the 16-row column sum inside fused_splitk_reduce,
// cs_gemm_f16x3.hip, which says why.)
#pragma once
#include "cs_common.h"

typedef unsigned cs_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned cs_u32x2 __attribute__((ext_vector_type(2)));

// ---- 1. the terms:  v += bias;  v = v * scale + shift;  v += rowvec[m / rv_rows];  v = act(v);  v += res  ----
// D = CsConvGemm or CsFuseK (fields bias, scale, shift, rowvec, res, ldr, ldrv, rv_rows, act); one float4 at row m, column n.
// M is the caller's row index type (int; wino_out_kernel's int64_t), so that its address arithmetic stays the caller's.
template <class D, class M>
__device__ __forceinline__ f32x4 cs_epi_terms4(const D& d, f32x4 v, M m, int n) {
  if (d.bias) v += *reinterpret_cast<const f32x4*>(d.bias + n);
  if (d.scale) v = v * *reinterpret_cast<const f32x4*>(d.scale + n) + *reinterpret_cast<const f32x4*>(d.shift + n);
  if (d.rowvec) v += *reinterpret_cast<const f32x4*>(d.rowvec + (int64_t)(m / d.rv_rows) * d.ldrv + n);
  if (d.act != CS_ACT_NONE) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = cs_act(v[e], d.act);
  }
  if (d.res) v += *reinterpret_cast<const f32x4*>(d.res + (int64_t)m * d.ldr + n);
  return v;
}
// the scalar twin (one column per lane): the caller loads its column's bias / scale / shift ONCE, outside its row loop
template <class D>
__device__ __forceinline__ float cs_epi_terms1(const D& d, float v, float bias, float scale, float shift, int m, int n) {
  v += bias;
  if (d.scale) v = v * scale + shift;
  if (d.rowvec) v += d.rowvec[(int64_t)(m / d.rv_rows) * d.ldrv + n];
  v = cs_act(v, d.act);
  if (d.res) v += d.res[(int64_t)m * d.ldr + n];
  return v;
}

// the fused GEGLU gate of ff.net.0.proj (attention.py:44-46): x * gelu(gate), the biases already added by the caller
__device__ __forceinline__ f32x4 cs_geglu4(f32x4 x, const f32x4& g) {
#pragma unroll
  for (int e = 0; e < 4; ++e) x[e] = x[e] * cs_gelu(g[e]);
  return x;
}

// ---- 2. the interleaved operand pair (CsConvGemm.out_format = 2) of v * out_scale ----
// Two forms, one conversion: cs_pair16 (partner lane = lane ^ 1) and cs_pair16_half32 (partner lane = lane ^ 32).
// A row is 64-byte chunks of 16 columns = [hi 0-7 | lo 0-7 | hi 8-15 | lo 8-15] (fp16 halves; hi = half(o), lo = half(o - hi)).
// PRECONDITION: adjacent lanes 2t / 2t + 1 hold columns 8g .. 8g+3 / 8g+4 .. 8g+7 of ONE row (`odd` = the second of them),
// and the call sits in a branch that is uniform over the wave: every lane takes part in the half swap (quad_perm 1,0,3,2),
// masked lanes with v = 0.  The even lane then holds [hi 8g .. 8g+7], the odd one [lo 8g .. 8g+7]: one 16-byte store each,
// at byte cs_pair_off(first column of the lane) of the row.  `oamax` is the lane's running max |v * out_scale|.
// (the conversion both forms share: o = v * out_scale -> running max |o|, H = the four hi halves, L = the four lo halves)
__device__ __forceinline__ void cs_pair_split4(const f32x4& v, float out_scale, float& oamax, cs_u32x2& H, cs_u32x2& L) {
  typedef _Float16 h4 __attribute__((ext_vector_type(4)));
  h4 hi, lo;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float o = v[e] * out_scale;
    oamax = fmaxf(oamax, fabsf(o));
    hi[e] = (_Float16)o;
    lo[e] = (_Float16)(o - (float)hi[e]);
  }
  H = __builtin_bit_cast(cs_u32x2, hi);
  L = __builtin_bit_cast(cs_u32x2, lo);
}
__device__ __forceinline__ cs_u32x4 cs_pair16(const f32x4& v, float out_scale, bool odd, float& oamax) {
  typedef cs_u32x2 u32x2;
  u32x2 H, L;
  cs_pair_split4(v, out_scale, oamax, H, L);
  const u32x2 send = odd ? H : L;
  u32x2 recv;
  recv[0] = (unsigned)__builtin_amdgcn_update_dpp(0, (int)send[0], 0xB1, 0xF, 0xF, true);
  recv[1] = (unsigned)__builtin_amdgcn_update_dpp(0, (int)send[1], 0xB1, 0xF, 0xF, true);
  cs_u32x4 r;
  r[0] = odd ? recv[0] : H[0];
  r[1] = odd ? recv[1] : H[1];
  r[2] = odd ? L[0] : recv[0];
  r[3] = odd ? L[1] : recv[1];
  return r;
}
// The second form, for a TRANSPOSED 32x32 MFMA accumulator (cs_gemm_f16x3.hip, TR kernels): the two halves of a row's eight
// columns sit 32 lanes apart, not one.  PRECONDITION: lanes l / l + 32 (l < 32) hold columns 8g .. 8g+3 / 8g+4 .. 8g+7 of ONE
// row, the whole wave is active (v_permlane32_swap ignores EXEC for what it reads; a masked lane passes v = 0).  The swap
// exchanges the upper half of the hi words with the lower half of the lo words, so lane l ends with [hi 8g .. 8g+7] and lane
// l + 32 with [lo 8g .. 8g+7]: one 16-byte store each at byte cs_pair_off(first column of the lane) of the row, as above.
__device__ __forceinline__ cs_u32x4 cs_pair16_half32(const f32x4& v, float out_scale, float& oamax) {
  cs_u32x2 H, L;
  cs_pair_split4(v, out_scale, oamax, H, L);
  // (vdst = H, src = L: lanes 32-63 of H <-> lanes 0-31 of L)
  const auto s0 = __builtin_amdgcn_permlane32_swap(H[0], L[0], false, false);
  const auto s1 = __builtin_amdgcn_permlane32_swap(H[1], L[1], false, false);
  cs_u32x4 r;
  r[0] = s0[0];      // lower lane: own hi 0-3      upper lane: the lower lane's lo 0-3
  r[1] = s1[0];
  r[2] = s0[1];      // lower lane: the upper lane's hi 4-7      upper lane: own lo 4-7
  r[3] = s1[1];
  return r;
}
// Whole-line stores from a TRANSPOSED 32x32 MFMA accumulator (cs_gemm_f16x3.hip, TR kernels).  There lane (r = l & 31,
// h = l >> 5) holds in x[g] the columns 8 g + 4 h + 0..3 of row r of the block: a store of x[g] touches 32 rows with 32 bytes
// each.  The four lanes of a quad (rows r0 + q, q = l & 3, same h) exchange their float4s -- a 4x4 transposition of float4s --
// so that x[s] of lane q becomes row r0 + s, columns 8 q + 4 h + 0..3: the store of slot s then covers eight rows with one whole
// 128-byte line of the block each (q = 0..3, h = 0..1 of a quad pair are one row's 32 columns), and a residual loaded at those
// addresses does too.  Two butterfly steps of DPP quad_perm moves (partner q ^ 1 swaps the odd / even slots, partner q ^ 2 the
// upper / lower pair); registers only, no LDS, no barrier, one block at a time.  PRECONDITION: the whole wave is active (a DPP
// move reads nothing from a lane EXEC masks out).  Values are moved, never changed: lanes l / l + 32 still hold the two halves
// of one row's eight columns afterwards, which is what cs_pair16_half32 asks for.
__device__ __forceinline__ void cs_quad_transpose4(f32x4 (&x)[4], int lane) {
  const bool o1 = lane & 1, o2 = lane & 2;
#pragma unroll
  for (int s = 0; s < 4; s += 2)       // slot bit 0 <-> lane bit 0 (quad_perm 1,0,3,2)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float a = x[s][e], b = x[s + 1][e];
      const float recv = __builtin_bit_cast(
          float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, o1 ? a : b), 0xB1, 0xF, 0xF, true));
      x[s][e] = o1 ? recv : a;
      x[s + 1][e] = o1 ? b : recv;
    }
#pragma unroll
  for (int s = 0; s < 2; ++s)          // slot bit 1 <-> lane bit 1 (quad_perm 2,3,0,1)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float a = x[s][e], b = x[s + 2][e];
      const float recv = __builtin_bit_cast(
          float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, o2 ? a : b), 0x4E, 0xF, 0xF, true));
      x[s][e] = o2 ? recv : a;
      x[s + 2][e] = o2 ? b : recv;
    }
}
__device__ __forceinline__ int cs_pair_off(int col) { return (col >> 4) * 64 + ((col & 8) ? 32 : 0) + ((col & 4) ? 16 : 0); }
// a converted value reached the fp16 range (its hi half would be +-inf): the sticky flag of the launch
template <class D>
__device__ __forceinline__ void cs_pair_flag(const D& d, bool opair, float oamax) {
  if (opair && d.status && oamax >= 65504.f) atomicOr(d.status, CS_STATUS_F16X3_OVERFLOW);
}

// ---- 3. fp64 (sum, sum of squares) per (statistics tile, column) for CsConvGemm.gn_part ----
// Form A: a workgroup of 16 row lanes `rl` x 16 float4 column lanes `cl`; x = the thread's own fp64 sums (or sums of squares)
// over its rows of columns 4 cl .. 4 cl + 3.  The 16 row lanes are added in lane order through sc; row lane 0 gets the totals.
// Called twice (sums, then squares) on the same sc, so it carries the barriers around its use of sc itself: EVERY thread of
// the workgroup calls it.  The caller's row lane 0 then writes the (sum, sum of squares) pairs of its four columns.
__device__ __forceinline__ void cs_colsum_lanes16(double (*sc)[64], const double (&x)[4], int rl, int cl, double (&tot)[4]) {
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 4; ++e) sc[rl][cl * 4 + e] = x[e];
  __syncthreads();
  if (rl == 0) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      double t = 0.0;
      for (int r2 = 0; r2 < 16; ++r2) t += sc[r2][cl * 4 + e];
      tot[e] = t;
    }
  }
}
// Form B: one thread adds ITS column n (at `col`) of a staged fp32 block of `rows` rows (row stride ld floats) in row order and
// writes the pair of statistics tile `tile`.  The caller owns the barriers between staging, this, and the next use of the block.
// (The K-wave kernel's 64-row tiles.  fused_splitk_reduce adds its 16-row blocks the same way in its own loop: see there.)
template <class D>
__device__ __forceinline__ void cs_colsum_staged(const D& d, const float* col, int ld, int rows, int tile, int n) {
  double ts = 0.0, tq = 0.0;
  for (int r2 = 0; r2 < rows; ++r2) {
    const double x = (double)col[r2 * ld];
    ts += x;
    tq += x * x;
  }
  double* o = d.gn_part + ((int64_t)tile * d.gn_ld + n) * 2;
  o[0] = ts;
  o[1] = tq;
}
