// What the flash-attention kernels share (cs_attention.hip: attn_kernel, fp32 MFMA; cs_attention_f16x3.hip: attn_f16x3_kernel,
// attn_presplit_kernel, attn_f16x3_img_kernel, fp16 hi / lo pairs on the fp16 MFMA): the tile layout, the block -> (query tile,
// sample, head) map with the grid it needs, the Q fragments, the split of one K / V unit into the LDS images, the online
// softmax of one key tile, the straight MFMA loops, the normalise-and-store tail, and the host's argument predicate.  ONE
// source each, so every kernel runs the same per-tile arithmetic in the same order and gives the same bits -- the in-kernel
// split, the tile-image route and the eight-wave variants are bit-identical by construction (profiles/attn_one_core_bits.txt).
// The build uses -ffp-contract=off: no expression here may be re-associated, and the exponent's fmaf stays an fmaf.
//
// All kernels use the "swapped" formulation, so the softmax's reduction axis is lane-local:
//   S^T[j][i] = sum_d K[j][d] Q[i][d]     O^T[d][i] += sum_j V[j][d] P^T[j][i]
// Register -> key map of the 32x32 C/D layout: lane (i = lane&31, half = lane>>5) holds S^T[j][i] for
// j = (r&3) + 8*(r>>2) + 4*half, r in [0,16).  The fp16 PV MFMA (jb, qq) takes registers r = 8qq..8qq+7 as its 8 k-slots, so
// k-slot (half, e) is key 32*jb + ((8qq+e)&3) + 8*((8qq+e)>>2) + 4*half; the V^T image stores key j at column vpos(j) = j
// with bits 2 and 3 swapped, which makes those 8 keys one contiguous 16-byte read.
#pragma once
#include "cs_common.h"

typedef _Float16 attn_h8 __attribute__((ext_vector_type(8)));
typedef _Float16 attn_h4 __attribute__((ext_vector_type(4)));

// ---- 1. the LDS tile of the fp16 kernels: [Kh | Kl] = [KT][LDK] each, then [Vh | Vl] = [DP][LDV] each (V^T, keys at vpos) ----
// (the fp32 kernel's tile -- floats, DP + 1 / DP + 4 -- stays with that kernel)
template <int DB, int KT>
struct AttnTile {
  static constexpr int DP = 32 * DB;
  static constexpr int LDK = DP + 8;          // halves; 16 consecutive rows hit 16 distinct 16-byte slots
  static constexpr int LDV = KT + 8;
  static constexpr int JB = KT / 32;          // 32-key score blocks
  static constexpr int KS = DP / 16;          // k-steps of the QK^T contraction
  static constexpr int K_HALVES = KT * LDK, V_HALVES = DP * LDV;      // one image
  static constexpr int TILE_HALVES = 2 * (K_HALVES + V_HALVES);
  static constexpr int TILE_BYTES = TILE_HALVES * 2;
};

__device__ __forceinline__ int vpos(int j) {   // swap bits 2 and 3
  return (j & ~12) | ((j & 4) << 1) | ((j & 8) >> 1);
}
// LDS offset (halves, within a V^T image) of the first of the four stores of V unit (channels 4*c4 .. 4*c4+3, key j)
template <int LDV>
__device__ __forceinline__ int attn_v_off(int c4, int j) { return (c4 * 4) * LDV + vpos(j); }

// ---- 2. block -> (query tile qt, sample b, head h), and the grid that map needs ----
// XCD-aware placement (speed only): block w runs on XCD w % 8, each XCD has its own 4 MB L2, and the query tiles of one
// (sample, head) all read the SAME K / V rows (or tile images) -- so the j-th block of XCD x takes query tile j % qtiles of
// group x + 8 * (j / qtiles): a group's workgroups share one L2 and run side by side (the decoder: 32 query tiles = the 32 CUs
// of an XCD).  In launch order every XCD would hold tiles of eight groups at once (77 MB of images against 4 MB of L2: each
// workgroup then pulls its 9.6 MB through the fabric, ~5 TB/s chip-wide -- that was the image kernel's bound).
// XCD = false is plain launch order (the fp32 kernel; A/B builds of the others with -DCS_ATTN_NO_XCD).
#ifdef CS_ATTN_NO_XCD
constexpr bool ATTN_XCD = false;
#else
constexpr bool ATTN_XCD = true;
#endif
// false: this workgroup is grid padding and exits whole
template <bool XCD>
__device__ __forceinline__ bool attn_block_map(int qtiles, int heads, int nbh, int& qt, int& b, int& h) {
  int bid = blockIdx.x;
  if constexpr (XCD) {
    const int xw = blockIdx.x & 7, xj = blockIdx.x >> 3;
    qt = xj % qtiles;
    bid = xw + 8 * (xj / qtiles);
    if (bid >= nbh) return false;
  } else {
    qt = bid % qtiles;
    bid /= qtiles;
  }
  h = bid % heads;
  b = bid / heads;
  return true;
}
template <bool XCD>
static inline int64_t attn_grid(int qtiles, int nb, int heads) {
  if (XCD) return (int64_t)qtiles * (((int64_t)heads * nb + 7) / 8 * 8);      // whole groups of eight (sample, head)s
  return (int64_t)qtiles * heads * nb;
}

// ---- 3. fp32 -> fp16 hi / lo, the Q fragments, one K unit and one V unit ----
__device__ __forceinline__ void split1(float v, _Float16& hi, _Float16& lo) {
  hi = (_Float16)v;
  lo = (_Float16)(v - (float)hi);
}
// operand split that also tracks the lane's largest |operand| (overflow report, see CS_STATUS_F16X3_OVERFLOW)
__device__ __forceinline__ void split1m(float v, _Float16& hi, _Float16& lo, float& amax) {
  amax = fmaxf(amax, fabsf(v));
  split1(v, hi, lo);
}

// Q fragments of query row qp: qh[t][e] = Q[i][16t + 8*half + e] * scale * qs (qs = the power-of-two operand pre-scale)
template <int KS>
__device__ __forceinline__ void attn_load_q(const float* __restrict__ qp, int dh, int half, float scale, float qs,
                                            attn_h8 (&qh)[KS], attn_h8 (&ql)[KS], float& amax) {
#pragma unroll
  for (int t = 0; t < KS; ++t)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int d = 16 * t + 8 * half + e;
      const float x = d < dh ? qp[d] * (scale * qs) : 0.f;
      _Float16 a, c;
      split1m(x, a, c, amax);
      qh[t][e] = a;
      ql[t][e] = c;
    }
}

// K unit (key j, 4 channels) -> 8 bytes of the hi image and of the lo image at `off` = j * LDK + 4 * c4.
// X1 = plain fp16 operands: the lo images are never read, so never written.
template <bool X1>
__device__ __forceinline__ void attn_split_k4(const float4& kv, float ks, _Float16* Kh, _Float16* Kl, int off, float& amax) {
  const float x[4] = {kv.x, kv.y, kv.z, kv.w};
  attn_h4 hi, lo;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    _Float16 a, c;
    split1m(x[e] * ks, a, c, amax);
    hi[e] = a;
    lo[e] = c;
  }
  *reinterpret_cast<attn_h4*>(Kh + off) = hi;
  if constexpr (!X1) *reinterpret_cast<attn_h4*>(Kl + off) = lo;
}
// V unit (4 channels, key j) -> four two-byte stores down a column of the V^T images, the first at `off` = attn_v_off(c4, j).
// Which thread takes which unit is the caller's: (4 channels, key j) with the key fastest in the kernels (a wave writes one
// contiguous run of a V^T row), (key j, 4 channels) in the pre-pass (coalesced reads).
template <bool X1, int LDV>
__device__ __forceinline__ void attn_split_v4(const float4& vv, float vs, _Float16* Vh, _Float16* Vl, int off, float& amax) {
  const float x[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    _Float16 a, c;
    split1m(x[e] * vs, a, c, amax);
    Vh[off + e * LDV] = a;
    if constexpr (!X1) Vl[off + e * LDV] = c;
  }
}

// ---- 4. the online softmax of one key tile (per query i = lane&31), in place on the score blocks ----
// E = the exponent policy: p(s, m) = the weight of score s under row maximum m, alpha(mrun, mnew) = what the old sums keep.
// fp16 kernels, in the accumulator's own units: sacc = logit * qs * ks, so with cexp = log2(e) / (qs * ks)
//   p * P_SCALE = exp2((sacc - m) * cexp + log2(P_SCALE))
// is one subtract, one fma and one v_exp_f32 per element (the row maximum m stays in raw units, the P_SCALE the PV operands
// need is folded into the exponent, and the running sum carries it until attn_store_out).
struct AttnExp2 {
  float cexp, lp;
  __device__ __forceinline__ float p(float s, float m) const {
#ifdef CS_ATTN_WHATIF_NO_EXP           // (timing-only what-if builds, tools/attn*_whatif.sh: wrong results)
    return fmaf(s - m, cexp, lp);
#else
    return __builtin_amdgcn_exp2f(fmaf(s - m, cexp, lp));
#endif
  }
  __device__ __forceinline__ float alpha(float mrun, float mnew) const { return __builtin_amdgcn_exp2f((mrun - mnew) * cexp); }
};
struct AttnExpF {                      // the fp32 kernel: logits in natural units
  __device__ __forceinline__ float p(float s, float m) const { return expf(s - m); }
  __device__ __forceinline__ float alpha(float mrun, float mnew) const { return expf(mrun - mnew); }
};

// s[jb][r] = score of key kt0 + 32*jb + (r&3) + 8*(r>>2) + 4*half on entry, its weight p on return; mrun / lrun = the running
// row maximum and (this half-wave's) row sum; oacc is rescaled for the new maximum
template <int KT, int DB, class E>
__device__ __forceinline__ void attn_softmax_tile(f32x16 (&s)[KT / 32], f32x16 (&oacc)[DB], float& mrun, float& lrun, int kt0,
                                                  int nk, int half, const E& ex) {
  constexpr int JB = KT / 32;
  if (kt0 + KT > nk) {               // ragged last tile only (wave-uniform): keys past nk take no weight
#pragma unroll
    for (int jb = 0; jb < JB; ++jb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int j = kt0 + jb * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (j >= nk) s[jb][r] = -INFINITY;
      }
  }
  float mloc = -INFINITY;
#pragma unroll
  for (int jb = 0; jb < JB; ++jb)
#pragma unroll
    for (int r = 0; r < 16; ++r) mloc = fmaxf(mloc, s[jb][r]);
  mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
  const float mnew = fmaxf(mrun, mloc);
  const float alpha = (mrun == -INFINITY) ? 0.f : ex.alpha(mrun, mnew);
  float psum = 0.f;
#pragma unroll
  for (int jb = 0; jb < JB; ++jb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float pv = ex.p(s[jb][r], mnew);
      s[jb][r] = pv;
      psum += pv;
    }
  lrun = lrun * alpha + psum;
  mrun = mnew;
#ifndef CS_ATTN_WHATIF_NO_RESCALE      // (timing-only what-if builds: wrong results)
#pragma unroll
  for (int d = 0; d < DB; ++d)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[d][r] *= alpha;
#endif
}

// ---- 5. the straight MFMA loops of the fp16 kernels (the image kernel's ring-scheduled ones are that kernel's own) ----
// each contraction = 3 v_mfma_f32_32x32x16_f16 (lo*hi + hi*lo + hi*hi), fp32 accumulate; X1: hi*hi alone
// S^T = K Q^T of the K images at Kh / Kl
template <bool X1, int DB, int KT>
__device__ __forceinline__ void attn_qk_tile(const _Float16* Kh, const _Float16* Kl, const attn_h8 (&qh)[AttnTile<DB, KT>::KS],
                                             const attn_h8 (&ql)[AttnTile<DB, KT>::KS], int l31, int half, f32x16 (&sacc)[KT / 32]) {
  using T = AttnTile<DB, KT>;
#pragma unroll
  for (int jb = 0; jb < T::JB; ++jb)
#pragma unroll
    for (int r = 0; r < 16; ++r) sacc[jb][r] = 0.f;
#pragma unroll
  for (int t = 0; t < T::KS; ++t)
#pragma unroll
    for (int jb = 0; jb < T::JB; ++jb) {
      const int off = (jb * 32 + l31) * T::LDK + 16 * t + 8 * half;
      const attn_h8 kh = *reinterpret_cast<const attn_h8*>(Kh + off);
      if constexpr (!X1) {
        const attn_h8 kl = *reinterpret_cast<const attn_h8*>(Kl + off);
        sacc[jb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kl, qh[t], sacc[jb], 0, 0, 0);
        sacc[jb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, ql[t], sacc[jb], 0, 0, 0);
      }
      sacc[jb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, qh[t], sacc[jb], 0, 0, 0);
    }
}

// O^T += V^T P^T of the V^T images at Vh / Vl, P^T split into hi / lo straight from the weights in s
template <bool X1, int DB, int KT>
__device__ __forceinline__ void attn_pv_tile(const _Float16* Vh, const _Float16* Vl, const f32x16 (&s)[KT / 32], int l31, int half,
                                             f32x16 (&oacc)[DB]) {
  using T = AttnTile<DB, KT>;
#pragma unroll
  for (int jb = 0; jb < T::JB; ++jb)
#pragma unroll
    for (int qq = 0; qq < 2; ++qq) {
      attn_h8 ph, pl;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        _Float16 a, c;
        split1(s[jb][8 * qq + e], a, c);
        ph[e] = a;
        pl[e] = c;
      }
#pragma unroll
      for (int d = 0; d < DB; ++d) {
        const int off = (32 * d + l31) * T::LDV + 32 * jb + 16 * qq + 8 * half;
        const attn_h8 vh = *reinterpret_cast<const attn_h8*>(Vh + off);
        if constexpr (!X1) {
          const attn_h8 vl = *reinterpret_cast<const attn_h8*>(Vl + off);
          oacc[d] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vl, ph, oacc[d], 0, 0, 0);
          oacc[d] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, pl, oacc[d], 0, 0, 0);
        }
        oacc[d] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, ph, oacc[d], 0, 0, 0);
      }
    }
}

// ---- 6. normalise and store O^T: row `qrow` of sample b, head h; vs = what the V operands (and so oacc) were scaled by ----
// (lrun carries whatever the policy's p carries -- P_SCALE in the fp16 kernels, which the P operands carried too; every lane
// takes part in the half-wave exchange, so the call sits outside any divergent branch)
template <int DB>
__device__ __forceinline__ void attn_store_out(const f32x16 (&oacc)[DB], float lrun, float vs, float* __restrict__ out, int b,
                                               int nq, int qrow, int ldo, int h, int dh, int half) {
  const float ltot = lrun + __shfl_xor(lrun, 32, 64);
  const float inv = 1.0f / (ltot * vs);
  if (qrow < nq) {
    float* op = out + ((int64_t)b * nq + qrow) * ldo + h * dh;
#pragma unroll
    for (int d = 0; d < DB; ++d)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int dd = 32 * d + 8 * g + 4 * half;
        if (dd < dh) {
          f32x4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = oacc[d][4 * g + e] * inv;
          *reinterpret_cast<f32x4*>(op + dd) = o;
        }
      }
  }
}

// ---- 7. the host's argument predicate (plain C++, no HIP call): what every attention entry refuses with CS_EINVAL ----
// rows of heads * dh floats inside their ld*, float4 access everywhere (dh and ld* multiples of 4, 16-byte aligned bases).
// ws = the tile-image workspace where the call will use it, NULL where it will not (then it is ignored, alignment included).
// The head width's upper end (256) is the dispatch's, not this predicate's.
static inline bool attn_args_ok(const void* q, const void* k, const void* v, const void* out, const void* ws, int nb, int nq,
                                int nk, int heads, int dh, int ldq, int ldk, int ldv, int ldo) {
  if (!q || !k || !v || !out || nb <= 0 || nq <= 0 || nk <= 0 || heads <= 0 || dh <= 0) return false;
  if ((dh & 3) || (ldq & 3) || (ldk & 3) || (ldv & 3) || (ldo & 3)) return false;
  if (ldq < heads * dh || ldk < heads * dh || ldv < heads * dh || ldo < heads * dh) return false;
  return !(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out | (uintptr_t)ws) & 15);
}
