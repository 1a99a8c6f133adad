// Scene-graph constraint accuracy on the MI355X: the layout table of scripts/eval_3dfront.py:411-415,722
// (helpers/metrics_3dfront.py:57-311 validate_constrains / validate_constrains_changes, :314-439 corners_from_box, box3d_iou,
// poly_area, box3d_vol, polygon_clip).  The reference walks the triples on the host and reads two boxes back per triple; here
//   cs_scene_constraints   one thread per triple over a ragged batch of scenes: verdict per triple, counts per scene and
//                          category with integer atomics (exact, order-free)
//   cs_box3d_iou_pairs     the same box3d_iou device function over M box pairs, so the clipping code is pinned on values
// Plain fp64 C++: every reference line is restated in its operation order from the fp32 box widened to fp64, products and sums
// are never contracted, comparisons and divisions keep IEEE semantics (nan > x is false, x / 0 is +-inf or nan) because the
// reference's verdicts lean on them.  The kernels are tiny and latency-bound: no LDS, no MFMA, vector loads and stores only.
#include "cs_common.h"

#pragma clang fp contract(off)

#define CS_HD __host__ __device__ __forceinline__

namespace {

constexpr int CONSTRAINT_THREADS = 128;
constexpr int CLIP_MAX = 8;            // a quadrilateral cut by four half-planes gains at most one vertex per cut
constexpr int N_CATEGORIES = 11;

// python's min(a, b) / max(a, b) on floats: the SECOND argument wins only when it compares strictly
CS_HD double py_min(double a, double b) { return b < a ? b : a; }
CS_HD double py_max(double a, double b) { return b > a ? b : a; }

// metrics_3dfront.py:50-54 denormalize -> helpers/util.py:559 (box * std) / scale + mean; norm = [mean[7] | std[7]] or NULL
CS_HD void load_box(const float* __restrict__ row, int params, const double* __restrict__ norm, double scale, double b[6]) {
  (void)params;                                            // the angle (index 6) is never read by any rule
  for (int i = 0; i < 6; ++i) {
    const double v = (double)row[i];
    b[i] = norm ? (v * norm[7 + i]) / scale + norm[i] : v;
  }
}

// :314-334 corners_from_box without the identity rotation: corner i of the 8, (x, y, z)
CS_HD void box_corner(const double b[6], bool with_translation, int i, double c[3]) {
  const double hw = b[2] / 2, hl = b[0] / 2;
  const double x = (i & 2) ? -hw : hw;                     // w/2, w/2, -w/2, -w/2, ...
  const double y = (i & 4) ? 0.0 : b[1];                   // h x4, 0 x4
  const double z = ((i & 3) == 1 || (i & 3) == 2) ? -hl : hl;   // l/2, -l/2, -l/2, l/2, ...
  c[0] = with_translation ? x + b[3] : x;
  c[1] = with_translation ? y + b[4] : y;
  c[2] = with_translation ? z + b[5] : z;
}

struct Poly {
  double x[CLIP_MAX], y[CLIP_MAX];
  int n;
};

CS_HD void poly_push(Poly& p, double x, double y) {
  if (p.n < CLIP_MAX) {
    p.x[p.n] = x;
    p.y[p.n] = y;
    ++p.n;
  }
}

// :396-439 polygon_clip (Sutherland-Hodgman, strict inside test); returns the vertex count, 0 = None
CS_HD int polygon_clip(const double sx[4], const double sy[4], const double cx[4], const double cy[4], Poly& out) {
  out.n = 4;
  for (int i = 0; i < 4; ++i) out.x[i] = sx[i], out.y[i] = sy[i];
  double c1x = cx[3], c1y = cy[3];
  for (int k = 0; k < 4; ++k) {
    const double c2x = cx[k], c2y = cy[k];
    Poly in = out;
    out.n = 0;
    double s0 = in.x[in.n - 1], s1 = in.y[in.n - 1];
    bool s_in = (c2x - c1x) * (s1 - c1y) > (c2y - c1y) * (s0 - c1x);
    for (int v = 0; v < in.n; ++v) {
      const double e0 = in.x[v], e1 = in.y[v];
      const bool e_in = (c2x - c1x) * (e1 - c1y) > (c2y - c1y) * (e0 - c1x);
      if (e_in != s_in) {                                  // :410-416 computeIntersection
        const double dc0 = c1x - c2x, dc1 = c1y - c2y, dp0 = s0 - e0, dp1 = s1 - e1;
        const double n1 = c1x * c2y - c1y * c2x, n2 = s0 * e1 - s1 * e0;
        const double n3 = 1.0 / (dc0 * dp1 - dc1 * dp0);
        poly_push(out, (n1 * dp0 - n2 * dc0) * n3, (n1 * dp1 - n2 * dc1) * n3);
      }
      if (e_in) poly_push(out, e0, e1);
      s0 = e0, s1 = e1, s_in = e_in;
    }
    c1x = c2x, c1y = c2y;
    if (out.n == 0) return 0;
  }
  return out.n;
}

// :337-370 box3d_iou on denormalised boxes -> (iou, iou_2d)
CS_HD void box3d_iou(const double b1[6], const double b2[6], bool with_translation, double* iou, double* iou_2d) {
  double c1[8][3], c2[8][3];
  for (int i = 0; i < 8; ++i) {
    box_corner(b1, with_translation, i, c1[i]);
    box_corner(b2, with_translation, i, c2[i]);
  }
  double r1x[4], r1y[4], r2x[4], r2y[4];                   // :350-351 the (z, x) footprints
  for (int i = 0; i < 4; ++i) {
    r1x[i] = c1[i][2], r1y[i] = c1[i][0];
    r2x[i] = c2[i][2], r2y[i] = c2[i][0];
  }
  // :385-387 poly_area = 0.5 |x . roll(y, 1) - y . roll(x, 1)|
  double a1p = 0, a1m = 0, a2p = 0, a2m = 0;
  for (int i = 0; i < 4; ++i) {
    const int j = (i + 3) & 3;
    a1p += r1x[i] * r1y[j], a1m += r1y[i] * r1x[j];
    a2p += r2x[i] * r2y[j], a2m += r2y[i] * r2x[j];
  }
  const double area1 = 0.5 * fabs(a1p - a1m), area2 = 0.5 * fabs(a2p - a2m);
  // :373-383 the clipped polygon's area (the reference asks Qhull; the polygon is convex: shoelace).  Fewer than three
  // vertices is where the reference raises: area 0.
  Poly p;
  double inter_area = 0.0;
  if (polygon_clip(r1x, r1y, r2x, r2y, p) >= 3) {
    double acc = 0;
    for (int i = 0; i < p.n; ++i) {
      const int j = i + 1 == p.n ? 0 : i + 1;
      acc += p.x[i] * p.y[j] - p.x[j] * p.y[i];
    }
    inter_area = 0.5 * fabs(acc);
  }
  *iou_2d = inter_area / (area1 + area2 - inter_area);
  const double ymax = py_min(c1[0][1], c2[0][1]), ymin = py_max(c1[4][1], c2[4][1]);
  const double inter_vol = inter_area * py_max(0.0, ymax - ymin);
  double vol[2];                                           // :389-394 box3d_vol
  for (int w = 0; w < 2; ++w) {
    const double(*c)[3] = w ? c2 : c1;
    double e[3];
    const int a[3] = {0, 1, 0}, b[3] = {1, 2, 4};
    for (int k = 0; k < 3; ++k) {
      const double dx = c[a[k]][0] - c[b[k]][0], dy = c[a[k]][1] - c[b[k]][1], dz = c[a[k]][2] - c[b[k]][2];
      e[k] = sqrt((dx * dx + dy * dy) + dz * dz);
    }
    vol[w] = e[0] * e[1] * e[2];
  }
  *iou = inter_vol / py_min(vol[0], vol[1]);               // the SMALLER volume, not the union (:366-368)
}

// :10-15 close_dis: min over the 8x8 corner pairs of sqrt(-2 a.b + |a|^2 + |b|^2); a negative argument gives nan and np.min
// hands the nan on.  Returns whether `> 0.45` holds (never for nan).
CS_HD bool corners_apart(const double bs[6], const double bo[6]) {
  double m = INFINITY;
  bool nan = false;
  for (int i = 0; i < 8; ++i) {
    double a[3];
    box_corner(bs, true, i, a);
    const double aa = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
    for (int j = 0; j < 8; ++j) {
      double b[3];
      box_corner(bo, true, j, b);
      const double bb = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2];
      const double ab = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
      const double d = sqrt((-2 * ab + aa) + bb);
      if (d != d) nan = true;
      else if (d < m) m = d;
    }
  }
  return !nan && m > 0.45;
}

// :17-18 cal_l2_distance
CS_HD double l2_2d(double ax, double ay, double bx, double by) {
  const double dx = bx - ax, dy = by - ay;
  return sqrt(dx * dx + dy * dy);
}

// one triple's rule (:74-177 = :198-309): category 0..10 -> 1 satisfied, 0 violated
CS_HD int constraint_verdict(int cat, const double s[6], const double o[6], bool strict, double overlap_threshold) {
  if (cat < 4) {                                           // left / right compare pz, front / behind compare px
    const double d = cat < 2 ? s[5] - o[5] : s[3] - o[3];
    const bool off = cat == 0 ? d > -0.05 : cat == 1 ? d < 0.05 : cat == 2 ? d < -0.05 : d > 0.05;
    if (off) return 0;
    if (strict) {
      double iou, iou_2d;
      box3d_iou(s, o, true, &iou, &iou_2d);
      if (iou > overlap_threshold) return 0;
    }
    return 1;
  }
  if (cat < 6) {                                           // bigger / smaller than
    const double vs = s[0] * s[1] * s[2], vo = o[0] * o[1] * o[2];
    const double r = (vs - vo) / vs;
    return cat == 4 ? !(r < 0.15) : !(r > -0.15);
  }
  if (cat < 8) {                                           // taller / shorter than
    const double hs = s[4] + s[1], ho = o[4] + o[1];
    const double r = (hs - ho) / hs;
    return cat == 6 ? !(r < 0.1) : !(r > -0.1);
  }
  if (cat == 8) return fabs(s[4] - o[4]) < 0.04;           // standing on
  if (cat == 9) return !corners_apart(s, o);               // close by
  // symmetrical to: the subject's centre flipped in x, z or both lands within 0.45 of the object's
  return l2_2d(-s[3], -s[5], o[3], o[5]) < 0.45 || l2_2d(-s[3], s[5], o[3], o[5]) < 0.45 ||
         l2_2d(s[3], -s[5], o[3], o[5]) < 0.45;
}

__global__ __launch_bounds__(CONSTRAINT_THREADS) void scene_constraints_kernel(
    const float* __restrict__ boxes, int64_t n_boxes, int ld, int params, const int64_t* __restrict__ triples,
    int64_t n_triples, const int64_t* __restrict__ box_ptr, const int64_t* __restrict__ triple_ptr, int n_scenes,
    const int32_t* __restrict__ pred_code, int n_preds, const uint8_t* __restrict__ keep, int mode,
    const double* __restrict__ norm, double scale, int strict, double overlap_threshold, int8_t* __restrict__ verdict,
    int32_t* __restrict__ counts, int32_t* __restrict__ status) {
  const int64_t t = (int64_t)blockIdx.x * CONSTRAINT_THREADS + threadIdx.x;
  if (t >= n_triples) return;
  // the scene: the last sc in [0, n_scenes) with triple_ptr[sc] <= t
  int lo = 0, hi = n_scenes - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (triple_ptr[mid] <= t) lo = mid;
    else hi = mid - 1;
  }
  const int sc = lo;
  const int64_t b0 = box_ptr[sc], b1 = box_ptr[sc + 1];
  const int64_t s = triples[t * 3 + 0], p = triples[t * 3 + 1], o = triples[t * 3 + 2];
  // anything that leaves its range is reported, never dereferenced
  if (triple_ptr[sc] > t || triple_ptr[sc + 1] <= t || b0 < 0 || b1 < b0 || b1 > n_boxes || s < 0 || s >= b1 - b0 || o < 0 ||
      o >= b1 - b0 || p < 0 || p >= n_preds) {
    verdict[t] = -1;
    if (status) atomicOr(status, CS_STATUS_CONSTRAINT_RANGE);
    return;
  }
  const int cat = pred_code[p];
  bool take = cat >= 0 && cat < N_CATEGORIES;
  if (take && mode != 0) {
    const uint8_t ks = keep[b0 + s], ko = keep[b0 + o];
    take = mode == 1 ? (ks == 1 && ko == 1) : (ks == 0 || ko == 0);
  }
  if (!take) {
    verdict[t] = -1;
    return;
  }
  double bs[6], bo[6];
  load_box(boxes + (b0 + s) * ld, params, norm, scale, bs);
  load_box(boxes + (b0 + o) * ld, params, norm, scale, bo);
  const int v = constraint_verdict(cat, bs, bo, strict != 0, overlap_threshold);
  verdict[t] = (int8_t)v;
  int32_t* c = counts + ((int64_t)sc * N_CATEGORIES + cat) * 2;
  if (v) atomicAdd(c, 1);
  atomicAdd(c + 1, 1);
}

__global__ __launch_bounds__(CONSTRAINT_THREADS) void box3d_iou_pairs_kernel(const float* __restrict__ box1,
                                                                             const float* __restrict__ box2, int64_t m,
                                                                             int ld, int params, int with_translation,
                                                                             double* __restrict__ iou,
                                                                             double* __restrict__ iou_2d) {
  const int64_t i = (int64_t)blockIdx.x * CONSTRAINT_THREADS + threadIdx.x;
  if (i >= m) return;
  double a[6], b[6], r, r2;
  load_box(box1 + i * ld, params, nullptr, 1.0, a);
  load_box(box2 + i * ld, params, nullptr, 1.0, b);
  box3d_iou(a, b, with_translation != 0, &r, &r2);
  iou[i] = r;
  iou_2d[i] = r2;
}

}  // namespace

extern "C" int cs_scene_constraints(const float* boxes, int64_t n_boxes, int ld, int params, const int64_t* triples,
                                    int64_t n_triples, const int64_t* box_ptr, const int64_t* triple_ptr, int n_scenes,
                                    const int32_t* pred_code, int n_preds, const uint8_t* keep, int mode, const double* norm,
                                    double scale, int strict, double overlap_threshold, int8_t* verdict, int32_t* counts,
                                    int32_t* status, cs_stream_t stream) {
  if (!boxes || !triples || !box_ptr || !triple_ptr || !pred_code || !verdict || !counts || n_boxes <= 0 || n_triples < 0 ||
      n_triples > 0x7fffffffll * CONSTRAINT_THREADS || n_scenes <= 0 || n_scenes > (1 << 24) || n_preds <= 0 ||
      (params != 6 && params != 7) || ld < params || mode < 0 || mode > 2 || (mode != 0 && !keep) ||
      (mode == 2 && params == 7) ||          // validate_constrains_changes hands 7 values to box3d_iou's 6-parameter default
      (norm && !(scale != 0.0)))
    return CS_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(counts, 0, (size_t)n_scenes * N_CATEGORIES * 2 * sizeof(int32_t), s);
  if (e != hipSuccess) return (int)e;
  if (n_triples == 0) return CS_OK;
  CS_LAUNCH(scene_constraints_kernel, dim3((unsigned)((n_triples + CONSTRAINT_THREADS - 1) / CONSTRAINT_THREADS)),
            dim3(CONSTRAINT_THREADS), 0, s, boxes, n_boxes, ld, params, triples, n_triples, box_ptr, triple_ptr, n_scenes,
            pred_code, n_preds, keep, mode, norm, scale, strict, overlap_threshold, verdict, counts, status);
  CS_CHECK_LAUNCH();
  return CS_OK;
}

extern "C" int cs_box3d_iou_pairs(const float* box1, const float* box2, int64_t m, int ld, int params, int with_translation,
                                  double* iou, double* iou_2d, cs_stream_t stream) {
  if (!box1 || !box2 || !iou || !iou_2d || m <= 0 || m > 0x7fffffffll * CONSTRAINT_THREADS || (params != 6 && params != 7) ||
      ld < params)
    return CS_EINVAL;
  CS_LAUNCH(box3d_iou_pairs_kernel, dim3((unsigned)((m + CONSTRAINT_THREADS - 1) / CONSTRAINT_THREADS)),
            dim3(CONSTRAINT_THREADS), 0, (hipStream_t)stream, box1, box2, m, ld, params, with_translation, iou, iou_2d);
  CS_CHECK_LAUNCH();
  return CS_OK;
}
