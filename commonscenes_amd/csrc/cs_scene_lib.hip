// Scenes from a mesh library on the MI355X: the producers of the layout + retrieval, layout + txt2shape and boxes-only
// scenes (helpers/visualize_scene.py:208-461 with render_type retrieval / txt2shape / onlybox).  The reference works one box
// at a time on the host (helpers/util.py:71-156, :335-421: a JSON file reopened per call, a numpy argmin per box, a trimesh
// copy per object, one trimesh.creation.cylinder per box edge); here three small launches cover all boxes of all scenes:
//   cs_scene_retrieve     get_closest_furniture_to_box (:71-83) for Q boxes: one wave per query strides its category's rows
//                         in ascending order (fp64, numpy's promotion and summation order), candidates replaced on strict <,
//                         then a lexicographic (d2, row) shuffle reduction = np.argmin's first minimum.  No LDS, no atomics.
//   cs_scene_place_boxes  one thread per box: retrieval's placement (:121-129, vertices.dot(R) + t) as the 3x4 map
//                         cs_scene_apply consumes, and the box corners with scene_fit_kernel's own expressions (bit-equal).
//   cs_scene_box_markers  create_bbox_marker (:393-421): one wave per (box, edge) writes a closed prism straight into the
//                         scene buffers cs_scene_apply fills.  The prism's layout is this library's (include/commonscenes_hip.h).
// All three are latency-bound: plain vector loads and stores, fp64 VALU, no MFMA.
#include "cs_common.h"

namespace {

constexpr int RETRIEVE_THREADS = 256;                 // four waves = four queries per workgroup
constexpr int PLACE_THREADS = 256;
constexpr int MARKER_THREADS = 64;                    // one wave per tube
constexpr double PI = 3.14159265358979323846;

__global__ __launch_bounds__(RETRIEVE_THREADS) void scene_retrieve_kernel(
    const double* __restrict__ sizes, int64_t m, const int64_t* __restrict__ cat_base, int ncat,
    const float* __restrict__ boxes, int64_t ld, const int32_t* __restrict__ query_cat, int64_t nq,
    int64_t* __restrict__ index, double* __restrict__ d2out, int32_t* __restrict__ status) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * (RETRIEVE_THREADS / 64) + (threadIdx.x >> 6);
  if (q >= nq) return;                                // (whole waves leave together: q is per wave)
  const float* b = boxes + q * ld;
  const float q0 = b[0], q1 = b[1], q2 = b[2];
  const int cat = query_cat[q];
  int st = 0;
  int64_t lo = 0, hi = 0;
  if (!(fabsf(q0) <= 3.4028234664e38f) || !(fabsf(q1) <= 3.4028234664e38f) || !(fabsf(q2) <= 3.4028234664e38f))
    st |= CS_RETRIEVE_STATUS_NONFINITE;
  if (cat < 0 || cat >= ncat) {
    st |= CS_RETRIEVE_STATUS_CATEGORY;
  } else {
    lo = cat_base[cat];
    hi = cat_base[cat + 1];
    if (lo < 0 || hi > m || lo >= hi) {               // an empty (or malformed) range: nothing is read through it
      st |= CS_RETRIEVE_STATUS_EMPTY;
      lo = hi = 0;
    }
  }
  double best = INFINITY;
  int64_t row = INT64_MAX;
  if (st == 0) {
    const double x0 = (double)q0, x1 = (double)q1, x2 = (double)q2;
    for (int64_t r = lo + lane; r < hi; r += 64) {
      const double* s = sizes + r * 3;
      const double d0 = s[0] - x0, d1 = s[1] - x1, d2c = s[2] - x2;
      const double d2 = (d0 * d0 + d1 * d1) + d2c * d2c;      // np.sum over a last axis of three: ((0 + a0) + a1) + a2
      if (d2 < best) {                                // strict: a lane keeps its first (lowest) row among equals
        best = d2;
        row = r;
      }
    }
    for (int o = 32; o > 0; o >>= 1) {
      const double ob = __shfl_xor(best, o, 64);
      const long long orow = __shfl_xor((long long)row, o, 64);
      if (ob < best || (ob == best && orow < row)) {
        best = ob;
        row = orow;
      }
    }
    if (row == INT64_MAX) st |= CS_RETRIEVE_STATUS_NODISTANCE;   // every distance overflowed or was NaN
  }
  if (lane == 0) {
    index[q] = st ? -1 : row;
    d2out[q] = st ? (double)INFINITY : best;
    status[q] = st;
  }
}

__global__ __launch_bounds__(PLACE_THREADS) void scene_place_kernel(const float* __restrict__ box7, int64_t n, int degrees,
                                                                    float* __restrict__ xform,
                                                                    float* __restrict__ box_points) {
  const int64_t obj = (int64_t)blockIdx.x * PLACE_THREADS + threadIdx.x;
  if (obj >= n) return;
  const float* b = box7 + obj * 7;
  const double dim[3] = {(double)b[0], (double)b[1], (double)b[2]};
  const double t[3] = {(double)b[3], (double)b[4], (double)b[5]};
  double ang = (double)b[6];
  if (degrees) ang = ang * (3.14159265358979323846 / 180.0);      // util.py:121 theta = angle * (np.pi / 180)
  const double cs = cos(ang), sn = sin(ang);
  // the corners: scene_fit_kernel's expressions, term for term (cs_scene.hip)
  float* bp = box_points + obj * 24;
  int q = 0;
  for (int i = -1; i <= 1; i += 2)
    for (int j = 0; j <= 1; ++j)
      for (int k = -1; k <= 1; k += 2, ++q) {
        const double px = dim[0] / 2 * i, py = dim[1] * j, pz = dim[2] / 2 * k;
        bp[q * 3 + 0] = (float)((px * cs + pz * sn) + t[0]);
        bp[q * 3 + 1] = (float)(py + t[1]);
        bp[q * 3 + 2] = (float)((-px * sn + pz * cs) + t[2]);
      }
  // v.dot(R) + t with R = [[c, 0, -s], [0, 1, 0], [s, 0, c]] (:122-129): no scale, no inversion
  const double A[3][4] = {{cs, 0, sn, t[0]}, {0, 1, 0, t[1]}, {-sn, 0, cs, t[2]}};
  float* xf = xform + obj * 12;
  for (int r = 0; r < 3; ++r)
    for (int e = 0; e < 4; ++e) xf[r * 4 + e] = (float)A[r][e];
}

__constant__ int MARKER_EDGES[12][2] = {{0, 1}, {0, 2}, {0, 4}, {1, 3}, {1, 5}, {2, 3},
                                        {2, 6}, {3, 7}, {4, 5}, {4, 6}, {5, 7}, {6, 7}};      // util.py:405

__global__ __launch_bounds__(MARKER_THREADS) void scene_markers_kernel(
    const float* __restrict__ box_points, int64_t n, const uint8_t* __restrict__ keep,
    const int64_t* __restrict__ out_vert_base, const int64_t* __restrict__ out_face_base, const float* __restrict__ color,
    int sections, double radius, float* __restrict__ out_verts, float* __restrict__ out_rgb, int64_t out_nverts,
    int64_t* __restrict__ out_faces, int32_t* __restrict__ face_object, int64_t out_nfaces) {
  const int64_t node = blockIdx.x / 12;
  const int edge = blockIdx.x % 12;
  if (node >= n || !keep[node]) return;
  const int S = sections;
  const int64_t tube_v = 2 * S + 2, tube_f = 4 * S;
  const int64_t nvb = out_vert_base[node], nfb = out_face_base[node];
  // a box whose twelve tubes would leave the buffers is skipped whole
  if (nvb < 0 || nvb > out_nverts || 12 * tube_v > out_nverts - nvb || nfb < 0 || nfb > out_nfaces ||
      12 * tube_f > out_nfaces - nfb)
    return;
  const int64_t vb = nvb + edge * tube_v, fb = nfb + edge * tube_f;
  const float* pa = box_points + node * 24 + MARKER_EDGES[edge][0] * 3;
  const float* pb = box_points + node * 24 + MARKER_EDGES[edge][1] * 3;
  const double a[3] = {(double)pa[0], (double)pa[1], (double)pa[2]};
  const double b[3] = {(double)pb[0], (double)pb[1], (double)pb[2]};
  const double d[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
  const double len = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
  int mi = 0;                                           // the axis of the smallest |d|, lowest index on ties
  if (fabs(d[1]) < fabs(d[mi])) mi = 1;
  if (fabs(d[2]) < fabs(d[mi])) mi = 2;
  double c[3];                                          // d x e_m
  if (mi == 0) {
    c[0] = 0, c[1] = d[2], c[2] = -d[1];
  } else if (mi == 1) {
    c[0] = -d[2], c[1] = 0, c[2] = d[0];
  } else {
    c[0] = d[1], c[1] = -d[0], c[2] = 0;
  }
  const double cl = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
  // zero or non-finite length (or a cross product that under- / overflowed): every vertex collapses onto a
  const bool flat = !(len > 0.0) || !(len <= 1.7976931348623157e308) || !(cl > 0.0) || !(cl <= 1.7976931348623157e308);
  double u[3] = {0, 0, 0}, w[3] = {0, 0, 0};
  if (!flat) {
    const double dn[3] = {d[0] / len, d[1] / len, d[2] / len};
    for (int e = 0; e < 3; ++e) u[e] = c[e] / cl;
    w[0] = dn[1] * u[2] - dn[2] * u[1];
    w[1] = dn[2] * u[0] - dn[0] * u[2];
    w[2] = dn[0] * u[1] - dn[1] * u[0];
  }
  const float cr = color[node * 3 + 0], cg = color[node * 3 + 1], cb = color[node * 3 + 2];
  for (int v = threadIdx.x; v < tube_v; v += MARKER_THREADS) {
    double p[3];
    if (flat) {
      p[0] = a[0], p[1] = a[1], p[2] = a[2];
    } else if (v >= 2 * S) {                            // the cap centres
      const double* e = v == 2 * S ? a : b;
      p[0] = e[0], p[1] = e[1], p[2] = e[2];
    } else {
      const double* e = v < S ? a : b;
      const int k = v < S ? v : v - S;
      const double ang = 2.0 * PI * (double)k / (double)S;
      const double ck = cos(ang), sk = sin(ang);
      for (int x = 0; x < 3; ++x) p[x] = e[x] + radius * (ck * u[x] + sk * w[x]);
    }
    float* o = out_verts + (vb + v) * 3;
    o[0] = (float)p[0];
    o[1] = (float)p[1];
    o[2] = (float)p[2];
    float* oc = out_rgb + (vb + v) * 3;
    oc[0] = cr;
    oc[1] = cg;
    oc[2] = cb;
  }
  for (int f = threadIdx.x; f < tube_f; f += MARKER_THREADS) {
    const int part = f / S, k = f % S, k1 = (k + 1) % S;
    int64_t i0, i1, i2;
    if (part == 0) {                                    // side: (a_k, a_k+1, b_k+1)
      i0 = k, i1 = k1, i2 = S + k1;
    } else if (part == 1) {                             // side: (a_k, b_k+1, b_k)
      i0 = k, i1 = S + k1, i2 = S + k;
    } else if (part == 2) {                             // cap at a, facing -d
      i0 = 2 * S, i1 = k1, i2 = k;
    } else {                                            // cap at b, facing +d
      i0 = 2 * S + 1, i1 = S + k, i2 = S + k1;
    }
    int64_t* o = out_faces + (fb + f) * 3;
    o[0] = vb + i0;
    o[1] = vb + i1;
    o[2] = vb + i2;
    face_object[fb + f] = (int32_t)node;
  }
}

}  // namespace

extern "C" int cs_scene_retrieve(const double* sizes, int64_t m, const int64_t* cat_base, int ncat, const float* boxes,
                                 int64_t ld, const int32_t* query_cat, int64_t nq, int64_t* index, double* d2,
                                 int32_t* status, cs_stream_t stream) {
  if (!sizes || !cat_base || !boxes || !query_cat || !index || !d2 || !status || m <= 0 || ncat <= 0 || ld < 3 || nq <= 0 ||
      nq > (1ll << 31))
    return CS_EINVAL;
  const int per = RETRIEVE_THREADS / 64;
  CS_LAUNCH(scene_retrieve_kernel, dim3((unsigned)((nq + per - 1) / per)), dim3(RETRIEVE_THREADS), 0, (hipStream_t)stream,
            sizes, m, cat_base, ncat, boxes, ld, query_cat, nq, index, d2, status);
  CS_CHECK_LAUNCH();
  return CS_OK;
}

extern "C" int cs_scene_place_boxes(const float* box7, int64_t n, int degrees, float* xform, float* box_points,
                                    cs_stream_t stream) {
  if (!box7 || !xform || !box_points || n <= 0 || n > (1ll << 31)) return CS_EINVAL;
  CS_LAUNCH(scene_place_kernel, dim3((unsigned)((n + PLACE_THREADS - 1) / PLACE_THREADS)), dim3(PLACE_THREADS), 0,
            (hipStream_t)stream, box7, n, degrees, xform, box_points);
  CS_CHECK_LAUNCH();
  return CS_OK;
}

extern "C" int cs_scene_box_markers(const float* box_points, int64_t n, const uint8_t* keep, const int64_t* out_vert_base,
                                    const int64_t* out_face_base, const float* color, int sections, float radius,
                                    float* out_verts, float* out_rgb, int64_t out_nverts, int64_t* out_faces,
                                    int32_t* face_object, int64_t out_nfaces, cs_stream_t stream) {
  if (!box_points || !keep || !out_vert_base || !out_face_base || !color || !out_verts || !out_rgb || !out_faces ||
      !face_object || n <= 0 || n > (1 << 24) || sections < CS_MARKER_MIN_SECTIONS || sections > CS_MARKER_MAX_SECTIONS ||
      !(radius > 0.f) || !(radius <= 3.4028234664e38f) || out_nverts < 0 || out_nfaces < 0)
    return CS_EINVAL;
  CS_LAUNCH(scene_markers_kernel, dim3((unsigned)(n * 12)), dim3(MARKER_THREADS), 0, (hipStream_t)stream, box_points, n, keep,
            out_vert_base, out_face_base, color, sections, (double)radius, out_verts, out_rgb, out_nverts, out_faces,
            face_object, out_nfaces);
  CS_CHECK_LAUNCH();
  return CS_OK;
}
