// Per-object views on the MI355X: the reference's object renderer (model/diff_utils/util_3d.py:135-189 init_mesh_renderer,
// :350-393 render_sdf / render_meshes; helpers/util.py:242-258 normalize_py3d_meshes), which runs pytorch3d's rasteriser and
// HardPhongShader.  Here a packed, ragged batch of B meshes becomes B images without leaving the device:
//   cs_view_normalize       common centre (fp64, fixed order) and one scale per mesh
//   cs_view_project         [normalise,] look-at perspective camera -> per-vertex snapped screen coordinates and view depth
//   cs_view_vertex_normals  area-weighted vertex normals, accumulated in 64-bit fixed point (bit-reproducible)
//   cs_view_raster          the rasteriser of cs_raster.h, one key image per mesh
//   cs_view_shade           key image -> pix_to_face / zbuf / perspective-correct barycentrics / hard-Phong RGBA
// All of it is HBM- or atomic-bound: no MFMA, LDS only for the reductions, plain vector loads and stores.
// Mesh i owns vert_count[i] vertices from vert_base[i] and face_count[i] faces from face_base[i]; faces carry packed
// (batch-global) vertex ids.  A range that leaves its buffer is skipped whole, a face whose ids leave its mesh's vertex range is
// never dereferenced.
#include "cs_common.h"
#include "cs_raster.h"

namespace {

constexpr int RED_THREADS = 1024;
constexpr int VERT_THREADS = 256;
constexpr int VERT_BLOCKS = 32;        // workgroups per mesh (grid-stride inside the mesh)

__device__ __forceinline__ bool vert_range(const int64_t* __restrict__ base, const int64_t* __restrict__ count, int m,
                                           int64_t total, int64_t& b, int64_t& c) {
  b = base[m], c = count[m];
  if (b < 0 || c < 0 || b > total || c > total - b) {
    b = 0, c = 0;
    return false;
  }
  return true;
}

// ---------------------------------------------------------------------------------------------------------------- normalise
// centre = mean over the vertices of all meshes: every thread sums its strided share in fp64, the 1024 partials are folded in
// a fixed tree, so the result does not depend on scheduling.  One workgroup: a batch is a few hundred thousand vertices.
__global__ __launch_bounds__(RED_THREADS) void view_centre_kernel(const float* __restrict__ verts, int64_t total_verts,
                                                                  const int64_t* __restrict__ vert_base,
                                                                  const int64_t* __restrict__ vert_count, int n,
                                                                  float* __restrict__ centre) {
  double s[3] = {0.0, 0.0, 0.0};
  int64_t cnt = 0;
  for (int m = 0; m < n; ++m) {
    int64_t b, c;
    vert_range(vert_base, vert_count, m, total_verts, b, c);
    cnt += c;
    for (int64_t v = threadIdx.x; v < c; v += RED_THREADS) {
      const float* p = verts + (b + v) * 3;
      s[0] += (double)p[0], s[1] += (double)p[1], s[2] += (double)p[2];
    }
  }
  __shared__ double red[RED_THREADS][3];
  for (int a = 0; a < 3; ++a) red[threadIdx.x][a] = s[a];
  __syncthreads();
  for (int o = RED_THREADS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o)
      for (int a = 0; a < 3; ++a) red[threadIdx.x][a] += red[threadIdx.x + o][a];
    __syncthreads();
  }
  if (threadIdx.x < 3) centre[threadIdx.x] = cnt > 0 ? (float)(red[0][threadIdx.x] / (double)cnt) : 0.f;
}

// one workgroup per mesh: max |v - centre| (exact, so the order is free), then out = (v - centre) / max.  A mesh whose max is
// 0 or not finite collapses to the origin (scale 0): it draws nothing.
__global__ __launch_bounds__(RED_THREADS) void view_normalize_kernel(const float* __restrict__ verts, int64_t total_verts,
                                                                     const int64_t* __restrict__ vert_base,
                                                                     const int64_t* __restrict__ vert_count,
                                                                     const float* __restrict__ centre,
                                                                     float* __restrict__ out) {
  int64_t b, c;
  vert_range(vert_base, vert_count, blockIdx.x, total_verts, b, c);
  const float cx = centre[0], cy = centre[1], cz = centre[2];
  float mx = 0.f;
  bool bad = false;
  for (int64_t v = threadIdx.x; v < c; v += RED_THREADS) {
    const float* p = verts + (b + v) * 3;
    const float x = p[0] - cx, y = p[1] - cy, z = p[2] - cz;
    const float r = sqrtf((x * x + y * y) + z * z);
    bad = bad || !(r <= 3.0e38f);
    mx = fmaxf(mx, r);
  }
  __shared__ float red[RED_THREADS / 64];
  __shared__ int redbad;
  if (threadIdx.x == 0) redbad = 0;
  __syncthreads();
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  if (bad) redbad = 1;
  __syncthreads();
  mx = red[0];
  for (int w = 1; w < RED_THREADS / 64; ++w) mx = fmaxf(mx, red[w]);
  const bool dead = redbad || !(mx > 0.f);
  for (int64_t v = threadIdx.x; v < c; v += RED_THREADS) {
    const float* p = verts + (b + v) * 3;
    float* o = out + (b + v) * 3;
    o[0] = dead ? 0.f : (p[0] - cx) / mx;
    o[1] = dead ? 0.f : (p[1] - cy) / mx;
    o[2] = dead ? 0.f : (p[2] - cz) / mx;
  }
}

// ------------------------------------------------------------------------------------------------------------------ project
struct Cam {
  float m[12];     // row-major 3x4 [R^T | T]: view = m . (p, 1)
};

// +X is left and +Y is up in NDC; pixel (row i, col j) has its centre at NDC (1 - (2j+1)/S, 1 - (2i+1)/S), i.e. the continuous
// pixel coordinate (centres at +0.5) is (1 - ndc) S / 2.  A vertex that is not finite, or at view depth <= 0, gets zview = NaN
// resp. its depth and screen (0, 0): the rasteriser drops its triangles by the depth alone.
__global__ __launch_bounds__(VERT_THREADS) void view_project_kernel(const float* __restrict__ src, int64_t total_verts,
                                                                    const int64_t* __restrict__ vert_base,
                                                                    const int64_t* __restrict__ vert_count, Cam cam,
                                                                    float focal, int size, int copy,
                                                                    float* __restrict__ world, int32_t* __restrict__ screen,
                                                                    float* __restrict__ zview) {
  int64_t b, c;
  vert_range(vert_base, vert_count, blockIdx.y, total_verts, b, c);
  const int64_t step = (int64_t)VERT_BLOCKS * VERT_THREADS;
  for (int64_t v = (int64_t)blockIdx.x * VERT_THREADS + threadIdx.x; v < c; v += step) {
    const float* p = src + (b + v) * 3;
    const float x = p[0], y = p[1], z = p[2];
    if (copy) {
      float* w = world + (b + v) * 3;
      w[0] = x, w[1] = y, w[2] = z;
    }
    const float xv = ((cam.m[0] * x + cam.m[1] * y) + cam.m[2] * z) + cam.m[3];
    const float yv = ((cam.m[4] * x + cam.m[5] * y) + cam.m[6] * z) + cam.m[7];
    float zv = ((cam.m[8] * x + cam.m[9] * y) + cam.m[10] * z) + cam.m[11];
    int sx = 0, sy = 0;
    if (!(fabsf(xv) <= 3.0e38f) || !(fabsf(yv) <= 3.0e38f) || !(fabsf(zv) <= 3.0e38f)) {
      zv = NAN;
    } else if (zv > 0.f) {
      const float half = 0.5f * (float)size;
      sx = snap((1.0f - focal * xv / zv) * half);
      sy = snap((1.0f - focal * yv / zv) * half);
    }
    screen[(b + v) * 2 + 0] = sx;
    screen[(b + v) * 2 + 1] = sy;
    zview[b + v] = zv;
  }
}

// ------------------------------------------------------------------------------------------------------------ vertex normals
// pytorch3d verts_normals_packed: every face adds (v1 - v0) x (v2 - v0) to its three vertices, then normalize(eps 1e-6).
// Float atomics would make the sum depend on the order the faces arrive in; integer adds commute, so the sum is taken in
// 64-bit fixed point.  Scale, per mesh: with e the largest side of the mesh's bounding box, every edge component is at most
// e and every cross-product component at most 2 e^2 =: bound; scale = 2^k with k = 39 - floor(log2(bound)), so one face adds
// less than 2^40 per component (plus the rounding of llrint) and a vertex can collect 2^22 (four million) faces before the
// int64 sum could wrap.  A unit-size marching-cubes mesh at 64^3 has |cross| ~ 2^-12 . bound, i.e. ~2^28 per face: 8 digits.
// bound == 0 or not finite (a point, or a non-finite vertex): scale 0, all normals of that mesh are 0.
__global__ __launch_bounds__(RED_THREADS) void view_normal_scale_kernel(const float* __restrict__ verts, int64_t total_verts,
                                                                        const int64_t* __restrict__ vert_base,
                                                                        const int64_t* __restrict__ vert_count,
                                                                        float* __restrict__ mesh_scale) {
  int64_t b, c;
  vert_range(vert_base, vert_count, blockIdx.x, total_verts, b, c);
  float lo = INFINITY, hi = -INFINITY, ext = 0.f;
  bool bad = false;
  __shared__ float red[RED_THREADS / 64][2];
  __shared__ int redbad;
  if (threadIdx.x == 0) redbad = 0;
  for (int a = 0; a < 3; ++a) {
    lo = INFINITY, hi = -INFINITY;
    for (int64_t v = threadIdx.x; v < c; v += RED_THREADS) {
      const float x = verts[(b + v) * 3 + a];
      bad = bad || !(fabsf(x) <= 3.0e38f);
      lo = fminf(lo, x), hi = fmaxf(hi, x);
    }
    lo = -wave_max(-lo), hi = wave_max(hi);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][0] = lo, red[threadIdx.x >> 6][1] = hi;
    __syncthreads();
    for (int w = 0; w < RED_THREADS / 64; ++w) lo = fminf(lo, red[w][0]), hi = fmaxf(hi, red[w][1]);
    ext = fmaxf(ext, hi - lo);
  }
  if (bad) redbad = 1;
  __syncthreads();
  if (threadIdx.x != 0) return;
  const float bound = 2.f * ext * ext;
  float sc = 0.f;
  if (!redbad && c > 0 && bound > 0.f && bound <= 3.0e38f) {
    int k = 39 - ilogbf(bound);
    k = min(max(k, -126), 127);
    sc = ldexpf(1.f, k);
  }
  mesh_scale[blockIdx.x] = sc;
}

__global__ __launch_bounds__(VERT_THREADS) void view_normal_zero_kernel(unsigned long long* __restrict__ accum,
                                                                        const int64_t* __restrict__ vert_base,
                                                                        const int64_t* __restrict__ vert_count,
                                                                        int64_t total_verts) {
  int64_t b, c;
  vert_range(vert_base, vert_count, blockIdx.y, total_verts, b, c);
  const int64_t step = (int64_t)VERT_BLOCKS * VERT_THREADS;
  for (int64_t v = (int64_t)blockIdx.x * VERT_THREADS + threadIdx.x; v < c * 3; v += step) accum[b * 3 + v] = 0ull;
}

// loads the face's three packed ids; false (nothing dereferenced) unless all lie inside the mesh's own vertex range
__device__ __forceinline__ bool face_ids(const int64_t* __restrict__ faces, int64_t f, int64_t vb, int64_t vc, int64_t id[3]) {
  bool ok = true;
  for (int i = 0; i < 3; ++i) {
    id[i] = faces[f * 3 + i];
    ok = ok && id[i] >= vb && id[i] - vb < vc;
  }
  return ok;
}

__global__ __launch_bounds__(VERT_THREADS) void view_normal_accum_kernel(
    const float* __restrict__ verts, int64_t total_verts, const int64_t* __restrict__ faces, int64_t total_faces,
    const int64_t* __restrict__ vert_base, const int64_t* __restrict__ vert_count, const int64_t* __restrict__ face_base,
    const int64_t* __restrict__ face_count, const float* __restrict__ mesh_scale, unsigned long long* __restrict__ accum) {
  int64_t vb, vc, fb, fc;
  if (!vert_range(vert_base, vert_count, blockIdx.y, total_verts, vb, vc)) return;
  if (!vert_range(face_base, face_count, blockIdx.y, total_faces, fb, fc)) return;
  const double sc = (double)mesh_scale[blockIdx.y];
  if (!(sc > 0.0)) return;
  const int64_t step = (int64_t)VERT_BLOCKS * VERT_THREADS;
  for (int64_t f = (int64_t)blockIdx.x * VERT_THREADS + threadIdx.x; f < fc; f += step) {
    int64_t id[3];
    if (!face_ids(faces, fb + f, vb, vc, id)) continue;
    double p[3][3];
    for (int i = 0; i < 3; ++i)
      for (int a = 0; a < 3; ++a) p[i][a] = (double)verts[id[i] * 3 + a];
    const double ux = p[1][0] - p[0][0], uy = p[1][1] - p[0][1], uz = p[1][2] - p[0][2];
    const double vx = p[2][0] - p[0][0], vy = p[2][1] - p[0][1], vz = p[2][2] - p[0][2];
    const long long q[3] = {llrint((uy * vz - uz * vy) * sc), llrint((uz * vx - ux * vz) * sc),
                            llrint((ux * vy - uy * vx) * sc)};
    for (int i = 0; i < 3; ++i)
      for (int a = 0; a < 3; ++a)
        if (q[a] != 0) atomicAdd(accum + id[i] * 3 + a, (unsigned long long)q[a]);     // two's complement: adds commute
  }
}

__global__ __launch_bounds__(VERT_THREADS) void view_normal_final_kernel(const unsigned long long* __restrict__ accum,
                                                                         const int64_t* __restrict__ vert_base,
                                                                         const int64_t* __restrict__ vert_count,
                                                                         int64_t total_verts,
                                                                         const float* __restrict__ mesh_scale,
                                                                         float* __restrict__ normals) {
  int64_t b, c;
  vert_range(vert_base, vert_count, blockIdx.y, total_verts, b, c);
  const double sc = (double)mesh_scale[blockIdx.y];
  const int64_t step = (int64_t)VERT_BLOCKS * VERT_THREADS;
  for (int64_t v = (int64_t)blockIdx.x * VERT_THREADS + threadIdx.x; v < c; v += step) {
    float n[3] = {0.f, 0.f, 0.f};
    if (sc > 0.0)
      for (int a = 0; a < 3; ++a) n[a] = (float)((double)(long long)accum[(b + v) * 3 + a] / sc);
    const float len = fmaxf(sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]), 1e-6f);     // F.normalize(eps=1e-6)
    for (int a = 0; a < 3; ++a) normals[(b + v) * 3 + a] = n[a] / len;
  }
}

// ----------------------------------------------------------------------------------------------------------------- rasterise
// returns 0 drawable, 1 dropped (a vertex nearer than zmin, or not finite), 2 nothing to draw
__device__ __forceinline__ int view_tri_setup(const int32_t* __restrict__ screen, const float* __restrict__ zview,
                                              const int64_t* __restrict__ faces, int64_t f, int64_t vb, int64_t vc, int size,
                                              float zmin, Tri& t) {
  int64_t id[3];
  if (!face_ids(faces, f, vb, vc, id)) return 2;
  bool behind = false;
  for (int i = 0; i < 3; ++i) {
    const float d = zview[id[i]];
    if (!(d >= zmin) || !(d <= 3.0e38f)) behind = true;
    t.d[i] = d;
    t.x[i] = screen[id[i] * 2 + 0];
    t.y[i] = screen[id[i] * 2 + 1];
  }
  if (behind) return 1;
  return tri_finish(t, size);
}

__global__ __launch_bounds__(256) void view_raster_init_kernel(unsigned long long* __restrict__ keys, int64_t n,
                                                               int32_t* __restrict__ dropped, int nmesh) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) keys[i] = ~0ull;
  if (i < nmesh) dropped[i] = 0;
}

__global__ __launch_bounds__(RASTER_THREADS) void view_raster_kernel(
    const int32_t* __restrict__ screen, const float* __restrict__ zview, int64_t total_verts,
    const int64_t* __restrict__ faces, int64_t total_faces, const int64_t* __restrict__ vert_base,
    const int64_t* __restrict__ vert_count, const int64_t* __restrict__ face_base, const int64_t* __restrict__ face_count,
    int size, float zmin, unsigned long long* __restrict__ keys, int32_t* __restrict__ dropped) {
  const int mesh = blockIdx.y;
  int64_t vb, vc, fb, fc;
  if (!vert_range(vert_base, vert_count, mesh, total_verts, vb, vc)) return;       // (uniform over the workgroup)
  if (!vert_range(face_base, face_count, mesh, total_faces, fb, fc)) return;
  unsigned long long* img = keys + (int64_t)mesh * size * size;                    // a face draws into its own mesh's image only
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * RASTER_THREADS;
  // every lane of a wave runs the same number of rounds (the cooperative part needs the whole wave)
  const int64_t wave_first = (int64_t)blockIdx.x * RASTER_THREADS + (threadIdx.x & ~63);
  int ndrop = 0;
  for (int64_t f0 = wave_first; f0 < fc; f0 += stride) {
    const int64_t f = f0 + lane;
    Tri t;
    int st = 2;
    tri_clear(t);
    if (f < fc) st = view_tri_setup(screen, zview, faces, fb + f, vb, vc, size, zmin, t);
    ndrop += st == 1;
    tri_draw_wave(t, st, fb + f0, lane, size, img);
  }
  for (int o = 32; o > 0; o >>= 1) ndrop += __shfl_xor(ndrop, o, 64);
  if (lane == 0 && ndrop) atomicAdd(dropped + mesh, ndrop);
}

// --------------------------------------------------------------------------------------------------------- resolve and shade
struct Eye {
  float c[3];
};

__device__ __forceinline__ float dot3(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

__device__ __forceinline__ void unit3(float* a) {             // F.normalize(eps=1e-6)
  const float len = fmaxf(sqrtf(dot3(a, a)), 1e-6f);
  a[0] /= len, a[1] /= len, a[2] /= len;
}

// HardPhongShader with pytorch3d's default PointLights / Materials (the reference hands the shader no lights of its own):
// light at (0, 1, 0), ambient 0.5, diffuse 0.3, specular 0.2, shininess 64, material colours 1; hard_rgb_blend on a white
// background; no clamp.
__global__ __launch_bounds__(256) void view_shade_kernel(
    const unsigned long long* __restrict__ keys, const float* __restrict__ world, const float* __restrict__ normals,
    const float* __restrict__ vert_rgb, const int32_t* __restrict__ screen, const float* __restrict__ zview,
    int64_t total_verts, const int64_t* __restrict__ faces, int64_t total_faces, const int64_t* __restrict__ vert_base,
    const int64_t* __restrict__ vert_count, const int64_t* __restrict__ face_base, const int64_t* __restrict__ face_count,
    int size, Eye eye, float* __restrict__ image, int64_t* __restrict__ pix_to_face, float* __restrict__ zbuf,
    float* __restrict__ bary) {
  const int mesh = blockIdx.y;
  const int64_t npix = (int64_t)size * size;
  const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (pix >= npix) return;
  const int64_t i = (int64_t)mesh * npix + pix;
  const unsigned long long key = keys[i];
  const int64_t f = (int64_t)(key & 0xffffffffull);
  float rgba[4] = {1.f, 1.f, 1.f, 0.f}, w[3] = {0.f, 0.f, 0.f}, depth = -1.f;
  int64_t face = -1;
  int64_t vb, vc, fb, fc, id[3];
  const bool ranges = vert_range(vert_base, vert_count, mesh, total_verts, vb, vc) &&
                      vert_range(face_base, face_count, mesh, total_faces, fb, fc);
  if (key != ~0ull && ranges && f >= fb && f - fb < fc && face_ids(faces, f, vb, vc, id)) {
    int x[3], y[3];
    float z[3];
    for (int c = 0; c < 3; ++c) x[c] = screen[id[c] * 2], y[c] = screen[id[c] * 2 + 1], z[c] = zview[id[c]];
    const int px = (int)(pix % size), py = (int)(pix / size);
    const int cx = px * SUB + SUB / 2, cy = py * SUB + SUB / 2;
    // the edge functions coverage used: for a negative winding the rasteriser swapped vertices 1 and 2, which negates all
    // three and the area, so the quotients below are the same numbers
    int64_t area = edge_fn(x[0], y[0], x[1], y[1], x[2], y[2]);
    int64_t e[3] = {edge_fn(x[1], y[1], x[2], y[2], cx, cy), edge_fn(x[2], y[2], x[0], y[0], cx, cy),
                    edge_fn(x[0], y[0], x[1], y[1], cx, cy)};
    if (area < 0) area = -area, e[0] = -e[0], e[1] = -e[1], e[2] = -e[2];
    if (area > 0) {
      face = f;
      depth = __uint_as_float((uint32_t)(key >> 32));
      const float a = (float)area;
      for (int c = 0; c < 3; ++c) w[c] = ((float)e[c] / a) / z[c];
      const float sum = (w[0] + w[1]) + w[2];
      for (int c = 0; c < 3; ++c) w[c] /= sum;
      float tex[3], n[3], p[3];
      for (int a3 = 0; a3 < 3; ++a3) {
        tex[a3] = (w[0] * vert_rgb[id[0] * 3 + a3] + w[1] * vert_rgb[id[1] * 3 + a3]) + w[2] * vert_rgb[id[2] * 3 + a3];
        n[a3] = (w[0] * normals[id[0] * 3 + a3] + w[1] * normals[id[1] * 3 + a3]) + w[2] * normals[id[2] * 3 + a3];
        p[a3] = (w[0] * world[id[0] * 3 + a3] + w[1] * world[id[1] * 3 + a3]) + w[2] * world[id[2] * 3 + a3];
      }
      unit3(n);
      float l[3] = {0.f - p[0], 1.f - p[1], 0.f - p[2]};
      unit3(l);
      const float cosa = dot3(n, l);
      const float diffuse = 0.3f * fmaxf(cosa, 0.f);
      float v[3] = {eye.c[0] - p[0], eye.c[1] - p[1], eye.c[2] - p[2]};
      unit3(v);
      const float r[3] = {-l[0] + 2.f * (cosa * n[0]), -l[1] + 2.f * (cosa * n[1]), -l[2] + 2.f * (cosa * n[2])};
      float s = cosa > 0.f ? fmaxf(dot3(v, r), 0.f) : 0.f;
      for (int k = 0; k < 6; ++k) s *= s;                       // ^64
      const float spec = 0.2f * s;
      for (int c = 0; c < 3; ++c) rgba[c] = (0.5f + diffuse) * tex[c] + spec;
      rgba[3] = 1.f;
    }
  }
  for (int c = 0; c < 4; ++c) image[i * 4 + c] = rgba[c];
  pix_to_face[i] = face;
  zbuf[i] = depth;
  for (int c = 0; c < 3; ++c) bary[i * 3 + c] = w[c];
}

bool batch_ok(int n, int64_t total_verts) { return n > 0 && n <= 65535 && total_verts > 0; }

}  // namespace

extern "C" int cs_view_normalize(const float* verts, int64_t total_verts, const int64_t* vert_base, const int64_t* vert_count,
                                 int n, float* centre, float* out_verts, cs_stream_t stream) {
  if (!verts || !vert_base || !vert_count || !centre || !out_verts || !batch_ok(n, total_verts)) return CS_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  CS_LAUNCH(view_centre_kernel, dim3(1), dim3(RED_THREADS), 0, s, verts, total_verts, vert_base, vert_count, n, centre);
  CS_CHECK_LAUNCH();
  CS_LAUNCH(view_normalize_kernel, dim3(n), dim3(RED_THREADS), 0, s, verts, total_verts, vert_base, vert_count, centre,
            out_verts);
  CS_CHECK_LAUNCH();
  return CS_OK;
}

extern "C" int cs_view_project(const float* verts, int64_t total_verts, const int64_t* vert_base, const int64_t* vert_count,
                               int n, int normalize, const float* cam12, float focal, int size, float* centre, float* world,
                               int32_t* screen, float* zview, cs_stream_t stream) {
  if (!verts || !vert_base || !vert_count || !cam12 || !centre || !world || !screen || !zview || !batch_ok(n, total_verts) ||
      size <= 0 || size > 8192 || !(focal > 0.f) || world == verts)
    return CS_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (normalize) {
    const int rc = cs_view_normalize(verts, total_verts, vert_base, vert_count, n, centre, world, stream);
    if (rc != CS_OK) return rc;
  }
  Cam cam;
  for (int e = 0; e < 12; ++e) cam.m[e] = cam12[e];
  CS_LAUNCH(view_project_kernel, dim3(VERT_BLOCKS, n), dim3(VERT_THREADS), 0, s, normalize ? (const float*)world : verts,
            total_verts, vert_base, vert_count, cam, focal, size, normalize ? 0 : 1, world, screen, zview);
  CS_CHECK_LAUNCH();
  return CS_OK;
}

extern "C" int cs_view_vertex_normals(const float* verts, int64_t total_verts, const int64_t* faces, int64_t total_faces,
                                      const int64_t* vert_base, const int64_t* vert_count, const int64_t* face_base,
                                      const int64_t* face_count, int n, int64_t* accum, float* mesh_scale, float* normals,
                                      cs_stream_t stream) {
  if (!verts || !faces || !vert_base || !vert_count || !face_base || !face_count || !accum || !mesh_scale || !normals ||
      !batch_ok(n, total_verts) || total_faces <= 0)
    return CS_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* acc = (unsigned long long*)accum;
  CS_LAUNCH(view_normal_scale_kernel, dim3(n), dim3(RED_THREADS), 0, s, verts, total_verts, vert_base, vert_count, mesh_scale);
  CS_CHECK_LAUNCH();
  CS_LAUNCH(view_normal_zero_kernel, dim3(VERT_BLOCKS, n), dim3(VERT_THREADS), 0, s, acc, vert_base, vert_count, total_verts);
  CS_CHECK_LAUNCH();
  CS_LAUNCH(view_normal_accum_kernel, dim3(VERT_BLOCKS, n), dim3(VERT_THREADS), 0, s, verts, total_verts, faces, total_faces,
            vert_base, vert_count, face_base, face_count, mesh_scale, acc);
  CS_CHECK_LAUNCH();
  CS_LAUNCH(view_normal_final_kernel, dim3(VERT_BLOCKS, n), dim3(VERT_THREADS), 0, s, acc, vert_base, vert_count, total_verts,
            mesh_scale, normals);
  CS_CHECK_LAUNCH();
  return CS_OK;
}

extern "C" int cs_view_raster(const int32_t* screen, const float* zview, int64_t total_verts, const int64_t* faces,
                              int64_t total_faces, const int64_t* vert_base, const int64_t* vert_count,
                              const int64_t* face_base, const int64_t* face_count, int n, int size, float zmin, uint64_t* keys,
                              int32_t* dropped, cs_stream_t stream) {
  if (!screen || !zview || !faces || !vert_base || !vert_count || !face_base || !face_count || !keys || !dropped ||
      !batch_ok(n, total_verts) || total_faces <= 0 || total_faces > 0x7fffffffll || size <= 0 || size > 8192 ||
      !(zmin > 0.f) || (int64_t)n * size * size > 0x7fffffffll * 256)
    return CS_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int64_t nkeys = (int64_t)n * size * size;
  CS_LAUNCH(view_raster_init_kernel, dim3((unsigned)((nkeys + 255) / 256)), dim3(256), 0, s, (unsigned long long*)keys, nkeys,
            dropped, n);
  CS_CHECK_LAUNCH();
  // workgroups per mesh: enough for the mean face count, capped; each grid-strides its mesh's faces
  const int per_mesh = cs_grid_for((total_faces + n - 1) / n, RASTER_THREADS, 64);
  CS_LAUNCH(view_raster_kernel, dim3(per_mesh, n), dim3(RASTER_THREADS), 0, s, screen, zview, total_verts, faces, total_faces,
            vert_base, vert_count, face_base, face_count, size, zmin, (unsigned long long*)keys, dropped);
  CS_CHECK_LAUNCH();
  return CS_OK;
}

extern "C" int cs_view_shade(const uint64_t* keys, const float* world, const float* normals, const float* vert_rgb,
                             const int32_t* screen, const float* zview, int64_t total_verts, const int64_t* faces,
                             int64_t total_faces, const int64_t* vert_base, const int64_t* vert_count,
                             const int64_t* face_base, const int64_t* face_count, int n, int size, const float* eye3,
                             float* image, int64_t* pix_to_face, float* zbuf, float* bary, cs_stream_t stream) {
  if (!keys || !world || !normals || !vert_rgb || !screen || !zview || !faces || !vert_base || !vert_count || !face_base ||
      !face_count || !eye3 || !image || !pix_to_face || !zbuf || !bary || !batch_ok(n, total_verts) || total_faces <= 0 ||
      total_faces > 0x7fffffffll || size <= 0 || size > 8192)
    return CS_EINVAL;
  Eye eye;
  for (int a = 0; a < 3; ++a) eye.c[a] = eye3[a];
  const int64_t npix = (int64_t)size * size;
  CS_LAUNCH(view_shade_kernel, dim3((unsigned)((npix + 255) / 256), n), dim3(256), 0, (hipStream_t)stream,
            (const unsigned long long*)keys, world, normals, vert_rgb, screen, zview, total_verts, faces, total_faces, vert_base,
            vert_count, face_base, face_count, size, eye, image, pix_to_face, zbuf, bary);
  CS_CHECK_LAUNCH();
  return CS_OK;
}
