// Scene assembly and the top-down view on the MI355X: the "post" side of the sampling path.
// The reference does this per object on the host right after sampling (helpers/visualize_scene.py:378-461 render_v2_full ->
// helpers/util.py:298-332 get_generated_models_v2 -> :158-189 fit_shapes_to_box_v2; :57-81 create_floor; :85-116 render_img
// with trimesh + pyrender).  Here the meshes never leave the device:
//   cs_scene_fit_boxes       per object: vertex bounds (one 1024-thread workgroup strides the object's vertices; min / max
//                            are exact, so the order is free), then ONE thread restates util.py:158-189 in fp64 as a 3x4
//                            affine map, rounded once to fp32, plus the box corners (:162-166, :186-188)
//   cs_scene_apply           one pass over the kept objects: out = A v + t (fp32, fixed order, no contraction), faces
//                            rebased to scene-global ids (winding reversed on `flip`), face -> object, vertex colours
//   cs_scene_raster_topdown  render_img's camera; exact integer coverage, one 64-bit atomic min per covered pixel
//   cs_scene_resolve         key image -> depth / object id / shaded rgb
// All four are HBM- or atomic-bound: no MFMA, no LDS beyond the bounds reduction, plain vector loads and stores.
//
// Work split of the rasteriser (generated triangles are a pixel or smaller, the floor quad covers most of the image): a wave
// takes 64 triangles at a time, one per lane, and every lane sets its own triangle up.  A triangle whose clamped bounding box
// holds at most RASTER_OWN_PIXELS pixel centres is walked by its own lane; the others are taken one after the other by the
// WHOLE wave (the owner's set-up is broadcast with shuffles, the 64 lanes stride the bounding box).  The key image makes the
// result independent of which path, wave or launch order drew a pixel.
#include "cs_common.h"
#include "cs_raster.h"

namespace {

constexpr int FIT_THREADS = 1024;
constexpr int APPLY_THREADS = 256;
constexpr int APPLY_BLOCKS = 32;       // workgroups per object (grid-stride inside the object)

__global__ __launch_bounds__(FIT_THREADS) void scene_fit_kernel(const float* __restrict__ verts, int64_t total_verts,
                                                                const int64_t* __restrict__ vert_base,
                                                                const int64_t* __restrict__ vert_count,
                                                                const float* __restrict__ box7, int degrees,
                                                                float* __restrict__ xform, float* __restrict__ box_points) {
  const int obj = blockIdx.x;
  const int64_t base = vert_base[obj];
  int64_t cnt = vert_count[obj];
  if (cnt < 0 || base < 0 || base > total_verts || cnt > total_verts - base) cnt = 0;   // never read outside `verts`
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int64_t v = threadIdx.x; v < cnt; v += FIT_THREADS) {
    const float* p = verts + (base + v) * 3;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      lo[a] = fminf(lo[a], p[a]);
      hi[a] = fmaxf(hi[a], p[a]);
    }
  }
  __shared__ float red[FIT_THREADS / 64][6];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    for (int o = 32; o > 0; o >>= 1) {
      lo[a] = fminf(lo[a], __shfl_xor(lo[a], o, 64));
      hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], o, 64));
    }
  }
  if ((threadIdx.x & 63) == 0) {
    for (int a = 0; a < 3; ++a) {
      red[threadIdx.x >> 6][a] = lo[a];
      red[threadIdx.x >> 6][3 + a] = hi[a];
    }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int w = 1; w < FIT_THREADS / 64; ++w) {
    for (int a = 0; a < 3; ++a) {
      lo[a] = fminf(lo[a], red[w][a]);
      hi[a] = fmaxf(hi[a], red[w][3 + a]);
    }
  }
  const float* b = box7 + (int64_t)obj * 7;
  const double dim[3] = {(double)b[0], (double)b[1], (double)b[2]};
  const double t[3] = {(double)b[3], (double)b[4], (double)b[5]};
  double ang = (double)b[6];
  if (degrees) ang = ang * (3.14159265358979323846 / 180.0);      // np.deg2rad
  const double cs = cos(ang), sn = sin(ang);                       // get_rotation_3dfront: [[c,0,-s],[0,1,0],[s,0,c]]
  // corners (:162-166) . R + t (:186-188)
  float* bp = box_points + (int64_t)obj * 24;
  int q = 0;
  for (int i = -1; i <= 1; i += 2)
    for (int j = 0; j <= 1; ++j)
      for (int k = -1; k <= 1; k += 2, ++q) {
        const double px = dim[0] / 2 * i, py = dim[1] * j, pz = dim[2] / 2 * k;
        bp[q * 3 + 0] = (float)((px * cs + pz * sn) + t[0]);
        bp[q * 3 + 1] = (float)(py + t[1]);
        bp[q * 3 + 2] = (float)((-px * sn + pz * cs) + t[2]);
      }
  float* xf = xform + (int64_t)obj * 12;
  if (cnt == 0) {                                                  // nothing to fit: identity
    for (int e = 0; e < 12; ++e) xf[e] = (e % 5 == 0) ? 1.f : 0.f;
    return;
  }
  const double l0[3] = {(double)lo[0], (double)lo[1], (double)lo[2]}, h0[3] = {(double)hi[0], (double)hi[1], (double)hi[2]};
  double c[3];
  for (int a = 0; a < 3; ++a) c[a] = l0[a] + (h0[a] - l0[a]) / 2;   // bounds[0] + extents / 2 of the UNROTATED bounds
  c[1] = l0[1];
  // v1 = P v - c with P (x,y,z) -> (-z,y,x); extent of v1 per axis, from lo / hi
  const double s[3] = {(-l0[2] - c[0]) - (-h0[2] - c[0]), (h0[1] - c[1]) - (l0[1] - c[1]), (h0[0] - c[2]) - (l0[0] - c[2])};
  double k[3];
  for (int a = 0; a < 3; ++a) k[a] = s[a] > 0 ? dim[a] / s[a] : 0.0;   // zero extent: the coordinate maps to 0
  // v3 = R^T diag(k) (P v - c) + t
  double A[3][4] = {{sn * k[2], 0, -cs * k[0], (-cs * k[0] * c[0] - sn * k[2] * c[2]) + t[0]},
                    {0, k[1], 0, -k[1] * c[1] + t[1]},
                    {cs * k[2], 0, sn * k[0], (sn * k[0] * c[0] - cs * k[2] * c[2]) + t[2]}};
  for (int r = 0; r < 3; ++r)
    for (int e = 0; e < 4; ++e) xf[r * 4 + e] = (float)A[r][e];
}

__global__ __launch_bounds__(APPLY_THREADS) void scene_apply_kernel(
    const float* __restrict__ verts, int64_t total_verts, const int64_t* __restrict__ faces, int64_t total_faces,
    const int64_t* __restrict__ vert_base, const int64_t* __restrict__ vert_count, const int64_t* __restrict__ face_base,
    const int64_t* __restrict__ face_count, const float* __restrict__ xform, const uint8_t* __restrict__ keep,
    const int64_t* __restrict__ out_vert_base, const int64_t* __restrict__ out_face_base, const float* __restrict__ color,
    int flip, float* __restrict__ out_verts, float* __restrict__ out_rgb, int64_t out_nverts,
    int64_t* __restrict__ out_faces, int32_t* __restrict__ face_object, int64_t out_nfaces) {
  const int obj = blockIdx.y;
  if (!keep[obj]) return;
  const int64_t vb = vert_base[obj], vc = vert_count[obj], fb = face_base[obj], fc = face_count[obj];
  const int64_t ovb = out_vert_base[obj], ofb = out_face_base[obj];
  // an object whose ranges leave the buffers is skipped whole: nothing is read or written outside them
  if (vb < 0 || vc < 0 || vb > total_verts || vc > total_verts - vb || fb < 0 || fc < 0 || fb > total_faces ||
      fc > total_faces - fb || ovb < 0 || ovb > out_nverts || vc > out_nverts - ovb || ofb < 0 || ofb > out_nfaces ||
      fc > out_nfaces - ofb)
    return;
  const float* xf = xform + (int64_t)obj * 12;
  float A[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) A[e] = xf[e];
  const float cr = color[obj * 3 + 0], cg = color[obj * 3 + 1], cb = color[obj * 3 + 2];
  const int64_t step = (int64_t)APPLY_BLOCKS * APPLY_THREADS, first = (int64_t)blockIdx.x * APPLY_THREADS + threadIdx.x;
  for (int64_t v = first; v < vc; v += step) {
    const float* p = verts + (vb + v) * 3;
    const float x = p[0], y = p[1], z = p[2];
    float* o = out_verts + (ovb + v) * 3;
    o[0] = ((A[0] * x + A[1] * y) + A[2] * z) + A[3];
    o[1] = ((A[4] * x + A[5] * y) + A[6] * z) + A[7];
    o[2] = ((A[8] * x + A[9] * y) + A[10] * z) + A[11];
    float* c = out_rgb + (ovb + v) * 3;
    c[0] = cr;
    c[1] = cg;
    c[2] = cb;
  }
  for (int64_t f = first; f < fc; f += step) {
    const int64_t* p = faces + (fb + f) * 3;
    const int64_t a = p[0] + ovb, b = p[1] + ovb, c = p[2] + ovb;
    int64_t* o = out_faces + (ofb + f) * 3;
    o[0] = flip ? c : a;                   // trimesh invert(): fliplr(faces)
    o[1] = b;
    o[2] = flip ? a : c;
    face_object[ofb + f] = obj;
  }
}

// returns 0 drawable, 1 dropped (a vertex nearer than znear, or not finite), 2 nothing to draw
__device__ int tri_setup(const float* __restrict__ verts, int64_t nverts, const int64_t* __restrict__ faces, int64_t f,
                         int size, float znear, Tri& t) {
  t.x0 = 0, t.x1 = -1, t.y0 = 0, t.y1 = -1, t.area = 1;
  bool behind = false;
  for (int i = 0; i < 3; ++i) {
    const int64_t id = faces[f * 3 + i];
    if (id < 0 || id >= nverts) return 2;                     // malformed index: never dereferenced
    const float x = verts[id * 3 + 0], y = verts[id * 3 + 1], z = verts[id * 3 + 2];
    const float d = 8.0f - y;
    if (!(d >= znear) || !(fabsf(x) <= 3.0e38f) || !(fabsf(z) <= 3.0e38f) || !(d <= 3.0e38f)) {
      behind = true;
      continue;
    }
    t.d[i] = d;
    t.x[i] = snap((1.0f + x / d) * 0.5f * (float)size);
    t.y[i] = snap((1.0f + z / d) * 0.5f * (float)size);
  }
  if (behind) return 1;
  return tri_finish(t, size);
}

__global__ __launch_bounds__(RASTER_THREADS) void scene_raster_kernel(const float* __restrict__ verts, int64_t nverts,
                                                                      const int64_t* __restrict__ faces, int64_t nfaces,
                                                                      int size, float znear,
                                                                      unsigned long long* __restrict__ keys,
                                                                      int32_t* __restrict__ dropped) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * RASTER_THREADS;
  // every lane of a wave runs the same number of rounds (the cooperative part needs the whole wave)
  const int64_t wave_first = (int64_t)blockIdx.x * RASTER_THREADS + (threadIdx.x & ~63);
  int ndrop = 0;
  for (int64_t f0 = wave_first; f0 < nfaces; f0 += stride) {
    const int64_t f = f0 + lane;
    Tri t;
    int st = 2;
    tri_clear(t);
    if (f < nfaces) st = tri_setup(verts, nverts, faces, f, size, znear, t);
    ndrop += st == 1;
    tri_draw_wave(t, st, f0, lane, size, keys);
  }
  for (int o = 32; o > 0; o >>= 1) ndrop += __shfl_xor(ndrop, o, 64);
  if (lane == 0 && ndrop) atomicAdd(dropped, ndrop);
}

__global__ __launch_bounds__(256) void scene_raster_init_kernel(unsigned long long* __restrict__ keys, int64_t n,
                                                                int32_t* __restrict__ dropped) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) keys[i] = ~0ull;
  if (i == 0) *dropped = 0;
}

__global__ __launch_bounds__(256) void scene_resolve_kernel(const unsigned long long* __restrict__ keys,
                                                            const float* __restrict__ verts, int64_t nverts,
                                                            const int64_t* __restrict__ faces, int64_t nfaces,
                                                            const float* __restrict__ vert_rgb,
                                                            const int32_t* __restrict__ face_object, int size,
                                                            float* __restrict__ depth, int32_t* __restrict__ object_id,
                                                            uint8_t* __restrict__ rgb) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)size * size) return;
  const unsigned long long key = keys[i];
  const int64_t f = (int64_t)(key & 0xffffffffull);
  float d = INFINITY, col[3] = {255.f, 255.f, 255.f};
  int oid = -1;
  if (key != ~0ull && f < nfaces) {
    int64_t id[3];
    bool ok = true;
    for (int c = 0; c < 3; ++c) {
      id[c] = faces[f * 3 + c];
      ok = ok && id[c] >= 0 && id[c] < nverts;
    }
    if (ok) {
      d = __uint_as_float((uint32_t)(key >> 32));
      oid = face_object[f];
      float p[3][3];
      for (int c = 0; c < 3; ++c)
        for (int a = 0; a < 3; ++a) p[c][a] = verts[id[c] * 3 + a];
      const float ux = p[1][0] - p[0][0], uy = p[1][1] - p[0][1], uz = p[1][2] - p[0][2];
      const float vx = p[2][0] - p[0][0], vy = p[2][1] - p[0][1], vz = p[2][2] - p[0][2];
      const float nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
      const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
      const float facing = len > 0.f ? fmaxf(ny / len, 0.f) : 0.f;      // the camera looks along -y
      const float shade = 0.3f + 0.7f * facing;
      for (int c = 0; c < 3; ++c) {
        const float v = vert_rgb[id[0] * 3 + c] * shade * 255.f;       // one colour per object: any corner's
        col[c] = fminf(fmaxf(floorf(v + 0.5f), 0.f), 255.f);
      }
    }
  }
  depth[i] = d;
  object_id[i] = oid;
  for (int c = 0; c < 3; ++c) rgb[i * 3 + c] = (uint8_t)col[c];
}

}  // namespace

extern "C" int cs_scene_fit_boxes(const float* verts, int64_t total_verts, const int64_t* vert_base,
                                  const int64_t* vert_count, const float* box7, int n, int degrees, float* xform,
                                  float* box_points, cs_stream_t stream) {
  if (!verts || !vert_base || !vert_count || !box7 || !xform || !box_points || n <= 0 || n > 65535 || total_verts < 0)
    return CS_EINVAL;
  CS_LAUNCH(scene_fit_kernel, dim3(n), dim3(FIT_THREADS), 0, (hipStream_t)stream, verts, total_verts, vert_base, vert_count,
            box7, degrees, xform, box_points);
  CS_CHECK_LAUNCH();
  return CS_OK;
}

extern "C" int cs_scene_apply(const float* verts, int64_t total_verts, const int64_t* faces, int64_t total_faces,
                              const int64_t* vert_base, const int64_t* vert_count, const int64_t* face_base,
                              const int64_t* face_count, const float* xform, const uint8_t* keep,
                              const int64_t* out_vert_base, const int64_t* out_face_base, const float* color, int n, int flip,
                              float* out_verts, float* out_rgb, int64_t out_nverts, int64_t* out_faces, int32_t* face_object,
                              int64_t out_nfaces, cs_stream_t stream) {
  if (!verts || !faces || !vert_base || !vert_count || !face_base || !face_count || !xform || !keep || !out_vert_base ||
      !out_face_base || !color || !out_verts || !out_rgb || !out_faces || !face_object || n <= 0 || n > 65535 ||
      total_verts < 0 || total_faces < 0 || out_nverts < 0 || out_nfaces < 0)
    return CS_EINVAL;
  CS_LAUNCH(scene_apply_kernel, dim3(APPLY_BLOCKS, n), dim3(APPLY_THREADS), 0, (hipStream_t)stream, verts, total_verts, faces,
            total_faces, vert_base, vert_count, face_base, face_count, xform, keep, out_vert_base, out_face_base, color, flip,
            out_verts, out_rgb, out_nverts, out_faces, face_object, out_nfaces);
  CS_CHECK_LAUNCH();
  return CS_OK;
}

extern "C" int cs_scene_raster_topdown(const float* verts, int64_t nverts, const int64_t* faces, int64_t nfaces, int size,
                                       float znear, uint64_t* keys, int32_t* dropped, cs_stream_t stream) {
  if (!verts || !faces || !keys || !dropped || nverts <= 0 || nfaces <= 0 || nfaces > 0x7fffffffll || size <= 0 ||
      size > 8192 || !(znear > 0.f))
    return CS_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int64_t npix = (int64_t)size * size;
  CS_LAUNCH(scene_raster_init_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, (unsigned long long*)keys, npix,
            dropped);
  CS_CHECK_LAUNCH();
  CS_LAUNCH(scene_raster_kernel, dim3(cs_grid_for(nfaces, RASTER_THREADS, 256 * 8)), dim3(RASTER_THREADS), 0, s, verts,
            nverts, faces, nfaces, size, znear, (unsigned long long*)keys, dropped);
  CS_CHECK_LAUNCH();
  return CS_OK;
}

extern "C" int cs_scene_resolve(const uint64_t* keys, const float* verts, int64_t nverts, const int64_t* faces,
                                int64_t nfaces, const float* vert_rgb, const int32_t* face_object, int size, float* depth,
                                int32_t* object_id, uint8_t* rgb, cs_stream_t stream) {
  if (!keys || !verts || !faces || !vert_rgb || !face_object || !depth || !object_id || !rgb || nverts <= 0 ||
      nfaces <= 0 || nfaces > 0x7fffffffll || size <= 0 || size > 8192)
    return CS_EINVAL;
  const int64_t npix = (int64_t)size * size;
  CS_LAUNCH(scene_resolve_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
            (const unsigned long long*)keys, verts, nverts, faces, nfaces, vert_rgb, face_object, size, depth, object_id, rgb);
  CS_CHECK_LAUNCH();
  return CS_OK;
}
