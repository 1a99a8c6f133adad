// The exact-coverage triangle rasteriser shared by the top-down scene view (cs_scene.hip) and the per-object views
// (cs_view.hip): vertices snapped to 1/256 pixel, int64 edge functions, top-left rule, perspective-correct fp32 depth and one
// 64-bit atomic min per covered pixel on a key image (depth bits << 32 | face id).  Each user projects its own vertices into
// a Tri (x, y, d), then calls tri_finish once and tri_draw_wave with the whole wave.
#pragma once
#include "cs_common.h"

namespace {

constexpr int RASTER_THREADS = 256;
constexpr int RASTER_OWN_PIXELS = 8;
constexpr int SUB = 256;               // sub-pixel grid: vertices snap to 1/256 pixel
constexpr float SNAP_LIMIT = 2097152.f;   // |pixel coordinate| clamp (2^21): edge functions stay below 2^62 in int64

struct Tri {
  int x[3], y[3];          // snapped to 1/256 pixel; after set-up the winding has positive area
  float d[3];              // depth of the three vertices
  int x0, x1, y0, y1;      // clamped pixel bounding box, inclusive; x1 < x0: nothing to draw
  int64_t area;            // twice the signed area in (1/256 pixel)^2, > 0
};

__device__ __forceinline__ int snap(float pix) {
  pix = fminf(fmaxf(pix, -SNAP_LIMIT), SNAP_LIMIT);
  return (int)floorf(pix * (float)SUB + 0.5f);
}

__device__ __forceinline__ int64_t edge_fn(int ax, int ay, int bx, int by, int px, int py) {
  return (int64_t)(bx - ax) * (int64_t)(py - ay) - (int64_t)(by - ay) * (int64_t)(px - ax);
}

// top-left rule for the positive winding of edge_fn (x right, y down): a top edge runs right, a left edge runs up
__device__ __forceinline__ bool top_left(int ax, int ay, int bx, int by) {
  const int dx = bx - ax, dy = by - ay;
  return (dy == 0 && dx > 0) || dy < 0;
}

__device__ __forceinline__ void tri_clear(Tri& t) {
  t.x0 = 0, t.x1 = -1, t.y0 = 0, t.y1 = -1, t.area = 1;
  for (int i = 0; i < 3; ++i) t.x[i] = t.y[i] = 0, t.d[i] = 1.f;
}

// after x / y / d are filled in: winding, area and the clamped bounding box.  returns 0 drawable, 2 nothing to draw
__device__ __forceinline__ int tri_finish(Tri& t, int size) {
  int64_t area = edge_fn(t.x[0], t.y[0], t.x[1], t.y[1], t.x[2], t.y[2]);
  if (area == 0) return 2;
  if (area < 0) {                                             // both faces are drawn: make the winding positive
    int ti = t.x[1]; t.x[1] = t.x[2]; t.x[2] = ti;
    ti = t.y[1]; t.y[1] = t.y[2]; t.y[2] = ti;
    float tf = t.d[1]; t.d[1] = t.d[2]; t.d[2] = tf;
    area = -area;
  }
  t.area = area;
  const int xmin = min(t.x[0], min(t.x[1], t.x[2])), xmax = max(t.x[0], max(t.x[1], t.x[2]));
  const int ymin = min(t.y[0], min(t.y[1], t.y[2])), ymax = max(t.y[0], max(t.y[1], t.y[2]));
  // pixel p's centre sits at p * 256 + 128: first centre >= min, last centre <= max (arithmetic shifts floor)
  t.x0 = max((xmin - SUB / 2 + SUB - 1) >> 8, 0);
  t.x1 = min((xmax - SUB / 2) >> 8, size - 1);
  t.y0 = max((ymin - SUB / 2 + SUB - 1) >> 8, 0);
  t.y1 = min((ymax - SUB / 2) >> 8, size - 1);
  if (t.x1 < t.x0 || t.y1 < t.y0) {
    t.x1 = t.x0 - 1;
    return 2;
  }
  return 0;
}

__device__ __forceinline__ void tri_pixel(const Tri& t, uint32_t face, int px, int py, int size,
                                          unsigned long long* __restrict__ keys) {
  const int cx = px * SUB + SUB / 2, cy = py * SUB + SUB / 2;
  const int64_t e0 = edge_fn(t.x[1], t.y[1], t.x[2], t.y[2], cx, cy);     // weight of vertex 0
  const int64_t e1 = edge_fn(t.x[2], t.y[2], t.x[0], t.y[0], cx, cy);
  const int64_t e2 = edge_fn(t.x[0], t.y[0], t.x[1], t.y[1], cx, cy);
  const bool in = (e0 > 0 || (e0 == 0 && top_left(t.x[1], t.y[1], t.x[2], t.y[2]))) &&
                  (e1 > 0 || (e1 == 0 && top_left(t.x[2], t.y[2], t.x[0], t.y[0]))) &&
                  (e2 > 0 || (e2 == 0 && top_left(t.x[0], t.y[0], t.x[1], t.y[1])));
  if (!in) return;
  float d = t.d[0];                 // a triangle parallel to the image plane has that depth exactly (so coplanar ones tie)
  if (t.d[0] != t.d[1] || t.d[1] != t.d[2]) {
    const float a = (float)t.area;
    const float inv = (((float)e0 / a) / t.d[0] + ((float)e1 / a) / t.d[1]) + ((float)e2 / a) / t.d[2];
    d = 1.0f / inv;                 // perspective-correct depth, > 0: its bits order like uints
  }
  const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | face;
  unsigned long long* k = keys + (int64_t)py * size + px;
  // keys only ever fall, so a (possibly stale) value already below ours means the atomic would change nothing
  if (__hip_atomic_load(k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= key) return;
  atomicMin(k, key);
}

__device__ __forceinline__ int64_t shfl64(int64_t v, int src) {
  const int lo = __shfl((int)(v & 0xffffffff), src, 64), hi = __shfl((int)(v >> 32), src, 64);
  return ((int64_t)hi << 32) | (uint32_t)lo;
}

// One round of a wave: lane l holds triangle `t` with status `st` (0 drawable) and face id face0 + l.  Must be reached by
// all 64 lanes.  A triangle whose clamped bounding box holds at most RASTER_OWN_PIXELS pixel centres is walked by its own
// lane; the others are taken one after the other by the whole wave (the owner's set-up is broadcast with shuffles).
__device__ __forceinline__ void tri_draw_wave(const Tri& t, int st, int64_t face0, int lane, int size,
                                              unsigned long long* __restrict__ keys) {
  const int64_t npix = st == 0 ? (int64_t)(t.x1 - t.x0 + 1) * (t.y1 - t.y0 + 1) : 0;
  if (npix > 0 && npix <= RASTER_OWN_PIXELS) {
    for (int py = t.y0; py <= t.y1; ++py)
      for (int px = t.x0; px <= t.x1; ++px) tri_pixel(t, (uint32_t)(face0 + lane), px, py, size, keys);
  }
  unsigned long long big = __ballot(npix > RASTER_OWN_PIXELS);
  while (big) {
    const int src = __ffsll((long long)big) - 1;
    big &= big - 1;
    Tri s;
    for (int i = 0; i < 3; ++i) {
      s.x[i] = __shfl(t.x[i], src, 64);
      s.y[i] = __shfl(t.y[i], src, 64);
      s.d[i] = __shfl(t.d[i], src, 64);
    }
    s.x0 = __shfl(t.x0, src, 64), s.x1 = __shfl(t.x1, src, 64);
    s.y0 = __shfl(t.y0, src, 64), s.y1 = __shfl(t.y1, src, 64);
    s.area = shfl64(t.area, src);
    const int w = s.x1 - s.x0 + 1;
    const int64_t n = (int64_t)w * (s.y1 - s.y0 + 1);
    for (int64_t p = lane; p < n; p += 64)
      tri_pixel(s, (uint32_t)(face0 + src), s.x0 + (int)(p % w), s.y0 + (int)(p / w), size, keys);
  }
}

}  // namespace
