// Mesh -> SDF on the MI355X: what the reference reads from `ori_sample_grid.h5` (dataset/threedfront_dataset.py:387-392,
// produced by a preprocessing binary that is not part of it) made from a triangle mesh, after the unit-sphere normalisation of
// util_3d.py:481-512 (get_normalize_mesh).  A packed, ragged batch of B meshes becomes B grids of n^3 nodes:
//   cs_mesh_sdf_moments   area-weighted centroid (fp64, fixed order) and the largest corner distance from it, per mesh
//   cs_mesh_sdf_pack      faces -> one 48-byte record per triangle: corners after (v - centroid) / scale, and the normal
//   cs_mesh_sdf_grid      every node against every triangle of its mesh: min squared distance, solid-angle sum, per slice
//   cs_mesh_sdf_finish    slices merged in slice order, sign from the winding number, truncation
// VALU-bound: no MFMA (the pair evaluation is a region walk, not a product), LDS holds the triangle records, which every lane
// of a wave reads at one address (a broadcast).  No floating-point atomic anywhere: a grid is a pure function of its mesh.
//
// meta (int64 [nb][6], on the device) describes mesh m: vert_base, vert_count, face_base, face_count, slices, ws_offset
// (bytes).  Faces carry mesh-LOCAL vertex ids.  A range that leaves its buffer, a slice count that is not the plan's, or a
// workspace range that leaves the workspace sets CS_SDF_STATUS_RANGE in status[m] and the mesh is skipped whole.
#include "cs_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int MOM_THREADS = 256;
constexpr int MOM_BLOCKS = CS_SDF_MOMENT_BLOCKS;
constexpr int PACK_THREADS = 256;
constexpr int GRID_THREADS = 256;
constexpr int NODES = 4;                      // nodes per lane, along the contiguous (z) axis
constexpr int CHUNK = CS_SDF_CHUNK;           // triangle records per LDS stage
constexpr int REC = 12;                       // floats per record: a, b, c, n = (b - a) x (c - a)
constexpr int MAX_SLICES = CS_SDF_MAX_SLICES;
constexpr float FAR = 1.0e18f;                // a record that contributes nothing: a point this far away, normal 0

// ------------------------------------------------------------------------------------------------------------------ the plan
// The ONE slice rule, on both sides of the launch.  A mesh's triangle range is cut, at chunk granularity, into `slices` equal
// runs of chunks so that a single 64^3 grid (256 workgroups of 1024 nodes) still fills the device; a function of the mesh's
// own face count and n only, so a grid does not depend on its batch.
__host__ __device__ inline int64_t node_groups(int n) { return (int64_t)n * n * ((n + NODES - 1) / NODES); }
__host__ __device__ inline int64_t node_blocks(int n) { return (node_groups(n) + GRID_THREADS - 1) / GRID_THREADS; }
__host__ __device__ inline int plan_slices(int64_t faces, int n, int64_t* chunks_per_slice) {
  const int64_t chunks = (faces + CHUNK - 1) / CHUNK;
  int64_t want = (1024 + node_blocks(n) - 1) / node_blocks(n);      // ~four workgroups per CU of one mesh
  const int64_t by_len = (chunks + 1) / 2;                          // a slice is at least two chunks long
  if (want > by_len) want = by_len;
  if (want > MAX_SLICES) want = MAX_SLICES;
  if (want < 1) want = 1;
  const int64_t cps = (chunks + want - 1) / want;
  if (chunks_per_slice) *chunks_per_slice = cps;
  return (int)((chunks + cps - 1) / cps);                           // no empty slice
}
__host__ __device__ inline int64_t plan_ws_bytes(int slices, int n) {
  const int64_t n3 = (int64_t)n * n * n;
  return ((int64_t)slices * n3 * 12 + 15) / 16 * 16;                // per slice: n^3 doubles (angle sums), n^3 floats (d^2)
}

struct MeshRange {
  int64_t vb, vc, fb, fc, slices, ws_off;
};

// the mesh's ranges, or false (and nothing of the mesh is touched)
__device__ __forceinline__ bool mesh_range(const int64_t* __restrict__ meta, int m, int64_t total_verts, int64_t total_faces,
                                           MeshRange& r) {
  const int64_t* p = meta + (int64_t)m * 6;
  r.vb = p[0], r.vc = p[1], r.fb = p[2], r.fc = p[3], r.slices = p[4], r.ws_off = p[5];
  return r.vb >= 0 && r.vc >= 1 && r.vb <= total_verts && r.vc <= total_verts - r.vb && r.fb >= 0 && r.fc >= 1 &&
         r.fb <= total_faces && r.fc <= total_faces - r.fb;
}

__device__ __forceinline__ bool finite3(float x, float y, float z) {
  return fabsf(x) <= 3.0e38f && fabsf(y) <= 3.0e38f && fabsf(z) <= 3.0e38f;
}

// the three corners of face f of a mesh, or false: an id outside [0, vc) is never dereferenced
__device__ __forceinline__ bool face_corners(const float* __restrict__ verts, const int64_t* __restrict__ faces,
                                             const MeshRange& r, int64_t f, float (&c)[3][3], int& why) {
  const int64_t* id = faces + (r.fb + f) * 3;
  const int64_t i0 = id[0], i1 = id[1], i2 = id[2];
  if (i0 < 0 || i0 >= r.vc || i1 < 0 || i1 >= r.vc || i2 < 0 || i2 >= r.vc) {
    why = CS_SDF_STATUS_INDEX;
    return false;
  }
  const int64_t ids[3] = {i0, i1, i2};
  bool ok = true;
  for (int k = 0; k < 3; ++k) {
    const float* v = verts + (r.vb + ids[k]) * 3;
    c[k][0] = v[0], c[k][1] = v[1], c[k][2] = v[2];
    ok = ok && finite3(v[0], v[1], v[2]);
  }
  if (!ok) why = CS_SDF_STATUS_NONFINITE;
  return ok;
}

// block-wide fp64 sum in a fixed tree; the result is valid in thread 0
template <int THREADS>
__device__ __forceinline__ double block_sum(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = THREADS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  const double s = red[0];
  __syncthreads();
  return s;
}

// ------------------------------------------------------------------------------------------------------------------- moments
// launch 1: block (x, m) sums area and area * triangle-centroid over faces x*256 + t, stepping MOM_BLOCKS*256, in fp64;
// partial[m][x] = (area, sx, sy, sz).  Faces with a bad id or a non-finite corner are left out (pack reports them).
__global__ __launch_bounds__(MOM_THREADS) void sdf_moment_partial_kernel(const float* __restrict__ verts, int64_t total_verts,
                                                                         const int64_t* __restrict__ faces,
                                                                         int64_t total_faces,
                                                                         const int64_t* __restrict__ meta,
                                                                         double* __restrict__ partial) {
  __shared__ double red[MOM_THREADS];
  const int m = blockIdx.y;
  MeshRange r;
  const bool live = mesh_range(meta, m, total_verts, total_faces, r);
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  if (live) {
    for (int64_t f = (int64_t)blockIdx.x * MOM_THREADS + threadIdx.x; f < r.fc; f += (int64_t)MOM_BLOCKS * MOM_THREADS) {
      float c[3][3];
      int why = 0;
      if (!face_corners(verts, faces, r, f, c, why)) continue;
      double e1[3], e2[3];
      for (int a = 0; a < 3; ++a) e1[a] = (double)c[1][a] - (double)c[0][a], e2[a] = (double)c[2][a] - (double)c[0][a];
      const double nx = e1[1] * e2[2] - e1[2] * e2[1], ny = e1[2] * e2[0] - e1[0] * e2[2], nz = e1[0] * e2[1] - e1[1] * e2[0];
      const double area = 0.5 * sqrt((nx * nx + ny * ny) + nz * nz);
      s[0] += area;
      for (int a = 0; a < 3; ++a) s[1 + a] += area * ((((double)c[0][a] + (double)c[1][a]) + (double)c[2][a]) / 3.0);
    }
  }
  for (int a = 0; a < 4; ++a) {
    const double t = block_sum<MOM_THREADS>(s[a], red);
    if (threadIdx.x == 0) partial[((int64_t)m * MOM_BLOCKS + blockIdx.x) * 4 + a] = t;
  }
}

// launch 2: one block per mesh folds the partials in block order, then takes the largest squared corner distance from the
// centroid (a maximum: exact, the order is free).  norm[m] = (cx, cy, cz, scale).  No area, or no extent: CS_SDF_STATUS_EMPTY
// and (0, 0, 0, 1).
__global__ __launch_bounds__(MOM_THREADS) void sdf_moment_final_kernel(const float* __restrict__ verts, int64_t total_verts,
                                                                       const int64_t* __restrict__ faces, int64_t total_faces,
                                                                       const int64_t* __restrict__ meta,
                                                                       const double* __restrict__ partial,
                                                                       double* __restrict__ norm, int32_t* __restrict__ status) {
  __shared__ double red[MOM_THREADS];
  const int m = blockIdx.x;
  MeshRange r;
  const bool live = mesh_range(meta, m, total_verts, total_faces, r);
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int b = 0; b < MOM_BLOCKS; ++b)
    for (int a = 0; a < 4; ++a) s[a] += partial[((int64_t)m * MOM_BLOCKS + b) * 4 + a];      // every thread: the same order
  const bool has_area = live && s[0] > 0.0 && s[0] <= 1.0e300;
  const double cx = has_area ? s[1] / s[0] : 0.0, cy = has_area ? s[2] / s[0] : 0.0, cz = has_area ? s[3] / s[0] : 0.0;
  double mx = 0.0;
  if (has_area) {
    for (int64_t f = threadIdx.x; f < r.fc; f += MOM_THREADS) {
      float c[3][3];
      int why = 0;
      if (!face_corners(verts, faces, r, f, c, why)) continue;
      for (int k = 0; k < 3; ++k) {
        const double x = (double)c[k][0] - cx, y = (double)c[k][1] - cy, z = (double)c[k][2] - cz;
        mx = fmax(mx, (x * x + y * y) + z * z);
      }
    }
  }
  red[threadIdx.x] = mx;
  __syncthreads();
  for (int o = MOM_THREADS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + o]);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double scale = sqrt(red[0]);
    const bool ok = has_area && scale > 0.0 && scale <= 1.0e300;
    double* o = norm + (int64_t)m * 4;
    o[0] = ok ? cx : 0.0, o[1] = ok ? cy : 0.0, o[2] = ok ? cz : 0.0, o[3] = ok ? scale : 1.0;
    if (!live) atomicOr(status + m, CS_SDF_STATUS_RANGE);
    else if (!ok) atomicOr(status + m, CS_SDF_STATUS_EMPTY);
  }
}

// ---------------------------------------------------------------------------------------------------------------------- pack
// One thread per face.  The corners go through (v - centroid) / scale in fp64 and are rounded once; the normal is taken in
// fp64 from the ROUNDED corners.  A triangle whose height is below sqrt(fp32 eps) of its longest edge has no usable fp32
// barycentrics (their cancellation error is eps (L / h)^2): it becomes the segment of its longest edge, written as the
// triangle (p, q, q) with normal 0 -- the region walk below then lands on the segment exactly and the solid angle is 0.
// A point triangle becomes (p, p, p).  A bad id or a non-finite corner writes the far point record and sets its status bit.
__global__ __launch_bounds__(PACK_THREADS) void sdf_pack_kernel(const float* __restrict__ verts, int64_t total_verts,
                                                                const int64_t* __restrict__ faces, int64_t total_faces,
                                                                const int64_t* __restrict__ meta,
                                                                const double* __restrict__ norm, float* __restrict__ tris,
                                                                int32_t* __restrict__ status) {
  const int m = blockIdx.y;
  MeshRange r;
  if (!mesh_range(meta, m, total_verts, total_faces, r)) {
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(status + m, CS_SDF_STATUS_RANGE);
    return;
  }
  const double cx = norm[(int64_t)m * 4 + 0], cy = norm[(int64_t)m * 4 + 1], cz = norm[(int64_t)m * 4 + 2];
  const double sc = norm[(int64_t)m * 4 + 3];
  for (int64_t f = (int64_t)blockIdx.x * PACK_THREADS + threadIdx.x; f < r.fc; f += (int64_t)gridDim.x * PACK_THREADS) {
    float c[3][3];
    int why = 0;
    float rec[REC];
    bool ok = face_corners(verts, faces, r, f, c, why);
    if (ok) {
      const double cen[3] = {cx, cy, cz};
      for (int k = 0; k < 3; ++k)
        for (int a = 0; a < 3; ++a) c[k][a] = (float)(((double)c[k][a] - cen[a]) / sc);
      ok = finite3(c[0][0], c[0][1], c[0][2]) && finite3(c[1][0], c[1][1], c[1][2]) && finite3(c[2][0], c[2][1], c[2][2]);
      if (!ok) why = CS_SDF_STATUS_NONFINITE;
    }
    if (!ok) {
      atomicOr(status + m, why);
      for (int e = 0; e < 9; ++e) rec[e] = FAR;
      rec[9] = rec[10] = rec[11] = 0.f;
    } else {
      // corners in lexicographic order, the orientation kept as a sign on the normal: a mesh with every face reversed packs
      // the same corners and the negated normals, so its distances carry the same bits and its angle sums the opposite sign
      double flip = 1.0;
      auto order = [&](int i, int j) {
        const bool gt = c[i][0] != c[j][0] ? c[i][0] > c[j][0] : (c[i][1] != c[j][1] ? c[i][1] > c[j][1] : c[i][2] > c[j][2]);
        if (gt) {
          for (int a = 0; a < 3; ++a) {
            const float t = c[i][a];
            c[i][a] = c[j][a], c[j][a] = t;
          }
          flip = -flip;
        }
      };
      order(0, 1), order(1, 2), order(0, 1);
      double e[3][3], l2[3];       // edges 0: a->b, 1: b->c, 2: c->a
      for (int k = 0; k < 3; ++k) {
        const int k1 = (k + 1) % 3;
        for (int a = 0; a < 3; ++a) e[k][a] = (double)c[k1][a] - (double)c[k][a];
        l2[k] = (e[k][0] * e[k][0] + e[k][1] * e[k][1]) + e[k][2] * e[k][2];
      }
      const double nx = e[0][1] * (-e[2][2]) - e[0][2] * (-e[2][1]);
      const double ny = e[0][2] * (-e[2][0]) - e[0][0] * (-e[2][2]);
      const double nz = e[0][0] * (-e[2][1]) - e[0][1] * (-e[2][0]);
      const double n2 = (nx * nx + ny * ny) + nz * nz;
      int lk = 0;                  // the longest edge starts at corner lk
      if (l2[1] > l2[lk]) lk = 1;
      if (l2[2] > l2[lk]) lk = 2;
      const double lmax2 = l2[lk];
      if (n2 <= 1.1920929e-7 * lmax2 * lmax2) {       // height^2 = n2 / lmax2 <= eps * lmax2
        const int k1 = (lk + 1) % 3;
        for (int a = 0; a < 3; ++a) rec[a] = c[lk][a], rec[3 + a] = c[k1][a], rec[6 + a] = c[k1][a];
        rec[9] = rec[10] = rec[11] = 0.f;
      } else {
        for (int k = 0; k < 3; ++k)
          for (int a = 0; a < 3; ++a) rec[k * 3 + a] = c[k][a];
        rec[9] = (float)(flip * nx), rec[10] = (float)(flip * ny), rec[11] = (float)(flip * nz);
      }
    }
    float4* o = reinterpret_cast<float4*>(tris + (r.fb + f) * REC);
    o[0] = make_float4(rec[0], rec[1], rec[2], rec[3]);
    o[1] = make_float4(rec[4], rec[5], rec[6], rec[7]);
    o[2] = make_float4(rec[8], rec[9], rec[10], rec[11]);
  }
}

// ---------------------------------------------------------------------------------------------------------------------- grid
// Block (x, s, m): node groups [256 x, 256 x + 256) of mesh m against the chunks of slice s.  A lane owns NODES nodes that
// differ in z only, so the x / y parts of every dot product are shared.  Records are staged through LDS in chunks of CHUNK,
// double-buffered: the next chunk's global loads are issued before the current chunk's arithmetic and land in the other
// buffer after it, one barrier per chunk.
//
// Per pair: Ericson's region walk gives the barycentric pair (v, w) of the closest point q = a + v ab + w ac by selects, the
// squared distance is |v ab + w ac - ap|^2 (a difference of points, never |ap|^2 - projection^2); the solid angle is Van
// Oosterom-Strackee with the numerator ap . n (n = ab x ac from the record: the triple product a . (b x c) of the corner
// vectors, with the terms that cancel removed) and the corner dot products from |ap|^2 - ab . ap and its kin.
// `vc = d1 d4 - d3 d2` and its two kin are NOT fused: for a segment record (a, b, b) both products are the same two numbers and
// the difference must be exactly 0.
__device__ __forceinline__ float rcp_fast(float x) { return __builtin_amdgcn_rcpf(x); }

__global__ __launch_bounds__(GRID_THREADS) void sdf_grid_kernel(const float* __restrict__ tris, int64_t total_faces,
                                                                const int64_t* __restrict__ meta, int n, double origin,
                                                                double step, char* __restrict__ ws, int64_t ws_bytes,
                                                                int32_t* __restrict__ status) {
  __shared__ float4 stage[2][CHUNK * REC / 4];
  const int m = blockIdx.z;
  const int64_t* mp = meta + (int64_t)m * 6;
  const int64_t fb = mp[2], fc = mp[3], slices = mp[4], ws_off = mp[5];
  int64_t cps = 0;
  const bool range_ok = fb >= 0 && fc >= 1 && fb <= total_faces && fc <= total_faces - fb;
  const bool plan_ok = range_ok && slices == plan_slices(fc, n, &cps) && ws_off >= 0 && (ws_off & 15) == 0 &&
                       ws_off <= ws_bytes && plan_ws_bytes((int)slices, n) <= ws_bytes - ws_off;
  if (!plan_ok) {      // (block-uniform: the whole block leaves before any barrier)
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) atomicOr(status + m, CS_SDF_STATUS_RANGE);
    return;
  }
  const int s = blockIdx.y;
  if (s >= slices) return;
  const int64_t f0 = (int64_t)s * cps * CHUNK;
  const int64_t f1 = (f0 + cps * CHUNK < fc) ? f0 + cps * CHUNK : fc;

  const int gpr = (n + NODES - 1) / NODES;
  const int64_t groups = (int64_t)n * n * gpr;
  const int64_t g = (int64_t)blockIdx.x * GRID_THREADS + threadIdx.x;
  const bool lane_live = g < groups;
  const int64_t gc = lane_live ? g : 0;
  const int row = (int)(gc / gpr), k0 = (int)(gc % gpr) * NODES;
  const int ix = row / n, iy = row % n;
  const float px = (float)(origin + ix * step), py = (float)(origin + iy * step);
  float pz[NODES];
#pragma unroll
  for (int j = 0; j < NODES; ++j) {
    const int k = (k0 + j < n) ? k0 + j : n - 1;      // a tail node repeats the last one; it is not stored
    pz[j] = (float)(origin + k * step);
  }
  float best[NODES];
  double wsum[NODES];
#pragma unroll
  for (int j = 0; j < NODES; ++j) best[j] = 3.0e38f, wsum[j] = 0.0;

  // stage loader: chunk of records [c0, c0 + CHUNK) of this slice -> 3 float4 per thread (CHUNK * 3 = 768 = 3 * 256)
  const float4* src = reinterpret_cast<const float4*>(tris + fb * REC);
  constexpr int PER = CHUNK * REC / 4 / GRID_THREADS;
  float4 pre[PER];
  auto fetch = [&](int64_t c0) {
#pragma unroll
    for (int e = 0; e < PER; ++e) {
      const int64_t q = c0 * (REC / 4) + e * GRID_THREADS + threadIdx.x;      // float4 index within the mesh's records
      pre[e] = q < f1 * (REC / 4) ? src[q] : make_float4(FAR, FAR, FAR, FAR);
    }
  };
  fetch(f0);
#pragma unroll
  for (int e = 0; e < PER; ++e) stage[0][e * GRID_THREADS + threadIdx.x] = pre[e];
  __syncthreads();
  int buf = 0;
  for (int64_t c0 = f0; c0 < f1; c0 += CHUNK) {
    const bool more = c0 + CHUNK < f1;
    if (more) fetch(c0 + CHUNK);
    const int cnt = (int)((f1 - c0 < CHUNK) ? f1 - c0 : CHUNK);
    const float4* rec = stage[buf];
    for (int t = 0; t < cnt; ++t) {
      const float4 r0 = rec[t * 3 + 0], r1 = rec[t * 3 + 1], r2 = rec[t * 3 + 2];
      const float ax = r0.x, ay = r0.y, az = r0.z, bx = r0.w, by = r1.x, bz = r1.y, cx = r1.z, cy = r1.w, cz = r2.x;
      const float nx = r2.y, ny = r2.z, nz = r2.w;
      const float abx = bx - ax, aby = by - ay, abz = bz - az, acx = cx - ax, acy = cy - ay, acz = cz - az;
      // parts shared by the lane's nodes (x, y)
      const float apx = px - ax, apy = py - ay, bpx = px - bx, bpy = py - by, cpx = px - cx, cpy = py - cy;
      const float d1xy = fmaf(abx, apx, aby * apy), d2xy = fmaf(acx, apx, acy * apy);
      const float d3xy = fmaf(abx, bpx, aby * bpy), d4xy = fmaf(acx, bpx, acy * bpy);
      const float d5xy = fmaf(abx, cpx, aby * cpy), d6xy = fmaf(acx, cpx, acy * cpy);
      const float aaxy = fmaf(apx, apx, apy * apy), bbxy = fmaf(bpx, bpx, bpy * bpy), ccxy = fmaf(cpx, cpx, cpy * cpy);
      const float numxy = fmaf(apx, nx, apy * ny);
#pragma unroll
      for (int j = 0; j < NODES; ++j) {
        const float apz = pz[j] - az, bpz = pz[j] - bz, cpz = pz[j] - cz;
        const float d1 = fmaf(abz, apz, d1xy), d2 = fmaf(acz, apz, d2xy);
        const float d3 = fmaf(abz, bpz, d3xy), d4 = fmaf(acz, bpz, d4xy);
        const float d5 = fmaf(abz, cpz, d5xy), d6 = fmaf(acz, cpz, d6xy);
        const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
        const float e43 = d4 - d3, e56 = d5 - d6;
        // interior first, then the regions in reverse order of Ericson's early returns: the last assignment wins
        const float den = rcp_fast((va + vb) + vc);
        float v = vb * den, w = vc * den;
        const float tbc = e43 * rcp_fast(e43 + e56);
        const bool r_bc = va <= 0.f && e43 >= 0.f && e56 >= 0.f;
        v = r_bc ? 1.0f - tbc : v, w = r_bc ? tbc : w;
        const bool r_ac = vb <= 0.f && d2 >= 0.f && d6 <= 0.f;
        const float tac = d2 * rcp_fast(d2 - d6);
        v = r_ac ? 0.f : v, w = r_ac ? tac : w;
        const bool r_c = d6 >= 0.f && d5 <= d6;
        v = r_c ? 0.f : v, w = r_c ? 1.f : w;
        const bool r_ab = vc <= 0.f && d1 >= 0.f && d3 <= 0.f;
        const float tab = d1 * rcp_fast(d1 - d3);
        v = r_ab ? tab : v, w = r_ab ? 0.f : w;
        const bool r_b = d3 >= 0.f && d4 <= d3;
        v = r_b ? 1.f : v, w = r_b ? 0.f : w;
        const bool r_a = d1 <= 0.f && d2 <= 0.f;
        v = r_a ? 0.f : v, w = r_a ? 0.f : w;
        const float qx = fmaf(acx, w, fmaf(abx, v, -apx)), qy = fmaf(acy, w, fmaf(aby, v, -apy));
        const float qz = fmaf(acz, w, fmaf(abz, v, -apz));
        const float dd = fmaf(qz, qz, fmaf(qy, qy, qx * qx));
        best[j] = fminf(best[j], dd);
        // solid angle: corner vectors are -ap, -bp, -cp; their triple product is -(ap . n)
        const float aa = fmaf(apz, apz, aaxy), bb = fmaf(bpz, bpz, bbxy), cc = fmaf(cpz, cpz, ccxy);
        const float la = __builtin_amdgcn_sqrtf(aa), lb = __builtin_amdgcn_sqrtf(bb), lc = __builtin_amdgcn_sqrtf(cc);
        const float num = -fmaf(apz, nz, numxy);
        const float ab_ = aa - d1, ca_ = aa - d2, bc_ = bb - e43;      // ap . bp, cp . ap, bp . cp
        const float dn = fmaf(ca_, lb, fmaf(bc_, la, fmaf(ab_, lc, (la * lb) * lc)));
        const float at = num == 0.f ? 0.f : atan2f(num, dn);           // in the triangle's plane: neither side, 0
        wsum[j] += (double)at;
      }
    }
    if (more) {
#pragma unroll
      for (int e = 0; e < PER; ++e) stage[buf ^ 1][e * GRID_THREADS + threadIdx.x] = pre[e];
    }
    __syncthreads();
    buf ^= 1;
  }
  if (!lane_live) return;
  const int64_t n3 = (int64_t)n * n * n;
  double* wpl = reinterpret_cast<double*>(ws + ws_off) + (int64_t)s * n3;
  float* dpl = reinterpret_cast<float*>(ws + ws_off + slices * n3 * 8) + (int64_t)s * n3;
  const int64_t node0 = (int64_t)row * n + k0;
#pragma unroll
  for (int j = 0; j < NODES; ++j) {
    if (k0 + j < n) {
      wpl[node0 + j] = wsum[j];
      dpl[node0 + j] = best[j];
    }
  }
}

// -------------------------------------------------------------------------------------------------------------------- finish
// One thread per node: min of the slices' squared distances, the angle sums added in slice order (fp64), w = sum / 2 pi (each
// term was atan2 = Omega / 2), inside when |w| >= level, value = -+ sqrt(d^2), clamped when truncating.
__global__ __launch_bounds__(256) void sdf_finish_kernel(const char* __restrict__ ws, int64_t ws_bytes,
                                                         const int64_t* __restrict__ meta, int n, int use_sign, float level,
                                                         float trunc, float* __restrict__ out, float* __restrict__ wout) {
  const int m = blockIdx.y;
  const int64_t* mp = meta + (int64_t)m * 6;
  const int64_t fc = mp[3], slices = mp[4], ws_off = mp[5];
  const int64_t n3 = (int64_t)n * n * n;
  const bool plan_ok = fc >= 1 && slices == plan_slices(fc, n, nullptr) && ws_off >= 0 && (ws_off & 15) == 0 &&
                       ws_off <= ws_bytes && plan_ws_bytes((int)slices, n) <= ws_bytes - ws_off;
  const double* wpl = reinterpret_cast<const double*>(ws + (plan_ok ? ws_off : 0));
  const float* dpl = reinterpret_cast<const float*>(ws + (plan_ok ? ws_off + slices * n3 * 8 : 0));
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n3; i += (int64_t)gridDim.x * 256) {
    float val = NAN, wn = NAN;      // a mesh whose plan does not check out (the grid kernel set its status bit): NaN
    if (plan_ok) {
      float d2 = dpl[i];
      double sum = wpl[i];
      for (int64_t s = 1; s < slices; ++s) {
        d2 = fminf(d2, dpl[s * n3 + i]);
        sum += wpl[s * n3 + i];
      }
      const double w = sum / 6.283185307179586476925286766559;
      wn = (float)w;
      const float d = sqrtf(d2);
      val = (use_sign && fabsf(wn) >= level) ? -d : d;
      if (trunc > 0.f) val = fminf(fmaxf(val, -trunc), trunc);
    }
    out[(int64_t)m * n3 + i] = val;
    if (wout) wout[(int64_t)m * n3 + i] = wn;
  }
}

bool batch_ok(int nb, int64_t total_verts, int64_t total_faces) {
  return nb >= 1 && nb <= 65535 && total_verts >= 1 && total_faces >= 1 && total_faces <= (int64_t)1 << 40;
}
bool res_ok(int n) { return n >= 2 && n <= 1024; }

}  // namespace

extern "C" int cs_mesh_sdf_plan(int64_t face_count, int n, int32_t* slices, int64_t* ws_bytes) {
  if (face_count < 1 || !res_ok(n) || !slices || !ws_bytes) return CS_EINVAL;
  *slices = plan_slices(face_count, n, nullptr);
  *ws_bytes = plan_ws_bytes(*slices, n);
  return CS_OK;
}

extern "C" int cs_mesh_sdf_moments(const float* verts, int64_t total_verts, const int64_t* faces, int64_t total_faces,
                                   const int64_t* meta, int nb, double* partial, double* norm, int32_t* status,
                                   cs_stream_t stream) {
  if (!verts || !faces || !meta || !partial || !norm || !status || !batch_ok(nb, total_verts, total_faces)) return CS_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  CS_LAUNCH(sdf_moment_partial_kernel, dim3(MOM_BLOCKS, nb), dim3(MOM_THREADS), 0, s, verts, total_verts, faces, total_faces,
            meta, partial);
  CS_CHECK_LAUNCH();
  CS_LAUNCH(sdf_moment_final_kernel, dim3(nb), dim3(MOM_THREADS), 0, s, verts, total_verts, faces, total_faces, meta, partial,
            norm, status);
  CS_CHECK_LAUNCH();
  return CS_OK;
}

extern "C" int cs_mesh_sdf_pack(const float* verts, int64_t total_verts, const int64_t* faces, int64_t total_faces,
                                const int64_t* meta, int nb, const double* norm, float* tris, int32_t* status,
                                cs_stream_t stream) {
  if (!verts || !faces || !meta || !norm || !tris || !status || !batch_ok(nb, total_verts, total_faces) ||
      ((uintptr_t)tris & 15))
    return CS_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int per_mesh = cs_grid_for((total_faces + nb - 1) / nb, PACK_THREADS, 256);
  CS_LAUNCH(sdf_pack_kernel, dim3(per_mesh, nb), dim3(PACK_THREADS), 0, s, verts, total_verts, faces, total_faces, meta, norm,
            tris, status);
  CS_CHECK_LAUNCH();
  return CS_OK;
}

extern "C" int cs_mesh_sdf_grid(const float* tris, int64_t total_faces, const int64_t* meta, int nb, int n, float bound,
                                int max_slices, void* ws, int64_t ws_bytes, int32_t* status, cs_stream_t stream) {
  if (!tris || !meta || !ws || !status || !batch_ok(nb, 1, total_faces) || !res_ok(n) || !(bound > 0.f) ||
      !(bound <= 3.0e38f) || max_slices < 1 || max_slices > MAX_SLICES || ws_bytes < 16 || ((uintptr_t)tris & 15) ||
      ((uintptr_t)ws & 15))
    return CS_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const double step = 2.0 * (double)bound / (double)(n - 1);
  CS_LAUNCH(sdf_grid_kernel, dim3((unsigned)node_blocks(n), max_slices, nb), dim3(GRID_THREADS), 0, s, tris, total_faces, meta,
            n, -(double)bound, step, (char*)ws, ws_bytes, status);
  CS_CHECK_LAUNCH();
  return CS_OK;
}

extern "C" int cs_mesh_sdf_finish(const void* ws, int64_t ws_bytes, const int64_t* meta, int nb, int n, int use_sign,
                                  float wind_level, float trunc, float* out, float* wout, cs_stream_t stream) {
  if (!ws || !meta || !out || nb < 1 || nb > 65535 || !res_ok(n) || ws_bytes < 16 || ((uintptr_t)ws & 15) ||
      !(wind_level > 0.f) || !(trunc >= 0.f))
    return CS_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int64_t n3 = (int64_t)n * n * n;
  CS_LAUNCH(sdf_finish_kernel, dim3(cs_grid_for(n3, 256, 4096), nb), dim3(256), 0, s, (const char*)ws, ws_bytes, meta, n,
            use_sign, wind_level, trunc, out, wout);
  CS_CHECK_LAUNCH();
  return CS_OK;
}
