// Polyline -> triangle-mesh unsigned distance on MI355X: the clearance of a planned path.
// pntf_plan returns waypoints; whether the path between them is collision-free is a question
// about its SEGMENTS (a 0.03-long step passes through a thin wall with both ends clear), which
// the reference never answers (test/gib_plan.py:92-109 and test/arm_plan.py end in an open3d
// viewer).  For each polyline: the exact minimum over its segments and the mesh's triangles of
// the segment -> triangle distance, and the lowest segment index that attains it.
//
// MI355X design: the arm kernel's shape (pntf_arm.hip).  One workgroup owns one polyline
// (grid.x) and one chunk of at most 1024 consecutive segments of it (grid.y); a lane owns four
// CONSECUTIVE segments, i.e. five points in registers, so the five point -> triangle tests
// (tri_d2, the point kernel's bits) serve four segments.  Lanes past the polyline's end repeat
// its last point: zero-length segments, whose distance is that point's own and whose index is
// the last real segment's, so they need no mask in the box, the minimum or the index.  The tile
// loop is the point kernel's (256 triangles per LDS tile, build_record, tri_culled); the
// segment terms are in pntf_path_geom.h.  Only the minimum is wanted, so the culling bound is
// the workgroup's current minimum d^2, lowered by cap^2 and by a relaxed read of what the
// polyline's other chunks have reached.  A planned path spans the scene, so the box a triangle
// is culled against is the WAVE's (its 256 consecutive segments), held in SGPRs: the test stays
// wave-uniform and each wave skips the triangles far from its own stretch of the path
// (the workgroup's box measured slower: DESIGN.md §3).  A triangle that ties
// the minimum is never culled (tri_culled culls with slack), so the lowest index survives too.
// One 64-bit atomicMin per workgroup on the key (fp32 bits of d^2 << 32) | segment index:
// order-preserving for d^2 >= 0, so the result is the exact minimum and the lowest index that
// attains it, independent of the chunking and of the rest of the batch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "pntf.h"
#include "pntf_path_geom.h"

namespace {

using namespace pntf_mesh;

typedef unsigned long long u64;

constexpr int SEGS = PTS;              // segments per lane (consecutive), SEGS + 1 points
constexpr int SPW = BLOCK * SEGS;      // segments per workgroup
constexpr u64 KEY_EMPTY = ((u64)0x7f800000u << 32) | 0xffffffffu;   // d^2 = +inf, where = -1

__device__ __forceinline__ float uniform(float v) {   // wave-uniform value -> SGPR
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}

__device__ __forceinline__ u64 wave_min_key(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 w = __shfl_xor(v, o);
    v = w < v ? w : v;
  }
  return v;
}

__global__ __launch_bounds__(BLOCK) void polyline_mesh_distance_kernel(
    const float* __restrict__ pts, int32_t L, const int32_t* __restrict__ cnt,
    const float* __restrict__ tris, int64_t t, float cap2, u64* __restrict__ acc) {
  __shared__ float4 s_rec[BLOCK * REC];
  __shared__ float s_red[4][8];
  __shared__ u64 s_key[4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t c = blockIdx.x;
  int np = cnt[c];
  np = np < 0 ? 0 : (np > L ? L : np);            // never read past the row
  const int nseg = np - 1;                         // a single point: one zero-length segment
  const int start = blockIdx.y * SPW;              // the chunk's first segment
  const bool single = np == 1 && start == 0;       // one point: chunk 0 treats it
  if (np < 1 || (start >= nseg && !single)) return;   // before any barrier
  const int last_seg = nseg > 0 ? nseg - 1 : 0;

  float px[SEGS + 1], py[SEGS + 1], pz[SEGS + 1];
  const float* row = pts + 3 * c * (int64_t)L;
#pragma unroll
  for (int m = 0; m <= SEGS; ++m) {
    const int i = start + SEGS * (int)threadIdx.x + m;
    const float* p = row + 3 * (int64_t)(i < nseg ? i : nseg);
    px[m] = p[0]; py[m] = p[1]; pz[m] = p[2];
  }
  float dx[SEGS], dy[SEGS], dz[SEGS], idd[SEGS], best[SEGS];
#pragma unroll
  for (int k = 0; k < SEGS; ++k) {
    dx[k] = px[k + 1] - px[k]; dy[k] = py[k + 1] - py[k]; dz[k] = pz[k + 1] - pz[k];
    const float dd = dot3(dx[k], dy[k], dz[k], dx[k], dy[k], dz[k]);
    idd[k] = dd > 0.f ? 1.f / dd : 0.f;
    best[k] = INFINITY;
  }
  // culling box: the wave's own points, wave-uniform
  float lo[3], hi[3];
  {
    float a[3] = {px[0], py[0], pz[0]}, b[3] = {px[0], py[0], pz[0]};
#pragma unroll
    for (int m = 1; m <= SEGS; ++m) {
      a[0] = fminf(a[0], px[m]); a[1] = fminf(a[1], py[m]); a[2] = fminf(a[2], pz[m]);
      b[0] = fmaxf(b[0], px[m]); b[1] = fmaxf(b[1], py[m]); b[2] = fmaxf(b[2], pz[m]);
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      a[d] = wave_min(a[d]);
      b[d] = wave_max(b[d]);
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) { lo[d] = uniform(a[d]); hi[d] = uniform(b[d]); }
  }
  float pext = 0.f;  // largest |coordinate| of the box
  for (int d = 0; d < 3; ++d) pext = fmaxf(pext, fmaxf(fabsf(lo[d]), fabsf(hi[d])));

  for (int64_t base = 0; base < t; base += BLOCK) {
    const int tcnt = (int)(t - base < BLOCK ? t - base : BLOCK);
    float mb = fminf(fminf(best[0], best[1]), fminf(best[2], best[3]));
    mb = wave_min(mb);
    __syncthreads();
    if (threadIdx.x < tcnt)
      build_record(tris + (base + threadIdx.x) * 9, s_rec + REC * threadIdx.x);
    if (lane == 0) s_red[wave][6] = mb;
    // what the polyline's other chunks have reached so far (any earlier value is valid)
    const float other = __uint_as_float((unsigned int)(
        __hip_atomic_load(acc + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> 32));
    __syncthreads();
    float bound = fminf(fminf(s_red[0][6], s_red[1][6]), fminf(s_red[2][6], s_red[3][6]));
    bound = uniform(fminf(bound, fminf(cap2, other)));
    for (int j = 0; j < tcnt; ++j) {
      const float4* r = s_rec + REC * j;
      if (tri_culled(r[8], r[9], lo, hi, pext, bound)) continue;  // exact (pntf_mesh_geom.h)
      float e[SEGS + 1];
#pragma unroll
      for (int m = 0; m <= SEGS; ++m) e[m] = tri_d2(px[m], py[m], pz[m], r);
#pragma unroll
      for (int k = 0; k < SEGS; ++k)
        best[k] = fminf(best[k], seg_tri_d2(px[k], py[k], pz[k], px[k + 1], py[k + 1],
                                            pz[k + 1], dx[k], dy[k], dz[k], idd[k], e[k],
                                            e[k + 1], r));
    }
  }
  static_assert(SEGS == 4, "the minima are written for four segments per lane");
  u64 key = KEY_EMPTY;
#pragma unroll
  for (int k = 0; k < SEGS; ++k) {
    const int i = start + SEGS * (int)threadIdx.x + k;
    const u64 v = ((u64)__float_as_uint(best[k]) << 32) | (unsigned int)(i < last_seg ? i : last_seg);
    key = v < key ? v : key;
  }
  key = wave_min_key(key);
  if (lane == 0) s_key[wave] = key;
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 k01 = s_key[0] < s_key[1] ? s_key[0] : s_key[1];
    u64 k23 = s_key[2] < s_key[3] ? s_key[2] : s_key[3];
    atomicMin(acc + c, k01 < k23 ? k01 : k23);
  }
}

// dist = min(cap, sqrt(d^2)); where = -1 when nothing was found or the cap decided (cap < d).
// A distance equal to a finite cap > 0 to the bit is a tie between the two: dist is the cap
// either way, where may be the segment or -1 (the cap also bounds the culling).
__global__ void polyline_finalize_kernel(const u64* __restrict__ acc, int64_t n, float cap,
                                         float* __restrict__ dist, int32_t* __restrict__ where) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const u64 key = acc[i];
  const float d = sqrtf(__uint_as_float((unsigned int)(key >> 32)));
  dist[i] = fminf(d, cap);
  if (where) where[i] = cap < d ? -1 : (int32_t)(unsigned int)key;
}

}  // namespace

extern "C" {

size_t pntf_polyline_workspace_bytes(int64_t q) { return q > 0 ? (size_t)q * sizeof(u64) : 0; }

int pntf_polyline_mesh_distance(const float* pts, int64_t q, int32_t L, const int32_t* cnt,
                                const float* tris, int64_t t, float cap, float* dist,
                                int32_t* where, void* ws, size_t ws_bytes, hipStream_t stream) {
  if (q < 0 || t < 0 || L < 0)
    return fail("pntf_polyline_mesh_distance: bad arguments (negative size)");
  if (q == 0) return PNTF_OK;
  if (!cnt || !dist || !ws || (L > 0 && !pts))
    return fail("pntf_polyline_mesh_distance: bad arguments (null pointer)");
  if (!(cap >= 0.f))
    return fail("pntf_polyline_mesh_distance: cap must be >= 0 (INFINITY = exact)");
  if (t == 0) return fail("pntf_polyline_mesh_distance: empty mesh");
  if (!tris) return fail("pntf_polyline_mesh_distance: bad arguments (null pointer)");
  if (q > 0x7fffffff) return fail("pntf_polyline_mesh_distance: too many polylines");
  if (ws_bytes < pntf_polyline_workspace_bytes(q))
    return fail("pntf_polyline_mesh_distance: workspace too small "
                "(pntf_polyline_workspace_bytes)");
  if ((uintptr_t)ws % sizeof(u64))
    return fail("pntf_polyline_mesh_distance: workspace must be 8-byte aligned");
  const int64_t chunks = L > 1 ? ((int64_t)L - 1 + SPW - 1) / SPW : (L == 1 ? 1 : 0);
  if (chunks > 65535) return fail("pntf_polyline_mesh_distance: more than 65535 segment chunks");
  u64* acc = reinterpret_cast<u64*>(ws);
  const unsigned g1 = (unsigned)((q + 255) / 256);
  hipLaunchKernelGGL((fill_kernel<u64, KEY_EMPTY>), dim3(g1), dim3(256), 0, stream, acc, q);
  if (chunks > 0)
    hipLaunchKernelGGL(polyline_mesh_distance_kernel, dim3((unsigned)q, (unsigned)chunks),
                       dim3(BLOCK), 0, stream, pts, L, cnt, tris, t, cap * cap, acc);
  hipLaunchKernelGGL(polyline_finalize_kernel, dim3(g1), dim3(256), 0, stream, acc, q, cap, dist,
                     where);
  return check_launch("polyline_mesh_distance_kernel");
}

}  // extern "C"
