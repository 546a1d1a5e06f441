// Point -> triangle-mesh unsigned distance on MI355X: the query the
// speed-sample generator makes for every sampled start / goal point,
// `point_obstacle_distance` (dataprocessing/speed_sampling_gpu.py:325-336), which the
// reference answers with the un-vendored CUDA extension bvh_distance_queries
// (.gitmodules:1-3, github.com/YuliangXiu/bvh-distance-queries, no pinned commit): a BVH
// over the triangles, exact closest point per (point, triangle), squared distance out,
// `torch.sqrt` in the caller (:334).
//
// MI355X design: the meshes here are the scaled Gibson obstacle meshes (10^3..10^5
// triangles) and a sampling round queries 8·numsamples points, so the work is a dense
// (points x triangles) min-reduction, VALU-bound, not a pointer-chasing tree walk.  Each
// workgroup owns 1024 points (four per lane, in registers) and a contiguous chunk of
// triangles, which it stages through LDS 256 at a time as precomputed records (edges,
// inverse edge lengths, unit normal, in-plane edge normals); every lane then reads the same
// record (LDS broadcast, conflict-free) and runs a branch-free distance (no divergence).  When the point grid alone cannot fill 256 CUs
// the triangle range is split over grid.y and the chunks combine with a global unsigned
// atomic min on the fp32 bit pattern of d^2 (order-preserving for d^2 >= 0, so the result
// is the exact minimum, independent of chunk order); a finalize pass takes the sqrt.
//
// Closest point on a triangle: the Voronoi regions of Ericson, "Real-Time Collision
// Detection" §5.1.5 (the algorithm bvh_distance_queries' device code uses) in a branch-free
// form — plane distance when the projection is inside, else the nearest edge; the oracle
// (oracle/mesh_oracle.py) keeps Ericson's branchy form, an independent formulation.
// Degenerate triangles (sin^2 of the angle at vertex a <= 1e-12) use the nearest edge.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>

#include "pntf.h"
#include "pntf_mesh_geom.h"

namespace pntf_mesh {

thread_local char g_err[512] = "";   // the text behind pntf_mesh_last_error

int fail(const char* what) {
  snprintf(g_err, sizeof g_err, "%s", what);
  return PNTF_ERR_ARG;
}

int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    snprintf(g_err, sizeof g_err, "%s: %s", what, hipGetErrorString(e));
    return PNTF_ERR_HIP;
  }
  return PNTF_OK;
}

}  // namespace pntf_mesh

namespace {

using namespace pntf_mesh;  // record, tri_d2, reductions, BLOCK / PTS / PPW (pntf_mesh_geom.h)

constexpr int TARGET_WG = 2048;  // 8 workgroups per CU on 256 CUs

// grid (ceil(n/PPW), n_chunks); chunk y covers triangles [y*per, min(t,(y+1)*per)).  Each
// lane owns PTS points (PPW = 256·PTS per workgroup), so one LDS record read serves PTS tests.
// SPLIT: combine through atomicMin on d^2 bits in `acc`; else write sqrt(d^2) to `dist`.
template <bool SPLIT>
__global__ __launch_bounds__(BLOCK) void mesh_distance_kernel(
    const float* __restrict__ pts, int64_t n, const float* __restrict__ tris, int64_t t,
    int64_t per, float* __restrict__ dist, unsigned int* __restrict__ acc) {
  __shared__ float4 s_rec[BLOCK * REC];
  float px[PTS], py[PTS], pz[PTS], best[PTS];
#pragma unroll
  for (int k = 0; k < PTS; ++k) {
    const int64_t i = (int64_t)blockIdx.x * PPW + k * BLOCK + threadIdx.x;
    px[k] = py[k] = pz[k] = 0.f;
    if (i < n) {
      px[k] = pts[3 * i]; py[k] = pts[3 * i + 1]; pz[k] = pts[3 * i + 2];
    }
    best[k] = INFINITY;
  }
  // Tile culling: the workgroup's point box [lo, hi] and the largest current best d^2 of its
  // points give a lower bound test per triangle — a triangle whose AABB is farther than
  // that from the point box cannot lower any point's minimum, so skipping it changes no
  // result bit.  It pays when a workgroup's points are compact (ops.point_mesh_distance
  // feeds them in Morton order).  The test is workgroup-uniform: no divergence.
  __shared__ float s_red[4][8];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float lo[3], hi[3];
  {
    float a[3] = {INFINITY, INFINITY, INFINITY}, b[3] = {-INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int k = 0; k < PTS; ++k) {
      const int64_t i = (int64_t)blockIdx.x * PPW + k * BLOCK + threadIdx.x;
      if (i < n) {
        a[0] = fminf(a[0], px[k]); a[1] = fminf(a[1], py[k]); a[2] = fminf(a[2], pz[k]);
        b[0] = fmaxf(b[0], px[k]); b[1] = fmaxf(b[1], py[k]); b[2] = fmaxf(b[2], pz[k]);
      }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      a[d] = wave_min(a[d]);
      b[d] = wave_max(b[d]);
    }
    if (lane == 0) {
#pragma unroll
      for (int d = 0; d < 3; ++d) { s_red[wave][d] = a[d]; s_red[wave][3 + d] = b[d]; }
    }
    __syncthreads();
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      lo[d] = fminf(fminf(s_red[0][d], s_red[1][d]), fminf(s_red[2][d], s_red[3][d]));
      hi[d] = fmaxf(fmaxf(s_red[0][3 + d], s_red[1][3 + d]),
                    fmaxf(s_red[2][3 + d], s_red[3][3 + d]));
    }
  }
  float pext = 0.f;  // largest |coordinate| of the workgroup's point box
  for (int d = 0; d < 3; ++d) pext = fmaxf(pext, fmaxf(fabsf(lo[d]), fabsf(hi[d])));
  const int64_t t0 = (int64_t)blockIdx.y * per;
  const int64_t t1 = t0 + per < t ? t0 + per : t;
  for (int64_t base = t0; base < t1; base += BLOCK) {
    const int cnt = (int)(t1 - base < BLOCK ? t1 - base : BLOCK);
    float mb = -INFINITY;  // dead lanes keep best = inf but are excluded
#pragma unroll
    for (int k = 0; k < PTS; ++k)
      if ((int64_t)blockIdx.x * PPW + k * BLOCK + threadIdx.x < n) mb = fmaxf(mb, best[k]);
    mb = wave_max(mb);
    __syncthreads();
    if (threadIdx.x < cnt) build_record(tris + (base + threadIdx.x) * 9, s_rec + REC * threadIdx.x);
    if (lane == 0) s_red[wave][6] = mb;
    __syncthreads();
    const float bound = fmaxf(fmaxf(s_red[0][6], s_red[1][6]), fmaxf(s_red[2][6], s_red[3][6]));
    for (int j = 0; j < cnt; ++j) {
      const float4 bmin = s_rec[REC * j + 8], bmax = s_rec[REC * j + 9];
      if (tri_culled(bmin, bmax, lo, hi, pext, bound)) continue;  // exact (pntf_mesh_geom.h)
#pragma unroll
      for (int k = 0; k < PTS; ++k)
        best[k] = fminf(best[k], tri_d2(px[k], py[k], pz[k], s_rec + REC * j));
    }
  }
#pragma unroll
  for (int k = 0; k < PTS; ++k) {
    const int64_t i = (int64_t)blockIdx.x * PPW + k * BLOCK + threadIdx.x;
    if (i >= n) continue;
    if (SPLIT)
      atomicMin(acc + i, __float_as_uint(best[k]));
    else
      dist[i] = sqrtf(best[k]);
  }
}

}  // namespace

extern "C" {

const char* pntf_mesh_last_error(void) { return pntf_mesh::g_err; }

int pntf_mesh_chunks(int64_t n, int64_t t) {
  if (n <= 0 || t <= 0) return 1;
  const int64_t gx = (n + PPW - 1) / PPW;
  const int64_t tiles = (t + BLOCK - 1) / BLOCK;
  int64_t c = (TARGET_WG + gx - 1) / gx;
  if (c > tiles) c = tiles;
  if (c > 65535) c = 65535;
  return (int)(c < 1 ? 1 : c);
}

int pntf_point_mesh_distance(const float* pts, int64_t n, const float* tris, int64_t t,
                             float* dist, int chunks, hipStream_t stream) {
  if (n < 0 || t < 0 || (n > 0 && (!pts || !dist)) || (t > 0 && !tris))
    return fail("pntf_point_mesh_distance: bad arguments");
  if (n == 0) return PNTF_OK;
  if (t == 0) return fail("pntf_point_mesh_distance: empty mesh");
  if ((n + PPW - 1) / PPW > 0x7fffffff)
    return fail("pntf_point_mesh_distance: too many points");
  if (chunks <= 0) chunks = pntf_mesh_chunks(n, t);
  if (chunks > 65535) return fail("pntf_point_mesh_distance: chunks > 65535");
  // whole LDS tiles per chunk, so only the last chunk has a ragged tile
  int64_t per = (t + chunks - 1) / chunks;
  per = (per + BLOCK - 1) / BLOCK * BLOCK;
  const int64_t c = (t + per - 1) / per;
  const dim3 grid((unsigned)((n + PPW - 1) / PPW), (unsigned)c);
  if (c == 1) {
    hipLaunchKernelGGL(mesh_distance_kernel<false>, grid, dim3(BLOCK), 0, stream, pts, n, tris,
                       t, per, dist, nullptr);
    return check_launch("mesh_distance_kernel");
  }
  unsigned int* acc = reinterpret_cast<unsigned int*>(dist);
  const unsigned g1 = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL((fill_kernel<unsigned int, D2_INF>), dim3(g1), dim3(256), 0, stream, acc,
                     n);
  hipLaunchKernelGGL(mesh_distance_kernel<true>, grid, dim3(BLOCK), 0, stream, pts, n, tris, t,
                     per, dist, acc);
  hipLaunchKernelGGL(finalize_kernel, dim3(g1), dim3(256), 0, stream, dist, n, INFINITY);
  return check_launch("mesh_distance_kernel");
}

}  // extern "C"
