// Grid travel time on MI355X: the first-order upwind (Godunov) Eikonal scheme on the n^3 node
// grid of the unit box, iterated to its fixed point.  The reference has no such solver (its
// scripts print statistics of the model's own outputs); this one gives the field a model's
// TravelTimes is judged against (pntf/evaluate.py field_report).  The scheme is specified in
// include/pntf.h (pntf_grid_travel_time_pass) and restated in fp64 by tests/eikonal_oracle.py.
//
// MI355X design.  The iteration is Jacobi: every node takes the minimum of its value and one
// update from its six neighbours' previous values, so it only lowers values and its fixed point
// is the fast-marching solution.  One PASS = one launch: a workgroup of 512 lanes owns an 8x8x8
// tile of one source's grid (grid.x = tiles, grid.y = sources), loads the tile and a one-node
// halo of Tin into LDS (10^3 floats, 4 KB), runs `inner` Jacobi sweeps in LDS with the halo
// held fixed (two barriers per sweep: all reads, then all writes), and writes its own nodes to
// Tout.  Each lane keeps its node's value and f = h / S in registers.  Tin and Tout are
// distinct buffers, so a pass reads only the previous pass's values whatever the order the
// workgroups run in: the state after p passes is a pure function of the inputs.  A tile that
// lowered any of its nodes adds 1 to changed[source] (one atomicAdd per workgroup); the host
// reads it every few passes and stops once a whole interval changed nothing.  Holding the halo
// fixed for `inner` sweeps changes the path, not the limit: values never rise and a state that
// one pass leaves unchanged is a state that one sweep leaves unchanged.
// Lanes past a ragged tile's edge hold +inf, which is what a neighbour outside the grid
// counts as, and write nothing.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "pntf.h"
#include "pntf_mesh_geom.h"

namespace {

using pntf_mesh::check_launch;
using pntf_mesh::fail;

constexpr int TILE = 8;                      // nodes per tile edge
constexpr int HALO = TILE + 2;               // LDS edge: the tile and one node on either side
constexpr int TILE_LANES = TILE * TILE * TILE;
constexpr int LDS_NODES = HALO * HALO * HALO;

// the tile's origin from the flat tile index (k fastest, as the nodes)
__device__ __forceinline__ void tile_origin(int32_t n, int& i0, int& j0, int& k0) {
  const int tpa = (n + TILE - 1) / TILE;
  const int t = blockIdx.x;
  k0 = TILE * (t % tpa);
  j0 = TILE * ((t / tpa) % tpa);
  i0 = TILE * (t / (tpa * tpa));
}

// One update of a node (include/pntf.h): p, q, r the per-axis minima of its two neighbours,
// f = h / S.  +inf marks "no value"; a, b, c are only subtracted when finite.
__device__ __forceinline__ float node_update(float p, float q, float r, float f) {
  const float lo = fminf(p, q), hi = fmaxf(p, q);
  const float a = fminf(lo, r), c = fmaxf(hi, r);
  const float b = fmaxf(lo, fminf(hi, r));
  float t = a + f;                                   // a = +inf gives +inf
  if (b < INFINITY && t > b) {
    const float d = a - b;
    t = (a + b + sqrtf(fmaxf(2.f * f * f - d * d, 0.f))) * 0.5f;
    if (c < INFINITY && t > c) {
      const float s = a + b + c;
      t = (s + sqrtf(fmaxf(s * s - 3.f * (a * a + b * b + c * c - f * f), 0.f))) / 3.f;
    }
  }
  return t;
}

__global__ __launch_bounds__(TILE_LANES) void grid_travel_time_pass_kernel(
    const float* __restrict__ speed, int32_t n, const float* __restrict__ Tin,
    float* __restrict__ Tout, int32_t inner, int32_t* __restrict__ changed) {
  __shared__ float s_T[LDS_NODES];
  int i0, j0, k0;
  tile_origin(n, i0, j0, k0);
  const int64_t n3 = (int64_t)n * n * n;
  const float* __restrict__ src_in = Tin + n3 * blockIdx.y;

  for (int e = threadIdx.x; e < LDS_NODES; e += TILE_LANES) {
    const int i = i0 - 1 + e / (HALO * HALO), j = j0 - 1 + (e / HALO) % HALO,
              k = k0 - 1 + e % HALO;
    const bool in = i >= 0 && i < n && j >= 0 && j < n && k >= 0 && k < n;
    s_T[e] = in ? src_in[((int64_t)i * n + j) * n + k] : INFINITY;
  }
  const int li = threadIdx.x / (TILE * TILE), lj = (threadIdx.x / TILE) % TILE,
            lk = threadIdx.x % TILE;
  const int i = i0 + li, j = j0 + lj, k = k0 + lk;
  const bool valid = i < n && j < n && k < n;
  const int64_t node = ((int64_t)i * n + j) * n + k;
  const float h = 1.f / (float)(n - 1);
  const float S = valid ? speed[node] : 0.f;
  const bool open = S > 0.f;                        // a wall (or a NaN speed) never updates
  const float f = h / S;
  const int c = ((li + 1) * HALO + lj + 1) * HALO + lk + 1;
  __syncthreads();
  const float first = s_T[c];
  float cur = first;
  for (int s = 0; s < inner; ++s) {
    const float p = fminf(s_T[c - HALO * HALO], s_T[c + HALO * HALO]);
    const float q = fminf(s_T[c - HALO], s_T[c + HALO]);
    const float r = fminf(s_T[c - 1], s_T[c + 1]);
    if (open) cur = fminf(cur, node_update(p, q, r, f));
    __syncthreads();                                 // every lane has read the old values
    if (open) s_T[c] = cur;
    __syncthreads();
  }
  if (valid) Tout[n3 * blockIdx.y + node] = cur;
  const int any = __syncthreads_or(__float_as_uint(cur) != __float_as_uint(first));
  if (threadIdx.x == 0 && any) atomicAdd(changed + blockIdx.y, 1);
}

// Initial state (include/pntf.h).  The geometry is fp64, one rounding per operation and no
// contraction, so that which nodes fall inside the ball is decided by the same arithmetic as
// the fp64 restatement in tests/, not by the fp32 rounding of the node coordinates.
__global__ __launch_bounds__(TILE_LANES) void grid_travel_time_init_kernel(
    const float* __restrict__ speed, int32_t n, const float* __restrict__ src, float radius,
    float* __restrict__ T) {
#pragma clang fp contract(off)
  int i0, j0, k0;
  tile_origin(n, i0, j0, k0);
  const int i = i0 + threadIdx.x / (TILE * TILE), j = j0 + (threadIdx.x / TILE) % TILE,
            k = k0 + threadIdx.x % TILE;
  if (i >= n || j >= n || k >= n) return;
  const int idx[3] = {i, j, k};
  const double h = 1.0 / (double)(n - 1);
  const double rh = (double)radius * h;
  double d2 = 0.0;
  int64_t near = 0;
  bool is_near = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double xs = (double)src[3 * blockIdx.y + a];
    const double u = (xs + 0.5) * (double)(n - 1);
    const int m = (int)fmin(fmax(floor(u + 0.5), 0.0), (double)(n - 1));   // NaN -> 0
    near = near * n + m;
    is_near = is_near && m == idx[a];
    const double dx = (-0.5 + h * (double)idx[a]) - xs;
    d2 = d2 + dx * dx;
  }
  const int64_t node = ((int64_t)i * n + j) * n + k;
  const float Sn = speed[near];
  float t = INFINITY;
  if ((is_near || d2 <= rh * rh) && speed[node] > 0.f && Sn > 0.f)
    t = (float)sqrt(d2) / Sn;
  T[(int64_t)n * n * n * blockIdx.y + node] = t;
}

// tiles of the n^3 grid, or 0 when they exceed the launch limits (2^32 lanes per dimension)
int64_t launch_tiles(int32_t n) {
  const int64_t tpa = ((int64_t)n + TILE - 1) / TILE;
  const int64_t tiles = tpa * tpa * tpa;
  return tpa > 2048 || tiles * TILE_LANES > 0xffffffffLL ? 0 : tiles;
}

}  // namespace

extern "C" {

int pntf_grid_travel_time_init(const float* speed, int32_t n, const float* src, int64_t q,
                               float radius, float* T, hipStream_t stream) {
  if (n < 2) return fail("pntf_grid_travel_time_init: n must be >= 2");
  if (q < 1) return fail("pntf_grid_travel_time_init: q must be >= 1");
  if (!(radius >= 0.f)) return fail("pntf_grid_travel_time_init: radius must be >= 0");
  if (!speed || !src || !T)
    return fail("pntf_grid_travel_time_init: bad arguments (null pointer)");
  const int64_t tiles = launch_tiles(n);
  if (!tiles || q > 65535)
    return fail("pntf_grid_travel_time_init: grid beyond the launch limits "
                "(ceil(n/8)^3 * 512 < 2^32 lanes, q <= 65535)");
  hipLaunchKernelGGL(grid_travel_time_init_kernel, dim3((unsigned)tiles, (unsigned)q),
                     dim3(TILE_LANES), 0, stream, speed, n, src, radius, T);
  return check_launch("grid_travel_time_init_kernel");
}

int pntf_grid_travel_time_pass(const float* speed, int32_t n, int64_t q, const float* Tin,
                               float* Tout, int32_t inner, int32_t* changed,
                               hipStream_t stream) {
  if (n < 2) return fail("pntf_grid_travel_time_pass: n must be >= 2");
  if (q < 1) return fail("pntf_grid_travel_time_pass: q must be >= 1");
  if (inner < 1) return fail("pntf_grid_travel_time_pass: inner must be >= 1");
  if (!speed || !Tin || !Tout || !changed)
    return fail("pntf_grid_travel_time_pass: bad arguments (null pointer)");
  if (Tin == Tout)
    return fail("pntf_grid_travel_time_pass: Tin and Tout must be distinct buffers");
  const int64_t tiles = launch_tiles(n);
  if (!tiles || q > 65535)
    return fail("pntf_grid_travel_time_pass: grid beyond the launch limits "
                "(ceil(n/8)^3 * 512 < 2^32 lanes, q <= 65535)");
  hipLaunchKernelGGL(grid_travel_time_pass_kernel, dim3((unsigned)tiles, (unsigned)q),
                     dim3(TILE_LANES), 0, stream, speed, n, Tin, Tout, inner, changed);
  return check_launch("grid_travel_time_pass_kernel");
}

}  // extern "C"
