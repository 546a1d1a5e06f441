// Grid paths on MI355X: the minimum-time path out of a solved grid travel time T (descent of
// T from a goal back to its source) and the travel time of polylines under the speed grid.
// Together they give a planned path its optimal baseline (pntf/evaluate.py path_optimality).
// The reference has neither (its scripts show paths in a viewer); both are specified in
// include/pntf.h ("Grid paths") and restated in numpy by tests/gridpath_oracle.py.
//
// MI355X design.  Descent is a dependent chain: each step's 8 loads of T wait for the point the
// previous step produced, a few hundred steps per query, so it is bound by load latency, not
// bandwidth (a query's n^3 floats of T, 1.1 MB at n = 65, stay in L2).  Eight lanes serve one
// query, one per corner of the current cell: each loads its corner and forms its term of
// (V, dV/dx, dV/dy, dV/dz), three xor-shuffle stages sum them in a fixed order and leave the
// result on all eight lanes, which then take the same step.  A workgroup is one wave = 8
// queries, so that 1024 queries spread over 128 CUs.  The loop is wave-uniform (it runs while
// any of the wave's queries is live); a finished query's lanes stop loading and storing but keep
// taking part in the shuffles, so no shuffle ever reads an inactive lane.  Every iteration
// either finishes its query or appends a point, and a point is appended only below row L: the
// loop ends after at most L iterations whatever T holds.
//
// Polyline time is a sum: one 256-lane workgroup per polyline, lane j owns segments j, j + 256,
// ... and adds their pieces in order; the 256 partial sums are added by a pairwise tree (xor
// shuffles 1..32 inside a wave, then the four waves through LDS), so a polyline's bits depend
// neither on its padding L nor on the other rows.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "pntf.h"
#include "pntf_grid_interp.h"
#include "pntf_mesh_geom.h"

namespace {

using pntf_grid::Cell;
using pntf_grid::Sample;
using pntf_grid::clamp_box;
using pntf_mesh::check_launch;
using pntf_mesh::fail;

constexpr int GROUP = 8;                 // lanes per query: the corners of a cell
constexpr int DESCENT_LANES = 64;        // one wave per workgroup = 8 queries
constexpr int TIME_LANES = 256;
constexpr float MAX_PIECES = 65536.f;    // pieces per segment (include/pntf.h)

__global__ __launch_bounds__(DESCENT_LANES) void grid_descent_kernel(
    const float* __restrict__ T, int32_t n, int64_t q, const float* __restrict__ src,
    const float* __restrict__ goal, float radius, float step, int32_t L,
    float* __restrict__ pts, int32_t* __restrict__ cnt, int32_t* __restrict__ status,
    float* __restrict__ tgoal) {
#pragma clang fp contract(off)
  const int corner = threadIdx.x & (GROUP - 1);
  const int64_t c = (int64_t)blockIdx.x * (DESCENT_LANES / GROUP) + threadIdx.x / GROUP;
  const bool live = c < q;
  const bool writer = live && corner == 0;
  const float* __restrict__ Tc = T + (int64_t)n * n * n * (live ? c : 0);
  float* __restrict__ P = pts + (live ? c : 0) * (int64_t)L * 3;
  const float h = 1.f / (float)(n - 1);
  float x = 0.f, y = 0.f, z = 0.f, sx = 0.f, sy = 0.f, sz = 0.f;
  if (live) {
    x = clamp_box(goal[3 * c]), y = clamp_box(goal[3 * c + 1]), z = clamp_box(goal[3 * c + 2]);
    sx = clamp_box(src[3 * c]), sy = clamp_box(src[3 * c + 1]), sz = clamp_box(src[3 * c + 2]);
  }
  if (writer) P[0] = x, P[1] = y, P[2] = z;
  bool done = !live;
  int count = 1, st = PNTF_DESCENT_ARRIVED;
  Sample cur = pntf_grid::cell_sample8(Tc, n, x, y, z, corner, !done);
  if (writer) tgoal[c] = cur.blocked ? INFINITY : cur.V;
  if (live && cur.blocked) st = PNTF_DESCENT_UNREACHABLE, done = true;
  const float rs = fmaxf(radius, 2.f) * h, rs2 = rs * rs, s = step * h;

  while (__any(!done)) {
    float nx = x, ny = y, nz = z;
    bool stepping = false;
    if (!done) {
      const float dx = x - sx, dy = y - sy, dz = z - sz;
      if ((dx * dx + dy * dy) + dz * dz <= rs2) {
        // inside the init ball the solver's field is the straight line: close with x_s
        if (__float_as_uint(x) != __float_as_uint(sx) || __float_as_uint(y) != __float_as_uint(sy) ||
            __float_as_uint(z) != __float_as_uint(sz)) {
          if (count == L) {
            st = PNTF_DESCENT_TRUNCATED;
          } else {
            if (writer) P[3 * count] = sx, P[3 * count + 1] = sy, P[3 * count + 2] = sz;
            ++count;
          }
        }
        done = true;
      } else {
        const float gn = sqrtf((cur.gx * cur.gx + cur.gy * cur.gy) + cur.gz * cur.gz);
        if (!(gn > 0.f) || !(gn < INFINITY)) {          // zero, NaN or overflowed
          st = PNTF_DESCENT_STALLED, done = true;
        } else {
          nx = clamp_box(x - s * (cur.gx / gn));
          ny = clamp_box(y - s * (cur.gy / gn));
          nz = clamp_box(z - s * (cur.gz / gn));
          stepping = true;
        }
      }
    }
    const Sample nxt = pntf_grid::cell_sample8(Tc, n, nx, ny, nz, corner, stepping);
    if (stepping) {
      if (nxt.blocked) {
        st = PNTF_DESCENT_BLOCKED, done = true;
      } else if (!(nxt.V < cur.V)) {
        st = PNTF_DESCENT_STALLED, done = true;
      } else if (count == L) {
        st = PNTF_DESCENT_TRUNCATED, done = true;
      } else {
        if (writer) P[3 * count] = nx, P[3 * count + 1] = ny, P[3 * count + 2] = nz;
        ++count;
        x = nx, y = ny, z = nz;
        cur = nxt;
      }
    }
  }
  if (live) {
    for (int r = count + corner; r < L; r += GROUP)
      P[3 * (int64_t)r] = 0.f, P[3 * (int64_t)r + 1] = 0.f, P[3 * (int64_t)r + 2] = 0.f;
    if (writer) cnt[c] = count, status[c] = st;
  }
}

__global__ __launch_bounds__(TIME_LANES) void grid_polyline_time_kernel(
    const float* __restrict__ speed, int32_t n, const float* __restrict__ pts, int32_t L,
    const int32_t* __restrict__ cnt, float sub, float* __restrict__ time) {
#pragma clang fp contract(off)
  __shared__ float s_red[TIME_LANES / 64];
  const int64_t c = blockIdx.x;
  const int nseg = min(max(cnt[c], 0), L) - 1;
  const float* __restrict__ P = pts + c * (int64_t)L * 3;
  const float piece = sub * (1.f / (float)(n - 1));
  float acc = 0.f;
  for (int i = threadIdx.x; i < nseg; i += TIME_LANES) {
    const float ax = P[3 * (int64_t)i], ay = P[3 * (int64_t)i + 1], az = P[3 * (int64_t)i + 2];
    const float dx = P[3 * (int64_t)i + 3] - ax, dy = P[3 * (int64_t)i + 4] - ay,
                dz = P[3 * (int64_t)i + 5] - az;
    const float len = sqrtf((dx * dx + dy * dy) + dz * dz);
    if (!(len < INFINITY)) {               // non-finite points: no lookup, the length itself
      acc = acc + len;
      continue;
    }
    if (len == 0.f) continue;              // a repeated point adds exactly 0
    const float mf = fminf(fmaxf(ceilf(len / piece), 1.f), MAX_PIECES);
    const int m = (int)mf;
    const float dl = len / mf;
    for (int p = 0; p < m; ++p) {
      const float t = ((float)p + 0.5f) / mf;
      const Cell cell = pntf_grid::cell_of(ax + t * dx, ay + t * dy, az + t * dz, n);
      bool blocked;
      const float V = pntf_grid::cell_value(speed, n, cell, true, blocked);
      acc = acc + (blocked ? INFINITY : dl / V);
    }
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) acc = acc + __shfl_xor(acc, o);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) time[c] = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

}  // namespace

extern "C" {

int pntf_grid_descent(const float* T, int32_t n, int64_t q, const float* src, const float* goal,
                      float radius, float step, int32_t L, float* pts, int32_t* cnt,
                      int32_t* status, float* tgoal, hipStream_t stream) {
  if (n < 2) return fail("pntf_grid_descent: n must be >= 2");
  if (q < 1) return fail("pntf_grid_descent: q must be >= 1");
  if (!(radius >= 0.f)) return fail("pntf_grid_descent: radius must be >= 0");
  if (!(step > 0.f && step <= 1.f)) return fail("pntf_grid_descent: step must be in (0, 1]");
  if (L < 2) return fail("pntf_grid_descent: L must be >= 2");
  if (!T || !src || !goal || !pts || !cnt || !status || !tgoal)
    return fail("pntf_grid_descent: bad arguments (null pointer)");
  const int64_t per = DESCENT_LANES / GROUP;
  if (n > 1624 || (q + per - 1) / per > 0x7fffffffLL)
    return fail("pntf_grid_descent: grid beyond the launch limits (n <= 1624 as the solver, "
                "q <= 8 (2^31 - 1))");
  hipLaunchKernelGGL(grid_descent_kernel, dim3((unsigned)((q + per - 1) / per)),
                     dim3(DESCENT_LANES), 0, stream, T, n, q, src, goal, radius, step, L, pts,
                     cnt, status, tgoal);
  return check_launch("grid_descent_kernel");
}

int pntf_grid_polyline_time(const float* speed, int32_t n, const float* pts, int64_t q,
                            int32_t L, const int32_t* cnt, float sub, float* time,
                            hipStream_t stream) {
  if (n < 2) return fail("pntf_grid_polyline_time: n must be >= 2");
  if (q < 1) return fail("pntf_grid_polyline_time: q must be >= 1");
  if (L < 1) return fail("pntf_grid_polyline_time: L must be >= 1");
  if (!(sub > 0.f && sub < INFINITY)) return fail("pntf_grid_polyline_time: sub must be > 0");
  if (!speed || !pts || !cnt || !time)
    return fail("pntf_grid_polyline_time: bad arguments (null pointer)");
  if (n > 1624 || q > 0x7fffffffLL)
    return fail("pntf_grid_polyline_time: grid beyond the launch limits (n <= 1624 as the "
                "solver, q < 2^31)");
  hipLaunchKernelGGL(grid_polyline_time_kernel, dim3((unsigned)q), dim3(TIME_LANES), 0, stream,
                     speed, n, pts, L, cnt, sub, time);
  return check_launch("grid_polyline_time_kernel");
}

}  // extern "C"
