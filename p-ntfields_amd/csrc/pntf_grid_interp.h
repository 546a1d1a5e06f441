// Trilinear interpolation on the grid solver's node grid (include/pntf.h, "Grid paths"): the
// cell of a point, the value and the exact gradient of the cell's trilinear polynomial, and the
// blocked test, shared by pntf_grid_descent and pntf_grid_polyline_time (pntf_gridpath.hip).
//
// Every sum here has one written-down order, the pairwise tree over the corner index
// l = 4 di + 2 dj + dk:  ((t0 + t1) + (t2 + t3)) + ((t4 + t5) + (t6 + t7)),
// which is also what three xor-shuffle stages (1, 2, 4) over 8 lanes holding one corner each
// compute, and no operation is contracted into an FMA, so the one-lane and the 8-lane form give
// the same bits and tests/gridpath_oracle.py can restate them operation by operation.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace pntf_grid {

// NaN lands in range too: fmaxf / fminf return the operand that is a number
__device__ __forceinline__ float clamp_box(float x) { return fminf(fmaxf(x, -0.5f), 0.5f); }

// one axis: cell index i in [0, n - 2] and weight w = u - i in [0, 1]
__device__ __forceinline__ void axis_cell(float x, int32_t n, int& i, float& w) {
#pragma clang fp contract(off)
  const float u = (clamp_box(x) + 0.5f) * (float)(n - 1);
  i = min(max((int)u, 0), n - 2);        // the max is a no-op for u in [0, n - 1]: belt and braces
  w = u - (float)i;
}

struct Cell {
  int i, j, k;
  float wx, wy, wz;
};

__device__ __forceinline__ Cell cell_of(float x, float y, float z, int32_t n) {
  Cell c;
  axis_cell(x, n, c.i, c.wx);
  axis_cell(y, n, c.j, c.wy);
  axis_cell(z, n, c.k, c.wz);
  return c;
}

// flat node index of the cell's corner (di, dj, dk), k fastest; < n^3 because i, j, k <= n - 2
__device__ __forceinline__ int64_t corner_node(const Cell& c, int32_t n, int di, int dj, int dk) {
  return ((int64_t)(c.i + di) * n + (c.j + dj)) * n + (c.k + dk);
}

__device__ __forceinline__ bool finite(float a) { return fabsf(a) < INFINITY; }   // false for NaN

// One lane, all 8 corners: V(x) of the array A (n, n, n) in the cell c.  blocked = a corner is
// non-finite or, with `positive`, <= 0; the value is then meaningless.
__device__ __forceinline__ float cell_value(const float* __restrict__ A, int32_t n, const Cell& c,
                                            bool positive, bool& blocked) {
#pragma clang fp contract(off)
  float t[8];
  bool bad = false;
#pragma unroll
  for (int l = 0; l < 8; ++l) {
    const int di = l >> 2, dj = (l >> 1) & 1, dk = l & 1;
    const float a = A[corner_node(c, n, di, dj, dk)];
    bad = bad || !finite(a) || (positive && !(a > 0.f));
    const float wa = di ? c.wx : 1.f - c.wx, wb = dj ? c.wy : 1.f - c.wy,
                wc = dk ? c.wz : 1.f - c.wz;
    t[l] = a * ((wa * wb) * wc);
  }
  blocked = bad;
  return ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]));
}

// Eight lanes, one corner each (lane & 7 = 4 di + 2 dj + dk): V, grad V and blocked at (x, y, z),
// the same on all eight lanes.  Every lane of the wave must call it (the shuffles need their
// partners); a lane with `active` false loads nothing and contributes a finite 0.
struct Sample {
  float V, gx, gy, gz;
  bool blocked;
};

__device__ __forceinline__ Sample cell_sample8(const float* __restrict__ A, int32_t n, float x,
                                               float y, float z, int corner, bool active) {
#pragma clang fp contract(off)
  const Cell c = cell_of(x, y, z, n);
  const int di = corner >> 2, dj = (corner >> 1) & 1, dk = corner & 1;
  float a = 0.f;
  if (active) a = A[corner_node(c, n, di, dj, dk)];
  const float wa = di ? c.wx : 1.f - c.wx, wb = dj ? c.wy : 1.f - c.wy,
              wc = dk ? c.wz : 1.f - c.wz;
  const float px = a * (wb * wc), py = a * (wa * wc), pz = a * (wa * wb);
  float V = a * ((wa * wb) * wc);
  float gx = di ? px : -px, gy = dj ? py : -py, gz = dk ? pz : -pz;
  int bad = !finite(a);
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) {
    V = V + __shfl_xor(V, o);
    gx = gx + __shfl_xor(gx, o);
    gy = gy + __shfl_xor(gy, o);
    gz = gz + __shfl_xor(gz, o);
    bad |= __shfl_xor(bad, o);
  }
  const float s = (float)(n - 1);
  return Sample{V, gx * s, gy * s, gz * s, bad != 0};
}

}  // namespace pntf_grid
