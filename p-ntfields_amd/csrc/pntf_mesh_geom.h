// Point -> triangle geometry shared by the mesh-distance kernels (pntf_mesh.hip: points given;
// pntf_arm.hip: points posed by forward kinematics in the kernel; pntf_path.hip: the points of
// polylines): the per-triangle LDS record, the branch-free squared distance, the culling test
// and the wave reductions.  One definition, so every kernel computes a (point, triangle) pair
// to the same bits.  Also the fill and finalize passes that bracket a launch which combines
// through an atomic min.
#ifndef PNTF_MESH_GEOM_H_
#define PNTF_MESH_GEOM_H_

#include <hip/hip_runtime.h>
#include <math.h>

namespace pntf_mesh {

// Host side of the geometry / grid units (defined in pntf_mesh.hip): both write the one
// thread-local text behind pntf_mesh_last_error.  fail returns PNTF_ERR_ARG; check_launch
// returns PNTF_ERR_HIP with "what: <HIP's text>" if a launch since the last call failed.
int fail(const char* what);
int check_launch(const char* what);

constexpr int BLOCK = 256;       // lanes per workgroup = triangles per LDS tile
constexpr int PTS = 4;           // points per lane, in registers
constexpr int PPW = BLOCK * PTS; // points per workgroup

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by,
                                      float bz) {
  return fmaf(ax, bx, fmaf(ay, by, az * bz));
}

// Per-triangle record staged in LDS (8 float4, built once per tile by one lane each):
//   [0] a, 1/|ab|^2   [1] ab, 1/|ac|^2   [2] ac, 1/|bc|^2   [3] bc, flat
//   [4] n^ (unit normal)   [5] m_ab = n^ x ab   [6] m_ac = ac x n^   [7] m_bc = n^ x bc
// m_* are in-plane edge normals pointing into the triangle, each with w = -INSIDE_TAU |m|;
// `flat` = 1 for a (near-)zero-area triangle (sin^2 of the angle at a <= 1e-12), whose
// distance is then its nearest edge.
//   [8] triangle AABB min   [9] triangle AABB max   (tile culling, see the kernels)
//
// Conditioning.  The cross product of a thin triangle (sine of the angle at a = s) cancels to
// |ab||ac|s, so in fp32 the direction of n^ is off by ~6e-8 / s and the plane distance q.n^ by
// |q| times that — 1e-5 at s = 1e-3, and almost always too small, which then wins tri_d2's
// min.  Where the fp32 cross product says sin^2 <= THIN_SIN2 (s <= 0.03; it still has five
// digits there), or gives nothing usable (zero, underflow), n^ and `flat` are taken again from
// the exact fp64 edge differences of the fp32 vertices and rounded to fp32 once: ~1e-16 / s,
// below the final rounding for every triangle that is not `flat`.  Above the threshold the
// fp32 normal keeps its bits; it is off by at most 6e-8 / 0.03 = 2e-6 of the query's in-plane
// distance from a (measured at s = 0.01 before the switch: 3e-7 at most).  About one triangle
// in 2000 of a random mesh is that thin at a, so few waves take the branch.
//
// The inside test of tri_d2 is q.m >= INSIDE_TAU |m| for the three edges, not >= 0: q = p - a
// carries an fp32 rounding of ~6e-8 |q|, and where two edges meet at an angle s a point of the
// plane up to that rounding / s BEYOND the tip passed all three tests at 0 and got the plane
// distance (~0) instead of its distance to the tip.  A point within INSIDE_TAU of an edge,
// seen from inside, now takes the edge distance, which is at most INSIDE_TAU farther than the
// plane distance.  INSIDE_TAU covers the roundings of q, m and the dot product (about
// 8 x 2^-24 |q||m|) for |q| <= 0.5.
constexpr int REC = 10;
constexpr float INSIDE_TAU = 2.5e-7f;
constexpr float THIN_SIN2 = 1e-3f;

__device__ __forceinline__ void build_record(const float* __restrict__ t, float4* __restrict__ r) {
  const float ax = t[0], ay = t[1], az = t[2];
  const float abx = t[3] - ax, aby = t[4] - ay, abz = t[5] - az;
  const float acx = t[6] - ax, acy = t[7] - ay, acz = t[8] - az;
  const float bcx = t[6] - t[3], bcy = t[7] - t[4], bcz = t[8] - t[5];
  const float ab2 = dot3(abx, aby, abz, abx, aby, abz);
  const float ac2 = dot3(acx, acy, acz, acx, acy, acz);
  const float bc2 = dot3(bcx, bcy, bcz, bcx, bcy, bcz);
  float nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;
  const float nn = dot3(nx, ny, nz, nx, ny, nz);
  bool flat = !(nn > 1e-12f * ab2 * ac2);
  const float inv = flat ? 0.f : 1.f / sqrtf(nn);
  nx *= inv; ny *= inv; nz *= inv;
  if (!(nn > THIN_SIN2 * ab2 * ac2)) {  // thin at a, flat, or too small for fp32: fp64 normal
    const double dabx = (double)t[3] - ax, daby = (double)t[4] - ay, dabz = (double)t[5] - az;
    const double dacx = (double)t[6] - ax, dacy = (double)t[7] - ay, dacz = (double)t[8] - az;
    const double dnx = daby * dacz - dabz * dacy, dny = dabz * dacx - dabx * dacz,
                 dnz = dabx * dacy - daby * dacx;
    const double dnn = fma(dnx, dnx, fma(dny, dny, dnz * dnz));
    flat = !(dnn > 1e-12 * fma(dabx, dabx, fma(daby, daby, dabz * dabz)) *
                       fma(dacx, dacx, fma(dacy, dacy, dacz * dacz)));
    const double dinv = flat ? 0.0 : 1.0 / sqrt(dnn);
    nx = (float)(dnx * dinv); ny = (float)(dny * dinv); nz = (float)(dnz * dinv);
  }
  const float wab = -INSIDE_TAU * __builtin_amdgcn_sqrtf(ab2),
              wac = -INSIDE_TAU * __builtin_amdgcn_sqrtf(ac2),
              wbc = -INSIDE_TAU * __builtin_amdgcn_sqrtf(bc2);
  r[0] = make_float4(ax, ay, az, ab2 > 0.f ? 1.f / ab2 : 0.f);
  r[1] = make_float4(abx, aby, abz, ac2 > 0.f ? 1.f / ac2 : 0.f);
  r[2] = make_float4(acx, acy, acz, bc2 > 0.f ? 1.f / bc2 : 0.f);
  r[3] = make_float4(bcx, bcy, bcz, flat ? 1.f : 0.f);
  r[4] = make_float4(nx, ny, nz, 0.f);
  r[5] = make_float4(ny * abz - nz * aby, nz * abx - nx * abz, nx * aby - ny * abx, wab);
  r[6] = make_float4(acy * nz - acz * ny, acz * nx - acx * nz, acx * ny - acy * nx, wac);
  r[7] = make_float4(ny * bcz - nz * bcy, nz * bcx - nx * bcz, nx * bcy - ny * bcx, wbc);
  r[8] = make_float4(fminf(ax, fminf(t[3], t[6])), fminf(ay, fminf(t[4], t[7])),
                     fminf(az, fminf(t[5], t[8])), 0.f);
  r[9] = make_float4(fmaxf(ax, fmaxf(t[3], t[6])), fmaxf(ay, fmaxf(t[4], t[7])),
                     fmaxf(az, fmaxf(t[5], t[8])), 0.f);
}

// workgroup-wide min / max of 256 lanes (4 waves): wave shuffles, then LDS
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
  return v;
}

// squared distance from q (= p - origin) to the segment origin + [0,1]·e, 1/|e|^2 = ie
__device__ __forceinline__ float seg_d2(float qx, float qy, float qz, float4 e, float ie) {
  const float tt = fminf(fmaxf(dot3(qx, qy, qz, e.x, e.y, e.z) * ie, 0.f), 1.f);
  const float rx = fmaf(-tt, e.x, qx), ry = fmaf(-tt, e.y, qy), rz = fmaf(-tt, e.z, qz);
  return dot3(rx, ry, rz, rx, ry, rz);
}

// q.m - INSIDE_TAU |m| for an in-plane edge normal of the record (the offset rides in m.w, so
// the test costs what q.m >= 0 did)
__device__ __forceinline__ float side(float qx, float qy, float qz, float4 m) {
  return fmaf(qx, m.x, fmaf(qy, m.y, fmaf(qz, m.z, m.w)));
}

// Branch-free |p - closest point of the triangle|^2: if p projects inside the triangle the
// distance is the plane distance, otherwise the nearest of the three edges (exactly the
// Voronoi regions of Ericson §5.1.5, evaluated without divergence: every lane of a wave
// runs the same instructions whatever region its point falls in).
__device__ __forceinline__ float tri_d2(float px, float py, float pz,
                                        const float4* __restrict__ r) {
  const float4 a = r[0], ab = r[1], ac = r[2], bc = r[3];
  const float qx = px - a.x, qy = py - a.y, qz = pz - a.z;           // p - a
  const float bx = qx - ab.x, by = qy - ab.y, bz = qz - ab.z;        // p - b
  float e = fminf(seg_d2(qx, qy, qz, ab, a.w), seg_d2(qx, qy, qz, ac, ab.w));
  e = fminf(e, seg_d2(bx, by, bz, bc, ac.w));
  const float4 n = r[4], m0 = r[5], m1 = r[6], m2 = r[7];
  const float h = dot3(qx, qy, qz, n.x, n.y, n.z);
  const bool inside = side(qx, qy, qz, m0) >= 0.f && side(qx, qy, qz, m1) >= 0.f &&
                      side(bx, by, bz, m2) >= 0.f && bc.w == 0.f;
  return inside ? fminf(h * h, e) : e;
}

// Exact tile culling, shared so every kernel skips by the same rule: a triangle whose AABB
// [bmin, bmax] is farther from the point box [lo, hi] than `bound` (a squared distance no
// point of the box needs to beat) cannot lower a minimum.  Cull only with slack: gap^2 and
// tri_d2 are both fp32-rounded, and a triangle whose true distance sits within a few ulp of
// the box gap (axis-aligned walls) could otherwise be culled although its computed d2 is
// below the bound.  The slack covers both roundings: relative to the bound, and absolute on
// the squared coordinate scale of the triangle and the point box (pext = its largest
// |coordinate|).
__device__ __forceinline__ bool tri_culled(float4 bmin, float4 bmax, const float* lo,
                                           const float* hi, float pext, float bound) {
  const float gx = fmaxf(fmaxf(bmin.x - hi[0], lo[0] - bmax.x), 0.f);
  const float gy = fmaxf(fmaxf(bmin.y - hi[1], lo[1] - bmax.y), 0.f);
  const float gz = fmaxf(fmaxf(bmin.z - hi[2], lo[2] - bmax.z), 0.f);
  const float ext = fmaxf(fmaxf(fmaxf(fabsf(bmin.x), fabsf(bmax.x)),
                                fmaxf(fmaxf(fabsf(bmin.y), fabsf(bmax.y)),
                                      fmaxf(fabsf(bmin.z), fabsf(bmax.z)))), pext);
  return dot3(gx, gy, gz, gx, gy, gz) > bound * (1.f + 1e-4f) + 1e-6f * ext * ext;
}

// acc[i] = VALUE for i < n: the start of an atomic-min reduction
template <class T, T VALUE>
static __global__ void fill_kernel(T* __restrict__ acc, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) acc[i] = VALUE;
}

constexpr unsigned int D2_INF = 0x7f800000u;   // fp32 bits of d^2 = +inf

// in place: fp32 bits of the minimum d^2 -> min(sqrt(d^2), cap); cap = INFINITY for none
static __global__ void finalize_kernel(float* __restrict__ dist, int64_t n, float cap) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n)
    dist[i] = fminf(sqrtf(__uint_as_float(reinterpret_cast<unsigned int*>(dist)[i])), cap);
}

}  // namespace pntf_mesh

#endif  // PNTF_MESH_GEOM_H_
