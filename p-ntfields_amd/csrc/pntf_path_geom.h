// Segment -> triangle geometry of the polyline kernel (pntf_path.hip), on top of the point ->
// triangle record and tri_d2 of pntf_mesh_geom.h (untouched: an endpoint's contribution has
// the bits the point kernel gives it).
//
// The squared distance of a (segment, triangle) pair is the minimum of
//   * the two endpoint -> triangle distances (tri_d2, computed by the caller so that
//     consecutive segments share them),
//   * the three segment -> edge distances (seg_seg_d2), and
//   * exactly 0 when the segment pierces the triangle (pierces).
// Either the segment meets the triangle (pierce, or a coplanar crossing, which crosses an
// edge), or the closest pair of points has an endpoint of the segment or lies on an edge of the
// triangle: the three terms are exhaustive.  Everything is written with selects: every lane of
// a wave runs the same instructions whatever case its pair is in.
#ifndef PNTF_PATH_GEOM_H_
#define PNTF_PATH_GEOM_H_

#include "pntf_mesh_geom.h"

namespace pntf_mesh {

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// Squared distance between the segments P + [0,1]·d and A + [0,1]·e, r = P - A, idd = 1/|d|^2
// and ie = 1/|e|^2 (0 for a zero-length one).  Clamped closest points of two segments (Ericson,
// "Real-Time Collision Detection" §5.1.9) without its case split: s of the two infinite lines,
// clamped; t = the edge's closest parameter to that point, clamped; s again = the segment's
// closest parameter to that point, clamped (a no-op unless t was clamped, up to rounding).
// Any (s, t) in the unit square is a pair of points of the two segments, so rounding can only
// make the result too large, never too small.  The line-line s is taken from the cross product
// n = d x e, s = ((n x e)·r) / |n|^2, not from |d|^2|e|^2 - (d·e)^2: the difference of
// products loses all digits for nearly parallel segments, the cross product keeps a relative
// error of ~1e-7 / sin(angle), which moves the point by ~1e-7 of the segment's length.  For
// parallel segments (n = 0, also a zero-length edge) s starts at 0 and the two projections
// alone are exact: the closest pair of two parallel segments has an endpoint of one of them.
// Only a closest point strictly inside the segment (0 < s < 1) counts; otherwise +inf: at s = 0
// or 1 the pair is (endpoint, edge), which the endpoint's tri_d2 already covers with the point
// kernel's bits.  So two segments that are nearest at their shared point tie bit for bit (the
// lower index wins), a polyline is never farther than its vertices by a rounding, and a
// zero-length segment (idd = 0, hence s = 0) is exactly its point.
__device__ __forceinline__ float seg_seg_d2(float rx, float ry, float rz, float dx, float dy,
                                            float dz, float idd, float4 e, float ie) {
  const float nx = dy * e.z - dz * e.y, ny = dz * e.x - dx * e.z, nz = dx * e.y - dy * e.x;
  const float nn = dot3(nx, ny, nz, nx, ny, nz);
  const float kx = ny * e.z - nz * e.y, ky = nz * e.x - nx * e.z, kz = nx * e.y - ny * e.x;
  float s = nn > 0.f ? clamp01(dot3(kx, ky, kz, rx, ry, rz) * __builtin_amdgcn_rcpf(nn)) : 0.f;
  float ux = fmaf(s, dx, rx), uy = fmaf(s, dy, ry), uz = fmaf(s, dz, rz);      // P(s) - A
  const float t = clamp01(dot3(ux, uy, uz, e.x, e.y, e.z) * ie);
  ux = fmaf(t, e.x, -rx); uy = fmaf(t, e.y, -ry); uz = fmaf(t, e.z, -rz);      // A(t) - P
  s = clamp01(dot3(ux, uy, uz, dx, dy, dz) * idd);
  ux = fmaf(-s, dx, ux); uy = fmaf(-s, dy, uy); uz = fmaf(-s, dz, uz);         // A(t) - P(s)
  return s > 0.f && s < 1.f ? dot3(ux, uy, uz, ux, uy, uz) : INFINITY;
}

// Does the segment p0 -> p1 pierce the triangle?  Plane offsets of the endpoints of opposite
// sign or zero but not both zero (a coplanar segment is left to the edge distances), triangle
// not flat, and the crossing point p0 + h0/(h0 - h1)·(p1 - p0) inside by the record's three
// in-plane edge normals — tested on (h0·w1 - h1·w0)·sign(h0 - h1), w = the endpoint's offset
// along an edge normal, so no division is needed.
__device__ __forceinline__ bool pierces(float p0x, float p0y, float p0z, float p1x, float p1y,
                                        float p1z, const float4* __restrict__ r) {
  const float4 a = r[0], ab = r[1], bc = r[3], n = r[4], m0 = r[5], m1 = r[6], m2 = r[7];
  const float q0x = p0x - a.x, q0y = p0y - a.y, q0z = p0z - a.z;
  const float q1x = p1x - a.x, q1y = p1y - a.y, q1z = p1z - a.z;
  const float h0 = dot3(q0x, q0y, q0z, n.x, n.y, n.z), h1 = dot3(q1x, q1y, q1z, n.x, n.y, n.z);
  const float sg = h0 - h1;
  const float c0 = h0 * dot3(q1x, q1y, q1z, m0.x, m0.y, m0.z) -
                   h1 * dot3(q0x, q0y, q0z, m0.x, m0.y, m0.z);
  const float c1 = h0 * dot3(q1x, q1y, q1z, m1.x, m1.y, m1.z) -
                   h1 * dot3(q0x, q0y, q0z, m1.x, m1.y, m1.z);
  const float c2 = h0 * dot3(q1x - ab.x, q1y - ab.y, q1z - ab.z, m2.x, m2.y, m2.z) -
                   h1 * dot3(q0x - ab.x, q0y - ab.y, q0z - ab.z, m2.x, m2.y, m2.z);
  const bool pos = sg > 0.f;
  return h0 * h1 <= 0.f && sg != 0.f && bc.w == 0.f && (pos ? c0 : -c0) >= 0.f &&
         (pos ? c1 : -c1) >= 0.f && (pos ? c2 : -c2) >= 0.f;
}

// |segment - triangle|^2 for the segment p0 -> p1 with d = p1 - p0 and idd = 1/|d|^2 (0 for a
// zero-length segment, whose distance is then its endpoint's, exactly tri_d2's bits);
// e0, e1 = tri_d2 of the two endpoints.
__device__ __forceinline__ float seg_tri_d2(float p0x, float p0y, float p0z, float p1x,
                                            float p1y, float p1z, float dx, float dy, float dz,
                                            float idd, float e0, float e1,
                                            const float4* __restrict__ r) {
  const float4 a = r[0], ab = r[1], ac = r[2], bc = r[3];
  const float qx = p0x - a.x, qy = p0y - a.y, qz = p0z - a.z;        // p0 - a
  const float bx = qx - ab.x, by = qy - ab.y, bz = qz - ab.z;        // p0 - b
  float g = fminf(seg_seg_d2(qx, qy, qz, dx, dy, dz, idd, ab, a.w),
                  seg_seg_d2(qx, qy, qz, dx, dy, dz, idd, ac, ab.w));
  g = fminf(g, seg_seg_d2(bx, by, bz, dx, dy, dz, idd, bc, ac.w));
  g = fminf(fminf(e0, e1), g);
  return pierces(p0x, p0y, p0z, p1x, p1y, p1z, r) ? 0.f : g;
}

}  // namespace pntf_mesh

#endif  // PNTF_PATH_GEOM_H_
