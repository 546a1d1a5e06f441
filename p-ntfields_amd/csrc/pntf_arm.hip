// Arm (serial chain) -> triangle-mesh unsigned distance on MI355X: the query of the arm
// speed-sample generator, `arm_obstacle_distance` (dataprocessing/speed_sampling_gpu.py:
// 153-218).  For each sampled joint vector the reference poses every collision-mesh vertex of
// every link with pytorch_kinematics (forward_kinematics(th, end_only=False)), materialises
// the n x V posed cloud, runs bvh_distance_queries over it and reduces with torch.min.
//
// MI355X design: the posing is fused in front of the dense culled point -> mesh kernel of
// pntf_mesh.hip and the per-configuration minimum behind it, so the cloud never exists in
// memory.  One workgroup owns one configuration (grid.x) and one chunk of at most 1024
// vertices of a single frame (grid.y), so its pose matrix is workgroup-uniform: it composes
// M_f = M_{f-1} · O_f · J_f(theta) from the root to its frame (the chain travels as a kernel
// argument: scalar loads, <= 16 small 3x4 products), poses its vertices in registers (four
// per lane) and runs the tile loop of pntf_mesh.hip on them — same LDS records, same
// branch-free tri_d2 (pntf_mesh_geom.h).  Because only the minimum over the workgroup's
// points is wanted, the culling bound is the workgroup's current MINIMUM d^2 (the point kernel
// must use the maximum), tightened by cap^2 and by a plain read of acc[c], which other chunks
// of the configuration have already lowered: none of the three is below the configuration's
// final minimum unless the result is capped anyway, so culling stays exact.  One link of one
// pose is a compact point set, so most tiles are culled to their AABB tests.  The result is
// combined by one atomicMin per workgroup on the fp32 bit pattern of d^2 (order-preserving
// for d^2 >= 0): the bits depend neither on the chunking nor on the rest of the batch.
// grid.x = configuration puts the chunks of one configuration far apart in launch order, so
// later chunks start from the minimum the earlier ones found.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>

#include "pntf.h"
#include "pntf_mesh_geom.h"

namespace {

using namespace pntf_mesh;

constexpr int MAXF = PNTF_ARM_MAX_FRAMES;

// The chain, passed by value (kernel argument segment: every read is a scalar load).
struct ArmChain {
  float origin[MAXF][12];  // O_f, 3x4 row-major
  float axis[MAXF][3];     // unit joint axis
  int type[MAXF];          // PNTF_JOINT_*
  int col[MAXF];           // column of theta the joint reads
  int voff[MAXF + 1];      // CSR offsets of the frames' vertices
  int coff[MAXF + 1];      // chunk table: frame f owns chunks [coff[f], coff[f+1])
  int dof;
};

// C (3x4) = A (3x4) · B (3x4), both with an implied last row (0 0 0 1)
__device__ __forceinline__ void mul34(const float* A, const float* B, float* C) {
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float s = fmaf(A[4 * r], B[c], fmaf(A[4 * r + 1], B[4 + c], A[4 * r + 2] * B[8 + c]));
      C[4 * r + c] = c == 3 ? s + A[4 * r + 3] : s;
    }
  }
}

__global__ __launch_bounds__(BLOCK) void arm_mesh_distance_kernel(
    const float* __restrict__ theta, const ArmChain ch, const float* __restrict__ verts,
    const float* __restrict__ tris, int64_t t, float cap2, unsigned int* __restrict__ acc) {
  __shared__ float4 s_rec[BLOCK * REC];
  __shared__ float s_red[4][8];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t c = blockIdx.x;
  const int chunk = blockIdx.y;
  int frame = 0;
  while (ch.coff[frame + 1] <= chunk) ++frame;  // coff[frames] = grid.y > chunk
  const int start = ch.voff[frame] + (chunk - ch.coff[frame]) * PPW;
  const int left = ch.voff[frame + 1] - start;
  const int cnt = left < PPW ? left : PPW;      // >= 1: empty frames own no chunk

  // forward kinematics to this frame (URDF convention), workgroup-uniform
  float M[12] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f};
  for (int g = 0; g <= frame; ++g) {
    float J[12] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f};
    const int type = ch.type[g];
    if (type != PNTF_JOINT_FIXED) {
      const float q = theta[c * ch.dof + ch.col[g]];
      const float ax = ch.axis[g][0], ay = ch.axis[g][1], az = ch.axis[g][2];
      if (type == PNTF_JOINT_REVOLUTE) {  // Rodrigues: cos·I + sin·[a]x + (1 - cos)·a aT
        const float sn = sinf(q), cs = cosf(q), v = 1.f - cs;
        J[0] = fmaf(v * ax, ax, cs);       J[1] = fmaf(v * ax, ay, -sn * az);
        J[2] = fmaf(v * ax, az, sn * ay);  J[4] = fmaf(v * ay, ax, sn * az);
        J[5] = fmaf(v * ay, ay, cs);       J[6] = fmaf(v * ay, az, -sn * ax);
        J[8] = fmaf(v * az, ax, -sn * ay); J[9] = fmaf(v * az, ay, sn * ax);
        J[10] = fmaf(v * az, az, cs);
      } else {                            // prismatic: slide along the axis
        J[3] = q * ax; J[7] = q * ay; J[11] = q * az;
      }
    }
    float O[12], T[12], N[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) O[k] = ch.origin[g][k];
    mul34(O, J, T);
    mul34(M, T, N);
#pragma unroll
    for (int k = 0; k < 12; ++k) M[k] = N[k];
  }

  // pose this workgroup's vertices; lanes past the chunk's end repeat its first vertex, so
  // they need no exclusion from the box or the minimum
  float px[PTS], py[PTS], pz[PTS], best[PTS];
#pragma unroll
  for (int k = 0; k < PTS; ++k) {
    const int j = k * BLOCK + threadIdx.x;
    const float* v = verts + 3 * (int64_t)(start + (j < cnt ? j : 0));
    const float vx = v[0], vy = v[1], vz = v[2];
    px[k] = fmaf(M[0], vx, fmaf(M[1], vy, fmaf(M[2], vz, M[3])));
    py[k] = fmaf(M[4], vx, fmaf(M[5], vy, fmaf(M[6], vz, M[7])));
    pz[k] = fmaf(M[8], vx, fmaf(M[9], vy, fmaf(M[10], vz, M[11])));
    best[k] = INFINITY;
  }
  float lo[3], hi[3];
  {
    float a[3] = {px[0], py[0], pz[0]}, b[3] = {px[0], py[0], pz[0]};
#pragma unroll
    for (int k = 1; k < PTS; ++k) {
      a[0] = fminf(a[0], px[k]); a[1] = fminf(a[1], py[k]); a[2] = fminf(a[2], pz[k]);
      b[0] = fmaxf(b[0], px[k]); b[1] = fmaxf(b[1], py[k]); b[2] = fmaxf(b[2], pz[k]);
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

  for (int64_t base = 0; base < t; base += BLOCK) {
    const int tcnt = (int)(t - base < BLOCK ? t - base : BLOCK);
    float mb = fminf(fminf(best[0], best[1]), fminf(best[2], best[3]));
    mb = wave_min(mb);
    __syncthreads();
    if (threadIdx.x < tcnt)
      build_record(tris + (base + threadIdx.x) * 9, s_rec + REC * threadIdx.x);
    if (lane == 0) s_red[wave][6] = mb;
    // what the configuration's other chunks have reached so far (any earlier value is valid)
    const float other = __uint_as_float(
        __hip_atomic_load(acc + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    __syncthreads();
    float bound = fminf(fminf(s_red[0][6], s_red[1][6]), fminf(s_red[2][6], s_red[3][6]));
    bound = fminf(bound, fminf(cap2, other));
    for (int j = 0; j < tcnt; ++j) {
      const float4 bmin = s_rec[REC * j + 8], bmax = s_rec[REC * j + 9];
      if (tri_culled(bmin, bmax, lo, hi, pext, bound)) continue;  // exact (pntf_mesh_geom.h)
#pragma unroll
      for (int k = 0; k < PTS; ++k)
        best[k] = fminf(best[k], tri_d2(px[k], py[k], pz[k], s_rec + REC * j));
    }
  }
  static_assert(PTS == 4, "the minimum above is written for four points per lane");
  float m = wave_min(fminf(fminf(best[0], best[1]), fminf(best[2], best[3])));
  __syncthreads();
  if (lane == 0) s_red[wave][7] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = fminf(fminf(s_red[0][7], s_red[1][7]), fminf(s_red[2][7], s_red[3][7]));
    atomicMin(acc + c, __float_as_uint(m));
  }
}

}  // namespace

extern "C" {

int pntf_arm_mesh_distance(const float* theta, int64_t n, int dof, int frames,
                           const float* origins, const int32_t* types, const float* axes,
                           const int32_t* cols, const float* verts, const int32_t* voff,
                           const float* tris, int64_t t, float cap, float* dist,
                           hipStream_t stream) {
  if (n < 0 || t < 0) return fail("pntf_arm_mesh_distance: bad arguments (negative size)");
  if (n == 0) return PNTF_OK;
  if (frames < 1 || frames > MAXF || dof < 0 || dof > PNTF_ARM_MAX_DOF)
    return fail("pntf_arm_mesh_distance: frames must be 1..16 and dof 0..16");
  if (!origins || !types || !axes || !cols || !voff || !dist || (dof > 0 && !theta))
    return fail("pntf_arm_mesh_distance: bad arguments (null pointer)");
  if (!(cap >= 0.f)) return fail("pntf_arm_mesh_distance: cap must be >= 0 (INFINITY = exact)");
  ArmChain ch = {};
  ch.dof = dof;
  int64_t chunks = 0;
  if (voff[0] != 0) return fail("pntf_arm_mesh_distance: voff[0] must be 0");
  for (int f = 0; f < frames; ++f) {
    if (types[f] != PNTF_JOINT_FIXED && types[f] != PNTF_JOINT_REVOLUTE &&
        types[f] != PNTF_JOINT_PRISMATIC)
      return fail("pntf_arm_mesh_distance: unknown joint type");
    if (types[f] != PNTF_JOINT_FIXED && (cols[f] < 0 || cols[f] >= dof))
      return fail("pntf_arm_mesh_distance: a frame reads a column >= dof");
    if (voff[f + 1] < voff[f]) return fail("pntf_arm_mesh_distance: voff must not decrease");
    for (int k = 0; k < 12; ++k) ch.origin[f][k] = origins[12 * f + k];
    for (int k = 0; k < 3; ++k) ch.axis[f][k] = axes[3 * f + k];
    ch.type[f] = types[f];
    ch.col[f] = cols[f];
    ch.voff[f] = voff[f];
    ch.coff[f] = (int)chunks;
    chunks += ((int64_t)voff[f + 1] - voff[f] + PPW - 1) / PPW;
    if (chunks > 65535) return fail("pntf_arm_mesh_distance: more than 65535 vertex chunks");
  }
  for (int f = frames; f <= MAXF; ++f) {
    ch.voff[f] = voff[frames];
    ch.coff[f] = (int)chunks;
  }
  if (voff[frames] > 0 && !verts)
    return fail("pntf_arm_mesh_distance: bad arguments (null pointer)");
  if (t == 0) return fail("pntf_arm_mesh_distance: empty mesh");
  if (!tris) return fail("pntf_arm_mesh_distance: bad arguments (null pointer)");
  if (n > 0x7fffffff) return fail("pntf_arm_mesh_distance: too many configurations");
  unsigned int* acc = reinterpret_cast<unsigned int*>(dist);
  const unsigned g1 = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL((fill_kernel<unsigned int, D2_INF>), dim3(g1), dim3(256), 0, stream, acc,
                     n);
  if (chunks > 0)
    hipLaunchKernelGGL(arm_mesh_distance_kernel, dim3((unsigned)n, (unsigned)chunks),
                       dim3(BLOCK), 0, stream, theta, ch, verts, tris, t, cap * cap, acc);
  hipLaunchKernelGGL(finalize_kernel, dim3(g1), dim3(256), 0, stream, dist, n, cap);
  return check_launch("arm_mesh_distance_kernel");
}

}  // extern "C"
