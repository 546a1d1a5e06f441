// TEST ONLY (tests/test_device_primitives.py): calls the __device__ primitives the fused kernels
// inline — pntf_field.h sp_sig, sig10, smooth_merge, head_sig, sincos_fast; pntf_wide.h wsp_sig,
// wx6_split, wx6_mma; pntf_taylor.h nx6_split, nx6_mma — one at a time from tiny kernels, with no
// network around them.  The headers are included exactly as csrc/pntf_kernels.hip includes them,
// and the test compiles this file with the flags and defines of the shipped wide unit, so these
// are the very functions the kernels use.  Nothing here is linked into libpntf.so.
//
// Every pointer is device memory.  A launcher waits for its kernel and returns the hipError_t.
#include <cstdint>

#include "pntf_quad.h"
#include "pntf_split.h"
#include "pntf_taylor.h"
#include "pntf_wide.h"

namespace {
using namespace pntf;

constexpr int EW_THREADS = 256, EW_BLOCKS = 4;   // a few workgroups, grid-stride over n

#define PROBE_EW_LOOP(i, n) \
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += gridDim.x * blockDim.x)

__global__ void sp_sig_kernel(const float* y, float* sp, float* sg, int n) {
  PROBE_EW_LOOP(i, n) {
    const SpSig o = sp_sig(y[i]);
    sp[i] = o.sp;
    sg[i] = o.sg;
  }
}
__global__ void sig10_kernel(const float* y, float* sg, int n) {
  PROBE_EW_LOOP(i, n) sg[i] = sig10(y[i]);
}
__global__ void wsp_sig_kernel(const float* y, float* sp, float* sg, int n) {
  PROBE_EW_LOOP(i, n) {
    const SpSig o = wsp_sig(y[i]);
    sp[i] = o.sp;
    sg[i] = o.sg;
  }
}
__global__ void merge_kernel(const float* zs, const float* zg, float* M, float* m, float* s0,
                             int n) {
  PROBE_EW_LOOP(i, n) {
    const Merge o = smooth_merge(zs[i], zg[i]);
    M[i] = o.M;
    m[i] = o.m;
    s0[i] = o.s0;
  }
}
__global__ void head_kernel(const float* y, float* tau, int n) {
  PROBE_EW_LOOP(i, n) tau[i] = head_sig(y[i]);
}
__global__ void sincos_kernel(const float* q, float* s, float* c, int n) {
  PROBE_EW_LOOP(i, n) {
    float sn, cs;
    sincos_fast(q[i], sn, cs);
    s[i] = sn;
    c[i] = cs;
  }
}

// One wave.  X (16 S x 32) and terms (3 x 16 S x 32) are row-major [feature][pair], C and out
// (32 x 32) row-major [out row][pair]; A0..A2 hold, per k block B and lane l, the 8 bf16 of the
// A operand of v_mfma_f32_32x32x16_bf16: element i = W[l & 31][16 B + 8 (l >> 5) + i in the
// MFMA's k order], i.e. the feature of register 8 b + i of lane half l >> 5 (wrow).
__global__ void wx6_kernel(const f32x4* A0, const f32x4* A1, const f32x4* A2, const float* X,
                           const float* C, float* terms, float* out, int S) {
  const int lane = threadIdx.x, j = lane & 31, h = lane >> 5, K = 16 * S;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = C[wrow(r, h) * 32 + j];
  for (int t = 0; 2 * t < S; ++t) {
    f32x16 v;   // input tile t in the layer layout: register r <-> feature row wrow(r, h)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int f = 32 * t + wrow(r, h);
      v[r] = f < K ? X[f * 32 + j] : 0.f;
    }
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int B = 2 * t + b;
      if (B < S) {
        wbf16x8 s[3];
        wx6_split(v, b, s);
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
          for (int i = 0; i < 8; ++i)
            terms[(p * K + 32 * t + wrow(8 * b + i, h)) * 32 + j] = static_cast<float>(s[p][i]);
        acc = wx6_mma(A0[B * 64 + lane], A1[B * 64 + lane], A2[B * 64 + lane], s, acc);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) out[wrow(r, h) * 32 + j] = acc[r];
}

// One wave, the 16-pair layout of pntf_taylor.h: lane (t, g) = (l & 15, l >> 4) holds rows
// 4 g .. 4 g + 3 of every 16-feature tile of pair t; k block B (32 features) is input tiles 2 B
// and 2 B + 1.  X (32 S x 16), terms (3 x 32 S x 16), C and out (16 x 16) as above; A0..A2 per
// block and lane the 8 bf16 of the A operand of v_mfma_f32_16x16x32_bf16: element i =
// W[l & 15][16 (2 B + (i >> 2)) + 4 (l >> 4) + (i & 3)].
__global__ void nx6_kernel(const f32x4* A0, const f32x4* A1, const f32x4* A2, const float* X,
                           const float* C, float* terms, float* out, int S) {
  const int lane = threadIdx.x, t = lane & 15, g = lane >> 4, K = 32 * S;
  f32x4 acc;
#pragma unroll
  for (int s = 0; s < 4; ++s) acc[s] = C[(4 * g + s) * 16 + t];
  for (int B = 0; B < S; ++B) {
    f32x4 lo, hi;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      lo[s] = X[(16 * (2 * B) + 4 * g + s) * 16 + t];
      hi[s] = X[(16 * (2 * B + 1) + 4 * g + s) * 16 + t];
    }
    nbf16x8 sp[3];
    nx6_split(lo, hi, sp);
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int i = 0; i < 8; ++i)
        terms[(p * K + 16 * (2 * B + (i >> 2)) + 4 * g + (i & 3)) * 16 + t] =
            static_cast<float>(sp[p][i]);
    acc = nx6_mma(A0[B * 64 + lane], A1[B * 64 + lane], A2[B * 64 + lane], sp, acc);
  }
#pragma unroll
  for (int s = 0; s < 4; ++s) out[(4 * g + s) * 16 + t] = acc[s];
}

int ew_blocks(int n) {
  const int b = (n + EW_THREADS - 1) / EW_THREADS;
  return b < 1 ? 1 : (b > EW_BLOCKS ? EW_BLOCKS : b);
}
int done() {
  const hipError_t e = hipDeviceSynchronize();
  const hipError_t l = hipGetLastError();
  return static_cast<int>(e != hipSuccess ? e : l);
}
constexpr int MAX_N = 1 << 16, MAX_S = 16;
}  // namespace

extern "C" {
int probe_sp_sig(const float* y, float* sp, float* sg, int n) {
  if (n < 0 || n > MAX_N) return -1;
  sp_sig_kernel<<<ew_blocks(n), EW_THREADS>>>(y, sp, sg, n);
  return done();
}
int probe_sig10(const float* y, float* sg, int n) {
  if (n < 0 || n > MAX_N) return -1;
  sig10_kernel<<<ew_blocks(n), EW_THREADS>>>(y, sg, n);
  return done();
}
int probe_wsp_sig(const float* y, float* sp, float* sg, int n) {
  if (n < 0 || n > MAX_N) return -1;
  wsp_sig_kernel<<<ew_blocks(n), EW_THREADS>>>(y, sp, sg, n);
  return done();
}
int probe_merge(const float* zs, const float* zg, float* M, float* m, float* s0, int n) {
  if (n < 0 || n > MAX_N) return -1;
  merge_kernel<<<ew_blocks(n), EW_THREADS>>>(zs, zg, M, m, s0, n);
  return done();
}
int probe_head(const float* y, float* tau, int n) {
  if (n < 0 || n > MAX_N) return -1;
  head_kernel<<<ew_blocks(n), EW_THREADS>>>(y, tau, n);
  return done();
}
int probe_sincos(const float* q, float* s, float* c, int n) {
  if (n < 0 || n > MAX_N) return -1;
  sincos_kernel<<<ew_blocks(n), EW_THREADS>>>(q, s, c, n);
  return done();
}
// S k blocks of 16 features (K = 16 S <= 256)
int probe_wx6(const void* A0, const void* A1, const void* A2, const float* X, const float* C,
              float* terms, float* out, int S) {
  if (S < 1 || S > MAX_S) return -1;
  wx6_kernel<<<1, 64>>>(static_cast<const f32x4*>(A0), static_cast<const f32x4*>(A1),
                        static_cast<const f32x4*>(A2), X, C, terms, out, S);
  return done();
}
// S k blocks of 32 features (K = 32 S <= 512)
int probe_nx6(const void* A0, const void* A1, const void* A2, const float* X, const float* C,
              float* terms, float* out, int S) {
  if (S < 1 || S > MAX_S) return -1;
  nx6_kernel<<<1, 64>>>(static_cast<const f32x4*>(A0), static_cast<const f32x4*>(A1),
                        static_cast<const f32x4*>(A2), X, C, terms, out, S);
  return done();
}
float probe_wide_kappa() { return WKAPPA; }
float probe_wide_kappa_inv() { return WKAPPA_INV; }
}
