#pragma once
// Wide τ / ∇τ kernels: 32 (start, goal) pairs per wave, every layer on split-bf16 MFMA
// ("wide kernels").
//
// Why 32 pairs: beside MFMAs on gfx950 every vector-memory instruction steals MFMA issue
// cycles (tests/diag/vmem_probe.hip, mfma32_probe.hip), and the 16-pair kernel of pntf_field.h
// loads one 1 KiB weight fragment per 4-8 of its MFMAs.  With 32 pairs as the MFMA's N
// dimension the weight stream costs half the loads per pair.
//
// Layout (same "transposed" formulation as pntf_field.h, 32-row tiles):
//   * lane l = (j, h), j = l & 31 the pair, h = l >> 5; a 32-feature activation tile is one
//     f32x16 per lane, register r holding feature row(r, h) = (r & 3) + 8 (r >> 2) + 4 h —
//     the C/D layout of the 32x32 MFMAs, so a layer's output tile is the next layer's B
//     operand as is: registers 8b..8b+7 are the B operand of k block b (16 features) of
//     v_mfma_f32_32x32x16_bf16;
//   * the weights are the A operand.  The fp32 "wide fragment order" (OFF_WIDE,
//     pack_wide_kernel), one buffer_load_dwordx4 per lane for 4 consecutive registers,
//        P[(((ot·KT + kt)·4 + u)·64 + l)·4 + s] = M[32 ot + (l & 31)][32 kt + 8 u + 4 (l >> 5) + s]
//     is read by the fp32 Fourier fold only; the layers read its split-bf16 copy (OFF_X6,
//     pack_x6_kernel): per 32 x 32 step 6 fragments, 3b + term for k block b, in each layer's
//     step order, so a layer streams linearly and the ring crosses layer boundaries;
//   * the bias enters as one fp32 MFMA per out tile (A = the bias column on the h = 0 lanes,
//     B = 1), and a residual as that MFMA's C operand, so neither costs VALU work;
//   * activations live in two banks X[8], Y[8] (256 features, or 2 points x 128 features),
//     both kept in the AGPR file; a layer accumulates straight into its out bank (xlayer);
//   * saved σ10 tiles (4 KiB per 32-feature tile and point) go to a per-wave scratch slot,
//     except the eight the reverse sweep needs at once, which stay in LDS.
// The one fp32 layer left is the Fourier fold of the instantiation that reads the environment
// table from global memory (BL = false, wide_fold); with the table in LDS (the headline's) the
// fold runs on split-bf16 too (wide_fold_x).
#include "pntf_field.h"
#include "pntf_stamp.h"

namespace pntf {

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r] = 0.f;
  return z;
}

// ---------------------------------------------------------------- split-bf16 products
// Each fp32 product runs as six v_mfma_f32_32x32x16_bf16 on three-term bf16 splits of both
// operands (the training GEMMs' scheme, pntf_gemm.hip x6_split): 2.67x the fp32 MFMA rate at
// fp32-level accuracy (20.4 -> 15.4 ms against the fp32 MFMA layers, DESIGN.md §3,
// profiles/r05_wide_x6.txt).  A tile's registers 8b..8b+7 are the B operand of k block b as
// they are (lane (j, h) holds feature rows wrow(8b + i, h), i = 0..7); the weights are
// pre-split in the same k order (OFF_X6, pack_x6_kernel).
// Weight fragments per split-bf16 step.  The ring must be that wide: the wide units build with
// -DPNTF_RING_NL=6 (pntf/build.py), and run_steps asserts it where a kernel is instantiated
// (the other units include this header with their 4-fragment rings).
constexpr int WNL = 6;
typedef __bf16 wbf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 wbf16x2 __attribute__((ext_vector_type(2)));
typedef float wf32x2 __attribute__((ext_vector_type(2)));
// three-term RNE split of registers 8b..8b+7 of a tile (x = x0 + x1 + x2, each bf16)
__device__ __forceinline__ void wx6_split(const f32x16& v, int b, wbf16x8 (&s)[3]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    wf32x2 x = {v[8 * b + 2 * i], v[8 * b + 2 * i + 1]};
    const wbf16x2 p0 = __builtin_convertvector(x, wbf16x2);
#ifdef PNTF_ABL_NOSPLIT   // diagnostics only (tests/diag ablations): one term, wrong results
    s[0][2 * i] = s[1][2 * i] = s[2][2 * i] = p0[0];
    s[0][2 * i + 1] = s[1][2 * i + 1] = s[2][2 * i + 1] = p0[1];
    continue;
#endif
#if PNTF_X6_DOT
    const wf32x2 r1 = x6_resid(x, p0);
    const wbf16x2 p1 = __builtin_convertvector(r1, wbf16x2);
    const wf32x2 r2 = x6_resid(r1, p1);
#else
    const wf32x2 r1 = x - __builtin_convertvector(p0, wf32x2);
    const wbf16x2 p1 = __builtin_convertvector(r1, wbf16x2);
    const wf32x2 r2 = r1 - __builtin_convertvector(p1, wf32x2);
#endif
    const wbf16x2 p2 = __builtin_convertvector(r2, wbf16x2);
    s[0][2 * i] = p0[0]; s[0][2 * i + 1] = p0[1];
    s[1][2 * i] = p1[0]; s[1][2 * i + 1] = p1[1];
    s[2][2 * i] = p2[0]; s[2][2 * i + 1] = p2[1];
  }
}
// the six products of order >= 2^-16, the small ones first
__device__ __forceinline__ f32x16 wx6_mma(const f32x4& w0, const f32x4& w1, const f32x4& w2,
                                          const wbf16x8 (&x)[3], f32x16 acc) {
  const wbf16x8 a0 = __builtin_bit_cast(wbf16x8, w0), a1 = __builtin_bit_cast(wbf16x8, w1),
                a2 = __builtin_bit_cast(wbf16x8, w2);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, x[0], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, x[1], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, x[2], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, x[0], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, x[1], acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, x[0], acc, 0, 0, 0);
}
// Activations carried pre-scaled by κ = 10/ln 2 (round 4).  The forward pass keeps
// y' = κ·y and h' = κ·h: encoder[0]'s weights and every forward bias column are packed times κ
// (pack_wide_kernel / pack_wide_aux_kernel), the interior layers' weights are not (W·h' + κ·b
// = κ·y), and the head row divides it out once per pair.  Then e^{-10|y|} = 2^{-|y'|} needs no
// scaling multiply and softplus₁₀'s log term no constant: κ·softplus₁₀(y) = max(y', 0) +
// log₂(1 + 2^{-|y'|}); σ(10 y) is unchanged, so the reverse sweep (σ tiles, unscaled Wᵀ) is
// as before.  One VALU op fewer per activation element (tests/diag ablation: -0.5 %).
// Tested on their own (tests/test_device_primitives.py): wx6_split's terms equal
// the RNE split bit for bit, wx6_mma issues exactly the six products (planted operands make a
// dropped one a gross error), and wsp_sig(fl(κ·y)) holds σ(10y) and, times ln 2 / 10,
// softplus₁₀(y) to 8·eps32·A with the rounding of κ·y counted in A; for y' >= 24 (10y >= 16.64)
// 1 + 2^{-y'} rounds to 1 and sp' is y' bit for bit.
constexpr float WKAPPA = WIDE_KAPPA;                  // 10 / ln 2
constexpr float WKAPPA_INV = 0.0693147180559945309f;  // ln 2 / 10
__device__ __forceinline__ SpSig wsp_sig(float y) {   // y = κ·(pre-activation)
#ifdef PNTF_ABL_CHEAPACT   // diagnostics only (tests/diag ablations): no transcendentals
  return SpSig{fmaxf(y, 0.f) * 0.5f + 0.01f, 0.5f};
#endif
  const float t = __builtin_amdgcn_exp2f(-fabsf(y));
  const float u = 1.f + t;
  const float r = __builtin_amdgcn_rcpf(u);
  const bool pos = y >= 0.f;
  SpSig o;
  // κ·softplus₁₀ (log2: v_log_f32), with the rounding error of 1 + t added back (pntf_field.h
  // one_plus_err; 1/ln 2 turns it into log2) so that the value is fp32-relative for y < 0 too
  o.sp = fmaf(one_plus_err(t, u), 1.44269504088896341f, pos ? y : 0.f) + __builtin_amdgcn_logf(u);
  o.sg = pos ? r : t * r;
  return o;
}

// feature row of register r in lane half h of a 32-row tile
__device__ __forceinline__ constexpr int wrow(int r, int h) {
  return (r & 3) + 8 * (r >> 2) + 4 * h;
}

// ---------------------------------------------------------------- scratch (saved σ10)
struct WScratch {
  Rsrc r;
};
__device__ __forceinline__ WScratch make_wscratch(float* p) {
  return WScratch{make_rsrc(p, p ? WSCRATCH_FLOATS_PER_WAVE * 4 : 0)};
}

// ---------------------------------------------------------------- LDS σ tiles
// The σ tiles the reverse sweep consumes at once when a phase starts — generator[-2]'s four
// (the head step, right after the forward -> reverse drain) and the merge switch's four (the
// merge Jacobian) — stay in LDS: 8 tiles x 4 KiB per wave, 128 KiB per workgroup (the kernel
// uses no other LDS).  From the scratch slot each of those reloads waited out a whole HBM
// round trip with nothing else in flight.  Layout as the scratch tiles: part q of a tile is
// 1 KiB contiguous (lane-major f32x4), so ds_write_b128 / ds_read_b128 are conflict-free.
typedef __attribute__((address_space(3))) f32x4 wlds_f4;
constexpr int WL_G3 = 0, WL_S0 = 4, WL_TILES = 8;
typedef __attribute__((address_space(3))) float wlds_f;
struct WLds {
  wlds_f4* p;          // this wave's region, offset by the lane
  const wlds_f* hw;    // the head row generator.4.weight (128 floats, staged once per workgroup)
};
__device__ __forceinline__ void lstore(WLds l, int t, const f32x16& v) {
#pragma unroll
  for (int q = 0; q < 4; ++q)
    l.p[(t * 4 + q) * 64] = f32x4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
}
__device__ __forceinline__ f32x16 lload(WLds l, int t) {
  f32x16 v;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const f32x4 p = l.p[(t * 4 + q) * 64];
#pragma unroll
    for (int s = 0; s < 4; ++s) v[4 * q + s] = p[s];
  }
  return v;
}

// ---------------------------------------------------------------- weight stream heads
constexpr int WF = (OFF_WIDE + OFF_FWD) * 4;   // byte base of the forward wide fragments
constexpr int WB = (OFF_WIDE + OFF_BWD) * 4;   // ... of the transposed ones
constexpr int WBC = (OFF_WIDE + W_OFF_BCOL) * 4;
constexpr int WHW = (OFF_WIDE + W_OFF_G4W) * 4;
constexpr int WG4B = (OFF_WIDE + W_OFF_G4B) * 4;

// A head gives the byte offset of fragment l of step j of a step sequence; WF / WB + OFF_*
// name a matrix by its byte offset in the fp32 wide region, and its split copy sits at 1.5x
// that offset in OFF_X6.
constexpr int wx6_base(int wide_base) { return OFF_X6 * 4 + (wide_base - OFF_WIDE * 4) / 2 * 3; }
// a layer (xlayer): its split copy is packed in its (kt, ot) step order, so step j reads
// fragments 6j..6j+5
struct WHead {
  int base;
  __device__ int operator()(int j, int l) const { return wx6_base(base) + (j * 6 + l) * 1024; }
};
// encoder[0] on Fourier features (OT 4, KT 8), (kt, ot) steps as any layer
struct WE0Head {
  __device__ int operator()(int j, int l) const {
    return wx6_base(WF + OFF_E0 * 4) + (j * 6 + l) * 1024;
  }
};
// reverse sweep head: generator[-2]^T (OT 8, KT 4)
__device__ __forceinline__ WHead wbwd_head() { return WHead{WB + OFF_G3 * 4}; }
// fp32 Fourier fold (wide_fold; encoder[0]^T, OT 8, KT 4) on the fp32 wide fragments: step
// st = (o·4 + kt)·2 + half reads the 4 fragments of out tile o + 4·half (sin rows o, cos rows
// o + 4)
struct WFoldHead {
  __device__ int operator()(int j, int l) const {
    const int o = j / 8, kt = (j / 2) % 4, half = j % 2;
    return WB + OFF_E0 * 4 + ((((o + 4 * half) * 4 + kt) * 4 + l) * 1024);
  }
};
// split-bf16 Fourier fold (wide_fold_x): step S = (p·4 + kt)·4 + ot_local over two passes p of
// 4 out tiles (sin/cos rows of feature tiles 2p, 2p + 1); the split copy of encoder[0]^T is
// packed in this order (pack_x6_kernel)
struct WFoldXHead {
  __device__ int operator()(int j, int l) const {
    return wx6_base(WB + OFF_E0 * 4) + (j * 6 + l) * 1024;
  }
};
// fragments per step of whatever a step sequence hands over to
template <class F>
constexpr int wnext_nl() {
  return std::is_same<F, WFoldHead>::value ? 4 : WNL;
}

// bias-column operands of a layer: fragment g holds out tiles 4g..4g+3 (lanes 0-31)
template <int OT>
struct BiasCols {
  f32x4 v[(OT + 3) / 4];
  __device__ __forceinline__ void load(Rsrc W, int lane, int plain_off) {
#pragma unroll
    for (int g = 0; g < (OT + 3) / 4; ++g)
      v[g] = bload(W, lane * 16, WBC + ((plain_off / 128 + g) * 64) * 16);
  }
  __device__ __forceinline__ float operator()(int ot) const { return v[ot / 4][ot % 4]; }
};

// env B reads (Fourier projections and fold) and head-row reads, each behind a hook for
// the tests/diag ablations (PNTF_ABL_NOBW / PNTF_ABL_NOHW: register stand-ins, wrong results)
__device__ __forceinline__ f32x4 wbw_load(const float* p) {
#ifdef PNTF_ABL_NOBW
  float v = 1e-3f * (float)(reinterpret_cast<uintptr_t>(p) & 255);
  asm volatile("v_mov_b32 %0, %0" : "+v"(v));
  return f32x4{v, v + 1e-4f, v + 2e-4f, v + 3e-4f};
#else
  return ld4(p);
#endif
}
// Where a lane reads its environment's B rows: global memory (any table), or the table staged
// in LDS once per workgroup when it fits (WBL_FLOATS; pntf_capi.hip picks the kernel).  The LDS
// reads take the Fourier projections' and the fold's B loads off the in-order vmcnt queue.
// Every use is of fl(2π·B) (load2pi): the staged table holds that product (the kernel scales
// it once per workgroup while staging), the global-table reads multiply per use.
template <bool BL>
struct WBt {
  __device__ __forceinline__ f32x4 load2pi(const PairIO& io, int i) const {
    return TWO_PI * wbw_load(io.Bw + i);
  }
};
template <>
struct WBt<true> {
  const wlds_f* t;   // this lane's environment in the staged table of 2π·B
  __device__ __forceinline__ f32x4 load2pi(const PairIO&, int i) const {
#ifdef PNTF_ABL_NOBW
    return TWO_PI * wbw_load(reinterpret_cast<const float*>(static_cast<uintptr_t>(i)));
#else
    return *reinterpret_cast<const wlds_f4*>(t + i);
#endif
  }
};

// head-row features 32 t + 8 u + 4 h .. + 3 (the rows of registers 4u..4u+3 of tile t): an
// LDS broadcast read (half the lanes share each address).  From the packed blob these 16
// loads per pass were sunk to their use and each waited out an L2 round trip with the whole
// weight ring (vmcnt(0)); tests/diag ablation: -0.5 % kernel time.
__device__ __forceinline__ f32x4 whw_load(const WLds& wl, int t, int u, int h) {
#ifdef PNTF_ABL_NOHW
  float v = 1e-3f * (float)((t * 4 + u + h) & 255);
  asm volatile("v_mov_b32 %0, %0" : "+v"(v));
  return f32x4{v, v + 1e-4f, v + 2e-4f, v + 3e-4f};
#else
  return *reinterpret_cast<const wlds_f4*>(wl.hw + 32 * t + 8 * u + 4 * h);
#endif
}

// ---------------------------------------------------------------- Fourier projections
// q[c][r] = x_c · 2πB[:, 32 kt + row(r, h)] for the lane's 16 feature rows of Fourier tile
// kt, both points; the B rows come from the pair's environment (io.Bw, dim x 128).
template <int DIM, class BT>
__device__ __forceinline__ void wfourier_q(const PairIO& io, const BT& bt, int kt, int h,
                                           f32x16 (&q)[2]) {
#pragma unroll
  for (int c = 0; c < 2; ++c) q[c] = zero16();
#pragma unroll
  for (int d = 0; d < DIM; ++d)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const f32x4 b = bt.load2pi(io, d * H + 32 * kt + 8 * u + 4 * h);
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int s = 0; s < 4; ++s) q[c][4 * u + s] = fmaf(io.x[c][d], b[s], q[c][4 * u + s]);
    }
}

// ---------------------------------------------------------------- Fourier fold (fp32)
// encoder[0]^T (256 x 128: OT 8, KT 4) fused with the Fourier Jacobian (:639-645), the last
// phase of the reverse sweep; Y holds dL/d(encoder[0] output) (2 points x 4 tiles).  On
// v_mfma_f32_32x32x2_f32 with the fp32 wide fragments, for the instantiation that reads the
// environment table from global memory: its registers fit beside the lane's B pointers, which
// wide_fold_x's do not (the split-bf16 fold is worth 0.2 ms of 14.6 where it fits, DESIGN.md
// §3 round 6).
template <int DIM, class BT, class AfterF>
__device__ __forceinline__ void wide_fold(Ring& ring, Rsrc W, const PairIO& io, BT bt,
                                          const f32x16 (&Y)[8], int lane, float (&ds)[DIM],
                                          float (&dg)[DIM], AfterF after) {
  const int h = lane >> 5;
  // Feature tile o pairs sin rows (out tile o) with cos rows (out tile o + 4) of the same q;
  // step (o, kt, half) accumulates half's out tile; after (o, 3, 1) the tile pair folds
  //   dτ/dx_c += Σ_rows 2πB[:, f] (dφ_sin cos q_f - dφ_cos sin q_f)
  float acc[2][DIM];
#pragma unroll
  for (int d = 0; d < DIM; ++d) acc[0][d] = acc[1][d] = 0.f;
  f32x16 ph[2][2];   // [sin | cos rows][point]
  run_steps<32, 4, wnext_nl<AfterF>(), SITE_FOLD>(
      ring, W, lane * 16, WFoldHead{}, after, [&](auto st, const f32x4 (&a)[4]) {
        constexpr int S = decltype(st)::value;
        constexpr int o = S / 8, kt = (S / 2) % 4, half = S % 2;
        if constexpr (kt == 0) {
#pragma unroll
          for (int c = 0; c < 2; ++c) ph[half][c] = zero16();
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int c = 0; c < 2; ++c)
              ph[half][c] = mfma32(a[u][s], Y[c * 4 + kt][4 * u + s], ph[half][c]);
        if constexpr (kt == 3 && half == 1) {
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            f32x4 bw[DIM];
#pragma unroll
            for (int d = 0; d < DIM; ++d) bw[d] = bt.load2pi(io, d * H + 32 * o + 8 * u + 4 * h);
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
              for (int s = 0; s < 4; ++s) {
                float q = 0.f;
#pragma unroll
                for (int d = 0; d < DIM; ++d) q = fmaf(io.x[c][d], bw[d][s], q);
                float sn, cs;
                sincos_fast(q, sn, cs);
                const int r = 4 * u + s;
                float gg = ph[0][c][r] * cs - ph[1][c][r] * sn;
#pragma unroll
                for (int d = 0; d < DIM; ++d) acc[c][d] = fmaf(bw[d][s], gg, acc[c][d]);
              }
          }
        }
      });
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    ds[d] = acc[0][d] + __shfl_xor(acc[0][d], 32);
    dg[d] = acc[1][d] + __shfl_xor(acc[1][d], 32);
  }
}

// ================================================================ accumulate-in-bank layers
// On gfx950 every VALU instruction beside v_mfma_f32_32x32x16_bf16 costs ~3 cycles wherever it
// is placed (profiles/r06_coexec_bf16_probe.txt), so the layer engine is built to issue as few
// as possible and to spread them over the steps (15.3 -> 14.4 ms against
// separate accumulators with grouped out tiles, profiles/r06_wide_variants.txt r06h):
//   * the out bank is the accumulator: out tile ot of the layer IS the MFMA C/D (the residual
//     is its initial value, the bias one fp32 MFMA at kt = 0), so no accumulator registers are
//     needed beside the two banks and each input tile is split once per layer, shared by all
//     its out tiles — the split is the largest VALU item (3.3 ms of 15.3 without sharing);
//   * steps (kt, ot), ot fastest; input tile kt is split at ot = 0;
//   * the epilogue of out tile t (softplus/σ with its four 16-byte σ stores, or the reverse
//     sweep's σ multiply) runs FUSED with the split of that tile in the NEXT layer, at its step
//     (kt = t, ot = 0): the tile-column is read out of the bank once, the epilogue applied in
//     VGPRs and the result split from there.  It is written back to the bank only where it is
//     read again after that layer (KEEP: a residual C-init, the Fourier fold's second pass);
//     the first layer of a residual block, whose output is nothing but the next layer's input,
//     never returns to the bank.  Running the epilogue ahead of the split (in chunks over the
//     steps before it) cost a bank read and write per element on top of the split's own read;
//     VALU work costs the same wherever it is placed, so only the count matters;
//   * the reverse sweep's σ tile of out tile t (4 NC quads) is loaded XPDS = 3 steps before
//     the split that uses it: tile 0's in the layer's own step STEPS - 3, tile t's in the next
//     layer's step t·OT - 3, after tile t - 1's quads were used at step (t - 1)·OT.
constexpr int XPDS = 3;
// no epilogue pending on the input bank: the tiles are split as they stand
struct XPlain {
  static constexpr bool EPI = false, PF = false;
  __device__ __forceinline__ void prefetch(int) {}
};
// every pending epilogue at once, written back (before a phase that reads the whole bank)
template <class L>
__device__ __forceinline__ void xflush(L& ly) {
  if constexpr (L::EPI) {
    static_for<0, L::OT>([&](auto tt) {
      constexpr int t = decltype(tt)::value;
      if constexpr (L::PF && t > 0) ly.prefetch(t);
#pragma unroll
      for (int c = 0; c < L::NC; ++c) ly.template tile<true>(t, c);
    });
  }
}

// Banks in the AGPR file: the banks pass an empty asm with an AGPR operand in every step (the
// VGPR file then holds the ring, the splits and the epilogue's temporaries; the fused
// epilogue + split reads a bank through v_accvgpr_read).  Left to the compiler both banks sit
// in the VGPR file and 190-310 VGPRs spill; one bank in each file is spill-free only with a
// shorter ring and ran 12-57 % slower (profiles/r06_wide_variants.txt
// r06o).
__device__ __forceinline__ void xagpr(f32x16& t) { asm("" : "+a"(t)); }

// One Linear layer on split-bf16 MFMA, accumulating in ly.out (bank index c·OT + ot), input
// bank `in` (c·KT + kt).  ly.init(ot) starts out tile ot at kt = 0 (bias MFMA / residual /
// zero).  pv is the layer that wrote `in` (pv.out is `in`) with its epilogue still pending, or
// XPlain: step (kt, 0) takes input tile kt through pv's epilogue and splits the result; KEEP
// says whether the bank gets it back.  pre(st) runs first in every step (loads for the next
// layer).
template <int OT, int KT, int NC, int SITE, bool KEEP, class L, class P, class PreF, class NextF>
__device__ __forceinline__ void xlayer(Ring& ring, Rsrc W, int wbase, f32x16 (&in)[8],
                                       int lane, L& ly, P& pv, PreF pre, NextF naddr) {
  static_assert(NC * KT <= 8 && NC * OT <= 8, "bank size");
  static_assert(L::OT == OT && L::KT == KT && L::NC == NC, "layer object shape");
  static_assert(XPDS < OT, "tile t - 1's sigma quads are used before tile t's are loaded");
  if constexpr (P::EPI) static_assert(P::OT == KT && P::NC == NC, "previous layer's shape");
  constexpr int STEPS = OT * KT;
  wbf16x8 xs[NC][2][3];
  run_steps<STEPS, WNL, wnext_nl<NextF>(), SITE>(
      ring, W, lane * 16, WHead{wbase}, naddr, [&](auto st, const f32x4 (&a)[WNL]) {
        constexpr int S = decltype(st)::value;
        constexpr int kt = S / OT, ot = S % OT;
        pre(st);
        if constexpr (P::PF && (S + XPDS) % OT == 0 && (S + XPDS) / OT < KT)
          pv.prefetch((S + XPDS) / OT);
        if constexpr (ot == 0) {
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            f32x16 v;
            if constexpr (P::EPI) v = pv.template tile<KEEP>(kt, c);
            else v = in[c * KT + kt];
#pragma unroll
            for (int b = 0; b < 2; ++b) wx6_split(v, b, xs[c][b]);
          }
        }
        if constexpr (kt == 0) ly.init(ot);
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int c = 0; c < NC; ++c)
            ly.out[c * OT + ot] = wx6_mma(a[3 * b], a[3 * b + 1], a[3 * b + 2], xs[c][b],
                                          ly.out[c * OT + ot]);
#pragma unroll
        for (int c = 0; c < NC; ++c) xagpr(ly.out[c * OT + ot]);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          xagpr(in[t]);
          xagpr(ly.out[t]);
        }
        if constexpr (L::PF && S == STEPS - XPDS) ly.prefetch(0);
      });
}

// ---- layer objects: OT, KT, NC; EPI: an epilogue pends on the out tiles; PF: it needs σ
// prefetches.  tile<KEEP>(t, c) reads out tile-column (t, c) from the bank, applies the
// epilogue, writes the result back when KEEP, and returns it.
// forward Linear + softplus10: out = sp(A·in + b (+ out if RES)); σ10 saved when SAVE (scratch
// tile sc0 + c·OT + t, or LDS tiles when IN_LDS); ACT0: encoder[0]'s compat quirk (:435-438)
template <int OT_, int KT_, int NC_, bool RES, bool SAVE, bool IN_LDS = false, bool ACT0 = false>
struct XFwdAct {
  static constexpr int OT = OT_, KT = KT_, NC = NC_;
  static constexpr bool EPI = true, PF = false;
  f32x16 (&out)[8];
  WScratch sc;
  int sc0, lane;
  BiasCols<OT_> bc;
  WLds wl;
  float cm;   // ACT0: 1 in compat mode
  __device__ __forceinline__ void init(int ot) {
#pragma unroll
    for (int c = 0; c < NC; ++c)
      out[c * OT + ot] = mfma32(bc(ot), 1.f, RES ? out[c * OT + ot] : zero16());
  }
  __device__ __forceinline__ void prefetch(int) {}
  template <bool KEEP>
  __device__ __forceinline__ f32x16 tile(int t, int c) {
    f32x16 v = out[c * OT + t];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      f32x4 g;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const SpSig r = wsp_sig(v[4 * q + s]);
        v[4 * q + s] = r.sp;
        g[s] = ACT0 ? fmaf(cm, __builtin_amdgcn_rcpf(2.f - r.sg) - r.sg, r.sg) : r.sg;
      }
      if constexpr (SAVE && IN_LDS) wl.p[((sc0 + c * OT + t) * 4 + q) * 64] = g;
      // nt: the σ stores stream past the L2 that holds the weights
      else if constexpr (SAVE) bstore<AUX_NT>(sc.r, g, lane * 16, (sc0 + c * OT + t) * 4096 + q * 1024);
    }
    if constexpr (KEEP) out[c * OT + t] = v;
    return v;
  }
};
// forward Linear without activation (encoder[-1], :234): nothing pending
template <int OT_, int KT_, int NC_>
struct XFwdLin {
  static constexpr int OT = OT_, KT = KT_, NC = NC_;
  static constexpr bool EPI = false, PF = false;
  f32x16 (&out)[8];
  BiasCols<OT_> bc;
  __device__ __forceinline__ void init(int ot) {
#pragma unroll
    for (int c = 0; c < NC; ++c) out[c * OT + ot] = mfma32(bc(ot), 1.f, zero16());
  }
  __device__ __forceinline__ void prefetch(int) {}
};
// reverse: out = (A^T·in (+ out if RES)) ⊙ σ tile mul0 + c·OT + t (if MUL); a tile's σ quads
// (4 per column) are loaded XPDS steps ahead of the fused split that multiplies by them
template <int OT_, int KT_, int NC_, bool RES, bool MUL>
struct XBwd {
  static constexpr int OT = OT_, KT = KT_, NC = NC_;
  static constexpr bool EPI = MUL, PF = MUL;
  f32x16 (&out)[8];
  WScratch sc;
  int mul0, lane;
  f32x4 sg[4 * NC_];
  __device__ __forceinline__ void init(int ot) {
    if constexpr (!RES) {
#pragma unroll
      for (int c = 0; c < NC; ++c) out[c * OT + ot] = zero16();
    }
  }
  __device__ __forceinline__ void prefetch(int t) {
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        sg[c * 4 + q] = __builtin_bit_cast(
            f32x4, __builtin_amdgcn_raw_buffer_load_b128(sc.r, lane * 16,
                                                         (mul0 + c * OT + t) * 4096 + q * 1024,
                                                         AUX_LOAD));
  }
  template <bool KEEP>
  __device__ __forceinline__ f32x16 tile(int t, int c) {
    // the product is rounded to fp32 before the split subtracts its leading term from it: it
    // must not contract into that subtraction as an fma (the bank gets the rounded product,
    // and the three terms must sum to it)
#pragma clang fp contract(off)
    f32x16 v = out[c * OT + t];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int s = 0; s < 4; ++s) v[4 * q + s] *= sg[c * 4 + q][s];
    if constexpr (KEEP) out[c * OT + t] = v;
    return v;
  }
};

// the split-bf16 fold in the kernels that stage the env-B table in LDS (the headline's); the
// global-table instantiations run the fp32 fold (wide_fold)
template <class BT>
constexpr bool xfold() { return std::is_same<BT, WBt<true>>::value; }

// ---------------------------------------------------------------- Fourier fold (split-bf16)
// encoder[0]^T on split-bf16 MFMA fused with the Fourier Jacobian (:639-645).  Two passes; in
// pass p the four out tiles sin(o), cos(o) for o = 2p, 2p + 1 accumulate in X (dead here:
// X[c·4 + ot_local]) over the 4 input tiles of Y, each input tile split once per pass and
// shared by the 4 tiles; after the pass the two feature tiles fold into dτ/dx_c as wide_fold.
// pv is encoder block 0's first layer transposed (a0ᵀ, out = Y) with its σ multiply pending:
// pass 0's split of tile kt runs it (as xlayer does) and writes Y back for pass 1.
template <int DIM, class BT, class P, class AfterF>
__device__ __forceinline__ void wide_fold_x(Ring& ring, Rsrc W, const PairIO& io, BT bt,
                                            f32x16 (&X)[8], f32x16 (&Y)[8], P& pv, int lane,
                                            float (&ds)[DIM], float (&dg)[DIM], AfterF after) {
  static_assert(P::OT == 4 && P::NC == 2, "previous layer's shape");
  const int h = lane >> 5;
  float acc[2][DIM];
#pragma unroll
  for (int d = 0; d < DIM; ++d) acc[0][d] = acc[1][d] = 0.f;
  wbf16x8 xs[2][2][3];
  run_steps<32, WNL, wnext_nl<AfterF>(), SITE_FOLD>(
      ring, W, lane * 16, WFoldXHead{}, after, [&](auto st, const f32x4 (&a)[WNL]) {
        constexpr int S = decltype(st)::value;
        constexpr int p = S / 16, kt = (S / 4) % 4, otl = S % 4;
        if constexpr (P::PF && p == 0 && (S + XPDS) % 4 == 0 && (S + XPDS) / 4 < 4)
          pv.prefetch((S + XPDS) / 4);
        if constexpr (otl == 0) {
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            f32x16 v;
            if constexpr (P::EPI && p == 0) v = pv.template tile<true>(kt, c);
            else v = Y[c * 4 + kt];
#pragma unroll
            for (int b = 0; b < 2; ++b) wx6_split(v, b, xs[c][b]);
          }
        }
        if constexpr (kt == 0) {
#pragma unroll
          for (int c = 0; c < 2; ++c) X[c * 4 + otl] = zero16();
        }
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int c = 0; c < 2; ++c)
            X[c * 4 + otl] = wx6_mma(a[3 * b], a[3 * b + 1], a[3 * b + 2], xs[c][b], X[c * 4 + otl]);
#pragma unroll
        for (int c = 0; c < 2; ++c) xagpr(X[c * 4 + otl]);
#pragma unroll
        for (int t = 0; t < 8; ++t) xagpr(Y[t]);   // both banks in the AGPR file (as xlayer)
        // after the pass: feature tiles o = 2p + ol, sin rows X[c·4 + 2 ol], cos X[c·4 + 2 ol + 1]
        if constexpr (kt == 3 && otl == 3) {
#pragma unroll
          for (int ol = 0; ol < 2; ++ol) {
            const int o = 2 * p + ol;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              f32x4 bw[DIM];
#pragma unroll
              for (int d = 0; d < DIM; ++d)
                bw[d] = bt.load2pi(io, d * H + 32 * o + 8 * u + 4 * h);
#pragma unroll
              for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                  float q = 0.f;
#pragma unroll
                  for (int d = 0; d < DIM; ++d) q = fmaf(io.x[c][d], bw[d][s], q);
                  float sn, cs;
                  sincos_fast(q, sn, cs);
                  const int r = 4 * u + s;
                  const float gg = X[c * 4 + 2 * ol][r] * cs - X[c * 4 + 2 * ol + 1][r] * sn;
#pragma unroll
                  for (int d = 0; d < DIM; ++d) acc[c][d] = fmaf(bw[d][s], gg, acc[c][d]);
                }
            }
          }
        }
      });
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    ds[d] = acc[0][d] + __shfl_xor(acc[0][d], 32);
    dg[d] = acc[1][d] + __shfl_xor(acc[1][d], 32);
  }
}

// ---------------------------------------------------------------- forward pass
// NN.out on 32 pairs.  GRAD: save σ tiles.  On entry the ring holds WE0Head; on return the
// first PF steps of `after`.  Returns τ of the lane's pair (same in both lane halves).  The
// encoder[0] epilogue and every layer's run fused with the next layer's split (above); KEEP
// where the tile is a residual (e0, b0, gb), not where it is only the next layer's input (a0,
// a1, b1, ga, the last gb).
template <int DIM, bool GRAD, class BT, class AfterF>
__device__ __forceinline__ float wide_forward_x(Ring& ring, Rsrc W, const PairIO& io, BT bt,
                                                f32x16 (&X)[8], f32x16 (&Y)[8], WScratch sc,
                                                WLds wl, int compat, int lane, AfterF after) {
  const int h = lane >> 5;
  // ---- encoder[0] (:186-190, :227), k-tile outer: X[c·4 + ot] accumulate 4 out tiles x 2
  // points; sin tiles (kt < 4) are computed at step (kt, 0), their cos partners (kt + 4)
  // kept in Y[c·4 + kt] until then; the input tile (sin or cos) is split once per kt and
  // shared by the 4 out tiles
  XFwdAct<4, 8, 2, false, GRAD, false, true> e0{X, sc, WT_E0, lane, {}, wl, compat ? 1.f : 0.f};
  e0.bc.load(W, lane, B_E0);
  XFwdAct<4, 4, 2, false, GRAD> a0{Y, sc, WT_EBLK, lane, {}, wl, 0.f};
  {
    f32x16 q[2], sn[2];
    wbf16x8 xs[2][2][3];
    wfourier_q<DIM>(io, bt, 0, h, q);
    run_steps<32, WNL, WNL, SITE_FWD_E0>(
        ring, W, lane * 16, WE0Head{}, WHead{WF + OFF_EBLK * 4},
        [&](auto st, const f32x4 (&a)[WNL]) {
          constexpr int S = decltype(st)::value;
          constexpr int kt = S / 4, ot = S % 4;
          if constexpr (ot == 0 && kt < 4) {
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
              for (int r = 0; r < 16; ++r) {
                float x0, x1;
                sincos_fast(q[c][r], x0, x1);
                sn[c][r] = x0;
                Y[c * 4 + kt][r] = x1;
              }
          }
          if constexpr (ot == 0) {
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
              for (int b = 0; b < 2; ++b)
                wx6_split(kt < 4 ? sn[c] : Y[c * 4 + (kt & 3)], b, xs[c][b]);
          }
          if constexpr (kt == 0) e0.init(ot);
#pragma unroll
          for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int c = 0; c < 2; ++c)
              X[c * 4 + ot] = wx6_mma(a[3 * b], a[3 * b + 1], a[3 * b + 2], xs[c][b], X[c * 4 + ot]);
#pragma unroll
          for (int c = 0; c < 2; ++c) xagpr(X[c * 4 + ot]);
#pragma unroll
          for (int t = 0; t < 8; ++t) {
            xagpr(X[t]);
            if (kt >= 4 || t % 4 < kt) xagpr(Y[t]);   // the cos tiles already computed
          }
          // next sin/cos tile's projections, after this tile's MFMAs are issued
          if constexpr (ot == 3 && kt < 3) wfourier_q<DIM>(io, bt, kt + 1, h, q);
          if constexpr (S == 16) a0.bc.load(W, lane, B_EBLK);
        });
  }

  // ---- encoder residual blocks (:228-232); X = h (2 points x 4 tiles).  Each layer's bias
  // columns are fetched at the first step of the layer before it.
  const int WE = WF + OFF_EBLK * 4;
  {
    XFwdAct<4, 4, 2, true, GRAD> b0{X, sc, WT_EBLK + 8, lane, {}, wl, 0.f};
    XFwdAct<4, 4, 2, false, GRAD> a1{Y, sc, WT_EBLK + 16, lane, {}, wl, 0.f};
    XFwdAct<4, 4, 2, true, GRAD> b1{X, sc, WT_EBLK + 24, lane, {}, wl, 0.f};
    XFwdLin<4, 4, 2> e3{Y, {}};
    xlayer<4, 4, 2, SITE_FWD_ENC, true>(ring, W, WE, X, lane, a0, e0,
                                        at<0>([&] { b0.bc.load(W, lane, B_EBLK + 128); }),
                                        WHead{WE + SZ_E * 4});
    xlayer<4, 4, 2, SITE_FWD_ENC, false>(ring, W, WE + SZ_E * 4, Y, lane, b0, a0,
                                         at<0>([&] { a1.bc.load(W, lane, B_EBLK + 256); }),
                                         WHead{WE + 2 * SZ_E * 4});
    xlayer<4, 4, 2, SITE_FWD_ENC, true>(ring, W, WE + 2 * SZ_E * 4, X, lane, a1, b0,
                                        at<0>([&] { b1.bc.load(W, lane, B_EBLK + 384); }),
                                        WHead{WE + 3 * SZ_E * 4});
    xlayer<4, 4, 2, SITE_FWD_ENC, false>(ring, W, WE + 3 * SZ_E * 4, Y, lane, b1, a1,
                                         at<0>([&] { e3.bc.load(W, lane, B_E3); }),
                                         WHead{WF + OFF_E3 * 4});
    // ---- encoder[-1] (:234) -> Y (zs = Y[0..3], zg = Y[4..7])
    xlayer<4, 4, 2, SITE_FWD_ENC, false>(ring, W, WF + OFF_E3 * 4, X, lane, e3, b1, NoPre{},
                                         WHead{WF + OFF_GBLK * 4});
  }

  // ---- symmetric smooth max / min merge (:236-244) -> X (u = [M | m], 8 tiles)
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    f32x16 s0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float zs = Y[t][r], zg = Y[4 + t][r];   // κ-scaled
      float d = zs - zg;
      float e = __builtin_amdgcn_exp2f(-fabsf(d));    // e^{-10|zs - zg|}
      float ue = 1.f + e;                             // κ·0.1·ln(1 + e), as wsp_sig's log term
      float cc = fmaf(one_plus_err(e, ue), 1.44269504088896341f, __builtin_amdgcn_logf(ue));
      X[t][r] = fmaxf(zs, zg) + cc;
      X[4 + t][r] = fminf(zs, zg) - cc;
      float rr = __builtin_amdgcn_rcpf(ue);
      s0[r] = (d >= 0.f) ? rr : e * rr;
    }
    if (GRAD) lstore(wl, WL_S0 + t, s0);
  }

  // ---- generator residual blocks (:246-249), rotated so that one loop body carries a
  // layer's pending epilogue into the next: ga0; (gb_i, ga_{i+1}) for i = 0, 1; gb2; g3
  XFwdAct<8, 8, 1, false, GRAD> ga{Y, sc, WT_GBLK, lane, {}, wl, 0.f};
  XFwdAct<8, 8, 1, true, GRAD> gb{X, sc, WT_GBLK + 8, lane, {}, wl, 0.f};
  ga.bc.load(W, lane, B_GBLK);
  XPlain plain;
  xlayer<8, 8, 1, SITE_FWD_GEN, true>(ring, W, WF + OFF_GBLK * 4, X, lane, ga, plain,
                                      at<0>([&] { gb.bc.load(W, lane, B_GBLK + 256); }),
                                      WHead{WF + (OFF_GBLK + SZ_G) * 4});
#pragma unroll 1
  for (int i = 0; i < 2; ++i) {
    const int wb = opaque(WF + (OFF_GBLK + (2 * i + 1) * SZ_G) * 4);
    const int wa = opaque(WF + (OFF_GBLK + (2 * i + 2) * SZ_G) * 4);
    const int wn = opaque(WF + (OFF_GBLK + (2 * i + 3) * SZ_G) * 4);
    const int ba = opaque(B_GBLK + (2 * i + 2) * 256);
    gb.sc0 = opaque(WT_GBLK + 16 * i + 8);
    xlayer<8, 8, 1, SITE_FWD_GEN, false>(ring, W, wb, Y, lane, gb, ga,
                                         at<0>([&] { ga.bc.load(W, lane, ba); }), WHead{wa});
    ga.sc0 = opaque(WT_GBLK + 16 * i + 16);
    xlayer<8, 8, 1, SITE_FWD_GEN, true>(ring, W, wa, X, lane, ga, gb,
                                        at<0>([&] { gb.bc.load(W, lane, ba + 256); }),
                                        WHead{wn});
  }
  // ---- generator block 2's second layer, then generator[-2] + act (:251-252) -> Y[0..3]
  XFwdAct<4, 8, 1, false, GRAD, true> g3{Y, sc, WL_G3, lane, {}, wl, 0.f};
  gb.sc0 = WT_GBLK + 16 * 2 + 8;
  xlayer<8, 8, 1, SITE_FWD_GEN, false>(ring, W, WF + (OFF_GBLK + 5 * SZ_G) * 4, Y, lane, gb, ga,
                                       at<0>([&] { g3.bc.load(W, lane, B_G3); }),
                                       WHead{WF + OFF_G3 * 4});
  xlayer<4, 8, 1, SITE_FWD_GEN, false>(ring, W, WF + OFF_G3 * 4, X, lane, g3, gb, NoPre{}, after);
  xflush(g3);
  // ---- head generator[-1] + sigmoid(0.1 y) (:254-255)
  float part = 0.f;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      f32x4 w = whw_load(wl, t, u, h);
#pragma unroll
      for (int s = 0; s < 4; ++s) part = fmaf(w[s], Y[t][4 * u + s], part);
    }
  part += __shfl_xor(part, 32);
  const float y4 = fmaf(part, WKAPPA_INV, bload(W, 0, WG4B)[0]);   // part = κ·(g4w·h3)
  return head_sig(y4);
}

// ---------------------------------------------------------------- reverse sweep
// Exact reverse mode (or out_backgrad when the forward stored the quirk).  On entry the ring
// holds wbwd_head(); on return the first PF steps of `after`.  ds/dg: dτ/dxs, dτ/dxg of the
// lane's pair (same in both halves).
template <int DIM, class BT, class AfterF>
__device__ __forceinline__ void wide_backward_x(Ring& ring, Rsrc W, const PairIO& io, BT bt,
                                                float tau, f32x16 (&X)[8], f32x16 (&Y)[8],
                                                WScratch sc, WLds wl, int lane,
                                                float (&ds)[DIM], float (&dg)[DIM],
                                                AfterF after) {
  const int h = lane >> 5;
  // ---- head and generator[-2] (:592-613): Y[t] = d · g4w ⊙ σ10(y3)
  const float dd = 0.1f * tau * (1.f - tau);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    f32x16 s3 = lload(wl, WL_G3 + t);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      f32x4 w = whw_load(wl, t, u, h);
#pragma unroll
      for (int s = 0; s < 4; ++s) Y[t][4 * u + s] = (dd * w[s]) * s3[4 * u + s];
    }
  }
  // du = G3^T dv ⊙ σ10(y2 of generator block 2) -> X   (G3^T: 256 x 128, OT 8, KT 4)
  XBwd<8, 4, 1, false, true> l3{X, sc, WT_GBLK + 16 * 2 + 8, lane, {}};
  XPlain plain;
  xlayer<8, 4, 1, SITE_BWD_GEN, true>(ring, W, WB + OFF_G3 * 4, Y, lane, l3, plain, NoPre{},
                                      WHead{WB + (OFF_GBLK + 5 * SZ_G) * 4});
  // ---- generator blocks, reverse (:615-618), rotated: lb_2; (la_i, lb_{i-1}) for i = 2, 1;
  // la_0 (no σ: it hands over to encoder[-1]^T).  l3's and la's products stay in the bank as
  // the next la's residual (KEEP); lb's feed only the next transpose.
  XBwd<8, 8, 1, false, true> lb{Y, sc, WT_GBLK + 16 * 2, lane, {}};
  XBwd<8, 8, 1, true, true> la{X, sc, 0, lane, {}};
  xlayer<8, 8, 1, SITE_BWD_GEN, true>(ring, W, WB + (OFF_GBLK + 5 * SZ_G) * 4, X, lane, lb, l3,
                                      NoPre{}, WHead{WB + (OFF_GBLK + 4 * SZ_G) * 4});
#pragma unroll 1
  for (int i = 2; i >= 1; --i) {
    const int wa = opaque(WB + (OFF_GBLK + (2 * i) * SZ_G) * 4);
    const int wb = opaque(WB + (OFF_GBLK + (2 * i - 1) * SZ_G) * 4);
    const int wn = opaque(WB + (OFF_GBLK + (2 * i - 2) * SZ_G) * 4);
    // du = G_i^T da + dr, then ⊙ σ10(y2_{i-1})
    la.mul0 = opaque(WT_GBLK + 16 * (i - 1) + 8);
    xlayer<8, 8, 1, SITE_BWD_GEN, false>(ring, W, wa, Y, lane, la, lb, NoPre{}, WHead{wb});
    // da = (G1_{i-1}^T dr) ⊙ σ10(y1_{i-1}) -> Y
    lb.mul0 = opaque(WT_GBLK + 16 * (i - 1));
    xlayer<8, 8, 1, SITE_BWD_GEN, true>(ring, W, wb, X, lane, lb, la, NoPre{}, WHead{wn});
  }
  {
    XBwd<8, 8, 1, true, false> l0{X, sc, 0, lane, {}};
    xlayer<8, 8, 1, SITE_BWD_GEN, false>(ring, W, WB + OFF_GBLK * 4, Y, lane, l0, lb, NoPre{},
                                         WHead{WB + OFF_E3 * 4});
  }
  // ---- merge Jacobian (:620-627): X[0..3] = dzs, X[4..7] = dzg
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    f32x16 s0 = lload(wl, WL_S0 + t);
    f32x16 s1 = 1.f - s0;
    f32x16 dM = X[t], dm = X[4 + t];
    X[t] = s0 * dM + s1 * dm;
    X[4 + t] = s1 * dM + s0 * dm;
  }
  // ---- encoder[-1]^T ⊙ σ10(y2 of encoder block 1), then the blocks, reverse (:629-636)
  const int WE = WB + OFF_EBLK * 4;
  {
    XBwd<4, 4, 2, false, true> e3{Y, sc, WT_EBLK + 24, lane, {}};
    XBwd<4, 4, 2, false, true> b1{X, sc, WT_EBLK + 16, lane, {}};
    XBwd<4, 4, 2, true, true> a1{Y, sc, WT_EBLK + 8, lane, {}};
    XBwd<4, 4, 2, false, true> b0{X, sc, WT_EBLK, lane, {}};
    XBwd<4, 4, 2, true, true> a0{Y, sc, WT_E0, lane, {}};
    xlayer<4, 4, 2, SITE_BWD_ENC, true>(ring, W, WB + OFF_E3 * 4, X, lane, e3, plain, NoPre{},
                                        WHead{WE + 3 * SZ_E * 4});
    xlayer<4, 4, 2, SITE_BWD_ENC, true>(ring, W, WE + 3 * SZ_E * 4, Y, lane, b1, e3, NoPre{},
                                        WHead{WE + 2 * SZ_E * 4});
    xlayer<4, 4, 2, SITE_BWD_ENC, false>(ring, W, WE + 2 * SZ_E * 4, X, lane, a1, b1, NoPre{},
                                         WHead{WE + 1 * SZ_E * 4});
    xlayer<4, 4, 2, SITE_BWD_ENC, true>(ring, W, WE + 1 * SZ_E * 4, Y, lane, b0, a1, NoPre{},
                                        WHead{WE});
    // a0ᵀ's σ multiply runs in the split-bf16 fold's first-pass splits; the fp32 fold reads
    // all of Y in every step, so there it runs first
    if constexpr (xfold<BT>()) {
      xlayer<4, 4, 2, SITE_BWD_ENC, false>(ring, W, WE, X, lane, a0, b0, NoPre{}, WFoldXHead{});
      wide_fold_x<DIM>(ring, W, io, bt, X, Y, a0, lane, ds, dg, after);
    } else {
      xlayer<4, 4, 2, SITE_BWD_ENC, false>(ring, W, WE, X, lane, a0, b0, NoPre{}, WFoldHead{});
      xflush(a0);
      wide_fold<DIM>(ring, W, io, bt, Y, lane, ds, dg, after);
    }
  }
}

// ---------------------------------------------------------------- kernel
template <int DIM, int KIND, bool BL>
__global__ __launch_bounds__(256, 1) void wide_field_kernel(FieldArgs a) {
  PNTF_CLOCK_SCOPE;
  constexpr bool GRAD = KIND != K_TAU && KIND != K_TRAVEL;
  const int lane = threadIdx.x & 63;
  const int slot = blockIdx.x * WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nslots = gridDim.x * WAVES;
  // tile indices are wave-uniform 32-bit values (kept in SGPRs): tile * WTILE must stay below
  // 2^31, so the host sends batches above 2^31 - 32 pairs to the wave-tile kernel instead
  // (pntf_capi.hip WIDE_MAX_PAIRS)
  const int ntiles = (int)((a.n + WTILE - 1) / WTILE);
  const WScratch sc =
      make_wscratch(GRAD ? a.ws + (int64_t)slot * WSCRATCH_FLOATS_PER_WAVE : nullptr);
  const Rsrc W = make_rsrc(a.P, PACKED_TOTAL_X6 * 4);
  __shared__ f32x4 wsig[GRAD ? WAVES * WL_TILES * 4 * 64 : 1];
  // each wave keeps its own copy of the head row (no workgroup barrier: a wave's LDS reads
  // follow its own writes in order)
  __shared__ f32x4 whead[WAVES * H / 4];
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const WLds wl{(wlds_f4*)wsig + (GRAD ? wv * (WL_TILES * 4 * 64) + lane : 0),
                (const wlds_f*)(whead + wv * (H / 4))};
  ((wlds_f*)(whead + wv * (H / 4)))[lane] = a.P[OFF_BIAS + B_G4W + lane];
  ((wlds_f*)(whead + wv * (H / 4)))[lane + 64] = a.P[OFF_BIAS + B_G4W + lane + 64];
  __shared__ f32x4 wbtab[BL ? WBL_FLOATS / 4 : 1];   // 2π·B (WBt<true>)
  if constexpr (BL) {   // the host checked n_env · DIM · H <= WBL_FLOATS
    const int nb4 = a.n_env * (DIM * H / 4);
    for (int i = threadIdx.x; i < nb4; i += 256)
      wbtab[i] = TWO_PI * *reinterpret_cast<const f32x4*>(a.Btab + 4 * i);
  }
  Ring ring;
  ring_fill<WNL>(ring, W, lane * 16, WE0Head{});
  if constexpr (BL) __syncthreads();
  for (int tile = slot; tile < ntiles; tile += nslots) {
    f32x16 X[8], Y[8];
    // the pair column, re-derived per tile from the lane·16 byte offset every load keeps
    // live (through an opaque copy, so it is not hoisted): a separate loop-invariant copy was
    // the one value that spilled
    int v16 = lane * 16;
    asm volatile("" : "+v"(v16));
    const int64_t pair = (int64_t)(tile * WTILE + ((v16 >> 4) & 31));
    PairIO io;
    const bool ok = load_pair<DIM>(a.xp, a.Btab, a.env, a.n, a.n_env, pair, io);
    WBt<BL> bt;
    if constexpr (BL) bt.t = (const wlds_f*)wbtab + (io.Bw - a.Btab);
    float tau;
    if constexpr (GRAD)
      tau = wide_forward_x<DIM, true>(ring, W, io, bt, X, Y, sc, wl, a.compat, lane,
                                      wbwd_head());
    else
      tau = wide_forward_x<DIM, false>(ring, W, io, bt, X, Y, sc, wl, a.compat, lane,
                                       WE0Head{});
    float ds[DIM], dg[DIM];
    if constexpr (GRAD) {
      drain_stores();
      wide_backward_x<DIM>(ring, W, io, bt, tau, X, Y, sc, wl, lane, ds, dg, WE0Head{});
    }
    const bool store = lane < 32 && pair < a.n;
    store_field<DIM, KIND>(a, pair, ok, store, tau, io, ds, dg);
  }
}

#if defined(PNTF_UTIL)
// ---------------------------------------------------------------- wide weight packing
// dst[(((ot·KT + kt)·4 + u)·64 + l)·4 + s] = M[32 ot + (l & 31)][32 kt + 8 u + 4 (l >> 5) + s]
// with M = src (rows x cols, row stride ld) or M = src^T (trans).
__global__ void pack_wide_kernel(const float* __restrict__ src, int rows, int cols, int ld,
                                 int trans, float scale, float* __restrict__ dst) {
  int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= (int64_t)rows * cols) return;
  int s = o & 3;
  int l = (o >> 2) & 63;
  int u = (o >> 8) & 3;
  int64_t rest = o >> 10;
  int KT = cols / 32;
  int kt = rest % KT;
  int ot = rest / KT;
  int n = 32 * ot + (l & 31);
  int k = 32 * kt + 8 * u + 4 * (l >> 5) + s;
  dst[o] = scale * (trans ? src[(int64_t)k * ld + n] : src[(int64_t)n * ld + k]);
}

// split-bf16 copy of the wide region's two directions (OFF_X6): step g = (matrix, ot, kt) of
// the fp32 region (1024 floats: fragments u = 0..3) becomes fragments 3b + term of k block b,
// whose element i is element i & 3 of fp32 fragment 2b + (i >> 2) of the same lane.  Within a
// matrix the steps are in the order its layer consumes them: (kt, ot) for xlayer and
// encoder[0], the two-pass order of wide_fold_x for encoder[0]^T.
__global__ void pack_x6_kernel(const float* __restrict__ wide, uint16_t* __restrict__ x6) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // (step, block, lane)
  if (t >= (int64_t)(2 * SZ_DIR / 1024) * 2 * 64) return;
  const int lane = (int)(t & 63), b = (int)((t >> 6) & 1);
  const int gf = (int)(t >> 7);   // fp32 step: matrix base + ot·KT + kt
  // the matrix (offset and shape in the direction's OFF_* order; Wᵀ in the second direction)
  const int dir = gf >= SZ_DIR / 1024, f = gf * 1024 - dir * SZ_DIR;
  int m0, out, in;
  if (f < OFF_EBLK) { m0 = OFF_E0; out = 128; in = 256; }
  else if (f < OFF_GBLK) { m0 = OFF_EBLK + (f - OFF_EBLK) / SZ_E * SZ_E; out = in = 128; }
  else if (f < OFF_G3) { m0 = OFF_GBLK + (f - OFF_GBLK) / SZ_G * SZ_G; out = in = 256; }
  else { m0 = OFF_G3; out = 128; in = 256; }
  if (dir) { const int x = out; out = in; in = x; }
  const int OT = out / 32, KT = in / 32;
  const int j = (f - m0) / 1024, ot = j / KT, kt = j % KT;
  // first fragment of (ot, kt, block b) in the layer's step order; term p at + p
  int64_t fr;
  if (dir && m0 == OFF_E0) {
    // encoder[0]^T for the split-bf16 fold: pass p = (ot % 4) / 2 covers feature tiles
    // 2p, 2p + 1 with their sin (ot < 4) and cos (ot >= 4) rows; step (p, kt, ot_local),
    // ot_local = ((ot % 4) % 2)·2 + ot / 4, fragments 3b + term
    const int pp = (ot % 4) / 2, ol = ((ot % 4) % 2) * 2 + ot / 4;
    fr = ((int64_t)(gf - j) + (pp * KT + kt) * 4 + ol) * 6 + 3 * b;
  } else {                     // step (kt, ot), fragments 3b + p
    fr = ((int64_t)(gf - j) + kt * OT + ot) * 6 + 3 * b;
  }
  const float* src = wide + (int64_t)gf * 1024;
  float v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = src[((2 * b + (i >> 2)) * 64 + lane) * 4 + (i & 3)];
  f32x16 tile;
#pragma unroll
  for (int i = 0; i < 16; ++i) tile[i] = v[i & 7];
  wbf16x8 s[3];
  wx6_split(tile, 0, s);
#pragma unroll
  for (int p = 0; p < 3; ++p)
    *reinterpret_cast<wbf16x8*>(x6 + ((fr + p) * 64 + lane) * 8) = s[p];
}

// bias columns, head vector and head bias of the wide region, from the plain bias block
__global__ void pack_wide_aux_kernel(const float* __restrict__ plain, float* __restrict__ wide) {
  const int o = blockIdx.x * blockDim.x + threadIdx.x;
  constexpr int NB = W_SZ_BCOL, NH = W_SZ_G4W;
  if (o < NB) {   // bias columns: fragment g, lane l, element s
    int s = o & 3, l = (o >> 2) & 63, g = o >> 8;
    wide[W_OFF_BCOL + o] = l < 32 ? WKAPPA * plain[128 * g + 32 * s + l] : 0.f;   // κ·bias
  } else if (o < NB + NH) {   // head vector: fragment (4t + u)
    int p = o - NB;
    int s = p & 3, l = (p >> 2) & 63, f = p >> 8;
    int t = f / 4, u = f % 4;
    wide[W_OFF_G4W + p] = plain[B_G4W + 32 * t + 8 * u + 4 * (l >> 5) + s];
  } else if (o < NB + NH + 4) {
    wide[W_OFF_G4B + (o - NB - NH)] = plain[B_G4B + (o - NB - NH)];
  }
}
#endif  // PNTF_UTIL

}  // namespace pntf
