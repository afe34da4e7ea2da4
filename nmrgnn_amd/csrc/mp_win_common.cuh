// Shared device pieces of the F = 64 window kernels: the eight-wave forward and backward (mp_win.hip, mp_win_bwd.hip), their
// sixteen-wave forms (mp_win16.hip, mp_win16_bwd.hip) and, through mp_wave_common.cuh, the wave-autonomous
// ones.  Three parts: winc = what does not depend on the workgroup's geometry (constants, DPP helpers, the rotation gather,
// the aggregate tile, the edge-gradient dot), w8c = 32-atom tiles walked by 512 threads, w16c = 64-atom tiles walked by 1024.
// A kernel file takes one geometry with `using namespace w8c;` or `using namespace w16c;` — either brings winc along.
#pragma once
#include <algorithm>

#include <hip/hip_runtime.h>

#include "mfma_gemm.cuh"   // f4zero
#include "h2_common.cuh"   // split2_pair, dma_rsrc, lds_dma16

namespace ng {

// ---- geometry-independent pieces ---------------------------------------------------------------------------
namespace winc {

constexpr int WF = 64;          // feature width
constexpr int WROWS = 288;      // window rows
constexpr int WC4 = WF / 4;     // float4 per row = lanes per atom

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// min over the 64 lanes, valid in lane 63: row_shr 1,2,4,8 inside rows of 16, then row_bcast 15 / 31
__device__ __forceinline__ int wave_min_i32(int v) {
  const int big = 0x7fffffff;
  v = min(v, __builtin_amdgcn_update_dpp(big, v, 0x111, 0xf, 0xf, false));   // row_shr:1
  v = min(v, __builtin_amdgcn_update_dpp(big, v, 0x112, 0xf, 0xf, false));   // row_shr:2
  v = min(v, __builtin_amdgcn_update_dpp(big, v, 0x114, 0xf, 0xf, false));   // row_shr:4
  v = min(v, __builtin_amdgcn_update_dpp(big, v, 0x118, 0xf, 0xf, false));   // row_shr:8
  v = min(v, __builtin_amdgcn_update_dpp(big, v, 0x142, 0xa, 0xf, false));   // row_bcast:15 -> rows 1,3
  v = min(v, __builtin_amdgcn_update_dpp(big, v, 0x143, 0xc, 0xf, false));   // row_bcast:31 -> rows 2,3
  return v;
}
// row_ror:S inside the 16 lanes of a DPP row
template <int S>
__device__ __forceinline__ int ror_i(int v) {
  if (S == 0) return v;
  return __builtin_amdgcn_update_dpp(0, v, 0x120 + (S & 15), 0xf, 0xf, false);
}
template <int S>
__device__ __forceinline__ float ror_f(float v) {
  return __builtin_bit_cast(float, ror_i<S>(__builtin_bit_cast(int, v)));
}
// acc += w * h for one float4 of features, as two v_pk_fma_f32
__device__ __forceinline__ void pk_axpy(f32x2& lo, f32x2& hi, float w, const float4& h) {
  const f32x2 ww = {w, w};
  lo = __builtin_elementwise_fma(ww, f32x2{h.x, h.y}, lo);
  hi = __builtin_elementwise_fma(ww, f32x2{h.z, h.w}, hi);
}
__device__ __forceinline__ float dot4(const float4& a, const float4& b) {
  return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
}

// ---- rotation gather (K <= 16) -------------------------------------------------------------------------------
// Lane c of an atom's 16-lane row owns neighbour slot c: ONE index and E weights per lane instead of
// every lane reading the whole list (which cost as much LDS bandwidth as the row gather itself).  In
// step s the lane uses the slot of lane (c + s) mod 16, fetched over the DPP network (row_ror:s) —
// each lane walks the neighbours in its own rotated order, the sum is the same.  All sixteen lanes of
// a row read the SAME bank group (4c..4c+3) of sixteen DIFFERENT window rows: still conflict-free.
// four rotation steps: row reads and FMAs are separate so that the reads of the NEXT four steps can be
// issued before the FMAs of the current four (the LDS latency is otherwise exposed: both waves of a SIMD
// run this phase in lockstep and wait at the same time)
template <int S0>
__device__ __forceinline__ void rot_load4(const char* __restrict__ wbytes, int roff, float4 (&h)[4]) {
  h[0] = *reinterpret_cast<const float4*>(wbytes + ror_i<S0 + 0>(roff));
  h[1] = *reinterpret_cast<const float4*>(wbytes + ror_i<S0 + 1>(roff));
  h[2] = *reinterpret_cast<const float4*>(wbytes + ror_i<S0 + 2>(roff));
  h[3] = *reinterpret_cast<const float4*>(wbytes + ror_i<S0 + 3>(roff));
}
// the same four rows from HBM / L2 (tiles whose range is wider than the window)
template <int S0>
__device__ __forceinline__ void rot_load4_global(const float4* __restrict__ src4, int c, int idx, float4 (&h)[4]) {
  h[0] = src4[(int64_t)ror_i<S0 + 0>(idx) * WC4 + c];
  h[1] = src4[(int64_t)ror_i<S0 + 1>(idx) * WC4 + c];
  h[2] = src4[(int64_t)ror_i<S0 + 2>(idx) * WC4 + c];
  h[3] = src4[(int64_t)ror_i<S0 + 3>(idx) * WC4 + c];
}
template <int E, int S0>
__device__ __forceinline__ void rot_fma4(const float4 (&h)[4], const float (&w)[E], f32x2 (&lo)[E], f32x2 (&hi)[E]) {
#pragma unroll
  for (int n = 0; n < E; ++n) pk_axpy(lo[n], hi[n], ror_f<S0 + 0>(w[n]), h[0]);
#pragma unroll
  for (int n = 0; n < E; ++n) pk_axpy(lo[n], hi[n], ror_f<S0 + 1>(w[n]), h[1]);
#pragma unroll
  for (int n = 0; n < E; ++n) pk_axpy(lo[n], hi[n], ror_f<S0 + 2>(w[n]), h[2]);
#pragma unroll
  for (int n = 0; n < E; ++n) pk_axpy(lo[n], hi[n], ror_f<S0 + 3>(w[n]), h[3]);
}

// ---- aggregate tile in LDS: TA atoms x E*64 --------------------------------------------------------------------
// H2 = false: fp32 rows [TA][E*64 + 4].  H2 = true: two fp16 piece planes [2][TA][E*64 + 8] (h2_common.cuh): the gather
// splits its sums where they are formed and the matrix phase runs on v_mfma_f32_16x16x32_f16 (18 instead of 48 MFMAs
// per wave and 32-atom tile at E = 3); aggregates are O(1-10) activations and are split unscaled.
template <int TA, int E>
struct AggTile {
  static constexpr int KF = E * WF;
  static constexpr int LD = KF + 4;                    // fp32 row stride (floats)
  static constexpr int ROWB = (KF + 8) * 2;            // fp16 plane row stride (bytes): 16 rows on disjoint 4-bank groups
  static constexpr int PLANE = TA * ROWB;
  static constexpr int BYTES_F32 = TA * LD * 4, BYTES_H2 = 2 * PLANE;
  static constexpr int BYTES = BYTES_H2 > BYTES_F32 ? BYTES_H2 : BYTES_F32;      // room for either form
};

// H2 rows carry a power-of-two scale when their largest entry reaches 2^15 (an aggregate of features is a forward quantity
// of any size — the reference's MPLayer is plain fp32): the 16 lanes of the row's DPP row hold all of it, the inverse goes
// to rs[atom] for the epilogue.  Every ordinary row has scale 1 and the same bits as without.
template <int TA, int E, bool H2>
__device__ __forceinline__ void tile_put(float* __restrict__ tb, int al, int c, f32x2 (&lo)[E], f32x2 (&hi)[E],
                                         float* __restrict__ rs) {
  if (H2) {
    float m = 0.f;
#pragma unroll
    for (int n = 0; n < E; ++n)
      m = fmaxf(fmaxf(m, fmaxf(fabsf(lo[n][0]), fabsf(lo[n][1]))), fmaxf(fabsf(hi[n][0]), fabsf(hi[n][1])));
    float rsv = 1.0f;
    if (__builtin_amdgcn_ballot_w64(m >= 32768.0f) != 0) {      // wave-uniform and never taken for ordinary activations
      m = fmaxf(m, ror_f<8>(m)); m = fmaxf(m, ror_f<4>(m)); m = fmaxf(m, ror_f<2>(m)); m = fmaxf(m, ror_f<1>(m));
      const int ef = (__builtin_bit_cast(int, m) >> 23) & 255;
      const bool big = ef >= 127 + 15 && ef != 255;
      const float S = big ? __builtin_bit_cast(float, (268 - ef) << 23) : 1.0f;       // 2^(14 - e): |S x| < 2^15
      rsv = big ? __builtin_bit_cast(float, (ef - 14) << 23) : 1.0f;
      const f32x2 S2 = {S, S};
#pragma unroll
      for (int n = 0; n < E; ++n) { lo[n] *= S2; hi[n] *= S2; }
    }
    if (c == 0) rs[al] = rsv;
    char* p = reinterpret_cast<char*>(tb) + al * AggTile<TA, E>::ROWB + 8 * c;
#pragma unroll
    for (int n = 0; n < E; ++n) {
      unsigned h0, l0, h1, l1;
      split2_pair(lo[n][0], lo[n][1], h0, l0);
      split2_pair(hi[n][0], hi[n][1], h1, l1);
      *reinterpret_cast<u32x2*>(p + n * (WF * 2)) = u32x2{h0, h1};
      *reinterpret_cast<u32x2*>(p + n * (WF * 2) + AggTile<TA, E>::PLANE) = u32x2{l0, l1};
    }
  } else {
#pragma unroll
    for (int n = 0; n < E; ++n)
      *reinterpret_cast<float4*>(tb + al * AggTile<TA, E>::LD + n * WF + 4 * c) = make_float4(lo[n][0], lo[n][1], hi[n][0], hi[n][1]);
  }
}

// ---- edge-gradient dot: de[i][j][n] = <dA[i][n][:], h[nlist[i][j]][:]> ------------------------------------------------
// one rotation step: this lane's chunk of dA[i][n][:] against the row of the slot that the rotation brings here; the
// partial lands in the accumulator of THAT slot's lane afterwards.  GLOBAL: rows from HBM / L2 instead of the window
template <int E, int S, bool GLOBAL>
__device__ __forceinline__ void edge_step(const char* __restrict__ wbytes, const float4* __restrict__ src4, int c, int roff,
                                          int gidx, const float4 (&da)[E], float (&out)[E]) {
  float4 hrow;
  if (!GLOBAL) hrow = *reinterpret_cast<const float4*>(wbytes + ror_i<S>(roff));
  else hrow = src4[(int64_t)ror_i<S>(gidx) * WC4 + c];
#pragma unroll
  for (int n = 0; n < E; ++n) {
    const float p = dot4(da[n], hrow);
    // slot (c + S) was processed here; rotate the partial back to its owner: out_j = sum_S ror_{16-S}(p_S)
    out[n] += ror_f<(16 - S) & 15>(p);
  }
}
// lane = (atom al of the tile, slot lane & 15) with the slot's neighbour index idx in a register; tb = the dA tile, row stride ld
template <int E, bool GLOBAL>
__device__ __forceinline__ void edge_dot(int lane, int al, int wlo, int idx, const float* __restrict__ tb, int ld,
                                         const float4* __restrict__ win4, const float4* __restrict__ src4, float (&out)[E]) {
  const int c = lane & 15;
  const int roff = min(max(idx - wlo, 0), WROWS - 1) * (WF * 4);
  const char* wbytes = reinterpret_cast<const char*>(win4) + 16 * c;
  float4 da[E];
#pragma unroll
  for (int n = 0; n < E; ++n) {
    da[n] = *reinterpret_cast<const float4*>(tb + al * ld + n * WF + 4 * c);
    out[n] = 0.f;
  }
  edge_step<E, 0, GLOBAL>(wbytes, src4, c, roff, idx, da, out);
  edge_step<E, 1, GLOBAL>(wbytes, src4, c, roff, idx, da, out);
  edge_step<E, 2, GLOBAL>(wbytes, src4, c, roff, idx, da, out);
  edge_step<E, 3, GLOBAL>(wbytes, src4, c, roff, idx, da, out);
  edge_step<E, 4, GLOBAL>(wbytes, src4, c, roff, idx, da, out);
  edge_step<E, 5, GLOBAL>(wbytes, src4, c, roff, idx, da, out);
  edge_step<E, 6, GLOBAL>(wbytes, src4, c, roff, idx, da, out);
  edge_step<E, 7, GLOBAL>(wbytes, src4, c, roff, idx, da, out);
  edge_step<E, 8, GLOBAL>(wbytes, src4, c, roff, idx, da, out);
  edge_step<E, 9, GLOBAL>(wbytes, src4, c, roff, idx, da, out);
  edge_step<E, 10, GLOBAL>(wbytes, src4, c, roff, idx, da, out);
  edge_step<E, 11, GLOBAL>(wbytes, src4, c, roff, idx, da, out);
  edge_step<E, 12, GLOBAL>(wbytes, src4, c, roff, idx, da, out);
  edge_step<E, 13, GLOBAL>(wbytes, src4, c, roff, idx, da, out);
  edge_step<E, 14, GLOBAL>(wbytes, src4, c, roff, idx, da, out);
  edge_step<E, 15, GLOBAL>(wbytes, src4, c, roff, idx, da, out);
}

template <int E>
struct EdgeDots { float v[E]; };      // returned in registers: an array passed out by pointer lived on the stack

// The global-memory variant is kept out of line: inlined next to the window variant it makes the compiler put vmcnt
// waits (for registers its loads may target) into the window path, which then stalls on the prefetch in flight.
template <int E>
__device__ __noinline__ EdgeDots<E> edge_dot_global(int lane, int al, int idx, const float* tb, int ld, const float4* src4) {
  float out[E];
  edge_dot<E, true>(lane, al, 0, idx, tb, ld, nullptr, src4, out);
  EdgeDots<E> r;
#pragma unroll
  for (int n = 0; n < E; ++n) r.v[n] = out[n];
  return r;
}

}  // namespace winc

// ---- eight-wave geometry: 32-atom tiles, 512 threads ------------------------------------------------------------------
namespace w8c {

using namespace winc;

constexpr int WTA = 32;         // atoms per tile
constexpr int WTHREADS = 512;

// every thread takes the same decision from the eight partial ranges (ctl[wave], ctl[8 + wave]); returns true when the
// window has to be restaged at the (updated) wlo.  mode: 0 = gather from the window, 1 = gather from global memory
__device__ __forceinline__ bool win_decide(const int* __restrict__ ctl, int& wlo, int& mode) {
  int lo = ctl[0], hi = ctl[8];
#pragma unroll
  for (int i = 1; i < 8; ++i) { lo = min(lo, ctl[i]); hi = max(hi, ctl[8 + i]); }
  mode = 0;
  if (hi < lo) return false;                                  // empty tile
  if (lo >= wlo && hi < wlo + WROWS) return false;            // window hit
  if (hi - lo + 1 > WROWS) { mode = 1; return false; }        // too wide
  wlo = max(0, lo - (WROWS - (hi - lo + 1)) / 2);
  return true;
}

// the window through registers: rows wlo .. wlo+287 of src4, rows past N as zeros
__device__ __forceinline__ void win_stage(float4* __restrict__ win4, const float4* __restrict__ src4,
                                          int wlo, int64_t N, int tid) {
  float4 v[9];
#pragma unroll
  for (int u = 0; u < 9; ++u) {
    const int idx = tid + WTHREADS * u;
    const int64_t row = (int64_t)wlo + (idx >> 4);
    v[u] = row < N ? src4[row * WC4 + (idx & 15)] : f4zero();
  }
#pragma unroll
  for (int u = 0; u < 9; ++u) win4[tid + WTHREADS * u] = v[u];
}
static_assert(WROWS * WC4 == 9 * WTHREADS, "window staging assumes 9 float4 per thread");

}  // namespace w8c

// ---- sixteen-wave geometry: 64-atom tiles, 1024 threads ---------------------------------------------------------------
namespace w16c {

using namespace winc;

constexpr int WTA = 64;         // atoms per tile
constexpr int WTHREADS = 1024;
constexpr int NW = WTHREADS / 64;

// as the eight-wave decision, from the sixteen partial ranges (ctl[wave], ctl[NW + wave]); a range whose width overflows
// an int is too wide as well
__device__ __forceinline__ bool win_decide(const int* __restrict__ ctl, int& wlo, int& mode) {
  int lo = ctl[0], hi = ctl[NW];
#pragma unroll
  for (int i = 1; i < NW; ++i) { lo = min(lo, ctl[i]); hi = max(hi, ctl[NW + i]); }
  mode = 0;
  if (hi < lo) return false;                                  // empty tile
  if (lo >= wlo && hi < wlo + WROWS) return false;            // window hit
  if (hi - lo + 1 > WROWS || hi - lo < 0) { mode = 1; return false; }      // too wide: gather from global memory
  wlo = max(0, lo - (WROWS - (hi - lo + 1)) / 2);
  return true;
}

// The window by LDS-DMA: its 288 rows are one contiguous 72-KB block of the source array — 72 wave-instructions of 1 KB
// straight into LDS, no registers in between.  The buffer is the block itself (base = row wlo, clipped at the array's end:
// rows past it read as zeros), so there is no 32-bit limit on the array and no register-staged second path (whose five
// per-lane 64-bit addresses, hoisted out of the tile loop, were spilled and reloaded every tile).
__device__ __forceinline__ void win_dma(float* __restrict__ win, const float* __restrict__ src, int wlo_v, int64_t N, int wave, int lane) {
  const int wlo = __builtin_amdgcn_readfirstlane(wlo_v);
  const int64_t rows = std::min<int64_t>(N - wlo, WROWS);
  const dma_i4 rs = dma_rsrc(src + (int64_t)wlo * WF, (unsigned)(rows * (WF * 4)));
#pragma unroll
  for (int j = 0; j < (WROWS * WF * 4 / 1024 + NW - 1) / NW; ++j) {
    const int kb = wave + NW * j;
    if (kb < WROWS * WF * 4 / 1024) lds_dma16(rs, reinterpret_cast<char*>(win) + kb * 1024, lane * 16, kb * 1024);
  }
}

}  // namespace w16c
}  // namespace ng
