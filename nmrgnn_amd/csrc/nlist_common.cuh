// The pieces the neighbour-list builders share (knn.hip, knn_cells.hip, ragged.hip, cutoff.hip), one copy of each: keys and
// cross-lane helpers, the sorted insertion, the wave-per-query selection, the row write-outs, the position-tile staging, the
// cutoff hit body and the host-side K ladder.  Every bit-for-bit promise between the builders (cell grid == brute force,
// ragged == uniform, count pass == fill pass) rests on their running the same expressions: they are here so that they are.
//
// The squared distance is pbc_dist2 (pbc.cuh, where DispTric::image needs it): ONE explicit fused-multiply-add chain,
// fmaf(dz, dz, fmaf(dy, dy, dx * dx)).  Left to -ffp-contract two instantiations may round differently by an ulp, and then
// two builders order a tie differently, or a cutoff row sized by the count pass is filled with one entry more.
//
// Why most pieces are macros: these kernels keep fully unrolled lists in registers, and the compiler's handling of them
// depends on when it sees the code.  Each piece was first written as a __forceinline__ function; every one of them that is a
// macro below changed the instructions of its kernels in that form (the insertion: knn_kernel<16, DispOpen> 49 -> 74 VGPRs
// with array references, 53 with a struct that owns the lists, and the occupancy with them; the others: another block layout
// or schedule, the key pack 30 to 76 more SGPRs in most wave kernels).  Expanded in place, every kernel is instruction for
// instruction what it was with its private copy.
//
// How to use the macros.  Each is ONE statement and wants its semicolon (do { } while (0)), so it is safe under an unbraced
// if / else; the exception is NG_KNN_WAVE_SELECT, which declares its result and says so.  Value arguments (upper case, and
// K, scale, lane, the output pointers) are parenthesised and evaluated where the private copy had them, some more than once:
// pass expressions without side effects.  The lists and counters a macro assigns (bd, bi, key, mn, LIST, cnt, cnt_pos, the
// tile sx / sy / sz) must be plain names of the caller's variables.  Locals end in an underscore; no argument may.  A #define
// is not scoped by the namespace below: the NG_ prefix is what keeps these apart from the rest of the library.
#pragma once
#include "pbc.cuh"

namespace ng {

constexpr int NL_TILE = 1024;      // candidates per [3][NL_TILE] LDS tile of the uniform brute-force kernels

// ---- keys ---------------------------------------------------------------------------------------------------------------
// (bits of the squared distance) << 32 | index: squared distances are non-negative floats, whose bit patterns order like the
// values, so key order IS (distance, index) order — one compare per slot instead of three
typedef unsigned long long knn_u64;
constexpr knn_u64 KNN_KEY_EMPTY = ((knn_u64)0x7f800000u << 32) | 0x7fffffffu;      // (inf, no index): the cell-grid lists
#define NG_KNN_KEY(D2, J) (((knn_u64)__builtin_bit_cast(unsigned, (D2)) << 32) | (J))
__device__ __forceinline__ float knn_key_d2(knn_u64 k) { return __builtin_bit_cast(float, (unsigned)(k >> 32)); }
__device__ __forceinline__ int knn_key_index(knn_u64 k) { return (int)(unsigned)k; }

__device__ __forceinline__ knn_u64 knn_readlane64(knn_u64 v, int l) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
  return ((knn_u64)hi << 32) | lo;
}
// lane l gets lane l - 1's value, lane 0 gets 0 (DPP wave_shr:1)
__device__ __forceinline__ knn_u64 knn_shr1(knn_u64 v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)v, 0x138, 0xf, 0xf, false);
  const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(v >> 32), 0x138, 0xf, 0xf, false);
  return ((knn_u64)hi << 32) | lo;
}

// ---- rows [T0, T0 + CNT) of one frame's positions FP -> the [3][NL_TILE] tile sx / sy / sz of the workgroup (256 threads) --
#define NG_NL_STAGE(sx, sy, sz, FP, T0, CNT)                                                                            \
  do {                                                                                                                  \
    __syncthreads();                                                                                                    \
    for (int t_ = threadIdx.x; t_ < (CNT); t_ += 256) {                                                                 \
      sx[t_] = (FP)[3 * ((T0) + t_)]; sy[t_] = (FP)[3 * ((T0) + t_) + 1]; sz[t_] = (FP)[3 * ((T0) + t_) + 2];           \
    }                                                                                                                   \
    __syncthreads();                                                                                                    \
  } while (0)

// ---- the sorted (distance, index) list of a brute-force thread: float bd[KMAX], int bi[KMAX] in registers -----------------
// Candidate (D2, J) into the list unless it is the query SELF, fully unrolled and branch-free; comparisons are strict, so
// among equal distances the one inserted first (the lower index: candidates come in ascending index) stays in front.
#define NG_KNN_INSERT(KMAX, bd, bi, D2, J, SELF)                                              \
  do {                                                                                        \
    if ((D2) < bd[(KMAX) - 1] && (J) != (SELF)) {                                             \
      _Pragma("unroll") for (int k_ = (KMAX) - 1; k_ >= 1; --k_) {                            \
        const bool shift_ = bd[k_ - 1] > (D2);          /* old element k-1 moves up */        \
        const bool here_ = !shift_ && bd[k_] > (D2);    /* candidate lands in slot k */       \
        bi[k_] = shift_ ? bi[k_ - 1] : (here_ ? (J) : bi[k_]);                                \
        bd[k_] = shift_ ? bd[k_ - 1] : (here_ ? (D2) : bd[k_]);                               \
      }                                                                                       \
      if (bd[0] > (D2)) { bd[0] = (D2); bi[0] = (J); }                                        \
    }                                                                                         \
  } while (0)

// The row ROW of a (bd, bi) list of KMAX slots, K of them written; a slot the search left at infinity is written as (0, 0.0).
// BASE + index is the batch-global index and index > FIRST means structure-local index > 0, what inv_degree counts
// (library.py:115-116): the uniform kernels pass (frame * n, 0), the ragged one (0, r.lo).
#define NG_KNN_WRITE_ROW(KMAX, K, bd, bi, ROW, BASE, FIRST, scale, nlist, edges, inv_degree) \
  do {                                                                                      \
    const int64_t row_ = (ROW);                                                             \
    int deg_ = 0;                                                                           \
    _Pragma("unroll") for (int k_ = 0; k_ < (KMAX); ++k_) {                                 \
      if (k_ < (K)) {                                                                       \
        const bool ok_ = bd[k_] < INFINITY;                                                 \
        (nlist)[row_ * (K) + k_] = ok_ ? (BASE) + bi[k_] : 0;                               \
        (edges)[row_ * (K) + k_] = ok_ ? sqrtf(bd[k_]) * (scale) : 0.f;                     \
        deg_ += (ok_ && bi[k_] > (FIRST)) ? 1 : 0;                                          \
      }                                                                                     \
    }                                                                                       \
    (inv_degree)[row_] = deg_ > 0 ? 1.0f / (float)deg_ : 0.f;                               \
  } while (0)

// the same row from a 64-bit-key list (the cell grid: indices local to the frame that starts at row BASE)
#define NG_KNN_WRITE_KEY_ROW(KMAX, K, key, ROW, BASE, scale, nlist, edges, inv_degree) \
  do {                                                                                \
    const int64_t row_ = (ROW);                                                       \
    int deg_ = 0;                                                                     \
    _Pragma("unroll") for (int k_ = 0; k_ < (KMAX); ++k_) {                           \
      if (k_ < (K)) {                                                                 \
        const float d2_ = knn_key_d2(key[k_]);                                        \
        const int j_ = knn_key_index(key[k_]);                                        \
        const bool ok_ = d2_ < INFINITY;                                              \
        (nlist)[row_ * (K) + k_] = ok_ ? (BASE) + j_ : 0;                             \
        (edges)[row_ * (K) + k_] = ok_ ? sqrtf(d2_) * (scale) : 0.f;                  \
        deg_ += (ok_ && j_ > 0) ? 1 : 0;                                              \
      }                                                                               \
    }                                                                                 \
    (inv_degree)[row_] = deg_ > 0 ? 1.0f / (float)deg_ : 0.f;                         \
  } while (0)

// ---- one WAVE per query: phases B and C of knn_wave_kernel (knn.hip), and the row of the list they leave -----------------
// key[s]: the key of this lane's candidate 64 s + lane (index local to the frame or structure; ~0 for none), mn their
// minimum.  DECLARES LIST in the caller's scope, the list held across the lanes: lane k = k-th smallest key, ~0 where the
// candidates ran out.  Because it declares (LIST, and its own tau_ and kth_), it is a run of statements and not one: use it
// once per scope, at block level, never as the body of an unbraced if or loop (a semicolon after it is an empty statement).
#define NG_KNN_WAVE_SELECT(STEPS, key, mn, K, LIST)                                                              \
  /* B: the K-th smallest lane minimum (keys of real candidates are distinct; absent ones are ~0 and rank last) */ \
  knn_u64 tau_ = ~0ull;                                                                                          \
  {                                                                                                              \
    int rank_ = 0;                                                                                               \
    for (int b_ = 0; b_ < 64; ++b_) rank_ += knn_readlane64(mn, b_) < mn ? 1 : 0;                                \
    const unsigned long long hit_ = __ballot(rank_ == (K) - 1 && mn != ~0ull);                                   \
    if (hit_) tau_ = knn_readlane64(mn, __builtin_ctzll(hit_));                                                  \
  }                                                                                                              \
  /* C: insert what lies at or below the bound: one wave-wide shift and two compares per insertion */            \
  knn_u64 LIST = ~0ull, kth_ = ~0ull;                                                                            \
  _Pragma("unroll") for (int s_ = 0; s_ < (STEPS); ++s_) {                                                       \
    unsigned long long m_ = __ballot(key[s_] <= tau_ && key[s_] != ~0ull);                                       \
    while (m_) {                                                                                                 \
      const int b_ = __builtin_ctzll(m_);                                                                        \
      m_ &= m_ - 1;                                                                                              \
      const knn_u64 c_ = knn_readlane64(key[s_], b_);                                                            \
      if (c_ < kth_) {                                                                                           \
        const knn_u64 prev_ = knn_shr1(LIST);                                                                    \
        LIST = c_ < prev_ ? prev_ : (c_ < LIST ? c_ : LIST);                                                     \
        kth_ = knn_readlane64(LIST, (K) - 1);                                                                    \
      }                                                                                                          \
    }                                                                                                            \
  }

// lane k writes slot k of row ROW; the list's indices are local to the frame or structure that starts at row BASE
#define NG_KNN_WAVE_WRITE_ROW(LIST, lane, K, ROW, BASE, scale, nlist, edges, inv_degree)   \
  do {                                                                                     \
    const int64_t row_ = (ROW);                                                            \
    const bool ok_ = (lane) < (K) && LIST != ~0ull;                                        \
    const int idx_ = (int)(unsigned)LIST;                                                  \
    const float d2_ = __builtin_bit_cast(float, (unsigned)(LIST >> 32));                   \
    if ((lane) < (K)) {                                                                    \
      (nlist)[row_ * (K) + (lane)] = ok_ ? (BASE) + idx_ : 0;                              \
      (edges)[row_ * (K) + (lane)] = ok_ ? sqrtf(d2_) * (scale) : 0.f;                     \
    }                                                                                      \
    const int deg_ = __popcll(__ballot(ok_ && idx_ > 0));                                  \
    if ((lane) == 0) (inv_degree)[row_] = deg_ > 0 ? 1.0f / (float)deg_ : 0.f;             \
  } while (0)

// ---- the cutoff hit of the one-thread kernels: candidate J of query I at squared distance D2 ----------------------------
// Counts it and, in the fill pass, writes (BASE + J, distance * scale, row ROW) at out + cnt: a row never writes past its
// own extent [out, lim), whatever the count pass saw.  J > FIRST: structure-local index > 0, as NG_KNN_WRITE_ROW.
#define NG_CUTOFF_HIT(FILL, D2, J, I, BASE, FIRST, ROW, cutoff2, scale, out, lim, col, dist, row_of, cnt, cnt_pos) \
  do {                                                                                                           \
    if ((D2) < (cutoff2) && (J) != (I)) {                                                                        \
      if ((FILL) && (out) + cnt < (lim)) {                                                                       \
        (col)[(out) + cnt] = (BASE) + (J);                                                                       \
        (dist)[(out) + cnt] = sqrtf(D2) * (scale);                                                               \
        if (row_of) (row_of)[(out) + cnt] = (ROW);                                                               \
      }                                                                                                          \
      ++cnt;                                                                                                     \
      cnt_pos += (J) > (FIRST) ? 1 : 0;                                                                          \
    }                                                                                                            \
  } while (0)

// ---- host: the list length of the kernel templates, KMAX = 16 / 32 / 64 for K; LAUNCH(KMAX) is the caller's launch ---------
#define NG_KNN_LADDER(K, LAUNCH) \
  do { if ((K) <= 16) { LAUNCH(16); } else if ((K) <= 32) { LAUNCH(32); } else { LAUNCH(64); } } while (0)

}  // namespace ng
