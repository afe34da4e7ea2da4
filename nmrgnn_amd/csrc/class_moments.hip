// Dense per-class moments for an evaluation report (nmrgnn/main.py:93-189, eval-tfrecords): the seven float64 sums of
// metrics.hip, for up to 1024 classes and up to 4 groupings of the name ids (atom name, residue, element, ...) in ONE pass
// over the atoms.  ng_name_metrics holds one bit per class in a uint32 and so stops at 32 classes; here a table
// class_of[m][id] gives the class ROW of name id `id` under grouping m (or -1), all groupings sharing one row space [0, K).
//
// An atom counts when w > 0 (false for 0, -0.0, negatives and NaN) and 0 <= name id < n_ids, and then with weight 1 (the
// reference selects rows by `wi > 0` and is unweighted afterwards).  Per row the sums are
//   {S0 = count, Sd2 = sum (y - p)^2, Sy, Sp, Syy, Spp, Syp},   y and p converted to double before any product.
// No atomics, bitwise deterministic: per-workgroup partials in a fixed order, then a second launch that sums them in a fixed
// order (the two stages of metrics.hip).
//
//   stage 1  workgroup b takes atom tiles b, b + nb, ...  Per tile the 256 threads write {y, p} as doubles and, per grouping,
//            the class row of their atom (-1: not counted / no class) to LDS.  Row r belongs to wave r & 3, lane
//            (r >> 2) & 63, accumulator r >> 8: a thread owns at most 4 rows at K = 1024 (28 doubles of accumulators, in
//            registers), and any K >= 4 spreads its rows over all four waves.  The loading waves also leave, per grouping m
//            and owning wave v, a 64-bit ballot of their atoms whose row under m is one of v's.  Wave v then visits exactly
//            those (atom, grouping) pairs, in the fixed order grouping, atom: the next set bit is found on the scalar unit,
//            the row and {y, p} are LDS reads at one address for the whole wave (a broadcast; the next pair's are issued
//            before this pair's adds), and the owning lane alone (a branch on the exec mask, not a select) adds the seven
//            terms.  Atoms without a label cost the walk nothing.  At the end partial[b][K][7] is written.
//   stage 2  one wave per (row, sum) adds partial[0..nb) (lane-strided, then a butterfly) and writes or adds moments.
//
// The grid is min(tiles, CM_MAX_BLOCKS), a constant and not the CU count: the partial order, and with it every bit of the
// result, is a function of (N, K) alone.  512 workgroups put two on a CU at 131072 atoms: a second wave on every SIMD hides
// LDS latency of the walk.
#include <algorithm>

#include "ng_internal.h"

namespace ng {

constexpr int CM_THREADS = 256;      // = atoms per tile
constexpr int CM_MAX_BLOCKS = 512;   // stage-1 workgroups (a constant: see above); scratch = 512 * K * 56 B, 29 MB at K = 1024
constexpr int CM_WAVES = CM_THREADS / 64;
constexpr int CM_SUMS = 7;
constexpr int CM_MAX_GROUPINGS = 4;
constexpr int CM_MAX_CLASSES = 1024;
constexpr int CM_MAX_IDS = 1 << 24;
constexpr int CM_MAX_OWNED = CM_MAX_CLASSES / CM_THREADS;

struct CmAcc {
  double s[CM_SUMS];
};

__device__ __forceinline__ void cm_add(CmAcc& a, bool mine, const double (&term)[CM_SUMS]) {
  if (mine) {
    asm volatile("" ::: "memory");   // keeps this a branch on the exec mask: seven adds, not seven adds and fourteen selects
#pragma unroll
    for (int j = 0; j < CM_SUMS; ++j) a.s[j] += term[j];
  }
}

// OWNED = ceil(K / 256): the accumulators a thread keeps
template <int OWNED>
__global__ __launch_bounds__(CM_THREADS) void class_moments_partial_kernel(
    int64_t N, int64_t n_tiles, const float* __restrict__ y, const float* __restrict__ w, const int32_t* __restrict__ names,
    const float* __restrict__ pred, int n_ids, int M, const int32_t* __restrict__ class_of, int K,
    double* __restrict__ partial) {
  __shared__ double2 yp[CM_THREADS];
  __shared__ int rows[CM_MAX_GROUPINGS][CM_THREADS];
  __shared__ unsigned long long pairs[CM_MAX_GROUPINGS][CM_WAVES][CM_WAVES];   // [grouping][owning wave][loading wave]
  const int t = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
  const bool walks = wave < K;   // this wave owns at least one row
  CmAcc acc[OWNED];
#pragma unroll
  for (int q = 0; q < OWNED; ++q)
#pragma unroll
    for (int j = 0; j < CM_SUMS; ++j) acc[q].s[j] = 0.0;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t i = tile * CM_THREADS + t;
    int c[CM_MAX_GROUPINGS] = {-1, -1, -1, -1};
    double yd = 0.0, pd = 0.0;
    if (i < N) {
      const int32_t nm = names[i];
      yd = (double)y[i];
      pd = (double)pred[i];
      if (w[i] > 0.f && nm >= 0 && nm < n_ids) {   // w > 0 is false for NaN; ids outside the table are in no class
#pragma unroll
        for (int m = 0; m < CM_MAX_GROUPINGS; ++m) {
          if (m < M) {
            const int32_t r = class_of[(int64_t)m * n_ids + nm];
            c[m] = (r >= 0 && r < K) ? r : -1;     // a value outside [-1, K) is -1: never an index
          }
        }
      }
    }
    yp[t] = make_double2(yd, pd);
#pragma unroll
    for (int m = 0; m < CM_MAX_GROUPINGS; ++m) {
      if (m < M) {
        rows[m][t] = c[m];
#pragma unroll
        for (int v = 0; v < CM_WAVES; ++v) {
          const unsigned long long b = __ballot(c[m] >= 0 && (c[m] & 3) == v);
          if (lane == 0) pairs[m][v][wave] = b;
        }
      }
    }
    __syncthreads();
    if (walks) {
      for (int m = 0; m < M; ++m) {
        for (int src = 0; src < CM_WAVES; ++src) {
          const unsigned long long bits = pairs[m][wave][src];
          unsigned long long todo = ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(bits >> 32)) << 32) |
                                    (unsigned)__builtin_amdgcn_readfirstlane((unsigned)bits);
          if (todo == 0) continue;
          int a = src * 64 + __builtin_ctzll(todo);
          int row = rows[m][a];
          double2 v = yp[a];
          while (todo) {
            todo &= todo - 1;
            const int a_next = todo ? src * 64 + __builtin_ctzll(todo) : a;
            const int row_next = rows[m][a_next];   // in flight during this pair's adds
            const double2 v_next = yp[a_next];
            const int r = __builtin_amdgcn_readfirstlane(row);
            const double d = v.x - v.y;
            const double term[CM_SUMS] = {1.0, d * d, v.x, v.y, v.x * v.x, v.y * v.y, v.x * v.y};
            const bool mine = ((r >> 2) & 63) == lane;
            const int q = r >> 8;
#pragma unroll
            for (int o = 0; o < OWNED; ++o)
              if (q == o) cm_add(acc[o], mine, term);
            a = a_next;
            row = row_next;
            v = v_next;
          }
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < OWNED; ++q) {
    const int row = q * CM_THREADS + lane * 4 + wave;
    if (row < K) {
      double* out = partial + ((int64_t)blockIdx.x * K + row) * CM_SUMS;
#pragma unroll
      for (int j = 0; j < CM_SUMS; ++j) out[j] = acc[q].s[j];
    }
  }
}

__global__ __launch_bounds__(64) void class_moments_final_kernel(int nb, int nkj, const double* __restrict__ partial,
                                                                 int accumulate, double* __restrict__ moments) {
  const int kj = blockIdx.x, lane = threadIdx.x;
  double s = 0.0;
  for (int b = lane; b < nb; b += 64) s += partial[(int64_t)b * nkj + kj];
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if (lane == 0) moments[kj] = accumulate ? moments[kj] + s : s;
}

}  // namespace ng

using namespace ng;

extern "C" int ng_class_moments(ng_ctx* ctx, void* stream, int64_t N, const float* y, const float* w, const int32_t* names,
                                const float* pred, int n_ids, int M, const int32_t* class_of, int K, int accumulate,
                                double* moments) {
  if (!ctx) return NG_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  NG_REQUIRE(ctx, N >= 0 && N < ((int64_t)1 << 31) - 256, "class moments: atom count outside [0, 2^31 - 256)");
  NG_REQUIRE(ctx, M >= 1 && M <= CM_MAX_GROUPINGS, "class moments: 1 to 4 groupings");
  NG_REQUIRE(ctx, K >= 1 && K <= CM_MAX_CLASSES, "class moments: 1 to 1024 classes");
  NG_REQUIRE(ctx, n_ids >= 0 && n_ids <= CM_MAX_IDS, "class moments: class table size outside [0, 2^24]");
  NG_REQUIRE(ctx, accumulate == 0 || accumulate == 1, "class moments: accumulate is 0 or 1");
  NG_REQUIRE(ctx, moments != nullptr, "class moments: no output");
  NG_REQUIRE(ctx, N == 0 || (y && w && names && pred), "class moments: missing input");
  NG_REQUIRE(ctx, n_ids == 0 || class_of, "class moments: missing class table");
  const int nkj = CM_SUMS * K;
  const int64_t n_tiles = cdiv(N, CM_THREADS);
  const int nb = (int)std::min<int64_t>(n_tiles, CM_MAX_BLOCKS);
  double* partial = (double*)workspace(ctx, (size_t)std::max(nb, 1) * nkj * sizeof(double));
  if (!partial) return NG_ERR_NOMEM;
  ProfScope ps(ctx, st, "class_moments");
  if (nb > 0) {
    const dim3 grid((unsigned)nb), block(CM_THREADS);
    switch ((int)cdiv(K, CM_THREADS)) {
      case 1:
        hipLaunchKernelGGL(class_moments_partial_kernel<1>, grid, block, 0, st, N, n_tiles, y, w, names, pred, n_ids, M,
                           class_of, K, partial);
        break;
      case 2:
        hipLaunchKernelGGL(class_moments_partial_kernel<2>, grid, block, 0, st, N, n_tiles, y, w, names, pred, n_ids, M,
                           class_of, K, partial);
        break;
      case 3:
        hipLaunchKernelGGL(class_moments_partial_kernel<3>, grid, block, 0, st, N, n_tiles, y, w, names, pred, n_ids, M,
                           class_of, K, partial);
        break;
      default:
        hipLaunchKernelGGL(class_moments_partial_kernel<CM_MAX_OWNED>, grid, block, 0, st, N, n_tiles, y, w, names, pred,
                           n_ids, M, class_of, K, partial);
        break;
    }
  }
  // nb == 0 (no atoms): the final launch writes zeros (or adds nothing)
  hipLaunchKernelGGL(class_moments_final_kernel, dim3((unsigned)nkj), dim3(64), 0, st, nb, nkj, partial, accumulate, moments);
  NG_HIP(ctx, hipGetLastError());
  return NG_OK;
}
