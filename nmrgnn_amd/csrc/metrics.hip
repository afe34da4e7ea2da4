// Per-name shift metrics (nmrgnn/metrics.py:22-116: NameRMSD, NameCount, NameCorr) as one device reduction.
//
// Per atom i and class k the reference's mask is m_ik = w_i * [name_i in label_idx_k] (metrics.py:38-39).  Every metric is
// a function of seven weighted sums per class:
//   {S0 = sum m, Sd2 = sum m (y - p)^2, Sy = sum m y, Sp = sum m p, Syy = sum m y^2, Spp = sum m p^2, Syp = sum m y p}
// so up to 32 classes are evaluated in ONE pass over the atoms: a uint32 membership table maps a name id to the bit set of
// the classes that contain it.  The sums are kept in float64 (the xm2 - xm^2 of shifts near 120 ppm would cancel most of
// the digits of fp32 moments) and are bitwise deterministic: no atomics, per-workgroup partials in a fixed tile order, then
// a second launch that sums the partials in a fixed order.
//
//   stage 1  workgroup b takes atom tiles b, b + nb, ...; per tile the 256 threads first write the tile's seven per-atom
//            terms (w-weighted, not yet masked) and the class bits to LDS; then thread t = g * 7K + kj (class k = kj / 7,
//            sum j = kj % 7, atom group g < 256 / 7K) adds the terms of atoms g, g + groups, ... whose bit k is set.
//            The groups are summed in order into partial[b][kj].
//   stage 2  one wave per kj sums partial[0..nb)[kj] (lane-strided, then a butterfly) and writes or adds moments[kj].
#include <algorithm>

#include "ng_internal.h"

namespace ng {

constexpr int NM_THREADS = 256;     // = atoms per tile
constexpr int NM_MAX_BLOCKS = 256;  // stage-1 workgroups: one per CU; the pass is launch-latency bound, not bandwidth bound
constexpr int NM_SUMS = 7;
constexpr int NM_MAX_CLASSES = 32;

__global__ __launch_bounds__(NM_THREADS) void name_metrics_partial_kernel(
    int64_t N, int64_t n_tiles, const float* __restrict__ y, const float* __restrict__ w, const int32_t* __restrict__ names,
    const float* __restrict__ pred, int n_names, const uint32_t* __restrict__ member, int K, double* __restrict__ partial) {
  __shared__ double terms[NM_SUMS][NM_THREADS];
  __shared__ uint32_t bits[NM_THREADS];
  __shared__ double red[NM_THREADS];
  const int t = threadIdx.x;
  const int nkj = NM_SUMS * K;
  const int groups = NM_THREADS / nkj;   // >= 1 for K <= 32 (7 * 32 = 224)
  const int g = t / nkj, kj = t - g * nkj;
  const int k = kj / NM_SUMS, j = kj - k * NM_SUMS;
  double acc = 0.0;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t i = tile * NM_THREADS + t;
    uint32_t b = 0;
    double m = 0.0, yd = 0.0, pd = 0.0;
    if (i < N) {
      const int32_t nm = names[i];
      b = (nm >= 0 && nm < n_names) ? member[nm] : 0u;   // ids outside the table (and negative ones) belong to no class
      m = (double)w[i];
      yd = (double)y[i];
      pd = (double)pred[i];
    }
    const double d = yd - pd;
    bits[t] = b;
    terms[0][t] = m;
    terms[1][t] = m * (d * d);
    terms[2][t] = m * yd;
    terms[3][t] = m * pd;
    terms[4][t] = m * (yd * yd);
    terms[5][t] = m * (pd * pd);
    terms[6][t] = m * (yd * pd);
    __syncthreads();
    if (g < groups) {
      for (int a = g; a < NM_THREADS; a += groups) acc += ((bits[a] >> k) & 1u) ? terms[j][a] : 0.0;
    }
    __syncthreads();
  }
  red[t] = acc;
  __syncthreads();
  if (t < nkj) {
    double s = 0.0;
    for (int q = 0; q < groups; ++q) s += red[q * nkj + t];
    partial[(int64_t)blockIdx.x * nkj + t] = s;
  }
}

__global__ __launch_bounds__(64) void name_metrics_final_kernel(int nb, int nkj, const double* __restrict__ partial,
                                                                int accumulate, double* __restrict__ moments) {
  const int kj = blockIdx.x, lane = threadIdx.x;
  double s = 0.0;
  for (int b = lane; b < nb; b += 64) s += partial[(int64_t)b * nkj + kj];
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if (lane == 0) moments[kj] = accumulate ? moments[kj] + s : s;
}

}  // namespace ng

using namespace ng;

extern "C" int ng_name_metrics(ng_ctx* ctx, void* stream, int64_t N, const float* y, const float* w, const int32_t* names,
                               const float* pred, int n_names, const uint32_t* member, int K, int accumulate,
                               double* moments) {
  if (!ctx) return NG_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  NG_REQUIRE(ctx, N >= 0, "name metrics: negative atom count");
  NG_REQUIRE(ctx, K >= 1 && K <= NM_MAX_CLASSES, "name metrics: 1 to 32 classes");
  NG_REQUIRE(ctx, n_names >= 0, "name metrics: negative membership table size");
  NG_REQUIRE(ctx, accumulate == 0 || accumulate == 1, "name metrics: accumulate is 0 or 1");
  NG_REQUIRE(ctx, moments != nullptr, "name metrics: no output");
  NG_REQUIRE(ctx, N == 0 || (y && w && names && pred), "name metrics: missing input");
  NG_REQUIRE(ctx, N == 0 || n_names == 0 || member, "name metrics: missing membership table");
  const int nkj = NM_SUMS * K;
  const int64_t n_tiles = cdiv(N, NM_THREADS);
  const int nb = (int)std::min<int64_t>(n_tiles, NM_MAX_BLOCKS);
  double* partial = (double*)workspace(ctx, (size_t)std::max(nb, 1) * nkj * sizeof(double));
  if (!partial) return NG_ERR_NOMEM;
  ProfScope ps(ctx, st, "name_metrics");
  if (nb > 0)
    hipLaunchKernelGGL(name_metrics_partial_kernel, dim3((unsigned)nb), dim3(NM_THREADS), 0, st, N, n_tiles, y, w, names,
                       pred, n_names, member, K, partial);
  // nb == 0 (no atoms): the final launch writes zeros (or adds nothing)
  hipLaunchKernelGGL(name_metrics_final_kernel, dim3((unsigned)nkj), dim3(64), 0, st, nb, nkj, partial, accumulate, moments);
  NG_HIP(ctx, hipGetLastError());
  return NG_OK;
}
