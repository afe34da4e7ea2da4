// Maximum-entropy reweighting of a trajectory against measured shifts (nmrgnn_amd/reweight.py): the hot path of
// the fit, its weights, and the weighted moments of the CSV.  With S [T][M] float32, y [M] float32, lambda [M] double and the log
// prior logw0 [T] (NULL: uniform, -log T; -inf: a frame of weight zero), all arithmetic in float64, S and y converted first:
//   d_tm = S_tm - y_m,  a_t = logw0_t - sum_m lambda_m d_tm,  logZ = log sum_t exp(a_t),  p_t = exp(a_t - logZ),
//   mean_m = sum_t p_t d_tm.
// It is attention with one query: ONE pass over S with a running maximum.  No atomics; every grid below is a function of (T, M)
// alone (never of the CU count), so every bit of a result is too.
//
// ng_reweight_eval, M <= 2048 ("register form"): a wave owns a contiguous span of frames, a lane 4 * NC columns of the row (NC =
//   ceil(M / 256) rounded up to 1, 2, 4 or 8: the instantiations serve M <= 256, 512, 1024, 2048).  With M % 4 == 0 and a 16-byte
//   aligned S (VEC) lane l holds columns 256 c + 4 l .. + 3 of chunk c and reads them as one 16-byte load, otherwise columns
//   64 j + l as dword loads.  The 4 NC float64 accumulators and two rows stay in registers (the next row is loaded before
//   this one is used); lambda (double) and y sit in LDS, each lane reading its own entries.  Per frame: dot product by a wave butterfly (the same bits in every lane: IEEE addition commutes),
//   then the online log-sum-exp step — when the maximum rises the accumulators and the running sum are scaled by
//   exp(max_old - max_new), which is 0 (not exp(-inf - a)) while max_old is still -inf; a frame with a_t = -inf is skipped, so
//   -inf - -inf never occurs.  The four waves of a workgroup merge through LDS in wave order; partial (max, sum, acc[M]) per
//   workgroup goes to the context's scratch, and a second launch merges the workgroups in their order by the same rule.
// ng_reweight_eval, 2048 < M <= 16384 ("two-pass form"): pass one writes the logits a_t and per-workgroup maxima (max is exact and
//   order-free), pass two knows the global maximum, so it needs no rescale: workgroup (b, cb) adds exp(a_t - max) d_tm over the
//   frames of span b for the 256 columns of block cb (S is read a second time), and the same merge launch finishes.
// A span whose frames are all -inf gives (-inf, 0, 0); a call whose frames all are gives logZ = -inf and mean = 0.  NaN in S, y
// or lambda propagates into logZ and the means; it is not handled.
#include <algorithm>
#include <cmath>

#include "ng_internal.h"

namespace ng {

constexpr int RW_THREADS = 256;
constexpr int RW_WAVES = RW_THREADS / 64;
constexpr int RW_MIN_SPAN = 8;          // frames per wave before the grid grows past one workgroup per 32 frames
constexpr int RW_MAX_BLOCKS = 1024;     // most partials the merge takes; the grid of the weights pass and of M <= 512
constexpr int RW2_MAX_BLOCKS = 256;     // two-pass form: times ceil(M / 256) >= 9 column blocks
constexpr int RW_MAX_REG_M = 2048;
constexpr int RW_MAX_M = 16384;
constexpr int RW_MERGE_COLS = 16, RW_MERGE_GROUPS = 64, RW_MERGE_THREADS = RW_MERGE_COLS * RW_MERGE_GROUPS;
// Workgroups of the register form: one round of workgroups on a 256-CU part at the occupancy the compiler's register count
// gives each instantiation (5+ / 3 / 2 waves per SIMD at 4, 16 and 32 columns per lane), so that no second, half-empty round
// follows.  Constants of (M) alone, not a device query: another part gets the same grid and the same bits.
static inline int rw_reg_blocks(int M) { return M <= 512 ? RW_MAX_BLOCKS : M <= 1024 ? 768 : 512; }
constexpr int WM_COLS = 64, WM_WAVES = 16;

__host__ __device__ __forceinline__ int64_t rw_min(int64_t a, int64_t b) { return a < b ? a : b; }

struct RwGrid {
  int nb;          // workgroups along the frames
  int64_t span;    // frames per wave: wave g = 4 * block + wave owns [g * span, min(T, (g + 1) * span))
};
static inline RwGrid rw_grid(int64_t T, int max_blocks) {
  RwGrid g;
  g.nb = (int)rw_min(cdiv(T, RW_WAVES * RW_MIN_SPAN), max_blocks);
  g.span = cdiv(T, (int64_t)g.nb * RW_WAVES);
  return g;
}

__device__ __forceinline__ double rw_neg_inf() { return -__builtin_huge_val(); }

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}

// exp(from - to) for from <= to, 0 when from is -inf (also when both are)
__device__ __forceinline__ double rw_rescale(double from, double to) { return from == rw_neg_inf() ? 0.0 : exp(from - to); }

template <int NC, bool VEC>
__device__ __forceinline__ int rw_col(int j, int lane) {
  return VEC ? (j >> 2) * 256 + lane * 4 + (j & 3) : j * 64 + lane;
}

// One row into registers.  Every load is issued (columns past M read a clamped address and are zeroed by a select): a branch
// around a load would make the compiler wait for each load on its own.
template <int NC, bool VEC>
__device__ __forceinline__ void rw_load_row(const float* __restrict__ row, int M, int lane, float (&v)[4 * NC]) {
  if constexpr (VEC) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int col = c * 256 + lane * 4;
      const bool ok = col < M;
      const float4 q = *reinterpret_cast<const float4*>(row + (ok ? col : M - 4));
      v[4 * c + 0] = ok ? q.x : 0.f;
      v[4 * c + 1] = ok ? q.y : 0.f;
      v[4 * c + 2] = ok ? q.z : 0.f;
      v[4 * c + 3] = ok ? q.w : 0.f;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4 * NC; ++j) {
      const int col = j * 64 + lane;
      const bool ok = col < M;
      const float q = row[ok ? col : M - 1];
      v[j] = ok ? q : 0.f;
    }
  }
}

// A compiler-only fence: the LDS reads of lambda and y stay where they are written, four columns at a time, instead of being
// hoisted out of the frame loop (3 registers per column) or gathered at its top
#define RW_LDS_FENCE() asm volatile("" ::: "memory")

// partial layout: ms [nb][2] = (max, sum), then acc [nb][M]
template <int NC, bool VEC>
__global__ __launch_bounds__(RW_THREADS) void reweight_partial_kernel(int64_t T, int M, int64_t span,
                                                                      const float* __restrict__ S, const float* __restrict__ y,
                                                                      const double* __restrict__ logw0,
                                                                      const double* __restrict__ lambda, int nb,
                                                                      double* __restrict__ partial) {
  constexpr int NV = 4 * NC;
  // lambda and y sit in LDS during the loop (entry j * 64 + lane: a lane reads its own, no bank conflict), which keeps the
  // registers for the accumulators and two rows; the same bytes are the merge slabs afterwards
  __shared__ double sm[(RW_WAVES - 1) * NC * 256];
  __shared__ double ms[RW_WAVES][2];
  double* lam_s = sm;
  float* y_s = reinterpret_cast<float*>(sm + NC * 256);
  double(*slab)[NC * 256] = reinterpret_cast<double(*)[NC * 256]>(sm);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int e = threadIdx.x; e < NC * 256; e += RW_THREADS) {
    const int col = rw_col<NC, VEC>(e >> 6, e & 63);
    const bool ok = col < M;
    lam_s[e] = ok ? lambda[col] : 0.0;
    y_s[e] = ok ? y[col] : 0.f;
  }
  __syncthreads();
  double acc[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) acc[j] = 0.0;
  const int64_t g = (int64_t)blockIdx.x * RW_WAVES + wave;
  const int64_t t0 = rw_min(g * span, T), t1 = rw_min(t0 + span, T);
  const double lw_uniform = -log((double)T);
  double m = rw_neg_inf(), s = 0.0;
  float cur[NV], nxt[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) nxt[j] = 0.f;
  if (t0 < t1) rw_load_row<NC, VEC>(S + t0 * M, M, lane, cur);
  for (int64_t t = t0; t < t1; ++t) {
    if (t + 1 < t1) rw_load_row<NC, VEC>(S + (t + 1) * M, M, lane, nxt);
    const double lw = logw0 ? logw0[t] : lw_uniform;
    double dot = 0.0;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      if ((j & 3) == 0) RW_LDS_FENCE();
      dot = fma(lam_s[j * 64 + lane], (double)cur[j] - (double)y_s[j * 64 + lane], dot);
    }
    const double a = lw - wave_sum_f64(dot);      // the same bits in every lane
#pragma unroll
    for (int j = 0; j < NV; ++j) asm volatile("" : "+v"(cur[j]));      // d is formed again below, not kept in 2 * NV registers
    if (a > m) {                                  // the maximum rises (a is finite or +inf)
      const double r = rw_rescale(m, a);
      s = s * r + 1.0;
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        if ((j & 3) == 0) RW_LDS_FENCE();
        acc[j] = fma(acc[j], r, (double)cur[j] - (double)y_s[j * 64 + lane]);
      }
      m = a;
    } else if (!(a == rw_neg_inf())) {            // a frame of weight zero adds nothing; NaN goes on
      const double w = exp(a - m);
      s += w;
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        if ((j & 3) == 0) RW_LDS_FENCE();
        acc[j] = fma(w, (double)cur[j] - (double)y_s[j * 64 + lane], acc[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < NV; ++j) cur[j] = nxt[j];
  }
  __syncthreads();      // every wave is done with lambda and y: their bytes become the slabs
  // the four waves in wave order, by the log-sum-exp rule
  if (lane == 0) {
    ms[wave][0] = m;
    ms[wave][1] = s;
  }
  __syncthreads();
  double mw = ms[0][0];
#pragma unroll
  for (int w = 1; w < RW_WAVES; ++w) mw = fmax(mw, ms[w][0]);
  const double r = rw_rescale(m, mw);
  if (wave > 0) {
#pragma unroll
    for (int j = 0; j < NV; ++j) slab[wave - 1][j * 64 + lane] = acc[j] * r;
  }
  __syncthreads();
  if (wave == 0) {
    double sw = 0.0;
#pragma unroll
    for (int w = 0; w < RW_WAVES; ++w) sw += ms[w][1] * rw_rescale(ms[w][0], mw);
    if (lane == 0) {
      partial[2 * (int64_t)blockIdx.x] = mw;
      partial[2 * (int64_t)blockIdx.x + 1] = sw;
    }
    double* out = partial + 2 * (int64_t)nb + (int64_t)blockIdx.x * M;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      double v = acc[j] * r;
#pragma unroll
      for (int w = 0; w < RW_WAVES - 1; ++w) v += slab[w][j * 64 + lane];
      const int col = rw_col<NC, VEC>(j, lane);
      if (col < M) out[col] = v;
    }
  }
}

// out = {logZ, mean[M]} from nb partials, in their order.  Workgroup x owns 16 columns; its 64 thread groups take the partials
// b = group, group + 64, ... (all of a thread's loads are in flight together: the launch is a few memory round trips) and are
// added in group order.
__global__ __launch_bounds__(RW_MERGE_THREADS) void reweight_merge_kernel(int nb, int M, const double* __restrict__ partial,
                                                                          double* __restrict__ out) {
  __shared__ double scale[RW_MAX_BLOCKS];
  __shared__ double red[RW_MERGE_THREADS];
  const int tid = threadIdx.x;
  const double* acc = partial + 2 * (int64_t)nb;
  double gm = rw_neg_inf();
  for (int b = tid; b < nb; b += RW_MERGE_THREADS) gm = fmax(gm, partial[2 * b]);
  red[tid] = gm;
  __syncthreads();
  for (int o = RW_MERGE_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] = fmax(red[tid], red[tid + o]);
    __syncthreads();
  }
  gm = red[0];
  __syncthreads();
  double z = 0.0;
  for (int b = tid; b < nb; b += RW_MERGE_THREADS) {
    const double sc = rw_rescale(partial[2 * b], gm);
    scale[b] = sc;
    z += partial[2 * b + 1] * sc;
  }
  red[tid] = z;
  __syncthreads();
  for (int o = RW_MERGE_THREADS / 2; o > 0; o >>= 1) {      // a fixed tree
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  const double Z = red[0];
  __syncthreads();
  const int c = tid & (RW_MERGE_COLS - 1), grp = tid / RW_MERGE_COLS;
  const int col = blockIdx.x * RW_MERGE_COLS + c;
  double a = 0.0;
  if (col < M) {
    const double* p = acc + col;
    int b = grp;
    for (; b + 3 * RW_MERGE_GROUPS < nb; b += 4 * RW_MERGE_GROUPS) {      // four loads in flight, added in b order
      double v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = p[(int64_t)(b + u * RW_MERGE_GROUPS) * M];
#pragma unroll
      for (int u = 0; u < 4; ++u) a = fma(v[u], scale[b + u * RW_MERGE_GROUPS], a);
    }
    for (; b < nb; b += RW_MERGE_GROUPS) a = fma(p[(int64_t)b * M], scale[b], a);
  }
  red[tid] = a;
  __syncthreads();
  if (tid < RW_MERGE_COLS && col < M) {
    double v = red[tid];
    for (int k = 1; k < RW_MERGE_GROUPS; ++k) v += red[k * RW_MERGE_COLS + tid];
    out[1 + col] = gm == rw_neg_inf() ? 0.0 : v / Z;
  }
  if (blockIdx.x == 0 && tid == 0) out[0] = gm == rw_neg_inf() ? gm : gm + log(Z);
}

// sum_m lambda_m (S_tm - y_m) of one row, the columns strided over the lanes (any M); the same bits in every lane
template <bool VEC>
__device__ __forceinline__ double rw_row_dot(const float* __restrict__ row, int M, const float* __restrict__ y,
                                             const double* __restrict__ lambda, int lane) {
  double dot = 0.0;
  if constexpr (VEC) {
    for (int col = lane * 4; col < M; col += 256) {
      const float4 q = *reinterpret_cast<const float4*>(row + col);
      dot = fma(lambda[col], (double)q.x - (double)y[col], dot);
      dot = fma(lambda[col + 1], (double)q.y - (double)y[col + 1], dot);
      dot = fma(lambda[col + 2], (double)q.z - (double)y[col + 2], dot);
      dot = fma(lambda[col + 3], (double)q.w - (double)y[col + 3], dot);
    }
  } else {
    for (int col = lane; col < M; col += 64) dot = fma(lambda[col], (double)row[col] - (double)y[col], dot);
  }
  return wave_sum_f64(dot);
}

// two-pass form, pass one: logits [T] and the maximum of every workgroup's frames
template <bool VEC>
__global__ __launch_bounds__(RW_THREADS) void reweight_logits_kernel(int64_t T, int M, int64_t span, const float* __restrict__ S,
                                                                     const float* __restrict__ y,
                                                                     const double* __restrict__ logw0,
                                                                     const double* __restrict__ lambda,
                                                                     double* __restrict__ logits, double* __restrict__ blockmax) {
  __shared__ double mx[RW_WAVES];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t g = (int64_t)blockIdx.x * RW_WAVES + wave;
  const int64_t t0 = rw_min(g * span, T), t1 = rw_min(t0 + span, T);
  const double lw_uniform = -log((double)T);
  double m = rw_neg_inf();
  for (int64_t t = t0; t < t1; ++t) {
    const double a = (logw0 ? logw0[t] : lw_uniform) - rw_row_dot<VEC>(S + t * M, M, y, lambda, lane);
    if (lane == 0) logits[t] = a;
    m = fmax(m, a);
  }
  if (lane == 0) mx[wave] = m;
  __syncthreads();
  if (threadIdx.x == 0) blockmax[blockIdx.x] = fmax(fmax(mx[0], mx[1]), fmax(mx[2], mx[3]));
}

// two-pass form, pass two: workgroup (b, cb) adds exp(a_t - max) d_tm over its frames for the columns [256 cb, 256 cb + 256)
template <bool VEC>
__global__ __launch_bounds__(RW_THREADS) void reweight_columns_kernel(int64_t T, int M, int64_t span, const float* __restrict__ S,
                                                                      const float* __restrict__ y,
                                                                      const double* __restrict__ logits,
                                                                      const double* __restrict__ blockmax, int nb,
                                                                      double* __restrict__ partial) {
  __shared__ double slab[RW_WAVES - 1][256];
  __shared__ double red[RW_THREADS];
  __shared__ double sw[RW_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  red[tid] = tid < nb ? blockmax[tid] : rw_neg_inf();      // nb <= RW2_MAX_BLOCKS = the workgroup size
  __syncthreads();
  for (int o = RW_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] = fmax(red[tid], red[tid + o]);
    __syncthreads();
  }
  const double gm = red[0];
  const int cb = blockIdx.y;
  int col[4];
  bool ok[4];
  double yd[4], acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    col[k] = cb * 256 + (VEC ? lane * 4 + k : k * 64 + lane);
    ok[k] = col[k] < M;
    yd[k] = ok[k] ? (double)y[col[k]] : 0.0;
    if (!ok[k]) col[k] = VEC ? M - 4 + k : M - 1;      // a clamped address, zeroed by a select
  }
  const int64_t g = (int64_t)blockIdx.x * RW_WAVES + wave;
  const int64_t t0 = rw_min(g * span, T), t1 = rw_min(t0 + span, T);
  double s = 0.0;
  for (int64_t tb = t0; tb < t1; tb += 64) {
    const int cnt = (int)rw_min(64, t1 - tb);
    double wv = 0.0;
    if (lane < cnt) {
      const double a = logits[tb + lane];
      wv = a == rw_neg_inf() ? 0.0 : exp(a - gm);
    }
    for (int i = 0; i < cnt; ++i) {
      const double w = __shfl(wv, i, 64);
      const float* row = S + (tb + i) * M;
      float q[4];
      if constexpr (VEC) {
        const float4 f = *reinterpret_cast<const float4*>(row + col[0]);
        q[0] = f.x; q[1] = f.y; q[2] = f.z; q[3] = f.w;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = row[col[k]];
      }
      s += w;
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[k] = fma(w, ok[k] ? (double)q[k] - yd[k] : 0.0, acc[k]);
    }
  }
  if (lane == 0) sw[wave] = s;
  if (wave > 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) slab[wave - 1][k * 64 + lane] = acc[k];
  }
  __syncthreads();
  if (wave == 0) {
    if (cb == 0 && lane == 0) {
      partial[2 * (int64_t)blockIdx.x] = gm;
      partial[2 * (int64_t)blockIdx.x + 1] = ((sw[0] + sw[1]) + sw[2]) + sw[3];
    }
    double* out = partial + 2 * (int64_t)nb + (int64_t)blockIdx.x * M;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      double v = acc[k];
#pragma unroll
      for (int w = 0; w < RW_WAVES - 1; ++w) v += slab[w][k * 64 + lane];
      if (ok[k]) out[col[k]] = v;
    }
  }
}

// p_t = exp(a_t - logZ) and the per-workgroup sums {sum p log(p / w0), sum p^2}: frames in order inside a wave, waves in order
template <bool VEC>
__global__ __launch_bounds__(RW_THREADS) void reweight_weights_kernel(int64_t T, int M, int64_t span, const float* __restrict__ S,
                                                                      const float* __restrict__ y,
                                                                      const double* __restrict__ logw0,
                                                                      const double* __restrict__ lambda,
                                                                      const double* __restrict__ logZ_p, double* __restrict__ p,
                                                                      double* __restrict__ partial) {
  __shared__ double st[RW_WAVES][2];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t g = (int64_t)blockIdx.x * RW_WAVES + wave;
  const int64_t t0 = rw_min(g * span, T), t1 = rw_min(t0 + span, T);
  const double lw_uniform = -log((double)T), logZ = *logZ_p;
  double e1 = 0.0, e2 = 0.0;
  for (int64_t t = t0; t < t1; ++t) {
    const double dot = rw_row_dot<VEC>(S + t * M, M, y, lambda, lane);
    const double a = (logw0 ? logw0[t] : lw_uniform) - dot;
    const double pt = a == rw_neg_inf() ? 0.0 : exp(a - logZ);
    if (lane == 0) p[t] = pt;
    e1 += pt == 0.0 ? 0.0 : pt * (-dot - logZ);      // log(p / w0) = a - logZ - logw0; a frame with p = 0 adds 0
    e2 += pt * pt;
  }
  if (lane == 0) {
    st[wave][0] = e1;
    st[wave][1] = e2;
  }
  __syncthreads();
  if (threadIdx.x < 2)
    partial[2 * (int64_t)blockIdx.x + threadIdx.x] = ((st[0][threadIdx.x] + st[1][threadIdx.x]) + st[2][threadIdx.x]) + st[3][threadIdx.x];
}

__global__ __launch_bounds__(RW_THREADS) void reweight_stats_kernel(int nb, const double* __restrict__ partial,
                                                                    double* __restrict__ stats) {
  __shared__ double red[2][RW_THREADS];
  const int tid = threadIdx.x;
  double e1 = 0.0, e2 = 0.0;
  for (int b = tid; b < nb; b += RW_THREADS) {
    e1 += partial[2 * b];
    e2 += partial[2 * b + 1];
  }
  red[0][tid] = e1;
  red[1][tid] = e2;
  __syncthreads();
  for (int o = RW_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) {
      red[0][tid] += red[0][tid + o];
      red[1][tid] += red[1][tid + o];
    }
    __syncthreads();
  }
  if (tid < 2) stats[tid] = red[tid][0];
}

// Weighted moments over frames: a workgroup owns 64 columns, its 16 waves the contiguous frame chunks [w c, (w + 1) c) with
// c = ceil(T / 16); frames in order inside a chunk, chunks added in wave order.  e_t = mu_t - mu_0 is exact in float64.
__global__ __launch_bounds__(WM_COLS * WM_WAVES) void weighted_moments_kernel(int64_t T, int64_t N, const float* __restrict__ mu,
                                                                              const double* __restrict__ p,
                                                                              float* __restrict__ mean, float* __restrict__ var) {
  __shared__ double red[2][WM_WAVES][WM_COLS];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t i = (int64_t)blockIdx.x * WM_COLS + lane;
  const bool ok = i < N;
  const int64_t ic = ok ? i : N - 1;
  const int64_t chunk = (T + WM_WAVES - 1) / WM_WAVES;
  const int64_t t0 = rw_min(wave * chunk, T), t1 = rw_min(t0 + chunk, T);
  const double m0 = (double)mu[ic];
  double se = 0.0, se2 = 0.0;
  int64_t t = t0;
  for (; t + 4 <= t1; t += 4) {      // four loads in flight, added in frame order
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = mu[(t + u) * N + ic];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const double e = (double)v[u] - m0, w = p[t + u];
      se = fma(w, e, se);
      se2 = fma(w * e, e, se2);
    }
  }
  for (; t < t1; ++t) {
    const double e = (double)mu[t * N + ic] - m0, w = p[t];
    se = fma(w, e, se);
    se2 = fma(w * e, e, se2);
  }
  red[0][wave][lane] = se;
  red[1][wave][lane] = se2;
  __syncthreads();
  if (wave == 0 && ok) {
    double a = red[0][0][lane], b = red[1][0][lane];
#pragma unroll
    for (int w = 1; w < WM_WAVES; ++w) {
      a += red[0][w][lane];
      b += red[1][w][lane];
    }
    double v = b - a * a;
    if (v < 0.0) v = 0.0;      // the difference can round below 0; NaN stays NaN
    mean[i] = (float)(m0 + a);
    var[i] = (float)v;
  }
}

static int rw_check(ng_ctx* ctx, int64_t T, int M, const void* S, const void* y, const void* lambda) {
  NG_REQUIRE(ctx, T >= 1 && T < ((int64_t)1 << 31), "reweight: frame count outside [1, 2^31)");
  NG_REQUIRE(ctx, M >= 1 && M <= RW_MAX_M, "reweight: 1 to 16384 observables");
  NG_REQUIRE(ctx, S && y && lambda, "reweight: S, y and lambda required");
  return NG_OK;
}

static inline bool rw_vec(int M, const float* S) { return (M & 3) == 0 && ((uintptr_t)S & 15) == 0; }

template <int NC>
static void rw_launch_partial(hipStream_t st, bool vec, const RwGrid& g, int64_t T, int M, const float* S, const float* y,
                              const double* logw0, const double* lambda, double* partial) {
  if (vec)
    hipLaunchKernelGGL((reweight_partial_kernel<NC, true>), dim3((unsigned)g.nb), dim3(RW_THREADS), 0, st, T, M, g.span, S, y,
                       logw0, lambda, g.nb, partial);
  else
    hipLaunchKernelGGL((reweight_partial_kernel<NC, false>), dim3((unsigned)g.nb), dim3(RW_THREADS), 0, st, T, M, g.span, S, y,
                       logw0, lambda, g.nb, partial);
}

}  // namespace ng

using namespace ng;

extern "C" int ng_reweight_eval(ng_ctx* ctx, void* stream, int64_t T, int M, const float* S, const float* y, const double* logw0,
                                const double* lambda, double* out) {
  if (!ctx) return NG_ERR_INVALID;
  if (int rc = rw_check(ctx, T, M, S, y, lambda)) return rc;
  NG_REQUIRE(ctx, out != nullptr, "reweight_eval: no output");
  hipStream_t st = (hipStream_t)stream;
  const bool vec = rw_vec(M, S);
  const bool two_pass = M > RW_MAX_REG_M;
  const RwGrid g = rw_grid(T, two_pass ? RW2_MAX_BLOCKS : rw_reg_blocks(M));
  const size_t n_partial = (size_t)g.nb * (2 + (size_t)M);
  const size_t doubles = n_partial + (two_pass ? (size_t)T + (size_t)g.nb : 0);
  double* partial = (double*)workspace(ctx, doubles * sizeof(double));
  if (!partial) return NG_ERR_NOMEM;
  ProfScope ps(ctx, st, "reweight_eval");
  if (!two_pass) {
    if (M <= 256) rw_launch_partial<1>(st, vec, g, T, M, S, y, logw0, lambda, partial);
    else if (M <= 512) rw_launch_partial<2>(st, vec, g, T, M, S, y, logw0, lambda, partial);
    else if (M <= 1024) rw_launch_partial<4>(st, vec, g, T, M, S, y, logw0, lambda, partial);
    else rw_launch_partial<8>(st, vec, g, T, M, S, y, logw0, lambda, partial);
  } else {
    double* logits = partial + n_partial;
    double* blockmax = logits + T;
    const dim3 grid2((unsigned)g.nb, (unsigned)cdiv(M, 256));
    if (vec) {
      hipLaunchKernelGGL(reweight_logits_kernel<true>, dim3((unsigned)g.nb), dim3(RW_THREADS), 0, st, T, M, g.span, S, y, logw0,
                         lambda, logits, blockmax);
      hipLaunchKernelGGL(reweight_columns_kernel<true>, grid2, dim3(RW_THREADS), 0, st, T, M, g.span, S, y, logits, blockmax,
                         g.nb, partial);
    } else {
      hipLaunchKernelGGL(reweight_logits_kernel<false>, dim3((unsigned)g.nb), dim3(RW_THREADS), 0, st, T, M, g.span, S, y, logw0,
                         lambda, logits, blockmax);
      hipLaunchKernelGGL(reweight_columns_kernel<false>, grid2, dim3(RW_THREADS), 0, st, T, M, g.span, S, y, logits, blockmax,
                         g.nb, partial);
    }
  }
  hipLaunchKernelGGL(reweight_merge_kernel, dim3((unsigned)cdiv(M, RW_MERGE_COLS)), dim3(RW_MERGE_THREADS), 0, st, g.nb, M,
                     partial, out);
  NG_HIP(ctx, hipGetLastError());
  return NG_OK;
}

extern "C" int ng_reweight_weights(ng_ctx* ctx, void* stream, int64_t T, int M, const float* S, const float* y,
                                   const double* logw0, const double* lambda, const double* logZ, double* p, double* stats) {
  if (!ctx) return NG_ERR_INVALID;
  if (int rc = rw_check(ctx, T, M, S, y, lambda)) return rc;
  NG_REQUIRE(ctx, logZ && p && stats, "reweight_weights: logZ, p and stats required");
  hipStream_t st = (hipStream_t)stream;
  const RwGrid g = rw_grid(T, RW_MAX_BLOCKS);
  double* partial = (double*)workspace(ctx, (size_t)g.nb * 2 * sizeof(double));
  if (!partial) return NG_ERR_NOMEM;
  ProfScope ps(ctx, st, "reweight_weights");
  if (rw_vec(M, S))
    hipLaunchKernelGGL(reweight_weights_kernel<true>, dim3((unsigned)g.nb), dim3(RW_THREADS), 0, st, T, M, g.span, S, y, logw0,
                       lambda, logZ, p, partial);
  else
    hipLaunchKernelGGL(reweight_weights_kernel<false>, dim3((unsigned)g.nb), dim3(RW_THREADS), 0, st, T, M, g.span, S, y, logw0,
                       lambda, logZ, p, partial);
  hipLaunchKernelGGL(reweight_stats_kernel, dim3(1), dim3(RW_THREADS), 0, st, g.nb, partial, stats);
  NG_HIP(ctx, hipGetLastError());
  return NG_OK;
}

extern "C" int ng_weighted_moments(ng_ctx* ctx, void* stream, int64_t T, int64_t N, const float* mu, const double* p, float* mean,
                                   float* var) {
  if (!ctx) return NG_ERR_INVALID;
  NG_REQUIRE(ctx, T >= 1 && T < ((int64_t)1 << 31), "weighted_moments: frame count outside [1, 2^31)");
  NG_REQUIRE(ctx, N >= 0 && N < ((int64_t)1 << 31), "weighted_moments: atom count outside [0, 2^31)");
  NG_REQUIRE(ctx, mu && p && mean && var, "weighted_moments: mu, p, mean and var required");
  if (N == 0) return NG_OK;
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(ctx, st, "weighted_moments");
  hipLaunchKernelGGL(weighted_moments_kernel, dim3((unsigned)cdiv(N, WM_COLS)), dim3(WM_COLS * WM_WAVES), 0, st, T, N, mu, p,
                     mean, var);
  NG_HIP(ctx, hipGetLastError());
  return NG_OK;
}
