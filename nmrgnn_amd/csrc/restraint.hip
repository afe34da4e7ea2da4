// Replica-averaged chemical-shift restraint: energy and its gradient with respect to the predicted shifts of R replicas.
//
//   mean_i      = (sum_r peaks[r*n + i]) / R           float32, replicas summed in order r = 0, 1, .. (R = 1: peaks[i])
//   E           = sum_i w_i (mean_i - y_i)^2           float32 terms (diff * diff * w), summed in float64
//   dpeaks[r,i] = w_i * (2 * (mean_i - y_i)) / R       the same value for every replica (R = 1: the bits of w * (2 * diff))
//
// Two launches, no atomics, bitwise deterministic (a store pass plus a fixed-order sum pass):
//   stage 1  one thread per atom: the replica mean, every replica's dpeaks, and the atom's term; the workgroup's terms are
//            summed by a fixed LDS tree in float64 into partial[workgroup]
//   stage 2  one workgroup: thread t sums partial[t], partial[t + 256], .. in order, then the same tree -> energy[0]
// Both stay parallel for a few hundred thousand atoms (stage 1: n / 256 workgroups; stage 2: ~n / 65536 terms per thread).
//
// ng_restraint_loss_ex: the same two stages for the restraint forms — replica weights, one energy per replica, a flat-bottom
// tolerance and a running (time) average kept on the device (the definitions are in include/nmrgnn_hip.h).
#include <algorithm>

#include "ng_common.h"

namespace ng {

constexpr int RS_ROWS = 256;

__device__ __forceinline__ double rs_tree(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int off = RS_ROWS / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(RS_ROWS) void restraint_atoms_kernel(int R, int64_t n, const float* __restrict__ peaks,
                                                                  const float* __restrict__ y, const float* __restrict__ w,
                                                                  float* __restrict__ dpeaks, double* __restrict__ partial) {
  __shared__ double red[RS_ROWS];
  const int64_t i = (int64_t)blockIdx.x * RS_ROWS + threadIdx.x;
  double term = 0.0;
  if (i < n) {
    float s = peaks[i];
    for (int r = 1; r < R; ++r) s += peaks[(int64_t)r * n + i];
    const float mean = s / (float)R;
    const float diff = mean - y[i];
    const float wi = w[i];
    const float t = diff * diff;
    term = (double)(t * wi);
    const float g = (wi * (2.0f * diff)) / (float)R;
    for (int r = 0; r < R; ++r) dpeaks[(int64_t)r * n + i] = g;
  }
  const double sum = rs_tree(term, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

__global__ __launch_bounds__(RS_ROWS) void restraint_sum_kernel(int64_t nparts, const double* __restrict__ partial,
                                                                double* __restrict__ energy) {
  __shared__ double red[RS_ROWS];
  double s = 0.0;
  for (int64_t p = threadIdx.x; p < nparts; p += RS_ROWS) s += partial[p];
  const double sum = rs_tree(s, red);
  if (threadIdx.x == 0) energy[0] = sum;
}

// ng_restraint_loss_ex (the arithmetic is stated in include/nmrgnn_hip.h).  Stage 1 runs G * nblk workgroups, group g =
// blockIdx.x / nblk (G = 1 in ensemble mode, R in independent mode); partial[g * nblk + b].  No fused multiply-add anywhere:
// every product and sum is rounded to float32 on its own, so a NumPy restatement gives the same bits.
__global__ __launch_bounds__(RS_ROWS) void restraint_ex_atoms_kernel(int R, int64_t n, int64_t nblk, int indep,
                                                                     const float* __restrict__ peaks, const float* __restrict__ y,
                                                                     const float* __restrict__ w, const float* __restrict__ c,
                                                                     const float* __restrict__ tol, float lambda,
                                                                     float* __restrict__ avg, const int32_t* __restrict__ primed,
                                                                     float* __restrict__ dpeaks, double* __restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ double red[RS_ROWS];
  const int64_t g = (int64_t)blockIdx.x / nblk;
  const int64_t i = ((int64_t)blockIdx.x - g * nblk) * RS_ROWS + threadIdx.x;
  double term = 0.0;
  if (i < n) {
    float m;
    if (indep) {
      m = peaks[g * n + i];
    } else if (c) {
      m = c[0] * peaks[i];
      for (int r = 1; r < R; ++r) m = m + c[r] * peaks[(int64_t)r * n + i];
    } else {
      float s = peaks[i];
      for (int r = 1; r < R; ++r) s += peaks[(int64_t)r * n + i];
      m = s / (float)R;
    }
    float a = m, da = 1.0f;                 // da = d a / d m for this call
    if (lambda > 0.0f) {
      const int64_t k = g * n + i;
      if (primed[0] != 0) {
        da = 1.0f - lambda;
        a = lambda * avg[k] + da * m;
      }
      avg[k] = a;
    }
    const float d = a - y[i];
    const float wi = w[i];
    float e = fabsf(d);
    if (tol) {
      const float x = e - tol[i];
      e = x < 0.0f ? 0.0f : x;              // not fmaxf: a NaN stays a NaN
    }
    term = (double)((e * e) * wi);
    float gr = wi * (2.0f * copysignf(e, d));   // tol NULL or 0: copysign(|d|, d) = d, the bits of w * (2 * d)
    if (da != 1.0f) gr = gr * da;
    if (indep) {
      dpeaks[g * n + i] = gr;
    } else if (c) {
      for (int r = 0; r < R; ++r) dpeaks[(int64_t)r * n + i] = gr * c[r];
    } else {
      const float q = gr / (float)R;
      for (int r = 0; r < R; ++r) dpeaks[(int64_t)r * n + i] = q;
    }
  }
  const double sum = rs_tree(term, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

// one workgroup per group: energy[g] = the fixed-order sum of partial[g * nblk ..]; then primed[0] = 1 (every stage-1
// workgroup has read the old flag by now: same stream, earlier launch)
__global__ __launch_bounds__(RS_ROWS) void restraint_ex_sum_kernel(int64_t nblk, const double* __restrict__ partial,
                                                                   double* __restrict__ energy, int32_t* __restrict__ primed) {
  __shared__ double red[RS_ROWS];
  const int64_t g = blockIdx.x;
  double s = 0.0;
  for (int64_t p = threadIdx.x; p < nblk; p += RS_ROWS) s += partial[g * nblk + p];
  const double sum = rs_tree(s, red);
  if (threadIdx.x == 0) {
    energy[g] = sum;
    if (primed && g == 0) primed[0] = 1;
  }
}

}  // namespace ng

using namespace ng;

extern "C" int ng_restraint_loss(ng_ctx* ctx, void* stream, int R, int64_t n, const float* peaks, const float* targets,
                                 const float* weights, double* energy, float* dpeaks) {
  if (!ctx) return NG_ERR_INVALID;
  NG_REQUIRE(ctx, R >= 1 && n >= 0 && (int64_t)R * n < ((int64_t)1 << 31), "restraint_loss: R >= 1, n >= 0, R * n below 2^31");
  NG_REQUIRE(ctx, energy, "restraint_loss: energy required");
  NG_REQUIRE(ctx, n == 0 || (peaks && targets && weights && dpeaks), "restraint_loss: arguments");
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard dg(ctx->device);
  const int64_t nblk = cdiv(n, RS_ROWS);
  double* partial = (double*)workspace(ctx, (size_t)std::max<int64_t>(nblk, 1) * sizeof(double));
  if (!partial) return NG_ERR_NOMEM;
  ProfScope ps(ctx, st, "restraint_loss");
  if (nblk > 0)
    hipLaunchKernelGGL(restraint_atoms_kernel, dim3((unsigned)nblk), dim3(RS_ROWS), 0, st, R, n, peaks, targets, weights,
                       dpeaks, partial);
  hipLaunchKernelGGL(restraint_sum_kernel, dim3(1), dim3(RS_ROWS), 0, st, nblk, partial, energy);
  NG_HIP(ctx, hipGetLastError());
  return NG_OK;
}

extern "C" int ng_restraint_loss_ex(ng_ctx* ctx, void* stream, int R, int64_t n, int mode, const float* peaks,
                                    const float* targets, const float* weights, const float* c, const float* tol, float lambda,
                                    float* avg, int32_t* primed, double* energy, float* dpeaks) {
  if (!ctx) return NG_ERR_INVALID;
  NG_REQUIRE(ctx, R >= 1 && n >= 0 && (int64_t)R * n < ((int64_t)1 << 31),
             "restraint_loss_ex: R >= 1, n >= 0, R * n below 2^31");
  NG_REQUIRE(ctx, mode == NG_RESTRAINT_ENSEMBLE || mode == NG_RESTRAINT_INDEPENDENT,
             "restraint_loss_ex: mode NG_RESTRAINT_ENSEMBLE or NG_RESTRAINT_INDEPENDENT");
  NG_REQUIRE(ctx, lambda >= 0.0f && lambda < 1.0f, "restraint_loss_ex: lambda in [0, 1)");
  NG_REQUIRE(ctx, !(mode == NG_RESTRAINT_INDEPENDENT && c), "restraint_loss_ex: replica weights c in ensemble mode only");
  NG_REQUIRE(ctx, !(lambda > 0.0f) || (avg && primed), "restraint_loss_ex: time averaging (lambda > 0) needs avg and primed");
  NG_REQUIRE(ctx, energy, "restraint_loss_ex: energy required");
  NG_REQUIRE(ctx, n == 0 || (peaks && targets && weights && dpeaks), "restraint_loss_ex: arguments");
  const int indep = mode == NG_RESTRAINT_INDEPENDENT;
  const int64_t G = indep ? R : 1;
  const int64_t nblk = cdiv(n, RS_ROWS);
  NG_REQUIRE(ctx, G * std::max<int64_t>(nblk, 1) < ((int64_t)1 << 24), "restraint_loss_ex: G * ceil(n / 256) below 2^24");
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard dg(ctx->device);
  double* partial = (double*)workspace(ctx, (size_t)std::max<int64_t>(G * nblk, 1) * sizeof(double));
  if (!partial) return NG_ERR_NOMEM;
  const bool averaging = lambda > 0.0f;
  ProfScope ps(ctx, st, "restraint_loss_ex");
  if (nblk > 0)
    hipLaunchKernelGGL(restraint_ex_atoms_kernel, dim3((unsigned)(G * nblk)), dim3(RS_ROWS), 0, st, R, n, nblk, indep, peaks,
                       targets, weights, c, tol, lambda, averaging ? avg : nullptr, averaging ? primed : nullptr, dpeaks, partial);
  hipLaunchKernelGGL(restraint_ex_sum_kernel, dim3((unsigned)G), dim3(RS_ROWS), 0, st, nblk, partial, energy,
                     averaging ? primed : nullptr);
  NG_HIP(ctx, hipGetLastError());
  return NG_OK;
}
