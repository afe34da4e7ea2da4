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
