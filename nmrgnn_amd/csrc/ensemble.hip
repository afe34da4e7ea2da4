// Moments over the replicas of an ensemble: per atom the mean and the unbiased variance of S predicted shifts mu[s][i], and
// the mean of S per-replica variances v[s][i] (the closed-form dropout variance of ng_head_fwd_var).  By the law of total
// variance  Var(delta_i) = mean_s v[s][i] + Var_s(mu[s][i]):  "model" part + "input" part.
//
// One thread per atom, replicas in their order: mu[s][i] is read with stride N, so a wave's loads are coalesced across atoms.
// Sums are float64 (as in metrics.hip) and shifted by the first replica: a nitrogen shift is about 120 ppm with a spread of a
// few hundredths, and sum d^2 - (sum d)^2 / S of d_s = mu_s - mu_0 cancels digits of the spread, not of the shift.  d_s is
// exact in float64, so a column of equal values gives var_input exactly 0.  No atomics; every result is rounded to float32 once.
#include "ng_internal.h"

namespace ng {

__global__ __launch_bounds__(256) void ensemble_moments_kernel(int S, int64_t N, const float* __restrict__ mu,
                                                               const float* __restrict__ v, float* __restrict__ mean,
                                                               float* __restrict__ var_input,
                                                               float* __restrict__ var_model) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const double m0 = (double)mu[i];
  double sd = 0.0, sd2 = 0.0, sv = v ? (double)v[i] : 0.0;
  for (int s = 1; s < S; ++s) {
    const double d = (double)mu[(int64_t)s * N + i] - m0;
    sd += d;
    sd2 += d * d;
    if (v) sv += (double)v[(int64_t)s * N + i];
  }
  mean[i] = (float)(m0 + sd / (double)S);
  double vi = 0.0;
  if (S > 1) {
    vi = (sd2 - sd * sd / (double)S) / (double)(S - 1);
    if (vi < 0.0) vi = 0.0;      // the difference of the two sums can round below 0; NaN stays NaN
  }
  var_input[i] = (float)vi;
  if (v) var_model[i] = (float)(sv / (double)S);
}

}  // namespace ng

using namespace ng;

extern "C" int ng_ensemble_moments(ng_ctx* ctx, void* stream, int S, int64_t N, const float* mu, const float* v, float* mean,
                                   float* var_input, float* var_model) {
  if (!ctx) return NG_ERR_INVALID;
  NG_REQUIRE(ctx, S >= 1, "ensemble_moments: at least one replica");
  NG_REQUIRE(ctx, N >= 0, "ensemble_moments: negative atom count");
  NG_REQUIRE(ctx, mu && mean && var_input, "ensemble_moments: mu, mean and var_input required");
  NG_REQUIRE(ctx, (v == nullptr) == (var_model == nullptr), "ensemble_moments: v and var_model are both given or both NULL");
  if (N == 0) return NG_OK;
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(ctx, st, "ensemble_moments");
  hipLaunchKernelGGL(ensemble_moments_kernel, dim3((unsigned)cdiv(N, 256)), dim3(256), 0, st, S, N, mu, v, mean, var_input,
                     var_model);
  NG_HIP(ctx, hipGetLastError());
  return NG_OK;
}
