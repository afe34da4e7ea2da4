// Fine-tuning: Adam over parameter groups of the flat buffer, and the clip factor of their gradient.
// The groups are at most NG_ADAM_MAX_SEGMENTS element ranges with a rate scale each; the table is a kernel argument BY VALUE
// (1.3 KB of the 4 KB argument block), read with scalar loads: no device table, no copy, nothing to keep alive for a capture.
// Both kernels walk segment by segment, grid-stride inside each: an element outside every segment, or in one of scale 0, is
// never addressed — neither its gradient nor its state.
#include <algorithm>
#include <cmath>

#include "ng_internal.h"

namespace ng {

struct SegTable {
  int64_t begin[NG_ADAM_MAX_SEGMENTS];
  int64_t end[NG_ADAM_MAX_SEGMENTS];
  float scale[NG_ADAM_MAX_SEGMENTS];
  int n;
};

constexpr int OPT_THREADS = 256;
constexpr int CLIP_MAX_BLOCKS = 1024;      // partials of the norm: a function of n alone, never of the CU count

// the update of adam_kernel (node_ops.hip), expression for expression; cf = 1 multiplies exactly
__global__ __launch_bounds__(OPT_THREADS) void adam_groups_kernel(SegTable tab, float* __restrict__ p, const float* __restrict__ g,
                                                                  float* __restrict__ m, float* __restrict__ v, float lr_t,
                                                                  float b1, float b2, float eps, float gscale,
                                                                  const double* __restrict__ clip) {
  const float cf = clip ? (float)clip[0] : 1.0f;
  for (int s = 0; s < tab.n; ++s) {
    const float sc = tab.scale[s];
    if (!(sc > 0.f)) continue;
    const float lr_s = lr_t * sc;
    const int64_t end = tab.end[s];
    for (int64_t i = tab.begin[s] + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < end;
         i += (int64_t)gridDim.x * blockDim.x) {
      const float gi = g[i] * gscale * cf;
      const float mi = b1 * m[i] + (1.0f - b1) * gi;
      const float vi = b2 * v[i] + (1.0f - b2) * gi * gi;
      m[i] = mi;
      v[i] = vi;
      p[i] -= lr_s * mi / (sqrtf(vi) + eps);
    }
  }
}

// the four waves of a workgroup in wave order; the butterfly leaves the same bits in every lane
__device__ __forceinline__ double block_sum_f64(double x, double* sm) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = x;
  __syncthreads();
  return (sm[0] + sm[1]) + (sm[2] + sm[3]);
}

__global__ __launch_bounds__(OPT_THREADS) void grad_sq_partial_kernel(SegTable tab, const float* __restrict__ g, float gscale,
                                                                      double* __restrict__ partial) {
  __shared__ double sm[OPT_THREADS / 64];
  double acc = 0.0;
  for (int s = 0; s < tab.n; ++s) {
    if (!(tab.scale[s] > 0.f)) continue;
    const int64_t end = tab.end[s];
    for (int64_t i = tab.begin[s] + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < end;
         i += (int64_t)gridDim.x * blockDim.x) {
      const double gi = (double)(g[i] * gscale);
      acc += gi * gi;
    }
  }
  const double tot = block_sum_f64(acc, sm);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

__global__ __launch_bounds__(OPT_THREADS) void grad_clip_final_kernel(int nb, const double* __restrict__ partial, double clipnorm,
                                                                      double* __restrict__ out2) {
  __shared__ double sm[OPT_THREADS / 64];
  double acc = 0.0;
  for (int i = threadIdx.x; i < nb; i += OPT_THREADS) acc += partial[i];
  const double norm = sqrt(block_sum_f64(acc, sm));
  if (threadIdx.x == 0) {
    // norm 0, NaN or inf: factor 1 (the comparison is false for NaN; inf is excluded by name)
    out2[0] = (norm > clipnorm && norm < (double)INFINITY) ? clipnorm / norm : 1.0;
    out2[1] = norm;
  }
}

// the refusals shared by both entry points; fills tab and counts the elements of segments with a scale > 0
static int seg_table(ng_ctx* ctx, int64_t n, int n_seg, const int64_t* seg_begin, const int64_t* seg_end, const float* seg_scale,
                     SegTable* tab, int64_t* active) {
  NG_REQUIRE(ctx, n >= 0, "segments: n is negative");
  NG_REQUIRE(ctx, n_seg >= 0 && n_seg <= NG_ADAM_MAX_SEGMENTS, "segments: at most 64 ranges");
  NG_REQUIRE(ctx, n_seg == 0 || (seg_begin && seg_end && seg_scale), "segments: NULL table");
  *tab = SegTable();
  *active = 0;
  for (int s = 0; s < n_seg; ++s) {
    const int64_t b = seg_begin[s], e = seg_end[s];
    NG_REQUIRE(ctx, b >= 0 && e <= n && b <= e, "segments: a range leaves [0, n) or ends before it begins");
    NG_REQUIRE(ctx, s == 0 || b >= seg_begin[s - 1], "segments: ranges are not sorted");
    NG_REQUIRE(ctx, s == 0 || b >= seg_end[s - 1], "segments: ranges overlap");
    NG_REQUIRE(ctx, std::isfinite(seg_scale[s]) && seg_scale[s] >= 0.f, "segments: a scale is negative or not finite");
    tab->begin[s] = b;
    tab->end[s] = e;
    tab->scale[s] = seg_scale[s];
    if (seg_scale[s] > 0.f) *active += e - b;
  }
  tab->n = n_seg;
  return NG_OK;
}

static inline dim3 opt_grid(int64_t work_items, int max_blocks) {
  return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(work_items, OPT_THREADS), max_blocks)));
}

}  // namespace ng

using namespace ng;

extern "C" int ng_adam_step_groups(ng_ctx* ctx, void* stream, int64_t n, float* p, const float* g, float* m, float* v, float lr,
                                   float beta1, float beta2, float eps, int64_t step, float grad_scale, int n_seg,
                                   const int64_t* seg_begin, const int64_t* seg_end, const float* seg_scale, const double* clip) {
  if (!ctx) return NG_ERR_INVALID;
  if (ctx->replay_armed)
    return fail(ctx, NG_ERR_UNSUPPORTED, "adam_groups: an armed replay context trains every parameter (ng_adam_step)");
  NG_REQUIRE(ctx, step >= 1, "adam_groups: step counts from 1");
  SegTable tab;
  int64_t active = 0;
  if (int rc = seg_table(ctx, n, n_seg, seg_begin, seg_end, seg_scale, &tab, &active)) return rc;
  NG_REQUIRE(ctx, active == 0 || (p && g && m && v), "adam_groups: NULL buffer");
  weights_bump(ctx);                 // as ng_adam_step: packed weight images are stale from here on
  if (n == 0) return NG_OK;
  const double lr_t = (double)lr * std::sqrt(1.0 - std::pow((double)beta2, (double)step)) /
                      (1.0 - std::pow((double)beta1, (double)step));
  if (active > 0) {
    ProfScope ps(ctx, (hipStream_t)stream, "adam_groups");
    hipLaunchKernelGGL(adam_groups_kernel, opt_grid(active, 256 * 8), dim3(OPT_THREADS), 0, (hipStream_t)stream, tab, p, g, m, v,
                       (float)lr_t, beta1, beta2, eps, grad_scale, clip);
    NG_HIP(ctx, hipGetLastError());
  }
  // images fed by frozen segments only are rebuilt too: correct, and one launch either way
  return repack_all(ctx, (hipStream_t)stream, p, p + n);
}

extern "C" int ng_grad_clip_factor(ng_ctx* ctx, void* stream, int64_t n, const float* g, float grad_scale, int n_seg,
                                   const int64_t* seg_begin, const int64_t* seg_end, const float* seg_scale, double clipnorm,
                                   double* out2) {
  if (!ctx) return NG_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  SegTable tab;
  int64_t active = 0;
  if (int rc = seg_table(ctx, n, n_seg, seg_begin, seg_end, seg_scale, &tab, &active)) return rc;
  NG_REQUIRE(ctx, clipnorm > 0.0 && std::isfinite(clipnorm), "grad_clip: clipnorm must be positive and finite");
  NG_REQUIRE(ctx, out2 != nullptr, "grad_clip: NULL output");
  NG_REQUIRE(ctx, active == 0 || g, "grad_clip: NULL gradient");
  const int nb = active > 0 ? (int)opt_grid(n, CLIP_MAX_BLOCKS).x : 0;
  double* partial = nullptr;
  if (nb > 0) {
    partial = (double*)workspace(ctx, (size_t)nb * sizeof(double));
    if (!partial) return NG_ERR_NOMEM;
  }
  ProfScope ps(ctx, st, "grad_clip");
  if (nb > 0)
    hipLaunchKernelGGL(grad_sq_partial_kernel, dim3(nb), dim3(OPT_THREADS), 0, st, tab, g, grad_scale, partial);
  hipLaunchKernelGGL(grad_clip_final_kernel, dim3(1), dim3(OPT_THREADS), 0, st, nb, partial, clipnorm, out2);
  NG_HIP(ctx, hipGetLastError());
  return NG_OK;
}
