// Ensemble-averaged training loss (nmrgnn_amd/engine.py: Engine.loss_groups): the two kernels around the
// existing NameLoss kernels.  A batch of G graphs is partitioned into Q groups by group_ptr [Q + 1] (graph indices); the R_q
// members of group q have the same n_q atoms and sit back to back, member r's atom i at row graph_ptr[group_ptr[q]] + r n_q + i.
// mean_ptr [Q + 1] is the prefix sum of n_q, M = mean_ptr[Q] the number of means.
//
//   ng_group_mean    mean_out[j] = the member mean of flat mean index j; y_out / w_out / names_out = the first member's rows
//   ng_group_spread  dpred of every member row from dmean[j]
//
// Both are ONE launch of one thread per flat mean index j (the work is balanced over j, not over groups: a batch holds
// thousands of groups of 1 to a few thousand atoms).  A workgroup owns the 256 indices [256 b, 256 b + 256); it finds the first
// and the last group that they touch by two uniform binary searches over mean_ptr (at most 256 groups apart: every group has
// at least one atom), and a thread then searches only between those.  Lanes of a wave hold consecutive i of (mostly) one group,
// so each of the R_q member streams is read, and in the spread written, as consecutive dwords.  M is known on the device only:
// the grid covers N >= M indices and a workgroup past M returns at once.  No atomics, no scratch, no host read: the same call
// writes the same bits, and both kernels can be captured.  Float32 throughout, every product and sum rounded on its own (no
// fused multiply-add), in member order: a NumPy restatement gives the same bits (tests/group_loss_ref.py).
//
// The device does not verify that the members of a group have equal sizes (the host does: Engine.loss_groups); a group whose
// members would reach outside [0, G) graphs or [0, N) rows is skipped, never read or written out of bounds.
#include "ng_internal.h"

namespace ng {

constexpr int GL_THREADS = 256;

// largest q in [lo, hi] with mean_ptr[q] <= j (mean_ptr[lo] <= j is the caller's)
__device__ __forceinline__ int gl_group_of(const int32_t* __restrict__ mean_ptr, int lo, int hi, int j) {
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (mean_ptr[mid] <= j) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

struct GlSlot {
  bool ok;          // this thread owns a mean index whose member rows all lie inside the batch
  int g0, R;        // first member graph, members
  int64_t row, n;   // member 0's row of this atom, rows between members
};

__device__ __forceinline__ GlSlot gl_slot(int64_t N, int G, int Q, const int32_t* __restrict__ graph_ptr,
                                          const int32_t* __restrict__ group_ptr, const int32_t* __restrict__ mean_ptr, int M,
                                          int j) {
  GlSlot s;
  s.ok = false;
  s.g0 = 0; s.R = 0; s.row = 0; s.n = 0;
  // the workgroup's group range, the same in every thread
  const int j0 = (int)blockIdx.x * GL_THREADS;
  const int j1 = min(j0 + GL_THREADS - 1, M - 1);
  const int q0 = gl_group_of(mean_ptr, 0, Q - 1, j0);
  const int q1 = gl_group_of(mean_ptr, q0, min(q0 + GL_THREADS - 1, Q - 1), j1);
  if (j >= M) return s;
  const int q = gl_group_of(mean_ptr, q0, q1, j);
  const int m0 = mean_ptr[q];
  const int n = mean_ptr[q + 1] - m0, i = j - m0;
  const int g0 = group_ptr[q], R = group_ptr[q + 1] - g0;
  if (i < 0 || i >= n || g0 < 0 || R < 1 || (int64_t)g0 + R > G) return s;
  const int64_t row = (int64_t)graph_ptr[g0] + i;
  if (row < 0 || row + (int64_t)(R - 1) * n >= N) return s;
  s.ok = true;
  s.g0 = g0; s.R = R; s.row = row; s.n = n;
  return s;
}

__global__ __launch_bounds__(GL_THREADS) void group_mean_kernel(int64_t N, int G, int Q, const int32_t* __restrict__ graph_ptr,
                                                                const int32_t* __restrict__ group_ptr,
                                                                const int32_t* __restrict__ mean_ptr,
                                                                const float* __restrict__ pred, const float* __restrict__ c,
                                                                const float* __restrict__ y, const float* __restrict__ w,
                                                                const int32_t* __restrict__ names, float* __restrict__ mean_out,
                                                                float* __restrict__ y_out, float* __restrict__ w_out,
                                                                int32_t* __restrict__ names_out) {
#pragma clang fp contract(off)
  const int M = mean_ptr[Q];
  if ((int64_t)blockIdx.x * GL_THREADS >= M) return;
  const int j = (int)blockIdx.x * GL_THREADS + (int)threadIdx.x;
  const GlSlot s = gl_slot(N, G, Q, graph_ptr, group_ptr, mean_ptr, M, j);
  if (!s.ok) return;
  const float* p = pred + s.row;
  float m;
  if (c) {
    const float* cg = c + s.g0;
    m = cg[0] * p[0];
    int r = 1;
    for (; r + 4 <= s.R; r += 4) {      // four loads in flight, added in member order
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = p[(int64_t)(r + u) * s.n];
#pragma unroll
      for (int u = 0; u < 4; ++u) m = m + cg[r + u] * v[u];
    }
    for (; r < s.R; ++r) m = m + cg[r] * p[(int64_t)r * s.n];
  } else {
    float sum = p[0];
    int r = 1;
    for (; r + 4 <= s.R; r += 4) {
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = p[(int64_t)(r + u) * s.n];
#pragma unroll
      for (int u = 0; u < 4; ++u) sum = sum + v[u];
    }
    for (; r < s.R; ++r) sum = sum + p[(int64_t)r * s.n];
    m = sum / (float)s.R;               // R = 1: x / 1 is x
  }
  mean_out[j] = m;
  y_out[j] = y[s.row];
  w_out[j] = w[s.row];
  if (names) names_out[j] = names[s.row];
}

__global__ __launch_bounds__(GL_THREADS) void group_spread_kernel(int64_t N, int G, int Q, const int32_t* __restrict__ graph_ptr,
                                                                  const int32_t* __restrict__ group_ptr,
                                                                  const int32_t* __restrict__ mean_ptr,
                                                                  const float* __restrict__ dmean, const float* __restrict__ c,
                                                                  float scale, float* __restrict__ dpred) {
#pragma clang fp contract(off)
  const int M = mean_ptr[Q];
  if ((int64_t)blockIdx.x * GL_THREADS >= M) return;
  const int j = (int)blockIdx.x * GL_THREADS + (int)threadIdx.x;
  const GlSlot s = gl_slot(N, G, Q, graph_ptr, group_ptr, mean_ptr, M, j);
  if (!s.ok) return;
  const float d = dmean[j];
  float* out = dpred + s.row;
  if (c) {
    const float* cg = c + s.g0;
    for (int r = 0; r < s.R; ++r) out[(int64_t)r * s.n] = (d * cg[r]) * scale;
  } else {
    const float q = (d / (float)s.R) * scale;
    for (int r = 0; r < s.R; ++r) out[(int64_t)r * s.n] = q;
  }
}

static int gl_check(ng_ctx* ctx, int64_t N, int G, int Q, const void* graph_ptr, const void* group_ptr, const void* mean_ptr) {
  NG_REQUIRE(ctx, Q >= 1, "group loss: at least one group");
  NG_REQUIRE(ctx, Q <= G, "group loss: more groups than graphs");
  NG_REQUIRE(ctx, N < ((int64_t)1 << 31), "group loss: 2^31 atoms or more");
  NG_REQUIRE(ctx, N >= G, "group loss: fewer atoms than graphs");
  NG_REQUIRE(ctx, graph_ptr && group_ptr && mean_ptr, "group loss: graph_ptr, group_ptr and mean_ptr required");
  return NG_OK;
}

}  // namespace ng

using namespace ng;

extern "C" int ng_group_mean(ng_ctx* ctx, void* stream, int64_t N, int G, int Q, const int32_t* graph_ptr,
                             const int32_t* group_ptr, const int32_t* mean_ptr, const float* pred, const float* c,
                             const float* y, const float* w, const int32_t* names, float* mean_out, float* y_out, float* w_out,
                             int32_t* names_out) {
  if (!ctx) return NG_ERR_INVALID;
  if (int rc = gl_check(ctx, N, G, Q, graph_ptr, group_ptr, mean_ptr)) return rc;
  NG_REQUIRE(ctx, pred && y && w && mean_out && y_out && w_out, "group_mean: pred, y, w and their outputs required");
  NG_REQUIRE(ctx, (names == nullptr) == (names_out == nullptr), "group_mean: names and names_out go together");
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(ctx, st, "group_mean");
  hipLaunchKernelGGL(group_mean_kernel, dim3((unsigned)cdiv(N, GL_THREADS)), dim3(GL_THREADS), 0, st, N, G, Q, graph_ptr,
                     group_ptr, mean_ptr, pred, c, y, w, names, mean_out, y_out, w_out, names_out);
  NG_HIP(ctx, hipGetLastError());
  return NG_OK;
}

extern "C" int ng_group_spread(ng_ctx* ctx, void* stream, int64_t N, int G, int Q, const int32_t* graph_ptr,
                               const int32_t* group_ptr, const int32_t* mean_ptr, const float* dmean, const float* c, float scale,
                               float* dpred) {
  if (!ctx) return NG_ERR_INVALID;
  if (int rc = gl_check(ctx, N, G, Q, graph_ptr, group_ptr, mean_ptr)) return rc;
  NG_REQUIRE(ctx, dmean && dpred, "group_spread: dmean and dpred required");
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(ctx, st, "group_spread");
  hipLaunchKernelGGL(group_spread_kernel, dim3((unsigned)cdiv(N, GL_THREADS)), dim3(GL_THREADS), 0, st, N, G, Q, graph_ptr,
                     group_ptr, mean_ptr, dmean, c, scale, dpred);
  NG_HIP(ctx, hipGetLastError());
  return NG_OK;
}
