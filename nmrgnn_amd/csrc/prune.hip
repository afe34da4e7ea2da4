// Receptive-field pruning of a graph batch (include/nmrgnn_hip.h: ng_receptive_hops, ng_prune_*).
// The model is strictly local: the shift of an atom depends on the atoms within mp_layers list steps of it.  Given the
// selected atoms, these kernels mark that field (one frontier round per hop along OUTGOING live entries), compress the
// batch to it, and expand per-atom values and the edge gradient back to the parent's shape.  Integer work and copies
// only: every output is a function of the inputs alone, so two calls give the same bits.
#include <hip/hip_runtime.h>

#include "ng_common.h"
#include "nmrgnn_hip.h"

namespace ng {

constexpr int PR_BLOCK = 256;
constexpr int PR_MAX_HOPS = 64;

// the liveness rule of ng_build_incoming_lists: edges > 0 (NULL: every entry) AND 0 <= target < N
__device__ __forceinline__ bool pr_live(const float* __restrict__ edges, int64_t e, int32_t t, int N) {
  return (edges == nullptr || edges[e] > 0.f) && t >= 0 && t < N;
}
__device__ __forceinline__ int pr_row(int64_t e, int K, const int32_t* __restrict__ row_of) {
  return K > 0 ? (int)(e / K) : row_of[e];
}

__global__ __launch_bounds__(PR_BLOCK) void pr_seed_kernel(int N, const int32_t* __restrict__ seed, int32_t* __restrict__ hop) {
  const int64_t i = (int64_t)blockIdx.x * PR_BLOCK + threadIdx.x;      // 64 bits: N may lie within one block of 2^31
  if (i < N) hop[i] = seed[i] != 0 ? 0 : -1;
}

// round d: every live entry of a row at hop d - 1 claims its target.  All contenders write the same d.
__global__ __launch_bounds__(PR_BLOCK) void pr_round_kernel(int64_t n_entries, int N, int K, int d, const int32_t* __restrict__ row_of,
                                                            const int32_t* __restrict__ nlist, const float* __restrict__ edges,
                                                            int32_t* hop) {
  const int64_t e = (int64_t)blockIdx.x * PR_BLOCK + threadIdx.x;
  if (e >= n_entries) return;
  const int i = pr_row(e, K, row_of);
  if (i < 0 || i >= N) return;
  if (__hip_atomic_load(&hop[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != d - 1) return;
  const int32_t t = nlist[e];
  if (!pr_live(edges, e, t, N)) return;
  atomicCAS(&hop[t], -1, d);
}

__global__ __launch_bounds__(PR_BLOCK) void pr_flags_kernel(int N, const int32_t* __restrict__ hop, int32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * PR_BLOCK + threadIdx.x;
  if (i < N) flag[i] = hop[i] >= 0 ? 1 : 0;
}

// degrees of the pruned CSR rows at the PARENT's row positions: the parent degree of a kept row with hop < hops, else 0
__global__ __launch_bounds__(PR_BLOCK) void pr_degrees_kernel(int N, int hops, const int32_t* __restrict__ row_ptr,
                                                              const int32_t* __restrict__ hop, int32_t* __restrict__ deg) {
  const int64_t i = (int64_t)blockIdx.x * PR_BLOCK + threadIdx.x;
  if (i >= N) return;
  const int h = hop[i];
  deg[i] = h >= 0 && h < hops ? row_ptr[i + 1] - row_ptr[i] : 0;
}

// per kept row: keep, hop_p, inv_degree_p, atoms_p (a thread per (atom, column)); CSR: row_ptr_p from the scanned degrees
__global__ __launch_bounds__(PR_BLOCK) void pr_rows_kernel(int N, int C, const int32_t* __restrict__ hop, const int32_t* __restrict__ idx,
                                                           const float* __restrict__ atoms, const float* __restrict__ inv_degree,
                                                           const int32_t* __restrict__ rp_full, int32_t* __restrict__ keep,
                                                           int32_t* __restrict__ hop_p, float* __restrict__ atoms_p,
                                                           float* __restrict__ inv_p, int32_t* __restrict__ row_ptr_p) {
  const int64_t t = (int64_t)blockIdx.x * PR_BLOCK + threadIdx.x;
  const int Cw = C > 0 ? C : 1;
  const int i = (int)(t / Cw), c = (int)(t % Cw);
  if (i >= N) return;
  const int h = hop[i];
  if (h < 0) return;
  const int r = idx[i];
  if (C > 0) atoms_p[(int64_t)r * C + c] = atoms[(int64_t)i * C + c];
  if (c == 0) {
    keep[r] = i;
    hop_p[r] = h;
    inv_p[r] = inv_degree[i];
    if (row_ptr_p) {
      row_ptr_p[r] = rp_full[i];
      if (r == idx[N] - 1) row_ptr_p[r + 1] = rp_full[N];
    }
  }
}

// padded form, a thread per parent slot of a kept row: the live slots of rows with hop < hops with compressed targets, every
// other slot dead: (first kept atom of the row's graph, 0.0) — the builders' (0, 0.0) shifted to the batch
__global__ __launch_bounds__(PR_BLOCK) void pr_slots_kernel(int64_t n_entries, int N, int K, int G, int hops,
                                                            const int32_t* __restrict__ graph_ptr, const int32_t* __restrict__ nlist,
                                                            const float* __restrict__ edges, const int32_t* __restrict__ hop,
                                                            const int32_t* __restrict__ idx, int32_t* __restrict__ nlist_p,
                                                            float* __restrict__ edges_p) {
  const int64_t e = (int64_t)blockIdx.x * PR_BLOCK + threadIdx.x;
  if (e >= n_entries) return;
  const int i = (int)(e / K), k = (int)(e % K);
  const int h = hop[i];
  if (h < 0) return;
  const int64_t o = (int64_t)idx[i] * K + k;
  const int32_t t = nlist[e];
  if (h < hops && pr_live(edges, e, t, N)) {       // the target sits at hop <= h + 1 <= hops: kept
    nlist_p[o] = idx[t];
    edges_p[o] = edges[e];
    return;
  }
  int lo = 0, hi = G;                              // the graph g with graph_ptr[g] <= i < graph_ptr[g + 1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (graph_ptr[mid] <= i) lo = mid; else hi = mid;
  }
  nlist_p[o] = idx[graph_ptr[lo]];
  edges_p[o] = 0.f;
}

// CSR form, a thread per parent entry of a kept row with hop < hops: same position inside the row.  An entry that is not
// live (a validated CSR batch holds none) becomes (the row itself, 0.0).
__global__ __launch_bounds__(PR_BLOCK) void pr_entries_csr_kernel(int64_t nnz, int N, int hops, const int32_t* __restrict__ row_ptr,
                                                                  const int32_t* __restrict__ row_of, const int32_t* __restrict__ col,
                                                                  const float* __restrict__ dist, const int32_t* __restrict__ hop,
                                                                  const int32_t* __restrict__ idx, const int32_t* __restrict__ rp_full,
                                                                  int32_t* __restrict__ col_p, float* __restrict__ dist_p,
                                                                  int32_t* __restrict__ row_of_p) {
  const int64_t e = (int64_t)blockIdx.x * PR_BLOCK + threadIdx.x;
  if (e >= nnz) return;
  const int i = row_of[e];
  if (i < 0 || i >= N) return;
  const int h = hop[i];
  if (h < 0 || h >= hops) return;
  const int64_t o = (int64_t)rp_full[i] + (e - row_ptr[i]);
  const int32_t t = col[e];
  const bool live = pr_live(dist, e, t, N);
  col_p[o] = live ? idx[t] : idx[i];
  dist_p[o] = live ? dist[e] : 0.f;
  row_of_p[o] = idx[i];
}

// every entry of the parent-shaped de: the pruned value where the entry was kept, +0.0 elsewhere
__global__ __launch_bounds__(PR_BLOCK) void pr_expand_de_kernel(int64_t n_entries, int N, int K, int hops, const int32_t* __restrict__ row_ptr,
                                                                const int32_t* __restrict__ row_of, const int32_t* __restrict__ nlist,
                                                                const float* __restrict__ edges, const int32_t* __restrict__ hop,
                                                                const int32_t* __restrict__ idx, const int32_t* __restrict__ row_ptr_p,
                                                                const float* __restrict__ de_p, float* __restrict__ de) {
  const int64_t e = (int64_t)blockIdx.x * PR_BLOCK + threadIdx.x;
  if (e >= n_entries) return;
  const int i = pr_row(e, K, row_of);
  float v = 0.f;
  if (i >= 0 && i < N) {
    const int h = hop[i];
    if (h >= 0 && h < hops && pr_live(edges, e, nlist[e], N))
      v = K > 0 ? de_p[(int64_t)idx[i] * K + (e % K)] : de_p[(int64_t)row_ptr_p[idx[i]] + (e - row_ptr[i])];
  }
  de[e] = v;
}

__global__ __launch_bounds__(PR_BLOCK) void pr_fill_kernel(int64_t n, float fill, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * PR_BLOCK + threadIdx.x;
  if (i < n) out[i] = fill;
}
__global__ __launch_bounds__(PR_BLOCK) void pr_scatter_rows_kernel(int M, int N, const int32_t* __restrict__ keep,
                                                                   const float* __restrict__ v, float* __restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * PR_BLOCK + threadIdx.x;
  if (r >= M) return;
  const int i = keep[r];
  if (i >= 0 && i < N) out[i] = v[r];
}

static unsigned pr_grid(int64_t n) { return (unsigned)cdiv(n, PR_BLOCK); }

}  // namespace ng

using namespace ng;

#define PR_SIZES(ctx, what)                                                                                         \
  NG_REQUIRE(ctx, N >= 0 && N < ((int64_t)1 << 31) - 1, what ": N out of range");                                   \
  NG_REQUIRE(ctx, K >= 0 && K <= 64, what ": K in [0, 64] (0: CSR form)");                                          \
  NG_REQUIRE(ctx, n_entries >= 0 && n_entries < ((int64_t)1 << 31), what ": fewer than 2^31 list entries");         \
  NG_REQUIRE(ctx, K == 0 || n_entries == N * (int64_t)K, what ": padded form has N*K entries");                     \
  NG_REQUIRE(ctx, hops >= 0 && hops <= PR_MAX_HOPS, what ": hops in [0, 64]")

extern "C" int ng_receptive_hops(ng_ctx* ctx, void* stream, int64_t N, int K, int64_t n_entries, const int32_t* row_ptr,
                                 const int32_t* row_of, const int32_t* nlist, const float* edges, const int32_t* seed, int hops,
                                 int32_t* hop) {
  if (!ctx) return NG_ERR_INVALID;
  PR_SIZES(ctx, "receptive hops");
  NG_REQUIRE(ctx, n_entries == 0 || nlist, "receptive hops: nlist required");
  NG_REQUIRE(ctx, n_entries == 0 || K > 0 || (row_ptr && row_of), "receptive hops: CSR form needs row_ptr and row_of");
  NG_REQUIRE(ctx, N == 0 || (seed && hop), "receptive hops: seed / hop required");
  if (N == 0) return NG_OK;
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard dg(ctx->device);
  ProfScope ps(ctx, st, "receptive_hops");
  hipLaunchKernelGGL(pr_seed_kernel, dim3(pr_grid(N)), dim3(PR_BLOCK), 0, st, (int)N, seed, hop);
  if (n_entries > 0)
    for (int d = 1; d <= hops; ++d)
      hipLaunchKernelGGL(pr_round_kernel, dim3(pr_grid(n_entries)), dim3(PR_BLOCK), 0, st, n_entries, (int)N, K, d, row_of, nlist, edges,
                         hop);
  NG_HIP(ctx, hipGetLastError());
  return NG_OK;
}

extern "C" int ng_prune_keep_flags(ng_ctx* ctx, void* stream, int64_t N, const int32_t* hop, int32_t* flag) {
  if (!ctx) return NG_ERR_INVALID;
  NG_REQUIRE(ctx, N >= 0 && N < ((int64_t)1 << 31) - 1 && (N == 0 || (hop && flag)), "prune flags: arguments");
  if (N == 0) return NG_OK;
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard dg(ctx->device);
  ProfScope ps(ctx, st, "prune_flags");
  hipLaunchKernelGGL(pr_flags_kernel, dim3(pr_grid(N)), dim3(PR_BLOCK), 0, st, (int)N, hop, flag);
  NG_HIP(ctx, hipGetLastError());
  return NG_OK;
}

extern "C" int ng_prune_degrees_csr(ng_ctx* ctx, void* stream, int64_t N, int hops, const int32_t* row_ptr, const int32_t* hop,
                                    int32_t* deg) {
  if (!ctx) return NG_ERR_INVALID;
  NG_REQUIRE(ctx, N >= 0 && N < ((int64_t)1 << 31) - 1 && (N == 0 || (row_ptr && hop && deg)), "prune degrees: arguments");
  NG_REQUIRE(ctx, hops >= 0 && hops <= PR_MAX_HOPS, "prune degrees: hops in [0, 64]");
  if (N == 0) return NG_OK;
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard dg(ctx->device);
  ProfScope ps(ctx, st, "prune_degrees");
  hipLaunchKernelGGL(pr_degrees_kernel, dim3(pr_grid(N)), dim3(PR_BLOCK), 0, st, (int)N, hops, row_ptr, hop, deg);
  NG_HIP(ctx, hipGetLastError());
  return NG_OK;
}

extern "C" int ng_prune_lists(ng_ctx* ctx, void* stream, int64_t N, int K, int C, int G, int hops, const int32_t* graph_ptr,
                              const int32_t* nlist, const float* edges, const float* atoms, const float* inv_degree,
                              const int32_t* hop, const int32_t* idx, int32_t* keep, int32_t* hop_p, float* atoms_p,
                              float* inv_degree_p, int32_t* nlist_p, float* edges_p) {
  if (!ctx) return NG_ERR_INVALID;
  const int64_t n_entries = N * (int64_t)(K > 0 ? K : 0);
  PR_SIZES(ctx, "prune lists");
  NG_REQUIRE(ctx, K > 0, "prune lists: padded form (K > 0); ng_prune_lists_csr for CSR");
  NG_REQUIRE(ctx, C >= 0 && G >= 1 && graph_ptr, "prune lists: C >= 0, at least one graph, graph_ptr");
  NG_REQUIRE(ctx, N == 0 || (nlist && edges && inv_degree && hop && idx && (atoms || C == 0)), "prune lists: inputs");
  NG_REQUIRE(ctx, N == 0 || (keep && hop_p && inv_degree_p && nlist_p && edges_p && (atoms_p || C == 0)), "prune lists: outputs");
  if (N == 0) return NG_OK;
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard dg(ctx->device);
  ProfScope ps(ctx, st, "prune_lists");
  hipLaunchKernelGGL(pr_rows_kernel, dim3(pr_grid(N * (int64_t)std::max(C, 1))), dim3(PR_BLOCK), 0, st, (int)N, C, hop, idx, atoms,
                     inv_degree, (const int32_t*)nullptr, keep, hop_p, atoms_p, inv_degree_p, (int32_t*)nullptr);
  hipLaunchKernelGGL(pr_slots_kernel, dim3(pr_grid(n_entries)), dim3(PR_BLOCK), 0, st, n_entries, (int)N, K, G, hops, graph_ptr, nlist,
                     edges, hop, idx, nlist_p, edges_p);
  NG_HIP(ctx, hipGetLastError());
  return NG_OK;
}

extern "C" int ng_prune_lists_csr(ng_ctx* ctx, void* stream, int64_t N, int64_t n_entries, int C, int hops, const int32_t* row_ptr,
                                  const int32_t* row_of, const int32_t* col, const float* dist, const float* atoms,
                                  const float* inv_degree, const int32_t* hop, const int32_t* idx, const int32_t* rp_full,
                                  int32_t* keep, int32_t* hop_p, float* atoms_p, float* inv_degree_p, int32_t* row_ptr_p,
                                  int32_t* col_p, float* dist_p, int32_t* row_of_p) {
  if (!ctx) return NG_ERR_INVALID;
  const int K = 0;
  PR_SIZES(ctx, "prune lists csr");
  NG_REQUIRE(ctx, C >= 0 && row_ptr_p, "prune lists csr: C >= 0, row_ptr_p");
  NG_REQUIRE(ctx, N == 0 || (row_ptr && inv_degree && hop && idx && rp_full && (atoms || C == 0)), "prune lists csr: inputs");
  NG_REQUIRE(ctx, n_entries == 0 || (row_of && col && dist), "prune lists csr: lists");
  NG_REQUIRE(ctx, N == 0 || (keep && hop_p && inv_degree_p && (atoms_p || C == 0)), "prune lists csr: row outputs");
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard dg(ctx->device);
  if (N == 0) { NG_HIP(ctx, hipMemsetAsync(row_ptr_p, 0, sizeof(int32_t), st)); return NG_OK; }
  ProfScope ps(ctx, st, "prune_lists_csr");
  NG_HIP(ctx, hipMemsetAsync(row_ptr_p, 0, sizeof(int32_t), st));      // M == 0: row_ptr_p is [0]
  hipLaunchKernelGGL(pr_rows_kernel, dim3(pr_grid(N * (int64_t)std::max(C, 1))), dim3(PR_BLOCK), 0, st, (int)N, C, hop, idx, atoms,
                     inv_degree, rp_full, keep, hop_p, atoms_p, inv_degree_p, row_ptr_p);
  if (n_entries > 0 && col_p && dist_p && row_of_p)      // NULL outputs: the pruned batch holds no entry
    hipLaunchKernelGGL(pr_entries_csr_kernel, dim3(pr_grid(n_entries)), dim3(PR_BLOCK), 0, st, n_entries, (int)N, hops, row_ptr, row_of,
                       col, dist, hop, idx, rp_full, col_p, dist_p, row_of_p);
  NG_HIP(ctx, hipGetLastError());
  return NG_OK;
}

extern "C" int ng_prune_expand_edge_grad(ng_ctx* ctx, void* stream, int64_t N, int K, int64_t n_entries, int hops,
                                         const int32_t* row_ptr, const int32_t* row_of, const int32_t* nlist, const float* edges,
                                         const int32_t* hop, const int32_t* idx, const int32_t* row_ptr_p, const float* de_p,
                                         float* de) {
  if (!ctx) return NG_ERR_INVALID;
  PR_SIZES(ctx, "prune expand edge grad");
  NG_REQUIRE(ctx, n_entries == 0 || (nlist && hop && idx && de), "prune expand edge grad: arguments");
  NG_REQUIRE(ctx, n_entries == 0 || K > 0 || (row_ptr && row_of && row_ptr_p), "prune expand edge grad: CSR form needs row_ptr, row_of, row_ptr_p");
  if (n_entries == 0) return NG_OK;
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard dg(ctx->device);
  ProfScope ps(ctx, st, "prune_expand_de");
  hipLaunchKernelGGL(pr_expand_de_kernel, dim3(pr_grid(n_entries)), dim3(PR_BLOCK), 0, st, n_entries, (int)N, K, hops, row_ptr, row_of,
                     nlist, edges, hop, idx, row_ptr_p, de_p, de);
  NG_HIP(ctx, hipGetLastError());
  return NG_OK;
}

extern "C" int ng_prune_expand_rows(ng_ctx* ctx, void* stream, int64_t N, int64_t M, const int32_t* keep, const float* v, float fill,
                                    float* out) {
  if (!ctx) return NG_ERR_INVALID;
  NG_REQUIRE(ctx, N >= 0 && N < ((int64_t)1 << 31) - 1 && M >= 0 && M <= N, "prune expand rows: 0 <= M <= N < 2^31 - 1");
  NG_REQUIRE(ctx, (N == 0 || out) && (M == 0 || (keep && v)), "prune expand rows: arguments");
  if (N == 0) return NG_OK;
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard dg(ctx->device);
  ProfScope ps(ctx, st, "prune_expand_rows");
  hipLaunchKernelGGL(pr_fill_kernel, dim3(pr_grid(N)), dim3(PR_BLOCK), 0, st, N, fill, out);
  if (M > 0) hipLaunchKernelGGL(pr_scatter_rows_kernel, dim3(pr_grid(M)), dim3(PR_BLOCK), 0, st, (int)M, (int)N, keep, v, out);
  NG_HIP(ctx, hipGetLastError());
  return NG_OK;
}
