// Neighbour lists of a RAGGED batch: G structures of different sizes, concatenated along the rows (graph_ptr [G+1] on the
// device), built in one launch per pass.  The uniform builders (knn.hip, cutoff.hip) take G frames of one
// topology with the frames on gridDim.y (G <= 65535); here a library of small molecules or a few proteins of different sizes
// is one call, G limited only by int32 rows.
//
// One thread per query row, 256 consecutive rows per workgroup.  A thread finds its row's structure by a binary search of
// graph_ptr; the rows of a workgroup belong to a run of consecutive structures, so the candidates the workgroup needs are one
// contiguous span of rows, [gp[first], gp[last + 1]).  That span streams through LDS tiles of float4 positions (one
// ds_read_b128 per candidate; lanes of different structures read different slots) and every thread walks only the part of a
// tile that lies inside its own structure.  A 24-atom molecule therefore costs its thread 23 candidate steps, not a wave of 64
// lanes with 40 idle (knn_wave_kernel) or a 256-thread workgroup of its own (knn_kernel).  For a structure of a few thousand
// atoms one thread per query is a serial chain of thousands of steps in too few waves, so the kNN rows of structures of
// 257..4096 atoms take a second launch, one wave per query (knn_ragged_wave_kernel), and the first launch skips them.
//
// Every convention is the uniform builders', so that each structure's rows are, bit for bit, what ng_knn_graph /
// ng_cutoff_fill_rows give for that structure alone, indices shifted by gp[g]: the same squared-distance expression
// (pbc.cuh: pbc_dist2, with DispOpen's c - q), candidates visited in ascending index with strict comparisons (ties -> lower
// index), distances sqrt(d2) * scale, unused kNN slots (0, 0.0), batch-global indices, inv_degree = 1/#(structure-local
// neighbour index > 0) (library.py:115-116), cutoff rows in ascending neighbour index.
//
// kNN structures of >= 16384 atoms (the uniform path's switch point) take the cell grid of knn_cells.hip, one call per such
// structure on its own rows: the ragged launch skips their rows, and a fix-up launch adds gp[g] to the frame-local indices the
// grid writes.  The cutoff builder is brute force at every size, as the uniform one is.
//
// Periodic boxes: every structure has a boundary kind of its own (the _pbc entry points: box [G][9], kind [G]).  The three
// kernels take the displacement policy as a template argument: DispOpen for the open entry points, DispPer (pbc.cuh) for the
// boxed ones, where a row loads the kind and box of ITS structure and each structure's rows are what ng_knn_graph_pbc /
// ng_cutoff_fill_rows_pbc give for it alone with its own box and flag.  The cell grid runs per structure with that structure's
// box pointer and kind, from a host copy of the kinds.
#include <algorithm>
#include <climits>

#include "ng_common.h"
#include "ng_internal.h"
#include "nlist_common.cuh"
#include "ragged.cuh"

namespace ng {

constexpr int RG_TILE = 1024;        // candidates per LDS tile: 16 KiB of float4
constexpr int RG_CELLS_MIN = 16384;  // kNN structures from this size on take the cell grid (knn.hip: knn_graph_impl)
constexpr int RG_WAVE_MIN = 256;     // kNN structures of more atoms, up to 4096, take one wave per query row

// the candidate span of a workgroup: the union of the ranges of its active rows (block-wide min / max through LDS);
// returns false when no row of the workgroup is active
__device__ __forceinline__ bool rg_span(bool active, RgRange r, int& s0, int& s1) {
  __shared__ int lo_s, hi_s;
  if (threadIdx.x == 0) { lo_s = INT_MAX; hi_s = INT_MIN; }
  __syncthreads();
  if (active) { atomicMin(&lo_s, r.lo); atomicMax(&hi_s, r.hi); }
  __syncthreads();
  s0 = lo_s; s1 = hi_s;
  return s0 < s1;
}

// rows [t0, t0 + cnt) of pos -> LDS
__device__ __forceinline__ void rg_stage(float4* sp, const float* __restrict__ pos, int t0, int cnt) {
  __syncthreads();
  for (int t = threadIdx.x; t < cnt; t += 256) {
    const float* p = pos + 3 * (int64_t)(t0 + t);
    sp[t] = make_float4(p[0], p[1], p[2], 0.f);
  }
  __syncthreads();
}

// kNN: the search of knn_kernel (knn.hip) over the row's own structure.  Rows of structures of (wlo, whi] atoms are left to
// knn_ragged_wave_kernel, rows of structures of `big` atoms or more to the cell grid (neither is written here).
// Disp: DispOpen (box / kind unused: the lists of the open entry points), or DispPer with box [G][9] and kind [G]: a row loads
// the box of its own structure; the candidate span and its LDS tiles stay shared over the workgroup.
template <int KMAX, class Disp>
__global__ __launch_bounds__(256) void knn_ragged_kernel(int G, int N, int K, float scale, int wlo, int whi, int big,
                                                         const float* __restrict__ pos,       // [N][3]
                                                         const int32_t* __restrict__ gp,      // [G+1]
                                                         int32_t* __restrict__ nlist,         // [N][K]
                                                         float* __restrict__ edges,           // [N][K]
                                                         float* __restrict__ inv_degree,      // [N]
                                                         const float* __restrict__ box,       // [G][9] or unused
                                                         const int32_t* __restrict__ kind) {  // [G] or unused
  __shared__ float4 sp[RG_TILE];
  const int i = blockIdx.x * 256 + threadIdx.x;
  RgRange r{0, 0, 0};
  if (i < N) r = rg_range(gp, G, N, i);
  const int n = r.hi - r.lo;
  const bool active = i < N && n < big && !(n > wlo && n <= whi);
  int s0, s1;
  if (!rg_span(active, r, s0, s1)) return;          // uniform over the workgroup
  Disp D;
  if (active) disp_load(D, box, kind, r.g);
  float qx = 0.f, qy = 0.f, qz = 0.f;
  if (active) { qx = pos[3 * (int64_t)i]; qy = pos[3 * (int64_t)i + 1]; qz = pos[3 * (int64_t)i + 2]; }
  float bd[KMAX];
  int bi[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) { bd[k] = INFINITY; bi[k] = 0; }

  for (int t0 = s0; t0 < s1; t0 += RG_TILE) {
    const int cnt = min(RG_TILE, s1 - t0);
    rg_stage(sp, pos, t0, cnt);
    if (active) {
      const int ta = max(r.lo, t0) - t0, tb = min(r.hi, t0 + cnt) - t0;
      for (int t = ta; t < tb; ++t) {
        const float4 c = sp[t];
        float dx, dy, dz;
        D(qx, qy, qz, c.x, c.y, c.z, dx, dy, dz);
        const float d2 = pbc_dist2(dx, dy, dz);
        const int j = t0 + t;
        NG_KNN_INSERT(KMAX, bd, bi, d2, j, i);
      }
    }
  }
  if (!active) return;
  NG_KNN_WRITE_ROW(KMAX, K, bd, bi, i, 0, r.lo, scale, nlist, edges, inv_degree);      // batch-global indices in the list
}

// One WAVE per query row for the rows of mid-sized structures (wlo, 64 * STEPS] atoms: the algorithm of knn_wave_kernel
// (knn.hip) on the row's own structure, keys (bits(d2) << 32 | structure-local index), so the lists are the other kernels'
// bit for bit.  One thread per query leaves a 2770-atom structure with 44 waves that each walk all 2770 candidates (0.44 ms);
// here it is 2770 waves of 44 steps.  Candidates are read from global memory (a structure of <= 4096 atoms is <= 48 KiB, held
// by the caches); the waves of rows outside (wlo, 64 * STEPS] leave after the search of graph_ptr.
template <int STEPS, class Disp>
__global__ __launch_bounds__(256) void knn_ragged_wave_kernel(int G, int N, int K, float scale, int wlo,
                                                              const float* __restrict__ pos, const int32_t* __restrict__ gp,
                                                              int32_t* __restrict__ nlist, float* __restrict__ edges,
                                                              float* __restrict__ inv_degree, const float* __restrict__ box,
                                                              const int32_t* __restrict__ kind) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = blockIdx.x * 4 + wave;
  if (i >= N) return;                             // uniform over the wave
  const RgRange r = rg_range(gp, G, N, i);
  const int lo = __builtin_amdgcn_readfirstlane(r.lo), n = __builtin_amdgcn_readfirstlane(r.hi) - lo;
  if (n <= wlo || n > 64 * STEPS) return;
  const float qx = pos[3 * (int64_t)i], qy = pos[3 * (int64_t)i + 1], qz = pos[3 * (int64_t)i + 2];
  const float* sp = pos + 3 * (int64_t)lo;
  Disp D;
  disp_load(D, box, kind, __builtin_amdgcn_readfirstlane(r.g));     // one structure, one kind per wave
  // A: keys of this lane's candidates t = 64 s + lane, and their minimum
  knn_u64 key[STEPS];
  knn_u64 mn = ~0ull;
#pragma unroll
  for (int s = 0; s < STEPS; ++s) {
    const int t = 64 * s + lane;
    const int tc = min(t, n - 1);
    float dx, dy, dz;
    D(qx, qy, qz, sp[3 * tc], sp[3 * tc + 1], sp[3 * tc + 2], dx, dy, dz);
    const float d2 = pbc_dist2(dx, dy, dz);
    knn_u64 k = NG_KNN_KEY(d2, (unsigned)t);
    if (t >= n || lo + t == i) k = ~0ull;
    key[s] = k;
    mn = k < mn ? k : mn;
  }
  NG_KNN_WAVE_SELECT(STEPS, key, mn, K, list);
  NG_KNN_WAVE_WRITE_ROW(list, lane, K, i, lo, scale, nlist, edges, inv_degree);
}

// frame-local -> batch-global indices of one structure's rows from the cell grid (n >= 16384 > K: every slot is real)
__global__ __launch_bounds__(256) void knn_ragged_offset_kernel(int64_t count, int off, int32_t* __restrict__ nlist) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s < count) nlist[s] += off;
}

// cutoff: count (FILL = false: deg[N]) or fill pass (col / dist / row_of at row_ptr, inv_degree) of cutoff_kernel
// (cutoff.hip) over the row's own structure; Disp / box / kind as knn_ragged_kernel
template <bool FILL, class Disp>
__global__ __launch_bounds__(256) void cutoff_ragged_kernel(int G, int N, float cutoff2, float scale,
                                                            const float* __restrict__ pos, const int32_t* __restrict__ gp,
                                                            int32_t* __restrict__ deg, const int32_t* __restrict__ row_ptr,
                                                            int32_t* __restrict__ col, float* __restrict__ dist,
                                                            float* __restrict__ inv_degree, int32_t* __restrict__ row_of,
                                                            const float* __restrict__ box, const int32_t* __restrict__ kind) {
  __shared__ float4 sp[RG_TILE];
  const int i = blockIdx.x * 256 + threadIdx.x;
  RgRange r{0, 0, 0};
  if (i < N) r = rg_range(gp, G, N, i);
  const bool active = i < N;
  int s0, s1;
  if (!rg_span(active, r, s0, s1)) return;
  Disp D;
  if (active) disp_load(D, box, kind, r.g);
  float qx = 0.f, qy = 0.f, qz = 0.f;
  if (active) { qx = pos[3 * (int64_t)i]; qy = pos[3 * (int64_t)i + 1]; qz = pos[3 * (int64_t)i + 2]; }
  int cnt = 0, cnt_pos = 0;
  int64_t out = 0, lim = 0;          // a row never writes past its own extent, whatever the count pass saw
  if (FILL && active) { out = row_ptr[i]; lim = row_ptr[i + 1]; }
  for (int t0 = s0; t0 < s1; t0 += RG_TILE) {
    const int m = min(RG_TILE, s1 - t0);
    rg_stage(sp, pos, t0, m);
    if (active) {
      const int ta = max(r.lo, t0) - t0, tb = min(r.hi, t0 + m) - t0;
      for (int t = ta; t < tb; ++t) {
        const float4 c = sp[t];
        float dx, dy, dz;
        D(qx, qy, qz, c.x, c.y, c.z, dx, dy, dz);
        const float d2 = pbc_dist2(dx, dy, dz);
        const int j = t0 + t;
        NG_CUTOFF_HIT(FILL, d2, j, i, 0, r.lo, i, cutoff2, scale, out, lim, col, dist, row_of, cnt, cnt_pos);
      }
    }
  }
  if (!active) return;
  if (FILL) inv_degree[i] = cnt_pos > 0 ? 1.0f / (float)cnt_pos : 0.f;
  else deg[i] = cnt;
}

// The checks every entry point makes, in the order they fire: those of the batch first, then (the kNN builder puts its slot
// count between the two) those of the boxed entry points (Disp::periodic): box [G][9] and kind [G] on the device; a host copy
// of the kinds, where given, holds -1, 0 or 1.
static int ragged_check_batch(ng_ctx* ctx, int G, int64_t N, int max_n, const float* pos, const int32_t* graph_ptr) {
  NG_REQUIRE(ctx, G >= 0 && N >= 0 && max_n >= 0, "ragged graph: negative size");
  NG_REQUIRE(ctx, N < ((int64_t)1 << 31), "ragged graph: batch exceeds int32 rows");
  NG_REQUIRE(ctx, max_n <= N, "ragged graph: max_n exceeds the batch");
  NG_REQUIRE(ctx, N == 0 || (G >= 1 && pos && graph_ptr), "ragged graph: positions and graph_ptr required");
  return NG_OK;
}

template <class Disp>
static int ragged_check_boxes(ng_ctx* ctx, int G, int64_t N, const float* box, const int32_t* kind, const int32_t* kind_host) {
  if (!Disp::periodic) return NG_OK;
  NG_REQUIRE(ctx, N == 0 || (box && kind), "ragged graph (pbc): box and kind required");
  if (kind_host)
    for (int g = 0; g < G; ++g)
      NG_REQUIRE(ctx, kind_host[g] >= -1 && kind_host[g] <= 1, "ragged graph (pbc): kind -1 (open), 0 or 1");
  return NG_OK;
}

// The three builders, each the whole of an open entry point (Disp = DispOpen; box / kind / kind_host NULL) and of its _pbc twin
// (DispPer).
template <class Disp>
static int knn_ragged(ng_ctx* ctx, void* stream, int G, int64_t N, int K, float scale, const float* pos,
                      const int32_t* graph_ptr, const int32_t* graph_ptr_host, int max_n, const float* box, const int32_t* kind,
                      const int32_t* kind_host, int32_t* nlist, float* edges, float* inv_degree) {
  if (!ctx) return NG_ERR_INVALID;
  NG_REQUIRE(ctx, K >= 1 && K <= 64, "knn (ragged): neighbour count must be in [1,64]");
  if (const int rc = ragged_check_batch(ctx, G, N, max_n, pos, graph_ptr)) return rc;
  NG_REQUIRE(ctx, N * K < ((int64_t)1 << 31), "knn (ragged): N * K exceeds int32 slots");
  if (const int rc = ragged_check_boxes<Disp>(ctx, G, N, box, kind, kind_host)) return rc;
  if (N == 0) return NG_OK;
  hipStream_t st = (hipStream_t)stream;
  // structures of the cell grid: only when one may be that large, from the host copy of graph_ptr
  const bool cells = !sw().knn_brute && !sw().knn_serial && max_n >= RG_CELLS_MIN;
  NG_REQUIRE(ctx, !cells || graph_ptr_host, "knn (ragged): graph_ptr_host required when max_n >= 16384");
  NG_REQUIRE(ctx, !cells || !Disp::periodic || kind_host, "knn (ragged, pbc): kind_host required when max_n >= 16384");
  const int big = cells ? RG_CELLS_MIN : INT_MAX;
  // one wave per query for structures of (256, 4096] atoms, sized by the largest of them (NG_KNN=serial / lanes: off, as the
  // uniform path's wave kernel)
  const int wmax = std::min(max_n, 4096);
  const int steps = (sw().knn_serial || sw().knn_lanes || max_n <= RG_WAVE_MIN) ? 0 : wmax <= 1024 ? 16 : wmax <= 2048 ? 32
                    : wmax <= 3072 ? 48 : 64;
  const int whi = 64 * steps;
  {
    ProfScope ps(ctx, st, Disp::periodic ? "knn_graph_ragged_pbc" : "knn_graph_ragged");
    const dim3 grid((unsigned)cdiv(N, 256)), block(256);
#define NG_RG(KM) hipLaunchKernelGGL((knn_ragged_kernel<KM, Disp>), grid, block, 0, st, G, (int)N, K, scale, RG_WAVE_MIN, whi, big, \
                                     pos, graph_ptr, nlist, edges, inv_degree, box, kind)
    NG_KNN_LADDER(K, NG_RG);
#undef NG_RG
    NG_HIP(ctx, hipGetLastError());
    if (steps) {
      const dim3 gw((unsigned)cdiv(N, 4));
#define NG_RGW(S) hipLaunchKernelGGL((knn_ragged_wave_kernel<S, Disp>), gw, block, 0, st, G, (int)N, K, scale, RG_WAVE_MIN, pos, \
                                     graph_ptr, nlist, edges, inv_degree, box, kind)
      if (steps == 16) NG_RGW(16); else if (steps == 32) NG_RGW(32); else if (steps == 48) NG_RGW(48); else NG_RGW(64);
#undef NG_RGW
      NG_HIP(ctx, hipGetLastError());
    }
  }
  if (!cells) return NG_OK;
  for (int g = 0; g < G; ++g) {
    const int lo = graph_ptr_host[g], n = graph_ptr_host[g + 1] - lo;
    NG_REQUIRE(ctx, lo >= 0 && n >= 0 && (int64_t)lo + n <= N, "knn (ragged): graph_ptr_host outside the batch");
    if (n < big) continue;
    // the rows the ragged launch skipped; the brute-force kernel cannot take them back, so a size the grid refuses is an error
    NG_REQUIRE(ctx, knn_cells_supported(1, n, K), "knn (ragged): structure too large for the cell grid");
    const int64_t s0 = (int64_t)lo * K;
    // the structure's own box and kind: the call ng_knn_graph_pbc makes for it alone
    const int kg = Disp::periodic ? kind_host[g] : -1;
    if (const int rc = knn_cells(ctx, st, 1, n, K, scale, pos + 3 * (int64_t)lo, nlist + s0, edges + s0, inv_degree + lo,
                                 kg >= 0 ? box + 9 * (int64_t)g : nullptr, kg == 1 ? 1 : 0))
      return rc;
    if (lo > 0) {
      hipLaunchKernelGGL(knn_ragged_offset_kernel, dim3((unsigned)cdiv((int64_t)n * K, 256)), dim3(256), 0, st,
                         (int64_t)n * K, lo, nlist + s0);
      NG_HIP(ctx, hipGetLastError());
    }
  }
  return NG_OK;
}

template <class Disp>
static int cutoff_count_ragged(ng_ctx* ctx, void* stream, int G, int64_t N, float cutoff, const float* pos,
                               const int32_t* graph_ptr, int max_n, const float* box, const int32_t* kind,
                               const int32_t* kind_host, int32_t* deg) {
  if (!ctx) return NG_ERR_INVALID;
  NG_REQUIRE(ctx, cutoff > 0.f, "cutoff graph (ragged): cutoff > 0");
  if (const int rc = ragged_check_batch(ctx, G, N, max_n, pos, graph_ptr)) return rc;
  if (const int rc = ragged_check_boxes<Disp>(ctx, G, N, box, kind, kind_host)) return rc;
  if (N == 0) return NG_OK;
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(ctx, st, Disp::periodic ? "cutoff_count_ragged_pbc" : "cutoff_count_ragged");
  hipLaunchKernelGGL((cutoff_ragged_kernel<false, Disp>), dim3((unsigned)cdiv(N, 256)), dim3(256), 0, st, G, (int)N,
                     cutoff * cutoff, 1.0f, pos, graph_ptr, deg, nullptr, nullptr, nullptr, nullptr, nullptr, box, kind);
  NG_HIP(ctx, hipGetLastError());
  return NG_OK;
}

template <class Disp>
static int cutoff_fill_ragged(ng_ctx* ctx, void* stream, int G, int64_t N, float cutoff, float scale, const float* pos,
                              const int32_t* graph_ptr, int max_n, const float* box, const int32_t* kind,
                              const int32_t* kind_host, const int32_t* row_ptr, int32_t* col, float* dist, float* inv_degree,
                              int32_t* row_of) {
  if (!ctx) return NG_ERR_INVALID;
  NG_REQUIRE(ctx, cutoff > 0.f, "cutoff graph (ragged): cutoff > 0");
  if (const int rc = ragged_check_batch(ctx, G, N, max_n, pos, graph_ptr)) return rc;
  if (const int rc = ragged_check_boxes<Disp>(ctx, G, N, box, kind, kind_host)) return rc;
  if (N == 0) return NG_OK;
  NG_REQUIRE(ctx, row_ptr && inv_degree, "cutoff graph (ragged): row_ptr and inv_degree required");
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(ctx, st, Disp::periodic ? "cutoff_fill_ragged_pbc" : "cutoff_fill_ragged");
  hipLaunchKernelGGL((cutoff_ragged_kernel<true, Disp>), dim3((unsigned)cdiv(N, 256)), dim3(256), 0, st, G, (int)N,
                     cutoff * cutoff, scale, pos, graph_ptr, nullptr, row_ptr, col, dist, inv_degree, row_of, box, kind);
  NG_HIP(ctx, hipGetLastError());
  return NG_OK;
}

}  // namespace ng

using namespace ng;

extern "C" int ng_knn_graph_ragged(ng_ctx* ctx, void* stream, int G, int64_t N, int K, float scale, const float* pos,
                                   const int32_t* graph_ptr, const int32_t* graph_ptr_host, int max_n, int32_t* nlist,
                                   float* edges, float* inv_degree) {
  return knn_ragged<DispOpen>(ctx, stream, G, N, K, scale, pos, graph_ptr, graph_ptr_host, max_n, nullptr, nullptr, nullptr,
                              nlist, edges, inv_degree);
}

extern "C" int ng_cutoff_count_ragged(ng_ctx* ctx, void* stream, int G, int64_t N, float cutoff, const float* pos,
                                      const int32_t* graph_ptr, int max_n, int32_t* deg) {
  return cutoff_count_ragged<DispOpen>(ctx, stream, G, N, cutoff, pos, graph_ptr, max_n, nullptr, nullptr, nullptr, deg);
}

extern "C" int ng_cutoff_fill_rows_ragged(ng_ctx* ctx, void* stream, int G, int64_t N, float cutoff, float scale,
                                          const float* pos, const int32_t* graph_ptr, int max_n, const int32_t* row_ptr,
                                          int32_t* col, float* dist, float* inv_degree, int32_t* row_of) {
  return cutoff_fill_ragged<DispOpen>(ctx, stream, G, N, cutoff, scale, pos, graph_ptr, max_n, nullptr, nullptr, nullptr,
                                      row_ptr, col, dist, inv_degree, row_of);
}

// every structure with a boundary kind of its own: box [G][9] (pbc.cuh; zeros for an open structure) and kind [G] (-1 open,
// 0 orthorhombic, 1 reduced triclinic) on the device
extern "C" int ng_knn_graph_ragged_pbc(ng_ctx* ctx, void* stream, int G, int64_t N, int K, float scale, const float* pos,
                                       const int32_t* graph_ptr, const int32_t* graph_ptr_host, int max_n, const float* box,
                                       const int32_t* kind, const int32_t* kind_host, int32_t* nlist, float* edges,
                                       float* inv_degree) {
  return knn_ragged<DispPer>(ctx, stream, G, N, K, scale, pos, graph_ptr, graph_ptr_host, max_n, box, kind, kind_host, nlist,
                             edges, inv_degree);
}

extern "C" int ng_cutoff_count_ragged_pbc(ng_ctx* ctx, void* stream, int G, int64_t N, float cutoff, const float* pos,
                                          const int32_t* graph_ptr, int max_n, const float* box, const int32_t* kind,
                                          const int32_t* kind_host, int32_t* deg) {
  return cutoff_count_ragged<DispPer>(ctx, stream, G, N, cutoff, pos, graph_ptr, max_n, box, kind, kind_host, deg);
}

extern "C" int ng_cutoff_fill_rows_ragged_pbc(ng_ctx* ctx, void* stream, int G, int64_t N, float cutoff, float scale,
                                              const float* pos, const int32_t* graph_ptr, int max_n, const float* box,
                                              const int32_t* kind, const int32_t* kind_host, const int32_t* row_ptr,
                                              int32_t* col, float* dist, float* inv_degree, int32_t* row_of) {
  return cutoff_fill_ragged<DispPer>(ctx, stream, G, N, cutoff, scale, pos, graph_ptr, max_n, box, kind, kind_host, row_ptr,
                                     col, dist, inv_degree, row_of);
}
