// Building a record store on the device (include/nmrgnn_hip.h: ng_store_from_batch, ng_label_moments).
//
// ng_store_from_batch is the inverse of ng_collate_batch (collate.hip): the rows of a ragged kNN batch (structures_to_batch:
// batch-global neighbour indices, graph_ptr) plus one label and one name id per atom become store rows row0 .. row0 + N with
// record-LOCAL indices, the store's padding convention (a slot that is not live holds nlist 0 and edges +0.0f), inv_degree
// recomputed from the local list, y = (shift, name id, mask) and w = mask.  Copies, one integer subtraction and one compare
// per list slot: every output is a function of the inputs alone, so two calls give the same bits; only the two counters add.
//
// Launch arithmetic (restated in tests/test_gpu_records.py): RC_TILE = 256 batch rows per workgroup trip, 256 threads,
// grid = min(ceil(N / RC_TILE), RC_MAX_BLOCKS = 1024) workgroups that stride over the tiles.  Per tile: thread t owns row
// tile0 + t for the search (binary search of graph_ptr; the structure's offset and size staged in LDS) and the label words
// (y, w); the workgroup then moves the tile's list rows cooperatively, a thread per chunk of a row, RC_UNROLL chunks in flight
// per thread before the first store, counting the slots with a local index > 0 per row in LDS (integer adds: order does not
// matter); thread t writes inv_degree of its row from that count; the atom rows of a tile are contiguous in the batch AND in
// the store, so they move as one flat run.  Chunk width: the list rows 16 bytes where K % 4 == 0 and the four list arrays are
// 16-byte aligned (row0 * K * 4 is then a multiple of 16), one word otherwise; the atom run 16 or 8 bytes where b_atoms and
// s_atoms + row0 * C are aligned so (an odd row0 with C = 10 leaves 8), one word otherwise, the run's last words one by one.
//
// ng_label_moments: per element c the float64 sums (count, sum y0, sum y0^2) over the labelled rows (y[:, 2] > 0) of the
// records ids[0..Rv), the element of a row being its first non-zero atom column.  Two stages as ng_name_metrics (metrics.hip):
// workgroup b takes the records ids[b], ids[b + nb], ... in 256-row tiles; per tile the threads stage (element, y0) in LDS,
// then thread (g, c) adds the rows g, g + groups, ... of element c in order; the groups are summed in order into
// partial[b][c][3]; a second launch sums the partials of every (c, j) in a fixed order.  No atomics: bitwise deterministic.
// More than 256 elements: one pass over the rows per 256 elements.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ng_common.h"
#include "nmrgnn_hip.h"

namespace ng {

constexpr int RC_TILE = 256;          // batch rows per workgroup trip == threads per workgroup
constexpr int RC_MAX_BLOCKS = 1024;   // 4 workgroups (16 waves) on each of 256 CUs
constexpr int RC_UNROLL = 4;          // list chunks a thread holds in flight

struct StoreArgs {
  const int32_t* graph_ptr; const float* b_atoms; const int32_t* b_nlist; const float* b_edges; const float* shift;
  const int32_t* name_id;
  float* s_atoms; int32_t* s_nlist; float* s_edges; float* s_inv; float* s_y; float* s_w;   // already advanced to row0
  int32_t* counters;
  int N, K, C, G;
  int vec_k, vec_c;                    // words per chunk: 4 or 1 for the list rows, 4, 2 or 1 for the atom run
};

// one list slot: (local index, edge) as the store keeps it; bad counts a live slot that points outside its structure
__device__ __forceinline__ void rc_slot(int32_t& nl, float& e, int32_t off, int32_t n, int& deg, int& bad) {
  const bool live = e > 0.0f;                               // false for +-0 and NaN
  const int64_t loc = (int64_t)nl - (int64_t)off;
  const bool inside = loc >= 0 && loc < (int64_t)n;
  bad += (live && !inside) ? 1 : 0;
  const bool keep = live && inside;
  nl = keep ? (int32_t)loc : 0;
  e = keep ? e : 0.0f;
  deg += nl > 0 ? 1 : 0;
}
__device__ __forceinline__ void rc_chunk(int32_t& nl, float& e, int32_t off, int32_t n, int& deg, int& bad) {
  rc_slot(nl, e, off, n, deg, bad);
}
__device__ __forceinline__ void rc_chunk(int4& nl, float4& e, int32_t off, int32_t n, int& deg, int& bad) {
  rc_slot(nl.x, e.x, off, n, deg, bad);
  rc_slot(nl.y, e.y, off, n, deg, bad);
  rc_slot(nl.z, e.z, off, n, deg, bad);
  rc_slot(nl.w, e.w, off, n, deg, bad);
}

// rows x q chunks of the tile's list rows (contiguous on both sides): localise, pad, count
template <typename TI, typename TF>
__device__ __forceinline__ int rc_move_lists(const TI* __restrict__ bn, const TF* __restrict__ be, TI* __restrict__ sn,
                                             TF* __restrict__ se, const int32_t* s_off, const int32_t* s_n, int* s_deg, int rows,
                                             int q, int t) {
  const int items = rows * q;
  int bad = 0;
  for (int base = t; base < items; base += RC_UNROLL * RC_TILE) {
    TI v[RC_UNROLL];
    TF e[RC_UNROLL];
#pragma unroll
    for (int u = 0; u < RC_UNROLL; ++u) {
      const int it = base + u * RC_TILE;
      const int itc = it < items ? it : base;              // a slot past the tile reads the thread's first chunk again
      v[u] = bn[itc];
      e[u] = be[itc];
    }
#pragma unroll
    for (int u = 0; u < RC_UNROLL; ++u) {
      const int it = base + u * RC_TILE;
      if (it < items) {
        const int r = it / q;
        int deg = 0;
        rc_chunk(v[u], e[u], s_off[r], s_n[r], deg, bad);
        sn[it] = v[u];
        se[it] = e[u];
        if (deg) atomicAdd(&s_deg[r], deg);
      }
    }
  }
  return bad;
}

template <typename T>
__device__ __forceinline__ void rc_copy_run(const T* __restrict__ s, T* __restrict__ d, int items, int t) {
  for (int base = t; base < items; base += RC_UNROLL * RC_TILE) {
    T v[RC_UNROLL];
#pragma unroll
    for (int u = 0; u < RC_UNROLL; ++u) {
      const int it = base + u * RC_TILE;
      v[u] = s[it < items ? it : base];
    }
#pragma unroll
    for (int u = 0; u < RC_UNROLL; ++u)
      if (base + u * RC_TILE < items) d[base + u * RC_TILE] = v[u];
  }
}

__global__ __launch_bounds__(RC_TILE) void store_from_batch_kernel(const StoreArgs a) {
  __shared__ int32_t s_off[RC_TILE];   // graph_ptr of the row's structure
  __shared__ int32_t s_n[RC_TILE];     // its atom count
  __shared__ int s_deg[RC_TILE];       // slots of the row with a local index > 0
  __shared__ int s_cnt[2];
  const int t = threadIdx.x;
  if (t < 2) s_cnt[t] = 0;
  int bad = 0, labelled = 0;
  const int n_tiles = (a.N + RC_TILE - 1) / RC_TILE;
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int tile0 = tile * RC_TILE;                     // < N < 2^31 - RC_TILE
    const int rows = min(RC_TILE, a.N - tile0);
    s_deg[t] = 0;
    if (t < rows) {
      const int i = tile0 + t;
      int lo = 0, hi = a.G;                               // the last g < G with graph_ptr[g] <= i
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.graph_ptr[mid] <= i) lo = mid; else hi = mid;
      }
      const int32_t off = a.graph_ptr[lo];
      const int64_t n = (int64_t)a.graph_ptr[lo + 1] - off;
      s_off[t] = off;
      s_n[t] = n > 0 ? (int32_t)std::min<int64_t>(n, INT32_MAX) : 0;   // a graph_ptr that does not ascend: no slot is inside
      const float sh = a.shift[i];
      const bool has = fabsf(sh) < INFINITY;              // false for NaN and +-inf
      const float m = has ? 1.0f : 0.0f;
      a.s_y[(int64_t)i * 3] = has ? sh : 0.0f;
      a.s_y[(int64_t)i * 3 + 1] = (float)a.name_id[i];
      a.s_y[(int64_t)i * 3 + 2] = m;
      a.s_w[i] = m;
      labelled += has ? 1 : 0;
    }
    __syncthreads();
    if (a.vec_k == 4) {
      const int kq = a.K >> 2;
      bad += rc_move_lists(reinterpret_cast<const int4*>(a.b_nlist) + (int64_t)tile0 * kq,
                           reinterpret_cast<const float4*>(a.b_edges) + (int64_t)tile0 * kq,
                           reinterpret_cast<int4*>(a.s_nlist) + (int64_t)tile0 * kq,
                           reinterpret_cast<float4*>(a.s_edges) + (int64_t)tile0 * kq, s_off, s_n, s_deg, rows, kq, t);
    } else {
      bad += rc_move_lists(a.b_nlist + (int64_t)tile0 * a.K, a.b_edges + (int64_t)tile0 * a.K, a.s_nlist + (int64_t)tile0 * a.K,
                           a.s_edges + (int64_t)tile0 * a.K, s_off, s_n, s_deg, rows, a.K, t);
    }
    {
      const float* src = a.b_atoms + (int64_t)tile0 * a.C;
      float* dst = a.s_atoms + (int64_t)tile0 * a.C;
      const int words = rows * a.C;                       // <= 256 * 4096
      const int wide = words / a.vec_c;
      if (a.vec_c == 4) rc_copy_run(reinterpret_cast<const float4*>(src), reinterpret_cast<float4*>(dst), wide, t);
      else if (a.vec_c == 2) rc_copy_run(reinterpret_cast<const float2*>(src), reinterpret_cast<float2*>(dst), wide, t);
      else rc_copy_run(src, dst, wide, t);
      const int done = wide * a.vec_c;                    // the run's last words (fewer than vec_c)
      if (t < words - done) dst[done + t] = src[done + t];
    }
    __syncthreads();
    if (t < rows) {
      const int deg = s_deg[t];
      a.s_inv[tile0 + t] = deg > 0 ? 1.0f / (float)deg : 0.f;
    }
    __syncthreads();                                      // the next trip rewrites the staged rows
  }
  if (bad) atomicAdd(&s_cnt[0], bad);
  if (labelled) atomicAdd(&s_cnt[1], labelled);
  __syncthreads();
  if (t < 2 && s_cnt[t]) atomicAdd(&a.counters[t], s_cnt[t]);
}

static bool rc_aligned(const void* p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) == 0; }

// ---- label moments ---------------------------------------------------------------------------------------------------

constexpr int LM_THREADS = 256;     // = rows per tile = elements per pass
constexpr int LM_MAX_BLOCKS = 256;  // stage-1 workgroups: one per CU
constexpr int LM_SUMS = 3;

__global__ __launch_bounds__(LM_THREADS) void label_moments_partial_kernel(int64_t R, int64_t Ntot, int C,
                                                                           const float* __restrict__ atoms,
                                                                           const float* __restrict__ y,
                                                                           const int64_t* __restrict__ rec_ptr,
                                                                           const int32_t* __restrict__ ids, int64_t Rv,
                                                                           double* __restrict__ partial) {
  __shared__ int s_el[LM_THREADS];
  __shared__ double s_y0[LM_THREADS];
  __shared__ double red[LM_SUMS][LM_THREADS];
  const int t = threadIdx.x;
  for (int cbase = 0; cbase < C; cbase += LM_THREADS) {
    const int Cp = min(C - cbase, LM_THREADS);            // elements of this pass
    const int groups = LM_THREADS / Cp;
    const int g = t / Cp, c = cbase + (t - g * Cp);
    double cnt = 0.0, s1 = 0.0, s2 = 0.0;
    for (int64_t v = blockIdx.x; v < Rv; v += gridDim.x) {
      const int64_t id = ids[v];
      if (id < 0 || id >= R) continue;                    // uniform over the workgroup
      const int64_t r0 = rec_ptr[id], r1 = rec_ptr[id + 1];
      if (r0 < 0 || r1 > Ntot || r1 < r0) continue;       // a record outside the store is never read
      for (int64_t row0 = r0; row0 < r1; row0 += LM_THREADS) {
        const int64_t row = row0 + t;
        int el = -1;
        double y0 = 0.0;
        if (row < r1 && y[row * 3 + 2] > 0.0f) {
          const float* ar = atoms + row * C;
          for (int k = 0; k < C; ++k)
            if (ar[k] != 0.0f) { el = k; break; }
          y0 = (double)y[row * 3];
        }
        s_el[t] = el;
        s_y0[t] = y0;
        __syncthreads();
        if (g < groups) {
          const int lim = (int)std::min<int64_t>(LM_THREADS, r1 - row0);
          for (int r = g; r < lim; r += groups)
            if (s_el[r] == c) {
              const double yy = s_y0[r];
              cnt += 1.0;
              s1 += yy;
              s2 += yy * yy;
            }
        }
        __syncthreads();
      }
    }
    red[0][t] = cnt;
    red[1][t] = s1;
    red[2][t] = s2;
    __syncthreads();
    if (t < Cp) {
      double o0 = 0.0, o1 = 0.0, o2 = 0.0;
      for (int q = 0; q < groups; ++q) {
        o0 += red[0][q * Cp + t];
        o1 += red[1][q * Cp + t];
        o2 += red[2][q * Cp + t];
      }
      double* p = partial + ((int64_t)blockIdx.x * C + (cbase + t)) * LM_SUMS;
      p[0] = o0;
      p[1] = o1;
      p[2] = o2;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(64) void label_moments_final_kernel(int nb, int ncj, const double* __restrict__ partial,
                                                                 double* __restrict__ out) {
  const int cj = blockIdx.x, lane = threadIdx.x;
  double s = 0.0;
  for (int b = lane; b < nb; b += 64) s += partial[(int64_t)b * ncj + cj];
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if (lane == 0) out[cj] = s;
}

}  // namespace ng

using namespace ng;

extern "C" int ng_store_from_batch(ng_ctx* ctx, void* stream, int64_t N, int K, int C, int G, const int32_t* graph_ptr,
                                   const float* b_atoms, const int32_t* b_nlist, const float* b_edges, const float* shift,
                                   const int32_t* name_id, int64_t row0, int64_t Ncap, float* s_atoms, int32_t* s_nlist,
                                   float* s_edges, float* s_inv_degree, float* s_y, float* s_w, int32_t* counters) {
  if (!ctx) return NG_ERR_INVALID;
  NG_REQUIRE(ctx, K >= 1 && K <= 4096 && C >= 1 && C <= 4096, "store_from_batch: K and C in [1, 4096]");
  NG_REQUIRE(ctx, N >= 0 && N < ((int64_t)1 << 31) - RC_TILE, "store_from_batch: N out of range");
  NG_REQUIRE(ctx, G >= 0 && (N == 0 || G >= 1) && G <= N, "store_from_batch: G structures of at least one atom each make up N atoms");
  NG_REQUIRE(ctx, row0 >= 0 && Ncap >= 0 && row0 <= Ncap && N <= Ncap - row0, "store_from_batch: rows [row0, row0 + N) of a store of Ncap rows");
  if (N == 0) return NG_OK;
  NG_REQUIRE(ctx, graph_ptr && b_atoms && b_nlist && b_edges && shift && name_id, "store_from_batch: batch arrays");
  NG_REQUIRE(ctx, s_atoms && s_nlist && s_edges && s_inv_degree && s_y && s_w, "store_from_batch: store arrays");
  NG_REQUIRE(ctx, counters, "store_from_batch: counters");
  StoreArgs a;
  a.graph_ptr = graph_ptr; a.b_atoms = b_atoms; a.b_nlist = b_nlist; a.b_edges = b_edges; a.shift = shift; a.name_id = name_id;
  a.s_atoms = s_atoms + row0 * C; a.s_nlist = s_nlist + row0 * K; a.s_edges = s_edges + row0 * K;
  a.s_inv = s_inv_degree + row0; a.s_y = s_y + row0 * 3; a.s_w = s_w + row0;
  a.counters = counters;
  a.N = (int)N; a.K = K; a.C = C; a.G = G;
  a.vec_k = (K % 4 == 0 && rc_aligned(b_nlist, 16) && rc_aligned(b_edges, 16) && rc_aligned(a.s_nlist, 16) && rc_aligned(a.s_edges, 16)) ? 4 : 1;
  a.vec_c = (rc_aligned(b_atoms, 16) && rc_aligned(a.s_atoms, 16)) ? 4 : (rc_aligned(b_atoms, 8) && rc_aligned(a.s_atoms, 8)) ? 2 : 1;
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard dg(ctx->device);
  ProfScope ps(ctx, st, "store_from_batch");
  const int64_t tiles = cdiv(N, RC_TILE);
  const unsigned grid = (unsigned)(tiles < RC_MAX_BLOCKS ? tiles : RC_MAX_BLOCKS);
  hipLaunchKernelGGL(store_from_batch_kernel, dim3(grid), dim3(RC_TILE), 0, st, a);
  NG_HIP(ctx, hipGetLastError());
  return NG_OK;
}

extern "C" int ng_label_moments(ng_ctx* ctx, void* stream, int64_t R, int64_t Ntot, int C, const float* atoms, const float* y,
                                const int64_t* rec_ptr, const int32_t* ids, int64_t Rv, double* out) {
  if (!ctx) return NG_ERR_INVALID;
  NG_REQUIRE(ctx, C >= 1 && C <= 4096, "label_moments: C in [1, 4096]");
  NG_REQUIRE(ctx, R >= 0 && Ntot >= R, "label_moments: a store of R records and Ntot >= R rows");
  NG_REQUIRE(ctx, Rv >= 0 && Rv < ((int64_t)1 << 31), "label_moments: Rv out of range");
  NG_REQUIRE(ctx, out != nullptr, "label_moments: no output");
  NG_REQUIRE(ctx, Rv == 0 || (atoms && y && rec_ptr && ids), "label_moments: store arrays / ids");
  hipStream_t st = (hipStream_t)stream;
  const int ncj = LM_SUMS * C;
  const int nb = (int)std::min<int64_t>(Rv, LM_MAX_BLOCKS);
  DeviceGuard dg(ctx->device);
  double* partial = (double*)workspace(ctx, (size_t)std::max(nb, 1) * ncj * sizeof(double));
  if (!partial) return NG_ERR_NOMEM;
  ProfScope ps(ctx, st, "label_moments");
  if (nb > 0)
    hipLaunchKernelGGL(label_moments_partial_kernel, dim3((unsigned)nb), dim3(LM_THREADS), 0, st, R, Ntot, C, atoms, y, rec_ptr,
                       ids, Rv, partial);
  // nb == 0 (an empty view): the final launch writes zeros
  hipLaunchKernelGGL(label_moments_final_kernel, dim3((unsigned)ncj), dim3(64), 0, st, nb, ncj, partial, out);
  NG_HIP(ctx, hipGetLastError());
  return NG_OK;
}
