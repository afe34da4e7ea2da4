// Mini-batch collation from a device-resident record store (include/nmrgnn_hip.h: ng_collate_batch).
// The store holds R records back to back (record r owns the rows [rec_ptr[r], rec_ptr[r + 1])) with record-local neighbour
// indices; a batch is the rows of the records ids[0..G) in that order, with graph_ptr[g] added to every neighbour index of
// graph g — the arrays graph.concat_graphs builds on the host.  Copies and one integer add per list slot: every output is
// a function of the inputs alone, nothing is allocated and nothing is accumulated, so two calls give the same bits.
//
// Launch arithmetic (restated in tests/test_gpu_collate.py): CL_TILE = 256 output atoms per workgroup trip, 256 threads,
// grid = min(ceil(N / CL_TILE), CL_MAX_BLOCKS = 1024) workgroups that stride over the tiles.  Per tile: thread t owns atom
// tile0 + t for the search (binary search of graph_ptr, source row and offset staged in LDS) and the per-atom words
// (inv_degree, y0, w, names, y_true); then the workgroup copies the tile's list rows and atom rows cooperatively, a thread
// per chunk of a row, CL_UNROLL chunks in flight per thread before the first store.  Chunk width: the list rows (nlist and
// edges together) 16 bytes where K % 4 == 0 and the four list arrays are 16-byte aligned, one word otherwise; the atom rows
// 16 bytes (C % 4 == 0), 8 bytes (C % 2 == 0) or one word, by C and the alignment of the two atoms arrays.
#include <hip/hip_runtime.h>

#include "ng_common.h"
#include "nmrgnn_hip.h"

namespace ng {

constexpr int CL_TILE = 256;          // output atoms per workgroup trip == threads per workgroup
constexpr int CL_MAX_BLOCKS = 1024;   // 4 workgroups (16 waves) on each of 256 CUs
constexpr int CL_UNROLL = 4;          // chunks of each array a thread holds in flight

struct CollateArgs {
  const float* s_atoms; const int32_t* s_nlist; const float* s_edges; const float* s_inv; const float* s_y; const float* s_w;
  const int64_t* rec_ptr; const int32_t* ids; const int32_t* graph_ptr;
  float* atoms; int32_t* nlist; float* edges; float* inv; float* y0; float* w; int32_t* names; float* y_true;
  int64_t R, Ntot;
  int N, K, C, G;
  int vec_k, vec_c;                    // words per chunk: 4 or 1 for the list rows, 4, 2 or 1 for the atom rows
};

__device__ __forceinline__ void cl_add(int32_t& v, int32_t off) { v += off; }
__device__ __forceinline__ void cl_add(int4& v, int32_t off) { v.x += off; v.y += off; v.z += off; v.w += off; }

// rows x q chunks of type T from the staged source rows to the tile's (contiguous) output rows
template <typename T>
__device__ __forceinline__ void cl_copy_rows(const T* __restrict__ s, T* __restrict__ d, const int64_t* s_src, int rows, int q,
                                             int t) {
  const int items = rows * q;
  for (int base = t; base < items; base += CL_UNROLL * CL_TILE) {
    T v[CL_UNROLL];
    bool ok[CL_UNROLL];
#pragma unroll
    for (int u = 0; u < CL_UNROLL; ++u) {
      const int it = base + u * CL_TILE;
      const int itc = it < items ? it : 0;                  // a slot past the tile, or of a skipped row, reads chunk 0 of
      const int r = itc / q, c = itc - r * q;              // the store (always there) and stores nothing
      const int64_t src = s_src[r];
      ok[u] = it < items && src >= 0;
      v[u] = s[ok[u] ? src * q + c : 0];
    }
#pragma unroll
    for (int u = 0; u < CL_UNROLL; ++u)
      if (ok[u]) d[base + u * CL_TILE] = v[u];
  }
}

// the same for the two list arrays at once: nlist + the graph's offset, edges as they are
template <typename TI, typename TF>
__device__ __forceinline__ void cl_copy_lists(const TI* __restrict__ sn, const TF* __restrict__ se, TI* __restrict__ dn,
                                              TF* __restrict__ de, const int64_t* s_src, const int32_t* s_off, int rows, int q,
                                              int t) {
  const int items = rows * q;
  for (int base = t; base < items; base += CL_UNROLL * CL_TILE) {
    TI v[CL_UNROLL];
    TF e[CL_UNROLL];
    bool ok[CL_UNROLL];
#pragma unroll
    for (int u = 0; u < CL_UNROLL; ++u) {
      const int it = base + u * CL_TILE;
      const int itc = it < items ? it : 0;                  // as cl_copy_rows
      const int r = itc / q, c = itc - r * q;
      const int64_t src = s_src[r];
      ok[u] = it < items && src >= 0;
      const int64_t o = ok[u] ? src * q + c : 0;
      v[u] = sn[o];
      e[u] = se[o];
      cl_add(v[u], s_off[r]);
    }
#pragma unroll
    for (int u = 0; u < CL_UNROLL; ++u)
      if (ok[u]) {
        dn[base + u * CL_TILE] = v[u];
        de[base + u * CL_TILE] = e[u];
      }
  }
}

__global__ __launch_bounds__(CL_TILE) void collate_kernel(const CollateArgs a) {
  __shared__ int64_t s_src[CL_TILE];   // source row of the tile's atom, -1: skip (ids / graph_ptr that do not fit the store)
  __shared__ int32_t s_off[CL_TILE];   // graph_ptr of its graph
  const int t = threadIdx.x;
  const int n_tiles = (a.N + CL_TILE - 1) / CL_TILE;
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int tile0 = tile * CL_TILE;                     // < N < 2^31 - CL_TILE
    const int rows = min(CL_TILE, a.N - tile0);
    if (t < rows) {
      const int i = tile0 + t;
      int lo = 0, hi = a.G;                               // the last g < G with graph_ptr[g] <= i
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.graph_ptr[mid] <= i) lo = mid; else hi = mid;
      }
      const int32_t off = a.graph_ptr[lo];
      const int64_t id = a.ids[lo];
      int64_t src = -1;
      if (id >= 0 && id < a.R && i >= off) {
        const int64_t r0 = a.rec_ptr[id], r1 = a.rec_ptr[id + 1];
        const int64_t s = r0 + (i - off);
        if (r0 >= 0 && s < r1 && r1 <= a.Ntot) src = s;   // a row outside its record is never read
      }
      s_src[t] = src;
      s_off[t] = off;
      if (src >= 0) {
        a.inv[i] = a.s_inv[src];
        a.w[i] = a.s_w[src];
        const float l0 = a.s_y[src * 3], l1 = a.s_y[src * 3 + 1], l2 = a.s_y[src * 3 + 2];
        a.y0[i] = l0;
        a.names[i] = (int32_t)l1;                         // truncation, as tf.cast / torch .to(int32)
        if (a.y_true) {
          a.y_true[(int64_t)i * 3] = l0;
          a.y_true[(int64_t)i * 3 + 1] = l1;
          a.y_true[(int64_t)i * 3 + 2] = l2;
        }
      }
    }
    __syncthreads();
    if (a.vec_k == 4) {
      const int kq = a.K >> 2;
      cl_copy_lists(reinterpret_cast<const int4*>(a.s_nlist), reinterpret_cast<const float4*>(a.s_edges),
                    reinterpret_cast<int4*>(a.nlist) + (int64_t)tile0 * kq, reinterpret_cast<float4*>(a.edges) + (int64_t)tile0 * kq,
                    s_src, s_off, rows, kq, t);
    } else {
      cl_copy_lists(a.s_nlist, a.s_edges, a.nlist + (int64_t)tile0 * a.K, a.edges + (int64_t)tile0 * a.K, s_src, s_off, rows, a.K,
                    t);
    }
    if (a.vec_c == 4) {
      const int cq = a.C >> 2;
      cl_copy_rows(reinterpret_cast<const float4*>(a.s_atoms), reinterpret_cast<float4*>(a.atoms) + (int64_t)tile0 * cq, s_src, rows,
                   cq, t);
    } else if (a.vec_c == 2) {
      const int cq = a.C >> 1;
      cl_copy_rows(reinterpret_cast<const float2*>(a.s_atoms), reinterpret_cast<float2*>(a.atoms) + (int64_t)tile0 * cq, s_src, rows,
                   cq, t);
    } else {
      cl_copy_rows(a.s_atoms, a.atoms + (int64_t)tile0 * a.C, s_src, rows, a.C, t);
    }
    __syncthreads();                                      // the next trip rewrites the staged rows
  }
}

static bool cl_aligned(const void* p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) == 0; }

}  // namespace ng

using namespace ng;

extern "C" int ng_collate_batch(ng_ctx* ctx, void* stream, int64_t R, int64_t Ntot, const float* s_atoms, const int32_t* s_nlist,
                                const float* s_edges, const float* s_inv_degree, const float* s_y, const float* s_w,
                                const int64_t* rec_ptr, const int32_t* ids, const int32_t* graph_ptr, int64_t N, int K, int C, int G,
                                float* atoms, int32_t* nlist, float* edges, float* inv_degree, float* y0, float* w, int32_t* names,
                                float* y_true) {
  if (!ctx) return NG_ERR_INVALID;
  NG_REQUIRE(ctx, K >= 1 && K <= 4096 && C >= 1 && C <= 4096, "collate: K and C in [1, 4096]");
  NG_REQUIRE(ctx, N >= 0 && N < ((int64_t)1 << 31) - CL_TILE, "collate: N out of range");
  NG_REQUIRE(ctx, G >= 0 && (N == 0 || G >= 1) && G <= N, "collate: G graphs of at least one atom each make up N atoms");
  NG_REQUIRE(ctx, R >= 0 && Ntot >= R && (N == 0 || R >= 1), "collate: a store of R records and Ntot >= R rows");
  if (N == 0) return NG_OK;
  NG_REQUIRE(ctx, s_atoms && s_nlist && s_edges && s_inv_degree && s_y && s_w && rec_ptr, "collate: store arrays");
  NG_REQUIRE(ctx, ids && graph_ptr, "collate: ids / graph_ptr");
  NG_REQUIRE(ctx, atoms && nlist && edges && inv_degree && y0 && w && names, "collate: outputs (y_true alone may be NULL)");
  CollateArgs a;
  a.s_atoms = s_atoms; a.s_nlist = s_nlist; a.s_edges = s_edges; a.s_inv = s_inv_degree; a.s_y = s_y; a.s_w = s_w;
  a.rec_ptr = rec_ptr; a.ids = ids; a.graph_ptr = graph_ptr;
  a.atoms = atoms; a.nlist = nlist; a.edges = edges; a.inv = inv_degree; a.y0 = y0; a.w = w; a.names = names; a.y_true = y_true;
  a.R = R; a.Ntot = Ntot;
  a.N = (int)N; a.K = K; a.C = C; a.G = G;
  a.vec_k = (K % 4 == 0 && cl_aligned(s_nlist, 16) && cl_aligned(s_edges, 16) && cl_aligned(nlist, 16) && cl_aligned(edges, 16)) ? 4 : 1;
  a.vec_c = (C % 4 == 0 && cl_aligned(s_atoms, 16) && cl_aligned(atoms, 16)) ? 4
            : (C % 2 == 0 && cl_aligned(s_atoms, 8) && cl_aligned(atoms, 8)) ? 2 : 1;
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard dg(ctx->device);
  ProfScope ps(ctx, st, "collate_batch");
  const int64_t tiles = cdiv(N, CL_TILE);
  const unsigned grid = (unsigned)(tiles < CL_MAX_BLOCKS ? tiles : CL_MAX_BLOCKS);
  hipLaunchKernelGGL(collate_kernel, dim3(grid), dim3(CL_TILE), 0, st, a);
  NG_HIP(ctx, hipGetLastError());
  return NG_OK;
}
