// Distance-cutoff neighbour lists in CSR form, for G frames of one topology (the ragged form: ragged.hip); mp_csr.hip runs
// message passing over them.
#include "ng_common.h"
#include "ng_internal.h"
#include "nlist_common.cuh"

namespace ng {

// Distance-cutoff graphs (BASELINE configs[4] "variable degree"): every OTHER atom of the same frame closer than
// `cutoff` (Angstrom) is a neighbour; rows are written in ascending neighbour index ("CSR-sorted": consecutive
// entries gather consecutive rows).  Two passes over LDS-tiled positions, one thread per query atom:
//   count:  deg[row]                               -> the caller's exclusive scan gives row_ptr
//   fill :  col (batch-global), dist*scale, inv_degree = 1/#(local neighbour index > 0)  (library.py:115-116)
// The count and the fill pass — and the one-thread, 16-lane and wave forms — must agree bit for bit on `d2 < cutoff2`, because
// rows are sized by the count and then filled: all take the squared distance from pbc_dist2 (nlist_common.cuh).
constexpr int CUT_TILE = NL_TILE;

template <bool FILL, class Disp>
__global__ __launch_bounds__(256) void cutoff_kernel(int n, float cutoff2, float scale, const float* __restrict__ pos,
                                                     int32_t* __restrict__ deg, const int32_t* __restrict__ row_ptr,
                                                     int32_t* __restrict__ col, float* __restrict__ dist,
                                                     float* __restrict__ inv_degree, int32_t* __restrict__ row_of,
    const float* __restrict__ box) {
  __shared__ float sx[CUT_TILE], sy[CUT_TILE], sz[CUT_TILE];
  const int frame = blockIdx.y;
  Disp D;
  D.load(box, frame);
  const int i = blockIdx.x * 256 + threadIdx.x;
  const float* fp = pos + (int64_t)frame * n * 3;
  float qx = 0.f, qy = 0.f, qz = 0.f;
  if (i < n) { qx = fp[3 * i]; qy = fp[3 * i + 1]; qz = fp[3 * i + 2]; }
  const int64_t row = (int64_t)frame * n + i;
  int cnt = 0, cnt_pos = 0;
  int64_t out = 0, lim = 0;          // a row never writes past its own extent, whatever the count pass saw
  if (FILL && i < n) { out = row_ptr[row]; lim = row_ptr[row + 1]; }
  for (int t0 = 0; t0 < n; t0 += CUT_TILE) {
    const int m = min(CUT_TILE, n - t0);
    NG_NL_STAGE(sx, sy, sz, fp, t0, m);
    if (i < n) {
      for (int t = 0; t < m; ++t) {
        float dx, dy, dz;
        D(qx, qy, qz, sx[t], sy[t], sz[t], dx, dy, dz);
        const float d2 = pbc_dist2(dx, dy, dz);
        const int j = t0 + t;
        NG_CUTOFF_HIT(FILL, d2, j, i, frame * n, 0, (int32_t)row, cutoff2, scale, out, lim, col, dist, row_of, cnt, cnt_pos);
      }
    }
  }
  if (i >= n) return;
  if (FILL) inv_degree[row] = cnt_pos > 0 ? 1.0f / (float)cnt_pos : 0.f;
  else deg[row] = cnt;
}

// The same with 16 lanes per query atom (round 3): lane s of an atom's group tests candidates s, s + 16, ..; a wave
// ballot per 16-candidate chunk gives the hits in ascending candidate order, so rows come out exactly as the
// one-thread-per-atom kernel writes them.  One thread per atom left a 2770-atom frame with 11 workgroups walking 2770
// candidates each, its hits stored one by one: 80 us (count) + 295 us (fill) per frame; this form: 256 threads = 16 atoms.
template <bool FILL, class Disp>
__global__ __launch_bounds__(256) void cutoff_s16_kernel(int n, float cutoff2, float scale, const float* __restrict__ pos,
                                                         int32_t* __restrict__ deg, const int32_t* __restrict__ row_ptr,
                                                         int32_t* __restrict__ col, float* __restrict__ dist,
                                                         float* __restrict__ inv_degree, int32_t* __restrict__ row_of,
    const float* __restrict__ box) {
  __shared__ float sx[CUT_TILE], sy[CUT_TILE], sz[CUT_TILE];
  const int frame = blockIdx.y;
  Disp D;
  D.load(box, frame);
  const int s = threadIdx.x & 15, grp = (threadIdx.x & 63) >> 4;
  const int i = blockIdx.x * 16 + (threadIdx.x >> 4);
  const float* fp = pos + (int64_t)frame * n * 3;
  const int ic = i < n ? i : n - 1;
  const float qx = fp[3 * ic], qy = fp[3 * ic + 1], qz = fp[3 * ic + 2];
  const int64_t row = (int64_t)frame * n + i;
  int cnt = 0, cnt_pos = 0;
  int64_t out = 0, lim = 0;          // a row never writes past its own extent, whatever the count pass saw
  if (FILL && i < n) { out = row_ptr[row]; lim = row_ptr[row + 1]; }
  for (int t0 = 0; t0 < n; t0 += CUT_TILE) {
    const int m = min(CUT_TILE, n - t0);
    NG_NL_STAGE(sx, sy, sz, fp, t0, m);
    for (int c0 = 0; c0 < m; c0 += 64) {          // wave-uniform trip count: every lane takes part in the ballots
      // four 16-candidate chunks per trip: their LDS reads are in flight together (a ballot per chunk in a plain loop
      // serialises on the LDS latency of each)
      bool hit[4];
      float d2[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int t = c0 + 16 * u + s;
        hit[u] = false;
        d2[u] = 0.f;
        if (t < m && i < n) {
          float dx, dy, dz;
          D(qx, qy, qz, sx[t], sy[t], sz[t], dx, dy, dz);
          d2[u] = pbc_dist2(dx, dy, dz);
          hit[u] = d2[u] < cutoff2 && t0 + t != i;
        }
      }
      if (!FILL) {        // counting needs no order: per-lane tallies, summed over the 16 lanes at the end
#pragma unroll
        for (int u = 0; u < 4; ++u) cnt += hit[u] ? 1 : 0;
        continue;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = t0 + c0 + 16 * u + s;
        const unsigned long long b = __ballot(hit[u]);
        const unsigned mine = (unsigned)(b >> (16 * grp)) & 0xFFFFu;
        const int p = cnt + __popc(mine & ((1u << s) - 1u));
        if (FILL && hit[u] && out + p < lim) {
          col[out + p] = frame * n + j;
          dist[out + p] = sqrtf(d2[u]) * scale;
          if (row_of) row_of[out + p] = (int32_t)row;
        }
        cnt += __popc(mine);
        // local neighbour index > 0 (library.py:115-116): candidate 0 of the frame does not count
        cnt_pos += __popc(t0 + c0 + 16 * u == 0 ? (mine & ~1u) : mine);
      }
    }
  }
  if (!FILL) {
    cnt += __shfl_xor(cnt, 1, 64); cnt += __shfl_xor(cnt, 2, 64); cnt += __shfl_xor(cnt, 4, 64); cnt += __shfl_xor(cnt, 8, 64);
  }
  if (i >= n || s != 0) return;
  if (FILL) inv_degree[row] = cnt_pos > 0 ? 1.0f / (float)cnt_pos : 0.f;
  else deg[row] = cnt;
}

// One WAVE per query atom, for molecule-sized calls (round 4; the counterpart of knn.hip: knn_wave_kernel): the 64 lanes test 64
// candidates per step, a ballot gives the hits in ascending candidate order — the order of the other cutoff kernels, same
// distance expression, so the rows are the same bit for bit — and the frame's positions are staged in LDS once per workgroup
// (n <= 4096).  A 2770-atom frame: count 27-38 us + fill 36 us (16 lanes per atom) -> a few us each.
constexpr int CUT_WAVE_MAXN = 4096;
template <bool FILL, class Disp>
__global__ __launch_bounds__(256) void cutoff_wave_kernel(int n, float cutoff2, float scale, const float* __restrict__ pos,
                                                          int32_t* __restrict__ deg, const int32_t* __restrict__ row_ptr,
                                                          int32_t* __restrict__ col, float* __restrict__ dist,
                                                          float* __restrict__ inv_degree, int32_t* __restrict__ row_of,
    const float* __restrict__ box) {
  extern __shared__ float cw_pos[];               // [3][n]
  float* sx = cw_pos; float* sy = cw_pos + n; float* sz = cw_pos + 2 * n;
  const int frame = blockIdx.y;
  Disp D;
  D.load(box, frame);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const float* fp = pos + (int64_t)frame * n * 3;
  for (int t = threadIdx.x; t < n; t += 256) { sx[t] = fp[3 * t]; sy[t] = fp[3 * t + 1]; sz[t] = fp[3 * t + 2]; }
  __syncthreads();
  const int i = blockIdx.x * 4 + wave;
  if (i >= n) return;                             // uniform over the wave
  const float qx = sx[i], qy = sy[i], qz = sz[i];
  const int64_t row = (int64_t)frame * n + i;
  int64_t out = 0, lim = 0;
  if (FILL) { out = row_ptr[row]; lim = row_ptr[row + 1]; }
  int cnt = 0, cnt_pos = 0;
  for (int tb = 0; tb < n; tb += 64) {
    const int t = tb + lane;
    const int tc = min(t, n - 1);
    float dx, dy, dz;
    D(qx, qy, qz, sx[tc], sy[tc], sz[tc], dx, dy, dz);
    const float d2 = pbc_dist2(dx, dy, dz);
    const bool hit = t < n && t != i && d2 < cutoff2;
    const unsigned long long m = __ballot(hit);
    if (FILL && hit) {
      const int64_t p = out + cnt + __popcll(m & ((1ull << lane) - 1ull));
      if (p < lim) {                              // a row never writes past its own extent
        col[p] = frame * n + t;
        dist[p] = sqrtf(d2) * scale;
        if (row_of) row_of[p] = (int32_t)row;
      }
    }
    cnt += __popcll(m);
    cnt_pos += __popcll(tb == 0 ? (m & ~1ull) : m);      // local neighbour index > 0 (library.py:115-116)
  }
  if (lane != 0) return;
  if (FILL) inv_degree[row] = cnt_pos > 0 ? 1.0f / (float)cnt_pos : 0.f;
  else deg[row] = cnt;
}

}  // namespace ng

using namespace ng;

// count (FILL = false) or fill pass of one displacement policy; the kernel choice of both passes is the same, so that they
// agree on every `d2 < cutoff2`
template <bool FILL, class Disp>
static int cutoff_launch(ng_ctx* ctx, hipStream_t st, int G, int n, float cutoff, float scale, const float* pos, const float* box,
                         int32_t* deg, const int32_t* row_ptr, int32_t* col, float* dist, float* inv_degree, int32_t* row_of) {
  NG_REQUIRE(ctx, G >= 0 && n >= 0 && cutoff > 0.f, "cutoff graph: sizes >= 0, cutoff > 0");
  NG_REQUIRE(ctx, (int64_t)G * n < (int64_t)1 << 31 && G <= 65535, "cutoff graph: batch too large");
  if (G == 0 || n == 0) return NG_OK;
  NG_REQUIRE(ctx, !Disp::periodic || box, "cutoff graph (pbc): box required");
  ProfScope ps(ctx, st, FILL ? "cutoff_fill" : "cutoff_count");
  if (!sw().knn_serial && !sw().knn_lanes && n <= CUT_WAVE_MAXN && (int64_t)G * n <= 16384)      // molecule-sized: one wave per atom
    hipLaunchKernelGGL((cutoff_wave_kernel<FILL, Disp>), dim3((unsigned)cdiv(n, 4), (unsigned)G), dim3(256), (size_t)3 * n * 4,
                       st, n, cutoff * cutoff, scale, pos, deg, row_ptr, col, dist, inv_degree, row_of, box);
  else if (sw().knn_serial)
    hipLaunchKernelGGL((cutoff_kernel<FILL, Disp>), dim3((unsigned)cdiv(n, 256), (unsigned)G), dim3(256), 0,
                       st, n, cutoff * cutoff, scale, pos, deg, row_ptr, col, dist, inv_degree, row_of, box);
  else
    hipLaunchKernelGGL((cutoff_s16_kernel<FILL, Disp>), dim3((unsigned)cdiv(n, 16), (unsigned)G), dim3(256), 0,
                       st, n, cutoff * cutoff, scale, pos, deg, row_ptr, col, dist, inv_degree, row_of, box);
  NG_HIP(ctx, hipGetLastError());
  return NG_OK;
}

extern "C" int ng_cutoff_count(ng_ctx* ctx, void* stream, int G, int n, float cutoff, const float* pos,
                               int32_t* deg) {
  if (!ctx) return NG_ERR_INVALID;
  return cutoff_launch<false, DispOpen>(ctx, (hipStream_t)stream, G, n, cutoff, 1.0f, pos, nullptr, deg, nullptr, nullptr,
                                        nullptr, nullptr, nullptr);
}

extern "C" int ng_cutoff_fill_rows(ng_ctx* ctx, void* stream, int G, int n, float cutoff, float scale, const float* pos,
                                   const int32_t* row_ptr, int32_t* col, float* dist, float* inv_degree, int32_t* row_of);
extern "C" int ng_cutoff_fill(ng_ctx* ctx, void* stream, int G, int n, float cutoff, float scale, const float* pos,
                              const int32_t* row_ptr, int32_t* col, float* dist, float* inv_degree) {
  return ng_cutoff_fill_rows(ctx, stream, G, n, cutoff, scale, pos, row_ptr, col, dist, inv_degree, nullptr);
}

// the same, also writing row_of[nnz] (the row of every entry: what the CSR backward walks) when it is not NULL
extern "C" int ng_cutoff_fill_rows(ng_ctx* ctx, void* stream, int G, int n, float cutoff, float scale, const float* pos,
                                   const int32_t* row_ptr, int32_t* col, float* dist, float* inv_degree, int32_t* row_of) {
  if (!ctx) return NG_ERR_INVALID;
  return cutoff_launch<true, DispOpen>(ctx, (hipStream_t)stream, G, n, cutoff, scale, pos, nullptr, nullptr, row_ptr, col, dist,
                                       inv_degree, row_of);
}

// periodic boxes: box [G][9] lower-triangular lattice vectors on the device (pbc.cuh), triclinic = 0 orthorhombic / 1 reduced;
// the caller keeps cutoff below half the smallest perpendicular width of every box
extern "C" int ng_cutoff_count_pbc(ng_ctx* ctx, void* stream, int G, int n, float cutoff, const float* pos, const float* box,
                                   int triclinic, int32_t* deg) {
  if (!ctx) return NG_ERR_INVALID;
  NG_REQUIRE(ctx, triclinic == 0 || triclinic == 1, "cutoff graph (pbc): triclinic flag 0 or 1");
  hipStream_t st = (hipStream_t)stream;
  return triclinic ? cutoff_launch<false, DispTric>(ctx, st, G, n, cutoff, 1.0f, pos, box, deg, nullptr, nullptr, nullptr, nullptr, nullptr)
                   : cutoff_launch<false, DispOrtho>(ctx, st, G, n, cutoff, 1.0f, pos, box, deg, nullptr, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int ng_cutoff_fill_rows_pbc(ng_ctx* ctx, void* stream, int G, int n, float cutoff, float scale, const float* pos,
                                       const float* box, int triclinic, const int32_t* row_ptr, int32_t* col, float* dist,
                                       float* inv_degree, int32_t* row_of) {
  if (!ctx) return NG_ERR_INVALID;
  NG_REQUIRE(ctx, triclinic == 0 || triclinic == 1, "cutoff graph (pbc): triclinic flag 0 or 1");
  hipStream_t st = (hipStream_t)stream;
  return triclinic ? cutoff_launch<true, DispTric>(ctx, st, G, n, cutoff, scale, pos, box, nullptr, row_ptr, col, dist, inv_degree, row_of)
                   : cutoff_launch<true, DispOrtho>(ctx, st, G, n, cutoff, scale, pos, box, nullptr, row_ptr, col, dist, inv_degree, row_of);
}
