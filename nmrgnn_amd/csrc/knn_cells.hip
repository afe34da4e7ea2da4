// K nearest neighbours through a uniform cell grid: the neighbour search of ng_knn_graph for LARGE frames
// (nmrgnn/library.py:106-117 -> nmrdata.parse_universe; SURVEY §8(f1) "a cell-list kNN HIP kernel is the natural
// follow-up").  The brute-force kernels of knn.hip visit n candidates per query: fine at protein size (2770 atoms:
// 35 us), 1e10 pair evaluations at 100 k atoms.  Here a query visits the atoms of the cells around it:
//   1. bounding box of the frame; cell edge L = 0.5 (K / density)^(1/3) (two shells of cells then usually settle the K
//      nearest); the grid is clipped to `cap` cells per frame
//   2. counting sort of the atoms by cell (integer atomics, ng_exclusive_scan_i32): sorted (x, y, z, index) records
//   3. one thread per SORTED atom (neighbouring threads sit in the same cell and walk the same ranges): shells of cells
//      r = 0, 1, 2, ... around its cell — a row of cells along x is one contiguous range of records — until the K-th
//      distance found is within r L of the query (everything unvisited is at least that far away) or the grid is exhausted
// Result: EXACTLY the lists of the brute-force kernels — (distance, index) ascending, ties to the lower index, the same
// fp32 distance expression (pbc_dist2) — whatever the grid; tests compare the two bit for bit.
#include <algorithm>

#include "ng_common.h"
#include "ng_internal.h"
#include "nlist_common.cuh"

extern "C" int ng_exclusive_scan_i32(ng_ctx*, void*, int64_t, const int32_t*, int32_t*);

namespace ng {

struct KcGrid {          // per frame
  float ox, oy, oz;      // lower corner
  float inv_l, l;        // 1 / cell edge, cell edge
  int nx, ny, nz;
};

__device__ __forceinline__ int kc_coord(float x, float o, float inv_l, int n) {
  return min(max((int)floorf((x - o) * inv_l), 0), n - 1);
}

// ---- 1. bounding box (KC_BOX_BLOCKS partial boxes per frame), then the grid of every frame -----------------------------
constexpr int KC_BOX_BLOCKS = 64;
constexpr float KC_CELL = 0.50f;

__device__ __forceinline__ void kc_box_reduce(float (&lo)[3], float (&hi)[3], float (*red)[16]) {
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { lo[a] = fminf(lo[a], __shfl_xor(lo[a], o)); hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], o)); }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int a = 0; a < 3; ++a) { red[a][w] = lo[a]; red[3 + a][w] = hi[a]; }
  __syncthreads();
}

__global__ __launch_bounds__(256) void kc_box_kernel(int n, const float* __restrict__ pos, float* __restrict__ boxes) {
  __shared__ float red[6][16];
  const float* fp = pos + (int64_t)blockIdx.y * n * 3;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += KC_BOX_BLOCKS * 256)
#pragma unroll
    for (int a = 0; a < 3; ++a) { const float v = fp[3 * i + a]; lo[a] = fminf(lo[a], v); hi[a] = fmaxf(hi[a], v); }
  kc_box_reduce(lo, hi, red);
  if (threadIdx.x < 6) {
    float v = red[threadIdx.x][0];
    for (int q = 1; q < 4; ++q) v = threadIdx.x < 3 ? fminf(v, red[threadIdx.x][q]) : fmaxf(v, red[threadIdx.x][q]);
    boxes[((int64_t)blockIdx.y * KC_BOX_BLOCKS + blockIdx.x) * 6 + threadIdx.x] = v;
  }
}

__global__ __launch_bounds__(64) void kc_grid_kernel(int n, int K, int cap, const float* __restrict__ boxes, KcGrid* __restrict__ grids) {
  __shared__ float red[6][16];
  const float* b = boxes + ((int64_t)blockIdx.x * KC_BOX_BLOCKS + threadIdx.x) * 6;
  float lo[3] = {b[0], b[1], b[2]}, hi[3] = {b[3], b[4], b[5]};
  kc_box_reduce(lo, hi, red);
  if (threadIdx.x == 0) {
    const float ex = fmaxf(red[3][0] - red[0][0], 1e-3f), ey = fmaxf(red[4][0] - red[1][0], 1e-3f), ez = fmaxf(red[5][0] - red[2][0], 1e-3f);
    // mean density of the box (a protein does not fill its box: the true local density is higher, the cells then hold more
    // atoms than aimed for — slower, never wrong)
    const float rho = (float)n / (ex * ey * ez);
    // cell edge = KC_CELL (K / rho)^(1/3) = 0.8 x the radius of the sphere that holds K atoms at that density: most queries
    // settle after the second shell (125 cells, ~8 K candidates).  Measured per 110,800-atom frame: 0.40 -> 235 us, 0.50 ->
    // 202, 0.60 -> 232, 0.72 (one shell for an interior atom, but a wave of 64 queries always has one that needs two) -> 320
    float l = KC_CELL * cbrtf((float)K / rho);
    int nx, ny, nz;
    for (;;) {
      nx = (int)fminf(ex / l, 4.0e6f) + 1; ny = (int)fminf(ey / l, 4.0e6f) + 1; nz = (int)fminf(ez / l, 4.0e6f) + 1;
      if ((int64_t)nx * ny * nz <= cap) break;
      l *= 1.26f;                                  // a factor of two in cell volume
    }
    KcGrid g;
    g.ox = red[0][0]; g.oy = red[1][0]; g.oz = red[2][0];
    g.l = l; g.inv_l = 1.0f / l;
    g.nx = nx; g.ny = ny; g.nz = nz;
    grids[blockIdx.x] = g;
  }
}

// ---- 2. counting sort by cell ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kc_count_kernel(int n, int cap, const float* __restrict__ pos, const KcGrid* __restrict__ grids,
                                                       int32_t* __restrict__ cell_of, int32_t* __restrict__ count) {
  const int frame = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const KcGrid g = grids[frame];
  const float* p = pos + ((int64_t)frame * n + i) * 3;
  const int cx = kc_coord(p[0], g.ox, g.inv_l, g.nx), cy = kc_coord(p[1], g.oy, g.inv_l, g.ny), cz = kc_coord(p[2], g.oz, g.inv_l, g.nz);
  const int c = (cz * g.ny + cy) * g.nx + cx;
  cell_of[(int64_t)frame * n + i] = c;
  atomicAdd(count + (int64_t)frame * cap + c, 1);
}

// records land in their cell's range in arrival order: the search result does not depend on it (explicit (distance,
// index) order), so the unordered fill is deterministic where it matters
__global__ __launch_bounds__(256) void kc_fill_kernel(int n, int cap, const float* __restrict__ pos, const int32_t* __restrict__ cell_of,
                                                      const int32_t* __restrict__ start, int32_t* __restrict__ cursor,
                                                      float4* __restrict__ rec) {
  const int frame = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t row = (int64_t)frame * n + i;
  const int64_t cell = (int64_t)frame * cap + cell_of[row];
  const int slot = start[cell] + atomicAdd(cursor + cell, 1);
  const float* p = pos + row * 3;
  rec[slot] = make_float4(p[0], p[1], p[2], __builtin_bit_cast(float, i));
}

// ---- 3. the search ------------------------------------------------------------------------------------------------------
// A list entry is ONE 64-bit key (nlist_common.cuh: NG_KNN_KEY), an empty slot KNN_KEY_EMPTY.  The insertion appears once in
// the kernel (one loop over the one or two record ranges of a row of cells): with a copy per call site, and four more for a
// four-deep prefetch, the kernel was instruction-fetch bound (6 us per ROW).
// the candidates of one row of cells — the record ranges [a0, b0) and [a1, b1) — into the query's list, distances through the
// displacement policy D (pbc.cuh); the one call site of each query kernel
template <int KMAX, class Disp>
__device__ __forceinline__ void kc_scan(const Disp& D, float4 q, int i, const float4* __restrict__ rec, int a0, int b0, int a1,
                                        int b1, knn_u64 (&key)[KMAX]) {
  const int len0 = b0 - a0, total = len0 + (b1 - a1);
  for (int u = 0; u < total; ++u) {
    const float4 c = rec[u < len0 ? a0 + u : a1 + (u - len0)];
    float dx, dy, dz;
    D(q.x, q.y, q.z, c.x, c.y, c.z, dx, dy, dz);
    const float d2 = pbc_dist2(dx, dy, dz);
    const unsigned j = __builtin_bit_cast(unsigned, c.w);
    const knn_u64 kk = NG_KNN_KEY(d2, j);
    if (kk < key[KMAX - 1] && (int)j != i) {
#pragma unroll
      for (int k = KMAX - 1; k >= 1; --k) {
        const bool shift = kk < key[k - 1];                 // old element k-1 moves up
        key[k] = shift ? key[k - 1] : (kk < key[k] ? kk : key[k]);
      }
      key[0] = kk < key[0] ? kk : key[0];
    }
  }
}

template <int KMAX>
__global__ __launch_bounds__(256) void kc_query_kernel(int n, int K, int cap, float scale, const KcGrid* __restrict__ grids,
                                                       const int32_t* __restrict__ start, const float4* __restrict__ rec,
                                                       int32_t* __restrict__ nlist, float* __restrict__ edges,
                                                       float* __restrict__ inv_degree) {
  const int frame = blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;      // sorted slot inside the frame
  if (p >= n) return;
  const KcGrid g = grids[frame];
  const float4 q = rec[(int64_t)frame * n + p];
  const int i = __builtin_bit_cast(int, q.w);
  const int cx = kc_coord(q.x, g.ox, g.inv_l, g.nx), cy = kc_coord(q.y, g.oy, g.inv_l, g.ny), cz = kc_coord(q.z, g.oz, g.inv_l, g.nz);
  const int32_t* st = start + (int64_t)frame * cap;
  knn_u64 key[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) key[k] = KNN_KEY_EMPTY;

  const int rmax = max(max(max(cx, g.nx - 1 - cx), max(cy, g.ny - 1 - cy)), max(cz, g.nz - 1 - cz));
  for (int r = 0; r <= rmax; ++r) {
    for (int dz = -r; dz <= r; ++dz) {
      const int z = cz + dz;
      if (z < 0 || z >= g.nz) continue;
      for (int dy = -r; dy <= r; ++dy) {
        const int y = cy + dy;
        if (y < 0 || y >= g.ny) continue;
        const int rowc = (z * g.ny + y) * g.nx;
        // a whole row of the shell (cells cx-r .. cx+r are one range of records), or — an interior row — only its two end cells
        const bool whole = abs(dz) == r || abs(dy) == r;
        const int xl = cx - r, xr = cx + r;
        int a0, b0, a1 = 0, b1 = 0;
        if (whole) {
          a0 = st[rowc + max(xl, 0)]; b0 = st[rowc + min(xr, g.nx - 1) + 1];
        } else {
          a0 = xl >= 0 ? st[rowc + xl] : 0; b0 = xl >= 0 ? st[rowc + xl + 1] : 0;
          a1 = xr < g.nx ? st[rowc + xr] : 0; b1 = xr < g.nx ? st[rowc + xr + 1] : 0;
        }
        kc_scan<KMAX>(DispOpen(), q, i, rec, a0, b0, a1, b1, key);
      }
    }
    // every atom outside the cube of shells 0..r is at least r L from the query (it is at least r whole cells away along
    // some axis; 0.1 % off for the rounding of the cell assignment).  Enough once the K-th distance is inside that.
    const float reach = (float)r * g.l * 0.999f;
    knn_u64 kth = KNN_KEY_EMPTY;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) kth = k == K - 1 ? key[k] : kth;      // (a run-time index would put the list on the stack)
    if (knn_key_d2(kth) <= reach * reach) break;
  }

  NG_KNN_WRITE_KEY_ROW(KMAX, K, key, (int64_t)frame * n + i, frame * n, scale, nlist, edges, inv_degree);
}

// ---- periodic boxes: the grid lives in fractional coordinates ----------------------------------------------------------
// Box (pbc.cuh) a = (ax, 0, 0), b = (bx, by, 0), c = (cx, cy, cz); an atom's cell is floor(n_axis * frac(f_axis)) of its
// fractional coordinates, whatever image the raw position is in.  Per-axis cell counts follow the perpendicular widths
// w_axis of the box (n_axis = w_axis / L, at least 1), so a cell is at least L thick along every axis.  Shells of cells wrap
// modulo the grid; along an axis of n cells a shell reaches at most lo = (n - 1) / 2 cells down and hi = n - 1 - lo up, so
// each cell is visited once even where 2r + 1 exceeds n.  An atom none of whose images lies in shells 0..r is more than
// r cells away along some axis that shell r does not yet cover: at least r * (w_axis / n_axis) away in the minimum image.
struct KpGrid {
  float ax, bx, by, cx, cy, cz;
  float iax, iby, icz;
  float wx, wy, wz;      // perpendicular thickness of one cell along a, b, c
  int nx, ny, nz;
};

__device__ __forceinline__ int kp_axis(float f, int n) {
  f -= floorf(f);
  return min(max((int)(f * (float)n), 0), n - 1);
}

__global__ __launch_bounds__(64) void kp_grid_kernel(int G, int n, int K, int cap, const float* __restrict__ box,
                                                     KpGrid* __restrict__ grids) {
  const int f = blockIdx.x * 64 + threadIdx.x;
  if (f >= G) return;
  const float* b = box + (int64_t)f * 9;
  KpGrid g;
  g.ax = b[0]; g.bx = b[3]; g.by = b[4]; g.cx = b[6]; g.cy = b[7]; g.cz = b[8];
  g.iax = 1.0f / g.ax; g.iby = 1.0f / g.by; g.icz = 1.0f / g.cz;
  const float v = g.ax * g.by * g.cz;
  const float bcx = g.by * g.cz, bcy = -g.bx * g.cz, bcz = g.bx * g.cy - g.by * g.cx;
  const float wa = v / sqrtf(bcx * bcx + bcy * bcy + bcz * bcz), wb = g.by * g.cz / sqrtf(g.cy * g.cy + g.cz * g.cz), wc = g.cz;
  // the cell edge of the open grid at the box's density (a filled box: the density is the true one)
  float l = KC_CELL * cbrtf((float)K * v / (float)n);
  int nx = 1, ny = 1, nz = 1;
  for (int it = 0; it < 256; ++it) {      // bounded: a box the host would refuse (NaN widths) ends as one cell
    nx = max((int)fminf(wa / l, 4.0e6f), 1); ny = max((int)fminf(wb / l, 4.0e6f), 1); nz = max((int)fminf(wc / l, 4.0e6f), 1);
    if ((int64_t)nx * ny * nz <= cap) break;
    nx = ny = nz = 1;
    l *= 1.26f;
  }
  g.nx = nx; g.ny = ny; g.nz = nz;
  g.wx = wa / (float)nx; g.wy = wb / (float)ny; g.wz = wc / (float)nz;
  grids[f] = g;
}

__global__ __launch_bounds__(256) void kp_count_kernel(int n, int cap, const float* __restrict__ pos, const KpGrid* __restrict__ grids,
                                                       int32_t* __restrict__ cell_of, int32_t* __restrict__ count) {
  const int frame = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const KpGrid g = grids[frame];
  const float* p = pos + ((int64_t)frame * n + i) * 3;
  const float fc = p[2] * g.icz;
  const float fb = fmaf(-fc, g.cy, p[1]) * g.iby;
  const float fa = fmaf(-fc, g.cx, fmaf(-fb, g.bx, p[0])) * g.iax;
  const int c = (kp_axis(fc, g.nz) * g.ny + kp_axis(fb, g.ny)) * g.nx + kp_axis(fa, g.nx);
  cell_of[(int64_t)frame * n + i] = c;
  atomicAdd(count + (int64_t)frame * cap + c, 1);
}

__device__ __forceinline__ int kp_wrap(int x, int n) { return x < 0 ? x + n : (x >= n ? x - n : x); }

template <int KMAX, class Disp>
__global__ __launch_bounds__(256) void kp_query_kernel(int n, int K, int cap, float scale, const KpGrid* __restrict__ grids,
                                                       const float* __restrict__ box, const int32_t* __restrict__ cell_of,
                                                       const int32_t* __restrict__ start, const float4* __restrict__ rec,
                                                       int32_t* __restrict__ nlist, float* __restrict__ edges,
                                                       float* __restrict__ inv_degree) {
  const int frame = blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;      // sorted slot inside the frame
  if (p >= n) return;
  const KpGrid g = grids[frame];
  Disp D;
  D.load(box, frame);
  const float4 q = rec[(int64_t)frame * n + p];
  const int i = __builtin_bit_cast(int, q.w);
  const int c = cell_of[(int64_t)frame * n + i];      // the cell the count pass gave the query
  const int cx = c % g.nx, cy = (c / g.nx) % g.ny, cz = c / (g.nx * g.ny);
  const int lox = (g.nx - 1) / 2, hix = g.nx - 1 - lox;
  const int loy = (g.ny - 1) / 2, hiy = g.ny - 1 - loy;
  const int loz = (g.nz - 1) / 2, hiz = g.nz - 1 - loz;
  const int32_t* st = start + (int64_t)frame * cap;
  knn_u64 key[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) key[k] = KNN_KEY_EMPTY;

  const int rmax = max(max(hix, hiy), hiz);
  for (int r = 0; r <= rmax; ++r) {
    const int xl = min(r, lox), xh = min(r, hix);
    for (int dz = -min(r, loz); dz <= min(r, hiz); ++dz) {
      const int z = kp_wrap(cz + dz, g.nz);
      const bool bz = dz == -r || dz == r;
      for (int dy = -min(r, loy); dy <= min(r, hiy); ++dy) {
        const int y = kp_wrap(cy + dy, g.ny);
        const int rowc = (z * g.ny + y) * g.nx;
        int a0 = 0, b0 = 0, a1 = 0, b1 = 0;
        if (bz || dy == -r || dy == r) {
          // a whole row of the shell: cells cx - xl .. cx + xh, one range of records or — wrapped — two
          const int x0 = cx - xl, x1 = cx + xh;
          if (x0 < 0) {
            a0 = st[rowc + x0 + g.nx]; b0 = st[rowc + g.nx]; a1 = st[rowc]; b1 = st[rowc + x1 + 1];
          } else if (x1 >= g.nx) {
            a0 = st[rowc + x0]; b0 = st[rowc + g.nx]; a1 = st[rowc]; b1 = st[rowc + x1 - g.nx + 1];
          } else {
            a0 = st[rowc + x0]; b0 = st[rowc + x1 + 1];
          }
        } else {
          // an interior row: its end cells, on the sides where the axis is not yet exhausted (r >= 1 here: distinct cells)
          if (r <= lox) { const int x = kp_wrap(cx - r, g.nx); a0 = st[rowc + x]; b0 = st[rowc + x + 1]; }
          if (r <= hix) { const int x = kp_wrap(cx + r, g.nx); a1 = st[rowc + x]; b1 = st[rowc + x + 1]; }
        }
        kc_scan<KMAX>(D, q, i, rec, a0, b0, a1, b1, key);
      }
    }
    // the thinnest cell along the axes shell r does not cover yet (0.1 % off for the rounding of the cell assignment)
    float w = INFINITY;
    if (r < hix) w = fminf(w, g.wx);
    if (r < hiy) w = fminf(w, g.wy);
    if (r < hiz) w = fminf(w, g.wz);
    if (w == INFINITY) break;                          // every cell visited
    const float reach = (float)r * w * 0.999f;
    knn_u64 kth = KNN_KEY_EMPTY;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) kth = k == K - 1 ? key[k] : kth;
    if (knn_key_d2(kth) <= reach * reach) break;
  }

  NG_KNN_WRITE_KEY_ROW(KMAX, K, key, (int64_t)frame * n + i, frame * n, scale, nlist, edges, inv_degree);
}

// cells per frame: about n / 4 (the grid kernel shrinks its grid to fit), a power of two in [64, 2^21]
static int kc_cell_cap(int n) {
  int cap = 64;
  while (cap < 4 * (int64_t)n && cap < (1 << 22)) cap <<= 1;
  return cap;
}

bool knn_cells_supported(int G, int n, int K) {
  return K >= 1 && K <= 64 && n >= 64 && (int64_t)G * kc_cell_cap(n) <= ((int64_t)1 << 26);
}

int knn_cells(ng_ctx* ctx, hipStream_t st, int G, int n, int K, float scale, const float* pos, int32_t* nlist, float* edges,
              float* inv_degree, const float* box, int triclinic) {
  const int cap = kc_cell_cap(n);
  const int64_t rows = (int64_t)G * n, cells = (int64_t)G * cap;
  // scratch: records [rows] float4 | cell_of [rows] | count [cells] | start [cells + 1] | grids [G] | partial boxes [G][64][6]
  // (periodic boxes: grids [G] KpGrid, no partial boxes)
  const size_t bytes = (size_t)rows * 16 + (size_t)rows * 4 + (size_t)cells * 4 + (size_t)(cells + 1) * 4 + (size_t)G * (sizeof(KpGrid) + KC_BOX_BLOCKS * 6 * 4) + 256;
  char* ws = (char*)workspace(ctx, bytes);
  if (!ws) return NG_ERR_NOMEM;
  float4* rec = reinterpret_cast<float4*>(ws);
  int32_t* cell_of = reinterpret_cast<int32_t*>(ws + (size_t)rows * 16);
  int32_t* count = cell_of + rows;
  int32_t* start = count + cells;
  KcGrid* grids = reinterpret_cast<KcGrid*>(start + cells + 1 + ((cells + 1) & 1));
  float* boxes = reinterpret_cast<float*>(grids + G);
  KpGrid* pgrids = reinterpret_cast<KpGrid*>(grids);
  const dim3 grid((unsigned)cdiv(n, 256), (unsigned)G), block(256);
  {
    ProfScope ps(ctx, st, "knn_cells_sort");
    NG_HIP(ctx, hipMemsetAsync(count, 0, (size_t)cells * 4, st));
    if (box) {
      hipLaunchKernelGGL(kp_grid_kernel, dim3((unsigned)cdiv(G, 64)), dim3(64), 0, st, G, n, K, cap, box, pgrids);
      hipLaunchKernelGGL(kp_count_kernel, grid, block, 0, st, n, cap, pos, pgrids, cell_of, count);
    } else {
      hipLaunchKernelGGL(kc_box_kernel, dim3(KC_BOX_BLOCKS, (unsigned)G), dim3(256), 0, st, n, pos, boxes);
      hipLaunchKernelGGL(kc_grid_kernel, dim3((unsigned)G), dim3(64), 0, st, n, K, cap, boxes, grids);
      hipLaunchKernelGGL(kc_count_kernel, grid, block, 0, st, n, cap, pos, grids, cell_of, count);
    }
    NG_HIP(ctx, hipGetLastError());
    const int rc = ng_exclusive_scan_i32(ctx, st, cells, count, start);
    if (rc) return rc;
    NG_HIP(ctx, hipMemsetAsync(count, 0, (size_t)cells * 4, st));      // now the fill cursors
    hipLaunchKernelGGL(kc_fill_kernel, grid, block, 0, st, n, cap, pos, cell_of, start, count, rec);
    NG_HIP(ctx, hipGetLastError());
  }
  ProfScope ps(ctx, st, "knn_cells_query");
#define NG_KP_TRIC(KM) hipLaunchKernelGGL((kp_query_kernel<KM, DispTric>), grid, block, 0, st, n, K, cap, scale, pgrids, box, \
                                          cell_of, start, rec, nlist, edges, inv_degree)
#define NG_KP_ORTHO(KM) hipLaunchKernelGGL((kp_query_kernel<KM, DispOrtho>), grid, block, 0, st, n, K, cap, scale, pgrids, box, \
                                           cell_of, start, rec, nlist, edges, inv_degree)
#define NG_KC(KM) hipLaunchKernelGGL(kc_query_kernel<KM>, grid, block, 0, st, n, K, cap, scale, grids, start, rec, nlist, edges, \
                                     inv_degree)
  if (box && triclinic) NG_KNN_LADDER(K, NG_KP_TRIC);
  else if (box) NG_KNN_LADDER(K, NG_KP_ORTHO);
  else NG_KNN_LADDER(K, NG_KC);
#undef NG_KP_TRIC
#undef NG_KP_ORTHO
#undef NG_KC
  NG_HIP(ctx, hipGetLastError());
  return NG_OK;
}

}  // namespace ng
