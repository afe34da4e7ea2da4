// Box gradients of a function of the edges: the strain derivative (the virial's negative) and dE/d(lattice vectors).
//
// For a live edge e = (i -> j) of frame g, u_e = D(r_i, r_j) is the displacement the list builders computed (pbc.cuh, the
// same policy call as pg_term in input_grad.hip), l_e = |u_e|, p_e = dd_e * scale * u_e / l_e = dE/du_e, and n_e the integer
// image triple with u_e = (r_j - r_i) + n_e h_g (h_g: rows a, b, c, lower triangular).  Per frame, in float64:
//   S_g = sum_e u_e (x) p_e     (symmetric: dE/d(eps) of r -> r (I + eps), h -> h (I + eps) at fixed lists and images)
//   B_g = sum_e n_e (x) p_e     (dE/dh at fixed Cartesian positions; zero under open boundaries)
// n_e is recovered from the builder's float displacement, not searched for again: delta = u_e - (r_j - r_i) in float64
// (exact), then rounded against c, b, a in turn on the triangular matrix.
//
// Two launches, no atomics, bitwise deterministic (cdna_hip_programming.md, Guideline 12: a store pass plus a
// per-destination sum pass):
//   stage 1  workgroup c owns rows [c*BG_ROWS, (c+1)*BG_ROWS); each thread sums its row's slots in slot order (15 doubles:
//            6 of S, 9 of B), and a segmented scan over the workgroup's rows (segments = frames, found by binary search of
//            graph_ptr) gives each frame's sum over the chunk.  A frame that lies strictly inside the chunk is final and
//            written out; the chunk's first frame and its last one (when different) go to partial[c][0] / partial[c][1].
//   stage 2  one wave per frame: the lane-strided sum of that frame's chunk partials in chunk order, then a butterfly.
//            Frames stage 1 finished are left alone; empty frames get zeros.
// Both stages stay parallel for one 443 k-atom frame (1732 chunks, 64 lanes) and for 4096 small molecules (4096 waves).
#include <algorithm>

#include "ng_common.h"
#include "pbc.cuh"

namespace ng {

constexpr int BG_ROWS = 256;   // rows per stage-1 chunk (= threads of its workgroup)
constexpr int BG_S = 6;        // xx yy zz xy xz yz
constexpr int BG_V = 15;       // 6 of S, 9 of B (row-major n_a p_b)
// the policy of a launch: the public triclinic flag (-1 open, 0 orthorhombic, 1 triclinic: one for the whole batch), or every
// frame by its own kind [G] (the ragged entry points; never a value a caller passes)
constexpr int BG_OPEN = -1, BG_TRIC = 1, BG_PER_FRAME = 2;      // 0: orthorhombic

// the frame of row i: the g with gp[g] <= i < gp[g + 1] (empty frames skipped), clamped to [0, G) (ragged.hip: rg_range)
__device__ __forceinline__ int bg_frame(const int32_t* __restrict__ gp, int G, int64_t i) {
  int a = 0, b = G;
  while (b - a > 1) {
    const int m = (a + b) >> 1;
    if (gp[m] <= i) a = m; else b = m;
  }
  return a;
}

// the image triple of a displacement: delta = u - (r_j - r_i) = n h, solved on the triangular matrix (z, then y, then x)
__device__ __forceinline__ void bg_image(const DispOrtho& D, double dx, double dy, double dz, double& nx, double& ny,
                                         double& nz) {
  nx = rint(dx / (double)D.lx);
  ny = rint(dy / (double)D.ly);
  nz = rint(dz / (double)D.lz);
}
__device__ __forceinline__ void bg_image(const DispTric& D, double dx, double dy, double dz, double& nx, double& ny,
                                         double& nz) {
  nz = rint(dz / (double)D.cz);
  dx -= nz * (double)D.cx;
  dy -= nz * (double)D.cy;
  ny = rint(dy / (double)D.by);
  dx -= ny * (double)D.bx;
  nx = rint(dx / (double)D.ax);
}
__device__ __forceinline__ void bg_image(const DispOpen&, double, double, double, double& nx, double& ny, double& nz) {
  nx = ny = nz = 0.0;
}
// a structure of a ragged batch: by its own kind (an open structure has no images, so its B stays zero)
__device__ __forceinline__ void bg_image(const DispPer& D, double dx, double dy, double dz, double& nx, double& ny,
                                         double& nz) {
  if (D.kind == 0) bg_image(D.O, dx, dy, dz, nx, ny, nz);
  else if (D.kind == 1) bg_image(D.T, dx, dy, dz, nx, ny, nz);
  else nx = ny = nz = 0.0;
}

// one frame's S [9] (symmetric, from the 6) and B [9]; dvec may be NULL; open boundaries write B = 0
template <bool PERIODIC>
__device__ __forceinline__ void bg_store(const double* v, int64_t g, double* __restrict__ strain, double* __restrict__ dvec) {
  double* s = strain + g * 9;
  s[0] = v[0]; s[1] = v[3]; s[2] = v[4];
  s[3] = v[3]; s[4] = v[1]; s[5] = v[5];
  s[6] = v[4]; s[7] = v[5]; s[8] = v[2];
  if (dvec)
    for (int k = 0; k < 9; ++k) dvec[g * 9 + k] = PERIODIC ? v[BG_S + k] : 0.0;
}

// row_ptr == NULL: padded lists (slots i*K .. i*K+K-1, live when edges > 0); otherwise CSR (row_ptr[i] .. row_ptr[i+1]).
// kind [G]: the boundary kind of every frame, read by DispPer alone (NULL otherwise)
template <class Disp>
__global__ __launch_bounds__(BG_ROWS) void box_grad_chunk_kernel(int64_t N, int K, const float* __restrict__ pos,
                                                                 const int32_t* __restrict__ row_ptr,
                                                                 const int32_t* __restrict__ col,
                                                                 const float* __restrict__ edges, const float* __restrict__ dd,
                                                                 float scale, int G, const int32_t* __restrict__ gp,
                                                                 const float* __restrict__ box, double* __restrict__ partial,
                                                                 double* __restrict__ strain, double* __restrict__ dvec,
                                                                 const int32_t* __restrict__ kind) {
  constexpr int NV = Disp::periodic ? BG_V : BG_S;
  __shared__ double sv[NV][BG_ROWS];
  __shared__ int fr[BG_ROWS];
  const int t = threadIdx.x;
  const int64_t c0 = (int64_t)blockIdx.x * BG_ROWS;
  const int nrows = (int)std::min<int64_t>(BG_ROWS, N - c0);
  const int64_t i = c0 + t;
  const bool active = t < nrows;
  double v[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = 0.0;
  int f = -1;
  if (active) {
    f = bg_frame(gp, G, i);
    Disp D;
    if (Disp::periodic) disp_load(D, box, kind, f);
    const float qx = pos[3 * i], qy = pos[3 * i + 1], qz = pos[3 * i + 2];
    const int64_t s0 = row_ptr ? row_ptr[i] : i * K, s1 = row_ptr ? row_ptr[i + 1] : i * K + K;
    for (int64_t s = s0; s < s1; ++s) {
      const float ge = dd[s];
      if (ge == 0.f || (edges && !(edges[s] > 0.f))) continue;
      const int64_t j = col[s];
      const float px = pos[3 * j], py = pos[3 * j + 1], pz = pos[3 * j + 2];
      float ux, uy, uz;
      D(qx, qy, qz, px, py, pz, ux, uy, uz);
      const double x = ux, y = uy, z = uz;
      const double len = sqrt(x * x + y * y + z * z);
      const double w = len > 0.0 ? (double)ge * (double)scale / len : 0.0;   // p = w u; a slot of length zero adds nothing
      const double wx = w * x, wy = w * y, wz = w * z;
      v[0] += x * wx; v[1] += y * wy; v[2] += z * wz;
      v[3] += x * wy; v[4] += x * wz; v[5] += y * wz;
      if (Disp::periodic) {
        double nx, ny, nz;
        bg_image(D, x - ((double)px - (double)qx), y - ((double)py - (double)qy), z - ((double)pz - (double)qz), nx, ny, nz);
        v[6] += nx * wx; v[7] += nx * wy; v[8] += nx * wz;
        v[9] += ny * wx; v[10] += ny * wy; v[11] += ny * wz;
        v[12] += nz * wx; v[13] += nz * wy; v[14] += nz * wz;
      }
    }
  }
  // segmented inclusive scan over the chunk's rows (Hillis-Steele; a segment = one frame's rows, contiguous)
  fr[t] = f;
#pragma unroll
  for (int k = 0; k < NV; ++k) sv[k][t] = v[k];
  __syncthreads();
  for (int off = 1; off < BG_ROWS; off <<= 1) {
    const bool take = active && t >= off && fr[t - off] == f;
    double add[NV];
    if (take) {
#pragma unroll
      for (int k = 0; k < NV; ++k) add[k] = sv[k][t - off];
    }
    __syncthreads();
    if (take) {
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        v[k] += add[k];
        sv[k][t] = v[k];
      }
    }
    __syncthreads();
  }
  if (!active || (t + 1 < nrows && fr[t + 1] == f)) return;   // only the last row of each frame's segment goes on
  const int first = fr[0], last = fr[nrows - 1];
  if (f == first || f == last) {
    double* p = partial + ((int64_t)blockIdx.x * 2 + (f == first ? 0 : 1)) * BG_V;
#pragma unroll
    for (int k = 0; k < NV; ++k) p[k] = v[k];
  } else {
    bg_store<Disp::periodic>(v, f, strain, dvec);
  }
}

// one wave per frame: the frames stage 1 left in chunk partials (or that are empty)
template <bool PERIODIC>
__global__ __launch_bounds__(256) void box_grad_frame_kernel(int64_t N, int G, const int32_t* __restrict__ gp,
                                                             const double* __restrict__ partial, double* __restrict__ strain,
                                                             double* __restrict__ dvec) {
  constexpr int NV = PERIODIC ? BG_V : BG_S;
  const int lane = threadIdx.x & 63;
  const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= G) return;
  const int64_t lo = std::min<int64_t>(std::max(gp[g], 0), N), hi = std::min<int64_t>(std::max<int64_t>(gp[g + 1], lo), N);
  double v[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = 0.0;
  if (hi > lo) {
    const int64_t cf = lo / BG_ROWS, cl = (hi - 1) / BG_ROWS;
    const int64_t end = std::min<int64_t>(N, (cl + 1) * BG_ROWS);
    if (cf == cl && lo > cf * BG_ROWS && hi < end) return;   // strictly inside one chunk: stage 1 wrote it
    for (int64_t c = cf + lane; c <= cl; c += 64) {
      const double* p = partial + (c * 2 + (lo <= c * BG_ROWS ? 0 : 1)) * BG_V;
#pragma unroll
      for (int k = 0; k < NV; ++k) v[k] += p[k];
    }
#pragma unroll
    for (int k = 0; k < NV; ++k)
      for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off, 64);
  }
  if (lane == 0) bg_store<PERIODIC>(v, g, strain, dvec);
}

}  // namespace ng

using namespace ng;

static int box_grad_common(ng_ctx* ctx, void* stream, int64_t N, int K, const float* pos, const int32_t* row_ptr,
                           const int32_t* col, const float* edges, const float* dd, float scale, int G,
                           const int32_t* graph_ptr, const float* box, int policy, const int32_t* kind, double* strain,
                           double* dvec) {
  NG_REQUIRE(ctx, N >= 0 && N < ((int64_t)1 << 31), "box_grad: atom count below 2^31");
  NG_REQUIRE(ctx, G >= 0, "box_grad: frame count G >= 0");
  NG_REQUIRE(ctx, N == 0 || G >= 1, "box_grad: atoms need at least one frame");
  if (G == 0) return NG_OK;
  NG_REQUIRE(ctx, graph_ptr && strain, "box_grad: graph_ptr and strain required");
  NG_REQUIRE(ctx, policy == BG_OPEN || box, "box_grad (pbc): box required");
  NG_REQUIRE(ctx, policy != BG_PER_FRAME || kind, "box_grad (ragged): kind required");
  NG_REQUIRE(ctx, N == 0 || (pos && col && dd), "box_grad: arguments");
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard dg(ctx->device);
  const int64_t nchunks = cdiv(N, BG_ROWS);
  double* partial = (double*)workspace(ctx, (size_t)std::max<int64_t>(nchunks, 1) * 2 * BG_V * sizeof(double));
  if (!partial) return NG_ERR_NOMEM;
  ProfScope ps(ctx, st, "box_grad");
  const dim3 block(BG_ROWS), grid2((unsigned)cdiv(G, 4));
#define NG_BG(Disp)                                                                                                         \
  do {                                                                                                                      \
    if (nchunks > 0)                                                                                                        \
      hipLaunchKernelGGL(box_grad_chunk_kernel<Disp>, dim3((unsigned)nchunks), block, 0, st, N, K, pos, row_ptr, col, edges, \
                         dd, scale, G, graph_ptr, box, partial, strain, dvec, kind);                                        \
    hipLaunchKernelGGL(box_grad_frame_kernel<Disp::periodic>, grid2, block, 0, st, N, G, graph_ptr, partial, strain, dvec); \
  } while (0)
  if (policy == BG_OPEN) NG_BG(DispOpen);
  else if (policy == BG_PER_FRAME) NG_BG(DispPer);
  else if (policy == BG_TRIC) NG_BG(DispTric);
  else NG_BG(DispOrtho);
#undef NG_BG
  NG_HIP(ctx, hipGetLastError());
  return NG_OK;
}

extern "C" int ng_box_grad(ng_ctx* ctx, void* stream, int64_t N, int K, const float* pos, const int32_t* nlist,
                           const float* edges, const float* dd, float scale, int G, const int32_t* graph_ptr, const float* box,
                           int triclinic, double* strain, double* dvec) {
  if (!ctx) return NG_ERR_INVALID;
  NG_REQUIRE(ctx, K >= 1 && N * K < ((int64_t)1 << 31), "box_grad: K >= 1, N * K below 2^31");
  NG_REQUIRE(ctx, N == 0 || edges, "box_grad: edges required (dead slots)");
  NG_REQUIRE(ctx, triclinic >= -1 && triclinic <= 1, "box_grad: triclinic flag -1 (open), 0 or 1");
  return box_grad_common(ctx, stream, N, K, pos, nullptr, nlist, edges, dd, scale, G, graph_ptr, box, triclinic, nullptr, strain,
                         dvec);
}

extern "C" int ng_box_grad_csr(ng_ctx* ctx, void* stream, int64_t N, int64_t nnz, const float* pos, const int32_t* row_ptr,
                               const int32_t* col, const float* dd, float scale, int G, const int32_t* graph_ptr,
                               const float* box, int triclinic, double* strain, double* dvec) {
  if (!ctx) return NG_ERR_INVALID;
  NG_REQUIRE(ctx, nnz >= 0 && nnz < ((int64_t)1 << 31), "box_grad_csr: nnz below 2^31");
  NG_REQUIRE(ctx, N == 0 || row_ptr, "box_grad_csr: row_ptr required");
  NG_REQUIRE(ctx, triclinic >= -1 && triclinic <= 1, "box_grad: triclinic flag -1 (open), 0 or 1");
  return box_grad_common(ctx, stream, N, 0, pos, row_ptr, col, nullptr, dd, scale, G, graph_ptr, box, triclinic, nullptr, strain,
                         dvec);
}

// ragged batches in boxes: every frame with a kind of its own, kind [G] (-1 open, 0 orthorhombic, 1 reduced triclinic) on the
// device next to box [G][9]; kind_host: the kinds in host memory, checked when given (may be NULL).  dvec of an open frame is 0
static int box_grad_ragged_check(ng_ctx* ctx, int G, const float* box, const int32_t* kind, const int32_t* kind_host) {
  NG_REQUIRE(ctx, G <= 0 || (box && kind), "box_grad (ragged): box and kind required");
  if (kind_host)
    for (int g = 0; g < G; ++g)
      NG_REQUIRE(ctx, kind_host[g] >= -1 && kind_host[g] <= 1, "box_grad (ragged): kind -1 (open), 0 or 1");
  return NG_OK;
}

extern "C" int ng_box_grad_ragged(ng_ctx* ctx, void* stream, int64_t N, int K, const float* pos, const int32_t* nlist,
                                  const float* edges, const float* dd, float scale, int G, const int32_t* graph_ptr,
                                  const float* box, const int32_t* kind, const int32_t* kind_host, double* strain,
                                  double* dvec) {
  if (!ctx) return NG_ERR_INVALID;
  NG_REQUIRE(ctx, K >= 1 && N * K < ((int64_t)1 << 31), "box_grad: K >= 1, N * K below 2^31");
  NG_REQUIRE(ctx, N == 0 || edges, "box_grad: edges required (dead slots)");
  if (const int rc = box_grad_ragged_check(ctx, G, box, kind, kind_host)) return rc;
  return box_grad_common(ctx, stream, N, K, pos, nullptr, nlist, edges, dd, scale, G, graph_ptr, box, BG_PER_FRAME, kind, strain,
                         dvec);
}

extern "C" int ng_box_grad_csr_ragged(ng_ctx* ctx, void* stream, int64_t N, int64_t nnz, const float* pos,
                                      const int32_t* row_ptr, const int32_t* col, const float* dd, float scale, int G,
                                      const int32_t* graph_ptr, const float* box, const int32_t* kind,
                                      const int32_t* kind_host, double* strain, double* dvec) {
  if (!ctx) return NG_ERR_INVALID;
  NG_REQUIRE(ctx, nnz >= 0 && nnz < ((int64_t)1 << 31), "box_grad_csr: nnz below 2^31");
  NG_REQUIRE(ctx, N == 0 || row_ptr, "box_grad_csr: row_ptr required");
  if (const int rc = box_grad_ragged_check(ctx, G, box, kind, kind_host)) return rc;
  return box_grad_common(ctx, stream, N, 0, pos, row_ptr, col, nullptr, dd, scale, G, graph_ptr, box, BG_PER_FRAME, kind, strain,
                         dvec);
}
