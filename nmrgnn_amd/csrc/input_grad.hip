// Gradients with respect to the model's inputs: the distances of the edges and, through them, the atom positions.
//
// ng_edge_mlp_dinput — the derivative of the edge function e(d) = mask * EdgeFCBlock(RBF(d)) (nmrgnn/model.py:251-261,
// nmrgnn/layers.py:137-140, nmrgnn/model.py:111-138) with respect to its scalar input d = d_eff, in forward mode.  Every
// row carries its value x and its tangent t = dx/dd through the hidden layers:
//   x0 = mask * exp(-(d - mu)^2 / gap)           t0 = x0 * (-2 (d - mu) / gap)
//   a  = x W_t + b_t      x' = act(a)            t' = act'(a) * (t W_t)
//   J  = mask * (t W_{Le-1})                     dd = sum_c de[c] J[c]
// The value and tangent rows of a tile multiply the same weights, so they are stacked as one A operand of twice the rows
// (rows 0 .. TR-1 values, TR .. 2TR-1 tangents) and go through v_mfma_f32_16x16x4_f32: exact fp32, no tape read (the
// hidden layers are recomputed from d_eff), so the result does not depend on how the forward computed e.  One workgroup
// owns TR rows at a time (grid-stride over tiles); the weights are staged through LDS in K-chunks; the last layer (E
// outputs) and the dot with de run on the VALU, each row's sum in column order: no atomics, bitwise deterministic.
//
// ng_positions_grad(_csr) — dpos[i] = sum over the slots (i -> j) of dd * scale * (r_i - r_j) / |r_i - r_j| minus the same
// term of every slot (s -> i) that points at i, walked through the incoming-edge lists.  One thread per atom, a gather:
// bitwise deterministic.  The two ends of a slot compute its term from the same operands in the same order, so what one
// atom gains the other loses exactly.
#include <algorithm>

#include "mfma_gemm.cuh"
#include "ng_common.h"
#include "pbc.cuh"
#include "ragged.cuh"

namespace ng {

constexpr int DI_THREADS = 256;           // 4 waves
constexpr int DI_MAX_LE = 6;
constexpr int DI_MAX_GRID = 1024;

struct DiPtrs {
  const float* p[DI_MAX_LE];
};

typedef float f32x4 __attribute__((ext_vector_type(4)));

// act(a) and act'(a) from the pre-activation (relu'(0) = 0 as TensorFlow defines it; sigmoid without overflow)
__device__ __forceinline__ void act_dual(int act, float a, float& y, float& g) {
  switch (act) {
    case 1: {
      const float t = expf(-fabsf(a));
      const float s = 1.0f / (1.0f + t);
      y = fmaxf(a, 0.0f) + log1pf(t);
      g = a >= 0.0f ? s : t * s;
      break;
    }
    case 2:
      y = fmaxf(a, 0.0f);
      g = a > 0.0f ? 1.0f : 0.0f;
      break;
    case 3:
      y = tanhf(a);
      g = 1.0f - y * y;
      break;
    default:
      y = a;
      g = 1.0f;
  }
}

// LDS (floats): two activation buffers of max(R * LD, TR * E), the weight chunk KC x LW, then TR distances, masks, slots.
// RB row blocks of 16 stacked rows (R = 16 RB rows = TR = 8 RB edges); every wave owns the column blocks w, w + 4, ...
// (at most NCB of them) of every hidden layer.
template <int RB, int NCB>
__global__ __launch_bounds__(DI_THREADS) void edge_dinput_kernel(
    int64_t n_rows, int H, int E, int Le, int act, const float* __restrict__ d_src, const float* __restrict__ d_eff,
    const int32_t* __restrict__ perm, const int32_t* __restrict__ n_live, const float* __restrict__ centers, float gap,
    DiPtrs W, DiPtrs B, const float* __restrict__ de, float* __restrict__ J_out, float* __restrict__ dd_out, int buf, int KC,
    int LW) {
  constexpr int R = 16 * RB, TR = R / 2;
  extern __shared__ __attribute__((aligned(16))) float di_lds[];
  float* bufs[2] = {di_lds, di_lds + buf};
  float* sW = di_lds + 2 * buf;
  float* s_d = sW + KC * LW;
  float* s_m = s_d + TR;
  int* s_slot = reinterpret_cast<int*>(s_m + TR);
  const int LD = H + 4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  const int HB = H / 16;
  int64_t nl = n_rows;
  if (perm) {
    if (*n_live < 0) return;      // nothing to do (a gate of the edge-function tables hands the call to the table): J_out, dd_out stay
    nl = std::min<int64_t>(*n_live, n_rows);
  }
  const int64_t n_tiles = (n_rows + TR - 1) / TR;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t r0 = tile * TR;
    __syncthreads();          // the previous tile is done with every buffer
    if (tid < TR) {
      const int64_t r = r0 + tid;
      int slot = -1;
      float m = 0.f, d = 0.f;
      if (r < n_rows) {
        slot = perm ? perm[r] : (int)r;
        if (r < nl && d_src[r] > 0.f) {
          m = 1.f;
          d = d_eff[r];
        }
      }
      s_slot[tid] = slot;
      s_m[tid] = m;
      s_d[tid] = d;
    }
    __syncthreads();
    float* cur = bufs[0];
    for (int idx = tid; idx < TR * H; idx += DI_THREADS) {
      const int row = idx / H, k = idx - row * H;
      float x = 0.f, t = 0.f;
      if (s_m[row] != 0.f) {
        const float diff = s_d[row] - centers[k];
        x = expf(-(diff * diff) / gap);
        t = x * (-2.0f * diff / gap);
      }
      cur[row * LD + k] = x;
      cur[(row + TR) * LD + k] = t;
    }
    int ib = 0;
    for (int layer = 0; layer < Le - 1; ++layer) {
      float* nxt = bufs[ib ^ 1];
      const float* Wt = W.p[layer];
      f32x4 acc[NCB][RB];
#pragma unroll
      for (int j = 0; j < NCB; ++j)
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) acc[j][rb] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int kb = 0; kb < H; kb += KC) {
        const int kc = std::min(KC, H - kb);
        __syncthreads();      // the previous chunk is consumed (and, at kb = 0, cur is complete)
        const int c4n = H / 4;
        for (int idx = tid; idx < kc * c4n; idx += DI_THREADS) {
          const int k = idx / c4n, c4 = idx - k * c4n;
          *reinterpret_cast<float4*>(sW + k * LW + 4 * c4) = *reinterpret_cast<const float4*>(Wt + (int64_t)(kb + k) * H + 4 * c4);
        }
        __syncthreads();
        for (int k0 = 0; k0 < kc; k0 += 4) {
          float a[RB];
#pragma unroll
          for (int rb = 0; rb < RB; ++rb) a[rb] = cur[(rb * 16 + l15) * LD + kb + k0 + l4];
#pragma unroll
          for (int j = 0; j < NCB; ++j) {
            const int cb = wave + 4 * j;
            if (cb < HB) {
              const float bv = sW[(k0 + l4) * LW + cb * 16 + l15];
#pragma unroll
              for (int rb = 0; rb < RB; ++rb) acc[j][rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[rb], bv, acc[j][rb], 0, 0, 0);
            }
          }
        }
      }
      // epilogue: lane holds D[row = 16 rb + 4 l4 + i][col = 16 cb + l15]; a value row and its tangent row (TR further)
      // sit in the same lane and register, row blocks rb and rb + RB/2
      const float* bt = B.p[layer];
#pragma unroll
      for (int j = 0; j < NCB; ++j) {
        const int cb = wave + 4 * j;
        if (cb < HB) {
          const int col = cb * 16 + l15;
          const float bias = bt[col];
#pragma unroll
          for (int rb = 0; rb < RB / 2; ++rb)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int row = rb * 16 + 4 * l4 + i;
              float y, g;
              act_dual(act, acc[j][rb][i] + bias, y, g);
              nxt[row * LD + col] = y;
              nxt[(row + TR) * LD + col] = g * acc[j][rb + RB / 2][i];
            }
        }
      }
      ib ^= 1;
      cur = nxt;
    }
    __syncthreads();          // the last hidden layer is complete
    // last layer on the tangent rows only: J[r][c] = mask_r * sum_k t[r][k] W[k][c]; its weights from LDS where they fit
    float* sJ = bufs[ib ^ 1];
    const float* Wl = W.p[Le - 1];
    if (H * E <= KC * LW) {
      for (int idx = tid; idx < H * E; idx += DI_THREADS) sW[idx] = Wl[idx];
      __syncthreads();
      Wl = sW;
    }
    for (int idx = tid; idx < TR * E; idx += DI_THREADS) {
      const int row = idx / E, c = idx - row * E;
      const float* tr = cur + (row + TR) * LD;
      float s = 0.f;
      for (int k = 0; k < H; ++k) s = fmaf(tr[k], Wl[k * E + c], s);
      const float Jv = s_m[row] != 0.f ? s : 0.f;
      sJ[idx] = Jv;
      const int slot = s_slot[row];
      if (J_out && slot >= 0) J_out[(int64_t)slot * E + c] = Jv;
    }
    __syncthreads();
    if (tid < TR) {
      const int slot = s_slot[tid];
      if (slot >= 0) {
        float s = 0.f;
        if (s_m[tid] != 0.f) {
          const float* g = de + (int64_t)slot * E;
          for (int c = 0; c < E; ++c) s = fmaf(g[c], sJ[tid * E + c], s);
        }
        dd_out[slot] = s;
      }
    }
  }
}

// the term of slot (i -> j): f * (r_i - r_j), f = g * scale / |r_i - r_j|; both ends call it with (i, j) in this order.
// r_i - r_j is minus the displacement D(r_i, r_j) the list builders computed for the edge (pbc.cuh; for DispOpen the same
// bits as r_i - r_j: a negated difference is exact).  A slot of length zero (coincident ends, which the cutoff builders
// list) contributes nothing: the gradient of |r| at 0 is taken as 0, a select on the finished factor, so that the length
// expression stays what it was
template <class Disp>
__device__ __forceinline__ float3 pg_term(const Disp& D, const float* __restrict__ pos, int64_t i, int64_t j, float g, float scale) {
  float ux, uy, uz;
  D(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], pos[3 * j], pos[3 * j + 1], pos[3 * j + 2], ux, uy, uz);
  const float vx = -ux, vy = -uy, vz = -uz;
  const float len = sqrtf(vx * vx + vy * vy + vz * vz);
  const float f = len > 0.f ? g * scale / len : 0.f;
  return make_float3(f * vx, f * vy, f * vz);
}

// row_ptr == NULL: padded lists (slots i*K .. i*K+K-1, a slot is live when edges > 0, source of slot s = s / K);
// otherwise CSR (entries row_ptr[i] .. row_ptr[i+1], all live, source of entry s = row_of[s]).
// D: the policy of row i's frame or structure, loaded by the kernel; both ends of an edge belong to the same one.
template <class Disp>
__device__ __forceinline__ void positions_grad_row(const Disp& D, int64_t i, int K, const float* __restrict__ pos,
                                                   const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                   const int32_t* __restrict__ row_of, const float* __restrict__ edges,
                                                   const float* __restrict__ dd, float scale,
                                                   const int32_t* __restrict__ csc_ptr, const int32_t* __restrict__ csc_edge,
                                                   float* __restrict__ dpos) {
  const int64_t s0 = row_ptr ? row_ptr[i] : i * K, s1 = row_ptr ? row_ptr[i + 1] : i * K + K;
  float ax = 0.f, ay = 0.f, az = 0.f;
  for (int64_t s = s0; s < s1; ++s) {
    const float g = dd[s];
    if (g == 0.f || (edges && !(edges[s] > 0.f))) continue;
    const float3 w = pg_term(D, pos, i, col[s], g, scale);
    ax += w.x;
    ay += w.y;
    az += w.z;
  }
  for (int p = csc_ptr[i]; p < csc_ptr[i + 1]; ++p) {
    const int64_t s = csc_edge[p];
    const float g = dd[s];
    if (g == 0.f) continue;
    const int64_t src = row_ptr ? (int64_t)row_of[s] : s / K;
    const float3 w = pg_term(D, pos, src, i, g, scale);
    ax -= w.x;
    ay -= w.y;
    az -= w.z;
  }
  dpos[3 * i] = ax;
  dpos[3 * i + 1] = ay;
  dpos[3 * i + 2] = az;
}

// Periodic policies: atom i belongs to frame i / n.
template <class Disp>
__global__ __launch_bounds__(256) void positions_grad_kernel(int64_t N, int K, const float* __restrict__ pos,
                                                             const int32_t* __restrict__ row_ptr,
                                                             const int32_t* __restrict__ col,
                                                             const int32_t* __restrict__ row_of,
                                                             const float* __restrict__ edges, const float* __restrict__ dd,
                                                             float scale, const int32_t* __restrict__ csc_ptr,
                                                             const int32_t* __restrict__ csc_edge, int n,
                                                             const float* __restrict__ box, float* __restrict__ dpos) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  Disp D;
  if (Disp::periodic) D.load(box, (int)(i / n));
  positions_grad_row(D, i, K, pos, row_ptr, col, row_of, edges, dd, scale, csc_ptr, csc_edge, dpos);
}

// The same rows on a ragged batch in boxes: atom i belongs to the structure the search of graph_ptr finds (ragged.cuh), and
// its edges use that structure's kind and box (pbc.cuh: DispPer).
__global__ __launch_bounds__(256) void positions_grad_ragged_kernel(int64_t N, int K, const float* __restrict__ pos,
                                                                    const int32_t* __restrict__ row_ptr,
                                                                    const int32_t* __restrict__ col,
                                                                    const int32_t* __restrict__ row_of,
                                                                    const float* __restrict__ edges,
                                                                    const float* __restrict__ dd, float scale,
                                                                    const int32_t* __restrict__ csc_ptr,
                                                                    const int32_t* __restrict__ csc_edge, int G,
                                                                    const int32_t* __restrict__ gp,
                                                                    const float* __restrict__ box,
                                                                    const int32_t* __restrict__ kind, float* __restrict__ dpos) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  DispPer D;
  D.load(box, kind, rg_range(gp, G, (int)N, (int)i).g);
  positions_grad_row(D, i, K, pos, row_ptr, col, row_of, edges, dd, scale, csc_ptr, csc_edge, dpos);
}

}  // namespace ng

using namespace ng;

extern "C" int ng_edge_mlp_dinput(ng_ctx* ctx, void* stream, int64_t n_slots, int H, int E, int Le, int act,
                                  const float* d_src, const float* d_eff, const int32_t* perm, const int32_t* n_live,
                                  const float* centers, float gap, const float* const* W, const float* const* b,
                                  const float* de, float* J_out, float* dd_out) {
  if (!ctx) return NG_ERR_INVALID;
  NG_REQUIRE(ctx, H % 16 == 0 && H >= 16 && H <= 512, "edge_mlp_dinput: edge_hidden_size % 16 == 0, 16 .. 512");
  NG_REQUIRE(ctx, E >= 1 && E <= 256, "edge_mlp_dinput: edge_feature_size 1 .. 256");
  NG_REQUIRE(ctx, Le >= 2 && Le <= DI_MAX_LE, "edge_mlp_dinput: edge_fc_layers 2 .. 6");
  NG_REQUIRE(ctx, act == NG_ACT_SOFTPLUS || act == NG_ACT_RELU || act == NG_ACT_TANH || act == NG_ACT_NONE,
             "edge_mlp_dinput: unknown activation code");
  NG_REQUIRE(ctx, gap > 0.f, "edge_mlp_dinput: rbf gap > 0");
  NG_REQUIRE(ctx, (perm == nullptr) == (n_live == nullptr), "edge_mlp_dinput: perm and n_live go together");
  NG_REQUIRE(ctx, n_slots >= 0 && n_slots < ((int64_t)1 << 31), "edge_mlp_dinput: slot count below 2^31");
  if (n_slots == 0) return NG_OK;
  NG_REQUIRE(ctx, d_src && d_eff && centers && W && b && de && dd_out, "edge_mlp_dinput: arguments");
  DiPtrs Wp{}, Bp{};
  for (int t = 0; t < Le; ++t) {
    NG_REQUIRE(ctx, W[t] && b[t], "edge_mlp_dinput: weights");
    NG_REQUIRE(ctx, t == Le - 1 || ((uintptr_t)W[t] & 15) == 0, "edge_mlp_dinput: hidden-layer weights 16-byte aligned");
    Wp.p[t] = W[t];
    Bp.p[t] = b[t];
  }
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard dg(ctx->device);
  // H <= 128: 32 edges per tile; wider layers 16, so that both activation buffers and a weight chunk fit the 160 KB of LDS
  const int RB = H <= 128 ? 4 : 2;
  const int R = 16 * RB, TR = R / 2;
  const int buf = std::max(R * (H + 4), TR * E);
  // weight chunk of KC rows: 8 KB up to H = 128 (two or three workgroups per CU), 32 KB at 256, 16 KB at 512
  const int KC = std::min(H, ((H <= 128 ? 2048 : H <= 256 ? 8192 : 4096) / H) & ~3);
  const int LW = H + (H % 32 == 0 ? 16 : 0);        // LW % 64 in {16, 48}: the 4 k rows of a B fragment hit distinct banks
  const size_t lds = (size_t)(2 * buf + KC * LW + 3 * TR) * 4;
  NG_REQUIRE(ctx, lds <= 160 * 1024, "edge_mlp_dinput: LDS budget");
  const int64_t tiles = cdiv(n_slots, TR);
  const dim3 grid((unsigned)std::min<int64_t>(tiles, DI_MAX_GRID)), block(DI_THREADS);
  ProfScope ps(ctx, st, "edge_mlp_dinput");
#define NG_DI(RBv, NCBv)                                                                                              \
  hipLaunchKernelGGL((edge_dinput_kernel<RBv, NCBv>), grid, block, lds, st, n_slots, H, E, Le, act, d_src, d_eff, perm, \
                     n_live, centers, gap, Wp, Bp, de, J_out, dd_out, buf, KC, LW)
  if (H <= 64) NG_DI(4, 1);
  else if (H <= 128) NG_DI(4, 2);
  else if (H <= 256) NG_DI(2, 4);
  else NG_DI(2, 8);
#undef NG_DI
  NG_HIP(ctx, hipGetLastError());
  return NG_OK;
}

static int positions_grad_common(ng_ctx* ctx, void* stream, int64_t N, int K, const float* pos, const int32_t* row_ptr,
                                 const int32_t* col, const int32_t* row_of, const float* edges, const float* dd, float scale,
                                 const int32_t* csc_ptr, const int32_t* csc_edge, float* dpos, int n = 0,
                                 const float* box = nullptr, int triclinic = -1) {
  NG_REQUIRE(ctx, N >= 0 && N < ((int64_t)1 << 31), "positions_grad: atom count below 2^31");
  if (triclinic >= 0) {
    NG_REQUIRE(ctx, triclinic <= 1, "positions_grad (pbc): triclinic flag 0 or 1");
    NG_REQUIRE(ctx, n >= 1 && N % n == 0, "positions_grad (pbc): atoms per frame n >= 1 dividing N");
  }
  if (N == 0) return NG_OK;
  NG_REQUIRE(ctx, pos && col && dd && csc_ptr && csc_edge && dpos, "positions_grad: arguments");
  NG_REQUIRE(ctx, triclinic < 0 || box, "positions_grad (pbc): box required");
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard dg(ctx->device);
  ProfScope ps(ctx, st, "positions_grad");
  const dim3 grid((unsigned)cdiv(N, 256)), block(256);
  if (triclinic < 0)
    hipLaunchKernelGGL(positions_grad_kernel<DispOpen>, grid, block, 0, st, N, K, pos, row_ptr, col, row_of, edges, dd, scale,
                       csc_ptr, csc_edge, 1, nullptr, dpos);
  else if (triclinic)
    hipLaunchKernelGGL(positions_grad_kernel<DispTric>, grid, block, 0, st, N, K, pos, row_ptr, col, row_of, edges, dd, scale,
                       csc_ptr, csc_edge, n, box, dpos);
  else
    hipLaunchKernelGGL(positions_grad_kernel<DispOrtho>, grid, block, 0, st, N, K, pos, row_ptr, col, row_of, edges, dd, scale,
                       csc_ptr, csc_edge, n, box, dpos);
  NG_HIP(ctx, hipGetLastError());
  return NG_OK;
}

extern "C" int ng_positions_grad(ng_ctx* ctx, void* stream, int64_t N, int K, const float* pos, const int32_t* nlist,
                                 const float* edges, const float* dd, float scale, const int32_t* csc_ptr,
                                 const int32_t* csc_edge, float* dpos) {
  if (!ctx) return NG_ERR_INVALID;
  NG_REQUIRE(ctx, K >= 1 && N * K < ((int64_t)1 << 31), "positions_grad: K >= 1, N * K below 2^31");
  NG_REQUIRE(ctx, N == 0 || edges, "positions_grad: edges required (dead slots)");
  return positions_grad_common(ctx, stream, N, K, pos, nullptr, nlist, nullptr, edges, dd, scale, csc_ptr, csc_edge, dpos);
}

extern "C" int ng_positions_grad_csr(ng_ctx* ctx, void* stream, int64_t N, int64_t nnz, const float* pos,
                                     const int32_t* row_ptr, const int32_t* col, const int32_t* row_of, const float* dd,
                                     float scale, const int32_t* csc_ptr, const int32_t* csc_edge, float* dpos) {
  if (!ctx) return NG_ERR_INVALID;
  NG_REQUIRE(ctx, nnz >= 0 && nnz < ((int64_t)1 << 31), "positions_grad_csr: nnz below 2^31");
  NG_REQUIRE(ctx, N == 0 || (row_ptr && row_of), "positions_grad_csr: row_ptr and row_of required");
  return positions_grad_common(ctx, stream, N, 0, pos, row_ptr, col, row_of, nullptr, dd, scale, csc_ptr, csc_edge, dpos);
}

// periodic boxes: box [G][9] (G = N / n) lower-triangular lattice vectors on the device, triclinic = 0 / 1 (pbc.cuh)
extern "C" int ng_positions_grad_pbc(ng_ctx* ctx, void* stream, int64_t N, int K, const float* pos, const int32_t* nlist,
                                     const float* edges, const float* dd, float scale, const int32_t* csc_ptr,
                                     const int32_t* csc_edge, int n, const float* box, int triclinic, float* dpos) {
  if (!ctx) return NG_ERR_INVALID;
  NG_REQUIRE(ctx, K >= 1 && N * K < ((int64_t)1 << 31), "positions_grad: K >= 1, N * K below 2^31");
  NG_REQUIRE(ctx, N == 0 || edges, "positions_grad: edges required (dead slots)");
  NG_REQUIRE(ctx, triclinic == 0 || triclinic == 1, "positions_grad (pbc): triclinic flag 0 or 1");
  return positions_grad_common(ctx, stream, N, K, pos, nullptr, nlist, nullptr, edges, dd, scale, csc_ptr, csc_edge, dpos, n, box,
                               triclinic);
}

extern "C" int ng_positions_grad_csr_pbc(ng_ctx* ctx, void* stream, int64_t N, int64_t nnz, const float* pos,
                                         const int32_t* row_ptr, const int32_t* col, const int32_t* row_of, const float* dd,
                                         float scale, const int32_t* csc_ptr, const int32_t* csc_edge, int n, const float* box,
                                         int triclinic, float* dpos) {
  if (!ctx) return NG_ERR_INVALID;
  NG_REQUIRE(ctx, nnz >= 0 && nnz < ((int64_t)1 << 31), "positions_grad_csr: nnz below 2^31");
  NG_REQUIRE(ctx, N == 0 || (row_ptr && row_of), "positions_grad_csr: row_ptr and row_of required");
  NG_REQUIRE(ctx, triclinic == 0 || triclinic == 1, "positions_grad (pbc): triclinic flag 0 or 1");
  return positions_grad_common(ctx, stream, N, 0, pos, row_ptr, col, row_of, nullptr, dd, scale, csc_ptr, csc_edge, dpos, n, box,
                               triclinic);
}

// ragged batches in boxes: graph_ptr [G+1], box [G][9] and kind [G] (-1 open, 0 orthorhombic, 1 reduced triclinic) on the
// device; kind_host: the kinds in host memory, checked when given (may be NULL)
static int positions_grad_ragged_common(ng_ctx* ctx, void* stream, int64_t N, int K, const float* pos, const int32_t* row_ptr,
                                        const int32_t* col, const int32_t* row_of, const float* edges, const float* dd,
                                        float scale, const int32_t* csc_ptr, const int32_t* csc_edge, int G,
                                        const int32_t* graph_ptr, const float* box, const int32_t* kind,
                                        const int32_t* kind_host, float* dpos) {
  NG_REQUIRE(ctx, N >= 0 && N < ((int64_t)1 << 31), "positions_grad: atom count below 2^31");
  NG_REQUIRE(ctx, G >= 0 && (N == 0 || G >= 1), "positions_grad (ragged): atoms need at least one structure");
  if (kind_host)
    for (int g = 0; g < G; ++g)
      NG_REQUIRE(ctx, kind_host[g] >= -1 && kind_host[g] <= 1, "positions_grad (ragged): kind -1 (open), 0 or 1");
  if (N == 0) return NG_OK;
  NG_REQUIRE(ctx, pos && col && dd && csc_ptr && csc_edge && dpos, "positions_grad: arguments");
  NG_REQUIRE(ctx, graph_ptr && box && kind, "positions_grad (ragged): graph_ptr, box and kind required");
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard dg(ctx->device);
  ProfScope ps(ctx, st, "positions_grad_ragged");
  hipLaunchKernelGGL(positions_grad_ragged_kernel, dim3((unsigned)cdiv(N, 256)), dim3(256), 0, st, N, K, pos, row_ptr, col, row_of,
                     edges, dd, scale, csc_ptr, csc_edge, G, graph_ptr, box, kind, dpos);
  NG_HIP(ctx, hipGetLastError());
  return NG_OK;
}

extern "C" int ng_positions_grad_ragged_pbc(ng_ctx* ctx, void* stream, int64_t N, int K, const float* pos, const int32_t* nlist,
                                            const float* edges, const float* dd, float scale, const int32_t* csc_ptr,
                                            const int32_t* csc_edge, int G, const int32_t* graph_ptr, const float* box,
                                            const int32_t* kind, const int32_t* kind_host, float* dpos) {
  if (!ctx) return NG_ERR_INVALID;
  NG_REQUIRE(ctx, K >= 1 && N * K < ((int64_t)1 << 31), "positions_grad: K >= 1, N * K below 2^31");
  NG_REQUIRE(ctx, N == 0 || edges, "positions_grad: edges required (dead slots)");
  return positions_grad_ragged_common(ctx, stream, N, K, pos, nullptr, nlist, nullptr, edges, dd, scale, csc_ptr, csc_edge, G,
                                      graph_ptr, box, kind, kind_host, dpos);
}

extern "C" int ng_positions_grad_csr_ragged_pbc(ng_ctx* ctx, void* stream, int64_t N, int64_t nnz, const float* pos,
                                                const int32_t* row_ptr, const int32_t* col, const int32_t* row_of,
                                                const float* dd, float scale, const int32_t* csc_ptr, const int32_t* csc_edge,
                                                int G, const int32_t* graph_ptr, const float* box, const int32_t* kind,
                                                const int32_t* kind_host, float* dpos) {
  if (!ctx) return NG_ERR_INVALID;
  NG_REQUIRE(ctx, nnz >= 0 && nnz < ((int64_t)1 << 31), "positions_grad_csr: nnz below 2^31");
  NG_REQUIRE(ctx, N == 0 || (row_ptr && row_of), "positions_grad_csr: row_ptr and row_of required");
  return positions_grad_ragged_common(ctx, stream, N, 0, pos, row_ptr, col, row_of, nullptr, dd, scale, csc_ptr, csc_edge, G,
                                      graph_ptr, box, kind, kind_host, dpos);
}
