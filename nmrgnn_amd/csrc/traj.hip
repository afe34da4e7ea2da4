// Binary trajectory frames -> positions: one launch turns a raw chunk of file bytes on the device (DCD or Amber NetCDF, as read
// from disk) into float32 out[G][n_out][3].  Component c of source atom a of frame g is the 32-bit word at
//   g * frame_stride + off_c + a * elem_stride
// so DCD is the planar case (elem_stride 4, the offsets one Fortran record apart) and NetCDF the interleaved one (elem_stride
// 12, the offsets 4 apart).  Words move as bits (uint32): a byte swap for the other endianness, no float arithmetic, so NaN
// payloads, -0.0 and subnormals come out bit for bit.
//
// A workgroup owns 256 consecutive output atoms of one frame.  Lane t reads the three words of its atom: consecutive lanes read
// consecutive words of one component in the planar case and one contiguous 12-byte-stride run in the interleaved one (its three
// loads cover the same cache lines).  The 768 words go through LDS (stride 3 words over the lanes: no bank conflict) and leave
// as three stores of 256 consecutive words.  With `sel` the source atom of lane t is sel[j]; the gather is as coalesced as the
// selection is.  A word whose exponent field is all ones is not finite: the workgroup's count of them goes to `bad` with one
// integer atomic (an exact count in any order).  All addressing is 64-bit; no scratch; capturable.
#include "ng_internal.h"

namespace ng {

constexpr int TRAJ_TILE = 256;

__device__ __forceinline__ uint32_t traj_bswap(uint32_t v) {
  return (v >> 24) | ((v >> 8) & 0x0000ff00u) | ((v << 8) & 0x00ff0000u) | (v << 24);
}

__global__ __launch_bounds__(TRAJ_TILE) void frames_decode_kernel(const unsigned char* __restrict__ raw, int64_t tiles,
                                                                  int64_t frame_stride, int64_t off_x, int64_t off_y,
                                                                  int64_t off_z, int64_t elem_stride, int swap, int64_t n_src,
                                                                  const int32_t* __restrict__ sel, int64_t n_out,
                                                                  uint32_t* __restrict__ out, int* __restrict__ bad) {
  __shared__ uint32_t tile[3 * TRAJ_TILE];
  __shared__ int nbad;
  const int t = threadIdx.x;
  const int64_t g = (int64_t)blockIdx.x / tiles;
  const int64_t j0 = ((int64_t)blockIdx.x % tiles) * TRAJ_TILE;
  const int64_t j = j0 + t;
  if (t == 0) nbad = 0;
  int cnt = 0;
  if (j < n_out) {
    const int64_t a = sel ? (int64_t)sel[j] : j;
    uint32_t w[3] = {0x7fc00000u, 0x7fc00000u, 0x7fc00000u};   // an index outside [0, n_src) reads nothing and is counted
    if (a >= 0 && a < n_src) {
      const unsigned char* p = raw + g * frame_stride + a * elem_stride;
      w[0] = *reinterpret_cast<const uint32_t*>(p + off_x);
      w[1] = *reinterpret_cast<const uint32_t*>(p + off_y);
      w[2] = *reinterpret_cast<const uint32_t*>(p + off_z);
      if (swap) {
        w[0] = traj_bswap(w[0]);
        w[1] = traj_bswap(w[1]);
        w[2] = traj_bswap(w[2]);
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      tile[3 * t + c] = w[c];
      cnt += (w[c] & 0x7f800000u) == 0x7f800000u;
    }
  }
  __syncthreads();
  if (cnt) atomicAdd(&nbad, cnt);
  const int64_t live = 3 * (n_out - j0 < TRAJ_TILE ? n_out - j0 : (int64_t)TRAJ_TILE);   // words of this tile
  uint32_t* dst = out + (g * n_out + j0) * 3;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int i = k * TRAJ_TILE + t;
    if (i < live) dst[i] = tile[i];
  }
  __syncthreads();
  if (t == 0 && nbad) atomicAdd(bad, nbad);
}

}  // namespace ng

using namespace ng;

extern "C" int ng_frames_decode(ng_ctx* ctx, void* stream, const void* raw, int64_t raw_bytes, int64_t G, int64_t frame_stride,
                                int64_t off_x, int64_t off_y, int64_t off_z, int64_t elem_stride, int swap, int64_t n_src,
                                const int32_t* sel, int64_t n_out, float* out, int* bad) {
  if (!ctx) return NG_ERR_INVALID;
  NG_REQUIRE(ctx, raw && out && bad, "frames_decode: raw, out and bad required");
  NG_REQUIRE(ctx, G >= 0 && n_src >= 0 && n_out >= 0, "frames_decode: negative frame or atom count");
  NG_REQUIRE(ctx, raw_bytes >= 0 && raw_bytes < ((int64_t)1 << 31), "frames_decode: a chunk holds fewer than 2^31 bytes");
  NG_REQUIRE(ctx, frame_stride >= 0 && off_x >= 0 && off_y >= 0 && off_z >= 0 && elem_stride >= 0,
             "frames_decode: negative offset or stride");
  NG_REQUIRE(ctx, frame_stride % 4 == 0 && off_x % 4 == 0 && off_y % 4 == 0 && off_z % 4 == 0 && elem_stride % 4 == 0,
             "frames_decode: offsets and strides are multiples of 4");
  NG_REQUIRE(ctx, ((uintptr_t)raw & 3) == 0, "frames_decode: raw is aligned to 4 bytes");
  NG_REQUIRE(ctx, swap == 0 || swap == 1, "frames_decode: swap is 0 or 1");
  NG_REQUIRE(ctx, sel != nullptr || n_out == n_src, "frames_decode: without sel, n_out equals n_src");
  if (G == 0 || n_out == 0) return NG_OK;
  NG_REQUIRE(ctx, n_src >= 1, "frames_decode: a selection needs source atoms");
  // the last word read must end inside raw; every term is checked against raw_bytes first, so the sum cannot overflow
  const int64_t off_max = std::max(off_x, std::max(off_y, off_z));
  const int64_t lim = (int64_t)1 << 31;
  NG_REQUIRE(ctx, off_max < lim && (G == 1 || frame_stride < lim) && (n_src == 1 || elem_stride < lim) && G <= lim && n_src <= lim,
             "frames_decode: layout exceeds the chunk");
  NG_REQUIRE(ctx, (G - 1) * frame_stride + off_max + (n_src - 1) * elem_stride + 4 <= raw_bytes,
             "frames_decode: the layout's last word ends beyond raw_bytes");
  const int64_t tiles = cdiv(n_out, TRAJ_TILE);
  NG_REQUIRE(ctx, tiles <= 0x7fffffff / G, "frames_decode: more than 2^31 - 1 workgroups");
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(ctx, st, "frames_decode");
  hipLaunchKernelGGL(frames_decode_kernel, dim3((unsigned)(G * tiles)), dim3(TRAJ_TILE), 0, st, (const unsigned char*)raw, tiles,
                     frame_stride, off_x, off_y, off_z, elem_stride, swap, n_src, sel, n_out, reinterpret_cast<uint32_t*>(out), bad);
  NG_HIP(ctx, hipGetLastError());
  return NG_OK;
}
