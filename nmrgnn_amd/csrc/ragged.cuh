// The structure of a row of a ragged batch (graph_ptr [G+1] on the device): shared by the list builders (ragged.hip) and the
// ragged position gradient (input_grad.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ng {

// the structure of row i: the g with gp[g] <= i < gp[g + 1] (gp non-decreasing, gp[0] = 0, gp[G] = N > i; empty structures
// are skipped over), and its row range clamped to [0, N) around i, so that a malformed graph_ptr cannot send a read out of
// the batch.  g lies in [0, G): a per-structure box or kind is read at an index inside its array.
struct RgRange {
  int lo, hi, g;
};
__device__ __forceinline__ RgRange rg_range(const int32_t* __restrict__ gp, int G, int N, int i) {
  int a = 0, b = G;
  while (b - a > 1) {
    const int m = (a + b) >> 1;
    if (gp[m] <= i) a = m; else b = m;
  }
  return {max(0, min(gp[a], i)), min(N, max(gp[a + 1], i + 1)), a};
}

}  // namespace ng
