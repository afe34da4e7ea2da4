// Periodic boxes under the minimum-image convention: the displacement policies of the neighbour-list builders (knn.hip,
// knn_cells.hip, cutoff.hip, ragged.hip) and of the position gradient (input_grad.hip).
//
// A box is three lattice vectors in lower-triangular form, [9] floats per frame, row-major: a = (ax, 0, 0),
// b = (bx, by, 0), c = (cx, cy, cz) — the GROMACS / MDAnalysis triclinic_vectors convention.  The host converts
// (a, b, c, alpha, beta, gamma) to that form and accepts only orthorhombic and reduced triclinic boxes
// (|bx| <= ax/2, |cx| <= ax/2, |cy| <= by/2).
//
// A policy D is called as D(q, c, d): d = the displacement from q to c, from the two RAW positions.  Every kernel that
// builds or differentiates a periodic edge calls the same policy with (query, candidate) in that order, so the cell grid
// and brute force see the same bits and the gradient uses exactly the vector behind each edge.
//   DispOpen   c - q: today's arithmetic, bit for bit (the open-boundary instantiations stay what they were)
//   DispOrtho  c - q, then rint per axis
//   DispTric   c - q, sequential z / y / x wrap; when the wrapped vector is not shorter than w_min / 2 (w_min: the smallest
//              perpendicular width) the nearest of its neighbouring images.  Below w_min / 2 it is provably the minimum
//              image: every other image is at least w_min - |d| away.  The neighbouring images are i a + j b + k c with
//              |k| <= nk, |j| <= nj, |i| <= ni.  The wrapped vector d has |d_x| <= a_x / 2, |d_y| <= b_y / 2, |d_z| <= c_z / 2,
//              so |d| <= R = sqrt(a_x^2 + b_y^2 + c_z^2) / 2, and the minimum image m = d + i a + j b + k c is no longer:
//              |d_z + k c_z| <= R gives |k| <= R / c_z + 1/2, |d_y + k c_y + j b_y| <= R gives |j| <= R / b_y + 1/2 +
//              nk |c_y| / b_y.  Along x, a = (a_x, 0, 0) moves nothing else: for given j and k the best i is the integer nearest to
//              -(d_x + j b_x + k c_x) / a_x, and |d_x + j b_x + k c_x| <= a_x / 2 + nj |b_x| + nk |c_x| puts it within
//              ni = ceil((nj |b_x| + nk |c_x|) / a_x) (on the tie at a whole quotient both candidates are equally long).
//              For the usual cells (cube-like boxes, the rhombic dodecahedron, the truncated octahedron) that is 1, 1, 1:
//              the 27 images, unrolled.  A box that is thin along c (c_z well below a_x, b_y) needs |k| = 2 and more:
//              a rolled search.
//   DispPer    a ragged batch, where every structure has a boundary kind of its own (-1 open, 0 orthorhombic, 1 reduced
//              triclinic; kind [G] int32 next to box [G][9]): loads the structure's kind and vectors and calls, at run time,
//              the operator() of the policy of that kind as it stands above.  An orthorhombic structure next to a triclinic
//              one runs DispOrtho's arithmetic, not DispTric's on zero off-diagonals (the two may differ in the last bit
//              when a wrapped component rounds just past L/2).
// Which policy runs is chosen on the host from the box values: a template argument, not a user switch.
#pragma once
#include <hip/hip_runtime.h>

namespace ng {

// the squared-distance expression of every builder, the only copy (nlist_common.cuh says why it is an explicit fma chain)
__device__ __forceinline__ float pbc_dist2(float dx, float dy, float dz) { return fmaf(dz, dz, fmaf(dy, dy, dx * dx)); }

struct DispOpen {
  static constexpr bool periodic = false;
  __device__ __forceinline__ void load(const float*, int) {}
  __device__ __forceinline__ void operator()(float qx, float qy, float qz, float cx, float cy, float cz, float& dx, float& dy,
                                             float& dz) const {
    dx = cx - qx; dy = cy - qy; dz = cz - qz;
  }
};

struct DispOrtho {
  static constexpr bool periodic = true;
  float lx, ly, lz, ix, iy, iz;
  __device__ __forceinline__ void load(const float* box, int frame) {
    const float* b = box + (int64_t)frame * 9;
    lx = b[0]; ly = b[4]; lz = b[8];
    ix = 1.0f / lx; iy = 1.0f / ly; iz = 1.0f / lz;
  }
  __device__ __forceinline__ void operator()(float qx, float qy, float qz, float cx, float cy, float cz, float& dx, float& dy,
                                             float& dz) const {
    dx = cx - qx; dy = cy - qy; dz = cz - qz;
    dx = fmaf(-lx, rintf(dx * ix), dx);
    dy = fmaf(-ly, rintf(dy * iy), dy);
    dz = fmaf(-lz, rintf(dz * iz), dz);
  }
};

struct DispTric {
  static constexpr bool periodic = true;
  float ax, bx, by, cx, cy, cz, iax, iby, icz, h2;
  int nk, nj, ni;      // the reach of the image search along c, b, a (see above)
  __device__ __forceinline__ void load(const float* box, int frame) {
    const float* b = box + (int64_t)frame * 9;
    ax = b[0]; bx = b[3]; by = b[4]; cx = b[6]; cy = b[7]; cz = b[8];
    iax = 1.0f / ax; iby = 1.0f / by; icz = 1.0f / cz;
    // perpendicular widths: V / |b x c|, V / |c x a| = by cz / |(cy, cz)|, V / |a x b| = cz
    const float v = ax * by * cz;
    const float bcx = by * cz, bcy = -bx * cz, bcz = bx * cy - by * cx;
    const float wa = v / sqrtf(bcx * bcx + bcy * bcy + bcz * bcz);
    const float wb = by * cz / sqrtf(cy * cy + cz * cz);
    const float w = fminf(fminf(wa, wb), cz);
    h2 = 0.25f * w * w;
    const float r = 0.5f * sqrtf(ax * ax + by * by + cz * cz) * 1.0001f;      // rounded up: one image too many is harmless
    nk = (int)(r * icz + 0.5f);
    nj = (int)(r * iby + 0.5f + (float)nk * fabsf(cy) * iby);
    ni = max((int)ceilf(((float)nj * fabsf(bx) + (float)nk * fabsf(cx)) * iax), 1);
  }
  __device__ __forceinline__ void image(int i, int j, int k, float ox, float oy, float oz, float& best, float& dx, float& dy,
                                        float& dz) const {
    const float ex = fmaf((float)k, cx, fmaf((float)j, bx, fmaf((float)i, ax, ox)));
    const float ey = fmaf((float)k, cy, fmaf((float)j, by, oy));
    const float ez = fmaf((float)k, cz, oz);
    const float e2 = pbc_dist2(ex, ey, ez);
    if (e2 < best) { best = e2; dx = ex; dy = ey; dz = ez; }
  }
  __device__ __forceinline__ void operator()(float qx, float qy, float qz, float px, float py, float pz, float& dx, float& dy,
                                             float& dz) const {
    dx = px - qx; dy = py - qy; dz = pz - qz;
    float s = rintf(dz * icz);
    dx = fmaf(-s, cx, dx); dy = fmaf(-s, cy, dy); dz = fmaf(-s, cz, dz);
    s = rintf(dy * iby);
    dx = fmaf(-s, bx, dx); dy = fmaf(-s, by, dy);
    s = rintf(dx * iax);
    dx = fmaf(-s, ax, dx);
    float best = pbc_dist2(dx, dy, dz);
    if (best >= h2) {
      const float ox = dx, oy = dy, oz = dz;
      if ((nk | nj | ni) <= 1) {
        for (int k = -1; k <= 1; ++k)
          for (int j = -1; j <= 1; ++j)
            for (int i = -1; i <= 1; ++i) image(i, j, k, ox, oy, oz, best, dx, dy, dz);
      } else {      // a thin box: every image within reach
#pragma unroll 1
        for (int k = -nk; k <= nk; ++k)
#pragma unroll 1
          for (int j = -nj; j <= nj; ++j)
#pragma unroll 1
            for (int i = -ni; i <= ni; ++i) image(i, j, k, ox, oy, oz, best, dx, dy, dz);
      }
    }
  }
};

// Lanes of one wave may sit in structures of different kinds: the switch runs per call, inside the candidate loops of the
// builders, and a wave pays for every kind it holds (the triclinic 27-image search included).
struct DispPer {
  static constexpr bool periodic = true;
  int kind = -1;
  DispOrtho O;
  DispTric T;
  __device__ __forceinline__ void load(const float* box, const int32_t* kinds, int g) {
    kind = kinds[g];
    if (kind == 0) O.load(box, g);
    else if (kind == 1) T.load(box, g);
  }
  __device__ __forceinline__ void operator()(float qx, float qy, float qz, float cx, float cy, float cz, float& dx, float& dy,
                                             float& dz) const {
    if (kind == 0) O(qx, qy, qz, cx, cy, cz, dx, dy, dz);
    else if (kind == 1) T(qx, qy, qz, cx, cy, cz, dx, dy, dz);
    else DispOpen()(qx, qy, qz, cx, cy, cz, dx, dy, dz);
  }
};

// true for the policy that takes a kind array and a structure index in load()
template <class Disp> struct disp_per_structure { static constexpr bool value = false; };
template <> struct disp_per_structure<DispPer> { static constexpr bool value = true; };

// D.load for structure (or frame) g, whichever form the policy takes; kinds is read by DispPer alone
template <class Disp>
__device__ __forceinline__ void disp_load(Disp& D, const float* box, const int32_t* kinds, int g) {
  if constexpr (disp_per_structure<Disp>::value) D.load(box, kinds, g);
  else D.load(box, g);
}

}  // namespace ng
