// Gaussian smoothing of a [D, H, W] volume (light_unet/smooth.py: gaussian_filter): one axis of
// scipy.ndimage.gaussian_filter per launch, by the contract written out in include/l3u.h -- the
// symmetric line pass in float64 with the outermost pair added first, the result rounded to the
// array's dtype.  This file is compiled with -ffp-contract=off (Makefile): every fp64 product and
// sum is rounded on its own, and each output's sum runs in one thread in the stated order, so the
// result does not depend on the launch shape.  No atomics.
//
// Both kernels stage a tile with its halo of `radius` taps per side through LDS, in the array's own
// type, every tap fetched through the boundary map: the map is resolved once per LDS row (per
// LDS column along x) when the tile is loaded, never per multiply, and a tap outside the volume in
// `constant` mode is replaced by cval (a double) when it is read back.  A thread then owns 4
// consecutive outputs along the filtered axis and keeps two sliding windows of 4 doubles, the
// left taps v[i + j] and the right taps v[i - j]: stepping j moves each window by one element, so
// a step costs 2 LDS reads for its 4 outputs instead of 8, and no tap is loaded from global memory
// more than once per tile.  The weights sit in LDS (65 doubles), read as a broadcast.
//
// Along z and y (gauss_lines): the volume is [outer][n][inner] with inner = H * W or W contiguous.
// A workgroup takes 256 bytes of inner (64 floats or 32 doubles: consecutive lanes on consecutive
// x, so every tap row is one coalesced load and one conflict-free LDS row) by 64 outputs along the
// axis; its 4 (8) quad rows walk the 16 quads of a column.  Halo re-reads between neighbouring
// tiles are 2r / 64 of the volume (6 % at r = 2) and come from L2.
// Along x (gauss_rows): a tile is 16 rows by 256 outputs, staged with its halo as row segments;
// lane q of a quad row owns outputs 4q .. 4q + 3 (resample_linear's split, csrc/resample.hip) and
// stores them as one 16-byte vector where the quad is whole and aligned.  The window reads are 4
// dwords apart between lanes: a 4-way conflict on ds_read_b32 (8 LDS cycles for 4 x 64 outputs,
// what 4 conflict-free reads of one output per lane would cost).
//
// As compiled for gfx950 (hipcc -O3, -Rpass-analysis=kernel-resource-usage; 256 threads each):
//   gauss_lines<float>   63 VGPRs, LDS 528 B static + (64 + 2r) * 256 B dynamic: 17.5 KiB at r = 2
//   gauss_lines<double>  61 VGPRs  (8 workgroups per CU, the wave limit), 48.5 KiB at r = 64 (3)
//   gauss_rows<float>    58 VGPRs, 106 SGPRs (7 per CU), LDS 528 B + 16 * (256 + 2r) * 4 B: 16.8 KiB
//                        at r = 2, 24.5 KiB at r = 64 (6)
//   gauss_rows<double>   57 VGPRs, LDS 528 B + 16 * (256 + 2r) * 8 B: 33.0 KiB at r = 2 (4 per CU),
//                        48.5 KiB at r = 64 (3)
// no scratch in any of them.
//
// There is no fused three-axis launch.  One was built and measured (a 14 x 14 x 64 float tile with
// its halo in 49 KiB of LDS, the z and y passes in place in LDS, 512 threads, bit-identical to the
// three launches): 0.306 ms against 0.242 ms for the three launches at 204 x 204 x 450 with radii
// 3, 3, 3 (README, profiles/smooth_bench.json), so it was deleted.
#include "common.h"

namespace l3u {
namespace {

constexpr int kMaxR = 64;          // the largest radius: the weight table and the halo are sized by it
constexpr int kTile = 64;          // outputs along the axis per gauss_lines tile
constexpr int kRowsX = 16, kTileX = 256;   // rows and outputs per gauss_rows tile
enum { kReflect = 0, kMirror = 1, kNearest = 2, kConstant = 3 };

// the in-volume index of tap k on an axis of length n; applied as often as needed: |k| may exceed
// n many times over.  `constant` clamps (the value is replaced when the tap is read back).
L3U_DEV int tap_index(int k, int n, int mode) {
  if (mode == kReflect) {
    int m = k % (2 * n);
    m = m < 0 ? m + 2 * n : m;
    return m >= n ? 2 * n - 1 - m : m;
  }
  if (mode == kMirror) {
    if (n == 1) return 0;
    const int p = 2 * n - 2;
    int m = k % p;
    m = m < 0 ? m + p : m;
    return m >= n ? p - m : m;
  }
  return min(max(k, 0), n - 1);
}

// 4 consecutive outputs from the taps ld(p), p relative to the first output's centre:
//   t = v[i] * w[r];  t = t + (v[i + j] + v[i - j]) * w[j + r] for j = -r .. -1
template <typename Load>
L3U_DEV void quad(const double* __restrict__ wl, int r, Load ld, double t[4]) {
  double a[4], b[4];
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    t[o] = ld(o) * wl[r];
    a[o] = ld(o - r);
    b[o] = ld(o + r);
  }
  for (int jj = 0; jj < r; ++jj) {          // j = jj - r
    const double w = wl[jj];
#pragma unroll
    for (int o = 0; o < 4; ++o) t[o] = t[o] + (a[o] + b[o]) * w;
    a[0] = a[1]; a[1] = a[2]; a[2] = a[3];
    b[3] = b[2]; b[2] = b[1]; b[1] = b[0];
    if (jj + 1 < r) {
      a[3] = ld(jj + 1 - r + 3);
      b[0] = ld(r - jj - 1);
    }
  }
}

L3U_DEV void load_weights(double* wl, const double* __restrict__ w, int r) {
  for (int i = (int)threadIdx.x; i <= r; i += 256) wl[i] = w[i];
}

// axis 0 (outer = 1, inner = H * W) and axis 1 (outer = D, inner = W).  blockIdx.x: the column
// tile, blockIdx.y strides over (outer, axis tile).
template <typename T>
__global__ __launch_bounds__(256) void gauss_lines(const T* __restrict__ src, T* __restrict__ dst,
                                                   int outer, int n, long long inner,
                                                   const double* __restrict__ w, int r, int mode,
                                                   double cval) {
  constexpr int kCols = 256 / (int)sizeof(T), kGroups = 256 / kCols;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ double wl[kMaxR + 2];   // 528 B: the dynamic region behind it stays 16-byte aligned
  T* tile = reinterpret_cast<T*>(smem);
  const int c = (int)threadIdx.x % kCols, g = (int)threadIdx.x / kCols;
  const long long x = (long long)blockIdx.x * kCols + c;
  const bool live = x < inner;
  const int ntile = (n + kTile - 1) / kTile, rows = kTile + 2 * r;
  const bool fill = mode == kConstant;
  load_weights(wl, w, r);
  for (long long it = blockIdx.y; it < (long long)outer * ntile; it += gridDim.y) {
    const int o = (int)(it / ntile), i0 = (int)(it - (long long)o * ntile) * kTile;
    const long long base = (long long)o * n * inner + x;
    __syncthreads();                                   // the previous tile has been read
    if (live)
      for (int p = g; p < rows; p += kGroups)
        tile[p * kCols + c] = src[base + tap_index(i0 - r + p, n, mode) * inner];
    __syncthreads();
    if (live)
      for (int q = g; q < kTile / 4; q += kGroups) {
        const int i = i0 + 4 * q;
        if (i >= n) break;
        double t[4];
        quad(wl, r, [&](int p) {
          const int k = i + p;
          const double v = (double)tile[(k - i0 + r) * kCols + c];
          return fill && (k < 0 || k >= n) ? cval : v;
        }, t);
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (i + u < n) dst[base + (long long)(i + u) * inner] = (T)t[u];
      }
  }
}

template <typename T>
L3U_DEV void store_quad(T* p, const double t[4], int valid) {
  typedef T v2 __attribute__((ext_vector_type(2)));
  typedef T v4 __attribute__((ext_vector_type(4)));
  if (valid >= 4 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
    if constexpr (sizeof(T) == 4) {
      *reinterpret_cast<v4*>(p) = v4{(T)t[0], (T)t[1], (T)t[2], (T)t[3]};
    } else {
      *reinterpret_cast<v2*>(p) = v2{(T)t[0], (T)t[1]};
      *reinterpret_cast<v2*>(p + 2) = v2{(T)t[2], (T)t[3]};
    }
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (u < valid) p[u] = (T)t[u];
  }
}

// axis 2: nrows = D * H contiguous rows of n.  blockIdx.x: the x tile, blockIdx.y strides over the
// row tiles.
template <typename T>
__global__ __launch_bounds__(256) void gauss_rows(const T* __restrict__ src, T* __restrict__ dst,
                                                  long long nrows, int n,
                                                  const double* __restrict__ w, int r, int mode,
                                                  double cval) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ double wl[kMaxR + 2];   // 528 B: the dynamic region behind it stays 16-byte aligned
  T* tile = reinterpret_cast<T*>(smem);
  const int pitch = kTileX + 2 * r;
  const int ql = (int)threadIdx.x & 63, rg = (int)threadIdx.x >> 6;
  const int x0 = (int)blockIdx.x * kTileX;
  const bool fill = mode == kConstant;
  load_weights(wl, w, r);
  const long long ntile = (nrows + kRowsX - 1) / kRowsX;
  for (long long it = blockIdx.y; it < ntile; it += gridDim.y) {
    const long long row0 = it * kRowsX;
    const int rows = (int)min((long long)kRowsX, nrows - row0);
    __syncthreads();                                   // the previous tile has been read
    for (int p = (int)threadIdx.x; p < pitch; p += 256) {
      const int m = tap_index(x0 - r + p, n, mode);    // once per tap column, for every row
      for (int y = 0; y < rows; ++y) tile[y * pitch + p] = src[(row0 + y) * n + m];
    }
    __syncthreads();
    const int i = x0 + 4 * ql;
    if (i < n)
      for (int y = rg; y < rows; y += 4) {
        const int off = y * pitch + r - x0;             // tile[off + k]: tap k of this row
        double t[4];
        quad(wl, r, [&](int p) {
          const int k = i + p;
          const double v = (double)tile[off + k];
          return fill && (k < 0 || k >= n) ? cval : v;
        }, t);
        store_quad(dst + (row0 + y) * n + i, t, n - i);
      }
  }
}

L3U_INLINE_HOST bool dims_ok(long long D, long long H, long long W) {
  return D > 0 && H > 0 && W > 0 && D < (1 << 30) && H < (1 << 30) && W < (1 << 30) &&
         D * H < (1ll << 31) && H * W < (1ll << 31) && D * H * W < (1ll << 40);
}

template <typename T>
int launch_axis(const T* src, T* dst, int D, int H, int W, int axis, const double* w, int r,
                int mode, double cval, hipStream_t stream) {
  if (axis == 2) {
    const long long nrows = (long long)D * H, ntile = (nrows + kRowsX - 1) / kRowsX;
    const dim3 grid((unsigned)((W + kTileX - 1) / kTileX), (unsigned)min(ntile, 4096ll));
    const size_t lds = (size_t)kRowsX * (kTileX + 2 * r) * sizeof(T);
    gauss_rows<T><<<grid, 256, lds, stream>>>(src, dst, nrows, W, w, r, mode, cval);
  } else {
    constexpr int kCols = 256 / (int)sizeof(T);
    const int outer = axis == 0 ? 1 : D, n = axis == 0 ? D : H;
    const long long inner = axis == 0 ? (long long)H * W : W;
    const long long work = (long long)outer * ((n + kTile - 1) / kTile);
    const dim3 grid((unsigned)((inner + kCols - 1) / kCols), (unsigned)min(work, 1024ll));
    const size_t lds = (size_t)(kTile + 2 * r) * 256;
    gauss_lines<T><<<grid, 256, lds, stream>>>(src, dst, outer, n, inner, w, r, mode, cval);
  }
  L3U_CHECK_LAUNCH();
}

}  // namespace
}  // namespace l3u

using namespace l3u;

extern "C" int l3u_gauss_max_radius(void) { return kMaxR; }

extern "C" int l3u_gauss_axis(const void* src, void* dst, int dtype, int D, int H, int W, int axis,
                              const double* w, int radius, int mode, double cval,
                              hipStream_t stream) {
  L3U_REQUIRE(src && dst && w && (dtype == 0 || dtype == 1) && dims_ok(D, H, W));
  L3U_REQUIRE(axis >= 0 && axis <= 2 && radius >= 0 && radius <= kMaxR);
  L3U_REQUIRE(mode >= kReflect && mode <= kConstant);
  const unsigned long long bytes = (unsigned long long)D * H * W * (dtype == 0 ? 4 : 8);
  const uintptr_t s = reinterpret_cast<uintptr_t>(src), d = reinterpret_cast<uintptr_t>(dst);
  L3U_REQUIRE(s + bytes <= d || d + bytes <= s);       // distinct buffers: no overlap at all
  if (dtype == 0)
    return launch_axis(static_cast<const float*>(src), static_cast<float*>(dst), D, H, W, axis, w,
                       radius, mode, cval, stream);
  return launch_axis(static_cast<const double*>(src), static_cast<double*>(dst), D, H, W, axis, w,
                     radius, mode, cval, stream);
}
