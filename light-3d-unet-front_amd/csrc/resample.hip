// Resampling a [D, H, W] volume to another grid (light_unet/resample.py): the semantics of
// scipy.ndimage.zoom(x, zoom, order, mode="nearest", grid_mode=True) for order 0 (labels, masks:
// the value of one source voxel, copied) and order 1 (images, probability maps: the 8 corners).
//
// The coordinates are not computed here.  The host builds, per axis and per output index, the
// clamped source indices (and for order 1 the fraction t) in float64, once per call; the kernels
// gather through those tables: no float64 divide, no floor, and the coordinates agree with the
// definition by construction.  A table entry is clamped to the source again on load (one integer
// instruction), so a bad table reads the wrong voxel but nothing outside the source.
//
// Work split: a 256-thread workgroup is TX x (256 / TX) threads, TX the power of two that covers a
// row's quads (4 consecutive output x).  A thread owns one quad column -- its x table entries are
// read once -- and walks the output rows (z, y) in a grid-stride loop; per row it reads the z / y
// table entries and forms the source row bases once, requests every source value of the quad, and
// stores the quad as one vector where it is whole and its address aligned (scalar stores
// otherwise: the tail of a row whose width is no multiple of 4, rows of such a volume that start
// unaligned, an unaligned dst).  Rows wider than 1024 take further columns in an outer loop.
// Offsets are long long (a case can pass 2^31 bytes).  No atomics and no cross-thread sums: the
// result does not depend on the launch shape.
#include "common.h"

namespace l3u {
namespace {

template <typename T> struct vec4_of;
template <> struct vec4_of<float> { typedef float type __attribute__((ext_vector_type(4))); };
template <> struct vec4_of<double> { typedef double type __attribute__((ext_vector_type(2))); };
template <> struct vec4_of<unsigned char> { typedef unsigned char type __attribute__((ext_vector_type(4))); };

// v[0..3] to p[0..3]; `whole`: all four exist.  One 16-byte store for float (two for double, one
// 4-byte store for uint8) when p is aligned to it.
template <typename T>
L3U_DEV void store_quad(T* p, const T (&v)[4], bool whole, int n) {
  typedef typename vec4_of<T>::type V;
  constexpr int kPer = (int)(sizeof(V) / sizeof(T));   // 4, or 2 for double
  if (whole && (reinterpret_cast<uintptr_t>(p) & (sizeof(V) - 1)) == 0) {
#pragma unroll
    for (int h = 0; h < 4 / kPer; ++h) {
      V q;
#pragma unroll
      for (int j = 0; j < kPer; ++j) q[j] = v[h * kPer + j];
      reinterpret_cast<V*>(p)[h] = q;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < n) p[j] = v[j];
  }
}

L3U_DEV int clampi(int v, int n) { return min(max(v, 0), n - 1); }

// the thread's place in the workgroup and the loop bounds shared by both kernels
struct Walk {
  int tx, TX, nq;
  long long row0, rstride;
};
L3U_DEV Walk walk(int lgx, int oW) {
  Walk w;
  w.TX = 1 << lgx;
  w.tx = (int)threadIdx.x & (w.TX - 1);
  w.nq = (oW + 3) >> 2;
  const int RY = 256 >> lgx;
  w.row0 = (long long)blockIdx.x * RY + ((int)threadIdx.x >> lgx);
  w.rstride = (long long)gridDim.x * RY;
  return w;
}

// order 0: idx[oD + oH + oW] source indices, axis 0 first
template <typename T>
__global__ __launch_bounds__(256) void resample_nearest(const T* __restrict__ src, int D, int H,
                                                        int W, T* __restrict__ dst, int oD, int oH,
                                                        int oW, const int* __restrict__ idx,
                                                        int lgx) {
  const Walk k = walk(lgx, oW);
  const int* ix = idx + oD + oH;
  const long long nrows = (long long)oD * oH;
  for (int q = k.tx; q < k.nq; q += k.TX) {
    const int x0 = 4 * q;
    int xs[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) xs[j] = clampi(ix[min(x0 + j, oW - 1)], W);
    for (long long row = k.row0; row < nrows; row += k.rstride) {
      const int z = (int)row / oH, y = (int)row - z * oH;   // nrows < 2^31 (entry check)
      const T* srow = src + ((long long)clampi(idx[z], D) * H + clampi(idx[oD + y], H)) * W;
      T v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = srow[xs[j]];
      store_quad(dst + row * oW + x0, v, x0 + 3 < oW, oW - x0);
    }
  }
}

// order 1: lo / hi [oD + oH + oW] clamped corner indices and t the fraction, axis 0 first.  The
// value is the float64 sum over the 8 corners in C order (axis 0 the slowest bit, the low corner
// first), each term (((double)src * w0) * w1) * w2 with w = 1 - t at the low corner and t at the
// high one -- scipy's own association, which makes the result scipy's bit for bit --, every
// operation rounded on its own, then rounded once to float.
template <typename S>
__global__ __launch_bounds__(256) void resample_linear(const S* __restrict__ src, int D, int H,
                                                       int W, float* __restrict__ dst, int oD,
                                                       int oH, int oW, const int* __restrict__ lo,
                                                       const int* __restrict__ hi,
                                                       const double* __restrict__ t, int lgx) {
#pragma clang fp contract(off)
  const Walk k = walk(lgx, oW);
  const int xo = oD + oH;
  const long long nrows = (long long)oD * oH;
  for (int q = k.tx; q < k.nq; q += k.TX) {
    const int x0 = 4 * q;
    int xl[4], xh[4];
    double tx[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = xo + min(x0 + j, oW - 1);
      xl[j] = clampi(lo[x], W);
      xh[j] = clampi(hi[x], W);
      tx[j] = t[x];
    }
    for (long long row = k.row0; row < nrows; row += k.rstride) {
      const int z = (int)row / oH, y = (int)row - z * oH;   // nrows < 2^31 (entry check)
      const double tz = t[z], ty = t[oD + y];
      const long long zb[2] = {(long long)clampi(lo[z], D) * H, (long long)clampi(hi[z], D) * H};
      const int yb[2] = {clampi(lo[oD + y], H), clampi(hi[oD + y], H)};
      const S* r[4];        // the four source rows, (z bit, y bit) in C order
#pragma unroll
      for (int c = 0; c < 4; ++c) r[c] = src + (zb[c >> 1] + yb[c & 1]) * W;
      S s[4][8];            // all 4 x 8 loads are requested before the first multiply
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int c = 0; c < 8; ++c) s[j][c] = r[c >> 1][(c & 1) ? xh[j] : xl[j]];
      const double wz[2] = {1.0 - tz, tz}, wy[2] = {1.0 - ty, ty};
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double wx[2] = {1.0 - tx[j], tx[j]};
        double acc = 0.0;
#pragma unroll
        for (int c = 0; c < 8; ++c)
          acc = acc + (((double)s[j][c] * wz[c >> 2]) * wy[(c >> 1) & 1]) * wx[c & 1];
        v[j] = (float)acc;
      }
      store_quad(dst + row * oW + x0, v, x0 + 3 < oW, oW - x0);
    }
  }
}

struct Launch { int grid, lgx; };
L3U_INLINE_HOST Launch plan(int oD, int oH, int oW) {
  const int nq = (oW + 3) / 4;
  int lgx = 0;
  while (lgx < 8 && (1 << lgx) < nq) ++lgx;
  const long long RY = 256 >> lgx, groups = ((long long)oD * oH + RY - 1) / RY;
  return {(int)(groups < 2048 ? groups : 2048), lgx};
}

L3U_INLINE_HOST bool dims_ok(int D, int H, int W) {
  return D > 0 && H > 0 && W > 0 && (long long)D * H < (1ll << 31) &&
         (long long)D * H * W < (1ll << 40);
}

}  // namespace
}  // namespace l3u

using namespace l3u;

extern "C" int l3u_resample(const void* src, int src_dtype, int D, int H, int W, void* dst,
                            int dst_dtype, int oD, int oH, int oW, int order, const int* lo,
                            const int* hi, const double* t, hipStream_t stream) {
  L3U_REQUIRE(src && dst && src != dst && lo && dims_ok(D, H, W) && dims_ok(oD, oH, oW));
  L3U_REQUIRE(order == 0 || order == 1);
  const Launch p = plan(oD, oH, oW);
  if (order == 1) {
    L3U_REQUIRE(hi && t && dst_dtype == 0 && (src_dtype == 0 || src_dtype == 1));
    float* d = static_cast<float*>(dst);
    if (src_dtype == 0)
      resample_linear<float><<<p.grid, 256, 0, stream>>>(static_cast<const float*>(src), D, H, W, d,
                                                         oD, oH, oW, lo, hi, t, p.lgx);
    else
      resample_linear<double><<<p.grid, 256, 0, stream>>>(static_cast<const double*>(src), D, H, W,
                                                          d, oD, oH, oW, lo, hi, t, p.lgx);
    L3U_CHECK_LAUNCH();
  }
  L3U_REQUIRE(dst_dtype == src_dtype && src_dtype >= 0 && src_dtype <= 2);
  switch (src_dtype) {
    case 0:
      resample_nearest<float><<<p.grid, 256, 0, stream>>>(
          static_cast<const float*>(src), D, H, W, static_cast<float*>(dst), oD, oH, oW, lo, p.lgx);
      break;
    case 1:
      resample_nearest<double><<<p.grid, 256, 0, stream>>>(
          static_cast<const double*>(src), D, H, W, static_cast<double*>(dst), oD, oH, oW, lo, p.lgx);
      break;
    default:
      resample_nearest<unsigned char><<<p.grid, 256, 0, stream>>>(
          static_cast<const unsigned char*>(src), D, H, W, static_cast<unsigned char*>(dst), oD, oH,
          oW, lo, p.lgx);
  }
  L3U_CHECK_LAUNCH();
}
