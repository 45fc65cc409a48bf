// Cubic B-spline resampling of a [D, H, W] volume (light_unet/resample.py: resample_spline): the
// semantics of scipy.ndimage.zoom(x, zoom, order=3, mode="nearest", grid_mode=True), by the
// contract written out in include/l3u.h -- the volume padded by 12 edge voxels per side, the
// recursive prefilter along axis 0, 1 and 2 in float64, then a 64-tap gather through host tables.
// This file is compiled with -ffp-contract=off (Makefile): every fp64 product, sum and difference
// is rounded on its own, and each line's recursion runs in index order in one thread, so the
// coefficients and the output do not depend on the launch shape.  No atomics.
//
// Prefilter, axis 0 and axis 1 (spline_lines): one thread per line, consecutive threads on
// consecutive x, so every load and store of a wave is one contiguous run.  The axis-0 pass reads
// the source through clamped indices and writes the padded volume (there is no pad kernel and no
// float64 copy of the source); the axis-1 pass runs in place.  A thread requests 8 elements of its
// line before it walks them: the dependent chain (2 fp64 operations per element) waits for memory
// once per 8 elements, and the other waves of the SIMD cover the chain's own latency.
//
// Prefilter, axis 2 (spline_rows): the lines are contiguous, so a workgroup stages a tile of 256
// rows x 16 doubles through LDS with coalesced 8-byte loads (16 lanes per row segment of 128
// bytes); thread r walks row r of the tile, its carry in a register from chunk to chunk, forwards
// for the causal sweep and then backwards for the anticausal one.  The tile's row pitch is 17
// doubles: the column walk's ds_read_b64 of 32 lanes then falls on 32 different bank pairs
// ((34 r) mod 64), where a pitch of 16 would put all of them on one.
//
// Gather (spline_gather): resample_linear's work split (csrc/resample.hip) -- a thread owns 4
// consecutive output x, reads their table entries once and walks the output rows (z, y) in a
// grid-stride loop; rows wider than 1024 take further columns in an outer loop; the quad is stored
// as one vector where it is whole and aligned.  The 4 x 4 x (4..7) coefficient neighbourhood of a
// quad comes through the vector L1 / L2 (the 16 loads of one (a, b) tap row are adjacent doubles);
// nothing is staged in LDS.  Offsets are long long.
#include "common.h"

namespace l3u {
namespace {

constexpr int kPad = 12;                       // edge voxels per side (scipy's pad for "nearest")
constexpr int kRows = 256, kChunk = 16, kPitch = kChunk + 1;

struct Pole { double z, lam, k0, kn; };

L3U_DEV int clampi(int v, int n) { return min(max(v, 0), n - 1); }

// One line in place: c[i * stride], i < n; ld(i) is the element's value before the pass.
//   c[i] = c[i] * lam;  c[0] = c[0] * k0;  c[i] = c[i] + z * c[i-1];
//   c[n-1] = kn * c[n-1];  c[i] = z * (c[i+1] - c[i]) downwards
template <typename Load>
L3U_DEV void filter_line(double* c, long long stride, int n, const Pole& k, Load ld) {
  double carry = 0.0;
  for (int i0 = 0; i0 < n; i0 += 8) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = ld(min(i0 + u, n - 1));
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (i0 + u < n) {
        const double s = v[u] * k.lam;
        carry = i0 + u == 0 ? s * k.k0 : s + k.z * carry;
        c[(i0 + u) * stride] = carry;
      }
  }
  carry = k.kn * carry;
  c[(n - 1) * stride] = carry;
  for (int i0 = n - 2; i0 >= 0; i0 -= 8) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = c[max(i0 - u, 0) * stride];
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (i0 - u >= 0) {
        carry = k.z * (carry - v[u]);
        c[(i0 - u) * stride] = carry;
      }
  }
}

// axis 0: the lines (i1, i2) of coef[D + 24][Hp][Wp], read from src[D][H][W] through clamped
// indices; blockIdx.y strides over i1
template <typename S>
__global__ __launch_bounds__(256) void spline_lines_axis0(const S* __restrict__ src, int D, int H,
                                                          int W, double* __restrict__ coef,
                                                          Pole k) {
  const int Hp = H + 2 * kPad, Wp = W + 2 * kPad;
  const int i2 = (int)(blockIdx.x * 256 + threadIdx.x);
  if (i2 >= Wp) return;
  const long long plane = (long long)H * W;
  for (int i1 = (int)blockIdx.y; i1 < Hp; i1 += (int)gridDim.y) {
    const S* s = src + (long long)clampi(i1 - kPad, H) * W + clampi(i2 - kPad, W);
    filter_line(coef + (long long)i1 * Wp + i2, (long long)Hp * Wp, D + 2 * kPad, k,
                [&](int i) { return (double)s[clampi(i - kPad, D) * plane]; });
  }
}

// axis 1: the lines (i0, i2) of coef[Dp][Hp][Wp] in place; blockIdx.y strides over i0
__global__ __launch_bounds__(256) void spline_lines_axis1(double* coef, int Dp, int Hp, int Wp,
                                                          Pole k) {
  const int i2 = (int)(blockIdx.x * 256 + threadIdx.x);
  if (i2 >= Wp) return;
  for (int i0 = (int)blockIdx.y; i0 < Dp; i0 += (int)gridDim.y) {
    double* c = coef + (long long)i0 * Hp * Wp + i2;
    filter_line(c, (long long)Wp, Hp, k, [&](int i) { return c[(long long)i * Wp]; });
  }
}

// axis 2: the nrows contiguous lines of n doubles each, in place, 256 rows per workgroup.  Four
// workgroups per CU (4 x 34 KiB of LDS; the register bound keeps the tile move from being unrolled
// into 173 VGPRs, which held a CU to two): the 702 workgroups of a 400 x 400 x 600 case are then
// resident at once instead of in two rounds, 0.98 - 1.07 ms against 1.57 ms for that pass.
__global__ __launch_bounds__(256, 4) void spline_rows(double* coef, long long nrows, int n, Pole k) {
  __shared__ double tile[kRows * kPitch];
  const int t = (int)threadIdx.x, col = t & (kChunk - 1), rsub = t >> 4;   // 16 rows per load step
  const int last = (n - 1) / kChunk * kChunk;
  for (long long r0 = (long long)blockIdx.x * kRows; r0 < nrows; r0 += (long long)gridDim.x * kRows) {
    const int rows = (int)min((long long)kRows, nrows - r0);
    double* base = coef + r0 * n;
    double carry = 0.0;
    // a tile moves between global memory and LDS with one thread-to-element mapping in both
    // directions and in both sweeps: a thread reloads only what it stored itself
    auto move = [&](int x0, bool in) {
      const bool live = x0 + col < n;
      long long g = (long long)rsub * n + x0 + col;
      int l = rsub * kPitch + col;
#pragma unroll 8
      for (int r = rsub; r < kRows; r += 16, g += 16ll * n, l += 16 * kPitch)
        if (live && r < rows) {
          if (in) tile[l] = base[g]; else base[g] = tile[l];
        }
    };
    for (int x0 = 0; x0 <= last; x0 += kChunk) {            // causal, chunks upwards
      move(x0, true);
      __syncthreads();
      if (t < rows) {
        double* row = tile + t * kPitch;
#pragma unroll
        for (int j = 0; j < kChunk; ++j)
          if (x0 + j < n) {
            const double s = row[j] * k.lam;
            carry = x0 + j == 0 ? s * k.k0 : s + k.z * carry;
            row[j] = carry;
          }
      }
      __syncthreads();
      move(x0, false);
    }
    for (int x0 = last; x0 >= 0; x0 -= kChunk) {            // anticausal, chunks downwards
      move(x0, true);
      __syncthreads();
      if (t < rows) {
        double* row = tile + t * kPitch;
#pragma unroll
        for (int j = kChunk - 1; j >= 0; --j)
          if (x0 + j < n) {
            carry = x0 + j == n - 1 ? k.kn * row[j] : k.z * (carry - row[j]);
            row[j] = carry;
          }
      }
      __syncthreads();
      move(x0, false);
    }
  }
}

typedef float f4v __attribute__((ext_vector_type(4)));

// start[oD + oH + oW] / w[oD + oH + oW][4], axis 0 first; lgx as in csrc/resample.hip: a workgroup
// is 2^lgx quad columns x (256 >> lgx) rows
__global__ __launch_bounds__(256) void spline_gather(const double* __restrict__ coef, int Dp, int Hp,
                                                     int Wp, float* __restrict__ dst, int oD, int oH,
                                                     int oW, const int* __restrict__ start,
                                                     const double* __restrict__ w, float lo, float hi,
                                                     int use_clip, int lgx) {
  const int TX = 1 << lgx, tx = (int)threadIdx.x & (TX - 1), RY = 256 >> lgx;
  const int nq = (oW + 3) >> 2, xo = oD + oH;
  const long long nrows = (long long)oD * oH;
  const long long row0 = (long long)blockIdx.x * RY + ((int)threadIdx.x >> lgx);
  const long long rstride = (long long)gridDim.x * RY;
  for (int q = tx; q < nq; q += TX) {
    const int x0 = 4 * q;
    int xs[4];
    double wx[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = xo + min(x0 + j, oW - 1);
      xs[j] = clampi(start[x], Wp - 3);
#pragma unroll
      for (int c = 0; c < 4; ++c) wx[j][c] = w[4ll * x + c];
    }
    for (long long row = row0; row < nrows; row += rstride) {
      const int z = (int)row / oH, y = (int)row - z * oH;   // nrows < 2^31 (entry check)
      const int zs = clampi(start[z], Dp - 3), ys = clampi(start[oD + y], Hp - 3);
      double wz[4], wy[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        wz[a] = w[4ll * z + a];
        wy[a] = w[4ll * (oD + y) + a];
      }
      double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
      for (int a = 0; a < 4; ++a) {
        double v[4][4][4];          // the 64 loads of a plane are requested before its first product
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const double* r = coef + ((long long)(zs + a) * Hp + (ys + b)) * Wp;
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int c = 0; c < 4; ++c) v[b][j][c] = r[xs[j] + c];
        }
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int c = 0; c < 4; ++c)
              acc[j] = acc[j] + ((v[b][j][c] * wz[a]) * wy[b]) * wx[j][c];
      }
      float o[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        o[j] = (float)acc[j];
        if (use_clip) o[j] = fminf(fmaxf(o[j], lo), hi);
      }
      float* p = dst + row * oW + x0;
      if (x0 + 3 < oW && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        f4v v4 = {o[0], o[1], o[2], o[3]};
        *reinterpret_cast<f4v*>(p) = v4;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (x0 + j < oW) p[j] = o[j];
      }
    }
  }
}

L3U_INLINE_HOST bool dims_ok(long long D, long long H, long long W) {
  return D > 0 && H > 0 && W > 0 && D * H < (1ll << 31) && D * H * W < (1ll << 40);
}

}  // namespace
}  // namespace l3u

using namespace l3u;

extern "C" int l3u_spline_prefilter_passes(const void* src, int src_dtype, int D, int H, int W,
                                           double* coef, double z, double lam, double k0, double kn,
                                           int passes, hipStream_t stream) {
  L3U_REQUIRE(src && coef && src != (const void*)coef && (src_dtype == 0 || src_dtype == 1));
  L3U_REQUIRE(dims_ok(D, H, W) && dims_ok((long long)D + 2 * kPad, (long long)H + 2 * kPad,
                                          (long long)W + 2 * kPad));
  L3U_REQUIRE(passes > 0 && passes <= 7);
  const int Dp = D + 2 * kPad, Hp = H + 2 * kPad, Wp = W + 2 * kPad;
  const Pole k = {z, lam, k0, kn};
  const unsigned gx = (unsigned)((Wp + 255) / 256);
  if (passes & 1) {
    const dim3 grid(gx, (unsigned)min(Hp, 65535));
    if (src_dtype == 0)
      spline_lines_axis0<float><<<grid, 256, 0, stream>>>(static_cast<const float*>(src), D, H, W,
                                                          coef, k);
    else
      spline_lines_axis0<double><<<grid, 256, 0, stream>>>(static_cast<const double*>(src), D, H, W,
                                                           coef, k);
  }
  if (passes & 2)
    spline_lines_axis1<<<dim3(gx, (unsigned)min(Dp, 65535)), 256, 0, stream>>>(coef, Dp, Hp, Wp, k);
  if (passes & 4) {
    const long long nrows = (long long)Dp * Hp, groups = (nrows + kRows - 1) / kRows;
    spline_rows<<<(int)(groups < 4096 ? groups : 4096), 256, 0, stream>>>(coef, nrows, Wp, k);
  }
  L3U_CHECK_LAUNCH();
}

extern "C" int l3u_spline_prefilter(const void* src, int src_dtype, int D, int H, int W,
                                    double* coef, double z, double lam, double k0, double kn,
                                    hipStream_t stream) {
  return l3u_spline_prefilter_passes(src, src_dtype, D, H, W, coef, z, lam, k0, kn, 7, stream);
}

extern "C" int l3u_resample_spline(const double* coef, int D, int H, int W, float* dst, int oD,
                                   int oH, int oW, const int* start, const double* w, float clip_lo,
                                   float clip_hi, int use_clip, hipStream_t stream) {
  L3U_REQUIRE(coef && dst && (const void*)coef != (const void*)dst && start && w);
  L3U_REQUIRE(dims_ok(D, H, W) && dims_ok(oD, oH, oW) &&
              dims_ok((long long)D + 2 * kPad, (long long)H + 2 * kPad, (long long)W + 2 * kPad));
  const int nq = (oW + 3) / 4;
  int lgx = 0;
  while (lgx < 8 && (1 << lgx) < nq) ++lgx;
  const long long RY = 256 >> lgx, groups = ((long long)oD * oH + RY - 1) / RY;
  spline_gather<<<(int)(groups < 2048 ? groups : 2048), 256, 0, stream>>>(
      coef, D + 2 * kPad, H + 2 * kPad, W + 2 * kPad, dst, oD, oH, oW, start, w, clip_lo, clip_hi,
      use_clip, lgx);
  L3U_CHECK_LAUNCH();
}
