// Surface-distance metrics on the device (light_unet/surface.py): an exact anisotropic 3D Euclidean
// distance transform over a bit-packed feature mask, the surface of a packed mask, and the
// reductions of a distance map over surface voxels (count, max, fixed-order fp64 sum, counts within
// tolerances, and the distances laid out for l3u_pp_select).
//
// The transform's contract is a float minimum: out = sqrt(min over features f of
// fl(fl(((z-fz)sz)^2 + ((y-fy)sy)^2) + ((x-fx)sx)^2)), every product and sum rounded to fp64 on its
// own -- scipy.ndimage.distance_transform_edt's own arithmetic.  Rounding is monotone, so the
// minimum separates into three line passes, each  h[j] = min_i fl(g[i] + fl(((j - i) s)^2)):
//   z: g is 0 at features and +inf elsewhere, so the pass is "the nearest feature of the column":
//      one thread per (y, x) column, a sweep up and a sweep down, coalesced across x;
//   y, x: a scan outwards from j over i = j -+ k that stops once fl((k s)^2) >= the best value so
//      far -- exact, because g >= 0 makes every farther candidate at least that large -- and is
//      bounded by the line length whatever the data.  A workgroup stages the whole line in LDS when
//      it has at most 512 elements, else a window of it (256 outputs plus a halo of 128 either
//      side); a candidate beyond the window is read from the pass's input in global memory, which
//      the pass never writes (the passes ping-pong between two buffers), so a line of any length
//      works.
// No lower envelope, no floating intersection points, no per-thread stack.  This file is compiled
// with -ffp-contract=off (Makefile) and every arithmetic function turns contraction off itself.
#include "common.h"

#include <math.h>

namespace l3u {
namespace {

typedef unsigned long long u64;

// y pass: a workgroup owns 16 x (one 128-byte line of doubles) of one z; x pass: 8 rows.  A line of at most kWin elements is staged whole (every candidate is in LDS); a
// longer one in windows of kOut outputs with kHalo elements either side (kWin in all).
constexpr int kYW = 16, kXRows = 8;
constexpr int kWin = 512, kOut = 256, kHalo = 128;   // y: 512 x 16 doubles = 64 KB at most; x: 32 KB
constexpr int kRedBlock = 4096;                     // voxels per reduction partial
constexpr int kRedVals = 12;                        // doubles per partial (11 used)
constexpr int kMaxTol = 8;

struct Tol { double v[kMaxTol]; };

L3U_INLINE_HOST int words_per_row(int W) { return (W + 63) / 64; }
L3U_INLINE_HOST bool dims_ok(int D, int H, int W) {
  return D > 0 && H > 0 && W > 0 && (long long)D * H * W < (1ll << 31);
}

// fl((k s)^2): the index difference times the spacing, rounded, then squared, rounded
L3U_DEV double sq_step(int k, double s) {
#pragma clang fp contract(off)
  const double d = (double)k * s;
  return d * d;
}

// ---- z pass: nearest feature of each (y, x) column ----------------------------------------------
__global__ __launch_bounds__(256) void edt_z(const u64* __restrict__ feat, double* __restrict__ g,
                                             double sz, int D, int H, int W, int WW) {
#pragma clang fp contract(off)
  const long long plane = (long long)H * W, fplane = (long long)H * WW;
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  if (c >= plane) return;
  const int y = (int)(c / W), x = (int)(c - (long long)y * W);
  const u64* fw = feat + (long long)y * WW + (x >> 6);
  const int sh = x & 63;
  int last = -1;
  for (int z = 0; z < D; ++z) {
    if ((fw[z * fplane] >> sh) & 1ull) last = z;
    g[z * plane + c] = last >= 0 ? sq_step(z - last, sz) : INFINITY;
  }
  int next = -1;
  for (int z = D - 1; z >= 0; --z) {
    if ((fw[z * fplane] >> sh) & 1ull) next = z;
    if (next >= 0) {
      const double v = sq_step(next - z, sz);
      double* p = g + z * plane + c;
      if (v < *p) *p = v;
    }
  }
}

// ---- the line minimum of the y and x passes ------------------------------------------------------
// win: the staged window, element i of the line at win[(i - wlo) * wstride] for wlo <= i < whi;
// line: element i of the line at line[i * lstride] in global memory (the pass's input).
L3U_DEV double line_min(const double* win, int wstride, int wlo, int whi,
                        const double* __restrict__ line, long long lstride, int j, int n, double s) {
#pragma clang fp contract(off)
  double best = win[(j - wlo) * wstride];   // j is always inside its own window
  const int kmax = max(j, n - 1 - j);       // the scan never leaves the line
  for (int k = 1; k <= kmax; ++k) {
    const double q = sq_step(k, s);
    if (!(q < best)) break;                 // g >= 0: nothing at distance >= k can be smaller
    const int a = j - k, b = j + k;
    if (a >= 0) {
      const double ga = a >= wlo ? win[(a - wlo) * wstride] : line[a * lstride];
      const double v = ga + q;
      best = v < best ? v : best;
    }
    if (b < n) {
      const double gb = b < whi ? win[(b - wlo) * wstride] : line[b * lstride];
      const double v = gb + q;
      best = v < best ? v : best;
    }
  }
  return best;
}

// The window plan of a line of n elements: the outputs per workgroup and the workgroups per line.
struct Plan { int out, tiles, win; };
L3U_INLINE_HOST Plan plan(int n) {
  if (n <= kWin) return {n, 1, n};
  return {kOut, (n + kOut - 1) / kOut, kWin};
}

// ---- y pass: a workgroup owns (z, `yo` output rows, 16 x) ------------------------------------------
__global__ __launch_bounds__(256) void edt_y(const double* __restrict__ in, double* __restrict__ out,
                                             double sy, int D, int H, int W, int yo, int nyt, int nxt) {
  extern __shared__ double edt_win[];
  int b = (int)blockIdx.x;
  const int xt = b % nxt;
  b /= nxt;
  const int yt = b % nyt, z = b / nyt;
  if (z >= D) return;
  const int tx = (int)threadIdx.x & (kYW - 1), ty = (int)threadIdx.x / kYW;
  constexpr int kTY = 256 / kYW;
  const int x = xt * kYW + tx, y0 = yt * yo, y1 = min(y0 + yo, H);
  const int wlo = max(y0 - kHalo, 0), whi = min(y1 + kHalo, H);   // whi - wlo <= the staged rows
  const bool xin = x < W;
  const double* col = in + (long long)z * H * W + (xin ? x : 0);
  for (int wy = wlo + ty; wy < whi; wy += kTY)
    edt_win[(wy - wlo) * kYW + tx] = xin ? col[(long long)wy * W] : INFINITY;
  __syncthreads();
  if (!xin) return;
  for (int y = y0 + ty; y < y1; y += kTY)
    out[((long long)z * H + y) * W + x] = line_min(edt_win + tx, kYW, wlo, whi, col, W, y, H, sy);
}

// ---- x pass: a workgroup owns 8 rows by `xo` output x; writes the square root ----------------------
__global__ __launch_bounds__(256) void edt_x(const double* __restrict__ in, double* __restrict__ out,
                                             double sx, long long nrows, int W, int xo, int nxt,
                                             int win) {
  extern __shared__ double edt_win[];
  const long long blk = blockIdx.x;
  const int xt = (int)(blk % nxt);
  const long long r0 = (blk / nxt) * kXRows;
  const int t = (int)threadIdx.x, x0 = xt * xo, x1 = min(x0 + xo, W);
  const int wlo = max(x0 - kHalo, 0), whi = min(x1 + kHalo, W);   // whi - wlo <= win
  for (int u = 0; u < kXRows; ++u) {
    const long long r = r0 + u;
    if (r >= nrows) break;
    const double* row = in + r * W;
    for (int i = wlo + t; i < whi; i += 256) edt_win[u * win + (i - wlo)] = row[i];
  }
  __syncthreads();
  for (int u = 0; u < kXRows; ++u) {
    const long long r = r0 + u;
    if (r >= nrows) break;
    for (int x = x0 + t; x < x1; x += 256) {
      const double m = line_min(edt_win + u * win, 1, wlo, whi, in + r * W, 1, x, W, sx);
      out[r * W + x] = sqrt(m);
    }
  }
}

// ---- surface of a packed mask: A & ~erode6(A), outside the volume 0 --------------------------------
__global__ __launch_bounds__(256) void surf_mask(const u64* __restrict__ in, u64* __restrict__ out,
                                                 int D, int H, int WW) {
  const long long nw = (long long)D * H * WW, rowsz = WW, plane = (long long)H * WW;
  const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
  if (w >= nw) return;
  const long long row = w / WW;
  const int wx = (int)(w - row * WW), z = (int)(row / H), y = (int)(row - (long long)z * H);
  const u64 c = in[w];
  const u64 l = wx > 0 ? in[w - 1] : 0ull, r = wx < WW - 1 ? in[w + 1] : 0ull;
  const u64 up = y > 0 ? in[w - rowsz] : 0ull, dn = y < H - 1 ? in[w + rowsz] : 0ull;
  const u64 fr = z > 0 ? in[w - plane] : 0ull, bk = z < D - 1 ? in[w + plane] : 0ull;
  const u64 xm = (c << 1) | (l >> 63), xp = (c >> 1) | (r << 63);   // padding bits are 0
  out[w] = c & ~(xm & xp & up & dn & fr & bk);
}

// ---- reductions over surface voxels ----------------------------------------------------------------
// Partial b covers the voxels [b * 4096, (b + 1) * 4096) of the flat order: a thread adds its 16
// voxels in index order, the workgroup adds its threads in the fixed order of block_sum256d.  The
// launch shape is a function of the volume alone, so the same input gives the same bits.
__global__ __launch_bounds__(256) void surf_partial(const double* __restrict__ dist,
                                                    const u64* __restrict__ surf, Tol tol, int T,
                                                    double* __restrict__ sd, double* __restrict__ part,
                                                    long long n, int W, int WW) {
  __shared__ double red[4];
  __shared__ unsigned cnt[1 + kMaxTol];
  __shared__ u64 mx;
  const int t = (int)threadIdx.x;
  if (t < 1 + kMaxTol) cnt[t] = 0;
  if (t == 0) mx = 0;
  __syncthreads();
  const long long base = (long long)blockIdx.x * kRedBlock;
  double sum = 0.0, dmax = 0.0;
  unsigned c0 = 0, ct[kMaxTol];
#pragma unroll
  for (int q = 0; q < kMaxTol; ++q) ct[q] = 0;
  for (int u = 0; u < kRedBlock / 256; ++u) {
    const long long i = base + u * 256 + t;
    if (i >= n) break;
    const long long row = i / W;
    const int x = (int)(i - row * W);
    const bool on = (surf[row * WW + (x >> 6)] >> (x & 63)) & 1ull;
    const double d = dist[i];
    sd[i] = on ? d : INFINITY;
    if (on) {
      ++c0;
      sum += d;
      dmax = d > dmax ? d : dmax;
#pragma unroll
      for (int q = 0; q < kMaxTol; ++q) ct[q] += (q < T && d <= tol.v[q]) ? 1u : 0u;
    }
  }
  const double bsum = block_sum256d(sum, red);
  // integer atomics in LDS: exact and order-independent (distances are >= 0, so their bit patterns
  // order as unsigned integers)
  if (c0) {
    atomicAdd(&cnt[0], c0);
    atomicMax(&mx, (u64)__double_as_longlong(dmax));
#pragma unroll
    for (int q = 0; q < kMaxTol; ++q)
      if (ct[q]) atomicAdd(&cnt[1 + q], ct[q]);
  }
  __syncthreads();
  double* p = part + (long long)blockIdx.x * kRedVals;
  if (t == 0) {
    p[0] = (double)cnt[0];
    p[1] = __longlong_as_double((long long)mx);
    p[2] = bsum;
  }
  if (t < kMaxTol) p[3 + t] = (double)cnt[1 + t];
}

// One wave: lane l adds the partials l, l + 64, ... in index order, then value q of the 64 lanes
// is combined in lane order.  res[11] = count, max, sum, counts within the tolerances.
__global__ __launch_bounds__(64) void surf_merge(const double* __restrict__ part, int nb,
                                                 double* __restrict__ res) {
  __shared__ double sh[64 * kRedVals];
  const int l = (int)threadIdx.x;
  double a[11];
#pragma unroll
  for (int q = 0; q < 11; ++q) a[q] = 0.0;
  for (int b = l; b < nb; b += 64) {
    const double* p = part + (long long)b * kRedVals;
#pragma unroll
    for (int q = 0; q < 11; ++q) {
      const double v = p[q];
      a[q] = q == 1 ? (v > a[q] ? v : a[q]) : a[q] + v;
    }
  }
#pragma unroll
  for (int q = 0; q < 11; ++q) sh[l * kRedVals + q] = a[q];
  __syncthreads();
  if (l < 11) {
    double r = 0.0;
    for (int k = 0; k < 64; ++k) {
      const double v = sh[k * kRedVals + l];
      r = l == 1 ? (v > r ? v : r) : r + v;
    }
    res[l] = r;
  }
}

}  // namespace
}  // namespace l3u

using namespace l3u;

extern "C" int l3u_edt(const unsigned long long* feat, double sz, double sy, double sx, double* out,
                       double* tmp, int D, int H, int W, int passes, hipStream_t stream) {
  L3U_REQUIRE(feat && out && tmp && out != tmp && dims_ok(D, H, W));
  L3U_REQUIRE(sz > 0.0 && sy > 0.0 && sx > 0.0 && passes >= 1 && passes <= 7);
  const int WW = words_per_row(W);
  const long long plane = (long long)H * W, nrows = (long long)D * H;
  if (passes & 1)
    edt_z<<<(unsigned)((plane + 255) / 256), 256, 0, stream>>>(feat, out, sz, D, H, W, WW);
  if (passes & 2) {
    const Plan p = plan(H);
    const int nxt = (W + kYW - 1) / kYW;
    const size_t lds = (size_t)p.win * kYW * sizeof(double);
    edt_y<<<(unsigned)((long long)D * p.tiles * nxt), 256, lds, stream>>>(out, tmp, sy, D, H, W, p.out,
                                                                         p.tiles, nxt);
  }
  if (passes & 4) {
    const Plan p = plan(W);
    const long long nrb = (nrows + kXRows - 1) / kXRows;
    const size_t lds = (size_t)kXRows * p.win * sizeof(double);
    edt_x<<<(unsigned)(nrb * p.tiles), 256, lds, stream>>>(tmp, out, sx, nrows, W, p.out, p.tiles,
                                                          p.win);
  }
  L3U_CHECK_LAUNCH();
}

extern "C" int l3u_surf_mask(const unsigned long long* in, unsigned long long* out, int D, int H,
                             int W, hipStream_t stream) {
  L3U_REQUIRE(in && out && in != out && dims_ok(D, H, W));
  const int WW = words_per_row(W);
  const long long nw = (long long)D * H * WW;
  surf_mask<<<(unsigned)((nw + 255) / 256), 256, 0, stream>>>(in, out, D, H, WW);
  L3U_CHECK_LAUNCH();
}

extern "C" int l3u_surf_nblocks(long long n) {
  return n > 0 && n < (1ll << 31) ? (int)((n + kRedBlock - 1) / kRedBlock) : 0;
}

extern "C" int l3u_surf_reduce(const double* dist, const unsigned long long* surf, const double* tol,
                               int ntol, double* sd, double* part, double* res, int D, int H, int W,
                               hipStream_t stream) {
  L3U_REQUIRE(dist && surf && sd && part && res && dist != sd && dims_ok(D, H, W));
  L3U_REQUIRE(ntol >= 0 && ntol <= kMaxTol && (ntol == 0 || tol));
  Tol t;
  for (int q = 0; q < kMaxTol; ++q) t.v[q] = q < ntol ? tol[q] : 0.0;
  const long long n = (long long)D * H * W;
  const int nb = (int)((n + kRedBlock - 1) / kRedBlock);
  surf_partial<<<nb, 256, 0, stream>>>(dist, surf, t, ntol, sd, part, n, W, words_per_row(W));
  surf_merge<<<1, 64, 0, stream>>>(part, nb, res);
  L3U_CHECK_LAUNCH();
}
