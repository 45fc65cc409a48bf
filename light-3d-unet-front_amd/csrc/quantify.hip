// Lesion uptake on the device (light_unet/quantify.py): the spherical mean around every lesion voxel
// (SUVpeak), the per-lesion reductions (count, fp64 sum, maximum and peak with their first voxels),
// and Dmax, the largest distance between two mask voxels, from the mask's corner voxels.
//
//   sphere mean   one workgroup per 4 x 8 x 64 output tile; a tile without a labelled voxel exits after
//                 reading its labels, otherwise the tile and its halo of uptake are staged in LDS
//                 (outside the volume: 0) and every labelled voxel adds the offset table in table order,
//                 in fp64, and divides by the number of offsets that stay inside the volume.
//   reductions    the host cuts every lesion's bounding box into z-slabs; one workgroup per (lesion,
//                 slab) item reduces in a fixed order, one thread per lesion merges its items in item
//                 order.  No float atomics: the same input gives the same bits.
//   corners       only a mask voxel that has, on each axis, a neighbour outside the mask can be an end
//                 of the farthest pair (a voxel between two mask voxels of one line is strictly closer
//                 to any third point than one of the two): a bit operation on the packed mask, then a
//                 prefix sum over popcounts compacts them to a coordinate list in ascending flat index.
//   farthest pair tiled all pairs over the upper triangle: a workgroup keeps 256 candidates in
//                 registers and walks tiles of 256 staged in LDS; the best (d2 bits, i, j) per
//                 workgroup, then one workgroup over the partials: the largest d2, then the smallest
//                 i, then the smallest j.
// Compiled with -ffp-contract=off (Makefile): d2 rounds every product and sum on its own.
#include "common.h"

#include <limits.h>
#include <math.h>

namespace l3u {
namespace {

typedef unsigned long long u64;

constexpr int kTZ = 4, kTY = 8, kTX = 64;   // the sphere mean's output tile: 256 threads x 8 voxels
constexpr int kMaxR = 4;                    // halo per side: (4 + 8)(8 + 8)(64 + 8) floats = 54 KB
constexpr int kMaxOff = 729;                // (2 * 4 + 1)^3
constexpr int kItemInts = 8;                // label, z0, z1, y0, y1, x0, x1 (ends exclusive), 0
constexpr int kVals = 8;                    // count, sum, max, its voxel, peak, its voxel, 0, 0
constexpr int kMaxCand = 1 << 18;
constexpr int kPairTile = 256, kPairGroup = 8;   // candidates per tile, j-tiles per workgroup

L3U_INLINE_HOST int words_per_row(int W) { return (W + 63) / 64; }
L3U_INLINE_HOST bool dims_ok(int D, int H, int W) {
  return D > 0 && H > 0 && W > 0 && (long long)D * H * W < (1ll << 31);
}

// ---- sphere mean ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void qt_peak(const float* __restrict__ up, const int* __restrict__ lab,
                                               const int* __restrict__ offs, int noff, int rz, int ry,
                                               int rx, double* __restrict__ peak, int D, int H, int W,
                                               int nty, int ntx) {
  extern __shared__ float qt_tile[];   // [SZ][SY][SX] floats, then rel[noff], then dzyx[noff]
  int b = (int)blockIdx.x;
  const int xt = b % ntx;
  b /= ntx;
  const int yt = b % nty, zt = b / nty;
  const int z0 = zt * kTZ, y0 = yt * kTY, x0 = xt * kTX;
  const int t = (int)threadIdx.x, lx = t & 63, lz = t >> 6;
  const int x = x0 + lx, z = z0 + lz;
  unsigned on = 0;
  if (x < W && z < D) {
#pragma unroll
    for (int u = 0; u < kTY; ++u) {
      const int y = y0 + u;
      if (y < H && lab[((long long)z * H + y) * W + x] > 0) on |= 1u << u;
    }
  }
  if (!__syncthreads_or(on != 0)) return;

  const int SZ = kTZ + 2 * rz, SY = kTY + 2 * ry, SX = kTX + 2 * rx;
  int* rel = reinterpret_cast<int*>(qt_tile + SZ * SY * SX);
  int* dzyx = rel + noff;
  for (int r = lz; r < SZ * SY; r += 4) {   // a wave per staged row
    const int iz = r / SY, iy = r - iz * SY;
    const int gz = z0 - rz + iz, gy = y0 - ry + iy;
    const bool rin = gz >= 0 && gz < D && gy >= 0 && gy < H;
    const float* row = up + ((long long)(rin ? gz : 0) * H + (rin ? gy : 0)) * W;
    for (int ix = lx; ix < SX; ix += 64) {
      const int gx = x0 - rx + ix;
      qt_tile[r * SX + ix] = (rin && gx >= 0 && gx < W) ? row[gx] : 0.f;
    }
  }
  for (int i = t; i < noff; i += 256) {
    const int dz = min(max(offs[i * 3], -rz), rz), dy = min(max(offs[i * 3 + 1], -ry), ry);
    const int dx = min(max(offs[i * 3 + 2], -rx), rx);   // never outside the staged halo
    rel[i] = (dz * SY + dy) * SX + dx;
    dzyx[i] = (dz + kMaxR) | ((dy + kMaxR) << 4) | ((dx + kMaxR) << 8);
  }
  __syncthreads();
  if (!on) return;
  const bool zx_in = z >= rz && z + rz < D && x >= rx && x + rx < W;
  for (int u = 0; u < kTY; ++u) {
    if (!((on >> u) & 1u)) continue;
    const int y = y0 + u;
    const float* c = qt_tile + ((lz + rz) * SY + (u + ry)) * SX + (lx + rx);
    double s = 0.0;
    for (int i = 0; i < noff; ++i) s += (double)c[rel[i]];   // outside the volume: + 0.0
    int n = noff;
    if (!(zx_in && y >= ry && y + ry < H)) {   // a border voxel counts the offsets that stay inside
      n = 0;
      for (int i = 0; i < noff; ++i) {
        const int q = dzyx[i];
        const int az = z + (q & 15) - kMaxR, ay = y + ((q >> 4) & 15) - kMaxR;
        const int ax = x + ((q >> 8) & 15) - kMaxR;
        n += (az >= 0 && az < D && ay >= 0 && ay < H && ax >= 0 && ax < W) ? 1 : 0;
      }
    }
    peak[((long long)z * H + y) * W + x] = s / (double)n;
  }
}

// ---- per-lesion reductions -----------------------------------------------------------------------
// (value, voxel) maximum of the workgroup: the larger value, among equal values the smaller voxel.
// A total order, so the tree gives one answer whatever its shape.
L3U_DEV void block_argmax(double& v, int& i, double* sv, int* si) {
  const int t = (int)threadIdx.x;
  sv[t] = v;
  si[t] = i;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) {
      const double ov = sv[t + s];
      const int oi = si[t + s];
      if (ov > sv[t] || (ov == sv[t] && oi < si[t])) {
        sv[t] = ov;
        si[t] = oi;
      }
    }
    __syncthreads();
  }
  v = sv[0];
  i = si[0];
  __syncthreads();
}

// One workgroup per item: the voxels of one label inside one z-slab of its bounding box.  A thread
// takes the box's voxels t, t + 256, ... in flat order (its first maximum is its smallest voxel),
// the workgroup adds its threads in the fixed order of block_sum256d.
__global__ __launch_bounds__(256) void qt_item_reduce(const float* __restrict__ up,
                                                      const int* __restrict__ lab,
                                                      const double* __restrict__ peak,
                                                      const int* __restrict__ items,
                                                      double* __restrict__ part, int D, int H, int W) {
  __shared__ double red[4];
  __shared__ double sv[256];
  __shared__ int si[256];
  __shared__ unsigned cnt;
  const int t = (int)threadIdx.x;
  const int* it = items + (long long)blockIdx.x * kItemInts;
  const int L = it[0];
  const int z0 = max(it[1], 0), z1 = min(it[2], D), y0 = max(it[3], 0), y1 = min(it[4], H);
  const int x0 = max(it[5], 0), x1 = min(it[6], W);
  if (t == 0) cnt = 0;
  __syncthreads();
  const int by = max(y1 - y0, 0), bx = max(x1 - x0, 0);
  const long long nb = (long long)max(z1 - z0, 0) * by * bx;
  unsigned c = 0;
  double sum = 0.0, mv = -INFINITY, pv = -INFINITY;
  int mi = INT_MAX, pi = INT_MAX;
  for (long long k = t; k < nb; k += 256) {
    const long long r = k / bx;
    const int xx = (int)(k - r * bx), zz = (int)(r / by), yy = (int)(r - (long long)zz * by);
    const long long idx = ((long long)(z0 + zz) * H + (y0 + yy)) * W + (x0 + xx);
    if (lab[idx] != L) continue;
    const double v = (double)up[idx];
    ++c;
    sum += v;
    if (v > mv) {
      mv = v;
      mi = (int)idx;
    }
    if (peak) {
      const double p = peak[idx];
      if (p > pv) {
        pv = p;
        pi = (int)idx;
      }
    }
  }
  const double bsum = block_sum256d(sum, red);
  if (c) atomicAdd(&cnt, c);   // an integer in LDS: exact and order-independent
  block_argmax(mv, mi, sv, si);
  block_argmax(pv, pi, sv, si);
  if (t == 0) {
    double* p = part + (long long)blockIdx.x * kVals;
    p[0] = (double)cnt;
    p[1] = bsum;
    p[2] = mv;
    p[3] = (double)mi;
    p[4] = pv;
    p[5] = (double)pi;
    p[6] = 0.0;
    p[7] = 0.0;
  }
}

// One thread per lesion: its items first[l] .. first[l + 1], in item order.
__global__ __launch_bounds__(64) void qt_item_merge(const double* __restrict__ part,
                                                    const int* __restrict__ first, int num,
                                                    double* __restrict__ res) {
  const int l = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (l >= num) return;
  double cnt = 0.0, sum = 0.0, mv = -INFINITY, mi = (double)INT_MAX, pv = -INFINITY,
         pi = (double)INT_MAX;
  for (int k = first[l]; k < first[l + 1]; ++k) {
    const double* p = part + (long long)k * kVals;
    cnt += p[0];
    sum += p[1];
    if (p[2] > mv || (p[2] == mv && p[3] < mi)) {
      mv = p[2];
      mi = p[3];
    }
    if (p[4] > pv || (p[4] == pv && p[5] < pi)) {
      pv = p[4];
      pi = p[5];
    }
  }
  double* r = res + (long long)l * kVals;
  r[0] = cnt;
  r[1] = sum;
  r[2] = mv;
  r[3] = mi;
  r[4] = pv;
  r[5] = pi;
  r[6] = 0.0;
  r[7] = 0.0;
}

// ---- corner voxels of a packed mask ----------------------------------------------------------------
// out = in & ~(x- & x+) & ~(y- & y+) & ~(z- & z+), everything outside the volume 0; bcnt[b] = the set
// bits of the 256 words of workgroup b.
__global__ __launch_bounds__(256) void qt_corners(const u64* __restrict__ in, u64* __restrict__ out,
                                                  int* __restrict__ bcnt, int D, int H, int WW) {
  __shared__ unsigned total;
  if (threadIdx.x == 0) total = 0;
  __syncthreads();
  const long long nw = (long long)D * H * WW, rowsz = WW, plane = (long long)H * WW;
  const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
  if (w < nw) {
    const long long row = w / WW;
    const int wx = (int)(w - row * WW), z = (int)(row / H), y = (int)(row - (long long)z * H);
    const u64 c = in[w];
    const u64 l = wx > 0 ? in[w - 1] : 0ull, r = wx < WW - 1 ? in[w + 1] : 0ull;
    const u64 up = y > 0 ? in[w - rowsz] : 0ull, dn = y < H - 1 ? in[w + rowsz] : 0ull;
    const u64 fr = z > 0 ? in[w - plane] : 0ull, bk = z < D - 1 ? in[w + plane] : 0ull;
    const u64 xm = (c << 1) | (l >> 63), xp = (c >> 1) | (r << 63);   // padding bits are 0
    const u64 o = c & ~(xm & xp) & ~(up & dn) & ~(fr & bk);
    out[w] = o;
    if (o) atomicAdd(&total, (unsigned)__popcll(o));
  }
  __syncthreads();
  if (threadIdx.x == 0) bcnt[blockIdx.x] = (int)total;
}

// One workgroup: pre[b] = the sum of cnt[0 .. b), pre[nb] = the total.
__global__ __launch_bounds__(256) void qt_scan(const int* __restrict__ cnt, int* __restrict__ pre,
                                               int nb) {
  __shared__ int sums[256];
  const int t = (int)threadIdx.x, per = (nb + 255) / 256;
  const int lo = min(t * per, nb), hi = min(lo + per, nb);
  int s = 0;
  for (int b = lo; b < hi; ++b) s += cnt[b];
  sums[t] = s;
  __syncthreads();
  int base = 0;
  for (int k = 0; k < t; ++k) base += sums[k];
  for (int b = lo; b < hi; ++b) {
    pre[b] = base;
    base += cnt[b];
  }
  if (t == 255) pre[nb] = base;
}

// cand[k] = (z, y, x, flat index) of the k-th set bit in ascending flat index.
__global__ __launch_bounds__(256) void qt_compact(const u64* __restrict__ bits,
                                                  const int* __restrict__ pre, int4* __restrict__ cand,
                                                  int ncand, int D, int H, int W, int WW) {
  __shared__ int scan[256];
  const int t = (int)threadIdx.x;
  const long long nw = (long long)D * H * WW;
  const long long w = (long long)blockIdx.x * 256 + t;
  u64 o = w < nw ? bits[w] : 0ull;
  const int mine = __popcll(o);
  scan[t] = mine;
  __syncthreads();
  for (int s = 1; s < 256; s <<= 1) {   // inclusive scan of the workgroup's popcounts
    const int v = t >= s ? scan[t - s] : 0;
    __syncthreads();
    scan[t] += v;
    __syncthreads();
  }
  if (!o) return;
  int k = pre[blockIdx.x] + scan[t] - mine;
  const long long row = w / WW;
  const int wx = (int)(w - row * WW), z = (int)(row / H), y = (int)(row - (long long)z * H);
  while (o) {
    const int bit = __ffsll((long long)o) - 1;
    o &= o - 1;
    const int x = wx * 64 + bit;
    if (k >= 0 && k < ncand && x < W) cand[k] = make_int4(z, y, x, (int)(row * W + x));
    ++k;
  }
}

// ---- farthest pair ---------------------------------------------------------------------------------
// the larger k1, among equal k1 the larger k2
L3U_DEV void block_max2(u64& k1, u64& k2, u64* s1, u64* s2) {
  const int t = (int)threadIdx.x;
  s1[t] = k1;
  s2[t] = k2;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) {
      const u64 a = s1[t + s], b = s2[t + s];
      if (a > s1[t] || (a == s1[t] && b > s2[t])) {
        s1[t] = a;
        s2[t] = b;
      }
    }
    __syncthreads();
  }
  k1 = s1[0];
  k2 = s2[0];
  __syncthreads();
}

// Workgroup (bi, g): candidates i of tile bi against the tiles max(bi, 8 g) .. 8 g + 7, pairs j > i.
// part[2 (bi * gridDim.y + g)] = the bits of the largest d2 (> 0 for two distinct voxels; 0: no pair)
// and ~(i << 32 | j), so that the larger second word is the smaller i, then the smaller j.
__global__ __launch_bounds__(256) void qt_pairs(const int4* __restrict__ cand, int n, double sz,
                                                double sy, double sx, u64* __restrict__ part, int T) {
#pragma clang fp contract(off)
  __shared__ int4 tile[kPairTile];
  __shared__ u64 s1[256], s2[256];
  const int t = (int)threadIdx.x, bi = (int)blockIdx.x, g = (int)blockIdx.y;
  const int jt0 = max(bi, g * kPairGroup), jt1 = min(T, (g + 1) * kPairGroup);
  u64 k1 = 0, k2 = 0;
  if (jt0 < jt1) {
    const int i = bi * kPairTile + t;
    const int4 ci = cand[min(i, n - 1)];
    double best = 0.0;
    int bj = -1;
    for (int jt = jt0; jt < jt1; ++jt) {
      __syncthreads();
      tile[t] = cand[min(jt * kPairTile + t, n - 1)];
      __syncthreads();
      const int m = min(kPairTile, n - jt * kPairTile);
      const int qmin = jt == bi ? t + 1 : 0;   // j > i
      for (int q = 0; q < m; ++q) {
        const int4 c = tile[q];
        const double a = (double)(c.x - ci.x) * sz, b = (double)(c.y - ci.y) * sy;
        const double e = (double)(c.z - ci.z) * sx;
        const double d2 = (a * a + b * b) + e * e;
        if (q >= qmin && d2 > best) {   // ascending j: the first maximum is the smallest j
          best = d2;
          bj = jt * kPairTile + q;
        }
      }
    }
    if (i < n && bj >= 0) {
      k1 = (u64)__double_as_longlong(best);
      k2 = ~(((u64)(unsigned)i << 32) | (u64)(unsigned)bj);
    }
    block_max2(k1, k2, s1, s2);
  }
  if (t == 0) {
    u64* p = part + 2 * ((long long)bi * gridDim.y + g);
    p[0] = k1;
    p[1] = k2;
  }
}

// res[3] = d2, the flat index of i, the flat index of j (0, -1, -1 without a pair)
__global__ __launch_bounds__(256) void qt_pairs_final(const u64* __restrict__ part, int np,
                                                      const int4* __restrict__ cand, int n,
                                                      double* __restrict__ res) {
  __shared__ u64 s1[256], s2[256];
  const int t = (int)threadIdx.x;
  u64 k1 = 0, k2 = 0;
  for (int b = t; b < np; b += 256) {
    const u64 a = part[2 * (long long)b], c = part[2 * (long long)b + 1];
    if (a > k1 || (a == k1 && c > k2)) {
      k1 = a;
      k2 = c;
    }
  }
  block_max2(k1, k2, s1, s2);
  if (t == 0) {
    if (k1 == 0) {
      res[0] = 0.0;
      res[1] = -1.0;
      res[2] = -1.0;
    } else {
      const u64 ij = ~k2;
      const int i = min((int)(ij >> 32), n - 1), j = min((int)(ij & 0xffffffffull), n - 1);
      res[0] = __longlong_as_double((long long)k1);
      res[1] = (double)cand[i].w;
      res[2] = (double)cand[j].w;
    }
  }
}

}  // namespace
}  // namespace l3u

using namespace l3u;

extern "C" int l3u_qt_peak(const float* uptake, const int* labels, const int* offs, int noff, int rz,
                           int ry, int rx, double* peak, int D, int H, int W, hipStream_t stream) {
  L3U_REQUIRE(uptake && labels && offs && peak && dims_ok(D, H, W));
  L3U_REQUIRE(noff >= 1 && noff <= kMaxOff && rz >= 0 && rz <= kMaxR && ry >= 0 && ry <= kMaxR &&
              rx >= 0 && rx <= kMaxR);
  const int ntz = (D + kTZ - 1) / kTZ, nty = (H + kTY - 1) / kTY, ntx = (W + kTX - 1) / kTX;
  const size_t lds = (size_t)(kTZ + 2 * rz) * (kTY + 2 * ry) * (kTX + 2 * rx) * sizeof(float) +
                     (size_t)noff * 2 * sizeof(int);
  qt_peak<<<(unsigned)((long long)ntz * nty * ntx), 256, lds, stream>>>(uptake, labels, offs, noff, rz,
                                                                        ry, rx, peak, D, H, W, nty, ntx);
  L3U_CHECK_LAUNCH();
}

extern "C" int l3u_qt_reduce(const float* uptake, const int* labels, const double* peak,
                             const int* items, int n_items, const int* first, int num, double* part,
                             double* res, int D, int H, int W, hipStream_t stream) {
  L3U_REQUIRE(uptake && labels && items && first && part && res && dims_ok(D, H, W));
  L3U_REQUIRE(n_items >= 1 && num >= 1 && num <= n_items);
  qt_item_reduce<<<n_items, 256, 0, stream>>>(uptake, labels, peak, items, part, D, H, W);
  qt_item_merge<<<(num + 63) / 64, 64, 0, stream>>>(part, first, num, res);
  L3U_CHECK_LAUNCH();
}

extern "C" int l3u_qt_corner_blocks(int D, int H, int W) {
  return dims_ok(D, H, W) ? (int)(((long long)D * H * words_per_row(W) + 255) / 256) : 0;
}

extern "C" int l3u_qt_corners(const unsigned long long* in, unsigned long long* out, int* bcnt,
                              int* bpre, int D, int H, int W, hipStream_t stream) {
  L3U_REQUIRE(in && out && in != out && bcnt && bpre && bcnt != bpre && dims_ok(D, H, W));
  const int nb = l3u_qt_corner_blocks(D, H, W);
  qt_corners<<<nb, 256, 0, stream>>>(in, out, bcnt, D, H, words_per_row(W));
  qt_scan<<<1, 256, 0, stream>>>(bcnt, bpre, nb);
  L3U_CHECK_LAUNCH();
}

extern "C" int l3u_qt_compact(const unsigned long long* bits, const int* bpre, int* cand, int ncand,
                              int D, int H, int W, hipStream_t stream) {
  L3U_REQUIRE(bits && bpre && cand && ncand >= 1 && dims_ok(D, H, W));
  qt_compact<<<l3u_qt_corner_blocks(D, H, W), 256, 0, stream>>>(
      bits, bpre, reinterpret_cast<int4*>(cand), ncand, D, H, W, words_per_row(W));
  L3U_CHECK_LAUNCH();
}

extern "C" int l3u_qt_pair_parts(int ncand) {
  if (ncand < 2 || ncand > kMaxCand) return 0;
  const int T = (ncand + kPairTile - 1) / kPairTile;
  return T * ((T + kPairGroup - 1) / kPairGroup);
}

extern "C" int l3u_qt_farthest(const int* cand, int ncand, double sz, double sy, double sx,
                               unsigned long long* part, double* res, hipStream_t stream) {
  L3U_REQUIRE(cand && part && res && ncand >= 2 && ncand <= kMaxCand);
  L3U_REQUIRE(sz > 0.0 && sy > 0.0 && sx > 0.0);
  const int T = (ncand + kPairTile - 1) / kPairTile, G = (T + kPairGroup - 1) / kPairGroup;
  const int4* c = reinterpret_cast<const int4*>(cand);
  qt_pairs<<<dim3(T, G), 256, 0, stream>>>(c, ncand, sz, sy, sx, part, T);
  qt_pairs_final<<<1, 256, 0, stream>>>(part, T * G, c, ncand, res);
  L3U_CHECK_LAUNCH();
}
