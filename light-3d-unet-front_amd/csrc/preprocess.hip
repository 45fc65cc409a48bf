// Case preprocessing on the device (the reference's scripts/preprocess_data.py): exact order
// statistics for np.percentile, the fp64 clip + normalise, and the body mask as a bit-packed
// volume with 6-neighbour morphology, population count and bounding box.
//
// Packed masks: one bit per voxel, x fastest, bit i of word wx of a row is x = 64 * wx + i (the
// lane order of a wave64 __ballot); a row (z, y) is WW = ceil(W / 64) words, padding bits are 0.
#include "common.h"

namespace l3u {
namespace {

typedef unsigned long long u64;
constexpr int kSelRanks = 4;   // order statistics tracked by one selection
// selection workspace (u64 words): prefix[4], remaining rank[4], group representative[4], NaN
// count, then the per-pass histograms (uint32 [8 passes][4 ranks][256 bins])
constexpr int kSelPre = 0, kSelK = 4, kSelRep = 8, kSelNan = 12, kSelHist = 16;
constexpr int kSelHistWords = 8 * kSelRanks * 256;   // uint32 words
constexpr size_t kSelBytes = kSelHist * sizeof(u64) + kSelHistWords * sizeof(unsigned);

// ---- monotone keys: a < b as numbers  <=>  key(a) < key(b) as unsigned; -0 counts as +0
L3U_DEV unsigned key_of(float v, bool& nan) {
  unsigned u = __float_as_uint(v);
  nan = (u & 0x7fffffffu) > 0x7f800000u;
  if ((u << 1) == 0u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
L3U_DEV u64 key_of(double v, bool& nan) {
  u64 u = (u64)__double_as_longlong(v);
  nan = (u & 0x7fffffffffffffffull) > 0x7ff0000000000000ull;
  if ((u << 1) == 0ull) u = 0ull;
  return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}
L3U_DEV double value_of(u64 key, bool f64) {
  if (f64) {
    const u64 u = (key & 0x8000000000000000ull) ? (key ^ 0x8000000000000000ull) : ~key;
    return __longlong_as_double((long long)u);
  }
  const unsigned k = (unsigned)key;
  const unsigned u = (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k;
  return (double)__uint_as_float(u);   // exact widening
}

__global__ void pp_sel_init(u64* ws, int nr, long long r0, long long r1, long long r2, long long r3) {
  const int t = threadIdx.x;
  if (t < kSelRanks) {
    const long long r = t == 0 ? r0 : (t == 1 ? r1 : (t == 2 ? r2 : r3));
    ws[kSelPre + t] = 0;
    ws[kSelK + t] = t < nr ? (u64)r : 0;
    ws[kSelRep + t] = 0;   // every rank starts in one group (the empty prefix)
  }
}

// One digit pass: count, per tracked prefix group, the byte `pass` (most significant first) of
// every key that carries the group's prefix.  Per-workgroup LDS histogram, flushed with integer
// atomics.  A wave whose matching lanes all hold one digit (runs of equal voxels: air) adds once.
template <typename T, typename K>
__global__ __launch_bounds__(256) void pp_sel_hist(const T* __restrict__ src, long long n, int pass,
                                                   int nb, int nr, u64* __restrict__ ws) {
  __shared__ unsigned h[kSelRanks * 256];
  __shared__ unsigned nan_cnt;
  const int tid = threadIdx.x, lane = tid & 63;
  for (int i = tid; i < kSelRanks * 256; i += 256) h[i] = 0;
  if (tid == 0) nan_cnt = 0;
  K pre[kSelRanks];
  bool act[kSelRanks];
#pragma unroll
  for (int r = 0; r < kSelRanks; ++r) {
    pre[r] = (K)ws[kSelPre + r];
    act[r] = r < nr && ws[kSelRep + r] == (u64)r;
  }
  __syncthreads();
  const int shift = 8 * (nb - 1 - pass);
  const long long stride = (long long)gridDim.x * 256;
  const long long nround = (n + 63) & ~63ll;   // whole waves run the loop together (ballots)
  for (long long i = (long long)blockIdx.x * 256 + tid; i < nround; i += stride) {
    const bool valid = i < n;
    bool nan = false;
    const K key = valid ? key_of(src[i], nan) : (K)0;
    if (pass == 0 && valid && nan) atomicAdd(&nan_cnt, 1u);
    const K hi = pass == 0 ? (K)0 : (K)(key >> (shift + 8));
    const int d = (int)((key >> shift) & 255);
#pragma unroll
    for (int r = 0; r < kSelRanks; ++r) {
      if (!act[r]) continue;
      const bool m = valid && !nan && (pass == 0 || hi == pre[r]);
      const u64 bm = __ballot(m);
      if (bm == 0) continue;
      const int first = __builtin_ctzll(bm);
      const int d0 = __builtin_amdgcn_readlane(d, first);
      const u64 same = __ballot(m && d == d0);
      if (same == bm) {
        if (lane == first) atomicAdd(&h[r * 256 + d0], (unsigned)__builtin_popcountll(bm));
      } else if (m) {
        atomicAdd(&h[r * 256 + d], 1u);
      }
    }
  }
  __syncthreads();
  unsigned* hist = reinterpret_cast<unsigned*>(ws + kSelHist) + pass * kSelRanks * 256;
  for (int i = tid; i < kSelRanks * 256; i += 256)
    if (h[i]) atomicAdd(&hist[i], h[i]);
  if (tid == 0 && nan_cnt) atomicAdd(&ws[kSelNan], (u64)nan_cnt);
}

// One workgroup: per rank, the bin of this pass that holds it and the rank inside that bin; then
// the groups of equal prefixes for the next pass.  The last pass writes the values (and the NaN
// count as out[4]).
__global__ __launch_bounds__(64) void pp_sel_pick(u64* __restrict__ ws, int pass, int nb, int nr,
                                                  int f64, double* __restrict__ out) {
  __shared__ unsigned h[kSelRanks * 256];
  __shared__ u64 npre[kSelRanks];
  const int t = threadIdx.x;
  const unsigned* hist = reinterpret_cast<const unsigned*>(ws + kSelHist) + pass * kSelRanks * 256;
  for (int i = t; i < kSelRanks * 256; i += 64) h[i] = hist[i];
  u64 pre = 0, k = 0;
  int g = 0;
  if (t < nr) {
    pre = ws[kSelPre + t];
    k = ws[kSelK + t];
    g = (int)ws[kSelRep + t];
  }
  __syncthreads();
  if (t < nr) {
    u64 cum = 0;
    int bin = 255;
    for (int b = 0; b < 256; ++b) {
      const u64 c = h[g * 256 + b];
      if (k < cum + c) { bin = b; break; }
      if (b < 255) cum += c;
    }
    pre = (pre << 8) | (u64)bin;
    k = k >= cum ? k - cum : 0;
    npre[t] = pre;
  }
  __syncthreads();
  if (t < nr) {
    int rep = t;
    for (int j = t - 1; j >= 0; --j)
      if (npre[j] == pre) rep = j;
    ws[kSelPre + t] = pre;
    ws[kSelK + t] = k;
    ws[kSelRep + t] = (u64)rep;
    if (pass == nb - 1) out[t] = value_of(pre, f64 != 0);
  }
  if (t == 0 && pass == nb - 1) out[kSelRanks] = (double)ws[kSelNan];
}

template <typename T, typename K>
int sel_launch(const T* src, long long n, int nr, u64* ws, double* out, int f64, hipStream_t st) {
  const int nb = (int)sizeof(K);
  const long long want = (n + 255) / 256;
  const int grid = (int)(want < 2048 ? want : 2048);
  for (int p = 0; p < nb; ++p) {
    pp_sel_hist<T, K><<<grid, 256, 0, st>>>(src, n, p, nb, nr, ws);
    pp_sel_pick<<<1, 64, 0, st>>>(ws, p, nb, nr, f64, out);
  }
  L3U_CHECK_LAUNCH();
}

// ---- packed masks --------------------------------------------------------------------------
L3U_INLINE_HOST int words_per_row(int W) { return (W + 63) / 64; }
L3U_INLINE_HOST int wave_grid(long long nwords) {
  const long long want = (nwords + 3) / 4;   // 4 waves per workgroup, one word per wave and step
  return (int)(want < 4096 ? (want < 1 ? 1 : want) : 4096);
}

// the reference's arithmetic, operation for operation in fp64 (np.clip, then (c - lo) / (hi - lo),
// then * (t1 - t0), then + t0): no contraction of the multiply and the add
L3U_DEV double normalize1(double x, double lo, double hi, double scale, double t0) {
#pragma clang fp contract(off)
  double c = x >= lo ? x : lo;
  c = c <= hi ? c : hi;
  double v = (c - lo) / (hi - lo);
  v = v * scale;
  v = v + t0;
  return v;
}

template <typename T>
__global__ __launch_bounds__(256) void pp_normalize(const T* __restrict__ src,
                                                    const double* __restrict__ clip, double scale,
                                                    double t0, double thr, double* __restrict__ o64,
                                                    float* __restrict__ o32, u64* __restrict__ bits,
                                                    long long nrows, int W, int WW) {
  const int lane = threadIdx.x & 63;
  const double lo = clip[0], hi = clip[1];
  const long long nw = nrows * WW, stride = (long long)gridDim.x * 4;
  for (long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); w < nw; w += stride) {
    const long long row = w / WW;
    const int x = (int)(w - row * WW) * 64 + lane;
    const bool valid = x < W;
    bool fg = false;
    if (valid) {
      const long long i = row * W + x;
      const double v = normalize1((double)src[i], lo, hi, scale, t0);
      if (o64) o64[i] = v;
      if (o32) o32[i] = (float)v;
      fg = v > thr;
    }
    const u64 bm = __ballot(fg);
    if (bits && lane == 0) bits[w] = bm;
  }
}

// op 0: v != 0, 1: v > arg, 2: v == arg (all compared as doubles: exact for every source type)
template <typename T>
__global__ __launch_bounds__(256) void pp_pack(const T* __restrict__ src, int op, double arg,
                                               u64* __restrict__ bits, long long nrows, int W,
                                               int WW) {
  const int lane = threadIdx.x & 63;
  const long long nw = nrows * WW, stride = (long long)gridDim.x * 4;
  for (long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); w < nw; w += stride) {
    const long long row = w / WW;
    const int x = (int)(w - row * WW) * 64 + lane;
    bool fg = false;
    if (x < W) {
      const double v = (double)src[row * W + x];
      fg = op == 0 ? v != 0.0 : (op == 1 ? v > arg : v == arg);
    }
    const u64 bm = __ballot(fg);
    if (lane == 0) bits[w] = bm;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void pp_unpack(const u64* __restrict__ bits, T* __restrict__ dst,
                                                 long long nrows, int W, int WW) {
  const long long n = nrows * W, stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const long long row = i / W;
    const int x = (int)(i - row * W);
    dst[i] = (T)((bits[row * WW + (x >> 6)] >> (x & 63)) & 1ull);
  }
}

// ---- 6-neighbour morphology ------------------------------------------------------------------
// A workgroup owns kTZ x kTY rows (all of x), stages them with a halo of `it` rows / planes into
// LDS, runs `it` iterations there (two buffers) and writes its rows.  Rows outside the volume are
// 0 at every iteration, for erosion too (scipy's border_value = 0).  Rows past the staged halo
// read as 0: what that gets wrong moves one row inwards per iteration and stops at the interior.
constexpr int kTZ = 8, kTY = 8;
constexpr int kMorphLds = 64 * 1024;

L3U_INLINE_HOST int morph_max_iters(int W) {
  const int WW = words_per_row(W);
  int it = 0;
  while (it < 8) {
    const long long rows = (long long)(kTZ + 2 * (it + 1)) * (kTY + 2 * (it + 1));
    if (2 * rows * WW * (long long)sizeof(u64) > kMorphLds) break;
    ++it;
  }
  return it;
}

__global__ __launch_bounds__(256) void pp_morph(const u64* __restrict__ in, u64* __restrict__ out,
                                                int erode, int it, int D, int H, int W, int WW) {
  extern __shared__ u64 pp_sm[];
  const int EZ = kTZ + 2 * it, EY = kTY + 2 * it, nw = EZ * EY * WW, plane = EY * WW;
  u64* a = pp_sm;
  u64* b = pp_sm + nw;
  const int z0 = (int)blockIdx.y * kTZ - it, y0 = (int)blockIdx.x * kTY - it;
  const u64 lastmask = (W & 63) ? ((1ull << (W & 63)) - 1ull) : ~0ull;
  for (int i = threadIdx.x; i < nw; i += 256) {
    const int row = i / WW, wx = i - row * WW, ez = row / EY, ey = row - ez * EY;
    const int z = z0 + ez, y = y0 + ey;
    const bool inside = z >= 0 && z < D && y >= 0 && y < H;
    a[i] = inside ? in[((long long)z * H + y) * WW + wx] : 0ull;
  }
  __syncthreads();
  for (int s = 0; s < it; ++s) {
    for (int i = threadIdx.x; i < nw; i += 256) {
      const int row = i / WW, wx = i - row * WW, ez = row / EY, ey = row - ez * EY;
      const int z = z0 + ez, y = y0 + ey;
      const bool inside = z >= 0 && z < D && y >= 0 && y < H;
      const u64 c = a[i];
      const u64 l = wx > 0 ? a[i - 1] : 0ull, r = wx < WW - 1 ? a[i + 1] : 0ull;
      const u64 up = ey > 0 ? a[i - WW] : 0ull, dn = ey < EY - 1 ? a[i + WW] : 0ull;
      const u64 fr = ez > 0 ? a[i - plane] : 0ull, bk = ez < EZ - 1 ? a[i + plane] : 0ull;
      const u64 xm = (c << 1) | (l >> 63), xp = (c >> 1) | (r << 63);
      u64 v = erode ? (c & xm & xp & up & dn & fr & bk) : (c | xm | xp | up | dn | fr | bk);
      if (wx == WW - 1) v &= lastmask;
      b[i] = inside ? v : 0ull;
    }
    __syncthreads();
    u64* t = a;
    a = b;
    b = t;
  }
  for (int i = threadIdx.x; i < kTZ * kTY * WW; i += 256) {
    const int row = i / WW, wx = i - row * WW, tz = row / kTY, ty = row - tz * kTY;
    const int z = z0 + it + tz, y = y0 + it + ty;
    if (z < D && y < H)
      out[((long long)z * H + y) * WW + wx] = a[((tz + it) * EY + (ty + it)) * WW + wx];
  }
}

// ---- population count and bounding box: stats[7] = count, min z, y, x, max z, y, x
__global__ void pp_stats_init(long long* stats) {
  const int t = threadIdx.x;
  if (t < 7) stats[t] = t == 0 ? 0ll : (t < 4 ? 0x7fffffffll : -1ll);
}

__global__ __launch_bounds__(256) void pp_stats(const u64* __restrict__ bits,
                                                long long* __restrict__ stats, long long nrows,
                                                int H, int WW) {
  __shared__ unsigned long long cnt;
  __shared__ int mn[3], mx[3];
  if (threadIdx.x == 0) cnt = 0;
  if (threadIdx.x < 3) { mn[threadIdx.x] = 0x7fffffff; mx[threadIdx.x] = -1; }
  __syncthreads();
  const long long nw = nrows * WW, stride = (long long)gridDim.x * 256;
  for (long long w = (long long)blockIdx.x * 256 + threadIdx.x; w < nw; w += stride) {
    const u64 v = bits[w];
    if (v == 0) continue;
    const long long row = w / WW;
    const int wx = (int)(w - row * WW), z = (int)(row / H), y = (int)(row - (long long)z * H);
    atomicAdd(&cnt, (unsigned long long)__builtin_popcountll(v));
    atomicMin(&mn[0], z);
    atomicMax(&mx[0], z);
    atomicMin(&mn[1], y);
    atomicMax(&mx[1], y);
    atomicMin(&mn[2], wx * 64 + __builtin_ctzll(v));
    atomicMax(&mx[2], wx * 64 + 63 - __builtin_clzll(v));
  }
  __syncthreads();
  if (threadIdx.x == 0 && cnt) atomicAdd(reinterpret_cast<unsigned long long*>(stats), cnt);
  if (threadIdx.x < 3 && mx[threadIdx.x] >= 0) {
    atomicMin(stats + 1 + threadIdx.x, (long long)mn[threadIdx.x]);
    atomicMax(stats + 4 + threadIdx.x, (long long)mx[threadIdx.x]);
  }
}

L3U_INLINE_HOST bool dims_ok(int D, int H, int W) {
  return D > 0 && H > 0 && W > 0 && (long long)D * H * W < (1ll << 40);
}

}  // namespace
}  // namespace l3u

using namespace l3u;

extern "C" int l3u_pp_select_ws_bytes(void) { return (int)kSelBytes; }

extern "C" int l3u_pp_select(const void* src, int is_f64, long long n, int nranks, long long r0,
                             long long r1, long long r2, long long r3, void* ws, double* out,
                             hipStream_t stream) {
  L3U_REQUIRE(src && ws && out && n > 0 && nranks >= 1 && nranks <= kSelRanks);
  const long long r[kSelRanks] = {r0, r1, r2, r3};
  for (int i = 0; i < nranks; ++i) L3U_REQUIRE(r[i] >= 0 && r[i] < n);
  u64* w = static_cast<u64*>(ws);
  const hipError_t e = hipMemsetAsync(ws, 0, kSelBytes, stream);
  if (e != hipSuccess) return (int)e;
  pp_sel_init<<<1, 64, 0, stream>>>(w, nranks, r0, r1, r2, r3);
  if (is_f64)
    return sel_launch<double, u64>(static_cast<const double*>(src), n, nranks, w, out, 1, stream);
  return sel_launch<float, unsigned>(static_cast<const float*>(src), n, nranks, w, out, 0, stream);
}

extern "C" int l3u_pp_normalize(const void* src, int is_f64, const double* clip, double scale,
                                double t0, double threshold, double* out64, float* out32,
                                unsigned long long* bits, int D, int H, int W, hipStream_t stream) {
  L3U_REQUIRE(src && clip && (out64 || out32 || bits) && dims_ok(D, H, W));
  const int WW = words_per_row(W);
  const long long nrows = (long long)D * H;
  const int grid = wave_grid(nrows * WW);
  if (is_f64)
    pp_normalize<double><<<grid, 256, 0, stream>>>(static_cast<const double*>(src), clip, scale, t0,
                                                   threshold, out64, out32, bits, nrows, W, WW);
  else
    pp_normalize<float><<<grid, 256, 0, stream>>>(static_cast<const float*>(src), clip, scale, t0,
                                                  threshold, out64, out32, bits, nrows, W, WW);
  L3U_CHECK_LAUNCH();
}

extern "C" int l3u_pp_pack(const void* src, int dtype, int op, double arg, unsigned long long* bits,
                           int D, int H, int W, hipStream_t stream) {
  L3U_REQUIRE(src && bits && dims_ok(D, H, W) && dtype >= 0 && dtype <= 3 && op >= 0 && op <= 2);
  const int WW = words_per_row(W);
  const long long nrows = (long long)D * H;
  const int grid = wave_grid(nrows * WW);
  switch (dtype) {
    case 0:
      pp_pack<float><<<grid, 256, 0, stream>>>(static_cast<const float*>(src), op, arg, bits, nrows, W, WW);
      break;
    case 1:
      pp_pack<double><<<grid, 256, 0, stream>>>(static_cast<const double*>(src), op, arg, bits, nrows, W, WW);
      break;
    case 2:
      pp_pack<unsigned char><<<grid, 256, 0, stream>>>(static_cast<const unsigned char*>(src), op, arg, bits, nrows, W, WW);
      break;
    default:
      pp_pack<int><<<grid, 256, 0, stream>>>(static_cast<const int*>(src), op, arg, bits, nrows, W, WW);
  }
  L3U_CHECK_LAUNCH();
}

extern "C" int l3u_pp_unpack(const unsigned long long* bits, void* dst, int dtype, int D, int H,
                             int W, hipStream_t stream) {
  L3U_REQUIRE(bits && dst && dims_ok(D, H, W) && (dtype == 0 || dtype == 2));
  const int WW = words_per_row(W);
  const long long nrows = (long long)D * H, want = (nrows * W + 255) / 256;
  const int grid = (int)(want < 8192 ? want : 8192);
  if (dtype == 0)
    pp_unpack<float><<<grid, 256, 0, stream>>>(bits, static_cast<float*>(dst), nrows, W, WW);
  else
    pp_unpack<unsigned char><<<grid, 256, 0, stream>>>(bits, static_cast<unsigned char*>(dst), nrows, W, WW);
  L3U_CHECK_LAUNCH();
}

extern "C" int l3u_pp_morph_max_iters(int W) { return W > 0 ? morph_max_iters(W) : 0; }

extern "C" int l3u_pp_morph(const unsigned long long* in, unsigned long long* out, int erode,
                            int iters, int D, int H, int W, hipStream_t stream) {
  L3U_REQUIRE(in && out && in != out && dims_ok(D, H, W));
  L3U_REQUIRE(iters >= 1 && iters <= morph_max_iters(W));
  const int WW = words_per_row(W);
  const size_t lds = 2 * (size_t)(kTZ + 2 * iters) * (kTY + 2 * iters) * WW * sizeof(u64);
  const dim3 grid((H + kTY - 1) / kTY, (D + kTZ - 1) / kTZ);
  L3U_REQUIRE(grid.y <= 65535u);
  pp_morph<<<grid, 256, lds, stream>>>(in, out, erode ? 1 : 0, iters, D, H, W, WW);
  L3U_CHECK_LAUNCH();
}

extern "C" int l3u_pp_mask_stats(const unsigned long long* bits, long long* stats, int D, int H,
                                 int W, hipStream_t stream) {
  L3U_REQUIRE(bits && stats && dims_ok(D, H, W));
  const int WW = words_per_row(W);
  const long long nrows = (long long)D * H, want = (nrows * WW + 255) / 256;
  const int grid = (int)(want < 1024 ? want : 1024);
  pp_stats_init<<<1, 64, 0, stream>>>(stats);
  pp_stats<<<grid, 256, 0, stream>>>(bits, stats, nrows, H, WW);
  L3U_CHECK_LAUNCH();
}
