// Resegmentation of lesions by an uptake threshold (light_unet/resegment.py): seeded region growing
// (geodesic reconstruction) restricted to a box, one threshold per seed.
//
//   bitmaps    a seed's box is two bitmaps, candidates (uptake >= thr, inside the body mask) and
//              reached, in l3u_pp_pack's layout relative to the box: 64-bit words, x fastest, bit b of
//              word w is x0 + 64 w + b, rows padded to whole words (padding bits 0).  A wave forms a
//              word from one coalesced 64-voxel row load with __ballot.
//   growing    reached |= cand & neighbours(reached), repeated until a sweep changes no word.  A sweep
//              also fills every run of candidates along x inside a word in one step (the carry of
//              cand + reached runs to the end of the run), so the number of sweeps follows the number
//              of words a path crosses, not its voxels.  The update is in place and monotone: every
//              bit it sets belongs to the region and no bit is cleared, so the fixed point does not
//              depend on the order in which threads read and write, and a sweep in which no thread
//              wrote has read the final state everywhere.
//   LDS path   one workgroup per seed whose two bitmaps fit the LDS budget: build, grow and commit
//              in one launch.
//   tiled path the bitmaps of a larger box live in a global arena (candidates and two reached
//              buffers); one launch grows every 8 x 8 x 4-word tile, staged with a halo of one row,
//              plane and word, to its own fixed point, reading one reached buffer and writing the
//              other, and counts the interior words it changed; the host relaunches until a launch
//              changes none.
//   ownership  own[v] = max over the seeds that reach v of (n + 1 - label), an integer atomicMax on a
//              zeroed map: exact and order-independent; the caller maps key k back to n + 1 - k
//              (l3u_ccl_stats_b's remap), which is the smallest label.
// All integer and bit work but the one comparison (double)uptake >= thr: the same input gives the
// same bits.
#include "common.h"

namespace l3u {
namespace {

typedef unsigned long long u64;

constexpr int kItemInts = 8;                 // label, z0, z1, y0, y1, x0, x1 (ends exclusive), path
constexpr int kTileInts = 4;                 // item, z, y and word origin of the tile inside the box
constexpr int kTZ = 8, kTY = 8, kTW = 4;     // a tile's interior: 256 words, one per thread
constexpr int kSZ = kTZ + 2, kSY = kTY + 2, kSW = kTW + 2;
constexpr int kStage = kSZ * kSY * kSW;      // 600 staged words per bitmap
constexpr int kLdsMax = 64 * 1024;           // the dynamic LDS a launch asks for at most
constexpr int kLdsHead = 16;                 // the sweep flag, ahead of the two bitmaps

struct Box {
  int L, z0, y0, x0, nz, ny, nx, wpr, path;
  long long nw;
  bool ok;
};

L3U_DEV Box load_box(const int* __restrict__ it, int D, int H, int W) {
  Box b;
  b.L = it[0];
  b.z0 = it[1];
  b.y0 = it[3];
  b.x0 = it[5];
  b.nz = it[2] - it[1];
  b.ny = it[4] - it[3];
  b.nx = it[6] - it[5];
  b.path = it[7];
  b.wpr = (b.nx + 63) >> 6;
  b.ok = b.L > 0 && b.z0 >= 0 && b.y0 >= 0 && b.x0 >= 0 && b.nz > 0 && b.ny > 0 && b.nx > 0 &&
         it[2] <= D && it[4] <= H && it[6] <= W;
  b.nw = b.ok ? (long long)b.nz * b.ny * b.wpr : 0;
  return b;
}

// Word w of box row (z, y): the candidates and the seed's candidates.  Called by a whole wave.
L3U_DEV void build_word(const float* __restrict__ up, const int* __restrict__ lab,
                        const void* __restrict__ body, int body_u8, double thr, const Box& b, int z,
                        int y, int w, int H, int W, u64& cw, u64& sw) {
  const int bx = w * 64 + ((int)threadIdx.x & 63);
  const bool in = bx < b.nx;
  const long long idx = ((long long)(b.z0 + z) * H + (b.y0 + y)) * W + b.x0 + (in ? bx : 0);
  bool cand = in && (double)up[idx] >= thr;
  if (body) {
    const bool on = body_u8 ? static_cast<const unsigned char*>(body)[idx] != 0
                            : static_cast<const float*>(body)[idx] != 0.f;
    cand = cand && on;
  }
  cw = __ballot(cand);
  sw = __ballot(cand && lab[idx] == b.L);
}

// r (a subset of c) grown along x to the ends of its runs of c inside the word
L3U_DEV u64 fill_x(u64 r, u64 c) {
  const u64 up = ((c + r) ^ c) & c;   // the carry clears a run from its lowest reached bit upwards
  const u64 rc = __brevll(c), rr = __brevll(r);
  const u64 dn = __brevll(((rc + rr) ^ rc) & rc);
  return r | up | dn;
}

// One sweep over the staged words [SZ][SY][SW]; words outside the stage count as 0.
L3U_DEV bool sweep_once(volatile u64* r, const u64* c, int SZ, int SY, int SW) {
  const int n = SZ * SY * SW, plane = SY * SW;
  bool ch = false;
  for (int k = (int)threadIdx.x; k < n; k += 256) {
    const u64 cw = c[k];
    const u64 old = r[k];
    if (old == cw) continue;   // nothing left to reach here (an empty word included)
    const int row = k / SW, w = k - row * SW, z = row / SY, y = row - z * SY;
    u64 nb = (old << 1) | (old >> 1);
    if (w > 0) nb |= r[k - 1] >> 63;
    if (w < SW - 1) nb |= r[k + 1] << 63;
    if (y > 0) nb |= r[k - SW];
    if (y < SY - 1) nb |= r[k + SW];
    if (z > 0) nb |= r[k - plane];
    if (z < SZ - 1) nb |= r[k + plane];
    const u64 in = old | (nb & cw);
    if (in == 0) continue;
    const u64 v = fill_x(in, cw);
    if (v != old) {
      r[k] = v;
      ch = true;
    }
  }
  return ch;
}

// Sweeps until one changes nothing; `flag` is an int in LDS.  Returns the sweeps that changed a word.
L3U_DEV int grow_fixed_point(volatile u64* r, const u64* c, int SZ, int SY, int SW,
                             volatile int* flag) {
  int ns = 0;
  for (;;) {
    if (threadIdx.x == 0) *flag = 0;
    __syncthreads();
    if (sweep_once(r, c, SZ, SY, SW)) *flag = 1;
    __syncthreads();
    const int ch = *flag;
    __syncthreads();
    if (!ch) break;
    ++ns;
  }
  return ns;
}

// the voxels of box word k of bitmap word m into the ownership map
L3U_DEV void commit_word(u64 m, const Box& b, int z, int y, int w, int key, int* __restrict__ own,
                         int H, int W) {
  const long long base = ((long long)(b.z0 + z) * H + (b.y0 + y)) * W + b.x0 + w * 64;
  while (m) {
    const int bit = __ffsll((long long)m) - 1;
    m &= m - 1;
    if (w * 64 + bit < b.nx) atomicMax(own + base + bit, key);
  }
}

// ---- LDS path: one workgroup per seed --------------------------------------------------------------
__global__ __launch_bounds__(256) void rs_grow_lds(const float* __restrict__ up,
                                                   const int* __restrict__ lab,
                                                   const void* __restrict__ body, int body_u8,
                                                   const int* __restrict__ items,
                                                   const double* __restrict__ thr, int n, int grow,
                                                   int* __restrict__ own, u64* __restrict__ reached,
                                                   int* __restrict__ sweeps, int lds_bytes, int D,
                                                   int H, int W) {
  extern __shared__ u64 rs_sm[];
  const int item = (int)blockIdx.x;
  const Box b = load_box(items + (long long)item * kItemInts, D, H, W);
  if (!b.ok || b.path != 0 || b.L > n || b.nw * 16 + kLdsHead > lds_bytes) return;   // uniform
  const int nw = (int)b.nw;
  volatile int* flag = reinterpret_cast<volatile int*>(rs_sm);
  u64* c = rs_sm + kLdsHead / 8;
  u64* r = c + nw;
  const int t = (int)threadIdx.x, wv = t >> 6, lane = t & 63;
  const double th = thr[item];
  for (int k = wv; k < nw; k += 4) {
    const int row = k / b.wpr, w = k - row * b.wpr, z = row / b.ny, y = row - z * b.ny;
    u64 cw, sw;
    build_word(up, lab, body, body_u8, th, b, z, y, w, H, W, cw, sw);
    if (lane == 0) {
      c[k] = cw;
      r[k] = sw;
    }
  }
  __syncthreads();
  const int ns = grow ? grow_fixed_point(r, c, b.nz, b.ny, b.wpr, flag) : 0;
  const int key = n + 1 - b.L;
  unsigned cnt = 0;
  for (int k = t; k < nw; k += 256) {
    const u64 m = r[k];
    if (!m) continue;
    cnt += (unsigned)__popcll(m);
    const int row = k / b.wpr, w = k - row * b.wpr, z = row / b.ny, y = row - z * b.ny;
    commit_word(m, b, z, y, w, key, own, H, W);
  }
  if (cnt) atomicAdd(reached + item, (u64)cnt);
  if (t == 0) sweeps[item] = ns;
}

// ---- tiled path ------------------------------------------------------------------------------------
struct Tile {
  int item, z0, y0, w0;
  bool ok;
};
L3U_DEV Tile load_tile(const int* __restrict__ tl, const int* __restrict__ items, int n, int D, int H,
                       int W, Box& b) {
  Tile q;
  q.item = tl[0];
  q.z0 = tl[1];
  q.y0 = tl[2];
  q.w0 = tl[3];
  q.ok = q.item >= 0 && q.item < n;
  if (q.ok) {
    b = load_box(items + (long long)q.item * kItemInts, D, H, W);
    q.ok = b.ok && b.path == 1 && b.L <= n && q.z0 >= 0 && q.z0 < b.nz && q.y0 >= 0 && q.y0 < b.ny &&
           q.w0 >= 0 && q.w0 < b.wpr;
  }
  return q;
}

// candidates and seed words of every tile into the arena (the seed words into the first buffer)
__global__ __launch_bounds__(256) void rs_tile_build(const float* __restrict__ up,
                                                     const int* __restrict__ lab,
                                                     const void* __restrict__ body, int body_u8,
                                                     const int* __restrict__ items,
                                                     const double* __restrict__ thr, int n,
                                                     const int* __restrict__ tiles,
                                                     const long long* __restrict__ aoff,
                                                     u64* __restrict__ arena, int D, int H, int W) {
  Box b;
  const Tile q = load_tile(tiles + (long long)blockIdx.x * kTileInts, items, n, D, H, W, b);
  if (!q.ok) return;
  u64* c = arena + aoff[q.item];
  u64* r = c + b.nw;
  const int wv = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  const double th = thr[q.item];
  for (int j = wv; j < kTZ * kTY * kTW; j += 4) {
    const int dw = j % kTW, dy = (j / kTW) % kTY, dz = j / (kTW * kTY);
    const int z = q.z0 + dz, y = q.y0 + dy, w = q.w0 + dw;
    if (z >= b.nz || y >= b.ny || w >= b.wpr) continue;   // uniform over the wave
    u64 cw, sw;
    build_word(up, lab, body, body_u8, th, b, z, y, w, H, W, cw, sw);
    if (lane == 0) {
      const long long k = ((long long)z * b.ny + y) * b.wpr + w;
      c[k] = cw;
      r[k] = sw;
    }
  }
}

// every tile to its own fixed point: reached buffer 1 + flip -> buffer 2 - flip
__global__ __launch_bounds__(256) void rs_tile_sweep(const int* __restrict__ items, int n,
                                                     const int* __restrict__ tiles,
                                                     const long long* __restrict__ aoff,
                                                     u64* __restrict__ arena, int flip,
                                                     unsigned* __restrict__ counter, int D, int H,
                                                     int W) {
  __shared__ u64 sc[kStage];
  __shared__ u64 sr[kStage];
  __shared__ int flag;
  Box b;
  const Tile q = load_tile(tiles + (long long)blockIdx.x * kTileInts, items, n, D, H, W, b);
  if (!q.ok) return;
  const u64* c = arena + aoff[q.item];
  const u64* rin = c + b.nw * (1 + flip);
  u64* rout = arena + aoff[q.item] + b.nw * (2 - flip);
  const int t = (int)threadIdx.x;
  for (int i = t; i < kStage; i += 256) {
    const int sw = i % kSW, sy = (i / kSW) % kSY, sz = i / (kSW * kSY);
    const int z = q.z0 - 1 + sz, y = q.y0 - 1 + sy, w = q.w0 - 1 + sw;
    const bool in = z >= 0 && z < b.nz && y >= 0 && y < b.ny && w >= 0 && w < b.wpr;
    const long long k = in ? ((long long)z * b.ny + y) * b.wpr + w : 0;
    sc[i] = in ? c[k] : 0ull;
    sr[i] = in ? rin[k] : 0ull;
  }
  __syncthreads();
  // thread t owns interior word (dz, dy, dw)
  const int dw = t % kTW, dy = (t / kTW) % kTY, dz = t / (kTW * kTY);
  const int z = q.z0 + dz, y = q.y0 + dy, w = q.w0 + dw;
  const int si = ((dz + 1) * kSY + (dy + 1)) * kSW + (dw + 1);
  const bool mine = z < b.nz && y < b.ny && w < b.wpr;
  const u64 before = sr[si];
  __syncthreads();
  grow_fixed_point(sr, sc, kSZ, kSY, kSW, &flag);
  const u64 after = sr[si];
  if (mine) rout[((long long)z * b.ny + y) * b.wpr + w] = after;
  const u64 moved = __ballot(mine && after != before);
  if ((t & 63) == 0 && moved) atomicAdd(counter, (unsigned)__popcll(moved));
}

// the reached buffer 1 + flip of every tile into the ownership map and the seeds' counts
__global__ __launch_bounds__(256) void rs_tile_commit(const int* __restrict__ items, int n,
                                                      const int* __restrict__ tiles,
                                                      const long long* __restrict__ aoff,
                                                      const u64* __restrict__ arena, int flip,
                                                      int* __restrict__ own, u64* __restrict__ reached,
                                                      int D, int H, int W) {
  Box b;
  const Tile q = load_tile(tiles + (long long)blockIdx.x * kTileInts, items, n, D, H, W, b);
  if (!q.ok) return;
  const u64* r = arena + aoff[q.item] + b.nw * (1 + flip);
  const int t = (int)threadIdx.x;
  const int dw = t % kTW, dy = (t / kTW) % kTY, dz = t / (kTW * kTY);
  const int z = q.z0 + dz, y = q.y0 + dy, w = q.w0 + dw;
  if (z >= b.nz || y >= b.ny || w >= b.wpr) return;
  const u64 m = r[((long long)z * b.ny + y) * b.wpr + w];
  if (!m) return;
  commit_word(m, b, z, y, w, n + 1 - b.L, own, H, W);
  atomicAdd(reached + q.item, (u64)__popcll(m));
}

L3U_INLINE_HOST bool dims_ok(int D, int H, int W) {
  return D > 0 && H > 0 && W > 0 && (long long)D * H * W < (1ll << 31);
}
L3U_INLINE_HOST int lds_budget(int max_lds_bytes) {
  if (max_lds_bytes == 0) return kLdsMax;
  return (max_lds_bytes < kLdsHead || max_lds_bytes > kLdsMax) ? -1 : max_lds_bytes;
}

}  // namespace
}  // namespace l3u

using namespace l3u;

extern "C" int l3u_rs_path(int nz, int ny, int nx, int max_lds_bytes) {
  const int budget = lds_budget(max_lds_bytes);
  if (budget < 0 || nz <= 0 || ny <= 0 || nx <= 0) return -1;
  const long long nw = (long long)nz * ny * ((nx + 63) / 64);
  return nw * 16 + kLdsHead <= budget ? 0 : 1;
}

extern "C" int l3u_rs_tiles(int nz, int ny, int nx) {
  if (nz <= 0 || ny <= 0 || nx <= 0) return 0;
  const long long t = (long long)((nz + kTZ - 1) / kTZ) * ((ny + kTY - 1) / kTY) *
                      (((nx + 63) / 64 + kTW - 1) / kTW);
  return t < (1ll << 31) ? (int)t : 0;
}

extern "C" int l3u_rs_grow(const float* uptake, const int* seeds, const void* body, int body_dtype,
                           const int* items, const double* thr, int n, int grow, int* own,
                           unsigned long long* reached, int* sweeps, const int* tiles, int n_tiles,
                           const long long* aoff, unsigned long long* arena, int max_lds_bytes, int D,
                           int H, int W, hipStream_t stream) {
  L3U_REQUIRE(uptake && seeds && items && thr && own && reached && sweeps && dims_ok(D, H, W));
  L3U_REQUIRE(n >= 1 && n_tiles >= 0 && (body_dtype == 0 || body_dtype == 2));
  L3U_REQUIRE(n_tiles == 0 || (tiles && aoff && arena));
  const int budget = lds_budget(max_lds_bytes);
  L3U_REQUIRE(budget >= 0);
  rs_grow_lds<<<n, 256, budget, stream>>>(uptake, seeds, body, body_dtype == 2, items, thr, n,
                                          grow ? 1 : 0, own, reached, sweeps, budget, D, H, W);
  if (n_tiles > 0)
    rs_tile_build<<<n_tiles, 256, 0, stream>>>(uptake, seeds, body, body_dtype == 2, items, thr, n,
                                               tiles, aoff, arena, D, H, W);
  L3U_CHECK_LAUNCH();
}

extern "C" int l3u_rs_sweep(const int* items, int n, const int* tiles, int n_tiles,
                            const long long* aoff, unsigned long long* arena, int flip,
                            unsigned int* counter, int D, int H, int W, hipStream_t stream) {
  L3U_REQUIRE(items && tiles && aoff && arena && counter && n >= 1 && n_tiles >= 1);
  L3U_REQUIRE((flip == 0 || flip == 1) && dims_ok(D, H, W));
  rs_tile_sweep<<<n_tiles, 256, 0, stream>>>(items, n, tiles, aoff, arena, flip, counter, D, H, W);
  L3U_CHECK_LAUNCH();
}

extern "C" int l3u_rs_commit(const int* items, int n, const int* tiles, int n_tiles,
                             const long long* aoff, const unsigned long long* arena, int flip, int* own,
                             unsigned long long* reached, int D, int H, int W, hipStream_t stream) {
  L3U_REQUIRE(items && tiles && aoff && arena && own && reached && n >= 1 && n_tiles >= 1);
  L3U_REQUIRE((flip == 0 || flip == 1) && dims_ok(D, H, W));
  rs_tile_commit<<<n_tiles, 256, 0, stream>>>(items, n, tiles, aoff, arena, flip, own, reached, D, H,
                                              W);
  L3U_CHECK_LAUNCH();
}
