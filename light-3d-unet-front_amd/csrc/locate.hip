// Patch locations on the device: rank-select over label voxels (the reference's
// PatchDataset._sample_locations, light_unet/datasets/patch_dataset.py:74-100).
//
// The reference lists np.argwhere(label > 0) and np.argwhere((label == 0) & body) on the host and
// keeps a few thousand rows of each, picked by np.random.randint.  Row k of np.argwhere(m) is the
// k-th set voxel of m in C order, so the rows the reference keeps are rank queries over a
// predicate that never has to be stored:
//   l3u_loc_count   per 4096-voxel block the number of voxels of each class, then (second launch
//                   of the same call) the exclusive prefix sums and the class totals;
//   l3u_loc_select  one wave per rank: upper-bound search of the prefix for the block, the block's
//                   predicate re-evaluated as 64 ballots, the row written by the lane that owns
//                   the voxel.
// Integer counts only: no floating point, no atomics, nothing that depends on scheduling.
#include "common.h"

namespace {

constexpr int kBlock = L3U_LOC_BLOCK;      // voxels per counted block
constexpr int kThreads = 256;              // 4 waves; a thread covers kBlock / kThreads voxels
constexpr int kPer = kBlock / kThreads;    // 16
constexpr int kScanThreads = 1024;
constexpr int kSelBatch = 8;               // 64-voxel words requested before the first ballot

template <typename T, int V>
struct alignas(sizeof(T) * V) LVec { T v[V]; };
template <int V>
struct alignas(V) BVec { unsigned char v[V]; };

// One block's two class counts by one workgroup (every wave ends with its own share in c0 / c1).
// V > 1: the block is whole and label / body are aligned to a V-voxel request (16 B of label per
// lane); the per-block COUNT does not depend on which lane holds which voxel, so thread t simply
// takes voxels (j * 256 + t) * V ... + V - 1 of the block.  V == 1: any alignment and the ragged
// last block, with clamped in-range loads and a select after the load.  All of a thread's loads
// are requested before the first compare.
template <typename T, int V, bool BODY>
L3U_DEV void count_block(const T* __restrict__ label, const unsigned char* __restrict__ body,
                         unsigned int n, unsigned int base, unsigned int& c0, unsigned int& c1) {
  constexpr int NL = kPer / V;
  LVec<T, V> lv[NL];
  BVec<V> bv[NL];
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    unsigned int i = base + (unsigned int)(j * kThreads + (int)threadIdx.x) * V;
    if (V == 1) i = i < n ? i : n - 1;
    lv[j] = *reinterpret_cast<const LVec<T, V>*>(label + i);
    if (BODY) bv[j] = *reinterpret_cast<const BVec<V>*>(body + i);
  }
#pragma unroll
  for (int j = 0; j < NL; ++j) {
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const unsigned int i = base + (unsigned int)(j * kThreads + (int)threadIdx.x) * V + k;
      const bool in = V > 1 || i < n;
      const T v = lv[j].v[k];
      const bool les = in && v > (T)0;
      const bool bg = in && v == (T)0 && (!BODY || bv[j].v[k] != 0);
      c0 += (unsigned int)__popcll(__ballot(les));
      c1 += (unsigned int)__popcll(__ballot(bg));
    }
  }
}

// One workgroup per block, ONE launch per volume: blocks below nvec take the V-wide requests, the
// others (the ragged last block; every block of an unaligned volume, nvec = 0) the clamped
// one-voxel form -- a workgroup-uniform choice between two complete load phases.
template <typename T, int V, bool BODY>
__global__ __launch_bounds__(kThreads) void loc_count_kernel(const T* __restrict__ label,
                                                             const unsigned char* __restrict__ body,
                                                             unsigned int n, int nvec, int nblocks,
                                                             unsigned int* __restrict__ prefix) {
  const int blk = (int)blockIdx.x;
  const unsigned int base = (unsigned int)blk * kBlock;   // <= n - 1 < 2^31: base + 4095 fits 32 bits
  unsigned int c0 = 0, c1 = 0;   // wave-uniform
  if (blk < nvec)
    count_block<T, V, BODY>(label, body, n, base, c0, c1);
  else
    count_block<T, 1, BODY>(label, body, n, base, c0, c1);
  __shared__ unsigned int part[kThreads / 64][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) part[wave][0] = c0, part[wave][1] = c1;
  __syncthreads();
  if (threadIdx.x < 2) {
    unsigned int s = 0;
    for (int w = 0; w < kThreads / 64; ++w) s += part[w][threadIdx.x];
    prefix[(size_t)threadIdx.x * (nblocks + 1) + blk] = s;
  }
}

// In place: counts[cls][0 .. nblocks) -> their exclusive prefix sums, entry nblocks the total.
// One workgroup per class walks the counts in tiles of 1024 in index order, with a running carry.
__global__ __launch_bounds__(kScanThreads) void loc_scan_kernel(unsigned int* __restrict__ prefix,
                                                                int nblocks) {
  unsigned int* p = prefix + (size_t)blockIdx.x * (nblocks + 1);
  __shared__ unsigned int wsum[kScanThreads / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned int carry = 0;
  for (int t0 = 0; t0 < nblocks; t0 += kScanThreads) {
    const int i = t0 + (int)threadIdx.x;
    const unsigned int ld = p[i < nblocks ? i : nblocks - 1];
    const unsigned int v = i < nblocks ? ld : 0u;
    unsigned int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned int o = __shfl_up(inc, d);
      if (lane >= d) inc += o;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    unsigned int woff = 0, tile = 0;
#pragma unroll
    for (int w = 0; w < kScanThreads / 64; ++w) {
      const unsigned int s = wsum[w];
      woff += w < wave ? s : 0u;
      tile += s;
    }
    if (i < nblocks) p[i] = carry + woff + inc - v;
    carry += tile;
    __syncthreads();
  }
  if (threadIdx.x == 0) p[nblocks] = carry;
}

// One wave per rank.  prefix: the class's row [nblocks + 1].
template <typename T, int CLS, bool BODY>
__global__ __launch_bounds__(kThreads) void loc_select_kernel(const T* __restrict__ label,
                                                              const unsigned char* __restrict__ body,
                                                              unsigned int n, int HW, int W,
                                                              const unsigned int* __restrict__ prefix,
                                                              int nblocks,
                                                              const long long* __restrict__ ranks, int R,
                                                              int case_idx, int4* __restrict__ rows) {
  const int lane = threadIdx.x & 63;
  const int r = (int)blockIdx.x * (kThreads / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (r >= R) return;
  const long long rank = ranks[r];
  const unsigned int total = prefix[nblocks];
  int4 row = make_int4(case_idx, -1, -1, -1);
  bool own = false;
  if (rank >= 0 && rank < (long long)total) {
    const unsigned int rk = (unsigned int)rank;
    // the last block whose exclusive prefix is <= rk (upper bound: empty blocks repeat their
    // neighbour's prefix and are stepped over).  Invariant: prefix[lo] <= rk < prefix[hi].
    int lo = 0, hi = nblocks;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (prefix[mid] <= rk) lo = mid; else hi = mid;
    }
    unsigned int res = rk - prefix[lo];
    const unsigned int base = (unsigned int)lo * kBlock;
    bool done = false;
    for (int w0 = 0; w0 < kBlock / 64 && !done; w0 += kSelBatch) {
      T v[kSelBatch];
      unsigned char bb[kSelBatch];
#pragma unroll
      for (int k = 0; k < kSelBatch; ++k) {
        const unsigned int i = base + (unsigned int)((w0 + k) * 64 + lane);
        const unsigned int ic = i < n ? i : n - 1;
        v[k] = label[ic];
        if (BODY) bb[k] = body[ic];
      }
#pragma unroll
      for (int k = 0; k < kSelBatch; ++k) {
        const unsigned int i = base + (unsigned int)((w0 + k) * 64 + lane);
        const bool set = i < n && (CLS == 0 ? v[k] > (T)0 : (v[k] == (T)0 && (!BODY || bb[k] != 0)));
        const unsigned long long m = __ballot(set);
        const unsigned int c = (unsigned int)__popcll(m);
        if (!done) {
          if (res < c) {
            done = true;
            own = set && (unsigned int)__popcll(m & ((1ull << lane) - 1ull)) == res;
            if (own) {
              const int z = (int)(i / (unsigned int)HW), rem = (int)(i - (unsigned int)z * (unsigned int)HW);
              const int y = rem / W;
              row = make_int4(case_idx, z, y, rem - y * W);
            }
          } else {
            res -= c;
          }
        }
      }
    }
  }
  // the owner writes; without one (rank out of range, or a prefix that does not belong to this
  // label) lane 0 writes the (case, -1, -1, -1) row
  const bool any = __ballot(own) != 0ull;
  if (any ? own : lane == 0) rows[r] = row;
}

template <typename T>
void count_launch(const void* label_, const unsigned char* body, unsigned int n, int nblocks,
                  unsigned int* prefix, hipStream_t stream) {
  const T* label = static_cast<const T*>(label_);
  constexpr int V = 16 / (int)sizeof(T);
  const bool aligned = (uintptr_t)label % 16 == 0 && (uintptr_t)body % V == 0;
  const int nvec = aligned ? (int)(n / kBlock) : 0;   // whole blocks of an aligned volume
  if (body)
    hipLaunchKernelGGL((loc_count_kernel<T, V, true>), dim3(nblocks), dim3(kThreads), 0, stream,
                       label, body, n, nvec, nblocks, prefix);
  else
    hipLaunchKernelGGL((loc_count_kernel<T, V, false>), dim3(nblocks), dim3(kThreads), 0, stream,
                       label, body, n, nvec, nblocks, prefix);
}

template <typename T>
void select_launch(const void* label_, const unsigned char* body, unsigned int n, int HW, int W,
                   const unsigned int* prefix, int nblocks, int cls, const long long* ranks, int R,
                   int case_idx, int4* rows, hipStream_t stream) {
  const T* label = static_cast<const T*>(label_);
  const dim3 grid((R + kThreads / 64 - 1) / (kThreads / 64)), block(kThreads);
  if (cls == 0)
    hipLaunchKernelGGL((loc_select_kernel<T, 0, false>), grid, block, 0, stream, label, body, n, HW, W,
                       prefix, nblocks, ranks, R, case_idx, rows);
  else if (body)
    hipLaunchKernelGGL((loc_select_kernel<T, 1, true>), grid, block, 0, stream, label, body, n, HW, W,
                       prefix, nblocks, ranks, R, case_idx, rows);
  else
    hipLaunchKernelGGL((loc_select_kernel<T, 1, false>), grid, block, 0, stream, label, body, n, HW, W,
                       prefix, nblocks, ranks, R, case_idx, rows);
}

}  // namespace

extern "C" int l3u_loc_nblocks(long long n) {
  return n > 0 && n < (1ll << 31) ? (int)((n + kBlock - 1) / kBlock) : 0;
}

extern "C" int l3u_loc_count(const void* label, int label_dtype, const unsigned char* body,
                             long long n, unsigned int* prefix, hipStream_t stream) {
  L3U_REQUIRE(n > 0 && n < (1ll << 31));
  L3U_REQUIRE(label && prefix && (label_dtype == 0 || label_dtype == 1));
  const int nblocks = l3u_loc_nblocks(n);
  if (label_dtype == 0)
    count_launch<float>(label, body, (unsigned int)n, nblocks, prefix, stream);
  else
    count_launch<double>(label, body, (unsigned int)n, nblocks, prefix, stream);
  hipLaunchKernelGGL(loc_scan_kernel, dim3(2), dim3(kScanThreads), 0, stream, prefix, nblocks);
  L3U_CHECK_LAUNCH();
}

extern "C" int l3u_loc_select(const void* label, int label_dtype, const unsigned char* body, int D,
                              int H, int W, const unsigned int* prefix, int cls,
                              const long long* ranks, int R, int case_idx, int* rows,
                              hipStream_t stream) {
  L3U_REQUIRE(D > 0 && H > 0 && W > 0 && R >= 0 && (cls == 0 || cls == 1));
  const long long n = (long long)D * H * W;
  L3U_REQUIRE(n < (1ll << 31));
  if (R == 0) return (int)hipSuccess;
  L3U_REQUIRE(label && prefix && ranks && rows && (label_dtype == 0 || label_dtype == 1));
  L3U_REQUIRE((uintptr_t)rows % 16 == 0);   // a row is one 16-byte store
  const int nblocks = l3u_loc_nblocks(n);
  const unsigned int* p = prefix + (size_t)cls * (nblocks + 1);
  if (label_dtype == 0)
    select_launch<float>(label, body, (unsigned int)n, H * W, W, p, nblocks, cls, ranks, R, case_idx,
                         reinterpret_cast<int4*>(rows), stream);
  else
    select_launch<double>(label, body, (unsigned int)n, H * W, W, p, nblocks, cls, ranks, R,
                          case_idx, reinterpret_cast<int4*>(rows), stream);
  L3U_CHECK_LAUNCH();
}
