// Lesion post-processing on the device: connected-component labelling and per-component
// statistics.  Replaces the host scipy/numpy work of
//   light_unet/models/metrics.py:38-63   get_connected_components (ndimage.label with its default
//                                        structure: face connectivity in every dimension of the
//                                        array -- 6 neighbours for a [D, H, W] volume, 8 for a
//                                        batched [B, D, H, W] array, where the same voxel of
//                                        consecutive batch items is connected; min_size filter +
//                                        relabel)
//   light_unet/models/metrics.py:107-213 component centres of mass, pairwise overlap (IoU) counts
//   light_unet/core/inferencer.py:62-111 bounding boxes, volumes and peak probability per component
// (host-bound with real volumes).  Integer work, bit-exact:
//   * labelling: lock-free union-find over the face neighbours (atomicMin links every root to the
//     SMALLER linear index, so the final root of a component is its first voxel in raster order);
//     components are then numbered by the rank of that first voxel (a chunk-count + scan +
//     ballot-ranked scatter), which is exactly scipy.ndimage.label's numbering (order of first
//     encounter in a C-order scan);
//   * statistics: 64-bit integer atomics (sizes, coordinate sums, bounding boxes) and the peak
//     probability as the max of non-negative float bit patterns (order-preserving), so no result
//     depends on the order in which workgroups arrive.
#include "common.h"
using namespace l3u;

namespace {

L3U_DEV int uf_find(const int* __restrict__ parent, int x) {
  int p = parent[x];
  while (p != x) {
    x = p;
    p = parent[x];
  }
  return x;
}

// every foreground voxel starts as its own root; -1 = background
__global__ __launch_bounds__(256) void ccl_init_kernel(const float* __restrict__ src, float thr,
                                                       int* __restrict__ parent, long long n) {
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    parent[i] = src[i] >= thr ? (int)i : -1;
}

// union of a and b: link the larger root under the smaller one (atomicMin keeps parent[x] <= x,
// so every path strictly decreases and the walk terminates)
L3U_DEV void uf_union(int* parent, int a, int b) {
  while (true) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }   // a > b: a becomes a child of b
    const int old = atomicMin(&parent[a], b);
    if (old == a) return;                            // a was still a root: linked
    a = old;                                         // linked elsewhere meanwhile: retry
  }
}

// face neighbours of [B][D][H][W]: x, y, z within an item and b (the same voxel of the previous
// item, offset S = D*H*W) -- ndimage.label's default structure for a 4-dimensional array
__global__ __launch_bounds__(256) void ccl_merge_kernel(int* __restrict__ parent, int B, int D, int H,
                                                        int W) {
  const long long S = (long long)D * H * W, n = B * S, HW = (long long)H * W;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    if (parent[i] < 0) continue;
    const long long r = i % S;
    const int x = (int)(r % W), y = (int)((r / W) % H), z = (int)(r / HW);
    if (x > 0 && parent[i - 1] >= 0) uf_union(parent, (int)i, (int)(i - 1));
    if (y > 0 && parent[i - W] >= 0) uf_union(parent, (int)i, (int)(i - W));
    if (z > 0 && parent[i - HW] >= 0) uf_union(parent, (int)i, (int)(i - HW));
    if (i >= S && parent[i - S] >= 0) uf_union(parent, (int)i, (int)(i - S));
  }
}

// parent[i] = root(i); count[c] = roots in chunk c (kCh voxels per chunk)
constexpr int kCh = 4096;
__global__ __launch_bounds__(256) void ccl_flatten_kernel(int* __restrict__ parent, long long n,
                                                          int* __restrict__ count) {
  __shared__ int red[4];
  const long long b0 = (long long)blockIdx.x * kCh;
  int c = 0;
  for (int k = threadIdx.x; k < kCh; k += 256) {
    const long long i = b0 + k;
    if (i < n && parent[i] >= 0) {
      const int r = uf_find(parent, (int)i);
      parent[i] = r;
      c += r == (int)i;
    }
  }
  c = (int)wave_sum((float)c);   // <= 4096: exact in fp32
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) count[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// exclusive scan of the chunk counts (one workgroup, any length); the total lands in count[nb]
__global__ __launch_bounds__(256) void ccl_scan_kernel(int* __restrict__ count, int nb) {
  __shared__ int part[256];
  const int per = (nb + 255) / 256, lo = threadIdx.x * per, hi = min(nb, lo + per);
  int s = 0;
  for (int i = lo; i < hi; ++i) s += count[i];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    int a = 0;
    for (int t = 0; t < 256; ++t) { const int v = part[t]; part[t] = a; a += v; }
    count[nb] = a;
  }
  __syncthreads();
  int a = part[threadIdx.x];
  for (int i = lo; i < hi; ++i) { const int v = count[i]; count[i] = a; a += v; }
}

// roots get their label, 1 + their rank in raster order: ballot ranks inside each round of 256
// consecutive voxels, rounds in order
__global__ __launch_bounds__(256) void ccl_root_label_kernel(const int* __restrict__ parent,
                                                             long long n,
                                                             const int* __restrict__ offs,
                                                             int* __restrict__ label) {
  __shared__ int wsum[4];
  __shared__ int base;
  const long long b0 = (long long)blockIdx.x * kCh;
  const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
  if (threadIdx.x == 0) base = offs[blockIdx.x];
  __syncthreads();
  for (int k0 = 0; k0 < kCh; k0 += 256) {
    const long long i = b0 + k0 + threadIdx.x;
    const bool root = i < n && parent[i] == (int)i;
    const unsigned long long m = __ballot(root);
    const int before = __popcll(m & ((1ull << ln) - 1ull));
    if (ln == 0) wsum[wv] = __popcll(m);
    __syncthreads();
    int pre = base;
    for (int w = 0; w < wv; ++w) pre += wsum[w];
    if (root) label[i] = pre + before + 1;
    __syncthreads();
    if (threadIdx.x == 0) base += (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void ccl_label_kernel(const int* __restrict__ parent,
                                                        int* __restrict__ label, long long n) {
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int p = parent[i];
    if (p < 0) label[i] = 0;
    else if (p != (int)i) label[i] = label[p];
  }
}

// per component l (1-based): stats[(l-1)*12 + k], k = 0 size, 1..3 sum of the three leading
// coordinates (c0, c1, c2), 4..6 their minima, 7..9 their maxima, 10 max prob (float bits;
// prob >= 0).  The leading coordinates are (z, y, x) of a 3-dimensional array and (b, z, y) of a
// 4-dimensional one (lead4): the reference keeps the first three of ndimage.center_of_mass's
// coordinates whatever the rank (metrics.py:99-124).  remap (optional) renumbers the labels in
// place first (0 drops the voxel).
__global__ __launch_bounds__(256) void ccl_stats_kernel(int* __restrict__ label,
                                                        const int* __restrict__ remap,
                                                        const float* __restrict__ prob,
                                                        unsigned long long* __restrict__ stats,
                                                        int B, int D, int H, int W, int lead4) {
  const long long S = (long long)D * H * W, n = B * S, HW = (long long)H * W;
  const int lane = threadIdx.x & 63;
  // whole waves run the loop together: a wave whose labelled lanes all carry ONE label (the inside
  // of a large component; a body mask is one component of millions of voxels) reduces its lanes
  // first and issues one set of atomics, instead of 64 colliding ones per statistic.  Integer
  // sums / minima / maxima: the same results in any grouping.
  const long long nround = (n + 63) & ~63ll;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < nround; i += (long long)gridDim.x * 256) {
    int l = i < n ? label[i] : 0;
    if (l > 0 && remap) {
      l = remap[l];
      label[i] = l;
    }
    const bool on = l > 0;
    const unsigned long long bm = __ballot(on);
    if (bm == 0) continue;
    const long long ic = i < n ? i : 0;
    const long long r = ic % S;
    const unsigned long long x = r % W, y = (r / W) % H, z = r / HW, b = ic / S;
    const unsigned long long c0 = lead4 ? b : z, c1 = lead4 ? z : y, c2 = lead4 ? y : x;
    unsigned long long pm = 0;
    if (on && prob) pm = (unsigned long long)__float_as_uint(fmaxf(prob[i], 0.f));
    const int first = __builtin_ctzll(bm);
    const int l0 = __builtin_amdgcn_readlane(l, first);
    if (__ballot(on && l == l0) == bm && __builtin_popcountll(bm) > 1) {
      unsigned long long v[10] = {on ? c0 : 0ull, on ? c1 : 0ull, on ? c2 : 0ull,
                                  on ? c0 : ~0ull, on ? c1 : ~0ull, on ? c2 : ~0ull,
                                  on ? c0 : 0ull, on ? c1 : 0ull, on ? c2 : 0ull, pm};
#pragma unroll
      for (int m = 1; m < 64; m <<= 1) {
#pragma unroll
        for (int k = 0; k < 10; ++k) {
          const unsigned long long o = __shfl_xor(v[k], m);
          v[k] = k < 3 ? v[k] + o : (k < 6 ? (o < v[k] ? o : v[k]) : (o > v[k] ? o : v[k]));
        }
      }
      if (lane == first) {
        unsigned long long* s = stats + (long long)(l0 - 1) * 12;
        atomicAdd(s + 0, (unsigned long long)__builtin_popcountll(bm));
        atomicAdd(s + 1, v[0]);
        atomicAdd(s + 2, v[1]);
        atomicAdd(s + 3, v[2]);
        atomicMin(s + 4, v[3]);
        atomicMin(s + 5, v[4]);
        atomicMin(s + 6, v[5]);
        atomicMax(s + 7, v[6]);
        atomicMax(s + 8, v[7]);
        atomicMax(s + 9, v[8]);
        if (prob) atomicMax(s + 10, v[9]);
      }
    } else if (on) {
      unsigned long long* s = stats + (long long)(l - 1) * 12;
      atomicAdd(s + 0, 1ull);
      atomicAdd(s + 1, c0);
      atomicAdd(s + 2, c1);
      atomicAdd(s + 3, c2);
      atomicMin(s + 4, c0);
      atomicMin(s + 5, c1);
      atomicMin(s + 6, c2);
      atomicMax(s + 7, c0);
      atomicMax(s + 8, c1);
      atomicMax(s + 9, c2);
      if (prob) atomicMax(s + 10, pm);
    }
  }
}

__global__ __launch_bounds__(256) void ccl_stats_init_kernel(unsigned long long* __restrict__ stats,
                                                             int ncomp) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < ncomp * 12; i += gridDim.x * 256) {
    const int k = i % 12;
    stats[i] = (k >= 4 && k <= 6) ? ~0ull : 0ull;
  }
}

// overlap counts of two labellings: inter[a * (nb + 1) + b] += 1 where both labels are > 0
__global__ __launch_bounds__(256) void ccl_pairs_kernel(const int* __restrict__ la,
                                                        const int* __restrict__ lb, int nb,
                                                        unsigned int* __restrict__ inter,
                                                        long long n) {
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int a = la[i], b = lb[i];
    if (a > 0 && b > 0) atomicAdd(inter + (long long)a * (nb + 1) + b, 1u);
  }
}

// ---- the threshold sweep: K binarisations of one probability map in one go ------------------
// level[v] = #{k : p[v] >= thr[k]} (thr strictly ascending, so the foreground at threshold k is
// level >= k + 1), and the K level volumes are labelled side by side: level k of a [D, H, W]
// volume lives at parent / label + k * n with indices LOCAL to the level (no neighbour across
// levels, unlike the batch axis of ccl_merge_kernel), so every level gets ndimage.label's own
// numbering and the limit stays n < 2^31.
constexpr int kMaxLv = 32;

// p = prob (* mask, one fp32 multiply as numpy's float32 product); a NaN compares false at every
// threshold (level 0).  hist[(lv) * 2 + (target >= 0.5)] counts voxels: LDS counters per
// workgroup, then one 64-bit atomic per non-empty bin per workgroup.
__global__ __launch_bounds__(256) void thr_levels_kernel(const float* __restrict__ prob,
                                                         const float* __restrict__ mask,
                                                         const float* __restrict__ target,
                                                         const float* __restrict__ thr, int K,
                                                         unsigned char* __restrict__ level,
                                                         unsigned long long* __restrict__ hist,
                                                         float* __restrict__ masked, long long n) {
  __shared__ float sthr[kMaxLv];
  __shared__ unsigned int sh[(kMaxLv + 1) * 2];
  const int nbin = (K + 1) * 2;
  if ((int)threadIdx.x < K) sthr[threadIdx.x] = thr[threadIdx.x];
  if ((int)threadIdx.x < nbin) sh[threadIdx.x] = 0u;
  __syncthreads();
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    float p = prob[i];
    if (mask) p = p * mask[i];
    if (masked) masked[i] = p;
    int lv = 0;
    for (int k = 0; k < K; ++k) lv += p >= sthr[k];
    level[i] = (unsigned char)lv;
    const int t = target ? (target[i] >= 0.5f) : 0;
    atomicAdd(&sh[lv * 2 + t], 1u);
  }
  __syncthreads();
  if ((int)threadIdx.x < nbin && sh[threadIdx.x])
    atomicAdd(hist + threadIdx.x, (unsigned long long)sh[threadIdx.x]);
}

__global__ __launch_bounds__(256) void ccl_init_lv_kernel(const unsigned char* __restrict__ level,
                                                          int k0, int K, int* __restrict__ parent,
                                                          long long n) {
  const long long tot = K * n;
  for (long long j = blockIdx.x * 256ll + threadIdx.x; j < tot; j += (long long)gridDim.x * 256) {
    const long long k = j / n, i = j - k * n;
    parent[j] = (int)level[i] >= k0 + (int)k + 1 ? (int)i : -1;
  }
}

__global__ __launch_bounds__(256) void ccl_merge_lv_kernel(int* __restrict__ parent, int K, int D,
                                                           int H, int W) {
  const long long n = (long long)D * H * W, tot = K * n, HW = (long long)H * W;
  for (long long j = blockIdx.x * 256ll + threadIdx.x; j < tot; j += (long long)gridDim.x * 256) {
    const long long k = j / n, i = j - k * n;
    int* p = parent + k * n;
    if (p[i] < 0) continue;
    const int x = (int)(i % W), y = (int)((i / W) % H), z = (int)(i / HW);
    if (x > 0 && p[i - 1] >= 0) uf_union(p, (int)i, (int)(i - 1));
    if (y > 0 && p[i - W] >= 0) uf_union(p, (int)i, (int)(i - W));
    if (z > 0 && p[i - HW] >= 0) uf_union(p, (int)i, (int)(i - HW));
  }
}

// the per-level forms of ccl_flatten / ccl_scan / ccl_root_label / ccl_label: blockIdx.y (or
// blockIdx.x of the scan) is the level; count holds nb + 1 ints per level
__global__ __launch_bounds__(256) void ccl_flatten_lv_kernel(int* __restrict__ parent, long long n,
                                                             int* __restrict__ count, int nb) {
  __shared__ int red[4];
  parent += (long long)blockIdx.y * n;
  count += (long long)blockIdx.y * (nb + 1);
  const long long b0 = (long long)blockIdx.x * kCh;
  int c = 0;
  for (int k = threadIdx.x; k < kCh; k += 256) {
    const long long i = b0 + k;
    if (i < n && parent[i] >= 0) {
      const int r = uf_find(parent, (int)i);
      parent[i] = r;
      c += r == (int)i;
    }
  }
  c = (int)wave_sum((float)c);   // <= 4096: exact in fp32
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) count[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void ccl_scan_lv_kernel(int* __restrict__ count, int nb) {
  __shared__ int part[256];
  count += (long long)blockIdx.x * (nb + 1);
  const int per = (nb + 255) / 256, lo = threadIdx.x * per, hi = min(nb, lo + per);
  int s = 0;
  for (int i = lo; i < hi; ++i) s += count[i];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    int a = 0;
    for (int t = 0; t < 256; ++t) { const int v = part[t]; part[t] = a; a += v; }
    count[nb] = a;
  }
  __syncthreads();
  int a = part[threadIdx.x];
  for (int i = lo; i < hi; ++i) { const int v = count[i]; count[i] = a; a += v; }
}

// offs[k] = components of the levels before k (offs[K] = all): where level k's segment of the
// statistics / overlap tables starts
__global__ void ccl_offs_lv_kernel(const int* __restrict__ count, int nb, int K,
                                   int* __restrict__ offs) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    int a = 0;
    for (int k = 0; k < K; ++k) { offs[k] = a; a += count[(long long)k * (nb + 1) + nb]; }
    offs[K] = a;
  }
}

__global__ __launch_bounds__(256) void ccl_root_label_lv_kernel(const int* __restrict__ parent,
                                                                long long n,
                                                                const int* __restrict__ offs, int nb,
                                                                int* __restrict__ label) {
  __shared__ int wsum[4];
  __shared__ int base;
  parent += (long long)blockIdx.y * n;
  label += (long long)blockIdx.y * n;
  offs += (long long)blockIdx.y * (nb + 1);
  const long long b0 = (long long)blockIdx.x * kCh;
  const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
  if (threadIdx.x == 0) base = offs[blockIdx.x];
  __syncthreads();
  for (int k0 = 0; k0 < kCh; k0 += 256) {
    const long long i = b0 + k0 + threadIdx.x;
    const bool root = i < n && parent[i] == (int)i;
    const unsigned long long m = __ballot(root);
    const int before = __popcll(m & ((1ull << ln) - 1ull));
    if (ln == 0) wsum[wv] = __popcll(m);
    __syncthreads();
    int pre = base;
    for (int w = 0; w < wv; ++w) pre += wsum[w];
    if (root) label[i] = pre + before + 1;
    __syncthreads();
    if (threadIdx.x == 0) base += (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void ccl_label_lv_kernel(const int* __restrict__ parent,
                                                           int* __restrict__ label, int K,
                                                           long long n) {
  const long long tot = K * n;
  for (long long j = blockIdx.x * 256ll + threadIdx.x; j < tot; j += (long long)gridDim.x * 256) {
    const long long k = j / n, i = j - k * n;
    const int p = parent[j];
    if (p < 0) label[j] = 0;
    else if (p != (int)i) label[j] = label[k * n + p];
  }
}

// ccl_stats_kernel for K level labellings of one [D, H, W] volume: component l of level k is row
// offs[k] + l - 1
__global__ __launch_bounds__(256) void ccl_stats_lv_kernel(const int* __restrict__ label,
                                                           const float* __restrict__ prob,
                                                           const int* __restrict__ offs,
                                                           unsigned long long* __restrict__ stats,
                                                           int K, int D, int H, int W) {
  const long long n = (long long)D * H * W, tot = K * n, HW = (long long)H * W;
  for (long long j = blockIdx.x * 256ll + threadIdx.x; j < tot; j += (long long)gridDim.x * 256) {
    const int l = label[j];
    if (l <= 0) continue;
    const long long k = j / n, i = j - k * n;
    const unsigned long long x = i % W, y = (i / W) % H, z = i / HW;
    unsigned long long* s = stats + ((long long)offs[k] + (l - 1)) * 12;
    atomicAdd(s + 0, 1ull);
    atomicAdd(s + 1, z);
    atomicAdd(s + 2, y);
    atomicAdd(s + 3, x);
    atomicMin(s + 4, z);
    atomicMin(s + 5, y);
    atomicMin(s + 6, x);
    atomicMax(s + 7, z);
    atomicMax(s + 8, y);
    atomicMax(s + 9, x);
    if (prob) atomicMax(s + 10, (unsigned long long)__float_as_uint(fmaxf(prob[i], 0.f)));
  }
}

// ccl_pairs_kernel for K level labellings against one target labelling: level k's
// (num_k + 1) x (nb + 1) table starts at (offs[k] + k) * (nb + 1)
__global__ __launch_bounds__(256) void ccl_pairs_lv_kernel(const int* __restrict__ la,
                                                           const int* __restrict__ lb, int nb,
                                                           const int* __restrict__ offs,
                                                           unsigned int* __restrict__ inter, int K,
                                                           long long n) {
  const long long tot = K * n;
  for (long long j = blockIdx.x * 256ll + threadIdx.x; j < tot; j += (long long)gridDim.x * 256) {
    const int a = la[j];
    if (a <= 0) continue;
    const long long k = j / n, i = j - k * n;
    const int b = lb[i];
    if (b > 0) atomicAdd(inter + ((long long)offs[k] + k + a) * (nb + 1) + b, 1u);
  }
}

int blocks_for(long long n) {
  const long long b = (n + 255) / 256;
  return (int)(b > 4096 ? 4096 : (b < 1 ? 1 : b));
}

}  // namespace

extern "C" {

int l3u_ccl_nchunks(long long n) { return (int)((n + kCh - 1) / kCh); }

int l3u_ccl_label_b(const float* src, float threshold, int* parent, int* label, int* chunk_count,
                    int B, int D, int H, int W, hipStream_t stream) {
  L3U_REQUIRE(src && parent && label && chunk_count && B > 0 && D > 0 && H > 0 && W > 0);
  const long long n = (long long)B * D * H * W;
  L3U_REQUIRE(n < (1ll << 31));
  const int nb = l3u_ccl_nchunks(n);
  hipLaunchKernelGGL(ccl_init_kernel, dim3(blocks_for(n)), dim3(256), 0, stream, src, threshold,
                     parent, n);
  hipLaunchKernelGGL(ccl_merge_kernel, dim3(blocks_for(n)), dim3(256), 0, stream, parent, B, D, H, W);
  hipLaunchKernelGGL(ccl_flatten_kernel, dim3(nb), dim3(256), 0, stream, parent, n, chunk_count);
  hipLaunchKernelGGL(ccl_scan_kernel, dim3(1), dim3(256), 0, stream, chunk_count, nb);
  hipLaunchKernelGGL(ccl_root_label_kernel, dim3(nb), dim3(256), 0, stream, parent, n, chunk_count,
                     label);
  hipLaunchKernelGGL(ccl_label_kernel, dim3(blocks_for(n)), dim3(256), 0, stream, parent, label, n);
  L3U_CHECK_LAUNCH();
}

int l3u_ccl_label(const float* src, float threshold, int* parent, int* label, int* chunk_count,
                  int D, int H, int W, hipStream_t stream) {
  return l3u_ccl_label_b(src, threshold, parent, label, chunk_count, 1, D, H, W, stream);
}

int l3u_ccl_stats_b(int* label, const int* remap, const float* prob, unsigned long long* stats,
                    int ncomp, int B, int D, int H, int W, int lead4, hipStream_t stream) {
  L3U_REQUIRE(label && stats && ncomp > 0 && B > 0 && D > 0 && H > 0 && W > 0);
  L3U_REQUIRE(lead4 == 0 ? B == 1 : lead4 == 1);
  const long long n = (long long)B * D * H * W;
  hipLaunchKernelGGL(ccl_stats_init_kernel, dim3(blocks_for(ncomp * 12ll)), dim3(256), 0, stream,
                     stats, ncomp);
  hipLaunchKernelGGL(ccl_stats_kernel, dim3(blocks_for(n)), dim3(256), 0, stream, label, remap,
                     prob, stats, B, D, H, W, lead4);
  L3U_CHECK_LAUNCH();
}

int l3u_ccl_stats(int* label, const int* remap, const float* prob, unsigned long long* stats,
                  int ncomp, int D, int H, int W, hipStream_t stream) {
  return l3u_ccl_stats_b(label, remap, prob, stats, ncomp, 1, D, H, W, 0, stream);
}

int l3u_ccl_pairs(const int* label_a, const int* label_b, int nb, unsigned int* inter, long long n,
                  hipStream_t stream) {
  L3U_REQUIRE(label_a && label_b && inter && nb >= 0 && n > 0);
  hipLaunchKernelGGL(ccl_pairs_kernel, dim3(blocks_for(n)), dim3(256), 0, stream, label_a, label_b,
                     nb, inter, n);
  L3U_CHECK_LAUNCH();
}

int l3u_ccl_lv_max_levels(long long n, long long max_bytes) {
  if (n <= 0) return 0;
  const long long per = n * 8 + ((long long)l3u_ccl_nchunks(n) + 1) * 4;   // parent + label + counts
  const long long g = max_bytes / per;
  return (int)(g < 1 ? 1 : (g > kMaxLv ? kMaxLv : g));
}

int l3u_thr_levels(const float* prob, const float* mask, const float* target, const float* thr,
                   int K, unsigned char* level, unsigned long long* hist, float* masked,
                   long long n, hipStream_t stream) {
  L3U_REQUIRE(prob && thr && level && hist && K >= 1 && K <= kMaxLv && n > 0);
  hipError_t e = hipMemsetAsync(hist, 0, sizeof(unsigned long long) * (K + 1) * 2, stream);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(thr_levels_kernel, dim3(blocks_for(n)), dim3(256), 0, stream, prob, mask,
                     target, thr, K, level, hist, masked, n);
  L3U_CHECK_LAUNCH();
}

int l3u_ccl_label_lv(const unsigned char* level, int k0, int K, int* parent, int* label,
                     int* chunk_count, int* offs, int D, int H, int W, hipStream_t stream) {
  L3U_REQUIRE(level && parent && label && chunk_count && offs && D > 0 && H > 0 && W > 0);
  L3U_REQUIRE(K >= 1 && k0 >= 0 && k0 + K <= kMaxLv);
  const long long n = (long long)D * H * W;
  L3U_REQUIRE(n < (1ll << 31));
  const int nb = l3u_ccl_nchunks(n);
  const int bl = blocks_for(K * n);
  hipLaunchKernelGGL(ccl_init_lv_kernel, dim3(bl), dim3(256), 0, stream, level, k0, K, parent, n);
  hipLaunchKernelGGL(ccl_merge_lv_kernel, dim3(bl), dim3(256), 0, stream, parent, K, D, H, W);
  hipLaunchKernelGGL(ccl_flatten_lv_kernel, dim3(nb, K), dim3(256), 0, stream, parent, n,
                     chunk_count, nb);
  hipLaunchKernelGGL(ccl_scan_lv_kernel, dim3(K), dim3(256), 0, stream, chunk_count, nb);
  hipLaunchKernelGGL(ccl_offs_lv_kernel, dim3(1), dim3(64), 0, stream, chunk_count, nb, K, offs);
  hipLaunchKernelGGL(ccl_root_label_lv_kernel, dim3(nb, K), dim3(256), 0, stream, parent, n,
                     chunk_count, nb, label);
  hipLaunchKernelGGL(ccl_label_lv_kernel, dim3(bl), dim3(256), 0, stream, parent, label, K, n);
  L3U_CHECK_LAUNCH();
}

int l3u_ccl_stats_lv(const int* label, const float* prob, const int* offs,
                     unsigned long long* stats, int total, int K, int D, int H, int W,
                     hipStream_t stream) {
  L3U_REQUIRE(label && offs && stats && total > 0 && K >= 1 && K <= kMaxLv && D > 0 && H > 0 &&
              W > 0);
  const long long n = (long long)D * H * W;
  hipLaunchKernelGGL(ccl_stats_init_kernel, dim3(blocks_for(total * 12ll)), dim3(256), 0, stream,
                     stats, total);
  hipLaunchKernelGGL(ccl_stats_lv_kernel, dim3(blocks_for(K * n)), dim3(256), 0, stream, label,
                     prob, offs, stats, K, D, H, W);
  L3U_CHECK_LAUNCH();
}

int l3u_ccl_pairs_lv(const int* label_lv, const int* label_b, int nb, const int* offs,
                     unsigned int* inter, int K, long long n, hipStream_t stream) {
  L3U_REQUIRE(label_lv && label_b && offs && inter && nb >= 0 && K >= 1 && K <= kMaxLv && n > 0);
  hipLaunchKernelGGL(ccl_pairs_lv_kernel, dim3(blocks_for(K * n)), dim3(256), 0, stream, label_lv,
                     label_b, nb, offs, inter, K, n);
  L3U_CHECK_LAUNCH();
}

}  // extern "C"
