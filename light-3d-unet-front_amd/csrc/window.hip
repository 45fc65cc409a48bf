// Whole-volume sliding-window inference, the device halves of sliding_window_inference_3d
// (light_unet/utils.py:11-139):
//   window_gather  batch of B windows [B][1][pd][ph][pw] cut out of the volume, zero padding
//                  past the volume edge (utils.py:96-113, np.pad constant 0)
//   window_blend   prob = sum_w pred_w * imp / sum_w imp over the windows covering each voxel,
//                  accumulated in the reference's window order (z, y, x loops, utils.py:88-132)
//                  with separate fp32 multiply and add (no FMA contraction), then prob/count
//                  where count > 0 (utils.py:135) -- the same float32 operation sequence as the
//                  reference's numpy accumulation, done by one thread per voxel (deterministic:
//                  no atomics, no order dependence on the batching)
//   window_occupancy / window_blend_masked  the same map times a body mask (trainer.py:401-402,
//                  inferencer.py:161-162) without the forwards of windows the mask empties: which
//                  windows hold a nonzero mask voxel, and the blend over a compact prediction
//                  buffer that stores +0 wherever the mask is 0
//   window_gather_flip / window_tta_merge  mirror test-time augmentation (not in the reference):
//                  the gather with a flip code per row, and the mean of a window's K predictions,
//                  each flipped back, written to the window's row of the prediction buffer
#include "common.h"
using namespace l3u;

namespace {

__global__ __launch_bounds__(256) void window_gather_kernel(
    const float* __restrict__ img, int D, int H, int W, const int* __restrict__ pos, int pd,
    int ph, int pw, float* __restrict__ out) {
  const int b = blockIdx.y;
  const long long P = (long long)pd * ph * pw;
  const int z0 = pos[3 * b], y0 = pos[3 * b + 1], x0 = pos[3 * b + 2];
  float* o = out + (long long)b * P;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < P; i += (long long)gridDim.x * 256) {
    const int k = (int)(i % pw), t = (int)(i / pw), j = t % ph, l = t / ph;
    const int z = z0 + l, y = y0 + j, x = x0 + k;
    o[i] = (z < D && y < H && x < W) ? img[((long long)z * H + y) * W + x] : 0.f;
  }
}

// covering window range [lo, hi) along one axis: positions ascending, window at p covers
// [p, p + len)
L3U_DEV void cover(const int* __restrict__ p, int n, int len, int v, int& lo, int& hi) {
  lo = n;
  hi = 0;
  for (int i = 0; i < n; ++i) {
    if (p[i] <= v && v < p[i] + len) {
      lo = min(lo, i);
      hi = max(hi, i + 1);
    }
  }
}

__global__ __launch_bounds__(256) void window_blend_kernel(
    const float* __restrict__ preds, const int* __restrict__ zp, int nz, const int* __restrict__ yp,
    int ny, const int* __restrict__ xp, int nx, const float* __restrict__ imp, int D, int H, int W,
    int pd, int ph, int pw, float* __restrict__ prob) {
  const long long V = (long long)D * H * W, P = (long long)pd * ph * pw;
  for (long long v = blockIdx.x * 256ll + threadIdx.x; v < V; v += (long long)gridDim.x * 256) {
    const int x = (int)(v % W), t = (int)(v / W), y = t % H, z = t / H;
    int z_lo, z_hi, y_lo, y_hi, x_lo, x_hi;
    cover(zp, nz, pd, z, z_lo, z_hi);
    cover(yp, ny, ph, y, y_lo, y_hi);
    cover(xp, nx, pw, x, x_lo, x_hi);
    float acc = 0.f, cnt = 0.f;
    for (int iz = z_lo; iz < z_hi; ++iz)
      for (int iy = y_lo; iy < y_hi; ++iy)
        for (int ix = x_lo; ix < x_hi; ++ix) {
          const long long li = ((long long)(z - zp[iz]) * ph + (y - yp[iy])) * pw + (x - xp[ix]);
          const long long win = ((long long)iz * ny + iy) * nx + ix;
          const float wgt = imp[li];
          acc = __fadd_rn(acc, __fmul_rn(preds[win * P + li], wgt));
          cnt = __fadd_rn(cnt, wgt);
        }
    prob[v] = cnt > 0.f ? __fdiv_rn(acc, cnt) : acc;
  }
}

// ---- windows outside the body mask ---------------------------------------------------------------
// 16-byte units of the mask element types (float32 / uint8) and "some element is nonzero" on one.
// A float compares as a float: -0.0 is zero, a NaN is not.
typedef unsigned int u4_t __attribute__((ext_vector_type(4)));
L3U_DEV bool nz1(float v) { return v != 0.f; }
L3U_DEV bool nz1(unsigned char v) { return v != 0; }
L3U_DEV bool nz16(const float* p) {
  const f4_t v = ldv4(p);
  return v[0] != 0.f || v[1] != 0.f || v[2] != 0.f || v[3] != 0.f;
}
L3U_DEV bool nz16(const unsigned char* p) {
  const u4_t v = *reinterpret_cast<const u4_t*>(p);
  return (v[0] | v[1] | v[2] | v[3]) != 0u;
}

// One workgroup per grid window: keep[win] = 1 iff the window's box, clipped to the volume, holds
// a nonzero mask element.  A row of the box is read in the 16-byte units of the address space (a
// unit that lies inside the row as one vector load, the ragged ends element by element), so rows
// of any alignment take wide loads in their middle.  Work item i = (row, unit); a thread stops at
// its first hit, the workgroup ORs the flags and thread 0 stores the word.  A thread's next load
// waits for the test of its last one, so an empty window (the only kind that is read to the end)
// costs one memory latency per sweep of the workgroup: 1024 threads keep 4x the loads of a
// 256-thread workgroup in flight (48^3 float window: 30 sweeps).
constexpr int kOccThreads = 1024;
template <typename M>
__global__ __launch_bounds__(kOccThreads) void window_occupancy_kernel(
    const M* __restrict__ mask, int D, int H, int W, const int* __restrict__ zp,
    const int* __restrict__ yp, int ny, const int* __restrict__ xp, int nx, int pd, int ph, int pw,
    int* __restrict__ keep) {
  constexpr int E = 16 / (int)sizeof(M);   // elements per unit
  const int win = blockIdx.x;
  const int ix = win % nx, t = win / nx, iy = t % ny, iz = t / ny;
  const int z0 = max(zp[iz], 0), y0 = max(yp[iy], 0), x0 = max(xp[ix], 0);
  const int z1 = min(zp[iz] + pd, D), y1 = min(yp[iy] + ph, H), x1 = min(xp[ix] + pw, W);
  const int cd = z1 - z0, ch = y1 - y0, cw = x1 - x0;
  int found = 0;
  if (cd > 0 && ch > 0 && cw > 0) {
    const int U = (cw + E - 1) / E + 1;   // units a row of cw elements can touch
    const long long items = (long long)cd * ch * U;
    for (long long i = threadIdx.x; i < items && !found; i += kOccThreads) {
      const int u = (int)(i % U), r = (int)(i / U), y = y0 + r % ch, z = z0 + r / ch;
      const M* row = mask + ((long long)z * H + y) * W + x0;
      // element offset (from the row's start) of the row's first 16-byte boundary, then unit u
      const int head = (int)((E - (int)(((uintptr_t)row / sizeof(M)) % E)) % E);
      const int lo = head - E + u * E, hi = lo + E;   // unit u = elements [lo, hi) of the row
      if (lo >= cw || hi <= 0) continue;
      if (lo >= 0 && hi <= cw && ((uintptr_t)(row + lo) & 15) == 0) {
        found = nz16(row + lo);
      } else {
        for (int k = max(lo, 0); k < min(hi, cw); ++k) found |= nz1(row[k]) ? 1 : 0;
      }
    }
  }
  const int any = __syncthreads_or(found);
  if (threadIdx.x == 0) keep[win] = any ? 1 : 0;
}

// window_blend_kernel for a compact prediction buffer and a body mask: a voxel with mask 0 is
// stored as +0 without reading a prediction; any other voxel accumulates its covering windows
// exactly as window_blend_kernel does (same order, same separate multiply / add / divide), reading
// window `win` from row slot[win] of preds, and the quotient is multiplied by the mask value.
// A covering window without a row (slot < 0: the caller broke the contract) is left out.
template <typename M>
__global__ __launch_bounds__(256) void window_blend_masked_kernel(
    const float* __restrict__ preds, const int* __restrict__ slot, const int* __restrict__ zp, int nz,
    const int* __restrict__ yp, int ny, const int* __restrict__ xp, int nx,
    const float* __restrict__ imp, const M* __restrict__ mask, int D, int H, int W, int pd, int ph,
    int pw, float* __restrict__ prob) {
  const long long V = (long long)D * H * W, P = (long long)pd * ph * pw;
  for (long long v = blockIdx.x * 256ll + threadIdx.x; v < V; v += (long long)gridDim.x * 256) {
    const float m = (float)mask[v];
    if (m == 0.f) {
      prob[v] = 0.f;
      continue;
    }
    const int x = (int)(v % W), t = (int)(v / W), y = t % H, z = t / H;
    int z_lo, z_hi, y_lo, y_hi, x_lo, x_hi;
    cover(zp, nz, pd, z, z_lo, z_hi);
    cover(yp, ny, ph, y, y_lo, y_hi);
    cover(xp, nx, pw, x, x_lo, x_hi);
    float acc = 0.f, cnt = 0.f;
    for (int iz = z_lo; iz < z_hi; ++iz)
      for (int iy = y_lo; iy < y_hi; ++iy)
        for (int ix = x_lo; ix < x_hi; ++ix) {
          const long long li = ((long long)(z - zp[iz]) * ph + (y - yp[iy])) * pw + (x - xp[ix]);
          const int s = slot[((long long)iz * ny + iy) * nx + ix];
          if (s < 0) continue;
          const float wgt = imp[li];
          acc = __fadd_rn(acc, __fmul_rn(preds[s * P + li], wgt));
          cnt = __fadd_rn(cnt, wgt);
        }
    prob[v] = __fmul_rn(cnt > 0.f ? __fdiv_rn(acc, cnt) : acc, m);
  }
}

// ---- mirror test-time augmentation ---------------------------------------------------------------
// A flip code has bit a set when axis a (0: D, 1: H, 2: W) of the zero-padded window is reversed.
// The exports read the codes from HOST arrays, check them there and hand them to the kernels in
// the launch arguments: the gather 4 bits per row (a launch covers at most kFlipRows rows), the
// merge 3 bits per term.
constexpr int kFlipRows = 1024;
struct FlipCodes { unsigned w[kFlipRows / 8]; };
L3U_DEV int flip_code(const FlipCodes& c, int r) { return (int)((c.w[r >> 3] >> ((r & 7) * 4)) & 7u); }
L3U_DEV f4_t rev4(f4_t v) { return f4_t{v[3], v[2], v[1], v[0]}; }

// window_gather_kernel with a flip per row: out[b][l][j][k] is the padded window's element at the
// mirrored index along every axis the row's code reverses (so the padding moves to the low end).
// VEC (pw % 4 == 0, out 16-byte aligned): a thread owns the 4 consecutive output elements of one
// W-row; their sources are 4 consecutive volume elements (read in descending order under a W flip),
// taken as one 16-byte load when they lie inside the volume on a 16-byte boundary, else one by one.
// Consecutive lanes read consecutive addresses with or without the W flip (descending lane order
// under it), so a wave's loads cover the same cache lines either way.
template <bool VEC>
__global__ __launch_bounds__(256) void window_gather_flip_kernel(
    const float* __restrict__ img, int D, int H, int W, const int* __restrict__ pos, FlipCodes codes,
    int pd, int ph, int pw, float* __restrict__ out) {
  constexpr int E = VEC ? 4 : 1;
  const int b = blockIdx.y;
  const int c = flip_code(codes, b);
  const bool fz = (c & 1) != 0, fy = (c & 2) != 0, fx = (c & 4) != 0;
  const long long P = (long long)pd * ph * pw, n = P / E;
  const int z0 = pos[3 * b], y0 = pos[3 * b + 1], x0 = pos[3 * b + 2];
  float* o = out + (long long)b * P;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const long long e = i * E;
    const int k = (int)(e % pw), t = (int)(e / pw), j = t % ph, l = t / ph;
    const int z = z0 + (fz ? pd - 1 - l : l), y = y0 + (fy ? ph - 1 - j : j);
    const bool row_in = z < D && y < H;
    const long long ro = ((long long)z * H + y) * W;   // used only when row_in
    if constexpr (VEC) {
      const int xs = x0 + (fx ? pw - 4 - k : k);   // the quad's lowest source x
      f4_t v = {0.f, 0.f, 0.f, 0.f};
      if (row_in) {
        const float* s = img + ro + xs;
        if (xs + 3 < W && ((uintptr_t)s & 15) == 0) {
          v = ldv4(s);
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (xs + q < W) v[q] = s[q];
        }
      }
      *reinterpret_cast<f4_t*>(o + e) = fx ? rev4(v) : v;
    } else {
      const int x = x0 + (fx ? pw - 1 - k : k);
      o[e] = (row_in && x < W) ? img[ro + x] : 0.f;
    }
  }
}

// dst[g][i] = (rows[g*K][F_c0(i)] + rows[g*K + 1][F_c1(i)] + ...) * (1 / K): the K predictions of
// a window, each flipped back, summed in term order with separate fp32 adds starting from term 0,
// then one multiply (exact: K is a power of two).  One thread per output element (VEC: per 4
// consecutive ones of a W-row; the mirrored quad of a W-flipped term is one aligned 16-byte load,
// reversed in registers), all K loads requested before the first add, no atomics.
template <int K, bool VEC>
__global__ __launch_bounds__(256) void window_tta_merge_kernel(
    const float* __restrict__ rows, unsigned codes, int pd, int ph, int pw, float* __restrict__ dst) {
  constexpr int E = VEC ? 4 : 1;
  constexpr float inv = 1.f / K;
  const long long P = (long long)pd * ph * pw, n = P / E;
  const float* src = rows + (long long)blockIdx.y * K * P;
  float* o = dst + (long long)blockIdx.y * P;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const long long e = i * E;
    const int k = (int)(e % pw), t = (int)(e / pw), j = t % ph, l = t / ph;
    if constexpr (VEC) {
      f4_t v[K];
#pragma unroll
      for (int q = 0; q < K; ++q) {
        const unsigned c = codes >> (3 * q);
        const int ls = (c & 1u) ? pd - 1 - l : l, js = (c & 2u) ? ph - 1 - j : j;
        const int ks = (c & 4u) ? pw - 4 - k : k;
        const f4_t a = ldv4(src + q * P + ((long long)ls * ph + js) * pw + ks);
        v[q] = (c & 4u) ? rev4(a) : a;
      }
      f4_t s = v[0];
#pragma unroll
      for (int q = 1; q < K; ++q) s = s + v[q];
      *reinterpret_cast<f4_t*>(o + e) = s * inv;
    } else {
      float v[K];
#pragma unroll
      for (int q = 0; q < K; ++q) {
        const unsigned c = codes >> (3 * q);
        const int ls = (c & 1u) ? pd - 1 - l : l, js = (c & 2u) ? ph - 1 - j : j;
        const int ks = (c & 4u) ? pw - 1 - k : k;
        v[q] = src[q * P + ((long long)ls * ph + js) * pw + ks];
      }
      float s = v[0];
#pragma unroll
      for (int q = 1; q < K; ++q) s = __fadd_rn(s, v[q]);
      o[e] = __fmul_rn(s, inv);
    }
  }
}

template <int K>
void tta_merge_launch(bool vec, dim3 grid, hipStream_t stream, const float* rows, unsigned codes,
                      int pd, int ph, int pw, float* dst) {
  if (vec)
    hipLaunchKernelGGL((window_tta_merge_kernel<K, true>), grid, dim3(256), 0, stream, rows, codes,
                       pd, ph, pw, dst);
  else
    hipLaunchKernelGGL((window_tta_merge_kernel<K, false>), grid, dim3(256), 0, stream, rows, codes,
                       pd, ph, pw, dst);
}

}  // namespace

extern "C" {

int l3u_window_gather(const float* img, int D, int H, int W, const int* pos, int B, int pd, int ph,
                      int pw, float* out, hipStream_t stream) {
  L3U_REQUIRE(D > 0 && H > 0 && W > 0 && B > 0 && pd > 0 && ph > 0 && pw > 0);
  const long long P = (long long)pd * ph * pw;
  long long nb = (P + 1023) / 1024;
  if (nb > 1024) nb = 1024;
  hipLaunchKernelGGL(window_gather_kernel, dim3((int)nb, B), dim3(256), 0, stream, img, D, H, W, pos,
                     pd, ph, pw, out);
  L3U_CHECK_LAUNCH();
}

int l3u_window_blend(const float* preds, const int* zpos, int nz, const int* ypos, int ny,
                     const int* xpos, int nx, const float* imp, int D, int H, int W, int pd, int ph,
                     int pw, float* prob, hipStream_t stream) {
  L3U_REQUIRE(D > 0 && H > 0 && W > 0 && nz > 0 && ny > 0 && nx > 0);
  const long long V = (long long)D * H * W;
  long long nb = (V + 255) / 256;
  if (nb > 65536) nb = 65536;
  hipLaunchKernelGGL(window_blend_kernel, dim3((int)nb), dim3(256), 0, stream, preds, zpos, nz, ypos,
                     ny, xpos, nx, imp, D, H, W, pd, ph, pw, prob);
  L3U_CHECK_LAUNCH();
}

int l3u_window_occupancy(const void* mask, int mask_dtype, int D, int H, int W, const int* zpos,
                         int nz, const int* ypos, int ny, const int* xpos, int nx, int pd, int ph,
                         int pw, int* keep, hipStream_t stream) {
  L3U_REQUIRE(D > 0 && H > 0 && W > 0 && nz > 0 && ny > 0 && nx > 0 && pd > 0 && ph > 0 && pw > 0);
  L3U_REQUIRE(mask_dtype == 0 || mask_dtype == 2);
  const long long nwin = (long long)nz * ny * nx;
  L3U_REQUIRE(nwin <= 0x7fffffffll);
  const dim3 grid((int)nwin), block(kOccThreads);
  if (mask_dtype == 0)
    hipLaunchKernelGGL(window_occupancy_kernel<float>, grid, block, 0, stream,
                       static_cast<const float*>(mask), D, H, W, zpos, ypos, ny, xpos, nx, pd, ph,
                       pw, keep);
  else
    hipLaunchKernelGGL(window_occupancy_kernel<unsigned char>, grid, block, 0, stream,
                       static_cast<const unsigned char*>(mask), D, H, W, zpos, ypos, ny, xpos, nx,
                       pd, ph, pw, keep);
  L3U_CHECK_LAUNCH();
}

int l3u_window_blend_masked(const float* preds, const int* slot, const int* zpos, int nz,
                            const int* ypos, int ny, const int* xpos, int nx, const float* imp,
                            const void* mask, int mask_dtype, int D, int H, int W, int pd, int ph,
                            int pw, float* prob, hipStream_t stream) {
  L3U_REQUIRE(D > 0 && H > 0 && W > 0 && nz > 0 && ny > 0 && nx > 0 && pd > 0 && ph > 0 && pw > 0);
  L3U_REQUIRE(mask_dtype == 0 || mask_dtype == 2);
  const long long V = (long long)D * H * W;
  long long nb = (V + 255) / 256;
  if (nb > 65536) nb = 65536;
  if (mask_dtype == 0)
    hipLaunchKernelGGL(window_blend_masked_kernel<float>, dim3((int)nb), dim3(256), 0, stream, preds,
                       slot, zpos, nz, ypos, ny, xpos, nx, imp, static_cast<const float*>(mask), D,
                       H, W, pd, ph, pw, prob);
  else
    hipLaunchKernelGGL(window_blend_masked_kernel<unsigned char>, dim3((int)nb), dim3(256), 0,
                       stream, preds, slot, zpos, nz, ypos, ny, xpos, nx, imp,
                       static_cast<const unsigned char*>(mask), D, H, W, pd, ph, pw, prob);
  L3U_CHECK_LAUNCH();
}

int l3u_window_gather_flip(const float* img, int D, int H, int W, const int* pos, const int* code,
                           int R, int pd, int ph, int pw, float* out, hipStream_t stream) {
  L3U_REQUIRE(D > 0 && H > 0 && W > 0 && R > 0 && pd > 0 && ph > 0 && pw > 0 && code != nullptr);
  for (int r = 0; r < R; ++r) L3U_REQUIRE(code[r] >= 0 && code[r] <= 7);
  const long long P = (long long)pd * ph * pw;
  const bool vec = pw % 4 == 0 && ((uintptr_t)out & 15) == 0;   // then every row and quad of out is aligned
  const long long n = vec ? P / 4 : P;
  long long nb = vec ? (n + 255) / 256 : (n + 1023) / 1024;
  if (nb > 1024) nb = 1024;
  for (int r0 = 0; r0 < R; r0 += kFlipRows) {
    const int nr = R - r0 < kFlipRows ? R - r0 : kFlipRows;
    FlipCodes fc = {};
    for (int r = 0; r < nr; ++r) fc.w[r >> 3] |= (unsigned)code[r0 + r] << ((r & 7) * 4);
    const dim3 grid((int)nb, nr);
    if (vec)
      hipLaunchKernelGGL(window_gather_flip_kernel<true>, grid, dim3(256), 0, stream, img, D, H, W,
                         pos + 3ll * r0, fc, pd, ph, pw, out + r0 * P);
    else
      hipLaunchKernelGGL(window_gather_flip_kernel<false>, grid, dim3(256), 0, stream, img, D, H, W,
                         pos + 3ll * r0, fc, pd, ph, pw, out + r0 * P);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return (int)err;
  }
  return (int)hipSuccess;
}

int l3u_window_tta_merge(const float* rows, const int* codes, int K, int G, int pd, int ph, int pw,
                         float* dst, hipStream_t stream) {
  L3U_REQUIRE((K == 1 || K == 2 || K == 4 || K == 8) && G > 0 && pd > 0 && ph > 0 && pw > 0);
  L3U_REQUIRE(G <= 65535 && codes != nullptr);
  unsigned packed = 0;
  for (int q = 0; q < K; ++q) {
    L3U_REQUIRE(codes[q] >= 0 && codes[q] <= 7);
    packed |= (unsigned)codes[q] << (3 * q);
  }
  const long long P = (long long)pd * ph * pw;
  const bool vec = pw % 4 == 0 && (((uintptr_t)rows | (uintptr_t)dst) & 15) == 0;
  const long long n = vec ? P / 4 : P;
  long long nb = (n + 255) / 256;
  if (nb > 4096) nb = 4096;
  const dim3 grid((int)nb, G);
  switch (K) {
    case 1: tta_merge_launch<1>(vec, grid, stream, rows, packed, pd, ph, pw, dst); break;
    case 2: tta_merge_launch<2>(vec, grid, stream, rows, packed, pd, ph, pw, dst); break;
    case 4: tta_merge_launch<4>(vec, grid, stream, rows, packed, pd, ph, pw, dst); break;
    default: tta_merge_launch<8>(vec, grid, stream, rows, packed, pd, ph, pw, dst); break;
  }
  L3U_CHECK_LAUNCH();
}

}  // extern "C"
