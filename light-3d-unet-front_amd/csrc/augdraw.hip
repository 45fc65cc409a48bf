// The random draws behind a batch of training patches, made on the device (include/l3u.h,
// "Training-patch draws on the device": the generator, the slots and the decision order are
// defined there and restated in Python by light_unet/patches.py restate_draws).  Replaces the
// per-item host RNG calls of PatchDataset.__getitem__ / _augment and MixedPatchDataset.__getitem__
// (light_unet/datasets/patch_dataset.py:114-220, :254-261) and the upload of their records and of
// the float64 noise array: with the step counter on the device, a captured
// l3u_aug_draw -> l3u_aug_patches -> l3u_counter_add chain draws a fresh batch per replay.
//
// Two launches: draw_kernel, one thread per item (decisions, the raw record, the l3u_aug_param
// record with its derived constants in float64, the per-domain counts), and noise_kernel, one
// thread per voxel of the items whose noise is on (Box-Muller in float64).  The settings travel by
// value in the kernel arguments; the tables and volumes are device memory.
#include "common.h"
using namespace l3u;

namespace {

typedef unsigned long long u64;

// the layouts light_unet/_native.py mirrors with ctypes (tests/test_aug_draw.py pins the same sizes)
static_assert(sizeof(l3u_aug_case) == 32 && sizeof(l3u_aug_tables) == 32, "l3u_aug_case / tables");
static_assert(sizeof(l3u_aug_cfg) == 232 && sizeof(l3u_aug_draw_rec) == 88, "l3u_aug_cfg / draw_rec");

struct DrawArgs {
  l3u_aug_tables tab[2];
  l3u_aug_cfg cfg[2];
  int ndom;
  double fl_ratio;
  u64 seed;
  const int* step;
  int B, pz, py, px;
};

L3U_DEV u64 draw_key(u64 seed, int step, int item) {
  return splitmix64(seed ^ splitmix64(((u64)(unsigned)step << 32) | (u64)(unsigned)item));
}
L3U_DEV u64 draw_bits(u64 key, int slot, u64 v) { return splitmix64(key ^ splitmix64((v << 8) | (u64)slot)); }
L3U_DEV double unit(u64 h) { return (double)(h >> 11) * 0x1p-53; }
L3U_DEV int choice(u64 h, int n) { return (int)__umul64hi(h, (u64)n); }
// lo + (hi - lo) * u with the product rounded on its own (no FMA), as numpy's uniform computes it
L3U_DEV double range(double lo, double hi, double u) {
  double p = (hi - lo) * u;
  asm volatile("" : "+v"(p));
  return lo + p;
}

// field-wise picks (a run-time index into the by-value argument arrays would copy them to scratch)
L3U_DEV const l3u_aug_tables& pick(const DrawArgs& a, const l3u_aug_tables*, int d) { return d ? a.tab[1] : a.tab[0]; }
L3U_DEV const l3u_aug_cfg& pick(const DrawArgs& a, const l3u_aug_cfg*, int d) { return d ? a.cfg[1] : a.cfg[0]; }

__global__ __launch_bounds__(64) void draw_kernel(DrawArgs a, l3u_aug_draw_rec* __restrict__ recs,
                                                  l3u_aug_param* __restrict__ prm,
                                                  int* __restrict__ counts) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= a.B) return;
  const int st = *a.step;
  const u64 key = draw_key(a.seed, st, b);
  auto bits = [&](int slot) { return draw_bits(key, slot, 0); };

  // MixedPatchDataset.__getitem__ (patch_dataset.py:254-261)
  int dom = 0;
  if (a.ndom == 2) {
    const int nfl = a.tab[0].n_lesion + a.tab[0].n_background;
    const int ndl = a.tab[1].n_lesion + a.tab[1].n_background;
    if (unit(bits(L3U_DRAW_DOMAIN)) < a.fl_ratio && nfl > 0) {
      if (counts) atomicAdd(counts, 1);
    } else if (ndl > 0) {
      dom = 1;
      if (counts) atomicAdd(counts + 1, 1);
    }
  }
  const l3u_aug_tables& T = pick(a, (const l3u_aug_tables*)nullptr, dom);
  const l3u_aug_cfg& C = pick(a, (const l3u_aug_cfg*)nullptr, dom);

  // PatchDataset.__getitem__'s location (patch_dataset.py:115-124)
  int table;
  if (unit(bits(L3U_DRAW_TABLE)) < C.lesion_ratio && T.n_lesion > 0) table = 0;
  else if (T.n_background > 0) table = 1;
  else table = 0;
  const int nrow = table ? T.n_background : T.n_lesion;
  const int loc = choice(bits(L3U_DRAW_LOCATION), nrow);
  const int* row = (table ? T.background : T.lesion) + 4ll * loc;
  const int ci = row[0], cz = row[1], cy = row[2], cx = row[3];
  const l3u_aug_case cs = T.cases[ci];

  // _augment's draws (patch_dataset.py:156-220): flip, rotation, scale, shift, noise
  l3u_aug_draw_rec r;
  r.domain = dom, r.case_idx = ci, r.table = table, r.loc = loc;
  r.cz = cz, r.cy = cy, r.cx = cx;
  r.step = st;
  r.flip_on = C.flip_on && unit(bits(L3U_DRAW_FLIP_ON)) < C.flip_prob;
  r.flip_axis = -1;
  if (r.flip_on) {
    const int k = choice(bits(L3U_DRAW_FLIP_AXIS), C.flip_naxes);
    r.flip_axis = C.flip_axes[k];
  }
  r.rot_on = C.rot_on && unit(bits(L3U_DRAW_ROT_ON)) < C.rot_prob;
  r.angle = 0.0;
  r.rot_a0 = r.rot_a1 = -1;
  if (r.rot_on) {
    r.angle = range(C.rot_lo, C.rot_hi, unit(bits(L3U_DRAW_ROT_ANGLE)));
    const int k = choice(bits(L3U_DRAW_ROT_PLANE), C.rot_nplanes);
    r.rot_a0 = C.rot_planes[k][0];
    r.rot_a1 = C.rot_planes[k][1];
  }
  r.scale_on = C.scale_on && unit(bits(L3U_DRAW_SCALE_ON)) < C.scale_prob;
  r.scale = r.scale_on ? range(C.scale_lo, C.scale_hi, unit(bits(L3U_DRAW_SCALE))) : 0.0;
  r.shift_on = C.shift_on && unit(bits(L3U_DRAW_SHIFT_ON)) < C.shift_prob;
  r.shift = r.shift_on ? range(C.shift_lo, C.shift_hi, unit(bits(L3U_DRAW_SHIFT))) : 0.0;
  r.noise_on = C.noise_on && unit(bits(L3U_DRAW_NOISE_ON)) < C.noise_prob;
  recs[b] = r;

  // the l3u_aug_param record, as light_unet/patches.py aug_param forms it
  const int pdim[3] = {a.pz, a.py, a.px};
  l3u_aug_param p;
  p.image = cs.image, p.label = cs.label;
  p.z0 = max(0, cz - a.pz / 2), p.y0 = max(0, cy - a.py / 2), p.x0 = max(0, cx - a.px / 2);
  p.sd = cs.sd, p.sh = cs.sh, p.sw = cs.sw;
  p.pz = a.pz, p.py = a.py, p.px = a.px;
  p.flip = r.flip_axis;
  p.rot_a0 = p.rot_a1 = -1;
  p.rot_c = p.rot_s = p.rot_off0 = p.rot_off1 = 0.0;
  if (r.rot_on) {
    const int a0 = min(r.rot_a0, r.rot_a1), a1 = max(r.rot_a0, r.rot_a1);
    double c, s;
    if (fmod(r.angle, 90.0) == 0.0) {   // exact at the quadrant angles, as cosdg / sindg are
      const int q = (((int)floor(r.angle / 90.0)) % 4 + 4) % 4;
      c = q == 0 ? 1.0 : (q == 2 ? -1.0 : 0.0);
      s = q == 1 ? 1.0 : (q == 3 ? -1.0 : 0.0);
    } else {
      const double rad = r.angle * 0.017453292519943295;
      c = cos(rad);
      s = sin(rad);
    }
    const double i0 = (double)(a0 == 0 ? a.pz : (a0 == 1 ? a.py : a.px) ) - 1.0;
    const double i1 = (double)(a1 == 0 ? a.pz : (a1 == 1 ? a.py : a.px) ) - 1.0;
    const double ic0 = i0 / 2, ic1 = i1 / 2;
    p.rot_a0 = a0, p.rot_a1 = a1;
    p.rot_c = c, p.rot_s = s;
    p.rot_off0 = ic0 - (c * ic0 + s * ic1);
    p.rot_off1 = ic1 - (-s * ic0 + c * ic1);
  }
  p.zoom = r.scale_on;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    p.zs[k] = p.zst[k] = 0;
    p.zf[k] = 0.0;
    if (r.scale_on) {
      const int n = pdim[k];
      const int zs = (int)rint((double)n * r.scale);   // Python's round: half to even
      p.zs[k] = zs;
      p.zst[k] = zs > n ? (zs - n) / 2 : 0;
      p.zf[k] = zs != 1 ? (double)(n - 1) / (double)(zs - 1) : 1.0;
    }
  }
  p.shift_on = r.shift_on;
  p.shift = (float)r.shift;
  p.noise_on = r.noise_on;
  prm[b] = p;
}

__global__ __launch_bounds__(256) void noise_kernel(DrawArgs a, const l3u_aug_draw_rec* __restrict__ recs,
                                                    double* __restrict__ noise, long long P) {
  const long long n = (long long)a.B * P;
  const int st = *a.step;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int b = (int)(i / P);
    if (!recs[b].noise_on) continue;
    const u64 v = (u64)(i - (long long)b * P);
    const double sigma = recs[b].domain ? a.cfg[1].noise_sigma : a.cfg[0].noise_sigma;
    const u64 key = draw_key(a.seed, st, b);
    const double u1 = (double)((draw_bits(key, L3U_DRAW_NOISE_U1, v) >> 11) + 1) * 0x1p-53;   // (0, 1]
    const double u2 = unit(draw_bits(key, L3U_DRAW_NOISE_U2, v));
    const double rr = sqrt(-2.0 * log(u1));
    noise[i] = sigma * (rr * cos(6.283185307179586 * u2));
  }
}

bool cfg_ok(const l3u_aug_cfg& c) {
  if (c.flip_on && (c.flip_naxes < 1 || c.flip_naxes > L3U_DRAW_MAX_AXES)) return false;
  if (c.rot_on && (c.rot_nplanes < 1 || c.rot_nplanes > L3U_DRAW_MAX_AXES)) return false;
  for (int k = 0; c.flip_on && k < c.flip_naxes; ++k)
    if (c.flip_axes[k] < 0 || c.flip_axes[k] > 2) return false;
  for (int k = 0; c.rot_on && k < c.rot_nplanes; ++k) {
    const int a0 = c.rot_planes[k][0], a1 = c.rot_planes[k][1];
    if (a0 < 0 || a0 > 2 || a1 < 0 || a1 > 2 || a0 == a1) return false;
  }
  return true;
}

}  // namespace

extern "C" int l3u_aug_draw(const l3u_aug_tables* tables, const l3u_aug_cfg* cfgs, int ndom,
                            double fl_ratio, unsigned long long seed, const int* step, int B, int pz,
                            int py, int px, l3u_aug_draw_rec* recs, l3u_aug_param* params,
                            double* noise, int* counts, hipStream_t stream) {
  L3U_REQUIRE(tables && cfgs && (ndom == 1 || ndom == 2) && step && B > 0 && pz > 0 && py > 0 &&
              px > 0 && recs && params && noise);
  DrawArgs a;
  long long rows = 0;
  for (int d = 0; d < 2; ++d) {
    a.tab[d] = tables[d < ndom ? d : 0];
    a.cfg[d] = cfgs[d < ndom ? d : 0];
    const l3u_aug_tables& t = a.tab[d];
    L3U_REQUIRE(t.n_lesion >= 0 && t.n_background >= 0 && cfg_ok(a.cfg[d]));
    L3U_REQUIRE(t.cases || t.n_lesion + t.n_background == 0);
    L3U_REQUIRE((t.lesion || t.n_lesion == 0) && (t.background || t.n_background == 0));
    if (d < ndom) rows += (long long)t.n_lesion + t.n_background;
  }
  // a domain without rows is never chosen while the other has some; a single dataset needs rows
  L3U_REQUIRE(rows > 0 && (ndom == 2 || a.tab[0].n_lesion + a.tab[0].n_background > 0));
  a.ndom = ndom, a.fl_ratio = fl_ratio, a.seed = seed, a.step = step;
  a.B = B, a.pz = pz, a.py = py, a.px = px;
  const long long P = (long long)pz * py * px, n = (long long)B * P;
  const long long nb = (n + 255) / 256;
  hipLaunchKernelGGL(draw_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, a, recs, params, counts);
  hipLaunchKernelGGL(noise_kernel, dim3((int)(nb > 8192 ? 8192 : nb)), dim3(256), 0, stream, a, recs,
                     noise, P);
  L3U_CHECK_LAUNCH();
}
