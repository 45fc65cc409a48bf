/*
 * l3u.h — C ABI of the MI355X (gfx950) hot path of the Light-3D-U-Net
 *         (Lightweight3DUNet training / inference step + FocalTverskyLoss).
 *
 * Library: light-3d-unet-front_amd/lib/libl3u_hip.so  (built by `make` in that directory).
 *
 * Conventions (every entry point):
 *   - plain device pointers + sizes, no framework types; the caller owns all memory, nothing is
 *     allocated inside, so every call is hipGraph-capturable;
 *   - the last argument is the hipStream_t to enqueue on; calls are asynchronous;
 *   - the return value is a hipError_t as int (0 = hipSuccess; hipErrorInvalidValue for a shape
 *     the kernels do not support, e.g. an H*W plane above 4096 voxels for the stencil);
 *   - activations are NCDHW with the spatial volume S = D*H*W contiguous per (n, c), stored as fp32
 *     or — entry points with the suffix _bf16, same arguments otherwise — as bf16 (l3u_bf16, the
 *     raw 16-bit pattern); kernels compute in fp32 either way (bf16 loads widen, stores round to
 *     nearest even), weights / records / partial sums are always fp32 (fp64 where marked); a tensor
 *     is (pointer, batch stride in elements) — channel stride is always S.  A batch stride larger
 *     than C*S addresses one channel range of a concatenation buffer (zero-copy torch.cat);
 *   - "rec" is the per-(n,c) InstanceNorm record of 8 floats:
 *       {mean, rstd, scale = k*gamma*rstd, shift = k*beta, k, gamma, beta, 0}
 *     and the normalised, activated value is lrelu(scale*(y - mean) + shift)
 *     with k the Dropout3d keep scale (0 or 1/(1-p); 1 without dropout);
 *   - partial-sum buffers are reduced in a fixed order (l3u_reduce_segments), so results are
 *     bitwise run-to-run reproducible.
 *
 * The reference (xxxxxxyp/Light-3D-Unet-Front) is pure Python/PyTorch: it has no native FFI.  Each
 * entry point below names the reference module call it replaces (file:line in the reference);
 * the Python host mirror (light_unet/) binds them through ctypes.
 */
#ifndef L3U_H
#define L3U_H

#include <hip/hip_runtime.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef unsigned short l3u_bf16;   /* bfloat16 bit pattern (torch.bfloat16 storage) */

/* ABI version of this header (L3U_ABI_VERSION); the ctypes binding refuses a library that reports
 * another.  3: l3u_norm_src.rank1, L3U_ADAMW_TICKET_INTS tickets, the l3u_sblock_* entry points
 * removed (round 3); the round-4 entry points.  5: l3u_pw_bwd_chunk (round 6).  Added since
 * without a new version (additive, nothing existing changed): l3u_window_occupancy,
 * l3u_window_blend_masked, l3u_window_gather_flip, l3u_window_tta_merge, l3u_resample,
 * l3u_spline_prefilter, l3u_spline_prefilter_passes, l3u_resample_spline, l3u_gauss_max_radius,
 * l3u_gauss_axis. */
#define L3U_ABI_VERSION 5
int l3u_abi_version(void);

/* Where an InstanceNorm record comes from when a consumer kernel finalizes it itself (no separate
 * l3u_in_finalize launch): the (count, mean, M2) partials l3u_pw_fwd emitted for the producing
 * GEMM, the affine parameters and the Dropout3d stream.  Every workgroup of the consumer merges
 * the partials of its (n, c) in the same fixed order (identical values everywhere) and the first
 * workgroup of each (n, c) stores the record to rec_out for the backward pass.                 */
typedef struct l3u_norm_src {
  const float* stat_part;      /* [N][C][nsb][3] */
  int nsb;
  int layer;                   /* dropout stream id */
  const float* gamma;          /* [C] or NULL (1) */
  const float* beta;           /* [C] or NULL (0) */
  float drop_p;                /* 0: no dropout */
  unsigned long long seed;
  const int* step;             /* device step counter or NULL */
  float* rec_out;              /* [N][C][8] or NULL */
  const float* rank1;          /* [C] or NULL: the normalised tensor is rank-1, channel c =
                                  rank1[c] * ONE stored channel (see "rank-1 operands" below);
                                  the record's slot 7 carries rank1[c] (0 otherwise) */
} l3u_norm_src;

/* Rank-1 operands (the first block's y1 = w1[c] * z1 and r = wsc[c] * x, unet3d.py:163-167 with
 * one input channel): a NEGATIVE batch stride (-ns) on the normalised operand of
 *   l3u_dwpw_fwd (x, with src/rec), l3u_norm_act_fwd / l3u_norm_act_pool_fwd (r),
 *   l3u_norm_act_bwd_reduce[_r1|_up] (r), l3u_pw_bwd (y), l3u_pw_bwd_tail[_r1|_up] (yr),
 *   l3u_dw3_bwd (x, with rec) and l3u_dw3_fwd (x, with rec or src; the shapes of
 *   l3u_dw3_bwd_rank1)
 * means that operand holds ONE channel per sample (batch stride ns) and channel c is
 * record[c][7] * it, the float product the materialised tensor would hold (bit for bit).  The
 * record's slot 7 is set when it is finalized from an l3u_norm_src with rank1 != NULL.  fp32
 * entry points only.                                                                          */

/* ---- depthwise 3x3x3 conv, stride 1, padding 1, no bias ------------------------------------
 * replaces nn.Conv3d(C, C, 3, 1, 1, groups=C, bias=False)
 *          (DepthwiseSeparableConv3d.depthwise, light_unet/models/unet3d.py:16-17, forward :21)
 * w: [C][27].  rec != NULL fuses a = lrelu(scale*(x-mean) + shift) into the input load (the
 * InstanceNorm1 + LeakyReLU + Dropout3d that precede conv2.depthwise, unet3d.py:84-89).      */
int l3u_dw3_nchunk(int N, int C, int D, int H, int W);   /* z/y chunks per (n, c) */
int l3u_dw3_bwd_rank1(int N, int C, int D, int H, int W); /* 1: l3u_dw3_bwd and l3u_dw3_fwd
                                                             take a rank-1 x at this shape */
int l3u_dw3_fwd(const float* x, long long x_nstride, const float* w, const float* rec,
                const l3u_norm_src* src, float* y, long long y_nstride, int N, int C, int D,
                int H, int W, hipStream_t stream);   /* src != NULL: finalize rec in-kernel */
/* fused backward (autograd of the same module): dx = conv^T(dz) (accumulate != 0: dx += ...),
 * dw_part[C][N*nchunk][27] partial weight gradients.  rec != NULL: dx receives
 * dpre = dA * k * lrelu'(pre) and in_part[C][N][nchunk][2] (fp64) = {sum dpre, sum dpre*xhat}.*/
int l3u_dw3_bwd(const float* dz, long long dz_nstride, const float* x, long long x_nstride,
                const float* w, const float* rec, float* dx, long long dx_nstride, int accumulate,
                float* dw_part, double* in_part, int N, int C, int D, int H, int W,
                hipStream_t stream);

/* ---- channel-contraction GEMM on MFMA (v_mfma_f32_16x16x4_f32) ------------------------------
 * Y[n][j][s] = sum_k Wm[j][k] X[n][k][s] (+ bias[j]) (+ Y if accumulate)
 * w_layout 0: Wm[j][k] = w[j*K + k]   (torch Conv3d 1x1 weight [Co][Ci]: forward)
 * w_layout 1: Wm[j][k] = w[k*Nout + j] (transposed: backward-data of a 1x1 conv, and
 *                                       ConvTranspose3d weight [Ci][Co*8])
 * replaces nn.Conv3d(Ci, Co, 1, bias=False)  (DepthwiseSeparableConv3d.pointwise, unet3d.py:18;
 *          shortcut conv unet3d.py:70-73; out_conv unet3d.py:201) and the GEMM of
 *          nn.ConvTranspose3d(Ci, Ci//2, 2, 2) (unet3d.py:119).
 * stat_part != NULL: emits InstanceNorm partials [N][Nout][l3u_pw_stat_nsb(K, Nout, S)][3] = (count, mean, M2)
 * of the output for the nn.InstanceNorm3d that follows (unet3d.py:51,62,72).                  */
int l3u_pw_stat_nsb(int K, int Nout, int S);
int l3u_pw_fwd(const float* x, long long x_nstride, const float* w, int w_layout,
               const float* bias, float* y, long long y_nstride, int accumulate,
               float* stat_part, int N, int K, int Nout, int S, hipStream_t stream);
/* two independent 1x1 convs of the same shape (no bias, no accumulate, w [Nout][K]) in ONE launch
 * (a ResidualBlock's Conv1x1 shortcut, unet3d.py:70-73, and its conv1.pointwise, :18: both
 * K = Cin -> Nout = Cout over the same volume); statistics partials as l3u_pw_fwd, both or none.
 * S and every batch stride % 4 == 0.                                                           */
int l3u_pw_fwd2(const float* xa, long long xa_nstride, const float* wa, float* ya,
                long long ya_nstride, float* stat_a, const float* xb, long long xb_nstride,
                const float* wb, float* yb, long long yb_nstride, float* stat_b, int N, int K,
                int Nout, int S, hipStream_t stream);
/* ---- fused depthwise-separable conv forward (one launch per DepthwiseSeparableConv3d) -------
 * replaces DepthwiseSeparableConv3d.forward (unet3d.py:20-23: depthwise 3^3 then pointwise 1x1)
 * and, with w_sc, the ResidualBlock's Conv1x1 shortcut on the same input (unet3d.py:70-73,80):
 *   Z = dw3(A) (A = x, or lrelu(IN(x))*dropout when rec / src is given: unet3d.py:84-89),
 *   y = w_pw . Z,  r = w_sc . x,  z (optional, may be NULL) = Z for the backward.
 * y_stat / r_stat: InstanceNorm (count, mean, M2) partials in the l3u_pw_fwd format with
 * l3u_dwpw_stat_nsb(...) partials per (n, c).  Supported shapes: l3u_dwpw_supported.          */
int l3u_dwpw_supported(int K, int Nout, int D, int H, int W, int shortcut);
int l3u_dwpw_stat_nsb(int K, int Nout, int D, int H, int W);
int l3u_dwpw_fwd(const float* x, long long x_nstride, const float* w_dw, const float* rec,
                 const l3u_norm_src* src, const float* w_pw, float* y, long long y_nstride,
                 float* y_stat, const float* w_sc, float* r, long long r_nstride, float* r_stat,
                 float* z, long long z_nstride, int N, int K, int Nout, int D, int H, int W,
                 hipStream_t stream);
/* weight gradient partials: part[N*nsc][J][K] = sum_s dY[n][j][s] X[n][k][s] per voxel chunk   */
int l3u_pw_bwd_weight_nparts(int N, int S);
/* the voxel chunk of those partials (nsc = ceil(S / chunk)); a multiple of 256, at most 512: each
 * chunk is one workgroup sweep of the kernels that write them (csrc/pwconv.hip pw_chunk_ok)     */
int l3u_pw_bwd_chunk(int S);
int l3u_pw_bwd_weight(const float* dy, long long dy_nstride, const float* x, long long x_nstride,
                      float* part, int N, int J, int K, int S, hipStream_t stream);

/* fused backward of the same 1x1 conv (Y = W X, W = w[j*K + k], torch weight [J][K]) in one
 * pass over dY: dx[n][k][s] = sum_j W[j][k] dY[n][j][s] (accumulate != 0: dx += ...) and
 * part[l3u_pw_bwd_nparts(N, J, K, S)][J][K] weight-gradient partials (summed over the first
 * index they give the gradient).
 * y != NULL: dy holds dpre of the preceding InstanceNorm and dY is formed on the fly as
 * l3u_in_bwd_apply would (rec / in_part[J][N][npart][2] as for that call); dY is not stored.
 * Replaces the autograd backward of DepthwiseSeparableConv3d.pointwise (unet3d.py:18) and of the
 * shortcut conv (unet3d.py:70-73), with the InstanceNorm backward of unet3d.py:51 folded in.
 * Supported shapes: l3u_pw_bwd_supported(J, K, S) != 0: S % 4 == 0 and either J <= 32, K <= 64
 * (one workgroup per voxel chunk) or J in {64, 128}, any K (one per 64-voxel tile and 16 columns
 * of K, for the small latency-bound levels).                                                     */
int l3u_pw_bwd_supported(int J, int K, int S);
/* the same backward for conv2.pointwise (sel 1: yr = y2, rec = rec2) or the Conv1x1 shortcut
 * (sel 2: yr = r, rec = rec_r) with the block tail's backward (l3u_norm_act_bwd_apply) formed on
 * the fly from dout, out, yr and the l3u_norm_act_bwd_reduce partials tail_part[J][N][npart][3]:
 * dY = rstd*gamma*(g - mean(g) - xhat*mean(g*xhat)), g = dout*lrelu'(out), never written.
 * Supported: l3u_pw_bwd_supported(J, K, S) with J <= 32 (the 48^3 / 24^3 levels).
 * Replaces the autograd backward of norm2 / relu2 / the residual add (unet3d.py:62-63,87-91)
 * fused with that of conv2.pointwise (:18) or the shortcut (:70-73).                            */
int l3u_pw_bwd_tail(const float* dout, long long dout_nstride, const float* out,
                    long long out_nstride, const float* yr, long long yr_nstride, const float* rec,
                    const double* tail_part, int npart, int sel, const float* x,
                    long long x_nstride, const float* w, float* dx, long long dx_nstride,
                    int accumulate, float* part, int N, int J, int K, int S, hipStream_t stream);
/* the same with a rank-1 dout[j] = dscale[j] * dz (dz one channel: l3u_outconv_bwd_dz)       */
int l3u_pw_bwd_tail_r1(const float* dz, long long dz_nstride, const float* dscale,
                       const float* out, long long out_nstride, const float* yr,
                       long long yr_nstride, const float* rec, const double* tail_part, int npart,
                       int sel, const float* x, long long x_nstride, const float* w, float* dx,
                       long long dx_nstride, int accumulate, float* part, int N, int J, int K,
                       int S, hipStream_t stream);
/* the same with dout = dskip + the next level's MaxPool3d backward (as l3u_norm_act_bwd_reduce_up) */
int l3u_pw_bwd_tail_up(const float* dskip, long long dskip_nstride, const float* dpool,
                       long long dpool_nstride, const unsigned char* idx, const float* out,
                       long long out_nstride, const float* yr, long long yr_nstride,
                       const float* rec, const double* tail_part, int npart, int sel,
                       const float* x, long long x_nstride, const float* w, float* dx,
                       long long dx_nstride, int accumulate, float* part, int N, int J, int K, int D,
                       int H, int W, hipStream_t stream);

int l3u_pw_bwd_nparts(int N, int J, int K, int S);
int l3u_pw_bwd(const float* dy, long long dy_nstride, const float* y, long long y_nstride,
               const float* rec, const double* in_part, int npart, const float* x,
               long long x_nstride, const float* w, float* dx, long long dx_nstride, int accumulate,
               float* part, int N, int J, int K, int S, hipStream_t stream);
/* two plain l3u_pw_bwd calls (y == NULL) of the same J, N and S in ONE launch (a ResidualBlock's
 * conv2.pointwise and Conv1x1 shortcut backwards, unet3d.py:18,70-73: both read the block tail's
 * dy2 / dr), for the shapes l3u_pw_bwd2_supported(J, S) accepts (J in {64, 128}, the 12^3 / 6^3
 * levels); each problem gets l3u_pw_bwd_nparts(N, J, K, S) partials and the results are the two
 * calls' bit for bit.                                                                            */
/* the block tail's two pointwise backwards (conv2.pointwise: sel 1, yr = y2; the Conv1x1
 * shortcut: sel 2, yr = r) of l3u_pw_bwd_tail in ONE launch, dout as l3u_pw_bwd_tail (dscale and
 * dpool NULL), l3u_pw_bwd_tail_r1 (dscale) or l3u_pw_bwd_tail_up (dpool, idx and the plane Hf x Wf);
 * dscale and dpool are mutually exclusive (both given: hipErrorInvalidValue, nothing launched);
 * a rank-1 yr (negative yrb_nstride, fp32) only for the second problem and only when J, Ka, Kb
 * <= 16; each problem's partials as l3u_pw_bwd_nparts(N, J, K, S), results bit-identical to the
 * two calls.                                                                                    */
int l3u_pw_bwd_tail_pair(const float* dout, long long dout_nstride, const float* dscale,
                         const float* dpool, long long dpool_nstride, const unsigned char* idx,
                         int Hf, int Wf, const float* out, long long out_nstride,
                         const double* tail_part, int npart, const float* yra, long long yra_nstride,
                         const float* reca, const float* xa, long long xa_nstride, const float* wa,
                         float* dxa, long long dxa_nstride, int acc_a, float* part_a, int Ka,
                         int sel_a, const float* yrb, long long yrb_nstride, const float* recb,
                         const float* xb, long long xb_nstride, const float* wb, float* dxb,
                         long long dxb_nstride, int acc_b, float* part_b, int Kb, int sel_b, int N,
                         int J, int S, hipStream_t stream);
int l3u_pw_bwd2_supported(int J, int S);
int l3u_pw_bwd2(const float* dya, long long dya_nstride, const float* xa, long long xa_nstride,
                const float* wa, float* dxa, long long dxa_nstride, int acc_a, float* part_a, int Ka,
                const float* dyb, long long dyb_nstride, const float* xb, long long xb_nstride,
                const float* wb, float* dxb, long long dxb_nstride, int acc_b, float* part_b, int Kb,
                int N, int J, int S, hipStream_t stream);

/* ---- InstanceNorm3d(affine=True, eps=1e-5) + LeakyReLU(0.01) + Dropout3d + residual --------
 * replaces nn.InstanceNorm3d / nn.LeakyReLU / nn.Dropout3d / "out + residual"
 *          (ResidualBlock.forward, unet3d.py:77-93)
 * in_finalize: merge (count, mean, M2) partials -> rec; drop_p > 0 draws the Dropout3d channel
 * mask from a counter hash of (seed, *step, layer, n, c) (graph-replay safe).               */
int l3u_in_finalize(const float* stat_part, int nsb, const float* gamma, const float* beta,
                    float drop_p, unsigned long long seed, const int* step, int layer, float* rec,
                    int N, int C, hipStream_t stream);
/* block output: out = lrelu(scale2*(y2-mean2) + shift2 + R), R = r (rec_r == NULL, nn.Identity
 * shortcut) or scale_r*(r-mean_r) + shift_r (Conv1x1 + InstanceNorm shortcut)                        */
int l3u_norm_act_nblocks(int S);
/* records come either ready (rec2 / rec_r) or are finalized in-kernel from src2 / src_r
 * (then also stored to src->rec_out); shortcut == 0 means the identity residual (R = r).       */
int l3u_norm_act_fwd(const float* y2, long long y2_nstride, const float* rec2,
                     const l3u_norm_src* src2, const float* r, long long r_nstride,
                     const float* rec_r, const l3u_norm_src* src_r, int shortcut, float* out,
                     long long out_nstride, int N, int C, int S, hipStream_t stream);
/* the same block tail fused with the MaxPool3d(kernel 2, stride 2) that follows it in the encoder
 * (DownBlock, unet3d.py:104-105): also writes pooled [N][C][D/2*H/2*W/2] (batch stride
 * pooled_nstride) and idx (argmax in the window, as l3u_maxpool2_fwd).  Needs even D, H,
 * W % 4 == 0 and 16-byte aligned activations.                                              */
int l3u_norm_act_pool_fwd(const float* y2, long long y2_nstride, const float* rec2,
                          const l3u_norm_src* src2, const float* r, long long r_nstride,
                          const float* rec_r, const l3u_norm_src* src_r, int shortcut, float* out,
                          long long out_nstride, float* pooled, long long pooled_nstride,
                          unsigned char* idx, int N, int C, int D, int H, int W,
                          hipStream_t stream);
/* backward of the block tail: part[C][N][nblocks][3] (fp64) = {sum g, sum g*xhat2, sum g*xhat_r},
 * g = dout * lrelu'(out); then dy2 / dr (dr = g for the identity shortcut)                   */
int l3u_norm_act_bwd_reduce(const float* dout, long long dout_nstride, const float* out,
                            long long out_nstride, const float* y2, long long y2_nstride,
                            const float* rec2, const float* r, long long r_nstride,
                            const float* rec_r, double* part, int N, int C, int S,
                            hipStream_t stream);
/* the same with a rank-1 dout[c] = dscale[c] * dz (dz one channel: l3u_outconv_bwd_dz)      */
int l3u_norm_act_bwd_reduce_r1(const float* dz, long long dz_nstride, const float* dscale,
                               const float* out, long long out_nstride, const float* y2,
                               long long y2_nstride, const float* rec2, const float* r,
                               long long r_nstride, const float* rec_r, double* part, int N, int C,
                               int S, hipStream_t stream);
/* the same with dout = dskip + the MaxPool3d(2) backward of the next level (DownBlock,
 * unet3d.py:104: l3u_maxpool2_bwd's expression applied on load, so the level-output gradient is
 * never stored): dpool [N][C][S/8] (batch stride dpool_nstride), idx [N][C][S/8] as written by
 * l3u_maxpool2_fwd; even D and H, W % 4 == 0.                                                 */
int l3u_norm_act_bwd_reduce_up(const float* dskip, long long dskip_nstride, const float* dpool,
                               long long dpool_nstride, const unsigned char* idx, const float* out,
                               long long out_nstride, const float* y2, long long y2_nstride,
                               const float* rec2, const float* r, long long r_nstride,
                               const float* rec_r, double* part, int N, int C, int D, int H, int W,
                               hipStream_t stream);
int l3u_norm_act_bwd_apply(const float* dout, long long dout_nstride, const float* out,
                           long long out_nstride, const float* y2, long long y2_nstride,
                           const float* rec2, const float* r, long long r_nstride,
                           const float* rec_r, const double* part, float* dy2,
                           long long dy2_nstride, float* dr, long long dr_nstride, int N, int C,
                           int S, hipStream_t stream);
/* reduce + apply as ONE launch when l3u_norm_act_nblocks(S) == 1 (one workgroup per plane: the
 * small levels); same part layout (nblocks = 1) and bit-identical results (unet3d.py:87-91)      */
int l3u_norm_act_bwd(const float* dout, long long dout_nstride, const float* out,
                     long long out_nstride, const float* y2, long long y2_nstride,
                     const float* rec2, const float* r, long long r_nstride, const float* rec_r,
                     double* part, float* dy2, long long dy2_nstride, float* dr,
                     long long dr_nstride, int N, int C, int S, hipStream_t stream);
/* the same with dout = dskip + the next level's MaxPool3d backward of dpool (l3u_maxpool2_bwd
 * folded in: no level-output gradient tensor, one launch fewer; unet3d.py:104,109), for planes of
 * <= 2048 voxels with even D / H and W % 4 == 0; bit-identical to l3u_maxpool2_bwd followed by
 * l3u_norm_act_bwd                                                                              */
int l3u_norm_act_bwd_up(const float* dskip, long long dskip_nstride, const float* dpool,
                        long long dpool_nstride, const unsigned char* idx, const float* out,
                        long long out_nstride, const float* y2, long long y2_nstride,
                        const float* rec2, const float* r, long long r_nstride,
                        const float* rec_r, double* part, float* dy2, long long dy2_nstride,
                        float* dr, long long dr_nstride, int N, int C, int D, int H, int W,
                        hipStream_t stream);
/* inner InstanceNorm backward: dy = rstd*gamma*(dpre - mean(dpre) - xhat*mean(dpre*xhat))     */
int l3u_in_bwd_apply(const float* dpre, long long dpre_nstride, const float* y, long long y_nstride,
                     const float* rec, const double* in_part, int npart, float* dy,
                     long long dy_nstride, int N, int C, int S, hipStream_t stream);

/* ---- MaxPool3d(2, 2) (DownBlock.pool, unet3d.py:101, forward :109) ------------------------
 * idx: uint8 [N][C][So] argmax slot (first max in (dz,dy,dx) order, as torch CPU)
 * bwd: dx = route(dy) + add (add may be NULL) — writes every input voxel                      */
int l3u_maxpool2_fwd(const float* x, long long x_nstride, float* y, long long y_nstride,
                     unsigned char* idx, int N, int C, int D, int H, int W, hipStream_t stream);
int l3u_maxpool2_bwd(const float* dy, long long dy_nstride, const unsigned char* idx,
                     const float* add, long long add_nstride, float* dx, long long dx_nstride,
                     int N, int C, int D, int H, int W, hipStream_t stream);

/* ---- ConvTranspose3d(Ci, Co, 2, 2) (UpBlock.up, unet3d.py:119, forward :127) ---------------
 * the whole forward in one launch: the [Co*8 x Ci] GEMM on MFMA with the scatter (and bias) in
 * its epilogue (x: [N][Ci][D*H*W], w: torch ConvTranspose3d weight [Ci][Co][2][2][2])        */
int l3u_convt_fwd(const float* x, long long x_nstride, const float* w, const float* bias,
                  float* out, long long out_nstride, int N, int Ci, int Co, int D, int H, int W,
                  hipStream_t stream);
/* the whole backward reading dY in place from the up-sampled gradient (no space-to-depth copy):
 * dx = the data-gradient GEMM with its X operand gathered from dy; wpart[P][Ci][Co*8] weight
 * partials and bpart[P][Co] bias partials (fp32, from the weight-gradient launch), P =
 * l3u_pw_bwd_weight_nparts(N, D*H*W) (dy: [N][Co][2D][2H][2W] with batch stride dy_nstride,
 * e.g. the lower half of the decoder's concat gradient)                                        */
int l3u_convt_bwd(const float* dy, long long dy_nstride, const float* x, long long x_nstride,
                  const float* w, float* dx, long long dx_nstride, float* wpart, float* bpart,
                  int N, int Ci, int Co, int D, int H, int W, hipStream_t stream);
/* the same backward as ONE launch (one workgroup per 64 low-res voxels and 16 input channels,
 * split over Co*8 rows by wave): dx, wpart[P][Ci][Co*8] and bpart[P][Co] (fp32) partials with
 * P = l3u_convt_bwd_fused_nparts(...) (0: shape not offered -> use l3u_convt_bwd; offered for
 * Co in {8, 16, 32, 64}, W % 4 == 0 and D*H*W <= 8192, where it beats the three-launch form).
 * Replaces the autograd backward of UpBlock.up (unet3d.py:119).                              */
int l3u_convt_bwd_fused_nparts(int N, int Ci, int Co, int D, int H, int W);
int l3u_convt_bwd_fused(const float* dy, long long dy_nstride, const float* x, long long x_nstride,
                        const float* w, float* dx, long long dx_nstride, float* wpart, float* bpart,
                        int N, int Ci, int Co, int D, int H, int W, hipStream_t stream);
/* ---- out_conv (1x1x1, C->1, bias) + Sigmoid (unet3d.py:201-202, forward :220-221) ----------
 * fwd: p = sigmoid(b + w.h); t != NULL also emits the FocalTversky first-stage partials
 *      ftl_part[N*nblocks][3] = {sum p*t, sum p, sum t} (reduce them with l3u_ftl_reduce)
 * bwd: dz = g*p*(1-p) with g = dp, or (dp == NULL) the FocalTversky gradient of the global sums
 *      (closed form, * gscale[0] if given); dh[c] = w[c]*dz;
 *      part[N*nblocks][C+1] (fp64) = {sum dz*h[c].., sum dz}; loss != NULL (dp == NULL): also
 *      loss[0] = (1 - TI)^gamma of the sums (what l3u_ftl_loss computes; saves that launch)    */
int l3u_outconv_nblocks(int S);
int l3u_outconv_fwd(const float* h, long long h_nstride, const float* w, const float* b, float* p,
                    const float* t, float* ftl_part, int N, int C, int S, hipStream_t stream);
int l3u_outconv_bwd(const float* dp, const float* p, const float* t, const double* sums,
                    double alpha, double beta, double gamma, double smooth, const float* gscale,
                    const float* h, long long h_nstride, const float* w, float* dh,
                    long long dh_nstride, double* part, float* loss, int N, int C, int S,
                    hipStream_t stream);
/* The FocalTversky form of l3u_outconv_bwd with the loss reduction folded in: instead of the
 * global sums it takes the out_conv forward's FocalTversky partials (ftl_part[ftl_nparts][3],
 * l3u_outconv_fwd) and every workgroup reduces them itself, in l3u_ftl_reduce's order (so the
 * sums, the loss and the gradient are bit-identical to l3u_ftl_reduce + l3u_outconv_bwd): the
 * single-process training step needs no separate reduce launch (losses.py:40-54). */
int l3u_outconv_bwd_ftl(const float* p, const float* t, const float* ftl_part, int ftl_nparts,
                        double alpha, double beta, double gamma, double smooth,
                        const float* gscale, const float* h, long long h_nstride, const float* w,
                        float* dh, long long dh_nstride, double* part, float* loss, int N, int C,
                        int S, hipStream_t stream);
/* the two out_conv backward forms writing dz = d(pre-sigmoid) [N][S] (batch stride dh_nstride)
 * into dh instead of dh[c] = w[c] * dz: out_conv (unet3d.py:201) is rank-1, so the last block's
 * tail backward takes dz and w through the _r1 entry points below and the [N][C][S] output
 * gradient is never stored (same values, bit for bit).                                       */
int l3u_outconv_bwd_dz(const float* dp, const float* p, const float* t, const double* sums,
                       double alpha, double beta, double gamma, double smooth, const float* gscale,
                       const float* h, long long h_nstride, const float* w, float* dh,
                       long long dh_nstride, double* part, float* loss, int N, int C, int S,
                       hipStream_t stream);
int l3u_outconv_bwd_ftl_dz(const float* p, const float* t, const float* ftl_part, int ftl_nparts,
                           double alpha, double beta, double gamma, double smooth,
                           const float* gscale, const float* h, long long h_nstride,
                           const float* w, float* dh, long long dh_nstride, double* part,
                           float* loss, int N, int C, int S, hipStream_t stream);

/* ---- Training patches (light_unet/datasets/patch_dataset.py:114-220) -----------------------
 * One record per patch: the case volume it is cut from (device pointers, [sd][sh][sw] fp32), the
 * crop start (max(0, center - patch // 2), zero padded past the volume end), and the augmentation
 * the host drew with the reference's RNG calls: flip axis (-1 none), rotation plane (rot_a0 < rot_a1,
 * -1 none) with scipy.ndimage.rotate's matrix entries and offsets, zoom (zoomed shape zs, the
 * out -> in factor zf = (in - 1) / (out - 1), the centre-crop start zst of the fit back to the
 * patch), intensity shift, gaussian noise on / off (the float64 noise values come in `noise`,
 * [B][pz][py][px], drawn by the host). */
typedef struct l3u_aug_param {
  const float* image;
  const float* label;
  int z0, y0, x0;
  int sd, sh, sw;
  int pz, py, px;
  int flip;
  int rot_a0, rot_a1;
  double rot_c, rot_s, rot_off0, rot_off1;
  int zoom;
  int zs[3];
  int zst[3];
  double zf[3];
  int shift_on;
  float shift;
  int noise_on;
} l3u_aug_param;

/* out_img / out_lab [B][pz][py][px] fp32 (the DataLoader batch, [B, 1, pz, py, px]); tmp_* the
 * same size (the rotated patches the zoom interpolates from). */
int l3u_aug_patches(const l3u_aug_param* params, int B, int pz, int py, int px, const double* noise,
                    float* tmp_img, float* tmp_lab, float* out_img, float* out_lab,
                    hipStream_t stream);

/* ---- Training-patch draws on the device (csrc/augdraw.hip) -----------------------------------
 * The random decisions behind a batch of training patches -- PatchDataset.__getitem__'s location
 * draw (patch_dataset.py:115-124), MixedPatchDataset's domain draw (:254-261) and _augment's
 * draws (:156-220) -- made by a stateless counter-based generator, so a captured launch chain
 * (l3u_aug_draw -> l3u_aug_patches -> l3u_counter_add(step, 1)) draws a fresh batch per replay.
 * Same distribution as the host draws of light_unet/patches.py, a different sample.
 *
 * The generator.  S = splitmix64 (the 64-bit finalizer of csrc/common.h: z += 0x9E3779B97F4A7C15;
 * z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31),
 * all arithmetic mod 2^64:
 *   key(seed, step, item) = S(seed ^ S((uint32(step) << 32) | uint32(item)))
 *   h(slot, v)            = S(key ^ S((v << 8) | slot))     slot < 256: L3U_DRAW_*; v = 0 except
 *                                                           for the noise slots (v = voxel index
 *                                                           in the patch, z-major)
 *   unit u                = (h >> 11) * 2^-53               in [0, 1)
 *   choice among n        = (h * n) >> 64                   high 64 bits of the 128-bit product
 *   range [lo, hi)        = lo + (hi - lo) * u              fp64; difference, product and sum each
 *                                                           rounded on its own (numpy's uniform)
 *   noise[v]              = sigma * (sqrt(-2 * ln u1) * cos(6.283185307179586 * u2)),  fp64,
 *                           u1 = ((h(NOISE_U1, v) >> 11) + 1) * 2^-53 in (0, 1],
 *                           u2 = unit of h(NOISE_U2, v)     (Box-Muller, mean 0)
 * Decisions per item, every probability test `u < prob` (slots in the order they are used):
 *   two domains (FL = 0, DLBCL = 1; len = n_lesion + n_background of a domain's tables):
 *     u(DOMAIN) < fl_ratio and len(FL) > 0 -> FL, counts[0] += 1; else len(DLBCL) > 0 -> DLBCL,
 *     counts[1] += 1; else FL (not counted).  One domain: domain 0, no draw, counts untouched.
 *   u(TABLE) < lesion_ratio and n_lesion > 0 -> lesion table; else n_background > 0 -> background
 *     table; else lesion table.  Row = choice(LOCATION) among the table's rows (case, z, y, x).
 *   flip: on and u(FLIP_ON) < prob -> axis = axes[choice(FLIP_AXIS)]
 *   rotation: on and u(ROT_ON) < prob -> angle = range(ROT_ANGLE), plane = planes[choice(ROT_PLANE)]
 *   scale / shift: on and u(*_ON) < prob -> range(SCALE / SHIFT);   noise: on and u(NOISE_ON) < prob.
 * The l3u_aug_param record is then formed as light_unet/patches.py aug_param forms it: crop start
 * max(0, c - p / 2) (integer division); the plane's axes sorted; rot_c / rot_s = cos / sin of
 * angle * (pi / 180) (exact at multiples of 90 degrees) and the offsets ic - R ic with
 * ic = (p - 1) / 2; zs = rint(p * scale) (half to even), zst = (zs - p) / 2 when zs > p else 0,
 * zf = (p - 1) / (zs - 1), 1 when zs == 1; shift rounded to float.  Unused fields are 0 (axes -1). */
#define L3U_DRAW_DOMAIN 0
#define L3U_DRAW_TABLE 1
#define L3U_DRAW_LOCATION 2
#define L3U_DRAW_FLIP_ON 3
#define L3U_DRAW_FLIP_AXIS 4
#define L3U_DRAW_ROT_ON 5
#define L3U_DRAW_ROT_ANGLE 6
#define L3U_DRAW_ROT_PLANE 7
#define L3U_DRAW_SCALE_ON 8
#define L3U_DRAW_SCALE 9
#define L3U_DRAW_SHIFT_ON 10
#define L3U_DRAW_SHIFT 11
#define L3U_DRAW_NOISE_ON 12
#define L3U_DRAW_NOISE_U1 13
#define L3U_DRAW_NOISE_U2 14
#define L3U_DRAW_MAX_AXES 8   /* entries of a flip-axis / rotation-plane list */

typedef struct l3u_aug_case {      /* one case volume resident on the device, [sd][sh][sw] fp32 */
  const float* image;
  const float* label;
  int sd, sh, sw;
  int pad;
} l3u_aug_case;

typedef struct l3u_aug_tables {    /* one dataset (domain); every pointer is device memory */
  const l3u_aug_case* cases;
  const int* lesion;               /* [n_lesion][4] = (case, z, y, x) */
  const int* background;           /* [n_background][4] */
  int n_lesion, n_background;
} l3u_aug_tables;

typedef struct l3u_aug_cfg {       /* PatchDataset's lesion_patch_ratio and augmentation config */
  double lesion_ratio;
  double flip_prob, rot_prob, scale_prob, shift_prob, noise_prob;
  double rot_lo, rot_hi, scale_lo, scale_hi, shift_lo, shift_hi, noise_sigma;
  int flip_on, rot_on, scale_on, shift_on, noise_on;
  int flip_naxes, rot_nplanes;     /* 1..L3U_DRAW_MAX_AXES where the augmentation is on */
  int flip_axes[L3U_DRAW_MAX_AXES];
  int rot_planes[L3U_DRAW_MAX_AXES][2];
  int pad;
} l3u_aug_cfg;

typedef struct l3u_aug_draw_rec {  /* what was drawn for one item, before any derived constant */
  int domain, case_idx, table;     /* table 0 lesion, 1 background */
  int loc;                         /* row of that table */
  int cz, cy, cx;                  /* the row's centre */
  int flip_on, flip_axis;          /* axis -1 when off */
  int rot_on, rot_a0, rot_a1;      /* the plane as listed in the config (unsorted); -1 when off */
  int scale_on, shift_on, noise_on;
  int step;                        /* the value of *step the item was drawn at */
  double angle, scale, shift;      /* 0 when off */
} l3u_aug_draw_rec;

/* tables[ndom], cfgs[ndom] (ndom 1 or 2; host structs, passed to the kernels by value: the call
 * reads no device memory on the host and allocates nothing).  step: device counter, read by the
 * kernels, NOT advanced here (l3u_counter_add).  recs[B], params[B], noise[B][pz][py][px] (written
 * for the items whose noise is on only) and counts[2] (int32, accumulated with atomicAdd; may be
 * NULL) are device memory.  Two launches: one thread per item, then one per voxel for the noise. */
int l3u_aug_draw(const l3u_aug_tables* tables, const l3u_aug_cfg* cfgs, int ndom, double fl_ratio,
                 unsigned long long seed, const int* step, int B, int pz, int py, int px,
                 l3u_aug_draw_rec* recs, l3u_aug_param* params, double* noise, int* counts,
                 hipStream_t stream);

/* ---- Lesion post-processing (light_unet/models/metrics.py:38-63,107-213;
 *      light_unet/core/inferencer.py:62-111) -------------------------------------------------
 * l3u_ccl_label: connected components of (src >= threshold) over the 6 face neighbours
 * (scipy.ndimage.label's default structure in 3 dims), numbered 1..n in the order of each
 * component's first voxel in a C-order scan (scipy's numbering); background 0.  Workspace:
 * parent[D*H*W] int32, chunk_count[l3u_ccl_nchunks(D*H*W) + 1] int32; the component count
 * lands in chunk_count[l3u_ccl_nchunks(D*H*W)].  label[D*H*W] int32.
 * l3u_ccl_stats: per component l (1-based) 12 uint64: size, sum z, sum y, sum x, min z, y, x,
 * max z, y, x, max prob as float bits (prob optional, >= 0), 0; remap (optional, int32 indexed by
 * the old label) renumbers the labels in place first (0 drops the voxel: the min_size filter).
 * l3u_ccl_pairs: inter[a * (nb + 1) + b] += voxels labelled a in label_a and b in label_b (both
 * > 0); inter zeroed by the caller. */
int l3u_ccl_nchunks(long long n);
int l3u_ccl_label(const float* src, float threshold, int* parent, int* label, int* chunk_count,
                  int D, int H, int W, hipStream_t stream);
int l3u_ccl_stats(int* label, const int* remap, const float* prob, unsigned long long* stats,
                  int ncomp, int D, int H, int W, hipStream_t stream);
int l3u_ccl_pairs(const int* label_a, const int* label_b, int nb, unsigned int* inter, long long n,
                  hipStream_t stream);
/* The batched forms (get_connected_components / match_components / calculate_lesion_metrics on a
 * [B, D, H, W] array, metrics.py:38-63,99-124): ndimage.label's default structure in 4 dims adds
 * the batch axis as a fourth face neighbour (voxel (b, z, y, x) touches (b - 1, z, y, x)), with the
 * same C-order numbering over the whole array; workspace and label sized B*D*H*W.  l3u_ccl_stats_b
 * records the array's three LEADING coordinates: (z, y, x) with lead4 = 0 (a 3-dimensional array,
 * B = 1) and (b, z, y) with lead4 = 1 (a 4-dimensional array, any B) -- the reference keeps the
 * first three of center_of_mass's coordinates whatever the rank.  l3u_ccl_label / l3u_ccl_stats
 * are the B = 1, lead4 = 0 forms. */
int l3u_ccl_label_b(const float* src, float threshold, int* parent, int* label, int* chunk_count,
                    int B, int D, int H, int W, hipStream_t stream);
int l3u_ccl_stats_b(int* label, const int* remap, const float* prob, unsigned long long* stats,
                    int ncomp, int B, int D, int H, int W, int lead4, hipStream_t stream);

/* The threshold sweep (Trainer.validate's threshold_sensitivity_range, trainer.py:423-439): all K
 * binarisations of one probability map in one launch sequence.
 * l3u_thr_levels: p = prob (* mask when given: one fp32 multiply, numpy's float32 product);
 * level[v] = number of k with p[v] >= thr[k] (thr[K] strictly ascending, 1 <= K <= 32; the same
 * fp32 >= as l3u_ccl_label; NaN compares false everywhere), so the foreground at thr[k] is
 * level >= k + 1.  hist[(K + 1) * 2] uint64 (zeroed here): voxels per (level, target >= 0.5),
 * target optional (column 1 stays 0).  masked (optional) receives p.
 * l3u_ccl_label_lv: labels the K binarisations level >= k0 + k + 1, k = 0..K-1 (k0 + K <= 32), of
 * one [D, H, W] volume, each exactly as l3u_ccl_label labels it.  The levels are independent
 * volumes with level-local parent indices (D*H*W < 2^31 whatever K): parent[K*n], label[K*n]
 * int32, chunk_count[K * (l3u_ccl_nchunks(n) + 1)] int32 with each level's component count in the
 * last slot of its row, and offs[K + 1] int32 = exclusive prefix sums of those counts.
 * l3u_ccl_stats_lv: l3u_ccl_stats for all K levels; component l of level k is row
 * offs[k] + l - 1 of stats[total * 12], total = offs[K] > 0.
 * l3u_ccl_pairs_lv: l3u_ccl_pairs of every level against ONE labelling label_b[n] with nb
 * components; level k's (num_k + 1) x (nb + 1) table starts at (offs[k] + k) * (nb + 1) of
 * inter[(offs[K] + K) * (nb + 1)] (zeroed by the caller).
 * l3u_ccl_lv_max_levels: how many levels' workspaces (parent, label, chunk_count) fit into
 * max_bytes for an n-voxel volume, clamped to 1..32 (pure host). */
int l3u_ccl_lv_max_levels(long long n, long long max_bytes);
int l3u_thr_levels(const float* prob, const float* mask, const float* target, const float* thr,
                   int K, unsigned char* level, unsigned long long* hist, float* masked,
                   long long n, hipStream_t stream);
int l3u_ccl_label_lv(const unsigned char* level, int k0, int K, int* parent, int* label,
                     int* chunk_count, int* offs, int D, int H, int W, hipStream_t stream);
int l3u_ccl_stats_lv(const int* label, const float* prob, const int* offs,
                     unsigned long long* stats, int total, int K, int D, int H, int W,
                     hipStream_t stream);
int l3u_ccl_pairs_lv(const int* label_lv, const int* label_b, int nb, const int* offs,
                     unsigned int* inter, int K, long long n, hipStream_t stream);

/* ---- UpBlock pad / crop (light_unet/models/unet3d.py:130-138) -----------------------------
 * dst[n][c][z][y][x] = src[n][c][z-oz][y-oy][x-ox] inside src's (sd, sh, sw) box, 0 elsewhere,
 * over the whole (dd, dh, dw) dst box.  Forward: the ConvTranspose3d output padded to the skip
 * volume (F.pad with diff//2 before, the rest after), written straight into the concat buffer;
 * backward (offsets negated): the concat gradient cropped to the ConvTranspose3d output. */
int l3u_box_copy(const float* src, long long src_nstride, int sd, int sh, int sw, float* dst,
                 long long dst_nstride, int dd, int dh, int dw, int oz, int oy, int ox, int N, int C,
                 hipStream_t stream);

/* ---- FocalTverskyLoss (light_unet/models/losses.py:11-54) ----------------------------------
 * sums = {sum p*t, sum p, sum t} over ALL voxels of the batch (pred.view(-1), losses.py:40-46),
 * reduced in double; loss = (1 - TI)^gamma; bwd writes dL/dp (* gscale[0] if given) or, with
 * through_sigmoid, dL/dz = dL/dp * p(1-p).  Under data parallelism the 3 sums are all-reduced
 * between l3u_ftl_sums and l3u_ftl_loss/bwd (exact global-batch semantics).                  */
int l3u_ftl_nblocks(long long numel);
int l3u_ftl_sums(const float* p, const float* t, long long numel, float* part, double* sums,
                 hipStream_t stream);
/* second stage only (partials from l3u_outconv_fwd): sums[3] = fixed-order sum of part[nparts][3] */
int l3u_ftl_reduce(const float* part, int nparts, double* sums, hipStream_t stream);
int l3u_ftl_loss(const double* sums, double alpha, double beta, double gamma, double smooth,
                 float* loss, hipStream_t stream);
int l3u_ftl_bwd(const float* p, const float* t, long long numel, const double* sums, double alpha,
                double beta, double gamma, double smooth, const float* gscale,
                int through_sigmoid, float* g, hipStream_t stream);

/* ---- The loss family on four sums: FocalTverskyLoss, CombinedLoss, DiceLoss -----------------
 * (light_unet/models/losses.py:11-54, :57-85, :88-113; get_loss_function :116-147)
 * sums[4] (fp64, fixed order) = {sum p*t, sum p, sum t, sum e} over ALL voxels of the batch, with
 * e_i = -(t max(ln p, -100) + (1 - t) max(ln(1 - p), -100)) as nn.BCELoss forms it (losses.py:83).
 *   L = w_ftl (1 - TI)^gamma + w_bce sums[3] / global_numel
 *       + w_dice (1 - (2 s0 + smooth_dice) / U),
 *   U = s1 + s2 + smooth_dice;  TI, alpha, beta, gamma, smooth_ftl as in l3u_ftl_loss.
 *   dL/dp_i = cA t_i + cB (1 - t_i) + cE (p_i - t_i) / max(p_i (1 - p_i), 1e-12),
 *   cA = w_ftl A + w_dice (Q - 2 / U), cB = w_ftl B + w_dice Q, Q = (2 s0 + smooth_dice) / U^2,
 *   cE = w_bce / global_numel (torch's binary_cross_entropy_backward).
 * The descriptor is nine plain scalars; global_numel is the GLOBAL element count (all ranks'
 * voxels under the exact data-parallel mode).  FocalTverskyLoss = (1, a, b, g, s, 0, M, 0, 0),
 * CombinedLoss = (ftl_weight, a, b, g, 1e-6, bce_weight, M, 0, 0), DiceLoss = (0, .., 0, M, 1,
 * smooth).  A term
 * whose weight is 0 is not evaluated.  Part buffers hold [l3u_ftl_nblocks(numel)][4] floats
 * (l3u_loss4_sums) or [N * l3u_outconv_nblocks(S)][4] (l3u_outconv_fwd_loss4); columns 0-2 are
 * bit-identical to the three-column FocalTversky forms.  No allocation, no atomics.           */
int l3u_loss4_sums(const float* p, const float* t, long long numel, float* part, double* sums,
                   hipStream_t stream);
int l3u_loss4_reduce(const float* part, int nparts, double* sums, hipStream_t stream);
int l3u_loss4_value(const double* sums,
    double w_ftl, double alpha, double beta, double gamma, double smooth_ftl, double w_bce,
    double global_numel, double w_dice, double smooth_dice,
    float* loss, hipStream_t stream);
int l3u_loss4_bwd(const float* p, const float* t, long long numel, const double* sums,
    double w_ftl, double alpha, double beta, double gamma, double smooth_ftl, double w_bce,
    double global_numel, double w_dice, double smooth_dice,
    const float* gscale, int through_sigmoid, float* g, hipStream_t stream);
/* l3u_outconv_fwd (unet3d.py:220-221) with the four-column partials ftl_part[N*nblocks][4]
 * (losses.py:40-42, :83, :108-109); t must be given.  The float4 path is taken only when
 * S % 4 == 0, h_nstride % 4 == 0 and h, p, t are 16-byte aligned; otherwise the scalar path.  */
int l3u_outconv_fwd_loss4(const float* h, long long h_nstride, const float* w, const float* b,
    float* p, const float* t, float* ftl_part, int N, int C, int S, hipStream_t stream);
/* l3u_outconv_bwd / l3u_outconv_bwd_dz with the family descriptor in place of (alpha, beta,
 * gamma, smooth) and sums[4] (losses.py:82-85, :108-113); the loss gradient is always formed in
 * the launch (no dp form).  The float4 path needs 16-byte aligned p, t, h, dh as well.         */
int l3u_outconv_bwd_loss4(const float* p, const float* t, const double* sums,
    double w_ftl, double alpha, double beta, double gamma, double smooth_ftl, double w_bce,
    double global_numel, double w_dice, double smooth_dice,
    const float* gscale, const float* h, long long h_nstride, const float* w, float* dh,
    long long dh_nstride, double* part, float* loss, int N, int C, int S, hipStream_t stream);
int l3u_outconv_bwd_loss4_dz(const float* p, const float* t, const double* sums,
    double w_ftl, double alpha, double beta, double gamma, double smooth_ftl, double w_bce,
    double global_numel, double w_dice, double smooth_dice,
    const float* gscale, const float* h, long long h_nstride, const float* w, float* dh,
    long long dh_nstride, double* part, float* loss, int N, int C, int S, hipStream_t stream);
/* the partial-reducing forms (l3u_outconv_bwd_ftl / _ftl_dz for the family): every workgroup
 * reduces loss_part[loss_nparts][4] itself in l3u_loss4_reduce's order, so the result is
 * bit-identical to l3u_loss4_reduce + l3u_outconv_bwd_loss4[_dz] (losses.py:82-85).           */
int l3u_outconv_bwd_loss4p(const float* p, const float* t, const float* loss_part, int loss_nparts,
    double w_ftl, double alpha, double beta, double gamma, double smooth_ftl, double w_bce,
    double global_numel, double w_dice, double smooth_dice,
    const float* gscale, const float* h, long long h_nstride, const float* w, float* dh,
    long long dh_nstride, double* part, float* loss, int N, int C, int S, hipStream_t stream);
int l3u_outconv_bwd_loss4p_dz(const float* p, const float* t, const float* loss_part, int loss_nparts,
    double w_ftl, double alpha, double beta, double gamma, double smooth_ftl, double w_bce,
    double global_numel, double w_dice, double smooth_dice,
    const float* gscale, const float* h, long long h_nstride, const float* w, float* dh,
    long long dh_nstride, double* part, float* loss, int N, int C, int S, hipStream_t stream);

/* ---- the first block's front (in_channels = 1, unet3d.py:163-167) --------------------------
 * one launch for the Conv1x1 shortcut r[c] = wr[c]*x, conv1.depthwise z1 = dw3(x) (one channel,
 * w_dw [27]) and conv1.pointwise y1[c] = w1[c]*z1, with the (count, mean, M2) partials of r and y1
 * ([N][C][l3u_front_nblocks(S)][3], the l3u_pw_fwd format) from the channel's own moments.
 * Replaces three launches of unet3d.py:70-73,16-18 for the init_conv block.  W % 4 == 0.
 * x is the caller's fp32 input; x_copy != NULL also receives x in the storage type (the bf16
 * network's backward reads its input in bf16).  y1 / r == NULL (fp32): not written; the
 * consumers take them as rank-1 operands (w1[c] * z1, w_sc[c] * x: see "Rank-1 operands").      */
int l3u_front_nblocks(int S);
int l3u_front_fwd(const float* x, long long x_nstride, const float* w_dw, const float* w1,
                  const float* wr, float* z1, float* y1, float* r, float* stat1, float* statr,
                  float* x_copy, int N, int C, int D, int H, int W, hipStream_t stream);

/* ---- grouped / dense 3x3x3 conv (stride 1, padding 1, no bias): the
 * use_depthwise_separable=False path of ResidualBlock (GroupedConv3d unet3d.py:26-34, chosen at
 * :46-47 / :57-58; nn.Conv3d unet3d.py:49 / :60, G = 1).  w: torch weight [Cout][Cin/G][3][3][3].
 * fwd: rec != NULL transforms the input on load, a = lrelu(scale*(x-mean)+shift) (the record of
 *      the preceding InstanceNorm + LeakyReLU + Dropout3d, unet3d.py:84-88); stat_part != NULL
 *      also writes the (count, mean, M2) partials [N][Cout][l3u_gconv3_nblocks(S)][3] that
 *      l3u_in_finalize / l3u_norm_src consume (the format of l3u_pw_fwd).
 * bwd_data: dx (+)= conv^T(dy); rec != NULL: the IN-fused form, dx = dpre = conv^T(dy)*k*
 *      lrelu'(pre) with pre from ep (the saved pre-IN activation) and the IN-backward partials
 *      in_part[Cin][N][l3u_gconv3_nblocks(S)][2] as l3u_dw3_bwd writes them.
 * bwd_weight: part[P][Cout][Cin/G][27], P = l3u_gconv3_wgrad_nparts(N, S); rec as in fwd.      */
int l3u_gconv3_nblocks(int S);
int l3u_gconv3_wgrad_nparts(int N, int S);
int l3u_gconv3_fwd(const float* x, long long x_nstride, const float* w, const float* rec,
                   float* y, long long y_nstride, float* stat_part, int N, int Cin, int Cout,
                   int G, int D, int H, int W, hipStream_t stream);
int l3u_gconv3_bwd_data(const float* dy, long long dy_nstride, const float* w, const float* rec,
                        const float* ep, long long ep_nstride, float* dx, long long dx_nstride,
                        int accumulate, double* in_part, int N, int Cin, int Cout, int G, int D,
                        int H, int W, hipStream_t stream);
int l3u_gconv3_bwd_weight(const float* dy, long long dy_nstride, const float* x,
                          long long x_nstride, const float* rec, float* part, int N, int Cin,
                          int Cout, int G, int D, int H, int W, hipStream_t stream);

/* ---- AdamW on the flat parameter buffer (torch.optim.AdamW, trainer.py:75-79) -------------
 * lr and step live on the device (graph-replay safe).  ONE launch: the last workgroup
 * to finish (ticket order; *ticket starts at 0 and is reset) advances *step and, when
 * counter2 != NULL, *counter2 (the model's Dropout3d stream counter, unet3d.py:66, so a
 * captured training step needs no separate counter launches).  p, g, m and v select the path
 * together: when all four are 16-byte aligned the update runs on 16-byte loads and stores (the
 * last numel % 4 elements one by one), otherwise element by element; both give the same bits.  */
int l3u_adamw_tick(float* p, const float* g, float* m, float* v, long long numel, const float* lr,
                   float beta1, float beta2, float eps, float weight_decay, int* step,
                   float grad_scale, int* ticket, int* counter2, hipStream_t stream);

/* ---- deterministic second-stage reduction --------------------------------------------------
 * items[nitems][8] int64 = {src_off, count, istride, tstride, len<=256, dst_off, accumulate, f64}:
 * dst[dst_off+t] (+)= sum_{i<count} src[src_off + i*istride + t*tstride], summed in fp64;
 * f64 != 0: the source is fp64 and offsets/strides count doubles from the same base.
 * Each output is ONE fp32 rounding of an fp64 sum taken in a fixed order (a function of the
 * item alone), and accumulate != 0 adds the prior dst in fp64 before that rounding.
 * src is 16-byte aligned (checked), and every item's per-lane offsets fit 32 bits:
 * (count-1)*istride + (len-1)*tstride < 2^31 (the engine checks it when it records an item). */
int l3u_reduce_segments(const float* src, const long long* items, int nitems, float* dst,
                        hipStream_t stream);
/* the same reduction fused with the AdamW update (l3u_adamw_tick's arithmetic and step /
 * counter2 / ticket protocol) of the parameters it produces, for one process (no gradient
 * exchange between the two): requires that every one of the numel parameters is the output of
 * exactly one item and that no item accumulates; g receives the reduced gradient as well.
 * ticket: L3U_ADAMW_TICKET_INTS zeroed ints (left zeroed; element 0 may be the l3u_adamw_tick
 * ticket of the same optimizer)                                                                */
#define L3U_TICKET_GROUPS 32
#define L3U_TICKET_STRIDE 32
#define L3U_ADAMW_TICKET_INTS (L3U_TICKET_STRIDE * (L3U_TICKET_GROUPS + 1))
int l3u_reduce_segments_adamw(const float* src, const long long* items, int nitems, float* g,
                              float* p, float* m, float* v, const float* lr, float beta1,
                              float beta2, float eps, float weight_decay, int* step,
                              float grad_scale, int* ticket, int* counter2, hipStream_t stream);

/* ---- whole-volume sliding-window inference (light_unet/utils.py:11-173) --------------------
 * gather: out[b] = volume[z:z+pd, y:y+ph, x:x+pw] of window b (pos[b] = {z, y, x}), zero past
 *         the volume edge (utils.py:96-113)
 * blend:  prob[v] = sum_w pred_w[v] * imp[v - pos_w] / sum_w imp[v - pos_w] over the windows
 *         covering v, in the reference's window order (z, y, x) with separate fp32 multiply and
 *         add; windows are the grid zpos x ypos x xpos, preds[(iz*ny + iy)*nx + ix][pd*ph*pw] */
int l3u_window_gather(const float* img, int D, int H, int W, const int* pos, int B, int pd, int ph,
                      int pw, float* out, hipStream_t stream);
int l3u_window_blend(const float* preds, const int* zpos, int nz, const int* ypos, int ny,
                     const int* xpos, int nx, const float* imp, int D, int H, int W, int pd, int ph,
                     int pw, float* prob, hipStream_t stream);

/* The same map times a body mask (prob_map * body_mask, trainer.py:401-402, inferencer.py:161-162)
 * without the forwards of windows that lie outside the mask.  mask: [D][H][W] of mask_dtype 0
 * float or 2 uint8 (l3u_pp_pack's codes); anything else returns hipErrorInvalidValue.
 * occupancy:    keep[(iz*ny + iy)*nx + ix] = 1 if some voxel of that grid window's box, clipped to
 *               the volume, has mask != 0 (a NaN counts as nonzero), else 0; one workgroup per
 *               window, no atomics
 * blend_masked: l3u_window_blend over a compact prediction buffer: window (iz, iy, ix) is row
 *               slot[(iz*ny + iy)*nx + ix] of preds, -1 where it was not computed.  A voxel with
 *               mask == 0 is stored as +0 and reads no prediction; every other voxel is accumulated
 *               as l3u_window_blend does (same window order, separate fp32 multiply / add / divide)
 *               and stored as that quotient times float(mask).  Every window covering a voxel with
 *               mask != 0 must have a row (occupancy keeps all of them); a covering window with a
 *               negative slot is left out of the sums, never indexed.  For finite predictions the
 *               result is bit for bit l3u_window_blend's map times the mask in float32.          */
int l3u_window_occupancy(const void* mask, int mask_dtype, int D, int H, int W, const int* zpos,
                         int nz, const int* ypos, int ny, const int* xpos, int nx, int pd, int ph,
                         int pw, int* keep, hipStream_t stream);
int l3u_window_blend_masked(const float* preds, const int* slot, const int* zpos, int nz,
                            const int* ypos, int ny, const int* xpos, int nx, const float* imp,
                            const void* mask, int mask_dtype, int D, int H, int W, int pd, int ph,
                            int pw, float* prob, hipStream_t stream);

/* Mirror test-time augmentation of the sliding window (not in the reference).  A flip code 0..7
 * has bit a set when axis a (0: D, 1: H, 2: W) of the zero-padded pd x ph x pw window is reversed
 * (F_c; the padding moves to the low end of a reversed axis; F_c is its own inverse).  `code` and
 * `codes` are HOST arrays: they are checked before anything is launched (a value outside 0..7
 * returns hipErrorInvalidValue) and travel in the launch arguments, so a captured launch keeps
 * the codes it was captured with.
 * gather_flip: out[r] = F_code[r] of the window l3u_window_gather cuts at pos[r] (pos: device,
 *              R x {z, y, x}); with every code 0 bit for bit l3u_window_gather's output.
 * tta_merge:   rows: [G*K][pd*ph*pw], the K predictions of window g adjacent (term j computed on
 *              the F_codes[j] input).  dst[g][i] = (rows[g*K][F_codes[0](i)] + rows[g*K + 1][..] +
 *              ...) * (1 / K): separate fp32 adds in term order starting from term 0, then one
 *              multiply; K in {1, 2, 4, 8} (K = 1, code 0: a copy), G <= 65535.  One thread per
 *              output element, no atomics; dst must not overlap rows.
 * Both take 16-byte loads and stores when pw % 4 == 0 and the row pointers are 16-byte aligned
 * (the gather: out; the merge: rows and dst), and an element-wise path otherwise.              */
int l3u_window_gather_flip(const float* img, int D, int H, int W, const int* pos, const int* code,
                           int R, int pd, int ph, int pw, float* out, hipStream_t stream);
int l3u_window_tta_merge(const float* rows, const int* codes, int K, int G, int pd, int ph, int pw,
                         float* dst, hipStream_t stream);

/* storage casts (the bf16 network's input / input gradient); n elements                      */
int l3u_cast_f32_bf16(const float* x, l3u_bf16* y, long long n, hipStream_t stream);
int l3u_cast_bf16_f32(const l3u_bf16* x, float* y, long long n, hipStream_t stream);

/* device counter += value (Dropout3d RNG stream position, advanced once per training forward) */
int l3u_counter_add(int* counter, int value, hipStream_t stream);

/* ---- bf16 twins (BASELINE config 3) --------------------------------------------------------
 * The same calls with the saved activations (forward inputs and outputs: what the backward
 * re-reads) stored as bf16; argument order and meaning are those of the fp32 entry point without
 * the suffix.  Gradients (every backward input/output gradient), weights, biases, InstanceNorm
 * records and the statistics / weight-gradient partials stay fp32 (fp64 where marked), and every
 * kernel computes in fp32 (bf16 loads widen exactly, stores round to nearest even).
 * l3u_outconv_* keep p / dp / t fp32 (the loss runs on fp32 probabilities); l3u_front_fwd reads
 * the caller's fp32 x and can write its bf16 copy (x_copy) for the backward.  l3u_maxpool2_bwd
 * has no bf16 twin: it reads no saved activation.                                          */
int l3u_dw3_fwd_bf16(const l3u_bf16* x, long long x_nstride, const float* w, const float* rec,
                     const l3u_norm_src* src, l3u_bf16* y, long long y_nstride, int N, int C, int D,
                     int H, int W, hipStream_t stream);
int l3u_dw3_bwd_bf16(const float* dz, long long dz_nstride, const l3u_bf16* x, long long x_nstride,
                     const float* w, const float* rec, float* dx, long long dx_nstride,
                     int accumulate, float* dw_part, double* in_part, int N, int C, int D, int H,
                     int W, hipStream_t stream);
int l3u_dwpw_fwd_bf16(const l3u_bf16* x, long long x_nstride, const float* w_dw, const float* rec,
                      const l3u_norm_src* src, const float* w_pw, l3u_bf16* y, long long y_nstride,
                      float* y_stat, const float* w_sc, l3u_bf16* r, long long r_nstride,
                      float* r_stat, l3u_bf16* z, long long z_nstride, int N, int K, int Nout,
                      int D, int H, int W, hipStream_t stream);
int l3u_maxpool2_fwd_bf16(const l3u_bf16* x, long long x_nstride, l3u_bf16* y, long long y_nstride,
                          unsigned char* idx, int N, int C, int D, int H, int W,
                          hipStream_t stream);
int l3u_outconv_fwd_bf16(const l3u_bf16* h, long long h_nstride, const float* w, const float* b,
                         float* p, const float* t, float* ftl_part, int N, int C, int S,
                         hipStream_t stream);
int l3u_outconv_bwd_bf16(const float* dp, const float* p, const float* t, const double* sums,
                         double alpha, double beta, double gamma, double smooth,
                         const float* gscale, const l3u_bf16* h, long long h_nstride,
                         const float* w, float* dh, long long dh_nstride, double* part, float* loss,
                         int N, int C, int S, hipStream_t stream);
int l3u_outconv_bwd_ftl_bf16(const float* p, const float* t, const float* ftl_part, int ftl_nparts,
                             double alpha, double beta, double gamma, double smooth,
                             const float* gscale, const l3u_bf16* h, long long h_nstride,
                             const float* w, float* dh, long long dh_nstride, double* part,
                             float* loss, int N, int C, int S, hipStream_t stream);
int l3u_outconv_bwd_dz_bf16(const float* dp, const float* p, const float* t, const double* sums,
                            double alpha, double beta, double gamma, double smooth,
                            const float* gscale, const l3u_bf16* h, long long h_nstride,
                            const float* w, float* dh, long long dh_nstride, double* part,
                            float* loss, int N, int C, int S, hipStream_t stream);
int l3u_outconv_bwd_ftl_dz_bf16(const float* p, const float* t, const float* ftl_part,
                                int ftl_nparts, double alpha, double beta, double gamma,
                                double smooth, const float* gscale, const l3u_bf16* h,
                                long long h_nstride, const float* w, float* dh,
                                long long dh_nstride, double* part, float* loss, int N, int C,
                                int S, hipStream_t stream);
int l3u_outconv_fwd_loss4_bf16(const l3u_bf16* h, long long h_nstride, const float* w, const float* b,
    float* p, const float* t, float* ftl_part, int N, int C, int S, hipStream_t stream);
int l3u_outconv_bwd_loss4_bf16(const float* p, const float* t, const double* sums,
    double w_ftl, double alpha, double beta, double gamma, double smooth_ftl, double w_bce,
    double global_numel, double w_dice, double smooth_dice,
    const float* gscale, const l3u_bf16* h, long long h_nstride, const float* w, float* dh,
    long long dh_nstride, double* part, float* loss, int N, int C, int S, hipStream_t stream);
int l3u_outconv_bwd_loss4_dz_bf16(const float* p, const float* t, const double* sums,
    double w_ftl, double alpha, double beta, double gamma, double smooth_ftl, double w_bce,
    double global_numel, double w_dice, double smooth_dice,
    const float* gscale, const l3u_bf16* h, long long h_nstride, const float* w, float* dh,
    long long dh_nstride, double* part, float* loss, int N, int C, int S, hipStream_t stream);
int l3u_outconv_bwd_loss4p_bf16(const float* p, const float* t, const float* loss_part, int loss_nparts,
    double w_ftl, double alpha, double beta, double gamma, double smooth_ftl, double w_bce,
    double global_numel, double w_dice, double smooth_dice,
    const float* gscale, const l3u_bf16* h, long long h_nstride, const float* w, float* dh,
    long long dh_nstride, double* part, float* loss, int N, int C, int S, hipStream_t stream);
int l3u_outconv_bwd_loss4p_dz_bf16(const float* p, const float* t, const float* loss_part, int loss_nparts,
    double w_ftl, double alpha, double beta, double gamma, double smooth_ftl, double w_bce,
    double global_numel, double w_dice, double smooth_dice,
    const float* gscale, const l3u_bf16* h, long long h_nstride, const float* w, float* dh,
    long long dh_nstride, double* part, float* loss, int N, int C, int S, hipStream_t stream);
int l3u_box_copy_bf16(const l3u_bf16* src, long long src_nstride, int sd, int sh, int sw,
                      l3u_bf16* dst, long long dst_nstride, int dd, int dh, int dw, int oz, int oy,
                      int ox, int N, int C, hipStream_t stream);
int l3u_front_fwd_bf16(const float* x, long long x_nstride, const float* w_dw, const float* w1,
                       const float* wr, l3u_bf16* z1, l3u_bf16* y1, l3u_bf16* r, float* stat1,
                       float* statr, l3u_bf16* x_copy, int N, int C, int D, int H, int W,
                       hipStream_t stream);
int l3u_norm_act_fwd_bf16(const l3u_bf16* y2, long long y2_nstride, const float* rec2,
                          const l3u_norm_src* src2, const l3u_bf16* r, long long r_nstride,
                          const float* rec_r, const l3u_norm_src* src_r, int shortcut,
                          l3u_bf16* out, long long out_nstride, int N, int C, int S,
                          hipStream_t stream);
int l3u_norm_act_pool_fwd_bf16(const l3u_bf16* y2, long long y2_nstride, const float* rec2,
                               const l3u_norm_src* src2, const l3u_bf16* r, long long r_nstride,
                               const float* rec_r, const l3u_norm_src* src_r, int shortcut,
                               l3u_bf16* out, long long out_nstride, l3u_bf16* pooled,
                               long long pooled_nstride, unsigned char* idx, int N, int C, int D,
                               int H, int W, hipStream_t stream);
int l3u_norm_act_bwd_reduce_bf16(const float* dout, long long dout_nstride, const l3u_bf16* out,
                                 long long out_nstride, const l3u_bf16* y2, long long y2_nstride,
                                 const float* rec2, const l3u_bf16* r, long long r_nstride,
                                 const float* rec_r, double* part, int N, int C, int S,
                                 hipStream_t stream);
int l3u_norm_act_bwd_reduce_up_bf16(const float* dskip, long long dskip_nstride, const float* dpool,
                                    long long dpool_nstride, const unsigned char* idx,
                                    const l3u_bf16* out, long long out_nstride, const l3u_bf16* y2,
                                    long long y2_nstride, const float* rec2, const l3u_bf16* r,
                                    long long r_nstride, const float* rec_r, double* part, int N,
                                    int C, int D, int H, int W, hipStream_t stream);
int l3u_norm_act_bwd_reduce_r1_bf16(const float* dz, long long dz_nstride, const float* dscale,
                                    const l3u_bf16* out, long long out_nstride, const l3u_bf16* y2,
                                    long long y2_nstride, const float* rec2, const l3u_bf16* r,
                                    long long r_nstride, const float* rec_r, double* part, int N,
                                    int C, int S, hipStream_t stream);
int l3u_norm_act_bwd_apply_bf16(const float* dout, long long dout_nstride, const l3u_bf16* out,
                                long long out_nstride, const l3u_bf16* y2, long long y2_nstride,
                                const float* rec2, const l3u_bf16* r, long long r_nstride,
                                const float* rec_r, const double* part, float* dy2,
                                long long dy2_nstride, float* dr, long long dr_nstride, int N,
                                int C, int S, hipStream_t stream);
int l3u_norm_act_bwd_bf16(const float* dout, long long dout_nstride, const l3u_bf16* out,
                          long long out_nstride, const l3u_bf16* y2, long long y2_nstride,
                          const float* rec2, const l3u_bf16* r, long long r_nstride,
                          const float* rec_r, double* part, float* dy2, long long dy2_nstride,
                          float* dr, long long dr_nstride, int N, int C, int S, hipStream_t stream);
int l3u_norm_act_bwd_up_bf16(const float* dskip, long long dskip_nstride, const float* dpool,
                             long long dpool_nstride, const unsigned char* idx,
                             const l3u_bf16* out, long long out_nstride, const l3u_bf16* y2,
                             long long y2_nstride, const float* rec2, const l3u_bf16* r,
                             long long r_nstride, const float* rec_r, double* part, float* dy2,
                             long long dy2_nstride, float* dr, long long dr_nstride, int N, int C,
                             int D, int H, int W, hipStream_t stream);
int l3u_in_bwd_apply_bf16(const float* dpre, long long dpre_nstride, const l3u_bf16* y,
                          long long y_nstride, const float* rec, const double* in_part, int npart,
                          float* dy, long long dy_nstride, int N, int C, int S, hipStream_t stream);
int l3u_pw_fwd_bf16(const l3u_bf16* x, long long x_nstride, const float* w, int w_layout,
                    const float* bias, l3u_bf16* y, long long y_nstride, int accumulate,
                    float* stat_part, int N, int K, int Nout, int S, hipStream_t stream);
int l3u_pw_fwd2_bf16(const l3u_bf16* xa, long long xa_nstride, const float* wa, l3u_bf16* ya,
                     long long ya_nstride, float* stat_a, const l3u_bf16* xb, long long xb_nstride,
                     const float* wb, l3u_bf16* yb, long long yb_nstride, float* stat_b, int N,
                     int K, int Nout, int S, hipStream_t stream);
int l3u_convt_fwd_bf16(const l3u_bf16* x, long long x_nstride, const float* w, const float* bias,
                       l3u_bf16* out, long long out_nstride, int N, int Ci, int Co, int D, int H,
                       int W, hipStream_t stream);
int l3u_pw_bwd_weight_bf16(const float* dy, long long dy_nstride, const l3u_bf16* x,
                           long long x_nstride, float* part, int N, int J, int K, int S,
                           hipStream_t stream);
int l3u_pw_bwd_tail_bf16(const float* dout, long long dout_nstride, const l3u_bf16* out,
                         long long out_nstride, const l3u_bf16* yr, long long yr_nstride,
                         const float* rec, const double* tail_part, int npart, int sel,
                         const l3u_bf16* x, long long x_nstride, const float* w, float* dx,
                         long long dx_nstride, int accumulate, float* part, int N, int J, int K,
                         int S, hipStream_t stream);
int l3u_pw_bwd_tail_up_bf16(const float* dskip, long long dskip_nstride, const float* dpool,
                            long long dpool_nstride, const unsigned char* idx, const l3u_bf16* out,
                            long long out_nstride, const l3u_bf16* yr, long long yr_nstride,
                            const float* rec, const double* tail_part, int npart, int sel,
                            const l3u_bf16* x, long long x_nstride, const float* w, float* dx,
                            long long dx_nstride, int accumulate, float* part, int N, int J, int K,
                            int D, int H, int W, hipStream_t stream);
int l3u_pw_bwd_tail_r1_bf16(const float* dz, long long dz_nstride, const float* dscale,
                            const l3u_bf16* out, long long out_nstride, const l3u_bf16* yr,
                            long long yr_nstride, const float* rec, const double* tail_part,
                            int npart, int sel, const l3u_bf16* x, long long x_nstride,
                            const float* w, float* dx, long long dx_nstride, int accumulate,
                            float* part, int N, int J, int K, int S, hipStream_t stream);
int l3u_pw_bwd_tail_pair_bf16(const float* dout, long long dout_nstride, const float* dscale,
                              const float* dpool, long long dpool_nstride, const unsigned char* idx,
                              int Hf, int Wf, const l3u_bf16* out, long long out_nstride,
                              const double* tail_part, int npart, const l3u_bf16* yra,
                              long long yra_nstride, const float* reca, const l3u_bf16* xa,
                              long long xa_nstride, const float* wa, float* dxa,
                              long long dxa_nstride, int acc_a, float* part_a, int Ka, int sel_a,
                              const l3u_bf16* yrb, long long yrb_nstride, const float* recb,
                              const l3u_bf16* xb, long long xb_nstride, const float* wb, float* dxb,
                              long long dxb_nstride, int acc_b, float* part_b, int Kb, int sel_b,
                              int N, int J, int S, hipStream_t stream);
int l3u_pw_bwd_bf16(const float* dy, long long dy_nstride, const l3u_bf16* y, long long y_nstride,
                    const float* rec, const double* in_part, int npart, const l3u_bf16* x,
                    long long x_nstride, const float* w, float* dx, long long dx_nstride,
                    int accumulate, float* part, int N, int J, int K, int S, hipStream_t stream);
int l3u_pw_bwd2_bf16(const float* dya, long long dya_nstride, const l3u_bf16* xa,
                     long long xa_nstride, const float* wa, float* dxa, long long dxa_nstride,
                     int acc_a, float* part_a, int Ka, const float* dyb, long long dyb_nstride,
                     const l3u_bf16* xb, long long xb_nstride, const float* wb, float* dxb,
                     long long dxb_nstride, int acc_b, float* part_b, int Kb, int N, int J, int S,
                     hipStream_t stream);
int l3u_convt_bwd_fused_bf16(const float* dy, long long dy_nstride, const l3u_bf16* x,
                             long long x_nstride, const float* w, float* dx, long long dx_nstride,
                             float* wpart, float* bpart, int N, int Ci, int Co, int D, int H, int W,
                             hipStream_t stream);
int l3u_convt_bwd_bf16(const float* dy, long long dy_nstride, const l3u_bf16* x,
                       long long x_nstride, const float* w, float* dx, long long dx_nstride,
                       float* wpart, float* bpart, int N, int Ci, int Co, int D, int H, int W,
                       hipStream_t stream);

/* ---- case preprocessing (csrc/preprocess.hip; the reference's scripts/preprocess_data.py) ----
 * l3u_pp_select: the order statistics of src[n] (float, or double when is_f64) at the 0-based
 * ranks r0..r(nranks-1) (1..4 of them, each < n), bit-exact, as doubles into out[0..nranks-1]
 * (a float widens exactly); out[4] receives the number of NaNs in src (they are left out of the
 * ranking: the caller decides what that means).  -0 ranks as +0.  A most-significant-digit-first
 * radix descent over monotone integer keys: per 8-bit digit one histogram sweep (LDS histogram per
 * workgroup, integer atomics: exact and order-independent) and one single-workgroup launch that
 * picks each rank's bin; 4 sweeps for float, 8 for double, no host round trip and no compaction.
 * ws: l3u_pp_select_ws_bytes() bytes of device workspace (cleared by the call).  out: 5 doubles.
 *
 * l3u_pp_normalize: v = (clip(x, lo, hi) - lo) / (hi - lo) * scale + t0 per voxel in fp64, each
 * operation rounded on its own (no fused multiply-add), with lo = clip[0], hi = clip[1] read from
 * device memory (hi > lo).  Writes v to out64 and / or its float rounding to out32 and / or the
 * packed mask v > threshold (compared in fp64) to bits; any of the three may be NULL.
 *
 * Packed masks: one bit per voxel of a [D, H, W] volume, x fastest; a row (z, y) is
 * ceil(W / 64) 64-bit words, bit i of word wx is x = 64 * wx + i, padding bits are 0.
 * l3u_pp_pack: bits from src of dtype 0 float, 1 double, 2 uint8, 3 int32 with op 0: v != 0,
 * 1: v > arg, 2: v == arg (compared as doubles).  l3u_pp_unpack: 0 / 1 into dst of dtype 0 float
 * or 2 uint8.
 * l3u_pp_morph: `iters` iterations (1..l3u_pp_morph_max_iters(W)) of dilation (erode = 0) or
 * erosion (erode = 1) with the 6-neighbour cross, in one launch; everything outside the volume
 * reads as 0 at every iteration, for erosion too.  in != out.
 * l3u_pp_mask_stats: stats[7] int64 = set voxels, min z, y, x, max z, y, x (min 2^31 - 1 and
 * max -1 for an empty mask). */
int l3u_pp_select_ws_bytes(void);
int l3u_pp_select(const void* src, int is_f64, long long n, int nranks, long long r0, long long r1,
                  long long r2, long long r3, void* ws, double* out, hipStream_t stream);
int l3u_pp_normalize(const void* src, int is_f64, const double* clip, double scale, double t0,
                     double threshold, double* out64, float* out32, unsigned long long* bits, int D,
                     int H, int W, hipStream_t stream);
int l3u_pp_pack(const void* src, int dtype, int op, double arg, unsigned long long* bits, int D,
                int H, int W, hipStream_t stream);
int l3u_pp_unpack(const unsigned long long* bits, void* dst, int dtype, int D, int H, int W,
                  hipStream_t stream);
int l3u_pp_morph_max_iters(int W);
int l3u_pp_morph(const unsigned long long* in, unsigned long long* out, int erode, int iters, int D,
                 int H, int W, hipStream_t stream);
int l3u_pp_mask_stats(const unsigned long long* bits, long long* stats, int D, int H, int W,
                      hipStream_t stream);

/* ---- patch locations (csrc/locate.hip; PatchDataset._sample_locations,
 * light_unet/datasets/patch_dataset.py:74-100) ----
 * The reference keeps rows of np.argwhere(label > 0) and of np.argwhere((label == 0) & body_mask)
 * picked by np.random.randint; row k of np.argwhere(m) is the k-th set voxel of m in C order, so
 * the kept rows are rank queries over a predicate that is never materialised.  Over the flat index
 * i = (z * H + y) * W + x of a [D, H, W] volume the two voxel classes are
 *   class 0 (lesion):      label[i] > 0
 *   class 1 (background):  label[i] == 0 && (body == NULL || body[i] != 0)
 * evaluated in the label's own type (label_dtype 0 float, 1 double, as l3u_pp_pack's codes; a NaN
 * or a negative label belongs to neither class); body is one byte per voxel (bool / uint8).
 *
 * l3u_loc_count: prefix[2][nblocks + 1] uint32, nblocks = l3u_loc_nblocks(n): per class the
 * EXCLUSIVE prefix sum of the per-block voxel counts (blocks of L3U_LOC_BLOCK voxels of the flat
 * order), entry nblocks the class total.  Integer sums in a fixed order: no atomics.
 * n = D * H * W with 0 < n < 2^31, else hipErrorInvalidValue before any launch.
 *
 * l3u_loc_select: rows[r] = (case_idx, z, y, x) of the ranks[r]-th voxel (0-based, C order) of
 * class cls, from the prefix l3u_loc_count wrote for the same label / body; a rank outside
 * [0, total) gives (case_idx, -1, -1, -1) and reads nothing out of range.  ranks: int64 device
 * memory; rows: int32 [R][4], 16-byte aligned; R >= 0 (R == 0: no launch, success).  Workspace is
 * the prefix alone: 8 bytes per L3U_LOC_BLOCK voxels. */
#define L3U_LOC_BLOCK 4096
int l3u_loc_nblocks(long long n);
int l3u_loc_count(const void* label, int label_dtype, const unsigned char* body, long long n,
                  unsigned int* prefix, hipStream_t stream);
int l3u_loc_select(const void* label, int label_dtype, const unsigned char* body, int D, int H,
                   int W, const unsigned int* prefix, int cls, const long long* ranks, int R,
                   int case_idx, int* rows, hipStream_t stream);

/* ---- resampling a case to another grid (csrc/resample.hip; light_unet/resample.py) ----
 * l3u_resample: dst[oD][oH][oW] from src[D][H][W] with the semantics of
 * scipy.ndimage.zoom(src, zoom, order = order, mode = "nearest", grid_mode = True): output index o
 * of an axis with n_in source and n_out output samples reads the source coordinate
 * c = (o + 0.5) * (n_in / n_out) - 0.5 (float64, not clamped).  The caller evaluates that, per
 * axis, into device tables of oD + oH + oW entries each (axis 0 first, then axis 1, then axis 2):
 *   order 0: lo[i] = clamp(floor(c + 0.5), 0, n_in - 1); hi and t are not read (may be NULL).
 *            dst[o] = src[lo], copied; dst_dtype == src_dtype, 0 float, 1 double or 2 uint8
 *            (l3u_pp_pack's codes).
 *   order 1: f = floor(c): lo[i] = clamp(f, 0, n_in - 1), hi[i] = clamp(f + 1, 0, n_in - 1),
 *            t[i] = c - f.  dst (dst_dtype 0, float) from src of dtype 0 or 1: the float64 sum over
 *            the 8 corners in C order (axis 0 the slowest bit, the low corner first) of
 *            (((double)src * w0) * w1) * w2, w = 1 - t at a low corner and t at a high one, every
 *            operation rounded on its own (no fused multiply-add), rounded once to float: scipy's
 *            own operation order, so the result is scipy's bit for bit.
 * With equal shapes every t is 0 and dst is src (rounded to float for a double source) bit for bit,
 * for finite values other than -0 (which comes back as +0).  Table indices outside the source are
 * clamped again on load: nothing outside src is read.  No atomics: the result is deterministic.
 * src != dst; any other dtype pairing or order returns hipErrorInvalidValue before any launch. */
int l3u_resample(const void* src, int src_dtype, int D, int H, int W, void* dst, int dst_dtype,
                 int oD, int oH, int oW, int order, const int* lo, const int* hi, const double* t,
                 hipStream_t stream);

/* ---- cubic B-spline resampling (csrc/spline.hip; light_unet/resample.py: resample_spline) ----
 * Order 3 of scipy.ndimage.zoom(src, zoom, order = 3, mode = "nearest", grid_mode = True), by this
 * definition (the project's own, not a transcription of scipy's C code: its float32 results equal
 * scipy 1.15.3's on tests/golden/spline.npz, the raw float64 sums agree to a few 1e-14 max|src|):
 *  1. Padding.  NP = 12.  The padded volume p[D + 24][H + 24][W + 24] is
 *     p[i0][i1][i2] = (double)src[clamp(i0 - 12)][clamp(i1 - 12)][clamp(i2 - 12)], each index
 *     clamped to its axis: np.pad(src, 12, mode = "edge").
 *  2. Prefilter.  Along axis 0, then axis 1, then axis 2, every line c[0 .. n-1] of the padded
 *     volume is filtered in place in float64, every product, sum and difference rounded on its own
 *     (no fused multiply-add, no reassociation, no scan), with the constants the caller computes
 *     once in double arithmetic and passes in: z = sqrt(3.0) - 2.0, lam = (1.0 - z) * (1.0 - 1.0 / z),
 *     k0 = 1.0 / (1.0 - z), kn = z / (z - 1.0):
 *         c[i] = c[i] * lam                  for all i
 *         c[0] = c[0] * k0
 *         c[i] = c[i] + z * c[i-1]           i = 1 .. n-1
 *         c[n-1] = kn * c[n-1]
 *         c[i] = z * (c[i+1] - c[i])         i = n-2 .. 0
 *     (the causal start is the closed form for a line extended by its first value; it differs from
 *     scipy's start only inside the outer pad, which no tap reads: the smallest tap index is 10).
 *  3. Tables.  Per axis with n_in source and n_out output samples and per output index o, in
 *     float64: cc = (o + 0.5) * (n_in / n_out) - 0.5, f = floor(cc), y = cc - f, u = 1.0 - y,
 *     start = (int)f - 1 + 12 (in [0, n_in + 20]), w0 = u*u*u/6.0, w1 = (y*y*(y-2.0)*3.0+4.0)/6.0,
 *     w2 = (u*u*(u-2.0)*3.0+4.0)/6.0, w3 = 1.0 - w0 - w1 - w2.  Device tables of oD + oH + oW
 *     entries, axis 0 first: start (int) and w (double [..][4]).
 *  4. Interpolation.  dst[o0][o1][o2] = (float) of the float64 sum, started at 0.0 and accumulated
 *     term by term over a, b, c in 0..3 in C order (a slowest), of
 *     ((coef[s0 + a][s1 + b][s2 + c] * w_axis0[a]) * w_axis1[b]) * w_axis2[c]; with use_clip != 0
 *     the float result becomes min(max(v, clip_lo), clip_hi) (a spline overshoots: a probability
 *     map can leave [0, 1]).
 * l3u_spline_prefilter: steps 1 and 2, src (src_dtype 0 float or 1 double) -> coef, a double
 * buffer of (D + 24) * (H + 24) * (W + 24) elements (0.9 GB for a 400 x 400 x 600 case); the
 * axis-0 pass reads src through the clamped indices, the other two run in place.  One prefilter
 * serves any number of output grids.  l3u_spline_prefilter_passes runs a subset (bit 0: the axis-0
 * pass src -> coef, bit 1: axis 1, bit 2: axis 2, on whatever coef holds; 7 is the prefilter), for
 * timing the passes apart.
 * l3u_resample_spline: step 4, coef of a [D][H][W] source -> dst[oD][oH][oW]; a start entry outside
 * [0, n_in + 20] is clamped again on load: nothing outside coef is read.
 * Every line's recursion and every output's sum runs in one thread in the stated order: no
 * atomics, and the result does not depend on the launch shape.  NULL or aliased pointers, another
 * src_dtype and sizes <= 0 return hipErrorInvalidValue before any launch. */
int l3u_spline_prefilter(const void* src, int src_dtype, int D, int H, int W, double* coef,
                         double z, double lam, double k0, double kn, hipStream_t stream);
int l3u_spline_prefilter_passes(const void* src, int src_dtype, int D, int H, int W, double* coef,
                                double z, double lam, double k0, double kn, int passes,
                                hipStream_t stream);
int l3u_resample_spline(const double* coef, int D, int H, int W, float* dst, int oD, int oH, int oW,
                        const int* start, const double* w, float clip_lo, float clip_hi,
                        int use_clip, hipStream_t stream);

/* ---- surface-distance metrics (csrc/surface.hip; light_unet/surface.py) ----
 * l3u_edt: the exact Euclidean distance transform of a packed feature mask (l3u_pp_pack's format,
 * bit 1 = feature voxel) with the spacings (sz, sy, sx) > 0: out[D][H][W] (double) holds
 *   sqrt(min over feature voxels f of fl(fl(((z-fz) sz)^2 + ((y-fy) sy)^2) + ((x-fx) sx)^2)),
 * every product and sum rounded to double once (nothing fused), summed in z, y, x order: the
 * arithmetic of scipy.ndimage.distance_transform_edt(~feat, sampling), whose map this is bit for
 * bit.  Without a feature voxel every output is +inf.  Three line passes (rounding is monotone, so
 * the float minimum separates): bit 0 of `passes` the z pass feat -> out, bit 1 the y pass
 * out -> tmp, bit 2 the x pass and the square root tmp -> out; passes = 7 is the transform, a
 * subset runs those passes alone on whatever the buffers hold (timing).  The y and x passes scan
 * outwards from each voxel and stop once the squared step alone reaches the best value; the scan is
 * bounded by the line length.  tmp: D * H * W doubles of workspace, out != tmp.
 * D * H * W < 2^31, else hipErrorInvalidValue before any launch.
 *
 * l3u_surf_mask: out = in & ~erode6(in) on packed masks (6-neighbour erosion, everything outside
 * the volume 0, so mask voxels on a volume face are surface): scipy's
 * in & ~binary_erosion(in, generate_binary_structure(3, 1)).  in != out.
 *
 * l3u_surf_reduce: over the voxels of the packed mask `surf`, of the distance map dist[D][H][W]:
 * res[11] (double) = their count, the maximum of dist (0 when there is none), the sum of dist, and
 * for q < ntol (0..8) the count of dist <= tol[q] at res[3 + q] (tol: HOST memory, read during the
 * call); sd[D][H][W] receives dist at surface voxels and +inf elsewhere, so that l3u_pp_select over
 * sd reads the order statistics of the surface distances at every rank below the count.  No float
 * atomics: part (l3u_surf_nblocks(D * H * W) * 12 doubles of workspace) takes one partial per 4096
 * voxels of the flat order, summed in a fixed order inside the workgroup, and one wave merges the
 * partials in a fixed order; the same input gives the same bits on every run.  dist != sd. */
int l3u_edt(const unsigned long long* feat, double sz, double sy, double sx, double* out,
            double* tmp, int D, int H, int W, int passes, hipStream_t stream);
int l3u_surf_mask(const unsigned long long* in, unsigned long long* out, int D, int H, int W,
                  hipStream_t stream);
int l3u_surf_nblocks(long long n);
int l3u_surf_reduce(const double* dist, const unsigned long long* surf, const double* tol, int ntol,
                    double* sd, double* part, double* res, int D, int H, int W, hipStream_t stream);

/* ---- lesion uptake (csrc/quantify.hip; light_unet/quantify.py) ----
 * All volumes are [D][H][W] with D * H * W < 2^31 (else hipErrorInvalidValue before any launch);
 * labels is l3u_ccl_label's int32 labelling (0 = background).  No float atomics anywhere: the same
 * input gives the same bits.  Uptake must be finite.
 *
 * l3u_qt_peak: the spherical mean around every labelled voxel c,
 *   peak[c] = S(c) / n(c),  S(c) = the double sum, from +0.0 and in table order, of
 *   uptake[c + offs[i]] over the offsets that stay inside the volume, n(c) their count,
 * the division in double.  offs: DEVICE int[noff][3] (dz, dy, dx), 1 <= noff <= 729, every
 * |dz| <= rz, |dy| <= ry, |dx| <= rx, and rz, ry, rx in 0..4 (the halo a workgroup stages; offsets
 * beyond it are clamped to it, never read outside the tile).  peak is written at labelled voxels
 * only; a 4 x 8 x 64 tile without one costs the read of its labels.
 *
 * l3u_qt_reduce: per label the voxel count, the double sum of uptake, the maximum of uptake with
 * the smallest flat index attaining it, and (peak != NULL) the same for peak.  items: DEVICE
 * int[n_items][8] = (label, z0, z1, y0, y1, x0, x1, 0), half-open boxes that partition each label's
 * voxels (clipped to the volume), the items of label l at first[l - 1] .. first[l] (DEVICE
 * int[num + 1], ascending).  One workgroup per item reduces in a fixed order into part
 * (n_items * 8 doubles of workspace); res[num][8] (double) = count, sum, max, its voxel, peak max,
 * its voxel, 0, 0, the items merged in item order (voxel = INT_MAX and max = -inf for a label without
 * voxels; the peak columns likewise when peak is NULL).
 *
 * l3u_qt_corners: out = the corner voxels of the packed mask `in` (l3u_pp_pack's format): mask
 * voxels that have, on each of the three axes, at least one of their two neighbours outside the
 * mask, the outside of the volume counting as outside.  Only they can be an end of the mask's
 * farthest pair.  bcnt[b] = the corner voxels in words [256 b, 256 b + 256) for
 * b < l3u_qt_corner_blocks(D, H, W) (0 for bad dimensions), bpre[b] = the sum of bcnt[0 .. b) and
 * bpre[blocks] = their total.  in != out, bcnt != bpre.
 * l3u_qt_compact: cand[k] = int[4] (z, y, x, flat index) of the k-th set voxel of `bits` in
 * ascending flat index, from l3u_qt_corners' bpre; writes below ncand only.
 *
 * l3u_qt_farthest: over the 2 <= ncand <= 2^18 candidates, res[3] (double) =
 *   the maximum over pairs of d2 = fl(fl(fl(dz sz)^2 + fl(dy sy)^2) + fl(dx sx)^2)
 * (dz, dy, dx the integer coordinate differences; nothing fused), then the flat indices i < j of
 * the pair attaining it with the smallest i, then the smallest j (cand ascending in flat index).
 * part: l3u_qt_pair_parts(ncand) * 2 unsigned long long of workspace (0 outside 2..2^18). */
int l3u_qt_peak(const float* uptake, const int* labels, const int* offs, int noff, int rz, int ry,
                int rx, double* peak, int D, int H, int W, hipStream_t stream);
int l3u_qt_reduce(const float* uptake, const int* labels, const double* peak, const int* items,
                  int n_items, const int* first, int num, double* part, double* res, int D, int H,
                  int W, hipStream_t stream);
int l3u_qt_corner_blocks(int D, int H, int W);
int l3u_qt_corners(const unsigned long long* in, unsigned long long* out, int* bcnt, int* bpre, int D,
                   int H, int W, hipStream_t stream);
int l3u_qt_compact(const unsigned long long* bits, const int* bpre, int* cand, int ncand, int D, int H,
                   int W, hipStream_t stream);
int l3u_qt_pair_parts(int ncand);
int l3u_qt_farthest(const int* cand, int ncand, double sz, double sy, double sx,
                    unsigned long long* part, double* res, hipStream_t stream);

/* ---- resegmentation by an uptake threshold (csrc/resegment.hip; light_unet/resegment.py) ----
 * Seeded region growing restricted to a box, one threshold per seed.  The seeds are the labels
 * 1..n of `seeds` (l3u_ccl_label's int32 labelling of a [D][H][W] volume, D * H * W < 2^31, else
 * hipErrorInvalidValue before any launch).  For seed i (label i + 1), with thr[i] a double:
 *   cand_i(v)  = (double)uptake[v] >= thr[i]  and, with a body mask, body[v] != 0
 *                (body_dtype 0 float, 2 uint8: l3u_pp_pack's codes; body may be NULL);
 *   box_i      = the half-open box of items[i], inside the volume;
 *   R_i        = the voxels v of box_i with cand_i(v) joined to a voxel of seed i with cand_i by a
 *                6-neighbour path whose voxels all lie in box_i and satisfy cand_i (connectivity
 *                through voxels outside the box does not count); with grow == 0 only the seed's
 *                own voxels with cand_i;
 *   own[v]     = max over {i : v in R_i} of (n - i), by integer atomicMax on a map the caller has
 *                ZEROED: n + 1 - own[v] is the smallest label reaching v, 0 stays "none";
 *   reached[i] += |R_i|  (the caller zeroes it).
 * Uptake must be finite.  All integer and bit work but that one comparison: the same input gives
 * the same bits; no float atomics.
 *
 * items: DEVICE int[n][8] = (label = i + 1, z0, z1, y0, y1, x0, x1, path), path =
 * l3u_rs_path(z1 - z0, y1 - y0, x1 - x0, max_lds_bytes): 0 when the box's two bitmaps (candidates
 * and reached: 64-bit words, x fastest from x0, rows padded to whole words, as l3u_pp_pack packs a
 * volume) and a 16-byte header fit max_lds_bytes of LDS (0: the default, 64 KiB, which is also the
 * most; 16 at least), 1 when they do not, -1 for bad arguments.  A row that is not consistent
 * (box outside the volume, another path than the budget allows) is skipped, never run.
 *
 * l3u_rs_grow: path 0 seeds are built, grown to the fixed point (sweeps of
 * reached |= cand & neighbours(reached) until one changes no word; sweeps[i] = the sweeps that
 * changed one) and committed to own / reached by one workgroup each.  For path 1 seeds it builds
 * the bitmaps in `arena`: seed i holds 3 nw_i words from aoff[i] (DEVICE long long[n]; nw_i = rows
 * x words per row): candidates, then two reached buffers, the seed in the first.  tiles: DEVICE
 * int[n_tiles][4] = (i, z, y, word) origins, relative to the box, of the 8 x 8 x 4-word tiles that
 * partition the path 1 boxes (l3u_rs_tiles(nz, ny, nx) of them per box); n_tiles may be 0.
 * l3u_rs_sweep: one launch grows every tile, staged with a halo of one plane, row and word, to its
 * own fixed point from reached buffer 1 + flip (flip 0 or 1) into buffer 2 - flip, and adds the
 * number of interior words it changed to *counter (DEVICE): relaunch with flip alternating until a
 * launch adds 0.
 * l3u_rs_commit: reached buffer 1 + flip of the path 1 seeds into own / reached. */
int l3u_rs_path(int nz, int ny, int nx, int max_lds_bytes);
int l3u_rs_tiles(int nz, int ny, int nx);
int l3u_rs_grow(const float* uptake, const int* seeds, const void* body, int body_dtype,
                const int* items, const double* thr, int n, int grow, int* own,
                unsigned long long* reached, int* sweeps, const int* tiles, int n_tiles,
                const long long* aoff, unsigned long long* arena, int max_lds_bytes, int D, int H,
                int W, hipStream_t stream);
int l3u_rs_sweep(const int* items, int n, const int* tiles, int n_tiles, const long long* aoff,
                 unsigned long long* arena, int flip, unsigned int* counter, int D, int H, int W,
                 hipStream_t stream);
int l3u_rs_commit(const int* items, int n, const int* tiles, int n_tiles, const long long* aoff,
                  const unsigned long long* arena, int flip, int* own, unsigned long long* reached,
                  int D, int H, int W, hipStream_t stream);

/* ---- Gaussian smoothing (csrc/smooth.hip; light_unet/smooth.py) ----
 * scipy.ndimage.gaussian_filter(src, sigma, mode = mode, cval = cval) of a [D][H][W] float or
 * double volume, by this definition (the project's own; its results equal scipy 1.15.3's bit for
 * bit on tests/golden/smooth.npz).  For each axis a = 0, 1, 2 in that order with sigma[a] > 1e-15
 * (another axis is skipped, not run with a unit kernel):
 *  1. Weights, on the host in float64 (numpy): r = (int)(truncate * sigma + 0.5), or a given
 *     radius; x = -r .. r; phi = exp(-0.5 / (sigma * sigma) * x^2); w = phi / sum(phi), w[0 .. 2r],
 *     symmetric bit for bit.  The caller uploads w as a device table.
 *  2. Line pass along a over the current array, every operation in float64 and rounded on its own
 *     (no product fused with a sum), with v[k] the array along the line and n its length:
 *         t = v[i] * w[r]
 *         t = t + (v[i + j] + v[i - j]) * w[j + r]      for j = -r, -r + 1, .., -1 in that order
 *     (the symmetric branch of scipy's correlate1d, the outermost pair added first); t is rounded
 *     to the array's type (float or double) and stored; the next axis reads the rounded values.
 *  3. A tap v[k] outside 0 .. n-1, by mode:
 *         0 reflect   m = k mod 2n (in 0 .. 2n-1), then 2n - 1 - m where m >= n
 *         1 mirror    m = k mod (2n - 2), then 2n - 2 - m where m >= n; n == 1 reads voxel 0
 *         2 nearest   k clamped to 0 .. n-1
 *         3 constant  the value cval, as a double
 *     The map is a closed form of k: r may exceed n many times over.
 * Inputs must be finite.
 * l3u_gauss_axis: step 2 along `axis` (0, 1 or 2), src -> dst, both of dtype 0 (float) or 1
 * (double) (l3u_pp_pack's codes); w: DEVICE double[2 * radius + 1] (entries 0 .. radius are read);
 * 0 <= radius <= l3u_gauss_max_radius() = 64, the halo a workgroup stages.  src and dst must not
 * overlap: the taps of a line are read after its first outputs are stored.  NULL or overlapping
 * buffers, another dtype, axis or mode, a radius outside the range and sizes <= 0 return
 * hipErrorInvalidValue before any launch.  Each output's sum runs in one thread in the stated
 * order: no atomics, and the result does not depend on the launch shape. */
int l3u_gauss_max_radius(void);
int l3u_gauss_axis(const void* src, void* dst, int dtype, int D, int H, int W, int axis,
                   const double* w, int radius, int mode, double cval, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* L3U_H */
