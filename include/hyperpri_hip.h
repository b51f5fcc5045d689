/* hyperpri_hip.h -- C ABI of libhyperpri_hip.so (MI355X / gfx950 only).
 *
 * The reference (GatorSense/HyperPRI) has no FFI: its hot path is plain torch.nn modules
 * (src/Experiments/model_parts.py, src/Experiments/models.py) whose arithmetic lives in ATen/cuDNN.
 * This library is what a maintainer would bind in their place: one launcher per kernel family and
 * direction, plain pointers and sizes, no torch types.  hyperpri_amd/_lib.py holds the ctypes binding;
 * INTEGRATION.md shows the reference-side shim.
 *
 * Conventions
 *   - Activations are fp32 NHWC.  A tensor view is (pointer, cs, coff): element (pixel p, channel c)
 *     lives at ptr[p*cs + coff + c]; cs and coff are multiples of 4 (16-byte channel vectors) and the
 *     pointer is 16-byte aligned.  Views into a wider buffer are how skip-concat (model_parts.py:87)
 *     costs no copy on the consumer side.
 *   - Every buffer, including workspaces, is owned by the caller (PyTorch caching allocator); the
 *     library never allocates, frees or synchronises.  All launches go to the given hipStream_t.
 *   - Return value: 0 = ok, <0 = error (HPRI_ERR_*); hpri_last_error() returns the thread's message.
 *     Nothing throws across the ABI.
 *   - Launchers are re-entrant (autograd calls them from worker threads).  The only process-wide state is immutable after
 *     its first use or atomic: the launch-plan options (read once from the environment under std::call_once, then
 *     atomics; hpri_set_option) and a per-device cache of the compute-unit count; the error message is thread-local.  Stamp
 *     buffers exist in the diagnostic builds (-DHPRI_STAMPS) only.
 */
#ifndef HYPERPRI_HIP_H
#define HYPERPRI_HIP_H

#include <stddef.h>
#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HPRI_OK 0
#define HPRI_ERR_ARG (-1)
#define HPRI_ERR_UNSUPPORTED (-2)
#define HPRI_ERR_WORKSPACE (-3)
#define HPRI_ERR_LAUNCH (-4)

#define HPRI_A_DIRECT 0 /* A operand read in place                                   */
#define HPRI_A_S2D 1    /* A operand gathered as 2x2 stride-2 patches (convT grads)  */
#define HPRI_E_DIRECT 0 /* NHWC store                                                */
#define HPRI_E_D2S 1    /* 2x2 stride-2 pixel-shuffle store (convT forward)          */

int hpri_version(void);
/* Launch-plan options (process-wide): "conv_nbx_min", "wgrad_xcd_min_tiles", "wgrad_xcd_min_strips", "bf16v3_tile_width", "bn_wide_cq" -- the problem sizes
 * from which the conv / weight-gradient kernels switch to their XCD-aware 1-D grids -- and "wgrad_cu_reserve": compute
 * units the fp32 Winograd weight gradient (one workgroup per CU, grids planned as exact multiples of the CU count) leaves to other
 * kernels, e.g. the channels of a collective that runs beside the backward (0 = none).  Results do not depend
 * on them, only block order and (for weight gradients) the number of partial slabs, i.e. the summation order.
 * "wgrad_skip_edge" (default 1): the fp32 Winograd weight gradient leaves out the MFMA k-steps whose four pixel columns all lie
 * right of the image edge, where dY is zero-filled; 0 runs every k-step of every strip.  Bit-identical results for finite
 * activations (a non-finite activation in the column beyond the edge-most valid one gives NaN only with 0).
 * "wino4_fast_epilogue" (default 1): workgroups of hpri_conv_wino4 / hpri_conv_wino4_bnred whose 16 x 8 pixels lie inside the image
 * and whose 64 channels are all written take, in launches without ReLU and accumulate, an epilogue without per-element selects; 0
 * sends every workgroup through the general epilogue.  Bit-identical results. */
int hpri_set_option(const char* name, int value);
/* A non-blocking stream of the lowest priority the current device offers (*priority receives it); the caller owns it. */


int hpri_get_option(const char* name);
const char* hpri_last_error(void);

/* ---- item queues of the persistent MFMA kernels (hpri_conv_bf16v3*, hpri_gemm_bf16v3 / hpri_convt_*_bf16*, hpri_gemm_f32v2 /
 * hpri_convt_*_f32v2) ----------------------------------------------------------------------------------------------------------
 * These launches start 2 x CUs workgroups, two per CU.  Without a queue every workgroup walks a fixed list of work items; a
 * workgroup that cannot become resident at once (another kernel -- an RCCL collective beside the backward of a DDP step,
 * PLTrainer.py:434-442 -- holds part of its CU) then runs its whole list late: one such workgroup costs a bf16 step 6-15 %.
 * hpri_set_item_queue(queue, bytes, stream) gives every later persistent launch ON THAT STREAM `queue` -- hpri_item_queue_bytes()
 * bytes of device memory, 256-byte aligned, zeroed once by the caller, owned by the caller and alive while it may launch -- as its
 * item counters: workgroups draw their items (same items, same per-XCD order, results bit-identical) and a late workgroup finds
 * nothing left.  The buffer holds two halves; launches on the stream alternate between them and each launch zeroes the half the
 * next one will use (the library keeps the parity per registered stream).  One queue per stream (launches of one stream run one
 * after the other; the null stream of one device per process); queue == NULL unregisters the stream. */
int hpri_item_queue_bytes(void);
/* ---- the half-precision build (libhyperpri_hip_f16.so: the same entry points with IEEE half as the 16-bit type of every "bf16" plane,
 * row and packed-weight argument; precision mode "f16" of hyperpri_amd) needs a loss scale: hpri_set_loss_scale(s) makes the fused
 * heads of the CALLING THREAD (hpri_outconv_bwd_bce, hpri_outconv_bwd_x16 with a target) form s times the loss gradient -- s a power
 * of two chosen by the caller from the number of logits, so that activation gradients sit in half's range -- and
 * hpri_scale_tensors(tensors, numel, n, 1 / s) takes it out of the parameter gradients afterwards.  In libhyperpri_hip.so (bf16:
 * eight exponent bits) both exist and the scale stays 1. */
int hpri_set_loss_scale(float scale);
int hpri_scale_tensors(float* const* tensors, const long long* numel, int ntensors, float scale, hipStream_t stream);
/* The scale of the non-fused heads is picked on the device from the gradient that arrives at the logits (a GradScaler-scaled or
 * sum-reduced loss brings one far above 1 / #logits): hpri_loss_scale_pick(gy, n, static, slot) writes
 * s = min(static, 2^floor(log2(2 / max|gy[0..n)|))) -- static when that maximum is 0 or not finite -- to slot[0] and 1 / s to slot[1];
 * slot is device memory of hpri_loss_scale_slot_floats() floats (the rest holds block maxima), no host synchronisation.
 * hpri_scale_tensors_dev is hpri_scale_tensors with the factor read from slot[0] (invert != 0: slot[1]);
 * hpri_unscale_accumulate: dst[k][i] += src[k][i] * slot[1] (a micro-batch's loss-scaled gradient added, unscaled, to the sum). */
int hpri_loss_scale_slot_floats(void);
int hpri_loss_scale_pick(const float* gy, long long n, float stat, float* slot, hipStream_t stream);
int hpri_scale_tensors_dev(float* const* tensors, const long long* numel, int ntensors, const float* slot, int invert, hipStream_t stream);
int hpri_unscale_accumulate(float* const* dst, const float* const* src, const long long* numel, int ntensors, const float* slot,
                            hipStream_t stream);
int hpri_set_item_queue(void* queue, size_t bytes, hipStream_t stream);

/* ---- weight packing: nn.Parameter layouts -> [chunk][tap][32][Ncols_pad] LDS panels ---------------
 * mode 0 conv fwd   (replaces cuDNN's filter transform for nn.Conv2d, model_parts.py:22,25,96; nn.Conv3d
 *                    models.py:169; nn.Linear models.py:108,103)
 * mode 1 conv dgrad (autograd of the same), mode 2 convT fwd (model_parts.py:63; models.py:198),
 * mode 3 convT dgrad.  K = reduction length per tap, Ncols = GEMM columns, src_d1 = dim 1 of the
 * source tensor. */
size_t hpri_packed_weight_floats(int K, int Ncols_pad, int T);
int hpri_pack_weight(const float* w, float* wp, int mode, int K, int Ncols, int Ncols_pad, int T, int Cup,
                     int src_d0, int src_d1, hipStream_t stream);

/* eval-mode conv->BN->ReLU folded into one conv (predict / validate / test paths, PLTrainer.py:142-162, 530-532):
 * hpri_bn_fold gives scale = gamma/sqrt(var+eps) and the folded bias; hpri_pack_weight_scaled packs w*scale; bit 1 of
 * hpri_conv_fwd's `accumulate` argument (value 2) turns on the ReLU epilogue. */
int hpri_bn_fold(const float* running_mean, const float* running_var, const float* gamma, const float* beta,
                 const float* conv_bias, float eps, int C, float* scale, float* fbias, hipStream_t stream);
int hpri_pack_weight_scaled(const float* w, float* wp, const float* colscale, int K, int Ncols, int Ncols_pad, int T,
                            int src_d1, hipStream_t stream);
/* the same fold for the bf16 / bf16x3 / bf16x6 modes (scale applied in fp32, then rounded / split into planes) */
int hpri_pack_weight_bf16_scaled(const float* w, void* wp, const float* colscale, int K, int Ncols, int Ncols_pad, int T,
                                 int src_d1, int split, hipStream_t stream);

/* 64-bit content fingerprint of n_words 32-bit words (order-independent integer sum; `out` is zeroed by the call, on the
 * stream).  Used by the verify mode of the packed-weight cache (hyperpri_amd/engine.py: HPRI_PACK_VERIFY=1), which catches
 * parameters rewritten through `p.data` -- writes the nn.Parameter version counter (the cache key that stands in for
 * model_parts.py:22's weight tensor) does not see. */
int hpri_fingerprint(const void* w, long long n_words, unsigned long long* out, hipStream_t stream);

/* ---- implicit-GEMM convolution, fp32 MFMA (conv_fwd.hip) ----------------------------------------
 * Replaces F.conv2d / F.conv3d / F.linear / F.conv_transpose2d forward and their data gradients
 * (model_parts.py:22,25,63,96; models.py:108,169,177,198).  hpri_conv_fwd_plan (host only) returns the split-K
 * factor chosen for the shape, the workspace it needs, and the number of BatchNorm partial records: stats
 * (optional) receives stat_tiles * Cout_pad float4 (mean, M2, count, 0), image-major.  y_cw (Cout <= y_cw <= Cout_pad) channels of
 * the output view are written, [Cout, y_cw) as zeros; `accumulate` bit 1: ReLU of result + bias, bit 0: y += that, in this order. */
int hpri_conv_fwd_plan(int N, int H, int W, int Cin_pad, int Cout_pad, int KS, int amode, int epi, int* ksplit,
                       int* stat_tiles, size_t* ws_floats);
int hpri_conv_fwd(const float* x, int x_cs, int x_coff, const float* wp, const float* bias, float* y, int y_cs,
                  int y_coff, float* stats, int N, int H, int W, int Cin_pad, int Cout, int Cout_pad, int y_cw,
                  int KS, int amode, int epi, int accumulate, int H2, int W2, int py0, int px0, int Cup, float* ws,
                  size_t ws_floats, hipStream_t stream);

/* ---- Winograd F(2x2,3x3), exact fp32 MFMA (conv_wino4.hip) --------------------------------------------------------
 * 3x3 / pad 1 / stride 1 convolutions (model_parts.py:22,25; models.py:169,177), forward and data gradient, with 16 instead
 * of 36 multiplies per 2x2 outputs: 4-wave workgroups of 16 x 8 pixels, two per CU, wave = frequency row.  hpri_wino4_pack
 * transforms the filters (U = G g G^T; mode 0 forward, mode 1 data gradient, optional per-column scale for the eval-mode BN
 * fold) into [K/8][16][Ncols_pad][8] (hpri_wino_packed_floats floats); hpri_conv_wino4_plan gives the number of BatchNorm partial
 * records (one per 16 x 8-pixel tile); `accumulate` bit 0: y += result, bit 1: ReLU.  x: fp32 NHWC view with channels
 * [Cin, Cin_pad) zero (Cin_pad a multiple of 8).  (conv_wino.hip holds the weight gradient of the same transform, below.) */
size_t hpri_wino_packed_floats(int K, int Ncols_pad);
int hpri_wino4_pack(const float* w, float* up, const float* colscale, int mode, int K, int Ncols, int Ncols_pad, int src_d1,
                    hipStream_t stream);
int hpri_conv_wino4_plan(int N, int H, int W, int* stat_tiles);
int hpri_conv_wino4(const float* x, int x_cs, int x_coff, const float* up, const float* bias, float* y, int y_cs, int y_coff,
                    float* stats, int N, int H, int W, int Cin_pad, int Cout, int Cout_pad, int y_cw, int accumulate,
                    hipStream_t stream);

/* hpri_conv_wino4 as a DATA GRADIENT (mode-1 pack, no bias, no accumulate) that also leaves the BatchNorm-backward partial sums of the
 * conv -> BN -> ReLU stage whose output gradient y it writes (model_parts.py:22-27's autograd): bn_x = that stage's pre-BN tensor
 * (fp32 NHWC view, same pixels / channels as y, Cout_pad channels wide), its per-channel mean / invstd / scale / shift, bn_relu;
 * bn_part[N * tiles][2][bn_cpart] (tiles: hpri_conv_wino4_plan) receives sum g*[y>0] and sum g*[y>0]*xhat per tile.  Finish with
 * hpri_bn_relu_bwd_fused, which then skips its two reduction sweeps over g and the pre-BN tensor. */
int hpri_conv_wino4_bnred(const float* x, int x_cs, int x_coff, const float* up, float* y, int y_cs, int y_coff, int N, int H,
                          int W, int Cin_pad, int Cout, int Cout_pad, int y_cw, const float* bn_x, int bn_x_cs, int bn_x_coff,
                          const float* bn_mean, const float* bn_invstd, const float* bn_scale, const float* bn_shift,
                          int bn_relu, float* bn_part, int bn_cpart, hipStream_t stream);
int hpri_bn_relu_bwd_fused(const float* partials, int part_blocks, int part_cpart, const float* dy, int dy_cs, int dy_coff,
                           const float* x, int x_cs, int x_coff, float* dx, int dx_cs, int dx_coff, const float* mean,
                           const float* invstd, const float* scale, const float* shift, float* dgamma, float* dbeta,
                           int accumulate_param_grads, float* dbias, int accumulate_dbias, float* workspace, size_t ws_floats,
                           long long P, long long pix_per_group, int C, int Cw, int relu, int use_batch_stats, void* planes,
                           long long plane_stride, int pl_cs, int pl_coff, int pl_cw, int npl, hipStream_t stream);


/* Winograd weight gradient (dU = sum over tiles of V * (A dY A^T), dg = G^T dU G): slabs ws[split][16][Cr][Nr] from
 * hpri_conv_wino_wgrad (sizes: hpri_wino_wgrad_plan), fixed-order sum + inverse filter transform into OIHW by
 * hpri_wino_wgrad_reduce. */
int hpri_wino_wgrad_plan(int N, int H, int W, int Cin_pad, int Cout_pad, int* splits, int* Cr, int* Nr);
int hpri_conv_wino_wgrad(const float* x, int x_cs, int x_coff, int x_cvalid, const float* dy, int dy_cs, int dy_coff,
                         int dy_cvalid, float* ws, size_t ws_floats, int N, int H, int W, int Cin_pad, int Cout_pad,
                         hipStream_t stream);
int hpri_wino_wgrad_reduce(const float* ws, float* dw, int N, int H, int W, int Cin, int Cin_pad, int Cout, int Cout_pad,
                           int accumulate, hipStream_t stream);

/* bf16-operand variants (precision mode "bf16", BASELINE.json config C5): operands rounded to bf16 while staged into
 * LDS, v_mfma_f32_32x32x16_bf16 with fp32 accumulate, fp32 activations in HBM.  Same modes, plan, workspace and
 * statistics contract as hpri_conv_fwd / hpri_pack_weight (plan: hpri_conv_fwd_bf16_plan).  split = 1 (precision mode
 * "bf16x3"): operands carried as bf16 hi + bf16 lo (16 mantissa bits), three MFMAs per product (hi*hi + hi*lo + lo*hi);
 * split = 2 ("bf16x6"): hi + mid + lo = the fp32 operand exactly, six MFMAs per product (fp32-class accuracy); the
 * packed weights hold split + 1 planes. */
int hpri_conv_fwd_bf16_plan(int N, int H, int W, int Cin_pad, int Cout_pad, int KS, int amode, int epi, int split,
                            int* ksplit, int* stat_tiles, size_t* ws_floats);
int hpri_pack_weight_bf16(const float* w, void* wp, int mode, int K, int Ncols, int Ncols_pad, int T, int src_d1,
                          int Cup, int split, hipStream_t stream);
/* The same for a layer whose INPUT-channel axis carries gap_len structural-zero channels from gap_at on (the padded concat of the
 * bf16 plane mode: [a | zeros up to a multiple of 32 | b]); modes 0 / 1; K (mode 0) resp. Ncols (mode 1) is the padded width, src_d1
 * the weight's own. */
int hpri_pack_weight_bf16_gap(const float* w, void* wp, int mode, int K, int Ncols, int Ncols_pad, int T, int src_d1, int gap_at,
                              int gap_len, hipStream_t stream);
int hpri_conv_fwd_bf16(const float* x, int x_cs, int x_coff, const void* wp, const float* bias, float* y, int y_cs,
                       int y_coff, float* stats, int N, int H, int W, int Cin_pad, int Cout, int Cout_pad, int y_cw,
                       int KS, int amode, int epi, int accumulate, int H2, int W2, int py0, int px0, int Cup, int split,
                       float* ws, size_t ws_floats, hipStream_t stream);
/* ConvTranspose2d(k2,s2) forward (model_parts.py:63-64) in the plain bf16 mode, result as ONE bf16 plane: channels [pl_coff,
 * pl_coff + Cup) of a plane buffer with pl_cs elements per hi-res pixel (the decoder's concat planes); also fp32 when y != NULL. */
int hpri_convt_fwd_bf16_pl(const float* x, int x_cs, int x_coff, const void* wp, const float* bias, float* y, int y_cs,
                           int y_coff, int N, int H, int W, int Cin_pad, int Cout, int Cout_pad, int H2, int W2, int py0, int px0,
                           int Cup, void* planes, int pl_cs, int pl_coff, hipStream_t stream);

/* bf16 activation PLANES: in the bf16 modes the producer of an activation writes it as bf16 NHWC
 * planes (plane 0 = bf16(x), plane 1 = bf16(x - hi), ...; `plane_stride` elements apart, `cs16` elements per pixel,
 * channels [C, cw16) zero), so the 3x3 convolution (model_parts.py:22,25; models.py:169,177; forward, or data gradient
 * with the mode-1 pack) brings BOTH operands into LDS by LDS-DMA.  hpri_to_planes is the generic producer (fp32 NHWC
 * view -> planes); plan / workspace / statistics contract as hpri_conv_fwd (split-K finish: hpri_splitk_finish). */
int hpri_to_planes(const float* x, int cs, int coff, void* planes, long long plane_stride, int cs16, int coff16,
                   long long P, int C, int cw16, int npl, hipStream_t stream);


int hpri_splitk_finish(const float* ws, int ksplit, int Cout_pad, const float* bias, float* y, int y_cs, int y_coff,
                       float* stats, int N, int HW, int Cout, int y_cw, int accumulate, int relu, hipStream_t stream);
/* First-layer fused ingest (conv_ingest.hip; predict path of the 16-bit modes).  Replaces, for nn.Conv3d(1, F, (D,3,3), padding=(0,1,1)) on
 * the caller's (N,1,D,H,W) cube -- reference models.py:169 (first_conv) as called at models.py:215-216 -- the pair layout pass
 * (hpri_nchw_to_nhwc_pl) + hpri_conv_bf16v3: the 3x3 pad-1 convolution reads the contiguous fp32 NC(D)HW tensor `x` itself (C = D
 * channels) and rounds it to the library's 16-bit type while staging.  `wp`: weights packed by hpri_pack_weight_bf16(_scaled)
 * ([chunk][tap][Cout_pad][32], channels beyond C zero; eval-mode BatchNorm folded in by the caller: hpri_bn_fold), `bias` (may be
 * null), `relu`; result as 16-bit rows y + pixel * y_cs + y_coff + channel (Cout a multiple of 4, y 8-byte aligned, y_cs / y_coff
 * multiples of 4) = the planes the next convolution stages.  One image of x must stay below 2 GiB.  Same accumulation order as
 * hpri_conv_bf16v3: bit-identical to the pair it replaces. */
int hpri_conv3x3_ingest_h16(const float* x, const void* wp, const float* bias, void* y, int y_cs, int y_coff, int N, int C, int H,
                            int W, int Cout, int Cout_pad, int relu, hipStream_t stream);
/* Third form of the plane convolution (conv_bf16v3.hip): 4-wave workgroups of 256 pixels x 64 channels, TWO per CU (one's
 * prologue / store + statistics epilogue runs under the other's MFMAs), v_mfma_f32_16x16x32_bf16 with the weights as the A
 * operand (a lane's accumulator registers are consecutive channels of one pixel: 16-byte stores without an LDS transpose).
 * x_plane is unused (one plane); `split` must be 0; `accumulate` bit 0: y += result, bit 1: ReLU; plan / workspace / statistics
 * contract as hpri_conv_fwd (records per 256-pixel tile: hpri_conv_bf16v3_plan); the output view must be float4-aligned.  Bit 2 of `accumulate` (value 4): the output view is bf16 (y points at bf16 elements,
 * y_cs / y_coff in elements; not with bit 0, not for split-K problems) -- the pre-BN tensor at 2 bytes per element, read by
 * hpri_bn_apply_relu_x16 / hpri_bn_relu_bwd_x16.  (Stamp builds, -DHPRI_STAMPS by tools/build_v3_diag.sh, add an undeclared
 * hpri_conv_bf16v3_dbg with a caller-given stagger and stamp buffer; the product libraries do not export it.) */
int hpri_conv_bf16v3_plan(int N, int H, int W, int Cin_pad, int Cout_pad, int* ksplit, int* stat_tiles,
                          size_t* ws_floats);
int hpri_conv_bf16v3(const void* xp, long long x_plane, int x_cs, int x_coff, const void* wp, const float* bias, float* y,
                     int y_cs, int y_coff, float* stats, int N, int H, int W, int Cin_pad, int Cout, int Cout_pad, int y_cw,
                     int accumulate, int split, float* ws, size_t ws_floats, hipStream_t stream);


/* hpri_conv_bf16v3 (no accumulate; hpri_conv_bf16v3_plan must report ksplit 1) whose result channels [y2_c0, y2_c0 + y2_cw) -- whole
 * 64-channel blocks -- are also (y2_only bit 0: only) written as bf16 rows, y2 + pixel * y2_cs + y2_coff + (channel - y2_c0): the
 * gradient of the upsampled half of a decoder concat for the plane-fed transposed-convolution kernels.  y2_only bit 1 (round 4): the
 * main output y holds bf16 rows as well (y_cs / y_coff in elements) -- the gradient of a planes-only skip tensor. */
int hpri_conv_bf16v3_y2(const void* xp, int x_cs, int x_coff, const void* wp, const float* bias, float* y, int y_cs, int y_coff,
                        float* stats, int N, int H, int W, int Cin_pad, int Cout, int Cout_pad, int y_cw, void* y2, int y2_cs,
                        int y2_coff, int y2_c0, int y2_cw, int y2_only, hipStream_t stream);


/* ---- fp32 GEMM for the 1x1 forms of the exact-fp32 mode, second form (gemm_f32v2.hip, round 4): ConvTranspose2d(k=2,s=2) forward and
 * data gradient (model_parts.py:63-64; models.py:198) and the plain row GEMM, on v_mfma_f32_32x32x2_f32 with both operands by LDS-DMA,
 * two persistent 4-wave workgroups of 256 pixels x 128 columns per CU.  hpri_pack_weight_f32k16 packs [chunk of 16 k][Ncols_pad][16]
 * (modes as hpri_pack_weight: 0 Linear forward W[n][k], 1 its data gradient, 2 ConvTranspose2d forward (column = tap*Cup + co), 3 its
 * data gradient (k = tap*Cup + co); src_d1 = dim 1 of the source tensor for modes 0 / 1).  x rows: x_cs floats apart (multiple of 4),
 * K_pad (multiple of 16) of them read from x_coff on; pad channels must hold zeros or meet zero weights.  `accumulate` bit 0: y +=
 * result (not for the depth-to-space form).  No statistics epilogue: layers in front of a BatchNorm keep hpri_conv_fwd. */
size_t hpri_packed_weight_f32k16_floats(int K, int Ncols_pad);
int hpri_pack_weight_f32k16(const float* w, float* wp, int mode, int K, int Ncols, int Ncols_pad, int Cup, int src_d1,
                            hipStream_t stream);
int hpri_gemm_f32v2(const float* x, int x_cs, int x_coff, const float* wp, const float* bias, float* y, int y_cs, int y_coff,
                    int N, long long HW, int K_pad, int Ncols, int Ncols_pad, int y_cw, int accumulate, hipStream_t stream);
int hpri_convt_fwd_f32v2(const float* x, int x_cs, int x_coff, const float* wp, const float* bias, float* y, int y_cs,
                         int y_coff, int N, int H, int W, int K_pad, int Cup, int Ncols_pad, int H2, int W2, int py0, int px0,
                         hipStream_t stream);
int hpri_convt_dgrad_f32v2(const float* dy, int dy_cs, int dy_coff, const float* wp, float* dx, int dx_cs, int dx_coff, int N,
                           int H, int W, int Cup, int Cin, int Cin_pad, int dx_cw, int H2, int W2, int py0, int px0,
                           int accumulate, hipStream_t stream);

/* ---- plane-fed GEMM for the 1x1 forms of the bf16 mode (gemm_bf16v3.hip): nn.Linear / Conv2d(k=1) forward and data gradient
 * (models.py:105-115,143; model_parts.py:96) and ConvTranspose2d(k=2,s=2) forward / data gradient (model_parts.py:63-64).
 * hpri_gemm_bf16v3: y[p, n] (+)= sum_k x[p, k] w[n, k] + bias[n]; x = bf16 planes of N*HW rows (x_cs elements per row, K_pad read
 * from x_coff on), w = hpri_pack_weight_bf16 with T = 1 (modes 0 / 1); outputs fp32 view y and / or bf16 view y16 (either may be
 * NULL), y_cw columns written (a multiple of 4 in [Ncols, Ncols_pad]); accumulate bit 0: add to y, bit 1: ReLU; stats: one record row of stat_cp columns per 256-row tile
 * (hpri_gemm_bf16v3_plan; tiles never straddle images) for hpri_bn_finalize.
 * hpri_convt_fwd_bf16v3: column tap*Cup + co (pack mode 2) -> pixel (py0 + 2y + tap/2, px0 + 2x + tap%2), channel co of the
 * [N, H2, W2] views; Cup % 16 == 0.  hpri_convt_dgrad_bf16v3: dx (+)= gather over the four parities of the dy planes (pack mode 3,
 * K = 4*Cup); Cup % 32 == 0. */
int hpri_gemm_bf16v3_plan(int N, long long HW, int* stat_tiles);
int hpri_gemm_bf16v3(const void* xp, int x_cs, int x_coff, const void* wp, const float* bias, float* y, int y_cs, int y_coff,
                     void* y16, int y16_cs, int y16_coff, float* stats, int stat_cp, int N, long long HW, int K_pad, int Ncols,
                     int Ncols_pad, int y_cw, int accumulate, hipStream_t stream);
int hpri_convt_fwd_bf16v3(const void* xp, int x_cs, int x_coff, const void* wp, const float* bias, float* y, int y_cs, int y_coff,
                          void* y16, int y16_cs, int y16_coff, int N, int H, int W, int K_pad, int Cup, int Ncols_pad, int H2,
                          int W2, int py0, int px0, hipStream_t stream);
int hpri_convt_dgrad_bf16v3(const void* dyp, int dy_cs, int dy_coff, const void* wp, float* dx, int dx_cs, int dx_coff, int N,
                            int H, int W, int Cup, int Cin, int Cin_pad, int dx_cw, int H2, int W2, int py0, int px0,
                            int accumulate, hipStream_t stream);
/* ... the same written as bf16 rows (round 4; no accumulate): a decoder stage's input has one reader of its gradient. */
int hpri_convt_dgrad_bf16v3_y16(const void* dyp, int dy_cs, int dy_coff, const void* wp, void* dx16, int dx_cs, int dx_coff, int N,
                                int H, int W, int Cup, int Cin, int Cin_pad, int dx_cw, int H2, int W2, int py0, int px0,
                                hipStream_t stream);

/* ---- weight gradients, fp32 MFMA, deterministic split-K (conv_wgrad.hip) --------------------------
 * Replaces the wgrad half of autograd for the same layers.  dst_mode 0 writes OIHW / (out,in),
 * dst_mode 1 writes ConvTranspose2d's (Cin,Cout,2,2).  Workspace: splits*KS*KS*Cr*Nr floats. */
int hpri_wgrad_plan(int N, int H, int W, int Cin_pad, int Cout_pad, int KS, int* splits, int* Cr, int* Nr);
int hpri_conv_wgrad(const float* x, int x_cs, int x_coff, int x_cvalid, const float* dy, int dy_cs, int dy_coff,
                    int dy_cvalid, float* ws, size_t ws_floats, int N, int H, int W, int Cin_pad, int Cout_pad, int KS,
                    int bmode, int H2, int W2, int py0, int px0, int Cup, hipStream_t stream);
int hpri_conv_wgrad_bf16(const float* x, int x_cs, int x_coff, int x_cvalid, const float* dy, int dy_cs, int dy_coff,
                         int dy_cvalid, float* ws, size_t ws_floats, int N, int H, int W, int Cin_pad, int Cout_pad,
                         int KS, int bmode, int H2, int W2, int py0, int px0, int Cup, int split, hipStream_t stream);
int hpri_wgrad_reduce(const float* ws, float* dw, int N, int H, int W, int Cin, int Cin_pad, int Cout, int Cout_pad,
                      int KS, int dst_mode, int Cup, int accumulate, hipStream_t stream);
/* The same fixed-order reduction for slabs whose pixel splits the caller planned itself (hpri_wgrad_bf16v2_plan). */
int hpri_wgrad_reduce_ex(const float* ws, float* dw, int splits, int Cr, int Nr, int Cin, int Cout, int KS, int dst_mode,
                         int Cup, int accumulate, hipStream_t stream);
/* Weight gradient of the 3x3 / pad 1 convolutions from bf16 PLANES (conv_wgrad_bf16v2.hip; precision mode "bf16"; the
 * autograd of model_parts.py:22,25 and models.py:169,177): plane 0 of the conv input and of the output gradient (NHWC,
 * strides / offsets / valid widths multiples of 8 elements), both by LDS-DMA; slabs ws[splits][9][Nr][Cr] (sizes from
 * the plan), finished by hpri_wgrad_reduce_ex(ws, dw, splits, Cr, Nr, Cin, Cout, 3, 0, 0, accumulate). */
int hpri_wgrad_bf16v2_plan(int N, int H, int W, int Cin_pad, int Cout_pad, int* splits, int* Cr, int* Nr);
int hpri_conv_wgrad_bf16v2(const void* x_planes, int x_cs, int x_coff, int x_cvalid, const void* dy_planes, int dy_cs,
                           int dy_coff, int dy_cvalid, float* ws, size_t ws_floats, int N, int H, int W, int Cin_pad,
                           int Cout_pad, hipStream_t stream);

/* Weight gradient of the 1x1 layers (nn.Linear / Conv2d(k=1): models.py:105-115,143) from bf16 PLANES (wgrad_bf16v3.hip): plane 0
 * of the layer input and of the output gradient, P pixel rows each (strides / offsets / valid widths multiples of 8 elements), both
 * by LDS-DMA; slabs ws[splits][Nr][Cr] (sizes from the plan), finished by hpri_wgrad_reduce_ex(ws, dw, splits, Cr, Nr, Cin, Cout, 1,
 * 0, 0, accumulate). */
int hpri_wgrad1x1_bf16v3_plan(long long P, int Cin_pad, int Cout_pad, int* splits, int* Cr, int* Nr);
int hpri_wgrad1x1_bf16v3(const void* x_planes, int x_cs, int x_coff, int x_cvalid, const void* dy_planes, int dy_cs, int dy_coff,
                         int dy_cvalid, float* ws, size_t ws_floats, long long P, int Cin_pad, int Cout_pad, hipStream_t stream);

/* ConvTranspose2d(k=2,s=2) weight gradient (model_parts.py:63-64) from bf16 planes: x [N,H,W] (Cin channels) and the gradient of the
 * upsampled tensor dy [N,H2,W2] (Cup channels from dy_coff on, Cup % 64 == 0), gathered by parity; slab rows n = tap*Cup + co; plan:
 * hpri_wgrad1x1_bf16v3_plan(N*H*W, Cin_pad, 4*Cup); finish: hpri_wgrad_reduce_ex(ws, dw, splits, Cr, Nr, Cin, 4*Cup, 1, 1, Cup, acc). */
int hpri_wgrad_convt_bf16v3(const void* x_planes, int x_cs, int x_coff, int x_cvalid, const void* dy_planes, int dy_cs, int dy_coff,
                            float* ws, size_t ws_floats, int N, int H, int W, int Cin_pad, int Cup, int H2, int W2, int py0, int px0,
                            hipStream_t stream);

/* ---- BatchNorm (+ReLU) (bn.hip): nn.BatchNorm2d/3d/1d + nn.ReLU, model_parts.py:23-27; models.py:113-114,
 * 172-173,178-179.  G groups = independent statistic sets (G = N for SpectralUNET's per-image loop,
 * models.py:132). */
int hpri_bn_finalize(const float* partials, int tiles_per_group, int G, int Cp, int C, const float* gamma,
                     const float* beta, float eps, float momentum, float* mean, float* invstd, float* var_unbiased,
                     float* scale, float* shift, float* running_mean, float* running_var,
                     long long* num_batches_tracked, hipStream_t stream);
int hpri_bn_eval_prepare(const float* running_mean, const float* running_var, const float* gamma, const float* beta,
                         float eps, int C, float* mean, float* invstd, float* scale, float* shift, hipStream_t stream);
int hpri_bn_apply_relu(const float* x, int x_cs, int x_coff, float* y, int y_cs, int y_coff, const float* scale,
                       const float* shift, long long P, long long pix_per_group, int C, int Cw, int relu,
                       hipStream_t stream);
int hpri_col_reduce_plan(long long pix_per_group, int G, int C, int* nblk, int* Cpart);
int hpri_bn_relu_bwd(const float* dy, int dy_cs, int dy_coff, const float* x, int x_cs, int x_coff, float* dx,
                     int dx_cs, int dx_coff, const float* mean, const float* invstd, const float* scale,
                     const float* shift, float* dgamma, float* dbeta, int accumulate_param_grads, float* dbias,
                     int accumulate_dbias, float* workspace, size_t ws_floats, long long P, long long pix_per_group,
                     int C, int Cw, int relu, int use_batch_stats, hipStream_t stream);
int hpri_col_sum(const float* src, int cs, int coff, float* out, int accumulate, float* workspace, size_t ws_floats,
                 long long P, int C, hipStream_t stream);
/* the same sum taken from the per-tile (mean, M2, count, 0) records a convolution epilogue leaves (`stats` of hpri_conv_wino4 /
 * hpri_conv_bf16v3 / hpri_conv_fwd): out[c] (+)= sum over tiles of mean * count of channel c0 + c.  The ConvTranspose2d bias gradient
 * (model_parts.py:63-64) without a pass over the gradient tensor: the data-gradient kernel that wrote it recorded its columns. */
int hpri_colsum_from_stats(const float* stats, int tiles, int Cpad, int c0, int C, float* out, int accumulate,
                           hipStream_t stream);
/* the same two passes, also writing their output as bf16 planes (hpri_to_planes layout; channels [C, pl_cw) zero) for
 * the bf16-mode convolutions: the producer writes the planes, so no conversion pass reads the fp32 tensor again */
int hpri_nchw_to_nhwc_pl(const float* src, float* dst, int N, int C, long long P, int cs, int coff, int Cw, void* planes,
                         long long plane_stride, int pl_cs, int pl_coff, int pl_cw, int npl, hipStream_t stream);
int hpri_maxpool2_fwd_pl(const float* x, int x_cs, int x_coff, float* y, int y_cs, int y_coff, int N, int H, int W, int C,
                         void* planes, long long plane_stride, int pl_cs, int pl_coff, int pl_cw, int npl,
                         hipStream_t stream);
int hpri_bn_apply_relu_pl(const float* x, int x_cs, int x_coff, float* y, int y_cs, int y_coff, const float* scale,
                          const float* shift, long long P, long long pix_per_group, int C, int Cw, int relu, void* planes,
                          long long plane_stride, int pl_cs, int pl_coff, int pl_cw, int npl, hipStream_t stream);
/* dx may be NULL when planes are given: the gradient is then written as bf16 planes only (plane-mode consumers read nothing else). */
int hpri_bn_relu_bwd_pl(const float* dy, int dy_cs, int dy_coff, const float* x, int x_cs, int x_coff, float* dx,
                        int dx_cs, int dx_coff, const float* mean, const float* invstd, const float* scale,
                        const float* shift, float* dgamma, float* dbeta, int accumulate_param_grads, float* dbias,
                        int accumulate_dbias, float* workspace, size_t ws_floats, long long P, long long pix_per_group,
                        int C, int Cw, int relu, int use_batch_stats, void* planes, long long plane_stride, int pl_cs,
                        int pl_coff, int pl_cw, int npl, hipStream_t stream);
/* The pre-BatchNorm tensor stored as bf16 (bf16 precision mode, HPRI_YR_BF16: hpri_conv_bf16v3 with bit 2 of `accumulate` writes
 * it; x16[p * x_cs + x_coff + c], 8-byte aligned channel quads): the normalise pass and the backward read 2 instead of 4 bytes
 * per element of model_parts.py:23,26's input; arithmetic and every other argument as the fp32 forms. */
int hpri_bn_apply_relu_x16(const void* x16, int x_cs, int x_coff, float* y, int y_cs, int y_coff, const float* scale,
                           const float* shift, long long P, long long pix_per_group, int C, int Cw, int relu, void* planes,
                           long long plane_stride, int pl_cs, int pl_coff, int pl_cw, int npl, hipStream_t stream);

int hpri_bn_relu_bwd_x16(const float* dy, int dy_cs, int dy_coff, const void* x16, int x_cs, int x_coff, float* dx,
                         int dx_cs, int dx_coff, const float* mean, const float* invstd, const float* scale,
                         const float* shift, float* dgamma, float* dbeta, int accumulate_param_grads, float* dbias,
                         int accumulate_dbias, float* workspace, size_t ws_floats, long long P, long long pix_per_group,
                         int C, int Cw, int relu, int use_batch_stats, void* planes, long long plane_stride, int pl_cs,
                         int pl_coff, int pl_cw, int npl, hipStream_t stream);
/* ... and with the incoming gradient stored as bf16 as well (the inner tensor of a DoubleConv in the bf16 mode: written by its only
 * producer, hpri_conv_bf16v3 with the bf16-output bit, read only here; dy_cs / dy_coff in elements) */
int hpri_bn_relu_bwd_x16_dy16(const void* dy16, int dy_cs, int dy_coff, const void* x16, int x_cs, int x_coff, float* dx,
                              int dx_cs, int dx_coff, const float* mean, const float* invstd, const float* scale,
                              const float* shift, float* dgamma, float* dbeta, int accumulate_param_grads, float* dbias,
                              int accumulate_dbias, float* workspace, size_t ws_floats, long long P, long long pix_per_group,
                              int C, int Cw, int relu, int use_batch_stats, void* planes, long long plane_stride, int pl_cs,
                              int pl_coff, int pl_cw, int npl, hipStream_t stream);

/* ---- bandwidth-bound ops (elementwise.hip) ---------------------------------------------------------
 * layout change at the module boundary (dataset.py:267-271 hands NC(D)HW), nn.MaxPool2d(2)
 * (model_parts.py:40), F.pad + torch.cat (model_parts.py:77-87; models.py:235-239), OutConv / final Linear
 * (model_parts.py:96; models.py:103,143), synthetic generator. */
int hpri_nchw_to_nhwc(const float* src, float* dst, int N, int C, long long P, int cs, int coff, int Cw,
                      hipStream_t stream);
int hpri_nhwc_to_nchw(const float* src, float* dst, int N, int C, long long P, int cs, int coff, int accumulate,
                      hipStream_t stream);
int hpri_maxpool2_fwd(const float* x, int x_cs, int x_coff, float* y, int y_cs, int y_coff, int N, int H, int W, int C,
                      hipStream_t stream);
int hpri_maxpool2_bwd(const float* x, int x_cs, int x_coff, const float* dy, int dy_cs, int dy_coff, float* dx,
                      int dx_cs, int dx_coff, int N, int H, int W, int C, int accumulate, hipStream_t stream);
/* bf16 mode (round 4): max-pooling over / into bf16 rows -- the skip tensors of the U-Nets (model_parts.py:40 after a bf16-mode
 * DoubleConv) exist as planes only.  _fwd_x16: input = plane 0 of the skip's planes, y (fp32) optional (NULL: planes only).
 * _bwd_x16: x_bf16 / dx_bf16 select the storage of the pool's input and of its gradient; dy is fp32. */
int hpri_maxpool2_fwd_x16(const void* x16, int x_cs, int x_coff, float* y, int y_cs, int y_coff, int N, int H, int W, int C,
                          void* planes, long long plane_stride, int pl_cs, int pl_coff, int pl_cw, int npl, hipStream_t stream);
int hpri_maxpool2_bwd_x16(const void* x, int x_bf16, int x_cs, int x_coff, const float* dy, int dy_cs, int dy_coff, void* dx,
                          int dx_bf16, int dx_cs, int dx_coff, int N, int H, int W, int C, int accumulate, hipStream_t stream);
int hpri_copy_slice(const float* src, int s_cs, int s_coff, float* dst, int d_cs, int d_coff, long long P, int C,
                    int accumulate, hipStream_t stream);
int hpri_copy_slice_any(const float* src, int s_cs, int s_coff, float* dst, int d_cs, int d_coff, long long P, int C,
                        int Cz, int accumulate, hipStream_t stream);
int hpri_fill_pad(float* dst, int cs, int coff, int N, int H, int W, int C, int y0, int y1, int x0, int x1,
                  hipStream_t stream);
/* F.pad with positive and/or negative widths in one pass (model_parts.py:77-80, the crop case): dst[n][y][x] = src[n][y-oy][x-ox]
 * inside the Hs x Ws source, 0 outside. */
int hpri_shift_copy(const float* src, int s_cs, int s_coff, int Hs, int Ws, float* dst, int d_cs, int d_coff, int N, int Hd,
                    int Wd, int oy, int ox, int C, int accumulate, hipStream_t stream);
int hpri_fill(float* dst, long long n, float value, hipStream_t stream);
int hpri_outconv_fwd(const float* x, int x_cs, int x_coff, const float* w, const float* b, float* y, int N,
                     long long P, int C, int K, hipStream_t stream);
int hpri_outconv_bwd_plan(int N, long long P, int C, int K, int* nblk, int* Cpart);
int hpri_outconv_bwd(const float* dy, const float* x, int x_cs, int x_coff, const float* w, float* dx, int dx_cs,
                     int dx_coff, int dx_cw, int dx_accumulate, float* dw, float* db, int accumulate_param_grads,
                     float* workspace, size_t ws_floats, int N, long long P, int C, int K, hipStream_t stream);
/* The head fused with the loss of PLTrainer.py:86: hpri_outconv_fwd_bce also leaves per-block fp64 partial sums of
 * BCEWithLogits(logits, target) (hpri_outconv_fwd_bce_blocks doubles; finish: hpri_bce_finish -> mean loss); hpri_outconv_bwd_bce
 * takes the LOGITS, the target and the device scalar arriving at the loss and forms (sigmoid(logits) - target) * g / n inside
 * the data- and weight-gradient kernels.  Three launches and two passes over the logits less than loss and head apart. */
size_t hpri_outconv_fwd_bce_blocks(int N, long long P);
int hpri_outconv_fwd_bce(const float* x, int x_cs, int x_coff, const float* w, const float* b, float* y, const float* target,
                         double* partial, size_t partial_doubles, int N, long long P, int C, int K, hipStream_t stream);
int hpri_bce_finish(const double* partial, int nblk, long long n, float* loss, hipStream_t stream);
int hpri_outconv_bwd_bce(const float* logits, const float* target, const float* gscale, const float* x, int x_cs, int x_coff,
                         const float* w, float* dx, int dx_cs, int dx_coff, int dx_cw, int dx_accumulate, float* dw, float* db,
                         int accumulate_param_grads, float* workspace, size_t ws_floats, int N, long long P, int C, int K,
                         hipStream_t stream);
/* The head of the bf16 mode (model_parts.py:96 / models.py:103,143 after a bf16-mode layer): the input is plane 0 of the last
 * activation's plane buffer -- bf16 NHWC rows, x_cs / x_coff in elements (multiples of 8), pad channels zero -- so no fp32 copy of
 * that tensor is written or read.  target != NULL: with the loss partials (forward) / `dy` holds the logits and the loss gradient is
 * formed inside the kernels (backward), as hpri_outconv_fwd_bce / hpri_outconv_bwd_bce.  dx: fp32, or (dx_bf16, one class) bf16 rows. */
int hpri_outconv_fwd_x16(const void* x16, int x_cs, int x_coff, const float* w, const float* b, float* y, const float* target,
                         double* partial, size_t partial_doubles, int N, long long P, int C, int K, hipStream_t stream);
int hpri_outconv_bwd_x16(const float* dy, const float* target, const float* gscale, const void* x16, int x_cs, int x_coff,
                         const float* w, void* dx, int dx_bf16, int dx_cs, int dx_coff, int dx_cw, int dx_accumulate, float* dw,
                         float* db, int accumulate_param_grads, float* workspace, size_t ws_floats, int N, long long P, int C, int K,
                         hipStream_t stream);
/* Sweeps fused with the BatchNorm backward (fp32, one statistics group, C <= 1024).
 *
 * hpri_bn_relu_outconv_bwd: backward of  x -> BatchNorm (+ ReLU) -> y -> 1x1 head with one class  in two sweeps of the pre-BN tensor
 * x: dx (channels [C, Cw) zeros), dgamma / dbeta, dbias (the bias of the convolution in front; as hpri_bn_relu_bwd) and the head's
 * dw / db.  Neither y nor the head's input gradient is read or written.  `dy` = the logit gradient (N * P values), or -- target !=
 * NULL -- the logits, with the gradient of the mean BCE-with-logits loss formed inside (gscale, loss scale: hpri_outconv_bwd_bce).
 * Every result equals hpri_outconv_bwd(_bce) followed by hpri_bn_relu_bwd bit for bit (same per-block partial sums, same finalize
 * kernels).  workspace: hpri_bn_relu_outconv_bwd_ws floats.
 *
 * hpri_bn_relu_bwd_pool: training-mode BatchNorm + ReLU backward of a stage whose output y (N x H x W) feeds MaxPool2d(2) and,
 * optionally, a skip connection.  The gradient of y arrives as its two terms -- dskip (full resolution; NULL: none) and dpool
 * (N x H/2 x W/2), routed to the first maximum of each 2x2 window of y as hpri_maxpool2_bwd does -- and is never stored.  dbias is
 * cleared (exactly zero in training mode) unless accumulate_dbias.  workspace: nblk * 2 * Cpart + 2 * C floats
 * (hpri_bn_relu_bwd_pool_plan).
 *
 * hpri_col_finalize: the second stage of the column reductions by itself: sums[k][c] = sum of `nblk` partial rows [nblk][2][Cpart]
 * in double, out1 / out2 (optional) (+)= sums[0] / sums[1], zero_out (optional) cleared. */
/* hpri_bn_relu_outconv_fwd: the forward of the same pair from the pre-BN tensor x (C <= 256): logits and, target != NULL, the fp64 loss
 * partials, bit for bit those of hpri_bn_apply_relu + hpri_outconv_fwd / hpri_outconv_fwd_bce; y is not stored. */
int hpri_bn_relu_outconv_fwd(const float* x, int x_cs, int x_coff, const float* scale, const float* shift, int relu, const float* w,
                             const float* b, float* y, const float* target, double* partial, size_t partial_doubles, int N,
                             long long P, int C, hipStream_t stream);
/* hpri_bn_apply_relu_pool: BatchNorm apply (+ ReLU) of a stage whose output is max-pooled next: y (N x H x W) and its MaxPool2d(2) map
 * (N x H/2 x W/2) in one pass over the pre-BN tensor, both bit-equal to hpri_bn_apply_relu followed by hpri_maxpool2_fwd. */
int hpri_bn_apply_relu_pool(const float* x, int x_cs, int x_coff, float* y, int y_cs, int y_coff, float* pool, int p_cs, int p_coff,
                            const float* scale, const float* shift, int N, int H, int W, int C, int Cw, int relu, hipStream_t stream);
size_t hpri_bn_relu_outconv_bwd_ws(int N, long long P, int C);
int hpri_bn_relu_outconv_bwd(const float* dy, const float* target, const float* gscale, const float* x, int x_cs, int x_coff,
                             const float* w, float* dx, int dx_cs, int dx_coff, int Cw, const float* mean, const float* invstd,
                             const float* scale, const float* shift, float* dgamma, float* dbeta, int accumulate_bn_grads,
                             float* dbias, int accumulate_dbias, float* dw, float* db, int accumulate_head_grads, float* workspace,
                             size_t ws_floats, int N, long long P, int C, int relu, int use_batch_stats, hipStream_t stream);
int hpri_bn_relu_bwd_pool_plan(int N, int H, int W, int C, int* nblk, int* Cpart);
int hpri_bn_relu_bwd_pool(const float* dskip, int ds_cs, int ds_coff, const float* dpool, int dp_cs, int dp_coff, const float* x,
                          int x_cs, int x_coff, float* dx, int dx_cs, int dx_coff, const float* mean, const float* invstd,
                          const float* scale, const float* shift, float* dgamma, float* dbeta, int accumulate_param_grads,
                          float* dbias, int accumulate_dbias, float* workspace, size_t ws_floats, int N, int H, int W, int C, int Cw,
                          hipStream_t stream);
int hpri_col_finalize(const float* part, int nblk, int Cpart, int C, float* sums, float* out1, float* out2, int accumulate,
                      float* zero_out, hipStream_t stream);
/* nn.Upsample(scale_factor=2, 'bilinear', align_corners=True) (model_parts.py:57; models.py:195) writing at a pixel
 * offset of a padded destination, its gather-form gradient, and the element-wise "attention" product x2*x1
 * (model_parts.py:84-85). */
int hpri_upsample2x_fwd(const float* x, int x_cs, int x_coff, float* y, int y_cs, int y_coff, int N, int H, int W, int H2,
                        int W2, int py0, int px0, int C, hipStream_t stream);
int hpri_upsample2x_bwd(const float* dy, int dy_cs, int dy_coff, float* dx, int dx_cs, int dx_coff, int N, int H, int W,
                        int H2, int W2, int py0, int px0, int C, int accumulate, hipStream_t stream);
int hpri_mul(const float* a, int a_cs, int a_coff, const float* b, int b_cs, int b_coff, float* out, int o_cs, int o_coff,
             long long P, int C, int accumulate, hipStream_t stream);
int hpri_synth_fill(float* dst, long long n, unsigned long long seed, int mode, float thr, float scale,
                    hipStream_t stream);

/* ---- the caller-side tail of a step (step.hip) ---------------------------------
 * What RootLightningModel does with the logits once the network returns them:
 *   hpri_bce_logits_fwd / _bwd   nn.BCEWithLogitsLoss() mean, `loss = self.f_criterion(pred, batch['mask'])`
 *                                (PLTrainer.py:86,109,131; params_HyperPRI.py:60) and its gradient
 *                                dlogits = (sigmoid(x) - y) * grad_out / n; `loss` and `grad_out` are device scalars.
 *   hpri_seg_counts              `seg = torch.sigmoid(pred.detach()) > threshold` and the TP/FP/FN/TN counts that
 *                                Accuracy / JaccardIndex / Dice (PLTrainer.py:62-68,88-91) reduce to;
 *                                counts[4] (int64: TP, FP, FN, TN) are accumulated, so one buffer serves an epoch.
 *   hpri_pr_curve_hist           PrecisionRecallCurve('binary', thresholds=500) (PLTrainer.py:542-543; torchmetrics
 *                                1.2.0 binned update): hist[2][T+1] int64, bin = #{k : thresholds[k] <= p}, accumulated.
 *   hpri_adam_step / hpri_sgd_step  optim.Adam / optim.SGD over every parameter tensor (PLTrainer.py:171-181):
 *                                host arrays of device pointers + element counts; `grad_scale` (nullable device
 *                                scalar) multiplies the gradients first (1/world_size after a sum all-reduce). */
size_t hpri_bce_workspace_doubles(long long n);
int hpri_bce_logits_fwd(const float* logits, const float* target, long long n, float* loss, double* workspace,
                        size_t ws_doubles, hipStream_t stream);
int hpri_bce_logits_bwd(const float* logits, const float* target, long long n, const float* grad_out, float* dlogits,
                        hipStream_t stream);
int hpri_seg_counts(const float* pred, const float* target, long long n, float threshold, int is_logits,
                    long long* counts, hipStream_t stream);
int hpri_pr_curve_hist(const float* pred, const float* target, long long n, const float* thresholds, int T,
                       int is_logits, long long* hist, hipStream_t stream);
int hpri_adam_step(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                   const long long* numel, int ntensors, float lr, float beta1, float beta2, float eps,
                   float weight_decay, int step, const float* grad_scale, hipStream_t stream);
int hpri_sgd_step(float* const* params, const float* const* grads, float* const* momentum_buf, const long long* numel,
                  int ntensors, float lr, float momentum, float weight_decay, int first_step, const float* grad_scale,
                  hipStream_t stream);

/* ---- ingest fast path (ingest.hip) ---------------------------------------------------
 * `HyperpriDataset.__getitem__` (dataset.py:261-271) loads an ENVI cube as (H, W, B), moves the band axis to the
 * front on the host and slices [hsi_lo:hsi_hi].  These two take the (H, W, B) array as it is:
 *   hpri_hwb_ingest  device (H,W,B) f32/f16 -> zero-padded channels-last fp32 [P][dst_cs], bands [lo, lo+C)
 *   hpri_hwb_h2d     host (pinned) fp32 (H,W,B) -> the same layout directly, as one async 2-D H2D copy
 *                    (pad channels must have been zeroed once by the caller). */
int hpri_hwb_ingest(const void* src, int src_dtype, float* dst, long long P, int B, int lo, int C, int dst_cs,
                    int dst_cw, hipStream_t stream);
int hpri_hwb_h2d(const float* host_src, float* dst, long long P, int B, int lo, int C, int dst_cs, hipStream_t stream);

/* ---- device-resident cube cache (cache.hip; hyperpri_amd/cache.py) ----------------------------------------
 * A training split is stored once in device memory and every batch is assembled from it by one gather pass that crops
 * and flips on the way (the reference's augmentation: RandomCrop with one RNG state for image and mask,
 * params_HyperPRI.py:201-203, dataset.py:283-293).  dtype arguments: 0 = float32, 1 = float16.
 *   hpri_hwb_store    device (P, B) f32/f16 pixel-major cube -> one cache slot (P, cs), cs = roundup(C, 8) (cs % 8 == 0 is
 *                     required): bands [lo, lo+C) at channels [0, C), zeros at [C, cs); the slot is f32 or f16.
 *   hpri_cube_gather  cache (slots, Hs, Ws, cs) f32/f16 -> dst (N, h, w, cs) fp32, zero-padded channels-last:
 *                       dst[i, y, x, :] = cache[slot_i, top_i + (flags_i & 1 ? h-1-y : y), left_i + (flags_i & 2 ? w-1-x : x), :]
 *                     table: N entries {slot, top, left, flags} of four int32 in DEVICE memory, 16-byte aligned.
 *   hpri_mask_gather  the same table, crop and flips over uint8 masks (slots, Hs, Ws) -> fp32 (N, 1, h, w).
 * A window larger than the frame (h > Hs or w > Ws) is an argument error.  The launchers cannot read the table: the kernels
 * clamp slot, top and left into the cache, so a bad entry yields the wrong window but never an access outside the buffers;
 * callers validate their tables on the host. */
int hpri_hwb_store(const void* src, int src_dtype, void* dst, int dst_dtype, long long P, int B, int lo, int C, int cs,
                   hipStream_t stream);
int hpri_cube_gather(const void* cache, int cache_dtype, int slots, int Hs, int Ws, int cs, const int* table, int N, int h,
                     int w, float* dst, hipStream_t stream);
int hpri_mask_gather(const unsigned char* masks, int slots, int Hs, int Ws, const int* table, int N, int h, int w,
                     float* dst, hipStream_t stream);

/* ---- cube cache, augmenting gather (cache_warp.hip; hyperpri_amd/cache.py: CubeAugment) -------------------
 * The batch resampled from the cached slots through one affine map per sample (rotation, zoom, sub-pixel shift, flips), with a
 * photometric gain / offset and a run of dropped bands; the mask follows through the same map, nearest neighbour.
 * Warp entry: 64 bytes = 16 32-bit words per sample, in DEVICE memory, 16-byte aligned:
 *     word 0 int32 slot | 1 int32 drop_lo | 2 int32 drop_n | 3 reserved (0) | 4..9 fp32 a00, a01, cx, a10, a11, cy |
 *     10 fp32 gain | 11 fp32 offset | 12..15 reserved (0)
 * Output pixel (y, x) of an h x w window:  u = x - (w-1)/2, v = y - (h-1)/2 (exact in fp32),
 *     sx = a00*u + a01*v + cx,  sy = a10*u + a11*v + cy       (source column / row, pixel centres at integers, fp32)
 *   hpri_cube_warp  dst[n, y, x, c] = gain * bilinear(slot, sy, sx, c) + offset for c < C: neighbours (floor sy, floor sx), (+0,+1),
 *                   (+1,+0), (+1,+1) with weights (1-fy)(1-fx), (1-fy)fx, fy(1-fx), fy*fx in fp32 (f16 slots convert on load); a
 *                   neighbour outside [0,Hs) x [0,Ws) counts as 0 and is not loaded, nor is one of weight 0 (integer sx, sy with
 *                   gain 1 and offset 0 return the stored bits).  Channels [drop_lo, drop_lo + drop_n) are exactly 0 after gain and
 *                   offset; pad channels [C, cs) are exactly 0 whatever the offset.  dst: (N, h, w, cs) fp32.
 *   hpri_mask_warp  dst[n, 0, y, x] = (float)mask[slot, floor(sy + 0.5), floor(sx + 0.5)], 0 outside the frame; the same entries.
 * The window may be larger than the frame (zero fill); h, w <= 4096.  The launchers cannot read the entries: the kernels clamp the
 * slot into the cache, sx / sy in floating point into [-1, Ws] / [-1, Hs] (a NaN too) and the drop run into [0, cs], so a bad
 * entry yields a wrong picture but never an access outside the buffers. */
int hpri_cube_warp(const void* cache, int cache_dtype, int slots, int Hs, int Ws, int cs, int C, const int* entries, int N,
                   int h, int w, float* dst, hipStream_t stream);
int hpri_mask_warp(const unsigned char* masks, int slots, int Hs, int Ws, const int* entries, int N, int h, int w, float* dst,
                   hipStream_t stream);

/* ---- cube cache, deforming gather (cache_warp.hip, cache_deform.hip; hyperpri_amd/cache.py: CubeDeform) ---
 * The warp pair's pass with an elastic displacement field in the coordinate, Gaussian noise in the value and a CutMix rectangle
 * that hands pixels to another sample of the batch.  Beside the warp entries a second record per sample:
 * Deform entry: 64 bytes = 16 32-bit words per sample, in DEVICE memory, 16-byte aligned:
 *     word 0 int32 mix_from (batch index in [0, N) of the sample that owns the rectangle's pixels; anything else, -1 included, or the
 *     sample's own index: no CutMix) | 1..4 int32 ry0, ry1, rx0, rx1 (the rectangle [ry0,ry1) x [rx0,rx1) in window coordinates,
 *     clamped into the window by the kernels; empty: none) | 5 int32 nodes_off (offset in floats of the sample's lattice in the node
 *     table; negative: no elastic field) | 6, 7 int32 gy, gx (lattice rows, columns) | 8 fp32 inv_pitch (1 / node spacing in output
 *     pixels) | 9 fp32 noise_sigma (applied only when > 0; NaN or negative: none) | 10, 11 uint32 k0, k1 (Philox key) | 12..15 reserved (0)
 *   hpri_elastic_field  field[n, y, x, :] = (dx, dy) in output pixels, fp32: ty = y * inv_pitch, iy = clamp(floor ty, 0, gy - 4),
 *                   fy = ty - iy (x alike), d = sum_a sum_b B_a(fy) B_b(fx) node[iy+a][ix+b] over 4 x 4 nodes of the sample's (gy, gx, 2)
 *                   row-major lattice, uniform cubic B-spline: B0 = (1-f)^3/6, B1 = (3f^3 - 6f^2 + 4)/6, B2 = (-3f^3 + 3f^2 + 3f + 1)/6,
 *                   B3 = f^3/6.  Exact +0 for a sample without a lattice, with gy < 4 or gx < 4, or whose
 *                   [nodes_off, nodes_off + 2*gy*gx) does not lie inside [0, nodes_len) (the kernel decides: the launcher cannot see
 *                   the entries).  nodes may be null when nodes_len is 0.
 *   hpri_cube_deform / hpri_mask_deform  output pixel (y, x) of sample s: the owner o = mix_from[s] when CutMix is on for s and the
 *                   pixel lies in its rectangle, else s (o's own CutMix words are ignored);
 *                       u = (x + field[o,y,x,0]) - (w-1)/2,  v = (y + field[o,y,x,1]) - (h-1)/2        (field == NULL: zeros)
 *                   then sx, sy, the sampling, gain, offset and band drop of hpri_cube_warp / hpri_mask_warp with o's WARP entry and
 *                   the same clamps.  Cube: out = base = fmaf(gain, acc, offset), or fmaf(sigma, z, base) when sigma[s] > 0 -- noise and
 *                   key are always those of s; dropped and pad channels stay exactly 0; the mask never sees noise.
 *                   z: Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85) under the key
 *                   (k0, k1) at the counter (lo32 e, hi32 e, 0, 0), e = (y*w + x) * (cs/4) + c0/4 in 64 bits; output words r0..r3 belong
 *                   to channels c0..c0+3; pairs (r0, r1), (r2, r3) through Box-Muller: u = ((r >> 9) + 0.5f) * 2^-23,
 *                   rad = sqrtf(-2 logf(u_a)), z_a = rad * cospif(2 u_b), z_b = rad * sinpif(2 u_b).
 *   hpri_deform_noise_host  host only, no device: bits4 = the four Philox words, z4 = the four normals of counter e under (k0, k1)
 *                   (either pointer may be null, not both) -- the generator of the kernel, through the shared csrc/deform_math.h.
 * Argument errors -- a null pointer other than field, dtype, sizes, cs % 8, C outside (0, cs], h or w above 4096, the size products,
 * 16-byte alignment of cache / dst / entries / deform / field (the node table: 8), nodes_len < 0 -- are reported before any launch. */
int hpri_elastic_field(const float* nodes, long long nodes_len, const int* deform, int N, int h, int w, float* field,
                       hipStream_t stream);
int hpri_cube_deform(const void* cache, int cache_dtype, int slots, int Hs, int Ws, int cs, int C, const int* entries,
                     const int* deform, const float* field, int N, int h, int w, float* dst, hipStream_t stream);
int hpri_mask_deform(const unsigned char* masks, int slots, int Hs, int Ws, const int* entries, const int* deform,
                     const float* field, int N, int h, int w, float* dst, hipStream_t stream);
int hpri_deform_noise_host(unsigned int k0, unsigned int k1, unsigned long long e, unsigned int* bits4, float* z4);

/* ---- colour-coded segmentation maps (segmap.hip; hyperpri_amd/evaluate.py) --------------------------------
 * The per-pixel arithmetic of eval_color_segmaps (PLTrainer.py:219-267) minus matplotlib: three bands of the image as a
 * gamma-corrected pseudo-RGB picture (:236-240, `img[hsi_rgb] ** (1 / 2.2)`), prediction and ground truth painted in the
 * colour-blind palette (:243-258: truth overwrites prediction, agreement overwrites both) and blended over the picture as
 * `imshow(img); imshow(overlay, alpha=0.6)` blends them (:263-264).  All in fp32, per pixel:
 *     v_k    = image[n, band_k, y, x]; NaN -> 0; clamped to [0, 1]                       k = R, G, B
 *     base_k = gamma == 1 ? v_k : powf(v_k, inv_gamma)
 *     p = is_logits ? 1 / (1 + expf(-pred)) : pred;  s = p > threshold;  g = ((int)mask) != 0     (as hpri_seg_counts decides)
 *     class  = s + 2 g            0 neither, 1 prediction only, 2 truth only, 3 both
 *     over   = class ? palette[class - 1] : (0, 0, 0);   out_k = alpha * over_k + (1 - alpha) * base_k
 *     rgb_k  = (uint8)(out_k * 255 + 0.5f)
 * The clamp and the NaN rule are this library's; they differ from the reference only where it would hand matplotlib a NaN or
 * a value outside [0, 1].  The reference's defaults, as data: palette (202,0,32)/255, (5,133,176)/255, (155,191,133)/255;
 * alpha 0.6 (a pixel of neither class is the picture darkened to 0.4); HSI: bands (125, 49, 0) of the band-sliced cube with
 * gamma 2.2; RGB images: bands (0, 1, 2), gamma 1.
 *   image    fp32; element (n, band, y, x) at image[n*sn + band*sc + y*sy + x*sx] (strides in elements, >= 0), C bands: the
 *            zero-padded channels-last views of the cube cache / stager (sc = 1, sx = cs) and plain (N, C, h, w) alike
 *   pred, mask  contiguous (N, h, w) fp32;   rgb  (N, h, w, 3) uint8;   classes  (N, h, w) uint8 or NULL
 *   gamma > 0, inv_gamma = 1 / gamma as the caller forms it (Python: 1 / 2.2, rounded to float once); 0 <= alpha <= 1
 *   p0* / p1* / p2*  the palette by value: prediction only, truth only, both, each R, G, B in [0, 1]
 * Argument errors (null pointer, a size <= 0, a band index outside [0, C), gamma <= 0, alpha or a palette entry outside
 * [0, 1]) are reported before any launch. */
int hpri_segmap_overlay(const float* image, long long sn, long long sc, long long sy, long long sx, int C, int band_r,
                        int band_g, int band_b, const float* pred, const float* mask, int N, int h, int w, float threshold,
                        int is_logits, float gamma, float inv_gamma, float alpha, float p0r, float p0g, float p0b, float p1r,
                        float p1g, float p1b, float p2r, float p2g, float p2b, unsigned char* rgb, unsigned char* classes,
                        hipStream_t stream);
/* The multi-class picture: the same base picture (bands, clamp, NaN rule, gamma as above) under the colours of a uint8 class map
 * (N, h, w), predicted (the `classes` output of hpri_seg_confusion) or true:
 *     out_k = class == 0 ? base_k : alpha * palette[class][k] + (1 - alpha) * base_k;   rgb_k = (uint8)(out_k * 255 + 0.5f)
 *   palette  K x 3 HOST floats in [0, 1] (row 0, the background's, is never shown); 2 <= K <= 64; a class value >= K paints as 0 */
int hpri_segmap_classes(const float* image, long long sn, long long sc, long long sy, long long sx, int C, int band_r,
                        int band_g, int band_b, const unsigned char* classes, int N, int h, int w, float gamma,
                        float inv_gamma, float alpha, const float* palette, int K, unsigned char* rgb, hipStream_t stream);

/* ---- the multi-class tail of a step (multiclass.hip; hyperpri_amd/trainer.py, evaluate.py) ----------------
 * The counterpart of the BCE / seg_counts entries above for K class planes per pixel, 2 <= K <= 64 (anything else is an
 * argument error, reported before any launch).
 *   logits       contiguous NCHW fp32 (N, K, h, w), HW = h * w: class plane k of image n starts at (n*K + k)*HW
 *   target       one class index per pixel, (N, HW); target_kind 0 = fp32 holding integers (truncated toward zero), 1 = uint8,
 *                2 = int64
 *   weight       K per-class weights on the device, or NULL (all 1)
 *   use_ignore, ignore_index   pixels whose target equals ignore_index contribute nothing (use_ignore = 0: no such value)
 * A target that is neither ignored nor inside [0, K) -- a NaN or out-of-range fp32 value included -- is INVALID.  It is checked
 * before any use and never indexes the weight or the logits.  It cannot be reported without a host synchronisation, so it
 * poisons the result: the cross-entropy becomes NaN (the gradient rows of such pixels are zero), the confusion pass counts it
 * in counts[K*K].
 *   hpri_softmax_ce_fwd   nn.CrossEntropyLoss(weight, ignore_index, reduction): per pixel lse = max + log(sum exp(x - max)) in
 *                         one pass (running maximum and sum), l = w[t] * (lse - x_t).  Writes lse (N, HW) for the backward;
 *                         loss[0] = mean ? sum l / sum w[t] : sum l (an all-ignored mean is 0 / 0 = NaN, as in torch);
 *                         denom[0] = the divisor (1 for a sum), read by the backward; totals (nullable, 3 doubles on the
 *                         device) accumulate sum l, sum w[t] and the invalid count across calls.  fp64 partial sums in a fixed
 *                         order: bit-reproducible.  workspace: hpri_softmax_ce_workspace_doubles of N * HW doubles (pure host).
 *   hpri_softmax_ce_bwd   with p_k = exp(x_k - lse), c = w[t] * grad_out / denom (grad_out: device scalar, NULL = 1):
 *                         dlogits_k = p_k * c for k != t, dlogits_t = -(sum over j != t of p_j) * c -- never p_t - 1;
 *                         exact zeros in all K planes of an ignored or invalid pixel.
 *   hpri_seg_confusion    pred = argmax over the planes (lowest index among equal maxima, a NaN counts as the maximum: the
 *                         rules of torch.argmax); counts[t*K + pred] += 1 (int64, K*K + 1 entries, accumulated across calls
 *                         like hpri_seg_counts), counts[K*K] += invalid targets, ignored pixels skipped; classes (nullable):
 *                         the uint8 class map (N, HW).  target and counts are both given or both NULL (a plain argmax).
 * 16-byte accesses are used when HW % 4 == 0 and every base pointer is 16-byte aligned, element accesses otherwise; the
 * results are the same bit for bit. */
size_t hpri_softmax_ce_workspace_doubles(long long npix);
int hpri_softmax_ce_fwd(const float* logits, const void* target, int target_kind, const float* weight, int N, int K,
                        long long HW, int use_ignore, long long ignore_index, int mean, float* loss, float* lse, float* denom,
                        double* totals, double* workspace, size_t ws_doubles, hipStream_t stream);
int hpri_softmax_ce_bwd(const float* logits, const float* lse, const void* target, int target_kind, const float* weight, int N,
                        int K, long long HW, int use_ignore, long long ignore_index, const float* denom, const float* grad_out,
                        float* dlogits, hipStream_t stream);
int hpri_seg_confusion(const float* logits, const void* target, int target_kind, int N, int K, long long HW, int use_ignore,
                       long long ignore_index, long long* counts, unsigned char* classes, hipStream_t stream);

/* ---- imbalance-aware binary losses (segloss.hip; hyperpri_amd/trainer.py: SegLoss and its subclasses) --------
 * One family over contiguous fp32 logits x and fp32 targets y in [0, 1] (soft labels allowed), n_img images of hw elements:
 *     loss = w_point * R_elems[ a_t * (1 - p_t)^focal_gamma * ce(x, y) ] + w_overlap * mean_groups[ (1 - T_g)^tversky_gamma ]
 *     ce(x, y) = pos_weight * y * softplus(-x) + (1 - y) * softplus(x);   1 - p_t = y * sigmoid(-x) + (1 - y) * sigmoid(x)
 *     a_t = focal_alpha * y + (1 - focal_alpha) * (1 - y)                  (focal_alpha < 0: a_t = 1)
 *     T_g = (I + s) / D,  D = I + alpha * (P - I) + beta * (Y - I) + s,  I = sum p*y, P = sum p, Y = sum y over group g, p = sigmoid(x)
 * R_elems: the mean (mean != 0) or the sum over all elements; a group: one image (per_image != 0) or the whole batch; s = smooth.
 * Dice is alpha = beta = 1/2 (the usual (2I + smooth) / (P + Y + smooth) has s = smooth / 2); focal_gamma = 0 with pos_weight != 1
 * is weighted BCE.  A weight of 0 drops its term: the kernels do not evaluate it.  Edge rules: D == 0 gives T = 1; T >= 1 gives a
 * term of 0 with derivative 0.
 *   hpri_seg_loss_fwd   one pass over x and y (fp64 partial sums per workgroup in a fixed order, no floating-point atomics:
 *                       bit-reproducible) and a one-workgroup finalize.  loss[0]: the loss; terms[0..2]: R_elems[...] and
 *                       mean_groups[...] before their weights (0 for a dropped term) and the mean of T_g;  state: what the backward
 *                       reads, hpri_seg_loss_state_doubles doubles -- state[0] = w_point (/ (n_img * hw) for a mean), then per
 *                       group c1_g, c0_g with  c1_g = w_overlap / G * dL/dT_g * (D - (I + s)(1 - alpha - beta)) / D^2,
 *                       c0_g = w_overlap / G * dL/dT_g * (-(I + s) * alpha) / D^2,  dL/dT = -gamma_t * (1 - T)^(gamma_t - 1).
 *                       workspace: hpri_seg_loss_workspace_doubles(n_img, hw) doubles (pure host functions, both).
 *   hpri_seg_loss_bwd   dlogits_i = grad_out * [ state[0] * d(pointwise_i)/dx_i + (c1_g * y_i + c0_g) * sigmoid(x_i) * sigmoid(-x_i) ]
 *                       in one pass, the focal derivative analytic for any y; grad_out: device scalar, NULL = 1.  The pointwise
 *                       parameters, the two weights and per_image must be those of the forward.
 * No host synchronisation anywhere.  16-byte accesses when hw % 4 == 0 and every base pointer is 16-byte aligned, element accesses
 * otherwise, bit-identical results.  Argument errors, reported before any launch: a null pointer, a size <= 0, pos_weight <= 0,
 * focal_gamma < 0, focal_alpha > 1, alpha < 0, beta < 0, alpha + beta == 0, smooth < 0, tversky_gamma <= 0, both weights 0, a
 * workspace that is too small, a state buffer (state_doubles: its size in doubles, forward and backward) smaller than
 * hpri_seg_loss_state_doubles(n_img, per_image). */
size_t hpri_seg_loss_workspace_doubles(int n_img, long long hw);
size_t hpri_seg_loss_state_doubles(int n_img, int per_image);
int hpri_seg_loss_fwd(const float* logits, const float* target, int n_img, long long hw, float w_point, float pos_weight,
                      float focal_gamma, float focal_alpha, int mean, float w_overlap, float tversky_alpha, float tversky_beta,
                      float smooth, float tversky_gamma, int per_image, float* loss, double* state, size_t state_doubles,
                      float* terms, double* workspace, size_t ws_doubles, hipStream_t stream);
int hpri_seg_loss_bwd(const float* logits, const float* target, int n_img, long long hw, float w_point, float pos_weight,
                      float focal_gamma, float focal_alpha, float w_overlap, int per_image, const double* state,
                      size_t state_doubles, const float* grad_out, float* dlogits, hipStream_t stream);

/* ---- test-time augmentation, the merge (tta.hip; hyperpri_amd/tta.py, evaluate.py) --------------------------
 * The logits of V dihedral views of a batch, brought back to the original h x w frame and merged in one launch.
 *   views   HOST array of V device pointers (1 <= V <= 8); view v is a contiguous fp32 (N, K, hv, wv) tensor, (hv, wv) = (h, w)
 *           for codes 0 .. 3 and (w, h) for codes 4 .. 7.  Pointers and codes travel as kernel arguments: nothing is uploaded.
 *   codes   HOST array of V view codes: 0 id, 1 flip_h (rows reversed), 2 flip_w (columns reversed), 3 rot180, 4 rot90
 *           (torch.rot90(x, 1, (-2, -1))), 5 rot270, 6 transpose, 7 antitranspose
 *   N, K, h, w   images, planes (1 <= K <= 64) and the ORIGINAL frame;  mode  0 logit, 1 prob
 *   out     (N, K, h, w) fp32;  spread  (N, h, w) fp32 or NULL (not computed)
 * With s_v = view v's value at the pixel that (y, x) was sent to:
 *   mode 0          out = (((s_0 + s_1) + s_2) ... + s_{V-1}) * (1 / V): fp32 adds in view order, one multiply by the fp32 quotient
 *                   1 / V, nothing fused -- bit-reproducible, and the input bits for V = 1 with id.
 *   mode 1, K = 1   p_v = 1 / (1 + exp(-s_v)), q_v = 1 / (1 + exp(s_v)) (each on its own: both tails stay accurate), means in view
 *                   order;  out = log(max(mean p, FLT_MIN)) - log(max(mean q, FLT_MIN)), the logit of the mean probability.
 *   mode 1, K > 1   per view the softmax over the K planes (row maximum subtracted), p_vk = exp(s_vk - m_v) * (1 / sum_v), the mean
 *                   over the views, out_k = log(max(mean p_k, FLT_MIN)): log-probabilities, softmax(out) = mean p.
 *   spread, K = 1   the population standard deviation over the views of p_v (both modes), two passes over registers
 *   spread, K > 1   the fraction of views whose own argmax differs from the argmax of the merged out (lowest index among equal
 *                   maxima, a NaN counts as the maximum)
 * The logarithms are evaluated in fp64 and rounded once (an fp32 logarithm's error grows with the logit); exp, the divisions and
 * the means are fp32.  NaN inputs propagate.  Every output element is written once and never read; no atomics; 64-bit offsets.  Argument errors (a null
 * pointer, V, K, a code or mode out of range, a size <= 0) are reported before any launch. */
int hpri_tta_merge(const float* const* views, const int* codes, int V, int N, int K, int h, int w, int mode, float* out,
                   float* spread, hipStream_t stream);

/* ---- connected components (components.hip; hyperpri_amd/components.py, evaluate.py) ------------------------
 * Label a binary decision map, measure its components, clean it; all results are integers.
 *   pred        contiguous (N, h, w), N*h*w < 2^31; pred_kind 0 = fp32, decided as hpri_seg_counts / hpri_segmap_overlay decide:
 *               p = is_logits ? 1 / (1 + expf(-x)) : x;  fg = p > threshold;   pred_kind 1 = uint8, fg = value != 0;
 *               pred_kind 2 = fp32 mask, fg = ((int)value) != 0, how the tail reads a mask (1, 2: threshold and is_logits unused).
 *               invert != 0 labels the background instead.
 *   connectivity  4 or 8.  Images never connect to each other.
 *   workspace   hpri_cc_workspace_ints 32-bit words on the device (pure host function; 0 for a bad shape), contents scratch.
 * Labelling is union-find over linear indices with parent[i] <= i (background -1; the root of a component is its smallest index):
 * a per-tile pass in LDS (hpri_cc_tile_h x hpri_cc_tile_w pixels per workgroup), a border pass that unites neighbours across tile
 * edges in global memory (every access to parent an agent-scope atomic: relaxed load / atomicMin), an out-of-place flatten.  The
 * phases are separate launches on `stream`; no workgroup waits for another; every loop over parent ends because an index (find) or a
 * value (union by atomicMin, retried on the returned value) strictly decreases.  Integer atomics only: bit-reproducible.
 *   hpri_cc_label    labels (N, h, w) int32: 0 background, 1..counts[n] per image in raster order of each component's first pixel
 *                    (the rank of its root; the numbering of scipy.ndimage.label);  counts (N) int32.
 *   hpri_cc_measure  one pass over labels: table row offsets[n] + label - 1 (rows ordered by image, label) = six int32: area, y0,
 *                    x0, y1, x1 (inclusive box), overlap = pixels of the component where ((int)truth) != 0 (0 without truth; truth
 *                    contiguous (N, h, w), truth_kind 0 = fp32, 1 = uint8, 2 = int32: value != 0, e.g. another label map).
 *                    table_rows >= sum of counts: rows past table_rows are never written; offsets: N + 1 int32 of device
 *                    scratch.  table_rows = 0: nothing is launched.
 *   hpri_cc_clean    out (N, h, w) uint8 = the cleaned decision: a foreground component (connectivity) with area < min_area becomes
 *                    background; a background component -- labelled with the DUAL connectivity, 4 for foreground 8 and 8 for
 *                    foreground 4 -- whose box touches no image edge and whose area <= max_hole becomes foreground.  Holes are
 *                    found in the input decision, not after speck removal: the two edits act on disjoint pixels, so their order
 *                    is immaterial.  out_logits (nullable): (N, h, w) fp32, +logit where the cleaned decision is foreground
 *                    and -logit elsewhere.  stats: four int64 on the device, ACCUMULATED like the buffer of hpri_seg_counts:
 *                    components removed, pixels removed, holes filled, pixels filled.
 * Argument errors (a null pointer, N, h or w <= 0, N*h*w >= 2^31, connectivity not 4 or 8, a kind outside 0..2, min_area or max_hole
 * negative) return -1 before any launch; a workspace that is too small returns -3. */
size_t hpri_cc_workspace_ints(int N, int h, int w);
int hpri_cc_tile_h(void);
int hpri_cc_tile_w(void);
int hpri_cc_label(const void* pred, int pred_kind, float threshold, int is_logits, int invert, int N, int h, int w,
                  int connectivity, int* labels, int* counts, int* workspace, size_t ws_ints, hipStream_t stream);
int hpri_cc_measure(const int* labels, const int* counts, const void* truth, int truth_kind, int N, int h, int w, int* table,
                    int table_rows, int* offsets, hipStream_t stream);
int hpri_cc_clean(const void* pred, int pred_kind, float threshold, int is_logits, int N, int h, int w, int connectivity,
                  int min_area, int max_hole, unsigned char* out, float* out_logits, float logit, long long* stats,
                  int* workspace, size_t ws_ints, hipStream_t stream);

/* ---- distance transform, selection histogram, thinning (distance.hip; hyperpri_amd/distance.py, evaluate.py) ---------------
 * Integers only; the atomics are integer adds and maxima on vector memory: every result is bit-reproducible.  pred, pred_kind,
 * threshold, is_logits: the decision of hpri_cc_label; maps are contiguous (N, h, w), N*h*w < 2^31; images never influence each other.
 *   hpri_edt            d2 (N, h, w) int32 = min(FAR, min over the sites q of the image of (y-qy)^2 + (x-qx)^2), FAR = h*h + w*w (an
 *                       image without a site is FAR everywhere).  sites 0: the background pixels, 1: the foreground pixels, 2: the
 *                       boundary -- foreground pixels with one of their four edge neighbours in the background or outside the image.
 *                       A column pass (one thread per column, down then up, hpri_edt_col_threads columns per workgroup) and an
 *                       in-place row pass (one workgroup of hpri_edt_row_threads threads per row, the row staged in LDS, an outward
 *                       scan per pixel that stops at k^2 >= best).  hpri_edt_far (pure host) gives FAR, or -1 where the transform
 *                       does not exist: a size <= 0, w > hpri_edt_max_width (the row's LDS budget), h*h + w*w >= 2^31.
 *   hpri_select_stats   over the pixels p of image n that the selector picks (sel_kind 0: uint8 map, value != 0; 1: int32 map, value
 *                       == 0, e.g. the sites of a distance transform) with values[p] >= 0:  stats[n*stats_stride] += their number,
 *                       stats[n*stats_stride + 1] = max(itself, their largest value).  ACCUMULATED: the caller zeroes.
 *   hpri_select_hist    hist[n*hist_stride + v] += 1 for each such pixel with v = values[p] < bins (a larger value is not counted).
 *                       ACCUMULATED.  Reduced in LDS first where bins <= hpri_select_hist_lds_bins.
 *   hpri_thin           Zhang-Suen thinning.  decide != 0: map = the uint8 decision of pred first (pairs = 0: only that).  Then
 *                       `pairs` times sub-iteration 1 map -> other and sub-iteration 2 other -> map: with P2..P9 the neighbours
 *                       clockwise from north (outside the image: background), B their sum and A the 0 -> 1 steps around the ring, a
 *                       foreground pixel goes when 2 <= B <= 6, A == 1 and P2*P4*P6 == 0, P4*P6*P8 == 0 (sub-iteration 1) or
 *                       P2*P4*P8 == 0, P2*P6*P8 == 0 (sub-iteration 2).  deleted[j*N + n] += pixels pair j took from image n
 *                       (pairs * N int32, ACCUMULATED).  A pair that deletes nothing leaves map as it is: map is converged.
 *   hpri_skeleton_links links[3n..3n+2] += S, E4, Ed of image n: skeleton pixels, horizontally or vertically adjacent pairs,
 *                       diagonally adjacent pairs whose two common edge neighbours are both off the skeleton.  ACCUMULATED.
 * Argument errors (a null pointer, a size <= 0, N*h*w >= 2^31, a kind, sites or sel_kind out of range, a row beyond
 * hpri_edt_max_width, h*h + w*w >= 2^31, bins <= 0, a stride below its row) return -1 before any launch. */
int hpri_edt_max_width(void);
int hpri_edt_col_threads(void);
int hpri_edt_row_threads(void);
int hpri_edt_far(int h, int w);
int hpri_select_hist_lds_bins(void);
int hpri_edt(const void* pred, int pred_kind, float threshold, int is_logits, int sites, int N, int h, int w, int* d2,
             hipStream_t stream);
int hpri_select_stats(const int* values, const void* selector, int sel_kind, int N, int per_image, int* stats, int stats_stride,
                      hipStream_t stream);
int hpri_select_hist(const int* values, const void* selector, int sel_kind, int N, int per_image, int bins, int* hist,
                     long long hist_stride, hipStream_t stream);
int hpri_thin(const void* pred, int pred_kind, float threshold, int is_logits, int N, int h, int w, int decide, int pairs,
              unsigned char* map, unsigned char* other, int* deleted, hipStream_t stream);
int hpri_skeleton_links(const unsigned char* skeleton, int N, int h, int w, int* links, hipStream_t stream);

/* ---- spectral statistics and projection (spectral.hip; hyperpri_amd/spectral.py) ---------------------------------------------
 * The band axis of the cube cache.  cache, cache_dtype, slots, Hs, Ws, cs: the slots as hpri_cube_gather reads them ((slots, Hs,
 * Ws, cs) fp32 / fp16, cs % 8 == 0 and cs <= hpri_band_max_cs, zeros above the bands); masks: (slots, Hs, Ws) uint8 (may be null
 * with select 0).  slot_table: n int32 on the device, the slots to read (clamped into the cache by the kernels).  select 0: every
 * pixel, 1: mask != 0, 2: mask == 0; a pixel that is not selected contributes exact zeros.
 *   hpri_band_moments   *count (int64) = the selected pixels, sums[c] (fp64, cs) = their sum of x[c].  With pivot (fp32, cs, zero pad
 *                       entries) and sumsq both given: sums[c] = sum of d[c] and sumsq[c] = sum of d[c]^2, d = x - pivot rounded once
 *                       to fp32.  One pass, 16-byte loads.
 *   hpri_band_gram      gram[i*cs + j] (fp64, cs x cs, the full symmetric matrix) = sum over the selected pixels of d[i] * d[j].
 *                       Products and sums on v_mfma_f32_32x32x2_f32 (bitwise an fmaf chain over the pixels); the upper triangle of
 *                       32 x 32 blocks is computed, the rest mirrored: exactly symmetric, pad rows and columns exactly zero.
 *   Both: a sum stays in fp32 for at most hpri_band_fp32_run pixels (one RUN: run r of list entry e covers its pixels [r * RUN,
 *   (r + 1) * RUN)) and is then added into an fp64 partial; partial a owns the runs a, a + PARTS, ... of the launch in that order
 *   (PARTS a constant: 2048 for the moments, 256 for the Gram matrix), and a finishing kernel adds the partials in ascending order.
 *   No floating-point atomic: two calls on the same arguments give the same bits on any gfx950 part.  workspace: at least
 *   hpri_band_workspace_bytes(cs) bytes, 16-byte aligned -- a function of cs alone (0 for a cs the family does not take).
 *   hpri_band_project   y[p*ks + k] = fmaf(W[k][cs-1], x[p][cs-1], ... fmaf(W[k][0], x[p][0], b[k])) for the `pixels` rows of a
 *                       zero-padded channels-last fp32 batch x (pixels, cs); ks = roundup(K, 8), weight (ks, cs) and bias (ks) fp32
 *                       with zero pad rows, columns and entries, so the pad channels of y are exact zeros.  v_mfma_f32_16x16x4_f32;
 *                       the weights stay in LDS for a workgroup's lifetime, 16-byte accesses both ways.  K <= hpri_band_project_max_k
 *                       (64); weights plus a 64-pixel tile must fit the LDS (cs <= 304 at ks = 64).
 *   hpri_band_affine    y[p*cs + c] = fmaf(x[p*cs + c], scale[c], shift[c]) for c < C, 0 for C <= c < cs.
 * Argument errors (a null pointer, a size <= 0, cs % 8 != 0 or beyond hpri_band_max_cs, a select or dtype out of range, a selection
 * without masks, K beyond the maximum, a workspace that is too small, a misaligned pointer) return -1 before any launch. */
int hpri_band_fp32_run(void);
int hpri_band_max_cs(void);
int hpri_band_project_max_k(void);
size_t hpri_band_workspace_bytes(int cs);
int hpri_band_moments(const void* cache, int cache_dtype, int slots, int Hs, int Ws, int cs, const unsigned char* masks,
                      const int* slot_table, int n, int select, const float* pivot, void* workspace, size_t workspace_bytes,
                      long long* count, double* sums, double* sumsq, hipStream_t stream);
int hpri_band_gram(const void* cache, int cache_dtype, int slots, int Hs, int Ws, int cs, const unsigned char* masks,
                   const int* slot_table, int n, int select, const float* pivot, void* workspace, size_t workspace_bytes,
                   double* gram, hipStream_t stream);
int hpri_band_project(const float* x, long long pixels, int cs, const float* weight, const float* bias, int K, float* y,
                      hipStream_t stream);
int hpri_band_affine(const float* x, long long pixels, int cs, int C, const float* scale, const float* shift, float* y,
                     hipStream_t stream);

/* ---- spectral detectors: RX, matched filter, ACE, SAM (detect.hip; hyperpri_amd/detect.py) ------------------------------------
 * x: the zero-padded channels-last fp32 batch (pixels, cs) hpri_band_project takes (cs % 8 == 0, cs <= hpri_band_max_cs); weight
 * (ks, cs) and bias (ks) fp32 with zero pad rows and columns: the first Kq <= cs rows are QUADRATIC rows (a whitener), the next
 * T <= hpri_band_detect_max_targets (8) rows FILTER rows, Kq + T <= ks.  Per pixel
 *   z[k] = fmaf(W[k][cend-1], x[cend-1], ... fmaf(W[k][0], x[0], b[k]))   every row k < Kq + T (v_mfma_f32_16x16x4_f32: bitwise this chain)
 *   q    = sum over k < Kq of z[k]^2,      t[j] = z[Kq + j], j < T
 * cend: a HOST array with one column extent per 16-row block of the Kq + T rows, each a multiple of 8 in [8, cs]; NULL: cs.  The k
 * loop of a block stops there (a lower-triangular whitener costs about half the MFMAs); for finite inputs the skipped terms are
 * exact no-ops, so z is the same up to the sign of a zero.  The caller owns the table: W lives on the device and is not inspected,
 * a table that cuts off a non-zero drops those terms.
 * The order of q depends on Kq alone (not on the pixel count, the grid or the pixel's place in its tile): with rb the 16-row blocks,
 * "wave" w in 0 .. 7 owns block 8 r + w in even rounds r and 8 r + 7 - w in odd ones; s(w, kq) = fmaf(z, z, s), from 0, over the
 * quadratic rows 16 rb + 4 kq + j (j = 0 .. 3) of w's blocks in round order; q = s(0,0) + s(0,1) + s(0,2) + s(0,3) + s(1,0) + ... +
 * s(7,3), added left to right.  No floating-point atomic: identical arguments give identical bits.
 * Outputs: q (pixels) fp32, may be NULL; scores (T, pixels) fp32 planes (NULL exactly when T == 0).  score selects what is written,
 * fused in the epilogue:  0: t[j];  1: the cosine t[j] * rsqrt(q), 0 where q == 0;  2, 3: the logit log(p) - log1p(-p) of 0, 1 with
 * p = clamp(value, 2^-24, 1 - 2^-24), and then q is written as the logit of p = q / (q + Kq) as well.
 * Identity metric: weight == NULL (then Kq == 0, cend == NULL): q = fmaf(x[c], x[c], q) from 0 and t[j] = fmaf(F[j][c], x[c], t[j])
 * from bias[j] (0 with bias == NULL), both ascending c; F = filters, (T, cs) fp32, 16-byte aligned (NULL otherwise and when T == 0).
 * No matrix unit: one memory-bound sweep with 16-byte loads; q is always written raw.
 * A bad size, a misaligned pointer, Kq + T not fitting ks, T beyond the maximum, a cs out of range, a bad extent or an unknown score
 * return -1 before any launch.  hpri_band_detect_max_targets is a pure host query. */
int hpri_band_detect_max_targets(void);
int hpri_band_detect(const float* x, long long pixels, int cs, const float* weight, const float* bias, int ks, int Kq, int T,
                     const float* filters, const int* cend, int score, float* q, float* scores, hipStream_t stream);

/* ---- spectral k-means: assignment and the fitting pass (cluster.hip; hyperpri_amd/cluster.py) ------------------------------------
 * A generic argmin of K affine scores of a centred pixel; K <= hpri_band_cluster_max_k (64), cs % 8 == 0 and cs <= hpri_band_max_cs.
 *   d[c]  = fp32(x[c] - pivot[c]), rounded once exactly as hpri_band_gram rounds it; pivot: fp32 (cs), zero pad entries; NULL: d = x
 *   z[k]  = fmaf(centers[k][cs-1], d[cs-1], ... fmaf(centers[k][0], d[0], bias[k]))   ascending c from the bias: bitwise the chain of
 *           hpri_band_project (v_mfma_f32_16x16x4_f32 with k = band); centers (ks, cs) fp32, ks = roundup(K, 8), zero pad rows and
 *           columns; bias (ks) fp32
 *   label = the lowest k < K with z[k] == min over k < K,  zmin = z[label].  Rows >= K never take part (no infinite bias is needed),
 *           and label < K holds for every input, non-finite ones included; what a NaN pixel is labelled is otherwise unspecified.
 * For a centroid g_k the caller passes centers[k] = -g_k and bias[k] = |g_k|^2 / 2; the kernels know nothing of that.
 *   hpri_band_assign        x: the zero-padded channels-last fp32 batch (pixels, cs) hpri_band_project takes.  Outputs, each may be NULL
 *                           but not all: labels (pixels) uint8; zmin (pixels) fp32; dist2 (pixels) fp32 = max(0, fmaf(2, zmin, s)) with
 *                           s = fmaf(d[c], d[c], s) from 0, ascending c (the squared distance to the nearest centroid); value (pixels)
 *                           fp32 = lut[label], lut: K fp32, given exactly when value is.  One pass; the centres stay in LDS for a
 *                           workgroup's lifetime (a tile of 64 pixels beside them, 32 where both do not fit: cs > 304 at ks = 64);
 *                           nothing of size pixels x K is written; the result of a pixel depends neither on the pixel count, nor on
 *                           the grid, nor on the pixel's place in its tile.
 *   hpri_band_cluster_sums  over the selected pixels of the listed slots (the leading arguments of hpri_band_gram, fp32 and fp16
 *                           caches): counts[k] (int64, K) = the pixels with label k, exact; sums[k*cs + c] (fp64, K x cs) = the sum of
 *                           d[c] over them; totals[0] = the sum of zmin, totals[1] = the sum over pixels and c of d[c]^2 (fp64).  A
 *                           pixel that is not selected contributes exact zeros and counts nowhere.  The labels are those
 *                           hpri_band_assign gives the same pixel, bit for bit: same d, same chain, same code.
 *     Summation: the runs are those of hpri_band_gram (hpri_band_fp32_run pixels).  Inside a run sums[k][c] is the fp32 chain
 *     acc = fmaf(onehot, d[p][c], acc) from 0 over ALL the run's pixels p in ascending order (v_mfma_f32_32x32x2_f32 with k = pixel,
 *     onehot = 1 for the pixel's cluster, else 0: a pixel of another cluster, one that is not selected and the zero pad add exact
 *     zeros).  After the run the chain is added into an fp64 partial; partial a owns the runs a, a + PARTS, ... of the launch in that
 *     order, PARTS = hpri_band_cluster_parts() = 256, a constant; a finishing kernel adds the partials in ascending order.  zmin and
 *     the per-pixel s (the fp32 chain above) are added in fp64 pixel by pixel: pixel i of a chunk of 64 (32 with the small tile) of a
 *     run goes to accumulator i of the run's partial, and the 64 accumulators are added in ascending order before the partials are.
 *     Counts: integer atomics inside a workgroup, then the partial scheme.  No floating-point atomic: the bits depend on the arguments
 *     and these constants only, not on the grid or the CU count.
 *     workspace: hpri_band_cluster_workspace_bytes(cs, K) bytes, 16-byte aligned; a pure host query, a function of its arguments
 *     alone (0 for a cs or K the pass does not take).
 * Argument errors (a null pointer, a size <= 0, cs % 8 != 0 or beyond hpri_band_max_cs, K outside [1, hpri_band_cluster_max_k], a select
 * or dtype out of range, a selection without masks, a workspace that is too small or misaligned, value without lut or lut without
 * value, no output at all, a misaligned pointer) return -1 before any launch. */
int hpri_band_cluster_max_k(void);
int hpri_band_cluster_parts(void);
size_t hpri_band_cluster_workspace_bytes(int cs, int K);
int hpri_band_assign(const float* x, long long pixels, int cs, const float* pivot, const float* centers, const float* bias, int K,
                     const float* lut, unsigned char* labels, float* zmin, float* dist2, float* value, hipStream_t stream);
int hpri_band_cluster_sums(const void* cache, int cache_dtype, int slots, int Hs, int Ws, int cs, const unsigned char* masks,
                           const int* slot_table, int n, int select, const float* pivot, const float* centers, const float* bias, int K,
                           void* workspace, size_t workspace_bytes, long long* counts, double* sums, double* totals,
                           hipStream_t stream);

/* ---- spectral Gaussian mixtures: scores and the E-step with the M-step's sums (mixture.hip; hyperpri_amd/mixture.py) ---------------
 * K <= hpri_band_gmm_max_components (8) Gaussians with full covariances in a shared projection to q <= hpri_band_gmm_max_dims (32)
 * dimensions; component k belongs to class classes[k] < C <= 8.  cs % 8 == 0 and cs <= hpri_band_max_cs; qp = roundup(q, 8).
 *   d[c]   = fp32(x[c] - pivot[c]), as hpri_band_assign rounds it; pivot: fp32 (cs), zero pad entries; NULL: d = x
 *   z[i]   = fmaf(weight[i][cs-1], d[cs-1], ... fmaf(weight[i][0], d[0], 0))      i < q: bitwise the chain of hpri_band_project from a
 *            zero bias; weight (qp, cs) fp32, zero pad rows and columns
 *   u_k[i] = fmaf(A[k][i][qp-1], z[qp-1], ... fmaf(A[k][i][0], z[0], a[k][i]))    A (K, qp, qp), a (K, qp) fp32, zero pad entries.  For a
 *            covariance Sigma_k = L_k L_k^T and a mean m_k the caller passes A_k = L_k^-1 and a_k = -A_k m_k
 *   m_k    = sum_i u_k[i]^2: with s_g = fmaf(u[i], u[i], s_g) from 0 over the rows i = 4 g + j (j = 0..3), then 16 + 4 g + j where
 *            qp > 16, of group g < 4, m_k = (s_0 + s_1) + (s_2 + s_3)
 *   l_k    = fmaf(-0.5, m_k, c[k]); c (K) fp32 = log pi_k - sum log diag L_k - (q / 2) log 2 pi, rounded once
 *   L_c    = mx + logf(sum expf(l_k - mx)), mx = max l_k, over the components k of class c in ascending k (a class without a
 *            component: -inf); L_all: the same over all k < K;  r_k = expf(l_k - mx) / sum_j expf(l_j - mx) over all j < K in
 *            ascending j: exp(l_k - L_all), and exactly 1 / n among n identical components
 *   hpri_band_gmm_score  x: the zero-padded channels-last fp32 batch (pixels, cs) hpri_band_assign takes, read as pixels / plane
 *                        images of `plane` pixels; classes: K ints in HOST memory.  Outputs, each may be NULL but not all (one that is
 *                        not asked for is not touched): loglik (images, C, plane) fp32 = L_c; logit (pixels) fp32 = L_1 - L_0, C == 2
 *                        only, not clamped; labels (pixels) uint8 = the lowest c < C with L_c == max, < C for every input; resp
 *                        (images, K, plane) fp32 = r_k; nll (pixels) fp32 = -L_all.  One pass; weight and A stay in LDS (a tile of 64
 *                        pixels beside them, 32 where both do not fit); nothing of size pixels x K q leaves the workgroup.
 *   hpri_band_gmm_sums   over the selected pixels of the listed slots (the leading arguments of hpri_band_cluster_sums), with
 *                        e_k = fp32(z - means[k]) (means (K, qp) fp32): *count (int64); N[k] = sum r_k; S[k*qp + i] = sum r_k e_k[i];
 *                        Q[(k*qp + i)*qp + j] = sum r_k e_k[i] e_k[j]; *LL = sum L_all (fp64; entries with i or j >= q: 0).
 *     Summation, as hpri_band_cluster_sums: inside a run of hpri_band_fp32_run pixels every sum is the fp32 chain
 *     acc = fmaf(fp32(r_k X[i]), X[j], acc) from 0 over ALL the run's pixels in ascending order (v_mfma_f32_32x32x2_f32, k = pixel),
 *     X = (e_k[0..q-1], 1): Q = (i, j), S = (i, q), N = (q, q); at q == 32, N = fmaf(r_k, 1, acc), S[i] = fmaf(fp32(r_k e_k[i]), 1, acc)
 *     for i < 31 and S[31] = fmaf(r_k, e_k[31], acc).  A pixel that is not selected has r_k = 0.  Runs go into
 *     hpri_band_gmm_parts() = 256 fp64 partials in run order, a finishing kernel adds those in ascending order; L_all is added in fp64
 *     per pixel slot of a chunk, as zmin there.  No floating-point atomic.  workspace: hpri_band_gmm_workspace_bytes(cs, q, K) bytes,
 *     16-byte aligned; a pure function of its arguments (0 for a cs, q or K the pass does not take).
 * Argument errors (a null pointer, a size <= 0, pixels % plane != 0, a bad cs, q, K or C, a class outside [0, C), logit with C != 2, no
 * output at all, a select or dtype out of range, a selection without masks, a short workspace, a misaligned pointer) return -1
 * before any launch. */
int hpri_band_gmm_max_components(void);
int hpri_band_gmm_max_dims(void);
int hpri_band_gmm_parts(void);
size_t hpri_band_gmm_workspace_bytes(int cs, int q, int K);
int hpri_band_gmm_score(const float* x, long long pixels, long long plane, int cs, const float* pivot, const float* weight, int q,
                        const float* A, const float* a, const float* c, const int* classes, int K, int C, float* loglik, float* logit,
                        unsigned char* labels, float* resp, float* nll, hipStream_t stream);
int hpri_band_gmm_sums(const void* cache, int cache_dtype, int slots, int Hs, int Ws, int cs, const unsigned char* masks,
                       const int* slot_table, int n, int select, const float* pivot, const float* weight, int q, const float* A,
                       const float* a, const float* c, const float* means, int K, void* workspace, size_t workspace_bytes,
                       long long* count, double* N, double* S, double* Q, double* LL, hipStream_t stream);

/* ---- spectral unmixing: abundance maps and ATGP endmembers (unmix.hip; hyperpri_amd/unmix.py) ------------------------------------
 * The linear mixing model x ~ E a with M <= hpri_band_unmix_max_members (8) endmembers E (C, M).  The host fits in fp64 and rounds
 * once: E = Q R, the thin QR with a positive diagonal of R.  x: the zero-padded channels-last fp32 batch (pixels, cs) of
 * hpri_band_detect (cs % 8 == 0, cs <= hpri_band_max_cs); basis: the rows of Q^T as fp32, zero-padded to (16, cs); members: E^T as fp32,
 * (M, cs) with zero pad columns; tri: 2 M M doubles, R (row-major, upper triangular) and then G = R^T R.  Per pixel
 *   1. y[m] = fmaf(basis[m][cs-1], x[cs-1], ... fmaf(basis[m][0], x[0], 0)), m < M   (v_mfma_f32_16x16x4_f32: bitwise this chain)
 *   2. in fp64: b = R^T y, and a minimises |y - R a|^2 = 2 (1/2 a^T G a - b^T a) + |y|^2 under the mode
 *        0 ucls  no constraint: G a = b, one Cholesky solve
 *        1 scls  sum a = 1:  a = u - lambda v,  G u = b,  G v = 1,  lambda = (sum u - 1) / sum v
 *        2 ncls  a >= 0            3 fcls  both
 *      Modes 2 and 3: the active-set rule of Lawson and Hanson with the equality carried through.
 *        start     ncls: S = {}, a = 0.  fcls: S = {j}, a = e_j, j = argmax_m (b[m] - G[m][m] / 2), the lowest index of a tie.
 *        sub-solve s = the minimiser on the support S, zero elsewhere (fcls: with lambda from the two solves above restricted to S;
 *                  ncls: lambda = 0).  A variable outside S has the identity's row and column and a zero right-hand side.
 *        feasible  (s[i] > 0 for every i in S): a = s, w = b - G a - lambda, j = argmax over i not in S of w[i] (the lowest index of
 *                  a tie); stop unless w[j] > tau = 2^-40 max_m G[m][m] max(1, max_m |y[m]|); else j joins S.
 *        otherwise alpha = min over {i in S: s[i] <= 0} of a[i] / (a[i] - s[i]) (0 where a[i] == 0); a <- a + alpha (s - a); every i
 *                  that attains alpha, and every i whose a[i] is not positive afterwards, leaves S and is set to exactly 0.
 *        cap       at most `cap` sub-solves (0: 3 M).  A pixel that would need another keeps its current feasible a and adds one to
 *                  capped[0] (unsigned 64-bit, ACCUMULATED with integer atomics; capped: 4 words, the others are left alone).
 *   3. abundances[m * pixels + p] = (float) a[m]: M planes.
 *   4. rmse (pixels), may be NULL: r[c] = fmaf(-members[M-1][c], a32[M-1], ... fmaf(-members[0][c], a32[0], x[c])) from the rounded
 *      abundances, s = fmaf(r[c], r[c], s) from 0, ascending c over cs, rmse = sqrtf(s / C).
 *   5. value (pixels), may be NULL: log(p) - log1p(-p) of p = clamp(f, 2^-24, 1 - 2^-24), f the fp32 sum, ascending m from 0, of a32[m]
 *      over the members whose bit is set in `foreground` (the clamp and the logit of hpri_band_detect).
 * No floating-point atomic; the result of a pixel depends neither on the pixel count, nor on the grid, nor on its place in a tile:
 * identical arguments give identical bits.
 *   hpri_band_extreme  one step of ATGP over the selected pixels of the listed slots (the leading arguments of hpri_band_gram, fp32
 *                      and fp16 caches).  basis: K <= 8 orthonormal fp32 rows, zero-padded to (16, cs) (may be NULL with K == 0).  Per
 *                      pixel y[k] as in 1., r[c] = fmaf(-basis[K-1][c], y[K-1], ... fmaf(-basis[0][c], y[0], x[c])), v = fmaf(r[c],
 *                      r[c], v) from 0, ascending c over cs (K == 0: the squared norm).  value[0] = the largest v, position[0] = e *
 *                      Hs * Ws + the pixel inside the slot, e the list entry; between equal v the lowest position; -1 when no pixel
 *                      is selected (a NaN never wins).  Per-workgroup (v, position) partials in the workspace, then one fixed-order
 *                      pick by the same total order: the result does not depend on the grid.  workspace:
 *                      hpri_band_extreme_workspace_bytes() bytes, 16-byte aligned; a pure host query, a constant.
 * Argument errors (a null pointer, a size <= 0, cs % 8 != 0 or beyond hpri_band_max_cs, M outside [1, 8], C outside [M, cs], a mode
 * outside [0, 3], a negative cap, a foreground bit beyond M, K outside [0, 8], a select or dtype out of range, a selection without
 * masks, a workspace that is too small, a misaligned pointer) return -1 before any launch. */
int hpri_band_unmix_max_members(void);
int hpri_band_unmix(const float* x, long long pixels, int cs, int C, const float* basis, const float* members, const double* tri,
                    int M, int mode, int cap, int foreground, float* abundances, float* rmse, float* value,
                    unsigned long long* capped, hipStream_t stream);
size_t hpri_band_extreme_workspace_bytes(void);
int hpri_band_extreme(const void* cache, int cache_dtype, int slots, int Hs, int Ws, int cs, const unsigned char* masks,
                      const int* slot_table, int n, int select, const float* basis, int K, void* workspace, size_t workspace_bytes,
                      float* value, long long* position, hipStream_t stream);

/* ---- guided filter: edge-preserving smoothing of score maps (guided.hip; hyperpri_amd/guided.py) ----------------------------------
 * The guided filter of He, Sun and Tang with a K-channel guide, 1 <= K <= hpri_guided_max_guides (3), for T >= 1 maps on one frame.
 * guide: fp32 channels-last (N, H, W, gs), K <= gs; the first K channels are read (gs = 1: a plain plane; a 16-byte aligned buffer with
 * gs % 4 == 0 is read in quads).  maps and out: fp32 planes (N, T, H, W).  1 <= radius <= hpri_guided_max_radius (8), eps > 0 (an fp32
 * value, used as a double).  The window of a pixel is the (2 radius + 1)^2 square clipped to the image, n the number of its in-image
 * pixels; nothing outside the image contributes.  Every window is walked row by row, its pixels inside a row from left to right.
 *   hpri_guided_coeffs  stage 1, per pixel k and map, centred on k itself so that no mean is subtracted from a moment:
 *       dI_j[a] = I_j[a] - I_k[a],  dp_j = p_j - p_k                                            fp32, j over the window of k
 *       S1[a] += dI_j[a],  S2[a][b] = fmaf(dI_j[a], dI_j[b], S2[a][b]) (a <= b),  s += dp_j,  Sp[a] = fmaf(dI_j[a], dp_j, Sp[a])
 *                                                                                               fp32 from 0, in the window's order
 *       in fp64, no contraction: m[a] = S1[a] / n;  A[a][b] = S2[a][b] / n - m[a] m[b], plus eps on the diagonal;  sn = s / n;
 *       c[a] = Sp[a] / n - m[a] sn;  a = A^-1 c.  K = 1: a = c / A, one division.  K > 1: the Cholesky factor column by column
 *       (L[j][j] = sqrt(A[j][j] - L[j][0]^2 - ...), L[i][j] = (A[i][j] - L[i][0] L[j][0] - ...) / L[j][j], subtractions in ascending
 *       order), z[i] = (c[i] - L[i][0] z[0] - ...) / L[i][i] ascending i, then a[i] = (z[i] - L[i+1][i] a[i+1] - ...) / L[i][i]
 *       descending i.
 *       workspace, fp32 (N, T, 2K+1, H, W):  planes 0 .. K-1: a;  K .. 2K-1: mI[a] = I_k[a] + m[a];  2K: mp = p_k + sn; each the fp64
 *       value rounded once.  A and mI do not depend on the map; a map's planes do not depend on T.
 *   hpri_guided_apply   stage 2, per pixel i and map:  t_k = fmaf(a_k[K-1], I_i[K-1] - mI_k[K-1], ... fmaf(a_k[0], I_i[0] - mI_k[0],
 *       mp_k)),  q = (t_k summed in fp32 from 0 over the window of i, in its order) / (float) n.  (The line through the window's own
 *       mean, never mean(a) . I + mean(b): the same reason as the centring.)
 *   domain 0 (linear): maps are taken and written as they are.  domain 1 (prob): stage 1 reads p = sigmoid(z) of the stored logits z
 *       (1 / (1 + exp(-|z|)), or exp(-|z|) times that for z < 0), stage 2 writes log(c) - log1p(-c) of c = clamp(q, 2^-24, 1 - 2^-24),
 *       the clamp and the logit of hpri_band_detect and hpri_band_unmix.
 * Both launches work on tiles of hpri_guided_tile_h x hpri_guided_tile_w pixels with a halo of radius in LDS, one lane a pixel; stage 1
 * takes the maps in groups of four.  No atomics: the result of a pixel depends on its neighbourhood and its distance to the image
 * borders, not on N, T, the grid or its place in a tile; identical arguments give identical bits.
 * workspace: hpri_guided_workspace_bytes(N, T, H, W, K) = 4 N T (2K+1) H W bytes (0 for sizes outside the limits: H W < 2^31,
 * N T H W < 2^40), 4-byte aligned; a pure host query.  Argument errors (a null pointer, a size < 1, K outside [1, 3], gs < K, a radius
 * outside [1, 8], eps not positive and finite, a domain other than 0 or 1, a workspace that is too small, a misaligned pointer) return
 * -1 before any launch. */
int hpri_guided_max_radius(void);
int hpri_guided_max_guides(void);
int hpri_guided_tile_h(void);
int hpri_guided_tile_w(void);
size_t hpri_guided_workspace_bytes(int N, int T, int H, int W, int K);
int hpri_guided_coeffs(const float* guide, int gs, int K, const float* maps, int N, int T, int H, int W, int radius, float eps,
                       int domain, void* workspace, size_t workspace_bytes, hipStream_t stream);
int hpri_guided_apply(const float* guide, int gs, int K, int N, int T, int H, int W, int radius, int domain, const void* workspace,
                      size_t workspace_bytes, float* out, hipStream_t stream);

/* ---- dense CRF: windowed mean-field refinement of score maps (crf.hip; hyperpri_amd/crf.py) ---------------------------------------
 * Mean-field inference in the fully connected CRF of Kraehenbuehl and Koltun restricted to a (2 radius + 1)^2 window (the convolutional
 * CRF of Teichmann and Cipolla), exact inside the window.  Forward only.
 *   unary   fp32 logits (N, C, H, W), 2 <= C <= hpri_crf_max_classes (8); binary = 1 (C must be 2): fp32 logits z (N, H, W), DEFINED as
 *           the two-class problem U = (0, z).
 *   guide   fp32 channels-last (N, H, W, gs), the first K channels are read, 0 <= K <= hpri_crf_max_guides (3), K <= gs (the layouts of
 *           hpri_guided_coeffs).  K = 0: no guide (the pointer may be NULL), and then w_a must be 0.
 *   1 <= radius <= hpri_crf_max_radius (8), 1 <= iterations <= hpri_crf_max_iterations (16).
 *   host constants, made in fp64 and rounded once to fp32 (hyperpri_amd.crf.crf_tables), host memory:
 *           ta[d] = exp(-d^2 / (2 theta_alpha^2)), tg[d] = exp(-d^2 / (2 theta_gamma^2)) for d = 0 .. radius (1 everywhere for an
 *           infinite theta), b = 1 / (2 theta_beta^2) > 0; weights w_a, w_s >= 0, finite.
 *   compat  NULL: Potts, mu(l, l') = -[l = l'].  Else a host-side fp32 C x C matrix, row-major, finite.
 * Per image, all in fp32 in this order:
 *   Q^0 = softmax(U);  softmax(L): e_l = expf(L_l - max L), the e_l summed in class order from the first, then Q_l = e_l / sum.
 *   for t = 1 .. iterations, per pixel i: the neighbours j = i + (dy, dx), dy ascending from -radius, dx ascending inside a row, the
 *   centre (0, 0) skipped; a neighbour outside the image contributes +0.0 (its Q is +0.0), so a pixel's result depends only on its
 *   neighbourhood and its distance to the borders.  Per neighbour:
 *       s = fmaf(dI_c, dI_c, s) from 0 over c = 0 .. K-1 ascending,  dI_c = I_j,c - I_i,c;   e = expf(-(s * b))   (K = 0: e = 1)
 *       ga = (w_a * ta[|dy|]) * ta[|dx|],  gs_ = (w_s * tg[|dy|]) * tg[|dx|], each product rounded;   k = fmaf(ga, e, gs_)
 *       M_l = fmaf(k, Q^(t-1)_j(l), M_l) from 0, for every class l
 *   m_l = M_l / (float)(n - 1), n the in-image pixels of the clipped window (its extents on the two axes multiplied); n = 1: m_l = 0.
 *   (The centre is skipped because a pixel's own belief is no message to itself -- mean field sums over j != i; n - 1 is the number of
 *   messages, so that w_a and w_s mean the same at a border, in a corner and inside.)
 *   L_l = U_l - p_l,  p_l = fmaf(mu(l, l'), m_l', p_l) from 0 over l' ascending;  Potts: L_l = U_l + m_l (the same value).
 *   Q^t = softmax(L).
 *   output 0 (logit): out = the last L, (N, C, H, W); binary: out = L_1 - L_0 (one fp32 subtraction), (N, H, W).
 *   output 1 (prob):  out = Q^iterations, (N, C, H, W); binary: Q_1, (N, H, W).
 * One launch per iteration -- no other launch, no host synchronisation, no upload: the tables, mu and the scalars are kernel arguments --
 * over two ping-pong copies of Q in workspace: hpri_crf_workspace_bytes(N, C, H, W) = 8 N C H W bytes (0 for sizes outside the limits:
 * C in [2, 8], H W < 2^31, N C H W < 2^40), 4-byte aligned, a pure host query; not touched (may be NULL) with iterations = 1.  A workgroup
 * owns a tile of hpri_crf_tile_h x hpri_crf_tile_w pixels, one lane a pixel, with the halo of the guide and of all C planes of Q in LDS;
 * the first launch forms softmax(U) while it fills LDS.  The kernel weights k are recomputed every iteration.  No atomics: the result
 * of a pixel depends on its neighbourhood and its distance to the image borders, not on N, the grid, the tile or its place in a tile;
 * identical arguments give identical bits.  Argument errors (a null pointer, a size < 1, C outside [2, 8], binary with C != 2, K outside
 * [0, 3], gs < K, a radius outside [1, 8], iterations outside [1, 16], a table that does not start at 1 or rises or is negative or NaN,
 * a weight that is negative or not finite, b not positive and finite with K > 0, w_a != 0 with K = 0, a compat entry that is not finite,
 * an output other than 0 or 1, a workspace that is too small, a misaligned pointer) return -1 before any launch. */
int hpri_crf_max_radius(void);
int hpri_crf_max_classes(void);
int hpri_crf_max_guides(void);
int hpri_crf_max_iterations(void);
int hpri_crf_tile_h(void);
int hpri_crf_tile_w(void);
size_t hpri_crf_workspace_bytes(int N, int C, int H, int W);
int hpri_dense_crf(const float* unary, int binary, const float* guide, int gs, int K, int N, int C, int H, int W, int radius,
                   int iterations, const float* ta, const float* tg, float b, float w_a, float w_s, const float* compat, int output,
                   void* workspace, size_t workspace_bytes, float* out, hipStream_t stream);

/* ---- trainable dense CRF: the backward through the mean-field iterations (crf.hip, crf_grad.hip; hyperpri_amd/crf.py) --------------
 * Gradients through hpri_dense_crf's T iterations to the unaries, w_a, w_s and the compatibility matrix mu; not to the guide or thetas.
 * In both entries w_a, w_s and compat are DEVICE pointers (one fp32 each; compat a row-major C x C matrix, NULL: Potts; w_a may be NULL
 * and is not read with K = 0), so that a training step has no host synchronisation and no upload.  They accept any finite value -- a
 * negative weight is a repulsive CRF, not an error; the host cannot check device values, a NaN or an infinity there gives NaN.
 *
 * hpri_dense_crf_train_forward: hpri_dense_crf's kernel and launches with the weights read from device memory; out is bit-identical to
 * hpri_dense_crf at the same parameter values.  keep = 0: nothing is kept, workspace as for hpri_dense_crf (two ping-pong plane sets,
 * untouched with iterations = 1).  keep = 1: workspace is the training workspace below, and iteration t writes Q^t into slot t - 1 of
 * its stack where the plain forward ping-pongs -- Q^1 .. Q^(T-1), and under output 1 also Q^T (both planes of a binary input; out is
 * then a device copy of it, of plane 1 for a binary input); there is no second pass over the window.  Q^0 = softmax(U) and, under output 0, nothing of iteration T is needed by the backward.
 *
 * hpri_crf_train_workspace_bytes(N, C, H, W, T): 8 T tiles (2 + C^2) + 4 (T + 2) N C H W bytes, tiles = N ceil(H / 16) ceil(W / 32): the
 * fp64 partial sums, the stack of T plane sets and two plane sets of gL; 8-byte aligned; 0 for sizes outside the limits or T outside
 * [1, 16]; a pure host query.  The backward reads the stack the forward of the same arguments wrote into the same workspace.
 *
 * hpri_dense_crf_backward, with g = grad_out in the output's shape; all fp32 in this order unless said otherwise:
 *   gL^T:  output 0: gL^T = g; binary: (-g, +g).  output 1: gv = g (binary: gv = (0, g)), d = fmaf(Q^T_l, gv_l, d) from 0 over l ascending,
 *          gL^T_l = Q^T_l * (gv_l - d).
 *   for t = T .. 1, per pixel j (one launch per t, the forward's tile, one lane a pixel):
 *     gU_j:  t = T: gU_j = gL^T_j; else gU_j = gU_j + gL^t_j; at t = 1 then gU_j = gU_j + gL^0_j -- the order t = T, T-1, .., 0, by the lane
 *            that owns the pixel.
 *     b_i(l) = gL^t_i(l) / (float)(n_i - 1), n_i the in-image pixels of pixel i's clipped window; n_i = 1: 0; i outside the image: +0.0.
 *     the window of j in the forward's order (dy ascending, dx ascending inside a row, the centre skipped), i = j + (dy, dx):
 *       s, e as the forward forms them for pixel j and neighbour i (s from dI_c = I_i,c - I_j,c; e = expf(-(s * b)))
 *       ka = (ta[|dy|] * ta[|dx|]) * e,  ps = tg[|dy|] * tg[|dx|], each product rounded
 *       GA_l = fmaf(ka, b_i(l), GA_l),  GS_l = fmaf(ps, b_i(l), GS_l) from 0       (K = 0: no GA and no exponential)
 *     H_l = fmaf(w_a, GA_l, w_s * GS_l)   (K = 0: H_l = w_s * GS_l)
 *     gQ_l' = -p_l',  p_l' = fmaf(mu(l, l'), H_l, p_l') from 0 over l ascending   (mu transposed; Potts: gQ_l = H_l)
 *     with Q = Q^(t-1)_j (t = 1: softmax(U_j) formed again, the forward's bits):
 *       d = fmaf(Q_l, gQ_l, d) from 0 over l ascending;   gL^(t-1)_j(l) = Q_l * (gQ_l - d)
 *     parameters, per pixel: a_l' = -(fmaf(mu(l, l'), GA_l, .) over l ascending) (Potts: GA_l'), A_j = fmaf(a_l', Q_l', A_j) from 0 over l'
 *       ascending; S_j likewise from GS; M_j(l, l') = -(H_l * Q_l').
 *   grad_w_a = sum A_j, grad_w_s = sum S_j, grad_compat(l, l') = sum M_j(l, l') over all pixels and iterations: the family's reduction
 *   rule -- every per-pixel value converted to fp64, summed per TILE AND ITERATION by the halving tree over the tile's 512 lanes (a lane
 *   outside the image adds 0), then one block of 256 threads adds the partial sums in fp64: the T x tiles sums taken in the order t
 *   descending from T, the tile index (image, tile row, tile column) ascending inside a t; thread j adds entries j, j + 256, .. of that
 *   sequence in that order, the halving tree adds the 256 threads' sums, and the total rounds once to fp32.  The sums do not depend on
 *   the grid.  No floating-point atomic anywhere.
 *   grad_unary in the unaries' shape (binary: gz = gU_1, (N, H, W)); grad_w_a, grad_w_s (one fp32 each) and grad_compat (C x C) are device
 *   pointers, each may be NULL (not wanted); grad_compat needs compat, grad_w_a needs K > 0.
 * Identical arguments give identical bits.  LDS: 8 KB for the sums and the forward's planes, with b where it holds Q.  Argument errors (as hpri_dense_crf's, without the checks of the weights' values; a workspace that is too small or
 * not 8-byte aligned; grad_compat without compat; grad_w_a with K = 0) return -1 before any launch. */
size_t hpri_crf_train_workspace_bytes(int N, int C, int H, int W, int T);
int hpri_dense_crf_train_forward(const float* unary, int binary, const float* guide, int gs, int K, int N, int C, int H, int W, int radius,
                                 int iterations, const float* ta, const float* tg, float b, const float* w_a, const float* w_s,
                                 const float* compat, int output, int keep, void* workspace, size_t workspace_bytes, float* out,
                                 hipStream_t stream);
int hpri_dense_crf_backward(const float* grad_out, const float* unary, int binary, const float* guide, int gs, int K, int N, int C, int H,
                            int W, int radius, int iterations, const float* ta, const float* tg, float b, const float* w_a,
                            const float* w_s, const float* compat, int output, void* workspace, size_t workspace_bytes, float* grad_unary,
                            float* grad_w_a, float* grad_w_s, float* grad_compat, hipStream_t stream);

/* ---- ridge filter: multi-scale Hessian vesselness for thin roots (ridge.hip; hyperpri_amd/ridge.py) -----------------------------
 * A scale-normalised Hessian ridge measure (after Frangi et al. and Sato et al.) of T >= 1 fp32 planes on an (N, H, W) frame.  Pixel
 * (y, x) of plane t of image n is maps[n image_stride + t plane_stride + (y W + x) pixel_stride] (strides in floats, pixel_stride >= 1):
 * a contiguous (N, T, H, W) tensor has (T H W, H W, 1), the first T channels of a channels-last buffer of cs channels (H W cs, 1, cs);
 * nothing else of the buffer is read.  domain 0 (linear) reads the values as they are, domain 1 (prob) sigmoid(z) of stored logits z,
 * as hpri_guided_coeffs does.
 *   scales  1 <= S <= hpri_ridge_max_scales (8).  Per scale s the host passes radii[s] = R in [1, hpri_ridge_max_radius (12)], the
 *       fp32 value sigma2[s] and three half-kernels taps[(3 s + k) 12 + j - 1], k = 0, 1, 2 for g0, g1, g2 and j = 1 .. R (host
 *       memory, S x 3 x 12 floats, entries past R ignored).  hyperpri_amd.ridge.ridge_taps makes them in fp64 and rounds them once:
 *       w(x) = exp(-x^2 / 2 sigma^2), g0 = w / (1 + 2 sum w), g1 = x w / (2 sum x^2 w), g2 = q / sum x^2 q with q = (x^2 / sigma^4 -
 *       1 / sigma^2) w, R = ceil(3 sigma).  There is no centre tap: every pass works on differences from its own centre, the implied
 *       centre taps are 1 - 2 sum g0, 0 and -2 sum g2, so the kernels are exactly unit-sum (g0) or zero-sum (g1, g2) whatever the
 *       rounding of the taps.
 *   borders  half-sample symmetric reflection rho (d c b a | a b c d), of period 2n: defined on images smaller than R, down to 1 x 1.
 *   row pass  per pixel and scale, fp32 from +0.0, c = I[y, x], for j = 1 .. R:
 *       dp = I[y, rho(x+j)] - c,  dm = I[y, rho(x-j)] - c
 *       s0 = fmaf(g0[j], dp + dm, s0),  r1 = fmaf(g1[j], dp - dm, r1),  r2 = fmaf(g2[j], dp + dm, r2)
 *       (s0 is the smoothed plane minus the pixel; the pixel is never added back into an fp32 value)
 *   column pass  fp32 from +0.0, for i = 1 .. R, + and - the rows rho(y + i) and rho(y - i) at the same x, c the pixel's own row:
 *       axx = fmaf(g0[i], (r2+ - r2c) + (r2- - r2c), axx),   Hxx = (r2c + axx) sigma2
 *       axy = fmaf(g1[i], r1+ - r1-, axy),                   Hxy = axy sigma2
 *       ayy = fmaf(g2[i], e+ + e-, ayy),                     Hyy = ayy sigma2,    e+- = (I+- - Ic) + (s0+- - s0c)
 *       (Lindeberg's normalisation, gamma = 1: one product by sigma2 each)
 *   measure  per pixel and scale in fp64 from the three fp32 values, no contraction:  mu = (Hxx + Hyy) / 2,
 *       d = sqrt(((Hxx - Hyy) / 2)^2 + Hxy^2).  polarity 0 (bright): l2 = mu - d, l1 = mu + d, gate mu < 0; 1 (dark): l2 = mu + d,
 *       l1 = mu - d, gate mu > 0; 2 (both): mu >= 0 gives l2 = mu + d, l1 = mu - d, else l2 = mu - d, l1 = mu + d, no gate.
 *       measure 0 (frangi): V = exp(-(l1 / l2)^2 / (2 beta^2)) (-expm1(-(l1^2 + l2^2) / (2 c^2))) where the gate holds and l2 != 0,
 *       else 0.  measure 1 (sato): V = max(-l2, 0), max(l2, 0), |l2| for bright, dark, both.
 *   across scales  the maximum of V over the scales in the order given; scale (may be NULL) receives the index of the first scale
 *       that attains it.  output 0 (value): out = (float) V.  output 1 (logit): out = logf(p) - log1pf(-p) of p = clamp((float) P,
 *       2^-24, 1 - 2^-24), P = V (frangi) or V / (V + c) (sato): the clamp and the logit of hpri_band_detect and hpri_band_unmix.
 *       hessian (may be NULL): fp32 (N, T, S, 3, H, W), Hxx | Hxy | Hyy.
 * One launch: a workgroup owns a tile of hpri_ridge_tile_h x hpri_ridge_tile_w pixels, one lane a pixel, with the reflected halo of
 * the largest R in LDS.  No atomics: the result of a pixel depends on its neighbourhood and its distance to the image borders, not on
 * N, T, the other maps, the grid, the tile or its place in a tile; a scale's Hessian planes do not depend on the other scales;
 * identical arguments give identical bits.  A constant plane of any magnitude gives H = +0.0 and V = 0; negating the input negates H.
 * Argument errors (a null maps, taps, radii, sigma2 or out, a size < 1, N T H W >= 2^31, S outside [1, 8], a radius outside [1, 12],
 * a pixel stride < 1 or a negative stride, a non-finite tap, sigma2, beta or c, beta <= 0 or c <= 0, a code out of range, a misaligned
 * pointer) return -1 before any launch. */
int hpri_ridge_max_scales(void);
int hpri_ridge_max_radius(void);
int hpri_ridge_tile_h(void);
int hpri_ridge_tile_w(void);
int hpri_ridge_filter(const float* maps, long long image_stride, long long plane_stride, long long pixel_stride, int N, int T, int H,
                      int W, const float* taps, const int* radii, const float* sigma2, int S, float beta, float c, int polarity,
                      int measure, int domain, int output, float* out, unsigned char* scale, float* hessian, hipStream_t stream);

/* ---- soft skeletons and the centerline loss clDice (skeleton.hip; hyperpri_amd/trainer.py, distance.py) ------------------------
 * fp32 planes (N, h, w), contiguous, values meant to lie in [0, 1]; 0 <= iters <= hpri_soft_skeleton_max_iters (32).
 *   E(I)[u] = min over the in-image part of the plus neighbourhood {N, W, C, E, S} of u,  D(I)[u] = max over the in-image 3x3
 *   I_0 = p,  I_{j+1} = E(I_j),  d_j = I_j - D(I_{j+1}),  S_0 = relu(d_0),  S_j = S_{j-1} + relu(fma(-S_{j-1}, d_j, d_j))
 *   hpri_soft_skeleton_fwd  S = S_iters in ONE launch (tiles of hpri_soft_skeleton_tile pixels a side with a halo of iters + 2 in
 *                           LDS: hpri_soft_skeleton_lds_bytes(iters)).  saved != NULL: also I_1 .. I_{iters+1} and S_0 ..
 *                           S_{iters-1}, hpri_soft_skeleton_saved_floats = (2 iters + 1) N h w floats, for the backward.
 *   hpri_soft_skeleton_bwd  grad_p from grad_S, one launch per level j = iters .. 0:  gd = gS (1 - S_{j-1}) [t_j > 0],
 *                           gS <- gS (1 - d_j [t_j > 0]),  gI_j = gd + route_E(gE + route_D(-gd)),  gE <- gI_j.  A min or a max
 *                           sends its gradient to its FIRST optimum in scan order (E: N, W, C, E, S; D: the window row by row);
 *                           the routes are gathers summed in a fixed order in fp64: no floating-point atomic, bit-reproducible,
 *                           independent of the tiling.  workspace: hpri_soft_skeleton_workspace_floats = 4 N h w floats.
 *   hpri_cldice_fwd         Sp = soft_skeleton(sigmoid(logits)) and Sy = soft_skeleton(target) in one launch (p = sigmoid(logits)
 *                           written once; Sp may be NULL), with per group (an image with per_image, else the batch)
 *                           tprec = (sum Sp y + s) / (sum Sp + s), tsens = (sum Sy p + s) / (sum Sy + s), cl = 1 - 2 tprec tsens /
 *                           (tprec + tsens) from fp64 partial sums per workgroup in a fixed order and a one-workgroup finalize:
 *                           loss[0] = weight * mean_g cl_g (+ base_weight * base_loss[0] with base_loss != NULL, a device scalar);
 *                           terms[0..2] = mean cl, mean tprec, mean tsens; state: 3 doubles per group (a, b, c below).  A ratio
 *                           with a zero denominator is 0; tprec + tsens == 0 gives cl = 1 and zero coefficients.
 *   hpri_cldice_bwd         dlogits = grad_out * (skeleton-backward(a_g y + b_g) + c_g Sy) * sigmoid(x) * sigmoid(-x) in iters + 1
 *                           launches, no host round trip; grad_out: device scalar, NULL = 1; grad_base != NULL: grad_base[0] =
 *                           grad_out * base_weight.
 *   hpri_centerline_counts  counts[4n .. 4n+3] += |skel(P)|, |skel(P) & T|, |skel(T)|, |skel(T) & P| of image n over uint8 maps
 *                           (non-zero = set).  ACCUMULATED.
 * The size functions are pure host functions.  Argument errors (a null pointer, a size <= 0, N > 32767, a side > 2^30, N*h*w >= 2^31, iters
 * outside [0, 32], smooth < 0, a buffer that is too small) return -1 before any launch. */
int hpri_soft_skeleton_tile(void);
int hpri_soft_skeleton_max_iters(void);
size_t hpri_soft_skeleton_lds_bytes(int iters);
size_t hpri_soft_skeleton_saved_floats(int N, int h, int w, int iters);
size_t hpri_soft_skeleton_workspace_floats(int N, int h, int w);
size_t hpri_cldice_workspace_doubles(int N, int h, int w);
size_t hpri_cldice_state_doubles(int N, int per_image);
int hpri_soft_skeleton_fwd(const float* p, int N, int h, int w, int iters, float* S, float* saved, size_t saved_floats,
                           hipStream_t stream);
int hpri_soft_skeleton_bwd(const float* p, const float* saved, size_t saved_floats, const float* grad_S, int N, int h, int w,
                           int iters, float* grad_p, float* workspace, size_t ws_floats, hipStream_t stream);
int hpri_cldice_fwd(const float* logits, const float* target, int N, int h, int w, int iters, float smooth, int per_image,
                    float weight, const float* base_loss, float base_weight, float* p, float* Sp, float* Sy, float* saved,
                    size_t saved_floats, float* loss, float* terms, double* state, size_t state_doubles, double* workspace,
                    size_t ws_doubles, hipStream_t stream);
int hpri_cldice_bwd(const float* logits, const float* target, const float* p, const float* Sy, const float* saved,
                    size_t saved_floats, int N, int h, int w, int iters, int per_image, const double* state, size_t state_doubles,
                    const float* grad_out, float base_weight, float* grad_base, float* dlogits, float* workspace, size_t ws_floats,
                    hipStream_t stream);
int hpri_centerline_counts(const unsigned char* skel_pred, const unsigned char* skel_truth, const unsigned char* pred,
                           const unsigned char* truth, int N, long long per_image, int* counts, hipStream_t stream);

/* ---- device sort, the Lovasz hinge and the ranking metrics (sort.hip; hyperpri_amd/losses.py, metrics.py) --------------------------
 *   hpri_sort_keys_f32      G groups of L fp32 keys, contiguous (G, L): perm[g][r] = the index inside group g of the key of rank r,
 *                           bit for bit the indices of torch.sort(keys[g], descending, stable=True): by numeric value, NaN above
 *                           +inf, -0.0 equal to +0.0, denormals in their order, ties in ascending index order; descending == 0:
 *                           ascending (NaN last).  sorted_keys != NULL: also the keys in that order, their original bits gathered
 *                           through perm.  A stable LSD radix sort, four 8-bit digits of an order-preserving uint32: a histogram
 *                           launch, then per digit count / scan / scatter launches over tiles of hpri_sort_tile keys and a final
 *                           gather -- 15 launches with the clearing of the histograms, for every size.  The rank inside a tile comes
 *                           from wave ballots and a fixed scan, never from the order in which atomics land: bit-reproducible.  A
 *                           digit that is the same in all keys of a group is skipped by the workgroups themselves (no host read).
 *                           The only synchronisation between workgroups is the kernel boundary.  1 <= G <= 65535, L >= 1,
 *                           G * L < 2^31; workspace: hpri_sort_workspace_bytes(G, L) bytes, 16-byte aligned.
 *   hpri_lovasz_hinge_fwd   the Lovasz hinge (Berman et al., CVPR 2018) of fp32 logits and a fp32 target, N images of per_image
 *                           pixels; a group is an image (per_image_groups != 0) or the batch.  s = target >= 0.5 ? +1 : -1,
 *                           e = 1 - logit * s (fp32), the group's pixels in the order of e descending (the sort above), G1 = the
 *                           group's positives, at rank r: P_r = positives among ranks 0 .. r, I_r = G1 - P_r, U_r = G1 + r + 1 - P_r,
 *                           w_r = 1 / U_r for a positive and I_r / ((U_r - 1) U_r) for a negative pixel (G1 == 0: w_0 = 1, else 0),
 *                           in fp64 from the integer counts; loss[0] = mean over the groups of sum_r relu(e_r) w_r (fp64 partial
 *                           sums in a fixed order); coef[i] = -s_i w_rank(i) / groups where e_i > 0 and 0 elsewhere, rounded once.
 *                           use_ignore != 0: pixels whose target equals ignore_index count for nothing (a group without any other
 *                           pixel contributes 0).  17 launches, no host synchronisation.  workspace:
 *                           hpri_lovasz_hinge_workspace_bytes(N, per_image, per_image_groups) bytes, 16-byte aligned.
 *   hpri_lovasz_hinge_bwd   dlogits[i] = coef[i] * grad_out[0] (grad_out: device scalar, NULL = 1): one launch.
 *   hpri_ranking_sums       one descending sort of n scores, then over the runs of equal scores (tp, fp: the positives and negatives
 *                           down to the end of a run, p_run and q_run: those of the run; target_kind 0: fp32, 1: uint8, non-zero
 *                           = positive): out[0] = the bits of the fp64 sum of p_run tp / (tp + fp) (average precision times the
 *                           positives P), out[1] = the sum of p_run (2 (N - fp) + q_run) (ROC AUC times 2 P N, N the negatives:
 *                           Mann-Whitney with ties counted half, an exact integer), out[2] = P.  17 launches.  workspace:
 *                           hpri_ranking_workspace_bytes(n) bytes, 16-byte aligned; n < 2^31.
 * The size functions and hpri_sort_tile are pure host functions (0 for sizes outside the limits).  A null pointer or a size outside the
 * limits returns -1, a workspace that is too small -3, both before any launch. */
int hpri_sort_tile(void);
size_t hpri_sort_workspace_bytes(int G, int L);
int hpri_sort_keys_f32(const float* keys, int G, int L, int descending, int* perm, float* sorted_keys, void* workspace,
                       size_t workspace_bytes, hipStream_t stream);
size_t hpri_lovasz_hinge_workspace_bytes(int N, long long per_image, int per_image_groups);
int hpri_lovasz_hinge_fwd(const float* logits, const float* target, int N, long long per_image, int per_image_groups, int use_ignore,
                          int ignore_index, float* loss, float* coef, void* workspace, size_t workspace_bytes, hipStream_t stream);
int hpri_lovasz_hinge_bwd(const float* coef, long long n, const float* grad_out, float* dlogits, hipStream_t stream);
size_t hpri_ranking_workspace_bytes(long long n);
int hpri_ranking_sums(const float* scores, const void* target, int target_kind, long long n, unsigned long long* out, void* workspace,
                      size_t workspace_bytes, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* HYPERPRI_HIP_H */
