/* vaegan_hip.h -- C ABI of libvaegan_hip.so: the MI355X (gfx950) kernels behind
 * the CelebA 64x64 beta-VAE-GAN training iteration.
 *
 * The reference (RicoFio/disentangle_mlp) has no FFI of its own: its hot path is
 * Python torch.nn modules (models/model.py) whose arithmetic is dispatched to
 * ATen.  Each entry point below replaces one ATen call site of that path; the
 * citation next to it is the reference line that reaches the op.  A maintainer
 * binds them with ctypes (INTEGRATION.md shows the stub) -- no torch types
 * cross this boundary, only device pointers, sizes and a hipStream_t.
 *
 * Conventions
 *   - all tensors are contiguous fp32, NCHW (activations), (Cout,Cin,5,5)
 *     (Conv2d weights), (Cin,Cout,5,5) (ConvTranspose2d weights), (out,in)
 *     (Linear weights): exactly the reference's state_dict layouts.
 *   - kernels never allocate; outputs / workspaces are caller-owned device
 *     buffers; `stream` is a hipStream_t (NULL = default stream).
 *   - every function returns 0 on success, VG_ERR_BAD_ARG (-1) for a rejected
 *     argument, VG_ERR_WORKSPACE (-2) for a too-small workspace, otherwise the
 *     hipError_t of the failed launch.  No exceptions cross the ABI.
 *   - launches are asynchronous, hold no global mutable state and are
 *     HIP-graph capturable.  (The tile-forcing knobs tests and tuning scripts use are process-globals,
 *     so they exist only in a second build of the same sources, libvaegan_hip_tuning.so, compiled with
 *     -DVG_TUNING: the section at the end of this header.)
 */
#ifndef VAEGAN_HIP_H
#define VAEGAN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VG_ERR_BAD_ARG (-1)
#define VG_ERR_WORKSPACE (-2)

/* activation codes for the fused BatchNorm kernels */
#define VG_ACT_NONE 0
#define VG_ACT_RELU 1  /* nn.ReLU          model.py:452,463,493 */
#define VG_ACT_LRELU 2 /* nn.LeakyReLU(.2) model.py:391,404     */

/* ABI version of this header: bumped on every incompatible change of a signature, of a packed-filter layout or of a
 * workspace contract.  vg_version() returns the value the library was built with; a binding must refuse a library
 * whose version is not the header's (the .so files are build products that travel with the working tree: a stale one
 * still exports every old symbol).  3: round 3.  4: round 4 (fp16 planes: VG_PLANES_F16, the *_amax arguments).
 * 6: vg_conv_general_* (the general forward convolution).  7: vg_adam_step_checked / vg_adam_step_dev_checked.
 * Entry points that are only ADDED (the four of csrc/fid_front.hip; vg_bn_eval_coeffs, vg_bn_eval_act_bwd;
 * vg_adam_step_ema, vg_adam_step_dev_ema; vg_grad_sumsq_partials, vg_grad_sumsq_multi, vg_grad_clip_finalize,
 * vg_adam_step_clip, vg_adam_step_dev_clip; vg_adam_prepare_dev, vg_adam_step_decay, vg_adam_step_dev_decay,
 * vg_reparam_kl_fwd_dev, vg_reparam_kl_bwd_dev; vg_adam_step_dev_ema_dev; the five vg_reparam_tc_* of
 * csrc/reparam_tc.hip; vg_linear_wgrad_adam, vg_linear_wgrad_adam_dev; the five vg_reparam_dip_* of
 * csrc/reparam_dip.hip; the three vg_agg_posterior_* of csrc/agg_posterior.hip; the five vg_reparam_mmd_* of
 * csrc/reparam_mmd.hip; the four vg_pair_* of csrc/pair_dist.hip; the two vg_recon_quality* of
 * csrc/recon_quality.hip; the five vg_reparam_klc_* of csrc/reparam_klc.hip; the three vg_diff_augment_* of
 * csrc/diff_augment.hip; the seven of csrc/factor_vae.hip; the three of csrc/gan_loss.hip;
 * vg_diff_augment_fwd_dev, vg_diff_augment_bwd_dev, vg_ada_update) change
 * nothing an existing caller sees and keep the version: a binding that needs them and finds a library without them
 * fails at the symbol lookup, as loudly. */
#define VG_ABI_VERSION 7
int vg_version(void);

/* ---- 5x5 convolutions, padding 2, stride 1 or 2 ----------------------------
 * y[B,Cout,OH,OW] = conv2d(x[B,Cin,H,W], w[Cout,Cin,5,5]) + bias;  OH=(H-1)/s+1.
 * nn.Conv2d forward: model.py:450,453,456 (encoder), :389,392,395,398 (discr.).
 * Also the input gradient of vg_convT5x5_fwd.  bias may be NULL. */
int vg_conv5x5_fwd(const float* x, const float* w, const float* bias, float* y,
                   int B, int Cin, int H, int W, int Cout, int stride, void* stream);

/* y[B,Cout,s*H,s*W] = conv_transpose2d(x[B,Cin,H,W], w[Cin,Cout,5,5], stride s,
 * padding 2, output_padding s-1) + bias.  nn.ConvTranspose2d forward with the
 * literal output_size of model.py:558-564 (deconv1..4, :495-507).  Also the
 * input gradient of vg_conv5x5_fwd (then w is the Conv2d weight [Cout,Cin,5,5]
 * read as [Cin_T=Cout, Cout_T=Cin], H*s must equal the conv input size). */
int vg_convT5x5_fwd(const float* x, const float* w, const float* bias, float* y,
                    int B, int Cin, int H, int W, int Cout, int stride, void* stream);

/* Pre-packed filters.  The implicit-GEMM kernels run fastest when the filter slab of a K
 * chunk is a verbatim 16-byte copy: vg_conv5x5_pack rewrites a weight tensor once per
 * weight version into [parity class][ci][tap][cout] (cout innermost, zero padded to a
 * multiple of 128 output / 8 input channels), vg_conv5x5_fwd_packed /
 * vg_convT5x5_fwd_packed consume it.  On the same tile variant the results are bit-identical
 * to the plain entry points (same K order); the tile heuristics of the two may differ.
 *   transposed = 0: w is [Cout,Cin,5,5], for vg_conv5x5_fwd_packed (stride ignored);
 *   transposed = 1: w is [Cin,Cout,5,5], for vg_convT5x5_fwd_packed with the SAME stride
 *                   (the stride-2 kernel walks the 4 output-parity classes separately).
 * `packed` holds vg_conv5x5_packed_floats(Cout, Cin) floats, 16-byte aligned. */
size_t vg_conv5x5_packed_floats(int Cout, int Cin);
int vg_conv5x5_pack(const float* w, float* packed, int Cout, int Cin, int transposed, int stride,
                    void* stream);
int vg_conv5x5_fwd_packed(const float* x, const float* packed, const float* bias, float* y,
                          int B, int Cin, int H, int W, int Cout, int stride, void* stream);
int vg_convT5x5_fwd_packed(const float* x, const float* packed, const float* bias, float* y,
                           int B, int Cin, int H, int W, int Cout, int stride, void* stream);
/* vg_conv5x5_fwd_packed that also leaves the statistics of its output for the BatchNorm that follows
 * (vg_conv_fusion.stats semantics: [slot][Cout][2] partial sums; vg_bn_finalize_stats consumes them) -- the
 * 3-channel first layers (model.py:389-390, 450-451), whose 67 MB / 34 MB outputs would otherwise be read once
 * more only to be summed.  `stats` holds vg_conv5x5_fwd_packed_stats_floats(...) floats. */
size_t vg_conv5x5_fwd_packed_stats_floats(int B, int Cin, int H, int W, int Cout, int stride);
int vg_conv5x5_fwd_packed_stats(const float* x, const float* packed, const float* bias, float* y,
                                int B, int Cin, int H, int W, int Cout, int stride,
                                float* stats, size_t stats_floats, void* stream);

/* Split arithmetics of vg_conv5x5_fwd / vg_convT5x5_fwd: every fp32 operand is split
 * into `planes` 16-bit values and the products whose plane indices sum to < planes are evaluated on the 16-bit
 * MFMA (v_mfma_f32_32x32x16_bf16 / _f16) with fp32 accumulation:
 *   planes = 2 | VG_PLANES_F16   fp16 hi/lo = 11 + 11 significand bits (residual <= 2^-24 relative), 3 MFMAs per product
 *               ("fp16x3"): fp32-equivalent (4e-7..6e-7 against fp64) at half the matrix work of bf16x6.  fp16 has 5
 *               exponent bits: each operand tensor is multiplied by an exact power of two taken from an UPPER BOUND of
 *               its largest magnitude, which the caller supplies in device memory (vg_conv_fusion.in_amax, the *_amax
 *               arguments below; vg_absmax* compute one, vg_bn_act_bwd / vg_bn_finalize_stats / vg_affine_act emit one
 *               on their way out); the scales are undone on the fp32 accumulators.  A bound that is too small overflows
 *               fp16 (inf / NaN in the output, never a silently wrong number); elements more than 2^-16 below the bound
 *               keep fewer than 22 bits: their error is bounded by 2^-40 of the bound.  THE PRODUCT DEFAULT of the
 *               Python layer.
 *   planes = 3  bf16 hi/mid/lo = the whole 24-bit mantissa, 6 MFMAs per product ("bf16x6"): every dropped
 *               term is below 2^-24 -- fp32-equivalent at any dynamic range (4e-7..9e-7 against fp64; the exact
 *               fp32-input MFMA kernels above: 5e-7..1e-6).  Opt-in; the 3-channel edge kernels always use it.
 *   planes = 2  bf16 hi/lo, 3 MFMAs per product ("bf16x3"): ~4.5e-6 relative error; opt-in.
 * Requires Cin % 16 == 0.  `packed` holds vg_conv5x5_packed_bf16split_bytes(Cout, Cin, planes) bytes
 * (16-byte aligned), written by vg_conv5x5_pack_bf16split once per weight version:
 *   transposed = 0: from w[Cout,Cin,5,5] for vg_conv5x5_fwd_bf16split with the SAME stride (the stride-2
 *                   kernel pairs taps differently from the stride-1 one);
 *   transposed = 1: from w[Cin,Cout,5,5] for vg_convT5x5_fwd_bf16split with the SAME stride.
 * Stride 2 runs on the 8-wavefront kernel of conv_ring.hip (both MFMA operands from LDS, the filter through a
 * global_load_lds DMA ring); layers whose tile grid would leave CUs idle split their input channels over
 * workgroups and sum the partial outputs in a fixed order: query the workspace (0 for most shapes). */
/* Fused BatchNorm around a stride-2 split-bf16 convolution (replaces the separate statistics and
 * normalise passes of F.batch_norm reached from model.py:451-458, 496-505, 390-400):
 *   in_scale / in_shift / in_act: the input is read as act(x * in_scale[c] + in_shift[c]) -- the producing layer's
 *     train-mode BatchNorm (scale = gamma * invstd, shift = beta - mean * scale) and activation (VG_ACT_*) applied
 *     while the patch is staged; zero padding pads the activated tensor.  NULL: the input is used as it is.
 *   stats: per-channel partial sums of THIS layer's output, [slot][Cout][2] floats (sum y, sum y^2 over the slot's
 *     pixels, bias included), `stats_floats` = vg_conv*_stats_floats(...) of them; vg_bn_finalize_stats turns them
 *     into the next BatchNorm's coefficients.  NULL: none.
 * vg_conv5x5_bf16split_fusable says whether a layer's kernel takes a non-empty fusion; *_stats_floats returns 0 for
 * layers that cannot emit statistics (other kernels, K-split layers). */
#define VG_PLANES_F16 0x100 /* flag of the `planes` arguments: the planes are IEEE half precision (with 2 planes only) */
typedef struct vg_conv_fusion {
  const float* in_scale;
  const float* in_shift;
  int in_act;
  float* stats;
  size_t stats_floats;
  /* fp16 planes (required then, ignored otherwise; not a fusion: every kernel of the family takes it): in_amax[0], DEVICE
   * memory, >= the largest |value| of the input as the kernel reads it (after in_scale / in_shift / in_act) */
  const float* in_amax;
} vg_conv_fusion;
int vg_conv5x5_bf16split_fusable(int transposed, int Cin, int Cout, int stride);
/* (the tile a layer runs on, and with it the slot count and the K split, depends on the arithmetic: two fp16 planes leave
 * room in the LDS for larger tiles) */
size_t vg_conv5x5_fwd_bf16split_stats_floats(int B, int Cin, int H, int W, int Cout, int stride, int planes);
size_t vg_convT5x5_fwd_bf16split_stats_floats(int B, int Cin, int H, int W, int Cout, int stride, int planes);
size_t vg_conv5x5_packed_bf16split_bytes(int Cout, int Cin, int planes);
/* w_amax (fp16 planes; NULL otherwise): w_amax[0] >= max |w|, DEVICE memory (vg_absmax / vg_absmax_multi); the pack
 * keeps the inverse of the filter's scale in a 16-byte trailer for the convolution's epilogue */
int vg_conv5x5_pack_bf16split(const float* w, void* packed, int Cout, int Cin, int transposed, int stride,
                           int planes, const float* w_amax, void* stream);
/* The same for several filters in one launch (`entries` is a HOST array; 24 filters per kernel launch): what a
 * training iteration calls after each optimizer step for every filter that step has changed. */
typedef struct {
  const float* w;
  void* packed;
  int Cout, Cin, transposed, stride;
  const float* w_amax; /* as vg_conv5x5_pack_bf16split */
} VgPackEntry;
int vg_conv5x5_pack_bf16split_multi(const VgPackEntry* entries, int count, int planes, void* stream);
size_t vg_conv5x5_fwd_bf16split_workspace_bytes(int B, int Cin, int H, int W, int Cout, int stride, int planes);
int vg_conv5x5_fwd_bf16split(const float* x, const void* packed, const float* bias, float* y,
                          int B, int Cin, int H, int W, int Cout, int stride, int planes,
                          void* workspace, size_t workspace_bytes, const vg_conv_fusion* fuse, void* stream);
size_t vg_convT5x5_fwd_bf16split_workspace_bytes(int B, int Cin, int H, int W, int Cout, int stride, int planes);
int vg_convT5x5_fwd_bf16split(const float* x, const void* packed, const float* bias, float* y,
                           int B, int Cin, int H, int W, int Cout, int stride, int planes,
                           void* workspace, size_t workspace_bytes, const vg_conv_fusion* fuse, void* stream);
/* Stride-1 transposed convolution 32 -> (1..3) channels in the same arithmetic, on the PLAIN filter w (Cin, Cout, 5, 5):
 * the decoder's last layer (ConvTranspose2d(32, 3, 5, 1, 2), /root/reference/models/model.py:507) and the data
 * gradient of the discriminator's first layer (model.py:389).  One pass over x with the filter resident in registers
 * (csrc/conv_thin_mfma.hip).  in_scale / in_shift / in_act: x is read as act(x * in_scale[ci] + in_shift[ci]) (the
 * producing layer's BatchNorm + activation, vg_conv_fusion semantics); NULL: as it is.  _ok: 1 when the shape is taken
 * (Cin == 32, Cout <= 3, W a multiple of 16 up to 128); otherwise use vg_convT5x5_fwd. */
int vg_convT5x5_s1_thin_bf16split_ok(int Cin, int H, int W, int Cout);
int vg_convT5x5_s1_thin_bf16split(const float* x, const float* w, const float* bias, float* y, int B, int Cin,
                                  int H, int W, int Cout, int planes, const float* in_scale, const float* in_shift,
                                  int in_act, void* stream);
/* Convolution from 1..3 input channels in the same arithmetic, on the PLAIN filter w (Cout, Cin, 5, 5): the first
 * layers of the discriminator (Conv2d(3, 32, 5, 1, 2), model.py:389) and the encoder (Conv2d(3, 64, 5, 2, 2),
 * model.py:450).  One write pass over y with the filter resident in registers (csrc/conv_thin_fwd.hip); `stats`
 * (or NULL) receives the per-channel partial sums of y for the BatchNorm that follows, vg_conv_fusion.stats layout
 * ([slot][Cout][2], vg_conv5x5_thin_bf16split_stats_floats(...) floats, slots = floats / (2 Cout)).  _ok: 1 when the
 * shape is taken (output width a multiple of 32, (output width / 32) * ceil(Cout / 32) <= 8); otherwise use
 * vg_conv5x5_fwd. */
int vg_conv5x5_thin_bf16split_ok(int Cin, int H, int W, int Cout, int stride);
size_t vg_conv5x5_thin_bf16split_stats_floats(int B, int Cin, int H, int W, int Cout, int stride);
int vg_conv5x5_thin_bf16split(const float* x, const float* w, const float* bias, float* y, int B, int Cin, int H, int W,
                              int Cout, int stride, int planes, float* stats, size_t stats_floats, void* stream);
/* ... and its weight gradient (dw (Cout, Cin, 5, 5), Cin <= 3, Cout <= 64; also the decoder's ConvTranspose2d(32, 3)
 * with the roles of x and gy swapped): one read pass over gy, x split once per workgroup into shifted bf16 plane
 * copies in LDS (csrc/conv_thin_wgrad.hip).  The workspace query returns 0 for shapes it does not take (output width
 * not a multiple of 16, ...): use vg_conv5x5_wgrad then.  workspace: 16-byte aligned; gy 16-byte aligned. */
size_t vg_conv5x5_thin_wgrad_bf16split_workspace_bytes(int B, int Cin, int H, int W, int Cout, int stride, int planes);
int vg_conv5x5_thin_wgrad_bf16split(const float* x, const float* gy, float* dw, int B, int Cin, int H, int W, int Cout,
                                    int stride, int planes, void* workspace, size_t workspace_bytes,
                                    /* gy read as act(gy * gy_scale[c] + gy_shift[c]) (NULL, NULL, 0: plain): the weight
                                     * gradient of ConvTranspose2d(32, 3) passes the layer's input here, the train-mode
                                     * BatchNorm + ReLU of its producer (model.py:505) is applied on load */
                                    const float* gy_scale, const float* gy_shift, int gy_act,
                                    int accumulate /* dw += (see vg_conv5x5_wgrad) */, void* stream);
/* vg_conv5x5_wgrad in the same arithmetic.  The reduction runs over images in groups of 16: gy is re-laid
 * batch-innermost inside the call (B zero-padded to a multiple of 16), x is staged straight from NCHW; needs
 * OW % 8 == 0 -- the workspace query returns 0 for shapes it does not take (use vg_conv5x5_wgrad).
 * workspace: 16-byte aligned. */
size_t vg_conv5x5_wgrad_bf16split_workspace_bytes(int B, int Cin, int H, int W, int Cout, int stride, int planes);
int vg_conv5x5_wgrad_bf16split(const float* x, const float* gy, float* dw, int B, int Cin, int H, int W,
                            int Cout, int stride, int planes, void* workspace, size_t workspace_bytes,
                            const float* in_scale, const float* in_shift, int in_act, int affine_on_gy,
                            /* fp16 planes (NULL otherwise): x_amax[0] >= max |x|, gy_amax[0] >= max |gy|, each of the
                             * operand as the kernel reads it (after the affine + activation where one applies), DEVICE */
                            const float* x_amax, const float* gy_amax,
                            int accumulate /* dw += (see vg_conv5x5_wgrad) */, void* stream);
/* in_scale / in_shift / in_act: one operand is read as act(v * scale[c] + shift[c]) (vg_conv_fusion semantics) --
 * x (Cin coefficients) when affine_on_gy == 0, gy (Cout coefficients; the weight gradient of a transposed
 * convolution passes the layer's input there) otherwise.  NULL, NULL, 0, 0: both operands as they are. */

/* ---- Linear layers in the fp16x3 arithmetic (csrc/gemm_split.hip) -------------------------------------------------
 * C[m][n] = sum_k A(m,k) * B(n,k) (+ bias[n]), A(m,k) = A[m*a_row_stride + k*a_k_stride], B alike; C row-major [M][N].
 * Per operand either the reduction index is contiguous (k stride 1; row stride % 4 == 0, 16-byte aligned base) or the
 * row index is (row stride 1).  K % 32 == 0.  One entry point serves nn.Linear (/root/reference/models/model.py:460-471,
 * 402-408, 490-492; replaces torch.nn.functional.linear and the two backward GEMMs autograd derives from it): forward
 * y = x W^T (A = x, B = W), data gradient gx = gy W (A = gy, B = W with b_row_stride = 1, b_k_stride = in_features),
 * weight gradient gW = gy^T x (A = gy with a_row_stride = 1, B = x with b_row_stride = 1; K = batch).  Arithmetic: the
 * convolutions' fp16x3 (planes = 2 | VG_PLANES_F16 above) -- a_amax[0] >= max |A|, b_amax[0] >= max |B|, DEVICE memory.
 * Short output grids split the reduction over workgroups: query the workspace (partial tiles, summed in a fixed order;
 * no atomics -- results are reproducible run to run). */
size_t vg_gemm_nt_f16x3_workspace_bytes(int M, int N, int K);
int vg_gemm_nt_f16x3(const float* A, const float* B, const float* bias, float* C, int M, int N, int K,
                     long a_row_stride, long a_k_stride, long b_row_stride, long b_k_stride,
                     const float* a_amax, const float* b_amax, void* workspace, size_t workspace_bytes, void* stream);
/* Grouped form: 1 <= groups <= VG_GEMM_MAX_GROUPS activations against ONE B (the passes of a network over unchanged
 * weights): C[g] = A[g] B^T (+ bias) for every g, B streamed, scaled and split once per launch.  A, C and a_amax are HOST
 * arrays of `groups` device pointers; M, N, K, the four strides, bias, B and b_amax are shared.  Every C[g] is bit for
 * bit what vg_gemm_nt_f16x3 returns for A[g] alone (same tiling, K split, MFMA order and slab sum).  Workspace: the
 * groups' slabs one after another (groups x the single call's). */
#define VG_GEMM_MAX_GROUPS 3
size_t vg_gemm_nt_f16x3_grouped_workspace_bytes(int groups, int M, int N, int K);
int vg_gemm_nt_f16x3_grouped(int groups, const float* const* A, const float* B, const float* bias, float* const* C,
                             int M, int N, int K, long a_row_stride, long a_k_stride, long b_row_stride,
                             long b_k_stride, const float* const* a_amax, const float* b_amax, void* workspace,
                             size_t workspace_bytes, void* stream);

/* ---- general forward convolution, fp16x3 (csrc/conv_general.hip) ---------------------------------------------------
 * y[b][co][oh][ow] = act(sum_{ci,kh,kw} x[b][ci][oh*stride_h + kh - pad_h][ow*stride_w + kw - pad_w] * w[co][ci][kh][kw]
 *                        + bias[co]),   OH = (H + 2 pad_h - KH) / stride_h + 1, OW alike; act = ReLU when relu != 0.
 * The convolutions of the FID Inception network (/root/reference/scoring/inception.py:16-310: BasicConv2d with its
 * eval-mode BatchNorm folded into w and bias; replaces torch.nn.functional.conv2d + batch_norm + relu): KH, KW in 1..15,
 * strides 1 or 2, paddings 0..15, H, W <= 8192, any channel counts.  Inference only; no im2col buffer exists.
 * Arithmetic: planes = 2 | VG_PLANES_F16 above -- x_amax[0] >= max |x| in DEVICE memory, the filter's bound goes into
 * the pack.  A bound that is too small gives inf / NaN, never a silently wrong number.
 *   packed: vg_conv_general_packed_bytes(Cout, Cin, KH, KW) bytes, 16-byte aligned, written by vg_conv_general_pack
 *     once per weight version from w[Cout][Cin][KH][KW] and w_amax[0] >= max |w| (DEVICE).  Layout, in 16-byte units,
 *     with K = Cin KH KW, nsteps = ceil(K / 32), CoutP = Cout rounded up to 128:
 *       [nsteps][2 planes hi, lo][4 k-blocks][CoutP] x 8 fp16: reduction index k = (kh KW + kw) Cin + ci, scaled, split,
 *           zero beyond K and Cout                                              nsteps * 8 * CoutP units
 *       [nsteps * 32] x (int32 ci, int32 kh << 16 | kw): what k addresses        nsteps * 16 units
 *       trailer: the inverse of the filter's power-of-two scale (one float)      1 unit
 *   y, y_image_stride: image b of the output starts at y + b * y_image_stride (floats, >= Cout OH OW) and is
 *     [Cout][OH][OW] contiguous: y may point at a channel slice of a larger NCHW tensor (the concatenated output of an
 *     Inception block), the other channels are not touched.
 *   y_amax (may be NULL): max |y| is added to y_amax[0] (atomic maximum on the bit pattern, DEVICE memory, zeroed by the
 *     caller): the next layer's x_amax; several launches may add into one slot.
 *   bias may be NULL.  The reduction is never split over workgroups: no workspace, results reproducible bit for bit.
 * Sizes whose 32-bit indices (an element of one input or output image, an output pixel of the batch) would overflow
 * are rejected with VG_ERR_BAD_ARG. */
size_t vg_conv_general_packed_bytes(int Cout, int Cin, int KH, int KW);
int vg_conv_general_pack(const float* w, void* packed, int Cout, int Cin, int KH, int KW, const float* w_amax,
                         void* stream);
int vg_conv_general_fwd(const float* x, const void* packed, const float* bias, float* y, int B, int Cin, int H, int W,
                        int Cout, int KH, int KW, int stride_h, int stride_w, int pad_h, int pad_w, long y_image_stride,
                        int relu, const float* x_amax, float* y_amax, void* stream);

/* Bounds for the fp16 planes: amax[0] = max(amax[0], max |x|) over n floats -- an atomic maximum on the bit pattern
 * (order-independent; a NaN in x ends up in the bound); the caller zeroes amax[0] first (or keeps accumulating a bound
 * over several tensors).  _affine: over act(x[b][c][hw] * scale[c] + shift[c]) (vg_conv_fusion semantics).  _multi: many
 * tensors in one launch (`entries` is a HOST array) -- the filters an optimizer step has changed. */
int vg_absmax(const float* x, size_t n, float* amax, void* stream);
int vg_absmax_affine(const float* x, const float* scale, const float* shift, int act, int B, int C, int HW, float* amax,
                     void* stream);
typedef struct {
  const float* x;
  size_t n;
  float* amax;
} VgAbsmaxEntry;
int vg_absmax_multi(const VgAbsmaxEntry* entries, int count, void* stream);

/* dw[Cout,Cin,5,5] = sum_{b,oh,ow} gy[b,co,oh,ow] * x[b,ci,s*oh+kh-2,s*ow+kw-2].
 * Weight gradient of nn.Conv2d (autograd of model.py:450...; new_betavaegan.py:103,121)
 * and, with the roles swapped (x := gy_T, gy := x_T), of nn.ConvTranspose2d.
 * x is [B,Cin,H,W], gy is [B,Cout,OH,OW] with OH=(H-1)/s+1.  Deterministic:
 * split-K partial slabs in `workspace` are summed in a fixed order. */
size_t vg_conv5x5_wgrad_workspace_bytes(int B, int Cin, int H, int W, int Cout, int stride);
int vg_conv5x5_wgrad(const float* x, const float* gy, float* dw, int B, int Cin, int H, int W,
                     int Cout, int stride, void* workspace, size_t workspace_bytes,
                     /* accumulate != 0: the result is ADDED to what dw holds (in the final fixed-order slab sum) -- a layer
                      * applied twice before one backward (D on the real and the generated batch, the decoder on the prior
                      * sample and the reconstruction: new_betavaegan.py:99-121, 144-163) gets its second weight gradient
                      * without the separate addition autograd would launch; fp addition is commutative: same bits */
                     int accumulate, void* stream);

/* out[c] = sum_{b,hw} g[b,c,hw]   (bias gradient of the convolutions).
 * workspace >= vg_bn_workspace_bytes(C). */
int vg_channel_sum(const float* g, float* out, int B, int C, int HW,
                   void* workspace, size_t workspace_bytes, void* stream);

/* ---- train-mode BatchNorm (+ReLU / LeakyReLU(0.2)) --------------------------
 * x is [B,C,HW] (HW=1 for BatchNorm1d).  Batch statistics (biased variance,
 * eps), y = act(gamma*(x-mean)*invstd + beta); running_mean/var updated with
 * `momentum` (unbiased variance), as F.batch_norm(training=True) does.
 * nn.BatchNorm2d/1d in train mode: model.py:451-458,462,468,492,496-505,390-400
 * (the reference never calls .eval()).  save_mean / save_invstd ([C]) are kept
 * for the backward.  running_mean / running_var may be NULL.
 * y_amax (may be NULL; ignored for HW == 1): max |y| is added to y_amax[0] (atomic maximum, DEVICE memory, zeroed by the
 * caller) -- the bound the fp16-plane consumers of y (a convolution, vg_gemm_nt_f16x3) scale it by.
 * workspace >= vg_bn_workspace_bytes(C). */
size_t vg_bn_workspace_bytes(int C);
int vg_bn_act_fwd(const float* x, const float* gamma, const float* beta, float* y,
                  float* running_mean, float* running_var, float* save_mean, float* save_invstd,
                  int B, int C, int HW, float eps, float momentum, int act, float* y_amax,
                  void* workspace, size_t workspace_bytes, void* stream);
/* gx, dgamma, dbeta from gy, the saved x and statistics (the activation mask is
 * recomputed from x, bit-identically to the forward). gx must not alias gy. */
int vg_bn_act_bwd(const float* gy, const float* x, const float* gamma, const float* beta,
                  const float* save_mean, const float* save_invstd,
                  float* gx, float* dgamma, float* dbeta,
                  int B, int C, int HW, int act,
                  int accumulate_param_grads /* dgamma, dbeta += (a layer used twice before one backward) */,
                  float* gx_amax /* NULL, or DEVICE: gx_amax[0] = max(gx_amax[0], max |gx|) -- see vg_absmax */,
                  void* workspace, size_t workspace_bytes, void* stream);
/* Fused-BatchNorm helpers.  vg_bn_finalize_stats turns a convolution's statistics slots
 * ([nslots][C][2] floats: vg_conv_fusion.stats) into the coefficients of the train-mode BatchNorm that follows it
 * -- save_mean / save_invstd for backward, scale = gamma * invstd and shift = beta - mean * scale for the consumer's
 * in_scale / in_shift -- and updates the running statistics (momentum, unbiased variance) as vg_bn_act_fwd does;
 * count = B * H * W.  vg_bn_stats does the same from a pass over x (layers whose producer cannot emit statistics).
 * vg_affine_act materialises y = act(x * scale[c] + shift[c]) (16-byte accesses when HW % 4 == 0) for consumers that cannot apply the
 * coefficients while they load.
 * act_amax (NULL, or DEVICE, zeroed by the caller): receives an upper bound of max |act(x * scale + shift)| over the
 * tensor, for the scale / shift written -- from the sums alone, without a pass over x: |x - mean| <= sigma sqrt(count - 1)
 * for the EXACT sigma, which is bounded from the computed variance plus the sums' rounding error (relative to sum x^2;
 * in each statistics slot no term may go through more than 16 roundings: a short fma chain and a butterfly), so that
 * a variance lost to cancellation (|mean| >> sigma) cannot push the data above the bound.  For accurate sums it is
 * ~|gamma| sqrt(count) + |beta|.  What an fp16-plane convolution that applies scale / shift on load needs as
 * vg_conv_fusion.in_amax.
 * y_amax of vg_affine_act: the exact max |y| (see vg_absmax). */
int vg_bn_finalize_stats(const float* stats, int nslots, int C, double count, const float* gamma, const float* beta,
                         float* running_mean, float* running_var, float* save_mean, float* save_invstd,
                         float* scale, float* shift, float eps, float momentum, float* act_amax,
                         void* workspace, size_t workspace_bytes, /* vg_bn_workspace_bytes(C) */ void* stream);
int vg_bn_stats(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                float* save_mean, float* save_invstd, float* scale, float* shift, int B, int C, int HW,
                float eps, float momentum, float* act_amax, void* workspace, size_t workspace_bytes, void* stream);
int vg_affine_act(const float* x, const float* scale, const float* shift, float* y, int B, int C, int HW, int act,
                  float* y_amax, void* stream);

/* ---- BatchNorm on running statistics (eval mode) -----------------------------
 * nn.BatchNorm2d / 1d after .eval(): F.batch_norm(training=False) of the modules at model.py:451-458, 462, 468, 492,
 * 496-505, 390-400 -- the reference's modules accept .eval() on the checkpoints exchanged with it; opt-in here
 * (model.enable_eval).  y = act(x * scale[c] + shift[c]) with FROZEN coefficients, applied by vg_affine_act or by the
 * consuming convolution on load (vg_conv_fusion.in_scale / in_shift), exactly as in train mode.
 * vg_bn_eval_coeffs (one launch): scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale, and
 * invstd = 1 / sqrt(running_var + eps) for the backward.  The running buffers are inputs only; nothing else is written.
 * `act`: the activation the consumer applies (validated; ReLU / LeakyReLU only shrink the bound).
 * stats / nslots / count (optional: NULL / 0 / 0): the statistics slots the producing convolution left of x
 * ([nslots][C][2]: vg_conv_fusion.stats; count = B * H * W) -- with them AND act_amax (DEVICE, zeroed by the caller) an
 * upper bound of max |act(x * scale + shift)| is added to act_amax[0] (atomic maximum), from the sums alone, no pass over
 * x: |x - m| <= sigma sqrt(count - 1) for the batch's exact mean and sigma, sigma bounded from the computed variance plus
 * the sums' rounding error as for vg_bn_finalize_stats, hence |scale x + shift| <= |scale| sigma sqrt(count - 1) +
 * |scale m + shift|.  Never below the data, also for a constant channel or a variance lost to cancellation.  Without
 * slots: coefficients only (vg_absmax_affine gives the exact bound).
 * vg_bn_eval_act_bwd: one pass over gy and the saved raw x.  gx = gy act'(scale x + shift) scale;
 * dbeta[c] = sum gy act', dgamma[c] = sum gy act' (x - mean[c]) invstd[c] (mean: the running mean the forward used).
 * dgamma / dbeta may be NULL; accumulate_param_grads, gx_amax, HW == 1, the fixed summation order and the 16-byte
 * accesses (HW % 4 == 0 and 16-byte aligned gy, x, gx only) as vg_bn_act_bwd.  A NaN gradient stays a NaN; a NaN
 * pre-activation under ReLU / LeakyReLU gives a NaN gradient.  B = 1 is an ordinary input.
 * workspace >= vg_bn_workspace_bytes(C) (needed only for parameter gradients of channels cut into several slices). */
int vg_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                      float* scale, float* shift, float* invstd, int C, float eps, int act,
                      const float* stats, int nslots, double count, float* act_amax, void* stream);
int vg_bn_eval_act_bwd(const float* gy, const float* x, const float* scale, const float* shift,
                       const float* mean, const float* invstd, float* gx, float* dgamma, float* dbeta,
                       int B, int C, int HW, int act, int accumulate_param_grads, float* gx_amax,
                       void* workspace, size_t workspace_bytes, void* stream);


/* ---- elementwise activations ------------------------------------------------
 * LeakyReLU(0.2) after lth_features (model.py:404), tanh after deconv4
 * (model.py:509,565), both with an optional per-channel bias add fused in:
 * y = act(x + bias[c]) for x [B,C,HW]; bias may be NULL. */
int vg_bias_act_fwd(const float* x, const float* bias, float* y, int B, int C, int HW, int act_kind, void* stream);
/* gx_amax (may be NULL): max |gx| is added to gx_amax[0] (atomic maximum; DEVICE memory, zeroed by the caller) -- the bound an
 * fp16-plane consumer of gx (the Linear layers' backward GEMMs) scales it by */
int vg_act_bwd(const float* gy, const float* y, float* gx, size_t n, int act_kind, float* gx_amax, void* stream);
#define VG_EW_LRELU 0
#define VG_EW_TANH 1
#define VG_EW_SIGMOID 2

/* ---- fused losses -----------------------------------------------------------
 * Loss scalars are written to device memory (no host sync). */

/* z = mu + eps*exp(logvar/2) (model.py:532-535) and
 * kl[0] = beta * (-0.5 * sum(1 + logvar - mu^2 - exp(logvar))) (new_betavaegan.py:64-65);
 * kl_rows ([B], may be NULL) gets the un-scaled per-sample KL (model.py:321). */
int vg_reparam_kl_fwd(const float* mu, const float* logvar, const float* eps, float* z, float* kl,
                      float* kl_rows, int B, int D, float beta, void* stream);
/* gmu = gz + gkl*beta*mu ; glogvar = gz*eps*0.5*exp(logvar/2) + gkl*beta*0.5*(exp(logvar)-1).
 * gz (tensor) and gkl (DEVICE scalar, the upstream gradient of kl[0]) may each be
 * NULL (treated as 0). */
int vg_reparam_kl_bwd(const float* gz, const float* mu, const float* logvar, const float* eps,
                      const float* gkl, float beta, float* gmu, float* glogvar, int B, int D, void* stream);
/* The two with beta read from DEVICE memory (beta_dev[0], fp32): a KL weight on a schedule changes between the replays
 * of an iteration captured in a HIP graph.  Same expressions -- (float)(beta * t), gkl * beta -- so the same fp32 beta
 * gives the same bits.  beta_dev == NULL is VG_ERR_BAD_ARG. */
int vg_reparam_kl_fwd_dev(const float* mu, const float* logvar, const float* eps, float* z, float* kl,
                          float* kl_rows, int B, int D, const float* beta_dev, void* stream);
int vg_reparam_kl_bwd_dev(const float* gz, const float* mu, const float* logvar, const float* eps,
                          const float* gkl, const float* beta_dev, float* gmu, float* glogvar, int B, int D,
                          void* stream);

/* ---- reparameterisation + the beta-TCVAE decomposition of the KL term (Chen et al. 2018, minibatch-weighted sampling;
 * DESIGN.md section 4.17; csrc/reparam_tc.hip).  With z_i = mu_i + eps_i*exp(logvar_i/2) and, for i, j < B, d < D,
 *   lq[i,j,d] = -0.5*(log 2pi + logvar[j,d] + (z[i,d] - mu[j,d])^2 * exp(-logvar[j,d]))
 *   lqzx_i = sum_d lq[i,i,d]       lqz_i = LSE_j(sum_d lq[i,j,d]) - log_bn       lqprod_i = sum_d (LSE_j lq[i,j,d] - log_bn)
 *   lpz_i  = sum_d -0.5*(log 2pi + z[i,d]^2)
 * the forward writes z and out4 = {loss, mi, tc, dwkl}: mi = sum_i (lqzx_i - lqz_i), tc = sum_i (lqz_i - lqprod_i),
 * dwkl = sum_i (lqprod_i - lpz_i), loss = alpha*mi + beta*tc + gamma*dwkl (sums over the batch; log_bn = log(B * dataset
 * size)), and what the backward reads instead of the pair terms: lse_joint ([B], fp64: LSE_j sum_d lq[i,j,d]) and lse_dim
 * ([B,D]: LSE_j lq[i,j,d]).  Two launches: one workgroup per sample, then one wavefront that sums the per-sample parts in
 * a fixed order.  The backward writes
 *   gmu = gloss*(Gmu + Gz) + gz      glogvar = gloss*(Glv + Gz*eps*0.5*exp(logvar/2)) + gz*eps*0.5*exp(logvar/2)
 * (Gz, Gmu, Glv: the partial derivatives of loss with z, mu, logvar taken as independent) in two launches -- the sums over
 * j in sample i's workgroup, the sums over i in workgroup j; gz (tensor) and gloss (DEVICE scalar, upstream of out4[0]) may
 * each be NULL: that term is absent (gloss == NULL is one elementwise launch).  No floating-point atomics: the same
 * inputs give the same bits.  1 <= B, D <= 1024.  `workspace`: vg_reparam_tc_workspace_bytes(B, D) bytes, 8-byte aligned
 * (the forward's content is not needed by the backward). */
size_t vg_reparam_tc_workspace_bytes(int B, int D);
int vg_reparam_tc_fwd(const float* mu, const float* logvar, const float* eps, float* z, float* out4, double* lse_joint,
                      float* lse_dim, int B, int D, float alpha, float beta, float gamma, float log_bn, void* workspace,
                      size_t workspace_bytes, void* stream);
int vg_reparam_tc_bwd(const float* gz, const float* mu, const float* logvar, const float* eps, const float* z,
                      const double* lse_joint, const float* lse_dim, const float* gloss, float alpha, float beta,
                      float gamma, float* gmu, float* glogvar, int B, int D, void* workspace, size_t workspace_bytes,
                      void* stream);
/* beta read from DEVICE memory (beta_dev[0], fp32), as vg_reparam_kl_fwd_dev: the same fp32 beta gives the same bits.
 * beta_dev == NULL is VG_ERR_BAD_ARG. */
int vg_reparam_tc_fwd_dev(const float* mu, const float* logvar, const float* eps, float* z, float* out4,
                          double* lse_joint, float* lse_dim, int B, int D, float alpha, const float* beta_dev, float gamma,
                          float log_bn, void* workspace, size_t workspace_bytes, void* stream);
int vg_reparam_tc_bwd_dev(const float* gz, const float* mu, const float* logvar, const float* eps, const float* z,
                          const double* lse_joint, const float* lse_dim, const float* gloss, float alpha,
                          const float* beta_dev, float gamma, float* gmu, float* glogvar, int B, int D, void* workspace,
                          size_t workspace_bytes, void* stream);

/* ---- reparameterisation + the DIP-VAE objectives (Kumar et al. 2018, variants I and II; DESIGN.md section 4.21;
 * csrc/reparam_dip.hip).  With z = mu + eps*exp(logvar/2) and, for b < B, i, j, d < D,
 *   kl   = -0.5*sum_{b,d}(1 + logvar - mu^2 - exp(logvar))
 *   m[d] = (1/B)*sum_b mu[b,d]        c[b,d] = mu[b,d] - m[d]
 *   C    = (1/B)*sum_b c_b c_b^T                                   variant 1  (Cov_p[mu(x)])
 *   C    = that + diag((1/B)*sum_b exp(logvar[b,:]))               variant 2  (Cov_q[z])
 *   od   = sum_{i != j} C_ij^2        dg = sum_i (C_ii - 1)^2
 * the forward writes z and out4 = {loss, kl, od, dg}, loss = beta*kl + B*(lambda_od*od + lambda_d*dg) (batch sums: loss / B
 * is the paper's objective with the paper's lambdas), and what the backward reads: cov ([D,D] fp32: C, symmetric to the
 * bit) and mean ([D] fp64: m).  Three launches: column statistics (fp64), one workgroup per 32 x 32 tile of C on or above
 * the diagonal (centred columns in LDS, fp32 FMA chains of 64 rows in a fixed order, their sums added in fp64), one
 * wavefront that sums the partials in a fixed order.  With G_ij = 2*lambda_od*C_ij (i != j), G_ii = 2*lambda_d*(C_ii - 1)
 * the backward writes
 *   gmu     = gloss*(beta*mu + 2*(c_b . G)) + gz
 *   glogvar = gloss*(beta*0.5*(exp(logvar) - 1) + [variant 2: G_dd*exp(logvar)]) + gz*eps*0.5*exp(logvar/2)
 * in one launch; gz (tensor) and gloss (DEVICE scalar, upstream of out4[0]) may each be NULL: that term is absent (gloss
 * == NULL is one elementwise launch).  No floating-point atomics: the same inputs give the same bits.  1 <= B, D <= 1024;
 * variant is 1 or 2.  `workspace`: vg_reparam_dip_workspace_bytes(B, D) bytes, 8-byte aligned (the forward's content is
 * not needed by the backward). */
size_t vg_reparam_dip_workspace_bytes(int B, int D);
int vg_reparam_dip_fwd(const float* mu, const float* logvar, const float* eps, float* z, float* out4, float* cov,
                       double* mean, int B, int D, int variant, float beta, float lambda_od, float lambda_d,
                       void* workspace, size_t workspace_bytes, void* stream);
int vg_reparam_dip_bwd(const float* gz, const float* mu, const float* logvar, const float* eps, const float* cov,
                       const double* mean, const float* gloss, int variant, float beta, float lambda_od, float lambda_d,
                       float* gmu, float* glogvar, int B, int D, void* workspace, size_t workspace_bytes, void* stream);
/* beta read from DEVICE memory (beta_dev[0], fp32), as vg_reparam_kl_fwd_dev: the same fp32 beta gives the same bits.
 * beta_dev == NULL is VG_ERR_BAD_ARG. */
int vg_reparam_dip_fwd_dev(const float* mu, const float* logvar, const float* eps, float* z, float* out4, float* cov,
                           double* mean, int B, int D, int variant, const float* beta_dev, float lambda_od,
                           float lambda_d, void* workspace, size_t workspace_bytes, void* stream);
int vg_reparam_dip_bwd_dev(const float* gz, const float* mu, const float* logvar, const float* eps, const float* cov,
                           const double* mean, const float* gloss, int variant, const float* beta_dev, float lambda_od,
                           float lambda_d, float* gmu, float* glogvar, int B, int D, void* workspace,
                           size_t workspace_bytes, void* stream);

/* ---- reparameterisation + the InfoVAE / WAE-MMD objective (Zhao et al. 2019; Tolstikhin et al. 2018; DESIGN.md section
 * 4.23; csrc/reparam_mmd.hip).  With z = mu + eps*exp(logvar/2), zp ([B,D]) draws from the prior N(0, I), d(a,b) = |a-b|^2
 * and the kernel k summed over n_bandwidths <= 8 bandwidths h_s > 0,
 *   kind 1 (rbf): k(d) = sum_s exp(-d/h_s)        kind 2 (imq): k(d) = sum_s h_s/(h_s + d)
 *   kl  = -0.5*sum_{b,d}(1 + logvar - mu^2 - exp(logvar))
 *   kzz = 1/(B(B-1))*sum_{i != j} k(z_i, z_j)     kpp = 1/(B(B-1))*sum_{i != j} k(zp_i, zp_j)     kzp = 1/B^2*sum_{i,j} k(z_i, zp_j)
 *   mmd = kzz + kpp - 2*kzp      (the unbiased U-statistic: it may be negative)
 * the forward writes z and out4 = {loss, kl, mmd, kzz}, loss = beta*kl + B*lambda_mmd*mmd (batch sums: loss / B is the
 * paper's objective with the paper's lambda), and what the backward reads: w ([2,B,B] fp32): w[0] = 4/(B(B-1))*k'(d(z_i,
 * z_j)), symmetric to the bit with a zero diagonal, and w[1] = -4/B^2*k'(d(z_i, zp_j)).  Three launches: z and the KL
 * partials (fp64), one workgroup per 32 x 32 tile of a pair matrix (zz and pp on or above the diagonal, zp in full; both
 * row blocks in LDS 64 columns at a time, every squared distance fp32 FMA chains of 16 DIFFERENCES in a fixed order, the
 * chain sums added in fp64 -- never |a|^2 + |b|^2 - 2 a.b, which cancels for close points; k and k' once per pair in
 * fp64, exp and true division), one wavefront that sums the partials in a fixed order.  With Gz_i = B*lambda_mmd*sum_j (w[0,i,j]*(z_i - z_j) + w[1,i,j]*
 * (z_i - zp_j)) the backward writes
 *   gmu     = gloss*(beta*mu + Gz) + gz
 *   glogvar = gloss*(beta*0.5*(exp(logvar) - 1) + Gz*eps*0.5*exp(logvar/2)) + gz*eps*0.5*exp(logvar/2)
 * in one launch; gz (tensor) and gloss (DEVICE scalar, upstream of out4[0]) may each be NULL: that term is absent (gloss
 * == NULL is one elementwise launch).  zp takes no gradient.  No floating-point atomics: the same inputs give the same
 * bits.  `bandwidths` is a HOST array of n_bandwidths floats, copied into the kernel arguments.  `workspace`:
 * vg_reparam_mmd_workspace_bytes(B, D) bytes (0 outside the shape range), 8-byte aligned (the forward's content is not
 * needed by the backward).  VG_ERR_BAD_ARG before any launch: a NULL pointer other than gz / gloss, B outside [2, 1024]
 * (the U-statistic has no value at B = 1), D outside [1, 1024], kind outside {1, 2}, n_bandwidths outside [1, 8], a
 * bandwidth that is not finite and > 0, a lambda_mmd that is not finite and >= 0, and -- here also VG_ERR_BAD_ARG -- a
 * workspace shorter than that. */
size_t vg_reparam_mmd_workspace_bytes(int B, int D);
int vg_reparam_mmd_fwd(const float* mu, const float* logvar, const float* eps, const float* zp, float* z, float* out4,
                       float* w, int B, int D, int kind, float beta, float lambda_mmd, const float* bandwidths,
                       int n_bandwidths, void* workspace, size_t workspace_bytes, void* stream);
int vg_reparam_mmd_bwd(const float* gz, const float* mu, const float* logvar, const float* eps, const float* z,
                       const float* zp, const float* w, const float* gloss, float beta, float lambda_mmd, float* gmu,
                       float* glogvar, int B, int D, void* workspace, size_t workspace_bytes, void* stream);
/* beta read from DEVICE memory (beta_dev[0], fp32), as vg_reparam_kl_fwd_dev: the same fp32 beta gives the same bits.
 * beta_dev == NULL is VG_ERR_BAD_ARG. */
int vg_reparam_mmd_fwd_dev(const float* mu, const float* logvar, const float* eps, const float* zp, float* z, float* out4,
                           float* w, int B, int D, int kind, const float* beta_dev, float lambda_mmd,
                           const float* bandwidths, int n_bandwidths, void* workspace, size_t workspace_bytes,
                           void* stream);
int vg_reparam_mmd_bwd_dev(const float* gz, const float* mu, const float* logvar, const float* eps, const float* z,
                           const float* zp, const float* w, const float* gloss, const float* beta_dev, float lambda_mmd,
                           float* gmu, float* glogvar, int B, int D, void* workspace, size_t workspace_bytes,
                           void* stream);

/* ---- reparameterisation + the controlled KL term: a capacity (Burgess et al. 2018; AnnealedVAE) over per-dimension
 * free bits (Kingma et al. 2016); csrc/reparam_klc.hip.  With z = mu + eps*exp(logvar/2), the
 * capacity C >= 0 (nats per sample) and the floor lambda = free_bits >= 0 (nats per dimension per sample),
 *   K[d] = -0.5*sum_b(1 + logvar - mu^2 - exp(logvar))      (fp64, fixed order)
 *   F[d] = max(K[d], B*lambda)                              (a NaN K[d] stays NaN)
 *   kl   = sum_d K[d]        T = sum_d F[d]                 (fp64, index order)
 *   above = #{d : K[d] > B*lambda}
 * the forward writes z and out4 = {loss, kl, T, above}, loss = beta*|T - B*C| (batch sums: loss / B is Burgess's term over
 * Kingma's batch-averaged floor; lambda = 0, C = 0 is the plain beta*kl), and what the backward reads and a caller may
 * want: gate ([D] fp32) = sgn(T - B*C)*[K[d] > B*lambda] in {-1, 0, +1} (sgn(0) = 0; NaN where a NaN went into T) and
 * kl_dim ([D] fp32) = K[d]/B.  Two launches: one workgroup per 64 rows x 64 columns writes z and its column sums to fixed
 * fp64 slots; ONE workgroup adds the slots in index order, applies the floor and forms the totals.  The backward writes
 *   gmu     = gloss*beta*gate[d]*mu + gz
 *   glogvar = gloss*beta*gate[d]*0.5*(exp(logvar) - 1) + gz*eps*0.5*exp(logvar/2)
 * in one elementwise launch; gz (tensor) and gloss (DEVICE scalar, upstream of out4[0]) may each be NULL: that term is
 * absent.  No floating-point atomics: the same inputs give the same bits.  `workspace`:
 * vg_reparam_klc_workspace_bytes(B, D) bytes (0 outside the shape range), 8-byte aligned (the forward's content is not
 * needed by the backward; the backward takes capacity and free_bits for symmetry and only checks them).  VG_ERR_BAD_ARG
 * before any launch: a NULL pointer other than gz / gloss, B or D outside [1, 1024], a free_bits or a capacity that is not
 * finite and >= 0, and -- here also VG_ERR_BAD_ARG -- a workspace shorter than that. */
size_t vg_reparam_klc_workspace_bytes(int B, int D);
int vg_reparam_klc_fwd(const float* mu, const float* logvar, const float* eps, float* z, float* out4, float* gate,
                       float* kl_dim, int B, int D, float beta, float capacity, float free_bits, void* workspace,
                       size_t workspace_bytes, void* stream);
int vg_reparam_klc_bwd(const float* gz, const float* mu, const float* logvar, const float* eps, const float* gate,
                       const float* gloss, float beta, float capacity, float free_bits, float* gmu, float* glogvar, int B,
                       int D, void* workspace, size_t workspace_bytes, void* stream);
/* beta AND the capacity read from DEVICE memory (beta_dev[0], capacity_dev[0], fp32): a capacity annealed every iteration
 * replays one captured graph.  The same fp32 values give the same bits.  Either word NULL is VG_ERR_BAD_ARG; the words'
 * values are not checked (a NaN capacity is a NaN loss). */
int vg_reparam_klc_fwd_dev(const float* mu, const float* logvar, const float* eps, float* z, float* out4, float* gate,
                           float* kl_dim, int B, int D, const float* beta_dev, const float* capacity_dev, float free_bits,
                           void* workspace, size_t workspace_bytes, void* stream);
int vg_reparam_klc_bwd_dev(const float* gz, const float* mu, const float* logvar, const float* eps, const float* gate,
                           const float* gloss, const float* beta_dev, const float* capacity_dev, float free_bits,
                           float* gmu, float* glogvar, int B, int D, void* workspace, size_t workspace_bytes,
                           void* stream);

/* ---- FactorVAE (Kim & Mnih 2018; disentanglement_lib's form): the pieces around the latent critic; DESIGN.md section
 * 4.32; csrc/factor_vae.hip.  The critic maps a code to two logits (l0: "drawn from q(z)", l1: "dimensions permuted
 * across the batch"); its GEMMs are not part of this library.
 *
 * vg_permute_dims: z_perm[i,d] = z[pi_d[i], d] with pi_d the STABLE ascending argsort of column d of u (ties by row index;
 * torch.sort's order: -0 == +0, NaN last), z, u, z_perm row-major fp32 [B,D].  Rank by counting: a workgroup stages 16
 * columns of u, all B rows, in LDS and every thread counts the rows that sort before its own; every element of z_perm is
 * written exactly once, no atomic, one launch, the same bits every run.  Forward only.  D >= 1; 1 <= B <=
 * VG_PERMUTE_MAX_BATCH: 16 columns x 2048 rows x 4 bytes are 128 KiB of the CU's 160 KiB of LDS (the next power of two
 * does not fit; B <= 256 and B <= 1024 take 16 and 64 KiB).  VG_ERR_BAD_ARG: a NULL pointer, z_perm aliasing z or u, B or D
 * outside that range.
 *
 * vg_factor_tc_fwd: the encoder phase's loss from logits [B,2] of the critic on z and kl, the DEVICE scalar of the
 * UNWEIGHTED KL summed over the batch (vg_reparam_kl_fwd with beta = 1):
 *   tc = sum_b (l0 - l1)  (fp64, fixed order)      out4 = {beta*kl + gamma*tc, kl, tc, #{b : l0 > l1}}
 * vg_factor_tc_bwd: glogits[b] = {+gamma*gloss, -gamma*gloss}, gkl = beta*gloss (gloss: DEVICE scalar, upstream of
 * out4[0]).  One launch each.  `workspace` is not used (vg_factor_tc_workspace_bytes returns 0; the arguments keep the
 * shape of the other objectives' entry points).  The `_dev` twins read beta AND gamma from device words (fp32): a gamma
 * annealed every iteration replays one captured graph; the same fp32 values give the same bits.  VG_ERR_BAD_ARG: a NULL
 * pointer (workspace excepted), B < 1.  The weights' values are not checked.
 *
 * vg_factor_critic_loss: the critic phase's cross-entropy on logits [2B,2] -- rows [0,B) are z (class 0), rows [B,2B)
 * permuted (class 1) --, its gradient and the accuracy, in one launch:
 *   x_b = l1 - l0 (b < B), l0 - l1 (b >= B)      loss = sum_b softplus(x_b) / divisor  (fp64 sum, fixed order)
 *   glogits[b] = -+sigmoid(x_b) / divisor on the row's own class, +- on the other      acc = #{b : x_b < 0} / (2B)
 * softplus and sigmoid in their overflow-safe forms (|x| = 1e4 gives x or 0, and exactly 1 or 0); a NaN logit is a NaN
 * loss; a tie x_b == 0 counts as wrong.  glogits and acc may be NULL.  VG_ERR_BAD_ARG: logits or loss NULL, glogits
 * aliasing logits, B < 1, a divisor that is not finite and > 0. */
#define VG_PERMUTE_MAX_BATCH 2048
int vg_permute_dims(const float* z, const float* u, float* z_perm, int B, int D, void* stream);
size_t vg_factor_tc_workspace_bytes(int B, int D);
int vg_factor_tc_fwd(const float* logits, const float* kl, float* out4, int B, float beta, float gamma, void* workspace,
                     size_t workspace_bytes, void* stream);
int vg_factor_tc_bwd(const float* gloss, float beta, float gamma, float* glogits, float* gkl, int B, void* workspace,
                     size_t workspace_bytes, void* stream);
int vg_factor_tc_fwd_dev(const float* logits, const float* kl, float* out4, int B, const float* beta_dev,
                         const float* gamma_dev, void* workspace, size_t workspace_bytes, void* stream);
int vg_factor_tc_bwd_dev(const float* gloss, const float* beta_dev, const float* gamma_dev, float* glogits, float* gkl,
                         int B, void* workspace, size_t workspace_bytes, void* stream);
int vg_factor_critic_loss(const float* logits, float* loss, float* glogits, float* acc, int B, float divisor,
                          void* stream);

/* ---- log-density under the aggregate posterior, at evaluation scale (the ELBO decomposition over a dataset and MIG:
 * Chen et al. 2018, section 4 and appendix C; csrc/agg_posterior.hip).  Forward only.  With
 *   lq[m,j,d] = log N(z[m,d]; mu[j,d], exp(logvar[j,d]))      m < M evaluation points, j < N posteriors, d < D
 * it writes the two UNNORMALISED log-sum-exps (the caller subtracts log N)
 *   lse_joint[m] = LSE_j sum_d lq[m,j,d]   (fp64, [M])        lse_dim[m,d] = LSE_j lq[m,j,d]   (fp32, [M,D])
 * A lane owns an evaluation point, a wavefront VG_AGG_POINT_TILE of them (four wavefronts to a workgroup); the rows stream
 * past as wavefront-uniform values, their constants sqrt(exp(-logvar)/2) and -(log 2 pi + logvar)/2 formed once per row
 * by a prepare pass.  The row sum over d is accumulated in fp64; both log-sum-exps keep a running maximum (no fixed
 * shift: a point far from every posterior gives a finite, correct value).  N is cut into `splits` ranges of whole row
 * tiles (VG_AGG_ROW_TILE rows) whose partial (max, sum) pairs a last kernel merges in split order: no atomics, the same
 * inputs and `splits` give the same bits.  splits == 0: chosen from (M, N, D) alone, separately for the joint kernel (many
 * short ranges: its partials are 16 bytes a point) and the per-dimension kernel.  A `splits` above the number of row
 * tiles (or above 1024) is CLAMPED, and ranges left empty by the rounding are dropped; vg_agg_posterior_splits returns
 * the count that runs (with splits == 0: the per-dimension kernel's; 0 for rejected sizes).  Six launches.
 * 1 <= D <= 1024, 1 <= N <= 2^24, 1 <= M with M * D < 2^38, splits >= 0: otherwise VG_ERR_BAD_ARG.  `workspace`:
 * vg_agg_posterior_workspace_bytes(M, N, D, splits) bytes (the same `splits` as the call), 256-byte aligned; a shorter
 * one is VG_ERR_WORKSPACE. */
#define VG_AGG_POINT_TILE 64
#define VG_AGG_ROW_TILE 8
int vg_agg_posterior_splits(int M, int N, int D, int splits);
size_t vg_agg_posterior_workspace_bytes(int M, int N, int D, int splits);
int vg_agg_posterior_lse(const float* z, const float* mu, const float* logvar, double* lse_joint, float* lse_dim, int M,
                         int N, int D, int splits, void* workspace, size_t workspace_bytes, void* stream);

/* ---- all-pairs squared Euclidean distances of two feature sets, reduced on the fly (sample-quality metrics: improved
 * precision / recall, Kynkaanniemi et al. 2019; density / coverage, Naeem et al. 2020; DESIGN.md section 4.25;
 * csrc/pair_dist.hip).  a[M,D] and b[N,D] are row-major fp32; no pointer needs more than a float's alignment.  With
 *   d2[i,j] = sum_d (a[i,d] - b[j,d])^2      formed from the DIFFERENCES (never the Gram form: identical rows give
 * exactly 0), one fp32 FMA chain in ascending d whose order depends neither on the tile, nor on `splits`, nor on which
 * operand is a and which is b -- d2 of two given rows has the same bits in every call that forms it;
 * |d2 - exact| <= (D + 3) 2^-24 exact.
 *   vg_pair_knn:   out[i, 0..K) (fp32, [M,K]) = the K smallest d2[i, .], ascending, 1 <= K <= VG_PAIR_MAX_K; slots for
 *                  which no candidate exists hold +inf.  exclude_self = 1 skips j == i BY INDEX (a duplicate row
 *                  elsewhere still counts, with distance 0); it requires a == b and M == N.  Any other non-zero value,
 *                  or 1 without those, is VG_ERR_BAD_ARG.
 *   vg_pair_hits:  count[i] (int32, [M]) = #{ j : d2[i,j] <= thr[j] }, thr fp32 [N], one threshold per COLUMN.  The
 *                  comparison is <=, as in Kynkaanniemi's code (the prdc package of Naeem et al. uses <: the two differ
 *                  on exact ties only); a NaN threshold or distance counts nothing.
 * A workgroup owns VG_PAIR_TILE rows of a and walks a range of column tiles (VG_PAIR_TILE rows of b each); N is cut into
 * `splits` ranges of whole column tiles whose partial lists / counts a second kernel merges in range order: no atomics,
 * nothing of size M x N in memory, the same bits every run and for every `splits`.  splits == 0: chosen from (M, N)
 * alone.  A `splits` above the number of column tiles (or above 1024) is CLAMPED, and ranges left empty by the rounding
 * are dropped; vg_pair_splits returns the count that runs (0 for rejected sizes).  Two launches each.
 * 1 <= M, N <= 2^20, 1 <= D <= 4096, splits >= 0: otherwise VG_ERR_BAD_ARG (the two planners return 0).  `workspace`:
 * vg_pair_workspace_bytes(M, N, D, K, splits) bytes (the same `splits` as the call; K = 1 for vg_pair_hits), 256-byte
 * aligned; a shorter one is VG_ERR_WORKSPACE. */
#define VG_PAIR_TILE 64
#define VG_PAIR_MAX_K 8
int vg_pair_splits(int M, int N, int D, int splits);
size_t vg_pair_workspace_bytes(int M, int N, int D, int K, int splits);
int vg_pair_knn(const float* a, const float* b, int exclude_self, float* out, int M, int N, int D, int K, int splits,
                void* workspace, size_t workspace_bytes, void* stream);
int vg_pair_hits(const float* a, const float* b, const float* thr, int* count, int M, int N, int D, int splits,
                 void* workspace, size_t workspace_bytes, void* stream);

/* ---- reconstruction quality of an image batch against its originals (the distortion side of a beta sweep: PSNR, SSIM,
 * Wang et al. 2004, and MS-SSIM, Wang et al. 2003, are formed from these three numbers per image; the reference logs only
 * a pixel MSE, new_betavaegan.py:189-197; csrc/recon_quality.hip).  x, y: contiguous fp32
 * [B,C,H,W]; out: fp64 [B,3], per image
 *   out[b,0] = sse  = sum_{c,h,w} (x - y)^2                                    (differences and squares in fp64)
 *   out[b,1] = ssim = mean of (2 mx my + C1)(2 sxy + C2) / ((mx^2 + my^2 + C1)(sx2 + sy2 + C2))
 *   out[b,2] = cs   = mean of (2 sxy + C2) / (sx2 + sy2 + C2)
 * both means over the C (H - window + 1)(W - window + 1) VALID window positions (no padding), with mx, my, sx2, sy2, sxy the
 * Gaussian-weighted window moments, C1 = (k1 L)^2, C2 = (k2 L)^2, L = data_range.  `window` is odd, 3..11; the taps
 * exp(-(i - (window - 1)/2)^2 / (2 sigma^2)), normalised to sum 1, are formed on the host in fp64.
 * Arithmetic: the five moments (x, y, x^2, y^2, xy) by a separable filter, a horizontal then a vertical pass, each ONE fp64
 * FMA chain in ascending tap order from 0 (products of the fp32 inputs formed in fp64: exact); sx2 = E[x^2] - mx^2 and
 * everything after it fp64 without contraction.  A pixel's value does not depend on the band or tile that formed it; x
 * against itself gives sse = 0 and ssim = cs = 1 exactly.  Per-pixel error against an exact evaluation <= ~3e-12 at the
 * defaults on |x|, |y| <= L/2.  A NaN or inf pixel makes its image's three outputs non-finite, no other's.
 * A workgroup owns one (image, channel, band of VG_RECON_BAND_ROWS output rows, tile of VG_RECON_TILE_COLS output
 * columns): inputs with their halo in LDS as fp32, the horizontal pass's results in LDS as fp64, a reduction by wavefront
 * shuffles into the workgroup's workspace slot; a second kernel adds an image's slots in index order.  No atomics, nothing
 * of the moments' size in memory, two launches, the same bits every run and wherever in the batch an image stands.
 * VG_ERR_BAD_ARG: a NULL pointer, a dimension < 1, `window` even or outside 3..11, H or W < window, sigma or data_range
 * not finite and > 0, k1 or k2 not finite and >= 0, more than 2^31 - 1 workgroups (B * C * bands * tiles), out or
 * workspace not 8-byte aligned; the workspace query returns 0 for the rejected sizes.  `workspace`:
 * vg_recon_quality_workspace_bytes(...) bytes; a shorter one is VG_ERR_WORKSPACE. */
#define VG_RECON_BAND_ROWS 16
#define VG_RECON_TILE_COLS 32
size_t vg_recon_quality_workspace_bytes(int B, int C, int H, int W, int window);
int vg_recon_quality(const float* x, const float* y, double* out, int B, int C, int H, int W, int window, double sigma,
                     double data_range, double k1, double k2, void* workspace, size_t workspace_bytes, void* stream);

/* ---- differentiable augmentation of the discriminator's inputs (Zhao et al. 2020, "Differentiable Augmentation for
 * Data-Efficient GAN Training"; the reference trains without one; csrc/diff_augment.hip).
 * x, y, gy, gx: contiguous fp32 [B,C,H,W], the output never the input; u: fp32 [B,8], uniforms in [0, 1), one row per
 * image; `policy`: a bit set of VG_AUGMENT_*, 1..7; p in [0, 1].  Per image, in this order:
 *   colour       b = u0 - 1/2, s = 2 u1, c = u2 + 1/2:  x1 = x + b;  x2 = (x1 - mean_C x1) s + mean_C x1;
 *                x3 = (x2 - m) c + m,  m = mean_CHW x2 = mean_CHW x + b
 *   translation  r_h = int(H/8 + 1/2), t_r = min(floor(u3 (2 r_h + 1)), 2 r_h) - r_h, t_c alike from u4 and W:
 *                y[c][i][j] = x3[c][i + t_r][j + t_c] inside the image, 0 outside
 *   cutout       k_h = int(H/2 + 1/2), n_h = H + 1 - (k_h mod 2), o_r = min(floor(u5 n_h), n_h - 1): rows
 *                o_r - floor(k_h/2) .. o_r - floor(k_h/2) + k_h - 1 are cut, columns alike from u6 and W; a position whose
 *                row AND column are cut is 0 (on the translated image)
 *   gate         the image is transformed iff u7 < p; otherwise its output is a bit copy of its input.
 * Each floor takes ONE fp32 product.  The backward is the transpose of the linear part and reads gy and u alone:
 *   g3 = gy masked and shifted back;  g2 = c g3 + (1 - c) mean_CHW g3;  gx = s g2 + (1 - s) mean_C g2;
 * a closed image's gx is a bit copy of its gy.  Without VG_AUGMENT_COLOR: ONE launch each way, the outputs are copies and
 * zeros (exact), no workspace is read (it may be NULL).  With it: TWO launches each way -- per (image, chunk of
 * VG_DIFF_AUGMENT_SUM_CHUNK elements of the image's C H W) the chunk's sum in fp64 into the workspace slot [image][chunk],
 * then the apply pass, where every thread adds its image's slots in index order; the colour arithmetic is fp32 (error
 * per element <= ~30 * 2^-24 (max|x| + 1/2) forward, of max|gy| backward).  Masks are selects: what is dropped is 0
 * whatever it held.  No floating-point atomic; the same bits every run and wherever in the batch an image stands; no host
 * read, no allocation: capturable.  No bound of max |y| is emitted: the 3-channel convolutions that consume y take none.
 * VG_ERR_BAD_ARG before any launch: a NULL x / u / y, y == x, B < 1, C outside 1..VG_DIFF_AUGMENT_MAX_CHANNELS, H or
 * W < 2, C H W or a grid past 2^31 - 1, policy outside 1..7, p outside [0, 1] or NaN, and with VG_AUGMENT_COLOR a NULL
 * or not 8-byte aligned workspace; the workspace query returns 0 for the rejected sizes.  `workspace` (with
 * VG_AUGMENT_COLOR): vg_diff_augment_workspace_bytes(...) bytes; a shorter one is VG_ERR_WORKSPACE. */
#define VG_AUGMENT_COLOR 1
#define VG_AUGMENT_TRANSLATION 2
#define VG_AUGMENT_CUTOUT 4
#define VG_DIFF_AUGMENT_MAX_CHANNELS 4
#define VG_DIFF_AUGMENT_SUM_CHUNK 4096
size_t vg_diff_augment_workspace_bytes(int B, int C, int H, int W);
int vg_diff_augment_fwd(const float* x, const float* u, float* y, int B, int C, int H, int W, int policy, float p,
                        void* workspace, size_t workspace_bytes, void* stream);
int vg_diff_augment_bwd(const float* gy, const float* u, float* gx, int B, int C, int H, int W, int policy, float p,
                        void* workspace, size_t workspace_bytes, void* stream);
/* The same two with p read from DEVICE memory (p_dev[0], fp32) by the kernels when they run: a p that changes between
 * replays of an iteration captured in a HIP graph (vg_ada_update below writes one).  The same kernels, the same launches
 * and, for the same p, the value entry points' bits element for element.  The host knows no p, so none is range-checked:
 * an image is transformed iff u7 < p_dev[0] whatever the word holds -- a word <= 0 closes every image, one > u7's largest
 * value opens every image, a NaN closes every image (u7 < NaN is false).  The backward reads the word when IT runs: the
 * word must not change between a forward and its backward, or the transpose is that of another gate.  A NULL p_dev is
 * VG_ERR_BAD_ARG; everything else as above. */
int vg_diff_augment_fwd_dev(const float* x, const float* u, float* y, int B, int C, int H, int W, int policy,
                            const float* p_dev, void* workspace, size_t workspace_bytes, void* stream);
int vg_diff_augment_bwd_dev(const float* gy, const float* u, float* gx, int B, int C, int H, int W, int policy,
                            const float* p_dev, void* workspace, size_t workspace_bytes, void* stream);

/* Adaptive discriminator augmentation (Karras et al. 2020, "Training GANs with Limited Data", section 3; DESIGN.md section
 * 4.35): the controller of the p above.  `state`: eight device words (32 bytes, 4-byte aligned) -- word 0 is the p_dev of
 * the _dev entry points.  One call per iteration on d_real[B], the discriminator's outputs on the real batch (logits with
 * threshold 0, probabilities with threshold 0.5):
 *   sign_sum += sum_b ((d[b] > threshold) - (d[b] < threshold))     integers: exact, no order shows; a NaN or a tie adds 0
 *   count += B;  calls += 1                                          (and is counted)
 * and once calls reaches `interval`:
 *   r_t = (float)sign_sum / (float)count                             one fp32 division
 *   s = (r_t > target) - (r_t < target)
 *   p = clamp(p + s * ((float)count * rate), 0, 1)                   ONE rounded fp32 product, ONE rounded fp32 sum, no FMA;
 *                                                                    s = 0 leaves p as it is; a NaN p stays a NaN
 *   rt = r_t;  adjustments += 1;  sign_sum = count = calls = 0.
 * With rate = 1 / (kimg * 1000) the step is Karras's batch * interval / (kimg * 1000), exact for a ragged last batch.
 * One workgroup, no floating-point atomic, plain stores, no host read: capturable.  The caller keeps interval * B below
 * 2^31.  VG_ERR_BAD_ARG before the launch: a NULL d_real or state, a state off a 4-byte boundary, B < 1, interval < 1, a
 * NaN threshold, a non-finite target or rate, rate < 0. */
typedef struct vg_ada_state {
  float p;           /* [0] the augmentation probability */
  int sign_sum;      /* [1] sum of the signs since the last adjustment */
  int count;         /* [2] outputs seen since the last adjustment */
  int calls;         /* [3] calls since the last adjustment */
  float rt;          /* [4] r_t of the last adjustment (0 before the first) */
  int adjustments;   /* [5] adjustments made */
  int reserved[2];   /* [6], [7] written 0 */
} vg_ada_state;
int vg_ada_update(const float* d_real, int B, float threshold, float target, float rate, int interval, void* state,
                  void* stream);

/* out[i] = g[i] * s[0] with s a DEVICE scalar: applies the upstream gradient of a
 * loss scalar to a gradient precomputed by the fused loss kernels, without a
 * host read of s (out may alias g). */
int vg_scale_by_scalar(const float* g, const float* s, float* out, size_t n, void* stream);

/* loss[0] = scale * sum((a-b)^2);  ga = gscale * 2*scale*(a-b)  (ga may be NULL).
 * scale=0.5: Dis_l / SIM (new_betavaegan.py:67-69); scale=1: pixel MSE (:71-75). */
int vg_sqdiff_loss(const float* a, const float* b, float* loss, float* ga, size_t n,
                   float scale, float gscale, void* workspace, size_t workspace_bytes, void* stream);
size_t vg_sqdiff_workspace_bytes(size_t n);

/* nn.BCELoss() against a constant label (new_betavaegan.py:53,101,118,153-154):
 * loss[0] = (1/divisor) * sum(-(t*max(log p,-100) + (1-t)*max(log(1-p),-100)));
 * gp = gscale/divisor * (p-t)/max(p*(1-p),1e-12)   (gp may be NULL).
 * divisor = B locally; the global batch under data parallelism. */
int vg_bce_loss(const float* p, float target, float* loss, float* gp, int B, float divisor,
                float gscale, void* stream);
/* The same with the label read from DEVICE memory (target_dev[0]): the per-iteration soft / flipped label of
 * new_betavaegan.py:89-90 changes between replays of an iteration captured in a HIP graph. */
int vg_bce_loss_dev(const float* p, const float* target_dev, float* loss, float* gp, int B, float divisor,
                    float gscale, void* stream);

/* the discriminator's head and its GAN loss fused (rows kernel + fixed-order sum forward, one kernel backward) -- Linear(2048 -> 1) + Sigmoid
 * (model.py:406-408) followed by nn.BCELoss against the iteration's label (new_betavaegan.py:101,118,153-154):
 *   p[b] = sigmoid(<feat[b,:], w> + bias[0]);  loss[0] = the vg_bce_loss of p;
 *   dlogit[b] = d loss / d logit[b] = (1/divisor) (p-t)/max(p(1-p),1e-12) * p (1-p)      (may be NULL)
 * (the same fp32 expressions as vg_bias_act_fwd(sigmoid) -> vg_bce_loss -> vg_act_bwd).  The label is `target`, or
 * target_dev[0] when target_dev != NULL (captured iterations).  Backward, given g = gloss[0] (device; NULL = 1):
 *   gfeat[b,k] = g dlogit[b] w[k];  gw[k] = g sum_b dlogit[b] feat[b,k];  gb[0] = g sum_b dlogit[b]
 * (each output may be NULL: a frozen discriminator only relays gfeat). */
size_t vg_dot_sigmoid_bce_workspace_bytes(int B);      /* the row terms of the loss (double), summed in a fixed order */
int vg_dot_sigmoid_bce_fwd(const float* feat, const float* w, const float* bias, float target, const float* target_dev,
                           float* p, float* loss, float* dlogit, int B, int K, float divisor,
                           void* workspace, size_t workspace_bytes, void* stream);
int vg_dot_sigmoid_bce_bwd(const float* dlogit, const float* gloss, const float* feat, const float* w, float* gfeat,
                           float* gw, float* gb, int B, int K, int accumulate_param_grads /* gw, gb += */, void* stream);

/* Adversarial losses on the LOGIT s (csrc/gan_loss.hip).  Per row, with label t:
 *   VG_GAN_LOGISTIC    l = (1-t) s + softplus(-s)     dl/ds = sigmoid(s) - t      (BCE-with-logits: nn.BCELoss's objective)
 *   VG_GAN_LSGAN       l = (s-t)^2 / 2                dl/ds = s - t
 *   VG_GAN_HINGE_REAL  l = max(0, 1-s)                dl/ds = -1 where 1-s > 0, else 0 (an exact tie: 0)
 *   VG_GAN_HINGE_FAKE  l = max(0, 1+s)                dl/ds = +1 where 1+s > 0, else 0
 *   VG_GAN_HINGE_GEN   l = -s                         dl/ds = -1
 * (the hinge kinds ignore t).  softplus(-s) = max(-s, 0) + log1p(exp(-|s|)) and sigmoid(s) from exp(-|s|): neither
 * overflows, and the gradient is never lost to the rounding of a probability.  A NaN logit gives a NaN loss and a NaN
 * gradient for every kind; +-inf give what the formulas give in IEEE arithmetic.
 *   vg_dot_gan_loss_fwd: logit[b] = <feat[b,:], w> + bias[0] (bias may be NULL);  p[b] = sigmoid(logit[b]) (for logging,
 *     any kind);  loss[0] = (1/divisor) sum_b l(logit[b]), the row terms added in double in index order (workspace);
 *     dlogit[b] = (1/divisor) dl/ds (may be NULL).  The label is `target`, or target_dev[0] when target_dev != NULL.
 *     16-byte loads when K % 4 == 0 and feat, w are 16-byte aligned, element loads otherwise.  Its backward is
 *     vg_dot_sigmoid_bce_bwd, which takes any dlogit.
 *   vg_gan_loss: the same on a logit vector (B,): p (may be NULL), loss[0] (may be NULL),
 *     glogit[b] = gscale/divisor dl/ds (may be NULL).
 * No atomics: the same bits every run. */
#define VG_GAN_LOGISTIC 0
#define VG_GAN_LSGAN 1
#define VG_GAN_HINGE_REAL 2
#define VG_GAN_HINGE_FAKE 3
#define VG_GAN_HINGE_GEN 4
size_t vg_dot_gan_loss_workspace_bytes(int B);
int vg_dot_gan_loss_fwd(const float* feat, const float* w, const float* bias, int kind, float target,
                        const float* target_dev, float* logit, float* p, float* loss, float* dlogit, int B, int K,
                        float divisor, void* workspace, size_t workspace_bytes, void* stream);
int vg_gan_loss(const float* logit, int kind, float target, const float* target_dev, float* p, float* loss,
                float* glogit, int B, float divisor, float gscale, void* stream);

/* ---- Adam (experiments/new_betavaegan.py:49-50: optim.Adam defaults, stepped 3x per iteration)
 * For each tensor: m += (1-beta1)(g-m); v = beta2 v + (1-beta2) g^2;
 * p -= (lr / bias_correction1) * m / (sqrt(v) / bias_correction2_sqrt + eps),
 * with bias_correction1 = 1 - beta1^step and bias_correction2_sqrt = sqrt(1 - beta2^step) computed by
 * the caller (double).  `tensors` is a HOST array of DEVICE pointers (fp32, n elements each);
 * any number of tensors, 24 per kernel launch.  No amsgrad / maximize; weight decay: vg_adam_step_decay below.
 * Two kernels stand behind the step entry points: the plain step (vg_adam_step, _checked, _dev, _dev_checked) and one
 * feature kernel, which every other entry point launches with what it turns on -- the averages, the clip record, the
 * weight decay, the decay word on the device -- as run-time arguments; element by element it gives the plain step's
 * bits.  `scalars` is two floats for the entry points paired with vg_adam_prepare (_dev, _dev_checked, _dev_ema,
 * _dev_clip: scalars[2..3] are never read) and four for those paired with vg_adam_prepare_dev (_dev_decay, _dev_ema_dev). */
typedef struct {
  float* p;
  const float* g;
  float* m;
  float* v;
  size_t n;
  /* NULL, or DEVICE memory: amax[0] = max(amax[0], max |p| after the update) -- the bound the fp16x3 Linear GEMMs
   * (vg_gemm_nt_f16x3) scale this weight by; the caller zeroes it before the step */
  float* amax;
} VgAdamTensor;
int vg_adam_step(const VgAdamTensor* tensors, int count, double lr, double beta1, double beta2, double eps,
                 double bias_correction1, double bias_correction2_sqrt, void* stream);
/* The same step with its scalars on the DEVICE, for an iteration captured in a HIP graph (kernel arguments are frozen
 * at capture; the step count is not).  vg_adam_prepare (one thread) writes scalars[0] = lr / (1 - beta1^step) and
 * scalars[1] = sqrt(1 - beta2^step), formed in double: with advance_device_counter the device counter step_dev[0] is
 * advanced by one and used (captured steps); without, the host's `step` (>= 1) is used and -- step_dev may be NULL --
 * stored in the counter (eager steps between replays keep it current; same expression, same bits).
 * vg_adam_step_dev is vg_adam_step reading those two scalars. */
int vg_adam_prepare(double step, double* step_dev, int advance_device_counter, double lr, double beta1, double beta2,
                    float* scalars, void* stream);
int vg_adam_step_dev(const VgAdamTensor* tensors, int count, double beta1, double beta2, double eps,
                     const float* scalars, void* stream);
/* The two steps with a non-finite guard.  `nonfinite` is NULL or a HOST array of `count` DEVICE words parallel to
 * `tensors` (any entry may be NULL); the words belong to the caller -- the library still holds no state.  The step ORs
 * into tensor i's word
 *   VG_NONFINITE_GRAD   an inf / NaN among the gradient elements it READ,
 *   VG_NONFINITE_PARAM  an inf / NaN among the parameter elements it WROTE,
 * and only ever ORs: a word stays up until the caller zeroes it, a clean step writes nothing (one atomicOr per
 * workgroup that saw something).  Tensors with n == 0 are skipped, their word untouched.  p, m, v and amax are
 * bit for bit those of the unchecked step, which is this one without words: these entry points DETECT, they do not
 * skip (that takes a grid-wide answer before the first store: the opt-in norm pass in front of vg_adam_step_clip
 * below) -- once a bit is up the weights are poisoned and the last good checkpoint is the way back. */
#define VG_NONFINITE_GRAD 1u
#define VG_NONFINITE_PARAM 2u
int vg_adam_step_checked(const VgAdamTensor* tensors, int count, double lr, double beta1, double beta2, double eps,
                         double bias_correction1, double bias_correction2_sqrt, unsigned* const* nonfinite,
                         void* stream);
int vg_adam_step_dev_checked(const VgAdamTensor* tensors, int count, double beta1, double beta2, double eps,
                             const float* scalars, unsigned* const* nonfinite, void* stream);
/* The weight gradient of a big Linear layer and its plain Adam step in ONE kernel: gy (M x N), x (M x K), the weight
 * and its moments p, m, v (N x K, fp32).  Every gradient element gW = gy^T x is formed as vg_gemm_nt_f16x3 forms it in
 * this orientation (A = gy with a_row_stride = 1, B = x with b_row_stride = 1, reduction M) and is used, in registers,
 * as the g of vg_adam_step_checked (host scalars) / vg_adam_step_dev_checked (the two device scalars of
 * vg_adam_prepare): p, m, v, the amax word and the flag bits are bit for bit what that pair leaves, and the gradient
 * is never written -- unless g_out (N x K, normally NULL) is given, which receives it as well (tests, diagnostics).
 * gy_amax / x_amax: the operands' bound words, as for vg_gemm_nt_f16x3.  amax: NULL, or the weight's bound word -- it
 * is ZEROED by a one-thread kernel in front of the fused kernel (in stream order behind the layer's data-gradient GEMM,
 * which reads the old bound), then max |p| is added to it.  nonfinite: NULL, or the weight's flag word (the GRAD bit
 * is judged on the gradient element, the PARAM bit on the new weight).
 * VG_ERR_BAD_ARG before any launch unless: the reduction M is a multiple of 32 and not split over workgroups
 * (vg_gemm_nt_f16x3_workspace_bytes(N, K, M) == 0), K % 4 == 0, and p, m, v (g_out) are 16-byte aligned -- every
 * element is then on the plain step's 16-byte body. */
int vg_linear_wgrad_adam(const float* gy, const float* x, int M, int N, int K, const float* gy_amax, const float* x_amax,
                         float* p, float* m, float* v, float* amax, unsigned* nonfinite, double lr, double beta1,
                         double beta2, double eps, double bias_correction1, double bias_correction2_sqrt, float* g_out,
                         void* stream);
int vg_linear_wgrad_adam_dev(const float* gy, const float* x, int M, int N, int K, const float* gy_amax,
                             const float* x_amax, float* p, float* m, float* v, float* amax, unsigned* nonfinite,
                             double beta1, double beta2, double eps, const float* scalars, float* g_out, void* stream);
/* The two checked steps that also keep an exponential moving average of the weights they write.  `ema` is a HOST
 * array of `count` DEVICE pointers parallel to `tensors` (fp32, n elements each, not overlapping p, g, m, v); after
 * an element's p is updated the same thread does
 *   e <- e + (float)(1 - ema_decay) * (p_new - e)
 * from the p it has just formed (8 more bytes per parameter; an inf / NaN in p goes into e unfiltered and is
 * reported by the guard as before).  Single entries may be NULL: those tensors are stepped and not averaged.
 * ema == NULL is VG_ERR_BAD_ARG (that is what the entry points above are for), as is an ema_decay outside (0, 1) --
 * before any launch.  `nonfinite` as above (may be NULL).  p, m, v, amax and the flag words are bit for bit those of
 * the checked step. */
int vg_adam_step_ema(const VgAdamTensor* tensors, int count, double lr, double beta1, double beta2, double eps,
                     double bias_correction1, double bias_correction2_sqrt, unsigned* const* nonfinite,
                     float* const* ema, double ema_decay, void* stream);
int vg_adam_step_dev_ema(const VgAdamTensor* tensors, int count, double beta1, double beta2, double eps,
                         const float* scalars, unsigned* const* nonfinite, float* const* ema, double ema_decay,
                         void* stream);
/* Clipping by global norm and skipping a non-finite step: one pass over the gradients in front of the step, all
 * answers in DEVICE memory (nothing here synchronises; the three calls can be captured in a HIP graph).
 *
 * vg_grad_sumsq_multi: `grads` / `n` are HOST arrays of `count` DEVICE pointers (fp32) and lengths; any count, 24
 * tensors per launch, tensors with n == 0 skipped.  Every workgroup writes the sum of squares of its 8192 elements,
 * formed in double from the first product on (exact squares, no overflow for any finite fp32), into a slot of its own:
 * partials[0 .. vg_grad_sumsq_partials(n, count)) in tensor order -- no atomics, the same bits run to run.
 * vg_grad_sumsq_partials (host only) is that number of slots, sum of ceil(n[i] / 8192); `capacity` is the number of
 * doubles `partials` holds.  An inf / NaN among the gradients makes its slot, and so the total, inf / NaN.
 *
 * vg_grad_clip_finalize (one workgroup) adds the partials in a fixed order in double and writes the caller-owned
 * record, four 32-bit words:
 *   record[0]  norm     float   (float)sqrt(sum)
 *   record[1]  coef     float   max_norm > 0: (float)min(1, max_norm / (norm + 1e-6)) in double -- torch's
 *                               clip_grad_norm_ formula (a NaN norm gives NaN, an inf norm 0: torch's behaviour);
 *                               max_norm <= 0: no clipping, 1.  With `skip` up: 0.
 *   record[2]  skip     uint32  1 when the norm is inf / NaN and skip_nonfinite != 0, else 0
 *   record[3]  skipped  uint32  += skip: a running count the caller zeroes and the kernel only increments
 *
 * vg_adam_step_clip / vg_adam_step_dev_clip: vg_adam_step_ema / vg_adam_step_dev_ema reading that record.  Every
 * gradient element is used as gs = coef * g (one fp32 rounding, that of g.mul_(coef)); p, m, v, amax, the flag words
 * and the averages are bit for bit those of the step above on such a gradient (the GRAD bit is judged on gs).  `ema`
 * may be NULL here (no average at all; ema_decay is then ignored), and single entries as above.  With `skip` up the
 * step stores nothing to p, m, v or an average: it adds max |p| of the unchanged weights to amax (the caller zeroed the
 * word) and ORs VG_NONFINITE_GRAD into the word of each tensor whose gradient holds an inf / NaN (VG_NONFINITE_PARAM
 * only if p was non-finite already).  The gradients themselves are never written.
 *
 * VG_ERR_BAD_ARG before any launch: partials or record NULL, capacity too small, a NaN max_norm, an ema_decay outside
 * (0, 1) when ema is given. */
size_t vg_grad_sumsq_partials(const size_t* n, int count);
int vg_grad_sumsq_multi(const float* const* grads, const size_t* n, int count, double* partials, size_t capacity,
                        void* stream);
int vg_grad_clip_finalize(const double* partials, size_t n_partials, double max_norm, int skip_nonfinite, float* record,
                          void* stream);
int vg_adam_step_clip(const VgAdamTensor* tensors, int count, double lr, double beta1, double beta2, double eps,
                      double bias_correction1, double bias_correction2_sqrt, unsigned* const* nonfinite,
                      float* const* ema, double ema_decay, const float* clip_record, void* stream);
int vg_adam_step_dev_clip(const VgAdamTensor* tensors, int count, double beta1, double beta2, double eps,
                          const float* scalars, unsigned* const* nonfinite, float* const* ema, double ema_decay,
                          const float* clip_record, void* stream);
/* Learning rate and weight decay on the DEVICE, weight decay inside the step.
 *
 * vg_adam_prepare_dev: vg_adam_prepare with lr and the weight decay read from DEVICE memory, hyper = [lr, weight_decay]
 * (two doubles) -- a schedule writes them between the replays of a captured step.  It leaves four floats:
 *   scalars[0]  (float)(lr / (1 - beta1^step))     the expressions of vg_adam_prepare: same lr, same bits
 *   scalars[1]  (float)sqrt(1 - beta2^step)
 *   scalars[2]  decoupled != 0 and wd != 0: (float)(1 - lr * wd), product and difference each rounded in double; else 1
 *   scalars[3]  decoupled == 0: (float)wd; else 0
 * Step and counter handling as vg_adam_prepare.  VG_ERR_BAD_ARG before the launch for a NULL hyper or scalars.
 *
 * vg_adam_step_decay / vg_adam_step_dev_decay: vg_adam_step_clip / vg_adam_step_dev_clip that also decay the weights,
 * in registers, with no memory traffic of their own.  `nonfinite`, `ema` and `clip_record` may each be NULL (no record:
 * gs = g, nothing is skipped).  Per element, in fp32, with gs = coef * g as in the clip step:
 *   coupled (L2, decoupled == 0), wd != 0:   gd = gs + (wd * p)   a rounded product, then a rounded sum;
 *                                            the update of the clip step runs on (p, gd)
 *   decoupled (AdamW), wd != 0:              pd = p * s2          one rounding, s2 as scalars[2];
 *                                            the update runs on (pd, gs)
 *   wd == 0:                                 neither term is formed (no 0 * inf): the bits of the clip step
 * p, m, v, amax, the flag words and the averages are bit for bit those of the clip step on such inputs; the GRAD bit is
 * judged on gs, amax and the PARAM bit on the final p.  With the record's skip word up nothing is stored and nothing
 * decays (the clip step's skip).  The host form takes weight_decay and decoupled as arguments and forms scalars[2..3]
 * by the expressions above; the _dev form reads all four scalars.  VG_ERR_BAD_ARG before any launch: a negative or
 * NaN weight_decay, and what the clip step rejects (but for the record). */
int vg_adam_prepare_dev(double step, double* step_dev, int advance_device_counter, const double* hyper, int decoupled,
                        double beta1, double beta2, float* scalars, void* stream);
int vg_adam_step_decay(const VgAdamTensor* tensors, int count, double lr, double beta1, double beta2, double eps,
                       double bias_correction1, double bias_correction2_sqrt, unsigned* const* nonfinite,
                       float* const* ema, double ema_decay, const float* clip_record, double weight_decay, int decoupled,
                       void* stream);
int vg_adam_step_dev_decay(const VgAdamTensor* tensors, int count, double beta1, double beta2, double eps,
                           const float* scalars, unsigned* const* nonfinite, float* const* ema, double ema_decay,
                           const float* clip_record, void* stream);
/* The EMA decay on the DEVICE: vg_adam_step_dev_decay with (float)(1 - decay) read from the device word `ema_omd` (one
 * fp32, an ordinary load, uniform over the grid) instead of formed from a host double -- a warm-up writes it between
 * the replays of a captured step.  Per element, after p is updated:
 *   *ema_omd == 1.0f   e <- p_new            the bits of p ("follow the weights": e + 1 (p - e) is not p in fp32)
 *   otherwise          e <- e + *ema_omd * (p_new - e)      as above; 0.0f follows the formula (e stays, p finite)
 * `scalars` from vg_adam_prepare_dev (all four words are read); `nonfinite`, `clip_record` and single ema[i] entries
 * may be NULL as there.  With the word holding (float)(1.0 - d) for a d in (0, 1): p, m, v, the averages, amax, the flag
 * words and the record are bit for bit those of vg_adam_step_dev_ema / _dev_clip / _dev_decay with ema_decay = d.  A
 * skipped step (the record's skip word up) stores nothing to an average.  VG_ERR_BAD_ARG before any launch: ema or
 * ema_omd NULL (the entry points above step without an average), and what vg_adam_step_dev_decay rejects. */
int vg_adam_step_dev_ema_dev(const VgAdamTensor* tensors, int count, double beta1, double beta2, double eps,
                             const float* scalars, unsigned* const* nonfinite, float* const* ema, const float* ema_omd,
                             const float* clip_record, void* stream);

/* ---- image I/O either side of the step -----------------
 * Input pipeline of dataloader/dataset.py:37-43 (ToTensor + Normalize(mean, std) of a
 * shuffled batch) on a uint8 image cache resident in HBM, layout [N][H][W][C] as decoded:
 *   out[b][c][h][w] = (cache[index[b]][h][w][c] / 255 - mean) / std      (IEEE fp32, bit-exact)
 * index holds B int64 image numbers (DEVICE memory), all in [0, N). */
int vg_u8_gather_normalize(const uint8_t* cache, const int64_t* index, float* out, int B, int C,
                           int H, int W, float mean, float stdv, void* stream);

/* out2[0] = min(x), out2[1] = max(x) over n floats (DEVICE scalars; exact in any order). */
size_t vg_minmax_workspace_bytes(size_t n);
int vg_minmax(const float* x, size_t n, float* out2, void* workspace, size_t workspace_bytes,
              void* stream);

/* torchvision.utils.save_image / make_grid (pinned 0.2.1) as called by utils/utils.py:12-36:
 * x[B,C,H,W] (C = 1 or 3) -> uint8 HWC grid[GH][GW][3].  minmax (DEVICE, from vg_minmax; NULL =
 * normalize=False): v = (clamp(x, min, max) - min) / (max - min + 1e-5); byte = trunc(clamp(
 * v * 255, 0, 255)).  B == 1 gives the un-padded image; otherwise nrow images per row, `padding`
 * pixels of pad_value between and around them.  vg_image_grid_shape returns GH, GW. */
int vg_image_grid_shape(int B, int H, int W, int nrow, int padding, int* grid_h, int* grid_w);
int vg_image_grid_u8(const float* x, const float* minmax, uint8_t* grid, int B, int C, int H, int W,
                     int nrow, int padding, float pad_value, void* stream);

/* ---- from the decoder's output to the FID features without a host round trip (csrc/fid_front.hip) ----------------
 * The FID route of experiments/new_betavaegan.py:231-235 is utils.py:23-29 (save_image(x[i], normalize=True) per
 * sample) -> files -> scoring/fid.py:68-105 (load, / 255, the Inception network).  These four kernels keep it on the
 * device; all are HBM-bound streaming kernels, correct for any base alignment and any width (16-byte accesses where
 * the addresses allow).
 *
 * vg_quantize_each_u8: save_image(x[i], normalize=True) for every image i of x[B,C,H,W] (C = 1 or 3; C = 1 is
 * replicated) at once: out[B][H][W][3] uint8, per image v = (clamp(x, min, max) - min) / (max - min + 1e-5),
 * byte = trunc(clamp(v * 255, 0, 255)) with that image's own min and max.  Bit-identical to vg_minmax +
 * vg_image_grid_u8 on each image alone (same operation order); two launches for the whole batch.
 * workspace: 2 * B floats (4-byte aligned). */
int vg_quantize_each_u8(const float* x, uint8_t* out, int B, int C, int H, int W, void* workspace,
                        size_t workspace_bytes, void* stream);

/* y[B,3,OH,OW] = scale * bilinear(img[B,H,W,3] / 255) + shift: F.interpolate(mode="bilinear", align_corners=False)
 * (scoring/inception.py:147-150; ATen's rule in fp32: source coordinate max(0, (o + 0.5) * in / out - 0.5), upper
 * neighbour clamped to in - 1) and normalize_input (:152-153: scale = 2, shift = -1) in one pass.  Any sizes; in == out
 * is the identity.  amax (may be NULL): max |y| is added to amax[0] (atomic maximum on the bit pattern, DEVICE memory,
 * zeroed by the caller: see vg_absmax) -- the first convolution's x_amax. */
int vg_resize_bilinear_u8(const uint8_t* img, float* y, int B, int H, int W, int OH, int OW, float scale, float shift,
                          float* amax, void* stream);

/* 3x3 pooling of x[B,C,H,W], stride 1 or 2, padding 0 or 1, OH = (H + 2 pad - 3) / stride + 1 (OW alike) -- the three
 * poolings of the FID Inception network (scoring/inception.py:210, 238, 271, 306; the MaxPool2d(3, 2) of its blocks and of torchvision's InceptionB / D):
 *   VG_POOL_MAX               F.max_pool2d(x, 3, stride, pad): padding reads as -inf, a NaN wins;
 *   VG_POOL_AVG_EXCLUDE_PAD   F.avg_pool2d(x, 3, stride, pad, count_include_pad=False).
 * out is a (B, out_channels_total, OH, OW) tensor: channels [out_channel_offset, out_channel_offset + C) are written,
 * the others are not touched (the contract of vg_conv_general_fwd's y / y_image_stride: a pooling branch writes its
 * slice of an Inception block's concatenated output).  amax (may be NULL): the true max |out| is added to amax[0]
 * (see vg_absmax; DEVICE, zeroed by the caller; several launches may add into one slot). */
#define VG_POOL_MAX 0
#define VG_POOL_AVG_EXCLUDE_PAD 1
int vg_pool3x3(const float* x, float* out, int B, int C, int H, int W, int stride, int pad, int mode,
               int out_channels_total, int out_channel_offset, float* amax, void* stream);

/* y[b][c] = mean over hw of x[b][c][hw]: nn.AdaptiveAvgPool2d((1, 1)) (scoring/inception.py:122).  One wavefront
 * per (b, c), a summation order that depends on HW alone: bit-reproducible, no atomics, no workspace. */
int vg_global_avg_pool(const float* x, float* y, int B, int C, int HW, void* stream);

#ifdef VG_TUNING
/* ---- tuning build only (libvaegan_hip_tuning.so): process-global knobs, never in the product library ---- */
/* Diagnostics / tuning only: force tile variant `variant` (>= 0; -1 restores the
 * heuristic) for mode 0 (vg_conv5x5_fwd) or 1 (vg_convT5x5_fwd).  Process-global;
 * never used by the product path. */
int vg_debug_set_conv_tile(int mode, int variant);
/* Diagnostics / tuning only: what=0 caps the wgrad cout tile (32/64/128, -1 = heuristic);
 * what=1 sets the split-K workgroup target (-1 = heuristic); what=2 the K groups of the 128-row
 * tile (1 or 2); what=3 the input channels per column tile (5 or 10); what=4: 0 = scalar gy loads;
 * what=5: output-pixel rows per chunk of vg_conv5x5_wgrad_bf16split (1 or 2; 0 = chosen by its plan). */
int vg_debug_set_wgrad(int what, int value);
/* The plans the three weight-gradient entry points would launch for a shape under the current knobs (host only, nothing
 * runs) -- from the same planning code as the launch.  Pointers: only their alignment is looked at.
 *   vg_debug_wgrad_plan        out[9]: tw, tm, cit, ks, splits, vec4, reducer (0 slab_sum4_kernel, 1 wgrad_reduce_kernel<16>,
 *                                      2 wgrad_reduce_kernel<4>, 3 slab_sum1_kernel), chunks, chunks per split
 *   vg_debug_wgrad_split_plan  out[9]: th, wco, mtiles, ntiles, units, upw, wgs, pieces, chunks
 *   vg_debug_wgrad_thin_plan   out[6]: mt, rb, bands, upw, wgs, reducer
 * VG_ERR_BAD_ARG: the entry point does not take the shape. */
int vg_debug_wgrad_plan(int B, int Cin, int H, int W, int Cout, int stride, const void* gy, const void* dw,
                        const void* workspace, int* out);
int vg_debug_wgrad_split_plan(int B, int Cin, int H, int W, int Cout, int stride, int planes, int* out);
int vg_debug_wgrad_thin_plan(int B, int Cin, int H, int W, int Cout, int stride, int planes, const void* dw,
                             const void* workspace, int* out);
/* split-bf16 kernels of conv_bf16split.hip: 0 = 128x128, 1 = 64x128, 2 = 64x64, 3 = 32x128, 4 = 32x256 (transposed, one
 * workgroup per output-parity class), 5 = 128x128 with the 4 wavefronts along cout, 6 = 32x256 quad (transposed, stride 2,
 * two planes: all four parity classes per workgroup, bit-identical to 4; ignored elsewhere), -1 = heuristic */
int vg_debug_set_conv_bf16split_tile(int variant);
/* stride-2 ring kernel of conv_ring.hip: 0 = 256 cout x 128 px, 1 / 2 = 128 x 128 (2x4 / 4x2 wavefronts),
 * 3 = 128 x 256 (transposed), -1 = heuristic */
int vg_debug_set_conv_ring_tile(int variant);
/* What the ring kernel would launch for a stride-2 shape (mode 0 forward, 1 transposed) under the current knob (host
 * only, nothing runs) -- the launch's own plan (ring_plan, conv_ring.hip), read out.
 *   out[6]: tile variant, K splits, then the pixel tile: images, rows, columns (of the output forward, of the input
 *           transposed); paired (transposed: 1 = a workgroup runs two parity classes).
 * VG_ERR_BAD_ARG: the kernel does not take the shape. */
int vg_debug_ring_route(int mode, int B, int Cin, int H, int W, int Cout, int planes, int* out);
/* One-pass BatchNorm backward by workgroup teams (bn.hip, bn_bwd_team_kernel): nv = 1 or 8 forces the team form, with that
 * many 16-byte vectors of x and of gy per lane (a member then holds 4096 * nv elements), on every shape it can take
 * (16-byte streams, <= 16 members per channel, max_wgs >= the members of one channel); nv = 0 restores the dispatch rule
 * of vg_bn_act_bwd.  max_wgs > 0 caps the resident workgroups the grid is sized by (0: the device's compute units), so
 * that small tensors get several members, ragged last members and several rounds. */
int vg_debug_set_bn_team(int nv, int max_wgs);
/* What vg_bn_act_bwd would launch for a shape under the current knobs, on the current device (nothing runs; gy, x, gx:
 * only their alignment is looked at) -- from the same planning code as the launch.
 *   out[5]: path (0 BatchNorm1d, 1 one pass <2>, 2 one pass <8>, 3 two passes, 4 team), nv, T (members per channel),
 *           teams, rounds; nv = T = teams = rounds = 0 off the team path. */
int vg_debug_bn_bwd_plan(int B, int C, int HW, const void* gy, const void* x, const void* gx, int* out);
/* General forward convolution (conv_general.hip): force the tile of every later vg_conv_general_fwd -- tm output channels
 * x tn output pixels, each 64 or 128, 0 = that side by the heuristic; anything else: VG_ERR_BAD_ARG, knobs unchanged. */
int vg_debug_set_conv_general_tile(int tm, int tn);
/* The instantiation vg_conv_general_fwd would launch for Cout output channels and npix = B OH OW output pixels under
 * the current knobs (host only, nothing runs) -- from the launch's own cg_tile.  pad: pad_h || pad_w of the launch.
 *   out[3]: tm, tn, pad (conv_general_kernel<tm, tn, pad>). */
int vg_debug_conv_general_tile(int Cout, long npix, int pad, int* out);
#endif

#ifdef __cplusplus
}
#endif
#endif /* VAEGAN_HIP_H */
