/* vsseg_hip.h — C ABI of libvsseg_hip.so: the MI355X (gfx950) hot path of the VS_Seg 2.5D attention U-Net.
 *
 * The reference (KCL-BMEIS/VS_Seg) has no FFI of its own: its seam is the Python object protocol between
 * `VSparams` and the model/loss objects.  This library sits *behind* that protocol; every entry
 * point below replaces the torch/ATen/cuDNN work the reference dispatches from the cited lines.  Plain pointers and
 * sizes only, no torch types; the caller owns every buffer; all calls are asynchronous on `stream` (a hipStream_t)
 * and return 0 or a negative VSSEG_E* code (text via vsseg_last_error()).
 *
 * Data layout: activations are channels-last [N][X][Y][Z][C] ("NDHWC", identical to torch.channels_last_3d strides
 * of a [N,C,X,Y,Z] tensor) described by vsseg_tensor; `pitch` lets a tensor be a channel slice of a wider buffer, and
 * `ptr2/csplit` let it be the concatenation of two dense tensors, so that the skip-connection concat (MONAI
 * SkipConnection, ref:params/networks/nets/unet2d5_spvPA.py:89) is never materialised by a copy.
 */
#ifndef VSSEG_HIP_H
#define VSSEG_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define VSSEG_F32 0
#define VSSEG_BF16 1

#define VSSEG_OK 0
#define VSSEG_EINVAL (-1)
#define VSSEG_ELAUNCH (-2)

#define VSSEG_ACT_NONE 0
#define VSSEG_ACT_PRELU 1
#define VSSEG_ACT_RELU 2
#define VSSEG_ACT_SIGMOID 3

#define VSSEG_RES_NONE 0
#define VSSEG_RES_ADD 1      /* out = f(acc) + res                      (ResidualUnit add, ref:.../convolutions.py:252-255) */
#define VSSEG_RES_RELUMASK 2 /* out = acc * (res > 0)                   (backward of the attention ReLU)                   */
#define VSSEG_RES_GATE 3     /* out = acc + res * (1 + gate[voxel])     (backward of AttentionBlock2 `att*x + x`, ref:.../attentionblock.py:43-47, fused
                              *  into the data gradient of the attention branch's first convolution: both flow into d(x))                          */

#define VSSEG_RES_IN1 5      /* out = f(acc) + in1[voxel] * in1_w[c] + in1_b[c]: a 1x1x1 convolution of a ONE-channel tensor added behind the activation (the first
                              *  ResidualUnit's residual convolution of the network input, ref:.../convolutions.py:241-255 with in_channels = 1): marching kernel only */

#define VSSEG_SEED_INDIRECT 0x80000000u /* OR-ed into a dropout `salt`: the `seed` argument is then the DEVICE ADDRESS of the 64-bit seed */

#define VSSEG_MAX_TAPS 27
#define VSSEG_STAT_SHARDS 256

typedef struct {
  void* ptr;     /* first element of the view (channel offset already applied) */
  int32_t dtype; /* VSSEG_F32 | VSSEG_BF16 */
  int32_t c;     /* channels in the view */
  int32_t pitch; /* elements between consecutive voxels (>= c, or >= max(csplit, c - csplit) for a two-part tensor) */
  int32_t n, x, y, z;
  /* Two-part tensors (the skip-connection concat, ref:params/networks/nets/unet2d5_spvPA.py:89 / MONAI SkipConnection):
   * channels [0, csplit) live at ptr, channels [csplit, c) at ptr2, both with the same pitch — the concat is the pair of
   * its (dense) operands and is never materialised.  ptr2 == NULL: ordinary tensor.  csplit must be a multiple of 16.
   * Accepted by vsseg_igemm (in, out, res), vsseg_wgrad (h) and vsseg_att_apply_fwd/bwd (x, dx); every other entry point
   * rejects it with VSSEG_EINVAL. */
  void* ptr2;
  int32_t csplit;
  int32_t reserved;  /* 0, or VSSEG_ZERO_PADDED on a destination: its channels c .. pitch-1 are zero padding the call may rewrite with zeros */
} vsseg_tensor;
#define VSSEG_ZERO_PADDED 1

/* Negative values of vsseg_igemm_desc.depth: which kernel runs the launch */
#define VSSEG_DEPTH_NOPREFETCH (-1)     /* the general kernel without prefetch: one halo buffer (half the LDS, more resident workgroups) */
#define VSSEG_DEPTH_STREAM (-2)         /* streaming kernel (sconv.hip) */
#define VSSEG_DEPTH_COMPUTE (-3)        /* compute kernel (cconv.hip) */
#define VSSEG_DEPTH_STREAM_SHUFFLE (-4) /* streaming kernel, fused output-parity classes */
#define VSSEG_DEPTH_MARCH (-5)          /* marching kernel (mconv.hip) */
#define VSSEG_DEPTH_MARCH_WREG (-6)     /* marching kernel, packed weights in registers */
#define VSSEG_DEPTH_DEEP (-7)           /* deep-level kernel (dconv.hip) */
#define VSSEG_DEPTH_TRANSITION (-8)     /* level 2 <-> 3 transition kernel (tconv.hip) */
#define VSSEG_DEPTH_GATHER (-9)         /* gathering marching kernel (gconv.hip) */

/* One implicit-GEMM launch over an output lattice q in [0,q): out[q*os+oo][n] = epi( sum_t sum_c in[q*is+off_t][c] * W[t][c][n] ).
 * Covers Conv3d forward, every parity class of ConvTranspose3d forward, and both data-gradients
 * (ref:params/networks/blocks/convolutions.py:114-146 and their autograd at ref:params/VSparams.py:461). */
typedef struct {
  vsseg_tensor in, out;
  int32_t q[3];            /* lattice extent */
  int32_t is[3], os[3], oo[3];
  int32_t ntaps;
  int32_t tap_off[VSSEG_MAX_TAPS][3]; /* input offset of each tap relative to q*is */
  int32_t tile[3];         /* output-lattice tile per workgroup; product must be 64*mtw */
  int32_t mtw;             /* 16-voxel M-tiles per wave: 1, 2 or 4 */
  int32_t nt;              /* 16-channel output tiles per workgroup (1..6) */
  int32_t nsplit;          /* output-channel splits (grid.y); packed weights hold nsplit*nt tiles */
  int32_t ck;              /* input channels staged per chunk (multiple of 8, divides padded Cin) */
  int32_t nchunks;
  int32_t ksteps;          /* K-steps (4 groups of 8 channels) per chunk */
  int32_t depth;           /* LDS-DMA prefetch distance in stages (1..3; 0 = 1): the halo ring holds depth+1 buffers.  Negative: one of the VSSEG_DEPTH_* selectors below — the general kernel without
                            * prefetch, or a specialised kernel with the same contract (outside its domain, or a value that is none of them: VSSEG_EINVAL, never a fallback).  The kernels' domains:
                            * VSSEG_DEPTH_TRANSITION (tconv.hip): class_split = 8 parity classes of a 3x3x3 stride-(2,2,2) transposed
                            * convolution / strided data gradient, 48 or 64 input and 48 output channels, tile 4x8x8 with mtw = 16, nt = 3, ck = in.c, bf16, plain / statistics / eval affine / accumulate epilogue;
                            * VSSEG_DEPTH_GATHER (gconv.hip): is = (2, 2, 1) 3x3x1 launches that read the fine level and write the coarse one — strided convolutions 16 -> 16 / 32 -> 32, data
                            * gradients of the transposed convolutions 32 -> 16 / 48 -> 32 —, tile = (x steps, 64 * mtw / tz rows, tz), ck = in.c in {16, 32}, one-part bf16 tensors, the same four epilogues */
  const void* wpack;       /* [nsplit][nchunks][ksteps][nt][64 lanes][8] in the compute dtype (== in.dtype) */
  /* epilogue: v = acc + bias; stats(v); v = v*scale+shift; v = act(v); residual; accumulate; store */
  const float* bias;       /* [cout] or NULL */
  const float* bias2;      /* second bias added to the first (merged 1x1x1 residual convolution) or NULL */
  const float* scale;      /* [cout] or NULL (eval-mode BatchNorm folded) */
  const float* shift;
  const float* alpha;      /* device pointer to the PReLU slope (1 element) */
  int32_t act;
  int32_t res_mode;
  vsseg_tensor res;
  int32_t accumulate;      /* out += value (gradient accumulation at fan-out points) */
  double* stats;           /* [VSSEG_STAT_SHARDS][2][cout_padded] sum / sum-of-squares of v, or NULL */
  int32_t stats_stride;    /* cout_padded */
  /* z-folded launches (a convolution without taps along z, with 1 real input or output channel, run on tensors whose 8
   * z-neighbours are reinterpreted as 8 channels; the packed weights are block-diagonal): output channel c of the launch is
   * real channel c % cout_mod for bias / bias2 / scale / shift / stats.  0: off. */
  int32_t cout_mod;
  const float* gate;       /* VSSEG_RES_GATE: fp32 attention map [N][X][Y][Z] of the output tensor, or NULL */
  const float* in_gate;    /* fp32 attention map [N][X][Y][Z] of the INPUT tensor, or NULL: input voxel v is multiplied by (1 + in_gate[v]) on load
                            * (AttentionBlock2 folded into the convolution that reads its output; marching kernel, VSSEG_DEPTH_MARCH, only) */
  /* All output-parity classes of a strided transposed convolution / data gradient in ONE launch of the general kernel (class_split = number of
   * classes, 2..8; 0 = off): `nsplit` = class_split, workgroup row s of the grid computes class s — ALL output channels (out.c = nt*16) at output
   * voxels q*os + class_oo[s] — from the class's own taps class_tap[s][0..class_ntaps[s]) (indices into tap_off, which lists the union of the classes'
   * input offsets; oo must be 0).  wpack is [class][nchunks][ksteps][nt][64][8] with ksteps = the largest class's; a class runs only its own K-steps.
   * One read of the halo table, one launch and one weight staging per class instead of 8 launches of 15-40 us on levels 3-5. */
  int32_t class_split;
  int32_t class_oo[8][3];
  int32_t class_ntaps[8];
  int32_t class_tap[8][8];
  /* A 1x1x1 convolution of the SAME input riding along (the ResidualUnit's residual convolution, ref:params/networks/blocks/convolutions.py:241-255; marching kernel,
   * VSSEG_DEPTH_MARCH / _MARCH_WREG, plain or statistics epilogue only): res_tiles more 16-channel output tiles that run only the K-steps of the centre tap; the input is read once
   * for both convolutions.  res_out.ptr != NULL: their values (+ bias_res) are stored there (bf16) — training, where the add sits behind the BatchNorm pass;
   * res_out.ptr == NULL: they are added to the main tiles behind their activation — eval: out = act(bn(conv(x))) + residual(x).  0: off. */
  int32_t res_tiles;
  const void* wpack_res;   /* [K-steps of the centre tap][res_tiles][64 lanes][8] in the compute dtype (planner.residual_tile_pack_map) */
  const float* bias_res;   /* [res_out.c] or NULL */
  vsseg_tensor res_out;
  const void* in1;         /* VSSEG_RES_IN1: one-channel tensor [N][X][Y][Z] in the compute dtype (bf16) */
  const float* in1_w;      /* [cout] weights and */
  const float* in1_b;      /* [cout] bias of the 1 -> cout convolution */
} vsseg_igemm_desc;

/* Weight gradient: dW[t][cP][cH] += sum_q P[q][cP] * H[q*hs + off_t][cH]  (fp32 atomics into the flat grad buffer).
 * Conv3d: P = dY, H = X.  ConvTranspose3d: P = X, H = dY. */
typedef struct {
  vsseg_tensor p, h;
  int32_t q[3];            /* lattice = spatial extent of P */
  int32_t hs[3];
  int32_t ntaps;
  int32_t tap_off[VSSEG_MAX_TAPS][3];
  int32_t tap_widx[VSSEG_MAX_TAPS]; /* flat index of the tap inside the weight's kernel dims */
  int32_t tile[3];         /* product must be a multiple of 32 */
  int32_t ntp;             /* 16-channel tiles of P */
  float* dw;               /* destination weight-gradient tensor (pre-zeroed or holding earlier contributions) */
  int64_t stride_p, stride_h, stride_tap; /* element strides of dw along cP, cH, tap */
  int32_t cp_valid, ch_valid;
  int32_t persistent_blocks;
  float* scratch;          /* partial-sum slabs: >= ceil(ch_valid/16) * ntaps * ntp*16 * 16 floats per workgroup */
  int64_t scratch_elems;   /* capacity in floats; the number of persistent workgroups is clamped to what fits */
  int32_t single_buffer;   /* 1: no prefetch, one LDS tile buffer (half the LDS, more resident workgroups); 0: double-buffered */
  int32_t hgroup;          /* 16-channel chunks of H one workgroup multiplies with the P tile it fetched (1..4; 0 = 1): P is read ceil(chunks/hgroup) times.
                            * Clamped by the library to a divisor of the chunk count that fits registers / LDS. */
  float* dbias_p;          /* optional: dbias_p[cP] += sum_q P[q][cP] (bias gradient of a convolution without BatchNorm, P = dY) or NULL */
  int32_t march;           /* 1: the marching kernel (csrc/mwgrad.hip; stride-1 3x3x1 bf16 only, outside its domain is an error): tile = (x steps per
                            * workgroup, rows per workgroup, z slices per workgroup in {2, 4, 8}); persistent_blocks / single_buffer / hgroup unused */
  const float* h_gate;     /* march = 1 only: fp32 attention map [N][X][Y][Z] of H, or NULL: H[v] is multiplied by (1 + h_gate[v]) on load (the gated
                            * tensor `att.repeat(C) * x + x` of AttentionBlock2 as the convolution input, never materialised) */
} vsseg_wgrad_desc;

/* Fused backward of one stride-1 3x3x1 Convolution block, Conv3d -> BatchNorm3d(train) -> Dropout -> PReLU (ref:params/networks/blocks/convolutions.py:114-156,
 * differentiated by loss.backward() at ref:params/VSparams.py:461): the second BatchNorm-backward pass (what vsseg_bn_act_bwd_apply computes) is applied ON LOAD,
 * and the data gradient and the weight gradient of the convolution are formed from the same LDS planes in ONE marching launch (csrc/mbwd.hip) — the
 * gradient of the convolution output is never written to HBM.  Call after vsseg_bn_act_bwd_reduce + vsseg_bn_act_bwd_finalize of the layer.  bf16 only;
 * outside its instantiated shapes the call fails with VSSEG_EINVAL (no fallback). */
typedef struct {
  vsseg_tensor y, dout;    /* convolution output before BatchNorm, gradient of the block output: [N][X][Y][Z][cout] */
  vsseg_tensor x;          /* convolution input [N][X][Y][Z][cin] */
  vsseg_tensor dx;         /* OUT: data gradient of x (overwritten) */
  const float *mean, *invstd, *gamma, *scale, *shift, *alpha; /* as for vsseg_bn_act_bwd_apply */
  const float *mean_dz, *mean_dzx;
  float p_drop;
  const uint8_t* keep;     /* keep-mask bytes written by vsseg_bn_act_fwd (required when p_drop > 0) */
  const void* wpack;       /* packed weights of the data gradient: [ksteps][nt][64 lanes][8] bf16 of the marching conv_dgrad plan (K = 9 * cout -> N = cin) */
  float* dw;               /* IN/OUT: weight gradient [cout][cin][3][3][1] fp32, += */
  int32_t tile[3];         /* (x steps per workgroup, rows per workgroup, z slices per workgroup in {2, 4, 8}); rows * z a multiple of 64 */
  float* scratch;          /* partial-sum slabs: (cout/16) * (9, or 10 with a residual convolution) * cin * 16 floats per workgroup */
  int64_t scratch_elems;
  /* Optional: the ResidualUnit's 1x1x1 residual convolution of the SAME input x (ref:params/networks/blocks/convolutions.py:241-255) rides along: dx also gets
   * Wr' dres, dw_res[cout][cin] += sum_q dres[q] x[q].  dres.ptr == NULL: no residual convolution.  dres may be the tensor `dout` itself (single-subunit units). */
  vsseg_tensor dres;       /* gradient of the residual convolution's output [N][X][Y][Z][cout] */
  const void* wpack_res;   /* packed weights of its data gradient: [ksteps][nt][64][8] bf16 of the conv_dgrad plan of the 1x1x1 convolution (K = cout -> N = cin, one chunk) */
  float* dw_res;           /* IN/OUT: its weight gradient [cout][cin] fp32, += */
  const float* x_gate;     /* optional fp32 attention map [N][X][Y][Z] of x: x[v] is multiplied by (1 + x_gate[v]) on load (AttentionBlock2 in front of the unit, never
                            * materialised; x may then be the two-part concat); dx is the gradient of the GATED tensor.  64 input channels with dres == dout only. */
} vsseg_conv_bwd_desc;
int vsseg_conv_bwd_fused(const vsseg_conv_bwd_desc* d, void* stream);

/* Two consecutive stride-1 3x3x1 convolutions of an INFERENCE forward as one launch (csrc/chain.hip; bf16):
 *   h   = act_a(scale_a * (conv_a(in) + bias_a) + shift_a)                         conv + eval-mode BatchNorm (folded) + PReLU, ref:params/networks/blocks/convolutions.py:114-146
 *   out = act_b(scale_b * (conv_b(h) + bias_b) + shift_b) [+ in * in1_w + in1_b]
 * h (cmid channels) lives in LDS only.  The pairs of the sliding-window predictor (ref:params/VSparams.py:553-567): the first ResidualUnit of the encoder, 1 -> 16 -> 16 with the
 * 1x1x1 residual convolution of the one-channel input added behind the second activation (ref:params/networks/blocks/convolutions.py:241-255), and the attention block of the
 * finest decoder level, 32 -> 16 -> 1 + sigmoid (ref:params/networks/blocks/attentionblock.py:20-41).  Results are bit-identical to the two vsseg_igemm marching launches
 * (VSSEG_DEPTH_MARCH) with the same packed weights.  With a BatchNorm in stage A it is not applicable in training (the BatchNorm needs the
 * statistics of all of h first). */
typedef struct {
  vsseg_tensor in;         /* bf16: a multiple of 8 channels (16-byte aligned voxel rows; may be two-part) or a COMPACT one-channel tensor (c = pitch = 1) standing for one zero-extended group */
  vsseg_tensor out;        /* same extent; bf16 with a multiple of 4 channels (<= 32), or 1..3 channels bf16 / fp32 (the attention map: c = 1, fp32) */
  int32_t cmid;            /* channels of h (16 or 32) */
  const void* wpack_a;     /* [K-steps of 9 taps x in channels][cmid / 16][64 lanes][8] bf16: the packed weights of conv_a's marching plan (planner.pack_map, nt = cmid / 16) */
  const float *bias_a, *scale_a, *shift_a; /* [cmid]; scale_a / shift_a NULL: 1 / 0 */
  const float* alpha_a;    /* device pointer to the PReLU slope of stage A */
  int32_t act_a;           /* VSSEG_ACT_NONE | VSSEG_ACT_PRELU | VSSEG_ACT_RELU */
  const void* wpack_b;     /* [K-steps of 9 taps x cmid][ceil(out.c / 16)][64 lanes][8] bf16 */
  const float *bias_b, *scale_b, *shift_b; /* [out.c] or NULL */
  const float* alpha_b;
  int32_t act_b;           /* VSSEG_ACT_* */
  const float *in1_w, *in1_b; /* [out.c] each or both NULL: + in[voxel] * in1_w[c] + in1_b[c] behind act_b (compact one-channel input only) */
  int32_t res_tiles;       /* 0, or ceil(out.c / 16): + bf16(residual(in) + bias_res) behind act_b, residual = a 1x1x1 convolution of `in` (the ResidualUnit's residual convolution,
                            * ref:params/networks/blocks/convolutions.py:241-255; ordinary multi-channel input only) */
  const void* wpack_res;   /* [K-steps of conv_a's centre tap][res_tiles][64 lanes][8] bf16 (planner.residual_tile_pack_map) */
  const float* bias_res;   /* [out.c] or NULL */
  int32_t tz;              /* plan: z voxels per workgroup column (1, 2, 4 or 8; in.z a multiple) */
  int32_t mtw;             /* ... 16-voxel M-tiles per wave: a workgroup owns ALL rows, in.y == waves * mtw * 16 / tz */
  int32_t lx;              /* ... x positions per workgroup (a segment re-fetches 4 input planes and recomputes 2 planes of h) */
  int32_t waves;           /* ... waves per workgroup: 4, 8 or 16 */
  int32_t lead;            /* ... iterations between the fetch of an input plane and its use: 1 (several small workgroups per CU) or 3 (one large one; always 3 for a compact input) */
} vsseg_chain_desc;
int vsseg_conv_chain(const vsseg_chain_desc* d, void* stream);
int vsseg_conv_chain_lds_bytes(const vsseg_chain_desc* d); /* LDS bytes of the launch, or VSSEG_EINVAL (vsseg_last_error: why the descriptor is outside the kernel's domain) */

const char* vsseg_last_error(void);
/* Forking a second stream without a marker packet on the first (ABI version 7).  Between vsseg_fork_arm(ev) and vsseg_fork_disarm() every kernel this library launches on the
   calling thread carries `ev` as the stop event of its own dispatch (a later kernel replaces an earlier one); vsseg_fork_disarm returns how many kernels carried it.
   vsseg_stream_wait_event(stream, ev) = hipStreamWaitEvent.  The training backward forks its weight-gradient stream this way: a hipEventRecord on the main stream delays the main
   stream's next kernel by ~5 us, 42 times per step. */
void* vsseg_fork_event_create(void);
int vsseg_fork_event_destroy(void* ev);
int vsseg_fork_arm(void* ev);
int vsseg_fork_disarm(void);
int vsseg_stream_wait_event(void* stream, void* ev);
int vsseg_version(void); /* 22: + vsseg_ball_scratch_bytes, vsseg_ball_morphology; 20: + vsseg_loss_opts, vsseg_ce_focal_sums, vsseg_loss_finalize, vsseg_loss_pred_bwd, vsseg_loss_pred_bwd_to; 19: + vsseg_surface_metrics; 18: + vsseg_fill_holes, vsseg_remove_small_components; 17: + vsseg_measure_scratch_bytes, vsseg_measurements; 16: + vsseg_topk_scratch_bytes, vsseg_topk_select, vsseg_ce_topk_select, vsseg_dice_ce_topk_finalize, vsseg_dice_ce_topk_pred_bwd, vsseg_dice_ce_topk_pred_bwd_to; 15: + vsseg_grad_norm_scratch_bytes, vsseg_grad_norm, vsseg_sgd, vsseg_adam_clipped, vsseg_clip_record; 14: + vsseg_ce_sums, vsseg_dice_ce_finalize, vsseg_dice_ce_pred_bwd, vsseg_dice_ce_pred_bwd_to; 13: + vsseg_patch_filter, vsseg_patch_tone; 12: + vsseg_crop_field, vsseg_field_job; 11: + vsseg_crop_affine, vsseg_affine_job; 10: + vsseg_swi_finalize_mirrored, vsseg_crop_job.flip is a three-axis mirror mask (was flip_x); 9: + vsseg_components_scratch_bytes, vsseg_components_label, vsseg_keep_largest_component; 8: + vsseg_surface_distances, vsseg_surface_scratch_bytes; 7: + vsseg_dice_pred_bwd_to, vsseg_dice_level_sums, vsseg_dice_tail_sums, vsseg_dice_att_bwd_levels, vsseg_fork_*, vsseg_stream_wait_event; 6: + launch plans with depth -8 (transition kernel) and -9 (gathering marching kernel); 5: vsseg_wgrad march = 2 (compute weight-gradient kernel), + vsseg_conv_to1, vsseg_conv_chain_desc without h_out (the training variant measured no gain and was deleted); 4: + vsseg_conv_chain; 3: the BatchNorm-block-on-load fields (in_bn_*, keep_*, x_bn_*: round-4 experiment, measured a loss, deleted) left the descriptors, depth -7 plans;
                            * 2: fixed-point accumulators documented + vsseg_fx_status; 1: the buffers below were described as plain doubles */

/* ---- Accumulator buffers are 64-bit FIXED-POINT integers, not doubles ------------------------------------------------------------------
 * Every `double*` accumulator of this ABI — vsseg_igemm_desc.stats and vsseg_bn_finalize's `stats`, the `sums` / `alpha_acc` of
 * vsseg_bn_act_bwd_reduce / _finalize, the `pred_sums` / `att_sums` of vsseg_dice_* — is declared `double*` for its size and alignment only:
 * each 8-byte slot holds a two's-complement int64 = round(value * scale), added to with integer atomics so that the total does not depend on
 * the order in which workgroups finish (a training step is run-to-run bit-identical).  Zero bytes are the value 0, so callers keep zero-filling
 * the buffers (vsseg_memset_zero) exactly as before; callers that READ or PRE-FILL a slot must use the scale of its family:
 *     VSSEG_FX_STAT_SCALE  2^20  BatchNorm forward statistics (sum, sum of squares);         per-workgroup partial |v| < 4.3e9
 *                                cross-entropy sums (vsseg_ce_sums)
 *     VSSEG_FX_GRAD_SCALE  2^44  BatchNorm / PReLU backward sums (sums, alpha_acc)           per-workgroup partial |v| < 256
 *     VSSEG_FX_DICE_SCALE  2^32  Dice sums (pred_sums, att_sums)                              per-workgroup partial |v| < 1.0e6
 * (vsseg_hard_dice_counts keeps REAL doubles: its sums are integers, exact in fp64 in any order.)
 * A partial sum outside its range, or a NaN / Inf one, is clamped and sets a sticky per-process device flag; while the flag is set the decoding
 * kernels (vsseg_bn_finalize, vsseg_bn_act_bwd_finalize, vsseg_dice_finalize, vsseg_dice_ce_finalize, vsseg_dice_ce_topk_finalize, vsseg_loss_finalize) return NaN, so a diverging run or an out-of-range loss scale
 * surfaces as NaN in the loss / statistics / gradients instead of as wrapped integers.  vsseg_fx_status reads (and optionally clears) the flag. */
typedef double vsseg_fx_acc; /* one accumulator slot (reinterpret as int64_t) */
#define VSSEG_FX_STAT_SCALE 1048576.0
#define VSSEG_FX_GRAD_SCALE 17592186044416.0
#define VSSEG_FX_DICE_SCALE 4294967296.0
static inline vsseg_fx_acc vsseg_fx_encode(double value, double scale) {
  union { int64_t i; double d; } u;
  double s = value * scale;
  u.i = (int64_t)(s < 0 ? s - 0.5 : s + 0.5);
  return u.d;
}
static inline double vsseg_fx_decode(vsseg_fx_acc slot, double scale) {
  union { int64_t i; double d; } u;
  u.d = slot;
  return (double)u.i / scale;
}
/* Returns 1 if a fixed-point partial sum was non-finite or out of range since the last reset, 0 if not, < 0 on error.  Synchronises `stream`.
 * reset != 0 clears the flag (after the caller has handled the diverged step). */
int vsseg_fx_status(int32_t reset, void* stream);

int vsseg_igemm(const vsseg_igemm_desc* d, void* stream);
int vsseg_igemm_lds_bytes(const vsseg_igemm_desc* d);
int vsseg_wgrad(const vsseg_wgrad_desc* d, void* stream);
/* Weight gradient of a 3x3x1 (k3 = 3) or 1x1x1 (k3 = 1) stride-1 convolution with ONE input or ONE output channel, as a bandwidth reduction
 * (no MFMA, no zero-extended operand):  dw[c*stride_c + tap] += sum_v t[v][c] * s[v + sign*off_tap],  zero padding.
 * t: the C-channel tensor (C = 8, 16, 32 or 64; y extent a multiple of 4), s: the one-channel field [N][X][Y][Z] in t's dtype.
 * Conv3d 1 -> C: t = dY, s = X, sign = +1.  Conv3d C -> 1: t = X, s = dY (its one real channel, compact), sign = -1.  stride_c = taps. */
int vsseg_wgrad_narrow(vsseg_tensor t, const void* s, int32_t k3, int32_t sign, float* dw, int64_t stride_c,
                       float* dbias /* sign = -1 only, or NULL: *dbias += sum_v s[v], the bias gradient of the C -> 1 convolution */,
                       float* scratch /* partial-sum slabs: >= k3*k3*C + 1 floats per workgroup */, int64_t scratch_elems, void* stream);
/* vsseg_wgrad_narrow for the 1 -> C, 3x3x1 convolution of a Convolution block (ref:params/networks/blocks/convolutions.py:114-156) with T = d(conv output) formed ON
 * LOAD from y (the convolution output), dout (the gradient of the block output) and the forward's keep-mask bytes — the second BatchNorm-backward pass, bit-identical
 * to vsseg_bn_act_bwd_apply, which is then not launched and d(conv output) is never written (the network input needs no data gradient).  bf16 only. */
int vsseg_wgrad_narrow_bn(vsseg_tensor y, vsseg_tensor dout, const uint8_t* keep, const float* mean, const float* invstd, const float* gamma, const float* scale, const float* shift, const float* alpha,
                          const float* mean_dz, const float* mean_dzx, float p_drop, const void* s, float* dw, int64_t stride_c, float* scratch, int64_t scratch_elems, void* stream);

/* Forward of a stride-1 3x3x1 convolution with ONE output channel (+ bias, + sigmoid): the second convolution of AttentionBlock1 on the two finest levels
 * (ref:params/networks/blocks/attentionblock.py:20-35: conv2 = Convolution(C/2 -> 1, conv_only) followed by Sigmoid).  A bandwidth kernel on the vector ALUs
 * (csrc/nconv.hip): every input voxel is read once, the output voxel's nine taps are partial sums exchanged between neighbouring threads.  in: one-part bf16,
 * 16 or 32 channels, y extent 16 .. 256 (a power of two; a workgroup owns all rows), z a multiple of 512 / y.  w: the fp32 master weights [1][C][3][3][1]
 * (rounded to bf16 inside, as the packed weights of the MFMA launches are).  out: dense one-channel fp32 / bf16 tensor of the input's extent.  lx: x planes per
 * workgroup (<= 0: all).  Outside this domain the call fails with VSSEG_EINVAL (no fallback: the caller lowers vsseg_igemm instead). */
int vsseg_conv_to1(vsseg_tensor in, const float* w, const float* bias /* [1] or NULL */, int32_t act /* VSSEG_ACT_NONE | VSSEG_ACT_SIGMOID */, vsseg_tensor out, int32_t lx, void* stream);

/* dst[i] = map[i] >= 0 ? cast(src[map[i]]) : 0 — (re)packs the fp32 master weights into MFMA fragment order. */
int vsseg_gather_cast(const float* src, const int32_t* map, const int32_t* map2 /* optional second addend, or NULL */, void* dst, int64_t n, int32_t dst_dtype, void* stream);
/* A 1x1x1 residual convolution merged into the centre tap of the k-tap convolution it is added to (last_conv_only ResidualUnit,
 * ref:params/networks/blocks/convolutions.py:217-255): its gradients are the centre-tap slice / the bias gradient of the merged conv. */
int vsseg_merge_residual_grads(const float* dw, const float* db, float* dwr, float* dbr, int32_t cout, int32_t cin, int32_t ktaps, int32_t centre, void* stream);

/* dst[n][x][y][z][0..cpad) <- src window (crop + zero-pad outside + zero-extend channels + cast). src is [N][SX][SY][SZ] f32, 1 channel.
 * Used for the network input (ref:params/VSparams.py:456) and for sliding-window crops (MONAI sliding_window_inference step 6). */
int vsseg_stage_input(const float* src, int32_t n, const int32_t sdims[3], const int32_t origin[3], vsseg_tensor dst, void* stream);

/* BatchNorm statistics: reduce shards -> mean, invstd, scale = gamma*invstd, shift = beta - mean*scale; running-stat update
 * (torch BatchNorm3d training semantics, momentum 0.1, unbiased running var; ref:.../convolutions.py:152). */
int vsseg_bn_finalize(const double* stats, int32_t stride, int32_t c, double count, const float* gamma, const float* beta, float eps, float momentum,
                      float* running_mean, float* running_var, int64_t* num_batches, float* mean, float* invstd, float* scale, float* shift, void* stream);
/* eval mode: scale = gamma/sqrt(rv+eps), shift = beta - rm*scale for every BN layer at once (flat param addressing). */
int vsseg_bn_fold_eval(const float* gamma, const float* beta, const float* rm, const float* rv, float eps, float* scale, float* shift, int32_t c, void* stream);

/* out = PReLU(dropout(y*scale+shift)) [+ res]   (ref:.../convolutions.py:148-156; residual add :252-255).
 * Dropout: keep-mask from Philox4x32-10(seed, salt, element index); p = 0 disables.  salt | VSSEG_SEED_INDIRECT: `seed` holds the
 * device address of the seed (every dropout entry point), so that a launch list with fixed arguments can be replayed with a new seed.
 * keep_out (or NULL): [voxels * c/8] bytes — the forward stores the keep-mask of every 8-channel group there, and a backward pass given the
 * same buffer as keep_in reads it instead of running Philox again (the three BN kernels are VALU-bound on the generator, not on HBM;
 * NULL regenerates the bit-identical mask from (seed, salt, element index)). */
int vsseg_bn_act_fwd(vsseg_tensor y, const float* scale, const float* shift, const float* alpha, float p_drop, uint64_t seed, uint32_t salt,
                     vsseg_tensor res, int32_t has_res, vsseg_tensor out, uint8_t* keep_out, void* stream);
/* Same with the residual computed on the fly as the 1x1x1 convolution of a ONE-channel tensor: res[v][c] = x1[v]*res_w[c] + res_b[c]
 * (first encoder ResidualUnit, in_channels = 1, ref:params/networks/blocks/convolutions.py:241-255); x1 is [N][X][Y][Z] in y's dtype. */
int vsseg_bn_act_fwd_res1(vsseg_tensor y, const float* scale, const float* shift, const float* alpha, float p_drop, uint64_t seed, uint32_t salt,
                          const void* x1, const float* res_w, const float* res_b, vsseg_tensor out, uint8_t* keep_out, void* stream);
/* Backward, pass 1: sums[shard][0][c] += dz, [1][c] += dz*xhat, [2][c] += dout, alpha_acc[shard] += dA*d(d<0). */
int vsseg_bn_act_bwd_reduce(vsseg_tensor y, vsseg_tensor dout, const float* mean, const float* invstd, const float* gamma, const float* beta,
                            const float* scale, const float* shift, /* the forward's folded affine: the PReLU/dropout branch is re-decided on the SAME fp32 value */
                            const float* alpha, float p_drop, uint64_t seed, uint32_t salt, double* sums, int32_t stride, double* alpha_acc, const uint8_t* keep_in, void* stream);
/* finalize: dgamma, dbeta, dalpha (+= into flat grads) and the two per-channel means used by pass 2 */
int vsseg_bn_act_bwd_finalize(const double* sums, int32_t stride, const double* alpha_acc, int32_t c, double count, float* dgamma, float* dbeta, float* dalpha,
                              float* mean_dz, float* mean_dzx, float* dres_bias /* += sum(dout) or NULL */, void* stream);
/* pass 2: dy = gamma*invstd*(dz - mean_dz - xhat*mean_dzx) */
int vsseg_bn_act_bwd_apply(vsseg_tensor y, vsseg_tensor dout, const float* mean, const float* invstd, const float* gamma, const float* beta,
                           const float* scale, const float* shift, const float* alpha, float p_drop, uint64_t seed, uint32_t salt, const float* mean_dz, const float* mean_dzx, vsseg_tensor dy,
                           const uint8_t* keep_in, void* stream);
/* debug/parity: write the keep-mask (0/1 as f32, [voxel][c]) the forward used */
int vsseg_dropout_mask(float* mask, int64_t nvox, int32_t c, float p_drop, uint64_t seed, uint32_t salt, void* stream);

/* AttentionBlock2: out = x * (1 + att)   (ref:params/networks/blocks/attentionblock.py:43-47); att is f32 [voxel]. */
int vsseg_att_apply_fwd(vsseg_tensor x, const float* att, vsseg_tensor out, void* stream);
/* dx (+)= dout*(1+att);  dpre[voxel][0] = (sum_c dout*x + datt_ext) * att*(1-att)  (sigmoid backward), channels 1..7 zero. */
/* accumulate_dx: 0 dx = dout*(1+att); 1 dx += ...; 2 dx is not written (its contribution is fused into a VSSEG_RES_GATE igemm launch). */
int vsseg_att_apply_bwd(vsseg_tensor x, const float* att, vsseg_tensor dout, const float* datt_ext, vsseg_tensor dx, int32_t accumulate_dx, vsseg_tensor dpre,
                        float* dbias /* += sum(dpre): bias gradient of the sigmoid convolution, or NULL */,
                        void* dpre1 /* optional compact [N,X,Y,Z] copy of channel 0 of dpre (x's dtype), or NULL */, void* stream);

/* generic helpers */
int vsseg_store_u64(uint64_t* dst, uint64_t value, void* stream);                 /* *dst = value by a one-thread kernel (the per-step dropout seed of a replayed launch list) */
int vsseg_memset_zero(void* dst, int64_t bytes, void* stream);                    /* hipMemsetAsync(dst, 0, bytes) on the caller's stream */
int vsseg_copy_bytes(const void* src, void* dst, int64_t bytes, void* stream);    /* device-to-device hipMemcpyAsync */
int vsseg_channel_sum(vsseg_tensor t, float* out /* [c], += */, void* stream);
int vsseg_add_inplace(vsseg_tensor dst, vsseg_tensor src, void* stream); /* dst += src */
int vsseg_copy_cast(vsseg_tensor src, vsseg_tensor dst, void* stream);  /* dst[v][0..c) = src[v][0..c) (fp32 / bf16 either side); fp32 [v][2] -> VSSEG_ZERO_PADDED bf16 rows of 8: one full-row store per voxel */

/* Dice_spvPA (ref:params/losses/dice_spvPA.py:238-297).  sums layout: see loss.hip. */
int vsseg_maxpool_label(const float* src, int32_t n, const int32_t sdims[3], const int32_t ratio[3], float* dst, void* stream);
int vsseg_dice_pred_sums(const float* logits, int32_t pitch, const float* label, int32_t n, int64_t nvox, int32_t hardness, double* sums /* [n][2][3] */, void* stream);
int vsseg_dice_att_sums(const float* att, const float* label, int32_t n, int64_t nvox, double* sums /* [n][3] */, void* stream);
int vsseg_dice_finalize(const double* pred_sums, const double* att_sums, int32_t n, int32_t nlevels, float* loss, float* coef /* [n][2][2] + [levels][n][2] */, void* stream);
int vsseg_dice_pred_bwd(const float* logits, int32_t pitch, const float* label, int32_t n, int64_t nvox, int32_t hardness, const float* coef, const float* gscale, float* dlogits, void* stream);
int vsseg_dice_att_bwd(const float* label, int32_t n, int64_t nvox, const float* coef, float inv_levels, const float* gscale, float* datt, void* stream);
/* The same sums with fewer passes and launches (the fused train step; the values feed the same vsseg_dice_finalize):
   vsseg_dice_level_sums — one pass over a level whose NEXT level pools (2, 2, 1) (the two finest levels of the 2.5D network): att_sums[n][3] of `att` against `label`,
   pooled = MaxPool3d((2,2,1))(label) (NULL: not wanted) and, when `logits` is given ([n][dims][2], the finest level), pred_sums[n][2][3].  dims must be made of
   2 x 2 x 4 blocks, operands 16-byte aligned.
   vsseg_dice_tail_sums — the remaining (coarse) levels in one launch: level i's label = MaxPool3d(sdims / dims[i])(src) is written to label[i] (NULL allowed when
   dims[i] == sdims: the level is src itself) and sums[i][n][3] are those of att[i] against it. */
#define VSSEG_DICE_MAX_LEVELS 8
typedef struct {
  int32_t n, nlevels;
  const float* src;   /* [n][sdims] */
  int32_t sdims[3];
  const float* att[VSSEG_DICE_MAX_LEVELS];
  float* label[VSSEG_DICE_MAX_LEVELS];
  int32_t dims[VSSEG_DICE_MAX_LEVELS][3];
  double* sums;       /* [nlevels][n][3], fixed-point (see below) */
} vsseg_dice_tail_desc;
int vsseg_dice_level_sums(const float* logits, const float* att, const float* label, int32_t n, const int32_t dims[3], int32_t hardness, double* pred_sums, double* att_sums, float* pooled, void* stream);
int vsseg_dice_tail_sums(const vsseg_dice_tail_desc* d, void* stream);
/* vsseg_dice_att_bwd of several levels in one launch: datt[i][b][v] = coef[i][b][0] * label[i][b][v] + coef[i][b][1] (times *gscale when given) */
typedef struct {
  int32_t n, nlevels;
  const float* label[VSSEG_DICE_MAX_LEVELS];
  float* datt[VSSEG_DICE_MAX_LEVELS];
  const float* coef[VSSEG_DICE_MAX_LEVELS]; /* this level's [n][2] slice of vsseg_dice_finalize's coef */
  int64_t nvox[VSSEG_DICE_MAX_LEVELS];
  const float* gscale;                      /* NULL = 1 */
} vsseg_dice_bwd_levels_desc;
int vsseg_dice_att_bwd_levels(const vsseg_dice_bwd_levels_desc* d, void* stream);
/* vsseg_dice_pred_bwd writing the gradient in a layout the training plan stages it in (the fused train step of vs_seg_amd.parallel.DataParallelTrainer: no fp32
   gradient tensor, no cast pass): dst = 2 channels of `n * nvox` voxels, fp32 or bf16 (round-to-nearest-even, as vsseg_copy_cast), pitch 2, or pitch 8 =
   VSSEG_ZERO_PADDED rows whose channels 2..7 are written as zeros (bf16) / left as they are (fp32).  gscale may be NULL (= 1). */
int vsseg_dice_pred_bwd_to(const float* logits, int32_t pitch, const float* label, int32_t n, int64_t nvox, int32_t hardness, const float* coef, const float* gscale, vsseg_tensor dst, void* stream);

/* A voxel-wise cross-entropy term beside the Dice loss (ABI version 14; what MONAI users know as DiceCELoss, the default loss of nnU-Net):
 *     loss = Dice_spvPA + ce_weight * CE,   CE = sum_{b,v} w[y] * (-log softmax(x_{b,v})[y]) / sum_{b,v} w[y],   w = (1, ce_foreground_weight)
 * = ce_weight * torch.nn.functional.cross_entropy(logits, y, weight=[1, ce_foreground_weight]): ONE mean over all n * nvox voxels of the batch, final logits only (the
 * attention-map terms and the hardness weight do not enter).  Label cast: y = 1 where (int)label == 1, else 0 — the cast of the Dice kernels.
 *   value     of a voxel: softplus(z) = max(z, 0) + log1p(exp(-|z|)) with z = x[1-y] - x[y]: finite for every finite logit (-log(p_y) is inf once p_y underflows)
 *   gradient  of a voxel: ce_weight * w[y] / W * (softmax(x) - onehot(y)), W = N_bg + ce_foreground_weight * N_fg, times *gscale where given, formed from the OTHER class's
 *             probability — (+k p0, -k p0) for y = 1, (-k p1, +k p1) for y = 0 — because p_y - 1 cancels once p_y rounds to 1
 * vsseg_ce_sums — one pass over logits and label: ce_sums[0..2] += (S_bg, S_fg, N_fg), the CE sums over the background / foreground voxels and the foreground count of
 *   the whole batch.  The slots are fixed-point accumulators (below) of scale VSSEG_FX_STAT_SCALE (2^20), NOT VSSEG_FX_DICE_SCALE: a voxel's value is |z|, not bounded by 1
 *   (batch 4 of 384x128x128 with every |z| = 100: 4.9e6 per workgroup — 2^32 leaves room for 1.0e6, 2^20 for 4.3e9; resolution 2^-20 per workgroup, <= 512 workgroups,
 *   on a sum that is divided by W >= the voxel count).  Zero the three slots first.  A NaN / Inf partial sum sets the sticky flag like every other accumulator.
 * vsseg_dice_ce_finalize — vsseg_dice_finalize that also decodes ce_sums: loss += ce_weight * (S_bg + w_fg * S_fg) / W in fp64 before the one cast to fp32, and
 *   ce_coef[0..1] = (ce_weight / W, ce_weight * w_fg / W) in device memory for the backward (no host read of N_fg).  coef is vsseg_dice_finalize's, unchanged.  While the
 *   fixed-point flag is set the loss and all coefficients are NaN.
 * vsseg_dice_ce_pred_bwd / _to — vsseg_dice_pred_bwd / _to with the CE gradient of the voxel added in fp32 to the Dice gradient and the sum stored ONCE, in every layout
 *   (a second pass would round the bf16 operand twice).  With ce_weight == 0 callers use the plain entry points: same launches and bits as before version 14. */
int vsseg_ce_sums(const float* logits, int32_t pitch, const float* label, int32_t n, int64_t nvox, double* ce_sums /* [3] */, void* stream);
int vsseg_dice_ce_finalize(const double* pred_sums, const double* att_sums, int32_t n, int32_t nlevels, const double* ce_sums, int64_t nvox, double ce_weight, double ce_foreground_weight, float* loss, float* coef,
                           float* ce_coef /* [2] */, void* stream);
int vsseg_dice_ce_pred_bwd(const float* logits, int32_t pitch, const float* label, int32_t n, int64_t nvox, int32_t hardness, const float* coef, const float* ce_coef, const float* gscale, float* dlogits, void* stream);
int vsseg_dice_ce_pred_bwd_to(const float* logits, int32_t pitch, const float* label, int32_t n, int64_t nvox, int32_t hardness, const float* coef, const float* ce_coef, const float* gscale, vsseg_tensor dst, void* stream);

/* The cross-entropy term over the HARDEST voxels only (ABI version 16; nnU-Net's Dice + TopK loss, DC_and_topk_loss with k = 10).  N = n * nvox voxels of the batch,
 * K = max(1, floor(N * P / 100)) computed by the caller from the shapes, P in (0, 100]:
 *     loss = Dice_spvPA + ce_weight * TopK,   TopK = (1 / K) * (sum of the K largest v_i),   v_i = w[y_i] * softplus(z_i)
 * with y, z, softplus and w = (1, ce_foreground_weight) as above, evaluated in fp32
 * = ce_weight * F.cross_entropy(logits, y, weight=[1, w_fg], reduction='none').flatten().topk(K).values.mean().  THE DIVISION IS BY K, as in nnU-Net and torch, NOT by the
 * weight sum W of the plain term; at P = 100 and w_fg = 1 the two terms are equal up to rounding.  The K voxels are those of the WHOLE BATCH of the call: in data-parallel
 * training each rank selects among the voxels of its own batch (nnU-Net's DDP behaviour).
 *   With t the K-th largest value, n_gt = #{v_i > t}, n_eq = #{v_i = t} (order-independent, ties included):
 *   value     (S_gt + (K - n_gt) * t) / K,  S_gt = sum of the v_i > t
 *   gradient  of a voxel: ce_weight * w[y] / K * c_i * (softmax(x) - onehot(y)), c_i = 1 where v_i > t, (K - n_gt) / n_eq where v_i = t (the tied voxels share what is
 *             left of K; one voxel at the threshold: torch's gradient), 0 below t; formed from the other class's probability and added in fp32 to the Dice gradient
 *             before the one store, as vsseg_dice_ce_pred_bwd does.
 * Values are ranked by their KEY: the uint32 bit pattern of the fp32 value (non-negative floats order like their bits), -0 as 0, a NaN as 0xFFFFFFFF — a NaN is always
 * selected: the loss is NaN and the sticky fixed-point flag is set, as with vsseg_ce_sums.
 * The select is a radix select, digits of 11 + 11 + 10 bits: three histogram passes over the elements (per-workgroup LDS histograms, flushed with integer atomics),
 * each followed by a one-workgroup scan that leaves the digit in the record; nothing is read by the host.  scratch: vsseg_topk_scratch_bytes() bytes of device memory,
 * 8-byte aligned, owned by the caller and ZEROED before every select (vsseg_memset_zero, together with the loss sums).  Its first 32 bytes are the result:
 *     offset  0  uint32  threshold_bits   key of the K-th largest element
 *     offset  4  uint32  passes_done      3 once the record is complete
 *     offset  8  uint64  n_gt             elements with a key above the threshold
 *     offset 16  uint64  n_eq             elements with the threshold's key        (n_gt < K <= n_gt + n_eq)
 *     offset 24  uint64  K
 * (both counts come from the histograms: there is no counting pass); the rest is the state that goes from kernel to kernel (vs_seg_amd/csrc/topk.h), S_gt included:
 * a fixed-point accumulator of scale VSSEG_FX_STAT_SCALE (the range argument of vsseg_ce_sums) filled by the LAST histogram pass, plus the part that the last
 * histogram itself determines (a bin of the last digit is one bit pattern: count * value, exact in fp64) — no pass for the sum either.
 * vsseg_topk_select — the select over an array of n values, 1 <= k <= n: the machinery on its own (no sum).  Negative values are outside the contract.
 * vsseg_ce_topk_select — keys are the v_i, computed on the fly from logits and label (vsseg_ce_sums's two load paths).
 * vsseg_dice_ce_topk_finalize — vsseg_dice_finalize that also decodes the record: loss += ce_weight * value in fp64 before the one cast, and
 *   topk_coef[0..7] = (ce_weight / K, ce_weight * w_fg / K, the tie share (K - n_gt) / n_eq, threshold_bits (uint32), (float)w_fg, 0, 0, 0) in device memory for the
 *   backward.  While the fixed-point flag is set the loss and the five coefficients are NaN (the threshold's bits 0xFFFFFFFF).
 * vsseg_dice_ce_topk_pred_bwd / _to — vsseg_dice_ce_pred_bwd / _to that recompute v_i, compare its key with the threshold and scale the voxel's cross-entropy gradient
 *   by c_i.  The select, the sum and the backward evaluate v_i by ONE device function with floating-point contraction off: the same bits in all of them. */
int64_t vsseg_topk_scratch_bytes(void);
int vsseg_topk_select(const float* values, int64_t n, int64_t k, void* scratch, void* stream);
int vsseg_ce_topk_select(const float* logits, int32_t pitch, const float* label, int32_t n, int64_t nvox, double ce_foreground_weight, int64_t k, void* scratch, void* stream);
int vsseg_dice_ce_topk_finalize(const double* pred_sums, const double* att_sums, int32_t n, int32_t nlevels, const void* topk_scratch, double ce_weight, double ce_foreground_weight, float* loss, float* coef,
                                float* topk_coef /* [8] */, void* stream);
int vsseg_dice_ce_topk_pred_bwd(const float* logits, int32_t pitch, const float* label, int32_t n, int64_t nvox, int32_t hardness, const float* coef, const float* topk_coef, const float* gscale, float* dlogits,
                                void* stream);
int vsseg_dice_ce_topk_pred_bwd_to(const float* logits, int32_t pitch, const float* label, int32_t n, int64_t nvox, int32_t hardness, const float* coef, const float* topk_coef, const float* gscale, vsseg_tensor dst,
                                   void* stream);

/* Region and focal options of the loss for small lesions (ABI version 20): the Tversky index (Salehi 2017; MONAI's TverskyLoss), its focal variant (Abraham 2019), one
 * ratio over the pooled sums of the batch (nnU-Net's batch_dice) and the focal cross-entropy (MONAI's DiceFocalLoss) — with the two Tversky terms the "Unified Focal" family
 * of Yeung 2022.  I, G, P are the three sums of a ratio as above (per sample and class for the logits, hardness-weighted when that is on; per level and sample for the
 * attention maps), eps = 1e-5, beta = tversky_beta in (0, 1), alpha = 1 - beta, gamma = focal_tversky_gamma in [0.25, 4]:
 *     T = (2 I + eps) / (2 a_P P + 2 a_G G + eps),   u = 1 - T,   term = u when gamma == 1, max(u, 1e-7)^gamma otherwise
 *   (a_P, a_G) = (alpha, beta) for the foreground class of the logits and for every attention map: a_P weights the false positives P - I, a_G the false negatives G - I;
 *   the background class of the logits is mirrored, (a_P, a_G) = (beta, alpha): its false positives are the foreground's false negatives.  beta > 0.5 makes a missed
 *   tumour voxel cost more than a false positive; beta = 0.5 is the Dice ratio (2 I + eps) / (G + P + eps).
 *   The floor 1e-7 is part of the definition (with gamma < 1 the derivative gamma u^(gamma - 1) is unbounded at a perfect prediction): below it the term is the constant
 *   1e-7^gamma and every coefficient of that ratio is 0.
 *   batch_dice: I, G, P are summed over the n samples of the call before the ratio is formed — one ratio per class, one per level; under data parallelism these are the
 *   samples of the rank (no collective).  The weights of the terms are unchanged: the mean over the 2 n (or 2 pooled) logits ratios plus 1 / L times the mean over each
 *   level's ratios.
 *   coefficients: with `region` the finalize leaves THREE per logits ratio, coef[n][2][3] = (dL/dI, dL/dG, dL/dP), followed by the attention maps' [levels][n][2] =
 *   (dL/dI, dL/dP) as before — vsseg_dice_att_bwd / _levels serve unchanged, given the slice at coef + 6 n.  Pooled ratios write the same coefficients for every sample.
 *   With region == 0 the layout is vsseg_dice_finalize's ([n][2][2] + [levels][n][2]) and so are the values.
 * Focal cross-entropy, gamma_c = ce_focal_gamma in [0, 5] (ce_mode VSSEG_CE_FOCAL), with y, z = x[1-y] - x[y], w and W = N_bg + w_fg N_fg of the plain term above:
 *     loss += ce_weight * sum_{b,v} w[y] q^gamma_c softplus(z) / W,   q = sigmoid(z) = 1 - p_y        (gamma_c -> 0: the plain term)
 *   value     q^gamma_c = exp(-gamma_c softplus(-z)) — never log(q) of a rounded probability: finite for every finite logit
 *   gradient  dz = ce_weight w[y] / W * q^gamma_c * (gamma_c (1 - q) softplus(z) + q) goes to the OTHER class's logit and -dz to the label's own
 * vsseg_ce_focal_sums — vsseg_ce_sums with the focal factor: the same three slots (S_bg, S_fg, N_fg) at scale VSSEG_FX_STAT_SCALE; q^gamma_c <= 1 bounds the values by
 *   the plain term's.  A NaN logit sets the sticky flag.
 * vsseg_loss_finalize — the finalize of every combination: `ce_state` is ce_sums (VSSEG_CE_PLAIN, VSSEG_CE_FOCAL: ce_coef[2] as vsseg_dice_ce_finalize leaves it), the
 *   select's scratch (VSSEG_CE_TOPK: ce_coef[8] as vsseg_dice_ce_topk_finalize leaves it) or NULL (VSSEG_CE_NONE).  nvox: voxels per sample.
 * vsseg_loss_pred_bwd / _to — d(loss)/d(logits) of every combination, fp32 tensor / staged layouts (vsseg_dice_pred_bwd_to's).  Per voxel, with g the one-hot label,
 *   s = d w / d p and t = d(w p) / d p of the hardness weight (0 and 1 without it): d/dp = A g t + B_G g s + B_P t with (A, B_G, B_P) = coef of the ratio.
 * Every number of the record is checked before anything is launched (VSSEG_EINVAL); nothing is read by the host; while the fixed-point flag is set the loss and all
 * coefficients are NaN. */
#define VSSEG_CE_NONE 0
#define VSSEG_CE_PLAIN 1
#define VSSEG_CE_TOPK 2
#define VSSEG_CE_FOCAL 3
typedef struct {
  int32_t region;              /* 0: the Dice ratio per sample, two coefficients per ratio (vsseg_dice_finalize); 1: the ratio above, three per logits ratio */
  int32_t batch_dice;          /* 1: pool the sums of the n samples before the ratio (needs region) */
  double tversky_beta;         /* in (0, 1)      (read with region) */
  double focal_tversky_gamma;  /* in [0.25, 4]   (read with region) */
  int32_t ce_mode;             /* VSSEG_CE_* */
  int32_t reserved;            /* 0 */
  double ce_weight;            /* finite, >= 0   (read with ce_mode != VSSEG_CE_NONE, as the two below) */
  double ce_foreground_weight; /* finite, > 0 */
  double ce_focal_gamma;       /* in [0, 5]      (read with VSSEG_CE_FOCAL) */
} vsseg_loss_opts;
int vsseg_ce_focal_sums(const float* logits, int32_t pitch, const float* label, int32_t n, int64_t nvox, double ce_focal_gamma, double* ce_sums /* [3] */, void* stream);
int vsseg_loss_finalize(const double* pred_sums, const double* att_sums, int32_t n, int32_t nlevels, const void* ce_state, int64_t nvox, const vsseg_loss_opts* opts, float* loss, float* coef, float* ce_coef,
                        void* stream);
int vsseg_loss_pred_bwd(const float* logits, int32_t pitch, const float* label, int32_t n, int64_t nvox, int32_t hardness, const float* coef, const float* ce_coef, const vsseg_loss_opts* opts, const float* gscale,
                        float* dlogits, void* stream);
int vsseg_loss_pred_bwd_to(const float* logits, int32_t pitch, const float* label, int32_t n, int64_t nvox, int32_t hardness, const float* coef, const float* ce_coef, const vsseg_loss_opts* opts, const float* gscale,
                           vsseg_tensor dst, void* stream);

/* torch.optim.Adam(lr, weight_decay) over the flat parameter buffer (ref:params/VSparams.py:388-391,462). */
int vsseg_adam(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps, float wd, float bc1, float bc2, float gscale, void* stream);

/* ---- gradient-norm clipping, SGD and AdamW over the same flat buffers (ABI version 15; beyond the reference, whose only optimiser is the Adam above) --------------
 * The clip record: 64 bytes of device memory, 8-byte aligned, owned and zeroed by the caller (zeroing it again resets the statistics).  vsseg_grad_norm writes it, the
 * update kernels read it, the host reads it only when it wants the statistics — nothing on the step path waits for the norm. */
typedef struct {
  double norm;      /*  0: L2 norm of gscale * g of the last vsseg_grad_norm call (NaN / Inf when the gradient held one) */
  float coef;       /*  8: min(1, max_norm / (norm + 1e-6)), formed in fp64 and rounded once (torch.nn.utils.clip_grad_norm_); 0 when skip is set */
  int32_t skip;     /* 12: 1 when the norm is NaN or Inf: the update kernels then leave parameters and optimiser state bitwise untouched */
  int64_t steps;    /* 16: calls since the record was zeroed */
  int64_t clipped;  /* 24: of them with a finite norm and coef < 1 */
  int64_t skipped;  /* 32: of them with skip = 1 */
  double norm_sum;  /* 40: sum of the finite norms */
  double norm_max;  /* 48: largest finite norm */
  int64_t reserved; /* 56 */
} vsseg_clip_record;
#define VSSEG_GRAD_NORM_SHARD 8192 /* elements per partial sum (one workgroup pass) */
#define VSSEG_GRAD_NORM_FINAL 256  /* partials the finalising workgroup consumes per pass */
/* vsseg_grad_norm — norm = |gscale| * sqrt(sum g[i]^2) over n elements, every square and every addition in fp64 (an fp32 square of 1e-30 is 0, of 1e25 is Inf).  Stage 1:
 *   partial s = the sum over the elements [s * SHARD, (s + 1) * SHARD) in a fixed in-workgroup order, stored to scratch[s].  Stage 2: one workgroup adds the partials
 *   (thread t: t, t + FINAL, ... in that order, then a fixed tree) and writes the record.  No atomics, no dependence on the grid: the same gradient gives the same bits on
 *   every run and every rank.  scratch: vsseg_grad_norm_scratch_bytes(n) bytes, 8-byte aligned, overwritten.  n == 0: norm 0, coef 1.  g may be null only then.
 *   VSSEG_EINVAL (before any launch): null / misaligned pointers, n < 0, max_norm not finite or <= 0, gscale not finite, too little scratch.
 * vsseg_sgd — torch.optim.SGD(lr, momentum, dampening 0, weight_decay, nesterov): g' = coef * gscale * g + wd * p; buf = momentum * buf + g' (a zeroed buf reproduces torch's
 *   first step); d = nesterov ? g' + momentum * buf : buf; p -= lr * d.  momentum == 0: d = g', buf is not touched and may be null.  VSSEG_EINVAL: null pointers, n < 0,
 *   momentum outside [0, 1), nesterov with momentum 0.
 * vsseg_adam_clipped — vsseg_adam with the gradient multiplied by coef; decoupled != 0: torch.optim.AdamW (p *= 1 - lr * wd first, no wd * p in the gradient).  With
 *   record == NULL and decoupled == 0 it IS vsseg_adam (same launch, same bits).
 * Both updates: record may be NULL (coef 1, never skipped); with record->skip set they return before their first store.  n == 0: no launch. */
int64_t vsseg_grad_norm_scratch_bytes(int64_t n); /* bytes of scratch, or VSSEG_EINVAL */
int vsseg_grad_norm(const float* g, int64_t n, float gscale, double max_norm, double* scratch, int64_t scratch_bytes, vsseg_clip_record* record, void* stream);
int vsseg_sgd(float* p, const float* g, float* buf, int64_t n, float lr, float momentum, float wd, int32_t nesterov, float gscale, const vsseg_clip_record* record, void* stream);
int vsseg_adam_clipped(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps, float wd, float bc1, float bc2, float gscale, int32_t decoupled,
                       const vsseg_clip_record* record, void* stream);

/* ---- data side: the reference's MONAI transform chain on volumes cached in HBM -------------------- */
/* One crop of one cached volume: RandFlipd(spatial_axis=0) then RandSpatialCropd / SpatialPadd's zero padding
 * (ref:params/VSparams.py:208-222).  origin is in flipped + padded coordinates and may be negative.  Since ABI version 10 the last field is a mirror MASK (bit 0 = x,
 * bit 1 = y, bit 2 = z; 0 and 1 mean what flip_x = 0 / 1 meant): the source coordinate of a mirrored axis is sdims-1-g, taken before the zero-padding test. */
typedef struct {
  const float* src;     /* [sx][sy][sz] fp32, z contiguous (the reference's X,Y,Z array order) */
  int32_t sdims[3];
  int32_t origin[3];
  int32_t flip;
} vsseg_crop_job;
/* dst[j][rx][ry][rz] for j < njobs; `jobs` is a DEVICE array of vsseg_crop_job structs, image and label of every batch element. */
int vsseg_crop_flip(const void* jobs, int32_t njobs, float* dst, const int32_t roi[3], void* stream);
/* Random rotation / scaling / intensity / noise augmentation of a crop (ABI version 11): what MONAI users know as RandAffined + RandScaleIntensityd + RandShiftIntensityd +
 * RandGaussianNoised, as ONE resampling gather per batch.  The kernel knows a 3x4 matrix and an intensity map per job, nothing about angles, mirrors or labels.
 *   coordinates  for the output voxel p = (x, y, z) of dst[j][x][y][z] the source coordinate, in voxel units of the cached volume, is evaluated in fp32 as
 *                  s_i = fmaf(m[4i+2], z, fmaf(m[4i+1], y, fmaf(m[4i], x, m[4i+3])))            (explicit fused operations: no dependence on the compiler's contraction)
 *   interp 0     trilinear: i0 = floorf(s), f = s - i0 per axis; the eight taps (i0 + a, a in {0,1}^3) carry the products of f (a = 1) and 1 - f (a = 0).  A tap outside the
 *                volume contributes exactly 0 (SpatialPadd's constant padding, continuous across the border): the VALUE is selected, the address of an outside tap is
 *                never formed or read, so neighbouring memory (NaN or not) cannot leak in.
 *   interp 1     nearest: index floorf(s + 0.5f) per axis, 0 outside the volume.
 *   intensity    v = fmaf(v, gain, bias); then, when noise_std != 0, v = fmaf(noise_std, n, v).
 *   noise        for the flattened patch index i = (x*ry + y)*rz + z of a job: g = i >> 2, k = i & 3,
 *                  r = philox4x32_10(counter = (lo32 g, hi32 g, noise_stream, 0), key = (lo32 seed, hi32 seed)),   u(w) = ((w >> 8) + 0.5f) * 2^-24   (fp32 arithmetic),
 *                  (n0, n1) = sqrtf(-2 logf(u(r.x))) * (cosf, sinf)(6.2831853f * u(r.y)),   (n2, n3) likewise from r.z, r.w;   n = n_k   (accurate logf / sincosf).
 *   labels       are jobs with interp = 1, gain = 1, bias = 0, noise_std = 0.
 * `jobs_dev` is the DEVICE array the kernel reads, `jobs_host` the caller's host copy of the same njobs records: the argument checks read the host copy (the entry point never
 * reads device memory, synchronises or allocates), so that null pointers, njobs < 1, a non-positive roi or sdims, an interp outside {0, 1} and a non-finite m / gain / bias /
 * noise_std are VSSEG_EINVAL before anything is launched.  A coordinate that is not finite or far outside the volume (a finite but absurd m) reads nothing and gives bias. */
typedef struct {
  const float* src;     /* [sx][sy][sz] fp32, z contiguous */
  int32_t sdims[3];
  int32_t interp;       /* 0 trilinear, 1 nearest */
  float m[12];          /* row-major 3x4: output index (x, y, z, 1) -> source coordinate */
  float gain, bias, noise_std;
  uint32_t noise_stream;
} vsseg_affine_job;
/* dst[j][rx][ry][rz] for j < njobs (16-byte aligned), one launch for image and label jobs of a whole batch. */
int vsseg_crop_affine(const vsseg_affine_job* jobs_host, const void* jobs_dev, int32_t njobs, float* dst, const int32_t roi[3], uint64_t seed, void* stream);
/* Elastic deformation and MR bias field on top of vsseg_crop_affine (ABI version 12): what MONAI users know as Rand3DElastic (in-plane) and RandBiasField.  Both are one smooth
 * random field over the PATCH, a 2-vector d for the deformation and a scalar b for the bias: a coarse lattice of random control values interpolated by uniform cubic
 * B-splines, evaluated inside the same gather.
 *   lattice      n_a = (roi_a - 1) / spacing_a + 4 nodes along axis a (integer division); node id n = (i*n_y + j)*n_z + k (64 bits);
 *                  r = philox4x32_10(counter = (lo32 n, hi32 n, noise_stream, 1), key = (lo32 seed, hi32 seed))     (fourth counter word 1: the noise uses 0, no counter is shared)
 *                  c_x, c_y, c_b = fmaf(2, u(r.x | r.y | r.z), -1) in [-1, 1), u as for the noise; r.w is unused.  noise_stream is the field stream too: the image job and the
 *                label job of one sample carry the same stream and so get the same deformation.
 *   field        at the output voxel p, per axis: i0 = p_a / spacing_a, f = (p_a mod spacing_a) / spacing_a; the weights
 *                  B0 = (1-f)^3/6,  B1 = (3f^3 - 6f^2 + 4)/6,  B2 = (-3f^3 + 3f^2 + 3f + 1)/6,  B3 = f^3/6
 *                apply to the nodes i0 .. i0+3, and F(c)(p) is the tensor-product sum over 4 x 4 x 4 nodes.  d_x = elastic_mag * F(c_x), d_y = elastic_mag * F(c_y), d_z = 0
 *                (in-plane only, like the rotation: the voxels are 0.4 x 0.4 x 1.5 mm), b = bias_log * F(c_b).  |F| <= 1, so |d| <= elastic_mag (voxels) and |b| <= bias_log.
 *                The fp32 evaluation order of F is not part of the contract; its error is: |F_fp32 - F_exact| <= 96 * 2^-24 (derived in tests/field_oracle.py).
 *   coordinates  x' = x + d_x, y' = y + d_y in fp32, then exactly the three fmaf of vsseg_crop_affine on (x', y', z): the deformation acts in patch space, and the matrix
 *                rotates, zooms and mirrors it with the patch.
 *   intensity    on the interpolated value v = v * expf(b) (accurate expf), then gain, bias and noise exactly as in vsseg_crop_affine.  Label jobs carry elastic_mag and bias_log = 0.
 *   zero ranges  with elastic_mag == 0 and bias_log == 0 in every job the launch is bit-identical to vsseg_crop_affine (x + 0, v * expf(0)).
 *   no folding   elastic_mag <= min(spacing_x, spacing_y) / 4 is required: the derivative of a cubic B-spline expansion is a convex combination of neighbouring control
 *                differences (each below 2 * elastic_mag) divided by the spacing, so every partial of d is below 2 * elastic_mag / spacing and the in-plane Jacobian
 *                determinant is above 1 - 4 * elastic_mag / spacing > 0.
 *   limit        the kernel holds one x-reduced plane of the lattice on chip: n_y * n_z <= 1024, otherwise VSSEG_EINVAL (choose a larger spacing).
 * Argument checks, on the host copy and before anything is launched: everything vsseg_crop_affine checks, spacing_a >= 1, elastic_mag and bias_log finite and >= 0, the
 * bound on elastic_mag and the lattice limit.  No atomics: a launch is bit-reproducible run to run. */
typedef struct {
  const float* src;     /* the fields of vsseg_affine_job, in its order ... */
  int32_t sdims[3];
  int32_t interp;
  float m[12];
  float gain, bias, noise_std;
  uint32_t noise_stream;
  float elastic_mag;    /* ... then the bound of the control-point displacement, in voxels of the patch */
  float bias_log;       /* and the bound of the log of the multiplicative bias */
} vsseg_field_job;
int vsseg_crop_field(const vsseg_field_job* jobs_host, const void* jobs_dev, int32_t njobs, float* dst, const int32_t roi[3], const int32_t spacing[3], uint64_t seed, void* stream);
/* Appearance augmentation of the image patches of a training batch (ABI version 13), applied AFTER the crop launch (vsseg_crop_flip, _affine or _field) in the fixed order
 * blur -> low resolution -> contrast -> gamma.  Blur and low resolution read in-plane neighbours of the resampled patch and contrast and gamma need statistics of the whole
 * patch, so none of them fits into the gather.  Both filters act in-plane only (x and y), like the rotation, the zoom and the elastic field: the voxels are 0.4 x 0.4 x 1.5 mm.
 *
 * vsseg_patch_filter: random Gaussian blur and simulated low-resolution acquisition.  src, dst and scratch are [njobs][rx][ry][rz] fp32 with z contiguous, 16-byte aligned,
 * src != dst; job j reads patch j of src (and of scratch) and writes patch j of dst, nothing else.
 *   reflect      reflect(i, n) is the edge-repeating reflection (..., 1, 0 | 0, 1, ..., n-1 | n-1, n-2, ...) of period 2n: m = i mod 2n (0 <= m < 2n), m < n ? m : 2n-1-m.
 *                It is defined for every i, because the roi may be shorter than the radius.  The halo of a job comes from the reflection alone: no address outside the
 *                job's own patch is formed or read.
 *   blur         radius R = `radius` (0: no blur), half-taps w_k = taps[k], k = 0..R, with w_0 + 2 sum_{k>=1} w_k = 1.  u = G_y(G_x(v)) with
 *                  G_a(v)[p] = sum_{k=-R..R} w_|k| * v[reflect(p_a + k, roi_a)]                (the other two coordinates of p unchanged)
 *                G_x(v) is rounded to fp32 before G_y reads it; each sum is accumulated in fp32, its order is not part of the contract (the error of a sum of 2R+1 terms
 *                is derived in tests/appearance_oracle.py).  The caller makes the taps: R = ceil(3 sigma) <= 5, w_k proportional to exp(-k^2 / (2 sigma^2)).
 *   low res      reads u (v when radius == 0).  n_a = coarse[a] samples along in-plane axis a (n_a == roi_a on both axes: no low resolution).  Coarse sample i sits at the
 *                source index q_a(i) = floor((2i + 1) * roi_a / (2 n_a)) (integer arithmetic).  Output index p has the coarse coordinate, in fp32 with a correctly
 *                rounded division,
 *                  t = clamp(((p + 0.5) * n_a) / roi_a - 0.5, 0, n_a - 1),   i0 = floor(t), i1 = min(i0 + 1, n_a - 1), phi = t - i0
 *                (an axis with n_a == roi_a takes i0 = i1 = p, phi = 0 without evaluating t).  With (i0, i1, phi_x) along x and (j0, j1, phi_y) along y the value is
 *                  lo = fmaf(phi_y, u[q_x(i0)][q_y(j1)] - u[q_x(i0)][q_y(j0)], u[q_x(i0)][q_y(j0)]),   hi = the same at q_x(i1),   out = fmaf(phi_x, hi - lo, lo)
 *                at the output's own z: nearest-neighbour down-sampling to n_x x n_y, bilinear up-sampling back.  n_a == roi_a returns u bit-exactly.
 *   neither      a job with radius == 0 and coarse == roi in-plane is a plain copy, bit for bit.
 *   launches     one kernel blurs (or copies); a second one, launched only when a job has low resolution, gathers.  A job with both families passes u through its patch of
 *                `scratch`, which may be null when no job has both (VSSEG_EINVAL otherwise).  No atomics: a launch is bit-reproducible run to run.
 * Argument checks, on the host copy and before anything is launched (the entry point never reads device memory, synchronises or allocates): no null pointers, src != dst,
 * njobs >= 1, 1 <= roi_a <= 65535, 16-byte alignment, 0 <= radius <= 5, with radius > 0 finite taps with |w_0 + 2 sum w_k - 1| <= 1e-5, 1 <= coarse_a <= roi_a. */
typedef struct {
  int32_t radius;       /* 0: no blur */
  float taps[6];        /* w_0 .. w_radius */
  int32_t coarse[2];    /* n_x, n_y; == roi in-plane: no low resolution */
} vsseg_filter_job;
int vsseg_patch_filter(const vsseg_filter_job* jobs_host, const void* jobs_dev, int32_t njobs, const float* src, float* dst, float* scratch, const int32_t roi[3], void* stream);
/* vsseg_patch_tone: contrast about the mean with the value range preserved (batchgenerators' ContrastAugmentation with preserve_range) and a gamma curve over the value range
 * (MONAI's RandAdjustContrast), in place on x = [njobs][n] fp32.  A job with contrast == 1 and gamma == 1 is left untouched (its stats are set to 0); every other job:
 *   pass 1       mn = min, mx = max, S = sum of its n values.  S is an fp64 sum over a FIXED assignment of elements to VSSEG_TONE_SHARDS shards: element i belongs to chunk
 *                i / 1024, chunk c to shard c mod VSSEG_TONE_SHARDS; the shards are combined in a fixed order.  No floating-point atomics: a launch is bit-reproducible
 *                run to run.  `work` is device scratch of njobs * VSSEG_TONE_SHARDS * 3 doubles (S, mn, mx of every shard); it needs no initialisation.
 *   statistics   mu = (float)(S / n);  stats[4j .. 4j+3] = {mn, mx, mu, 0} is left filled for inspection, like acc2 of vsseg_normalize_intensity.
 *   pass 2       with c = contrast, g = gamma and the contrast map
 *                  T(x) = fminf(fmaxf(fmaf(x - mu, c, mu), mn), mx)   (x - mu rounded to fp32),        T(x) = x when c == 1
 *                a = T(mn), b = T(mx), r = b - a, y = T(x);  out = y when g == 1, otherwise
 *                  out = fmaf(powf((y - a) / (r + 1e-7f), g), r, a)             (accurate powf and division)
 *                A constant patch (r = 0) comes out unchanged and finite.
 * nnU-Net rescales the result of its gamma transform to the mean and standard deviation the patch had before (retain_stats); that is deliberately left out: it would add
 * another reduction pass over the patch.  The inverted-image gamma variant is out of scope.
 * Argument checks, on the host copy and before anything is launched: no null pointers, njobs >= 1, n >= 1, contrast and gamma finite and in (0, 2). */
#define VSSEG_TONE_SHARDS 128
typedef struct {
  float contrast, gamma;  /* 1, 1: the job is left untouched */
} vsseg_tone_job;
int vsseg_patch_tone(const vsseg_tone_job* jobs_host, const void* jobs_dev, int32_t njobs, float* x, int64_t n, float* stats, double* work, void* stream);
/* Acquisition artefacts on the image patches of a training batch (ABI version 21), applied AFTER the crop launch and BEFORE vsseg_patch_filter / vsseg_patch_tone (an artefact
 * of the acquisition precedes post-hoc appearance changes): thick slices along z, phase-encode ghosting along x or y and a k-space spike, what TorchIO users know as
 * RandomAnisotropy, RandomGhosting and RandomSpike.  Each has an exact image-domain form for the cases below, so no FFT is taken.  Motion and Gibbs ringing are out of scope.
 * src, dst and scratch are [njobs][rx][ry][rz] fp32 with z contiguous, 16-byte aligned, src != dst; job j reads patch j of src (and of scratch) and writes patch j of dst,
 * nothing else.  The order is fixed, y = S(G(T(v))), and the result of each stage is rounded to fp32 before the next stage reads it.
 *   thick T      f = `thick` (1: off, v passes bit-exactly), o = `thick_offset`, 0 <= o < f.  Slab of z: k(z) = (z + o) / f (integer division); the first and the last slab of
 *                a column may be short, and (rz - 1 + o) / f == 0 is one slab.  m_k = the fp32 sum of the slab's voxels in ascending z, divided by their count (correctly
 *                rounded); c_k = (first + last z index of the slab) / 2, a multiple of 0.5 and exact in fp32.  For the output z with k = k(z): the pair (a, b) is (k, k+1)
 *                if z >= c_k and (k-1, k) otherwise; a pair that leaves the range of slabs collapses to the end slab with phi = 0, otherwise
 *                  phi = (z - c_a) / (c_b - c_a)   (fp32, correctly rounded division),        out = fmaf(phi, m_b - m_a, m_a)
 *                slab means along z, interpolated linearly back between the slab centres: a thick-slice acquisition resampled to the grid of the patch.
 *   ghosting G   axis a = `ghost_axis` (0 = x, 1 = y), N = roi_a, n = `ghosts` (0: off; otherwise n >= 2 divides N), s = N / n, alpha = `ghost_alpha` in (0, 1], u the input
 *                of the stage.  In k-space along a every n-th line is scaled by 1 - alpha and the DC line is left alone (TorchIO's rule); in image space, which is the
 *                contract, for the voxel at index i of a line along a:
 *                  mu = (float)(sum of the N voxels of the line in fp64 / N),     S = sum_{j=0..n-1} u[(i + j s) mod N]   (fp32; the order is not part of the contract),
 *                  c = alpha / n   (fp32, correctly rounded),                      out = fmaf(alpha, mu, fmaf(-c, S, u[i]))
 *                n copies of the line, shifted by multiples of s, are subtracted with weight alpha / n and the mean is put back: the mean of every line is preserved and a
 *                constant line comes out unchanged, both up to the rounding bound derived in tests/acquisition_oracle.py.
 *   spike S      amp = `spike_amp` (0: off), (kx, ky) = `spike_k`, phase = `spike_phase`, w the input of the stage.  In k-space amp rx ry / 2 e^{+-i phase} is added at
 *                (kx, ky) and at (-kx, -ky) of every z slice; in image space, at the voxel (x, y, z):
 *                  t = ((kx x mod rx) ry + (ky y mod ry) rx) mod (rx ry)   (64-bit integers: the phase is reduced before any rounding, the argument stays below 2 pi + phase),
 *                  theta = fmaf(6.2831853f, (float)t / (float)(rx ry), phase),     out = fmaf(amp, cosf(theta), w)     (accurate cosf, correctly rounded division)
 *   neutral      a job with thick == 1, ghosts == 0 and spike_amp == 0 is a plain copy, bit for bit.
 *   launches     at most two kernels: one forms T, one G and S (and the copy).  A job with thick slices AND ghosting or a spike passes T(v) through its patch of `scratch`,
 *                which may be null when no job needs it (VSSEG_EINVAL otherwise).  No atomics: a launch is bit-reproducible run to run.
 * Argument checks, on the host copy and before anything is launched (the entry point never reads device memory, synchronises or allocates): no null pointers, src != dst,
 * 1 <= njobs <= 65535, 1 <= roi_a <= 65535, 16-byte alignment, 1 <= thick <= 8, 0 <= thick_offset < thick, ghost_axis in {0, 1}, ghosts 0 or (>= 2 and a divisor of roi_axis),
 * with ghosts != 0 ghost_alpha finite and in (0, 1], spike_amp and spike_phase finite, with spike_amp != 0: 0 <= spike_k < roi in-plane and not (0, 0). */
typedef struct {
  int32_t thick;          /* slab height f in voxels along z, 1: off */
  int32_t thick_offset;   /* o, 0 <= o < f */
  int32_t ghost_axis;     /* 0 = x, 1 = y */
  int32_t ghosts;         /* n >= 2 dividing roi[ghost_axis]; 0: off */
  float   ghost_alpha;    /* in (0, 1] when ghosts != 0 */
  float   spike_amp;      /* 0: off */
  int32_t spike_k[2];     /* 0 <= kx < rx, 0 <= ky < ry, not both 0 when spike_amp != 0 */
  float   spike_phase;    /* radians, in [0, 2 pi) */
} vsseg_acquisition_job;
int vsseg_patch_acquisition(const vsseg_acquisition_job* jobs_host, const void* jobs_dev, int32_t njobs, const float* src, float* dst, float* scratch, const int32_t roi[3], void* stream);
/* NormalizeIntensityd (ref:params/VSparams.py:213): y = (x - mean) / std over all n voxels (population std; std == 0: no
 * division).  acc2 = 2 doubles of device scratch (sum, sum of squares; left filled for inspection). */
int vsseg_normalize_intensity(const float* x, float* y, int64_t n, double* acc2, void* stream);

/* Sliding-window blend (MONAI sliding_window_inference steps 6-7; call site ref:params/VSparams.py:568-574). */
/* (seg == NULL: only cnt += w — the weight map of a window geometry, which does not depend on the data; cnt == NULL: only out += w * seg) */
int vsseg_swi_accumulate(const float* seg /* [rx][ry][rz][c] */, const float* imap /* [rx][ry][rz] */, const int32_t roi[3], const int32_t start[3], int32_t c,
                         float* out /* [PX][PY][PZ][c] */, float* cnt /* [PX][PY][PZ] */, const int32_t pdims[3], void* stream);
int vsseg_swi_finalize(const float* out, const float* cnt, const int32_t pdims[3], const int32_t pad_before[3], const int32_t dims[3], int32_t c, float* dst /* [X][Y][Z][c] */, void* stream);
/* One pass of mirrored test-time augmentation (ABI version 10): `out` / `cnt` are the blend of SWI(flip_m(volume)) in the padded frame of the MIRRORED volume, `mirror` is m as in
   vsseg_crop_job.flip.  For every image voxel g: v[k] = out[o*c+k] / cnt[o] (the quotient of vsseg_swi_finalize, bit for bit) at o = pad_before + g', g' = dims-1-g on the mirrored
   axes; softmax != 0: v = softmax of v over the c channels; then dst[g*c+k] = (first ? v[k] : dst[g*c+k] + v[k]) * scale.  The caller passes scale = 1 on every pass but the
   last, where it is 1 / number of passes (a power of two: exact). */
int vsseg_swi_finalize_mirrored(const float* out, const float* cnt, const int32_t pdims[3], const int32_t pad_before[3], const int32_t dims[3], int32_t c, int32_t mirror, int32_t softmax,
                                int32_t first, float scale, float* dst /* [X][Y][Z][c] */, void* stream);
/* hard Dice of argmax vs label (ref:params/VSparams.py:393-408): counts[0]=|P∩G|, [1]=|P|, [2]=|G| */
int vsseg_hard_dice_counts(const float* logits, int32_t pitch, const float* label, int64_t nvox, double* counts, void* stream);
int vsseg_argmax2(const float* logits, int32_t pitch, int64_t nvox, uint8_t* dst, void* stream);

/* Surface distances of the argmax prediction P (ties -> class 0, as vsseg_argmax2) against the label G = ((int)label == 1), as vsseg_hard_dice_counts reads them
   (ABI version 8): edges E(M) = M AND NOT erode(M) with the 6-connected cross, voxels outside the volume background; d(P->G) = for every voxel of E(P) the Euclidean
   distance in mm (voxel extents `spacing`) to the nearest voxel of E(G), d(G->P) the same the other way round.  out[0] = hd = max of the two directions' `percentile`
   (numpy.percentile, linear interpolation; 100 = the maximum), out[1] = assd = (sum d(P->G) + sum d(G->P)) / (|E(P)| + |E(G)|); both masks empty: NaN, one empty: +inf.
   One volume [X][Y][Z] per call: logits [X][Y][Z][2] fp32 (pitch 2, 8-byte aligned), label [X][Y][Z] fp32, out 2 fp32 in device memory.  A sequence of launches on
   `stream` without host synchronisation: the counts stay on the device.  Bit-identical from call to call.  scratch: device memory of vsseg_surface_scratch_bytes(dims)
   bytes, 256-byte aligned, overwritten (a call on another stream needs its own).  dims: 1 .. 8192 on every axis. */
int64_t vsseg_surface_scratch_bytes(const int32_t dims[3]); /* bytes of scratch, or VSSEG_EINVAL */
int vsseg_surface_distances(const float* logits, int32_t pitch, const float* label, const int32_t dims[3], const float spacing[3] /* mm per voxel along x, y, z */,
                            double percentile /* 0 .. 100 */, void* scratch, int64_t scratch_bytes, float* out, void* stream);
/* vsseg_surface_distances plus the normalised surface Dice (NSD) at tolerances in mm, from the same edge pass and the same distance transform (ABI version 19; the
   metric of the Medical Segmentation Decathlon and Metrics Reloaded, MONAI's compute_surface_dice without sub-voxels).  Masks, edges, d(P->G), d(G->P), operands, scratch,
   stream and determinism as above: one volume per call, launches on `stream` only, no host read, no allocation, bit-identical from call to call; the same number of
   launches and no pass over the volume or the bounding box beyond those of vsseg_surface_distances (the counting rides on the first histogram pass).
   tolerances_mm: ntol (0 .. 8) finite values >= 0 in HOST memory, read before the call returns; may be NULL when ntol = 0.  out: 3 + 3 * ntol fp32 in device memory:
     out[0] = hd, out[1] = assd: the same bits vsseg_surface_distances writes for the same arguments;
     out[2] = masd = (mean d(P->G) + mean d(G->P)) / 2, formed in fp64 from the two per-direction sums;
     for tolerance t: out[3+3t] = nsd = (nP + nG) / (|E(P)| + |E(G)|), out[4+3t] = nP / |E(P)| (surface precision), out[5+3t] = nG / |E(G)| (surface recall), where nP
     counts the voxels of E(P) within tau_t of E(G) and nG those of E(G) within tau_t of E(P): exact integer counts (integer atomics), each quotient formed once in fp64
     and rounded once to fp32.
   "Within tau" is decided on the squared distance field, never on a square root: a voxel counts when f <= t2, f the fp32 value the distance transform left for that voxel
   and direction and t2 = (float)((double)tau * (double)tau); a tie counts, f = +inf never does.  Where the field is exact (unit spacing: integers below 2^24; spacings
   such as 0.5 / 1.5: dyadic rationals) so is the result.
   Empty masks (MONAI): both edge sets empty: every output NaN; exactly one empty: hd, assd, masd = +inf, every nsd = 0, the fraction over the empty set NaN, the other 0.
   Checked before anything is launched: everything vsseg_surface_distances checks, ntol in 0 .. 8, tolerances_mm non-null when ntol > 0, every tolerance finite and >= 0. */
int vsseg_surface_metrics(const float* logits, int32_t pitch, const float* label, const int32_t dims[3], const float spacing[3] /* mm per voxel along x, y, z */,
                          double percentile /* 0 .. 100 */, const float* tolerances_mm /* host, ntol values */, int32_t ntol /* 0 .. 8 */, void* scratch, int64_t scratch_bytes,
                          float* out /* 3 + 3 * ntol fp32, device */, void* stream);

/* Connected components of the foreground of a two-class prediction and the prediction filtered to the largest of them (ABI version 9; the post-transform that MONAI
   spells AsDiscrete + KeepLargestConnectedComponent; beyond the reference, which reports and exports the raw argmax).  One volume [X][Y][Z] per call: logits
   [X][Y][Z][2] fp32 (pitch 2, 8-byte aligned), never written.
   Foreground P = logits[v][1] > logits[v][0], the rule of vsseg_argmax2 (ties and NaN are background).  connectivity 6, 18 or 26: two foreground voxels are neighbours
   when their index offset d has every |d_a| <= 1 and |dx| + |dy| + |dz| <= 1, 2 or 3; voxels outside the volume are background.
   labels: int32 [X][Y][Z], 0 on the background and 1 + the smallest linear index (x * Y + y) * Z + z of its component on a foreground voxel: a function of the mask alone.
   Largest component: most voxels, ties to the smallest label (the component met first in raster order, as numpy.bincount(...).argmax() picks it); P empty: none.
   out: fp32 [X][Y][Z][2] (8-byte aligned), channel 1 = 1.0 on the largest component and 0.0 elsewhere, channel 0 = 1 - channel 1: a one-hot "probability" tensor that
   vsseg_hard_dice_counts, vsseg_argmax2 and vsseg_surface_distances read like any other prediction.
   stats: four int64 in device memory (8-byte aligned): [0] |P|, [1] number of components, [2] voxels of the largest, [3] its label (0 when P is empty); may be NULL
   for vsseg_keep_largest_component.
   A sequence of launches on `stream` without host synchronisation; only integer atomics decide anything, so a call is bit-identical from run to run.  No kernel waits
   for another workgroup.  scratch: device memory of vsseg_components_scratch_bytes(dims) bytes (8 B per voxel), 256-byte aligned, overwritten (a call on another stream
   needs its own).  dims: 1 .. 8192 on every axis and X * Y * Z < 2^31 - 1. */
int64_t vsseg_components_scratch_bytes(const int32_t dims[3]); /* bytes of scratch, or VSSEG_EINVAL */
int vsseg_components_label(const float* logits, int32_t pitch, const int32_t dims[3], int32_t connectivity, void* scratch, int64_t scratch_bytes, int32_t* labels, int64_t* stats,
                           void* stream);
int vsseg_keep_largest_component(const float* logits, int32_t pitch, const int32_t dims[3], int32_t connectivity, void* scratch, int64_t scratch_bytes, float* out,
                                 int64_t* stats /* may be NULL */, void* stream);

/* Two more post-transforms on the same foreground, connectivities, domain, scratch (vsseg_components_scratch_bytes) and output format as vsseg_keep_largest_component
   (ABI version 18; MONAI's FillHoles and RemoveSmallObjects).  out: fp32 [X][Y][Z][2] (8-byte aligned), channel 1 = 1.0 on the result and 0.0 elsewhere, channel 0 =
   1 - channel 1; logits are never written; stats: four int64 in device memory (8-byte aligned), may be NULL.
   vsseg_fill_holes: the result is P united with H, the union of the connected components of the COMPLEMENT of P (at `connectivity`, that of the background; 6 is
   scipy.ndimage.binary_fill_holes' default and the dual of a 26-connected foreground, 26 is what MONAI's FillHoles uses) that contain no voxel on the border of the volume
   (a voxel with an index equal to 0 or to dim - 1).  A volume with an extent of 1 or 2 along an axis has no holes; a tunnel through a ring is not a hole; an empty P
   gives an empty result.  stats: [0] |P|, [1] number of holes, [2] |H|, [3] |P| + |H|.  Launches: init, one pass that reads the logits and leaves |P| and the bounding
   box of P (8 B per voxel), the tile labelling / merge / flatten of the components above on the complement of P inside that box only, a count, and one pass that writes
   the result (8 B per voxel).  A background component of the box without a voxel on a face of the box is a hole, every other one is not (components.hip states why).
   vsseg_remove_small_components: the result is the union of the components of P (at `connectivity`) with at least min_voxels voxels (strictly smaller ones are
   removed: skimage.morphology.remove_small_objects' rule); min_voxels <= 1 keeps P; min_voxels is a host argument, nothing is read back.  stats: [0] |P|, [1] number
   of components of P, [2] kept voxels, [3] kept components.  The launches of vsseg_keep_largest_component with its selection replaced by a count.
   Both: a sequence of launches on `stream` without host synchronisation or allocation, bit-identical from run to run (only integer atomics decide anything), no kernel
   waits for another workgroup.  Argument checks, before anything is launched: logits / scratch / out not null, alignment (logits, out, stats 8 B, scratch 256 B),
   pitch == 2, dims in the domain, connectivity 6 / 18 / 26, min_voxels >= 0, scratch_bytes large enough. */
int vsseg_fill_holes(const float* logits, int32_t pitch, const int32_t dims[3], int32_t connectivity, void* scratch, int64_t scratch_bytes, float* out,
                     int64_t* stats /* may be NULL */, void* stream);
int vsseg_remove_small_components(const float* logits, int32_t pitch, const int32_t dims[3], int32_t connectivity, int64_t min_voxels, void* scratch, int64_t scratch_bytes,
                                  float* out, int64_t* stats /* may be NULL */, void* stream);

/* Ball morphology of the same foreground at a radius in mm (ABI version 22; scipy.ndimage.binary_dilation / binary_erosion / binary_closing / binary_opening with a ball
   that follows the voxel spacing).  One volume [X][Y][Z] per call: logits [X][Y][Z][2] fp32 (pitch 2, 8-byte aligned), never written; foreground P = logits[v][1] >
   logits[v][0] (ties and NaN are background); spacing = mm per voxel along x, y, z (fp32); radius_mm = r >= 0.
   The ball: an integer offset d has the squared length f(d) = fmaf(ax, ax, fmaf(ay, ay, az * az)) in fp32 with a_a = spacing[a] * (float)d_a (the accumulation order of the
   distance transform of vsseg_surface_distances), and belongs to the ball when f(d) <= t2 = (float)((double)r * (double)r); a tie belongs, as in vsseg_surface_metrics.
   Where the products are exact (unit spacing, dyadic spacings such as 0.5 / 1.5) so is the ball; elsewhere an offset whose fp64 squared length lies within a few 2^-24
   (relative) of r^2 may fall on either side.  At r = 0 the ball is the single offset 0 and every operation returns the one-hot of P.
   op 0, dilate(M): every voxel of the volume with a voxel of M at a ball offset; outside the volume there is no foreground (binary_dilation, border_value = 0).
   op 1, erode(M): every voxel of M with no BACKGROUND VOXEL OF THE VOLUME at a ball offset; positions outside the volume are ignored, they are not background
   (binary_erosion, border_value = 1), so a mask cut by the field of view does not shrink at the border, closing is extensive and opening anti-extensive there too.
   op 2, close(M) = erode(dilate(M)); op 3, open(M) = dilate(erode(M)), both with the same ball.  An empty P gives an empty result, an all-foreground volume is unchanged.
   out: fp32 [X][Y][Z][2] (8-byte aligned), channel 1 = 1.0 on the result and 0.0 elsewhere, channel 0 = 1 - channel 1: the one-hot format of vsseg_keep_largest_component.
   stats: four int64 in device memory (8-byte aligned), may be NULL: [0] |P|, [1] |result|, [2] |result \ P| (added), [3] |P \ result| (removed): exact integer counts.
   Launches: init; one pass that reads the logits and leaves |P| and the bounding box of P (8 B per voxel); per stage (one for dilate / erode, two for close / open) two
   kernels confined to the work box W = that box grown by reach + 1 voxels per axis, reach_a = floor(r / spacing[a]): a banded exact separable squared-distance pass
   along z and y, and one along x fused with the compare against t2 (ball.hip states why the band of reach + 1 is exact and why W suffices); one pass that writes the
   result (8 B per voxel) and counts.  No host synchronisation, no allocation, no kernel waits for another workgroup, the grids depend on dims alone, and only integer
   atomics combine workgroups: a call is bit-identical from run to run.  scratch: device memory of vsseg_ball_scratch_bytes(dims) bytes (a record and 6 B per voxel),
   256-byte aligned, overwritten (a call on another stream needs its own).
   Domain: dims 1 .. 8192 on every axis and X * Y * Z < 2^31 - 1; spacing positive and finite; r finite and >= 0; reach_a <= 32 voxels on every axis (13 mm at 0.41 mm).
   Argument checks, before anything is launched: logits / spacing / scratch / out not null, alignment, pitch == 2, dims, spacing, scratch_bytes, op in 0 .. 3, radius,
   reach; the message names the offending value. */
int64_t vsseg_ball_scratch_bytes(const int32_t dims[3]); /* bytes of scratch, or VSSEG_EINVAL */
int vsseg_ball_morphology(const float* logits, int32_t pitch, const int32_t dims[3], const float spacing[3], int32_t op /* 0 dilate, 1 erode, 2 close, 3 open */, double radius_mm,
                          void* scratch, int64_t scratch_bytes, float* out, int64_t* stats /* may be NULL */, void* stream);

/* Size and position of the argmax prediction P = (logits[v][1] > logits[v][0]) (the rule of vsseg_argmax2: ties and NaN are background) and of the label
   G = ((int)label[v] == 1) (the rule of vsseg_hard_dice_counts) (ABI version 17; beyond the reference, which reports the hard Dice only).  One volume [X][Y][Z] per call:
   logits [X][Y][Z][2] fp32 (pitch 2, 8-byte aligned), label [X][Y][Z] fp32 or NULL, spacing = mm per voxel along x, y, z.  out: nine fp64 in device memory (8-byte aligned):
     [0], [1]  voxels_pred, voxels_label              |P|, |G|: exact integers
     [2], [3]  volume_pred_mm3, volume_label_mm3      count * (sx * sy * sz), the product formed in fp64 from the fp32 spacing
     [4]       centroid_distance_mm                   Euclidean distance between the two centres of mass (fp64, from exact integer sums of the voxel indices); NaN when
                                                      either mask is empty
     [5], [6]  max_diameter_pred_mm, _label_mm        the largest distance between the centres of two voxels of the mask (the 3-D Feret diameter; pyradiomics'
                                                      Maximum3DDiameter taken between voxel centres); a single voxel: 0, an empty mask: NaN
     [7], [8]  max_axial_diameter_pred_mm, _label_mm  the same over pairs of voxels with equal z: the largest in-plane diameter over the axial slices; a single voxel: 0,
                                                      an empty mask: NaN
   label == NULL: every label field and [4] are NaN.  The squared distance of a pair, (sx dx)^2 + (sy dy)^2 + (sz dz)^2, is formed in fp32 from exact integer differences
   (FMA contraction allowed: a relative error of a few 2^-24; exact at unit spacing and extents below 2048); the maximum is taken over the fp32 values and its square root
   once, in fp64.  The farthest pair is searched among the two x extremes of every (y, z) column of the mask (with dy and dz fixed a pair whose x extent can grow is not
   the farthest), restricted to the mask's (y, z) bounding box; that search is quadratic in the occupied columns, hence the
   domain: dims 1 .. 8192 on every axis and Y * Z <= 2^18 (512 x 512 in-plane in any orientation); anything else returns VSSEG_EINVAL with a message that names dims.
   A sequence of launches on `stream` (init, one streaming pass of 12 B per voxel - 8 B without a label -, the pair stage, finalize) without host synchronisation or
   allocation; no kernel waits for another workgroup and the grids depend on dims alone.  Only integer atomics (64-bit sums, min / max of indices and of the bit patterns
   of non-negative floats) combine workgroups, so a call is bit-identical from run to run.  scratch: device memory of vsseg_measure_scratch_bytes(dims) bytes (a record
   and 16 B per (y, z) column), 256-byte aligned, overwritten (a call on another stream needs its own).
   Argument checks, before anything is launched: logits / spacing / scratch / out not null, alignment, pitch == 2, dims in the domain, spacing positive and finite,
   scratch_bytes large enough. */
int64_t vsseg_measure_scratch_bytes(const int32_t dims[3]); /* bytes of scratch, or VSSEG_EINVAL */
int vsseg_measurements(const float* logits, int32_t pitch, const float* label /* may be NULL */, const int32_t dims[3], const float spacing[3], void* scratch,
                       int64_t scratch_bytes, double* out /* 9 fp64, device */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
