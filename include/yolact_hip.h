/* yolact_hip.h — C-ABI of libyolact_hip.so, the MI355X (gfx950) hot path of YOLACT.
 *
 * The reference (feiyuhuahuo/Yolact_minimal) has NO native interface for this path: every tensor
 * op goes through torch.nn / ATen, and its only native file is the Cython greedy NMS
 * (cython_nms.pyx:24-74).  So the entry points below are what a maintainer would bind *instead of*
 * the ATen calls at the cited reference lines.  Conventions:
 *   - extern "C", raw DEVICE pointers + explicit sizes + a hipStream_t (passed as void*);
 *   - fp32 everywhere, activations NHWC ([B][H][W][C], C contiguous), weights [Cout][KH][KW][Cin];
 *   - every call is asynchronous on `stream`; nothing allocates, frees or synchronises;
 *   - scratch memory is supplied by the caller (ask ym_*_workspace_bytes first);
 *   - return 0 on success, a negative YM_E* code otherwise; ym_last_error() gives the text.
 * No torch types appear here.  The Python host (yolact_minimal_amd/hip.py) binds these with ctypes.
 */
#ifndef YOLACT_HIP_H
#define YOLACT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YM_OK 0
#define YM_EINVAL (-1)   /* bad argument (shape, alignment, null pointer) */
#define YM_ENOSPC (-2)   /* workspace too small */
#define YM_ELAUNCH (-3)  /* hipGetLastError() after a launch was not hipSuccess */

#define YM_ACT_NONE 0
#define YM_ACT_RELU 1
#define YM_ACT_TANH 2
#define YM_ACT_GELU 3   /* exact erf GELU (Swin Mlp, modules/swin_transformer.py:88) — forward only */

typedef void* ym_stream_t; /* hipStream_t */

int ym_abi_version(void);
const char* ym_last_error(void);

/* ---- layout / parameter preparation ----------------------------------------------------------- */

/* NCHW fp32 image -> NHWC with C padded to 4 (pad lanes = 0).  Replaces the implicit layout of
 * `self.backbone(img)` input, reference modules/yolact.py:142. in:[B][C][H][W] (C<=4) out:[B][H][W][4] */
int ym_nchw_to_nhwc4(const float* in, float* out, int B, int C, int H, int W, ym_stream_t s);

/* OIHW fp32 weight (torch state-dict layout) -> [Cout][KH][KW][cin_pad] with zero padding of the
 * channel dim, rows zero-extended to k_pad floats (k_pad >= KH*KW*cin_pad, multiple of 32). */
int ym_pack_conv_weight(const float* w_oihw, float* w_packed, int Cout, int Cin, int KH, int KW,
                        int cin_pad, int k_pad, ym_stream_t s);

/* Eval-mode BatchNorm folded to y = x*scale + shift (reference modules/resnet.py:24,28,32 in eval):
 * scale = gamma / sqrt(var + eps), shift = beta - mean*scale. */
int ym_fold_bn(const float* gamma, const float* beta, const float* mean, const float* var, float eps,
               float* scale, float* shift, int C, ym_stream_t s);

/* ---- fused convolution (implicit GEMM on the f32 MFMA pipe) ------------------------------------- */

typedef struct {
    int n_begin, n_end;      /* output-channel range [n_begin, n_end) routed to this segment      */
    float* out;              /* element (b, pixel, n) lives at out[b*batch_stride + pixel*pitch + (n-n_begin)] */
    int64_t batch_stride;    /* floats */
    int32_t pitch;           /* floats between consecutive output pixels */
    int32_t act;             /* YM_ACT_* applied to this segment */
} ym_conv_seg;

typedef struct {
    const float* in;         /* NHWC [B][H][W][Cin]; for Cin==4 ("stem" mode) the packed weight uses cin_pad=4 */
    const float* weight;     /* packed by ym_pack_conv_weight: [Cout][k_pad] */
    const float* scale;      /* [Cout] or NULL (=1) : folded BN scale */
    const float* shift;      /* [Cout] or NULL (=0) : folded BN shift or conv bias */
    const float* residual;   /* NULL or NHWC [B][Ho][Wo][Cout] added before the activation */
    int32_t B, H, W, Cin, Cout, KH, KW, stride, pad, Ho, Wo, k_pad;
    int32_t nseg;            /* 1..3 */
    ym_conv_seg seg[3];
    /* tuning knobs (0 = library heuristic); yolact_minimal_amd/tuned_gfx950.json holds measured choices */
    int32_t tile_m, tile_n;  /* workgroup kernel: 128/64 (workgroup tile); wave kernel: 64/32 (per-wave tile) */
    int32_t ksplit;          /* workgroup kernel: K slices across the grid (slices > 1 need workspace) */
    int32_t kwaves;          /* 0 = LDS-tiled workgroup kernel; 1/2/4/8 = wave-private kernel with that many
                                waves of one workgroup splitting K for each output tile (tile_m x tile_n = the WAVE's tile, 32 / 64).
                                With stages = 22 / 23 / 24: the DMA-ring variant (kwaves 1 / 2 / 4, tile 32x32, 64x32 or 32x64, Cin % 32
                                == 0): every wave streams its operands through a private LDS ring of 2 / 3 / 4 K tiles filled by
                                global->LDS DMA; with tile 32x32, kwaves 4 it also takes tail_tiles / tail_ksplit (<= 8 slices) */
    int32_t transposed;      /* 0 = convolution.  1 = DATA GRADIENT of that convolution (conv-transpose gather):
                                `in` is dy NHWC [B][H][W][Cin] (H,W = the forward OUTPUT size, Cin = forward Cout
                                padded to a multiple of 32), the result is dx [B][Ho][Wo][Cout] (Ho,Wo = forward
                                INPUT size, Cout = forward Cin), stride/pad/KH/KW are the forward conv's, and
                                `weight` comes from ym_pack_conv_weight_dgrad.  Autograd counterpart of every
                                nn.Conv2d on the path (loss_total.backward(), reference train.py:126). */
    int32_t stages;          /* workgroup kernel operand staging: 0/2 = registers, double buffer; 3 = registers, loads two K tiles
                                ahead (forward: not the 128x128 tile; data gradient: 64x64 only); 22/23 = direct global->LDS DMA, ring
                                of 2/3; 24 = ring of 4, 33/34 = ring of 3/4 with software-pipelined fragments (64x64 forward tile only);
                                42/43/44/46/48 = PERSISTENT direct-to-LDS kernel, ring of 2/3/4/6/8 (64x64 tile, plain NHWC
                                output, ReLU or no activation, no bn_sum; anything else falls back to 22/23/24): grid_wgs workgroups walk
                                the (tile, K slice) items and the operand stream runs on across item boundaries;
                                52/53/54 = WEIGHT-STATIONARY 1x1 / stride-1 kernel, ring of 2/3/4 (tile 64x256, 128x128 or 256x64, plain
                                NHWC output, ReLU or no activation, no bnb_y, filter slice <= 64 KB and slice + ring <= 160 KB of LDS;
                                anything else runs as the 64x64 tile with 22).  Any other value, and a value that does not exist for
                                the tile, runs the register double buffer; ym_conv2d_effective_plan reports what a descriptor resolves to */
    double* bn_sum;          /* optional [Cout] fp64 accumulators (zeroed by the caller): the epilogue adds the */
    double* bn_sumsq;        /* per-channel sum / sum of squares of the conv OUTPUT (train-mode BN statistics).  */
                             /* Only when ym_conv2d_fuses_bn_stats(desc) == 1 (plain NHWC output).               */
    int32_t* tile_counters;  /* optional, >= ym_conv2d_tile_counters(desc) int32, ZERO before the first launch (the  */
                             /* kernel leaves them zero): with a K split and a plain NHWC output, the LAST workgroup  */
                             /* to finish an output tile sums the slices (in slice order: deterministic) and runs the  */
                             /* epilogue in the same launch; NULL = separate reduce launch.  One buffer may be shared  */
                             /* by launches that are ordered on one stream, never by concurrent ones.                  */
    int32_t nlevels;         /* 0 = one image size.  1..5 = "pyramid" input: `in` holds nlevels feature maps of DIFFERENT sizes back   */
    int32_t level_h[5];      /* to back, level-major ([level][B][h][w][Cin]); the same filter runs over all of them in ONE launch   */
    int32_t level_w[5];      /* (the shared PredictionModule of modules/yolact.py:149-157 is one conv per level in the reference). */
                             /* Stride 1, pad = K/2 only; H/W/Ho/Wo of the descriptor are ignored, M = sum_l B*h_l*w_l.  A plain   */
                             /* output (one segment, batch_stride 0) keeps the input's row order; a segmented output places level l's pixel p of image b at        */
                             /* out[b*batch_stride + (sum_{j<l} h_j*w_j + p)*pitch] = the reference's cat over levels (:155-157).     */
    int32_t tail_tiles;      /* workgroup-quantisation fix (needs tile_counters, ksplit <= 1, plain NHWC output): the   */
    int32_t tail_ksplit;     /* LAST tail_tiles output tiles are each split into tail_ksplit K slices, so that e.g. 580  */
                             /* tiles on 256 CUs become 512 whole tiles + 68x4 quarter tiles instead of 2-or-3 per CU.   */
    int32_t mma;             /* matrix pipe of the workgroup kernel.  0 = f32 MFMA (v_mfma_f32_32x32x2_f32: exact fp32 products, the    */
                             /* parity mode).  3 / 6 = "split bf16": every fp32 operand is split on its way into LDS into two / three  */
                             /* bf16 terms and the 3 / 6 most significant cross products run on v_mfma_f32_32x32x16_bf16 with fp32     */
                             /* accumulation (relative error per product typically ~2^-17 / ~2^-23, at most 3 * 2^-16 / 5 * 2^-24: the */
                             /* dropped cross terms and the residual after two / three bf16 roundings of 2^-8 each; tensors in HBM     */
                             /* stay fp32).  Needs Cin % 32 == 0, kwaves == 0, no pyramid input; register staging only: stages 3 = two */
                             /* register sets (every tile), any other value the double buffer.                                         */
    int32_t bnb_relu;        /* Train-mode BatchNorm BACKWARD statistics, fused.  A data-gradient launch (transposed = 1) writes the   */
    const float* bnb_y;      /* gradient dout[M][Cout] of the PREVIOUS layer's BN output; with bnb_y != NULL its epilogue also adds    */
    const float* bnb_out;    /* that BN's two backward sums to bn_sum / bn_sumsq (zeroed by the caller): bn_sum[c] += sum_m dz,        */
    const float* bnb_mean;   /* bn_sumsq[c] += sum_m dz * xhat, where xhat = (y - mean) * invstd, y = bnb_y = that layer's raw conv    */
    const float* bnb_invstd; /* output [M][Cout], and dz = dout masked by the layer's ReLU when bnb_relu: out > 0 with                 */
    const float* bnb_gamma;  /* bnb_out = its saved output, or (bnb_out == NULL) xhat * gamma + beta > 0 re-derived exactly as the     */
    const float* bnb_beta;   /* forward pass computed it.  Same sums as the first pass of ym_bn_train_bwd, which                       */
                             /* ym_bn_train_bwd_apply then skips.  Needs ym_conv2d_fuses_bn_stats(desc) == 1.                          */
    int32_t grid_wgs;        /* persistent kernel (stages 4x): workgroups to launch; 0 = as many as the CUs hold (LDS-limited, at most  */
                             /* 4 per CU), never more than there are work items.  Wave kernel with DMA rings (kwaves > 0, stages 22-24):  */
                             /* waves per workgroup, 0 = 4 (1 / 2 with kwaves <= that: single tiles are balanced over the CUs)            */
    int32_t bn_ordered;      /* (in what was the struct's trailing padding: its size is unchanged.)  != 0 with bn_sum: ORDERED statistics.  */
                             /* bn_sum is then the base of a partial buffer double[ym_conv2d_bn_partial_rows(desc)][2][Cout] (8-byte        */
                             /* aligned, no zero fill needed) and bn_sumsq is unused: instead of atomics, exactly one workgroup stores its   */
                             /* column sums to part[row][0][c] (bn_sum term) and part[row][1][c] (bn_sumsq term) for every row and every     */
                             /* c < Cout; ym_bn_partials_finish then adds the rows in a fixed order.  Forward statistics and bnb_* sums.     */
} ym_conv_desc;

/* y = act(conv(x, w) * scale + shift + residual), one launch (plus a reduce launch if K is split).
 * Replaces: conv+BN+ReLU(+add) of Bottleneck.forward (modules/resnet.py:20-40), the stem
 * (modules/resnet.py:88-90), conv+bias+ReLU of FPN / ProtoNet (modules/yolact.py:62-68,37-47) and,
 * with three segments, the bbox/conf/coef convs + tanh + permute/reshape/cat of
 * PredictionModule.forward + Yolact.forward (modules/yolact.py:27-30,155-157). */
size_t ym_sizeof_conv_desc(void);                      /* for bindings: must equal their mirror of ym_conv_desc */
size_t ym_conv2d_workspace_bytes(const ym_conv_desc* d);
int ym_conv2d_tile_counters(const ym_conv_desc* d);   /* output tiles of the chosen plan (0 if K is not split) */
int ym_conv2d_fuses_bn_stats(const ym_conv_desc* d);
/* The plan ym_conv2d_fwd would run for this descriptor (16-byte aligned workspace assumed), in the row encoding of the tuned table:
 * out = [tile_m, tile_n, ksplit, kwaves, stages, tail_tiles, tail_ksplit, grid_wgs].  Host only: needs no device, and looks at the
 * descriptor's pointers for nullness and alignment only.  `stages` is canonical: 2 = register double buffer (whatever value asked
 * for it; pyramid and stem always), 3 = register ring where it is built, 22/23/24 = direct-to-LDS ring of 2/3/4 (with kwaves > 0:
 * the wave kernel's DMA rings), 33/34 = DMA ring with pipelined fragments, 40 + depth = the persistent ring actually launched,
 * 50 + depth = weight-stationary ring, 0 = wave kernel without DMA.  tail_tiles / tail_ksplit are the plan's after clamping (0 / 0:
 * the tail was dropped); grid_wgs is the descriptor's where the chosen kernel reads it, else 0.  Returns YM_OK, or the error of an
 * invalid descriptor. */
int ym_conv2d_effective_plan(const ym_conv_desc* d, int32_t out[8]);
int ym_conv2d_bn_partial_rows(const ym_conv_desc* d); /* rows of the bn_ordered partial buffer the chosen plan writes (M tiles, or   */
                                                      /* walkers x wave rows of the weight-stationary kernel); 0 if the statistics do  */
                                                      /* not fuse (ym_conv2d_fuses_bn_stats(desc) == 0)                                */
/* Ordered sum of per-row partials part[rows][2][C] (fp64) into sums = sum[C] | sumsq[C] (fp64, overwritten), the layout
 * ym_bn_train_fwd_stats / ym_bn_train_bwd_apply read.  The order is fixed: for each of the two terms and each channel, slice s
 * (s = 0..15) adds the rows k = s, s + 16, s + 32, ... in ascending k starting from 0.0; then the 16 slice sums are added in
 * ascending s starting from 0.0.  The result depends on the partials alone, not on how the launch was scheduled. */
int ym_bn_partials_finish(const void* part, int rows, int C, void* sums, ym_stream_t s);
/* Launches, since the library was loaded, whose sums on a statistic or gradient path end in floating-point atomics (their result
 * depends on the order in which workgroups retire): ym_conv2d_fwd with bn_sum and bn_ordered == 0, ym_bn_train_fwd / ym_bn_train_bwd /
 * ym_act_bias_bwd (dbias) with the small workspace, ym_swin_window_attention_bwd.  Host-side, monotonic; a step that leaves it where
 * it was is bit-reproducible.  (The reported loss scalars are summed with atomics too; nothing reads them back, they do not count.) */
int64_t ym_unordered_sum_launches(void);
int ym_conv2d_fwd(const ym_conv_desc* d, void* workspace, size_t workspace_bytes, ym_stream_t s);

/* ---- Swin-T backward + AdamW (row a18 under loss.backward(); reference train.py:62-63,126) ---------------------------
 * LayerNorm backward over the last dim of x [M][C] (statistics recomputed): dx, dgamma, dbeta (overwritten). */
size_t ym_layernorm_bwd_workspace_bytes(int C);
int ym_layernorm_bwd(const float* dy, const float* x, const float* gamma, float eps, int64_t M, int C, float* dx, float* dgamma,
                     float* dbeta, void* workspace, size_t workspace_bytes, ym_stream_t s);
/* Backward of ym_patch_merge_layernorm: dy [B*ceil(H/2)*ceil(W/2)][4C], x NHWC [B][H][W][C] -> dx (same shape as x; every
 * element written), dgamma / dbeta [4C].  workspace >= ym_layernorm_bwd_workspace_bytes(4*C). */
int ym_patch_merge_layernorm_bwd(const float* dy, const float* x, int B, int H, int W, int C, const float* gamma, float eps,
                                 float* dx, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, ym_stream_t s);
/* DropPath + residual add in one pass (modules/swin_transformer.py:71-82 with the call sites :285,288): out = res + (y / keep) *
 * floor(keep + rnd[b]) in the reference's operation order; rnd [B] is the raw torch.rand draw, res / y / out are [B][per_sample]
 * (per_sample % 4 == 0).  Backward: the residual's gradient is dout, dy = (dout * mask) / keep. */
int ym_drop_path_add(const float* res, const float* y, const float* rnd, float keep, float* out, int B, int64_t per_sample,
                     ym_stream_t s);
int ym_drop_path_bwd(const float* dout, const float* rnd, float keep, float* dy, int B, int64_t per_sample, ym_stream_t s);
/* Exact (erf) GELU of Mlp.forward (modules/swin_transformer.py:92-96) on a saved pre-activation; n % 4 == 0. */
int ym_gelu_fwd(const float* z, float* out, int64_t n, ym_stream_t s);
int ym_gelu_bwd(const float* dy, const float* z, float* dz, int64_t n, ym_stream_t s);
/* Backward of ym_swin_window_attention: dout [B*H*W][C] -> dqkv [B*H*W][3C] (every element written), and ACCUMULATED into
 * caller-zeroed buffers: dqkv_bias_pad [3C] (gradient reaching the qkv bias through the padded tokens, to be added to the
 * qkv Linear's bias gradient) and dtable [(2*window-1)^2][heads] (relative-position-bias table). */
int ym_swin_window_attention_bwd(const float* qkv, const float* qkv_bias, const float* rel_bias_table, const float* dout, int B,
                                 int H, int W, int C, int heads, int window, int shift, float* dqkv, float* dqkv_bias_pad,
                                 float* dtable, ym_stream_t s);
/* torch.optim.AdamW (amsgrad=False) on flat fp32 buffers, step >= 1 (reference train.py:63: lr, weight_decay=0.05). */
int ym_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int step, ym_stream_t s);

/* ---- train_aug pixel work (next row f4; reference utils/augmentations.py:60-77,138-216,230-252) ---------------------------
 * The random decisions of one sample (drawn on the host in the reference's `random` call order):
 *   source H x W -> mirror -> crop (cx, cy, cw, ch) -> pad to the q x q square at (px, py), border = norm_mean -> bilinear resize
 *   to r x r -> final_mode 0: r == S | 1: paste at (fx, fy) into S x S (border = norm_mean) | 2: crop S x S at (fx, fy).
 * photometric: optional brightness add / contrast scale (each clipped to 0..255), then BGR->HSV, S *= saturation, H += hue
 * (wrapped to 0..360), HSV->BGR, clip.  mean / std in BGR order (config.py:66-67). */
typedef struct {
    int32_t H, W, mirror, cx, cy, cw, ch, q, px, py, r, S, final_mode, fx, fy, has_brightness, has_contrast;
    float brightness, contrast, saturation, hue, mean[3], std[3];
} ym_aug_plan;
/* img HWC BGR (uint8 if is_u8 else float32) -> out [3][S][S] normalised RGB planes, one launch. */
int ym_train_aug_image(const void* img_hwc_bgr, int is_u8, const ym_aug_plan* plan, float* out_chw, ym_stream_t s);
/* masks [n][H][W] (uint8 / float32), keep [k] indices of the surviving instances -> out [k][S][S] (bilinear, border 0).  uint8 masks
 * of an already-square crop (plan->cw == plan->ch) take OpenCV's 8-bit fixed-point resize, as in the reference (its masks stay uint8
 * there: utils/augmentations.py:138-141,180-181): a {0,1} mask comes out {0,1}. */
int ym_train_aug_masks(const void* masks, int is_u8, const int32_t* keep, int k, const ym_aug_plan* plan, float* out,
                       ym_stream_t s);
/* The two entries above for a whole training batch: the samples are images of DIFFERENT sizes, the output one [B][3][S][S] tensor.
 *   `items` is a HOST table of B <= YM_AUG_MAX_SAMPLES samples.  It is read during the call and travels to the kernels by value in
 * their arguments, 16 samples per launch (B = 17 .. 32: two launches per entry): no copy to the device, no synchronisation, nothing
 * to keep alive afterwards.  Sample b: its plan (plan.S == S), its image `img` (HWC BGR [plan.H][plan.W][3] on the device; the
 * images need not share an allocation), its instance masks `masks` ([n_masks][plan.H][plan.W]; may be NULL when k == 0) and its
 * k surviving instances, which are rows [row0, row0 + k) of `keep_dev` (device int32, indices into ITS masks) and of the mask
 * output; row0 is the sum of the earlier samples' k, total_k the sum of all.  is_u8 is the dtype of every image (image entry) /
 * every mask (mask entry); the 8-bit resize of an already-square crop is chosen per sample (is_u8 && plan.cw == plan.ch).
 *   ym_train_aug_image_batch: grid = ceil(S * S / 256) x samples, out [B][3][S][S].  ym_train_aug_masks_batch: grid =
 * ceil(S * S / 256) x mask rows, out [total_k][S][S]; total_k == 0 is a no-op; a keep index outside 0 .. n_masks - 1 reads nothing
 * and gives a zero row.  ym_train_aug_image / ym_train_aug_masks are the one-sample instances of the same two kernels (keep as
 * keep_dev, row0 = 0), so a row of a batch equals the single call bit for bit.  YM_EINVAL before any launch: B outside
 * 1 .. YM_AUG_MAX_SAMPLES, a null table / image / output pointer, plan.S != S, an invalid plan, k < 0, k > 0 with null masks or
 * n_masks <= 0, row0 or total_k off the running sum, total_k > 0 with a null keep_dev or output. */
#define YM_AUG_MAX_SAMPLES 32            /* = YM_RAGGED_MAX_IMAGES: the images arrive as one frame batch */
typedef struct ym_aug_item {
    ym_aug_plan plan;
    int32_t n_masks;
    const void* img;
    const void* masks;
    int32_t k, row0;
} ym_aug_item;
size_t ym_sizeof_aug_item(void);                       /* for bindings: must equal their mirror of ym_aug_item */
int ym_train_aug_image_batch(const ym_aug_item* items, int B, int S, int is_u8, float* out, ym_stream_t s);
int ym_train_aug_masks_batch(const ym_aug_item* items, int B, int S, int is_u8, const int32_t* keep_dev, int total_k, float* out,
                             ym_stream_t s);
/* Window training (utils/rect.py): only the top-left Hn x Wn WINDOW of every S x S sample, out [B][3][Hn][Wn] / [total_k][Hn][Wn],
 * grid = ceil(Hn * Wn / 256) x samples / rows.  The same two kernels: a pixel's arithmetic depends on its coordinates in the square
 * only, so the rows equal the square result's [:Hn, :Wn] bit for bit, and the entries above are the Hn = Wn = S case.  Plans and
 * items are unchanged (plan.S == S).  YM_EINVAL before any launch as above, and for a window outside 1 .. S on either axis. */
int ym_train_aug_image_batch_window(const ym_aug_item* items, int B, int S, int Hn, int Wn, int is_u8, float* out, ym_stream_t s);
int ym_train_aug_masks_batch_window(const ym_aug_item* items, int B, int S, int Hn, int Wn, int is_u8, const int32_t* keep_dev,
                                    int total_k, float* out, ym_stream_t s);

/* ---- evaluation inner products right after after_nms (next row f2) -----------------------------------------------
 * mask_iou (utils/box_utils.py:189-200): masks_a [n][P], masks_b [g][P] fp32 in {0,1} (P = img_h*img_w < 2^24) ->
 * iou [n][g] = inter / ((area_a + area_b) - inter), the reference's fp32 matmul evaluated as popcounts of bit rows
 * (exact, so bit-identical; 0/0 -> NaN).  Every mask is read from HBM once. */
size_t ym_mask_iou_workspace_bytes(int n, int g, int64_t P);
int ym_mask_iou(const float* masks_a, int n, const float* masks_b, int g, int64_t P, float* iou, void* workspace,
                size_t workspace_bytes, ym_stream_t s);
/* box_iou (utils/box_utils.py:8-37) of corner boxes [n][4] x [g][4] -> [n][g]. */
int ym_box_iou(const float* boxes_a, int n, const float* boxes_b, int g, float* iou, ym_stream_t s);
/* The matching loop of prep_metrics (utils/common_utils.py:186-216) for both IoU types and every threshold at once:
 * matched[type][t][i] = 1 iff prediction i (visited in order, class pred_cls[i]) found an unused gt of its class with
 * IoU > thresholds[t] (largest such IoU; double comparison like the python floats).  g <= 512. */
int ym_match_detections(const float* iou_box, const float* iou_mask, const int32_t* pred_cls, const int32_t* gt_cls, int n,
                        int g, const double* thresholds, int T, int num_classes, uint8_t* matched, ym_stream_t s);

/* COCO RLE of n binary masks [n][H][W] (fp32, nonzero = foreground), next row f3: what pycocotools.mask.encode(
 * np.asfortranarray(mask)) + .decode('ascii') yield in MakeJson.add_mask (utils/common_utils.py:88-96).  Per mask i:
 * counts[i*cap_runs .. +nruns[i]) = column-major run lengths starting with the zeros run, and the compressed ASCII string
 * str[i*cap_str .. +str_len[i]).  If a mask needs more than cap_runs runs (or cap_str bytes) nruns[i] still holds the
 * number of runs and str_len[i] = -1: call again with larger buffers.  W <= 4096; workspace >= n*cap_runs*4 bytes. */
int ym_rle_encode(const float* masks, int n, int H, int W, uint32_t* counts, int cap_runs, int32_t* nruns, uint8_t* str,
                  int cap_str, int32_t* str_len, void* workspace, size_t workspace_bytes, ym_stream_t s);

/* COCO annotation -> dense instance masks, next row f4 (the reader): what `self.coco.annToMask(aa)` yields per annotation in
 * COCODetection.__getitem__ (utils/coco.py:96) = pycocotools annToRLE (frPyObjects over the polygon list, merge = union) +
 * decode, i.e. cocoapi maskApi.c rleFrPoly / rleMerge / rleDecode.
 * ym_poly_to_mask: xy = every polygon's vertices (x0, y0, x1, y1, ... as in the JSON, float64) back to back; polygon p owns the
 *   vertices [poly_off[p], poly_off[p+1]) (counted in (x, y) pairs); annotation a owns the polygons [ann_off[a], ann_off[a+1]).
 * ym_runs_to_mask: the uncompressed-RLE form ({'counts': [...]}): annotation a owns counts[run_off[a] .. run_off[a+1]).
 * masks: [n][H][W] uint8 {0, 1}, 4-byte aligned.  W <= 4096.  Masks whose two bitmaps (see ym_ann_to_mask_workspace_bytes) do
 * not fit the LDS need that much workspace; otherwise workspace may be NULL. */
size_t ym_ann_to_mask_workspace_bytes(int n, int H, int W);
int ym_poly_to_mask(const double* xy, const int32_t* poly_off, const int32_t* ann_off, int n, int H, int W, uint8_t* masks,
                    void* workspace, size_t workspace_bytes, ym_stream_t s);
int ym_runs_to_mask(const uint32_t* counts, const int32_t* run_off, int n, int H, int W, uint8_t* masks, void* workspace,
                    size_t workspace_bytes, ym_stream_t s);

/* ym_ann_to_mask_ragged: the annotations of B <= YM_RAGGED_MAX_IMAGES images of DIFFERENT sizes, polygon lists and run lengths mixed,
 * in ONE launch (the batched loader; ym_poly_to_mask / ym_runs_to_mask are its one-image instances: the same kernel, the same bits).
 * Host tables, read during the call and passed to the kernel by value -- no device copy, no synchronisation, nothing to keep alive
 * (the contract of ym_after_nms_ragged, whose table type `images` borrows; declared below):
 *   images[b]    = {img_h_b, img_w_b, offset_b}: image b's block is [n_b][img_h_b][img_w_b] uint8 at masks + offset_b BYTES, what
 *                  ym_poly_to_mask writes for that image alone; offset_b is a multiple of YM_RAGGED_ALIGN_BYTES, blocks do not overlap;
 *   ann_first    = [B + 1]: image b owns the annotations [ann_first[b], ann_first[b + 1]) (n_b = 0 is allowed), ann_first[0] = 0,
 *                  n = ann_first[B]; the annotations are ordered by image.
 * Device arrays, indexed over the whole batch:
 *   ann_kind[a]  = 0: a list of polygons, 1: uncompressed run lengths;
 *   ann_off      = [n + 1]: annotation a owns the entries item_off[ann_off[a] .. ann_off[a + 1]): the start of each of its items, then
 *                  one closing end (the two kinds index different arrays, so every annotation closes its own list).  An item of a
 *                  polygon annotation is a polygon and its entries count (x, y) pairs of `xy`; a run-length annotation has exactly
 *                  one item and its two entries index `counts`.  An annotation without polygons owns the closing entry alone.
 * `xy` may be NULL when no annotation is a polygon list, `counts` when none is run lengths.  masks is 4-byte aligned, W <= 4096 and
 * H * W < 2^31 per image.  Images whose two bitmaps do not fit the LDS (ym_ann_to_mask_workspace_bytes(1, H, W) > 0) take them from
 * `workspace`, one slice per annotation: ym_ann_to_mask_ragged_workspace_bytes = the sum of those (0 when every image fits, and 0
 * for tables the entry would refuse); YM_ENOSPC when it is short.  n = 0 launches nothing. */
struct ym_ragged_image;
size_t ym_ann_to_mask_ragged_workspace_bytes(const struct ym_ragged_image* images, const int32_t* ann_first, int B);
int ym_ann_to_mask_ragged(const double* xy, const uint32_t* counts, const int32_t* item_off, const int32_t* ann_off,
                          const int32_t* ann_kind, const struct ym_ragged_image* images, const int32_t* ann_first, int B,
                          uint8_t* masks, void* workspace, size_t workspace_bytes, ym_stream_t s);

/* ---- training: weight gradient, batch-norm with batch statistics, small backward ops, SGD -------------------
 * These replace what autograd + ATen/cuDNN execute for `loss_total.backward()` / `optimizer.step()`
 * (reference train.py:124-130) and nn.BatchNorm2d in train mode (modules/resnet.py:10-14,46). */

/* OIHW weight -> [Cin][KH][KW][cout_pad] for the transposed gather above (cout_pad % 32 == 0, zero padded). */
int ym_pack_conv_weight_dgrad(const float* w_oihw, float* w_packed, int Cout, int Cin, int KH, int KW, int cout_pad,
                              ym_stream_t s);

/* All the weight packings of a training step in one launch (after the optimizer step every layer's forward and dgrad image is
 * stale at once).  items_dev: DEVICE array, one entry per destination image, ordered by first_chunk:
 *   kind 0: ym_pack_conv_weight   into dst [rows][pad_b]          (pad_a = cin_pad, pad_b = k_pad, rows >= cout zero padded)
 *   kind 1: ym_pack_conv_weight_dgrad into dst [cin][kh][kw][pad_a] (pad_a = cout_pad)
 * Chunks of an item: kind 0: ceil(rows * pad_b / 1024); kind 1: ceil(cin*kh*kw / 32) * (pad_a / 32) (32 x 32 transpose tiles).
 * first_chunk = running sum of the chunks of the preceding items; total_chunks = the sum over all items. */
typedef struct {
    const float* src;        /* OIHW weight */
    float* dst;
    int32_t cout, cin, kh, kw, pad_a, pad_b, rows, kind;
    uint32_t first_chunk;
    uint32_t reserved;
} ym_pack_item;
int ym_pack_conv_weights_batch(const ym_pack_item* items_dev, int n_items, int total_chunks, ym_stream_t s);

typedef struct {
    const float* x;          /* forward input NHWC [B][H][W][Cin] (Cin = padded channel pitch; 4 for the stem) */
    const float* dy;         /* output gradient [B][Ho][Wo][Cout] (Cout = channel pitch, multiple of 4) */
    float* dw;               /* OIHW [Cout_real][Cin_real][KH][KW], overwritten */
    int32_t B, H, W, Cin, Cin_real, Cout, Cout_real, KH, KW, stride, pad, Ho, Wo;
    int32_t msplit;          /* 0 = heuristic; pixel-range slices across the grid */
    int32_t accumulate;      /* 1: dw += gradient (a weight shared by several convs of one step, e.g. the prediction head over the */
                             /* five FPN levels, modules/yolact.py:149-153); 0: overwrite                                         */
    int32_t row_end[2];      /* output-channel ranges routed to separate OIHW tensors (the head's conf | bbox | coef convs run as   */
    float* dw_seg[2];        /* ONE 351-channel conv): rows [0,row_end[0]) -> dw, [row_end[0],row_end[1]) -> dw_seg[0],            */
                             /* [row_end[1],Cout_real) -> dw_seg[1].  row_end[0] = 0 means a single tensor (dw).                 */
    int32_t lds_buffers;     /* tuning knob: 0 / 2 = double-buffered pixel steps (2 workgroups per CU), 1 = single buffer (3 per CU);   */
                             /* 22 / 23 / 24 = operands DMA'd global -> LDS (no staging registers): 32 pixels x ring of 2, 16 pixels x  */
                             /* ring of 3 / 4 (more than 64 output channels only; Cin % 32 != 0 runs as 2).  Same products in the same  */
                             /* order: for a given msplit every variant returns the same bits.                                           */
} ym_wgrad_desc;
size_t ym_conv2d_wgrad_workspace_bytes(const ym_wgrad_desc* d);
int ym_conv2d_wgrad(const ym_wgrad_desc* d, void* workspace, size_t workspace_bytes, ym_stream_t s);
/* The two halves of ym_conv2d_wgrad apart, so that the slab reductions of MANY layers run as one launch (a res101 step has 104
 * backbone weight gradients; reference: one `at::conv_backward` weight kernel per layer under `loss.backward()`, train.py:125).
 * ym_conv2d_wgrad_slabs: first pass only -- the msplit partial gradients stay in `workspace` (which must then live, unshared, until
 * the batched reduction has run) and *item describes the pending reduction (d->row_end[0] must be 0: one destination tensor).
 * ym_wgrad_reduce_batch: `items_dev` = n_items such records in DEVICE memory, `first_block` of each set by the caller to the sum of
 * `blocks` of the records before it, total_blocks = the sum over all; sums every item's slabs in slab order (the same bits as
 * ym_conv2d_wgrad) into its OIHW tensor.  Items of one batch must not share a destination. */
typedef struct {
    const float* slabs;      /* = workspace of the slab pass */
    float* dw;               /* OIHW destination (d->dw) */
    uint32_t first_block;    /* IN: set by the caller when it builds the table */
    uint32_t blocks;         /* OUT: 256-thread blocks this item occupies in the batched launch */
    uint32_t plan[14];       /* OUT: opaque (sizes, slab stride, division constants) */
} ym_wgrad_reduce_item;
int ym_conv2d_wgrad_slabs(const ym_wgrad_desc* d, void* workspace, size_t workspace_bytes, ym_wgrad_reduce_item* item, ym_stream_t s);
int ym_wgrad_reduce_batch(const ym_wgrad_reduce_item* items_dev, int n_items, uint32_t total_blocks, ym_stream_t s);

/* BatchNorm2d forward in TRAIN mode on a conv output y [M][C] (C % 4 == 0): batch mean / biased variance
 * (fp64 accumulation), running stats updated in place with `momentum` (unbiased variance, torch semantics),
 * out = relu?( (y-mean)*invstd*gamma + beta + residual? ).  save_mean/save_invstd [C] feed the backward.
 * workspace >= 16*C bytes; with ym_bn_train_fwd_workspace_bytes(M, C) the statistics pass writes per-workgroup partials to
 * workspace + 16*C as double[rows][2][C], rows = (ym_bn_train_fwd_workspace_bytes(M, C) - 16*C) / (16*C), and sums them in the
 * order of ym_bn_partials_finish (no atomics); the first 16*C bytes then hold sum[C] | sumsq[C]. */
size_t ym_bn_train_fwd_workspace_bytes(int64_t M, int C);
int ym_bn_train_fwd(const float* y, int64_t M, int C, const float* gamma, const float* beta, float eps, float momentum,
                    float* running_mean, float* running_var, const float* residual, int relu, float* out,
                    float* save_mean, float* save_invstd, void* workspace, size_t workspace_bytes, ym_stream_t s);
/* Same, but the first 16*C bytes of `workspace` already hold the fp64 sum[C] | sumsq[C] of y (accumulated by
 * ym_conv2d_fwd through ym_conv_desc.bn_sum / bn_sumsq): skips the statistics pass over y. */
int ym_bn_train_fwd_stats(const float* y, int64_t M, int C, const float* gamma, const float* beta, float eps,
                          float momentum, float* running_mean, float* running_var, const float* residual, int relu,
                          float* out, float* save_mean, float* save_invstd, const void* stats, ym_stream_t s);

/* Backward of the above: dz = dout * (out > 0 if relu); dres (optional) = dz; dgamma/dbeta [C];
 * out may be NULL with relu = 1 when the forward had NO residual and `beta` is given: the mask is then re-derived from y with the
 * forward's exact affine (one pass less over HBM); beta is otherwise unused and may be NULL.
 * dy = gamma*invstd*(dz - mean(dz) - xhat*mean(dz*xhat)).  workspace >= 16*C bytes; with
 * ym_bn_train_bwd_workspace_bytes(M, C) the column sums use per-workgroup partials (larger grid, no atomics, ordered sum). */
size_t ym_bn_train_bwd_workspace_bytes(int64_t M, int C);
int ym_bn_train_bwd(const float* dout, const float* out, const float* y, int64_t M, int C, const float* gamma,
                    const float* beta, const float* save_mean, const float* save_invstd, int relu, float* dy, float* dres,
                    float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, ym_stream_t s);

/* Second pass of ym_bn_train_bwd alone: `stats` = fp64 sum_m dz [C] | sum_m dz*xhat [C], already accumulated by the epilogue of the
 * data-gradient conv that produced `dout` (ym_conv_desc.bnb_*).  Every other argument as in ym_bn_train_bwd. */
int ym_bn_train_bwd_apply(const float* dout, const float* out, const float* y, int64_t M, int C, const float* gamma,
                          const float* beta, const float* save_mean, const float* save_invstd, int relu, float* dy, float* dres,
                          float* dgamma, float* dbeta, const void* stats, ym_stream_t s);

/* Gradient of the fused prediction-head output w.r.t. the 351(+pad)-channel conv output, for all FPN levels in one launch:
 * the loss hands back dclass [B][N][nc], dbox [B][N][4], dcoef [B][N][cd] (N = anchors of all levels, anchor = (pixel, a) level by
 * level); row r of dz (level-major "pyramid" order: level l owns rows lev_row[l] .. lev_row[l+1), each B*hw_l rows = (image, pixel))
 * gets [na*nc | na*4 | na*cd * (1 - coef^2) | 0-pad] = the reference's permute/reshape/cat/tanh backward (modules/yolact.py:27-30,
 * 155-157).  lev_row / lev_anchor: int32[nlev+1] on the HOST (row offsets, anchor offsets of the levels).  g_scale: optional device
 * float[3] multiplying the class / box / coef parts (the upstream gradients of the loss terms), NULL = 1. */
int ym_head_grad_gather(const float* dclass, const float* dbox, const float* dcoef, const float* coef, int B, int N, int nc, int cd,
                        int na, int nlev, const int32_t* lev_row, const int32_t* lev_anchor, int pitch, const float* g_scale,
                        float* dz, ym_stream_t s);
/* dst_i[0..n_i) = src[off_i .. off_i + n_i) for up to three destinations (or += with accumulate): splits a concatenated bias /
 * statistics vector back into the parameters' own gradient slots in one launch. */
int ym_scatter3(const float* src, float* d0, int n0, float* d1, int n1, float* d2, int n2, int accumulate, ym_stream_t s);

/* Backward of a fused conv epilogue `y = act(conv + bias)`: dz = dy * act'(y) (dz may be NULL or == dy for
 * YM_ACT_NONE), dbias[C] = column sums of dz (optional).  workspace >= 8*C bytes when dbias != NULL; with
 * >= 16*C + min(1024, ceil(M/32..)) * 16*C bytes (ym_bn_train_bwd_workspace_bytes(M, C) always suffices) the sums use per-workgroup
 * partials + an ordered finish instead of fp64 atomics. */
int ym_act_bias_bwd(const float* dy, const float* y, int64_t M, int C, int act, float* dz, float* dbias, void* workspace,
                    size_t workspace_bytes, ym_stream_t s);

/* lincomb_mask_loss (modules/yolact.py:241-291) for ONE image, forward and backward in one pass on the f32 MFMA:
 *   loss += sum_p (wscale/area_p) * sum_pix BCE(crop_p(sigmoid(proto[pix] . coef_p)), gt_masks_ds[gt_idx[p]][pix])
 * and, with gscale = d(total)/d(loss_i) (= mask_alpha/Hp/Wp/total_pos), dproto [Hp*Wp][32] (overwritten) and
 * dcoef_full[anchor_idx[p]][32] (rows of the positives overwritten).  proto [Hp*Wp][32], coef_pos [n][32], box_pos [n][4]
 * (matched gt boxes: crop window, padding 1, and area), gt_masks_ds [n_gt][Hp*Wp] in {0,1}, n <= 128.
 * loss_accum is a device fp64 scalar the caller zeroes once per batch. */
size_t ym_mask_loss_workspace_bytes(void);
int ym_mask_loss_fwd_bwd(const float* proto, const float* coef_pos, const float* box_pos, const int32_t* gt_idx,
                         const float* gt_masks_ds, const int64_t* anchor_idx, int n, int Hp, int Wp, float wscale, float gscale,
                         double* loss_accum, float* dproto, float* dcoef_full, void* workspace, size_t workspace_bytes,
                         ym_stream_t s);
/* The same for a batch in one launch pair (workgroup row = image), reading the positives' coefficients / matched boxes /
 * matched gt index straight from the per-image full tensors through anchor_idx (no gathered copies): items is a HOST array. */
typedef struct {
    const float* proto;          /* [Hp*Wp][32] */
    const float* coef_full;      /* [N][32] coefficient predictions of the image */
    const float* anchor_box;     /* [N][4]  matched gt box per anchor (ym_match_anchors) */
    const int64_t* anchor_gt;    /* [N]     matched gt index per anchor */
    const float* gt_masks_ds;    /* [n_gt][Hp*Wp] in {0,1} */
    const int64_t* anchor_idx;   /* [n]     anchors trained on (the positives, sub-sampled to masks_to_train) */
    int32_t n;                   /* 0 <= n <= 128; 0: the item is skipped */
    float wscale;                /* positives / n */
    const int32_t* n_dev;        /* NULL, or a device int32 holding the image's positive count: the kernel trains on the first
                                    min(*n_dev, n) entries of anchor_idx and uses wscale = *n_dev / that (the host never reads it) */
    float* dproto;               /* [Hp*Wp][32] overwritten (untouched when n == 0) */
    float* dcoef_full;           /* [N][32] rows anchor_idx overwritten */
} ym_mask_loss_item;
size_t ym_mask_loss_batch_workspace_bytes(int B);
/* total_pos_dev: NULL, or a device int32 by which gscale is divided (gscale = mask_alpha / Hp / Wp then). */
int ym_mask_loss_batch(const ym_mask_loss_item* items, int B, int Hp, int Wp, float gscale, const int32_t* total_pos_dev,
                       double* loss_accum, void* workspace, size_t workspace_bytes, ym_stream_t s);
/* Window training: the prototype map is the top-left Hp x Wp of a VIRTUAL Pv x Pv map (Pv >= Hp, Wp) and the boxes live in that
 * square's frame.  The crop window of a positive is box * Pv on both axes with the reference's padding of 1, clamped to the
 * physical map: rows >= Hp and columns >= Wp do not exist, contribute nothing and are never read.  1 / area uses the box as it
 * is; the caller's gscale carries mask_alpha / Pv / Pv.  Hp * Wp need not be a multiple of the 32-pixel tile.  Pv = 0: per-axis
 * extents -- the two entries above are that instance of the same kernels and return the same bits.  YM_EINVAL for 0 < Pv < Hp or Wp. */
int ym_mask_loss_batch_window(const ym_mask_loss_item* items, int B, int Hp, int Wp, int Pv, float gscale,
                              const int32_t* total_pos_dev, double* loss_accum, void* workspace, size_t workspace_bytes, ym_stream_t s);
int ym_mask_loss_fwd_bwd_window(const float* proto, const float* coef_pos, const float* box_pos, const int32_t* gt_idx,
                                const float* gt_masks_ds, const int64_t* anchor_idx, int n, int Hp, int Wp, int Pv, float wscale,
                                float gscale, double* loss_accum, float* dproto, float* dcoef_full, void* workspace,
                                size_t workspace_bytes, ym_stream_t s);

/* match() for ONE image (utils/box_utils.py:57-83, encode :104-114): gt_boxes_cls [g][5] = (x1,y1,x2,y2,class) in [0,1]
 * coordinates, anchors [N][4] (cx,cy,w,h).  Writes offsets [N][4], conf [N] int64 (class+1 / 0 background / -1 neutral),
 * anchor_box [N][4] (matched gt corners), anchor_gt [N] int64 (matched gt index).  First maximum wins a tie (torch.max), the
 * last gt wins a shared best anchor (the sequential loop :72-73).  1 <= g <= 256; workspace >= 4*N bytes. */
int ym_match_anchors(const float* gt_boxes_cls, int g, const float* anchors, int N, float pos_thre, float neg_thre,
                     float* offsets, int64_t* conf, float* anchor_box, int64_t* anchor_gt, void* workspace,
                     size_t workspace_bytes, ym_stream_t s);

/* The same for a batch in one launch (workgroup = image): gt_boxes_cls / g are HOST arrays of B device pointers / gt counts;
 * the outputs are the [B][N]... batch buffers; workspace >= 4*B*N bytes. */
int ym_match_anchors_batch(const float* const* gt_boxes_cls, const int32_t* g, int B, const float* anchors, int N, float pos_thre,
                           float neg_thre, float* offsets, int64_t* conf, float* anchor_box, int64_t* anchor_gt, void* workspace,
                           size_t workspace_bytes, ym_stream_t s);

/* category_loss (modules/yolact.py:205-232: OHEM hard negatives at neg_pos_ratio, softmax CE summed / total positives) and
 * box_loss (:234-239: smooth-L1 over positives / total positives) for a batch, with their gradients (d total / d input):
 * class_p [B][N][C], box_p/offsets [B][N][4], conf [B][N] -> dclass, dbox (fully overwritten), num_pos int32 [B+1]
 * (per image, then the total) and the two device fp64 scalars loss_c, loss_b (already scaled by conf_alpha / bbox_alpha).
 * Equal OHEM marks are ranked by anchor index (torch.sort leaves their order unspecified).  No host synchronisation. */
size_t ym_loss_workspace_bytes(int B, int N);
int ym_class_box_loss(const float* class_p, const float* box_p, const float* offsets, const int64_t* conf, int B, int N, int C,
                      float conf_alpha, float bbox_alpha, int neg_pos_ratio, float* dclass, float* dbox, int32_t* num_pos,
                      double* loss_c, double* loss_b, void* workspace, size_t workspace_bytes, ym_stream_t s);

/* The positives the mask loss trains on (modules/yolact.py:255-267): conf [B][N] (> 0 = positive), num_pos [B] their counts (from
 * ym_class_box_loss), keys [B][N] iid uniform [0,1) draws.  idx[b][0 .. min(count, cap)) = all positives of image b in anchor order
 * when count <= cap, else the `cap` positives with the largest keys (a uniformly random subset, the reference's randperm[:cap]),
 * in anchor order; equal keys by anchor index.  No host synchronisation. */
int ym_select_positives(const int64_t* conf, const float* keys, int B, int N, int cap, const int32_t* num_pos, int64_t* idx,
                        ym_stream_t s);

/* The gt masks at the size of a prediction map (modules/yolact.py:247-251, :302-304): out [n][out_h][out_w] =
 * F.interpolate(masks [n][H][W], (out_h, out_w), bilinear, align_corners=False) > 0.5, exactly 0.0f / 1.0f, with one scale per
 * axis.  For a square map it equals ym_mask_resize_binarize bit for bit; that one scales both axes by the longer side. */
int ym_gt_masks_downsample(const float* masks, int n, int H, int W, int out_h, int out_w, float* out, ym_stream_t s);

/* semantic_seg_loss (modules/yolact.py:293-313) for ONE image: seg_nhwc [P][pitch] logits (channels >= num_classes are
 * padding), gt_masks_ds [g][P] in {0,1} (down-sampled + binarised gt masks), gt_cls[j*gt_cls_stride] the class of gt j.
 * loss_accum += coeff * sum BCE-with-logits(seg, target) with target[c][pix] = max over gts of class c; dseg [P][pitch] =
 * coeff * (sigmoid - target), zero in the padding channels.  coeff = semantic_alpha / H / W / B. */
int ym_semantic_loss(const float* seg_nhwc, int P, int pitch, int num_classes, const float* gt_masks_ds, const int64_t* gt_cls,
                     int gt_cls_stride, int g, float coeff, float* dseg, double* loss_accum, ym_stream_t s);
/* The same for the batch in one launch: seg_nhwc / dseg [B][P][pitch]; gt_masks_ds / gt_cls / g are HOST arrays of B device
 * pointers / gt counts (g[i] = 0: no gt, pointers ignored). */
int ym_semantic_loss_batch(const float* seg_nhwc, int B, int P, int pitch, int num_classes, const float* const* gt_masks_ds,
                           const int64_t* const* gt_cls, int gt_cls_stride, const int32_t* g, float coeff, float* dseg,
                           double* loss_accum, ym_stream_t s);

int ym_maxpool3x3s2_bwd(const float* x, const float* dy, float* dx, int B, int H, int W, int C, ym_stream_t s);
/* The training pair that carries the argmax instead of re-deriving it: fwd_idx also writes idx [B][Ho][Wo][C] uint8 (window
 * position 3*dy + dx of the winner under ATen's rule, 4-byte aligned), bwd_idx gathers dx from idx + dy alone (x is not read).
 * ATen's rule: the first maximum in scan order, which for a window of nothing but -inf is its first valid (non-padding) element, and
 * the last NaN of a window that holds one.  ym_maxpool3x3s2_bwd re-derives the same winner from x: both give the same dx. */
int ym_maxpool3x3s2_fwd_idx(const float* in, float* out, uint8_t* idx, int B, int H, int W, int C, ym_stream_t s);
int ym_maxpool3x3s2_bwd_idx(const uint8_t* idx, const float* dy, float* dx, int B, int H, int W, int C, ym_stream_t s);
int ym_bilinear2x_bwd(const float* dy, float* dx, int B, int H, int W, int C, int align_corners, ym_stream_t s);

/* torch.optim.SGD(momentum, weight_decay) on one flat fp32 buffer (reference train.py:61,130). */
int ym_sgd_step(float* param, const float* grad, float* momentum_buf, int64_t n, float lr, float momentum,
                float weight_decay, int first_step, ym_stream_t s);

/* ---- small NHWC ops ------------------------------------------------------------------------------ */

/* MaxPool2d(3, stride 2, pad 1), reference modules/resnet.py:91. C % 4 == 0. */
int ym_maxpool3x3s2_fwd(const float* in, float* out, int B, int H, int W, int C, ym_stream_t s);
/* The ResNet stem in eval mode as ONE launch (modules/resnet.py:86-91: conv1 7x7/2 pad 3 -> bn1 -> relu -> maxpool 3x3/2 pad 1):
 * img NCHW [B][3][H][W] (read directly: no NHWC4 copy), w_packed = ym_pack_conv_weight(conv1.weight, cin_pad 4, k_pad 224)
 * [64][224], scale / shift [64] from ym_fold_bn, out NHWC [B][Hp][Wp][64] with Hp = ((H-1)/2+1 + 1)/2 ... (the two layers'
 * usual output sizes).  The 64-channel conv output never reaches HBM.  Same MFMA order and epilogue arithmetic as
 * ym_nchw_to_nhwc4 + ym_conv2d_fwd (stem mode) + ym_maxpool3x3s2_fwd: the same bits. */
int ym_stem_conv_bn_relu_maxpool(const float* img_nchw, const float* w_packed, const float* scale, const float* shift, float* out,
                                 int B, int H, int W, int k_pad, ym_stream_t s);

/* Bilinear x2 upsample, align_corners 0 (FPN, modules/yolact.py:70-71) or 1 (ProtoNet, :43). C % 4 == 0. */
int ym_bilinear2x_fwd(const float* in, float* out, int B, int H, int W, int C, int align_corners, ym_stream_t s);

/* softmax over the last dim of [rows][C] (F.softmax(class_pred, -1), modules/yolact.py:163). in may equal out. */
int ym_softmax_rows(const float* in, float* out, int64_t rows, int C, ym_stream_t s);

/* ---- Swin-T blocks (modules/swin_transformer.py); Linear layers are 1x1 ym_conv2d_fwd on [tokens][C] ---------- */

/* nn.LayerNorm over the last dim of [M][C] (C % 4 == 0, C <= 1536); in-place allowed. (:225,228,297,425,:470) */
int ym_layernorm(const float* x, const float* gamma, const float* beta, float eps, float* out, int64_t M, int C,
                 ym_stream_t s);

/* PatchMerging gather + norm (:299-323): x NHWC [B][H][W][C] -> out [B*ceil(H/2)*ceil(W/2)][4C] =
 * LayerNorm(concat(x[2i,2j], x[2i+1,2j], x[2i,2j+1], x[2i+1,2j+1])), zero padded for odd H/W. */
int ym_patch_merge_layernorm(const float* x, int B, int H, int W, int C, const float* gamma, const float* beta, float eps,
                             float* out, ym_stream_t s);

/* (Shifted-)window multi-head self-attention, everything between the qkv and proj Linears of one block
 * (WindowAttention.forward :172-199 + pad/roll/window_partition/window_reverse/un-roll/crop of :249-283):
 * qkv [B*H*W][3C] (q|k|v, head-major inside each), qkv_bias [3C] (value of padded tokens), rel_bias_table
 * [(2*window-1)^2][heads]; window must be 7 and C/heads == 32; shift 0 or window/2.  out [B*H*W][C]. */
int ym_swin_window_attention(const float* qkv, const float* qkv_bias, const float* rel_bias_table, int B, int H, int W, int C,
                             int heads, int window, int shift, float* out, ym_stream_t s);

/* ---- pre-processing (SURVEY.md §8f "next" row 1) ------------------------------------------------------------- */

/* `val_aug(img, val_size)` (utils/augmentations.py:219-227 = pad_to_square :138-165 + cv2.resize :188 +
 * normalize_and_toRGB :212-216) on the device: HWC BGR image (uint8 if is_uint8 else float32, DEVICE pointer) ->
 * out [3][S][S] float32 RGB, (x - mean) / std.  mean_bgr / std_bgr are HOST pointers to 3 floats (config.py:66-67). */
int ym_val_preprocess(const void* img_hwc_bgr, int is_uint8, int H, int W, int S, const float* mean_bgr,
                      const float* std_bgr, float* out_chw_rgb, ym_stream_t s);
/* ym_val_preprocess_batch (declared with the ragged tables below): B frames of different sizes in one launch. */

/* ---- detection post-processing (utils/output_utils.py) ---------------------------------------------- */

typedef struct {
    int32_t num_anchors;     /* N */
    int32_t num_classes;     /* C including background (81) */
    int32_t coef_dim;        /* 32 */
    int32_t top_k;           /* cfg.top_k = 200 (<= 256) */
    int32_t max_det;         /* cfg.max_detections = 100 (<= 128) */
    float score_thre;        /* cfg.nms_score_thre = 0.05 */
    float iou_thre;          /* cfg.nms_iou_thre = 0.5 */
    float img_size;          /* cfg.img_size, used by the greedy ("traditional") path only */
} ym_nms_cfg;

/* The one workspace size for both single-image entries below: the larger of what fast_nms and greedy NMS need for one image (the
 * latter, = ym_greedy_nms_batch_workspace_bytes(cfg, 1)).  Host only, 0 on a bad cfg. */
size_t ym_nms_workspace_bytes(const ym_nms_cfg* cfg);

/* `nms()` with fast_nms (utils/output_utils.py:126-163 + :11-43 + box_iou utils/box_utils.py:8-37)
 * for ONE image.  Inputs: class_pred [N][C] (softmaxed), box_pred [N][4], coef_pred [N][coef_dim],
 * anchors [N][4] (cx,cy,w,h).  Outputs (device): out_count int32[1] (n <= max_det; 0 means the
 * reference returns five Nones), out_ids int64[max_det], out_scores f32[max_det],
 * out_boxes f32[max_det][4] (x1,y1,x2,y2 in 0..1), out_coefs f32[max_det][coef_dim]. */
int ym_detect_fast_nms(const float* class_pred, const float* box_pred, const float* coef_pred,
                       const float* anchors, const ym_nms_cfg* cfg, int32_t* out_count, int64_t* out_ids,
                       float* out_scores, float* out_boxes, float* out_coefs, void* workspace,
                       size_t workspace_bytes, ym_stream_t s);

/* The same for a batch of B images in ONE launch set (grid row = image; SURVEY.md §0.3: the reference's nms() is batch-1 only,
 * eval.py loops over images): class_pred [B][N][C], box_pred [B][N][4], coef_pred [B][N][coef_dim]; outputs out_count int32[B],
 * out_ids [B][max_det], out_scores [B][max_det], out_boxes [B][max_det][4], out_coefs [B][max_det][coef_dim] (rows past an
 * image's count are unspecified).  Per image the result equals ym_detect_fast_nms on that image.
 * workspace >= ym_nms_batch_workspace_bytes(cfg, B). */
size_t ym_nms_batch_workspace_bytes(const ym_nms_cfg* cfg, int B);
int ym_detect_fast_nms_batch(const float* class_pred, const float* box_pred, const float* coef_pred, const float* anchors,
                             const ym_nms_cfg* cfg, int B, int32_t* out_count, int64_t* out_ids, float* out_scores,
                             float* out_boxes, float* out_coefs, void* workspace, size_t workspace_bytes, ym_stream_t s);

/* Same contract, greedy per-class NMS: replaces traditional_nms (utils/output_utils.py:84-123) and the
 * Cython kernel it calls (cython_nms.pyx:24-74) without the 80 D2H/H2D round trips.  It IS ym_detect_greedy_nms_batch (below) with
 * B = 1: its rule, its checks, its workspace (workspace >= ym_nms_workspace_bytes(cfg)). */
int ym_detect_greedy_nms(const float* class_pred, const float* box_pred, const float* coef_pred,
                         const float* anchors, const ym_nms_cfg* cfg, int32_t* out_count, int64_t* out_ids,
                         float* out_scores, float* out_boxes, float* out_coefs, void* workspace,
                         size_t workspace_bytes, ym_stream_t s);

/* The greedy path for a batch of B images in ONE launch set (grid row = image), with the argument order, layouts and checks of
 * ym_detect_fast_nms_batch: 1 <= B <= 65535, YM_ENOSPC before any launch when the workspace is too small, out_count int32[B],
 * outputs padded to max_det rows per image (rows past an image's count are unspecified; an image without an anchor over the
 * score threshold gets out_count 0 and nothing else of it is written).
 *   Per class: candidates = kept anchors with score > score_thre; order = score descending, equal scores by HIGHER candidate
 *   index first (oracle/greedy_nms.c); a candidate is dropped iff an earlier KEPT candidate of its class has ovr >= iou_thre on
 *   the boxes multiplied by img_size ("+ 1" widths, heights and areas, IEEE division).  The kernel settles 64 sorted candidates
 *   at a time inside one wave and then tests all later ones against that chunk's survivors: two workgroup barriers per 64
 *   candidates, the sequential result exactly.  The order is a counting rank, O(n^2) per class of n candidates.
 *   Per image: the max_det highest scores over all kept (class, candidate) pairs, equal scores in class-major, ascending anchor
 *   order; boxes = (b * img_size) / img_size; coefficients gathered from coef_pred.
 * ym_detect_greedy_nms is this entry with B = 1, so B = 1 gives its values bit for bit by construction.
 * Workspace per image (every term rounded up to 256 bytes), with S = ym_nms_batch_workspace_bytes(cfg, 1), n = (C-1) * N:
 *   S + 4 n (candidate lists) + 4 (C-1) (their lengths) + n (kept flags)          when N <= 4096
 *   ... + 4 n (candidate by rank)                                                 when N >  4096
 * A class of up to 4096 candidates keeps its sorted boxes, scores, order and alive flags in LDS (25 bytes per candidate); a larger
 * one reads its boxes through the order in global memory.  N = 18525, C = 81: 19.8 MB per image.
 * ym_greedy_nms_batch_workspace_bytes is host only, linear in B, 0 on a bad cfg or B < 1. */
size_t ym_greedy_nms_batch_workspace_bytes(const ym_nms_cfg* cfg, int B);
int ym_detect_greedy_nms_batch(const float* class_pred, const float* box_pred, const float* coef_pred, const float* anchors,
                               const ym_nms_cfg* cfg, int B, int32_t* out_count, int64_t* out_ids, float* out_scores,
                               float* out_boxes, float* out_coefs, void* workspace, size_t workspace_bytes, ym_stream_t s);

/* y[i] = exp(x[i]) rounded to nearest float — the exp of the box decode (utils/output_utils.py:150, `torch.exp`), exposed so
 * that the parity suite can compare it with oracle/expf_cr.c on arbitrary inputs (bit-identical by construction: same IEEE
 * double operation sequence).  The reference's own torch.exp is MKL VML (1 ulp off this value in 1.1 % of inputs). */
int ym_expf_cr(const float* x, float* y, int64_t n, ym_stream_t s);

/* Drop-in for `cython_nms.nms(dets, thresh)` (cython_nms.pyx:24) on device data: dets [n][5]
 * (x1,y1,x2,y2,score), "+1" areas, suppress ovr >= thresh; keep_mask uint8[n] (1 = kept), in original
 * index order like np.where(suppressed == 0).  Equal scores go by HIGHER index first; one workgroup, the chunked suppression of
 * ym_detect_greedy_nms_batch over the one list, its order a counting rank (O(n^2)).  workspace >= ym_greedy_nms_workspace_bytes(n). */
size_t ym_greedy_nms_workspace_bytes(int n);
int ym_greedy_nms(const float* dets, int n, float thresh, uint8_t* keep_mask, int32_t* out_count,
                  void* workspace, size_t workspace_bytes, ym_stream_t s);

/* Mask assembly: sigmoid(proto[Hp*Wp][K] @ coef[n][K]^T) cropped to the box window (padding 1) ->
 * out [n][Hp][Wp].  Replaces utils/output_utils.py:217-222 (+ crop, utils/box_utils.py:147-168) and
 * the same product in lincomb_mask_loss (modules/yolact.py:275-276).  K must be 32. do_crop=0 skips crop. */
int ym_mask_assemble(const float* proto, const float* coefs, const float* boxes, int n, int Hp, int Wp,
                     int K, int do_crop, float* out, ym_stream_t s);

/* F.interpolate(masks, (S,S), bilinear, align_corners=False) -> gt(0.5) -> slice to [n][img_h][img_w]
 * (utils/output_utils.py:224-228), S = max(img_h, img_w).  out values are exactly 0.0f / 1.0f. */
int ym_mask_resize_binarize(const float* masks, int n, int Hp, int Wp, int img_h, int img_w, float* out,
                            ym_stream_t s);

/* box_p *= S; box_p.int()  (utils/output_utils.py:230-231): boxes_f is scaled IN PLACE like the reference. */
int ym_boxes_to_pixels(float* boxes_f, int32_t* boxes_px, int n, float S, ym_stream_t s);

/* after_nms (utils/output_utils.py:200-233) for a batch of B images in one launch set: prototype x coefficient product, sigmoid,
 * crop, bilinear resize to S = max(img_h, img_w), > 0.5, slice — fused, the [n][Hp][Wp] soft masks never reach HBM — plus the
 * in-place box scaling + truncation.  proto [B][Hp][Wp][32]; coefs [B][max_det][32], boxes [B][max_det][4] (scaled IN PLACE),
 * counts int32[B] on the DEVICE (NULL = every image has max_det detections; B = 1 with max_det = n is the single-image call);
 * masks [B][max_det][img_h][img_w] (only slots < count are written, on the fused and on the two-kernel path), boxes_px int32
 * [B][max_det][4].
 * workspace >= ym_after_nms_batch_workspace_bytes(...) (0 unless the image is much smaller than the prototype map). */
size_t ym_after_nms_batch_workspace_bytes(int max_det, int Hp, int Wp, int img_h, int img_w);
int ym_after_nms_batch(const float* proto, const float* coefs, float* boxes, const int32_t* counts, int B, int max_det, int Hp,
                       int Wp, int K, int img_h, int img_w, int do_crop, float* masks, int32_t* boxes_px, void* workspace,
                       size_t workspace_bytes, ym_stream_t s);

/* draw_img (utils/output_utils.py:327-369) on the device: masks blended with the class palette, box outlines, label plates, label
 * text, the fps overlay and the cutout matte, for B frames in the padded layout of ym_after_nms_batch.  Everything is integer
 * arithmetic, so the result is exact:
 *   masks (unless YM_DRAW_HIDE_MASK): s = (sum_i int(masks[i]) * (ids[i] + 1)) mod (num_classes - 1), every pixel becomes
 *     (4 * palette[s] + 6 * img + 5) / 10  ==  cv2.addWeighted(colour, 0.4, img, 0.6, 0);
 *   boxes (unless YM_DRAW_HIDE_BBOX): per pixel the smallest i that touches it wins (the reference draws i = n-1 .. 0): the 1-px
 *     outline through (x1,y1)-(x2,y2), the filled plate x1..x1+text_w, y1..y1+text_h+5 (inclusive) in palette[ids[i] + 1], the
 *     label "{name}: {score:.2f}" ("{name}" with YM_DRAW_HIDE_SCORE) in white with its baseline at (x1, y1 + 15);
 *   YM_DRAW_REAL_TIME: pixels y < text_h + 8, x < text_w + 8 become 3 * v / 5, then fps_text in white, baseline (0, text_h + 2);
 *   cutout_total (optional, [B][H][W][3]): img where s != 0, else 255.
 * Text uses the caller's 1-bit fixed-cell font: uint16 font[95][YM_DRAW_FONT_HEIGHT], codes 0x20..0x7E, bit x of a row = column x of
 * the YM_DRAW_FONT_ADVANCE wide cell; text_w = len * YM_DRAW_FONT_ADVANCE, text_h = YM_DRAW_FONT_HEIGHT.  The score text is
 * formatted on the device: cents = rint(double(score) * 100), round-half-to-even, i.e. Python's format.
 * img / out uint8 [B][H][W][3] BGR (out may be img); masks f32 [B][max_det][H][W] holding 0 / 1; ids int64, scores f32,
 * boxes_px int32 x4 [B][max_det]; counts int32[B] on the DEVICE (NULL = all max_det rows valid; B = 1 with max_det = n is the
 * single-picture call).  Rows past the count, and rows with score < visual_thre when visual_thre > 0, are skipped on the device; a
 * frame without a surviving row is copied unchanged.  palette uint8 [palette_n][3]; names char [num_names][YM_DRAW_NAME_STRIDE],
 * NUL-padded; labels are cut at YM_DRAW_LABEL_MAX characters.  fps_text is a HOST string (<= 32 characters).  No host
 * synchronisation, no device-to-host copy.  workspace >= ym_draw_workspace_bytes(B, max_det), max_det <= YM_DRAW_MAX_DET. */
#define YM_DRAW_HIDE_MASK 1
#define YM_DRAW_HIDE_BBOX 2
#define YM_DRAW_HIDE_SCORE 4
#define YM_DRAW_REAL_TIME 8
#define YM_DRAW_FONT_ADVANCE 12
#define YM_DRAW_FONT_HEIGHT 14
#define YM_DRAW_NAME_STRIDE 40
#define YM_DRAW_LABEL_MAX 44
#define YM_DRAW_MAX_DET 512
size_t ym_draw_workspace_bytes(int B, int max_det);
int ym_draw_detections_batch(const uint8_t* img, const float* masks, const int64_t* ids, const float* scores, const int32_t* boxes_px,
                             const int32_t* counts, int B, int max_det, int H, int W, const uint8_t* palette, int palette_n,
                             int num_classes, const char* names, int num_names, const uint16_t* font, int flags, float visual_thre,
                             const char* fps_text, uint8_t* out, uint8_t* cutout_total, void* workspace, size_t workspace_bytes,
                             ym_stream_t s);

/* The per-object mattes of cfg.cutout: out[i] = img where masks[i] != 0, else 255; img uint8 [H][W][3], masks f32 [n][H][W],
 * out uint8 [n][H][W][3] (full frames: the caller slices [y1:y2, x1:x2]). */
int ym_draw_cutout_objects(const uint8_t* img, const float* masks, int n, int H, int W, uint8_t* out, ym_stream_t s);


/* ---- bit-packed instance masks --------------------------------------------------------------------------------------------
 * Every consumer of a detection mask asks one question of a pixel (0 or 1), so the masks can travel as 1 bit per pixel:
 *   bits: uint64 [n][H][Wq], Wq = ceil(W / 64), contiguous.  Bit k (LSB = 0) of word j of row y of mask i is pixel (y, 64*j + k);
 *   bits at x >= W are ZERO (producers guarantee it, consumers rely on it).  In the padded batch form [B][max_det][H][Wq] the rows
 *   at or past an image's count are unspecified, like the dense tensor's.
 * 100 x 480 x 640 masks are 3.84 MB instead of 122.88 MB.  One wave-wide ballot over 64 consecutive pixels is one word.
 * Host view (little-endian): numpy.unpackbits(bits.view(uint8).reshape(n, H, Wq * 8), axis=-1, bitorder='little')[..., :W].
 *
 * ym_after_nms_batch_packed: ym_after_nms_batch with the masks written as bits.  Per pixel the arithmetic is the dense kernel's
 * (same patch, same source coordinates, same interpolation expression), so a bit equals (dense value != 0) exactly; the dense
 * tensor exists nowhere, not in the workspace either.  Same workspace as ym_after_nms_batch (ym_after_nms_batch_workspace_bytes:
 * the soft masks of the strongly down-scaled case). */
int ym_after_nms_batch_packed(const float* proto, const float* coefs, float* boxes, const int32_t* counts, int B, int max_det, int Hp,
                              int Wp, int K, int img_h, int img_w, int do_crop, uint64_t* mask_bits, int32_t* boxes_px,
                              void* workspace, size_t workspace_bytes, ym_stream_t s);
/* dense masks [n][H][W] (float32, or uint8 when is_u8; nonzero = foreground) -> bits, and bits -> float32 0.0 / 1.0. */
int ym_pack_masks(const void* masks, int is_u8, int n, int H, int W, uint64_t* bits, ym_stream_t s);
int ym_unpack_masks(const uint64_t* bits, int n, int H, int W, float* masks, ym_stream_t s);

/* ---- after_nms for a batch whose images differ in size ------------------------------------------------------------------------
 * ym_after_nms_ragged[_packed]: ym_after_nms_batch[_packed] with img_h, img_w replaced by a HOST table of B entries, one per image:
 * its output size and `offset`, the first element (float, or 64-bit word when packed) of its mask block in `masks`.  Image b's block
 * is [max_det][img_h_b][img_w_b] floats (packed: [max_det][img_h_b][ceil(img_w_b / 64)] words) at masks + offset_b: exactly what the
 * uniform entry writes for a batch of that one size, so every consumer of one image's padded rows takes the block as it is.  Rows
 * at or past counts[b] are NOT written, and nothing outside the blocks is.  boxes are scaled in place and boxes_px written with
 * S_b = max(img_h_b, img_w_b) per image.
 *   The table is read during the call and travels to the kernels by value in their arguments: no copy to the device, no
 * synchronisation, nothing to keep alive afterwards.  B <= YM_RAGGED_MAX_IMAGES.  Every block starts at a multiple of
 * YM_RAGGED_ALIGN_BYTES bytes from `masks` (the dense kernel stores 16 bytes at a time when img_w % 4 == 0, and an odd max_det x odd
 * height x odd width would leave the next block misaligned), `masks` itself is 16-byte aligned, blocks do not overlap: YM_EINVAL
 * otherwise.  One fused launch covers every image whose scale fits the fused kernel (grid = largest tile count x max_det x B; tiles
 * and slots an image does not have exit at once); images much smaller than the prototype map (max(h, w) under about 2.7x its side)
 * take the two-kernel path (ym_mask_assemble, then the resize bounded by counts[b] on the device: the launch set all four entries
 * share) one by one through `workspace` >= ym_after_nms_ragged_workspace_bytes(...) (0 when every image fits; also 0 for arguments
 * the entries would refuse). */
#define YM_RAGGED_MAX_IMAGES 32
#define YM_RAGGED_ALIGN_BYTES 256
typedef struct ym_ragged_image {
    int32_t img_h, img_w;
    int64_t offset; /* elements from `masks` to this image's block (for a table of frames: from the frame buffer to this frame) */
} ym_ragged_image;
size_t ym_after_nms_ragged_workspace_bytes(const ym_ragged_image* images, int B, int max_det, int Hp, int Wp);
int ym_after_nms_ragged(const float* proto, const float* coefs, float* boxes, const int32_t* counts, int B, int max_det, int Hp,
                        int Wp, int K, const ym_ragged_image* images, int do_crop, float* masks, int32_t* boxes_px, void* workspace,
                        size_t workspace_bytes, ym_stream_t s);
int ym_after_nms_ragged_packed(const float* proto, const float* coefs, float* boxes, const int32_t* counts, int B, int max_det, int Hp,
                               int Wp, int K, const ym_ragged_image* images, int do_crop, uint64_t* mask_bits, int32_t* boxes_px,
                               void* workspace, size_t workspace_bytes, ym_stream_t s);
/* ym_pack_masks_ragged: ym_pack_masks for the dense blocks of B <= YM_RAGGED_MAX_IMAGES images of different sizes in ONE launch.
 * `src` is a HOST array of B device pointers, block b = [rows[b]][img_h_b][img_w_b] float32 (uint8 when is_uint8; nonzero =
 * foreground); `rows` is a HOST array; both travel to the kernel by value with the table.  Output block b = [rows[b]][img_h_b]
 * [ceil(img_w_b / 64)] words at bits + images[b].offset, bit for bit what ym_pack_masks writes for that block alone (pad bits zero);
 * the table rules are those above (offsets in words).  A block of 0 rows is skipped; nothing outside the blocks is written. */
int ym_pack_masks_ragged(const void* const* src, int is_uint8, const int32_t* rows, const ym_ragged_image* images, int B,
                         uint64_t* bits, ym_stream_t s);

/* ---- window mode: a network that ran on the top-left Hn x Wn of its square input ---------------------------------------------------
 * The square input of a non-square frame is picture at the top-left and norm_mean (normalised: exactly 0.0) below / right of it.
 * ym_val_preprocess_window writes only the top-left Hn x Wn of the S x S result, the network runs on that, and its prototype map is
 * the top-left Hp x Wp = Hn/4 x Wn/4 of the VIRTUAL Pv x Pv map (Pv = S / 4) the square run would have produced; boxes stay in 0..1 of
 * the S x S square.  ym_after_nms_window[_packed] is ym_after_nms_ragged[_packed] (same table, same layout, same launch path; one
 * output size is the one-entry table) with that virtual extent:
 *   - box -> prototype pixels and the crop window use Pv on BOTH axes (clamped to [0, Pv] as before);
 *   - the resize scale is Pv / max(img_h_b, img_w_b) on both axes;
 *   - source indices clamp to the physical Hp - 1 / Wp - 1, so an output row whose source lies past the window reads row Hp - 1,
 *     crop status included (bilinear interpolation over the replicate-padded map);
 *   - boxes_px as before: S_b = max(img_h_b, img_w_b).
 * Pv >= max(Hp, Wp) (YM_EINVAL otherwise).  The older entries are the Pv = 0 case of the same kernels ("the map is the whole extent")
 * and return the bits they always did.  Workspace: ym_after_nms_window_workspace_bytes (the fused kernel is chosen by Pv / S). */
size_t ym_after_nms_window_workspace_bytes(const ym_ragged_image* images, int B, int max_det, int Hp, int Wp, int Pv);
int ym_after_nms_window(const float* proto, const float* coefs, float* boxes, const int32_t* counts, int B, int max_det, int Hp,
                        int Wp, int K, const ym_ragged_image* images, int Pv, int do_crop, float* masks, int32_t* boxes_px,
                        void* workspace, size_t workspace_bytes, ym_stream_t s);
int ym_after_nms_window_packed(const float* proto, const float* coefs, float* boxes, const int32_t* counts, int B, int max_det, int Hp,
                               int Wp, int K, const ym_ragged_image* images, int Pv, int do_crop, uint64_t* mask_bits,
                               int32_t* boxes_px, void* workspace, size_t workspace_bytes, ym_stream_t s);

/* ---- frames of different sizes: the two ends of a mixed-size request ----------------------------------------------------------
 * The same table type describes a batch of FRAMES: entry b = {img_h_b, img_w_b, offset_b}, frame b is HWC BGR [img_h_b][img_w_b][3]
 * at `frames + offset_b`, offset counted in elements of the frame buffer (bytes for uint8, floats for float32).  The rules are the
 * mask blocks': 1 .. YM_RAGGED_MAX_IMAGES entries, positive sizes, every frame at a multiple of YM_RAGGED_ALIGN_BYTES bytes, no two
 * frames overlapping (YM_EINVAL otherwise); the table is read during the call and travels by value in the kernel arguments.
 *
 * ym_val_preprocess_batch: ym_val_preprocess for B frames in ONE launch (grid = ceil(S * S / 256) x B), out [B][3][S][S].  It is the
 * same kernel as ym_val_preprocess (that entry is its B = 1 instance), so frame b of a batch equals the single call bit for bit.
 *
 * ym_draw_detections_ragged[_packed]: ym_draw_detections_batch[_packed] with `H, W` replaced by two tables and no cutout_total.
 * `frames[b]` is frame b's size and its first BYTE in both `img` and `out` (one layout for the two buffers; out == img is legal);
 * `mask_blocks` is the table that was given to ym_after_nms_ragged[_packed] (offsets in floats / 64-bit words from `masks`), its
 * sizes must equal `frames`' (YM_EINVAL); it may be NULL with YM_DRAW_HIDE_MASK.  B <= YM_RAGGED_MAX_IMAGES.  Output bytes per
 * frame are those of the uniform entry called on that frame alone.  At most two frame launches: the images whose rows are whole
 * 4-pixel groups at aligned addresses take the 16-byte path, the others the element-wise one; the grid is the largest tile count of
 * a launch's images x B, workgroups of other images or past an image's own tiles exit before touching memory.  Nothing outside
 * the frames is written.  Workspace: ym_draw_workspace_bytes(B, max_det), as for the uniform entries.  The four ym_draw_detections_*
 * entries share one launch path (draw.hip, draw_launches): only the limits differ -- B <= 65535 and the cutout matte for one frame
 * size, B <= YM_RAGGED_MAX_IMAGES and no matte for the tables -- and each entry reports errors under its own name. */
int ym_val_preprocess_batch(const void* frames, int is_uint8, const ym_ragged_image* images, int B, int S, const float* mean_bgr,
                            const float* std_bgr, float* out, ym_stream_t s);
/* The same launch with an output of [B][3][Hn][Wn], 0 < Hn, Wn <= S: the top-left window of every frame's S x S result, bit for bit
 * (a pixel's arithmetic depends on its own coordinates only; scale = max(img_h, img_w) / S as before).  Hn = Wn = S is
 * ym_val_preprocess_batch.  The caller picks a window that holds every frame's picture (rect_window in the Python package). */
int ym_val_preprocess_window(const void* frames, int is_uint8, const ym_ragged_image* images, int B, int S, int Hn, int Wn,
                             const float* mean_bgr, const float* std_bgr, float* out, ym_stream_t s);
int ym_draw_detections_ragged(const uint8_t* img, const float* masks, const int64_t* ids, const float* scores, const int32_t* boxes_px,
                              const int32_t* counts, int B, int max_det, const ym_ragged_image* frames,
                              const ym_ragged_image* mask_blocks, const uint8_t* palette, int palette_n, int num_classes,
                              const char* names, int num_names, const uint16_t* font, int flags, float visual_thre,
                              const char* fps_text, uint8_t* out, void* workspace, size_t workspace_bytes, ym_stream_t s);
int ym_draw_detections_ragged_packed(const uint8_t* img, const uint64_t* mask_bits, const int64_t* ids, const float* scores,
                                     const int32_t* boxes_px, const int32_t* counts, int B, int max_det,
                                     const ym_ragged_image* frames, const ym_ragged_image* mask_blocks, const uint8_t* palette,
                                     int palette_n, int num_classes, const char* names, int num_names, const uint16_t* font,
                                     int flags, float visual_thre, const char* fps_text, uint8_t* out, void* workspace,
                                     size_t workspace_bytes, ym_stream_t s);

/* ym_mask_iou on bit rows: bits_a [n][words], bits_b [g][words], words = H * Wq < 2^18.  Exact integers through the same
 * finalize step, so bit-identical to ym_mask_iou on the dense masks (0/0 -> NaN). */
size_t ym_mask_iou_packed_workspace_bytes(int n, int g, int64_t words);
int ym_mask_iou_packed(const uint64_t* bits_a, int n, const uint64_t* bits_b, int g, int64_t words, float* iou, void* workspace,
                       size_t workspace_bytes, ym_stream_t s);
/* ym_rle_encode from bits [n][H][Wq]: same outputs, same "buffers too small" protocol. */
int ym_rle_encode_packed(const uint64_t* bits, int n, int H, int W, uint32_t* counts, int cap_runs, int32_t* nruns, uint8_t* str,
                         int cap_str, int32_t* str_len, void* workspace, size_t workspace_bytes, ym_stream_t s);
/* ym_rle_encode_ragged_packed: the detection dump of a whole request (eval.py:59-67, the rows MakeJson.add_bbox / add_mask receive)
 * for B <= YM_RAGGED_MAX_IMAGES images of different sizes in at most THREE launches (encode, scan, gather), without a host read.
 * ids / scores [B][max_det], boxes_px [B][max_det][4], counts [B] and det_bits + det_blocks are what ym_after_nms_ragged_packed left
 * (the uniform entry's [B][max_det][H][Wq] is the table {H, W, b * max_det * H * Wq}); a reader of whole words needs the blocks
 * 8-byte aligned only: det_bits 8-byte aligned, offsets in words, blocks not overlapping.  `live` is a HOST array of B flags, 0 =
 * the image is padding; it travels by value with the table.
 *   Row r of image b is a record iff live[b], r < counts[b] (read on the device) and (box[3] - box[1]) * (box[2] - box[0]) > 0 in
 * 64-bit integers (eval.py:65).  Every row gets its records[b * max_det + r]; a row that is no record gets all zeros (state 0) and
 * its mask words are never read.  A record carries the row's class, score and box and the string ym_rle_encode_packed writes for its
 * mask: the strings of the state-1 rows lie back to back in `strings` in (image, row) order, str_off = the exclusive sum of the
 * str_len before it (integer sums in a fixed order: the layout is a function of the lengths alone), header = {total string bytes,
 * records, records of state 2, 0}.  Each mask is encoded into a slab of 4 * cap_runs bytes of the workspace first; a mask of more
 * than cap_runs runs or a string longer than its slab gets state 2, str_len 0 and the runs it needs in nruns (encode it again with
 * larger buffers).  Nothing is written past strings_bytes or past a slab.
 *   Workspace: ym_rle_encode_ragged_workspace_bytes = B * max_det * cap_runs * 4 bytes of transition positions + B * max_det slabs of
 * 4 * cap_runs bytes, in that order (0 for arguments the entry would refuse).  `strings` holds at least the worst case
 * B * max_det * 4 * cap_runs bytes.  YM_ENOSPC when either is short.  YM_EINVAL, before any launch, for B outside
 * 1..YM_RAGGED_MAX_IMAGES, max_det < 1, cap_runs < 1, a width above 4096 or img_h * img_w >= 2^31, blocks that are misaligned or
 * overlap, B * max_det * 4 * cap_runs >= 2^31, null pointers. */
typedef struct ym_rle_record {   /* one detection row of a request, 40 bytes */
    int32_t class_id;            /* ids[b][r] */
    float   score;
    int32_t box[4];              /* boxes_px[b][r] */
    int32_t str_off, str_len;    /* its string in the request's compact buffer */
    int32_t nruns;               /* runs of the mask (also when state == 2) */
    int32_t state;               /* 0 no record, 1 encoded, 2 buffers too small */
} ym_rle_record;
size_t ym_sizeof_rle_record(void);
size_t ym_rle_encode_ragged_workspace_bytes(const ym_ragged_image* det_blocks, int B, int max_det, int cap_runs);
int ym_rle_encode_ragged_packed(const int64_t* ids, const float* scores, const int32_t* boxes_px, const int32_t* counts, int B, int max_det,
                                const uint64_t* det_bits, const ym_ragged_image* det_blocks, const uint8_t* live, int cap_runs,
                                ym_rle_record* records, uint8_t* strings, int64_t strings_bytes, int32_t* header, void* workspace,
                                size_t workspace_bytes, ym_stream_t s);
/* ym_draw_detections_batch / ym_draw_cutout_objects with the mask term read from bits [B][max_det][H][Wq] / [n][H][Wq]: output
 * bytes identical to the dense calls. */
int ym_draw_detections_batch_packed(const uint8_t* img, const uint64_t* mask_bits, const int64_t* ids, const float* scores,
                                    const int32_t* boxes_px, const int32_t* counts, int B, int max_det, int H, int W,
                                    const uint8_t* palette, int palette_n, int num_classes, const char* names, int num_names,
                                    const uint16_t* font, int flags, float visual_thre, const char* fps_text, uint8_t* out,
                                    uint8_t* cutout_total, void* workspace, size_t workspace_bytes, ym_stream_t s);
int ym_draw_cutout_objects_packed(const uint8_t* img, const uint64_t* mask_bits, int n, int H, int W, uint8_t* out, ym_stream_t s);

/* ---- device-resident mAP accumulator (utils/common_utils.py:107-262, eval.py:35-69,106) ---------------------------------------
 * The log: one row per (image slot, detection row) at position image_index * max_det + row, kept as three arrays:
 *   log_score fp32, log_class int32 (-1 = no data point), log_flags uint32 (bit type * T + k set = prediction matched at
 *   threshold k of IoU type `type`, 0 = box, 1 = mask; T <= YM_EVAL_MAX_THRESHOLDS),
 * plus gt_count int64 [num_classes] (ground-truth instances per class) and class_rows int32 [num_classes] (data points per class).
 * The caller initialises log_class to -1 and the two counters to 0; nothing here reads the host.
 *
 * ym_eval_match_log: prep_metrics (utils/common_utils.py:174-216) for ONE image on its padded after_nms_batch(sync=False) rows.
 *   ids int64 [n], scores fp32 [n], count int32 on the device (NULL = all n rows valid; clamped to 0..n), n <= YM_EVAL_MAX_DET;
 *   iou_box / iou_mask fp32 [n][g]; gt fp32 [g][5] whose column 4 is the class (float -> int by truncation); g <= 512 (g = 0 is
 *   allowed: nothing matches); thresholds fp64 [T] on the device.
 * The matching is ym_match_detections' (one device function): predictions in row order, rows below the count only, IoU strictly
 * greater than the fp64 threshold, the first gt wins among equal IoUs, a gt is used once per (type, threshold).  Rows at or past
 * the count, and rows whose class is outside 0..num_classes-1, are written with class -1, score 0 and no flags.  The image's gt
 * instances are added to gt_count and its data points to class_rows with INTEGER atomics.  An image whose count is 0 writes no data
 * point and adds no gt positives (eval.py:53-54 skips it before prep_metrics).  The image's rows are log_*[log_offset .. log_offset + n).
 *
 * ym_eval_ap: the AP of every (type, threshold, class) cell, APDataObject.get_ap operation for operation in fp64 (no contraction):
 *   log_flags uint32 [rows]; order int64 [rows] = log positions sorted by (class ascending, score descending, position ascending),
 *   NULL when log_flags already is in that order; seg int64 [num_classes + 1] = first sorted row of each class (rows of class -1
 *   sort first: seg[0] is their number); gt_count int64 [num_classes].
 *   ap fp64 [2][T][num_classes]: tp = running count of set flags, precision = tp / (rank + 1), recall = tp / num_gt, envelope =
 *   suffix maximum of precision; for each of the 101 grid values (double)k / 100.0 the envelope at the first rank whose recall
 *   quotient is >= the grid value (0 when it never is); the 101 samples are added left to right and divided by 101.  A cell with
 *   num_gt == 0 or without rows is 0.  empty uint8 [num_classes] = 1 when the class has no rows and num_gt == 0.
 * A class is walked in passes of YM_EVAL_AP_ROWS_PER_PASS rows with carried state (true positives still ahead, envelope so far), so
 * its length is unbounded.  workspace >= ym_eval_ap_workspace_bytes(rows) (the flags in sorted order: O(rows)).  No floating-point
 * atomics: results repeat bit for bit. */
#define YM_EVAL_MAX_DET 1024
#define YM_EVAL_MAX_THRESHOLDS 16
#define YM_EVAL_AP_ROWS_PER_PASS 1024
int ym_eval_match_log(const int64_t* ids, const float* scores, const int32_t* count, int n, const float* iou_box,
                      const float* iou_mask, const float* gt, int g, const double* thresholds, int T, int num_classes,
                      float* log_score, int32_t* log_class, uint32_t* log_flags, int64_t log_offset, int64_t* gt_count,
                      int32_t* class_rows, ym_stream_t s);
size_t ym_eval_ap_workspace_bytes(int64_t rows);
int ym_eval_ap(const uint32_t* log_flags, const int64_t* order, int64_t rows, const int64_t* seg, const int64_t* gt_count, int T,
               int num_classes, double* ap, uint8_t* empty, void* workspace, size_t workspace_bytes, ym_stream_t s);
/* ym_eval_add_ragged_packed: the metric stage of a whole request -- ym_mask_iou_packed + ym_box_iou + ym_eval_match_log for B <=
 * YM_RAGGED_MAX_IMAGES images of different sizes in at most THREE launches; the log, gt_count and class_rows end up exactly as after
 * B single-image calls.
 *   ids int64 / scores fp32 [B][max_det], boxes_px int32 [B][max_det][4], counts int32 [B] on the device (clamped to 0..max_det);
 *   det_bits + det_blocks: the packed masks and the table that ym_after_nms_ragged_packed was given;
 *   gt fp32 [gt_first[B]][5] = x1 y1 x2 y2 in 0..1 and the class, NOT modified: the boxes are scaled in the kernel, x * (float)img_w_b
 *   and y * (float)img_h_b with one rounding each (what an in-place fp32 scaling of the tensor leaves);
 *   gt_first: HOST int32 [B + 1], ascending: image b owns rows gt_first[b] .. gt_first[b + 1], g_b of them, 0 <= g_b <= 512;
 *   gt_bits + gt_blocks: block b = [g_b][img_h_b][ceil(img_w_b / 64)] words, sizes equal to det_blocks';
 *   image_index: HOST int64 [B], image b's rows are log_*[image_index[b] * max_det ..); < 0 = the entry is padding: nothing of it is
 *   read, written or counted; log_rows = rows of the three log arrays.
 * The tables are read during the call and travel to the kernels by value: no device copy, no synchronisation, no host read.
 *   launch 1 (skipped when no image has ground truth): one workgroup per (20-word chunk of an image's mask rows, group of 128 gt rows),
 *     grid.x = sum of ceil(words_b / 20) over the images that are not padding and have g_b > 0; a workgroup finds its image from the
 *     prefix of that sum, loads only the detection rows below counts[b], in passes of 128, and writes its own exact integer partials;
 *   launch 2: per pair (row below the count, gt) the mask IoU from the summed partials -- ym_mask_iou_packed's finalize step -- and
 *     the box IoU -- ym_box_iou's formula on (float)boxes_px and the scaled gt box;
 *   launch 3: workgroup b is ym_eval_match_log's workgroup for image b (one device function: same matching, same log writes, same
 *     integer atomics; an image whose count is 0 adds no data point and no gt positives, g_b = 0 logs the rows without flags).
 * No floating-point atomics.  YM_EINVAL, before any launch, for B outside 1..YM_RAGGED_MAX_IMAGES, max_det outside
 * 1..YM_EVAL_MAX_DET, T outside 1..YM_EVAL_MAX_THRESHOLDS, g_b > 512 or a descending gt_first, table entries that differ in size,
 * lie at no multiple of YM_RAGGED_ALIGN_BYTES or overlap, img_h_b * ceil(img_w_b / 64) >= 2^18, (image_index[b] + 1) * max_det >
 * log_rows, two equal indices >= 0, null pointers; YM_ENOSPC for workspace_bytes < ym_eval_add_ragged_workspace_bytes(...) (the
 * partials and the IoUs of every image; a host function of the sizes; 0 for arguments the entry refuses). */
size_t ym_eval_add_ragged_workspace_bytes(const ym_ragged_image* det_blocks, const int32_t* gt_first, int B, int max_det);
int ym_eval_add_ragged_packed(const int64_t* ids, const float* scores, const int32_t* boxes_px, const int32_t* counts, int B, int max_det,
                              const uint64_t* det_bits, const ym_ragged_image* det_blocks, const float* gt, const int32_t* gt_first,
                              const uint64_t* gt_bits, const ym_ragged_image* gt_blocks, const int64_t* image_index,
                              const double* thresholds, int T, int num_classes, float* log_score, int32_t* log_class,
                              uint32_t* log_flags, int64_t log_rows, int64_t* gt_count, int32_t* class_rows, void* workspace,
                              size_t workspace_bytes, ym_stream_t s);

/* ---- device-resident COCO evaluator (eval.py:90-104: pycocotools COCOeval on the dumped detections) --------------------------
 * The protocol is the published cocoapi's (cocoeval.py evaluate / computeIoU / evaluateImg / accumulate, maskApi.c bbIou / rleIou)
 * with its default parameters, which the caller passes as device arrays (iouThrs, recThrs, areaRng, maxDets, eps = spacing(1)).
 * All IoUs and quotients are fp64 without contraction; every sum is an integer count; integer atomics only; nothing reads the host.
 *
 * ym_coco_iou_box: bbIou.  dt_xywh fp64 [n][4], gt_xywh fp64 [g][4] ([x, y, w, h]), iscrowd uint8 [g] -> iou fp64 [n][g]:
 *   w = min(dx+dw, gx+gw) - max(dx, gx), h likewise; w <= 0 or h <= 0 -> 0; i = w*h; u = crowd ? da : da + ga - i; i / u.
 * ym_coco_iou_mask_packed: rleIou on bit rows ("bit-packed instance masks": bits_d [n][words], bits_g [g][words], words = H * Wq):
 *   i = |d & g|; i == 0 -> 0; else i / (crowd ? |d| : |d| + |g| - i).  area_d int32 [n] = |d| (the detection's segm area).
 *
 * The log: one row per (image slot, detection row) at position image_index * max_det + row: log_score fp32, log_class int32 (-1 =
 * no data point), log_rank int32 (the row's rank among the image's rows of its class: score descending, equal scores in row order),
 * log_flags uint32 [YM_COCO_WORDS_PER_ROW] = one word per (IoU type, area range), word type * YM_COCO_AREAS + a: bit k = matched at
 * threshold k, bit 16 + k = ignored at threshold k.  npig int64 [YM_COCO_AREAS][num_classes] (non-ignored gts), class_rows int32
 * [num_classes] (data points per class).  The caller initialises log_class to -1 and the counters to 0.
 *
 * ym_coco_match_log: computeIoU's ordering and evaluateImg for ONE image, every category, area range, threshold and IoU type.
 *   ids int64 [n], scores fp32 [n], count int32 on the device (NULL = n), n <= YM_EVAL_MAX_DET (n = 0: only the gts are counted);
 *   boxes_px int32 [n][4] or NULL: rows whose pixel box has (x2-x1)*(y2-y1) <= 0 are no detections (eval.py:65);
 *   iou_box / iou_mask fp64 [n][g] and area_box fp64 [n] / area_mask int32 [n] (the detection's area per IoU type); an IoU type whose
 *   area pointer is NULL is not evaluated; gt_class int32 [g], gt_iscrowd uint8 [g], gt_area fp64 [g], g <= YM_COCO_MAX_GT;
 *   thresholds fp64 [T], T <= YM_EVAL_MAX_THRESHOLDS; area_rng fp64 [YM_COCO_AREAS][2]; max_rank = maxDets[-1].
 *   A gt is ignored when iscrowd or area < lo or area > hi; the gts of a category are walked non-ignored first (stable).  Per
 *   detection in rank order: best = min(t, 1 - 1e-10), m = none; skip a gt already matched at this threshold unless it is a crowd;
 *   STOP when m is a non-ignored gt and the current gt is ignored; skip if iou < best; else take it (among equal IoUs the later
 *   gt wins).  A matched detection inherits its gt's ignore flag; an unmatched one whose own area is outside the range is ignored.
 *   Rows of rank >= max_rank, rows at or past the count and rows of a class outside 0..num_classes-1 are written with class -1.
 *
 * ym_coco_accumulate: accumulate.  order int64 [rows] = log positions by (class ascending, score descending, position ascending), seg
 *   int64 [num_classes + 1] as for ym_eval_ap; rec_thrs fp64 [R], max_dets int32 [M] on the device; kinds: bit 0 = bbox, bit 1 = segm.
 *   precision fp64 [2][T][R][num_classes][YM_COCO_AREAS][M] and recall fp64 [2][T][num_classes][YM_COCO_AREAS][M], which the caller
 *   initialises to -1; a cell with npig == 0 keeps it.  Otherwise, over the category's rows of rank < maxDet: tp / fp = running
 *   counts of matched / unmatched non-ignored rows, rc = tp / npig, pr = tp / ((fp + tp) + eps), recall = rc[-1] (0 without rows),
 *   envelope from the back, precision[r] = pr at the first row with rc >= rec_thrs[r] (0 when there is none).  A category is walked
 *   in passes of YM_COCO_ROWS_PER_PASS rows with carried state, so its length is unbounded.
 *   workspace >= ym_coco_accumulate_workspace_bytes(rows) (flag words and ranks in sorted order). */
#define YM_COCO_MAX_GT 512
#define YM_COCO_AREAS 4
#define YM_COCO_WORDS_PER_ROW 8
#define YM_COCO_ROWS_PER_PASS 1024
int ym_coco_iou_box(const double* dt_xywh, int n, const double* gt_xywh, int g, const uint8_t* iscrowd, double* iou, ym_stream_t s);
int ym_coco_iou_mask_packed(const uint64_t* bits_d, int n, const uint64_t* bits_g, int g, int64_t words, const uint8_t* iscrowd,
                            double* iou, int32_t* area_d, ym_stream_t s);
int ym_coco_match_log(const int64_t* ids, const float* scores, const int32_t* count, int n, const int32_t* boxes_px,
                      const double* iou_box, const double* iou_mask, const double* area_box, const int32_t* area_mask,
                      const int32_t* gt_class, const uint8_t* gt_iscrowd, const double* gt_area, int g,
                      const double* thresholds, int T, const double* area_rng, int num_classes, int max_rank,
                      float* log_score, int32_t* log_class, int32_t* log_rank, uint32_t* log_flags, int64_t log_offset,
                      int64_t* npig, int32_t* class_rows, ym_stream_t s);
size_t ym_coco_accumulate_workspace_bytes(int64_t rows);
int ym_coco_accumulate(const uint32_t* log_flags, const int32_t* log_rank, const int64_t* order, int64_t rows, const int64_t* seg,
                       const int64_t* npig, const double* rec_thrs, int R, const int32_t* max_dets, int M, int T,
                       int num_classes, double eps, int kinds, double* precision, double* recall, void* workspace,
                       size_t workspace_bytes, ym_stream_t s);
/* ym_eval_coco_add_ragged_packed: evaluateImg for a whole request -- ym_coco_iou_box + ym_coco_iou_mask_packed + ym_coco_match_log
 * for B <= YM_RAGGED_MAX_IMAGES images of different sizes in at most THREE launches; log_score, log_class, log_rank, log_flags, npig
 * and class_rows end up exactly as after B single-image calls.
 *   ids int64 / scores fp32 [B][max_det], boxes_px int32 [B][max_det][4], counts int32 [B] on the device (clamped to 0..max_det);
 *   det_bits + det_blocks: the packed masks and the table that ym_after_nms_ragged_packed was given;
 *   gt_class int32 [G], gt_iscrowd uint8 [G], gt_area fp64 [G], gt_xywh fp64 [G][4] on the device, G = gt_first[B];
 *   gt_first: HOST int32 [B + 1], ascending: image b owns the gts gt_first[b] .. gt_first[b + 1], g_b of them, 0 <= g_b <= YM_COCO_MAX_GT;
 *   gt_bits + gt_blocks: block b = [g_b][img_h_b][ceil(img_w_b / 64)] words, sizes equal to det_blocks';
 *   image_index: HOST int64 [B], image b's rows are log_*[image_index[b] * max_det ..); < 0 = the entry is padding: nothing of it is
 *   read, written or counted; log_rows = rows of the log arrays (log_flags has YM_COCO_WORDS_PER_ROW words per row);
 *   thresholds, T, area_rng, num_classes, max_rank: as for ym_coco_match_log;
 *   kinds: bit 0 = bbox, bit 1 = segm.  An IoU type that is off is not evaluated and needs none of its inputs: without bbox gt_xywh
 *   may be NULL (and boxes_px, then every row below its count is a detection); without segm det_bits, det_blocks, gt_bits and
 *   gt_blocks may be NULL.
 * The tables are read during the call and travel to the kernels by value: no device copy, no synchronisation, no host read.
 *   launch 1 (segm only): one workgroup per (20-word chunk of an image's mask rows, group of 128 gt rows), grid.x = sum of
 *     ceil(words_b / 20) over the images that are not padding -- ALSO those with g_b = 0: an unmatched detection whose own area is
 *     outside the range is ignored, so its popcount is needed without any gt; a workgroup finds its image from the prefix of that
 *     sum, loads only the detection rows below counts[b], in passes of 128, and writes its own exact integer partials (the pair
 *     loop of ym_mask_iou_packed);
 *   launch 2, fp64 without contraction: per row below the count area_mask = the sum of its partials and area_box = w * h; per pair
 *     (row below the count, gt) the mask IoU of ym_coco_iou_mask_packed from the summed partials and the box IoU by
 *     ym_coco_iou_box's formula on (x1, y1, x2 - x1, y2 - y1) of boxes_px (exact in fp64);
 *   launch 3: workgroup b is ym_coco_match_log's workgroup for image b (one device function: same ordering, same matching, same log
 *     writes, same integer atomics; an image whose count is 0 only counts its gts).
 * Integer atomics only.  YM_EINVAL, before any launch, for B outside 1..YM_RAGGED_MAX_IMAGES, max_det outside 1..YM_EVAL_MAX_DET, T
 * outside 1..YM_EVAL_MAX_THRESHOLDS, kinds outside 1..3, g_b > YM_COCO_MAX_GT or a descending gt_first, table entries that differ in
 * size, lie at no multiple of YM_RAGGED_ALIGN_BYTES or overlap, img_h_b * ceil(img_w_b / 64) >= 2^24, (image_index[b] + 1) * max_det >
 * log_rows, two equal indices >= 0, null pointers of an enabled kind; YM_ENOSPC for workspace_bytes <
 * ym_eval_coco_add_ragged_workspace_bytes(...) (the IoUs, areas and partials of every image; a host function of the sizes; det_blocks
 * may be NULL without segm; 0 for arguments the entry refuses). */
size_t ym_eval_coco_add_ragged_workspace_bytes(const ym_ragged_image* det_blocks, const int32_t* gt_first, int B, int max_det, int kinds);
int ym_eval_coco_add_ragged_packed(const int64_t* ids, const float* scores, const int32_t* boxes_px, const int32_t* counts, int B,
                                   int max_det, const uint64_t* det_bits, const ym_ragged_image* det_blocks, const int32_t* gt_class,
                                   const uint8_t* gt_iscrowd, const double* gt_area, const double* gt_xywh, const int32_t* gt_first,
                                   const uint64_t* gt_bits, const ym_ragged_image* gt_blocks, const int64_t* image_index,
                                   const double* thresholds, int T, const double* area_rng, int num_classes, int max_rank, int kinds,
                                   float* log_score, int32_t* log_class, int32_t* log_rank, uint32_t* log_flags, int64_t log_rows,
                                   int64_t* npig, int32_t* class_rows, void* workspace, size_t workspace_bytes, ym_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* YOLACT_HIP_H */
