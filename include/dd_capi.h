/*
 * dd_capi.h — C-ABI of libdd.so, the MI355X (gfx950) Data Diet scoring/pruning kernels.
 *
 * Boundary: the reference has no FFI; its scoring path is the Python function
 *   sparse_loader(train_loader, train_samples, net, device, sparsity, batch_size, num_workers)
 *   (reference get_scores_and_prune.py:8-34).
 * Each entry point below replaces one step of that function (or one step the north star adds
 * to it); the file:line it replaces is cited on each declaration.  The Python host side
 * (data_diet_distributed_amd/get_scores_and_prune.py) keeps the reference signature and calls
 * these through ctypes (binding: INTEGRATION.md).
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer owned by the caller (torch tensors on the host side);
 *     no entry point allocates device memory: scratch comes from a caller workspace whose size
 *     is returned by the matching *_workspace_bytes query;
 *   - `stream` is a hipStream_t passed as void*; work is enqueued on it, nothing synchronises
 *     (entry points are graph-capturable);
 *   - return 0 on success, a negative DD_E* code on error; dd_last_error() returns a
 *     thread-local message for the last failing call on this thread;
 *   - stateless and reentrant; one process per GPU.
 */
#ifndef DD_CAPI_H
#define DD_CAPI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DD_OK 0
#define DD_EINVAL (-1)   /* bad argument (null pointer, negative size, unsupported shape) */
#define DD_ELAUNCH (-2)  /* HIP launch / runtime error */
#define DD_EWORKSPACE (-3) /* workspace too small */

/* ABI version, bumped on any signature change. */
int dd_abi_version(void);

/* Operand halves of the split MFMA convolutions (pack and forward must agree):
 *   DD_OPERANDS_BF16X3: v = hi + lo in bf16, products hi*hi + hi*lo + lo*hi with fp32
 *     accumulation (~2^-17 relative per product); any fp32 range.  The GraNd passes.
 *   DD_OPERANDS_F16X3: the same in fp16 (~2^-22 relative per product, at the same MFMA
 *     rate); operands must stay below 65504 in magnitude (values below 6.1e-5 carry an
 *     absolute error of at most 2^-25).  The EL2N forward (batch-normalised activations, raw
 *     weights): its ResNet-50 scores stay within the north star's 1e-3 of fp32.
 *     fp16 packs / launches exist for the statistics epilogue (every staging mode) and the
 *     generic run-time epilogue.
 * Weight scale: a pack holds W * scale and its forward multiplies the accumulators by
 * acc_scale = 1 / scale, both powers of two, so the product is exact.  bf16: scale 1.  fp16:
 * the host picks scale = 2^(13 - ceil(log2 max|W|)) so the weights' lo halves stay clear of
 * fp16's subnormal range (a small weight's lo half would otherwise carry ~2^-25 absolute
 * error: the ResNet GraNd forward's worst rows, tools/emulate_split_grand.py). */
#define DD_OPERANDS_BF16X3 0
#define DD_OPERANDS_F16X3 1

/* Message for the last non-zero return on the calling thread ("" if none). */
const char* dd_last_error(void);

/* ---------------------------------------------------------------------------------------- *
 * Input feed (reference data/loader.py:8-11 transform, applied per image in
 * MyDataset.__getitem__ :19-23 by the DataLoader workers of get_scores_and_prune.py:11):
 *   out[i, c, p] = (img[i, c, p] / 255 - mean[c]) / std[c]      (ToTensor + Normalize)
 * img: uint8 [n, C, HW] (CHW per image); out: fp32 [n, C, HW].  mean/std: host values.
 * ---------------------------------------------------------------------------------------- */
int dd_normalize_u8(const uint8_t* img, int64_t n, int32_t channels, int64_t hw,
                    const float* mean_host, const float* std_host, float* out, void* stream);

/* Same, gathering images by index: out[j] = normalize(img[index[j]]), j < n. */
int dd_normalize_u8_gather(const uint8_t* img, const int64_t* index, int64_t n,
                           int32_t channels, int64_t hw, const float* mean_host,
                           const float* std_host, float* out, void* stream);

/* Synthetic training set generated in HBM (replaces the dataset source of reference
 * data/loader.py:27-33 — torchvision CIFAR10(download=True) — for offline and ImageNet-shape
 * runs, BASELINE config 5).  Writes examples idx0 .. idx0+n-1 of the set named by `seed`:
 * img uint8 [n, C, h, w] and labels int64 [n] (labels may be NULL).  Every byte is a pure
 * function of (seed, global index, c, y, x), so shards generated on different ranks agree
 * with one whole-set generation; the hash is defined in dd_synth.hip and restated by
 * oracle/synth.py. */
int dd_synth_images_u8(uint64_t seed, int64_t idx0, int64_t n, int32_t channels, int32_t h,
                       int32_t w, int32_t num_classes, uint8_t* img, int64_t* labels,
                       void* stream);

/* ---------------------------------------------------------------------------------------- *
 * EL2N (reference get_scores_and_prune.py:16-18):
 *   p = softmax(logits[b, :]); e = p - onehot(label[b]); score[b] = ||e||_2
 * logits fp32 [B, C] row-major, labels int64 [B] in [0, C).
 * Outputs (each may be NULL):
 *   score[B]   : the EL2N score of each row (replaces the per-example .item() loop :19-20)
 *   e[B, C]    : the residual rows = d(sum CE)/d(logits), the GraNd backward seed; the
 *                label entry is written as -sum_{j != y} p_j (no p_y - 1 cancellation)
 *   accum[B]   : accum[b] += score[b]  (K-checkpoint ensemble running sum)
 *   bad_labels int32 [1] (device): += the number of rows whose label lies outside [0, C).
 * A label outside [0, C) is where the reference's one_hot(target, num_classes) raises (:17,
 * RuntimeError).  The kernel cannot raise, so such a row's score, accum term and e row are
 * NaN and the row is counted in bad_labels (one integer atomic add per bad row); the caller
 * reads the count back and raises (the engine does so once per job, after the score
 * all-gather, so every rank raises together).  ABI 9.
 * ---------------------------------------------------------------------------------------- */
int dd_el2n(const float* logits, const int64_t* labels, int64_t B, int32_t C,
            float* score, float* e, float* accum, int32_t* bad_labels, void* stream);

/* ---------------------------------------------------------------------------------------- *
 * The other logit scores of the same forward (absent from the reference, which keeps EL2N
 * only): one launch, one read of the logits, any subset.  Purely additive: no existing
 * signature or result changes, so dd_abi_version() stays 10.
 *
 * Per row: logits z[0..C), label y, m = max_j z_j, e_j = exp(z_j - m), s = sum_j e_j.  Every
 * statistic is oriented so that larger means harder:
 *   loss        (m - z_y) + log s             cross-entropy as log-sum-exp, never -log(p_y)
 *   margin      max_{j != y} z_j - z_y        one fp32 subtraction (the quantity behind AUM)
 *   entropy     log s - (sum_j e_j (z_j - m)) / s     a term with e_j == 0 contributes 0
 *   error       1.0 if max_{j != y} z_j >= z_y else 0.0   (a tie with the label is an error)
 *   wrong_mass  (sum_{j != y} e_j) / s        1 - p_y without the cancellation (as dd_el2n's
 *                                             e_y); one minus the Cartography confidence
 * logits fp32 [B, C] row-major, labels int64 [B].  Outputs, each fp32 [B] and each may be NULL
 * (a statistic that is not asked for costs no store):
 *   loss_accum, margin_accum, entropy_accum, error_accum, wrong_mass_accum:
 *       accum[b] += the row's statistic (the K-checkpoint running sum; dd_ensemble_finalize
 *       makes the mean);
 *   var_mean, var_m2 (both or neither) with the 1-based checkpoint ordinal k: Welford's update
 *       of w = wrong_mass over the checkpoints, in checkpoint order 1..K,
 *           mean_k = mean_{k-1} + (w - mean_{k-1}) / k,   M2 += (w - mean_{k-1}) (w - mean_k)
 *       (k == 1 writes mean = w, M2 = 0 without reading the buffers);
 *       dd_variability_finalize then gives the population standard deviation
 *       out[i] = sqrt(max(M2[i], 0) / K) (NaN stays NaN), Dataset Cartography's variability.
 *   bad_labels int32 [1] (device): += the number of rows whose label lies outside [0, C).
 * NaN rules: a row with a label outside [0, C) (dd_el2n's rule: counted once, one integer
 * atomic add), or with a NaN or +inf logit, gives NaN in every requested statistic and
 * accumulator term (-inf logits are unspecified).
 * margin / error need C >= 2.  B == 0 returns DD_OK; nothing requested, C < 1, B < 0, NULL
 * logits / labels with B > 0, one pointer of the Welford pair without the other, or the pair
 * with k < 1 are DD_EINVAL before any launch.
 * A row's results depend on that row alone and are reduced in an order fixed by C (no float
 * atomics): bitwise independent of B, of the row's position and of the buffers' alignment.
 * No synchronisation inside (graph-capturable).
 * ---------------------------------------------------------------------------------------- */
int dd_logit_scores(const float* logits, const int64_t* labels, int64_t B, int32_t C,
                    float* loss_accum, float* margin_accum, float* entropy_accum,
                    float* error_accum, float* wrong_mass_accum, float* var_mean, float* var_m2,
                    int32_t k, int32_t* bad_labels, void* stream);
int dd_variability_finalize(const float* m2, int64_t n, int32_t K, float* out, void* stream);

/* ---------------------------------------------------------------------------------------- *
 * GraNd per-example gradient norms (north star (b); absent from the reference, which scores
 * with EL2N only — get_scores_and_prune.py:15-18; layers hooked: models/resnet.py:12-18,
 * 22-23, 40-47, 52-53, 71, 78).
 *
 * For a Conv2d with weight [Cout, Cin, kh, kw] (no bias, groups = 1), input activation
 * act fp32 NCHW [B, Cin, H, W] and output gradient gout fp32 NCHW [B, Cout, Ho, Wo]:
 *   sq_accum[b] += sum_{o, m} ( col_scale[o] * sum_t U_b[t, m] * gout[b, o, t] )^2
 * where U_b is the im2col of act[b] (t = output position, m = (c, ky, kx)).  col_scale may be
 * NULL (= 1); it carries a folded BatchNorm's gamma / sqrt(var + eps) when the forward ran
 * with BN folded into the conv.
 *   method DD_PEGRAD_DIRECT: per example G_b = U_b^T gout_b on MFMA, squared and summed in
 *     registers (2 T d_a d_g flop);
 *   method DD_PEGRAD_GHOST : sum_{t,t'} (U U^T)_{tt'} (gout gout^T)_{tt'} — the ghost-norm
 *     identity, both T x T Grams on MFMA (2 T^2 (d_a + d_g) flop);
 *   method DD_PEGRAD_AUTO  : the cheaper of the two for this geometry.
 * The result is deterministic (no float atomics): partial sums go to the workspace and are
 * reduced in a fixed order.
 * ---------------------------------------------------------------------------------------- */
#define DD_PEGRAD_AUTO 0
#define DD_PEGRAD_DIRECT 1
#define DD_PEGRAD_GHOST 2
#define DD_PEGRAD_DIRECT3X3 3 /* reported by dd_conv_pegrad_method only: the all-taps kernel */
#define DD_PEGRAD_PGRAM 4     /* reported only: ghost by shifted input-position Grams, for maps of
                                 <= 64 positions at DD_PREC_BF16X3: K_a = sum_tap P[p(t,tap)][p(t',tap)]
                                 with P = a^T a, so 2 (Ti^2 cin + To^2 cout) flop per example */
#define DD_PEGRAD_STEM 5      /* reported only: direct over the <= 32 im2col rows of an input conv
                                 with cin * 9 <= 32 (the network's first conv, 3 channels) at
                                 DD_PREC_BF16X3; bound by reading gout once */
#define DD_PEGRAD_DIRECT1X1 6 /* reported only: direct for a 1x1 conv (pad 0, stride 1 or 2) at
                                 DD_PREC_BF16X3: G = U^T g as a split-bf16 GEMM over positions */
#define DD_PEGRAD_PGRAM_Q 7   /* reported only: the shifted-Gram ghost for a 3x3 / pad 1 /
                                 stride 1 conv on a 16 x 16 map (T = 256, ResNet-18 layer2) at
                                 DD_PREC_BF16X3, tiled by quarters of the output positions (P
                                 does not fit LDS whole): 2 (Ti^2 cin + To^2 cout) flop per
                                 example; chosen by GHOST (AUTO keeps DIRECT3X3, measured faster
                                 on this shape: DESIGN.md §4.2) */

/* precision of the norm kernels:
 *   DD_PREC_FP32   exact fp32 MFMA (v_mfma_f32_32x32x2_f32 / 16x16x4_f32) everywhere;
 *   DD_PREC_BF16X3 split-bf16 MFMA where a kernel exists (3x3 stride-1 direct): each operand
 *                  v = hi + lo in bf16, products hi*hi + hi*lo + lo*hi accumulated in fp32
 *                  (~1e-5 relative per product; the GraNd tolerance is 1e-3). */
#define DD_PREC_FP32 0
#define DD_PREC_BF16X3 1

typedef struct dd_conv_geom {
  int64_t batch;   /* B */
  int32_t cin, h, w;      /* input  [B, cin, h, w] */
  int32_t cout, ho, wo;   /* output [B, cout, ho, wo] */
  int32_t kh, kw;         /* kernel */
  int32_t stride, pad;    /* symmetric stride / zero padding */
} dd_conv_geom;

/* Which kernel a (method, precision) request resolves to for this geometry:
 * DD_PEGRAD_DIRECT, DD_PEGRAD_GHOST, DD_PEGRAD_DIRECT3X3, DD_PEGRAD_PGRAM, DD_PEGRAD_STEM or
 * DD_PEGRAD_DIRECT1X1;
 * <0 on a bad argument. */
int dd_conv_pegrad_method(const dd_conv_geom* geom, int method, int precision);

size_t dd_conv_pegrad_workspace_bytes(const dd_conv_geom* geom, int method, int precision);

int dd_conv_pegrad_sqnorm(const float* act, const float* gout, const dd_conv_geom* geom,
                          const float* col_scale, int method, int precision, float* sq_accum,
                          void* workspace, size_t workspace_bytes, void* stream);

/* CIFAR head of the GraNd pass (reference models/resnet.py:94-96, avg_pool2d(out, 4) ->
 * linear), fp32 NCHW:
 *   dd_head_pool:     feat[b][c] = mean_p a[b][c][p]                          (a [B][C][hw])
 *   dd_head_backward: d[b][c][p] = scale * (sum_j e[b][j] W[j][c]) * (a[b][c][p] > 0)
 *     with e [B][ncls] the EL2N residual (the CE logit gradient), W [ncls][C] the classifier
 *     weight and scale = 1 / hw: the gradient w.r.t. the last block's pre-ReLU output, one
 *     pass over a (replaces e @ W, the broadcast divide and the ReLU mask as three torch ops). */
int dd_head_pool(const float* a, int64_t B, int32_t C, int32_t hw, float* feat, void* stream);
int dd_head_backward(const float* a, const float* e, const float* w, int64_t B, int32_t C,
                     int32_t hw, int32_t ncls, float scale, float* d, void* stream);

/* Classifier forward (reference models/resnet.py:96 `self.linear(out)`, nn.Linear :78):
 *   out[b][c] = sum_k feat[b][k] W[c][k] + (bias ? bias[c] : 0)
 * feat fp32 [B, d_in] (d_in <= 4096), W fp32 [d_out, d_in], bias fp32 [d_out] or NULL, out fp32
 * [B, d_out].  Each row is reduced in a fixed order from that row alone, so logits are
 * bitwise independent of B (chunk size, shard size, world size). */
int dd_linear_forward(const float* feat, const float* w, const float* bias, int64_t B,
                      int32_t d_in, int32_t d_out, float* out, void* stream);

/* Linear layer y = a W^T + bias (reference models/resnet.py:78, 96):
 *   sq_accum[b] += ||a_b||^2 * ||g_b||^2 + (has_bias ? ||g_b||^2 : 0)
 * act fp32 [B, d_in], gout fp32 [B, d_out] (for the classifier, gout = the EL2N residual e). */
int dd_linear_pegrad_sqnorm(const float* act, const float* gout, int64_t B, int32_t d_in,
                            int32_t d_out, int32_t has_bias, float* sq_accum, void* stream);

/* Eval-mode BatchNorm affine parameters (grand_params: all — the per-example gradient over
 * every parameter, as torch.func per-sample gradients define it; the BN layers are reference
 * models/resnet.py:13, 16, 24, 44, 46, 48, 53, 72).  With the BN output
 * out = gamma_c * xhat + beta_c and g = d loss / d out:
 *   sq_accum[b] += sum_c ( (sum_t g[b,c,t] * (v[b,c,t] - r[b,c,t] - beta_c)) / gamma_c )^2
 *                        + ( sum_t g[b,c,t] )^2
 * v fp32 [B, C, hw] must equal out + r wherever g != 0: the post-ReLU activation for a BN
 * followed by a ReLU (g vanishes where it clipped), or the block output with r = the
 * shortcut value for the last BN of a residual block (r may be NULL).  gamma_c != 0.
 * Deterministic (one fixed-order reduction per example). */
int dd_bn_pegrad_sqnorm(const float* v, const float* r, const float* g, int64_t B, int32_t C,
                        int64_t hw, const float* gamma, const float* beta, float* sq_accum,
                        void* stream);

/* ---------------------------------------------------------------------------------------- *
 * Backbone 3x3 / stride-1 / pad-1 convolution on split-bf16 MFMA (the ResNet convs of
 * reference models/resnet.py:12-15 (BasicBlock conv1 at stride 1, conv2) and :42-43
 * (Bottleneck conv2 at stride 1), i.e. 88% of ResNet-18 flops).  The reference runs them
 * through PyTorch (get_scores_and_prune.py:15); here they back the scoring passes.
 *   dd_conv3x3_pack: fp32 weights [cout][cin][3][3] -> bf16 hi/lo pack (device, caller-owned,
 *     dd_conv3x3_pack_bytes(out_ch, in_ch) bytes).  transpose_flip = 0 packs the forward conv
 *     (out_ch = cout, in_ch = cin); = 1 packs its backward-data conv (out_ch = cin,
 *     in_ch = cout, weights transposed and spatially flipped).  A forward pack with
 *     cin <= 5 (the input conv, reference models/resnet.py:71) uses the stem layout: the
 *     three kx taps of each channel become 3 cin pseudo-channels of the centre column, so
 *     the conv runs one K step per tap row; only dd_conv3x3_forward reads it.
 *   dd_conv3x3_forward: y[B][cout][h][w] = epi(conv(xf(x[B][cin][h][w]), packed)),
 *     xf(v)  = max(v * in_scale[g][c] + in_shift[g][c], in_relu ? 0 : -inf)   (input
 *              transform: the producer's train-mode BN + ReLU, reference models/resnet.py:28;
 *              identity when in_scale = in_shift = NULL), g = b / group_size;
 *     epi(v) = ((v + bias[o]) + residual) -> max(.,0) if relu -> 0 where !(mask_src > 0);
 *     bias / residual / mask_src may be NULL.  w in {8, 16, 32}; h a multiple of the
 *     row block (4 rows at w=32, 8 rows at w=16 and w=8), or 4x4.  fp32 accumulation;
 *     ~1e-5 relative vs fp32.
 *     stats (may be NULL): BN partial statistics of y over rows b < n_stat, laid out
 *     [G][cout][tiles_per_group][2] (sum, sum of squares) with G = ceil(B / group_size) and
 *     one partial per 32 consecutive positions of a group's examples (two images at 4x4):
 *     tiles_per_group = dd_conv3x3_tiles_per_group(h, w, group_size) = group_size*h*w/32;
 *     consumed by dd_bn_finalize with images_per_tile = max(1, 32 / (h*w)).  group_size
 *     must be even at 8x8 and a multiple of 4 at 4x4 when in_scale or stats is given.
 *     Padded-width launches (ABI 10): with the statistics epilogue alone (stats given; no
 *     bias, residual, masks or relu; cin > 5) the widths that are not a tile width also run
 *     here -- 32 < w <= 64 with w % 4 == 0 (any cout), and with cout padded to a multiple of
 *     128: 16 < w <= 32 with w % 4 == 0, 8 < w <= 16, and 4 < w <= 8 with h <= 8 and an even
 *     group_size; any h (the last row block may overhang): the ImageNet-stem network's
 *     56x56 / 28x28 / 14x14 / 7x7 maps (reference models/resnet.py:42-43).  The image is
 *     staged into the next tile width with zero columns / rows, which are never stored or
 *     counted; the partials keep the layout above on the padded grid: tiles_per_group =
 *     group_size * ceil(h / rb) * rb * wt / 32 ((rb, wt) = (2, 64), (4, 32), (8, 16),
 *     (8, 8)), images_per_tile 1.  DD_CONV_PW=0 turns them off.
 *   dd_conv3x3_tiles_per_group: partials per BN group of the stats layout (< 0 if
 *     unsupported).
 *   dd_conv3x3_padded_supported: 1 where a statistics launch of this shape takes the
 *     padded-width tiles (not a native shape; see above), else 0.
 *   mask_out / mask_in (may be NULL; dd_conv3x3_mask_bytes(B, cout, h, w) bytes): the ReLU
 *     mask (y > 0) in the kernel's fragment order, 1 bit per output.  A launch writing
 *     mask_out and a later launch of the same geometry (B, h, w, output channels) reading
 *     mask_in (in place of mask_src) see the same (example, channel, position) at the same
 *     bit, so the GraNd backward reads 1/32 of the bytes of the fp32 activation it masks by
 *     (reference BasicBlock ReLUs, models/resnet.py:28, 31).
 * ---------------------------------------------------------------------------------------- */
size_t dd_conv3x3_pack_bytes(int32_t out_channels, int32_t in_channels);
int dd_conv3x3_pack(const float* w, int32_t cout, int32_t cin, int32_t transpose_flip,
                    int32_t operands, float scale, void* packed, void* stream);
int dd_conv3x3_tiles_per_group(int32_t h, int32_t w, int32_t group_size);
int dd_conv3x3_padded_supported(int32_t h, int32_t w, int32_t cin, int32_t cout,
                                int32_t group_size);
size_t dd_conv3x3_mask_bytes(int64_t B, int32_t cout, int32_t h, int32_t w);
int dd_conv3x3_forward(const float* x, int64_t B, int32_t cin, int32_t h, int32_t w,
                       const void* packed, int32_t cout, const float* bias,
                       const float* residual, const float* mask_src, int32_t relu,
                       const float* in_scale, const float* in_shift, int32_t in_relu,
                       int32_t group_size, int64_t n_stat, float* stats, uint16_t* mask_out,
                       const uint16_t* mask_in, float* y, int32_t operands, float acc_scale,
                       void* stream);
/* Residual-unit output fused into the next unit's first conv (EL2N pass, train-mode BN):
 *   dd_conv3x3_forward_unit_input: x = max(y_prev * in_scale[g][c] + in_shift[g][c] + R, 0)
 *     with R = 0 (res NULL: the stem's BN + ReLU), res (identity shortcut) or res *
 *     res_scale[g][c] + res_shift[g][c] (the projection shortcut's BN), i.e. reference
 *     models/resnet.py:31-32 (out = bn2(conv2(.)); out += shortcut(x); relu(out)) and :89
 *     (relu(bn1(conv1(x)))), computed while the conv stages it: x is written to x_out
 *     [B][cin][h][w] once (the unit's output, which the next unit adds as its shortcut) and
 *     y = conv(x) with BN statistics as dd_conv3x3_forward (stats required, group_size as
 *     there).  Replaces a dd_bn_apply pass over y_prev and res plus the conv's read of its
 *     output.  x_out is bitwise dd_bn_apply's output, y bitwise dd_conv3x3_forward's on it.
 *   dd_conv3x3_unit_input_supported: 1 where the fused form exists (the scoring tiles: 32x32,
 *     and 16x16 / 8x8 with cout a multiple of 128; cin > 5), else 0. */
int dd_conv3x3_unit_input_supported(int32_t h, int32_t w, int32_t cin, int32_t cout,
                                    int32_t group_size);
int dd_conv3x3_forward_unit_input(const float* y_prev, const float* in_scale,
                                  const float* in_shift, const float* res,
                                  const float* res_scale, const float* res_shift, float* x_out,
                                  int64_t B, int32_t cin, int32_t h, int32_t w,
                                  const void* packed, int32_t cout, int32_t group_size,
                                  int64_t n_stat, float* stats, float* y, int32_t operands,
                                  float acc_scale, void* stream);

/* ---------------------------------------------------------------------------------------- *
 * The ImageNet stem's 7x7 / stride 2 / pad 3 conv, 3 -> cout <= 64 channels (reference
 * models/resnet.py ImageNet stem; BASELINE config 5), the EL2N launch shape (ABI 10):
 *   y [B][cout][h/2][w/2] = conv(x [B][3][h][w]) with BN partial statistics over rows b < n_stat
 *   in groups of group_size, one partial per (group, channel, 32-position fragment of an
 *   output-row pair): tiles_per_group = dd_stem7_tiles_per_group(h, w, group_size) =
 *   group_size * ceil(h / 4) * 8, images_per_tile 1 for dd_bn_finalize.
 * h, w even, w / 2 a multiple of 4 and at most 128.  The staged rows replace the implicit
 * GEMM's per-chunk gathers (dd_conv_gemm_forward's dense mode).
 *   dd_stem7_pack: W [cout][3][7][7] -> hi/lo fragment pack (dd_stem7_pack_bytes() bytes) in
 *     the `operands` halves (scale: a power of two for fp16, 1 for bf16; the forward takes its
 *     inverse as acc_scale).
 * ---------------------------------------------------------------------------------------- */
size_t dd_stem7_pack_bytes(void);
int dd_stem7_pack(const float* w, int32_t cout, int32_t operands, float scale, void* packed,
                  void* stream);
int dd_stem7_supported(int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t group_size);
int dd_stem7_tiles_per_group(int32_t h, int32_t w, int32_t group_size);
int dd_stem7_forward(const float* x, int64_t B, int32_t h, int32_t w, const void* packed,
                     int32_t cout, int32_t group_size, int64_t n_stat, float* stats, float* y,
                     int32_t operands, float acc_scale, void* stream);

/* ---------------------------------------------------------------------------------------- *
 * ResNet downsampling head (reference models/resnet.py:12 BasicBlock conv1 at stride 2 and
 * :20-23 its 1x1 stride-2 projection shortcut), split-bf16 MFMA, one launch for both:
 *   y    = epi(conv3x3_s2_p1(x, packed3x3))   [B][cout][ho][wo], x [B][cin][2 ho][2 wo]
 *   y_sc = epi_sc(conv1x1_s2(x, packed1x1))   (packed1x1 / y_sc NULL: no shortcut)
 * epi(v) = relu?(v + bias[o]) (bias may be NULL); stats / stats_sc: grouped BN partials as
 * for dd_conv3x3_forward with tiles_per_group = dd_down_tiles_per_group(ho, wo, group_size).
 * The shortcut reads exactly the centre tap of the stride-2 window, so it shares the staged
 * input and B fragments.  Output shapes: wo = 32 with even ho, wo = 16 with ho % 4 == 0,
 * 8x8, 4x4.  Padded-width heads (ABI 10): the statistics launch of a stride-2 conv alone (no
 * shortcut, bias or relu; cin > 64; cout padded to a multiple of 128), the ResNet-50
 * Bottleneck conv2 at stride 2 (reference models/resnet.py:42-43), also runs at 16 < wo <= 32
 * with wo % 4 == 0, 8 < wo <= 16 with wo even, and 4 < wo <= 8, any ho: the ImageNet-stem
 * network's 56 -> 28, 28 -> 14, 14 -> 7 heads.  The map is staged into the next tile width
 * with zero columns / rows, never stored or counted; tiles_per_group = group_size *
 * ceil(ho / rb) * 2 (rb = 2 / 4 / 8), images_per_tile 1.  DD_DOWN_PW=0 turns them off.
 *   dd_down_padded_supported: 1 where such a launch takes the padded-width head, else 0.
 *   dd_conv1x1_pack: 1x1 weights [cout][cin] -> hi/lo fragment pack in the `operands` halves
 *     (dd_conv1x1_pack_bytes(out_ch, in_ch)); transpose = 1 packs W^T (out = cin, in = cout).
 * `operands` (DD_OPERANDS_*) of the forward entry points must be the packs'; the fp16 form
 * exists for the statistics epilogue (with or without the staging transform) and the run-time
 * epilogue.
 * ---------------------------------------------------------------------------------------- */
size_t dd_conv1x1_pack_bytes(int32_t out_channels, int32_t in_channels);
int dd_conv1x1_pack(const float* w, int32_t cout, int32_t cin, int32_t transpose,
                    int32_t operands, float scale, void* packed, void* stream);
int dd_down_tiles_per_group(int32_t ho, int32_t wo, int32_t group_size);
int dd_down_padded_supported(int32_t ho, int32_t wo, int32_t cin, int32_t cout,
                             int32_t group_size);
int dd_down_forward(const float* x, int64_t B, int32_t cin, int32_t ho, int32_t wo,
                    const void* packed3x3, const void* packed1x1, int32_t cout,
                    const float* bias, int32_t relu, float* stats, float* y,
                    const float* bias_sc, int32_t relu_sc, float* stats_sc, float* y_sc,
                    int32_t group_size, int64_t n_stat, int32_t operands, float acc_scale,
                    float acc_scale_sc, void* stream);
/* The downsampling head with its input computed while staging (EL2N pass, train-mode BN;
 * replaces a dd_bn_apply pass and the head's read of its output):
 *   dd_down_forward_unit_input: x = max(y_prev * in_scale[g][c] + in_shift[g][c] (+ res), 0),
 *     then y / y_sc and their BN statistics as dd_down_forward (stats required; no bias or
 *     ReLU epilogue).  With res (the previous BasicBlock unit's identity shortcut) x is that
 *     unit's output relu(bn2(conv2(.)) + shortcut) (reference models/resnet.py:31-32), which
 *     only this head reads, so it is never written; res needs packed1x1 / y_sc / stats_sc (the
 *     stage head's projection).  Without res and without a shortcut, x is the producer's
 *     BN + ReLU (a Bottleneck's stride-2 conv2, reference :42).  x is bitwise dd_bn_apply's
 *     output, y / y_sc / stats bitwise dd_down_forward's on it. */
int dd_down_forward_unit_input(const float* y_prev, const float* in_scale,
                               const float* in_shift, const float* res, int64_t B, int32_t cin,
                               int32_t ho, int32_t wo, const void* packed3x3,
                               const void* packed1x1, int32_t cout, float* stats, float* y,
                               float* stats_sc, float* y_sc, int32_t group_size,
                               int64_t n_stat, int32_t operands, float acc_scale,
                               float acc_scale_sc, void* stream);
/* Backward-data of the head (the GraNd backward through models/resnet.py:12, :20-23):
 *   dx = (conv3x3_s2^T(dh, W) + conv1x1_s2^T(dz, Ws)) * (mask_src > 0)   [B][cin][2ho][2wo]
 * dh, dz [B][cout][ho][wo] (dz / packed1x1_t NULL: no shortcut; mask_src NULL: no mask);
 * packed3x3_t = dd_conv3x3_pack(W, transpose_flip = 1), packed1x1_t = dd_conv1x1_pack(Ws,
 * transpose = 1).  Computed as the 4 sub-pixel parity classes of dx (no zero insertion). */
int dd_down_backward(const float* dh, const float* dz, int64_t B, int32_t cout, int32_t ho,
                     int32_t wo, const void* packed3x3_t, const void* packed1x1_t, int32_t cin,
                     const float* mask_src, const uint32_t* mask_bits, float* dx,
                     void* stream);

/* The ReLU-backward mask of a downsampling head's input as bits (the GraNd backward, reference
 * models/resnet.py:31 relu of the previous block's output): dd_down_backward takes either the
 * fp32 tensor (mask_src: dx = 0 where !(mask_src > 0)) or mask_bits = plane bits, bit p & 31
 * of word ((b * cin + c) * 4 ho wo + p) >> 5 (wo in {4, 8, 16}), one 32nd of its bytes.
 *   dd_conv3x3_mask_plane_bits: the mask_out words of a dd_conv3x3_forward launch (B, cout,
 *     h, w, ungrouped) -> plane bits [B * cout * h * w / 32] (h * w a multiple of 32). */
int dd_conv3x3_mask_plane_bits(const uint16_t* mask, int64_t B, int32_t cout, int32_t h,
                               int32_t w, uint32_t* bits, void* stream);

/* ---------------------------------------------------------------------------------------- *
 * 1x1 convolution on split-bf16 MFMA (ResNet-50 Bottleneck conv1 / conv3, reference
 * models/resnet.py:40, 44, and the 1x1 projection shortcuts :49-54 at stride 1 or 2), the
 * GEMM y[b][o][p] = sum_c W[o][c] xf(x[b][c][stride * p]) over the flattened (b, p) space:
 *   packed = dd_conv1x1_pack(W, transpose = 0) (forward) or (W, transpose = 1) (backward-data:
 *     out = cin, in = cout, stride 1);
 *   epi(v) = ((v + bias[o]) + residual + up2(res_up2)) -> max(.,0) if relu -> 0 where
 *     !(mask_src > 0); up2(r)[b][o][y][x] = r[b][o][y/2][x/2] at even (y, x), else 0 (the
 *     backward of a stride-2 projection fused into the block-input gradient);
 *   xf / in_scale / in_shift / in_relu / group_size / n_stat / stats exactly as
 *     dd_conv3x3_forward, with tiles_per_group = dd_conv1x1_tiles_per_group(ho, wo,
 *     group_size) = group_size * ho * wo / 64 (requires group_size * ho * wo % 128 == 0):
 *     one partial per 64 consecutive positions of the group's flattened (example, position)
 *     space, consumed by dd_bn_finalize with images_per_tile = -64.
 * Any h, w (even at stride 2); output [B][cout][h / stride][w / stride].
 * ---------------------------------------------------------------------------------------- */
int dd_conv1x1_tiles_per_group(int32_t ho, int32_t wo, int32_t group_size);
int dd_conv1x1_forward(const float* x, int64_t B, int32_t cin, int32_t h, int32_t w,
                       int32_t stride, const void* packed, int32_t cout, const float* bias,
                       const float* residual, const float* res_up2, const float* mask_src,
                       int32_t relu, const float* in_scale, const float* in_shift,
                       int32_t in_relu, int32_t group_size, int64_t n_stat, float* stats,
                       float* y, int32_t operands, float acc_scale, void* stream);
/* A ResNet-50 unit's output fused into the next unit's first (1x1, stride-1) conv (ABI 8;
 * the EL2N forward of configs 4-5, reference models/resnet.py:57-63): the conv's input is
 *   xout = relu(y_prev * scale + shift [+ xres (* xres_scale + xres_shift)])
 * computed while staging in dd_bn_apply's arithmetic order (bitwise that pass), written to xout
 * once (the next unit's residual / projection input), and y / stats are those of
 * dd_conv1x1_forward(xout, ...) with the grouped BN statistics epilogue (no bias, residual,
 * mask or ReLU on y). scale / shift / xres_* are [G][cin] per group_size rows; xres NULL: no
 * residual; xres_scale / xres_shift NULL: an identity residual. Needs h * w % 4 == 0 and
 * 16-byte aligned tensors (DD_EINVAL otherwise). */
int dd_conv1x1_forward_unit_input(const float* y_prev, const float* scale, const float* shift,
                                  const float* xres, const float* xres_scale,
                                  const float* xres_shift, float* xout, int64_t B, int32_t cin,
                                  int32_t h, int32_t w, const void* packed, int32_t cout,
                                  int32_t group_size, int64_t n_stat, float* stats, float* y,
                                  int32_t operands, float acc_scale, void* stream);

/* ---------------------------------------------------------------------------------------- *
 * Any kh x kw convolution (stride 1 or 2, zero padding `pad`) as an implicit GEMM on the same
 * kernel: the ResNet-50 ImageNet-stem network of config 5 (reference models/resnet.py: the
 * 7x7/2 stem conv and the 3x3 convs at 56 / 28 / 14 / 7, stride 1 and 2), forward only.
 *   packed = dd_conv_gemm_pack(W [cout][cin][kh][kw]) (dd_conv_gemm_pack_bytes bytes): K is
 *     (tap, channel) tap-major with each tap's channels padded to 32, or (channel, tap) dense
 *     (PyTorch's weight order, padded to 32) when dd_conv_gemm_dense(cin, kh, kw) = 1
 *     (inputs with fewer than 32 channels: the 7x7 stem's K = 147 in 5 chunks, not 49);
 *   y[B][cout][ho][wo], ho = (h + 2 pad - kh) / stride + 1 (likewise wo),
 *     = epi(sum_{c,ky,kx} W[o][c][ky][kx] xf(x)[b][c][ho*s + ky - pad][wo*s + kx - pad]),
 *     xf applied before the zero padding (a dense pack takes no xf); bias / residual / relu /
 *     in_* / group_size / n_stat / stats exactly as dd_conv1x1_forward.
 * ---------------------------------------------------------------------------------------- */
int dd_conv_gemm_dense(int32_t cin, int32_t kh, int32_t kw);
size_t dd_conv_gemm_pack_bytes(int32_t out_channels, int32_t in_channels, int32_t kh,
                               int32_t kw);
int dd_conv_gemm_pack(const float* w, int32_t cout, int32_t cin, int32_t kh, int32_t kw,
                      int32_t operands, float scale, void* packed, void* stream);
int dd_conv_gemm_forward(const float* x, int64_t B, int32_t cin, int32_t h, int32_t w,
                         int32_t kh, int32_t kw, int32_t stride, int32_t pad,
                         const void* packed, int32_t cout, const float* bias,
                         const float* residual, int32_t relu, const float* in_scale,
                         const float* in_shift, int32_t in_relu, int32_t group_size,
                         int64_t n_stat, float* stats, float* y, int32_t operands,
                         float acc_scale, void* stream);

/* ---------------------------------------------------------------------------------------- *
 * Grouped train-mode BatchNorm (the reference's scoring forward runs BN with batch
 * statistics: train.py:59-63 never calls .eval(); BN layers models/resnet.py:13-16, 72).
 * One launch carries G = ceil(B / group_size) pinned batches, each normalised with its own
 * statistics; rows b >= n_valid are excluded (a ragged final batch).
 *   dd_channel_stats: partials of any NCHW tensor y [B][C][hw] in the layout above with
 *     tiles_per_group = group_size, images_per_tile = 1, row_tiles = 1.
 *   dd_bn_finalize: per (group, channel): mean, biased variance over count(g) * hw values
 *     (count(g) = clamp(n_valid - g * group_size, 0, group_size); the first
 *     ceil(count / images_per_tile) * row_tiles tiles; images_per_tile = -T < 0: tiles of T
 *     consecutive positions of the group's flattened (example, position) space, the first
 *     ceil(count * hw / T) of them), summed in double in a fixed order;
 *     scale = gamma / sqrt(var + eps), shift = beta - mean * scale  ([G][C] fp32 each).
 *   dd_bn_apply: out = relu?(y * scale + shift + R) with R = 0 (residual NULL), the raw
 *     residual, or max?(residual * res_scale + res_shift) (its own BN, res_relu);
 *     reference BasicBlock tail models/resnet.py:30-31.  pool_out [B][C] (may be NULL):
 *     the spatial mean of out (the CIFAR head avg_pool2d(out, 4), :94); out may then be NULL.
 *     Pooling needs hw / 4 a power of two <= 64 and 16-B aligned tensors.
 * ---------------------------------------------------------------------------------------- */
int dd_channel_stats(const float* y, int64_t B, int32_t C, int64_t hw, int32_t group_size,
                     int64_t n_stat, float* stats, void* stream);
int dd_bn_finalize(const float* stats, int64_t n_groups, int32_t group_size, int64_t n_valid,
                   int32_t tiles_per_group, int32_t images_per_tile, int32_t row_tiles,
                   int32_t C, int64_t hw, const float* gamma, const float* beta, float eps,
                   float* scale, float* shift, void* stream);
/* dd_bn_apply_maxpool: the ImageNet stem tail, relu(y * scale + shift) then max_pool2d(3,
 *   stride 2, padding 1) in one pass: out [B][C][(h-1)/2+1][(w-1)/2+1] (the 112x112 stem
 *   output is never written at full resolution). */
int dd_bn_apply_maxpool(const float* y, int64_t B, int32_t C, int32_t h, int32_t w,
                        int32_t group_size, const float* scale, const float* shift,
                        float* out, void* stream);
int dd_bn_apply(const float* y, int64_t B, int32_t C, int64_t hw, int32_t group_size,
                const float* scale, const float* shift, const float* residual,
                const float* res_scale, const float* res_shift, int32_t res_relu, int32_t relu,
                float* out, float* pool_out, void* stream);

/* ---------------------------------------------------------------------------------------- *
 * K-checkpoint ensemble (north star (c); the reference scores one hard-coded checkpoint,
 * train.py:61, train_sparse.py:23, ddp.py:72).
 *   dd_sqrt_accumulate : accum[b] += sqrt(sq[b])       (GraNd norm of one checkpoint)
 *   dd_ensemble_finalize: out[i] = accum[i] / K          (mean over K checkpoints)
 * ---------------------------------------------------------------------------------------- */
int dd_sqrt_accumulate(const float* sq, int64_t B, float* accum, void* stream);
int dd_ensemble_finalize(const float* accum, int64_t n, int32_t K, float* out, void* stream);

/* ---------------------------------------------------------------------------------------- *
 * Keep-set selection (reference get_scores_and_prune.py:22-24):
 *   samples = int((1 - sparsity) * train_samples)                          (:22)
 *   indices = [i for i, s in sorted(scores, key=s, reverse=True)[:samples]]  (:23-24)
 * dd_keep_count returns `samples` with the reference's IEEE-double truncation.
 *
 * dd_select_topk: keys fp32 [n] (key i belongs to index i), k in [0, n].  Writes
 *   idx_out int64 [k] : the k indices of largest key, ordered by key descending and, among
 *                       equal keys, by ascending index (Python's stable sort with
 *                       reverse=True keeps visit order; +0.0 == -0.0 as in Python);
 *   thr_out fp32 [1]  : the k-th largest key (NULL allowed; unspecified when k == 0).
 *   nan_count_out int32 [1] (device, NULL allowed): number of NaN keys.  The reference's
 *                       sort is undefined on NaN; here NaN ranks below every number.  The
 *                       host wrapper reads this after the call and raises (no sync inside).
 * One read of the keys for an 11-bit top-digit histogram (the threshold bin), a second that
 * compacts the m >= k keys in or above that bin in index order, then three stable LSD radix
 * passes over them on the low ceil(R / 3) bits of key - base (R = the survivors' key range
 * in bits, decided on the device); n < 2^31.  Workspace: dd_select_workspace_bytes(n), 16-byte
 * aligned (its per-call state is cleared on the stream: reusable across calls and graph replays).
 * ---------------------------------------------------------------------------------------- */
int64_t dd_keep_count(int64_t train_samples, double sparsity);

size_t dd_select_workspace_bytes(int64_t n);

int dd_select_topk(const float* keys, int64_t n, int64_t k, int64_t* idx_out, float* thr_out,
                   int32_t* nan_count_out, void* workspace, size_t workspace_bytes,
                   void* stream);

/* ---------------------------------------------------------------------------------------- *
 * Keep-set selection with per-class quotas (absent from the reference, whose only rule is the
 * global top-k above).  Purely additive: no existing signature or result changes, so
 * dd_abi_version() stays 10.
 *
 * Within class c (labels[i] == c) the members are ranked by key descending, ties by ascending
 * index, NaN below every number (+0.0 == -0.0): dd_select_topk's order restricted to the class.
 * Class c keeps the members at in-class ranks [skip[c], skip[c] + quota[c]).
 *
 * dd_class_counts: labels int64 [n]; counts_out int64 [num_classes] (device) = members per
 *   class; bad_label_out int32 [1] (device) = labels outside [0, num_classes), which count
 *   into no class.  Both are cleared first.  Integer atomics only; n < 2^31.
 *
 * dd_select_topk_by_class: keys fp32 [n], labels int64 [n], skip / quota int64 [num_classes]
 *   (device), k_total = sum of the quotas, in [0, n].  Writes
 *   idx_out int64 [k_total] : every kept index, ordered by key descending and ties by ascending
 *                       index over the whole set (the order dd_select_topk gives); never
 *                       written past k_total entries;
 *   nan_count_out int32 [1] (device, NULL allowed): number of NaN keys;
 *   err_out int32 [1] (device): labels outside [0, num_classes) + classes with skip < 0,
 *                       quota < 0 or skip + quota above the class's size + 1 if the kept
 *                       entries do not number k_total.  Non-zero: idx_out is unspecified.  The
 *                       host wrapper reads it after the call and raises (no sync inside).
 * The full stable order comes from dd_select_topk with k = n; a stable counting pass over the
 * class ids along that order gives every entry its in-class rank (per-block class histograms,
 * a scan over blocks, an in-tile rank), and a stable compaction of the entries inside their
 * class's window writes idx_out.  n < 2^31, num_classes <= 2^20.  Workspace:
 * dd_select_by_class_workspace_bytes(n, num_classes) (0 for unsupported sizes), 16-byte
 * aligned; its per-call state is cleared on the stream: reusable across calls and graph replays.
 * ---------------------------------------------------------------------------------------- */
int dd_class_counts(const int64_t* labels, int64_t n, int64_t num_classes, int64_t* counts_out,
                    int32_t* bad_label_out, void* stream);

size_t dd_select_by_class_workspace_bytes(int64_t n, int64_t num_classes);

int dd_select_topk_by_class(const float* keys, const int64_t* labels, int64_t n,
                            int64_t num_classes, const int64_t* skip, const int64_t* quota,
                            int64_t k_total, int64_t* idx_out, int32_t* nan_count_out,
                            int32_t* err_out, void* workspace, size_t workspace_bytes,
                            void* stream);

/* ---------------------------------------------------------------------------------------- *
 * Distance to the class prototype in feature space (absent from the reference, whose one score
 * is a function of the logits).  Purely additive: no existing signature or result changes, so
 * dd_abi_version() stays 10.
 *
 *   mu_c    = mean of f_i over every example of the dataset with label c
 *   proto_i = || f_i - mu_{y_i} ||_2          (f_i fp32 [D]: the row the classifier consumes)
 *
 * The mean spans launch chunks, lanes and ranks, so it is summed in fixed point: exact integer
 * addition is order-free, which keeps the scores bitwise independent of the chunk size, the lane
 * count and the world size (a float sum over shards could not).  Integer atomics only.
 * Limits of all three: 1 <= D <= 4096 (dd_linear_forward's), 1 <= C <= 2^20, n (B) < 2^31;
 * outside them, or a NULL buffer that the call would touch, is DD_EINVAL before any launch.
 * No allocation, no synchronisation inside (graph-capturable).
 *
 * dd_class_feature_sums: feat fp32 [n][D], labels int64 [n], sums int64 [C][D], bad_feat int32
 *   [C] (device).  sums[y_i][d] += q(f_i[d]) with q(v) = round-to-nearest-even(v * 2^24) as
 *   int64.  It ACCUMULATES (the caller clears both buffers): two calls over a split of the rows
 *   equal one call over all of them, whatever the split, the row order or the launch geometry.
 *   A row with an element that is NaN, infinite or has |v| >= 2^15 adds nothing to sums and adds
 *   one to bad_feat[y_i].  A row whose label lies outside [0, C) adds nothing anywhere (dd_el2n /
 *   dd_logit_scores count such rows).  |q| < 2^39, so a class of fewer than 2^24 members cannot
 *   overflow; the caller rejects larger classes (dd_class_counts gives the sizes).
 *   order int64 [n] or NULL: the sequence in which the rows are visited, meant to be the rows
 *   stable-sorted by label; an entry outside [0, n) names no row.  A workgroup takes a run of
 *   consecutive entries and every column, sums in int64 registers while the class stays the same
 *   and issues one 64-bit atomic per column when it changes and at the end of the run: about
 *   (n / rows-per-workgroup + C) D atomics.  NULL takes the rows as they lie: the same sums,
 *   more atomics.  n == 0 returns DD_OK.
 *
 * dd_class_centroids: counts int64 [C] (dd_class_counts), centroids fp32 [C][D]:
 *   centroids[c][d] = (float)(((double)sums[c][d] / (double)counts[c]) * 2^-24);
 *   0 where counts[c] == 0 (nothing reads it); NaN where bad_feat[c] != 0, so that every member
 *   of a class with an unrepresentable row scores NaN, on every rank alike.
 *
 * dd_proto_scores: feat fp32 [B][D], labels int64 [B], centroids fp32 [C][D]; score / accum fp32
 *   [B], either may be NULL but not both:
 *   score[b] = sqrt(sum_d (feat[b][d] - centroids[y_b][d])^2) in fp32;  accum[b] += score[b].
 *   A label outside [0, C) gives NaN (dd_el2n's rule), a NaN or infinite feature gives NaN.
 *   Each row is reduced from that row alone in an order fixed by D alone: bitwise independent
 *   of B, of the row's position and of the buffers' alignment.  B == 0 returns DD_OK.
 * ---------------------------------------------------------------------------------------- */
int dd_class_feature_sums(const float* feat, const int64_t* labels, const int64_t* order,
                          int64_t n, int32_t D, int64_t C, int64_t* sums, int32_t* bad_feat,
                          void* stream);

int dd_class_centroids(const int64_t* sums, const int64_t* counts, const int32_t* bad_feat,
                       int64_t C, int32_t D, float* centroids, void* stream);

int dd_proto_scores(const float* feat, const int64_t* labels, const float* centroids, int64_t B,
                    int32_t D, int64_t C, float* score, float* accum, void* stream);

/* ---------------------------------------------------------------------------------------- *
 * Distance to the nearest neighbour of the same class in feature space: a redundancy signal (a
 * near-duplicate scores close to 0).  Purely additive: dd_abi_version() stays 10.
 *
 *   nn_r = min over candidates j of the query's class with c_id[j] != q_id[r] of || q_r - c_j ||_2
 *
 * q fp32 [nq][D] (queries) and c fp32 [nc][D] (candidates), both grouped by class: q_off / c_off
 * int64 [C + 1] (device) give segment k of q, which is searched in segment k of c only; a segment
 * may be empty.  Offsets that decrease or leave the buffers are clamped on the device (never an
 * access outside); a query row outside every segment has no candidate.  q_id / c_id int64: the
 * rows' global example indices; the candidate with the query's own id is skipped.
 *
 * The search minimises key(r, j) = ||c_j||^2 - 2 q_r . c_j over the segment, the dot product on
 * split MFMA (hi.hi + hi.lo + lo.hi of the `operands` halves, fp32 accumulation, 32x32x16, D
 * zero-padded to a multiple of 16, K order fixed by D), ||c_j||^2 in fp32 in an order fixed by
 * D, and keeps the smallest (key, c_id) pair, compared lexicographically: a tie goes to the
 * smaller id.  No atomics.  A candidate row with a non-finite element is never chosen (its key is
 * NaN, and a NaN key is never the smaller one; so is the key of a pair whose halves leave the
 * operand type's range, |v| >= 65504 in fp16).  The value is then taken in fp32 from the fp32
 * rows, one row per wave in an order fixed by D (dd_proto_scores' reduction):
 *   dist[r] = sqrt(sum_d (q[r][d] - c[pick][d])^2),  nn_id[r] = c_id[pick],  accum[r] += dist[r]
 * so an exact duplicate scores exactly 0, and the MFMA rounding decides only WHICH neighbour is
 * picked: d^2(pick) - d^2(best) <= 2 eps (||q||^2 + max_j ||c_j||^2) with
 * eps = (2^-22 fp16 halves | 2^-16 bf16 halves) + (D + 2) 2^-24.
 * No admissible candidate (a class of one): dist = +inf, nn_id = -1.  A query row with a
 * non-finite element: dist = NaN, nn_id = -1.  Any of dist / nn_id / accum may be NULL, not all.
 *
 * dist[r] and nn_id[r] depend on row r, on the candidate SET of its class and on D: bitwise
 * independent of the batching of the queries, of nq, of the rows' positions and the buffers'
 * alignment, and of the launch geometry.
 *
 * Limits: 1 <= D <= 4096, 1 <= C <= 2^20, 0 <= nq, nc < 2^31, operands DD_OPERANDS_F16X3 or
 * DD_OPERANDS_BF16X3; outside them, a NULL buffer the call would touch, or a workspace that is
 * too small or not 16-byte aligned is DD_EINVAL with a message before any launch.  nq == 0
 * returns DD_OK.  The workspace (dd_nn_workspace_bytes: host only, 0 for bad arguments) holds
 * the halves of every row, split once per call: 4 (nq + nc) pad16(D) bytes, plus 4 (nq + nc).
 * No allocation, no synchronisation inside (graph-capturable); plain vector stores only.
 * ---------------------------------------------------------------------------------------- */
size_t dd_nn_workspace_bytes(int64_t nq, int64_t nc, int32_t D, int32_t operands);

int dd_nn_same_class(const float* q, const int64_t* q_id, const int64_t* q_off, int64_t nq,
                     const float* c, const int64_t* c_id, const int64_t* c_off, int64_t nc,
                     int64_t C, int32_t D, int32_t operands, float* dist, int64_t* nn_id,
                     float* accum, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------- *
 * The k nearest neighbours of a row over ALL classes in feature space: the mean distance to them
 * (a density / coverage signal that needs no labels) and the share of them that carry another
 * label (deep k-NN label-noise filtering).  Purely additive: dd_abi_version() stays 10.
 *
 *   N_k(r) = the k candidates j with c_id[j] != q_id[r] with the smallest (d^2(r, j), c_id[j]),
 *            compared lexicographically
 *   mean_dist[r] = (1 / k) sum over j in N_k(r) of || q_r - c_j ||_2
 *   disagree[r]  = |{ j in N_k(r) : c_label[j] != q_label[r] }| / k
 *
 * q fp32 [nq][D] (queries) and c fp32 [nc][D] (candidates), in any order; q_id / c_id int64: the
 * rows' global example indices (distinct among the candidates); q_label / c_label int64, compared
 * for equality only, and NULL is allowed when neither disagree nor accum_disagree is asked for.
 *
 * The search picks on dd_nn_same_class's key, key(r, j) = ||c_j||^2 - 2 q_r . c_j, the dot product
 * on split MFMA (hi.hi + hi.lo + lo.hi of the `operands` halves, fp32 accumulation, 32x32x16, D
 * zero-padded to a multiple of 16, K order fixed by D), and keeps the k smallest (key, c_id)
 * pairs; a tie goes to the smaller id.  A workgroup searches one of `splits` contiguous candidate
 * segments for 128 queries and writes the segment's k smallest pairs per query to the workspace;
 * a second kernel takes the k smallest of those.  splits == 0 lets the library choose the count
 * from nq and nc alone (two workgroups per compute unit where the sizes allow).  No atomics.  A
 * candidate with a non-finite element is never picked (its key is NaN; only a finite key is
 * admitted, so a pair whose halves leave the operand type's range, |v| >= 65504 in fp16, is not
 * picked either).  The values are then taken in fp32 from the fp32 rows, one row per wave in an
 * order fixed by D (dd_proto_scores' reduction), for slot i = 0 .. k - 1 in ascending (key, id):
 *   dist[r][i] = sqrt(sum_d (q[r][d] - c[pick_i][d])^2),  nbr_id[r][i] = c_id[pick_i]
 * so an exact duplicate contributes exactly 0 and the MFMA rounding decides only WHICH rows are
 * picked: for every pick p, d^2(p) - d^2(k-th best) <= 2 eps (||q||^2 + max_j ||c_j||^2), eps as
 * for dd_nn_same_class.  mean_dist is the sum of the k distances in slot order (accumulated in
 * double, rounded once) over k; accum_dist[r] += mean_dist[r], accum_disagree[r] += disagree[r].
 * Fewer than k admissible candidates: the unused slots hold dist = +inf and nbr_id = -1,
 * mean_dist = +inf and disagree = NaN.  A query row with a non-finite element: NaN everywhere,
 * ids of -1.  Any output may be NULL, not all.
 *
 * Invariance: a key is a function of the two rows and D alone, and the k smallest of a set of
 * (key, id) pairs under one total order do not depend on how the set is split or traversed.  So
 * every output of row r depends on row r, on the candidate SET, on D and on k: bitwise
 * independent of `splits`, of the batching of the queries, of nq, of the rows' positions and the
 * buffers' alignment, and of the launch geometry.
 *
 * Limits: 1 <= k <= DD_KNN_MAX_K, 1 <= D <= 4096, 0 <= nq, nc < 2^31, 0 <= splits <= 64, operands
 * DD_OPERANDS_F16X3 or DD_OPERANDS_BF16X3; outside them, a NULL buffer the call would touch, no
 * output requested, or a workspace that is too small or not 16-byte aligned is DD_EINVAL with a
 * message before any launch.  nq == 0 returns DD_OK.  The workspace (dd_knn_workspace_bytes: host
 * only, 0 for bad arguments; it depends on `splits` as passed to dd_knn) holds the halves of
 * every row, split once per call, 4 (nq + nc) pad16(D) bytes, 4 nc bytes of norms and the
 * partial lists, 8 nq splits k bytes, each region rounded up to 256.  No allocation, no
 * synchronisation inside (graph-capturable); plain vector stores only.
 * ---------------------------------------------------------------------------------------- */
#define DD_KNN_MAX_K 16

size_t dd_knn_workspace_bytes(int64_t nq, int64_t nc, int32_t D, int32_t k, int32_t splits,
                              int32_t operands);

int dd_knn(const float* q, const int64_t* q_id, const int64_t* q_label, int64_t nq,
           const float* c, const int64_t* c_id, const int64_t* c_label, int64_t nc, int32_t D,
           int32_t k, int32_t splits, int32_t operands, float* dist, int64_t* nbr_id,
           float* mean_dist, float* disagree, float* accum_dist, float* accum_disagree,
           void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------- *
 * Greedy k-center (farthest-first traversal; Sener & Savarese's core-set baseline) over feature
 * rows, inside groups: the coverage keep-set.  Purely additive: dd_abi_version() stays 10.
 *
 * rows fp32 [n][D] in GROUP ORDER: group g is rows [off[g], off[g + 1]) (off int64 [G + 1] on the
 * device, ascending, off[G] <= n), in ascending id inside a group (ids int64 [n], distinct inside
 * a group, 0 <= id < 2^31).  seeds int64: POSITIONS of rows, group g's at
 * [seed_off[g], seed_off[g + 1]) (seed_off int64 [G + 1] on the device), each inside its group;
 * max_seeds is the longest list (host).  picks int64 [G] on the device: the rows group g takes
 * after its seeds, seeds + picks <= the group's size; steps = max(picks) (host: the loop bound).
 *
 *   d2(i, c)  = sum_d (rows[i][d] - rows[c][d])^2, in fp32 from the fp32 rows, never
 *               |a|^2 + |b|^2 - 2 ab: an exact duplicate is at exactly 0, and on small-integer
 *               rows every sum is exact.  The order of the additions is fixed by D alone (lane l
 *               of a wave takes columns 256 j + 4 l + 0..3 in ascending order into one fma chain,
 *               then a fixed butterfly).
 *   mind2[i]  = min over the kept rows c of i's group of d2(i, c); -1 for a kept row; +inf in a
 *               group that keeps nothing
 *   step t of group g (t < picks[g]) takes the not-yet-kept row with the largest mind2, a tie to
 *   the smaller id:   picked[t][g] = its id,  radius2[t][g] = its mind2 at that moment
 *   and (t, g) with t >= picks[g]: picked = -1, radius2 = -1.  A kept row is never taken again.
 *   bad[0] += the rows with a NaN or infinite element (the caller clears it, and rejects the
 *   call's results when it is non-zero).
 *
 * Launches (all on `stream`, nothing read back, no allocation): one init; ceil(max_seeds / S) seed
 * launches, each folding up to S centres per group, staged in LDS, into rows read once (S =
 * seed_batch, 0: 8, capped so that S centres fit 48 KB); steps + 1 pick launches, launch t
 * folding the centre that launch t - 1 published and publishing one candidate per workgroup with a
 * 64-bit atomic maximum on (bits(mind2) << 32) | ~position into slot [t][g] of the workspace; one
 * finish launch.  The launch boundaries are the only ordering between workgroups: no kernel waits
 * for another workgroup.  `blocks`: workgroups per group (0: from n and G alone).
 *
 * Invariance: a d2 is a function of the two rows and D alone and min / max are order-independent,
 * so every output is bitwise independent of seed_batch, blocks, the rows' alignment, the other
 * groups and their layout, and of whether a centre arrives as a seed or as a pick.
 *
 * Limits: 0 <= n < 2^31, 1 <= D <= 4096, 1 <= G <= DD_KCENTER_MAX_GROUPS, 0 <= steps,
 * max_seeds <= n, 0 <= seed_batch <= DD_KCENTER_MAX_SEED_BATCH, 0 <= blocks <=
 * DD_KCENTER_MAX_BLOCKS; outside them, a NULL buffer the call would touch or
 * a workspace below dd_kcenter_workspace_bytes (host only; 0 for bad arguments; 8 max(steps, 1) G
 * bytes rounded up to 256) is DD_EINVAL with a message before any launch.  n == 0 returns DD_OK.
 * ---------------------------------------------------------------------------------------- */
#define DD_KCENTER_MAX_SEED_BATCH 64
#define DD_KCENTER_MAX_BLOCKS 4096
#define DD_KCENTER_MAX_GROUPS 65535

size_t dd_kcenter_workspace_bytes(int64_t n, int32_t D, int32_t G, int64_t steps);

/* The centres one seed launch folds per group for this D and `seed_batch` as passed to
 * dd_kcenter_greedy (host only; 0 for bad arguments). */
int32_t dd_kcenter_seed_batch(int32_t D, int32_t seed_batch);

int dd_kcenter_greedy(const float* rows, const int64_t* ids, int64_t n, int32_t D,
                      const int64_t* off, int32_t G, const int64_t* seeds,
                      const int64_t* seed_off, int64_t max_seeds, const int64_t* picks,
                      int64_t steps, int32_t seed_batch, int32_t blocks, int64_t* picked,
                      float* radius2, float* mind2, int32_t* bad, void* workspace,
                      size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DD_CAPI_H */
