/*
 * lseg_hip.h -- C ABI of the MI355X-native LSeg forward engine (liblseg_hip.so).
 *
 * Drop-in boundary for ONE hot path of isl-org/lang-seg: LSegNet.forward()
 * (modules/models/lseg_net.py:160-205 and everything it calls).  The reference
 * has no FFI layer -- the path sits behind a Python class API -- so these
 * entry points are what a ctypes binding inside the reference's
 * modules/models/lseg_net.py would call.  Every function
 * cites the reference interface it replaces.
 *
 * Conventions
 *   - plain C: pointers, sizes, ints.  No torch / C++ types cross the boundary.
 *   - every pointer named dev_* / d_* is DEVICE memory (HBM) owned by the caller;
 *     host pointers are named host_* .
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all work
 *     is stream-ordered, nothing synchronises the host unless documented.
 *   - one handle per device, not thread-safe per handle (the reference runs one
 *     Python thread per GPU replica: additional_utils/models.py:229-238).
 *   - return value: LSEG_OK (0) or a negative lseg_status; lseg_last_error()
 *     gives a message.  No C++ exception crosses the boundary.
 *   - there is NO CPU fallback: without a gfx950 device every compute entry
 *     point returns LSEG_ERR_NO_DEVICE.
 */
#ifndef LSEG_HIP_H
#define LSEG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LSEG_ABI_VERSION 1

typedef enum {
    LSEG_OK = 0,
    LSEG_ERR_INVALID = -1,     /* bad argument / shape */
    LSEG_ERR_NO_DEVICE = -2,   /* no HIP device / wrong arch */
    LSEG_ERR_HIP = -3,         /* a HIP runtime call failed */
    LSEG_ERR_STATE = -4,       /* call order (params not finalised, tokens not set...) */
    LSEG_ERR_UNSUPPORTED = -5, /* configuration outside what the engine implements */
    LSEG_ERR_MISSING_PARAM = -6
} lseg_status;

typedef enum { LSEG_F32 = 0, LSEG_F16 = 1, LSEG_BF16 = 2, LSEG_I64 = 3,
               LSEG_F16_SPLIT = 4   /* lseg_config.image_dtype only: split-precision validation mode, see below */
} lseg_dtype;

/* Resample op that follows the 1x1 conv of act_postprocessK
 * (modules/models/lseg_vit.py:446-523 / 315-396). */
typedef enum { LSEG_RS_IDENTITY = 0, LSEG_RS_CONVT = 1, LSEG_RS_CONV_S2 = 2 } lseg_resample;

/* Shape description of one network variant; mirrors the constants hard-coded at
 * lseg_net.py:119-123,142-146, lseg_vit.py:221-272, lseg_blocks.py:24-52 and the
 * [3P] timm / CLIP model dims.  Filled by the Python shim from `--backbone`. */
typedef struct {
    int32_t abi_version;      /* = LSEG_ABI_VERSION */
    /* image tower (timm VisionTransformer) */
    int32_t patch;            /* 16 | 32 */
    int32_t dim;              /* 1024 | 768 */
    int32_t depth;            /* 24 | 12 */
    int32_t heads;            /* 16 | 12 ; head_dim must be 64 */
    int32_t hooks[4];         /* lseg_net.py:119-123 */
    int32_t pos_grid;         /* pretrained pos-embed grid side (384/patch) */
    /* reassemble + DPT head */
    int32_t reassemble_ch[4]; /* channels after the 1x1 conv */
    int32_t resample_kind[4]; /* lseg_resample */
    int32_t resample_k[4];    /* ConvTranspose kernel=stride, or 3 for conv_s2 */
    int32_t features;         /* --num_features (256) */
    int32_t out_c;            /* 512 (768 for clipRN50x16_vitl16_384) */
    int32_t arch_option;      /* 0 | 1 (bottleneck_block) | 2 (depthwise_block), lseg_net.py:148-154 */
    int32_t block_depth;
    int32_t activation;       /* 0 relu, 1 lrelu, 2 tanh (lseg_net.py:47-52) */
    /* CLIP text tower */
    int32_t text_vocab, text_ctx, text_width, text_heads, text_layers;
    /* execution plan */
    int32_t img_h, img_w;     /* input size, multiples of patch (and such that the reassemble pyramid is a x2 ladder) */
    int32_t max_batch;        /* workspace is sized for this many images per call */
    int32_t max_labels;       /* workspace is sized for this many labels (K) */
    int32_t image_dtype;      /* MFMA operand type of the image tower: LSEG_BF16 (default), LSEG_F16, or LSEG_F16_SPLIT = every
                               * 16-bit operand as a (hi, lo) fp16 pair, three MFMA products per K-step (~21 mantissa bits: the
                               * reference's tower is fp32).  ~1/4 of the bf16 rate; a validation mode: its masks equal the
                               * reference's except at fp16-ulp ties of the reference's own fp16 logits.  Inference only. */
    int32_t flags;            /* bit 0: run the text tower on all text_ctx positions (reference schedule)
                               * instead of the exact causal truncation to max(EOT)+1 positions
                               * bit 1 (training): keep the gradient of the fp16 correlation in bf16 / fp32 instead of reproducing the
                               * reference's HALF-precision backward of `logit_scale * image_features.half() @ text_features.t()`
                               * (lseg_net.py:194): there d(logits), dA = d(logits) @ text and logit_scale * dA are fp16 tensors, and with
                               * d(logits) ~ 1 / (valid pixels) ~ 1e-6 they sit in fp16's subnormal range (step 6e-8) -- softmax
                               * probabilities below ~N * 3e-8 flush to zero.  Default (bit clear) = the reference's arithmetic.
                               * bit 2: batch-invariant schedule -- no split-K at small batches, so every GEMM accumulates K in one order
                               * whatever the batch size and image b of a batch equals the same image run alone to fp32 round-off
                               * (default: attn.proj / mlp.fc2 / the deep 3x3 convs split their contraction when B <= ~6)
                               * bit 3 (training): deterministic reductions -- the bias-gradient and BatchNorm column sums write partial
                               * rows summed in a fixed order instead of fp32 atomics: two runs of the same step on the same inputs
                               * give BIT-identical gradients (what torch.use_deterministic_algorithms buys the reference's
                               * training loop, modules/lsegmentation_module.py:66-81); one small extra launch per sum, no measurable cost per step (the
                               * Python front sets it by default: lseg_hip/engine.py, LSEG_DETERMINISTIC=0 clears it)
                               * bit 4 (training): train the arch_option 1/2 head blocks (lseg_net.py:43-79,198-201).  Without it
                               * lseg_set_train refuses arch_option 1/2; with it the train-mode forward keeps every block's output,
                               * n = max(block_depth - 1, 0) + 1 extra fp32 [max_batch, max_labels, h, w] plane sets (276 MB each at 8 x
                               * 150 labels, 480x480), and lseg_backward returns the gradient of scratch.head_block.depthwise.depthwise.
                               * {weight, bias} (bucket 0) -- always in a fixed summation order, bit 3 or not.  Not with per-image label
                               * sets (the zero-shot network has no head blocks).
                               * bit 5: the image tower is torchvision's ResNet-101 (the zero-shot CLIP-ResNet-101 network,
                               * LSegRNNetZS, lseg_net_zs.py:243-363): stem 7x7/2 + max-pool, layer1..4 (3, 4, 23, 3 Bottleneck v1.5
                               * blocks, every BatchNorm folded from its running statistics) feed scratch.layer1..4_rn with 256 / 512 /
                               * 1024 / 2048 channels at img/4 .. img/32; the neck, head and text tower are the ViT networks' own.
                               * Parameters under the reference's keys pretrained.layer1.{0,1,4.*}, pretrained.layer{2,3,4}.*.  The ViT
                               * fields (patch, dim, depth, heads, hooks, pos_grid, reassemble_*, resample_*) are ignored.  Refused:
                               * img_h / img_w not a multiple of 32 (LSEG_ERR_INVALID), image_dtype LSEG_F16_SPLIT, arch_option != 0 and
                               * lseg_set_train (LSEG_ERR_UNSUPPORTED).  Inference only, unless bit 6 is set.
                               * bit 6 (training, with bit 5 only; on a ViT config LSEG_ERR_INVALID): train the DECODER above the ResNet-101
                               * tower.  lseg_set_train(h, 1) is accepted (bf16 operands): the train-mode forward runs every conv of the
                               * tower on its unfolded weights and all 104 BatchNorms on batch statistics (biased variance), updating
                               * running_mean / running_var in the bound tensors (momentum 0.1, unbiased variance) -- the reference's
                               * module in train() with the pretrained group at lr 0.  lseg_backward* stops at the four stage outputs:
                               * scratch.* (layerN_rn, the refinenets, head1) is the whole trainable set, in bucket 0
                               * (lseg_num_grad_buckets = 1); pretrained.* has no bucket, no gradient and no optimizer state, and an
                               * optimizer step does not touch its masters or operand copies.  lseg_set_frozen_encoder keeps refusing the
                               * tower; synchronised BatchNorm (lseg_set_bn_sync with world_size > 1) is refused by the forward.  After
                               * lseg_set_train(h, 0) the next forward folds the BatchNorms again, from the updated running statistics. */
} lseg_config;

typedef struct lseg_engine* lseg_handle;

/* ---- life cycle ------------------------------------------------------------------
 * replaces: LSegNet.__init__ / LSeg.__init__ (lseg_net.py:104-158,208-226) as far as
 * device-side state is concerned (module construction itself stays in Python). */
int lseg_abi_version(void);
int lseg_device_count(void);
int lseg_create(const lseg_config* cfg, int device, lseg_handle* out);
int lseg_destroy(lseg_handle h);
const char* lseg_last_error(lseg_handle h);   /* h may be NULL: last error of this thread */

/* ---- parameters ------------------------------------------------------------------
 * replaces: nn.Module.load_state_dict / BaseModel.load (lseg_net.py:81-92).  `key` is a
 * state-dict key relative to `net.`, e.g.
 * "pretrained.model.blocks.3.attn.qkv.weight".  The engine converts/repacks into its
 * own HBM copies (bf16/fp16 tiles, BN folded into the conv weights, ConvTranspose
 * re-laid as a GEMM) during lseg_finalize_params; the caller's tensor is only read.
 * Re-bind + finalize again after the weights change (e.g. after an optimizer step). */
int lseg_bind_param(lseg_handle h, const char* key, const void* dev_ptr, int dtype,
                    const int64_t* shape, int ndim);
int lseg_finalize_params(lseg_handle h, void* stream);

/* ---- text --------------------------------------------------------------------------
 * replaces: `text = clip.tokenize(labels)` being handed to
 * `clip_pretrained.encode_text(text)` (lseg_net.py:158,163-164,181-183) and the fp16
 * L2 normalisation (lseg_net.py:192).  Tokens are what clip.tokenize returns: int64
 * [K, ctx] on the HOST.  lseg_encode_text runs the 12-layer tower and leaves the
 * normalised fp16 features [K, out_c] in the engine.  lseg_forward re-runs it on every
 * call (reference semantics) unless text caching is switched on. */
int lseg_set_text_tokens(lseg_handle h, const int64_t* host_tokens, int K, int ctx);
/* Text features computed elsewhere -- the value of `self.clip_pretrained.encode_text(text)` (lseg_net.py:183), fp16 [K, out_c] in
 * device memory, not necessarily normalised -- instead of tokens: the engine applies the fp16 L2 normalisation of :192 and never runs
 * its text tower until the next lseg_set_text_tokens (label banks of an application, lseg_app.py:350-355). */
int lseg_set_text_features(lseg_handle h, const void* dev_feat_f16, int K, void* stream);
int lseg_encode_text(lseg_handle h, void* stream);
int lseg_set_text_cache(lseg_handle h, int enabled);   /* 0 (default) = re-encode per forward */
int lseg_get_text_features(lseg_handle h, void* dev_out_f16 /* [K,out_c] fp16 */, void* stream);
/* Zero-shot variant -- replaces: LSegNetZS.forward(x, class_info) (lseg_net_zs.py:177-214): every image brings
 * its OWN label set.  labels_per_image = k > 0: the K = B*k token rows are grouped per image, image b is
 * correlated with rows [b*k, (b+1)*k) only and lseg_forward writes [B,k,img_h,img_w]; 0 (default) = one
 * label set shared by the batch.  Takes effect at the next lseg_forward (which must be called with B = K/k).
 * Train mode (lseg_set_train) accepts k = 1..8 (larger k: LSEG_ERR_UNSUPPORTED) with arch_option 0 only: lseg_forward writes the
 * [B,k,img_h,img_w] logits, lseg_train_loss / lseg_backward* take the loss over those k label planes per image (target values in
 * [0, k), anything else ignored) and back-propagate through the per-image correlation (LSegmentationModuleZS.training_step). */
int lseg_set_text_grouping(lseg_handle h, int labels_per_image);
/* Open-vocabulary batches: every image brings its own label list, of its OWN length (one list per request, lseg_app.py:350-355).
 * host_counts int32 [B] on the host, each in [1, 32767]: image b owns host_counts[b] consecutive rows of the K = sum of counts token rows
 * of lseg_set_text_tokens / lseg_set_text_features, image 0's rows first.  The SUM of the counts (not only each count) must be <=
 * max_labels: the lists' text rows are concatenated in the max_labels rows of the text workspace, and the training workspaces
 * (planes, rows, transposed panels) are sized on that bound; a larger sum returns LSEG_ERR_INVALID.  NULL or B = 0 clears it.  Takes
 * effect at the next forward; setting either grouping clears the other (any lseg_set_text_grouping call clears this one).
 * While set, lseg_forward_labels and lseg_forward_labels_conf run ONE batched forward and stream every image against its own rows
 * (csrc/corr_argmax.hip, the ragged instantiations; labels index the image's own list; a list of one label: label2 = -1, score2 = -inf)
 * under the conditions the shared set streams under: commuted schedule, out_c = 512, arch_option 0, no LSEG_CORR_GENERIC.  Everything
 * else in inference -- lseg_forward (logits, uint8 masks), lseg_forward_lowres, other widths, head blocks, split precision -- returns
 * LSEG_ERR_UNSUPPORTED before any kernel runs; nothing falls back.
 * Train mode (lseg_set_train) takes the lists too, on the fused-loss route only: lseg_forward with NO logits output, then lseg_train_loss /
 * lseg_backward with a target / lseg_backward_scaled.  dev_target int64 [B,H,W] holds, for image b, values in [0, host_counts[b]) or
 * ignore_index (anything else contributes no loss, as a target >= K does for a shared set); the loss is sum(nll) / sum(valid pixels) over
 * the batch, each image's softmax over its OWN labels, BatchNorm on the whole batch; lseg_train_loss' counts are {correct, labeled} of
 * the batch.  Any out_c % 64 == 0 up to 1024.  A logits output, the d(logits) hand-over of lseg_backward, arch_option 1/2 and the
 * ResNet-101 tower (flags bit 6) return LSEG_ERR_UNSUPPORTED before any kernel runs; lseg_forward_stats
 * and lseg_episode_stats after such a forward return LSEG_ERR_STATE.  A forward whose B differs from the B given here, or whose K differs
 * from the sum of the counts, returns LSEG_ERR_INVALID.  Afterwards the state is that of a streamed forward: lseg_forward_stats and the
 * "lowres" tap return LSEG_ERR_STATE.  Text cache, external text features, the overflow sentinel and profiling are unchanged. */
int lseg_set_text_groups(lseg_handle h, const int32_t* host_counts, int B);

/* ---- forward -----------------------------------------------------------------------
 * replaces: LSeg.forward(x, labelset) (lseg_net.py:160-205).
 *   dev_x          fp32 [B,3,img_h,img_w] NCHW, normalised like lseg_module.py:37-50
 *   dev_logits_out fp32 [B,K,img_h,img_w], caller-allocated, freshly written (the caller
 *                  may mutate it afterwards: encoding_models.py:138).  May be NULL.
 *   dev_argmax_out uint8 [B,img_h,img_w]: the mask = argmax over the labels of the output logits (first maximum wins, like
 *                  torch.max(pred, 1) at lsegmentation_module.py:114-117), computed from the low-resolution logits through the
 *                  x2 bilinear on the fly; optional, may be NULL.  With dev_logits_out == NULL the full-resolution logits
 *                  (138 MB per image at K = 150) are never materialised.  K <= 256. */
int lseg_forward(lseg_handle h, const float* dev_x, int B, float* dev_logits_out,
                 uint8_t* dev_argmax_out, void* stream);

/* Decoded images in: the input format of EVERY forward entry (lseg_forward*, lseg_forward_lowres, lseg_forward_features, inference and
 * train mode alike) is engine state.  Default: fp32 NCHW, normalised by the caller, as documented above.
 * replaces: transforms.ToTensor() + transforms.Normalize(mean, std) (lseg_module.py:37-50) in front of LSeg.forward.
 *   enabled != 0: dev_x of the forward entries is read as `const uint8_t*` [B,img_h,img_w,3] -- HWC, RGB, densely packed, 16-byte
 *                 aligned -- and the first stage (the patch-embedding operand pack, or the ResNet-101 stem) computes
 *                 (float(v) / 255 - mean[c]) / std[c] per value in fp32, torch's operations in torch's order, each correctly rounded.
 *                 Every output is bit-identical to the same entry fed the tensor ToTensor + Normalize produce on the host.
 *   enabled == 0: fp32 NCHW again; host_mean3 / host_std3 are not read (may be NULL).
 * The pointer's type is not checked (it cannot be): the caller states the format here and passes matching memory.
 * Errors: a NULL or non-finite mean / std, std[c] == 0: LSEG_ERR_INVALID (checked before the handle).  image_dtype LSEG_F16_SPLIT
 * (its first stage reads fp32 only) and a ViT patch size that is no multiple of 16: LSEG_ERR_UNSUPPORTED; the format stays as it was. */
int lseg_set_input_u8(lseg_handle h, int enabled, const float* host_mean3, const float* host_std3);

/* Masks for any K <= 32767 without the logits in memory.
 * replaces: LSeg.forward (lseg_net.py:160-205) through the correlation of lseg_net.py:194-203 AND the caller's torch.max(pred, 1)
 *   (lsegmentation_module.py:114-117) -- the [B,K,img_h,img_w] logits (922 MB per image at K = 1000) are neither written nor read.
 *   dev_label_out int16 [B,img_h,img_w]: arg-max over the labels of exactly the logits lseg_forward would have written (first maximum
 *                  wins); with per-image label sets the index within the image's own k labels
 *   dev_score_out  fp32 [B,img_h,img_w]: the winning logit; optional, may be NULL
 * On the commuted schedule with one shared label set, out_c = 512 and arch_option 0 the labels are STREAMED (csrc/corr_argmax.hip: text
 * panels through LDS, a running (best, label) pair per output pixel).  Every other configuration (other widths, head blocks, per-image
 * label sets, the split-precision mode, LSEG_CORR_GENERIC) forms the low-resolution logits as lseg_forward does and takes the arg-max
 * through the x2 bilinear on the fly, like dev_argmax_out.  Text cache / external text features, the overflow sentinel and flags bit 2
 * behave as in lseg_forward.  After a STREAMED forward no low-resolution logits exist: lseg_forward_stats and the "lowres" tap return
 * LSEG_ERR_STATE until another forward has run.  K > 32767, train mode: LSEG_ERR_UNSUPPORTED. */
int lseg_forward_labels(lseg_handle h, const float* dev_x, int B, int16_t* dev_label_out, float* dev_score_out, void* stream);

/* lseg_forward_labels with a confidence: the runner-up and the log-sum-exp over all labels beside the arg-max, still without the logits.
 * replaces: torch.topk(pred, 2, 1) and torch.logsumexp(pred, 1) on the logits of lseg_net.py:194-203 (what a caller needs for the softmax
 *   probability of the winner, exp(score - lse), and the top-2 margin, score - score2) -- the [B,K,img_h,img_w] logits are not written.
 *   dev_label_out / dev_score_out: as in lseg_forward_labels, bit for bit
 *   dev_label2_out int16, dev_score2_out fp32 [B,img_h,img_w]: the largest logit among the labels != label and its label; equal values go
 *                  to the lower label, so (label, label2) are entries 0 and 1 of a stable descending sort over the labels and a later
 *                  label that EQUALS the winner is the runner-up.  One label (K = 1, or one label per image): label2 = -1, score2 = -inf
 *   dev_lse_out    fp32 [B,img_h,img_w]: log(sum_k exp(logit_k)), accumulated online in fp32 as score + log(sum_k exp(logit_k - running max))
 * Each of the last three may be NULL.  Streamed under the conditions of lseg_forward_labels (csrc/corr_argmax.hip, the CONF instantiation:
 * the running state grows from (best, label) to (best, second, both labels, sum)); every other configuration reduces the low-resolution
 * logits through the x2 bilinear on the fly.  State rules and errors as for lseg_forward_labels: after a STREAMED forward no
 * low-resolution logits exist; K > 32767 and train mode: LSEG_ERR_UNSUPPORTED; a NULL x or label output: LSEG_ERR_INVALID. */
int lseg_forward_labels_conf(lseg_handle h, const float* dev_x, int B, int16_t* dev_label_out, float* dev_score_out, int16_t* dev_label2_out,
                             float* dev_score2_out, float* dev_lse_out, void* stream);

/* lseg_forward_labels with the cross-entropy against a target mask, still without the logits: the validation step's loss, pixAcc and IoU
 * for any label set -- one shared set of any K <= 32767, or the per-image lists of lseg_set_text_groups -- in one forward.
 * replaces: the criterion's value nn.CrossEntropyLoss(ignore_index)(pred, target) (lsegmentation_module.py:72) and batch_pix_accuracy +
 *   batch_intersection_union on torch.max(pred, 1)[1] (:49-50,59-60) -- the [B,K,img_h,img_w] logits are neither written nor read.
 *   dev_target       int64 [B,img_h,img_w]; with per-image lists image b's values index its own list.  A pixel is VALID iff target !=
 *                    ignore_index and 0 <= target < K (per-image lists: < the image's own count) -- the rule of lseg_op_stats_finish's
 *                    d_nll and of the ragged training loss
 *   dev_label_out / dev_score_out: as in lseg_forward_labels, bit for bit
 *   dev_lse_out      fp32 [B,img_h,img_w]: as in lseg_forward_labels_conf, bit for bit (the same online sum)
 *   dev_nll_plane_out fp32 [B,img_h,img_w]: lse - logit[target] per valid pixel, 0 elsewhere
 *   dev_nll          double [2] = {sum over the valid pixels of double(lse) - double(logit[target]), number of valid pixels}: the layout of
 *                    lseg_forward_stats' dev_nll; fixed-order partials, no atomics -- two calls on the same input give the same bits
 *   dev_counts       int64: filled exactly as lseg_op_label_stats (accumulate = 0, no class map) fills it from dev_label_out and dev_target:
 *                    [2+3K] for one shared set (K = labels per image with lseg_set_text_grouping), {correct, labeled} + the three
 *                    concatenated areas [2 + 3 sum of counts] for per-image lists
 * Every output but dev_label_out may be NULL.  Streamed under the conditions of lseg_forward_labels (csrc/corr_argmax.hip, the LOSS
 * instantiation: the target's logit is kept when its label passes through the registers; a label part of the split keeps -inf unless it
 * holds the target, the merge takes the max); the configurations lseg_forward_labels_conf reduces from the low-resolution logits (other
 * widths, head blocks, a fixed number of labels per image, LSEG_CORR_GENERIC) are reduced from them here too, with the same outputs; the
 * per-image lists stay refused where lseg_forward_labels refuses them.  State rules and errors as for lseg_forward_labels_conf; a NULL
 * target: LSEG_ERR_INVALID; train mode: LSEG_ERR_UNSUPPORTED (lseg_train_loss has the loss there). */
int lseg_forward_labels_loss(lseg_handle h, const float* dev_x, int B, const int64_t* dev_target, int ignore_index, int16_t* dev_label_out,
                             float* dev_score_out, float* dev_lse_out, float* dev_nll_plane_out, double* dev_nll, int64_t* dev_counts,
                             void* stream);

/* The logits BEFORE scratch.output_conv (lseg_net.py:203), for callers that read them through the x2 bilinear themselves (the
 * multi-scale evaluator's lseg_op_eval_accumulate_lowres): the inference forward exactly as lseg_forward runs it -- text cache, external
 * text features, per-image label sets (Kout = labels per image), overflow sentinel, profiling and the arch_option 1/2 head blocks
 * included -- with no [B,K,img_h,img_w] tensor written.
 *   dev_low_out    fp32 [B, Kout, img_h/2, img_w/2]: lseg_op_upsample2x_planes of it is bit-identical to the logits lseg_forward writes
 *                  for the same input (34.6 MB per image at K = 150, crop 480, instead of 138 MB)
 * On the commuted schedule without head blocks the planes are formed straight in dev_low_out; the other schedules hold them in engine
 * memory and copy them out.  Afterwards the engine is in the state an lseg_forward leaves: lseg_forward_stats, lseg_episode_stats and
 * the "lowres" tap work.  Train mode: LSEG_ERR_UNSUPPORTED; a NULL output: LSEG_ERR_INVALID. */
int lseg_forward_lowres(lseg_handle h, const float* dev_x, int B, float* dev_low_out, void* stream);

/* Label panels over held image features: run the image tower once, keep what the correlation reads, score any slice of the label set
 * from it later (the multi-scale evaluator's BatchedMultiEval.forward_labels: peak memory set by the panel, not by K).
 *   lseg_features_bytes    the sizes of the two held buffers for B images at the engine's img_h / img_w: feat fp16
 *                          [B, img_h/4 + 2, img_w/4 + 2, out_c] (the head feature map g before the x2 upsample, padded NHWC: 15.2 MB per
 *                          480 x 480 image) and scale fp32 [B, img_h/2, img_w/2] (logit_scale / ||up(g)|| per low-resolution pixel)
 *   lseg_forward_features  the inference forward of lseg_forward through the commuted head GEMM, the cell dot products and the scale
 *                          plane, then both copied into the caller's buffers device to device.  No text is read (no label set needs to be
 *                          set); the dot products always come from the stand-alone kernel -- the route lseg_forward_lowres takes for
 *                          K > 157 -- whatever K is set.  Overflow sentinel and profiling as in lseg_forward.
 *   lseg_score_features    dev_low_out fp32 [B, rows, img_h/2, img_w/2] = the low-resolution logits (lseg_forward_lowres' output) of text
 *                          rows [row0, row0 + rows) of the CURRENT label set for the held images: the generic correlation GEMM on that
 *                          slice of the text matrix, then the scaled x2 upsample with the held scale plane.  The text is encoded first
 *                          under the rules of lseg_forward (text cache, external text features).  For a label set lseg_forward_lowres
 *                          runs on the same route (K > 157 at out_c = 512, or LSEG_CORR_GENERIC) plane row0 + j equals its plane
 *                          row0 + j bit for bit, for any row0 and rows: an output element is one chain of MFMAs over the 512 channels
 *                          in ascending order whatever tile the row count picks, and nothing is split.  For smaller label sets the two
 *                          differ in the last bits of the scale plane (the fused kernel's dot products).  Buffers 16-byte aligned.
 * Both are accepted where the commuted correlation runs: the commuted schedule (no debug taps, no split precision), arch_option 0, an
 * even img_w/4, no LSEG_CORR_FULLRES, one label set shared by the batch, inference mode (any out_c the engine accepts: at widths other
 * than 512 lseg_forward_lowres takes the generic route for every K, so the planes are bit-identical for every K); per-image label sets of either
 * kind, train mode and everything else return LSEG_ERR_UNSUPPORTED before any kernel runs -- nothing falls back.  rows < 1 or
 * row0 + rows > K: LSEG_ERR_INVALID; B outside [1, max_batch]: LSEG_ERR_INVALID.  Afterwards the engine is in the state of a streamed
 * forward: lseg_forward_stats, lseg_episode_stats and the "lowres" tap return LSEG_ERR_STATE until another forward has run. */
int lseg_features_bytes(lseg_handle h, int B, size_t* feat_bytes, size_t* scale_bytes);
int lseg_forward_features(lseg_handle h, const float* dev_x, int B, void* dev_feat_out, float* dev_scale_out, void* stream);
int lseg_score_features(lseg_handle h, const void* dev_feat, const float* dev_scale, int B, int row0, int rows, float* dev_low_out,
                        void* stream);

/* The metric / loss step after the path, without the full-resolution logits: statistics of the LAST lseg_forward's output against a
 * target mask -- replaces batch_pix_accuracy + batch_intersection_union on `pred` (lsegmentation_module.py:49-50,59-60) and the value
 * of the criterion (:72).  dev_target int64 [B,img_h,img_w]; dev_counts / dev_nll as in lseg_op_seg_stats. */
int lseg_forward_stats(lseg_handle h, const int64_t* dev_target, int ignore_index, int64_t* dev_counts, double* dev_nll, void* stream);

/* The few-shot episode evaluation of the zero-shot networks on the LAST lseg_forward's output (csrc/episode.hip) -- replaces
 * Evaluator.classify_prediction(out.argmax(1), target, ignore) (fewshot_data/common/evaluation.py:12-39), AverageMeter.update
 * (fewshot_data/common/logger.py:29-34) and the value of the 2-class criterion (lsegmentation_module_zs.py:338-343) as
 * test_lseg_zs.py:289-312 and LSegmentationModuleZS.training_step / validation_step (:100-143, :157-192) call them.  Reads the
 * (img_h/2, img_w/2) logits wherever the forward left them (an inference forward or a train-mode one: the sources of lseg_forward_stats
 * and lseg_train_loss) through output_conv's x2 bilinear on the fly; the workspace is the engine's own scratch.  Arguments and outputs
 * as lseg_op_episode_stats.  LSEG_ERR_STATE after lseg_forward_labels or before any forward; LSEG_ERR_INVALID unless the last forward
 * had exactly 2 labels per image (labels_per_image = 2, or one shared label set with K = 2). */
int lseg_episode_stats(lseg_handle h, const int64_t* dev_target, const uint8_t* dev_ignore, int ignore_index, const int64_t* dev_class_id,
                       int nclass, int64_t* dev_inter_buf, int64_t* dev_union_buf, int64_t* dev_areas, double* dev_nll, int64_t* dev_flags,
                       void* stream);

/* Intermediate taps for parity tests (names: "act1".."act4", "layer1".."layer4",
 * "rn1".."rn4", "path1".."path4", "image_features", "lowres").  Copies the tensor in the oracle's layout
 * ([B,N,D] / NCHW fp32) into dev_out; *n_elems gets the element count. */
int lseg_get_intermediate(lseg_handle h, const char* name, float* dev_out, size_t cap_elems,
                          size_t* n_elems, void* stream);
/* Debug mode keeps fp32 snapshots of the 4 hooked block outputs ("act1".."act4", the
 * reference's forward hooks at lseg_vit.py:12-16,421-424) during lseg_forward. */
int lseg_set_debug(lseg_handle h, int enabled);

/* ---- measurement -------------------------------------------------------------------
 * Per-kernel-family HIP-event timing on the engine's stream (bench.py roofline leg).
 * family names, in mask-bit order: "forward" (bit 0), "mlp_fc1", "mlp_fc2", "attn_proj", "attn_qkv", "attention", "layernorm" (the
 * ViT block's kernels: timm vision_transformer.py Block, invoked from lseg_vit.py:196-197).  lseg_set_profiling(h, 1) = forward +
 * mlp_fc1; any other non-zero value is a bit mask over the families; 0 switches the events off.  Events for 64 forwards are created
 * by the call, outside any timed region.  flops_per_launch = 2MNK of the family's GEMM (4 N^2 D per image for attention). */
int lseg_set_profiling(lseg_handle h, int enabled);
/* Range check of the image tower's 16-bit activations (every 16-bit activation buffer of the plan, as the forwards so far left them):
 * host_out4[0] = non-finite values (fp16 operands overflow at 65504 -- the reference's tower is fp32, lseg_vit.py:196-197, and cannot),
 * [1] = finite values with |x| >= 2^15, [2] = the largest finite |x| (fp32 bit pattern), [3] = elements scanned.  Synchronises the
 * stream.  The Python mirror runs it once after every (re)pack of an fp16 engine and falls back to bf16 loudly when [0] > 0. */
int lseg_check_range(lseg_handle h, uint64_t* host_out4, void* stream);
/* The always-on companion of lseg_check_range: every inference lseg_forward raises a device flag when the head feature map carries an inf / NaN
 * (any non-finite value of the 16-bit image tower ends up there) and copies it to pinned host memory behind the forward.  This call never
 * synchronises: it returns 1 once a COMPLETED forward was flagged (sticky until `reset`), else 0 -- i.e. an overflow on image n is seen at the
 * latest when image n+1 is submitted.  The Python mirror falls back to bf16 operands loudly on it (fp16 saturates at 65504; the reference's
 * tower is fp32, lseg_vit.py:196-197). */
int lseg_overflow_seen(lseg_handle h, int reset);
int lseg_get_profile(lseg_handle h, const char* family, double* total_ms, int64_t* launches,
                     double* flops_per_launch);

/* ---- single-operator entry points (unit parity tests call these through the ABI) --
 * All tensors are device pointers; dtype codes are lseg_dtype. */

/* C[M,N] = act(A[M,K] @ W[N,K]^T + bias) (+ residual); A,W: bf16 or fp16 (`ab_dtype`),
 * bias fp32 [N] or NULL, residual fp32 [M,N] or NULL, C: out_dtype.  act: 0 none,
 * 1 GELU(erf), 2 QuickGELU, 3 ReLU.   (timm Linear / CLIP Linear / 1x1 conv) */
int lseg_op_gemm(const void* d_A, const void* d_W, const float* d_bias, const float* d_residual,
                 void* d_C, int M, int N, int K, int ab_dtype, int out_dtype, int act, void* stream);
/* The four GEMM forms of a timm Block (lseg_vit.py:196-197 -> [3P] timm Block / Attention / Mlp) on the engine's specialised epilogues,
 * standalone: kind 0  C = T(A W^T + b)  (T = ab_dtype);  1  C = T(gelu(A W^T + b))  (mlp.fc1);  2  C += A W^T + b on an fp32 C (the residual
 * stream: attn.proj, mlp.fc2; d_Cq is read and written);  3  the qkv Linear with timm's reshape/permute folded into the store: d_Cq = q and
 * d_Ck = k as [B*heads, npad, 64], d_Cv = v TRANSPOSED [B*heads, 64, npad] (N = 3*heads*64, M = B*ntok, pad rows untouched).
 * max_grid > 0 caps the persistent grid (tools/epilogue_table.py).  d_bias fp32 [N] is required. */
int lseg_op_gemm_vit(const void* d_A, const void* d_W, const float* d_bias, void* d_Cq, void* d_Ck, void* d_Cv, int M, int N, int K,
                     int ab_dtype, int kind, int ntok, int npad, int max_grid, void* stream);
/* One GEMM of the family the engine launches, described the way its schedules describe it (csrc/engine.h: lin_args, add_residual, qkv_args,
 * pixshuf_args, to_periodic_rows), with the launcher's tools-only knobs exposed: the operator tests reach every epilogue, tile and schedule
 * at small shapes through it (tests/test_gpu_gemm_family.py).  A [M, K] and W [N, K] are row-major 16-bit operands of ab_dtype, bias fp32 [N]
 * ([ch] for form 2) or NULL (form 0 only).
 *   form 0  linear: C [M, N] = out_dtype(act(A W^T + bias) [+ residual [M, N] of res_dtype]); act 0 none, 1 GELU, 3 ReLU.  nsplit > 1: split-K,
 *           slab s = C + s * c_split_stride (fp32 elements) holds the partial product over K-steps [s * split_steps, (s + 1) * split_steps) of
 *           64; needs bias == residual == NULL and ranges that tile K / 64 exactly.
 *   form 1  qkv: N = 3 * heads * 64, K = heads * 64, M = B * ntok; C = q and Ck = k as [B * heads, npad, 64], Cv = v^T [B * heads, 64, npad],
 *           pad tokens untouched; qscale != 0 multiplies q before its single rounding.
 *   form 2  ConvTranspose2d(kernel = stride = s) as a GEMM: rows m = (b, y, x) on the (ho, wo) grid, columns n = (i * s + j) * ch + co; C is the
 *           padded NHWC map [B, ho * s + 2, wo * s + 2, ch], whose one-pixel border is untouched; bias fp32 [ch].
 *   form 3  periodic rows (the patch embedding): rows m = (b, r), r < p_div, land in row b * p_mul + r + p_off of C [*, N] and add row
 *           r + p_off of residual [*, ldr] (res_dtype).
 * tag 0 | 1: the two symbols of the GELU epilogue.  tile 0: the launcher's cost model; 1 = 64x64, 2 = 128x128, 6 = 256x256 (taken when the
 * epilogue has that instantiation and N % 256 == 0, else 128x128).  max_grid: 0 or a multiple of 8, caps the persistent grid.
 * LSEG_ERR_INVALID / LSEG_ERR_UNSUPPORTED before anything is launched: a NULL required pointer, a shape that does not fit the form, whatever
 * launch_gemm refuses (K % 64, split-K ranges that do not tile K, qscale without the specialised qkv epilogue, ...). */
typedef struct lseg_gemm_case {
    int form;
    const void* A; const void* W; const float* bias; const void* residual;
    void* C; void* Ck; void* Cv;
    int M, N, K, ab_dtype, out_dtype, res_dtype, act;
    int tag, tile, max_grid;
    int nsplit, split_steps; size_t c_split_stride;
    int ntok, npad, heads; float qscale;          /* form 1 */
    int ho, wo, s, ch;                            /* form 2 */
    int p_div, p_mul, p_off, ldr;                 /* form 3 */
} lseg_gemm_case;
int lseg_op_gemm_ex(const lseg_gemm_case* c, void* stream);
/* What that launch decides on a device of `cus` compute units, host only (no device needed, the pointers are only looked at for their
 * alignment): out4 = {epilogue id (0 generic, 1 LIN16, 2 LIN16_GELU, 3 RES32, 4 QKV16, 6 LIN16_F16, 7 PIX16, 8 PART32, 11 LIN32),
 * tile (1 | 2 | 6), workgroups, most work items ((tile, K-range) pairs) one workgroup walks}.  Refuses what lseg_op_gemm_ex refuses. */
int lseg_op_gemm_ex_plan(const lseg_gemm_case* c, int cus, int* out4);
/* The residual form alone -- d_C (fp32 [rows_alloc, N], rows_alloc >= M) += A W^T + bias, in place: attn.proj / mlp.fc2 of a timm Block
 * (lseg_vit.py:196-197) -- with the caller stating how many rows of d_A and d_C are ALLOCATED.  When they reach the next multiple of 256
 * the launch takes the hand-scheduled 256 x 128 kernel (csrc/gemm_asm.hip: whole tiles, no masks; rows >= M of d_C are overwritten with
 * values nobody should read); impl = 0 forces the generic kernel family, 1 requires the hand-scheduled one (LSEG_ERR_UNSUPPORTED when the
 * shape does not qualify), -1 lets the launcher choose like the engine does.  max_grid > 0 caps the persistent grid. */
int lseg_op_gemm_res32(const void* d_A, const void* d_W, const float* d_bias, float* d_C, int M, int N, int K, int rows_alloc,
                       int ab_dtype, int impl, int max_grid, void* stream);
/* Column reductions of the training step, standalone (the bias gradients of every Linear / conv and the BatchNorm batch statistics of
 * the DPT residual units: autograd of nn.Linear / nn.Conv2d / nn.BatchNorm2d under modules/lsegmentation_module.py:66-81).
 *   lseg_op_colsum:       d_out[c] (+)= sum_r in[r, c], in 16-bit [R, ld] row-major, C <= ld columns, fp32 out
 *   lseg_op_bn_stats:     d_stats[c] = sum x, d_stats[C + c] = sum x^2 over a padded NHWC map [B, H+2, W+2, C] (zero border)
 *   lseg_op_bn_bwd_stats: d_bstats[c] = sum dy, d_bstats[C + c] = sum dy (x - mean_c) rstd_c, mean / rstd from d_stats over `count` = B H W
 * d_det_ws (optional, det_cap_floats floats): the DETERMINISTIC form (lseg_config.flags bit 3) -- one partial row per row block, summed in
 * a fixed order -- instead of fp32 atomics.  Same values up to summation order; two runs of the deterministic form are bit-identical. */
int lseg_op_colsum(const void* d_in, int dtype, float* d_out, int R, int C, int ld, int accumulate, float* d_det_ws, size_t det_cap_floats,
                   void* stream);
int lseg_op_bn_stats(const void* d_x_padded, float* d_stats, int B, int H, int W, int C, int dtype, float* d_det_ws, size_t det_cap_floats,
                     void* stream);
int lseg_op_bn_bwd_stats(const void* d_dy_padded, const void* d_x_padded, const float* d_stats, float* d_bstats, int B, int H, int W, int C,
                         float eps, int dtype, float* d_det_ws, size_t det_cap_floats, void* stream);
/* LayerNorm over the last dim: in fp32|fp16 [M,D] -> out bf16|fp16 [M,D] */
int lseg_op_layernorm(const void* d_in, int in_dtype, const float* d_gamma, const float* d_beta,
                      void* d_out, int out_dtype, int M, int D, float eps, void* stream);
/* softmax(Q K^T * scale [+causal]) V for head_dim 64.
 * q,k: [BH, Npad, 64]; vt: [BH, 64, Npad] (V transposed); out: [B, Ntok, H*64]. */
int lseg_op_attention(const void* d_q, const void* d_k, const void* d_vt, void* d_out,
                      int B, int H, int Ntok, int Npad, int dtype, int causal, float scale,
                      void* stream);
/* The same product for a q that already carries softmax scale * log2(e) (the inference engine folds it into the qkv Linear's epilogue,
 * one rounding): out = softmax2(Q' K^T) V with softmax2 in base 2, no mask.  d_lse2 (optional, fp32 [B*H, Npad]) receives log2 sum_k
 * 2^(q'.k).  Same layouts as lseg_op_attention. */
int lseg_op_attention_prescaled(const void* d_q, const void* d_k, const void* d_vt, void* d_out, float* d_lse2,
                                int B, int H, int Ntok, int Npad, int dtype, void* stream);
/* Both of the above through one entry, the engine's launcher as it is: prescaled = 0 (scale applied to the scores, optional causal mask)
 * or 1 (q carries scale * log2(e), `scale` ignored, no causal form: LSEG_ERR_UNSUPPORTED).  d_lse2 (optional, fp32 [B*H, Npad]) receives
 * log2 sum_k 2^(s_k scale log2(e)) over the unmasked keys of each query row -- what the training step saves for the backward.
 * Refused: Npad % 128 != 0 or Npad < Ntok, dtype LSEG_F32, NULL q / k / vt / out, B, H or Ntok < 1.
 *
 * PADDING CONTRACT of the forward (rows Ntok .. Npad-1 of q and k, columns Ntok .. Npad-1 of every vt row), read from csrc/attention.hip:
 *   q    padded rows: any finite value.  They are loaded by the lanes of a partly filled wave; nothing computed from them is stored.
 *        (Pre-scaled form: a padded row can fire its wave's refresh of the reference maximum, which moves the roundings of the wave's
 *        real rows within their error bound; the plain form's outputs do not depend on the padding bit for bit.)
 *   k    padded rows: any finite value.  Their scores are replaced by -inf before the row maximum is taken.
 *   vt   padded columns: any finite value.  They meet a probability of exactly 0 in the P V product (0 x finite = 0; an inf or NaN there
 *        would poison the row).
 *   out  [B, Ntok, H*64] has no padding: every element is written.
 *   lse2 rows < Ntok of every head are written; rows Ntok .. Npad-1 are LEFT UNWRITTEN (they keep what the caller put there). */
int lseg_op_attention_ex(const void* d_q, const void* d_k, const void* d_vt, void* d_out, float* d_lse2, int B, int H, int Ntok, int Npad,
                         int dtype, int causal, float scale, int prescaled, void* stream);
/* What that launch decides on a device of `cus` compute units, host only (no device needed): out6 = {waves per workgroup (2 | 4; a
 * workgroup owns 32 x waves query rows of one head), query blocks per head, workgroups, 64-key tiles the last query block walks,
 * 1 when the head -> XCD map applies (B * H % 8 == 0) else 0, dynamic LDS bytes (two stages of a K and a V^T tile)}.
 * Refused: B, H, Ntok or cus < 1, prescaled with causal (LSEG_ERR_UNSUPPORTED), NULL out6. */
int lseg_op_attention_plan(int B, int H, int Ntok, int causal, int prescaled, int cus, int* out6);
/* The split-precision ("strict") forward: every operand is a pair of fp16 planes, x = hi + lo, the lo plane `*_plane` ELEMENTS behind the
 * hi plane (q and k share qk_plane); softmax(Q K^T scale) V in fp32, no mask; out [B, Ntok, H*64] written as hi and lo planes.
 * Padded rows / columns of q, k, vt are never read (any value, finite or not).  Refused: NULL q / k / vt / out, B, H or Ntok < 1. */
int lseg_op_attention_strict(const void* d_q, const void* d_k, const void* d_vt, void* d_out, size_t qk_plane, size_t vt_plane,
                             size_t out_plane, int B, int H, int Ntok, int Npad, float scale, void* stream);
/* 3x3 conv, NHWC, zero-padded borders: in [B,H+2,W+2,Cin] (bf16, border = 0) ->
 * out [B,Ho+2,Wo+2,Cout] interior written; w_packed [Cout, 9*Cin] bf16 (tap-major).
 * stride 1|2, relu_in / relu_out flags, bias fp32 [Cout] or NULL, residual (same
 * geometry as out, bf16) or NULL. */
int lseg_op_conv3x3(const void* d_in, const void* d_w_packed, const float* d_bias,
                    const void* d_residual, void* d_out, int B, int H, int W, int Cin, int Cout,
                    int stride, int relu_in, int relu_out, void* stream);
/* ResNet-101 tower operators (lseg_config.flags bit 5), dtype LSEG_BF16 | LSEG_F16 for every 16-bit map:
 *   lseg_op_rn_stem     conv1 7x7 / 2, pad 3, 3 -> 64 channels, + bias + ReLU, fp32 accumulation: d_x fp32 NCHW [B,3,H,W] (H, W even) ->
 *                       d_out padded NHWC [B,H/2+2,W/2+2,64] (interior written).  d_w fp32 [147][64] (tap k = (ci*7 + ky)*7 + kx, the
 *                       BatchNorm folded in), d_bias fp32 [64].
 *   lseg_op_rn_maxpool  max-pool 3x3 / 2, pad 1 of a padded NHWC map of NON-NEGATIVE values [B,H+2,W+2,C] (zero border) ->
 *                       [B,H/2+2,W/2+2,C] interior; bit-exact (C % 8 == 0).
 *   lseg_op_conv        1x1 (ksize 1, pad 0, w_packed [Cout, Cin]) or 3x3 (ksize 3, pad 1, w_packed [Cout, 9*Cin] tap-major) conv,
 *                       stride 1|2, on padded NHWC maps as lseg_op_conv3x3, bias fp32 [Cout] or NULL, residual (geometry of out) or
 *                       NULL; relu_out applies ReLU, BEFORE the residual add (relu_after_res = 0, the DPT units' order) or AFTER it
 *                       (relu_after_res = 1: relu(conv + bias + residual), the bottleneck's).  Cin % 64 == 0.
 *   lseg_op_bn_apply_res  train-mode BatchNorm of the tower (flags bit 6) from batch sums, one streaming pass over a padded NHWC map
 *                       [B,H+2,W+2,C] (C % 8 == 0; interior written, the zero border untouched): d_y = [relu](bn(d_x) + r), bn(x) =
 *                       gamma (x - mean) / sqrt(var + eps) + beta with mean / BIASED var from d_stats fp32 [2C] = {sum x, sum x^2} over
 *                       the B H W pixels (lseg_op_bn_stats).  r = 0 (d_res_pad NULL), the plain map d_res_pad (d_res_stats NULL: the
 *                       identity of a bottleneck), or bn_r(d_res_pad) from d_res_stats / d_res_gamma / d_res_beta (the downsample branch
 *                       of a stage's first block).  d_y_pad may be d_x_pad (in place) and d_res_pad may be d_y_pad. */
int lseg_op_bn_apply_res(const void* d_x_pad, void* d_y_pad, const float* d_stats, const float* d_gamma, const float* d_beta, const void* d_res_pad,
                         const float* d_res_stats, const float* d_res_gamma, const float* d_res_beta, int B, int H, int W, int C, float eps,
                         int relu, int dtype, void* stream);
int lseg_op_rn_stem(const float* d_x, const float* d_w, const float* d_bias, void* d_out, int B, int H, int W, int dtype, void* stream);
/* lseg_op_rn_stem from a uint8 [B,H,W,3] image (csrc/input_u8.hip): the normalisation of lseg_set_input_u8 fused into the read; the
 * output equals lseg_op_rn_stem's on the torch-normalised fp32 tensor bit for bit.  Pointers 16-byte aligned, H and W even.  Arguments
 * are checked before the device is touched. */
int lseg_op_rn_stem_u8(const uint8_t* d_x, const float* d_w, const float* d_bias, void* d_out, int B, int H, int W, int dtype,
                       const float* host_mean3, const float* host_std3, void* stream);
/* The patch-embedding GEMM's operand rows (lseg_vit.py:179, the conv as an im2col gather): d_A 16-bit [B*(H/P)*(W/P), 3*P*P], column
 * k = c*P*P + i*P + j, from the fp32 NCHW image (P % 8 == 0) or, _u8, from a uint8 [B,H,W,3] image with the normalisation of
 * lseg_set_input_u8 fused in (P % 16 == 0; bit-equal to the fp32 form on the torch-normalised tensor).  dtype LSEG_BF16 | LSEG_F16,
 * pointers 16-byte aligned, H and W multiples of P.  Arguments are checked before the device is touched. */
int lseg_op_patch_rows(const float* d_x, void* d_A, int B, int H, int W, int P, int dtype, void* stream);
int lseg_op_patch_rows_u8(const uint8_t* d_x, void* d_A, int B, int H, int W, int P, int dtype, const float* host_mean3,
                          const float* host_std3, void* stream);
int lseg_op_rn_maxpool(const void* d_in, void* d_out, int B, int H, int W, int C, int dtype, void* stream);
int lseg_op_conv(const void* d_in, const void* d_w_packed, const float* d_bias, const void* d_residual, void* d_out, int B, int H, int W,
                 int Cin, int Cout, int ksize, int stride, int relu_out, int relu_after_res, int dtype, void* stream);
/* One implicit-GEMM conv of the family the engine launches, described the way Engine::conv3x3 describes it, with the launcher's tools-only
 * knobs exposed: the operator tests reach every conv tile, epilogue and schedule at small shapes through it (tests/test_gpu_conv_family.py).
 * in: padded NHWC [B, H+2, W+2, Cin] (the border is READ: it is the conv's padding, zero in the engine); w [Cout, taps * Cin] tap-major
 * (taps = 9 for ksize 3, pad 1; 1 for ksize 1, pad 0, which reads the interior only); out: padded NHWC [B, Ho+2, Wo+2, Cout], interior
 * written, Ho = (H - 1) / stride + 1.  out = T(relu?(conv(relu_in ? relu(in) : in) + bias) + residual + residual2), or with relu_after_res
 * T(relu(conv + bias + residual [+ residual2])); residual / residual2 have the geometry and type of out (out may alias residual).
 * out_relu (optional, geometry of out): the stored out with its negative halves cleared (-0 -> +0); needs the specialised padded-NHWC
 * epilogue (Cout % 128 == 0, a bias, 16-byte aligned maps), refused otherwise.  relu_in is implemented for bf16 and fp16 alike.
 * nsplit > 1: the split-K form Engine::conv3x3 launches at small batch: out = fp32 slabs, slab s = out + s * c_split_stride floats holds
 * the [B*Ho*Wo, Cout] partial product over K-steps [s * split_steps, (s + 1) * split_steps) of 64; no bias, residual, ReLU or out_relu.
 * tile 0: the launcher's cost model; 1 = 64x64, 2 = 128x128, 6 = 256x256.  max_grid: 0 or a multiple of 8, caps the persistent grid.
 * Every refusal (LSEG_ERR_INVALID / LSEG_ERR_UNSUPPORTED) comes before a device is asked for. */
typedef struct lseg_conv_case {
    const void* in; const void* w; const float* bias; const void* residual; const void* residual2;
    void* out; void* out_relu;
    int B, H, W, Cin, Cout, ksize, stride, dtype;
    int relu_in, relu_out, relu_after_res;
    int tile, max_grid;
    int nsplit, split_steps; size_t c_split_stride;
} lseg_conv_case;
int lseg_op_conv_ex(const lseg_conv_case* c, void* stream);
/* What that launch decides on a device of `cus` compute units, host only: out4 = {epilogue id (0 generic, 5 PAD16, 8 PART32), tile
 * (1 | 2 | 6), workgroups, most work items one workgroup walks}.  Refuses what lseg_op_conv_ex refuses. */
int lseg_op_conv_ex_plan(const lseg_conv_case* c, int cus, int* out4);
/* The split-K plan Engine::conv3x3 makes for a conv of M = B*Ho*Wo rows, N = Cout columns and K = taps * Cin with a slab workspace of
 * ws_floats floats, host only: *ns slabs of *steps K-steps of 64 (the last range possibly shorter); *ns = 1: the conv runs unsplit. */
int lseg_op_conv_splitk_plan(int M, int N, int K, size_t ws_floats, int* ns, int* steps);
/* The reduction behind a split-K conv: out (padded NHWC [B, Ho+2, Wo+2, C], interior written) = T(f(bias + sum of `ns` fp32 slabs
 * [B*Ho*Wo, C], `stride` floats apart)) with the ReLU / residual / residual2 / out_relu forms of lseg_op_conv_ex.  C % 8 == 0,
 * stride % 4 == 0, and d_part, d_res, d_res2, d_out, d_out_relu 16-byte aligned (the kernel moves 8 channels per access).  Argument refusals come before a device is asked for. */
int lseg_op_conv_reduce_pad(const float* d_part, int ns, size_t stride, const float* d_bias, const void* d_res, const void* d_res2, void* d_out,
                            void* d_out_relu, int B, int Ho, int Wo, int C, int relu, int relu_after_res, int dtype, void* stream);
/* 3x3 conv weight gradient on the K-major operand path: d_dw fp32 [Cout, 9 * Cin] (tap-major) = sum over the padded pixels of
 * dy_pad[p, co] * f(x_pad)[p + tap shift, ci], f = ReLU when relu_x; dy_pad [B, H+2, W+2, Cout] with a ZERO border, x_pad [B, H+2, W+2, Cin].
 * d_ws: ws_floats floats of scratch for the split-K slabs -- its size bounds the slab count.  Returns the slab count (>= 1) or a negative
 * status; refused before anything is launched: Cin % 128 != 0, ws_floats < Cout * 9 * Cin. */
int lseg_op_conv_wgrad(const void* d_dy_pad, const void* d_x_pad, float* d_dw, int relu_x, int B, int H, int W, int Cin, int Cout, float* d_ws,
                       size_t ws_floats, int dtype, void* stream);
/* Linear weight gradient on the same path: d_dw fp32 [rows_out, cols_out] (+)= dy[:, :rows_out]^T x[:, :cols_out] over the M rows of
 * dy [M, ldy] and x [M, ldx] (16-bit).  Refused before anything is launched: cols_out % 128 != 0, ws_floats < rows_out * cols_out. */
int lseg_op_wgrad_kmajor(const void* d_dy, int ldy, const void* d_x, int ldx, int M, int rows_out, int cols_out, float* d_dw, int accumulate,
                         float* d_ws, size_t ws_floats, int dtype, void* stream);
/* Weight packers, one launch each.  conv_dgrad_pack: wd[ci, t, co] = wp[co, 8 - t, ci] (16-bit, a permutation).  pack_conv3x3: w fp32
 * [Co, Ci, 3, 3] (+ eval BatchNorm fold when bn_w != NULL, + conv bias) -> wp [Co, 9, Cip] of dtype (fp32 allowed), channels ci >= Ci are NOT
 * written (the caller's zeros stay), bias_out fp32 [Co] (optional).  pack_conv1x1: w fp32 [Co, Ci] (+ BatchNorm fold when bn_w != NULL)
 * -> wp [Co, Ci], bias_out fp32 [Co] (zeros without BatchNorm). */
int lseg_op_conv_dgrad_pack(const void* d_wp, void* d_wd, int Co, int Ci, void* stream);
int lseg_op_pack_conv3x3(const float* d_w, const float* d_bn_w, const float* d_bn_b, const float* d_bn_m, const float* d_bn_v, float bn_eps,
                         const float* d_conv_bias, void* d_wp, float* d_bias_out, int Co, int Ci, int Cip, int dtype, void* stream);
int lseg_op_pack_conv1x1(const float* d_w, const float* d_bn_w, const float* d_bn_b, const float* d_bn_m, const float* d_bn_v, float bn_eps,
                         void* d_wp, float* d_bias_out, int Co, int Ci, int dtype, void* stream);
/* bilinear x2, align_corners=True, NHWC bf16: in [B,H+2,W+2,C] (padded) -> out [B,2H,2W,C] */
int lseg_op_upsample2x_nhwc(const void* d_in, void* d_out, int B, int H, int W, int C, void* stream);
/* bilinear x2, align_corners=True, NCHW fp32 planes: in [P,H,W] -> out [P,2H,2W]
 * (scratch.output_conv, lseg_net.py:203,219-221) */
int lseg_op_upsample2x_planes(const float* d_in, float* d_out, int P, int H, int W, void* stream);
/* The tail of the commuted head (DESIGN.md par. 3.4) in one pass: label planes R at the quarter resolution, d_in_padded fp32 [B*K, H+2, W+2]
 * (1-pixel border), per-pixel scale s/||u|| d_scale fp32 [B, 2H, 2W] -> logits d_out fp32 [B, K, 4H, 4W] =
 * output_conv(fp16(scale * bilinear_x2(R))) (lseg_net.py:194-196 rounding, :203 upsample).  two_stage != 0 runs the two materialising
 * kernels instead (d_low_scratch fp32 [B,K,2H,2W]): same bits.  LSEG_ERR_UNSUPPORTED for an odd W and for a W whose row band does not
 * fit the 160 KB LDS (184 bytes per column in one pass: W <= 890; 32 in the two-stage form). */
int lseg_op_upsample4x_planes_scaled(const float* d_in_padded, const float* d_scale, float* d_out, int B, int K, int H, int W, int two_stage,
                                     float* d_low_scratch, void* stream);
/* The other kernels of the output tail, one launch each, for the fp64 operator tests in tests/test_gpu_output_tail.py.  All refuse
 * (LSEG_ERR_INVALID: NULL pointer, B / H / W < 1, H or W < 2 where a bilinear is taken; LSEG_ERR_UNSUPPORTED: C % 8 != 0 or C > 1024)
 * before anything is launched.
 *   pixel_gram         d_g16pad fp16 padded NHWC [B, H+2, W+2, C] (finite border: it enters the last row's and column's records)
 *                      -> d_gram fp32 [B, H, W, 5], the records of lseg_op_corr_planes for any C (the generic schedule's producer)
 *   norm_scale_plane   d_gram [B, H, W, 5] -> d_scale fp32 [B, 2H, 2W] = s / ||u||, ||u||^2 the 10-term quadratic form of the x2
 *                      bilinear's (align_corners=True) four weights over the cell's dot products.  d_flag (may be NULL): set to 1 when
 *                      a squared norm is not finite, never cleared
 *   upsample_norm_f16  d_g32pad fp32 padded NHWC [B, H+2, W+2, C] (border never read) -> d_a16 fp16 [B, 2H, 2W, C] =
 *                      fp16(scale * fp16(u / ||u||)), u = the x2 bilinear of g (strict mode and label sets beyond the LDS limit) */
int lseg_op_pixel_gram(const void* d_g16pad, float* d_gram, int B, int H, int W, int C, void* stream);
int lseg_op_norm_scale_plane(const float* d_gram, float* d_scale, int B, int H, int W, float s, unsigned* d_flag, void* stream);
int lseg_op_upsample_norm_f16(const float* d_g32pad, void* d_a16, int B, int H, int W, int C, float scale, void* stream);
/* pixel x text correlation (lseg_net.py:187-196): feat fp32 [M,C]; text fp16 [K,C]
 * (already L2-normalised); logits fp32 [B,K,P] with M = B*P.  Internally:
 * a = fp16(scale * fp16(feat/||feat||)); logits = fp16(a @ text^T). */
int lseg_op_correlation(const float* d_feat, const void* d_text_f16, float* d_logits,
                        int B, int P, int C, int K, float logit_scale, void* stream);

/* fused scratch.head1 + pixel normalisation (lseg_net.py:185-194, out_c = 512): x bf16 [M,F] pixels,
 * w bf16 [512,F], bias fp32 [512]  ->  a fp16 [M,512] = fp16(scale * fp16(v/||v||_2)), v = x w^T + bias
 * (the A operand of the correlation GEMM; the fp32 features are never materialised). */
int lseg_op_head_features(const void* d_x_bf16, const void* d_w_bf16, const float* d_bias, void* d_a_f16,
                          int M, int F, float logit_scale, void* stream);

/* Segmentation statistics of a score tensor against a target mask, on the device (one pass over the scores).
 * replaces: the host-side metric / loss step after LSeg.forward --
 *   batch_pix_accuracy + batch_intersection_union ([3P] encoding/utils/metrics.py; called at
 *   lsegmentation_module.py:49-50,59-60 and through SegmentationMetric.update at test_lseg.py:385-388), and the
 *   forward value of SegmentationLosses = nn.CrossEntropyLoss(ignore_index) ([3P] encoding/nn/loss.py; :72).
 * d_scores fp32 [B,K,H,W]; d_target int64 [B,H,W] (values -1 = unlabeled / 0..K-1);
 * d_counts int64 [2+3K] = {correct, labeled, area_inter[K], area_pred[K], area_lab[K]}  (union = pred + lab - inter);
 * d_nll double [2] = {sum over valid pixels of -log_softmax(scores)[target], number of valid pixels}. */
int lseg_op_seg_stats(const float* d_scores, const int64_t* d_target, int B, int K, int H, int W, int ignore_index,
                      int64_t* d_counts, double* d_nll, void* stream);
/* The same statistics (and / or the masks) straight from the LOW-resolution logits [B,K,h,w] the engine keeps before
 * scratch.output_conv (lseg_net.py:203): every pixel of the [B,2h,2w] grid reads them through the x2 bilinear (align_corners=True)
 * on the fly, so the metric / mask step needs no full-resolution logits.  d_target int64 [B,2h,2w] or NULL (then d_counts / d_nll
 * are not touched); d_argmax uint8 [B,2h,2w] or NULL. */
int lseg_op_seg_stats_lowres(const float* d_low, const int64_t* d_target, int B, int K, int h, int w, int ignore_index,
                             int64_t* d_counts, double* d_nll, uint8_t* d_argmax, void* stream);

/* Few-shot episode statistics of 2-label scores, bare (csrc/episode.hip; the kernel behind lseg_episode_stats).
 * replaces: Evaluator.classify_prediction (fewshot_data/common/evaluation.py:12-39: per image torch.histc x 3 and a host
 *   synchronisation), AverageMeter.update's index_add_ (fewshot_data/common/logger.py:29-31) and nn.CrossEntropyLoss() on [B,2,H*W]
 *   (lsegmentation_module_zs.py:338-343).
 * d_scores fp32 [B,2,H,W] (up = 0), or the low-resolution logits [B,2,H/2,W/2] read through the x2 bilinear (align_corners=True) on the
 *   fly (up = 1; H, W even and >= 4): bit-identical to lseg_op_upsample2x_planes of the same planes.
 * d_target int64 [B,H,W]; d_ignore uint8 [B,H,W] or NULL.  Per pixel pred = (v1 > v0) (a tie is class 0, torch's first maximum).  Where
 *   the ignore mask is set neither pred nor target counts; a target outside {0, 1} is in no area_gt and no intersection, pred still
 *   counts there.  The cross-entropy is logsumexp(v0, v1) - v[target] over the pixels with target in {0, 1} and != ignore_index; the
 *   ignore MASK does not enter it (the reference hands `target` to the criterion).
 * d_areas int64 [B,6] per image {inter0, inter1, pred0, pred1, gt0, gt1} (union = pred + gt - inter), exact;
 * d_nll double [B,2] per image {sum, pixels}: per-workgroup partials in d_ws folded in a fixed order -- two calls on the same input
 *   give the same bits;
 * d_flags int64 [2] = {pixels with ignore set and target != 0 (the reference asserts 0), pixels with a target outside {0, 1} that is
 *   not ignore_index}.  d_areas, d_nll and d_flags are overwritten.
 * Meter scatter (optional: d_class_id, d_inter_buf, d_union_buf all given or all NULL): d_class_id int64 [B], the int64 [2,nclass]
 *   buffers get every image's inter / union ADDED to column d_class_id[b] (duplicates add up).  The caller validates the ids on the host
 *   (it has them there: they picked the label pairs); the kernel skips an id outside [0, nclass) rather than write out of bounds.
 * d_ws / ws_bytes: at least lseg_op_episode_stats_ws_bytes(B, H, W) bytes of device scratch, 8-byte aligned. */
size_t lseg_op_episode_stats_ws_bytes(int B, int H, int W);
int lseg_op_episode_stats(const float* d_scores, const int64_t* d_target, const uint8_t* d_ignore, int B, int H, int W, int up,
                          int ignore_index, const int64_t* d_class_id, int nclass, int64_t* d_inter_buf, int64_t* d_union_buf,
                          int64_t* d_areas, double* d_nll, int64_t* d_flags, void* d_ws, size_t ws_bytes, void* stream);

/* Segmentation statistics of a LABEL MAP against a target mask (csrc/label_stats.hip): lseg_op_seg_stats' counters for the routes that
 * never form the [B,K,H,W] scores (lseg_forward_labels, the ragged lists of lseg_set_text_groups, BatchedMultiEval.forward_labels).
 * replaces: batch_pix_accuracy + batch_intersection_union ([3P] encoding/utils/metrics.py) on torch.max(scores, 1)[1].
 * d_label int16 [B,H,W]; d_target int64 [B,H,W]; any alignment of their elements (a lane reads four pixels: one 8-byte label load and
 *   two 16-byte target loads where the addresses allow, element loads at the ends of an image).
 * Shared label set (d_offsets NULL): d_counts int64 [2+3K] = {correct, labeled, area_inter[K], area_pred[K], area_lab[K]}, the layout of
 *   lseg_op_seg_stats.  Per pixel (label l, target t): t == -1 or t == ignore_index is unlabeled and counts nowhere; any other t < 0
 *   counts nowhere and is flagged; otherwise labeled++ and area_pred[l]++, and for t < K area_lab[t]++ and, when l == t, correct++ and
 *   area_inter[l]++; t >= K is flagged and is in no area_lab and no intersection (the predicted area still counts, as in
 *   lseg_op_episode_stats).  With ignore_index = -1, or a target that holds no ignore_index, this is lseg_op_seg_stats' rule: the counts
 *   equal its counts for any scores whose first-maximum arg-max is d_label, exactly.
 * Ragged lists (d_offsets int32 [B+1] on the DEVICE, the prefix sum of the per-image counts as lseg_op_corr_argmax_ragged leaves it; K =
 *   the largest count, an upper bound for every image): labels and targets of image b index its own list [0, k_b).  Without d_class_map
 *   the areas are indexed offsets[b] + l and have length offsets[B], which takes K's place in the d_counts layout.  With d_class_map
 *   int32 [offsets[B]] prediction and target both go through class_map[offsets[b] + l] in [0, nclass): three areas of length nclass,
 *   a pixel is correct when the two class ids agree, duplicate ids add up, and an id outside [0, nclass) is skipped, never written out
 *   of bounds (the caller validates the ids on the host, as for lseg_op_episode_stats).
 * d_flags int64 [2] = {pixels whose target is neither unlabeled nor inside its label range, pixels whose label is outside its range (these
 *   count nowhere)}.  accumulate = 0 overwrites d_counts and d_flags, 1 adds to both: a meter can live on the device across batches.
 * Areas: while 3 x bins x 4 bytes fit 48 KiB (bins <= 4096; bins = K, or nclass with a map) every workgroup keeps its three histograms in
 *   LDS and flushes the non-zero bins with 64-bit atomics; above that every update is a 64-bit global atomic.  Integer sums: exact in any
 *   order.  lseg_op_label_stats_plan (host only, no device) returns out2 = {route: 0 LDS / 1 global, bins per workgroup (0 on route 1)}.
 * Before anything is launched or the device is touched: LSEG_ERR_INVALID for a NULL required pointer, B, H, W or K < 1, a map without
 *   offsets or with nclass < 1, pointers not aligned to their element; LSEG_ERR_UNSUPPORTED for K > 32767 or H W > 2^31 - 1. */
int lseg_op_label_stats_plan(int K_or_bins, int* out2);
/* Which schedule the inference forward runs for a request, and whether it refuses it before any launch: host only, no handle, no device.
 * n requests; request i reads in13 + 13 i = {wanted outputs, K, group_k, ragged, arch_option, out_c, quarter-resolution width, debug,
 * strict (split precision), the commuted head is packed for out_c, LSEG_CORR_FULLRES set, LSEG_CORR_GENERIC set, LSEG_NO_UPSAMPLE4X set} with
 * wanted = bit 0 logits, 1 uint8 masks, 2 labels, 3 score, 4 low-resolution logits, 5 runner-up (label2 or score2), 6 lse, 7 held
 * features, 8 loss, 9 the loss's target; and writes out6 + 6 i = {refusal status (0 | LSEG_ERR_INVALID | LSEG_ERR_UNSUPPORTED; the
 * refusals that read the engine's state -- finalised, tokens set, B, train mode, the label list lengths, grouped K, uint8 masks beyond
 * K = 256 -- are not in it), tail, source of the quarter-resolution label planes, commuted, corr_low, corr_fused}.
 * tail: 0 held features, 1 streamed ragged labels, 2 streamed shared-set labels, 3 one-pass x4 upsample into the logits, 4 x2 upsample
 * into the low-resolution output, 5 planes in memory from the quarter-resolution planes, 6 / 7 / 8 planes in memory from the (2h, 2w)
 * feature map made by the commuted head + upsample_norm / the row-norm GEMM / head1 + l2norm.  planes (tails 3..5): 1 the dedicated
 * correlation kernel, 2 per-image GEMMs, 3 the generic GEMM; 0 elsewhere.  The route of a refused request is unspecified. */
int lseg_op_forward_route(const int32_t* in13, int n, int32_t* out6);
/* How the label head of the training step runs for a configuration, and whether the train-mode forward refuses it: host only, no handle,
 * no device.  n rows; row i reads in11 + 11 i = {group_k, ragged lists set, longest list, K, head blocks (0: none), arch_option,
 * lseg_config.flags bit 1 set, image dtype (LSEG_F16 | LSEG_BF16), out_c, a logits output wanted, LSEG_CORR_RAGGED_GEMM set} and writes
 * out8 + 8 i = {refusal status (0 | LSEG_ERR_UNSUPPORTED; the refusals that read the engine's state are not in it), mode, label planes
 * per image, row pitch of d(low) (up64 of the longest list | 8 | up64(K)), dtype of the d(low) rows, a transposed dgrad operand is made,
 * head blocks run, which refusal}.  refusal, the first that holds: 1 either grouping with arch_option != 0, 2 ragged lists with a logits
 * output, 3 group_k outside 1..8 or out_c not a multiple of 8 in [8, 1024]; 0 none.
 * mode: 0 one label set shared by the batch, 1 group_k labels per image, 2 ragged lists on per-image GEMMs, 3 ragged lists on the
 * one-launch kernels. */
int lseg_op_train_head_plan(const int32_t* in11, int n, int32_t* out8);
int lseg_op_label_stats(const int16_t* d_label, const int64_t* d_target, int B, int H, int W, int K, int ignore_index,
                        const int32_t* d_offsets, const int32_t* d_class_map, int nclass, int64_t* d_counts, int64_t* d_flags,
                        int accumulate, void* stream);
/* lseg_op_seg_stats_lowres for a label set walked in PANELS (csrc/label_stats.hip): metrics and the cross-entropy value with peak memory
 * set by the panel, not by K -- the scoring side of the held-features route (lseg_forward_features / lseg_score_features).
 *   lseg_op_stats_fold_lowres  d_low fp32 [B,rows,h,w]: the low-resolution logits of labels row0 .. row0+rows-1, read through output_conv's
 *       x2 bilinear (align_corners=True) on the fly -- every value is bit-identical to lseg_op_upsample2x_planes of the same planes.  Per
 *       pixel of the [B,2h,2w] grid (d_target int64, d_label int16, d_best / d_sum / d_tlogit fp32): `if v > best: (best, label) = (v, k)`
 *       (panels in ascending label order: the first maximum wins), the online sum of exp(v - best) by lseg_op_eval_merge_labels' rule (a new
 *       best rescales, sum = sum * exp(old_best - new_best) + 1; any other value adds exp(v - best)), and d_tlogit = v where k == target
 *       (NaN until a panel holds the target).  first = 1 writes the state without reading it.  h, w >= 2; d_label 4-byte, the fp32 planes
 *       and d_target 8-byte aligned (a lane owns a pixel pair).  row0 + rows > 32767: LSEG_ERR_UNSUPPORTED.
 *   lseg_op_stats_finish       d_counts int64 [2+3K] exactly as lseg_op_label_stats (shared label set, accumulate = 0) gives from d_label --
 *       one kernel body -- and d_nll double [2] = {sum over valid pixels (target in [0, K), != ignore_index) of best + log(sum) - tlogit,
 *       number of those pixels}: per-workgroup partials in d_ws folded in ascending order, so two calls on the same input give the same
 *       bits.  d_flags int64 [3] = lseg_op_label_stats' two words and the number of valid pixels whose target no panel covered (a caller
 *       error: left out of the sum and the count).  d_ws: lseg_op_stats_finish_ws_bytes(B, H, W) bytes of device scratch, 8-byte aligned.
 * The state of K labels is the same bits for every partition into panels (label, best, tlogit exactly; sum is one chain of fp32 operations
 * in label order whatever the panels).  LSEG_ERR_INVALID before anything is launched for NULL pointers and shapes < 1. */
int lseg_op_stats_fold_lowres(const float* d_low, int B, int rows, int row0, int h, int w, const int64_t* d_target,
                              int16_t* d_label, float* d_best, float* d_sum, float* d_tlogit, int first, void* stream);
size_t lseg_op_stats_finish_ws_bytes(int B, int H, int W);
int lseg_op_stats_finish(const int16_t* d_label, const float* d_best, const float* d_sum, const float* d_tlogit, const int64_t* d_target,
                         int B, int H, int W, int K, int ignore_index, int64_t* d_counts, double* d_nll, int64_t* d_flags, void* d_ws,
                         size_t ws_bytes, void* stream);

/* The pixel x text correlation on the engine's commuted schedule (DESIGN.md par. 3.4), one dedicated kernel (csrc/corr.hip).
 * replaces: `logits_per_image = self.logit_scale * image_features.half() @ text_features.t()` (modules/models/lseg_net.py:194) together
 *   with the norm of lseg_net.py:190 -- as label planes R[b, k, p] = t_k . g_p on the quarter-resolution map g (the combined
 *   head1 o out_conv 1x1 conv output, padded NHWC fp16) and the five dot products of every 2x2 cell of g that the norm of the
 *   x2-up-sampled feature is made of; the scale / fp16 rounding / upsample kernels consume both.
 * d_g16pad fp16 [B, H+2, W+2, C] (C = 512); d_text16 fp16 [K, C] (K x (2C + 16) bytes must fit the 160 KB LDS: K <= 157);
 * d_planes fp32 [B, K, (H+2)(W+2)] -- interior pixels written; d_gram fp32 [B, H, W, 5] = {g.g, g.g(x+1), g.g(y+1), g.g(y+1,x+1),
 * g(x+1).g(y+1)} or NULL (planes only).  LSEG_ERR_UNSUPPORTED for other C / larger K (the engine then takes its generic GEMM). */
int lseg_op_corr_planes(const void* d_g16pad, const void* d_text16, float* d_planes, float* d_gram, int B, int K, int H, int W, int C,
                        void* stream);
/* The streamed-panel correlation + arg-max behind lseg_forward_labels, bare (csrc/corr_argmax.hip).
 * replaces: lseg_net.py:194-203 (correlation, the two x2 bilinears with the per-pixel scale and the fp16 rounding between them) followed by
 *   torch.max(pred, 1) (lsegmentation_module.py:114-117), for any K: d_label[b, y, x] = first arg-max over k of the value
 *   lseg_op_upsample4x_planes_scaled would write to out[b, k, y, x] from lseg_op_corr_planes' planes; d_score = that value.
 * d_g16pad fp16 [B, H+2, W+2, C] (C = 512); d_text16 fp16 [K, C]; d_scale fp32 [B, 2H, 2W]; d_label int16 [B, 4H, 4W]; d_score fp32
 * [B, 4H, 4W] or NULL.  H, W >= 2.  d_ws / ws_bytes: optional workspace -- with 96 B H W bytes per part the labels of a tile are split over
 * up to 8 workgroups and merged (same result: ascending parts, first maximum wins); NULL = one workgroup per tile streams all K.
 * LSEG_ERR_UNSUPPORTED for other C, K > 32767 or maps beyond the kernel's 32-bit offsets. */
int lseg_op_corr_argmax(const void* d_g16pad, const void* d_text16, const float* d_scale, int16_t* d_label, float* d_score, int B, int K,
                        int H, int W, int C, void* d_ws, size_t ws_bytes, void* stream);
/* lseg_op_corr_argmax with the confidence outputs of lseg_forward_labels_conf, bare.
 * replaces: torch.topk(pred, 2, 1) and torch.logsumexp(pred, 1) on the logits of lseg_net.py:194-203, for any K: d_label / d_score are
 *   lseg_op_corr_argmax's bit for bit; (d_label2, d_score2) = entry 1 of a stable descending sort over k of the values
 *   lseg_op_upsample4x_planes_scaled would write (K = 1: -1 / -inf); d_lse = their log-sum-exp (fp32, online).
 * d_label2 int16, d_score2 / d_lse fp32 [B, 4H, 4W], each or NULL (all NULL = lseg_op_corr_argmax).  d_ws / ws_bytes: with 256 B H W bytes
 * per part (16 per output pixel: five planes) the labels of a tile are split and merged in ascending order -- top-2 by the same rule
 * (bit-equal), lse by log-add-exp (another summation order: equal within fp32 rounding).  Errors as lseg_op_corr_argmax. */
int lseg_op_corr_argmax_conf(const void* d_g16pad, const void* d_text16, const float* d_scale, int16_t* d_label, float* d_score,
                             int16_t* d_label2, float* d_score2, float* d_lse, int B, int K, int H, int W, int C, void* d_ws, size_t ws_bytes,
                             void* stream);
/* lseg_op_corr_argmax(_conf) for RAGGED per-image label sets, bare: image b is correlated with host_counts[b] consecutive rows of d_text16
 * (fp16 [sum of counts, C]: image 0's rows first) only, and every label output indexes the image's OWN list, 0 .. host_counts[b] - 1.
 * Image b's five planes are bit-equal to lseg_op_corr_argmax_conf with B = 1 on its slices of the inputs (with a workspace: lse within
 * fp32 rounding, as there).  A list of one label behaves as K = 1: label2 = -1, score2 = -inf, lse = score.
 *   host_counts int32 [B] in HOST memory: the launcher validates them without a device round trip and forms the offsets itself (a device
 *              array of offsets could not be checked before the launch; this is the design chosen of the two, so there is no caller-made
 *              offsets[0] to be wrong)
 *   d_offsets  int32 [B + 1] device scratch: filled on the stream with the prefix sum of the counts (the values travel as kernel
 *              arguments: host_counts may be freed as soon as the call returns) and read by the kernels behind it
 *   d_label2 / d_score2 / d_lse: all NULL = the plain arg-max instantiation, any of them = the confidence one
 *   d_ws / ws_bytes: as lseg_op_corr_argmax(_conf); the label parts (whole panels) are sized from the LARGEST count, a part beyond an
 *              image's own count is neither written nor merged
 * LSEG_ERR_INVALID, before anything is launched: a count < 1 or > 32767, a NULL required pointer (inputs, host_counts, d_offsets,
 * d_label), B < 1, H or W < 2.  LSEG_ERR_UNSUPPORTED: C != 512, maps or text tables beyond the kernel's 32-bit offsets. */
int lseg_op_corr_argmax_ragged(const void* d_g16pad, const void* d_text16, const float* d_scale, const int32_t* host_counts, int32_t* d_offsets,
                               int16_t* d_label, float* d_score, int16_t* d_label2, float* d_score2, float* d_lse, int B, int H, int W, int C,
                               void* d_ws, size_t ws_bytes, void* stream);
/* The label split that launch takes when it plans for `cus` compute units and a workspace of ws_bytes (0 = none), host only: out2 =
 * {parts, labels per part (a multiple of the panel)}.  Part s of image b holds its labels [s * out2[1], min((s + 1) * out2[1], count_b))
 * and exists only when that range is not empty.  conf != 0: the confidence instantiation (16 instead of 6 bytes per pixel and part). */
int lseg_op_corr_argmax_ragged_split(const int32_t* host_counts, int B, int H, int W, int conf, size_t ws_bytes, int cus, int* out2);
/* The tile geometry that kernel was compiled with (host memory, no device needed), for the CPU index model of its tile -> footprint
 * mapping: out8 = {mid rows/columns per tile band, mid rows/columns of its footprint, base rows/columns of its footprint, labels per
 * panel, LDS pitch of a text row in bytes, labels per interpolation chunk, output rows per wave, dynamic LDS bytes}. */
int lseg_op_corr_argmax_geometry(int* out8);
/* lseg_op_corr_argmax with the cross-entropy of lseg_forward_labels_loss, bare: one shared set of K rows (host_counts NULL) or ragged
 * per-image lists (host_counts int32 [B] on the HOST as for lseg_op_corr_argmax_ragged; K is then not read).
 * replaces: F.cross_entropy(pred, target, ignore_index, reduction='none' / 'sum') and torch.max(pred, 1) on the logits of
 *   lseg_net.py:194-203, for any K.
 * d_target int64 [B, 4H, 4W]; a pixel is VALID iff target != ignore_index and 0 <= target < K (ragged: < host_counts[b]).
 * d_label / d_score: lseg_op_corr_argmax's bit for bit; d_lse: lseg_op_corr_argmax_conf's bit for bit.
 * d_tlogit fp32 [B, 4H, 4W]: the value lseg_op_upsample4x_planes_scaled would write to out[b, target, y, x] (where target == label it IS
 *   d_score); -inf where the pixel is not valid.  d_nll_plane fp32: d_lse - d_tlogit, 0 where not valid.
 * d_nll double [2] = {sum over the valid pixels of double(lse) - double(tlogit), their number}.  The sum is formed in a fixed order without
 *   atomics: lseg_op_corr_argmax_loss_plan gives out4 = {threads per workgroup, pixels per workgroup, workgroups, bytes of partials};
 *   workgroup j owns pixels [j * out4[1], (j + 1) * out4[1]) of the flattened maps, lane t of it pixels j * out4[1] + t + out4[0] * m, and
 *   the partials are added in ascending order.
 * Every output after d_label may be NULL.
 * d_ws / ws_bytes: ONE workspace, 8-byte aligned, pieces in this order, each rounded up to 256 bytes: ragged: B + 1 int32 offsets; d_nll
 *   given: the partials; d_nll or d_nll_plane given: an fp32 [B, 4H, 4W] plane for each of d_lse / d_tlogit that is NULL (the reduction
 *   reads both).  lseg_op_corr_argmax_loss_ws_bytes(B, H, W, ragged, want_nll, temp_planes, parts) returns these bytes plus `parts` label
 *   parts of 224 B H W bytes each (14 per output pixel: score, lse, tlogit, label); what the workspace holds beyond the required pieces
 *   is used for the label split as in lseg_op_corr_argmax_conf (label / score / tlogit bit-equal to the unsplit form -- tlogit by max:
 *   exactly one part holds the target's label -- lse by log-add-exp).  A call that needs no piece takes d_ws = NULL.
 * Refusals as lseg_op_corr_argmax_conf / _ragged, plus LSEG_ERR_INVALID for a NULL target and for a workspace smaller than the required
 * pieces; every refusal happens before anything is launched and writes no output. */
int lseg_op_corr_argmax_loss(const void* d_g16pad, const void* d_text16, const float* d_scale, const int64_t* d_target, int ignore_index,
                             const int32_t* host_counts, int B, int K, int H, int W, int C, int16_t* d_label, float* d_score, float* d_lse,
                             float* d_tlogit, float* d_nll_plane, double* d_nll, void* d_ws, size_t ws_bytes, void* stream);
size_t lseg_op_corr_argmax_loss_ws_bytes(int B, int H, int W, int ragged, int want_nll, int temp_planes, int parts);
int lseg_op_corr_argmax_loss_plan(int B, int H, int W, int64_t* out4);

/* Device side of the multi-scale / flip sliding-window evaluator that calls the forward (additional_utils/encoding_models.py:54-155
 * MultiEvalModule.forward, module_inference, pad_image, crop_image, flip_image; additional_utils/models.py:55-140).  Per scale:
 *   lseg_op_eval_make_crops  d_img fp32 [C,height,width] (the resized image, C <= 3) -> d_crops fp32 [(1+flip)*n, C, crop, crop], n =
 *                            h_grids*w_grids: crop (idh,idw) starts at (idh*stride, idw*stride), pixels beyond the image take pad[c]
 *                            (= -mean/std, :144-155); with flip the second half holds the mirrored twins (:135-137)
 *   lseg_op_eval_accumulate  d_outs fp32 [(1+flip)*n, K, crop, crop] (the engine's logits for that stack) -> d_map fp32 [K,height,width]:
 *                            out + flip(out_twin) summed over the covering boxes in (idh,idw) order, divided by their count, cropped
 *                            to the un-padded size (:100-121); ph, pw = size of the padded image the boxes are clipped to.  Arguments
 *                            are checked before the device is touched, as for every accumulate / finalize entry below:
 *                            LSEG_ERR_INVALID for NULL or not 4-byte aligned pointers, or boxes that do not cover the map
 *   lseg_op_eval_resize      d_dst [P,Ho,Wo] (+)= bilinear(d_src [P,Hi,Wi]), align_corners=True (:78, :123: the image resize and
 *                            `scores += resize_image(outputs, h, w)`) */
int lseg_op_eval_make_crops(const float* d_img, float* d_crops, int C, int height, int width, int crop, int stride, int h_grids, int w_grids,
                            int flip, const float* host_pad3, void* stream);
int lseg_op_eval_accumulate(const float* d_outs, float* d_map, int K, int height, int width, int ph, int pw, int crop, int stride,
                            int h_grids, int w_grids, int flip, void* stream);
int lseg_op_eval_resize(const float* d_src, float* d_dst, int P, int Hi, int Wi, int Ho, int Wo, int accumulate, void* stream);
/* The crops of one scale straight from ONE decoded image: d_img uint8 [src_h, src_w, 3] (HWC) -> d_crops fp32
 * [(1+flip)*n, 3, crop, crop].  One kernel (csrc/input_u8.hip) in the reference's order -- normalise ((v / 255 - mean) / std, as
 * lseg_set_input_u8), bilinear align_corners=True resize to (height, width), pad with host_pad3, cut, mirror -- with the arithmetic of
 * lseg_op_eval_resize: bit-equal to lseg_op_eval_resize + lseg_op_eval_make_crops on the torch-normalised fp32 image. */
int lseg_op_eval_make_crops_u8(const uint8_t* d_img, float* d_crops, int src_h, int src_w, int height, int width, int crop, int stride,
                               int h_grids, int w_grids, int flip, const float* host_pad3, const float* host_mean3, const float* host_std3,
                               void* stream);
/* lseg_op_eval_accumulate on the logits lseg_forward_lowres leaves: d_low fp32 [(1+flip)*n, K, crop/2, crop/2] is read through
 * output_conv's x2 bilinear (align_corners=True) on the fly, so the [(1+flip)*n, K, crop, crop] stack never exists.  Defined as -- and
 * bit-identical to -- lseg_op_eval_accumulate(lseg_op_upsample2x_planes(d_low)): per covering box in (idh,idw) order
 * v = up(low_b)[y-h0, x-w0] (+ up(low_twin_b)[y-h0, crop-1-(x-w0)], the twin's tap taken at the mirrored full-resolution coordinate),
 * acc += v, then acc / count.  crop even and >= 4.  Arguments are checked before the device is touched: LSEG_ERR_INVALID for NULLs, an
 * odd or too small crop, or boxes that do not cover the map. */
int lseg_op_eval_accumulate_lowres(const float* d_low, float* d_map, int K, int height, int width, int ph, int pw, int crop, int stride,
                                   int h_grids, int w_grids, int flip, void* stream);
/* The same accumulation for PART of a scale's grid, so that a scale with more crops than fit in memory runs as several forwards.
 * A window is boxes [first_box, first_box + n_box) of the grid in row-major (idh,idw) order; d_outs fp32 [(1+flip)*n_box, K, crop, crop]
 * holds only their logits (twins in the second half).  For every pixel of d_sum fp32 [K,height,width] that a box of the window covers,
 * d_sum += out + flip(out_twin) per covering box of the window in ascending box order; no division.  Pixels no box of the window covers
 * are neither read nor written, and the launch is sized by the window's footprint.  The caller zeroes d_sum before the first window,
 * submits the windows of any partition of the grid in ascending order and then calls lseg_op_eval_finalize: the result is bit-identical
 * to lseg_op_eval_accumulate on the whole stack (the same fp32 additions from 0 in the same order, then the same division).
 *   lseg_op_eval_accumulate_window_lowres  the same over d_low fp32 [(1+flip)*n_box, K, crop/2, crop/2], read through the x2 bilinear
 *                                          with lseg_op_eval_accumulate_lowres' tap arithmetic (crop even and >= 4)
 *   lseg_op_eval_finalize                  d_map = d_sum / (number of boxes of the whole grid covering the pixel); d_map == d_sum allowed
 * Arguments are checked before the device is touched: LSEG_ERR_INVALID for NULLs, n_box <= 0, a window outside the grid, boxes that do
 * not cover the map, or (lowres) an odd or too small crop. */
int lseg_op_eval_accumulate_window(const float* d_outs, float* d_sum, int K, int height, int width, int ph, int pw, int crop, int stride,
                                   int h_grids, int w_grids, int flip, int first_box, int n_box, void* stream);
int lseg_op_eval_accumulate_window_lowres(const float* d_low, float* d_sum, int K, int height, int width, int ph, int pw, int crop, int stride,
                                          int h_grids, int w_grids, int flip, int first_box, int n_box, void* stream);
int lseg_op_eval_finalize(const float* d_sum, float* d_map, int K, int height, int width, int ph, int pw, int crop, int stride, int h_grids,
                          int w_grids, void* stream);
/* Label panels of the multi-scale evaluator (BatchedMultiEval.forward_labels): fold one panel of fused scores into a running per-pixel
 * state, so that torch.max / torch.sort / torch.logsumexp over a [K,H,W] score tensor need no such tensor.
 *   d_scores fp32 [rows,H,W]: the scores of labels row0 .. row0+rows-1, taken in ascending label order
 *   d_label int16 / d_score fp32 [H,W]: the arg-max so far and its score (required)
 *   d_label2 int16 / d_score2 fp32 [H,W]: the runner-up; d_sum fp32 [H,W]: the sum of exp(score_k - best) over the labels seen
 * Per pixel and plane: `if v > best: (second, label2) = (best, label); (best, label) = (v, k)  elif v > second: (second, label2) = (v, k)`
 * -- entries 0 and 1 of a stable descending sort over all labels submitted (equal values go to the lower label; a later label equal to
 * the winner is the runner-up), the rules of lseg_forward_labels_conf -- and the online log-sum-exp of csrc/corr_argmax.hip's CONF
 * instantiation, relative to the running best in fp32: a new best rescales, sum = sum * exp(old_best - new_best) + 1, any other value
 * adds exp(v - best).  first = 1: the state is written without being read (no clear launch); last = 1: d_sum receives
 * score + log(sum), the log-sum-exp.  One label in all: label2 = -1, score2 = -inf.  d_label2, d_score2, d_sum may each be NULL, on
 * EVERY call of a sequence or on none (d_label2 needs d_score2, its running state); with all three NULL only (best, label) is kept and
 * equals the first two outputs of the full form bit for bit.  Pointers aligned to their element; a lane owns four consecutive pixels
 * and uses 16-byte accesses wherever an address allows.  row0 + rows > 32767: LSEG_ERR_UNSUPPORTED; NULL required pointers, rows < 1,
 * row0 < 0: LSEG_ERR_INVALID. */
int lseg_op_eval_merge_labels(const float* d_scores, int rows, int row0, int H, int W,
                              int16_t* d_label, float* d_score, int16_t* d_label2, float* d_score2, float* d_sum,
                              int first, int last, void* stream);

/* Backward of one Linear layer y = x W^T + b -- first brick of the training step (the reference gets
 * it from torch autograd under LSegmentationModule.training_step, lsegmentation_module.py:66-81).  bf16/fp16 operands,
 * fp32 accumulate, both GEMMs on the forward MFMA kernel with the contraction dimension transposed onto the fast axis:
 *   d_dx [M,K] (operand dtype)  = dY [M,N] . W [N,K]          (may be NULL)
 *   d_dw [N,K] fp32             = dY^T [N,M] . X [M,K]         (may be NULL)
 *   d_db [N]   fp32             = column sums of dY            (may be NULL)
 * N and K multiples of 64. */
int lseg_op_linear_backward(const void* d_dy, const void* d_x, const void* d_w, int ab_dtype, void* d_dx, float* d_dw,
                            float* d_db, int M, int N, int K, void* stream);

/* Backward of LayerNorm over the last dimension (timm norm1/norm2 on the fp32 residual stream; autograd in the
 * reference): d_dy [M,D] (fp32 / bf16 / fp16), d_x [M,D] fp32 (the forward input), d_gamma [D];
 * d_dx [M,D] fp32 (= or += when accumulate_dx: the residual stream's gradient), d_dgamma / d_dbeta [D] fp32. */
int lseg_op_layernorm_backward(const void* d_dy, int dy_dtype, const float* d_x, const float* d_gamma, float* d_dx,
                               float* d_dgamma, float* d_dbeta, int M, int D, float eps, int accumulate_dx, void* stream);

/* Backward of a stride-1 3x3 convolution in the padded-NHWC layout (the DPT head's convs, lseg_blocks.py:73-108,
 * 237-255; autograd in the reference), bf16 operands, built on the forward kernels:
 *   d_dx_pad [B,H+2,W+2,Cin] bf16, interior written (caller keeps the border zero) = conv3x3(dY, W flipped / channel-swapped)
 *   d_dw     [Cout, 9*Cin]  fp32 (tap-major, like d_w_packed)            = dY^T x (9 row-shifted copies of X)^T, one GEMM
 * d_dy_pad [B,H+2,W+2,Cout] bf16 with a ZERO border, d_x_pad the forward input.  Either output may be NULL. */
int lseg_op_conv3x3_backward(const void* d_dy_pad, const void* d_x_pad, const void* d_w_packed, void* d_dx_pad, float* d_dw,
                             int B, int H, int W, int Cin, int Cout, void* stream);

/* More backward bricks (autograd in the reference; each checked against torch autograd in tests/test_gpu_ops.py):
 *   gelu_backward           d_dx = d_dy * GELU'(d_pre), erf form (timm Mlp.act), bf16/fp16 [n]
 *   upsample2x_nhwc_backward  transpose of lseg_op_upsample2x_nhwc: d_dout [B,2H,2W,C] bf16 -> d_din_pad [B,H+2,W+2,C] interior
 *   softmax_ce_backward     d_dscores [B,K,H,W] fp32 = (softmax_k - 1[k = target]) / n_valid (0 at ignored pixels);
 *                           d_nll = the double[2] written by lseg_op_seg_stats (n_valid in d_nll[1]) */
int lseg_op_gelu_backward(const void* d_dy, const void* d_pre, void* d_dx, int64_t n, int dtype, void* stream);
int lseg_op_quickgelu_backward(const void* d_dy, const void* d_pre, void* d_dx, int64_t n, int dtype, void* stream);   /* CLIP: x*sigmoid(1.702x) */
int lseg_op_upsample2x_nhwc_backward(const void* d_dout, void* d_din_pad, int B, int H, int W, int C, void* stream);
int lseg_op_softmax_ce_backward(const float* d_scores, const int64_t* d_target, float* d_dscores, int B, int K, int H, int W,
                                int ignore_index, const double* d_nll, void* stream);

/* Backward of lseg_op_attention (softmax(Q K^T * scale) V, head_dim 64, no mask); the reference gets it from autograd through
 * [3P] timm Attention.forward (lseg_vit.py:196-197).  Flash-style recomputation (csrc/attention_bwd2.hip), no atomics:
 * d_q,d_k [BH,Npad,64], d_vt [BH,64,Npad], d_o / d_do [B,Ntok,H*64] (forward layouts, bf16/fp16); d_lse2 [BH,Npad] fp32 = log2 of
 * each query row's sum_k exp2(s_k * scale * log2e) (the forward's running statistics) -- a dQ kernel and a
 * dK/dV kernel in the forward kernel's MFMA / direct-to-LDS structure, writing d(qkv Linear output) [B*Ntok, 3*H*64] (bf16/fp16)
 * directly.  d_ws: lseg_op_attention_backward_ws_bytes(B, H, Npad) bytes of device scratch, or NULL (then allocated per call).
 * What is computed, from the operands as given: P = exp2(Q K^T scale log2(e) - lse2), D = rowsum(dO o O), dS = P o (dO V^T - D) scale,
 * dQ = dS K, dK = dS^T Q, dV = P^T dO (P and dS rounded once to the operand type).
 * Refused: Npad % 128 != 0 or Npad < Ntok, dtype LSEG_F32, a NULL operand, B, H or Ntok < 1, q / k / vt / o / do / ws not 16-byte aligned.
 *
 * PADDING CONTRACT of the backward (rows Ntok .. Npad-1 of q, k, lse2; columns Ntok .. Npad-1 of every vt row), read from
 * csrc/attention_bwd2.hip.  d_o and d_do [B, Ntok, H*64] have no padding; the prep kernel supplies dO = 0 and D = 0 for padded queries.
 *   k    padded rows: any finite value.  dQ: their probabilities are replaced by 0 and 0 x k stays 0.  dK / dV: their lanes store nothing.
 *   vt   padded columns: any finite value (dQ multiplies dO . v_pad by the probability 0).
 *   q    padded rows: finite AND bounded together with lse2 (next line).  The dK / dV kernel does NOT mask padded queries: they add
 *        P x 0 and 0 x q, which is 0 only while P is finite after its rounding to the operand type and q is finite.
 *   lse2 padded rows: finite, and for every padded row r and every key j < Ntok
 *            q_r . k_j scale log2(e) - lse2[r] <= 15 (fp16) | 127 (bf16),
 *        so that exp2 of it stays finite in the operand type (0 x inf is NaN in the matrix pipe).  lseg_op_attention_ex leaves these
 *        rows unwritten: the caller initialises them once.  All-zero q and lse2 padding -- zero-allocated buffers, as the engine's are --
 *        satisfies this (P = 1).
 *   dqkv [B*Ntok, 3*H*64] has no padding: every element is written.  d_ws is overwritten entirely. */
size_t lseg_op_attention_backward_ws_bytes(int B, int H, int Npad);
int lseg_op_attention_backward_qkv(const void* d_q, const void* d_k, const void* d_vt, const void* d_o, const void* d_do,
                                   const float* d_lse2, void* d_dqkv, void* d_ws, int B, int H, int Ntok, int Npad, int dtype,
                                   float scale, void* stream);

/* Train-mode BatchNorm2d on the padded-NHWC bf16 maps (ResidualConvUnit_custom bn1/bn2 under net.train(),
 * lseg_blocks.py:276-283; the reference runs SyncBatchNorm, i.e. d_stats / the backward sums are what a multi-GPU step
 * all-reduces).  Maps are [B,H+2,W+2,C] with a zero border; statistics over the B*H*W image pixels, biased variance.
 *   forward : d_stats [2C] fp32 = {sum x, sum x^2}; d_y_pad (may be NULL: statistics only) = gamma*(x-mean)*rstd + beta
 *   backward: d_dx_pad = gamma*rstd*(dy - mean(dy) - xhat*mean(dy*xhat)); d_dgamma_dbeta [2C] = {dbeta = sum dy, dgamma = sum dy*xhat}
 * relu_backward: d_dx = d_dy where d_x > 0 (bf16/fp16, n elements). */
int lseg_op_bn_train_forward(const void* d_x_pad, void* d_y_pad, float* d_stats, const float* d_gamma, const float* d_beta,
                             int B, int H, int W, int C, float eps, void* stream);
int lseg_op_bn_train_backward(const void* d_dy_pad, const void* d_x_pad, const float* d_stats, const float* d_gamma, void* d_dx_pad,
                              float* d_dgamma_dbeta, int B, int H, int W, int C, float eps, void* stream);
int lseg_op_relu_backward(const void* d_dy, const void* d_x, void* d_dx, int64_t n, void* stream);

/* The training backward's data-movement kernels (ViT embedding / readout and the DPT neck's resamplers; autograd in the reference), one
 * launch each, for the exact operator tests in tests/test_gpu_train_glue.py.  All refuse (LSEG_ERR_INVALID: NULL pointer or a size
 * below 1; LSEG_ERR_UNSUPPORTED: a channel count the 16-byte lanes cannot cover) before anything is launched.  "16-bit" = bf16 or fp16.
 *   pos_resize           d_out [1+gh*gw, D] fp32 = row 0 of d_pos [1+g_old^2, D] copied, the g_old x g_old grid resized bilinearly
 *                        (align_corners=False, lseg_vit.py:149-163).  The source coordinate max(0, (i+0.5)*(g_old/g)-0.5) is
 *                        evaluated in fp32 as in PyTorch's fp32 resize: it, and so the tap fraction, is off by up to
 *                        3 * 2^-24 * (src+0.5) absolute (not one rounding of the fraction); the tests hold it to that
 *   pos_resize_backward  its transpose, d_dposemb [1+g_old^2, D] += ; d_dcls [D] += d_dpos[0] (d cls_token; may be NULL).  Fixed
 *                        summation order (output y, then x ascending), bit-reproducible
 *   embed_backward       d_gx [B,ntok,D] fp32 -> d_dtok [B*(ntok-1), D] 16-bit = the patch rows rounded to nearest-even,
 *                        d_dpos [ntok, D] fp32 = sum over b (b ascending)
 *   readout_cat          d_x [B,ntok,D] fp32 -> d_cat [B*(ntok-1), 2D] 16-bit = {patch row, cls row} (lseg_vit.py:87-88); D % 8 == 0
 *   readout_cat_backward d_gx [B,ntok,D] fp32: patch rows += d_dcat[:, :D], cls row += sum_p d_dcat[:, D:] (32 interleaved partial
 *                        sums over p, then those in order); D % 8 == 0
 *   unpad_rows           padded NHWC [B,H+2,W+2,C] 16-bit -> rows [B*H*W, C]; C % 8 == 0
 *   dilate2              d_dy_pad [B,Ho+2,Wo+2,C] (Ho = (H-1)/2+1, Wo alike) -> d_dyd_pad [B,H+2,W+2,C], ALL of it zeroed, then
 *                        dyd[2y,2x] = dy[y,x]: the stride-2 3x3 conv's backward is the stride-1 one on dyd; C % 8 == 0
 *   unpixshuf            d_dl_pad [B,gh*s+2,gw*s+2,C] -> d_dg [B*gh*gw, s*s*C], dg[(b,y,x), (i*s+j)*C+c] = dl[b, y*s+i, x*s+j, c]
 *                        (interior coordinates): the ConvTranspose2d(kernel = stride = s) output as GEMM rows; C % 8 == 0
 *   pack_convT           ConvTranspose2d weight [Ci,Co,s,s] fp32 -> GEMM weight d_wp [(i*s+j)*Cp+co, Cp(ci)] in `dtype`; only the
 *                        Ci x Co real entries are written (the caller zeroes the padding once)
 *   convT_wgrad_unpack   the GEMM weight gradient d_dw [s*s*Cp, Cp] fp32 -> d_dst [C,C,s,s] (= or +=), padded rows / columns ignored
 *   conv_wgrad_unpack    d_dst OIHW [Co,Ci,3,3] (= or +=) sum over nsplit slabs of tap-major d_dw [Co_p, 9, Cip], slab s at
 *                        d_dw + s*split_stride (floats), summed s ascending
 *   fold_rows            d_dst[c] (= or +=) sum_{r<R} d_src[r*ld + c], c < C (the ConvTranspose bias gradient: R = s*s, ld = Cp)
 *   sum_partials         d_dst[i] (= or +=) sum_{s<nsplit} d_part[s*stride + i], i < n; n and stride multiples of 4
 *   bn_running_update    train-mode BatchNorm2d's running statistics from d_stats [2C] = {sum x, sum x^2} over `count` elements per
 *                        channel: rmean = (1-m) rmean + m mean, rvar = (1-m) rvar + m var_unbiased, var = max(E[x^2] - mean^2, 0)
 *                        * count/(count-1); at count == 1 there is no unbiased estimate and the (zero) biased variance is used */
int lseg_op_pos_resize(const float* d_pos, float* d_out, int g_old, int gh, int gw, int D, void* stream);
int lseg_op_pos_resize_backward(const float* d_dpos, float* d_dposemb, float* d_dcls, int g_old, int gh, int gw, int D, void* stream);
int lseg_op_embed_backward(const float* d_gx, void* d_dtok, float* d_dpos, int B, int ntok, int D, int dtype, void* stream);
int lseg_op_readout_cat(const float* d_x, void* d_cat, int B, int ntok, int D, int dtype, void* stream);
int lseg_op_readout_cat_backward(const void* d_dcat, float* d_gx, int B, int ntok, int D, int dtype, void* stream);
int lseg_op_unpad_rows(const void* d_in_pad, void* d_rows, int B, int H, int W, int C, void* stream);
int lseg_op_dilate2(const void* d_dy_pad, void* d_dyd_pad, int B, int H, int W, int C, void* stream);
int lseg_op_unpixshuf(const void* d_dl_pad, void* d_dg, int B, int gh, int gw, int s, int C, void* stream);
int lseg_op_pack_convT(const float* d_w, void* d_wp, int Ci, int Co, int Cp, int s, int dtype, void* stream);
int lseg_op_convT_wgrad_unpack(const float* d_dw, float* d_dst, int C, int Cp, int s, int accumulate, void* stream);
int lseg_op_conv_wgrad_unpack(const float* d_dw, float* d_dst, int Co, int Ci, int Cip, int accumulate, int nsplit, size_t split_stride,
                              void* stream);
int lseg_op_fold_rows(const float* d_src, float* d_dst, int R, int C, int ld, int accumulate, void* stream);
int lseg_op_sum_partials(const float* d_part, float* d_dst, int nsplit, size_t n, size_t stride, int accumulate, void* stream);
int lseg_op_bn_running_update(const float* d_stats, float* d_rmean, float* d_rvar, int C, double count, float momentum, void* stream);

/* Head-side backward bricks (lseg_net.py:185-203 under autograd):
 *   upsample2x_planes_backward_rows  d_dout [B,K,2H,2W] fp32 (d of the output logits) -> d_rows [B*H*W, ldk] bf16/fp16, columns
 *                                    0..K-1 (the rest pre-zeroed by the caller): transpose of output_conv's x2 bilinear, already in
 *                                    the row layout the correlation backward (lseg_op_linear_backward with N = ldk) consumes
 *   l2norm_scale_backward            d_dx [M,C] = (scale/||x||) (d_da - xh (xh . d_da)), xh = x/||x||; x fp32, da/dx bf16|fp16 */
int lseg_op_upsample2x_planes_backward_rows(const float* d_dout, void* d_rows, int B, int K, int H, int W, int ldk, int out_dtype,
                                            void* stream);
int lseg_op_l2norm_scale_backward(const void* d_da, int da_dtype, const float* d_x, void* d_dx, int dx_dtype, int M, int C, float scale,
                                  void* stream);
/* Per-image label sets on the training path (LSegNetZS, lseg_net_zs.py:198-208; csrc/corr_group.hip), G = labels per image, 1..8.
 * corr_group_fwd: d_low fp32 [B,G,hw] (fp16 values) = fp16(d_a16 fp16 [B*hw,C] . d_tnorm fp16 [B*G,C]^T) per image, fp32 accumulation
 *   (the rounding points of the shared label set's correlation GEMM in the train-mode forward).
 * corr_group_bwd: d_df [B*hw,C] (df_dtype, 16-bit) = backward of a = scale * f / ||f|| (d_feat fp32 [B*hw,C]) for
 *   dA = rt(sum_k d_rows[row,k] T[b*G+k]) (fp32 accumulation, rt = rounding to rows_dtype); rows_dtype fp16: the gradient reaching f is
 *   fp16(scale * dA) (the reference's half-precision head gradient), bf16: T is rounded to bf16 and the scale applied un-rounded
 *   (lseg_config.flags bit 1).  d_rows [B*hw, ldk] 16-bit, ldk % 8 == 0, columns >= G ignored.  == lseg_op_gemm + lseg_op_l2norm_scale_backward
 *   on the same operands, without dA in memory. */
int lseg_op_corr_group_fwd(const void* d_a16, const void* d_tnorm, float* d_low, int B, int hw, int G, int C, void* stream);
int lseg_op_corr_group_bwd(const void* d_rows, int rows_dtype, int ldk, const void* d_tnorm, const float* d_feat, void* d_df, int df_dtype,
                           int B, int hw, int G, int C, float scale, void* stream);
/* Fused backward of the loss the reference takes on the full-resolution logits -- CrossEntropyLoss(ignore_index)(output_conv(low)),
 * lsegmentation_module.py:72 on lseg_net.py:203 -- from the LOW-resolution logits d_low fp32 [B,K,h,w] and the target mask int64
 * [B,2h,2w]: the x2 bilinear, the softmax and the bilinear's transpose in registers, so the [B,K,2h,2w] logits and their gradient
 * (2 x 138 MB per image at K = 150, 480x480) never exist.  Outputs: d_nll double [2] = {sum of -log_softmax[target] over the valid
 * pixels, number of valid pixels} (the loss is their ratio), d_rows [B*h*w, ldk] bf16|fp16 = d loss / d low in the row layout the
 * correlation backward consumes (all ldk columns written, zeros beyond K; ldk % 8 == 0), d_lse_ws fp32 [B*2h*2w] scratch. */
int lseg_op_upsample_ce_backward_rows(const float* d_low, const int64_t* d_target, int B, int K, int h, int w, int ignore_index,
                                      double* d_nll, float* d_lse_ws, void* d_rows, int ldk, int out_dtype, void* stream);
/* The ragged forms of the two loss kernels (csrc/ragged_train.hip), for per-image label lists of any lengths: host_counts int32 [B] on the
 * host, each in [1, 32767]; d_low fp32 = the images' planes CONCATENATED, image b's [k_b,h,w] at prefix[b] * h * w floats (prefix = the
 * exclusive prefix sum of the counts); d_target int64 [B,2h,2w] with values in [0, k_b) or ignore_index for image b (anything else
 * contributes no loss); d_prefix int32 [B + 1] device scratch the call fills on the stream.
 *   ragged_ce_fwd       d_nll double [2] = {sum of -log_softmax[target] over the valid pixels of the batch, their number}, d_counts2
 *                       int64 [2] = {correct, labeled} of the arg-max through the x2 bilinear (lseg_op_seg_stats_lowres' rule), d_lse
 *                       fp32 [B*2h*2w] = the per-pixel log-sum-exp over the image's own labels.
 *   ragged_ce_bwd_rows  runs the forward, then d_rows [B*h*w, ldk] bf16|fp16 = d loss / d low with ONE row pitch for the batch
 *                       (ldk % 8 == 0, >= the largest count); columns >= k_b of image b's rows are exactly zero.  1 / (valid pixels) is
 *                       the batch count; d_grad_scale (device float, or NULL = 1) multiplies the gradient.
 *   ragged_ce_plan      host only, no device: out8 = {labels in all, largest count, up64(largest count) = the engine's row pitch,
 *                       workgroups of the forward, workgroups of the backward, lanes per workgroup, sum of up64(k_b) = columns of the
 *                       per-image transposed text panels of the correlation backward, fp32 values of the concatenated planes}. */
/* The correlation of the ragged training step (csrc/ragged_train.hip), in its two stages.  `stage`: 1 = per-image launches of the generic
 * GEMM (the fallback and the yardstick; the engine takes it when the environment variable LSEG_CORR_RAGGED_GEMM is set), 2 = ONE launch
 * for the whole batch, 0 = whichever the engine takes.  C % 64 == 0, C <= 1024.
 *   corr_ragged_fwd   d_low (concatenated planes, fp32 holding fp16 values) = fp16(d_a16 fp16 [B*hw,C] . d_tnorm fp16 [sum k_b, C]^T) per
 *                     image against its own rows, fp32 accumulation, one fp16 rounding per logit (the shared set's rounding points).
 *                     Stage 2: text rows through LDS in panels of 16 labels, pixel rows read once, v_mfma_f32_16x16x32_f16 over
 *                     ascending k with the generic GEMM's operand roles -- planes bit-equal to stage 1.
 *   corr_ragged_bwd   d_df [B*hw,C] (df_dtype, 16-bit) = backward of a = scale * f / ||f|| (d_feat fp32 [B*hw,C]) for dA_b = rt(d_rows_b .
 *                     T_b), with lseg_op_corr_group_bwd's conventions for rows_dtype (fp16: fp16(scale * dA); bf16: T rounded to bf16, the
 *                     scale un-rounded).  d_rows [B*hw, ldk], ldk % 64 == 0 and >= up64(largest count); columns >= k_b must be zero.
 *                     Stage 1: per-image transposed text panels [C, up64(k_b)] and dA in scratch allocated on the stream, B GEMMs + one
 *                     L2-norm backward.  Stage 2: dA in fp32 fused multiply-adds over ascending labels (text rows through LDS in panels
 *                     of 16), the scale and the L2-norm backward fused as in corr_group_bwd with its row reductions: no dA in memory.
 *   corr_ragged_plan  host only: out8 = {stage-1 forward launches, stage-1 backward launches, panel columns = sum of up64(k_b),
 *                     up64(largest count), labels in all, B*hw*C, stage-2 forward workgroups (64 pixel rows each), stage-2 backward
 *                     workgroups (16 pixel rows each)}. */
int lseg_op_corr_ragged_plan(const int32_t* host_counts, int B, int hw, int C, int* out8);
int lseg_op_corr_ragged_fwd(const void* d_a16, const void* d_tnorm, float* d_low, const int32_t* host_counts, int B, int hw, int C, int stage,
                            void* stream);
int lseg_op_corr_ragged_bwd(const void* d_rows, int rows_dtype, int ldk, const void* d_tnorm, const float* d_feat, void* d_df, int df_dtype,
                            const int32_t* host_counts, int B, int hw, int C, float scale, int stage, void* stream);
int lseg_op_ragged_ce_plan(const int32_t* host_counts, int B, int h, int w, int* out8);
int lseg_op_ragged_ce_fwd(const float* d_low, const int64_t* d_target, const int32_t* host_counts, int* d_prefix, int B, int h, int w,
                          int ignore_index, double* d_nll, int64_t* d_counts2, float* d_lse, void* stream);
int lseg_op_ragged_ce_bwd_rows(const float* d_low, const int64_t* d_target, const int32_t* host_counts, int* d_prefix, int B, int h, int w,
                               int ignore_index, double* d_nll, float* d_lse_ws, void* d_rows, int ldk, int out_dtype,
                               const float* d_grad_scale, void* stream);
/* The same gradient as fp32 PLANES d_planes [B,K,h,w] (the input of the head blocks' backward) and, if d_ksum is not NULL, its per-pixel
 * sum over the labels d_ksum [B,h,w] (what a bottleneck block routes to its arg-max label).  Rounded to fp16 and transposed, d_planes
 * equals the d_rows of lseg_op_upsample_ce_backward_rows. */
int lseg_op_upsample_ce_backward_planes(const float* d_low, const int64_t* d_target, int B, int K, int h, int w, int ignore_index,
                                        double* d_nll, float* d_lse_ws, float* d_planes, float* d_ksum, void* stream);
/* Backward of ONE arch_option 1/2 head block (lseg_net.py:43-79; csrc/head_train.hip) on fp32 planes [B,K,H,W]:
 *   forward  z = conv2d(in[b,k], w9 [3x3], bias) (+ max_k in[b,:,p] if bottleneck),  out = act(z) if apply_act else z
 *   d_dy = d out; d_out_saved = out (needed when apply_act; act 0 relu, 1 leaky_relu(0.01), 2 tanh, derivative from the output).
 *   d_dx: dx_dtype LSEG_F32 = planes [B,K,H,W]; LSEG_F16 / LSEG_BF16 = rows [B*H*W, ldk] (ldk % 8 == 0, >= K, zeros beyond K), the
 *   layout and rounding the correlation backward reads.  The bottleneck's max routes sum_k dz[b,k,p] to the FIRST maximal k (torch.max).
 *   d_dw [9], d_db [1]: written (accumulate 0) or added to (accumulate 1), summed in a fixed order (bit-reproducible).
 *   d_ws (optional, ws_floats >= lseg_op_head_block_backward_ws(...) floats): scratch; NULL = allocated on the stream. */
size_t lseg_op_head_block_backward_ws(int B, int K, int H, int W, int apply_act);
int lseg_op_head_block_backward(const float* d_in, const float* d_out_saved, const float* d_dy, const float* d_w9, int B, int K, int H, int W,
                                int bottleneck, int act, int apply_act, void* d_dx, int dx_dtype, int ldk, float* d_dw, float* d_db,
                                int accumulate, float* d_ws, int64_t ws_floats, void* stream);

/* ---- training step ------------------------------------------------------------------------------------------------------------
 * replaces: LSegmentationModule.training_step (modules/lsegmentation_module.py:66-81) -- `out = self(img)` in train() mode,
 * `loss = criterion(out, target)` (SegmentationLosses = CrossEntropyLoss(ignore_index), [3P] encoding/nn/loss.py), autograd's
 * backward -- plus what the Trainer does around it: DistributedDataParallel's bucketed gradient all-reduce and SyncBatchNorm
 * (utils.py:20-22,34) through two callbacks, and SGD with the two learning-rate groups of configure_optimizers (:119-127,165-171).
 *
 *   lseg_set_train(h, 1)   net.train(): lseg_forward keeps the activations the backward needs, the refinenets' BatchNorm uses batch
 *                          statistics and updates running_mean / running_var IN the caller's bound tensors (momentum 0.1).  bf16 only.
 *                          ResNet-101 tower (flags bit 5): LSEG_ERR_UNSUPPORTED unless flags bit 6 is set; with it the tower's BatchNorms
 *                          run on batch statistics too and the step trains scratch.* only (see flags bit 6).
 *                          arch_option 1/2 (head blocks) needs lseg_config.flags bit 4, else LSEG_ERR_UNSUPPORTED.
 *                          Ragged per-image label lists (lseg_set_text_groups) may be set before or after: the fused-loss route then
 *                          runs per image (see lseg_set_text_groups); with them set, arch_option 1/2 and the ResNet-101 tower
 *                          are refused here and at the forward.  flags bit 3 holds as for a shared set: the ragged loss kernels
 *                          have no fp32 atomics, the gradients are bit-reproducible.
 *   lseg_bind_grad         where the gradient of parameter `key` is written: fp32, same shape/layout as the bound parameter (the
 *                          caller's .grad tensor, typically a view into a flat bucket).  Unbound parameters get engine-owned buffers
 *                          (lseg_grad_ptr).  Trainable = pretrained.* and scratch.* tensors the forward touches; the CLIP text tower
 *                          is frozen (it is in no optimizer group of the reference) and its features are constants of the step.
 *   lseg_backward          after a train-mode lseg_forward: either dev_dlogits fp32 [B,K,H,W] ([B,k,H,W] with per-image label sets) (autograd hands it over), or
 *                          dev_target int64 [B,H,W] (then the loss is the mean CE over pixels != ignore_index and dev_loss, if not
 *                          NULL, receives double[2] = {sum of -log p[target], number of valid pixels}).  accumulate != 0 adds to the
 *                          gradient buffers (accumulate_grad_batches), 0 overwrites them.
 *   lseg_train_loss        the criterion's VALUE on the last train-mode forward (`loss = self.criterion(out, target)`, :72) without the
 *                          backward: dev_loss double[2] as above, dev_counts (or NULL) int64[2] = {correct, labeled} of the arg-max
 *                          mask on the valid pixels (`train_accuracy`, :76-79).  A following lseg_backward / lseg_backward_scaled on
 *                          the same target reuses its per-pixel log-sum-exp.
 *   lseg_backward_scaled   lseg_backward(target) whose d(logits) is multiplied by *dev_grad_scale (a float in device memory, read by
 *                          the kernel: no host synchronisation) -- the d(loss) autograd hands to `loss.backward()` (:81 via Lightning).
 *   lseg_grad_bucket       gradients complete in buckets: 0 = DPT head + reassemble, 1+j = ViT block depth-1-j (+ the readout hooked
 *                          on it), the last one also patch_embed / cls_token / pos_embed.  The bucket callback fires on the host right
 *                          after the last kernel of a bucket has been ENQUEUED on `stream` (record an event there and launch the
 *                          all-reduce on a side stream: it overlaps the remaining backward GEMMs).
 *   lseg_set_bn_sync       SyncBatchNorm: `fn(user, dev_ptr, n, stream)` must sum dev_ptr[0..n) over the ranks in place, ordered on
 *                          `stream`; called for the 2C batch sums of every BatchNorm (forward) and the 2C gradient sums (backward).
 *                          world_size = number of ranks (divides the sums).  NULL / 1 = per-GPU statistics.
 *   lseg_sgd_step          w -= lr * (mu * m + g + wd * w) on the bound fp32 parameters with the engine's momentum buffers, then
 *                          re-packs the MFMA operand copies.
 *   lseg_sgd_momentum      device pointer of a parameter's momentum buffer (torch.optim.SGD's state['momentum_buffer'], what
 *                          Lightning checkpoints under 'optimizer_states'); lseg_sgd_mark_initialized(h, 1) after restoring them makes
 *                          the next step a regular one (the first step of SGD copies the gradient into the buffer instead).
 *   lseg_adam_step         replaces torch.optim.Adam(params_list, lr=base_lr, betas=(0.9, 0.999), weight_decay=...) of the --midasproto
 *                          protocol (modules/lsegmentation_module.py:152-163, modules/lsegmentation_module_zs.py:270-281), amsgrad and
 *                          maximize off: g += wd*w; m = b1*m + (1-b1)*g; v = b2*v + (1-b2)*g*g;
 *                          w -= lr / (1-b1^step) * m / (sqrt(v) / sqrt(1-b2^step) + eps) on the bound fp32 parameters in one launch that
 *                          also writes the same-layout MFMA operand copies, then the partial re-pack of lseg_sgd_step.  `step` is the
 *                          count of THIS step (torch's state['step'] after it, >= 1); the hyper-parameters are doubles because torch
 *                          derives the bias corrections from Python floats.  A group at lr 0 still moves m and v; w is not written.
 *   lseg_adam_state        device pointer of a parameter's exp_avg (which = 0) / exp_avg_sq (which = 1), torch.optim.Adam's state under
 *                          those names; both start at zero.  Mirrors lseg_sgd_momentum.
 *   lseg_set_frozen_encoder  replaces the `pretrained.model` group at lr = 0 of use_pretrained='clip_fixed'
 *                          (modules/lsegmentation_module_zs.py:220-235), which still pays the whole ViT backward: with it enabled
 *                          pretrained.model.* is not trainable -- lseg_grad_bucket returns -1 for it, it gets no gradient buffer and
 *                          no optimizer state, lseg_sgd_step / lseg_adam_step skip it -- and lseg_backward* stops after the four
 *                          ProjectReadouts' own gradients (no timm Block, attention or embedding backward).  Every bucket callback still
 *                          fires once, in order; pretrained.act_postprocess* take lr_pretrained, scratch.* lr_scratch.  The train-mode
 *                          forward computes the same logits, bit for bit, and keeps one block's activations instead of `depth`.
 *                          Legal only before the first lseg_set_train(h, 1) (afterwards LSEG_ERR_STATE); LSEG_ERR_UNSUPPORTED on the
 *                          ResNet-101 tower. */
typedef void (*lseg_reduce_cb)(void* user, void* dev_ptr, int64_t n_floats, void* stream);
typedef void (*lseg_bucket_cb)(void* user, int bucket, void* stream);
int lseg_set_train(lseg_handle h, int enabled);
int lseg_bind_grad(lseg_handle h, const char* key, float* dev_grad);
int lseg_grad_ptr(lseg_handle h, const char* key, float** dev_out, size_t* n_elems);
int lseg_grad_bucket(lseg_handle h, const char* key);          /* bucket index, or -1 if `key` is not a trainable parameter */
int lseg_num_grad_buckets(lseg_handle h);
int lseg_backward(lseg_handle h, const float* dev_dlogits, const int64_t* dev_target, int ignore_index, int accumulate,
                  double* dev_loss, void* stream);
int lseg_train_loss(lseg_handle h, const int64_t* dev_target, int ignore_index, double* dev_loss, int64_t* dev_counts, void* stream);
int lseg_backward_scaled(lseg_handle h, const int64_t* dev_target, int ignore_index, int accumulate, const float* dev_grad_scale, void* stream);
int lseg_sgd_momentum(lseg_handle h, const char* key, float** dev_out, size_t* n_elems);
int lseg_sgd_mark_initialized(lseg_handle h, int initialized);
int lseg_set_bn_sync(lseg_handle h, lseg_reduce_cb fn, void* user, int world_size);
int lseg_set_bucket_callback(lseg_handle h, lseg_bucket_cb fn, void* user);
int lseg_sgd_step(lseg_handle h, float lr_pretrained, float lr_scratch, float momentum, float weight_decay, void* stream);
int lseg_adam_step(lseg_handle h, double lr_pretrained, double lr_scratch, double beta1, double beta2, double eps, double weight_decay,
                   int64_t step, void* stream);
int lseg_adam_state(lseg_handle h, const char* key, int which /* 0 = exp_avg, 1 = exp_avg_sq */, float** dev_out, size_t* n_elems);
int lseg_set_frozen_encoder(lseg_handle h, int enabled);

#ifdef __cplusplus
}
#endif
#endif /* LSEG_HIP_H */
