// ops.h -- host-side launchers of every kernel in the engine (all stream-ordered, return 0 or <0).
#pragma once
#include "common.h"
#include "gemm.h"

namespace lseg {

inline size_t up64(size_t v) { return (v + 63) / 64 * 64; }       // a count rounded up to the GEMM's K-step

int launch_attention(const void* q, const void* k, const void* vt, void* out, int B, int H, int ntok,
                     int npad, int dtype, int causal, float scale, hipStream_t stream);

int launch_layernorm(const void* in, int in_dtype, const float* gamma, const float* beta, void* out, int out_dtype,
                     int M, int D, float eps, hipStream_t st);
// x += bias + sum of `nsplit` split-K partial slabs (`stride` floats apart), then LayerNorm of the updated rows (gamma NULL: update only)
int launch_layernorm_reduce(float* x, const float* part, int nsplit, size_t stride, const float* bias, const float* gamma, const float* beta,
                            void* out, int out_dtype, int M, int D, float eps, hipStream_t st);
// epilogue of a split-K 3x3 conv: sum of `ns` fp32 slabs [B*Ho*Wo, C] + bias, ReLU, skip inputs -> padded NHWC map (+ its ReLU copy);
// relu_after_res: the ReLU after the skip add (ResNet bottleneck) instead of before it
int launch_conv_reduce_pad(const float* part, int ns, size_t stride, const float* bias, const void* res, const void* res2, void* out, void* out_relu,
                           int B, int Ho, int Wo, int C, int relu, int dtype, hipStream_t st, int relu_after_res = 0);
// split-K plan of a small-batch conv [M x N] over K (engine.hip, Engine::conv3x3): *ns slabs of *steps 64-wide K-steps (the last range possibly
// shorter), slabs within ws_floats; *ns = 1: the conv runs unsplit.  Host only.
void conv_splitk_plan(int M, int N, int K, size_t ws_floats, int* ns, int* steps);
int launch_im2col_patch(const float* x, void* A, int B, int H, int W, int P, int dtype, hipStream_t st);
int launch_pos_resize(const float* pos, float* out, int g_old, int gh, int gw, int D, hipStream_t st);
int launch_cls_rows(const float* cls, const float* pos, float* x, int B, int ntok, int D, hipStream_t st);
int launch_readout_cat(const float* x, void* A, int B, int ntok, int D, int dtype, hipStream_t st);
int launch_upsample2x_nhwc(const void* in, void* out, int B, int H, int W, int C, int dtype, hipStream_t st);
int launch_upsample2x_planes(const float* in, float* out, int P, int H, int W, hipStream_t st);
int launch_combine_1x1(const float* wh, const float* bh, const float* wo, const float* bo, float* wc, float* bc, int Co, int Cm, int Ci,
                       hipStream_t st);
int launch_pixel_gram(const void* g16, float* gram, int B, int H, int W, int C, hipStream_t st);
int launch_norm_scale_plane(const float* gram, float* scale, int B, int H, int W, float s, hipStream_t st, unsigned* flag = nullptr);
int launch_upsample2x_planes_scaled(const float* in_padded, const float* scale, float* out, int P, int K, int H, int W, hipStream_t st);
int launch_upsample4x_planes_scaled(const float* in_padded, const float* scale, float* out, int P, int K, int H, int W, hipStream_t st);
int launch_upsample_norm_f16(const float* g, void* a, int B, int H, int W, int C, float scale, hipStream_t st);
int launch_l2norm_scale_f16(const float* f, void* a, int M, int C, float scale, hipStream_t st);
int launch_text_embed(const int64_t* tok, const float* emb, const float* pos, void* x, int rows, int L, int ctx, int W, hipStream_t st);
int launch_text_pool(const void* x, const int* eot, void* pooled, int K, int L, int W, hipStream_t st);
int launch_text_l2norm(const void* t, void* out, int K, int C, hipStream_t st);
int launch_convert(const void* in, int in_dtype, void* out, int out_dtype, size_t n, hipStream_t st);
int launch_range16(const void* p, size_t n, int dtype, unsigned long long* out4, hipStream_t st);
int launch_convert2d(const void* in, int in_dtype, void* out, int out_dtype, int R, int C, int ld, hipStream_t st);
int launch_transpose_convert(const void* in, int in_dtype, void* out, int out_dtype, int R, int C, hipStream_t st);
int launch_pack_conv3x3(const float* w, const float* bn_w, const float* bn_b, const float* bn_m, const float* bn_v,
                        float bn_eps, const float* conv_bias, void* wp, float* bias_out, int Co, int Ci, int Cip, int dtype,
                        hipStream_t st);      // dtype DT_F32: wp is a float buffer (split-precision packs go through fp32)
int launch_pack_convT(const float* w, void* wp, int Ci, int Co, int Cp, int s, int dtype, hipStream_t st);
int launch_nhwc_to_nchw_f32(const void* in, float* out, int B, int H, int W, int C, int Cs, int pad, int dtype, hipStream_t st, size_t lo_plane = 0);
int launch_rows_to_nchw_f32(const float* in, float* out, int B, int HW, int C, hipStream_t st);
int launch_head_block(const float* in, float* out, const float* w9, const float* bias, int B, int K, int H, int W,
                      int bottleneck, int act, int apply_act, hipStream_t st);
int launch_argmax_planes(const float* in, uint8_t* out, int B, int K, int HW, hipStream_t st);
int launch_layernorm_backward(const void* dy, int dy_dtype, const float* x, const float* gamma, float* dx, float* dgamma,
                              float* dbeta, int M, int D, float eps, int accumulate, hipStream_t st, int accumulate_params = 0,
                              float* partial_ws = nullptr,       // partial_ws: [LN_BWD_PARTIAL_BLOCKS, 2D] floats -> no atomics
                              void* dx16 = nullptr);             // optional 16-bit copy (dy's type) of the updated dx
constexpr int LN_BWD_PARTIAL_BLOCKS = 1024;
int launch_transpose16(const void* in, void* out, int R, int C, int ldi, int ldo, hipStream_t st, int shift = 0, int relu = 0);
int launch_bn_train_forward(const void* x, void* y, float* stats, const float* gamma, const float* beta, int B, int H, int W, int C,
                            float eps, int dtype, hipStream_t st);
int launch_bn_train_backward(const void* dy, const void* x, const float* stats, const float* gamma, void* dx, float* bstats,
                             int B, int H, int W, int C, float eps, int dtype, hipStream_t st);
int launch_relu_backward(const void* dy, const void* x, void* dx, size_t n, hipStream_t st);
int launch_upsample2x_planes_backward_rows(const float* dout, void* rows, int B, int K, int H, int W, int ldk, int dtype, hipStream_t st);
// the same transpose written as fp32 planes [B,K,H,W] (the head blocks' backward input)
int launch_upsample2x_planes_backward_planes(const float* dout, float* planes, int B, int K, int H, int W, hipStream_t st);
// head_train.hip -- arch_option 1/2 head blocks on the training path (lseg_net.py:43-79,198-201)
// forward of one block = launch_head_block's arithmetic, plus kstar [B,H,W] = first arg-max label of `in` (bottleneck; may be NULL)
int launch_head_block_train(const float* in, float* out, int* kstar, const float* w9, const float* bias, int B, int K, int H, int W,
                            int bottleneck, int act, int apply_act, hipStream_t st);
// per pixel: dz = act'(y) dy (apply_act) or dy (dz optional, may alias dy), ksum = sum_k dz, kstar = first arg-max of x (each optional)
int launch_head_bwd_prep(const float* dy, const float* y, const float* x, float* dz, float* ksum, int* kstar, int B, int K, int HW, int act,
                         int apply_act, hipStream_t st);
// partial rows of 10 floats one launch_head_block_backward writes
size_t head_block_bwd_partials(int B, int H, int W);
// backward of one block from dz (its pre-activation gradient): dx -> fp32 planes (out_dtype DT_F32; times act'(x) when lower_act >= 0,
// label sums in ksum_out) or 16-bit rows [B*H*W, ldk]; {dW, db} partial rows -> partial
int launch_head_block_backward(const float* dz, const float* ksum, const int* kstar, const float* x, const float* w9, void* out, int out_dtype,
                               int ldk, int lower_act, float* ksum_out, float* partial, int B, int K, int H, int W, int bottleneck, hipStream_t st);
// dW[9], db[1] (+)= fixed-order sum of nrows partial rows
int launch_head_dw_reduce(const float* partial, int nrows, float* dW, float* db, int accumulate, hipStream_t st);
// corr_group.hip -- per-image label sets (LSegNetZS, lseg_net_zs.py:198-208) on the training path: G = labels per image, 1..CORR_GROUP_MAX
constexpr int CORR_GROUP_MAX = 8;
bool corr_group_supported(int G, int C);
// low [B, G, hw] fp32 (fp16 values) = fp16(a16 [B*hw, C] . tnorm [B*G, C]^T per image), fp32 accumulation
int launch_corr_group_fwd(const void* a16, const void* tnorm, float* low, int B, int hw, int G, int C, hipStream_t st);
// df [B*hw, C] = L2-norm/scale backward (feat fp32) of dA = sum_k rows[:, k] T[b*G + k] -- the shared path's GEMM + l2norm_scale_backward
int launch_corr_group_bwd(const void* rows, int rows_dtype, int ldk, const void* tnorm, const float* feat, void* df, int df_dtype, int B, int hw,
                          int G, int C, float scale, hipStream_t st);
// ragged_train.hip -- the loss of the training step for ragged per-image label sets: planes of image b at prefix[b] * h * w of `low`
// prefix [B + 1] (host) = exclusive prefix sum of the validated counts (each in [1, 32767]); kmax = the largest count
int ragged_prefix(const int32_t* host_counts, int B, int* prefix, int& kmax);
// launch geometry without a device: out8 = {labels in all, largest count, drows pitch up64(largest), forward workgroups, backward
// workgroups, lanes per workgroup, columns of the per-image transposed text panels (sum of up64(k_b)), fp32 values of the planes}
int ragged_ce_plan(const int32_t* host_counts, int B, int h, int w, int* out8);
// the 4-tap footprint of the x2 bilinear's transpose both fused CE backward kernels assume (elementwise.hip), checked per geometry
bool x2_footprint_is_4(int H);
// the per-image correlation of the ragged step on the generic GEMM (see ragged_train.hip): forward planes, transposed text panels, dA + L2-norm backward
bool corr_ragged_supported(int C);
int corr_ragged_plan(const int32_t* host_counts, int B, int hw, int C, int* out8);
int launch_corr_ragged_fwd(const void* a16, const void* tnorm, float* low, const int* host_prefix, int B, int hw, int C, hipStream_t st);
// stage two: one launch for the batch each way (d_prefix on the device); LSEG_CORR_RAGGED_GEMM selects stage one instead
bool corr_ragged_use_gemm();
int launch_corr_ragged_fwd_fused(const void* a16, const void* tnorm, float* low, const int* d_prefix, int B, int hw, int C, hipStream_t st);
int launch_corr_ragged_bwd_fused(const void* rows, int rows_dtype, int ldk, const void* tnorm, const float* feat, void* df, int df_dtype,
                                 const int* d_prefix, int kmax, int B, int hw, int C, float scale, hipStream_t st);
int launch_corr_ragged_panels(const void* tsrc, void* tnT, const int* host_prefix, int B, int C, hipStream_t st);
int launch_corr_ragged_bwd(const void* rows, int rows_dtype, int ldk, const void* tnT, const float* zero_bias, const float* feat, void* da,
                           void* df, int df_dtype, const int* host_prefix, int B, int hw, int C, float scale, hipStream_t st);
int launch_ragged_offsets(int* d_prefix, const int* host_prefix, int n, hipStream_t st);
int launch_ragged_ce_fwd(const float* low, const int64_t* target, const int* d_prefix, int B, int h, int w, int ignore_index,
                         unsigned long long* counts2, double* nll, float* lse_out, hipStream_t st);
int launch_ragged_ce_bwd_rows(const float* low, const int64_t* target, const float* lse, const double* nll, void* rows, const int* d_prefix,
                              int B, int h, int w, int ldk, int ignore_index, int dtype, hipStream_t st, const float* gscale = nullptr);
int launch_l2norm_scale_backward(const void* da, int da_dtype, const float* x, void* dx, int dx_dtype, int M, int C, float scale, hipStream_t st);
int launch_gelu_backward(const void* dy, const void* pre, void* dx, size_t n, int dtype, hipStream_t st, int quick = 0);
int launch_upsample2x_nhwc_backward(const void* dout, void* din, int B, int H, int W, int C, int dtype, hipStream_t st);
int launch_softmax_ce_backward(const float* scores, const int64_t* target, float* dz, int B, int K, int HW, int ignore_index,
                               const double* nll, hipStream_t st);
int launch_conv_dgrad_pack(const void* wp, void* wd, int Co, int Ci, hipStream_t st);
// det_ws (optional, det_cap floats): deterministic reductions -- partial rows + a fixed-order sum instead of fp32 atomics
int launch_colsum16(const void* in, int dtype, float* out, int R, int C, int ld, hipStream_t st, int accumulate = 0,
                    float* det_ws = nullptr, size_t det_cap = 0);
int launch_relu_backward_add(const void* dy, const void* x, const void* add, void* dx, size_t n, int dtype, hipStream_t st);
int launch_seg_stats_ex(const float* scores, const int64_t* target, int B, int K, int HW, int ignore_index, unsigned long long* counts,
                        double* nll, uint8_t* argmax_out, int up, int h, int w, hipStream_t st, float* lse_out = nullptr);
int launch_upsample_ce_backward_rows(const float* low, const int64_t* target, const float* lse, const double* nll, void* rows, int B, int K,
                                     int H, int W, int ldk, int ignore_index, int dtype, hipStream_t st, const float* gscale = nullptr);
// the same gradient as fp32 planes [B,K,H,W] and (ksum, optional) its per-pixel sum over the labels
int launch_upsample_ce_backward_planes(const float* low, const int64_t* target, const float* lse, const double* nll, float* planes, float* ksum,
                                       int B, int K, int H, int W, int ignore_index, hipStream_t st, const float* gscale = nullptr);
int launch_seg_stats(const float* scores, const int64_t* target, int B, int K, int HW, int ignore_index,
                     unsigned long long* counts, double* nll, hipStream_t st);
// corr_argmax.hip -- masks for any K <= 32767.  The streamed kernel: g padded NHWC fp16 [B, H+2, W+2, 512], T fp16 [K, 512], scale fp32
// [B, 2H, 2W] (launch_norm_scale_plane) -> label int16 / score fp32 (optional) [B, 4H, 4W], no label planes in memory
bool corr_argmax_supported(int K, int C);
void corr_argmax_geometry(int* out8);
// The outputs of the route, each the maps' shape: label int16 always; score fp32, and for label confidence the runner-up (label2 int16 /
// score2 fp32: entry 1 of a stable descending sort over k; -1 / -inf when K = 1) and lse fp32 = log-sum-exp over all K, each optional.
// tlogit belongs to the loss form: the launchers take it from CorrLoss, callers leave it NULL
struct CorrOut { int16_t* label; float* score; int16_t* label2; float* score2; float* lse; float* tlogit; };
// the cross-entropy (no runner-up with it): beside label / score / lse, tlogit fp32 = the logit of the pixel's target label (-inf where the
// target is not valid: == ignore_index or outside [0, K), ragged: [0, count_b)), nll_plane fp32 = lse - tlogit (0 where not valid) and
// nll double [2] = {sum over the valid pixels of double(lse) - double(tlogit), their number} in a fixed order (partial: corr_loss_plan's
// bytes of device scratch).  tlogit / nll_plane / nll each optional; the sum and the plane read the lse and tlogit planes, so those must
// be given with either.  target int64, the maps' shape
struct CorrLoss { const int64_t* target; int ignore_index; float* tlogit; float* nll_plane; double* nll; double* partial; };
void corr_loss_plan(size_t npix, int64_t* out4);          // host only: {threads, pixels per workgroup, workgroups, bytes of partials}
size_t corr_loss_partial_bytes_max();                     // the partials of the largest plan
// the ONE streamed entry, maps [B, 4H, 4W].  What is asked for selects the kernel's mode: loss = the cross-entropy form, else any of
// label2 / score2 / lse = label confidence, else the arg-max.  ws (optional): room for the label parts of a tile, per part and output
// pixel the planes of the mode (ca_part_bytes there: 6 / 16 / 14 bytes).  host_counts / d_offsets (both or neither) = ragged per-image label sets: image
// b against host_counts[b] consecutive rows of T, labels local to its list; host_counts int32 [B] on the host (each in [1, 32767]),
// d_offsets int32 [B + 1] device scratch, filled with their prefix sum on the stream; K is unused, the parts are sized from the largest count
int launch_corr_argmax(const void* g, const void* T, const float* scale, const CorrOut& out, int B, int K, int H, int W, int C, hipStream_t st,
                       void* ws = nullptr, size_t ws_bytes = 0, const CorrLoss* loss = nullptr, const int32_t* host_counts = nullptr,
                       int* d_offsets = nullptr);
// host only: out2 = {label parts, labels per part} of a ragged launch when it plans for `cus` compute units
int corr_argmax_ragged_split(const int32_t* host_counts, int B, int H, int W, int conf, size_t ws_bytes, int cus, int* out2);
// the ONE fallback entry, the same outputs in the same modes from planes in memory (the int16 form of launch_seg_stats_ex's mask output,
// up = 1): low fp32 [B, K, h, w] -> maps [B, 2h, 2w]
int launch_seg_labels16(const float* low, int B, int K, int h, int w, const CorrOut& out, const CorrLoss* loss, hipStream_t st);
// lseg_op_corr_argmax_loss: the streamed entry with everything it needs beside the outputs carved from ONE caller workspace
size_t corr_argmax_loss_ws_bytes(int B, int H, int W, int ragged, int want_nll, int temp_planes, int parts);
int corr_argmax_loss_op(const void* g, const void* T, const float* scale, const int64_t* target, int ignore_index, const int32_t* host_counts,
                        int B, int K, int H, int W, int C, int16_t* label, float* score, float* lse, float* tlogit, float* nll_plane, double* nll,
                        void* ws, size_t ws_bytes, hipStream_t st);
// episode.hip -- few-shot episode evaluation (Evaluator.classify_prediction + AverageMeter.update + the 2-class criterion): scores fp32
// [B,2,H,W] (up = 0) or low-resolution logits [B,2,H/2,W/2] read through the x2 bilinear (up = 1), target int64 / ignore uint8 (or NULL)
// [B,H,W] -> areas int64 [B,6], nll double [B,2], flags int64 [2], optional scatter into the meter's int64 [2,nclass] buffers
size_t episode_stats_ws_bytes(int B, int H, int W);
int launch_episode_stats(const float* scores, const int64_t* target, const uint8_t* ignore, int B, int H, int W, int up, int ignore_index,
                         const int64_t* class_id, int nclass, int64_t* inter_buf, int64_t* union_buf, int64_t* areas, double* nll,
                         int64_t* flags, void* ws, size_t ws_bytes, hipStream_t st);
// label_stats.hip -- seg_stats' counters and loss value without the score planes: from a label map (shared label set, ragged per-image
// lists with device offsets [B + 1], optionally mapped into [0, nclass) by class_map), and from the per-pixel state
// (label, best, sum of exp(v - best), target logit) that stats_fold_lowres builds panel by panel from low-resolution logits [B,rows,h,w].
// Every argument check comes before the device is touched.
int label_stats_plan(int bins, int* out2);                // host only: {route (0 = LDS histograms, 1 = global atomics), bins per workgroup}
int launch_label_stats(const int16_t* label, const int64_t* target, int B, int H, int W, int K, int ignore_index, const int32_t* offsets,
                       const int32_t* class_map, int nclass, int64_t* counts, int64_t* flags, int accumulate, hipStream_t st);
int launch_stats_fold_lowres(const float* low, int B, int rows, int row0, int h, int w, const int64_t* target, int16_t* label, float* best,
                             float* sum, float* tlogit, int first, hipStream_t st);
size_t stats_finish_ws_bytes(int B, int H, int W);
int launch_stats_finish(const int16_t* label, const float* best, const float* sum, const float* tlogit, const int64_t* target, int B, int H,
                        int W, int K, int ignore_index, int64_t* counts, double* nll, int64_t* flags, void* ws, size_t ws_bytes,
                        hipStream_t st);

// ---- split-precision ("strict") mode (strict.hip): 16-bit tensors as (hi, lo) fp16 planes `plane` elements apart --------------
int launch_convert_split(const void* in, int in_dtype, void* out, size_t n, size_t plane, hipStream_t st);
int launch_ln_split(const float* x, const float* gamma, const float* beta, void* out, size_t plane, int M, int D, float eps, hipStream_t st);
int launch_im2col_split(const float* x, void* A, size_t plane, int B, int H, int W, int P, hipStream_t st);
int launch_readout_cat_split(const float* x, void* A, size_t plane, int B, int ntok, int D, hipStream_t st);
int launch_upsample2x_nhwc_split(const void* in, size_t in_plane, void* out, size_t out_plane, int B, int H, int W, int C, hipStream_t st);
int launch_relu_split(const void* in, size_t in_plane, void* out, size_t out_plane, size_t n, hipStream_t st);
int launch_attention_strict(const void* q, const void* k, const void* vt, void* out, size_t qk_plane, size_t vt_plane, size_t out_plane,
                            int B, int H, int ntok, int npad, float scale, hipStream_t st);

size_t attention_backward_ws_bytes(int B, int H, int npad);
int launch_attention_backward_qkv(const void* q, const void* k, const void* vt, const void* o, const void* d_o, const float* lse2, void* dqkv,
                                  void* ws, int B, int H, int ntok, int npad, int dtype, float scale, hipStream_t stream);

// dW [rows_out, cols_out] (+)= dY[:, :rows_out]^T X[:, :cols_out], contraction over the M rows of dY [M, ldy] / X [M, ldx] (16-bit), through the
// K-major operand path of the GEMM (no transposed copies); `ws` = fp32 scratch for the split-K slabs (ws_floats >= rows_out * cols_out).
// Returns LSEG_ERR_UNSUPPORTED (and launches nothing) when cols_out % 128 != 0: callers keep the transposing path for those.
bool wgrad_kmajor_ok(int rows_out, int cols_out, size_t ws_floats);
int launch_wgrad_kmajor(const void* dy, int ldy, const void* x, int ldx, int M, int rows_out, int cols_out, float* dw, int accumulate,
                        float* ws, size_t ws_floats, int ab_dtype, hipStream_t st);

// 3x3 conv weight gradient in the padded-NHWC layout through the same path: slabs [ns][Cout][9 * Cin] (tap-major) in `ws`; *ns_out = slab count
// (the caller sums / re-layouts them: launch_conv_wgrad_unpack / launch_sum_partials).  Needs Cin % 128 == 0.
int launch_conv_wgrad_kmajor(const void* dy_pad, const void* x_pad, int relu_x, int B, int H, int W, int Cin, int Cout, float* ws, size_t ws_floats,
                             int ab_dtype, int* ns_out, hipStream_t st);

// ---- engine-level training step (train.hip) --------------------------------------------------------------------------------
int launch_attention_lse(const void* q, const void* k, const void* vt, void* out, float* lse2, int B, int H, int ntok, int npad, int dtype,
                         int causal, float scale, hipStream_t stream);
int launch_attention_ex(const void* q, const void* k, const void* vt, void* out, float* lse2, int B, int H, int ntok, int npad, int dtype,
                        int causal, float scale, int prescaled, hipStream_t stream);
// What launch_attention_ex launches on a device of `cus` compute units (host only): nw = waves per workgroup (2 | 4), nqb = query blocks of
// 32 nw rows per head, grid = workgroups, last_tiles = 64-key tiles the last query block walks, xcd_map = the head -> XCD map applies
// (B * H % 8 == 0), lds = dynamic LDS bytes.  Refuses B, H, ntok, cus < 1 and prescaled with causal.
struct AttnPlan { int nw, nqb, grid, last_tiles, xcd_map, lds; };
int plan_attention(int B, int H, int ntok, int causal, int prescaled, int cus, AttnPlan& p);
int launch_bn_stats(const void* x, float* stats, int B, int H, int W, int C, int dtype, hipStream_t st, int pre_zeroed = 0,
                    float* det_ws = nullptr, size_t det_cap = 0);
int launch_bn_apply(const void* x, void* y, const float* stats, const float* gamma, const float* beta, const void* res1, const void* res2,
                    int B, int H, int W, int C, float eps, double count, int dtype, hipStream_t st,
                    void* y_relu = nullptr);      // y_relu: ReLU(y), same geometry (y may then be NULL)
int launch_bn_bwd_stats(const void* dy, const void* x, const float* stats, float* bstats, int B, int H, int W, int C, float eps,
                        double count, int dtype, hipStream_t st, float* det_ws = nullptr, size_t det_cap = 0);
int launch_bn_bwd_apply(const void* dy, const void* x, const float* stats, const float* bstats, const float* gamma, void* dx,
                        int B, int H, int W, int C, float eps, double count, int dtype, hipStream_t st);
// corr.hip: dedicated pixel x text correlation on the commuted schedule (label planes + cell dot products of g from one pass)
bool corr_planes_supported(int K, int C);
int launch_corr_planes(const void* g16pad, const void* T16, float* R, float* gram, int B, int K, int H, int W, int C, hipStream_t st);
int launch_bn_running_update(const float* stats, float* rmean, float* rvar, int C, double count, float momentum, hipStream_t st);
int launch_gelu_forward(const void* pre, void* out, size_t n, int dtype, hipStream_t st);
int launch_unpad_rows(const void* in, void* out, int B, int H, int W, int C, hipStream_t st);
int launch_dilate2(const void* dy, void* dyd, int B, int Ho, int Wo, int H, int W, int C, hipStream_t st);
int launch_unpixshuf(const void* dl, void* dg, int B, int gh, int gw, int s, int C, hipStream_t st);
int launch_readout_cat_bwd(const void* dcat, float* gx, int B, int ntok, int D, int dtype, hipStream_t st);
int launch_embed_bwd(const float* gx, void* dtok, float* dpos, int B, int ntok, int D, int dtype, hipStream_t st);
int launch_pos_resize_bwd(const float* dpos, float* dposemb, float* dcls, int g_old, int gh, int gw, int D, hipStream_t st);
int launch_conv_wgrad_unpack(const float* dw, float* dst, int Co, int Ci, int Cip, int accumulate, hipStream_t st, int nsplit = 1, size_t split_stride = 0);
int launch_sum_partials(const float* part, float* dst, int nsplit, size_t n, size_t stride, int accumulate, hipStream_t st);
int launch_convT_wgrad_unpack(const float* dw, float* dst, int C, int Cp, int s, int accumulate, hipStream_t st);
int launch_fold_rows(const float* src, float* dst, int R, int C, int ld, int accumulate, hipStream_t st);
int launch_sgd(float* w, const float* g, float* m, void* w16, size_t n, float lr, float mu, float wd, int first, int dtype, hipStream_t st);
// table-driven launches of the optimizer step (tables live in device memory, sorted by blk0)
struct SgdSeg {
    float* w; const float* g; float* m;      // fp32 master, gradient, momentum
    uint16_t* w16; float* w32;               // the engine's same-layout copies of the parameter (either may be NULL)
    unsigned long long n;
    unsigned blk0;                           // first block of this parameter (4096 elements per block)
    int scratch;                             // learning-rate group: 0 = pretrained.*, 1 = scratch.*  (lsegmentation_module.py:119-127)
    int vec;                                 // every pointer 16-byte aligned (w16: 8) -> float4 path
};
struct AdamSeg {                              // SgdSeg with the two moment buffers of torch.optim.Adam (exp_avg, exp_avg_sq)
    float* w; const float* g; float* m; float* v;
    uint16_t* w16; float* w32;
    unsigned long long n;
    unsigned blk0;
    int scratch;
    int vec;
};
int launch_adam_multi(const AdamSeg* dev_segs, int nseg, unsigned blocks, float ss_pre, float ss_scr, float b1, float omb1, float b2, float omb2,
                      float bc2s, float eps, float wd, int dtype, hipStream_t st);
struct ZeroJob { float* p; unsigned n; };      // one block per job
int launch_zero_multi(const ZeroJob* dev_jobs, int njobs, hipStream_t st);
struct TransposeJob { const uint16_t* src; uint16_t* dst; int R, C; unsigned blk0; int tiles_r; };   // dst [C, R] = src [R, C]^T, R and C multiples of 8
int launch_sgd_multi(const SgdSeg* dev_segs, int nseg, unsigned blocks, float lr_pre, float lr_scr, float mu, float wd, int first, int dtype,
                     hipStream_t st);
int launch_transpose16_multi(const TransposeJob* dev_jobs, int njobs, unsigned blocks, hipStream_t st);

// ---- multi-scale / flip evaluator data movement (evaluator.hip) ---------------------------------------------------------------
int launch_eval_make_crops(const float* img, float* crops, int C, int height, int width, int crop, int stride, int h_grids, int w_grids,
                           int flip, const float* pad3, hipStream_t st);
int launch_eval_accumulate(const float* outs, float* outputs, int K, int height, int width, int ph, int pw, int crop, int stride, int h_grids,
                           int w_grids, int flip, hipStream_t st);
int launch_eval_accumulate_lowres(const float* low, float* outputs, int K, int height, int width, int crop, int stride, int h_grids, int w_grids,
                                  int flip, hipStream_t st);
int launch_eval_accumulate_window(const float* outs, float* sum, int K, int height, int width, int crop, int stride, int w_grids, int flip,
                                  int first, int nbox, int lowres, hipStream_t st);
int launch_eval_finalize(const float* sum, float* map, int K, int height, int width, int crop, int stride, int h_grids, int w_grids,
                         hipStream_t st);
int launch_eval_resize(const float* src, float* dst, int P, int Hi, int Wi, int Ho, int Wo, int accumulate, hipStream_t st);
// label panels of the multi-scale evaluator: scores [rows, H, W] (labels row0 ..) folded into the per-pixel (best, label, runner-up, label2,
// exp-sum) state; label2 / score2 / sum optional
int launch_eval_merge_labels(const float* scores, int rows, int row0, int H, int W, int16_t* label, float* score, int16_t* label2, float* score2,
                             float* sum, int first, int last, hipStream_t st);

// ---- resnet.hip: the torchvision ResNet-101 image tower (lseg_config.flags bit 5) ----
// stem: conv1 7x7/2 pad 3 (3 -> 64) + folded BN + ReLU, fp32 NCHW [B,3,H,W] -> padded NHWC 16-bit [B, Ho+2, Wo+2, 64]; w: fp32 [147][64]
// (BN-folded, k = (ci*7 + ky)*7 + kx), bias fp32 [64]
// relu 0: the raw conv output (train mode: bn1 on batch statistics follows)
int launch_rn_stem(const float* x, const float* w, const float* bias, void* out, int B, int H, int W, int dtype, hipStream_t st, int relu = 1);
// train-mode BatchNorm of the tower on a padded NHWC map [B, H+2, W+2, C] (interior written, border untouched): y = [relu](bn(x) + r) with
// bn from the batch sums `stats` [2C] over `count` pixels (biased variance); r = 0 (res NULL), res (rstats NULL) or bn_r(res) with sums,
// gamma and beta of its own.  y may alias x, res may alias y.
int launch_bn_apply_res(const void* x, void* y, const float* stats, const float* gamma, const float* beta, const void* res, const float* rstats,
                        const float* rgamma, const float* rbeta, int B, int H, int W, int C, float eps, double count, int relu, int dtype,
                        hipStream_t st);
// max-pool 3x3/2 pad 1 on a padded NHWC 16-bit map of NON-NEGATIVE values [B, H+2, W+2, C] -> padded [B, Ho+2, Wo+2, C]
int launch_rn_maxpool(const void* in, void* out, int B, int H, int W, int C, int dtype, hipStream_t st);
// BN-folding packers: 1x1 conv weight [Co, Ci] (+ BN) -> [Co, Ci] 16-bit + fp32 bias; stem 7x7 [64, 3, 7, 7] (+ BN) -> fp32 [147][64] + bias
int launch_pack_conv1x1(const float* w, const float* bn_w, const float* bn_b, const float* bn_m, const float* bn_v, float bn_eps,
                        void* wp, float* bias_out, int Co, int Ci, int dtype, hipStream_t st);
int launch_pack_rn_stem(const float* w, const float* bn_w, const float* bn_b, const float* bn_m, const float* bn_v, float bn_eps,
                        float* wp, float* bias_out, hipStream_t st);

// ---- input_u8.hip: decoded images in -- uint8 [B, H, W, 3] (HWC, RGB, dense), ToTensor + Normalize(mean, std) fused into the first stage:
// v -> (float(v) / 255 - mean[c]) / std[c] in fp32, torch's order and rounding.  Each launch writes what its fp32 counterpart
// (launch_im2col_patch, launch_rn_stem, launch_eval_resize + launch_eval_make_crops) writes for the torch-normalised tensor, bit for bit
struct NormU8 { float mean[3], std[3]; };
int norm_u8_check(const char* what, const float* mean, const float* std, NormU8* out);      // NULL, non-finite, std == 0: LSEG_ERR_INVALID
// the argument contract of the two launches below (alignment, geometry, dtype), without a device.  The launches themselves do not check:
// their callers do, once -- the op-level C entries before they look for a device, the engine's first stage on the caller's image pointer
int im2col_patch_u8_check(const void* x, const void* A, int B, int H, int W, int P, int dtype);
int rn_stem_u8_check(const void* x, const void* w, const void* bias, const void* out, int B, int H, int W, int dtype);
int launch_im2col_patch_u8(const uint8_t* x, void* A, int B, int H, int W, int P, int dtype, const NormU8& n, hipStream_t st);
int launch_rn_stem_u8(const uint8_t* x, const float* w, const float* bias, void* out, int B, int H, int W, int dtype, const NormU8& n,
                      hipStream_t st, int relu = 1);
// img uint8 [Hi, Wi, 3] -> crops fp32 [(1 + flip) * h_grids * w_grids, 3, crop, crop] of the image resized to (height, width)
int launch_eval_make_crops_u8(const uint8_t* img, float* crops, int Hi, int Wi, int height, int width, int crop, int stride, int h_grids,
                              int w_grids, int flip, const float* pad3, const NormU8& n, hipStream_t st);

}  // namespace lseg
