// engine.h -- the whole-forward plan of LSeg on one MI355X (owned buffers, packed weights).
#pragma once
#include <cmath>
#include <map>
#include <string>
#include <vector>

#include "ops.h"
#include "forward_route.h"
#include "train_head.h"
#include "../../include/lseg_hip.h"

namespace lseg {

struct BoundParam {
    const void* ptr = nullptr;
    int dtype = 0;
    std::vector<int64_t> shape;
    size_t numel() const { size_t n = 1; for (auto s : shape) n *= (size_t)s; return n; }
};

// w: packed [n, k] MFMA operand; b: fp32 bias.  Train mode adds wt = w transposed [k, n] (dgrad GEMM operand) for Linears and
// wd = the flipped / channel-swapped 3x3 weights (dgrad as a forward conv) for convs.
struct Lin { uint16_t* w = nullptr; float* b = nullptr; int n = 0, k = 0; uint16_t* wt = nullptr; uint16_t* wd = nullptr; };

// ---- GemmArgs builders: the one description of each GEMM shape the schedules (engine.hip, train.hip) launch.  A builder sets what its
// shape needs and nothing else; whatever is particular to one call site follows the call as an explicit line.
inline GemmArgs gemm_operands(const void* A, const Lin& w, int M) {       // A [M, w.k] against w [w.n, w.k], + w.b
    GemmArgs g;
    gemm_args_init(g);
    g.A = (const uint16_t*)A; g.W = w.w; g.M = M; g.N = w.n; g.K = w.k; g.lda = w.k; g.ldw = w.k; g.bias = w.b;
    return g;
}
// C [M, w.n] = A . w^T + w.b: nn.Linear, a 1x1 conv on pixel rows
inline GemmArgs lin_args(const void* A, const Lin& w, int M, void* C, int out_dtype) {
    GemmArgs g = gemm_operands(A, w, M);
    g.C = C; g.out_dtype = out_dtype; g.ldc = w.n; g.map_mode = MAP_LINEAR;
    return g;
}
inline void add_residual(GemmArgs& g, const void* res, int res_dtype) { g.res_mode = RES_DEST; g.res = res; g.res_dtype = res_dtype; }
inline void to_padded(GemmArgs& g, int ho, int wo) { g.map_mode = MAP_PADDED; g.ho = ho; g.wo = wo; }     // rows = pixels of a padded NHWC map
// the fused q/k/v Linear: q, k -> [b, head, t, 64], v -> [b, head, 64, t]
inline GemmArgs qkv_args(const void* A, const Lin& w, int M, void* q, void* k, void* vt, int ntok, int npad, int heads, int out_dtype) {
    GemmArgs g = gemm_operands(A, w, M);
    g.out_dtype = out_dtype; g.map_mode = MAP_QKV;
    g.C = q; g.Ck = k; g.Cv = vt; g.qkv_dim = w.k; g.qkv_ntok = ntok; g.qkv_npad = npad; g.qkv_heads = heads;
    return g;
}
// ConvTranspose2d(k = s = stride) on the (ho, wo) grid as a GEMM with a pixel-shuffle scatter into the padded (ho*s, wo*s) map
inline GemmArgs pixshuf_args(const void* A, const Lin& w, int M, void* C, int ch, int s, int ho, int wo, int out_dtype) {
    GemmArgs g = gemm_operands(A, w, M);
    g.bias_mod = ch; g.C = C; g.out_dtype = out_dtype; g.ldc = ch;
    g.map_mode = MAP_PIXSHUF; g.ho = ho; g.wo = wo; g.ps_s = s; g.ps_C = ch;
    return g;
}
// rows m = (image, r) with r < p_div land in row image * p_mul + r + p_off of C, plus row r + p_off of a [*, ldr] table shared by the images:
// the patch embedding writes token rows 1.. of every image and adds the position embedding (p_div = patches, p_mul = tokens, p_off = 1)
inline void to_periodic_rows(GemmArgs& g, const void* table, int table_dtype, int ldr, int p_div, int p_mul, int p_off) {
    g.res_mode = RES_PERIODIC; g.res = table; g.res_dtype = table_dtype; g.ldr = ldr;
    g.map_mode = MAP_PERIODIC; g.p_div = p_div; g.p_mul = p_mul; g.p_off = p_off;
}
inline float logit_scale() { return expf(logf(1.0f / 0.07f)); }            // lseg_net.py:141

struct VitBlock { float *g1 = nullptr, *b1 = nullptr, *g2 = nullptr, *b2 = nullptr; Lin qkv, proj, fc1, fc2; };
struct TextBlock { float *g1 = nullptr, *b1 = nullptr, *g2 = nullptr, *b2 = nullptr; Lin qkv, out, fc, proj; };
// c1/c2: BN-folded convs (eval).  Train mode: r1/r2 = the raw convs, BN affine parameters in fp32, per-unit saved maps.
struct Rcu {
    Lin c1, c2;
    Lin r1, r2;
    float *g1 = nullptr, *be1 = nullptr, *g2 = nullptr, *be2 = nullptr;
    std::string key;                                                       // "scratch.refinenetR.resConfUnitU."
    uint16_t *cv1 = nullptr, *n1 = nullptr, *cv2 = nullptr;                // conv1 out, ReLU(bn1 out), conv2 out (padded NHWC)
    const uint16_t* in_relu = nullptr;                                     // ReLU(unit input) of the last train-mode forward (NULL: clamp in the K-loop)
    float *st1 = nullptr, *st2 = nullptr;                                  // [2C] batch sums of bn1 / bn2
};
struct Refine { Rcu u1, u2; Lin out_conv; bool has_u1 = false; };

struct ProfileSlot { double total_ms = 0; int64_t launches = 0; double flops = 0; };

// saved tensors of one ViT block for the backward (train mode): everything 16-bit is an MFMA operand of a wgrad / dgrad GEMM
struct BlockSave {
    float *xin = nullptr, *xmid = nullptr, *lse = nullptr;
    uint16_t *ln1 = nullptr, *q = nullptr, *k = nullptr, *vt = nullptr, *att = nullptr, *ln2 = nullptr, *pre = nullptr, *mlp = nullptr;
};
// buffers of one reassemble level (Engine::reassemble): train mode keeps one set per level, inference shares one (ropre NULL, no dro)
struct LevelSave { uint16_t *cat = nullptr, *ropre = nullptr, *ro = nullptr, *r1 = nullptr, *tmp = nullptr, *dro = nullptr; };

typedef void (*lseg_reduce_fn)(void* user, void* dev_ptr, int64_t n_floats, void* stream);   // in-place sum over ranks
typedef void (*lseg_bucket_fn)(void* user, int bucket, void* stream);                        // the bucket's gradients are enqueued

class Engine {
public:
    Engine(const lseg_config& c, int device);
    ~Engine();
    int init();                               // allocate workspace
    int bind(const char* key, const void* p, int dtype, const int64_t* shape, int ndim);
    int finalize(hipStream_t st);
    int set_tokens(const int64_t* host_tok, int K, int ctx);
    int set_text_features(const void* dev_feat_f16, int K, hipStream_t st);
    bool text_external_ = false;   // the text features were handed in (lseg_set_text_features): forward never runs the text tower
    int encode_text(hipStream_t st);
    struct LabelConf { int16_t* label2 = nullptr; float* score2 = nullptr; float* lse = nullptr; };
    struct HeldOut { void* feat; float* scale; };
    // What one forward is asked for: every member optional, filled by name.  forward_route (forward_route.h) maps the request to the
    // schedule that runs, check_request refuses what none serves.
    struct ForwardOut {
        float* logits = nullptr;          // fp32 [B,Kout,img_h,img_w] (lseg_forward)
        uint8_t* argmax = nullptr;        // uint8 [B,img_h,img_w] masks, K <= 256 (lseg_forward)
        // label / score (int16 / fp32 [B,img_h,img_w], lseg_forward_labels): masks for any K <= 32767; with no other output wanted the
        // labels are streamed (corr_argmax.hip): no (2h, 2w) or full-resolution label plane is written.  score needs label
        int16_t* label = nullptr; float* score = nullptr;
        float* low = nullptr;             // fp32 [B,Kout,img_h/2,img_w/2] (lseg_forward_lowres): the logits output_conv would upsample
        LabelConf conf;                   // lseg_forward_labels_conf; needs label: the runner-up and the log-sum-exp beside the arg-max
        // lseg_forward_features: the forward stops behind the scale plane and copies what the correlation reads -- g16pad_ and nscale_ --
        // into the caller's buffers; no text is read, the gram is pixel_gram's whatever K is set
        const HeldOut* held = nullptr;
        // lseg_forward_labels_loss; needs label, excludes conf's runner-up and every other output: the cross-entropy beside the arg-max --
        // conf.lse is its lse output, the rest is ops.h' CorrLoss; streamed where the labels stream, seg_labels16 on the planes elsewhere
        const CorrLoss* loss = nullptr;
    };
    int forward(const float* x, int B, const ForwardOut& out, hipStream_t st);
    // lseg_set_input_u8: the image pointer of every forward entry (inference and train mode) is uint8 [B, img_h, img_w, 3] and the first
    // stage normalises it (input_u8.hip); off = fp32 NCHW, the default.  The pointer keeps its `const float*` type through the schedule:
    // only the first stage (patch_embed, the ResNet stem) dereferences it, and that is where the format is looked at
    int set_input_u8(bool on, const NormU8& norm);        // norm: validated by the caller (norm_u8_check), read only when on
    // lseg_forward_labels_loss: the labels forward with the loss, then (dev_counts given) lseg_op_label_stats on the label map it wrote.
    // The planes nobody asked for (lse, tlogit), the reduction's partials and label_stats' flag words live in loss_ws_, made on first use
    int forward_labels_loss(const float* x, int B, const int64_t* target, int ignore_index, int16_t* label_out, float* score_out, float* lse_out,
                            float* nll_plane_out, double* nll, int64_t* counts, hipStream_t st);
    // label panels over held features (lseg_forward_features / lseg_score_features): the bytes of the two held buffers for B images, and
    // the low-resolution logits of text rows [row0, row0 + rows) from them -- correlate_planes + upsample2x_planes_scaled, the K > 157
    // route of lseg_forward_lowres plane for plane
    void features_bytes(int B, size_t* feat_bytes, size_t* scale_bytes) const;
    int score_features(const void* feat, const float* scale, int B, int row0, int rows, float* low_out, hipStream_t st);
    int get_text_features(void* out_f16, hipStream_t st);
    int forward_stats(const int64_t* target, int ignore_index, int64_t* counts, double* nll, hipStream_t st);
    // few-shot episode statistics of the last forward's 2 label planes (episode.hip), inference or train-mode forward alike
    int episode_stats(const int64_t* target, const uint8_t* ignore, int ignore_index, const int64_t* class_id, int nclass, int64_t* inter_buf,
                      int64_t* union_buf, int64_t* areas, double* nll, int64_t* flags, hipStream_t st);
    int get_intermediate(const char* name, float* out, size_t cap, size_t* n, hipStream_t st);
    int get_profile(const char* family, double* ms, int64_t* launches, double* flops);
    // 16-bit range check of the image tower (fp16 operands saturate at 65504): scans every 16-bit activation buffer of the plan
    int check_range(unsigned long long* host_out4, hipStream_t st);
    // Always-on overflow sentinel of the inference forward: norm_scale_plane_kernel raises a device flag when the head feature map carries an
    // inf / NaN (anything non-finite in the 16-bit tower ends up there); the flag is copied to pinned host memory behind every forward and
    // read WITHOUT synchronising: 1 as soon as a COMPLETED forward was flagged (sticky until reset), 0 otherwise.
    int overflow_seen(bool reset);
    // ---- training step (train.hip; modules/lsegmentation_module.py:66-81) ----
    int set_train(bool on);
    int bind_grad(const char* key, float* dev_ptr);
    int grad_ptr(const char* key, float** out, size_t* n);
    int backward(const float* dlogits, const int64_t* target, int ignore_index, int accumulate, double* dev_loss2, hipStream_t st,
                 const float* dev_grad_scale = nullptr);
    int train_loss(const int64_t* target, int ignore_index, double* dev_loss2, int64_t* dev_counts2, hipStream_t st);
    int sgd_momentum(const char* key, float** out, size_t* n);
    int sgd_mark_initialized(bool on) { sgd_first_ = !on; return 0; }
    int sgd_step(float lr_pretrained, float lr_scratch, float momentum, float weight_decay, hipStream_t st);
    int adam_step(double lr_pretrained, double lr_scratch, double beta1, double beta2, double eps, double weight_decay, long long step, hipStream_t st);
    int adam_state(const char* key, int which, float** out, size_t* n);
    int set_frozen_encoder(bool on);
    int n_buckets() const { return resnet_ ? 1 : cfg.depth + 1; }
    int bucket_of(const std::string& key) const;
    lseg_reduce_fn bn_sync_fn = nullptr; void* bn_sync_user = nullptr; int bn_world = 1;
    lseg_bucket_fn bucket_fn = nullptr; void* bucket_user = nullptr;
    bool train_mode = false;

    lseg_config cfg;
    int device;
    bool text_cache = false, text_valid = false, debug = false;
    int group_k = 0;              // > 0: per-image label sets of this size (LSegNetZS), see lseg_set_text_grouping
    // ragged per-image label sets (lseg_set_text_groups): image b owns groups_[b] consecutive text rows; empty = none
    int set_text_groups(const int32_t* host_counts, int B);
    void clear_text_groups() { groups_.clear(); }
    bool ragged() const { return !groups_.empty(); }
    std::string err;

private:
    void* dalloc(size_t bytes, bool zero = true);
    int need(const std::string& key, BoundParam& out, std::initializer_list<int64_t> shape);
    int pack_linear(const std::string& wkey, const std::string& bkey, int n, int k, int dt, Lin& out, hipStream_t st, bool image = false);
    int pack_f32(const std::string& key, size_t n, float*& out, hipStream_t st);
    int pack_conv3(const std::string& wkey, const std::string& bn_prefix, const std::string& bias_key, int co, int ci,
                   int cop, int cip, Lin& out, hipStream_t st);
    // ksize 1: a 1x1 conv (w.k = Cin) on the padded map; relu_after_res: relu(conv + res) (ResNet bottleneck) instead of relu(conv) + res
    int conv3x3(const void* in, const Lin& w, const void* res, const void* res2, void* out, int B, int H, int W,
                int stride, int relu_in, int relu_out, hipStream_t st, void* out_relu = nullptr, bool* relu_written = nullptr,
                int ksize = 3, int relu_after_res = 0);
    int pack_conv1(const std::string& wkey, const std::string& bn_prefix, int co, int ci, Lin& out, hipStream_t st);
    int pack_resnet(hipStream_t st);
    int resnet_forward(const float* x, int B, hipStream_t st);
    int refine(int r, int B, hipStream_t st, bool stop_before_upsample = false);
    // stages the inference and the train-mode forward share; the destination buffers are the caller's
    int patch_embed(const float* x_in, float* x, int B, hipStream_t st);                       // im2col, patch GEMM + pos-embed, cls rows
    int reassemble(int l, const float* x, const LevelSave& v, int B, hipStream_t st);          // readout .. layerN_rn -> rn_[l]
    int out_conv(int l, int B, hipStream_t st);                                                // up_[l] -> path_[l]
    int correlate_planes(const uint16_t* t, const uint16_t* pixels, int K, int npix, int p_div, float* planes, int round_mid, hipStream_t st);
    int text_fork(hipStream_t st);
    int text_join(hipStream_t st);
    int check_grouping(int B);
    int check_ragged_train();                        // ... and of a train-mode forward / lseg_set_train while they are set
    int check_held(const char* what);                // the refusals of lseg_forward_features / lseg_score_features: where corr_low does not hold
    // ---- Engine::forward: the request as plain values and its refusals before any launch (forward_request.hip), the stages of its tails
    RouteIn route_in(const ForwardOut& out) const;
    int check_request(const float* x, int B, const ForwardOut& out, const RouteIn& r);
    // ... and of the training step: forward_train, train_loss and backward refuse here, before any state changes
    TrainHeadIn train_head_in(bool logits) const;
    int check_train_forward(int B, const TrainHead& plan);
    int check_train_loss(const int64_t* target);
    int check_backward(const float* dlogits, const int64_t* target, const float* dev_grad_scale);
    int image_tower(const float* x_in, int B, hipStream_t st);                 // ViT blocks + reassemble, or ResNet-101 + layerN_rn -> rn_[0..3]
    int scale_plane(int B, bool corr_fused, hipStream_t st);                   // g16pad_, gram_ (corr_fused: rpl_ too), nscale_, overflow sentinel
    int label_planes(int B, FwdPlanes src, hipStream_t st);                    // rpl_ = the label planes at quarter resolution; low_ pending
    int feature_planes(FwdTail tail, int B, hipStream_t st);                   // a16_ at (2h, 2w) by one of the three feature paths, then low_
    int head_blocks(int B, int kout, const float** low, hipStream_t st);       // arch_option 1 / 2 on low_; *low = the planes the outputs read
    int planes_outputs(const ForwardOut& out, const float* low, int B, int kout, hipStream_t st);
    std::vector<int32_t> groups_;
    char* loss_ws_ = nullptr;                        // forward_labels_loss: {lse, tlogit} fp32 [max_batch,img_h,img_w], partials, flags
    int* d_goff_ = nullptr;                          // [max_batch + 1] prefix sum of groups_, written by the ragged launch
    int flush_events();
    int materialize_low(hipStream_t st);
    bool low_pending_ = false; int low_planes_ = 0, low_k_ = 0;      // low_ = scaled x2 upsample of rpl_ not yet written (one-pass x4 upsample ran)
    // train.hip
    int train_alloc();
    int finalize_train(hipStream_t st);
    int forward_train(const float* x, int B, float* logits, hipStream_t st);
    // the label head of the training step, each stage a switch over train_head_.mode (train_head.h)
    int train_correlate(const TrainHead& plan, int B, hipStream_t st);                          // a16_ -> low_, the dgrad operand where the plan has one
    int ensure_loss(const int64_t* target, int ignore_index, hipStream_t st, bool force = false);      // nll_, counts_, lse_px_ of this forward and target, once
    int publish_loss(double* dev_loss2, int64_t* dev_counts2, hipStream_t st);
    int loss_rows(const TrainHead& plan, const float* dlogits, const int64_t* target, int ignore_index, double* dev_loss2,
                  const float* dev_grad_scale, hipStream_t st);                 // drows_ = d(low) rows [B*hw1, Kp], or the head blocks' planes in low2_
    int head_blocks_backward(const TrainHead& plan, int acc, hipStream_t st);                   // gradient planes in low2_ -> drows_, {dW, db}
    int train_correlate_backward(const TrainHead& plan, hipStream_t st);                        // drows_ -> df_
    int rcu_train(const uint16_t* in, const uint16_t* in_relu, Rcu& U, const uint16_t* res2, uint16_t* out, uint16_t* out_relu, int B, int H, int W,
                  hipStream_t st);
    int rcu_backward(const uint16_t* dout, const uint16_t* in, Rcu& U, uint16_t* din, int lev, int B, int H, int W, int acc, hipStream_t st);
    int linear_gelu_saved(GemmArgs& g, uint16_t* pre, uint16_t* out, hipStream_t st);
    int lin_bwd(const uint16_t* dy, int M, int N, int K, const uint16_t* x, const uint16_t* wt, uint16_t* dx, float* dw, float* db,
                int acc, hipStream_t st, int dw_rows = -1, const uint16_t* dgelu_pre = nullptr);
    int conv_bwd(const uint16_t* dy_pad, const uint16_t* x_pad, int relu_x, const Lin& w, uint16_t* dx_pad, float* dw_dst, int B, int H,
                 int W, int Cin, int Cout, int Ci_real, int Co_real, int acc, hipStream_t st);
    int pick_split(int M, int N, int nk, GemmArgs& g);
    int block_backward(int i, int B, int acc, hipStream_t st);
    int readout_backward(int l, int B, int acc, hipStream_t st);
    int reassemble_backward(int l, int B, int acc, hipStream_t st);
    int refine_backward(int r, int B, int acc, hipStream_t st);
    float* grad(const std::string& key, size_t n);
    void bucket_done(int b, hipStream_t st) { if (bucket_fn) bucket_fn(bucket_user, b, (void*)st); }
    int bn_sync(float* p, int n, hipStream_t st) { if (bn_sync_fn && bn_world > 1) bn_sync_fn(bn_sync_user, p, n, (void*)st); return 0; }

    std::map<std::string, BoundParam> bound_;
    std::vector<void*> allocs_;
    std::vector<std::pair<const uint16_t*, size_t>> act16_;     // every 16-bit image-tower activation buffer (check_range)
    unsigned long long* range_out_ = nullptr;
    unsigned* ovf_dev_ = nullptr; unsigned* ovf_host_ = nullptr; hipEvent_t ev_ovf_ = nullptr; bool ovf_pending_ = false, ovf_sticky_ = false;
    bool finalized_ = false, inited_ = false;
    int last_B_ = 0, last_kout_ = 0;
    const float* last_low_ = nullptr;
    bool labels_only_ = false;                                        // the last forward streamed its labels: low_ holds no planes of it

    // derived geometry
    int gh_, gw_, np_, ntok_, npad_, img_dt_;
    int rows_alloc_ = 0;                        // allocated rows of x_ / ln_ / att_ / mlp_: max_batch * ntok rounded up to 256 (gemm_asm.hip)
    bool in_u8_ = false; NormU8 in_norm_ = {};  // input format (set_input_u8)
    int image_stem(const float* x, const float* w, const float* bias, int B, int relu, hipStream_t st);      // ResNet stem in the input's format
    bool strict_ = false;                       // split-precision mode (lseg_config.image_dtype == LSEG_F16_SPLIT)
    std::map<const void*, size_t> plane_;       // 16-bit buffer -> element offset of its lo plane
    size_t pl(const void* p) const { auto it = plane_.find(p); return it == plane_.end() ? 0 : it->second; }
    int igemm(GemmArgs& g, hipStream_t st);     // image-tower GEMM: fills the split-precision planes when strict_
    int split_residual(GemmArgs& g, int M, int N, int K);
    float* ws_split_ = nullptr; size_t ws_split_rows_ = 0, ws_split_n_ = 0;      // ws_split_n_: floats in ws_split_
    float* pack_tmp_ = nullptr; size_t pack_tmp_n_ = 0;
    uint16_t* relu_tmp_ = nullptr;
    int pack_tmp(size_t n, hipStream_t st);
    int lh_[4], lw_[4];          // spatial size of reassembled level l (0..3)
    int cp_[4];                  // reassemble channels rounded up to 64 (ViT-B/32: 96 -> 128), extra channels are 0
    int tnpad_;

    // ---- packed parameters -------------------------------------------------------------------
    Lin patch_;
    float *cls_ = nullptr, *pos_raw_ = nullptr, *pos_ = nullptr;
    std::vector<VitBlock> blocks_;
    Lin readout_[4], r1x1_[4], rsmp_[4], layer_rn_[4];
    Refine refine_[4];           // index r-1
    Lin head1_;
    Lin headc_;                  // head1 o refinenet1.out_conv as ONE 1x1 conv (applied before the x2 upsample: engine.hip "commuted head")
    float *headc_w32_ = nullptr, *gpad_ = nullptr;
    uint16_t* g16pad_ = nullptr; float *rpl_ = nullptr, *gram_ = nullptr, *nscale_ = nullptr;     // commuted correlation (engine.hip)
    float *hb_w_ = nullptr, *hb_b_ = nullptr;
    float *tok_emb_ = nullptr, *tpos_ = nullptr, *tlnf_g_ = nullptr, *tlnf_b_ = nullptr;
    std::vector<TextBlock> tblocks_;
    Lin tproj_;

    // ---- torchvision ResNet-101 image tower (lseg_config.flags bit 5; resnet.hip, Engine::resnet_forward) ------------------------
    // c1 / c3 / ds: BN-folded 1x1 convs, c2: BN-folded 3x3 conv (stride on it: Bottleneck v1.5)
    // train mode (flags bit 6): r1 / r2 / r3 / rds = the UNFOLDED convs (bias = zeros_), bn[i] = {gamma, beta} in the caller's bound
    // tensors, st[i] = [2C] batch sums of bn1 / bn2 / bn3 / downsample.1, key = "pretrained.layerL.J."
    struct RnBlock {
        Lin c1, c2, c3, ds; int width = 0, stride = 1; bool has_ds = false;
        Lin r1, r2, r3, rds;
        const float *ga[4] = {}, *be[4] = {}; float* st[4] = {};
        std::string key;
    };
    bool resnet_ = false;
    bool rn_train_ = false;                                  // flags bit 6: lseg_set_train is accepted, the decoder above the tower trains
    float *rs_stem_wraw_ = nullptr, *rs_stem_st_ = nullptr, *ones_ = nullptr;      // stem conv1 unfolded [147][64], its batch sums [128]
    const float *rs_stem_ga_ = nullptr, *rs_stem_be_ = nullptr;
    // conv outputs whose batch sums are taken need a zero border of their own geometry: per-stage conv2 / conv3 / downsample outputs
    uint16_t *rs_t2l_[4] = {}, *rs_c3l_[4] = {}, *rs_dsl_[4] = {};
    int resnet_forward_train(const float* x, int B, hipStream_t st);
    int finalize_train_resnet(hipStream_t st);
    int rn_bn(const uint16_t* x, uint16_t* y, RnBlock& k, int i, const uint16_t* res, int res_bn, int relu, int B, int H, int W, int C, hipStream_t st);
    float *rs_stem_w_ = nullptr, *rs_stem_b_ = nullptr;      // stem conv1 + bn1 folded: fp32 [147][64], [64]
    std::vector<RnBlock> rs_blocks_[4];
    uint16_t *rs_stem_ = nullptr, *rs_pool_ = nullptr;     // stem output (H/2, zero border: the max-pool reads it), max-pool output (H/4)
    uint16_t *rs_t1_[4] = {}, *rs_t1in_[4] = {};             // conv1 outputs (zero border: conv2 reads them with 3x3 taps) at the stage's
                                                             // resolution / at the previous stage's (block 0 of layer2..4, whose conv2 has stride 2)
    uint16_t *rs_t2_ = nullptr, *rs_ds_ = nullptr;           // conv2 output, downsample output: read only at the centre (1x1 conv, residual)

    // ---- workspace -----------------------------------------------------------------------------
    float* x_ = nullptr;
    uint16_t *ln_ = nullptr, *q_ = nullptr, *k_ = nullptr, *vt_ = nullptr, *att_ = nullptr, *mlp_ = nullptr;
    uint16_t *patchA_ = nullptr, *catA_ = nullptr, *ro_ = nullptr, *r1_ = nullptr, *tmp_pad_ = nullptr;
    uint16_t* L_[4] = {};         // reassembled maps, padded NHWC
    uint16_t* rn_[4] = {};        // layerN_rn outputs, padded NHWC
    uint16_t *rnr_[4] = {}, *sumr_[4] = {};   // ReLU(rn_) / ReLU(sum_) written by the producing conv's epilogue (refine())
    bool rn_relu_ok_[4] = {};
    uint16_t *t1_[4] = {}, *sum_[4] = {}, *t2_[4] = {};   // refinenet temporaries per level
    uint16_t* up_[4] = {};        // upsampled (plain) per level
    uint16_t* path_[4] = {};      // path_r outputs: r=4..2 padded at next level's size, r=1 plain
    float* feat_ = nullptr;
    uint16_t* a16_ = nullptr;
    float *low_ = nullptr, *low2_ = nullptr, *low3_ = nullptr;
    float* acts_[4] = {};
    // text
    int K_ = 0;
    int tl_ = 0;                  // text positions actually computed (<= text_ctx), see set_tokens
    int64_t* d_tok_ = nullptr;
    int* d_eot_ = nullptr;
    uint16_t *tx_ = nullptr, *tln_ = nullptr, *tq_ = nullptr, *tk_ = nullptr, *tvt_ = nullptr, *tatt_ = nullptr,
             *tmlp_ = nullptr, *tpool_ = nullptr, *tfeat_ = nullptr, *tnorm_ = nullptr;

    // ---- train mode (allocated by set_train(true)) ------------------------------------------------------------------------
    bool train_alloc_ = false, train_fwd_valid_ = false;
    const int64_t* loss_target_ = nullptr; int loss_ignore_ = 0;      // train_loss() already ran seg_stats for this forward and this target
    int train_B_ = 0;
    TrainHead train_head_;        // how the label head of the last train-mode forward ran: the plan train_loss and backward follow
    // ragged per-image label sets of the last train-mode forward (train_head_.ragged()): host prefix sums [B + 1] (d_goff_ holds them
    // on the device) and the per-image transposed text panels [out_c, up64(k_b)] of the correlation backward, concatenated
    std::vector<int> train_rag_;
    uint16_t* tnT_rag_ = nullptr;
    std::vector<BlockSave> sv_;
    float* xlast_ = nullptr;               // output of the last block (= xin of a virtual block `depth`)
    LevelSave lv_[4];
    uint16_t *dmapA_[4] = {}, *dmapB_[4] = {}, *dmapC_[4] = {}, *dmapD_[4] = {};   // gradient maps per pyramid level (padded NHWC, zero border)
    uint16_t *dpath_[4] = {};              // d path_{l+1}: aliases the level-(l-1) map it is produced in
    uint16_t *dpath0_ = nullptr;           // d path_1 rows [B*4*h*w, F]
    // arch_option 1/2 head blocks in train mode (lseg_config.flags bit 4; head_train.hip): n applications of the shared block
    int hb_n_ = 0;                         // 0: no head blocks are trained
    std::vector<float*> hb_out_;           // saved block outputs x_1..x_n, fp32 planes [B,K,h,w] each
    int* hb_kstar_ = nullptr;              // bottleneck: first arg-max label of each block's input, [n][B*h*w]
    float* hb_ks_[2] = {};                 // bottleneck: per-pixel label sums of the gradient planes (ping-pong)
    float* hb_part_ = nullptr;             // {dW, db} partial rows of the n block backwards
    const float* train_out_ = nullptr;     // head output of the last train-mode forward (low_ without head blocks)
    uint16_t *drn_[4] = {}, *dL_[4] = {};
    uint16_t *rowsA_ = nullptr, *rowsB_ = nullptr;  // row-major 16-bit temporaries (GEMM operand views of gradient maps)
    uint16_t *ddil_ = nullptr, *dtmp_ = nullptr;    // stride-2 reassemble conv: dilated dY, d(1x1 output)
    uint16_t *tn16_ = nullptr;
    uint16_t *ws_a_ = nullptr, *ws_b_ = nullptr;    // transposed operands of the wgrad GEMMs
    size_t ws_a_n_ = 0, ws_b_n_ = 0;
    float* ws_part_ = nullptr; size_t ws_part_n_ = 0;   // split-K partial results of the weight-gradient GEMMs
    float* ws_dw_ = nullptr; size_t ws_dw_n_ = 0;   // wgrad output in the engine's packed layout before the re-layout into the parameter's
    float *ws_stats_ = nullptr, *zeros_ = nullptr, *ws_ln_ = nullptr;
    float* ws_det_ = nullptr; size_t ws_det_n_ = 0;     // cfg.flags bit 3: partial rows of the deterministic column reductions
    float *gx_ = nullptr, *dpos_ = nullptr, *lse_px_ = nullptr;     // lse_px_: per-pixel log-sum-exp of the up-sampled logits [B, 2h, 2w]
    char* attn_ws_ = nullptr;              // per-layer scratch of the attention backward (transposed / head-major operand copies)
    uint16_t *g16_ = nullptr, *dmlp_ = nullptr, *dln_ = nullptr, *datt_ = nullptr, *dqkv_ = nullptr, *dtok_ = nullptr;
    bool g16_valid_ = false;                             // g16_ currently equals the 16-bit rounding of gx_ (written by the LayerNorm backward)
    uint16_t *drows_ = nullptr, *da_ = nullptr, *df_ = nullptr, *tnT_ = nullptr;
    unsigned long long* counts_ = nullptr; double* nll_ = nullptr;
    struct GradSlot { float* ptr = nullptr; size_t n = 0; bool bound = false; };
    std::map<std::string, GradSlot> grads_;
    bool sgd_first_ = true;
    // the optimizer step as table-driven launches: one multi-tensor SGD (which also refreshes the same-layout copies finalize() keeps of a
    // parameter: `direct_`), one multi-matrix transpose for the W^T copies, then only the packs with a real re-layout
    struct DirectDst { uint16_t* w16 = nullptr; float* w32 = nullptr; bool conflict = false; };
    std::map<std::string, DirectDst> direct_;
    void note_direct(const std::string& key, uint16_t* w16, float* w32);
    bool sgd_owns(const std::string& key) const { return partial_pack_ && sgd_keys_.count(key) != 0; }
    std::map<std::string, int> sgd_keys_;   // parameters the SGD table updates (and whose direct copies it writes)
    bool partial_pack_ = false;            // finalize() running inside sgd_step: skip what the optimizer kernel already wrote and the frozen text tower
    bool eval_stale_ = false;              // eval-only packs (BN-folded convs, commuted head) are behind the masters: refreshed by the next eval forward
    SgdSeg* sgd_table_ = nullptr; int sgd_nseg_ = 0; unsigned sgd_blocks_ = 0; bool sgd_dirty_ = true;
    float* mom_flat_ = nullptr; size_t mom_flat_n_ = 0;
    TransposeJob* wt_table_ = nullptr; int wt_n_ = 0; unsigned wt_blocks_ = 0;
    int build_sgd_table();
    // optimizer_segments: the walk both optimizer tables share -- one entry per trainable parameter with a gradient buffer, in key order
    int optimizer_segments(std::vector<SgdSeg>& segs);
    std::map<std::string, std::pair<size_t, size_t>> opt_off_;   // key -> {float offset in a flat state allocation, elements}: filled by the walk
    int repack_after_step(hipStream_t st);
    static bool is_encoder_key(const std::string& key) { return key.compare(0, 17, "pretrained.model.") == 0; }
    // frozen encoder (lseg_set_frozen_encoder): pretrained.model.* is not trainable -- no gradient, no optimizer state, and the backward
    // stops at the four readouts; the train-mode forward then keeps ONE block's activations instead of `depth`
    bool frozen_ = false;
    // fused Adam (torch.optim.Adam): exp_avg / exp_avg_sq of every trainable parameter in one flat allocation, [all m | all v]
    AdamSeg* adam_table_ = nullptr; int adam_nseg_ = 0; unsigned adam_blocks_ = 0; bool adam_dirty_ = true;
    float* adam_flat_ = nullptr; size_t adam_flat_n_ = 0;      // adam_flat_n_: padded floats of ONE moment
    int build_adam_table();
    void optimizer_dirty() { sgd_dirty_ = true; adam_dirty_ = true; }
    // small buffers that are accumulated into with atomics, zeroed by ONE launch per pass once their list is known (recorded during the
    // first pass, which still uses one memset each): [0] the forward's BatchNorm batch sums, [1] the backward's bias gradients
    struct ZeroSet { std::vector<ZeroJob> host; ZeroJob* dev = nullptr; int n = 0; bool ready = false; };
    ZeroSet zero_fwd_, zero_bwd_;
    bool zero_note(ZeroSet& z, float* p, size_t n);       // true: the buffer was zeroed by this pass's launch_zero_multi
    int zero_begin(ZeroSet& z, hipStream_t st);
    int zero_end(ZeroSet& z);
    int bias_sum(const uint16_t* dy, float* db, int R, int C, int ld, int acc, hipStream_t st);

    // ---- side stream: the (small, latency-bound) text tower overlaps the image tower ----------------
    hipStream_t text_stream_ = nullptr;
    hipEvent_t ev_fork_ = nullptr, ev_join_ = nullptr, ev_text_done_ = nullptr;
    bool text_pending_ = false, text_forked_ = false;

    // ---- profiling: HIP-event pairs around kernel families on the caller's stream (lseg_set_profiling mask bit = family index) --------
public:
    enum ProfFamily { PF_FWD = 0, PF_FC1, PF_FC2, PF_PROJ, PF_QKV, PF_ATTN, PF_LN, PF_CORR, PF_N };
    unsigned prof_mask = 0;
    int reserve_events(int n);
    int events_per_forward() const;
private:
    struct ProfFam { std::vector<std::pair<hipEvent_t, hipEvent_t>> ev; ProfileSlot slot; };
    ProfFam pf_[PF_N];
    std::vector<hipEvent_t> ev_pool_, ev_free_;
    hipEvent_t get_event();
    hipEvent_t prof_begin(int fam, hipStream_t st);
    void prof_end(int fam, hipEvent_t e0, double flops, hipStream_t st);
};

}  // namespace lseg
