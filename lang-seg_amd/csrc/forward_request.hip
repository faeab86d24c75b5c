// forward_request.hip -- what Engine::forward may be asked for: the request as the plain values of forward_route.h, and every refusal that
// is decided before a launch, in one order, with its message.  (Two refusals stay in the forward, engine.hip: check_grouping behind
// the text join, and the uint8 masks with K > 256 behind the planes in memory.)  The same for the training step: the plan's inputs
// (train_head.h) and the refusals of forward_train, train_loss and backward.
#include "engine.h"

#include <algorithm>
#include <cstdlib>

namespace lseg {

#define TRY(expr) do { int _r = (expr); if (_r != 0) return _r; } while (0)

// the request of a forward and the engine's configuration as the values forward_route / forward_refusal decide on
RouteIn Engine::route_in(const ForwardOut& out) const {
    // A/B switches (tools, tests), read once per process: the correlation at (2h, 2w); the round-4 generic GEMM + pixel_gram pair; no one-pass x4
    static const bool corr_full = getenv("LSEG_CORR_FULLRES") != nullptr, corr_generic = getenv("LSEG_CORR_GENERIC") != nullptr,
                      no_4x = getenv("LSEG_NO_UPSAMPLE4X") != nullptr;
    RouteIn r;
    r.logits = out.logits; r.argmax = out.argmax; r.label = out.label; r.score = out.score; r.low = out.low;
    r.runner_up = out.conf.label2 || out.conf.score2; r.lse = out.conf.lse; r.held = out.held; r.loss = out.loss; r.target = out.loss && out.loss->target;
    r.K = K_; r.group_k = group_k; r.ragged = ragged(); r.arch_option = cfg.arch_option; r.out_c = cfg.out_c; r.lw0 = lw_[0];
    r.debug = debug; r.strict = strict_; r.headc_packed = headc_.n == cfg.out_c;
    r.corr_full = corr_full; r.corr_generic = corr_generic; r.no_4x = no_4x;
    return r;
}

// forward_refusal's findings (plain values) with the refusals that read the engine's state between them, in the order they are reported
int Engine::check_request(const float* x, int B, const ForwardOut& out, const RouteIn& r) {
    const lseg_config& c = cfg;
    const FwdRefusal f = forward_refusal(r);
    if (f == REFUSE_CONF_NEEDS_LABEL) return set_error(LSEG_ERR_INVALID, "the confidence outputs need the label output");
    if (f == REFUSE_LOSS_NOT_ALONE) return set_error(LSEG_ERR_INVALID, "the loss outputs need the label output and a target, and come with no other output");
    if (!finalized_) return set_error(LSEG_ERR_STATE, "parameters not finalised (call lseg_finalize_params)");
    if (K_ < 1 && !out.held) return set_error(LSEG_ERR_STATE, "no text tokens set (call lseg_set_text_tokens)");
    if (B < 1 || B > c.max_batch) return set_error(LSEG_ERR_INVALID, "B=%d outside [1, max_batch=%d]", B, c.max_batch);
    if (!x) return set_error(LSEG_ERR_INVALID, "x is NULL");
    if (out.held) TRY(check_held("lseg_forward_features"));      // (groupings and train mode are refused there: nothing below meets them)
    if (f == REFUSE_SCORE_NEEDS_LABEL) return set_error(LSEG_ERR_INVALID, "a score output needs the label output");
    if (f == REFUSE_INT16_K) return set_error(LSEG_ERR_UNSUPPORTED, "int16 labels need K <= 32767 (K=%d)", K_);
    if (ragged()) {
        if ((int)groups_.size() != B) return set_error(LSEG_ERR_INVALID, "ragged label sets: set for %d images, forward called with B=%d", (int)groups_.size(), B);
        long total = 0;
        for (int k : groups_) total += k;
        if (total != K_) return set_error(LSEG_ERR_INVALID, "ragged label sets: %d token rows != %ld labels over the %d images", K_, total, B);
    }
    if (train_mode) {                    // net.train(): activations saved for lseg_backward, BatchNorm on batch statistics
        if (ragged()) TRY(check_ragged_train());      // the fused-loss route (train.hip); forward_train refuses a logits output
        if (out.label) return set_error(LSEG_ERR_UNSUPPORTED, "label output is an inference feature (train mode is on)");
        if (out.argmax) return set_error(LSEG_ERR_UNSUPPORTED, "argmax output is an inference feature (train mode is on)");
        if (out.low) return set_error(LSEG_ERR_UNSUPPORTED, "low-resolution logits output is an inference feature (train mode is on)");
        return 0;
    }
    // nothing but the streamed labels exists for ragged groups: every other request is refused before a kernel runs, nothing falls back
    if (f == REFUSE_RAGGED_NOT_LABELS)
        return set_error(LSEG_ERR_UNSUPPORTED, "ragged label sets have no logits: only lseg_forward_labels / lseg_forward_labels_conf run with them");
    if (f == REFUSE_RAGGED_ROUTE)
        return set_error(LSEG_ERR_UNSUPPORTED, "ragged label sets need the streamed kernel: the commuted schedule (no debug taps, no split precision), "
                                               "out_c 512 (is %d), arch_option 0 (is %d), no LSEG_CORR_GENERIC / LSEG_CORR_FULLRES", c.out_c, c.arch_option);
    return 0;
}

// The input format of every forward entry.  The split-precision mode has a first stage of its own (strict.hip: the image as (hi, lo) fp16
// planes) with no uint8 form: refused, nothing falls back.  The patch rows need patch % 16 == 0 (a lane owns 16 pixels of a patch row)
int Engine::set_input_u8(bool on, const NormU8& n) {
    if (!on) { in_u8_ = false; return 0; }
    if (strict_) return set_error(LSEG_ERR_UNSUPPORTED, "lseg_set_input_u8: the split-precision mode (image_dtype LSEG_F16_SPLIT) reads fp32 images only");
    if (!resnet_ && cfg.patch % 16) return set_error(LSEG_ERR_UNSUPPORTED, "lseg_set_input_u8: patch=%d must be a multiple of 16", cfg.patch);
    in_norm_ = n; in_u8_ = true;
    return 0;
}

// ragged label sets in train mode: the fused-loss route on the plain head only.  Refused before any kernel runs: the arch_option 1/2 head
// blocks (their planes are rectangular) and the ResNet-101 decoder-training mode (never run with ragged sets: refused rather than left
// untested).  Deterministic reductions (flags bit 3) need nothing new: the ragged loss kernels hold no fp32 atomic -- the counts are
// integers and the gradient reads only the valid-pixel count, so the rows are bit-reproducible; the loss VALUE is a double atomic sum,
// order-dependent in its last bits exactly as seg_stats_kernel's is
int Engine::check_ragged_train() {
    if (cfg.arch_option != 0) return set_error(LSEG_ERR_UNSUPPORTED, "ragged label sets in train mode need arch_option 0 (is %d): the head blocks "
                                                                      "work on rectangular [B,K,h,w] planes", cfg.arch_option);
    if (resnet_) return set_error(LSEG_ERR_UNSUPPORTED, "ragged label sets in train mode are not implemented for the ResNet-101 tower (decoder training)");
    if (!corr_ragged_supported(cfg.out_c)) return set_error(LSEG_ERR_UNSUPPORTED, "ragged label sets in train mode need out_c %% 64 == 0 and <= 1024 (is %d)", cfg.out_c);
    return 0;
}

// ---- the training step (train.hip): the plan's inputs, and every refusal of forward_train / train_loss / backward before any state changes
TrainHeadIn Engine::train_head_in(bool logits) const {
    TrainHeadIn in;
    in.group_k = group_k; in.ragged = ragged();
    for (int k : groups_) in.kmax = std::max(in.kmax, (int)k);
    in.K = K_; in.hb_n = hb_n_; in.arch_option = cfg.arch_option; in.unrounded = cfg.flags & 2; in.img_dt = img_dt_; in.out_c = cfg.out_c;
    in.logits = logits; in.ragged_gemm = corr_ragged_use_gemm();
    return in;
}

int Engine::check_train_forward(int B, const TrainHead& plan) {
    if (!train_alloc_) return set_error(LSEG_ERR_STATE, "train mode was not enabled (lseg_set_train)");
    TRY(check_grouping(B));
    // (per-image label sets with head blocks: check_grouping above reports the grouped kind, check_request the ragged kind through this)
    if (plan.refusal == TRAIN_REFUSE_HEAD_BLOCKS) return check_ragged_train();
    // ragged per-image label sets: only the fused loss reads their planes (check_request refused everything else before this point)
    if (plan.refusal == TRAIN_REFUSE_RAGGED_LOGITS)
        return set_error(LSEG_ERR_UNSUPPORTED, "ragged label sets have no [B,K,H,W] logits in train mode either: pass no logits output "
                                               "and take the loss from lseg_train_loss / lseg_backward with a target");
    if (plan.refusal == TRAIN_REFUSE_GROUP_SIZE)
        return set_error(LSEG_ERR_UNSUPPORTED, "train mode with per-image label sets supports 1..%d labels per image (got %d) and out_c %% 8 == 0",
                         CORR_GROUP_MAX, group_k);
    return 0;
}

int Engine::check_train_loss(const int64_t* target) {
    if (!train_mode || !train_fwd_valid_) return set_error(LSEG_ERR_STATE, "lseg_train_loss needs a train-mode lseg_forward first");
    if (!target) return set_error(LSEG_ERR_INVALID, "lseg_train_loss: target is NULL");
    return 0;
}

int Engine::check_backward(const float* dlogits, const int64_t* target, const float* dev_grad_scale) {
    if (!train_mode || !train_fwd_valid_) return set_error(LSEG_ERR_STATE, "lseg_backward needs a train-mode lseg_forward first");
    if (dlogits && dev_grad_scale) return set_error(LSEG_ERR_INVALID, "lseg_backward: a gradient scale only applies to the fused loss (target given)");
    if (!dlogits && !target) return set_error(LSEG_ERR_INVALID, "lseg_backward: give d(logits) or a target mask");
    if (train_head_.ragged() && dlogits)
        return set_error(LSEG_ERR_UNSUPPORTED, "ragged label sets have no [B,K,H,W] logits: lseg_backward takes a target, not d(logits)");
    return 0;
}

// held features exist only where the forward's corr_low holds (the correlation commuted below the x2 upsample reads g16pad_ and nscale_ and
// nothing else) and for one label set shared by the batch: everything else is refused before a kernel runs, nothing falls back.
// (No bound on out_c: pixel_gram and the generic GEMM take every width the engine accepts -- the 512 of the streamed labels is the
// width of THEIR kernel, which nothing here runs)
int Engine::check_held(const char* what) {
    if (train_mode) return set_error(LSEG_ERR_UNSUPPORTED, "%s is an inference feature (train mode is on)", what);
    RouteIn r = route_in(ForwardOut{});
    r.held = true;
    const FwdRefusal f = forward_refusal(r);           // (with nothing else asked for: one of the two held-feature refusals or none)
    if (f == REFUSE_HELD_GROUPED) return set_error(LSEG_ERR_UNSUPPORTED, "%s: per-image label sets have no held-feature form (one label set shared by the batch)", what);
    if (f == REFUSE_HELD_ROUTE)
        return set_error(LSEG_ERR_UNSUPPORTED, "%s needs the commuted correlation: the commuted schedule (no debug taps, no split precision), "
                                               "arch_option 0 (is %d), an even quarter-resolution width (is %d), no LSEG_CORR_FULLRES",
                         what, cfg.arch_option, lw_[0]);
    return 0;
}

}  // namespace lseg
