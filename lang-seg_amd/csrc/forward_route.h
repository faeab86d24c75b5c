// forward_route.h -- which schedule Engine::forward runs for a request, and which requests it refuses, as pure functions of plain values
// (no engine, no device): the one table the forward switches over and lseg_op_forward_route / tests/test_forward_route_host.py pin.
#pragma once
#include "ops.h"

namespace lseg {

// the output tails of the inference forward, each named after what it launches behind the image tower and the refinenets
enum FwdTail {
    // corr_low: headc_ GEMM -> g16pad_, gram, scale plane (+ the overflow sentinel copy), then
    TAIL_HELD = 0,            // g16pad_ / nscale_ copied to the caller; no text is read
    TAIL_STREAM_RAGGED,       // corr_argmax over per-image label lists
    TAIL_STREAM_SHARED,       // corr_argmax over the one label set
    TAIL_X4_LOGITS,           // label planes at quarter resolution, then the one-pass scaled x4 upsample into `logits`
    TAIL_X2_LOW_OUT,          // label planes at quarter resolution, then the scaled x2 upsample straight into `low`
    TAIL_PLANES,              // label planes at quarter resolution, scaled x2 upsample into low_, then the planes-in-memory tail
    // not corr_low: a (2h, 2w) feature map a16_, the correlation on it into low_, then the planes-in-memory tail
    TAIL_FEAT_COMMUTED,       // headc_ GEMM (fp32) + upsample_norm_f16
    TAIL_FEAT_ROWNORM,        // head1 GEMM with the MAP_ROWNORM epilogue
    TAIL_FEAT_HEAD1,          // head1 GEMM (fp32) + l2norm_scale_f16
};
// where the quarter-resolution label planes (and the gram behind the scale plane) come from on the corr_low tails that have them
enum FwdPlanes { PLANES_NONE = 0, PLANES_FUSED /* corr_planes: planes + gram */, PLANES_GROUPED /* pixel_gram + B GEMMs */,
                 PLANES_GENERIC /* pixel_gram + one GEMM */ };

struct RouteIn {
    // what the caller wants: ForwardOut's members as booleans (runner_up: conf.label2 or conf.score2; lse: conf.lse; target: loss->target)
    bool logits = false, argmax = false, label = false, score = false, low = false, runner_up = false, lse = false, held = false,
         loss = false, target = false;
    int K = 0, group_k = 0;
    bool ragged = false;
    int arch_option = 0, out_c = 0, lw0 = 0;       // lw0: width of the quarter-resolution map (lw_[0])
    bool debug = false, strict = false;
    bool headc_packed = false;                     // headc_.n == out_c: finalize() packed the commuted head
    bool corr_full = false, corr_generic = false, no_4x = false;       // LSEG_CORR_FULLRES, LSEG_CORR_GENERIC, LSEG_NO_UPSAMPLE4X
};
struct Route { bool commuted, corr_low, corr_fused; FwdTail tail; FwdPlanes planes; };

inline Route forward_route(const RouteIn& r) {
    Route o;
    // the two 1x1 convs behind refinenet1's upsample run as one GEMM below it (everything but the debug taps / the split-precision mode)
    o.commuted = !r.debug && !r.strict && r.headc_packed;
    // ... and so does the correlation
    o.corr_low = o.commuted && !r.corr_full && (r.lw0 % 2) == 0;
    // the dedicated kernel: one label set shared by the batch that fits the LDS
    o.corr_fused = o.corr_low && !r.held && !r.corr_generic && r.group_k == 0 && !r.ragged && corr_planes_supported(r.K, r.out_c);
    o.planes = PLANES_NONE;
    if (!o.corr_low) {
        o.tail = o.commuted ? TAIL_FEAT_COMMUTED : (r.out_c == 512 && !r.debug && !r.strict) ? TAIL_FEAT_ROWNORM : TAIL_FEAT_HEAD1;
        return o;
    }
    if (r.held) o.tail = TAIL_HELD;
    else if (r.ragged) o.tail = TAIL_STREAM_RAGGED;            // (forward_refusal let only the streamed labels through)
    else if (r.label && !r.logits && !r.argmax && !r.corr_generic && r.group_k == 0 && r.arch_option == 0 && corr_argmax_supported(r.K, r.out_c))
        o.tail = TAIL_STREAM_SHARED;                           // masks only, any K.  (`low` wanted as well still streams: as the parent)
    else {
        o.planes = o.corr_fused ? PLANES_FUSED : r.group_k > 0 ? PLANES_GROUPED : PLANES_GENERIC;
        if (r.logits && !r.argmax && r.arch_option == 0 && !r.no_4x) o.tail = TAIL_X4_LOGITS;
        else if (r.low && !r.logits && !r.argmax && !r.label && r.arch_option == 0) o.tail = TAIL_X2_LOW_OUT;
        else o.tail = TAIL_PLANES;
    }
    return o;
}

// The refusals of a request that plain values decide, in the order Engine::check_request reports them (it interleaves the ones that
// need the engine's state: see there).  0: none.
enum FwdRefusal {
    REFUSE_NONE = 0,
    REFUSE_CONF_NEEDS_LABEL,      // LSEG_ERR_INVALID
    REFUSE_LOSS_NOT_ALONE,        // LSEG_ERR_INVALID
    REFUSE_HELD_GROUPED,          // LSEG_ERR_UNSUPPORTED
    REFUSE_HELD_ROUTE,            // LSEG_ERR_UNSUPPORTED
    REFUSE_SCORE_NEEDS_LABEL,     // LSEG_ERR_INVALID
    REFUSE_INT16_K,               // LSEG_ERR_UNSUPPORTED
    REFUSE_RAGGED_NOT_LABELS,     // LSEG_ERR_UNSUPPORTED    (inference only, as the next)
    REFUSE_RAGGED_ROUTE,          // LSEG_ERR_UNSUPPORTED
};
inline FwdRefusal forward_refusal(const RouteIn& r) {
    const bool commuted = !r.debug && !r.strict && r.headc_packed;
    if ((r.runner_up || r.lse) && !r.label) return REFUSE_CONF_NEEDS_LABEL;
    if (r.loss && (!r.label || !r.target || r.runner_up || r.logits || r.argmax || r.low || r.held)) return REFUSE_LOSS_NOT_ALONE;
    if (r.held && (r.group_k > 0 || r.ragged)) return REFUSE_HELD_GROUPED;
    if (r.held && (!commuted || r.corr_full || (r.lw0 % 2) != 0 || r.arch_option != 0)) return REFUSE_HELD_ROUTE;
    if (r.score && !r.label) return REFUSE_SCORE_NEEDS_LABEL;
    if (r.label && !r.ragged && (r.group_k > 0 ? r.group_k : r.K) > 32767) return REFUSE_INT16_K;
    if (r.ragged && !(r.label && !r.logits && !r.argmax && !r.low)) return REFUSE_RAGGED_NOT_LABELS;
    if (r.ragged && (!commuted || r.corr_full || (r.lw0 % 2) != 0 || r.corr_generic || r.arch_option != 0 || r.out_c != 512)) return REFUSE_RAGGED_ROUTE;
    return REFUSE_NONE;
}
inline int refusal_status(FwdRefusal f) {       // lseg_status values (include/lseg_hip.h): 0, LSEG_ERR_INVALID -1, LSEG_ERR_UNSUPPORTED -5
    return f == REFUSE_NONE ? 0 : (f == REFUSE_CONF_NEEDS_LABEL || f == REFUSE_LOSS_NOT_ALONE || f == REFUSE_SCORE_NEEDS_LABEL) ? -1 : -5;
}

}  // namespace lseg
