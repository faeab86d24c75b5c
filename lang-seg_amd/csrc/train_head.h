// train_head.h -- how the label head of the training step runs (correlation, loss rows, correlation backward) and which combinations it
// refuses, as a pure function of plain values (no engine, no device): the one plan Engine::forward_train makes and train_loss / backward
// read, pinned by lseg_op_train_head_plan / tests/test_train_head_host.py.
#pragma once
#include "ops.h"

namespace lseg {

enum TrainMode {
    TRAIN_SHARED = 0,         // one label set shared by the batch: correlate_planes, transposed text as the dgrad operand, GEMM + l2norm backward
    TRAIN_GROUPED,            // group_k labels per image (corr_group.hip): the backward reads tnorm_ itself
    TRAIN_RAGGED_GEMM,        // per-image label lists, stage one (LSEG_CORR_RAGGED_GEMM): per-image GEMMs, transposed panels for the dgrad
    TRAIN_RAGGED_FUSED,       // per-image label lists, stage two: one launch each way, the backward reads tnorm_ itself
};
// in the order forward_train's callers meet them (check_ragged_train / check_grouping report the first, check_train_forward the others)
enum TrainRefusal {
    TRAIN_REFUSE_NONE = 0,
    TRAIN_REFUSE_HEAD_BLOCKS,         // LSEG_ERR_UNSUPPORTED: per-image label sets (either kind) with arch_option 1 / 2
    TRAIN_REFUSE_RAGGED_LOGITS,       // LSEG_ERR_UNSUPPORTED: ragged planes are no [B,K,H,W] logits
    TRAIN_REFUSE_GROUP_SIZE,          // LSEG_ERR_UNSUPPORTED: group_k outside corr_group_supported
};

struct TrainHeadIn {
    int group_k = 0;
    bool ragged = false; int kmax = 0;        // per-image label lists set, and the longest of them
    int K = 0, hb_n = 0, arch_option = 0;
    bool unrounded = false;                   // lseg_config.flags bit 1: the un-rounded gradient
    int img_dt = DT_BF16, out_c = 0;
    bool logits = false;                      // the forward is asked for a [B,K,H,W] logits output
    bool ragged_gemm = false;                 // corr_ragged_use_gemm()
};
struct TrainHead {
    TrainMode mode = TRAIN_SHARED;
    int kout = 0;                 // label planes per image (ragged: unused, the lists differ)
    int Kp = 0;                   // row pitch of d(low): per-image sets (G <= 8) hand the grouped kernel one 16-byte row per pixel
    int hdt = DT_F16;             // dtype of the d(low) rows: fp16 as the reference's half backward, img_dt under flags bit 1
    int kmax = 0;                 // ragged: the longest list
    bool dgrad_operand = false;   // a transposed text operand is made for the correlation's dgrad GEMM(s)
    bool head_blocks = false;     // arch_option 1 / 2 blocks run behind the correlation
    TrainRefusal refusal = TRAIN_REFUSE_NONE;
    bool ragged() const { return mode == TRAIN_RAGGED_GEMM || mode == TRAIN_RAGGED_FUSED; }
};

inline TrainHead train_head_plan(const TrainHeadIn& in) {
    TrainHead p;
    p.mode = in.ragged ? (in.ragged_gemm ? TRAIN_RAGGED_GEMM : TRAIN_RAGGED_FUSED) : in.group_k > 0 ? TRAIN_GROUPED : TRAIN_SHARED;
    p.kout = in.group_k > 0 ? in.group_k : in.K;
    p.kmax = in.ragged ? in.kmax : 0;
    p.Kp = in.ragged ? (int)up64(in.kmax) : in.group_k > 0 ? 8 : (int)up64(in.K);
    p.hdt = in.unrounded ? in.img_dt : DT_F16;
    p.dgrad_operand = p.mode == TRAIN_SHARED || p.mode == TRAIN_RAGGED_GEMM;
    p.head_blocks = in.hb_n > 0;
    if ((in.ragged || in.group_k > 0) && in.arch_option != 0) p.refusal = TRAIN_REFUSE_HEAD_BLOCKS;
    else if (in.ragged && in.logits) p.refusal = TRAIN_REFUSE_RAGGED_LOGITS;
    else if (in.group_k > 0 && !corr_group_supported(in.group_k, in.out_c)) p.refusal = TRAIN_REFUSE_GROUP_SIZE;
    return p;
}

}  // namespace lseg
