// capi.hip -- extern "C" surface of liblseg_hip.so (declared in include/lseg_hip.h).
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>

#include "engine.h"

using namespace lseg;

struct lseg_engine { Engine* e; };

#define GUARD(h) if (!(h) || !(h)->e) return set_error(LSEG_ERR_INVALID, "NULL handle")

static int require_device() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1)
        return set_error(LSEG_ERR_NO_DEVICE, "no HIP device visible: the LSeg engine has no CPU fallback");
    return 0;
}

extern "C" {

int lseg_abi_version(void) { return LSEG_ABI_VERSION; }

int lseg_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* lseg_last_error(lseg_handle h) { (void)h; return last_error(); }

int lseg_create(const lseg_config* cfg, int device, lseg_handle* out) {
    if (!cfg || !out) return set_error(LSEG_ERR_INVALID, "lseg_create: NULL argument");
    int r = require_device();
    if (r) return r;
    int n = lseg_device_count();
    if (device < 0 || device >= n) return set_error(LSEG_ERR_NO_DEVICE, "device %d not in [0,%d)", device, n);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return set_error(LSEG_ERR_HIP, "hipGetDeviceProperties failed");
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return set_error(LSEG_ERR_NO_DEVICE, "device %d is %s; this library is built for gfx950 (MI355X) only", device, prop.gcnArchName);
    Engine* e = new (std::nothrow) Engine(*cfg, device);
    if (!e) return set_error(LSEG_ERR_HIP, "out of host memory");
    r = e->init();
    if (r) { delete e; return r; }
    lseg_engine* h = new (std::nothrow) lseg_engine{e};
    if (!h) { delete e; return set_error(LSEG_ERR_HIP, "out of host memory"); }
    *out = h;
    return LSEG_OK;
}

int lseg_destroy(lseg_handle h) {
    if (!h) return LSEG_OK;
    delete h->e;
    delete h;
    return LSEG_OK;
}

int lseg_bind_param(lseg_handle h, const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim) {
    GUARD(h);
    return h->e->bind(key, dev_ptr, dtype, shape, ndim);
}
int lseg_finalize_params(lseg_handle h, void* stream) { GUARD(h); return h->e->finalize((hipStream_t)stream); }

int lseg_set_text_tokens(lseg_handle h, const int64_t* host_tokens, int K, int ctx) {
    GUARD(h);
    if (!host_tokens) return set_error(LSEG_ERR_INVALID, "tokens NULL");
    return h->e->set_tokens(host_tokens, K, ctx);
}
int lseg_set_text_features(lseg_handle h, const void* dev_feat_f16, int K, void* stream) {
    GUARD(h);
    return h->e->set_text_features(dev_feat_f16, K, (hipStream_t)stream);
}
int lseg_encode_text(lseg_handle h, void* stream) { GUARD(h); return h->e->encode_text((hipStream_t)stream); }
int lseg_set_text_cache(lseg_handle h, int enabled) { GUARD(h); h->e->text_cache = enabled != 0; return LSEG_OK; }
int lseg_set_text_grouping(lseg_handle h, int labels_per_image) {
    GUARD(h);
    if (labels_per_image < 0 || labels_per_image > h->e->cfg.max_labels)
        return set_error(LSEG_ERR_INVALID, "labels_per_image=%d outside [0, max_labels]", labels_per_image);
    h->e->group_k = labels_per_image;
    h->e->clear_text_groups();               // either grouping clears the other
    return LSEG_OK;
}
int lseg_set_text_groups(lseg_handle h, const int32_t* host_counts, int B) {
    GUARD(h);
    return h->e->set_text_groups(host_counts, B);
}
int lseg_get_text_features(lseg_handle h, void* dev_out, void* stream) {
    GUARD(h);
    if (!dev_out) return set_error(LSEG_ERR_INVALID, "out NULL");
    return h->e->get_text_features(dev_out, (hipStream_t)stream);
}

int lseg_set_input_u8(lseg_handle h, int enabled, const float* host_mean3, const float* host_std3) {
    NormU8 n = {};
    if (enabled) {                       // the values are checked before the handle: a bad std is LSEG_ERR_INVALID with or without a device
        int r = norm_u8_check("lseg_set_input_u8", host_mean3, host_std3, &n);
        if (r) return r;
    }
    GUARD(h);
    return h->e->set_input_u8(enabled != 0, n);
}

int lseg_forward(lseg_handle h, const float* dev_x, int B, float* dev_logits_out, uint8_t* dev_argmax_out, void* stream) {
    GUARD(h);
    Engine::ForwardOut out;
    out.logits = dev_logits_out; out.argmax = dev_argmax_out;
    return h->e->forward(dev_x, B, out, (hipStream_t)stream);
}

int lseg_forward_labels(lseg_handle h, const float* dev_x, int B, int16_t* dev_label_out, float* dev_score_out, void* stream) {
    GUARD(h);
    if (!dev_label_out) return set_error(LSEG_ERR_INVALID, "label output is NULL");     // (to the engine an empty request is no error)
    Engine::ForwardOut out;
    out.label = dev_label_out; out.score = dev_score_out;
    return h->e->forward(dev_x, B, out, (hipStream_t)stream);
}

int lseg_forward_labels_conf(lseg_handle h, const float* dev_x, int B, int16_t* dev_label_out, float* dev_score_out, int16_t* dev_label2_out,
                             float* dev_score2_out, float* dev_lse_out, void* stream) {
    GUARD(h);
    if (!dev_label_out) return set_error(LSEG_ERR_INVALID, "label output is NULL");
    Engine::ForwardOut out;
    out.label = dev_label_out; out.score = dev_score_out; out.conf = Engine::LabelConf{dev_label2_out, dev_score2_out, dev_lse_out};
    return h->e->forward(dev_x, B, out, (hipStream_t)stream);
}

int lseg_forward_labels_loss(lseg_handle h, const float* dev_x, int B, const int64_t* dev_target, int ignore_index, int16_t* dev_label_out,
                             float* dev_score_out, float* dev_lse_out, float* dev_nll_plane_out, double* dev_nll, int64_t* dev_counts, void* stream) {
    GUARD(h);
    return h->e->forward_labels_loss(dev_x, B, dev_target, ignore_index, dev_label_out, dev_score_out, dev_lse_out, dev_nll_plane_out, dev_nll,
                                     dev_counts, (hipStream_t)stream);
}

int lseg_forward_lowres(lseg_handle h, const float* dev_x, int B, float* dev_low_out, void* stream) {
    GUARD(h);
    if (!dev_low_out) return set_error(LSEG_ERR_INVALID, "low-resolution logits output is NULL");
    Engine::ForwardOut out;
    out.low = dev_low_out;
    return h->e->forward(dev_x, B, out, (hipStream_t)stream);
}

int lseg_features_bytes(lseg_handle h, int B, size_t* feat_bytes, size_t* scale_bytes) {
    GUARD(h);
    if (B < 1 || B > h->e->cfg.max_batch) return set_error(LSEG_ERR_INVALID, "B=%d outside [1, max_batch=%d]", B, h->e->cfg.max_batch);
    h->e->features_bytes(B, feat_bytes, scale_bytes);
    return LSEG_OK;
}

int lseg_forward_features(lseg_handle h, const float* dev_x, int B, void* dev_feat_out, float* dev_scale_out, void* stream) {
    GUARD(h);
    if (!dev_feat_out || !dev_scale_out) return set_error(LSEG_ERR_INVALID, "held-feature output is NULL");
    const Engine::HeldOut held{dev_feat_out, dev_scale_out};
    Engine::ForwardOut out;
    out.held = &held;
    return h->e->forward(dev_x, B, out, (hipStream_t)stream);
}

int lseg_score_features(lseg_handle h, const void* dev_feat, const float* dev_scale, int B, int row0, int rows, float* dev_low_out, void* stream) {
    GUARD(h);
    return h->e->score_features(dev_feat, dev_scale, B, row0, rows, dev_low_out, (hipStream_t)stream);
}

int lseg_forward_stats(lseg_handle h, const int64_t* dev_target, int ignore_index, int64_t* dev_counts, double* dev_nll, void* stream) {
    GUARD(h);
    return h->e->forward_stats(dev_target, ignore_index, dev_counts, dev_nll, (hipStream_t)stream);
}

int lseg_episode_stats(lseg_handle h, const int64_t* dev_target, const uint8_t* dev_ignore, int ignore_index, const int64_t* dev_class_id,
                       int nclass, int64_t* dev_inter_buf, int64_t* dev_union_buf, int64_t* dev_areas, double* dev_nll, int64_t* dev_flags,
                       void* stream) {
    GUARD(h);
    return h->e->episode_stats(dev_target, dev_ignore, ignore_index, dev_class_id, nclass, dev_inter_buf, dev_union_buf, dev_areas, dev_nll,
                               dev_flags, (hipStream_t)stream);
}

int lseg_set_debug(lseg_handle h, int enabled) { GUARD(h); h->e->debug = enabled != 0; return LSEG_OK; }
int lseg_get_intermediate(lseg_handle h, const char* name, float* dev_out, size_t cap, size_t* n, void* stream) {
    GUARD(h);
    if (!name || !dev_out) return set_error(LSEG_ERR_INVALID, "NULL argument");
    return h->e->get_intermediate(name, dev_out, cap, n, (hipStream_t)stream);
}

int lseg_check_range(lseg_handle h, uint64_t* out4, void* stream) {
    GUARD(h);
    if (!out4) return set_error(LSEG_ERR_INVALID, "NULL argument");
    unsigned long long tmp[4] = {0, 0, 0, 0};
    const int r = h->e->check_range(tmp, (hipStream_t)stream);
    for (int i = 0; i < 4; ++i) out4[i] = tmp[i];
    return r;
}

int lseg_overflow_seen(lseg_handle h, int reset) { GUARD(h); return h->e->overflow_seen(reset != 0); }

int lseg_set_profiling(lseg_handle h, int enabled) {
    GUARD(h);
    // 1 = the whole forward + the MLP fc1 GEMM (rounds 1-2); otherwise a mask, bit f = family f in lseg_get_profile's order
    h->e->prof_mask = enabled == 1 ? 3u : (unsigned)enabled;
    if (enabled) return h->e->reserve_events(2 * h->e->events_per_forward() * 64);     // events for 64 forwards, created outside any timed loop
    return LSEG_OK;
}
int lseg_get_profile(lseg_handle h, const char* family, double* total_ms, int64_t* launches, double* flops) {
    GUARD(h);
    if (!family) return set_error(LSEG_ERR_INVALID, "family NULL");
    return h->e->get_profile(family, total_ms, launches, flops);
}

// ---- training step -----------------------------------------------------------------------------------------
int lseg_set_train(lseg_handle h, int enabled) { GUARD(h); return h->e->set_train(enabled != 0); }
int lseg_bind_grad(lseg_handle h, const char* key, float* dev_grad) { GUARD(h); return h->e->bind_grad(key, dev_grad); }
int lseg_grad_ptr(lseg_handle h, const char* key, float** dev_out, size_t* n) { GUARD(h); return h->e->grad_ptr(key, dev_out, n); }
int lseg_grad_bucket(lseg_handle h, const char* key) { if (!h || !h->e || !key) return -1; return h->e->bucket_of(key); }
int lseg_num_grad_buckets(lseg_handle h) { if (!h || !h->e) return 0; return h->e->n_buckets(); }
int lseg_backward(lseg_handle h, const float* dev_dlogits, const int64_t* dev_target, int ignore_index, int accumulate,
                  double* dev_loss, void* stream) {
    GUARD(h);
    return h->e->backward(dev_dlogits, dev_target, ignore_index, accumulate, dev_loss, (hipStream_t)stream);
}
int lseg_backward_scaled(lseg_handle h, const int64_t* dev_target, int ignore_index, int accumulate, const float* dev_grad_scale, void* stream) {
    GUARD(h);
    return h->e->backward(nullptr, dev_target, ignore_index, accumulate, nullptr, (hipStream_t)stream, dev_grad_scale);
}
int lseg_train_loss(lseg_handle h, const int64_t* dev_target, int ignore_index, double* dev_loss, int64_t* dev_counts, void* stream) {
    GUARD(h);
    return h->e->train_loss(dev_target, ignore_index, dev_loss, dev_counts, (hipStream_t)stream);
}
int lseg_sgd_momentum(lseg_handle h, const char* key, float** dev_out, size_t* n) { GUARD(h); return h->e->sgd_momentum(key, dev_out, n); }
int lseg_sgd_mark_initialized(lseg_handle h, int initialized) { GUARD(h); return h->e->sgd_mark_initialized(initialized != 0); }
int lseg_set_bn_sync(lseg_handle h, lseg_reduce_cb fn, void* user, int world_size) {
    GUARD(h);
    if (world_size < 1) return set_error(LSEG_ERR_INVALID, "world_size %d", world_size);
    h->e->bn_sync_fn = fn; h->e->bn_sync_user = user; h->e->bn_world = fn ? world_size : 1;
    return LSEG_OK;
}
int lseg_set_bucket_callback(lseg_handle h, lseg_bucket_cb fn, void* user) {
    GUARD(h);
    h->e->bucket_fn = fn; h->e->bucket_user = user;
    return LSEG_OK;
}
int lseg_sgd_step(lseg_handle h, float lr_pretrained, float lr_scratch, float momentum, float weight_decay, void* stream) {
    GUARD(h);
    return h->e->sgd_step(lr_pretrained, lr_scratch, momentum, weight_decay, (hipStream_t)stream);
}
int lseg_adam_step(lseg_handle h, double lr_pretrained, double lr_scratch, double beta1, double beta2, double eps, double weight_decay,
                   int64_t step, void* stream) {
    GUARD(h);
    return h->e->adam_step(lr_pretrained, lr_scratch, beta1, beta2, eps, weight_decay, (long long)step, (hipStream_t)stream);
}
int lseg_adam_state(lseg_handle h, const char* key, int which, float** dev_out, size_t* n) { GUARD(h); return h->e->adam_state(key, which, dev_out, n); }
int lseg_set_frozen_encoder(lseg_handle h, int enabled) { GUARD(h); return h->e->set_frozen_encoder(enabled != 0); }

// ---- single operators -----------------------------------------------------------------------------------
static int op_dt(int lseg_dt, int* out) {
    if (lseg_dt == LSEG_F32) { *out = DT_F32; return 0; }
    if (lseg_dt == LSEG_F16) { *out = DT_F16; return 0; }
    if (lseg_dt == LSEG_BF16) { *out = DT_BF16; return 0; }
    return set_error(LSEG_ERR_INVALID, "dtype %d", lseg_dt);
}

int lseg_op_gemm(const void* A, const void* W, const float* bias, const float* residual, void* C, int M, int N, int K,
                 int ab_dtype, int out_dtype, int act, void* stream) {
    int r = require_device(); if (r) return r;
    int ab, od;
    if ((r = op_dt(ab_dtype, &ab)) || (r = op_dt(out_dtype, &od))) return r;
    GemmArgs g;
    gemm_args_init(g);
    g.A = (const uint16_t*)A; g.W = (const uint16_t*)W; g.M = M; g.N = N; g.K = K; g.lda = K; g.ldw = K;
    g.bias = bias; g.act = act;
    if (residual) { g.res_mode = RES_DEST; g.res = residual; g.res_dtype = DT_F32; }
    if (getenv("LSEG_GEMM_DBG") && (atoi(getenv("LSEG_GEMM_DBG")) & 4)) {   // tools/gemm_phase_probe.py: timing dump
        g.res_mode = RES_NONE; g.res2 = residual;
    }
    g.C = C; g.out_dtype = od; g.ldc = N; g.map_mode = MAP_LINEAR;
    return launch_gemm(g, ab, (hipStream_t)stream);
}

int lseg_op_gemm_vit(const void* A, const void* W, const float* bias, void* Cq, void* Ck, void* Cv, int M, int N, int K, int ab_dtype, int kind,
                     int ntok, int npad, int max_grid, void* stream) {
    int r = require_device(); if (r) return r;
    int ab;
    if ((r = op_dt(ab_dtype, &ab))) return r;
    if (kind < 0 || kind > 3 || !bias) return set_error(LSEG_ERR_INVALID, "lseg_op_gemm_vit: kind 0..3 and a bias");
    GemmArgs g;
    gemm_args_init(g);
    g.A = (const uint16_t*)A; g.W = (const uint16_t*)W; g.M = M; g.N = N; g.K = K; g.lda = K; g.ldw = K;
    g.bias = bias; g.C = Cq; g.ldc = N; g.out_dtype = ab; g.map_mode = MAP_LINEAR; g.max_grid = max_grid;
    if (kind == 1) { g.act = ACT_GELU; g.tag = 1; }
    if (kind == 2) { g.res_mode = RES_DEST; g.res = Cq; g.res_dtype = DT_F32; g.out_dtype = DT_F32; }
    if (kind == 3) {
        if (N % 192 || ntok < 1 || npad < ntok || M % ntok) return set_error(LSEG_ERR_INVALID, "lseg_op_gemm_vit: qkv needs N = 3 * heads * 64, M = B * ntok");
        g.map_mode = MAP_QKV; g.Ck = Ck; g.Cv = Cv; g.qkv_dim = N / 3; g.qkv_ntok = ntok; g.qkv_npad = npad; g.qkv_heads = N / 192;
    }
    return launch_gemm(g, ab, (hipStream_t)stream);
}

int lseg_op_gemm_res32(const void* A, const void* W, const float* bias, float* C, int M, int N, int K, int rows_alloc, int ab_dtype, int impl,
                       int max_grid, void* stream) {
    int r = require_device(); if (r) return r;
    int ab;
    if ((r = op_dt(ab_dtype, &ab))) return r;
    if (!bias || M < 1 || rows_alloc < M) return set_error(LSEG_ERR_INVALID, "lseg_op_gemm_res32: needs a bias and rows_alloc >= M");
    GemmArgs g;
    gemm_args_init(g);
    g.A = (const uint16_t*)A; g.W = (const uint16_t*)W; g.M = M; g.N = N; g.K = K; g.lda = K; g.ldw = K;
    g.bias = bias; g.C = C; g.ldc = N; g.map_mode = MAP_LINEAR; g.max_grid = max_grid;
    g.res_mode = RES_DEST; g.res = C; g.res_dtype = DT_F32; g.out_dtype = DT_F32;
    g.rows_alloc = impl == 0 ? 0 : rows_alloc;
    if (impl == 1) {
        if (!gemm_res32_asm_eligible(g, ab)) return set_error(LSEG_ERR_UNSUPPORTED, "lseg_op_gemm_res32: shape / padding does not qualify for the hand-scheduled kernel");
        return launch_gemm_res32_asm(g, ab, (hipStream_t)stream);
    }
    return launch_gemm(g, ab, (hipStream_t)stream);
}

// lseg_gemm_case -> the GemmArgs the schedules would build for it (engine.h builders); every refusal of a malformed case
static int gemm_case_args(const lseg_gemm_case* c, GemmArgs& g, int* ab) {
    if (!c) return set_error(LSEG_ERR_INVALID, "lseg_op_gemm_ex: NULL case");
    int r, od, rd = DT_F32;
    if ((r = op_dt(c->ab_dtype, ab)) || (r = op_dt(c->out_dtype, &od))) return r;
    if (*ab == DT_F32) return set_error(LSEG_ERR_INVALID, "lseg_op_gemm_ex: operands must be bf16 or fp16");
    if (c->residual && (r = op_dt(c->res_dtype, &rd))) return r;
    if (!c->A || !c->W || !c->C) return set_error(LSEG_ERR_INVALID, "lseg_op_gemm_ex: NULL operand or output");
    if (c->M < 1 || c->N < 1 || c->K < 1) return set_error(LSEG_ERR_INVALID, "lseg_op_gemm_ex: empty problem %dx%dx%d", c->M, c->N, c->K);
    if (c->form < 0 || c->form > 3) return set_error(LSEG_ERR_INVALID, "lseg_op_gemm_ex: form %d (0..3)", c->form);
    if (c->tag < 0 || c->tag > 1) return set_error(LSEG_ERR_INVALID, "lseg_op_gemm_ex: tag %d (0 | 1)", c->tag);
    if (c->tile != 0 && c->tile != 1 && c->tile != 2 && c->tile != 6) return set_error(LSEG_ERR_INVALID, "lseg_op_gemm_ex: tile %d (0, 1, 2, 6)", c->tile);
    if (c->max_grid < 0 || (c->max_grid % 8)) return set_error(LSEG_ERR_INVALID, "lseg_op_gemm_ex: max_grid %d (0 or a multiple of 8)", c->max_grid);
    if (c->act != ACT_NONE && c->act != ACT_GELU && c->act != ACT_RELU) return set_error(LSEG_ERR_INVALID, "lseg_op_gemm_ex: act %d (0, 1, 3)", c->act);
    if (c->form != 0 && (c->act != ACT_NONE || c->nsplit > 1 || !c->bias))
        return set_error(LSEG_ERR_INVALID, "lseg_op_gemm_ex: forms 1..3 take a bias, no activation and no split-K");
    if (c->form != 0 && c->form != 3 && c->residual) return set_error(LSEG_ERR_INVALID, "lseg_op_gemm_ex: forms 1 and 2 take no residual");
    if (c->nsplit < 0 || c->split_steps < 0) return set_error(LSEG_ERR_INVALID, "lseg_op_gemm_ex: negative split-K range");
    Lin w;
    w.w = (uint16_t*)c->W; w.b = (float*)c->bias; w.n = c->N; w.k = c->K;
    switch (c->form) {
        case 0:
            g = lin_args(c->A, w, c->M, c->C, od);
            g.act = c->act;
            if (c->residual) add_residual(g, c->residual, rd);
            g.nsplit = c->nsplit; g.split_steps = c->split_steps; g.c_split_stride = c->c_split_stride;
            break;
        case 1:
            if (c->heads < 1 || c->K != c->heads * 64 || c->N != 3 * c->K || c->ntok < 1 || c->npad < c->ntok || c->M % c->ntok || !c->Ck || !c->Cv)
                return set_error(LSEG_ERR_INVALID, "lseg_op_gemm_ex: qkv needs K = heads * 64, N = 3 K, M = B * ntok, npad >= ntok, Ck and Cv");
            g = qkv_args(c->A, w, c->M, c->C, c->Ck, c->Cv, c->ntok, c->npad, c->heads, od);
            g.qkv_qscale = c->qscale;
            break;
        case 2:
            if (c->s < 1 || c->ch < 1 || c->ho < 1 || c->wo < 1 || c->N != c->s * c->s * c->ch || c->M % (c->ho * c->wo))
                return set_error(LSEG_ERR_INVALID, "lseg_op_gemm_ex: pixel shuffle needs N = s * s * ch and M = B * ho * wo");
            g = pixshuf_args(c->A, w, c->M, c->C, c->ch, c->s, c->ho, c->wo, od);
            break;
        default:
            if (!c->residual || c->p_div < 1 || c->p_off < 0 || c->p_mul < c->p_div + c->p_off || c->M % c->p_div || c->ldr < c->N)
                return set_error(LSEG_ERR_INVALID, "lseg_op_gemm_ex: periodic rows need a table, M = B * p_div, p_mul >= p_div + p_off >= p_div, ldr >= N");
            g = lin_args(c->A, w, c->M, c->C, od);
            to_periodic_rows(g, c->residual, rd, c->ldr, c->p_div, c->p_mul, c->p_off);
            break;
    }
    g.tag = c->tag; g.tile_hint = c->tile; g.max_grid = c->max_grid;
    return 0;
}

int lseg_op_gemm_ex(const lseg_gemm_case* c, void* stream) {
    GemmArgs g;
    int ab, r = gemm_case_args(c, g, &ab);
    if (r) return r;
    if ((r = gemm_check(g, ab))) return r;                 // every refusal of the launcher, before a device is asked for
    if ((r = require_device())) return r;
    return launch_gemm(g, ab, (hipStream_t)stream);
}

int lseg_op_gemm_ex_plan(const lseg_gemm_case* c, int cus, int* out4) {
    if (!out4) return set_error(LSEG_ERR_INVALID, "lseg_op_gemm_ex_plan: NULL pointer");
    GemmArgs g;
    int ab, r = gemm_case_args(c, g, &ab);
    if (r) return r;
    GemmPlan p;
    if ((r = gemm_plan(g, ab, cus, p))) return r;
    out4[0] = p.epi; out4[1] = p.tile; out4[2] = p.grid; out4[3] = p.items;
    return 0;
}

int lseg_op_colsum(const void* in, int dtype, float* out, int R, int C, int ld, int accumulate, float* det_ws, size_t det_cap, void* stream) {
    int r = require_device(); if (r) return r;
    int dt;
    if ((r = op_dt(dtype, &dt))) return r;
    if (!in || !out || R < 1 || C < 1 || ld < C) return set_error(LSEG_ERR_INVALID, "lseg_op_colsum: R, C >= 1, ld >= C");
    return launch_colsum16(in, dt, out, R, C, ld, (hipStream_t)stream, accumulate, det_ws, det_ws ? det_cap : 0);
}

int lseg_op_bn_stats(const void* x, float* stats, int B, int H, int W, int C, int dtype, float* det_ws, size_t det_cap, void* stream) {
    int r = require_device(); if (r) return r;
    int dt;
    if ((r = op_dt(dtype, &dt))) return r;
    if (!x || !stats || (C % 8)) return set_error(LSEG_ERR_INVALID, "lseg_op_bn_stats: C must be a multiple of 8");
    return launch_bn_stats(x, stats, B, H, W, C, dt, (hipStream_t)stream, 0, det_ws, det_ws ? det_cap : 0);
}

int lseg_op_bn_bwd_stats(const void* dy, const void* x, const float* stats, float* bstats, int B, int H, int W, int C, float eps, int dtype,
                         float* det_ws, size_t det_cap, void* stream) {
    int r = require_device(); if (r) return r;
    int dt;
    if ((r = op_dt(dtype, &dt))) return r;
    if (!dy || !x || !stats || !bstats || (C % 8)) return set_error(LSEG_ERR_INVALID, "lseg_op_bn_bwd_stats: C must be a multiple of 8");
    return launch_bn_bwd_stats(dy, x, stats, bstats, B, H, W, C, eps, (double)B * H * W, dt, (hipStream_t)stream, det_ws, det_ws ? det_cap : 0);
}

int lseg_op_layernorm(const void* in, int in_dtype, const float* gamma, const float* beta, void* out, int out_dtype,
                      int M, int D, float eps, void* stream) {
    int r = require_device(); if (r) return r;
    int id, od;
    if ((r = op_dt(in_dtype, &id)) || (r = op_dt(out_dtype, &od))) return r;
    return launch_layernorm(in, id, gamma, beta, out, od, M, D, eps, (hipStream_t)stream);
}

int lseg_op_attention(const void* q, const void* k, const void* vt, void* out, int B, int H, int Ntok, int Npad,
                      int dtype, int causal, float scale, void* stream) {
    int r = require_device(); if (r) return r;
    int dt;
    if ((r = op_dt(dtype, &dt))) return r;
    return launch_attention(q, k, vt, out, B, H, Ntok, Npad, dt, causal, scale, (hipStream_t)stream);
}

int lseg_op_attention_prescaled(const void* q, const void* k, const void* vt, void* out, float* lse2, int B, int H, int Ntok, int Npad,
                                int dtype, void* stream) {
    int r = require_device(); if (r) return r;
    int dt;
    if ((r = op_dt(dtype, &dt))) return r;
    return launch_attention_ex(q, k, vt, out, lse2, B, H, Ntok, Npad, dt, 0, 1.0f, 1, (hipStream_t)stream);
}

int lseg_op_attention_ex(const void* q, const void* k, const void* vt, void* out, float* lse2, int B, int H, int Ntok, int Npad, int dtype,
                         int causal, float scale, int prescaled, void* stream) {
    int r = require_device(); if (r) return r;
    int dt;
    if ((r = op_dt(dtype, &dt))) return r;
    if (!q || !k || !vt || !out) return set_error(LSEG_ERR_INVALID, "attention_ex: NULL pointer");
    if (B < 1 || H < 1 || Ntok < 1) return set_error(LSEG_ERR_INVALID, "attention_ex: bad shape");
    return launch_attention_ex(q, k, vt, out, lse2, B, H, Ntok, Npad, dt, causal, scale, prescaled, (hipStream_t)stream);
}

int lseg_op_attention_plan(int B, int H, int Ntok, int causal, int prescaled, int cus, int* out6) {
    if (!out6) return set_error(LSEG_ERR_INVALID, "attention_plan: NULL pointer");
    AttnPlan p;
    const int r = plan_attention(B, H, Ntok, causal, prescaled, cus, p);
    if (r) return r;
    out6[0] = p.nw; out6[1] = p.nqb; out6[2] = p.grid; out6[3] = p.last_tiles; out6[4] = p.xcd_map; out6[5] = p.lds;
    return 0;
}

int lseg_op_attention_strict(const void* q, const void* k, const void* vt, void* out, size_t qk_plane, size_t vt_plane, size_t out_plane,
                             int B, int H, int Ntok, int Npad, float scale, void* stream) {
    int r = require_device(); if (r) return r;
    if (!q || !k || !vt || !out) return set_error(LSEG_ERR_INVALID, "attention_strict: NULL pointer");
    if (B < 1 || H < 1 || Ntok < 1) return set_error(LSEG_ERR_INVALID, "attention_strict: bad shape");
    return launch_attention_strict(q, k, vt, out, qk_plane, vt_plane, out_plane, B, H, Ntok, Npad, scale, (hipStream_t)stream);
}

// One description of an implicit-GEMM conv on padded NHWC maps, the way Engine::conv3x3 builds it: lseg_op_conv3x3, lseg_op_conv and
// lseg_op_conv_ex all launch what this returns.
static GemmArgs conv_args(const void* in, const void* w_packed, const float* bias, const void* residual, const void* residual2, void* out, int B,
                          int H, int W, int Cin, int Cout, int ksize, int stride, int relu_in, int relu_out, int relu_after_res, int dt) {
    GemmArgs g;
    gemm_args_init(g);
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1, taps = ksize == 1 ? 1 : 9;
    g.A = (const uint16_t*)in; g.W = (const uint16_t*)w_packed; g.M = B * Ho * Wo; g.N = Cout; g.K = taps * Cin;
    g.lda = Cin; g.ldw = taps * Cin;
    g.conv = 1; g.ksize = ksize; g.cin = Cin; g.hp = H + 2; g.wp = W + 2; g.ho = Ho; g.wo = Wo; g.stride = stride; g.relu_in = relu_in;
    g.bias = bias; g.act = relu_out ? ACT_RELU : ACT_NONE;
    if (residual) { g.res_mode = RES_DEST; g.res = residual; g.res_dtype = dt; g.res2 = residual2; g.relu_after_res = relu_after_res; }
    g.C = out; g.out_dtype = dt; g.ldc = Cout; g.map_mode = MAP_PADDED;
    return g;
}

int lseg_op_conv3x3(const void* in, const void* w_packed, const float* bias, const void* residual, void* out, int B,
                    int H, int W, int Cin, int Cout, int stride, int relu_in, int relu_out, void* stream) {
    int r = require_device(); if (r) return r;
    const GemmArgs g = conv_args(in, w_packed, bias, residual, nullptr, out, B, H, W, Cin, Cout, 3, stride, relu_in, relu_out, 0, DT_BF16);
    return launch_gemm(g, DT_BF16, (hipStream_t)stream);
}

int lseg_op_rn_stem(const float* x, const float* w, const float* bias, void* out, int B, int H, int W, int dtype, void* stream) {
    int r = require_device(); if (r) return r;
    int dt;
    if ((r = op_dt(dtype, &dt))) return r;
    return launch_rn_stem(x, w, bias, out, B, H, W, dt, (hipStream_t)stream);
}

// the uint8 first stages (input_u8.hip): the argument checks come before the device is looked for
int lseg_op_rn_stem_u8(const uint8_t* x, const float* w, const float* bias, void* out, int B, int H, int W, int dtype, const float* host_mean3,
                       const float* host_std3, void* stream) {
    int r, dt;
    NormU8 n;
    if ((r = norm_u8_check("rn_stem_u8", host_mean3, host_std3, &n))) return r;
    if ((r = op_dt(dtype, &dt))) return r;
    if ((r = rn_stem_u8_check(x, w, bias, out, B, H, W, dt))) return r;
    if ((r = require_device())) return r;
    return launch_rn_stem_u8(x, w, bias, out, B, H, W, dt, n, (hipStream_t)stream);
}

int lseg_op_patch_rows(const float* x, void* A, int B, int H, int W, int P, int dtype, void* stream) {
    int r, dt;
    if (!x || !A) return set_error(LSEG_ERR_INVALID, "patch_rows: NULL pointer");
    if ((r = op_dt(dtype, &dt))) return r;
    if (dt == DT_F32) return set_error(LSEG_ERR_INVALID, "patch_rows: dtype %d", dtype);
    if (B < 1 || H < 1 || W < 1 || P < 1 || H % P || W % P) return set_error(LSEG_ERR_INVALID, "patch_rows: B=%d H=%d W=%d P=%d (H, W multiples of P)", B, H, W, P);
    if (P % 8) return set_error(LSEG_ERR_UNSUPPORTED, "patch_rows: P=%d must be a multiple of 8", P);
    if (((uintptr_t)x | (uintptr_t)A) & 15) return set_error(LSEG_ERR_INVALID, "patch_rows: pointers must be 16-byte aligned");
    if ((r = require_device())) return r;
    return launch_im2col_patch(x, A, B, H, W, P, dt, (hipStream_t)stream);
}

int lseg_op_patch_rows_u8(const uint8_t* x, void* A, int B, int H, int W, int P, int dtype, const float* host_mean3, const float* host_std3,
                          void* stream) {
    int r, dt;
    NormU8 n;
    if ((r = norm_u8_check("patch_rows_u8", host_mean3, host_std3, &n))) return r;
    if ((r = op_dt(dtype, &dt))) return r;
    if ((r = im2col_patch_u8_check(x, A, B, H, W, P, dt))) return r;
    if ((r = require_device())) return r;
    return launch_im2col_patch_u8(x, A, B, H, W, P, dt, n, (hipStream_t)stream);
}

int lseg_op_rn_maxpool(const void* in, void* out, int B, int H, int W, int C, int dtype, void* stream) {
    int r = require_device(); if (r) return r;
    int dt;
    if ((r = op_dt(dtype, &dt))) return r;
    return launch_rn_maxpool(in, out, B, H, W, C, dt, (hipStream_t)stream);
}

int lseg_op_conv(const void* in, const void* w_packed, const float* bias, const void* residual, void* out, int B, int H, int W, int Cin,
                 int Cout, int ksize, int stride, int relu_out, int relu_after_res, int dtype, void* stream) {
    int r = require_device(); if (r) return r;
    int dt;
    if ((r = op_dt(dtype, &dt))) return r;
    if (dt == DT_F32) return set_error(LSEG_ERR_INVALID, "lseg_op_conv: 16-bit maps only");
    if (ksize != 1 && ksize != 3) return set_error(LSEG_ERR_INVALID, "lseg_op_conv: ksize %d (1 or 3)", ksize);
    if (stride != 1 && stride != 2) return set_error(LSEG_ERR_INVALID, "lseg_op_conv: stride %d (1 or 2)", stride);
    const GemmArgs g = conv_args(in, w_packed, bias, residual, nullptr, out, B, H, W, Cin, Cout, ksize, stride, 0, relu_out, relu_after_res, dt);
    return launch_gemm(g, dt, (hipStream_t)stream);
}

// lseg_conv_case -> the GemmArgs Engine::conv3x3 would build for it; every refusal of a malformed case
static int conv_case_args(const lseg_conv_case* c, GemmArgs& g, int* dt) {
    if (!c) return set_error(LSEG_ERR_INVALID, "lseg_op_conv_ex: NULL case");
    int r;
    if ((r = op_dt(c->dtype, dt))) return r;
    if (*dt == DT_F32) return set_error(LSEG_ERR_INVALID, "lseg_op_conv_ex: 16-bit maps only");
    if (!c->in || !c->w || !c->out) return set_error(LSEG_ERR_INVALID, "lseg_op_conv_ex: NULL operand or output");
    if (c->B < 1 || c->H < 1 || c->W < 1 || c->Cin < 1 || c->Cout < 1) return set_error(LSEG_ERR_INVALID, "lseg_op_conv_ex: empty problem");
    if (c->ksize != 1 && c->ksize != 3) return set_error(LSEG_ERR_INVALID, "lseg_op_conv_ex: ksize %d (1 or 3)", c->ksize);
    if (c->stride != 1 && c->stride != 2) return set_error(LSEG_ERR_INVALID, "lseg_op_conv_ex: stride %d (1 or 2)", c->stride);
    if (c->tile != 0 && c->tile != 1 && c->tile != 2 && c->tile != 6) return set_error(LSEG_ERR_INVALID, "lseg_op_conv_ex: tile %d (0, 1, 2, 6)", c->tile);
    if (c->max_grid < 0 || (c->max_grid % 8)) return set_error(LSEG_ERR_INVALID, "lseg_op_conv_ex: max_grid %d (0 or a multiple of 8)", c->max_grid);
    if (c->residual2 && !c->residual) return set_error(LSEG_ERR_INVALID, "lseg_op_conv_ex: residual2 without residual");
    if (c->relu_after_res && (!c->residual || !c->relu_out)) return set_error(LSEG_ERR_INVALID, "lseg_op_conv_ex: relu_after_res needs relu_out and a residual");
    if (c->nsplit < 0 || c->split_steps < 0) return set_error(LSEG_ERR_INVALID, "lseg_op_conv_ex: negative split-K range");
    g = conv_args(c->in, c->w, c->bias, c->residual, c->residual2, c->out, c->B, c->H, c->W, c->Cin, c->Cout, c->ksize, c->stride,
                  c->relu_in ? 1 : 0, c->relu_out ? 1 : 0, c->relu_after_res ? 1 : 0, *dt);
    g.C_relu = c->out_relu;
    if (c->nsplit > 1) {                       // what Engine::conv3x3 launches before conv_reduce_pad: fp32 slabs, MAP_LINEAR, no epilogue terms
        if (c->bias || c->residual || c->out_relu || c->relu_out || c->relu_in)
            return set_error(LSEG_ERR_INVALID, "lseg_op_conv_ex: the split-K form takes no bias, residual, ReLU or out_relu");
        if (c->c_split_stride < (size_t)g.M * g.N) return set_error(LSEG_ERR_INVALID, "lseg_op_conv_ex: c_split_stride is smaller than one slab");
        g.out_dtype = DT_F32; g.map_mode = MAP_LINEAR;
        g.nsplit = c->nsplit; g.split_steps = c->split_steps; g.c_split_stride = c->c_split_stride;
    }
    g.tile_hint = c->tile; g.max_grid = c->max_grid;
    return 0;
}

int lseg_op_conv_ex(const lseg_conv_case* c, void* stream) {
    GemmArgs g;
    int dt, r = conv_case_args(c, g, &dt);
    if (r) return r;
    if ((r = gemm_check(g, dt))) return r;                 // every refusal of the launcher, before a device is asked for
    if ((r = require_device())) return r;
    return launch_gemm(g, dt, (hipStream_t)stream);
}

int lseg_op_conv_ex_plan(const lseg_conv_case* c, int cus, int* out4) {
    if (!out4) return set_error(LSEG_ERR_INVALID, "lseg_op_conv_ex_plan: NULL pointer");
    GemmArgs g;
    int dt, r = conv_case_args(c, g, &dt);
    if (r) return r;
    GemmPlan p;
    if ((r = gemm_plan(g, dt, cus, p))) return r;
    out4[0] = p.epi; out4[1] = p.tile; out4[2] = p.grid; out4[3] = p.items;
    return 0;
}

int lseg_op_conv_splitk_plan(int M, int N, int K, size_t ws_floats, int* ns, int* steps) {
    if (!ns || !steps) return set_error(LSEG_ERR_INVALID, "lseg_op_conv_splitk_plan: NULL pointer");
    if (M < 1 || N < 64 || (N % 64) || K < 64 || (K % 64)) return set_error(LSEG_ERR_INVALID, "lseg_op_conv_splitk_plan: M >= 1, N and K multiples of 64");
    conv_splitk_plan(M, N, K, ws_floats, ns, steps);
    return 0;
}

int lseg_op_conv_reduce_pad(const float* part, int ns, size_t stride, const float* bias, const void* res, const void* res2, void* out, void* out_relu,
                            int B, int Ho, int Wo, int C, int relu, int relu_after_res, int dtype, void* stream) {
    int dt, r;
    if ((r = op_dt(dtype, &dt))) return r;
    if (dt == DT_F32) return set_error(LSEG_ERR_INVALID, "conv_reduce_pad: 16-bit maps only");
    if (!part || !out) return set_error(LSEG_ERR_INVALID, "conv_reduce_pad: NULL slabs or output");
    if (ns < 1 || B < 1 || Ho < 1 || Wo < 1 || C < 1) return set_error(LSEG_ERR_INVALID, "conv_reduce_pad: ns, B, Ho, Wo, C >= 1");
    if (C % 8) return set_error(LSEG_ERR_UNSUPPORTED, "conv_reduce_pad: C=%d must be a multiple of 8", C);
    if (ns > 1 && stride < (size_t)B * Ho * Wo * C) return set_error(LSEG_ERR_INVALID, "conv_reduce_pad: stride=%zu is smaller than one slab", stride);
    if (stride % 4) return set_error(LSEG_ERR_INVALID, "conv_reduce_pad: stride must be a multiple of 4 floats");
    if (res2 && !res) return set_error(LSEG_ERR_INVALID, "conv_reduce_pad: res2 without res");
    const void* const vec[5] = {part, res, res2, out, out_relu};                                        // float4 slab loads, uint4 map loads and stores
    for (const void* p : vec)
        if ((uintptr_t)p % 16) return set_error(LSEG_ERR_INVALID, "conv_reduce_pad: part, res, res2, out and out_relu must be 16-byte aligned");
    if ((r = require_device())) return r;
    return launch_conv_reduce_pad(part, ns, stride, bias, res, res2, out, out_relu, B, Ho, Wo, C, relu ? 1 : 0, dt, (hipStream_t)stream,
                                  res && relu_after_res ? 1 : 0);
}

int lseg_op_conv_wgrad(const void* dy_pad, const void* x_pad, float* dw, int relu_x, int B, int H, int W, int Cin, int Cout, float* ws, size_t ws_floats,
                       int dtype, void* stream) {
    int dt, r;
    if ((r = op_dt(dtype, &dt))) return r;
    if (dt == DT_F32) return set_error(LSEG_ERR_INVALID, "conv_wgrad: 16-bit maps only");
    if (!dy_pad || !x_pad || !dw || !ws || B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1) return set_error(LSEG_ERR_INVALID, "conv_wgrad: bad arguments");
    if ((Cin % 128) != 0 || !wgrad_kmajor_ok(Cout, 9 * Cin, ws_floats))
        return set_error(LSEG_ERR_UNSUPPORTED, "conv_wgrad: needs Cin %% 128 == 0 and a workspace of Cout * 9 * Cin floats (Cin=%d Cout=%d)", Cin, Cout);
    if ((r = require_device())) return r;
    int ns = 0;
    if ((r = launch_conv_wgrad_kmajor(dy_pad, x_pad, relu_x ? 1 : 0, B, H, W, Cin, Cout, ws, ws_floats, dt, &ns, (hipStream_t)stream))) return r;
    const size_t n = (size_t)Cout * 9 * Cin;
    if ((r = launch_sum_partials(ws, dw, ns, n, n, 0, (hipStream_t)stream))) return r;
    return ns;
}

int lseg_op_wgrad_kmajor(const void* dy, int ldy, const void* x, int ldx, int M, int rows_out, int cols_out, float* dw, int accumulate, float* ws,
                         size_t ws_floats, int dtype, void* stream) {
    int dt, r;
    if ((r = op_dt(dtype, &dt))) return r;
    if (dt == DT_F32) return set_error(LSEG_ERR_INVALID, "wgrad_kmajor: 16-bit operands only");
    if (!dy || !x || !dw || !ws || M < 1 || rows_out < 1 || cols_out < 1 || ldy < rows_out || ldx < cols_out || (ldy % 8) || (ldx % 8))
        return set_error(LSEG_ERR_INVALID, "wgrad_kmajor: bad arguments (ldy >= rows_out, ldx >= cols_out, both multiples of 8)");
    if (!wgrad_kmajor_ok(rows_out, cols_out, ws_floats))
        return set_error(LSEG_ERR_UNSUPPORTED, "wgrad_kmajor: needs cols_out %% 128 == 0 and a workspace of rows_out * cols_out floats (%d x %d)", rows_out, cols_out);
    if ((r = require_device())) return r;
    return launch_wgrad_kmajor(dy, ldy, x, ldx, M, rows_out, cols_out, dw, accumulate ? 1 : 0, ws, ws_floats, dt, (hipStream_t)stream);
}

int lseg_op_conv_dgrad_pack(const void* wp, void* wd, int Co, int Ci, void* stream) {
    if (!wp || !wd || Co < 1 || Ci < 1) return set_error(LSEG_ERR_INVALID, "conv_dgrad_pack: bad arguments");
    int r = require_device(); if (r) return r;
    return launch_conv_dgrad_pack(wp, wd, Co, Ci, (hipStream_t)stream);
}

int lseg_op_pack_conv3x3(const float* w, const float* bn_w, const float* bn_b, const float* bn_m, const float* bn_v, float bn_eps, const float* conv_bias,
                         void* wp, float* bias_out, int Co, int Ci, int Cip, int dtype, void* stream) {
    int dt, r;
    if ((r = op_dt(dtype, &dt))) return r;
    if (!w || !wp || Co < 1 || Ci < 1 || Cip < Ci) return set_error(LSEG_ERR_INVALID, "pack_conv3x3: bad arguments (Cip >= Ci)");
    if (bn_w && (!bn_b || !bn_m || !bn_v)) return set_error(LSEG_ERR_INVALID, "pack_conv3x3: BatchNorm needs weight, bias, mean and variance");
    if ((r = require_device())) return r;
    return launch_pack_conv3x3(w, bn_w, bn_b, bn_m, bn_v, bn_eps, conv_bias, wp, bias_out, Co, Ci, Cip, dt, (hipStream_t)stream);
}

int lseg_op_pack_conv1x1(const float* w, const float* bn_w, const float* bn_b, const float* bn_m, const float* bn_v, float bn_eps, void* wp,
                         float* bias_out, int Co, int Ci, int dtype, void* stream) {
    int dt, r;
    if ((r = op_dt(dtype, &dt))) return r;
    if (!w || !wp || !bias_out || Co < 1 || Ci < 1) return set_error(LSEG_ERR_INVALID, "pack_conv1x1: bad arguments");
    if (bn_w && (!bn_b || !bn_m || !bn_v)) return set_error(LSEG_ERR_INVALID, "pack_conv1x1: BatchNorm needs weight, bias, mean and variance");
    if ((r = require_device())) return r;
    return launch_pack_conv1x1(w, bn_w, bn_b, bn_m, bn_v, bn_eps, wp, bias_out, Co, Ci, dt, (hipStream_t)stream);
}

int lseg_op_upsample2x_nhwc(const void* in, void* out, int B, int H, int W, int C, void* stream) {
    int r = require_device(); if (r) return r;
    return launch_upsample2x_nhwc(in, out, B, H, W, C, DT_BF16, (hipStream_t)stream);
}

int lseg_op_upsample2x_planes(const float* in, float* out, int P, int H, int W, void* stream) {
    int r = require_device(); if (r) return r;
    return launch_upsample2x_planes(in, out, P, H, W, (hipStream_t)stream);
}

int lseg_op_upsample4x_planes_scaled(const float* in_padded, const float* scale, float* out, int B, int K, int H, int W, int two_stage,
                                     float* low_scratch, void* stream) {
    int r = require_device(); if (r) return r;
    if (!in_padded || !scale || !out || B < 1 || K < 1 || H < 2 || W < 2) return set_error(LSEG_ERR_INVALID, "upsample4x_planes_scaled: bad arguments");
    if (!two_stage) return launch_upsample4x_planes_scaled(in_padded, scale, out, B * K, K, H, W, (hipStream_t)stream);
    if (!low_scratch) return set_error(LSEG_ERR_INVALID, "upsample4x_planes_scaled: the two-stage form needs the [B,K,2H,2W] scratch");
    r = launch_upsample2x_planes_scaled(in_padded, scale, low_scratch, B * K, K, H, W, (hipStream_t)stream);
    if (r) return r;
    return launch_upsample2x_planes(low_scratch, out, B * K, 2 * H, 2 * W, (hipStream_t)stream);
}

// ---- the output tail's remaining kernels, one launch each (tests/test_gpu_output_tail.py holds them to fp64 references) ----------------
int lseg_op_pixel_gram(const void* d_g16pad, float* d_gram, int B, int H, int W, int C, void* stream) {
    int r = require_device(); if (r) return r;
    if (!d_g16pad || !d_gram || B < 1 || H < 1 || W < 1 || C < 1) return set_error(LSEG_ERR_INVALID, "pixel_gram: bad arguments");
    return launch_pixel_gram(d_g16pad, d_gram, B, H, W, C, (hipStream_t)stream);
}

int lseg_op_norm_scale_plane(const float* d_gram, float* d_scale, int B, int H, int W, float s, unsigned* d_flag, void* stream) {
    int r = require_device(); if (r) return r;
    if (!d_gram || !d_scale || B < 1 || H < 2 || W < 2) return set_error(LSEG_ERR_INVALID, "norm_scale_plane: bad arguments (H, W >= 2)");
    return launch_norm_scale_plane(d_gram, d_scale, B, H, W, s, (hipStream_t)stream, d_flag);
}

int lseg_op_upsample_norm_f16(const float* d_g32pad, void* d_a16, int B, int H, int W, int C, float scale, void* stream) {
    int r = require_device(); if (r) return r;
    if (!d_g32pad || !d_a16 || B < 1 || H < 2 || W < 2 || C < 1) return set_error(LSEG_ERR_INVALID, "upsample_norm_f16: bad arguments (H, W >= 2)");
    return launch_upsample_norm_f16(d_g32pad, d_a16, B, H, W, C, scale, (hipStream_t)stream);
}

int lseg_op_correlation(const float* feat, const void* text_f16, float* logits, int B, int P, int C, int K,
                        float logit_scale, void* stream) {
    int r = require_device(); if (r) return r;
    if (C % 64) return set_error(LSEG_ERR_UNSUPPORTED, "correlation: C=%d must be a multiple of 64", C);
    const size_t M = (size_t)B * P;
    uint16_t* a = nullptr;
    LSEG_HIP_TRY(hipMallocAsync((void**)&a, M * C * sizeof(uint16_t), (hipStream_t)stream));
    r = launch_l2norm_scale_f16(feat, a, (int)M, C, logit_scale, (hipStream_t)stream);
    if (!r) {
        GemmArgs g;
        gemm_args_init(g);
        if (P % 4 == 0) {      // the engine's orientation: labels = rows, pixels = columns (16-byte stores along the label planes)
            g.A = (const uint16_t*)text_f16; g.W = a; g.M = K; g.N = (int)M; g.K = C; g.lda = C; g.ldw = C;
            g.round_mid = 1; g.C = logits; g.out_dtype = DT_F32; g.map_mode = MAP_LABELPLANES; g.p_div = P;
        } else {
            g.A = a; g.W = (const uint16_t*)text_f16; g.M = (int)M; g.N = K; g.K = C; g.lda = C; g.ldw = C;
            g.round_mid = 1; g.C = logits; g.out_dtype = DT_F32; g.map_mode = MAP_NCHW; g.p_div = P;
        }
        r = launch_gemm(g, DT_F16, (hipStream_t)stream);
    }
    (void)hipFreeAsync(a, (hipStream_t)stream);
    return r;
}

int lseg_op_head_features(const void* x_bf16, const void* w_bf16, const float* bias, void* a_f16, int M, int F,
                          float logit_scale, void* stream) {
    int r = require_device(); if (r) return r;
    GemmArgs g;
    gemm_args_init(g);
    g.A = (const uint16_t*)x_bf16; g.W = (const uint16_t*)w_bf16; g.M = M; g.N = 512; g.K = F; g.lda = F; g.ldw = F;
    g.bias = bias; g.C = a_f16; g.out_dtype = DT_F16; g.ldc = 512; g.map_mode = MAP_ROWNORM; g.rn_scale = logit_scale;
    return launch_gemm(g, DT_BF16, (hipStream_t)stream);
}

int lseg_op_corr_argmax(const void* d_g16pad, const void* d_tnorm, const float* d_scale, int16_t* d_label, float* d_score, int B, int K, int H, int W,
                        int C, void* d_ws, size_t ws_bytes, void* stream) {
    return launch_corr_argmax(d_g16pad, d_tnorm, d_scale, CorrOut{d_label, d_score}, B, K, H, W, C, (hipStream_t)stream, d_ws, ws_bytes);
}
int lseg_op_corr_argmax_conf(const void* d_g16pad, const void* d_tnorm, const float* d_scale, int16_t* d_label, float* d_score, int16_t* d_label2,
                             float* d_score2, float* d_lse, int B, int K, int H, int W, int C, void* d_ws, size_t ws_bytes, void* stream) {
    return launch_corr_argmax(d_g16pad, d_tnorm, d_scale, CorrOut{d_label, d_score, d_label2, d_score2, d_lse}, B, K, H, W, C, (hipStream_t)stream,
                              d_ws, ws_bytes);
}

size_t lseg_op_episode_stats_ws_bytes(int B, int H, int W) { return episode_stats_ws_bytes(B, H, W); }
int lseg_op_episode_stats(const float* d_scores, const int64_t* d_target, const uint8_t* d_ignore, int B, int H, int W, int up,
                          int ignore_index, const int64_t* d_class_id, int nclass, int64_t* d_inter_buf, int64_t* d_union_buf,
                          int64_t* d_areas, double* d_nll, int64_t* d_flags, void* d_ws, size_t ws_bytes, void* stream) {
    int r = require_device();
    if (r) return r;
    return launch_episode_stats(d_scores, d_target, d_ignore, B, H, W, up, ignore_index, d_class_id, nclass, d_inter_buf, d_union_buf, d_areas,
                                d_nll, d_flags, d_ws, ws_bytes, (hipStream_t)stream);
}

// forward_route.h: the route table of Engine::forward for n requests (host only, no engine, no device)
int lseg_op_forward_route(const int32_t* in13, int n, int32_t* out6) {
    if (!in13 || !out6 || n < 1) return set_error(LSEG_ERR_INVALID, "forward_route: NULL pointer or n < 1");
    for (int i = 0; i < n; ++i, in13 += 13, out6 += 6) {
        RouteIn r;
        const int w = in13[0];
        r.logits = w & 1; r.argmax = w & 2; r.label = w & 4; r.score = w & 8; r.low = w & 16; r.runner_up = w & 32; r.lse = w & 64;
        r.held = w & 128; r.loss = w & 256; r.target = w & 512;
        r.K = in13[1]; r.group_k = in13[2]; r.ragged = in13[3]; r.arch_option = in13[4]; r.out_c = in13[5]; r.lw0 = in13[6];
        r.debug = in13[7]; r.strict = in13[8]; r.headc_packed = in13[9]; r.corr_full = in13[10]; r.corr_generic = in13[11]; r.no_4x = in13[12];
        const Route t = forward_route(r);
        out6[0] = refusal_status(forward_refusal(r));
        out6[1] = t.tail; out6[2] = t.planes; out6[3] = t.commuted; out6[4] = t.corr_low; out6[5] = t.corr_fused;
    }
    return LSEG_OK;
}

// train_head.h: the plan of the training step's label head for n configurations (host only, no engine, no device)
int lseg_op_train_head_plan(const int32_t* in11, int n, int32_t* out8) {
    if (!in11 || !out8 || n < 1) return set_error(LSEG_ERR_INVALID, "train_head_plan: NULL pointer or n < 1");
    for (int i = 0; i < n; ++i, in11 += 11, out8 += 8) {
        TrainHeadIn r;
        r.group_k = in11[0]; r.ragged = in11[1]; r.kmax = in11[2]; r.K = in11[3]; r.hb_n = in11[4]; r.arch_option = in11[5];
        r.unrounded = in11[6]; r.img_dt = in11[7]; r.out_c = in11[8]; r.logits = in11[9]; r.ragged_gemm = in11[10];
        const TrainHead p = train_head_plan(r);
        out8[0] = p.refusal == TRAIN_REFUSE_NONE ? 0 : LSEG_ERR_UNSUPPORTED;
        out8[1] = p.mode; out8[2] = p.kout; out8[3] = p.Kp; out8[4] = p.hdt; out8[5] = p.dgrad_operand; out8[6] = p.head_blocks;
        out8[7] = p.refusal;
    }
    return LSEG_OK;
}

// label_stats.hip: every check of these launchers comes before the device is touched (a refusal needs no device)
int lseg_op_label_stats_plan(int K_or_bins, int* out2) { return label_stats_plan(K_or_bins, out2); }
int lseg_op_label_stats(const int16_t* d_label, const int64_t* d_target, int B, int H, int W, int K, int ignore_index, const int32_t* d_offsets,
                        const int32_t* d_class_map, int nclass, int64_t* d_counts, int64_t* d_flags, int accumulate, void* stream) {
    return launch_label_stats(d_label, d_target, B, H, W, K, ignore_index, d_offsets, d_class_map, nclass, d_counts, d_flags, accumulate,
                              (hipStream_t)stream);
}
int lseg_op_stats_fold_lowres(const float* d_low, int B, int rows, int row0, int h, int w, const int64_t* d_target, int16_t* d_label,
                              float* d_best, float* d_sum, float* d_tlogit, int first, void* stream) {
    return launch_stats_fold_lowres(d_low, B, rows, row0, h, w, d_target, d_label, d_best, d_sum, d_tlogit, first, (hipStream_t)stream);
}
size_t lseg_op_stats_finish_ws_bytes(int B, int H, int W) { return stats_finish_ws_bytes(B, H, W); }
int lseg_op_stats_finish(const int16_t* d_label, const float* d_best, const float* d_sum, const float* d_tlogit, const int64_t* d_target, int B,
                         int H, int W, int K, int ignore_index, int64_t* d_counts, double* d_nll, int64_t* d_flags, void* d_ws, size_t ws_bytes,
                         void* stream) {
    return launch_stats_finish(d_label, d_best, d_sum, d_tlogit, d_target, B, H, W, K, ignore_index, d_counts, d_nll, d_flags, d_ws, ws_bytes,
                               (hipStream_t)stream);
}

int lseg_op_corr_argmax_ragged(const void* d_g16pad, const void* d_text16, const float* d_scale, const int32_t* host_counts, int32_t* d_offsets,
                               int16_t* d_label, float* d_score, int16_t* d_label2, float* d_score2, float* d_lse, int B, int H, int W, int C,
                               void* d_ws, size_t ws_bytes, void* stream) {
    if (!host_counts) return set_error(LSEG_ERR_INVALID, "corr_argmax_ragged: NULL pointer");       // (the entry would take one shared set)
    return launch_corr_argmax(d_g16pad, d_text16, d_scale, CorrOut{d_label, d_score, d_label2, d_score2, d_lse}, B, 0, H, W, C, (hipStream_t)stream,
                              d_ws, ws_bytes, nullptr, host_counts, d_offsets);
}
int lseg_op_corr_argmax_ragged_split(const int32_t* host_counts, int B, int H, int W, int conf, size_t ws_bytes, int cus, int* out2) {
    return corr_argmax_ragged_split(host_counts, B, H, W, conf, ws_bytes, cus, out2);
}
int lseg_op_corr_argmax_geometry(int* out8) {
    if (!out8) return set_error(LSEG_ERR_INVALID, "corr_argmax_geometry: NULL pointer");
    corr_argmax_geometry(out8);
    return LSEG_OK;
}
int lseg_op_corr_argmax_loss(const void* d_g16pad, const void* d_text16, const float* d_scale, const int64_t* d_target, int ignore_index,
                             const int32_t* host_counts, int B, int K, int H, int W, int C, int16_t* d_label, float* d_score, float* d_lse,
                             float* d_tlogit, float* d_nll_plane, double* d_nll, void* d_ws, size_t ws_bytes, void* stream) {
    return corr_argmax_loss_op(d_g16pad, d_text16, d_scale, d_target, ignore_index, host_counts, B, K, H, W, C, d_label, d_score, d_lse, d_tlogit,
                               d_nll_plane, d_nll, d_ws, ws_bytes, (hipStream_t)stream);
}
size_t lseg_op_corr_argmax_loss_ws_bytes(int B, int H, int W, int ragged, int want_nll, int temp_planes, int parts) {
    return corr_argmax_loss_ws_bytes(B, H, W, ragged, want_nll, temp_planes, parts);
}
int lseg_op_corr_argmax_loss_plan(int B, int H, int W, int64_t* out4) {
    if (!out4 || B < 1 || H < 1 || W < 1) return set_error(LSEG_ERR_INVALID, "corr_argmax_loss_plan: B=%d H=%d W=%d out4=%p", B, H, W, (void*)out4);
    corr_loss_plan((size_t)B * 16 * H * W, out4);
    return LSEG_OK;
}

int lseg_op_seg_stats(const float* d_scores, const int64_t* d_target, int B, int K, int H, int W, int ignore_index,
                      int64_t* d_counts, double* d_nll, void* stream) {
    int r = require_device(); if (r) return r;
    if (!d_scores || !d_target || !d_counts || !d_nll) return set_error(LSEG_ERR_INVALID, "seg_stats: NULL pointer");
    if (B < 1 || K < 1 || K > 4096 || H < 1 || W < 1) return set_error(LSEG_ERR_INVALID, "seg_stats: bad shape B=%d K=%d %dx%d", B, K, H, W);
    return launch_seg_stats(d_scores, d_target, B, K, H * W, ignore_index, reinterpret_cast<unsigned long long*>(d_counts),
                            d_nll, (hipStream_t)stream);
}

int lseg_op_seg_stats_lowres(const float* d_low, const int64_t* d_target, int B, int K, int h, int w, int ignore_index,
                             int64_t* d_counts, double* d_nll, uint8_t* d_argmax, void* stream) {
    int r = require_device(); if (r) return r;
    if (!d_low || (!d_target && !d_argmax) || (d_target && (!d_counts || !d_nll))) return set_error(LSEG_ERR_INVALID, "seg_stats_lowres: NULL pointer");
    if (B < 1 || K < 1 || h < 2 || w < 2) return set_error(LSEG_ERR_INVALID, "seg_stats_lowres: bad shape");
    return launch_seg_stats_ex(d_low, d_target, B, K, 4 * h * w, ignore_index, reinterpret_cast<unsigned long long*>(d_counts), d_nll,
                               d_argmax, 1, h, w, (hipStream_t)stream);
}

int lseg_op_corr_planes(const void* d_g16pad, const void* d_text16, float* d_planes, float* d_gram, int B, int K, int H, int W, int C,
                        void* stream) {
    int r = require_device(); if (r) return r;
    if (!d_g16pad || !d_text16 || !d_planes) return set_error(LSEG_ERR_INVALID, "corr_planes: NULL pointer");
    return launch_corr_planes(d_g16pad, d_text16, d_planes, d_gram, B, K, H, W, C, (hipStream_t)stream);
}

int lseg_op_upsample_ce_backward_rows(const float* d_low, const int64_t* d_target, int B, int K, int h, int w, int ignore_index,
                                      double* d_nll, float* d_lse_ws, void* d_rows, int ldk, int out_dtype, void* stream) {
    int r = require_device(); if (r) return r;
    if (!d_low || !d_target || !d_nll || !d_lse_ws || !d_rows) return set_error(LSEG_ERR_INVALID, "upsample_ce_backward_rows: NULL pointer");
    if (B < 1 || K < 1 || h < 2 || w < 2) return set_error(LSEG_ERR_INVALID, "upsample_ce_backward_rows: bad shape");
    int dt;
    if (out_dtype == LSEG_BF16) dt = DT_BF16; else if (out_dtype == LSEG_F16) dt = DT_F16;
    else return set_error(LSEG_ERR_INVALID, "upsample_ce_backward_rows: out_dtype %d", out_dtype);
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* counts = nullptr;
    LSEG_HIP_TRY(hipMallocAsync((void**)&counts, (size_t)(2 + 3 * K) * sizeof(unsigned long long), st));
    r = launch_seg_stats_ex(d_low, d_target, B, K, 4 * h * w, ignore_index, counts, d_nll, nullptr, 1, h, w, st, d_lse_ws);
    if (!r) r = launch_upsample_ce_backward_rows(d_low, d_target, d_lse_ws, d_nll, d_rows, B, K, h, w, ldk, ignore_index, dt, st);
    (void)hipFreeAsync(counts, st);
    return r;
}

// ragged per-image label sets on the training path (ragged_train.hip)
int lseg_op_ragged_ce_plan(const int32_t* host_counts, int B, int h, int w, int* out8) { return ragged_ce_plan(host_counts, B, h, w, out8); }
static int ragged_op_prefix(const char* what, const int32_t* host_counts, int B, int* d_prefix, int ldk, hipStream_t st) {
    if (B < 1 || B > 65535) return set_error(LSEG_ERR_INVALID, "%s: B=%d", what, B);
    std::vector<int> prefix((size_t)B + 1, 0);
    int kmax = 0;
    int r = ragged_prefix(host_counts, B, prefix.data(), kmax);
    if (r) return r;
    if (ldk && ldk < kmax) return set_error(LSEG_ERR_INVALID, "%s: ldk=%d < the largest count %d", what, ldk, kmax);
    return launch_ragged_offsets(d_prefix, prefix.data(), B + 1, st);
}
int lseg_op_ragged_ce_fwd(const float* d_low, const int64_t* d_target, const int32_t* host_counts, int* d_prefix, int B, int h, int w,
                          int ignore_index, double* d_nll, int64_t* d_counts2, float* d_lse, void* stream) {
    if (!d_low || !d_target || !host_counts || !d_prefix || !d_nll || !d_counts2 || !d_lse) return set_error(LSEG_ERR_INVALID, "ragged_ce_fwd: NULL pointer");
    if (h < 2 || w < 2) return set_error(LSEG_ERR_INVALID, "ragged_ce_fwd: bad shape");
    int r = require_device(); if (r) return r;
    hipStream_t st = (hipStream_t)stream;
    r = ragged_op_prefix("ragged_ce_fwd", host_counts, B, d_prefix, 0, st);
    if (r) return r;
    return launch_ragged_ce_fwd(d_low, d_target, d_prefix, B, h, w, ignore_index, reinterpret_cast<unsigned long long*>(d_counts2), d_nll, d_lse, st);
}
int lseg_op_ragged_ce_bwd_rows(const float* d_low, const int64_t* d_target, const int32_t* host_counts, int* d_prefix, int B, int h, int w,
                               int ignore_index, double* d_nll, float* d_lse_ws, void* d_rows, int ldk, int out_dtype,
                               const float* d_grad_scale, void* stream) {
    if (!d_low || !d_target || !host_counts || !d_prefix || !d_nll || !d_lse_ws || !d_rows) return set_error(LSEG_ERR_INVALID, "ragged_ce_bwd_rows: NULL pointer");
    if (h < 2 || w < 2) return set_error(LSEG_ERR_INVALID, "ragged_ce_bwd_rows: bad shape");
    int dt;
    if (out_dtype == LSEG_BF16) dt = DT_BF16; else if (out_dtype == LSEG_F16) dt = DT_F16;
    else return set_error(LSEG_ERR_INVALID, "ragged_ce_bwd_rows: out_dtype %d", out_dtype);
    if (ldk < 8 || (ldk & 7)) return set_error(LSEG_ERR_INVALID, "ragged_ce_bwd_rows: ldk=%d must be a multiple of 8", ldk);
    int r = require_device(); if (r) return r;
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* counts = nullptr;
    LSEG_HIP_TRY(hipMallocAsync((void**)&counts, 2 * sizeof(unsigned long long), st));      // (before anything is launched)
    r = ragged_op_prefix("ragged_ce_bwd_rows", host_counts, B, d_prefix, ldk, st);
    if (!r) r = launch_ragged_ce_fwd(d_low, d_target, d_prefix, B, h, w, ignore_index, counts, d_nll, d_lse_ws, st);
    if (!r) r = launch_ragged_ce_bwd_rows(d_low, d_target, d_lse_ws, d_nll, d_rows, d_prefix, B, h, w, ldk, ignore_index, dt, st, d_grad_scale);
    (void)hipFreeAsync(counts, st);
    return r;
}

int lseg_op_corr_ragged_plan(const int32_t* host_counts, int B, int hw, int C, int* out8) { return corr_ragged_plan(host_counts, B, hw, C, out8); }
// stage: 0 = what the engine takes (stage two unless LSEG_CORR_RAGGED_GEMM is set), 1 = the per-image GEMMs, 2 = the one-launch kernels
static int ragged_stage(int stage, int* out) {
    if (stage < 0 || stage > 2) return set_error(LSEG_ERR_INVALID, "ragged correlation: stage %d (0 engine's, 1 per-image GEMM, 2 one launch)", stage);
    *out = stage ? stage : (corr_ragged_use_gemm() ? 1 : 2);
    return 0;
}
int lseg_op_corr_ragged_fwd(const void* d_a16, const void* d_tnorm, float* d_low, const int32_t* host_counts, int B, int hw, int C, int stage,
                            void* stream) {
    if (!d_a16 || !d_tnorm || !d_low) return set_error(LSEG_ERR_INVALID, "corr_ragged_fwd: NULL pointer");
    int plan[8], sg;
    int r = corr_ragged_plan(host_counts, B, hw, C, plan); if (r) return r;
    if ((r = ragged_stage(stage, &sg))) return r;
    r = require_device(); if (r) return r;
    hipStream_t st = (hipStream_t)stream;
    std::vector<int> prefix((size_t)B + 1, 0);
    int kmax = 0;
    if ((r = ragged_prefix(host_counts, B, prefix.data(), kmax))) return r;
    if (sg == 1) return launch_corr_ragged_fwd(d_a16, d_tnorm, d_low, prefix.data(), B, hw, C, st);
    int* dp = nullptr;
    LSEG_HIP_TRY(hipMallocAsync((void**)&dp, ((size_t)B + 1) * sizeof(int), st));
    r = launch_ragged_offsets(dp, prefix.data(), B + 1, st);
    if (!r) r = launch_corr_ragged_fwd_fused(d_a16, d_tnorm, d_low, dp, B, hw, C, st);
    (void)hipFreeAsync(dp, st);
    return r;
}
int lseg_op_corr_ragged_bwd(const void* d_rows, int rows_dtype, int ldk, const void* d_tnorm, const float* d_feat, void* d_df, int df_dtype,
                            const int32_t* host_counts, int B, int hw, int C, float scale, int stage, void* stream) {
    if (!d_rows || !d_tnorm || !d_feat || !d_df) return set_error(LSEG_ERR_INVALID, "corr_ragged_bwd: NULL pointer");
    int plan[8], rd, dd, sg;
    int r = corr_ragged_plan(host_counts, B, hw, C, plan); if (r) return r;
    if ((r = op_dt(rows_dtype, &rd)) || (r = op_dt(df_dtype, &dd))) return r;
    if ((r = ragged_stage(stage, &sg))) return r;
    if (rd == DT_F32 || dd == DT_F32) return set_error(LSEG_ERR_INVALID, "corr_ragged_bwd: 16-bit rows and df");
    if (ldk < plan[3] || ldk % 64 != 0) return set_error(LSEG_ERR_INVALID, "corr_ragged_bwd: ldk=%d must be a multiple of 64 and >= %d", ldk, plan[3]);
    r = require_device(); if (r) return r;
    hipStream_t st = (hipStream_t)stream;
    std::vector<int> prefix((size_t)B + 1, 0);
    int kmax = 0;
    if ((r = ragged_prefix(host_counts, B, prefix.data(), kmax))) return r;
    if (sg == 2) {
        int* dp = nullptr;
        LSEG_HIP_TRY(hipMallocAsync((void**)&dp, ((size_t)B + 1) * sizeof(int), st));
        r = launch_ragged_offsets(dp, prefix.data(), B + 1, st);
        if (!r) r = launch_corr_ragged_bwd_fused(d_rows, rd, ldk, d_tnorm, d_feat, d_df, dd, dp, kmax, B, hw, C, scale, st);
        (void)hipFreeAsync(dp, st);
        return r;
    }
    // stage one; scratch on the stream: the bf16 rounding of the text rows (bf16 rows only), the transposed panels, dA, a bias of zeros
    const size_t n_t = (size_t)plan[4] * C, n_p = (size_t)plan[2] * C, n_da = (size_t)plan[5];
    char* ws = nullptr;
    const size_t bytes = (n_t + n_p + n_da) * 2 + (size_t)C * sizeof(float);
    LSEG_HIP_TRY(hipMallocAsync((void**)&ws, bytes, st));
    uint16_t *t16 = (uint16_t*)ws, *pan = t16 + n_t, *da = pan + n_p;
    float* zb = (float*)(da + n_da);
    r = hipMemsetAsync(zb, 0, (size_t)C * sizeof(float), st) == hipSuccess ? 0 : set_error(LSEG_ERR_HIP, "corr_ragged_bwd: memset");
    const void* tsrc = d_tnorm;
    if (!r && rd == DT_BF16) { r = launch_convert(d_tnorm, DT_F16, t16, DT_BF16, n_t, st); tsrc = t16; }
    if (!r) r = launch_corr_ragged_panels(tsrc, pan, prefix.data(), B, C, st);
    if (!r) r = launch_corr_ragged_bwd(d_rows, rd, ldk, pan, zb, d_feat, da, d_df, dd, prefix.data(), B, hw, C, scale, st);
    (void)hipFreeAsync(ws, st);
    return r;
}

int lseg_op_eval_make_crops(const float* d_img, float* d_crops, int C, int height, int width, int crop, int stride, int h_grids, int w_grids,
                            int flip, const float* host_pad3, void* stream) {
    int r = require_device(); if (r) return r;
    if (!d_img || !d_crops || !host_pad3) return set_error(LSEG_ERR_INVALID, "eval_make_crops: NULL pointer");
    if (C < 1 || C > 3 || height < 1 || width < 1 || crop < 1 || stride < 1 || h_grids < 1 || w_grids < 1)
        return set_error(LSEG_ERR_INVALID, "eval_make_crops: bad geometry");
    return launch_eval_make_crops(d_img, d_crops, C, height, width, crop, stride, h_grids, w_grids, flip ? 1 : 0, host_pad3, (hipStream_t)stream);
}
int lseg_op_eval_make_crops_u8(const uint8_t* d_img, float* d_crops, int src_h, int src_w, int height, int width, int crop, int stride, int h_grids,
                               int w_grids, int flip, const float* host_pad3, const float* host_mean3, const float* host_std3, void* stream) {
    NormU8 n;
    int r = norm_u8_check("eval_make_crops_u8", host_mean3, host_std3, &n);
    if (r) return r;
    if (!d_img || !d_crops || !host_pad3) return set_error(LSEG_ERR_INVALID, "eval_make_crops_u8: NULL pointer");
    if (src_h < 1 || src_w < 1 || height < 1 || width < 1 || crop < 1 || stride < 1 || h_grids < 1 || w_grids < 1 ||
        (long long)h_grids * w_grids > 0x3fffffff)
        return set_error(LSEG_ERR_INVALID, "eval_make_crops_u8: bad geometry");
    if ((uintptr_t)d_crops & 3) return set_error(LSEG_ERR_INVALID, "eval_make_crops_u8: the crops must be 4-byte aligned");
    if ((r = require_device())) return r;
    return launch_eval_make_crops_u8(d_img, d_crops, src_h, src_w, height, width, crop, stride, h_grids, w_grids, flip ? 1 : 0, host_pad3, n,
                                     (hipStream_t)stream);
}
// the geometry contract of the accumulate and finalize entries, checked before the device is touched: a [K, height, width] map inside the
// padded (ph, pw) image that the h_grids x w_grids boxes cover; lowres: the logits are crop/2 x crop/2 planes
static int eval_geometry_check(const char* what, const void* d_a, const void* d_b, int K, int height, int width, int ph, int pw, int crop, int stride,
                               int h_grids, int w_grids, int lowres) {
    if (!d_a || !d_b) return set_error(LSEG_ERR_INVALID, "%s: NULL pointer", what);
    if (lowres && (crop < 4 || (crop & 1)))
        return set_error(LSEG_ERR_INVALID, "%s: crop=%d must be even and >= 4 (the planes are crop/2 x crop/2)", what, crop);
    if (K < 1 || height < 1 || width < 1 || height > ph || width > pw || crop < 1 || stride < 1 || h_grids < 1 || w_grids < 1 ||
        (long long)h_grids * w_grids > 0x3fffffff || (long long)(h_grids - 1) * stride + crop < ph || (long long)(w_grids - 1) * stride + crop < pw)
        return set_error(LSEG_ERR_INVALID, "%s: the boxes do not cover the %dx%d map", what, ph, pw);
    if (((uintptr_t)d_a | (uintptr_t)d_b) & 3) return set_error(LSEG_ERR_INVALID, "%s: pointers must be 4-byte aligned", what);
    return 0;
}
int lseg_op_eval_accumulate(const float* d_outs, float* d_map, int K, int height, int width, int ph, int pw, int crop, int stride,
                            int h_grids, int w_grids, int flip, void* stream) {
    int r = eval_geometry_check("eval_accumulate", d_outs, d_map, K, height, width, ph, pw, crop, stride, h_grids, w_grids, 0);
    if (r) return r;
    r = require_device(); if (r) return r;
    return launch_eval_accumulate(d_outs, d_map, K, height, width, ph, pw, crop, stride, h_grids, w_grids, flip ? 1 : 0, (hipStream_t)stream);
}
int lseg_op_eval_accumulate_lowres(const float* d_low, float* d_map, int K, int height, int width, int ph, int pw, int crop, int stride,
                                   int h_grids, int w_grids, int flip, void* stream) {
    int r = eval_geometry_check("eval_accumulate_lowres", d_low, d_map, K, height, width, ph, pw, crop, stride, h_grids, w_grids, 1);
    if (r) return r;
    r = require_device(); if (r) return r;
    return launch_eval_accumulate_lowres(d_low, d_map, K, height, width, crop, stride, h_grids, w_grids, flip ? 1 : 0, (hipStream_t)stream);
}
static int eval_accumulate_window(const char* what, const float* d_outs, float* d_sum, int K, int height, int width, int ph, int pw, int crop,
                                  int stride, int h_grids, int w_grids, int flip, int first_box, int n_box, int lowres, void* stream) {
    int r = eval_geometry_check(what, d_outs, d_sum, K, height, width, ph, pw, crop, stride, h_grids, w_grids, lowres);
    if (r) return r;
    if (n_box < 1 || first_box < 0 || (long long)first_box + n_box > (long long)h_grids * w_grids)
        return set_error(LSEG_ERR_INVALID, "%s: boxes [%d, %d + %d) are not a window of the %dx%d grid", what, first_box, first_box, n_box, h_grids,
                         w_grids);
    r = require_device(); if (r) return r;
    return launch_eval_accumulate_window(d_outs, d_sum, K, height, width, crop, stride, w_grids, flip ? 1 : 0, first_box, n_box, lowres,
                                         (hipStream_t)stream);
}
int lseg_op_eval_accumulate_window(const float* d_outs, float* d_sum, int K, int height, int width, int ph, int pw, int crop, int stride,
                                   int h_grids, int w_grids, int flip, int first_box, int n_box, void* stream) {
    return eval_accumulate_window("eval_accumulate_window", d_outs, d_sum, K, height, width, ph, pw, crop, stride, h_grids, w_grids, flip,
                                  first_box, n_box, 0, stream);
}
int lseg_op_eval_accumulate_window_lowres(const float* d_low, float* d_sum, int K, int height, int width, int ph, int pw, int crop, int stride,
                                          int h_grids, int w_grids, int flip, int first_box, int n_box, void* stream) {
    return eval_accumulate_window("eval_accumulate_window_lowres", d_low, d_sum, K, height, width, ph, pw, crop, stride, h_grids, w_grids, flip,
                                  first_box, n_box, 1, stream);
}
int lseg_op_eval_finalize(const float* d_sum, float* d_map, int K, int height, int width, int ph, int pw, int crop, int stride, int h_grids,
                          int w_grids, void* stream) {
    int r = eval_geometry_check("eval_finalize", d_sum, d_map, K, height, width, ph, pw, crop, stride, h_grids, w_grids, 0);
    if (r) return r;
    r = require_device(); if (r) return r;
    return launch_eval_finalize(d_sum, d_map, K, height, width, crop, stride, h_grids, w_grids, (hipStream_t)stream);
}
int lseg_op_eval_merge_labels(const float* d_scores, int rows, int row0, int H, int W, int16_t* d_label, float* d_score, int16_t* d_label2,
                              float* d_score2, float* d_sum, int first, int last, void* stream) {
    if (!d_scores || !d_label || !d_score) return set_error(LSEG_ERR_INVALID, "eval_merge_labels: NULL pointer (scores, label and score are required)");
    if (rows < 1 || row0 < 0 || H < 1 || W < 1) return set_error(LSEG_ERR_INVALID, "eval_merge_labels: bad shape");
    if ((long long)row0 + rows > 32767) return set_error(LSEG_ERR_UNSUPPORTED, "eval_merge_labels: int16 labels need row0 + rows <= 32767 (%d + %d)", row0, rows);
    if (d_label2 && !d_score2) return set_error(LSEG_ERR_INVALID, "eval_merge_labels: the runner-up label needs the runner-up score (its running state)");
    if ((((uintptr_t)d_scores | (uintptr_t)d_score | (uintptr_t)d_score2 | (uintptr_t)d_sum) & 3) || (((uintptr_t)d_label | (uintptr_t)d_label2) & 1))
        return set_error(LSEG_ERR_INVALID, "eval_merge_labels: pointers must be aligned to their element");
    int r = require_device(); if (r) return r;
    return launch_eval_merge_labels(d_scores, rows, row0, H, W, d_label, d_score, d_label2, d_score2, d_sum, first ? 1 : 0, last ? 1 : 0,
                                    (hipStream_t)stream);
}
int lseg_op_eval_resize(const float* d_src, float* d_dst, int P, int Hi, int Wi, int Ho, int Wo, int accumulate, void* stream) {
    int r = require_device(); if (r) return r;
    if (!d_src || !d_dst) return set_error(LSEG_ERR_INVALID, "eval_resize: NULL pointer");
    if (P < 1 || Hi < 1 || Wi < 1 || Ho < 1 || Wo < 1) return set_error(LSEG_ERR_INVALID, "eval_resize: bad shape");
    return launch_eval_resize(d_src, d_dst, P, Hi, Wi, Ho, Wo, accumulate ? 1 : 0, (hipStream_t)stream);
}

int lseg_op_linear_backward(const void* d_dy, const void* d_x, const void* d_w, int ab_dtype, void* d_dx, float* d_dw,
                            float* d_db, int M, int N, int K, void* stream) {
    int r = require_device(); if (r) return r;
    int ab;
    if ((r = op_dt(ab_dtype, &ab))) return r;
    if (ab != DT_BF16 && ab != DT_F16) return set_error(LSEG_ERR_INVALID, "linear_backward: operands must be bf16 or fp16");
    if (!d_dy || !d_x || !d_w) return set_error(LSEG_ERR_INVALID, "linear_backward: NULL operand");
    if (M < 1 || (N % 64) || (K % 64) || N < 64 || K < 64)
        return set_error(LSEG_ERR_UNSUPPORTED, "linear_backward: N=%d and K=%d must be multiples of 64 (M=%d >= 1)", N, K, M);
    hipStream_t st = (hipStream_t)stream;
    const int Mp = (M + 63) / 64 * 64;                    // wgrad contracts over M: pad to the GEMM's K-step with zeros
    uint16_t *wt = nullptr, *dyt = nullptr, *xt = nullptr;
    auto cleanup = [&]() { if (wt) (void)hipFreeAsync(wt, st); if (dyt) (void)hipFreeAsync(dyt, st); if (xt) (void)hipFreeAsync(xt, st); };
    GemmArgs g;
    if (d_dx) {     // dX[M,K] = dY[M,N] . W[N,K]      (A = dY, "weights" = W^T [K,N], contraction over N)
        if (hipMallocAsync((void**)&wt, (size_t)K * N * 2, st) != hipSuccess) { cleanup(); return set_error(LSEG_ERR_HIP, "linear_backward: out of device memory"); }
        if ((r = launch_transpose16(d_w, wt, N, K, K, N, st))) { cleanup(); return r; }
        gemm_args_init(g);
        g.A = (const uint16_t*)d_dy; g.W = wt; g.M = M; g.N = K; g.K = N; g.lda = N; g.ldw = N;
        g.C = d_dx; g.out_dtype = ab; g.ldc = K; g.map_mode = MAP_LINEAR;
        if ((r = launch_gemm(g, ab, st))) { cleanup(); return r; }
    }
    float* wsk = nullptr;
    if (d_dw && wgrad_kmajor_ok(N, K, (size_t)16 * N * K)) {     // the operands as they are (K-major path: no transposed copies)
        if (hipMallocAsync((void**)&wsk, (size_t)16 * N * K * sizeof(float), st) != hipSuccess) { cleanup(); return set_error(LSEG_ERR_HIP, "linear_backward: out of device memory"); }
        r = launch_wgrad_kmajor(d_dy, N, d_x, K, M, N, K, d_dw, 0, wsk, (size_t)16 * N * K, ab, st);
        (void)hipFreeAsync(wsk, st);
        if (r) { cleanup(); return r; }
    } else if (d_dw) {     // dW[N,K] = dY^T[N,M] . X[M,K]    (A = dY^T [N,Mp], "weights" = X^T [K,Mp], contraction over M)
        if (hipMallocAsync((void**)&dyt, (size_t)N * Mp * 2, st) != hipSuccess ||
            hipMallocAsync((void**)&xt, (size_t)K * Mp * 2, st) != hipSuccess) { cleanup(); return set_error(LSEG_ERR_HIP, "linear_backward: out of device memory"); }
        if ((r = launch_transpose16(d_dy, dyt, M, N, N, Mp, st)) || (r = launch_transpose16(d_x, xt, M, K, K, Mp, st))) { cleanup(); return r; }
        gemm_args_init(g);
        g.A = dyt; g.W = xt; g.M = N; g.N = K; g.K = Mp; g.lda = Mp; g.ldw = Mp;
        g.C = d_dw; g.out_dtype = DT_F32; g.ldc = K; g.map_mode = MAP_LINEAR;
        if ((r = launch_gemm(g, ab, st))) { cleanup(); return r; }
    }
    if (d_db && (r = launch_colsum16(d_dy, ab, d_db, M, N, N, st))) { cleanup(); return r; }
    cleanup();
    return LSEG_OK;
}

int lseg_op_layernorm_backward(const void* d_dy, int dy_dtype, const float* d_x, const float* d_gamma, float* d_dx,
                               float* d_dgamma, float* d_dbeta, int M, int D, float eps, int accumulate_dx, void* stream) {
    int r = require_device(); if (r) return r;
    int dt;
    if ((r = op_dt(dy_dtype, &dt))) return r;
    if (!d_dy || !d_x || !d_gamma || !d_dx || !d_dgamma || !d_dbeta) return set_error(LSEG_ERR_INVALID, "layernorm_backward: NULL pointer");
    if (M < 1) return set_error(LSEG_ERR_INVALID, "layernorm_backward: M=%d", M);
    return launch_layernorm_backward(d_dy, dt, d_x, d_gamma, d_dx, d_dgamma, d_dbeta, M, D, eps, accumulate_dx, (hipStream_t)stream);
}

int lseg_op_conv3x3_backward(const void* d_dy_pad, const void* d_x_pad, const void* d_w_packed, void* d_dx_pad, float* d_dw,
                             int B, int H, int W, int Cin, int Cout, void* stream) {
    int r = require_device(); if (r) return r;
    if (!d_dy_pad || !d_w_packed) return set_error(LSEG_ERR_INVALID, "conv3x3_backward: NULL operand");
    if ((Cin % 64) || (Cout % 64)) return set_error(LSEG_ERR_UNSUPPORTED, "conv3x3_backward: Cin=%d, Cout=%d must be multiples of 64", Cin, Cout);
    hipStream_t st = (hipStream_t)stream;
    uint16_t *wd = nullptr, *dyt = nullptr, *xt9 = nullptr;
    auto cleanup = [&]() { if (wd) (void)hipFreeAsync(wd, st); if (dyt) (void)hipFreeAsync(dyt, st); if (xt9) (void)hipFreeAsync(xt9, st); };
    auto fail = [&](int code) { cleanup(); return code; };
    if (d_dx_pad) {
        // dX = conv3x3(dY, W flipped and channel-swapped): the forward implicit-GEMM kernel, roles of Cin / Cout exchanged
        if (hipMallocAsync((void**)&wd, (size_t)Cin * 9 * Cout * 2, st) != hipSuccess) return fail(set_error(LSEG_ERR_HIP, "conv3x3_backward: out of device memory"));
        if ((r = launch_conv_dgrad_pack(d_w_packed, wd, Cout, Cin, st))) return fail(r);
        if ((r = lseg_op_conv3x3(d_dy_pad, wd, nullptr, nullptr, d_dx_pad, B, H, W, Cout, Cin, 1, 0, 0, stream))) return fail(r);
    }
    if (d_dw) {
        // dW[co, tap, ci] = sum over padded positions m of dY[m, co] * X[m + shift(tap), ci]; dY's zero border removes the
        // positions whose shifted partner falls outside the image.  One GEMM: dY^T [Co, Mp] x (9 shifted X^T) [9*Ci, Mp]^T.
        if (!d_x_pad) return fail(set_error(LSEG_ERR_INVALID, "conv3x3_backward: wgrad needs the forward input"));
        const int Mp = B * (H + 2) * (W + 2), Mpp = (Mp + 63) / 64 * 64;
        const size_t wsn = (size_t)16 * Cout * 9 * Cin;
        if ((Cin % 128) == 0 && wgrad_kmajor_ok(Cout, 9 * Cin, wsn)) {      // the maps as they are (K-major operands, tap shifts in the loader)
            float* wsk = nullptr;
            int ns = 1;
            if (hipMallocAsync((void**)&wsk, wsn * sizeof(float), st) != hipSuccess) return fail(set_error(LSEG_ERR_HIP, "conv3x3_backward: out of device memory"));
            r = launch_conv_wgrad_kmajor(d_dy_pad, d_x_pad, 0, B, H, W, Cin, Cout, wsk, wsn, DT_BF16, &ns, st);
            if (!r) r = launch_sum_partials(wsk, d_dw, ns, (size_t)Cout * 9 * Cin, (size_t)Cout * 9 * Cin, 0, st);
            (void)hipFreeAsync(wsk, st);
            cleanup();
            return r;
        }
        if (hipMallocAsync((void**)&dyt, (size_t)Cout * Mpp * 2, st) != hipSuccess ||
            hipMallocAsync((void**)&xt9, (size_t)9 * Cin * Mpp * 2, st) != hipSuccess) return fail(set_error(LSEG_ERR_HIP, "conv3x3_backward: out of device memory"));
        if ((r = launch_transpose16(d_dy_pad, dyt, Mp, Cout, Cout, Mpp, st))) return fail(r);
        for (int t = 0; t < 9; ++t) {
            const int shift = (t / 3 - 1) * (W + 2) + (t % 3 - 1);
            if ((r = launch_transpose16(d_x_pad, xt9 + (size_t)t * Cin * Mpp, Mp, Cin, Cin, Mpp, st, shift))) return fail(r);
        }
        GemmArgs g;
        gemm_args_init(g);
        g.A = dyt; g.W = xt9; g.M = Cout; g.N = 9 * Cin; g.K = Mpp; g.lda = Mpp; g.ldw = Mpp;
        g.C = d_dw; g.out_dtype = DT_F32; g.ldc = 9 * Cin; g.map_mode = MAP_LINEAR;
        if ((r = launch_gemm(g, DT_BF16, st))) return fail(r);
    }
    cleanup();
    return LSEG_OK;
}

int lseg_op_quickgelu_backward(const void* d_dy, const void* d_pre, void* d_dx, int64_t n, int dtype, void* stream) {
    int r = require_device(); if (r) return r;
    int dt;
    if ((r = op_dt(dtype, &dt))) return r;
    if (dt == DT_F32 || !d_dy || !d_pre || !d_dx || n < 1) return set_error(LSEG_ERR_INVALID, "quickgelu_backward: bf16/fp16 tensors, n >= 1");
    return launch_gelu_backward(d_dy, d_pre, d_dx, (size_t)n, dt, (hipStream_t)stream, 1);
}

int lseg_op_gelu_backward(const void* d_dy, const void* d_pre, void* d_dx, int64_t n, int dtype, void* stream) {
    int r = require_device(); if (r) return r;
    int dt;
    if ((r = op_dt(dtype, &dt))) return r;
    if (dt == DT_F32 || !d_dy || !d_pre || !d_dx || n < 1) return set_error(LSEG_ERR_INVALID, "gelu_backward: bf16/fp16 tensors, n >= 1");
    return launch_gelu_backward(d_dy, d_pre, d_dx, (size_t)n, dt, (hipStream_t)stream);
}

int lseg_op_upsample2x_nhwc_backward(const void* d_dout, void* d_din_pad, int B, int H, int W, int C, void* stream) {
    int r = require_device(); if (r) return r;
    if (!d_dout || !d_din_pad || B < 1 || H < 2 || W < 2) return set_error(LSEG_ERR_INVALID, "upsample2x_nhwc_backward: bad arguments");
    return launch_upsample2x_nhwc_backward(d_dout, d_din_pad, B, H, W, C, DT_BF16, (hipStream_t)stream);
}

int lseg_op_softmax_ce_backward(const float* d_scores, const int64_t* d_target, float* d_dscores, int B, int K, int H, int W,
                                int ignore_index, const double* d_nll, void* stream) {
    int r = require_device(); if (r) return r;
    if (!d_scores || !d_target || !d_dscores || !d_nll || B < 1 || K < 1) return set_error(LSEG_ERR_INVALID, "softmax_ce_backward: bad arguments");
    return launch_softmax_ce_backward(d_scores, d_target, d_dscores, B, K, H * W, ignore_index, d_nll, (hipStream_t)stream);
}

size_t lseg_op_attention_backward_ws_bytes(int B, int H, int Npad) { return attention_backward_ws_bytes(B, H, Npad); }

int lseg_op_attention_backward_qkv(const void* d_q, const void* d_k, const void* d_vt, const void* d_o, const void* d_do,
                                   const float* d_lse2, void* d_dqkv, void* d_ws, int B, int H, int Ntok, int Npad, int dtype,
                                   float scale, void* stream) {
    int r = require_device(); if (r) return r;
    int dt;
    if ((r = op_dt(dtype, &dt))) return r;
    if (!d_q || !d_k || !d_vt || !d_o || !d_do || !d_lse2 || !d_dqkv) return set_error(LSEG_ERR_INVALID, "attention_backward_qkv: NULL pointer");
    if (B < 1 || H < 1 || Ntok < 1) return set_error(LSEG_ERR_INVALID, "attention_backward_qkv: bad shape");
    hipStream_t st = (hipStream_t)stream;
    void* ws = d_ws;
    if (!ws && hipMallocAsync(&ws, attention_backward_ws_bytes(B, H, Npad), st) != hipSuccess)
        return set_error(LSEG_ERR_HIP, "attention_backward_qkv: out of device memory");
    r = launch_attention_backward_qkv(d_q, d_k, d_vt, d_o, d_do, d_lse2, d_dqkv, ws, B, H, Ntok, Npad, dt, scale, st);
    if (!d_ws) (void)hipFreeAsync(ws, st);
    return r;
}

int lseg_op_bn_train_forward(const void* d_x_pad, void* d_y_pad, float* d_stats, const float* d_gamma, const float* d_beta,
                             int B, int H, int W, int C, float eps, void* stream) {
    int r = require_device(); if (r) return r;
    if (!d_x_pad || !d_stats || (d_y_pad && (!d_gamma || !d_beta))) return set_error(LSEG_ERR_INVALID, "bn_train_forward: NULL pointer");
    return launch_bn_train_forward(d_x_pad, d_y_pad, d_stats, d_gamma, d_beta, B, H, W, C, eps, DT_BF16, (hipStream_t)stream);
}

int lseg_op_bn_apply_res(const void* d_x_pad, void* d_y_pad, const float* d_stats, const float* d_gamma, const float* d_beta, const void* d_res_pad,
                         const float* d_res_stats, const float* d_res_gamma, const float* d_res_beta, int B, int H, int W, int C, float eps,
                         int relu, int dtype, void* stream) {
    int r = require_device(); if (r) return r;
    if (dtype != LSEG_BF16 && dtype != LSEG_F16) return set_error(LSEG_ERR_INVALID, "lseg_op_bn_apply_res: dtype must be LSEG_BF16 or LSEG_F16");
    return launch_bn_apply_res(d_x_pad, d_y_pad, d_stats, d_gamma, d_beta, d_res_pad, d_res_stats, d_res_gamma, d_res_beta, B, H, W, C, eps,
                               (double)B * H * W, relu, dtype == LSEG_F16 ? DT_F16 : DT_BF16, (hipStream_t)stream);
}

int lseg_op_bn_train_backward(const void* d_dy_pad, const void* d_x_pad, const float* d_stats, const float* d_gamma, void* d_dx_pad,
                              float* d_dgamma_dbeta, int B, int H, int W, int C, float eps, void* stream) {
    int r = require_device(); if (r) return r;
    if (!d_dy_pad || !d_x_pad || !d_stats || !d_gamma || !d_dx_pad || !d_dgamma_dbeta) return set_error(LSEG_ERR_INVALID, "bn_train_backward: NULL pointer");
    return launch_bn_train_backward(d_dy_pad, d_x_pad, d_stats, d_gamma, d_dx_pad, d_dgamma_dbeta, B, H, W, C, eps, DT_BF16, (hipStream_t)stream);
}

int lseg_op_relu_backward(const void* d_dy, const void* d_x, void* d_dx, int64_t n, void* stream) {
    int r = require_device(); if (r) return r;
    if (!d_dy || !d_x || !d_dx || n < 1) return set_error(LSEG_ERR_INVALID, "relu_backward: bad arguments");
    return launch_relu_backward(d_dy, d_x, d_dx, (size_t)n, (hipStream_t)stream);
}

// ---- the training backward's data-movement ("glue") kernels, one launch each: what the whole-network runs reach only through 24 bf16
// blocks is checked exactly (tests/test_gpu_train_glue.py).  Every wrapper refuses what its kernel cannot do and launches nothing.
static int glue_dt16(int lseg_dt, int* out, const char* who) {
    if (lseg_dt == LSEG_F16) { *out = DT_F16; return 0; }
    if (lseg_dt == LSEG_BF16) { *out = DT_BF16; return 0; }
    return set_error(LSEG_ERR_INVALID, "%s: dtype must be LSEG_BF16 or LSEG_F16", who);
}

int lseg_op_pos_resize(const float* d_pos, float* d_out, int g_old, int gh, int gw, int D, void* stream) {
    int r = require_device(); if (r) return r;
    if (!d_pos || !d_out || g_old < 1 || gh < 1 || gw < 1 || D < 1) return set_error(LSEG_ERR_INVALID, "pos_resize: bad arguments");
    return launch_pos_resize(d_pos, d_out, g_old, gh, gw, D, (hipStream_t)stream);
}

int lseg_op_pos_resize_backward(const float* d_dpos, float* d_dposemb, float* d_dcls, int g_old, int gh, int gw, int D, void* stream) {
    int r = require_device(); if (r) return r;
    if (!d_dpos || !d_dposemb || g_old < 1 || gh < 1 || gw < 1 || D < 1) return set_error(LSEG_ERR_INVALID, "pos_resize_backward: bad arguments");
    return launch_pos_resize_bwd(d_dpos, d_dposemb, d_dcls, g_old, gh, gw, D, (hipStream_t)stream);
}

int lseg_op_embed_backward(const float* d_gx, void* d_dtok, float* d_dpos, int B, int ntok, int D, int dtype, void* stream) {
    int r = require_device(); if (r) return r;
    int dt;
    if ((r = glue_dt16(dtype, &dt, "embed_backward"))) return r;
    if (!d_gx || !d_dtok || !d_dpos || B < 1 || ntok < 2 || D < 1) return set_error(LSEG_ERR_INVALID, "embed_backward: bad arguments (ntok >= 2)");
    return launch_embed_bwd(d_gx, d_dtok, d_dpos, B, ntok, D, dt, (hipStream_t)stream);
}

int lseg_op_readout_cat(const float* d_x, void* d_cat, int B, int ntok, int D, int dtype, void* stream) {
    int r = require_device(); if (r) return r;
    int dt;
    if ((r = glue_dt16(dtype, &dt, "readout_cat"))) return r;
    if (!d_x || !d_cat || B < 1 || ntok < 2 || D < 1) return set_error(LSEG_ERR_INVALID, "readout_cat: bad arguments (ntok >= 2)");
    if (D % 8) return set_error(LSEG_ERR_UNSUPPORTED, "readout_cat: D=%d must be a multiple of 8", D);
    return launch_readout_cat(d_x, d_cat, B, ntok, D, dt, (hipStream_t)stream);
}

int lseg_op_readout_cat_backward(const void* d_dcat, float* d_gx, int B, int ntok, int D, int dtype, void* stream) {
    int r = require_device(); if (r) return r;
    int dt;
    if ((r = glue_dt16(dtype, &dt, "readout_cat_backward"))) return r;
    if (!d_dcat || !d_gx || B < 1 || ntok < 2 || D < 1) return set_error(LSEG_ERR_INVALID, "readout_cat_backward: bad arguments (ntok >= 2)");
    if (D % 8) return set_error(LSEG_ERR_UNSUPPORTED, "readout_cat_backward: D=%d must be a multiple of 8", D);
    return launch_readout_cat_bwd(d_dcat, d_gx, B, ntok, D, dt, (hipStream_t)stream);
}

int lseg_op_unpad_rows(const void* d_in_pad, void* d_rows, int B, int H, int W, int C, void* stream) {
    int r = require_device(); if (r) return r;
    if (!d_in_pad || !d_rows || B < 1 || H < 1 || W < 1 || C < 1) return set_error(LSEG_ERR_INVALID, "unpad_rows: bad arguments");
    if (C % 8) return set_error(LSEG_ERR_UNSUPPORTED, "unpad_rows: C=%d must be a multiple of 8", C);
    return launch_unpad_rows(d_in_pad, d_rows, B, H, W, C, (hipStream_t)stream);
}

int lseg_op_dilate2(const void* d_dy_pad, void* d_dyd_pad, int B, int H, int W, int C, void* stream) {
    int r = require_device(); if (r) return r;
    if (!d_dy_pad || !d_dyd_pad || B < 1 || H < 1 || W < 1 || C < 1) return set_error(LSEG_ERR_INVALID, "dilate2: bad arguments");
    if (C % 8) return set_error(LSEG_ERR_UNSUPPORTED, "dilate2: C=%d must be a multiple of 8", C);
    return launch_dilate2(d_dy_pad, d_dyd_pad, B, (H - 1) / 2 + 1, (W - 1) / 2 + 1, H, W, C, (hipStream_t)stream);
}

int lseg_op_unpixshuf(const void* d_dl_pad, void* d_dg, int B, int gh, int gw, int s, int C, void* stream) {
    int r = require_device(); if (r) return r;
    if (!d_dl_pad || !d_dg || B < 1 || gh < 1 || gw < 1 || s < 1 || C < 1) return set_error(LSEG_ERR_INVALID, "unpixshuf: bad arguments");
    if (C % 8) return set_error(LSEG_ERR_UNSUPPORTED, "unpixshuf: C=%d must be a multiple of 8", C);
    return launch_unpixshuf(d_dl_pad, d_dg, B, gh, gw, s, C, (hipStream_t)stream);
}

int lseg_op_pack_convT(const float* d_w, void* d_wp, int Ci, int Co, int Cp, int s, int dtype, void* stream) {
    int r = require_device(); if (r) return r;
    int dt;
    if ((r = op_dt(dtype, &dt))) return r;
    if (!d_w || !d_wp || Ci < 1 || Co < 1 || s < 1 || Cp < Ci || Cp < Co) return set_error(LSEG_ERR_INVALID, "pack_convT: bad arguments (Cp >= Ci, Co)");
    return launch_pack_convT(d_w, d_wp, Ci, Co, Cp, s, dt, (hipStream_t)stream);
}

int lseg_op_convT_wgrad_unpack(const float* d_dw, float* d_dst, int C, int Cp, int s, int accumulate, void* stream) {
    int r = require_device(); if (r) return r;
    if (!d_dw || !d_dst || C < 1 || s < 1 || Cp < C) return set_error(LSEG_ERR_INVALID, "convT_wgrad_unpack: bad arguments (Cp >= C)");
    return launch_convT_wgrad_unpack(d_dw, d_dst, C, Cp, s, accumulate ? 1 : 0, (hipStream_t)stream);
}

int lseg_op_conv_wgrad_unpack(const float* d_dw, float* d_dst, int Co, int Ci, int Cip, int accumulate, int nsplit, size_t split_stride,
                              void* stream) {
    int r = require_device(); if (r) return r;
    if (!d_dw || !d_dst || Co < 1 || Ci < 1 || Cip < Ci || nsplit < 1) return set_error(LSEG_ERR_INVALID, "conv_wgrad_unpack: bad arguments (Cip >= Ci)");
    if (nsplit > 1 && split_stride < (size_t)Co * 9 * Cip)
        return set_error(LSEG_ERR_INVALID, "conv_wgrad_unpack: split_stride=%zu is smaller than one slab", split_stride);
    return launch_conv_wgrad_unpack(d_dw, d_dst, Co, Ci, Cip, accumulate ? 1 : 0, (hipStream_t)stream, nsplit, split_stride);
}

int lseg_op_fold_rows(const float* d_src, float* d_dst, int R, int C, int ld, int accumulate, void* stream) {
    int r = require_device(); if (r) return r;
    if (!d_src || !d_dst || R < 1 || C < 1 || ld < C) return set_error(LSEG_ERR_INVALID, "fold_rows: R, C >= 1, ld >= C");
    return launch_fold_rows(d_src, d_dst, R, C, ld, accumulate ? 1 : 0, (hipStream_t)stream);
}

int lseg_op_sum_partials(const float* d_part, float* d_dst, int nsplit, size_t n, size_t stride, int accumulate, void* stream) {
    int r = require_device(); if (r) return r;
    if (!d_part || !d_dst || nsplit < 1 || n < 1) return set_error(LSEG_ERR_INVALID, "sum_partials: bad arguments");
    if ((n & 3) || (stride & 3)) return set_error(LSEG_ERR_INVALID, "sum_partials: n and stride must be multiples of 4");
    if (nsplit > 1 && stride < n) return set_error(LSEG_ERR_INVALID, "sum_partials: stride=%zu is smaller than n=%zu", stride, n);
    return launch_sum_partials(d_part, d_dst, nsplit, n, stride, accumulate ? 1 : 0, (hipStream_t)stream);
}

int lseg_op_bn_running_update(const float* d_stats, float* d_rmean, float* d_rvar, int C, double count, float momentum, void* stream) {
    int r = require_device(); if (r) return r;
    if (!d_stats || !d_rmean || !d_rvar || C < 1 || !(count >= 1.0)) return set_error(LSEG_ERR_INVALID, "bn_running_update: C >= 1, count >= 1");
    return launch_bn_running_update(d_stats, d_rmean, d_rvar, C, count, momentum, (hipStream_t)stream);
}

int lseg_op_upsample2x_planes_backward_rows(const float* d_dout, void* d_rows, int B, int K, int H, int W, int ldk, int out_dtype,
                                            void* stream) {
    int r = require_device(); if (r) return r;
    int dt;
    if ((r = op_dt(out_dtype, &dt))) return r;
    if (dt == DT_F32 || !d_dout || !d_rows || B < 1 || K < 1 || H < 2 || W < 2) return set_error(LSEG_ERR_INVALID, "upsample2x_planes_backward_rows: bad arguments");
    return launch_upsample2x_planes_backward_rows(d_dout, d_rows, B, K, H, W, ldk, dt, (hipStream_t)stream);
}

int lseg_op_l2norm_scale_backward(const void* d_da, int da_dtype, const float* d_x, void* d_dx, int dx_dtype, int M, int C, float scale,
                                  void* stream) {
    int r = require_device(); if (r) return r;
    int a, b;
    if ((r = op_dt(da_dtype, &a)) || (r = op_dt(dx_dtype, &b))) return r;
    if (a == DT_F32 || b == DT_F32 || !d_da || !d_x || !d_dx || M < 1) return set_error(LSEG_ERR_INVALID, "l2norm_scale_backward: 16-bit da/dx, fp32 x");
    return launch_l2norm_scale_backward(d_da, a, d_x, d_dx, b, M, C, scale, (hipStream_t)stream);
}

int lseg_op_corr_group_fwd(const void* d_a16, const void* d_tnorm, float* d_low, int B, int hw, int G, int C, void* stream) {
    int r = require_device(); if (r) return r;
    if (!d_a16 || !d_tnorm || !d_low) return set_error(LSEG_ERR_INVALID, "corr_group_fwd: NULL pointer");
    return launch_corr_group_fwd(d_a16, d_tnorm, d_low, B, hw, G, C, (hipStream_t)stream);
}

int lseg_op_corr_group_bwd(const void* d_rows, int rows_dtype, int ldk, const void* d_tnorm, const float* d_feat, void* d_df, int df_dtype,
                           int B, int hw, int G, int C, float scale, void* stream) {
    int r = require_device(); if (r) return r;
    int a, b;
    if ((r = op_dt(rows_dtype, &a)) || (r = op_dt(df_dtype, &b))) return r;
    if (!d_rows || !d_tnorm || !d_feat || !d_df) return set_error(LSEG_ERR_INVALID, "corr_group_bwd: NULL pointer");
    return launch_corr_group_bwd(d_rows, a, ldk, d_tnorm, d_feat, d_df, b, B, hw, G, C, scale, (hipStream_t)stream);
}

size_t lseg_op_head_block_backward_ws(int B, int K, int H, int W, int apply_act) {
    if (B < 1 || K < 1 || H < 1 || W < 1) return 0;
    return (apply_act ? (size_t)B * K * H * W : 0) + 2 * (size_t)B * H * W + 10 * head_block_bwd_partials(B, H, W);
}

int lseg_op_head_block_backward(const float* d_in, const float* d_out_saved, const float* d_dy, const float* d_w9, int B, int K, int H, int W,
                                int bottleneck, int act, int apply_act, void* d_dx, int dx_dtype, int ldk, float* d_dw, float* d_db,
                                int accumulate, float* d_ws, int64_t ws_floats, void* stream) {
    int r = require_device(); if (r) return r;
    int dt;
    if ((r = op_dt(dx_dtype, &dt))) return r;
    if (!d_in || !d_dy || !d_w9 || !d_dx || !d_dw || !d_db || (apply_act && !d_out_saved))
        return set_error(LSEG_ERR_INVALID, "head_block_backward: NULL pointer");
    if (B < 1 || K < 1 || H < 1 || W < 1) return set_error(LSEG_ERR_INVALID, "head_block_backward: bad shape");
    if ((bottleneck != 0 && bottleneck != 1) || act < 0 || act > 2) return set_error(LSEG_ERR_INVALID, "head_block_backward: bottleneck %d, act %d", bottleneck, act);
    if (dt != DT_F32 && (ldk < K || (ldk & 7))) return set_error(LSEG_ERR_INVALID, "head_block_backward: ldk=%d must be a multiple of 8 and >= K=%d", ldk, K);
    const int64_t need = (int64_t)lseg_op_head_block_backward_ws(B, K, H, W, apply_act);
    if (d_ws && ws_floats < need) return set_error(LSEG_ERR_INVALID, "head_block_backward: workspace of %lld floats, %lld needed", (long long)ws_floats, (long long)need);
    hipStream_t st = (hipStream_t)stream;
    float* ws = d_ws;
    if (!ws) LSEG_HIP_TRY(hipMallocAsync((void**)&ws, (size_t)need * sizeof(float), st));
    const size_t n = (size_t)B * K * H * W, np = (size_t)B * H * W;
    float* dz = apply_act ? ws : nullptr;
    float* ksum = ws + (apply_act ? n : 0);
    int* kstar = reinterpret_cast<int*>(ksum + np);
    float* part = ksum + 2 * np;
    r = launch_head_bwd_prep(d_dy, d_out_saved, d_in, dz, bottleneck ? ksum : nullptr, bottleneck ? kstar : nullptr, B, K, H * W, act, apply_act, st);
    if (!r) r = launch_head_block_backward(apply_act ? dz : d_dy, ksum, kstar, d_in, d_w9, d_dx, dt, ldk, -1, nullptr, part, B, K, H, W, bottleneck, st);
    if (!r) r = launch_head_dw_reduce(part, (int)head_block_bwd_partials(B, H, W), d_dw, d_db, accumulate, st);
    if (!d_ws) (void)hipFreeAsync(ws, st);
    return r;
}

int lseg_op_upsample_ce_backward_planes(const float* d_low, const int64_t* d_target, int B, int K, int h, int w, int ignore_index,
                                        double* d_nll, float* d_lse_ws, float* d_planes, float* d_ksum, void* stream) {
    int r = require_device(); if (r) return r;
    if (!d_low || !d_target || !d_nll || !d_lse_ws || !d_planes) return set_error(LSEG_ERR_INVALID, "upsample_ce_backward_planes: NULL pointer");
    if (B < 1 || K < 1 || h < 2 || w < 2) return set_error(LSEG_ERR_INVALID, "upsample_ce_backward_planes: bad shape");
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* counts = nullptr;
    LSEG_HIP_TRY(hipMallocAsync((void**)&counts, (size_t)(2 + 3 * K) * sizeof(unsigned long long), st));
    r = launch_seg_stats_ex(d_low, d_target, B, K, 4 * h * w, ignore_index, counts, d_nll, nullptr, 1, h, w, st, d_lse_ws);
    if (!r) r = launch_upsample_ce_backward_planes(d_low, d_target, d_lse_ws, d_nll, d_planes, d_ksum, B, K, h, w, ignore_index, st);
    (void)hipFreeAsync(counts, st);
    return r;
}

}  // extern "C"
