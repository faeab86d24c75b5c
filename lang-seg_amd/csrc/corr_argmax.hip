// corr_argmax.hip -- masks for label sets of any size: the pixel x text correlation of LSeg (modules/models/lseg_net.py:187-196), the two
// x2 bilinears behind it (lseg_net.py:203) and torch.max(pred, 1) (lsegmentation_module.py:114-117) as ONE gfx950 kernel that never
// writes a label plane.  Per output pixel it keeps a running (best value, best label) pair while the labels stream past in panels.
//
// Inputs are what the engine holds on the commuted low-resolution schedule (engine.hip "commuted correlation"): g = padded NHWC fp16
// [B, h+2, w+2, 512], T = normalised fp16 text features [K, 512], scale = the per-pixel factor of norm_scale_plane_kernel [B, 2h, 2w].
// Outputs: label int16 [B, 4h, 4w] and (optional) score fp32 [B, 4h, 4w] = exactly the value upsample4x_planes_scaled_kernel would have
// written to logits[b, label, y, x]: the same MFMA instruction / operand roles / k order as corr_planes_kernel and the generic GEMM's
// MAP_LABELPLANES for R, and the shared interpolation functions of common.h (ups_low_value, hlerp, vlerp) behind it.
//
// Structure (one workgroup = 4 waves = one tile; the TILE is the outer loop, the label PANEL the inner one):
//   * tile = a band of CA_LB x CA_LB pixels of the (2h, 2w) "mid" map; it owns the output pixels whose upper-left mid tap lies in the
//     band (what upsample4x_planes_scaled_kernel does per row band).  Their footprint is <= 29 x 29 mid pixels and <= 16 x 16 base
//     pixels (tests/test_corr_argmax_host.py pins the mapping; the launcher re-checks it for the shape at hand).
//   * the tile's g -- 16 fragments of 16 pixels x 512 channels -- is loaded ONCE into MFMA operand registers (wave v: base rows 4v..4v+3)
//     and stays there while the panels stream: g traffic = 256 KB per tile whatever K is.
//   * per panel of CA_P = 48 labels: T rows -> LDS (pitch 1040 B, re-streamed from L2 per tile), 192 v_mfma_f32_16x16x32_f16 per wave
//     with the pixels as rows, accumulators -> LDS staging Rs [48][16 x 16] fp32.
//   * per chunk of 16 labels: all threads form the (2h, 2w) logits of the footprint, Lr [16][29 x 29]; then every lane owns one output
//     COLUMN and <= 15 consecutive output rows (wave = row group): for the chunk's labels in ascending order it walks its rows with
//     rolling horizontal interpolants (the row taps are wave-uniform and live in scalar registers) and keeps (best, arg) with a
//     strict `>` -- the first maximum wins, as in torch.max.
//   * (best, arg) never leave the registers until the last panel: 6 bytes are written per output pixel, once.
//   * a 120 x 120 map has 81 tiles per image for 256 CUs: given a workspace the launcher splits the labels of a tile over up to 8
//     workgroups (whole panels each, the split that minimises rounds x panels), each writes its (score, label) plane, and a merge
//     kernel takes them in ascending label order with the same strict `>` (6 B x pixels x splits through HBM, ~17 MB at B = 4).
//   * label confidence (lseg_op_corr_argmax_conf, the CONF instantiation): the state grows to (best, second, arg | arg2 << 16, sum of
//     exp(value - best)) -- 45 more registers per lane, 4 labels instead of 8 walk the rows together to make room (508 VGPRs, no
//     scratch) -- and 16 B per pixel are written: label, score, runner-up label and score, lse = best + log(sum).  A label part writes
//     the same five planes (16 B x pixels x splits) and the merge combines them in ascending order: top-2 by the same strict `>` rule,
//     lse by log-add-exp.  The arg-max instantiation compiles to the instructions it had before the template parameter existed.
// Around the kernel there is ONE of everything, each a template over the mode (CaMode: arg-max / CONF / LOSS): one host plan of a launch
// (CaPlan: tiles, panels, label parts), one launch site (ca_launch, the six instantiations listed once in CA_VARIANTS), one merge of
// the label parts (corr_argmax_merge_kernel), one fallback on planes in memory (seg_labels16_kernel).  The per-value rules -- the valid
// target, the one-exp log-sum-exp step, the top-2 push, the log-add-exp, the write-out -- are device functions the three share, so
// "the same bits" between the forms holds by construction.
// LDS: T 49 920 + Rs 49 920 + Lr 54 016 + row taps 1 024 = 154 880 B of the CU's 160 KB.
// Traffic per image at 120 x 120, K = 1000 (81 tiles, 21 panels): g 21 MB (halo included) from HBM, T 81 x 1 MB from L2, 1.4 MB written --
// against the 922 MB logits write (and read) this replaces.  The panel-outer alternative would read g 15 MB x 21 panels and carry the
// state through HBM (6 B x 230 400 pixels x 2 x 21 = 58 MB).  Bound: VALU (the interpolation), not memory and not MFMA -- see DESIGN §3.4.
#include "ops.h"
#include "gemm.h"
#include "../../include/lseg_hip.h"

#include <atomic>
#include <vector>

namespace lseg {
namespace {

constexpr int CA_C = 512;                   // channels
constexpr int CA_KS = CA_C / 32;            // k-steps of 32 channels
constexpr int CA_PITCH = CA_C * 2 + 16;     // LDS row pitch of T in bytes
constexpr int CA_LB = 28;                   // mid rows / columns of a tile's band
constexpr int CA_MT = CA_LB + 1;            // mid rows / columns of its footprint
constexpr int CA_BT = 16;                   // base rows / columns of its footprint (= one MFMA fragment of pixels per row)
constexpr int CA_P = 48;                    // labels per panel
constexpr int CA_NLB = CA_P / 16;
constexpr int CA_LC = 16;                   // labels per interpolation chunk
constexpr int CA_LU = 8;                    // labels that walk the output rows together
constexpr int CA_RP = CA_BT * CA_BT + 4;    // floats per label in Rs (+4: the 16 labels of a store land in different banks)
constexpr int CA_LP = (CA_MT * CA_MT + 3) / 4 * 4;   // floats per label in Lr
constexpr int CA_ROWS = 15;                 // output rows per wave
constexpr int CA_OMAX_Y = 4 * CA_ROWS;      // owned output rows per tile (<= 58 by construction)
constexpr int CA_OMAX_X = 64;               // owned output columns per tile (one per lane)
constexpr int CA_SLOTS = (CA_MT * CA_MT + 255) / 256;
constexpr size_t CA_LDS = (size_t)CA_P * CA_PITCH + (size_t)CA_P * CA_RP * 4 + (size_t)CA_LC * CA_LP * 4 + 64 * 16;

// first output index whose upper tap floor(r * o) is >= a   (r = (n_mid - 1) / (n_out - 1), the kernel's own float arithmetic)
__host__ __device__ inline int ca_first_out(float r, int a) {
    int o = (int)ceilf((float)a / r);
    while (o > 0 && (int)(r * (float)(o - 1)) >= a) --o;
    while ((int)(r * (float)o) < a) ++o;
    return o;
}
__host__ __device__ inline int ca_end_out(float r, int first, int a_end, int n_out) {
    int o = first;
    while (o < n_out && (int)(r * (float)o) < a_end) ++o;
    return o;
}

// what a run keeps per pixel beside (best, arg): nothing / the runner-up and the exp-sum / the exp-sum and the target's logit
enum class CaMode { ARGMAX, CONF, LOSS };
inline CaMode ca_mode(const CorrOut& out, const CorrLoss* loss) {
    return loss ? CaMode::LOSS : (out.label2 || out.score2 || out.lse) ? CaMode::CONF : CaMode::ARGMAX;
}
// bytes per output pixel of the planes a label part writes: label int16 + score fp32, CONF label2 int16 + score2 + lse fp32, LOSS lse + tlogit fp32
constexpr size_t ca_part_bytes(CaMode m) { return 2 + 4 + (m == CaMode::CONF ? 2 + 4 + 4 : m == CaMode::LOSS ? 4 + 4 : 0); }

// a pixel enters the loss iff its target is a label of the set at hand (label_stats_kernel's pixel_nll rule)
__device__ __forceinline__ bool valid_target(long long t, int ignore_index, int K) {
    return t != (long long)ignore_index && t >= 0 && t < (long long)K;
}

// one more value v into an online log-sum-exp whose running maximum is `best` (updated by the caller afterwards): one exp per value --
// exp(-|v - best|) rescales the sum when v is the new maximum and is v's own term otherwise (best = -inf before the first value:
// exp(-inf) = 0 and the sum starts at 1)
__device__ __forceinline__ void lse_push(float& sum, float v, float best) {
    const float e = __expf(-fabsf(v - best));
    sum = v > best ? fmaf(sum, e, 1.f) : sum + e;
}

// CONF = the label-confidence instantiation (lseg_op_corr_argmax_conf): besides (best, arg) every owned pixel keeps the runner-up
// (second, arg2) -- the largest value among the labels != arg, ties to the lower label, i.e. entry 1 of a stable descending sort over k
// -- and the sum s of exp(value - best) over all labels seen, so that lse = best + log(s) (the running maximum of an online
// log-sum-exp IS best: no separate m).  arg and arg2 share one register (16 bits each): 3 x 15 state registers on top of the arg-max's.
//
// RAGGED = per-image label sets of any size (lseg_op_corr_argmax_ragged): `offsets` int32 [B + 1] is the prefix sum of the images' label
// counts; image b streams rows [offsets[b], offsets[b + 1]) of T_all only and reports labels local to its own list, and the kernel's K
// (unused by the launcher there) gives way to the image's count.  A label part that lies beyond its image's count returns before it
// touches anything: the merge kernel skips it (it reads the same offsets), no identity element is ever written.  With RAGGED = false
// nothing of this is compiled: the shared-set instantiations keep their instructions and registers.
//
// LOSS = the cross-entropy instantiation (lseg_op_corr_argmax_loss; CONF = false): besides (best, arg) every owned pixel keeps the sum s of
// exp(value - best) -- CONF's recurrence, so lse is CONF's bit for bit -- and tlogit, the logit of the pixel's TARGET label, taken when that
// label walks past (it passes through the registers exactly once; -inf until then, and for good where the target is not valid).  There is
// no runner-up: the target's label rides in the upper half of arg's register where CONF keeps arg2 (0xffff = not valid: no label
// reaches it), and tlogit takes the place of second -- the same 3 x 15 state registers on top of the arg-max's, so the same 4 labels walk
// the rows together.  `target` is int64 [B, 4H, 4W]; a pixel is valid iff target != ignore_index and 0 <= target < K (RAGGED: the
// image's own count) -- label_stats_kernel's pixel_nll rule.  Rows past K enter neither the sum nor tlogit (the `< K` guard CONF has).
template <bool CONF, bool RAGGED, bool LOSS = false>
__global__ __launch_bounds__(256, 1) void corr_argmax_kernel(const uint16_t* __restrict__ g, const uint16_t* __restrict__ T_all,
                                                            const float* __restrict__ scale, int16_t* __restrict__ label,
                                                            float* __restrict__ score, int B, int K_all, int H, int W, int tiles_y, int tiles_x,
                                                            int nsplit, int split_labels, size_t split_stride, int16_t* __restrict__ label2,
                                                            float* __restrict__ score2, float* __restrict__ lse, const int* __restrict__ offsets,
                                                            const long long* __restrict__ target = nullptr, int ignore_index = 0,
                                                            float* __restrict__ tlogit = nullptr) {
    static_assert(!(CONF && LOSS), "the loss form keeps no runner-up");
    extern __shared__ __attribute__((aligned(16))) char lds[];
    char* tlds = lds;
    float* Rs = reinterpret_cast<float*>(lds + CA_P * CA_PITCH);
    float* Lr = Rs + CA_P * CA_RP;
    int4* rtab = reinterpret_cast<int4*>(Lr + CA_LC * CA_LP);
    const int HP = H + 2, WP = W + 2, Hl = 2 * H, Wl = 2 * W, Ho = 4 * H, Wo = 4 * W;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, kg = lane >> 4;

    // label split `sp` of tile `ut` covers labels [k_lo, k_hi) (whole panels) and writes plane `sp` of the (label, score) workspace
    const unsigned ut = blockIdx.x / (unsigned)nsplit, sp = blockIdx.x - ut * (unsigned)nsplit;
    const unsigned q = ut / (unsigned)tiles_x, tx = ut - q * (unsigned)tiles_x;
    const unsigned b = q / (unsigned)tiles_y, ty = q - b * (unsigned)tiles_y;
    const int row0 = RAGGED ? offsets[b] : 0;                            // (workgroup-uniform: scalar loads)
    const int K = RAGGED ? offsets[b + 1] - row0 : K_all;
    const uint16_t* __restrict__ T = T_all + (size_t)row0 * CA_C;
    const int k_lo = (int)sp * split_labels, k_hi = k_lo + split_labels < K ? k_lo + split_labels : K;
    if constexpr (RAGGED) {
        if (k_lo >= K) return;                                           // an empty part of a short list (before the first barrier)
    }
    const int Ya = (int)ty * CA_LB, Xa = (int)tx * CA_LB;
    const int Yb = Ya + CA_LB < Hl - 1 ? Ya + CA_LB : Hl - 1, Xb = Xa + CA_LB < Wl - 1 ? Xa + CA_LB : Wl - 1;   // last mid row / column read
    const int nmy = Yb - Ya + 1, nmx = Xb - Xa + 1;
    const float ry1 = (float)(H - 1) / (float)(Hl - 1), rx1 = (float)(W - 1) / (float)(Wl - 1);
    const float ry2 = (float)(Hl - 1) / (float)(Ho - 1), rx2 = (float)(Wl - 1) / (float)(Wo - 1);
    const int by_lo = (int)(ry1 * (float)Ya), bx_lo = (int)(rx1 * (float)Xa);            // base origin of the footprint

    // ---- owned output rows / columns; the row taps of the tile -> LDS -> scalar registers -------------------------------------------
    const int yo_first = ca_first_out(ry2, Ya), yo_end = ca_end_out(ry2, yo_first, Ya + CA_LB, Ho);
    const int xo_first = ca_first_out(rx2, Xa), xo_end = ca_end_out(rx2, xo_first, Xa + CA_LB, Wo);
    if (tid < 64) {
        int yo = yo_first + tid;
        yo = yo < yo_end ? yo : yo_end - 1;
        int y0, y1;
        float ly;
        src_tap(ry2, yo, Hl, y0, y1, ly);
        rtab[tid] = make_int4((y0 - Ya) * CA_MT, (y1 - Ya) * CA_MT, __float_as_int(ly), 0);
    }
    const int per = (yo_end - yo_first + 3) / 4;                         // <= CA_ROWS (launcher)
    const int ys = yo_first + wave * per;
    const int nrow = ys >= yo_end ? 0 : (ys + per < yo_end ? per : yo_end - ys);
    int xo = xo_first + lane;
    const bool cvalid = xo < xo_end;
    xo = cvalid ? xo : xo_end - 1;
    int cx0, cx1;
    float clx;
    src_tap(rx2, xo, Wl, cx0, cx1, clx);
    cx0 -= Xa; cx1 -= Xa;

    // ---- this thread's mid pixels of the footprint (stage 1) -------------------------------------------------------------------------
    int s_roff[CA_SLOTS], s_dx[CA_SLOTS], s_dy[CA_SLOTS], s_loff[CA_SLOTS];
    float s_lx[CA_SLOTS], s_ly[CA_SLOTS], s_sc[CA_SLOTS];
#pragma unroll
    for (int s = 0; s < CA_SLOTS; ++s) {
        const int i = tid + 256 * s;
        const bool ok = i < nmy * nmx;
        const int my = ok ? i / nmx : 0, mx = ok ? i - my * nmx : 0;
        int y0, y1, x0, x1;
        src_tap(ry1, Ya + my, H, y0, y1, s_ly[s]);
        src_tap(rx1, Xa + mx, W, x0, x1, s_lx[s]);
        s_roff[s] = (y0 - by_lo) * CA_BT + (x0 - bx_lo);
        s_dx[s] = x1 - x0;
        s_dy[s] = (y1 - y0) * CA_BT;
        s_loff[s] = ok ? my * CA_MT + mx : -1;
        s_sc[s] = scale[((size_t)b * Hl + Ya + my) * Wl + Xa + mx];
    }

    // ---- LOSS: the owned pixels' targets, before the fragments fill the registers (already shifted into the upper half of arg) ---------------
    constexpr int CA_TROWS = LOSS ? CA_ROWS : 1;
    int tg16[CA_TROWS];
    if constexpr (LOSS) {
#pragma unroll
        for (int j = 0; j < CA_ROWS; ++j) {
            int tg = 0xffff;
            if (j < nrow && cvalid) {
                const long long t = target[((size_t)b * Ho + ys + j) * Wo + xo];
                if (t != (long long)ignore_index && t >= 0 && t < (long long)K) tg = (int)t;   // valid_target, spelled out: the call reorders this body's code
            }
            tg16[j] = (int)((unsigned)tg << 16);
        }
    }

    // ---- g: the tile's fragments, once (rows / columns clamped into the map: a clamped pixel is a copy nothing reads) ------------------
    i32x4_t gf[CA_KS][4];
    {
        int bx = bx_lo + c;
        bx = bx < W - 1 ? bx : W - 1;
        const char* gbase = reinterpret_cast<const char*>(g);
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            int by = by_lo + 4 * wave + rr;
            by = by < H - 1 ? by : H - 1;
            const uint32_t off = (((uint32_t)b * (uint32_t)HP + (uint32_t)(1 + by)) * (uint32_t)WP + (uint32_t)(1 + bx)) * (CA_C * 2) + (uint32_t)kg * 16u;
#pragma unroll
            for (int ks = 0; ks < CA_KS; ++ks) gf[ks][rr] = *reinterpret_cast<const i32x4_t*>(gbase + off + ks * 64);
        }
    }
    __syncthreads();                                                    // rtab
    int r_y0[CA_ROWS], r_y1[CA_ROWS];
    float r_ly[CA_ROWS];
#pragma unroll
    for (int j = 0; j < CA_ROWS; ++j) {
        int idx = ys - yo_first + j;
        idx = idx < 63 ? idx : 63;
        const int4 e = rtab[idx];
        r_y0[j] = __builtin_amdgcn_readfirstlane(e.x);
        r_y1[j] = __builtin_amdgcn_readfirstlane(e.y);
        r_ly[j] = __int_as_float(__builtin_amdgcn_readfirstlane(e.z));
    }

    float best[CA_ROWS];
    int arg[CA_ROWS];
#pragma unroll
    for (int j = 0; j < CA_ROWS; ++j) { best[j] = -INFINITY; arg[j] = 0; }
    constexpr int CA_CROWS = CONF ? CA_ROWS : 1;
    float second[CA_CROWS], esum[CA_CROWS];                              // CONF; arg[j] = arg | arg2 << 16 there
#pragma unroll
    for (int j = 0; j < CA_CROWS; ++j) { second[j] = -INFINITY; esum[j] = 0.f; }
    float lsum[CA_TROWS], tl[CA_TROWS];                                  // LOSS; arg[j] = arg | target << 16 there (0xffff: not valid)
#pragma unroll
    for (int j = 0; j < CA_TROWS; ++j) { lsum[j] = 0.f; tl[j] = -INFINITY; }
    if constexpr (LOSS) {
#pragma unroll
        for (int j = 0; j < CA_ROWS; ++j) arg[j] = tg16[j];
    }

    for (int pb = k_lo; pb < k_hi; pb += CA_P) {
        // ---- T panel -> LDS (rows past K repeat the last label: computed, never compared) ------------------------------------------------
        for (int i = tid; i < CA_P * (CA_C / 8); i += 256) {
            const int row = i / (CA_C / 8), ch = i - row * (CA_C / 8);
            int lab = pb + row;
            lab = lab < K ? lab : K - 1;
            *reinterpret_cast<i32x4_t*>(tlds + row * CA_PITCH + ch * 16) = *reinterpret_cast<const i32x4_t*>(T + (size_t)lab * CA_C + ch * 8);
        }
        __syncthreads();
        // ---- R tile of the panel: pixels as rows, one accumulator chain over the 16 k-steps in ascending order --------------------------
        {
            f32x4_t acc[CA_NLB][4];
#pragma unroll
            for (int lb = 0; lb < CA_NLB; ++lb)
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) acc[lb][rr] = f32x4_t{0.f, 0.f, 0.f, 0.f};
            // the T fragments of k-step ks + 1 are requested before the MFMAs of k-step ks: with one wave per SIMD nothing else hides the LDS
            auto tread = [&](int ks, int lb) { return *reinterpret_cast<const i32x4_t*>(tlds + (lb * 16 + c) * CA_PITCH + kg * 16 + ks * 64); };
            i32x4_t tf[2][CA_NLB];
#pragma unroll
            for (int lb = 0; lb < CA_NLB; ++lb) tf[0][lb] = tread(0, lb);
#pragma unroll
            for (int ks = 0; ks < CA_KS; ++ks) {
                if (ks + 1 < CA_KS) {
#pragma unroll
                    for (int lb = 0; lb < CA_NLB; ++lb) tf[(ks + 1) & 1][lb] = tread(ks + 1, lb);
                }
#pragma unroll
                for (int lb = 0; lb < CA_NLB; ++lb)
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) acc[lb][rr] = mfma16<F16>(gf[ks][rr], tf[ks & 1][lb], acc[lb][rr]);
                __builtin_amdgcn_sched_barrier(0);
            }
            // D rows 4 kg .. 4 kg + 3 = 4 consecutive pixels of base row 4 wave + rr, D column c = label 16 lb + c
#pragma unroll
            for (int lb = 0; lb < CA_NLB; ++lb)
#pragma unroll
                for (int rr = 0; rr < 4; ++rr)
                    *reinterpret_cast<f32x4_t*>(Rs + (lb * 16 + c) * CA_RP + (4 * wave + rr) * CA_BT + 4 * kg) = acc[lb][rr];
        }
        __syncthreads();
        for (int cb = 0; cb < CA_P && pb + cb < K; cb += CA_LC) {
            // ---- stage 1: the (2h, 2w) logits of the footprint for the chunk's 16 labels (rows past K repeat the last label) -------------
            // One wave per SIMD: nothing but the next labels' reads hides an LDS round trip, so four labels are in flight per pass
#pragma unroll 4
            for (int l = 0; l < CA_LC; ++l) {
                const float* Rl = Rs + (cb + l) * CA_RP;
                float* Ll = Lr + l * CA_LP;
#pragma unroll
                for (int s = 0; s < CA_SLOTS; ++s) {
                    if (s_loff[s] < 0) continue;
                    const float* p = Rl + s_roff[s];
                    Ll[s_loff[s]] = ups_low_value(s_sc[s], p[0], p[s_dx[s]], p[s_dy[s]], p[s_dy[s] + s_dx[s]], s_lx[s], s_ly[s]);
                }
            }
            __syncthreads();
            // ---- stage 2: output_conv's bilinear + the running arg-max, labels in ascending order ----------------------------------------
            // CA_LU labels walk the rows together: the row pattern (which mid row is new) is the same for every label, so one uniform
            // branch serves CA_LU independent interpolants and their 2 CA_LU LDS reads are in flight at once (CONF: 4 -- its 45 more state
            // registers leave no room for 8 interpolant pairs, and its per-value arithmetic hides the LDS reads of 4)
            constexpr int LU = CONF || LOSS ? 4 : CA_LU;
            for (int l0 = 0; l0 < CA_LC && pb + cb + l0 < K; l0 += LU) {
                const float* Ll = Lr + l0 * CA_LP;
                const int lab0 = pb + cb + l0;
                float h0[LU], h1[LU];
#pragma unroll
                for (int u = 0; u < LU; ++u) { h0[u] = 0.f; h1[u] = 0.f; }
                int c0 = -1, c1 = -1;                                    // the mid rows h0 / h1 hold (wave-uniform)
#pragma unroll
                for (int j = 0; j < CA_ROWS; ++j) {
                    if (j >= nrow) continue;                              // (wave-uniform)
                    const int y0 = r_y0[j], y1 = r_y1[j];
                    if (y0 != c0) {
                        if (y0 == c1) {
#pragma unroll
                            for (int u = 0; u < LU; ++u) h0[u] = h1[u];
                        } else {
#pragma unroll
                            for (int u = 0; u < LU; ++u) h0[u] = hlerp(Ll[u * CA_LP + y0 + cx0], Ll[u * CA_LP + y0 + cx1], clx);
                        }
                        c0 = y0;
                    }
                    if (y1 != c1) {
                        if (y1 == c0) {
#pragma unroll
                            for (int u = 0; u < LU; ++u) h1[u] = h0[u];
                        } else {
#pragma unroll
                            for (int u = 0; u < LU; ++u) h1[u] = hlerp(Ll[u * CA_LP + y1 + cx0], Ll[u * CA_LP + y1 + cx1], clx);
                        }
                        c1 = y1;
                    }
#pragma unroll
                    for (int u = 0; u < LU; ++u) {
                        const float v = vlerp(h0[u], h1[u], r_ly[j]);
                        if constexpr (LOSS) {
                            if (lab0 + u < K) {                                                   // CONF's sum, the target's logit on its way past
                                const float e = __expf(-fabsf(v - best[j]));
                                if ((int)((unsigned)arg[j] >> 16) == lab0 + u) tl[j] = v;
                                if (v > best[j]) {
                                    lsum[j] = fmaf(lsum[j], e, 1.f);
                                    best[j] = v;
                                    arg[j] = (int)((unsigned)arg[j] & 0xffff0000u) | (lab0 + u);
                                } else {
                                    lsum[j] += e;
                                }
                            }
                        } else if constexpr (!CONF) {
                            if (lab0 + u < K && v > best[j]) { best[j] = v; arg[j] = lab0 + u; }      // first maximum wins
                        } else if (lab0 + u < K) {
                            // lse_push spelled out with the branch it shares (as a call it costs this body scratch): one exp per value --
                            // exp(-|v - best|) rescales the sum when v is the new maximum and is v's own term otherwise
                            const float e = __expf(-fabsf(v - best[j]));
                            if (v > best[j]) {                                                    // first maximum wins; the old one is the runner-up
                                esum[j] = fmaf(esum[j], e, 1.f);
                                second[j] = best[j]; best[j] = v;
                                arg[j] = (int)((unsigned)arg[j] << 16) | (lab0 + u);
                            } else {
                                esum[j] += e;
                                if (v > second[j]) { second[j] = v; arg[j] = (arg[j] & 0xffff) | ((lab0 + u) << 16); }   // a later equal of best lands here
                            }
                        }
                    }
                }
            }
            __syncthreads();
        }
    }

    if (cvalid) {
#pragma unroll
        for (int j = 0; j < CA_ROWS; ++j) {
            if (j >= nrow) continue;
            const size_t o = (size_t)sp * split_stride + ((size_t)b * Ho + ys + j) * Wo + xo;
            if constexpr (LOSS) {
                label[o] = (int16_t)(arg[j] & 0xffff);
                if (score) score[o] = best[j];
                if (lse) lse[o] = best[j] + logf(lsum[j]);
                if (tlogit) tlogit[o] = tl[j];
            } else if constexpr (!CONF) {
                label[o] = (int16_t)arg[j];
                if (score) score[o] = best[j];
            } else {
                label[o] = (int16_t)(arg[j] & 0xffff);
                if (score) score[o] = best[j];
                if (label2) label2[o] = second[j] == -INFINITY ? (int16_t)-1 : (int16_t)((unsigned)arg[j] >> 16);   // one label: no runner-up
                if (score2) score2[o] = second[j];
                if (lse) lse[o] = best[j] + logf(esum[j]);
            }
        }
    }
}

// a pixel's results -> the planes of its mode, each but the label optional (the merge and the fallback; the streamed kernel's own
// write-out forms lse only where it is wanted)
template <CaMode MODE>
__device__ __forceinline__ void ca_store(const CorrOut& out, size_t o, int a, float m, int a2, float m2, float l, float t) {
    out.label[o] = (int16_t)a;
    if (out.score) out.score[o] = m;
    if constexpr (MODE == CaMode::CONF) {
        if (out.label2) out.label2[o] = (int16_t)a2;
        if (out.score2) out.score2[o] = m2;
    }
    if constexpr (MODE != CaMode::ARGMAX) {
        if (out.lse) out.lse[o] = l;
    }
    if constexpr (MODE == CaMode::LOSS) {
        if (out.tlogit) out.tlogit[o] = t;
    }
}

// one more value (v, label k) into a pixel's running top-2, labels arriving in ascending order: the rule of the streamed kernel's CONF body,
// shared by the merge and the fallback -- strict `>` twice, so equal values keep the lower label and a later equal of best is the runner-up
__device__ inline void top2_push(float v, int k, float& best, int& arg, float& second, int& arg2) {
    const bool nb = v > best, ns = !nb && v > second;                  // (selects, not branches: the state stays in registers)
    second = nb ? best : (ns ? v : second);
    arg2 = nb ? arg : (ns ? k : arg2);
    best = nb ? v : best;
    arg = nb ? k : arg;
}

// log(exp(l) + exp(pl)): the log-sum-exp of two label parts
__device__ __forceinline__ float lse_add(float l, float pl) { return fmaxf(l, pl) + log1pf(expf(-fabsf(l - pl))); }

// ragged label sets (offsets != NULL): image i / img_pix owns ceil(count / split_labels) parts, the rest were never written and are not read
__device__ inline int ca_parts_of(const int* __restrict__ offsets, int split_labels, unsigned img_pix, size_t i, int nsplit) {
    if (!offsets) return nsplit;
    const size_t b = i / img_pix;
    const int parts = (offsets[b + 1] - offsets[b] + split_labels - 1) / split_labels;
    return parts < nsplit ? parts : nsplit;
}

// the planes of the label parts (w, each [nsplit][n]) -> the final outputs.  Parts in ascending order = labels in ascending order: the
// winner by strict `>`, the first maximum wins (CONF: a part's winner and then its runner-up are pushed like single labels -- the
// runner-up can only matter when the winner became the new best); lse by log-add-exp; tlogit by max -- exactly one part holds the
// target's label, every other part left -inf
template <CaMode MODE>
__global__ __launch_bounds__(256) void corr_argmax_merge_kernel(CorrOut w, CorrOut out, int nsplit, size_t n, const int* __restrict__ offsets,
                                                                int split_labels, unsigned img_pix) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        float m = w.score[i], m2 = -INFINITY, l = 0.f, t = 0.f;
        int a = w.label[i], a2 = -1;
        if constexpr (MODE == CaMode::CONF) { m2 = w.score2[i]; a2 = w.label2[i]; }
        if constexpr (MODE != CaMode::ARGMAX) l = w.lse[i];
        if constexpr (MODE == CaMode::LOSS) t = w.tlogit[i];
        const int parts = ca_parts_of(offsets, split_labels, img_pix, i, nsplit);
        for (int s = 1; s < parts; ++s) {
            const size_t o = (size_t)s * n + i;
            if constexpr (MODE == CaMode::CONF) {
                top2_push(w.score[o], w.label[o], m, a, m2, a2);
                top2_push(w.score2[o], w.label2[o], m, a, m2, a2);      // -inf (a part of one label) never enters
            } else {
                const float v = w.score[o];
                if (v > m) { m = v; a = w.label[o]; }
            }
            if constexpr (MODE != CaMode::ARGMAX) l = lse_add(l, w.lse[o]);
            if constexpr (MODE == CaMode::LOSS) t = fmaxf(t, w.tlogit[o]);
        }
        ca_store<MODE>(out, i, a, m, a2, m2, l, t);
    }
}

// ---- the cross-entropy sum of the (lse, tlogit) planes: nll = {sum over the valid pixels of double(lse) - double(tlogit), their number} ------
// Fixed order, no atomics: workgroup j owns the pixels [j * chunk, (j + 1) * chunk) (chunk a multiple of CL_THREADS: lane t of it takes
// pixel j * chunk + t + CL_THREADS * m for m = 0, 1, ...), its lanes' sums meet in a shuffle tree and the four wave totals are added in
// ascending order into partial j; corr_loss_fold_kernel's one wave then adds the partials (lane l: l, l + 64, ... ascending, then the same
// tree).  Two runs on the same planes give the same bits.  The valid rule is the streamed kernel's (label_stats_kernel's pixel_nll).
// plane (optional) = float(lse - tlogit), 0 where the pixel is not valid.
constexpr int CL_THREADS = 256;
constexpr int CL_MIN_PIXELS = 4096;                       // pixels per workgroup at least (sixteen per lane)
constexpr int CL_MAX_GROUPS = 1024;                       // partials at most: 16 KB of workspace

// {pixels per workgroup, workgroups} for n pixels
inline void cl_plan(size_t n, size_t& chunk, int& groups) {
    size_t g = (n + CL_MIN_PIXELS - 1) / CL_MIN_PIXELS;
    g = g < 1 ? 1 : (g > (size_t)CL_MAX_GROUPS ? (size_t)CL_MAX_GROUPS : g);
    chunk = ((n + g - 1) / g + CL_THREADS - 1) / CL_THREADS * CL_THREADS;
    groups = (int)((n + chunk - 1) / chunk);
}

template <typename Count>                                 // (unsigned in the reduction, double once the counts are partials)
__device__ inline void cl_wave_sum(double& s, Count& c) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s += __shfl_down(s, off, 64);
        c += __shfl_down(c, off, 64);
    }
}

__global__ __launch_bounds__(CL_THREADS) void corr_loss_reduce_kernel(const float* __restrict__ lse, const float* __restrict__ tlogit,
                                                                      const long long* __restrict__ target, int ignore_index, int K,
                                                                      const int* __restrict__ offsets, unsigned img_pix, size_t n, size_t chunk,
                                                                      float* __restrict__ plane, double* __restrict__ partial) {
    __shared__ double ws[CL_THREADS / 64];
    __shared__ unsigned wc[CL_THREADS / 64];
    const size_t lo = blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
    double s = 0.0;
    unsigned c = 0;
    for (size_t i = lo + threadIdx.x; i < hi; i += CL_THREADS) {
        const long long t = target[i];
        int k = K;
        if (offsets) {
            const size_t b = i / img_pix;
            k = offsets[b + 1] - offsets[b];
        }
        const bool valid = valid_target(t, ignore_index, k);
        const float l = lse[i], g = tlogit[i];
        if (valid) { s += (double)l - (double)g; ++c; }
        if (plane) plane[i] = valid ? l - g : 0.f;
    }
    cl_wave_sum(s, c);
    if ((threadIdx.x & 63) == 0) { ws[threadIdx.x >> 6] = s; wc[threadIdx.x >> 6] = c; }
    __syncthreads();
    if (threadIdx.x == 0 && partial) {
        double ts = ws[0];
        unsigned tc = wc[0];
#pragma unroll
        for (int w = 1; w < CL_THREADS / 64; ++w) { ts += ws[w]; tc += wc[w]; }
        partial[2 * (size_t)blockIdx.x] = ts;
        partial[2 * (size_t)blockIdx.x + 1] = (double)tc;
    }
}

__global__ __launch_bounds__(64) void corr_loss_fold_kernel(const double* __restrict__ partial, int groups, double* __restrict__ nll) {
    double s = 0.0, c = 0.0;
    for (int i = threadIdx.x; i < groups; i += 64) { s += partial[2 * i]; c += partial[2 * i + 1]; }
    cl_wave_sum(s, c);
    if (threadIdx.x == 0) { nll[0] = s; nll[1] = c; }
}

// the fallback: what the streamed kernel's callers get when the (2h, 2w) planes exist in memory -- the x2-upsampled logits read through
// the bilinear on the fly (seg_stats_kernel's `up` form), labels in ascending order through the streamed kernel's per-value rules: the
// winner by strict `>`; CONF the runner-up through top2_push; CONF / LOSS the online log-sum-exp whose running maximum is the winner
// (lse_push); LOSS tlogit = the value of the target's plane at this pixel, the very bilerp the loop meets at k = target (-inf where
// the target is not valid).  K = 1: label2 = -1, score2 = -inf, lse = score
template <CaMode MODE>
__global__ __launch_bounds__(256) void seg_labels16_kernel(const float* __restrict__ low, int K, int h, int w, size_t npix,
                                                           const long long* __restrict__ target, int ignore_index, CorrOut out) {
    const int Wo = 2 * w, HW = 4 * h * w;
    const float ry = (float)(h - 1) / (float)(2 * h - 1), rx = (float)(w - 1) / (float)(2 * w - 1);
    const size_t kstride = (size_t)h * w;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < npix; i += (size_t)gridDim.x * blockDim.x) {
        const int p = (int)(i % HW);
        const size_t b = i / HW;
        const int yo = p / Wo, xo = p - yo * Wo;
        int y0, y1, x0, x1;
        float ly, lx;
        src_tap(ry, yo, h, y0, y1, ly);
        src_tap(rx, xo, w, x0, x1, lx);
        const float* col = low + b * (size_t)K * kstride + (size_t)y0 * w + x0;
        const int o01 = x1 - x0, o10 = (y1 - y0) * w, o11 = o10 + o01;
        int tg = -1;
        if constexpr (MODE == CaMode::LOSS) {
            const long long t = target[i];
            if (valid_target(t, ignore_index, K)) tg = (int)t;
        }
        float m = -INFINITY, m2 = -INFINITY, es = 0.f, tl = -INFINITY;
        int arg = 0, arg2 = -1;
        for (int k = 0; k < K; ++k) {
            const float* cc = col + (size_t)k * kstride;
            const float v = bilerp(cc[0], cc[o01], cc[o10], cc[o11], lx, ly);
            if constexpr (MODE != CaMode::ARGMAX) lse_push(es, v, m);
            if constexpr (MODE == CaMode::LOSS) tl = k == tg ? v : tl;
            if constexpr (MODE == CaMode::CONF) {
                top2_push(v, k, m, arg, m2, arg2);
            } else if (v > m) {
                m = v;
                arg = k;
            }
        }
        ca_store<MODE>(out, i, arg, m, m2 == -INFINITY ? -1 : arg2, m2, m + logf(es), tl);
    }
}

// the tile -> footprint mapping for this shape, in the kernel's own arithmetic (tests/test_corr_argmax_host.py is its model)
bool ca_tiles_fit(int n_base, int n_mid, int n_out, int max_out) {
    const float r1 = (float)(n_base - 1) / (float)(n_mid - 1), r2 = (float)(n_mid - 1) / (float)(n_out - 1);
    int covered = 0;
    for (int a = 0; a < n_mid; a += CA_LB) {
        const int bmid = a + CA_LB < n_mid - 1 ? a + CA_LB : n_mid - 1;
        const int lo = (int)(r1 * (float)a);
        int hi = (int)(r1 * (float)bmid);
        hi += hi < n_base - 1;
        if (hi - lo + 1 > CA_BT) return false;
        const int first = ca_first_out(r2, a), end = ca_end_out(r2, first, a + CA_LB, n_out);
        if (first != covered || end - first > max_out) return false;
        covered = end;
    }
    return covered == n_out;
}

}  // namespace

// the kernel's tile geometry, for the host-side index model: {CA_LB, CA_MT, CA_BT, CA_P, CA_PITCH, CA_LC, CA_ROWS, dynamic LDS bytes}
void corr_argmax_geometry(int* out8) {
    const int v[8] = {CA_LB, CA_MT, CA_BT, CA_P, CA_PITCH, CA_LC, CA_ROWS, (int)CA_LDS};
    for (int i = 0; i < 8; ++i) out8[i] = v[i];
}

bool corr_argmax_supported(int K, int C) { return C == CA_C && K >= 1 && K <= 32767; }

namespace {

// label splits: the fewest rounds x (panels per split + ~1 panel of set-up) over the CUs, each part whole panels
int ca_pick_split(int panels, long ntiles, size_t npix, size_t part_bytes, bool has_ws, size_t ws_bytes, int cus) {
    int nsplit = 1;
    long best_cost = 0;
    for (int s = 1; s <= 8 && s <= panels; ++s) {
        const int per = (panels + s - 1) / s;
        if ((per * (s - 1)) >= panels) continue;                       // the last split would be empty
        if (s > 1 && (!has_ws || ws_bytes < (size_t)s * npix * part_bytes || ntiles * s >= (1L << 31))) break;
        const long cost = ((ntiles * s + cus - 1) / cus) * (long)(per + 1);
        if (s == 1 || cost < best_cost) { best_cost = cost; nsplit = s; }
    }
    return nsplit;
}

// the merge of the label parts and the fallback on planes in memory, by mode
void (*const CA_MERGE[3])(CorrOut, CorrOut, int, size_t, const int*, int, unsigned) = {
    corr_argmax_merge_kernel<CaMode::ARGMAX>, corr_argmax_merge_kernel<CaMode::CONF>, corr_argmax_merge_kernel<CaMode::LOSS>};
void (*const CA_FALLBACK[3])(const float*, int, int, int, size_t, const long long*, int, CorrOut) = {
    seg_labels16_kernel<CaMode::ARGMAX>, seg_labels16_kernel<CaMode::CONF>, seg_labels16_kernel<CaMode::LOSS>};

// one launch: the tiles of the map, the panels of the (largest) label set and how they are split into parts of whole panels
struct CaPlan {
    int tiles_y, tiles_x;
    long ntiles;               // over the batch
    int panels, nsplit, split_labels;
    size_t npix;               // output pixels of the batch = values per plane of one part
    unsigned img_pix;          // of one image
};
CaPlan ca_plan(int B, int Kmax, int H, int W, CaMode mode, size_t ws_bytes, int cus) {
    CaPlan p;
    p.tiles_y = (2 * H + CA_LB - 1) / CA_LB;
    p.tiles_x = (2 * W + CA_LB - 1) / CA_LB;
    p.ntiles = (long)B * p.tiles_y * p.tiles_x;
    p.img_pix = (unsigned)(16 * H * W);
    p.npix = (size_t)B * p.img_pix;
    p.panels = (Kmax + CA_P - 1) / CA_P;
    p.nsplit = ca_pick_split(p.panels, p.ntiles, p.npix, ca_part_bytes(mode), ws_bytes > 0, ws_bytes, cus);
    p.split_labels = (p.panels + p.nsplit - 1) / p.nsplit * CA_P;
    return p;
}

// the planes the streamed kernel writes: the caller's when one workgroup per tile streams all labels, else the workspace's, each
// [nsplit][npix] -- the fp32 planes first (score; CONF score2, lse; LOSS lse, tlogit), the int16 planes (label; CONF label2) behind them.
// A part always writes all the planes of its mode
CorrOut ca_part_planes(const CorrOut& out, void* ws, const CaPlan& p, CaMode mode) {
    if (p.nsplit == 1) return out;
    const size_t pn = (size_t)p.nsplit * p.npix;
    float* f = reinterpret_cast<float*>(ws);
    CorrOut w{};
    w.score = f; f += pn;
    if (mode == CaMode::CONF) { w.score2 = f; f += pn; }
    if (mode != CaMode::ARGMAX) { w.lse = f; f += pn; }
    if (mode == CaMode::LOSS) { w.tlogit = f; f += pn; }
    w.label = reinterpret_cast<int16_t*>(f);
    if (mode == CaMode::CONF) w.label2 = w.label + pn;
    return w;
}

// what the streamed kernel reads (offsets: the device prefix sum of a ragged launch; target / ignore_index: LOSS)
struct CaIn { const uint16_t* g; const uint16_t* T; const float* scale; int B, K, H, W; const int* offsets; const long long* target; int ignore_index; };

// the one launch site.  A single part covers all labels (split_labels >= K) and its plane offset is 0: the same arguments serve both forms
template <bool CONF, bool RAGGED, bool LOSS>
void ca_launch(const CaPlan& p, const CaIn& in, const CorrOut& w, hipStream_t st) {
    hipLaunchKernelGGL((corr_argmax_kernel<CONF, RAGGED, LOSS>), dim3((unsigned)(p.ntiles * p.nsplit)), dim3(256), CA_LDS, st, in.g, in.T, in.scale,
                       w.label, w.score, in.B, in.K, in.H, in.W, p.tiles_y, p.tiles_x, p.nsplit, p.split_labels, p.npix, w.label2, w.score2, w.lse,
                       in.offsets, in.target, in.ignore_index, w.tlogit);
}

// the instantiations, listed once: the opt-in to > 64 KB of dynamic LDS walks the list, the dispatch picks from it
struct CaVariant { const void* kernel; void (*launch)(const CaPlan&, const CaIn&, const CorrOut&, hipStream_t); };
template <bool CONF, bool RAGGED, bool LOSS = false>
CaVariant ca_variant() { return {reinterpret_cast<const void*>(corr_argmax_kernel<CONF, RAGGED, LOSS>), ca_launch<CONF, RAGGED, LOSS>}; }
const CaVariant CA_VARIANTS[6] = {ca_variant<false, false>(), ca_variant<true, false>(), ca_variant<false, true>(), ca_variant<true, true>(),
                                  ca_variant<false, false, true>(), ca_variant<false, true, true>()};
const CaVariant& ca_variant_of(CaMode mode, bool ragged) {
    switch (mode) {
        case CaMode::LOSS: return CA_VARIANTS[4 + ragged];
        case CaMode::CONF: return CA_VARIANTS[2 * ragged + 1];
        default: return CA_VARIANTS[2 * ragged];
    }
}

// workgroups of the streaming kernels behind it (the merge, the fallback): grid-stride over npix pixels
int ca_stream_grid(size_t npix) { return (int)std::min<size_t>((npix + 255) / 256, 256 * 16); }

// the sum and the plane read the lse and tlogit planes; the sum writes its partials
bool ca_reduction_ok(const float* lse, const CorrLoss& L) { return !(L.nll || L.nll_plane) || (lse && L.tlogit && (!L.nll || L.partial)); }

// the offsets of a ragged launch travel as kernel arguments, 64 per launch: nothing of the caller's host memory is read after the call returns
struct CaOffsetChunk { int v[64]; };
__global__ __launch_bounds__(64) void corr_argmax_offsets_kernel(int* __restrict__ dst, CaOffsetChunk c, int n) {
    if ((int)threadIdx.x < n) dst[threadIdx.x] = c.v[threadIdx.x];
}

}  // namespace

// the streaming reduction behind both loss forms (nothing to do when neither the sum nor the plane is wanted)
static int launch_corr_loss_reduce(const float* lse, const CorrLoss& L, int K, const int* d_offsets, unsigned img_pix, size_t npix, hipStream_t st) {
    if (!L.nll && !L.nll_plane) return 0;
    size_t chunk;
    int groups;
    cl_plan(npix, chunk, groups);
    hipLaunchKernelGGL(corr_loss_reduce_kernel, dim3(groups), dim3(CL_THREADS), 0, st, lse, (const float*)L.tlogit,
                       reinterpret_cast<const long long*>(L.target), L.ignore_index, K, d_offsets, img_pix, npix, chunk, L.nll_plane,
                       L.nll ? L.partial : (double*)nullptr);
    LSEG_HIP_TRY(hipGetLastError());
    if (L.nll) {
        hipLaunchKernelGGL(corr_loss_fold_kernel, dim3(1), dim3(64), 0, st, (const double*)L.partial, groups, L.nll);
        LSEG_HIP_TRY(hipGetLastError());
    }
    return 0;
}

// the counts of a ragged launch -> their prefix sum (B + 1 entries) and the largest; LSEG_ERR_INVALID for a count outside [1, 32767]
static int ca_ragged_prefix(const int32_t* host_counts, int B, std::vector<int>& prefix, int& kmax) {
    if (!host_counts) return set_error(LSEG_ERR_INVALID, "corr_argmax_ragged: NULL counts");
    if (B < 1) return set_error(LSEG_ERR_INVALID, "corr_argmax_ragged: B=%d", B);
    prefix.assign((size_t)B + 1, 0);
    long total = 0;
    kmax = 0;
    for (int b = 0; b < B; ++b) {
        const int k = host_counts[b];
        if (k < 1 || k > 32767) return set_error(LSEG_ERR_INVALID, "corr_argmax_ragged: image %d has %d labels, outside [1, 32767]", b, k);
        total += k;
        // the kernel's row origins are int32 and T + row * 512 must stay a valid 2^31-row table
        if (total > 0x7fffffffL) return set_error(LSEG_ERR_UNSUPPORTED, "corr_argmax_ragged: %ld text rows exceed the kernel's 32-bit row offsets", total);
        prefix[b + 1] = (int)total;
        kmax = k > kmax ? k : kmax;
    }
    return 0;
}

// The streamed route, every form of it.  g: padded NHWC fp16 [B, H+2, W+2, 512]; T: fp16 [K, 512]; scale: fp32 [B, 2H, 2W].
// out: label int16 [B, 4H, 4W] and, each optional, score fp32 / label2 int16 / score2 fp32 / lse fp32 of that shape.  The mode follows from
// what is asked for: `loss` = the LOSS instantiation (no runner-up; out.tlogit is taken from loss->tlogit), else any of label2 / score2 /
// lse = CONF, else the arg-max.
// loss (optional): tlogit / nll_plane fp32 [B, 4H, 4W], nll double [2], each optional; the sum and the plane read lse and tlogit, so both
// must be given with either, and the sum needs `partial` (corr_loss_plan's bytes)
// ws (optional, ws_bytes): with ca_part_bytes(mode) x B x 16 H W bytes per part the labels of a tile are split over up to 8 workgroups
// (whole panels each, planes as ca_part_planes lays them out) and merged afterwards -- a 120 x 120 map has only 81 tiles per image for
// 256 CUs; without it one workgroup per tile streams all K
// host_counts / d_offsets (both or neither): ragged per-image label sets -- image b against host_counts[b] consecutive rows of T, labels
// local to its own list.  host_counts int32 [B] on the HOST is validated here, before anything is launched; its prefix sum is written
// to d_offsets (device, int32 [B + 1]) on the stream once every check has passed.  K is unused: the LARGEST count sizes the label parts
int launch_corr_argmax(const void* g, const void* T, const float* scale, const CorrOut& out_, int B, int K, int H, int W, int C, hipStream_t st,
                       void* ws, size_t ws_bytes, const CorrLoss* loss, const int32_t* host_counts, int* d_offsets) {
    const bool ragged = host_counts != nullptr;
    CorrOut out = out_;
    out.tlogit = loss ? loss->tlogit : nullptr;
    const CaMode mode = ca_mode(out, loss);
    std::vector<int> prefix;
    if (ragged) {
        const char* who = loss ? "corr_argmax_loss" : "corr_argmax_ragged";
        if (!g || !T || !scale || !out.label || !d_offsets) return set_error(LSEG_ERR_INVALID, "%s: NULL pointer", who);
        if (C != CA_C) return set_error(LSEG_ERR_UNSUPPORTED, "%s: C=%d (C must be 512)", who, C);
        if (const int r = ca_ragged_prefix(host_counts, B, prefix, K)) return r;
    }
    if (!g || !T || !scale || !out.label) return set_error(LSEG_ERR_INVALID, "corr_argmax: NULL pointer");
    if (loss) {
        if (!loss->target) return set_error(LSEG_ERR_INVALID, "corr_argmax_loss: NULL target");
        if (out.label2 || out.score2) return set_error(LSEG_ERR_INVALID, "corr_argmax_loss: the loss form keeps no runner-up");
        if (!ca_reduction_ok(out.lse, *loss))
            return set_error(LSEG_ERR_INVALID, "corr_argmax_loss: the reduction reads the lse and tlogit planes and writes its partials");
        if (((uintptr_t)loss->target | (uintptr_t)loss->nll | (uintptr_t)loss->partial) & 7)
            return set_error(LSEG_ERR_INVALID, "corr_argmax_loss: target / nll / partials must be 8-byte aligned");
    }
    if (K > 32767) return set_error(LSEG_ERR_UNSUPPORTED, "corr_argmax: int16 labels need K <= 32767 (K=%d)", K);
    if (!corr_argmax_supported(K, C)) return set_error(LSEG_ERR_UNSUPPORTED, "corr_argmax: K=%d C=%d (C must be 512, K >= 1)", K, C);
    if (B < 1 || H < 2 || W < 2) return set_error(LSEG_ERR_INVALID, "corr_argmax: B=%d H=%d W=%d", B, H, W);
    // (there are fewer tiles than base pixels, ceil(2H / 28) <= H: the bound on the output pixels keeps their number far below 2^31 too)
    if ((size_t)B * (H + 2) * (W + 2) * CA_C * 2 >= ((size_t)1 << 32) || (size_t)B * 16 * H * W >= ((size_t)1 << 31))
        return set_error(LSEG_ERR_UNSUPPORTED, "corr_argmax: B=%d %dx%d exceeds the kernel's 32-bit offsets", B, H, W);
    if (!ca_tiles_fit(H, 2 * H, 4 * H, CA_OMAX_Y) || !ca_tiles_fit(W, 2 * W, 4 * W, CA_OMAX_X))
        return set_error(LSEG_ERR_UNSUPPORTED, "corr_argmax: %dx%d: a tile's footprint exceeds %dx%d base pixels", H, W, CA_BT, CA_BT);
    int dev = 0;
    LSEG_HIP_TRY(hipGetDevice(&dev));
    static std::atomic<unsigned long long> attr_done{0};             // per-device opt-in to > 64 KB of dynamic LDS (cf. corr.hip)
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(attr_done.load(std::memory_order_acquire) & bit)) {
        for (const CaVariant& v : CA_VARIANTS) LSEG_HIP_TRY(hipFuncSetAttribute(v.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr_done.fetch_or(bit, std::memory_order_release);
    }
    const CaPlan p = ca_plan(B, K, H, W, mode, ws ? ws_bytes : 0, device_cu_count(dev) > 0 ? device_cu_count(dev) : 1);
    if (ragged) {
        for (int i0 = 0; i0 <= B; i0 += 64) {
            CaOffsetChunk ch;
            const int n = std::min(64, B + 1 - i0);
            for (int i = 0; i < 64; ++i) ch.v[i] = i < n ? prefix[i0 + i] : 0;
            hipLaunchKernelGGL(corr_argmax_offsets_kernel, dim3(1), dim3(64), 0, st, d_offsets + i0, ch, n);
            LSEG_HIP_TRY(hipGetLastError());
        }
    }
    const int* offsets = ragged ? d_offsets : nullptr;
    const CaIn in{(const uint16_t*)g, (const uint16_t*)T, scale, B, K, H, W, offsets, loss ? reinterpret_cast<const long long*>(loss->target) : nullptr,
                  loss ? loss->ignore_index : 0};
    const CorrOut w = ca_part_planes(out, ws, p, mode);
    ca_variant_of(mode, ragged).launch(p, in, w, st);
    LSEG_HIP_TRY(hipGetLastError());
    if (p.nsplit > 1) {
        const auto merge = CA_MERGE[(int)mode];
        hipLaunchKernelGGL(merge, dim3(ca_stream_grid(p.npix)), dim3(256), 0, st, w, out, p.nsplit, p.npix, offsets, p.split_labels, p.img_pix);
        LSEG_HIP_TRY(hipGetLastError());
    }
    return loss ? launch_corr_loss_reduce(out.lse, *loss, K, offsets, p.img_pix, p.npix, st) : 0;
}

// the label split a ragged launch of this shape would take, without a device: out2 = {parts, labels per part}.  Part s of image b covers the
// image's labels [s * out2[1], min((s + 1) * out2[1], count_b)) and exists only when that range is not empty.  cus = compute units to plan for
int corr_argmax_ragged_split(const int32_t* host_counts, int B, int H, int W, int conf, size_t ws_bytes, int cus, int* out2) {
    if (!out2) return set_error(LSEG_ERR_INVALID, "corr_argmax_ragged_split: NULL pointer");
    std::vector<int> prefix;
    int kmax = 0;
    if (const int r = ca_ragged_prefix(host_counts, B, prefix, kmax)) return r;
    if (H < 2 || W < 2 || cus < 1) return set_error(LSEG_ERR_INVALID, "corr_argmax_ragged_split: H=%d W=%d cus=%d", H, W, cus);
    const CaPlan p = ca_plan(B, kmax, H, W, conf ? CaMode::CONF : CaMode::ARGMAX, ws_bytes, cus);
    out2[0] = p.nsplit;
    out2[1] = p.split_labels;
    return 0;
}

// the reduction's partial layout for n pixels, host only: out4 = {threads per workgroup, pixels per workgroup, workgroups, bytes of partials}
void corr_loss_plan(size_t npix, int64_t* out4) {
    size_t chunk;
    int groups;
    cl_plan(npix, chunk, groups);
    out4[0] = CL_THREADS; out4[1] = (int64_t)chunk; out4[2] = groups; out4[3] = (int64_t)groups * 2 * (int64_t)sizeof(double);
}

size_t corr_loss_partial_bytes_max() { return (size_t)CL_MAX_GROUPS * 2 * sizeof(double); }

// the caller's one workspace of lseg_op_corr_argmax_loss, in this order, each piece rounded up to 256 bytes: the offsets of a ragged call
// (B + 1 int32), the reduction's partials (when the sum is wanted), an lse and a tlogit plane the caller did not pass while asking for
// the sum or the plane (fp32 [B, 4H, 4W] each), and behind them `parts` label parts of the LOSS mode (ca_part_bytes per output pixel)
static size_t cl_up(size_t v) { return (v + 255) / 256 * 256; }
size_t corr_argmax_loss_ws_bytes(int B, int H, int W, int ragged, int want_nll, int temp_planes, int parts) {
    if (B < 1 || H < 1 || W < 1 || temp_planes < 0 || temp_planes > 2 || parts < 0) return 0;
    const size_t npix = (size_t)B * 16 * H * W;
    int64_t plan[4];
    corr_loss_plan(npix, plan);
    return (ragged ? cl_up(((size_t)B + 1) * 4) : 0) + (want_nll ? cl_up((size_t)plan[3]) : 0) + (size_t)temp_planes * cl_up(npix * 4) +
           (parts > 1 ? (size_t)parts * npix * ca_part_bytes(CaMode::LOSS) : 0);
}

int corr_argmax_loss_op(const void* g, const void* T, const float* scale, const int64_t* target, int ignore_index, const int32_t* host_counts,
                        int B, int K, int H, int W, int C, int16_t* label, float* score, float* lse, float* tlogit, float* nll_plane, double* nll,
                        void* ws, size_t ws_bytes, hipStream_t st) {
    if (!g || !T || !scale || !label || !target) return set_error(LSEG_ERR_INVALID, "corr_argmax_loss: NULL pointer");
    if (B < 1 || H < 2 || W < 2) return set_error(LSEG_ERR_INVALID, "corr_argmax_loss: B=%d H=%d W=%d", B, H, W);
    if ((size_t)B * 16 * H * W >= ((size_t)1 << 31)) return set_error(LSEG_ERR_UNSUPPORTED, "corr_argmax_loss: B=%d %dx%d exceeds the kernel's 32-bit offsets", B, H, W);
    const bool red = nll || nll_plane;
    const int temps = red ? (lse ? 0 : 1) + (tlogit ? 0 : 1) : 0;
    const size_t head = corr_argmax_loss_ws_bytes(B, H, W, host_counts != nullptr, nll != nullptr, temps, 0);
    if (head && (!ws || ws_bytes < head || ((uintptr_t)ws & 7)))
        return set_error(LSEG_ERR_INVALID, "corr_argmax_loss: this call needs an 8-byte aligned workspace of at least %zu bytes "
                                           "(lseg_op_corr_argmax_loss_ws_bytes), got %zu", head, ws ? ws_bytes : (size_t)0);
    const size_t npix = (size_t)B * 16 * H * W;
    char* p = static_cast<char*>(ws);
    auto take = [&](size_t bytes) { char* q = p; p += cl_up(bytes); return q; };
    int* d_offsets = host_counts ? reinterpret_cast<int*>(take(((size_t)B + 1) * 4)) : nullptr;
    int64_t plan[4];
    corr_loss_plan(npix, plan);
    CorrLoss L{target, ignore_index, tlogit, nll_plane, nll, nll ? reinterpret_cast<double*>(take((size_t)plan[3])) : nullptr};
    if (red && !lse) lse = reinterpret_cast<float*>(take(npix * 4));
    if (red && !tlogit) L.tlogit = reinterpret_cast<float*>(take(npix * 4));
    const size_t rest = ws ? ws_bytes - head : 0;
    return launch_corr_argmax(g, T, scale, CorrOut{label, score, nullptr, nullptr, lse}, B, K, H, W, C, st, rest ? p : nullptr, rest, &L, host_counts,
                              d_offsets);
}

// The fallback on planes in memory, the streamed route's outputs in its three modes (chosen as there): low fp32 [B, K, h, w] = the
// (2h, 2w) logits of the engine -> out's planes [B, 2h, 2w]; loss as launch_corr_argmax (one label set of K planes per image: a fixed
// number of labels per image is K of them with targets in [0, K))
int launch_seg_labels16(const float* low, int B, int K, int h, int w, const CorrOut& out_, const CorrLoss* loss, hipStream_t st) {
    CorrOut out = out_;
    out.tlogit = loss ? loss->tlogit : nullptr;
    const CaMode mode = ca_mode(out, loss);
    const char* who = mode == CaMode::LOSS ? "seg_loss16" : mode == CaMode::CONF ? "seg_conf16" : "seg_argmax16";
    if (!low || !out.label || (loss && !loss->target)) return set_error(LSEG_ERR_INVALID, "%s: NULL pointer", who);
    if (K < 1 || K > 32767) return set_error(LSEG_ERR_UNSUPPORTED, "%s: int16 labels need 1 <= K <= 32767 (K=%d)", who, K);
    if (B < 1 || h < 2 || w < 2) return set_error(LSEG_ERR_INVALID, "%s: B=%d h=%d w=%d", who, B, h, w);
    if (loss && !ca_reduction_ok(out.lse, *loss))
        return set_error(LSEG_ERR_INVALID, "%s: the reduction reads the lse and tlogit planes and writes its partials", who);
    const size_t npix = (size_t)B * 4 * h * w;
    const auto kernel = CA_FALLBACK[(int)mode];
    hipLaunchKernelGGL(kernel, dim3(ca_stream_grid(npix)), dim3(256), 0, st, low, K, h, w, npix,
                       loss ? reinterpret_cast<const long long*>(loss->target) : nullptr, loss ? loss->ignore_index : 0, out);
    LSEG_HIP_TRY(hipGetLastError());
    return loss ? launch_corr_loss_reduce(out.lse, *loss, K, nullptr, (unsigned)(4 * h * w), npix, st) : 0;
}

}  // namespace lseg
