// episode.hip -- the few-shot episode evaluation of the zero-shot networks on the device: what the reference does after
// `out = self(img, class_info)` in test_lseg_zs.py:289-312 and LSegmentationModuleZS.training_step / validation_step
// (modules/lsegmentation_module_zs.py:100-143, 157-192):
//   Evaluator.classify_prediction(out.argmax(1), target, ignore)   fewshot_data/common/evaluation.py:12-39 -- per IMAGE, three
//                                                                   torch.histc calls and one host synchronisation each
//   AverageMeter.update(area_inter, area_union, class_id, loss)     fewshot_data/common/logger.py:29-34 -- index_add_ into [2, nclass]
//   criterion(out, target)                                          nn.CrossEntropyLoss() over the 2 label planes (:338-343)
// One pass over the two label planes of every image -- full-resolution scores [B,2,H,W] (up = 0) or the engine's low-resolution
// logits [B,2,h,w] read through output_conv's x2 bilinear on the fly (up = 1; src_tap / bilerp: bit-identical to the materialised
// logits, as seg_stats_kernel) -- the int64 target and the optional uint8 ignore mask.  Per pixel
//   pred = v1 > v0 (a tie is class 0: torch's first maximum), gt = target, ign = ignore != 0
//   ign: neither pred nor gt counts (the reference turns both into 255, which histc(min=0, max=1) drops)
//   else area_pred[pred]++, and for gt in {0, 1}: area_gt[gt]++, area_inter[pred]++ when pred == gt
//   cross-entropy logsumexp(v0, v1) - v[gt] over gt in {0, 1}, gt != ignore_index (the ignore MASK does not enter: the reference
//   hands `target` to the criterion, not the masked copy)
// A workgroup never mixes images; an image spans `bpi` workgroups.  The integer areas go through LDS and one global atomic per
// non-zero counter and workgroup (exact, so order-free); the meter scatter adds the workgroup's share of inter / union = pred + gt -
// inter (linear in the counters, never negative on any pixel subset) into column class_id[b].  The NLL sum is NOT an atomic: every
// workgroup writes {sum, count} to its own workspace slot and episode_fold_kernel adds the slots of an image in ascending order, so
// two calls on the same input give the same bits.
#include "ops.h"
#include "../../include/lseg_hip.h"

namespace lseg {
namespace {

constexpr int EP_THREADS = 256, EP_WAVES = EP_THREADS / 64;
constexpr int EP_NCNT = 9;      // inter0, inter1, pred0, pred1, gt0, gt1, ign && gt != 0, target outside {0, 1, ignore_index}, CE pixels

struct EpAcc {
    unsigned int c[EP_NCNT];
    double loss;
};

__device__ __forceinline__ void ep_pixel(float v0, float v1, long long gt, bool ign, int ignore_index, EpAcc& a) {
    const int pred = v1 > v0 ? 1 : 0;
    const bool g0 = gt == 0, g1 = gt == 1, gt01 = g0 || g1, on = !ign;
    a.c[0] += on && g0 && !pred;
    a.c[1] += on && g1 && pred;
    a.c[2] += on && !pred;
    a.c[3] += on && pred;
    a.c[4] += on && g0;
    a.c[5] += on && g1;
    a.c[6] += ign && !g0;                                 // the reference asserts there is none (evaluation.py:18)
    if (gt != (long long)ignore_index) {
        if (gt01) {
            // seg_stats_kernel's log-sum-exp at K = 2: the maximum first, one exponential
            const float m = pred ? v1 : v0, o = pred ? v0 : v1;
            const float lse = m + __logf(1.f + __expf(o - m));
            a.loss += (double)(lse - (gt ? v1 : v0));
            ++a.c[8];
        } else {
            ++a.c[7];
        }
    }
}

__global__ __launch_bounds__(EP_THREADS) void episode_stats_kernel(
    const float* __restrict__ scores, const long long* __restrict__ target, const uint8_t* __restrict__ ignore, int HW, int bpi, int up,
    int h, int w, int ignore_index, const long long* __restrict__ class_id, int nclass, unsigned long long* __restrict__ inter_buf,
    unsigned long long* __restrict__ union_buf, unsigned long long* __restrict__ areas, unsigned long long* __restrict__ flags,
    double* __restrict__ ws) {
    __shared__ unsigned int cnt[EP_NCNT];
    __shared__ double wloss[EP_WAVES];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / bpi, j = blockIdx.x - b * bpi;
    if (tid < EP_NCNT) cnt[tid] = 0;
    __syncthreads();

    const long long* tg = target + (size_t)b * HW;
    const uint8_t* ig = ignore ? ignore + (size_t)b * HW : nullptr;
    const size_t plane = up ? (size_t)h * w : (size_t)HW;
    const float* s0 = scores + (size_t)b * 2 * plane;
    const float* s1 = s0 + plane;
    const int Wo = 2 * w;
    const float ry = up ? (float)(h - 1) / (float)(2 * h - 1) : 0.f, rx = up ? (float)(w - 1) / (float)(2 * w - 1) : 0.f;

    EpAcc a;
#pragma unroll
    for (int i = 0; i < EP_NCNT; ++i) a.c[i] = 0;
    a.loss = 0.0;

    auto pixel = [&](int p, long long gt) {
        float v0, v1;
        if (up) {
            const int yo = p / Wo, xo = p - yo * Wo;
            int y0, y1, x0, x1;
            float ly, lx;
            src_tap(ry, yo, h, y0, y1, ly);
            src_tap(rx, xo, w, x0, x1, lx);
            const int o00 = y0 * w + x0, o01 = y0 * w + x1, o10 = y1 * w + x0, o11 = y1 * w + x1;
            v0 = bilerp(s0[o00], s0[o01], s0[o10], s0[o11], lx, ly);
            v1 = bilerp(s1[o00], s1[o01], s1[o10], s1[o11], lx, ly);
        } else {
            v0 = s0[p];
            v1 = s1[p];
        }
        ep_pixel(v0, v1, gt, ig ? ig[p] != 0 : false, ignore_index, a);
    };

    // the image's target row starts at an 8-byte boundary of any parity: `head` pixels up to the first 16-byte boundary, then pairs
    // through one 16-byte load each, then the odd pixel that may be left
    const int head = HW > 0 ? (int)((reinterpret_cast<uintptr_t>(tg) >> 3) & 1) : 0;
    const int npair = (HW - head) >> 1;
    const int tail0 = head + 2 * npair;
    for (int q = j * EP_THREADS + tid; q < npair; q += bpi * EP_THREADS) {
        const int p = head + 2 * q;
        const longlong2 t2 = *reinterpret_cast<const longlong2*>(tg + p);
        pixel(p, t2.x);
        pixel(p + 1, t2.y);
    }
    if (j == 0 && tid < head + (HW - tail0)) {            // at most two pixels
        const int p = tid < head ? tid : tail0 + (tid - head);
        pixel(p, tg[p]);
    }

    // wave reduction by shuffles, then LDS: integer atomics for the counters, a fixed-order sum of the four wave totals for the loss
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int i = 0; i < EP_NCNT; ++i) a.c[i] += __shfl_down(a.c[i], off, 64);
        a.loss += __shfl_down(a.loss, off, 64);
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int i = 0; i < EP_NCNT; ++i)
            if (a.c[i]) atomicAdd(&cnt[i], a.c[i]);
        wloss[tid >> 6] = a.loss;
    }
    __syncthreads();
    if (tid < 6) {
        if (cnt[tid]) atomicAdd(&areas[(size_t)b * 6 + tid], (unsigned long long)cnt[tid]);
    } else if (tid < 8) {
        if (cnt[tid]) atomicAdd(&flags[tid - 6], (unsigned long long)cnt[tid]);
    } else if (tid == 8) {
        double s = wloss[0];
#pragma unroll
        for (int i = 1; i < EP_WAVES; ++i) s += wloss[i];
        ws[2 * (size_t)blockIdx.x] = s;
        ws[2 * (size_t)blockIdx.x + 1] = (double)cnt[8];
    } else if (tid < 11 && inter_buf) {                   // AverageMeter.update's index_add_ (logger.py:30-31), class plane c
        const int c = tid - 9;
        const long long cid = class_id[b];
        if (cid >= 0 && cid < nclass) {                   // the host refused anything else before the launch; never write outside
            const unsigned int in = cnt[c], un = cnt[2 + c] + cnt[4 + c] - cnt[c];
            if (in) atomicAdd(&inter_buf[(size_t)c * nclass + cid], (unsigned long long)in);
            if (un) atomicAdd(&union_buf[(size_t)c * nclass + cid], (unsigned long long)un);
        }
    }
}

// nll[b] = {sum, count} of image b: its bpi workspace slots in ascending order
__global__ void episode_fold_kernel(const double* __restrict__ ws, double* __restrict__ nll, int B, int bpi) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double* p = ws + 2 * (size_t)b * bpi;
    double s = 0.0, n = 0.0;
    for (int j = 0; j < bpi; ++j) { s += p[2 * j]; n += p[2 * j + 1]; }
    nll[2 * (size_t)b] = s;
    nll[2 * (size_t)b + 1] = n;
}

// workgroups per image: 2048 pixels (4 pairs per lane) each, capped so that the grid stays near 8 workgroups per compute unit
int episode_bpi(int B, int HW) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    const long long want = ((long long)HW + 8 * EP_THREADS - 1) / (8 * EP_THREADS);
    const long long cap = std::max<long long>(1, (long long)device_cu_count(dev) * 8 / B);
    return (int)std::max<long long>(1, std::min(want, cap));
}

}  // namespace

size_t episode_stats_ws_bytes(int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1 || (long long)H * W > 0x7fffffffLL) return 0;
    return (size_t)B * episode_bpi(B, H * W) * 2 * sizeof(double);
}

int launch_episode_stats(const float* scores, const int64_t* target, const uint8_t* ignore, int B, int H, int W, int up, int ignore_index,
                         const int64_t* class_id, int nclass, int64_t* inter_buf, int64_t* union_buf, int64_t* areas, double* nll,
                         int64_t* flags, void* ws, size_t ws_bytes, hipStream_t st) {
    if (!scores || !target || !areas || !nll || !flags || !ws) return set_error(LSEG_ERR_INVALID, "episode_stats: NULL pointer");
    if (B < 1 || H < 1 || W < 1 || (long long)H * W > 0x7fffffffLL) return set_error(LSEG_ERR_INVALID, "episode_stats: bad shape B=%d %dx%d", B, H, W);
    if (up && ((H & 1) || (W & 1) || H < 4 || W < 4))
        return set_error(LSEG_ERR_INVALID, "episode_stats: up = 1 reads [B,2,H/2,W/2] logits, H and W must be even and >= 4 (got %dx%d)", H, W);
    if ((reinterpret_cast<uintptr_t>(target) & 7) || (reinterpret_cast<uintptr_t>(ws) & 7))
        return set_error(LSEG_ERR_INVALID, "episode_stats: target / workspace must be 8-byte aligned");
    const bool meter = class_id || inter_buf || union_buf;
    if (meter && (!class_id || !inter_buf || !union_buf || nclass < 1))
        return set_error(LSEG_ERR_INVALID, "episode_stats: the meter scatter needs class_id, inter_buf, union_buf and nclass >= 1 (nclass=%d)", nclass);
    const int HW = H * W, bpi = episode_bpi(B, HW);
    const size_t need = (size_t)B * bpi * 2 * sizeof(double);
    if (ws_bytes < need) return set_error(LSEG_ERR_INVALID, "episode_stats: workspace of %zu bytes, %zu needed (lseg_op_episode_stats_ws_bytes)", ws_bytes, need);
    if ((long long)B * bpi > 0x7fffffffLL) return set_error(LSEG_ERR_INVALID, "episode_stats: B=%d too large", B);
    LSEG_HIP_TRY(hipMemsetAsync(areas, 0, (size_t)B * 6 * sizeof(int64_t), st));
    LSEG_HIP_TRY(hipMemsetAsync(flags, 0, 2 * sizeof(int64_t), st));
    hipLaunchKernelGGL(episode_stats_kernel, dim3(B * bpi), dim3(EP_THREADS), 0, st, scores, reinterpret_cast<const long long*>(target), ignore, HW,
                       bpi, up, H / 2, W / 2, ignore_index, meter ? reinterpret_cast<const long long*>(class_id) : nullptr, nclass,
                       meter ? reinterpret_cast<unsigned long long*>(inter_buf) : nullptr,
                       meter ? reinterpret_cast<unsigned long long*>(union_buf) : nullptr, reinterpret_cast<unsigned long long*>(areas),
                       reinterpret_cast<unsigned long long*>(flags), static_cast<double*>(ws));
    LSEG_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(episode_fold_kernel, dim3((B + 63) / 64), dim3(64), 0, st, static_cast<const double*>(ws), nll, B, bpi);
    LSEG_HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace lseg
