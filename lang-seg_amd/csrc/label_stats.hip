// label_stats.hip -- segmentation statistics and the cross-entropy value WITHOUT the [B,K,H,W] score planes: what seg_stats_kernel
// (elementwise.hip) computes from the scores, computed from what the logit-free routes leave behind.
//   label_stats_kernel<false>   the counters of a LABEL MAP int16 [B,H,W] against the int64 target: {correct, labeled, area_inter[],
//                               area_pred[], area_lab[]} in seg_stats' layout, for one label set shared by the batch (K <= 32767), for
//                               ragged per-image lists (labels and targets local to the image's own list, areas indexed offsets[b] + l)
//                               and for ragged lists mapped into one vocabulary (class_map[offsets[b] + l] in [0, nclass))
//   stats_fold_lowres_kernel    one PANEL of low-resolution logits [B,rows,h,w] folded into the per-pixel state (label, best, sum of
//                               exp(v - best), the target's logit) of the [B,2h,2w] grid, read through output_conv's x2 bilinear on the
//                               fly (src_tap / bilerp: the bits lseg_op_upsample2x_planes writes)
//   label_stats_kernel<true>    the same counters from the state's label plane plus the NLL sum best + log(sum) - tlogit over the valid
//                               pixels: per-workgroup {sum, pixels} partials, folded in ascending order by stats_nll_fold_kernel
// The pixel rule (label l, target t, label range k of the image), shared by both instantiations:
//   t == -1 or t == ignore_index          unlabeled: nothing counts
//   t < 0 otherwise                       flags[0]; nothing counts (seg_stats: target + 1 <= 0)
//   l outside [0, k)                      flags[1]; nothing counts (there is no bin for such a prediction)
//   otherwise labeled++, area_pred[l]++ and
//     t >= k                              flags[0]; in no area_lab and no intersection (seg_stats counts such a pixel the same way)
//     t <  k                              area_lab[t]++, and correct++ / area_inter[l]++ when l == t (mapped: when the class ids agree)
// With ignore_index = -1 (or any target that holds no ignore_index) this is seg_stats_kernel's rule, so the counters equal
// lseg_op_seg_stats of any scores whose first-maximum arg-max is the label map -- integers, hence exactly.
// A lane owns runs of four consecutive pixels in the frame of the label plane's 8-byte words: one 8-byte label load, the targets as two
// 16-byte loads where that address is 16-byte aligned (four 8-byte loads otherwise); the up to three pixels before the first whole run
// and after the last are read element by element.  A workgroup never mixes images; an image spans `bpi` workgroups.
// Areas: LS_LDS_BUDGET = 48 KiB of LDS per workgroup for the three histograms (3 x bins x 4 bytes: bins <= 4096, the cap seg_stats has;
// three such workgroups still fit a compute unit's 160 KiB, and the launch asks only for what its bins need, so small label sets keep
// full occupancy), flushed with one 64-bit global atomic per non-zero bin; above the budget every area update is a 64-bit global atomic
// of its own.  Consecutive pixels of a lane that hit the same bin are merged first (a mask is piecewise constant).  Integer sums are
// exact in any order.
#include <algorithm>

#include "ops.h"
#include "../../include/lseg_hip.h"

namespace lseg {
namespace {

constexpr int LS_THREADS = 256, LS_WAVES = LS_THREADS / 64;
constexpr int LS_LDS_BUDGET = 48 * 1024;
constexpr int LS_LDS_BINS = LS_LDS_BUDGET / 12;           // 4096
constexpr int LS_NSCALAR = 5;                             // correct, labeled, flags[0], flags[1], flags[2] (finish: target never covered)

typedef short ls_i16x4 __attribute__((ext_vector_type(4)));

struct LsArgs {
    const int16_t* label;
    const long long* target;
    const int* offsets;          // [B + 1] or NULL
    const int* class_map;        // [offsets[B]] or NULL
    unsigned long long* counts;
    unsigned long long* flags;   // [2] ([3] for the finish form)
    int HW, bpi, K, nclass, ignore_index, use_lds, nb_local;
    // finish form
    const float* best;
    const float* sum;
    const float* tlogit;
    double* ws;
};

__global__ void label_stats_clear_kernel(unsigned long long* __restrict__ counts, unsigned long long* __restrict__ flags,
                                         const int* __restrict__ offsets, int B, int nb_host, int nflags) {
    const long long nb = offsets ? (long long)offsets[B] : (long long)nb_host;
    const long long n = 2 + 3 * std::max<long long>(nb, 0);
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) counts[i] = 0;
    if (blockIdx.x == 0 && (int)threadIdx.x < nflags) flags[threadIdx.x] = 0;
}

template <bool NLL>
__global__ __launch_bounds__(LS_THREADS) void label_stats_kernel(const LsArgs a) {
    extern __shared__ unsigned int hist[];                // [3][nb_local] on the LDS route
    __shared__ unsigned int sc[LS_NSCALAR];
    __shared__ double wloss[LS_WAVES];
    __shared__ unsigned int wvalid[LS_WAVES];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / a.bpi, j = blockIdx.x - b * a.bpi;
    const int nb_local = a.nb_local;
    if (a.use_lds)
        for (int i = tid; i < 3 * nb_local; i += LS_THREADS) hist[i] = 0;
    if (tid < LS_NSCALAR) sc[tid] = 0;
    __syncthreads();

    // the image's label range, the offset of its bins inside an area array, and that array's length
    int k = a.K, base = 0;
    long long nb_total = a.K;
    const int* map = nullptr;
    if (a.offsets) {
        const int o0 = a.offsets[b], o1 = a.offsets[b + 1];
        k = o0 >= 0 && o1 > o0 ? std::min(o1 - o0, a.K) : 0;
        base = o0;
        nb_total = a.offsets[gridDim.x / a.bpi];
        if (a.class_map) { map = a.class_map + o0; base = 0; nb_total = a.nclass; }
    }
    unsigned long long* const areas = a.counts + 2;
    const int nclass = a.nclass, ignore_index = a.ignore_index;

    // consecutive hits of one bin by this lane travel as one update
    int pbin[3] = {-1, -1, -1};
    unsigned int pn[3] = {0, 0, 0};
    auto flush = [&](int arr) {
        if (!pn[arr]) return;
        if (a.use_lds) {
            atomicAdd(&hist[arr * nb_local + pbin[arr]], pn[arr]);
        } else {
            const long long g = (long long)base + pbin[arr];
            if (g >= 0 && g < nb_total) atomicAdd(&areas[arr * nb_total + g], (unsigned long long)pn[arr]);
        }
        pn[arr] = 0;
    };
    auto bump = [&](int arr, int bin) {
        if (bin != pbin[arr]) { flush(arr); pbin[arr] = bin; }
        ++pn[arr];
    };
    // the bin of label l of this image inside an area array (local frame), -1 = no bin (a class id outside [0, nclass))
    auto bin_of = [&](int l) -> int {
        if (!map) return l;
        const int id = map[l];
        return id >= 0 && id < nclass ? id : -1;
    };
    unsigned int c_correct = 0, c_labeled = 0, c_f0 = 0, c_f1 = 0, c_f2 = 0, nvalid = 0;
    double loss = 0.0;

    auto pixel = [&](int l, long long t) {
        if (t == -1 || t == (long long)ignore_index) return;
        if (t < 0) { ++c_f0; return; }
        if (l < 0 || l >= k) { ++c_f1; return; }
        ++c_labeled;
        const int pb = bin_of(l);
        if (pb >= 0) bump(1, pb);
        if (t >= k) { ++c_f0; return; }
        const int tb = bin_of((int)t);
        if (tb >= 0) bump(2, tb);
        if (map ? (pb >= 0 && pb == tb) : l == (int)t) { ++c_correct; bump(0, pb); }
    };
    auto pixel_nll = [&](long long t, float bestv, float sumv, float tl) {
        if (t == (long long)ignore_index || t < 0 || t >= a.K) return;
        if (tl != tl) { ++c_f2; return; }                  // the target's label was in no panel the caller folded
        loss += (double)(bestv + __logf(sumv) - tl);
        ++nvalid;
    };

    const int HW = a.HW;
    const int16_t* lb = a.label + (size_t)b * HW;
    const long long* tg = a.target + (size_t)b * HW;
    const float* pb_ = NLL ? a.best + (size_t)b * HW : nullptr;
    const float* ps_ = NLL ? a.sum + (size_t)b * HW : nullptr;
    const float* pt_ = NLL ? a.tlogit + (size_t)b * HW : nullptr;
    // `head` pixels up to the label plane's first 8-byte boundary, then whole runs of four, then the pixels left
    const int head = std::min(HW, (int)(((8 - (reinterpret_cast<uintptr_t>(lb) & 7)) & 7) >> 1));
    const int nrun = (HW - head) >> 2;
    const int tail0 = head + 4 * nrun;
    for (int q = j * LS_THREADS + tid; q < nrun; q += a.bpi * LS_THREADS) {
        const int p = head + 4 * q;
        const ls_i16x4 l4 = *reinterpret_cast<const ls_i16x4*>(lb + p);
        long long t4[4];
        if ((reinterpret_cast<uintptr_t>(tg + p) & 15) == 0) {
            const longlong2 t01 = *reinterpret_cast<const longlong2*>(tg + p), t23 = *reinterpret_cast<const longlong2*>(tg + p + 2);
            t4[0] = t01.x; t4[1] = t01.y; t4[2] = t23.x; t4[3] = t23.y;
        } else {                                          // 8 bytes off: the middle pair is aligned
            const longlong2 t12 = *reinterpret_cast<const longlong2*>(tg + p + 1);
            t4[0] = tg[p]; t4[1] = t12.x; t4[2] = t12.y; t4[3] = tg[p + 3];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) pixel((int)l4[e], t4[e]);
        if (NLL) {
            float b4[4], s4[4], g4[4];
            const float* src[3] = {pb_ + p, ps_ + p, pt_ + p};
            float* dst[3] = {b4, s4, g4};
#pragma unroll
            for (int v = 0; v < 3; ++v) {
                if ((reinterpret_cast<uintptr_t>(src[v]) & 15) == 0) {
                    const f32x4_t x = *reinterpret_cast<const f32x4_t*>(src[v]);
                    dst[v][0] = x[0]; dst[v][1] = x[1]; dst[v][2] = x[2]; dst[v][3] = x[3];
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) dst[v][e] = src[v][e];
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) pixel_nll(t4[e], b4[e], s4[e], g4[e]);
        }
    }
    if (j == 0 && tid < head + (HW - tail0)) {            // at most six pixels
        const int p = tid < head ? tid : tail0 + (tid - head);
        const long long t = tg[p];
        pixel((int)lb[p], t);
        if (NLL) pixel_nll(t, pb_[p], ps_[p], pt_[p]);
    }
    flush(0); flush(1); flush(2);

    // wave reduction by shuffles, then LDS: integer atomics for the counters, a fixed-order sum of the wave totals for the loss
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        c_correct += __shfl_down(c_correct, off, 64);
        c_labeled += __shfl_down(c_labeled, off, 64);
        c_f0 += __shfl_down(c_f0, off, 64);
        c_f1 += __shfl_down(c_f1, off, 64);
        if (NLL) {
            c_f2 += __shfl_down(c_f2, off, 64);
            nvalid += __shfl_down(nvalid, off, 64);
            loss += __shfl_down(loss, off, 64);
        }
    }
    if ((tid & 63) == 0) {
        if (c_correct) atomicAdd(&sc[0], c_correct);
        if (c_labeled) atomicAdd(&sc[1], c_labeled);
        if (c_f0) atomicAdd(&sc[2], c_f0);
        if (c_f1) atomicAdd(&sc[3], c_f1);
        if (NLL) {
            if (c_f2) atomicAdd(&sc[4], c_f2);
            wloss[tid >> 6] = loss;
            wvalid[tid >> 6] = nvalid;
        }
    }
    __syncthreads();
    if (tid < 2) {
        if (sc[tid]) atomicAdd(&a.counts[tid], (unsigned long long)sc[tid]);
    } else if (tid < (NLL ? 5 : 4)) {
        if (sc[tid]) atomicAdd(&a.flags[tid - 2], (unsigned long long)sc[tid]);
    } else if (NLL && tid == 5) {
        double s = wloss[0];
        unsigned int n = wvalid[0];
#pragma unroll
        for (int i = 1; i < LS_WAVES; ++i) { s += wloss[i]; n += wvalid[i]; }
        a.ws[2 * (size_t)blockIdx.x] = s;
        a.ws[2 * (size_t)blockIdx.x + 1] = (double)n;
    }
    if (a.use_lds) {
        for (int i = tid; i < 3 * nb_local; i += LS_THREADS) {
            const unsigned int v = hist[i];
            if (!v) continue;
            const int arr = i / nb_local;
            const long long g = (long long)base + (i - arr * nb_local);
            if (g >= 0 && g < nb_total) atomicAdd(&areas[arr * nb_total + g], (unsigned long long)v);
        }
    }
}

// nll = {sum, pixels}: the workgroups' slots in ascending order, by one lane
__global__ void stats_nll_fold_kernel(const double* __restrict__ ws, double* __restrict__ nll, int n) {
    if (blockIdx.x || threadIdx.x) return;
    double s = 0.0, c = 0.0;
    for (int i = 0; i < n; ++i) { s += ws[2 * i]; c += ws[2 * i + 1]; }
    nll[0] = s;
    nll[1] = c;
}

// ---- one panel of low-resolution logits into the per-pixel state ------------------------------------------------------------------------
// A lane owns two horizontally adjacent pixels of the [2h, 2w] grid (2w is even: a pair never leaves its row, and with bases aligned to
// the pair every state access is one 4- or 8-byte word).  The recurrence is eval_merge_labels_kernel's: strict `>` keeps the first
// maximum (panels arrive in ascending label order), one exponential per value -- exp(-|v - best|) rescales the sum when v is the new
// best and is v's own term otherwise.  tlogit starts as NaN: "no panel has held this pixel's target yet", which the finish kernel counts.
__global__ __launch_bounds__(256) void stats_fold_lowres_kernel(const float* __restrict__ low, int rows, int row0, int h, int w,
                                                                const long long* __restrict__ target, int16_t* __restrict__ label,
                                                                float* __restrict__ best, float* __restrict__ sum,
                                                                float* __restrict__ tlogit, int first, long long npair) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= npair) return;
    const int Wo = 2 * w, Ho = 2 * h, wp = w;               // wp pairs per output row
    const long long rowi = q / wp;
    const int xo = (int)(q - rowi * wp) * 2;
    const int b = (int)(rowi / Ho), yo = (int)(rowi - (long long)b * Ho);
    const float ry = (float)(h - 1) / (float)(Ho - 1), rx = (float)(w - 1) / (float)(Wo - 1);
    int y0, y1, xa0, xa1, xb0, xb1;
    float ly, lxa, lxb;
    src_tap(ry, yo, h, y0, y1, ly);
    src_tap(rx, xo, w, xa0, xa1, lxa);
    src_tap(rx, xo + 1, w, xb0, xb1, lxb);
    const size_t p = (size_t)q * 2;
    const float ninf = -__builtin_huge_valf();
    float bs[2] = {ninf, ninf}, s[2] = {0.f, 0.f}, tl[2] = {__builtin_nanf(""), __builtin_nanf("")};
    int16_t lab[2] = {-1, -1};
    if (!first) {
        const float2 b2 = *reinterpret_cast<const float2*>(best + p), s2 = *reinterpret_cast<const float2*>(sum + p),
                     t2 = *reinterpret_cast<const float2*>(tlogit + p);
        const short2 l2 = *reinterpret_cast<const short2*>(label + p);
        bs[0] = b2.x; bs[1] = b2.y; s[0] = s2.x; s[1] = s2.y; tl[0] = t2.x; tl[1] = t2.y; lab[0] = l2.x; lab[1] = l2.y;
    }
    const long long tg[2] = {target[p], target[p + 1]};
    const size_t plane = (size_t)h * w;
    const float* c = low + (size_t)b * rows * plane;
    const int r0 = y0 * w, r1 = y1 * w;
#pragma unroll 2
    for (int jr = 0; jr < rows; ++jr, c += plane) {
        const float v[2] = {bilerp(c[r0 + xa0], c[r0 + xa1], c[r1 + xa0], c[r1 + xa1], lxa, ly),
                            bilerp(c[r0 + xb0], c[r0 + xb1], c[r1 + xb0], c[r1 + xb1], lxb, ly)};
        const int kk = row0 + jr;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const float ex = __expf(-fabsf(v[e] - bs[e]));
            if (v[e] > bs[e]) {
                s[e] = s[e] * ex + 1.f;
                bs[e] = v[e]; lab[e] = (int16_t)kk;
            } else {
                s[e] += ex;
            }
            if (tg[e] == (long long)kk) tl[e] = v[e];
        }
    }
    *reinterpret_cast<float2*>(best + p) = make_float2(bs[0], bs[1]);
    *reinterpret_cast<float2*>(sum + p) = make_float2(s[0], s[1]);
    *reinterpret_cast<float2*>(tlogit + p) = make_float2(tl[0], tl[1]);
    *reinterpret_cast<short2*>(label + p) = make_short2(lab[0], lab[1]);
}

// workgroups per image: 16384 pixels (sixteen runs per lane) each at least -- more when the LDS histograms are long -- capped so that the
// grid stays near 2 workgroups per compute unit: every workgroup ends by adding its non-zero bins to the SAME 3 x bins words, and with
// thousands of workgroups those same-address atomics cost as much as the pixels (36 maps of 480 x 480 at K = 150: 82.6 us with 8
// workgroups per compute unit and 4096 pixels each, 65.8 us this way -- 1.26 TB/s, still a fifth of the stream rate; what holds the
// rest has not been profiled)
int label_stats_bpi(int B, int HW, int lds_bins) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    const long long per = std::max<long long>(64 * LS_THREADS, 64LL * lds_bins);
    const long long want = ((long long)HW + per - 1) / per;
    const long long cap = std::max<long long>(1, (long long)std::max(device_cu_count(dev), 1) * 2 / B);
    return (int)std::max<long long>(1, std::min(want, cap));
}

int have_device(const char* who) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1) return set_error(LSEG_ERR_NO_DEVICE, "%s: no HIP device visible", who);
    return 0;
}

int check_shape(const char* who, int B, int H, int W, int K) {
    if (B < 1 || H < 1 || W < 1 || K < 1) return set_error(LSEG_ERR_INVALID, "%s: bad shape B=%d %dx%d K=%d", who, B, H, W, K);
    if (K > 32767) return set_error(LSEG_ERR_UNSUPPORTED, "%s: int16 labels hold K <= 32767 (got %d)", who, K);
    if ((long long)H * W > 0x7fffffffLL) return set_error(LSEG_ERR_UNSUPPORTED, "%s: a %dx%d map is beyond the kernel's 32-bit pixel index", who, H, W);
    return 0;
}

}  // namespace

int label_stats_plan(int bins, int* out2) {
    if (!out2 || bins < 1) return set_error(LSEG_ERR_INVALID, "label_stats_plan: bins=%d, out2=%p", bins, (void*)out2);
    const bool lds = bins <= LS_LDS_BINS;
    out2[0] = lds ? 0 : 1;
    out2[1] = lds ? bins : 0;
    return 0;
}

int launch_label_stats(const int16_t* label, const int64_t* target, int B, int H, int W, int K, int ignore_index, const int32_t* offsets,
                       const int32_t* class_map, int nclass, int64_t* counts, int64_t* flags, int accumulate, hipStream_t st) {
    if (!label || !target || !counts || !flags) return set_error(LSEG_ERR_INVALID, "label_stats: NULL pointer");
    if (class_map && !offsets) return set_error(LSEG_ERR_INVALID, "label_stats: a class map belongs to ragged lists (d_offsets is NULL)");
    if (class_map && nclass < 1) return set_error(LSEG_ERR_INVALID, "label_stats: nclass=%d with a class map", nclass);
    if (int r = check_shape("label_stats", B, H, W, K)) return r;
    if ((reinterpret_cast<uintptr_t>(label) & 1) || (reinterpret_cast<uintptr_t>(target) & 7) || (reinterpret_cast<uintptr_t>(counts) & 7) ||
        (reinterpret_cast<uintptr_t>(flags) & 7) || (reinterpret_cast<uintptr_t>(offsets) & 3) || (reinterpret_cast<uintptr_t>(class_map) & 3))
        return set_error(LSEG_ERR_INVALID, "label_stats: pointers must be aligned to their element");
    if (int r = have_device("label_stats")) return r;
    int plan[2];
    const int bins = class_map ? nclass : K;              // the bins one workgroup can touch
    label_stats_plan(bins, plan);
    LsArgs a{};
    a.label = label; a.target = reinterpret_cast<const long long*>(target); a.offsets = offsets; a.class_map = class_map;
    a.counts = reinterpret_cast<unsigned long long*>(counts); a.flags = reinterpret_cast<unsigned long long*>(flags);
    a.HW = H * W; a.K = K; a.nclass = nclass; a.ignore_index = ignore_index; a.use_lds = plan[0] == 0; a.nb_local = plan[1];
    a.bpi = label_stats_bpi(B, a.HW, plan[1]);
    if ((long long)B * a.bpi > 0x7fffffffLL) return set_error(LSEG_ERR_UNSUPPORTED, "label_stats: B=%d too large", B);
    if (!accumulate) {
        hipLaunchKernelGGL(label_stats_clear_kernel, dim3(64), dim3(256), 0, st, a.counts, a.flags, class_map ? nullptr : offsets, B, bins, 2);
        LSEG_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(label_stats_kernel<false>, dim3(B * a.bpi), dim3(LS_THREADS), (size_t)3 * plan[1] * sizeof(unsigned int), st, a);
    LSEG_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_stats_fold_lowres(const float* low, int B, int rows, int row0, int h, int w, const int64_t* target, int16_t* label, float* best,
                             float* sum, float* tlogit, int first, hipStream_t st) {
    if (!low || !target || !label || !best || !sum || !tlogit) return set_error(LSEG_ERR_INVALID, "stats_fold_lowres: NULL pointer");
    if (B < 1 || rows < 1 || row0 < 0 || h < 2 || w < 2)
        return set_error(LSEG_ERR_INVALID, "stats_fold_lowres: bad shape B=%d rows=%d row0=%d %dx%d (h, w >= 2)", B, rows, row0, h, w);
    if ((long long)row0 + rows > 32767)
        return set_error(LSEG_ERR_UNSUPPORTED, "stats_fold_lowres: int16 labels need row0 + rows <= 32767 (%d + %d)", row0, rows);
    const long long npair = (long long)B * 2 * h * w;     // B x 2h rows x w pairs
    const long long blocks = (npair + 255) / 256;
    if (blocks > 0x7fffffffLL || (long long)rows * h * w > 0x7fffffffLL) return set_error(LSEG_ERR_UNSUPPORTED, "stats_fold_lowres: too many pixels");
    if ((reinterpret_cast<uintptr_t>(low) & 3) || (reinterpret_cast<uintptr_t>(target) & 7) || (reinterpret_cast<uintptr_t>(label) & 3) ||
        ((reinterpret_cast<uintptr_t>(best) | reinterpret_cast<uintptr_t>(sum) | reinterpret_cast<uintptr_t>(tlogit)) & 7))
        return set_error(LSEG_ERR_INVALID, "stats_fold_lowres: the state planes must be aligned to a pixel pair (label 4 bytes, best / sum / tlogit 8)");
    if (int r = have_device("stats_fold_lowres")) return r;
    hipLaunchKernelGGL(stats_fold_lowres_kernel, dim3((unsigned)blocks), dim3(256), 0, st, low, rows, row0, h, w,
                       reinterpret_cast<const long long*>(target), label, best, sum, tlogit, first ? 1 : 0, npair);
    LSEG_HIP_TRY(hipGetLastError());
    return 0;
}

size_t stats_finish_ws_bytes(int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1 || (long long)H * W > 0x7fffffffLL) return 0;
    // sized for the most workgroups any K takes (the LDS bins only ever lower the count)
    return (size_t)B * label_stats_bpi(B, H * W, 0) * 2 * sizeof(double);
}

int launch_stats_finish(const int16_t* label, const float* best, const float* sum, const float* tlogit, const int64_t* target, int B, int H,
                        int W, int K, int ignore_index, int64_t* counts, double* nll, int64_t* flags, void* ws, size_t ws_bytes,
                        hipStream_t st) {
    if (!label || !best || !sum || !tlogit || !target || !counts || !nll || !flags || !ws)
        return set_error(LSEG_ERR_INVALID, "stats_finish: NULL pointer");
    if (int r = check_shape("stats_finish", B, H, W, K)) return r;
    if ((reinterpret_cast<uintptr_t>(label) & 1) || ((reinterpret_cast<uintptr_t>(best) | reinterpret_cast<uintptr_t>(sum) |
        reinterpret_cast<uintptr_t>(tlogit)) & 3) || ((reinterpret_cast<uintptr_t>(target) | reinterpret_cast<uintptr_t>(counts) |
        reinterpret_cast<uintptr_t>(nll) | reinterpret_cast<uintptr_t>(flags) | reinterpret_cast<uintptr_t>(ws)) & 7))
        return set_error(LSEG_ERR_INVALID, "stats_finish: pointers must be aligned to their element");
    if (int r = have_device("stats_finish")) return r;
    int plan[2];
    label_stats_plan(K, plan);
    LsArgs a{};
    a.label = label; a.target = reinterpret_cast<const long long*>(target);
    a.counts = reinterpret_cast<unsigned long long*>(counts); a.flags = reinterpret_cast<unsigned long long*>(flags);
    a.HW = H * W; a.K = K; a.ignore_index = ignore_index; a.use_lds = plan[0] == 0; a.nb_local = plan[1];
    a.best = best; a.sum = sum; a.tlogit = tlogit; a.ws = static_cast<double*>(ws);
    a.bpi = label_stats_bpi(B, a.HW, plan[1]);
    const size_t need = (size_t)B * a.bpi * 2 * sizeof(double);
    if (ws_bytes < need) return set_error(LSEG_ERR_INVALID, "stats_finish: workspace of %zu bytes, %zu needed (lseg_op_stats_finish_ws_bytes)", ws_bytes, need);
    if ((long long)B * a.bpi > 0x7fffffffLL) return set_error(LSEG_ERR_UNSUPPORTED, "stats_finish: B=%d too large", B);
    hipLaunchKernelGGL(label_stats_clear_kernel, dim3(64), dim3(256), 0, st, a.counts, a.flags, (const int*)nullptr, B, K, 3);
    LSEG_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(label_stats_kernel<true>, dim3(B * a.bpi), dim3(LS_THREADS), (size_t)3 * plan[1] * sizeof(unsigned int), st, a);
    LSEG_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(stats_nll_fold_kernel, dim3(1), dim3(64), 0, st, static_cast<const double*>(ws), nll, B * a.bpi);
    LSEG_HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace lseg
