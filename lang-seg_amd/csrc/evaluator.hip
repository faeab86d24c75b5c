// evaluator.hip -- device side of the multi-scale / flip sliding-window evaluator, the direct caller of the forward
// (additional_utils/encoding_models.py:54-155 MultiEvalModule.forward / module_inference / pad_image / crop_image / flip_image,
//  additional_utils/models.py:55-140 LSeg_MultiEvalModule.forward).  The reference does this with one torch op
// per crop (pad per channel, slice, flip, slice-add, count) around 2 x n_crops B = 1 forwards; here every scale is
//   make_crops  : resized image -> the whole stack of padded crops AND their mirrored twins, one pass
//   (the engine runs the stack as one batch)
//   accumulate  : the stack of logits -> count-normalised score map of the scale (flip-add, overlap-add in the reference's box order,
//                 divide, crop to the un-padded size), one pass, no atomics
//   resize_add  : scores (+)= bilinear(map) at the input resolution (also used for the image resize itself)
#include <algorithm>

#include "ops.h"
#include "../../include/lseg_hip.h"

namespace lseg {
namespace {

// crops [(1 + flip) * n, C, crop, crop]; crop k = (idh, idw) starts at (idh * stride, idw * stride) of the (virtually padded) image;
// pixels outside [0, height) x [0, width) take pad[c] = -mean[c] / std[c] (pad_image, :144-155); twin n + k = crop k mirrored in x
__global__ void eval_make_crops_kernel(const float* __restrict__ img, float* __restrict__ crops, int C, int height, int width, int crop,
                                       int stride, int w_grids, int n, int flip, float pad0, float pad1, float pad2) {
    const size_t total = (size_t)(flip ? 2 : 1) * n * C * crop * crop;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % crop);
        size_t p = i / crop;
        const int y = (int)(p % crop); p /= crop;
        const int c = (int)(p % C);
        const int kf = (int)(p / C);
        const int k = kf >= n ? kf - n : kf;
        const int xs = kf >= n ? crop - 1 - x : x;
        const int idh = k / w_grids, idw = k - idh * w_grids;
        const int yy = idh * stride + y, xx = idw * stride + xs;
        const float pv = c == 0 ? pad0 : (c == 1 ? pad1 : pad2);
        crops[i] = (yy < height && xx < width) ? img[((size_t)c * height + yy) * width + xx] : pv;
    }
}

// outputs [K, height, width]: sum over the boxes covering the pixel, in the reference's (idh, idw) order, of
// outs[k] + flip_x(outs[n + k]), divided by the number of covering boxes (encoding_models.py:100-121)
__global__ void eval_accumulate_kernel(const float* __restrict__ outs, float* __restrict__ outputs, int K, int height, int width, int ph, int pw,
                                       int crop, int stride, int h_grids, int w_grids, int flip) {
    const int n = h_grids * w_grids;
    const size_t total = (size_t)K * height * width;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % width);
        const int y = (int)((i / width) % height);
        const int k = (int)(i / ((size_t)width * height));
        float acc = 0.f, cnt = 0.f;
        for (int idh = 0; idh < h_grids; ++idh) {
            const int h0 = idh * stride, h1 = min(h0 + crop, ph);
            if (y < h0 || y >= h1) continue;
            for (int idw = 0; idw < w_grids; ++idw) {
                const int w0 = idw * stride, w1 = min(w0 + crop, pw);
                if (x < w0 || x >= w1) continue;
                const int b = idh * w_grids + idw;
                const size_t o = (((size_t)b * K + k) * crop + (y - h0)) * crop;
                float v = outs[o + (x - w0)];
                if (flip) v += outs[o + (size_t)n * K * crop * crop + (crop - 1 - (x - w0))];
                acc += v;
                cnt += 1.f;
            }
        }
        outputs[i] = acc / cnt;
    }
}

// ---- the run-of-four form of the same sum: eval_accumulate_lowres_kernel (a whole grid, from 0.f, counted and divided) and
// eval_accumulate_window_kernel (a window of the grid, continued from the sum in memory, divided by eval_finalize_kernel).  One wave per
// output row (k, y), four rows per block; a lane produces runs of four consecutive x.  Both add, per pixel, out + flip_x(twin) of the
// covering boxes in ascending (idh, idw) order: the additions of eval_accumulate_kernel, so the same bits.
// The boxes idx of one grid axis covering coordinate c of the map, idx * stride <= c < idx * stride + crop (the clip of the last box to
// the padded size never cuts inside the map):
struct CoverRange { int lo, hi; };
__device__ __forceinline__ CoverRange cover_range(int c, int crop, int stride, int grids) {
    return {c < crop ? 0 : (c - crop) / stride + 1, min(c / stride, grids - 1)};
}

// A row's columns [x_lo, x_hi) as nq runs of four: run q covers x = x_lo + 4 q - shift .. + 3, shifted so that every interior run is
// 16 bytes aligned in memory whatever the width and the map's offset; the row's first / last run may be partial.
__device__ __forceinline__ void run_frame(const float* row, int x_lo, int x_hi, int& shift, int& nq) {
    shift = (int)((reinterpret_cast<uintptr_t>(row + x_lo) >> 2) & 3);
    nq = (x_hi - x_lo + shift + 3) >> 2;
}
// the run at xb: valid[e] = inside [x_lo, x_hi); xs[e] clamped into the row (an invalid element computes a neighbour's value, not stored)
__device__ __forceinline__ void run_columns(int xb, int x_lo, int x_hi, int width, int (&xs)[4], bool (&valid)[4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        valid[e] = xb + e >= x_lo && xb + e < x_hi;
        xs[e] = min(max(xb + e, 0), width - 1);
    }
}
__device__ __forceinline__ bool all4(const bool (&m)[4]) { return m[0] && m[1] && m[2] && m[3]; }
// row[xb + e] = o[e] where m[e]: one 16-byte store when all four (then the run is interior, hence aligned), scalar stores otherwise
__device__ __forceinline__ void store_run(float* row, int xb, const float (&o)[4], const bool (&m)[4]) {
    if (all4(m)) {
        const f32x4_t ov = {o[0], o[1], o[2], o[3]};
        *reinterpret_cast<f32x4_t*>(row + xb) = ov;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (m[e]) row[xb + e] = o[e];
    }
}

__device__ __forceinline__ float pick4(const float (&w)[4], int j) { return j == 0 ? w[0] : (j == 1 ? w[1] : (j == 2 ? w[2] : w[3])); }

// up(plane)[row taps ra / rb, ly][columns xl[0..3]]: xl non-decreasing (rev = 0) or non-increasing (rev = 1), neighbours at most 1 apart.
// The eight taps of the four outputs lie in four consecutive low-resolution columns (r < 1/2: four consecutive outputs advance the left
// tap by at most 2), so two rows x four columns are loaded once and feed all four outputs.
__device__ __forceinline__ void taps4(const float* __restrict__ ra, const float* __restrict__ rb, const int (&xl)[4], float r, int hl, float ly,
                                      int rev, float (&v)[4]) {
    int x0[4], x1[4];
    float lx[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) src_tap(r, xl[e], hl, x0[e], x1[e], lx[e]);
    const int c = rev ? x0[3] : x0[0];                   // the leftmost tap of the run; every other one is in [c, c + 3]
    float wa[4], wb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = min(c + j, hl - 1);
        wa[j] = ra[col];
        wb[j] = rb[col];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
        v[e] = bilerp(pick4(wa, x0[e] - c), pick4(wa, x1[e] - c), pick4(wb, x0[e] - c), pick4(wb, x1[e] - c), lx[e], ly);
}

// the source rows of full-resolution row yb of a box: the row itself, or (LOW: planes of side = crop / 2, the logits the engine holds
// before output_conv) the two taps and weight of output_conv's x2 bilinear -- src_tap / bilerp (common.h), the arithmetic of
// upsample2x_planes_kernel with its ry = rx = r, so a LOW value is the bit pattern the materialised full-resolution plane would hold
template <bool LOW>
__device__ __forceinline__ void row_taps(float r, int yb, int side, int& y0, int& y1, float& ly) {
    y0 = y1 = yb;
    ly = 0.f;
    if (LOW) {
        src_tap(r, yb, side, y0, y1, ly);
        y0 = min(y0, side - 1); y1 = min(y1, side - 1);
    }
}

// One box (plane p [side, side], columns from w0 of the map; its mirrored twin's plane at p + twin) at the run's columns xs: in[e] = valid[e]
// and the box covers xs[e]; v[e] = box + twin there, added before the pair meets the accumulator.  The twin's value is that of the MIRRORED
// full-resolution column crop - 1 - (x - w0) (LOW: the tap of that column; mirroring a value interpolated at x would round differently).
// !LOW: four covered columns are consecutive logits -- one 16-byte load each for box and twin (descending) where the address allows, four
// 4-byte loads otherwise; a run the box covers in part reads element by element.
template <bool LOW>
__device__ __forceinline__ void box_values(const float* __restrict__ p, size_t twin, int y0, int y1, float ly, const int (&xs)[4],
                                           const bool (&valid)[4], int w0, int crop, int side, float r, int flip, bool (&in)[4], float (&v)[4]) {
    int xl[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        in[e] = valid[e] && xs[e] >= w0 && xs[e] < w0 + crop;
        xl[e] = min(max(xs[e] - w0, 0), crop - 1);
        v[e] = 0.f;
    }
    if (LOW) {
        taps4(p + (size_t)y0 * side, p + (size_t)y1 * side, xl, r, side, ly, 0, v);
        if (flip) {
            int xm[4];
            float t[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) xm[e] = crop - 1 - xl[e];
            taps4(p + twin + (size_t)y0 * side, p + twin + (size_t)y1 * side, xm, r, side, ly, 1, t);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += t[e];
        }
        return;
    }
    const float* s = p + (size_t)y0 * crop;
    if (all4(in)) {                                       // xl[e] = xl[0] + e
        const float* a4 = s + xl[0];
        if ((reinterpret_cast<uintptr_t>(a4) & 15) == 0) {
            const f32x4_t t = *reinterpret_cast<const f32x4_t*>(a4);
            v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = a4[e];
        }
        if (flip) {
            const float* m4 = s + twin + (crop - 1 - xl[3]);   // the mirrored columns of e = 3, 2, 1, 0
            if ((reinterpret_cast<uintptr_t>(m4) & 15) == 0) {
                const f32x4_t t = *reinterpret_cast<const f32x4_t*>(m4);
                v[0] += t[3]; v[1] += t[2]; v[2] += t[1]; v[3] += t[0];
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] += m4[3 - e];
            }
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (in[e]) {
                v[e] = s[xl[e]];
                if (flip) v[e] += s[twin + (crop - 1 - xl[e])];
            }
    }
}

// The whole grid of a scale from its low-resolution logits, low [(1 + flip) * n, K, crop / 2, crop / 2]: outputs [K, height, width] =
// sum / count, every in-row element stored.  Bytes read per crop fall 4x against the full-resolution form and stay in L1 / L2 across
// neighbouring runs.
__global__ __launch_bounds__(256) void eval_accumulate_lowres_kernel(const float* __restrict__ low, float* __restrict__ outputs, int K, int height,
                                                                     int width, int crop, int stride, int h_grids, int w_grids, int flip) {
    const int hl = crop >> 1;
    const size_t rows = (size_t)K * height;
    const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const int k = (int)((unsigned)row / (unsigned)height);              // rows < 2^31 (launcher)
    const int y = (int)((unsigned)row - (unsigned)k * (unsigned)height);
    const float r = (float)(hl - 1) / (float)(crop - 1);
    const size_t plane = (size_t)hl * hl;
    const size_t twin = (size_t)h_grids * w_grids * K * plane;
    const CoverRange hc = cover_range(y, crop, stride, h_grids);
    float* orow = outputs + row * (size_t)width;
    const bool every[4] = {true, true, true, true};
    int shift, nq;
    run_frame(orow, 0, width, shift, nq);
    for (int q = lane; q < nq; q += 64) {
        const int xb = 4 * q - shift;
        int xs[4];
        bool valid[4];
        run_columns(xb, 0, width, width, xs, valid);
        const int w_lo = cover_range(xs[0], crop, stride, w_grids).lo, w_hi = cover_range(xs[3], crop, stride, w_grids).hi;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        int cnt[4] = {0, 0, 0, 0};
        for (int idh = hc.lo; idh <= hc.hi; ++idh) {
            int y0, y1;
            float ly;
            row_taps<true>(r, y - idh * stride, hl, y0, y1, ly);
            for (int idw = w_lo; idw <= w_hi; ++idw) {
                bool in[4];
                float v[4];
                box_values<true>(low + ((size_t)(idh * w_grids + idw) * K + k) * plane, twin, y0, y1, ly, xs, every, idw * stride, crop, hl, r,
                                 flip, in, v);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (in[e]) { acc[e] += v[e]; cnt[e] += 1; }
            }
        }
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = acc[e] / (float)cnt[e];
        store_run(orow, xb, o, valid);
    }
}

// A WINDOW of a scale's grid: boxes [first, first + nbox) in (idh, idw) order, outs [(1 + flip) * nbox, K, side, side] holding only their
// logits (LOW: side = crop / 2, else side = crop).  For every map pixel some box of the window covers, sum[k, y, x] += the window's
// covering boxes, so windows submitted in ascending order leave the bits of the one-launch kernels' un-divided acc.  A pixel no box of
// the window covers is neither read nor written.  Rows y_lo .. y_lo + ny - 1 and columns [x_lo, x_hi) are the bounding rectangle of the
// window's boxes on the map (the launcher).
template <bool LOW>
__global__ __launch_bounds__(256) void eval_accumulate_window_kernel(const float* __restrict__ outs, float* __restrict__ sum, int K, int height,
                                                                     int width, int crop, int stride, int w_grids, int flip, int first, int nbox,
                                                                     int y_lo, int ny, int x_lo, int x_hi) {
    const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (size_t)K * ny) return;
    const int lane = threadIdx.x & 63;
    const int k = (int)((unsigned)row / (unsigned)ny);                  // K * ny < 2^31 (launcher)
    const int y = y_lo + (int)((unsigned)row - (unsigned)k * (unsigned)ny);
    const int side = LOW ? crop >> 1 : crop;
    const float r = (float)(side - 1) / (float)(crop - 1);            // LOW only
    const size_t plane = (size_t)side * side;
    const size_t twin = (size_t)nbox * K * plane;
    const int last = first + nbox - 1;
    const int ih_a = first / w_grids, ih_b = last / w_grids;
    const int iw_a = first - ih_a * w_grids, iw_b = last - ih_b * w_grids;
    const CoverRange hc = cover_range(y, crop, stride, ih_b + 1);       // the window's grid rows covering y: from ih_a, up to ih_b
    const int h_lo = max(hc.lo, ih_a), h_hi = hc.hi;
    if (h_lo > h_hi) return;
    float* orow = sum + ((size_t)k * height + y) * (size_t)width;
    int shift, nq;
    run_frame(orow, x_lo, x_hi, shift, nq);
    for (int q = lane; q < nq; q += 64) {
        const int xb = x_lo + 4 * q - shift;
        int xs[4];
        bool valid[4];
        run_columns(xb, x_lo, x_hi, width, xs, valid);
        const int w_lo = cover_range(xs[0], crop, stride, w_grids).lo, w_hi = cover_range(xs[3], crop, stride, w_grids).hi;
        // which of the four pixels the window covers at all: only those touch sum
        bool cov[4] = {false, false, false, false};
        for (int idh = h_lo; idh <= h_hi; ++idh) {
            const int a = max(w_lo, idh == ih_a ? iw_a : 0), b = min(w_hi, idh == ih_b ? iw_b : w_grids - 1);
            for (int idw = a; idw <= b; ++idw) {
                const int w0 = idw * stride;
#pragma unroll
                for (int e = 0; e < 4; ++e) cov[e] = cov[e] || (valid[e] && xs[e] >= w0 && xs[e] < w0 + crop);
            }
        }
        if (!(cov[0] || cov[1] || cov[2] || cov[3])) continue;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        if (all4(cov)) {                                                   // as store_run
            const f32x4_t sv = *reinterpret_cast<const f32x4_t*>(orow + xb);
            acc[0] = sv[0]; acc[1] = sv[1]; acc[2] = sv[2]; acc[3] = sv[3];
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (cov[e]) acc[e] = orow[xb + e];
        }
        for (int idh = h_lo; idh <= h_hi; ++idh) {
            const int a = max(w_lo, idh == ih_a ? iw_a : 0), b = min(w_hi, idh == ih_b ? iw_b : w_grids - 1);
            int y0, y1;
            float ly;
            row_taps<LOW>(r, y - idh * stride, side, y0, y1, ly);
            for (int idw = a; idw <= b; ++idw) {
                bool in[4];
                float v[4];
                box_values<LOW>(outs + ((size_t)(idh * w_grids + idw - first) * K + k) * plane, twin, y0, y1, ly, xs, valid, idw * stride, crop,
                                side, r, flip, in, v);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (in[e]) acc[e] += v[e];
            }
        }
        store_run(orow, xb, acc, cov);
    }
}

// map = sum / (number of boxes of the WHOLE grid covering the pixel): the division of the one-launch kernels (their count as a float).
// Element-wise, so map == sum is fine; 16 bytes per lane where both pointers allow.
__device__ __forceinline__ float eval_cover_count(size_t i, int height, int width, int crop, int stride, int h_grids, int w_grids) {
    const CoverRange hc = cover_range((int)((i / width) % height), crop, stride, h_grids);
    const CoverRange wc = cover_range((int)(i % width), crop, stride, w_grids);
    return (float)((hc.hi - hc.lo + 1) * (wc.hi - wc.lo + 1));
}
__global__ void eval_finalize_kernel(const float* sum, float* map, size_t total, int height, int width, int crop, int stride, int h_grids,
                                     int w_grids, int vec) {
    const size_t n4 = vec ? total / 4 : 0;
    for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < n4; j += (size_t)gridDim.x * blockDim.x) {
        const f32x4_t s = reinterpret_cast<const f32x4_t*>(sum)[j];
        f32x4_t o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = s[e] / eval_cover_count(4 * j + e, height, width, crop, stride, h_grids, w_grids);
        reinterpret_cast<f32x4_t*>(map)[j] = o;
    }
    for (size_t i = 4 * n4 + blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
        map[i] = sum[i] / eval_cover_count(i, height, width, crop, stride, h_grids, w_grids);
}

// dst [P, Ho, Wo] (+)= bilinear(src [P, Hi, Wi]), align_corners=True (F.interpolate / upsample_bilinear2d's arithmetic)
__global__ void eval_resize_kernel(const float* __restrict__ src, float* __restrict__ dst, int P, int Hi, int Wi, int Ho, int Wo, int accumulate) {
    const size_t total = (size_t)P * Ho * Wo;
    const float ry = Ho > 1 ? (float)(Hi - 1) / (float)(Ho - 1) : 0.f, rx = Wo > 1 ? (float)(Wi - 1) / (float)(Wo - 1) : 0.f;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int xo = (int)(i % Wo);
        const int yo = (int)((i / Wo) % Ho);
        const size_t p = i / ((size_t)Wo * Ho);
        int y0, y1, x0, x1;
        float ly, lx;
        src_tap(ry, yo, Hi, y0, y1, ly);
        src_tap(rx, xo, Wi, x0, x1, lx);
        const float* s = src + p * (size_t)Hi * Wi;
        const float v = bilerp(s[(size_t)y0 * Wi + x0], s[(size_t)y0 * Wi + x1], s[(size_t)y1 * Wi + x0], s[(size_t)y1 * Wi + x1], lx, ly);
        dst[i] = accumulate ? dst[i] + v : v;
    }
}

// ---- label panels: fold `rows` score planes [rows, npix] (labels row0 .. row0 + rows - 1, ascending) into the running per-pixel state
// (best, label, runner-up, label2, s = sum of exp(value - best)); the stable descending top-2 of lseg_forward_labels_conf -- strict `>`
// twice, so equal values go to the lower label and a later label equal to the winner is the runner-up -- and its online log-sum-exp whose
// running maximum IS best: one exp per value, exp(-|v - best|) rescales s when v is the new best and is v's own term otherwise (best =
// -inf before the first label: exp(-inf) = 0 and s starts at 1).  HBM-bound: every score is read once, the state once per panel.
// A lane owns one run of four consecutive pixels of the flattened [H, W] map and walks the panel's planes with the state in registers.
// The run frame is the score plane's (run_frame), so its interior runs are 16 bytes aligned; every other array -- and every plane of the
// panel, whose alignment moves with npix -- takes the vector access where ITS address allows and element accesses otherwise.
template <typename V, typename T>
__device__ __forceinline__ void load_run(const T* p, bool full, const bool (&m)[4], T (&o)[4]) {
    if (full && (reinterpret_cast<uintptr_t>(p) & (sizeof(V) - 1)) == 0) {
        const V t = *reinterpret_cast<const V*>(p);
        o[0] = t[0]; o[1] = t[1]; o[2] = t[2]; o[3] = t[3];
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (m[e]) o[e] = p[e];
    }
}
template <typename V, typename T>
__device__ __forceinline__ void store_run_any(T* p, bool full, const bool (&m)[4], const T (&o)[4]) {
    if (full && (reinterpret_cast<uintptr_t>(p) & (sizeof(V) - 1)) == 0) {
        const V t = {o[0], o[1], o[2], o[3]};
        *reinterpret_cast<V*>(p) = t;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (m[e]) p[e] = o[e];
    }
}
typedef short i16x4_t __attribute__((ext_vector_type(4)));

// CONF = false keeps (best, label) only; first: the state is not read; last: sum leaves as the log-sum-exp best + log(s)
template <bool CONF>
__global__ __launch_bounds__(256) void eval_merge_labels_kernel(const float* __restrict__ scores, int rows, int row0, long long npix,
                                                                int16_t* __restrict__ label, float* __restrict__ score,
                                                                int16_t* __restrict__ label2, float* __restrict__ score2,
                                                                float* __restrict__ sum, int first, int last, int shift, long long nq) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= nq) return;
    const long long xb = 4 * q - shift;                   // the run's first pixel; -3 .. -1 for the partial first run
    bool m[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) m[e] = xb + e >= 0 && xb + e < npix;
    const bool full = all4(m);
    const float ninf = -__builtin_huge_valf();
    float best[4] = {ninf, ninf, ninf, ninf}, sec[4] = {ninf, ninf, ninf, ninf}, s[4] = {0.f, 0.f, 0.f, 0.f};
    int16_t lab[4] = {-1, -1, -1, -1}, lab2[4] = {-1, -1, -1, -1};
    if (!first) {
        load_run<f32x4_t>(score + xb, full, m, best);
        load_run<i16x4_t>(label + xb, full, m, lab);
        if (CONF) {
            if (score2) load_run<f32x4_t>(score2 + xb, full, m, sec);
            if (label2) load_run<i16x4_t>(label2 + xb, full, m, lab2);
            if (sum) load_run<f32x4_t>(sum + xb, full, m, s);
        }
    }
    const float* p = scores + xb;
#pragma unroll 4
    for (int j = 0; j < rows; ++j, p += npix) {
        float v[4] = {ninf, ninf, ninf, ninf};            // an element outside the map never wins and is never stored
        load_run<f32x4_t>(p, full, m, v);
        const int16_t k = (int16_t)(row0 + j);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (CONF) {
                const float ex = __expf(-fabsf(v[e] - best[e]));
                s[e] = v[e] > best[e] ? s[e] * ex + 1.f : s[e] + ex;
            }
            if (v[e] > best[e]) {
                if (CONF) { sec[e] = best[e]; lab2[e] = lab[e]; }
                best[e] = v[e]; lab[e] = k;
            } else if (CONF && v[e] > sec[e]) {
                sec[e] = v[e]; lab2[e] = k;
            }
        }
    }
    store_run_any<f32x4_t>(score + xb, full, m, best);
    store_run_any<i16x4_t>(label + xb, full, m, lab);
    if (CONF) {
        if (score2) store_run_any<f32x4_t>(score2 + xb, full, m, sec);
        if (label2) store_run_any<i16x4_t>(label2 + xb, full, m, lab2);
        if (sum) {
            if (last) {
#pragma unroll
                for (int e = 0; e < 4; ++e) s[e] = best[e] + logf(s[e]);
            }
            store_run_any<f32x4_t>(sum + xb, full, m, s);
        }
    }
}

inline int grid_for(size_t total) {
    size_t g = (total + 255) / 256;
    if (g > 256 * 16) g = 256 * 16;
    return (int)(g < 1 ? 1 : g);
}

}  // namespace

int launch_eval_make_crops(const float* img, float* crops, int C, int height, int width, int crop, int stride, int h_grids, int w_grids,
                           int flip, const float* pad3, hipStream_t st) {
    const int n = h_grids * w_grids;
    hipLaunchKernelGGL(eval_make_crops_kernel, dim3(grid_for((size_t)(flip ? 2 : 1) * n * C * crop * crop)), dim3(256), 0, st, img, crops, C,
                       height, width, crop, stride, w_grids, n, flip, pad3[0], pad3[1], pad3[2]);
    LSEG_HIP_TRY(hipGetLastError());
    return 0;
}
int launch_eval_accumulate(const float* outs, float* outputs, int K, int height, int width, int ph, int pw, int crop, int stride, int h_grids,
                           int w_grids, int flip, hipStream_t st) {
    hipLaunchKernelGGL(eval_accumulate_kernel, dim3(grid_for((size_t)K * height * width)), dim3(256), 0, st, outs, outputs, K, height, width,
                       ph, pw, crop, stride, h_grids, w_grids, flip);
    LSEG_HIP_TRY(hipGetLastError());
    return 0;
}
int launch_eval_accumulate_lowres(const float* low, float* outputs, int K, int height, int width, int crop, int stride, int h_grids, int w_grids,
                                  int flip, hipStream_t st) {
    const size_t rows = (size_t)K * height;
    if (rows > 0x7fffffffu) return set_error(LSEG_ERR_UNSUPPORTED, "eval_accumulate_lowres: too many rows");
    hipLaunchKernelGGL(eval_accumulate_lowres_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, low, outputs, K, height, width, crop,
                       stride, h_grids, w_grids, flip);
    LSEG_HIP_TRY(hipGetLastError());
    return 0;
}
// the bounding rectangle of boxes [first, first + nbox) on the [height, width] map is the launch; a window wholly in the padding launches nothing
int launch_eval_accumulate_window(const float* outs, float* sum, int K, int height, int width, int crop, int stride, int w_grids, int flip,
                                  int first, int nbox, int lowres, hipStream_t st) {
    const int last = first + nbox - 1;
    const int ih_a = first / w_grids, ih_b = last / w_grids;
    const long long y_lo = (long long)ih_a * stride, y_hi = std::min<long long>((long long)ih_b * stride + crop, height);
    long long x_lo = 0, x_hi = width;
    if (ih_a == ih_b) {
        x_lo = (long long)(first - ih_a * w_grids) * stride;
        x_hi = std::min<long long>((long long)(last - ih_b * w_grids) * stride + crop, width);
    }
    if (y_lo >= y_hi || x_lo >= x_hi) return 0;
    const int ny = (int)(y_hi - y_lo);
    const size_t rows = (size_t)K * ny;
    if (rows > 0x7fffffffu) return set_error(LSEG_ERR_UNSUPPORTED, "eval_accumulate_window: too many rows");
    const dim3 grid((unsigned)((rows + 3) / 4));
    if (lowres)
        hipLaunchKernelGGL(eval_accumulate_window_kernel<true>, grid, dim3(256), 0, st, outs, sum, K, height, width, crop, stride, w_grids, flip,
                           first, nbox, (int)y_lo, ny, (int)x_lo, (int)x_hi);
    else
        hipLaunchKernelGGL(eval_accumulate_window_kernel<false>, grid, dim3(256), 0, st, outs, sum, K, height, width, crop, stride, w_grids, flip,
                           first, nbox, (int)y_lo, ny, (int)x_lo, (int)x_hi);
    LSEG_HIP_TRY(hipGetLastError());
    return 0;
}
int launch_eval_finalize(const float* sum, float* map, int K, int height, int width, int crop, int stride, int h_grids, int w_grids,
                         hipStream_t st) {
    const size_t total = (size_t)K * height * width;
    const int vec = ((reinterpret_cast<uintptr_t>(sum) | reinterpret_cast<uintptr_t>(map)) & 15) == 0;
    hipLaunchKernelGGL(eval_finalize_kernel, dim3(grid_for((total + 3) / 4)), dim3(256), 0, st, sum, map, total, height, width, crop, stride,
                       h_grids, w_grids, vec);
    LSEG_HIP_TRY(hipGetLastError());
    return 0;
}
// one launch per label panel; the frame of the runs is the score plane's, first = 1 writes the state without reading it
int launch_eval_merge_labels(const float* scores, int rows, int row0, int H, int W, int16_t* label, float* score, int16_t* label2, float* score2,
                             float* sum, int first, int last, hipStream_t st) {
    const long long npix = (long long)H * W;
    const int shift = (int)((reinterpret_cast<uintptr_t>(score) >> 2) & 3);
    const long long nq = (npix + shift + 3) >> 2;
    const long long blocks = (nq + 255) / 256;
    if (blocks > 0x7fffffffLL) return set_error(LSEG_ERR_UNSUPPORTED, "eval_merge_labels: too many pixels");
    if (label2 || score2 || sum)
        hipLaunchKernelGGL(eval_merge_labels_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, scores, rows, row0, npix, label, score, label2,
                           score2, sum, first, last, shift, nq);
    else
        hipLaunchKernelGGL(eval_merge_labels_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, scores, rows, row0, npix, label, score, label2,
                           score2, sum, first, last, shift, nq);
    LSEG_HIP_TRY(hipGetLastError());
    return 0;
}
int launch_eval_resize(const float* src, float* dst, int P, int Hi, int Wi, int Ho, int Wo, int accumulate, hipStream_t st) {
    hipLaunchKernelGGL(eval_resize_kernel, dim3(grid_for((size_t)P * Ho * Wo)), dim3(256), 0, st, src, dst, P, Hi, Wi, Ho, Wo, accumulate);
    LSEG_HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace lseg
