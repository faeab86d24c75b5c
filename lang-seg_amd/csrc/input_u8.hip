// input_u8.hip -- the input stage for decoded images: uint8 [B, H, W, 3] (HWC, RGB, dense) in, the first stage's operand out, with
// torchvision's ToTensor + Normalize(mean, std) fused into the read (lseg_module.py:37-50 builds that transform):
//     v -> (float(v) / 255 - mean[c]) / std[c]         three correctly rounded fp32 operations, in torch's order
// Three kernels, one per first stage: the patch-embedding operand rows of the ViT towers (the uint8 form of im2col_patch_kernel,
// elementwise.hip), the ResNet-101 stem (the uint8 form of rn_stem_kernel, resnet.hip) and the crops of one scale of the multi-scale
// evaluator (normalise + eval_resize_kernel + eval_make_crops_kernel of evaluator.hip in one pass).  Each writes the bits its fp32
// counterpart writes when it is fed the torch-normalised tensor: the normalised value of a byte depends on (byte, channel) alone, so
// every block first fills a 3 x 256 table in LDS with the three roundings spelled out and the kernels read the table -- the same
// bits as the arithmetic per pixel, two divisions per table entry instead of per pixel.
#include <algorithm>
#include <cmath>

#include "ops.h"
#include "../../include/lseg_hip.h"

namespace lseg {
namespace {

// div, sub, div: no contraction (there is no product to fuse, the pragma keeps it that way), no reciprocal multiply
__device__ __forceinline__ float norm_u8_value(int v, float mean, float std) {
#pragma clang fp contract(off)
    return __fdiv_rn(__fsub_rn(__fdiv_rn((float)v, 255.f), mean), std);
}
// lut[c * 256 + v]; ends with a barrier
__device__ __forceinline__ void fill_norm_lut(float* lut, const NormU8& n) {
    for (int i = threadIdx.x; i < 3 * 256; i += blockDim.x) {
        const int c = i >> 8;
        lut[i] = norm_u8_value(i & 255, c == 0 ? n.mean[0] : (c == 1 ? n.mean[1] : n.mean[2]), c == 0 ? n.std[0] : (c == 1 ? n.std[1] : n.std[2]));
    }
    __syncthreads();
}
__device__ __forceinline__ uint32_t byte_of(const uint4 (&q)[3], int i) {          // byte i of 48 (i is a compile-time constant after unrolling)
    const uint4& w = q[i >> 4];
    const int k = (i >> 2) & 3;
    const uint32_t u = k == 0 ? w.x : (k == 1 ? w.y : (k == 2 ? w.z : w.w));
    return (u >> (8 * (i & 3))) & 0xffu;
}

inline unsigned grid_for(size_t total) { return (unsigned)std::min<size_t>((total + 255) / 256, 256 * 16); }

// ---- patch-embedding operand rows: x uint8 [B, H, W, 3] -> A [B*gh*gw, 3*P*P] (k = c*P*P + i*P + j), the layout of im2col_patch_kernel.
// A lane owns one run of 16 pixels of an image row: 48 contiguous bytes in (three 16-byte loads; run g starts at byte 48 g of the dense
// image, so consecutive lanes read consecutive runs and a wave reads 3 KB of contiguous image rows), 16 values of each channel out (two
// 16-byte stores per channel).  P % 16 == 0 keeps a run inside one patch row; W % 16 == 0 follows from W % P == 0.
__global__ __launch_bounds__(256) void im2col_patch_u8_kernel(const uint8_t* __restrict__ x, uint16_t* __restrict__ A, int B, int H, int W, int P,
                                                              int dtype, NormU8 n) {
    __shared__ float lut[3 * 256];
    fill_norm_lut(lut, n);
    const int gh = H / P, gw = W / P, wr = W / 16;
    const size_t Kd = (size_t)3 * P * P;
    const size_t total = (size_t)B * H * wr;
    for (size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x; g < total; g += (size_t)gridDim.x * blockDim.x) {
        const int xr = (int)(g % wr);
        const size_t row = g / wr;
        const int y = (int)(row % H), b = (int)(row / H);
        const uint4* src = reinterpret_cast<const uint4*>(x + g * 48);
        const uint4 q[3] = {src[0], src[1], src[2]};
        const int x0 = xr * 16, px = x0 / P, j0 = x0 - px * P, py = y / P, i = y - py * P;
        const size_t m = ((size_t)b * gh + py) * gw + px;
        uint16_t* dst = A + m * Kd + (size_t)i * P + j0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            uint32_t o[8];
#pragma unroll
            for (int e = 0; e < 8; ++e)
                o[e] = pack2_dt(lut[c * 256 + byte_of(q, 6 * e + c)], lut[c * 256 + byte_of(q, 6 * e + 3 + c)], dtype);
            uint4* d = reinterpret_cast<uint4*>(dst + (size_t)c * P * P);
            d[0] = make_uint4(o[0], o[1], o[2], o[3]);
            d[1] = make_uint4(o[4], o[5], o[6], o[7]);
        }
    }
}

// ---- ResNet-101 stem (conv1 7x7/2 + folded bn1 + relu) from uint8 HWC.  rn_stem_kernel's arithmetic -- one thread = one output pixel,
// 64 fp32 accumulators, the taps in (channel, ky, kx) order through fmaf, zero for a tap outside the image -- with the taps read from an
// LDS tile instead of the fp32 NCHW image: a block owns STEM_TY x STEM_TX output pixels and first stages the (2 TY + 5) x (2 TX + 5) x 3
// normalised input window.  The window's rows are contiguous byte runs of the image; they are fetched as the 16-byte chunks (aligned in
// the image buffer) that cover them, one chunk per lane, and every byte of a chunk that lies in the window is scattered to its
// (channel, row, column) slot.  Only the last chunk of the whole buffer can reach past its end: that one is read byte by byte.
constexpr int STEM_K = 147, STEM_C = 64;
constexpr int STEM_TX = 32, STEM_TY = 8;
constexpr int STEM_IW = 2 * STEM_TX + 5, STEM_IH = 2 * STEM_TY + 5;      // 69 x 21 input window
constexpr int STEM_LD = 72;                                              // LDS row pitch of the window (floats)
constexpr int STEM_CHUNKS = 16;                                          // chunk slots per window row: 69 * 3 = 207 bytes span <= 14 chunks

template <bool RELU>
__global__ __launch_bounds__(256) void rn_stem_u8_kernel(const uint8_t* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                         uint16_t* __restrict__ out, int B, int H, int W, int Ho, int Wo, int dtype, NormU8 n) {
    __shared__ float4 ws[STEM_K * STEM_C / 4];
    __shared__ float bs[STEM_C];
    __shared__ float lut[3 * 256];
    __shared__ float tile[3 * STEM_IH * STEM_LD];
    for (int i = threadIdx.x; i < STEM_K * STEM_C / 4; i += blockDim.x) ws[i] = reinterpret_cast<const float4*>(w)[i];
    if (threadIdx.x < STEM_C) bs[threadIdx.x] = bias[threadIdx.x];
    for (int i = threadIdx.x; i < 3 * STEM_IH * STEM_LD; i += blockDim.x) tile[i] = 0.f;       // taps outside the image stay 0
    fill_norm_lut(lut, n);                                                                      // (barrier)
    const int b = blockIdx.z, oy0 = blockIdx.y * STEM_TY, ox0 = blockIdx.x * STEM_TX;
    const int iy_lo = 2 * oy0 - 3, ix_lo = 2 * ox0 - 3;
    const long long total_bytes = (long long)B * H * W * 3;
    const int cx0 = ix_lo < 0 ? 0 : ix_lo, cx1 = ix_lo + STEM_IW > W ? W : ix_lo + STEM_IW;   // image columns [cx0, cx1) of the window
    for (int t = threadIdx.x; t < STEM_IH * STEM_CHUNKS; t += blockDim.x) {
        const int r = t / STEM_CHUNKS, ck = t - r * STEM_CHUNKS;
        const int iy = iy_lo + r;
        if (iy < 0 || iy >= H || cx1 <= cx0) continue;
        const long long rowbase = ((long long)b * H + iy) * W * 3;
        const long long a0 = rowbase + (long long)cx0 * 3, a1 = rowbase + (long long)cx1 * 3;  // bytes [a0, a1) of the buffer
        const long long ca = ((a0 >> 4) + ck) << 4;                                             // this lane's chunk starts here
        if (ca >= a1) continue;
        uint32_t wv[4];
        if (ca + 16 <= total_bytes) {
            const uint4 q = *reinterpret_cast<const uint4*>(x + ca);
            wv[0] = q.x; wv[1] = q.y; wv[2] = q.z; wv[3] = q.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                wv[k] = 0u;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (ca + 4 * k + e < total_bytes) wv[k] |= (uint32_t)x[ca + 4 * k + e] << (8 * e);
            }
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const long long a = ca + k;
            if (a < a0 || a >= a1) continue;
            const int rel = (int)(a - rowbase);                 // byte within the image row
            const int px = rel / 3, ch = rel - 3 * px;
            const uint32_t v = (wv[k >> 2] >> (8 * (k & 3))) & 0xffu;
            tile[(ch * STEM_IH + r) * STEM_LD + (px - ix_lo)] = lut[ch * 256 + v];
        }
    }
    __syncthreads();
    const int tx = threadIdx.x % STEM_TX, ty = threadIdx.x / STEM_TX;
    const int ox = ox0 + tx, oy = oy0 + ty;
    if (ox >= Wo || oy >= Ho) return;
    float acc[STEM_C];
#pragma unroll
    for (int c = 0; c < STEM_C; ++c) acc[c] = 0.f;
    for (int ci = 0; ci < 3; ++ci) {
        for (int ky = 0; ky < 7; ++ky) {
            const float* row = tile + (ci * STEM_IH + 2 * ty + ky) * STEM_LD + 2 * tx;
#pragma unroll 1
            for (int kx = 0; kx < 7; ++kx) {          // (not unrolled, as in rn_stem_kernel: 64 accumulators + one tap's 16 weight quads)
                const float v = row[kx];
                const float4* wk = ws + ((ci * 7 + ky) * 7 + kx) * (STEM_C / 4);
#pragma unroll
                for (int c4 = 0; c4 < STEM_C / 4; ++c4) {
                    const float4 q = wk[c4];
                    acc[4 * c4 + 0] = fmaf(v, q.x, acc[4 * c4 + 0]);
                    acc[4 * c4 + 1] = fmaf(v, q.y, acc[4 * c4 + 1]);
                    acc[4 * c4 + 2] = fmaf(v, q.z, acc[4 * c4 + 2]);
                    acc[4 * c4 + 3] = fmaf(v, q.w, acc[4 * c4 + 3]);
                }
            }
        }
    }
    uint4* dst = reinterpret_cast<uint4*>(out + (((size_t)b * (Ho + 2) + oy + 1) * (Wo + 2) + ox + 1) * STEM_C);
#pragma unroll
    for (int c8 = 0; c8 < STEM_C / 8; ++c8) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) { const float t = acc[c8 * 8 + k] + bs[c8 * 8 + k]; v[k] = RELU ? (t > 0.f ? t : 0.f) : t; }
        dst[c8] = make_uint4(pack2_dt(v[0], v[1], dtype), pack2_dt(v[2], v[3], dtype), pack2_dt(v[4], v[5], dtype), pack2_dt(v[6], v[7], dtype));
    }
}

// ---- the crops of one scale of the multi-scale evaluator from ONE uint8 [Hi, Wi, 3] image: normalise, bilinear align_corners=True resize
// to (height, width), pad with pad[c] up to the crop grid, cut -- the reference's order (encoding_models.py:66-99), which the float path
// runs as eval_resize_kernel + eval_make_crops_kernel.  A lane owns one pixel of one crop, all three channels: it takes the four taps'
// normalised values from the table, interpolates with src_tap / bilerp exactly as eval_resize_kernel does, and writes the crop and its
// mirrored twin.  The taps are a gather of 3-byte pixels (two adjacent pixels on each of two rows), read as bytes; the stores are one
// float per lane, consecutive lanes consecutive columns, as in eval_make_crops_kernel.
__global__ __launch_bounds__(256) void eval_make_crops_u8_kernel(const uint8_t* __restrict__ img, float* __restrict__ crops, int Hi, int Wi, int height,
                                                                 int width, int crop, int stride, int w_grids, int nbox, int flip, float pad0,
                                                                 float pad1, float pad2, NormU8 n) {
    __shared__ float lut[3 * 256];
    fill_norm_lut(lut, n);
    const float ry = height > 1 ? (float)(Hi - 1) / (float)(height - 1) : 0.f, rx = width > 1 ? (float)(Wi - 1) / (float)(width - 1) : 0.f;
    const size_t plane = (size_t)crop * crop;
    const size_t total = (size_t)nbox * plane;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int xc = (int)(i % crop);
        const int yc = (int)((i / crop) % crop);
        const int k = (int)(i / plane);
        const int idh = k / w_grids, idw = k - idh * w_grids;
        const int yy = idh * stride + yc, xx = idw * stride + xc;
        float v[3] = {pad0, pad1, pad2};
        if (yy < height && xx < width) {
            int y0, y1, x0, x1;
            float ly, lx;
            src_tap(ry, yy, Hi, y0, y1, ly);
            src_tap(rx, xx, Wi, x0, x1, lx);
            const uint8_t *p00 = img + ((size_t)y0 * Wi + x0) * 3, *p01 = img + ((size_t)y0 * Wi + x1) * 3;
            const uint8_t *p10 = img + ((size_t)y1 * Wi + x0) * 3, *p11 = img + ((size_t)y1 * Wi + x1) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c)
                v[c] = bilerp(lut[c * 256 + p00[c]], lut[c * 256 + p01[c]], lut[c * 256 + p10[c]], lut[c * 256 + p11[c]], lx, ly);
        }
        float* o = crops + (size_t)k * 3 * plane + (size_t)yc * crop;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c * plane + xc] = v[c];
        if (flip) {
            float* t = o + (size_t)nbox * 3 * plane;
#pragma unroll
            for (int c = 0; c < 3; ++c) t[c * plane + (crop - 1 - xc)] = v[c];
        }
    }
}

}  // namespace

int norm_u8_check(const char* what, const float* mean, const float* std, NormU8* out) {
    if (!mean || !std) return set_error(LSEG_ERR_INVALID, "%s: mean / std is NULL", what);
    for (int c = 0; c < 3; ++c) {
        if (!std::isfinite(mean[c]) || !std::isfinite(std[c])) return set_error(LSEG_ERR_INVALID, "%s: mean[%d] / std[%d] is not finite", what, c, c);
        if (std[c] == 0.f) return set_error(LSEG_ERR_INVALID, "%s: std[%d] is 0", what, c);
        out->mean[c] = mean[c]; out->std[c] = std[c];
    }
    return 0;
}

int im2col_patch_u8_check(const void* x, const void* A, int B, int H, int W, int P, int dtype) {
    if (!x || !A) return set_error(LSEG_ERR_INVALID, "patch_rows_u8: NULL pointer");
    if (dtype != DT_BF16 && dtype != DT_F16) return set_error(LSEG_ERR_INVALID, "patch_rows_u8: dtype %d", dtype);
    if (B < 1 || H < 1 || W < 1 || P < 1 || H % P || W % P) return set_error(LSEG_ERR_INVALID, "patch_rows_u8: B=%d H=%d W=%d P=%d (H, W multiples of P)", B, H, W, P);
    if (P % 16) return set_error(LSEG_ERR_UNSUPPORTED, "patch_rows_u8: P=%d must be a multiple of 16 (a lane owns 16 pixels of a patch row)", P);
    if (((uintptr_t)x | (uintptr_t)A) & 15) return set_error(LSEG_ERR_INVALID, "patch_rows_u8: pointers must be 16-byte aligned");
    return 0;
}
int launch_im2col_patch_u8(const uint8_t* x, void* A, int B, int H, int W, int P, int dtype, const NormU8& n, hipStream_t st) {
    hipLaunchKernelGGL(im2col_patch_u8_kernel, dim3(grid_for((size_t)B * H * (W / 16))), dim3(256), 0, st, x, (uint16_t*)A, B, H, W, P, dtype, n);
    LSEG_HIP_TRY(hipGetLastError());
    return 0;
}

int rn_stem_u8_check(const void* x, const void* w, const void* bias, const void* out, int B, int H, int W, int dtype) {
    if (!x || !w || !bias || !out) return set_error(LSEG_ERR_INVALID, "rn_stem_u8: NULL pointer");
    if (B < 1 || B > 65535 || H < 2 || W < 2 || (H & 1) || (W & 1)) return set_error(LSEG_ERR_INVALID, "rn_stem_u8: B=%d H=%d W=%d (H, W even)", B, H, W);
    if (dtype != DT_BF16 && dtype != DT_F16) return set_error(LSEG_ERR_INVALID, "rn_stem_u8: dtype %d", dtype);
    if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)out) & 15) return set_error(LSEG_ERR_INVALID, "rn_stem_u8: pointers must be 16-byte aligned");
    return 0;
}
int launch_rn_stem_u8(const uint8_t* x, const float* w, const float* bias, void* out, int B, int H, int W, int dtype, const NormU8& n, hipStream_t st,
                      int relu) {
    const int Ho = H / 2, Wo = W / 2;
    const dim3 grid((Wo + STEM_TX - 1) / STEM_TX, (Ho + STEM_TY - 1) / STEM_TY, B);
    if (grid.y > 65535) return set_error(LSEG_ERR_UNSUPPORTED, "rn_stem_u8: H=%d is too tall for one launch", H);
    if (relu) hipLaunchKernelGGL(rn_stem_u8_kernel<true>, grid, dim3(256), 0, st, x, w, bias, (uint16_t*)out, B, H, W, Ho, Wo, dtype, n);
    else hipLaunchKernelGGL(rn_stem_u8_kernel<false>, grid, dim3(256), 0, st, x, w, bias, (uint16_t*)out, B, H, W, Ho, Wo, dtype, n);
    LSEG_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_eval_make_crops_u8(const uint8_t* img, float* crops, int Hi, int Wi, int height, int width, int crop, int stride, int h_grids,
                              int w_grids, int flip, const float* pad3, const NormU8& n, hipStream_t st) {
    const int nbox = h_grids * w_grids;
    hipLaunchKernelGGL(eval_make_crops_u8_kernel, dim3(grid_for((size_t)nbox * crop * crop)), dim3(256), 0, st, img, crops, Hi, Wi, height, width,
                       crop, stride, w_grids, nbox, flip, pad3[0], pad3[1], pad3[2], n);
    LSEG_HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace lseg
