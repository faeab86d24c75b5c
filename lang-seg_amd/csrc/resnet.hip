// resnet.hip -- the torchvision ResNet-101 image tower of the zero-shot CLIP-ResNet-101 network (lseg_config.flags bit 5;
// reference modules/models/lseg_vit_zs.py _make_pretrained_clip_rn101 / _make_resnet_backbone).  Eval mode: every BatchNorm is
// folded into its conv (running statistics, eps 1e-5).
//
// What lives here: the stem (conv1 7x7/2 + bn1 + relu) as a direct fp32 kernel, the 3x3/2 max-pool, and the BN-folding packers.
// The bottleneck convs themselves run on the GEMM family (gemm.hip implicit conv: ksize 1 | 3, stride 1 | 2, relu_after_res);
// Engine::resnet_forward strings them together.  Every map is padded NHWC 16-bit (a 1-pixel zero border, as the DPT neck's maps).
#include <algorithm>

#include "ops.h"
#include "../../include/lseg_hip.h"

namespace lseg {

namespace {

constexpr int STEM_K = 147;             // 3 x 7 x 7 taps
constexpr int STEM_C = 64;

// Stem: one thread = one output pixel, all 64 output channels in fp32 registers.  The BN-folded weights [147][64] (37.6 KB) sit in
// LDS and are read as wave-uniform float4 broadcasts; the 147 input taps are read straight from the fp32 NCHW image (adjacent lanes =
// adjacent output columns: stride-2 reads that stay within a few cache lines per row).  ~1.1 GFLOP per 480 x 480 image: a small
// share of the tower's 72 GFLOP.  An im2col + MFMA GEMM would need a [B*Ho*Wo, 192] 16-bit operand
// (0.8 GB at B = 36) and round the image to 16 bits before the first conv; this keeps the stem in fp32 like the reference.
template <bool RELU>
__global__ __launch_bounds__(256) void rn_stem_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                      uint16_t* __restrict__ out, int B, int H, int W, int Ho, int Wo, int dtype) {
    __shared__ float4 ws[STEM_K * STEM_C / 4];
    __shared__ float bs[STEM_C];
    for (int i = threadIdx.x; i < STEM_K * STEM_C / 4; i += blockDim.x) ws[i] = reinterpret_cast<const float4*>(w)[i];
    if (threadIdx.x < STEM_C) bs[threadIdx.x] = bias[threadIdx.x];
    __syncthreads();
    const size_t total = (size_t)B * Ho * Wo;
    const size_t m = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (m >= total) return;
    const int ox = (int)(m % Wo), oy = (int)((m / Wo) % Ho), b = (int)(m / ((size_t)Wo * Ho));
    float acc[STEM_C];
#pragma unroll
    for (int c = 0; c < STEM_C; ++c) acc[c] = 0.f;
    const int iy0 = 2 * oy - 3, ix0 = 2 * ox - 3;
    for (int ci = 0; ci < 3; ++ci) {
        const float* plane = x + ((size_t)b * 3 + ci) * H * W;
        for (int ky = 0; ky < 7; ++ky) {
            const int iy = iy0 + ky;
            const bool rok = iy >= 0 && iy < H;
            const float* row = plane + (size_t)(rok ? iy : 0) * W;
#pragma unroll 1
            for (int kx = 0; kx < 7; ++kx) {          // (not unrolled: 64 accumulators + one tap's 16 weight quads stay under 128 VGPRs)
                const int ix = ix0 + kx;
                const float v = (rok && ix >= 0 && ix < W) ? row[ix] : 0.f;
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

// Max-pool 3x3 / 2, pad 1: one thread = one output pixel x 8 channels (16-byte loads and store).  The input is the stem's ReLU output
// (>= 0), so the zero border of the padded map gives the same maximum as torch's -inf padding.  For non-negative bf16 / fp16 values
// the order of the values is the order of their bit patterns as unsigned integers: the max is taken on the raw 16-bit words -- exact,
// dtype-independent, and a NaN (pattern above +inf) propagates as torch's max-pool propagates it.
__device__ __forceinline__ uint32_t max2u16(uint32_t a, uint32_t b) {
    const uint32_t lo = (a & 0xffffu) > (b & 0xffffu) ? (a & 0xffffu) : (b & 0xffffu);
    const uint32_t hi = (a >> 16) > (b >> 16) ? (a >> 16) : (b >> 16);
    return lo | (hi << 16);
}
__global__ __launch_bounds__(256) void rn_maxpool_kernel(const uint16_t* __restrict__ in, uint16_t* __restrict__ out, int B, int H, int W,
                                                         int Ho, int Wo, int C) {
    const int c8n = C >> 3;
    const size_t total = (size_t)B * Ho * Wo * c8n;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % c8n) * 8;
        const size_t m = i / c8n;
        const int ox = (int)(m % Wo), oy = (int)((m / Wo) % Ho), b = (int)(m / ((size_t)Wo * Ho));
        uint4 r = make_uint4(0u, 0u, 0u, 0u);
        // output (oy, ox) covers input rows 2oy-1 .. 2oy+1 = padded rows 2oy .. 2oy+2 (all inside the padded map: 2*(Ho-1)+2 <= H+1)
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            const int py = 2 * oy + dy;
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int px = 2 * ox + dx;
                const uint4 v = *reinterpret_cast<const uint4*>(in + (((size_t)b * (H + 2) + py) * (W + 2) + px) * C + c);
                r.x = max2u16(r.x, v.x); r.y = max2u16(r.y, v.y); r.z = max2u16(r.z, v.z); r.w = max2u16(r.w, v.w);
            }
        }
        *reinterpret_cast<uint4*>(out + (((size_t)b * (Ho + 2) + oy + 1) * (Wo + 2) + ox + 1) * C + c) = r;
    }
}

// 1x1 conv + BN: wp[co, ci] = w[co, ci] * s[co], bias[co] = bn_b - bn_m * s, s = bn_w / sqrt(bn_v + eps); bn_w NULL: no BatchNorm (s = 1, bias 0)
__global__ void pack_conv1x1_kernel(const float* w, const float* bn_w, const float* bn_b, const float* bn_m, const float* bn_v, float eps,
                                    void* wp, float* bias_out, int Co, int Ci, int dtype) {
    const size_t n = (size_t)Co * Ci;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int co = (int)(i / Ci), ci = (int)(i % Ci);
        const float s = bn_w ? bn_w[co] * rsqrtf(bn_v[co] + eps) : 1.f;
        store_from_f32(wp, i, dtype, w[i] * s);
        if (ci == 0) bias_out[co] = bn_w ? bn_b[co] - bn_m[co] * s : 0.f;
    }
}

// stem conv1 [64, 3, 7, 7] + bn1 -> fp32 [147][64] (tap-major, the layout rn_stem_kernel reads), bias [64]
__global__ void pack_rn_stem_kernel(const float* w, const float* bn_w, const float* bn_b, const float* bn_m, const float* bn_v, float eps,
                                    float* wp, float* bias_out) {
    const int n = STEM_C * STEM_K;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int co = i / STEM_K, k = i % STEM_K;
        const float s = bn_w[co] * rsqrtf(bn_v[co] + eps);
        wp[k * STEM_C + co] = w[i] * s;
        if (k == 0) bias_out[co] = bn_b[co] - bn_m[co] * s;
    }
}

// Train-mode BatchNorm of the tower on a padded NHWC map, interior pixels only (the zero border stays as it is: conv2's 3x3 window and
// the next launch_bn_stats read it): y = bn(x) with mean / biased variance from the batch sums `stats` = {sum x, sum x^2} [2C] over
// 1 / inv_n pixels; RES 1 adds a plain map (the identity of blocks 1..), RES 2 adds a second map normalised with batch sums of its own
// (block 0's downsample branch); then the optional ReLU.  One lane = one pixel x 8 channels: 16-byte loads and one 16-byte store; the
// per-channel scale / shift pairs are computed once per thread (the grid stride is a multiple of C / 8 for the tower's power-of-two
// widths).  y may be x (in place) and res may be y (relu(bn3(t) + x) written over x): each element is read by the lane that then
// writes it, hence no __restrict__ on the maps.
template <int RES>
__global__ __launch_bounds__(256) void rn_bn_apply_res_kernel(const uint16_t* x, uint16_t* y, const float* __restrict__ stats,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta, const uint16_t* res,
                                                              const float* __restrict__ rstats, const float* __restrict__ rgamma,
                                                              const float* __restrict__ rbeta, int B, int H, int W, int C, float eps, float inv_n,
                                                              int relu, int dtype) {
    const int c8n = C >> 3;
    const size_t n = (size_t)B * H * W * c8n;
    const bool fixed_c = ((size_t)gridDim.x * blockDim.x) % c8n == 0;
    float sc[8], sh[8], rsc[8], rsh[8];
    auto affine = [&](const float* st, const float* g, const float* b, int c0, float* scale, float* shift) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float4 s1 = *reinterpret_cast<const float4*>(st + c0 + 4 * h), s2 = *reinterpret_cast<const float4*>(st + C + c0 + 4 * h);
            const float4 g4 = *reinterpret_cast<const float4*>(g + c0 + 4 * h), b4 = *reinterpret_cast<const float4*>(b + c0 + 4 * h);
            const float a1[4] = {s1.x, s1.y, s1.z, s1.w}, a2[4] = {s2.x, s2.y, s2.z, s2.w}, gg[4] = {g4.x, g4.y, g4.z, g4.w}, bb[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float m = a1[k] * inv_n;
                const float r = gg[k] * rsqrtf(fmaxf(a2[k] * inv_n - m * m, 0.f) + eps);
                scale[4 * h + k] = r; shift[4 * h + k] = bb[k] - m * r;
            }
        }
    };
    auto load_c = [&](int c0) {
        affine(stats, gamma, beta, c0, sc, sh);
        if (RES == 2) affine(rstats, rgamma, rbeta, c0, rsc, rsh);
    };
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (fixed_c && i < n) load_c((int)(i % c8n) * 8);
    for (; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int c0 = (int)(i % c8n) * 8;
        if (!fixed_c) load_c(c0);
        size_t p = i / c8n;
        const int xx = (int)(p % W); p /= W;
        const int yy = (int)(p % H);
        const int b = (int)(p / H);
        const size_t off = (((size_t)b * (H + 2) + yy + 1) * (W + 2) + xx + 1) * C + c0;
        const uint4 ux = *reinterpret_cast<const uint4*>(x + off);
        uint4 ur = make_uint4(0u, 0u, 0u, 0u);
        if (RES != 0) ur = *reinterpret_cast<const uint4*>(res + off);
        const uint16_t *ex = reinterpret_cast<const uint16_t*>(&ux), *er = reinterpret_cast<const uint16_t*>(&ur);
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float t = fmaf(load_as_f32(ex, k, dtype), sc[k], sh[k]);
            if (RES == 1) t += load_as_f32(er, k, dtype);
            if (RES == 2) t += fmaf(load_as_f32(er, k, dtype), rsc[k], rsh[k]);
            v[k] = relu ? fmaxf(t, 0.f) : t;
        }
        *reinterpret_cast<uint4*>(y + off) = make_uint4(pack2_dt(v[0], v[1], dtype), pack2_dt(v[2], v[3], dtype), pack2_dt(v[4], v[5], dtype),
                                                        pack2_dt(v[6], v[7], dtype));
    }
}

unsigned grid_of(size_t total) {
    size_t g = (total + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > 65535 * 4 ? 65535 * 4 : g));
}

}  // namespace

int launch_rn_stem(const float* x, const float* w, const float* bias, void* out, int B, int H, int W, int dtype, hipStream_t st, int relu) {
    if (B < 1 || H < 2 || W < 2 || (H & 1) || (W & 1)) return set_error(LSEG_ERR_INVALID, "rn_stem: B=%d H=%d W=%d (H, W even)", B, H, W);
    if (dtype != DT_BF16 && dtype != DT_F16) return set_error(LSEG_ERR_INVALID, "rn_stem: dtype %d", dtype);
    const int Ho = H / 2, Wo = W / 2;
    const size_t total = (size_t)B * Ho * Wo;
    if (relu) hipLaunchKernelGGL(rn_stem_kernel<true>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x, w, bias, (uint16_t*)out, B, H, W, Ho, Wo, dtype);
    else hipLaunchKernelGGL(rn_stem_kernel<false>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x, w, bias, (uint16_t*)out, B, H, W, Ho, Wo, dtype);
    LSEG_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_bn_apply_res(const void* x, void* y, const float* stats, const float* gamma, const float* beta, const void* res, const float* rstats,
                        const float* rgamma, const float* rbeta, int B, int H, int W, int C, float eps, double count, int relu, int dtype,
                        hipStream_t st) {
    if (B < 1 || H < 1 || W < 1 || C < 8 || C % 8) return set_error(LSEG_ERR_INVALID, "bn_apply_res: B=%d H=%d W=%d C=%d (C a multiple of 8)", B, H, W, C);
    if (dtype != DT_BF16 && dtype != DT_F16) return set_error(LSEG_ERR_INVALID, "bn_apply_res: dtype %d", dtype);
    if (!x || !y || !stats || !gamma || !beta || !(count > 0)) return set_error(LSEG_ERR_INVALID, "bn_apply_res: NULL pointer / count");
    if (rstats && (!res || !rgamma || !rbeta)) return set_error(LSEG_ERR_INVALID, "bn_apply_res: a normalised residual needs its map, gamma and beta");
    const dim3 grid(std::min(grid_of((size_t)B * H * W * (C / 8)), 4096u)), block(256);      // grid-stride: the per-channel affine is computed once per thread
    const float inv_n = (float)(1.0 / count);
    const uint16_t *xp = (const uint16_t*)x, *rp = (const uint16_t*)res;
    if (rstats) hipLaunchKernelGGL(rn_bn_apply_res_kernel<2>, grid, block, 0, st, xp, (uint16_t*)y, stats, gamma, beta, rp, rstats, rgamma, rbeta, B, H, W, C, eps, inv_n, relu, dtype);
    else if (res) hipLaunchKernelGGL(rn_bn_apply_res_kernel<1>, grid, block, 0, st, xp, (uint16_t*)y, stats, gamma, beta, rp, rstats, rgamma, rbeta, B, H, W, C, eps, inv_n, relu, dtype);
    else hipLaunchKernelGGL(rn_bn_apply_res_kernel<0>, grid, block, 0, st, xp, (uint16_t*)y, stats, gamma, beta, rp, rstats, rgamma, rbeta, B, H, W, C, eps, inv_n, relu, dtype);
    LSEG_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_rn_maxpool(const void* in, void* out, int B, int H, int W, int C, int dtype, hipStream_t st) {
    if (B < 1 || H < 2 || W < 2 || (H & 1) || (W & 1) || C % 8) return set_error(LSEG_ERR_INVALID, "rn_maxpool: B=%d H=%d W=%d C=%d", B, H, W, C);
    if (dtype != DT_BF16 && dtype != DT_F16) return set_error(LSEG_ERR_INVALID, "rn_maxpool: dtype %d", dtype);
    const int Ho = H / 2, Wo = W / 2;
    hipLaunchKernelGGL(rn_maxpool_kernel, dim3(grid_of((size_t)B * Ho * Wo * (C / 8))), dim3(256), 0, st, (const uint16_t*)in, (uint16_t*)out,
                       B, H, W, Ho, Wo, C);
    LSEG_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_pack_conv1x1(const float* w, const float* bn_w, const float* bn_b, const float* bn_m, const float* bn_v, float bn_eps,
                        void* wp, float* bias_out, int Co, int Ci, int dtype, hipStream_t st) {
    hipLaunchKernelGGL(pack_conv1x1_kernel, dim3(grid_of((size_t)Co * Ci)), dim3(256), 0, st, w, bn_w, bn_b, bn_m, bn_v, bn_eps, wp, bias_out,
                       Co, Ci, dtype);
    LSEG_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_pack_rn_stem(const float* w, const float* bn_w, const float* bn_b, const float* bn_m, const float* bn_v, float bn_eps,
                        float* wp, float* bias_out, hipStream_t st) {
    hipLaunchKernelGGL(pack_rn_stem_kernel, dim3(grid_of((size_t)STEM_C * STEM_K)), dim3(256), 0, st, w, bn_w, bn_b, bn_m, bn_v, bn_eps, wp, bias_out);
    LSEG_HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace lseg
