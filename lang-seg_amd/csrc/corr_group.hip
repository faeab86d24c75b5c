// corr_group.hip -- the per-image ("grouped") correlation of the zero-shot network on the TRAINING path (modules/models/lseg_net_zs.py:
// 198-208: image b is scored against its own G text rows [b*G, (b+1)*G) only, G = 2 for ['others', class]), forward and backward.
//
//   forward   low[b, k, p] = fp16( sum_c a16[b*hw + p, c] * T[b*G + k, c] )          fp32 accumulation, one fp16 rounding per logit:
//             the rounding points of the generic GEMM with round_mid = 1 that the shared label set takes (train.hip, forward_train)
//   backward  dA  = rt( sum_k d[row, k] * T[b*G + k, :] )                           fp32 accumulation, rt = rounding to the rows' type
//             dA' = fp16(logit_scale * dA)   (fp16 rows: the reference's half-precision d(image_features.half()), DESIGN par. 3.6)
//             df  = L2-norm backward of a = scale * f / ||f|| against the saved fp32 feature row f, written in the image operand type
//             == the shared path's  GEMM(drows x tnT) -> l2norm_scale_backward  pair, without the dA round trip through memory
//
// Both are HBM-bound streams.  The image's G text rows live in REGISTERS for the life of a workgroup: a workgroup covers a contiguous
// range of pixel rows of ONE image (grid.y = image), so T is read once per workgroup, never per row.
//   * forward: one wave per pixel row, 16-byte loads (8 fp16 channels per lane), v_dot2_f32_f16 against the resident T, one wave
//     reduction per label.  Replaces the B launches of an M = G GEMM through 128/256-row tiles of the inference path's form.
//   * backward: one wave per pixel row in the lane layout of elementwise.hip's l2norm_scale_bwd_kernel (lane owns float4 chunks
//     lane + 64 i of the row): the fp32 row reads are 16 bytes per lane, and the row reductions (||f||^2 and f . dA') run in the SAME order
//     as that kernel, so the two paths give the same bits wherever their dA agree.  dA is formed with fp32 fused multiply-adds on fp16
//     operands converted exactly (not v_dot2): d sits in fp16's SUBNORMAL range by construction (d(loss)/d(logit) ~ 1 / pixels), and
//     the FMA chain keeps every product exact and rounds each partial sum once, independent of the denorm mode of a dot instruction.
//     At G = 2 dA is exactly fp(d0 T0 + d1 T1): one rounding, as an MFMA with fp32 accumulation gives it.  Cost: G x 8 FMAs per lane and
//     row at out_c = 512, hidden under the 3 KB of traffic per row.
#include "ops.h"
#include "../../include/lseg_hip.h"

namespace lseg {
namespace {

typedef _Float16 __attribute__((ext_vector_type(2))) h2_t;

__device__ __forceinline__ float wave_sum_g(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float dot2_f16(uint32_t a, uint32_t b, float c) {
    return __builtin_amdgcn_fdot2(__builtin_bit_cast(h2_t, a), __builtin_bit_cast(h2_t, b), c, false);
}
__device__ __forceinline__ float rows_to_f32(uint32_t w, int hi, int dtype) {
    const uint16_t h = (uint16_t)(hi ? (w >> 16) : (w & 0xffffu));
    return dtype == DT_F16 ? f16_to_f32(h) : bf16_to_f32(h);
}
__device__ __forceinline__ float round_dt(float v, int dtype) {
    return dtype == DT_F16 ? round_f16(v) : bf16_to_f32(f32_to_bf16(v));
}

constexpr int FWD_ROWS_PER_BLOCK = 256;       // 4 waves x 16 iterations x RU = 4 rows
constexpr int FWD_RU = 4;
constexpr int BWD_ROWS_PER_BLOCK = 64;        // 4 waves x 8 iterations x RU = 2 rows
constexpr int BWD_RU = 2;

// a [B*hw, C] fp16, t [B*G, C] fp16 -> low [B, G, hw] fp32 (fp16 values).  C % 8 == 0, C <= 512 * NV.
template <int G, int NV>
__global__ __launch_bounds__(256) void corr_group_fwd_kernel(const uint16_t* __restrict__ a, const uint16_t* __restrict__ t,
                                                             float* __restrict__ low, int hw, int C) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y;
    const int nc = C >> 3;
    uint4 tr[G][NV];
#pragma unroll
    for (int k = 0; k < G; ++k)
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int j = lane + 64 * i;
            tr[k][i] = j < nc ? reinterpret_cast<const uint4*>(t + ((size_t)b * G + k) * C)[j] : make_uint4(0, 0, 0, 0);
        }
    const uint16_t* ab = a + (size_t)b * hw * C;
    float* lb = low + (size_t)b * G * hw;
    const int p0 = blockIdx.x * FWD_ROWS_PER_BLOCK, p1 = min(p0 + FWD_ROWS_PER_BLOCK, hw);
    for (int p = p0 + wave * FWD_RU; p < p1; p += 4 * FWD_RU) {
        uint4 av[FWD_RU][NV];
#pragma unroll
        for (int r = 0; r < FWD_RU; ++r)
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int j = lane + 64 * i;
                av[r][i] = (p + r < p1 && j < nc) ? reinterpret_cast<const uint4*>(ab + (size_t)(p + r) * C)[j] : make_uint4(0, 0, 0, 0);
            }
#pragma unroll
        for (int r = 0; r < FWD_RU; ++r) {
            float mine = 0.f;
#pragma unroll
            for (int k = 0; k < G; ++k) {
                float acc = 0.f;
#pragma unroll
                for (int i = 0; i < NV; ++i) {
                    acc = dot2_f16(av[r][i].x, tr[k][i].x, acc);
                    acc = dot2_f16(av[r][i].y, tr[k][i].y, acc);
                    acc = dot2_f16(av[r][i].z, tr[k][i].z, acc);
                    acc = dot2_f16(av[r][i].w, tr[k][i].w, acc);
                }
                acc = wave_sum_g(acc);
                if (lane == k) mine = acc;
            }
            if (lane < G && p + r < p1) lb[(size_t)lane * hw + p + r] = round_f16(mine);
        }
    }
}

// rows [B*hw, ldk] (fp16 | bf16, first G columns read), t [B*G, C] fp16, x [B*hw, C] fp32 -> dx [B*hw, C] (dx_dtype).
// rdt == DT_BF16 (lseg_config.flags bit 1): T is rounded to bf16 like the shared path's tn16_, dA is bf16 and the scale is applied un-rounded.
template <int G, int MAXV>
__global__ __launch_bounds__(256) void corr_group_bwd_kernel(const uint16_t* __restrict__ rows, int rdt, int ldk, const uint16_t* __restrict__ t,
                                                             const float* __restrict__ x, uint16_t* __restrict__ dx, int dx_dtype, int hw, int C,
                                                             float scale) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y;
    const int nv = C >> 2;
    float4 tf[G][MAXV];
#pragma unroll
    for (int k = 0; k < G; ++k)
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int g = lane + 64 * i;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (g < nv) {
                const uint2 u = reinterpret_cast<const uint2*>(t + ((size_t)b * G + k) * C)[g];
                v.x = rows_to_f32(u.x, 0, DT_F16); v.y = rows_to_f32(u.x, 1, DT_F16);
                v.z = rows_to_f32(u.y, 0, DT_F16); v.w = rows_to_f32(u.y, 1, DT_F16);
                if (rdt != DT_F16) { v.x = round_dt(v.x, rdt); v.y = round_dt(v.y, rdt); v.z = round_dt(v.z, rdt); v.w = round_dt(v.w, rdt); }
            }
            tf[k][i] = v;
        }
    const float post = rdt == DT_F16 ? 1.f : scale;
    const int p0 = blockIdx.x * BWD_ROWS_PER_BLOCK, p1 = min(p0 + BWD_ROWS_PER_BLOCK, hw);
    for (int p = p0 + wave * BWD_RU; p < p1; p += 4 * BWD_RU) {
        float4 xv[BWD_RU][MAXV];
        uint4 dr[BWD_RU];
#pragma unroll
        for (int r = 0; r < BWD_RU; ++r) {
            const bool ok = p + r < p1;
            const size_t row = (size_t)b * hw + (ok ? p + r : p);
            dr[r] = *reinterpret_cast<const uint4*>(rows + row * ldk);
#pragma unroll
            for (int i = 0; i < MAXV; ++i) {
                const int g = lane + 64 * i;
                if (g < nv) xv[r][i] = reinterpret_cast<const float4*>(x + row * C)[g];
            }
        }
#pragma unroll
        for (int r = 0; r < BWD_RU; ++r) {
            if (p + r >= p1) break;
            const size_t row = (size_t)b * hw + p + r;
            const uint32_t dw[4] = {dr[r].x, dr[r].y, dr[r].z, dr[r].w};
            float dk[G];
#pragma unroll
            for (int k = 0; k < G; ++k) dk[k] = rows_to_f32(dw[k >> 1], k & 1, rdt);
            float4 gv[MAXV];
            float s = 0.f, d = 0.f;
#pragma unroll
            for (int i = 0; i < MAXV; ++i) {
                const int g = lane + 64 * i;
                if (g < nv) {
                    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                    for (int k = 0; k < G; ++k) {
                        acc.x = __builtin_fmaf(dk[k], tf[k][i].x, acc.x); acc.y = __builtin_fmaf(dk[k], tf[k][i].y, acc.y);
                        acc.z = __builtin_fmaf(dk[k], tf[k][i].z, acc.z); acc.w = __builtin_fmaf(dk[k], tf[k][i].w, acc.w);
                    }
                    gv[i].x = round_dt(acc.x, rdt); gv[i].y = round_dt(acc.y, rdt); gv[i].z = round_dt(acc.z, rdt); gv[i].w = round_dt(acc.w, rdt);
                    if (rdt == DT_F16) {      // fp16(logit_scale * dA): the reference's d(image_features.half()) (lseg_net_zs.py:205 under autograd)
                        gv[i].x = round_f16(scale * gv[i].x); gv[i].y = round_f16(scale * gv[i].y);
                        gv[i].z = round_f16(scale * gv[i].z); gv[i].w = round_f16(scale * gv[i].w);
                    }
                    const float4 xx = xv[r][i];
                    // (the reductions of l2norm_scale_bwd_kernel, term for term)
                    s += xx.x * xx.x + xx.y * xx.y + xx.z * xx.z + xx.w * xx.w;
                    d += xx.x * gv[i].x + xx.y * gv[i].y + xx.z * gv[i].z + xx.w * gv[i].w;
                }
            }
            const float n2 = wave_sum_g(s);
            const float inv = rsqrtf(n2), proj = wave_sum_g(d) / n2;
#pragma unroll
            for (int i = 0; i < MAXV; ++i) {
                const int g = lane + 64 * i;
                if (g < nv) {
                    const float4 xx = xv[r][i];
                    const float o[4] = {post * inv * (gv[i].x - xx.x * proj), post * inv * (gv[i].y - xx.y * proj),
                                        post * inv * (gv[i].z - xx.z * proj), post * inv * (gv[i].w - xx.w * proj)};
                    uint2 pk;
                    pk.x = pack2_dt(o[0], o[1], dx_dtype);
                    pk.y = pack2_dt(o[2], o[3], dx_dtype);
                    reinterpret_cast<uint2*>(dx + row * C)[g] = pk;
                }
            }
        }
    }
}

}  // namespace

#define CHECK_LAUNCH() LSEG_HIP_TRY(hipGetLastError())

bool corr_group_supported(int G, int C) { return G >= 1 && G <= CORR_GROUP_MAX && C >= 8 && C % 8 == 0 && C <= 1024; }

int launch_corr_group_fwd(const void* a16, const void* tnorm, float* low, int B, int hw, int G, int C, hipStream_t st) {
    if (!corr_group_supported(G, C)) return set_error(LSEG_ERR_UNSUPPORTED, "grouped correlation: G=%d (1..%d), C=%d (multiple of 8, <= 1024)", G, CORR_GROUP_MAX, C);
    if (B < 1 || hw < 1) return set_error(LSEG_ERR_INVALID, "grouped correlation: B=%d hw=%d", B, hw);
    if (B > 65535) return set_error(LSEG_ERR_UNSUPPORTED, "grouped correlation: B=%d", B);
    const dim3 grid((unsigned)((hw + FWD_ROWS_PER_BLOCK - 1) / FWD_ROWS_PER_BLOCK), (unsigned)B);
    const uint16_t *a = (const uint16_t*)a16, *t = (const uint16_t*)tnorm;
#define CGF(GG, NN) hipLaunchKernelGGL((corr_group_fwd_kernel<GG, NN>), grid, dim3(256), 0, st, a, t, low, hw, C)
#define CGF_G(GG) do { if (C <= 512) CGF(GG, 1); else CGF(GG, 2); } while (0)
    switch (G) {
        case 1: CGF_G(1); break; case 2: CGF_G(2); break; case 3: CGF_G(3); break; case 4: CGF_G(4); break;
        case 5: CGF_G(5); break; case 6: CGF_G(6); break; case 7: CGF_G(7); break; default: CGF_G(8); break;
    }
#undef CGF_G
#undef CGF
    CHECK_LAUNCH();
    return 0;
}

int launch_corr_group_bwd(const void* rows, int rows_dtype, int ldk, const void* tnorm, const float* feat, void* df, int df_dtype, int B, int hw,
                          int G, int C, float scale, hipStream_t st) {
    if (!corr_group_supported(G, C) || C % 4 != 0) return set_error(LSEG_ERR_UNSUPPORTED, "grouped correlation backward: G=%d (1..%d), C=%d", G, CORR_GROUP_MAX, C);
    if (ldk < 8 || ldk % 8 != 0) return set_error(LSEG_ERR_INVALID, "grouped correlation backward: ldk=%d must be a multiple of 8", ldk);
    if (rows_dtype == DT_F32 || df_dtype == DT_F32) return set_error(LSEG_ERR_INVALID, "grouped correlation backward: 16-bit rows and df");
    if (B < 1 || hw < 1 || B > 65535) return set_error(LSEG_ERR_INVALID, "grouped correlation backward: B=%d hw=%d", B, hw);
    const dim3 grid((unsigned)((hw + BWD_ROWS_PER_BLOCK - 1) / BWD_ROWS_PER_BLOCK), (unsigned)B);
    const uint16_t *r = (const uint16_t*)rows, *t = (const uint16_t*)tnorm;
    uint16_t* o = (uint16_t*)df;
#define CGB(GG, VV) hipLaunchKernelGGL((corr_group_bwd_kernel<GG, VV>), grid, dim3(256), 0, st, r, rows_dtype, ldk, t, feat, o, df_dtype, hw, C, scale)
#define CGB_G(GG) do { if (C <= 256) CGB(GG, 1); else if (C <= 512) CGB(GG, 2); else CGB(GG, 4); } while (0)
    switch (G) {
        case 1: CGB_G(1); break; case 2: CGB_G(2); break; case 3: CGB_G(3); break; case 4: CGB_G(4); break;
        case 5: CGB_G(5); break; case 6: CGB_G(6); break; case 7: CGB_G(7); break; default: CGB_G(8); break;
    }
#undef CGB_G
#undef CGB
    CHECK_LAUNCH();
    return 0;
}

}  // namespace lseg
