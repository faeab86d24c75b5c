// ragged_train.hip -- the loss of the training step for RAGGED per-image label sets (lseg_set_text_groups in train mode): image b is
// scored against its own k_b text rows, 1 <= k_b, the lists independent of each other.  The low-resolution logit planes are
// concatenated: image b's k_b planes [k_b, h, w] start at prefix[b] * h * w floats, prefix = the exclusive prefix sum of the counts
// (device, int32 [B + 1]).  There is no rectangular [B, K, 2h, 2w] tensor on this route: the loss and its gradient are taken on the
// planes through output_conv's x2 bilinear on the fly, as the shared-set kernels of elementwise.hip do (seg_stats_kernel `up` form,
// upsample_ce_bwd_rows_kernel<false>).  These are their ragged forms, written as kernels of their own: the shared-set kernels'
// instruction streams do not change.
//
//   forward   per full-resolution pixel P of image b: z_k(P) = bilerp of plane k (k < k_b), the online log-sum-exp in ascending k, the
//             first-maximum arg-max; lse[P] saved; nll += lse - z_t for t != ignore_index, 0 <= t < k_b (a target >= k_b contributes
//             no loss, exactly as a target >= K in seg_stats_kernel); counts = {correct, labeled} with seg_stats' rule (labeled: t + 1 > 0;
//             correct: arg-max == t).  Per-class areas over local label indices mean nothing and are not produced.
//   backward  rows[(b*h*w + p), k] = sum over the 4x4 footprint of w(P -> p) * (exp(z_k(P) - lse(P)) - [k = t(P)]) * gscale / n_valid for
//             k < k_b, EXACTLY ZERO for k_b <= k < ldk: one row pitch ldk = up64(max_b k_b) for the whole batch, n_valid the BATCH count.
//
// The correlation around them has two stages.  Stage two (the default): one launch each way for the whole batch, corr_ragged_fwd_kernel
// (MFMA, planes bit-equal to stage one) and corr_ragged_bwd_kernel (dA + scale + L2-norm backward fused) below.  Stage one
// (LSEG_CORR_RAGGED_GEMM, the fallback and the yardstick): per image on the generic GEMM -- forward with round_mid = 1 into the image's
// planes; backward drows_b x T_b^T on per-image transposed text panels, then l2norm_scale_backward over all rows.
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "ops.h"
#include "../../include/lseg_hip.h"

namespace lseg {
namespace {

// the prefix sums of a launch travel as kernel arguments, 64 per launch: nothing of the caller's host memory is read after the call returns
struct RtOffsetChunk { int v[64]; };
__global__ __launch_bounds__(64) void ragged_offsets_kernel(int* __restrict__ dst, RtOffsetChunk c, int n) {
    if ((int)threadIdx.x < n) dst[threadIdx.x] = c.v[threadIdx.x];
}

__global__ __launch_bounds__(256) void ragged_ce_fwd_kernel(const float* __restrict__ low, const long long* __restrict__ target,
                                                            const int* __restrict__ prefix, int h, int w, size_t npix, int ignore_index,
                                                            unsigned long long* __restrict__ counts, double* __restrict__ nll,
                                                            float* __restrict__ lse_out) {
    double loss = 0.0;
    unsigned int nvalid = 0, ncorrect = 0, nlabeled = 0;
    const int Wo = 2 * w, HW = 4 * h * w;
    const size_t kstride = (size_t)h * w;
    const float ry = (float)(h - 1) / (float)(2 * h - 1), rx = (float)(w - 1) / (float)(2 * w - 1);
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < npix; i += (size_t)gridDim.x * blockDim.x) {
        const int p = (int)(i % HW);
        const int b = (int)(i / HW);
        const int k0 = prefix[b], K = prefix[b + 1] - k0;
        const int yo = p / Wo, xo = p - yo * Wo;
        int y0, y1, x0, x1;
        float ly, lx;
        src_tap(ry, yo, h, y0, y1, ly);
        src_tap(rx, xo, w, x0, x1, lx);
        const float* col = low + (size_t)k0 * kstride + (size_t)y0 * w + x0;
        const int o01 = x1 - x0, o10 = (y1 - y0) * w, o11 = o10 + o01;
        const long long t = target[i];
        float m = -INFINITY, ssum = 0.f, at_t = 0.f;
        int arg = 0;
        for (int k = 0; k < K; ++k) {
            const float* c = col + (size_t)k * kstride;
            const float v = bilerp(c[0], c[o01], c[o10], c[o11], lx, ly);      // upsample_bilinear2d's association (seg_stats_kernel)
            if (v > m) {                                  // first maximum wins
                ssum = ssum * __expf(m - v) + 1.f;
                m = v; arg = k;
            } else {
                ssum += __expf(v - m);
            }
            if (k == t) at_t = v;
        }
        const float lz = m + __logf(ssum);
        lse_out[i] = lz;
        if (t + 1 > 0) {                                   // metrics.py: target + 1 > 0 is a labelled pixel (seg_stats_kernel)
            ++nlabeled;
            if ((long long)arg == t) ++ncorrect;
        }
        if (t != (long long)ignore_index && t >= 0 && t < K) {
            loss += (double)(lz - at_t);
            ++nvalid;
        }
    }
    __shared__ double lred[256];
    __shared__ unsigned int nred[3][256];
    lred[threadIdx.x] = loss; nred[0][threadIdx.x] = nvalid; nred[1][threadIdx.x] = ncorrect; nred[2][threadIdx.x] = nlabeled;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            lred[threadIdx.x] += lred[threadIdx.x + s];
#pragma unroll
            for (int j = 0; j < 3; ++j) nred[j][threadIdx.x] += nred[j][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (nred[0][0]) { atomicAdd(&nll[0], lred[0]); atomicAdd(&nll[1], (double)nred[0][0]); }
        if (nred[1][0]) atomicAdd(&counts[0], (unsigned long long)nred[1][0]);
        if (nred[2][0]) atomicAdd(&counts[1], (unsigned long long)nred[2][0]);
    }
}

// one lane = one low-resolution pixel, its 3x3 neighbourhood and 4x4 footprint (upsample_ce_bwd_rows_kernel<false>, term for term), over
// the image's own k_b planes; the columns from k_b to ldk are written as zeros
__global__ __launch_bounds__(256) void ragged_ce_bwd_rows_kernel(const float* __restrict__ low, const long long* __restrict__ target,
                                                                 const float* __restrict__ lse, const double* __restrict__ nll,
                                                                 uint16_t* __restrict__ rows, const int* __restrict__ prefix, int B, int H, int W,
                                                                 int ldk, int ignore_index, int dtype, const float* __restrict__ gscale) {
    const int Ho = 2 * H, Wo = 2 * W;
    const size_t npix = (size_t)B * H * W;
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const int x = (int)(i % W);
    const int y = (int)((i / W) % H);
    const int b = (int)(i / ((size_t)W * H));
    const int kb0 = prefix[b], K = prefix[b + 1] - kb0;
    const float inv_n = (nll[1] > 0.0 ? (float)(1.0 / nll[1]) : 0.f) * (gscale ? *gscale : 1.f);
    const float ry = (float)(H - 1) / (float)(Ho - 1), rx = (float)(W - 1) / (float)(Wo - 1);
    float wy[4], ly[4], wx[4], lx[4];
    int jy[4], jx[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int yo = 2 * y - 1 + r;
        wy[r] = 0.f; ly[r] = 0.f; jy[r] = 0;
        if (yo >= 0 && yo < Ho) {
            const float sy = ry * (float)yo;
            const int y0 = (int)sy, y1 = y0 + (y0 < H - 1);
            const float l = sy - (float)y0;
            wy[r] = (y0 == y ? 1.f - l : 0.f) + (y1 == y ? l : 0.f);
            ly[r] = l; jy[r] = y0 - (y - 1);
        }
        const int xo = 2 * x - 1 + r;
        wx[r] = 0.f; lx[r] = 0.f; jx[r] = 0;
        if (xo >= 0 && xo < Wo) {
            const float sx = rx * (float)xo;
            const int x0 = (int)sx, x1 = x0 + (x0 < W - 1);
            const float l = sx - (float)x0;
            wx[r] = (x0 == x ? 1.f - l : 0.f) + (x1 == x ? l : 0.f);
            lx[r] = l; jx[r] = x0 - (x - 1);
        }
    }
    float coef[4][4], lz[4][4];
    int tl[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int yo = 2 * y - 1 + r, xo = 2 * x - 1 + c;
            coef[r][c] = 0.f; lz[r][c] = 1e30f; tl[r][c] = -1;      // inactive: exp(z - 1e30) = 0
            const float wgt = wy[r] * wx[c];
            if (wgt != 0.f) {
                const size_t pi = ((size_t)b * Ho + yo) * Wo + xo;
                const long long t = target[pi];
                if (t != (long long)ignore_index && t >= 0 && t < K) { coef[r][c] = wgt * inv_n; lz[r][c] = lse[pi]; tl[r][c] = (int)t; }
            }
        }
    const int ya = y > 0 ? y - 1 : 0, yb = y < H - 1 ? y + 1 : H - 1, xa = x > 0 ? x - 1 : 0, xb = x < W - 1 ? x + 1 : W - 1;
    const int ro[3] = {ya * W, y * W, yb * W}, co[3] = {xa, x, xb};
    const float* plane = low + (size_t)kb0 * H * W;
    uint16_t* orow = rows + i * (size_t)ldk;
    for (int k0 = 0; k0 < ldk; k0 += 8) {
        float out[8];
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
            const int k = k0 + kk;
            float acc = 0.f;
            if (k < K) {
                const float* pl = plane + (size_t)k * H * W;
                float L[3][3];
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int c = 0; c < 3; ++c) L[a][c] = pl[ro[a] + co[c]];
                float Hc[3][4];
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        const float p0 = jx[c] ? L[a][1] : L[a][0], p1 = jx[c] ? L[a][2] : L[a][1];
                        Hc[a][c] = (1.f - lx[c]) * p0 + lx[c] * p1;
                    }
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const float q0 = jy[r] ? Hc[1][c] : Hc[0][c], q1 = jy[r] ? Hc[2][c] : Hc[1][c];
                        const float z = (1.f - ly[r]) * q0 + ly[r] * q1;
                        acc += coef[r][c] * (__expf(z - lz[r][c]) - (tl[r][c] == k ? 1.f : 0.f));
                    }
            }
            out[kk] = acc;
        }
        *reinterpret_cast<uint4*>(orow + k0) = make_uint4(pack2_dt(out[0], out[1], dtype), pack2_dt(out[2], out[3], dtype),
                                                          pack2_dt(out[4], out[5], dtype), pack2_dt(out[6], out[7], dtype));
    }
}

// ---- stage two: the correlation of the whole batch in ONE launch each way -----------------------------------------------------------
// forward: a workgroup = 64 pixel rows of one image (grid.y = image), a wave = 16 of them.  The pixel rows are read ONCE, as the MFMA
// operand fragments of the wave (C / 32 x 16 bytes per lane, resident for the life of the wave); the image's text rows stream through LDS
// in panels of 16 labels (a 2-label list wastes 14 of 16 MFMA rows of one panel, nothing more).  Operand roles and k order are the generic
// GEMM's (gemm.hip: acc = mfma(W fragment, A fragment, acc) over ascending 32-wide k-steps): A operand = text rows, B operand = pixel
// rows, v_mfma_f32_16x16x32_f16, fp32 accumulation from zero, one fp16 rounding per logit -- the planes are bit-equal to stage one.
//   LDS: 16 rows of C + 8 halves (the 16-byte pad staggers the rows over the banks for the 16-byte fragment reads).
constexpr int RT_PANEL = 16, RT_FWD_ROWS = 64, RT_BWD_ROWS = 16, RT_BWD_RU = 4;

template <int MAXKS>
__global__ __launch_bounds__(256) void corr_ragged_fwd_kernel(const uint16_t* __restrict__ a, const uint16_t* __restrict__ t,
                                                              float* __restrict__ low, const int* __restrict__ prefix, int hw, int C) {
    __shared__ uint4 tl4[RT_PANEL * (1024 + 8) / 8];
    uint16_t* tl = reinterpret_cast<uint16_t*>(tl4);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y;
    const int k0g = prefix[b], K = prefix[b + 1] - k0g;
    const int nks = C >> 5, pitch = C + 8, n16 = C >> 3;
    const int pix = blockIdx.x * RT_FWD_ROWS + wave * 16 + (lane & 15), kq = lane >> 4;
    const bool pok = pix < hw;
    i32x4_t pf[MAXKS];
    const uint16_t* arow = a + ((size_t)b * hw + (pok ? pix : hw - 1)) * C + kq * 8;
#pragma unroll
    for (int ks = 0; ks < MAXKS; ++ks) {
        pf[ks] = i32x4_t{0, 0, 0, 0};
        if (ks < nks && pok) pf[ks] = *reinterpret_cast<const i32x4_t*>(arow + ks * 32);
    }
    float* lb = low + (size_t)k0g * hw;
    for (int kp = 0; kp < K; kp += RT_PANEL) {
        __syncthreads();                                   // the previous panel's fragment reads are done
        for (int idx = tid; idx < RT_PANEL * n16; idx += 256) {
            const int r = idx / n16, c = idx - r * n16;
            uint4 v = make_uint4(0, 0, 0, 0);              // labels past the list: zero rows, their outputs are not stored
            if (kp + r < K) v = reinterpret_cast<const uint4*>(t + (size_t)(k0g + kp + r) * C)[c];
            *reinterpret_cast<uint4*>(tl + r * pitch + c * 8) = v;
        }
        __syncthreads();
        f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
        const uint16_t* trow = tl + (lane & 15) * pitch + kq * 8;
#pragma unroll
        for (int ks = 0; ks < MAXKS; ++ks)
            if (ks < nks) acc = mfma16<F16>(*reinterpret_cast<const i32x4_t*>(trow + ks * 32), pf[ks], acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) {                      // D: lane l, reg r -> label kp + (l >> 4) * 4 + r, pixel l & 15
            const int label = kp + kq * 4 + r;
            if (label < K && pok) lb[(size_t)label * hw + pix] = round_f16(acc[r]);
        }
    }
}

__device__ __forceinline__ float rt_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float rt_round_dt(float v, int dtype) { return dtype == DT_F16 ? round_f16(v) : bf16_to_f32(f32_to_bf16(v)); }
__device__ __forceinline__ float rt_half_of(uint32_t w, int hi) { return f16_to_f32((uint16_t)(hi ? (w >> 16) : (w & 0xffffu))); }

// backward: dA = sum over the image's labels (ascending) of d[row, k] T[k, :] in fp32 fused multiply-adds on exactly converted operands,
// rounded once to the rows' type, then the scale and the L2-norm backward against the saved fp32 feature row -- corr_group_bwd_kernel
// (corr_group.hip) with a run-time label count: the same lane layout (lane owns the float4 chunks lane + 64 i of the row), the same
// roundings (fp16 rows: fp16(scale * fp16(dA)); bf16 rows: T rounded to bf16, the scale un-rounded) and the row reductions in that
// kernel's order, term for term.  A workgroup = 16 pixel rows of one image, 4 per wave, their accumulators resident; the text rows stream
// through LDS in panels of 16 labels (fp16, 32 KB at C = 1024), read as 8 bytes per lane and chunk (consecutive lanes, no bank conflict).
// No dA round trip through memory, no transposed text panels.
template <int MAXV>
__global__ __launch_bounds__(256) void corr_ragged_bwd_kernel(const uint16_t* __restrict__ rows, int rdt, int ldk, const uint16_t* __restrict__ t,
                                                              const float* __restrict__ x, uint16_t* __restrict__ dx, int dx_dtype,
                                                              const int* __restrict__ prefix, int hw, int C, float scale) {
    __shared__ uint4 tl4[RT_PANEL * 1024 / 8];
    uint16_t* tl = reinterpret_cast<uint16_t*>(tl4);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y;
    const int k0g = prefix[b], K = prefix[b + 1] - k0g;
    const int nv = C >> 2, n16 = C >> 3;
    const int p0 = blockIdx.x * RT_BWD_ROWS + wave * RT_BWD_RU;
    float4 acc[RT_BWD_RU][MAXV];
#pragma unroll
    for (int r = 0; r < RT_BWD_RU; ++r)
#pragma unroll
        for (int i = 0; i < MAXV; ++i) acc[r][i] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int kp = 0; kp < K; kp += RT_PANEL) {
        __syncthreads();
        for (int idx = tid; idx < RT_PANEL * n16; idx += 256) {
            const int r = idx / n16, c = idx - r * n16;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (kp + r < K) v = reinterpret_cast<const uint4*>(t + (size_t)(k0g + kp + r) * C)[c];
            if (rdt != DT_F16) {       // T in the rows' type: the bf16 rounding of an fp16 value (fewer significant bits) is an fp16 value again
                uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    w[j] = pack2<F16>(rt_round_dt(rt_half_of(w[j], 0), rdt), rt_round_dt(rt_half_of(w[j], 1), rdt));
                v = make_uint4(w[0], w[1], w[2], w[3]);
            }
            *reinterpret_cast<uint4*>(tl + r * C + c * 8) = v;
        }
        __syncthreads();
        float dk[RT_BWD_RU][RT_PANEL];
#pragma unroll
        for (int r = 0; r < RT_BWD_RU; ++r) {
            const int p = p0 + r < hw ? p0 + r : hw - 1;
            const uint4* dr = reinterpret_cast<const uint4*>(rows + ((size_t)b * hw + p) * ldk + kp);       // kp + 16 <= up64(K) <= ldk
            const uint4 d0 = dr[0], d1 = dr[1];
            const uint32_t dw[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
#pragma unroll
            for (int k = 0; k < RT_PANEL; ++k) {
                const uint16_t h = (uint16_t)((k & 1) ? (dw[k >> 1] >> 16) : (dw[k >> 1] & 0xffffu));
                dk[r][k] = rdt == DT_F16 ? f16_to_f32(h) : bf16_to_f32(h);
            }
        }
#pragma unroll
        for (int k = 0; k < RT_PANEL; ++k) {               // ascending labels; rows past the list are zeros against zero columns of d
#pragma unroll
            for (int i = 0; i < MAXV; ++i) {
                const int g = lane + 64 * i;
                if (g < nv) {
                    const uint2 u = reinterpret_cast<const uint2*>(tl + k * C)[g];
                    const float t0 = rt_half_of(u.x, 0), t1 = rt_half_of(u.x, 1), t2 = rt_half_of(u.y, 0), t3 = rt_half_of(u.y, 1);
#pragma unroll
                    for (int r = 0; r < RT_BWD_RU; ++r) {
                        acc[r][i].x = __builtin_fmaf(dk[r][k], t0, acc[r][i].x); acc[r][i].y = __builtin_fmaf(dk[r][k], t1, acc[r][i].y);
                        acc[r][i].z = __builtin_fmaf(dk[r][k], t2, acc[r][i].z); acc[r][i].w = __builtin_fmaf(dk[r][k], t3, acc[r][i].w);
                    }
                }
            }
        }
    }
    const float post = rdt == DT_F16 ? 1.f : scale;
#pragma unroll
    for (int r = 0; r < RT_BWD_RU; ++r) {
        if (p0 + r >= hw) break;                           // wave-uniform
        const size_t row = (size_t)b * hw + p0 + r;
        float4 gv[MAXV], xv[MAXV];
        float s = 0.f, d = 0.f;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int g = lane + 64 * i;
            if (g < nv) {
                xv[i] = reinterpret_cast<const float4*>(x + row * C)[g];
                gv[i].x = rt_round_dt(acc[r][i].x, rdt); gv[i].y = rt_round_dt(acc[r][i].y, rdt);
                gv[i].z = rt_round_dt(acc[r][i].z, rdt); gv[i].w = rt_round_dt(acc[r][i].w, rdt);
                if (rdt == DT_F16) {
                    gv[i].x = round_f16(scale * gv[i].x); gv[i].y = round_f16(scale * gv[i].y);
                    gv[i].z = round_f16(scale * gv[i].z); gv[i].w = round_f16(scale * gv[i].w);
                }
                const float4 xx = xv[i];
                s += xx.x * xx.x + xx.y * xx.y + xx.z * xx.z + xx.w * xx.w;
                d += xx.x * gv[i].x + xx.y * gv[i].y + xx.z * gv[i].z + xx.w * gv[i].w;
            }
        }
        const float n2 = rt_wave_sum(s);
        const float inv = rsqrtf(n2), proj = rt_wave_sum(d) / n2;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int g = lane + 64 * i;
            if (g < nv) {
                const float4 xx = xv[i];
                uint2 pk;
                pk.x = pack2_dt(post * inv * (gv[i].x - xx.x * proj), post * inv * (gv[i].y - xx.y * proj), dx_dtype);
                pk.y = pack2_dt(post * inv * (gv[i].z - xx.z * proj), post * inv * (gv[i].w - xx.w * proj), dx_dtype);
                reinterpret_cast<uint2*>(dx + row * C)[g] = pk;
            }
        }
    }
}

int rt_fwd_grid(int B, int h, int w) { return (int)std::min<size_t>(((size_t)B * 4 * h * w + 255) / 256, 256 * 16); }

}  // namespace

#define CHECK_LAUNCH() LSEG_HIP_TRY(hipGetLastError())

// prefix [B + 1] (host) = exclusive prefix sum of the validated counts; kmax = the largest count
int ragged_prefix(const int32_t* host_counts, int B, int* prefix, int& kmax) {
    if (!host_counts || !prefix) return set_error(LSEG_ERR_INVALID, "ragged label sets: NULL counts");
    if (B < 1 || B > 65535) return set_error(LSEG_ERR_INVALID, "ragged label sets: B=%d", B);
    prefix[0] = 0;
    kmax = 0;
    for (int b = 0; b < B; ++b) {
        if (host_counts[b] < 1 || host_counts[b] > 32767)
            return set_error(LSEG_ERR_INVALID, "ragged label sets: image %d has %d labels, outside [1, 32767]", b, host_counts[b]);
        if ((long)prefix[b] + host_counts[b] > (1L << 24)) return set_error(LSEG_ERR_INVALID, "ragged label sets: more than 2^24 labels in all");
        prefix[b + 1] = prefix[b] + host_counts[b];
        kmax = std::max(kmax, (int)host_counts[b]);
    }
    return 0;
}

// out8 = {labels in all, largest count, row pitch of drows = up64(largest count), workgroups of the forward, workgroups of the backward,
//         lanes per workgroup, columns of the per-image transposed text panels in all = sum of up64(k_b), fp32 values of the planes}
int ragged_ce_plan(const int32_t* host_counts, int B, int h, int w, int* out8) {
    if (!out8) return set_error(LSEG_ERR_INVALID, "ragged_ce_plan: NULL pointer");
    if (B < 1 || B > 65535) return set_error(LSEG_ERR_INVALID, "ragged label sets: B=%d", B);
    std::vector<int> prefix((size_t)B + 1, 0);
    int kmax = 0;
    if (const int r = ragged_prefix(host_counts, B, prefix.data(), kmax)) return r;
    if (h < 2 || w < 2) return set_error(LSEG_ERR_INVALID, "ragged_ce_plan: h=%d w=%d", h, w);
    if ((size_t)prefix[B] * h * w >= ((size_t)1 << 31)) return set_error(LSEG_ERR_UNSUPPORTED, "ragged_ce_plan: %d planes of %dx%d exceed 2^31 values", prefix[B], h, w);
    long panel_cols = 0;
    for (int b = 0; b < B; ++b) panel_cols += (host_counts[b] + 63) / 64 * 64;
    out8[0] = prefix[B]; out8[1] = kmax; out8[2] = (kmax + 63) / 64 * 64;
    out8[3] = rt_fwd_grid(B, h, w);
    out8[4] = (int)(((size_t)B * h * w + 255) / 256);
    out8[5] = 256;
    out8[6] = (int)panel_cols;
    out8[7] = prefix[B] * h * w;
    return 0;
}

int launch_ragged_offsets(int* d_prefix, const int* host_prefix, int n, hipStream_t st) {
    for (int i0 = 0; i0 < n; i0 += 64) {
        RtOffsetChunk ch;
        const int m = std::min(64, n - i0);
        for (int i = 0; i < 64; ++i) ch.v[i] = i < m ? host_prefix[i0 + i] : 0;
        hipLaunchKernelGGL(ragged_offsets_kernel, dim3(1), dim3(64), 0, st, d_prefix + i0, ch, m);
        CHECK_LAUNCH();
    }
    return 0;
}

// low: the concatenated planes (see the head of the file); target int64 [B, 2h, 2w]; d_prefix int32 [B + 1] already on the device;
// counts2 {correct, labeled}, nll {sum, valid}: zeroed here; lse_out fp32 [B, 2h, 2w]
int launch_ragged_ce_fwd(const float* low, const int64_t* target, const int* d_prefix, int B, int h, int w, int ignore_index,
                         unsigned long long* counts2, double* nll, float* lse_out, hipStream_t st) {
    if (!low || !target || !d_prefix || !counts2 || !nll || !lse_out) return set_error(LSEG_ERR_INVALID, "ragged_ce_fwd: NULL pointer");
    if (B < 1 || h < 2 || w < 2) return set_error(LSEG_ERR_INVALID, "ragged_ce_fwd: B=%d h=%d w=%d", B, h, w);
    LSEG_HIP_TRY(hipMemsetAsync(counts2, 0, 2 * sizeof(unsigned long long), st));
    LSEG_HIP_TRY(hipMemsetAsync(nll, 0, 2 * sizeof(double), st));
    const size_t npix = (size_t)B * 4 * h * w;
    hipLaunchKernelGGL(ragged_ce_fwd_kernel, dim3(rt_fwd_grid(B, h, w)), dim3(256), 0, st, low, reinterpret_cast<const long long*>(target), d_prefix,
                       h, w, npix, ignore_index, counts2, nll, lse_out);
    CHECK_LAUNCH();
    return 0;
}

// rows: [B*h*w, ldk] fp16 / bf16, every column written (zeros from the image's count on); ldk % 8 == 0 and >= the largest count (the
// caller's to guarantee: the device counts are not read back)
int launch_ragged_ce_bwd_rows(const float* low, const int64_t* target, const float* lse, const double* nll, void* rows, const int* d_prefix,
                              int B, int h, int w, int ldk, int ignore_index, int dtype, hipStream_t st, const float* gscale) {
    if (!low || !target || !lse || !nll || !rows || !d_prefix) return set_error(LSEG_ERR_INVALID, "ragged_ce_bwd_rows: NULL pointer");
    if (B < 1 || h < 2 || w < 2) return set_error(LSEG_ERR_INVALID, "ragged_ce_bwd_rows: B=%d h=%d w=%d", B, h, w);
    if (ldk < 8 || (ldk & 7)) return set_error(LSEG_ERR_INVALID, "ragged_ce_bwd_rows: ldk=%d must be a multiple of 8", ldk);
    if (dtype != DT_F16 && dtype != DT_BF16) return set_error(LSEG_ERR_INVALID, "ragged_ce_bwd_rows: 16-bit rows");
    if (!x2_footprint_is_4(h) || !x2_footprint_is_4(w)) return set_error(LSEG_ERR_UNSUPPORTED, "ragged_ce_bwd_rows: %dx%d map outside the 4-tap footprint", h, w);
    const size_t npix = (size_t)B * h * w;
    hipLaunchKernelGGL(ragged_ce_bwd_rows_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, low,
                       reinterpret_cast<const long long*>(target), lse, nll, (uint16_t*)rows, d_prefix, B, h, w, ldk, ignore_index, dtype, gscale);
    CHECK_LAUNCH();
    return 0;
}

// ---- the per-image correlation around the loss kernels, on the generic GEMM (the engine's route and lseg_op_corr_ragged_*) -----------
bool corr_ragged_supported(int C) { return C >= 64 && C % 64 == 0 && C <= 1024; }

// out8 = {GEMM launches of the stage-one forward (B), launches of the stage-one backward (B GEMMs + one L2-norm backward), columns of the
//         transposed text panels (sum of up64(k_b)), row pitch of d(low) rows up64(largest count), labels in all, elements of the dA
//         scratch B*hw*C, workgroups of the one-launch forward (64 pixel rows each), workgroups of the one-launch backward (16 each)}
int corr_ragged_plan(const int32_t* host_counts, int B, int hw, int C, int* out6) {
    if (!out6) return set_error(LSEG_ERR_INVALID, "corr_ragged_plan: NULL pointer");
    if (B < 1 || B > 65535 || hw < 1) return set_error(LSEG_ERR_INVALID, "corr_ragged_plan: B=%d hw=%d", B, hw);
    if (!corr_ragged_supported(C)) return set_error(LSEG_ERR_UNSUPPORTED, "ragged correlation: C=%d (multiple of 64, <= 1024)", C);
    std::vector<int> prefix((size_t)B + 1, 0);
    int kmax = 0;
    if (const int r = ragged_prefix(host_counts, B, prefix.data(), kmax)) return r;
    if ((double)B * hw * C >= 2.0e9) return set_error(LSEG_ERR_UNSUPPORTED, "corr_ragged_plan: B*hw*C exceeds 2^31");
    size_t cols = 0;
    for (int b = 0; b < B; ++b) cols += up64(host_counts[b]);
    out6[0] = B; out6[1] = B + 1; out6[2] = (int)cols; out6[3] = (int)up64(kmax); out6[4] = prefix[B]; out6[5] = B * hw * C;
    out6[6] = B * ((hw + RT_FWD_ROWS - 1) / RT_FWD_ROWS); out6[7] = B * ((hw + RT_BWD_ROWS - 1) / RT_BWD_ROWS);
    return 0;
}

// LSEG_CORR_RAGGED_GEMM (any value): the A/B switch -- the ragged correlation on stage one, the per-image launches of the generic GEMM
// (the fallback and the yardstick), instead of the one-launch kernels
bool corr_ragged_use_gemm() {
    static const bool v = getenv("LSEG_CORR_RAGGED_GEMM") != nullptr;
    return v;
}

// stage two, forward: one launch for the batch.  d_prefix int32 [B + 1] on the device; kmax = the largest count (grid sizing is per pixel)
int launch_corr_ragged_fwd_fused(const void* a16, const void* tnorm, float* low, const int* d_prefix, int B, int hw, int C, hipStream_t st) {
    if (!a16 || !tnorm || !low || !d_prefix) return set_error(LSEG_ERR_INVALID, "corr_ragged_fwd: NULL pointer");
    if (!corr_ragged_supported(C)) return set_error(LSEG_ERR_UNSUPPORTED, "ragged correlation: C=%d (multiple of 64, <= 1024)", C);
    if (B < 1 || B > 65535 || hw < 1) return set_error(LSEG_ERR_INVALID, "corr_ragged_fwd: B=%d hw=%d", B, hw);
    const dim3 grid((unsigned)((hw + RT_FWD_ROWS - 1) / RT_FWD_ROWS), (unsigned)B);
    const uint16_t *a = (const uint16_t*)a16, *t = (const uint16_t*)tnorm;
#define RTF(N) hipLaunchKernelGGL((corr_ragged_fwd_kernel<N>), grid, dim3(256), 0, st, a, t, low, d_prefix, hw, C)
    if (C <= 256) RTF(8); else if (C <= 512) RTF(16); else RTF(32);
#undef RTF
    CHECK_LAUNCH();
    return 0;
}

// stage two, backward: rows [B*hw, ldk] -> df [B*hw, C] in one launch; ldk % 16 == 0 and >= the largest count rounded up to 16
int launch_corr_ragged_bwd_fused(const void* rows, int rows_dtype, int ldk, const void* tnorm, const float* feat, void* df, int df_dtype,
                                 const int* d_prefix, int kmax, int B, int hw, int C, float scale, hipStream_t st) {
    if (!rows || !tnorm || !feat || !df || !d_prefix) return set_error(LSEG_ERR_INVALID, "corr_ragged_bwd: NULL pointer");
    if (!corr_ragged_supported(C)) return set_error(LSEG_ERR_UNSUPPORTED, "ragged correlation: C=%d (multiple of 64, <= 1024)", C);
    if (rows_dtype == DT_F32 || df_dtype == DT_F32) return set_error(LSEG_ERR_INVALID, "corr_ragged_bwd: 16-bit rows and df");
    if (ldk % RT_PANEL != 0 || ldk < (kmax + RT_PANEL - 1) / RT_PANEL * RT_PANEL)
        return set_error(LSEG_ERR_INVALID, "corr_ragged_bwd: ldk=%d must be a multiple of 16 and cover the largest count %d", ldk, kmax);
    if (B < 1 || B > 65535 || hw < 1) return set_error(LSEG_ERR_INVALID, "corr_ragged_bwd: B=%d hw=%d", B, hw);
    const dim3 grid((unsigned)((hw + RT_BWD_ROWS - 1) / RT_BWD_ROWS), (unsigned)B);
    const uint16_t *r = (const uint16_t*)rows, *t = (const uint16_t*)tnorm;
    uint16_t* o = (uint16_t*)df;
#define RTB(V) hipLaunchKernelGGL((corr_ragged_bwd_kernel<V>), grid, dim3(256), 0, st, r, rows_dtype, ldk, t, feat, o, df_dtype, d_prefix, hw, C, scale)
    if (C <= 256) RTB(1); else if (C <= 512) RTB(2); else RTB(4);
#undef RTB
    CHECK_LAUNCH();
    return 0;
}

// low (concatenated planes, image b's at prefix[b] * hw) = fp16(a16_b [hw, C] . tnorm_b [k_b, C]^T), fp32 accumulation, one fp16 rounding
// per logit: B launches of the generic GEMM with round_mid = 1, the shared label set's rounding points
int launch_corr_ragged_fwd(const void* a16, const void* tnorm, float* low, const int* host_prefix, int B, int hw, int C, hipStream_t st) {
    if (!a16 || !tnorm || !low || !host_prefix) return set_error(LSEG_ERR_INVALID, "corr_ragged_fwd: NULL pointer");
    if (!corr_ragged_supported(C)) return set_error(LSEG_ERR_UNSUPPORTED, "ragged correlation: C=%d (multiple of 64, <= 1024)", C);
    for (int b = 0; b < B; ++b) {
        GemmArgs g;
        gemm_args_init(g);
        g.A = (const uint16_t*)a16 + (size_t)b * hw * C; g.W = (const uint16_t*)tnorm + (size_t)host_prefix[b] * C;
        g.M = hw; g.N = host_prefix[b + 1] - host_prefix[b]; g.K = C; g.lda = C; g.ldw = C;
        g.round_mid = 1; g.C = low + (size_t)host_prefix[b] * hw; g.out_dtype = DT_F32; g.map_mode = MAP_NCHW; g.p_div = hw;
        if (const int r = launch_gemm(g, DT_F16, st)) return r;
    }
    return 0;
}

// the dgrad operands: per-image transposed text panels [C, up64(k_b)], concatenated, zero in the pad columns.  tsrc: the text rows in the
// rows' type (fp16 as they are, or their bf16 rounding)
int launch_corr_ragged_panels(const void* tsrc, void* tnT, const int* host_prefix, int B, int C, hipStream_t st) {
    if (!tsrc || !tnT || !host_prefix) return set_error(LSEG_ERR_INVALID, "corr_ragged_panels: NULL pointer");
    size_t cols = 0;
    for (int b = 0; b < B; ++b) cols += up64(host_prefix[b + 1] - host_prefix[b]);
    LSEG_HIP_TRY(hipMemsetAsync(tnT, 0, cols * C * 2, st));
    cols = 0;
    for (int b = 0; b < B; ++b) {
        const int kb = host_prefix[b + 1] - host_prefix[b], Kpb = (int)up64(kb);
        if (const int r = launch_transpose16((const uint16_t*)tsrc + (size_t)host_prefix[b] * C, (uint16_t*)tnT + cols * C, kb, C, C, Kpb, st)) return r;
        cols += Kpb;
    }
    return 0;
}

// dA_b = rows_b [hw, ldk] . T_b per image on its panel (K = up64(k_b) <= ldk: the columns beyond are zeros and are not read) into da
// [B*hw, C] (rows' type), then the scale and L2-norm backward over all rows at once: df [B*hw, C].  zero_bias: C fp32 zeros
int launch_corr_ragged_bwd(const void* rows, int rows_dtype, int ldk, const void* tnT, const float* zero_bias, const float* feat, void* da,
                           void* df, int df_dtype, const int* host_prefix, int B, int hw, int C, float scale, hipStream_t st) {
    if (!rows || !tnT || !zero_bias || !feat || !da || !df || !host_prefix) return set_error(LSEG_ERR_INVALID, "corr_ragged_bwd: NULL pointer");
    if (!corr_ragged_supported(C)) return set_error(LSEG_ERR_UNSUPPORTED, "ragged correlation: C=%d (multiple of 64, <= 1024)", C);
    if (rows_dtype == DT_F32 || df_dtype == DT_F32) return set_error(LSEG_ERR_INVALID, "corr_ragged_bwd: 16-bit rows and df");
    if (ldk < 64 || ldk % 64 != 0) return set_error(LSEG_ERR_INVALID, "corr_ragged_bwd: ldk=%d must be a multiple of 64", ldk);
    size_t cols = 0;
    for (int b = 0; b < B; ++b) {
        const int Kpb = (int)up64(host_prefix[b + 1] - host_prefix[b]);
        if (Kpb > ldk) return set_error(LSEG_ERR_INVALID, "corr_ragged_bwd: ldk=%d < up64 of image %d's count", ldk, b);
        GemmArgs g;
        gemm_args_init(g);
        g.A = (const uint16_t*)rows + (size_t)b * hw * ldk; g.W = (const uint16_t*)tnT + cols * C;
        g.M = hw; g.N = C; g.K = Kpb; g.lda = ldk; g.ldw = Kpb; g.bias = zero_bias;
        g.C = (uint16_t*)da + (size_t)b * hw * C; g.out_dtype = rows_dtype; g.ldc = C; g.map_mode = MAP_LINEAR;
        if (const int r = launch_gemm(g, rows_dtype, st)) return r;
        cols += Kpb;
    }
    return launch_l2norm_scale_backward(da, rows_dtype, feat, df, df_dtype, B * hw, C, scale, st);
}

}  // namespace lseg
