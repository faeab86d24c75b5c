// head_train.hip -- the arch_option 1/2 head blocks (modules/models/lseg_net.py:43-79, applied at :198-201) on the TRAINING path.
//
// One shared module runs n = max(block_depth - 1, 0) + 1 times on the fp32 label planes x_0 = the correlation output [B,K,h,w]:
//   z_j = conv3x3_1ch(x_j; w, b) (+ max_k x_j[b,:,p] for the bottleneck),   x_{j+1} = act(z_j) for j < n-1,  x_n = z_{n-1}
// The forward keeps every x_{j+1} and, for the bottleneck, the index k*_j[b,p] of the FIRST maximal label of x_j (what torch.max(dim=1)
// returns and routes its gradient to).  The backward of block j takes dz_j (the gradient of its pre-activation) and
//   dx_j[p]   = sum_t w[t] dz_j[p - t]  (zero padded)  + [k = k*_j[p]] S_j[p],      S_j[p] = sum_k dz_j[b,k,p]
//   dW[t]    += sum_{b,k,p} dz_j[b,k,p] x_j[b,k,p + t],   db += sum dz_j
// and hands the block below either dz_{j-1} = act'(x_j) dx_j (fp32 planes, x_j being block j-1's saved output) together with S_{j-1},
// or -- block 0 -- dx_0 straight in the 16-bit row layout [B*h*w, ldk] the correlation backward consumes: the rounding of the `.float()`
// of lseg_net.py:196 under autograd and the planes -> rows re-layout in the same store.  The last block's dz = d(out) and its S come
// from the fused CE backward (elementwise.hip, upsample_ce_bwd_rows_kernel<true>) or, on the d(logits) hand-over path, from
// upsample2x_planes_bwd_rows_kernel<true> + head_bwd_prep_kernel.
//
// All stencil kernels here are HBM streams over [B,K,h,w] planes (276 MB per plane set at B = 8, K = 150, 480x480).  The block
// backward tiles 64 x 4 pixels of one image per workgroup and walks the labels in chunks of 8: each chunk's dz and x tiles (+1 halo)
// go through LDS, so every plane element is read from memory once per chunk however many taps use it; each lane owns one pixel for all
// labels, which keeps k*, S and the 10 weight-gradient partial sums in registers.  The weight gradient leaves as one partial row per
// workgroup (wave shuffles + a fixed LDS order) and head_dw_reduce_kernel sums the rows of all n blocks in a fixed order: no atomics,
// the same step twice gives the same bits.
#include "ops.h"
#include "../../include/lseg_hip.h"

namespace lseg {
namespace {

constexpr int TX = 64, TY = 4, KC = 8;             // pixel tile of a workgroup (256 lanes), labels per LDS chunk
constexpr int HX = TX + 2, HY = TY + 2, HP = HX * HY;

__device__ __forceinline__ float act_fwd(float v, int act) {
    if (act == 0) return fmaxf(v, 0.f);
    if (act == 1) return v > 0.f ? v : 0.01f * v;
    return tanhf(v);
}
// autograd's backward of the activation in terms of its OUTPUT y (relu: threshold_backward on the result; leaky_relu: y > 0 iff its input
// is; tanh: tanh_backward = g * (1 - y^2))
__device__ __forceinline__ float act_bwd(float g, float y, int act) {
    if (act == 0) return y > 0.f ? g : 0.f;
    if (act == 1) return y > 0.f ? g : g * 0.01f;
    return g * (1.f - y * y);
}

__device__ __forceinline__ float wave_sum_h(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// train-mode forward of one block: the inference kernel's arithmetic (elementwise.hip, head_block_kernel: same operation order, so the
// same bits), plus the first arg-max label of the input per pixel for the bottleneck's backward
__global__ void head_block_train_fwd_kernel(const float* __restrict__ in, float* __restrict__ out, int* __restrict__ kstar,
                                            const float* __restrict__ w9, const float* __restrict__ bias, int B, int K, int H, int W,
                                            int bottleneck, int act, int apply_act) {
    const size_t n = (size_t)B * H * W;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % W);
        const int y = (int)((i / W) % H);
        const int b = (int)(i / ((size_t)W * H));
        float mx = -INFINITY, best = -INFINITY;
        int bi = 0;
        if (bottleneck)
            for (int k = 0; k < K; ++k) {
                const float v = in[(((size_t)b * K + k) * H + y) * W + x];
                mx = fmaxf(mx, v);
                if (v > best) { best = v; bi = k; }
            }
        if (bottleneck && kstar) kstar[i] = bi;
        for (int k = 0; k < K; ++k) {
            const float* pl = in + ((size_t)b * K + k) * H * W;
            float acc = bias[0];
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    const int yy = y + dy, xx = x + dx;
                    if (yy >= 0 && yy < H && xx >= 0 && xx < W) acc += w9[(dy + 1) * 3 + dx + 1] * pl[(size_t)yy * W + xx];
                }
            if (bottleneck) acc += mx;
            if (apply_act) acc = act_fwd(acc, act);
            out[(((size_t)b * K + k) * H + y) * W + x] = acc;
        }
    }
}

// per pixel: dz = act'(y) dy (apply_act) or dy, written to dz (optional, may alias dy); S = sum_k dz (optional); k* = first arg-max
// label of x (optional).  The one-block op's front end and the hand-over path's S.
__global__ void head_bwd_prep_kernel(const float* dy, const float* __restrict__ y, const float* __restrict__ x, float* dz,
                                     float* __restrict__ ksum, int* __restrict__ kstar, int B, int K, int HW, int act, int apply_act) {
    const size_t n = (size_t)B * HW;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t b = i / HW, p = i % HW;
        float s = 0.f, best = -INFINITY;
        int bi = 0;
        for (int k = 0; k < K; ++k) {
            const size_t e = (b * K + k) * HW + p;
            float g = dy[e];
            if (apply_act) g = act_bwd(g, y[e], act);
            if (dz) dz[e] = g;
            s += g;
            if (kstar) {
                const float v = x[e];
                if (v > best) { best = v; bi = k; }
            }
        }
        if (ksum) ksum[i] = s;
        if (kstar) kstar[i] = bi;
    }
}

// backward of one block (see the file comment).  out_dtype DT_F32: fp32 planes [B,K,H,W] (optionally times act'(x) of the block below,
// lower_act >= 0, with their label sums in ksum_out); else 16-bit rows [B*H*W, ldk], every column written (zeros from K on).
// partial[blockIdx][10] = this workgroup's {dW[0..8], db}.
__global__ __launch_bounds__(256) void head_block_bwd_kernel(const float* __restrict__ dz, const float* __restrict__ ksum,
                                                             const int* __restrict__ kstar, const float* __restrict__ x,
                                                             const float* __restrict__ w9, void* __restrict__ out, int out_dtype, int ldk,
                                                             int lower_act, float* __restrict__ ksum_out, float* __restrict__ partial,
                                                             int B, int K, int H, int W, int bottleneck) {
    __shared__ float sdz[KC][HP], sx[KC][HP];
    __shared__ float red[4][10];
    const int tid = threadIdx.x, tx = tid % TX, ty = tid / TX;
    const int tiles_x = (W + TX - 1) / TX, tiles_y = (H + TY - 1) / TY;
    const int bt = blockIdx.x;
    const int b = bt / (tiles_x * tiles_y), t = bt % (tiles_x * tiles_y);
    const int y0 = (t / tiles_x) * TY, x0 = (t % tiles_x) * TX;
    const int px = x0 + tx, py = y0 + ty;
    const bool valid = px < W && py < H;
    const size_t HW = (size_t)H * W, pix = valid ? (size_t)py * W + px : 0;
    const size_t bpix = (size_t)b * HW + pix;
    float wt[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) wt[q] = w9[q];
    int ks = -1;
    float S = 0.f;
    if (bottleneck && valid) { ks = kstar[bpix]; S = ksum[bpix]; }
    float dw[9], db = 0.f, so = 0.f;
#pragma unroll
    for (int q = 0; q < 9; ++q) dw[q] = 0.f;
    const bool rows = out_dtype != DT_F32;
    const int K8 = (K + KC - 1) / KC * KC;
    for (int k0 = 0; k0 < K8; k0 += KC) {
        __syncthreads();                                // the previous chunk's readers are done
        for (int e = tid; e < KC * HP; e += 256) {
            const int kk = e / HP, r = e - kk * HP;
            const int ly = r / HX, lx = r - ly * HX;
            const int gy = y0 + ly - 1, gx = x0 + lx - 1, k = k0 + kk;
            float vz = 0.f, vx = 0.f;
            if (k < K && gy >= 0 && gy < H && gx >= 0 && gx < W) {
                const size_t o = ((size_t)b * K + k) * HW + (size_t)gy * W + gx;
                vz = dz[o]; vx = x[o];
            }
            sdz[kk][r] = vz; sx[kk][r] = vx;
        }
        __syncthreads();
        float o8[KC];
#pragma unroll
        for (int kk = 0; kk < KC; ++kk) {
            const int k = k0 + kk;
            const float* Z = sdz[kk];
            const float* X = sx[kk];
            const int c = (ty + 1) * HX + tx + 1;
            const float dzc = Z[c];
            // dx[p] = sum_t w[t] dz[p - t]; the forward's tap t = (a, e) reads x[p + (a-1, e-1)]
            float g = 0.f;
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int e = 0; e < 3; ++e) g += wt[a * 3 + e] * Z[c - (a - 1) * HX - (e - 1)];
            if (k == ks) g += S;
            if (lower_act >= 0) g = act_bwd(g, X[c], lower_act);
            if (!valid || k >= K) g = 0.f;
            so += g;
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int e = 0; e < 3; ++e) dw[a * 3 + e] += dzc * X[c + (a - 1) * HX + (e - 1)];
            db += dzc;
            o8[kk] = g;
        }
        if (valid) {
            if (rows) {
                *reinterpret_cast<uint4*>((uint16_t*)out + bpix * (size_t)ldk + k0) =
                    make_uint4(pack2_dt(o8[0], o8[1], out_dtype), pack2_dt(o8[2], o8[3], out_dtype),
                               pack2_dt(o8[4], o8[5], out_dtype), pack2_dt(o8[6], o8[7], out_dtype));
            } else {
#pragma unroll
                for (int kk = 0; kk < KC; ++kk)
                    if (k0 + kk < K) ((float*)out)[((size_t)b * K + k0 + kk) * HW + pix] = o8[kk];
            }
        }
    }
    if (valid) {
        if (rows)
            for (int k0 = K8; k0 < ldk; k0 += 8) *reinterpret_cast<uint4*>((uint16_t*)out + bpix * (size_t)ldk + k0) = make_uint4(0, 0, 0, 0);
        if (ksum_out) ksum_out[bpix] = so;
    }
    // the workgroup's weight-gradient partials: wave sums, then the 4 waves in order
    const int lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int q = 0; q < 9; ++q) {
        const float v = wave_sum_h(dw[q]);
        if (lane == 0) red[wv][q] = v;
    }
    {
        const float v = wave_sum_h(db);
        if (lane == 0) red[wv][9] = v;
    }
    __syncthreads();
    if (tid < 10) partial[(size_t)blockIdx.x * 10 + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// dW[0..8], db (+)= the sum of nrows partial rows of 10, in a fixed order (one workgroup)
__global__ __launch_bounds__(256) void head_dw_reduce_kernel(const float* __restrict__ partial, int nrows, float* __restrict__ dW,
                                                             float* __restrict__ db, int accumulate) {
    __shared__ float red[256][10];
    const int tid = threadIdx.x;
    float s[10];
#pragma unroll
    for (int q = 0; q < 10; ++q) s[q] = 0.f;
    for (int r = tid; r < nrows; r += 256)
#pragma unroll
        for (int q = 0; q < 10; ++q) s[q] += partial[(size_t)r * 10 + q];
#pragma unroll
    for (int q = 0; q < 10; ++q) red[tid][q] = s[q];
    for (int h = 128; h >= 1; h >>= 1) {
        __syncthreads();
        if (tid < h)
#pragma unroll
            for (int q = 0; q < 10; ++q) red[tid][q] += red[tid + h][q];
    }
    __syncthreads();
    if (tid < 9) dW[tid] = (accumulate ? dW[tid] : 0.f) + red[0][tid];
    if (tid == 9) db[0] = (accumulate ? db[0] : 0.f) + red[0][9];
}

inline int grid_for(size_t total, int block = 256) {      // cap + grid-stride, as elementwise.hip
    size_t g = (total + block - 1) / block;
    if (g > 256 * 16) g = 256 * 16;
    if (g < 1) g = 1;
    return (int)g;
}

}  // namespace

#define CHECK_LAUNCH() LSEG_HIP_TRY(hipGetLastError())

int launch_head_block_train(const float* in, float* out, int* kstar, const float* w9, const float* bias, int B, int K, int H, int W,
                            int bottleneck, int act, int apply_act, hipStream_t st) {
    hipLaunchKernelGGL(head_block_train_fwd_kernel, dim3(grid_for((size_t)B * H * W)), dim3(256), 0, st, in, out, kstar, w9, bias, B, K, H, W,
                       bottleneck, act, apply_act);
    CHECK_LAUNCH();
    return 0;
}

int launch_head_bwd_prep(const float* dy, const float* y, const float* x, float* dz, float* ksum, int* kstar, int B, int K, int HW, int act,
                         int apply_act, hipStream_t st) {
    hipLaunchKernelGGL(head_bwd_prep_kernel, dim3(grid_for((size_t)B * HW)), dim3(256), 0, st, dy, y, x, dz, ksum, kstar, B, K, HW, act, apply_act);
    CHECK_LAUNCH();
    return 0;
}

size_t head_block_bwd_partials(int B, int H, int W) {
    return (size_t)B * ((H + TY - 1) / TY) * ((W + TX - 1) / TX);
}

int launch_head_block_backward(const float* dz, const float* ksum, const int* kstar, const float* x, const float* w9, void* out, int out_dtype,
                               int ldk, int lower_act, float* ksum_out, float* partial, int B, int K, int H, int W, int bottleneck, hipStream_t st) {
    if (out_dtype != DT_F32 && (ldk < K || (ldk & 7))) return set_error(LSEG_ERR_INVALID, "head block backward: ldk=%d must be a multiple of 8 and >= K=%d", ldk, K);
    if (bottleneck && (!kstar || !ksum)) return set_error(LSEG_ERR_INVALID, "head block backward: the bottleneck needs k* and the label sums");
    const size_t nblk = head_block_bwd_partials(B, H, W);
    hipLaunchKernelGGL(head_block_bwd_kernel, dim3((unsigned)nblk), dim3(256), 0, st, dz, ksum, kstar, x, w9, out, out_dtype, ldk, lower_act,
                       ksum_out, partial, B, K, H, W, bottleneck);
    CHECK_LAUNCH();
    return 0;
}

int launch_head_dw_reduce(const float* partial, int nrows, float* dW, float* db, int accumulate, hipStream_t st) {
    hipLaunchKernelGGL(head_dw_reduce_kernel, dim3(1), dim3(256), 0, st, partial, nrows, dW, db, accumulate);
    CHECK_LAUNCH();
    return 0;
}

}  // namespace lseg
