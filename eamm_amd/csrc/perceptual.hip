// The pyramid perceptual loss around its convolutions (reference modules/model.py:10-68 and :236-248, modules/util.py:1005-1052): VGG19's
// thirteen 3x3 convolutions run on the convolution kernels this library already has; the kernels here are everything else, each with
// its backward:
//   * vgg_input_kernel / vgg_input_backward_kernel -- one pyramid level (zero-pad 6, depth-wise 13x13 Gaussian, every inv-th row and
//     column kept), normalised with VGG's mean / std, written as the 32-channel NHWC tensor conv1_1 reads (channels 3..31 zero) and,
//     where asked, un-normalised as NCHW (ImagePyramide's output).  The backward is the transposed Gaussian as a GATHER per source
//     pixel, as antialias_down_backward_kernel (motion_backward.hip).
//   * relu_pool_kernel / relu_pool_backward_kernel -- ReLU in place and MaxPool2d(2, 2) in one pass over 2x2 cells; the backward of
//     both in one pass: windows do not overlap, so a pixel reads at most one pooled gradient (no scatter).
//   * l1_pair_* -- w * mean|a - b| as a fixed-order two-stage sum, and in the same pass g = (w / N) sign(a - b).
// All HBM-bound: float4 along the channel axis, grid-stride loops over a grid sized to the chip, no float atomics -- every result is
// the same bits from run to run.
#include "pointwise.h"

#include <algorithm>

namespace eamm {

namespace {

constexpr int PERC_THREADS = 64 * BLOCK_WAVES;   // the workgroup sums below are block_reduce's
constexpr int PERC_MAX_GRID = 256 * 8;           // 256 CUs x 8 workgroups of 256 threads; the loops stride over the rest
constexpr int L1_MAX_GRID = 1024;                // a constant (not the device's CU count): the sum's order depends on N alone

unsigned perc_grid(size_t items, int cap = PERC_MAX_GRID) {
    return (unsigned)std::max<size_t>(1, std::min<size_t>((items + PERC_THREADS - 1) / PERC_THREADS, (size_t)cap));
}

__device__ __forceinline__ float relu1(float v) { return v < 0.f ? 0.f : v; }
__device__ __forceinline__ float4 relu4(float4 v) { return make_float4(relu1(v.x), relu1(v.y), relu1(v.z), relu1(v.w)); }
__device__ __forceinline__ float sign_scaled(float d, float gs) { return d > 0.f ? gs : (d < 0.f ? -gs : 0.f); }

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// one pyramid level: src [B,3,H,W] -> out [B,h,w,32] ((level - mean) / std in channels 0..2, zeros above) and / or level [B,3,h,w]
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vgg_input_kernel(const float* __restrict__ src, const float* __restrict__ aa_w,
                                                        const float* __restrict__ mean, const float* __restrict__ stdv, int B, int H, int W,
                                                        int inv, float4* __restrict__ out, float* __restrict__ level) {
    const int h = H / inv, w = W / inv;
    const size_t plane = (size_t)H * W, small = (size_t)h * w, total = (size_t)B * small;
    float m[3] = {0.f, 0.f, 0.f}, sd[3] = {1.f, 1.f, 1.f};
    if (out)
        for (int c = 0; c < 3; ++c) {
            m[c] = mean[c];
            sd[c] = stdv[c];
        }
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(idx % w), y = (int)((idx / w) % h);
        const size_t b = idx / small;
        float v[3];
        if (inv == 1) {
            for (int c = 0; c < 3; ++c) v[c] = src[(b * 3 + c) * plane + (size_t)y * W + x];
        } else {
            const int cy = y * inv - 6, cx = x * inv - 6;
            for (int c = 0; c < 3; ++c) {
                const float* p = src + (b * 3 + c) * plane;
                const float* k = aa_w + c * 169;
                float s = 0.f;
                for (int ky = 0; ky < 13; ++ky) {
                    const int yy = cy + ky;
                    if ((unsigned)yy >= (unsigned)H) continue;
                    for (int kx = 0; kx < 13; ++kx) {
                        const int xx = cx + kx;
                        if ((unsigned)xx >= (unsigned)W) continue;
                        s = fmaf(p[(size_t)yy * W + xx], k[ky * 13 + kx], s);
                    }
                }
                v[c] = s;
            }
        }
        if (level)
            for (int c = 0; c < 3; ++c) level[(b * 3 + c) * small + (size_t)y * w + x] = v[c];
        if (out) {
            float4* o = out + idx * 8;
            o[0] = make_float4((v[0] - m[0]) / sd[0], (v[1] - m[1]) / sd[1], (v[2] - m[2]) / sd[2], 0.f);
#pragma unroll
            for (int k = 1; k < 8; ++k) o[k] = zero;
        }
    }
}

// g [B,h,w,Cg] (channels 0..2 read; or null) and / or glevel [B,3,h,w] (or null) -> dsrc [B,3,H,W].  A normalised gradient is divided
// by std BEFORE it is weighted, so that this kernel on g equals itself on glevel = (the inv 1 kernel on g) bit for bit.
__global__ __launch_bounds__(256) void vgg_input_backward_kernel(const float* __restrict__ g, int Cg, const float* __restrict__ glevel,
                                                                 const float* __restrict__ aa_w, const float* __restrict__ stdv, int B, int H,
                                                                 int W, int inv, float* __restrict__ dsrc) {
    const int h = H / inv, w = W / inv;
    const size_t plane = (size_t)H * W, small = (size_t)h * w, total = (size_t)B * plane;
    float sd[3] = {1.f, 1.f, 1.f};
    if (g)
        for (int c = 0; c < 3; ++c) sd[c] = stdv[c];
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int X = (int)(idx % W), Y = (int)((idx / W) % H);
        const size_t b = idx / plane;
        // forward: level[y][x] = sum_{ky,kx} k[ky][kx] src[s y - 6 + ky][s x - 6 + kx]  =>  ky = Y - s y + 6 in [0, 13)
        int y_lo = Y, y_hi = Y, x_lo = X, x_hi = X;
        if (inv != 1) {
            y_lo = max(0, (Y - 6 + inv - 1) / inv), y_hi = min(h - 1, (Y + 6) / inv);
            x_lo = max(0, (X - 6 + inv - 1) / inv), x_hi = min(w - 1, (X + 6) / inv);
        }
        float acc[3] = {0.f, 0.f, 0.f};
        for (int y = y_lo; y <= y_hi; ++y) {
            const int ky = Y - inv * y + 6;
            for (int x = x_lo; x <= x_hi; ++x) {
                const int kx = X - inv * x + 6;
                const size_t pix = (size_t)y * w + x;
                float gv[3];
                if (g) {
                    const float4 q = *reinterpret_cast<const float4*>(g + (b * small + pix) * Cg);
                    gv[0] = q.x / sd[0];
                    gv[1] = q.y / sd[1];
                    gv[2] = q.z / sd[2];
                    if (glevel)
                        for (int c = 0; c < 3; ++c) gv[c] += glevel[(b * 3 + c) * small + pix];
                } else {
                    for (int c = 0; c < 3; ++c) gv[c] = glevel[(b * 3 + c) * small + pix];
                }
                if (inv == 1) {
                    for (int c = 0; c < 3; ++c) acc[c] = gv[c];
                } else {
                    for (int c = 0; c < 3; ++c) acc[c] = fmaf(gv[c], aa_w[c * 169 + ky * 13 + kx], acc[c]);
                }
            }
        }
        const size_t r = (size_t)Y * W + X;
        for (int c = 0; c < 3; ++c) dsrc[(b * 3 + c) * plane + r] = acc[c];
    }
}

hipError_t vgg_input_launch(const float* src, const float* aa_w, const float* mean, const float* stdv, int B, int H, int W, int inv,
                            float* out, float* level, hipStream_t s) {
    const size_t total = (size_t)B * (H / inv) * (W / inv);
    hipLaunchKernelGGL(vgg_input_kernel, dim3(perc_grid(total)), dim3(PERC_THREADS), 0, s, src, aa_w, mean, stdv, B, H, W, inv,
                       reinterpret_cast<float4*>(out), level);
    return hipGetLastError();
}

hipError_t vgg_input_backward_launch(const float* g, int Cg, const float* glevel, const float* aa_w, const float* stdv, int B, int H, int W,
                                     int inv, float* dsrc, hipStream_t s) {
    hipLaunchKernelGGL(vgg_input_backward_kernel, dim3(perc_grid((size_t)B * H * W)), dim3(PERC_THREADS), 0, s, g, Cg, glevel, aa_w, stdv, B,
                       H, W, inv, dsrc);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// ReLU in place + MaxPool2d(2, 2): one thread per 2x2 cell and four channels.  Cells cover ceil(H/2) x ceil(W/2), so an odd last
// row or column is rectified too; only a complete cell is a pooling window (sizes floor).
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void relu_pool_kernel(float4* __restrict__ x, int B, int H, int W, int C4, float4* __restrict__ pooled) {
    const int Hc = (H + 1) / 2, Wc = (W + 1) / 2, hp = H / 2, wp = W / 2;
    const size_t total = (size_t)B * Hc * Wc * C4;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(idx % C4);
        size_t t = idx / C4;
        const int cx = (int)(t % Wc);
        t /= Wc;
        const int cy = (int)(t % Hc);
        const size_t b = t / Hc;
        const bool hasx = 2 * cx + 1 < W, hasy = 2 * cy + 1 < H;
        float4* p = x + ((b * H + 2 * cy) * W + 2 * cx) * C4 + c4;
        const size_t row = (size_t)W * C4;
        const float4 v00 = relu4(p[0]);
        p[0] = v00;
        float4 v01 = v00, v10 = v00, v11 = v00;
        if (hasx) p[C4] = v01 = relu4(p[C4]);
        if (hasy) p[row] = v10 = relu4(p[row]);
        if (hasx && hasy) {
            p[row + C4] = v11 = relu4(p[row + C4]);
            if (pooled)
                pooled[((b * hp + cy) * wp + cx) * C4 + c4] =
                    make_float4(fmaxf(fmaxf(v00.x, v01.x), fmaxf(v10.x, v11.x)), fmaxf(fmaxf(v00.y, v01.y), fmaxf(v10.y, v11.y)),
                                fmaxf(fmaxf(v00.z, v01.z), fmaxf(v10.z, v11.z)), fmaxf(fmaxf(v00.w, v01.w), fmaxf(v10.w, v11.w)));
        }
    }
}

// dx = (y > 0) * (dy + dp routed to the window's FIRST maximum in row-major order); dy and dp may each be null
__global__ __launch_bounds__(256) void relu_pool_backward_kernel(const float4* __restrict__ y, const float4* __restrict__ dy,
                                                                 const float4* __restrict__ dp, int B, int H, int W, int C4,
                                                                 float4* __restrict__ dx) {
    const int Hc = (H + 1) / 2, Wc = (W + 1) / 2, hp = H / 2, wp = W / 2;
    const size_t total = (size_t)B * Hc * Wc * C4;
    const size_t row = (size_t)W * C4;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(idx % C4);
        size_t t = idx / C4;
        const int cx = (int)(t % Wc);
        t /= Wc;
        const int cy = (int)(t % Hc);
        const size_t b = t / Hc;
        const bool hasx = 2 * cx + 1 < W, hasy = 2 * cy + 1 < H;
        const size_t base = ((b * H + 2 * cy) * W + 2 * cx) * C4 + c4;
        const size_t off[4] = {0, (size_t)C4, row, row + C4};
        const bool has[4] = {true, hasx, hasy, hasx && hasy};
        float yv[4][4], gv[4][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f), d = a;
            if (has[k]) {
                a = y[base + off[k]];
                if (dy) d = dy[base + off[k]];
            }
            yv[k][0] = a.x; yv[k][1] = a.y; yv[k][2] = a.z; yv[k][3] = a.w;
            gv[k][0] = d.x; gv[k][1] = d.y; gv[k][2] = d.z; gv[k][3] = d.w;
        }
        if (dp && has[3]) {
            const float4 q = dp[((b * hp + cy) * wp + cx) * C4 + c4];
            const float qv[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                int win = 0;
                float best = yv[0][c];
#pragma unroll
                for (int k = 1; k < 4; ++k)
                    if (yv[k][c] > best) {
                        best = yv[k][c];
                        win = k;
                    }
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k == win) gv[k][c] += qv[c];
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (has[k])
                dx[base + off[k]] = make_float4(yv[k][0] > 0.f ? gv[k][0] : 0.f, yv[k][1] > 0.f ? gv[k][1] : 0.f,
                                                yv[k][2] > 0.f ? gv[k][2] : 0.f, yv[k][3] > 0.f ? gv[k][3] : 0.f);
    }
}

hipError_t relu_pool_launch(float* x, int B, int H, int W, int C, float* pooled, hipStream_t s) {
    const size_t total = (size_t)B * ((H + 1) / 2) * ((W + 1) / 2) * (C / 4);
    hipLaunchKernelGGL(relu_pool_kernel, dim3(perc_grid(total)), dim3(PERC_THREADS), 0, s, reinterpret_cast<float4*>(x), B, H, W, C / 4,
                       reinterpret_cast<float4*>(pooled));
    return hipGetLastError();
}

hipError_t relu_pool_backward_launch(const float* y, const float* dy, const float* dp, int B, int H, int W, int C, float* dx, hipStream_t s) {
    const size_t total = (size_t)B * ((H + 1) / 2) * ((W + 1) / 2) * (C / 4);
    hipLaunchKernelGGL(relu_pool_backward_kernel, dim3(perc_grid(total)), dim3(PERC_THREADS), 0, s, reinterpret_cast<const float4*>(y),
                       reinterpret_cast<const float4*>(dy), reinterpret_cast<const float4*>(dp), B, H, W, C / 4,
                       reinterpret_cast<float4*>(dx));
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// w * mean|a - b| and g = (w / N) sign(a - b): workgroup j's partial is the sum of its threads' grid-stride sums through the fixed
// tree of block_reduce; one workgroup then adds the partials, thread t taking t, t + 256, ... in that order.  The grid depends on N
// alone, so the value is the same bits on every run and every device.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void l1_pair_partial_kernel(const float* __restrict__ a, const float* __restrict__ b, long long n, float gs,
                                                              float* __restrict__ g, double* __restrict__ partial) {
    __shared__ double red[BLOCK_WAVES];
    const long long n4 = n >> 2;
    const float4* a4 = reinterpret_cast<const float4*>(a);
    const float4* b4 = reinterpret_cast<const float4*>(b);
    float4* g4 = reinterpret_cast<float4*>(g);
    float sum = 0.f;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const float4 p = a4[i], q = b4[i];
        const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z, dw = p.w - q.w;
        sum += (fabsf(dx) + fabsf(dy)) + (fabsf(dz) + fabsf(dw));
        g4[i] = make_float4(sign_scaled(dx, gs), sign_scaled(dy, gs), sign_scaled(dz, gs), sign_scaled(dw, gs));
    }
    const long long tail = 4 * n4 + threadIdx.x;   // the up-to-three elements behind the last float4: workgroup 0's first threads
    if (blockIdx.x == 0 && tail < n) {
        const float d = a[tail] - b[tail];
        sum += fabsf(d);
        g[tail] = sign_scaled(d, gs);
    }
    const double total = block_reduce<SumOp, Lanes::First>((double)sum, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void l1_pair_final_kernel(const double* __restrict__ partial, int count, double scale, float* __restrict__ value) {
    __shared__ double red[BLOCK_WAVES];
    double sum = 0.0;
    for (int i = threadIdx.x; i < count; i += blockDim.x) sum += partial[i];
    const double total = block_reduce<SumOp, Lanes::First>(sum, red);
    if (threadIdx.x == 0) value[0] = (float)(total * scale);
}

// out = g * grad_value[0]: the whole backward of l1_pair
__global__ __launch_bounds__(256) void l1_pair_backward_kernel(const float* __restrict__ g, long long n, const float* __restrict__ grad_value,
                                                               float* __restrict__ out) {
    const float s = grad_value[0];
    const long long n4 = n >> 2;
    const float4* g4 = reinterpret_cast<const float4*>(g);
    float4* o4 = reinterpret_cast<float4*>(out);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const float4 v = g4[i];
        o4[i] = make_float4(v.x * s, v.y * s, v.z * s, v.w * s);
    }
    const long long tail = 4 * n4 + threadIdx.x;
    if (blockIdx.x == 0 && tail < n) out[tail] = g[tail] * s;
}

int l1_pair_partials(long long n) { return (int)perc_grid((size_t)std::max<long long>(1, n >> 2), L1_MAX_GRID); }

hipError_t l1_pair_launch(const float* a, const float* b, long long n, float weight, float* value, float* g, double* partial, hipStream_t s) {
    const int grid = l1_pair_partials(n);
    hipLaunchKernelGGL(l1_pair_partial_kernel, dim3(grid), dim3(PERC_THREADS), 0, s, a, b, n, (float)((double)weight / (double)n), g, partial);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(l1_pair_final_kernel, dim3(1), dim3(PERC_THREADS), 0, s, partial, grid, (double)weight / (double)n, value);
    return hipGetLastError();
}

hipError_t l1_pair_backward_launch(const float* g, long long n, const float* grad_value, float* out, hipStream_t s) {
    hipLaunchKernelGGL(l1_pair_backward_kernel, dim3(perc_grid((size_t)std::max<long long>(1, n >> 2))), dim3(PERC_THREADS), 0, s, g, n,
                       grad_value, out);
    return hipGetLastError();
}

}  // namespace eamm
