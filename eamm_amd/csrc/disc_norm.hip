// What follows the convolution in a discriminator block (reference modules/discriminator.py:25-33), fused, on NHWC fp32 maps:
// InstanceNorm2d(affine, eps, biased variance, no running statistics) -> LeakyReLU(0.2) -> optional AvgPool2d(2) with floor sizes
// (an odd last row or column feeds no window), and its backward.  `norm` = 0 is block 0's mode without the normalisation.
//
//   forward   disc_stats_partial_kernel  per image and pixel range: sum and sum of squares per channel, accumulated in double;
//             disc_stats_final_kernel    the ranges added in index order -> stats [B][C][2] DOUBLES = (mean, 1 / sqrt(var + eps));
//             disc_apply_kernel          reads x once, writes only what the block returns (the pooled map with `pool`).
//   backward  recomputes z = xhat * gamma + beta from the saved x and stats; dz = slope(z) * (grad_out / 4 into its window | grad_out),
//             zero for a dropped odd row or column; the two sums per (b, c) a1 = sum dz, a2 = sum dz * xhat by the same two stages;
//             dgamma = sum_b a2, dbeta = sum_b a1 in image order;  dx = rstd * gamma * (dz - a1 / n - xhat * a2 / n).
// A thread owns four channels (one 16-byte access per pixel), the 256 / (C / 4) row lanes of a block stride the pixels.  No float
// atomics, every sum in a fixed order: the same bits on every run.  The kernels hold their sums in registers (no scratch).
// The statistics stay in double and xhat is formed in double: with few values per channel the backward's dz - a1 / n - xhat * a2 / n
// cancels to eps / (var + eps) of its terms (two values: xhat = +-1 up to 1e-5), which fp32 statistics would round away.
#include "conv_common.h"

#include <algorithm>

namespace eamm {

namespace {

constexpr int DN_PARTS = 64;        // pixel ranges per image, at most
constexpr float DN_SLOPE = 0.2f;    // F.leaky_relu(out, 0.2)

struct DiscNormArgs {
    const float* x;       // [B,H,W,C] the convolution's output
    const double* stats;  // [B,C,2] (mean, rstd)
    const float* gamma;   // [C]
    const float* beta;    // [C]
    const float* dout;    // backward: [B,Ho,Wo,C]
    int H, W, C, norm, pool;
    int parts, per;       // pixel ranges per image and their length
};

// the statistics and affine parameters of four channels of one image
struct DnParams {
    double mean[4], rstd[4];
    f32x4 ga, be;
};

__device__ __forceinline__ void dn_load_params(const DiscNormArgs& p, int b, int c4, DnParams& q) {
    if (!p.norm) return;
    const double* st = p.stats + ((size_t)b * p.C + c4 * 4) * 2;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        q.mean[k] = st[2 * k];
        q.rstd[k] = st[2 * k + 1];
    }
    q.ga = reinterpret_cast<const f32x4*>(p.gamma)[c4];
    q.be = reinterpret_cast<const f32x4*>(p.beta)[c4];
}

// xhat (double) and z (norm: xhat * gamma + beta; else x itself) of four channels of one pixel
__device__ __forceinline__ void dn_z(const DiscNormArgs& p, const f32x4& xv, const DnParams& q, double (&xhat)[4], f32x4& z) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (p.norm) {
            xhat[k] = ((double)xv[k] - q.mean[k]) * q.rstd[k];
            z[k] = (float)xhat[k] * q.ga[k] + q.be[k];
        } else {
            xhat[k] = (double)xv[k];
            z[k] = xv[k];
        }
    }
}

__device__ __forceinline__ f32x4 dn_leaky(const f32x4& z) {
    f32x4 r;
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = z[k] > 0.f ? z[k] : DN_SLOPE * z[k];
    return r;
}

// the two-stage block reduction's first stage: row lanes r > 0 hand their eight doubles to lane r = 0 of their channel group, which
// adds them in row order and writes part[((b * parts + part) * C + c) * 2 + {0, 1}]
__device__ __forceinline__ void dn_block_sums(double (&s)[8], int c4n, int rows, int c4, int r, double* red, double* dst) {
    if (r > 0 && r < rows)
#pragma unroll
        for (int k = 0; k < 8; ++k) red[(size_t)threadIdx.x * 8 + k] = s[k];
    __syncthreads();
    if (r == 0) {
        for (int q = 1; q < rows; ++q)
#pragma unroll
            for (int k = 0; k < 8; ++k) s[k] += red[(size_t)(q * c4n + c4) * 8 + k];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            dst[(c4 * 4 + k) * 2 + 0] = s[k];
            dst[(c4 * 4 + k) * 2 + 1] = s[4 + k];
        }
    }
}

}  // namespace

// grid (parts, B): sum x and sum x^2 over the pixel range, per channel
__global__ __launch_bounds__(256) void disc_stats_partial_kernel(const DiscNormArgs p, double* __restrict__ part) {
    __shared__ double red[256 * 8];
    const int c4n = p.C >> 2, rows = 256 / c4n, c4 = threadIdx.x % c4n, r = threadIdx.x / c4n;
    const int HW = p.H * p.W, b = blockIdx.y;
    const int p0 = blockIdx.x * p.per, p1 = min(HW, p0 + p.per);
    double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (r < rows) {
        const f32x4* xp = reinterpret_cast<const f32x4*>(p.x) + (size_t)b * HW * c4n + c4;
        for (int pp = p0 + r; pp < p1; pp += rows) {
            const f32x4 v = xp[(size_t)pp * c4n];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                s[k] += (double)v[k];
                s[4 + k] += (double)v[k] * (double)v[k];
            }
        }
    }
    dn_block_sums(s, c4n, rows, c4, r, red, part + ((size_t)b * p.parts + blockIdx.x) * p.C * 2);
}

// one thread per (b, c): the ranges in index order -> (mean, rstd)
__global__ __launch_bounds__(256) void disc_stats_final_kernel(const double* __restrict__ part, int B, int C, int parts, int HW, float eps,
                                                               double* __restrict__ stats) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * C) return;
    const int b = i / C, c = i % C;
    double s = 0.0, ss = 0.0;
    for (int k = 0; k < parts; ++k) {
        s += part[(((size_t)b * parts + k) * C + c) * 2 + 0];
        ss += part[(((size_t)b * parts + k) * C + c) * 2 + 1];
    }
    const double mean = s / HW, var = fmax(ss / HW - mean * mean, 0.0);
    stats[(size_t)i * 2 + 0] = mean;
    stats[(size_t)i * 2 + 1] = 1.0 / sqrt(var + (double)eps);
}

// one thread per (output pixel, four channels)
__global__ __launch_bounds__(256) void disc_apply_kernel(const DiscNormArgs p, int B, float* __restrict__ out) {
    const int c4n = p.C >> 2;
    const int Ho = p.pool ? p.H / 2 : p.H, Wo = p.pool ? p.W / 2 : p.W;
    const long long total = (long long)B * Ho * Wo * c4n;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c4 = (int)(i % c4n);
    long long t = i / c4n;
    const int ox = (int)(t % Wo);
    t /= Wo;
    const int oy = (int)(t % Ho), b = (int)(t / Ho);
    DnParams q;
    dn_load_params(p, b, c4, q);
    const f32x4* xp = reinterpret_cast<const f32x4*>(p.x) + (size_t)b * p.H * p.W * c4n + c4;
    double xhat[4];
    f32x4 z, y;
    if (p.pool) {
        y = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            dn_z(p, xp[((size_t)(2 * oy + (e >> 1)) * p.W + 2 * ox + (e & 1)) * c4n], q, xhat, z);
            y += dn_leaky(z);
        }
        y *= 0.25f;
    } else {
        dn_z(p, xp[((size_t)oy * p.W + ox) * c4n], q, xhat, z);
        y = dn_leaky(z);
    }
    reinterpret_cast<f32x4*>(out)[i] = y;
}

namespace {

// dz of four channels at input pixel (y, x) of image b, from the pooled or the full-size grad_out
__device__ __forceinline__ f32x4 dn_dz(const DiscNormArgs& p, int b, int y, int x, int c4, int c4n, const f32x4& z) {
    f32x4 g = {0.f, 0.f, 0.f, 0.f};
    if (p.pool) {
        const int Ho = p.H / 2, Wo = p.W / 2;
        if (y < 2 * Ho && x < 2 * Wo) g = reinterpret_cast<const f32x4*>(p.dout)[(((size_t)b * Ho + (y >> 1)) * Wo + (x >> 1)) * c4n + c4] * 0.25f;
    } else {
        g = reinterpret_cast<const f32x4*>(p.dout)[(((size_t)b * p.H + y) * p.W + x) * c4n + c4];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) g[k] = z[k] > 0.f ? g[k] : DN_SLOPE * g[k];
    return g;
}

}  // namespace

// grid (parts, B), norm only: a1 = sum dz, a2 = sum dz * xhat over the pixel range, per channel
__global__ __launch_bounds__(256) void disc_bwd_partial_kernel(const DiscNormArgs p, double* __restrict__ part) {
    __shared__ double red[256 * 8];
    const int c4n = p.C >> 2, rows = 256 / c4n, c4 = threadIdx.x % c4n, r = threadIdx.x / c4n;
    const int HW = p.H * p.W, b = blockIdx.y;
    const int p0 = blockIdx.x * p.per, p1 = min(HW, p0 + p.per);
    double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (r < rows) {
        DnParams q;
        dn_load_params(p, b, c4, q);
        const f32x4* xp = reinterpret_cast<const f32x4*>(p.x) + (size_t)b * HW * c4n + c4;
        for (int pp = p0 + r; pp < p1; pp += rows) {
            double xhat[4];
            f32x4 z;
            dn_z(p, xp[(size_t)pp * c4n], q, xhat, z);
            const f32x4 dz = dn_dz(p, b, pp / p.W, pp % p.W, c4, c4n, z);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                s[k] += (double)dz[k];
                s[4 + k] += (double)dz[k] * xhat[k];
            }
        }
    }
    dn_block_sums(s, c4n, rows, c4, r, red, part + ((size_t)b * p.parts + blockIdx.x) * p.C * 2);
}

// one thread per (b, c): the ranges in index order -> sums [B][C][2] = (a1, a2) in double
__global__ __launch_bounds__(256) void disc_bwd_final_kernel(const double* __restrict__ part, int B, int C, int parts, double* __restrict__ sums) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * C) return;
    const int b = i / C, c = i % C;
    double a1 = 0.0, a2 = 0.0;
    for (int k = 0; k < parts; ++k) {
        a1 += part[(((size_t)b * parts + k) * C + c) * 2 + 0];
        a2 += part[(((size_t)b * parts + k) * C + c) * 2 + 1];
    }
    sums[(size_t)i * 2 + 0] = a1;
    sums[(size_t)i * 2 + 1] = a2;
}

// one thread per channel: the images in index order
__global__ __launch_bounds__(256) void disc_bwd_param_kernel(const double* __restrict__ sums, int B, int C, float* __restrict__ dgamma,
                                                             float* __restrict__ dbeta) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double a1 = 0.0, a2 = 0.0;
    for (int b = 0; b < B; ++b) {
        a1 += sums[((size_t)b * C + c) * 2 + 0];
        a2 += sums[((size_t)b * C + c) * 2 + 1];
    }
    if (dbeta != nullptr) dbeta[c] = (float)a1;
    if (dgamma != nullptr) dgamma[c] = (float)a2;
}

// one thread per (input pixel, four channels)
__global__ __launch_bounds__(256) void disc_bwd_dx_kernel(const DiscNormArgs p, int B, const double* __restrict__ sums, float* __restrict__ dx) {
    const int c4n = p.C >> 2, HW = p.H * p.W;
    const long long total = (long long)B * HW * c4n;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c4 = (int)(i % c4n);
    const long long t = i / c4n;
    const int pp = (int)(t % HW), b = (int)(t / HW);
    DnParams q;
    dn_load_params(p, b, c4, q);
    double xhat[4];
    f32x4 z;
    dn_z(p, reinterpret_cast<const f32x4*>(p.x)[i], q, xhat, z);
    f32x4 g = dn_dz(p, b, pp / p.W, pp % p.W, c4, c4n, z);
    if (p.norm) {
        const double* sm = sums + ((size_t)b * p.C + c4 * 4) * 2;
        const double inv = 1.0 / HW;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            g[k] = (float)(q.rstd[k] * (double)q.ga[k] * ((double)g[k] - sm[2 * k] * inv - xhat[k] * (sm[2 * k + 1] * inv)));
    }
    reinterpret_cast<f32x4*>(dx)[i] = g;
}

namespace {

int dn_parts(int HW) { return std::max(1, std::min(DN_PARTS, (HW + 63) / 64)); }

DiscNormArgs dn_args(const float* x, const double* stats, const float* gamma, const float* beta, const float* dout, int H, int W, int C,
                     int norm, int pool) {
    DiscNormArgs a{};
    a.x = x;
    a.stats = stats;
    a.gamma = gamma;
    a.beta = beta;
    a.dout = dout;
    a.H = H;
    a.W = W;
    a.C = C;
    a.norm = norm;
    a.pool = pool;
    a.parts = dn_parts(H * W);
    a.per = (H * W + a.parts - 1) / a.parts;
    return a;
}

}  // namespace

const char* disc_norm_refusal(int B, int H, int W, int C, int norm, int pool) {
    if (B < 1 || H < 1 || W < 1 || B > 65535) return "B, H, W must be positive (B at most 65535)";
    if (C < 4 || (C & 3) || C > 1024) return "C must be a multiple of 4, at most 1024";
    if ((unsigned long long)B * H * W * C >= (1ull << 31)) return "tensor too large (2^31 elements)";
    if (norm && (long long)H * W < 2) return "InstanceNorm needs more than one value per channel (H * W >= 2)";
    if (pool && (H < 2 || W < 2)) return "a map below 2 x 2 has no pooling window";
    return nullptr;
}

// forward: the ranges' sums (doubles); backward: those and the per-(b, c) sums (doubles).  Floats, 0 without the normalisation.
size_t disc_norm_workspace_floats(int B, int H, int W, int C, int norm, int backward) {
    if (disc_norm_refusal(B, H, W, C, norm, 0) || !norm) return 0;
    const size_t part = (size_t)B * dn_parts(H * W) * C * 2, sums = backward ? (size_t)B * C * 2 : 0;
    return round64(2 * (part + sums));
}

hipError_t disc_norm_act_pool_launch(const float* x, const float* gamma, const float* beta, int B, int H, int W, int C, int norm, int pool,
                                     float eps, double* stats, float* out, float* workspace, hipStream_t s) {
    if (disc_norm_refusal(B, H, W, C, norm, pool)) return hipErrorInvalidValue;
    const DiscNormArgs a = dn_args(x, stats, gamma, beta, nullptr, H, W, C, norm, pool);
    if (norm) {
        double* part = reinterpret_cast<double*>(workspace);
        hipLaunchKernelGGL(disc_stats_partial_kernel, dim3(a.parts, B), dim3(256), 0, s, a, part);
        hipLaunchKernelGGL(disc_stats_final_kernel, dim3((B * C + 255) / 256), dim3(256), 0, s, part, B, C, a.parts, H * W, eps, stats);
    }
    const long long total = (long long)B * (pool ? H / 2 : H) * (pool ? W / 2 : W) * (C / 4);
    hipLaunchKernelGGL(disc_apply_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a, B, out);
    return hipGetLastError();
}

hipError_t disc_norm_act_pool_backward_launch(const float* x, const double* stats, const float* gamma, const float* beta, const float* dout,
                                              int B, int H, int W, int C, int norm, int pool, float* dx, float* dgamma, float* dbeta,
                                              float* workspace, hipStream_t s) {
    if (disc_norm_refusal(B, H, W, C, norm, pool)) return hipErrorInvalidValue;
    const DiscNormArgs a = dn_args(x, stats, gamma, beta, dout, H, W, C, norm, pool);
    double* part = reinterpret_cast<double*>(workspace);
    double* sums = norm ? part + (size_t)B * a.parts * C * 2 : nullptr;
    if (norm) {
        hipLaunchKernelGGL(disc_bwd_partial_kernel, dim3(a.parts, B), dim3(256), 0, s, a, part);
        hipLaunchKernelGGL(disc_bwd_final_kernel, dim3((B * C + 255) / 256), dim3(256), 0, s, part, B, C, a.parts, sums);
        if (dgamma != nullptr || dbeta != nullptr)
            hipLaunchKernelGGL(disc_bwd_param_kernel, dim3((C + 255) / 256), dim3(256), 0, s, sums, B, C, dgamma, dbeta);
    }
    if (dx != nullptr) {
        const long long total = (long long)B * H * W * (C / 4);
        hipLaunchKernelGGL(disc_bwd_dx_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a, B, sums, dx);
    }
    return hipGetLastError();
}

}  // namespace eamm
