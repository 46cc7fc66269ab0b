// Backward of the key-point heads' reduction (reference modules/keypoint_detector.py:77-105 / :180-205; forward: kp_head_launch in
// motion.hip): temperature softmax over the interior window of the 7x7 "same" convolution's NHWC output, soft-argmax, heat-map
// weighted sum of the jacobian maps.  With p = softmax(l / T) over the window and, per (image b, key point k, pixel i),
//     a_i = g_value . grid_i + sum_c g_jac[c] J_c,i + g_heatmap_i
// autograd's result is
//     dL/dl_i   = p_i (a_i - sum_j p_j a_j) / T
//     dL/dJ_c,i = g_jac[c] p_i                      (njm == 1: summed over k in key-point order)
// and sum_j p_j a_j = g_value . value + g_jac . jacobian + sum_j p_j g_heatmap_j, where value and jacobian are the forward's
// outputs: only the last term is a reduction over the map, and only a heat-map gradient needs it.  Three launches:
//   * kp_head_bwd_hmdot_kernel (only with g_heatmap)  sum_j exp(l_j / T - M) g_heatmap_j per pixel slice, one block per (image,
//     slice, group of KG key points) as kp_head_slice_kernel reads the logits;
//   * kp_head_bwd_const_kernel   the slices added in slice order + the two dot products -> c[b][k] (deterministic: no atomics);
//   * kp_head_backward_kernel    one read of the logits, one write of the gradient: a pixel's Cs contiguous floats belong to Cs / 4
//     adjacent lanes, a float4 each; the grid is sized by pixels.  Everything outside the window and every channel >= K + 4 njm
//     is written as zero, so the caller's buffer needs no initialisation.
// p is recomputed as expf(l / T - M) / S from the forward's saved (M, S) -- the heat-map pass's own expression.
#include "kernels.h"

#include <algorithm>

namespace eamm {

namespace {

__device__ __forceinline__ float kp_grid_coord(int j, int n) { return 2.f * ((float)j / (float)(n - 1)) - 1.f; }

// g_value . v + g_jac . j as ONE fmaf chain: the constant c[b][k] (v, j = the forward's value / jacobian) and the per-pixel a_i
// (v, j = the pixel's grid point / jacobian maps) go through the same operations, so that a window of a single pixel (p = 1,
// value = grid, jacobian = J) gives a logit gradient of exactly zero
__device__ __forceinline__ float kp_dot(const float* gv, float vx, float vy, const float* gj, const float* j) {
    float t = 0.f;
    if (gv) {
        t = fmaf(gv[0], vx, t);
        t = fmaf(gv[1], vy, t);
    }
    if (gj) {
        t = fmaf(gj[0], j[0], t);
        t = fmaf(gj[1], j[1], t);
        t = fmaf(gj[2], j[2], t);
        t = fmaf(gj[3], j[3], t);
    }
    return t;
}

constexpr int KP_BWD_KG = 8;   // key points per block of the heat-map dot product

__global__ __launch_bounds__(256) void kp_head_bwd_hmdot_kernel(const float* __restrict__ logits, const float* __restrict__ stats,
                                                               const float* __restrict__ g_heatmap, int K, int h, int w, int Cs, int off,
                                                               int oh, int ow, float temperature, int S, float* __restrict__ part) {
    constexpr int KG = KP_BWD_KG;
    __shared__ float red[4][KG];
    const int b = blockIdx.x, sl = blockIdx.y, k0 = blockIdx.z * KG;
    const int kn = min(KG, K - k0);
    const int n = oh * ow;
    const int i0 = (int)((long long)n * sl / S), i1 = (int)((long long)n * (sl + 1) / S);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float* base = logits + (size_t)b * h * w * Cs;
    const float* gh = g_heatmap + ((size_t)b * K + k0) * n;
    float m[KG], acc[KG];
#pragma unroll
    for (int k = 0; k < KG; ++k) {
        m[k] = k < kn ? stats[((size_t)b * K + k0 + k) * 2] : 0.f;
        acc[k] = 0.f;
    }
    for (int i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
        const float* px = base + (size_t)((i / ow + off) * w + i % ow + off) * Cs + k0;
#pragma unroll
        for (int k = 0; k < KG; ++k)
            if (k < kn) acc[k] = fmaf(expf(px[k] / temperature - m[k]), gh[(size_t)k * n + i], acc[k]);
    }
#pragma unroll
    for (int k = 0; k < KG; ++k) {
        float x = acc[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
        if (lane == 0) red[wave][k] = x;
    }
    __syncthreads();
    if ((int)threadIdx.x < kn)
        part[((size_t)b * K + k0 + threadIdx.x) * S + sl] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

__global__ __launch_bounds__(256) void kp_head_bwd_const_kernel(const float* __restrict__ stats, const float* __restrict__ value,
                                                               const float* __restrict__ jacobian, const float* __restrict__ g_value,
                                                               const float* __restrict__ g_jac, const float* __restrict__ part, int BK, int S,
                                                               float* __restrict__ cst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= BK) return;
    float c = kp_dot(g_value ? g_value + 2 * (size_t)i : nullptr, g_value ? value[2 * (size_t)i] : 0.f, g_value ? value[2 * (size_t)i + 1] : 0.f,
                     g_jac ? g_jac + 4 * (size_t)i : nullptr, g_jac ? jacobian + 4 * (size_t)i : nullptr);
    if (part) {
        float t = 0.f;
        for (int sl = 0; sl < S; ++sl) t += part[(size_t)i * S + sl];
        c += t / stats[2 * (size_t)i + 1];
    }
    cst[i] = c;
}

// the gradient of channel c of the pixel (xx, yy) of the window; px = the pixel's Cs logits
__device__ __forceinline__ float kp_head_grad_channel(const float* __restrict__ px, const float* __restrict__ stats, const float* __restrict__ cst,
                                                      const float* __restrict__ g_value, const float* __restrict__ g_jac,
                                                      const float* __restrict__ g_heatmap, int b, int c, int K, int njm, int xx, int yy, int oh,
                                                      int ow, float temperature) {
    if (c < K) {
        const size_t bk = (size_t)b * K + c;
        const float p = expf(px[c] / temperature - stats[2 * bk]) / stats[2 * bk + 1];
        float a = kp_dot(g_value ? g_value + 2 * bk : nullptr, kp_grid_coord(xx, ow), kp_grid_coord(yy, oh),
                         g_jac ? g_jac + 4 * bk : nullptr, px + K + 4 * (njm == 1 ? 0 : c));
        if (g_heatmap) a += g_heatmap[bk * ((size_t)oh * ow) + (size_t)yy * ow + xx];
        return p * (a - cst[bk]) / temperature;
    }
    if (!g_jac) return 0.f;
    const int m = (c - K) >> 2, cc = (c - K) & 3;
    if (njm != 1) {   // map m belongs to key point m
        const size_t bk = (size_t)b * K + m;
        return g_jac[4 * bk + cc] * (expf(px[m] / temperature - stats[2 * bk]) / stats[2 * bk + 1]);
    }
    float t = 0.f;    // the single map feeds every key point: key-point order
    for (int k = 0; k < K; ++k) {
        const size_t bk = (size_t)b * K + k;
        t = fmaf(g_jac[4 * bk + cc], expf(px[k] / temperature - stats[2 * bk]) / stats[2 * bk + 1], t);
    }
    return t;
}

__global__ __launch_bounds__(256) void kp_head_backward_kernel(const float* __restrict__ logits, const float* __restrict__ stats,
                                                              const float* __restrict__ cst, const float* __restrict__ g_value,
                                                              const float* __restrict__ g_jac, const float* __restrict__ g_heatmap, int B, int K,
                                                              int njm, int h, int w, int Cs, int off, int oh, int ow, float temperature,
                                                              float* __restrict__ grad) {
    const int q4 = Cs >> 2;                       // lanes per pixel
    const int total = B * h * w * q4;             // (< 2^31: the launcher's check)
    const int cend = K + 4 * njm;
    for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < total; g += gridDim.x * blockDim.x) {
        const int pix = g / q4, c0 = 4 * (g - pix * q4);
        const int xx = pix % w - off, yy = (pix / w) % h - off;
        float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
        if (xx >= 0 && xx < ow && yy >= 0 && yy < oh && c0 < cend) {
            const float* px = logits + (size_t)pix * Cs;
            const int b = pix / (h * w);
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                o[j] = c0 + j < cend ? kp_head_grad_channel(px, stats, cst, g_value, g_jac, g_heatmap, b, c0 + j, K, njm, xx, yy, oh, ow, temperature)
                                     : 0.f;
            r = make_float4(o[0], o[1], o[2], o[3]);
        }
        *reinterpret_cast<float4*>(grad + (size_t)pix * Cs + c0) = r;
    }
}

}  // namespace

size_t kp_head_backward_workspace_floats(int B, int K) { return (size_t)B * K * (KP_HEAD_BWD_SLICES + 1); }

hipError_t kp_head_backward_launch(const float* logits, const float* stats, const float* value, const float* jacobian, const float* g_value,
                                   const float* g_jacobian, const float* g_heatmap, int B, int K, int njm, int h, int w, int Cs, int pad,
                                   float temperature, float* grad_logits, float* ws, hipStream_t s) {
    const int off = 3 - pad, oh = h - 2 * off, ow = w - 2 * off;
    if (off < 0 || oh < 1 || ow < 1 || B < 1 || K < 1 || (Cs & 3) || Cs < K + 4 * njm || (njm != 0 && njm != 1 && njm != K) ||
        (long long)B * h * w * Cs >= (1ll << 31) || B > 65535)
        return hipErrorInvalidValue;
    if (njm == 0) g_jacobian = nullptr;
    if (g_jacobian && !jacobian) return hipErrorInvalidValue;
    const int S = KP_HEAD_BWD_SLICES;
    float* part = ws;
    float* cst = ws + (size_t)B * K * S;
    if (g_heatmap)
        hipLaunchKernelGGL(kp_head_bwd_hmdot_kernel, dim3(B, S, (K + KP_BWD_KG - 1) / KP_BWD_KG), dim3(256), 0, s, logits, stats, g_heatmap, K, h,
                           w, Cs, off, oh, ow, temperature, S, part);
    hipLaunchKernelGGL(kp_head_bwd_const_kernel, dim3((B * K + 255) / 256), dim3(256), 0, s, stats, value, jacobian, g_value, g_jacobian,
                       g_heatmap ? part : nullptr, B * K, S, cst);
    // HBM-bound: up to 8 blocks per CU, the rest of the pixels by the grid stride
    const long long lanes = (long long)B * h * w * (Cs >> 2);
    const int blocks = (int)std::min<long long>((lanes + 255) / 256, 2048);
    hipLaunchKernelGGL(kp_head_backward_kernel, dim3(blocks), dim3(256), 0, s, logits, stats, cst, g_value, g_jacobian, g_heatmap, B, K, njm, h,
                       w, Cs, off, oh, ow, temperature, grad_logits);
    return hipGetLastError();
}

}  // namespace eamm
