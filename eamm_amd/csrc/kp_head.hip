// The key-point heads' reduction, forward next to backward (reference modules/keypoint_detector.py:77-105 / :180-205): temperature
// softmax over the interior window of the 7x7 "same" convolution's NHWC output, soft-argmax, heat-map weighted sum of the jacobian
// maps.
//
// Forward: one block per (image, key point) for few images (kp_head_kernel), pixel slices over the whole chip + a combine step for
// batched calls (kp_head_slice_kernel, kp_head_combine_kernel, kp_head_heatmap_kernel).
//
// Backward: with p = softmax(l / T) over the window and, per (image b, key point k, pixel i),
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
#include "pointwise.h"

#include <algorithm>

namespace eamm {

// The Cs logits of pixel i (row-major) of the oh x ow window that starts at (off, off) of an image's [h,w,Cs] map `base`.
__device__ __forceinline__ const float* window_pixel(const float* __restrict__ base, int i, int ow, int off, int w, int Cs) {
    return base + (size_t)((i / ow + off) * w + i % ow + off) * Cs;
}

// ---- forward ----
// One block per (key point k, image b).  logits: [B,h,w,Cs] from the 7x7 "same" MFMA convolution; channel k is
// the key-point logit, channels K + 4*m + c the jacobian maps.  The reference convolves with padding `pad` (0),
// i.e. only the interior [off, off+oh) x [off, off+ow), off = 3 - pad, exists: heatmap = softmax(logit /
// temperature) over that window, value = sum heatmap * grid(oh, ow), jacobian = sum heatmap * jacobian_map.
__global__ __launch_bounds__(256) void kp_head_kernel(const float* __restrict__ logits, int K, int njm, int h, int w,
                                                      int Cs, int off, int oh, int ow, float temperature,
                                                      float* __restrict__ value, float* __restrict__ jacobian,
                                                      float* __restrict__ heatmap, float* __restrict__ stats) {
    __shared__ float red[BLOCK_WAVES];
    const int k = blockIdx.x, b = blockIdx.y;
    const int n = oh * ow;
    const float* base = logits + (size_t)b * h * w * Cs;
    float m = -INFINITY;
    for (int i = threadIdx.x; i < n; i += blockDim.x) m = fmaxf(m, window_pixel(base, i, ow, off, w, Cs)[k] / temperature);
    m = block_reduce<MaxOp>(m, red);
    float s = 0.f, vx = 0.f, vy = 0.f, j0 = 0.f, j1 = 0.f, j2 = 0.f, j3 = 0.f;
    const int jm = njm > 0 ? K + 4 * (njm == 1 ? 0 : k) : 0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int yy = i / ow, xx = i % ow;
        const float* px = window_pixel(base, i, ow, off, w, Cs);
        const float e = expf(px[k] / temperature - m);
        s += e;
        vx = fmaf(e, grid_coord(xx, ow), vx);
        vy = fmaf(e, grid_coord(yy, oh), vy);
        if (njm > 0) {
            j0 = fmaf(e, px[jm + 0], j0);
            j1 = fmaf(e, px[jm + 1], j1);
            j2 = fmaf(e, px[jm + 2], j2);
            j3 = fmaf(e, px[jm + 3], j3);
        }
    }
    s = block_reduce<SumOp>(s, red);
    vx = block_reduce<SumOp>(vx, red);
    vy = block_reduce<SumOp>(vy, red);
    if (njm > 0) {
        j0 = block_reduce<SumOp>(j0, red);
        j1 = block_reduce<SumOp>(j1, red);
        j2 = block_reduce<SumOp>(j2, red);
        j3 = block_reduce<SumOp>(j3, red);
    }
    if (threadIdx.x == 0) {
        value[((size_t)b * K + k) * 2 + 0] = vx / s;
        value[((size_t)b * K + k) * 2 + 1] = vy / s;
        if (njm > 0 && jacobian) {
            float* jo = jacobian + ((size_t)b * K + k) * 4;
            jo[0] = j0 / s; jo[1] = j1 / s; jo[2] = j2 / s; jo[3] = j3 / s;
        }
        if (stats) {      // the softmax's maximum and denominator, for the backward
            stats[((size_t)b * K + k) * 2 + 0] = m;
            stats[((size_t)b * K + k) * 2 + 1] = s;
        }
    }
    if (heatmap) {
        float* ho = heatmap + ((size_t)b * K + k) * n;
        for (int i = threadIdx.x; i < n; i += blockDim.x) ho[i] = expf(window_pixel(base, i, ow, off, w, Cs)[k] / temperature - m) / s;
    }
}

// Round 6, batched calls: the reductions split over PIXEL SLICES so that the whole chip streams the logits, each line read by one block.
// The per-(image, key point) kernel above runs K x B blocks that each read one float of every 256-byte logit line three times over;
// with one block per image (a first version of this round, 109 us per 64-frame batch against 116) the 67 MB of a batch hang on 64 CUs
// at ~30 GB/s each.  Here block (b, slice) owns n / S pixels and ALL key points of a group of KG: pass 1 its slice's maxima, pass 2 the
// sums relative to them (the slice's lines come out of the L2 the second time) -> `part` [B][K][S][8] = (max, s, vx, vy, j0..j3).
// kp_head_combine_kernel folds the slices in slice order: M = max m_s, total = sum_s exp(m_s - M) * part_s (deterministic; the
// rescaling rounds once more than the one-block form: <= 2e-7 of the value), writes value / jacobian and (M, S) for the optional
// heat-map pass kp_head_heatmap_kernel.
template <int KG>
__global__ __launch_bounds__(256) void kp_head_slice_kernel(const float* __restrict__ logits, int K, int njm, int h, int w, int Cs,
                                                            int off, int oh, int ow, float temperature, int S,
                                                            float* __restrict__ part) {
    constexpr int NV = 7;                       // s, vx, vy, j0..j3
    __shared__ float red[BLOCK_WAVES][KG * NV];   // one row per wave
    __shared__ float fin[KG];
    const int b = blockIdx.x, sl = blockIdx.y, k0 = blockIdx.z * KG;
    const int kn = min(KG, K - k0);
    const int n = oh * ow;
    const int i0 = (int)((long long)n * sl / S), i1 = (int)((long long)n * (sl + 1) / S);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float* base = logits + (size_t)b * h * w * Cs;
    float m[KG];
#pragma unroll
    for (int k = 0; k < KG; ++k) m[k] = -INFINITY;
    for (int i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
        const float* px = window_pixel(base, i, ow, off, w, Cs) + k0;
#pragma unroll
        for (int k = 0; k < KG; ++k)
            if (k < kn) m[k] = fmaxf(m[k], px[k] / temperature);
    }
#pragma unroll
    for (int k = 0; k < KG; ++k) {
        m[k] = wave_reduce<MaxOp>(m[k]);
        if (lane == 0) red[wave][k] = m[k];
    }
    __syncthreads();
    if (threadIdx.x < KG) fin[threadIdx.x] = fold_waves<MaxOp>(&red[0][threadIdx.x], KG * NV);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < KG; ++k) m[k] = fin[k];
    __syncthreads();
    float acc[KG][NV];
#pragma unroll
    for (int k = 0; k < KG; ++k)
#pragma unroll
        for (int v = 0; v < NV; ++v) acc[k][v] = 0.f;
    for (int i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
        const int yy = i / ow, xx = i % ow;
        const float* px = window_pixel(base, i, ow, off, w, Cs);
        const float gx = grid_coord(xx, ow), gy = grid_coord(yy, oh);
#pragma unroll
        for (int k = 0; k < KG; ++k) {
            if (k < kn) {
                const float e = expf(px[k0 + k] / temperature - m[k]);
                acc[k][0] += e;
                acc[k][1] = fmaf(e, gx, acc[k][1]);
                acc[k][2] = fmaf(e, gy, acc[k][2]);
                if (njm > 0) {
                    const float* pj = px + K + 4 * (njm == 1 ? 0 : k0 + k);
                    acc[k][3] = fmaf(e, pj[0], acc[k][3]);
                    acc[k][4] = fmaf(e, pj[1], acc[k][4]);
                    acc[k][5] = fmaf(e, pj[2], acc[k][5]);
                    acc[k][6] = fmaf(e, pj[3], acc[k][6]);
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < KG; ++k)
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const float x = wave_reduce<SumOp>(acc[k][v]);
            if (lane == 0) red[wave][k * NV + v] = x;
        }
    __syncthreads();
    if (threadIdx.x < kn * 8) {
        const int k = threadIdx.x >> 3, v = threadIdx.x & 7;
        const float r = v == 0 ? fin[k] : fold_waves<SumOp>(&red[0][k * NV + v - 1], KG * NV);
        part[(((size_t)b * K + k0 + k) * S + sl) * 8 + v] = r;
    }
}

__global__ __launch_bounds__(64) void kp_head_combine_kernel(const float* __restrict__ part, int K, int njm, int S,
                                                            float* __restrict__ value, float* __restrict__ jacobian,
                                                            float* __restrict__ stats) {
    const int b = blockIdx.x;
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        const float* p = part + ((size_t)b * K + k) * S * 8;
        float M = -INFINITY;
        for (int sl = 0; sl < S; ++sl) M = fmaxf(M, p[sl * 8]);
        float t[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int sl = 0; sl < S; ++sl) {
            const float sc = expf(p[sl * 8] - M);        // (an empty slice has max -inf: scale 0, sums 0)
#pragma unroll
            for (int v = 0; v < 7; ++v) t[v] = fmaf(sc, p[sl * 8 + 1 + v], t[v]);
        }
        value[((size_t)b * K + k) * 2 + 0] = t[1] / t[0];
        value[((size_t)b * K + k) * 2 + 1] = t[2] / t[0];
        if (njm > 0 && jacobian) {
            float* jo = jacobian + ((size_t)b * K + k) * 4;
            jo[0] = t[3] / t[0]; jo[1] = t[4] / t[0]; jo[2] = t[5] / t[0]; jo[3] = t[6] / t[0];
        }
        stats[((size_t)b * K + k) * 2 + 0] = M;
        stats[((size_t)b * K + k) * 2 + 1] = t[0];
    }
}

__global__ __launch_bounds__(256) void kp_head_heatmap_kernel(const float* __restrict__ logits, const float* __restrict__ stats, int K, int h,
                                                             int w, int Cs, int off, int oh, int ow, float temperature, int S,
                                                             float* __restrict__ heatmap) {
    const int b = blockIdx.x, sl = blockIdx.y;
    const int n = oh * ow;
    const int i0 = (int)((long long)n * sl / S), i1 = (int)((long long)n * (sl + 1) / S);
    const float* base = logits + (size_t)b * h * w * Cs;
    const float* st = stats + (size_t)b * K * 2;
    for (int k = 0; k < K; ++k) {      // (k outer: a wave's stores of one key point are contiguous)
        const float M = st[2 * k], Sd = st[2 * k + 1];
        float* ho = heatmap + ((size_t)b * K + k) * n;
        for (int i = i0 + threadIdx.x; i < i1; i += blockDim.x)
            ho[i] = expf(window_pixel(base, i, ow, off, w, Cs)[k] / temperature - M) / Sd;
    }
}

size_t kp_head_workspace_floats(int B, int K) { return (size_t)B * K * (KP_HEAD_SLICES * 8 + 2); }

hipError_t kp_head_launch(const float* logits, int B, int K, int njm, int h, int w, int Cs, int pad, float temperature,
                          float* value, float* jacobian, float* heatmap, hipStream_t s, float* ws, float* stats_out) {
    const int off = 3 - pad, oh = h - 2 * off, ow = w - 2 * off;
    if (off < 0 || oh < 1 || ow < 1) return hipErrorInvalidValue;
    // batched calls with a workspace: pixel slices over the whole chip + a combine step (round 6, kp_head_slice_kernel above).  Few images
    // (or no workspace): one block per (image, key point).  EAMM_KP_HEAD_SLICE_MIN_B (tuning aid): < 0 never
    static const int slice_min_b = (int)knob_int("EAMM_KP_HEAD_SLICE_MIN_B", 8);
    if (ws != nullptr && slice_min_b >= 0 && B >= slice_min_b) {
        constexpr int KG = 10;
        const int S = KP_HEAD_SLICES;
        float* part = ws;
        float* stats = stats_out ? stats_out : ws + (size_t)B * K * S * 8;
        hipLaunchKernelGGL(kp_head_slice_kernel<KG>, dim3(B, S, (K + KG - 1) / KG), dim3(256), 0, s, logits, K, njm, h, w, Cs, off, oh, ow,
                           temperature, S, part);
        hipLaunchKernelGGL(kp_head_combine_kernel, dim3(B), dim3(64), 0, s, part, K, njm, S, value, jacobian, stats);
        if (heatmap)
            hipLaunchKernelGGL(kp_head_heatmap_kernel, dim3(B, S), dim3(256), 0, s, logits, stats, K, h, w, Cs, off, oh, ow, temperature, S, heatmap);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(kp_head_kernel, dim3(K, B), dim3(256), 0, s, logits, K, njm, h, w, Cs, off, oh, ow, temperature,
                       value, jacobian, heatmap, stats_out);
    return hipGetLastError();
}

// ---- backward ----
namespace {

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
    __shared__ float red[BLOCK_WAVES][KG];
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
        const float* px = window_pixel(base, i, ow, off, w, Cs) + k0;
#pragma unroll
        for (int k = 0; k < KG; ++k)
            if (k < kn) acc[k] = fmaf(expf(px[k] / temperature - m[k]), gh[(size_t)k * n + i], acc[k]);
    }
#pragma unroll
    for (int k = 0; k < KG; ++k) {
        const float x = wave_reduce<SumOp>(acc[k]);
        if (lane == 0) red[wave][k] = x;
    }
    __syncthreads();
    if ((int)threadIdx.x < kn)
        part[((size_t)b * K + k0 + threadIdx.x) * S + sl] = fold_waves<SumOp>(&red[0][threadIdx.x], KG);
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
        float a = kp_dot(g_value ? g_value + 2 * bk : nullptr, grid_coord(xx, ow), grid_coord(yy, oh),
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
