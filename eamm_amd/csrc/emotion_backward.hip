// Backward of the emotion detector's small kernels (emotion.hip): the stem's MaxPool2d(3, 2, 1) and the Conv1d `final` stack
// (reference modules/util.py:1245, :1287-1295; differentiated there by autograd when model.py:312-413 trains Emotion_k).
// Gather form, fixed summation order, no atomics: every gradient element is written once and a frame's result does not depend on
// the batch it is computed in.
#include "kernels.h"

#include <algorithm>

namespace eamm {

namespace {
// the window (oy, ox)'s winner as ATen's CPU kernel picks it: taps in (ky, kx) raster order, a later tap only replaces the current
// one when it is larger (or NaN), so the FIRST maximum keeps the gradient; returns its pixel index y * W + x
__device__ __forceinline__ int maxpool_winner(const float* __restrict__ plane, int oy, int ox, int H, int W, int C) {
    const int y0 = max(2 * oy - 1, 0), y1 = min(2 * oy + 2, H), x0 = max(2 * ox - 1, 0), x1 = min(2 * ox + 2, W);
    int best = y0 * W + x0;
    float m = -INFINITY;
    for (int yy = y0; yy < y1; ++yy)
        for (int xx = x0; xx < x1; ++xx) {
            const float v = plane[(size_t)(yy * W + xx) * C];
            if (v > m || v != v) {
                m = v;
                best = yy * W + xx;
            }
        }
    return best;
}
}  // namespace

// dx[b,y,x,c] = the sum of dy over the (up to four) windows whose winner, recomputed from the saved input, is (y, x)
__global__ __launch_bounds__(256) void emo_maxpool_backward_kernel(const float* __restrict__ in, const float* __restrict__ dy, int B, int H,
                                                                   int W, int C, float* __restrict__ dx) {
    const int Ho = H / 2, Wo = W / 2;
    const size_t total = (size_t)B * H * W * C;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        size_t t = i / C;
        const int x = (int)(t % W);
        t /= W;
        const int y = (int)(t % H);
        const int b = (int)(t / H);
        const float* plane = in + (size_t)b * H * W * C + c;
        // an even coordinate lies in window i / 2 only, an odd one in (i - 1) / 2 and (i + 1) / 2
        const int oy0 = y >> 1, oy1 = (y + 1) >> 1, ox0 = x >> 1, ox1 = (x + 1) >> 1;
        float s = 0.f;
        for (int oy = oy0; oy <= oy1 && oy < Ho; ++oy)
            for (int ox = ox0; ox <= ox1 && ox < Wo; ++ox)
                if (maxpool_winner(plane, oy, ox, H, W, C) == y * W + x) s += dy[(((size_t)b * Ho + oy) * Wo + ox) * C + c];
        dx[i] = s;
    }
}

// One thread per frame: emo_final_kernel's forward again (the activations are 160 floats), then its backward.  da [B,64] is
// written directly; the frame's 98 weight gradients go to part[b][98], which emo_final_wgrad_reduce_kernel adds over the frames.
// w: c1w[2*4] c1b[2] c2w[4*2*4] c2b[4] c3w[4*4*3] c3b[4]
__global__ __launch_bounds__(64) void emo_final_backward_kernel(const float* __restrict__ a, const float* __restrict__ w,
                                                                const float* __restrict__ g_value, const float* __restrict__ g_jacobian, int B,
                                                                float* __restrict__ da, float* __restrict__ part) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float *c1w = w, *c1b = w + 8, *c2w = w + 10, *c2b = w + 42, *c3w = w + 46;
    const float* x = a + (size_t)b * 64;
    float y1[2][32];
    for (int o = 0; o < 2; ++o)
        for (int t = 0; t < 32; ++t) {
            float s = 0.f;
            for (int k = 0; k < 4; ++k) {
                const int i = 2 * t - 1 + k;
                if (i >= 0 && i < 64) s = fmaf(c1w[o * 4 + k], x[i], s);
            }
            y1[o][t] = s + c1b[o];
        }
    float y2[2][16];
    for (int o = 0; o < 2; ++o)
        for (int t = 0; t < 16; ++t) y2[o][t] = fmaxf(fmaxf(y1[o][2 * t], y1[o][2 * t + 1]), 0.f);
    float y3[4][8];
    for (int o = 0; o < 4; ++o)
        for (int t = 0; t < 8; ++t) {
            float s = 0.f;
            for (int c = 0; c < 2; ++c)
                for (int k = 0; k < 4; ++k) {
                    const int i = 2 * t - 1 + k;
                    if (i >= 0 && i < 16) s = fmaf(c2w[(o * 2 + c) * 4 + k], y2[c][i], s);
                }
            y3[o][t] = fmaxf(s + c2b[o], 0.f);
        }
    // r[o][t] (t < 2: value, else jacobian): its gradient; an output the loss does not read has none
    float gr[4][6];
    for (int o = 0; o < 4; ++o)
        for (int t = 0; t < 6; ++t)
            gr[o][t] = t < 2 ? (g_value ? g_value[((size_t)b * 4 + o) * 2 + t] : 0.f) : (g_jacobian ? g_jacobian[((size_t)b * 4 + o) * 4 + (t - 2)] : 0.f);
    float* gw = part + (size_t)b * 98;
    // Conv1d(4,4,3)
    float d3[4][8];
    for (int c = 0; c < 4; ++c)
        for (int u = 0; u < 8; ++u) d3[c][u] = 0.f;
    for (int o = 0; o < 4; ++o) {
        float sb = 0.f;
        for (int t = 0; t < 6; ++t) sb += gr[o][t];
        gw[94 + o] = sb;
        for (int c = 0; c < 4; ++c)
            for (int k = 0; k < 3; ++k) {
                float s = 0.f;
                const float wv = c3w[(o * 4 + c) * 3 + k];
                for (int t = 0; t < 6; ++t) {
                    s = fmaf(gr[o][t], y3[c][t + k], s);
                    d3[c][t + k] = fmaf(wv, gr[o][t], d3[c][t + k]);
                }
                gw[46 + (o * 4 + c) * 3 + k] = s;
            }
    }
    // ReLU, Conv1d(2,4,4,2,1)
    float d2[2][16];
    for (int c = 0; c < 2; ++c)
        for (int i = 0; i < 16; ++i) d2[c][i] = 0.f;
    for (int o = 0; o < 4; ++o) {
        float sb = 0.f;
        for (int t = 0; t < 8; ++t) {
            if (!(y3[o][t] > 0.f)) d3[o][t] = 0.f;
            sb += d3[o][t];
        }
        gw[42 + o] = sb;
        for (int c = 0; c < 2; ++c)
            for (int k = 0; k < 4; ++k) {
                float s = 0.f;
                const float wv = c2w[(o * 2 + c) * 4 + k];
                for (int t = 0; t < 8; ++t) {
                    const int i = 2 * t - 1 + k;
                    if (i >= 0 && i < 16) {
                        s = fmaf(d3[o][t], y2[c][i], s);
                        d2[c][i] = fmaf(wv, d3[o][t], d2[c][i]);
                    }
                }
                gw[10 + (o * 2 + c) * 4 + k] = s;
            }
    }
    // ReLU, MaxPool1d(2,2) (the first of two equal values takes the gradient), Conv1d(1,2,4,2,1)
    float dxv[64];
    for (int i = 0; i < 64; ++i) dxv[i] = 0.f;
    for (int o = 0; o < 2; ++o) {
        float d1[32];
        float sb = 0.f;
        for (int t = 0; t < 16; ++t) {
            const float g = y2[o][t] > 0.f ? d2[o][t] : 0.f;
            const bool first = !(y1[o][2 * t + 1] > y1[o][2 * t]);
            d1[2 * t] = first ? g : 0.f;
            d1[2 * t + 1] = first ? 0.f : g;
            sb += g;
        }
        gw[8 + o] = sb;
        for (int k = 0; k < 4; ++k) {
            float s = 0.f;
            const float wv = c1w[o * 4 + k];
            for (int t = 0; t < 32; ++t) {
                const int i = 2 * t - 1 + k;
                if (i >= 0 && i < 64) {
                    s = fmaf(d1[t], x[i], s);
                    dxv[i] = fmaf(wv, d1[t], dxv[i]);
                }
            }
            gw[o * 4 + k] = s;
        }
    }
    for (int i = 0; i < 64; ++i) da[(size_t)b * 64 + i] = dxv[i];
}

// dw[j] = sum over the frames of part[b][j], b ascending
__global__ __launch_bounds__(128) void emo_final_wgrad_reduce_kernel(const float* __restrict__ part, int B, float* __restrict__ dw) {
    const int j = threadIdx.x;
    if (j >= 98) return;
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += part[(size_t)b * 98 + j];
    dw[j] = s;
}

hipError_t emo_maxpool_backward_launch(const float* in, const float* dy, int B, int H, int W, int C, float* dx, hipStream_t s) {
    const size_t total = (size_t)B * H * W * C;
    hipLaunchKernelGGL(emo_maxpool_backward_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 65536)), dim3(256), 0, s, in, dy, B, H,
                       W, C, dx);
    return hipGetLastError();
}

size_t emo_final_backward_workspace_floats(int B) { return (size_t)B * 98; }

hipError_t emo_final_backward_launch(const float* a, const float* w, const float* g_value, const float* g_jacobian, int B, float* da,
                                     float* dw, float* workspace, hipStream_t s) {
    hipLaunchKernelGGL(emo_final_backward_kernel, dim3((B + 63) / 64), dim3(64), 0, s, a, w, g_value, g_jacobian, B, da, workspace);
    hipLaunchKernelGGL(emo_final_wgrad_reduce_kernel, dim3(1), dim3(128), 0, s, workspace, B, dw);
    return hipGetLastError();
}

}  // namespace eamm
