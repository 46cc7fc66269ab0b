// Small kernels of the emotion detector Emotion_k (reference modules/util.py:1223-1527) around its convolutions: the stem's
// MaxPool2d(3, 2, 1), AdaptiveAvgPool2d(1), the positional embedding get_embedder(10) (util.py:97-145), the fully connected
// layers (classify.last_fc, fc_p, fc_all) and the Conv1d `final` stack.  Every reduction runs in a fixed order, without atomics,
// so a frame's result does not depend on the batch it is computed in.
#include "kernels.h"

#include <algorithm>

namespace eamm {

// NHWC [B,H,W,C] -> [B,H/2,W/2,C]; the padding never wins (as -inf)
__global__ __launch_bounds__(256) void emo_maxpool_kernel(const float* __restrict__ in, int B, int H, int W, int C,
                                                          float* __restrict__ out) {
    const int Ho = H / 2, Wo = W / 2;
    const size_t total = (size_t)B * Ho * Wo * C;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        size_t t = i / C;
        const int x = (int)(t % Wo);
        t /= Wo;
        const int y = (int)(t % Ho);
        const int b = (int)(t / Ho);
        float m = -INFINITY;
        for (int dy = -1; dy <= 1; ++dy) {
            const int yy = 2 * y + dy;
            if (yy < 0 || yy >= H) continue;
            for (int dx = -1; dx <= 1; ++dx) {
                const int xx = 2 * x + dx;
                if (xx < 0 || xx >= W) continue;
                m = fmaxf(m, in[(((size_t)b * H + yy) * W + xx) * C + c]);
            }
        }
        out[i] = m;
    }
}

// NHWC [B,P,C] -> [B,C]: the mean over the P pixels, summed in raster order
__global__ __launch_bounds__(256) void emo_avgpool_kernel(const float* __restrict__ in, int B, int P, int C, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * C) return;
    const int b = i / C, c = i - b * C;
    const float* q = in + (size_t)b * P * C + c;
    float s = 0.f;
    for (int p = 0; p < P; ++p) s += q[(size_t)p * C];
    out[i] = s / (float)P;
}

// (value [B,10,2], jacobian [B,10,2,2]) -> [B,10*126]: per key point the six numbers d = (vx, vy, j00, j01, j10, j11) as
// [d, sin(d), cos(d), sin(2d), cos(2d), ..., sin(512d), cos(512d)] (include_input, log-sampled frequencies 2^0 .. 2^9).
// x * 2^f is exact in fp32; sinf / cosf are the accurate library functions (arguments reach ~1e3 rad).
__global__ __launch_bounds__(256) void emo_embed_kernel(const float* __restrict__ value, const float* __restrict__ jacobian, int B,
                                                        float* __restrict__ out) {
    constexpr int KP = 10, E = 126;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * KP * E) return;
    const int j = i % E, k = (i / E) % KP, b = i / (E * KP);
    const int fn = j / 6, d = j - fn * 6;
    const int bk = b * KP + k;
    const float x = d < 2 ? value[bk * 2 + d] : jacobian[bk * 4 + d - 2];
    float v = x;
    if (fn > 0) {
        const float a = x * (float)(1 << ((fn - 1) >> 1));
        v = ((fn - 1) & 1) ? cosf(a) : sinf(a);
    }
    out[i] = v;
}

// out[b, o] = act(bias[o] + sum_k x[b, k] w[k, o]) with x = [x0 (K0 columns) | x1 (K1 columns)] and the weight transposed
// ([K0+K1][O]: consecutive lanes read consecutive outputs).  EMO_FR frames per workgroup share each weight load; k ascends.
constexpr int EMO_FR = 8;
__global__ __launch_bounds__(256) void emo_linear_kernel(const float* __restrict__ x0, int K0, const float* __restrict__ x1, int K1,
                                                         const float* __restrict__ wt, const float* __restrict__ bias, int O, int B,
                                                         int relu, float* __restrict__ out) {
    extern __shared__ float xs[];   // [EMO_FR][K0+K1]
    const int K = K0 + K1;
    const int b0 = blockIdx.y * EMO_FR, nb = min(EMO_FR, B - b0);
    for (int i = threadIdx.x; i < EMO_FR * K; i += blockDim.x) {
        const int f = i / K, k = i - f * K;
        float v = 0.f;
        if (f < nb) v = k < K0 ? x0[(size_t)(b0 + f) * K0 + k] : x1[(size_t)(b0 + f) * K1 + (k - K0)];
        xs[i] = v;
    }
    __syncthreads();
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= O) return;
    float acc[EMO_FR];
#pragma unroll
    for (int f = 0; f < EMO_FR; ++f) acc[f] = 0.f;
    for (int k = 0; k < K; ++k) {
        const float w = wt[(size_t)k * O + o];
#pragma unroll
        for (int f = 0; f < EMO_FR; ++f) acc[f] = fmaf(xs[f * K + k], w, acc[f]);
    }
    const float bo = bias[o];
#pragma unroll
    for (int f = 0; f < EMO_FR; ++f) {
        if (f >= nb) break;
        float v = acc[f] + bo;
        if (relu) v = fmaxf(v, 0.f);
        out[(size_t)(b0 + f) * O + o] = v;
    }
}

// `final` on the [B,1,64] fc_all output (util.py:1266-1274): Conv1d(1,2,4,2,1) -> MaxPool1d(2,2) -> ReLU -> Conv1d(2,4,4,2,1) -> ReLU
// -> Conv1d(4,4,3) = r [B,4,6]; value = r[:,:,:2] -> [B,4,2], jacobian = r[:,:,2:] -> [B,4,2,2].  One thread per frame.
// w: c1w[2*4] c1b[2] c2w[4*2*4] c2b[4] c3w[4*4*3] c3b[4]
__global__ __launch_bounds__(64) void emo_final_kernel(const float* __restrict__ a, const float* __restrict__ w, int B,
                                                       float* __restrict__ value, float* __restrict__ jacobian) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float *c1w = w, *c1b = w + 8, *c2w = w + 10, *c2b = w + 42, *c3w = w + 46, *c3b = w + 94;
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
    for (int o = 0; o < 4; ++o)
        for (int t = 0; t < 6; ++t) {
            float s = 0.f;
            for (int c = 0; c < 4; ++c)
                for (int k = 0; k < 3; ++k) s = fmaf(c3w[(o * 4 + c) * 3 + k], y3[c][t + k], s);
            const float r = s + c3b[o];
            if (t < 2) {
                if (value) value[((size_t)b * 4 + o) * 2 + t] = r;
            } else if (jacobian) {
                jacobian[((size_t)b * 4 + o) * 4 + (t - 2)] = r;
            }
        }
}

static int grid_for(size_t n) { return (int)std::min<size_t>((n + 255) / 256, 65536); }

hipError_t emo_maxpool_launch(const float* in, int B, int H, int W, int C, float* out, hipStream_t s) {
    hipLaunchKernelGGL(emo_maxpool_kernel, dim3(grid_for((size_t)B * (H / 2) * (W / 2) * C)), dim3(256), 0, s, in, B, H, W, C, out);
    return hipGetLastError();
}

hipError_t emo_avgpool_launch(const float* in, int B, int P, int C, float* out, hipStream_t s) {
    hipLaunchKernelGGL(emo_avgpool_kernel, dim3((B * C + 255) / 256), dim3(256), 0, s, in, B, P, C, out);
    return hipGetLastError();
}

hipError_t emo_embed_launch(const float* value, const float* jacobian, int B, float* out, hipStream_t s) {
    hipLaunchKernelGGL(emo_embed_kernel, dim3((B * 1260 + 255) / 256), dim3(256), 0, s, value, jacobian, B, out);
    return hipGetLastError();
}

hipError_t emo_linear_launch(const float* x0, int K0, const float* x1, int K1, const float* wt, const float* bias, int O, int B,
                             int relu, float* out, hipStream_t s) {
    const size_t lds = sizeof(float) * EMO_FR * (K0 + K1);
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    hipLaunchKernelGGL(emo_linear_kernel, dim3((O + 255) / 256, (B + EMO_FR - 1) / EMO_FR), dim3(256), lds, s, x0, K0, x1, K1, wt, bias,
                       O, B, relu, out);
    return hipGetLastError();
}

hipError_t emo_final_launch(const float* a, const float* w, int B, float* value, float* jacobian, hipStream_t s) {
    hipLaunchKernelGGL(emo_final_kernel, dim3((B + 63) / 64), dim3(64), 0, s, a, w, B, value, jacobian);
    return hipGetLastError();
}

}  // namespace eamm
