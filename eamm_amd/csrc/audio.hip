// Kernels of the audio network AT_net2 (reference modules/util.py:514-612) that the convolution kernels do not cover:
//   audio_conv1      audio_eocder.0: conv2d(1, 64, 3, 1, 1) + BatchNorm (folded) + ReLU on the raw MFCC window, NHWC-64 out
//   audio_maxpool    nn.MaxPool2d(3, stride) without padding, NHWC
//   audio_scale      `audio_eocder_fc(...) * weight` (util.py:593; weight is a run-time argument, never folded)
//   lstm_rec         the LSTM recurrence of one layer (nn.LSTM gate order i, f, g, o) over S steps, one persistent launch
//
// lstm_rec: LSTM_WG = 16 workgroups of 256 threads, one per CU (84 KB of LDS each).  Workgroup g owns hidden units
// 16g .. 16g+15: the 64 rows of W_hh that feed them (their four gates) stay in LDS for the whole launch, so the cell update is
// local and only h_t (N x 256 floats) crosses workgroups each step.  That hand-off uses data-tagged granules
// (cdna_hip_programming.md §6 Guideline 16, R2): every h value is published as one 8-byte {tag, value} word by an agent-scope
// atomic store, double-buffered by step parity, and every workgroup polls the N x 256 words with agent-scope atomic loads until
// all tags equal the step's tag; no flag and no fence.  Tags are a per-handle counter that never repeats, so stale words of
// earlier launches never match.  Every wait is bounded by a wall-clock limit; on expiry the workgroup writes the error word
// (host-visible) and leaves.  The input projection x W_ih^T + b arrives precomputed for every step (one GEMM per layer).
// Workgroup residency: 16 workgroups on a 256-CU chip, one per CU by their LDS use (MI355X_MICROARCH.md, Residency).
#include "conv_common.h"

namespace eamm {

__global__ __launch_bounds__(256) void audio_conv1_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ b, int F, int H, int W, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;   // (frame, y, x, channel), channel fastest
    if (i >= (size_t)F * H * W * 64) return;
    const int co = (int)(i & 63);
    const size_t p = i >> 6;
    const int xx = (int)(p % W), yy = (int)((p / W) % H);
    const size_t f = p / ((size_t)W * H);
    const float* xf = x + f * H * W;
    float acc = 0.f;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
        const int y = yy + dy - 1;
        if (y < 0 || y >= H) continue;
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int xs = xx + dx - 1;
            if (xs < 0 || xs >= W) continue;
            acc = fmaf(xf[y * W + xs], w[(dy * 3 + dx) * 64 + co], acc);
        }
    }
    out[i] = fmaxf(acc + b[co], 0.f);
}

__global__ __launch_bounds__(256) void audio_maxpool_kernel(const float* __restrict__ in, int F, int H, int W, int C, int sy, int sx,
                                                            int Ho, int Wo, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;   // (frame, oy, ox, channel / 4)
    const int C4 = C >> 2;
    if (i >= (size_t)F * Ho * Wo * C4) return;
    const int c4 = (int)(i % C4);
    const size_t p = i / C4;
    const int ox = (int)(p % Wo), oy = (int)((p / Wo) % Ho);
    const size_t f = p / ((size_t)Wo * Ho);
    const float4* src = reinterpret_cast<const float4*>(in);
    float4 m = src[((f * H + oy * sy) * W + ox * sx) * C4 + c4];
    for (int dy = 0; dy < 3; ++dy)
        for (int dx = 0; dx < 3; ++dx) {
            const float4 v = src[((f * H + oy * sy + dy) * W + ox * sx + dx) * C4 + c4];
            m.x = fmaxf(m.x, v.x);
            m.y = fmaxf(m.y, v.y);
            m.z = fmaxf(m.z, v.z);
            m.w = fmaxf(m.w, v.w);
        }
    reinterpret_cast<float4*>(out)[i] = m;
}

__global__ __launch_bounds__(256) void audio_scale_kernel(float* __restrict__ x, size_t n, float s) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] = x[i] * s;
}

hipError_t audio_conv1_launch(const float* x, const float* w, const float* b, int F, int H, int W, float* out, hipStream_t s) {
    const size_t n = (size_t)F * H * W * 64;
    hipLaunchKernelGGL(audio_conv1_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, w, b, F, H, W, out);
    return hipGetLastError();
}

hipError_t audio_maxpool_launch(const float* in, int F, int H, int W, int C, int sy, int sx, float* out, hipStream_t s) {
    if (C % 4 || H < 3 || W < 3) return hipErrorInvalidValue;
    const int Ho = (H - 3) / sy + 1, Wo = (W - 3) / sx + 1;
    const size_t n = (size_t)F * Ho * Wo * (C / 4);
    hipLaunchKernelGGL(audio_maxpool_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, F, H, W, C, sy, sx, Ho, Wo, out);
    return hipGetLastError();
}

hipError_t audio_scale_launch(float* x, size_t n, float scale, hipStream_t s) {
    hipLaunchKernelGGL(audio_scale_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, n, scale);
    return hipGetLastError();
}

// ---- LSTM recurrence -----------------------------------------------------------------------------------------------------------
constexpr int LSTM_HID = 256, LSTM_ROWS = 64, LSTM_MAXN = 8;
constexpr size_t LSTM_LDS_FLOATS = (size_t)LSTM_HID * LSTM_ROWS + LSTM_MAXN * LSTM_HID + 4 * LSTM_MAXN * LSTM_ROWS + LSTM_MAXN * LSTM_ROWS;

__device__ __forceinline__ float lstm_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }

__global__ __launch_bounds__(256) void lstm_rec_kernel(const LstmArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* Ws = sm;                                   // [256 k][64 r]: local row r = 16 * gate + unit
    float* hs = Ws + LSTM_HID * LSTM_ROWS;            // [N][256] h of the previous step
    float* red = hs + LSTM_MAXN * LSTM_HID;           // [4 k-quarters][N][64] partial dot products
    float* gs = red + 4 * LSTM_MAXN * LSTM_ROWS;      // [N][64] gate pre-activations
    const int g = blockIdx.x, tid = threadIdx.x, N = a.N;
    {
        const float4* src = reinterpret_cast<const float4*>(a.whh + (size_t)g * LSTM_HID * LSTM_ROWS);
        for (int i = tid; i < LSTM_HID * LSTM_ROWS / 4; i += 256) reinterpret_cast<float4*>(Ws)[i] = src[i];
    }
    const int cn = tid >> 4, cj = tid & 15, unit = g * 16 + cj;   // cell thread: clip cn, unit
    const bool cell = tid < N * 16;
    float c = cell ? a.c[cn * LSTM_HID + unit] : 0.f;
    float h = 0.f;
    for (int i = tid; i < N * LSTM_HID; i += 256) hs[i] = a.h0[i];
    __syncthreads();
    const int kq = tid >> 6, r = tid & 63;   // wave kq sums k in [64 kq, 64 kq + 64) for local row r
    for (int s = 0; s < a.S; ++s) {
        // this step's input projection (+ clip bias) for the gate sums below, loaded before the dot products hide its latency;
        // the N x 64 gate rows are spread over the 256 threads (two per thread for N > 4)
        float xv[2] = {0.f, 0.f};
        static_for<2>([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            const int i = tid + 256 * j;
            if (i < N * LSTM_ROWS) {
                const int n = i >> 6, rr = i & 63;
                const int grow = (rr >> 4) * LSTM_HID + g * 16 + (rr & 15);
                xv[j] = a.xproj[(size_t)(n * a.S + s) * 4 * LSTM_HID + grow];
                if (a.clipb) xv[j] += a.clipb[n * 4 * LSTM_HID + grow];
            }
        });
        float acc[LSTM_MAXN];
        static_for<LSTM_MAXN>([&](auto nc) { acc[decltype(nc)::value] = 0.f; });
        const float* wp = Ws + kq * 64 * LSTM_ROWS + r;
        const float* hp = hs + kq * 64;
        for (int k = 0; k < 64; ++k) {
            const float w = wp[k * LSTM_ROWS];
            static_for<LSTM_MAXN>([&](auto nc) {
                constexpr int n = decltype(nc)::value;
                if (n < N) acc[n] = fmaf(w, hp[n * LSTM_HID + k], acc[n]);
            });
        }
        static_for<LSTM_MAXN>([&](auto nc) {
            constexpr int n = decltype(nc)::value;
            if (n < N) red[(kq * LSTM_MAXN + n) * LSTM_ROWS + r] = acc[n];
        });
        __syncthreads();
        static_for<2>([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            const int i = tid + 256 * j;
            if (i < N * LSTM_ROWS) {
                const int n = i >> 6, rr = i & 63;
                float v = red[(0 * LSTM_MAXN + n) * LSTM_ROWS + rr] + red[(1 * LSTM_MAXN + n) * LSTM_ROWS + rr];
                v += red[(2 * LSTM_MAXN + n) * LSTM_ROWS + rr];
                v += red[(3 * LSTM_MAXN + n) * LSTM_ROWS + rr];
                gs[n * LSTM_ROWS + rr] = v + xv[j];
            }
        });
        __syncthreads();
        const unsigned tag = a.epoch0 + (unsigned)s;
        unsigned long long* gb = a.gran + (size_t)(s & 1) * LSTM_MAXN * LSTM_HID;
        if (cell) {
            const float* gp = gs + cn * LSTM_ROWS;
            const float ig = lstm_sigmoid(gp[cj]), fg = lstm_sigmoid(gp[16 + cj]), gg = tanhf(gp[32 + cj]), og = lstm_sigmoid(gp[48 + cj]);
            c = fg * c + ig * gg;
            h = og * tanhf(c);
            a.y[(size_t)cn * a.ystride + (size_t)s * LSTM_HID + unit] = h;
            __hip_atomic_store(gb + cn * LSTM_HID + unit, ((unsigned long long)tag << 32) | __float_as_uint(h), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        }
        if (s + 1 == a.S) break;
        // h_s of every workgroup -> LDS: thread tid polls unit tid of every clip (one wave gathering all words instead was slower:
        // 16.6 against 14.2 us per step-layer at T = 2048, N = 1)
        bool ok = true;
        for (int n = 0; n < N && ok; ++n) {
            const unsigned long long t0 = wall_clock64();
            for (;;) {
                const unsigned long long x = __hip_atomic_load(gb + n * LSTM_HID + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if ((unsigned)(x >> 32) == tag) {
                    hs[n * LSTM_HID + tid] = __uint_as_float((unsigned)x);
                    break;
                }
                if (wall_clock64() - t0 > a.limit) {
                    ok = false;
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
        }
        if (__syncthreads_or(!ok)) {
            if (!ok) __hip_atomic_store(a.err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            return;
        }
    }
    if (cell) {
        a.c[cn * LSTM_HID + unit] = c;
        a.hT[cn * LSTM_HID + unit] = h;
    }
}

void lstm_pack_whh_host(const float* whh /*[1024][256]*/, float* dst /*[16][256][64]*/) {
    for (int g = 0; g < LSTM_WG; ++g)
        for (int k = 0; k < LSTM_HID; ++k)
            for (int r = 0; r < LSTM_ROWS; ++r)
                dst[((size_t)g * LSTM_HID + k) * LSTM_ROWS + r] = whh[(size_t)((r >> 4) * LSTM_HID + g * 16 + (r & 15)) * LSTM_HID + k];
}

hipError_t lstm_rec_launch(const LstmArgs& a, hipStream_t s) {
    if (a.N < 1 || a.N > LSTM_MAXN || a.S < 1) return hipErrorInvalidValue;
    const size_t lds = sizeof(float) * LSTM_LDS_FLOATS;
    static lds_once_mask configured{0};
    if (hipError_t e = ensure_dynamic_lds(lstm_rec_kernel, lds, &configured); e != hipSuccess) return e;
    hipLaunchKernelGGL(lstm_rec_kernel, dim3(LSTM_WG), dim3(256), lds, s, a);
    return hipGetLastError();
}

}  // namespace eamm
