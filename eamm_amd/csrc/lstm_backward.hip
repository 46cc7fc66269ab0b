// Backward of one LSTM layer of AT_net2 (reference modules/util.py:551, :596-598; train.py's first stage back-propagates an L1
// loss on the audio-driven key points through it), and the small kernels the operator-level forward needs around lstm_rec_kernel
// (audio.hip), which itself is unchanged:
//   lstm_pack_whh_dev   W_hh [1024][256] on the device -> lstm_rec_kernel's image [16][256][64] (lstm_pack_whh_host's layout)
//   lstm_scan           gate pre-activations [N,T,1024] (xproj + h_{t-1} W_hh^T, recomputed from the saved y) -> the activated
//                       gates in place and c_t [N,T,256]: an element-wise scan over T, one thread per (clip, unit)
//   lstm_bwd            the backward recurrence over T steps, one persistent launch
//
// lstm_bwd mirrors the forward's partition: LSTM_WG = 16 workgroups of 256 threads, workgroup g owns hidden units 16g .. 16g+15
// and keeps the 1024 x 16 slice W_hh[:, 16g .. 16g+15] (64 KB) in LDS for the whole launch.  Stepping t = T-1 .. 0 it forms
//     dh_t[unit] = dy_t[unit] + sum_row dgates_{t+1}[row] W_hh[row, unit]
// for its own units from ALL N x 1024 gate gradients of step t+1, carries dc locally, computes its own N x 64 dgates_t, writes
// them to the [N,T,1024] output (= the gradient of the input projection) and publishes them to the other workgroups.  The
// hand-off is the forward's: 8-byte {tag, value} words stored and polled with agent-scope relaxed atomics
// (cdna_hip_programming.md section 6 Guideline 16), double-buffered by step parity -- a workgroup can overwrite the words of step
// t+2 only after it has gathered step t+1 from every workgroup, which each published after reading step t+2 -- no flag and no
// fence.  The operator zeroes the granule buffer on the stream before every launch and tags start at 1, so stale words never
// match.  Every wait is bounded by the forward's wall-clock limit; on expiry the workgroup sets the host-visible error word and
// fills the rest of its output rows with NaN, so that a timed-out step cannot pass for a result.
// LDS: 16 x (64 x 16 + 16) + 8 x 1024 + 16 x 8 x 16 floats = 105 KB: one workgroup per CU, 16 of the chip's 256 CUs.
#include "conv_common.h"

namespace eamm {

namespace {
constexpr int LB_HID = 256, LB_GATES = 1024, LB_MAXN = 8;
constexpr int LB_SLICE = 64 * 16 + 16;   // 64 rows x 16 units of W, + 16 floats: the four row slices of a wave hit 64 different banks
constexpr size_t LB_LDS_FLOATS = (size_t)16 * LB_SLICE + LB_MAXN * LB_GATES + 16 * LB_MAXN * 16;

__device__ __forceinline__ float lb_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }
}  // namespace

__global__ __launch_bounds__(256) void lstm_pack_whh_kernel(const float* __restrict__ whh, float* __restrict__ dst) {
    const int i = blockIdx.x * 256 + threadIdx.x;   // ((g * 256 + k) * 64 + r)
    if (i >= LSTM_WG * LB_HID * 64) return;
    const int r = i & 63, k = (i >> 6) & 255, g = i >> 14;
    dst[i] = whh[(size_t)((r >> 4) * LB_HID + g * 16 + (r & 15)) * LB_HID + k];
}

__global__ __launch_bounds__(256) void lstm_scan_kernel(float* __restrict__ gates, int N, int T, float* __restrict__ c) {
    const int i = blockIdx.x * 256 + threadIdx.x;   // (clip, unit)
    if (i >= N * LB_HID) return;
    const int n = i >> 8, unit = i & 255;
    float cv = 0.f;
    for (int t = 0; t < T; ++t) {
        float* gp = gates + ((size_t)n * T + t) * LB_GATES + unit;
        const float ig = lb_sigmoid(gp[0]), fg = lb_sigmoid(gp[LB_HID]), gg = tanhf(gp[2 * LB_HID]), og = lb_sigmoid(gp[3 * LB_HID]);
        cv = fg * cv + ig * gg;
        gp[0] = ig;
        gp[LB_HID] = fg;
        gp[2 * LB_HID] = gg;
        gp[3 * LB_HID] = og;
        c[((size_t)n * T + t) * LB_HID + unit] = cv;
    }
}

__global__ __launch_bounds__(256) void lstm_bwd_kernel(const LstmBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* Ws = sm;                                // 16 slices of [64 rows][16 units] (+ 16 floats of padding each)
    float* dg = Ws + 16 * LB_SLICE;                // [N][1024] gate gradients of the step after this one
    float* red = dg + LB_MAXN * LB_GATES;          // [16 row slices][N][16 units] partial sums
    const int g = blockIdx.x, tid = threadIdx.x, N = a.N, T = a.T;
    for (int i = tid; i < LB_GATES * 16; i += 256) {
        const int row = i >> 4, u = i & 15;
        Ws[(row >> 6) * LB_SLICE + (row & 63) * 16 + u] = a.whh[(size_t)row * LB_HID + g * 16 + u];
    }
    __syncthreads();
    // the dot products: thread -> (row slice q, unit u); the cell update: thread -> (clip cn, unit cj), the same split of tid
    const int q = tid >> 4, u = tid & 15, cn = q, cj = u, unit = g * 16 + cj;
    const bool cell = tid < N * 16;
    float dc = 0.f;
    const float nanv = __uint_as_float(0x7FC00000u);
    for (int s = 0; s < T; ++s) {
        const int t = T - 1 - s;
        // this step's saved values, loaded before the wait hides their latency
        float ig = 0.f, fg = 0.f, gg = 0.f, og = 0.f, ct = 0.f, cp = 0.f, dh = 0.f;
        const size_t row = (size_t)cn * T + t;
        if (cell) {
            const float* ap = a.acts + row * LB_GATES + unit;
            ig = ap[0];
            fg = ap[LB_HID];
            gg = ap[2 * LB_HID];
            og = ap[3 * LB_HID];
            ct = a.c[row * LB_HID + unit];
            cp = t > 0 ? a.c[(row - 1) * LB_HID + unit] : 0.f;
            dh = a.dy[row * LB_HID + unit];
        }
        if (s > 0) {
            // dgates of step t + 1 of every workgroup -> LDS: thread tid polls rows tid, tid + 256, .. of every clip
            const unsigned tag = (unsigned)s;   // iteration s - 1 published with tag 1 + (s - 1)
            const unsigned long long* gb = a.gran + (size_t)((s - 1) & 1) * LB_MAXN * LB_GATES;
            bool ok = true;
            for (int i = tid; i < N * LB_GATES && ok; i += 256) {
                const unsigned long long t0 = wall_clock64();
                for (;;) {
                    const unsigned long long x = __hip_atomic_load(gb + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if ((unsigned)(x >> 32) == tag) {
                        dg[i] = __uint_as_float((unsigned)x);
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
                if (cell)
                    for (int tt = t; tt >= 0; --tt)
                        for (int k = 0; k < 4; ++k) a.dx[((size_t)cn * T + tt) * LB_GATES + k * LB_HID + unit] = nanv;
                return;
            }
            float acc[LB_MAXN];
            static_for<LB_MAXN>([&](auto nc) { acc[decltype(nc)::value] = 0.f; });
            const float* wp = Ws + q * LB_SLICE + u;
            const float* dp = dg + q * 64;
            for (int k = 0; k < 64; ++k) {
                const float w = wp[k * 16];
                static_for<LB_MAXN>([&](auto nc) {
                    constexpr int n = decltype(nc)::value;
                    if (n < N) acc[n] = fmaf(w, dp[n * LB_GATES + k], acc[n]);
                });
            }
            static_for<LB_MAXN>([&](auto nc) {
                constexpr int n = decltype(nc)::value;
                if (n < N) red[(q * LB_MAXN + n) * 16 + u] = acc[n];
            });
            __syncthreads();
            if (cell) {
                float v = 0.f;
                for (int k = 0; k < 16; ++k) v += red[(k * LB_MAXN + cn) * 16 + cj];
                dh += v;
            }
        }
        if (cell) {
            const float tc = tanhf(ct);
            const float d_o = dh * tc;
            dc += dh * og * (1.f - tc * tc);
            float d[4];
            d[0] = dc * gg * ig * (1.f - ig);        // i
            d[1] = dc * cp * fg * (1.f - fg);        // f
            d[2] = dc * ig * (1.f - gg * gg);        // g
            d[3] = d_o * og * (1.f - og);            // o
            dc *= fg;
            unsigned long long* gb = a.gran + (size_t)(s & 1) * LB_MAXN * LB_GATES + cn * LB_GATES + unit;
            const unsigned long long tag = (unsigned long long)(unsigned)(s + 1) << 32;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                a.dx[row * LB_GATES + k * LB_HID + unit] = d[k];
                if (s + 1 < T) __hip_atomic_store(gb + k * LB_HID, tag | __float_as_uint(d[k]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        // the next step's poll writes dg and its partial sums write red: every read of this step is behind a barrier by then
        // (the barrier after `red` for dg; the next step's __syncthreads_or for red)
    }
}

hipError_t lstm_pack_whh_dev_launch(const float* whh, float* dst, hipStream_t s) {
    hipLaunchKernelGGL(lstm_pack_whh_kernel, dim3(LSTM_WG * LB_HID * 64 / 256), dim3(256), 0, s, whh, dst);
    return hipGetLastError();
}

hipError_t lstm_scan_launch(float* gates, int N, int T, float* c, hipStream_t s) {
    if (N < 1 || N > LB_MAXN || T < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lstm_scan_kernel, dim3(N), dim3(256), 0, s, gates, N, T, c);
    return hipGetLastError();
}

hipError_t lstm_bwd_launch(const LstmBwdArgs& a, hipStream_t s) {
    if (a.N < 1 || a.N > LB_MAXN || a.T < 1) return hipErrorInvalidValue;
    const size_t lds = sizeof(float) * LB_LDS_FLOATS;
    static lds_once_mask configured{0};
    if (hipError_t e = ensure_dynamic_lds(lstm_bwd_kernel, lds, &configured); e != hipSuccess) return e;
    hipLaunchKernelGGL(lstm_bwd_kernel, dim3(LSTM_WG), dim3(256), lds, s, a);
    return hipGetLastError();
}

}  // namespace eamm
