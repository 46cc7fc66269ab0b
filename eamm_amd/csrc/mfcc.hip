// Waveform -> MFCC on the device: the reference's input front end (demo.py:314-318, python_speech_features.mfcc(speech, 16000,
// winstep=0.01) with the package's defaults) for one or more clips in one launch.
//
// Per 400-sample frame of the pre-emphasised, virtually zero-padded signal (step 160, rectangular window):
//     P[k]  = |DFT512(frame)[k]|^2 / 512, k = 0..256        the 512-point real DFT as a 256-point complex FFT of the packed
//                                                           sequence z[n] = y[2n] + i y[2n+1] plus the real-split post-pass
//     E     = sum_k P[k]                                    (0 -> DBL_EPSILON)
//     fb_j  = sum_i P[i] * tri_j(i), j = 0..25               integer bin edges MEL_EDGES (0 -> DBL_EPSILON)
//     c_n   = (1 + 11 sin(pi n / 22)) * DCT-II_ortho(log fb)[n], n = 1..12;  c_0 = log E
//
// Shape: one workgroup of 256 threads owns MFCC_FPB consecutive frames of one clip.  It stages the frames' span of
// 160 * (MFCC_FPB - 1) + 400 pre-emphasised samples in LDS (read once from global memory; the pad is virtual), packs each frame
// bit-reversed into LDS and runs the eight radix-2 stages for all its frames together (four butterflies per thread per stage),
// then the post-pass, the filter sums (one thread per frame and filter, bins in ascending order), the energy (32 lanes per
// frame, nine bins each in ascending order, then a fixed xor-shuffle tree), log and the 12 x 26 DCT (one thread per output).
//
// Determinism: every value of a frame is produced by the same instruction sequence whichever slot of its workgroup the frame
// occupies, and every reduction has a fixed order; this file is compiled with -ffp-contract=off (csrc/Makefile) so that the
// compiler cannot fuse a multiply-add in one unrolled iteration and not in another.  A frame's 13 values therefore depend on its
// own samples only: the same samples give bit-identical rows whatever the clip length, the clip count or the workgroup.
//
// Precision: everything after the float32 samples is float64 (pre-emphasis, FFT, twiddles from sincospi, power, sums, log, DCT);
// only the 13 results are rounded to float32.  A float32 version (same shape) was measured first: 6.7e-4 max abs against the
// float64 oracle on 82 s of 1 kHz brick-wall low-passed noise, over the 2e-4 tolerance.  In mel bands that hold only the frame's
// leakage, a tiny share of its energy, the FFT's absolute error (which scales with the whole frame) is a large part of the band's
// energy, and the log magnifies it.  float64 costs 31 -> 48 us per 82 s of audio on one MI355X.
#include "kernels.h"

namespace eamm {

namespace {

constexpr int MFCC_FRAME = 400, MFCC_STEP = 160, MFCC_NFILT = 26, MFCC_NCEP = 13, MFCC_BINS = 257;
constexpr int MFCC_FPB = 8;                                           // frames per workgroup
constexpr int MFCC_THREADS = 256;
constexpr int MFCC_SPAN = MFCC_STEP * (MFCC_FPB - 1) + MFCC_FRAME;   // 1520 samples staged per workgroup
constexpr double MFCC_EPS = 2.220446049250313e-16;                   // DBL_EPSILON, numpy.finfo(float).eps

// floor(513 * mel2hz(linspace(hz2mel(0), hz2mel(8000), 28)) / 16000): filter j rises over [e_j, e_j+1) and falls over
// [e_j+1, e_j+2); bin 256 lies under no filter
__constant__ int MEL_EDGES[MFCC_NFILT + 2] = {0,  2,  4,  7,  10, 13,  16,  20,  24,  29,  34,  40,  46,  53,
                                              60, 68, 77, 87, 97, 109, 122, 136, 152, 169, 188, 209, 231, 256};

__device__ __forceinline__ int bitrev8(int v) { return (int)(__builtin_bitreverse32((unsigned)v) >> 24); }

__device__ __forceinline__ double2 cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// x'[n] of the signal padded with `pad` zeros on each side
__device__ __forceinline__ double padded(const float* __restrict__ x, long long S, int pad, long long n) {
    const long long m = n - pad;
    return (m >= 0 && m < S) ? (double)x[m] : 0.0;
}

}  // namespace

__global__ __launch_bounds__(MFCC_THREADS) void mfcc_kernel(const float* __restrict__ pcm, long long S, long long clip_stride,
                                                             int pad, long long F, float* __restrict__ out) {
    __shared__ double s_y[MFCC_SPAN];                      // pre-emphasised samples of the workgroup's frames
    __shared__ double2 s_z[MFCC_FPB][256];                 // FFT work arrays
    __shared__ double s_p[MFCC_FPB][MFCC_BINS + 3];        // power spectra
    __shared__ double2 s_tw[256];                          // W512^k = exp(-2 pi i k / 512)
    __shared__ double s_dct[MFCC_NCEP - 1][MFCC_NFILT];    // lifter * ortho DCT-II, outputs 1..12
    __shared__ double s_logfb[MFCC_FPB][MFCC_NFILT];
    __shared__ double s_loge[MFCC_FPB];

    const int tid = threadIdx.x;
    const long long f0 = (long long)blockIdx.x * MFCC_FPB;
    const float* __restrict__ x = pcm + (long long)blockIdx.y * clip_stride;
    const long long L = S + 2LL * pad;

    {
        double sn, cs;
        sincospi(-(double)tid / 256.0, &sn, &cs);
        s_tw[tid] = make_double2(cs, sn);
    }
    for (int i = tid; i < (MFCC_NCEP - 1) * MFCC_NFILT; i += MFCC_THREADS) {
        const int n = i / MFCC_NFILT + 1, m = i % MFCC_NFILT;
        const double lift = 1.0 + 11.0 * sinpi((double)n / 22.0);
        s_dct[n - 1][m] = lift * sqrt(2.0 / MFCC_NFILT) * cospi((double)(n * (2 * m + 1)) / (2.0 * MFCC_NFILT));
    }
    // pre-emphasis y[n] = x'[n] - 0.97 x'[n-1] (y[0] = x'[0]) of the padded signal; samples at n >= L read as zero
    const long long base = f0 * MFCC_STEP;
    for (int i = tid; i < MFCC_SPAN; i += MFCC_THREADS) {
        const long long n = base + i;
        double v = 0.0;
        if (n < L) {
            v = padded(x, S, pad, n);
            if (n > 0) v = v - 0.97 * padded(x, S, pad, n - 1);
        }
        s_y[i] = v;
    }
    __syncthreads();

    // z[n] = y[2n] + i y[2n+1] (zero for 2n >= 400), stored in bit-reversed order for the decimation-in-time stages
    for (int i = tid; i < MFCC_FPB * 256; i += MFCC_THREADS) {
        const int fl = i >> 8, n = i & 255;
        const double* y = s_y + fl * MFCC_STEP;
        s_z[fl][bitrev8(n)] = 2 * n < MFCC_FRAME ? make_double2(y[2 * n], y[2 * n + 1]) : make_double2(0.0, 0.0);
    }
    __syncthreads();

#pragma unroll
    for (int st = 1; st <= 8; ++st) {
        const int half = 1 << (st - 1);
#pragma unroll
        for (int r = 0; r < MFCC_FPB * 128 / MFCC_THREADS; ++r) {
            const int item = tid + r * MFCC_THREADS, fl = item >> 7, b = item & 127;
            const int j = b & (half - 1), i0 = ((b >> (st - 1)) << st) + j, i1 = i0 + half;
            const double2 t = cmul(s_tw[j << (9 - st)], s_z[fl][i1]);
            const double2 a = s_z[fl][i0];
            s_z[fl][i0] = make_double2(a.x + t.x, a.y + t.y);
            s_z[fl][i1] = make_double2(a.x - t.x, a.y - t.y);
        }
        __syncthreads();
    }

    // real split: X[k] = (Z[k] + conj Z[256-k]) / 2 - (i / 2) W512^k (Z[k] - conj Z[256-k]),  P[k] = |X[k]|^2 / 512
    for (int i = tid; i < MFCC_FPB * MFCC_BINS; i += MFCC_THREADS) {
        const int fl = i / MFCC_BINS, k = i % MFCC_BINS;
        const double2 a = s_z[fl][k & 255], c = s_z[fl][(256 - k) & 255];
        const double2 e = make_double2(0.5 * (a.x + c.x), 0.5 * (a.y - c.y));     // (Z[k] + conj Z[256-k]) / 2
        const double2 d = make_double2(0.5 * (a.x - c.x), 0.5 * (a.y + c.y));     // (Z[k] - conj Z[256-k]) / 2
        const double2 w = k < 256 ? s_tw[k] : make_double2(-1.0, 0.0);
        const double2 wd = cmul(w, d);
        const double xr = e.x + wd.y, xi = e.y - wd.x;                             // e - i * wd
        s_p[fl][k] = (xr * xr + xi * xi) * (1.0 / 512.0);
    }
    __syncthreads();

    // filter sums (one thread per frame and filter) and the frame energy (32 lanes per frame)
    if (tid < MFCC_FPB * MFCC_NFILT) {
        const int fl = tid / MFCC_NFILT, j = tid % MFCC_NFILT;
        const int lo = MEL_EDGES[j], mid = MEL_EDGES[j + 1], hi = MEL_EDGES[j + 2];
        const double* p = s_p[fl];
        double acc = 0.0;
        for (int b = lo; b < mid; ++b) acc = acc + p[b] * ((double)(b - lo) / (double)(mid - lo));
        for (int b = mid; b < hi; ++b) acc = acc + p[b] * ((double)(hi - b) / (double)(hi - mid));
        s_logfb[fl][j] = log(acc == 0.0 ? MFCC_EPS : acc);
    }
    {
        const int fl = tid >> 5, lane = tid & 31;
        double acc = 0.0;
        for (int k = lane; k < MFCC_BINS; k += 32) acc = acc + s_p[fl][k];
#pragma unroll
        for (int off = 16; off > 0; off >>= 1) acc = acc + __shfl_xor(acc, off, 32);
        if (lane == 0) s_loge[fl] = log(acc == 0.0 ? MFCC_EPS : acc);
    }
    __syncthreads();

    if (tid < MFCC_FPB * MFCC_NCEP) {
        const int fl = tid / MFCC_NCEP, n = tid % MFCC_NCEP;
        const long long f = f0 + fl;
        if (f < F) {
            double v = s_loge[fl];
            if (n > 0) {
                v = 0.0;
                for (int m = 0; m < MFCC_NFILT; ++m) v = v + s_dct[n - 1][m] * s_logfb[fl][m];
            }
            out[((long long)blockIdx.y * F + f) * MFCC_NCEP + n] = (float)v;
        }
    }
}

long long mfcc_frames(long long n_samples, int pad) {
    if (n_samples < 1 || pad < 0) return 0;
    const long long L = n_samples + 2LL * pad;
    return L <= MFCC_FRAME ? 1 : 1 + (L - MFCC_FRAME + MFCC_STEP - 1) / MFCC_STEP;
}

hipError_t mfcc_launch(const float* pcm, long long n_samples, int n_clips, long long clip_stride, int pad, float* out,
                       hipStream_t stream) {
    const long long F = mfcc_frames(n_samples, pad);
    const long long blocks = (F + MFCC_FPB - 1) / MFCC_FPB;
    if (F < 1 || blocks > 0x7fffffffLL || n_clips < 1 || n_clips > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mfcc_kernel, dim3((unsigned)blocks, (unsigned)n_clips), dim3(MFCC_THREADS), 0, stream, pcm, n_samples,
                       clip_stride, pad, F, out);
    return hipGetLastError();
}

}  // namespace eamm
