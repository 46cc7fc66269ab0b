// The emotion video's preprocessing on the device: the reference demo's three image steps per driving frame (demo.py:490
// resize, demo.py:146-182 get_aligned_image, demo.py:184-190 -> augmentation.py:403-431 the test-time augmentation) and the
// portrait crop (demo.py:433-454).  Frames are HWC, coordinates (x = column, y = row).
//
//   resize_aa_kernel        S0: uint8 [N,H,W,C] -> uint8 [N,256,256,3] = trunc(255 * zoom(gaussian(x / 255)))
//                               (skimage.transform.resize with anti-aliasing = ndi.gaussian_filter(mode='mirror') followed by
//                               ndi.zoom(order=1, mode='mirror', grid_mode=True)); separable blur, rows then columns, taps from the
//                               host; then linear interpolation at in = (o + 0.5) * in / 256 - 0.5 with mirrored neighbours
//   similarity_warp_kernel  S1: uint8 [N,H,W,C] -> 256 x 256, output (x, y) samples the frame at M (x, y, 1) (skimage warp,
//                               order 1, zero outside); float32 NHWC [N,256,256,3], or trunc(255 v) / 255 as float32 NCHW [N,3,256,256]
//   emotion_augment_kernel  S2..S6 fused: mouth noise, horizontal flip, rotation (skimage rotate), perspective (cv2.warpPerspective
//                               with BORDER_REPLICATE, 1/32-pixel fixed-point coordinates), quantisation to k / 255
//
// The augmentation is gather-through: an output pixel computes S5's four neighbours, each of them S4's bilinear sample of the
// flipped, noised, aligned frame, read from global memory (the aligned frame, 786 KB, stays in L2).  Every intermediate value is
// produced by one function of its own coordinates (s4_rgb, s0_blurred), so it is the same wherever it is needed: an output
// frame depends only on its source frame and the clip's parameters, never on the launch it is part of.
//
// Precision: float64 from the uint8 / float32 inputs on.  The file is compiled with -ffp-contract=off (csrc/Makefile), so the
// device performs exactly the float64 operations, in the same order, as eamm_amd/video_input.py's numpy oracle.
#include "kernels.h"

#include <climits>

namespace eamm {

namespace {

constexpr int VP_OUT = 256;          // every output of this file is 256 x 256
constexpr int VP_THREADS = 256;      // one output row per workgroup

// ndimage 'mirror': d c b | a b c d | c b a
__device__ __forceinline__ int mirror_index(int i, int n) {
    if (n == 1) return 0;
    const int period = 2 * n - 2;
    i %= period;
    if (i < 0) i += period;
    return i >= n ? period - i : i;
}

// S0's blurred image at (y, x) of one frame: sum over the column taps of (sum over the row taps), taps in ascending order
__device__ __forceinline__ double s0_blurred(const unsigned char* __restrict__ frame, int H, int W, int C, int y, int x, int ch,
                                             const VideoResizeTaps& t) {
    double acc = 0.0;
    for (int j = -t.rx; j <= t.rx; ++j) {
        const int xx = mirror_index(x + j, W);
        double col = 0.0;
        for (int i = -t.ry; i <= t.ry; ++i) {
            const int yy = mirror_index(y + i, H);
            col = col + t.wy[i + t.ry] * ((double)frame[((long long)yy * W + xx) * C + ch] / 255.0);
        }
        acc = acc + t.wx[j + t.rx] * col;
    }
    return acc;
}

// the splitmix64 finaliser
__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the device mouth noise (include/eamm_hip.h, eamm_op_emotion_augment): uniform on [0, 1) in steps of 2^-24
__device__ __forceinline__ float noise_hash(unsigned long long seed, long long frame, int idx, int ch, int mouth_px) {
    constexpr unsigned long long GOLDEN = 0x9E3779B97F4A7C15ull;
    const unsigned long long key = mix64(seed + GOLDEN);
    const unsigned long long ctr = ((unsigned long long)frame * (unsigned long long)mouth_px + (unsigned long long)idx) * 3ull +
                                   (unsigned long long)ch + 1ull;
    return (float)(mix64(key + ctr * GOLDEN) >> 40) * (1.0f / 16777216.0f);
}

// skimage's bilinear_interpolation (order 1, mode 'constant', cval 0): neighbours floor / ceil, each one outside reads 0
template <class Fetch>
__device__ __forceinline__ void bilinear3(double r, double c, int H, int W, Fetch fetch, double out[3]) {
    const double fr = floor(r), fc = floor(c);
    const double cr = ceil(r), cc = ceil(c);
    const double dr = r - fr, dc = c - fc;
    double tl[3] = {0.0, 0.0, 0.0}, tr[3] = {0.0, 0.0, 0.0}, bl[3] = {0.0, 0.0, 0.0}, br[3] = {0.0, 0.0, 0.0};
    const bool r0 = fr >= 0.0 && fr < (double)H, r1 = cr >= 0.0 && cr < (double)H;
    const bool c0 = fc >= 0.0 && fc < (double)W, c1 = cc >= 0.0 && cc < (double)W;
    if (r0 && c0) fetch((int)fr, (int)fc, tl);
    if (r0 && c1) fetch((int)fr, (int)cc, tr);
    if (r1 && c0) fetch((int)cr, (int)fc, bl);
    if (r1 && c1) fetch((int)cr, (int)cc, br);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double top = (1.0 - dc) * tl[k] + dc * tr[k];
        const double bottom = (1.0 - dc) * bl[k] + dc * br[k];
        out[k] = (1.0 - dr) * top + dr * bottom;
    }
}

struct AugFrame {
    const float* __restrict__ aligned;   // the source frame [256][256][3]
    const float* __restrict__ noise;     // its explicit mouth noise [mh][mw][3], or null: the device hash
    long long src;
};

// S2 + S3: the flipped, noised aligned frame at (row, col)
__device__ __forceinline__ void s3_rgb(const AugFrame& f, const VideoAugParams& p, int row, int col, double v[3]) {
    const int q = p.flip ? VP_OUT - 1 - col : col;
    const int my = row - p.mouth_y, mx = q - p.mouth_x;
    if (my >= 0 && my < p.mouth_h && mx >= 0 && mx < p.mouth_w) {
        const int idx = my * p.mouth_w + mx;
        for (int k = 0; k < 3; ++k)
            v[k] = f.noise ? (double)f.noise[(long long)idx * 3 + k] : (double)noise_hash(p.noise_seed, f.src, idx, k, p.mouth_h * p.mouth_w);
    } else {
        const float* px = f.aligned + ((long long)row * VP_OUT + q) * 3;
        v[0] = (double)px[0];
        v[1] = (double)px[1];
        v[2] = (double)px[2];
    }
}

// S4: the rotated image at the integer pixel (x, y): input (x', y') = R (x, y, 1)
__device__ __forceinline__ void s4_rgb(const AugFrame& f, const VideoAugParams& p, int x, int y, double v[3]) {
    const double c = p.rot[0] * (double)x + p.rot[1] * (double)y + p.rot[2];
    const double r = p.rot[3] * (double)x + p.rot[4] * (double)y + p.rot[5];
    bilinear3(r, c, VP_OUT, VP_OUT, [&](int rr, int cc, double* o) { s3_rgb(f, p, rr, cc, o); }, v);
}

// OpenCV's cvRound of a clamped double, then the 1/32 split
__device__ __forceinline__ int fixed32(double v) {
    v = fmax((double)INT_MIN, fmin((double)INT_MAX, v));
    return (int)rint(v);
}

}  // namespace

__global__ __launch_bounds__(VP_THREADS) void resize_aa_kernel(const unsigned char* __restrict__ in, int H, int W, int C,
                                                               VideoResizeTaps taps, unsigned char* __restrict__ out) {
    const int ox = threadIdx.x, oy = blockIdx.x;
    const long long n = blockIdx.y;
    const unsigned char* frame = in + n * H * (long long)W * C;
    const double sy = (double)H / (double)VP_OUT, sx = (double)W / (double)VP_OUT;
    const double cy = ((double)oy + 0.5) * sy - 0.5, cx = ((double)ox + 0.5) * sx - 0.5;
    const double fy0 = floor(cy), fx0 = floor(cx);
    const double fy = cy - fy0, fx = cx - fx0;
    const int y0 = mirror_index((int)fy0, H), y1 = mirror_index((int)fy0 + 1, H);
    const int x0 = mirror_index((int)fx0, W), x1 = mirror_index((int)fx0 + 1, W);
    unsigned char* o = out + ((n * VP_OUT + oy) * VP_OUT + ox) * 3;
    for (int ch = 0; ch < 3; ++ch) {
        const double b00 = s0_blurred(frame, H, W, C, y0, x0, ch, taps), b01 = s0_blurred(frame, H, W, C, y0, x1, ch, taps);
        const double b10 = s0_blurred(frame, H, W, C, y1, x0, ch, taps), b11 = s0_blurred(frame, H, W, C, y1, x1, ch, taps);
        const double top = (1.0 - fx) * b00 + fx * b01;
        const double bottom = (1.0 - fx) * b10 + fx * b11;
        const double v = ((1.0 - fy) * top + fy * bottom) * 255.0;
        o[ch] = (unsigned char)fmin(255.0, fmax(0.0, trunc(v)));     // uint8(v * 255): truncation (demo.py:162)
    }
}

__global__ __launch_bounds__(VP_THREADS) void similarity_warp_kernel(const unsigned char* __restrict__ in, int H, int W, int C,
                                                                     const double* __restrict__ maps, int mode, void* __restrict__ out) {
    const int x = threadIdx.x, y = blockIdx.x;
    const long long n = blockIdx.y;
    const unsigned char* frame = in + n * H * (long long)W * C;
    const double* m = maps + n * 6;
    const double c = m[0] * (double)x + m[1] * (double)y + m[2];
    const double r = m[3] * (double)x + m[4] * (double)y + m[5];
    double v[3];
    bilinear3(r, c, H, W, [&](int rr, int cc, double* o) {
        const unsigned char* px = frame + ((long long)rr * W + cc) * C;
        o[0] = (double)px[0] / 255.0;
        o[1] = (double)px[1] / 255.0;
        o[2] = (double)px[2] / 255.0;
    }, v);
    if (mode == 0) {
        float* o = static_cast<float*>(out) + ((n * VP_OUT + y) * VP_OUT + x) * 3;
        o[0] = (float)v[0];
        o[1] = (float)v[1];
        o[2] = (float)v[2];
    } else {
        float* o = static_cast<float*>(out) + n * 3 * VP_OUT * VP_OUT + (long long)y * VP_OUT + x;
        for (int k = 0; k < 3; ++k) o[(long long)k * VP_OUT * VP_OUT] = (float)(fmin(255.0, fmax(0.0, trunc(v[k] * 255.0))) / 255.0);
    }
}

__global__ __launch_bounds__(VP_THREADS) void emotion_augment_kernel(const float* __restrict__ aligned, long long n_src, long long t0,
                                                                     const double* __restrict__ hinv, const float* __restrict__ noise,
                                                                     VideoAugParams p, float* __restrict__ out) {
    const int x = threadIdx.x, y = blockIdx.x;
    const long long t = blockIdx.y;                          // output frame t0 + t
    const long long src = (t0 + t) % n_src;
    AugFrame f;
    f.aligned = aligned + src * VP_OUT * VP_OUT * 3;
    f.noise = noise ? noise + src * (long long)p.mouth_h * p.mouth_w * 3 : nullptr;
    f.src = src;
    // S5: M^-1 (x, y, 1) in 1/32 pixels (OpenCV's WarpPerspectiveInvoker: W = 32 / W, X = cvRound(X0 * W))
    const double* h = hinv + src * 9;
    const double X0 = h[0] * (double)x + h[1] * (double)y + h[2];
    const double Y0 = h[3] * (double)x + h[4] * (double)y + h[5];
    double Wd = h[6] * (double)x + h[7] * (double)y + h[8];
    Wd = Wd != 0.0 ? 32.0 / Wd : 0.0;
    const int X = fixed32(X0 * Wd), Y = fixed32(Y0 * Wd);
    const int sx = X >> 5, sy = Y >> 5, ax = X & 31, ay = Y & 31;
    // BORDER_REPLICATE: each neighbour index clamped on its own
    const int xs0 = min(max(sx, 0), VP_OUT - 1), xs1 = min(max(sx + 1, 0), VP_OUT - 1);
    const int ys0 = min(max(sy, 0), VP_OUT - 1), ys1 = min(max(sy + 1, 0), VP_OUT - 1);
    const double w0 = (double)((32 - ax) * (32 - ay)) / 1024.0, w1 = (double)(ax * (32 - ay)) / 1024.0;
    const double w2 = (double)((32 - ax) * ay) / 1024.0, w3 = (double)(ax * ay) / 1024.0;
    double v0[3], v1[3], v2[3], v3[3];
    s4_rgb(f, p, xs0, ys0, v0);
    s4_rgb(f, p, xs1, ys0, v1);
    s4_rgb(f, p, xs0, ys1, v2);
    s4_rgb(f, p, xs1, ys1, v3);
    float* o = out + t * 3 * VP_OUT * VP_OUT + (long long)y * VP_OUT + x;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double v = v0[k] * w0 + v1[k] * w1 + v2[k] * w2 + v3[k] * w3;
        // S6: img_as_ubyte (rint(255 v) clipped) then back to k / 255, float32
        const double q = fmin(255.0, fmax(0.0, rint(v * 255.0)));
        o[(long long)k * VP_OUT * VP_OUT] = (float)(q / 255.0);
    }
}

hipError_t resize_aa_launch(const unsigned char* in, int n, int H, int W, int C, const VideoResizeTaps& taps, unsigned char* out,
                            hipStream_t stream) {
    if (n < 1 || n > 65535 || H < 1 || W < 1 || (C != 3 && C != 4) || taps.ry < 0 || taps.rx < 0 || taps.ry >= VIDEO_MAX_RADIUS ||
        taps.rx >= VIDEO_MAX_RADIUS)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(resize_aa_kernel, dim3(VP_OUT, (unsigned)n), dim3(VP_THREADS), 0, stream, in, H, W, C, taps, out);
    return hipGetLastError();
}

hipError_t similarity_warp_launch(const unsigned char* in, int n, int H, int W, int C, const double* maps, int mode, void* out,
                                  hipStream_t stream) {
    if (n < 1 || n > 65535 || H < 1 || W < 1 || (C != 3 && C != 4) || (mode != 0 && mode != 1)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(similarity_warp_kernel, dim3(VP_OUT, (unsigned)n), dim3(VP_THREADS), 0, stream, in, H, W, C, maps, mode, out);
    return hipGetLastError();
}

hipError_t emotion_augment_launch(const float* aligned, long long n_src, long long t0, int count, const double* hinv, const float* noise,
                                  const VideoAugParams& p, float* out, hipStream_t stream) {
    if (n_src < 1 || t0 < 0 || count < 1 || count > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(emotion_augment_kernel, dim3(VP_OUT, (unsigned)count), dim3(VP_THREADS), 0, stream, aligned, n_src, t0, hinv,
                       noise, p, out);
    return hipGetLastError();
}

}  // namespace eamm
