// What the element-wise and gather kernels share (motion.hip, motion_backward.hip, warp.hip, kp_head.hip, equivariance.hip; the wave
// reduction also batchnorm.hip): the coordinate grid, the sparse motion T_k, the ONE grid_sample sampling position that forward and
// backward kernels both start from (zeros padding) and its reflection-padding form, the bilinear resize position, and the wave /
// workgroup reductions.  Device code only.
#pragma once
#include "kernels.h"

namespace eamm {

// x = 2*(j/(n-1)) - 1, as make_coordinate_grid builds it (reference modules/util.py:844-848).
__device__ __forceinline__ float grid_coord(int j, int n) { return 2.f * ((float)j / (float)(n - 1)) - 1.f; }

// T_k(z) = J_k (z - kp_d) + kp_s (reference modules/dense_motion.py:53-63); rec = kd.xy ks.xy J00 J01 J10 J11.
// (rx, ry) = z - kp_d, which the record gradients need.
__device__ __forceinline__ void sparse_motion(const float* __restrict__ rec, float gx, float gy, float& tx, float& ty, float& rx,
                                              float& ry) {
    rx = gx - rec[0];
    ry = gy - rec[1];
    tx = fmaf(rec[5], ry, rec[4] * rx) + rec[2];
    ty = fmaf(rec[7], ry, rec[6] * rx) + rec[3];
}
__device__ __forceinline__ void sparse_motion(const float* __restrict__ rec, float gx, float gy, float& tx, float& ty) {
    float rx, ry;
    sparse_motion(rec, gx, gy, tx, ty, rx, ry);
}

// F.grid_sample(mode='bilinear', padding_mode='zeros', align_corners=False): where the sample (gx, gy) lies in a W x H map --
// the north-west corner, the fractions towards the +1 corners, and whether any corner can be inside the map.  The backward
// kernels differentiate exactly this position; the forward kernels take their corner weights from it (bilinear_setup).
struct SamplePos {
    int x0, y0;
    float ax, ay;   // weight of the +1 corner
    bool valid;
};
__device__ __forceinline__ SamplePos sample_pos(float gx, float gy, int W, int H) {
    const float ix = ((gx + 1.f) * (float)W - 1.f) * 0.5f;
    const float iy = ((gy + 1.f) * (float)H - 1.f) * 0.5f;
    const float fx = floorf(ix), fy = floorf(iy);
    SamplePos p;
    // clamp before the int conversion so that wild coordinates stay out of range instead of wrapping
    p.x0 = (int)fminf(fmaxf(fx, -2.f), (float)W);
    p.y0 = (int)fminf(fmaxf(fy, -2.f), (float)H);
    p.ax = ix - fx;
    p.ay = iy - fy;
    p.valid = ix > -2.f && ix < (float)W + 1.f && iy > -2.f && iy < (float)H + 1.f;   // false for NaN too
    return p;
}

// F.grid_sample(mode='bilinear', padding_mode='reflection', align_corners=False): the same un-normalised position, reflected about
// -0.5 and size - 0.5 as often as it takes (the distance from -0.5 modulo the size, counted back on an odd number of flips), then
// clipped to [0, size - 1].  Always valid: x0 / y0 lie inside the map, and only a +1 corner can lie outside -- it weighs nothing
// (the caller skips it).  A position that is not finite lands on pixel 0.
__device__ __forceinline__ float reflect_clip(float i, int size) {
    const float span = (float)size;
    const float a = fabsf(i + 0.5f);
    const float extra = fmodf(a, span);
    const int flips = (int)fminf(floorf(a / span), 1073741824.f);
    const float r = (flips & 1) ? span - extra - 0.5f : extra - 0.5f;
    return fminf((float)(size - 1), fmaxf(r, 0.f));
}
__device__ __forceinline__ SamplePos sample_pos_reflect(float gx, float gy, int W, int H) {
    const float ix = reflect_clip(((gx + 1.f) * (float)W - 1.f) * 0.5f, W);
    const float iy = reflect_clip(((gy + 1.f) * (float)H - 1.f) * 0.5f, H);
    const float fx = floorf(ix), fy = floorf(iy);
    SamplePos p;
    p.x0 = (int)fx;
    p.y0 = (int)fy;
    p.ax = ix - fx;
    p.ay = iy - fy;
    p.valid = true;
    return p;
}

// the forward's form: the four corner weights; an invalid position has weights 0 and corner -2 (every tap out of range)
struct Bilinear {
    int x0, y0;
    float wnw, wne, wsw, wse;
};
__device__ __forceinline__ Bilinear bilinear_setup(float gx, float gy, int W, int H) {
    const SamplePos p = sample_pos(gx, gy, W, H);
    Bilinear b;
    b.x0 = p.x0;
    b.y0 = p.y0;
    b.wnw = (1.f - p.ax) * (1.f - p.ay);
    b.wne = p.ax * (1.f - p.ay);
    b.wsw = (1.f - p.ax) * p.ay;
    b.wse = p.ax * p.ay;
    if (!p.valid) {
        b.wnw = b.wne = b.wsw = b.wse = 0.f;
        b.x0 = b.y0 = -2;
    }
    return b;
}

// F.interpolate(mode='bilinear', align_corners=False) source position (reference generator.py:55,83).
struct Lerp {
    int i0, i1;
    float l1;
};
__device__ __forceinline__ Lerp lerp_setup(int dst, int in, int out) {
    const float scale = (float)in / (float)out;
    float s = scale * ((float)dst + 0.5f) - 0.5f;
    s = fmaxf(s, 0.f);
    Lerp l;
    l.i0 = (int)s;
    l.i1 = l.i0 + (l.i0 < in - 1 ? 1 : 0);
    l.l1 = s - (float)l.i0;
    return l;
}

// ---- reductions over a wave and over a workgroup of BLOCK_WAVES waves (256 threads), fixed trees: deterministic ----
struct SumOp {
    template <class T> __device__ static T apply(T a, T b) { return a + b; }
};
struct MaxOp {
    __device__ static float apply(float a, float b) { return fmaxf(a, b); }
};

// Who holds the result.  All: the butterfly, every lane / thread.  First: the halving tree, lane 0 / thread 0 only (the same
// bits there as the butterfly's).
enum class Lanes { All, First };

template <class Op, Lanes L = Lanes::All, class T>
__device__ __forceinline__ T wave_reduce(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = Op::apply(v, L == Lanes::All ? __shfl_xor(v, o, 64) : __shfl_down(v, o, 64));
    return v;
}

constexpr int BLOCK_WAVES = 4;

// the waves' values red[0], red[stride], ... folded in wave order, starting from wave 0's
template <class Op, class T>
__device__ __forceinline__ T fold_waves(const T* red, int stride = 1) {
    T r = red[0];
#pragma unroll
    for (int i = 1; i < BLOCK_WAVES; ++i) r = Op::apply(r, red[i * stride]);
    return r;
}

// red: BLOCK_WAVES values of LDS.  All: every thread folds the waves' values starting from wave 0's.  First (sums only): thread 0
// folds them starting from zero -- the two differ in the sign of a sum of negative zeros -- and the other threads get zero.
template <class Op, Lanes L = Lanes::All, class T>
__device__ __forceinline__ T block_reduce(T v, T* red) {
    v = wave_reduce<Op, L>(v);
    __syncthreads();                  // `red` may still be read from the previous call
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if constexpr (L == Lanes::All) return fold_waves<Op>(red);
    T s = T(0);
    if (threadIdx.x == 0)
        for (int i = 0; i < BLOCK_WAVES; ++i) s = Op::apply(s, red[i]);
    return s;
}

}  // namespace eamm
