// The warps by the dense-motion flow, forward next to backward (reference modules/generator.py:50-57, 79-86):
//   * warp_features_kernel           out = grid_sample(feat, flow, bilinear, zeros, align_corners=False) * occlusion, NHWC
//   * warp_image_kernel              the 'deformed' side output: the RGB source sampled by the flow resized to the frame
//   * warp_features_backward_kernel  the gradient of the first with respect to the features, the flow and the occlusion map: what
//     autograd derives from F.grid_sample and the multiply.  HBM-bound: dout read once, the four corner lines re-read, d_feat
//     accumulated with float atomics (as ATen's grid_sampler backward does; with one source for all frames the frames'
//     contributions land on the same map).
// Forward and backward start from the same sampling position (pointwise.h: sample_pos).
#include "pointwise.h"

#include <algorithm>

namespace eamm {

// flow / occlusion at feature-map pixel (y,x): direct read when the motion grid matches the feature
// map, else the reference's bilinear resize (generator.py:52-56, 82-83).
__device__ __forceinline__ void flow_at(const float2* __restrict__ defo, const float* __restrict__ occ, int h,
                                        int w, int H, int W, int y, int x, float& gx, float& gy, float& o) {
    if (h == H && w == W) {
        const float2 d = defo[y * w + x];
        gx = d.x;
        gy = d.y;
        o = occ ? occ[y * w + x] : 1.f;
        return;
    }
    const Lerp ly = lerp_setup(y, h, H), lx = lerp_setup(x, w, W);
    const float2 d00 = defo[ly.i0 * w + lx.i0], d01 = defo[ly.i0 * w + lx.i1];
    const float2 d10 = defo[ly.i1 * w + lx.i0], d11 = defo[ly.i1 * w + lx.i1];
    const float wy1 = ly.l1, wy0 = 1.f - wy1, wx1 = lx.l1, wx0 = 1.f - wx1;
    gx = wy0 * (wx0 * d00.x + wx1 * d01.x) + wy1 * (wx0 * d10.x + wx1 * d11.x);
    gy = wy0 * (wx0 * d00.y + wx1 * d01.y) + wy1 * (wx0 * d10.y + wx1 * d11.y);
    o = 1.f;
    if (occ) {
        o = wy0 * (wx0 * occ[ly.i0 * w + lx.i0] + wx1 * occ[ly.i0 * w + lx.i1]) +
            wy1 * (wx0 * occ[ly.i1 * w + lx.i0] + wx1 * occ[ly.i1 * w + lx.i1]);
    }
}

// ---------------------------------------------------------------------------------------------
// feature warp: out = grid_sample(feat, deformation) * occlusion  (generator.py:50-57, 79-84), NHWC,
// one thread per (pixel, 4 channels): a wave covers 256 contiguous channels of one pixel, so every
// corner gather is a 1 KiB coalesced read.  Also emits the first res-block's pre-activation
// relu(bn1(out)) (util.py:873-874) so that the bottleneck convolutions read ready operands.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void warp_features_kernel(const float* __restrict__ feat,
                                                            const float* __restrict__ deformation,
                                                            const float* __restrict__ occlusion, int n, int ns,
                                                            int hf, int wf, int C, int h, int w,
                                                            float* __restrict__ out, float* __restrict__ out2,
                                                            const float* __restrict__ s2,
                                                            const float* __restrict__ t2) {
    // one thread = one pixel x TWO 4-channel groups (c4 and c4 + c4n/2): the flow / bilinear setup is shared and
    // eight 16-byte gathers are in flight per thread; a wave still covers contiguous 1 KiB runs of each half
    const int c4n = C >> 2, half_n = c4n >> 1;
    const size_t total = (size_t)n * hf * wf * half_n;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (size_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(idx % half_n);
        const size_t pix = idx / half_n;
        const int x = (int)(pix % wf);
        const int y = (int)((pix / wf) % hf);
        const int f = (int)(pix / ((size_t)wf * hf));
        float gx, gy, o;
        flow_at(reinterpret_cast<const float2*>(deformation) + (size_t)f * h * w,
                occlusion ? occlusion + (size_t)f * h * w : nullptr, h, w, hf, wf, y, x, gx, gy, o);
        const Bilinear b = bilinear_setup(gx, gy, wf, hf);
        const float4* src = reinterpret_cast<const float4*>(feat + (size_t)((ns == 1) ? 0 : f) * hf * wf * C) + c4;
        const bool x0ok = (unsigned)b.x0 < (unsigned)wf, x1ok = (unsigned)(b.x0 + 1) < (unsigned)wf;
        const bool y0ok = (unsigned)b.y0 < (unsigned)hf, y1ok = (unsigned)(b.y0 + 1) < (unsigned)hf;
        const float wgt[4] = {b.wnw, b.wne, b.wsw, b.wse};
        const bool cok[4] = {y0ok && x0ok, y0ok && x1ok, y1ok && x0ok, y1ok && x1ok};
        // clamp the corner coordinates so every load is in range; the VALUE of an out-of-range corner is replaced by zero
        // (grid_sample's zeros padding; a zero weight would let a non-finite border value through as 0 * Inf = NaN)
        const int xa = min(max(b.x0, 0), wf - 1), xb = min(max(b.x0 + 1, 0), wf - 1);
        const int ya = min(max(b.y0, 0), hf - 1), yb = min(max(b.y0 + 1, 0), hf - 1);
        const size_t off[4] = {(size_t)(ya * wf + xa) * c4n, (size_t)(ya * wf + xb) * c4n, (size_t)(yb * wf + xa) * c4n,
                               (size_t)(yb * wf + xb) * c4n};
        float4 v[2][4];
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int k = 0; k < 4; ++k) v[g][k] = src[off[k] + g * half_n];
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (!cok[k]) v[g][k] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int k = 0; k < 4; ++k) {   // same accumulation order as before: nw, ne, sw, se
                acc.x = fmaf(v[g][k].x, wgt[k], acc.x); acc.y = fmaf(v[g][k].y, wgt[k], acc.y);
                acc.z = fmaf(v[g][k].z, wgt[k], acc.z); acc.w = fmaf(v[g][k].w, wgt[k], acc.w);
            }
            acc.x *= o; acc.y *= o; acc.z *= o; acc.w *= o;
            const size_t oidx = pix * c4n + c4 + g * half_n;
            reinterpret_cast<float4*>(out)[oidx] = acc;
            if (out2) {
                const float4 s = reinterpret_cast<const float4*>(s2)[c4 + g * half_n];
                const float4 t = reinterpret_cast<const float4*>(t2)[c4 + g * half_n];
                float4 a;
                a.x = fmaxf(fmaf(acc.x, s.x, t.x), 0.f); a.y = fmaxf(fmaf(acc.y, s.y, t.y), 0.f);
                a.z = fmaxf(fmaf(acc.z, s.z, t.z), 0.f); a.w = fmaxf(fmaf(acc.w, s.w, t.w), 0.f);
                reinterpret_cast<float4*>(out2)[oidx] = a;
            }
        }
    }
}

// 'deformed' side output: flow resized to the frame, grid_sample of the RGB source (generator.py:86).
__global__ __launch_bounds__(256) void warp_image_kernel(const float* __restrict__ src,
                                                         const float* __restrict__ deformation, int n, int ns, int H,
                                                         int W, int h, int w, float* __restrict__ out, int Cplanes,
                                                         int Cout) {
    const size_t total = (size_t)n * H * W;
    const size_t plane = (size_t)H * W;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(idx % W);
        const int y = (int)((idx / W) % H);
        const int f = (int)(idx / plane);
        float gx, gy, o;
        flow_at(reinterpret_cast<const float2*>(deformation) + (size_t)f * h * w, nullptr, h, w, H, W, y, x, gx, gy,
                o);
        const Bilinear b = bilinear_setup(gx, gy, W, H);
        const float* s = src + (size_t)((ns == 1) ? 0 : f) * Cplanes * plane;
        const bool x0ok = (unsigned)b.x0 < (unsigned)W, x1ok = (unsigned)(b.x0 + 1) < (unsigned)W;
        const bool y0ok = (unsigned)b.y0 < (unsigned)H, y1ok = (unsigned)(b.y0 + 1) < (unsigned)H;
        for (int c = 0; c < Cout; ++c) {
            const float* pc = s + c * plane;
            float v = 0.f;
            if (y0ok && x0ok) v = fmaf(pc[b.y0 * W + b.x0], b.wnw, v);
            if (y0ok && x1ok) v = fmaf(pc[b.y0 * W + b.x0 + 1], b.wne, v);
            if (y1ok && x0ok) v = fmaf(pc[(b.y0 + 1) * W + b.x0], b.wsw, v);
            if (y1ok && x1ok) v = fmaf(pc[(b.y0 + 1) * W + b.x0 + 1], b.wse, v);
            out[((size_t)f * Cout + c) * plane + (size_t)y * W + x] = v;
        }
    }
}

// one thread per (pixel, 4 channels); LPP lanes per pixel (C / 4) reduce the flow / occlusion partials before one atomic
__global__ __launch_bounds__(256) void warp_features_backward_kernel(const float* __restrict__ feat, const float* __restrict__ defo,
                                                                     const float* __restrict__ occ, const float* __restrict__ dout,
                                                                     int n, int ns, int hf, int wf, int C, float* __restrict__ dfeat,
                                                                     float* __restrict__ ddefo, float* __restrict__ docc) {
    const int c4n = C >> 2;
    const size_t total = (size_t)n * hf * wf * c4n;
    const bool pow2 = (c4n & (c4n - 1)) == 0 && c4n <= 64;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(idx % c4n);
        const size_t pix = idx / c4n;
        const int f = (int)(pix / ((size_t)wf * hf));
        const float2 g = reinterpret_cast<const float2*>(defo)[pix];
        const float o = occ ? occ[pix] : 1.f;
        const SamplePos b = sample_pos(g.x, g.y, wf, hf);
        // a thread owns channels c4 + k * c4n (k = 0..3): the lanes of a pixel touch CONSECUTIVE floats, so each atomic
        // instruction of the wave lands on whole cache lines (4 x fewer L2 atomic operations than a float4 per lane)
        const float* gp = dout + pix * C + c4;
        const float go[4] = {gp[0], gp[c4n], gp[2 * c4n], gp[3 * c4n]};
        const size_t sbase = (size_t)((ns == 1) ? 0 : f) * hf * wf;
        float dgx = 0.f, dgy = 0.f, dsum = 0.f;
        if (b.valid) {
            const float wx[2] = {1.f - b.ax, b.ax}, wy[2] = {1.f - b.ay, b.ay};
#pragma unroll
            for (int cy = 0; cy < 2; ++cy)
#pragma unroll
                for (int cx = 0; cx < 2; ++cx) {
                    const int yy = b.y0 + cy, xx = b.x0 + cx;
                    if ((unsigned)yy >= (unsigned)hf || (unsigned)xx >= (unsigned)wf) continue;   // zeros padding: no value, no gradient
                    const size_t src = (sbase + (size_t)yy * wf + xx) * C + c4;
                    const float* vp = feat + src;
                    const float dot = go[0] * vp[0] + go[1] * vp[c4n] + go[2] * vp[2 * c4n] + go[3] * vp[3 * c4n];   // sum_c dout * feat
                    const float w = wx[cx] * wy[cy];
                    dsum = fmaf(w, dot, dsum);
                    dgx = fmaf((cx ? 1.f : -1.f) * wy[cy], dot, dgx);                            // d w / d ix
                    dgy = fmaf((cy ? 1.f : -1.f) * wx[cx], dot, dgy);                            // d w / d iy
                    if (dfeat != nullptr) {
                        float* d = dfeat + src;
                        const float s = w * o;
#pragma unroll
                        for (int k = 0; k < 4; ++k) atomicAdd(d + k * c4n, go[k] * s);
                    }
                }
        }
        // ix = ((gx + 1) W - 1) / 2: d ix / d gx = W / 2 (likewise y); the occlusion factor multiplies the sampled value
        float pgx = dgx * o * 0.5f * (float)wf, pgy = dgy * o * 0.5f * (float)hf, po = dsum;
        if (pow2) {   // the c4n lanes of a pixel are a power-of-two aligned group of the wave
            for (int off = c4n >> 1; off > 0; off >>= 1) {
                pgx += __shfl_xor(pgx, off, 64);
                pgy += __shfl_xor(pgy, off, 64);
                po += __shfl_xor(po, off, 64);
            }
            if (c4 == 0) {
                if (ddefo != nullptr) {
                    atomicAdd(ddefo + pix * 2, pgx);
                    atomicAdd(ddefo + pix * 2 + 1, pgy);
                }
                if (docc != nullptr) atomicAdd(docc + pix, po);
            }
        } else {
            if (ddefo != nullptr) {
                atomicAdd(ddefo + pix * 2, pgx);
                atomicAdd(ddefo + pix * 2 + 1, pgy);
            }
            if (docc != nullptr) atomicAdd(docc + pix, po);
        }
    }
}

// ---- launchers ----
static inline int grid_for(size_t total, int cap = 16384) {
    return (int)std::min<size_t>((total + 255) / 256, (size_t)cap);
}

hipError_t warp_features_launch(const float* feat, const float* deformation, const float* occlusion, int n, int ns,
                                int hf, int wf, int C, int h, int w, float* out, float* out2, const float* s2,
                                const float* t2, hipStream_t s) {
    if (C % 8) return hipErrorInvalidValue;
    const size_t total = (size_t)n * hf * wf * (C / 8);
    hipLaunchKernelGGL(warp_features_kernel, dim3(grid_for(total, 1 << 20)), dim3(256), 0, s, feat, deformation,
                       occlusion, n, ns, hf, wf, C, h, w, out, out2, s2, t2);
    return hipGetLastError();
}

hipError_t warp_image_launch(const float* src, const float* deformation, int n, int ns, int H, int W, int h, int w,
                             float* out, hipStream_t s, int src_planes, int channels) {
    const size_t total = (size_t)n * H * W;
    hipLaunchKernelGGL(warp_image_kernel, dim3(grid_for(total)), dim3(256), 0, s, src, deformation, n, ns, H, W, h, w,
                       out, src_planes, channels);
    return hipGetLastError();
}

hipError_t warp_features_backward_launch(const float* feat, const float* defo, const float* occ, const float* dout, int n, int ns,
                                         int hf, int wf, int C, float* dfeat, float* ddefo, float* docc, hipStream_t s) {
    if (C % 4 || n < 1) return hipErrorInvalidValue;
    const size_t total = (size_t)n * hf * wf * (C / 4);
    // the in-wave reduction needs every lane of a pixel's group alive: whole groups per block, and a grid that covers the
    // tensor in one sweep of whole blocks (256 is a multiple of every power-of-two group size)
    const size_t blocks = (total + 255) / 256;
    if (blocks > (size_t)0x7FFFFFFF) return hipErrorInvalidValue;
    hipLaunchKernelGGL(warp_features_backward_kernel, dim3((unsigned)blocks), dim3(256), 0, s, feat, defo, occ, dout, n, ns, hf, wf, C,
                       dfeat, ddefo, docc);
    return hipGetLastError();
}

}  // namespace eamm
