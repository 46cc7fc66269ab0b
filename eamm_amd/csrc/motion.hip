// HBM-bound kernels of the dense-motion path: key-point records, heat-map / sparse-motion / warped-source front end, the
// softmax-over-motions flow head (the two inference forms and the training entry's), anti-alias down-sampling and the
// once-per-clip source preparation; beside them the layout and format changes of the frozen path (broadcast_features,
// nchw_to_nhwc_pad, to_u8).  One thread per output element group, NHWC / float4 accesses.  Their backward: motion_backward.hip.
// The warps that consume the flow are warp.hip, the key-point heads' reduction is kp_head.hip, the final layer's second half is
// conv_col7.hip; what these share is pointwise.h.
//
// Semantics follow SURVEY.md Appendix A; each kernel cites the reference lines it replaces.
#include "pointwise.h"

#include <algorithm>

namespace eamm {

// ---------------------------------------------------------------------------------------------
// key-point records: J_k = J_source,k * inverse(J_driving,k)  (dense_motion.py:55-56)
// ---------------------------------------------------------------------------------------------
__global__ void kp_prepare_kernel(const float* __restrict__ kd_val, const float* __restrict__ kd_jac,
                                  const float* __restrict__ ks_val, const float* __restrict__ ks_jac, int n, int ns,
                                  int K, float* __restrict__ rec, int* __restrict__ bad) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * K) return;
    const int f = i / K, k = i - f * K;
    const int sf = (ns == 1) ? 0 : f;
    float* r = rec + (size_t)i * KP_STRIDE;
    r[0] = kd_val[i * 2 + 0];
    r[1] = kd_val[i * 2 + 1];
    r[2] = ks_val[(sf * K + k) * 2 + 0];
    r[3] = ks_val[(sf * K + k) * 2 + 1];
    float j00 = 1.f, j01 = 0.f, j10 = 0.f, j11 = 1.f;
    if (kd_jac != nullptr) {
        const float* d = kd_jac + (size_t)i * 4;
        const float* s = ks_jac + (size_t)(sf * K + k) * 4;
        const float det = d[0] * d[3] - d[1] * d[2];
        if (!(fabsf(det) > 0.f) || !isfinite(det)) atomicExch(bad, 1);  // torch.inverse raises here
        const float inv = 1.f / det;
        const float i00 = d[3] * inv, i01 = -d[1] * inv, i10 = -d[2] * inv, i11 = d[0] * inv;
        j00 = fmaf(s[1], i10, s[0] * i00);
        j01 = fmaf(s[1], i11, s[0] * i01);
        j10 = fmaf(s[3], i10, s[2] * i00);
        j11 = fmaf(s[3], i11, s[2] * i01);
    }
    r[4] = j00;
    r[5] = j01;
    r[6] = j10;
    r[7] = j11;
}

// ---------------------------------------------------------------------------------------------
// front end: heat-maps (dense_motion.py:32-45, util.py:815-836), sparse motions (:47-67) and the K+1
// bilinear warps of the down-sampled source (:69-79), written straight into the hourglass input
// layout: channel 4k = heat_k, 4k+1..3 = RGB warped by T_k (:93-94), zero-padded to Cpad channels.
// ---------------------------------------------------------------------------------------------
// Image channels beyond three (num_channels 4 .. 6; generator.py:14 accepts any): the channels are handled in GROUPS of three,
// one launch per group g: the per-motion record of the hourglass input grows to G float4 -- group 0 writes (heat, c0, c1, c2) at
// slot k G, group g >= 1 writes (c_3g, c_3g+1, c_3g+2, 0) at slot k G + g -- so that a motion's C + 1 real values stay contiguous
// (heat, c0 .. c_{C-1}) for C <= 6, which is how pad_state_dict lays the filters out.  sparse_deformed planes: [n, K+1, Ctot, h, w],
// this launch writes channels coff .. coff + cn - 1.  One group (G = 1, Ctot = 3, cn = 3): the RGB layout of rounds 1-4.
__global__ __launch_bounds__(256) void motion_front_kernel(const float* __restrict__ rec_all,
                                                           const float4* __restrict__ src_small, int ns, int K, int h,
                                                           int w, float variance, int Cpad,
                                                           float* __restrict__ hg_in,
                                                           float* __restrict__ sparse_deformed, int G, int g, int Ctot, int cn) {
    const int f = blockIdx.y;
    const int pi = blockIdx.x * blockDim.x + threadIdx.x;
    if (pi >= h * w) return;
    const int y = pi / w, x = pi - y * w;
    const float gx = grid_coord(x, w), gy = grid_coord(y, h);
    const float4* src = src_small + (size_t)((ns == 1) ? 0 : f) * h * w;
    const float* rec = rec_all + (size_t)f * K * KP_STRIDE;
    float4* dst = reinterpret_cast<float4*>(hg_in + ((size_t)f * h * w + pi) * Cpad);
    const size_t plane = (size_t)h * w;
    const int coff = 3 * g;
    float* sd = sparse_deformed ? sparse_deformed + ((size_t)f * (K + 1) * Ctot + coff) * plane + pi : nullptr;
    for (int k = 0; k <= K; ++k) {
        float tx = gx, ty = gy, heat = 0.f;
        if (k > 0) {
            const float* r = rec + (k - 1) * KP_STRIDE;
            sparse_motion(r, gx, gy, tx, ty);
            const float dx = gx - r[0], dy = gy - r[1];
            const float sx = gx - r[2], sy = gy - r[3];
            // |z - kp|^2 with the fused multiply-add written out: left to the compiler, a packed multiply of the two squares
            // (two roundings) can take its place
            heat = expf(-0.5f * fmaf(dx, dx, dy * dy) / variance) - expf(-0.5f * fmaf(sx, sx, sy * sy) / variance);
        }
        const Bilinear b = bilinear_setup(tx, ty, w, h);
        float r_ = 0.f, g_ = 0.f, b_ = 0.f;
        const bool x0ok = (unsigned)b.x0 < (unsigned)w, x1ok = (unsigned)(b.x0 + 1) < (unsigned)w;
        const bool y0ok = (unsigned)b.y0 < (unsigned)h, y1ok = (unsigned)(b.y0 + 1) < (unsigned)h;
        // branch-free taps: out-of-range corners read a clamped address and the loaded VALUE is replaced by zero (zeros
        // padding, util.py:69-79; zeroing the weight instead would turn a non-finite border pixel into 0 * Inf = NaN) --
        // a bounds branch around each load made the four loads of a key point, and the key points, wait for one another
        const int xa = min(max(b.x0, 0), w - 1), xb = min(max(b.x0 + 1, 0), w - 1);
        const int ya = min(max(b.y0, 0), h - 1) * w, yb = min(max(b.y0 + 1, 0), h - 1) * w;
        const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 lnw = src[ya + xa], lne = src[ya + xb], lsw = src[yb + xa], lse = src[yb + xb];
        const float4 vnw = (y0ok && x0ok) ? lnw : z4, vne = (y0ok && x1ok) ? lne : z4;
        const float4 vsw = (y1ok && x0ok) ? lsw : z4, vse = (y1ok && x1ok) ? lse : z4;
        const float wnw = b.wnw, wne = b.wne, wsw = b.wsw, wse = b.wse;
        r_ = fmaf(vnw.x, wnw, r_); g_ = fmaf(vnw.y, wnw, g_); b_ = fmaf(vnw.z, wnw, b_);
        r_ = fmaf(vne.x, wne, r_); g_ = fmaf(vne.y, wne, g_); b_ = fmaf(vne.z, wne, b_);
        r_ = fmaf(vsw.x, wsw, r_); g_ = fmaf(vsw.y, wsw, g_); b_ = fmaf(vsw.z, wsw, b_);
        r_ = fmaf(vse.x, wse, r_); g_ = fmaf(vse.y, wse, g_); b_ = fmaf(vse.z, wse, b_);
        dst[k * G + g] = g == 0 ? make_float4(heat, r_, g_, b_) : make_float4(r_, g_, b_, 0.f);
        if (sd) {
            sd[(size_t)(k * Ctot + 0) * plane] = r_;
            if (cn > 1) sd[(size_t)(k * Ctot + 1) * plane] = g_;
            if (cn > 2) sd[(size_t)(k * Ctot + 2) * plane] = b_;
        }
    }
    if (g == 0)
        for (int c4 = (K + 1) * G; c4 < Cpad / 4; ++c4) dst[c4] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// ---------------------------------------------------------------------------------------------
// head: mask = softmax over the K+1 motion logits, deformation = sum_k mask_k * T_k, occlusion =
// sigmoid(logit K+1)  (dense_motion.py:98-111).  logits come from the 7x7 MFMA convolution as
// [n,h,w,32] (channels 0..K mask, K+1 occlusion, rest padding).
// ---------------------------------------------------------------------------------------------
constexpr int HEAD_MAXK = 31;

// the occlusion logit where it is slot K + 1 of the mask logits' register line (K <= 30)
__device__ __forceinline__ float head_occ_slot(const float (&l)[32], int K) {
    float ov = 0.f;
#pragma unroll
    for (int k = 1; k < 32; ++k)
        if (k == K + 1) ov = l[k];
    return ov;
}

// l[0..K] mask logits, ov the occlusion logit of pixel pi of frame f -> softmax, flow, sigmoid, outputs
__device__ __forceinline__ void head_finish(float (&l)[32], float ov, const float* __restrict__ rec, int K, int h, int w, int f,
                                            int pi, int has_occ, float* __restrict__ deformation,
                                            float* __restrict__ occlusion, float* __restrict__ mask_out,
                                            float* __restrict__ occ_out) {
    const int y = pi / w, x = pi - y * w;
    const float gx = grid_coord(x, w), gy = grid_coord(y, h);
    float mx = l[0];
#pragma unroll
    for (int k = 1; k < 32; ++k)
        if (k <= K) mx = fmaxf(mx, l[k]);
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < 32; ++k)
        if (k <= K) {
            l[k] = expf(l[k] - mx);
            sum += l[k];
        }
    float dx = 0.f, dy = 0.f;
    const size_t plane = (size_t)h * w;
#pragma unroll
    for (int k = 0; k < 32; ++k)
        if (k <= K) {
            const float mk = l[k] / sum;
            float tx = gx, ty = gy;
            if (k > 0) sparse_motion(rec + (k - 1) * KP_STRIDE, gx, gy, tx, ty);
            dx = fmaf(mk, tx, dx);
            dy = fmaf(mk, ty, dy);
            if (mask_out) mask_out[((size_t)f * (K + 1) + k) * plane + pi] = mk;
        }
    reinterpret_cast<float2*>(deformation)[(size_t)f * plane + pi] = make_float2(dx, dy);
    if (has_occ) {
        const float o = 1.f / (1.f + expf(-ov));
        occlusion[(size_t)f * plane + pi] = o;
        if (occ_out) occ_out[(size_t)f * plane + pi] = o;
    }
}

__global__ __launch_bounds__(256) void motion_head_kernel(const float* __restrict__ logits,
                                                          const float* __restrict__ rec_all, int K, int h, int w,
                                                          int has_occ, float* __restrict__ deformation,
                                                          float* __restrict__ occlusion, float* __restrict__ mask_out,
                                                          float* __restrict__ occ_out) {
    const int f = blockIdx.y;
    const int pi = blockIdx.x * blockDim.x + threadIdx.x;
    if (pi >= h * w) return;
    const float4* lg4 = reinterpret_cast<const float4*>(logits + ((size_t)f * h * w + pi) * 32);
    float l[32];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float4 v = lg4[i];
        l[4 * i + 0] = v.x; l[4 * i + 1] = v.y; l[4 * i + 2] = v.z; l[4 * i + 3] = v.w;
    }
    head_finish(l, head_occ_slot(l, K), rec_all + (size_t)f * K * KP_STRIDE, K, h, w, f, pi, has_occ, deformation, occlusion,
                mask_out, occ_out);
}

// The training entry's form: the mask logits [n,h,w,ld] (channels 0..K) and the occlusion logit [n,h,w,ldo] (channel 0; lo null:
// none) come from convolutions of any channel stride, so the line is filled float by float; the occlusion logit travels beside
// it, which lets K = 31 fill all 32 slots.  Same softmax, flow combine and sigmoid: bit-equal to motion_head_kernel.
__global__ __launch_bounds__(256) void motion_head_forward_kernel(const float* __restrict__ lm, int ld, const float* __restrict__ lo,
                                                                  int ldo, const float* __restrict__ rec_all, int K, int h, int w,
                                                                  float* __restrict__ mask, float* __restrict__ deformation,
                                                                  float* __restrict__ occlusion) {
    const int f = blockIdx.y;
    const int pi = blockIdx.x * blockDim.x + threadIdx.x;
    if (pi >= h * w) return;
    const float* row = lm + ((size_t)f * h * w + pi) * ld;
    float l[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) l[k] = k <= K ? row[k] : 0.f;
    const float ov = lo ? lo[((size_t)f * h * w + pi) * ldo] : 0.f;
    head_finish(l, ov, rec_all + (size_t)f * K * KP_STRIDE, K, h, w, f, pi, lo != nullptr, deformation, occlusion, mask, nullptr);
}

// Row-split form: the 7x7 head ran as a 7x1 (vertical) MFMA convolution with N = (dx, co), co < NC = K+1(+1):
// part[f,y,x',dx*NC+co] (pixel stride PS floats).  One block = 64 pixels of one row; the 70 x 7*NC partial products
// are staged in LDS (odd row stride: conflict-free column walks), then each thread gathers its 7 horizontal taps,
// adds the bias and finishes as above.
constexpr int HR_TILE = 64;
__global__ __launch_bounds__(HR_TILE) void motion_head_rowsplit_kernel(const float* __restrict__ part, int PS, int NC,
                                                                       const float* __restrict__ bias,
                                                                       const float* __restrict__ rec_all, int K, int h,
                                                                       int w, int has_occ,
                                                                       float* __restrict__ deformation,
                                                                       float* __restrict__ occlusion,
                                                                       float* __restrict__ mask_out,
                                                                       float* __restrict__ occ_out) {
    extern __shared__ float tile[];   // [(HR_TILE + 6)][7*NC | 1]
    const int NV = 7 * NC, LD = NV | 1;
    const int x0 = blockIdx.x * HR_TILE, y = blockIdx.y, f = blockIdx.z;
    const float* row = part + ((size_t)(f * h + y) * w) * PS;
    if (((NV | PS) & 3) == 0) {   // 16-byte loads (the pixel stride and the used width are multiples of 4 floats)
        const int NV4 = NV >> 2;
        for (int i = threadIdx.x; i < (HR_TILE + 6) * NV4; i += blockDim.x) {
            const int px = i / NV4, c4 = i - px * NV4;
            const int x = x0 + px - 3;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if ((unsigned)x < (unsigned)w) v = *reinterpret_cast<const float4*>(row + (size_t)x * PS + 4 * c4);
            float* d = tile + px * LD + 4 * c4;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
    } else {
        for (int i = threadIdx.x; i < (HR_TILE + 6) * NV; i += blockDim.x) {
            const int px = i / NV, c = i - px * NV;
            const int x = x0 + px - 3;
            tile[px * LD + c] = (unsigned)x < (unsigned)w ? row[(size_t)x * PS + c] : 0.f;
        }
    }
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x >= w) return;
    float l[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) {
        float v = 0.f;
        if (k < NC) {
            v = bias[k];
            for (int dx = 0; dx < 7; ++dx) v += tile[(threadIdx.x + dx) * LD + dx * NC + k];
        }
        l[k] = v;
    }
    head_finish(l, head_occ_slot(l, K), rec_all + (size_t)f * K * KP_STRIDE, K, h, w, f, y * w + x, has_occ, deformation,
                occlusion, mask_out, occ_out);
}

// ---------------------------------------------------------------------------------------------
// once per clip: NCHW RGB source -> (a) NHWC zero-padded to Cpad channels for the 7x7 MFMA encoder
// convolution, (b) anti-aliased, down-sampled [h,w,4] copy for the motion front end
// (AntiAliasInterpolation2d, util.py:1044-1052: zero pad 6, depthwise 13x13, keep every inv_scale-th
// row/column -- only the kept outputs are computed).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void source_to_nhwc_kernel(const float* __restrict__ src, int ns, int H, int W,
                                                             int Cpad, float* __restrict__ dst) {
    const size_t plane = (size_t)H * W;
    const int c4n = Cpad >> 2;
    const size_t total = (size_t)ns * plane * c4n;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (size_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(idx % c4n);
        const size_t pix = idx / c4n;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c4 == 0) {
            const size_t b = pix / plane, r = pix % plane;
            const float* p = src + b * 3 * plane + r;
            v = make_float4(p[0], p[plane], p[2 * plane], 0.f);
        }
        reinterpret_cast<float4*>(dst)[idx] = v;
    }
}

// cn (1 .. 4) channels coff .. coff + cn - 1 of a source with Cplanes planes per image -> one float4 per kept pixel, written at
// float4 slot `slot` of the pixel's c4pad slots; `fill`: the pixel's other slots are zeroed (the first launch of a pixel line).
__global__ __launch_bounds__(256) void antialias_down_kernel(const float* __restrict__ src,
                                                             const float* __restrict__ aa_w, int ns, int H, int W,
                                                             int inv_scale, int c4pad, float4* __restrict__ dst, int Cplanes,
                                                             int coff, int cn, int slot, int fill) {
    const int h = H / inv_scale, w = W / inv_scale;
    const size_t plane = (size_t)H * W;
    const size_t total = (size_t)ns * h * w;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int x = (int)(idx % w), y = (int)((idx / w) % h), b = (int)(idx / ((size_t)w * h));
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (inv_scale == 1) {
        for (int c = 0; c < cn; ++c) acc[c] = src[((size_t)b * Cplanes + coff + c) * plane + (size_t)y * W + x];
    } else {
        const int cy = y * inv_scale - 6, cx = x * inv_scale - 6;
        for (int c = 0; c < cn; ++c) {
            const float* p = src + ((size_t)b * Cplanes + coff + c) * plane;
            const float* k = aa_w + (coff + c) * 169;
            float s = 0.f;
            for (int ky = 0; ky < 13; ++ky) {
                const int yy = cy + ky;
                if ((unsigned)yy >= (unsigned)H) continue;
                for (int kx = 0; kx < 13; ++kx) {
                    const int xx = cx + kx;
                    if ((unsigned)xx >= (unsigned)W) continue;
                    s = fmaf(p[(size_t)yy * W + xx], k[ky * 13 + kx], s);
                }
            }
            acc[c] = s;
        }
    }
    dst[idx * c4pad + slot] = make_float4(acc[0], acc[1], acc[2], acc[3]);
    if (fill)
        for (int k = 0; k < c4pad; ++k)
            if (k != slot) dst[idx * c4pad + k] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// prediction [n,3,H,W] float -> [n,H,W,3] uint8 (img_as_ubyte rounding), the frame format demo.py:507 saves.
__global__ __launch_bounds__(256) void to_u8_kernel(const float* __restrict__ pred, int n, int H, int W,
                                                    uint8_t* __restrict__ out) {
    const size_t plane = (size_t)H * W;
    const size_t total = (size_t)n * plane;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (size_t)gridDim.x * blockDim.x) {
        const size_t f = idx / plane, r = idx % plane;
        const float* p = pred + f * 3 * plane + r;
        for (int c = 0; c < 3; ++c) {
            const float v = fminf(fmaxf(rintf(p[c * plane] * 255.f), 0.f), 255.f);
            out[idx * 3 + c] = (uint8_t)v;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
static inline int grid_for(size_t total, int cap = 16384) {
    return (int)std::min<size_t>((total + 255) / 256, (size_t)cap);
}

hipError_t kp_prepare_launch(const float* kd_val, const float* kd_jac, const float* ks_val, const float* ks_jac, int n,
                             int ns, int K, float* kp_rec, int* bad_flag, hipStream_t s) {
    hipLaunchKernelGGL(kp_prepare_kernel, dim3((n * K + 255) / 256), dim3(256), 0, s, kd_val, kd_jac, ks_val, ks_jac,
                       n, ns, K, kp_rec, bad_flag);
    return hipGetLastError();
}

hipError_t motion_front_launch(const float* kp_rec, const float* src_small, int n, int ns, int K, int h, int w,
                               float variance, int Cpad, float* hg_in, float* sparse_deformed, hipStream_t s, int groups,
                               int channels, size_t group_stride) {
    // one launch per group of three image channels (groups = 1, channels = 3: the RGB layout); src_small of group g starts
    // group_stride floats behind group g - 1's
    if (groups < 1 || groups > 2 || channels < 1 || channels > 3 * groups || (K + 1) * 4 * groups > Cpad) return hipErrorInvalidValue;
    for (int g = 0; g < groups; ++g)
        hipLaunchKernelGGL(motion_front_kernel, dim3((h * w + 255) / 256, n), dim3(256), 0, s, kp_rec,
                           reinterpret_cast<const float4*>(src_small + (size_t)g * group_stride), ns, K, h, w, variance, Cpad, hg_in,
                           sparse_deformed, groups, g, groups == 1 ? 3 : channels, std::min(3, channels - 3 * g));
    return hipGetLastError();
}

hipError_t motion_head_launch(const float* logits, const float* kp_rec, int n, int K, int h, int w, int has_occ,
                              float* deformation, float* occlusion, float* mask_out, float* occ_out, hipStream_t s) {
    if (K > HEAD_MAXK - 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(motion_head_kernel, dim3((h * w + 255) / 256, n), dim3(256), 0, s, logits, kp_rec, K, h, w,
                       has_occ, deformation, occlusion, mask_out, occ_out);
    return hipGetLastError();
}

hipError_t motion_head_forward_launch(const float* lm, int ld, const float* lo, int ldo, const float* rec, int n, int K, int h, int w,
                                      float* mask, float* deformation, float* occlusion, hipStream_t s) {
    if (K < 1 || K > HEAD_MAXK || ld < K + 1 || (lo && ldo < 1)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(motion_head_forward_kernel, dim3((h * w + 255) / 256, n), dim3(256), 0, s, lm, ld, lo, ldo, rec, K, h, w, mask,
                       deformation, occlusion);
    return hipGetLastError();
}

hipError_t motion_head_rowsplit_launch(const float* part, int PS, int NC, const float* bias, const float* kp_rec, int n,
                                       int K, int h, int w, int has_occ, float* deformation, float* occlusion,
                                       float* mask_out, float* occ_out, hipStream_t s) {
    if (K > HEAD_MAXK - 1 || NC > 32) return hipErrorInvalidValue;
    const size_t lds = sizeof(float) * (HR_TILE + 6) * ((7 * NC) | 1);
    hipLaunchKernelGGL(motion_head_rowsplit_kernel, dim3((w + HR_TILE - 1) / HR_TILE, h, n), dim3(HR_TILE), lds, s, part,
                       PS, NC, bias, kp_rec, K, h, w, has_occ, deformation, occlusion, mask_out, occ_out);
    return hipGetLastError();
}

// A generator built without a motion network (dense_motion_params=None, generator.py:22-23, 64): the encoder features go
// to the bottleneck unwarped -- frame i gets source i (or the one cached source); second output relu(x*s + t) is the first
// res-block's pre-activation for the direct convolution form.
__global__ void broadcast_features_kernel(const float4* __restrict__ feat, int ns, size_t per_frame4, int C4, size_t total4,
                                          float4* __restrict__ out, float4* __restrict__ out2, const float4* __restrict__ s2,
                                          const float4* __restrict__ t2) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (size_t)gridDim.x * blockDim.x) {
        const size_t f = i / per_frame4, r = i - f * per_frame4;
        const float4 v = feat[(ns == 1 ? 0 : f) * per_frame4 + r];
        out[i] = v;
        if (out2 != nullptr) {
            const float4 s = s2[r % C4], t = t2[r % C4];
            float4 a;
            a.x = fmaxf(fmaf(v.x, s.x, t.x), 0.f); a.y = fmaxf(fmaf(v.y, s.y, t.y), 0.f);
            a.z = fmaxf(fmaf(v.z, s.z, t.z), 0.f); a.w = fmaxf(fmaf(v.w, s.w, t.w), 0.f);
            out2[i] = a;
        }
    }
}

hipError_t broadcast_features_launch(const float* feat, int n, int ns, int hf, int wf, int C, float* out, float* out2,
                                     const float* s2, const float* t2, hipStream_t s) {
    if (C & 3) return hipErrorInvalidValue;
    const size_t per_frame4 = (size_t)hf * wf * C / 4, total4 = per_frame4 * n;
    const int blocks = (int)std::min<size_t>((total4 + 255) / 256, (size_t)1 << 16);
    hipLaunchKernelGGL(broadcast_features_kernel, dim3(blocks), dim3(256), 0, s, reinterpret_cast<const float4*>(feat), ns,
                       per_frame4, C / 4, total4, reinterpret_cast<float4*>(out), reinterpret_cast<float4*>(out2),
                       reinterpret_cast<const float4*>(s2), reinterpret_cast<const float4*>(t2));
    return hipGetLastError();
}

hipError_t source_prepare_launch(const float* src, const float* aa_w, int ns, int H, int W, int inv_scale, int Cpad,
                                 float* src_nhwc, float* src_small, hipStream_t s) {
    const size_t t1 = (size_t)ns * H * W * (Cpad / 4);
    hipLaunchKernelGGL(source_to_nhwc_kernel, dim3(grid_for(t1)), dim3(256), 0, s, src, ns, H, W, Cpad, src_nhwc);
    const size_t t2 = (size_t)ns * (H / inv_scale) * (W / inv_scale);
    hipLaunchKernelGGL(antialias_down_kernel, dim3((unsigned)((t2 + 255) / 256)), dim3(256), 0, s, src, aa_w, ns, H, W,
                       inv_scale, 1, reinterpret_cast<float4*>(src_small), 3, 0, 3, 0, 1);
    return hipGetLastError();
}

hipError_t antialias_down_launch(const float* src, const float* aa_w, int ns, int H, int W, int inv_scale, int Cpad,
                                 float* dst, hipStream_t s, int src_planes, int first_channel, int channels, int slot) {
    // `channels` (1 .. 4) channels from first_channel on of a source with src_planes planes per image (aa_w: one 13x13 filter per
    // plane) into float4 slot `slot` of every pixel's Cpad / 4 slots; slot 0 also zeroes the pixel's other slots
    if (channels < 1 || channels > 4 || slot < 0 || slot >= Cpad / 4 || first_channel + channels > src_planes) return hipErrorInvalidValue;
    const size_t t2 = (size_t)ns * (H / inv_scale) * (W / inv_scale);
    hipLaunchKernelGGL(antialias_down_kernel, dim3((unsigned)((t2 + 255) / 256)), dim3(256), 0, s, src, aa_w, ns, H, W,
                       inv_scale, Cpad / 4, reinterpret_cast<float4*>(dst), src_planes, first_channel, channels, slot, slot == 0 ? 1 : 0);
    return hipGetLastError();
}

// [B,C,h,w] feature map -> [B,h,w,Cpad] (zero padded): the layout the MFMA convolutions read (the key-point detectors' input).
__global__ __launch_bounds__(256) void nchw_to_nhwc_pad_kernel(const float* __restrict__ src, int B, int C, int HW,
                                                               int Cpad, float* __restrict__ dst, int planes) {
    const size_t total = (size_t)B * HW * Cpad;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(idx % Cpad);
        const size_t pix = idx / Cpad;
        const size_t b = pix / HW, r = pix % HW;
        dst[idx] = c < C ? src[(b * planes + c) * HW + r] : 0.f;     // (the first C of `planes` planes per image)
    }
}

hipError_t nchw_to_nhwc_pad_launch(const float* src, int B, int C, int H, int W, int Cpad, float* dst, hipStream_t s, int planes) {
    const size_t total = (size_t)B * H * W * Cpad;
    hipLaunchKernelGGL(nchw_to_nhwc_pad_kernel, dim3(grid_for(total)), dim3(256), 0, s, src, B, C, H * W, Cpad, dst, planes > 0 ? planes : C);
    return hipGetLastError();
}

hipError_t to_u8_launch(const float* pred, int n, int H, int W, uint8_t* out, hipStream_t s) {
    hipLaunchKernelGGL(to_u8_kernel, dim3(grid_for((size_t)n * H * W)), dim3(256), 0, s, pred, n, H, W, out);
    return hipGetLastError();
}

}  // namespace eamm