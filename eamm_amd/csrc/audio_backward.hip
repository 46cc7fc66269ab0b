// The operators that make AT_net2's audio CNN and `decon` tail differentiable (reference modules/util.py:539-576; train.py's first
// stage trains them through an L1 loss on the audio-driven key points):
//
//   audio_maxpool_backward  MaxPool2d(3, (sy, sx)) without padding: a gather per input pixel over the windows that contain it, each
//                           window's winner recomputed from the input (the first maximum in row-major order, ATen's rule); the
//                           windows overlap, so nothing is scattered and there are no atomics.
//   deconv4s2_gather        ConvTranspose2d(k4, s2, p1) FORWARD and DATA GRADIENT as implicit GEMMs on v_mfma_f32_32x32x2_f32: the
//                           main loop is conv_gather_gemm.h's, on 64 x 64 tiles of four 32 x 32 waves; the kernel supplies the source
//                           pixel of a row, the tap walk and its store:
//                             forward: output pixel (2y+py, 2x+px) reads the 2x2 input neighbourhood (y-1+py+ty, x-1+px+tx) with tap
//                               (ky, kx) = (3-py-2ty, 3-px-2tx) -- the four-phase form of eamm_deconv_api.hip, one parity class per
//                               block, M = B*H*W, N = Cout, K = 4 taps x Cin; nothing is zero-stuffed;
//                             data gradient: dX[y,x] = sum over the 16 taps of dY[2y+ky-1, 2x+kx-1] W[:, :, ky, kx]^T: a 4x4 stride-2
//                               pad-1 convolution of dY, a gather per input pixel, M = B*H*W, N = Cin, K = 16 taps x Cout.
//                           Both read their filter from an image packed on the device by deconv4s2_pack_kernel.
//   deconv4s2_wgrad         dW[ci,co,ky,kx] = sum_p X[p][ci] dY[2p + (ky,kx) - 1][co]: backward.hip's strided_wgrad_kernel with X as its
//                           dense and dY as its gathered operand, 16 taps, pad 1; the pixel-split slabs summed in slice order.
//   deconv4s2_bias_grad     db[co] = sum_p dY[p][co], row lanes in a fixed order, the fold in double.
#include "conv_gather_gemm.h"

#include <algorithm>

namespace eamm {

__global__ __launch_bounds__(256) void audio_maxpool_backward_kernel(const float* __restrict__ in, const float* __restrict__ dy, int F, int H,
                                                                     int W, int C, int sy, int sx, int Ho, int Wo, float* __restrict__ dx) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;   // (frame, y, x, channel / 4)
    const int C4 = C >> 2;
    if (i >= (size_t)F * H * W * C4) return;
    const int c4 = (int)(i % C4);
    const size_t p = i / C4;
    const int x = (int)(p % W), y = (int)((p / W) % H);
    const size_t f = p / ((size_t)W * H);
    const f32x4* src = reinterpret_cast<const f32x4*>(in);
    const f32x4* g = reinterpret_cast<const f32x4*>(dy);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    // windows (oy, ox) with oy*sy <= y <= oy*sy + 2
    const int oy0 = y >= 2 ? (y - 2 + sy - 1) / sy : 0, oy1 = min(Ho - 1, y / sy);
    const int ox0 = x >= 2 ? (x - 2 + sx - 1) / sx : 0, ox1 = min(Wo - 1, x / sx);
    for (int oy = oy0; oy <= oy1; ++oy)
        for (int ox = ox0; ox <= ox1; ++ox) {
            const int me = (y - oy * sy) * 3 + (x - ox * sx);
            f32x4 m = src[((f * H + oy * sy) * W + ox * sx) * C4 + c4];
            int w0 = 0, w1 = 0, w2 = 0, w3 = 0;
            for (int k = 1; k < 9; ++k) {
                const f32x4 v = src[((f * H + oy * sy + k / 3) * W + ox * sx + k % 3) * C4 + c4];
                if (v.x > m.x) { m.x = v.x; w0 = k; }
                if (v.y > m.y) { m.y = v.y; w1 = k; }
                if (v.z > m.z) { m.z = v.z; w2 = k; }
                if (v.w > m.w) { m.w = v.w; w3 = k; }
            }
            const f32x4 d = g[((f * Ho + oy) * Wo + ox) * C4 + c4];
            if (w0 == me) acc.x += d.x;
            if (w1 == me) acc.y += d.y;
            if (w2 == me) acc.z += d.z;
            if (w3 == me) acc.w += d.w;
        }
    reinterpret_cast<f32x4*>(dx)[i] = acc;
}

hipError_t audio_maxpool_backward_launch(const float* in, const float* dy, int F, int H, int W, int C, int sy, int sx, float* dx, hipStream_t s) {
    if (C % 4 || H < 3 || W < 3 || sy < 1 || sx < 1 || sy > 3 || sx > 3) return hipErrorInvalidValue;
    const int Ho = (H - 3) / sy + 1, Wo = (W - 3) / sx + 1;
    const size_t n = (size_t)F * H * W * (C / 4);
    hipLaunchKernelGGL(audio_maxpool_backward_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, dy, F, H, W, C, sy, sx, Ho, Wo, dx);
    return hipGetLastError();
}

// ---- ConvTranspose2d(k4, s2, p1) -------------------------------------------------------------------------------------------------
namespace {

constexpr int T4_BM = 64, T4_BN = 64;

struct T4Args {
    const float* src;    // forward: x [B,H,W,Cin]; data gradient: dY [B,2H,2W,Cout]
    const float* w;      // deconv4s2_pack_kernel's image
    const float* bias;   // forward only, nullable
    float* out;          // forward: [B,2H,2W,N]; data gradient: [B,H,W,N]
    int H, W;            // the input map: the M = B*H*W rows of either GEMM
    int Cs, N;           // channels of src (the GEMM's K per tap) and of out
    int M, mtiles, ntiles;
    unsigned src_bytes, w_bytes;
};

}  // namespace

// image [N tile][class][tap][K chunk][64 n][32 k]; forward: 4 classes x 4 taps, k = ci, n = co; data gradient: 1 class x 16 taps,
// k = co, n = ci; columns beyond N are zeros
template <bool FWD>
__global__ __launch_bounds__(256) void deconv4s2_pack_kernel(const float* __restrict__ w, int Cin, int Cout, size_t total, float* __restrict__ dst) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int k = (int)(i & 31), n = (int)((i >> 5) & 63);
    size_t c = i >> 11;
    const int ncc = (FWD ? Cin : Cout) / 32;
    const int cc = (int)(c % ncc);
    c /= ncc;
    const int tap = (int)(c % (FWD ? 4 : 16));
    c /= (FWD ? 4 : 16);
    int cls = 0;
    if (FWD) {
        cls = (int)(c & 3);
        c >>= 2;
    }
    const int ntile = (int)c;
    int ci, co, ky, kx;
    if (FWD) {
        ci = cc * 32 + k;
        co = ntile * 64 + n;
        ky = 3 - (cls >> 1) - 2 * (tap >> 1);
        kx = 3 - (cls & 1) - 2 * (tap & 1);
    } else {
        co = cc * 32 + k;
        ci = ntile * 64 + n;
        ky = tap >> 2;
        kx = tap & 3;
    }
    dst[i] = (ci < Cin && co < Cout) ? w[(((size_t)ci * Cout + co) * 4 + ky) * 4 + kx] : 0.f;
}

// block (class, M tile, N tile); FWD: class = 2 py + px, the parity of the output pixel; data gradient: one class
template <bool FWD>
__global__ __launch_bounds__(256) void deconv4s2_gather_kernel(const T4Args p) {
    constexpr int BM = T4_BM, BN = T4_BN, BK = CONV_BK, LDK = CONV_LDK, NTAP = FWD ? 4 : 16;
    constexpr int A_PER = BM / 32;
    __shared__ __attribute__((aligned(16))) float As[2 * BM * LDK];
    __shared__ __attribute__((aligned(16))) float Bs[2 * BN * LDK];

    const GatherLanes g = gather_lanes<2>(threadIdx.x);
    const int l31 = g.l31, half = g.half, wm = g.wm, wn = g.wn;

    int L = blockIdx.x;
    const int ntile = L % p.ntiles;
    L /= p.ntiles;
    const int mtile = L % p.mtiles;
    L /= p.mtiles;
    const int cls = L, py = cls >> 1, px = cls & 1;
    const int mbase = mtile * BM;
    const int ncc = p.Cs / BK, nchunks = NTAP * ncc;
    const int Hs = FWD ? p.H : 2 * p.H, Ws = FWD ? p.W : 2 * p.W;   // the source map

    // operand loader: (qy, qx) = the source pixel of tap (0, 0), for the rows arow + 32 j that this thread stages
    const int arow = g.arow, acol = g.acol;
    int qy[A_PER], qx[A_PER], qb[A_PER];
#pragma unroll
    for (int j = 0; j < A_PER; ++j) {
        const int m = mbase + arow + 32 * j;
        if (m < p.M) {
            const int x = m % p.W, t = m / p.W;
            const int y = t % p.H;
            qy[j] = FWD ? y - 1 + py : 2 * y - 1;
            qx[j] = FWD ? x - 1 + px : 2 * x - 1;
            qb[j] = (t / p.H) * Hs * Ws;
        } else {
            qy[j] = -(1 << 20);   // never inside the map
            qx[j] = 0;
            qb[j] = 0;
        }
    }
    const __amdgpu_buffer_rsrc_t rs0 = gather_rsrc(p.src, p.src_bytes);
    const __amdgpu_buffer_rsrc_t rsw = gather_rsrc(p.w, p.w_bytes);
    const int wtile = (ntile * (FWD ? 4 : 1) + cls) * nchunks;

    // chunk ci = (tap, channel chunk cc): tap outer, as the packed image has it
    auto chunk = [&](int ci) {
        const int tap = ci / ncc, cc = ci - tap * ncc;
        const int ty = FWD ? tap >> 1 : tap >> 2, tx = FWD ? tap & 1 : tap & 3;
        const int coff = cc * BK + acol;
        return gather_chunk(rs0, [&, ty, tx, coff](int j) {
            const int yy = qy[j] + ty, xx = qx[j] + tx;
            const bool ok = ((unsigned)yy < (unsigned)Hs) & ((unsigned)xx < (unsigned)Ws);
            return ok ? (unsigned)((qb[j] + yy * Ws + xx) * p.Cs + coff) * 4u : GG_OOB;
        }, wtile + ci);
    };

    f32x16 acc[1][1];
    gather_gemm<1, 1, 2, 2>(acc, As, Bs, rsw, g, 0, nchunks, chunk);

    // D layout: lane -> column n = lane % 32; register r -> row (r % 4) + 8 (r / 4) + 4 (lane / 32)
    const int n = ntile * BN + wn * 32 + l31;
    if (n >= p.N) return;
    const float bias = (FWD && p.bias) ? p.bias[n] : 0.f;
    static_for<16>([&](auto rc) {
        constexpr int r = decltype(rc)::value;
        const int m = mbase + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (m < p.M) {
            const int x = m % p.W, t = m / p.W;
            const int y = t % p.H, b = t / p.H;
            if (FWD) p.out[(((size_t)b * 2 * p.H + 2 * y + py) * 2 * p.W + 2 * x + px) * p.N + n] = acc[0][0][r] + bias;
            else p.out[(size_t)m * p.N + n] = acc[0][0][r];
        }
    });
}

// one block per 32 channels: 8 row lanes stride the pixels, LDS folds them in double
__global__ __launch_bounds__(256) void deconv4s2_bias_grad_kernel(const float* __restrict__ dy, long long P, int Cout, float* __restrict__ db) {
    __shared__ double red[8][32];
    const int cl = threadIdx.x & 31, r = threadIdx.x >> 5, c = blockIdx.x * 32 + cl;
    double s = 0.0;
    if (c < Cout)
        for (long long pp = r; pp < P; pp += 8) s += (double)dy[pp * Cout + c];
    red[r][cl] = s;
    __syncthreads();
    if (r == 0 && c < Cout) {
        for (int k = 1; k < 8; ++k) s += red[k][cl];
        db[c] = (float)s;
    }
}

namespace {
bool t4_shape_ok(int B, int H, int W, int Cin, int Cout) {
    if (B < 1 || H < 1 || W < 1 || Cin < CONV_BK || Cout < CONV_BK || Cin % CONV_BK || Cout % CONV_BK) return false;
    // 32-bit element offsets in the kernels, 32-bit byte ranges in the buffer descriptors
    const unsigned long long big = std::max<unsigned long long>((unsigned long long)B * H * W * Cin, 4ull * B * H * W * Cout);
    return big * sizeof(float) < 0xFFFFFFF0ull && 16ull * ((Cin + 63) / 64 * 64) * ((Cout + 63) / 64 * 64) * sizeof(float) < 0x7FFFFFF0ull;
}
size_t t4_packed_elems(int Cin, int Cout, bool fwd) {   // 16 (class, tap) pairs either way
    return fwd ? (size_t)((Cout + 63) / 64) * 16 * (Cin / 32) * 64 * 32 : (size_t)((Cin + 63) / 64) * 16 * (Cout / 32) * 64 * 32;
}
}  // namespace

size_t deconv4s2_workspace_floats(int B, int H, int W, int Cin, int Cout, int which) {
    if (!t4_shape_ok(B, H, W, Cin, Cout)) return 0;
    if (which == 0 || which == 1) return round64(t4_packed_elems(Cin, Cout, which == 0));
    if (which != 2) return 0;
    return strided_wgrad_workspace_floats(B * H * W, Cin, Cout, 4);
}

template <bool FWD>
static hipError_t t4_gather(const float* src, const float* weight, const float* bias, int B, int H, int W, int Cin, int Cout, float* out,
                            float* workspace, size_t workspace_floats, hipStream_t s) {
    const size_t need = deconv4s2_workspace_floats(B, H, W, Cin, Cout, FWD ? 0 : 1);
    if (need == 0 || workspace_floats < need || (reinterpret_cast<uintptr_t>(workspace) & 15)) return hipErrorInvalidValue;
    const size_t packed = t4_packed_elems(Cin, Cout, FWD);
    hipLaunchKernelGGL(deconv4s2_pack_kernel<FWD>, dim3((unsigned)((packed + 255) / 256)), dim3(256), 0, s, weight, Cin, Cout, packed, workspace);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    T4Args a{};
    a.src = src;
    a.w = workspace;
    a.bias = bias;
    a.out = out;
    a.H = H;
    a.W = W;
    a.Cs = FWD ? Cin : Cout;
    a.N = FWD ? Cout : Cin;
    a.M = B * H * W;
    a.mtiles = (a.M + T4_BM - 1) / T4_BM;
    a.ntiles = (a.N + T4_BN - 1) / T4_BN;
    a.src_bytes = (unsigned)((size_t)a.M * (FWD ? 1 : 4) * a.Cs * sizeof(float));
    a.w_bytes = (unsigned)(packed * sizeof(float));
    const long long blocks = (FWD ? 4ll : 1ll) * a.mtiles * a.ntiles;
    if (blocks > 0x7FFFFFFFll) return hipErrorInvalidValue;
    note_mfma_flops(2.0 * 16.0 * a.Cs * (double)a.mtiles * T4_BM * (double)a.ntiles * T4_BN);
    hipLaunchKernelGGL(deconv4s2_gather_kernel<FWD>, dim3((unsigned)blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t deconv4s2_forward_launch(const float* x, const float* weight, const float* bias, int B, int H, int W, int Cin, int Cout, float* out,
                                    float* workspace, size_t workspace_floats, hipStream_t s) {
    return t4_gather<true>(x, weight, bias, B, H, W, Cin, Cout, out, workspace, workspace_floats, s);
}

hipError_t deconv4s2_dgrad_launch(const float* dy, const float* weight, int B, int H, int W, int Cin, int Cout, float* dx, float* workspace,
                                  size_t workspace_floats, hipStream_t s) {
    return t4_gather<false>(dy, weight, nullptr, B, H, W, Cin, Cout, dx, workspace, workspace_floats, s);
}

hipError_t deconv4s2_wgrad_launch(const float* x, const float* dy, int B, int H, int W, int Cin, int Cout, float* dweight, float* dbias,
                                  float* workspace, size_t workspace_floats, hipStream_t s) {
    const size_t need = deconv4s2_workspace_floats(B, H, W, Cin, Cout, 2);
    if (need == 0 || workspace_floats < need || (reinterpret_cast<uintptr_t>(workspace) & 15)) return hipErrorInvalidValue;
    // dense = x: the rows of [Cin][Cout][4][4], the reference's ConvTranspose2d layout
    if (hipError_t e = strided_wgrad_launch(x, dy, B, H, W, Cin, Cout, 4, 1, dweight, workspace, s); e != hipSuccess) return e;
    if (dbias) {
        hipLaunchKernelGGL(deconv4s2_bias_grad_kernel, dim3((Cout + 31) / 32), dim3(256), 0, s, dy, 4ll * B * H * W, Cout, dbias);
        return hipGetLastError();
    }
    return hipSuccess;
}

}  // namespace eamm
