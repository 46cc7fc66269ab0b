// The operators that make AT_net2's audio CNN and `decon` tail differentiable (reference modules/util.py:539-576; train.py's first
// stage trains them through an L1 loss on the audio-driven key points):
//
//   audio_maxpool_backward  MaxPool2d(3, (sy, sx)) without padding: a gather per input pixel over the windows that contain it, each
//                           window's winner recomputed from the input (the first maximum in row-major order, ATen's rule); the
//                           windows overlap, so nothing is scattered and there are no atomics.
//   deconv4s2_gather        ConvTranspose2d(k4, s2, p1) FORWARD and DATA GRADIENT as implicit GEMMs on v_mfma_f32_32x32x2_f32, in
//                           conv_s2_backward.hip's gather form (raw buffer loads, an out-of-range offset reads zero, LDS double
//                           buffer, one barrier per 32-channel chunk, 64 x 64 tiles of four 32 x 32 waves):
//                             forward: output pixel (2y+py, 2x+px) reads the 2x2 input neighbourhood (y-1+py+ty, x-1+px+tx) with tap
//                               (ky, kx) = (3-py-2ty, 3-px-2tx) -- the four-phase form of eamm_deconv_api.hip, one parity class per
//                               block, M = B*H*W, N = Cout, K = 4 taps x Cin; nothing is zero-stuffed;
//                             data gradient: dX[y,x] = sum over the 16 taps of dY[2y+ky-1, 2x+kx-1] W[:, :, ky, kx]^T: a 4x4 stride-2
//                               pad-1 convolution of dY, a gather per input pixel, M = B*H*W, N = Cin, K = 16 taps x Cout.
//                           Both read their filter from an image packed on the device by deconv4s2_pack_kernel.
//   deconv4s2_wgrad         dW[ci,co,ky,kx] = sum_p X[p][ci] dY[2p + (ky,kx) - 1][co]: conv_s2_backward.hip's stride-2 weight
//                           gradient with the operands' roles swapped and 16 taps, the pixel-split slabs summed in slice order.
//   deconv4s2_bias_grad     db[co] = sum_p dY[p][co], row lanes in a fixed order, the fold in double.
#include "conv_common.h"

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

struct T4WgradArgs {
    const float* x;      // [B,H,W,Cin]
    const float* dy;     // [B,2H,2W,Cout]
    int H, W, Cin, Cout;
    int P;               // B*H*W
    int per_split, splits, mt, nt;
    float* partial;      // [splits][16][mt*64 ci][nt*64 co]
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
    constexpr int A_PER = BM / 32, B_PER = BN / 32;
    __shared__ __attribute__((aligned(16))) float As[2 * BM * LDK];
    __shared__ __attribute__((aligned(16))) float Bs[2 * BN * LDK];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, half = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;

    int L = blockIdx.x;
    const int ntile = L % p.ntiles;
    L /= p.ntiles;
    const int mtile = L % p.mtiles;
    L /= p.mtiles;
    const int cls = L, py = cls >> 1, px = cls & 1;
    const int mbase = mtile * BM;
    const int ncc = p.Cs / BK, nchunks = NTAP * ncc;
    const int Hs = FWD ? p.H : 2 * p.H, Ws = FWD ? p.W : 2 * p.W;   // the source map

    // operand loader: this thread stages rows arow + 32 j, 16 bytes at column acol; (qy, qx) = the source pixel of tap (0, 0)
    const int arow = tid >> 3, acol = (tid & 7) * 4;
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
    const __amdgpu_buffer_rsrc_t rs0 = __builtin_amdgcn_make_buffer_rsrc((void*)p.src, 0, p.src_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsw = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, p.w_bytes, 0x00020000);
    constexpr unsigned OOB = 0xFFFFFFF0u;
    const int wtile = (ntile * (FWD ? 4 : 1) + cls) * nchunks;

    u32x4 av[A_PER], bv[B_PER];
    auto load_chunk = [&](int ci) {
        const int tap = ci / ncc, cc = ci - tap * ncc;
        const int ty = FWD ? tap >> 1 : tap >> 2, tx = FWD ? tap & 1 : tap & 3;
        const int coff = cc * BK + acol;
#pragma unroll
        for (int j = 0; j < A_PER; ++j) {
            const int yy = qy[j] + ty, xx = qx[j] + tx;
            const bool ok = ((unsigned)yy < (unsigned)Hs) & ((unsigned)xx < (unsigned)Ws);
            const unsigned off = ok ? (unsigned)((qb[j] + yy * Ws + xx) * p.Cs + coff) * 4u : OOB;
            av[j] = __builtin_amdgcn_raw_buffer_load_b128(rs0, off, 0, 0);
        }
        const unsigned woff = (unsigned)((wtile + ci) * (BN * BK) + tid * 4) * 4u;
#pragma unroll
        for (int j = 0; j < B_PER; ++j) bv[j] = __builtin_amdgcn_raw_buffer_load_b128(rsw, woff + j * 4096u, 0, 0);
    };
    auto store_chunk = [&](int st) {
        float* a = As + st * BM * LDK + arow * LDK + acol;
#pragma unroll
        for (int j = 0; j < A_PER; ++j) *reinterpret_cast<u32x4*>(a + j * 32 * LDK) = av[j];
        float* b = Bs + st * BN * LDK + arow * LDK + acol;
#pragma unroll
        for (int j = 0; j < B_PER; ++j) *reinterpret_cast<u32x4*>(b + j * 32 * LDK) = bv[j];
    };

    f32x16 acc;
    static_for<16>([&](auto rc) { acc[decltype(rc)::value] = 0.f; });
    auto compute = [&](int st) {
        const float* a_base = As + st * BM * LDK + (wm * 32 + l31) * LDK + half * 4;
        const float* b_base = Bs + st * BN * LDK + (wn * 32 + l31) * LDK + half * 4;
#pragma unroll
        for (int s = 0; s < BK / 8; ++s) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(a_base + s * 8);
            const f32x4 b = *reinterpret_cast<const f32x4*>(b_base + s * 8);
#pragma unroll
            for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], b[t], acc, 0, 0, 0);
        }
    };

    load_chunk(0);
    store_chunk(0);
    __syncthreads();
    int st = 0;
    for (int ci = 0; ci < nchunks; ++ci) {
        const bool more = ci + 1 < nchunks;
        if (more) load_chunk(ci + 1);
        compute(st);
        if (more) store_chunk(st ^ 1);
        __syncthreads();
        st ^= 1;
    }

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
            if (FWD) p.out[(((size_t)b * 2 * p.H + 2 * y + py) * 2 * p.W + 2 * x + px) * p.N + n] = acc[r] + bias;
            else p.out[(size_t)m * p.N + n] = acc[r];
        }
    });
}

// block (N tile, M tile, tap, split): D[64 ci][64 co] = sum over the split's input pixels, 4 waves of 32 x 32
__global__ __launch_bounds__(256) void deconv4s2_wgrad_kernel(const T4WgradArgs p) {
    constexpr int KC = 32, TM = 64, TN = 64, LD = TM + 4;
    __shared__ __attribute__((aligned(16))) float As[KC * LD];
    __shared__ __attribute__((aligned(16))) float Bs[KC * LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    int L = blockIdx.x;
    const int nti = L % p.nt; L /= p.nt;
    const int mti = L % p.mt; L /= p.mt;
    const int tap = L % 16; L /= 16;
    const int split = L;
    const int ky = tap >> 2, kx = tap & 3;
    const int p0 = split * p.per_split, p1 = min(p.P, p0 + p.per_split);
    const int Ho = 2 * p.H, Wo = 2 * p.W;
    f32x16 acc;
    static_for<16>([&](auto rc) { acc[decltype(rc)::value] = 0.f; });
    // loader: thread -> (rows lr and lr + 16 of the chunk, 16-byte group lq of the tile's 64 channels)
    const int lq = tid & 15, lr = tid >> 4;
    const int ci = mti * TM + lq * 4, co = nti * TN + lq * 4;
    const bool ci_ok = ci < p.Cin, co_ok = co < p.Cout;
    f32x4 ra[2], rb[2];
    auto fetch = [&](int pc) {
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
            const int pp = pc + lr + 16 * h2;
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            ra[h2] = z;
            rb[h2] = z;
            if (pp < p1) {
                const int x = pp % p.W, t = pp / p.W;
                const int y = t % p.H, b = t / p.H;
                const int oy = 2 * y + ky - 1, ox = 2 * x + kx - 1;
                if (ci_ok) ra[h2] = *reinterpret_cast<const f32x4*>(p.x + (size_t)pp * p.Cin + ci);
                if (co_ok && (unsigned)oy < (unsigned)Ho && (unsigned)ox < (unsigned)Wo)
                    rb[h2] = *reinterpret_cast<const f32x4*>(p.dy + (((size_t)b * Ho + oy) * Wo + ox) * p.Cout + co);
            }
        }
    };
    if (p0 < p1) fetch(p0);
    for (int pc = p0; pc < p1; pc += KC) {
        __syncthreads();
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
            *reinterpret_cast<f32x4*>(As + (lr + 16 * h2) * LD + lq * 4) = ra[h2];
            *reinterpret_cast<f32x4*>(Bs + (lr + 16 * h2) * LD + lq * 4) = rb[h2];
        }
        __syncthreads();
        if (pc + KC < p1) fetch(pc + KC);
#pragma unroll
        for (int s = 0; s < KC / 2; ++s) {   // A[m][k]: lane -> m = lane % 32, k = lane / 32
            const float av = As[(2 * s + (lane >> 5)) * LD + wm * 32 + (lane & 31)];
            const float bv = Bs[(2 * s + (lane >> 5)) * LD + wn * 32 + (lane & 31)];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
        }
    }
    float* out = p.partial + (((size_t)split * 16 + tap) * (p.mt * TM) + mti * TM + wm * 32) * (size_t)(p.nt * TN) + nti * TN + wn * 32;
    static_for<16>([&](auto rc) {
        constexpr int r = decltype(rc)::value;
        const int m = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        out[(size_t)m * (p.nt * TN) + (lane & 31)] = acc[r];
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
size_t t4_round64(size_t n) { return (n + 63) / 64 * 64; }
size_t t4_packed_elems(int Cin, int Cout, bool fwd) {   // 16 (class, tap) pairs either way
    return fwd ? (size_t)((Cout + 63) / 64) * 16 * (Cin / 32) * 64 * 32 : (size_t)((Cin + 63) / 64) * 16 * (Cout / 32) * 64 * 32;
}
int t4_wgrad_splits(int tiles, int P) { return std::max(1, std::min(1024 / std::max(1, tiles) + 1, P / 64)); }
}  // namespace

size_t deconv4s2_workspace_floats(int B, int H, int W, int Cin, int Cout, int which) {
    if (!t4_shape_ok(B, H, W, Cin, Cout)) return 0;
    if (which == 0 || which == 1) return t4_round64(t4_packed_elems(Cin, Cout, which == 0));
    if (which != 2) return 0;
    const int mt = (Cin + 63) / 64, nt = (Cout + 63) / 64;
    return t4_round64((size_t)t4_wgrad_splits(mt * nt * 16, B * H * W) * 16 * mt * 64 * nt * 64);
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
    T4WgradArgs a{};
    a.x = x;
    a.dy = dy;
    a.H = H;
    a.W = W;
    a.Cin = Cin;
    a.Cout = Cout;
    a.P = B * H * W;
    a.mt = (Cin + 63) / 64;
    a.nt = (Cout + 63) / 64;
    const int tiles = a.mt * a.nt * 16;
    const int splits = t4_wgrad_splits(tiles, a.P);
    a.per_split = ((a.P + splits - 1) / splits + 31) / 32 * 32;
    a.splits = (a.P + a.per_split - 1) / a.per_split;   // <= splits: the workspace holds them
    a.partial = workspace;
    note_mfma_flops(2.0 * 16 * (double)a.splits * a.per_split * (a.mt * 64.0) * (a.nt * 64.0));
    hipLaunchKernelGGL(deconv4s2_wgrad_kernel, dim3((unsigned)(tiles * a.splits)), dim3(256), 0, s, a);
    // the reduce writes [rows][columns][taps] = [Cin][Cout][4][4]: the reference's ConvTranspose2d layout
    if (hipError_t e = conv_wgrad_reduce_launch(workspace, a.splits, 16, a.mt * 64, a.nt * 64, Cin, Cout, dweight, s); e != hipSuccess) return e;
    if (dbias) {
        hipLaunchKernelGGL(deconv4s2_bias_grad_kernel, dim3((Cout + 31) / 32), dim3(256), 0, s, dy, 4ll * a.P, Cout, dbias);
        return hipGetLastError();
    }
    return hipSuccess;
}

}  // namespace eamm
