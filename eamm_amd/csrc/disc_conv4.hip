// The discriminator's convolution (reference modules/discriminator.py:14: nn.Conv2d(kernel_size=4), no padding, stride 1) on NHWC
// fp32 maps with an OIHW device filter: forward, data gradient and weight gradient.
//
//   * disc_conv4_kernel -- out[B,H+2pad-3,W+2pad-3,N] = valid 4x4 correlation of x zero-padded by `pad`.  pad = 0 is the forward;
//     pad = 3 on conv_pack_dev's `transposed` image (out / in swapped, taps flipped) is the data gradient.  An implicit GEMM with
//     M = the output pixels in raster order, N = the output channels, K = 16 taps x Cin / 32 chunks on conv_gather_gemm.h's loop
//     (v_mfma_f32_32x32x2_f32); the padding ring and the M tail are buffer offsets of GG_OOB, which read zeros: the loop has no
//     branch.  Tiles: 128 x 64 where N is a multiple of 64 (2 x 2 waves of 64 x 32; LDS 2 x (128 + 64) rows x 36 floats = 54 KiB,
//     two workgroups per CU), else 128 x 32 (4 x 1 waves).  The LDS row stride of CONV_LDK = 36 floats keeps the loop's ds_read_b128
//     of 32 consecutive rows conflict-free (conv_gather_gemm.h).
//   * the THIN form (CP = 4 | 8 | 16 floats per input pixel: the image, or the image with the key-point heat maps, zero-padded to
//     CP channels): the kx taps of one filter row are contiguous in such a map, so a 32-wide K chunk is 32 / CP consecutive taps
//     -- K = 16 CP instead of 16 x 32 -- and off(j) of the gather protocol depends on the thread's column acol.  Its filter image
//     is disc_pack_thin_kernel's: k = tap * CP + c, channels at and above the filter's own count packed as zeros.
//   * the weight gradient dW[co][ci][ky][kx] = sum_p dY[p][co] X[p + (ky, kx)][ci] is backward.hip's strided_wgrad_kernel with stride
//     1, pad 0 (dense = dY, gathered = X) and the bias gradient its conv_bias_grad kernels: pixel-split slabs summed in slice order.
// No float atomics: every element is written once, the same bits on every run.
#include "conv_gather_gemm.h"

#include <algorithm>

namespace eamm {

namespace {

struct Conv4Args {
    const float* x;      // [B,H,W,Cx]
    const float* w;      // packed filter image [ntiles][nchunks][BN][32]
    const float* bias;   // [>= N] or null
    float* out;          // [B,Ho,Wo,N]
    int H, W, Cx;        // Cx: floats per input pixel
    int Ho, Wo, N, pad;  // N: floats per output pixel (columns stored)
    int M;               // B*Ho*Wo
    int ntiles, nchunks;
    unsigned x_bytes, w_bytes;
};

}  // namespace

// block (M tile, N tile), N fastest: neighbouring blocks share their A rows in L2
template <int MT, int NT, int WM, int WN, int CP>
__global__ __launch_bounds__(256) void disc_conv4_kernel(const Conv4Args p) {
    constexpr int BM = WM * MT * 32, BN = WN * NT * 32, BK = CONV_BK, LDK = CONV_LDK;
    constexpr int A_PER = BM / 32;
    __shared__ __attribute__((aligned(16))) float As[2 * BM * LDK];
    __shared__ __attribute__((aligned(16))) float Bs[2 * BN * LDK];

    const GatherLanes g = gather_lanes<WN>(threadIdx.x);
    const int ntile = blockIdx.x % p.ntiles, mtile = blockIdx.x / p.ntiles;
    const int mbase = mtile * BM;

    // the rows arow + 32 j this thread stages: the output pixel's top-left input coordinate and its image's first pixel
    int iy[A_PER], ix[A_PER], ib[A_PER];
#pragma unroll
    for (int j = 0; j < A_PER; ++j) {
        const int m = mbase + g.arow + 32 * j;
        if (m < p.M) {
            ix[j] = m % p.Wo - p.pad;
            const int t = m / p.Wo;
            iy[j] = t % p.Ho - p.pad;
            ib[j] = (t / p.Ho) * p.H * p.W;
        } else {
            iy[j] = 1 << 20;   // never inside the map
            ix[j] = 0;
            ib[j] = 0;
        }
    }
    const __amdgpu_buffer_rsrc_t rsx = gather_rsrc(p.x, p.x_bytes);
    const __amdgpu_buffer_rsrc_t rsw = gather_rsrc(p.w, p.w_bytes);
    const int wtile = ntile * p.nchunks;
    const int acol = g.acol;

    // chunk ci: ordinary form (channel chunk cc, tap) as conv_pack_dev orders them; thin form k = ci * 32 + acol = tap * CP + c
    auto chunk = [&](int ci) {
        int tap, coff;
        if constexpr (CP == 0) {
            tap = ci & 15;
            coff = (ci >> 4) * BK + acol;
        } else {
            const int k = ci * BK + acol;
            tap = k / CP;
            coff = k % CP;
        }
        const int ky = tap >> 2, kx = tap & 3;
        return gather_chunk(rsx, [&, ky, kx, coff](int j) {
            const int yy = iy[j] + ky, xx = ix[j] + kx;
            const bool ok = ((unsigned)yy < (unsigned)p.H) & ((unsigned)xx < (unsigned)p.W);
            return ok ? (unsigned)((ib[j] + yy * p.W + xx) * p.Cx + coff) * 4u : GG_OOB;
        }, wtile + ci);
    };

    f32x16 acc[MT][NT];
    gather_gemm<MT, NT, WM, WN>(acc, As, Bs, rsw, g, 0, p.nchunks, chunk);

    // D layout: lane -> column n = lane % 32; register r -> row (r % 4) + 8 (r / 4) + 4 (lane / 32)
    static_for<MT>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        static_for<NT>([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            const int n = ntile * BN + (g.wn * NT + j) * 32 + g.l31;
            const bool nok = n < p.N;
            const float bias = (p.bias != nullptr && nok) ? p.bias[n] : 0.f;
            static_for<16>([&](auto rc) {
                constexpr int r = decltype(rc)::value;
                const int m = mbase + (g.wm * MT + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * g.half;
                if (nok && m < p.M) p.out[(size_t)m * p.N + n] = acc[i][j][r] + bias;
            });
        });
    });
}

// the thin form's filter image from OIHW w [Cout][Cw][4][4]: [ntiles][16 CP / 32][BN][32], k = tap * CP + c, zeros for c >= Cw
__global__ __launch_bounds__(256) void disc_pack_thin_kernel(const float* __restrict__ w, int Cout, int Cw, int CP, int BN,
                                                             float* __restrict__ dst, int total) {
    const int nchunks = 16 * CP / CONV_BK;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int kl = idx % CONV_BK, nl = (idx / CONV_BK) % BN;
        const int ci = (idx / (CONV_BK * BN)) % nchunks, nt = idx / (CONV_BK * BN * nchunks);
        const int k = ci * CONV_BK + kl, tap = k / CP, c = k % CP, o = nt * BN + nl;
        dst[idx] = (o < Cout && c < Cw) ? w[((size_t)o * Cw + c) * 16 + tap] : 0.f;
    }
}

namespace {

struct Conv4Plan {
    int BN, ntiles, nchunks, Nstore, Cx;
    size_t packed;
};

// thin = 0: x [.,Cin], N = Cout columns.  thin = CP forward (transposed = 0): x [.,CP], the filter has Cin <= CP channels.
// thin = CP data gradient (transposed = 1): x = dY [.,Cin], the Cout <= CP real columns are stored with a pixel stride of CP.
Conv4Plan conv4_plan(int Cin, int Cout, int transposed, int thin) {
    Conv4Plan P;
    const bool thin_fwd = thin && !transposed;
    P.Nstore = (thin && transposed) ? thin : Cout;
    P.Cx = thin_fwd ? thin : Cin;
    P.BN = P.Nstore % 64 == 0 ? 64 : 32;
    P.ntiles = (P.Nstore + P.BN - 1) / P.BN;
    P.nchunks = thin_fwd ? 16 * thin / CONV_BK : 16 * (Cin / CONV_BK);
    P.packed = (size_t)P.ntiles * P.nchunks * P.BN * CONV_BK;
    return P;
}

template <int CP>
void conv4_run(const Conv4Args& a, int BN, unsigned blocks, hipStream_t s) {
    if (BN == 64) hipLaunchKernelGGL((disc_conv4_kernel<2, 1, 2, 2, CP>), dim3(blocks), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((disc_conv4_kernel<1, 1, 4, 1, CP>), dim3(blocks), dim3(256), 0, s, a);
}

}  // namespace

// Why a shape is refused (null: it is not).  The entry and the workspace query share it.
const char* disc_conv4_refusal(int B, int H, int W, int Cin, int Cout, int pad, int transposed, int thin) {
    if (B < 1) return "B must be positive";
    if (pad != 0 && pad != 3) return "pad must be 0 (forward) or 3 (data gradient)";
    if (H < 1 || W < 1 || (pad == 0 && (H < 4 || W < 4))) return "H and W must be at least 4 (the filter is 4 x 4, without padding)";
    if ((pad == 3) != (transposed != 0)) return "pad = 3 goes with transposed = 1 (the data gradient), pad = 0 with transposed = 0";
    if (thin != 0 && thin != 4 && thin != 8 && thin != 16) return "thin must be 0, 4, 8 or 16 floats per pixel";
    if (!thin && (Cin < CONV_BK || Cin % CONV_BK)) return "Cin must be a multiple of 32";
    if (!thin && (Cout < CONV_BK || Cout % CONV_BK)) return "Cout must be a multiple of 32";
    if (thin && !transposed && (Cin < 1 || Cin > thin)) return "thin forward: Cin (the filter's channels) must be 1 .. thin";
    if (thin && !transposed && (Cout < CONV_BK || Cout % CONV_BK)) return "Cout must be a multiple of 32";
    if (thin && transposed && (Cin < CONV_BK || Cin % CONV_BK)) return "thin data gradient: Cin (grad_out's channels) must be a multiple of 32";
    if (thin && transposed && (Cout < 1 || Cout > thin)) return "thin data gradient: Cout (the filter's channels) must be 1 .. thin";
    const Conv4Plan P = conv4_plan(Cin, Cout, transposed, thin);
    const unsigned long long Ho = H + 2 * pad - 3, Wo = W + 2 * pad - 3;
    // 32-bit byte offsets in the buffer descriptors, 32-bit pixel counts in the kernel
    if ((unsigned long long)B * H * W * P.Cx * sizeof(float) >= 0xFFFFFFF0ull || (unsigned long long)B * Ho * Wo * P.Nstore >= (1ull << 31) ||
        (unsigned long long)P.packed * sizeof(float) >= 0xFFFFFFF0ull)
        return "tensor too large (4 GiB of input, 2^31 output elements)";
    return nullptr;
}

size_t disc_conv4_workspace_floats(int B, int H, int W, int Cin, int Cout, int pad, int transposed, int thin) {
    if (disc_conv4_refusal(B, H, W, Cin, Cout, pad, transposed, thin)) return 0;
    return round64(conv4_plan(Cin, Cout, transposed, thin).packed);
}

hipError_t disc_conv4_launch(const float* x, int B, int H, int W, int Cin, const float* weight, const float* bias, int Cout, int pad,
                             int transposed, int thin, float* out, float* workspace, hipStream_t s) {
    if (disc_conv4_refusal(B, H, W, Cin, Cout, pad, transposed, thin)) return hipErrorInvalidValue;
    const Conv4Plan P = conv4_plan(Cin, Cout, transposed, thin);
    const bool thin_fwd = thin && !transposed;
    if (thin_fwd) {
        const int total = (int)P.packed;
        hipLaunchKernelGGL(disc_pack_thin_kernel, dim3(std::min((total + 255) / 256, 1 << 16)), dim3(256), 0, s, weight, Cout, Cin, thin, P.BN,
                           workspace, total);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    } else {
        // N = Cout (zeros in the image's columns Cout .. ntiles * BN), K = 16 taps x Cin
        if (hipError_t e = conv_pack_dev_launch(weight, Cout, Cin, 16, P.BN, transposed, workspace, s); e != hipSuccess) return e;
    }
    Conv4Args a{};
    a.x = x;
    a.w = workspace;
    a.bias = bias;
    a.out = out;
    a.H = H;
    a.W = W;
    a.Cx = P.Cx;
    a.Ho = H + 2 * pad - 3;
    a.Wo = W + 2 * pad - 3;
    a.N = P.Nstore;
    a.pad = pad;
    a.M = B * a.Ho * a.Wo;
    a.ntiles = P.ntiles;
    a.nchunks = P.nchunks;
    a.x_bytes = (unsigned)((size_t)B * H * W * P.Cx * sizeof(float));
    a.w_bytes = (unsigned)(P.packed * sizeof(float));
    const long long mtiles = (a.M + 127) / 128, blocks = mtiles * P.ntiles;
    if (blocks > 0x7FFFFFFFll) return hipErrorInvalidValue;
    note_mfma_flops(2.0 * P.nchunks * CONV_BK * (double)mtiles * 128.0 * (double)P.ntiles * P.BN);   // executed, on whole tiles
    if (!thin_fwd) conv4_run<0>(a, P.BN, (unsigned)blocks, s);
    else if (thin == 4) conv4_run<4>(a, P.BN, (unsigned)blocks, s);
    else if (thin == 8) conv4_run<8>(a, P.BN, (unsigned)blocks, s);
    else conv4_run<16>(a, P.BN, (unsigned)blocks, s);
    return hipGetLastError();
}

// ---- weight and bias gradient --------------------------------------------------------------------------------------------------
// x [B,H,W,Cx], dy [B,H-3,W-3,Cout] -> dweight [Cout][Cx][4][4] (or null), dbias [Cout] (or null).  Cx: 4 | 8 | 16 (thin) or a multiple of 32.
const char* disc_conv4_wgrad_refusal(int B, int H, int W, int Cx, int Cout) {
    if (B < 1) return "B must be positive";
    if (H < 4 || W < 4) return "H and W must be at least 4 (the filter is 4 x 4, without padding)";
    if (Cx != 4 && Cx != 8 && Cx != 16 && (Cx < CONV_BK || Cx % CONV_BK)) return "Cin must be 4, 8, 16 (thin) or a multiple of 32";
    if (Cout < CONV_BK || Cout % CONV_BK || Cout > 1024) return "Cout must be a multiple of 32, at most 1024";
    if ((unsigned long long)B * H * W * std::max(Cx, Cout) >= (1ull << 31)) return "tensor too large (2^31 elements)";
    return nullptr;
}

size_t disc_conv4_wgrad_workspace_floats(int B, int H, int W, int Cx, int Cout) {
    if (disc_conv4_wgrad_refusal(B, H, W, Cx, Cout)) return 0;
    return strided_wgrad_workspace_floats(B * (H - 3) * (W - 3), Cout, Cx, 4) + round64(conv_bias_grad_workspace_floats(Cout));
}

hipError_t disc_conv4_wgrad_launch(const float* x, const float* dy, int B, int H, int W, int Cx, int Cout, float* dweight, float* dbias,
                                   float* workspace, hipStream_t s) {
    if (disc_conv4_wgrad_refusal(B, H, W, Cx, Cout)) return hipErrorInvalidValue;
    const int Ho = H - 3, Wo = W - 3;
    if (dweight != nullptr)   // (null: the bias gradient alone, for a frozen filter with a trainable bias)
        if (hipError_t e = strided_wgrad_launch(dy, x, B, Ho, Wo, Cout, Cx, 4, 0, dweight, workspace, s, 1, H, W); e != hipSuccess) return e;
    if (dbias == nullptr) return hipSuccess;
    return conv_bias_grad_launch(dy, (long long)B * Ho * Wo, Cout, dbias, workspace + strided_wgrad_workspace_floats(B * Ho * Wo, Cout, Cx, 4), s);
}

}  // namespace eamm
