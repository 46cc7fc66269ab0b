// Stride-2 KSxKS convolution (pad KS/2) on NHWC fp32 activations as an implicit GEMM on the CDNA4 matrix cores: the first
// 3x3 convolution of a down-sampling ResNet BasicBlock and its 1x1 `downsample` shortcut (reference modules/util.py:1069-1099,
// Emotion_k layer2..layer4, :1291-1305).
//
// The same GEMM as conv_mfma.hip's register-staged kernel -- M = B*Ho*Wo output pixels, N = Cout, K = taps * Cin, exact fp32
// via v_mfma_f32_32x32x2_f32 -- on the same main loop (conv_gather_gemm.h), with the stride in the row offsets that this kernel hands
// to it: output pixel (oy, ox) reads input pixel (2 oy + ky - KS/2, 2 ox + kx - KS/2), out of the image reads zero.  The weights are
// pack_conv's plain image ([ntiles][nchunks][BN][BK]), the epilogue (bias, residual, activation) and split-K slabs are
// conv_common.h's, so nothing of the stride-1 kernels changes.
//
// This file is the FORWARD (the engine's eamm_emo_detect and, on a filter packed on the device, the differentiable operator
// eamm_op_conv_s2); its data and weight gradients are conv_s2_backward.hip.
#include "conv_gather_gemm.h"

#include <algorithm>
#include <cstring>

namespace eamm {

template <int KS, int MT, int NT, int WM, int WN>
__global__ __launch_bounds__(256) void conv_s2_kernel(const ConvArgs p, int Hin, int Win) {
    constexpr int BM = WM * MT * 32, BN = WN * NT * 32;
    constexpr int BK = CONV_BK, LDK = CONV_LDK;
    constexpr int T = KS * KS;
    constexpr int A_PER = BM / 32;
    static_assert(WM * WN == 4, "4 waves per block");

    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                 // [2][BM][LDK]
    float* Bs = smem + 2 * BM * LDK;  // [2][BN][LDK]

    const GatherLanes g = gather_lanes<WN>(threadIdx.x);
    const int l31 = g.l31, half = g.half, wm = g.wm, wn = g.wn;

    int L = xcd_remap(blockIdx.x, gridDim.x);
    const int ntile = L % p.ntiles;
    L /= p.ntiles;
    const int mtile = L % p.mtiles;
    L /= p.mtiles;
    const int split = L;
    const int mbase = mtile * BM;
    const int c_begin = split * p.chunks_per_split;
    const int c_end = min(p.nchunks, c_begin + p.chunks_per_split);

    // operand loader: (ry, rx) = the input pixel of tap (0, 0) + pad for the rows arow + 32 j that this thread stages
    const int arow = g.arow, acol = g.acol;
    int ry[A_PER], rx[A_PER], rb[A_PER];
#pragma unroll
    for (int j = 0; j < A_PER; ++j) {
        const int m = mbase + arow + 32 * j;
        if (m < p.M) {
            int b, y, x;
            pix_decode(p, m, b, y, x);
            ry[j] = 2 * y;
            rx[j] = 2 * x;
            rb[j] = b * Hin * Win;
        } else {
            ry[j] = -(1 << 20);  // never inside the image
            rx[j] = 0;
            rb[j] = 0;
        }
    }

    const __amdgpu_buffer_rsrc_t rs0 = gather_rsrc(p.in0, p.in0_bytes);
    const __amdgpu_buffer_rsrc_t rsw = gather_rsrc(p.w, p.w_bytes);
    const int wtile = ntile * p.nchunks;

    auto chunk = [&](int ci) {
        const int cc = ci / T, tap = ci - cc * T;
        const int dy = tap / KS - KS / 2, dx = tap % KS - KS / 2;
        const int coff = cc * BK + acol;
        return gather_chunk(rs0, [&, dy, dx, coff](int j) {
            const int yy = ry[j] + dy, xx = rx[j] + dx;
            const bool ok = ((unsigned)yy < (unsigned)Hin) & ((unsigned)xx < (unsigned)Win);
            return ok ? (unsigned)((rb[j] + yy * Win + xx) * p.C0 + coff) * 4u : GG_OOB;
        }, wtile + ci);
    };

    f32x16 acc[MT][NT];
    gather_gemm<MT, NT, WM, WN>(acc, As, Bs, rsw, g, c_begin, c_end, chunk);

    conv_epilogue<MT, NT, BN>(p, acc, mbase, ntile, wm, wn, l31, half, 0, split);
}

// split-K: the slabs summed in slice order (fixed, no atomics), then conv_common.h's epilogue
__global__ __launch_bounds__(256) void conv_s2_reduce_kernel(const ConvArgs p, int splits) {
    const size_t total = (size_t)p.M * p.Cout;
    const size_t slab = (size_t)p.Mpad * p.Npad;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int n = (int)(idx % p.Cout);
        const int r = (int)(idx / p.Cout);
        float s = 0.f;
        for (int sp = 0; sp < splits; ++sp) s += p.partial[(size_t)sp * slab + (size_t)r * p.Npad + n];
        int b, y, x;
        pix_decode(p, r, b, y, x);
        epilogue_store(p, 0, b, y, x, n, s + p.bias[n], 0.f, 0.f);
    }
}

template <int KS, int MT, int NT, int WM, int WN>
static hipError_t s2_cfg(const ConvArgs& a, int Hin, int Win, int blocks, hipStream_t stream) {
    constexpr int BM = WM * MT * 32, BN = WN * NT * 32;
    constexpr size_t lds = sizeof(float) * 2 * (BM + BN) * CONV_LDK;
    auto kern = conv_s2_kernel<KS, MT, NT, WM, WN>;
    static lds_once_mask configured{0};
    if (hipError_t e = ensure_dynamic_lds(kern, lds, &configured); e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), lds, stream, a, Hin, Win);
    return hipGetLastError();
}

template <int KS>
static hipError_t s2_tile(int BN, const ConvArgs& a, int Hin, int Win, int blocks, hipStream_t stream) {
    if (BN == 128) return s2_cfg<KS, 2, 2, 2, 2>(a, Hin, Win, blocks, stream);
    if (BN == 64) return s2_cfg<KS, 2, 1, 2, 2>(a, Hin, Win, blocks, stream);
    if (BN == 32) return s2_cfg<KS, 1, 1, 4, 1>(a, Hin, Win, blocks, stream);
    return hipErrorInvalidValue;
}

size_t conv_s2_partial_elems(const ConvLayer& L, int B, int Hin, int Win) {
    return conv_plan(L, B * (Hin / 2) * (Win / 2)).partial_elems;
}

hipError_t conv_s2_launch(const ConvLayer& L, const float* in, int B, int Hin, int Win, int act, const float* resid, float* out,
                          float* partial, size_t partial_cap, hipStream_t stream) {
    if (L.phase || L.dma_cfg || L.C1 || L.kh != L.kw || (L.kh != 1 && L.kh != 3) || (Hin & 1) || (Win & 1) || L.BM != 128)
        return hipErrorInvalidValue;
    ConvArgs a;
    std::memset(&a, 0, sizeof(a));
    a.in0 = in;
    a.C0 = L.C0;
    a.H = Hin / 2;
    a.W = Win / 2;
    a.nphase = 1;
    a.M = B * a.H * a.W;
    a.w = L.w;
    {   // buffer-descriptor ranges (32-bit)
        const size_t b0 = (size_t)B * Hin * Win * L.C0 * sizeof(float);
        const size_t bw = (size_t)L.ntiles * L.nchunks * L.BN * CONV_BK * sizeof(float);
        if (b0 >= 0xFFFFFFF0ull || bw >= 0xFFFFFFF0ull) return hipErrorInvalidValue;
        a.in0_bytes = (unsigned)b0;
        a.w_bytes = (unsigned)bw;
    }
    a.bias = L.bias;
    a.Cout = L.Cout;
    a.nchunks = L.nchunks;
    ConvPlan pl = conv_plan(L, a.M);
    while (pl.splits > 1 && pl.partial_elems > partial_cap) pl = conv_plan(L, a.M, pl.splits - 1);
    if (pl.splits > 1 && partial == nullptr) return hipErrorInvalidValue;
    a.mtiles = pl.mtiles;
    a.ntiles = pl.ntiles;
    a.chunks_per_split = pl.chunks_per_split;
    a.Mpad = pl.Mpad;
    a.Npad = pl.Npad;
    a.partial = pl.splits > 1 ? partial : nullptr;
    a.act = act;
    a.resid = resid;
    a.out = out;
    a.linear = ((a.H | a.W) & 1) ? 1 : 0;
    const int blocks = pl.mtiles * pl.ntiles * pl.splits;
    note_mfma_flops(2.0 * pl.mtiles * L.BM * (double)pl.ntiles * L.BN * (double)L.nchunks * CONV_BK);
    hipError_t e = L.kh == 3 ? s2_tile<3>(L.BN, a, Hin, Win, blocks, stream) : s2_tile<1>(L.BN, a, Hin, Win, blocks, stream);
    if (e != hipSuccess) return e;
    if (pl.splits > 1) {
        const size_t total = (size_t)a.M * L.Cout;
        const int rb = (int)std::min<size_t>((total + 255) / 256, 4096);
        hipLaunchKernelGGL(conv_s2_reduce_kernel, dim3(rb), dim3(256), 0, stream, a, pl.splits);
        e = hipGetLastError();
    }
    return e;
}

}  // namespace eamm
