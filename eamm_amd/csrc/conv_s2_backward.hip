// Backward of the stride-2 KSxKS convolution of conv_s2.hip (KS 1 or 3, pad KS/2, NHWC fp32, OIHW filter, no bias): what makes
// Emotion_k's ResNet-18 trunk trainable (reference modules/util.py:1069-1099: the first 3x3 convolution of a down-sampling
// BasicBlock and its 1x1 `downsample` shortcut; model.py:312-413 back-propagates the second stage's losses into them).
//
//   * conv_s2_dgrad_kernel -- dX [B,Hin,Win,Cin] from dY [B,Hin/2,Win/2,Cout] as a GATHER.  Output pixel (oy, ox) read input pixel
//     (2 oy + ky - KS/2, 2 ox + kx - KS/2), so an input pixel's parity (iy & 1, ix & 1) fixes which taps reach it: with KS = 3 an
//     even coordinate is reached by the centre tap only (from o = i / 2), an odd one by tap 0 (from o = (i + 1) / 2, if it exists)
//     and tap 2 (from o = (i - 1) / 2) -- 1, 2, 2 or 4 of the nine taps per class; with KS = 1 only the even / even pixels are
//     reached.  Each class is an implicit GEMM on v_mfma_f32_32x32x2_f32 with M = the B * Hin/2 * Win/2 pixels of the class, N = Cin,
//     K = (taps of the class) x Cout: the forward's 9 taps per 4 input pixels of multiplies (a zero-inserted dY through a stride-1
//     kernel would do four times that).  The main loop is conv_gather_gemm.h's; this kernel supplies the class's tap list, the dY row
//     offsets and its scatter of the class back into dX.  The filter is conv_pack_dev's `transposed` image
//     ([Cin tiles][Cout/32 x taps][BN][32], taps flipped), of which a class reads its own chunks.  No atomics: every element of dX
//     is written once, the exact zeros of a 1x1's odd pixels included.
//   * the weight gradient dW[co][ci][ky][kx] = sum_p dY[p][co] X[2 p + (ky, kx) - KS/2][ci] is backward.hip's strided_wgrad_kernel with
//     dY as its dense and X as its gathered operand (strided_wgrad_launch).
#include "conv_gather_gemm.h"

#include <algorithm>

namespace eamm {

namespace {

constexpr int DG_BM = 64, DG_BN = 64;   // 4 waves of one 32 x 32 tile each

struct S2DgradArgs {
    const float* dy;   // [B,Ho,Wo,Cout]
    const float* w;    // conv_pack_dev_launch(weight, N = Cin, K = Cout, T, BN = 64, transposed = 1)
    float* dx;         // [B,2Ho,2Wo,Cin]
    int B, Ho, Wo, Cin, Cout;
    int M;             // B*Ho*Wo: the pixels of one parity class
    int mtiles, ntiles;
    unsigned dy_bytes, w_bytes;
};

}  // namespace

// block (class, M tile, N tile); class = 2 (iy & 1) + (ix & 1)
template <int KS>
__global__ __launch_bounds__(256) void conv_s2_dgrad_kernel(const S2DgradArgs p) {
    constexpr int BM = DG_BM, BN = DG_BN, BK = CONV_BK, LDK = CONV_LDK, T = KS * KS;
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
    const int py = L >> 1, px = L & 1;
    const int mbase = mtile * BM;
    // taps of this class: KS = 3 -> (1 + py) x (1 + px); KS = 1 -> one for the even / even class, none for the others
    const int ny = KS == 3 ? 1 + py : (py == 0), nx = KS == 3 ? 1 + px : (px == 0);
    const int ntap = ny * nx;
    const int nchunks = ntap * (p.Cout / BK);

    // operand loader: (qy, qx) = the pixel's index inside its class, for the rows arow + 32 j that this thread stages
    const int arow = g.arow, acol = g.acol;
    int qy[A_PER], qx[A_PER], qb[A_PER];
#pragma unroll
    for (int j = 0; j < A_PER; ++j) {
        const int m = mbase + arow + 32 * j;
        if (m < p.M) {
            qx[j] = m % p.Wo;
            const int t = m / p.Wo;
            qy[j] = t % p.Ho;
            qb[j] = (t / p.Ho) * p.Ho * p.Wo;
        } else {
            qy[j] = 1 << 20;   // never inside the map
            qx[j] = 0;
            qb[j] = 0;
        }
    }
    const __amdgpu_buffer_rsrc_t rs0 = gather_rsrc(p.dy, p.dy_bytes);
    const __amdgpu_buffer_rsrc_t rsw = gather_rsrc(p.w, p.w_bytes);
    const int wtile = ntile * T * (p.Cout / BK);

    // chunk ci = (channel chunk cc, tap (jy, jx) of the class).  Odd coordinate: tap 0 comes from the NEXT output pixel, tap 2 from
    // this one; even coordinate: the centre tap
    auto chunk = [&](int ci) {
        const int cc = ci / ntap, tj = ci - cc * ntap;
        const int jy = tj / nx, jx = tj - jy * nx;
        int ky = 0, kx = 0, oy = 0, ox = 0;
        if (KS == 3) {
            ky = py ? 2 * jy : 1;
            kx = px ? 2 * jx : 1;
            oy = (py && jy == 0) ? 1 : 0;
            ox = (px && jx == 0) ? 1 : 0;
        }
        const int coff = cc * BK + acol;
        // the transposed image keeps forward tap t in chunk cc * T + (T - 1 - t)
        return gather_chunk(rs0, [&, oy, ox, coff](int j) {
            const int yy = qy[j] + oy, xx = qx[j] + ox;
            const bool ok = (yy < p.Ho) & (xx < p.Wo);
            return ok ? (unsigned)((qb[j] + yy * p.Wo + xx) * p.Cout + coff) * 4u : GG_OOB;
        }, wtile + cc * T + (T - 1 - (ky * KS + kx)));
    };

    f32x16 acc[1][1];
    gather_gemm<1, 1, 2, 2>(acc, As, Bs, rsw, g, 0, nchunks, chunk);

    // D layout: lane -> column n = lane % 32; register r -> row (r % 4) + 8 (r / 4) + 4 (lane / 32)
    const int n = ntile * BN + wn * 32 + l31;
    if (n >= p.Cin) return;
    const int Hin = 2 * p.Ho, Win = 2 * p.Wo;
    static_for<16>([&](auto rc) {
        constexpr int r = decltype(rc)::value;
        const int m = mbase + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (m < p.M) {
            const int x = m % p.Wo, t = m / p.Wo;
            const int y = t % p.Ho, b = t / p.Ho;
            p.dx[(((size_t)b * Hin + 2 * y + py) * Win + 2 * x + px) * p.Cin + n] = acc[0][0][r];
        }
    });
}

namespace {
bool s2_shape_ok(int B, int Hin, int Win, int Cin, int Cout, int ks) {
    if (B < 1 || Hin < 2 || Win < 2 || (Hin & 1) || (Win & 1) || Cin < CONV_BK || Cout < CONV_BK || Cin % CONV_BK || Cout % CONV_BK) return false;
    if (ks != 1 && ks != 3) return false;
    // 32-bit element offsets in the kernels, 32-bit byte ranges in the buffer descriptors
    const unsigned long long big = std::max<unsigned long long>((unsigned long long)B * Hin * Win * Cin, (unsigned long long)B * (Hin / 2) * (Win / 2) * Cout);
    return big * sizeof(float) < 0xFFFFFFF0ull && (unsigned long long)9 * Cin * Cout * sizeof(float) < 0x7FFFFFF0ull;
}
}  // namespace

bool conv_s2_backward_supported(int B, int Hin, int Win, int Cin, int Cout, int ks) { return s2_shape_ok(B, Hin, Win, Cin, Cout, ks); }

size_t conv_s2_dgrad_workspace_floats(int B, int Hin, int Win, int Cin, int Cout, int ks) {
    if (!s2_shape_ok(B, Hin, Win, Cin, Cout, ks)) return 0;
    return round64(conv_packed_elems(ks * ks, Cout, Cin, DG_BN, 1));   // N = Cin tiles of 64, K = taps x Cout
}

hipError_t conv_s2_dgrad_launch(const float* dy, const float* weight, int B, int Hin, int Win, int Cin, int Cout, int ks, float* dx,
                                float* workspace, size_t workspace_floats, hipStream_t s) {
    const size_t need = conv_s2_dgrad_workspace_floats(B, Hin, Win, Cin, Cout, ks);
    if (need == 0 || workspace_floats < need || (reinterpret_cast<uintptr_t>(workspace) & 15)) return hipErrorInvalidValue;
    hipError_t e = conv_pack_dev_launch(weight, Cin, Cout, ks * ks, DG_BN, 1, workspace, s);
    if (e != hipSuccess) return e;
    S2DgradArgs a{};
    a.dy = dy;
    a.w = workspace;
    a.dx = dx;
    a.B = B;
    a.Ho = Hin / 2;
    a.Wo = Win / 2;
    a.Cin = Cin;
    a.Cout = Cout;
    a.M = B * a.Ho * a.Wo;
    a.mtiles = (a.M + DG_BM - 1) / DG_BM;
    a.ntiles = (Cin + DG_BN - 1) / DG_BN;
    a.dy_bytes = (unsigned)((size_t)a.M * Cout * sizeof(float));
    a.w_bytes = (unsigned)(conv_packed_elems(ks * ks, Cout, Cin, DG_BN, 1) * sizeof(float));
    const long long blocks = 4ll * a.mtiles * a.ntiles;
    if (blocks > 0x7FFFFFFFll) return hipErrorInvalidValue;
    // executed: per class (taps of the class) x Cout deep, on whole 64 x 64 tiles
    note_mfma_flops(2.0 * (ks == 3 ? 9.0 : 1.0) * Cout * (double)a.mtiles * DG_BM * (double)a.ntiles * DG_BN);
    if (ks == 3) hipLaunchKernelGGL(conv_s2_dgrad_kernel<3>, dim3((unsigned)blocks), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(conv_s2_dgrad_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

size_t conv_s2_wgrad_workspace_floats(int B, int Hin, int Win, int Cin, int Cout, int ks) {
    if (!s2_shape_ok(B, Hin, Win, Cin, Cout, ks)) return 0;
    return strided_wgrad_workspace_floats(B * (Hin / 2) * (Win / 2), Cout, Cin, ks);
}

hipError_t conv_s2_wgrad_launch(const float* x, const float* dy, int B, int Hin, int Win, int Cin, int Cout, int ks, float* dweight,
                                float* workspace, size_t workspace_floats, hipStream_t s) {
    const size_t need = conv_s2_wgrad_workspace_floats(B, Hin, Win, Cin, Cout, ks);
    if (need == 0 || workspace_floats < need || (reinterpret_cast<uintptr_t>(workspace) & 15)) return hipErrorInvalidValue;
    return strided_wgrad_launch(dy, x, B, Hin / 2, Win / 2, Cout, Cin, ks, ks / 2, dweight, workspace, s);   // OIHW
}

}  // namespace eamm
