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
//     kernel would do four times that).  The operand staging is conv_s2.hip's (raw buffer loads, an out-of-range offset reads
//     zero, LDS double buffer, one barrier per 32-channel chunk); the filter is conv_pack_dev's `transposed` image
//     ([Cin tiles][Cout/32 x taps][BN][32], taps flipped), of which a class reads its own chunks.  No atomics: every element of dX
//     is written once, the exact zeros of a 1x1's odd pixels included.
//   * conv_s2_wgrad_kernel -- dW[co][ci][ky][kx] = sum_p dY[p][co] X[2 p + (ky, kx) - KS/2][ci]: backward.hip's conv_wgrad_kernel
//     form, one GEMM per tap with M = Cout, N = Cin, K = the output pixels split over the pixel range, the stride in the X row
//     address (out-of-image rows are zeros), the slabs summed in slice order by backward.hip's conv_wgrad_reduce_kernel.
#include "conv_common.h"

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

struct S2WgradArgs {
    const float* x;    // [B,Hin,Win,Cin]
    const float* dy;   // [B,Ho,Wo,Cout]
    int Hin, Win, Ho, Wo, Cin, Cout, ks;
    int P;             // B*Ho*Wo
    int per_split;     // output pixels per split (a multiple of the 32-pixel chunk)
    int splits, mt, nt;
    float* partial;    // [splits][taps][mt*64][nt*64]
};

}  // namespace

// block (class, M tile, N tile); class = 2 (iy & 1) + (ix & 1)
template <int KS>
__global__ __launch_bounds__(256) void conv_s2_dgrad_kernel(const S2DgradArgs p) {
    constexpr int BM = DG_BM, BN = DG_BN, BK = CONV_BK, LDK = CONV_LDK, T = KS * KS;
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
    const int py = L >> 1, px = L & 1;
    const int mbase = mtile * BM;
    // taps of this class: KS = 3 -> (1 + py) x (1 + px); KS = 1 -> one for the even / even class, none for the others
    const int ny = KS == 3 ? 1 + py : (py == 0), nx = KS == 3 ? 1 + px : (px == 0);
    const int ntap = ny * nx;
    const int nchunks = ntap * (p.Cout / BK);

    // operand loader: this thread stages rows arow + 32 j, 16 bytes at column acol; (qy, qx) = the pixel's index inside its class
    const int arow = tid >> 3, acol = (tid & 7) * 4;
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
    const __amdgpu_buffer_rsrc_t rs0 = __builtin_amdgcn_make_buffer_rsrc((void*)p.dy, 0, p.dy_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsw = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, p.w_bytes, 0x00020000);
    constexpr unsigned OOB = 0xFFFFFFF0u;
    const int wtile = ntile * T * (p.Cout / BK);

    u32x4 av[A_PER], bv[B_PER];
    auto load_chunk = [&](int ci) {
        const int cc = ci / ntap, tj = ci - cc * ntap;
        const int jy = tj / nx, jx = tj - jy * nx;
        // odd coordinate: tap 0 comes from the NEXT output pixel, tap 2 from this one; even coordinate: the centre tap
        int ky = 0, kx = 0, oy = 0, ox = 0;
        if (KS == 3) {
            ky = py ? 2 * jy : 1;
            kx = px ? 2 * jx : 1;
            oy = (py && jy == 0) ? 1 : 0;
            ox = (px && jx == 0) ? 1 : 0;
        }
        const int coff = cc * BK + acol;
#pragma unroll
        for (int j = 0; j < A_PER; ++j) {
            const int yy = qy[j] + oy, xx = qx[j] + ox;
            const bool ok = (yy < p.Ho) & (xx < p.Wo);
            const unsigned off = ok ? (unsigned)((qb[j] + yy * p.Wo + xx) * p.Cout + coff) * 4u : OOB;
            av[j] = __builtin_amdgcn_raw_buffer_load_b128(rs0, off, 0, 0);
        }
        // the transposed image keeps forward tap t in chunk cc * T + (T - 1 - t)
        const int wchunk = cc * T + (T - 1 - (ky * KS + kx));
        const unsigned woff = (unsigned)((wtile + wchunk) * (BN * BK) + tid * 4) * 4u;
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

    if (nchunks > 0) {
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
    }

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
            p.dx[(((size_t)b * Hin + 2 * y + py) * Win + 2 * x + px) * p.Cin + n] = acc[r];
        }
    });
}

// block (N tile, M tile, tap, split): D[64 co][64 ci] = sum over the split's output pixels, 4 waves of 32 x 32
__global__ __launch_bounds__(256) void conv_s2_wgrad_kernel(const S2WgradArgs p) {
    constexpr int KC = 32, TM = 64, TN = 64, LD = TM + 4;
    __shared__ __attribute__((aligned(16))) float As[KC * LD];
    __shared__ __attribute__((aligned(16))) float Bs[KC * LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    int L = blockIdx.x;
    const int nti = L % p.nt; L /= p.nt;
    const int mti = L % p.mt; L /= p.mt;
    const int taps = p.ks * p.ks;
    const int tap = L % taps; L /= taps;
    const int split = L;
    const int dyo = tap / p.ks - p.ks / 2, dxo = tap % p.ks - p.ks / 2;
    const int p0 = split * p.per_split, p1 = min(p.P, p0 + p.per_split);
    f32x16 acc;
    static_for<16>([&](auto rc) { acc[decltype(rc)::value] = 0.f; });
    // loader: thread -> (rows lr and lr + 16 of the chunk, 16-byte group lq of the tile's 64 channels)
    const int lq = tid & 15, lr = tid >> 4;
    const int co = mti * TM + lq * 4, ci = nti * TN + lq * 4;
    const bool co_ok = co < p.Cout, ci_ok = ci < p.Cin;
    f32x4 ra[2], rb[2];
    auto fetch = [&](int pc) {
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
            const int pp = pc + lr + 16 * h2;
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            ra[h2] = z;
            rb[h2] = z;
            if (pp < p1) {
                const int ox = pp % p.Wo, t = pp / p.Wo;
                const int oy = t % p.Ho, b = t / p.Ho;
                const int iy = 2 * oy + dyo, ix = 2 * ox + dxo;
                if (co_ok) ra[h2] = *reinterpret_cast<const f32x4*>(p.dy + (size_t)pp * p.Cout + co);
                if (ci_ok && (unsigned)iy < (unsigned)p.Hin && (unsigned)ix < (unsigned)p.Win)
                    rb[h2] = *reinterpret_cast<const f32x4*>(p.x + (((size_t)b * p.Hin + iy) * p.Win + ix) * p.Cin + ci);
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
    float* out = p.partial + (((size_t)split * taps + tap) * (p.mt * TM) + mti * TM + wm * 32) * (size_t)(p.nt * TN) + nti * TN + wn * 32;
    static_for<16>([&](auto rc) {
        constexpr int r = decltype(rc)::value;
        const int m = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        out[(size_t)m * (p.nt * TN) + (lane & 31)] = acc[r];
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
int s2_wgrad_splits(int tiles, int P) { return std::max(1, std::min(1024 / std::max(1, tiles) + 1, P / 64)); }
size_t round64(size_t n) { return (n + 63) / 64 * 64; }
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
    const int mt = (Cout + 63) / 64, nt = (Cin + 63) / 64, taps = ks * ks;
    return round64((size_t)s2_wgrad_splits(mt * nt * taps, B * (Hin / 2) * (Win / 2)) * taps * mt * 64 * nt * 64);
}

hipError_t conv_s2_wgrad_launch(const float* x, const float* dy, int B, int Hin, int Win, int Cin, int Cout, int ks, float* dweight,
                                float* workspace, size_t workspace_floats, hipStream_t s) {
    const size_t need = conv_s2_wgrad_workspace_floats(B, Hin, Win, Cin, Cout, ks);
    if (need == 0 || workspace_floats < need || (reinterpret_cast<uintptr_t>(workspace) & 15)) return hipErrorInvalidValue;
    S2WgradArgs a{};
    a.x = x;
    a.dy = dy;
    a.Hin = Hin;
    a.Win = Win;
    a.Ho = Hin / 2;
    a.Wo = Win / 2;
    a.Cin = Cin;
    a.Cout = Cout;
    a.ks = ks;
    a.P = B * a.Ho * a.Wo;
    a.mt = (Cout + 63) / 64;
    a.nt = (Cin + 63) / 64;
    const int taps = ks * ks, tiles = a.mt * a.nt * taps;
    const int splits = s2_wgrad_splits(tiles, a.P);
    a.per_split = ((a.P + splits - 1) / splits + 31) / 32 * 32;
    a.splits = (a.P + a.per_split - 1) / a.per_split;   // <= splits: the workspace holds them
    a.partial = workspace;
    note_mfma_flops(2.0 * taps * (double)a.splits * a.per_split * (a.mt * 64.0) * (a.nt * 64.0));
    hipLaunchKernelGGL(conv_s2_wgrad_kernel, dim3((unsigned)(tiles * a.splits)), dim3(256), 0, s, a);
    return conv_wgrad_reduce_launch(workspace, a.splits, taps, a.mt * 64, a.nt * 64, Cout, Cin, dweight, s);
}

}  // namespace eamm
