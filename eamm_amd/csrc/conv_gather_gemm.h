// The register-staged implicit GEMM's main loop, once: conv_mfma.hip, conv_s2.hip, conv_s2_backward.hip (data gradient) and
// audio_backward.hip (ConvTranspose2d forward and data gradient) all run it.
//
// A block of 4 waves computes a BM x BN = (WM*MT*32) x (WN*NT*32) tile of D = A B^T on v_mfma_f32_32x32x2_f32, K walked in chunks of
// CONV_BK = 32 channels.  Both operands go HBM/L2 -> VGPR -> LDS through raw buffer loads (an offset of GG_OOB lies beyond every
// descriptor's range and reads zeros: padding and the M tail without a branch), LDS is double buffered ([2][BM][CONV_LDK] and
// [2][BN][CONV_LDK] floats), one barrier per chunk; the next chunk's loads are in flight under this chunk's MFMAs.  A lane reads FOUR
// consecutive k with one ds_read_b128 (lanes 0-31 k = 8s+{0..3}, lanes 32-63 k = 8s+{4..7}; A and B use the same permutation of K).
//
// A kernel that uses the loop supplies
//   * g = gather_lanes<WN>(threadIdx.x) and its per-row state, for the rows g.arow + 32 j (j < BM / 32) of the tile that this
//     thread stages,
//   * chunk(ci) -> gather_chunk(resource, off, wchunk) for chunk ci: off(j) is the BYTE offset in `resource` of row j's 16 bytes at
//     column acol, or GG_OOB; wchunk is the index of the chunk's [BN][CONV_BK] tile in the packed filter image (conv_pack's layout),
//   * the LDS, the chunk range [c_begin, c_end) (which may be empty: the accumulators are then zeros) and its own epilogue.
// The accumulators are indexed through static_for only, so that none of them is demoted to scratch.
#pragma once
#include "conv_common.h"

namespace eamm {

constexpr unsigned GG_OOB = 0xFFFFFFF0u;   // out of every buffer descriptor's range (the launchers refuse tensors that large)

// A thread's places in the block: wave (wm, wn) of the WM x WN grid, lane l31 + 32 half of the MFMA layout, and the loader's split of a
// chunk -- rows arow + 32 j, the 16 bytes at float column acol.  The kernel makes it once and uses it for its row state and epilogue too.
struct GatherLanes {
    int tid, l31, half, wm, wn, arow, acol;
};
template <int WN>
__device__ __forceinline__ GatherLanes gather_lanes(int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    return GatherLanes{tid, lane & 31, lane >> 5, wave / WN, wave % WN, tid >> 3, (tid & 7) * 4};
}

__device__ __forceinline__ __amdgpu_buffer_rsrc_t gather_rsrc(const float* base, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, bytes, 0x00020000);
}

// one K chunk: where operand A's rows come from and which tile of the packed filter is operand B
template <typename Off>
struct GatherChunk {
    __amdgpu_buffer_rsrc_t rsrc;
    Off off;
    int wchunk;
};
template <typename Off>
__device__ __forceinline__ GatherChunk<Off> gather_chunk(__amdgpu_buffer_rsrc_t rsrc, Off off, int wchunk) {
    return GatherChunk<Off>{rsrc, off, wchunk};
}

template <int MT, int NT, int WM, int WN, typename Chunk>
__device__ __forceinline__ void gather_gemm(f32x16 (&acc)[MT][NT], float* As /*[2][BM][LDK]*/, float* Bs /*[2][BN][LDK]*/,
                                            __amdgpu_buffer_rsrc_t rsw, const GatherLanes g, int c_begin, int c_end, Chunk chunk) {
    constexpr int BM = WM * MT * 32, BN = WN * NT * 32;
    constexpr int BK = CONV_BK, LDK = CONV_LDK;
    constexpr int A_PER = BM / 32, B_PER = BN / 32;
    static_assert(WM * WN == 4, "4 waves per block");

    const int tid = g.tid, l31 = g.l31, half = g.half, wm = g.wm, wn = g.wn, arow = g.arow, acol = g.acol;

    u32x4 av[A_PER], bv[B_PER];
    auto load_chunk = [&](int ci) {
        const auto ck = chunk(ci);
#pragma unroll
        for (int j = 0; j < A_PER; ++j) av[j] = __builtin_amdgcn_raw_buffer_load_b128(ck.rsrc, ck.off(j), 0, 0);
        const unsigned woff = (unsigned)(ck.wchunk * (BN * BK) + tid * 4) * 4u;
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

    static_for<MT>([&](auto ic) {
        static_for<NT>([&](auto jc) {
            static_for<16>([&](auto rc) { acc[decltype(ic)::value][decltype(jc)::value][decltype(rc)::value] = 0.f; });
        });
    });

    auto compute = [&](int st) {
        const float* a_base = As + st * BM * LDK + (wm * MT * 32 + l31) * LDK + half * 4;
        const float* b_base = Bs + st * BN * LDK + (wn * NT * 32 + l31) * LDK + half * 4;
#pragma unroll
        for (int s = 0; s < BK / 8; ++s) {
            f32x4 a[MT], b[NT];
#pragma unroll
            for (int i = 0; i < MT; ++i) a[i] = *reinterpret_cast<const f32x4*>(a_base + i * 32 * LDK + s * 8);
#pragma unroll
            for (int j = 0; j < NT; ++j) b[j] = *reinterpret_cast<const f32x4*>(b_base + j * 32 * LDK + s * 8);
            static_for<4>([&](auto tc) {
                constexpr int t = decltype(tc)::value;
                static_for<MT>([&](auto ic) {
                    constexpr int i = decltype(ic)::value;
                    static_for<NT>([&](auto jc) {
                        constexpr int j = decltype(jc)::value;
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][t], b[j][t], acc[i][j], 0, 0, 0);
                    });
                });
            });
        }
    };

    // LDS double buffer, one barrier per K chunk
    if (c_begin < c_end) {
        load_chunk(c_begin);
        store_chunk(0);
        __syncthreads();
        int st = 0;
        for (int ci = c_begin; ci < c_end; ++ci) {
            const bool more = ci + 1 < c_end;
            if (more) load_chunk(ci + 1);  // buffer loads in flight under the MFMAs
            compute(st);
            if (more) store_chunk(st ^ 1);
            __syncthreads();
            st ^= 1;
        }
    }
}

}  // namespace eamm
