// Column-patch kernels for the 7x1 (vertical) MFMA convolutions: the generator's final 7x7 convolution (reference
// modules/generator.py:47,92: Conv2d(64 -> 3, 7x7, pad 3) + sigmoid) and the row-split flow head.
//
// The final layer runs as a 7x1 convolution with N = (dx, co) = 21 "output channels" followed by a horizontal gather of the seven
// dx taps.  The im2col-style kernel re-fetched its activation operand once per vertical tap -- 7 x 268 MB
// through L2 per launch at 256^2 x 16 frames, which bounds it (5.6 TB/s of L2 -> LDS traffic for 89 TFLOP/s).  Here a persistent
// workgroup walks 16x16-pixel tiles:
//   * per channel chunk the (16+6) x 16 input patch is DMA'd into LDS once; vertical tap t of output pixel (r, c) is patch pixel
//     (r + t, c) = the same LDS image a constant distance further on, so the seven taps' A fragments cost no address arithmetic
//     at all (an immediate offset);
//   * the whole weight tensor stays resident in LDS;
//   * the patch of the next (tile, chunk) unit streams in behind the MFMAs of the current one.
// Operand traffic drops from 7x to 22/16 = 1.4x the activation; the kernels are matrix-pipe bound.
//
// Which kernel runs when (conv_col7_launch / conv_col7_fused_launch; the engine fuses from final_fused_min_rows tile rows on):
//   conv_col7_kernel   plain: 32x32x2 fp32 MFMAs, N padded to 32; the [B,H,W,32] partial products go to HBM and
//                      final_shift_sum_kernel (at the end of this file) gathers them.  Small launches, e.g. one frame per call; tile code 4000.
//   conv_col7q_kernel  fused, fp32 products on the 4x4x1 multi-block MFMA (N = 24): gather, bias and sigmoid in the tile's
//                      epilogue.  The training entry eamm_op_final_conv_sigmoid and tile code 4003.
//   conv_col7b_kernel  fused, split-bf16 products (fp32-exact): the engine's default, tile code 4002.
//   conv_col7s_kernel  the flow head (N = 84 of 96, streamed weights, one workgroup per tile); tile code 4001.
// Shared: the tile walk (Col7Pos) and the work split (col7_units) by the three final-layer kernels; the fp32 patch stage
// (Col7Patch), the weight prologue and the unit loop (col7_walk_f32) by the two fp32 ones, which differ in the MFMA body of a
// unit and in what happens to a finished tile; the gather epilogue (col7_gather_tile) by the two fused ones.
#include "conv_common.h"

#include <algorithm>

namespace eamm {

typedef __attribute__((address_space(3))) void* lds_ptr_t;

namespace {
constexpr int CT = 16;                   // tile side
constexpr int CPR = CT + 6;              // patch rows (halo 3 above and below)
constexpr int CPIX = CPR * CT;           // 352 patch pixels = 44 DMA instructions of 8 pixels
constexpr int CWAVES = 8;
constexpr int CMAXCH = 2;                // channel chunks whose weights fit beside the two patch stages
constexpr size_t LDS_BUDGET = 160 * 1024;
}  // namespace

struct Col7Args {
    const float* in;       // [B,H,W,C]
    unsigned in_bytes, w_bytes;
    int C, B, H, W;
    int tiles_x, tiles_y, tiles;   // tiles per row / column / in total (B * tiles_y * tiles_x)
    const float* w;        // packed [C/32][7][32][32], LDS-DMA swizzle; conv_col7b_kernel: col7_pack_split_host's three-plane bf16 image
    float* out;            // [B,H,W,32]   (plain form)
    const float* bias;     // [3]          (fused forms)
    float* final_out;      // [B,3,H,W]    (fused forms): sigmoid(7x7 convolution + bias)
    int dbg;               // diagnostic (EAMM_COL7_DBG, tools/final_layer_bench.py; wrong results): 1 no patch DMA in the loop, 2 no tile epilogue
};

// The fused forms: the horizontal gather of the seven dx taps, the bias and the sigmoid happen in the tile's epilogue instead
// of in final_shift_sum_kernel -- the [B,H,W,32] partial products (65.5 MB written + read back per 8 frames at 256x256)
// never leave the CU.  Output column x needs the partial columns x-3 .. x+3, so a workgroup owns whole ROWS of tiles and
// walks them left to right: when tile T (columns c0 .. c0+15) is finished its partial products go to LDS (the stage that has
// just been consumed), the outputs of columns c0-3 .. c0+12 are formed from them and from the last six partial columns of
// tile T-1 (a 2 x 8 KB carry ring in the last 16 KB of LDS), and columns 10..15 become the next carry.

namespace {
constexpr int PS = 21;                         // partial products per pixel kept: (dx, co); odd stride: conflict-free column walks
constexpr int CARRY = CT * 6 * PS;             // six partial columns of a tile
}  // namespace

// Epilogue of a finished tile of the fused final layer (both MFMA forms): `scratch` holds the tile's partial products
// P[row][column][dx*3 + co]; forms the outputs of columns tx0-3 .. tx0+12 (.. tx0+15 for the row's last tile) from them and from
// the carry of the tile to the left, + bias, sigmoid, NCHW store; then saves columns 10..15 as the next tile's carry.
__device__ __forceinline__ void col7_gather_tile(const Col7Args& p, const float* scratch, float* Carry, const float (&bias_r)[3],
                                                 int b, int ty0, int tx0, int tid) {
    const int tix = tx0 / CT;
    const bool last = tix == p.tiles_x - 1;
    const float* carry_in = Carry + (tix & 1) * CARRY;          // columns tx0-6 .. tx0-1 (from tile T-1)
    float* carry_out = Carry + ((tix + 1) & 1) * CARRY;
    const int ncol = last ? CT + 3 : CT;                          // the row's last tile also finishes its last three columns
    // One thread per (row, output column): 16 rows x 32 column slots (16 or 19 used) = the 512 threads, the three
    // output channels in registers -- no integer division, no divergent tap loop (round 3 ran `i % ncol`, `i / ncol`
    // per output and a branch per tap: ~5 us of the ~17 us a tile takes; the stage is matrix-pipe time otherwise).
    // Tap dx of output column xl reads partial column c = xl - 6 + dx of this tile, of the carry (c < 0) or nothing.
    {
        const int xl = tid & 31, row = tid >> 5;
        const int x = tx0 - 3 + xl, y = ty0 + row;
        float v0 = bias_r[0], v1 = bias_r[1], v2 = bias_r[2];
#pragma unroll
        for (int dx = 0; dx < 7; ++dx) {
            const int c = xl - 6 + dx;
            const bool in_tile = (unsigned)c < (unsigned)CT, in_carry = (c < 0) & (tix > 0);
            // clamped (always valid) addresses, values selected afterwards: the loads issue back to back
            const float* src = in_tile ? scratch + (row * CT + c) * PS + dx * 3
                                       : carry_in + (row * 6 + max(c, -6) + 6) * PS + dx * 3;
            const float* safe = (in_tile | in_carry) ? src : scratch;
            const float p0 = safe[0], p1 = safe[1], p2 = safe[2];
            const bool use = in_tile | in_carry;
            v0 += use ? p0 : 0.f;
            v1 += use ? p1 : 0.f;
            v2 += use ? p2 : 0.f;
        }
        if (xl < ncol && x >= 0 && x < p.W && y < p.H) {
            float* o = p.final_out + ((size_t)b * 3 * p.H + y) * p.W + x;
            const size_t plane = (size_t)p.H * p.W;
            o[0] = 1.f / (1.f + __expf(-v0));
            o[plane] = 1.f / (1.f + __expf(-v1));
            o[2 * plane] = 1.f / (1.f + __expf(-v2));
        }
    }
    for (int i = tid; i < CARRY; i += CWAVES * 64) {                // columns 10..15 -> the next tile's carry
        const int n = i % PS, t2 = i / PS;
        const int c6 = t2 % 6, row = t2 / 6;
        carry_out[i] = scratch[(row * CT + 10 + c6) * PS + n];
    }
}


// Tile walk of a column-patch workgroup.  A unit is a (tile, 32-channel chunk) pair; ROWS: the workgroup's items are tile ROWS
// (first + k * gridDim.x), each walked tile by tile from the left; otherwise single tiles.  The position is advanced
// incrementally: round 3 re-derived it from the unit index with integer divisions inside every DMA piece -- ~180 vector
// instructions per unit and wave in the MFMA stream (the f32 MFMA shares the vector pipe: PMC SQ_INSTS_VALU 296 per unit and
// wave against 112 MFMAs), a fifth of the kernel.
struct Col7Pos {
    int cc, tix, t, b, ty0, tx0;
};
template <bool ROWS>
__device__ __forceinline__ void col7_pos_decode(Col7Pos& s, const Col7Args& p) {
    if constexpr (ROWS) {
        s.b = s.t / p.tiles_y;
        s.ty0 = (s.t - s.b * p.tiles_y) * CT;
        s.tx0 = s.tix * CT;
    } else {
        const int tt = s.t / p.tiles_x;
        s.tx0 = (s.t - tt * p.tiles_x) * CT;
        s.b = tt / p.tiles_y;
        s.ty0 = (tt - s.b * p.tiles_y) * CT;
    }
}
template <bool ROWS>
__device__ __forceinline__ void col7_pos_next(Col7Pos& s, const Col7Args& p, int cchunks, int grid) {
    if (++s.cc < cchunks) return;
    s.cc = 0;
    if constexpr (ROWS) {
        if (++s.tix < p.tiles_x) {
            s.tx0 = s.tix * CT;
            return;
        }
        s.tix = 0;
    }
    s.t += grid;
    col7_pos_decode<ROWS>(s, p);     // (the divisions: once per tile row / tile, not per DMA piece)
}

// The work split that goes with the walk: the units of this workgroup (its items first + k * gridDim.x, all chunks of each tile).
template <bool ROWS>
__device__ __forceinline__ int col7_units(const Col7Args& p, int chunks) {
    const int first = blockIdx.x, grid = (int)gridDim.x;
    const int items = ROWS ? p.B * p.tiles_y : p.tiles;
    const int my_items = first < items ? (items - first + grid - 1) / grid : 0;
    return my_items * (ROWS ? p.tiles_x : 1) * chunks;
}

// ---------------------------------------------------------------------------------------------------------
// The two fp32 kernels: LDS = [cchunks * 7][32 n][32 k] weights (swizzled), [2] patch stages of (16+6) x 16 pixels x 32 k
// (swizzled), fused: [2][CARRY].
namespace {
constexpr int A_STAGE = CPIX * CONV_BK;        // floats of a patch stage (44 KiB)
constexpr int W_TAP = 32 * CONV_BK;            // floats of one (chunk, tap) weight tile
constexpr int A_PIECES = CPIX / 8;             // 44 DMA pieces of 8 pixels
constexpr size_t col7_f32_lds_bytes(int cchunks, bool fused) {
    return sizeof(float) * (cchunks * 7 * W_TAP + 2 * A_STAGE + (fused ? 2 * CARRY : 0));
}
static_assert(col7_f32_lds_bytes(CMAXCH, true) <= LDS_BUDGET, "LDS budget");
}  // namespace

// The fp32 patch stage.  The pieces a lane issues: piece j = wave + 8 i (i = 0..5, j < 44) covers patch pixels 8 j .. 8 j + 7, a
// lane's pixel q = 8 j + lane / 8 = (row q / 16 - 3, column q % 16) of the tile and its 16-byte slot never change -- decoded once.
struct Col7Patch {
    int qr[6], qc[6], rel[6];
    int wave;
    float* As;             // [2][A_STAGE]
    __amdgpu_buffer_rsrc_t rsi;
    __device__ __forceinline__ Col7Patch(const Col7Args& p, float* stages, int wave_, int lane)
        : wave(wave_), As(stages), rsi(__builtin_amdgcn_make_buffer_rsrc((void*)p.in, 0, p.in_bytes, 0x00020000)) {
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const int q = (wave + CWAVES * i) * 8 + (lane >> 3);
            qr[i] = (q >> 4) - 3;
            qc[i] = q & 15;
            rel[i] = (qr[i] * p.W + qc[i]) * p.C + (((lane & 7) ^ ((q >> 1) & 7)) << 2);
        }
    }
    // patch piece i of the unit at `pos` into stage st (nothing where the wave has no piece i); pixels outside the image are
    // zero-filled by the hardware through the out-of-range offset
    template <int i>
    __device__ __forceinline__ void piece(const Col7Args& p, const Col7Pos& pos, int st) const {
        const int j = wave + CWAVES * i;
        if (j >= A_PIECES) return;
        const int y = pos.ty0 + qr[i], x = pos.tx0 + qc[i];
        const bool ok = ((unsigned)y < (unsigned)p.H) & ((unsigned)x < (unsigned)p.W);
        const int base = ((pos.b * p.H + pos.ty0) * p.W + pos.tx0) * p.C + pos.cc * CONV_BK;       // wave-uniform
        const unsigned off = ok ? (unsigned)(base + rel[i]) * 4u : 0xFFFFFFF0u;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsi, (lds_ptr_t)(As + st * A_STAGE + j * (8 * CONV_BK)), 16, off, 0, 0, 0);
    }
};

// The program of an fp32 column-patch workgroup around its MFMA body: all weights and the first patch in the prologue, then per
// unit   unit(patch stage, the chunk's weights, next_piece)   -- the body issues next_piece(integral_constant<i>), i = 0..5,
// between its MFMAs: piece i of the next unit's patch into the other stage --, on a tile's last chunk
// finish(position, the stage just consumed, carry ring)   (every wave may still be reading that stage), and one barrier.
template <bool ROWS, typename Unit, typename Finish>
__device__ __forceinline__ void col7_walk_f32(const Col7Args& p, float* smem, int wave, int lane, Unit&& unit, Finish&& finish) {
    const int cchunks = p.C / CONV_BK;
    float* const Ws = smem;
    float* const As = smem + cchunks * 7 * W_TAP;
    float* const Carry = As + 2 * A_STAGE;
    const int units = col7_units<ROWS>(p, cchunks);
    if (units == 0) return;

    const __amdgpu_buffer_rsrc_t rsw = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, p.w_bytes, 0x00020000);
    const Col7Patch patch(p, As, wave, lane);
    for (int j = wave; j < cchunks * 7 * 4; j += CWAVES) {   // 1 KiB pieces of the weight tensor
        const unsigned off = (unsigned)(j * (8 * CONV_BK) + lane * 4) * 4u;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsw, (lds_ptr_t)(Ws + j * (8 * CONV_BK)), 16, off, 0, 0, 0);
    }
    Col7Pos cur{0, 0, (int)blockIdx.x, 0, 0, 0};
    col7_pos_decode<ROWS>(cur, p);
    static_for<6>([&](auto ic) { patch.template piece<decltype(ic)::value>(p, cur, 0); });
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    const bool dma = !(p.dbg & 1), epilogue = !(p.dbg & 2);
    for (int u = 0; u < units; ++u) {
        const int st = u & 1;
        const bool more = dma && u + 1 < units;
        Col7Pos nxt = cur;
        col7_pos_next<ROWS>(nxt, p, cchunks, (int)gridDim.x);
        unit(As + st * A_STAGE, Ws + cur.cc * 7 * W_TAP, [&](auto ic) {
            if (more) patch.template piece<decltype(ic)::value>(p, nxt, st ^ 1);
        });
        if (cur.cc == cchunks - 1 && epilogue) finish(cur, As + st * A_STAGE, Carry);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        cur = nxt;
    }
}

// The plain form: per unit 7 taps x 4 K steps x 4 MFMAs 32x32x2 (N = 21 padded to 32); a finished tile's partial products go
// to p.out for final_shift_sum_kernel.
__global__ __launch_bounds__(CWAVES * 64) void conv_col7_kernel(const Col7Args p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, half = lane >> 5;

    f32x16 acc;
    static_for<16>([&](auto rc) { acc[decltype(rc)::value] = 0.f; });

    // this lane's pixel inside the tile: wave w owns rows 2w, 2w+1
    const int trow = 2 * wave + (l31 >> 4), tcol = l31 & 15;
    const int idx0 = trow * CT + tcol;                                      // patch pixel of tap 0 (dy = -3)
    const int a_off = idx0 * CONV_BK + ((half ^ ((idx0 >> 1) & 7)) << 2);   // + 8*s for K step s via XOR; + tap * CT * BK
    const int b_off = l31 * CONV_BK + ((half ^ ((l31 >> 1) & 7)) << 2);

    col7_walk_f32<false>(
        p, smem, wave, lane,
        [&](const float* a_stage, const float* w_stage, auto&& next_piece) {
            // the next unit's patch pieces (wave, wave+8, ...: 5 or 6 per wave) ride along
            f32x4 a[2], bb[2];
            auto fetch = [&](auto tc, auto sc_, int buf) {
                constexpr int t = decltype(tc)::value, s = decltype(sc_)::value;
                a[buf] = *reinterpret_cast<const f32x4*>(a_stage + ((a_off ^ (8 * s)) + t * CT * CONV_BK));
                bb[buf] = *reinterpret_cast<const f32x4*>(w_stage + ((b_off ^ (8 * s)) + t * W_TAP));
            };
            fetch(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{}, 0);
            static_for<28>([&](auto gc) {
                constexpr int g = decltype(gc)::value;       // (tap, K step) index
                if constexpr (g + 1 < 28)
                    fetch(std::integral_constant<int, (g + 1) / 4>{}, std::integral_constant<int, (g + 1) % 4>{}, (g + 1) & 1);
                __builtin_amdgcn_sched_barrier(0);
                static_for<4>([&](auto qc) {
                    constexpr int q = decltype(qc)::value;
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[g & 1][q], bb[g & 1][q], acc, 0, 0, 0);
                });
                if constexpr (g % 4 == 1 && g / 4 < 6) {     // one patch piece after every 16 MFMAs, 6 slots
                    __builtin_amdgcn_sched_barrier(0);
                    next_piece(std::integral_constant<int, g / 4>{});
                    __builtin_amdgcn_sched_barrier(0);
                }
            });
        },
        [&](const Col7Pos& pos, float*, float*) {
            // lanes 0..31 of a wave hold the 32 channels of one pixel -> 128-byte rows
            static_for<16>([&](auto rc) {
                constexpr int r = decltype(rc)::value;
                const int m = (r & 3) + 8 * (r >> 2) + 4 * half;   // pixel of the wave's 32: row m / 16, column m % 16
                const int y = pos.ty0 + 2 * wave + (m >> 4), x = pos.tx0 + (m & 15);
                if (y < p.H && x < p.W) p.out[((size_t)(pos.b * p.H + y) * p.W + x) * 32 + l31] = acc[r];
                acc[r] = 0.f;
            });
        });
}

// ---------------------------------------------------------------------------------------------------------
// The fused fp32 form on the MULTI-BLOCK MFMA v_mfma_f32_4x4x1_16b_f32.  N = (dx, co) = 21 of a 32-wide tile multiplies zeros in
// a third of its matrix-pipe time (the 32x32x2 form of round 3); the 4x4x1 form has an N granule of FOUR: with the A-block
// broadcast (cbsz = 4, abid = g) one instruction is D[i][lane p] += W[n = 4 g + i][k] * X[pixel p][k] -- 64 pixels
// (the lanes) x 4 columns x one k in 8 cycles, the same 64 FLOP / cycle / SIMD as the 32x32x2 form -- so six groups g cover
// n = 0..23: 24 / 21 = 14 % padding instead of 52 %, 0.75 x the matrix-pipe cycles.  A wave owns 64 pixels (4 rows of the
// 16x16 tile) and three of the six groups (waves 0-3: n 0..11, waves 4-7: n 12..23); per (tap, 16-byte slot of the channel
// chunk) it reads ONE ds_read_b128 of the patch (lane = pixel: its 4 k values) and ONE of the weights (lane = n: W[n][4 k]),
// and issues 4 k x 3 groups = 12 MFMAs on three rotating accumulators.
// (One patch piece of the next unit per tap, six of the seven taps: issuing them twice as densely at the start of the unit
// measured the same -- 210.4 vs 213.4 us at 8 frames, 3915 vs 3912 frames/s in the pipeline.)
template <int NH, typename NextPiece>
__device__ __forceinline__ void col7q_unit(const float* a_stage, const float* w_stage, int a_off, int b_off, f32x4 (&acc)[3],
                                           NextPiece&& next_piece) {
    constexpr int EVERY = 8;                         // (tap, slot) groups per patch piece of the next unit
    f32x4 xa[2], wb[2];
    auto fetch = [&](auto tc, auto sc_, int buf) {
        constexpr int t = decltype(tc)::value, sl = decltype(sc_)::value;
        xa[buf] = *reinterpret_cast<const f32x4*>(a_stage + ((a_off ^ (4 * sl)) + t * CT * CONV_BK));
        wb[buf] = *reinterpret_cast<const f32x4*>(w_stage + ((b_off ^ (4 * sl)) + t * W_TAP));
    };
    fetch(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{}, 0);
    static_for<56>([&](auto gc) {
        constexpr int g = decltype(gc)::value;       // (tap, slot) index: 7 taps x 8 slots of 4 channels
        if constexpr (g + 1 < 56)
            fetch(std::integral_constant<int, (g + 1) / 8>{}, std::integral_constant<int, (g + 1) % 8>{}, (g + 1) & 1);
        __builtin_amdgcn_sched_barrier(0);
        static_for<4>([&](auto qc) {
            constexpr int q = decltype(qc)::value;
            // srcA = weights (block abid broadcast to all sixteen blocks), srcB = the 64 pixels
            acc[0] = __builtin_amdgcn_mfma_f32_4x4x1f32(wb[g & 1][q], xa[g & 1][q], acc[0], 4, 3 * NH + 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_4x4x1f32(wb[g & 1][q], xa[g & 1][q], acc[1], 4, 3 * NH + 1, 0);
            acc[2] = __builtin_amdgcn_mfma_f32_4x4x1f32(wb[g & 1][q], xa[g & 1][q], acc[2], 4, 3 * NH + 2, 0);
        });
        if constexpr (g % EVERY == EVERY / 2 - 1 && g / EVERY < 6) {
            __builtin_amdgcn_sched_barrier(0);
            next_piece(std::integral_constant<int, g / EVERY>{});
            __builtin_amdgcn_sched_barrier(0);
        }
    });
}

__global__ __launch_bounds__(CWAVES * 64) void conv_col7q_kernel(const Col7Args p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pg = wave & 3, nh = wave >> 2;       // pixel group (rows 4 pg .. 4 pg + 3), half of the six n groups

    f32x4 acc[3];
    static_for<3>([&](auto gc) { acc[decltype(gc)::value] = f32x4{0.f, 0.f, 0.f, 0.f}; });

    // this lane's pixel inside the tile (srcB): row 4 pg + lane / 16, column lane % 16; tap 0 (dy = -3) is the same patch pixel
    const int idx0 = (4 * pg + (lane >> 4)) * CT + (lane & 15);
    const int a_off = idx0 * CONV_BK + (((idx0 >> 1) & 7) << 2);       // ^ 4 * slot; + tap * CT * BK (keeps (idx >> 1) & 7)
    // this lane's weight row (srcA): n = lane (only lanes 4 g .. 4 g + 3 of the broadcast block are read: n < 24)
    const int nrow = lane & 31;
    const int b_off = nrow * CONV_BK + (((nrow >> 1) & 7) << 2);
    const float bias_r[3] = {p.bias[0], p.bias[1], p.bias[2]};

    col7_walk_f32<true>(
        p, smem, wave, lane,
        [&](const float* a_stage, const float* w_stage, auto&& next_piece) {
            if (nh == 0) col7q_unit<0>(a_stage, w_stage, a_off, b_off, acc, next_piece);
            else col7q_unit<1>(a_stage, w_stage, a_off, b_off, acc, next_piece);
        },
        [&](const Col7Pos& pos, float* scratch, float* Carry) {
            // once every wave is done with the stage it takes the tile's partial products P[row][column][n], n = 12 nh + 4 g + i
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            float* dst = scratch + idx0 * PS + 12 * nh;
            static_for<3>([&](auto gc) {
                constexpr int g = decltype(gc)::value;
                static_for<4>([&](auto ic) {
                    constexpr int i = decltype(ic)::value;
                    if (12 * nh + 4 * g + i < PS) dst[4 * g + i] = acc[g][i];
                    acc[g][i] = 0.f;
                });
            });
            __syncthreads();
            col7_gather_tile(p, scratch, Carry, bias_r, pos.b, pos.ty0, pos.tx0, tid);
        });
}

// ---------------------------------------------------------------------------------------------------------
// The fused final layer with SPLIT-BF16 products (as SPLIT of wino4_gemm_kernel and FORM 1 of conv_patch_poly_kernel): every fp32
// operand is the exact sum of three bf16 values taken by truncation, a = a1 + a2 + a3, and a * b is the six terms of conv_common.h's
// term table on v_mfma_f32_32x32x16_bf16 with fp32 accumulation.  Rows are the wave's 32 pixels (2 tile rows x 16 columns, as
// conv_col7_kernel), columns n = (dx, co) padded from 21 to 32: 7 taps x 6 MFMAs of 32 cycles per 16 channels against
// 7 x 16 x 12 / 2 of 9.3 in the 4x4x1 form.
//   * A lane's seven vertical taps are seven different patch pixels, so splitting the fragment after the LDS read (as the other two
//     kernels do) would split every patch value seven times.  Here a value is split ONCE: the DMA lands fp32 in LDS, 16 channels
//     of the 22 x 16 patch per unit (22 pieces of 1 KiB, one patch row each), and each wave splits the pieces IT fetched
//     (split3_bf16) into a plane image [plane][k octet][pixel][8 bf16]: tap t is still the same image a constant 256 B further on,
//     a wave's 32 pixels of a (tap, plane, octet) are 512 contiguous bytes (one conflict-free ds_read_b128), and because a wave
//     reads back only its own DMA no barrier stands between landing and split, only the wave's vmcnt.
//   * The weights come split from the host (col7_pack_split_host): [16-channel group][tap][plane][k octet][21 rows][8 bf16], whole
//     in LDS (55 KiB); lanes of columns >= 21 re-read row 20 (a B column only reaches its own output column, never stored).
//   * LDS: weights 56 KiB, ONE fp32 stage 22 KiB, TWO plane stages 2 x 33 KiB, carry ring 15.75 KiB = 163 584 B.  Unit u: the
//     MFMAs read plane stage u & 1 while the DMA of unit u + 1 lands in the fp32 stage; then the wave splits its pieces into plane
//     stage (u + 1) & 1, whose readers finished before the previous barrier: one barrier per unit.  The finished tile's partial
//     products go to the plane stage just consumed.
// Work split, tile walk, carry ring and gather epilogue are shared with the kernels above; the staging is its own.
namespace {
constexpr int SG = 16;                                    // channels per unit
constexpr int S_WBLK = 2 * PS * 16;                       // bytes of a (group, tap, plane) weight block: [octet][21 rows][8 bf16]
constexpr int S_WGROUP = 7 * 3 * S_WBLK;                  // ... of a 16-channel group
constexpr int S_WBYTES = (CMAXCH * 2 * S_WGROUP + 1023) / 1024 * 1024;   // weights region, whole DMA pieces (57 344 B)
constexpr int S_ROWS = CPR;                               // DMA pieces per unit: one 16-pixel patch row x 16 channels = 1 KiB
constexpr int S_F32 = S_ROWS * 1024;                      // the fp32 stage (22 528 B)
constexpr int S_OCT = CPIX * 16;                          // bytes of a (plane, octet): 352 pixels x 8 bf16
constexpr int S_PLANE = 2 * S_OCT;
constexpr int S_PSTAGE = 3 * S_PLANE;                     // a plane stage (33 792 B)
constexpr int S_LDS = S_WBYTES + S_F32 + 2 * S_PSTAGE + 2 * CARRY * 4;
static_assert(S_LDS <= LDS_BUDGET, "LDS budget");
static_assert(CT * CT * PS * 4 <= S_PSTAGE, "the tile's partial products fit a consumed plane stage");
static_assert(CPR <= 3 * CWAVES, "at most three pieces per wave");
}  // namespace

__global__ __launch_bounds__(CWAVES * 64) void conv_col7b_kernel(const Col7Args p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];  // weight planes, fp32 stage, [2] plane stages, [2][CARRY]
    char* const Ws = reinterpret_cast<char*>(smem);
    char* const Fs = Ws + S_WBYTES;
    char* const Ps = Fs + S_F32;
    float* const Carry = reinterpret_cast<float*>(Ps + 2 * S_PSTAGE);
    const int groups = p.C / SG;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, half = lane >> 5;

    const __amdgpu_buffer_rsrc_t rsi = __builtin_amdgcn_make_buffer_rsrc((void*)p.in, 0, p.in_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsw = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, p.w_bytes, 0x00020000);
    constexpr unsigned OOB = 0xFFFFFFF0u;

    const int units = col7_units<true>(p, groups);
    if (units == 0) return;

    // Patch piece i of this wave = patch row j = wave + 8 i (j < 22): DMA lane L lands at byte 16 L of the piece and fetches
    // pixel L & 15, channels 8 h + 4 q .. + 3 of the group (h = (L >> 4) & 1, q = L >> 5): the split lane s = 16 h + pixel then
    // reads its eight channels as the 16-byte slots s and 32 + s, both lane-linear.
    const int d_px = lane & 15;
    const int d_rel = d_px * p.C + 8 * ((lane >> 4) & 1) + 4 * (lane >> 5);
    auto dma_patch_piece = [&](auto ic, const Col7Pos& pos) {
        constexpr int i = decltype(ic)::value;
        const int j = wave + CWAVES * i;
        const int y = pos.ty0 + j - 3, x = pos.tx0 + d_px;
        const bool ok = ((unsigned)y < (unsigned)p.H) & ((unsigned)x < (unsigned)p.W);
        const int base = ((pos.b * p.H + y) * p.W + pos.tx0) * p.C + pos.cc * SG;       // wave-uniform
        const unsigned off = ok ? (unsigned)(base + d_rel) * 4u : OOB;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsi, (lds_ptr_t)(Fs + j * 1024), 16, off, 0, 0, 0);
    };
    // The wave's pieces, fp32 stage -> plane stage `dst`: round 0 lanes 0-31 piece wave, lanes 32-63 piece wave + 8; round 1
    // lanes 0-31 piece wave + 16 (waves 0-5).  Lane s of a piece: pixel s & 15, k octet s >> 4.
    auto split_pieces = [&](char* dst) {
        static_for<2>([&](auto rc) {
            constexpr int r = decltype(rc)::value;
            const int j = r == 0 ? wave + CWAVES * half : wave + 2 * CWAVES;
            if (r == 0 || (half == 0 && j < S_ROWS)) {
                const char* src = Fs + j * 1024 + l31 * 16;
                const f32x4 x0 = *reinterpret_cast<const f32x4*>(src), x1 = *reinterpret_cast<const f32x4*>(src + 512);
                u32x4 pl[3];
                split3_bf16(x0, x1, pl);
                char* d = dst + (l31 >> 4) * S_OCT + (j * CT + (l31 & 15)) * 16;
                static_for<3>([&](auto kc) { *reinterpret_cast<u32x4*>(d + decltype(kc)::value * S_PLANE) = pl[decltype(kc)::value]; });
            }
        });
    };

    // ---- prologue: all weight planes + the first unit's patch, split
    for (int j = wave; j < groups * S_WGROUP / 1024 + 1; j += CWAVES)    // 1 KiB pieces; the image is padded to whole pieces
        if (j * 1024 < (int)p.w_bytes)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsw, (lds_ptr_t)(Ws + j * 1024), 16, (unsigned)(j * 1024 + lane * 16), 0, 0, 0);
    Col7Pos cur{0, 0, (int)blockIdx.x, 0, 0, 0};
    col7_pos_decode<true>(cur, p);
    static_for<3>([&](auto ic) {
        if (wave + CWAVES * decltype(ic)::value < S_ROWS) dma_patch_piece(ic, cur);
    });
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    split_pieces(Ps);
    __syncthreads();

    f32x16 acc;
    static_for<16>([&](auto rc) { acc[decltype(rc)::value] = 0.f; });
    // A: this lane's pixel of the wave's 32 (rows 2 wave, 2 wave + 1: patch pixel 32 wave + l31 at tap 0) and k octet;
    // B: its weight row (column n = l31; columns >= 21 re-read row 20) and k octet
    const int a_off = half * S_OCT + (32 * wave + l31) * 16;
    const int b_off = half * (PS * 16) + min(l31, PS - 1) * 16;
    const float bias_r[3] = {p.bias[0], p.bias[1], p.bias[2]};

    for (int u = 0; u < units; ++u) {
        const int st = u & 1;
        const bool more = u + 1 < units;
        const int b = cur.b, ty0 = cur.ty0, tx0 = cur.tx0, cc = cur.cc;
        Col7Pos nxt = cur;
        col7_pos_next<true>(nxt, p, groups, (int)gridDim.x);
        const char* a_stage = Ps + st * S_PSTAGE + a_off;
        const char* w_stage = Ws + cc * S_WGROUP + b_off;
        // 7 taps x 6 MFMAs; three plane reads of each operand per tap, one per MFMA gap; the next unit's patch pieces (2 or 3
        // per wave) ride behind the first three taps
        u32x4 ap[2][3], wp[2][3];
        auto fetch = [&](auto tc, int buf) {
            constexpr int t = decltype(tc)::value;
            static_for<3>([&](auto kc) {
                constexpr int k = decltype(kc)::value;
                ap[buf][k] = *reinterpret_cast<const u32x4*>(a_stage + k * S_PLANE + t * (CT * 16));
                wp[buf][k] = *reinterpret_cast<const u32x4*>(w_stage + (t * 3 + k) * S_WBLK);
            });
        };
        fetch(std::integral_constant<int, 0>{}, 0);
        static_for<7>([&](auto tc) {
            constexpr int t = decltype(tc)::value;
            if constexpr (t + 1 < 7) fetch(std::integral_constant<int, t + 1>{}, (t + 1) & 1);
            __builtin_amdgcn_sched_barrier(0);
            static_for<SPLIT_TERMS>([&](auto mc) {   // a1b3 | a3b1 a2b1 a1b1 | a2b2 a1b2
                constexpr int pa = SPLIT_TERM_A[decltype(mc)::value], pb = SPLIT_TERM_B[decltype(mc)::value];
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, ap[t & 1][pa]),
                                                              __builtin_bit_cast(bf16x8_t, wp[t & 1][pb]), acc, 0, 0, 0);
            });
            if constexpr (t < 3) {
                __builtin_amdgcn_sched_barrier(0);
                if (more && wave + CWAVES * t < S_ROWS) dma_patch_piece(tc, nxt);
            }
            __builtin_amdgcn_sched_barrier(0);
        });
        if (more) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            split_pieces(Ps + (st ^ 1) * S_PSTAGE);
        }
        if (cc == groups - 1) {
            // every wave is done with this unit's plane stage (the next unit's planes went to the other one): it becomes the
            // scratch for the tile's partial products P[row][column][dx*3 + co]
            __syncthreads();
            float* const scratch = reinterpret_cast<float*>(Ps + st * S_PSTAGE);
            static_for<16>([&](auto rc) {
                constexpr int r = decltype(rc)::value;
                const int m = (r & 3) + 8 * (r >> 2) + 4 * half;
                const int row = 2 * wave + (m >> 4), col = m & 15;
                if (l31 < PS) scratch[(row * CT + col) * PS + l31] = acc[r];
                acc[r] = 0.f;
            });
            __syncthreads();
            col7_gather_tile(p, scratch, Carry, bias_r, b, ty0, tx0, tid);
        }
        __syncthreads();
        cur = nxt;
    }
}
// ---------------------------------------------------------------------------------------------------------
// Same tile geometry for the row-split flow head (7x1 over N = 7 x (K+2) = 84 of 96, two concatenated inputs, 128 input
// channels): the weights ([4][7][96][32] = 336 KiB) do not fit, so they stream one (chunk, tap) tile per barrier interval
// (NT x 4 KiB, double buffered) next to the two patch stages; one workgroup per 16x16 tile.
struct Col7sArgs {
    const float* in0;      // [B,H,W,C0]
    const float* in1;      // [B,H,W,C1] or null
    unsigned in0_bytes, in1_bytes, w_bytes;
    int C0, C1, B, H, W;
    int tiles_x, tiles_y;
    const float* w;        // packed [(C0+C1)/32][7][NT*32][32], LDS-DMA swizzle
    float* out;            // [B,H,W,PS]
    int PS;                // pixel stride of `out` in floats (>= NT*32)
};

template <int NT>
__global__ __launch_bounds__(CWAVES * 64) void conv_col7s_kernel(const Col7sArgs p) {
    constexpr int BK = CONV_BK;
    constexpr int A_STAGE = CPIX * BK;             // floats (44 KiB)
    constexpr int W_STAGE = NT * 32 * BK;          // one (chunk, tap) weight tile
    constexpr int A_PIECES = CPIX / 8;             // 44
    constexpr int W_PIECES = NT * 4;
    extern __shared__ __attribute__((aligned(16))) float smem[];  // [2][A_STAGE] patches, [2][W_STAGE] weights
    float* const As = smem;
    float* const Ws = smem + 2 * A_STAGE;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, half = lane >> 5;
    const int cchunks = (p.C0 + p.C1) / BK;
    const int nint = cchunks * 7;

    int t = xcd_remap(blockIdx.x, gridDim.x);
    const int tx0 = (t % p.tiles_x) * CT;
    t /= p.tiles_x;
    const int ty0 = (t % p.tiles_y) * CT;
    const int b = t / p.tiles_y;

    const __amdgpu_buffer_rsrc_t rs0 = __builtin_amdgcn_make_buffer_rsrc((void*)p.in0, 0, p.in0_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs1 =
        __builtin_amdgcn_make_buffer_rsrc((void*)(p.in1 ? p.in1 : p.in0), 0, p.in1 ? p.in1_bytes : 0u, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsw = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, p.w_bytes, 0x00020000);
    constexpr unsigned OOB = 0xFFFFFFF0u;

    auto dma_patch_piece = [&](int j, int cc, int st) {
        const int q = j * 8 + (lane >> 3);
        const int y = ty0 + (q >> 4) - 3, x = tx0 + (q & 15);
        const bool ok = ((unsigned)y < (unsigned)p.H) & ((unsigned)x < (unsigned)p.W);
        const int slot = ((lane & 7) ^ ((q >> 1) & 7)) << 2;
        const int c0 = cc * BK;
        const bool first = c0 < p.C0;
        const int C = first ? p.C0 : p.C1;
        const int coff = first ? c0 : c0 - p.C0;
        const unsigned off = ok ? (unsigned)(((b * p.H + y) * p.W + x) * C + coff + slot) * 4u : OOB;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(first ? rs0 : rs1, (lds_ptr_t)(As + st * A_STAGE + j * (8 * BK)), 16, off, 0, 0, 0);
    };
    auto dma_weight_piece = [&](int j, int it, int st) {   // piece j (0..W_PIECES-1) of interval it
        const unsigned off = (unsigned)((it * NT * 32 + j * 8) * BK + lane * 4) * 4u;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsw, (lds_ptr_t)(Ws + st * W_STAGE + j * (8 * BK)), 16, off, 0, 0, 0);
    };

    for (int j = wave; j < A_PIECES; j += CWAVES) dma_patch_piece(j, 0, 0);
    for (int j = wave; j < W_PIECES; j += CWAVES) dma_weight_piece(j, 0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    f32x16 acc[NT];
    static_for<NT>([&](auto jc) { static_for<16>([&](auto rc) { acc[decltype(jc)::value][decltype(rc)::value] = 0.f; }); });

    const int trow = 2 * wave + (l31 >> 4), tcol = l31 & 15;
    const int idx0 = trow * CT + tcol;
    const int a_off = idx0 * BK + ((half ^ ((idx0 >> 1) & 7)) << 2);
    const int b_off = l31 * BK + ((half ^ ((l31 >> 1) & 7)) << 2);

    int cc = 0, tap = 0;
    for (int it = 0; it < nint; ++it) {
        const bool more_w = it + 1 < nint, more_a = cc + 1 < cchunks;
        const float* a_stage = As + (cc & 1) * A_STAGE + tap * (CT * BK);
        const float* w_stage = Ws + (it & 1) * W_STAGE;
        f32x4 a[2], bb[2][NT];
        auto fetch = [&](auto sc_, int buf) {
            constexpr int s = decltype(sc_)::value;
            a[buf] = *reinterpret_cast<const f32x4*>(a_stage + (a_off ^ (8 * s)));
#pragma unroll
            for (int j = 0; j < NT; ++j) bb[buf][j] = *reinterpret_cast<const f32x4*>(w_stage + (b_off ^ (8 * s)) + j * 32 * BK);
        };
        fetch(std::integral_constant<int, 0>{}, 0);
        static_for<4>([&](auto stc) {
            constexpr int step = decltype(stc)::value;
            if constexpr (step + 1 < 4) fetch(std::integral_constant<int, step + 1>{}, (step + 1) & 1);
            __builtin_amdgcn_sched_barrier(0);
            static_for<4 * NT>([&](auto qc) {
                constexpr int q = decltype(qc)::value;
                constexpr int tq = q / NT, j = q % NT;
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[step & 1][tq], bb[step & 1][j][tq], acc[j], 0, 0, 0);
            });
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (step == 0) {          // next interval's weights: pieces wave, wave + 8, ...
                if (more_w)
                    for (int j = wave; j < W_PIECES; j += CWAVES) dma_weight_piece(j, it + 1, (it + 1) & 1);
            } else if constexpr (step == 1) {   // next chunk's patch: piece tap*8 + wave (44 pieces over the 7 taps)
                const int j = tap * CWAVES + wave;
                if (more_a && j < A_PIECES) dma_patch_piece(j, cc + 1, (cc + 1) & 1);
            }
            __builtin_amdgcn_sched_barrier(0);
        });
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (++tap == 7) {
            tap = 0;
            ++cc;
        }
    }
    static_for<NT>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        static_for<16>([&](auto rc) {
            constexpr int r = decltype(rc)::value;
            const int m = (r & 3) + 8 * (r >> 2) + 4 * half;
            const int y = ty0 + 2 * wave + (m >> 4), x = tx0 + (m & 15);
            if (y < p.H && x < p.W) p.out[((size_t)(b * p.H + y) * p.W + x) * p.PS + j * 32 + l31] = acc[j][r];
        });
    });
}

hipError_t conv_col7s_launch(const float* in0, int C0, const float* in1, int C1, int B, int H, int W, const float* w_swizzled,
                             int ntile32, float* out, int pixel_stride, hipStream_t stream) {
    if (C0 % CONV_BK || C1 % CONV_BK || C0 < CONV_BK || ntile32 != 3 || pixel_stride < ntile32 * 32)
        return hipErrorInvalidValue;
    Col7sArgs a{};
    a.in0 = in0;
    a.in1 = C1 ? in1 : nullptr;
    const size_t px = (size_t)B * H * W;
    const size_t b0 = px * C0 * 4, b1 = px * C1 * 4, wb = (size_t)((C0 + C1) / CONV_BK) * 7 * ntile32 * 32 * CONV_BK * 4;
    if (b0 >= 0xFFFFFFF0ull || b1 >= 0xFFFFFFF0ull || wb >= 0xFFFFFFF0ull) return hipErrorInvalidValue;
    a.in0_bytes = (unsigned)b0;
    a.in1_bytes = (unsigned)b1;
    a.w_bytes = (unsigned)wb;
    a.C0 = C0;
    a.C1 = C1;
    a.B = B;
    a.H = H;
    a.W = W;
    a.tiles_x = (W + CT - 1) / CT;
    a.tiles_y = (H + CT - 1) / CT;
    a.w = w_swizzled;
    a.out = out;
    a.PS = pixel_stride;
    constexpr size_t lds = sizeof(float) * (2 * CPIX * CONV_BK + 2 * 3 * 32 * CONV_BK);
    static_assert(lds <= 160 * 1024, "LDS budget");
    static lds_once_mask configured{0};
    if (hipError_t e = ensure_dynamic_lds(conv_col7s_kernel<3>, lds, &configured); e != hipSuccess) return e;
    note_mfma_flops(2.0 * a.tiles_x * a.tiles_y * B * (CT * CT) * 7.0 * (ntile32 * 32) * (C0 + C1));
    hipLaunchKernelGGL(conv_col7s_kernel<3>, dim3(a.tiles_x * a.tiles_y * B), dim3(CWAVES * 64), lds, stream, a);
    return hipGetLastError();
}

// floats of device memory the three-plane image of conv_col7b_kernel takes (whole 1 KiB DMA pieces)
size_t col7_split_packed_elems(int cin_packed) { return ((size_t)(cin_packed / SG) * S_WGROUP + 1023) / 1024 * 256; }

// The row-split 7x1 weights w [Cout <= 21][Cin][7] (to_rowsplit of the folded 7x7 filter: the fp32-ROUNDED values the fp32 image is
// packed from) as three bf16 planes by truncation (split3_bf16_host), so w1 + w2 + w3 is that float exactly.  Image [16-channel group][tap][plane][k octet][21 rows][8]: lane
// (row n, octet h) of conv_col7b_kernel reads the group's channels 8 h .. 8 h + 7 with one ds_read_b128.
void col7_pack_split_host(const float* w, int Cout, int Cin, const int* cin_map, int cin_packed, uint16_t* dst) {
    const size_t total = 2 * col7_split_packed_elems(cin_packed);
    for (size_t i = 0; i < total; ++i) dst[i] = 0;
    for (int n = 0; n < Cout && n < PS; ++n)
        for (int cp = 0; cp < cin_packed; ++cp) {
            const int c = cin_map ? cin_map[cp] : cp;
            if (c < 0 || c >= Cin) continue;
            for (int t = 0; t < 7; ++t) {
                uint16_t pl[3];
                split3_bf16_host(w[((size_t)n * Cin + c) * 7 + t], pl);
                const int g = cp / SG, h = (cp % SG) >> 3, e = cp & 7;
                uint16_t* blk = dst + ((size_t)(g * 7 + t) * 3 * S_WBLK + h * (PS * 16) + n * 16) / 2 + e;
                for (int k = 0; k < 3; ++k) blk[k * (S_WBLK / 2)] = pl[k];
            }
        }
}

// What the final layer's launches have in common: the shape checks and every argument but the weights' and the outputs'.
static hipError_t col7_fill_args(Col7Args& a, const float* in, int C, int B, int H, int W) {
    if (C % CONV_BK || C / CONV_BK > CMAXCH || C < CONV_BK) return hipErrorInvalidValue;
    const size_t ib = (size_t)B * H * W * C * 4;
    if (ib >= 0xFFFFFFF0ull) return hipErrorInvalidValue;
    a.in = in;
    a.in_bytes = (unsigned)ib;
    a.C = C;
    a.B = B;
    a.H = H;
    a.W = W;
    a.tiles_x = (W + CT - 1) / CT;
    a.tiles_y = (H + CT - 1) / CT;
    a.tiles = B * a.tiles_x * a.tiles_y;
#ifdef EAMM_EXPERIMENTS   // diagnostic builds only (make EXPERIMENTS=1): the product library never drops the DMA / the epilogue
    static const int dbg = (int)knob_int("EAMM_COL7_DBG", 0);
    a.dbg = dbg;
#endif
    return hipSuccess;
}

// One persistent workgroup per CU at the most (LDS: one workgroup per CU is resident), over `items` tiles or tile rows.
template <typename K>
static hipError_t col7_launch_kernel(K kern, lds_once_mask* configured, size_t lds, int items, const Col7Args& a, hipStream_t stream) {
    if (hipError_t e = ensure_dynamic_lds(kern, LDS_BUDGET, configured); e != hipSuccess) return e;
    int dev = 0, cus = 256;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    hipLaunchKernelGGL(kern, dim3(std::min(items, cus)), dim3(CWAVES * 64), lds, stream, a);
    return hipGetLastError();
}

hipError_t conv_col7_launch(const float* in, int C, int B, int H, int W, const float* w_swizzled, float* out,
                            hipStream_t stream) {
    Col7Args a{};
    if (hipError_t e = col7_fill_args(a, in, C, B, H, W); e != hipSuccess) return e;
    a.w = w_swizzled;
    a.w_bytes = (unsigned)(C / CONV_BK * 7 * W_TAP * sizeof(float));
    a.out = out;
    static lds_once_mask configured{0};
    note_mfma_flops(2.0 * a.tiles * (CT * CT) * 7.0 * 32 * C);          // N = 32 columns issued
    return col7_launch_kernel(conv_col7_kernel, &configured, col7_f32_lds_bytes(C / CONV_BK, false), a.tiles, a, stream);
}

// w_split (the layer's three-plane image) given: the split-bf16 product form; otherwise the fp32 form on the 4x4x1 MFMA.
hipError_t conv_col7_fused_launch(const float* in, int C, int B, int H, int W, const float* w_swizzled, const float* bias,
                                  float* out_nchw, hipStream_t stream, const float* w_split) {
    if (!bias || !out_nchw) return hipErrorInvalidValue;
    Col7Args a{};
    if (hipError_t e = col7_fill_args(a, in, C, B, H, W); e != hipSuccess) return e;
    a.bias = bias;
    a.final_out = out_nchw;
    // The layer counts what its fp32 form issues (N = 24), whatever the product form: bench.py prices `stage_roofline.final`
    // against the fp32 matrix peak, and the fp32-equivalent of the N = 32 columns issued by the split form exceeded it (1.02 of
    // the peak).
    note_mfma_flops(2.0 * a.tiles * (CT * CT) * 7.0 * 24 * C);
    static lds_once_mask configured_b{0}, configured_q{0};
    if (w_split) {
        a.w = w_split;
        a.w_bytes = (unsigned)(col7_split_packed_elems(C) * 4);
        return col7_launch_kernel(conv_col7b_kernel, &configured_b, S_LDS, B * a.tiles_y, a, stream);
    }
    a.w = w_swizzled;
    a.w_bytes = (unsigned)(C / CONV_BK * 7 * W_TAP * sizeof(float));
    return col7_launch_kernel(conv_col7q_kernel, &configured_q, col7_f32_lds_bytes(C / CONV_BK, true), B * a.tiles_y, a, stream);
}

// Final 7x7 convolution, second half (generator.py:92-93).  The MFMA kernel ran it as a 7x1 (vertical)
// convolution with N = (dx, co): part[b,y,x',dx*3+co] = sum_{dy,c} in[b,y+dy-3,x',c] * w[co,c,dy,dx].
// Here the seven horizontal taps are gathered: out[b,co,y,x] = sigmoid(bias[co] + sum_dx part[b,y,x+dx-3,
// dx*3+co]) (zero outside the row), written NCHW.  One block = one row segment of 128 pixels staged in
// LDS (row stride 33 dwords: conflict-free for the per-pixel column walk).
constexpr int FS_TILE = 128, FS_LD = 33;
__global__ __launch_bounds__(128) void final_shift_sum_kernel(const float* __restrict__ part,
                                                              const float* __restrict__ bias, int H, int W,
                                                              float* __restrict__ out) {
    __shared__ float tile[(FS_TILE + 6) * FS_LD];
    const int x0 = blockIdx.x * FS_TILE, y = blockIdx.y, b = blockIdx.z;
    const float4* row = reinterpret_cast<const float4*>(part + ((size_t)(b * H + y) * W) * 32);
    for (int i = threadIdx.x; i < (FS_TILE + 6) * 8; i += blockDim.x) {
        const int px = i >> 3, c4 = i & 7;
        const int x = x0 + px - 3;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if ((unsigned)x < (unsigned)W) v = row[(size_t)x * 8 + c4];
        float* d = tile + px * FS_LD + c4 * 4;
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x >= W) return;
    float acc[3] = {bias[0], bias[1], bias[2]};
#pragma unroll
    for (int dx = 0; dx < 7; ++dx) {
        const float* s = tile + (threadIdx.x + dx) * FS_LD + dx * 3;
        acc[0] += s[0];
        acc[1] += s[1];
        acc[2] += s[2];
    }
    const size_t plane = (size_t)H * W;
#pragma unroll
    for (int co = 0; co < 3; ++co)
        out[((size_t)b * 3 + co) * plane + (size_t)y * W + x] = 1.f / (1.f + expf(-acc[co]));
}

hipError_t final_shift_sum_launch(const float* part, const float* bias, int n, int H, int W, float* out,
                                  hipStream_t s) {
    hipLaunchKernelGGL(final_shift_sum_kernel, dim3((W + FS_TILE - 1) / FS_TILE, H, n), dim3(FS_TILE), 0, s, part,
                       bias, H, W, out);
    return hipGetLastError();
}

}  // namespace eamm
