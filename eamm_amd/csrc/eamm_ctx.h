// The generator handle and what its C-ABI translation units share: eamm_api.hip (handle, weights, workspace, source encoding),
// eamm_forward.hip (launch plan, the per-frame pass as one function per stage, profiling), eamm_op_*.hip (operator entries, over
// op_common.h), eamm_train_api.hip.  Around the handle: PassProfile (the stage profile), FrameView (the slice of the workspace one
// launch sequence works on) and what eamm_forward.hip defines for the other translation units.
#pragma once
#include "../../include/eamm_hip.h"
#include "api_common.h"

#include <functional>

using namespace eamm;

// Optional stage timing of eamm_forward_frames with HIP events on the caller's stream (bench.py roofline leg) and the executed
// matrix-core flops of every call: eamm_forward_frames brackets a call with begin_call / end_call, forward_view marks the stage
// boundaries, eamm_profile_read folds the finished event sets into the totals (all in eamm_forward.hip).
struct PassProfile {
    static constexpr int NSTAGE = 22;      // front, hg_enc, hg_dec, head, warp, bneck_transform, bneck_conv, up, final + bneck_gemm_kernel
                                           // + bneck_union_ms (wall time during which ANY chain is in its bottleneck stage), bneck_windows_ms (sum of
                                           // the chains' bottleneck windows), exec_gflop / bneck_exec_gflop (executed MFMA GFLOP of the recorded
                                           // calls, all chains: whole pass / bottleneck GEMMs) + 14..21 executed MFMA GFLOP of each of the eight
                                           // recorded stage intervals (front, hg_enc, hg_dec, head, warp, bottleneck, up, final), all chains
    static constexpr int MAXCHAIN = 4;     // chains whose bottleneck window is recorded per call
    static constexpr int NMARK = 8;        // stage boundaries recorded per call (bottleneck is split from sub-events)
    static constexpr int NSUB = 64;        // per-launch events inside the bottleneck (4 per res-block + 1)
    static constexpr int PROF_CALLS = 256; // event sets kept before the host must read them
    struct Call {                          // one recorded call
        int n = 0, nchain = 0, sub = 0;    // frames; whole-pass chains recorded; sub-events used (0: direct form)
        bool complete = false;             // every mark recorded (false: the call failed midway and its set is skipped)
        double flops = 0, flops_bneck = 0, stage_flops[NMARK] = {0};   // executed MFMA flops, all chains: pass / bottleneck / per interval
    };
    bool on = false;
    std::vector<hipEvent_t> events;        // PROF_CALLS * (NMARK+1 + NSUB): stage marks of the main stream's sequence, then sub-events
    std::vector<hipEvent_t> chain_ev;      // PROF_CALLS * MAXCHAIN * 2: start / end of each whole-pass chain's bottleneck stage
    std::vector<Call> calls;               // PROF_CALLS records, sized once by eamm_profile_enable: the first `used` await a read
    int used = 0;
    hipEvent_t *ev = nullptr, *cev = nullptr;   // the event sets of the call being enqueued (null: it is not recorded)
    Call cur;                              // ... and its record (flops are counted whether or not it is recorded)
    double ms[NSTAGE] = {0};
    long ncalls = 0, nframes = 0;

    void begin_call(int n, int chains);
    void account(int interval);            // flops launched since the last mark belong to the stage interval that ends here
    hipError_t mark(int i, hipStream_t s, int chain) {       // stage boundary i of chain `chain`'s sequence (events: chain 0 only)
        if (i > 0) account(i - 1);
        return ev && chain == 0 ? hipEventRecord(ev[i], s) : hipSuccess;
    }
    // one more per-launch event inside chain 0's bottleneck; edge 0 / 1: chain `chain` enters / leaves its bottleneck
    hipError_t sub(hipStream_t s) { return ev && cur.sub < NSUB ? hipEventRecord(ev[NMARK + 1 + cur.sub++], s) : hipSuccess; }
    hipError_t window(int chain, int edge, hipStream_t s) { return cev && chain < MAXCHAIN ? hipEventRecord(cev[2 * chain + edge], s) : hipSuccess; }
    hipError_t end_call(hipStream_t s);                      // the last stage ends where the call ends (after the join)
};

struct eamm_ctx : eamm::CtxBase {
    eamm_config cfg{};
    int ns_cached = 0;

    // derived geometry
    int H = 0, W = 0, h = 0, w = 0, hf = 0, wf = 0, K = 0, nb = 0, nd = 0;
    int Cb = 0;                 // bottleneck channels
    int Cp0 = 0;                // hourglass input channels padded to a multiple of 32
    int Csrc = 32;              // RGB source padded for the 7x7 MFMA encoder conv
    std::vector<int> enc_c;     // hourglass encoder output channels e_1..e_nb
    std::vector<int> dec_c;     // hourglass decoder output channels u_0..u_{nb-1}
    std::vector<int> down_c;    // generator encoder channels [be, ...]
    std::vector<int> up_c;      // generator decoder output channels
    // The four lists above and Cb hold the widths the KERNELS run at: the reference's widths rounded up to the 32-channel granule.
    // The *_r lists are the reference's own (what the state_dict has): when they differ, eamm_finalize_weights first pads the
    // state_dict into the equivalent wider network (zero filters, identity BatchNorm on the extra channels: they carry exact zeros).
    std::vector<int> enc_r, dec_r, down_r, up_r;
    int Cb_r = 0;
    bool padded_widths = false;
    // Image channels (num_channels, reference modules/generator.py:14,25,46): the kernels are written for three (a float4 per pixel:
    // RGB + a zero; the hourglass input line is (heat, R, G, B) per motion).  One or two channels run as the equivalent
    // three-channel network -- zero filters on the missing input channels of `first` / the hourglass's first block / the flow
    // head, zero filters + bias on the missing outputs of `final` (pad_state_dict) -- on a zero-extended source; the three-channel
    // results land in the staging buffers below and only the real channels are copied to the caller's tensors.
    int Cimg = 3;
    int G = 1, Cpl = 3;         // four to six image channels: G = 2 groups of three, Cpl = 6 planes in the zero-extended source copy
    float *stage_pred = nullptr, *stage_deformed = nullptr, *stage_sparse = nullptr;

    // layers
    ConvLayer first, final_conv, head;
    float *first7_w = nullptr, *first7_bias = nullptr;   // the first block on its dedicated 3-channel kernel (conv_first.hip), or null
    int first7 = 1;                                       // EAMM_FIRST7: 0 = the generic 7x7 kernel on the 32-channel-padded source
    std::vector<LayerSet> down, hg_enc, hg_dec, res1, res2, up;
    std::vector<WinoLayer> wres1, wres2;   // Winograd F(2x2,3x3) packing of the bottleneck convolutions
    std::vector<WinoLayer> w4res1, w4res2; // Winograd F(4x4,3x3) packing (bottleneck maps with sides divisible by 4)
    std::vector<WinoLayer> w4down;         // ... and of the generator encoder's DownBlock2d levels (source encoding, once per clip / per module call without cache)
    std::vector<WinoLayer> w4enc;          // F(4x4,3x3) packing of the hourglass encoder convolutions (Cout == 0: level not eligible)
    int enc_wino = 1;                      // hourglass DownBlock2d levels in F(4x4,3x3) form + pooled output transform (EAMM_ENC_WINO)
    int enc_wino_min_mflop = 3000;         // ... for levels of at least this many direct-form MFLOP per call (EAMM_ENC_WINO_MIN_MFLOP): smaller ones are
                                           // launch-bound and one launch beats three (measured 256x256: 1 frame 810 vs 804, 4 frames equal,
                                           // 8 frames 2896 -> 2960, 12 frames 2849 -> 2968, 16 frames 3529 -> 3659; 512x512 x 8: 911 -> 948 frames/s)
    int enc_wino_min_tiles = 32;           // ... and of at least this many 4x4 tiles (EAMM_ENC_WINO_MIN_TILES; x4 for levels with > 100 MB of transformed
                                           // weights): the 4x4-map level has 16 tiles at 16 frames against 151 MB and stays direct
    int bneck_chains = 2;                  // bottleneck as this many chains of frames on as many streams (EAMM_BNECK_CHAINS; 1 = off)
    int pass_chains = 0;                   // the whole per-frame pass as this many chains (EAMM_PASS_CHAINS; 1 = off; 0 = the default: two chains
                                           // when each chain's F(4x4) GEMM keeps enough workgroups (pass_chains_min_blocks); otherwise off)
    int pass_chains_min_blocks = 80;       // automatic mode: fewest bottleneck-GEMM workgroups per chain (EAMM_PASS_CHAINS_MIN_BLOCKS)
    int pass_chains_min_frames = 8;        // ... from this many frames per call (EAMM_PASS_CHAINS_MIN_FRAMES)
    std::vector<hipStream_t> side_streams; // the other chains' streams of the call being enqueued: pool_streams or own_streams (StreamLease in eamm_forward.hip)
    std::vector<hipStream_t> pool_streams; // ... the device's shared pool (chain_stream(), not owned)
    std::vector<hipStream_t> own_streams;  // ... this handle's private set: used while the caller's stream is being captured or another
                                           // thread holds the pool; created on first need, destroyed with the handle
    int private_streams = 0;               // EAMM_PRIVATE_STREAMS=1: always the private set
    int last_streams = 0;                  // which set the last call used: 0 pool, 1 private (pool taken), 2 private (capture)
    hipEvent_t ev_fork = nullptr;
    int epi_v = 0;                         // EAMM_WINO4_EPI_V=1: timing experiment (wrong results): see conv_winograd4.hip DBG 30
    float* epi_scratch = nullptr;
    std::vector<hipEvent_t> ev_join;
    int cur_call_frames = 0;               // frames of the call being enqueued (all chains)
    int wino_tile = 4;                     // preferred output tile (EAMM_WINO_TILE): 4 -> F(4x4) where it applies, 2 -> F(2x2)
    int wino4_variant = 6;                 // wino4_gemm_kernel pipeline variant, 0 | 3 | 6 (3: one DMA piece per 8 MFMAs; 2.062 -> 2.047 ms per step vs
                                           // one per 4; 6 = 3 with the V stream loaded non-temporally where every GEMM workgroup of the call has a CU
                                           // of its own, 3 for larger calls: wino4_variant_for, eamm_forward.hip)
    bool wino4_variant_pinned = false;     // EAMM_WINO4_VARIANT set: that variant for every call size
    int cus = 256;                         // the device's CU count, read ONCE in eamm_create (the per-call launch rules size their splits by it)
    float* wino_v = nullptr;               // [16][F*hf*wf/4][Cb] (F(2x2)) or [36][F*hf*wf/16][Cb] transformed activations
    float* wino_z = nullptr;               // [24][F*hf*wf/16][Cb] x-folded products of the split F(4x4) form (few tiles)
    size_t wino_z_elems = 0;               // its size in floats
    int wino_min_m = 49152;                // smallest pixel count for which the bottleneck runs in Winograd F(2x2) form
    int wino4_min_m = 0;                   // ... in F(4x4) form: with the transform-point rows split over workgroups it wins from one frame up
    std::vector<float*> pre_s, pre_t;  // res-block pre-activation scale/shift (norm1)
    float* aa_w = nullptr;
    float* head_bias = nullptr;    // mask / occlusion biases when the head runs row-split (applied by the head kernel)
    int head_nc = 0;               // > 0: head is a 7x1 convolution over (dx, co), co < head_nc
    float* head_w_swz = nullptr;   // its weights with a 96-wide N tile in LDS-DMA layout (conv_col7s_kernel), or null
    float* final_bias = nullptr;   // bias of the final conv, applied by the shift-sum kernel
    float* final_part = nullptr;   // [F,H,W,32] (dx,co) partial products of the final 7x7 conv
    float* final_w_swz = nullptr;  // the 7x1 weights in LDS-DMA layout for the column-patch kernel (conv_col7.hip)
    float* final_w3 = nullptr;     // ... and as three bf16 planes (col7_pack_split_host): the fused launches run split-bf16 products
    int col7 = 1;                  // EAMM_COL7: 0 = im2col-style kernel for the final convolution
    int final_fused = 1;           // EAMM_FINAL_FUSED: 0 = partial products to HBM + final_shift_sum_kernel (round 2)
    int final_fused_min_rows = 128; // ... from this many rows of 16x16 tiles per call (EAMM_FINAL_FUSED_MIN_ROWS)
    int head_col7_min_tiles = 128; // fewest 16x16 tiles for which the flow head uses the column-patch kernel (EAMM_HEAD_COL7_MIN_TILES)

    // source cache (exportable): feat [S,hf,wf,Cb], src_small [S,h,w,4], src_full [S,3,H,W]
    float *feat = nullptr, *src_small = nullptr, *src_full = nullptr;
    // encoder temporaries
    float* src_nhwc = nullptr;
    std::vector<float*> enc_tmp;  // first output, then each down-block output except the last (= feat)
    // per-frame workspace
    float* kp_rec = nullptr;
    int* bad_flag = nullptr;
    float* hg_in = nullptr;
    std::vector<float*> e_buf, u_buf;
    float *logits = nullptr, *deformation = nullptr, *occlusion = nullptr;
    float *xa = nullptr, *xb = nullptr, *act = nullptr, *tmp = nullptr;
    std::vector<float*> up_buf;
    float* partial = nullptr;
    size_t partial_elems = 0;

    double flops_frame = 0, flops_encode = 0;

    PassProfile prof;

    // ---- training-mode forward (eamm_train_api.hip; SURVEY.md 8f row N4, second slice) ---------------------------------
    bool train_mode = false;               // eamm_set_training before finalisation: convolutions packed WITHOUT BatchNorm folded in
    float* raw = nullptr;                  // pre-BatchNorm convolution output of the site in flight (largest: F x H x W x down_c[1])
    float* train_sums = nullptr;           // the CALLER's [6 Cmax + 2] buffer: packed statistics of the site in flight (what the replicas all-reduce)
    float* train_stat = nullptr;           // [2 Cmax] mean, scale of the site in flight
    float* bn_work = nullptr;              // partial sums workspace
    int train_cmax = 0;
    std::vector<std::string> site_names;   // BatchNorm sites in execution order (state_dict prefixes)
    std::vector<std::function<int()>> steps;   // the forward as resumable steps; a step returns 1 when statistics await the
    size_t step_pc = 0;                        // caller's all-reduce, 0 to go on, < 0 on error
    int pending_c = 0;                     // channels of the site whose sums are pending
};

// ---- plan rules that more than one translation unit applies (the per-call rules live in eamm_forward.hip) ----------------

// F(4x4) with few tiles: the six rows of transform points are split over 6, 3 or 2 workgroups per 64 x 64 (tile, cout)
// block -- the largest split that still fits one round of the chip, one block per CU; 1 = no split.  A POOLED level (hourglass
// encoder, source down blocks) takes at least 2: its epilogue is the output-transform kernel's.
inline int wino4_row_split(const eamm_ctx* c, int tiles, int ntiles, bool pooled = false) {
    const int nblk = ((tiles + 63) / 64) * ntiles;
    for (int g : {6, 3, 2})
        if (nblk * g <= c->cus) return g;
    return pooled ? 2 : 1;
}

// Whole-pass chains in automatic mode (EAMM_PASS_CHAINS=0): two; four from 64 frames per call, where every chain still gets
// 16 (256x256: 4150 -> 4197 frames/s, profiles/r04_experiments.txt section 16; four chains of 8 at 32 frames gain nothing)
inline int auto_pass_chains(int frames) { return frames >= 64 ? 4 : 2; }
// ... and the most any call of this handle can use (pass_chains is clamped to 0..4 in eamm_create): one split-K slab and one
// stream per chain
inline int max_pass_chains(const eamm_ctx* c) { return c->pass_chains == 0 ? auto_pass_chains(c->cfg.max_frames) : c->pass_chains; }

// The ConvIO of a single-input convolution over B images of Hin x Win; a second input, residual, pooling ... are the caller's to add
inline ConvIO conv_io(const float* in0, int B, int Hin, int Win, int act, float* out, float* partial, size_t partial_cap) {
    ConvIO io{};
    io.in0 = in0;
    io.B = B;
    io.Hin = Hin;
    io.Win = Win;
    io.act = act;
    io.out = out;
    io.partial = partial;
    io.partial_cap = partial_cap;
    return io;
}

// The F(4x4) kernels address V ([36][tiles][Cin]) and Z ([24][tiles][Cout]) through 32-bit buffer descriptors
// (wino4_gemm_launch refuses from 0xFFFFF000 bytes): a call with more tiles than this takes the direct kernels.
inline bool wino4_fits(size_t tiles, int cin, int cout) {
    return 36.0 * tiles * cin * 4.0 < 4294963200.0 && 24.0 * tiles * cout * 4.0 < 4294963200.0;
}

// The slice of the per-frame workspace one launch sequence works on: frames [f0, f0 + n) of a call (every per-frame
// buffer is frame-major, so a slice is a pointer offset) with its own split-K slab and Winograd buffers.
struct FrameView {
    int n = 0, ns = 1;
    const float *kd_val = nullptr, *kd_jac = nullptr, *ks_val = nullptr, *ks_jac = nullptr;
    const float *feat = nullptr, *src_small = nullptr, *src_full = nullptr;
    float *kp_rec = nullptr, *hg_in = nullptr, *logits = nullptr, *deformation = nullptr, *occlusion = nullptr;
    float *xa = nullptr, *xb = nullptr, *act = nullptr, *tmp = nullptr, *final_part = nullptr;
    std::vector<float*> e_buf, u_buf, up_buf;
    float* partial = nullptr;
    size_t partial_elems = 0;
    float *wino_v = nullptr, *wino_z = nullptr;
    eamm_outputs out{};
};

// ---- defined in eamm_forward.hip for the other translation units ---------------------------------------------------------
// Side stream k of `device` from the pool every handle of the process shares (created on first use, never destroyed; null on
// failure); StreamLease leases the pool per call.
hipStream_t chain_stream(int device, int k);
// The view of frames [f0, f0 + n) of a call whose sources number ns_call (1, or one per frame), on split-K slab `slab`
FrameView make_view(const eamm_ctx* c, int f0, int n, int ns_call, int slab, const float* kd_val, const float* kd_jac,
                    const float* ks_val, const float* ks_jac, const eamm_outputs* o);
// The stages of the per-frame pass without a BatchNorm site inside: eamm_train_begin runs these same launch sequences between
// its own convolution / BatchNorm sites.  Each enqueues on s and returns an EAMM_* code.
int stage_motion_front(eamm_ctx* c, const FrameView& v, hipStream_t s);        // kp_prepare + motion_front
int stage_flow_head(eamm_ctx* c, const FrameView& v, hipStream_t s);           // 7x7 head conv + softmax / flow / sigmoid
int stage_warp(eamm_ctx* c, const FrameView& v, hipStream_t s, bool pre_act);  // features (+ r0's pre-activation) and 'deformed'
int stage_final(eamm_ctx* c, const FrameView& v, hipStream_t s);               // final 7x7 + sigmoid (+ uint8 frames)
// A pooled DownBlock2d level in F(4x4,3x3) form: whether it pays, by the caller's own rule, and its launches
enum class Wino4Pooled { HOURGLASS, SOURCE };
bool wino4_pooled_pays(const eamm_ctx* c, const WinoLayer& L, int tiles, Wino4Pooled caller);
int launch_wino4_pooled(eamm_ctx* c, const WinoLayer& L, const float* in, int n, int Hin, int Win, float* out, float* vbuf,
                        float* zbuf, hipStream_t s);
