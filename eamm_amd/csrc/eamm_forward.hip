// The per-frame half of OcclusionAwareGenerator.forward (reference modules/generator.py:64-97) behind the C ABI of
// include/eamm_hip.h:
//   eamm_forward_frames -- per frame batch: key-point records, motion front end, hourglass, flow head,
//                          feature warp, bottleneck, up blocks, final 7x7 + sigmoid
// with the rules that pick each stage's launch form for a call of n frames (ONE function per rule: the launch sequence and
// eamm_describe_plan both call it), the chains' stream pool, and the stage profile, whose layout is forward_view's.
#include "eamm_ctx.h"
#include <mutex>

// The chains' side streams come from a per-device pool shared by every handle of the process (created on first use, never
// destroyed): the runtime multiplexes streams onto a few hardware queues (four by default), and a second handle with its own
// three streams made two chains of one call share a queue -- measured: a 64-frame call's four chains 4199 frames/s alone, 4007
// beside another handle's streams.  The pool is LEASED for the duration of one call's enqueue (StreamLease below): a call that
// finds it taken by another host thread, or whose caller's stream is being captured into a HIP graph (the side streams join
// that capture until it ends, so nobody else may touch them meanwhile), runs on the handle's own private streams instead.
// Calls of different handles that follow one another on the pool share the streams' ORDER, never their dependencies: every
// call forks from and joins to its caller's stream with its own events.
namespace {
constexpr int POOL_MAXDEV = 64, POOL_MAXCHAIN = 15;
std::mutex g_pool_mu;
hipStream_t g_pool[POOL_MAXDEV][POOL_MAXCHAIN] = {};
std::mutex g_pool_lease[POOL_MAXDEV];

}  // namespace

hipStream_t chain_stream(int device, int k) {   // (declared in eamm_ctx.h: eamm_finalize_weights takes the handle's streams from here)
    if (device < 0 || device >= POOL_MAXDEV || k < 0 || k >= POOL_MAXCHAIN) return nullptr;
    std::lock_guard<std::mutex> lock(g_pool_mu);
    if (!g_pool[device][k] && hipStreamCreateWithFlags(&g_pool[device][k], hipStreamNonBlocking) != hipSuccess) g_pool[device][k] = nullptr;
    return g_pool[device][k];
}

namespace {

// Picks the side streams of ONE eamm_forward_frames call (c->side_streams) and holds the pool's lease while the call enqueues.
struct StreamLease {
    eamm_ctx* c;
    bool held = false;
    int rc = EAMM_OK;
    StreamLease(eamm_ctx* ctx, hipStream_t caller) : c(ctx) {
        if (c->pool_streams.empty()) return;   // a handle without chains
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(caller, &cap) != hipSuccess) {
            (void)hipGetLastError();
            cap = hipStreamCaptureStatusNone;
        }
        const bool capturing = cap != hipStreamCaptureStatusNone;
        const bool in_range = c->device >= 0 && c->device < POOL_MAXDEV;
        if (!capturing && !c->private_streams && in_range && g_pool_lease[c->device].try_lock()) {
            held = true;
            c->side_streams = c->pool_streams;
            c->last_streams = 0;
            return;
        }
        // (the private twins are created with the pool streams in eamm_finalize_weights, outside any capture)
        if (c->own_streams.size() < c->pool_streams.size()) {
            rc = fail(c, EAMM_ERR_STATE, "handle has no private chain streams (weights not finalized?)");
            return;
        }
        c->side_streams = c->own_streams;
        c->last_streams = capturing ? 2 : 1;
    }
    ~StreamLease() {
        if (held) g_pool_lease[c->device].unlock();
    }
};

// 0 = direct, 2 = Winograd F(2x2,3x3), 4 = Winograd F(4x4,3x3) for a call of n frames
int bottleneck_form(const eamm_ctx* c, int n) {
    const int hf = c->hf, wf = c->wf;
    if (c->wres1.empty()) return 0;
    const size_t px = (size_t)n * hf * wf;
    if (!c->w4res1.empty() && hf % 4 == 0 && wf % 4 == 0 && px >= (size_t)c->wino4_min_m) return 4;
    // F(2x2) tiles are the 2x2 pixel quads: odd map sides (a configuration eamm_create accepts) take the direct form
    return (px >= (size_t)c->wino_min_m && !(hf & 1) && !(wf & 1)) ? 2 : 0;
}

// Point-row split of the bottleneck's F(4x4) GEMMs for an unchained call of n frames (wino4_row_split, eamm_ctx.h)
int wino4_groups(const eamm_ctx* c, int n) { return wino4_row_split(c, n * (c->hf / 4) * (c->wf / 4), (c->Cb + 63) / 64); }

// GEMM variant 6 (= 3 with the V stream loaded non-temporally) pays only while all the GEMM workgroups of a call are co-resident,
// one per CU: the four cout workgroups of a tile row then pull a V line through the L2 together.  16 frames at 256x256 (two chains
// of 128 workgroups): + 0.3 %; 128 frames (four chains of 512): - 2 % (profiles/r05_experiments.txt 13) -- those keep variant 3.
int wino4_variant_for(const eamm_ctx* c, int call_frames) {
    if (c->wino4_variant != 6 || c->wino4_variant_pinned) return c->wino4_variant;
    const size_t wgs = (((size_t)call_frames * (c->hf / 4) * (c->wf / 4) + 63) / 64) * ((c->Cb + 63) / 64);
    return wgs <= (size_t)c->cus ? 6 : 3;
}

// Chains: the frames of a call are independent, so the F(4x4) bottleneck can run as K groups of frames on K streams.
// Each chain alternates an HBM-bound input transform with an MFMA-bound GEMM that fills 1/K of the chip; while one
// chain's transform streams through HBM the other chains' GEMMs own the matrix pipes, and a chain's transform moves only
// its share of the data -- measured at 16 frames, 256x256: bottleneck 2.74 -> 2.50 ms per step with K = 2 (K = 3, 4 lose
// it again to launch / queue overheads).  Every chain gets whole frames and a whole number of 64-tile GEMM blocks.
int bottleneck_chains(const eamm_ctx* c, int n) {
    if (bottleneck_form(c, n) != 4 || c->bneck_chains < 2 || c->side_streams.empty() || wino4_groups(c, n) != 1) return 1;
    int chains = std::min<int>(c->bneck_chains, (int)c->side_streams.size() + 1);
    const int tiles_pf = (c->hf / 4) * (c->wf / 4);
    while (chains > 1 && (n < chains || ((n / chains) * tiles_pf) % 64 != 0 || ((n / chains + 1) * tiles_pf) % 64 != 0)) --chains;
    return chains;
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

FrameView make_view(const eamm_ctx* c, int f0, int n, int ns_call, int slab, const float* kd_val, const float* kd_jac,
                           const float* ks_val, const float* ks_jac, const eamm_outputs* o) {
    FrameView v;
    const size_t F = (size_t)f0, K = c->K;
    const size_t HW = (size_t)c->H * c->W, hw = (size_t)c->h * c->w, hwf = (size_t)c->hf * c->wf;
    const size_t sf = ns_call > 1 ? F : 0;   // per-frame sources (the module's batch contract) move with the frames
    v.n = n;
    v.ns = ns_call > 1 ? n : 1;
    v.kd_val = kd_val + F * K * 2;
    v.kd_jac = kd_jac ? kd_jac + F * K * 4 : nullptr;
    v.ks_val = ks_val + sf * K * 2;
    v.ks_jac = ks_jac ? ks_jac + sf * K * 4 : nullptr;
    v.feat = c->feat + sf * hwf * c->Cb;
    v.src_small = c->src_small + sf * hw * 4;
    v.src_full = c->src_full + sf * c->Cpl * HW;
    v.kp_rec = c->kp_rec + F * K * KP_STRIDE;
    v.hg_in = c->hg_in ? c->hg_in + F * hw * c->Cp0 : nullptr;            // (no motion network: these four do not exist)
    for (int i = 0; i < c->nb; ++i) {
        v.e_buf.push_back(c->e_buf[i] + F * (hw >> (2 * (i + 1))) * c->enc_c[i]);
        v.u_buf.push_back(c->u_buf[i] + F * (hw >> (2 * (c->nb - 1 - i))) * c->dec_c[i]);
    }
    v.logits = c->logits ? c->logits + F * hw * (c->head_nc ? 128 : 32) : nullptr;
    v.deformation = c->deformation ? c->deformation + F * hw * 2 : nullptr;
    v.occlusion = c->occlusion ? c->occlusion + F * hw : nullptr;
    v.xa = c->xa + F * hwf * c->Cb;
    v.xb = c->xb + F * hwf * c->Cb;
    v.act = c->act + F * hwf * c->Cb;
    v.tmp = c->tmp + F * hwf * c->Cb;
    for (int i = 0; i < c->nd; ++i) v.up_buf.push_back(c->up_buf[i] + F * (hwf << (2 * (i + 1))) * c->up_c[i]);
    v.final_part = c->final_part + F * HW * 32;
    v.partial = c->partial + (size_t)slab * c->partial_elems;
    v.partial_elems = c->partial_elems;
    v.wino_v = c->wino_v ? c->wino_v + 4 * F * hwf * c->Cb : nullptr;                  // sized 4 x activations per frame
    v.wino_z = c->wino_z ? c->wino_z + 24 * (F * hwf / 16) * c->Cb : nullptr;
    v.out = *o;
    const size_t CO = c->Cimg > 3 ? c->Cimg : 3;   // channels of the tensors the pass writes (staging tensors for one or two)
    if (o->prediction) v.out.prediction = o->prediction + F * CO * HW;
    if (o->mask) v.out.mask = o->mask + F * (K + 1) * hw;
    if (o->sparse_deformed) v.out.sparse_deformed = o->sparse_deformed + F * (K + 1) * CO * hw;
    if (o->occlusion_map) v.out.occlusion_map = o->occlusion_map + F * hw;
    if (o->deformed) v.out.deformed = o->deformed + F * CO * HW;
    if (o->deformation) v.out.deformation = o->deformation + F * hw * 2;
    if (o->frames_u8) v.out.frames_u8 = o->frames_u8 + F * HW * 3;
    return v;
}

// Chains over the WHOLE per-frame pass: the frames of a call are independent, so a call of n frames can run as K launch
// sequences of n/K frames on K streams.  The sequences drift apart (the host enqueues them one after the other), and the
// chip then runs one chain's HBM- or latency-bound kernels (input transforms, warps, the small-grid deep hourglass levels
// and their split-K reductions) beside the other chain's MFMA-bound ones.  Needs the F(4x4) bottleneck with whole 64-tile
// GEMM blocks per chain; EAMM_PASS_CHAINS (0 / 1 = off).
int pass_chains(const eamm_ctx* c, int n) {
    const bool automatic = c->pass_chains == 0;
    const int tiles_pf = (c->hf / 4) * (c->wf / 4);
    auto fits = [&](int K) {
        if (K < 2 || (int)c->side_streams.size() + 1 < K) return false;
        if (n < c->pass_chains_min_frames || n < K) return false;
        if (automatic) {   // only while a chain's bottleneck GEMM keeps >= 80 one-per-CU blocks (measured 256x256, frames/s off -> on:
            // 8 frames = 64 blocks per chain 2981 -> 2397; 10: 2695 -> 2794; 12: 3018 -> 3105; 16: 3720 -> 3790; 24: 3716 -> 3864;
            // 32: 3871 -> 3980; 512x512 x 4: 941 -> 952, x 8: 985 -> 1006)
            if (((n / K) * tiles_pf / 64) * ((c->Cb + 63) / 64) < c->pass_chains_min_blocks) return false;
        }
        for (int k = 0; k < 2; ++k) {   // both chain sizes (n/K and n/K + 1 when n % K != 0)
            const int nk = n / K + k;
            if (k == 1 && n % K == 0) break;
            if (bottleneck_form(c, nk) != 4 || (nk * tiles_pf) % 64 != 0) return false;
        }
        return true;
    };
    if (!automatic) return fits(c->pass_chains) ? c->pass_chains : 1;
    if (auto_pass_chains(n) == 4 && fits(4)) return 4;   // (eamm_ctx.h)
    return fits(2) ? 2 : 1;
}

// Whether hourglass encoder level i runs in F(4x4,3x3) form (input transform, point-row-split GEMM, pooled output transform)
// in a launch sequence of n frames: the level was packed (eamm_finalize_weights), has enough 4x4 tiles -- four times as many
// where its transformed weights exceed ~100 MB (the 4x4-map level: 151 MB) -- and enough direct-form MFLOP (2 * 9 * 16 pixels
// per tile); smaller levels are launch-bound and one launch beats three
bool enc_level_wino4(const eamm_ctx* c, int i, int n) {
    if (i >= (int)c->w4enc.size() || !c->w4enc[i].Cout) return false;
    const WinoLayer& L = c->w4enc[i];
    const int tiles = n * ((c->h >> i) / 4) * ((c->w >> i) / 4);
    const bool heavy = 144.0 * L.Cin * L.Cout > 100e6;
    return tiles >= c->enc_wino_min_tiles * (heavy ? 4 : 1) && 288e-6 * tiles * L.Cin * L.Cout >= (double)c->enc_wino_min_mflop;
}

// Whether the final layer of a launch sequence of n frames takes the fused column-patch form (gather of the seven horizontal
// taps + bias + sigmoid in the tile epilogue), one workgroup per ROW of 16x16 tiles: only when those rows fill at least half the
// chip (measured 256x256: 16 frames 0.289 -> 0.283 ms per step, 65 MB written + read back per 8 frames gone; ONE frame has 16
// tile rows: 0.029 -> 0.262 ms, so small calls keep the two-kernel form)
bool final_is_fused(const eamm_ctx* c, int n) {
    return c->final_w_swz && c->final_conv.BN == 32 && c->final_fused && n * ((c->H + 15) / 16) >= c->final_fused_min_rows;
}

// One launch sequence over the frames of `v` on stream s.  `chained`: another sequence runs beside this one.
// phase: the whole pass, or its two halves around the feature warp (PH_PRE: key points ... flow head; PH_POST: warp ... final
// layer).  With `joint` (first chain's PH_POST) the warps run ONCE for all the call's frames -- the view `joint` -- and the
// other chains' PH_POST skip them and start behind c->ev_warp.
enum { PH_ALL = 0, PH_PRE = 1, PH_POST = 2 };
int forward_view(eamm_ctx* c, const FrameView& v, hipStream_t s, hipEvent_t* ev, bool chained, hipEvent_t* cev = nullptr,
                 int phase = PH_ALL, const FrameView* joint = nullptr) {
    const int n = v.n, ns = v.ns;
    const int h = c->h, w = c->w, hf = c->hf, wf = c->wf, K = c->K;
    const bool occ = c->cfg.estimate_occlusion_map != 0;
    // a convolution of this view's n frames at Hin x Win, on the view's split-K slab
    auto conv_for = [&](const float* in0, int Hin, int Win, int act, float* out) {
        return conv_io(in0, n, Hin, Win, act, out, v.partial, v.partial_elems);
    };
    // executed matrix-core flops launched since the last mark belong to the stage interval that ends here
    auto account = [&](int interval) {
        const double f = take_mfma_flops();
        c->call_flops += f;
        c->call_stage_flops[interval] += f;
        if (interval == 5) c->call_flops_bneck += f;
    };
#define STAGE_MARK(i)                                  \
    do {                                               \
        if ((i) > 0) account((i) - 1);                 \
        if (ev) {                                      \
            HIP_TRY(c, hipEventRecord(ev[i], s));      \
            c->prof_marks.back() = (i) + 1;            \
        }                                              \
    } while (0)
    const int nr = c->cfg.num_bottleneck_blocks;
    const int form = bottleneck_form(c, n);
    const bool wino = form != 0;
    if (c->nb == 0) {   // no motion network (generator.py:64 is false): the encoder features enter the bottleneck as they are
        STAGE_MARK(0); STAGE_MARK(1); STAGE_MARK(2); STAGE_MARK(3); STAGE_MARK(4);
        HIP_TRY(c, broadcast_features_launch(v.feat, n, ns, hf, wf, c->Cb, v.xa, wino ? nullptr : v.act, c->pre_s[0], c->pre_t[0], s));
        STAGE_MARK(5);
    } else {
    if (phase != PH_POST) {
    STAGE_MARK(0);
    // key-point records; 'jacobian' missing from kp_driving => identity (dense_motion.py:55)
    HIP_TRY(c, kp_prepare_launch(v.kd_val, v.kd_jac, v.ks_val, v.kd_jac ? v.ks_jac : nullptr, n, ns, K, v.kp_rec, c->bad_flag, s));
    // heat-maps + sparse motions + K+1 warped sources -> hourglass input     dense_motion.py:88-94
    HIP_TRY(c, motion_front_launch(v.kp_rec, v.src_small, n, ns, K, h, w, c->cfg.kp_variance, c->Cp0, v.hg_in,
                                   v.out.sparse_deformed, s, c->G, c->Cimg > 3 ? c->Cimg : 3, (size_t)c->cfg.max_sources * h * w * 4));
    STAGE_MARK(1);
    // hourglass encoder                                                       util.py:956-960
    for (int i = 0; i < c->nb; ++i) {
        ConvIO io = conv_for(i == 0 ? v.hg_in : v.e_buf[i - 1], h >> i, w >> i, ACT_RELU, v.e_buf[i]);
        io.pool = 1;
        if (enc_level_wino4(c, i, n)) {
            // F(4x4,3x3): 4x fewer MACs; the transform-point rows are split over workgroups (>= 2: the pooled epilogue is
            // the output-transform kernel's)
            const WinoLayer& L = c->w4enc[i];
            const int g = wino4_row_split(c, n * (io.Hin / 4) * (io.Win / 4), L.ntiles, true);
            HIP_TRY(c, wino4_transform_launch(io.in0, nullptr, nullptr, n, io.Hin, io.Win, L.Cin, v.wino_v, s));
            // pipeline variant 0 (one DMA piece per 4 MFMAs): within noise of the bottleneck's variant at these sizes, and a
            // different instantiation -- per-kernel averages in traces / PMC passes stay those of the bottleneck launches alone
            HIP_TRY(c, wino4_gemm_launch(L, v.wino_v, n, io.Hin, io.Win, ACT_RELU, nullptr, io.out, s, 0, g, v.wino_z, 1));
            continue;
        }
        HIP_TRY(c, conv_launch(pick(c, c->hg_enc[i], (size_t)n * io.Hin * io.Win), io, s));
    }
    STAGE_MARK(2);
    // hourglass decoder: nearest x2 and the skip concatenation are folded into the operand loader
    for (int i = 0; i < c->nb; ++i) {
        ConvIO io = conv_for(i == 0 ? v.e_buf[c->nb - 1] : v.u_buf[i - 1], h >> (c->nb - i), w >> (c->nb - i), ACT_RELU, v.u_buf[i]);
        io.in1 = i == 0 ? nullptr : v.e_buf[c->nb - 1 - i];
        if (int urc = launch_up(c, c->hg_dec[i], io, s)) return urc;
    }
    STAGE_MARK(3);
    // mask / occlusion logits, then softmax + flow combine + sigmoid         dense_motion.py:98-111
    {
        ConvIO io = conv_for(v.u_buf[c->nb - 1], h, w, ACT_NONE, v.logits);
        io.in1 = v.hg_in;
        ConvLayer head = c->head;
        float* defo = v.deformation;
        if (c->head_nc) {
            head.Cout = 128;  // partial products written with a 128-float pixel stride (7*nc used)
            // the column-patch kernel runs one workgroup per 16x16-pixel tile: below ~half a chip of tiles (4 frames at
            // 64x64) the split-K im2col kernel is faster (measured: 1 frame 0.122 -> 0.073 ms, 4 frames 0.122 -> 0.094 ms)
            const int head_tiles = n * ((h + 15) / 16) * ((w + 15) / 16);
            if (c->head_w_swz && head_tiles >= c->head_col7_min_tiles)
                HIP_TRY(c, conv_col7s_launch(io.in0, head.C0, io.in1, head.C1, n, h, w, c->head_w_swz, 3, v.logits, 128, s));
            else
                HIP_TRY(c, conv_launch(head, io, s));
            HIP_TRY(c, motion_head_rowsplit_launch(v.logits, 128, c->head_nc, c->head_bias, v.kp_rec, n, K, h, w,
                                                   occ ? 1 : 0, defo, v.occlusion, v.out.mask, v.out.occlusion_map, s));
        } else {
            head.Cout = 32;  // logits are written with a 32-float pixel stride; channels >= K+2 have zero weights
            HIP_TRY(c, conv_launch(head, io, s));
            HIP_TRY(c, motion_head_launch(v.logits, v.kp_rec, n, K, h, w, occ ? 1 : 0, defo, v.occlusion, v.out.mask,
                                          v.out.occlusion_map, s));
        }
        if (v.out.deformation)
            HIP_TRY(c, hipMemcpyAsync(v.out.deformation, defo, (size_t)n * h * w * 2 * sizeof(float),
                                      hipMemcpyDeviceToDevice, s));
    }
    }   // phase != PH_POST
    if (phase == PH_PRE) {
        account(3);
        return EAMM_OK;
    }
    if (phase == PH_POST && joint == nullptr) {
        HIP_TRY(c, hipStreamWaitEvent(s, c->ev_warp, 0));    // the first chain's launch warped this chain's frames as well
    } else {
        if (phase == PH_POST)   // every chain's flow is ready (the caller made this stream wait for the others' PH_PRE)
            for (size_t k = 0; k < c->ev_join.size(); ++k) HIP_TRY(c, hipStreamWaitEvent(s, c->ev_join[k], 0));
        STAGE_MARK(4);
        // feature warp x occlusion (+ r0's pre-activation for the direct form)       generator.py:79-84
        const FrameView& wv = joint ? *joint : v;
        HIP_TRY(c, warp_features_launch(wv.feat, wv.deformation, occ ? wv.occlusion : nullptr, wv.n, wv.ns, hf, wf, c->Cb, h, w,
                                        wv.xa, wino ? nullptr : wv.act, c->pre_s[0], c->pre_t[0], s));
        if (wv.out.deformed)                                                        // generator.py:86
            HIP_TRY(c, warp_image_launch(wv.src_full, wv.deformation, wv.n, wv.ns, c->H, c->W, h, w, wv.out.deformed, s, c->Cpl,
                                         c->Cimg > 3 ? c->Cimg : 3));
        if (joint) HIP_TRY(c, hipEventRecord(c->ev_warp, s));
        STAGE_MARK(5);
    }
    }
    // bottleneck                                                               generator.py:89
    float *x = v.xa, *xn = v.xb;
    if (cev) HIP_TRY(c, hipEventRecord(cev[0], s));
    hipEvent_t* sub = (ev && wino && 4 * nr + 1 <= eamm_ctx::NSUB) ? ev + eamm_ctx::NMARK + 1 : nullptr;
    int nsub = 0;
#define SUB_MARK()                                               \
    do {                                                         \
        if (sub) HIP_TRY(c, hipEventRecord(sub[nsub++], s));     \
    } while (0)
    const bool wino4 = form == 4;
    const int w4g = (wino4 && !chained) ? wino4_groups(c, n) : 1;   // a chained view shares the chip: never split the point rows
    // (round 5: splitting a whole-pass chain's bottleneck once more -- 2 x 2 sub-chains of 4 frames -- was built and measured
    //  neutral, 3917 vs 3958 frames/s: the input transform is latency-bound and does not shrink with the frames per launch;
    //  profiles/r05_experiments.txt section 2, git 9500c6c)
    const int chains = chained ? 1 : bottleneck_chains(c, n);
    const int w4var = wino4_variant_for(c, chained ? c->cur_call_frames : n);
    auto split_stream = [&](int k) { return c->side_streams[k - 1]; };
    hipEvent_t split_fork = c->ev_fork;
    auto split_join = [&](int k) { return c->ev_join[k - 1]; };
    if (chains > 1) {
        const size_t per_frame = (size_t)hf * wf * c->Cb;
        const int nbase = n / chains, nrem = n % chains;   // the first nrem chains take one more frame
        HIP_TRY(c, hipEventRecord(split_fork, s));
        for (int k = 1; k < chains; ++k) HIP_TRY(c, hipStreamWaitEvent(split_stream(k), split_fork, 0));
        for (int i = 0; i < nr; ++i) {
            for (int k = 0; k < chains; ++k) {
                hipStream_t sk = k ? split_stream(k) : s;
                const int nk = nbase + (k < nrem ? 1 : 0);
                const size_t f0 = (size_t)k * nbase + std::min(k, nrem);
                float* xk = x + f0 * per_frame;
                float* xnk = xn + f0 * per_frame;
                float* tk = v.tmp + f0 * per_frame;
                float* vk = v.wino_v + 4 * f0 * per_frame;   // 2.25 nk frames used of the 4 nk reserved for this chain
                // events around the main stream's (chain 0's) kernels only: they time those launches while the other
                // chains' run beside them
                if (k == 0) SUB_MARK();
                HIP_TRY(c, wino4_transform_launch(xk, c->pre_s[i], c->pre_t[i], nk, hf, wf, c->Cb, vk, sk));
                if (k == 0) SUB_MARK();
                HIP_TRY(c, wino4_gemm_launch(c->w4res1[i], vk, nk, hf, wf, ACT_RELU, nullptr, tk, sk, w4var, 1, nullptr));
                if (k == 0) SUB_MARK();
                HIP_TRY(c, wino4_transform_launch(tk, nullptr, nullptr, nk, hf, wf, c->Cb, vk, sk));
                if (k == 0) SUB_MARK();
                HIP_TRY(c, wino4_gemm_launch(c->w4res2[i], vk, nk, hf, wf, ACT_NONE, xk, xnk, sk, w4var, 1, nullptr));
            }
            std::swap(x, xn);
        }
        SUB_MARK();
        for (int k = 1; k < chains; ++k) {
            HIP_TRY(c, hipEventRecord(split_join(k), split_stream(k)));
            HIP_TRY(c, hipStreamWaitEvent(s, split_join(k), 0));
        }
    }
    for (int i = 0; i < nr && wino && chains == 1; ++i) {
        // conv1(relu(norm1(x))): the pre-activation rides on the input transform; norm2 + relu in the epilogue
        SUB_MARK();
        if (wino4) {
            // EAMM_WINO4_EPI_V (timing experiment, wrong results): only the stage's FIRST transform runs (every GEMM then reads that
            // V: realistic operand values), and the GEMMs' epilogues write V-sized extra output instead (variant 50)
            const bool epi = c->epi_v && c->epi_scratch && w4g == 1;
            float* escr = epi ? c->epi_scratch + (size_t)3 * (v.xa - c->xa) : v.wino_z;
            const int wvar = epi ? 50 : w4var;
            if (!epi || i == 0) HIP_TRY(c, wino4_transform_launch(x, c->pre_s[i], c->pre_t[i], n, hf, wf, c->Cb, v.wino_v, s));
            SUB_MARK();
            HIP_TRY(c, wino4_gemm_launch(c->w4res1[i], v.wino_v, n, hf, wf, ACT_RELU, nullptr, v.tmp, s, wvar, w4g, escr));
            SUB_MARK();
            if (!epi) HIP_TRY(c, wino4_transform_launch(v.tmp, nullptr, nullptr, n, hf, wf, c->Cb, v.wino_v, s));
            SUB_MARK();
            HIP_TRY(c, wino4_gemm_launch(c->w4res2[i], v.wino_v, n, hf, wf, ACT_NONE, x, xn, s, wvar, w4g, escr));   // out += x
        } else {
            HIP_TRY(c, wino_transform_launch(x, c->pre_s[i], c->pre_t[i], n, hf, wf, c->Cb, v.wino_v, s));
            SUB_MARK();
            HIP_TRY(c, wino_gemm_launch(c->wres1[i], v.wino_v, n, hf, wf, ACT_RELU, nullptr, v.tmp, s));
            SUB_MARK();
            HIP_TRY(c, wino_transform_launch(v.tmp, nullptr, nullptr, n, hf, wf, c->Cb, v.wino_v, s));
            SUB_MARK();
            HIP_TRY(c, wino_gemm_launch(c->wres2[i], v.wino_v, n, hf, wf, ACT_NONE, x, xn, s));   // out += x
        }
        std::swap(x, xn);
    }
    if (chains == 1) SUB_MARK();
#undef SUB_MARK
    if (sub) c->prof_sub.back() = nsub;
    for (int i = 0; i < nr && !wino; ++i) {
        const ConvIO a = conv_for(v.act, hf, wf, ACT_RELU, v.tmp);  // conv1 -> norm2 (folded) -> relu
        HIP_TRY(c, conv_launch(pick(c, c->res1[i], (size_t)n * hf * wf), a, s));
        ConvIO b = conv_for(v.tmp, hf, wf, ACT_NONE, xn);
        b.resid = x;       // out += x
        if (i + 1 < nr) {  // next block's relu(norm1(.))
            b.out2 = v.act;
            b.s2 = c->pre_s[i + 1];
            b.t2 = c->pre_t[i + 1];
        }
        HIP_TRY(c, conv_launch(pick(c, c->res2[i], (size_t)n * hf * wf), b, s));
        std::swap(x, xn);
    }
    STAGE_MARK(6);
    if (cev) HIP_TRY(c, hipEventRecord(cev[1], s));
    // up blocks                                                                generator.py:90-91
    const float* cur = x;
    for (int i = 0; i < c->nd; ++i) {
        if (int urc = launch_up(c, c->up[i], conv_for(cur, hf << i, wf << i, ACT_RELU, v.up_buf[i]), s)) return urc;
        cur = v.up_buf[i];
    }
    STAGE_MARK(7);
    // final 7x7 + sigmoid, written NCHW straight into the caller's buffer      generator.py:92-93
    {
        ConvIO io = conv_for(cur, c->H, c->W, ACT_NONE, v.final_part);
        if (c->Cimg > 3) {   // plain 7x7 kernel, sigmoid + NCHW store in the epilogue, straight into the caller's [n,C,H,W]
            io.act = ACT_SIGMOID;
            io.nchw = 1;
            io.out = v.out.prediction;
            HIP_TRY(c, conv_launch(c->final_conv, io, s));
            account(7);
            return EAMM_OK;
        }
        ConvLayer fl = c->final_conv;
        fl.Cout = 32;  // 32-float pixel stride; channels >= 21 have zero weights
        if (final_is_fused(c, n)) {
            HIP_TRY(c, conv_col7_fused_launch(cur, fl.C0, n, c->H, c->W, c->final_w_swz, c->final_bias, v.out.prediction, s));
        } else {
            if (c->final_w_swz && fl.BN == 32)
                HIP_TRY(c, conv_col7_launch(cur, fl.C0, n, c->H, c->W, c->final_w_swz, v.final_part, s));
            else
                HIP_TRY(c, conv_launch(fl, io, s));
            HIP_TRY(c, final_shift_sum_launch(v.final_part, c->final_bias, n, c->H, c->W, v.out.prediction, s));
        }
    }
    if (v.out.frames_u8) HIP_TRY(c, to_u8_launch(v.out.prediction, n, c->H, c->W, v.out.frames_u8, s));
    account(7);
#undef STAGE_MARK
    return EAMM_OK;   // (the caller records the last stage mark, after joining the chains)
}

}  // namespace

// -------------------------------------------------------------------------------------------------
extern "C" {

int eamm_forward_frames(eamm_ctx* c, int n, const float* kd_val, const float* kd_jac, const float* ks_val,
                        const float* ks_jac, const eamm_outputs* o, void* stream_) {
    if (!c || !kd_val || !ks_val || !o || !o->prediction) return fail(c, EAMM_ERR_ARG, "null argument");
    if (!c->finalized) return fail(c, EAMM_ERR_STATE, "call eamm_finalize_weights first");
    if (c->ns_cached < 1) return fail(c, EAMM_ERR_STATE, "no source cached: call eamm_encode_source first");
    if (n < 1 || n > c->cfg.max_frames) return fail(c, EAMM_ERR_ARG, "n=%d outside [1,%d]", n, c->cfg.max_frames);
    if (kd_jac != nullptr && ks_jac == nullptr)
        return fail(c, EAMM_ERR_ARG, "kp_driving jacobian given without kp_source jacobian");
    const int ns = c->ns_cached;
    if (ns != 1 && ns != n) return fail(c, EAMM_ERR_ARG, "%d cached sources cannot serve %d frames (need 1 or n)", ns, n);
    if ((o->occlusion_map) && !c->cfg.estimate_occlusion_map)
        return fail(c, EAMM_ERR_ARG, "occlusion_map requested but estimate_occlusion_map is off");
    if (c->nb == 0 && (o->mask || o->sparse_deformed || o->deformed || o->deformation))
        return fail(c, EAMM_ERR_ARG, "this generator has no motion network: only 'prediction' exists (generator.py:64-95)");
    DeviceGuard guard(c->device);
    if (guard.status != hipSuccess) return fail(c, EAMM_ERR_HIP, "hipSetDevice(%d) failed", c->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream_);
    const eamm_outputs* const user = o;
    eamm_outputs staged = *o;
    if (o->frames_u8 && c->Cimg != 3) return fail(c, EAMM_ERR_ARG, "uint8 RGB frames need num_channels == 3");
    if (c->Cimg < 3) {   // one or two image channels: the pass writes three-channel staging tensors (eamm_ctx.h: Cimg)
        if (o->frames_u8) return fail(c, EAMM_ERR_ARG, "uint8 RGB frames need num_channels == 3");
        staged.prediction = c->stage_pred;
        if (o->deformed) staged.deformed = c->stage_deformed;
        if (o->sparse_deformed) staged.sparse_deformed = c->stage_sparse;
        o = &staged;
    }

    StreamLease lease(c, s);
    if (lease.rc) return lease.rc;
    hipEvent_t* ev = nullptr;  // stage boundaries (of the main stream's sequence), recorded only while profiling
    hipEvent_t* cev = nullptr; // bottleneck window of every whole-pass chain
    const int chains = pass_chains(c, n);
    c->cur_pass_chains = chains;
    c->cur_call_frames = n;
    if (c->profiling && c->prof_used < eamm_ctx::PROF_CALLS) {
        ev = c->prof_events.data() + (size_t)c->prof_used * (eamm_ctx::NMARK + 1 + eamm_ctx::NSUB);
        cev = c->prof_chain_ev.data() + (size_t)c->prof_used * eamm_ctx::MAXCHAIN * 2;
        c->prof_n.push_back(n);
        c->prof_sub.push_back(0);
        c->prof_marks.push_back(0);
        c->prof_nchain.push_back(std::min(chains, (int)eamm_ctx::MAXCHAIN));
        c->prof_flops.push_back(0.0);
        c->prof_flops_bneck.push_back(0.0);
        ++c->prof_used;
    }
    (void)take_mfma_flops();
    c->call_flops = c->call_flops_bneck = 0.0;
    for (double& f : c->call_stage_flops) f = 0.0;
    if (chains == 1) {
        if (int rc = forward_view(c, make_view(c, 0, n, ns, 0, kd_val, kd_jac, ks_val, ks_jac, o), s, ev, false, cev)) return rc;
    } else {
        const int nbase = n / chains, nrem = n % chains;   // the first nrem chains take one more frame
        HIP_TRY(c, hipEventRecord(c->ev_fork, s));
        for (int k = 1; k < chains; ++k) HIP_TRY(c, hipStreamWaitEvent(c->side_streams[k - 1], c->ev_fork, 0));
        // EAMM_WARP_JOINT: the chains meet once, after their flow heads: ONE warp launch over all frames (an HBM-bound kernel
        // that fills the chip alone; per chain it runs beside the other chain's kernels at half the rate), then they part again
        const bool joint = c->warp_joint && c->nb > 0 && c->ev_warp != nullptr;
        for (int pass = 0; pass < (joint ? 2 : 1); ++pass) {
            for (int k = 0; k < chains; ++k) {
                const int nk = nbase + (k < nrem ? 1 : 0), f0 = k * nbase + std::min(k, nrem);
                const FrameView v = make_view(c, f0, nk, ns, k, kd_val, kd_jac, ks_val, ks_jac, o);
                const FrameView all = make_view(c, 0, n, ns, 0, kd_val, kd_jac, ks_val, ks_jac, o);
                hipStream_t sk = k ? c->side_streams[k - 1] : s;
                if (int rc = forward_view(c, v, sk, k ? nullptr : ev, true, (cev && k < eamm_ctx::MAXCHAIN) ? cev + 2 * k : nullptr,
                                          joint ? (pass == 0 ? PH_PRE : PH_POST) : PH_ALL, (joint && pass == 1 && k == 0) ? &all : nullptr))
                    return rc;
                if (joint && pass == 0 && k > 0) HIP_TRY(c, hipEventRecord(c->ev_join[k - 1], sk));
            }
        }
        for (int k = 1; k < chains; ++k) {
            HIP_TRY(c, hipEventRecord(c->ev_join[k - 1], c->side_streams[k - 1]));
            HIP_TRY(c, hipStreamWaitEvent(s, c->ev_join[k - 1], 0));
        }
    }
    if (c->Cimg < 3) {   // the real channels of every frame: rows of C planes out of rows of three
        const size_t HW = (size_t)c->H * c->W * sizeof(float), hw = (size_t)c->h * c->w * sizeof(float), C = (size_t)c->Cimg;
        HIP_TRY(c, hipMemcpy2DAsync(user->prediction, C * HW, c->stage_pred, 3 * HW, C * HW, (size_t)n, hipMemcpyDeviceToDevice, s));
        if (user->deformed)
            HIP_TRY(c, hipMemcpy2DAsync(user->deformed, C * HW, c->stage_deformed, 3 * HW, C * HW, (size_t)n, hipMemcpyDeviceToDevice, s));
        if (user->sparse_deformed)
            HIP_TRY(c, hipMemcpy2DAsync(user->sparse_deformed, C * hw, c->stage_sparse, 3 * hw, C * hw, (size_t)n * (c->K + 1),
                                        hipMemcpyDeviceToDevice, s));
    }
    if (ev) {   // the last stage ends where the call ends (after the join)
        HIP_TRY(c, hipEventRecord(ev[eamm_ctx::NMARK], s));
        c->prof_marks.back() = eamm_ctx::NMARK + 1;
        c->prof_flops.back() = c->call_flops;
        c->prof_flops_bneck.back() = c->call_flops_bneck;
        for (int i = 0; i < eamm_ctx::NMARK; ++i)
            c->prof_stage_flops[(size_t)(c->prof_used - 1) * eamm_ctx::NMARK + i] = c->call_stage_flops[i];
    }
    return EAMM_OK;
}

int eamm_profile_enable(eamm_ctx* c, int on) {
    if (!c) return EAMM_ERR_ARG;
    DeviceGuard guard(c->device);
    if (guard.status != hipSuccess) return fail(c, EAMM_ERR_HIP, "hipSetDevice(%d) failed", c->device);
    if (on && c->prof_events.empty()) {
        c->prof_events.resize((size_t)eamm_ctx::PROF_CALLS * (eamm_ctx::NMARK + 1 + eamm_ctx::NSUB));
        for (auto& e : c->prof_events) HIP_TRY(c, hipEventCreate(&e));
        c->prof_chain_ev.resize((size_t)eamm_ctx::PROF_CALLS * eamm_ctx::MAXCHAIN * 2);
        for (auto& e : c->prof_chain_ev) HIP_TRY(c, hipEventCreate(&e));
        c->prof_stage_flops.assign((size_t)eamm_ctx::PROF_CALLS * eamm_ctx::NMARK, 0.0);
    }
    c->profiling = on != 0;
    return EAMM_OK;
}

int eamm_profile_read(eamm_ctx* c, double* stage_ms, int nstage, int64_t* calls, int64_t* frames, int reset) {
    if (!c || !stage_ms || nstage != eamm_ctx::NSTAGE) return fail(c, EAMM_ERR_ARG, "nstage must be %d", eamm_ctx::NSTAGE);
    DeviceGuard guard(c->device);
    if (guard.status != hipSuccess) return fail(c, EAMM_ERR_HIP, "hipSetDevice(%d) failed", c->device);
    // stage index of each of the NMARK recorded intervals; the bottleneck interval (5) is split below
    static const int stage_of[eamm_ctx::NMARK] = {0, 1, 2, 3, 4, 6, 7, 8};
    int dropped = 0;
    for (int k = 0; k < c->prof_used; ++k) {  // fold finished event sets into the totals
        hipEvent_t* ev = c->prof_events.data() + (size_t)k * (eamm_ctx::NMARK + 1 + eamm_ctx::NSUB);
        // a call that failed midway leaves a partly recorded set: skip it (its events are re-recorded by a later call)
        bool ok = c->prof_marks[k] == eamm_ctx::NMARK + 1 && hipEventSynchronize(ev[eamm_ctx::NMARK]) == hipSuccess;
        double ms_set[eamm_ctx::NSTAGE] = {0};
        for (int i = 0; ok && i < eamm_ctx::NMARK; ++i) {
            float ms = 0.f;
            ok = hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess;
            ms_set[stage_of[i]] += ms;
        }
        const int nsub = c->prof_sub[k];
        if (ok && nsub > 1) {  // Winograd form: even intervals are input transforms, odd ones the GEMM kernels
            hipEvent_t* sub = ev + eamm_ctx::NMARK + 1;
            double tr = 0;
            for (int i = 0; ok && i + 1 < nsub; i += 2) {
                float ms = 0.f;
                ok = hipEventElapsedTime(&ms, sub[i], sub[i + 1]) == hipSuccess;
                tr += ms;
            }
            ms_set[5] += tr;
            ms_set[6] -= tr;
            for (int i = 1; ok && i + 1 < nsub; i += 2) {   // the GEMM kernels' own durations on the main stream
                float ms = 0.f;
                ok = hipEventElapsedTime(&ms, sub[i], sub[i + 1]) == hipSuccess;
                ms_set[9] += ms;
            }
        }
        if (ok) {   // bottleneck windows of the whole-pass chains, on the clock of this call's first event
            hipEvent_t* cv = c->prof_chain_ev.data() + (size_t)k * eamm_ctx::MAXCHAIN * 2;
            const int nc = c->prof_nchain[k];
            float t0[eamm_ctx::MAXCHAIN], t1[eamm_ctx::MAXCHAIN];
            for (int j = 0; ok && j < nc; ++j)
                ok = hipEventSynchronize(cv[2 * j + 1]) == hipSuccess && hipEventElapsedTime(&t0[j], ev[0], cv[2 * j]) == hipSuccess &&
                     hipEventElapsedTime(&t1[j], ev[0], cv[2 * j + 1]) == hipSuccess;
            if (ok) {
                int order[eamm_ctx::MAXCHAIN];
                for (int j = 0; j < nc; ++j) order[j] = j;
                std::sort(order, order + nc, [&](int a, int b) { return t0[a] < t0[b]; });
                double uni = 0, sum = 0, cur0 = 0, cur1 = -1;
                for (int q = 0; q < nc; ++q) {
                    const int j = order[q];
                    sum += t1[j] - t0[j];
                    if (cur1 < cur0 || t0[j] > cur1) {   // a new disjoint interval
                        if (cur1 >= cur0) uni += cur1 - cur0;
                        cur0 = t0[j];
                        cur1 = t1[j];
                    } else {
                        cur1 = std::max<double>(cur1, t1[j]);
                    }
                }
                if (cur1 >= cur0) uni += cur1 - cur0;
                ms_set[10] = uni;
                ms_set[11] = sum;
                ms_set[12] = c->prof_flops[k] * 1e-9;
                ms_set[13] = c->prof_flops_bneck[k] * 1e-9;
                for (int i = 0; i < eamm_ctx::NMARK; ++i) ms_set[14 + i] = c->prof_stage_flops[(size_t)k * eamm_ctx::NMARK + i] * 1e-9;
            }
        }
        if (!ok) {
            (void)hipGetLastError();
            ++dropped;
            continue;
        }
        for (int i = 0; i < eamm_ctx::NSTAGE; ++i) c->prof_ms[i] += ms_set[i];
        c->prof_calls += 1;
        c->prof_frames += c->prof_n[k];
    }
    (void)dropped;
    c->prof_used = 0;
    c->prof_n.clear();
    c->prof_sub.clear();
    c->prof_marks.clear();
    c->prof_nchain.clear();
    c->prof_flops.clear();
    c->prof_flops_bneck.clear();
    for (int i = 0; i < nstage; ++i) stage_ms[i] = c->prof_ms[i];
    if (calls) *calls = c->prof_calls;
    if (frames) *frames = c->prof_frames;
    if (reset) {
        for (double& v : c->prof_ms) v = 0;
        c->prof_calls = c->prof_frames = 0;
    }
    return EAMM_OK;
}

int eamm_bottleneck_form(const eamm_ctx* c, int n) { return (c && n > 0) ? bottleneck_form(c, n) : EAMM_ERR_ARG; }
int eamm_bottleneck_chains(const eamm_ctx* c, int n) {
    if (!c || n <= 0) return EAMM_ERR_ARG;
    const int whole = pass_chains(c, n);   // chains over the whole pass take precedence over chains inside the bottleneck
    return whole > 1 ? whole : bottleneck_chains(c, n);
}
int eamm_pass_chains(const eamm_ctx* c, int n) {
    if (!c || n <= 0) return EAMM_ERR_ARG;
    return pass_chains(c, n);
}
int eamm_last_stream_set(const eamm_ctx* c) { return c ? c->last_streams : EAMM_ERR_ARG; }
int eamm_describe_plan(const eamm_ctx* c, int n, char* buf, int cap) {
    if (!c || n <= 0 || n > c->cfg.max_frames || !c->finalized) return EAMM_ERR_ARG;
    const int pc = pass_chains(c, n), nk = pc > 1 ? n / pc : n;
    const int form = bottleneck_form(c, nk), bc = pc > 1 ? pc : bottleneck_chains(c, n);
    std::string enc = "[";
    for (int i = 0; i < c->nb; ++i)   // (per launch sequence: one chain's frames)
        enc += std::string(i ? ", " : "") + (enc_level_wino4(c, i, nk) ? "\"wino4\"" : "\"direct\"");
    enc += "]";
    char tmp[1024];
    const int len = snprintf(tmp, sizeof tmp,
                             "{\"frames\": %d, \"pass_chains\": %d, \"frames_per_chain\": %d, \"bottleneck_form\": %d, \"bottleneck_chains\": %d, "
                             "\"wino4_groups\": %d, \"wino4_variant\": %d, \"hg_encoder\": %s, \"final\": \"%s\", \"warp_joint\": %d, "
                             "\"side_streams\": %d, \"experiments_build\": %d}",
                             n, pc, nk, form, bc, (form == 4 && pc == 1 && bc == 1) ? wino4_groups(c, n) : 1, wino4_variant_for(c, n), enc.c_str(),
                             final_is_fused(c, nk) ? "col7q fused" : "col7 + shift-sum", c->warp_joint, (int)c->pool_streams.size(),
                             eamm_build_experiments());
    if (buf && cap > 0) {
        const int m = std::min(len, cap - 1);
        std::memcpy(buf, tmp, (size_t)m);
        buf[m] = 0;
    }
    return len;
}

}  // extern "C"
