// The per-frame half of OcclusionAwareGenerator.forward (reference modules/generator.py:64-97) behind the C ABI of
// include/eamm_hip.h:
//   eamm_forward_frames -- per frame batch: key-point records, motion front end, hourglass, flow head,
//                          feature warp, bottleneck, up blocks, final 7x7 + sigmoid
// In this order: the chains' stream pool and make_view; the rules that pick each stage's launch form for a call of n frames (ONE
// function per rule: the launch sequence and eamm_describe_plan both call it); ONE function per stage (eamm_ctx.h declares those
// that eamm_train_begin and eamm_encode_source share); forward_view, the sequence of stage marks and stage calls; PassProfile.
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

FrameView make_view(const eamm_ctx* c, int f0, int n, int ns_call, int slab, const float* kd_val, const float* kd_jac,
                    const float* ks_val, const float* ks_jac, const eamm_outputs* o) {   // (FrameView: eamm_ctx.h)
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

// Whether hourglass encoder level i runs in F(4x4,3x3) form in a launch sequence of n frames (wino4_pooled_pays below)
bool enc_level_wino4(const eamm_ctx* c, int i, int n) {
    if (i >= (int)c->w4enc.size()) return false;
    return wino4_pooled_pays(c, c->w4enc[i], n * ((c->h >> i) / 4) * ((c->w >> i) / 4), Wino4Pooled::HOURGLASS);
}

// Whether the final layer of a launch sequence of n frames takes the fused column-patch form (gather of the seven horizontal
// taps + bias + sigmoid in the tile epilogue), one workgroup per ROW of 16x16 tiles: only when those rows fill at least half the
// chip (measured 256x256: 16 frames 0.289 -> 0.283 ms per step, 65 MB written + read back per 8 frames gone; ONE frame has 16
// tile rows: 0.029 -> 0.262 ms, so small calls keep the two-kernel form)
bool final_is_fused(const eamm_ctx* c, int n) {
    return c->final_w_swz && c->final_conv.BN == 32 && c->final_fused && n * ((c->H + 15) / 16) >= c->final_fused_min_rows;
}

// a convolution of the view's n frames at Hin x Win, on the view's split-K slab
ConvIO conv_for(const FrameView& v, const float* in0, int Hin, int Win, int act, float* out) {
    return conv_io(in0, v.n, Hin, Win, act, out, v.partial, v.partial_elems);
}

}  // namespace

// ---- the stages: each enqueues one stage of the pass for the frames of `v` on stream s ----------------------------------
// Whether a pooled DownBlock2d level runs in F(4x4,3x3) form (input transform, point-row-split GEMM, pooled output transform)
// for a launch of `tiles` 4x4 tiles: the level was packed (eamm_finalize_weights), has enough tiles and enough direct-form
// MFLOP (2 * 9 * 16 pixels per tile); smaller levels are launch-bound and one launch beats three.  The two callers' rules
// differ and stay apart on purpose (unifying them would change which kernel runs for widths beyond the shipped ones): HOURGLASS
// asks four times the tiles where the transformed weights exceed ~100 MB (the 4x4-map level: 151 MB); SOURCE borrows
// workspaces sized for the frames, so they must exist and the tiles must fit their 32-bit descriptors (wino4_fits).
bool wino4_pooled_pays(const eamm_ctx* c, const WinoLayer& L, int tiles, Wino4Pooled caller) {
    if (!L.Cout) return false;
    const int min_tiles = c->enc_wino_min_tiles * (caller == Wino4Pooled::HOURGLASS && 144.0 * L.Cin * L.Cout > 100e6 ? 4 : 1);
    if (caller == Wino4Pooled::SOURCE && !(c->wino_v && c->wino_z && wino4_fits((size_t)tiles, L.Cin, L.Cout))) return false;
    return tiles >= min_tiles && 288e-6 * tiles * L.Cin * L.Cout >= (double)c->enc_wino_min_mflop;
}

int launch_wino4_pooled(eamm_ctx* c, const WinoLayer& L, const float* in, int n, int Hin, int Win, float* out, float* vbuf,
                        float* zbuf, hipStream_t s) {
    // F(4x4,3x3): 4x fewer MACs; the transform-point rows are split over workgroups (>= 2: the pooled epilogue is the
    // output-transform kernel's)
    const int g = wino4_row_split(c, n * (Hin / 4) * (Win / 4), L.ntiles, true);
    HIP_TRY(c, wino4_transform_launch(in, nullptr, nullptr, n, Hin, Win, L.Cin, vbuf, s));
    // pipeline variant 0 (one DMA piece per 4 MFMAs): within noise of the bottleneck's variant at these sizes, and a
    // different instantiation -- per-kernel averages in traces / PMC passes stay those of the bottleneck launches alone
    HIP_TRY(c, wino4_gemm_launch(L, vbuf, n, Hin, Win, ACT_RELU, nullptr, out, s, 0, g, zbuf, 1));
    return EAMM_OK;
}

int stage_motion_front(eamm_ctx* c, const FrameView& v, hipStream_t s) {
    // key-point records; 'jacobian' missing from kp_driving => identity (dense_motion.py:55)
    HIP_TRY(c, kp_prepare_launch(v.kd_val, v.kd_jac, v.ks_val, v.kd_jac ? v.ks_jac : nullptr, v.n, v.ns, c->K, v.kp_rec, c->bad_flag, s));
    // heat-maps + sparse motions + K+1 warped sources -> hourglass input     dense_motion.py:88-94
    HIP_TRY(c, motion_front_launch(v.kp_rec, v.src_small, v.n, v.ns, c->K, c->h, c->w, c->cfg.kp_variance, c->Cp0, v.hg_in,
                                   v.out.sparse_deformed, s, c->G, c->Cimg > 3 ? c->Cimg : 3, (size_t)c->cfg.max_sources * c->h * c->w * 4));
    return EAMM_OK;
}

static int stage_hg_encoder(eamm_ctx* c, const FrameView& v, hipStream_t s) {   // util.py:956-960
    for (int i = 0; i < c->nb; ++i) {
        ConvIO io = conv_for(v, i == 0 ? v.hg_in : v.e_buf[i - 1], c->h >> i, c->w >> i, ACT_RELU, v.e_buf[i]);
        io.pool = 1;
        if (enc_level_wino4(c, i, v.n)) {
            if (int rc = launch_wino4_pooled(c, c->w4enc[i], io.in0, v.n, io.Hin, io.Win, io.out, v.wino_v, v.wino_z, s)) return rc;
            continue;
        }
        HIP_TRY(c, conv_launch(pick(c, c->hg_enc[i], (size_t)v.n * io.Hin * io.Win), io, s));
    }
    return EAMM_OK;
}

// nearest x2 and the skip concatenation are folded into the operand loader
static int stage_hg_decoder(eamm_ctx* c, const FrameView& v, hipStream_t s) {
    const int nb = c->nb;
    for (int i = 0; i < nb; ++i) {
        ConvIO io = conv_for(v, i == 0 ? v.e_buf[nb - 1] : v.u_buf[i - 1], c->h >> (nb - i), c->w >> (nb - i), ACT_RELU, v.u_buf[i]);
        io.in1 = i == 0 ? nullptr : v.e_buf[nb - 1 - i];
        if (int rc = launch_up(c, c->hg_dec[i], io, s)) return rc;
    }
    return EAMM_OK;
}

// mask / occlusion logits, then softmax + flow combine + sigmoid         dense_motion.py:98-111
int stage_flow_head(eamm_ctx* c, const FrameView& v, hipStream_t s) {
    const int n = v.n, h = c->h, w = c->w, K = c->K;
    const int occ = c->cfg.estimate_occlusion_map ? 1 : 0;
    ConvIO io = conv_for(v, v.u_buf[c->nb - 1], h, w, ACT_NONE, v.logits);
    io.in1 = v.hg_in;
    ConvLayer head = c->head;
    if (c->head_nc) {
        head.Cout = 128;  // partial products written with a 128-float pixel stride (7*nc used)
        // the column-patch kernel runs one workgroup per 16x16-pixel tile: below ~half a chip of tiles (4 frames at
        // 64x64) the split-K im2col kernel is faster (measured: 1 frame 0.122 -> 0.073 ms, 4 frames 0.122 -> 0.094 ms)
        const int head_tiles = n * ((h + 15) / 16) * ((w + 15) / 16);
        if (c->head_w_swz && head_tiles >= c->head_col7_min_tiles)
            HIP_TRY(c, conv_col7s_launch(io.in0, head.C0, io.in1, head.C1, n, h, w, c->head_w_swz, 3, v.logits, 128, s));
        else
            HIP_TRY(c, conv_launch(head, io, s));
        HIP_TRY(c, motion_head_rowsplit_launch(v.logits, 128, c->head_nc, c->head_bias, v.kp_rec, n, K, h, w, occ, v.deformation,
                                               v.occlusion, v.out.mask, v.out.occlusion_map, s));
    } else {
        head.Cout = 32;  // logits are written with a 32-float pixel stride; channels >= K+2 have zero weights
        HIP_TRY(c, conv_launch(head, io, s));
        HIP_TRY(c, motion_head_launch(v.logits, v.kp_rec, n, K, h, w, occ, v.deformation, v.occlusion, v.out.mask,
                                      v.out.occlusion_map, s));
    }
    if (v.out.deformation)
        HIP_TRY(c, hipMemcpyAsync(v.out.deformation, v.deformation, (size_t)n * h * w * 2 * sizeof(float), hipMemcpyDeviceToDevice, s));
    return EAMM_OK;
}

// feature warp x occlusion (generator.py:79-84) and 'deformed' (generator.py:86).  pre_act: also write r0's pre-activation
// relu(norm1(.)) for the direct-form bottleneck (the Winograd forms apply it in their input transform; training runs norm1
// as a BatchNorm site of its own)
int stage_warp(eamm_ctx* c, const FrameView& v, hipStream_t s, bool pre_act) {
    const bool occ = c->cfg.estimate_occlusion_map != 0;
    HIP_TRY(c, warp_features_launch(v.feat, v.deformation, occ ? v.occlusion : nullptr, v.n, v.ns, c->hf, c->wf, c->Cb, c->h, c->w,
                                    v.xa, pre_act ? v.act : nullptr, c->pre_s[0], c->pre_t[0], s));
    if (v.out.deformed)
        HIP_TRY(c, warp_image_launch(v.src_full, v.deformation, v.n, v.ns, c->H, c->W, c->h, c->w, v.out.deformed, s, c->Cpl,
                                     c->Cimg > 3 ? c->Cimg : 3));
    return EAMM_OK;
}

// ---- bottleneck (generator.py:89): three forms, one function each; the blocks ping-pong between xa and xb (stage_up).
// `timed`: record the profile's per-launch sub-events -- before each of the four launches of a block on s, once after the last.

// F(4x4,3x3), as `chains` groups of frames on as many streams (bottleneck_chains; a view of a whole-pass chain, `chained`, shares
// the chip already and runs as one).  conv1(relu(norm1(x))): the pre-activation rides on the input transform; norm2 + relu in
// the GEMM's epilogue; conv2's epilogue adds x.
// (round 5: splitting a whole-pass chain's bottleneck once more -- 2 x 2 sub-chains of 4 frames -- was built and measured
//  neutral, 3917 vs 3958 frames/s: the input transform is latency-bound and does not shrink with the frames per launch;
//  profiles/r05_experiments.txt section 2, git 9500c6c)
static int bottleneck_wino4(eamm_ctx* c, const FrameView& v, hipStream_t s, bool chained, bool timed) {
    const int n = v.n, hf = c->hf, wf = c->wf, nr = c->cfg.num_bottleneck_blocks;
    const int chains = chained ? 1 : bottleneck_chains(c, n);
    // one chain may split the point rows over workgroups, through Z (never a chained view; several chains only where the split is 1)
    const int groups = chained ? 1 : wino4_groups(c, n);
    // EAMM_WINO4_EPI_V (timing experiment, wrong results, experiments build): only the stage's FIRST transform runs (every GEMM
    // then reads that V: realistic operand values), and the GEMMs' epilogues write V-sized extra output instead (variant 50)
    const bool epi = c->epi_v && c->epi_scratch && chains == 1 && groups == 1;
    float* zbuf = epi ? c->epi_scratch + (size_t)3 * (v.xa - c->xa) : chains > 1 ? nullptr : v.wino_z;
    const int var = epi ? 50 : wino4_variant_for(c, chained ? c->cur_call_frames : n);
    const size_t per_frame = (size_t)hf * wf * c->Cb;
    const int nbase = n / chains, nrem = n % chains;   // the first nrem chains take one more frame
    float *x = v.xa, *xn = v.xb;
    if (chains > 1) {
        HIP_TRY(c, hipEventRecord(c->ev_fork, s));
        for (int k = 1; k < chains; ++k) HIP_TRY(c, hipStreamWaitEvent(c->side_streams[k - 1], c->ev_fork, 0));
    }
    for (int i = 0; i < nr; ++i) {
        for (int k = 0; k < chains; ++k) {
            hipStream_t sk = k ? c->side_streams[k - 1] : s;
            const int nk = nbase + (k < nrem ? 1 : 0);
            const size_t f0 = (size_t)k * nbase + std::min(k, nrem);
            float* xk = x + f0 * per_frame;
            float* xnk = xn + f0 * per_frame;
            float* tk = v.tmp + f0 * per_frame;
            float* vk = v.wino_v + 4 * f0 * per_frame;   // 2.25 nk frames used of the 4 nk reserved for this chain
            // events around the main stream's (chain 0's) kernels only: they time those launches while the other
            // chains' run beside them
            const bool ev = timed && k == 0;
            if (ev) HIP_TRY(c, c->prof.sub(s));
            if (!epi || i == 0) HIP_TRY(c, wino4_transform_launch(xk, c->pre_s[i], c->pre_t[i], nk, hf, wf, c->Cb, vk, sk));
            if (ev) HIP_TRY(c, c->prof.sub(s));
            HIP_TRY(c, wino4_gemm_launch(c->w4res1[i], vk, nk, hf, wf, ACT_RELU, nullptr, tk, sk, var, groups, zbuf));
            if (ev) HIP_TRY(c, c->prof.sub(s));
            if (!epi) HIP_TRY(c, wino4_transform_launch(tk, nullptr, nullptr, nk, hf, wf, c->Cb, vk, sk));
            if (ev) HIP_TRY(c, c->prof.sub(s));
            HIP_TRY(c, wino4_gemm_launch(c->w4res2[i], vk, nk, hf, wf, ACT_NONE, xk, xnk, sk, var, groups, zbuf));   // out += x
        }
        std::swap(x, xn);
    }
    if (timed) HIP_TRY(c, c->prof.sub(s));
    for (int k = 1; k < chains; ++k) {
        HIP_TRY(c, hipEventRecord(c->ev_join[k - 1], c->side_streams[k - 1]));
        HIP_TRY(c, hipStreamWaitEvent(s, c->ev_join[k - 1], 0));
    }
    return EAMM_OK;
}

// F(2x2,3x3): the same four launches per block, with the F(2x2) kernels
static int bottleneck_wino2(eamm_ctx* c, const FrameView& v, hipStream_t s, bool timed) {
    const int n = v.n, hf = c->hf, wf = c->wf, nr = c->cfg.num_bottleneck_blocks;
    float *x = v.xa, *xn = v.xb;
    for (int i = 0; i < nr; ++i) {
        if (timed) HIP_TRY(c, c->prof.sub(s));
        HIP_TRY(c, wino_transform_launch(x, c->pre_s[i], c->pre_t[i], n, hf, wf, c->Cb, v.wino_v, s));
        if (timed) HIP_TRY(c, c->prof.sub(s));
        HIP_TRY(c, wino_gemm_launch(c->wres1[i], v.wino_v, n, hf, wf, ACT_RELU, nullptr, v.tmp, s));
        if (timed) HIP_TRY(c, c->prof.sub(s));
        HIP_TRY(c, wino_transform_launch(v.tmp, nullptr, nullptr, n, hf, wf, c->Cb, v.wino_v, s));
        if (timed) HIP_TRY(c, c->prof.sub(s));
        HIP_TRY(c, wino_gemm_launch(c->wres2[i], v.wino_v, n, hf, wf, ACT_NONE, x, xn, s));   // out += x
        std::swap(x, xn);
    }
    if (timed) HIP_TRY(c, c->prof.sub(s));
    return EAMM_OK;
}

// direct form: the block's input arrives pre-activated in v.act (the warp's, then conv2's, second output)
static int bottleneck_direct(eamm_ctx* c, const FrameView& v, hipStream_t s) {
    const int n = v.n, hf = c->hf, wf = c->wf, nr = c->cfg.num_bottleneck_blocks;
    float *x = v.xa, *xn = v.xb;
    for (int i = 0; i < nr; ++i) {
        const ConvIO a = conv_for(v, v.act, hf, wf, ACT_RELU, v.tmp);  // conv1 -> norm2 (folded) -> relu
        HIP_TRY(c, conv_launch(pick(c, c->res1[i], (size_t)n * hf * wf), a, s));
        ConvIO b = conv_for(v, v.tmp, hf, wf, ACT_NONE, xn);
        b.resid = x;       // out += x
        if (i + 1 < nr) {  // next block's relu(norm1(.))
            b.out2 = v.act;
            b.s2 = c->pre_s[i + 1];
            b.t2 = c->pre_t[i + 1];
        }
        HIP_TRY(c, conv_launch(pick(c, c->res2[i], (size_t)n * hf * wf), b, s));
        std::swap(x, xn);
    }
    return EAMM_OK;
}

// chain: index of this launch sequence among the call's whole-pass chains (0: the caller's stream, whose launches are timed)
static int stage_bottleneck(eamm_ctx* c, const FrameView& v, hipStream_t s, int chain, bool chained) {
    const bool timed = chain == 0 && 4 * c->cfg.num_bottleneck_blocks + 1 <= PassProfile::NSUB;
    switch (bottleneck_form(c, v.n)) {
        case 4: return bottleneck_wino4(c, v, s, chained, timed);
        case 2: return bottleneck_wino2(c, v, s, timed);
        default: return bottleneck_direct(c, v, s);
    }
}

static int stage_up(eamm_ctx* c, const FrameView& v, hipStream_t s) {   // generator.py:90-91
    const float* x = (c->cfg.num_bottleneck_blocks & 1) ? v.xb : v.xa;   // the bottleneck's blocks ping-pong between the two
    for (int i = 0; i < c->nd; ++i) {
        if (int rc = launch_up(c, c->up[i], conv_for(v, x, c->hf << i, c->wf << i, ACT_RELU, v.up_buf[i]), s)) return rc;
        x = v.up_buf[i];
    }
    return EAMM_OK;
}

// final 7x7 + sigmoid on the last up block's output, written NCHW straight into the caller's buffer      generator.py:92-93
int stage_final(eamm_ctx* c, const FrameView& v, hipStream_t s) {
    const float* in = v.up_buf[c->nd - 1];
    ConvIO io = conv_for(v, in, c->H, c->W, ACT_NONE, v.final_part);
    if (c->Cimg > 3) {   // plain 7x7 kernel, sigmoid + NCHW store in the epilogue, straight into the caller's [n,C,H,W]
        io.act = ACT_SIGMOID;
        io.nchw = 1;
        io.out = v.out.prediction;
        HIP_TRY(c, conv_launch(c->final_conv, io, s));
        return EAMM_OK;
    }
    ConvLayer fl = c->final_conv;
    fl.Cout = 32;  // 32-float pixel stride; channels >= 21 have zero weights
    if (final_is_fused(c, v.n)) {
        HIP_TRY(c, conv_col7_fused_launch(in, fl.C0, v.n, c->H, c->W, c->final_w_swz, c->final_bias, v.out.prediction, s, c->final_w3));
    } else {
        if (c->final_w_swz && fl.BN == 32)
            HIP_TRY(c, conv_col7_launch(in, fl.C0, v.n, c->H, c->W, c->final_w_swz, v.final_part, s));
        else
            HIP_TRY(c, conv_launch(fl, io, s));
        HIP_TRY(c, final_shift_sum_launch(v.final_part, c->final_bias, v.n, c->H, c->W, v.out.prediction, s));
    }
    if (v.out.frames_u8) HIP_TRY(c, to_u8_launch(v.out.prediction, v.n, c->H, c->W, v.out.frames_u8, s));
    return EAMM_OK;
}

// One launch sequence over the frames of `v` on stream s.  chain: its index among the call's whole-pass chains; `chained`: other
// sequences run beside it.  (The caller records the last stage mark, after joining the chains.)
static int forward_view(eamm_ctx* c, const FrameView& v, hipStream_t s, int chain, bool chained) {
    PassProfile& p = c->prof;
    const bool direct = bottleneck_form(c, v.n) == 0;
    int rc;
    for (int i = 0; i <= (c->nb ? 0 : 4); ++i) HIP_TRY(c, p.mark(i, s, chain));
    if (c->nb == 0) {   // no motion network (generator.py:64 is false): the encoder features enter the bottleneck as they are
        HIP_TRY(c, broadcast_features_launch(v.feat, v.n, v.ns, c->hf, c->wf, c->Cb, v.xa, direct ? v.act : nullptr, c->pre_s[0],
                                             c->pre_t[0], s));
    } else {
        if ((rc = stage_motion_front(c, v, s))) return rc;
        HIP_TRY(c, p.mark(1, s, chain));
        if ((rc = stage_hg_encoder(c, v, s))) return rc;
        HIP_TRY(c, p.mark(2, s, chain));
        if ((rc = stage_hg_decoder(c, v, s))) return rc;
        HIP_TRY(c, p.mark(3, s, chain));
        if ((rc = stage_flow_head(c, v, s))) return rc;
        HIP_TRY(c, p.mark(4, s, chain));
        if ((rc = stage_warp(c, v, s, direct))) return rc;
    }
    HIP_TRY(c, p.mark(5, s, chain));
    HIP_TRY(c, p.window(chain, 0, s));
    if ((rc = stage_bottleneck(c, v, s, chain, chained))) return rc;
    HIP_TRY(c, p.mark(6, s, chain));
    HIP_TRY(c, p.window(chain, 1, s));
    if ((rc = stage_up(c, v, s))) return rc;
    HIP_TRY(c, p.mark(7, s, chain));
    if ((rc = stage_final(c, v, s))) return rc;
    p.account(7);
    return EAMM_OK;
}

// ---- PassProfile (eamm_ctx.h) -------------------------------------------------------------------------------------------
void PassProfile::begin_call(int n, int chains) {
    (void)take_mfma_flops();
    cur = Call{};
    cur.n = n;
    cur.nchain = std::min(chains, (int)MAXCHAIN);
    const bool rec = on && used < PROF_CALLS;
    ev = rec ? events.data() + (size_t)used * (NMARK + 1 + NSUB) : nullptr;
    cev = rec ? chain_ev.data() + (size_t)used * MAXCHAIN * 2 : nullptr;
    if (rec) calls[used++] = Call{};   // (incomplete until end_call)
}
void PassProfile::account(int interval) {
    const double f = take_mfma_flops();
    cur.flops += f;
    cur.stage_flops[interval] += f;
    if (interval == 5) cur.flops_bneck += f;
}
hipError_t PassProfile::end_call(hipStream_t s) {
    if (!ev) return hipSuccess;
    const hipError_t e = hipEventRecord(ev[NMARK], s);
    cur.complete = e == hipSuccess;
    calls[used - 1] = cur;
    ev = cev = nullptr;
    return e;
}

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
    const int chains = pass_chains(c, n);
    c->cur_call_frames = n;
    c->prof.begin_call(n, chains);
    if (chains == 1) {
        if (int rc = forward_view(c, make_view(c, 0, n, ns, 0, kd_val, kd_jac, ks_val, ks_jac, o), s, 0, false)) return rc;
    } else {
        const int nbase = n / chains, nrem = n % chains;   // the first nrem chains take one more frame
        HIP_TRY(c, hipEventRecord(c->ev_fork, s));
        for (int k = 1; k < chains; ++k) HIP_TRY(c, hipStreamWaitEvent(c->side_streams[k - 1], c->ev_fork, 0));
        for (int k = 0; k < chains; ++k) {
            const int nk = nbase + (k < nrem ? 1 : 0), f0 = k * nbase + std::min(k, nrem);
            const FrameView v = make_view(c, f0, nk, ns, k, kd_val, kd_jac, ks_val, ks_jac, o);
            if (int rc = forward_view(c, v, k ? c->side_streams[k - 1] : s, k, true)) return rc;
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
    HIP_TRY(c, c->prof.end_call(s));
    return EAMM_OK;
}

int eamm_profile_enable(eamm_ctx* c, int on) {
    if (!c) return EAMM_ERR_ARG;
    DeviceGuard guard(c->device);
    if (guard.status != hipSuccess) return fail(c, EAMM_ERR_HIP, "hipSetDevice(%d) failed", c->device);
    PassProfile& p = c->prof;
    if (on && p.events.empty()) {
        p.events.resize((size_t)PassProfile::PROF_CALLS * (PassProfile::NMARK + 1 + PassProfile::NSUB));
        for (auto& e : p.events) HIP_TRY(c, hipEventCreate(&e));
        p.chain_ev.resize((size_t)PassProfile::PROF_CALLS * PassProfile::MAXCHAIN * 2);
        for (auto& e : p.chain_ev) HIP_TRY(c, hipEventCreate(&e));
        p.calls.resize(PassProfile::PROF_CALLS);
    }
    p.on = on != 0;
    return EAMM_OK;
}

int eamm_profile_read(eamm_ctx* c, double* stage_ms, int nstage, int64_t* calls, int64_t* frames, int reset) {
    constexpr int NSTAGE = PassProfile::NSTAGE, NMARK = PassProfile::NMARK, NSUB = PassProfile::NSUB, MAXCHAIN = PassProfile::MAXCHAIN;
    if (!c || !stage_ms || nstage != NSTAGE) return fail(c, EAMM_ERR_ARG, "nstage must be %d", NSTAGE);
    DeviceGuard guard(c->device);
    if (guard.status != hipSuccess) return fail(c, EAMM_ERR_HIP, "hipSetDevice(%d) failed", c->device);
    PassProfile& p = c->prof;
    // stage index of each of the NMARK recorded intervals; the bottleneck interval (5) is split below
    static const int stage_of[NMARK] = {0, 1, 2, 3, 4, 6, 7, 8};
    for (int k = 0; k < p.used; ++k) {  // fold finished event sets into the totals
        const PassProfile::Call& call = p.calls[k];
        hipEvent_t* ev = p.events.data() + (size_t)k * (NMARK + 1 + NSUB);
        // a call that failed midway leaves a partly recorded set: skip it (its events are re-recorded by a later call)
        bool ok = call.complete && hipEventSynchronize(ev[NMARK]) == hipSuccess;
        double ms_set[NSTAGE] = {0};
        auto span = [&](hipEvent_t a, hipEvent_t b) {   // milliseconds from a to b; clears ok on failure
            float ms = 0.f;
            ok = ok && hipEventElapsedTime(&ms, a, b) == hipSuccess;
            return (double)ms;
        };
        for (int i = 0; ok && i < NMARK; ++i) ms_set[stage_of[i]] += span(ev[i], ev[i + 1]);
        if (const int nsub = call.sub; ok && nsub > 1) {  // Winograd form: even intervals are input transforms, odd ones the GEMM kernels
            hipEvent_t* sub = ev + NMARK + 1;
            double tr = 0;
            for (int i = 0; ok && i + 1 < nsub; i += 2) tr += span(sub[i], sub[i + 1]);
            ms_set[5] += tr;
            ms_set[6] -= tr;
            for (int i = 1; ok && i + 1 < nsub; i += 2) ms_set[9] += span(sub[i], sub[i + 1]);   // the GEMM kernels' own durations on the main stream
        }
        if (ok) {   // bottleneck windows of the whole-pass chains, on the clock of this call's first event
            hipEvent_t* cv = p.chain_ev.data() + (size_t)k * MAXCHAIN * 2;
            const int nc = call.nchain;
            double t0[MAXCHAIN], t1[MAXCHAIN];
            for (int j = 0; ok && j < nc; ++j) {
                ok = hipEventSynchronize(cv[2 * j + 1]) == hipSuccess;
                t0[j] = span(ev[0], cv[2 * j]), t1[j] = span(ev[0], cv[2 * j + 1]);
            }
            if (ok) {
                int order[MAXCHAIN];
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
                ms_set[12] = call.flops * 1e-9;
                ms_set[13] = call.flops_bneck * 1e-9;
                for (int i = 0; i < NMARK; ++i) ms_set[14 + i] = call.stage_flops[i] * 1e-9;
            }
        }
        if (!ok) {
            (void)hipGetLastError();
            continue;
        }
        for (int i = 0; i < NSTAGE; ++i) p.ms[i] += ms_set[i];
        p.ncalls += 1;
        p.nframes += call.n;
    }
    p.used = 0;
    for (int i = 0; i < nstage; ++i) stage_ms[i] = p.ms[i];
    if (calls) *calls = p.ncalls;
    if (frames) *frames = p.nframes;
    if (reset) {
        for (double& v : p.ms) v = 0;
        p.ncalls = p.nframes = 0;
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
                             "\"wino4_groups\": %d, \"wino4_variant\": %d, \"hg_encoder\": %s, \"final\": \"%s\", "
                             "\"final_products\": \"%s\", \"side_streams\": %d, \"experiments_build\": %d}",
                             n, pc, nk, form, bc, (form == 4 && pc == 1 && bc == 1) ? wino4_groups(c, n) : 1, wino4_variant_for(c, n), enc.c_str(),
                             final_is_fused(c, nk) ? "col7q fused" : "col7 + shift-sum",
                             final_is_fused(c, nk) && c->final_w3 ? "split-bf16" : "fp32", (int)c->pool_streams.size(),
                             eamm_build_experiments());
    if (buf && cap > 0) {
        const int m = std::min(len, cap - 1);
        std::memcpy(buf, tmp, (size_t)m);
        buf[m] = 0;
    }
    return len;
}

}  // extern "C"
