// The operator entries of the C ABI (eamm_op_*, include/eamm_hip.h): each runs ONE kernel family of the path -- or one
// operator of the differentiable training graph -- on caller-provided device buffers, without a handle.
#include "eamm_ctx.h"
#include <algorithm>
#include <mutex>

namespace {

// `iters` back-to-back run()s between two HIP events on `s`; *avg_ms gets their mean only when every step succeeded
template <typename Run>
hipError_t time_launches(hipStream_t s, int iters, float* avg_ms, Run run) {
    if (iters <= 0 || !avg_ms) return hipSuccess;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    if (e == hipSuccess) e = hipEventRecord(e0, s);
    for (int i = 0; i < iters && e == hipSuccess; ++i) e = run();
    if (e == hipSuccess) e = hipEventRecord(e1, s);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    if (e == hipSuccess) *avg_ms = ms / iters;
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return e;
}

// An operator call's temporary device buffers (dev_alloc / upload): freed on every path, once the caller's stream is done
// with them.  Errors land in `err`; the entry hands them on to eamm_last_error(NULL).
struct OpBuffers : CtxBase {
    hipStream_t s;
    OpBuffers(int dev, hipStream_t st) : s(st) { device = dev; }
    ~OpBuffers() {
        if (owned.empty()) return;
        (void)hipStreamSynchronize(s);
        for (void* p : owned) (void)hipFree(p);
    }
};

struct ConvOp {   // eamm_op_conv's arguments
    const float *in0, *in1;
    int C0, C1, B, Hin, Win, up;
    const float *w, *b;
    int Cout, kh, kw, act, pool;
    const float* resid;
    int splitk, tile_n;
    float* out;
    int iters;
    float* avg_ms;
    hipStream_t s;
};

// the caller's OIHW filter [Cout][Cin][kh][kw] (BatchNorm folded) and, with_bias, its bias [Cout]
HostConv op_weights(const ConvOp& a, int Cin, bool with_bias = true) {
    HostConv f;
    f.Cout = a.Cout;
    f.Cin = Cin;
    f.kh = a.kh;
    f.kw = a.kw;
    f.w.assign(a.w, a.w + (size_t)a.Cout * Cin * a.kh * a.kw);
    if (with_bias) f.b.assign(a.b, a.b + a.Cout);
    return f;
}

// 4002: the final layer whole (7x7, 3 output channels, bias, sigmoid -> NCHW) on the fused column-patch kernel, with the
// row-split weights of the engine's final_w_swz
int op_conv_final(OpBuffers* t, const ConvOp& a) {
    if (a.kh != 7 || a.kw != 7 || a.Cout != 3 || a.act != 2 || a.up || a.pool || a.resid || a.C1 || a.C0 % 32 || a.C0 > 64 || a.C0 < 32)
        return fail(t, EAMM_ERR_ARG, "eamm_op_conv: unsupported fused final-layer configuration");
    HostConv f = op_weights(a, a.C0);
    const std::vector<float> bias = to_rowsplit(&f);
    float *w = nullptr, *b = nullptr;
    int rc = upload_conv_image(t, &w, f, nullptr, a.C0, conv_tile_n(f.Cout), MODE_PLAIN, true);
    if (rc || (rc = upload(t, &b, bias))) return rc;
    auto fused_final = [&]() { return conv_col7_fused_launch(a.in0, a.C0, a.B, a.Hin, a.Win, w, b, a.out, a.s); };
    HIP_TRY(t, fused_final());
    HIP_TRY(t, time_launches(a.s, a.iters, a.avg_ms, fused_final));
    return EAMM_OK;
}

// column-patch kernels of the 7x1 convolutions: 4000 final layer (Cout = the 32-float pixel stride, weights resident), 4001
// flow head (two inputs, Cout = 96, streamed weights); the weights come row-split, no bias (the gather kernels add it)
int op_conv_col7(OpBuffers* t, const ConvOp& a) {
    const bool streamed = a.tile_n == 4001;
    const int bn = streamed ? 96 : 32;
    if (a.kh != 7 || a.kw != 1 || a.up || a.pool || a.resid || a.splitk > 1 || a.Cout != bn || a.act != 0 || a.C0 % 32 || a.C1 % 32 ||
        (!streamed && (a.C1 || a.C0 > 64)))
        return fail(t, EAMM_ERR_ARG, "eamm_op_conv: unsupported column-patch configuration");
    float* w = nullptr;
    if (int rc = upload_conv_image(t, &w, op_weights(a, a.C0 + a.C1, false), nullptr, a.C0 + a.C1, bn, MODE_PLAIN, true)) return rc;
    auto col7 = [&]() {
        return streamed ? conv_col7s_launch(a.in0, a.C0, a.in1, a.C1, a.B, a.Hin, a.Win, w, 3, a.out, 96, a.s)
                        : conv_col7_launch(a.in0, a.C0, a.B, a.Hin, a.Win, w, a.out, a.s);
    };
    HIP_TRY(t, col7());
    HIP_TRY(t, time_launches(a.s, a.iters, a.avg_ms, col7));
    return EAMM_OK;
}

// spatial-patch kernels of the up-convolution: 3000 collapsed-phase form, 3003 polyphase minimal-filtering form (splitk > 1:
// its channel reduction over that many workgroups)
int op_conv_patch(OpBuffers* t, const ConvOp& a) {
    const bool pp = a.tile_n == 3003;
    const int psplit = a.splitk > 1 ? a.splitk : 1;
    if (a.kh != 3 || a.kw != 3 || !a.up || a.pool || a.resid || (a.Cout & 3) || (psplit > 1 && (!pp || ((a.C0 + a.C1) / 32) % psplit)))
        return fail(t, EAMM_ERR_ARG, "eamm_op_conv: unsupported patch-kernel configuration");
    PatchLayer P;
    float* ppart = nullptr;
    const size_t ppart_elems = psplit > 1 ? (size_t)psplit * a.B * 4 * a.Hin * a.Win * a.Cout : 0;
    int rc = pack_patch(t, op_weights(a, a.C0 + a.C1), nullptr, a.C0, a.C1, pp, &P);
    if (rc || (psplit > 1 && (rc = dev_alloc(t, &ppart, ppart_elems)))) return rc;
    auto patch = [&]() {
        return pp ? patch_poly_launch(P, a.in0, a.in1, a.B, a.Hin, a.Win, a.act, a.out, a.s, psplit, ppart, ppart_elems)
                  : patch_phase_launch(P, a.in0, a.in1, a.B, a.Hin, a.Win, a.act, a.out, a.s);
    };
    HIP_TRY(t, patch());
    HIP_TRY(t, time_launches(a.s, a.iters, a.avg_ms, patch));
    return EAMM_OK;
}

// Winograd: input transform + GEMM; 2000 F(2x2,3x3), 2100 + pipeline variant (0, 3, 6) F(4x4,3x3), 2150 + groups (2, 3, 6):
// F(4x4,3x3) with the transform-point rows split over workgroups + output-transform kernel
int op_conv_wino(OpBuffers* t, const ConvOp& a) {
    const bool w4 = a.tile_n >= 2100;
    const int w4_groups = a.tile_n >= 2150 ? a.tile_n - 2150 : 1;
    const int w4_variant = w4_groups > 1 ? 0 : a.tile_n - 2100;   // (an unknown variant or split is wino4_gemm_launch's to refuse)
    if ((!w4 && a.tile_n != 2000) || a.kh != 3 || a.kw != 3 || a.up || (a.pool && (w4_groups == 1 || a.resid)) || a.C1 || a.splitk > 1 || a.C0 % 64 ||
        (a.Cout & 3) || (w4 && ((a.Hin & 3) || (a.Win & 3))))
        return fail(t, EAMM_ERR_ARG, "eamm_op_conv: unsupported Winograd configuration");
    WinoLayer W;
    float *V = nullptr, *Zb = nullptr;
    int rc = pack_wino(t, op_weights(a, a.C0), w4 ? 4 : 2, &W);
    if (rc || (rc = dev_alloc(t, &V, (size_t)16 * a.B * (a.Hin / 2) * (a.Win / 2) * a.C0))) return rc;
    // (+ 4: 16 bytes of slack)
    if ((rc = dev_alloc(t, &Zb, (size_t)24 * a.B * ((a.Hin + 3) / 4) * ((a.Win + 3) / 4) * a.Cout + 4))) return rc;
    // timing-mode knob: EAMM_OP_WINO_PART = 1 times the input transform alone, 2 the GEMM alone
    const int part = env_int("EAMM_OP_WINO_PART", 0);
    bool timing = false;
    auto winograd = [&]() {
        const bool tr = !timing || part != 2, gm = !timing || part != 1;
        hipError_t e = hipSuccess;
        if (w4) {
            if (tr) e = wino4_transform_launch(a.in0, nullptr, nullptr, a.B, a.Hin, a.Win, a.C0, V, a.s);
            if (e != hipSuccess || !gm) return e;
            return wino4_gemm_launch(W, V, a.B, a.Hin, a.Win, a.act, a.resid, a.out, a.s, w4_variant, w4_groups, Zb, a.pool);
        }
        if (tr) e = wino_transform_launch(a.in0, nullptr, nullptr, a.B, a.Hin, a.Win, a.C0, V, a.s);
        if (e != hipSuccess || !gm) return e;
        return wino_gemm_launch(W, V, a.B, a.Hin, a.Win, a.act, a.resid, a.out, a.s);
    };
    HIP_TRY(t, winograd());
    timing = true;
    HIP_TRY(t, time_launches(a.s, a.iters, a.avg_ms, winograd));
    return EAMM_OK;
}

// the implicit GEMM: tile_n 0 automatic, 32 / 64 / 128 the register-staged 128 x tile_n kernel, 1000 + id an LDS-DMA tile
int op_conv_gemm(OpBuffers* t, const ConvOp& a) {
    const int dma_cfg = a.tile_n > 1000 ? a.tile_n - 1000 : 0;
    int BM = 0, BN = a.tile_n > 0 ? a.tile_n : conv_tile_n(a.Cout);
    if (dma_cfg) {
        if (!conv_dma_tile(dma_cfg, &BM, &BN) || a.kw == 1 || a.kh == 7) return fail(t, EAMM_ERR_ARG, "unknown / unsupported dma tile");
    } else if (BN != 32 && BN != 64 && BN != 128) {
        return fail(t, EAMM_ERR_ARG, "tile_n must be 32/64/128 or 1000+dma id");
    }
    ConvLayer L;
    int rc = pack_conv(t, op_weights(a, a.C0 + a.C1), nullptr, a.C0, a.C1, a.up ? MODE_PHASE : MODE_PLAIN, dma_cfg, &L, dma_cfg ? 0 : BN);
    if (rc) return rc;
    ConvIO io = conv_io(a.in0, a.B, a.Hin, a.Win, a.act, a.out, nullptr, conv_plan(L, a.B * a.Hin * a.Win, a.splitk).partial_elems);
    io.in1 = a.C1 ? a.in1 : nullptr;
    io.pool = a.pool;
    io.resid = a.resid;
    if (io.partial_cap && (rc = dev_alloc(t, &io.partial, io.partial_cap))) return rc;
    auto gemm = [&]() { return conv_launch(L, io, a.s, a.splitk); };
    HIP_TRY(t, gemm());
    HIP_TRY(t, time_launches(a.s, a.iters, a.avg_ms, gemm));
    return EAMM_OK;
}

// eamm_op_conv: the family of tile_n (include/eamm_hip.h), then the caller's stream drained
int op_conv_run(OpBuffers* t, const ConvOp& a) {
    int rc;
    if (a.tile_n == 4002) rc = op_conv_final(t, a);
    else if (a.tile_n == 4000 || a.tile_n == 4001) rc = op_conv_col7(t, a);
    else if (a.tile_n == 3000 || a.tile_n == 3003) rc = op_conv_patch(t, a);
    else if (a.tile_n >= 2000 && a.tile_n < 2200) rc = op_conv_wino(t, a);
    else rc = op_conv_gemm(t, a);
    if (rc) return rc;
    HIP_TRY(t, hipStreamSynchronize(a.s));
    return EAMM_OK;
}

// The preamble and return of an eamm_op_* entry: argument check, the device made current for the call, the caller's stream
#define OP_ENTRY(cond, msg)                                                                      \
    if (cond) return fail(nullptr, EAMM_ERR_ARG, msg);                                           \
    DeviceGuard guard(device);                                                                   \
    if (guard.status != hipSuccess) return fail(nullptr, EAMM_ERR_HIP, "hipSetDevice failed");   \
    hipStream_t s = reinterpret_cast<hipStream_t>(stream_)
#define OP_DONE(e, name) \
    return (e) == hipSuccess ? EAMM_OK : fail(nullptr, EAMM_ERR_HIP, name " failed: %s", hipGetErrorString(e))

}  // namespace

// -------------------------------------------------------------------------------------------------
extern "C" {

int eamm_op_conv(int device, const float* in0, int C0, const float* in1, int C1, int B, int Hin, int Win, int up,
                 const float* w_host, const float* b_host, int Cout, int kh, int kw, int act, int pool,
                 const float* resid, int splitk, int tile_n, float* out, int iters, float* avg_ms, void* stream_) {
    const bool shape_ok = (kh == 3 && kw == 3) || (kh == 7 && kw == 7) || (kh == 7 && kw == 1);
    OP_ENTRY(!in0 || !w_host || !b_host || !out || !shape_ok || C0 % CONV_BK || C1 % CONV_BK || (up && (kh != 3 || kw != 3)),
             "eamm_op_conv: bad argument");
    const ConvOp a{in0, in1, C0, C1, B, Hin, Win, up, w_host, b_host, Cout, kh, kw, act, pool, resid, splitk, tile_n, out, iters, avg_ms, s};
    OpBuffers t(device, s);
    if (int rc = op_conv_run(&t, a)) return fail(nullptr, rc, "%s", t.err.c_str());
    return EAMM_OK;
}

int eamm_op_one_euro(int device, const float* x, int T, int E, float mincutoff, float beta, float dcutoff, float freq, float scale,
                     float* out, float* state, int resume, void* stream_) {
    OP_ENTRY(!x || !out || T < 0 || E < 1 || (resume && !state), "eamm_op_one_euro: bad argument");
    const hipError_t e = one_euro_launch(x, T, E, mincutoff, beta, dcutoff, freq, scale, out, s, state, resume);
    return e == hipSuccess ? EAMM_OK : fail(nullptr, EAMM_ERR_HIP, "one_euro_kernel: %s", hipGetErrorString(e));
}

int64_t eamm_op_mfcc_frames(int64_t n_samples, int pad) { return mfcc_frames(n_samples, pad); }

int eamm_op_mfcc(int device, const float* pcm, int64_t n_samples, int n_clips, int64_t clip_stride, int pad, float* out, void* stream_) {
    OP_ENTRY(!pcm || !out || n_samples < 1 || n_clips < 1 || n_clips > 65535 || pad < 0 || (n_clips > 1 && clip_stride < n_samples),
             "eamm_op_mfcc: bad argument (n_samples >= 1, 1 <= n_clips <= 65535, pad >= 0, clip_stride >= n_samples)");
    const hipError_t e = mfcc_launch(pcm, n_samples, n_clips, clip_stride, pad, out, s);
    return e == hipSuccess ? EAMM_OK : fail(nullptr, EAMM_ERR_HIP, "mfcc_kernel: %s", hipGetErrorString(e));
}

int eamm_op_resize_aa(int device, const uint8_t* in, int n, int H, int W, int C, const double* taps_y, int ry, const double* taps_x,
                      int rx, uint8_t* out, void* stream_) {
    OP_ENTRY(!in || !out || !taps_y || !taps_x || n < 1 || n > 65535 || H < 1 || W < 1 || H > 8192 || W > 8192 || (C != 3 && C != 4) ||
                 ry < 0 || rx < 0 || ry >= VIDEO_MAX_RADIUS || rx >= VIDEO_MAX_RADIUS,
             "eamm_op_resize_aa: bad argument (1 <= n <= 65535, sides 1..8192, C = 3 | 4, tap radii 0..31)");
    VideoResizeTaps t{};
    std::memcpy(t.wy, taps_y, sizeof(double) * (2 * ry + 1));
    std::memcpy(t.wx, taps_x, sizeof(double) * (2 * rx + 1));
    t.ry = ry;
    t.rx = rx;
    const hipError_t e = resize_aa_launch(in, n, H, W, C, t, out, s);
    OP_DONE(e, "eamm_op_resize_aa");
}

int eamm_op_similarity_warp(int device, const uint8_t* in, int n, int H, int W, int C, const double* maps, int mode, void* out,
                            void* stream_) {
    OP_ENTRY(!in || !out || !maps || n < 1 || n > 65535 || H < 1 || W < 1 || H > 8192 || W > 8192 || (C != 3 && C != 4) ||
                 (mode != 0 && mode != 1),
             "eamm_op_similarity_warp: bad argument (1 <= n <= 65535, sides 1..8192, C = 3 | 4, mode 0 | 1)");
    const hipError_t e = similarity_warp_launch(in, n, H, W, C, maps, mode, out, s);
    OP_DONE(e, "eamm_op_similarity_warp");
}

int eamm_op_emotion_augment(int device, const float* aligned, int64_t n_src, int64_t t0, int count, int flip, const double* rot,
                            const double* hinv, const float* noise, uint64_t noise_seed, int mouth_x, int mouth_y, int mouth_w,
                            int mouth_h, float* out, void* stream_) {
    OP_ENTRY(!aligned || !rot || !hinv || !out || n_src < 1 || t0 < 0 || count < 1 || count > 65535 || mouth_x < 0 || mouth_y < 0 ||
                 mouth_w < 1 || mouth_h < 1 || mouth_x + mouth_w > 256 || mouth_y + mouth_h > 256,
             "eamm_op_emotion_augment: bad argument (n_src >= 1, t0 >= 0, 1 <= count <= 65535, a mouth rectangle inside 256 x 256)");
    VideoAugParams p{};
    std::memcpy(p.rot, rot, sizeof p.rot);
    p.noise_seed = noise_seed;
    p.flip = flip ? 1 : 0;
    p.mouth_x = mouth_x;
    p.mouth_y = mouth_y;
    p.mouth_w = mouth_w;
    p.mouth_h = mouth_h;
    const hipError_t e = emotion_augment_launch(aligned, n_src, t0, count, hinv, noise, p, out, s);
    OP_DONE(e, "eamm_op_emotion_augment");
}

int eamm_op_warp(int device, const float* feat, const float* deformation, const float* occlusion, int n, int ns, int hf,
                 int wf, int C, int h, int w, float* out, int iters, float* avg_ms, void* stream_) {
    OP_ENTRY(!feat || !deformation || !out || n < 1 || (ns != 1 && ns != n) || hf < 1 || wf < 1 || h < 1 || w < 1 || C < 8 || (C & 7),
             "eamm_op_warp: bad argument");
    auto run = [&]() { return warp_features_launch(feat, deformation, occlusion, n, ns, hf, wf, C, h, w, out, nullptr, nullptr, nullptr, s); };
    hipError_t e = run();
    if (e == hipSuccess) e = time_launches(s, iters, avg_ms, run);
    // (no stream synchronisation outside the timing branch: like every other operator entry the work is only ENQUEUED on
    // `stream` -- the differentiable forward calls this three times per pass and must stay capturable)
    if (e == hipSuccess) e = hipGetLastError();
    OP_DONE(e, "eamm_op_warp");
}

int eamm_op_warp_backward(int device, const float* feat, const float* deformation, const float* occlusion, const float* grad_out,
                          int n, int ns, int hf, int wf, int C, float* grad_feat, float* grad_deformation, float* grad_occlusion,
                          void* stream_) {
    OP_ENTRY(!feat || !deformation || !grad_out || n < 1 || (ns != 1 && ns != n) || hf < 1 || wf < 1 || C < 4 || (C & 3) ||
                 (!grad_feat && !grad_deformation && !grad_occlusion) || (grad_occlusion && !occlusion),
             "eamm_op_warp_backward: bad argument");
    // the kernel accumulates: the gradients start from zero here, on the caller's stream
    hipError_t e = hipSuccess;
    if (grad_feat) e = hipMemsetAsync(grad_feat, 0, (size_t)ns * hf * wf * C * sizeof(float), s);
    if (e == hipSuccess && grad_deformation) e = hipMemsetAsync(grad_deformation, 0, (size_t)n * hf * wf * 2 * sizeof(float), s);
    if (e == hipSuccess && grad_occlusion) e = hipMemsetAsync(grad_occlusion, 0, (size_t)n * hf * wf * sizeof(float), s);
    if (e == hipSuccess)
        e = warp_features_backward_launch(feat, deformation, occlusion, grad_out, n, ns, hf, wf, C, grad_feat, grad_deformation,
                                          grad_occlusion, s);
    OP_DONE(e, "eamm_op_warp_backward");
}

// ---- convolution with DEVICE weights (training path): pack on the device into the caller's workspace, then the forward kernels
namespace {
struct ConvDevPlan {
    bool wino4 = false;
    int groups = 1;         // F(4x4): rows of transform points split over this many workgroups per tile (few tiles), as the engine does
    size_t zbuf = 0;        // floats of the split form's x-folded products
    int BN = 0, ntiles = 0;
    size_t packed = 0, bias = 0, aux = 0;   // floats: packed filter, padded bias, Winograd V or split-K partials
    ConvLayer L;
};
bool conv_dev_plan(int B, int H, int W, int Cin, int Cout, int kh, int kw, ConvDevPlan* P) {
    if (B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || Cin % CONV_BK || (Cout & 3)) return false;
    if (!((kh == 3 && kw == 3) || (kh == 7 && kw == 7))) return false;
    const long long Mq = (long long)B * (H / 4) * (W / 4);
    // F(4x4,3x3) where the bottleneck's kernel applies and the tile count fills the chip; else the register-staged implicit GEMM
    static const int wino_off = knob_int("EAMM_CONV_DEV_WINO4", 1) == 0;
    static const long long wino_min_tiles = knob_int("EAMM_CONV_DEV_WINO4_MIN_TILES", 2048);
    P->wino4 = !wino_off && kh == 3 && kw == 3 && Cin % (2 * CONV_BK) == 0 && !(H & 3) && !(W & 3) && Mq >= wino_min_tiles &&
               (unsigned long long)36 * Mq * Cin * sizeof(float) < 0xFFFFF000ull &&
               wino4_packed_elems(Cout, Cin, 64) * sizeof(float) < 0xFFFFF000ull;
    if (P->wino4) {
        P->BN = 64;
        P->ntiles = (Cout + 63) / 64;
        P->packed = wino4_packed_elems(Cout, Cin, 64);
        P->aux = (size_t)36 * Mq * Cin;
        // a single launch of <= 128 64-tile workgroups leaves half the chip idle (the engine runs two chains there): split
        // the transform-point rows over 2 / 3 / 6 workgroups per tile, as the engine's one-chain calls do
        const long long nb = ((Mq + 63) / 64) * P->ntiles;
        for (int gsel : {6, 3, 2})
            if (nb * gsel <= 256) {
                P->groups = gsel;
                break;
            }
        if (P->groups > 1) P->zbuf = (size_t)24 * Mq * Cout;
    } else {
        ConvLayer& L = P->L;
        L.kh = kh;
        L.kw = kw;
        L.C0 = Cin;
        L.Cout = Cout;
        L.BN = conv_tile_n(Cout);
        L.ntiles = (Cout + L.BN - 1) / L.BN;
        L.nchunks = kh * kw * (Cin / CONV_BK);
        P->BN = L.BN;
        P->ntiles = L.ntiles;
        P->packed = conv_packed_elems(kh * kw, Cin, Cout, L.BN, 1);
        P->aux = conv_plan(L, B * H * W, 0).partial_elems;
    }
    P->bias = (size_t)P->ntiles * P->BN;
    auto up = [](size_t n) { return (n + 63) / 64 * 64; };   // 256-byte aligned sections
    P->packed = up(P->packed);
    P->bias = up(P->bias);
    P->aux = up(P->aux);
    P->zbuf = up(P->zbuf);
    return true;
}
}  // namespace

namespace {
// A per-device vector of zeros (never written after its allocation): the bias of the convolutions that have none.
const float* device_zeros(int device, size_t n, hipStream_t stream) {
    constexpr size_t CAP = 16384;
    constexpr int MAXDEV = 64;
    static std::mutex mu;
    static float* zeros[MAXDEV] = {};
    if (n > CAP || device < 0 || device >= MAXDEV) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    if (!zeros[device]) {
        // first use: hipMalloc + a synchronous hipMemset -- neither is legal while `stream` is being captured into a graph (they
        // would invalidate the capture): the caller then pads its bias with a kernel instead, and a later eager call allocates
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(stream, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) {
            (void)hipGetLastError();
            return nullptr;
        }
        void* p = nullptr;
        if (hipMalloc(&p, CAP * sizeof(float)) != hipSuccess) return nullptr;
        if (hipMemset(p, 0, CAP * sizeof(float)) != hipSuccess) {   // synchronous: visible to every stream that follows
            (void)hipFree(p);
            return nullptr;
        }
        zeros[device] = static_cast<float*>(p);
    }
    return zeros[device];
}
}  // namespace

size_t eamm_op_conv_dev_workspace_floats(int B, int H, int W, int Cin, int Cout, int kh, int kw) {
    ConvDevPlan P;
    return conv_dev_plan(B, H, W, Cin, Cout, kh, kw, &P) ? P.packed + P.bias + P.aux + P.zbuf : 0;
}

int eamm_op_conv_dev(int device, const float* x, int B, int H, int W, int Cin, const float* weight, const float* bias, int Cout, int kh,
                     int kw, int transposed, float* out, float* workspace, size_t workspace_floats, void* stream_) {
    ConvDevPlan P;
    if (!x || !weight || !out || !workspace || !conv_dev_plan(B, H, W, Cin, Cout, kh, kw, &P))
        return fail(nullptr, EAMM_ERR_ARG, "eamm_op_conv_dev: bad argument (3x3 or 7x7, Cin a multiple of 32, Cout of 4)");
    if (workspace_floats < P.packed + P.bias + P.aux + P.zbuf || (reinterpret_cast<uintptr_t>(workspace) & 15))
        return fail(nullptr, EAMM_ERR_ARG, "eamm_op_conv_dev: workspace too small or misaligned (%zu floats needed)", P.packed + P.bias + P.aux + P.zbuf);
    DeviceGuard guard(device);
    if (guard.status != hipSuccess) return fail(nullptr, EAMM_ERR_HIP, "hipSetDevice failed");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream_);
    float *wp = workspace, *bp = workspace + P.packed, *aux = workspace + P.packed + P.bias;
    // the kernels read ntiles * BN bias values: a bias of exactly that length is read where it lies, a missing one (every data
    // gradient) is the device's shared zero vector -- the padding kernel only runs for a Cout off the tile grid
    hipError_t e = hipSuccess;
    const int nbias = P.ntiles * P.BN;
    if (bias && nbias == Cout) {
        bp = const_cast<float*>(bias);
    } else if (const float* z = bias ? nullptr : device_zeros(device, (size_t)nbias, s)) {
        bp = const_cast<float*>(z);
    } else {
        e = bias_pad_dev_launch(bias, Cout, nbias, bp, s);
    }
    if (e == hipSuccess && P.wino4) {
        WinoLayer WL;
        WL.Cin = Cin;
        WL.Cout = Cout;
        WL.tile = 4;
        WL.BN = 64;
        WL.ntiles = P.ntiles;
        WL.u = wp;
        WL.bias = bp;
        e = wino4_pack_dev_launch(weight, Cout, Cin, 64, transposed, wp, s);
        if (e == hipSuccess) e = wino4_transform_launch(x, nullptr, nullptr, B, H, W, Cin, aux, s);
        if (e == hipSuccess)
            e = wino4_gemm_launch(WL, aux, B, H, W, ACT_NONE, nullptr, out, s, P.groups > 1 ? 0 : 3, P.groups,
                                  P.groups > 1 ? aux + P.aux : nullptr, 0);
    } else if (e == hipSuccess) {
        ConvLayer& L = P.L;
        L.w = wp;
        L.bias = bp;
        e = conv_pack_dev_launch(weight, Cout, Cin, kh * kw, L.BN, transposed, wp, s);
        if (e == hipSuccess) e = conv_launch(L, conv_io(x, B, H, W, ACT_NONE, out, P.aux ? aux : nullptr, P.aux), s, 0);
    }
    if (e != hipSuccess) return fail(nullptr, EAMM_ERR_HIP, "eamm_op_conv_dev failed: %s", hipGetErrorString(e));
    return EAMM_OK;
}

// ---- the 7x7 layers with three channels on one side (conv7_thin.hip)
size_t eamm_op_conv7_thin_workspace_floats(int B, int H, int W, int N) {
    if (B < 1 || H < 1 || W < 1 || (N != 32 && N != 64)) return 0;
    return conv7_thin_workspace_floats(B, H, W, N);
}

int eamm_op_conv7_thin(int device, const float* thin, const float* weight, const float* bias, int B, int H, int W, int N, int transposed,
                       float* out, float* workspace, size_t workspace_floats, void* stream_) {
    OP_ENTRY(!thin || !weight || !out || !workspace || B < 1 || H < 1 || W < 1 || (N != 32 && N != 64) ||
                 workspace_floats < conv7_thin_workspace_floats(B, H, W, N) || (long long)B * H * W * 64 >= (1ll << 31),
             "eamm_op_conv7_thin: bad argument (N = 32 | 64, workspace of eamm_op_conv7_thin_workspace_floats)");
    hipError_t e = conv7_thin_in_launch(thin, weight, bias, B, H, W, N, transposed, out, workspace, s);
    OP_DONE(e, "eamm_op_conv7_thin");
}

int eamm_op_conv7_thin_wgrad(int device, const float* thin, const float* wide, int B, int H, int W, int N, int thin_is_input,
                             float* grad_weight, float* workspace, size_t workspace_floats, void* stream_) {
    OP_ENTRY(!thin || !wide || !grad_weight || !workspace || B < 1 || H < 1 || W < 1 || (N != 32 && N != 64) ||
                 workspace_floats < conv7_thin_workspace_floats(B, H, W, N) || (long long)B * H * W * 64 >= (1ll << 31),
             "eamm_op_conv7_thin_wgrad: bad argument");
    hipError_t e = conv7_thin_wgrad_launch(thin, wide, B, H, W, N, thin_is_input, grad_weight, workspace, s);
    OP_DONE(e, "eamm_op_conv7_thin_wgrad");
}

int eamm_op_final_conv_sigmoid(int device, const float* x, const float* weight, const float* bias, int B, int H, int W, int C,
                               float* out_nchw, float* workspace, size_t workspace_floats, void* stream_) {
    OP_ENTRY(!x || !weight || !bias || !out_nchw || !workspace || B < 1 || H < 1 || W < 1 || (C != 32 && C != 64) ||
                 workspace_floats < (size_t)7 * C * 32 || (reinterpret_cast<uintptr_t>(workspace) & 15),
             "eamm_op_final_conv_sigmoid: bad argument (C = 32 | 64, workspace of 7 * C * 32 floats)");
    hipError_t e = col7_pack_dev_launch(weight, C, workspace, s);
    if (e == hipSuccess) e = conv_col7_fused_launch(x, C, B, H, W, workspace, bias, out_nchw, s);
    OP_DONE(e, "eamm_op_final_conv_sigmoid");
}

size_t eamm_op_conv_wgrad_workspace_floats(int B, int H, int W, int Cin, int Cout, int kh, int kw) {
    if (B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || kh < 1 || kw < 1) return 0;
    return conv_wgrad_workspace_floats(B, H, W, Cin, Cout, kh, kw);
}

int eamm_op_conv_wgrad(int device, const float* x, const float* grad_out, int B, int H, int W, int Cin, int Cout, int kh, int kw,
                       float* grad_weight, float* grad_bias, float* workspace, size_t workspace_floats, void* stream_) {
    OP_ENTRY(!x || !grad_out || !grad_weight || !workspace || B < 1 || H < 1 || W < 1 || Cin < 4 || Cout < 4 || (Cin & 3) || (Cout & 3) ||
                 Cout > 1024 || kh < 1 || kw < 1 || !(kh & 1) || !(kw & 1) || kh > 7 || kw > 7,
             "eamm_op_conv_wgrad: bad argument (channels multiples of 4, Cout <= 1024, odd filter up to 7x7)");
    hipError_t e = conv_wgrad_launch(x, grad_out, B, H, W, Cin, Cout, kh, kw, grad_weight, grad_bias, workspace, workspace_floats, s);
    OP_DONE(e, "eamm_op_conv_wgrad");
}

size_t eamm_op_conv_saved_transform_offset(int B, int H, int W, int Cin, int Cout, int kh, int kw) {
    ConvDevPlan P;
    if (!conv_dev_plan(B, H, W, Cin, Cout, kh, kw, &P) || !P.wino4 || !conv_wgrad_takes_transformed(B, H, W, Cin, Cout, kh, kw))
        return (size_t)-1;
    return P.packed + P.bias;
}

int eamm_op_conv_wgrad_saved(int device, const float* x_transformed, const float* grad_out, int B, int H, int W, int Cin, int Cout,
                             float* grad_weight, float* grad_bias, float* workspace, size_t workspace_floats, void* stream_) {
    OP_ENTRY(!x_transformed || !grad_out || !grad_weight || !workspace || eamm_op_conv_saved_transform_offset(B, H, W, Cin, Cout, 3, 3) == (size_t)-1 ||
                 Cout > 1024,
             "eamm_op_conv_wgrad_saved: only where eamm_op_conv_saved_transform_offset names a saved transform");
    hipError_t e = conv_wgrad_launch(nullptr, grad_out, B, H, W, Cin, Cout, 3, 3, grad_weight, grad_bias, workspace, workspace_floats,
                                     s, x_transformed);
    OP_DONE(e, "eamm_op_conv_wgrad_saved");
}

// ---- differentiable dense-motion front end and flow head (motion.hip forward kernels, motion_backward.hip) -----------------------
int eamm_op_antialias_down(int device, const float* source, const float* aa_weight, int B, int H, int W, int inv_scale, float* small,
                           void* stream_) {
    // (inv_scale 2: forward only -- the engines' once-per-clip launch at that scale is compared with this one; the backward entry keeps 1 | 4)
    OP_ENTRY(!source || !small || B < 1 || H < 1 || W < 1 || (inv_scale != 1 && inv_scale != 2 && inv_scale != 4) ||
                     (inv_scale != 1 && !aa_weight) || H % inv_scale || W % inv_scale,
                 "eamm_op_antialias_down: bad argument (inv_scale 1 | 2 | 4: the 13x13 sigma-1.5 buffer at every scale)");
    hipError_t e = antialias_down_launch(source, aa_weight, B, H, W, inv_scale, 4, small, s);
    OP_DONE(e, "eamm_op_antialias_down");
}

int eamm_op_antialias_down_backward(int device, const float* grad_small, const float* aa_weight, int B, int H, int W, int inv_scale,
                                    float* grad_source, void* stream_) {
    OP_ENTRY(!grad_small || !grad_source || B < 1 || H < 1 || W < 1 || (inv_scale != 1 && inv_scale != 4) ||
                     (inv_scale == 4 && !aa_weight) || H % inv_scale || W % inv_scale,
                 "eamm_op_antialias_down_backward: bad argument");
    hipError_t e = antialias_down_backward_launch(grad_small, aa_weight, B, H, W, inv_scale, grad_source, s);
    OP_DONE(e, "eamm_op_antialias_down_backward");
}

int eamm_op_kp_records(int device, const float* kd_val, const float* kd_jac, const float* ks_val, const float* ks_jac, int n, int K,
                       float* records, int* singular_flag, void* stream_) {
    OP_ENTRY(!kd_val || !ks_val || !records || !singular_flag || n < 1 || K < 1 || K > 31 || ((kd_jac == nullptr) != (ks_jac == nullptr)),
                 "eamm_op_kp_records: bad argument");
    hipError_t e = kp_prepare_launch(kd_val, kd_jac, ks_val, ks_jac, n, n, K, records, singular_flag, s);
    OP_DONE(e, "eamm_op_kp_records");
}

int eamm_op_kp_records_backward(int device, const float* kd_jac, const float* ks_jac, const float* grad_records, int n, int K,
                                float* grad_kd_val, float* grad_ks_val, float* grad_kd_jac, float* grad_ks_jac, void* stream_) {
    OP_ENTRY(!grad_records || n < 1 || K < 1 || ((kd_jac == nullptr) != (ks_jac == nullptr)) ||
                     ((grad_kd_jac || grad_ks_jac) && !kd_jac),
                 "eamm_op_kp_records_backward: bad argument");
    hipError_t e = kp_records_backward_launch(kd_jac, ks_jac, grad_records, n, K, grad_kd_val, grad_ks_val, grad_kd_jac, grad_ks_jac, s);
    OP_DONE(e, "eamm_op_kp_records_backward");
}

size_t eamm_op_motion_workspace_floats(int n, int K, int h, int w) {
    if (n < 1 || K < 1 || h < 1 || w < 1) return 0;
    return motion_backward_workspace_floats(n, K, h, w);
}

int eamm_op_motion_front(int device, const float* records, const float* small, int n, int K, int h, int w, float kp_variance, int Cpad,
                         float* hourglass_in, float* sparse_deformed, void* stream_) {
    OP_ENTRY(!records || !small || !hourglass_in || n < 1 || K < 1 || K > 31 || h < 2 || w < 2 || Cpad < 4 * (K + 1) || (Cpad & 3) ||
                     !(kp_variance > 0.f),
                 "eamm_op_motion_front: bad argument");
    hipError_t e = motion_front_launch(records, small, n, n, K, h, w, kp_variance, Cpad, hourglass_in, sparse_deformed, s);
    OP_DONE(e, "eamm_op_motion_front");
}

int eamm_op_motion_front_backward(int device, const float* records, const float* small, int n, int K, int h, int w, float kp_variance,
                                  int Cpad, const float* grad_hourglass_in, const float* grad_sparse_deformed, float* grad_small,
                                  float* grad_records, float* workspace, size_t workspace_floats, void* stream_) {
    OP_ENTRY(!records || !small || !grad_records || !workspace || (!grad_hourglass_in && !grad_sparse_deformed) || n < 1 || K < 1 ||
                     K > 31 || h < 2 || w < 2 || Cpad < 4 * (K + 1) || (Cpad & 3) || !(kp_variance > 0.f) ||
                     workspace_floats < motion_backward_workspace_floats(n, K, h, w),
                 "eamm_op_motion_front_backward: bad argument");
    hipError_t e = motion_front_backward_launch(records, small, n, K, h, w, kp_variance, Cpad, grad_hourglass_in, grad_sparse_deformed,
                                                grad_small, grad_records, workspace, s);
    OP_DONE(e, "eamm_op_motion_front_backward");
}

int eamm_op_motion_head(int device, const float* mask_logits, int ld, const float* occlusion_logits, int ldo, const float* records, int n,
                        int K, int h, int w, float* mask, float* deformation, float* occlusion, void* stream_) {
    OP_ENTRY(!mask_logits || !records || !mask || !deformation || n < 1 || K < 1 || K > 31 || h < 2 || w < 2 || ld < K + 1 ||
                     (occlusion_logits && (ldo < 1 || !occlusion)),
                 "eamm_op_motion_head: bad argument");
    hipError_t e = motion_head_forward_launch(mask_logits, ld, occlusion_logits, ldo, records, n, K, h, w, mask, deformation, occlusion, s);
    OP_DONE(e, "eamm_op_motion_head");
}

int eamm_op_motion_head_backward(int device, const float* mask, const float* occlusion, const float* records, int n, int K, int h, int w,
                                 const float* grad_mask, const float* grad_deformation, const float* grad_occlusion,
                                 float* grad_mask_logits, int ld, float* grad_occlusion_logits, int ldo, float* grad_records,
                                 float* workspace, size_t workspace_floats, void* stream_) {
    OP_ENTRY(!mask || !records || !grad_mask_logits || !grad_records || !workspace || n < 1 || K < 1 || K > 31 || h < 2 || w < 2 ||
                     ld < K + 1 || (grad_occlusion_logits && (ldo < 1 || !occlusion)) ||
                     workspace_floats < motion_backward_workspace_floats(n, K, h, w),
                 "eamm_op_motion_head_backward: bad argument");
    hipError_t e = motion_head_backward_launch(mask, occlusion, records, n, K, h, w, grad_mask, grad_deformation, grad_occlusion,
                                               grad_mask_logits, ld, grad_occlusion_logits, ldo, grad_records, workspace, s);
    OP_DONE(e, "eamm_op_motion_head_backward");
}

// ---- the key-point heads' reduction as a differentiable operator (motion.hip forward kernels, kp_head_backward.hip) -----------------
size_t eamm_op_kp_head_workspace_floats(int B, int K) {
    if (B < 1 || K < 1) return 0;
    return std::max(kp_head_workspace_floats(B, K), kp_head_backward_workspace_floats(B, K));
}

int eamm_op_kp_head(int device, const float* logits, int B, int K, int njm, int h, int w, int Cs, int pad, float temperature, float* value,
                    float* jacobian, float* heatmap, float* stats, float* workspace, size_t workspace_floats, void* stream_) {
    OP_ENTRY(!logits || !value || !workspace || B < 1 || B > 65535 || K < 1 || (njm != 0 && njm != 1 && njm != K) || h < 1 || w < 1 ||
                     Cs < K + 4 * njm || pad < 0 || pad > 3 || h - 6 + 2 * pad < 1 || w - 6 + 2 * pad < 1 || !(temperature > 0.f) ||
                     workspace_floats < eamm_op_kp_head_workspace_floats(B, K),
                 "eamm_op_kp_head: bad argument (njm 0 | 1 | K, Cs >= K + 4 njm, a window of at least 1 x 1, workspace of "
                 "eamm_op_kp_head_workspace_floats)");
    hipError_t e = kp_head_launch(logits, B, K, njm, h, w, Cs, pad, temperature, value, njm > 0 ? jacobian : nullptr, heatmap, s, workspace, stats);
    OP_DONE(e, "eamm_op_kp_head");
}

int eamm_op_kp_head_backward(int device, const float* logits, const float* stats, const float* value, const float* jacobian,
                             const float* g_value, const float* g_jacobian, const float* g_heatmap, int B, int K, int njm, int h, int w, int Cs,
                             int pad, float temperature, float* grad_logits, float* workspace, size_t workspace_floats, void* stream_) {
    OP_ENTRY(!logits || !stats || !value || !grad_logits || !workspace || B < 1 || B > 65535 || K < 1 || (njm != 0 && njm != 1 && njm != K) ||
                     h < 1 || w < 1 || Cs < K + 4 * njm || (Cs & 3) || pad < 0 || pad > 3 || h - 6 + 2 * pad < 1 || w - 6 + 2 * pad < 1 ||
                     !(temperature > 0.f) || (njm > 0 && g_jacobian && !jacobian) || (long long)B * h * w * Cs >= (1ll << 31) ||
                     (reinterpret_cast<uintptr_t>(logits) & 15) || (reinterpret_cast<uintptr_t>(grad_logits) & 15) ||
                     workspace_floats < eamm_op_kp_head_workspace_floats(B, K),
                 "eamm_op_kp_head_backward: bad argument (njm 0 | 1 | K, Cs a multiple of 4 and >= K + 4 njm, 16-byte aligned tensors of "
                 "fewer than 2^31 floats, workspace of eamm_op_kp_head_workspace_floats)");
    hipError_t e = kp_head_backward_launch(logits, stats, value, jacobian, g_value, g_jacobian, g_heatmap, B, K, njm, h, w, Cs, pad, temperature,
                                           grad_logits, workspace, s);
    OP_DONE(e, "eamm_op_kp_head_backward");
}

// ---- the stride-2 convolution of Emotion_k's ResNet trunk as a differentiable operator (conv_s2.hip, conv_s2_backward.hip) ------------
namespace {
// forward: pack_conv's plain image + a zero bias + the split-K slabs, in 256-byte aligned sections of the caller's workspace
struct ConvS2Plan {
    ConvLayer L;
    size_t packed = 0, bias = 0, partial = 0;
};
bool conv_s2_plan(int B, int Hin, int Win, int Cin, int Cout, int k, ConvS2Plan* P) {
    if (!conv_s2_backward_supported(B, Hin, Win, Cin, Cout, k)) return false;
    ConvLayer& L = P->L;
    L.kh = L.kw = k;
    L.C0 = Cin;
    L.Cout = Cout;
    L.BN = conv_tile_n(Cout);
    L.ntiles = (Cout + L.BN - 1) / L.BN;
    L.nchunks = k * k * (Cin / CONV_BK);
    auto up = [](size_t n) { return (n + 63) / 64 * 64; };
    P->packed = up(conv_packed_elems(k * k, Cin, Cout, L.BN, 1));
    P->bias = up((size_t)L.ntiles * L.BN);
    P->partial = up(conv_s2_partial_elems(L, B, Hin, Win));
    return true;
}
}  // namespace

size_t eamm_op_conv_s2_workspace_floats(int B, int Hin, int Win, int Cin, int Cout, int k) {
    ConvS2Plan P;
    return conv_s2_plan(B, Hin, Win, Cin, Cout, k, &P) ? P.packed + P.bias + P.partial : 0;
}

int eamm_op_conv_s2(int device, const float* x, int B, int Hin, int Win, int Cin, const float* weight, int Cout, int k, float* out,
                    float* workspace, size_t workspace_floats, void* stream_) {
    ConvS2Plan P;
    OP_ENTRY(!x || !weight || !out || !workspace || !conv_s2_plan(B, Hin, Win, Cin, Cout, k, &P) ||
                 workspace_floats < P.packed + P.bias + P.partial || (reinterpret_cast<uintptr_t>(workspace) & 15),
             "eamm_op_conv_s2: bad argument (k 1 | 3, Hin and Win even, Cin and Cout multiples of 32, workspace of "
             "eamm_op_conv_s2_workspace_floats, 16-byte aligned)");
    ConvLayer& L = P.L;
    L.w = workspace;
    L.bias = workspace + P.packed;
    hipError_t e = conv_pack_dev_launch(weight, Cout, Cin, k * k, L.BN, 0, L.w, s);
    if (e == hipSuccess) e = bias_pad_dev_launch(nullptr, Cout, L.ntiles * L.BN, L.bias, s);
    if (e == hipSuccess)
        e = conv_s2_launch(L, x, B, Hin, Win, ACT_NONE, nullptr, out, P.partial ? workspace + P.packed + P.bias : nullptr, P.partial, s);
    OP_DONE(e, "eamm_op_conv_s2");
}

size_t eamm_op_conv_s2_dgrad_workspace_floats(int B, int Hin, int Win, int Cin, int Cout, int k) {
    return conv_s2_dgrad_workspace_floats(B, Hin, Win, Cin, Cout, k);
}

int eamm_op_conv_s2_dgrad(int device, const float* grad_out, int B, int Hin, int Win, int Cin, const float* weight, int Cout, int k,
                          float* grad_x, float* workspace, size_t workspace_floats, void* stream_) {
    const size_t need = conv_s2_dgrad_workspace_floats(B, Hin, Win, Cin, Cout, k);
    OP_ENTRY(!grad_out || !weight || !grad_x || !workspace || need == 0 || workspace_floats < need || (reinterpret_cast<uintptr_t>(workspace) & 15),
             "eamm_op_conv_s2_dgrad: bad argument (k 1 | 3, Hin and Win even, Cin and Cout multiples of 32, workspace of "
             "eamm_op_conv_s2_dgrad_workspace_floats, 16-byte aligned)");
    const hipError_t e = conv_s2_dgrad_launch(grad_out, weight, B, Hin, Win, Cin, Cout, k, grad_x, workspace, workspace_floats, s);
    OP_DONE(e, "eamm_op_conv_s2_dgrad");
}

size_t eamm_op_conv_s2_wgrad_workspace_floats(int B, int Hin, int Win, int Cin, int Cout, int k) {
    return conv_s2_wgrad_workspace_floats(B, Hin, Win, Cin, Cout, k);
}

int eamm_op_conv_s2_wgrad(int device, const float* x, const float* grad_out, int B, int Hin, int Win, int Cin, int Cout, int k,
                          float* grad_weight, float* workspace, size_t workspace_floats, void* stream_) {
    const size_t need = conv_s2_wgrad_workspace_floats(B, Hin, Win, Cin, Cout, k);
    OP_ENTRY(!x || !grad_out || !grad_weight || !workspace || need == 0 || workspace_floats < need || (reinterpret_cast<uintptr_t>(workspace) & 15),
             "eamm_op_conv_s2_wgrad: bad argument (k 1 | 3, Hin and Win even, Cin and Cout multiples of 32, workspace of "
             "eamm_op_conv_s2_wgrad_workspace_floats, 16-byte aligned)");
    const hipError_t e = conv_s2_wgrad_launch(x, grad_out, B, Hin, Win, Cin, Cout, k, grad_weight, workspace, workspace_floats, s);
    OP_DONE(e, "eamm_op_conv_s2_wgrad");
}

// ---- Emotion_k's stem max-pool and `final` Conv1d stack as differentiable operators (emotion.hip, emotion_backward.hip) ----------------
int eamm_op_emo_maxpool(int device, const float* x, int B, int H, int W, int C, float* out, void* stream_) {
    OP_ENTRY(!x || !out || B < 1 || H < 2 || W < 2 || (H & 1) || (W & 1) || C < 1 || (long long)B * H * W * C >= (1ll << 31),
             "eamm_op_emo_maxpool: bad argument (H and W even, fewer than 2^31 elements)");
    const hipError_t e = emo_maxpool_launch(x, B, H, W, C, out, s);
    OP_DONE(e, "eamm_op_emo_maxpool");
}

int eamm_op_emo_maxpool_backward(int device, const float* x, const float* grad_out, int B, int H, int W, int C, float* grad_x, void* stream_) {
    OP_ENTRY(!x || !grad_out || !grad_x || B < 1 || H < 2 || W < 2 || (H & 1) || (W & 1) || C < 1 || (long long)B * H * W * C >= (1ll << 31),
             "eamm_op_emo_maxpool_backward: bad argument (H and W even, fewer than 2^31 elements)");
    const hipError_t e = emo_maxpool_backward_launch(x, grad_out, B, H, W, C, grad_x, s);
    OP_DONE(e, "eamm_op_emo_maxpool_backward");
}

int eamm_op_emo_final(int device, const float* a, const float* w98, int B, float* value, float* jacobian, void* stream_) {
    OP_ENTRY(!a || !w98 || (!value && !jacobian) || B < 1, "eamm_op_emo_final: bad argument");
    const hipError_t e = emo_final_launch(a, w98, B, value, jacobian, s);
    OP_DONE(e, "eamm_op_emo_final");
}

size_t eamm_op_emo_final_workspace_floats(int B) { return B < 1 ? 0 : emo_final_backward_workspace_floats(B); }

int eamm_op_emo_final_backward(int device, const float* a, const float* w98, const float* g_value, const float* g_jacobian, int B,
                               float* grad_a, float* grad_w98, float* workspace, size_t workspace_floats, void* stream_) {
    OP_ENTRY(!a || !w98 || !grad_a || !grad_w98 || !workspace || B < 1 || workspace_floats < emo_final_backward_workspace_floats(B),
             "eamm_op_emo_final_backward: bad argument (workspace of eamm_op_emo_final_workspace_floats)");
    const hipError_t e = emo_final_backward_launch(a, w98, g_value, g_jacobian, B, grad_a, grad_w98, workspace, s);
    OP_DONE(e, "eamm_op_emo_final_backward");
}

}  // extern "C"

// ---- AT_net2's LSTM layer, max-pools and ConvTranspose2d(k4, s2, p1) as differentiable operators (audio.hip, lstm_backward.hip,
// audio_backward.hip) ------------------------------------------------------------------------------------------------------------
namespace {

constexpr int LSTM_OP_MAXN = 8, LSTM_OP_HID = 256, LSTM_OP_GATES = 1024;
constexpr size_t LSTM_OP_PACKED = (size_t)LSTM_WG * LSTM_OP_HID * 64;                  // lstm_rec_kernel's W_hh image
constexpr size_t LSTM_OP_STATE = (size_t)3 * LSTM_OP_MAXN * LSTM_OP_HID;               // h0, hT, c
constexpr size_t LSTM_OP_GRAN_F = (size_t)2 * 2 * LSTM_OP_MAXN * LSTM_OP_HID;          // [2][8][256] 8-byte words, in floats
constexpr size_t LSTM_OP_GRAN_B = (size_t)2 * 2 * LSTM_OP_MAXN * LSTM_OP_GATES;        // [2][8][1024] 8-byte words, in floats

// The operators' timeout word (pinned, device-mapped) and wall-clock limit, one per device of the process: an operator call has no
// handle to keep them on.  Sticky, as a handle's: after a timed-out recurrence every later call and eamm_op_lstm_check fail.
struct LstmOpState {
    int* err_host = nullptr;
    int* err_dev = nullptr;
    unsigned long long limit = 0;
};
std::mutex g_lstm_mu;
LstmOpState g_lstm[64];

hipError_t lstm_op_state(int device, LstmOpState** out) {   // the device is selected (DeviceGuard)
    if (device < 0 || device >= 64) return hipErrorInvalidDevice;
    std::lock_guard<std::mutex> lock(g_lstm_mu);
    LstmOpState& st = g_lstm[device];
    if (!st.err_host) {
        int* host = nullptr;
        if (hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&host), sizeof(int), hipHostMallocMapped | hipHostMallocCoherent); e != hipSuccess)
            return e;
        *host = 0;
        if (hipError_t e = hipHostGetDevicePointer(reinterpret_cast<void**>(&st.err_dev), host, 0); e != hipSuccess) {
            (void)hipHostFree(host);
            return e;
        }
        int khz = 100000;   // a wait may take 10 s of wall clock, as the audio handle's (eamm_audio_api.hip)
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) != hipSuccess || khz <= 0) khz = 100000;
        st.limit = (unsigned long long)khz * 1000ull * 10ull;
        st.err_host = host;
    }
    *out = &st;
    return hipSuccess;
}

bool lstm_op_shape_ok(int N, int T) { return N >= 1 && N <= LSTM_OP_MAXN && T >= 1 && (long long)N * T * LSTM_OP_GATES < (1ll << 31); }

const char* const kLstmTimedOut = "an LSTM operator's recurrence timed out waiting for another workgroup: its results are invalid (NaN from "
                                  "the step it stopped at) and the LSTM operators of this device are unusable";

}  // namespace

extern "C" {

size_t eamm_op_lstm_workspace_floats(int N, int T) { return lstm_op_shape_ok(N, T) ? LSTM_OP_PACKED + LSTM_OP_STATE + LSTM_OP_GRAN_F : 0; }

int eamm_op_lstm_forward(int device, const float* xproj, const float* w_hh, int N, int T, float* y, float* workspace, size_t workspace_floats,
                         void* stream_) {
    OP_ENTRY(!xproj || !w_hh || !y || !workspace || !lstm_op_shape_ok(N, T) || workspace_floats < eamm_op_lstm_workspace_floats(N, T) ||
                 (reinterpret_cast<uintptr_t>(workspace) & 15),
             "eamm_op_lstm_forward: bad argument (1 to 8 clips, T >= 1, workspace of eamm_op_lstm_workspace_floats, 16-byte aligned)");
    LstmOpState* st = nullptr;
    hipError_t e = lstm_op_state(device, &st);
    if (e == hipSuccess && __atomic_load_n(st->err_host, __ATOMIC_ACQUIRE)) return fail(nullptr, EAMM_ERR_HIP, "%s", kLstmTimedOut);
    float* state = workspace + LSTM_OP_PACKED;
    if (e == hipSuccess) e = lstm_pack_whh_dev_launch(w_hh, workspace, s);
    // zero state, and a granule buffer of this call's own zeroed on the stream: tags start at 1, so no stale word can match
    if (e == hipSuccess) e = hipMemsetAsync(state, 0, sizeof(float) * (LSTM_OP_STATE + LSTM_OP_GRAN_F), s);
    // a timed-out workgroup leaves without writing: the steps it did not reach stay NaN
    if (e == hipSuccess) e = hipMemsetAsync(y, 0xFF, sizeof(float) * (size_t)N * T * LSTM_OP_HID, s);
    if (e == hipSuccess) {
        LstmArgs a{};
        a.whh = workspace;
        a.xproj = xproj;
        a.clipb = nullptr;
        a.N = N;
        a.S = T;
        a.h0 = state;
        a.hT = state + LSTM_OP_MAXN * LSTM_OP_HID;
        a.c = state + 2 * LSTM_OP_MAXN * LSTM_OP_HID;
        a.y = y;
        a.ystride = (long long)T * LSTM_OP_HID;
        a.gran = reinterpret_cast<unsigned long long*>(state + LSTM_OP_STATE);
        a.epoch0 = 1;
        a.limit = st->limit;
        a.err = st->err_dev;
        e = lstm_rec_launch(a, s);
    }
    OP_DONE(e, "eamm_op_lstm_forward");
}

int eamm_op_lstm_scan(int device, float* gates, int N, int T, float* c, void* stream_) {
    OP_ENTRY(!gates || !c || !lstm_op_shape_ok(N, T), "eamm_op_lstm_scan: bad argument (1 to 8 clips, T >= 1)");
    const hipError_t e = lstm_scan_launch(gates, N, T, c, s);
    OP_DONE(e, "eamm_op_lstm_scan");
}

size_t eamm_op_lstm_backward_workspace_floats(int N, int T) { return lstm_op_shape_ok(N, T) ? LSTM_OP_GRAN_B : 0; }

int eamm_op_lstm_backward(int device, const float* acts, const float* c, const float* w_hh, const float* grad_y, int N, int T,
                          float* grad_xproj, float* workspace, size_t workspace_floats, void* stream_) {
    OP_ENTRY(!acts || !c || !w_hh || !grad_y || !grad_xproj || !workspace || !lstm_op_shape_ok(N, T) ||
                 workspace_floats < eamm_op_lstm_backward_workspace_floats(N, T) || (reinterpret_cast<uintptr_t>(workspace) & 15),
             "eamm_op_lstm_backward: bad argument (1 to 8 clips, T >= 1, workspace of eamm_op_lstm_backward_workspace_floats, 16-byte "
             "aligned)");
    LstmOpState* st = nullptr;
    hipError_t e = lstm_op_state(device, &st);
    if (e == hipSuccess && __atomic_load_n(st->err_host, __ATOMIC_ACQUIRE)) return fail(nullptr, EAMM_ERR_HIP, "%s", kLstmTimedOut);
    if (e == hipSuccess) e = hipMemsetAsync(workspace, 0, sizeof(float) * LSTM_OP_GRAN_B, s);
    if (e == hipSuccess) {
        LstmBwdArgs a{};
        a.whh = w_hh;
        a.acts = acts;
        a.c = c;
        a.dy = grad_y;
        a.dx = grad_xproj;
        a.N = N;
        a.T = T;
        a.gran = reinterpret_cast<unsigned long long*>(workspace);
        a.limit = st->limit;
        a.err = st->err_dev;
        e = lstm_bwd_launch(a, s);
    }
    OP_DONE(e, "eamm_op_lstm_backward");
}

int eamm_op_lstm_check(int device, void* stream_) {
    OP_ENTRY(false, "");
    LstmOpState* st = nullptr;
    hipError_t e = lstm_op_state(device, &st);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess && __atomic_load_n(st->err_host, __ATOMIC_ACQUIRE)) return fail(nullptr, EAMM_ERR_HIP, "%s", kLstmTimedOut);
    OP_DONE(e, "eamm_op_lstm_check");
}

int eamm_op_audio_maxpool(int device, const float* x, int B, int H, int W, int C, int sy, int sx, float* out, void* stream_) {
    OP_ENTRY(!x || !out || B < 1 || H < 3 || W < 3 || C < 4 || C % 4 || sy < 1 || sy > 2 || sx < 1 || sx > 2 ||
                 (long long)B * H * W * C >= (1ll << 31),
             "eamm_op_audio_maxpool: bad argument (map sides >= 3, strides 1 | 2, C a multiple of 4, fewer than 2^31 elements)");
    const hipError_t e = audio_maxpool_launch(x, B, H, W, C, sy, sx, out, s);
    OP_DONE(e, "eamm_op_audio_maxpool");
}

int eamm_op_audio_maxpool_backward(int device, const float* x, const float* grad_out, int B, int H, int W, int C, int sy, int sx,
                                   float* grad_x, void* stream_) {
    OP_ENTRY(!x || !grad_out || !grad_x || B < 1 || H < 3 || W < 3 || C < 4 || C % 4 || sy < 1 || sy > 2 || sx < 1 || sx > 2 ||
                 (long long)B * H * W * C >= (1ll << 31),
             "eamm_op_audio_maxpool_backward: bad argument (map sides >= 3, strides 1 | 2, C a multiple of 4, fewer than 2^31 elements)");
    const hipError_t e = audio_maxpool_backward_launch(x, grad_out, B, H, W, C, sy, sx, grad_x, s);
    OP_DONE(e, "eamm_op_audio_maxpool_backward");
}

size_t eamm_op_deconv4s2_workspace_floats(int B, int H, int W, int Cin, int Cout) { return deconv4s2_workspace_floats(B, H, W, Cin, Cout, 0); }

int eamm_op_deconv4s2(int device, const float* x, int B, int H, int W, int Cin, const float* weight, const float* bias, int Cout, float* out,
                      float* workspace, size_t workspace_floats, void* stream_) {
    const size_t need = deconv4s2_workspace_floats(B, H, W, Cin, Cout, 0);
    OP_ENTRY(!x || !weight || !out || !workspace || need == 0 || workspace_floats < need || (reinterpret_cast<uintptr_t>(workspace) & 15),
             "eamm_op_deconv4s2: bad argument (Cin and Cout multiples of 32, workspace of eamm_op_deconv4s2_workspace_floats, 16-byte "
             "aligned)");
    const hipError_t e = deconv4s2_forward_launch(x, weight, bias, B, H, W, Cin, Cout, out, workspace, workspace_floats, s);
    OP_DONE(e, "eamm_op_deconv4s2");
}

size_t eamm_op_deconv4s2_dgrad_workspace_floats(int B, int H, int W, int Cin, int Cout) {
    return deconv4s2_workspace_floats(B, H, W, Cin, Cout, 1);
}

int eamm_op_deconv4s2_dgrad(int device, const float* grad_out, int B, int H, int W, int Cin, const float* weight, int Cout, float* grad_x,
                            float* workspace, size_t workspace_floats, void* stream_) {
    const size_t need = deconv4s2_workspace_floats(B, H, W, Cin, Cout, 1);
    OP_ENTRY(!grad_out || !weight || !grad_x || !workspace || need == 0 || workspace_floats < need ||
                 (reinterpret_cast<uintptr_t>(workspace) & 15),
             "eamm_op_deconv4s2_dgrad: bad argument (Cin and Cout multiples of 32, workspace of eamm_op_deconv4s2_dgrad_workspace_floats, "
             "16-byte aligned)");
    const hipError_t e = deconv4s2_dgrad_launch(grad_out, weight, B, H, W, Cin, Cout, grad_x, workspace, workspace_floats, s);
    OP_DONE(e, "eamm_op_deconv4s2_dgrad");
}

size_t eamm_op_deconv4s2_wgrad_workspace_floats(int B, int H, int W, int Cin, int Cout) {
    return deconv4s2_workspace_floats(B, H, W, Cin, Cout, 2);
}

int eamm_op_deconv4s2_wgrad(int device, const float* x, const float* grad_out, int B, int H, int W, int Cin, int Cout, float* grad_weight,
                            float* grad_bias, float* workspace, size_t workspace_floats, void* stream_) {
    const size_t need = deconv4s2_workspace_floats(B, H, W, Cin, Cout, 2);
    OP_ENTRY(!x || !grad_out || !grad_weight || !workspace || need == 0 || workspace_floats < need ||
                 (reinterpret_cast<uintptr_t>(workspace) & 15),
             "eamm_op_deconv4s2_wgrad: bad argument (Cin and Cout multiples of 32, workspace of eamm_op_deconv4s2_wgrad_workspace_floats, "
             "16-byte aligned)");
    const hipError_t e = deconv4s2_wgrad_launch(x, grad_out, B, H, W, Cin, Cout, grad_weight, grad_bias, workspace, workspace_floats, s);
    OP_DONE(e, "eamm_op_deconv4s2_wgrad");
}

}  // extern "C"

// ---- the frozen inference path's small kernels, one launch each (conv_first.hip, motion.hip, emotion.hip, audio.hip): what the engines
// call per frame or once per clip, on the caller's buffers.  Nothing here but the argument checks and the engines' own *_launch calls.
namespace {
constexpr int OP_GRID_YZ = 65535;   // a grid's y / z extent
bool op_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
bool op_count_ok(long long a, long long b, long long c = 1, long long d = 1) {   // positive factors, product below 2^31
    if (a < 1 || b < 1 || c < 1 || d < 1) return false;
    const long long lim = 1ll << 31;
    return a < lim && b < lim && c < lim && d < lim && a * b < lim && a * b * c < lim && a * b * c * d < lim;
}
}  // namespace

extern "C" {

int eamm_op_first7(int device, const float* source, int ns, int H, int W, const float* w_host, const float* b_host, int Cout, float* out,
                   void* stream_) {
    OP_ENTRY(!source || !w_host || !b_host || !out || !first7_supported(Cout) || !op_count_ok(ns, H, W, Cout),
             "eamm_op_first7: bad argument (Cout 32 | 64 | 96 | 128, fewer than 2^31 output elements)");
    OpBuffers t(device, s);
    std::vector<float> packed((size_t)196 * Cout);
    first7_pack_host(w_host, Cout, packed.data());
    float *w = nullptr, *b = nullptr;
    int rc = upload(&t, &w, packed);
    if (!rc) rc = upload(&t, &b, std::vector<float>(b_host, b_host + Cout));
    if (rc) return fail(nullptr, rc, "%s", t.err.c_str());
    const hipError_t e = first7_launch(source, w, b, ns, H, W, Cout, out, s);
    OP_DONE(e, "eamm_op_first7");
}

int eamm_op_motion_head_infer(int device, const float* logits, const float* records, int n, int K, int h, int w, int has_occ,
                              float* deformation, float* occlusion, float* mask_out, float* occ_out, void* stream_) {
    OP_ENTRY(!logits || !records || !deformation || n < 1 || n > OP_GRID_YZ || K < 1 || K > 30 || h < 2 || w < 2 || !op_count_ok(n, h, w, 32) ||
                 (has_occ != 0 && has_occ != 1) || (has_occ && !occlusion) || !op_aligned16(logits) || (reinterpret_cast<uintptr_t>(deformation) & 7),
             "eamm_op_motion_head_infer: bad argument (1 <= K <= 30, h and w >= 2, n <= 65535, occlusion where has_occ)");
    const hipError_t e = motion_head_launch(logits, records, n, K, h, w, has_occ, deformation, occlusion, mask_out, occ_out, s);
    OP_DONE(e, "eamm_op_motion_head_infer");
}

int eamm_op_motion_head_rowsplit(int device, const float* part, int PS, int NC, const float* bias, const float* records, int n, int K, int h,
                                 int w, int has_occ, float* deformation, float* occlusion, float* mask_out, float* occ_out, void* stream_) {
    OP_ENTRY(!part || !bias || !records || !deformation || n < 1 || n > OP_GRID_YZ || K < 1 || K > 30 || h < 2 || h > OP_GRID_YZ || w < 2 ||
                 (has_occ != 0 && has_occ != 1) || (has_occ && !occlusion) || NC > 32 || NC < K + 1 + has_occ || PS < 7 * NC ||
                 !op_count_ok(n, h, w, PS) || !op_aligned16(part) || (reinterpret_cast<uintptr_t>(deformation) & 7),
             "eamm_op_motion_head_rowsplit: bad argument (1 <= K <= 30, K + 1 + has_occ <= NC <= 32, PS >= 7 NC, h and w >= 2, n and h <= "
             "65535, occlusion where has_occ)");
    const hipError_t e = motion_head_rowsplit_launch(part, PS, NC, bias, records, n, K, h, w, has_occ, deformation, occlusion, mask_out, occ_out, s);
    OP_DONE(e, "eamm_op_motion_head_rowsplit");
}

int eamm_op_final_shift_sum(int device, const float* part, const float* bias, int n, int H, int W, float* out, void* stream_) {
    OP_ENTRY(!part || !bias || !out || n < 1 || n > OP_GRID_YZ || H < 1 || H > OP_GRID_YZ || W < 1 || !op_count_ok(n, H, W, 32) || !op_aligned16(part),
             "eamm_op_final_shift_sum: bad argument (n and H <= 65535, fewer than 2^31 partial products)");
    const hipError_t e = final_shift_sum_launch(part, bias, n, H, W, out, s);
    OP_DONE(e, "eamm_op_final_shift_sum");
}

int eamm_op_to_u8(int device, const float* prediction, int n, int H, int W, uint8_t* out, void* stream_) {
    OP_ENTRY(!prediction || !out || !op_count_ok(n, H, W, 3), "eamm_op_to_u8: bad argument");
    const hipError_t e = to_u8_launch(prediction, n, H, W, out, s);
    OP_DONE(e, "eamm_op_to_u8");
}

int eamm_op_warp_image(int device, const float* source, const float* deformation, int n, int ns, int H, int W, int h, int w, int src_planes,
                       int channels, float* out, void* stream_) {
    OP_ENTRY(!source || !deformation || !out || n < 1 || (ns != 1 && ns != n) || channels < 1 || channels > src_planes ||
                 !op_count_ok(n, H, W, src_planes) || !op_count_ok(n, h, w, 2) || (reinterpret_cast<uintptr_t>(deformation) & 7),
             "eamm_op_warp_image: bad argument (ns 1 | n, 1 <= channels <= src_planes)");
    const hipError_t e = warp_image_launch(source, deformation, n, ns, H, W, h, w, out, s, src_planes, channels);
    OP_DONE(e, "eamm_op_warp_image");
}

int eamm_op_source_prepare(int device, const float* source, const float* aa_weight, int ns, int H, int W, int inv_scale, int Cpad,
                           float* source_nhwc, float* small, void* stream_) {
    OP_ENTRY(!source || !source_nhwc || !small || (inv_scale != 1 && inv_scale != 2 && inv_scale != 4) || (inv_scale != 1 && !aa_weight) ||
                 Cpad < 4 || (Cpad & 3) || !op_count_ok(ns, H, W, Cpad) || H % inv_scale || W % inv_scale || !op_aligned16(source_nhwc) ||
                 !op_aligned16(small),
             "eamm_op_source_prepare: bad argument (inv_scale 1 | 2 | 4 dividing H and W, Cpad a multiple of 4)");
    const hipError_t e = source_prepare_launch(source, aa_weight, ns, H, W, inv_scale, Cpad, source_nhwc, small, s);
    OP_DONE(e, "eamm_op_source_prepare");
}

int eamm_op_broadcast_features(int device, const float* feat, int n, int ns, int hf, int wf, int C, float* out, float* out2, const float* scale,
                               const float* shift, void* stream_) {
    OP_ENTRY(!feat || !out || n < 1 || (ns != 1 && ns != n) || C < 4 || (C & 3) || !op_count_ok(n, hf, wf, C) || (out2 && (!scale || !shift)) ||
                 !op_aligned16(feat) || !op_aligned16(out) || !op_aligned16(out2) || !op_aligned16(scale) || !op_aligned16(shift),
             "eamm_op_broadcast_features: bad argument (ns 1 | n, C a multiple of 4, scale and shift where out2, 16-byte aligned)");
    const hipError_t e = broadcast_features_launch(feat, n, ns, hf, wf, C, out, out2, scale, shift, s);
    OP_DONE(e, "eamm_op_broadcast_features");
}

int eamm_op_nchw_to_nhwc_pad(int device, const float* src, int B, int C, int planes, int H, int W, int Cpad, float* dst, void* stream_) {
    OP_ENTRY(!src || !dst || C < 1 || planes < C || Cpad < C || !op_count_ok(B, H, W, Cpad) || !op_count_ok(B, H, W, planes),
             "eamm_op_nchw_to_nhwc_pad: bad argument (1 <= C <= planes, C <= Cpad)");
    const hipError_t e = nchw_to_nhwc_pad_launch(src, B, C, H, W, Cpad, dst, s, planes);
    OP_DONE(e, "eamm_op_nchw_to_nhwc_pad");
}

int eamm_op_emo_avgpool(int device, const float* x, int B, int P, int C, float* out, void* stream_) {
    OP_ENTRY(!x || !out || !op_count_ok(B, P, C), "eamm_op_emo_avgpool: bad argument");
    const hipError_t e = emo_avgpool_launch(x, B, P, C, out, s);
    OP_DONE(e, "eamm_op_emo_avgpool");
}

int eamm_op_emo_embed(int device, const float* value, const float* jacobian, int B, float* out, void* stream_) {
    OP_ENTRY(!value || !jacobian || !out || !op_count_ok(B, 1260), "eamm_op_emo_embed: bad argument");
    const hipError_t e = emo_embed_launch(value, jacobian, B, out, s);
    OP_DONE(e, "eamm_op_emo_embed");
}

int eamm_op_emo_linear(int device, const float* x0, int K0, const float* x1, int K1, const float* wt, const float* bias, int O, int B, int relu,
                       float* out, void* stream_) {
    OP_ENTRY(!x0 || !wt || !bias || !out || K0 < 1 || K1 < 0 || (K1 > 0 && !x1) || K0 > 2048 || K1 > 2048 || K0 + K1 > 2048 || B < 1 ||
                 B > 8 * OP_GRID_YZ || !op_count_ok(K0 + K1, O) || !op_count_ok(B, O) || (relu != 0 && relu != 1),
             "eamm_op_emo_linear: bad argument (K0 >= 1, K1 >= 0 with x1 where K1 > 0, K0 + K1 <= 2048)");
    const hipError_t e = emo_linear_launch(x0, K0, x1, K1, wt, bias, O, B, relu, out, s);
    OP_DONE(e, "eamm_op_emo_linear");
}

int eamm_op_audio_conv1(int device, const float* x, const float* w, const float* b, int F, int H, int W, float* out, void* stream_) {
    OP_ENTRY(!x || !w || !b || !out || !op_count_ok(F, H, W, 64), "eamm_op_audio_conv1: bad argument");
    const hipError_t e = audio_conv1_launch(x, w, b, F, H, W, out, s);
    OP_DONE(e, "eamm_op_audio_conv1");
}

int eamm_op_audio_scale(int device, float* x, size_t n, float scale, void* stream_) {
    OP_ENTRY(!x || n < 1 || n > ((size_t)1 << 39), "eamm_op_audio_scale: bad argument (1 <= n <= 2^39)");
    const hipError_t e = audio_scale_launch(x, n, scale, s);
    OP_DONE(e, "eamm_op_audio_scale");
}

}  // extern "C"

#undef OP_ENTRY
#undef OP_DONE
