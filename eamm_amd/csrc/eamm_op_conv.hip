// eamm_op_conv, the benchmark and test entry of every forward convolution family, and eamm_op_warp: the two operator entries that
// can time their launches (include/eamm_hip.h).
#include "op_common.h"

namespace {

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

// spatial-patch kernels of the up-convolution: 3000 collapsed-phase form, 3003 polyphase minimal-filtering form as the engine
// runs a decoder up block (splitk > 1: its channel reduction over that many workgroups, fp32 products; else the split-bf16
// products), 3004 the polyphase form with fp32 products forced
int op_conv_patch(OpBuffers* t, const ConvOp& a) {
    const bool pp = a.tile_n == 3003 || a.tile_n == 3004;
    const int psplit = a.splitk > 1 ? a.splitk : 1;
    if (a.kh != 3 || a.kw != 3 || !a.up || a.pool || a.resid || (a.Cout & 3) || (psplit > 1 && (!pp || ((a.C0 + a.C1) / 32) % psplit)))
        return fail(t, EAMM_ERR_ARG, "eamm_op_conv: unsupported patch-kernel configuration");
    PatchLayer P;
    float* ppart = nullptr;
    const size_t ppart_elems = psplit > 1 ? (size_t)psplit * a.B * 4 * a.Hin * a.Win * a.Cout : 0;
    int rc = pack_patch(t, op_weights(a, a.C0 + a.C1), nullptr, a.C0, a.C1, pp, &P, a.tile_n == 3003);
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
    else if (a.tile_n == 3000 || a.tile_n == 3003 || a.tile_n == 3004) rc = op_conv_patch(t, a);
    else if (a.tile_n >= 2000 && a.tile_n < 2200) rc = op_conv_wino(t, a);
    else rc = op_conv_gemm(t, a);
    if (rc) return rc;
    HIP_TRY(t, hipStreamSynchronize(a.s));
    return EAMM_OK;
}

}  // namespace

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

}  // extern "C"
