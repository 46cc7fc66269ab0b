// eamm_op_conv, the benchmark and test entry of every forward convolution family, and eamm_op_warp: the two operator entries that
// can time their launches; eamm_op_conv_ex / eamm_op_warp_ex, the same calls with the operands that only the engine sets (fused
// pre-activation, second output, NCHW store, split hand-over); eamm_op_wino_transform, the Winograd input transforms alone
// (include/eamm_hip.h).
#include "op_common.h"

namespace {

struct ConvOp {   // eamm_op_conv_ex's arguments (eamm_op_conv: everything from pre_s to split_n is zero)
    const float *in0, *in1;
    int C0, C1, B, Hin, Win, up;
    const float *w, *b;
    int Cout, kh, kw, act, pool;
    const float* resid;
    int splitk, tile_n;
    float* out;
    int iters;
    float* avg_ms;
    const float *pre_s, *pre_t;   // Winograd input transform: relu(x * pre_s + pre_t) first
    float* out2;                  // implicit GEMM: ConvIO::out2 / s2 / t2 / nchw / split_n
    const float *s2, *t2;
    int nchw, split_n;
    const char* name;             // the entry called: every refusal starts with it
    hipStream_t s;
};

// Why the call is refused before any device work (null: it is not).  The rules of the engine-only operands are conv_launch's and the
// transform kernels', checked here so that a host pointer never reaches a launch.
const char* conv_refusal(const ConvOp& a) {
    const bool staged = a.tile_n == 0 || a.tile_n == 32 || a.tile_n == 64 || a.tile_n == 128;   // the register-staged kernel
    const bool gemm = staged || (a.tile_n > 1000 && a.tile_n <= 1005);
    const bool wino = a.tile_n >= 2000 && a.tile_n < 2200;
    // 1x1 (a dense layer as build_dense packs it): the register-staged kernel only, the LDS-DMA tiles have no such instance
    const bool shape_ok = (a.kh == 3 && a.kw == 3) || (a.kh == 7 && a.kw == 7) || (a.kh == 7 && a.kw == 1) ||
                          (a.kh == 1 && a.kw == 1 && staged && !a.up);
    if (!a.in0 || !a.w || !a.b || !a.out || !shape_ok || a.C0 % CONV_BK || a.C1 % CONV_BK || (a.up && (a.kh != 3 || a.kw != 3)))
        return "bad argument";
    if ((a.tile_n == 4002 || a.tile_n == 4003) &&
        (a.kh != 7 || a.kw != 7 || a.Cout != 3 || a.act != 2 || a.up || a.pool || a.resid || a.C1 || a.C0 % 32 || a.C0 > 64 || a.C0 < 32))
        return a.tile_n == 4002 ? "unsupported fused final-layer configuration (tile code 4002)"
                                : "unsupported fused final-layer configuration (tile code 4003)";
    if ((a.pre_s != nullptr) != (a.pre_t != nullptr)) return "pre_scale and pre_shift come together";
    if (a.pre_s && !wino) return "pre_scale / pre_shift belong to the Winograd input transform (tile codes 2000, 21xx)";
    const bool second = a.out2 || a.s2 || a.t2;
    if ((second || a.nchw || a.split_n) && !gemm)
        return "out2 / scale2 / shift2 / nchw / split_n belong to the implicit GEMM (tile codes 0, 32, 64, 128, 1001..1005)";
    if (a.split_n < 0 || (a.nchw != 0 && a.nchw != 1)) return "bad nchw / split_n";
    if ((a.s2 != nullptr) != (a.t2 != nullptr) || (a.s2 && !a.out2)) return "scale2 and shift2 come together, with out2";
    if (a.out2 && !a.s2 && a.split_n == 0) return "out2 needs scale2 and shift2";
    // float4 accesses: the transforms read pre_scale / pre_shift, conv_epilogue_lds scale2 / shift2 and writes out2, four floats at a time
    if (!op_aligned16(a.pre_s) || !op_aligned16(a.pre_t) || !op_aligned16(a.out2) || !op_aligned16(a.s2) || !op_aligned16(a.t2))
        return "pre_scale, pre_shift, out2, scale2 and shift2 must be 16-byte aligned";
    if (a.pool && (a.resid || a.nchw || a.out2 || a.split_n))
        return "pool does not combine with resid, nchw, out2 or split_n (the pooled epilogue has none of them)";
    if (a.split_n > 0 && (!a.out2 || a.resid || a.nchw || a.Cout <= a.split_n || a.Cout > a.split_n + 4))
        return "split_n needs out2, no resid / pool / nchw, and split_n < Cout <= split_n + 4";
    return nullptr;
}

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

// 4002: the final layer whole (7x7, 3 output channels, bias, sigmoid -> NCHW) on the fused column-patch kernel as the engine
// runs it: the row-split weights of its final_w_swz and their three-plane image final_w3 (split-bf16 products); 4003: the same
// with fp32 products forced (no three-plane image)
int op_conv_final(OpBuffers* t, const ConvOp& a) {
    HostConv f = op_weights(a, a.C0);
    const std::vector<float> bias = to_rowsplit(&f);
    float *w = nullptr, *b = nullptr, *w3 = nullptr;
    int rc = upload_conv_image(t, &w, f, nullptr, a.C0, conv_tile_n(f.Cout), MODE_PLAIN, true);
    if (rc || (rc = upload(t, &b, bias)) || (a.tile_n == 4002 && (rc = upload_col7_split(t, &w3, f, nullptr, a.C0)))) return rc;
    auto fused_final = [&]() { return conv_col7_fused_launch(a.in0, a.C0, a.B, a.Hin, a.Win, w, b, a.out, a.s, w3); };
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
        return fail(t, EAMM_ERR_ARG, "%s: unsupported column-patch configuration", a.name);
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
        return fail(t, EAMM_ERR_ARG, "%s: unsupported patch-kernel configuration", a.name);
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
        return fail(t, EAMM_ERR_ARG, "%s: unsupported Winograd configuration", a.name);
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
            if (tr) e = wino4_transform_launch(a.in0, a.pre_s, a.pre_t, a.B, a.Hin, a.Win, a.C0, V, a.s);
            if (e != hipSuccess || !gm) return e;
            return wino4_gemm_launch(W, V, a.B, a.Hin, a.Win, a.act, a.resid, a.out, a.s, w4_variant, w4_groups, Zb, a.pool);
        }
        if (tr) e = wino_transform_launch(a.in0, a.pre_s, a.pre_t, a.B, a.Hin, a.Win, a.C0, V, a.s);
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
        if (!conv_dma_tile(dma_cfg, &BM, &BN) || a.kw == 1 || a.kh == 7) return fail(t, EAMM_ERR_ARG, "%s: unknown / unsupported dma tile", a.name);
    } else if (BN != 32 && BN != 64 && BN != 128) {
        return fail(t, EAMM_ERR_ARG, "%s: tile_n must be 32/64/128 or 1000+dma id", a.name);
    }
    ConvLayer L;
    int rc = pack_conv(t, op_weights(a, a.C0 + a.C1), nullptr, a.C0, a.C1, a.up ? MODE_PHASE : MODE_PLAIN, dma_cfg, &L, dma_cfg ? 0 : BN);
    if (rc) return rc;
    ConvIO io = conv_io(a.in0, a.B, a.Hin, a.Win, a.act, a.out, nullptr, conv_plan(L, a.B * a.Hin * a.Win, a.splitk).partial_elems);
    io.in1 = a.C1 ? a.in1 : nullptr;
    io.pool = a.pool;
    io.resid = a.resid;
    io.nchw = a.nchw;
    io.out2 = a.out2;
    io.s2 = a.s2;
    io.t2 = a.t2;
    io.split_n = a.split_n;
    if (io.partial_cap && (rc = dev_alloc(t, &io.partial, io.partial_cap))) return rc;
    auto gemm = [&]() { return conv_launch(L, io, a.s, a.splitk); };
    HIP_TRY(t, gemm());
    HIP_TRY(t, time_launches(a.s, a.iters, a.avg_ms, gemm));
    return EAMM_OK;
}

// eamm_op_conv: the family of tile_n (include/eamm_hip.h), then the caller's stream drained
int op_conv_run(OpBuffers* t, const ConvOp& a) {
    int rc;
    if (a.tile_n == 4002 || a.tile_n == 4003) rc = op_conv_final(t, a);
    else if (a.tile_n == 4000 || a.tile_n == 4001) rc = op_conv_col7(t, a);
    else if (a.tile_n == 3000 || a.tile_n == 3003 || a.tile_n == 3004) rc = op_conv_patch(t, a);
    else if (a.tile_n >= 2000 && a.tile_n < 2200) rc = op_conv_wino(t, a);
    else rc = op_conv_gemm(t, a);
    if (rc) return rc;
    HIP_TRY(t, hipStreamSynchronize(a.s));
    return EAMM_OK;
}

// eamm_op_conv / eamm_op_conv_ex under the caller's name (a.name)
int op_conv_call(int device, ConvOp a, void* stream_) {
    if (const char* why = conv_refusal(a)) return fail(nullptr, EAMM_ERR_ARG, "%s: %s", a.name, why);
    DeviceGuard guard(device);
    if (guard.status != hipSuccess) return fail(nullptr, EAMM_ERR_HIP, "hipSetDevice failed");
    a.s = reinterpret_cast<hipStream_t>(stream_);
    OpBuffers t(device, a.s);
    if (int rc = op_conv_run(&t, a)) return fail(nullptr, rc, "%s", t.err.c_str());
    return EAMM_OK;
}

// eamm_op_warp / eamm_op_warp_ex under the caller's `name`
int op_warp_call(const char* name, int device, const float* feat, const float* deformation, const float* occlusion, int n, int ns, int hf,
                 int wf, int C, int h, int w, float* out, float* out2, const float* scale2, const float* shift2, int iters, float* avg_ms,
                 void* stream_) {
    if (!feat || !deformation || !out || n < 1 || (ns != 1 && ns != n) || hf < 1 || wf < 1 || h < 1 || w < 1 || C < 8 || (C & 7) ||
        (out2 != nullptr) != (scale2 != nullptr) || (out2 != nullptr) != (shift2 != nullptr))
        return fail(nullptr, EAMM_ERR_ARG, "%s: bad argument", name);
    DeviceGuard guard(device);
    if (guard.status != hipSuccess) return fail(nullptr, EAMM_ERR_HIP, "hipSetDevice failed");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream_);
    auto run = [&]() { return warp_features_launch(feat, deformation, occlusion, n, ns, hf, wf, C, h, w, out, out2, scale2, shift2, s); };
    hipError_t e = run();
    if (e == hipSuccess) e = time_launches(s, iters, avg_ms, run);
    // (no stream synchronisation outside the timing branch: like every other operator entry the work is only ENQUEUED on
    // `stream` -- the differentiable forward calls this three times per pass and must stay capturable)
    if (e == hipSuccess) e = hipGetLastError();
    OP_DONE(e, name);
}

}  // namespace

extern "C" {

int eamm_op_conv_ex(int device, const float* in0, int C0, const float* in1, int C1, int B, int Hin, int Win, int up,
                    const float* w_host, const float* b_host, int Cout, int kh, int kw, int act, int pool,
                    const float* resid, int splitk, int tile_n, float* out, int iters, float* avg_ms,
                    const float* pre_scale, const float* pre_shift, float* out2, const float* scale2, const float* shift2, int nchw,
                    int split_n, void* stream_) {
    return op_conv_call(device,
                        ConvOp{in0, in1, C0, C1, B, Hin, Win, up, w_host, b_host, Cout, kh, kw, act, pool, resid, splitk, tile_n, out, iters,
                               avg_ms, pre_scale, pre_shift, out2, scale2, shift2, nchw, split_n, "eamm_op_conv_ex", nullptr},
                        stream_);
}

int eamm_op_conv(int device, const float* in0, int C0, const float* in1, int C1, int B, int Hin, int Win, int up,
                 const float* w_host, const float* b_host, int Cout, int kh, int kw, int act, int pool,
                 const float* resid, int splitk, int tile_n, float* out, int iters, float* avg_ms, void* stream_) {
    return op_conv_call(device,
                        ConvOp{in0, in1, C0, C1, B, Hin, Win, up, w_host, b_host, Cout, kh, kw, act, pool, resid, splitk, tile_n, out, iters,
                               avg_ms, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, "eamm_op_conv", nullptr},
                        stream_);
}

// the final layer's host packing alone (no device): the row-split fp32 weights and their three-plane bf16 image
size_t eamm_final_split_planes_elems(int C) { return (C == 32 || C == 64) ? 2 * col7_split_packed_elems(C) : 0; }
int eamm_final_split_planes(const float* w_host, int C, float* rowsplit, uint16_t* planes) {
    if (!w_host || !rowsplit || !planes || (C != 32 && C != 64))
        return fail(nullptr, EAMM_ERR_ARG, "eamm_final_split_planes: bad argument (C = 32 | 64)");
    HostConv f;
    f.Cout = 3;
    f.Cin = C;
    f.kh = f.kw = 7;
    f.w.assign(w_host, w_host + (size_t)3 * C * 49);
    f.b.assign(3, 0.f);
    to_rowsplit(&f);
    std::copy(f.w.begin(), f.w.end(), rowsplit);
    col7_pack_split_host(f.w.data(), f.Cout, f.Cin, nullptr, C, planes);
    return EAMM_OK;
}

// the Winograd input transform alone, as the engine launches it: V[(tile + 2)^2][B * H/tile * W/tile][C]
int eamm_op_wino_transform(int device, const float* x, const float* scale, const float* shift, int B, int H, int W, int C, int tile,
                           float* V, void* stream_) {
    const bool tile_ok = tile == 2 || tile == 4;
    OP_ENTRY(!x || !V || !tile_ok || B < 1 || H < 1 || W < 1 || C < 1 || H % tile || W % tile || (C & 3) ||
                 (scale != nullptr) != (shift != nullptr) || !op_aligned16(x) || !op_aligned16(V) || !op_aligned16(scale) ||
                 !op_aligned16(shift) || !op_count_ok((tile + 2) * (tile + 2), (long long)B * (H / tile) * (W / tile), C),
             "eamm_op_wino_transform: bad argument");
    OP_DONE(tile == 4 ? wino4_transform_launch(x, scale, shift, B, H, W, C, V, s) : wino_transform_launch(x, scale, shift, B, H, W, C, V, s),
            "eamm_op_wino_transform");
}

int eamm_op_warp_ex(int device, const float* feat, const float* deformation, const float* occlusion, int n, int ns, int hf, int wf, int C,
                    int h, int w, float* out, int iters, float* avg_ms, float* out2, const float* scale2, const float* shift2,
                    void* stream_) {
    return op_warp_call("eamm_op_warp_ex", device, feat, deformation, occlusion, n, ns, hf, wf, C, h, w, out, out2, scale2, shift2, iters,
                        avg_ms, stream_);
}

int eamm_op_warp(int device, const float* feat, const float* deformation, const float* occlusion, int n, int ns, int hf,
                 int wf, int C, int h, int w, float* out, int iters, float* avg_ms, void* stream_) {
    return op_warp_call("eamm_op_warp", device, feat, deformation, occlusion, n, ns, hf, wf, C, h, w, out, nullptr, nullptr, nullptr, iters,
                        avg_ms, stream_);
}

}  // extern "C"
