// The training path's convolutions as operator entries: DEVICE weights, packed on the device into the caller's workspace, then the
// forward kernels; the thin 7x7 layers; the weight gradients; the stride-2 and the transposed 4x4 convolutions with their gradients.
#include "op_common.h"

// ---- convolution with DEVICE weights (training path): pack on the device into the caller's workspace, then the forward kernels
namespace {

struct ConvDevPlan {
    bool wino4 = false;
    int groups = 1;         // F(4x4): rows of transform points split over this many workgroups per tile (few tiles), as the engine does
    size_t zbuf = 0;        // floats of the split form's x-folded products
    int BN = 0, ntiles = 0;
    size_t packed = 0, bias = 0, aux = 0;   // floats, in 256-byte aligned sections: packed filter, padded bias, Winograd V or split-K partials
    ConvLayer L;
};
bool conv_dev_plan(int B, int H, int W, int Cin, int Cout, int kh, int kw, ConvDevPlan* P) {
    if (B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || Cin % CONV_BK || (Cout & 3)) return false;
    if (!((kh == 3 && kw == 3) || (kh == 7 && kw == 7) || (kh == 1 && kw == 1))) return false;   // 1x1: the discriminator's prediction layer
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
        P->packed = round64(wino4_packed_elems(Cout, Cin, 64));
        P->aux = round64((size_t)36 * Mq * Cin);
        // a single launch of <= 128 64-tile workgroups leaves half the chip idle (the engine runs two chains there): split
        // the transform-point rows over 2 / 3 / 6 workgroups per tile, as the engine's one-chain calls do
        const long long nb = ((Mq + 63) / 64) * P->ntiles;
        for (int gsel : {6, 3, 2})
            if (nb * gsel <= 256) {
                P->groups = gsel;
                break;
            }
        if (P->groups > 1) P->zbuf = round64((size_t)24 * Mq * Cout);
    } else {
        ConvLayer& L = P->L = plain_conv_layer(kh, kw, Cin, Cout);
        P->BN = L.BN;
        P->ntiles = L.ntiles;
        P->packed = round64(conv_packed_elems(kh * kw, Cin, Cout, L.BN, 1));
        P->aux = round64(conv_plan(L, B * H * W, 0).partial_elems);
    }
    P->bias = round64((size_t)P->ntiles * P->BN);
    return true;
}

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

// the stride-2 forward: pack_conv's plain image + a zero bias + the split-K slabs, in 256-byte aligned sections of the caller's workspace
struct ConvS2Plan {
    ConvLayer L;
    size_t packed = 0, bias = 0, partial = 0;
};
bool conv_s2_plan(int B, int Hin, int Win, int Cin, int Cout, int k, ConvS2Plan* P) {
    if (!conv_s2_backward_supported(B, Hin, Win, Cin, Cout, k)) return false;
    const ConvLayer& L = P->L = plain_conv_layer(k, k, Cin, Cout);
    P->packed = round64(conv_packed_elems(k * k, Cin, Cout, L.BN, 1));
    P->bias = round64((size_t)L.ntiles * L.BN);
    P->partial = round64(conv_s2_partial_elems(L, B, Hin, Win));
    return true;
}

}  // namespace

extern "C" {

size_t eamm_op_conv_dev_workspace_floats(int B, int H, int W, int Cin, int Cout, int kh, int kw) {
    ConvDevPlan P;
    return conv_dev_plan(B, H, W, Cin, Cout, kh, kw, &P) ? P.packed + P.bias + P.aux + P.zbuf : 0;
}

int eamm_op_conv_dev(int device, const float* x, int B, int H, int W, int Cin, const float* weight, const float* bias, int Cout, int kh,
                     int kw, int transposed, float* out, float* workspace, size_t workspace_floats, void* stream_) {
    ConvDevPlan P;
    if (!x || !weight || !out || !workspace || !conv_dev_plan(B, H, W, Cin, Cout, kh, kw, &P))
        return fail(nullptr, EAMM_ERR_ARG, "eamm_op_conv_dev: bad argument (1x1, 3x3 or 7x7, Cin a multiple of 32, Cout of 4)");
    const size_t need = P.packed + P.bias + P.aux + P.zbuf;
    if (!op_workspace_ok(workspace, workspace_floats, need, true))
        return fail(nullptr, EAMM_ERR_ARG, "eamm_op_conv_dev: workspace too small or misaligned (%zu floats needed)", need);
    OP_ENTRY(false, "");
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
    OP_DONE(e, "eamm_op_conv_dev");
}

// ---- the 7x7 layers with three channels on one side (conv7_thin.hip)
size_t eamm_op_conv7_thin_workspace_floats(int B, int H, int W, int N) {
    return B < 1 || H < 1 || W < 1 || (N != 32 && N != 64) ? 0 : conv7_thin_workspace_floats(B, H, W, N);
}

int eamm_op_conv7_thin(int device, const float* thin, const float* weight, const float* bias, int B, int H, int W, int N, int transposed,
                       float* out, float* workspace, size_t workspace_floats, void* stream_) {
    OP_ENTRY(!thin || !weight || !out || B < 1 || H < 1 || W < 1 || (N != 32 && N != 64) || (long long)B * H * W * 64 >= (1ll << 31) ||
                 !op_workspace_ok(workspace, workspace_floats, conv7_thin_workspace_floats(B, H, W, N), false),
             "eamm_op_conv7_thin: bad argument (N = 32 | 64, workspace of eamm_op_conv7_thin_workspace_floats)");
    OP_DONE(conv7_thin_in_launch(thin, weight, bias, B, H, W, N, transposed, out, workspace, s), "eamm_op_conv7_thin");
}

int eamm_op_conv7_thin_wgrad(int device, const float* thin, const float* wide, int B, int H, int W, int N, int thin_is_input,
                             float* grad_weight, float* workspace, size_t workspace_floats, void* stream_) {
    OP_ENTRY(!thin || !wide || !grad_weight || B < 1 || H < 1 || W < 1 || (N != 32 && N != 64) || (long long)B * H * W * 64 >= (1ll << 31) ||
                 !op_workspace_ok(workspace, workspace_floats, conv7_thin_workspace_floats(B, H, W, N), false),
             "eamm_op_conv7_thin_wgrad: bad argument");
    OP_DONE(conv7_thin_wgrad_launch(thin, wide, B, H, W, N, thin_is_input, grad_weight, workspace, s), "eamm_op_conv7_thin_wgrad");
}

int eamm_op_final_conv_sigmoid(int device, const float* x, const float* weight, const float* bias, int B, int H, int W, int C,
                               float* out_nchw, float* workspace, size_t workspace_floats, void* stream_) {
    OP_ENTRY(!x || !weight || !bias || !out_nchw || B < 1 || H < 1 || W < 1 || (C != 32 && C != 64) ||
                 !op_workspace_ok(workspace, workspace_floats, (size_t)7 * C * 32, true),
             "eamm_op_final_conv_sigmoid: bad argument (C = 32 | 64, workspace of 7 * C * 32 floats)");
    hipError_t e = col7_pack_dev_launch(weight, C, workspace, s);
    if (e == hipSuccess) e = conv_col7_fused_launch(x, C, B, H, W, workspace, bias, out_nchw, s);
    OP_DONE(e, "eamm_op_final_conv_sigmoid");
}

size_t eamm_op_conv_wgrad_workspace_floats(int B, int H, int W, int Cin, int Cout, int kh, int kw) {
    return B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || kh < 1 || kw < 1 ? 0 : conv_wgrad_workspace_floats(B, H, W, Cin, Cout, kh, kw);
}

int eamm_op_conv_wgrad(int device, const float* x, const float* grad_out, int B, int H, int W, int Cin, int Cout, int kh, int kw,
                       float* grad_weight, float* grad_bias, float* workspace, size_t workspace_floats, void* stream_) {
    OP_ENTRY(!x || !grad_out || !grad_weight || !workspace || B < 1 || H < 1 || W < 1 || Cin < 4 || Cout < 4 || (Cin & 3) || (Cout & 3) ||
                 Cout > 1024 || kh < 1 || kw < 1 || !(kh & 1) || !(kw & 1) || kh > 7 || kw > 7,
             "eamm_op_conv_wgrad: bad argument (channels multiples of 4, Cout <= 1024, odd filter up to 7x7)");
    OP_DONE(conv_wgrad_launch(x, grad_out, B, H, W, Cin, Cout, kh, kw, grad_weight, grad_bias, workspace, workspace_floats, s), "eamm_op_conv_wgrad");
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

// ---- the stride-2 convolution of Emotion_k's ResNet trunk as a differentiable operator (conv_s2.hip, conv_s2_backward.hip) ------------
size_t eamm_op_conv_s2_workspace_floats(int B, int Hin, int Win, int Cin, int Cout, int k) {
    ConvS2Plan P;
    return conv_s2_plan(B, Hin, Win, Cin, Cout, k, &P) ? P.packed + P.bias + P.partial : 0;
}

int eamm_op_conv_s2(int device, const float* x, int B, int Hin, int Win, int Cin, const float* weight, int Cout, int k, float* out,
                    float* workspace, size_t workspace_floats, void* stream_) {
    ConvS2Plan P;
    OP_ENTRY(!x || !weight || !out || !conv_s2_plan(B, Hin, Win, Cin, Cout, k, &P) ||
                 !op_workspace_ok(workspace, workspace_floats, P.packed + P.bias + P.partial, true),
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
    OP_ENTRY(!grad_out || !weight || !grad_x || need == 0 || !op_workspace_ok(workspace, workspace_floats, need, true),
             "eamm_op_conv_s2_dgrad: bad argument (k 1 | 3, Hin and Win even, Cin and Cout multiples of 32, workspace of "
             "eamm_op_conv_s2_dgrad_workspace_floats, 16-byte aligned)");
    OP_DONE(conv_s2_dgrad_launch(grad_out, weight, B, Hin, Win, Cin, Cout, k, grad_x, workspace, workspace_floats, s), "eamm_op_conv_s2_dgrad");
}

size_t eamm_op_conv_s2_wgrad_workspace_floats(int B, int Hin, int Win, int Cin, int Cout, int k) {
    return conv_s2_wgrad_workspace_floats(B, Hin, Win, Cin, Cout, k);
}

int eamm_op_conv_s2_wgrad(int device, const float* x, const float* grad_out, int B, int Hin, int Win, int Cin, int Cout, int k,
                          float* grad_weight, float* workspace, size_t workspace_floats, void* stream_) {
    const size_t need = conv_s2_wgrad_workspace_floats(B, Hin, Win, Cin, Cout, k);
    OP_ENTRY(!x || !grad_out || !grad_weight || need == 0 || !op_workspace_ok(workspace, workspace_floats, need, true),
             "eamm_op_conv_s2_wgrad: bad argument (k 1 | 3, Hin and Win even, Cin and Cout multiples of 32, workspace of "
             "eamm_op_conv_s2_wgrad_workspace_floats, 16-byte aligned)");
    OP_DONE(conv_s2_wgrad_launch(x, grad_out, B, Hin, Win, Cin, Cout, k, grad_weight, workspace, workspace_floats, s), "eamm_op_conv_s2_wgrad");
}

// ---- AT_net2's ConvTranspose2d(k4, s2, p1) as a differentiable operator (audio_backward.hip) -------------------------------------------
size_t eamm_op_deconv4s2_workspace_floats(int B, int H, int W, int Cin, int Cout) { return deconv4s2_workspace_floats(B, H, W, Cin, Cout, 0); }

int eamm_op_deconv4s2(int device, const float* x, int B, int H, int W, int Cin, const float* weight, const float* bias, int Cout, float* out,
                      float* workspace, size_t workspace_floats, void* stream_) {
    const size_t need = deconv4s2_workspace_floats(B, H, W, Cin, Cout, 0);
    OP_ENTRY(!x || !weight || !out || need == 0 || !op_workspace_ok(workspace, workspace_floats, need, true),
             "eamm_op_deconv4s2: bad argument (Cin and Cout multiples of 32, workspace of eamm_op_deconv4s2_workspace_floats, 16-byte "
             "aligned)");
    OP_DONE(deconv4s2_forward_launch(x, weight, bias, B, H, W, Cin, Cout, out, workspace, workspace_floats, s), "eamm_op_deconv4s2");
}

size_t eamm_op_deconv4s2_dgrad_workspace_floats(int B, int H, int W, int Cin, int Cout) {
    return deconv4s2_workspace_floats(B, H, W, Cin, Cout, 1);
}

int eamm_op_deconv4s2_dgrad(int device, const float* grad_out, int B, int H, int W, int Cin, const float* weight, int Cout, float* grad_x,
                            float* workspace, size_t workspace_floats, void* stream_) {
    const size_t need = deconv4s2_workspace_floats(B, H, W, Cin, Cout, 1);
    OP_ENTRY(!grad_out || !weight || !grad_x || need == 0 || !op_workspace_ok(workspace, workspace_floats, need, true),
             "eamm_op_deconv4s2_dgrad: bad argument (Cin and Cout multiples of 32, workspace of eamm_op_deconv4s2_dgrad_workspace_floats, "
             "16-byte aligned)");
    OP_DONE(deconv4s2_dgrad_launch(grad_out, weight, B, H, W, Cin, Cout, grad_x, workspace, workspace_floats, s), "eamm_op_deconv4s2_dgrad");
}

size_t eamm_op_deconv4s2_wgrad_workspace_floats(int B, int H, int W, int Cin, int Cout) {
    return deconv4s2_workspace_floats(B, H, W, Cin, Cout, 2);
}

int eamm_op_deconv4s2_wgrad(int device, const float* x, const float* grad_out, int B, int H, int W, int Cin, int Cout, float* grad_weight,
                            float* grad_bias, float* workspace, size_t workspace_floats, void* stream_) {
    const size_t need = deconv4s2_workspace_floats(B, H, W, Cin, Cout, 2);
    OP_ENTRY(!x || !grad_out || !grad_weight || need == 0 || !op_workspace_ok(workspace, workspace_floats, need, true),
             "eamm_op_deconv4s2_wgrad: bad argument (Cin and Cout multiples of 32, workspace of eamm_op_deconv4s2_wgrad_workspace_floats, "
             "16-byte aligned)");
    const hipError_t e = deconv4s2_wgrad_launch(x, grad_out, B, H, W, Cin, Cout, grad_weight, grad_bias, workspace, workspace_floats, s);
    OP_DONE(e, "eamm_op_deconv4s2_wgrad");
}

}  // extern "C"
