// The differentiable operators of the training graph that are no convolutions: the warp's backward (warp.hip), the dense-motion front end and
// flow head, the key-point heads' reduction, Emotion_k's max-pool and `final` stack, AT_net2's LSTM layer and max-pools.
#include "op_common.h"

// ---- the LSTM operators' sizes and per-device state (audio.hip, lstm_backward.hip)
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

// ---- differentiable dense-motion front end and flow head (motion.hip, motion_backward.hip) ----------------------------------------
int eamm_op_antialias_down(int device, const float* source, const float* aa_weight, int B, int H, int W, int inv_scale, float* small,
                           void* stream_) {
    // (inv_scale 2: forward only -- the engines' once-per-clip launch at that scale is compared with this one; the backward entry keeps 1 | 4)
    OP_ENTRY(!source || !small || B < 1 || H < 1 || W < 1 || (inv_scale != 1 && inv_scale != 2 && inv_scale != 4) ||
                     (inv_scale != 1 && !aa_weight) || H % inv_scale || W % inv_scale,
                 "eamm_op_antialias_down: bad argument (inv_scale 1 | 2 | 4: the 13x13 sigma-1.5 buffer at every scale)");
    OP_DONE(antialias_down_launch(source, aa_weight, B, H, W, inv_scale, 4, small, s), "eamm_op_antialias_down");
}

int eamm_op_antialias_down_backward(int device, const float* grad_small, const float* aa_weight, int B, int H, int W, int inv_scale,
                                    float* grad_source, void* stream_) {
    OP_ENTRY(!grad_small || !grad_source || B < 1 || H < 1 || W < 1 || (inv_scale != 1 && inv_scale != 4) ||
                     (inv_scale == 4 && !aa_weight) || H % inv_scale || W % inv_scale,
                 "eamm_op_antialias_down_backward: bad argument");
    OP_DONE(antialias_down_backward_launch(grad_small, aa_weight, B, H, W, inv_scale, grad_source, s), "eamm_op_antialias_down_backward");
}

int eamm_op_kp_records(int device, const float* kd_val, const float* kd_jac, const float* ks_val, const float* ks_jac, int n, int K,
                       float* records, int* singular_flag, void* stream_) {
    OP_ENTRY(!kd_val || !ks_val || !records || !singular_flag || n < 1 || K < 1 || K > 31 || ((kd_jac == nullptr) != (ks_jac == nullptr)),
                 "eamm_op_kp_records: bad argument");
    OP_DONE(kp_prepare_launch(kd_val, kd_jac, ks_val, ks_jac, n, n, K, records, singular_flag, s), "eamm_op_kp_records");
}

int eamm_op_kp_records_backward(int device, const float* kd_jac, const float* ks_jac, const float* grad_records, int n, int K,
                                float* grad_kd_val, float* grad_ks_val, float* grad_kd_jac, float* grad_ks_jac, void* stream_) {
    OP_ENTRY(!grad_records || n < 1 || K < 1 || ((kd_jac == nullptr) != (ks_jac == nullptr)) || ((grad_kd_jac || grad_ks_jac) && !kd_jac),
                 "eamm_op_kp_records_backward: bad argument");
    hipError_t e = kp_records_backward_launch(kd_jac, ks_jac, grad_records, n, K, grad_kd_val, grad_ks_val, grad_kd_jac, grad_ks_jac, s);
    OP_DONE(e, "eamm_op_kp_records_backward");
}

size_t eamm_op_motion_workspace_floats(int n, int K, int h, int w) {
    return n < 1 || K < 1 || h < 1 || w < 1 ? 0 : motion_backward_workspace_floats(n, K, h, w);
}

int eamm_op_motion_front(int device, const float* records, const float* small, int n, int K, int h, int w, float kp_variance, int Cpad,
                         float* hourglass_in, float* sparse_deformed, void* stream_) {
    OP_ENTRY(!records || !small || !hourglass_in || n < 1 || K < 1 || K > 31 || h < 2 || w < 2 || Cpad < 4 * (K + 1) || (Cpad & 3) ||
                     !(kp_variance > 0.f),
                 "eamm_op_motion_front: bad argument");
    OP_DONE(motion_front_launch(records, small, n, n, K, h, w, kp_variance, Cpad, hourglass_in, sparse_deformed, s), "eamm_op_motion_front");
}

int eamm_op_motion_front_backward(int device, const float* records, const float* small, int n, int K, int h, int w, float kp_variance,
                                  int Cpad, const float* grad_hourglass_in, const float* grad_sparse_deformed, float* grad_small,
                                  float* grad_records, float* workspace, size_t workspace_floats, void* stream_) {
    OP_ENTRY(!records || !small || !grad_records || (!grad_hourglass_in && !grad_sparse_deformed) || n < 1 || K < 1 || K > 31 || h < 2 ||
                     w < 2 || Cpad < 4 * (K + 1) || (Cpad & 3) || !(kp_variance > 0.f) ||
                     !op_workspace_ok(workspace, workspace_floats, motion_backward_workspace_floats(n, K, h, w), false),
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
    OP_ENTRY(!mask || !records || !grad_mask_logits || !grad_records || n < 1 || K < 1 || K > 31 || h < 2 || w < 2 || ld < K + 1 ||
                     (grad_occlusion_logits && (ldo < 1 || !occlusion)) ||
                     !op_workspace_ok(workspace, workspace_floats, motion_backward_workspace_floats(n, K, h, w), false),
                 "eamm_op_motion_head_backward: bad argument");
    hipError_t e = motion_head_backward_launch(mask, occlusion, records, n, K, h, w, grad_mask, grad_deformation, grad_occlusion,
                                               grad_mask_logits, ld, grad_occlusion_logits, ldo, grad_records, workspace, s);
    OP_DONE(e, "eamm_op_motion_head_backward");
}

// ---- the key-point heads' reduction as a differentiable operator (kp_head.hip) ------------------------------------------------------
size_t eamm_op_kp_head_workspace_floats(int B, int K) {
    return B < 1 || K < 1 ? 0 : std::max(kp_head_workspace_floats(B, K), kp_head_backward_workspace_floats(B, K));
}

int eamm_op_kp_head(int device, const float* logits, int B, int K, int njm, int h, int w, int Cs, int pad, float temperature, float* value,
                    float* jacobian, float* heatmap, float* stats, float* workspace, size_t workspace_floats, void* stream_) {
    OP_ENTRY(!logits || !value || B < 1 || B > 65535 || K < 1 || (njm != 0 && njm != 1 && njm != K) || h < 1 || w < 1 ||
                     Cs < K + 4 * njm || pad < 0 || pad > 3 || h - 6 + 2 * pad < 1 || w - 6 + 2 * pad < 1 || !(temperature > 0.f) ||
                     !op_workspace_ok(workspace, workspace_floats, eamm_op_kp_head_workspace_floats(B, K), false),
                 "eamm_op_kp_head: bad argument (njm 0 | 1 | K, Cs >= K + 4 njm, a window of at least 1 x 1, workspace of "
                 "eamm_op_kp_head_workspace_floats)");
    hipError_t e = kp_head_launch(logits, B, K, njm, h, w, Cs, pad, temperature, value, njm > 0 ? jacobian : nullptr, heatmap, s, workspace, stats);
    OP_DONE(e, "eamm_op_kp_head");
}

int eamm_op_kp_head_backward(int device, const float* logits, const float* stats, const float* value, const float* jacobian,
                             const float* g_value, const float* g_jacobian, const float* g_heatmap, int B, int K, int njm, int h, int w, int Cs,
                             int pad, float temperature, float* grad_logits, float* workspace, size_t workspace_floats, void* stream_) {
    OP_ENTRY(!logits || !stats || !value || !grad_logits || B < 1 || B > 65535 || K < 1 || (njm != 0 && njm != 1 && njm != K) ||
                     h < 1 || w < 1 || Cs < K + 4 * njm || (Cs & 3) || pad < 0 || pad > 3 || h - 6 + 2 * pad < 1 || w - 6 + 2 * pad < 1 ||
                     !(temperature > 0.f) || (njm > 0 && g_jacobian && !jacobian) || (long long)B * h * w * Cs >= (1ll << 31) ||
                     !op_aligned16(logits) || !op_aligned16(grad_logits) ||
                     !op_workspace_ok(workspace, workspace_floats, eamm_op_kp_head_workspace_floats(B, K), false),
                 "eamm_op_kp_head_backward: bad argument (njm 0 | 1 | K, Cs a multiple of 4 and >= K + 4 njm, 16-byte aligned tensors of "
                 "fewer than 2^31 floats, workspace of eamm_op_kp_head_workspace_floats)");
    hipError_t e = kp_head_backward_launch(logits, stats, value, jacobian, g_value, g_jacobian, g_heatmap, B, K, njm, h, w, Cs, pad, temperature,
                                           grad_logits, workspace, s);
    OP_DONE(e, "eamm_op_kp_head_backward");
}

// ---- Emotion_k's stem max-pool and `final` Conv1d stack as differentiable operators (emotion.hip, emotion_backward.hip) ----------------
int eamm_op_emo_maxpool(int device, const float* x, int B, int H, int W, int C, float* out, void* stream_) {
    OP_ENTRY(!x || !out || B < 1 || H < 2 || W < 2 || (H & 1) || (W & 1) || C < 1 || (long long)B * H * W * C >= (1ll << 31),
             "eamm_op_emo_maxpool: bad argument (H and W even, fewer than 2^31 elements)");
    OP_DONE(emo_maxpool_launch(x, B, H, W, C, out, s), "eamm_op_emo_maxpool");
}

int eamm_op_emo_maxpool_backward(int device, const float* x, const float* grad_out, int B, int H, int W, int C, float* grad_x, void* stream_) {
    OP_ENTRY(!x || !grad_out || !grad_x || B < 1 || H < 2 || W < 2 || (H & 1) || (W & 1) || C < 1 || (long long)B * H * W * C >= (1ll << 31),
             "eamm_op_emo_maxpool_backward: bad argument (H and W even, fewer than 2^31 elements)");
    OP_DONE(emo_maxpool_backward_launch(x, grad_out, B, H, W, C, grad_x, s), "eamm_op_emo_maxpool_backward");
}

int eamm_op_emo_final(int device, const float* a, const float* w98, int B, float* value, float* jacobian, void* stream_) {
    OP_ENTRY(!a || !w98 || (!value && !jacobian) || B < 1, "eamm_op_emo_final: bad argument");
    OP_DONE(emo_final_launch(a, w98, B, value, jacobian, s), "eamm_op_emo_final");
}

size_t eamm_op_emo_final_workspace_floats(int B) { return B < 1 ? 0 : emo_final_backward_workspace_floats(B); }

int eamm_op_emo_final_backward(int device, const float* a, const float* w98, const float* g_value, const float* g_jacobian, int B,
                               float* grad_a, float* grad_w98, float* workspace, size_t workspace_floats, void* stream_) {
    OP_ENTRY(!a || !w98 || !grad_a || !grad_w98 || B < 1 ||
                 !op_workspace_ok(workspace, workspace_floats, emo_final_backward_workspace_floats(B), false),
             "eamm_op_emo_final_backward: bad argument (workspace of eamm_op_emo_final_workspace_floats)");
    OP_DONE(emo_final_backward_launch(a, w98, g_value, g_jacobian, B, grad_a, grad_w98, workspace, s), "eamm_op_emo_final_backward");
}

// ---- AT_net2's LSTM layer and max-pools as differentiable operators (audio.hip, lstm_backward.hip, audio_backward.hip) ----------------
size_t eamm_op_lstm_workspace_floats(int N, int T) { return lstm_op_shape_ok(N, T) ? LSTM_OP_PACKED + LSTM_OP_STATE + LSTM_OP_GRAN_F : 0; }

int eamm_op_lstm_forward(int device, const float* xproj, const float* w_hh, int N, int T, float* y, float* workspace, size_t workspace_floats,
                         void* stream_) {
    OP_ENTRY(!xproj || !w_hh || !y || !lstm_op_shape_ok(N, T) ||
                 !op_workspace_ok(workspace, workspace_floats, eamm_op_lstm_workspace_floats(N, T), true),
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
    OP_DONE(lstm_scan_launch(gates, N, T, c, s), "eamm_op_lstm_scan");
}

size_t eamm_op_lstm_backward_workspace_floats(int N, int T) { return lstm_op_shape_ok(N, T) ? LSTM_OP_GRAN_B : 0; }

int eamm_op_lstm_backward(int device, const float* acts, const float* c, const float* w_hh, const float* grad_y, int N, int T,
                          float* grad_xproj, float* workspace, size_t workspace_floats, void* stream_) {
    OP_ENTRY(!acts || !c || !w_hh || !grad_y || !grad_xproj || !lstm_op_shape_ok(N, T) ||
                 !op_workspace_ok(workspace, workspace_floats, eamm_op_lstm_backward_workspace_floats(N, T), true),
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
    OP_DONE(audio_maxpool_launch(x, B, H, W, C, sy, sx, out, s), "eamm_op_audio_maxpool");
}

int eamm_op_audio_maxpool_backward(int device, const float* x, const float* grad_out, int B, int H, int W, int C, int sy, int sx,
                                   float* grad_x, void* stream_) {
    OP_ENTRY(!x || !grad_out || !grad_x || B < 1 || H < 3 || W < 3 || C < 4 || C % 4 || sy < 1 || sy > 2 || sx < 1 || sx > 2 ||
                 (long long)B * H * W * C >= (1ll << 31),
             "eamm_op_audio_maxpool_backward: bad argument (map sides >= 3, strides 1 | 2, C a multiple of 4, fewer than 2^31 elements)");
    OP_DONE(audio_maxpool_backward_launch(x, grad_out, B, H, W, C, sy, sx, grad_x, s), "eamm_op_audio_maxpool_backward");
}

}  // extern "C"
