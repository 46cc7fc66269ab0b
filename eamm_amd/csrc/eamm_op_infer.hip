// The operator entries of the inference path: the clip preprocessing (One-Euro filter, MFCC front end, the emotion video's resize,
// alignment and augmentation) and the frozen path's small kernels.
#include "op_common.h"

extern "C" {

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
    OP_DONE(resize_aa_launch(in, n, H, W, C, t, out, s), "eamm_op_resize_aa");
}

int eamm_op_similarity_warp(int device, const uint8_t* in, int n, int H, int W, int C, const double* maps, int mode, void* out,
                            void* stream_) {
    OP_ENTRY(!in || !out || !maps || n < 1 || n > 65535 || H < 1 || W < 1 || H > 8192 || W > 8192 || (C != 3 && C != 4) ||
                 (mode != 0 && mode != 1),
             "eamm_op_similarity_warp: bad argument (1 <= n <= 65535, sides 1..8192, C = 3 | 4, mode 0 | 1)");
    OP_DONE(similarity_warp_launch(in, n, H, W, C, maps, mode, out, s), "eamm_op_similarity_warp");
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
    OP_DONE(emotion_augment_launch(aligned, n_src, t0, count, hinv, noise, p, out, s), "eamm_op_emotion_augment");
}

// ---- the frozen inference path's small kernels, one launch each (conv_first.hip, motion.hip, warp.hip, conv_col7.hip, emotion.hip, audio.hip): what the engines
// call per frame or once per clip, on the caller's buffers.  Nothing here but the argument checks and the engines' own *_launch calls.

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
    OP_DONE(first7_launch(source, w, b, ns, H, W, Cout, out, s), "eamm_op_first7");
}

int eamm_op_motion_head_infer(int device, const float* logits, const float* records, int n, int K, int h, int w, int has_occ,
                              float* deformation, float* occlusion, float* mask_out, float* occ_out, void* stream_) {
    OP_ENTRY(!logits || !records || !deformation || n < 1 || n > OP_GRID_YZ || K < 1 || K > 30 || h < 2 || w < 2 || !op_count_ok(n, h, w, 32) ||
                 (has_occ != 0 && has_occ != 1) || (has_occ && !occlusion) || !op_aligned16(logits) || (reinterpret_cast<uintptr_t>(deformation) & 7),
             "eamm_op_motion_head_infer: bad argument (1 <= K <= 30, h and w >= 2, n <= 65535, occlusion where has_occ)");
    OP_DONE(motion_head_launch(logits, records, n, K, h, w, has_occ, deformation, occlusion, mask_out, occ_out, s), "eamm_op_motion_head_infer");
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
    OP_DONE(final_shift_sum_launch(part, bias, n, H, W, out, s), "eamm_op_final_shift_sum");
}

int eamm_op_to_u8(int device, const float* prediction, int n, int H, int W, uint8_t* out, void* stream_) {
    OP_ENTRY(!prediction || !out || !op_count_ok(n, H, W, 3), "eamm_op_to_u8: bad argument");
    OP_DONE(to_u8_launch(prediction, n, H, W, out, s), "eamm_op_to_u8");
}

int eamm_op_warp_image(int device, const float* source, const float* deformation, int n, int ns, int H, int W, int h, int w, int src_planes,
                       int channels, float* out, void* stream_) {
    OP_ENTRY(!source || !deformation || !out || n < 1 || (ns != 1 && ns != n) || channels < 1 || channels > src_planes ||
                 !op_count_ok(n, H, W, src_planes) || !op_count_ok(n, h, w, 2) || (reinterpret_cast<uintptr_t>(deformation) & 7),
             "eamm_op_warp_image: bad argument (ns 1 | n, 1 <= channels <= src_planes)");
    OP_DONE(warp_image_launch(source, deformation, n, ns, H, W, h, w, out, s, src_planes, channels), "eamm_op_warp_image");
}

int eamm_op_source_prepare(int device, const float* source, const float* aa_weight, int ns, int H, int W, int inv_scale, int Cpad,
                           float* source_nhwc, float* small, void* stream_) {
    OP_ENTRY(!source || !source_nhwc || !small || (inv_scale != 1 && inv_scale != 2 && inv_scale != 4) || (inv_scale != 1 && !aa_weight) ||
                 Cpad < 4 || (Cpad & 3) || !op_count_ok(ns, H, W, Cpad) || H % inv_scale || W % inv_scale || !op_aligned16(source_nhwc) ||
                 !op_aligned16(small),
             "eamm_op_source_prepare: bad argument (inv_scale 1 | 2 | 4 dividing H and W, Cpad a multiple of 4)");
    OP_DONE(source_prepare_launch(source, aa_weight, ns, H, W, inv_scale, Cpad, source_nhwc, small, s), "eamm_op_source_prepare");
}

int eamm_op_broadcast_features(int device, const float* feat, int n, int ns, int hf, int wf, int C, float* out, float* out2, const float* scale,
                               const float* shift, void* stream_) {
    OP_ENTRY(!feat || !out || n < 1 || (ns != 1 && ns != n) || C < 4 || (C & 3) || !op_count_ok(n, hf, wf, C) || (out2 && (!scale || !shift)) ||
                 !op_aligned16(feat) || !op_aligned16(out) || !op_aligned16(out2) || !op_aligned16(scale) || !op_aligned16(shift),
             "eamm_op_broadcast_features: bad argument (ns 1 | n, C a multiple of 4, scale and shift where out2, 16-byte aligned)");
    OP_DONE(broadcast_features_launch(feat, n, ns, hf, wf, C, out, out2, scale, shift, s), "eamm_op_broadcast_features");
}

int eamm_op_nchw_to_nhwc_pad(int device, const float* src, int B, int C, int planes, int H, int W, int Cpad, float* dst, void* stream_) {
    OP_ENTRY(!src || !dst || C < 1 || planes < C || Cpad < C || !op_count_ok(B, H, W, Cpad) || !op_count_ok(B, H, W, planes),
             "eamm_op_nchw_to_nhwc_pad: bad argument (1 <= C <= planes, C <= Cpad)");
    OP_DONE(nchw_to_nhwc_pad_launch(src, B, C, H, W, Cpad, dst, s, planes), "eamm_op_nchw_to_nhwc_pad");
}

int eamm_op_emo_avgpool(int device, const float* x, int B, int P, int C, float* out, void* stream_) {
    OP_ENTRY(!x || !out || !op_count_ok(B, P, C), "eamm_op_emo_avgpool: bad argument");
    OP_DONE(emo_avgpool_launch(x, B, P, C, out, s), "eamm_op_emo_avgpool");
}

int eamm_op_emo_embed(int device, const float* value, const float* jacobian, int B, float* out, void* stream_) {
    OP_ENTRY(!value || !jacobian || !out || !op_count_ok(B, 1260), "eamm_op_emo_embed: bad argument");
    OP_DONE(emo_embed_launch(value, jacobian, B, out, s), "eamm_op_emo_embed");
}

int eamm_op_emo_linear(int device, const float* x0, int K0, const float* x1, int K1, const float* wt, const float* bias, int O, int B, int relu,
                       float* out, void* stream_) {
    OP_ENTRY(!x0 || !wt || !bias || !out || K0 < 1 || K1 < 0 || (K1 > 0 && !x1) || K0 > 2048 || K1 > 2048 || K0 + K1 > 2048 || B < 1 ||
                 B > 8 * OP_GRID_YZ || !op_count_ok(K0 + K1, O) || !op_count_ok(B, O) || (relu != 0 && relu != 1),
             "eamm_op_emo_linear: bad argument (K0 >= 1, K1 >= 0 with x1 where K1 > 0, K0 + K1 <= 2048)");
    OP_DONE(emo_linear_launch(x0, K0, x1, K1, wt, bias, O, B, relu, out, s), "eamm_op_emo_linear");
}

int eamm_op_audio_conv1(int device, const float* x, const float* w, const float* b, int F, int H, int W, float* out, void* stream_) {
    OP_ENTRY(!x || !w || !b || !out || !op_count_ok(F, H, W, 64), "eamm_op_audio_conv1: bad argument");
    OP_DONE(audio_conv1_launch(x, w, b, F, H, W, out, s), "eamm_op_audio_conv1");
}

int eamm_op_audio_scale(int device, float* x, size_t n, float scale, void* stream_) {
    OP_ENTRY(!x || n < 1 || n > ((size_t)1 << 39), "eamm_op_audio_scale: bad argument (1 <= n <= 2^39)");
    OP_DONE(audio_scale_launch(x, n, scale, s), "eamm_op_audio_scale");
}

}  // extern "C"
